import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
"""Time the Dreamer-V1 Normal latent and its KL, forward plus backward: the
torch chains of compute_stochastic_state / td.kl_divergence against
ops.gaussian_state / ops.normal_kl, eager and inside a hipGraph of 16 calls.
Cases: the latent at [50, 60] bf16 with statistics (one observe step) and at
[2500, 60] bf16 without (one imagination step), the KL mean at [2500, 30]
fp32.  The variants alternate within each repeat; the spread over repeats is
printed with the median."""
import statistics
import torch
import torch.distributions as td
import torch.nn.functional as F
from sheeprl_amd import ops

CALLS, ITERS, REPS = 16, 200, 7
MIN_STD = 0.1


def state_torch(pre, want_stats):
    mean, std = torch.chunk(pre.float(), 2, -1)
    std = F.softplus(std) + MIN_STD
    sample = td.Independent(td.Normal(mean, std), 1).rsample().to(pre.dtype)
    return (sample, mean, std) if want_stats else (sample,)


def state_fused(pre, want_stats):
    eps = torch.randn(*pre.shape[:-1], pre.shape[-1] // 2, dtype=torch.float32, device=pre.device)
    return [t for t in ops.gaussian_state(pre, eps, MIN_STD, want_stats) if t is not None]


def kl_torch(pm, ps, qm, qs):
    return td.kl_divergence(td.Independent(td.Normal(pm, ps), 1), td.Independent(td.Normal(qm, qs), 1)).mean()


def kl_fused(pm, ps, qm, qs):
    return ops.normal_kl(pm, ps, qm, qs).mean()


def state_case(N, want_stats):
    pre = (3 * torch.randn(N, 60, device="cuda")).to(torch.bfloat16).requires_grad_()
    cot = [torch.randn(N, 30, device="cuda").to(torch.bfloat16)] + [torch.randn(N, 30, device="cuda")] * 2
    cot = cot if want_stats else cot[:1]
    return {
        name: (lambda fn=fn: torch.autograd.grad(fn(pre, want_stats), pre, cot))
        for name, fn in (("torch", state_torch), ("fused", state_fused))
    }


def kl_case(N):
    pm, qm = (torch.randn(N, 30, device="cuda").requires_grad_() for _ in range(2))
    ps, qs = ((0.1 + F.softplus(torch.randn(N, 30, device="cuda"))).requires_grad_() for _ in range(2))
    args = (pm, ps, qm, qs)
    return {
        name: (lambda fn=fn: torch.autograd.grad(fn(*args), args))
        for name, fn in (("torch", kl_torch), ("fused", kl_fused))
    }


def timed(fn):
    t0, t1 = torch.cuda.Event(True), torch.cuda.Event(True)
    t0.record()
    for _ in range(ITERS):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / (ITERS * CALLS) * 1000


torch.manual_seed(0)
CASES = (
    ("state [50, 60] bf16 stats", state_case(50, True)),
    ("state [2500, 60] bf16 sample only", state_case(2500, False)),
    ("kl.mean [2500, 30] fp32", kl_case(2500)),
)
for label, variants in CASES:
    runs = {}
    for name, call in variants.items():

        def step(call=call):
            for _ in range(CALLS):
                call()

        for _ in range(3):
            step()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            step()
        torch.cuda.current_stream().wait_stream(s)
        with torch.cuda.graph(g):
            step()
        for _ in range(5):
            g.replay()
        torch.cuda.synchronize()
        runs[name, "eager"] = step
        runs[name, "graph"] = g.replay
    times = {k: [] for k in runs}
    for _ in range(REPS):
        for k, fn in runs.items():
            times[k].append(timed(fn))
    for (name, how), ts in times.items():
        print(f"{label}: {name:5s} {how:5s}: median {statistics.median(ts):7.2f} us/call fwd+bwd "
              f"(min {min(ts):.2f}, max {max(ts):.2f}, {REPS} repeats)")
