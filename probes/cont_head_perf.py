import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
"""Time the continuous actor head (sample + clip + entropy, forward plus
backward) at [1024, 2A] bf16: the torch chain of Actor.forward against
ops.continuous_actor_head, eager and inside a hipGraph of 16 heads (one
imagination rollout's worth).  The variants alternate within each repeat;
the spread over repeats is printed with the median."""
import statistics
import torch
import torch.distributions as td
from sheeprl_amd import ops

N, CALLS, ITERS, REPS = 1024, 16, 50, 7
INIT_STD, MIN_STD, MAX_STD, CLIP = 2.0, 0.1, 1.0, 1.0


def torch_chain(pre):
    mean, std = torch.chunk(pre.float(), 2, -1)
    std = (MAX_STD - MIN_STD) * torch.sigmoid(std + INIT_STD) + MIN_STD
    dist = td.Independent(td.Normal(torch.tanh(mean), std), 1)
    actions = dist.rsample()
    clip = torch.full_like(actions, CLIP)
    actions = actions * (clip / torch.maximum(clip, torch.abs(actions))).detach()
    return actions, dist.entropy()


def fused(pre):
    eps = torch.randn(*pre.shape[:-1], pre.shape[-1] // 2, dtype=torch.float32, device=pre.device)
    return ops.continuous_actor_head(pre, eps, "scaled_normal", INIT_STD, MIN_STD, MAX_STD, CLIP)


def timed(fn):
    t0, t1 = torch.cuda.Event(True), torch.cuda.Event(True)
    t0.record()
    for _ in range(ITERS):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / (ITERS * CALLS) * 1000


for A in (1, 6, 21):
    torch.manual_seed(A)
    pre = (3 * torch.randn(N, 2 * A, device="cuda")).to(torch.bfloat16).requires_grad_()
    ge = torch.randn(N, device="cuda")
    runs = {}
    for name, head in (("torch", torch_chain), ("fused", fused)):
        ga = torch.randn(N, A, device="cuda").to(torch.float32 if name == "torch" else torch.bfloat16)

        def step(head=head, ga=ga):
            for _ in range(CALLS):
                actions, entropy = head(pre)
                torch.autograd.grad([actions, entropy], pre, [ga, ge])

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
        print(f"A={A:2d} {name:5s} {how:5s}: median {statistics.median(ts):7.2f} us/head fwd+bwd "
              f"(min {min(ts):.2f}, max {max(ts):.2f}, {REPS} repeats)")
