"""ops.gaussian_state (kernels gauss_state_fwd / gauss_state_bwd) and
ops.normal_kl (normal_kl_fwd / normal_kl_bwd) against their formulas in fp64,
and their wiring into the Dreamer-V1 RSSM.

The shapes cover every lane-group width with a partial last group, wave and
block, the DV1 default S = 30, the S = 64 boundary and the S > 64 column loop."""

import itertools

import pytest
import torch
import torch.distributions as td
import torch.nn.functional as F

requires_gpu = pytest.mark.gpu
SHAPES = [(259, 1), (67, 3), (37, 6), (13, 30), (5, 64), (3, 70)]
DTYPES = [torch.float32, torch.bfloat16]
MIN_STD = 0.1
# (N, S, dtype, want_stats, outputs that take a gradient)
STATE_CASES = [(*ns, dt, ws, "all") for ns, dt, ws in itertools.product(SHAPES, DTYPES, [True, False])] + [
    (37, 6, torch.bfloat16, True, "sample"),
    (37, 6, torch.bfloat16, True, "stats"),
]
# (N, S, whether the prior side requires grad)
KL_CASES = [(*ns, True) for ns in SHAPES] + [(37, 6, False)]


@pytest.fixture()
def _gpu_ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sheeprl_amd.ops import has_ext
    assert has_ext(), "HIP extension _sheep_hip not built — GPU path would silently degrade"


def _ref(pre, eps):
    """(sample, mean, std) in fp64 from the rounded pre."""
    a, b = pre.double().chunk(2, -1)
    sd = F.softplus(b) + MIN_STD
    return a + sd * eps.double(), a, sd


def _close(got, want, dtype):
    # the bounds of test_gpu_cont_head.py — fp32: 3e-4; bf16: two ulps of
    # output rounding
    tol = 3e-4 if dtype == torch.float32 else 2.0**-7
    torch.testing.assert_close(got.double(), want.detach(), atol=tol, rtol=tol)


def _inputs(N, S, dtype, device):
    torch.manual_seed(N * 100 + S)
    pre = (3 * torch.randn(N, 2 * S, device=device)).to(dtype).requires_grad_()
    return pre, torch.randn(N, S, device=device)


def _kl_inputs(N, S, device, prior_grad=True):
    torch.manual_seed(N * 100 + S)
    pm, qm = torch.randn(2, N, S, device=device).unbind(0)
    ps, qs = (0.1 + F.softplus(torch.randn(2, N, S, device=device))).unbind(0)
    return [t.clone().requires_grad_(prior_grad or i < 2) for i, t in enumerate((pm, ps, qm, qs))]


def _check_state(pre, eps, dtype, want_stats, grads):
    from sheeprl_amd import ops

    N, S = eps.shape
    cot = [torch.randn(N, S, device=pre.device) for _ in range(3)]
    cot[0] = cot[0].to(dtype)
    use = [grads != "stats", want_stats and grads != "sample", want_stats and grads != "sample"]
    pre64 = pre.detach().double().requires_grad_()
    want = _ref(pre64, eps)
    sum((w * c.double()).sum() for w, c, u in zip(want, cot, use) if u).backward()

    got = ops.gaussian_state(pre, eps, MIN_STD, want_stats)
    assert got[0].dtype == dtype and got[0].shape == (N, S)
    _close(got[0], want[0], dtype)
    for g, w in zip(got[1:], want[1:]):
        assert (g is None) == (not want_stats)
        if want_stats:
            assert g.dtype == torch.float32 and g.shape == (N, S)
            _close(g, w, torch.float32)
    sum((g * c).sum() for g, c, u in zip(got, cot, use) if u).backward()
    assert pre.grad.dtype == dtype
    _close(pre.grad, pre64.grad, dtype)


def _check_kl(params):
    from sheeprl_amd import ops

    p64 = [t.detach().double().requires_grad_(t.requires_grad) for t in params]
    g = torch.randn(params[0].shape[0], device=params[0].device)
    want = td.kl_divergence(td.Independent(td.Normal(p64[0], p64[1]), 1), td.Independent(td.Normal(p64[2], p64[3]), 1))
    (want * g.double()).sum().backward()
    kl = ops.normal_kl(*params)
    assert kl.dtype == torch.float32 and kl.shape == want.shape
    _close(kl, want, torch.float32)
    (kl * g).sum().backward()
    for t, t64 in zip(params, p64):
        assert (t.grad is None) == (not t.requires_grad)
        if t.requires_grad:
            _close(t.grad, t64.grad, torch.float32)


@requires_gpu
@pytest.mark.parametrize("N,S,dtype,want_stats,grads", STATE_CASES)
def test_gaussian_state_matches_fp64(_gpu_ext, N, S, dtype, want_stats, grads):
    _check_state(*_inputs(N, S, dtype, "cuda"), dtype, want_stats, grads)


@requires_gpu
@pytest.mark.parametrize("N,S,prior_grad", KL_CASES)
def test_normal_kl_matches_fp64(_gpu_ext, N, S, prior_grad):
    _check_kl(_kl_inputs(N, S, "cuda", prior_grad))


@requires_gpu
@pytest.mark.parametrize("switch", ["1", "0"])
def test_rssm_v1_routes_to_fused_state(_gpu_ext, monkeypatch, switch):
    from sheeprl_amd.algos.dreamer_v1.dreamer_v1 import RSSMV1

    monkeypatch.setenv("SHEEPRL_AMD_GAUSS_STATE", switch)
    S, dt = 30, torch.bfloat16
    torch.manual_seed(0)
    rssm = RSSMV1(torch.nn.Linear(S + 3, 8), torch.nn.Linear(8 + 5, 2 * S), torch.nn.Linear(8, 2 * S), MIN_STD)
    rssm = rssm.cuda().to(dt)
    h, emb = torch.randn(1, 7, 8, device="cuda").to(dt), torch.randn(1, 7, 5, device="cuda").to(dt)
    calls = [
        (lambda: rssm._transition(h), rssm.transition_model(h)),
        (lambda: rssm._representation(h, emb), rssm.representation_model(torch.cat((h, emb), -1))),
    ]
    for call, pre in calls:
        torch.manual_seed(11)
        (mean, std), sample = call()
        assert sample.dtype == dt and mean.dtype == std.dtype == torch.float32
        torch.manual_seed(11)
        if switch == "1":
            eps = torch.randn(1, 7, S, dtype=torch.float32, device="cuda")
            x, a, sd = _ref(pre, eps)
            _close(sample, x, dt)
            _close(mean, a, torch.float32)
            _close(std, sd, torch.float32)
        else:  # the torch chain itself: the same draw gives the same bits
            a, b = torch.chunk(pre.float(), 2, -1)
            sd = F.softplus(b) + MIN_STD
            assert torch.equal(sample, td.Independent(td.Normal(a, sd), 1).rsample().to(dt))
            assert torch.equal(mean, a) and torch.equal(std, sd)
    (mean, std), sample = rssm._transition(h, want_stats=False)
    assert sample.shape == (1, 7, S) and ((mean is None and std is None) == (switch == "1"))


def test_cpu_fallback_matches_fp64():
    _check_state(*_inputs(5, 3, torch.float32, "cpu"), torch.float32, True, "all")
    _check_kl(_kl_inputs(5, 3, "cpu"))
