"""ops.continuous_actor_head (kernels cont_head_fwd / cont_head_bwd) against
the head's formulas in fp64, its routing, and its wiring into Actor.forward.

The shapes cover every lane-group width with a partial last group, wave and
block, the A = 64 boundary and the A > 64 column loop."""

import math

import pytest
import torch
import torch.distributions as td
import torch.nn.functional as F

requires_gpu = pytest.mark.gpu
MODES = ["scaled_normal", "tanh_normal"]
DTYPES = [torch.float32, torch.bfloat16]
INIT_STD, MIN_STD, MAX_STD = 2.0, 0.1, 1.0


@pytest.fixture()
def _gpu_ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sheeprl_amd.ops import has_ext
    assert has_ext(), "HIP extension _sheep_hip not built — GPU path would silently degrade"


def _ref(pre, eps, mode, clip):
    """(unclipped x, actions, entropy or None) in fp64 from the rounded pre."""
    a, b = pre.double().chunk(2, -1)
    e = eps.double()
    if mode == "tanh_normal":
        x, ent = torch.tanh(5 * torch.tanh(a / 5) + (F.softplus(b + INIT_STD) + MIN_STD) * e), None
    else:
        sd = (MAX_STD - MIN_STD) * torch.sigmoid(b + INIT_STD) + MIN_STD
        x = torch.tanh(a) + sd * e
        ent = (0.5 + 0.5 * math.log(2 * math.pi) + sd.log()).sum(-1)
    y = x * (clip / x.abs().clamp(min=clip)).detach() if clip > 0 else x
    return x, y, ent


def _close(got, want, dtype):
    # fp32: the bound test_tanh_normal_fused_matches_eager grants this math;
    # bf16: two ulps of output rounding
    tol = 3e-4 if dtype == torch.float32 else 2.0**-7
    torch.testing.assert_close(got.double(), want, atol=tol, rtol=tol)


def _head(pre, eps, mode, clip):
    from sheeprl_amd import ops
    return ops.continuous_actor_head(pre, eps, mode, INIT_STD, MIN_STD, MAX_STD, clip)


def _inputs(N, A, dtype, device):
    torch.manual_seed(N * 100 + A)
    pre = (3 * torch.randn(N, 2 * A, device=device)).to(dtype).requires_grad_()
    return pre, torch.randn(N, A, device=device)


@requires_gpu
@pytest.mark.parametrize("N,A", [(259, 1), (67, 3), (37, 6), (13, 17), (5, 64), (3, 70)])
@pytest.mark.parametrize("clip", [0.0, 1.0])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_kernel_matches_fp64(_gpu_ext, mode, dtype, clip, N, A):
    pre, eps = _inputs(N, A, dtype, "cuda")
    ga = torch.randn(N, A, device="cuda").to(dtype)
    ge = torch.randn(N, device="cuda")
    pre64 = pre.detach().double().requires_grad_()
    x, y, ent = _ref(pre64, eps, mode, clip)
    if clip > 0:
        assert (x.abs() < clip).any()
        # tanh_normal's x is a tanh: it cannot pass 1, so only the
        # scaled_normal cases reach the rescaling side of the clip
        assert mode == "tanh_normal" or (x.abs() > clip).any()
    loss64 = (y * ga.double()).sum() + ((ent * ge.double()).sum() if ent is not None else 0)
    loss64.backward()

    actions, entropy = _head(pre, eps, mode, clip)
    assert actions.dtype == dtype and actions.shape == (N, A)
    _close(actions, y.detach(), dtype)
    loss = (actions * ga).sum()
    assert (entropy is None) == (mode == "tanh_normal")
    if entropy is not None:
        assert entropy.dtype == torch.float32 and entropy.shape == (N,)
        _close(entropy, ent.detach(), torch.float32)
        loss = loss + (entropy * ge).sum()
    loss.backward()
    assert pre.grad.dtype == dtype
    _close(pre.grad, pre64.grad, dtype)


@requires_gpu
def test_backward_without_entropy_gradient(_gpu_ext):
    N, A = 37, 6
    pre, eps = _inputs(N, A, torch.float32, "cuda")
    ga = torch.randn(N, A, device="cuda")
    pre64 = pre.detach().double().requires_grad_()
    (_ref(pre64, eps, "scaled_normal", 1.0)[1] * ga.double()).sum().backward()
    actions, _ = _head(pre, eps, "scaled_normal", 1.0)
    (actions * ga).sum().backward()
    _close(pre.grad[:, A:], pre64.grad[:, A:], torch.float32)  # std logits: no entropy term
    _close(pre.grad[:, :A], pre64.grad[:, :A], torch.float32)


@requires_gpu
@pytest.mark.parametrize("A,G", [(1, 4), (3, 4), (6, 8), (17, 32), (64, 64), (70, 64)])
def test_route(_gpu_ext, A, G):
    from sheeprl_amd.ops import require_ext
    assert require_ext().cont_head_route(1024, A) == G


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_actor_routes_to_fused_head(_gpu_ext, monkeypatch, mode, dtype):
    from sheeprl_amd.algos.dreamer_v3.agent import Actor
    from sheeprl_amd.distributions import FusedContinuousDist

    monkeypatch.setenv("SHEEPRL_AMD_CONT_HEAD", "1")
    torch.manual_seed(0)
    actor = Actor(12, [3], True, distribution=mode, dense_units=16, mlp_layers=1).cuda().to(dtype)
    state = torch.randn(7, 12, device="cuda").to(dtype)
    torch.manual_seed(11)
    (actions,), (dist,) = actor(state)
    assert isinstance(dist, FusedContinuousDist)
    pre = actor.mlp_heads[0](actor.model(state))
    torch.manual_seed(11)
    eps = torch.randn(7, 3, dtype=torch.float32, device="cuda")
    _, y, ent = _ref(pre.detach(), eps, mode, 1.0)
    _close(actions, y, dtype)
    assert actions.abs().max() <= 1.0
    if mode == "scaled_normal":
        _close(dist.entropy(), ent, torch.float32)
    else:
        with pytest.raises(NotImplementedError):
            dist.entropy()
    # everything else comes from the td distribution of the torch path
    assert dist.log_prob(actions.float()).shape == (7,)

    greedy_actions, greedy_dists = actor(state[:1].view(1, 1, 12), greedy=True)
    assert greedy_actions[0].shape == (1, 1, 3) and isinstance(greedy_dists[0], td.Independent)
    monkeypatch.setenv("SHEEPRL_AMD_CONT_HEAD", "0")
    assert isinstance(actor(state)[1][0], td.Independent)


@pytest.mark.parametrize("mode", MODES)
def test_cpu_fallback_matches_fp64(mode):
    pre, eps = _inputs(5, 3, torch.float32, "cpu")
    pre64 = pre.detach().double().requires_grad_()
    _, y, ent = _ref(pre64, eps, mode, 1.0)
    actions, entropy = _head(pre, eps, mode, 1.0)
    _close(actions, y.detach(), torch.float32)
    assert (entropy is None) == (mode == "tanh_normal")
    if entropy is not None:
        _close(entropy, ent.detach(), torch.float32)
    y.sum().backward()
    actions.sum().backward()
    _close(pre.grad, pre64.grad, torch.float32)
