"""MultiDiscrete (ragged-head) DreamerV3 behaviour path on the GPU: the ragged
categorical straight-through kernels against the per-head ``cat_st`` kernels
(bit-identical by construction), the multi-head fast rollout and loss against
the module loop, and the DV3 / P2E-DV3 CLI runs on ``dummy_multidiscrete``."""

import os

import pytest
import torch

requires_gpu = pytest.mark.gpu

if torch.cuda.is_available():
    from sheeprl_amd import ops
    from sheeprl_amd.ops._ext import require_ext

# short head, width-1 head, exactly one wave, one past a wave, three-trip loop
SIZES = [3, 1, 64, 65, 130]
ROWS = 5  # not a multiple of the 4 waves per block: tail waves exist
UNIMIX = 0.01


@pytest.fixture(scope="module", autouse=True)
def _check_env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sheeprl_amd.ops import has_ext

    assert has_ext(), "HIP extension _sheep_hip not built — GPU path would silently degrade"


def _segments(sizes):
    off = 0
    for k in sizes:
        yield off, k
        off += k


def _inputs(dtype, seed):
    torch.manual_seed(seed)
    A = sum(SIZES)
    raw = (torch.randn(ROWS, A, device="cuda") * 2).to(dtype)
    urand = torch.rand(ROWS, A, device="cuda")
    return raw, urand


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("sample", [True, False])
def test_ragged_fwd_bit_identical_to_per_head(dtype, sample):
    ext = require_ext()
    raw, urand = _inputs(dtype, 0)
    m, onehot, s = ext.cat_st_ragged_fwd(raw, urand if sample else None, SIZES, UNIMIX, sample)
    assert m.dtype == torch.float32 and s.dtype == torch.float32 and onehot.dtype == dtype
    for off, k in _segments(SIZES):
        u = urand[:, off : off + k].contiguous() if sample else None
        m_h, oh_h, s_h = ext.cat_st_fwd(raw[:, off : off + k].contiguous(), u, UNIMIX, sample)
        assert torch.equal(m[:, off : off + k], m_h), (off, k)
        assert torch.equal(s[:, off : off + k], s_h), (off, k)
        assert torch.equal(onehot[:, off : off + k], oh_h), (off, k)
    assert torch.equal(onehot.float().sum(-1), torch.full((ROWS,), float(len(SIZES)), device="cuda"))


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ragged_fwd_o_strided_destinations(dtype):
    ext = require_ext()
    raw, urand = _inputs(dtype, 1)
    A = sum(SIZES)
    m_ref, oh_ref, s_ref = ext.cat_st_ragged_fwd(raw, urand, SIZES, UNIMIX, True)

    m = torch.empty(ROWS, A, device="cuda")
    s = torch.empty(ROWS, A, device="cuda")
    onehot = torch.full((ROWS, A), 7.0, device="cuda", dtype=dtype)
    off, sentinel = 11, -3.0
    wide = torch.full((ROWS, off + A + 9), sentinel, device="cuda", dtype=dtype)
    ext.cat_st_ragged_fwd_o(raw, urand, SIZES, UNIMIX, True, m, s, onehot, wide[:, off : off + A])
    assert torch.equal(m, m_ref) and torch.equal(s, s_ref)
    assert torch.equal(onehot, oh_ref)
    assert torch.equal(wide[:, off : off + A], oh_ref)
    assert (wide[:, :off] == sentinel).all() and (wide[:, off + A :] == sentinel).all()

    # log-probs only: no one-hot destination, nothing else written
    m2 = torch.empty_like(m)
    s2 = torch.empty_like(s)
    ext.cat_st_ragged_fwd_o(raw, None, SIZES, UNIMIX, False, m2, s2)
    assert torch.equal(m2, m_ref) and torch.equal(s2, s_ref)


@requires_gpu
def test_ragged_host_checks():
    ext = require_ext()
    raw, urand = _inputs(torch.float32, 2)
    with pytest.raises(RuntimeError):
        ext.cat_st_ragged_fwd(raw, urand, SIZES[:-1], UNIMIX, True)  # sum(sizes) != A
    with pytest.raises(RuntimeError):
        ext.cat_st_ragged_fwd(raw, urand, [0] + SIZES, UNIMIX, True)  # empty head
    with pytest.raises(RuntimeError):
        ext.cat_st_ragged_fwd(raw[:, :9].contiguous(), urand[:, :9].contiguous(), [1] * 9, UNIMIX, True)  # > 8 heads
    with pytest.raises(RuntimeError):
        ext.cat_st_ragged_fwd(raw, urand.double(), SIZES, UNIMIX, True)  # urand dtype


@requires_gpu
def test_ragged_op_more_heads_than_one_launch():
    """ops.categorical_st_ragged beyond the one-launch head limit: runs of
    MAX_RAGGED_HEADS heads, still bit-identical to the per-head kernels."""
    ext = require_ext()
    assert ext.MAX_RAGGED_HEADS == ops.MAX_RAGGED_HEADS
    torch.manual_seed(6)
    sizes = [2, 3, 1, 4, 2, 5, 3, 2, 4, 1, 3]  # 11 heads: runs of 8 + 3
    A = sum(sizes)
    raw = torch.randn(ROWS, A, device="cuda", requires_grad=True)
    urand = torch.rand(ROWS, A, device="cuda")
    gm = torch.randn(ROWS, A, device="cuda")
    m, onehot = ops.categorical_st_ragged(raw, sizes, unimix=UNIMIX, sample=True, urand=urand)
    (m * gm).sum().backward()
    for off, k in _segments(sizes):
        m_h, oh_h, s_h = ext.cat_st_fwd(raw.detach()[:, off : off + k].contiguous(),
                                        urand[:, off : off + k].contiguous(), UNIMIX, True)
        assert torch.equal(m[:, off : off + k], m_h), (off, k)
        assert torch.equal(onehot[:, off : off + k], oh_h), (off, k)
        g_h = ext.cat_st_bwd(gm[:, off : off + k].contiguous(), torch.zeros_like(oh_h), s_h, UNIMIX)
        assert torch.equal(raw.grad[:, off : off + k], g_h), (off, k)


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ragged_bwd_bit_identical_to_per_head(dtype):
    ext = require_ext()
    raw, urand = _inputs(dtype, 3)
    A = sum(SIZES)
    _, _, s = ext.cat_st_ragged_fwd(raw, urand, SIZES, UNIMIX, True)
    gm = torch.randn(ROWS, A, device="cuda")
    gon = torch.randn(ROWS, A, device="cuda").to(dtype)
    graw = ext.cat_st_ragged_bwd(gm, gon, s, SIZES, UNIMIX)
    assert graw.dtype == dtype
    for off, k in _segments(SIZES):
        ref = ext.cat_st_bwd(gm[:, off : off + k].contiguous(), gon[:, off : off + k].contiguous(),
                             s[:, off : off + k].contiguous(), UNIMIX)
        assert torch.equal(graw[:, off : off + k], ref), (off, k)
    # gon absent == gon of zeros
    g_none = ext.cat_st_ragged_bwd(gm, None, s, SIZES, UNIMIX, dtype)
    g_zero = ext.cat_st_ragged_bwd(gm, torch.zeros_like(gon), s, SIZES, UNIMIX)
    assert g_none.dtype == dtype
    assert torch.equal(g_none, g_zero)


@requires_gpu
def test_ragged_autograd_matches_eager():
    torch.manual_seed(4)
    A = sum(SIZES)
    raw = torch.randn(ROWS, 3, A, device="cuda")
    gm = torch.randn(ROWS, 3, A, device="cuda")
    raw_g = raw.clone().requires_grad_()
    m, _ = ops.categorical_st_ragged(raw_g, SIZES, unimix=UNIMIX, sample=False)
    (m * gm).sum().backward()
    raw_e = raw.clone().requires_grad_()
    m_ref = torch.cat(
        [
            torch.log((1 - UNIMIX) * torch.softmax(raw_e[..., off : off + k], -1) + UNIMIX / k)
            for off, k in _segments(SIZES)
        ],
        -1,
    )
    (m_ref * gm).sum().backward()
    # the fp32 bound of test_gpu_kernels.test_categorical_st_gpu
    assert torch.allclose(m, m_ref, atol=1e-4, rtol=1e-4), (m - m_ref).abs().max()
    assert torch.allclose(raw_g.grad, raw_e.grad, atol=1e-4, rtol=1e-4), (raw_g.grad - raw_e.grad).abs().max()


@requires_gpu
@pytest.mark.timeout(600)
def test_fast_imagination_multidiscrete_matches_module_loop():
    """imagine_rollout with three action heads vs the module-based loop given
    the same uniforms (fp32)."""
    from sheeprl_amd.algos.dreamer_v3.agent import RSSM, Actor, RecurrentModel
    from sheeprl_amd.algos.dreamer_v3.imagine import imagine_applicable, imagine_rollout
    from sheeprl_amd.models import MLP

    dims = [3, 5, 2]
    B, A, H, S, K, DU, P, HZ = 7, sum(dims), 16, 4, 4, 16, 20, 6
    SK = S * K
    torch.manual_seed(3)
    rssm = RSSM(
        RecurrentModel(SK + A, H, DU),
        MLP(24 + H, SK, [P], activation="silu", layer_norm=True, layer_norm_eps=1e-3),
        MLP(H, SK, [P], activation="silu", layer_norm=True, layer_norm_eps=1e-3),
        discrete=K,
        unimix=0.01,
    ).cuda()
    actor = Actor(SK + H, dims, False, dense_units=DU, mlp_layers=2, unimix=0.01).cuda()
    assert imagine_applicable(rssm, actor)

    z0 = torch.rand(B, SK, device="cuda")
    h0 = torch.randn(B, H, device="cuda")

    # module-loop reference (same structure as dreamer_v3.train's fallback)
    torch.manual_seed(11)
    with torch.no_grad():
        prior = z0.view(1, B, SK)
        rec = h0.view(1, B, H)
        latent = torch.cat((prior, rec), -1)
        traj_ref = [latent[0]]
        act = torch.cat(actor(latent)[0], dim=-1)
        acts_ref = [act[0]]
        for i in range(1, HZ + 1):
            prior, rec = rssm.imagination(prior, rec, act)
            prior = prior.view(1, B, SK)
            latent = torch.cat((prior, rec), -1)
            traj_ref.append(latent[0])
            act = torch.cat(actor(latent)[0], dim=-1)
            acts_ref.append(act[0])
    traj_ref = torch.stack(traj_ref)
    acts_ref = torch.stack(acts_ref)

    # replicate the module loop's philox consumption order: per step, one
    # torch.rand(1, B, K_h) per head in head order
    def head_draws():
        return torch.cat([torch.rand(1, B, k, device="cuda")[0] for k in dims], -1)

    torch.manual_seed(11)
    ua, ut = [head_draws()], []
    for i in range(HZ):
        ut.append(torch.rand(B, S, K, device="cuda"))
        ua.append(head_draws())
    traj, acts = imagine_rollout(rssm, actor, z0, h0, HZ, urand_t=torch.stack(ut), urand_a=torch.stack(ua))
    assert acts.shape == (HZ + 1, B, A)
    assert torch.equal(acts, acts_ref)
    assert torch.allclose(traj, traj_ref, atol=1e-4, rtol=1e-4), (traj - traj_ref).abs().max()


@requires_gpu
def test_reinforce_loss_multidiscrete_matches_eager():
    """ops.reinforce_loss on concatenated per-head log-probs / one-hots vs the
    eager multi-head actor loss of dreamer_v3.train's fallback (value and
    gradient with respect to the head logits)."""
    from sheeprl_amd.distributions import LogProbCategorical

    torch.manual_seed(5)
    dims = [3, 5, 2]
    HZ, F, A = 3, 5, sum(dims)
    logits = torch.randn(HZ + 1, F, A, device="cuda")
    acts = torch.cat(
        [
            torch.nn.functional.one_hot(torch.randint(0, k, (HZ + 1, F), device="cuda"), k).float()
            for k in dims
        ],
        -1,
    )
    adv = torch.randn(HZ, F, 1, device="cuda")
    disc = torch.rand(HZ, F, 1, device="cuda")
    ent_coef = 3e-4

    lg = logits.clone().requires_grad_()
    m, _ = ops.categorical_st_ragged(lg, dims, unimix=UNIMIX, sample=False)
    loss = ops.reinforce_loss(m, acts, adv, disc, ent_coef)
    loss.backward()

    le = logits.clone().requires_grad_()
    policies = [
        LogProbCategorical(torch.log((1 - UNIMIX) * torch.softmax(le[..., off : off + k], -1) + UNIMIX / k))
        for off, k in _segments(dims)
    ]
    objective = (
        torch.stack(
            [
                p.log_prob(a.detach().float()).unsqueeze(-1)[:-1]
                for p, a in zip(policies, torch.split(acts, dims, dim=-1))
            ],
            dim=-1,
        ).sum(dim=-1)
        * adv
    )
    entropy = ent_coef * torch.stack([p.entropy() for p in policies], -1).sum(dim=-1)
    ref_loss = -torch.mean(disc * (objective + entropy.unsqueeze(dim=-1)[:-1]))
    ref_loss.backward()

    # bounds of test_gpu_kernels.test_fused_behaviour_losses_match_eager
    assert torch.allclose(loss, ref_loss, atol=1e-5, rtol=1e-5), (loss, ref_loss)
    assert torch.allclose(lg.grad, le.grad, atol=1e-6), (lg.grad - le.grad).abs().max()


# ---------------------------------------------------------------------------
# end-to-end: the CLI runs on a MultiDiscrete env must take the fast rollout
# ---------------------------------------------------------------------------

TINY_DV = [
    "algo.dense_units=8",
    "algo.mlp_layers=1",
    "algo.world_model.encoder.cnn_channels_multiplier=2",
    "algo.world_model.recurrent_model.recurrent_state_size=8",
    "algo.world_model.transition_model.hidden_size=8",
    "algo.world_model.representation_model.hidden_size=8",
    "algo.world_model.discrete_size=4",
    "algo.world_model.stochastic_size=4",
    "algo.per_rank_batch_size=2",
    "algo.per_rank_sequence_length=4",
    "algo.horizon=3",
    "algo.total_steps=16",
    "algo.learning_starts=4",
    "algo.replay_ratio=0.5",
    "buffer.size=64",
    "algo.run_test=False",
]


def _run_multidiscrete(tmp_path, monkeypatch, module, extra):
    from sheeprl_amd.cli import run

    head_counts = []
    real = module.imagine_rollout

    def counting(rssm, actor, *args, **kwargs):
        head_counts.append(len(actor.mlp_heads))
        return real(rssm, actor, *args, **kwargs)

    monkeypatch.setattr(module, "imagine_rollout", counting)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        run(
            [
                "env=dummy",
                "runtime.accelerator=cuda",
                "runtime.precision=bf16",
                "runtime.devices=1",
                "checkpoint.every=0",
                "checkpoint.save_last=False",
                "metric.log_every=1",
                "env.num_envs=2",
                "seed=0",
                "dry_run=False",
                "algo.mlp_keys.encoder=[state]",
                *extra,
                "env.id=dummy_multidiscrete",
                *TINY_DV,
            ]
        )
    finally:
        os.chdir(cwd)
    return head_counts


def _assert_fast_rollout_ran(head_counts):
    assert head_counts, "the fast imagination rollout never ran"
    assert all(n > 1 for n in head_counts), head_counts


@requires_gpu
@pytest.mark.timeout(300)
def test_gpu_dreamer_v3_multidiscrete_bf16(tmp_path, monkeypatch):
    from sheeprl_amd.algos.dreamer_v3 import dreamer_v3

    _assert_fast_rollout_ran(_run_multidiscrete(tmp_path, monkeypatch, dreamer_v3, ["exp=dreamer_v3"]))


@requires_gpu
@pytest.mark.timeout(300)
def test_gpu_dreamer_v3_nine_heads_keeps_module_loop(tmp_path, monkeypatch):
    """More heads than one ragged launch takes: the run must train through the
    module loop as before, not enter the fast path."""
    from sheeprl_amd.algos.dreamer_v3 import dreamer_v3

    dims = ",".join(["2"] * (ops.MAX_RAGGED_HEADS + 1))
    head_counts = _run_multidiscrete(
        tmp_path, monkeypatch, dreamer_v3, ["exp=dreamer_v3", f"env.wrapper_kwargs.action_dims=[{dims}]"]
    )
    assert head_counts == []


@requires_gpu
@pytest.mark.timeout(300)
def test_gpu_p2e_dv3_multidiscrete_bf16(tmp_path, monkeypatch):
    from sheeprl_amd.algos.p2e_dv3 import p2e_dv3_exploration

    _assert_fast_rollout_ran(_run_multidiscrete(
        tmp_path, monkeypatch, p2e_dv3_exploration,
        ["exp=p2e_dv3_exploration", "algo.ensembles.n=2", "algo.ensembles.dense_units=8",
         "algo.ensembles.mlp_layers=1"],
    ))
