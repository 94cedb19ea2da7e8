"""cat_st_sample_o, the inference-only sampler of the imagination rollout:
its one-hots must be bit-identical to cat_st_fwd_o's for the same uniforms.

The row counts leave the last wave (64/G rows) and the last block partial at
every group width G the kernel is instantiated for."""

import pytest
import torch

requires_gpu = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _check_env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sheeprl_amd.ops import has_ext

    assert has_ext(), "HIP extension _sheep_hip not built — GPU path would silently degrade"


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,S,K", [(3, 5, 4), (5, 3, 9), (7, 4, 32), (3, 2, 64), (2, 3, 255)])
def test_sample_matches_cat_st_fwd_o(dtype, B, S, K):
    from sheeprl_amd.ops._ext import require_ext

    ext = require_ext()
    torch.manual_seed(B * 1000 + K)
    SK = S * K
    raw = (torch.randn(B, S, K, device="cuda") * 3).to(dtype)
    # exact ties in the logits exercise the lowest-index tie-break as well
    raw[0, 0, :] = raw[0, 0, 0]
    urand = torch.rand(B, S, K, device="cuda")
    urand[0, 0, :] = 0.5
    unimix = 0.01

    m = torch.empty(B, S, K, device="cuda", dtype=torch.float32)
    s = torch.empty(B, S, K, device="cuda", dtype=torch.float32)
    # one-hots into row-strided slices of wider buffers, as the rollout does
    buf_a = torch.full((B, SK + 7), 7.0, device="cuda", dtype=dtype)
    buf_a2 = torch.full((B, 3 + SK), 7.0, device="cuda", dtype=dtype)
    ext.cat_st_fwd_o(raw, urand, unimix, m, buf_a[:, :SK], s, buf_a2[:, 3:])
    buf_b = torch.full((B, SK + 7), 7.0, device="cuda", dtype=dtype)
    buf_b2 = torch.full((B, 3 + SK), 7.0, device="cuda", dtype=dtype)
    ext.cat_st_sample_o(raw, urand, unimix, buf_b[:, :SK], buf_b2[:, 3:])

    # whole buffers: equal one-hots and untouched padding columns
    assert torch.equal(buf_b, buf_a)
    assert torch.equal(buf_b2, buf_a2)
    oh = buf_b[:, :SK].reshape(B, S, K).float()
    assert torch.equal(oh.sum(-1), torch.ones(B, S, device="cuda"))
    assert ((oh == 0) | (oh == 1)).all()
    assert torch.equal(buf_b2[:, 3:], buf_b[:, :SK])
    # the tied row takes the lowest index
    assert oh[0, 0, 0] == 1

    # contiguous one-hot, no second output
    c = torch.empty(B, S, K, device="cuda", dtype=dtype)
    ext.cat_st_sample_o(raw, urand, unimix, c)
    assert torch.equal(c.view(B, SK), buf_a[:, :SK])


@requires_gpu
def test_rollout_same_with_sampler_and_cat_st_fwd_o(monkeypatch):
    """imagine_rollout with fixed uniforms returns identical trajectories and
    actions with the new sampler and with cat_st_fwd_o (bf16)."""
    from sheeprl_amd.algos.dreamer_v3.agent import RSSM, Actor, RecurrentModel
    from sheeprl_amd.algos.dreamer_v3.imagine import imagine_applicable, imagine_rollout
    from sheeprl_amd.models import MLP

    B, A, H, S, K, DU, P, HZ = 7, 5, 16, 4, 4, 16, 20, 6
    SK = S * K
    torch.manual_seed(3)
    rssm = RSSM(
        RecurrentModel(SK + A, H, DU),
        MLP(24 + H, SK, [P], activation="silu", layer_norm=True, layer_norm_eps=1e-3),
        MLP(H, SK, [P], activation="silu", layer_norm=True, layer_norm_eps=1e-3),
        discrete=K,
        unimix=0.01,
    ).cuda().to(torch.bfloat16)
    actor = Actor(SK + H, [A], False, dense_units=DU, mlp_layers=2, unimix=0.01).cuda().to(torch.bfloat16)
    assert imagine_applicable(rssm, actor)

    z0 = torch.rand(B, SK, device="cuda").to(torch.bfloat16)
    h0 = torch.randn(B, H, device="cuda").to(torch.bfloat16)
    urand_t = torch.rand(HZ, B, S, K, device="cuda")
    urand_a = torch.rand(HZ + 1, B, A, device="cuda")

    monkeypatch.setenv("SHEEPRL_AMD_CAT_SAMPLE", "1")
    traj1, acts1 = imagine_rollout(rssm, actor, z0, h0, HZ, urand_t=urand_t, urand_a=urand_a)
    monkeypatch.setenv("SHEEPRL_AMD_CAT_SAMPLE", "0")
    traj0, acts0 = imagine_rollout(rssm, actor, z0, h0, HZ, urand_t=urand_t, urand_a=urand_a)
    assert torch.equal(traj1, traj0)
    assert torch.equal(acts1, acts0)
    zs = traj1[1:, :, :SK].reshape(HZ, B, S, K).float()
    assert torch.equal(zs.sum(-1), torch.ones(HZ, B, S, device="cuda"))
