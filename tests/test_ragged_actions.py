"""MultiDiscrete (ragged-head) DreamerV3 behaviour path, CPU side: the eager
reference of ``ops.categorical_st_ragged``, the relaxed ``imagine_applicable``
gate and ``Actor.policy_log_probs``."""

import torch

from sheeprl_amd import ops

SIZES = [3, 1, 5]
UNIMIX = 0.01


def _segments(sizes):
    off = 0
    for k in sizes:
        yield off, k
        off += k


def test_categorical_st_ragged_cpu_matches_per_head():
    torch.manual_seed(0)
    A = sum(SIZES)
    raw = torch.randn(6, 4, A)
    gm = torch.randn(6, 4, A)

    raw_r = raw.clone().requires_grad_()
    m, onehot = ops.categorical_st_ragged(raw_r, SIZES, unimix=UNIMIX, sample=False)
    assert m.dtype == torch.float32 and m.shape == raw.shape and onehot.shape == raw.shape
    (m * gm).sum().backward()

    raw_h = raw.clone().requires_grad_()
    ms, ohs = [], []
    for off, k in _segments(SIZES):
        mh, oh = ops.categorical_st(raw_h[..., off : off + k], unimix=UNIMIX, sample=False)
        ms.append(mh)
        ohs.append(oh)
    m_ref, oh_ref = torch.cat(ms, -1), torch.cat(ohs, -1)
    (m_ref * gm).sum().backward()

    assert torch.equal(m, m_ref)
    assert torch.equal(onehot, oh_ref)
    assert torch.allclose(raw_r.grad, raw_h.grad, atol=1e-6, rtol=0), (raw_r.grad - raw_h.grad).abs().max()


def test_categorical_st_ragged_cpu_sampling_follows_urand():
    torch.manual_seed(1)
    A = sum(SIZES)
    raw = torch.randn(32, A)
    urand = torch.rand(32, A)
    m, onehot = ops.categorical_st_ragged(raw, SIZES, unimix=UNIMIX, sample=True, urand=urand)
    for off, k in _segments(SIZES):
        u = urand[:, off : off + k]
        g = -torch.log(torch.clamp(-torch.log(u.clamp_min(1e-20)), min=1e-20))
        idx = (m[:, off : off + k] + g).argmax(-1)
        assert torch.equal(onehot[:, off : off + k], torch.nn.functional.one_hot(idx, k).to(raw.dtype))
    # one draw per head, every row
    assert torch.equal(onehot.sum(-1), torch.full((32,), float(len(SIZES))))


def _rssm_and_actor(actions_dim, is_continuous=False):
    from sheeprl_amd.algos.dreamer_v3.agent import RSSM, Actor, RecurrentModel
    from sheeprl_amd.models import MLP

    H, S, K, DU, P = 16, 4, 4, 16, 20
    SK = S * K
    A = sum(actions_dim)
    rssm = RSSM(
        RecurrentModel(SK + A, H, DU),
        MLP(24 + H, SK, [P], activation="silu", layer_norm=True, layer_norm_eps=1e-3),
        MLP(H, SK, [P], activation="silu", layer_norm=True, layer_norm_eps=1e-3),
        discrete=K,
        unimix=UNIMIX,
    )
    actor = Actor(SK + H, actions_dim, is_continuous, dense_units=DU, mlp_layers=2, unimix=UNIMIX)
    return rssm, actor, SK + H


def test_imagine_applicable_accepts_multidiscrete_actor():
    from sheeprl_amd.algos.dreamer_v3.imagine import imagine_applicable

    torch.manual_seed(2)
    rssm, actor, _ = _rssm_and_actor([3, 5, 2])
    assert len(actor.mlp_heads) == 3
    assert imagine_applicable(rssm, actor)
    rssm_c, actor_c, _ = _rssm_and_actor([4], is_continuous=True)
    assert not imagine_applicable(rssm_c, actor_c)


def test_imagine_applicable_rejects_more_heads_than_one_launch_takes():
    """The ragged kernel's head table holds MAX_RAGGED_HEADS entries: an actor
    with more heads must keep the module loop, not reach the fast path."""
    from sheeprl_amd.algos.dreamer_v3.imagine import imagine_applicable

    assert ops.MAX_RAGGED_HEADS == 8
    torch.manual_seed(4)
    rssm, actor, _ = _rssm_and_actor([2] * ops.MAX_RAGGED_HEADS)
    assert imagine_applicable(rssm, actor)
    rssm9, actor9, _ = _rssm_and_actor([2] * (ops.MAX_RAGGED_HEADS + 1))
    assert len(actor9.mlp_heads) == 9
    assert not imagine_applicable(rssm9, actor9)


def test_categorical_st_ragged_cpu_more_heads_than_one_launch():
    torch.manual_seed(5)
    sizes = [2, 3, 1, 4, 2, 5, 3, 2, 4, 1, 3]  # 11 heads
    raw = torch.randn(5, sum(sizes), requires_grad=True)
    m, onehot = ops.categorical_st_ragged(raw, sizes, unimix=UNIMIX, sample=False)
    for off, k in _segments(sizes):
        m_h, oh_h = ops.categorical_st(raw[:, off : off + k], unimix=UNIMIX, sample=False)
        assert torch.equal(m[:, off : off + k], m_h)
        assert torch.equal(onehot[:, off : off + k], oh_h)
    m.sum().backward()
    assert torch.isfinite(raw.grad).all()


def test_policy_log_probs_matches_per_head_dists():
    torch.manual_seed(3)
    _, actor, latent = _rssm_and_actor([3, 5, 2])
    state = torch.randn(4, 7, latent)
    with torch.no_grad():
        got = actor.policy_log_probs(state)
        ref = torch.cat([d.logits for d in actor(state, greedy=True)[1]], -1)
    assert got.shape == (4, 7, 10)
    assert torch.equal(got, ref)
