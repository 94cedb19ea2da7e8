"""Fused unimix-categorical straight-through head.

Replaces the DV3 stochastic-state subgraph (unimix mixing dreamer_v3/agent.py
:437-449 + one-hot ST sampling dreamer_v2/utils.py:44): softmax -> uniform
mix -> log -> gumbel sample -> one-hot -> straight-through, ~20 eager kernels,
collapsed to rand + one fwd kernel (+ one bwd kernel).

Returns (mixed_log_probs fp32, st_sample input-dtype).  The straight-through
gradient of the sample flows through the mixed probabilities p, identical to
``onehot + p - p.detach()``.
"""

from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from sheeprl_amd.ops._ext import require_ext, use_hip


def _ref_fwd(raw: Tensor, unimix: float, u: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor]:
    """CPU reference for one head [..., K]: (m, s, one-hot); ``u`` (uniforms of
    raw's shape) drives the Gumbel-max sample, ``None`` takes argmax(m)."""
    K = raw.shape[-1]
    s = torch.softmax(raw.float(), dim=-1)
    m = torch.log((1.0 - unimix) * s + unimix / K)
    score = m
    if u is not None:
        score = m - torch.log(torch.clamp(-torch.log(u.clamp_min(1e-20)), min=1e-20))
    return m, s, torch.nn.functional.one_hot(score.argmax(-1), K).to(raw.dtype)


def _ref_bwd(gm: Tensor, gon: Optional[Tensor], s: Tensor, unimix: float) -> Tensor:
    """CPU reference for one head: fp32 grad wrt the raw logits."""
    p = (1.0 - unimix) * s + unimix / s.shape[-1]
    t = gm.float() / p
    if gon is not None:
        t = t + gon.float()
    acc = (t * s).sum(-1, keepdim=True)
    return (1.0 - unimix) * s * (t - acc)


class _CategoricalST(torch.autograd.Function):
    @staticmethod
    def forward(ctx, raw: Tensor, unimix: float, sample: bool) -> Tuple[Tensor, Tensor]:
        if use_hip(raw):
            rawc = raw.contiguous()
            u = torch.rand(rawc.shape, dtype=torch.float32, device=raw.device) if sample else None
            m, onehot, s = require_ext().cat_st_fwd(rawc, u, float(unimix), bool(sample))
        else:
            u = torch.rand(raw.shape, dtype=torch.float32, device=raw.device) if sample else None
            m, s, onehot = _ref_fwd(raw, unimix, u)
        ctx.save_for_backward(s)
        ctx.unimix = unimix
        ctx.raw_dtype = raw.dtype
        return m, onehot

    @staticmethod
    def backward(ctx, gm: Tensor, gon: Tensor):
        (s,) = ctx.saved_tensors
        unimix = ctx.unimix
        if use_hip(s):
            graw = require_ext().cat_st_bwd(gm.contiguous(), gon.contiguous().to(ctx.raw_dtype), s, float(unimix))
        else:
            graw = _ref_bwd(gm, gon, s, unimix).to(ctx.raw_dtype)
        return graw, None, None


def categorical_st(raw_logits: Tensor, unimix: float = 0.01, sample: bool = True) -> Tuple[Tensor, Tensor]:
    """raw_logits [..., K] -> (mixed log-probs fp32 [..., K], one-hot ST sample)."""
    return _CategoricalST.apply(raw_logits, unimix, sample)


# heads one ragged kernel launch takes (its by-value head table; the
# extension exports the same number as ``MAX_RAGGED_HEADS``)
MAX_RAGGED_HEADS = 8


def _head_groups(sizes: Sequence[int]):
    """(column offset, width, sizes) of consecutive runs of at most
    MAX_RAGGED_HEADS heads — one kernel launch each."""
    off = 0
    for i in range(0, len(sizes), MAX_RAGGED_HEADS):
        grp = list(sizes[i : i + MAX_RAGGED_HEADS])
        yield off, sum(grp), grp
        off += sum(grp)


class _CategoricalSTRagged(torch.autograd.Function):
    """``_CategoricalST`` over ragged heads: columns [off_h, off_h + K_h) of
    the last axis are head h, each with its own softmax, unimix denominator
    and sample.  One HIP launch per direction for up to MAX_RAGGED_HEADS
    heads; beyond that, one launch per run of MAX_RAGGED_HEADS heads on
    column slices (same results, the heads are independent)."""

    @staticmethod
    def forward(
        ctx, raw: Tensor, sizes: Tuple[int, ...], unimix: float, sample: bool, urand: Optional[Tensor]
    ) -> Tuple[Tensor, Tensor]:
        if use_hip(raw):
            rawc = raw.contiguous()
            if sample:
                if urand is None:
                    urand = torch.rand(rawc.shape, dtype=torch.float32, device=raw.device)
                urand = urand.contiguous()
            else:
                urand = None
            ext = require_ext()
            if len(sizes) <= MAX_RAGGED_HEADS:
                m, onehot, s = ext.cat_st_ragged_fwd(rawc, urand, list(sizes), float(unimix), bool(sample))
            else:
                parts = [
                    ext.cat_st_ragged_fwd(
                        rawc[..., off : off + w].contiguous(),
                        None if urand is None else urand[..., off : off + w].contiguous(),
                        grp, float(unimix), bool(sample),
                    )
                    for off, w, grp in _head_groups(sizes)
                ]
                m, onehot, s = (torch.cat([p[i] for p in parts], -1) for i in range(3))
        else:
            if sample and urand is None:
                urand = torch.rand(raw.shape, dtype=torch.float32, device=raw.device)
            heads, off = [], 0
            for K in sizes:
                u = urand[..., off : off + K] if sample else None
                heads.append(_ref_fwd(raw[..., off : off + K], unimix, u))
                off += K
            m, s, onehot = (torch.cat([h[i] for h in heads], -1) for i in range(3))
        ctx.save_for_backward(s)
        ctx.sizes = tuple(sizes)
        ctx.unimix = unimix
        ctx.raw_dtype = raw.dtype
        # an unused output (the one-hot of a log-probs-only call) reaches
        # backward as None instead of a materialized zero tensor
        ctx.set_materialize_grads(False)
        return m, onehot

    @staticmethod
    def backward(ctx, gm: Optional[Tensor], gon: Optional[Tensor]):
        (s,) = ctx.saved_tensors
        unimix = ctx.unimix
        if gm is None and gon is None:
            return None, None, None, None, None
        if gm is None:
            gm = torch.zeros_like(s)
        if use_hip(s):
            ext = require_ext()
            gmc = gm.contiguous().float()
            gonc = None if gon is None else gon.contiguous().to(ctx.raw_dtype)
            if len(ctx.sizes) <= MAX_RAGGED_HEADS:
                graw = ext.cat_st_ragged_bwd(gmc, gonc, s, list(ctx.sizes), float(unimix), ctx.raw_dtype)
            else:
                graw = torch.cat(
                    [
                        ext.cat_st_ragged_bwd(
                            gmc[..., off : off + w].contiguous(),
                            None if gonc is None else gonc[..., off : off + w].contiguous(),
                            s[..., off : off + w].contiguous(),
                            grp, float(unimix), ctx.raw_dtype,
                        )
                        for off, w, grp in _head_groups(ctx.sizes)
                    ],
                    -1,
                )
        else:
            gs, off = [], 0
            for K in ctx.sizes:
                gon_h = None if gon is None else gon[..., off : off + K]
                gs.append(_ref_bwd(gm[..., off : off + K], gon_h, s[..., off : off + K], unimix))
                off += K
            graw = torch.cat(gs, -1).to(ctx.raw_dtype)
        return graw, None, None, None, None


def categorical_st_ragged(
    raw_logits: Tensor,
    sizes: Sequence[int],
    unimix: float = 0.01,
    sample: bool = True,
    urand: Optional[Tensor] = None,
) -> Tuple[Tensor, Tensor]:
    """raw_logits [..., A] with A = sum(sizes) -> (per-head mixed log-probs fp32
    [..., A], per-head one-hot ST samples [..., A]).  ``urand`` ([..., A] fp32
    uniforms) replaces the internal ``torch.rand`` draw for parity tests.

    Any head count works on CPU and on HIP.  One kernel launch covers up to
    ``MAX_RAGGED_HEADS`` (8) heads; more heads are processed in runs of 8 on
    column slices, with identical results.  The fast imagination rollout
    (``imagine_applicable``) only takes actors within the one-launch limit."""
    sizes = tuple(int(k) for k in sizes)
    if not sizes or min(sizes) < 1 or sum(sizes) != raw_logits.shape[-1]:
        raise ValueError(f"head sizes {sizes} do not partition the last dimension {raw_logits.shape[-1]}")
    if urand is not None and (urand.shape != raw_logits.shape or urand.dtype != torch.float32):
        raise ValueError("urand must be fp32 with the logits' shape")
    return _CategoricalSTRagged.apply(raw_logits, sizes, unimix, sample, urand)
