"""Few-row LayerNorm(+SiLU) routing: at the scan's row counts contiguous and
row-strided operands must give the same results whichever kernel the host
dispatch picks (N = 64 / 65 straddle the backward's default few-row limit;
the forward routes by stride alone), and the ``*_acc`` backward adds to its
fp32 accumulators instead of overwriting them.  test_ln_wide_rows_k4 runs
the same checks at N=65, D=1536, the one shape here that reaches the bf16
K=4 vectorized kernels, and asserts that route first.

Reference: float64 on the same quantized inputs; bounds are test_ln_act's for
the dtype (forward 1e-5 / 3e-2, gx 1e-4 / 1e-1, gw/gb atol 1e-3 / 0.3 with
rtol 5e-2)."""

import pytest
import torch

requires_gpu = pytest.mark.gpu

EPS = 1e-3


@pytest.fixture(scope="module", autouse=True)
def _check_env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sheeprl_amd.ops import has_ext

    assert has_ext(), "HIP extension _sheep_hip not built — GPU path would silently degrade"


def _ref(x, w, b, gy, silu):
    """float64 LN(+SiLU) forward and backward: y, mean, rstd, gx, gw, gb."""
    x = x.double().requires_grad_()
    w = w.double().requires_grad_()
    b = b.double().requires_grad_()
    mean = x.mean(-1, keepdim=True)
    var = x.var(-1, unbiased=False, keepdim=True)
    rstd = torch.rsqrt(var + EPS)
    y = (x - mean) * rstd * w + b
    if silu:
        y = torch.nn.functional.silu(y)
    y.backward(gy.double())
    return y.detach(), x.grad, w.grad, b.grad


@requires_gpu
@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D", [64, 256, 512])
@pytest.mark.parametrize("N", [1, 16, 64, 65])
def test_ln_few_rows(N, D, dtype, silu):
    from sheeprl_amd.ops._ext import require_ext

    _check(require_ext(), N, D, dtype, silu)


@requires_gpu
@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ln_wide_rows_k4(dtype, silu):
    """N=65, D=1536: in bf16 the vectorized wave-per-row kernels with K=4
    (48 of 64 lanes active), forward and backward, contiguous and row-strided;
    in fp32 (96 lanes would be needed) the block-per-row kernels, uncached."""
    from sheeprl_amd.ops._ext import require_ext

    ext = require_ext()
    N, D = 65, 1536
    itemsize = torch.empty((), dtype=dtype).element_size()
    want = ("VEC", 4, False) if dtype == torch.bfloat16 else ("ROW", 0, False)
    # the strides _check runs: contiguous, forward slice of [N, D+24], backward slice of [N, 8+D]
    for backward, stride in ((False, D), (False, D + 24), (True, D), (True, 8 + D)):
        assert tuple(ext.ln_act_route(N, D, stride, itemsize, backward)) == want, (backward, stride)
    _check(ext, N, D, dtype, silu)


def _check(ext, N, D, dtype, silu):
    torch.manual_seed(N * 1000 + D)
    dev = "cuda"
    x = torch.randn(N, D, device=dev).to(dtype)
    w = torch.randn(D, device=dev)
    b = torch.randn(D, device=dev)
    gy = torch.randn(N, D, device=dev).to(dtype)
    y_ref, gx_ref, gw_ref, gb_ref = _ref(x, w, b, gy, silu)

    ftol = 1e-5 if dtype == torch.float32 else 3e-2
    btol = 1e-4 if dtype == torch.float32 else 1e-1
    wtol = 1e-3 if dtype == torch.float32 else 0.3

    # forward: contiguous output and a row-strided slice of a wider buffer
    stats = {}
    for strided in (False, True):
        buf = torch.full((N, D + 24), 7.0, device=dev, dtype=dtype)
        y = buf[:, 8 : 8 + D] if strided else torch.empty(N, D, device=dev, dtype=dtype)
        mean = torch.empty(N, device=dev, dtype=torch.float32)
        rstd = torch.empty(N, device=dev, dtype=torch.float32)
        ext.ln_act_fwd_o(x, w, b, EPS, silu, y, mean, rstd)
        assert torch.allclose(y.double(), y_ref, atol=ftol, rtol=ftol), (strided, (y.double() - y_ref).abs().max())
        if strided:
            assert (buf[:, :8] == 7).all() and (buf[:, 8 + D :] == 7).all()
        stats[strided] = (mean, rstd)
    xd = x.double()
    assert torch.allclose(stats[False][0].double(), xd.mean(-1), atol=1e-5, rtol=1e-5)
    assert torch.allclose(stats[False][1].double(), torch.rsqrt(xd.var(-1, unbiased=False) + EPS),
                          atol=1e-5, rtol=1e-4)
    # (fp32 sums of D <= 1536 unit-scale terms, divided by D: ~2^-24 * sqrt(D) in any order)
    assert torch.allclose(stats[True][0], stats[False][0], atol=1e-5, rtol=1e-5)
    assert torch.allclose(stats[True][1], stats[False][1], atol=1e-5, rtol=1e-4)

    # backward: gy contiguous and row-strided, accumulators pre-filled
    mean, rstd = stats[False]
    for strided in (False, True):
        if strided:
            gbuf = torch.full((N, 8 + D), 7.0, device=dev, dtype=dtype)
            gbuf[:, 8:] = gy
            gy_in = gbuf[:, 8:]
        else:
            gy_in = gy
        gw0 = torch.randn(D, device=dev)
        gb0 = torch.randn(D, device=dev)
        gw_acc, gb_acc = gw0.clone(), gb0.clone()
        gx = torch.empty(N, D, device=dev, dtype=dtype)
        ext.ln_act_bwd_acc(gy_in, x, w, b, mean, rstd, silu, gx, gw_acc, gb_acc)
        assert torch.allclose(gx.double(), gx_ref, atol=btol, rtol=btol), (strided, (gx.double() - gx_ref).abs().max())
        assert torch.allclose((gw_acc - gw0).double(), gw_ref, atol=wtol, rtol=5e-2), (
            strided, ((gw_acc - gw0).double() - gw_ref).abs().max())
        assert torch.allclose((gb_acc - gb0).double(), gb_ref, atol=wtol, rtol=5e-2), (
            strided, ((gb_acc - gb0).double() - gb_ref).abs().max())
        # added to, not overwritten: the pre-fill is still in there
        assert torch.allclose(gw_acc.double(), gw0.double() + gw_ref, atol=wtol, rtol=5e-2)
