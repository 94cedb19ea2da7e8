"""The categorical straight-through kernel family on the GPU.  Every sampler
kernel runs one of four shared device cores (wave forward / backward,
group-serial forward, lane-per-column backward), so the out-variants, the
strided and second-destination paths and the reset-fused kernels must agree
bit for bit with the plain kernels; the serial family agrees with the wave
family up to summation order.  The extension entry points are called directly.
"""

import pytest
import torch

requires_gpu = pytest.mark.gpu

if torch.cuda.is_available():
    from sheeprl_amd.ops._ext import require_ext

B, S = 3, 5  # 15 waves: not a multiple of the 4 waves per block, the tail block has idle waves
# width-1 row, partial wave, exactly one trip, one lane into a second trip, three trips
WIDTHS = [1, 9, 64, 65, 130]
DTYPES = [torch.float32, torch.bfloat16]  # libm path, fast intrinsics
UNIMIX = 0.01
SENTINEL = -7.0
# reset-fused geometries (S, K, A, H): H/S = 4; H/S = 96 (the h-slice loop takes two trips)
RESET_GEOMS = [(5, 9, 3, 20), (2, 65, 1, 192)]


@pytest.fixture(scope="module", autouse=True)
def _check_env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sheeprl_amd.ops import has_ext

    assert has_ext(), "HIP extension _sheep_hip not built — GPU path would silently degrade"


def _logits(K, dtype, seed, s=S):
    torch.manual_seed(seed)
    raw = (torch.randn(B, s, K, device="cuda") * 2).to(dtype)
    urand = torch.rand(B, s, K, device="cuda")
    return raw, urand


def _padded(rows, cols, dtype, left, right):
    """[rows, cols] column slice of a wider sentinel-filled buffer."""
    buf = torch.full((rows, left + cols + right), SENTINEL, device="cuda", dtype=dtype)
    return buf, buf[:, left : left + cols]


def _sentinels_untouched(buf, left, cols):
    return bool((buf[:, :left] == SENTINEL).all()) and bool((buf[:, left + cols :] == SENTINEL).all())


def _binary_f(dtype):
    """[B, 1] reset flags in {0, 1} with both values present."""
    return torch.tensor([[0.0], [1.0], [0.0]], device="cuda", dtype=dtype)


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", WIDTHS)
def test_fwd_o_equals_fwd(K, dtype):
    """cat_st_fwd_o == cat_st_fwd: contiguous outputs, a row-strided one-hot
    destination, and a second destination at another row stride."""
    ext = require_ext()
    raw, urand = _logits(K, dtype, 0)
    m_ref, oh_ref, s_ref = ext.cat_st_fwd(raw, urand, UNIMIX, True)
    assert bool((oh_ref.float().sum(-1) == 1).all())

    def outputs():
        return torch.empty(B, S, K, device="cuda"), torch.empty(B, S, K, device="cuda")

    m, s = outputs()
    oh = torch.empty(B, S, K, device="cuda", dtype=dtype)
    ext.cat_st_fwd_o(raw, urand, UNIMIX, m, oh, s)
    assert torch.equal(m, m_ref) and torch.equal(s, s_ref) and torch.equal(oh, oh_ref)

    m, s = outputs()
    buf, oh = _padded(B, S * K, dtype, 3, 5)
    ext.cat_st_fwd_o(raw, urand, UNIMIX, m, oh, s)
    assert torch.equal(m, m_ref) and torch.equal(s, s_ref)
    assert torch.equal(oh.reshape(B, S, K), oh_ref)
    assert _sentinels_untouched(buf, 3, S * K)

    m, s = outputs()
    buf, oh = _padded(B, S * K, dtype, 3, 5)
    buf2, oh2 = _padded(B, S * K, dtype, 1, 10)
    assert oh2.stride(0) != oh.stride(0)
    ext.cat_st_fwd_o(raw, urand, UNIMIX, m, oh, s, oh2)
    assert torch.equal(m, m_ref) and torch.equal(s, s_ref)
    assert torch.equal(oh.reshape(B, S, K), oh_ref) and torch.equal(oh2.reshape(B, S, K), oh_ref)
    assert _sentinels_untouched(buf, 3, S * K) and _sentinels_untouched(buf2, 1, S * K)


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", WIDTHS)
def test_bwd_o_equals_bwd_and_closed_form(K, dtype):
    """cat_st_bwd_o without gon2 == cat_st_bwd.  With gon2 the kernel adds
    gm/p + gon + gon2 in that order, which no cat_st_bwd call reproduces, so
    that path is held to the float64 closed form
    (1-u) * s * (t - sum t*s), t = gm/p + gon + gon2: fp32 accumulation over
    at most 130 terms and one final rounding give atol = rtol = 1e-5 in fp32
    and one bf16 ulp of the result plus 1e-5 in bf16."""
    ext = require_ext()
    raw, urand = _logits(K, dtype, 1)
    _, _, s = ext.cat_st_fwd(raw, urand, UNIMIX, True)
    gm = torch.randn(B, S, K, device="cuda")
    gon = torch.randn(B, S, K, device="cuda").to(dtype)
    gon2 = torch.randn(B, S, K, device="cuda").to(dtype)

    ref = ext.cat_st_bwd(gm, gon, s, UNIMIX)
    out = torch.full((B, S, K), SENTINEL, device="cuda", dtype=dtype)
    ext.cat_st_bwd_o(gm, gon, None, s, UNIMIX, out)
    assert torch.equal(out, ref)

    out2 = torch.full((B, S, K), SENTINEL, device="cuda", dtype=dtype)
    ext.cat_st_bwd_o(gm, gon, gon2, s, UNIMIX, out2)
    s64 = s.double()
    t = gm.double() / ((1.0 - UNIMIX) * s64 + UNIMIX / K) + gon.double() + gon2.double()
    closed = (1.0 - UNIMIX) * s64 * (t - (t * s64).sum(-1, keepdim=True))
    err = (out2.double() - closed).abs()
    print(f"K={K} {dtype}: max |gon2 path - closed form| = {err.max().item():.3e}")
    if dtype == torch.float32:
        bound = 1e-5 + 1e-5 * closed.abs()
    else:
        # bf16 has 8 significand bits: ulp(x) = 2^(floor(log2|x|) - 7)
        ulp = torch.where(closed == 0, torch.zeros_like(closed), torch.exp2(torch.floor(torch.log2(closed.abs())) - 7))
        bound = ulp + 1e-5
    assert bool((err <= bound).all()), (err - bound).max().item()


def _reset_inputs(geom, dtype, seed):
    s_, K, A, H = geom
    raw, urand = _logits(K, dtype, seed, s=s_)
    SK = s_ * K

    def g(*shape):
        return torch.randn(*shape, device="cuda").to(dtype)

    return raw, urand, SK, g


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geom", RESET_GEOMS)
def test_resets_fwd_equals_unfused_pair(geom, dtype):
    """cat_st_resets_fwd == cat_st_fwd_o followed by scan_resets_fwd: m, s, the
    one-hot and the next step's x[:, :SK+A] / hu[:, :H] blocks, written into
    column slices of wider buffers as in the scan.  The one-hot is exact in
    bf16, so the unfused path's re-read of it rounds nothing."""
    ext = require_ext()
    s_, K, A, H = geom
    raw, urand, SK, g = _reset_inputs(geom, dtype, 2)
    iz, h, ih, act, f = g(B, SK), g(B, H), g(B, H), g(B, A), _binary_f(dtype)

    def run(fused):
        m = torch.empty(B, s_, K, device="cuda")
        s = torch.empty(B, s_, K, device="cuda")
        z = torch.empty(B, SK, device="cuda", dtype=dtype)
        xbuf, x = _padded(B, SK + A, dtype, 2, 6)
        hubuf, hu = _padded(B, H, dtype, 4, 8)
        if fused:
            ext.cat_st_resets_fwd(raw, urand, UNIMIX, m, z, s, iz, h, ih, act, f, x, hu)
        else:
            ext.cat_st_fwd_o(raw, urand, UNIMIX, m, z.view(B, s_, K), s)
            ext.scan_resets_fwd(z, iz, h, ih, act, f, x, hu, False)
        assert _sentinels_untouched(xbuf, 2, SK + A) and _sentinels_untouched(hubuf, 4, H)
        return m, s, z, x, hu

    for name, a, b in zip(("m", "s", "onehot", "x_next", "hu_next"), run(True), run(False)):
        assert torch.equal(a, b), name


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geom", RESET_GEOMS)
def test_resets_bwd_equals_unfused_pair(geom, dtype):
    """cat_st_resets_bwd == scan_resets_bwd followed by cat_st_bwd_o with the
    produced gz_carry as gon2: graw, gh_carry, ga and both init-state
    accumulators (started from the same non-zero values).  In fp32 the two
    paths are the same arithmetic for any f; in bf16 the unfused path rounds
    the carry (1-f)*gx to bf16 before the ST backward reads it, which is exact
    only because f is 0 or 1 — keep f binary."""
    ext = require_ext()
    s_, K, A, H = geom
    raw, urand, SK, g = _reset_inputs(geom, dtype, 3)
    _, _, s = ext.cat_st_fwd(raw, urand, UNIMIX, True)
    gm = torch.randn(B, s_, K, device="cuda")
    gon, ghp, f = g(B, s_, K), g(B, H), _binary_f(dtype)
    _, ghu = _padded(B, H, dtype, 0, 8)  # [B, :H] of the [B, H + D] GEMM output
    ghu.copy_(g(B, H))
    _, gx = _padded(B, SK + A, dtype, 2, 6)
    gx.copy_(g(B, SK + A))
    gih0, giz0 = torch.randn(B, H, device="cuda"), torch.randn(B, SK, device="cuda")

    def run(fused):
        graw = torch.full((B, s_, K), SENTINEL, device="cuda", dtype=dtype)
        gh_carry = torch.full((B, H), SENTINEL, device="cuda", dtype=dtype)
        ga = torch.full((B, A), SENTINEL, device="cuda", dtype=dtype)
        gih, giz = gih0.clone(), giz0.clone()
        if fused:
            ext.cat_st_resets_bwd(gm, gon, s, UNIMIX, graw, ghu, ghp, gx, f, gh_carry, ga, gih, giz)
        else:
            gz_carry = torch.empty(B, SK, device="cuda", dtype=dtype)
            ext.scan_resets_bwd(ghu, ghp, gx, f, gh_carry, gz_carry, ga, gih, giz)
            ext.cat_st_bwd_o(gm, gon, gz_carry.view(B, s_, K), s, UNIMIX, graw)
        return graw, gh_carry, ga, gih, giz

    fused, unfused = run(True), run(False)
    for name, a, b in zip(("graw", "gh_carry", "ga", "gih_acc", "giz_acc"), fused, unfused):
        assert torch.equal(a, b), name
    assert not torch.equal(fused[3], gih0) and not torch.equal(fused[4], giz0)  # the accumulators did move


@requires_gpu
@pytest.mark.parametrize("KD", [16, 32])
def test_serial_family_matches_wave_family(KD):
    """g16_cat_st (one thread per group, serial libm sums) against cat_st_fwd
    in fp32 (one wave per row, libm, 64-lane tree sums).  An identity GEMM
    (W = I, bias = 0) hands the serial kernel the bf16 logits exactly.  The
    two differ only in summation order: s within 1e-6; m = log p with unit-
    scale logits stays inside (-8, 0), where two fp32 ulps are 9.6e-7 < 1e-6.
    One uniform per group is driven to 1 - 1e-7 and the rest held at 0.3, so
    no argmax sits on a near-tie and the one-hots are equal."""
    ext = require_ext()
    N = 64
    groups = N // KD
    torch.manual_seed(4)
    logits = torch.randn(B, N, device="cuda").to(torch.bfloat16)
    W = torch.eye(N, device="cuda", dtype=torch.bfloat16)
    bias = torch.zeros(N, device="cuda", dtype=torch.bfloat16)
    urand = torch.full((B, groups, KD), 0.3, device="cuda")
    pick = torch.randint(0, KD, (B, groups), device="cuda")
    urand.scatter_(-1, pick.unsqueeze(-1), 1.0 - 1e-7)

    m = torch.empty(B, N, device="cuda")
    z = torch.empty(B, N, device="cuda", dtype=torch.bfloat16)
    s = torch.empty(B, groups, KD, device="cuda")
    ext.g16_cat_st(logits, W, bias, urand, m, z, s, KD, UNIMIX)
    m_ref, oh_ref, s_ref = ext.cat_st_fwd(logits.float().view(B, groups, KD), urand, UNIMIX, True)
    dm = (m.view(B, groups, KD) - m_ref).abs().max().item()
    ds = (s - s_ref).abs().max().item()
    print(f"KD={KD}: max |m diff| = {dm:.3e}, max |s diff| = {ds:.3e}")
    assert dm <= 1e-6 and ds <= 1e-6
    assert torch.equal(z.float().view(B, groups, KD), oh_ref)
    assert torch.equal(oh_ref.argmax(-1), pick)
