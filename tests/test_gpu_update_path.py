"""The kernels that write the parameters — adam_step_mt, rmsprop_step_mt,
clip_grad_norm_mt, ema_update, chlast_bias_sum, obs_norm — against plain
float64 torch on the CPU (torch.optim.Adam on float64 clones where it applies),
at the chunk-table boundaries (last chunk of a tensor / first chunk of the
next), with guard bands around every parameter and gradient."""

import pytest
import torch

requires_gpu = pytest.mark.gpu

if torch.cuda.is_available():
    from sheeprl_amd import ops
    from sheeprl_amd.ops import has_ext


@pytest.fixture(scope="module", autouse=True)
def _check_env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    # on a GPU box the extension MUST be present: fail loudly, never fall back
    from sheeprl_amd.ops import has_ext

    assert has_ext(), "HIP extension _sheep_hip not built — GPU path would silently degrade"


# ---------------------------------------------------------------------------
# shared parameter set
# ---------------------------------------------------------------------------

# around the 256-thread block and the 4096-element chunk, one / two / three chunks
SIZES = (1, 255, 256, 257, 4095, 4096, 4097, 8193, 12289)
CONV_SHAPE = (8, 4, 3, 3)
GUARD = 64
SENTINEL = -77.0  # exact in bf16; no update below produces it


class ParamSet:
    """1-D parameters carved from one flat buffer with GUARD-element sentinel
    bands between them (gradients likewise), a channels_last conv weight with
    a channels_last gradient, and an empty parameter — in that order."""

    def __init__(self, dtype, seed=0, sizes=SIZES, conv=True, empty=True):
        gen = torch.Generator().manual_seed(seed)
        self.dtype = dtype
        total = GUARD + sum(n + GUARD for n in sizes)
        flat_p = torch.full((total,), SENTINEL)
        flat_g = torch.full((total,), SENTINEL)
        self.guard_mask = torch.ones(total, dtype=torch.bool)
        self.spans = []
        o = GUARD
        for n in sizes:
            flat_p[o : o + n] = torch.randn(n, generator=gen)
            flat_g[o : o + n] = 0.0
            self.guard_mask[o : o + n] = False
            self.spans.append((o, n))
            o += n + GUARD
        self.flat_p = flat_p.to(dtype).cuda()
        self.flat_g = flat_g.to(dtype).cuda()
        self.params = []
        for o, n in self.spans:
            p = torch.nn.Parameter(self.flat_p[o : o + n])
            p.grad = self.flat_g[o : o + n]
            assert p.data_ptr() == self.flat_p.data_ptr() + o * self.flat_p.element_size()
            assert p.is_contiguous() and p.grad.is_contiguous()
            self.params.append(p)
        if conv:
            w = torch.randn(CONV_SHAPE, generator=gen).to(dtype).cuda()
            p = torch.nn.Parameter(w.contiguous(memory_format=torch.channels_last))
            p.grad = torch.zeros_like(p)
            assert p.grad.stride() == p.stride() and not p.is_contiguous()
            self.params.append(p)
        if empty:
            p = torch.nn.Parameter(torch.empty(0, dtype=dtype, device="cuda"))
            p.grad = torch.empty(0, dtype=dtype, device="cuda")
            self.params.append(p)

    def clones64(self):
        """float64 CPU leaf clones for the reference optimizer."""
        return [torch.nn.Parameter(p.detach().cpu().double().contiguous()) for p in self.params]

    def draw_grads(self, gen, scale=1.0, shift=0.0, integer=None):
        """New gradient values, rounded to the set's dtype, as CPU tensors."""
        out = []
        for p in self.params:
            if integer is not None:
                g = torch.randint(-integer, integer + 1, p.shape, generator=gen).float()
            else:
                g = torch.randn(p.shape, generator=gen) * scale + shift
            out.append(g.to(self.dtype))
        return out

    def write_grads(self, grads, refs=None, skip=()):
        """Write into the existing gradient buffers (addresses stay put)."""
        for i, (p, g) in enumerate(zip(self.params, grads)):
            if i in skip:
                continue
            p.grad.copy_(g.cuda())
            if refs is not None:
                refs[i].grad = g.double()

    def assert_guards(self):
        for name, flat in (("param", self.flat_p), ("grad", self.flat_g)):
            band = flat.cpu().float()[self.guard_mask]
            assert bool((band == SENTINEL).all()), f"{name} guard band overwritten"

    def assert_grads_zero(self, skip=()):
        for i, p in enumerate(self.params):
            if i not in skip:
                assert int(p.grad.count_nonzero()) == 0, f"grad {i} not zeroed by the kernel"


def _bf16_ulp(x):
    """Spacing of bf16 (8-bit significand) at |x|, as float64; 0 at 0."""
    x = x.double().abs()
    _, e = torch.frexp(x)  # x = m * 2**e, m in [0.5, 1)
    ulp = torch.ldexp(torch.ones_like(x), e - 8)
    return torch.where(x == 0, torch.zeros_like(x), ulp)


def _round_bf16_(refs):
    for r in refs:
        r.data.copy_(r.data.to(torch.bfloat16).double())


class _UlpBudget:
    """bf16 parameters: the kernel computes the update in fp32 from bf16 p and
    rounds to nearest, the reference does the same from fp64.  Two roundings of
    nearly equal values can only land on neighbouring bf16 values, so each
    step adds at most one bf16 ulp (taken at that step's magnitude) to the
    distance between the two trajectories.  Where p and the update cancel,
    the ulp of the result is smaller than the fp32 error of the subtraction
    itself, 2^-24 of the operands, so that is allowed on top."""

    def __init__(self, refs):
        self.budget = [torch.zeros_like(r.data) for r in refs]
        self.prev = [r.data.clone() for r in refs]

    def check(self, params, refs, what):
        for i, (p, r) in enumerate(zip(params, refs)):
            got = p.detach().cpu().double()
            ref = r.detach()
            self.budget[i] += _bf16_ulp(torch.maximum(got.abs(), ref.abs()))
            # |p| + |lr * upd| <= 2 |p_before| + |p_after|
            self.budget[i] += 2.0**-24 * (2 * self.prev[i].abs() + ref.abs())
            self.prev[i] = ref.clone()
            err = (got - ref).abs()
            assert bool((err <= self.budget[i]).all()), (
                what, i, float(err.max()), float((err - self.budget[i]).max()))


def _close(got, ref, rtol, atol, what):
    got = got.detach().cpu().double()
    ref = ref.detach().double()
    err = (got - ref).abs()
    bound = atol + rtol * ref.abs()
    assert bool((err <= bound).all()), (what, float(err.max()), float((err - bound).max()))


def _check_params(ps, refs, dtype, budget, what, skip=()):
    if dtype is torch.float32:
        for i, (p, r) in enumerate(zip(ps, refs)):
            if i not in skip:
                _close(p, r, 1e-5, 1e-5, (what, "p", i))
    else:
        budget.check(ps, refs, what)


# ---------------------------------------------------------------------------
# 1. Adam multi-tensor
# ---------------------------------------------------------------------------


@requires_gpu
@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_adam_multi_tensor(dtype, weight_decay):
    from sheeprl_amd.optim import FusedAdam

    ps = ParamSet(dtype, seed=1)
    refs = ps.clones64()
    opt = FusedAdam(ps.params, lr=1e-2, weight_decay=weight_decay)
    ref = torch.optim.Adam(refs, lr=1e-2, weight_decay=weight_decay)
    budget = _UlpBudget(refs)
    gen = torch.Generator().manual_seed(101)
    for step in range(1, 7):
        ps.write_grads(ps.draw_grads(gen), refs)
        opt.step()
        ref.step()
        assert opt._zeroes_grads_in_kernel is True, "multi-tensor path not taken"
        if dtype is torch.bfloat16:
            _round_bf16_(refs)
        _check_params(ps.params, refs, dtype, budget, step)
        # fp32 master moments: with bf16 parameters they see the same inputs
        # as the reference only while weight decay does not feed p back in
        if dtype is torch.float32 or weight_decay == 0.0:
            for i, (p, r) in enumerate(zip(ps.params, refs)):
                for k in ("exp_avg", "exp_avg_sq"):
                    assert opt.state[p][k].dtype == torch.float32
                    _close(opt.state[p][k], ref.state[r][k], 1e-5, 1e-6, (step, k, i))
        ps.assert_grads_zero()
        ps.assert_guards()


# ---------------------------------------------------------------------------
# 2. missing gradients
# ---------------------------------------------------------------------------


@requires_gpu
@pytest.mark.parametrize("late", [0, 2])
def test_adam_missing_gradients(late):
    """Parameter `late` has no gradient on step 1 and joins on step 2; one
    middle parameter never has a gradient.  Each parameter is bias-corrected
    with its own step count, as in torch.optim.Adam."""
    from sheeprl_amd.optim import FusedAdam

    ps = ParamSet(torch.float32, seed=2, sizes=(257, 4097, 4096, 300, 8193), conv=False, empty=False)
    never = 3
    refs = ps.clones64()
    opt = FusedAdam(ps.params, lr=1e-2)
    ref = torch.optim.Adam(refs, lr=1e-2)
    ps.params[never].grad = None
    frozen = ps.flat_p.clone()
    gen = torch.Generator().manual_seed(102)
    for step in range(1, 5):
        grads = ps.draw_grads(gen)
        absent = {never, late} if step == 1 else {never}
        for i, (p, r) in enumerate(zip(ps.params, refs)):
            if i in absent:
                p.grad = None
                r.grad = None
            else:
                # fresh tensors here: the eager per-parameter path leaves the
                # zeroing to the training loop
                p.grad = grads[i].cuda()
                r.grad = grads[i].double()
        opt.step()
        ref.step()
        # one shared step count on step 1, per-parameter counts afterwards
        assert opt._zeroes_grads_in_kernel is (step == 1)
        for i, (p, r) in enumerate(zip(ps.params, refs)):
            _close(p, r, 1e-5, 1e-5, (step, i))
        o, n = ps.spans[never]
        assert torch.equal(ps.flat_p[o - GUARD : o + n + GUARD], frozen[o - GUARD : o + n + GUARD])
        assert len(opt.state[ps.params[never]]) == 0
        ps.assert_guards()


# ---------------------------------------------------------------------------
# 3. chunk-table cache
# ---------------------------------------------------------------------------


@requires_gpu
def test_adam_table_cache_invalidation():
    from sheeprl_amd.optim import FusedAdam

    ps = ParamSet(torch.float32, seed=3)
    refs = ps.clones64()
    opt = FusedAdam(ps.params, lr=1e-2)
    ref = torch.optim.Adam(refs, lr=1e-2)
    gen = torch.Generator().manual_seed(103)
    for _ in range(2):
        ps.write_grads(ps.draw_grads(gen), refs)
        opt.step()
        ref.step()
    table = opt._mt_cache[id(opt.param_groups[0])]
    grads = ps.draw_grads(gen)
    ps.write_grads(grads, refs)
    moved = 4
    old = ps.params[moved].grad
    ps.params[moved].grad = grads[moved].cuda().clone()
    assert ps.params[moved].grad.data_ptr() != old.data_ptr()
    opt.step()
    ref.step()
    assert opt._zeroes_grads_in_kernel is True
    assert opt._mt_cache[id(opt.param_groups[0])] is not table, "stale chunk table reused"
    for i, (p, r) in enumerate(zip(ps.params, refs)):
        _close(p, r, 1e-5, 1e-5, ("moved grad", i))
    assert int(ps.params[moved].grad.count_nonzero()) == 0
    # the abandoned buffer still holds the gradient written before the swap
    assert torch.equal(old.cpu(), grads[moved])
    ps.assert_guards()


@requires_gpu
def test_adam_two_groups():
    from sheeprl_amd.optim import FusedAdam

    ps = ParamSet(torch.float32, seed=4)
    refs = ps.clones64()
    cut = 5
    hyper = [dict(lr=1e-2, betas=(0.9, 0.999)), dict(lr=3e-3, betas=(0.8, 0.99))]
    opt = FusedAdam([dict(params=ps.params[:cut], **hyper[0]), dict(params=ps.params[cut:], **hyper[1])])
    ref = torch.optim.Adam([dict(params=refs[:cut], **hyper[0]), dict(params=refs[cut:], **hyper[1])])
    gen = torch.Generator().manual_seed(104)
    for step in range(1, 4):
        ps.write_grads(ps.draw_grads(gen), refs)
        opt.step()
        ref.step()
        assert opt._zeroes_grads_in_kernel is True
        for i, (p, r) in enumerate(zip(ps.params, refs)):
            _close(p, r, 1e-5, 1e-5, (step, i))
        ps.assert_grads_zero()
        ps.assert_guards()
    assert len(opt._mt_cache) == 2


# ---------------------------------------------------------------------------
# 4. graph replay
# ---------------------------------------------------------------------------


@requires_gpu
@pytest.mark.timeout(120)
def test_adam_graph_replay_step_counts():
    """Replays must bias-correct with the advancing device step counter: p
    after replay k equals the reference after warmup + k steps."""
    from sheeprl_amd.optim import FusedAdam
    from sheeprl_amd.parallel.graphs import CUDAGraphStep

    ps = ParamSet(torch.float32, seed=5)
    refs = ps.clones64()
    opt = FusedAdam(ps.params, lr=1e-2)
    ref = torch.optim.Adam(refs, lr=1e-2)
    gen = torch.Generator().manual_seed(105)

    def fn(static):
        for i, p in enumerate(ps.params):
            p.grad.copy_(static[f"g{i}"])
        opt.step()

    warmup = 2
    g0 = ps.draw_grads(gen)
    graphed = CUDAGraphStep(fn, {f"g{i}": g.cuda() for i, g in enumerate(g0)}, warmup=warmup)
    for _ in range(warmup):  # capture records, it does not run
        for r, g in zip(refs, g0):
            r.grad = g.double()
        ref.step()
    step_t = opt.state[ps.params[0]]["step_t"]
    addr = step_t.data_ptr()
    for k in range(1, 6):
        gk = ps.draw_grads(gen)
        for r, g in zip(refs, gk):
            r.grad = g.double()
        ref.step()
        graphed({f"g{i}": g.cuda() for i, g in enumerate(gk)})
        torch.cuda.synchronize()
        for i, (p, r) in enumerate(zip(ps.params, refs)):
            _close(p, r, 1e-5, 1e-5, (k, i))
        assert float(step_t.item()) == warmup + k
        ps.assert_grads_zero()
        ps.assert_guards()
    assert opt.state[ps.params[0]]["step_t"].data_ptr() == addr


# ---------------------------------------------------------------------------
# 5. state_dict round trip
# ---------------------------------------------------------------------------


def _tensor_state(opt):
    out = {}
    params = [p for g in opt.param_groups for p in g["params"]]
    for i, p in enumerate(params):
        for k, v in opt.state[p].items():
            if isinstance(v, torch.Tensor):
                out[(i, k)] = v
    return out


@requires_gpu
@pytest.mark.parametrize("kind", ["adam", "rmsprop_tf"])
def test_state_round_trip_bf16(kind):
    """bf16 parameters: the fp32 state must come back from load_state_dict as
    fp32, bit for bit — asserted BEFORE any kernel sees the loaded buffers."""
    from sheeprl_amd.optim import FusedAdam, RMSpropTF

    def make(params):
        if kind == "adam":
            return FusedAdam(params, lr=1e-2, weight_decay=1e-2)
        return RMSpropTF(params, lr=1e-2, momentum=0.9, centered=True)

    a = ParamSet(torch.bfloat16, seed=6)
    opt = make(a.params)
    gen = torch.Generator().manual_seed(106)
    for _ in range(3):
        a.write_grads(a.draw_grads(gen, scale=3.0, shift=1.0))
        opt.step()
    sd = opt.state_dict()
    saved = {k: v.clone() for k, v in _tensor_state(opt).items()}
    if kind == "adam":
        assert any(k[1] == "step_t" for k in saved)

    b = ParamSet(torch.bfloat16, seed=6)
    for p, q in zip(a.params, b.params):
        q.data.copy_(p.data)
    opt2 = make(b.params)
    opt2.load_state_dict(sd)
    loaded = _tensor_state(opt2)
    assert loaded.keys() == saved.keys()
    for k, v in loaded.items():
        assert v.dtype == torch.float32, (k, v.dtype)
        assert v.is_cuda, k
        assert v.numel() == 0 or v.data_ptr() != _tensor_state(opt)[k].data_ptr(), k
        assert torch.equal(v, saved[k]), k
    assert opt2._mt_cache == {}

    grads = a.draw_grads(gen, scale=3.0, shift=1.0)
    a.write_grads(grads)
    b.write_grads(grads)
    opt.step()
    opt2.step()
    assert len(opt2._mt_cache) == 1, "multi-tensor path not taken"
    for i, (p, q) in enumerate(zip(a.params, b.params)):
        assert torch.equal(p, q), i
    after, after2 = _tensor_state(opt), _tensor_state(opt2)
    for k in after:
        assert after2[k].dtype == torch.float32 and torch.equal(after[k], after2[k]), k
    a.assert_guards()
    b.assert_guards()


@requires_gpu
@pytest.mark.parametrize("kind", ["adam", "rmsprop_tf"])
def test_non_fp32_state_is_refused(kind):
    """State that is not float32 must stop step() before any launch.  The
    bf16 state here is a view of an fp32-sized buffer, so it is float-sized
    in memory whatever happens."""
    from sheeprl_amd.optim import FusedAdam, RMSpropTF

    ps = ParamSet(torch.bfloat16, seed=16, sizes=(257, 4097), conv=False, empty=False)
    opt = FusedAdam(ps.params, lr=1e-2) if kind == "adam" else RMSpropTF(ps.params, lr=1e-2)
    gen = torch.Generator().manual_seed(116)
    ps.write_grads(ps.draw_grads(gen))
    opt.step()
    key = "exp_avg_sq" if kind == "adam" else "square_avg"
    st = opt.state[ps.params[1]]
    n = st[key].numel()
    st[key] = torch.zeros(n, dtype=torch.float32, device="cuda").view(torch.bfloat16)[:n]
    before = ps.flat_p.clone()
    ps.write_grads(ps.draw_grads(gen))
    with pytest.raises(RuntimeError, match="float32"):
        opt.step()
    assert torch.equal(ps.flat_p, before), "a kernel ran before the check"


# ---------------------------------------------------------------------------
# 6. RMSpropTF multi-tensor
# ---------------------------------------------------------------------------


class _RMSpropTF64:
    """float64 transcription of RMSpropTF's formulas: square_avg starts at
    ones, v <- rho v + (1-rho) g^2, centered subtracts the squared running
    mean of g, eps sits INSIDE the sqrt, momentum accumulates g / avg."""

    def __init__(self, params, lr, alpha, eps, weight_decay, momentum, centered):
        self.params = params
        self.lr, self.alpha, self.eps, self.wd = lr, alpha, eps, weight_decay
        self.momentum, self.centered = momentum, centered
        self.sq = [torch.ones_like(p.data) for p in params]
        self.ga = [torch.zeros_like(p.data) for p in params]
        self.mb = [torch.zeros_like(p.data) for p in params]

    @torch.no_grad()
    def step(self):
        for i, p in enumerate(self.params):
            g = p.grad
            if self.wd != 0:
                g = g + self.wd * p.data
            self.sq[i] = self.alpha * self.sq[i] + (1 - self.alpha) * g * g
            if self.centered:
                self.ga[i] = self.alpha * self.ga[i] + (1 - self.alpha) * g
                avg = (self.sq[i] - self.ga[i] ** 2 + self.eps).sqrt()
            else:
                avg = (self.sq[i] + self.eps).sqrt()
            if self.momentum > 0:
                self.mb[i] = self.momentum * self.mb[i] + g / avg
                p.data -= self.lr * self.mb[i]
            else:
                p.data -= self.lr * g / avg


@requires_gpu
@pytest.mark.parametrize("weight_decay", [0.0, 1e-3])
@pytest.mark.parametrize("momentum,centered", [(0.0, False), (0.9, False), (0.9, True)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rmsprop_tf_multi_tensor(dtype, momentum, centered, weight_decay):
    from sheeprl_amd.optim import RMSpropTF

    ps = ParamSet(dtype, seed=7)
    refs = ps.clones64()
    hyper = dict(lr=1e-2, alpha=0.9, eps=1e-10, weight_decay=weight_decay, momentum=momentum, centered=centered)
    opt = RMSpropTF(ps.params, **hyper)
    ref = _RMSpropTF64(refs, **hyper)
    budget = _UlpBudget(refs)
    gen = torch.Generator().manual_seed(107)
    for step in range(1, 7):
        # centered: avg^2 = s - a^2 cancels when a gradient keeps one value;
        # randn * 3 + 1 keeps the running variance well away from 0
        ps.write_grads(ps.draw_grads(gen, scale=3.0, shift=1.0), refs)
        opt.step()
        ref.step()
        assert len(opt._mt_cache) == 1, "multi-tensor path not taken"
        if dtype is torch.bfloat16:
            _round_bf16_(refs)
        _check_params(ps.params, refs, dtype, budget, step)
        if dtype is torch.float32 or weight_decay == 0.0:
            for i, p in enumerate(ps.params):
                st = opt.state[p]
                _close(st["square_avg"], ref.sq[i], 1e-5, 1e-6, (step, "square_avg", i))
                if centered:
                    _close(st["grad_avg"], ref.ga[i], 1e-5, 1e-6, (step, "grad_avg", i))
                if momentum > 0:
                    _close(st["momentum_buffer"], ref.mb[i], 1e-5, 1e-6, (step, "momentum_buffer", i))
        ps.assert_guards()


# ---------------------------------------------------------------------------
# 7. gradient-norm clip
# ---------------------------------------------------------------------------


def _runtime():
    from sheeprl_amd.parallel import Runtime

    return Runtime.__new__(Runtime)  # clipping needs no process-group state


def _exact_norm(grads):
    """sqrt of the exact integer sum of squares, in float64."""
    return float(sum(int((g.double() ** 2).sum().item()) for g in grads if g is not None)) ** 0.5


def _check_clip(rt, opt, ps, grads, max_norm, dtype, absent=()):
    """One clip call over integer-valued gradients already written to ps."""
    present = [None if i in absent else g for i, g in enumerate(grads)]
    norm = _exact_norm(present)
    # gradients in [-8, 8] over < 2^18 elements: every partial sum of squares
    # is an integer below 2^24, exact in fp32 in any order
    assert norm**2 < 2**24
    before = ps.flat_g.clone()
    got = rt.clip_gradients(None, opt, max_norm=max_norm)
    assert id(opt) in rt._clip_cache, "fused clip path not taken"
    assert got.dtype == torch.float32
    assert abs(float(got.item()) - norm) <= 2.4e-7 * norm, (float(got.item()), norm)
    if max_norm > norm:
        assert torch.equal(ps.flat_g, before)
    for i, (p, g) in enumerate(zip(ps.params, grads)):
        if i in absent:
            assert p.grad is None
            continue
        ref = g.double() * min(1.0, max_norm / (norm + 1e-6))
        out = p.grad.detach().cpu().double()
        if max_norm > norm:
            assert torch.equal(out, g.double()), i
        elif dtype is torch.float32:
            assert bool(((out - ref).abs() <= 1e-6 * ref.abs()).all()), (i, float((out - ref).abs().max()))
        else:
            ulp = _bf16_ulp(torch.maximum(out.abs(), ref.abs()))
            assert bool(((out - ref).abs() <= ulp).all()), (i, float((out - ref).abs().max()))
    ps.assert_guards()
    return norm


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_clip_grad_norm_exact(dtype):
    from sheeprl_amd.optim import FusedAdam

    rt = _runtime()
    ps = ParamSet(dtype, seed=8)
    opt = FusedAdam(ps.params, lr=0.0)
    gen = torch.Generator().manual_seed(108)

    grads = ps.draw_grads(gen, integer=8)
    ps.write_grads(grads)
    norm = _check_clip(rt, opt, ps, grads, 2.0 * _exact_norm(grads), dtype)  # above: untouched
    table = rt._clip_cache[id(opt)]
    # second call, other max_norm, same table: now below the norm
    _check_clip(rt, opt, ps, grads, norm / 3.0, dtype)
    assert rt._clip_cache[id(opt)] is table

    # a gradient pointer changes between calls
    grads = ps.draw_grads(gen, integer=8)
    ps.write_grads(grads)
    ps.params[5].grad = grads[5].cuda().clone()
    _check_clip(rt, opt, ps, grads, 0.5, dtype)
    assert rt._clip_cache[id(opt)] is not table, "stale chunk table reused"

    # some gradients missing
    grads = ps.draw_grads(gen, integer=8)
    ps.write_grads(grads)
    absent = (0, 6)
    for i in absent:
        ps.params[i].grad = None
    _check_clip(rt, opt, ps, grads, 1.0, dtype, absent=absent)

    # all-zero gradients: norm 0, nothing scaled (no 0/0)
    zeros = [torch.zeros_like(g) for g in grads]
    ps.write_grads(zeros, skip=absent)
    got = rt.clip_gradients(None, opt, max_norm=1.0)
    assert float(got.item()) == 0.0
    for i, p in enumerate(ps.params):
        if i not in absent:
            assert int(p.grad.count_nonzero()) == 0 and bool(torch.isfinite(p.grad).all())
    ps.assert_guards()


@requires_gpu
def test_clip_grad_norm_two_optimizers_one_runtime():
    from sheeprl_amd.optim import FusedAdam

    rt = _runtime()
    a = ParamSet(torch.float32, seed=9)
    b = ParamSet(torch.float32, seed=10, sizes=(4097, 300), conv=False, empty=False)
    oa, ob = FusedAdam(a.params, lr=0.0), FusedAdam(b.params, lr=0.0)
    gen = torch.Generator().manual_seed(109)
    for _ in range(2):
        ga, gb = a.draw_grads(gen, integer=8), b.draw_grads(gen, integer=8)
        a.write_grads(ga)
        b.write_grads(gb)
        _check_clip(rt, oa, a, ga, 3.0, torch.float32)
        _check_clip(rt, ob, b, gb, 2.0, torch.float32)
        b.assert_guards()
        a.assert_guards()
    assert rt._clip_cache[id(oa)] is not rt._clip_cache[id(ob)]


@requires_gpu
def test_clip_grad_norm_mixed_dtypes_falls_back():
    """fp32 and bf16 gradients together are not the kernel's case: torch's
    clip_grad_norm_ runs instead.  It returns each bf16 tensor's norm in bf16
    (half an ulp, 2^-9, each), so the total is within 2^-8 of exact; the
    scaled gradients add bf16 roundings (2^-9 each) of the coefficient and of
    the product to that: 2^-7 in all."""
    from sheeprl_amd.optim import FusedAdam

    rt = _runtime()
    gen = torch.Generator().manual_seed(110)
    ps = [torch.nn.Parameter(torch.zeros(n, device="cuda", dtype=dt))
          for n, dt in ((4097, torch.float32), (300, torch.bfloat16), (5000, torch.bfloat16))]
    grads = [torch.randint(-8, 9, p.shape, generator=gen).float() for p in ps]
    for p, g in zip(ps, grads):
        p.grad = g.to(p.dtype).cuda()
    opt = FusedAdam(ps, lr=0.0)
    norm = _exact_norm(grads)
    max_norm = norm / 4.0
    got = rt.clip_gradients(None, opt, max_norm=max_norm)
    assert id(opt) not in getattr(rt, "_clip_cache", {})
    assert abs(float(got) - norm) <= 2.0**-8 * norm
    for p, g in zip(ps, grads):
        ref = g.double() * max_norm / (norm + 1e-6)
        out = p.grad.cpu().double()
        assert bool(((out - ref).abs() <= 2.0**-7 * ref.abs()).all())


# ---------------------------------------------------------------------------
# 8. EMA
# ---------------------------------------------------------------------------

EMA_SIZES = (1, 257, 4097, 2048 * 256 + 5)  # the last one exceeds the 2048-block grid cap


@pytest.fixture
def ema_kernel_calls(monkeypatch):
    """Number of tensors handed to the ema_update kernel launcher, per call."""
    from sheeprl_amd.ops._ext import require_ext

    ext = require_ext()
    calls = []
    real = ext.ema_update

    def spy(tgts, srcs, tau):
        calls.append(len(tgts))
        return real(tgts, srcs, tau)

    monkeypatch.setattr(ext, "ema_update", spy)
    return calls


@requires_gpu
@pytest.mark.parametrize("tau", [0.0, 0.02, 1.0])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ema_update(dtype, tau, ema_kernel_calls):
    gen = torch.Generator().manual_seed(111)
    # |x| <= 4: three fp32 roundings of values below 4 (2.4e-7 each at most)
    # plus the rounding of (1 - tau) stay under the project's atol of 1e-6
    t = [torch.randn(n, generator=gen).clamp_(-4, 4).to(dtype) for n in EMA_SIZES]
    s = [torch.randn(n, generator=gen).clamp_(-4, 4).to(dtype) for n in EMA_SIZES]
    tg = [x.cuda() for x in t]
    sg = [x.cuda() for x in s]
    ops.ema_update_(tg, sg, tau)
    assert ema_kernel_calls == [len(EMA_SIZES)], "kernel path not taken"
    for i, (a, b, got, src_after) in enumerate(zip(t, s, tg, sg)):
        ref = (1.0 - tau) * a.double() + tau * b.double()
        out = got.cpu().double()
        if dtype is torch.float32:
            assert bool(((out - ref).abs() <= 1e-6).all()), (i, float((out - ref).abs().max()))
        else:
            # one bf16 ulp of the result, plus the fp32 error of the two
            # products and the sum (2^-24 each, and as much for the rounded
            # tau and 1 - tau), which is all that is left where they cancel
            bound = _bf16_ulp(torch.maximum(out.abs(), ref.abs())) + 2.0**-22 * (a.double().abs() + b.double().abs())
            assert bool(((out - ref).abs() <= bound).all()), (i, float(((out - ref).abs() - bound).max()))
        assert torch.equal(src_after.cpu(), b), "source modified"


@requires_gpu
def test_ema_update_strided_views(ema_kernel_calls):
    """Equal but non-dense strides on both sides: the flat kernel would walk
    numel elements from data_ptr and hit the skipped columns."""
    gen = torch.Generator().manual_seed(112)
    tb = torch.randn(6, 10, generator=gen)
    sb = torch.randn(6, 10, generator=gen)
    tg, sg = tb.cuda(), sb.cuda()
    t, s = tg[:, ::2], sg[:, ::2]
    assert t.stride() == s.stride() and not t.is_contiguous()
    ops.ema_update_([t], [s], 0.25)
    assert ema_kernel_calls == [], "flat kernel launched on non-dense views"
    ref = 0.75 * tb[:, ::2].double() + 0.25 * sb[:, ::2].double()
    out = tg.cpu()
    assert bool(((out[:, ::2].double() - ref).abs() <= 1e-6).all())
    assert torch.equal(out[:, 1::2], tb[:, 1::2]), "skipped elements written"
    assert torch.equal(sg.cpu(), sb)


@requires_gpu
def test_ema_update_mixed_dtype_pair(ema_kernel_calls):
    """fp32 target, bf16 source: the kernel reads both sides as the target's
    dtype, so this pair must take the strided path."""
    gen = torch.Generator().manual_seed(113)
    t = torch.randn(4097, generator=gen).clamp_(-4, 4)
    s = torch.randn(4097, generator=gen).clamp_(-4, 4).to(torch.bfloat16)
    tg, sg = t.cuda(), s.cuda()
    ops.ema_update_([tg], [sg], 0.02)
    assert ema_kernel_calls == [], "kernel launched on a mixed-dtype pair"
    ref = 0.98 * t.double() + 0.02 * s.double()
    assert tg.dtype == torch.float32
    assert bool(((tg.cpu().double() - ref).abs() <= 1e-6).all())


# ---------------------------------------------------------------------------
# 9. channels-last bias sum
# ---------------------------------------------------------------------------

CHLAST_SHAPES = [
    (2, 1, 3, 5),
    (2, 3, 3, 5),
    (1, 96, 4, 4),
    (2, 257, 2, 3),  # C above the block size
    (4, 3, 256, 256),  # grid cap reached, C does not divide gridDim * blockDim
    (3, 5, 1, 1),
]


def _chlast_grad(shape, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    g = torch.randint(-4, 5, shape, generator=gen).to(dtype)
    # |g| <= 4 over at most 2^18 rows: every partial sum is an integer < 2^24
    assert 4 * g.numel() // shape[1] < 2**24
    return g, g.double().sum((0, 2, 3))


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", CHLAST_SHAPES)
def test_chlast_bias_sum_exact(shape, dtype):
    from sheeprl_amd.ops._ext import require_ext

    g, ref = _chlast_grad(shape, dtype, 114)
    gg = g.cuda().contiguous(memory_format=torch.channels_last)
    out = require_ext().chlast_bias_sum(gg, shape[1])
    assert out.dtype == torch.float32 and out.shape == (shape[1],)
    assert torch.equal(out.cpu().double(), ref)


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", CHLAST_SHAPES)
def test_chlast_bias_sum_through_conv_backward(shape, dtype, monkeypatch):
    from sheeprl_amd.models.models import FastBiasConv2d
    from sheeprl_amd.ops._ext import require_ext

    ext = require_ext()
    calls = []
    real = ext.chlast_bias_sum

    def spy(g, C):
        calls.append(tuple(g.shape))
        return real(g, C)

    monkeypatch.setattr(ext, "chlast_bias_sum", spy)
    N, C, H, W = shape
    conv = FastBiasConv2d(1, C, 1).to(device="cuda", dtype=dtype)
    conv.weight.requires_grad_(False)  # only the bias gradient is under test
    x = torch.zeros(N, 1, H, W, device="cuda", dtype=dtype).contiguous(memory_format=torch.channels_last)
    y = conv(x)
    g, ref = _chlast_grad(shape, dtype, 115)
    y.backward(g.cuda().contiguous(memory_format=torch.channels_last))
    assert calls == [shape], "bias gradient did not go through chlast_bias_sum"
    assert conv.bias.grad.dtype == dtype
    # the fp32 sum is exact, so the bias gradient is the exact sum rounded once
    assert torch.equal(conv.bias.grad.cpu(), ref.to(dtype))


# ---------------------------------------------------------------------------
# 10. observation normalise
# ---------------------------------------------------------------------------

OBS_SIZES = (1, 3, 5, 6, 7, 4096 + 1, 2048 * 256 * 4 + 7)  # the last one exceeds the grid cap


def _bytes(n):
    # every residue mod 256 appears once n >= 256 (37 is odd)
    return ((torch.arange(n) * 37 + 11) % 256).to(torch.uint8)


@requires_gpu
@pytest.mark.parametrize("n", OBS_SIZES)
def test_obs_norm(n):
    x = _bytes(n)
    if n >= 256:
        assert x.unique().numel() == 256
    xg = x.cuda()
    assert xg.data_ptr() % 4 == 0
    got = ops.normalize_obs(xg)
    assert got.dtype == torch.float32 and got.shape == x.shape
    ref = x.double() / 255 - 0.5
    # 2 fp32 ulps at 0.5
    assert bool(((got.cpu().double() - ref).abs() <= 1.2e-7).all())
    assert torch.equal(xg.cpu(), x)


@requires_gpu
@pytest.mark.parametrize("n", [7, 4096 + 1])
def test_obs_norm_unaligned_view(n):
    """buf[1:] is contiguous but starts at an odd address: no uchar4 loads."""
    buf = _bytes(n + 1).cuda()
    x = buf[1:]
    assert x.is_contiguous() and x.data_ptr() % 4 != 0
    got = ops.normalize_obs(x)
    ref = _bytes(n + 1)[1:].double() / 255 - 0.5
    assert bool(((got.cpu().double() - ref).abs() <= 1.2e-7).all())
