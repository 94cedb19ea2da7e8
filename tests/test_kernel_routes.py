"""Which kernel a shape takes: the host routing of LayerNorm(+SiLU) and the
GRU gates, asked through ``ln_act_route`` / ``gru_gates_route``.

The route functions touch no device API, so this runs in the CPU suite.  The
table rows are worked out by hand from the dispatch conditions (see
docs/kernels.md), not by calling the function under test; the sweep checks the
preconditions the kernels rely on (alignment, lane counts, row-count gates).
"""

import itertools
from pathlib import Path

import pytest

FEW = 64  # the default few-row limit, passed explicitly so the environment cannot move it
BF16, FP32 = 2, 4


@pytest.fixture(scope="module")
def ext():
    ops_dir = Path(__file__).resolve().parent.parent / "sheeprl_amd" / "ops"
    if not list(ops_dir.glob("_sheep_hip*.so")):
        pytest.skip("extension not built in-tree")
    from sheeprl_amd.ops._ext import require_ext

    return require_ext()


FWD, BWD = (False,), (True,)
BOTH = (False, True)

# (N, D, stride or None for contiguous, itemsize, directions, few_rows, expected (kind, param, cached))
LN_TABLE = [
    # the few-row rule: backward only, and only up to the limit
    (16, 512, None, BF16, BWD, FEW, ("ROW", 0, True)),
    (16, 512, None, BF16, FWD, FEW, ("CL", 64, True)),
    (64, 512, None, BF16, BWD, FEW, ("ROW", 0, True)),
    (65, 512, None, BF16, BWD, FEW, ("CL", 64, False)),
    (16, 512, None, BF16, BWD, 0, ("CL", 64, True)),
    # channels-last lane counts: pow2 and the conv widths 96/192
    (1 << 20, 32, None, BF16, BOTH, FEW, ("CL", 4, False)),
    (4103, 96, None, BF16, BOTH, FEW, ("CL", 12, False)),
    (4103, 192, None, BF16, BOTH, FEW, ("CL", 24, False)),
    # vectorized wave-per-row: K=2 preferred, K=4 when D/(2V) > 64
    (16384, 1024, None, FP32, BOTH, FEW, ("VEC", 4, False)),
    (4096, 640, None, FP32, BOTH, FEW, ("VEC", 4, False)),
    (4096, 768, None, FP32, BOTH, FEW, ("VEC", 4, False)),
    (16384, 1024, None, BF16, BOTH, FEW, ("VEC", 2, False)),
    (4096, 1536, None, BF16, BOTH, FEW, ("VEC", 4, False)),
    (4096, 2048, None, BF16, BOTH, FEW, ("VEC", 4, False)),
    (65, 1536, None, BF16, BOTH, FEW, ("VEC", 4, False)),
    # fp32 at the same widths: D/(4*4) = 96, 128 > 64 lanes -> block per row
    (4096, 1536, None, FP32, BOTH, FEW, ("ROW", 0, False)),
    (4096, 2048, None, FP32, BOTH, FEW, ("ROW", 0, False)),
    (65, 1536, None, FP32, BOTH, FEW, ("ROW", 0, False)),
    # row-strided operands never take CL
    (65, 512, 536, BF16, BOTH, FEW, ("VEC", 2, False)),
    (16, 512, 536, BF16, BOTH, FEW, ("ROW", 0, True)),
    # the forward/backward asymmetry at D <= 256
    (100, 256, 264, FP32, FWD, FEW, ("VEC", 2, False)),
    (100, 256, 264, FP32, BWD, FEW, ("SMALL", 0, False)),
    (16, 256, 264, FP32, BOTH, FEW, ("SMALL", 0, True)),
    (100, 2049, None, FP32, BOTH, FEW, ("ROW", 0, False)),
]

# (N, H, itemsize, directions, expected (kind, C, cached))
GRU_TABLE = [
    (16, 2048, BF16, BOTH, ("WIDE", 16, True)),   # min(512/16, ceil(2048/128)) = min(32, 16)
    (64, 2112, BF16, BOTH, ("WIDE", 8, True)),    # min(512/64, ceil(2112/128)) = min(8, 17)
    (65, 2048, BF16, FWD, ("VEC", 1, False)),
    (65, 2048, BF16, BWD, ("ROW", 1, False)),
    (65, 2049, BF16, FWD, ("ROW", 1, False)),
    (16, 512, BF16, BOTH, ("ROW", 1, True)),
]


@pytest.mark.parametrize("row", LN_TABLE, ids=lambda r: f"N{r[0]}-D{r[1]}-s{r[2]}-i{r[3]}-few{r[5]}")
def test_ln_route_table(ext, row):
    N, D, stride, itemsize, directions, few, want = row
    for backward in directions:
        got = ext.ln_act_route(N, D, D if stride is None else stride, itemsize, backward, few)
        assert tuple(got) == want, (backward, got)


@pytest.mark.parametrize("row", GRU_TABLE, ids=lambda r: f"N{r[0]}-H{r[1]}")
def test_gru_route_table(ext, row):
    N, H, itemsize, directions, want = row
    for backward in directions:
        got = ext.gru_gates_route(N, H, itemsize, backward)
        assert tuple(got) == want, (backward, got)


def test_ln_route_default_few_rows(ext):
    """few_rows omitted means the process-wide limit: 64, or what
    SHEEPRL_AMD_LN_FEW_ROWS said when the process started."""
    import os

    few = int(os.environ.get("SHEEPRL_AMD_LN_FEW_ROWS", FEW))
    for N in (16, 64, 65):
        assert ext.ln_act_route(N, 512, 512, BF16, True) == ext.ln_act_route(N, 512, 512, BF16, True, few)


def test_ln_route_invariants(ext):
    Ns = (1, 16, 64, 65, 300)
    Ds = (31, 32, 64, 96, 256, 264, 512, 640, 1024, 1536, 2048, 2049)
    seen = set()
    for N, D, pad, itemsize, backward in itertools.product(Ns, Ds, (0, 8, 24, 1), (2, 4), BOTH):
        stride = D + pad
        V = 16 // itemsize
        kind, param, cached = ext.ln_act_route(N, D, stride, itemsize, backward, FEW)
        where = (N, D, stride, itemsize, backward, kind, param)
        seen.add(kind)
        assert cached == (N <= 64), where
        if kind == "CL":
            assert stride == D and D == param * V, where
            assert param in (2, 4, 8, 12, 16, 24, 32, 64), where
            assert not (backward and N <= FEW), where
        elif kind == "VEC":
            assert param in (2, 4), where
            assert N > 64 and stride % V == 0, where
            assert D % (param * V) == 0 and D // (param * V) <= 64, where
        elif kind == "SMALL":
            assert D <= 256 and param == 0, where
        else:
            assert kind == "ROW" and param == 0, where
    assert seen == {"CL", "VEC", "SMALL", "ROW"}


def test_gru_route_invariants(ext):
    for N, H, itemsize, backward in itertools.product(
        (1, 16, 64, 65, 300), (200, 512, 2047, 2048, 2112, 4096), (2, 4), BOTH
    ):
        kind, C, cached = ext.gru_gates_route(N, H, itemsize, backward)
        where = (N, H, itemsize, backward, kind, C)
        assert cached == (N <= 64), where
        if kind == "WIDE":
            # every column chunk is non-empty and the grid stays bounded
            assert N <= 64 and H >= 2048 and 1 <= C <= 512 and (C - 1) * -(-H // C) < H, where
        else:
            assert C == 1, where
            if kind == "VEC":
                assert not backward and N > 64 and H % (16 // itemsize) == 0, where
            else:
                assert kind == "ROW", where
