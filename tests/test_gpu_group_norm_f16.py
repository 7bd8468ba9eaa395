"""GroupNorm (+ fused ReLU) per row range on fp16 matrices through the C ABI (csrc/ln_norm.hip: ln_group_norm_forward_segments_f16 /
_backward_segments_f16) against fp64 (`pytest -m gpu`).  There is no fp16 call over the whole matrix: here the whole matrix is the one
range [0, m], which blocks its rows as the whole-matrix kernels do, so the shapes below reach the same edges of the mapping.

Reference: the fp64 GroupNorm of tests/dense_reference.py on the fp16 inputs converted exactly to fp64.  Bounds, derived: an fp16 kernel
is the fp32 kernel between an exact conversion on load and one round-to-nearest-even on store, so for every element of y and grad_x

    |out16 - ref64| <= B32 + 2^-11 (|ref64| + B32) + 2^-25

with B32 the bound dense_reference gives the fp32 kernel for that element, the second term one fp16 rounding of a normal number (the
fp32 result lies within B32 of ref64) and the third half the fp16 subnormal spacing.  mean, rstd, scale, shift, grad_gamma and grad_beta
are never stored in fp16: the fp32 bounds, unchanged.  By construction, and asserted bit for bit: mean_rstd, scale_shift, grad_gamma and
grad_beta are those of the fp32 entry point on x.float() / grad_y.float(), and y / grad_x its outputs rounded with .half().  The ReLU mask
of the backward is x a + b > 0 in fp32 (dense_reference.gn_apply_fp32), not y16 > 0: a positive value below 2^-25 is stored as 0 and
still passes its gradient.  Each test prints its worst error / bound ratios (`pytest -s`); nothing is asserted on those figures."""
import numpy as np
import pytest
import torch

from tests import cloud_batch_reference as B
from tests import dense_reference as R

pytestmark = pytest.mark.gpu

EPS16 = 2.0 ** -11
HALF_SUBNORMAL = 2.0 ** -25
SENTINEL = 777.0  # (exact in fp16)
GUARD = 64
ERR_ARG, ERR_UNSUPPORTED = -1, -2
# rows_per_pass = 256 / (C / 4), a slab is 16 rows_per_pass rows: a single row; fewer rows than one pass; two slabs at the widest pass;
# two general cases; one row per pass and several slabs
SHAPES = [(1, 8), (3, 64), (4100, 4), (400, 32), (700, 64), (40, 1024)]


def dev():
    return torch.device("cuda", 0)


def gpu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def f16_bound(ref, b32):
    ref, b32 = np.abs(R.f64(ref)), R.f64(b32)
    return b32 + EPS16 * (ref + b32) + HALF_SUBNORMAL


def half_input(m, c, mean, std, seed):
    """mean + std N(0, 1) rounded to fp16 (the input IS the fp16 number), |values| < 6e4."""
    x = R.gn_input(m, c, mean, std, seed).astype(np.float16)
    assert np.isfinite(x).all() and float(np.abs(x.astype(np.float64)).max()) < 6e4
    return x


def buf(n, dtype, offset=0):
    """(whole allocation, the n elements `offset` elements behind its start), everything the sentinel."""
    whole = torch.full((offset + n + GUARD,), SENTINEL, dtype=dtype, device=dev())
    return whole, whole[offset:offset + n]


def call(x, gy, gamma, beta, groups, eps, relu, rows=None, starts=None, half=True, offset=0, dirty_ws=True):
    """One forward + backward pair through the C ABI on sentinel-guarded buffers (its own zero fill: next_workspace NULL).  x, gy: fp16
    NumPy arrays; half=False runs the fp32 entry points on the same numbers.  `starts` None: the one range [0, m], its statistics
    returned without the range axis.  `offset`: the matrices start that many ELEMENTS behind an allocation's start.  Returns NumPy
    outputs; asserts every sentinel behind an output and behind the workspace."""
    from lattice_net_amd import _lib
    lib, p = _lib.load(), _lib.ptr
    m, c = x.shape
    dtype = torch.float16 if half else torch.float32
    whole = starts is None
    starts = [0, m] if whole else starts
    segs = len(starts) - 1
    keep = []

    def mat(a):
        alloc, view = buf(m * c, dtype, offset)
        view.copy_(gpu(a).to(dtype).reshape(-1))
        keep.append(alloc)
        return view

    xd, gd = mat(x), mat(gy)
    (y_all, y), (dx_all, dx) = buf(m * c, dtype, offset), buf(m * c, dtype, offset)
    (mr_all, mr), (ss_all, ss) = buf(segs * 2 * groups, torch.float32), buf(segs * 2 * c, torch.float32)
    (dg_all, dg), (db_all, db) = buf(c, torch.float32), buf(c, torch.float32)
    w, b = gpu(gamma), gpu(beta)
    nbytes = int(lib.ln_group_norm_segments_workspace_bytes(c, segs))
    ws = torch.full((nbytes // 8 + 8,), 5.0 if dirty_ws else 0.0, dtype=torch.float64, device=dev())
    ws[nbytes // 8:] = 5.0
    rows_dev = None if rows is None else torch.tensor([rows], dtype=torch.int32, device=dev())
    stream = _lib.stream_ptr(dev())
    sfx = "_f16" if half else ""
    sd = torch.tensor([int(v) for v in starts], dtype=torch.int32, device=dev())
    keep.append(sd)
    fwd, bwd, tail = getattr(lib, "ln_group_norm_forward_segments" + sfx), getattr(lib, "ln_group_norm_backward_segments" + sfx), (p(sd), segs, stream)
    _lib.check(fwd(p(xd), p(w), p(b), m, c, groups, float(eps), int(relu), p(y), p(mr), p(ss), p(ws), nbytes, None, 0, p(rows_dev), *tail), "forward")
    _lib.check(bwd(p(xd), p(gd), p(w), p(mr), p(ss), m, c, groups, int(relu), p(dx), p(dg) if w is not None else None,
                   p(db) if b is not None else None, p(ws), nbytes, None, 0, p(rows_dev), *tail), "backward")
    torch.cuda.synchronize()
    for name, alloc, n, off in (("y", y_all, m * c, offset), ("grad_x", dx_all, m * c, offset), ("mean_rstd", mr_all, mr.numel(), 0),
                                ("scale_shift", ss_all, ss.numel(), 0), ("grad_gamma", dg_all, c, 0), ("grad_beta", db_all, c, 0)):
        assert bool((alloc[off + n:] == SENTINEL).all()) and bool((alloc[:off] == SENTINEL).all()), f"{name}: a sentinel next to the output was overwritten"
    assert bool((ws[nbytes // 8:] == 5.0).all()), "the workspace was written behind its size"
    out = {"y": y.view(m, c), "grad_x": dx.view(m, c), "mean_rstd": mr if whole else mr.view(segs, -1), "scale_shift": ss if whole else ss.view(segs, -1)}
    if w is not None:
        out["grad_gamma"] = dg
    if b is not None:
        out["grad_beta"] = db
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def assert_same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    bad = bits(a) != bits(b)
    assert not bad.any(), f"{what}: {int(bad.sum())} elements differ bit for bit, first {tuple(np.argwhere(bad)[0])}"


def assert_is_the_fp32_call_rounded(got16, got32, what):
    """The by-construction half of the contract: the statistics and parameter gradients of the fp32 call, its y / grad_x rounded once."""
    for k in got16:
        if k in ("y", "grad_x"):
            assert got16[k].dtype == np.float16
            assert_same_bits(got16[k], gpu(got32[k]).half().cpu().numpy(), f"{what} {k} against the fp32 call rounded")
        else:
            assert_same_bits(got16[k], got32[k], f"{what} {k} against the fp32 call")


def check_rows(got, x, gy, gamma, beta, groups, eps, relu, rows, what):
    """One range (or the whole matrix) of an fp16 call against fp64.  Returns worst error / bound per output."""
    m, c = x.shape
    live = m if rows is None else max(0, min(int(rows), m))
    x32 = x.astype(np.float32)
    ratios = {"rstd": R.assert_gn_statistics(got["mean_rstd"], x, groups, eps, rows, what)}
    R.assert_gn_scale_shift(got["scale_shift"], got["mean_rstd"], gamma, beta, c, groups, what)
    ss = R.f64(got["scale_shift"]).reshape(2, c)
    y32 = R.gn_apply_fp32(x32, got["scale_shift"], relu, rows)  # (bit for bit what the fp32 kernel holds before the store)
    y = R.f64(got["y"])
    assert not y[live:].any(), f"{what}: y is not zero behind row {live}"
    ref = R.f64(x)[:live] * ss[0] + ss[1]
    b32 = 3 * R.EPS32 * (np.abs(R.f64(x)[:live] * ss[0]) + np.abs(ss[1]))
    if relu:
        assert not y[:live][y32[:live] == 0].any(), f"{what}: y is not zero where x a + b <= 0 in fp32"
        ref = np.where(y32[:live] == 0, 0.0, ref)
    bound = f16_bound(ref, b32)
    R.assert_within(y[:live], ref, bound, f"{what} y")
    ratios["y"] = R.worst_ratio(y[:live], ref, bound)
    mask = (y32 > 0) if relu else None
    refs, bounds = R.gn_backward_reference(x, gy, mask, gamma, got["mean_rstd"], groups, rows)
    assert not got["grad_x"][live:].any(), f"{what}: grad_x is not zero behind row {live}"
    for name, r_, b_ in zip(("grad_x", "grad_gamma", "grad_beta"), refs, bounds):
        if name in got:
            b_ = f16_bound(r_, b_) if name == "grad_x" else b_
            R.assert_within(got[name], r_, b_, f"{what} {name}")
            ratios[name] = R.worst_ratio(got[name], r_, b_)
    return ratios


def merge(worst, ratios):
    worst.update({k: max(v, worst.get(k, 0.0)) for k, v in ratios.items()})


def groups_of(c):
    return sorted({1, B.module_groups(c), c})


# (|mean| / std up to 30; the widest keeps below 6e4)
FAMILIES = ((0.0, 1.0), (60.0, 2.0), (-3000.0, 100.0))


@pytest.mark.parametrize("m,c", SHAPES, ids=[f"{m}x{c}" for m, c in SHAPES])
def test_rows_against_fp64_and_the_fp32_call(m, c):
    worst = {}
    for k, groups in enumerate(groups_of(c)):
        mean, std = FAMILIES[k % len(FAMILIES)]
        x, gy = half_input(m, c, mean, std, 3 * c + k), half_input(m, c, 0.0, 1.0, 5 * c + k)
        gamma, beta = R.gn_params(c, True, c + k)
        for relu in (False, True):
            for with_beta in (True, False):
                bt = beta if with_beta else None
                what = f"[{m}, {c}] groups={groups} relu={relu} beta={with_beta}"
                got = call(x, gy, gamma, bt, groups, 1e-5, relu)
                merge(worst, check_rows(got, x, gy, gamma, bt, groups, 1e-5, relu, None, what))
                assert_is_the_fp32_call_rounded(got, call(x, gy, gamma, bt, groups, 1e-5, relu, half=False), what)
    print(f"GroupNorm fp16 [{m}, {c}]: worst error / bound {worst}")


@pytest.mark.parametrize("m,c,groups", [(4100, 4, 1), (400, 32, 16), (40, 1024, 32)])
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
def test_rows_exact(m, c, groups, relu):
    """Small integers (dense_reference.gn_exact_*; an even number of elements per group, eps = 0): mean, rstd = 1/2, scale, shift, y and the
    parameter gradients are the integer results bit for bit (every y is a small integer, exact in fp16); grad_x within its bound."""
    x, gy = R.gn_exact_input(m, c, groups).astype(np.float16), R.gn_exact_grad(m, c).astype(np.float16)
    gamma, beta = R.gn_exact_params(c)
    got = call(x, gy, gamma, beta, groups, 0.0, relu)
    cg = c // groups
    mean = (np.arange(groups) % 5 - 2).astype(np.float64)
    R.assert_exact(got["mean_rstd"][:groups], mean, "mean")
    R.assert_exact(got["mean_rstd"][groups:] * 2, np.ones(groups), "2 rstd")
    a = R.f64(gamma) / 2
    b = R.f64(beta) - np.repeat(mean, cg) * a
    R.assert_exact(got["scale_shift"], np.concatenate([a, b]), "scale_shift")
    y_ref = R.f64(x) * a + b
    if relu:
        y_ref = np.maximum(y_ref, 0)
    R.assert_exact(got["y"], y_ref, "y")
    g = R.f64(gy) * ((y_ref > 0) if relu else 1.0)
    R.assert_exact(got["grad_gamma"], (g * (R.f64(x) - np.repeat(mean, cg))).sum(0) / 2, "grad_gamma")
    R.assert_exact(got["grad_beta"], g.sum(0), "grad_beta")
    refs, bounds = R.gn_backward_reference(x, gy, (y_ref > 0) if relu else None, gamma, got["mean_rstd"], groups)
    R.assert_within(got["grad_x"], refs[0], f16_bound(refs[0], bounds[0]), "grad_x")


@pytest.mark.parametrize("rows", [0, 1, 299, 350])
def test_rows_under_a_device_row_count(rows):
    """A [300, 64] tensor of which *rows_dev rows count: the rows from there to 300 are exact zeros in y / grad_x (their x and grad_y are
    large and never read into a sum), the sentinels behind row 300 untouched (asserted in call())."""
    m, c, groups = 300, 64, 32
    live = min(rows, m)
    x, gy = half_input(m, c, 2.0, 1.5, 11), half_input(m, c, 0.0, 1.0, 12)
    x[live:] = np.where(np.arange(c) % 2, -6e4, 6e4).astype(np.float16)
    gy[live:] = np.float16(-5e4)
    gamma, beta = R.gn_params(c, True, 7)
    got = call(x, gy, gamma, beta, groups, 1e-5, True, rows=rows)
    for k, v in got.items():
        assert np.isfinite(v).all(), f"rows_dev={rows}: {k} is not finite"
    if rows == 0:  # the range is empty: zeros everywhere, no statistics written, nothing added to the parameter gradients
        assert not got["y"].any() and not got["grad_x"].any() and not got["grad_gamma"].any() and not got["grad_beta"].any()
        assert (got["mean_rstd"] == SENTINEL).all() and (got["scale_shift"] == SENTINEL).all()
        return
    ratios = check_rows(got, x, gy, gamma, beta, groups, 1e-5, True, rows, f"rows_dev={rows}")
    assert_is_the_fp32_call_rounded(got, call(x, gy, gamma, beta, groups, 1e-5, True, rows=rows, half=False), f"rows_dev={rows}")
    print(f"GroupNorm fp16 rows_dev={rows}: worst error / bound {ratios}")


def test_an_8_byte_aligned_pointer_is_accepted():
    """Matrices 8 bytes (4 fp16 elements) behind a 16-byte boundary: accepted, and the bits of the aligned call."""
    m, c, groups = 400, 32, 32
    x, gy = half_input(m, c, 0.5, 2.0, 1), half_input(m, c, 0.0, 1.0, 2)
    gamma, beta = R.gn_params(c, True, 3)
    base = call(x, gy, gamma, beta, groups, 1e-5, True)
    moved = call(x, gy, gamma, beta, groups, 1e-5, True, offset=4)
    for k in base:
        assert_same_bits(moved[k], base[k], f"8-byte aligned: {k}")
    starts = [0, 1, 1, 150, 400]
    base = call(x, gy, gamma, beta, groups, 1e-5, True, starts=starts)
    moved = call(x, gy, gamma, beta, groups, 1e-5, True, starts=starts, offset=4)
    for k in base:
        live = [0, 2, 3]  # (range 1 is empty: its statistics are whatever the buffer held)
        a, b = (moved[k][live], base[k][live]) if k in ("mean_rstd", "scale_shift") else (moved[k], base[k])
        assert_same_bits(a, b, f"8-byte aligned, ranges: {k}")


def test_refusals_write_nothing():
    """A pointer 2 bytes off, 6 and 1028 channels, groups that do not divide the channels, a short workspace and 65 ranges: each returns
    its code, and no output, statistic or workspace word changes."""
    from lattice_net_amd import _lib
    lib, p = _lib.load(), _lib.ptr
    m = 40
    stream = _lib.stream_ptr(dev())
    starts = torch.arange(0, 66, dtype=torch.int32, device=dev())
    # (channels, groups, element offset of x, workspace bytes short by, ranges, code)
    cases = [(32, 32, 1, 0, 0, ERR_ARG), (6, 3, 0, 0, 0, ERR_UNSUPPORTED), (1028, 4, 0, 0, 0, ERR_UNSUPPORTED), (32, 5, 0, 0, 0, ERR_ARG),
             (32, 32, 0, 8, 0, ERR_ARG), (32, 32, 0, 0, 65, ERR_UNSUPPORTED), (32, 32, 1, 0, 4, ERR_ARG), (32, 32, 0, 8, 4, ERR_ARG)]
    for c, groups, off, short, segs, code in cases:
        n = 80 * 1028
        (x_all, x), (g_all, g) = buf(n, torch.float16, off), buf(n, torch.float16, off)
        (y_all, y), (dx_all, dx) = buf(n, torch.float16, off), buf(n, torch.float16, off)
        stats = [buf(66 * 2 * 1028, torch.float32)[0] for _ in range(2)]
        grads = [buf(1028, torch.float32)[0] for _ in range(2)]
        w = torch.ones((1028,), device=dev())
        segs = segs or 1
        nbytes = int(lib.ln_group_norm_segments_workspace_bytes(min(c, 1024), min(segs, 64)))
        ws = torch.full((nbytes // 8 + 8,), 5.0, dtype=torch.float64, device=dev())
        tail = (p(starts), segs, stream)
        fwd, bwd = lib.ln_group_norm_forward_segments_f16, lib.ln_group_norm_backward_segments_f16
        what = f"channels={c} groups={groups} offset={off} short={short} ranges={segs}"
        rc = fwd(p(x), p(w), p(w), m, c, groups, 1e-5, 1, p(y), p(stats[0]), p(stats[1]), p(ws), nbytes - short, None, 0, None, *tail)
        assert rc == code, (what, "forward", rc, lib.ln_last_error_string())
        rc = bwd(p(x), p(g), p(w), p(stats[0]), p(stats[1]), m, c, groups, 1, p(dx), p(grads[0]), p(grads[1]), p(ws), nbytes - short, None, 0, None, *tail)
        assert rc == code, (what, "backward", rc, lib.ln_last_error_string())
        torch.cuda.synchronize()
        for t in [y_all, dx_all] + stats + grads:
            assert bool((t == SENTINEL).all()), f"{what}: a refused call wrote an output"
        assert bool((ws == 5.0).all()), f"{what}: a refused call wrote the workspace"


def test_two_runs_and_two_graph_replays_are_bitwise_equal():
    from lattice_net_amd import _lib
    lib, p = _lib.load(), _lib.ptr
    m, c, groups = 700, 64, 32
    x, gy = gpu(half_input(m, c, 0.5, 2.0, 21)), gpu(half_input(m, c, 0.0, 1.0, 22))
    gamma, beta = (gpu(v) for v in R.gn_params(c, True, 23))
    starts = {True: torch.tensor([0, 1, 1, 150, 700], dtype=torch.int32, device=dev()), False: torch.tensor([0, 700, 700, 700, 700], dtype=torch.int32, device=dev())}
    nbytes = int(lib.ln_group_norm_segments_workspace_bytes(c, 4))
    outs = {k: torch.zeros(s, dtype=d, device=dev()) for k, s, d in (("y", (m, c), torch.float16), ("dx", (m, c), torch.float16),
                                                                      ("mr", (4, 2 * groups), torch.float32), ("ss", (4, 2 * c), torch.float32),
                                                                      ("dg", (c,), torch.float32), ("db", (c,), torch.float32))}
    ws = torch.zeros((nbytes // 8,), dtype=torch.float64, device=dev())

    def pair(ranged):
        stream = _lib.stream_ptr(dev())
        o = outs
        tail = (p(starts[ranged]), 4, stream)  # (not ranged: the whole matrix as the first of four ranges)
        fwd, bwd = lib.ln_group_norm_forward_segments_f16, lib.ln_group_norm_backward_segments_f16
        _lib.check(fwd(p(x), p(gamma), p(beta), m, c, groups, 1e-5, 1, p(o["y"]), p(o["mr"]), p(o["ss"]), p(ws), nbytes, None, 0, None, *tail), "forward")
        _lib.check(bwd(p(x), p(gy), p(gamma), p(o["mr"]), p(o["ss"]), m, c, groups, 1, p(o["dx"]), p(o["dg"]), p(o["db"]), p(ws), nbytes, None, 0,
                       None, *tail), "backward")

    def snapshot():
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in outs.items()}

    def refill():  # (every run starts from the same buffers: an empty range leaves its statistics as they are)
        for v in outs.values():
            v.fill_(3.0)

    for ranged in (False, True):
        refill()
        pair(ranged)
        first = snapshot()
        refill()
        pair(ranged)
        second = snapshot()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                pair(ranged)
        torch.cuda.synchronize()
        replays = []
        for _ in range(2):
            refill()
            graph.replay()
            replays.append(snapshot())
        for name, other in (("second run", second), ("first replay", replays[0]), ("second replay", replays[1])):
            for k in first:
                assert torch.equal(first[k], other[k]), f"ranged={ranged}: {k} of the {name} differs from the first run"


def many_small_ranges():
    sizes = np.random.default_rng(64).integers(1, 10, size=64)
    return [0] + [int(v) for v in np.cumsum(sizes)]


# (channels, row_starts, tensor height, device row count)
RANGE_CASES = {
    "32-one_row-empty-two_long": (32, [0, 1, 1, 150, 400], 400, None),
    "64-one_row-empty-two_long": (64, [0, 1, 1, 150, 400], 400, None),
    "32-64_ranges_of_1_to_9_rows": (32, many_small_ranges(), many_small_ranges()[-1] + 7, None),
    "64-64_ranges_of_1_to_9_rows": (64, many_small_ranges(), many_small_ranges()[-1] + 7, None),
    "64-device_row_count_below_the_last_range": (64, [0, 1, 1, 150, 400], 400, 260),
}


@pytest.mark.parametrize("case", list(RANGE_CASES))
def test_ranges_are_the_whole_matrix_call_on_their_rows(case):
    """Every range: y, grad_x and mean_rstd bit for bit those of the one-range fp16 call on its rows alone (which the tests above hold to
    fp64); grad_gamma / grad_beta within the summed bounds of the ranges; an empty range leaves its statistics untouched; zeros behind the
    last live row."""
    c, starts, height, rows = RANGE_CASES[case]
    groups = B.module_groups(c)
    x, gy = half_input(height, c, 0.5, 2.0, 31), half_input(height, c, 0.0, 1.0, 32)
    segs, live = B.segments(starts, height, rows)
    for s, (lo, hi) in enumerate(segs):
        x[lo:hi] = (x[lo:hi].astype(np.float32) * np.float32(1 + s % 4) + np.float32(3 * (s % 5) - 4)).astype(np.float16)
    x[live:] = np.where(np.arange(c) % 2, -6e4, 6e4).astype(np.float16)
    gy[live:] = np.float16(-5e4)
    gamma, beta = R.gn_params(c, True, 33)
    got = call(x, gy, gamma, beta, groups, 1e-5, True, rows=rows, starts=starts)
    assert not got["y"][live:].any() and not got["grad_x"][live:].any(), "not zero behind the last live row"
    dg, b_dg, db, b_db = np.zeros(c), np.zeros(c), np.zeros(c), np.zeros(c)
    worst = {}
    for s, (lo, hi) in enumerate(segs):
        if hi == lo:
            assert (got["mean_rstd"][s] == SENTINEL).all() and (got["scale_shift"][s] == SENTINEL).all(), f"range {s} is empty and wrote statistics"
            continue
        alone = call(x[lo:hi], gy[lo:hi], gamma, beta, groups, 1e-5, True)
        for k, a, b in (("y", got["y"][lo:hi], alone["y"]), ("grad_x", got["grad_x"][lo:hi], alone["grad_x"]),
                        ("mean_rstd", got["mean_rstd"][s], alone["mean_rstd"]), ("scale_shift", got["scale_shift"][s], alone["scale_shift"])):
            assert_same_bits(a, b, f"{case} range {s} [{lo}, {hi}) {k}")
        mask = R.gn_apply_fp32(x[lo:hi].astype(np.float32), got["scale_shift"][s], True) > 0
        refs, bounds = R.gn_backward_reference(x[lo:hi], gy[lo:hi], mask, gamma, got["mean_rstd"][s], groups)
        dg, b_dg, db, b_db = dg + refs[1], b_dg + bounds[1], db + refs[2], b_db + bounds[2]
    for name, r_, b_ in (("grad_gamma", dg, b_dg), ("grad_beta", db, b_db)):
        R.assert_within(got[name], r_, b_, f"{case} {name}")
        worst[name] = R.worst_ratio(got[name], r_, b_)
    got32 = call(x, gy, gamma, beta, groups, 1e-5, True, rows=rows, starts=starts, half=False)
    keep = [s for s, (lo, hi) in enumerate(segs) if hi > lo]
    for k in ("mean_rstd", "scale_shift"):
        got[k], got32[k] = got[k][keep], got32[k][keep]
    assert_is_the_fp32_call_rounded(got, got32, case)
    print(f"GroupNorm fp16 ranges {case}: worst error / bound {worst}")
