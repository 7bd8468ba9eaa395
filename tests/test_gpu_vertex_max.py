"""The vertex-side maximum of PointNetModule against plain NumPy references, element by element and bit for bit (`pytest -m gpu`):
k_csr_segment_max and its decode, the fused reduction around it (ln_pointnet_reduce_forward / _backward), ln_csr_group_sizes
(csrc/ln_csr.hip) and the centring tail k_distribute_centre (csrc/ln_glue.hip), called through the C ABI.

The segment max keeps its own copy of the run combining of the segment reduce: a segmented suffix maximum over the lane groups of a wave,
an LDS hand-over across the four waves of a workgroup, a "whole row: plain store, else 64-bit atomicMax" decision, a token count on the
same run bookkeeping, and a (value, ~token) packing whose zero word means "no token".  ln_launch_segment_max picks the instance
<VEC, COMB> from the row width and the alignment of the source; the tests are parametrised over this table
(tests/vertex_max_reference.py: DISPATCH, checked against the rule without a GPU):

    <4, true>    4, 8, 32, 64, 256 (aligned source)             4: 64 lane groups per wave; 256: one, only the LDS path combines
    <4, false>   12, 96, 260                                    260: 65 lanes per segment
    <1, true>    1, 2; 8 and 64 with the source offset by one float
    <1, false>   3, 7; 128 offset by one float

over every origin of the CSR (tests/test_gpu_segment_reduce.py: the bucketed build in slot and canonical order, the atomic build, eight kd
regions under both slot orders, ln_csr_build over a synthetic index with rows of 0 .. 4100 tokens), and d = 1 and d = 6 on the slot origin.

These kernels select and copy: every comparison is exact (a zero maximum may carry either sign where the header does not say).  They do
not bound a row id against `rows`, and the synthetic index names rows up to the capacity: every call passes rows = the table's capacity
and buffers of that many rows, with sentinels behind them.

Not held: which value and token an element with a NaN among its own tokens returns (only that the NaN stays in its element), and the
64-bit-index instance of k_distribute_centre_clouds, which needs more than 2^31 elements."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cloud_invalid_vertex_reference as V
from tests import vertex_max_reference as R
from tests.test_gpu_segment_reduce import EDGE_COUNTS, ORIGINS, build_origin, hot_cloud, synthetic_index

pytestmark = pytest.mark.gpu

LN_CSR_SEG = 16          # csrc/ln_csr.h: CSR entries per segment
SENTINEL_BYTE = 0xA5
SENTINEL_INT = -12345  # (no token id, no count, and not the -1 of "no token")
SENTINEL = 777.0
CASES = [case for cases in R.DISPATCH.values() for case in cases]  # (channels, source aligned)
CASE_IDS = [f"c{c}" + ("" if aligned else "off") for c, aligned in CASES]


def dev():
    return torch.device("cuda", 0)


def gpu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(dev()) if dtype is None else t.to(dev(), dtype)


def lib_and_stream():
    from lattice_net_amd import _lib
    return _lib.load(), _lib.stream_ptr(dev())


class Origin:
    """One lattice, the splat indices whose CSR the kernels walk, and what the tests need of both on the host."""

    def __init__(self, name):
        if name == "csr_build":  # (the lattice only lends its capacity to ln_csr_build)
            lat, _ = build_origin("csr_build", hot_cloud(3, seed=3, n_uniform=200, n_dup=5, n_hot=50), 0.5, 6000)
            idx = synthetic_index(6000, seed=1)
        elif name.startswith("slot_d"):
            d = int(name[len("slot_d"):])
            lat, idx = build_origin("slot", hot_cloud(d, seed=d, n_hot=1200), 0.6, 40000)
        else:
            lat, idx = build_origin(name, hot_cloud(3, seed=1), 0.5, 20000)
        self.name, self.lat, self.idx = name, lat, idx
        self.rows = lat.m_hash_table.capacity()  # NOT nr_lattice_vertices(): the kernels do not bound a row id
        self.tokens = idx.numel()
        self.buf, self.csr, self.max_seg, self.grp_row, _ = lat._csr(idx)
        self.groups = lat.m_hash_table._storage.hashed() if self.grp_row is not None else self.rows
        torch.cuda.synchronize()
        self.idx_np = idx.cpu().numpy().astype(np.int64)
        ok = (self.idx_np >= 0) & (self.idx_np < self.rows)
        self.counts = np.bincount(self.idx_np[ok], minlength=self.rows)
        self.hot = int(np.argmax(self.counts))
        # the first CSR segment of the hottest row, read back from the CSR itself
        host = self.buf.cpu().numpy()
        o_grp, o_tok = ((p - self.buf.data_ptr()) // 4 for p in (self.csr.grp_start, self.csr.csr_tok))
        grp_start = host[o_grp:o_grp + self.groups + 1]
        group = self.hot if self.grp_row is None else int(np.flatnonzero(self.grp_row[:self.groups].cpu().numpy() == self.hot)[0])
        beg, end = int(grp_start[group]), int(grp_start[group + 1])
        assert end - beg == self.counts[self.hot], (name, beg, end, self.counts[self.hot])
        self.hot_first_segment = host[o_tok + beg:o_tok + beg + LN_CSR_SEG].astype(np.int64)
        assert (self.idx_np[self.hot_first_segment] == self.hot).all(), name

    def csr_args(self):
        from lattice_net_amd import _lib
        return C.byref(self.csr), _lib.ptr(self.grp_row), self.max_seg


@pytest.fixture(scope="module")
def origins():
    """name -> Origin, built on first use and kept for the module (the references are recomputed per case, the lattices are not)."""
    built = {}

    def get(name):
        if name not in built:
            built[name] = Origin(name)
        return built[name]

    yield get
    built.clear()


def upload_rows(a, aligned=True):
    """[n, c] float32 on the device, its first element on a 16-byte boundary or one float behind one."""
    flat = torch.empty((a.size + 4,), dtype=torch.float32, device=dev())
    off = 0 if aligned else 1
    view = flat[off:off + a.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
    assert view.data_ptr() % 16 == 4 * off
    return view


def same_values(got, ref):
    """bool array: bit for bit, zeros of either sign equal."""
    return (got.view(np.uint32) == ref.view(np.uint32)) | ((got == 0) & (ref == 0))


def assert_same(got, ref, what, exact_zero_sign=False):
    ok = (got.view(np.uint32) == ref.view(np.uint32)) if exact_zero_sign else same_values(got, ref)
    if not ok.all():
        i = tuple(int(v) for v in np.argwhere(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} elements differ, first {i}: got {got[i]!r}, reference {ref[i]!r}")


def assert_same_int(got, ref, what):
    if not np.array_equal(got, ref):
        bad = got != ref
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} elements differ, first {i}: got {int(got[i])}, reference {int(ref[i])}")


def run_segment_max(o, src, c):
    """ln_csr_segment_max over o's CSR into NaN / sentinel pre-filled outputs, sentinel rows behind them and sentinel bytes behind
    packed_ws; one synchronisation."""
    lib, stream = lib_and_stream()
    rows = o.rows
    packed = torch.full((rows * c * 8 + 64,), SENTINEL_BYTE, dtype=torch.uint8, device=dev())
    out = torch.full((rows + 4, c), float("nan"), device=dev())
    arg = torch.full((rows + 4, c), SENTINEL_INT, dtype=torch.int32, device=dev())
    rc = lib.ln_csr_segment_max(*o.csr_args(), src.data_ptr(), c, rows, packed.data_ptr(), out.data_ptr(), arg.data_ptr(), stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.ln_last_error_string()
    out, arg = out.cpu().numpy(), arg.cpu().numpy()
    assert (packed[rows * c * 8:].cpu().numpy() == SENTINEL_BYTE).all(), "bytes behind packed_ws were written"
    assert np.isnan(out[rows:]).all() and (arg[rows:] == SENTINEL_INT).all(), "rows behind the outputs were written"
    assert (arg[:rows] != SENTINEL_INT).all(), "an element of out_arg was not written"
    return out[:rows], arg[:rows]


def ties_source(tokens, c, seed):
    return np.random.default_rng(seed).integers(-3, 4, (tokens, c)).astype(np.float32)


def random_source(tokens, c, seed):
    f = np.random.default_rng(seed).standard_normal((tokens, c)).astype(np.float32)
    f[::3] = np.round(f[::3])
    return f


def hot_winner_outside_first_segment(o, src):
    """bool [c]: the smallest token attaining the hottest row's maximum lies outside that row's first CSR segment."""
    toks = np.flatnonzero(o.idx_np == o.hot)
    x = src[toks]
    win = np.where(x == x.max(0), toks[:, None], R.NO_TOKEN).min(0)
    return ~np.isin(win, o.hot_first_segment)


def check_segment_max(o, c, aligned, seed):
    what = f"{o.name} c={c}{'' if aligned else ' offset'}"
    # ties: nearly every (row, channel) has its maximum several times, in different segments, waves and workgroups of the hot rows.  The
    # order of a row's tokens in the CSR is the build's (atomics): the seed is moved until, for the hottest row, the smallest-token rule
    # across segments is what decides at least one channel
    for attempt in range(64):
        src = ties_source(o.tokens, c, seed + 1000 * attempt)
        if hot_winner_outside_first_segment(o, src).any():
            break
    assert hot_winner_outside_first_segment(o, src).any(), f"{what}: no seed puts a winner of the hottest row outside its first segment"
    assert o.counts[o.hot] > 32 * LN_CSR_SEG  # more than a workgroup's worth of segments at 8 lanes each
    for form, src in (("ties", src), ("random", random_source(o.tokens, c, seed + 1))):
        ref_max, ref_arg, ref_counts = R.segment_max(src, o.idx_np, o.rows)
        assert np.array_equal(ref_counts, o.counts)
        out, arg = run_segment_max(o, upload_rows(src, aligned), c)
        assert not np.isnan(out).any(), f"{what} {form}: an element of out_max was not written"
        assert_same(out, ref_max, f"{what} {form} max")
        assert_same_int(arg, ref_arg, f"{what} {form} arg")


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("origin", ORIGINS)
def test_segment_max_every_instance_every_origin(origins, origin, case):
    c, aligned = case
    assert R.segment_max_instance(c, aligned) in R.DISPATCH
    check_segment_max(origins(origin), c, aligned, seed=100 * ORIGINS.index(origin) + c)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("d", [1, 6])
def test_segment_max_other_dimensions(origins, d, case):
    """The bucketed build of 2 and of 7 tokens per point (slot origin)."""
    c, aligned = case
    check_segment_max(origins(f"slot_d{d}"), c, aligned, seed=7000 + 10 * d + c)


@pytest.mark.parametrize("c", [32, 7])
@pytest.mark.parametrize("origin", ["csr_build", "slot"])
def test_segment_max_special_values(origins, origin, c):
    """Rows of special values among N(0, 1) rows, on the rows with the most tokens (the hottest first): +Inf twice (the smaller token
    wins), only negative values (every packed word is below the one of +0; the 0 word still means "no token"), only -Inf, -0.0 and +0.0
    mixed above negative values (one value: the smallest token of either sign), denormals of both signs and one channel of negative
    denormals only (returned as they are, not flushed).
    NaN isolation: with NaN on half the tokens of one row in one channel, every other (row, channel) element is what it was without.
    What the NaN element itself returns is not specified and not asserted."""
    o = origins(origin)
    rng = np.random.default_rng(c)
    src = rng.standard_normal((o.tokens, c)).astype(np.float32)
    r = [int(v) for v in np.argsort(-o.counts, kind="stable")[:6]]
    assert o.counts[r[-1]] >= 20 and r[0] == o.hot
    toks = [np.flatnonzero(o.idx_np == row) for row in r]
    tiny = np.float32(2.0 ** -149)
    inf_pair = toks[0][[len(toks[0]) // 3, 2 * len(toks[0]) // 3]]
    src[inf_pair] = np.inf
    src[toks[1]] = -np.abs(src[toks[1]]) - np.float32(0.5)
    src[toks[2]] = -np.inf
    src[toks[3]] = np.where(rng.random((toks[3].size, c)) < 0.5, np.where(rng.random((toks[3].size, c)) < 0.5, -0.0, 0.0), -1.5)
    src[toks[3][0]] = -0.0
    src[toks[4]] = rng.integers(-5, 6, (toks[4].size, c)).astype(np.float32) * tiny
    src[toks[4], 0] = -np.abs(src[toks[4], 0]) - tiny
    ref_max, ref_arg, _ = R.segment_max(src, o.idx_np, o.rows)
    # the reference says what the case is meant to say
    assert (ref_max[r[0]] == np.inf).all() and (ref_arg[r[0]] == inf_pair[0]).all()
    assert (ref_max[r[1]] < 0).all() and (ref_max[r[2]] == -np.inf).all() and (ref_arg[r[2]] == toks[2][0]).all()
    assert (ref_max[r[3]] == 0).all() and (ref_arg[r[3]] == toks[3][0]).all()
    assert (ref_max[r[4], 0] < 0).all() and (np.abs(ref_max[r[4]]) <= 5 * 2.0 ** -149).all() and ref_max[r[4]].any()
    out, arg = run_segment_max(o, upload_rows(src), c)
    assert_same(out, ref_max, f"{origin} c={c} special max")
    assert_same_int(arg, ref_arg, f"{origin} c={c} special arg")
    poisoned = src.copy()
    poisoned[toks[5][::2], 1] = np.nan
    out2, arg2 = run_segment_max(o, upload_rows(poisoned), c)
    rest = np.ones((o.rows, c), bool)
    rest[r[5], 1] = False
    assert_same(np.where(rest, out2, 0), np.where(rest, out, 0), f"{origin} c={c} beside the NaN element, max", exact_zero_sign=True)
    assert_same_int(np.where(rest, arg2, 0), np.where(rest, arg, 0), f"{origin} c={c} beside the NaN element, arg")


# ---------------------------------------------------------------------------------------------------------- the fused reduction
@pytest.mark.parametrize("bary_stride", [1, 5])
@pytest.mark.parametrize("min_points", [1, 4, 17])
@pytest.mark.parametrize("c", [4, 12, 32, 5])
@pytest.mark.parametrize("origin", ["atomic", "slot", "regions_space", "csr_build"])
def test_pointnet_reduce_forward_every_instance(origins, origin, c, min_points, bary_stride):
    """out (maxima | barycentric weights of the winners) and out_arg bit for bit against pointnet_reduce; the token counts the segment
    max leaves in the workspace (behind the rows * channels packed words: hot rows add theirs with atomics) against np.bincount; rows of
    15 / 16 / 17 tokens at min_points = 17 dropped, dropped, kept; row 0 dropped whatever its count."""
    o = origins(origin)
    lib, stream = lib_and_stream()
    rows = o.rows
    seed = 1000 * c + 10 * min_points + bary_stride
    src = ties_source(o.tokens, c, seed)
    bary = np.random.default_rng(seed + 1).standard_normal(o.tokens * bary_stride).astype(np.float32)
    need = lib.ln_pointnet_reduce_workspace_bytes(rows, c)
    assert need >= rows * c * 8 + rows * 4
    ws = torch.full((need + 64,), SENTINEL_BYTE, dtype=torch.uint8, device=dev())
    out = torch.full((rows + 4, 2 * c), float("nan"), device=dev())
    arg = torch.full((rows + 4, c), SENTINEL_INT, dtype=torch.int32, device=dev())
    src_t, bary_t = upload_rows(src), gpu(bary)
    rc = lib.ln_pointnet_reduce_forward(*o.csr_args(), src_t.data_ptr(), c, bary_t.data_ptr(), bary_stride, rows, min_points, ws.data_ptr(), need,
                                        out.data_ptr(), arg.data_ptr(), stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.ln_last_error_string()
    ws, out, arg = ws.cpu().numpy(), out.cpu().numpy(), arg.cpu().numpy()
    assert (ws[need:] == SENTINEL_BYTE).all(), "bytes behind the workspace were written"
    assert np.isnan(out[rows:]).all() and (arg[rows:] == SENTINEL_INT).all(), "rows behind the outputs were written"
    out, arg = out[:rows], arg[:rows]
    assert not np.isnan(out).any() and (arg != SENTINEL_INT).all(), "an element of the outputs was not written"
    what = f"{origin} c={c} min_points={min_points} bary_stride={bary_stride}"
    assert_same_int(ws[rows * c * 8:rows * c * 8 + rows * 4].view(np.int32), o.counts, f"{what} counts")
    ref_out, ref_arg, ref_counts = V.pointnet_reduce(src, o.idx_np, bary, rows, min_points, bary_stride=bary_stride)
    assert np.array_equal(ref_counts, o.counts)
    assert_same(out, ref_out, f"{what} out", exact_zero_sign=True)
    assert_same_int(arg, ref_arg, f"{what} arg")
    kept = (o.counts >= min_points) & (o.counts > 0) & (np.arange(rows) != 0)
    assert o.counts[0] >= 17 or origin != "csr_build"
    assert o.counts[0] > 0 and not out[0].any() and (arg[0] == -1).all()
    assert np.array_equal((arg >= 0).all(1), kept) and np.array_equal((arg == -1).all(1), ~kept)
    if origin == "csr_build":
        assert set(EDGE_COUNTS) - {0} <= set(o.counts[1:])
    if origin == "csr_build" and min_points == 17:
        for n, keeps in ((15, False), (16, False), (17, True)):
            at = np.flatnonzero(o.counts == n)
            at = at[at != 0]
            assert at.size and ((arg[at] >= 0).all() if keeps else (arg[at] == -1).all() and not out[at].any()), n


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("double_stride", [False, True], ids=["strideC", "stride2C"])
@pytest.mark.parametrize("c", [32, 5])
def test_pointnet_reduce_backward_every_form(c, double_stride, offset):
    """The vector instance (channels % 4 == 0, aligned), the scalar one (5 channels) and the unaligned fallback (grad_src one float behind
    a 16-byte boundary), at grad_stride = channels and 2 x channels, against pointnet_reduce_backward; every element of a NaN pre-filled
    grad_src is written; the tokens of row 0 and of no row are zero although out_arg names winners on row 0."""
    lib, stream = lib_and_stream()
    rng = np.random.default_rng(10 * c + 2 * double_stride + offset)
    rows, tokens = 300, 5003
    idx = rng.integers(-1, rows, tokens)
    idx[rng.choice(tokens, 40, replace=False)] = 0
    src = ties_source(tokens, c, c)
    _, arg, counts = R.segment_max(src, idx, rows)  # (winners on every row that has tokens, row 0 included)
    arg[counts < 14] = -1                           # dropped rows
    assert (arg[0] >= 0).all() and (arg[1:] == -1).all(1).any()
    stride = 2 * c if double_stride else c
    grad_out = rng.standard_normal(rows * stride).astype(np.float32)
    exp = V.pointnet_reduce_backward(grad_out, arg, idx, tokens, grad_stride=stride)
    assert exp[idx == 0].any()  # the reference formula alone would hand row 0's winners a gradient: the kernel skips idx <= 0
    exp[idx <= 0] = 0
    flat = torch.full((tokens * c + 8,), float("nan"), device=dev())
    off = 1 if offset else 0
    flat[off + tokens * c:] = SENTINEL
    g = flat[off:off + tokens * c]
    assert g.data_ptr() % 16 == 4 * off
    arg_t, idx_t, grad_t = gpu(arg), gpu(idx, torch.int32), gpu(grad_out)
    rc = lib.ln_pointnet_reduce_backward(grad_t.data_ptr(), stride, arg_t.data_ptr(), idx_t.data_ptr(), tokens, c, g.data_ptr(), stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.ln_last_error_string()
    host = flat.cpu().numpy()
    assert (host[off + tokens * c:] == SENTINEL).all() and (off == 0 or np.isnan(host[0])), "elements around grad_src were written"
    got = host[off:off + tokens * c].reshape(tokens, c)
    assert not np.isnan(got).any(), "an element of grad_src was not written"
    assert exp.any() and not got[idx <= 0].any()
    assert_same(got, exp, f"c={c} grad_stride={stride} offset={off}", exact_zero_sign=True)


@pytest.mark.parametrize("origin", ORIGINS)
def test_group_sizes_every_origin(origins, origin):
    o = origins(origin)
    lib, stream = lib_and_stream()
    counts = torch.full((o.rows + 4,), SENTINEL_INT, dtype=torch.int32, device=dev())
    rc = lib.ln_csr_group_sizes(o.csr_args()[0], o.csr_args()[1], o.groups, o.rows, counts.data_ptr(), stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.ln_last_error_string()
    counts = counts.cpu().numpy()
    assert (counts[o.rows:] == SENTINEL_INT).all(), "elements behind counts were written"
    assert_same_int(counts[:o.rows], o.counts, f"{origin} group sizes")
    assert o.counts.max() >= 1200 and (o.counts == 0).any()


@pytest.mark.parametrize("val_dim", [1, 2, 5])
@pytest.mark.parametrize("pos_dim", [1, 2, 3, 6])
def test_distribute_centre_widths(pos_dim, val_dim):
    """k_distribute_centre on rows [position (pos_dim) | values (val_dim) | barycentric weight], a token count whose element count is no
    multiple of the 256 threads of a workgroup; idx of -1, 0 and valid rows, counts with zeros (the max(counts, 1) divisor), sentinel
    rows behind out.  The 64-bit-index instance of k_distribute_centre_clouds needs more than 2^31 elements and stays untested."""
    lib, stream = lib_and_stream()
    width, tokens, rows = pos_dim + val_dim + 1, 1013, 50
    assert (tokens * width) % 256 != 0 and tokens * width > 256
    rng = np.random.default_rng(10 * pos_dim + val_dim)
    idx = rng.integers(-1, rows, tokens)
    d = rng.standard_normal((tokens, width)).astype(np.float32)
    sums = (rng.standard_normal((rows, pos_dim)) * 7).astype(np.float32)
    counts = rng.integers(0, 10, rows)
    counts[[1, 2]] = 0
    idx[:8] = [-1, 0, 1, 2, rows - 1, 1, 0, -1]
    assert (counts[idx[idx > 0]] == 0).any() and (idx == 0).any() and (idx == -1).any()
    out = torch.full((tokens + 4, width), SENTINEL, device=dev())
    d_t, idx_t, sums_t, counts_t = gpu(d), gpu(idx, torch.int32), gpu(sums), gpu(counts, torch.int32)
    rc = lib.ln_distribute_centre(d_t.data_ptr(), idx_t.data_ptr(), sums_t.data_ptr(), counts_t.data_ptr(), tokens, width, pos_dim, out.data_ptr(),
                                  stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.ln_last_error_string()
    out = out.cpu().numpy()
    assert (out[tokens:] == SENTINEL).all(), "rows behind the output were written"
    exp = V.distribute_centre(d, idx, sums, counts, pos_dim)
    assert not exp[idx <= 0].any() and exp[idx > 0].all()
    assert np.array_equal(out[:tokens].view(np.uint32), exp.view(np.uint32))
