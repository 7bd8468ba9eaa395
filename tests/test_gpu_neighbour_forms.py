"""Every form of the neighbour traversal (csrc/ln_neighbours.h) against the exact reference of tests/neighbour_reference.py, entry for entry
(`pytest -m gpu`).  ln_neighbours is called through the C ABI on the tables of lattices built through the Lattice API; the reference is
evaluated on the keys and rows of those very tables (read back from the device), so it holds under every row numbering and slot order.
Every comparison is integer equality: no tolerance anywhere in this file.

Forms (ln_neighbours_body): the same-level integer form at dilations 1, 2, 3, 5; the same-level float form, reached by a coordinate beyond
+-2^22 (d = 1, 2; also with both forms live in one launch) and by a dilation >= 2^18; the kernel's own `flip` argument; the level-crossing
forms (scale 1/2 with its centre and odd-(d+1) rules, scale 2) at dilations 1 and 2; the fused launch behind a splat
(k_reduce_and_neighbours); and the rows between *nr_filled and query_rows_upper, which must read LN_NOT_VISITED."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import neighbour_reference as NR

pytestmark = pytest.mark.gpu
SENTINEL = -77
NOT_VISITED = -2


def dev():
    return torch.device("cuda", 0)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def N(t):
    return t.detach().cpu().numpy()


_LATTICES = {}


def lattice(kind, d, table="hash", order="canonical"):
    """(lattice, keys [m, d], dict key -> row) of a cloud, built once per module.  table "space": the second build over a slot map
    calibrated on the first; order: the row numbering of the build."""
    key = (kind, d, table, order)
    if key not in _LATTICES:
        from lattice_net_amd import Lattice
        from lattice_net_amd import lattice as LL
        pos, sigma = NR.cloud(kind, d)
        prev = LL.set_row_order(order), LL.set_slot_order("space" if table == "space" else "hash")
        try:
            lat = Lattice(sigmas=[sigma] * d, capacity=NR.CAPACITY, device=dev())
            lat.begin_splat()
            idx, _ = lat.just_create_verts(T(pos), True)
            lat.nr_lattice_vertices()
            if table == "space":
                lat.calibrate_regions(idx)
                lat.begin_splat()
                lat.just_create_verts(T(pos), True)
                lat.nr_lattice_vertices()
                st = lat.m_hash_table._storage
                assert st.slot_map is not None and st.row_regions is not None, "the table must be space-ordered"
                assert st.rows_follow_space == (order == "slot")
        finally:
            LL.set_row_order(prev[0])
            LL.set_slot_order(prev[1])
        _LATTICES[key] = with_keys(lat)
    return _LATTICES[key]


def with_keys(lat):
    m = lat.nr_lattice_vertices()
    assert int(N(lat.m_hash_table._counters)[1]) == 0, "the build reported a status bit"
    keys = N(lat.m_hash_table.m_keys_tensor)[:m].copy()
    td = NR.table_dict(keys)
    assert len(td) == m, "every row of the table has its own key"
    return lat, keys, td


def run(lat_q, lat_n, dilation, flip, rows_upper):
    """ln_neighbours into a sentinel-filled buffer longer than rows_upper * E -> (rc, int32 array of the whole buffer)"""
    from lattice_net_amd import _lib
    E = NR.extent(lat_q.pos_dim())
    buf = torch.full((rows_upper * E + 3 * E + 5,), SENTINEL, dtype=torch.int32, device=dev())
    tq, tn = lat_q.m_hash_table.c_table(), lat_n.m_hash_table.c_table()
    rc = _lib.load().ln_neighbours(C.byref(tq), rows_upper, C.byref(tn), lat_q.m_lvl, lat_n.m_lvl, int(dilation), int(flip), _lib.ptr(buf),
                                   _lib.stream_ptr(dev()))
    torch.cuda.synchronize()
    return rc, N(buf)


def check(lat_q, lat_n, keys_q, dict_n, lvl_diff, dilation, what):
    """Both flips x both launch bounds of one (query, neighbours, dilation) against the reference; returns the reference and the kernel's list at flip 0"""
    m, d = keys_q.shape
    E = NR.extent(d)
    assert m % NR.rows_per_workgroup(d) != 0, "the last workgroup must be a partial one"
    assert NR.largest_coordinate(keys_q, lvl_diff, dilation) < NR.FLOAT_EXACT
    lists, refs = {}, {}
    for flip in (0, 1):
        ref = refs[flip] = NR.neighbour_list(keys_q, dict_n, lvl_diff, dilation, flip)
        for upper in (m, m + 2 * NR.rows_per_workgroup(d) + 3):
            rc, out = run(lat_q, lat_n, dilation, flip, upper)
            assert rc == 0, (what, flip, upper)
            got = out[: m * E].reshape(m, E)
            bad = np.argwhere(got != ref)
            assert bad.size == 0, (what, f"flip {flip} rows_upper {upper}: {len(bad)} entries differ, first (row, slot) {tuple(bad[0])}: "
                                         f"got {got[tuple(bad[0])]}, exact {ref[tuple(bad[0])]}")
            assert np.all(out[m * E: upper * E] == NOT_VISITED), (what, flip, upper, "rows beyond nr_filled must read LN_NOT_VISITED")
            assert np.all(out[upper * E:] == SENTINEL), (what, flip, upper, "written beyond query_rows_upper")
        lists[flip] = got
    perm = [e ^ 1 for e in range(E - 1)] + [E - 1]
    assert np.array_equal(lists[1], lists[0][:, perm]), (what, "flip = 1 must be flip = 0 with the slots of every axis swapped")
    return refs[0], lists[0]


def assert_same_level_invariants(nbr):
    m, E = nbr.shape
    rows = np.arange(m)
    assert np.array_equal(nbr[:, E - 1], rows)
    for a in range((E - 1) // 2):
        for here, there in ((2 * a, 2 * a + 1), (2 * a + 1, 2 * a)):
            j = nbr[:, here]
            ok = j >= 0
            assert np.array_equal(nbr[j[ok], there], rows[ok]), (a, here)


@pytest.mark.parametrize("order", ["canonical", "slot"])
@pytest.mark.parametrize("table", ["hash", "space"])
@pytest.mark.parametrize("d", range(1, 7))
def test_integer_form(d, table, order):
    """dilation 1, 2, 3, 5 x flip 0, 1 x launch bound, over hashed and space-ordered slots (k_neighbours then walks the row regions of
    the table), in both row numberings; plus what holds without a reference: the centre is the row itself, np and nm are mutual"""
    lat, keys, td = lattice("lines", d, table, order)
    assert not NR.beyond_threshold(keys).any()
    for dilation in NR.SMALL_DILATIONS:
        ref, got = check(lat, lat, keys, td, 0, dilation, ("lines", d, table, order, dilation))
        NR.assert_same_level_not_vacuous(ref, (d, dilation))
        assert_same_level_invariants(got)


@pytest.mark.parametrize("kind", ["beyond", "straddle"])
@pytest.mark.parametrize("d", [1, 2])
def test_float_form_by_coordinate(d, kind):
    lat, keys, td = lattice(kind, d)
    beyond = NR.beyond_threshold(keys)
    if kind == "beyond":
        assert beyond.all(), "every vertex must have a coordinate beyond +-2^22"
    else:
        assert 0.25 <= beyond.mean() <= 0.75, "a quarter of the vertices on either side of the threshold"
    for dilation in NR.FLOAT_COORD_DILATIONS:
        ref, got = check(lat, lat, keys, td, 0, dilation, (kind, d, dilation))
        NR.assert_same_level_not_vacuous(ref, (kind, d, dilation))
        assert_same_level_invariants(got)


@pytest.mark.parametrize("d", [1, 3])
def test_float_form_by_dilation(d):
    """dilation 2^18 and 2^18 + 1: two clusters that far apart along one axis (hits), everything else absent or beyond the key format"""
    lat, keys, td = lattice("far", d)
    for dilation in NR.FAR_DILATIONS:
        ref, got = check(lat, lat, keys, td, 0, dilation, ("far", d, dilation))
        assert NR.shares(ref)["hit_count"] >= 16
        assert_same_level_invariants(got)


_CROSSING = {}


def crossing(d):
    if d not in _CROSSING:
        fine, fk, fd = lattice("crossing", d)
        coarse = fine.create_coarse_verts()
        assert coarse.m_hash_table._storage.key_format == 0 and coarse.m_lvl == fine.m_lvl + 1
        _CROSSING[d] = (fine, fk, fd) + with_keys(coarse)
    return _CROSSING[d]


@pytest.mark.parametrize("d", range(1, 7))
def test_level_crossing_forms(d):
    """fine -> coarse (scale 1/2: the centre rule, for odd d + 1 the integer-neighbour rule) and coarse -> fine (scale 2), the coarse level a
    raw-format key table made by create_coarse_verts; dilation 1, 2 x flip 0, 1 x launch bound"""
    fine, fk, fd, coarse, ck, cd = crossing(d)
    for dilation in NR.CROSSING_DILATIONS:
        ref, _ = check(fine, coarse, fk, cd, -1, dilation, ("fine_to_coarse", d, dilation))
        NR.assert_fine_to_coarse_conditions(ref, d, dilation, (d, dilation))
        ref, _ = check(coarse, fine, ck, fd, 1, dilation, ("coarse_to_fine", d, dilation))
        s = NR.shares(ref)
        assert s["unvisited"] == 0.0 and s["centre_unvisited"] == 0.0 and s["hits"] >= 0.05 and s["absent"] >= 0.05, s


@pytest.mark.parametrize("deterministic", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("width", [32, 5])
@pytest.mark.parametrize("d", range(1, 7))
def test_fused_launch(d, width, dtype, deterministic):
    """The list ln_splat_accumulate_and_neighbours[_f16] writes behind a splat: rows_upper rows, the reference on [0, m), LN_NOT_VISITED on
    [m, rows_upper)"""
    from lattice_net_amd import Lattice
    from lattice_net_amd import lattice as LL
    pos, sigma = NR.cloud("lines", d)
    vals = torch.from_numpy(np.random.default_rng(d).standard_normal((len(pos), width)).astype(np.float32)).to(dev()).to(dtype)
    prev = LL.set_deterministic(deterministic)
    try:
        lat = Lattice(sigmas=[sigma] * d, capacity=NR.CAPACITY, device=dev())
        assert lat.prefetch_neighbours
        lat.begin_splat()
        lat.splat_standalone(T(pos), vals)
        lat, keys, td = with_keys(lat)  # (reads the vertex count: a build that had to be replayed has issued the fused launch again)
        st = lat.m_hash_table._storage
        pre = st.nbr_cache.get(("prefetch", st.uid, st.version, lat.m_lvl))
        assert pre is not None, "the fused entry point did not run"
        torch.cuda.synchronize()
    finally:
        LL.set_deterministic(prev)
    got = N(pre[0])
    m, E = len(keys), NR.extent(d)
    rows_upper = min(NR.CAPACITY, len(pos) * (d + 1))
    assert got.shape == (rows_upper, E) and rows_upper > m
    ref = NR.neighbour_list(keys, td, 0, 1, 0)
    NR.assert_same_level_not_vacuous(ref, d)
    assert np.array_equal(got[:m], ref)
    assert np.all(got[m:] == NOT_VISITED)


def test_argument_errors_launch_nothing():
    from lattice_net_amd import _lib
    lat, keys, _ = lattice("lines", 3)
    other, _, _ = lattice("lines", 2)
    m, E = len(keys), NR.extent(3)
    lib = _lib.load()
    tq, tn, t2 = lat.m_hash_table.c_table(), lat.m_hash_table.c_table(), other.m_hash_table.c_table()
    for what, args in (("two levels apart", (tq, tn, 1, 3, 1)), ("two levels apart", (tq, tn, 3, 1, 1)), ("dilation 0", (tq, tn, 1, 1, 0)),
                       ("dilation -1", (tq, tn, 1, 1, -1)), ("pos_dim mismatch", (tq, t2, 1, 1, 1))):
        buf = torch.full((m * E + 7,), SENTINEL, dtype=torch.int32, device=dev())
        a, b, lq, ln, dilation = args
        rc = lib.ln_neighbours(C.byref(a), m, C.byref(b), lq, ln, dilation, 0, _lib.ptr(buf), _lib.stream_ptr(dev()))
        torch.cuda.synchronize()
        assert rc == -1, (what, rc)  # LN_ERR_ARG
        assert lib.ln_last_error_string(), what
        assert np.all(N(buf) == SENTINEL), what
