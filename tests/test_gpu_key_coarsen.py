"""The key-built coarse level (ln_coarsen: k_insert_coarse<D> + the ranking behind it, reached through Lattice.create_coarse_verts)
against the oracle's serial `coarsen_keys`, at every position dimension 1 .. 6 (`pytest -m gpu`).

Everything compared here is an integer: vertex counts, keys IN ORDER (coarse row r is the r-th first occurrence in (fine row, token)
order: centre, then per axis np, then nm), levels, and the level-crossing neighbour lists in both directions and both flips.  No
tolerance anywhere in this file.  The clouds, the oracle's tables and the conditions that keep a case from being vacuous live in
tests/table_reference.py; tests/test_table_reference.py evaluates them without a GPU, and the tests below assert the conditions again
on the keys they read back from the device.

Edges: fine levels without a seed (0 coarse rows); 4, 255, 256 and 257 fine vertices at d = 3 and 2 at d = 1 (the kernel's workgroup is
256 rows; a fine level of ONE vertex cannot be built from points: a point inserts d + 1 of them); `fine_rows_upper` beyond and below
the fine vertex count through the C ABI; wide d = 5 / 6 fine levels in the lattice key format whose halved keys fit the raw format of
the coarse table, or do not (reported, not silently wrong); a second coarsening, of a raw-format fine table; fine levels numbered
in slot order, in space order and hashed into the whole table."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import lattice_oracle as O
from tests import table_reference as R

pytestmark = pytest.mark.gpu
VAL_DIM = 3


def dev():
    return torch.device("cuda", 0)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def N(t):
    return t.detach().cpu().numpy()


def build_fine(pos, sigma, cap=R.CAP):
    """Fine level with VAL_DIM-wide values (the coarse level takes its value width from it) -> (lattice, vertex count)"""
    from lattice_net_amd import Lattice
    d = pos.shape[1]
    lat = Lattice(sigmas=[float(sigma)] * d, capacity=int(cap), device=dev())
    lat.begin_splat()
    lat.splat_standalone(T(pos), torch.ones((len(pos), VAL_DIM), device=dev()))
    m = lat.nr_lattice_vertices()
    assert int(N(lat.m_hash_table._counters)[1]) == 0, "the fine build reported a status bit"
    return lat, m


def keys_of(lat):
    m = lat.nr_lattice_vertices()
    return N(lat.m_hash_table.m_keys_tensor)[:m].copy()


def assert_coarse_level(fine, coarse, expect_keys, what):
    """count, keys in order, level, values, key format of a level made by create_coarse_verts"""
    mc = coarse.nr_lattice_vertices()
    assert mc == len(expect_keys), (what, "coarse vertex count", mc, len(expect_keys))
    got = N(coarse.m_hash_table.m_keys_tensor)
    bad = np.nonzero((got[:mc] != expect_keys).any(axis=1))[0]
    assert bad.size == 0, (what, f"{bad.size} coarse rows hold another key, first row {bad[0]}: got {got[bad[0]]}, oracle {expect_keys[bad[0]]}")
    assert not got[mc:].any(), (what, "key rows beyond the vertex count must stay zero")
    assert coarse.lvl() == fine.lvl() + 1
    assert coarse.m_hash_table._storage.key_format == 0, "the coarse table holds halved keys: raw format"
    assert tuple(coarse.values().shape) == (mc, VAL_DIM) and not bool(coarse.values().any())
    assert int(N(coarse.m_hash_table._counters)[1]) == 0, (what, "status bit")


def assert_crossing_neighbours(fine, coarse, t_fine, t_coarse, what):
    """coarse -> fine and fine -> coarse neighbour lists at dilation 1, both flips, against the oracle's traversal"""
    fk, ck = R.keys_of(t_fine), R.keys_of(t_coarse)
    for flip in (False, True):
        assert np.array_equal(N(coarse.neighbours(fine, 1, flip)), O.neighbour_rows(ck, t_fine, coarse.lvl(), fine.lvl(), 1, flip)), (what, "coarse -> fine", flip)
        assert np.array_equal(N(fine.neighbours(coarse, 1, flip)), O.neighbour_rows(fk, t_coarse, fine.lvl(), coarse.lvl(), 1, flip)), (what, "fine -> coarse", flip)


@pytest.mark.parametrize("d", range(1, 7))
def test_coarse_level_equals_the_oracle(d):
    pos, sigma = R.main_cloud(d)
    t, _, _, tc = R.main_oracle(d)
    fine, m = build_fine(pos, sigma)
    fk = keys_of(fine)
    assert m == t.nr_filled and np.array_equal(fk, R.keys_of(t))
    R.assert_coarsen_conditions(R.coarsen_rows(fk), d)
    coarse = fine.create_coarse_verts()
    assert_coarse_level(fine, coarse, R.keys_of(tc), d)
    assert_crossing_neighbours(fine, coarse, t, tc, d)
    # the fine level is untouched
    assert fine.nr_lattice_vertices() == m and np.array_equal(keys_of(fine), fk) and fine.lvl() == 1


@pytest.mark.parametrize("count", [1, 2])
@pytest.mark.parametrize("d", R.NO_SEED_DIMS)
def test_fine_level_without_a_seed_gives_an_empty_coarse_level(d, count):
    """No all-even fine vertex: 0 coarse rows, no error.  A neighbour query of the fine level into it finds nothing: every slot the
    traversal looks at reads -1, and the slots it never looks at (the centre of a vertex that is not all-even; for odd d + 1 a
    neighbour with a half-integer coordinate) read -2 exactly where the oracle leaves them unvisited."""
    pts, sigma = R.no_seed_points(d, count)
    t, _, _ = R.oracle_build(pts, sigma)
    fine, m = build_fine(pts, sigma)
    assert m == t.nr_filled and not R.seeds_of(keys_of(fine)).any()
    coarse = fine.create_coarse_verts()
    assert_coarse_level(fine, coarse, np.zeros((0, d), np.int32), (d, count))
    empty = O.OracleHashTable(R.CAP, d)
    for flip in (False, True):
        nbr = N(fine.neighbours(coarse, 1, flip))
        assert nbr.shape == (m, 2 * (d + 1) + 1) and (nbr < 0).all()
        ref = O.neighbour_rows(R.keys_of(t), empty, 1, 2, 1, flip)
        assert np.array_equal(nbr, ref)
        assert (nbr[ref != O.NOT_VISITED] == -1).all()


@pytest.mark.parametrize("target", R.BLOCK_EDGE_COUNTS)
def test_fine_vertex_counts_around_the_workgroup(target):
    pts, sigma = R.points_for_vertex_count(target)
    t, _, _ = R.oracle_build(pts, sigma)
    tc = R.oracle_coarse(t)
    fine, m = build_fine(pts, sigma)
    assert m == target == t.nr_filled
    R.assert_coarsen_conditions(R.coarsen_rows(keys_of(fine)), target)
    coarse = fine.create_coarse_verts()
    assert_coarse_level(fine, coarse, R.keys_of(tc), target)
    assert_crossing_neighbours(fine, coarse, t, tc, target)


@pytest.mark.parametrize("d", R.ONE_POINT_DIMS)
def test_fine_level_of_one_point(d):
    pts, sigma = R.one_point_with_a_seed(d)
    t, _, _ = R.oracle_build(pts, sigma)
    tc = R.oracle_coarse(t)
    fine, m = build_fine(pts, sigma)
    assert m == d + 1 and tc.nr_filled >= 2
    coarse = fine.create_coarse_verts()
    assert_coarse_level(fine, coarse, R.keys_of(tc), d)
    assert_crossing_neighbours(fine, coarse, t, tc, d)


def coarsen_through_the_abi(fine, rows_upper):
    """What create_coarse_verts does, with a fine_rows_upper of the caller's choosing: buffers sized for it, then ln_coarsen"""
    from lattice_net_amd import _lib
    from lattice_net_amd.lattice import _build_sizes
    coarse = fine._new_coarse()
    coarse.m_hash_table._storage.key_format = _lib.LN_KEYS_RAW
    tokens = rows_upper * (2 * (fine.pos_dim() + 1) + 1)
    coarse._choose_hash_capacity(tokens, fresh=True)
    cap = coarse.m_hash_table._storage.hashed()
    ws = fine._workspace(_build_sizes(tokens, cap)[0])
    csr_buf, csr, _ = fine._alloc_csr(tokens, cap)
    tf, tc = fine.m_hash_table.c_table(), coarse.m_hash_table.c_table()
    rc = _lib.load().ln_coarsen(C.byref(tf), rows_upper, C.byref(tc), C.byref(csr), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev()))
    assert rc == 0, _lib.load().ln_last_error_string()
    torch.cuda.synchronize()
    coarse.m_hash_table._storage.touch()
    coarse.m_hash_table.m_nr_filled_is_dirty = True
    return coarse, csr_buf


@pytest.mark.parametrize("d", R.CLAMP_DIMS)
def test_fine_rows_upper_through_the_c_abi(d):
    """fine_rows_upper = m + 300: the same table as m (rows beyond the count hand out no token).  fine_rows_upper = m // 2: the oracle's
    loop over the first m // 2 fine rows, lookups still answered by the whole fine table."""
    pos, sigma = R.main_cloud(d)
    t, _, _, tc = R.main_oracle(d)
    fine, m = build_fine(pos, sigma)
    fk = keys_of(fine)
    assert np.array_equal(fk, R.keys_of(t))
    for rows_upper, expect in ((m, R.keys_of(tc)), (m + 300, R.keys_of(tc)), (m // 2, R.coarsen_rows(fk, m // 2)["keys"])):
        coarse, _keep = coarsen_through_the_abi(fine, rows_upper)
        mc = coarse.nr_lattice_vertices()
        assert mc == len(expect), (d, rows_upper, mc, len(expect))
        assert np.array_equal(N(coarse.m_hash_table.m_keys_tensor)[:mc], expect), (d, rows_upper)
        assert not N(coarse.m_hash_table.m_keys_tensor)[mc:].any()
    half = R.coarsen_rows(fk, m // 2)
    assert 20 <= len(half["keys"]) < tc.nr_filled and len(R.coarsen_rows(fk[: m // 2])["tokens"]) < len(half["tokens"])


@pytest.mark.parametrize("d,reach", list(R.WIDE))
def test_wide_fine_level_in_the_lattice_key_format(d, reach):
    """The fine keys lie beyond the raw format, so the fine table is in the lattice format and k_insert_coarse looks its np / nm
    neighbours up there; the coarse table is raw.  Halved keys that fit reproduce the oracle; one that does not fit is reported."""
    import lattice_net_amd as L
    pos, t, _, _ = R.wide_cloud(d, reach)
    fine, m = build_fine(pos, 1.0, R.WIDE_CAP)
    fk = keys_of(fine)
    assert m == t.nr_filled and np.array_equal(fk, R.keys_of(t))
    assert fine.m_hash_table._storage.key_format == 1 and not R.fits_raw_format(fk)
    expect = R.coarsen_rows(fk)
    fits = R.fits_raw_format(expect["keys"])
    assert fits == R.WIDE[(d, reach)] and expect["seeds"] >= 20
    if fits:
        tc = R.wide_oracle_coarse(d, reach)
        coarse = fine.create_coarse_verts()
        assert_coarse_level(fine, coarse, R.keys_of(tc), (d, reach))
        assert_crossing_neighbours(fine, coarse, t, tc, (d, reach))
    else:
        with pytest.raises(L.LatticeNetHipError, match="packed 64-bit"):
            fine.create_coarse_verts()


@pytest.mark.parametrize("d", R.TWO_LEVEL_DIMS)
def test_two_key_built_levels(d):
    """create_coarse_verts on the result of create_coarse_verts: the fine table of the second call is in the raw key format"""
    pos, sigma = R.main_cloud(d)
    t, _, _, tc = R.main_oracle(d)
    tc2 = R.oracle_coarse(tc)
    fine, _ = build_fine(pos, sigma)
    coarse = fine.create_coarse_verts()
    assert_coarse_level(fine, coarse, R.keys_of(tc), (d, "first"))
    R.assert_coarsen_conditions(R.coarsen_rows(keys_of(coarse)), (d, "second"))
    coarse2 = coarse.create_coarse_verts()
    assert_coarse_level(coarse, coarse2, R.keys_of(tc2), (d, "second"))
    assert coarse2.lvl() == 3 and coarse2.m_sigmas == pytest.approx([4 * sigma] * d)
    assert_crossing_neighbours(coarse, coarse2, tc, tc2, (d, "second"))


@pytest.mark.parametrize("numbering", ["slot", "space", "full"])
def test_fine_level_in_other_numberings(numbering):
    """d = 3.  The fine rows in slot order, in space order (over a calibrated slot map) and hashed into the whole table: the coarse key
    SET is the oracle's, and the coarse ORDER is the oracle's after its fine rows are relabelled by the fine level's permutation —
    the first-occurrence rule applied to the fine rows as the device numbered them."""
    import lattice_net_amd as L
    from lattice_net_amd import lattice as LL
    d = 3
    pos, sigma = R.main_cloud(d)
    t, _, _, tc = R.main_oracle(d)
    prev_row = LL.set_row_order("canonical" if numbering == "full" else "slot")
    prev_slot = LL.set_slot_order("space" if numbering == "space" else "hash")
    prev_policy = L.set_hash_capacity_policy("full" if numbering == "full" else "tokens")
    try:
        fine = L.Lattice(sigmas=[sigma] * d, capacity=R.CAP, device=dev())
        fine.begin_splat()
        idx, _ = fine.splat_standalone(T(pos), torch.ones((len(pos), VAL_DIM), device=dev()))
        m = fine.nr_lattice_vertices()
        if numbering == "space":
            fine.calibrate_regions(idx)
            fine.begin_splat()
            fine.splat_standalone(T(pos), torch.ones((len(pos), VAL_DIM), device=dev()))
            m = fine.nr_lattice_vertices()
            st = fine.m_hash_table._storage
            assert st.slot_map is not None and st.rows_follow_space, "the fine table must be space-ordered"
        if numbering == "full":
            assert fine.m_hash_table._storage.hashed() == R.CAP
        coarse = fine.create_coarse_verts()
        mc = coarse.nr_lattice_vertices()
    finally:
        LL.set_row_order(prev_row)
        LL.set_slot_order(prev_slot)
        L.set_hash_capacity_policy(prev_policy)
    fk = keys_of(fine)
    perm = R.row_permutation(fk, R.keys_of(t))  # (asserts the fine vertex set)
    if numbering == "full":
        assert np.array_equal(perm, np.arange(m))
    else:
        assert not np.array_equal(perm, np.arange(m)), "the fine level came out in the oracle's numbering: nothing is relabelled"
    ck = N(coarse.m_hash_table.m_keys_tensor)[:mc]
    assert mc == tc.nr_filled
    R.row_permutation(ck, R.keys_of(tc))  # the coarse key set is the oracle's
    expect = R.coarsen_rows(fk)
    R.assert_coarsen_conditions(expect, numbering)
    assert np.array_equal(ck, expect["keys"]), (numbering, "coarse keys in the order of the relabelled fine rows")
    assert coarse.lvl() == 2 and tuple(coarse.values().shape) == (mc, VAL_DIM) and not bool(coarse.values().any())
