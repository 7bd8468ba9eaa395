"""tests/table_reference.py without a GPU: the integer restatement of the key-built coarse level agrees with the oracle's `coarsen_keys`
at full length on every cloud the GPU tests use, its stop after a number of fine rows is the oracle's loop cut short, and every case
of tests/test_gpu_key_coarsen.py and tests/test_gpu_position_lookup.py meets the conditions that keep it from being vacuous (the GPU
tests assert the same conditions again on what they compare)."""
import numpy as np
import pytest

from oracle import lattice_oracle as O
from tests import table_reference as R


def oracle_coarsen_first_rows(t_fine, rows):
    """O.coarsen_keys over the first `rows` fine rows, lookups answered by the whole fine table: the oracle's own loop, cut short by
    lowering the count it runs to"""
    tc = O.OracleHashTable(R.CAP, t_fine.pos_dim)
    kept = t_fine.nr_filled
    t_fine.nr_filled = rows  # (retrieve() walks the slot entries, which still name every row)
    try:
        O.coarsen_keys(t_fine, tc)
    finally:
        t_fine.nr_filled = kept
    return tc


@pytest.mark.parametrize("d", range(1, 7))
def test_coarsening_reference_equals_the_oracle_and_the_main_clouds_meet_the_conditions(d):
    t, _, _, tc = R.main_oracle(d)
    c = R.coarsen_rows(R.keys_of(t))
    assert np.array_equal(c["keys"], R.keys_of(tc)), (d, "coarse keys in order")
    R.assert_coarsen_conditions(c, d)
    assert 1500 <= t.nr_filled <= 8000 and R.fits_raw_format(c["keys"])
    # the oracle's tables sit far below the 300-probe retrieval limit
    assert R.longest_probe_run(t) < R.PROBE_MARGIN and R.longest_probe_run(tc) < R.PROBE_MARGIN


@pytest.mark.parametrize("d", R.CLAMP_DIMS)
def test_clamped_coarsening_is_the_oracles_loop_cut_short(d):
    t, _, _, tc = R.main_oracle(d)
    m = t.nr_filled
    half = R.coarsen_rows(R.keys_of(t), m // 2)
    assert np.array_equal(half["keys"], R.keys_of(oracle_coarsen_first_rows(t, m // 2)))
    assert 20 <= len(half["keys"]) < tc.nr_filled, "half the rows must give a smaller, non-trivial coarse level"
    # some lookup of the first half is answered by a row of the second half: the clamp must not shorten the fine table itself
    short = R.coarsen_rows(R.keys_of(t)[: m // 2])
    assert len(short["tokens"]) < len(half["tokens"])
    for rows in (m, m + 300):
        assert np.array_equal(R.coarsen_rows(R.keys_of(t), rows)["keys"], R.keys_of(tc))


@pytest.mark.parametrize("d", R.TWO_LEVEL_DIMS)
def test_second_coarsening_of_a_raw_format_table(d):
    _, _, _, tc = R.main_oracle(d)
    tc2 = R.oracle_coarse(tc)
    c2 = R.coarsen_rows(R.keys_of(tc))
    assert np.array_equal(c2["keys"], R.keys_of(tc2))
    R.assert_coarsen_conditions(c2, ("second level", d))


@pytest.mark.parametrize("d", R.NO_SEED_DIMS)
@pytest.mark.parametrize("count", [1, 2])
def test_points_without_a_seed(d, count):
    pts, sigma = R.no_seed_points(d, count)
    t, _, _ = R.oracle_build(pts, sigma)
    assert t.nr_filled >= d + 1 and not R.seeds_of(R.keys_of(t)).any()
    assert R.oracle_coarse(t).nr_filled == 0 and len(R.coarsen_rows(R.keys_of(t))["keys"]) == 0


@pytest.mark.parametrize("d", [1, 3, 5])
def test_every_simplex_of_an_odd_dimension_has_a_seed(d):
    """why NO_SEED_DIMS holds even dimensions only"""
    pos, sigma = R.main_cloud(d)
    assert R.seeds_of(R.simplex_keys_of(pos, sigma)).any(axis=1).all()


def test_block_edge_subsets_have_the_vertex_counts_they_are_named_after():
    for target in R.BLOCK_EDGE_COUNTS:
        pts, sigma = R.points_for_vertex_count(target)
        t, _, _ = R.oracle_build(pts, sigma)
        assert t.nr_filled == target
        c = R.coarsen_rows(R.keys_of(t))
        assert np.array_equal(c["keys"], R.keys_of(R.oracle_coarse(t)))
        R.assert_coarsen_conditions(c, target)
    # the smallest fine level a build from points can make: the d + 1 vertices of one point (a count of 1 is out of reach)
    for d in R.ONE_POINT_DIMS:
        pts, sigma = R.one_point_with_a_seed(d)
        t, _, _ = R.oracle_build(pts, sigma)
        assert t.nr_filled == d + 1
        c = R.coarsen_rows(R.keys_of(t))
        assert c["seeds"] >= 1 and len(c["keys"]) >= 2 and np.array_equal(c["keys"], R.keys_of(R.oracle_coarse(t)))


@pytest.mark.parametrize("d,reach", list(R.WIDE))
def test_wide_clouds_fit_the_raw_format_or_not_as_listed(d, reach):
    _, t, _, _ = R.wide_cloud(d, reach)
    lo, hi = R.raw_range(d)
    kmax = int(np.abs(R.keys_of(t)).max())
    assert hi < kmax < (12288 if d == 5 else 3584), "the fine level: beyond the raw format, inside the lattice format"
    c = R.coarsen_rows(R.keys_of(t))
    assert c["seeds"] >= 20
    assert R.fits_raw_format(c["keys"]) == R.WIDE[(d, reach)]
    if R.WIDE[(d, reach)]:
        assert np.array_equal(c["keys"], R.keys_of(R.wide_oracle_coarse(d, reach)))
    else:
        outside = (c["keys"] < lo).any(axis=1) | (c["keys"] > hi).any(axis=1)
        assert 1 <= outside.sum() < len(outside) // 2, "a few halved keys beyond the raw format, most of them inside"


@pytest.mark.parametrize("d,v,n", R.LOOKUP_CASES)
def test_lookup_queries_hold_the_three_kinds(d, v, n):
    pos, sigma, t, _, _ = R.lookup_oracle(d)
    for q, kind in R.lookup_calls(d, n):
        assert q.shape == (len(kind), d) and q.dtype == np.float32
        vals = np.ones((t.nr_filled, 1), np.float32)
        _, idx, w = R.oracle_lookup(t, vals, q, sigma)
        R.assert_query_kinds(idx, kind, d, (d, n))
        assert np.all((idx >= 0) == (w != -1.0))


def test_the_other_lookup_situations_hold_the_three_kinds_too():
    for d in R.REHASH_DIMS:
        q, kind = R.rehash_queries(d)
        t, sigma = R.rehash_clouds(d)[3], R.rehash_clouds(d)[2]
        R.assert_query_kinds(R.oracle_lookup(t, np.ones((t.nr_filled, 1), np.float32), q, sigma)[1], kind, d, ("rehash", d))
    for (d, reach), fits in R.WIDE.items():
        if fits:
            q, kind = R.wide_queries(d, reach)
            t = R.wide_cloud(d, reach)[1]
            R.assert_query_kinds(R.oracle_lookup(t, np.ones((t.nr_filled, 1), np.float32), q, 1.0)[1], kind, d, ("wide", d))
    for d in R.LOADED_DIMS:
        q, kind = R.loaded_queries(d)
        t = R.loaded_table(d)[1]
        R.assert_query_kinds(R.oracle_lookup(t, np.ones((t.nr_filled, 1), np.float32), q, R.MAIN[d][2])[1], kind, d, ("loaded", d))


def test_lookup_cases_cover_every_width_and_count():
    assert {c[0] for c in R.LOOKUP_CASES} == set(range(1, 7))
    assert {1, 3, 64, 65} <= {c[1] for c in R.LOOKUP_CASES}
    assert {0, 1, 256, 257, 1500} <= {c[2] for c in R.LOOKUP_CASES}


@pytest.mark.parametrize("d", R.REHASH_DIMS)
def test_rehash_clouds(d):
    first, second, sigma, t, (i1, w1), (i2, w2), m1 = R.rehash_clouds(d)
    # the first build hashes into 16384 slots, the table owns more: the incremental build has to re-hash
    assert max(16384, 2 * len(first) * (d + 1)) < R.REHASH_CAP
    assert t.nr_filled > 2 * m1 and i1.max() == m1 - 1 and i2.max() == t.nr_filled - 1
    # looking the positions up afterwards gives the indices and weights of their builds
    vals = np.zeros((t.nr_filled, 1), np.float32)
    for pts, (i, w) in ((first, (i1, w1)), (second, (i2, w2))):
        _, qi, qw = O.slice_no_precomputation(t, vals, O.scale_positions(pts, R.sigmas(d, sigma)))
        assert np.array_equal(qi, i) and np.array_equal(qw, w)


@pytest.mark.parametrize("d", R.LOADED_DIMS)
def test_loaded_tables_stay_below_the_probe_limit(d):
    cap, t, _, _ = R.loaded_table(d)
    assert 0.78 <= t.nr_filled / cap <= 0.8
    assert R.longest_probe_run(t) < R.PROBE_MARGIN, R.longest_probe_run(t)


def test_slice_bound_and_fp64_forms():
    """the fp64 slice equals the oracle's fp32 one within the bound it is used with, and the scatter is its transpose"""
    d, v, n = 3, 5, 300
    pos, sigma, t, _, _ = R.lookup_oracle(d)
    q, kind = R.queries(pos, sigma, n, 3, R.MAIN[d][1])
    rng = np.random.default_rng(1)
    vals = rng.standard_normal((t.nr_filled, v)).astype(np.float32)
    out, idx, w = O.slice_no_precomputation(t, vals, O.scale_positions(q, R.sigmas(d, sigma)))
    ref, mag = R.slice_fp64(vals, idx, w, n)
    assert np.all(np.abs(out - ref) <= R.slice_bound(mag, d))
    assert np.all(out[kind == 2] == 0.0) and np.all(mag[kind == 2] == 0.0)
    g = rng.standard_normal((n, v)).astype(np.float32)
    gv, gmag, count = R.scatter_fp64(g, idx, w, t.nr_filled)
    assert np.isclose((gv * vals).sum(), (ref * g).sum(), rtol=1e-9)
    assert count.sum() == (idx >= 0).sum() and np.all(gmag[count == 0] == 0.0)
