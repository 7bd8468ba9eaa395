"""tests/neighbour_reference.py without a GPU: the exact integer reference of the neighbour traversal agrees with the oracle (which
imitates the traversal's float arithmetic) entry for entry, it notices every seeded wrong traversal on every case the GPU test runs, and
the committed clouds meet the conditions that keep those cases from being vacuous.  The tables are the oracle's (the GPU builds the same
vertex sets: test_gpu_parity.py, test_gpu_build_paths.py); test_gpu_neighbour_forms.py asserts the same conditions again on the lists it
compares."""
import numpy as np
import pytest

from oracle import lattice_oracle as O
from tests import neighbour_reference as NR

CASES = NR.cases()
LEVELS = {0: (1, 1), -1: (1, 2), 1: (2, 1)}  # lvl_diff -> (query level, neighbour level) as the oracle takes them


def case_id(c):
    return "-".join(str(x) for x in c)


def keys_of(t):
    return t.keys[: t.nr_filled]


def case_sides(kind, d, direction):
    """(query keys, oracle neighbour table, dict of that table)"""
    fine, coarse = NR.oracle_tables(kind, d)
    table = {"same": fine, "fine_to_coarse": coarse, "coarse_to_fine": fine}[direction]
    qk, _ = NR.sides(keys_of(fine), None if coarse is None else keys_of(coarse), direction)
    return qk, table, NR.table_dict(keys_of(table))


@pytest.mark.parametrize("d", range(1, 7))
def test_exact_reference_equals_the_oracle(d):
    """d = 1 .. 6 x level difference -1, 0, +1 x dilation 1, 2, 3, 5 x both flips, every coordinate below 2^24"""
    for lvl_diff, way in ((0, "same"), (-1, "fine_to_coarse"), (1, "coarse_to_fine")):
        qk, table, td = case_sides("crossing", d, way)
        for dilation in (1, 2, 3, 5):
            assert NR.largest_coordinate(qk, lvl_diff, dilation) < NR.FLOAT_EXACT
            for flip in (False, True):
                ref = NR.neighbour_list(qk, td, lvl_diff, dilation, flip)
                oracle = O.neighbour_rows(qk, table, *LEVELS[lvl_diff], dilation, flip)
                assert ref.dtype == oracle.dtype and np.array_equal(ref, oracle), (d, way, dilation, flip, int(np.sum(ref != oracle)))


@pytest.mark.parametrize("case", [c for c in CASES if c[0] != "crossing" and c[0] != "lines"], ids=case_id)
def test_exact_reference_equals_the_oracle_on_the_float_form_clouds(case):
    kind, d, way, dilation = case
    qk, table, td = case_sides(kind, d, way)
    assert NR.largest_coordinate(qk, 0, dilation) < NR.FLOAT_EXACT
    for flip in (False, True):
        assert np.array_equal(NR.neighbour_list(qk, td, 0, dilation, flip), O.neighbour_rows(qk, table, 1, 1, dilation, flip))


def test_rounding_of_halves_is_roundf():
    k2 = np.array([-5, -4, -3, -2, -1, 0, 1, 2, 3, 4, 5], np.int64)
    assert np.array_equal(NR._halve_rounding_half_away(k2), O._round_half_away(k2.astype(np.float32) / np.float32(2)))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_seeded_wrong_traversal_is_noticed(case):
    kind, d, way, dilation = case
    qk, _, td = case_sides(kind, d, way)
    for flip in (0, 1):
        ref = NR.neighbour_list(qk, td, NR.LVL_DIFF[way], dilation, flip)
        for wrong in NR.WRONG:
            got = NR.neighbour_list(qk, td, NR.LVL_DIFF[way], dilation, flip, wrong=wrong)
            if NR.wrong_applies(wrong, d, way, dilation):
                assert not np.array_equal(got, ref), (case, flip, wrong)
            else:
                assert np.array_equal(got, ref), (case, flip, wrong)  # (the reasons in wrong_applies are facts, not excuses)


def test_every_wrong_traversal_applies_somewhere_at_every_dimension():
    for d in range(1, 7):
        for wrong in NR.WRONG:
            ways = [c for c in CASES if c[1] == d and NR.wrong_applies(wrong, *c[1:])]
            assert ways or (wrong == "no_odd_rule" and (d + 1) % 2 == 0), (d, wrong)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_cases_are_not_vacuous(case):
    kind, d, way, dilation = case
    qk, _, td = case_sides(kind, d, way)
    m = len(qk)
    assert 100 <= m <= 12000 and m % NR.rows_per_workgroup(d) != 0, m
    assert NR.largest_coordinate(qk, NR.LVL_DIFF[way], dilation) < NR.FLOAT_EXACT
    nbr = NR.neighbour_list(qk, td, NR.LVL_DIFF[way], dilation, 0)
    if way == "fine_to_coarse":
        NR.assert_fine_to_coarse_conditions(nbr, d, dilation, case)
    elif way == "same" and kind != "far":
        NR.assert_same_level_not_vacuous(nbr, case)
    elif kind == "far":
        assert NR.shares(nbr)["hit_count"] >= 16, case
    if way == "same":
        assert np.array_equal(nbr[:, -1], np.arange(m))
    beyond = NR.beyond_threshold(qk)
    if kind == "beyond":
        assert beyond.all()
    elif kind == "straddle":
        assert 0.25 <= beyond.mean() <= 0.75
        # both forms inside one workgroup: some run of ROWS consecutive rows holds vertices of either side
        rows = NR.rows_per_workgroup(d)
        tiles = [beyond[i:i + rows] for i in range(0, m, rows)]
        assert any(t.any() and not t.all() for t in tiles)
    else:
        assert not beyond.any()
    assert (dilation >= NR.INT_FORM_DILATION) == (kind == "far")


def test_structural_exceptions_of_the_fine_to_coarse_conditions():
    """fine_to_coarse_conditions names the cases where a 1 % share cannot hold; everywhere else all four are asserted"""
    for d in range(1, 7):
        for dilation in NR.CROSSING_DILATIONS:
            can = NR.fine_to_coarse_conditions(d, dilation)
            assert can["looked_up"] == (not (d in (2, 4, 6) and dilation == 2))
            assert can["absent"] == (can["looked_up"] and (d, dilation) != (1, 1))
            assert can["absent_share"] == (d != 6)
