"""CPU checks of tests/slice_f16_reference.py, the reference and bound test_gpu_slice_f16.py holds k_slice_forward_f16 to.

- The kernel's arithmetic emulated in NumPy fp32 in both forms a compiler may give it (product and sum rounded apart, or one fused
  multiply-add) stays inside the bound on every case and run of the GPU test and is the rounded fp64 sum bit for bit on the exact run.
  The worst error / bound ratio is printed (`pytest -s`); the one rounding to fp16 alone brings it close to 1 (half an ulp of a number
  just above a power of two is the whole 2^-11 |ref| term), so 0.9 .. 1 is what a correct kernel shows.
- Five wrong kernels, planted in the emulation, each fall outside the bound or fail the exact run on at least one case.
- slice_f16_instance agrees with hand-worked examples of ln_slice_forward_f16_impl, and the case list reaches all 18 instances."""
import numpy as np
import pytest

from tests import slice_f16_reference as S

_RATIOS = {}


@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_fp32_emulations_are_inside_the_bound(name):
    case = S.CASES_BY_NAME[name]
    worst = {}
    for run in S.RUNS:
        values, idx, w = S.make_inputs(case, run)
        for form in S.FORMS:
            got = S.emulate_slice_f16(values, idx, w, case.n, case.d, form)
            worst[(run, form)] = S.assert_slice_f16(got, values, idx, w, case.n, case.d, run, f"{name} {run} {form}")
    _RATIOS[name] = worst
    print(f"{name} worst error / bound: " + ", ".join(f"{r} {f} {x:.3f}" for (r, f), x in worst.items() if r != "exact"))
    assert max(worst.values()) <= 1.0


def test_the_cancel_run_cancels_and_the_bound_is_the_formula():
    """|ref| << mag on the cancel run (median over the elements below 1 / 16), so its bound is far below one fp16 rounding of a partial
    sum; the bound is the stated formula, element by element, on hand-made numbers."""
    case = S.CASES_BY_NAME["d3-V64-n293"]
    values, idx, w = S.make_inputs(case, "cancel")
    ref, mag = S.slice_f16_ref(values, idx, w, case.n, case.d)
    live = mag > 0
    assert float(np.median(np.abs(ref[live]) / mag[live])) < 1.0 / 16
    assert float(np.median(S.slice_f16_bound(ref, mag, case.d)[live] / (2.0 ** -11 * mag[live]))) < 1.0 / 8
    ref, mag = np.array([0.0, 3.0, -1000.0, 2.0 ** -20]), np.array([0.0, 5.0, 1000.0, 2.0 ** -20])
    for d in (1, 6):
        e32 = 2 * (d + 1) * 2.0 ** -24 * mag
        want = [2.0 ** -25, e32[1] + 2.0 ** -11 * (3.0 + e32[1]), e32[2] + 2.0 ** -11 * (1000.0 + e32[2]), e32[3] + 2.0 ** -25]
        np.testing.assert_array_equal(S.slice_f16_bound(ref, mag, d), np.array(want))


def test_reference_skips_absent_slots_and_counts_every_live_one():
    """slice_f16_ref against a token-by-token Python loop, with a NaN row nobody names and w = -1 in the absent slots."""
    case = S.CASES_BY_NAME["d4-V12-n293-row0"]
    values, idx, w = S.make_inputs(case, "exact")
    values = values.copy()
    values[1, :] = np.float16(np.nan)
    idx = np.where(idx == 1, 2, idx)
    ref, mag = S.slice_f16_ref(values, idx, w, case.n, case.d)
    want, wmag = np.zeros_like(ref), np.zeros_like(mag)
    for t in range(case.n * (case.d + 1)):
        if idx[t] >= 0:
            term = values[idx[t]].astype(np.float64) * float(w[t])
            want[t // (case.d + 1)] += term
            wmag[t // (case.d + 1)] += np.abs(term)
    np.testing.assert_array_equal(ref, want)
    np.testing.assert_array_equal(mag, wmag)
    assert np.isfinite(ref).all() and np.all(w[idx < 0] == -1.0)


def test_inputs_have_the_edges_the_gpu_test_relies_on():
    for case in S.CASES:
        m = S.case_rows(case)
        for run in S.RUNS:
            values, idx, w = S.make_inputs(case, run)
            i2 = idx.reshape(case.n, case.d + 1)
            assert values.dtype == np.float16 and values.shape == (m, case.v) and m <= 5000 and case.n <= 3000
            assert idx.max(initial=-1) < m and np.all(w[idx < 0] == -1.0) and np.all(w[idx >= 0] != 0)
            assert bool((idx == 0).any()) == (case.row0 and case.n >= 4), case.name
            assert np.isnan(values[0]).all() != case.row0 and np.isfinite(values[1:]).all()
            if case.n >= 4:
                assert (i2[S.P_ALL_ABSENT] < 0).all()
                assert i2[S.P_FIRST_ABSENT, 0] < 0 and (i2[S.P_FIRST_ABSENT, 1:] >= 0).all()
                assert i2[S.P_LAST_ABSENT, -1] < 0 and (i2[S.P_LAST_ABSENT, :-1] >= 0).all()
            if case.n >= 250:
                assert 0.02 < float((idx < 0).mean()) < 0.09, (case.name, float((idx < 0).mean()))
            if run == "exact":
                assert np.all(w * S.FRAC == np.round(w * S.FRAC)) and np.abs(w).max() <= 1 and (case.n < 30 or (w[idx >= 0] < 0).any())
                assert np.all(values[1:] == np.round(values[1:])) and np.abs(values[1:]).max() <= 64
            else:
                assert np.all(w[idx >= 0] > 0)
            again = S.make_inputs(case, run)
            assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip((values, idx, w), again))


@pytest.mark.parametrize("fault", S.FAULTS)
def test_wrong_kernels_fall_outside(fault):
    """Each planted fault fails the bound of the random or cancel run, or the bit-for-bit comparison of the exact run, on at least one
    case of the list; the unfaulted emulation passes on that same case and run."""
    caught = []
    for case in S.CASES:
        hv = S.case_instance(case)[0]
        for run in S.RUNS:
            values, idx, w = S.make_inputs(case, run)
            for form in S.FORMS:
                try:
                    S.assert_slice_f16(S.emulate_slice_f16(values, idx, w, case.n, case.d, form, fault, hv), values, idx, w, case.n, case.d, run,
                                       f"{case.name} {run} {fault}")
                except AssertionError:
                    S.assert_slice_f16(S.emulate_slice_f16(values, idx, w, case.n, case.d, form), values, idx, w, case.n, case.d, run, "no fault")
                    caught.append((case.name, run))
    runs = sorted({r for _, r in caught})
    print(f"{fault}: caught on {len({c for c, _ in caught})} of {len(S.CASES)} cases, runs {runs}")
    assert caught, f"{fault} survives every case: add a case"
    if fault in ("acc_f16", "round_each", "w_f16"):
        assert "cancel" in runs, runs  # (the run made for them: the exact run's sums rarely reach 2^8, where a second rounding would show)
    if fault in ("no_skip", "last_word"):
        assert "exact" in runs, runs


def test_instance_table():
    """Hand-worked examples of ln_slice_forward_f16_impl: (d, V, values pointer, out pointer) -> (HV, CH) or the error code."""
    A = S.ALIGNED
    table = {
        (3, 64, A, A): (8, 8), (3, 64, A + 8, A): (4, 0), (3, 64, A, A + 8): (4, 0), (3, 64, A + 16, A + 32): (8, 8),
        (1, 8, A, A): (8, 0), (6, 72, A, A): (8, 0), (2, 128, A, A): (8, 0), (5, 520, A, A): (8, 0), (3, 16, A, A + 8): (4, 0),
        (3, 4, A, A): (4, 0), (4, 12, A, A): (4, 0), (4, 12, A + 8, A + 8): (4, 0), (3, 68, A, A): (4, 0),
        (3, 6, A, A): S.LN_ERR_UNSUPPORTED, (3, 2, A, A): S.LN_ERR_UNSUPPORTED, (3, 0, A, A): S.LN_ERR_UNSUPPORTED,
        (0, 64, A, A): S.LN_ERR_UNSUPPORTED, (7, 64, A, A): S.LN_ERR_UNSUPPORTED, (3, 6, A + 2, 0): S.LN_ERR_UNSUPPORTED,
        (3, 64, A + 2, A): S.LN_ERR_ARG, (3, 64, A + 4, A): S.LN_ERR_ARG, (3, 64, A, A + 2): S.LN_ERR_ARG, (3, 12, A, A + 4): S.LN_ERR_ARG,
        (3, 64, 0, A): S.LN_ERR_ARG, (3, 64, A, 0): S.LN_ERR_ARG,
    }
    for args, want in table.items():
        assert S.slice_f16_instance(*args) == want, (args, S.slice_f16_instance(*args), want)
    assert S.slice_f16_instance(3, 64, 0, 0, n=0) == (8, 8)  # (no point: null buffers pass the checks, nothing is launched)
    assert S.slice_f16_grid(33, 64, 8) == (264, 2) and S.slice_f16_grid(1, 4, 4) == (1, 1) and S.slice_f16_grid(57, 72, 8) == (513, 3)


def test_cases_reach_every_instance():
    """All 18 instances k_slice_forward_f16<d + 1, HV, CH>, d = 1 .. 6 x {(4, 0), (8, 0), (8, 8)}, the HV = 4 ones also at a width that is
    a multiple of 8 behind an 8-byte-aligned pointer, and the grid edges."""
    reached = {(c.d,) + S.case_instance(c) for c in S.CASES}
    assert reached == {(d, hv, ch) for d in range(1, 7) for hv, ch in ((4, 0), (8, 0), (8, 8))}, reached
    for d in range(1, 7):
        assert {(c.v, c.off_values, c.off_out) for c in S.CASES if c.d == d and S.case_instance(c) == (4, 0)} >= {(4, 0, 0), (12, 0, 0), (64, 8, 0), (16, 0, 8)}
        assert {c.v for c in S.CASES if c.d == d and S.case_instance(c) == (8, 0)} >= {8, 72}
    works = {S.slice_f16_grid(c.n, c.v, S.case_instance(c)[0])[0] for c in S.CASES}
    assert {1, 255, 256, 257} <= works and any(wk % 256 and wk > 256 for wk in works)
    assert any(c.v == 520 for c in S.CASES) and any(c.n == 1 for c in S.CASES)
