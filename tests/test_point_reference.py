"""CPU checks of tests/point_reference.py, the references and bounds test_gpu_slice_classify.py holds the HIP kernels to.

- The NumPy fp32 emulation of the wave-tiled backward (tile walk, slabs, scatter) and a plain torch fp32 evaluation stay inside every
  bound at the shapes of the GPU test, and are the fp64 result bit for bit on the exact run.  Each test prints its worst error / bound
  ratio per output (`pytest -s`); a ratio near 1 would mean a rounding was not counted.
- Planted faults in the emulation are each caught by a bound or by the exact run.
- The dispatch tables name every kernel form the GPU test claims to reach."""
import numpy as np
import pytest

from tests import point_reference as P


def check(fn, inp, n, d, form, exact, what):
    ref, mag, bound = P.sc_backward_reference(inp, n, d, form)
    if exact:
        P.assert_exact_representable(mag, what)
    return P.assert_sc_backward(fn(inp, n, d), ref, bound, exact, what)


def both_runs(d, v, c, n, fns):
    form = P.sc_backward_form(d, v, c)
    out = {}
    for exact in (False, True):
        inp = P.make_sc_inputs(n, P.table_rows(n), d, v, c, seed=v + c + d, exact=exact)
        for fn in fns:
            out[(fn.__name__, exact)] = check(fn, inp, n, d, form, exact, f"d={d} V={v} C={c} n={n} {fn.__name__} exact={exact}")
    worst = {k: max(r[k] for r in out.values()) for k in next(iter(out.values()))}
    print(f"d={d} V={v} C={c} n={n} worst error / bound: " + ", ".join(f"{k} {x:.3f}" for k, x in worst.items()))
    assert max(worst.values()) <= 1.0
    return worst


@pytest.mark.parametrize("d,v,c", P.WAVE_BWD_CASES)
def test_emulation_and_torch_fp32_inside_the_bounds_small(d, v, c):
    both_runs(d, v, c, P.N_WAVE_SMALL, (P.emulate_sc_backward_wave, P.torch_fp32_sc_backward))


@pytest.mark.parametrize("d,v,c", [(3, 32, 13), (2, 64, 21), (3, 96, 21), (2, 128, 13)])
def test_emulation_and_torch_fp32_inside_the_bounds_beyond_the_grid_cap(d, v, c):
    """One instance per channel width, both class-tile counts and both lattice dimensions at the multi-tile size of the GPU test (the
    bounds depend on the instance only through d, V and C)."""
    assert P.sc_backward_grid(P.N_WAVE_LARGE, P.sc_backward_form(d, v, c)) == P.WAVE_BWD_GRID
    both_runs(d, v, c, P.N_WAVE_LARGE, (P.emulate_sc_backward_wave, P.torch_fp32_sc_backward))


@pytest.mark.parametrize("d,v,c,n", [(4, 8, 20, 2 * 64 * 512 + 9), (3, 5, 3, 2 * 64 * 512 + 9), (3, 160, 24, 1037), (3, 250, 16, 333)])
def test_torch_fp32_inside_the_bounds_of_the_general_forms(d, v, c, n):
    both_runs(d, v, c, n, (P.torch_fp32_sc_backward,))


@pytest.mark.parametrize("fault", P.FAULTS)
def test_planted_faults_are_caught(fault):
    """Each fault of the emulation fails a bound of the random run or the bit-for-bit comparison of the exact run (d = 3, V = 64, C = 21:
    two channel chunks, two class tiles; n = 16 * 4 * 3 + 5: the last tile ragged)."""
    d, v, c, n = 3, 64, 21, 16 * 4 * 3 + 5
    form = P.sc_backward_form(d, v, c)
    caught = []
    for exact in (False, True):
        inp = P.make_sc_inputs(n, P.table_rows(n), d, v, c, seed=7, exact=exact)
        ref, mag, bound = P.sc_backward_reference(inp, n, d, form)
        P.assert_sc_backward(P.emulate_sc_backward_wave(inp, n, d), ref, bound, exact, "no fault")
        try:
            P.assert_sc_backward(P.emulate_sc_backward_wave(inp, n, d, fault=fault), ref, bound, exact, fault)
        except AssertionError as e:
            caught.append(("exact" if exact else "random") + ": " + str(e).split(":")[0])
    print(fault, "->", caught)
    assert len(caught) == 2, (fault, caught)


def test_inputs_have_the_edges_the_gpu_test_relies_on():
    for n, d in ((P.N_WAVE_SMALL, 2), (P.N_FWD_WAVE, 3), (P.N_WAVE_LARGE, 3)):
        m = P.table_rows(n)
        idx, w = P.make_tokens(n, m, d, seed=3)
        i2 = idx.reshape(n, d + 1)
        share = float((idx < 0).mean())
        assert 0.15 < share < 0.3, share
        assert int((i2 < 0).all(1).sum()) >= n // 11
        assert np.all(w[idx < 0] == -1.0) and np.all(w[idx >= 0] > 0)
        assert idx.max() < m
        if n * (d + 1) > 1000:
            assert P.token_counts(idx, m)[m // 2] > 150
    idx, w = P.make_tokens(100, 40, 3, seed=1, exact=True)
    assert np.all(w * P.FRAC == np.round(w * P.FRAC))


def test_dispatch_tables_reach_every_kernel_form():
    """The shape -> kernel-form table at the top of test_gpu_slice_classify.py, recomputed from the LDS formulas of the dispatch."""
    assert sorted((d,) + P.sc_forward_form(d, v, c) for d, v, c in P.WAVE_FWD_CASES) == [(d, "wave", ct) for d in (2, 3) for ct in range(4, 33, 4)]
    assert sorted({(d,) + P.sc_backward_form(d, v, c)[1:] for d, v, c in P.WAVE_BWD_CASES}) == \
        [(d, u, ctl) for d in (2, 3) for u in (1, 2, 3, 4) for ctl in (1, 2)]
    from tests.test_gpu_slice_classify import GENERAL_CASES
    for (d, v, c, n), (fwd, bwd) in GENERAL_CASES.items():
        assert P.sc_forward_form(d, v, c) == fwd, (d, v, c, P.sc_forward_form(d, v, c))
        assert P.sc_backward_form(d, v, c) == bwd, (d, v, c, P.sc_backward_form(d, v, c))
    fw = {f for f, _ in GENERAL_CASES.values()}
    bw = {b for _, b in GENERAL_CASES.values()}
    assert {("v4", pb) for pb in (64, 32, 16)} <= fw and {("scalar", pb) for pb in (64, 32, 16, 8)} <= fw
    assert {(k, pb) for k in ("v4", "scalar") for pb in (64, 32, 16, 8)} <= bw
    # misaligned pointers leave the float4 kernels
    assert P.sc_forward_form(3, 32, 13, aligned=False) == ("scalar", 64) and P.sc_backward_form(3, 32, 13, aligned=False) == ("scalar", 64)


def test_scatter_reference_counts_every_token_once():
    rng = np.random.default_rng(0)
    n, m, d, v = 300, 20, 3, 5
    idx, w = P.make_tokens(n, m, d, seed=2, exact=True)
    g = rng.integers(-3, 4, (n, 1, v)).astype(np.float32)
    old = rng.integers(-4, 5, (m, v)).astype(np.float32)
    ref, bound, _ = P.scatter_backward_reference(g, idx, w, d + 1, old)
    want = old.astype(np.float64)
    for t in range(n * (d + 1)):
        if idx[t] >= 0:
            want[idx[t]] += g[t // (d + 1), 0].astype(np.float64) * float(w[t])
    np.testing.assert_array_equal(ref, want)
    assert np.all(bound[P.token_counts(idx, m) > 0] > 0)


@pytest.mark.parametrize("d,v,c,n", [(3, 32, 13, 293), (2, 96, 20, 69), (5, 7, 3, 1000), (3, 64, 50, 100)])
def test_ordered_logits_are_the_oracles(d, v, c, n):
    from oracle import lattice_oracle as O
    for exact in (False, True):
        inp = P.make_sc_inputs(n, P.table_rows(n), d, v, c, seed=5, exact=exact)
        P.assert_equal_bits(P.sc_forward_reference(inp, n),
                            O.slice_classify(inp["values"], inp["delta_w"], inp["lin_w"], inp["lin_b"], inp["idx"], inp["w"], n), "logits")
