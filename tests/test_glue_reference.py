"""tests/glue_reference.py checked on the CPU (no GPU, no marker): the fp64 references agree with torch's float64 autograd, a faithful
fp32 emulation of the kernels' summation order stays within every bound at the shapes the GPU tests run, every exact case is exactly
representable, the label semantics are those of the gather formulation, and the results of wrong sums and wrong label handling do
not pass."""
import numpy as np
import pytest
import torch

from tests import glue_reference as G
from tests.dense_reference import assert_equal_bits, assert_exact, assert_within, worst_ratio


# ------------------------------------------------------------------------------------------------------------------ against torch fp64
@pytest.mark.parametrize("rows,cols,g_dim", [(7, 5, 0), (7, 5, 1), (1, 9, 1), (9, 1, 0), (64, 3, 0), (3, 65, 1)])
def test_weight_norm_reference_agrees_with_torch_float64(rows, cols, g_dim):
    v_np, g_np, gw_np = G.wn_random_case(rows, cols, g_dim, rows * 31 + cols)
    v = torch.from_numpy(v_np).double().requires_grad_(True)
    g = torch.from_numpy(g_np).double().reshape((rows, 1) if g_dim == 0 else (1, cols)).requires_grad_(True)
    w = v * (g / v.norm())
    w.backward(torch.from_numpy(gw_np).double())
    (w_ref, n_ref, gv_ref, gg_ref), _ = G.weight_norm_reference(v_np, g_np, g_dim, gw_np)
    assert_within(w, w_ref, 1e-14, "w")
    assert_within(v.norm(), n_ref, 1e-13, "norm")
    assert_within(v.grad, gv_ref, 1e-14, "grad_v")
    assert_within(g.grad.reshape(-1), gg_ref, 1e-13, "grad_g")


@pytest.mark.parametrize("ignore", [None, -100, 2])
@pytest.mark.parametrize("n,classes", [(1, 3), (40, 5), (257, 20)])
def test_nll_reference_agrees_with_torch_float64(n, classes, ignore):
    lp_np, target_np = G.nll_random_case(n, classes, ignore, n + classes, out_of_range=False)
    lp = torch.from_numpy(lp_np).double().requires_grad_(True)
    loss = torch.nn.functional.nll_loss(lp, torch.from_numpy(target_np), ignore_index=-(1 << 40) if ignore is None else ignore)
    loss_ref, count, grad_ref, _ = G.nll_reference(lp_np, target_np, ignore, 3.0)
    if ignore is not None and bool((target_np == ignore).all()):
        assert loss_ref == 0.0 and count == 1.0 and not grad_ref.any()  # (torch: 0 / 0)
        return
    (3.0 * loss).backward()
    assert_within(loss, loss_ref, 1e-14, "loss")
    assert_within(lp.grad, grad_ref, 1e-15, "grad")


# ------------------------------------------------------------------------------------------------------------------ label semantics
def six_rows():
    lp = np.array([[-1.0, -2.0, -4.0], [-8.0, -16.0, -32.0], [-0.5, -0.25, -0.125], [-3.0, -5.0, -7.0], [-9.0, -10.0, -11.0], [-64.0, -128.0, -256.0]],
                  np.float32)
    return lp, np.array([1, -1, 3, -100, 10, 2], np.int64)  # in range, below (-> 0), C (-> 2), the ignore value, C + 7 (-> 2), last class


def test_clamp_and_ignore_on_six_rows():
    lp, target = six_rows()
    loss, count, grad, sum_abs = G.nll_reference(lp, target, -100, 2.0)
    picked = [-2.0, -8.0, -0.125, -11.0, -256.0]
    assert count == 5.0 and loss == -sum(picked) / 5 and sum_abs == -sum(picked)
    want = np.zeros((6, 3))
    for row, col in ((0, 1), (1, 0), (2, 2), (4, 2), (5, 2)):
        want[row, col] = -2.0 / 5
    assert np.array_equal(grad, want)
    # an out-of-range value that is the ignore_index is ignored, not clamped; without an ignore_index every row counts
    loss, count, grad, _ = G.nll_reference(lp, target, 10, 1.0)
    assert count == 5.0 and loss == (2.0 + 8.0 + 0.125 + 3.0 + 256.0) / 5 and not grad[4].any() and grad[3, 0] == -0.2
    loss, count, _, _ = G.nll_reference(lp, target, None, 1.0)
    assert count == 6.0 and loss == (2.0 + 8.0 + 0.125 + 3.0 + 11.0 + 256.0) / 6
    # every label ignored
    loss, count, grad, sum_abs = G.nll_reference(lp, np.full(6, 1, np.int64), 1, 1.0)
    assert loss == 0.0 and count == 1.0 and sum_abs == 0.0 and not grad.any()


@pytest.mark.parametrize("ignore", [None, -100, 10, 1])
def test_torch_fallback_has_the_reference_label_semantics(ignore):
    """losses.nll_loss_gather on CPU tensors (the gather formulation every non-float32-CUDA input takes) against the reference, loss
    and gradient, on the six rows; with a -inf and a NaN planted in an ignored row and in non-target columns it must not move."""
    from lattice_net_amd.losses import nll_loss_gather
    lp_np, target = six_rows()
    for planted in (False, True):
        lp_np = lp_np.copy()
        if planted:
            lp_np[0, 0], lp_np[5, 1] = -np.inf, np.nan
            if ignore is not None:
                rows = np.nonzero(target == ignore)[0]
                lp_np[rows] = -np.inf
        loss_ref, _, grad_ref, _ = G.nll_reference(lp_np, target, ignore, 1.0)
        lp = torch.from_numpy(lp_np).double().requires_grad_(True)
        loss = nll_loss_gather(lp, torch.from_numpy(target), ignore)
        loss.backward()
        assert_within(loss, loss_ref, 1e-14, f"loss ignore={ignore} planted={planted}")
        assert_within(lp.grad, grad_ref, 1e-15, f"grad ignore={ignore} planted={planted}")


# ------------------------------------------------------------------------------------------------------------------ emulation within bounds
hold_weight_norm = G.assert_weight_norm


def merge(worst, ratios):
    for k, r in ratios.items():
        worst[k] = max(r, worst.get(k, 0.0))


def test_weight_norm_emulation_is_within_every_bound():
    worst = {}
    for rows, cols, g_dim in G.wn_shapes() + [G.WN_LARGEST]:
        for scale in (1.0,) if rows * cols > (1 << 20) else (1.0, 2.0 ** -20, 2.0 ** 20):
            v, g, gw = G.wn_random_case(rows, cols, g_dim, rows * 7 + cols + g_dim, scale)
            merge(worst, hold_weight_norm(G.weight_norm_emulate(v, g, g_dim, gw), v, g, g_dim, gw, f"{rows}x{cols} g_dim={g_dim} scale={scale}"))
    print(f"weight norm emulation: worst error / bound {worst}")
    assert max(worst.values()) <= 1.0


def test_weight_norm_scaling_by_a_power_of_two_is_exact():
    """Every operator on the path scales exactly with v * 2^s while nothing under- or overflows: w and grad_g keep their bits,
    grad_v * 2^s is grad_v."""
    rows, cols, g_dim = 65, 17, 0
    v, g, gw = G.wn_random_case(rows, cols, g_dim, 5)
    base = G.weight_norm_emulate(v, g, g_dim, gw)
    for s in (2.0 ** -20, 2.0 ** 20):
        vs, gs, gws = G.wn_random_case(rows, cols, g_dim, 5, s)
        assert np.array_equal(vs, v * np.float32(s)) and np.array_equal(gws, gw)
        out = G.weight_norm_emulate(vs, gs, g_dim, gws)
        assert_equal_bits(out[0], base[0], "w")
        assert_equal_bits(out[1], base[1] * np.float32(s), "norm")
        assert_equal_bits(out[2] * np.float32(s), base[2], "grad_v")
        assert_equal_bits(out[3], base[3], "grad_g")


def test_weight_norm_cancellation_makes_the_bound_tight():
    """The drawn gw makes the two terms of grad_v cancel: the result is far smaller than either, which is what an absolute tolerance
    on the largest element cannot see."""
    v, g, gw = G.wn_random_case(64, 65, 0, 1)
    (_, _, gv, _), mags = G.weight_norm_reference(v, g, 0, gw)
    assert np.median(np.abs(gv)) < 0.01 * np.median(mags["gv_direct"])


def test_weight_norm_bounds_reject_wrong_sums():
    """What a kernel with a wrong sum would return, produced by running the faithful emulation on altered inputs and held to the
    reference of the true ones: the last element missing from the sum of squares (exact cases: the norm is no longer 2^k); the last
    lane missing from the fold of the dot products (gw zeroed at k = lanes - 1 mod lanes: grad_g leaves its bound)."""
    for rows, cols, g_dim in ((3, 341, 0), (25, 41, 1), (65, 16, 0), (4, 1000, 1)):
        v, g, gw, ref = G.wn_exact_case(rows, cols, g_dim)
        short = v.copy()
        short.reshape(-1)[-1] = 0
        assert G.weight_norm_emulate(short, g, g_dim)[1] != ref[1]
        assert G.weight_norm_emulate(v, g, g_dim)[1] == ref[1]
        v, g, gw = G.wn_random_case(rows, cols, g_dim, 3)
        J, K = G.wn_jk(rows, cols, g_dim)
        lanes = G.wn_lanes(J)
        fewer = G.wn_as_jk(gw.copy(), g_dim)  # (a view: the writes land in the copy)
        fewer[:, np.arange(K) % lanes == lanes - 1] = 0
        fewer = fewer if g_dim == 0 else fewer.T
        ref, mags = G.weight_norm_reference(v, g, g_dim, gw)
        bound = G.weight_norm_bounds(rows, cols, g_dim, mags)["grad_g"]
        assert_within(G.weight_norm_emulate(v, g, g_dim, gw)[3], ref[3], bound, "faithful grad_g")
        with pytest.raises(AssertionError):
            assert_within(G.weight_norm_emulate(v, g, g_dim, fewer)[3], ref[3], bound, "grad_g without the last lane")


def nll_cases():
    for n in G.NLL_N_SMALL:
        for classes in G.NLL_CLASSES_SMALL:
            yield n, classes
    for n, classes in zip(G.NLL_N_LARGE, (2, 5, 2)):
        yield n, classes


def test_nll_emulation_is_within_the_bound():
    worst = 0.0
    for n, classes in nll_cases():
        for ignore in G.nll_ignore_modes(classes):
            lp, target = G.nll_random_case(n, classes, ignore, n + classes)
            loss_ref, count_ref, _, sum_abs = G.nll_reference(lp, target, ignore)
            loss, count = G.nll_emulate(lp, target, ignore)
            assert float(count) == count_ref, (n, classes, ignore)
            bound = G.nll_loss_bound(n, count_ref, sum_abs)
            assert_within(loss, loss_ref, bound, f"n={n} C={classes} ignore={ignore}")
            worst = max(worst, worst_ratio(loss, loss_ref, bound))
    print(f"NLL emulation: worst error / bound {worst}")
    assert worst <= 1.0


def test_nll_checks_reject_wrong_label_handling():
    """The faithful emulation on altered labels, held to the reference of the true ones: out-of-range labels skipped instead of
    clamped; the rows behind the first trip of the grid-stride loop (blocks * 256 rows) never visited.  The count gives both away."""
    lp, target = G.nll_random_case(257, 5, -100, 1)
    _, count_ref, _, _ = G.nll_reference(lp, target, -100)
    skipped = np.where((target < 0) | (target >= 5), -100, target)
    assert float(G.nll_emulate(lp, target, -100)[1]) == count_ref
    assert float(G.nll_emulate(lp, skipped, -100)[1]) != count_ref
    for n, wrong in ((256, False), (257, True), (524289, True)):
        lp, target = G.nll_random_case(n, 2, -100, 2)
        _, count_ref, _, _ = G.nll_reference(lp, target, -100)
        first_trip = target.copy()
        first_trip[G.nll_blocks(n) * G.LN_NLL_THREADS:] = -100
        assert (float(G.nll_emulate(lp, first_trip, -100)[1]) != count_ref) == wrong


# ------------------------------------------------------------------------------------------------------------------ exact cases
def test_every_weight_norm_exact_case_is_representable_and_the_emulation_reproduces_it():
    kept = 0
    for rows, cols, g_dim in G.wn_shapes() + [G.WN_LARGEST]:
        case = G.wn_exact_case(rows, cols, g_dim)
        if case is None:
            continue
        kept += 1
        v, g, gw, ref = case
        assert set(np.unique(v)) <= {-1.0, 0.0, 1.0} and v.reshape(-1)[-1] != 0
        nz = int(np.count_nonzero(v))
        assert nz & (nz - 1) == 0 and (nz.bit_length() - 1) % 2 == 0  # 4^k
        assert_exact(ref[1], np.float64(2 ** ((nz.bit_length() - 1) // 2)), "norm")
        out = G.weight_norm_emulate(v, g, g_dim, gw)
        for name, o, r in zip(("w", "norm", "grad_v", "grad_g"), out, ref):
            assert np.array_equal(np.asarray(r).astype(np.float32).astype(np.float64), r), name
            assert_equal_bits(o, np.asarray(r, np.float32), f"{rows}x{cols} g_dim={g_dim} {name}")
    assert kept == len(G.wn_shapes()) + 1  # none is dropped today; a generator change that drops one shows up here


def test_every_nll_exact_case_is_representable_and_the_emulation_reproduces_it():
    for n, classes in nll_cases():
        case = G.nll_exact_case(n, classes)
        assert case is not None, (n, classes)
        lp, target, grad_loss, (loss, count, grad, sum_abs) = case
        assert int(count) == count and int(count) & (int(count) - 1) == 0
        assert np.float64(np.float32(loss)) == loss and sum_abs < 2 ** 24
        assert np.array_equal(grad.astype(np.float32).astype(np.float64), grad)
        got_loss, got_count = G.nll_emulate(lp, target, -100)
        assert float(got_loss) == loss and float(got_count) == count, (n, classes)


def test_nll_emulation_reproduces_the_recorded_bits_of_the_one_cloud_call():
    """tests/golden/nll_one_cloud_bits.json (glue_reference.nll_golden_cases): the emulation of a cloud's sum gives the two loss_count
    words the kernels of the earlier, separate one-cloud family wrote, the sign of a zero loss included."""
    cases = 0
    for case, lp, target, _ in G.nll_golden_cases():
        loss, count = G.nll_emulate(lp, target, case["ignore"])
        got = np.array([loss, count], np.float32).view(np.uint32)
        assert [int(got[0]), int(got[1])] == case["loss_count"], (case, got)
        cases += 1
    assert cases == 9 * (3 * 3 + 1)
