"""CPU checks of tests/lovasz_reference.py: the fp32 emulation of csrc/ln_lovasz.hip stays inside every bound on every input family
of test_gpu_lovasz.py, the fp64 reference agrees with LovaszSoftmax in float64 on fixture F13, and planted faults are caught."""
import numpy as np
import pytest
import torch

from lattice_net_amd.losses import LovaszSoftmax

from . import lovasz_reference as R

TILE = R.LN_LV_TILE
SIZES = [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 903]


def _emulated(lp, y, ignore, red, what, gradient=True, fault=None):
    return R.check(R.emulate(lp, y, ignore, red, fault=fault), lp, y, ignore, red, what, gradient=gradient)


@pytest.mark.parametrize("n", SIZES)
def test_emulation_is_inside_the_bounds_on_separated_errors(n):
    for c, ignore, red in ((1, None, "mean"), (2, 0, "sum"), (3, 7, "mean"), (20, 0, "mean")):
        y = R.labels(n, c, n + c, out_of_range=(c == 3))
        lp = R.separated(n, c, 11 * n + c)
        assert n == 1 or R.separation(lp, y) >= 0.25 / (n + 1) > 2.0 ** -20
        _emulated(lp, y, ignore, red, f"separated n={n} c={c}")


def test_emulation_is_inside_the_bounds_with_absent_and_single_classes():
    n, c = 2 * TILE + 903, 3
    lp = R.separated(n, c, 5)
    _emulated(lp, R.labels(n, c, 1, absent=1), 0, "mean", "class 1 absent")
    _emulated(lp, R.labels(n, c, 1, all_one=2), None, "mean", "all points in class 2")
    _emulated(lp, R.labels(n, c, 1, all_one=0), 0, "mean", "all points in the ignore class")


@pytest.mark.parametrize("mode", ["right", "wrong", "mixed"])
def test_emulation_is_inside_the_bounds_on_exact_ties(mode):
    for n, c in ((1, 2), (65, 3), (TILE + 1, 3), (2 * TILE + 903, 20)):
        lp, y = R.ties(n, c, n, mode)
        _emulated(lp, y, 0, "mean", f"ties {mode} n={n} c={c}")


def test_emulation_is_inside_the_loss_bounds_on_softmax_of_random_logits():
    for n, c in ((65, 3), (2 * TILE + 903, 20)):
        lp = R.softmax_random(n, c, n)
        _emulated(lp, R.labels(n, c, 3), 0, "mean", f"softmax n={n}", gradient=False)


def test_reference_agrees_with_float64_lovasz_softmax_on_f13(golden):
    f = golden("F13_losses")
    for name in [str(x) for x in f["case_names"]]:
        lp, labels, ignore = f[f"{name}/logp"], f[f"{name}/labels"], int(f[f"{name}/ignore"])
        for red in ("mean", "sum"):
            x = torch.from_numpy(lp).double().clone().requires_grad_(True)
            loss = LovaszSoftmax(ignore_index=ignore, reduction=red)(x, torch.from_numpy(labels))
            loss.backward()
            ref_loss, _, ref_grad = R.reference(lp.astype(np.float64), labels, ignore, red)
            assert abs(loss.item() - ref_loss) <= 5e-6 * max(abs(ref_loss), 1.0), (name, red, loss.item(), ref_loss)
            g = x.grad.numpy()
            assert np.max(np.abs(g - ref_grad)) <= 3e-5 * max(np.max(np.abs(ref_grad)), 1e-30), (name, red)
            # and with the fixture itself (the reference project's float32 run), F13's float64 tolerances
            fx = float(f[f"{name}/lovasz_{red}"])
            assert abs(ref_loss - fx) <= 5e-6 * max(abs(fx), 1.0), (name, red)


def _caught(lp, y, ignore, red, fault):
    with pytest.raises(AssertionError, match="error / bound"):
        _emulated(lp, y, ignore, red, fault, fault=fault)


def test_planted_faults_are_caught():
    n, c = 2 * TILE + 903, 3
    lp_t, y_t = R.ties(n, c, 4, "mixed")
    _emulated(lp_t, y_t, 0, "mean", "ties, no fault")
    _caught(lp_t, y_t, 0, "mean", "unstable_ties")
    lp, y = R.separated(n, c, 9), R.labels(n, c, 2, absent=1)
    _emulated(lp, y, 0, "mean", "separated, no fault")
    _caught(lp, y, 0, "mean", "ignore_counted")
    _caught(lp, y, 0, "mean", "absent_counted")
    _caught(lp, y, 0, "mean", "tile_last_dropped")
    # the last element of a partial tile (one class: it is a foreground element, whose coefficient is not 0)
    _caught(R.separated(64, 1, 1), R.labels(64, 1, 1), None, "sum", "tile_last_dropped")


def test_fp32_jaccard_difference_misses_the_gradient_bound_at_workload_size(capsys):
    n, c = 120000, 2
    lp, y = R.separated(n, c, 3), R.labels(n, c, 3)
    assert R.separation(lp, y) >= 0.25 / (n + 1) > 2.0 ** -20
    ratios = _emulated(lp, y, None, "mean", "closed form")
    _caught(lp, y, None, "mean", "jaccard_difference")
    # the figure (not an assertion): the torch form in float32 against the same bound
    x = torch.from_numpy(lp).clone().requires_grad_(True)
    LovaszSoftmax(ignore_index=None)(x, torch.from_numpy(y)).backward()
    _, _, ref_grad = R.reference(lp, y, None, "mean")
    miss = R.worst_ratio(x.grad.numpy(), ref_grad, R.grad_bound(ref_grad))
    with capsys.disabled():
        print(f"\n[lovasz] n={n}: emulated kernels error/bound (loss, per class, gradient) = {ratios[0]:.3f}, {ratios[1]:.3f}, {ratios[2]:.3f}; "
              f"torch float32 form misses the gradient bound by a factor {miss:.3g}")
