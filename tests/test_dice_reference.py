"""CPU checks around the generalized soft Dice loss: tests/dice_reference.py reproduces fixture F13 and its fp32 emulation of
csrc/ln_dice.hip stays inside the counted bounds; the torch form of GeneralizedSoftDiceLoss(points_per_cloud=) is the mean of the
clouds' single-cloud losses and points_per_cloud=None is the former formula bit for bit; the host half of the C ABI (workspace size,
refusals) works without a GPU."""
import numpy as np
import pytest
import torch

from lattice_net_amd import _lib
from lattice_net_amd.losses import GeneralizedSoftDiceLoss

from . import dice_reference as R


def test_reference_reproduces_f13(golden):
    f = golden("F13_losses")
    names = [str(x) for x in f["case_names"]]
    assert names
    for name in names:
        lp, labels, ignore = f[f"{name}/logp"], f[f"{name}/labels"], int(f[f"{name}/ignore"])
        ref = R.reference(lp.astype(np.float64), labels, None, ignore)
        fx = float(f[f"{name}/dice"])
        assert abs(ref["loss"] - fx) <= 5e-6 * max(abs(fx), 1.0), (name, ref["loss"], fx)
        g_ref = f[f"{name}/dice_grad"].astype(np.float64)
        assert np.max(np.abs(ref["grad"] - g_ref)) <= 1e-5 * max(np.max(np.abs(g_ref)), 1e-30), name
        assert ref["per_cloud"].shape == (1,) and ref["per_cloud"][0] == ref["loss"]


def test_reference_gradient_is_the_derivative_of_its_loss():
    lp, y = R.inputs(23, 5, 1).astype(np.float64), R.labels(23, 5, 1, "wild")
    for n0, ignore in ((None, None), (7, 2)):
        ref = R.reference(lp, y, n0, ignore)
        for i, c in ((0, 0), (5, 2), (22, 4), (8, 3)):
            h = np.zeros_like(lp)
            h[i, c] = 1e-6
            num = (R.reference(lp + h, y, n0, ignore)["loss"] - R.reference(lp - h, y, n0, ignore)["loss"]) / 2e-6
            assert abs(num - ref["grad"][i, c]) <= 1e-9, (n0, i, c)


@pytest.mark.parametrize("n,c,n0,ignore,family,kind", [
    (1, 1, None, None, "softmax", "random"), (1000, 20, None, 0, "softmax", "wild"), (257, 33, 7, 40, "onehot", "absent"),
    (65, 255, None, None, "softmax", "one"), (256, 256, 1, 0, "softmax", "wild"), (300, 257, 7, None, "onehot", "wild"),
    (1000, 1024, 300, 3, "softmax", "random"), (R.rows_past_the_tile_cap(64), 64, None, 1, "softmax", "random")])
def test_emulation_is_inside_the_bounds(n, c, n0, ignore, family, kind):
    lp, y = R.inputs(n, c, n + c, family), R.labels(n, c, 3, kind)
    scale = float(np.float32(-0.37))
    R.check(R.emulate(lp, y, n0, ignore, grad_loss=scale), lp, y, n0, ignore, f"{(n, c, n0)}", grad_loss=scale)


def test_exact_inputs_give_exact_counts_in_the_emulation_and_a_planted_fault_is_caught():
    lp, y = R.inputs(1000, 3, 2, "exact"), R.labels(1000, 3, 2)
    got = R.emulate(lp, y, 300, 0)
    ref = R.reference(lp, y, 300, 0)
    assert np.array_equal(got["stats"], ref["stats"]) and not np.isnan(got["grad"]).any()
    got["stats"][1, 0, 1] += 1.0
    with pytest.raises(AssertionError, match="error / bound"):
        R.check(got, lp, y, 300, 0, ref=ref)
    lp, y = R.inputs(1000, 20, 2), R.labels(1000, 20, 2)
    got = R.emulate(lp, y, None, 0)
    got["grad"][17, 3] *= np.float32(1.0 + 2.0 ** -12)
    with pytest.raises(AssertionError, match="error / bound"):
        R.check(got, lp, y, None, 0)


def test_tiling_covers_a_cloud_and_the_cap_is_where_the_tiles_grow():
    for c in (1, 2, 19, 20, 32, 33, 64, 255, 256, 257, 1024):
        step_rows = R.tiling(1, c)[0]
        assert step_rows == (256 // c if c <= 256 else 1)
        edge = R.rows_past_the_tile_cap(c)
        for length in (1, step_rows, step_rows + 1, edge - 1, edge, 3 * edge + 5):
            sr, tile_rows, tiles = R.tiling(length, c)
            assert tile_rows % sr == 0 and (tiles - 1) * tile_rows < length <= tiles * tile_rows and tiles <= R.LN_DICE_MAX_TILES
        assert R.tiling(edge - 1, c)[1] == step_rows * R.LN_DICE_STEPS < R.tiling(edge, c)[1]


def _old_formula(output, target, ignore_index):
    """GeneralizedSoftDiceLoss.forward as it stood before points_per_cloud existed."""
    nr_classes = output.shape[1]
    probs = output.exp()
    target = target.reshape(-1)
    picked = probs.gather(1, target.unsqueeze(1)).squeeze(1)
    intersection = torch.zeros(nr_classes, dtype=probs.dtype, device=probs.device).index_add_(0, target, picked)
    counts = torch.zeros(nr_classes, dtype=probs.dtype, device=probs.device).index_add_(0, target, torch.ones_like(picked))
    union = probs.sum(0) + counts
    loss_per_class = 1.0 - 2.0 * intersection / (union + 1e-6)
    if ignore_index is not None:
        weight = (torch.arange(nr_classes, device=probs.device) != int(ignore_index)).to(probs.dtype)
        loss_per_class = loss_per_class * weight
    return loss_per_class.sum() / nr_classes


def test_points_per_cloud_none_is_the_former_formula_bit_for_bit():
    for dtype in (torch.float32, torch.float64):
        for n, c, ignore in ((10, 4, None), (257, 20, 0), (1, 1, None), (0, 3, 1)):
            lp = torch.from_numpy(R.inputs(n, c, n)).to(dtype)
            y = torch.from_numpy(R.labels(n, c, n))
            got = []
            for fn in (lambda x: GeneralizedSoftDiceLoss(ignore_index=ignore)(x, y), lambda x: _old_formula(x, y, ignore)):
                x = lp.clone().requires_grad_(True)
                loss = fn(x)
                loss.backward()
                got.append((loss.detach().numpy().tobytes(), x.grad.numpy().tobytes()))
            assert got[0] == got[1], (dtype, n, c)


@pytest.mark.parametrize("n,n0", [(10, 4), (10, 1), (10, 10), (10, 25), (12, 4), (0, 4)])
def test_torch_form_per_cloud_is_the_mean_of_the_single_cloud_calls(n, n0):
    c = 5
    for ignore in (None, 2, 9):
        lp = torch.from_numpy(R.inputs(n, c, 3 * n + 1)).double()
        y = torch.from_numpy(R.labels(n, c, n, "absent" if ignore == 2 else "random"))
        x = lp.clone().requires_grad_(True)
        loss = GeneralizedSoftDiceLoss(ignore_index=ignore, points_per_cloud=n0)(x, y)
        loss.backward()
        ranges = R.cloud_ranges(n, n0)
        xs = lp.clone().requires_grad_(True)
        single = GeneralizedSoftDiceLoss(ignore_index=ignore)
        mean = sum(single(xs[lo:hi], y[lo:hi]) for lo, hi in ranges) / len(ranges) if ranges else xs.sum() * 0.0
        mean.backward()
        assert abs(loss.item() - mean.item()) <= 1e-12 and loss.dtype == torch.float64
        assert x.grad.shape == (n, c) and (n == 0 or float((x.grad - xs.grad).abs().max()) <= 1e-12)
        ref = R.reference(lp.numpy(), y.numpy(), n0, ignore)
        assert abs(loss.item() - ref["loss"]) <= 1e-12 and (n == 0 or np.max(np.abs(x.grad.numpy() - ref["grad"])) <= 1e-12)
    with pytest.raises(ValueError):
        GeneralizedSoftDiceLoss(points_per_cloud=0)


def test_workspace_size_is_a_pure_host_function_and_total():
    lib = _lib.load()
    for n in (0, 1, 255, 120000, (1 << 31) - 1, 1 << 40, -5):
        for n0 in (-3, 0, 1, 7500, (1 << 31) - 1, 1 << 40):
            for c in (-5, 0, 1, 20, 256, 257, 1024, 5000):
                assert lib.ln_dice_workspace_bytes(n, n0, c) >= 256
    # room for one [3, C] partial per tile of every cloud and the class terms
    n, n0, c = 120000, 7500, 20
    tiles = R.tiling(n0, c)[2]
    assert lib.ln_dice_workspace_bytes(n, n0, c) >= 16 * (tiles * 3 * c * 4 + c * 4)
    assert lib.ln_dice_workspace_bytes(n, n, c) >= R.tiling(n, c)[2] * 3 * c * 4 + c * 4
    assert lib.ln_dice_workspace_bytes(n, n0, c) <= 24 * n * c + 16 * 16 * c + 1024


def test_argument_errors_are_reported_not_fatal():
    """Refusals come before any GPU call: null pointers and bad sizes return LN_ERR_ARG with a message, on a machine without a GPU too."""
    lib = _lib.load()
    one = 8  # a non-null pointer that is never followed: every call below is refused before a launch

    def fwd(n=10, n0=4, c=3, lp=one, y=one, ws=one, ws_bytes=1 << 30, loss=one, coef=one):
        return lib.ln_dice_forward(lp, y, n, n0, c, 0, ws, ws_bytes, loss, None, None, coef, None)

    def bwd(n=10, n0=4, c=3, lp=one, y=one, coef=one, g=one, out=one):
        return lib.ln_dice_backward(lp, y, coef, g, n, n0, c, out, None)

    for call, text in ((lambda: fwd(c=0), b"bad sizes"), (lambda: fwd(c=1025), b"bad sizes"), (lambda: fwd(n=-1), b"bad sizes"),
                       (lambda: fwd(n0=0), b"points_per_cloud"), (lambda: fwd(n=(1 << 31) // 3 + 1), b"2^31"),
                       (lambda: fwd(n=R.MAX_CLOUDS + 1, n0=1), b"at most 65535"), (lambda: fwd(n=2 * R.MAX_CLOUDS + 1, n0=2), b"at most 65535"),
                       (lambda: fwd(loss=None), b"null buffer"), (lambda: fwd(lp=None), b"null buffer"), (lambda: fwd(y=None), b"null buffer"),
                       (lambda: fwd(coef=None), b"null buffer"), (lambda: fwd(ws=None), b"workspace"),
                       (lambda: fwd(ws_bytes=lib.ln_dice_workspace_bytes(10, 4, 3) - 1), b"workspace"),
                       (lambda: fwd(n=0, loss=None), b"null buffer"),
                       (lambda: bwd(c=0), b"bad sizes"), (lambda: bwd(c=1025), b"bad sizes"), (lambda: bwd(n0=0), b"points_per_cloud"),
                       (lambda: bwd(n=R.MAX_CLOUDS + 1, n0=1), b"at most 65535"), (lambda: bwd(lp=None), b"null buffer"),
                       (lambda: bwd(y=None), b"null buffer"), (lambda: bwd(coef=None), b"null buffer"), (lambda: bwd(g=None), b"null buffer"),
                       (lambda: bwd(out=None), b"null buffer")):
        assert call() == -1 and text in lib.ln_last_error_string(), lib.ln_last_error_string()
    assert bwd(n=0, lp=None, y=None, coef=None, g=None, out=None) == 0  # no points: nothing to write, nothing launched
    with pytest.raises(_lib.LatticeNetHipError, match="ln_dice_forward"):
        _lib.check(fwd(c=0), "ln_dice_forward")
    names = lib.ln_kernel_names().decode().split(",")
    assert {"k_dice_partials", "k_dice_finish", "k_dice_backward"} <= set(names)
