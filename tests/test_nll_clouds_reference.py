"""tests/nll_clouds_reference.py checked without a GPU: the fp64 reference against torch's own nll_loss in float64, the fp32 emulation
against the reference and against glue_reference.nll_emulate, the torch form of losses.NLLLoss / nll_loss_gather(weight=,
points_per_cloud=) against the reference, and LNN.compute_class_weights against its formula."""
import numpy as np
import pytest
import torch

from . import glue_reference as G
from . import nll_clouds_reference as R

# (n, n0, C, ignore_index, ignored shares of the clouds, weights): weights present and absent, an all-ignored cloud, a shorter last cloud
CASES = ((300, 300, 5, None, (0.0,), None), (300, 1000, 5, 2, (0.3,), "random"), (1000, 300, 20, 0, (0.0, 0.5, 1.0, 0.2), None),
         (1000, 300, 20, 0, (0.0, 0.5, 1.0, 0.2), "random"), (901, 300, 3, -100, (0.99, 0.0, 0.5, 0.0), "frequency"),
         (65, 1, 4, 1, (0.0, 1.0), "random"), (2100, 1025, 7, 7, (0.5, 0.0, 0.0), None))


def build(n, n0, c, ignore, shares, kind, seed=0):
    lp = R.log_probs_case(n, c, seed + n + c)
    y = R.labels_case(n, n0, c, ignore, shares, seed + 1, out_of_range=False)  # (torch's nll_loss takes no label outside [0, C))
    return lp, y, R.weights_case(kind, c, seed + 2, y, ignore)


def torch_nll(lp, y, ignore, w):
    """torch.nn.functional.nll_loss in float64; a slice without a counted label gives NaN there (0 / 0): it contributes 0."""
    out = torch.nn.functional.nll_loss(torch.from_numpy(np.asarray(lp, dtype=np.float64)), torch.from_numpy(y),
                                       weight=None if w is None else torch.from_numpy(w.astype(np.float64)),
                                       ignore_index=-100 if ignore is None else ignore, reduction="mean")
    return 0.0 if torch.isnan(out) else float(out)


@pytest.mark.parametrize("case", CASES)
def test_reference_is_the_mean_over_the_clouds_of_torchs_nll_loss(case):
    n, n0, c, ignore, shares, kind = case
    lp, y, w = build(*case)
    if ignore is None:
        assert (y != -100).all()
    ref = R.reference(lp, y, n0, ignore, w)
    ranges = R.cloud_ranges(n, n0)
    assert ref["clouds"] == len(ranges) == -(-n // min(n0, n))
    per = [torch_nll(lp[lo:hi], y[lo:hi], ignore, w) for lo, hi in ranges]
    assert np.allclose(ref["per_cloud"], per, rtol=1e-12, atol=1e-14)
    assert abs(ref["loss"] - sum(per) / len(per)) <= 1e-12 * max(abs(ref["loss"]), 1.0)
    if len(ranges) == 1:
        assert abs(ref["loss"] - torch_nll(lp, y, ignore, w)) <= 1e-12
    empty = [b for b in range(len(ranges)) if shares[b % len(shares)] == 1.0 and ignore is not None]
    assert len(empty) == (0 if 1.0 not in shares else len(ranges) // len(shares))
    for b in empty:  # an all-ignored cloud: loss 0, the backward's divisor 1, no gradient
        assert ref["per_cloud"][b] == 0.0 and ref["weight_sum"][b] == 1.0 and not ref["grad"][ranges[b][0]:ranges[b][1]].any()


@pytest.mark.parametrize("case", CASES)
def test_reference_gradient_is_autograds(case):
    n, n0, c, ignore, shares, kind = case
    lp, y, w = build(*case)
    ref = R.reference(lp, y, n0, ignore, w, grad_loss=0.75)
    x = torch.from_numpy(lp.astype(np.float64)).requires_grad_(True)
    total = 0.0
    for lo, hi in R.cloud_ranges(n, n0):
        if (y[lo:hi] != (-100 if ignore is None else ignore)).any():
            total = total + torch.nn.functional.nll_loss(x[lo:hi], torch.from_numpy(y[lo:hi]), weight=None if w is None else torch.from_numpy(w.astype(np.float64)),
                                                         ignore_index=-100 if ignore is None else ignore)
    (0.75 * total / ref["clouds"]).backward()
    assert np.allclose(ref["grad"], x.grad.numpy(), rtol=1e-12, atol=1e-15)


def test_skewed_case_separates_the_batch_mean_from_the_mean_over_the_clouds():
    lp, y, n0, ignore = R.skewed_case()
    ref = R.reference(lp, y, n0, ignore)
    counted = [(y[lo:hi] != ignore).mean() for lo, hi in R.cloud_ranges(len(y), n0)]
    assert counted[0] == 1.0 and 0.4 < counted[1] < 0.6 and 0.0 < counted[2] < 0.03 and 0.05 < counted[3] < 0.15
    whole = R.batch_wide(lp, y, ignore)
    assert abs(whole - torch_nll(lp, y, ignore, None)) <= 1e-12
    assert abs(whole - ref["loss"]) > 1e-3 * abs(ref["loss"]), (whole, ref["loss"])


@pytest.mark.parametrize("case", CASES)
def test_emulation_is_within_the_counted_bounds_and_repeats_glue_reference(case):
    n, n0, c, ignore, shares, kind = case
    lp, y, w = build(*case)
    y = R.labels_case(n, n0, c, ignore, shares, 1)  # with labels outside [0, C)
    got = R.emulate(lp, y, n0, ignore, w, grad_loss=0.75)
    ratios = R.check(got, lp, y, n0, ignore, w, f"{case}", grad_loss=0.75)
    assert max(ratios.values()) <= 1.0
    if w is None:
        for b, (lo, hi) in enumerate(R.cloud_ranges(n, n0)):
            loss, count = G.nll_emulate(lp[lo:hi], y[lo:hi], ignore)
            assert loss.tobytes() == got["per_cloud"][b].tobytes() and count.tobytes() == got["weight_sum"][b].tobytes()


def test_emulation_of_an_exact_case_is_the_reference():
    for n, n0, c, weighted in ((1000, 300, 3, True), (1000, 300, 20, False), (2100, 1025, 5, True)):
        lp, y, w, g = R.exact_case(n, n0, c, weighted)
        got, ref = R.emulate(lp, y, n0, -100, w, g), R.reference(lp, y, n0, -100, w, g)
        assert np.array_equal(got["weight_sum"].astype(np.float64), ref["weight_sum"])
        assert np.array_equal(got["per_cloud"], ref["per_cloud"].astype(np.float32))  # (one division of exact sums)
        assert max(R.check(got, lp, y, n0, -100, w, "exact", g, ref=ref).values()) <= 1.0


def test_poisoned_inputs_leave_the_reference_unchanged():
    n, n0, c, ignore = 1000, 300, 20, 10
    lp = R.log_probs_case(n, c, 3)
    y = R.labels_case(n, n0, c, ignore, (0.0, 0.5, 1.0, 0.99), 4)
    w = R.weights_case("random", c, 5)
    assert not R.used_classes(y, c, ignore)[ignore]  # labels outside [0, C) clamp to 0 and C - 1, never to the ignored class
    lp2, w2 = R.poisoned(lp, y, ignore, w)
    assert np.isnan(w2[ignore]) and (~np.isfinite(lp2)).sum() == n * c - (y != ignore).sum()
    a, b = R.reference(lp, y, n0, ignore, w), R.reference(lp2, y, n0, ignore, w2)
    assert all(np.array_equal(a[k], b[k]) for k in R.OUTPUTS)


@pytest.mark.parametrize("case", CASES)
def test_torch_form_on_cpu_float64(case):
    from lattice_net_amd.losses import NLLLoss, nll_loss_gather
    n, n0, c, ignore, shares, kind = case
    lp, _, _ = build(*case)
    y = R.labels_case(n, n0, c, ignore, shares, 1)
    w = R.weights_case(kind, c, 2, y, ignore)
    lp, w2 = R.poisoned(lp, y, ignore, w)  # NaN / -inf wherever the formula may not look
    ref = R.reference(lp, y, n0, ignore, w2, grad_loss=0.75)
    wt = None if w2 is None else torch.from_numpy(w2.astype(np.float64))
    for form in ("module", "function"):
        x = torch.from_numpy(lp.astype(np.float64)).requires_grad_(True)
        if form == "module":
            loss = NLLLoss(weight=wt, ignore_index=ignore, points_per_cloud=n0)(x, torch.from_numpy(y))
        else:
            loss = nll_loss_gather(x, torch.from_numpy(y), ignore, weight=wt, points_per_cloud=n0)
        assert loss.dtype == torch.float64 and abs(loss.item() - ref["loss"]) <= 1e-12 * max(abs(ref["loss"]), 1.0), (form, loss.item(), ref["loss"])
        (0.75 * loss).backward()
        assert np.allclose(x.grad.numpy(), ref["grad"], rtol=1e-12, atol=1e-15) and not np.isnan(x.grad.numpy()).any()
    if len(R.cloud_ranges(n, n0)) == 1:  # weight alone: one cloud
        x = torch.from_numpy(lp.astype(np.float64))
        assert abs(float(nll_loss_gather(x, torch.from_numpy(y), ignore, weight=wt)) - ref["loss"]) <= 1e-12 * max(abs(ref["loss"]), 1.0)


def test_torch_form_other_dtypes_and_the_default_path():
    from lattice_net_amd import losses
    lp, y, n0, ignore = R.skewed_case()
    ref = R.reference(lp, y, n0, ignore)
    got = losses.NLLLoss(ignore_index=ignore, points_per_cloud=n0)(torch.from_numpy(lp), torch.from_numpy(y))
    assert got.dtype == torch.float32 and abs(float(got) - ref["loss"]) <= 1e-5 * abs(ref["loss"])
    half = losses.NLLLoss(ignore_index=ignore, points_per_cloud=n0)(torch.from_numpy(lp).bfloat16(), torch.from_numpy(y))
    assert half.dtype == torch.bfloat16 and abs(float(half) - ref["loss"]) <= 0.05 * abs(ref["loss"])
    # neither weight nor points_per_cloud: the former formula, to the bit
    x = torch.from_numpy(lp)
    keep = torch.from_numpy(y) != ignore
    picked = x.gather(1, torch.from_numpy(y).clamp(0, 4).unsqueeze(1)).squeeze(1)
    former = -torch.where(keep, picked, torch.zeros_like(picked)).sum() / keep.sum().clamp(min=1).to(picked.dtype)
    assert torch.equal(losses.nll_loss_gather(x, torch.from_numpy(y), ignore), former)
    assert torch.equal(losses.NLLLoss(ignore_index=ignore)(x, torch.from_numpy(y)), former)
    assert "NLLLoss" in losses.__all__
    from latticenet_py.lattice.lovasz_loss import LovaszSoftmax, NLLLoss
    assert NLLLoss is losses.NLLLoss and LovaszSoftmax is losses.LovaszSoftmax
    assert float(losses.NLLLoss(points_per_cloud=3)(torch.zeros((0, 4)), torch.zeros((0,), dtype=torch.int64))) == 0.0
    with pytest.raises(ValueError):
        losses.NLLLoss(points_per_cloud=0)
    with pytest.raises(ValueError):
        losses.nll_loss_gather(x, torch.from_numpy(y), weight=torch.ones(3))


def test_compute_class_weights_is_the_formula():
    from lattice_net_amd.models import LNN
    freq = np.array([0.5, 0.0, 0.25, 1e-6, 0.2499, 1.0], dtype=np.float64)
    net = LNN.__new__(LNN)  # (the method needs the model's device only)
    torch.nn.Module.__init__(net)
    net._device = torch.device("cpu")
    for f in (freq, freq.astype(np.float32), torch.from_numpy(freq)):
        w = net.compute_class_weights(f, 2)
        assert w.dtype == torch.float32 and w.device.type == "cpu" and w.shape == (6,)
        want = 1.0 / np.log(1.05 + freq)
        want[2] = 1e-8
        assert np.allclose(w.numpy().astype(np.float64), want, rtol=5e-6, atol=0.0)  # 1.05 + f rounded to float32 (1.2e-7) moves log(1.05) = 0.0488 by 2.4e-6 of itself
        assert np.allclose(w.numpy(), R.class_weights(freq, 2), rtol=5e-6)
    assert abs(float(w[1]) - 20.4959) < 1e-3 and abs(float(w[5]) - 1.39297) < 1e-4
