"""losses.SegmentationLoss and losses.log_softmax on CPU tensors: the loss from logits and its gradient are the function the fp64
references of the three pieces describe (head_reference.py, lovasz_reference.py, nll_clouds_reference.py chained by hand), one cloud and
per cloud, with and without class weights, with one of the two losses switched off; and the reference's own LovaszSoftmax on F13."""
import numpy as np
import pytest
import torch

from . import head_reference as H
from . import lovasz_reference as LR
from . import nll_clouds_reference as NR


def test_log_softmax_and_special_values():
    from lattice_net_amd.losses import log_softmax
    x = H.logits_case(6, 20, 3)
    x[1, :] = -np.inf
    x[3, 7] = np.nan
    x[4, :5] = -np.inf
    ref = H.forward_reference(x)
    got = log_softmax(torch.from_numpy(x).double()).numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(ref[[1, 3]]).all() and np.isneginf(got[4, :5]).all()
    fin = np.isfinite(ref)
    assert np.max(np.abs(got[fin] - ref[fin])) <= 1e-13
    g = H.logits_case(6, 20, 4, spread=1.0).astype(np.float64)
    xx = torch.from_numpy(x[[0, 2, 5]]).double().requires_grad_(True)
    log_softmax(xx).backward(torch.from_numpy(g[[0, 2, 5]]))
    assert np.max(np.abs(xx.grad.numpy() - H.backward_reference(ref[[0, 2, 5]], g[[0, 2, 5]]))) <= 1e-13


def _composed(logits, y, ignore, lw, nw, w, n0):
    from lattice_net_amd.losses import SegmentationLoss
    x = torch.from_numpy(np.array(logits)).requires_grad_(True)
    m = SegmentationLoss(ignore, lovasz_weight=lw, nll_weight=nw, class_weight=None if w is None else torch.from_numpy(w), points_per_cloud=n0)
    loss = m(x, torch.from_numpy(y))
    loss.backward()
    return float(loss.detach()), x.grad.numpy()


@pytest.mark.parametrize("n0", (None, 100))
@pytest.mark.parametrize("weighted", (False, True))
def test_segmentation_loss_is_the_fp64_function(n0, weighted):
    """In float64 against the references to 1e-12 of the largest magnitude, in float32 to 1e-5."""
    n, c, ignore = 257, 7, 2
    x = H.logits_case(n, c, 41, spread=2.0).astype(np.float64)
    y = H.labels_case(n, c, 41, ignore)
    w = H.weights_case(c, 3) if weighted else None
    lp = H.forward_reference(x)
    ranges = NR.cloud_ranges(n, n if n0 is None else n0)
    lov, dl = 0.0, np.zeros((n, c))
    for lo, hi in ranges:
        l, _, d = LR.reference(lp[lo:hi], y[lo:hi], ignore, "mean")
        lov += l / len(ranges)
        dl[lo:hi] = d / len(ranges)
    nll = NR.reference(lp, y, n if n0 is None else n0, ignore, w)
    for lw, nw in ((0.5, 0.5), (1.0, 0.0), (0.0, 2.0)):
        ref_loss = lw * lov + nw * nll["loss"]
        ref_grad = H.backward_reference(lp, lw * dl + nw * nll["grad"])
        loss, grad = _composed(x, y, ignore, lw, nw, w, n0)
        assert abs(loss - ref_loss) <= 1e-12 * max(abs(ref_loss), 1.0), (lw, nw)
        assert np.max(np.abs(grad - ref_grad)) <= 1e-12 * max(np.max(np.abs(ref_grad)), 1e-30), (lw, nw)
        loss32, grad32 = _composed(x.astype(np.float32), y, ignore, lw, nw, w, n0)
        assert abs(loss32 - ref_loss) <= 1e-5 * max(abs(ref_loss), 1.0)
        assert np.max(np.abs(grad32 - ref_grad)) <= 1e-5 * max(np.max(np.abs(ref_grad)), 1e-30)


def test_nll_alone_keeps_ignored_rows_out_of_the_loss():
    """With the Lovasz half off, -inf log-probabilities in a row whose label is ignored do not reach the loss (a point with the ignore
    label is background of the other classes in the Lovasz half, so there the row is live)."""
    from lattice_net_amd.losses import SegmentationLoss
    n, c, ignore = 64, 5, 1
    x = H.logits_case(n, c, 9)
    y = H.labels_case(n, c, 9, ignore)
    gone = y == ignore
    assert gone.any() and not gone.all()
    bad = np.array(x)
    bad[gone, 0] = -np.inf
    m = SegmentationLoss(ignore, lovasz_weight=0.0, nll_weight=1.0)
    a, b = m(torch.from_numpy(x), torch.from_numpy(y)), m(torch.from_numpy(bad), torch.from_numpy(y))
    assert bool(torch.isfinite(b)) and torch.equal(a, b)  # (the -inf logit changes its own row's softmax only: that row is ignored)
    with pytest.raises(ValueError):
        m(torch.zeros(4), torch.zeros(4, dtype=torch.int64))
    assert float(SegmentationLoss(ignore, 0.0, 0.0)(torch.from_numpy(x), torch.from_numpy(y))) == 0.0


def test_segmentation_loss_on_f13(golden):
    """The reference's own LovaszSoftmax on F13 (tests/golden/make_losses_fixture.py).  The fixture holds no NLL value, so the NLL half
    is torch.nn.functional.nll_loss on the same log-probabilities.  The fixture's inputs are log-probabilities: as logits they are
    their own log-softmax up to rounding."""
    from lattice_net_amd.losses import SegmentationLoss
    f = golden("F13_losses")
    for name in [str(s) for s in f["case_names"]]:
        logp, labels, ignore = torch.from_numpy(f[f"{name}/logp"]).float(), torch.from_numpy(f[f"{name}/labels"]), int(f[f"{name}/ignore"])
        assert f"{name}/nll" not in f
        lov = float(f[f"{name}/lovasz_mean"])
        nll = float(torch.nn.functional.nll_loss(logp.double(), labels, ignore_index=ignore)) if bool((labels != ignore).any()) else 0.0
        loss = float(SegmentationLoss(ignore)(logp, labels))
        ref = 0.5 * lov + 0.5 * nll
        assert abs(loss - ref) <= 4e-6 * max(abs(ref), 1.0), (name, loss, ref)
        only = float(SegmentationLoss(ignore, lovasz_weight=1.0, nll_weight=0.0)(logp, labels))
        assert abs(only - lov) <= 4e-6 * max(abs(lov), 1.0), (name, only, lov)


def test_reference_layout_alias():
    from latticenet_py.lattice.lovasz_loss import SegmentationLoss, log_softmax
    from lattice_net_amd import losses
    assert SegmentationLoss is losses.SegmentationLoss and log_softmax is losses.log_softmax
