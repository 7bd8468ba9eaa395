"""CPU checks of the per-cloud Lovasz-Softmax loss and IoU counts: tests/lovasz_clouds_reference.py against lovasz_reference.py, the
torch forms of losses.LovaszSoftmax(points_per_cloud=) and Scores.accumulate_scores(points_per_cloud=) against it, and the difference
between the per-cloud and the whole-batch quantities that the feature exists for."""
import numpy as np
import pytest
import torch

from . import lovasz_clouds_reference as RC
from . import lovasz_reference as R

TILE = R.LN_LV_TILE
# (n0, clouds, points of the last cloud, classes)
SMALL = [(1, 1, 1, 2), (1, 5, 1, 3), (3, 7, 2, 20), (65, 3, 65, 3), (65, 4, 1, 20), (65, 2, 64, 2), (TILE + 1, 3, TILE, 3)]


def test_one_cloud_is_the_single_cloud_reference():
    for n, c in ((1, 2), (65, 3), (TILE + 1, 20)):
        lp, y = R.softmax_random(n, c, n), R.labels(n, c, n, out_of_range=True)
        for red in ("mean", "sum"):
            loss, pc, g = R.reference(lp, y, 0, red)
            for n0 in (n, n + 5):
                got = RC.reference(lp, y, n0, 0, red)
                assert got[0] == loss and got[1][0] == loss and np.array_equal(got[2][0], pc) and np.array_equal(got[3], g)
            e = RC.emulate(lp, y, n, 0, red)
            e1 = R.emulate(lp, y, 0, red)
            assert e[0].tobytes() == np.float32(e1[0]).tobytes() and np.array_equal(e[3], e1[2])


def test_permuting_whole_clouds_permutes_per_cloud_and_keeps_the_loss():
    n0, clouds, c = 65, 5, 3
    lp, y = RC.batch(n0, clouds, n0, c, 3, "softmax")
    loss, per_cloud, per_class, grad = RC.reference(lp, y, n0, 0)
    perm = np.array([3, 0, 4, 2, 1])
    rows = np.concatenate([np.arange(b * n0, (b + 1) * n0) for b in perm])
    loss2, per_cloud2, per_class2, grad2 = RC.reference(lp[rows], y[rows], n0, 0)
    assert np.array_equal(per_cloud2, per_cloud[perm]) and np.array_equal(per_class2, per_class[perm]) and np.array_equal(grad2, grad[rows])
    assert abs(loss2 - loss) <= RC.cloud_sum_depth(clouds) * 2.0 ** -53 * loss  # fp64 sum of the same non-negative terms in another order
    e, e2 = RC.emulate(lp, y, n0, 0), RC.emulate(lp[rows], y[rows], n0, 0)
    assert np.array_equal(e2[1], e[1][perm])
    assert abs(float(e2[0]) - float(e[0])) <= 2 * (RC.cloud_sum_depth(clouds) + 2) * R.EPS32 * loss


@pytest.mark.parametrize("shape", SMALL)
def test_emulated_kernels_stay_inside_every_bound(shape):
    n0, clouds, last, c = shape
    worst = np.zeros(4)
    for family, gradient in (("separated", True), ("ties_mixed", True), ("softmax", False)):
        lp, y = RC.batch(n0, clouds, last, c, 5, family)
        for red in ("mean", "sum"):
            worst = np.maximum(worst, RC.check(RC.emulate(lp, y, n0, 0, red), lp, y, n0, 0, red, f"{shape} {family} {red}", gradient=gradient))
    print(f"\n[lovasz clouds] {shape}: emulated kernels error/bound (loss, per cloud, per class, gradient) = "
          + ", ".join(f"{w:.3f}" for w in worst))


@pytest.mark.parametrize("shape", SMALL)
def test_torch_form_in_float64_is_the_reference(shape):
    from lattice_net_amd.losses import LovaszSoftmax
    n0, clouds, last, c = shape
    lp, y = RC.batch(n0, clouds, last, c, 9, "separated")
    for ignore, red in ((0, "mean"), (None, "sum"), (c + 3, "mean")):
        loss, _, _, grad = RC.reference(lp, y, n0, ignore, red)
        x = torch.from_numpy(lp).double().requires_grad_(True)
        out = LovaszSoftmax(ignore, red, points_per_cloud=n0)(x, torch.from_numpy(y))
        out.backward()
        assert abs(out.item() - loss) <= 1e-12, (shape, ignore, red, out.item(), loss)
        assert np.max(np.abs(x.grad.numpy() - grad)) <= 1e-12, (shape, ignore, red)
    with pytest.raises(ValueError):
        LovaszSoftmax(0, "none", points_per_cloud=n0)
    # points_per_cloud=None stays today's single-cloud function
    ref1 = R.reference(lp, y, 0, "mean")[0]
    assert abs(float(LovaszSoftmax(0)(torch.from_numpy(lp).double(), torch.from_numpy(y))) - ref1) <= 1e-12


def test_whole_batch_loss_is_another_function():
    """3 clouds x 65 points, C = 3, class 1 absent from cloud 1 only: the whole-batch loss differs from the per-cloud one by far more
    than any rounding, and it sends a gradient to [cloud 1, class 1] where the per-cloud gradient is exactly zero."""
    from lattice_net_amd.losses import LovaszSoftmax
    n0, clouds, c = 65, 3, 3
    lp = R.softmax_random(n0 * clouds, c, 1)
    y = np.concatenate([R.labels(n0, c, b, absent=1 if b == 1 else None) for b in range(clouds)])
    assert not (y[n0:2 * n0] == 1).any() and (y[:n0] == 1).any() and (y[2 * n0:] == 1).any()
    loss, per_cloud, per_class, grad = RC.reference(lp, y, n0, None)
    bound = RC.loss_bound(per_cloud, RC.per_cloud_bounds(per_class, y, n0, None, "mean"))
    xs = [torch.from_numpy(lp).double().requires_grad_(True) for _ in range(2)]
    whole = LovaszSoftmax(None)(xs[0], torch.from_numpy(y))
    clouds_loss = LovaszSoftmax(None, points_per_cloud=n0)(xs[1], torch.from_numpy(y))
    whole.backward()
    clouds_loss.backward()
    assert abs(clouds_loss.item() - loss) <= 1e-12
    assert abs(whole.item() - loss) > 100 * bound, (whole.item(), loss, bound)
    assert not grad[n0:2 * n0, 1].any() and not xs[1].grad[n0:2 * n0, 1].numpy().any()
    assert xs[0].grad[n0:2 * n0, 1].abs().max() > 0


def _scores_of(calls, unlabeled):
    from lattice_net_amd.losses import Scores
    s = Scores()
    for args, kw in calls:
        s.accumulate_scores(*args, unlabeled, **kw)
    return s


@pytest.mark.parametrize("shape", [(65, 3, 65, 3), (65, 4, 1, 20), (7, 5, 6, 2)])
def test_scores_per_cloud_equals_cloud_by_cloud(shape):
    n0, clouds, last, c = shape
    n = n0 * (clouds - 1) + last
    s, y = RC.iou_inputs(n, c, 4)
    # class 1 is missing from the ground truth of cloud 1 but predicted there
    second = y[n0:2 * n0]
    second[(second == 1) | (second >= c)] = 0  # (a label above C - 1 would be clamped to C - 1, which is class 1 when C = 2)
    s[n0, :] = 0.0
    s[n0, 1] = 9.0
    ts, ty = torch.from_numpy(s), torch.from_numpy(y)
    for unlabeled in (0, None, c + 2):
        one_by_one = _scores_of([((ts[lo:hi], ty[lo:hi]), {}) for lo, hi in RC.cloud_ranges(n, n0)], unlabeled)
        batched = _scores_of([((ts, ty), {"points_per_cloud": n0})], unlabeled)
        whole = _scores_of([((ts, ty), {})], unlabeled)
        ref_i, ref_u = RC.iou_counts(s, y, n0, unlabeled)
        for got in (one_by_one, batched):
            assert np.array_equal(got.intersection_per_class.numpy(), ref_i) and np.array_equal(got.union_per_class.numpy(), ref_u)
        assert batched.compute_stats() == one_by_one.compute_stats()
        assert not torch.equal(whole.union_per_class, batched.union_per_class)
        batched.accumulate_scores(ts, ty, unlabeled, points_per_cloud=n0)  # a second call adds
        assert np.array_equal(batched.union_per_class.numpy(), 2 * ref_u)
