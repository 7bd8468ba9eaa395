"""fp64 reference, fp32 emulation and error bounds for the PER-CLOUD Lovasz-Softmax loss (ln_lovasz_forward_clouds) and a NumPy
reference of the per-cloud intersection / union counts (ln_iou_counts_clouds).  Built on tests/lovasz_reference.py, which stays the
reference of one cloud: test_lovasz_clouds_reference.py checks this module on the CPU, test_gpu_lovasz_clouds.py and
test_gpu_iou_counts_clouds.py hold the kernels to it.

Operator (include/latticenet_hip.h).  The n rows are cloud-major: cloud b owns rows [b n0, min((b + 1) n0, n)), B = ceil(n / n0).
    per_cloud[b], per_class[b, :]   = lovasz_reference.reference on cloud b's rows alone
    loss                            = (sum_b per_cloud[b]) / B
    d loss / d logp on cloud b      = that cloud's gradient / B

Bounds, counted as in lovasz_reference.py ((fp32 roundings on the kernels' path) * 2^-24 * (the magnitude they act on)):
  gradient      the single-cloud coefficient [R_GRAD = 9: 8 roundings and the second-order unit] divided by float(B) (exact
                conversion, B <= 65535) in ONE IEEE division — no rounded reciprocal in between: R_GRAD + 1.  When B is a power of
                two the division is a change of exponent, exact (the coefficients are 0 or far above the subnormal range): R_GRAD,
                and the row is bitwise the single-cloud row times 1 / B.  Through ln_lovasz_backward: one more (R_GRAD_BACKWARD).
  per_cloud[b]  lovasz_reference.loss_bound of that cloud: the kernels run the same code on the cloud's segment.
  per_class     lovasz_reference.per_class_bound with the cloud's length.
  loss          every per_cloud[b] is >= 0.  k_lovasz_cloud_mean adds them strided over 256 threads — ceil(B / 256) additions in
                series per thread, the first onto 0 — then 6 levels of the wave's shuffle tree and 3 additions over the waves:
                cloud_sum_depth(B) = ceil(B / 256) + 6 + 3 roundings on a sum of non-negative numbers, one division by float(B)
                (exact conversion, B <= 65535) and one unit for the second-order terms:
                loss_bound = mean_b(bound of per_cloud[b]) + (cloud_sum_depth(B) + 2) * 2^-24 * mean_b(per_cloud[b]).
"""
import numpy as np

from . import lovasz_reference as R

THREADS = R.LN_LV_THREADS
MAX_CLOUDS = 65535  # include/latticenet_hip.h


def cloud_ranges(n, n0):
    """[(first row, end row)] of every cloud."""
    return [(lo, min(lo + n0, n)) for lo in range(0, n, n0)]


def is_power_of_two(b):
    return b >= 1 and (b & (b - 1)) == 0


def r_grad(clouds, through_backward=False):
    return (R.R_GRAD_BACKWARD if through_backward else R.R_GRAD) + (0 if is_power_of_two(clouds) else 1)


def cloud_sum_depth(clouds):
    return (clouds + THREADS - 1) // THREADS + 6 + 3


def reference(logp, target, n0, ignore_index=None, reduction="mean"):
    """fp64: (loss, per_cloud [B], per_class [B, C], d loss / d logp [n, C])."""
    lp = np.asarray(logp, dtype=np.float64)
    y = np.asarray(target, dtype=np.int64).reshape(-1)
    n, c = lp.shape
    ranges = cloud_ranges(n, n0)
    per_cloud = np.zeros(len(ranges))
    per_class = np.zeros((len(ranges), c))
    grad = np.zeros((n, c))
    for b, (lo, hi) in enumerate(ranges):
        per_cloud[b], per_class[b], g = R.reference(lp[lo:hi], y[lo:hi], ignore_index, reduction)
        grad[lo:hi] = g / len(ranges)
    return (per_cloud.sum() / len(ranges) if ranges else 0.0), per_cloud, per_class, grad


def cloud_mean32(per_cloud):
    """k_lovasz_cloud_mean in NumPy float32."""
    b = len(per_cloud)
    m = (b + THREADS - 1) // THREADS
    pp = np.zeros(m * THREADS, np.float32)
    pp[:b] = per_cloud
    acc = np.zeros(THREADS, np.float32)
    for row in pp.reshape(m, THREADS):
        acc = acc + row
    return R._block_sum(acc) / np.float32(b)


def emulate(logp, target, n0, ignore_index=None, reduction="mean"):
    """The kernels' arithmetic in NumPy float32: lovasz_reference.emulate per cloud, the coefficient divided by float(B), the mean."""
    lp = np.asarray(logp, dtype=np.float32)
    y = np.asarray(target, dtype=np.int64).reshape(-1)
    n, c = lp.shape
    ranges = cloud_ranges(n, n0)
    per_cloud = np.zeros(len(ranges), np.float32)
    per_class = np.zeros((len(ranges), c), np.float32)
    grad = np.zeros((n, c), np.float32)
    for b, (lo, hi) in enumerate(ranges):
        per_cloud[b], per_class[b], g = R.emulate(lp[lo:hi], y[lo:hi], ignore_index, reduction)
        grad[lo:hi] = g / np.float32(len(ranges))
    return cloud_mean32(per_cloud), per_cloud, per_class, grad


# ---- bounds ------------------------------------------------------------------------------------------------------------------------
def per_cloud_bounds(ref_per_class, target, n0, ignore_index, reduction):
    y = np.asarray(target, dtype=np.int64).reshape(-1)
    c = ref_per_class.shape[1]
    return np.array([R.loss_bound(ref_per_class[b], hi - lo, reduction, R.counting_classes(y[lo:hi], c, ignore_index))
                     for b, (lo, hi) in enumerate(cloud_ranges(len(y), n0))])


def per_class_bounds(ref_per_class, n, n0):
    return np.stack([R.per_class_bound(ref_per_class[b], hi - lo) for b, (lo, hi) in enumerate(cloud_ranges(n, n0))])


def loss_bound(ref_per_cloud, bounds_per_cloud):
    b = len(ref_per_cloud)
    return float(np.mean(bounds_per_cloud) + (cloud_sum_depth(b) + 2) * R.EPS32 * np.mean(np.abs(ref_per_cloud)))


def check(got, logp, target, n0, ignore_index, reduction, what="", gradient=True, through_backward=False, grad_scale=1.0, ref=None):
    """got = (loss, per_cloud or None, per_class or None, grad or None) against the fp64 reference (`ref`: reference(...) computed by
    the caller); every figure within its bound.  Returns the worst error / bound ratios (loss, per cloud, per class, gradient)."""
    lp = np.asarray(logp, dtype=np.float32)
    n = lp.shape[0]
    loss, per_cloud, per_class, grad = ref if ref is not None else reference(lp, target, n0, ignore_index, reduction)
    pcb = per_cloud_bounds(per_class, target, n0, ignore_index, reduction)
    ratios = [R.worst_ratio(got[0], loss, loss_bound(per_cloud, pcb)), 0.0, 0.0, 0.0]
    if got[1] is not None:
        ratios[1] = R.worst_ratio(got[1], per_cloud, pcb)
    if got[2] is not None:
        ratios[2] = R.worst_ratio(got[2], per_class, per_class_bounds(per_class, n, n0))
    if gradient and got[3] is not None:
        ratios[3] = R.worst_ratio(got[3], grad * grad_scale, R.grad_bound(grad * grad_scale, r_grad(len(per_cloud), through_backward)))
    assert max(ratios) <= 1.0, (f"{what}: error / bound = loss {ratios[0]:.3g}, per cloud {ratios[1]:.3g}, per class {ratios[2]:.3g}, "
                                f"gradient {ratios[3]:.3g}")
    return tuple(ratios)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def batch(n0, clouds, last, c, seed, family="separated"):
    """A cloud-major batch generated cloud by cloud with lovasz_reference's families: `clouds` clouds of n0 points, the last one of
    `last` points.  Meant for ignore_index = 0.  Cloud 0 carries labels outside [0, C), cloud 1 lacks class 1 (the others have it),
    cloud 2 is all class 0 (with ignore_index = 0: no class counts), cloud 3 all class C - 1.  family: "separated", "softmax", or
    "ties_right" / "ties_wrong" / "ties_mixed" — errors in {0, 1} exactly, so equal errors sit on both sides of every cloud boundary
    and a sort that reached across a boundary would order them otherwise.  Returns (logp [n, C] float32, labels [n] int64)."""
    lens = [n0] * (clouds - 1) + [last]
    lps, ys = [], []
    for b, m in enumerate(lens):
        if family.startswith("ties_"):
            lp, y = R.ties(m, c, seed + 31 * b, family[5:])
        else:
            lp = R.separated(m, c, seed + 31 * b) if family == "separated" else R.softmax_random(m, c, seed + 31 * b)
            y = R.labels(m, c, seed + 7 * b, absent=1 if b == 1 else None, all_one={2: 0, 3: c - 1}.get(b), out_of_range=b == 0)
        lps.append(lp)
        ys.append(y)
    return np.concatenate(lps), np.concatenate(ys)


# ---- intersection / union counts ---------------------------------------------------------------------------------------------------
def iou_counts(scores, target, n0, unlabeled_index):
    """(intersection [C], union [C]) int64: Scores.accumulate_scores' arithmetic cloud by cloud (np.argmax returns the first maximum)."""
    s = np.asarray(scores)
    y = np.asarray(target, dtype=np.int64).reshape(-1)
    n, c = s.shape
    inter, union = np.zeros(c, np.int64), np.zeros(c, np.int64)
    for lo, hi in cloud_ranges(n, n0):
        pred, gt = np.argmax(s[lo:hi], 1), y[lo:hi]
        hit = np.bincount(pred[pred == gt], minlength=c)[:c]
        n_gt = np.bincount(np.clip(gt, 0, c - 1), minlength=c)[:c]
        n_pred = np.bincount(pred, minlength=c)[:c]
        in_gt = n_gt > 0
        if unlabeled_index is not None and 0 <= int(unlabeled_index) < c:
            in_gt[int(unlabeled_index)] = False
        inter += hit * in_gt
        union += (n_gt + n_pred - hit) * in_gt
    return inter, union


def iou_inputs(n, c, seed):
    """Scores with tied maxima (rows of few distinct values, all-equal rows, the maximum repeated at a higher index) and labels of
    which some lie outside [0, C)."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 4, (n, c)).astype(np.float32)  # many exact ties
    s[::7] = 0.5                                         # all-equal rows: class 0 wins
    y = rng.integers(0, c, n)
    y[::11] = -2
    y[5::13] = c + 3
    return s, y.astype(np.int64)
