"""fp64 reference, counted error bounds and an fp32 emulation for the per-cloud, class-weighted NLL loss of csrc/ln_nll.hip
(ln_nll_forward_clouds / ln_nll_backward_clouds).  Plain NumPy on the CPU, in the vocabulary of glue_reference.py, whose fp32 emulation of a
cloud's sum (nll_emulate_cloud) and partition (nll_blocks) it uses — ln_nll_forward is the one-cloud entry into the same kernels: test_nll_clouds_reference.py checks this module without a GPU,
test_gpu_nll_clouds.py holds the kernels to it.

Per cloud b (rows [b n0, min((b + 1) n0, n)), B = ceil(n / n0)), over the labels that count (y_i != ignore_index; labels outside
[0, C) clamped, carrying the weight of the class they clamp to; w = 1 without weights):
    N_b = sum w[y_i] lp[i, y_i],  W_b = sum w[y_i],  D_b = W_b if W_b != 0 else 1
    per_cloud[b] = -N_b / D_b,  weight_sum[b] = D_b,  loss = sum_b per_cloud[b] / B
    grad[i, y_i] = -grad_loss w[y_i] / (B D_b) on the counted rows, 0 elsewhere.

A bound is (fp32 roundings on the kernel's path) * 2^-24 * (sum of the magnitudes they act on), first order as in glue_reference.py
(the largest count here is about 30).  The counts, from the kernel:
    depth(len) = ceil(len / (blocks 256)) `acc +=` of one thread + 6 (shuffle tree) + 3 ((s0 + s1) + (s2 + s3), counted as
                 glue_reference.nll_count counts it) + 6 + 8 (the finish: the tree of a 512-lane layout and its 8 wave totals);
                 a short cloud that takes the wave or the one-block form adds zeros in the steps it leaves out — the count stays an
                 upper bound
    N_b: depth + 1 with weights (the product w lp), depth without          on A_b = sum |w lp|
    W_b: depth with weights                                                 on sum |w|;  without weights a sum of ones, exact to 2^24
    per_cloud: (e_N + |per_cloud| e_W) / (|D| - e_W), and the division (1) on |per_cloud| and on that error
    loss: the clouds' errors / B, and ceil(B / 1024) + 6 + 15 + 1 roundings (a thread's chain, the shuffle tree, the 16 wave totals,
          the division) on sum_b (|per_cloud[b]| + its error) / B
    grad: relative to itself: float(B) * weight_sum (1), the division (1), with weights the product grad_loss * w (1), plus
          e_W / (|D| - e_W); times (1 + 1e-3) for the second-order terms (asserted: the relative bound stays below 1e-3, so they are
          below 1e-3 of it), plus one fp32 denormal step.  Exactly +-0 wherever the reference is 0."""
import numpy as np

from tests.dense_reference import EPS32, assert_within, f32, f64, worst_ratio
from tests.glue_reference import (LN_ERR_ARG, LN_ERR_UNSUPPORTED, LN_NLL_BLOCKS, LN_NLL_THREADS, LN_OK, NO_LABEL, _ceil_div, _chain,  # noqa: F401
                                  _wave_tree, nll_blocks, nll_emulate_cloud, nll_labels)

# csrc/ln_nll.hip
LN_NLLC_WAVE_ROWS = 64        # clouds up to this many rows: a wave per cloud
LN_NLLC_ROWS_PER_BLOCK = 1024  # clouds up to this many rows: one workgroup, no partials
LN_NLLC_FINISH_THREADS = 1024
LN_NLLC_FUSED_CLOUDS = 64
MAX_CLOUDS = 65535
TINY32 = 2.0 ** -149
OUTPUTS = ("loss", "per_cloud", "weight_sum", "grad")


def cloud_ranges(n, n0):
    n0 = max(1, min(int(n0), max(n, 1)))
    return [(lo, min(lo + n0, n)) for lo in range(0, n, n0)]


def class_weights(frequencies, background_idx):
    """The formula of LNN.compute_class_weights in float32 NumPy: 1 / log(1.05 + f), the background class at 1e-8."""
    w = (np.float32(1.0) / np.log(np.float32(1.05) + np.asarray(frequencies, dtype=np.float32))).astype(np.float32)
    w[background_idx] = np.float32(1e-8)
    return w


def read_mask(target, classes, ignore_index):
    """[n, C] bool: the elements of log_probs the kernels may read — (counted row, clamped label)."""
    live, tc = nll_labels(target, classes, ignore_index)
    m = np.zeros((len(tc), classes), bool)
    m[np.arange(len(tc))[live], tc[live]] = True
    return m


def used_classes(target, classes, ignore_index):
    """[C] bool: the classes whose weight the kernels may read."""
    live, tc = nll_labels(target, classes, ignore_index)
    u = np.zeros(classes, bool)
    u[tc[live]] = True
    return u


def poisoned(lp, target, ignore_index, weight=None):
    """Copies of lp and weight with NaN and -inf (alternating) in every element the kernels must not read."""
    lp = np.array(lp, dtype=np.float32)
    n, c = lp.shape
    bad = np.where((np.arange(n)[:, None] + np.arange(c)[None, :]) % 2 == 0, np.float32("nan"), np.float32("-inf")).astype(np.float32)
    lp = np.where(read_mask(target, c, ignore_index), lp, bad).astype(np.float32)
    if weight is not None:
        weight = np.where(used_classes(target, c, ignore_index), weight, np.float32("nan")).astype(np.float32)
    return lp, weight


def reference(lp, target, n0, ignore_index=None, weight=None, grad_loss=1.0):
    """fp64 outputs and the magnitudes the bounds multiply.  Reads lp at the clamped label of the counted rows and weight at the classes
    of such labels, nothing else."""
    lp = f64(lp)
    n, classes = lp.shape
    live, tc = nll_labels(target, classes, ignore_index)
    ranges = cloud_ranges(n, n0)
    B = len(ranges)
    rows = np.arange(n)
    with np.errstate(all="ignore"):  # (what stands in the rows and classes that do not count is dropped by `where`, never multiplied)
        w = np.where(live, 1.0 if weight is None else f64(weight).reshape(-1)[tc], 0.0)
        terms = np.where(live, w * lp[rows, tc], 0.0)
    starts = [lo for lo, _ in ranges]

    def per_cloud_sum(x):
        return np.add.reduceat(x, starts) if B else np.zeros(0)

    out = {"num": per_cloud_sum(terms), "num_abs": per_cloud_sum(np.abs(terms)), "den": per_cloud_sum(w), "den_abs": per_cloud_sum(np.abs(w))}
    out["weight_sum"] = np.where(out["den"] != 0.0, out["den"], 1.0)
    out["per_cloud"] = -out["num"] / out["weight_sum"]
    cloud_of_row = rows // max(1, min(int(n0), max(n, 1)))
    grad = np.zeros((n, classes))
    grad[rows[live], tc[live]] = (-float(grad_loss) * w / (B * out["weight_sum"][cloud_of_row]))[live] if B else 0.0
    out["loss"] = float(np.sum(out["per_cloud"]) / B) if B else 0.0
    out["grad"] = grad
    out["clouds"] = B
    return out


def depth(length):
    """Roundings of one cloud's fixed-order sum (module docstring)."""
    return _ceil_div(max(length, 1), nll_blocks(length) * LN_NLL_THREADS) + 6 + 3 + 6 + 8


def loss_depth(B):
    return _ceil_div(max(B, 1), LN_NLLC_FINISH_THREADS) + 6 + 15 + 1


def bounds(ref, n, n0, weighted, grad_loss=1.0):
    ranges = cloud_ranges(n, n0)
    B = len(ranges)
    d = np.full(B, float(depth(ranges[0][1] - ranges[0][0])) if B else 0.0)
    if B:
        d[-1] = depth(ranges[-1][1] - ranges[-1][0])  # (only the last cloud may be shorter)
    e_n = (d + (1 if weighted else 0)) * EPS32 * ref["num_abs"]
    e_w = d * EPS32 * ref["den_abs"] if weighted else np.zeros(B)
    D, pc = np.abs(ref["weight_sum"]), np.abs(ref["per_cloud"])
    assert (e_w < 1e-3 * D).all()
    e_q = (e_n + pc * e_w) / (D - e_w)
    e_pc = e_q + EPS32 * (pc + e_q)
    rel = (2 + (1 if weighted else 0)) * EPS32 + e_w / (D - e_w)
    assert (rel < 1e-3).all()
    rel_rows = rel[np.arange(n) // max(1, min(int(n0), max(n, 1)))]
    g = np.abs(ref["grad"])
    return {"per_cloud": e_pc, "weight_sum": e_w,
            "loss": (np.sum(e_pc) + loss_depth(B) * EPS32 * np.sum(pc + e_pc)) / max(B, 1),
            "grad": np.where(g > 0, g * rel_rows[:, None] * (1 + 1e-3) + TINY32, 0.0)}


def check(got, lp, target, n0, ignore_index, weight, what="", grad_loss=1.0, ref=None):
    """Every output of `got` (a dict with the keys of OUTPUTS; "grad" may be missing) within its bound of the fp64 reference, element by
    element.  Returns the worst error / bound ratio per output."""
    n = np.shape(lp)[0]
    ref = reference(lp, target, n0, ignore_index, weight, grad_loss) if ref is None else ref
    bnd = bounds(ref, n, n0, weight is not None, grad_loss)
    ratios = {}
    for k in OUTPUTS:
        if k in got:
            g = np.asarray(f64(got[k])).reshape(np.shape(ref[k]))
            assert_within(g, np.asarray(ref[k], dtype=np.float64), bnd[k], f"{what} {k}")
            ratios[k] = worst_ratio(g, np.asarray(ref[k], dtype=np.float64), bnd[k])
    return ratios


# ------------------------------------------------------------------------------------------------------------------ fp32 emulation
def emulate(lp, target, n0, ignore_index=None, weight=None, grad_loss=1.0):
    """The kernels in fp32 NumPy: the same partition, strides, trees and finishing order, every operator rounded to fp32."""
    lp = f32(lp)
    n, classes = lp.shape
    live, tc = nll_labels(target, classes, ignore_index)
    ranges = cloud_ranges(n, n0)
    B = len(ranges)
    w32 = None if weight is None else f32(weight).reshape(-1)
    per_cloud, weight_sum = np.zeros(B, np.float32), np.zeros(B, np.float32)
    grad = np.zeros((n, classes), np.float32)
    g = np.float32(grad_loss)
    with np.errstate(all="ignore"):
        for b, (lo, hi) in enumerate(ranges):
            rows = np.arange(lo, hi)[live[lo:hi]]
            cls = tc[rows]
            w = np.ones(rows.size, np.float32) if w32 is None else w32[cls]
            val, wts = np.zeros(hi - lo, np.float32), np.zeros(hi - lo, np.float32)
            val[rows - lo] = lp[rows, cls] if w32 is None else w * lp[rows, cls]
            wts[rows - lo] = w
            N, W = nll_emulate_cloud(val, wts)
            D = W if W != 0 else np.float32(1)
            per_cloud[b], weight_sum[b] = -N / D, D
            d = np.float32(B) * D
            grad[rows, cls] = -g / d if w32 is None else (-g * w) / d
        T = LN_NLLC_FINISH_THREADS
        trips = max(_ceil_div(B, T), 1)
        buf = np.zeros(trips * T, np.float32)
        buf[:B] = per_cloud
        s = _wave_tree(_chain(buf.reshape(trips, T)).reshape(T // 64, 64))
        t = s[0]
        for k in range(1, T // 64):
            t = t + s[k]
        loss = np.float32(t / np.float32(B)) if B else np.float32(0)
    return {"loss": loss, "per_cloud": per_cloud, "weight_sum": weight_sum, "grad": grad}


# ------------------------------------------------------------------------------------------------------------------ cases
def labels_case(n, n0, classes, ignore_index, shares, seed, out_of_range=True):
    """Labels uniform in [0, C); in cloud b a share shares[b % len(shares)] of them ignore_index (1.0: every one); with out_of_range
    every eleventh of the rest -1, C or C + 7 in turn (skipped where that value is the ignore_index)."""
    rng = np.random.default_rng(seed)
    target = rng.integers(0, classes, n).astype(np.int64)
    if out_of_range:
        for k, bad in enumerate((-1, classes, classes + 7)):
            if ignore_index is None or bad != int(ignore_index):
                target[k * 3 + 1::33] = bad
    if ignore_index is not None:
        for b, (lo, hi) in enumerate(cloud_ranges(n, n0)):
            share = shares[b % len(shares)]
            target[lo:hi][rng.random(hi - lo) < share] = int(ignore_index)
    return target


def log_probs_case(n, classes, seed, cloud_scale=None, n0=None):
    """Log-softmax of N(0, 1) logits, fp32; with cloud_scale the logits of cloud b are multiplied by 1 + cloud_scale * b (the clouds'
    losses then differ)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, classes))
    if cloud_scale:
        for b, (lo, hi) in enumerate(cloud_ranges(n, n0)):
            x[lo:hi] *= 1.0 + cloud_scale * b
    return (x - np.log(np.sum(np.exp(x), axis=1, keepdims=True))).astype(np.float32)


def weights_case(kind, classes, seed, target=None, ignore_index=None):
    """None; "random": uniform in [0.1, 10]; "frequency": class_weights of the labels' own frequencies, class 0 the background."""
    if kind is None:
        return None
    if kind == "random":
        return np.random.default_rng(seed).uniform(0.1, 10.0, classes).astype(np.float32)
    assert kind == "frequency"
    live, tc = nll_labels(target, classes, ignore_index)
    freq = np.bincount(tc[live], minlength=classes) / max(int(live.sum()), 1)
    return class_weights(freq, 0)


def exact_case(n, n0, classes, weighted, ignore_index=-100):
    """Integer log-probabilities in [-8, -1], weights powers of two in [1/4, 4], every third label ignored, grad_loss = 3: every
    partial sum is a multiple of 1/4 far below 2^24, so the sums are exact whatever their order and the emulation's only roundings are
    the divisions, the mean and the gradient's products."""
    i = np.arange(n)
    lp = (-1.0 - ((i[:, None] * 3 + np.arange(classes)[None, :] * 5 + i[:, None] // 9) % 8)).astype(np.float32)
    target = ((i * 7 + i // 5) % classes).astype(np.int64)
    target[2::3] = ignore_index
    weight = (2.0 ** ((np.arange(classes) * 3) % 5 - 2)).astype(np.float32) if weighted else None
    return lp, target, weight, 3.0


def skewed_case():
    """The case the per-cloud mean exists for: four clouds of 257 points, C = 5, ignored shares 0 %, 50 %, 99 % and 90 %, the clouds'
    logits scaled by 1, 2, 3, 4 — the batch-wide mean is dominated by the first cloud.  (lp, target, n0, ignore_index)."""
    n0, c, ignore = 257, 5, 0
    n = 4 * n0
    lp = log_probs_case(n, c, 7, cloud_scale=1.0, n0=n0)
    target = np.random.default_rng(8).integers(1, c, n).astype(np.int64)
    target = np.where(labels_case(n, n0, c, -7, (0.0, 0.5, 0.99, 0.9), 9, out_of_range=False) == -7, ignore, target)
    return lp, target, n0, ignore


def batch_wide(lp, target, ignore_index=None, weight=None):
    """fp64: the loss of the whole batch as one cloud (what nll_loss_gather without points_per_cloud computes)."""
    return reference(lp, target, max(np.shape(lp)[0], 1), ignore_index, weight)["loss"]
