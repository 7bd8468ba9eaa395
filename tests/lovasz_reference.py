"""fp64 reference, fp32 emulation and error bounds for the Lovasz-Softmax kernels (csrc/ln_lovasz.hip).  Plain NumPy on the CPU:
test_lovasz_reference.py checks this module without a GPU, test_gpu_lovasz.py holds the kernels to it.

Operator (include/latticenet_hip.h, ln_lovasz_forward).  Per class c: p = exp(lp[:, c]) (a p below the smallest normal float counts
as 0), fg_i = [clamp(y_i, 0, C-1) == c], e = |expm1(lp)| = |1 - p| for foreground and p for background; the errors in descending
order, EQUAL ERRORS BY ASCENDING POINT INDEX (`argsort(-e, kind="stable")`); with G = #fg and, after element k of that order,
U = G + #background and I = G - #foreground:
    g_k = 1 / U (k foreground),  I / (U (U - 1)) (k background)        [= J_k - J_{k-1}, J_k = 1 - I / U, g_0 = J_0]
    loss_c = sum_k e_(k) g_k,   d loss_c / d lp[i, c] = s_i g_rank(i) p_ic   (s = -1 foreground, +1 background)
A class counts when G > 0 and c != ignore_index; loss = sum of the counting loss_c, divided by max(#counting, 1) for "mean".

Bounds, in the vocabulary of dense_reference.py: (fp32 roundings on the kernel's path) * 2^-24 * (magnitude they act on).  The library
is compiled with -ffp-contract=off and without fast-math: `/` is the IEEE division, expf and expm1f are the device library's, whose
documented error (HIP math API) is 1 ulp = 2 * 2^-24 relative, counted as 2 roundings each.

  g_k         foreground: float(U) [1, exact below 2^24] and the division [1] = 2.  Background: float(I) [1], U (U - 1) formed in 64-bit
              integers and converted once [1], the division [1] = 3.  G, U, I are integers: exact whenever kernel and reference
              agree on the order.
  gradient    R_GRAD = 9:  expf [2] + g [3] + the product g p [1] + scale = 1 / #counting [1] + the product with it [1] = 8, and one
              unit for the second-order terms of (1 + 2^-24)^8.  Relative to |reference|: the gradient is a product, it has no sum.
              The error e does not enter it.
              R_GRAD_BACKWARD = 10: the product with grad_loss on top.
  loss_c      every term e g is >= 0, so a sum of depth D adds at most D * 2^-24 * (the sum).  A term carries expf or expm1f [2]
              (expm1f: the foreground error 1 - p is not formed by a subtraction that cancels when the prediction is right) + g [3]
              + the product [1] = 6.  Depth of the fixed-order sum (sum_depth): 8 items per thread in series, the 6-level shuffle
              tree of a wave, 3 adds over the waves of the workgroup; then over the tiles of the class (k_lovasz_finish):
              ceil(tiles / 256) in series per thread, 6 levels, 3 adds.   R_loss(n) = 6 + sum_depth(n) + 1 (second order).
              Near-ties need no term of their own: sum_k e_(k) g_k over the order of e IS the Lovasz extension of the Jaccard set
              function at e, a function of e alone that is monotone and positively homogeneous for e >= 0, so errors within
              (1 +- 2 * 2^-24) of the true ones give a value within the same factor whatever order their rounding produced.  (The
              gradient has no such property: it is compared only where kernel and reference must agree on the order.)
  loss        the counting classes in series [<= C adds of non-negative numbers] and the division by #counting [1]:
              R_loss(n) + C + 1, relative to the sum of the per-class references.
"""
import numpy as np

EPS32 = 2.0 ** -24
TINY32 = 2.0 ** -126
# csrc/ln_lovasz.hip
LN_LV_THREADS = 256
LN_LV_IPT = 8
LN_LV_TILE = LN_LV_THREADS * LN_LV_IPT
LN_LV_MAX_CLASSES = 1024

R_GRAD = 9
R_GRAD_BACKWARD = 10


def tiles(n):
    return (n + LN_LV_TILE - 1) // LN_LV_TILE


def sum_depth(n):
    return LN_LV_IPT + 6 + 3 + (tiles(n) + LN_LV_THREADS - 1) // LN_LV_THREADS + 6 + 3


def r_loss(n):
    return 6 + sum_depth(n) + 1


def r_total(n, c):
    return r_loss(n) + c + 1


def _counting(G, ignore_index):
    c = G.shape[0]
    counts = G > 0
    if ignore_index is not None and 0 <= int(ignore_index) < c:
        counts[int(ignore_index)] = False
    return counts


def reference(logp, target, ignore_index=None, reduction="mean"):
    """fp64: (loss, per_class [C] with 0 for the classes that do not count, d loss / d logp [N, C])."""
    lp = np.asarray(logp, dtype=np.float64)
    n, c = lp.shape
    y = np.clip(np.asarray(target, dtype=np.int64).reshape(-1), 0, c - 1)
    p = np.exp(lp)
    p[p < TINY32] = 0.0
    G = np.bincount(y, minlength=c)[:c]
    counts = _counting(G.copy(), ignore_index)
    scale = 1.0 / max(int(counts.sum()), 1) if reduction == "mean" else 1.0
    per_class = np.zeros(c)
    grad = np.zeros((n, c))
    for k in np.flatnonzero(counts):
        fg = y == k
        e = np.where(fg, np.abs(np.expm1(lp[:, k])), p[:, k])
        order = np.argsort(-e, kind="stable")
        fgs = fg[order]
        F = np.cumsum(fgs)
        U = G[k] + (np.arange(1, n + 1) - F)
        I = G[k] - F
        with np.errstate(divide="ignore", invalid="ignore"):
            g = np.where(fgs, 1.0 / U, I / (U.astype(np.float64) * (U - 1)))
        per_class[k] = np.sum(e[order] * g)
        grad[order, k] = np.where(fgs, -g, g) * p[order, k] * scale
    return per_class.sum() * scale, per_class, grad


def _tree64(x):
    """lane 0 of `for off in 32, 16, ..: x += shfl_down(x, off)` over the last axis (64 lanes)."""
    h = 32
    while h >= 1:
        x = x[..., :h] + x[..., h:2 * h]
        h //= 2
    return x[..., 0]


def _block_sum(x):
    """x [..., 256] float32 -> the workgroup's fixed-order sum: shuffle tree per wave, the four wave sums in series."""
    w = _tree64(x.reshape(x.shape[:-1] + (4, 64)))
    t = w[..., 0]
    for k in range(1, 4):
        t = t + w[..., k]
    return t


def _class_sum(terms):
    """The kernels' summation of one class's float32 terms (sorted order): k_lovasz_dot per tile, k_lovasz_finish over the tiles."""
    n = terms.shape[0]
    nblk = tiles(n)
    t = np.zeros(nblk * LN_LV_TILE, np.float32)
    t[:n] = terms
    t = t.reshape(nblk, 4, LN_LV_IPT, 64)  # position = (tile, wave, round, lane)
    acc = np.zeros((nblk, 4, 64), np.float32)
    for j in range(LN_LV_IPT):
        acc = acc + t[:, :, j, :]
    partial = _block_sum(acc.reshape(nblk, 256))
    m = (nblk + LN_LV_THREADS - 1) // LN_LV_THREADS
    pp = np.zeros(m * LN_LV_THREADS, np.float32)
    pp[:nblk] = partial
    pp = pp.reshape(m, LN_LV_THREADS)
    acc = np.zeros(LN_LV_THREADS, np.float32)
    for r in range(m):
        acc = acc + pp[r]
    return _block_sum(acc)


FAULTS = ("unstable_ties", "jaccard_difference", "ignore_counted", "absent_counted", "tile_last_dropped")


def emulate(logp, target, ignore_index=None, reduction="mean", fault=None):
    """The kernels' arithmetic in NumPy float32 (exp / expm1 are NumPy's float32 ones: within an ulp, like the device's).  `fault`
    plants one of FAULTS.  Returns (loss, per_class, d loss / d logp) as float32."""
    assert fault is None or fault in FAULTS, fault
    lp = np.asarray(logp, dtype=np.float32)
    n, c = lp.shape
    y = np.clip(np.asarray(target, dtype=np.int64).reshape(-1), 0, c - 1)
    one = np.float32(1)
    p = np.exp(lp)
    p[p < np.float32(TINY32)] = 0
    G = np.bincount(y, minlength=c)[:c]
    counts = _counting(G.copy(), None if fault == "ignore_counted" else ignore_index)
    if fault == "absent_counted":
        counts = counts | (G == 0)
        if ignore_index is not None and 0 <= int(ignore_index) < c:
            counts[int(ignore_index)] = False
    counting = max(int(counts.sum()), 1)
    scale = one / np.float32(counting) if reduction == "mean" else one
    per_class = np.zeros(c, np.float32)
    grad = np.zeros((n, c), np.float32)
    total = np.float32(0)
    pos = np.arange(n)
    for k in np.flatnonzero(counts):
        fg = y == k
        e = np.where(fg, np.abs(np.expm1(lp[:, k])), p[:, k]).astype(np.float32)
        key = np.uint32(0x7FFFFFFF) - (e.view(np.uint32) & np.uint32(0x7FFFFFFF))
        if fault == "unstable_ties":
            order = (n - 1 - np.argsort(key[::-1], kind="stable"))  # ties by descending point index
        else:
            order = np.argsort(key, kind="stable")
        fgs = fg[order]
        F = np.cumsum(fgs)
        U = int(G[k]) + (pos + 1 - F)
        I = int(G[k]) - F
        with np.errstate(divide="ignore", invalid="ignore"):
            if fault == "jaccard_difference":
                J = one - I.astype(np.float32) / U.astype(np.float32)
                g = np.concatenate((J[:1], J[1:] - J[:-1])).astype(np.float32)
            else:
                g = np.where(fgs, one / U.astype(np.float32), I.astype(np.float32) / (U * (U - 1)).astype(np.float32)).astype(np.float32)
            terms = e[order] * g
            coef = (np.where(fgs, -g, g) * p[order, k]) * scale
        if fault == "tile_last_dropped":
            last = (pos % LN_LV_TILE == LN_LV_TILE - 1) | (pos == n - 1)
            terms = np.where(last, np.float32(0), terms)
            coef = np.where(last, np.float32(0), coef)
        per_class[k] = _class_sum(terms.astype(np.float32))
        grad[order, k] = coef
        total = total + per_class[k]
    return (total / np.float32(counting) if reduction == "mean" else total), per_class, grad


# ---- bounds ------------------------------------------------------------------------------------------------------------------------
def per_class_bound(ref_per_class, n):
    return r_loss(n) * EPS32 * np.abs(ref_per_class)


def loss_bound(ref_per_class, n, reduction="mean", counting=1):
    s = float(np.sum(np.abs(ref_per_class)))
    return r_total(n, len(ref_per_class)) * EPS32 * (s / max(counting, 1) if reduction == "mean" else s)


def grad_bound(ref_grad, r=R_GRAD):
    return r * EPS32 * np.abs(ref_grad)


def counting_classes(target, c, ignore_index):
    y = np.clip(np.asarray(target, dtype=np.int64).reshape(-1), 0, c - 1)
    return int(_counting(np.bincount(y, minlength=c)[:c], ignore_index).sum())


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements with a non-zero bound; elements whose bound is 0 must be equal (inf otherwise)."""
    got, ref, bound = (np.asarray(a, dtype=np.float64) for a in (got, ref, np.broadcast_to(bound, np.shape(ref))))
    err = np.abs(got - ref)
    if not np.all(np.isfinite(got)):
        return np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(np.max(r)) if r.size else 0.0


def check(got, logp, target, ignore_index, reduction, what="", gradient=True, r_grad=R_GRAD, grad_scale=1.0):
    """got = (loss, per_class or None, grad or None) against the fp64 reference of the float32 inputs; every figure within its bound.
    Returns the worst error / bound ratios (loss, per_class, gradient)."""
    lp = np.asarray(logp, dtype=np.float32)
    n, c = lp.shape
    loss, per_class, grad = reference(lp, target, ignore_index, reduction)
    counting = counting_classes(target, c, ignore_index)
    ratios = [worst_ratio(got[0], loss, loss_bound(per_class, n, reduction, counting)), 0.0, 0.0]
    if got[1] is not None:
        ratios[1] = worst_ratio(got[1], per_class, per_class_bound(per_class, n))
    if gradient and got[2] is not None:
        ratios[2] = worst_ratio(got[2], grad * grad_scale, grad_bound(grad * grad_scale, r_grad))
    assert max(ratios) <= 1.0, f"{what}: error / bound = loss {ratios[0]:.3g}, per class {ratios[1]:.3g}, gradient {ratios[2]:.3g}"
    return tuple(ratios)


# ---- input families ----------------------------------------------------------------------------------------------------------------
def labels(n, c, seed, absent=None, all_one=None, out_of_range=False):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, c, n)
    if absent is not None and c > 1:
        y[y == absent] = (absent + 1) % c
    if all_one is not None:
        y[:] = all_one
    if out_of_range and n >= 2:
        y[0], y[-1] = -3, c + 5  # clamped to 0 and c - 1
    return y.astype(np.int64)


def separated(n, c, seed):
    """p[i, k] = (perm_k(i) + 0.25) / (n + 1): inside a class all errors, foreground (1 - p) and background (p) alike, differ by at
    least 0.5 / (n + 1) before the rounding of log p to float32."""
    rng = np.random.default_rng(seed)
    p = np.stack([(rng.permutation(n) + 0.25) / (n + 1) for _ in range(c)], 1)
    return np.log(p).astype(np.float32)


def separation(logp, target):
    """Smallest gap between two errors of one class, computed in fp64 from the float32 inputs."""
    lp = np.asarray(logp, dtype=np.float64)
    n, c = lp.shape
    y = np.clip(np.asarray(target, dtype=np.int64).reshape(-1), 0, c - 1)
    gap = np.inf
    for k in range(c):
        e = np.sort(np.where(y == k, np.abs(np.expm1(lp[:, k])), np.exp(lp[:, k])))
        if n > 1:
            gap = min(gap, float(np.min(np.diff(e))))
    return gap


def ties(n, c, seed, mode):
    """log-probabilities in {0, -200}: p in {1, 0} and e in {0, 1} exactly.  mode: 'right' (p = 1 exactly at the label), 'wrong'
    (p = 1 exactly off the label), 'mixed' (independent coin flips).  Returns (logp, labels)."""
    rng = np.random.default_rng(seed)
    y = labels(n, c, seed + 1)
    onehot = np.zeros((n, c), bool)
    onehot[np.arange(n), y] = True
    if mode == "right":
        hot = onehot
    elif mode == "wrong":
        hot = ~onehot
    else:
        hot = rng.random((n, c)) < 0.5
    return np.where(hot, 0.0, -200.0).astype(np.float32), y


def softmax_random(n, c, seed, spread=3.0):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, c)) * spread
    z = z - z.max(1, keepdims=True)
    return (z - np.log(np.exp(z).sum(1, keepdims=True))).astype(np.float32)
