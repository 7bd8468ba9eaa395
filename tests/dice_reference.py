"""fp64 reference, fp32 emulation and error bounds for the generalized soft Dice loss of csrc/ln_dice.hip (ln_dice_forward /
ln_dice_backward), one cloud and per cloud.  test_dice_reference.py checks this module on the CPU, test_gpu_dice.py holds the kernels
to it.

Operator (include/latticenet_hip.h).  The n rows are cloud-major: cloud b owns rows [b n0, min((b + 1) n0, n)), B = ceil(n / n0).
Per cloud, with p = exp(logp), w_c = 0 for c == ignore_index, else 1:
    I_c = sum_i p_ic [y_i = c],  S_c = sum_i p_ic,  G_c = #{y_i = c},  D_c = S_c + G_c + 1e-6       (stats = I, S, G)
    per_cloud = sum_c w_c (1 - 2 I_c / D_c) / C,      loss = sum_b per_cloud[b] / B
    a_c = 2 w_c / (C D_c B),  b_c = a_c I_c / D_c     (coef),      d loss / d logp[i, c] = -p_ic (a_c [y_i = c] - b_c)
A label outside [0, C) belongs to no class (it counts in S only).

Bounds: (fp32 roundings on the kernels' path) * EPS32 * (the magnitude they act on), m roundings taken as gamma(m) = m EPS32 /
(1 - m EPS32) so that the products of (1 + delta) are covered, not only their first order.  Counted from the kernels' constants:
  K_EXP = 2     the kernels call OCML expf, documented to 1 ulp = 2 EPS32 of the result.  A result below the smallest normal float may
                come back as anything in [0, TINY32]: every sum carries (its number of terms) * TINY32 besides.
  I, S          all terms >= 0.  depth(len, C) additions lie on the longest path of the fixed order: `steps` in series in a lane
                (tile_rows / step_rows of tiling()), step_rows - 1 over the lanes of a class in LDS (C <= 256), `tiles` over the
                cloud's partials in the finishing workgroup.  |error| <= gamma(K_EXP + depth) * value.
  G             integer, exact; as a float exact up to 2^24 (one rounding beyond, counted in D).
  D             float(G), S + G, + 1e-6f and the constant's own rounding: R_D = 4 besides the error of S.
  class term    q = 2 I / D: the errors of I and D and R_Q = 1 division (2 I is exact); 1 - q: one more on |1 - q|.
  per_cloud     C - 1 additions in class order and the division by C: gamma(C) on the sum of the terms' magnitudes.
  loss          the clouds strided over 256 threads in series, 6 levels of the wave's shuffle tree, 3 additions over the waves, the
                division by B: gamma(ceil(B / 256) + 6 + 3 + 1) on the mean of the clouds' magnitudes.
  a             C D, 2 w / (C D), / B: R_A = 3 besides the error of D (float(C), float(B), 2 w are exact).
  b             a I, / D: R_B = 2 besides the errors of a, I and D — in all 2 (error of D) + (error of I) + 5.
  gradient      expf (K_EXP), a - b (1, on a + b), p t and grad_loss (p t) (R_GRAD_MUL = 2): every element within
                [K_EXP + 1 + 2 + the worse of the relative errors of a and b] * EPS32 * |grad_loss| p (a [y = c] + b),
                the sum of the magnitudes of its two terms; evaluated below term by term.
None of these constants is fitted to a measured error.
"""
import numpy as np

EPS32 = 2.0 ** -24
TINY32 = 2.0 ** -126
K_EXP = 2
# csrc/ln_dice.hip
LN_DICE_THREADS = 256
LN_DICE_STEPS = 16
LN_DICE_MAX_TILES = 512
MAX_CLASSES = 1024
MAX_CLOUDS = 65535
R_D, R_Q, R_A, R_B, R_GRAD_MUL = 4, 1, 3, 2, 2


def gamma(m):
    return m * EPS32 / (1.0 - m * EPS32)


def rel(*deltas):
    """Bound of |prod (1 + d_i) / prod (1 - d_j) - 1| for |d| <= deltas."""
    s = sum(deltas)
    return s / (1.0 - s)


def tiling(length, c):
    """ln_dice_tiling: (rows per step of a workgroup, rows per tile, tiles) of a cloud of `length` rows."""
    step_rows = LN_DICE_THREADS // c if c <= LN_DICE_THREADS else 1
    steps = LN_DICE_STEPS
    cap = step_rows * LN_DICE_MAX_TILES
    if length > cap * LN_DICE_STEPS:
        steps = (length + cap - 1) // cap
    tile_rows = step_rows * steps
    return step_rows, tile_rows, (length + tile_rows - 1) // tile_rows


def rows_past_the_tile_cap(c):
    """The first cloud length at which the tiles grow beyond LN_DICE_STEPS steps (LN_DICE_MAX_TILES tiles are no longer enough)."""
    return tiling(1, c)[0] * LN_DICE_STEPS * LN_DICE_MAX_TILES + 1


def depth(length, c):
    step_rows, tile_rows, tiles = tiling(length, c)
    return tile_rows // step_rows + (step_rows - 1) + tiles


def cloud_sum_depth(clouds):
    return (clouds + LN_DICE_THREADS - 1) // LN_DICE_THREADS + 6 + 3


def cloud_ranges(n, n0):
    n0 = max(1, min(n0, max(n, 1)))
    return [(lo, min(lo + n0, n)) for lo in range(0, n, n0)]


def _weights(c, ignore_index, dtype):
    w = np.ones(c, dtype)
    if ignore_index is not None and 0 <= int(ignore_index) < c:
        w[int(ignore_index)] = 0
    return w


def reference(logp, target, n0=None, ignore_index=None):
    """fp64: dict(loss, per_cloud [B], stats [B, 3, C], coef [B, 2, C], grad [n, C] = d loss / d logp); n0=None: one cloud."""
    lp = np.asarray(logp, dtype=np.float64)
    y = np.asarray(target, dtype=np.int64).reshape(-1)
    n, c = lp.shape
    ranges = cloud_ranges(n, n if n0 is None else n0)
    nb = len(ranges)
    w = _weights(c, ignore_index, np.float64)
    per_cloud, stats, coef, grad = np.zeros(nb), np.zeros((nb, 3, c)), np.zeros((nb, 2, c)), np.zeros((n, c))
    for b, (lo, hi) in enumerate(ranges):
        p = np.exp(lp[lo:hi])
        onehot = y[lo:hi, None] == np.arange(c)[None, :]
        inter, s, g = (p * onehot).sum(0), p.sum(0), onehot.sum(0).astype(np.float64)
        d = s + g + 1e-6
        stats[b] = inter, s, g
        per_cloud[b] = (w * (1.0 - 2.0 * inter / d)).sum() / c
        coef[b, 0] = 2.0 * w / (c * d) / nb
        coef[b, 1] = coef[b, 0] * inter / d
        grad[lo:hi] = -p * (coef[b, 0] * onehot - coef[b, 1])
    return dict(loss=per_cloud.sum() / nb if nb else 0.0, per_cloud=per_cloud, stats=stats, coef=coef, grad=grad)


def bounds(ref, logp, target, n0=None, ignore_index=None, grad_loss=1.0):
    """Error bounds of every output of the kernels around `ref` = reference(...) (the gradient: of grad_loss * ref["grad"])."""
    lp = np.asarray(logp, dtype=np.float64)
    y = np.asarray(target, dtype=np.int64).reshape(-1)
    n, c = lp.shape
    ranges = cloud_ranges(n, n if n0 is None else n0)
    nb = len(ranges)
    w = _weights(c, ignore_index, np.float64)
    e_stats, e_coef, e_pc, e_grad = np.zeros((nb, 3, c)), np.zeros((nb, 2, c)), np.zeros(nb), np.zeros((n, c))
    for b, (lo, hi) in enumerate(ranges):
        inter, s, g = ref["stats"][b]
        a, bb = ref["coef"][b]
        d = s + g + 1e-6
        gs = gamma(K_EXP + depth(hi - lo, c))
        e_i = gs * inter + g * TINY32
        e_s = gs * s + (hi - lo) * TINY32
        e_g = np.where(g > 2.0 ** 24, EPS32 * g, 0.0)
        e_stats[b] = e_i, e_s, e_g
        d_d = e_s / d + gamma(R_D)
        q = 2.0 * inter / d
        e_q = 2.0 * e_i / d / (1.0 - d_d - EPS32) + q * rel(d_d, R_Q * EPS32)
        e_t = w * (e_q + EPS32 * (np.abs(1.0 - q) + e_q))
        t = w * np.abs(1.0 - q)
        e_pc[b] = (e_t.sum() + gamma(c) * (t + e_t).sum()) / c
        d_a = rel(d_d, R_A * EPS32)
        d_b = rel(d_a, d_d, R_B * EPS32)
        e_a = a * d_a
        e_b = bb * d_b + a * e_i / d * (1.0 + d_b) + TINY32  # (a product that lands below the smallest normal float: TINY32 at most)
        e_coef[b] = e_a, e_b
        p = np.exp(lp[lo:hi])
        onehot = y[lo:hi, None] == np.arange(c)[None, :]
        mag = a * onehot + bb                                                     # sum of the magnitudes of the two terms
        e_term = np.where(onehot, (e_a + e_b) * (1.0 + EPS32) + EPS32 * (a + bb), e_b)  # of a - b, or of -b
        e_p = K_EXP * EPS32 * p + TINY32
        e_grad[lo:hi] = abs(grad_loss) * (p * e_term + e_p * (mag + e_term) + gamma(R_GRAD_MUL) * (p + e_p) * (mag + e_term)
                                              + 2 * TINY32)
    pc = np.abs(ref["per_cloud"])
    e_loss = (e_pc.mean() + gamma(cloud_sum_depth(nb) + 1) * (pc + e_pc).mean()) if nb else 0.0
    return dict(loss=e_loss, per_cloud=e_pc, stats=e_stats, coef=e_coef, grad=e_grad)


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements with a non-zero bound; elements whose bound is 0 must be equal (inf otherwise)."""
    got, ref, bound = (np.asarray(a, dtype=np.float64) for a in (got, ref, np.broadcast_to(bound, np.shape(ref))))
    if got.size == 0:
        return 0.0
    err = np.abs(got - ref)
    if np.isnan(err).any():
        return float("inf")
    zero = bound == 0
    if (err[zero] != 0).any():
        return float("inf")
    return float(np.max(err[~zero] / bound[~zero])) if (~zero).any() else 0.0


OUTPUTS = ("loss", "per_cloud", "stats", "coef", "grad")


def check(got, logp, target, n0, ignore_index, what="", grad_loss=1.0, ref=None):
    """got: dict with any of OUTPUTS (the gradient for `grad_loss`) against the fp64 reference; every figure within its bound.  Returns the
    worst error / bound ratio per output given."""
    ref = ref if ref is not None else reference(logp, target, n0, ignore_index)
    bnd = bounds(ref, logp, target, n0, ignore_index, grad_loss)
    ratios = {}
    for k in OUTPUTS:
        if got.get(k) is not None:
            ratios[k] = worst_ratio(got[k], ref[k] * (grad_loss if k == "grad" else 1.0), bnd[k])
    assert all(r <= 1.0 for r in ratios.values()), f"{what}: error / bound = " + ", ".join(f"{k} {r:.3g}" for k, r in ratios.items())
    return ratios


# ---- the kernels' arithmetic in NumPy float32 ------------------------------------------------------------------------------------------
def _block_sum(x):
    """x [256] float32 -> the workgroup's fixed-order sum: shuffle tree per wave (lane 0's path only), the four wave sums in series."""
    w = np.stack([_shuffle_down_sum(x[k * 64:(k + 1) * 64]) for k in range(4)])
    t = w[0]
    for k in range(1, 4):
        t = np.float32(t + w[k])
    return t


def _shuffle_down_sum(x):
    x = x.astype(np.float32).copy()
    for off in (32, 16, 8, 4, 2, 1):
        shifted = np.concatenate((x[off:], x[:off]))  # __shfl_down beyond lane 63 returns the lane's own value: irrelevant for lane 0
        x = x + shifted
    return x[0]


def emulate(logp, target, n0=None, ignore_index=None, grad_loss=1.0):
    """The three kernels in NumPy float32 (np.exp in place of expf), in their summation order."""
    f = np.float32
    lp = np.asarray(logp, dtype=f)
    y = np.asarray(target, dtype=np.int64).reshape(-1)
    n, c = lp.shape
    ranges = cloud_ranges(n, n if n0 is None else n0)
    nb = len(ranges)
    w = _weights(c, ignore_index, f)
    per_cloud, stats, coef, grad = np.zeros(nb, f), np.zeros((nb, 3, c), f), np.zeros((nb, 2, c), f), np.zeros((n, c), f)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for b, (lo, hi) in enumerate(ranges):
            step_rows, tile_rows, tiles = tiling(hi - lo, c)
            steps = tile_rows // step_rows
            p = np.zeros((tiles * tile_rows, c), f)
            p[:hi - lo] = np.exp(lp[lo:hi])
            onehot = np.zeros((tiles * tile_rows, c), bool)
            onehot[:hi - lo] = y[lo:hi, None] == np.arange(c)[None, :]
            p4 = p.reshape(tiles, steps, step_rows, c)
            m4 = onehot.reshape(tiles, steps, step_rows, c)
            acc_i, acc_s = np.zeros((tiles, step_rows, c), f), np.zeros((tiles, step_rows, c), f)
            for k in range(steps):  # a lane's walk
                acc_s = acc_s + p4[:, k]
                acc_i = acc_i + np.where(m4[:, k], p4[:, k], f(0))
            part_i, part_s = acc_i[:, 0], acc_s[:, 0]
            for r in range(1, step_rows):  # the lanes of a class
                part_i, part_s = part_i + acc_i[:, r], part_s + acc_s[:, r]
            inter, s = np.zeros(c, f), np.zeros(c, f)
            for k in range(tiles):  # the finishing workgroup
                inter, s = inter + part_i[k], s + part_s[k]
            g = onehot.sum(0).astype(f)
            d = (s + g) + f(1e-6)
            stats[b] = inter, s, g
            terms = w * (f(1) - (f(2) * inter) / d)
            total = terms[0]
            for k in range(1, c):
                total = f(total + terms[k])
            per_cloud[b] = total / f(c)
            a = ((f(2) * w) / (f(c) * d)) / f(nb)
            coef[b] = a, (a * inter) / d
            oh = onehot[:hi - lo]
            grad[lo:hi] = -f(grad_loss) * (p[:hi - lo] * np.where(oh, a - coef[b, 1], -coef[b, 1]))
    m = (nb + LN_DICE_THREADS - 1) // LN_DICE_THREADS
    pp = np.zeros(m * LN_DICE_THREADS, f)
    pp[:nb] = per_cloud
    acc = np.zeros(LN_DICE_THREADS, f)
    for row in pp.reshape(m, LN_DICE_THREADS):
        acc = acc + row
    loss = _block_sum(acc) / f(nb) if nb else f(0)
    return dict(loss=loss, per_cloud=per_cloud, stats=stats, coef=coef, grad=grad)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def log_softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    x = x - x.max(1, keepdims=True)
    return x - np.log(np.exp(x).sum(1, keepdims=True))


def inputs(n, c, seed, family="softmax"):
    """logp [n, C] float32.  "softmax": log-softmax of logits uniform in [-6, 6] (a dynamic range of e^+-6); "onehot": confident rows,
    one logit 30 above the others; "exact": entries 0 or -inf, one 0 per row (p is exactly 1 or 0)."""
    rng = np.random.default_rng(seed)
    if family == "softmax":
        return log_softmax64(rng.uniform(-6.0, 6.0, (n, c))).astype(np.float32)
    hot = rng.integers(0, c, n)
    if family == "onehot":
        x = rng.uniform(-1.0, 1.0, (n, c))
        x[np.arange(n), hot] += 30.0
        return log_softmax64(x).astype(np.float32)
    assert family == "exact"
    lp = np.full((n, c), -np.inf, np.float32)
    lp[np.arange(n), hot] = 0.0
    return lp


def labels(n, c, seed, kind="random"):
    """int64 [n].  "random"; "one": all points of class C - 1; "absent": class 0 and every odd class missing (C > 1); "wild": every
    fifth label outside [0, C) — negative or >= C."""
    rng = np.random.default_rng(seed + 977)
    y = rng.integers(0, c, n).astype(np.int64)
    if kind == "one":
        y[:] = c - 1
    elif kind == "absent" and c > 1:
        y = rng.choice(np.arange(2, c, 2) if c > 2 else np.array([1]), n).astype(np.int64)
    elif kind == "wild":
        y[::5] = np.where(rng.integers(0, 2, len(y[::5])) == 0, -1 - rng.integers(0, 3, len(y[::5])), c + rng.integers(0, 3, len(y[::5])))
    return y
