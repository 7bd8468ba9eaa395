"""fp64 references, per-element error bounds and fp32 emulations for the weight normalisation of csrc/ln_glue.hip
(k_weight_norm_forward / k_weight_norm_backward) and the fused mean NLL loss of one cloud, ln_nll_forward / ln_nll_backward of
csrc/ln_nll.hip (k_nll_clouds_wave / k_nll_clouds_partials / k_nll_clouds_finish / k_nll_clouds_backward on one cloud).
Plain NumPy on the CPU, in the vocabulary of dense_reference.py: test_glue_reference.py checks this module without a GPU,
test_gpu_weight_norm_nll.py holds the kernels to it.

A bound is (number of fp32 roundings on the kernel's path) * 2^-24 * (sum of the magnitudes the roundings act on); the counting
argument stands next to each count.  The library is compiled with -O3 -ffp-contract=off and without any fast-math flag
(lattice_net_amd/build_ext.py FLAGS), so `a * b + c` is two roundings and hipcc keeps its default of correctly rounded fp32 square
roots and divisions: sqrtf and `/` count one rounding each.  Counts are first-order (k * 2^-24, not k 2^-24 / (1 - k 2^-24)): the
largest k here is about 8200 (the 2^24-element parameter), where the second-order term is 5e-4 of the bound.

Both references take the fp32 inputs converted exactly to fp64."""
import json
import os

import numpy as np

from tests.dense_reference import EPS32, assert_within, f32, f64, worst_ratio

# csrc/ln_glue.hip
LN_WN_THREADS = 1024
LN_WN_MAX_G = 1024
LN_WN_MAX_ELEMENTS = 1 << 24
# csrc/ln_nll.hip (LN_NLLC_BLOCKS, LN_NLLC_THREADS, LN_NLLC_ROWS_PER_BLOCK / LN_NLLC_THREADS)
LN_NLL_BLOCKS = 512
LN_NLL_THREADS = 256
LN_NLL_PER_THREAD = 4  # blocks = ceil(n / (256 * 4)), at least 1, at most LN_NLL_BLOCKS
NO_LABEL = -(1 << 62)  # lattice_net_amd.losses._NO_LABEL: "no ignore_index"

# include/latticenet_hip.h
LN_OK, LN_ERR_ARG, LN_ERR_UNSUPPORTED = 0, -1, -2


def _ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------ weight norm
def wn_jk(rows, cols, g_dim):
    """(J, K): the number of magnitudes and the extent of the other dimension (LnWnShape)."""
    return (rows, cols) if g_dim == 0 else (cols, rows)


def wn_as_jk(a, g_dim):
    """a [rows, cols] seen as [J, K]."""
    return a if g_dim == 0 else a.T


def wn_lanes(J):
    return LN_WN_THREADS // J


def wn_k_values(J, cap=LN_WN_MAX_ELEMENTS):
    """The K at which the dot products of the backward change their path for this J: one or two elements per thread, one short of /
    exactly / one more than a full set of lanes, three rounds and one element."""
    lanes = wn_lanes(J)
    ks = sorted({1, 2, lanes - 1, lanes, lanes + 1, 3 * lanes + 1})
    return [k for k in ks if k >= 1 and J * k <= cap]


def wn_counts(rows, cols, g_dim):
    """Roundings on the path to each output, by the line of the kernel that makes them.

    k_weight_norm_forward:
      sum of squares: x * x (1), `acc +=` L = ceil(rows cols / 1024) times, the shuffle tree (6), the 16 wave totals from LDS (16).
      Every term is positive, so that is a relative error of the sum; sqrtf halves a relative error and rounds once:
          n_rel = (1 + L + 6 + 16) / 2 + 1                                  on n
      w[i] = v[i] * (g[j] / n): the division (1), the product (1), n:        w = n_rel + 2      on |w|
    k_weight_norm_backward (reads the forward's fp32 n; the reference uses the fp64 norm, so n_rel appears wherever n does):
      dot[j]: gw * v (1), `acc +=` ceil(K / lanes) times with lanes = 1024 / J, `d +=` lanes times over s_part:
          dot = 1 + ceil(K / lanes) + lanes                                  on A[j] = sum_k |gw v|
      gg[j] = d / n: the division (1), n:                                    grad_g = dot + 1 + n_rel    on A[j] / n
      t = block sum of d * g[j]: the product (1), the shuffle tree (6), 16 LDS adds:
          t = dot + 1 + 6 + 16                                               on T = sum_j |g[j]| A[j]
      dn_over_n = -t / (n * n * n): two products, one division, n three times:   dn = t + 3 + 3 n_rel   on T / n^3
      gv[i] = gw[i] * (g[j] / n) + v[i] * dn_over_n:
          first term : division, product, the add, n:                        gv_direct = 3 + n_rel       on |gw g / n|
          second term: product, the add:                                     gv_norm = dn + 2            on |v| T / n^3"""
    J, K = wn_jk(rows, cols, g_dim)
    L = _ceil_div(rows * cols, LN_WN_THREADS)
    n_rel = (1 + L + 6 + 16) / 2.0 + 1
    lanes = wn_lanes(J)
    dot = 1 + _ceil_div(K, lanes) + lanes
    t = dot + 1 + 6 + 16
    dn = t + 3 + 3 * n_rel
    return {"norm": n_rel, "w": n_rel + 2, "grad_g": dot + 1 + n_rel, "gv_direct": 3 + n_rel, "gv_norm": dn + 2}


def weight_norm_reference(v, g, g_dim, gw=None):
    """fp64  w = v g / n,  n = ||v||_F,  grad_g[j] = sum_k gw v / n,  grad_v = gw g / n - v (sum_j g[j] sum_k gw v) / n^3  for v, gw
    [rows, cols] and g [J].  Returns (w, norm, grad_v, grad_g) — the gradients None without gw — and the magnitudes their bounds
    multiply, each of its output's shape: {"w", "norm", "grad_g", "gv_direct", "gv_norm"} (wn_counts names the count of each)."""
    v, g = f64(v), f64(g).reshape(-1)
    rows, cols = v.shape
    J, K = wn_jk(rows, cols, g_dim)
    assert g_dim in (0, 1) and g.shape == (J,)
    gb = g[:, None] if g_dim == 0 else g[None, :]  # g[j] at every element
    with np.errstate(all="ignore"):
        n = np.sqrt(np.sum(v * v))
        w = v * (gb / n)
        mags = {"w": np.abs(w), "norm": np.abs(n)}
        if gw is None:
            return (w, n, None, None), mags
        gw = f64(gw)
        axis = 1 if g_dim == 0 else 0
        dot = np.sum(gw * v, axis=axis)
        A = np.sum(np.abs(gw * v), axis=axis)
        t = np.sum(g * dot)
        T = np.sum(np.abs(g) * A)
        grad_g = dot / n
        direct = gw * gb / n
        grad_v = direct - v * t / n ** 3
        mags.update({"grad_g": A / n, "gv_direct": np.abs(direct), "gv_norm": np.abs(v) * T / n ** 3})
    return (w, n, grad_v, grad_g), mags


def weight_norm_bounds(rows, cols, g_dim, mags):
    """{"w", "norm", "grad_v", "grad_g"}: count * 2^-24 * magnitude, the two terms of grad_v each with its own count."""
    c = wn_counts(rows, cols, g_dim)
    with np.errstate(all="ignore"):
        out = {"w": c["w"] * EPS32 * mags["w"], "norm": c["norm"] * EPS32 * mags["norm"]}
        if "grad_g" in mags:
            out["grad_g"] = c["grad_g"] * EPS32 * mags["grad_g"]
            out["grad_v"] = EPS32 * (c["gv_direct"] * mags["gv_direct"] + c["gv_norm"] * mags["gv_norm"])
    return out


def assert_weight_norm(got, v, g, g_dim, gw, what=""):
    """got = (w, norm, grad_v, grad_g) of one forward + backward: each within its bound of the fp64 reference, element by element, NaN
    and Inf exactly where fp64 has them.  Returns the worst error / bound ratio per output."""
    ref, mags = weight_norm_reference(v, g, g_dim, gw)
    bounds = weight_norm_bounds(v.shape[0], v.shape[1], g_dim, mags)
    ratios = {}
    for name, got_, ref_ in zip(("w", "norm", "grad_v", "grad_g"), got, ref):
        assert_within(np.asarray(f64(got_)).reshape(np.shape(ref_)), ref_, bounds[name], f"{what} {name}")
        ratios[name] = worst_ratio(np.asarray(f64(got_)).reshape(np.shape(ref_)), ref_, bounds[name])
    return ratios


def _wave_tree(x):
    """x [..., waves, 64] fp32: lane 0 of `for off = 32 .. 1: x += __shfl_down(x, off)`; only the lanes below `off` feed lane 0."""
    x = x.copy()
    off = 32
    while off:
        x[..., :off] = x[..., :off] + x[..., off:2 * off]
        off >>= 1
    return x[..., 0]


def _chain(terms):
    """terms [steps, ...] fp32: acc = 0; acc += terms[s] in order."""
    acc = np.zeros(terms.shape[1:], np.float32)
    for s in range(terms.shape[0]):
        acc = acc + terms[s]
    return acc


def _wn_block_sum(x):
    """ln_wn_block_sum over 1024 thread values: 16 wave trees, then t = 0; t += s_red[w]."""
    waves = _wave_tree(x.reshape(LN_WN_THREADS // 64, 64))
    return _chain(waves[:, None])[0]


def weight_norm_emulate(v, g, g_dim, gw=None):
    """The two kernels in fp32 NumPy: the same per-thread strides, shuffle tree and LDS order, every operator rounded to fp32.
    Returns (w, norm, grad_v, grad_g) in fp32."""
    v, g = f32(v), f32(g).reshape(-1)
    rows, cols = v.shape
    J, K = wn_jk(rows, cols, g_dim)
    total = rows * cols
    L = _ceil_div(total, LN_WN_THREADS)
    with np.errstate(all="ignore"):
        flat = np.zeros(L * LN_WN_THREADS, np.float32)
        flat[:total] = v.reshape(-1)
        n = np.sqrt(_wn_block_sum(_chain((flat * flat).reshape(L, LN_WN_THREADS))))
        gb = g[:, None] if g_dim == 0 else g[None, :]
        w = v * (gb / n)
        if gw is None:
            return w, n, None, None
        gw = f32(gw)
        lanes = wn_lanes(J)
        rounds = _ceil_div(K, lanes)
        prod = np.zeros((J, rounds * lanes), np.float32)
        prod[:, :K] = wn_as_jk(gw, g_dim) * wn_as_jk(v, g_dim)
        part = _chain(np.moveaxis(prod.reshape(J, rounds, lanes), 1, 0))  # [J, lanes]: thread (kl, j) walks k = kl, kl + lanes, ..
        d = _chain(np.moveaxis(part, 1, 0))
        grad_g = d / n
        mine = np.zeros(LN_WN_THREADS, np.float32)
        mine[:J] = d * g
        t = _wn_block_sum(mine)
        dn_over_n = -t / ((n * n) * n)
        grad_v = gw * (gb / n) + v * dn_over_n
    return w, n, grad_v, grad_g


def wn_random_case(rows, cols, g_dim, seed, scale=1.0):
    """v = scale * N(0, 1), g in [0.5, 1.5], gw[j, k] = 0.7 v[j, k] / (scale g[j]) + 1e-3 N(0, 1): without the noise gw g / n and
    v t / n^3 are both 0.7 v / (scale n), so the two terms of grad_v cancel to about 1e-3 of either and a bound on the sum of their
    magnitudes says something about the difference; g still differs from magnitude to magnitude (a wrong j shows)."""
    rng = np.random.default_rng(seed)
    J, _ = wn_jk(rows, cols, g_dim)
    v0 = rng.standard_normal((rows, cols)).astype(np.float32)
    g = rng.uniform(0.5, 1.5, J).astype(np.float32)
    gb = g[:, None] if g_dim == 0 else g[None, :]
    gw = (np.float32(0.7) * v0 / gb + np.float32(1e-3) * rng.standard_normal((rows, cols)).astype(np.float32)).astype(np.float32)
    return (v0 * np.float32(scale)).astype(np.float32), g, gw


def wn_exact_case(rows, cols, g_dim):
    """v in {0, +-1} with exactly 4^k non-zeros (the last element among them), so n = 2^k; g powers of two in [1/4, 4]; gw integers in
    [-3, 3].  Every partial sum is an integer or a multiple of 1/4 far below 2^24 and every output a dyadic rational; the case is
    returned only if every fp64 output is its own fp32 value (None otherwise: the caller drops it, nothing is loosened).
    Returns (v, g, gw, (w, norm, grad_v, grad_g)).
    What it exercises: indexing (which j, which element, the last element), the order-free parts of every sum and the final
    divisions, bit for bit.  What it does not: k is capped at 5, so v has at most 1024 non-zeros and, at large shapes (2^24 elements
    above all), almost every product of the dot fold is zero: the long accumulation chains there are checked by the random run and
    its counted bound only."""
    total = rows * cols
    J, _ = wn_jk(rows, cols, g_dim)
    k = 0
    while 4 ** (k + 1) <= total and k < 5:
        k += 1
    nz = 4 ** k
    idx = total - 1 - (np.arange(nz) * total) // nz
    flat = np.zeros(total, np.float32)
    flat[idx] = np.where((idx * 7 + idx // 5) % 3 == 0, -1.0, 1.0)
    v = flat.reshape(rows, cols)
    g = (2.0 ** ((np.arange(J) * 3) % 5 - 2)).astype(np.float32)
    i = np.arange(total)
    gw = (((i * 5 + i // 7) % 7) - 3).astype(np.float32).reshape(rows, cols)
    ref, _ = weight_norm_reference(v, g, g_dim, gw)
    assert ref[1] == 2.0 ** k
    for r in ref:
        if not np.array_equal(np.asarray(r).astype(np.float32).astype(np.float64), r):
            return None
    return v, g, gw, ref


# ------------------------------------------------------------------------------------------------------------------ NLL
def nll_blocks(n):
    return max(1, min(_ceil_div(n, LN_NLL_THREADS * LN_NLL_PER_THREAD), LN_NLL_BLOCKS))


def nll_count(n):
    """Roundings on the way to the loss: `acc +=` ceil(n / (blocks * 256)) times per thread of k_nll_clouds_partials, its shuffle tree (6)
    and (s0 + s1) + (s2 + s3) (3 adds, 2 on any path; counted 3); in k_nll_clouds_finish the shuffle tree (6) and the 8 wave totals (8); the
    division.  (Up to 1024 rows the finish, up to 64 the four waves too, are left out: they would add zeros, and the count stays an upper
    bound.)  The count of live labels is a sum of ones: exact in fp32 up to 2^24."""
    return _ceil_div(max(n, 1), nll_blocks(n) * LN_NLL_THREADS) + 6 + 3 + 6 + 8 + 1


def nll_labels(target, classes, ignore_index):
    """(live, clamped): labels equal to ignore_index are skipped (whatever their value, in range or not); the others are clamped to
    [0, classes - 1] — the semantics of the kernels of csrc/ln_nll.hip and of the gather formulation in losses.nll_loss_gather."""
    target = np.asarray(target, dtype=np.int64).reshape(-1)
    live = np.ones(target.shape, bool) if ignore_index is None else target != int(ignore_index)
    return live, np.clip(target, 0, classes - 1)


def nll_reference(lp, target, ignore_index=None, grad_loss=1.0):
    """fp64  loss = -sum_live lp[i, y_i] / max(count, 1),  count = max(#live, 1) as the kernel publishes it,
    grad_lp[i, y_i] = -grad_loss / count on the live rows and 0 elsewhere, and sum_live |lp[i, y_i]| (what the bound multiplies).
    Log-probabilities of rows that are ignored and of columns that are not the target are never read."""
    lp = f64(lp)
    n, classes = lp.shape
    live, tc = nll_labels(target, classes, ignore_index)
    count = max(int(live.sum()), 1)
    picked = lp[np.arange(n)[live], tc[live]]
    with np.errstate(all="ignore"):
        loss = -np.sum(picked) / count if picked.size else 0.0
        sum_abs = float(np.sum(np.abs(picked))) if picked.size else 0.0
    grad = np.zeros((n, classes))
    grad[np.arange(n)[live], tc[live]] = -float(grad_loss) / count
    return loss, float(count), grad, sum_abs


def nll_loss_bound(n, count, sum_abs):
    return nll_count(n) * EPS32 * sum_abs / count


def nll_emulate_cloud(val, wts):
    """The fixed-order sum of one cloud (k_nll_clouds_partials + phase 1 of k_nll_clouds_finish; the one-workgroup and the one-wave
    forms leave out steps that add +0) in fp32: val / wts [len] hold what a row adds to the two accumulators (0 where the label does
    not count: adding +0 to an accumulator that started at +0 changes no bit).  Returns (N, W) as fp32."""
    n = val.shape[0]
    blocks = nll_blocks(n)
    per_trip = blocks * LN_NLL_THREADS
    trips = max(_ceil_div(n, per_trip), 1)
    out = []
    for x in (val, wts):
        buf = np.zeros(trips * per_trip, np.float32)
        buf[:n] = x
        s = _wave_tree(_chain(buf.reshape(trips, blocks, LN_NLL_THREADS // 64, 64)))  # [blocks, 4]
        partial = np.zeros(LN_NLL_BLOCKS, np.float32)
        partial[:blocks] = (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])
        out.append(_chain(_wave_tree(partial.reshape(LN_NLL_BLOCKS // 64, 64))[:, None])[0])
    return out


def nll_emulate(lp, target, ignore_index=None):
    """ln_nll_forward in fp32 NumPy, the case of one cloud without weights of nll_clouds_reference.emulate: (loss, count)."""
    lp = f32(lp)
    n, classes = lp.shape
    live, tc = nll_labels(target, classes, ignore_index)
    with np.errstate(all="ignore"):
        val = np.where(live, lp[np.arange(n), tc], np.float32(0)).astype(np.float32)  # (a skipped row adds nothing: acc is never -0)
        a, c = nll_emulate_cloud(val, live.astype(np.float32))
        c = c if c != 0 else np.float32(1)
        return np.float32(-a / c), np.float32(c)


def assert_nll(loss_count, grad_lp, lp, target, ignore_index, grad_loss, what=""):
    """loss within its bound, loss_count[1] exactly max(count, 1); the gradient float32(-grad_loss / count) within one rounding at the
    clamped target of each live row, exactly +-0 everywhere else and free of NaN.  Returns the worst error / bound ratio of the loss."""
    n = np.shape(lp)[0]
    loss, count, grad, sum_abs = nll_reference(lp, target, ignore_index, grad_loss)
    got = f64(loss_count).reshape(2)
    bound = nll_loss_bound(n, count, sum_abs)
    assert got[1] == count, f"{what}: count {got[1]!r}, expected {count!r}"
    assert_within(got[0], np.float64(loss), bound, f"{what} loss")
    if grad_lp is not None:
        assert_within(grad_lp, grad, EPS32 * np.abs(grad), f"{what} grad_log_probs")
    return worst_ratio(got[0], np.float64(loss), bound)


def nll_random_case(n, classes, ignore_index, seed, out_of_range=True):
    """Log-softmax of N(0, 1) logits; labels uniform in [0, classes); a fifth of them ignore_index (when there is one); with
    out_of_range every eleventh of the rest -1, classes or classes + 7 in turn (skipped where that value is the ignore_index)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, classes))
    lp = (x - np.log(np.sum(np.exp(x), axis=1, keepdims=True))).astype(np.float32)
    target = rng.integers(0, classes, n).astype(np.int64)
    if out_of_range:
        for k, bad in enumerate((-1, classes, classes + 7)):
            if ignore_index is None or bad != int(ignore_index):
                target[k * 3 + 1::33] = bad
    if ignore_index is not None:
        target[rng.random(n) < 0.2] = int(ignore_index)
    return lp, target


def nll_exact_case(n, classes, ignore_index=-100):
    """Log-probabilities that are integers in [-8, -1]; the first 2^m rows live (2^m the largest power of two <= n) with labels that
    walk over the classes, the rest ignore_index; grad_loss = 3.  The sum is an integer below 2^24, loss and gradient are dyadic.
    Returns (lp, target, grad_loss, (loss, count, grad_lp, sum_abs)), or None if an output is not its own fp32 value."""
    assert n >= 1
    i = np.arange(n)
    lp = (-1.0 - ((i[:, None] * 3 + np.arange(classes)[None, :] * 5 + i[:, None] // 9) % 8)).astype(np.float32)
    livecount = 1 << (n.bit_length() - 1)
    target = ((i * 7 + i // 5) % classes).astype(np.int64)
    target[livecount:] = ignore_index
    ref = nll_reference(lp, target, ignore_index, 3.0)
    if ref[3] >= 2 ** 24 or ref[1] != livecount:
        return None
    for r in ref[:3]:
        if not np.array_equal(np.asarray(r).astype(np.float32).astype(np.float64), r):
            return None
    return lp, target, 3.0, ref


NLL_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nll_one_cloud_bits.json")


def nll_golden_cases():
    """What ln_nll_forward / ln_nll_backward wrote on an MI355X while they still had kernels of their own in ln_glue.hip, recorded bit for
    bit: n across every form boundary (wave, one workgroup, partials and finish) x classes x ignore_index, and per n a case with every
    label ignored (loss -0).  Yields (case, lp, target, grad_loss); case["loss_count"]: two uint32 words, case["grad_sha256"]: of the
    bytes of the float32 gradient [n, classes]."""
    with open(NLL_GOLDEN) as f:
        golden = json.load(f)
    for case in golden["cases"]:
        lp, target = nll_random_case(case["n"], case["classes"], case["ignore"], case["seed"])
        if case["all_ignored"]:
            target = np.full(case["n"], case["ignore"], np.int64)
        yield case, lp, target, golden["grad_loss"]


# the shapes test_gpu_weight_norm_nll.py runs (test_glue_reference.py runs the emulation at the same ones)
WN_J = (1, 2, 63, 64, 65, 511, 512, 513, 1000, 1023, 1024)
WN_ELEMENT_EDGE_SHAPES = ((3, 341), (341, 3), (32, 32), (25, 41), (41, 25))  # 1023, 1024 and 1025 elements
WN_LARGEST = (16384, 1024, 1)  # 2^24 elements, J = 1024, lanes = 1, L = 16384
NLL_N_SMALL = (1, 255, 256, 257, 1023, 1024, 1025)
NLL_N_LARGE = (524288, 524289, 1200003)  # 512 workgroups exactly; the cap with one element in a further trip; a ragged tail
NLL_CLASSES_SMALL = (1, 2, 5, 20, 33)


def wn_shapes():
    """Every (rows, cols, g_dim) of the J x K grid, both g_dim, and the element-count edges."""
    out = []
    for g_dim in (0, 1):
        for J in WN_J:
            for K in wn_k_values(J):
                out.append((J, K, 0) if g_dim == 0 else (K, J, 1))
        out += [(r, c, g_dim) for r, c in WN_ELEMENT_EDGE_SHAPES]
    return out


def nll_ignore_modes(classes):
    """none, in range, torch's default -100, and a value >= classes (classes + 7 is also one of the out-of-range labels)."""
    return (None, classes // 2, -100, classes + 7)
