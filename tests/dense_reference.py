"""fp64 references and per-element error bounds for the dense network-layer kernels: GroupNorm (csrc/ln_norm.hip), the per-token
linear + LeakyReLU (csrc/ln_mlp.hip) and the max-centring (csrc/ln_centre.hip).  Plain NumPy on the CPU: test_dense_reference.py
checks this module without a GPU, test_gpu_dense_layers.py holds the kernels to it.

Vocabulary of test_gpu_segment_reduce.py.  A bound is (number of fp32 roundings on the kernel's path) * 2^-24 * (sum of the magnitudes
the roundings act on); the counting argument stands next to each bound.  The library is compiled with -ffp-contract=off, so `a * b + c`
is two roundings and an fmaf is one.  Every operator has two runs: `random` (each finite element within its bound of the fp64 result,
NaN / +-Inf exactly where fp64 has them) and `exact` (small integers, parameters that are small integers or powers of two: every
partial sum is exact in fp32, the result is the integer result bit for bit in any summation order)."""
import numpy as np

EPS32 = 2.0 ** -24

# csrc/ln_norm.hip
LN_GN_PASSES = 16
LN_GN_REPLICAS = 32
# csrc/ln_mlp.hip
LN_MLP_TILE = 64
LN_MLP_W_GRID = 512
# csrc/ln_centre.hip
LN_MC_ITERS = 4


def f64(a):
    """Anything array-like (a torch tensor on any device included) as a NumPy fp64 array."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def f32(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float32)


def _first(mask):
    return tuple(int(i) for i in np.argwhere(mask)[0])


def assert_within(got, ref, bound, what=""):
    """Element by element: the same NaN / +Inf / -Inf pattern as the fp64 reference, finite elements within `bound` (an array of ref's
    shape, or a scalar)."""
    got, ref = f64(got), f64(ref)
    bound = np.broadcast_to(f64(bound), ref.shape)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    for name, f in (("isnan", np.isnan), ("isposinf", np.isposinf), ("isneginf", np.isneginf)):
        bad = f(got) != f(ref)
        if bad.any():
            i = _first(bad)
            raise AssertionError(f"{what}: {name} differs in {int(bad.sum())} elements, first {i}: got {got[i]!r}, fp64 {ref[i]!r}")
    fin = np.isfinite(ref)
    with np.errstate(invalid="ignore"):
        err = np.where(fin, np.abs(got - ref), 0.0)
        bad = fin & ~(err <= bound)  # (a NaN bound fails)
    if bad.any():
        i = _first(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside the bound, first {i}: got {got[i]!r}, fp64 {ref[i]!r}, "
                             f"error {err[i]:.3e}, bound {bound[i]:.3e}")


def worst_ratio(got, ref, bound):
    """max error / bound over the finite elements with a non-zero bound (a figure to report, never asserted on)."""
    got, ref = f64(got), f64(ref)
    bound = np.broadcast_to(f64(bound), ref.shape)
    ok = np.isfinite(ref) & np.isfinite(got) & (bound > 0)
    return float(np.max(np.abs(got[ok] - ref[ok]) / bound[ok])) if ok.any() else 0.0


def assert_exact(got, ref, what=""):
    """Integer operands: the fp32 result is the integer result itself, bit for bit."""
    got, ref = f64(got), f64(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(np.all(ref == np.round(ref))) and (ref.size == 0 or float(np.abs(ref).max()) < 2 ** 24), f"{what}: the reference is not an exact fp32 integer"
    bad = got != ref
    if bad.any():
        i = _first(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} elements differ from the integer result, first {i}: got {got[i]!r}, exact {ref[i]!r}")


def assert_equal_bits(a, b, what=""):
    a, b = f32(a), f32(b)
    bad = a.view(np.uint32) != b.view(np.uint32)
    if bad.any():
        i = _first(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} elements differ bit for bit, first {i}: {a[i]!r} vs {b[i]!r}")


# ------------------------------------------------------------------------------------------------------------------ GroupNorm
def gn_rows_per_pass(c):
    return 256 // (c // 4)


def gn_chain(c):
    """fp32 roundings of k_gn_stats per term of a channel sum: the subtraction of the thread's pivot and the product (2), the chain of
    LN_GN_PASSES adds of one thread; from there on (the pivot put back, the fold of the workgroup, the atomics, the moments) everything
    is fp64 and adds a few 2^-53; the result is rounded to fp32 once (1).  The same for every width."""
    return 2 + LN_GN_PASSES + 1


def gn_pivot_rows(live, c):
    """For each of the first `live` rows the row whose value the kernel subtracts from it in fp32: a workgroup takes a slab of
    rows_per_pass * LN_GN_PASSES rows, thread rp of a channel quad the rows slab_start + k * rows_per_pass + rp, and the first of
    them (k = 0) is its pivot."""
    rpp = gn_rows_per_pass(c)
    i = np.arange(live)
    slab = rpp * LN_GN_PASSES
    return (i // slab) * slab + (i % slab) % rpp


def gn_params(c, affine, seed):
    """gamma in +-[0.5, 2] (every fifth channel negative), beta in [-1, 1]; (None, None) without affine parameters."""
    if not affine:
        return None, None
    rng = np.random.default_rng(seed)
    sign = np.where(np.arange(c) % 5 == 4, -1, 1)
    return (rng.uniform(0.5, 2.0, c) * sign).astype(np.float32), rng.uniform(-1.0, 1.0, c).astype(np.float32)


def gn_input(m, c, mean, std, seed):
    """mean + std * N(0, 1), fp32."""
    rng = np.random.default_rng(seed)
    return (mean + std * rng.standard_normal((m, c))).astype(np.float32)


def gn_conditioning_input(m, c, mean, std):
    """The seeded inputs of the conditioning requirement, the same for the kernels and for torch's fp32 GroupNorm on the CPU (whose own
    worst rstd error on them is 1e-6 .. 9e-6: Welford in fp32 at mean / std = 3000)."""
    return gn_input(m, c, mean, std, c)


def gn_outlier_input(m, c, row, shift, seed):
    """N(0, 1) with one row moved by `shift` standard deviations, alternating in sign over the channels (row 0 is the "invalid" vertex of
    a lattice, and any row may be a pivot of the kernel's shifted sums)."""
    x = gn_input(m, c, 0.0, 1.0, seed)
    x[row] += shift * np.where(np.arange(c) % 2, -1, 1)
    return x


def gn_statistics(x, groups, eps, rows=None):
    """fp64 group mean, rstd = 1 / sqrt(var + eps) and std over the first `rows` rows of x [M, C] (all rows when None; an empty set of
    rows has mean 0 and variance 0, as the kernel defines it)."""
    x = f64(x)
    m, c = x.shape
    rows = m if rows is None else max(0, min(int(rows), m))
    cg = c // groups
    if rows == 0:
        mean, var = np.zeros(groups), np.zeros(groups)
    else:
        xg = x[:rows].reshape(rows, groups, cg)
        mean = xg.mean(axis=(0, 2))
        var = ((xg - mean[None, :, None]) ** 2).mean(axis=(0, 2))  # two-pass: no cancellation
    return mean, 1.0 / np.sqrt(var + eps), np.sqrt(var)


# the conditioning requirement (README: fp32 features within 1e-5 relative): every rstd within 1e-5 relative, every mean within
# 1e-6 * (|mean| + std) — what torch's fp32 native_group_norm meets on the same inputs (test_dense_reference.py)
GN_RSTD_RTOL = 1e-5
GN_MEAN_RTOL = 1e-6


def assert_gn_statistics(mean_rstd, x, groups, eps, rows=None, what=""):
    mean, rstd, std = gn_statistics(x, groups, eps, rows)
    got = f64(mean_rstd).reshape(2, groups)
    assert_within(got[0], mean, GN_MEAN_RTOL * (np.abs(mean) + std), f"{what} mean")
    assert_within(got[1], rstd, GN_RSTD_RTOL * rstd, f"{what} rstd")
    return worst_ratio(got[1], rstd, GN_RSTD_RTOL * rstd)


def assert_gn_scale_shift(scale_shift, mean_rstd, gamma, beta, c, groups, what=""):
    """a[c] = gamma * rstd (one rounding of the fp32 product: within one ulp of the product of the published fp32 rstd);
    b[c] = beta - mean * a, formed in fp64 from the fp64 mean and rounded once; the published mean is that mean rounded to fp32, so
    against the published mean: 2^-24 |mean a| for the mean's rounding + 2^-24 (|beta| + |mean a|) for the result's."""
    cg = c // groups
    mr = f64(mean_rstd).reshape(2, groups)
    mean, rstd = np.repeat(mr[0], cg), np.repeat(mr[1], cg)
    gamma = np.ones(c) if gamma is None else f64(gamma)
    beta = np.zeros(c) if beta is None else f64(beta)
    ss = f64(scale_shift).reshape(2, c)
    assert_within(ss[0], gamma * rstd, EPS32 * np.abs(gamma * rstd), f"{what} scale")
    assert_within(ss[1], beta - mean * ss[0], EPS32 * (np.abs(beta) + 2 * np.abs(mean * ss[0])), f"{what} shift")


def gn_apply_fp32(x, scale_shift, relu, rows=None):
    """y the way k_gn_apply evaluates it: fl(fl(x * a) + b) in fp32 (no contraction), max(., 0) with ReLU, zeros beyond `rows`."""
    x = f32(x)
    m, c = x.shape
    ss = f32(scale_shift).reshape(2, c)
    with np.errstate(all="ignore"):
        y = (x * ss[0][None, :]).astype(np.float32) + ss[1][None, :]
    if relu:
        y = np.where(y > 0, y, np.float32(0.0)).astype(np.float32)  # fmaxf(NaN, 0) = 0
    if rows is not None:
        y[max(0, min(int(rows), m)):] = 0.0
    return y


def assert_gn_apply(y, x, scale_shift, relu, rows=None, what=""):
    """Given the kernel's own scale / shift: y = x a + b within 2 roundings (product, sum; one spare: 3 * 2^-24 (|x a| + |b|)) of the fp64
    value, the zero pattern of the ReLU exactly {fl(fl(x a) + b) <= 0}, and exact zeros in the rows beyond `rows`."""
    x64 = f64(x)
    m, c = x64.shape
    live = m if rows is None else max(0, min(int(rows), m))
    ss = f64(scale_shift).reshape(2, c)
    y = f64(y)
    y32 = gn_apply_fp32(x, scale_shift, relu, rows)
    if live < m:
        bad = y[live:] != 0
        if bad.any():
            i = _first(bad)
            raise AssertionError(f"{what}: y is not zero in {int(bad.sum())} elements beyond row {live}, first {(i[0] + live, i[1])}: {y[live:][i]!r}")
    with np.errstate(all="ignore"):
        ref = x64[:live] * ss[0] + ss[1]
        bound = 3 * EPS32 * (np.abs(x64[:live] * ss[0]) + np.abs(ss[1]))
    if relu:
        zero_got, zero_want = y[:live] == 0, y32[:live] == 0
        bad = zero_got != zero_want
        if bad.any():
            i = _first(bad)
            raise AssertionError(f"{what}: the zero pattern of the ReLU differs in {int(bad.sum())} elements, first {i}: y {y[:live][i]!r}, "
                                 f"x a + b in fp32 {y32[:live][i]!r}")
        ref = np.where(zero_want, 0.0, ref)
    assert_within(y[:live], ref, np.broadcast_to(bound, ref.shape), f"{what} y")
    return worst_ratio(y[:live], ref, np.broadcast_to(bound, ref.shape))


def gn_backward_reference(x, gy, mask, gamma, mean_rstd, groups, rows=None):
    """The backward of GroupNorm in fp64 with the statistics (mean, rstd per group: `mean_rstd`, taken as exact numbers) and the ReLU
    mask given — the places an error of the forward can come from are checked on their own:
        g' = gy * mask,  ds[c] = sum_i g' (x - mean),  db[c] = sum_i g'
        dgamma = ds * rstd,  dbeta = db
        c2[g] = -sum_{c in g} gamma ds * rstd^3 / cnt,   c3[g] = -c2 mean - sum_{c in g} gamma db * rstd / cnt
        dx = g' gamma rstd + x c2 + c3     ( = g' gamma rstd + (x - mean) c2 - sum gamma db rstd / cnt )
    Returns the three gradients and their bounds.  Roundings, with K = gn_chain(c) for a channel sum and p the pivot the kernel subtracts
    from a row in fp32 (gn_pivot_rows; per thread S = sum g' (x - p) and Q = sum g', then sum g' x = S + p Q in fp64, so that
    ds - db mean = sum over threads of S + (p - mean) Q):
        dbeta : K * 2^-24 * sum |g'|
        dgamma: K * 2^-24 * rstd * sum |g'| (|x - p| + |mean - p|)
        dx    : fp32 apply, no contraction: fl(gamma rstd), two products, c2 and c3 rounded to fp32, two adds: at most 4 roundings on
                any term: 4 * 2^-24 * (|g' gamma rstd| + |x c2| + |c3|); + the error of the sums inside c2, c3 (c3 is formed in fp64
                from the same c2, so that error reaches dx as d(c2) |x - mean|): K * 2^-24 * (sum_{c in g} |gamma| A[c] rstd^3 |x - mean|
                + sum_{c in g} |gamma| B[c] rstd) / cnt  with A = sum |g'| (|x - p| + |mean - p|), B = sum |g'|.
    Rows beyond `rows` get dx = 0 and count nowhere."""
    x, gy = f64(x), f64(gy)
    m, c = x.shape
    live = m if rows is None else max(0, min(int(rows), m))
    cg = c // groups
    mr = f64(mean_rstd).reshape(2, groups)
    mean, rstd = np.repeat(mr[0], cg), np.repeat(mr[1], cg)
    gamma = np.ones(c) if gamma is None else f64(gamma)
    xs = x[:live]
    g = gy[:live] * (1.0 if mask is None else f64(mask)[:live])
    piv = xs[gn_pivot_rows(live, c)]
    K = gn_chain(c) * EPS32
    cnt = max(live, 1) * cg
    with np.errstate(all="ignore"):
        ds = (g * (xs - mean)).sum(0)
        db = g.sum(0)
        A = (np.abs(g) * (np.abs(xs - piv) + np.abs(mean - piv))).sum(0)
        B = np.abs(g).sum(0)
        dgamma, dbeta = ds * rstd, db
        b_dgamma, b_dbeta = K * rstd * A, K * B

        def group(v):
            return np.repeat(v.reshape(groups, cg).sum(1), cg)

        c2 = -group(gamma * ds) * rstd ** 3 / cnt
        c3 = -c2 * mean - group(gamma * db) * rstd / cnt
        dx = np.zeros_like(x)
        b_dx = np.zeros_like(x)
        dx[:live] = g * gamma * rstd + xs * c2 + c3
        b_dx[:live] = 4 * EPS32 * (np.abs(g * gamma * rstd) + np.abs(xs * c2) + np.abs(c3)) \
            + K * (group(np.abs(gamma) * A) * rstd ** 3 * np.abs(xs - mean) + group(np.abs(gamma) * B) * rstd) / cnt
    return (dx, dgamma, dbeta), (b_dx, b_dgamma, b_dbeta)


def gn_exact_input(m, c, groups):
    """Integer rows for the exact run: x = mean[g] + 2 s with mean[g] = g % 5 - 2 and s = +1 on even rows, -1 on odd rows (so that a row
    left out or counted twice moves the mean off its integer); the last row of an odd number of rows alternates over its channels
    instead.  With an even number of elements per group the group mean is that integer and the variance exactly 4: rstd = 1/2 with
    eps = 0.  Every difference of two rows is 0 or +-4, every partial sum an integer far below 2^24."""
    i, ch = np.arange(m)[:, None], np.arange(c)[None, :]
    s = 1 - 2 * np.where((m % 2 == 1) & (i == m - 1), ch % 2, i % 2)
    return ((ch // (c // groups)) % 5 - 2 + 2 * s).astype(np.float32)


def gn_exact_grad(m, c):
    """Even integers in [-8, 8] that differ from row to row and channel to channel."""
    i, ch = np.arange(m)[:, None], np.arange(c)[None, :]
    return (2 * ((i * 7 + ch * 3 + (i // 9)) % 9 - 4)).astype(np.float32)


def gn_exact_params(c):
    """gamma in {2, 4, -2}, beta small integers: with rstd = 1/2 scale and shift are integers."""
    ch = np.arange(c)
    return np.array([2.0, 4.0, -2.0], np.float32)[ch % 3], ((ch % 7) - 3).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ linear + LeakyReLU
# (rows, cin, cout, slope, bias, x needs grad): the branch of csrc/ln_mlp.hip each one is here for
MLP_CASES = {
    "4to16-w_groups_G4-rows_48000": (48000, 4, 16, 0.2, True, False),
    "16to32-w_256_to_1024_pairs": (48000, 16, 32, 0.2, True, True),
    "1to1-w_groups_G256-scalar_forward": (4097, 1, 1, 0.2, True, True),
    "3to5-scalar_forward-scalar_backward_x-G17": (1000, 3, 5, 0.2, True, True),
    "16to15-vector_backward_x_scalar_inner_loop": (3000, 16, 15, 0.2, True, True),
    "9to1-no_activation": (48000, 9, 1, -1.0, True, True),
    "32to64-w_tiled": (3333, 32, 64, 0.2, True, True),
    "127to80-w_untiled_40_pairs_per_thread": (700, 127, 80, 0.2, True, True),
    "80to128-w_tiled_10240_pairs": (700, 80, 128, 0.0, True, True),
    "96to96-bias-streaming": (2000, 96, 96, -1.0, True, True),
    "16to32-rows_1": (1, 16, 32, 0.2, True, True),
    "16to32-rows_63": (63, 16, 32, 0.0, True, True),
    "16to32-rows_64": (64, 16, 32, 0.2, False, True),
    "16to32-rows_65-last_tile_of_1": (65, 16, 32, 0.2, True, True),
    "4to16-rows_64x512-1-last_tile_of_63": (64 * 512 - 1, 4, 16, 0.2, True, True),
    "4to16-rows_64x512+1-w_grid_cap-two_tiles_per_workgroup": (64 * 512 + 1, 4, 16, 0.0, True, True),
    "32to64-rows_64x512+1-w_tiled_grid_cap": (64 * 512 + 1, 32, 64, 0.2, False, False),
    "4to64-forward_grid_stride": (70000, 4, 64, 0.2, True, True),
    "5to8-no_bias-slope_0": (1000, 5, 8, 0.0, False, True),
}


def mlp_forward_reference(x, w, b, slope, y_got):
    """fp64 y = act(x w^T + b) and its bound (cin + 1) * 2^-24 * (sum |x w| + |b|): a chain of cin fmafs starting from the bias, one
    product with the slope.  The branch of the activation is the one the kernel took (y_got > 0), so that an element whose pre-activation
    rounds across zero is compared with the same branch; where the fp64 pre-activation is further from zero than the bound the two
    signs must agree (asserted here: a kernel that takes the wrong branch does not hide behind its own mask)."""
    x, w = f64(x), f64(w)
    pre = x @ w.T
    mag = np.abs(x) @ np.abs(w).T
    if b is not None:
        pre = pre + f64(b)[None, :]
        mag = mag + np.abs(f64(b))[None, :]
    bound = (x.shape[1] + 1) * EPS32 * mag
    if slope < 0:
        return pre, bound, None
    mask = f64(y_got) > 0
    with np.errstate(invalid="ignore"):
        clear = np.isfinite(pre) & (np.abs(pre) > bound)
        bad = clear & (mask != (pre > 0))
    if bad.any():
        i = _first(bad)
        raise AssertionError(f"linear forward: the activation took the wrong branch in {int(bad.sum())} elements, first {i}: y {f64(y_got)[i]!r}, "
                             f"fp64 pre-activation {pre[i]!r}")
    return np.where(mask, pre, pre * slope), bound, mask


def mlp_w_chain(rows, cin, cout):
    """Roundings on the way to one element of grad_w / grad_b: a workgroup walks ceil(tiles / grid) tiles of LN_MLP_TILE rows in one fmaf
    chain (with fewer than 256 (o, i) pairs the rows of a tile are split over G = 256 // pairs thread groups, folded by G adds), writes
    a slab; ln_k_sum_slabs adds ceil(grid / 16) slabs per thread and folds 16 threads."""
    tiles = -(-rows // LN_MLP_TILE)
    grid = max(1, min(tiles, LN_MLP_W_GRID))
    pairs = cin * cout
    G = 256 // pairs if pairs < 256 else 1
    return LN_MLP_TILE * -(-tiles // grid) + G + -(-grid // 16) + 16


def mlp_backward_reference(x, w, gy, mask, slope):
    """fp64 gradients with g' = gy * (mask ? 1 : slope) (mask: the kernel's own y > 0; None: no activation), and their bounds:
        grad_x[t, i] = sum_o g' w     : (cout + 1) * 2^-24 * sum_o |g' w|   (the product with the slope, a chain of cout fmafs)
        grad_w[o, i] = sum_t g' x     : (mlp_w_chain + 1) * 2^-24 * sum_t |g' x|
        grad_b[o]    = sum_t g'       : (mlp_w_chain + 1) * 2^-24 * sum_t |g'|"""
    x, w, gy = f64(x), f64(w), f64(gy)
    rows, cin = x.shape
    cout = w.shape[0]
    g = gy if mask is None else gy * np.where(mask, 1.0, slope)
    K = (mlp_w_chain(rows, cin, cout) + 1) * EPS32
    gx, b_gx = g @ w, (cout + 1) * EPS32 * (np.abs(g) @ np.abs(w))
    gw, b_gw = g.T @ x, K * (np.abs(g).T @ np.abs(x))
    gb, b_gb = g.sum(0), K * np.abs(g).sum(0)
    return (gx, gw, gb), (b_gx, b_gw, b_gb)


def mlp_exact_case(rows, cin, cout, slope):
    """Integer x, gy in [-3, 3], weights in {-2, -1, 0, 1, 2}, integer bias; slopes 0, -1 (none) or 0.5 (with even gy: g' stays an
    integer).  Every sum over rows stays below 2^24 for rows <= 2^20."""
    t = np.arange(rows)[:, None]
    x = ((t * 5 + np.arange(cin)[None, :] * 3 + t // 11) % 7 - 3).astype(np.float32)
    gy = (2 * ((t * 3 + np.arange(cout)[None, :] * 5 + t // 13) % 4) - 3).astype(np.float32)
    if 0 < slope:
        gy, x = gy * 2, x * 2  # (pre-activations and gradients even: slope * pre and slope * gy are integers)
    o, i = np.arange(cout)[:, None], np.arange(cin)[None, :]
    w = ((o * 2 + i) % 5 - 2).astype(np.float32)
    b = (np.arange(cout) % 5 - 2).astype(np.float32) * (2 if 0 < slope else 1)
    return x, w, b, gy


# ------------------------------------------------------------------------------------------------------------------ max-centre
def mc_reference(x, gamma, beta):
    """By rule, not by any library's tie behaviour: the maximum over k of x [N, K, C] is the first k that attains it; a NaN counts as
    larger than everything and the first NaN wins (the reference expression x - (gamma * x.max(1) + beta) propagates NaN).
    out = x - fl(fl(gamma * max) + beta): three roundings, 3 * 2^-24 * (|x| + |gamma max| + |beta|)."""
    x, gamma, beta = f64(x), f64(gamma), f64(beta)
    n, K, c = x.shape
    isn = np.isnan(x)
    best = np.max(np.where(isn, -np.inf, x), axis=1, keepdims=True)
    hit = np.where(isn.any(axis=1, keepdims=True), isn, x == best)
    am = np.argmax(hit, axis=1)  # first True
    mx = np.take_along_axis(x, am[:, None, :], axis=1)[:, 0, :]
    with np.errstate(all="ignore"):
        out = x - (gamma * mx + beta)[:, None, :]
        bound = 3 * EPS32 * (np.abs(x) + np.abs(gamma * mx)[:, None, :] + np.abs(beta))
    return out, bound, mx, am


def mc_backward_reference(g, mx, am, gamma):
    """s[n, c] = sum_k g;  grad_x = g, minus gamma * s at k = arg-max only (elsewhere grad_x is g itself, bit for bit: bound 0);
    grad_gamma[c] = -sum_n s max,  grad_beta[c] = -sum_n s.  Roundings: s is a chain of K - 1 adds; at the arg-max one product and one
    subtraction more: (K + 1) * 2^-24 * (|g| + |gamma| sum_k |g|).  The parameter sums: K - 1 for s, one product, LN_MC_ITERS adds per
    thread, the fold of the 256 // C point lanes, ceil(blocks / 16) + 16 adds in ln_k_sum_slabs."""
    g, mx, gamma = f64(g), f64(mx), f64(gamma)
    n, K, c = g.shape
    s = g.sum(1)
    sa = np.abs(g).sum(1)
    onehot = np.arange(K)[None, :, None] == am[:, None, :]
    with np.errstate(all="ignore"):
        gx = g - onehot * (gamma * s)[:, None, :]
        b_gx = onehot * ((K + 1) * EPS32 * (np.abs(g) + (np.abs(gamma) * sa)[:, None, :]))
        ggamma, gbeta = -(s * mx).sum(0), -s.sum(0)
        lanes = 256 // c
        blocks = -(-n // (lanes * LN_MC_ITERS)) if n else 0
        chain = (K - 1) + 1 + LN_MC_ITERS + lanes + -(-blocks // 16) + 16
        b_ggamma = chain * EPS32 * (sa * np.abs(mx)).sum(0)
        b_gbeta = chain * EPS32 * sa.sum(0)
    return (gx, ggamma, gbeta), (b_gx, b_ggamma, b_gbeta)


def mc_input(n, K, c, kind, seed):
    """randn; relu (post-activation: many exact zeros, every seventh point a row of zeros only); neginf (-Inf entries, every fifth point
    all -Inf in channel 0); nan (NaN entries: alone, twice in a column, next to +Inf); exact (integers in [-3, 3]: ties everywhere)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, K, c)).astype(np.float32)
    if kind == "relu":
        x = np.maximum(x, 0)
        x[::7] = 0
    elif kind == "neginf":
        x[rng.random((n, K, c)) < 0.15] = -np.inf
        x[::5, :, 0] = -np.inf
    elif kind == "nan":
        x[rng.random((n, K, c)) < 0.05] = np.nan
        x[1::6, K - 1, :] = np.nan
        x[2::6, 0, :] = np.inf
    elif kind == "exact":
        x = rng.integers(-3, 4, (n, K, c)).astype(np.float32)
    return x
