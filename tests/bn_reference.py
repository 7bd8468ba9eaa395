"""fp64 reference and per-element error bounds for the BatchNorm kernels (csrc/ln_norm.hip: k_bn_apply, k_bn_apply_eval,
k_bn_backward_eval, and k_gn_stats / k_gn_backward_apply at one channel per group).  Plain NumPy on the CPU, in the vocabulary of
dense_reference.py: test_bn_reference.py checks this module without a GPU, test_gpu_batch_norm.py holds the kernels to it.

Training mode IS GroupNorm with groups == channels — the statistics come from the same k_gn_stats launch, the backward from the same
k_gn_backward_apply — so its checks are dense_reference's own (assert_gn_statistics, assert_gn_scale_shift, assert_gn_apply,
gn_backward_reference) with groups = c, and the counting arguments written there carry over unchanged.  New here:

running statistics (training, n live rows, n >= 2; with n < 2 they keep their bits):
    running_mean' = (1 - mom) running_mean + mom mean,    running_var' = (1 - mom) running_var + mom var n / (n - 1)
  formed in fp64 from the fp64 moments and rounded to fp32 once: 2^-24 |ref| for that rounding, + mom x the statistic's own allowance,
  which is the project's conditioning requirement (dense_reference.GN_MEAN_RTOL, GN_RSTD_RTOL), not a new number:
    mean: GN_MEAN_RTOL (|mean| + std);   var n / (n - 1): 2 GN_RSTD_RTOL (var + eps) n / (n - 1)
  (rstd = (var + eps)^-1/2 within 1e-5 relative is var + eps within 2e-5 relative).
evaluation forward (statistics = the running ones):
    rstd = fl(1 / sqrt(running_var + eps)) from fp64: one rounding;  a = fl(gamma rstd): 2 * 2^-24 |a| with rstd's;
    b = fl(beta - running_mean a) formed in fp64 from the kernel's fp32 a: 2^-24 (|beta| + 2 |running_mean a|), the bound of
    assert_gn_scale_shift;  y: assert_gn_apply given the kernel's own scale / shift.
evaluation backward:
    dx = fl(g' a): one rounding, one spare: 2 * 2^-24 |g' a|;  dgamma = (ds - db running_mean) rstd and dbeta = db come from the same
    k_gn_stats sums: the dgamma / dbeta bounds of gn_backward_reference with the running mean in the place of the batch mean."""
import numpy as np

from tests import dense_reference as R

EPS32 = R.EPS32
f64, f32 = R.f64, R.f32


def live_rows(m, rows):
    return m if rows is None else max(0, min(int(rows), m))


def bn_statistics(x, eps, rows=None):
    """fp64 channel mean, rstd = 1 / sqrt(var + eps) (biased variance) and std over the live rows."""
    return R.gn_statistics(x, f64(x).shape[1], eps, rows)


def bn_running_reference(x, running_mean, running_var, momentum, eps, rows=None):
    """The running statistics after one training call on x, in fp64, and their bounds.  n < 2: unchanged, bound 0 (bit for bit)."""
    x = f64(x)
    n = live_rows(x.shape[0], rows)
    rm, rv = f64(running_mean), f64(running_var)
    if n < 2:
        return (rm.copy(), rv.copy()), (np.zeros_like(rm), np.zeros_like(rv))
    mean, rstd, std = bn_statistics(x, eps, rows)
    var = std ** 2
    unbias = n / (n - 1.0)
    new_rm = (1.0 - momentum) * rm + momentum * mean
    new_rv = (1.0 - momentum) * rv + momentum * var * unbias
    b_rm = EPS32 * np.abs(new_rm) + momentum * R.GN_MEAN_RTOL * (np.abs(mean) + std)
    b_rv = EPS32 * np.abs(new_rv) + momentum * 2 * R.GN_RSTD_RTOL * (var + eps) * unbias
    return (new_rm, new_rv), (b_rm, b_rv)


def assert_bn_running(got_mean, got_var, x, running_mean, running_var, momentum, eps, rows=None, what=""):
    """Returns the worst error / bound ratios (mean, var); with n < 2 the comparison is bitwise."""
    (rm, rv), (b_rm, b_rv) = bn_running_reference(x, running_mean, running_var, momentum, eps, rows)
    if live_rows(f64(x).shape[0], rows) < 2:
        R.assert_equal_bits(got_mean, running_mean, f"{what} running_mean (fewer than 2 rows: unchanged)")
        R.assert_equal_bits(got_var, running_var, f"{what} running_var (fewer than 2 rows: unchanged)")
        return 0.0, 0.0
    R.assert_within(got_mean, rm, b_rm, f"{what} running_mean")
    R.assert_within(got_var, rv, b_rv, f"{what} running_var")
    return R.worst_ratio(got_mean, rm, b_rm), R.worst_ratio(got_var, rv, b_rv)


def assert_bn_training_forward(y, mean_rstd, scale_shift, x, gamma, beta, eps, relu, rows=None, what=""):
    """Training forward = GroupNorm at groups == channels.  Returns {"rstd", "y"} worst ratios."""
    c = f64(x).shape[1]
    ratios = {"rstd": R.assert_gn_statistics(mean_rstd, x, c, eps, rows, what)}
    R.assert_gn_scale_shift(scale_shift, mean_rstd, gamma, beta, c, c, what)
    ratios["y"] = R.assert_gn_apply(y, x, scale_shift, relu, rows, what)
    return ratios


def bn_training_backward_reference(x, gy, mask, gamma, mean_rstd, rows=None):
    """(dx, dgamma, dbeta), bounds: gn_backward_reference at groups == channels."""
    return R.gn_backward_reference(x, gy, mask, gamma, mean_rstd, f64(x).shape[1], rows)


def bn_eval_affine_reference(gamma, beta, running_mean, running_var, eps):
    """fp64 rstd, a = gamma rstd, b = beta - running_mean a of the evaluation mode."""
    rm, rv = f64(running_mean), f64(running_var)
    c = rm.shape[0]
    gamma = np.ones(c) if gamma is None else f64(gamma)
    beta = np.zeros(c) if beta is None else f64(beta)
    with np.errstate(all="ignore"):
        rstd = 1.0 / np.sqrt(rv + eps)
    a = gamma * rstd
    return rstd, a, beta - rm * a


def assert_bn_eval_forward(y, mean_rstd, scale_shift, x, gamma, beta, running_mean, running_var, eps, relu, rows=None, what=""):
    """mean_rstd = (running_mean bit for bit, rstd within one rounding), a within 2 roundings, b within the shift bound given the
    kernel's own a, y through assert_gn_apply given the kernel's own scale / shift.  Returns {"a", "y"} worst ratios."""
    c = f64(x).shape[1]
    rstd, a, _ = bn_eval_affine_reference(gamma, beta, running_mean, running_var, eps)
    mr = f64(mean_rstd).reshape(2, c)
    ss = f64(scale_shift).reshape(2, c)
    R.assert_equal_bits(f32(mean_rstd).reshape(2, c)[0], running_mean, f"{what} published mean")
    R.assert_within(mr[1], rstd, EPS32 * rstd, f"{what} rstd")
    R.assert_within(ss[0], a, 2 * EPS32 * np.abs(a), f"{what} scale")
    rm = f64(running_mean)
    beta64 = np.zeros(c) if beta is None else f64(beta)
    R.assert_within(ss[1], beta64 - rm * ss[0], EPS32 * (np.abs(beta64) + 2 * np.abs(rm * ss[0])), f"{what} shift")
    return {"a": R.worst_ratio(ss[0], a, 2 * EPS32 * np.abs(a)), "y": R.assert_gn_apply(y, x, scale_shift, relu, rows, what)}


def bn_eval_backward_reference(x, gy, mask, mean_rstd, scale_shift, rows=None):
    """Evaluation backward given the kernel's published (running_mean, rstd) and scale a: dx = g' a, dgamma = sum g' (x - running_mean)
    rstd, dbeta = sum g'; zeros in the rows beyond `rows`.  Returns the three gradients and their bounds."""
    x64, gy64 = f64(x), f64(gy)
    m, c = x64.shape
    live = live_rows(m, rows)
    a = f64(scale_shift).reshape(2, c)[0]
    g = gy64[:live] * (1.0 if mask is None else f64(mask)[:live])
    dx, b_dx = np.zeros_like(x64), np.zeros_like(x64)
    with np.errstate(all="ignore"):
        dx[:live] = g * a
        b_dx[:live] = 2 * EPS32 * np.abs(g * a)
    (_, dgamma, dbeta), (_, b_dgamma, b_dbeta) = R.gn_backward_reference(x, gy, mask, None, mean_rstd, c, rows)
    return (dx, dgamma, dbeta), (b_dx, b_dgamma, b_dbeta)


# ---- the whole layer in fp64 (what torch.nn.BatchNorm1d computes in float64: test_bn_reference.py compares the two) --------------------
def bn_layer_reference(x, gy, gamma, beta, running_mean, running_var, momentum, eps, training, relu=False, rows=None):
    """One call of the layer in fp64: y, (dx, dgamma, dbeta) for the upstream gradient gy, and the running statistics after it.
    training with n < 2 (torch refuses it; the kernels define it): variance 0, rstd = 1 / sqrt(eps), y = act(beta) in the live row, the
    running statistics unchanged; n = 0: zeros only.  Without running statistics (None) the batch statistics are used in either mode."""
    x64 = f64(x)
    m, c = x64.shape
    live = live_rows(m, rows)
    g1 = np.ones(c) if gamma is None else f64(gamma)
    b1 = np.zeros(c) if beta is None else f64(beta)
    batch = training or running_mean is None
    if batch:
        mean, rstd, _ = bn_statistics(x64, eps, rows)
        new_stats = (None, None) if running_mean is None else bn_running_reference(x64, running_mean, running_var, momentum, eps, rows)[0]
    else:
        mean = f64(running_mean)
        rstd = bn_eval_affine_reference(None, None, running_mean, running_var, eps)[0]
        new_stats = (f64(running_mean).copy(), f64(running_var).copy())
    y = np.zeros_like(x64)
    y[:live] = (x64[:live] - mean) * rstd * g1 + b1
    mask = None
    if relu:
        mask = y > 0
        y = np.where(mask, y, 0.0)
    mean_rstd = np.concatenate([mean, rstd])
    if batch:
        grads, _ = bn_training_backward_reference(x64, gy, mask, gamma, mean_rstd, rows)
    else:
        grads, _ = bn_eval_backward_reference(x64, gy, mask, mean_rstd, np.concatenate([g1 * rstd, b1 - mean * g1 * rstd]), rows)
    return y, grads, new_stats
