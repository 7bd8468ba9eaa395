"""NumPy restatement of the row ranges of a batch of clouds in one lattice (Lattice.cloud_row_starts, k_cloud_row_starts of
csrc/ln_norm.hip) and the per-range GroupNorm checks built on tests/dense_reference.py.  Plain NumPy on the CPU:
test_cloud_batch_ranges.py checks this module without a GPU, the GPU tests hold the kernels to it."""
import numpy as np

from tests import dense_reference as R


def cloud_of_key(key0, step, clouds):
    """Cloud of a vertex from the first coordinate of its key: cloud c is shifted by c * step and stays within half a step of the origin."""
    key0 = np.asarray(key0, dtype=np.int64)
    return np.clip(np.floor_divide(key0 + step // 2, step), 0, clouds - 1)


def row_starts_of_clouds(cloud_of_row, clouds):
    """(row_starts [clouds + 1], order flag): row_starts[c] = first row whose cloud is >= c (cloud-major rows: the first row of cloud
    c; a cloud without a row starts where the next one does), row_starts[clouds] = number of rows; flag = some row's cloud is smaller
    than its predecessor's."""
    cloud_of_row = np.asarray(cloud_of_row, dtype=np.int64)
    flag = int(bool((np.diff(cloud_of_row) < 0).any()))
    starts = np.searchsorted(cloud_of_row, np.arange(clouds + 1), side="left") if not flag else None
    return starts, flag


def row_starts_of_splat_indices(idx, points_per_cloud, tokens_per_point, clouds, rows):
    """The ranges from the splat indices of a build (idx [points * tokens_per_point], -1 = no vertex): every vertex belongs to the
    cloud of the points that touch it, and no vertex is touched by two clouds."""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    cloud_of_token = (np.arange(idx.size) // tokens_per_point) // points_per_cloud
    ok = idx >= 0
    cloud_of_row = np.full(rows, -1, np.int64)
    cloud_of_row[idx[ok]] = cloud_of_token[ok]
    assert (cloud_of_row >= 0).all(), "a vertex no point touches"
    assert np.array_equal(cloud_of_row[idx[ok]], cloud_of_token[ok]), "a vertex shared by two clouds"
    return row_starts_of_clouds(cloud_of_row, clouds)


def segments(row_starts, m, rows=None):
    """[(lo, hi)] per range the way the kernels clamp them: the rows that count end at min(m, row_starts[-1], rows)."""
    rs = [int(v) for v in row_starts]
    live = max(0, min(m, rs[-1], m if rows is None else int(rows)))
    out = []
    for s in range(len(rs) - 1):
        lo = min(max(rs[s], 0), live)
        out.append((lo, min(max(rs[s + 1], lo), live)))
    return out, live


def module_groups(c):
    """GroupNormLatticeModule's rule."""
    return 32 if c % 32 == 0 else max(c // 2, 1)


def check_forward(x, y, mean_rstd, scale_shift, gamma, beta, groups, eps, relu, row_starts, rows=None, what=""):
    """Every range against the fp64 GroupNorm reference of its rows alone (dense_reference's bounds), zeros behind the last range.
    Returns the worst error / bound ratios."""
    m, c = x.shape
    segs, live = segments(row_starts, m, rows)
    y = R.f32(y)
    worst = {"rstd": 0.0, "y": 0.0}
    assert not y[live:].any(), f"{what}: y is not zero behind row {live}"
    for s, (lo, hi) in enumerate(segs):
        if hi == lo:
            continue
        w = f"{what} range {s} [{lo}, {hi})"
        worst["rstd"] = max(worst["rstd"], R.assert_gn_statistics(mean_rstd[s], x[lo:hi], groups, eps, None, w))
        R.assert_gn_scale_shift(scale_shift[s], mean_rstd[s], gamma, beta, c, groups, w)
        worst["y"] = max(worst["y"], R.assert_gn_apply(y[lo:hi], x[lo:hi], scale_shift[s], relu, None, w))
    return worst


def backward_reference(x, gy, y, mean_rstd, gamma, groups, relu, row_starts, rows=None):
    """fp64 gradients and bounds: grad_x per range from that range's reference, grad_gamma / grad_beta the sums of the ranges'
    references with the sums of their bounds (one bound per term of the sum over clouds)."""
    m, c = x.shape
    segs, live = segments(row_starts, m, rows)
    dx, b_dx = np.zeros((m, c)), np.zeros((m, c))
    dg, b_dg, db, b_db = np.zeros(c), np.zeros(c), np.zeros(c), np.zeros(c)
    mask = (R.f32(y) > 0) if relu else None
    for s, (lo, hi) in enumerate(segs):
        if hi == lo:
            continue
        ref, bound = R.gn_backward_reference(x[lo:hi], gy[lo:hi], None if mask is None else mask[lo:hi], gamma, mean_rstd[s], groups)
        dx[lo:hi], b_dx[lo:hi] = ref[0], bound[0]
        dg, b_dg, db, b_db = dg + ref[1], b_dg + bound[1], db + ref[2], b_db + bound[2]
    return (dx, dg, db), (b_dx, b_dg, b_db)
