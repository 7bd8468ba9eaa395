"""NumPy restatement of the per-cloud "invalid vertex" rule of a batch of clouds in one lattice
(Lattice.set_cloud_batch(per_cloud_invalid_vertex=True); ln_distribute_centre_clouds, ln_pointnet_reduce_forward_clouds and
ln_pointnet_reduce_backward of include/latticenet_hip.h).  Plain NumPy on the CPU, float32 where the kernels compute in float32:
test_cloud_invalid_vertex_reference.py checks this module without a GPU, the GPU tests hold the kernels to it bit for bit."""
import numpy as np


def cloud_of_token(t, tokens_per_cloud, clouds):
    """Token t belongs to cloud min(t / tokens_per_cloud, clouds - 1): the last cloud takes what is left."""
    return np.minimum(np.asarray(t, dtype=np.int64) // int(tokens_per_cloud), clouds - 1)


def invalid_rows(row_starts, rows):
    """bool [rows]: row r is the invalid vertex of cloud c exactly when r == row_starts[c] and row_starts[c] < row_starts[c + 1].  An empty
    cloud has none, row_starts[clouds] itself is none (rows from there on belong to no cloud)."""
    rs = [int(v) for v in row_starts]
    out = np.zeros(rows, dtype=bool)
    for c in range(len(rs) - 1):
        if rs[c] < rs[c + 1] and 0 <= rs[c] < rows:
            out[rs[c]] = True
    return out


def distribute_centre(d, idx, sums, counts, pos_dim, tokens_per_cloud=None, row_starts=None):
    """out[t, :pos_dim] = d[t, :pos_dim] - sums[idx[t]] / max(counts[idx[t]], 1) in float32, the other columns copied; the row of token t is
    zero when idx[t] < 0 or idx[t] == row_starts[cloud of t].  row_starts None: the single-cloud rule, zero when idx[t] <= 0."""
    d = np.asarray(d, dtype=np.float32)
    idx = np.asarray(idx, dtype=np.int64)
    tokens = d.shape[0]
    if row_starts is None:
        dropped = idx <= 0
    else:
        clouds = len(row_starts) - 1
        first = np.asarray(row_starts, dtype=np.int64)[cloud_of_token(np.arange(tokens), tokens_per_cloud, clouds)]
        dropped = (idx < 0) | (idx == first)
    safe = np.where(idx >= 0, idx, 0)
    out = d.copy()
    denom = np.maximum(np.asarray(counts, dtype=np.int64)[safe], 1).astype(np.float32)
    out[:, :pos_dim] = d[:, :pos_dim] - np.asarray(sums, dtype=np.float32)[safe] / denom[:, None]
    out[dropped] = 0
    return out


def _ordered(x):
    """float32 -> uint32 whose unsigned order is the order of the floats: what the segment max compares."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def pointnet_reduce(src, idx, bary, rows, min_points, row_starts=None, bary_stride=1):
    """(out [rows, 2C] float32, arg [rows, C] int32, counts [rows]): per row the maximum over its tokens of src[t, c] (equal values: the
    smallest token) and the barycentric weight bary[t * bary_stride] of the winning token t; rows with fewer than min_points tokens and
    invalid rows (row 0 when row_starts is None) are zero with arg = -1, and so are rows without a token.  Tokens with idx outside
    [0, rows) belong to no row."""
    src = np.asarray(src, dtype=np.float32)
    src = np.where(src == 0, np.float32(0), src)  # -0 and +0 are one value to the maximum: it is written as +0, ties go to the smallest token
    idx = np.asarray(idx, dtype=np.int64)
    bary = np.asarray(bary, dtype=np.float32).reshape(-1)
    tokens, ch = src.shape
    tok = np.flatnonzero((idx >= 0) & (idx < rows))
    counts = np.bincount(idx[tok], minlength=rows)
    if row_starts is None:
        invalid = np.arange(rows) == 0
    else:
        invalid = invalid_rows(row_starts, rows)
    keep = (counts >= min_points) & ~invalid & (counts > 0)
    out = np.zeros((rows, 2 * ch), dtype=np.float32)
    arg = np.full((rows, ch), -1, dtype=np.int32)
    row_of = idx[tok]
    for c in range(ch):
        key = _ordered(src[tok, c]).astype(np.int64)
        order = np.lexsort((tok, -key, row_of))  # by row, then largest value, then smallest token
        first = np.ones(order.size, dtype=bool)
        first[1:] = row_of[order][1:] != row_of[order][:-1]
        win_tok, win_row = tok[order][first], row_of[order][first]
        ok = keep[win_row]
        arg[win_row[ok], c] = win_tok[ok]
        out[win_row[ok], c] = src[win_tok[ok], c]
        out[win_row[ok], ch + c] = bary[win_tok[ok] * bary_stride]
    return out, arg, counts


def pointnet_reduce_backward(grad_out, arg, idx, tokens, grad_stride=None):
    """grad_src[t, c] = grad_out[idx[t], c] if arg[idx[t], c] == t else 0 (grad_out [rows, >= C]: the first C columns are the maxima's;
    with grad_stride, grad_out is flat and row r starts at r * grad_stride)."""
    grad_out = np.asarray(grad_out, dtype=np.float32)
    idx = np.asarray(idx, dtype=np.int64)
    ch = arg.shape[1]
    if grad_stride is not None:
        flat = np.ascontiguousarray(grad_out).reshape(-1)
        assert flat.size >= (arg.shape[0] - 1) * grad_stride + ch
        grad_out = np.lib.stride_tricks.as_strided(flat, (arg.shape[0], ch), (4 * grad_stride, 4))
    g = np.zeros((tokens, ch), dtype=np.float32)
    t = np.flatnonzero(idx >= 0)
    won = arg[idx[t]] == t[:, None]
    g[t] = np.where(won, grad_out[idx[t], :ch], 0)
    return g


def make_batch(sizes, tokens_per_cloud, ch=6, width=5, pos_dim=3, seed=0, short_last=0):
    """Clouds of `sizes[c]` rows and tokens_per_cloud tokens each (the last one `short_last` tokens fewer); token indices of a cloud lie in
    its own row range or are -1; the first row of every cloud that has rows gets at least 5 tokens."""
    rng = np.random.default_rng(seed)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    parts = []
    for c, m in enumerate(sizes):
        n = tokens_per_cloud - (short_last if c == len(sizes) - 1 else 0)
        if m == 0:
            parts.append(np.full(n, -1))
            continue
        local = rng.integers(-1, m, n)
        local[rng.choice(n, 5, replace=False)] = 0
        parts.append(np.where(local >= 0, local + starts[c], -1))
    idx = np.concatenate(parts)
    tokens = idx.size
    d = rng.standard_normal((tokens, width)).astype(np.float32)
    rows = int(starts[-1])
    counts = np.bincount(idx[idx >= 0], minlength=rows)
    sums = np.zeros((rows, pos_dim), np.float32)
    np.add.at(sums, idx[idx >= 0], d[idx >= 0, :pos_dim])
    src = rng.standard_normal((tokens, ch)).astype(np.float32).round(1)  # (rounded: equal values, ties go to the smallest token)
    return dict(idx=idx, d=d, sums=sums, counts=counts, src=src, starts=starts, rows=rows, tokens=tokens, pos_dim=pos_dim)
