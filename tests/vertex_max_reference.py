"""NumPy restatement of the vertex-side maximum of PointNetModule (ln_csr_segment_max of include/latticenet_hip.h: k_csr_segment_max and
its decode in csrc/ln_csr.hip), and the dispatch rule of ln_launch_segment_max as a table.  Plain NumPy on the CPU:
test_vertex_max_reference.py checks this module against a brute-force loop without a GPU, tests/test_gpu_vertex_max.py holds the kernels
to it bit for bit.  The fused reduction around it (min_points rule, row 0, barycentric weights, backward) and the centring tail are
restated in tests/cloud_invalid_vertex_reference.py and used from there."""
import numpy as np

NO_TOKEN = np.iinfo(np.int64).max


def segment_max(src, idx, rows):
    """(max [rows, C] float32, arg [rows, C] int32, counts [rows] int64): per (row, channel) the maximum of src[t, c] over the tokens t with
    0 <= idx[t] < rows and idx[t] == row, and the smallest token attaining it; -0.0 and +0.0 are one value (a zero maximum is written as
    +0.0, the smallest token of either sign wins); rows without tokens get 0 / -1.  An element with a NaN among its tokens: the value is
    what np.maximum gives and arg is -1 — the kernels' answer there is not specified, the tests do not compare it."""
    src = np.asarray(src, dtype=np.float32)
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    tokens, ch = src.shape
    assert idx.size == tokens
    out = np.zeros((rows, ch), dtype=np.float32)
    arg = np.full((rows, ch), -1, dtype=np.int32)
    tok = np.flatnonzero((idx >= 0) & (idx < rows))
    counts = np.bincount(idx[tok], minlength=rows).astype(np.int64)
    if tok.size == 0:
        return out, arg, counts
    tok = tok[np.argsort(idx[tok], kind="stable")]  # by row, tokens ascending inside a row
    row_of = idx[tok]
    starts = np.flatnonzero(np.concatenate([[True], row_of[1:] != row_of[:-1]]))
    present = row_of[starts]
    vals = src[tok]
    vals = np.where(vals == 0, np.float32(0), vals)
    best = np.maximum.reduceat(vals, starts, axis=0)
    # second pass: the smallest token among those that equal their row's maximum
    seg = np.repeat(np.arange(starts.size), np.diff(np.concatenate([starts, [tok.size]])))
    cand = np.where(vals == best[seg], tok[:, None], NO_TOKEN)
    win = np.minimum.reduceat(cand, starts, axis=0)
    out[present] = best
    arg[present] = np.where(win == NO_TOKEN, -1, win).astype(np.int32)
    return out, arg, counts


# ln_launch_segment_max: a lane owns VEC channels (4 when channels % 4 == 0 and the source is 16-byte aligned, else 1); the run-combining
# form COMB is taken when the lanes of one segment, channels / VEC, are a power of two <= 64 (no segment straddles a wave).
def segment_max_instance(channels, aligned):
    """(VEC, COMB) of the k_csr_segment_max instance that serves rows of `channels` floats (aligned: the source pointer is a multiple of 16)."""
    vec = 4 if (channels % 4 == 0 and aligned) else 1
    lanes = channels // vec
    return vec, bool(lanes <= 64 and (lanes & (lanes - 1)) == 0)


# instance -> the (channels, source aligned) pairs the GPU tests run it at.  4: 64 lane groups per wave; 256: one lane group per wave (the
# shuffle loop runs zero times, only the LDS hand-over combines); 260: more than 64 lanes per segment; offset sources: the scalar lanes
# at widths the vector instances would take.
DISPATCH = {
    (4, True): [(4, True), (8, True), (32, True), (64, True), (256, True)],
    (4, False): [(12, True), (96, True), (260, True)],
    (1, True): [(1, True), (2, True), (8, False), (64, False)],
    (1, False): [(3, True), (7, True), (128, False)],
}
