"""The NumPy segment maximum the GPU tests hold k_csr_segment_max to (tests/vertex_max_reference.py), without a GPU: against a brute-force
loop over rows, channels and tokens on a few hundred tokens with ties, zeros of both signs, infinities, denormals, rows of only negative
values and ids that name no row; the generalised arguments of the fused reduction's restatement (bary_stride, grad_stride, ids >= rows);
and the dispatch table of ln_launch_segment_max the GPU tests are parametrised over."""
import numpy as np
import pytest

from tests import cloud_invalid_vertex_reference as V
from tests import vertex_max_reference as R


def brute_force(src, idx, rows):
    tokens, ch = src.shape
    out = np.zeros((rows, ch), np.float32)
    arg = np.full((rows, ch), -1, np.int32)
    counts = np.zeros(rows, np.int64)
    for r in range(rows):
        for c in range(ch):
            best = None
            for t in range(tokens):
                if idx[t] != r:
                    continue
                x = src[t, c]
                if best is None or x > best:  # (-0.0 > +0.0 is False: equal zeros keep the first token)
                    best, arg[r, c] = x, t
            if best is not None:
                out[r, c] = best
        counts[r] = int(np.sum(idx == r))
    return out, arg, counts


def same_value(a, b):
    """Bit for bit, except that zeros of either sign are equal."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))))


def special_case():
    """300 tokens over 12 rows, 5 channels: integer ties everywhere, then rows of special values."""
    rng = np.random.default_rng(3)
    rows, tokens, ch = 12, 300, 5
    idx = rng.integers(-1, rows + 2, tokens)  # -1, rows and rows + 1 name no row
    idx[idx == 7] = 3                          # row 7 has no token
    src = rng.integers(-3, 4, (tokens, ch)).astype(np.float32)
    tiny = np.float32(2.0 ** -149)

    def toks(r):
        return np.flatnonzero(idx == r)

    src[toks(1)] = -np.abs(src[toks(1)]) - 1                                   # only negative values
    src[toks(2)] = -np.inf                                                     # only -Inf
    src[toks(4)[[3, 9]]] = np.inf                                              # +Inf twice: the smaller token
    src[toks(5)] = np.where(rng.random((toks(5).size, ch)) < 0.5, -0.0, 0.0)   # zeros of both signs
    src[toks(5)[0]] = -0.0
    src[toks(6)] = np.where(rng.random((toks(6).size, ch)) < 0.5, -0.0, -2.0)  # -0.0 above negative values
    src[toks(8)] = rng.integers(-5, 6, (toks(8).size, ch)).astype(np.float32) * tiny  # denormals of both signs
    src[toks(8), 0] = -np.abs(src[toks(8), 0]) - tiny                          # ... one channel of negative denormals only
    src[toks(9)[::2]] = -np.inf                                                # -Inf beside finite values
    return src, idx, rows


def test_segment_max_against_brute_force():
    src, idx, rows = special_case()
    out, arg, counts = R.segment_max(src, idx, rows)
    eo, ea, ec = brute_force(src, idx, rows)
    assert out.dtype == np.float32 and arg.dtype == np.int32 and counts.dtype == np.int64
    assert same_value(out, eo) and np.array_equal(arg, ea) and np.array_equal(counts, ec)
    t = lambda r: np.flatnonzero(idx == r)
    assert (out[1] < 0).all() and (out[2] == -np.inf).all() and (arg[2] == t(2)[0]).all()
    assert (out[4] == np.inf).all() and (arg[4] == t(4)[3]).all()
    assert (out[5] == 0).all() and (arg[5] == t(5)[0]).all() and (out[6] == 0).all()
    assert not out[7].any() and (arg[7] == -1).all() and counts[7] == 0
    assert (out[8, 0] < 0).all() and (np.abs(out[8]) <= 5 * 2.0 ** -149).all() and out[8].any()  # denormals come back as they are
    assert np.isfinite(out[9]).all()
    assert counts.sum() == np.sum((idx >= 0) & (idx < rows))


def test_segment_max_random_rows_and_empty_input():
    rng = np.random.default_rng(4)
    idx = rng.integers(-2, 40, 500)
    src = rng.standard_normal((500, 3)).astype(np.float32)
    src[::3] = np.round(src[::3])
    out, arg, counts = R.segment_max(src, idx, 33)  # ids 33 .. 39 name no row
    eo, ea, ec = brute_force(src, idx, 33)
    assert same_value(out, eo) and np.array_equal(arg, ea) and np.array_equal(counts, ec)
    out, arg, counts = R.segment_max(np.zeros((4, 2), np.float32), np.full(4, -1), 3)
    assert not out.any() and (arg == -1).all() and not counts.any()


def test_a_nan_touches_its_own_element_only():
    src, idx, rows = special_case()
    base = R.segment_max(src, idx, rows)
    poisoned = src.copy()
    poisoned[np.flatnonzero(idx == 3)[2], 1] = np.nan
    out, arg, _ = R.segment_max(poisoned, idx, rows)
    rest = np.ones((rows, src.shape[1]), bool)
    rest[3, 1] = False
    assert same_value(out[rest], base[0][rest]) and np.array_equal(arg[rest], base[1][rest])


def test_the_fused_restatement_agrees_with_the_segment_max():
    """pointnet_reduce (a lexsort per channel) and segment_max (reduceat) are written independently: they name the same winners; the
    barycentric half reads bary[t * bary_stride]; ids >= rows belong to no row; grad_stride addresses a flat grad_out."""
    src, idx, rows = special_case()
    ch = src.shape[1]
    rng = np.random.default_rng(5)
    bary = rng.standard_normal(src.shape[0] * 5).astype(np.float32)
    m, a, n = R.segment_max(src, idx, rows)
    for min_points in (1, 4, 30):
        for stride in (1, 5):
            out, arg, counts = V.pointnet_reduce(src, idx, bary, rows, min_points, bary_stride=stride)
            keep = (n >= min_points) & (n > 0) & (np.arange(rows) != 0)
            assert np.array_equal(counts, n) and keep.any() and not keep.all()
            assert same_value(out[keep, :ch], m[keep]) and np.array_equal(arg[keep], a[keep])
            assert np.array_equal(out[keep, ch:], bary[a[keep].astype(np.int64) * stride])
            assert not out[~keep].any() and (arg[~keep] == -1).all()
    out, arg, _ = V.pointnet_reduce(src, idx, bary, rows, 1)
    inside = np.where(idx < rows, idx, -1)
    g2 = rng.standard_normal((rows, 2 * ch)).astype(np.float32)
    grad = V.pointnet_reduce_backward(g2, arg, inside, src.shape[0])
    assert np.array_equal(grad, V.pointnet_reduce_backward(g2.reshape(-1), arg, inside, src.shape[0], grad_stride=2 * ch))
    tight = np.ascontiguousarray(g2[:, :ch])
    assert np.array_equal(grad, V.pointnet_reduce_backward(tight.reshape(-1), arg, inside, src.shape[0], grad_stride=ch))
    for t in range(src.shape[0]):
        for c in range(ch):
            want = g2[inside[t], c] if inside[t] >= 0 and arg[inside[t], c] == t else 0.0
            assert grad[t, c] == want


@pytest.mark.parametrize("instance", list(R.DISPATCH))
def test_every_instance_has_a_width_in_its_row_of_the_table(instance):
    cases = R.DISPATCH[instance]
    assert cases and all(R.segment_max_instance(c, aligned) == instance for c, aligned in cases)


def test_the_dispatch_table_and_the_edges_of_the_rule():
    assert set(R.DISPATCH) == {(4, True), (4, False), (1, True), (1, False)}
    assert [c for c, _ in R.DISPATCH[(4, True)]] == [4, 8, 32, 64, 256] and all(a for _, a in R.DISPATCH[(4, True)])
    assert [c for c, _ in R.DISPATCH[(4, False)]] == [12, 96, 260]
    assert R.DISPATCH[(1, True)] == [(1, True), (2, True), (8, False), (64, False)]
    assert R.DISPATCH[(1, False)] == [(3, True), (7, True), (128, False)]
    # the edges of the rule: 64 lanes still combine, 65 do not; an unaligned source never takes the vector lanes
    assert R.segment_max_instance(256, True) == (4, True) and R.segment_max_instance(260, True) == (4, False)
    assert R.segment_max_instance(64, False) == (1, True) and R.segment_max_instance(128, False) == (1, False)
    assert R.segment_max_instance(4, True) == (4, True) and R.segment_max_instance(4, False) == (1, True)
