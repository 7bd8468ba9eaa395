"""fp64 references and per-element bounds for the lattice convolution between TWO lattices (csrc/ln_conv.hip, csrc/ln_conv_f16.hip:
coarsen and finefy, where the mq query rows and the mn gathered rows belong to different lattices).  Plain NumPy on the CPU, in the
vocabulary of dense_reference.py: test_conv_reference.py checks this module without a GPU, test_gpu_conv_two_lattices.py holds the
kernels to it at the filter extent E = 9, test_gpu_conv_filter_extents.py at E = 1, 5, 7, 11, 13, 15, 17 (every function here takes any E >= 1).

The three products of one convolution out = conv(nbr_q, vals, W), vals [mn, V], W [E V, F], G = d loss / d out [mq, F]:
    forward      out[m, f]      = sum_e sum_v vals[nbr_q[m, e], v] W[e V + v, f]                      (mq rows)
    grad_filter  gW[e V + v, f] = sum_m vals[nbr_q[m, e], v] G[m, f]                                  (over mq rows)
    grad_values  gv[n, v]       = sum_e sum_f G[nbr_n[n, flip(e)], f] W[e V + v, f]                   (mn rows)
an absent neighbour (-1) contributes a zero row; flip(e) = e ^ 1 for e < E - 1, the last slot maps to itself (LN_CONV_FLIP_NEIGHBOURS);
grad_values is `forward` on G over the list with the roles swapped, with the slots flipped and the bank read as its per-slot transpose
(LN_CONV_TRANSPOSED_FILTER).  Each reference comes with `bound`, the same product on the absolute values of every operand: what an
evaluation in ANY order can be off by is a multiple of 2^-24 of it (close_terms of test_gpu_parity.py), and it dominates every partial
sum of the product in any order.

Two operand families (dense_reference.py): `random` (each element within rtol * bound of the fp64 result) and `exact` (small integers:
every partial sum is an integer below 2^24, so the fp32 result is the fp64 result bit for bit in any summation order, through the bf16x3
split as well: an integer below 2^8 is one bf16)."""
import numpy as np

from tests import dense_reference as R

f64, f32 = R.f64, R.f32
HOT_ROWS = 80  # rows of one slot that name the same id: more than a 64-row tile


def flip_slots(E):
    """slot read in the place of slot e under LN_CONV_FLIP_NEIGHBOURS"""
    return [e ^ 1 for e in range(E - 1)] + [E - 1]


def _one_list(rows, into, E, rng, lo):
    """[rows, E] int32, ids in [lo, into) or -1, drawn independently; planted by construction at every extent E >= 1: row rows - 1
    wholly absent (in the partial last tile), rows 0 and rows - 2 without an absent neighbour, the id `lo` and the largest id into - 1,
    and the largest id HOT_ROWS times in a row of slot 1 (across a 64-row tile boundary; slot 0 at E = 1, where it is the only one)."""
    assert rows >= HOT_ROWS + 8 and into >= lo + 2 and E >= 1
    n = rng.integers(lo - 1, into, (rows, E)).astype(np.int32)
    n[n == lo - 1] = -1
    for r in (0, rows - 2):
        n[r] = rng.integers(lo, into, E)
    n[1, 0] = lo
    n[2, E - 1] = into - 1
    n[3:3 + HOT_ROWS, min(1, E - 1)] = into - 1
    n[rows - 1] = -1
    return n


def two_lattice_lists(mq, mn, E, rng, row0_unreferenced=False):
    """(nbr_q [mq, E] with ids in [0, mn) or -1, nbr_n [mn, E] with ids in [0, mq) or -1) as a coarse / fine pair has them, the two drawn
    independently (the backward does not require them to be mutual) and without an identity slot.  `row0_unreferenced`: the id 0 appears
    in neither list (the smallest id is 1), for the run that poisons row 0 of the gathered operand."""
    lo = 1 if row0_unreferenced else 0
    return _one_list(mq, mn, E, rng, lo), _one_list(mn, mq, E, rng, lo)


def small_list(rows, into, E, rng, row0_unreferenced=False):
    """[rows, E] int32 for ANY row count from 1 on (_one_list needs 88 rows for what it plants): the cases at the edges of the kernels'
    own row tiles (1, 15 .. 17, 63 .. 65 rows).  Ids drawn independently in [lo, into) (lo = 1 with `row0_unreferenced`), about one
    entry in eight absent (as in _one_permutation: absent neighbours inside every partial tile); planted: row 0 without an absent
    neighbour and naming the largest id into - 1 in its last slot, and, where there is more than one row, row rows - 1 wholly absent."""
    lo = 1 if row0_unreferenced else 0
    assert rows >= 1 and into >= lo + 2 and E >= 1
    n = rng.integers(lo, into, (rows, E)).astype(np.int32)
    n[rng.random((rows, E)) < 0.125] = -1
    n[0] = rng.integers(lo, into, E)
    n[0, E - 1] = into - 1
    if rows > 1:
        n[rows - 1] = -1
    return n


def _one_permutation(rows, into, rng, lo):
    """[rows, 1] int32: every id of [lo, into) at most once, the other rows absent (about one in eight, and all that the ids do not
    reach); rows 0 and rows - 2 present, the ids `lo` and into - 1 named, row rows - 1 absent."""
    assert rows >= 8 and into >= lo + 4
    n = np.full((rows, 1), -1, np.int32)
    at = rng.permutation(rows - 3) + 1                     # rows 1 .. rows - 3 in random order; rows 0 and rows - 2 taken below
    ids = rng.permutation(np.arange(lo + 1, into - 1))     # the ids between the two ends
    k = min(at.size - at.size // 8, ids.size)
    n[at[:k], 0] = ids[:k]
    n[0, 0], n[rows - 2, 0] = lo, into - 1
    return n


def permutation_lists(mq, mn, rng, row0_unreferenced=False):
    """The E = 1 pair: one-column lists that are NOT the identity (the per-row linear layers pass the identity, the kernels trust
    whatever ids they are given): an injective map with absent entries in each direction, drawn independently."""
    lo = 1 if row0_unreferenced else 0
    return _one_permutation(mq, mn, rng, lo), _one_permutation(mn, mq, rng, lo)


def list_properties(nbr, into):
    """What _one_list plants, read back from a list (for the CPU test)."""
    nbr = np.asarray(nbr)
    valid = nbr[nbr >= 0]
    hot = 0
    for e in range(nbr.shape[1]):
        ids, counts = np.unique(nbr[:, e][nbr[:, e] >= 0], return_counts=True)
        hot = max(hot, int(counts.max()) if counts.size else 0)
    return {"in_range": bool(nbr.min() >= -1 and nbr.max() < into), "all_absent_rows": int(np.sum(np.all(nbr < 0, axis=1))),
            "full_rows": int(np.sum(np.all(nbr >= 0, axis=1))), "has_zero": bool(np.any(valid == 0)), "has_largest": bool(np.any(valid == into - 1)),
            "hot": hot}


def operands(family, mq, mn, E, V, F, rng, half=False):
    """(vals [mn, V], W [E V, F], G [mq, F]) as fp32 arrays (`half`: every element an fp16 number).
    random: N(0, 1) rows scaled per row by exp(U(-6, 6)) for vals and G (both are gathered and split into bf16 parts by one of the three
    products), W ~ N(0, 1 / (E V)); with `half` no exponent spread.  exact: small integers (smaller with `half`: results below 2048)."""
    if family == "exact":
        a, w = (2, 1) if half else (3, 2)
        return (rng.integers(-a, a + 1, (mn, V)).astype(np.float32), rng.integers(-w, w + 1, (E * V, F)).astype(np.float32),
                rng.integers(-a, a + 1, (mq, F)).astype(np.float32))
    assert family == "random"
    vals, G = rng.standard_normal((mn, V)), rng.standard_normal((mq, F))
    W = rng.standard_normal((E * V, F)) / np.sqrt(E * V)
    if half:
        return tuple(x.astype(np.float16).astype(np.float32) for x in (vals, W, G))
    vals = vals * np.exp(rng.uniform(-6, 6, (mn, 1)))
    G = G * np.exp(rng.uniform(-6, 6, (mq, 1)))
    return vals.astype(np.float32), W.astype(np.float32), G.astype(np.float32)


def _gather(x, ids):
    """rows of x by id, a zero row for an absent neighbour (whatever row 0 holds)"""
    return np.where(ids[:, None] >= 0, x[np.maximum(ids, 0)], 0.0)


def forward(nbr, vals, W, flip=False, transposed=False):
    """out [rows of nbr, F] in fp64 and its bound.  W: [E V, F]; `transposed`: the [E F, V] bank of the convolution being differentiated,
    slot e contributes through filter[e F:(e + 1) F, :]^T."""
    nbr, vals, W = np.asarray(nbr), f64(vals), f64(W)
    E, V = nbr.shape[1], vals.shape[1]
    bank = W.reshape(E, -1, V).transpose(0, 2, 1) if transposed else W.reshape(E, V, -1)
    slots = flip_slots(E) if flip else list(range(E))
    out = np.zeros((nbr.shape[0], bank.shape[2]))
    bound = np.zeros_like(out)
    for e in range(E):
        rows = _gather(vals, nbr[:, slots[e]])
        out += rows @ bank[e]
        bound += np.abs(rows) @ np.abs(bank[e])
    return out, bound


def grad_filter(nbr_q, vals, G):
    """gW [E V, F] in fp64 and its bound"""
    nbr_q, vals, G = np.asarray(nbr_q), f64(vals), f64(G)
    E, V = nbr_q.shape[1], vals.shape[1]
    out = np.zeros((E, V, G.shape[1]))
    bound = np.zeros_like(out)
    for e in range(E):
        rows = _gather(vals, nbr_q[:, e])
        out[e] = rows.T @ G
        bound[e] = np.abs(rows).T @ np.abs(G)
    return out.reshape(E * V, -1), bound.reshape(E * V, -1)


def grad_values(nbr_n, G, W):
    """gv [mn, V] in fp64 and its bound: the forward on G over the swapped list with both flags"""
    return forward(nbr_n, G, W, flip=True, transposed=True)


def assert_exact_family(bound, ref=None, half=False, what=""):
    """The magnitude condition of the `exact` family, asserted on the reference before anything is compared with it: the sum of the
    magnitudes of an element's terms (which dominates every partial sum in any order) below 2^24; fp16 results below 2048."""
    assert float(np.max(bound)) < 2 ** 24, f"{what}: partial sums may reach {float(np.max(bound))}, not exact in fp32"
    if half:
        assert float(np.max(np.abs(ref))) < 2048, f"{what}: results up to {float(np.max(np.abs(ref)))} are not exact in fp16"


def _shares(got, ref, bound, rtol, rel):
    err = np.abs(got - ref)
    lim = rtol * bound + rel * np.abs(ref)
    with np.errstate(invalid="ignore"):
        share = np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), np.where(err > 0, np.inf, 0.0))
    return err, lim, np.where(np.isfinite(got), share, np.inf)


def worst_share(got, ref, bound, rtol, rel=0.0):
    """The largest share of its allowance rtol * bound + rel * |ref| that any element uses (inf: an element is not finite, or off where
    nothing is allowed).  A figure to print, never asserted on."""
    share = _shares(f64(got), f64(ref), f64(bound), rtol, rel)[2]
    return float(np.max(share)) if share.size else 0.0


def within(got, ref, bound, rtol, what="", rel=0.0):
    """Element by element |got - ref| <= rtol * bound + rel * |ref|; an element that is not finite where the fp64 result is fails.
    Reports the worst element; returns worst_share."""
    got, ref, bound = f64(got), f64(ref), f64(bound)
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(bound)), f"{what}: the reference is not finite"
    lost = ~np.isfinite(got)
    if lost.any():
        i = tuple(int(k) for k in np.argwhere(lost)[0])
        raise AssertionError(f"{what}: {int(lost.sum())} elements not finite, first {i}: got {got[i]!r}, fp64 {ref[i]!r}")
    err, lim, share = _shares(got, ref, bound, rtol, rel)
    i = np.unravel_index(int(np.argmax(share)), share.shape) if share.size else ()
    worst = float(share[i]) if share.size else 0.0
    assert worst <= 1.0, (f"{what}: {int(np.sum(share > 1.0))} elements outside the bound, worst {tuple(int(k) for k in i)}: got {got[i]!r}, fp64 {ref[i]!r}, "
                          f"error {err[i]:.3e} = {worst:.3g} x allowed {lim[i]:.3e}")
    return worst


def exact(got, ref, what=""):
    """`exact` family: the result is the integer result itself"""
    got = f64(got)
    lost = ~np.isfinite(got)
    if lost.any():
        i = tuple(int(k) for k in np.argwhere(lost)[0])
        raise AssertionError(f"{what}: {int(lost.sum())} elements not finite, first {i}: got {got[i]!r}, exact {f64(ref)[i]!r}")
    R.assert_exact(got, ref, what)
