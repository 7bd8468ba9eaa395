"""fp64 reference, per-element error bound and case list for the fp16 slice forward: k_slice_forward_f16 behind ln_slice_forward_f16 /
ln_slice_forward_f16_prepare_backward (csrc/ln_rows.hip) — fp16 lattice rows in, fp32 arithmetic, fp16 sliced rows out.  NumPy on the
CPU: test_slice_f16_reference.py checks this module without a GPU, test_gpu_slice_f16.py holds the kernel to it.

Vocabulary of point_reference.py and dense_reference.py.  Tokens come without a hash build: idx = random rows in [0, m) with a share
of -1, w barycentric-like with w = -1 in the absent slots — a kernel that fails to skip an absent vertex is off by a whole row (row 0,
which is all NaN in the cases where no token names it).  Every case has three runs:
- random: standard-normal values rounded to fp16; every element within slice_f16_bound of the fp64 sum over the fp16 inputs;
- cancel: the rows a point reads alternate in sign at near-equal magnitude and the weights of its even and odd slots sum to the same,
  so that |ref| << mag: the bound is then a few fp32 roundings of mag, far below one fp16 rounding of a partial sum;
- exact : values integers in [-64, 64], w multiples of 1/8 in [-1, 1]: every product and every partial sum is a multiple of 1/8 below
  2^10, which fp32 holds exactly (13 bits), so the kernel's fp32 sum IS the fp64 sum and its output is that sum rounded to fp16 once,
  bit for bit (slice_f16_exact).  fp16 holds a multiple of 1/8 itself only below 2^8: below that the output is the fp64 sum itself,
  from there on its one rounding.  (This run is for wrong rows, wrong words and lost skips; a second rounding shows on the cancel run.)"""
from collections import namedtuple

import numpy as np

from tests.dense_reference import EPS32, assert_equal_bits, assert_within, f64, worst_ratio  # noqa: F401 (the tests' vocabulary)
from tests.point_reference import FRAC, GUARD_ROWS, SENTINEL, table_rows  # noqa: F401

F16, F32 = np.float16, np.float32
RUNS = ("random", "cancel", "exact")

# include/latticenet_hip.h
LN_OK, LN_ERR_ARG, LN_ERR_UNSUPPORTED = 0, -1, -2
LN_MAX_POS_DIM = 6


def div_up(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------ dispatch
def slice_f16_instance(d, v, values_ptr, out_ptr, n=1):
    """(HV, CH) of the k_slice_forward_f16<d + 1, HV, CH> that ln_slice_forward_f16_impl launches for n > 0 points, or the error code
    it returns, in the order of its checks.  HV: halves per thread (16-byte words when the width and both pointers allow, else 8-byte
    words); CH = 8: the eight-chunks-per-row instance (64 channels in 16-byte words), else 0."""
    if not (n >= 0 and 1 <= d <= LN_MAX_POS_DIM and v >= 4 and v % 4 == 0):
        return LN_ERR_UNSUPPORTED
    if n > 0 and (values_ptr == 0 or out_ptr == 0):
        return LN_ERR_ARG
    if (values_ptr | out_ptr) & 7:
        return LN_ERR_ARG
    wide = v % 8 == 0 and ((values_ptr | out_ptr) & 15) == 0
    return (8, 8 if v == 64 else 0) if wide else (4, 0)


def slice_f16_grid(n, v, hv):
    """(work, workgroups of 256 threads): one thread per (point, word of HV halves)."""
    work = n * (v // hv)
    return work, div_up(work, 256)


# ------------------------------------------------------------------------------------------------------------------ the cases
# off_values / off_out: bytes in front of the array inside a larger allocation; row0: some token names row 0 (else row 0 is all NaN)
Case = namedtuple("Case", "name d v n off_values off_out row0")
ALIGNED = 0x7F0000001000  # a 16-byte-aligned stand-in for a device address (the dispatch reads the low bits only)


def _case(d, v, n, off_values=0, off_out=0, row0=False, tag=""):
    name = f"d{d}-V{v}-n{n}" + (f"-values+{off_values}" if off_values else "") + (f"-out+{off_out}" if off_out else "") + (
        "-row0" if row0 else "") + (f"-{tag}" if tag else "")
    return Case(name, d, v, n, off_values, off_out, row0)


N_INSTANCE = 293  # more than one workgroup at every width below, a last workgroup with idle threads
# (v, off_values, off_out, row0): HV = 4 in one chunk and in three; HV = 8 in one chunk and in nine; HV = 8, CH = 8; the widths that
# would go wide behind a pointer that is 8- but not 16-byte aligned
_WIDTHS = [(4, 0, 0, False), (12, 0, 0, True), (8, 0, 0, False), (72, 0, 0, True), (64, 0, 0, False), (64, 8, 0, False), (16, 0, 8, False)]
INSTANCE_CASES = [_case(d, v, N_INSTANCE, ov, oo, r0) for d in range(1, LN_MAX_POS_DIM + 1) for v, ov, oo, r0 in _WIDTHS] + [
    _case(3, 520, 37, tag="one_wide_row")]
GRID_CASES = [
    _case(3, 4, 1, tag="work1"),                  # n = 1, one thread
    _case(3, 64, 1, tag="work8"),                 # n = 1 in the CH = 8 instance
    _case(3, 12, 85, tag="work255"),
    _case(3, 8, 256, tag="work256"),
    _case(3, 4, 257, tag="work257"),
    _case(2, 64, 32, tag="work256"),
    _case(2, 64, 33, tag="work264"),              # a second workgroup with 8 working threads
    _case(2, 72, 57, row0=True, tag="work513"),   # a third workgroup with one
]
CASES = INSTANCE_CASES + GRID_CASES
CASES_BY_NAME = {c.name: c for c in CASES}
assert len(CASES_BY_NAME) == len(CASES)


def case_instance(case):
    return slice_f16_instance(case.d, case.v, ALIGNED + case.off_values, ALIGNED + case.off_out)


def case_rows(case):
    """Rows of the value table: a few tokens per row, an even number (the cancel run gives the rows alternating signs)."""
    return 2 * div_up(table_rows(case.n), 2)


# ------------------------------------------------------------------------------------------------------------------ inputs
ABSENT_SHARE = 0.05
P_ALL_ABSENT, P_FIRST_ABSENT, P_LAST_ABSENT = 1, 2, 3  # planted points (cases with n >= 4)


def make_tokens(n, m, d, seed, run="random", row0=False):
    """idx [n (d+1)] int32 rows in [0, m) (in [2, m) unless `row0`) with ~5 % of them -1; from n = 4 on point 1 wholly absent, point 2
    with its first vertex alone absent, point 3 with its last alone.  w [n (d+1)] fp32, -1 in the absent slots, else
      random: positive, summing to 1 per point;
      cancel: the same with the odd slots rescaled so that the live odd and even slots sum to the same, and idx of slot r moved to a
              row of parity r % 2 (make_values gives the rows of a parity one sign);
      exact : non-zero multiples of 1/8 in [-1, 1]."""
    rng = np.random.default_rng(seed)
    dp1 = d + 1
    lo = 0 if row0 else 2
    idx = rng.integers(lo, m, (n, dp1)).astype(np.int32)
    spare = rng.integers(lo, m, (n, dp1)).astype(np.int32)
    idx[rng.random((n, dp1)) < ABSENT_SHARE] = -1
    if n >= 4:
        idx[P_ALL_ABSENT] = -1
        for p, r in ((P_FIRST_ABSENT, 0), (P_LAST_ABSENT, d)):
            idx[p] = np.where(idx[p] < 0, spare[p], idx[p])
            idx[p, r] = -1
    if row0 and n >= 4:
        idx[0, 0] = 0
    if run == "cancel":
        moved = (idx & ~1) | (np.arange(dp1, dtype=np.int32)[None, :] & 1)
        idx = np.where(idx >= 0, moved, idx).astype(np.int32)
    live = idx >= 0
    if run == "exact":
        k = rng.integers(1, FRAC + 1, (n, dp1)) * rng.choice([-1, 1], (n, dp1))
        w = (k / FRAC).astype(F32)
    else:
        w = rng.random((n, dp1)) + 0.05
        w = np.where(live, w, 0.0)
        if run == "cancel":
            odd = (np.arange(dp1) & 1).astype(bool)[None, :]
            so, se = (w * odd).sum(1, keepdims=True), (w * ~odd).sum(1, keepdims=True)
            w = np.where(odd & (so > 0) & (se > 0), w * se / np.where(so > 0, so, 1.0), w)
        w = (w / np.maximum(w.sum(1, keepdims=True), 1e-30)).astype(F32)
    w[~live] = -1.0
    return idx.reshape(-1), w.reshape(-1)


def make_values(m, v, seed, run="random", row0=False):
    """fp16 [m, v].  random: N(0, 1).  cancel: +-b[c] (1 + 2^-6 u), sign by the parity of the row, b[c] in [8, 40], u in [-1, 1].
    exact: integers in [-64, 64].  Row 0 is all NaN unless some token names it (`row0`)."""
    rng = np.random.default_rng(seed + 7919)
    if run == "exact":
        x = rng.integers(-64, 65, (m, v)).astype(F16)
    elif run == "cancel":
        b = 8.0 * (1.0 + np.minimum(np.abs(rng.standard_normal(v)), 4.0))
        sign = np.where(np.arange(m) % 2, -1.0, 1.0)[:, None]
        x = (sign * b[None, :] * (1.0 + 2.0 ** -6 * rng.uniform(-1, 1, (m, v)))).astype(F16)
    else:
        x = rng.standard_normal((m, v)).astype(F16)
    if not row0:
        x[0, :] = F16(np.nan)
    return x


def make_inputs(case, run, seed=0):
    """(values fp16 [m, v], idx, w) of one run of a case; the same arrays on every call."""
    m = case_rows(case)
    seed = seed + 1000 * RUNS.index(run) + 31 * case.d + case.v + 7 * case.n
    idx, w = make_tokens(case.n, m, case.d, seed, run, case.row0)
    return make_values(m, case.v, seed, run, case.row0), idx, w


# ------------------------------------------------------------------------------------------------------------------ reference and bound
def slice_f16_ref(values_f16, idx, w, n, d):
    """(ref, mag) in fp64 on the fp16 inputs: ref[p] = sum_r [idx_r >= 0] values[idx_r] w_r, mag[p] the same sum of absolute values.
    Absent slots are never read (a NaN row nobody names stays out)."""
    x = f64(values_f16)
    v = x.shape[1]
    idx2 = np.asarray(idx).reshape(n, d + 1)
    w64 = f64(w).reshape(n, d + 1)
    ref, mag = np.zeros((n, v)), np.zeros((n, v))
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(d + 1):
            ok = idx2[:, r] >= 0
            p = x[idx2[ok, r]] * w64[ok, r][:, None]
            ref[ok] += p
            mag[ok] += np.abs(p)
    return ref, mag


def slice_f16_bound(ref, mag, d):
    """The kernel's path to an element: the fp16 value widened to fp32 (exact), at most d + 1 products and d + 1 adds in fp32 — each
    term of the sum passes through at most one rounding of its product and d + 1 roundings of partial sums no larger than mag, and a
    contracted multiply-add only drops roundings — so the fp32 sum is within e32 = 2 (d + 1) 2^-24 mag of the fp64 sum (twice the
    first-order count: the second-order terms are far inside).  Then one rounding to fp16: half an ulp of a number no larger than
    |ref| + e32, 2^-11 relative, and never less than half the fp16 subnormal spacing, 2^-25.  No constant comes from a GPU run."""
    e32 = 2 * (d + 1) * EPS32 * mag
    return e32 + np.maximum(2.0 ** -11 * (np.abs(ref) + e32), 2.0 ** -25)


def slice_f16_exact(ref, mag, what=""):
    """The output of the exact run: the premise (every sum of absolute terms a multiple of 1/8 below 2^10: fp32 adds it up without a
    rounding in any order) checked from the reference alone, then the fp64 sum rounded to fp16 once."""
    assert float(np.max(mag, initial=0.0)) < 2 ** 10 and bool(np.all(ref * FRAC == np.round(ref * FRAC))), \
        f"{what}: the sums of the exact run are not multiples of 1 / {FRAC} below 2^10"
    return ref.astype(F16)


def _first_worst(got, ref, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(np.isfinite(ref) & (bound > 0), np.abs(f64(got) - ref) / bound, 0.0)
    ratio = np.nan_to_num(ratio, nan=np.inf)
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else ()
    return (tuple(int(j) for j in i), float(ratio[i])) if ratio.size else ((), 0.0)


def assert_slice_f16(got_f16, values_f16, idx, w, n, d, run, what=""):
    """One output [n, v] of the kernel (or of an emulation) against the reference of its inputs: the exact run bit for bit, the other
    runs element by element within slice_f16_bound.  A failure names `what` (case and run), the element and its error / bound ratio.
    Returns the worst ratio (0 for the exact run)."""
    got = np.asarray(got_f16)
    assert got.dtype == F16, got.dtype
    ref, mag = slice_f16_ref(values_f16, idx, w, n, d)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if run == "exact":
        assert_equal_bits(got.astype(F32), slice_f16_exact(ref, mag, what).astype(F32), f"{what} against the fp64 sum rounded to fp16 once")
        return 0.0
    bound = slice_f16_bound(ref, mag, d)
    i, ratio = _first_worst(got, ref, bound)
    assert_within(got, ref, bound, f"{what} (worst error / bound {ratio:.3f} at element {i})")
    return worst_ratio(got, ref, bound)


# ------------------------------------------------------------------------------------------------------------------ emulations
FORMS = ("separate", "contracted")
# (a) accumulation in fp16, (b) weights rounded to fp16 first, (c) the absent-vertex skip removed, (d) the sum rounded to fp16 after
# every vertex, (e) the last word of a row taken from the word before it
FAULTS = ("acc_f16", "w_f16", "no_skip", "round_each", "last_word")


def emulate_slice_f16(values_f16, idx, w, n, d, form="separate", fault=None, hv=4):
    """k_slice_forward_f16 in NumPy fp32: vertices r ascending, absent ones skipped, one rounding to fp16 at the end.
    form "separate": acc = fl(acc + fl(v w)); "contracted": acc = fl(acc + v w), the product (11 x 24 bits) and the sum formed in
    fp64 and rounded to fp32.  `fault`: one of FAULTS, planted for test_slice_f16_reference.py; `hv`: halves per word (for last_word)."""
    x16 = np.asarray(values_f16)
    v = x16.shape[1]
    idx2 = np.asarray(idx).reshape(n, d + 1)
    w2 = np.asarray(w, F32).reshape(n, d + 1)
    if fault == "w_f16":
        w2 = w2.astype(F16).astype(F32)
    acc = np.zeros((n, v), F32)
    with np.errstate(all="ignore"):
        for r in range(d + 1):
            ok = (idx2[:, r] >= 0)[:, None] | (fault == "no_skip")
            x = x16[np.maximum(idx2[:, r], 0)].astype(F32)
            if fault == "last_word" and v >= 2 * hv:
                x[:, v - hv:] = x[:, v - 2 * hv:v - hv]
            wr = w2[:, r:r + 1]
            if fault == "acc_f16":
                new = (acc + (x * wr).astype(F16).astype(F32)).astype(F16).astype(F32)
            elif form == "contracted":
                new = (acc.astype(np.float64) + x.astype(np.float64) * wr.astype(np.float64)).astype(F32)
            else:
                new = acc + x * wr
            if fault == "round_each":
                new = new.astype(F16).astype(F32)
            acc = np.where(ok, new, acc).astype(F32)
        return acc.astype(F16)
