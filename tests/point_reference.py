"""fp64 references and per-element error bounds for the point-side kernels: the fused slice + classifier head (csrc/ln_classify.hip and
the general kernels of csrc/ln_rows.hip behind it), plain slice and gather with their backward scatters.  NumPy / torch on the CPU:
test_point_reference.py checks this module without a GPU, test_gpu_slice_classify.py holds the kernels to it.

Vocabulary of dense_reference.py.  A bound is (number of fp32 roundings on the longest path to the element) * 2^-24 * (sum of the
absolute values of the terms that make up the element); the counting argument stands next to each bound and holds for ANY order of a
sum (a sum of K terms has at most K - 1 adds on a path, whatever the tree: the matrix instructions, the 8-lane DPP sums and the slab
sums all reorder).  Every case has two runs: `random` (within the bounds) and `exact` (values, classifier and incoming gradients small
integers, w and delta_w multiples of 1/8: every product and every partial sum in any order is a multiple of 1/8 far below 2^24 / 8,
so each output is the fp64 result bit for bit, the atomic scatter included).

Tokens come without a hash build: idx = random rows in [0, m) with a share of -1, w barycentric-like with w = -1 in the absent slots
(the convention of slice_no_precomputation)."""
import numpy as np
import torch

from oracle import lattice_oracle as O
from tests.dense_reference import EPS32, assert_equal_bits, assert_within, f32, f64, worst_ratio  # noqa: F401 (the tests' vocabulary)

F32 = np.float32
FRAC = 8  # the exact run's operands are multiples of 1 / FRAC
GUARD_ROWS = 64
SENTINEL = 12345.0

# csrc/ln_classify.hip, csrc/ln_rows.hip, csrc/ln_common.h
WAVE_BWD_GRID = 512      # ln_sc_backward_wave_grid
WAVE_BWD_TILE = 16
GENERAL_BWD_GRID = 512   # ln_sc_backward_grid
GENERAL_FWD_GRID = 2048
LDS_FLOATS = 64 * 1024 // 4
LN_SC_BLOCKS = 3
LN_SC_MAX_ACC = 16
LN_SC_FWD_MAX_CPT = 16


def div_up(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------ dispatch
def _points_per_tile(v, c, arrays_of_v):  # ln_sc_points_per_tile
    for pb in (64, 32, 16, 8):
        if c * (v + 1) + pb * (arrays_of_v * v + c) <= LDS_FLOATS:
            return pb
    return 0


def sc_forward_form(d, v, c, aligned=True):
    """The kernel ln_slice_classify_forward launches: ("wave", CT), ("v4", PB), ("scalar", PB) or None (LN_ERR_UNSUPPORTED).
    `aligned`: the values pointer is 16-byte aligned."""
    if v % 32 == 0 and c <= 32 and d in (2, 3) and aligned and c * v * 4 <= 16 * 1024:
        return ("wave", 4 * min(div_up(c, 4), 8))
    if v % 4 == 0 and aligned:
        for pb in (64, 32, 16):
            if (c + pb) * (v + 1) + 2 * pb * (d + 1) <= LDS_FLOATS and div_up(c, 256 // pb) <= LN_SC_FWD_MAX_CPT:
                return ("v4", pb)
    pb = _points_per_tile(v, c, 1)
    return ("scalar", pb) if pb else None


def sc_backward_form(d, v, c, aligned=True):
    """The kernel ln_slice_classify_backward launches: ("wave", U, CTL), ("v4", PB), ("scalar", PB) or None.  `aligned`: values and
    grad_sliced are both 16-byte aligned."""
    if v % 32 == 0 and v <= 128 and c <= 32 and d in (2, 3) and aligned:
        return ("wave", v // 32, 2 if c > 16 else 1)
    cp = (c + 3) & ~3
    if v % 4 == 0 and cp * v <= 256 * LN_SC_BLOCKS * 16 and aligned:
        for pb in (64, 32, 16, 8):
            if pb * (2 * v + cp + 2 * (d + 1)) + c * v <= LDS_FLOATS:
                return ("v4", pb)
        return None
    if c * v > 256 * LN_SC_MAX_ACC:
        return None
    pb = _points_per_tile(v, c, 2)
    return ("scalar", pb) if pb else None


def sc_backward_grid(n, form):
    if form[0] == "wave":
        return min(div_up(div_up(n, WAVE_BWD_TILE), 4), WAVE_BWD_GRID)
    return min(div_up(n, form[1]), GENERAL_BWD_GRID)


def sc_point_chain(n, form):
    """fp32 adds on the longest path of a sum over the n points of g_lin_w / g_lin_b, in any order inside each stage:
      wave kernels : a wave adds the 16 points of each of its ceil(tiles / (4 grid)) tiles into its accumulator (16 adds per tile,
                     whatever the matrix instruction does inside), the four waves of a workgroup are added through LDS (4);
      general      : a thread adds the PB points of each of its workgroup's ceil(tiles / grid) tiles in one chain;
      ln_k_sum_slabs2 : a thread adds ceil(grid / 16) slabs, 16 threads are folded (16), the result is added to the output (1)."""
    if n == 0:
        return 0
    grid = sc_backward_grid(n, form)
    if form[0] == "wave":
        per_group = WAVE_BWD_TILE * div_up(div_up(n, WAVE_BWD_TILE), 4 * grid) + 4
    else:
        per_group = form[1] * div_up(div_up(n, form[1]), grid)
    return per_group + div_up(grid, 16) + 16 + 1


# ------------------------------------------------------------------------------------------------------------------ inputs
def make_tokens(n, m, d, seed, absent=0.15, exact=False):
    """idx [n (d+1)] int32 random rows with ~`absent` of them -1, every 11th point wholly absent, and one row (m // 2) named by up to
    300 of the tokens; w [n (d+1)] fp32 barycentric-like (positive, summing to 1 per point; multiples of 1/8 in the exact run) with
    w = -1 in the absent slots."""
    rng = np.random.default_rng(seed)
    dp1 = d + 1
    idx = rng.integers(0, m, (n, dp1)).astype(np.int32)
    hot = rng.random((n, dp1)) < min(1.0, 300.0 / max(n * dp1, 1))
    idx[hot] = m // 2
    idx[rng.random((n, dp1)) < absent] = -1
    idx[5::11] = -1
    if exact:
        w = rng.integers(0, FRAC + 1, (n, dp1)).astype(F32) / FRAC
    else:
        w = rng.random((n, dp1)).astype(F32) + F32(0.05)
        w = (w / w.sum(1, keepdims=True)).astype(F32)
    w[idx < 0] = -1.0
    return idx.reshape(-1), w.reshape(-1)


def make_sc_inputs(n, m, d, v, c, seed, exact=False):
    """Operands of one slice-classify case.  random: standard normal, delta_w = 0.1 N(0, 1).  exact: integers in [-2, 2], delta_w in
    {-2 .. 2} / 8.  The four accumulated outputs start from non-zero contents (`*0`): N(0, 1), or integers in [-4, 4]."""
    rng = np.random.default_rng(seed + 1)
    idx, w = make_tokens(n, m, d, seed, exact=exact)
    dp1 = d + 1
    if exact:
        def draw(*shape):
            return rng.integers(-2, 3, shape).astype(F32)

        def old(*shape):
            return rng.integers(-4, 5, shape).astype(F32)
        dw = rng.integers(-2, 3, (n, dp1)).astype(F32) / FRAC
    else:
        def draw(*shape):
            return rng.standard_normal(shape).astype(F32)
        old = draw
        dw = (0.1 * rng.standard_normal((n, dp1))).astype(F32)
    return dict(values=draw(m, v), delta_w=dw, lin_w=draw(c, v), lin_b=draw(c), grad_logits=draw(n, c), idx=idx, w=w,
                g_values0=old(m, v), g_delta_w0=old(n, dp1), g_lin_w0=old(c, v), g_lin_b0=old(c))


# ------------------------------------------------------------------------------------------------------------------ fp64 references
def _scatter64(m, v, rows, contrib):
    """out[rows[k]] += contrib[k] in fp64 (index_add: the contributions of a row in one pass, no Python loop over tokens)."""
    out = torch.zeros((m, v), dtype=torch.float64)
    out.index_add_(0, torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)), torch.from_numpy(np.ascontiguousarray(contrib)))
    return out.numpy()


def token_counts(idx, m):
    idx = np.asarray(idx).reshape(-1)
    return np.bincount(idx[idx >= 0], minlength=m).astype(np.float64)


def w_effective(w, delta_w):
    """fp32(w + delta_w), every slot (the absent ones too): what the kernels form first and publish as w_eff."""
    return (f32(w).reshape(-1) + f32(delta_w).reshape(-1)).astype(F32)


def sc_forward_reference(inp, n):
    """The logits of the ordered fp32 evaluation (rows r ascending, channels v ascending, product and sum rounded apart): the kernels
    are bit-identical to it in every form."""
    c, v = inp["lin_w"].shape
    if n == 0:
        return np.zeros((0, c), F32)
    return ordered_slice_classify(inp["values"], inp["delta_w"], inp["lin_w"], inp["lin_b"], inp["idx"], inp["w"], n)


def ordered_slice_classify(values, delta_w, lin_w, lin_b, idx, w, n):
    """oracle.lattice_oracle.slice_classify with the loop over classes vectorised: the same fp32 operations on every element in the
    same order (test_point_reference.py holds the two together bit for bit), V instead of C V passes over the points."""
    v = values.shape[1]
    idx2 = np.asarray(idx).reshape(n, -1)
    weff = w_effective(w, delta_w).reshape(n, -1)
    h = np.zeros((n, v), F32)
    for r in range(idx2.shape[1]):
        ok = idx2[:, r] >= 0
        h[ok] = h[ok] + values[idx2[ok, r]] * weff[ok, r][:, None]
    acc = np.zeros((n, lin_w.shape[0]), F32)
    for vi in range(v):
        acc = acc + lin_w[None, :, vi] * h[:, vi:vi + 1]
    return acc + lin_b[None, :]


def sc_backward_reference(inp, n, d, form):
    """fp64 results of ln_slice_classify_backward with g_values scattered by the entry point, the magnitudes (sums of absolute terms)
    and the bounds, as three dicts over g_values, g_delta_w, g_lin_w, g_lin_b, grad_sliced, w_eff.  Absent vertices are skipped;
    w_eff = fp32(w + delta_w) is formed first and taken as an exact number from there on.  `form`: sc_backward_form(...)."""
    values, lin_w, g = f64(inp["values"]), f64(inp["lin_w"]), f64(inp["grad_logits"])
    m, v = values.shape
    c = lin_w.shape[0]
    dp1 = d + 1
    idx = np.asarray(inp["idx"]).reshape(n, dp1)
    weff32 = w_effective(inp["w"], inp["delta_w"])
    weff = f64(weff32).reshape(n, dp1)
    gs, gs_abs = g @ lin_w, np.abs(g) @ np.abs(lin_w)
    h, h_abs = np.zeros((n, v)), np.zeros((n, v))
    gdw, gdw_abs = np.zeros((n, dp1)), np.zeros((n, dp1))
    gv, gv_abs = np.zeros((m, v)), np.zeros((m, v))
    for r in range(dp1):
        ok = idx[:, r] >= 0
        x = values[idx[ok, r]]
        wr = weff[ok, r][:, None]
        h[ok] += x * wr
        h_abs[ok] += np.abs(x * wr)
        gdw[ok, r] = np.einsum("pv,pv->p", x, gs[ok])
        gdw_abs[ok, r] = np.einsum("pv,pv->p", np.abs(x), gs_abs[ok])
        gv += _scatter64(m, v, idx[ok, r], gs[ok] * wr)
        gv_abs += _scatter64(m, v, idx[ok, r], gs_abs[ok] * np.abs(wr))
    old = {k: f64(inp[k + "0"]) for k in ("g_values", "g_delta_w", "g_lin_w", "g_lin_b")}
    ref = dict(g_values=old["g_values"] + gv, g_delta_w=old["g_delta_w"] + gdw, g_lin_w=old["g_lin_w"] + g.T @ h,
               g_lin_b=old["g_lin_b"] + g.sum(0), grad_sliced=gs, w_eff=f64(weff32))
    mag = dict(g_values=np.abs(old["g_values"]) + gv_abs, g_delta_w=np.abs(old["g_delta_w"]) + gdw_abs,
               g_lin_w=np.abs(old["g_lin_w"]) + np.abs(g).T @ h_abs, g_lin_b=np.abs(old["g_lin_b"]) + np.abs(g).sum(0),
               grad_sliced=gs_abs, w_eff=np.abs(f64(weff32)))
    chain = sc_point_chain(n, form)
    cnt = token_counts(idx, m)[:, None]
    bound = dict(
        # gs[p, v] = sum_c g W: each product rounded once (an fmaf: not at all), at most C - 1 adds on a path (zero padding adds nothing)
        grad_sliced=c * EPS32 * mag["grad_sliced"],
        # one fp32 add, the reference forms the same fp32 number: bit for bit
        w_eff=0.0 * mag["w_eff"],
        # values[row] . gs: the C roundings inside gs, the product (1), at most V - 1 adds of the dot, the add onto the old value (1)
        g_delta_w=(c + 1 + (v - 1) + 1) * EPS32 * mag["g_delta_w"],
        # h = sum_r values * w_eff: product and at most d adds (d + 1); g * h (1); the sum over points and slabs onto the old value
        g_lin_w=(dp1 + 1 + chain) * EPS32 * mag["g_lin_w"],
        # the matrix instruction multiplies by 1.0 (exact), the general kernels add g itself: the sum over points and slabs only
        g_lin_b=max(chain, 1) * EPS32 * mag["g_lin_b"],
        # gs (C), the product with w_eff (1), one atomic add per token of the row, the first of them onto the old value
        g_values=(c + 1 + cnt) * EPS32 * mag["g_values"])
    return ref, mag, bound


def assert_exact_representable(mag, what=""):
    """The premise of the exact run, from the reference alone: the largest sum of absolute terms of any output, in units of 1 / FRAC,
    is below 2^24, so no partial sum in any order needs a 25th bit."""
    for k, a in mag.items():
        top = float(np.max(a)) * FRAC if np.size(a) else 0.0
        assert top < 2 ** 24, f"{what} {k}: sum of absolute terms {top / FRAC} * {FRAC} is not below 2^24; shrink the integer ranges"


def assert_sc_backward(got, ref, bound, exact, what=""):
    """got / ref / bound: dicts over the six outputs.  Returns the worst error / bound ratio per output (reported, never asserted)."""
    ratios = {}
    for k in ("g_values", "g_delta_w", "g_lin_w", "g_lin_b", "grad_sliced", "w_eff"):
        g_ = f64(got[k]).reshape(ref[k].shape)
        if exact or k == "w_eff":
            bad = g_ != ref[k]
            if bad.any():
                i = tuple(int(j) for j in np.argwhere(bad)[0])
                raise AssertionError(f"{what} {k}: {int(bad.sum())} elements differ from the fp64 result, first {i}: got {g_[i]!r}, "
                                     f"fp64 {ref[k][i]!r}")
            ratios[k] = 0.0
        else:
            assert_within(g_, ref[k], bound[k], f"{what} {k}")
            ratios[k] = worst_ratio(g_, ref[k], bound[k])
    return ratios


def assert_sc_parameter_gradients(g_delta_w, g_lin_w, g_lin_b, grad_logits, values, delta_w, lin_w, idx, w, d, what=""):
    """g_delta_w, g_lin_w and g_lin_b of one backward call from zeroed contents, element by element within the counted bounds of the
    kernel form the shape takes (for the tests that reach the kernels through the Lattice / autograd layers).  Returns the ratios."""
    values, lin_w, g = f32(values), f32(lin_w), f32(grad_logits)
    n, c = g.shape
    m, v = values.shape
    idx = np.asarray(idx.detach().cpu() if hasattr(idx, "detach") else idx).reshape(-1)
    inp = dict(values=values, delta_w=f32(delta_w).reshape(n, d + 1), lin_w=lin_w, grad_logits=g, idx=idx, w=f32(w).reshape(-1),
               g_values0=np.zeros((m, v), F32), g_delta_w0=np.zeros((n, d + 1), F32), g_lin_w0=np.zeros((c, v), F32), g_lin_b0=np.zeros(c, F32))
    ref, _, bound = sc_backward_reference(inp, n, d, sc_backward_form(d, v, c))
    ratios = {}
    for k, got in (("g_delta_w", g_delta_w), ("g_lin_w", g_lin_w), ("g_lin_b", g_lin_b)):
        assert_within(f64(got).reshape(ref[k].shape), ref[k], bound[k], f"{what} {k}")
        ratios[k] = worst_ratio(f64(got).reshape(ref[k].shape), ref[k], bound[k])
    return ratios


# ------------------------------------------------------------------------------------------------------------------ fp32 evaluations
def torch_fp32_sc_backward(inp, n, d):
    """A plain fp32 evaluation with torch on the CPU (matmul, index_add): an independent implementation the bounds must admit."""
    t = {k: torch.from_numpy(np.ascontiguousarray(a)) for k, a in inp.items()}
    dp1 = d + 1
    idx = t["idx"].reshape(n, dp1).long()
    ok = idx >= 0
    weff = (t["w"].reshape(n, dp1) + t["delta_w"])
    x = t["values"][idx.clamp(min=0)] * ok[:, :, None]           # [n, d+1, V]
    h = (x * weff[:, :, None]).sum(1)
    g = t["grad_logits"]
    gs = g @ t["lin_w"]
    gv = t["g_values0"].clone()
    gv.index_add_(0, idx[ok], (gs[:, None, :] * weff[:, :, None])[ok])
    return dict(g_values=gv.numpy(), g_delta_w=(t["g_delta_w0"] + (x * gs[:, None, :]).sum(2) * ok).numpy(),
                g_lin_w=(t["g_lin_w0"] + g.t() @ h).numpy(), g_lin_b=(t["g_lin_b0"] + g.sum(0)).numpy(), grad_sliced=gs.numpy(),
                w_eff=weff.reshape(-1).numpy())


FAULTS = ("drop_last_tile", "tile_twice", "absent_row0", "gdw_overwrite", "w_not_weff", "swap_classes", "chunk1_from_chunk0")


def emulate_sc_backward_wave(inp, n, d, fault=None):
    """k_slice_classify_backward_wave + ln_k_sum_slabs2 + k_sc_scatter_atomic in NumPy fp32, stage by stage in the kernels' order:
    h in 32-channel chunks (r ascending), gh = g @ W one class after the other, the g_delta_w dot as four-channel partial sums per
    lane, U of them per lane, then three butterfly steps over the 8 lanes, the classifier gradients per wave over its tiles
    (tile = 16 points, wave w of workgroup b owns tiles 4 b + w + k * 4 grid), the four waves added in order, the slabs added by
    16 threads of ceil(grid / 16) slabs each and folded in order, everything accumulated onto the old contents.
    `fault`: one of FAULTS, planted for test_point_reference.py."""
    values, lin_w, g = f32(inp["values"]), f32(inp["lin_w"]), f32(inp["grad_logits"])
    m, v = values.shape
    c = lin_w.shape[0]
    dp1, u = d + 1, v // 32
    idx = np.asarray(inp["idx"]).reshape(n, dp1)
    weff = w_effective(inp["w"], inp["delta_w"]).reshape(n, dp1)
    ok = idx >= 0
    gs = np.zeros((n, v), F32)
    for ci in range(c):
        gs = gs + g[:, ci:ci + 1] * lin_w[ci][None, :]
    h = np.zeros((n, v), F32)
    gdw = np.zeros((n, dp1), F32)
    for r in range(dp1):
        x = values[np.where(ok[:, r], idx[:, r], 0)]
        if fault != "absent_row0":
            x = np.where(ok[:, r:r + 1], x, F32(0))
        h = h + x * weff[:, r:r + 1]
        p = (x * gs).reshape(n, u, 8, 4)
        lane = np.zeros((n, 8), F32)
        for k in range(u):
            lane = lane + (((p[:, k, :, 0] + p[:, k, :, 1]) + p[:, k, :, 2]) + p[:, k, :, 3])
        lane = lane + lane[:, [1, 0, 3, 2, 5, 4, 7, 6]]
        lane = lane + lane[:, [2, 3, 0, 1, 6, 7, 4, 5]]
        lane = lane + lane[:, ::-1]
        gdw[:, r] = np.where(ok[:, r], lane[:, r % 8], F32(0))
    if fault == "chunk1_from_chunk0":
        h[:, 32:64] = h[:, 0:32]
    g_delta_w = gdw if fault == "gdw_overwrite" else f32(inp["g_delta_w0"]) + gdw
    # classifier gradients: [h | 1] per wave
    tiles = div_up(n, 16)
    grid = sc_backward_grid(n, ("wave", u, 1)) if n else 0
    nw = 4 * grid
    steps = div_up(tiles, nw) if n else 0
    ga = g.copy()
    if fault == "swap_classes":
        ga[:, [1, 2]] = ga[:, [2, 1]]
    h1 = np.concatenate([h, np.ones((n, 1), F32)], 1)
    pad = steps * nw * 16 - n
    gp = np.concatenate([ga, np.zeros((pad, c), F32)])
    hp = np.concatenate([h1, np.zeros((pad, v + 1), F32)])
    if fault == "drop_last_tile":
        gp[(tiles - 1) * 16:] = 0
    gp, hp = gp.reshape(steps, nw, 16, c), hp.reshape(steps, nw, 16, v + 1)
    acc = np.zeros((nw, c, v + 1), F32)
    for k in range(steps):
        for j in range(0, 16, 4):  # one matrix instruction: four points' products summed, then added to the accumulator
            acc = acc + np.einsum("wjc,wjv->wcv", gp[k, :, j:j + 4], hp[k, :, j:j + 4])
        if fault == "tile_twice" and k == 0:
            acc[1] = acc[1] + np.einsum("jc,jv->cv", gp[0, 1], hp[0, 1]).astype(F32)
    acc = acc.reshape(grid, 4, c, v + 1)
    slabs = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3] if grid else acc.sum(1)
    part = np.zeros((16, c, v + 1), F32)
    for s in range(grid):
        part[s % 16] = part[s % 16] + slabs[s]
    tot = np.zeros((c, v + 1), F32)
    for k in range(16):
        tot = tot + part[k]
    wt = f32(inp["w"]).reshape(n, dp1) if fault == "w_not_weff" else weff
    gv = f32(inp["g_values0"]).copy()
    for r in range(dp1):
        np.add.at(gv, idx[ok[:, r], r], (gs * wt[:, r:r + 1])[ok[:, r]])
    return dict(g_values=gv, g_delta_w=g_delta_w, g_lin_w=f32(inp["g_lin_w0"]) + tot[:, :v], g_lin_b=f32(inp["g_lin_b0"]) + tot[:, v],
                grad_sliced=gs, w_eff=weff.reshape(-1))


# ------------------------------------------------------------------------------------------------------------------ slice / gather
def slice_forward_reference(values, idx, w, n):
    """Ordered fp32 form (r ascending, absent rows skipped): k_slice_forward is bit-identical to it."""
    v = values.shape[1]
    return O.slice_with_precomputation(values, idx, w, n) if n else np.zeros((0, v), F32)


def gather_forward_reference(values, idx, w, n):
    dp1 = (idx.shape[0] // n) if n else 1
    v = values.shape[1]
    return O.gather_with_precomputation(values, idx, w, n) if n else np.zeros((0, dp1 * (v + 1)), F32)


def scatter_backward_reference(grad, idx, w, dp1, old):
    """grad_values[idx[p, r]] += grad[p, r] * w[p, r] in fp64 onto `old`, for grad [n, d+1, V] (gather backward) or [n, 1, V]
    (slice backward: the same row for every r).  Returns (ref, bound): one product (1) and one atomic add per token of the row, the
    first of them onto the old contents."""
    old = f64(old)
    m, v = old.shape
    grad = f64(grad)
    n = grad.shape[0]
    idx = np.asarray(idx).reshape(n, dp1)
    w = f64(w).reshape(n, dp1)
    out, mag = old.copy(), np.abs(old)
    for r in range(dp1):
        ok = idx[:, r] >= 0
        contrib = grad[ok, r if grad.shape[1] > 1 else 0] * w[ok, r][:, None]
        out += _scatter64(m, v, idx[ok, r], contrib)
        mag += _scatter64(m, v, idx[ok, r], np.abs(contrib))
    return out, (1 + token_counts(idx, m)[:, None]) * EPS32 * mag, mag


# ------------------------------------------------------------------------------------------------------------------ the cases
# shared by test_point_reference.py (CPU: the emulation and torch fp32 inside the bounds) and test_gpu_slice_classify.py (the kernels)
N_WAVE_LARGE = 2 * 32768 + 16 * 5 + 7   # beyond the 512-workgroup cap: waves walk three or two tiles, the last tile is ragged
N_WAVE_SMALL = 16 * 4 + 5               # five tiles: three of the four waves of the second workgroup have none
N_FWD_WAVE = 64 * 4 * 2 + 37
WAVE_BWD_CASES = [(d, v, c) for d in (2, 3) for v in (32, 64, 96, 128) for c in (13, 21)]
WAVE_FWD_CASES = [(d, v, c) for d in (2, 3) for v, c in ((32, 3), (96, 8), (32, 9), (96, 16), (32, 20), (96, 24), (32, 27), (96, 32))]


def table_rows(n):
    """Rows of the value table of a case with n points: a few tokens per row, a few thousand rows at the most."""
    return int(min(4096, max(16, n // 3)))
