"""Weight normalisation (ln_weight_norm_forward / _backward, csrc/ln_glue.hip) and the fused mean NLL loss of one cloud (ln_nll_forward /
_backward, the one-cloud entry of csrc/ln_nll.hip) against fp64, element by element (`pytest -m gpu`).

References, bounds and their counting arguments live in tests/glue_reference.py (checked on the CPU by test_glue_reference.py, which
also runs an fp32 emulation of the kernels' summation order through the same bounds).  Every raw call writes into buffers that sit
inside larger allocations filled with a sentinel; the sentinels before and behind each output are compared bit for bit after every
call.  Each family prints its worst error / bound ratios (`pytest -s`); nothing is asserted on them beyond the bounds themselves.

Not held: ||v|| outside 2^-20 .. 2^20 times the drawn scale (n^3 leaves the normal fp32 range around 2^+-42), more than 2^24 live
labels (the fp32 count stops being exact) and n * classes >= 2^31 (more than 8 GB of log-probabilities)."""
import hashlib

import numpy as np
import pytest
import torch

from tests import glue_reference as G
from tests.dense_reference import assert_equal_bits, assert_within, f32, f64

pytestmark = pytest.mark.gpu

GUARD = 64  # sentinel floats before and behind every output (256 bytes: the output keeps the allocation's 16-byte alignment)
SENTINEL = -777.25
NAN_BITS = 0x7FC00ABC  # what the NLL gradient buffer holds before the backward writes it


def dev():
    return torch.device("cuda", 0)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def lib_and_stream():
    from lattice_net_amd import _lib
    return _lib.load(), _lib.stream_ptr(dev())


def merge(worst, ratios):
    for k, r in ratios.items():
        worst[k] = max(r, worst.get(k, 0.0))


class Guarded:
    """`numel` floats inside a larger allocation of sentinels, `offset` floats (4 bytes each) off 16-byte alignment."""

    def __init__(self, numel, offset=0, prefill_bits=None):
        self.numel, self.lo = numel, GUARD + offset
        self.whole = torch.full((self.lo + numel + GUARD,), SENTINEL, dtype=torch.float32, device=dev())
        self.part = self.whole[self.lo:self.lo + numel]
        self.ptr = self.whole.data_ptr() + 4 * self.lo
        assert self.ptr % 16 == 4 * (offset % 4)
        if prefill_bits is not None:
            self.part.view(torch.int32).fill_(prefill_bits)
        self.sentinel_bits = int(torch.tensor([SENTINEL], dtype=torch.float32).view(torch.int32))

    def guards_intact(self, what=""):
        bits = self.whole.view(torch.int32)
        assert bool((bits[:self.lo] == self.sentinel_bits).all()), f"{what}: the sentinels before the output were overwritten"
        assert bool((bits[self.lo + self.numel:] == self.sentinel_bits).all()), f"{what}: the sentinels behind the output were overwritten"

    def untouched(self, what="", bits=None):
        self.guards_intact(what)
        want = self.sentinel_bits if bits is None else bits
        assert bool((self.part.view(torch.int32) == want).all()), f"{what}: a refused call wrote its output"

    def numpy(self, shape=None):
        a = self.part.cpu().numpy()
        return a if shape is None else a.reshape(shape)


# ================================================================================================================== weight norm
def wn_buffers(rows, cols, g_dim, offset=0):
    J, _ = G.wn_jk(rows, cols, g_dim)
    return {"w": Guarded(rows * cols, offset), "norm": Guarded(1, offset), "grad_v": Guarded(rows * cols, offset), "grad_g": Guarded(J, offset)}


def wn_call(dv, dg, dgw, rows, cols, g_dim, bufs, backward=True):
    """The two raw calls on device tensors (None: a null pointer); returns the two return codes (the second None without backward)."""
    lib, stream = lib_and_stream()
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    o = {k: (None if b is None else b.ptr) for k, b in bufs.items()}
    rc_f = lib.ln_weight_norm_forward(p(dv), p(dg), rows, cols, g_dim, o["w"], o["norm"], stream)
    rc_b = lib.ln_weight_norm_backward(p(dv), p(dg), p(dgw), o["norm"], rows, cols, g_dim, o["grad_v"], o["grad_g"], stream) if backward else None
    torch.cuda.synchronize()
    return rc_f, rc_b


def wn_run(v, g, g_dim, gw, offset=0, what=""):
    """Forward + backward through the C ABI: (w, norm, grad_v, grad_g) as NumPy arrays, sentinels checked."""
    rows, cols = v.shape
    bufs = wn_buffers(rows, cols, g_dim, offset)
    assert wn_call(gpu(v), gpu(g), gpu(gw), rows, cols, g_dim, bufs) == (0, 0), what
    for name, b in bufs.items():
        b.guards_intact(f"{what} {name}")
    return bufs["w"].numpy((rows, cols)), bufs["norm"].numpy()[0], bufs["grad_v"].numpy((rows, cols)), bufs["grad_g"].numpy()


def same_bits(a, b, what):
    for name, x, y in zip(("w", "norm", "grad_v", "grad_g"), a, b):
        assert_equal_bits(np.asarray(x), np.asarray(y), f"{what} {name}")


def check_wn_random(rows, cols, g_dim, worst, scales=(1.0, 2.0 ** -20, 2.0 ** 20)):
    """One shape: the random run at every scale within its bounds; the scaled runs bit for bit the unscaled one (a power of two
    scales every operator on the path exactly); a second run at outputs 4 bytes off 16-byte alignment bit for bit the first."""
    base = None
    for scale in scales:
        what = f"{rows}x{cols} g_dim={g_dim} scale={scale}"
        v, g, gw = G.wn_random_case(rows, cols, g_dim, rows * 7 + cols + g_dim, scale)
        out = wn_run(v, g, g_dim, gw, what=what)
        merge(worst, G.assert_weight_norm(out, v, g, g_dim, gw, what))
        if base is None:
            base = out
            same_bits(wn_run(v, g, g_dim, gw, offset=1, what=what + " misaligned"), out, what + " misaligned")
        else:
            s = np.float32(scale)
            same_bits((out[0], out[1], out[2] * s, out[3]), (base[0], base[1] * s, base[2], base[3]), what + " against scale 1")


def check_wn_exact(rows, cols, g_dim):
    case = G.wn_exact_case(rows, cols, g_dim)
    if case is None:
        return 0
    v, g, gw, ref = case
    out = wn_run(v, g, g_dim, gw, what=f"exact {rows}x{cols} g_dim={g_dim}")
    for name, o, r in zip(("w", "norm", "grad_v", "grad_g"), out, ref):
        assert_within(np.asarray(f64(o)).reshape(np.shape(r)), r, 0.0, f"exact {rows}x{cols} g_dim={g_dim} {name}")
    return 1


def jk_shapes(J, g_dim):
    return [(J, K, 0) if g_dim == 0 else (K, J, 1) for K in G.wn_k_values(J)]


@pytest.mark.parametrize("g_dim", [0, 1])
@pytest.mark.parametrize("J", G.WN_J)
def test_weight_norm_random(J, g_dim):
    """J magnitudes (1, 2, around the wave and workgroup boundaries, 1000, the limit 1024) x K in {1, 2, lanes - 1, lanes, lanes + 1,
    3 lanes + 1}: w, norm, grad_v, grad_g within their bounds, with gw drawn so that the two terms of grad_v cancel; the same with v
    scaled by 2^-20 and 2^20.  K = 1 is (rows, 1) with g_dim 0 and (1, cols) with g_dim 1."""
    worst = {}
    for rows, cols, gd in jk_shapes(J, g_dim):
        check_wn_random(rows, cols, gd, worst)
    print(f"weight norm random J={J} g_dim={g_dim}: worst error / bound {worst}")


@pytest.mark.parametrize("g_dim", [0, 1])
@pytest.mark.parametrize("J", G.WN_J)
def test_weight_norm_exact(J, g_dim):
    """v in {0, +-1} with 4^k non-zeros (n = 2^k), g powers of two, gw small integers: every output bit for bit."""
    shapes = jk_shapes(J, g_dim)
    assert sum(check_wn_exact(*s) for s in shapes) == len(shapes)  # (test_glue_reference.py: no case is dropped)


@pytest.mark.parametrize("g_dim", [0, 1])
def test_weight_norm_element_count_edges(g_dim):
    """1023, 1024 and 1025 elements: the last thread without an element, every thread with one, the first thread with two."""
    worst = {}
    for rows, cols in G.WN_ELEMENT_EDGE_SHAPES:
        check_wn_random(rows, cols, g_dim, worst)
        assert check_wn_exact(rows, cols, g_dim) == 1
    print(f"weight norm 1023 / 1024 / 1025 elements g_dim={g_dim}: worst error / bound {worst}")


def test_weight_norm_largest_parameter():
    """Exactly 2^24 elements, 16384 x 1024 with one magnitude per column: J = 1024, one lane per magnitude, 16384 elements per thread
    in the sum of squares."""
    rows, cols, g_dim = G.WN_LARGEST
    worst = {}
    check_wn_random(rows, cols, g_dim, worst, scales=(1.0,))
    assert check_wn_exact(rows, cols, g_dim) == 1
    print(f"weight norm 16384x1024 g_dim=1: worst error / bound {worst}")


@pytest.mark.parametrize("rows,cols,g_dim", [(5, 7, 0), (5, 7, 1), (1, 1, 0), (64, 17, 1)])
def test_weight_norm_of_a_zero_direction(rows, cols, g_dim):
    """v = 0: n = 0 exactly, and NaN exactly where the fp64 chain v * (g / n) and its gradients have NaN."""
    J, _ = G.wn_jk(rows, cols, g_dim)
    v = np.zeros((rows, cols), np.float32)
    g = np.linspace(0.0, 2.0, J).astype(np.float32)  # (a zero magnitude among them: 0 / 0)
    gw = np.arange(rows * cols, dtype=np.float32).reshape(rows, cols) - 3
    out = wn_run(v, g, g_dim, gw, what="v = 0")
    assert_equal_bits(np.asarray(out[1]), np.float32(0.0), "norm")
    G.assert_weight_norm(out, v, g, g_dim, gw, "v = 0")
    ref, _ = G.weight_norm_reference(v, g, g_dim, gw)
    assert np.isnan(ref[0]).all() and np.isnan(ref[2]).all() and np.isnan(ref[3]).all()  # (what the line above compared with)


def test_weight_norm_two_runs_are_bitwise_equal():
    for rows, cols, g_dim in ((1000, 3, 0), (3, 1000, 1), (513, 5, 0), (297, 32, 1)):
        v, g, gw = G.wn_random_case(rows, cols, g_dim, 11)
        same_bits(wn_run(v, g, g_dim, gw), wn_run(v, g, g_dim, gw), f"{rows}x{cols} g_dim={g_dim} second run")


def test_weight_norm_refusals_write_nothing_and_the_next_call_is_right():
    """More than 1024 magnitudes and more than 2^24 elements are LN_ERR_UNSUPPORTED, g_dim 2 and a null pointer LN_ERR_ARG; nothing
    is launched: every output and sentinel keeps its bits.  (The buffers have the full size of the refused shape.)"""
    cases = [((1025, 1, 0), G.LN_ERR_UNSUPPORTED, None), ((1, 1025, 1), G.LN_ERR_UNSUPPORTED, None),
             ((16385, 1024, 1), G.LN_ERR_UNSUPPORTED, None), ((8, 8, 2), G.LN_ERR_ARG, None), ((0, 8, 0), G.LN_ERR_ARG, None)]
    cases += [((8, 8, 0), G.LN_ERR_ARG, null) for null in ("v", "g", "gw", "w", "norm", "grad_v", "grad_g")]
    for (rows, cols, g_dim), code, null in cases:
        numel = max(rows * cols, 1)
        dv, dgw = torch.ones((numel,), device=dev()), torch.ones((numel,), device=dev())
        dg = torch.ones((max(rows, cols),), device=dev())
        bufs = {"w": Guarded(numel), "norm": Guarded(1), "grad_v": Guarded(numel), "grad_g": Guarded(max(rows, cols))}
        ins = {"v": dv, "g": dg, "gw": dgw}
        passed = dict(bufs)
        if null in ins:
            ins[null] = None
        elif null is not None:
            passed[null] = None
        # (a null w concerns the forward alone, and no forward has written the norm a backward would read: the backward is not called)
        rc_f, rc_b = wn_call(ins["v"], ins["g"], ins["gw"], rows, cols, g_dim, passed, backward=null != "w")
        what = f"{rows}x{cols} g_dim={g_dim} null={null}"
        if null in ("gw", "grad_v", "grad_g"):  # (arguments of the backward call only: the forward is valid and runs)
            assert (rc_f, rc_b) == (0, code), (what, rc_f, rc_b)
            for name in ("grad_v", "grad_g"):
                bufs[name].untouched(f"{what} {name}")
        elif null == "w":
            assert (rc_f, rc_b) == (code, None), (what, rc_f, rc_b)
            for name, b in bufs.items():
                b.untouched(f"{what} {name}")
        else:
            assert (rc_f, rc_b) == (code, code), (what, rc_f, rc_b)
            for name, b in bufs.items():
                b.untouched(f"{what} {name}")
        # the next valid call
        v, g, gw = G.wn_random_case(65, 9, 1, 4)
        G.assert_weight_norm(wn_run(v, g, 1, gw, what="after " + what), v, g, 1, gw, "after " + what)


@pytest.mark.parametrize("rows,cols,g_dim", [(65, 9, 0), (9, 65, 1), (1024, 2, 0), (1, 9, 1)])
def test_weight_norm_function_is_held_to_the_same_bounds(rows, cols, g_dim):
    """The autograd wrapper (g shaped [rows, 1] / [1, cols] as the layers keep it): outputs and both gradients within the bounds, bit
    for bit what the raw calls give."""
    from lattice_net_amd.lattice_modules import WeightNormFunction
    v_np, g_np, gw_np = G.wn_random_case(rows, cols, g_dim, 21)
    v = gpu(v_np).requires_grad_(True)
    g = gpu(g_np).reshape((rows, 1) if g_dim == 0 else (1, cols)).requires_grad_(True)
    w = WeightNormFunction.apply(v, g, g_dim)
    w.backward(gpu(gw_np))
    assert g.grad.shape == g.shape and v.grad.shape == v.shape
    raw = wn_run(v_np, g_np, g_dim, gw_np)
    got = (f32(w), raw[1], f32(v.grad), f32(g.grad).reshape(-1))
    same_bits(got, raw, "wrapper against the raw calls")
    print(f"WeightNormFunction {rows}x{cols} g_dim={g_dim}: worst error / bound {G.assert_weight_norm(got, v_np, g_np, g_dim, gw_np, 'wrapper')}")


# ================================================================================================================== NLL
def nll_call(d_lp, d_target, n, classes, ignore, d_grad_loss, loss_count, grad, ws, ws_bytes):
    lib, stream = lib_and_stream()
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    ig = G.NO_LABEL if ignore is None else int(ignore)
    rc_f = lib.ln_nll_forward(p(d_lp), p(d_target), n, classes, ig, p(ws), ws_bytes, None if loss_count is None else loss_count.ptr, stream)
    rc_b = lib.ln_nll_backward(p(d_target), p(d_grad_loss), None if loss_count is None else loss_count.ptr, n, classes, ig,
                               None if grad is None else grad.ptr, stream)
    torch.cuda.synchronize()
    return rc_f, rc_b


def dirty_workspace():
    """The partial sums of a previous call must not matter: the workspace arrives full of 1e30."""
    lib, _ = lib_and_stream()
    nbytes = int(lib.ln_nll_workspace_bytes())
    assert nbytes == G.LN_NLL_BLOCKS * 2 * 4
    return torch.full((nbytes // 4,), 1e30, dtype=torch.float32, device=dev()), nbytes


def nll_run(lp, target, ignore, grad_loss, offset=0, what=""):
    """Forward + backward through the C ABI, the gradient buffer pre-filled with a NaN pattern: (loss_count [2], grad [n, C])."""
    n, classes = lp.shape
    loss_count, grad = Guarded(2, offset), Guarded(n * classes, offset, prefill_bits=NAN_BITS)
    ws, ws_bytes = dirty_workspace()
    d_lp, d_target = (gpu(lp), gpu(target)) if n else (None, None)
    rcs = nll_call(d_lp, d_target, n, classes, ignore, gpu(np.array([grad_loss], np.float32)), loss_count, grad, ws, ws_bytes)
    assert rcs == (0, 0), (what, rcs)
    loss_count.guards_intact(f"{what} loss_count")
    grad.guards_intact(f"{what} grad_log_probs")
    return loss_count.numpy(), grad.numpy((n, classes))


def nll_shapes(n):
    return [(n, c) for c in G.NLL_CLASSES_SMALL] if n in G.NLL_N_SMALL else [(n, (2, 5, 2)[G.NLL_N_LARGE.index(n)])]


@pytest.mark.parametrize("n", G.NLL_N_SMALL + G.NLL_N_LARGE)
def test_nll_random(n):
    """Every n (one thread, around one workgroup, around one workgroup's four elements per thread, exactly 512 workgroups, the cap
    with a further trip of the grid-stride loop, a ragged tail) x classes x ignore_index (none, in range, -100 with -100 labels,
    >= C) with labels -1, C and C + 7 among the live ones: loss within its bound, the count exact, the gradient — written over a NaN
    pattern — the rounded quotient at the clamped target of each live row and +-0 everywhere else."""
    worst = 0.0
    for n_, classes in nll_shapes(n):
        for ignore in G.nll_ignore_modes(classes):
            what = f"n={n} C={classes} ignore={ignore}"
            lp, target = G.nll_random_case(n, classes, ignore, n + classes)
            loss_count, grad = nll_run(lp, target, ignore, 3.0, what=what)
            worst = max(worst, G.assert_nll(loss_count, grad, lp, target, ignore, 3.0, what))
    print(f"NLL random n={n}: worst error / bound of the loss {worst}")


@pytest.mark.parametrize("n", G.NLL_N_SMALL + G.NLL_N_LARGE)
def test_nll_exact(n):
    """Integer log-probabilities, a power of two of live labels (the rest -100): loss, count and gradient bit for bit."""
    for n_, classes in nll_shapes(n):
        case = G.nll_exact_case(n, classes)
        assert case is not None  # (test_glue_reference.py: no case is dropped)
        lp, target, grad_loss, (loss, count, grad_ref, _) = case
        loss_count, grad = nll_run(lp, target, -100, grad_loss, what=f"exact n={n} C={classes}")
        assert_within(loss_count, np.array([loss, count]), 0.0, f"exact n={n} C={classes} loss_count")
        assert_within(grad, grad_ref, 0.0, f"exact n={n} C={classes} grad")


def test_nll_reproduces_the_recorded_bits_of_the_earlier_kernels():
    """tests/golden/nll_one_cloud_bits.json (glue_reference.nll_golden_cases): loss_count word for word, the sign of a zero loss
    included, and the gradient byte for byte, at every n around the boundaries between the wave, the one-workgroup and the partials +
    finish forms; n = 0 with null log_probs / target."""
    cases = 0
    for case, lp, target, grad_loss in G.nll_golden_cases():
        loss_count, grad = nll_run(lp, target, case["ignore"], grad_loss, what=str(case))
        got = loss_count.view(np.uint32)
        assert [int(got[0]), int(got[1])] == case["loss_count"], (case, got)
        assert hashlib.sha256(np.ascontiguousarray(grad).tobytes()).hexdigest() == case["grad_sha256"], case
        cases += 1
    assert cases == 9 * (3 * 3 + 1)


@pytest.mark.parametrize("n", [1, 257, 524289])
def test_nll_every_label_ignored(n):
    """Loss compares equal to 0, the count reads 1, the gradient is zeros only (no NaN of the pre-fill survives)."""
    for ignore, value in ((1, 1), (-100, -100), (9, 9)):
        lp, _ = G.nll_random_case(n, 2, None, 3)
        target = np.full(n, value, np.int64)
        loss_count, grad = nll_run(lp, target, ignore, 2.0, what=f"all ignored n={n} ignore={ignore}")
        assert loss_count[0] == 0.0 and loss_count[1] == 1.0
        assert not np.isnan(grad).any() and not grad.any()


@pytest.mark.parametrize("n", [1, 257, 1025, 1200003])
def test_nll_one_live_label_in_the_last_row(n):
    lp, _ = G.nll_random_case(n, 5, None, 4)
    target = np.full(n, -100, np.int64)
    target[-1] = 3
    loss_count, grad = nll_run(lp, target, -100, 1.0, what=f"one live label n={n}")
    assert_equal_bits(loss_count, np.array([-lp[-1, 3], 1.0], np.float32), "loss_count")
    want = np.zeros((n, 5))
    want[-1, 3] = -1.0
    assert_within(grad, want, 0.0, "grad")


def test_nll_non_finite_log_probabilities():
    """-inf at a live target: loss +inf.  -inf or NaN in an ignored row or a column that is not the target: nothing moves, bit for
    bit (those elements are never read)."""
    n, classes = 1025, 5
    lp, target = G.nll_random_case(n, classes, -100, 6)
    live, tc = G.nll_labels(target, classes, -100)
    assert live[0] or live[1]
    clean = nll_run(lp, target, -100, 2.0, what="clean")
    dirty = lp.copy()
    dirty[~live] = np.where(np.arange(classes) % 2, -np.inf, np.nan).astype(np.float32)
    rows = np.nonzero(live)[0]
    dirty[rows, (tc[rows] + 1) % classes] = np.nan
    dirty[rows, (tc[rows] + 2) % classes] = -np.inf
    out = nll_run(dirty, target, -100, 2.0, what="non-finite where nothing is read")
    assert_equal_bits(out[0], clean[0], "loss_count")
    assert_equal_bits(out[1], clean[1], "grad")
    row = int(rows[len(rows) // 2])
    dirty[row, tc[row]] = -np.inf
    loss_count, grad = nll_run(dirty, target, -100, 2.0, what="-inf at a live target")
    assert np.isposinf(loss_count[0]) and loss_count[1] == clean[0][1]
    assert_equal_bits(grad, clean[1], "grad with an infinite loss")
    G.assert_nll(loss_count, grad, dirty, target, -100, 2.0, "-inf at a live target")


def test_nll_of_no_rows():
    """n = 0: loss 0 and count 1 from the forward (null log_probs / target are fine), the backward returns OK and writes nothing."""
    for classes in (1, 5):
        loss_count, grad = Guarded(2), Guarded(8, prefill_bits=NAN_BITS)
        ws, ws_bytes = dirty_workspace()
        rcs = nll_call(None, None, 0, classes, -100, gpu(np.ones(1, np.float32)), loss_count, grad, ws, ws_bytes)
        assert rcs == (0, 0)
        loss_count.guards_intact("loss_count")
        lc = loss_count.numpy()
        assert lc[0] == 0.0 and lc[1] == 1.0
        grad.untouched("grad of no rows", bits=NAN_BITS)


def test_nll_refusals_write_nothing_and_the_next_call_is_right():
    """classes = 0, a negative n, a null buffer and a workspace one byte short (or none) are all LN_ERR_ARG (the code this entry
    point has always returned for its workspace, as ln_norm.hip and ln_lovasz.hip do; other files use LN_ERR_WORKSPACE); nothing is
    launched: loss_count, the gradient, the workspace and every sentinel keep their bits."""
    n, classes = 300, 5
    lp, target = G.nll_random_case(n, classes, -100, 8)
    d_lp, d_target, d_gl = gpu(lp), gpu(target), gpu(np.ones(1, np.float32))
    ws, ws_bytes = dirty_workspace()
    # (forward arguments, backward arguments, expected codes; None: that call is valid and runs)
    for what, fwd, bwd in (
            ("classes = 0", dict(classes=0), dict(classes=0)),
            ("n < 0", dict(n=-1), dict(n=-1)),
            ("null log_probs", dict(lp=None), None),
            ("null target", dict(target=None), dict(target=None)),
            ("null loss_count", dict(loss_count=None), dict(loss_count=None)),
            ("workspace one byte short", dict(ws_bytes=ws_bytes - 1), None),
            ("null workspace", dict(ws=None), None),
            ("null grad_loss", None, dict(grad_loss=None)),
            ("null grad_log_probs", None, dict(grad=None))):
        lib, stream = lib_and_stream()
        loss_count, grad = Guarded(2), Guarded(n * classes, prefill_bits=NAN_BITS)
        a = dict(lp=d_lp, target=d_target, n=n, classes=classes, ws=ws, ws_bytes=ws_bytes, loss_count=loss_count, grad_loss=d_gl, grad=grad,
                 code=G.LN_ERR_ARG)
        p = lambda t: None if t is None else (t.ptr if isinstance(t, Guarded) else t.data_ptr())  # noqa: E731
        if fwd is not None:
            f = {**a, **fwd}
            rc = lib.ln_nll_forward(p(f["lp"]), p(f["target"]), f["n"], f["classes"], -100, p(f["ws"]), f["ws_bytes"], p(f["loss_count"]), stream)
            assert rc == f["code"], (what, "forward", rc)
        if bwd is not None:
            b = {**a, **bwd}
            rc = lib.ln_nll_backward(p(b["target"]), p(b["grad_loss"]), p(b["loss_count"]), b["n"], b["classes"], -100, p(b["grad"]), stream)
            assert rc == b["code"], (what, "backward", rc)
        torch.cuda.synchronize()
        if fwd is not None:
            loss_count.untouched(f"{what} loss_count")
        if bwd is not None:
            grad.untouched(f"{what} grad", bits=NAN_BITS)
        assert torch.equal(ws, torch.full_like(ws, 1e30)), f"{what}: the workspace was written"
        out = nll_run(lp, target, -100, 1.0, what="after " + what)
        G.assert_nll(out[0], out[1], lp, target, -100, 1.0, "after " + what)


def test_nll_two_runs_and_a_misaligned_run_are_bitwise_equal():
    for n, classes in ((1025, 20), (1200003, 2)):
        lp, target = G.nll_random_case(n, classes, -100, 9)
        a = nll_run(lp, target, -100, 0.75)
        for offset in (0, 1):
            b = nll_run(lp, target, -100, 0.75, offset=offset)
            assert_equal_bits(a[0], b[0], f"n={n} offset={offset} loss_count")
            assert_equal_bits(a[1], b[1], f"n={n} offset={offset} grad")


@pytest.mark.parametrize("ignore", [None, -100, 2, 12])
def test_nll_loss_gather_is_held_to_the_same_bounds(ignore):
    """The autograd wrapper on float32 CUDA inputs (it takes the kernels: the graph node says so), labels out of range included."""
    import lattice_net_amd.losses as L
    n, classes = 1025, 5
    lp_np, target_np = G.nll_random_case(n, classes, ignore, 12)
    lp = gpu(lp_np).requires_grad_(True)
    loss = L.nll_loss_gather(lp, gpu(target_np), ignore)
    assert type(loss.grad_fn).__name__.startswith("_NllFunction"), type(loss.grad_fn).__name__
    (loss * 3.0).backward()
    raw = nll_run(lp_np, target_np, ignore, 3.0)
    assert_equal_bits(f32(loss).reshape(1), raw[0][:1], "wrapper loss against the raw call")
    assert_equal_bits(f32(lp.grad), raw[1], "wrapper gradient against the raw call")
    ratio = G.assert_nll(raw[0], f32(lp.grad), lp_np, target_np, ignore, 3.0, f"wrapper ignore={ignore}")
    print(f"nll_loss_gather ignore={ignore}: worst error / bound of the loss {ratio}")
