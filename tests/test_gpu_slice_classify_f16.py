"""The DeformSlice head on fp16 lattice values (csrc/ln_classify_f16.hip) through the C ABI (`pytest -m gpu`): ln_gather_forward_f16,
ln_slice_classify_forward_f16, ln_slice_classify_backward_f16.

fp16 -> fp32 is exact and the fp16 kernels keep tiles, grids, slab layout and order of operations of the fp32 kernels, so there is no
error analysis of their own: every output must equal, BIT FOR BIT, what the fp32 entry point gives on the same values widened to fp32.
Every case draws P.make_sc_inputs, rounds the values to fp16 (v16), runs the fp16 call on v16 and the fp32 call on v16.astype(float32)
with every other operand identical (the accumulated outputs start from the same non-zero contents), and asserts
- logits, grad_sliced, w_eff, g_delta_w, g_lin_w, g_lin_b of the two calls equal bit for bit;
- the logits equal P.sc_forward_reference (the ordered fp32 evaluation on the CPU) on the widened values bit for bit: not only two GPU
  kernels that share text are compared;
- the backward outputs within the counted bounds of P.sc_backward_reference, and in the exact (small-integer) run equal to fp64.
Every output of the fp16 call has 64 sentinel rows behind it, the workspace 256 guard bytes and the slabs no workgroup owns.

Cases (tests/point_reference.py and the GENERAL_CASES of tests/test_gpu_slice_classify.py, which hold the fp32 kernels to fp64 at the
same shapes): the 16 wave forward instances, the 16 wave backward instances beyond the grid cap and with idle waves, every GENERAL_CASES
entry whose forms are v4 at both ends (PB = 64 / 32 / 16 forward, 64 / 16 / 8 backward, d = 4, C = 50, beyond both grid caps) and the
two mixed pairings (wave forward, v4 backward with PB = 32).  test_cases_reach_every_form asserts on the CPU that this is every
(form, PB) a V % 4 == 0 shape can take.  Here `aligned` means: values 8-byte aligned, grad_sliced 16-byte aligned.

Each test prints its worst error / bound ratio per bounded output (`pytest -s`); nothing is asserted on that figure."""
import itertools

import numpy as np
import pytest
import torch

from tests import point_reference as P
from tests.test_gpu_slice_classify import GENERAL_CASES, GUARD, WS_GUARD, Guarded, dev, gpu, lib_

pytestmark = pytest.mark.gpu

LN_ERR_ARG, LN_ERR_UNSUPPORTED, LN_ERR_WORKSPACE = -1, -2, -4
BWD_KEYS = ("g_delta_w", "g_lin_w", "g_lin_b", "grad_sliced", "w_eff")

V4_CASES = [k for k, (f, b) in GENERAL_CASES.items() if f[0] == "v4" and b is not None and b[0] == "v4"]
MIXED_CASES = [(3, 160, 8, 293), (3, 160, 24, 293)]
SCALAR_SHAPES = [(3, 5, 3), (2, 30, 20), (3, 512, 20)]  # (the last: fp32 has a scalar forward and no backward for it)


def _form_pb(form):
    return None if form is None or form[0] == "scalar" else (form[0], form[1] if form[0] == "v4" else None)


def test_cases_reach_every_form():
    """CPU only: the (form, PB) pairs of the cases are all the pairs sc_forward_form / sc_backward_form return at V % 4 == 0."""
    can_f, can_b = set(), set()
    for d, v, c in itertools.product(range(1, 7), range(4, 1025, 4), (1, 3, 8, 13, 20, 21, 32, 33, 40, 50, 64)):
        can_f.add(_form_pb(P.sc_forward_form(d, v, c)))
        can_b.add(_form_pb(P.sc_backward_form(d, v, c)))
    shapes = [(d, v, c) for d, v, c in P.WAVE_FWD_CASES + P.WAVE_BWD_CASES] + [k[:3] for k in V4_CASES + MIXED_CASES]
    got_f = {_form_pb(P.sc_forward_form(*s)) for s in shapes}
    got_b = {_form_pb(P.sc_backward_form(*s)) for s in shapes}
    assert got_f == can_f - {None} and got_b == can_b - {None}, (can_f - got_f, can_b - got_b)
    assert len(V4_CASES) == 8 and all(GENERAL_CASES[k][0][0] == "wave" and GENERAL_CASES[k][1][0] == "v4" for k in MIXED_CASES)


def gpu_h(v16, offset=0):
    """fp16 device copy; `offset` halves in front of it: a view whose pointer is 2 * offset bytes off its alignment"""
    v16 = np.ascontiguousarray(v16)
    buf = torch.zeros((v16.size + 8,), dtype=torch.float16, device=dev())
    t = buf[offset:offset + v16.size].view(v16.shape)
    t.copy_(torch.from_numpy(v16))
    assert t.data_ptr() % 8 == (2 * offset) % 8
    return t


def make_case(d, v, c, n, exact, seed=0, edit=None):
    """(inputs with `values` widened from fp16, the fp16 values).  `edit(v16, inp)` may plant edge values before the widening."""
    m = P.table_rows(n)
    inp = P.make_sc_inputs(n, m, d, v, c, seed + 1000 * exact, exact)
    v16 = inp["values"].astype(np.float16)
    if edit is not None:
        edit(v16, inp)
    inp["values"] = v16.astype(np.float32)
    assert np.array_equal(inp["values"].astype(np.float16).view(np.uint16), v16.view(np.uint16)) or np.isnan(inp["values"]).any()
    return inp, v16


class Calls:
    """One case on the device: operands, and the forward / backward of either dtype into fresh guarded outputs."""

    def __init__(self, inp, v16, d, n, values32=None, offset_h=0, offset_gs=0):
        self._lib, self.lib = lib_()
        self.inp, self.d, self.n = inp, d, n
        self.c, self.v = inp["lin_w"].shape
        self.m = inp["values"].shape[0]
        self.st = self._lib.stream_ptr(dev())
        self.values = {True: gpu_h(v16, offset_h), False: gpu(inp["values"] if values32 is None else values32)}
        self.dw, self.lw, self.lb, self.idx, self.w, self.gl = (gpu(inp[k]) for k in ("delta_w", "lin_w", "lin_b", "idx", "w", "grad_logits"))
        self.offset_gs = offset_gs

    def forward(self, half):
        logits = Guarded(self.n, self.c)
        fn = self.lib.ln_slice_classify_forward_f16 if half else self.lib.ln_slice_classify_forward
        rc = fn(self.values[half].data_ptr(), self.dw.data_ptr(), self.lw.data_ptr(), self.lb.data_ptr(), self.idx.data_ptr(), self.w.data_ptr(),
                self.n, self.d, self.v, self.c, logits.ptr(), self.st)
        torch.cuda.synchronize()
        return rc, logits

    def backward(self, half, g_values=None, short_ws=0):
        inp, n, d, v, c = self.inp, self.n, self.d, self.v, self.c
        out = dict(g_delta_w=Guarded(n, d + 1, inp["g_delta_w0"]), g_lin_w=Guarded(c, v, inp["g_lin_w0"]), g_lin_b=Guarded(c, 1, inp["g_lin_b0"]),
                   grad_sliced=Guarded(n, v, offset=self.offset_gs if half else 0), w_eff=Guarded(n * (d + 1), 1))
        size = self.lib.ln_slice_classify_backward_f16_workspace_bytes if half else self.lib.ln_slice_classify_backward_workspace_bytes
        ws_bytes = size(n, d, v, c)
        ws = torch.full((ws_bytes + WS_GUARD,), 0xA5, dtype=torch.uint8, device=dev())
        fn = self.lib.ln_slice_classify_backward_f16 if half else self.lib.ln_slice_classify_backward
        rc = fn(self.gl.data_ptr(), self.values[half].data_ptr(), self.dw.data_ptr(), self.lw.data_ptr(), self.idx.data_ptr(), self.w.data_ptr(),
                n, d, v, c, None if g_values is None else g_values.data_ptr(), out["g_delta_w"].ptr(), out["g_lin_w"].ptr(),
                out["g_lin_b"].ptr(), out["grad_sliced"].ptr(), out["w_eff"].ptr(), ws.data_ptr(), ws_bytes - short_ws, self.st)
        torch.cuda.synchronize()
        return rc, out, ws


def assert_untouched(inp, logits, out, ws, what):
    """After a refused (or empty) call: every output buffer bitwise as it was."""
    if logits is not None:
        assert bool((logits.buf == P.SENTINEL).all()), f"{what}: logits were written"
    if out is not None:
        for k in ("g_delta_w", "g_lin_w", "g_lin_b"):
            P.assert_equal_bits(out[k].numpy().reshape(-1), inp[k + "0"].reshape(-1), f"{what} {k}")
        for k in ("grad_sliced", "w_eff"):
            assert bool((out[k].buf == P.SENTINEL).all()), f"{what}: {k} was written"
        for k, o in out.items():
            o.check(f"{what} {k}")
        assert bool((ws == 0xA5).all()), f"{what}: the workspace was written"


def run_case(d, v, c, n, exact, edit=None, finite_twin=None):
    """Forward and backward of one case in both dtypes; returns the worst error / bound ratios of the bounded backward outputs.
    `finite_twin(values32)`: edits the fp32 call's values (the NaN case: the fp32 call and the references see a finite row 0)."""
    what = f"f16 d={d} V={v} C={c} n={n} {'exact' if exact else 'random'}"
    inp, v16 = make_case(d, v, c, n, exact, edit=edit)
    if finite_twin is not None:
        finite_twin(inp["values"])
    calls = Calls(inp, v16, d, n)
    rc16, logits16 = calls.forward(True)
    assert rc16 == 0, calls.lib.ln_last_error_string()
    rc32, logits32 = calls.forward(False)
    assert rc32 == 0, calls.lib.ln_last_error_string()
    P.assert_equal_bits(logits16.numpy(), logits32.numpy(), f"{what} logits against the fp32 call")
    P.assert_equal_bits(logits16.numpy(), P.sc_forward_reference(inp, n), f"{what} logits against the ordered fp32 evaluation")
    logits16.check(f"{what} logits")
    rc16, out16, ws = calls.backward(True)
    assert rc16 == 0, calls.lib.ln_last_error_string()
    rc32, out32, _ = calls.backward(False)
    assert rc32 == 0, calls.lib.ln_last_error_string()
    for k in BWD_KEYS:
        P.assert_equal_bits(out16[k].numpy(), out32[k].numpy(), f"{what} {k} against the fp32 call")
        out16[k].check(f"{what} {k}")
    form_b = P.sc_backward_form(d, v, c)
    used = 4 * P.sc_backward_grid(n, form_b) * (c * v + c) if n else 0
    assert bool((ws[used:] == 0xA5).all()), f"{what}: the workspace was written beyond the slabs of the launched workgroups"
    if n == 0:
        assert_untouched(inp, logits16, out16, ws, what)
        return {}
    inp_ref = dict(inp, g_values0=np.zeros((calls.m, v), np.float32))
    ref, mag, bound = P.sc_backward_reference(inp_ref, n, d, form_b)
    ratios = {}
    for k in BWD_KEYS:
        got = P.f64(out16[k].numpy()).reshape(ref[k].shape)
        if exact or k == "w_eff":
            bad = got != ref[k]
            assert not bad.any(), f"{what} {k}: {int(bad.sum())} elements differ from the fp64 result"
        else:
            P.assert_within(got, ref[k], bound[k], f"{what} {k}")
            ratios[k] = P.worst_ratio(got, ref[k], bound[k])
    if exact:
        P.assert_exact_representable({k: mag[k] for k in BWD_KEYS}, what)
    return ratios


def both_runs(d, v, c, n, **kw):
    r = run_case(d, v, c, n, False, **kw)
    run_case(d, v, c, n, True, **kw)
    print(f"F16 d={d} V={v} C={c} n={n} forms {P.sc_forward_form(d, v, c)} / {P.sc_backward_form(d, v, c)} worst error / bound: "
          + ", ".join(f"{k} {x:.3f}" for k, x in r.items()))


@pytest.mark.parametrize("d,v,c", P.WAVE_FWD_CASES)
def test_forward_wave_instances(d, v, c):
    assert P.sc_forward_form(d, v, c)[0] == "wave"
    both_runs(d, v, c, P.N_FWD_WAVE)


@pytest.mark.parametrize("d,v,c", P.WAVE_BWD_CASES)
def test_backward_wave_instances_beyond_the_grid_cap(d, v, c):
    form = P.sc_backward_form(d, v, c)
    assert form[0] == "wave" and P.sc_backward_grid(P.N_WAVE_LARGE, form) == P.WAVE_BWD_GRID
    both_runs(d, v, c, P.N_WAVE_LARGE)


@pytest.mark.parametrize("d,v,c", P.WAVE_BWD_CASES)
def test_backward_wave_instances_with_idle_waves(d, v, c):
    both_runs(d, v, c, P.N_WAVE_SMALL)


@pytest.mark.parametrize("d,v,c,n", V4_CASES + MIXED_CASES, ids=[f"d{d}-V{v}-C{c}-n{n}" for d, v, c, n in V4_CASES + MIXED_CASES])
def test_v4_forms_and_mixed_pairings(d, v, c, n):
    both_runs(d, v, c, n)


# ------------------------------------------------------------------------------------------------------------------ edge inputs
EDGE_SHAPES = [(3, 32, 13), (3, 8, 20)]  # wave / wave and v4 / v4


@pytest.mark.parametrize("d,v,c", EDGE_SHAPES)
def test_no_point(d, v, c):
    """n = 0 returns 0 and writes nothing (run_case asserts every buffer untouched)."""
    both_runs(d, v, c, 0)


@pytest.mark.parametrize("d,v,c", EDGE_SHAPES)
def test_a_point_with_all_vertices_absent(d, v, c):
    """P.make_tokens makes every 11th point wholly absent: its logits are the bias, bit for bit, its gradient rows as the fp32 call's."""
    n = 293
    inp, v16 = make_case(d, v, c, n, False)
    absent = (inp["idx"].reshape(n, d + 1) < 0).all(1)
    assert absent.sum() >= n // 11
    calls = Calls(inp, v16, d, n)
    rc, logits = calls.forward(True)
    assert rc == 0, calls.lib.ln_last_error_string()
    P.assert_equal_bits(logits.numpy()[absent], np.broadcast_to(inp["lin_b"], (int(absent.sum()), c)), "logits of absent points")
    both_runs(d, v, c, n)


@pytest.mark.parametrize("d,v,c", EDGE_SHAPES)
def test_nan_in_a_row_no_token_names(d, v, c):
    """Row 0 is what an absent vertex's clamped index reads.  With an fp16 NaN in it and no token naming it every output is, bit for bit,
    that of the fp32 call (and of the references) on a table whose row 0 is zero."""
    def edit(v16, inp):
        inp["idx"][inp["idx"] == 0] = 1
        v16[0, :] = np.float16(np.nan)

    def finite_twin(values32):
        values32[0, :] = 0.0
    both_runs(d, v, c, 293, edit=edit, finite_twin=finite_twin)


@pytest.mark.parametrize("d,v,c", EDGE_SHAPES)
def test_largest_values_and_denormals(d, v, c):
    """+-65504 and fp16 denormals widen exactly: still bitwise the fp32 call, the ordered evaluation and within the fp64 bounds.  (The
    random run only: the planted values are not the small integers the exact run's premise asks for.)"""
    def edit(v16, inp):
        tiny = np.float16(2.0 ** -24)
        v16[1, :], v16[2, :], v16[3, :], v16[4, ::2] = np.float16(65504), np.float16(-65504), tiny, -3 * tiny
        v16[5:9, 1::3] = np.float16(2.0 ** -15)  # the largest power of two below the normal range
        assert tiny > 0 and float(tiny) == 2.0 ** -24
    r = run_case(d, v, c, 293, False, edit=edit)
    print(f"F16 d={d} V={v} C={c} largest values and denormals, worst error / bound: " + ", ".join(f"{k} {x:.3f}" for k, x in r.items()))


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("d,v,c", SCALAR_SHAPES)
def test_scalar_form_shapes_are_refused(d, v, c):
    assert P.sc_forward_form(d, v, c)[0] == "scalar" and (P.sc_backward_form(d, v, c) or ("scalar",))[0] == "scalar"
    n = 100
    inp = P.make_sc_inputs(n, P.table_rows(n), d, v, c, 7)
    v16 = inp["values"].astype(np.float16)
    calls = Calls(inp, v16, d, n)
    rc, logits = calls.forward(True)
    msg = calls.lib.ln_last_error_string().decode()
    assert rc == LN_ERR_UNSUPPORTED and f"V={v}" in msg and f"C={c}" in msg and f"d={d}" in msg, (rc, msg)
    rcb, out, ws = calls.backward(True)
    msg = calls.lib.ln_last_error_string().decode()
    assert rcb == LN_ERR_UNSUPPORTED and f"V={v}" in msg and f"C={c}" in msg and f"d={d}" in msg, (rcb, msg)
    assert_untouched(inp, logits, out, ws, f"refused d={d} V={v} C={c}")


@pytest.mark.parametrize("d,v,c", [(3, 32, 13), (3, 8, 20)])
def test_misaligned_pointers_are_refused(d, v, c):
    n = 100
    inp = P.make_sc_inputs(n, P.table_rows(n), d, v, c, 8)
    v16 = inp["values"].astype(np.float16)
    calls = Calls(inp, v16, d, n, offset_h=1)  # values 2 bytes off
    rc, logits = calls.forward(True)
    rcb, out, ws = calls.backward(True)
    assert rc == LN_ERR_UNSUPPORTED and rcb == LN_ERR_UNSUPPORTED, (rc, rcb)
    msg = calls.lib.ln_last_error_string().decode()
    assert f"V={v}" in msg and f"C={c}" in msg and f"d={d}" in msg and "aligned" in msg, msg
    assert_untouched(inp, logits, out, ws, "values 2 bytes off")
    calls = Calls(inp, v16, d, n, offset_gs=1)  # grad_sliced 4 bytes off
    rcb, out, ws = calls.backward(True)
    assert rcb == LN_ERR_UNSUPPORTED, rcb
    assert_untouched(inp, None, out, ws, "grad_sliced 4 bytes off")


def test_g_values_and_a_short_workspace_are_refused():
    d, v, c, n = 3, 32, 13, 100
    inp = P.make_sc_inputs(n, P.table_rows(n), d, v, c, 9)
    calls = Calls(inp, inp["values"].astype(np.float16), d, n)
    gv = torch.full((calls.m, v), 3.0, device=dev())
    rc, out, ws = calls.backward(True, g_values=gv)
    assert rc == LN_ERR_ARG, rc
    assert_untouched(inp, None, out, ws, "non-NULL g_values")
    assert bool((gv == 3.0).all())
    rc, out, ws = calls.backward(True, short_ws=4)
    assert rc == LN_ERR_WORKSPACE, rc
    assert_untouched(inp, None, out, ws, "short workspace")


# ------------------------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("v", [8, 9, 32, 130])
@pytest.mark.parametrize("d", [2, 3, 4])
@pytest.mark.parametrize("n", [293, 2048 * 64 + 69])
def test_gather_forward(d, v, n):
    """ln_gather_forward_f16 on absent-token inputs: bitwise ln_gather_forward on the widened values and the CPU reference."""
    _lib, lib = lib_()
    st = _lib.stream_ptr(dev())
    m = P.table_rows(n)
    dp1 = d + 1
    idx_np, w_np = P.make_tokens(n, m, d, seed=v + d)
    v16 = np.random.default_rng(v * 7 + d).standard_normal((m, v)).astype(np.float16)
    v32 = v16.astype(np.float32)
    idx, w = gpu(idx_np), gpu(w_np)
    vals16, vals32 = gpu_h(v16, offset=1 if v % 2 else 0), gpu(v32)  # (no alignment is asked for: odd widths put rows on odd halves anyway)
    out16, out32 = Guarded(n, dp1 * (v + 1)), Guarded(n, dp1 * (v + 1))
    assert lib.ln_gather_forward_f16(vals16.data_ptr(), idx.data_ptr(), w.data_ptr(), n, d, v, out16.ptr(), st) == 0, lib.ln_last_error_string()
    assert lib.ln_gather_forward(vals32.data_ptr(), idx.data_ptr(), w.data_ptr(), n, d, v, out32.ptr(), st) == 0, lib.ln_last_error_string()
    torch.cuda.synchronize()
    assert torch.equal(out16.t.view(torch.int32), out32.t.view(torch.int32)), f"d={d} V={v} n={n}: differs from ln_gather_forward bit for bit"
    P.assert_equal_bits(out16.numpy(), P.gather_forward_reference(v32, idx_np, w_np, n).reshape(n, dp1 * (v + 1)), f"d={d} V={v} n={n} gather")
    out16.check(f"d={d} V={v} n={n} gather")
    assert GUARD == P.GUARD_ROWS
