"""The per-vertex linear layer on fp16 rows (csrc/ln_linear_f16.hip) against fp64 at every form of its own dispatch
(csrc/ln_linear_f16_plan.h), element by element, through the C ABI, with the helpers of tests/conv_reference.py and in the conventions
of test_gpu_conv_f16_forms.py: outputs pre-filled with NaN, NaN sentinels behind every output, the workspace exactly the queried size
with sentinel bytes behind it, rc checked, one synchronize before anything is read.

CASES: (rows, cin, cout, x_off).  Which launches a row takes is not written here but asked of the plan itself:
tests/test_linear_f16_plan.py::test_linear_f16_table_reaches_every_form runs tests/cabi/linear_f16_plan_check.cpp over this table on the
CPU and names any form that no case takes.  Row counts: 1, 15, 65 and 1300, 513 (just above one slab chunk of 512 rows), 1025 (just
above two), and 32 833 = 513 tiles of 64 rows, at which a workgroup walks a second tile behind one staging of its bank.  Each case runs
four times (RUNS): with and without bias, residual, grad_x and grad_b, each option once alone with one other and once in full.

The reference sees the weights as the kernels do, rounded to fp16 (w.astype(float16)); x, the residual and grad_y are fp16 numbers.
Bounds (those of the fp16 convolution tests): y and grad_x within 1e-5 x (sum of the magnitudes of the terms, bias and residual
included) + 2^-11 |ref| (fp32 accumulation in any order, one rounding of an fp16 result); grad_w and grad_b within 1e-5 x (sum of
magnitudes).  Worst error / bound measured on an MI355X: see DESIGN.md 4.6."""
import ctypes

import numpy as np
import pytest
import torch

from lattice_net_amd import _lib
from tests import conv_reference as C
from tests.test_gpu_conv_f16_forms import _half_at
from tests.test_gpu_conv_two_lattices import RTOL, SENTINEL, _dev, _intact, _rng, _workspace
from tests.test_linear_f16_plan import build_checker, linear_f16_plans

pytestmark = pytest.mark.gpu
REL = {"y": 2.0 ** -11, "grad_x": 2.0 ** -11, "grad_w": 0.0, "grad_b": 0.0}
GUARD = 64  # NaN elements behind every output

ISSUE_ROWS = (1, 15, 65, 1300, 513, 1025)
ISSUE_WIDTHS = [(16, 16), (32, 32), (64, 16), (16, 64), (128, 32), (32, 128), (96, 48), (48, 96), (256, 256), (64, 240), (24, 20), (4, 3),
                (130, 7), (64, 64)]
CASES = [
    (1300, 16, 16, 0),     # K = 16 steps both ways; weight-gradient tile (1, 1); three slabs
    (65, 32, 32, 0),       # K = 32; one row into a second tile
    (1300, 64, 16, 0),     # weight-gradient tile (1, 4)
    (513, 16, 64, 0),      # tile (4, 1); two slabs
    (1025, 128, 32, 0),    # three slabs
    (1300, 32, 128, 0),    # one chunk of 128 columns
    (15, 96, 48, 0),       # chunks 2, 1; input gradient K = 16 steps over 48, chunks 4, 2; one slab
    (1300, 48, 96, 0),     # K = 16 steps over 48; weight-gradient tiles (4, 2), (4, 1), (2, 2), (2, 1)
    (1025, 256, 256, 0),   # the largest bank: two chunks of 128 columns each way; sixteen weight-gradient tiles (4, 4)
    (1300, 64, 240, 0),    # chunks 8, 4, 2, 1; the bias gradient summed by five launches
    (1300, 24, 20, 0),     # one thread per element; weight-gradient fallback
    (1, 4, 3, 0),          # ... one row
    (1025, 130, 7, 0),     # ... gridDim.y = 4
    (513, 64, 64, 2),      # a matrix-core shape with `x` 2 bytes off: forward and weight gradient element-wise, input gradient on the matrix cores
    # beyond the issue's list: what its widths and row counts do not reach
    (1300, 32, 256, 0),    # one chunk of 256 columns
    (1, 64, 64, 0),        # one row on the matrix cores
    (15, 24, 20, 0),       # fallback, one slab
    (513, 4, 3, 0),        # fallback, two slabs
    (32833, 16, 16, 0),    # 513 tiles: two tiles per workgroup, the last workgroup with one
]
# (bias, residual, grad_x, grad_b)
RUNS = [(True, True, True, True), (False, False, False, False), (True, False, True, False), (False, True, False, True)]


def _id(c):
    return "%dx%dto%d" % c[:3] + ("-x+%d" % c[3] if c[3] else "")


def _operands(family, case, rng):
    """x [rows, cin], w [cout, cin], bias [cout], residual [rows, cout], grad_y [rows, cout] as fp32 arrays; x, residual and grad_y hold
    fp16 numbers.  exact: small integers (w in -1..1: an fp16 number, results below 2048)."""
    rows, cin, cout = case[:3]
    if family == "exact":
        i = lambda a, shape: rng.integers(-a, a + 1, shape).astype(np.float32)
        return i(2, (rows, cin)), i(1, (cout, cin)), i(2, (cout,)), i(2, (rows, cout)), i(2, (rows, cout))
    h = lambda a: a.astype(np.float16).astype(np.float32)
    w = (rng.standard_normal((cout, cin)) / np.sqrt(cin)).astype(np.float32)  # fp32 master weights: NOT fp16 numbers
    return (h(rng.standard_normal((rows, cin))), w, rng.standard_normal((cout,)).astype(np.float32), h(rng.standard_normal((rows, cout))),
            h(rng.standard_normal((rows, cout))))


def _references(x, w, bias, residual, gy):
    """{name: (fp64 reference, sum of the magnitudes of its terms)} for the full run; `y0`: the product alone"""
    x, wh, bias, residual, gy = C.f64(x), C.f64(w.astype(np.float16)), C.f64(bias), C.f64(residual), C.f64(gy)
    ax, aw, ag = np.abs(x), np.abs(wh), np.abs(gy)
    return {"y0": (x @ wh.T, ax @ aw.T), "bias": (bias[None, :], np.abs(bias)[None, :]), "residual": (residual, np.abs(residual)),
            "grad_x": (gy @ wh, ag @ aw), "grad_w": (gy.T @ x, ag.T @ ax), "grad_b": (gy.sum(0), ag.sum(0))}


def _expected(refs, run):
    bias, residual, grad_x, grad_b = run
    y, by = refs["y0"]
    for k, on in (("bias", bias), ("residual", residual)):
        if on:
            y, by = y + refs[k][0], by + refs[k][1]
    want = {"y": (y, by), "grad_w": refs["grad_w"]}
    if grad_x:
        want["grad_x"] = refs["grad_x"]
    if grad_b:
        want["grad_b"] = refs["grad_b"]
    return want


def _out(shape, dtype):
    """an output pre-filled with NaN with GUARD elements of NaN behind it: (flat buffer, view of `shape`)"""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), float("nan"), dtype=dtype, device="cuda")
    return buf, buf[:n].view(shape)


class _Call:
    """One forward + backward through the C ABI over device operands; nothing is read before check()."""

    def __init__(self, case, d, run, rows=None):
        lib = _lib.load()
        self.case, self.run = case, run
        n_alloc, cin, cout, _ = case
        rows = n_alloc if rows is None else rows
        bias, residual, grad_x, grad_b = run
        self.bufs = {"y": _out((n_alloc, cout), torch.float16), "grad_w": _out((cout, cin), torch.float32)}
        if grad_x:
            self.bufs["grad_x"] = _out((n_alloc, cin), torch.float16)
        if grad_b:
            self.bufs["grad_b"] = _out((cout,), torch.float32)
        self.rows = rows
        self.q = lib.ln_linear_backward_f16_workspace_bytes(rows, cin, cout)
        self.ws = _workspace(self.q)
        p = lambda k: _lib.ptr(self.bufs[k][1]) if k in self.bufs else None
        self.rcs = [lib.ln_linear_forward_f16(_lib.ptr(d["x"]), _lib.ptr(d["w"]), _lib.ptr(d["bias"]) if bias else None,
                                              _lib.ptr(d["residual"]) if residual else None, rows, cin, cout, p("y"), None),
                    lib.ln_linear_backward_f16(_lib.ptr(d["x"]), _lib.ptr(d["grad_y"]), _lib.ptr(d["w"]), rows, cin, cout, p("grad_x"), p("grad_w"),
                                               p("grad_b"), _lib.ptr(self.ws), self.q, None)]
        self.err = lib.ln_last_error_string()

    def results(self):
        """after the synchronize: {name: fp64-comparable array of the first `rows` rows}; sentinels and untouched rows checked"""
        assert self.rcs == [0, 0], (self.rcs, self.err)
        _intact(self.ws, self.q, f"ln_linear_backward_f16 {_id(self.case)}")
        got = {}
        for k, (buf, view) in self.bufs.items():
            assert bool(torch.isnan(buf[view.numel():]).all()), f"{_id(self.case)} {self.run}: elements behind {k} were written"
            a = view
            if k in ("y", "grad_x"):
                assert bool(torch.isnan(view[self.rows:]).all()), f"{_id(self.case)} {self.run}: rows of {k} behind the last were written"
                a = view[:self.rows]
            got[k] = a.float().cpu().numpy() if a.dtype == torch.float16 else a.cpu().numpy()
        return got


def _device(case, x, w, bias, residual, gy):
    return {"x": _half_at(x, case[3]), "w": _dev(w), "bias": _dev(bias), "residual": _half_at(residual), "grad_y": _half_at(gy)}


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_linear_f16_integer_operands_bit_for_bit(case):
    ops = _operands("exact", case, _rng(case, 0))
    refs = _references(*ops)
    full = _expected(refs, RUNS[0])
    for k, (ref, bound) in full.items():  # the reference meets the family's condition before any result is compared with it
        C.assert_exact_family(bound, ref, half=k in ("y", "grad_x"), what=k)
    d = _device(case, *ops)
    calls = [_Call(case, d, run) for run in RUNS]
    torch.cuda.synchronize()
    for call in calls:
        got = call.results()
        for k, (ref, _) in _expected(refs, call.run).items():
            C.exact(got[k], ref, f"{_id(case)} {call.run} {k}")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_linear_f16_random_operands_within_the_fp32_accumulation_bound(case):
    """Every element within 1e-5 of the sum of the magnitudes of its terms, plus 2^-11 |ref| for the two fp16 results; the full run
    twice: bitwise the same."""
    ops = _operands("random", case, _rng(case, 1))
    refs = _references(*ops)
    d = _device(case, *ops)
    calls = [_Call(case, d, run) for run in RUNS] + [_Call(case, d, RUNS[0])]
    torch.cuda.synchronize()
    results = [call.results() for call in calls]
    for call, got in zip(calls[:len(RUNS)], results):
        want = _expected(refs, call.run)
        shares = {k: C.worst_share(got[k], *want[k], RTOL, REL[k]) for k in want}
        print("LINEAR_F16 random %s %s: worst error / bound: %s" % (_id(case), "".join("BRXG"[j] if on else "-" for j, on in enumerate(call.run)),
                                                                     " ".join(f"{k} {s:.3g}" for k, s in shares.items())))
        for k in want:
            C.within(got[k], *want[k], RTOL, f"{_id(case)} {call.run} {k}", rel=REL[k])
    for k in results[0]:
        assert np.array_equal(results[0][k], results[-1][k]), f"{_id(case)}: {k} differs between two runs"


POISON = [(1300, 64, 64, 0), (1300, 48, 96, 0), (1300, 24, 20, 0), (1300, 64, 64, 2), (600, 256, 32, 0)]


@pytest.mark.parametrize("case", POISON, ids=_id)
def test_linear_f16_nan_rows_stay_where_they_are(case):
    """Integer operands in buffers of case[0] rows, the call over 37 rows fewer (a partial wave, a partial tile, a partial slab chunk):
    the rows behind `rows` of x, the residual and grad_y are NaN and change nothing, bit for bit; then one row of x inside is NaN and
    y differs in that row alone (all of it NaN), as a clamped index with a select leaves it and a multiply with zero would not."""
    n_alloc, cin, cout, _ = case
    rows, hot = n_alloc - 37, 700 if n_alloc > 800 else 130
    x, w, bias, residual, gy = _operands("exact", case, _rng(case, 2))
    refs = _references(x[:rows], w, bias, residual[:rows], gy[:rows])
    want = _expected(refs, RUNS[0])
    for k, (ref, bound) in want.items():
        C.assert_exact_family(bound, ref, half=k in ("y", "grad_x"), what=k)
    for a in (x, residual, gy):
        a[rows:] = np.nan
    x_hot = x.copy()
    x_hot[hot] = np.nan
    d = _device(case, x, w, bias, residual, gy)
    d_hot = dict(d, x=_half_at(x_hot, case[3]))
    lib = _lib.load()
    y_hot_buf, y_hot = _out((n_alloc, cout), torch.float16)
    call = _Call(case, d, RUNS[0], rows=rows)
    rc = lib.ln_linear_forward_f16(_lib.ptr(d_hot["x"]), _lib.ptr(d["w"]), _lib.ptr(d["bias"]), _lib.ptr(d["residual"]), rows, cin, cout, _lib.ptr(y_hot), None)
    torch.cuda.synchronize()
    assert rc == 0, lib.ln_last_error_string()
    got = call.results()
    for k, (ref, _) in want.items():
        C.exact(got[k], ref, f"{_id(case)} {k}, NaN rows behind `rows`")
    y_hot = y_hot[:rows].float().cpu().numpy()
    assert np.isnan(y_hot[hot]).all(), f"{_id(case)}: the NaN row of x did not reach its row of y"
    keep = np.arange(rows) != hot
    C.exact(y_hot[keep], want["y"][0][keep], f"{_id(case)} y, x[{hot}] = NaN")
    assert bool(torch.isnan(y_hot_buf[rows * cout:]).all())


def _launches(call):
    """return code of `call()` and the number of kernel launches of the library it made (test_gpu_lovasz.py)"""
    lib = _lib.load()
    assert lib.ln_profile_begin(b"*", 64) == 0
    rc = call()
    ms, count = ctypes.c_double(), ctypes.c_int()
    assert lib.ln_profile_end(ctypes.byref(ms), ctypes.byref(count)) == 0
    return rc, count.value


def test_linear_f16_no_rows():
    """rows == 0: rc 0, nothing is read (every input pointer NULL), y and grad_x stay as they were, grad_w and grad_b are zeros, the
    workspace is neither needed nor touched"""
    lib = _lib.load()
    cin, cout = 64, 48
    (yb, y), (gxb, gx), (gwb, gw), (gbb, gb) = (_out((8, cout), torch.float16), _out((8, cin), torch.float16), _out((cout, cin), torch.float32),
                                                _out((cout,), torch.float32))
    q = lib.ln_linear_backward_f16_workspace_bytes(0, cin, cout)
    ws = _workspace(q)
    rcs = [lib.ln_linear_forward_f16(None, None, None, None, 0, cin, cout, _lib.ptr(y), None),
           lib.ln_linear_backward_f16(None, None, None, 0, cin, cout, _lib.ptr(gx), _lib.ptr(gw), _lib.ptr(gb), _lib.ptr(ws), q, None),
           lib.ln_linear_backward_f16(None, None, None, 0, cin, cout, None, _lib.ptr(gw), None, None, 0, None)]
    torch.cuda.synchronize()
    assert rcs == [0, 0, 0], lib.ln_last_error_string()
    assert bool(torch.isnan(yb).all()) and bool(torch.isnan(gxb).all())
    assert bool((gw == 0).all()) and bool((gb == 0).all()) and bool(torch.isnan(gwb[cout * cin:]).all()) and bool(torch.isnan(gbb[cout:]).all())
    assert bool((ws == SENTINEL).all()), "ln_linear_backward_f16 at 0 rows wrote its workspace"


def test_linear_f16_refusals_return_their_code_and_write_nothing():
    lib = _lib.load()
    rows, cin, cout = 700, 64, 48
    ARG, WORKSPACE = -1, -4
    x, w, bias, residual, gy = _operands("exact", (rows, cin, cout, 0), _rng((rows, cin, cout), 3))
    d = _device((rows, cin, cout, 0), x, w, bias, residual, gy)
    outs = {"y": _out((rows, cout), torch.float16), "grad_x": _out((rows, cin), torch.float16), "grad_w": _out((cout, cin), torch.float32),
            "grad_b": _out((cout,), torch.float32)}
    q = lib.ln_linear_backward_f16_workspace_bytes(rows, cin, cout)
    ws = _workspace(q)
    P = {k: _lib.ptr(v) for k, v in d.items()}
    O = {k: _lib.ptr(v[1]) for k, v in outs.items()}

    def fwd(x=P["x"], w=P["w"], y=O["y"], rows=rows, cin=cin, cout=cout):
        return lambda: lib.ln_linear_forward_f16(x, w, P["bias"], P["residual"], rows, cin, cout, y, None)

    def bwd(x=P["x"], gy=P["grad_y"], w=P["w"], gx=O["grad_x"], gw=O["grad_w"], wsp=_lib.ptr(ws), nbytes=q, rows=rows, cin=cin, cout=cout):
        return lambda: lib.ln_linear_backward_f16(x, gy, w, rows, cin, cout, gx, gw, O["grad_b"], wsp, nbytes, None)

    refused = [("forward rows < 0", fwd(rows=-1), ARG), ("forward cin < 1", fwd(cin=0), ARG), ("forward cout < 1", fwd(cout=0), ARG),
               ("forward null x", fwd(x=None), ARG), ("forward null w", fwd(w=None), ARG), ("forward null y", fwd(y=None), ARG),
               ("backward rows < 0", bwd(rows=-1), ARG), ("backward cin < 1", bwd(cin=0), ARG), ("backward cout < 1", bwd(cout=-1), ARG),
               ("backward null x", bwd(x=None), ARG), ("backward null grad_y", bwd(gy=None), ARG), ("backward null w with grad_x", bwd(w=None), ARG),
               ("backward null grad_w", bwd(gw=None), ARG), ("backward null workspace", bwd(wsp=None), WORKSPACE),
               ("backward workspace one byte short", bwd(nbytes=q - 1), WORKSPACE), ("backward workspace of 0 bytes", bwd(nbytes=0), WORKSPACE)]
    for what, call, code in refused:
        rc, launches = _launches(call)
        msg = lib.ln_last_error_string()
        assert rc == code and launches == 0 and b"ln_linear_" in msg, (what, rc, code, launches, msg)
    torch.cuda.synchronize()
    for k, (buf, _) in outs.items():
        assert bool(torch.isnan(buf).all()), f"a refused call wrote {k}"
    assert bool((ws == SENTINEL).all()), "a refused call wrote the workspace"


@pytest.fixture(scope="module")
def plan_tool(tmp_path_factory):
    """the plan checker as a plain host program (no sanitizer: those builds run in the CPU tests of test_linear_f16_plan.py)"""
    return build_checker(tmp_path_factory.mktemp("plan_lin16_tool"), sanitize=False)


@pytest.mark.parametrize("case", [(1300, 64, 240, 0), (1025, 256, 256, 0), (1025, 130, 7, 0), (513, 64, 64, 2)], ids=_id)
def test_linear_f16_plan_is_what_runs(plan_tool, case):
    """The launches the profile hooks count are the launches the plan lists (+ one slab sum for grad_w and one for grad_b): the plan is
    what ln_linear_f16.hip executes, not a description beside it."""
    assert case in CASES
    rows, cin, cout, _ = case
    plan = linear_f16_plans(plan_tool, [case])[case]
    lib = _lib.load()
    d = _device(case, *_operands("exact", case, _rng(case, 4)))
    (_, y), (_, gx), (_, gw), (_, gb) = (_out((rows, cout), torch.float16), _out((rows, cin), torch.float16), _out((cout, cin), torch.float32),
                                         _out((cout,), torch.float32))
    q = lib.ln_linear_backward_f16_workspace_bytes(rows, cin, cout)
    ws = _workspace(q)
    P = {k: _lib.ptr(v) for k, v in d.items()}
    calls = {"forward": (lambda: lib.ln_linear_forward_f16(P["x"], P["w"], P["bias"], P["residual"], rows, cin, cout, _lib.ptr(y), None),
                         plan["FWD"]["launches"]),
             "backward": (lambda: lib.ln_linear_backward_f16(P["x"], P["grad_y"], P["w"], rows, cin, cout, _lib.ptr(gx), _lib.ptr(gw), _lib.ptr(gb),
                                                             _lib.ptr(ws), q, None), plan["GW"]["launches"] + 2 + plan["GX"]["launches"]),
             "backward, grad_w alone": (lambda: lib.ln_linear_backward_f16(P["x"], P["grad_y"], None, rows, cin, cout, None, _lib.ptr(gw), None,
                                                                           _lib.ptr(ws), q, None), plan["GW"]["launches"] + 1)}
    for k, (call, want) in calls.items():
        rc, launches = _launches(call)
        assert rc == 0 and launches == want, (k, rc, launches, want, plan)
    torch.cuda.synchronize()
