"""The fp16 slice forward against fp64, element by element, at every kernel instance (`pytest -m gpu`): k_slice_forward_f16 behind
ln_slice_forward_f16 / ln_slice_forward_f16_prepare_backward (csrc/ln_rows.hip), the kernel on the output side of every fp16 chain.

The C ABI is driven directly (lattice_net_amd._lib) with token arrays from tests/slice_f16_reference.py — random rows with 5 % of the
tokens absent (idx = -1, w = -1), a point wholly absent, one without its first and one without its last vertex; no hash build.  The
reference, the bound with its counting argument and the case list live there (checked on the CPU by test_slice_f16_reference.py, which
also asserts that the cases reach all 18 instances k_slice_forward_f16<d + 1, HV, CH>, d = 1 .. 6 x (HV, CH) in (4, 0) (8, 0) (8, 8)).
Every case runs three times: random and cancel within the bound, exact bit for bit the fp64 sum rounded to fp16 once.

Every `out` lies between 64 rows of a sentinel on both sides, the accumulator of ln_slice_forward_f16_prepare_backward is written over
NaNs and has a sentinel tail behind `zero_elems`, and row 0 of the values — what an absent vertex's clamped index loads — is all NaN
wherever no token names it.  The last part of the file reaches the kernel through SliceLattice on real lattices at d = 1 and d = 6.

Each test prints its worst error / bound ratio per output (`pytest -s`); nothing is asserted on that figure."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import slice_f16_reference as S
from tests.test_gpu_slice_classify import dev, lib_

pytestmark = pytest.mark.gpu

F16, F32 = np.float16, np.float32
TAIL = 4096  # sentinel floats behind the accumulator


# ------------------------------------------------------------------------------------------------------------------ device buffers
class HalfOut:
    """n * v halves of a sentinel between S.GUARD_ROWS rows of it on both sides, `offset` bytes off a 16-byte boundary."""

    def __init__(self, n, v, offset=0):
        guard = S.GUARD_ROWS * max(v, 4)  # (a multiple of 8 halves: the array itself starts 16-byte aligned)
        self.n, self.v = n, v
        self.lo, self.size = guard + offset // 2, n * v
        self.buf = torch.full((self.lo + self.size + guard,), S.SENTINEL, dtype=torch.float16, device=dev())
        self.before = self.buf.clone()
        assert self.buf.data_ptr() % 16 == 0

    def ptr(self):
        return self.buf.data_ptr() + 2 * self.lo

    def bits(self):
        return self.buf.view(torch.int16)

    def check(self, what):
        same = self.bits() == self.before.view(torch.int16)
        assert bool(same[:self.lo].all()) and bool(same[self.lo + self.size:].all()), f"{what}: the sentinel around out was written"

    def untouched(self):
        return torch.equal(self.bits(), self.before.view(torch.int16))

    def numpy(self):
        return self.buf[self.lo:self.lo + self.size].cpu().numpy().reshape(self.n, self.v)


class Acc:
    """The fp32 accumulator: NaN over [0, zero_elems), a sentinel tail behind it."""

    def __init__(self, zero_elems):
        self.ze = zero_elems
        self.buf = torch.full((zero_elems + TAIL,), float("nan"), dtype=torch.float32, device=dev())
        self.buf[zero_elems:] = S.SENTINEL
        self.before = self.buf.clone()

    def ptr(self):
        return self.buf.data_ptr()

    def check(self, what):
        assert bool((self.buf[:self.ze].view(torch.int32) == 0).all()), f"{what}: the accumulator is not +0 over its {self.ze} elements"
        assert bool((self.buf[self.ze:] == S.SENTINEL).all()), f"{what}: the accumulator was written beyond zero_elems = {self.ze}"

    def untouched(self):
        return torch.equal(self.buf.view(torch.int32), self.before.view(torch.int32))


class Operands:
    """values (fp16, `offset` bytes off a 16-byte boundary inside a larger allocation), idx and w of one run on the device."""

    def __init__(self, values16, idx, w, n, d, offset=0):
        values16 = np.ascontiguousarray(values16)
        self._lib, self.lib = lib_()
        self.st = self._lib.stream_ptr(dev())
        self.n, self.d, self.v = n, d, values16.shape[1]
        self.vbuf = torch.zeros((values16.size + 16,), dtype=torch.float16, device=dev())
        lo = offset // 2
        self.vbuf[lo:lo + values16.size].copy_(torch.from_numpy(values16.reshape(-1)))
        self.values_ptr = self.vbuf.data_ptr() + offset
        self.idx = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(dev())
        self.w = torch.from_numpy(np.ascontiguousarray(w, dtype=F32)).to(dev())
        self.idx_ptr = self.idx.data_ptr() if self.idx.numel() else self.vbuf.data_ptr()
        self.w_ptr = self.w.data_ptr() if self.w.numel() else self.vbuf.data_ptr()

    def call(self, out_ptr, acc_ptr=None, zero_elems=None, n=None, d=None, v=None, null=()):
        """ln_slice_forward_f16, or with `zero_elems` ln_slice_forward_f16_prepare_backward; `null`: operands passed as NULL."""
        ptrs = dict(values=self.values_ptr, idx=self.idx_ptr, w=self.w_ptr, out=out_ptr)
        for k in null:
            ptrs[k] = None
        args = (ptrs["values"], ptrs["idx"], ptrs["w"], self.n if n is None else n, self.d if d is None else d, self.v if v is None else v,
                ptrs["out"])
        if zero_elems is None:
            rc = self.lib.ln_slice_forward_f16(*args, self.st)
        else:
            rc = self.lib.ln_slice_forward_f16_prepare_backward(*args, acc_ptr, zero_elems, self.st)
        torch.cuda.synchronize()
        return rc

    def launches(self, *a, **kw):
        """(return code, kernel launches of the library) of one call"""
        assert self.lib.ln_profile_begin(b"*", 64) == 0
        rc = self.call(*a, **kw)
        ms, count = C.c_double(), C.c_int()
        assert self.lib.ln_profile_end(C.byref(ms), C.byref(count)) == 0
        return rc, count.value

    def error(self):
        return self.lib.ln_last_error_string().decode()


def bits16(a):
    return np.ascontiguousarray(a, dtype=F16).view(np.uint16)


def assert_same_halves(a, b, what):
    S.assert_equal_bits(np.asarray(a, F16).astype(F32), np.asarray(b, F16).astype(F32), what)


# ------------------------------------------------------------------------------------------------------------------ every instance
@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_every_instance_and_grid_edge(name):
    case = S.CASES_BY_NAME[name]
    n, d, v = case.n, case.d, case.v
    m = S.case_rows(case)
    ratios = {}
    for run in S.RUNS:
        what = f"{name} {run}"
        values, idx, w = S.make_inputs(case, run)
        ops = Operands(values, idx, w, n, d, case.off_values)
        out = HalfOut(n, v, case.off_out)
        assert S.slice_f16_instance(d, v, ops.values_ptr, out.ptr()) == S.case_instance(case), what  # the pointers are what the case says
        assert ops.call(out.ptr()) == 0, ops.error()
        out.check(what)
        got = out.numpy()
        ratios[run] = S.assert_slice_f16(got, values, idx, w, n, d, run, what)
        if n >= 4:
            assert not bits16(got[S.P_ALL_ABSENT]).any(), f"{what}: a point without a vertex is not +0 bit for bit"
        # the same launch with the accumulator of the backward pass behind it: the same rows, the accumulator +0 and not a float further
        acc, out2 = Acc(m * v), HalfOut(n, v, case.off_out)
        assert ops.call(out2.ptr(), acc.ptr(), m * v) == 0, ops.error()
        out2.check(what)
        acc.check(what)
        assert_same_halves(out2.numpy(), got, f"{what} ln_slice_forward_f16_prepare_backward against ln_slice_forward_f16")
    print(f"SLICE F16 {name} instance {S.case_instance(case)} worst error / bound: forward random {ratios['random']:.3f}, "
          f"forward cancel {ratios['cancel']:.3f}")


def test_two_runs_are_bitwise_equal():
    case = S.CASES_BY_NAME["d3-V64-n293"]
    values, idx, w = S.make_inputs(case, "random")
    ops = Operands(values, idx, w, case.n, case.d)
    outs = []
    for _ in range(2):
        out = HalfOut(case.n, case.v)
        assert ops.call(out.ptr()) == 0, ops.error()
        outs.append(out.numpy())
    assert_same_halves(outs[0], outs[1], "two runs of one case")


# ------------------------------------------------------------------------------------------------------------------ range
@pytest.mark.parametrize("d,v", [(1, 4), (3, 8), (6, 64), (3, 16)])
def test_largest_values_round_and_overflow_as_fp16_does(d, v):
    """65504 under a single live weight 1.0 is 65504; two live vertices of 65504 under 0.75 each are 98256 in fp32, whose
    round-to-nearest in fp16 is +inf; the same negated."""
    big = 65504.0
    values = np.ones((16, v), F16)
    values[0, :], values[1, :], values[2, :] = F16(np.nan), F16(big), F16(-big)
    idx = np.full((4, d + 1), -1, np.int32)
    w = np.full((4, d + 1), -1.0, F32)
    idx[0, 0], w[0, 0] = 1, 1.0
    idx[1, :2], w[1, :2] = 1, 0.75
    idx[2, d], w[2, d] = 2, 1.0
    idx[3, d - 1:], w[3, d - 1:] = 2, 0.75
    ops = Operands(values, idx.reshape(-1), w.reshape(-1), 4, d)
    out = HalfOut(4, v)
    assert ops.call(out.ptr()) == 0, ops.error()
    out.check("largest values")
    want = np.repeat(np.array([big, np.inf, -big, -np.inf], F16)[:, None], v, axis=1)
    assert_same_halves(out.numpy(), want, f"d={d} V={v} largest values")
    ref, _ = S.slice_f16_ref(values, idx.reshape(-1), w.reshape(-1), 4, d)
    assert ref[1, 0] == 98256.0 and ref[3, 0] == -98256.0


@pytest.mark.parametrize("d,v", [(1, 4), (3, 8), (6, 64)])
def test_subnormal_values_and_outputs(d, v):
    """fp16 subnormal rows k 2^-24 (|k| < 1024) under weights 1/8: every output, at most 7 * 1023 * 2^-27, lands below the normal range.
    Random k: within the bound (its 2^-25 term).  k a multiple of 8: the sum is a multiple of 2^-24, the output the fp64 sum bit for bit."""
    n, m = 293, 98
    worst = 0.0
    for step in (1, 8):
        rng = np.random.default_rng(d * 100 + v + step)
        k = step * rng.integers(-(1023 // step), 1023 // step + 1, (m, v))
        values = (k * 2.0 ** -24).astype(F16)
        assert np.array_equal(values.astype(np.float64), k * 2.0 ** -24)
        values[0, :] = F16(np.nan)
        idx, w = S.make_tokens(n, m, d, seed=step, run="random")
        w = np.where(idx >= 0, F32(0.125), F32(-1.0)).astype(F32)
        ops = Operands(values, idx, w, n, d)
        out = HalfOut(n, v)
        assert ops.call(out.ptr()) == 0, ops.error()
        out.check("subnormal")
        ref, _ = S.slice_f16_ref(values, idx, w, n, d)
        assert np.abs(ref).max() < 2.0 ** -14 and np.abs(ref).max() > 0
        worst = max(worst, S.assert_slice_f16(out.numpy(), values, idx, w, n, d, "random", f"subnormal d={d} V={v} step {step}"))
        if step == 8:
            assert np.array_equal(ref.astype(F16).astype(np.float64), ref)
            assert_same_halves(out.numpy(), ref.astype(F16), f"subnormal d={d} V={v}: representable sums")
    print(f"SLICE F16 subnormal d={d} V={v} worst error / bound: forward random {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------ the zero fill
def _zero_fill_sizes():
    out = []
    for d, v, n in ((3, 8, 5), (2, 64, 33)):  # one workgroup with 5 working threads; two, the second with 8
        grid = S.slice_f16_grid(n, v, 8)[1]
        out += [(d, v, n, ze) for ze in (0, 1, grid * 256, grid * 256 + 1)]
    return out + [(3, 8, 5, 100003)]  # one workgroup: 391 trips of the grid-stride loop


@pytest.mark.parametrize("d,v,n,zero_elems", _zero_fill_sizes())
def test_prepare_backward_zero_fills_exactly_its_elements(d, v, n, zero_elems):
    case = S.Case("zero_fill", d, v, n, 0, 0, False)
    values, idx, w = S.make_inputs(case, "random")
    ops = Operands(values, idx, w, n, d)
    plain, out, acc = HalfOut(n, v), HalfOut(n, v), Acc(zero_elems)
    assert ops.call(plain.ptr()) == 0, ops.error()
    assert ops.call(out.ptr(), acc.ptr(), zero_elems) == 0, ops.error()
    what = f"d={d} V={v} n={n} zero_elems={zero_elems}"
    acc.check(what)
    out.check(what)
    assert_same_halves(out.numpy(), plain.numpy(), what)
    S.assert_slice_f16(out.numpy(), values, idx, w, n, d, "random", what)


def test_prepare_backward_without_an_accumulator():
    """A NULL accumulator with zero_elems > 0: nothing to fill, the same rows."""
    case = S.CASES_BY_NAME["d2-V64-n33-work264"]
    values, idx, w = S.make_inputs(case, "random")
    ops = Operands(values, idx, w, case.n, case.d)
    plain, out = HalfOut(case.n, case.v), HalfOut(case.n, case.v)
    assert ops.call(plain.ptr()) == 0, ops.error()
    assert ops.call(out.ptr(), None, 1000) == 0, ops.error()
    out.check("NULL accumulator")
    assert_same_halves(out.numpy(), plain.numpy(), "NULL accumulator")


@pytest.mark.parametrize("zero_elems", [0, 1, 1024, 5001])
@pytest.mark.parametrize("null", [(), ("values", "idx", "w", "out")])
def test_no_point(zero_elems, null):
    """n = 0: LN_OK, `out` untouched, an accumulator zeroed over zero_elems (through ln_zero_async) and not beyond; null operands legal."""
    case = S.CASES_BY_NAME["d3-V8-n256-work256"]
    values, idx, w = S.make_inputs(case, "random")
    ops = Operands(values, idx, w, case.n, case.d)
    out, acc = HalfOut(4, case.v), Acc(zero_elems)
    assert ops.call(out.ptr(), n=0, null=null) == 0, ops.error()
    assert acc.untouched()
    assert ops.call(out.ptr(), acc.ptr(), zero_elems, n=0, null=null) == 0, ops.error()
    acc.check(f"n = 0, zero_elems = {zero_elems}")
    assert ops.call(out.ptr(), None, zero_elems, n=0, null=null) == 0, ops.error()
    assert out.untouched(), "n = 0: out was written"


# ------------------------------------------------------------------------------------------------------------------ refusals
REFUSALS = {
    "V=6": (dict(v=6), S.LN_ERR_UNSUPPORTED), "V=2": (dict(v=2), S.LN_ERR_UNSUPPORTED), "V=0": (dict(v=0), S.LN_ERR_UNSUPPORTED),
    "pos_dim=0": (dict(d=0), S.LN_ERR_UNSUPPORTED), "pos_dim=7": (dict(d=7), S.LN_ERR_UNSUPPORTED),
    "values+2": (dict(off_values=2), S.LN_ERR_ARG), "values+4": (dict(off_values=4), S.LN_ERR_ARG),
    "out+2": (dict(off_out=2), S.LN_ERR_ARG), "out+4": (dict(off_out=4), S.LN_ERR_ARG),
    "null-values": (dict(null=("values",)), S.LN_ERR_ARG), "null-idx": (dict(null=("idx",)), S.LN_ERR_ARG),
    "null-w": (dict(null=("w",)), S.LN_ERR_ARG), "null-out": (dict(null=("out",)), S.LN_ERR_ARG),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_write_nothing(name):
    """Each refusal returns its code with a message that names the entry point, launches nothing and writes no byte of `out` or of the
    accumulator, through both entry points."""
    how, code = REFUSALS[name]
    n, d, v = 100, 3, 64
    case = S.Case("refusal", d, v, n, 0, 0, False)
    values, idx, w = S.make_inputs(case, "random")
    ops = Operands(values, idx, w, n, d, how.get("off_values", 0))
    out, acc = HalfOut(n, v, how.get("off_out", 0)), Acc(n * v)
    kw = dict(v=how.get("v"), d=how.get("d"), null=how.get("null", ()))
    vptr, optr = (0 if "values" in kw["null"] else ops.values_ptr), (0 if "out" in kw["null"] else out.ptr())
    if not set(kw["null"]) & {"idx", "w"}:
        assert S.slice_f16_instance(how.get("d", d), how.get("v", v), vptr, optr, n) == code
    for entry in ("forward", "prepare_backward"):
        extra = (acc.ptr(), n * v) if entry == "prepare_backward" else ()
        rc, count = ops.launches(out.ptr(), *extra, **kw)
        msg = ops.error()
        assert rc == code and count == 0, (name, entry, rc, count)
        assert "ln_slice_forward_f16" in msg, (name, msg)
        assert out.untouched() and acc.untouched(), f"{name} {entry}: a refused call wrote"


# ------------------------------------------------------------------------------------------------------------------ the Python surface
def _real_lattice(d, n, seed):
    """A lattice of d dimensions built from n random positions; (lattice, positions, idx with 5 % of the tokens absent, w)."""
    from lattice_net_amd import Lattice
    rng = np.random.default_rng(seed)
    pos = torch.from_numpy(((rng.random((n, d), dtype=F32) - 0.5) * 3).astype(F32)).to(dev())
    lat = Lattice(sigmas=[0.3] * d, capacity=200000, device=dev())
    lat.begin_splat()
    idx, w = lat.just_create_verts(pos, True)
    idx = idx.clone()
    idx[torch.from_numpy(rng.random(idx.numel()) < 0.05).to(idx.device)] = -1  # vertices the table could not hold read as absent
    return lat, pos, idx, w, rng


@pytest.mark.parametrize("d,v", [(1, 64), (1, 12), (6, 64), (6, 12)])
def test_slice_lattice_at_the_outer_dimensions(d, v):
    """SliceLattice.apply on fp16 values at d = 1 and d = 6 (DP1 = 2 and 7), as test_gpu_surface.py does it for d = 2 .. 5: the forward
    within slice_f16_bound, the fp16 gradient within the bound of an fp32 sum rounded once (test_gpu_reduce_instance.py); twice, so the
    second forward meets the accumulator the first backward left dirty."""
    from lattice_net_amd import SliceLattice
    from tests.test_gpu_reduce_instance import rounded_sum_limit, scatter64
    n = 1000
    lat, pos, idx, w, rng = _real_lattice(d, n, 100 * d + v)
    m = lat.nr_lattice_vertices()
    assert 0 < m <= 5000 * (d + 1)
    vals = torch.tensor(rng.standard_normal((m, v)), dtype=torch.float16, device=dev(), requires_grad=True)
    G = torch.tensor(rng.standard_normal((n, v)), dtype=torch.float16, device=dev())
    idx_np, w_np = idx.cpu().numpy(), w.cpu().numpy()
    vals_np, g_np = vals.detach().cpu().numpy(), G.cpu().numpy()
    gref, gmag = scatter64(g_np.astype(np.float64), idx_np, w_np, m, src_div=d + 1)
    lim = rounded_sum_limit(gref, gmag)
    for trip in range(2):
        what = f"SliceLattice d={d} V={v} trip {trip}"
        vals.grad = None
        lat.set_values(vals.detach())
        out = SliceLattice.apply(vals, lat, pos, idx, w)
        assert out.dtype == torch.float16 and out.shape == (n, v)
        out.backward(G)
        assert vals.grad.dtype == torch.float16 and vals.grad.shape == (m, v)
        fwd = S.assert_slice_f16(out.detach().cpu().numpy(), vals_np, idx_np, w_np, n, d, "random", f"{what} forward")
        err = np.abs(vals.grad.cpu().numpy().astype(np.float64) - gref)
        i = np.unravel_index(int(np.argmax(err / lim)), err.shape)
        assert np.all(err <= lim), f"{what} backward: element {i}: error {err[i]:.3e}, bound {lim[i]:.3e}, ratio {err[i] / lim[i]:.3f}"
        print(f"SLICE F16 {what} worst error / bound: SliceLattice forward {fwd:.3f}, SliceLattice backward {float(np.max(err / lim)):.3f}")


@pytest.mark.parametrize("needs_grad", [False, True])
def test_slice_lattice_refuses_fp16_values_of_width_6(needs_grad):
    """Width 6 is no multiple of 4: a LatticeNetHipError that carries LN_ERR_UNSUPPORTED, nothing launched, the values as they were."""
    from lattice_net_amd import SliceLattice
    from lattice_net_amd._lib import LatticeNetHipError
    _, lib = lib_()
    lat, pos, idx, w, rng = _real_lattice(3, 200, 6)
    m = lat.nr_lattice_vertices()
    vals = torch.tensor(rng.standard_normal((m, 6)), dtype=torch.float16, device=dev(), requires_grad=needs_grad)
    keep = vals.detach().clone()
    lat.set_values(vals.detach())
    installed = lat.values()
    torch.cuda.synchronize()
    assert lib.ln_profile_begin(b"*", 64) == 0
    try:
        with pytest.raises(LatticeNetHipError) as e:
            SliceLattice.apply(vals, lat, pos, idx, w)
    finally:
        torch.cuda.synchronize()
        ms, count = C.c_double(), C.c_int()
        assert lib.ln_profile_end(C.byref(ms), C.byref(count)) == 0
    assert f"code {S.LN_ERR_UNSUPPORTED}" in str(e.value) and "ln_slice_forward_f16" in str(e.value), str(e.value)
    assert count.value == 0, f"{count.value} kernels were launched"
    assert lat.values().data_ptr() == installed.data_ptr() and lat.values().shape == (m, 6) and lat.values().dtype == torch.float16
    assert torch.equal(lat.values().view(torch.int16), keep.view(torch.int16))
