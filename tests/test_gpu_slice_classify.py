"""The point-side kernels against fp64, element by element, at every kernel form (`pytest -m gpu`): the fused slice + classifier head
(csrc/ln_classify.hip, the general kernels of csrc/ln_rows.hip behind it), plain slice and gather with their backward scatters.

The C ABI is driven directly (lattice_net_amd._lib) with token arrays from tests/point_reference.py: random rows with ~25 % of the
tokens absent (idx = -1, w = -1), whole points absent, one row named by hundreds of tokens; no hash build.  References, bounds and
their counting arguments live in tests/point_reference.py (checked on the CPU by test_point_reference.py).  Every case runs twice:
- random: logits bit for bit against the ordered fp32 evaluation, the six backward outputs within their counted bounds, element by
  element; the four accumulated outputs (g_values, g_delta_w, g_lin_w, g_lin_b) start from non-zero contents;
- exact: small integers and multiples of 1/8: all six backward outputs equal fp64 bit for bit.
Every output has 64 rows of a sentinel behind it (the workspace: 256 bytes, and the slabs no workgroup owns) that must stay untouched.

Shape -> kernel form (ln_sc_forward_wave, ln_sc_backward_wave, ln_slice_classify_forward, ln_slice_classify_backward; recomputed
from the LDS formulas by point_reference.sc_forward_form / sc_backward_form and asserted in test_point_reference.py):

  forward  wave<DP1, CT>     V % 32 == 0, C <= 32, C V <= 4096, d in {2, 3}, values 16-byte aligned; CT = 4 ceil(C / 4)
           d in {2, 3} x (V, C) in (32, 3) (96, 8) (32, 9) (96, 16) (32, 20) (96, 24) (32, 27) (96, 32): CT = 4 .. 32, 16 / 16 instances
  backward wave<DP1, U, CTL> V % 32 == 0, V <= 128, C <= 32, d in {2, 3}, values and grad_sliced aligned; U = V / 32, CTL = 1 + (C > 16)
           d in {2, 3} x V in {32, 64, 96, 128} x C in {13, 21}: 16 / 16 instances, each at n = 65623 (grid capped at 512 workgroups:
           waves walk three or two tiles, last tile ragged) and n = 69 (waves without a tile)
  general  GENERAL_CASES below: forward v4 PB = 64 / 32 / 16 (all it has), forward scalar PB = 64 / 32 / 16 / 8, backward v4 and scalar
           PB = 64 / 32 / 16 / 8 each: every form is reached.  (V = 512, C = 20 has a forward but no backward: LN_ERR_UNSUPPORTED.)
  mixed    V = 160, C in {8, 24}: wave forward, v4 backward
  misaligned values or grad_sliced (4 bytes off): accepted (ln_check_rows asks for nothing), every float4 kernel steps aside: scalar forms

Each test prints its worst error / bound ratio per output (`pytest -s`); nothing is asserted on that figure."""
import numpy as np
import pytest
import torch

from tests import point_reference as P

pytestmark = pytest.mark.gpu

LN_ERR_UNSUPPORTED = -2
GUARD = P.GUARD_ROWS
WS_GUARD = 256

# (d, V, C, n) -> (forward form, backward form)
GENERAL_CASES = {
    (3, 8, 20, 293): (("v4", 64), ("v4", 64)),
    (4, 32, 13, 293): (("v4", 64), ("v4", 64)),         # d = 4 leaves the wave kernels at V % 32 == 0
    (3, 64, 50, 293): (("v4", 64), ("v4", 64)),         # C = 50 likewise
    (3, 160, 50, 293): (("v4", 32), ("v4", 16)),
    (3, 256, 20, 150): (("v4", 32), ("v4", 16)),
    (3, 256, 40, 150): (("v4", 16), ("v4", 8)),
    (3, 160, 8, 293): (("wave", 8), ("v4", 32)),        # mixed pairing
    (3, 160, 24, 293): (("wave", 24), ("v4", 32)),
    (3, 5, 3, 293): (("scalar", 64), ("scalar", 64)),
    (2, 30, 20, 293): (("scalar", 64), ("scalar", 64)),
    (3, 150, 20, 293): (("scalar", 64), ("scalar", 32)),
    (3, 250, 16, 150): (("scalar", 32), ("scalar", 16)),
    (3, 510, 8, 100): (("scalar", 16), ("scalar", 8)),
    (5, 777, 5, 100): (("scalar", 8), ("scalar", 8)),
    (3, 512, 20, 100): (("scalar", 8), None),           # V % 4 == 0 but no float4 tile fits; the backward has no form for it
    # beyond the grid caps (forward 2048 workgroups, backward 512): the grid-stride walk over several tiles, last tile ragged
    (3, 8, 3, 2048 * 64 + 64 + 5): (("v4", 64), ("v4", 64)),
    (3, 5, 3, 2048 * 64 + 64 + 5): (("scalar", 64), ("scalar", 64)),
    (4, 8, 20, 512 * 64 * 2 + 9): (("v4", 64), ("v4", 64)),
    (3, 5, 3, 512 * 64 * 2 + 9): (("scalar", 64), ("scalar", 64)),
}


def dev():
    return torch.device("cuda", 0)


def lib_():
    from lattice_net_amd import _lib
    return _lib, _lib.load()


class Guarded:
    """A [rows, cols] fp32 device array with GUARD rows of a sentinel behind it (and, with `offset` floats of it in front: a view
    whose pointer is 4 * offset bytes off its 16-byte alignment)."""

    def __init__(self, rows, cols, init=None, offset=0):
        self.n = rows * cols
        self.offset = offset
        self.buf = torch.full((offset + self.n + GUARD * cols,), P.SENTINEL, dtype=torch.float32, device=dev())
        self.t = self.buf[offset:offset + self.n].view(rows, cols)
        if init is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32)).reshape(rows, cols))
        assert self.t.data_ptr() % 16 == (4 * offset) % 16

    def ptr(self):
        return self.t.data_ptr()

    def check(self, what):
        assert bool((self.buf[:self.offset] == P.SENTINEL).all()) and bool((self.buf[self.offset + self.n:] == P.SENTINEL).all()), \
            f"{what}: the sentinel around the array was written"

    def numpy(self):
        return self.t.cpu().numpy()


def gpu(a, offset=0):
    a = np.ascontiguousarray(a)
    if offset == 0:
        return torch.from_numpy(a).to(dev())
    buf = torch.zeros((a.size + 4,), dtype=torch.float32, device=dev())
    t = buf[offset:offset + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    return t


def run_sc(d, v, c, n, exact, misalign=None, seed=0):
    """Forward and backward of one case through the C ABI; returns the worst error / bound ratios."""
    _lib, lib = lib_()
    what = f"d={d} V={v} C={c} n={n} {'exact' if exact else 'random'}" + (f" misaligned {misalign}" if misalign else "")
    m = P.table_rows(n)
    dp1 = d + 1
    inp = P.make_sc_inputs(n, m, d, v, c, seed + 1000 * exact, exact)
    form_b = P.sc_backward_form(d, v, c, aligned=misalign is None)
    st = _lib.stream_ptr(dev())
    values = gpu(inp["values"], offset=1 if misalign == "values" else 0)
    dw, lw, lb, idx, w, gl = (gpu(inp[k]) for k in ("delta_w", "lin_w", "lin_b", "idx", "w", "grad_logits"))
    logits = Guarded(n, c)
    rc = lib.ln_slice_classify_forward(values.data_ptr(), dw.data_ptr(), lw.data_ptr(), lb.data_ptr(), idx.data_ptr(), w.data_ptr(),
                                       n, d, v, c, logits.ptr(), st)
    assert rc == 0, lib.ln_last_error_string()
    P.assert_equal_bits(logits.numpy(), P.sc_forward_reference(inp, n), f"{what} logits")
    logits.check(f"{what} logits")
    out = dict(g_values=Guarded(m, v, inp["g_values0"]), g_delta_w=Guarded(n, dp1, inp["g_delta_w0"]), g_lin_w=Guarded(c, v, inp["g_lin_w0"]),
               g_lin_b=Guarded(c, 1, inp["g_lin_b0"]), grad_sliced=Guarded(n, v, offset=1 if misalign == "grad_sliced" else 0),
               w_eff=Guarded(n * dp1, 1))
    ws_bytes = lib.ln_slice_classify_backward_workspace_bytes(n, d, v, c)
    ws = torch.full((ws_bytes + WS_GUARD,), 0xA5, dtype=torch.uint8, device=dev())
    rc = lib.ln_slice_classify_backward(gl.data_ptr(), values.data_ptr(), dw.data_ptr(), lw.data_ptr(), idx.data_ptr(), w.data_ptr(), n, d, v, c,
                                        out["g_values"].ptr(), out["g_delta_w"].ptr(), out["g_lin_w"].ptr(), out["g_lin_b"].ptr(),
                                        out["grad_sliced"].ptr(), out["w_eff"].ptr(), ws.data_ptr(), ws_bytes, st)
    torch.cuda.synchronize()
    if form_b is None:
        assert rc == LN_ERR_UNSUPPORTED, (what, rc)
        for k in ("g_values", "g_delta_w", "g_lin_w", "g_lin_b"):
            P.assert_equal_bits(out[k].numpy().reshape(-1), inp[k + "0"].reshape(-1), f"{what} {k} after a refused call")
        return {}
    assert rc == 0, lib.ln_last_error_string()
    ref, mag, bound = P.sc_backward_reference(inp, n, d, form_b)
    if exact:
        P.assert_exact_representable(mag, what)
    ratios = P.assert_sc_backward({k: o.numpy() for k, o in out.items()}, ref, bound, exact, what)
    for k, o in out.items():
        o.check(f"{what} {k}")
    used = 4 * P.sc_backward_grid(n, form_b) * (c * v + c) if n else 0
    assert bool((ws[used:] == 0xA5).all()), f"{what}: the workspace was written beyond the slabs of the launched workgroups"
    return ratios


def both_runs(d, v, c, n, misalign=None):
    r = run_sc(d, v, c, n, False, misalign)
    run_sc(d, v, c, n, True, misalign)
    print(f"d={d} V={v} C={c} n={n} forms {P.sc_forward_form(d, v, c, misalign != 'values')} / {P.sc_backward_form(d, v, c, misalign is None)}"
          " worst error / bound: " + ", ".join(f"{k} {x:.3f}" for k, x in r.items()))


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


@pytest.mark.parametrize("d,v,c,n", list(GENERAL_CASES), ids=[f"d{d}-V{v}-C{c}-n{n}" for d, v, c, n in GENERAL_CASES])
def test_general_kernel_forms(d, v, c, n):
    assert (P.sc_forward_form(d, v, c), P.sc_backward_form(d, v, c)) == GENERAL_CASES[(d, v, c, n)]
    both_runs(d, v, c, n)


@pytest.mark.parametrize("which", ["values", "grad_sliced"])
@pytest.mark.parametrize("d,v,c", [(3, 32, 13), (2, 96, 20)])
def test_misaligned_pointers_take_the_scalar_kernels(which, d, v, c):
    """ln_check_rows and the header ask for no alignment and the dispatch steps from the wave kernels over the float4 kernels to the
    scalar ones when `values` (forward and backward) or `grad_sliced` (backward) is not 16-byte aligned: the call is accepted and
    meets the bounds of the scalar form."""
    assert P.sc_backward_form(d, v, c, aligned=False)[0] == "scalar" and P.sc_forward_form(d, v, c, aligned=False)[0] == "scalar"
    both_runs(d, v, c, 293, misalign=which)


@pytest.mark.parametrize("d,v,c", [(3, 32, 13), (2, 128, 21), (3, 8, 20), (3, 5, 3), (3, 160, 24)])
@pytest.mark.parametrize("n", [0, 1])
def test_one_point_and_no_point(d, v, c, n):
    both_runs(d, v, c, n)


# ------------------------------------------------------------------------------------------------------------------ slice / gather
@pytest.mark.parametrize("v", [1, 3, 4, 8, 33, 64])
@pytest.mark.parametrize("d", [2, 3, 5])
@pytest.mark.parametrize("n", [517, 1, 0])
def test_slice_and_gather(d, v, n):
    """ln_slice_forward, ln_slice_forward_prepare_backward, ln_slice_backward, ln_gather_forward, ln_gather_backward on the absent-token
    inputs: forwards bit for bit against the ordered fp32 form, backwards within (1 + tokens of the row) * 2^-24 * magnitude onto
    non-zero contents, and bit for bit on the integer run."""
    _lib, lib = lib_()
    st = _lib.stream_ptr(dev())
    m = P.table_rows(n)
    dp1 = d + 1
    worst = {}
    for exact in (False, True):
        what = f"d={d} V={v} n={n} {'exact' if exact else 'random'}"
        rng = np.random.default_rng(v * 7 + d + exact)
        idx_np, w_np = P.make_tokens(n, m, d, seed=v + d, exact=exact)

        def draw(*shape):
            return (rng.integers(-3, 4, shape) if exact else rng.standard_normal(shape)).astype(np.float32)
        vals_np, gs_np, gg_np, old_np = draw(m, v), draw(n, 1, v), draw(n, dp1, v + 1), draw(m, v)
        vals, idx, w = gpu(vals_np), gpu(idx_np), gpu(w_np)
        # slice forward, alone and with the accumulator of its backward zeroed on the way
        want = P.slice_forward_reference(vals_np, idx_np, w_np, n)
        out = Guarded(n, v)
        assert lib.ln_slice_forward(vals.data_ptr(), idx.data_ptr(), w.data_ptr(), n, d, v, out.ptr(), st) == 0, lib.ln_last_error_string()
        P.assert_equal_bits(out.numpy(), want, f"{what} slice")
        out.check(f"{what} slice")
        out, acc = Guarded(n, v), Guarded(m, v, old_np)
        rc = lib.ln_slice_forward_prepare_backward(vals.data_ptr(), idx.data_ptr(), w.data_ptr(), n, d, v, out.ptr(), acc.ptr(), m * v, st)
        assert rc == 0, lib.ln_last_error_string()
        P.assert_equal_bits(out.numpy(), want, f"{what} slice (prepare_backward)")
        P.assert_equal_bits(acc.numpy(), np.zeros((m, v), np.float32), f"{what} zeroed accumulator")
        out.check(f"{what} slice (prepare_backward)")
        acc.check(f"{what} accumulator: only grad_accumulator_elems floats are zeroed")
        # gather forward
        out = Guarded(n, dp1 * (v + 1))
        assert lib.ln_gather_forward(vals.data_ptr(), idx.data_ptr(), w.data_ptr(), n, d, v, out.ptr(), st) == 0, lib.ln_last_error_string()
        P.assert_equal_bits(out.numpy(), P.gather_forward_reference(vals_np, idx_np, w_np, n).reshape(n, dp1 * (v + 1)), f"{what} gather")
        out.check(f"{what} gather")
        # the two scatters
        for name, fn, g_np in (("slice_backward", lib.ln_slice_backward, gs_np), ("gather_backward", lib.ln_gather_backward, gg_np)):
            acc = Guarded(m, v, old_np)
            g = gpu(g_np)
            assert fn(g.data_ptr(), idx.data_ptr(), w.data_ptr(), n, d, v, acc.ptr(), st) == 0, lib.ln_last_error_string()
            ref, bound, mag = P.scatter_backward_reference(g_np[:, :, :v], idx_np, w_np, dp1, old_np)
            if exact:
                P.assert_exact_representable({name: mag}, what)
                bad = acc.numpy().astype(np.float64) != ref
                assert not bad.any(), f"{what} {name}: {int(bad.sum())} elements differ from the fp64 result"
            else:
                P.assert_within(acc.numpy(), ref, bound, f"{what} {name}")
                worst[name] = P.worst_ratio(acc.numpy(), ref, bound)
            acc.check(f"{what} {name}")
    print(f"d={d} V={v} n={n} worst error / bound: " + ", ".join(f"{k} {x:.3f}" for k, x in worst.items()))
