"""The fp16 convolution (csrc/ln_conv_f16.hip) against fp64 at every form of its own dispatch (csrc/ln_conv_f16_plan.h), element by
element, through the C ABI with planted neighbour lists (tests/conv_reference.py), in the conventions of test_gpu_conv_two_lattices.py:
mq != mn and no row count a multiple of 64, outputs pre-filled with NaN, the filter-gradient workspace exactly the queried size with
sentinel bytes behind it, rc checked, one synchronize before anything is read.

CASES: one row per form.  Which launches a row takes is not written here but asked of the plan itself:
tests/test_conv_f16_plan.py::test_f16_table_reaches_every_form runs tests/cabi/conv_f16_plan_check.cpp over this table on the CPU
and names any form that no case takes.  Each case runs three products (test_f16_three_products): the forward (flags 0, mq rows,
V -> F), the value gradient (flags 3 over the swapped list, mn rows, F -> V, `grad_out` in the place of `values`) and the filter
gradient (mq rows).  The row counts above 16 384 sit just above the boundaries at which k_conv_f16_tiled takes 2, 3 and 4 sub-tiles
(16 385 / 32 769 / 49 153 rows at 64 gathered channels, 32 769 / 65 537 / 98 305 at 32: asserted in the plan checker)."""
import ctypes

import numpy as np
import pytest
import torch

from lattice_net_amd import _lib
from tests import conv_reference as C
from tests.test_conv_f16_plan import build_checker, f16_plans
from tests.test_gpu_conv_two_lattices import E, FLIP_WT, RTOL, SENTINEL, _dev, _intact, _nan, _references, _rng, _workspace

pytestmark = pytest.mark.gpu
FLIP, TRANSPOSED = 1, 2  # LN_CONV_FLIP_NEIGHBOURS, LN_CONV_TRANSPOSED_FILTER
REL = {"forward": 2.0 ** -11, "grad_values": 2.0 ** -11, "grad_filter": 0.0}  # one rounding of an fp16 result; the filter gradient is fp32

# (mq, mn, V, F, values_off, grad_out_off): byte offsets of the two arrays from 16-byte alignment
CASES = [
    # whole bank in LDS, one sub-tile: the four (V, F) pairs, forward and (swapped) value gradient
    (4500, 1300, 32, 32, 0, 0),
    (4500, 1300, 32, 64, 0, 0),
    (1300, 4500, 64, 32, 0, 0),
    (1500, 1100, 64, 64, 0, 0),
    # 2, 3 and 4 sub-tiles: line-shaped gather (64 channels in) and fragment gather (32 in), each count once as the value gradient
    (16391, 32771, 64, 64, 0, 0),   # forward T = 2 line; value gradient T = 3 line
    (49157, 32773, 64, 32, 0, 0),   # forward T = 4 line; value gradient 32 -> 64 T = 2 fragment
    (65539, 98311, 32, 32, 0, 0),   # forward T = 3 fragment; value gradient T = 4 fragment
    # per-slot kernel: every gathered width as forward and as value gradient, every chunk width at a nonzero column offset
    (1500, 1100, 16, 240, 0, 0),    # K = 16 steps; chunks 8, 4, 2, 1; filter-gradient tiles (1, 4), (1, 2), (1, 1)
    (1100, 1500, 256, 16, 0, 0),    # 256 in, one chunk of 16 columns; value gradient 16 -> 256: two chunks of 128
    (1500, 1100, 128, 256, 0, 0),   # two chunks of 128; value gradient 256 -> 128: two chunks of 64
    (1300, 1100, 256, 112, 0, 0),   # 256 in: chunks 4, 2, 1
    (1500, 1100, 96, 64, 0, 0),     # 96 in; value gradient 64 -> 96
    (1100, 1500, 64, 96, 0, 0),     # 64 in off the tiled shapes; value gradient 96 -> 64
    (1500, 1100, 32, 128, 0, 0),    # 32 in, one chunk of 128; value gradient 128 -> 32
    (1100, 1500, 128, 32, 0, 0),    # value gradient 32 -> 128
    (1500, 1100, 64, 64, 8, 0),     # a tiled shape on the per-slot kernel: `values` 8 bytes off
    # one thread per output element
    (700, 500, 48, 32, 0, 0),       # 48 gathered channels; filter-gradient tiles (2, 2), (1, 2)
    (400, 300, 32, 24, 0, 0),       # columns no multiple of 16; filter-gradient fallback, V F <= 4096
    (500, 400, 64, 64, 2, 0),       # a matrix-core shape with `values` 2 bytes off
    # filter gradient
    (1300, 1100, 112, 112, 0, 0),   # all nine (vt, ft) pairs, every offset nonzero somewhere
    (700, 500, 72, 60, 0, 0),       # fallback, gridDim.z = 2
    (700, 500, 96, 64, 0, 4),       # `grad_out` 4 bytes off: fallback at V F > 4096 (and the value gradient off the per-slot kernel)
]


def _id(c):
    return "%dx%d-%dto%d" % c[:4] + ("-values+%d" % c[4] if c[4] else "") + ("-grad_out+%d" % c[5] if c[5] else "")


def _half_at(a, off=0):
    """the fp16 device copy of `a` at a pointer `off` bytes past 16-byte alignment"""
    assert off % 2 == 0 and 0 <= off < 16
    a = np.ascontiguousarray(a.astype(np.float16))
    buf = torch.zeros((a.size + 8,), dtype=torch.float16, device="cuda")
    t = buf[off // 2:off // 2 + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == off
    return t


def _three_products(case, nbr_q, nbr_n, vals, W, G, G_vg=None):
    """(forward, grad_values, grad_filter) of the library as fp64-comparable NumPy arrays; `G_vg`: what the value gradient gathers,
    where it is not G"""
    mq, mn, v, f, voff, goff = case
    lib = _lib.load()
    d_q, d_n = _dev(nbr_q), _dev(nbr_n)
    d_vals, d_W, d_G = _half_at(vals, voff), _half_at(W), _half_at(G, goff)
    d_G_vg = d_G if G_vg is None else _half_at(G_vg, goff)
    out, gv, gw = _nan(mq, f, torch.float16), _nan(mn, v, torch.float16), _nan(E * v, f)
    q = lib.ln_conv_grad_filter_f16_workspace_bytes(mq, E, v, f)
    ws = _workspace(q)
    rcs = [lib.ln_conv_forward_f16(_lib.ptr(d_q), _lib.ptr(d_vals), _lib.ptr(d_W), mq, E, v, f, 0, _lib.ptr(out), None),
           lib.ln_conv_forward_f16(_lib.ptr(d_n), _lib.ptr(d_G_vg), _lib.ptr(d_W), mn, E, f, v, FLIP_WT, _lib.ptr(gv), None),
           lib.ln_conv_grad_filter_f16(_lib.ptr(d_q), _lib.ptr(d_vals), _lib.ptr(d_G), mq, E, v, f, _lib.ptr(gw), _lib.ptr(ws), q, None)]
    torch.cuda.synchronize()
    assert rcs == [0, 0, 0], lib.ln_last_error_string()
    _intact(ws, q, "ln_conv_grad_filter_f16")
    return {"forward": out.float().cpu().numpy(), "grad_values": gv.float().cpu().numpy(), "grad_filter": gw.cpu().numpy()}


def _exact_operands(case, rng, row0_unreferenced=False):
    mq, mn, v, f = case[:4]
    nbr_q, nbr_n = C.two_lattice_lists(mq, mn, E, rng, row0_unreferenced=row0_unreferenced)
    vals, W, G = C.operands("exact", mq, mn, E, v, f, rng, half=True)
    refs = _references(nbr_q, nbr_n, vals, W, G)
    for k, (ref, bound) in refs.items():  # the reference meets the family's condition before any result is compared with it
        C.assert_exact_family(bound, ref, half=k != "grad_filter", what=k)
    return nbr_q, nbr_n, vals, W, G, refs


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_f16_forms_integer_operands_bit_for_bit(case):
    nbr_q, nbr_n, vals, W, G, refs = _exact_operands(case, _rng(case, 0))
    got = _three_products(case, nbr_q, nbr_n, vals, W, G)
    for k in refs:
        C.exact(got[k], refs[k][0], f"{_id(case)} fp16 {k}")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_f16_forms_random_operands_within_the_fp32_accumulation_bound(case):
    """The reference sees the operands as rounded to fp16.  Every element within 1e-5 of the sum of the magnitudes of its terms (fp32
    accumulation in any order), plus one rounding of the result, 2^-11 |ref|, for the two products that come back in fp16."""
    mq, mn, v, f = case[:4]
    rng = _rng(case, 1)
    nbr_q, nbr_n = C.two_lattice_lists(mq, mn, E, rng)
    vals, W, G = C.operands("random", mq, mn, E, v, f, rng, half=True)
    refs = _references(nbr_q, nbr_n, vals, W, G)
    got = _three_products(case, nbr_q, nbr_n, vals, W, G)
    shares = {k: C.worst_share(got[k], *refs[k], RTOL, REL[k]) for k in refs}
    print("F16_FORMS random %s: worst error / allowance: %s" % (_id(case), " ".join(f"{k} {s:.3g}" for k, s in shares.items())))
    for k in refs:
        C.within(got[k], *refs[k], RTOL, f"{_id(case)} fp16 {k}", rel=REL[k])


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_f16_forms_nan_in_row_0_reaches_no_row_that_does_not_name_it(case):
    """k_conv_f16_tiled loads row 0 in the place of an absent neighbour and selects zero afterwards, in its line-shaped and in its
    fragment-shaped gather.  No list names id 0 here and row 0 of the gathered operand is NaN (vals for the forward and the filter
    gradient, G for the value gradient): a form that multiplied by zero instead would spread one overflowed vertex to every row with
    a missing neighbour."""
    nbr_q, nbr_n, vals, W, G, refs = _exact_operands(case, _rng(case, 2), row0_unreferenced=True)
    vals_p, G_p = vals.copy(), G.copy()
    vals_p[0], G_p[0] = np.nan, np.nan
    got = _three_products(case, nbr_q, nbr_n, vals_p, W, G, G_vg=G_p)  # (G[0] is a term of the filter gradient: left finite there)
    C.exact(got["forward"], refs["forward"][0], f"{_id(case)} forward, vals[0] = NaN")
    C.exact(got["grad_filter"], refs["grad_filter"][0], f"{_id(case)} grad_filter, vals[0] = NaN")
    C.exact(got["grad_values"], refs["grad_values"][0], f"{_id(case)} grad_values, G[0] = NaN")


# ---- the FLIP-only and TRANSPOSED-only instances -----------------------------------------------------------------------------------
SMALL = [(4500, 1300, 64, 32), (4500, 1300, 96, 48)]  # tiled; per-slot (chunks of 32 and 16 columns)


@pytest.mark.parametrize("family", ["exact", "random"])
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "%dx%d-%dto%d" % s)
def test_f16_single_flags(shape, family):
    """flags 1 alone (slots flipped, the bank as given) and flags 2 alone (slots as given, the bank as the per-slot transpose
    [E F, V]): the template instances that neither the forward nor the value gradient of a training step runs."""
    mq, mn, v, f = shape
    rng = _rng(shape, 3 if family == "exact" else 4)
    nbr_q, _ = C.two_lattice_lists(mq, mn, E, rng)
    vals, W, _ = C.operands(family, mq, mn, E, v, f, rng, half=True)
    Wt = np.ascontiguousarray(W.reshape(E, v, f).transpose(0, 2, 1)).reshape(E * f, v)
    refs = {"flip": C.forward(nbr_q, vals, W, flip=True), "transposed": C.forward(nbr_q, vals, Wt, transposed=True)}
    assert not np.array_equal(refs["flip"][0], refs["transposed"][0]) and np.array_equal(refs["transposed"][0], C.forward(nbr_q, vals, W)[0])
    if family == "exact":
        for k, (ref, bound) in refs.items():
            C.assert_exact_family(bound, ref, half=True, what=k)
    lib = _lib.load()
    d_q, d_vals, d_W, d_Wt = _dev(nbr_q), _half_at(vals), _half_at(W), _half_at(Wt)
    outs = {"flip": _nan(mq, f, torch.float16), "transposed": _nan(mq, f, torch.float16)}
    rcs = [lib.ln_conv_forward_f16(_lib.ptr(d_q), _lib.ptr(d_vals), _lib.ptr(d_W), mq, E, v, f, FLIP, _lib.ptr(outs["flip"]), None),
           lib.ln_conv_forward_f16(_lib.ptr(d_q), _lib.ptr(d_vals), _lib.ptr(d_Wt), mq, E, v, f, TRANSPOSED, _lib.ptr(outs["transposed"]), None)]
    torch.cuda.synchronize()
    assert rcs == [0, 0], lib.ln_last_error_string()
    for k, (ref, bound) in refs.items():
        got = outs[k].float().cpu().numpy()
        if family == "exact":
            C.exact(got, ref, f"{shape} flags {k}")
        else:
            print("F16_FORMS %s %s: worst error / allowance %.3g" % (shape, k, C.worst_share(got, ref, bound, RTOL, 2.0 ** -11)))
            C.within(got, ref, bound, RTOL, f"{shape} flags {k}", rel=2.0 ** -11)


# ---- row counts at the edges of the kernels' own tiles -------------------------------------------------------------------------------
INTO = 37   # rows of the gathered lattice in the edge cases
GUARD = 8   # rows of NaN behind an output


@pytest.mark.parametrize("v,f", [(64, 64), (96, 32), (48, 24)], ids=["tiled", "per-slot", "generic"])
def test_f16_forward_row_count_edges(v, f):
    """1 row, and one row either side of the 16 rows of a wave and the 64 rows of a tile: integer operands, bit for bit; the rows behind
    the last one stay as they were."""
    lib = _lib.load()
    launched = []
    for m in (1, 15, 16, 17, 63, 64, 65):
        rng = _rng((m, v, f), 5)
        nbr = C.small_list(m, INTO, E, rng)
        vals, W, _ = C.operands("exact", m, INTO, E, v, f, rng, half=True)
        ref, bound = C.forward(nbr, vals, W)
        C.assert_exact_family(bound, ref, half=True, what="forward")
        out = _nan(m + GUARD, f, torch.float16)
        ins = (_dev(nbr), _half_at(vals), _half_at(W))
        rc = lib.ln_conv_forward_f16(_lib.ptr(ins[0]), _lib.ptr(ins[1]), _lib.ptr(ins[2]), m, E, v, f, 0, _lib.ptr(out), None)
        assert rc == 0, lib.ln_last_error_string()
        launched.append((m, ref, out, ins))
    torch.cuda.synchronize()
    for m, ref, out, _ in launched:
        C.exact(out[:m].float().cpu().numpy(), ref, f"{v}->{f} forward at {m} rows")
        assert bool(torch.isnan(out[m:]).all()), f"{v}->{f} at {m} rows: rows behind the last were written"


@pytest.mark.parametrize("v,f", [(48, 32), (72, 60)], ids=["matrix-core", "fallback"])
def test_f16_filter_gradient_row_count_edges(v, f):
    """1 row, and one row either side of the fallback's 32-row sub-tile, the 64-row sub-tile and the 512-row chunk (one slab / two
    slabs), and 577 = 512 + 64 + 1 rows."""
    lib = _lib.load()
    launched = []
    for m in (1, 31, 32, 33, 63, 64, 65, 511, 512, 513, 577):
        rng = _rng((m, v, f), 6)
        nbr = C.small_list(m, INTO, E, rng)
        vals, _, G = C.operands("exact", m, INTO, E, v, f, rng, half=True)
        ref, bound = C.grad_filter(nbr, vals, G)
        C.assert_exact_family(bound, what="grad_filter")
        q = lib.ln_conv_grad_filter_f16_workspace_bytes(m, E, v, f)
        ws, gw = _workspace(q), _nan(E * v, f)
        ins = (_dev(nbr), _half_at(vals), _half_at(G))
        rc = lib.ln_conv_grad_filter_f16(_lib.ptr(ins[0]), _lib.ptr(ins[1]), _lib.ptr(ins[2]), m, E, v, f, _lib.ptr(gw), _lib.ptr(ws), q, None)
        assert rc == 0, lib.ln_last_error_string()
        launched.append((m, ref, gw, ws, q, ins))
    torch.cuda.synchronize()
    for m, ref, gw, ws, q, _ in launched:
        C.exact(gw.cpu().numpy(), ref, f"{v}x{f} filter gradient at {m} rows")
        _intact(ws, q, f"ln_conv_grad_filter_f16 at {m} rows")


def test_f16_no_rows():
    """m = 0: rc 0; the forward leaves its output as it was, the filter gradient is all zeros"""
    lib = _lib.load()
    v, f = 64, 64
    out, gw = _nan(GUARD, f, torch.float16), _nan(E * v, f)
    d = _half_at(np.ones((GUARD, v), np.float32))
    d_W = _half_at(np.ones((E * v, f), np.float32))
    d_nbr = _dev(np.zeros((GUARD, E), np.int32))
    q = lib.ln_conv_grad_filter_f16_workspace_bytes(0, E, v, f)
    ws = _workspace(q)
    rcs = [lib.ln_conv_forward_f16(_lib.ptr(d_nbr), _lib.ptr(d), _lib.ptr(d_W), 0, E, v, f, 0, _lib.ptr(out), None),
           lib.ln_conv_forward_f16(None, None, None, 0, E, v, f, FLIP_WT, None, None),
           lib.ln_conv_grad_filter_f16(_lib.ptr(d_nbr), _lib.ptr(d), _lib.ptr(d), 0, E, v, f, _lib.ptr(gw), _lib.ptr(ws), q, None)]
    torch.cuda.synchronize()
    assert rcs == [0, 0, 0], lib.ln_last_error_string()
    assert bool(torch.isnan(out).all()) and bool((gw == 0).all())
    assert bool((ws == SENTINEL).all()), "ln_conv_grad_filter_f16 at 0 rows wrote its workspace"


# ---- what is launched ----------------------------------------------------------------------------------------------------------------
def _launches(call):
    """return code of `call()` and the number of kernel launches of the library it made (test_gpu_lovasz.py)"""
    lib = _lib.load()
    assert lib.ln_profile_begin(b"*", 64) == 0
    rc = call()
    ms, count = ctypes.c_double(), ctypes.c_int()
    assert lib.ln_profile_end(ctypes.byref(ms), ctypes.byref(count)) == 0
    return rc, count.value


def test_f16_filter_gradient_refuses_rows_that_do_not_fit_lds():
    """300 x 220 is no matrix-core shape and 32 rows of 300 + 220 floats are more than 64 KB of LDS: LN_ERR_UNSUPPORTED with the sizes
    in the message, nothing launched, nothing written."""
    lib = _lib.load()
    m, v, f = 300, 300, 220
    d_nbr = _dev(np.zeros((m, E), np.int32))
    d_vals, d_G = _half_at(np.ones((m, v), np.float32)), _half_at(np.ones((m, f), np.float32))
    q = lib.ln_conv_grad_filter_f16_workspace_bytes(m, E, v, f)
    ws = torch.full((q + 4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    gw = torch.full((E * v, f), 7.0, device="cuda")
    rc, launches = _launches(lambda: lib.ln_conv_grad_filter_f16(_lib.ptr(d_nbr), _lib.ptr(d_vals), _lib.ptr(d_G), m, E, v, f, _lib.ptr(gw), _lib.ptr(ws),
                                                                 q, None))
    msg = lib.ln_last_error_string()
    assert rc != 0 and launches == 0 and b"ln_conv_grad_filter_f16" in msg, (rc, launches, msg)
    assert all(str(x).encode() in msg for x in (v, f, v + f)), msg
    torch.cuda.synchronize()
    assert bool((gw == 7.0).all()) and bool((ws == SENTINEL).all())


@pytest.fixture(scope="module")
def plan_tool(tmp_path_factory):
    """the plan checker as a plain host program (no sanitizer: those builds run in the CPU tests of test_conv_f16_plan.py)"""
    return build_checker(tmp_path_factory.mktemp("plan_f16_tool"), sanitize=False)


@pytest.mark.parametrize("case", [(16391, 32771, 64, 64, 0, 0), (1500, 1100, 16, 240, 0, 0), (1300, 1100, 112, 112, 0, 0)], ids=_id)
def test_f16_plan_is_what_runs(plan_tool, case):
    """The launches the profile hooks count are the launches the plan lists (a tiled forward, a per-slot forward in four chunks, the
    nine tiles of the 112 x 112 filter gradient and its slab sum): the plan is what ln_conv_f16.hip executes, not a description beside it."""
    assert case in CASES
    mq, mn, v, f, voff, goff = case
    plan = f16_plans(plan_tool, [case], E)[case]
    lib = _lib.load()
    rng = _rng(case, 7)
    nbr_q, nbr_n = C.two_lattice_lists(mq, mn, E, rng)
    vals, W, G = C.operands("exact", mq, mn, E, v, f, rng, half=True)
    d_q, d_n, d_vals, d_W, d_G = _dev(nbr_q), _dev(nbr_n), _half_at(vals, voff), _half_at(W), _half_at(G, goff)
    out, gv, gw = _nan(mq, f, torch.float16), _nan(mn, v, torch.float16), _nan(E * v, f)
    q = lib.ln_conv_grad_filter_f16_workspace_bytes(mq, E, v, f)
    ws = _workspace(q)
    calls = {"FWD": lambda: lib.ln_conv_forward_f16(_lib.ptr(d_q), _lib.ptr(d_vals), _lib.ptr(d_W), mq, E, v, f, 0, _lib.ptr(out), None),
             "VG": lambda: lib.ln_conv_forward_f16(_lib.ptr(d_n), _lib.ptr(d_G), _lib.ptr(d_W), mn, E, f, v, FLIP_WT, _lib.ptr(gv), None),
             "GF": lambda: lib.ln_conv_grad_filter_f16(_lib.ptr(d_q), _lib.ptr(d_vals), _lib.ptr(d_G), mq, E, v, f, _lib.ptr(gw), _lib.ptr(ws), q, None)}
    for k, call in calls.items():
        rc, launches = _launches(call)
        want = plan[k]["launches"] + (1 if k == "GF" else 0)  # (+ the slab sum behind the filter gradient's tiles)
        assert rc == 0 and launches == want, (k, rc, launches, plan[k])
    torch.cuda.synchronize()
    assert plan["FWD"]["launches"] == (4 if v == 16 else 1) and plan["GF"]["launches"] == (9 if v == 112 else 5 if v == 16 else 1)
