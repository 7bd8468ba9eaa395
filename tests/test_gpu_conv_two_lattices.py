"""The convolution between TWO lattices (coarsen, finefy: mq query rows gather from mn rows of another lattice) against fp64 at every
kernel form, element by element, through the C ABI with synthetic neighbour lists (tests/conv_reference.py) so that the row counts are
chosen: the kernels never see mn, trust the ids, take -1 for a zero row and handle their own row tails, and none of that can go wrong
on a single lattice, where every id is below m, the last slot is the identity and the list is symmetric.

SHAPES: one row per form of csrc/ln_conv_plan.h at the smallest round row counts that reach it (E = 9; none a multiple of 64 or 192:
every form runs a partial last tile).  Which launches a row takes is not written here but asked of the plan itself:
tests/test_conv_plan.py::test_two_lattice_shapes_reach_every_form runs tests/cabi/conv_plan_check.cpp over this table on the CPU.

Conventions of test_gpu_conv_workspace.py: outputs pre-filled with NaN, the workspace exactly the queried size with sentinel bytes
behind it, rc == 0, one synchronize before anything is read."""
import numpy as np
import pytest
import torch

from lattice_net_amd import _lib
from tests import conv_reference as C

pytestmark = pytest.mark.gpu
E = 9
RTOL = 1e-5
SENTINEL = 0xA5
FLIP_WT = 3  # LN_CONV_FLIP_NEIGHBOURS | LN_CONV_TRANSPOSED_FILTER

# (mq, mn, V, F): forward over mq rows V -> F, filter gradient over mq rows, value gradient over mn rows F -> V
SHAPES = [
    (300, 211, 5, 3),        # generic kernels throughout
    (1500, 1100, 16, 32),    # whole bank in LDS; fp32 filter gradient summed inside the value-gradient launch
    (4500, 1200, 32, 32),    # k_conv_forward_b3; bf16x3 filter gradient (32 x 32 blocks) summed inside the value-gradient launch
    (1500, 1100, 64, 64),    # fp32 16-row kernel, slots split 9 ways + sum, both directions
    (4500, 1300, 48, 80),    # fp32 16-row kernel, two chunk widths; generic value gradient
    (4500, 1300, 64, 64),    # bf16x3 16-row kernel, one sub-tile, slots split; 64 x 64 filter-gradient blocks
    (1300, 4500, 64, 64),    # ... as the value gradient
    (7500, 2000, 64, 64),    # bf16x3 16-row kernel, three sub-tiles, slots split
    (18500, 5000, 64, 256),  # three sub-tiles, two 128-column chunks, unsplit; wide value gradient of 64 columns, slots split
    (4500, 1300, 128, 128),  # wide form, slots split 9 ways; 128 x 128 filter-gradient blocks
    (1300, 4500, 128, 128),  # ... as the value gradient
    (4500, 1300, 128, 96),   # split-K pairs, slots split; 32 x 96 blocks
    (4500, 1300, 96, 128),   # 96 x 32 blocks; fp32 value gradient in two chunk widths
    (4500, 1200, 32, 64),    # 32 x 64 blocks
    (1200, 4500, 32, 64),    # bf16x3 16-row value gradient of 32 columns
    (4500, 1300, 64, 32),    # 64 x 32 blocks
    (24400, 6000, 96, 96),   # split-K pairs unsplit (24 400: just above the 127 * 192 rows from which 192-row workgroups fill half the chip)
    (24400, 6000, 128, 64),  # wide form unsplit, 64 columns; bf16x3 16-row value gradient of 128 columns
    (24400, 6000, 128, 128), # wide form unsplit, 128 columns; wide value gradient, slots split 5 ways
]
# the fp16 kernels: matrix cores for these channel counts, the scalar kernels for the 5 -> 3 row
F16_SHAPES = [s for s in SHAPES if (s[2] in (16, 32, 64, 96, 128, 256) and s[3] % 16 == 0) or s[2:] == (5, 3)]


def _id(s):
    return "%dx%d-%dto%d" % s


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rng(shape, k):
    return np.random.default_rng(list(shape) + [k])


def _nan(rows, cols, dtype=torch.float32):
    return torch.full((rows, cols), float("nan"), dtype=dtype, device="cuda")


def _workspace(q):
    return torch.full((q + 4096,), SENTINEL, dtype=torch.uint8, device="cuda")


def _intact(ws, q, what):
    assert bool((ws[q:] == SENTINEL).all()), f"{what}: bytes behind the workspace were written"


def _forward(lib, d_nbr, d_vals, d_W, rows, v, f, flags=0, e=E):
    """launches ln_conv_forward_ws inside exactly its queried workspace; (out, check to run after the synchronize).  `e`: the filter
    extent (tests/test_gpu_conv_filter_extents.py shares these helpers)"""
    q = lib.ln_conv_forward_workspace_bytes(rows, e, v, f)
    ws, out = _workspace(q), _nan(rows, f)
    rc = lib.ln_conv_forward_ws(_lib.ptr(d_nbr), _lib.ptr(d_vals), _lib.ptr(d_W), rows, e, v, f, flags, _lib.ptr(out), _lib.ptr(ws), q, None, None)
    assert rc == 0, lib.ln_last_error_string()
    return out, lambda: _intact(ws, q, "ln_conv_forward_ws")


def _backward(lib, d_q, d_n, d_vals, d_G, d_W, mq, mn, v, f, e=E):
    q = lib.ln_conv_backward_workspace_bytes(mq, mn, e, v, f)
    ws, gv, gw = _workspace(q), _nan(mn, v), _nan(e * v, f)
    rc = lib.ln_conv_backward(_lib.ptr(d_q), _lib.ptr(d_n), _lib.ptr(d_vals), _lib.ptr(d_G), _lib.ptr(d_W), mq, mn, e, v, f, _lib.ptr(gv), _lib.ptr(gw),
                              _lib.ptr(ws), q, None, None)
    assert rc == 0, lib.ln_last_error_string()
    return gw, gv, lambda: _intact(ws, q, "ln_conv_backward")


def _three_products_f32(nbr_q, nbr_n, vals, W, G, shape, e=E):
    """(out, gW, gv) of the library as NumPy arrays"""
    mq, mn, v, f = shape
    lib = _lib.load()
    d_q, d_n, d_vals, d_W, d_G = _dev(nbr_q), _dev(nbr_n), _dev(vals), _dev(W), _dev(G)
    out, ok_f = _forward(lib, d_q, d_vals, d_W, mq, v, f, e=e)
    gw, gv, ok_b = _backward(lib, d_q, d_n, d_vals, d_G, d_W, mq, mn, v, f, e=e)
    torch.cuda.synchronize()
    ok_f(), ok_b()
    return out.cpu().numpy(), gw.cpu().numpy(), gv.cpu().numpy()


def _references(nbr_q, nbr_n, vals, W, G):
    return {"forward": C.forward(nbr_q, vals, W), "grad_filter": C.grad_filter(nbr_q, vals, G), "grad_values": C.grad_values(nbr_n, G, W)}


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_f32_random_operands_within_1e5_of_fp64(shape):
    """Each of the three products is one chained accumulation (ops = 1 of close_terms): every element within 1e-5 of the sum of the
    magnitudes of its terms, rows with a 2^17 spread of exponents."""
    mq, mn, v, f = shape
    rng = _rng(shape, 0)
    nbr_q, nbr_n = C.two_lattice_lists(mq, mn, E, rng)
    vals, W, G = C.operands("random", mq, mn, E, v, f, rng)
    got = dict(zip(("forward", "grad_filter", "grad_values"), _three_products_f32(nbr_q, nbr_n, vals, W, G, shape)))
    refs = _references(nbr_q, nbr_n, vals, W, G)
    shares = {k: C.worst_share(got[k], *refs[k], RTOL) for k in refs}
    print("TWO_LATTICES f32 random %s: worst error / (1e-5 bound): %s" % (_id(shape), " ".join(f"{k} {s:.3g}" for k, s in shares.items())))
    for k in refs:
        C.within(got[k], *refs[k], RTOL, f"{_id(shape)} {k}")


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_f32_integer_operands_bit_for_bit(shape):
    mq, mn, v, f = shape
    rng = _rng(shape, 1)
    nbr_q, nbr_n = C.two_lattice_lists(mq, mn, E, rng)
    vals, W, G = C.operands("exact", mq, mn, E, v, f, rng)
    refs = _references(nbr_q, nbr_n, vals, W, G)
    for k, (ref, bound) in refs.items():
        C.assert_exact_family(bound, what=k)
    got = dict(zip(("forward", "grad_filter", "grad_values"), _three_products_f32(nbr_q, nbr_n, vals, W, G, shape)))
    for k in refs:
        C.exact(got[k], refs[k][0], f"{_id(shape)} {k}")


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_f32_nan_in_row_0_reaches_no_row_that_does_not_name_it(shape):
    """The kernels load row 0 in the place of an absent neighbour and select zero afterwards.  No list names id 0 here and row 0 of the
    gathered operand is NaN (vals for the forward and the filter gradient, G for the value gradient): a form that multiplied by a zero
    weight instead would spread one overflowed vertex to every row with a missing neighbour."""
    mq, mn, v, f = shape
    rng = _rng(shape, 2)
    nbr_q, nbr_n = C.two_lattice_lists(mq, mn, E, rng, row0_unreferenced=True)
    vals, W, G = C.operands("exact", mq, mn, E, v, f, rng)
    refs = _references(nbr_q, nbr_n, vals, W, G)
    for k, (ref, bound) in refs.items():
        C.assert_exact_family(bound, what=k)
    vals_p, G_p = vals.copy(), G.copy()
    vals_p[0], G_p[0] = np.nan, np.nan
    lib = _lib.load()
    d_q, d_n, d_W = _dev(nbr_q), _dev(nbr_n), _dev(W)
    d_vals, d_vals_p, d_G, d_G_p = _dev(vals), _dev(vals_p), _dev(G), _dev(G_p)
    out, ok_f = _forward(lib, d_q, d_vals_p, d_W, mq, v, f)
    gw, _, ok_b = _backward(lib, d_q, d_n, d_vals_p, d_G, d_W, mq, mn, v, f)
    _, gv, ok_b2 = _backward(lib, d_q, d_n, d_vals, d_G_p, d_W, mq, mn, v, f)  # (G[0] = NaN is a term of the filter gradient: not read here)
    torch.cuda.synchronize()
    ok_f(), ok_b(), ok_b2()
    C.exact(out.cpu().numpy(), refs["forward"][0], f"{_id(shape)} forward, vals[0] = NaN")
    C.exact(gw.cpu().numpy(), refs["grad_filter"][0], f"{_id(shape)} grad_filter, vals[0] = NaN")
    C.exact(gv.cpu().numpy(), refs["grad_values"][0], f"{_id(shape)} grad_values, G[0] = NaN")


@pytest.mark.parametrize("family", ["exact", "random"])
@pytest.mark.parametrize("shape", F16_SHAPES, ids=_id)
def test_f16_three_products(shape, family):
    """fp16 operands, fp32 accumulation: forward, value gradient (both flags, over the swapped list) and filter gradient.  The reference
    sees the operands as rounded to fp16.  Forward and value gradient come back in fp16: one rounding of the result, 2^-11 |ref|, on
    top of the fp32 accumulation's 1e-5 bound; the filter gradient comes back in fp32."""
    mq, mn, v, f = shape
    rng = _rng(shape, 3 if family == "exact" else 4)
    nbr_q, nbr_n = C.two_lattice_lists(mq, mn, E, rng)
    vals, W, G = C.operands(family, mq, mn, E, v, f, rng, half=True)
    refs = _references(nbr_q, nbr_n, vals, W, G)
    if family == "exact":
        for k, (ref, bound) in refs.items():
            C.assert_exact_family(bound, ref, half=k != "grad_filter", what=k)
    lib = _lib.load()
    d_q, d_n = _dev(nbr_q), _dev(nbr_n)
    d_vals, d_W, d_G = (_dev(x.astype(np.float16)) for x in (vals, W, G))
    out, gv, gw = _nan(mq, f, torch.float16), _nan(mn, v, torch.float16), _nan(E * v, f)
    q = lib.ln_conv_grad_filter_f16_workspace_bytes(mq, E, v, f)
    ws = _workspace(q)
    rcs = [lib.ln_conv_forward_f16(_lib.ptr(d_q), _lib.ptr(d_vals), _lib.ptr(d_W), mq, E, v, f, 0, _lib.ptr(out), None),
           lib.ln_conv_forward_f16(_lib.ptr(d_n), _lib.ptr(d_G), _lib.ptr(d_W), mn, E, f, v, FLIP_WT, _lib.ptr(gv), None),
           lib.ln_conv_grad_filter_f16(_lib.ptr(d_q), _lib.ptr(d_vals), _lib.ptr(d_G), mq, E, v, f, _lib.ptr(gw), _lib.ptr(ws), q, None)]
    torch.cuda.synchronize()
    assert rcs == [0, 0, 0], lib.ln_last_error_string()
    _intact(ws, q, "ln_conv_grad_filter_f16")
    got = {"forward": out.float().cpu().numpy(), "grad_values": gv.float().cpu().numpy(), "grad_filter": gw.cpu().numpy()}
    if family == "exact":
        for k in refs:
            C.exact(got[k], refs[k][0], f"{_id(shape)} fp16 {k}")
        return
    rel = {"forward": 2.0 ** -11, "grad_values": 2.0 ** -11, "grad_filter": 0.0}
    shares = {k: C.worst_share(got[k], *refs[k], RTOL, rel[k]) for k in refs}
    print("TWO_LATTICES f16 random %s: worst error / allowance: %s" % (_id(shape), " ".join(f"{k} {s:.3g}" for k, s in shares.items())))
    for k in refs:
        C.within(got[k], *refs[k], RTOL, f"{_id(shape)} fp16 {k}", rel=rel[k])


def test_coarsen_then_finefy_between_two_large_levels():
    """32 -> 64 coarsen and 64 -> 32 finefy through autograd on real lattices whose coarse level is above LN_CONV_B3_MIN_ROWS, against
    fp64 through the oracle's neighbour lists: that the lists the library builds between two large levels are the ones its kernels
    are fed is what the synthetic lists above cannot show."""
    from lattice_net_amd import CoarsenLattice, FinefyLattice, Lattice
    from lattice_net_amd.synthetic import cube_cloud
    from oracle import lattice_oracle as O
    from tests.test_gpu_parity import close_terms, oracle_build
    pos_np = cube_cloud(30000, 11)
    pos = _dev(pos_np)
    fine = Lattice(sigmas=[0.05] * 3, capacity=200000, device=torch.device("cuda", 0))
    fine.begin_splat()
    fine.just_create_verts(pos, False)
    fine.set_positions(pos)
    mf = fine.nr_lattice_vertices()
    v, f = 32, 64
    rng = np.random.default_rng(1)
    fv = torch.tensor(rng.standard_normal((mf, v)).astype(np.float32), device="cuda", requires_grad=True)
    W1 = torch.tensor((rng.standard_normal((E * v, f)) / np.sqrt(E * v)).astype(np.float32), device="cuda", requires_grad=True)
    cv, cwrap = CoarsenLattice.apply(fv, fine, W1)
    coarse = cwrap.lattice
    mc = coarse.nr_lattice_vertices()
    assert mc >= 4096 and mf > mc, (mf, mc)
    W2 = torch.tensor((rng.standard_normal((E * f, v)) / np.sqrt(E * f)).astype(np.float32), device="cuda", requires_grad=True)
    up, _ = FinefyLattice.apply(cv, coarse, fine, W2)
    G = torch.tensor(rng.standard_normal((mf, v)).astype(np.float32), device="cuda")
    (up * G).sum().backward()
    tf, _, _, _ = oracle_build(pos_np, 0.05, 200000)
    tc, _, _, _ = oracle_build(pos_np, 0.1, 200000, write=False)
    assert tf.nr_filled == mf and tc.nr_filled == mc
    n_cf = torch.from_numpy(O.neighbour_rows(tc.keys[:mc], tf, 2, 1, 1, False).astype(np.int64))
    n_fc = torch.from_numpy(O.neighbour_rows(tf.keys[:mf], tc, 1, 2, 1, False).astype(np.int64))

    def rowify(vals, nbr, rows_in):
        padded = torch.cat([vals, torch.zeros((1, vals.shape[1]), dtype=vals.dtype)], 0)
        return padded[torch.where(nbr >= 0, nbr, torch.full_like(nbr, rows_in))].reshape(nbr.shape[0], -1)

    def graph(x, w1, w2, g):
        c = rowify(x, n_cf, mf) @ w1
        u = rowify(c, n_fc, mc) @ w2
        (u * g).sum().backward()
        return c.detach().numpy(), u.detach().numpy(), x.grad.numpy(), w1.grad.numpy(), w2.grad.numpy()

    def leaves(absolute):
        ts = [t.detach().cpu().double() for t in (fv, W1, W2)]
        return [(t.abs() if absolute else t).requires_grad_(True) for t in ts]

    ref = graph(*leaves(False), G.cpu().double())
    bound = graph(*leaves(True), G.cpu().double().abs())  # the same two-stage graph on the absolute values of every operand
    got = [t.detach().cpu().numpy() for t in (cv, up, fv.grad, W1.grad, W2.grad)]
    for name, g, r, b, ops in zip(("coarse values", "fine values", "grad values", "grad W1", "grad W2"), got, ref, bound, (1, 2, 2, 2, 2)):
        assert g.shape == r.shape, name
        close_terms(g, r, b, ops=ops)
