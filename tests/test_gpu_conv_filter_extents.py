"""The lattice convolution at filter extents OTHER than 9 against fp64, element by element, at every kernel form such an extent can
take: E = 1 (every bias-free 1 x 1 layer of the network is a convolution over the identity list) and E = 5, 7, 11, 13, 15
(lattices of d = 1, 2, 4, 5, 6), with E = 17 as the first extent whose neighbour ids no longer fit the kernels' LDS staging.
tests/test_gpu_conv_two_lattices.py holds E = 9; its conventions and helpers are the ones used here (C ABI, synthetic lists of
tests/conv_reference.py, outputs pre-filled with NaN, the workspace exactly the queried size with sentinel bytes behind it, rc == 0,
one synchronize before anything is read).

What the extent changes (csrc/ln_conv_plan.h): the slot split's last part holds fewer slots than the others wherever E is no
multiple of e_per; the wide split searches 2..E; the flip e ^ 1 leaves the last slot alone, so at E = 1 it is the identity; the
E == 9-only forms (k_conv_forward_b3, the whole-bank kernel, the bf16x3 filter gradient, both fused backwards) are closed, so every
filter gradient runs k_grad_filter_mfma with gridDim.y = E and every backward is two calls, the slab sum riding in the bank split of
the value-gradient convolution where there is one.

SHAPES: (E, mq, mn, V, F), the smallest round row counts that reach each form (none a multiple of 64 or 192).  Which launches a row
takes is asked of the plan itself: tests/test_conv_plan.py::test_other_extent_shapes_reach_every_form, on the CPU."""
import numpy as np
import pytest
import torch

from lattice_net_amd import _lib
from tests import conv_reference as C
from tests.test_gpu_conv_two_lattices import (FLIP_WT, RTOL, _backward, _dev, _forward, _intact, _nan, _three_products_f32, _workspace)

pytestmark = pytest.mark.gpu
FLIP = 1  # LN_CONV_FLIP_NEIGHBOURS

SHAPES = [
    (1, 300, 211, 5, 3),          # generic kernels throughout, one slot
    (1, 1500, 1100, 64, 64),      # fp32 16-row kernel, unsplit (E < 2); filter gradient's slab sum launched on its own
    (1, 4500, 1300, 96, 96),      # bf16x3 16-row kernel, 64 + 32 columns (a level-1 1 x 1 layer); tile-2 filter gradient
    (1, 1300, 4500, 64, 64),      # ... as the value gradient
    (1, 18500, 5000, 64, 256),    # bf16x3 16-row kernel, three sub-tiles, two 128-column chunks; value gradient of 16-column chunks
    (1, 12300, 3100, 128, 256),   # wide form unsplit (a level-0 1 x 1 layer)
    (5, 300, 211, 5, 3),          # generic kernels throughout
    (5, 18500, 5000, 64, 256),    # three sub-tiles, unsplit; wide value gradient of 64 columns, slots split 5 ways
    (5, 1300, 4500, 128, 128),    # wide value gradient of 128 columns, slots split 5 ways
    (5, 12300, 3100, 128, 224),   # wide form unsplit, 128 columns + split-K pairs unsplit; generic value gradient; tile-2 filter gradient
    (7, 1500, 1100, 16, 32),      # fp32 16-row kernel, slots split 7 ways (the whole-bank kernel's shape at E = 9); tile-1 filter gradient
    (7, 4500, 1200, 32, 32),      # bf16x3 16-row kernel of 32 columns (k_conv_forward_b3's and the fused backward's shape at E = 9)
    (7, 9500, 2100, 64, 64),      # bf16x3, three sub-tiles, 4 splits of 2 slots: the last holds one
    (7, 11500, 3000, 128, 128),   # wide form, 4 splits of 2 slots: the last holds one; fp32 value gradient split the same way
    (11, 1500, 1100, 64, 64),     # fp32 16-row kernel, slots split 11 ways, both directions; tile-4 filter gradient
    (11, 4500, 1300, 64, 64),     # bf16x3, one sub-tile, 6 splits of 2 slots: the last holds one
    (11, 1300, 4500, 64, 64),     # ... as the value gradient
    (11, 12300, 3100, 128, 256),  # wide form unsplit, two 128-column chunks; fp32 value gradient, 3 splits of 4 slots: the last holds three
    (13, 4500, 1300, 48, 80),     # fp32 16-row kernel, two chunk widths, 7 splits of 2 slots: the last holds one; generic value gradient
    (13, 8300, 2100, 16, 256),    # fp32 16-row kernel, unsplit, two 128-column chunks
    (13, 4500, 1300, 128, 128),   # wide form, 7 splits of 2 slots: the last holds one
    (13, 1200, 4500, 32, 64),     # bf16x3 16-row value gradient of 32 columns, 7 splits of 2
    (13, 1300, 4500, 64, 128),    # wide value gradient of 64 columns, 7 splits of 2
    (15, 4500, 1300, 64, 64),     # bf16x3, three sub-tiles, 8 splits of 2 slots: the last holds one
    (17, 4500, 1300, 64, 64),     # ... its twin one slot further: the ids no longer fit LDS, fp32 kernels on both sides
    (15, 4500, 1300, 128, 96),    # split-K pairs, 8 splits of 2 slots: the last holds one
    (15, 1300, 4500, 128, 128),   # wide value gradient, 8 splits of 2
]
# ln_linear_backward (rows, cin, cout) beyond the E = 1 rows above: the grad_w slab sum rides in the grad_x bank split; no bank at all
LINEAR_SHAPES = [(s[1], s[4], s[3]) for s in SHAPES if s[0] == 1] + [(4500, 48, 96), (3001, 48, 192)]
# fp16 kernels: one matrix-core shape and the scalar 5 -> 3 shape per extent
F16_SHAPES = [(5, 1500, 1100, 64, 64), (7, 1500, 1100, 32, 96), (11, 1500, 1100, 96, 32), (15, 1500, 1100, 16, 128)] + [(e, 300, 211, 5, 3) for e in (5, 7, 11, 15)]
PRODUCTS = ("forward", "grad_filter", "grad_values")


def _id(s):
    return "E%d-%dx%d-%dto%d" % s


def _rng(shape, k):
    return np.random.default_rng(list(shape) + [k])


def _lists(shape, rng, row0_unreferenced=False, planted=False):
    """E = 1: a one-column list that is not the identity (a permutation with absent entries; `planted`: the list of every other
    extent, with its repeats of one id)"""
    e, mq, mn = shape[:3]
    if e == 1 and not planted:
        return C.permutation_lists(mq, mn, rng, row0_unreferenced)
    return C.two_lattice_lists(mq, mn, e, rng, row0_unreferenced)


def _references(nbr_q, nbr_n, vals, W, G):
    return {"forward": C.forward(nbr_q, vals, W), "grad_filter": C.grad_filter(nbr_q, vals, G), "grad_values": C.grad_values(nbr_n, G, W)}


def _products(nbr_q, nbr_n, vals, W, G, shape):
    return dict(zip(PRODUCTS, _three_products_f32(nbr_q, nbr_n, vals, W, G, shape[1:], e=shape[0])))


def _forward_flipped_is_the_forward(nbr_q, vals, W, shape, want):
    """E = 1: the flip leaves the last slot alone, so LN_CONV_FLIP_NEIGHBOURS changes no bit"""
    e, mq, _, v, f = shape
    lib = _lib.load()
    out, ok = _forward(lib, _dev(nbr_q), _dev(vals), _dev(W), mq, v, f, flags=FLIP, e=e)
    torch.cuda.synchronize()
    ok()
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{_id(shape)}: the flipped forward differs from the plain one at E = 1"


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_f32_random_operands_within_1e5_of_fp64(shape):
    """Each product is one chained accumulation: every element within 1e-5 of the sum of the magnitudes of its terms, rows with a 2^17
    spread of exponents."""
    e, mq, mn, v, f = shape
    rng = _rng(shape, 0)
    nbr_q, nbr_n = _lists(shape, rng)
    vals, W, G = C.operands("random", mq, mn, e, v, f, rng)
    got = _products(nbr_q, nbr_n, vals, W, G, shape)
    refs = _references(nbr_q, nbr_n, vals, W, G)
    shares = {k: C.worst_share(got[k], *refs[k], RTOL) for k in refs}
    print("FILTER_EXTENTS f32 random %s: worst error / (1e-5 bound): %s" % (_id(shape), " ".join(f"{k} {s:.3g}" for k, s in shares.items())))
    for k in refs:
        C.within(got[k], *refs[k], RTOL, f"{_id(shape)} {k}")
    if e == 1:
        _forward_flipped_is_the_forward(nbr_q, vals, W, shape, got["forward"])


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_f32_integer_operands_bit_for_bit(shape):
    e, mq, mn, v, f = shape
    rng = _rng(shape, 1)
    for planted in ((False, True) if e == 1 else (True,)):
        nbr_q, nbr_n = _lists(shape, rng, planted=planted)
        vals, W, G = C.operands("exact", mq, mn, e, v, f, rng)
        refs = _references(nbr_q, nbr_n, vals, W, G)
        for k, (ref, bound) in refs.items():
            C.assert_exact_family(bound, what=k)
        got = _products(nbr_q, nbr_n, vals, W, G, shape)
        for k in refs:
            C.exact(got[k], refs[k][0], f"{_id(shape)} {k}")
        if e == 1:
            _forward_flipped_is_the_forward(nbr_q, vals, W, shape, got["forward"])


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_f32_nan_in_row_0_reaches_no_row_that_does_not_name_it(shape):
    """No list names id 0 and row 0 of the gathered operand is NaN (vals for the forward and the filter gradient, G for the value
    gradient): the kernels load row 0 in the place of an absent neighbour and must select zero afterwards."""
    e, mq, mn, v, f = shape
    rng = _rng(shape, 2)
    nbr_q, nbr_n = _lists(shape, rng, row0_unreferenced=True)
    vals, W, G = C.operands("exact", mq, mn, e, v, f, rng)
    refs = _references(nbr_q, nbr_n, vals, W, G)
    for k, (ref, bound) in refs.items():
        C.assert_exact_family(bound, what=k)
    vals_p, G_p = vals.copy(), G.copy()
    vals_p[0], G_p[0] = np.nan, np.nan
    lib = _lib.load()
    d_q, d_n, d_W = _dev(nbr_q), _dev(nbr_n), _dev(W)
    d_vals, d_vals_p, d_G, d_G_p = _dev(vals), _dev(vals_p), _dev(G), _dev(G_p)
    out, ok_f = _forward(lib, d_q, d_vals_p, d_W, mq, v, f, e=e)
    gw, _, ok_b = _backward(lib, d_q, d_n, d_vals_p, d_G, d_W, mq, mn, v, f, e=e)
    _, gv, ok_b2 = _backward(lib, d_q, d_n, d_vals, d_G_p, d_W, mq, mn, v, f, e=e)  # (G[0] = NaN is a term of the filter gradient: not read here)
    torch.cuda.synchronize()
    ok_f(), ok_b(), ok_b2()
    C.exact(out.cpu().numpy(), refs["forward"][0], f"{_id(shape)} forward, vals[0] = NaN")
    C.exact(gw.cpu().numpy(), refs["grad_filter"][0], f"{_id(shape)} grad_filter, vals[0] = NaN")
    C.exact(gv.cpu().numpy(), refs["grad_values"][0], f"{_id(shape)} grad_values, G[0] = NaN")


def _linear_backward(lib, d_ident, d_x, d_gy, d_w, rows, cin, cout, with_grad_x=True):
    q = lib.ln_linear_backward_workspace_bytes(rows, cin, cout)
    ws, gx, gw = _workspace(q), _nan(rows, cin), _nan(cout, cin)
    rc = lib.ln_linear_backward(_lib.ptr(d_ident), _lib.ptr(d_x), _lib.ptr(d_gy), _lib.ptr(d_w), rows, cin, cout, _lib.ptr(gx) if with_grad_x else None,
                                _lib.ptr(gw), _lib.ptr(ws), q, None)
    assert rc == 0, lib.ln_last_error_string()
    return gx, gw, lambda: _intact(ws, q, "ln_linear_backward")


@pytest.mark.parametrize("family", ["exact", "random"])
@pytest.mark.parametrize("shape", LINEAR_SHAPES, ids=lambda s: "%dx%dto%d" % s)
def test_linear_backward_over_the_identity_list(shape, family):
    """Both gradients of y = x w^T (w [cout, cin]) as ln_linear_backward computes them: grad_w = grad_y^T x (the filter gradient with
    grad_y as the gathered rows) and grad_x = grad_y w (a plain-bank convolution in whose bank split the slab sum of grad_w rides
    where it has one).  Without grad_x the sum is launched on its own and grad_w must not change by a bit."""
    rows, cin, cout = shape
    rng = _rng(shape, 5 if family == "exact" else 6)
    gy, w, x = C.operands(family, rows, rows, 1, cout, cin, rng)  # (vals [rows, cout], W [cout, cin], G [rows, cin])
    ident = np.arange(rows, dtype=np.int32).reshape(rows, 1)
    refs = {"grad_w": C.grad_filter(ident, gy, x), "grad_x": C.forward(ident, gy, w)}
    if family == "exact":
        for k, (ref, bound) in refs.items():
            C.assert_exact_family(bound, what=k)
    lib = _lib.load()
    d_ident, d_x, d_gy, d_w = _dev(ident), _dev(x), _dev(gy), _dev(w)
    gx, gw, ok = _linear_backward(lib, d_ident, d_x, d_gy, d_w, rows, cin, cout)
    _, gw_alone, ok_alone = _linear_backward(lib, d_ident, d_x, d_gy, d_w, rows, cin, cout, with_grad_x=False)
    torch.cuda.synchronize()
    ok(), ok_alone()
    got = {"grad_w": gw.cpu().numpy(), "grad_x": gx.cpu().numpy()}
    assert np.array_equal(gw_alone.cpu().numpy().view(np.uint32), got["grad_w"].view(np.uint32)), "grad_w depends on whether grad_x is asked for"
    if family == "exact":
        for k in refs:
            C.exact(got[k], refs[k][0], f"{shape} {k}")
        return
    shares = {k: C.worst_share(got[k], *refs[k], RTOL) for k in refs}
    print("FILTER_EXTENTS linear backward %dx%dto%d: worst error / (1e-5 bound): %s" % (shape + (" ".join(f"{k} {s:.3g}" for k, s in shares.items()),)))
    for k in refs:
        C.within(got[k], *refs[k], RTOL, f"{shape} {k}")


@pytest.mark.parametrize("family", ["exact", "random"])
@pytest.mark.parametrize("shape", F16_SHAPES, ids=_id)
def test_f16_three_products(shape, family):
    """fp16 operands, fp32 accumulation, run-time extent (k_conv_mfma_f16; the tiled form is E == 9 only): forward, value gradient
    (both flags, over the swapped list) and filter gradient.  Forward and value gradient come back in fp16: one rounding of the
    result, 2^-11 |ref|, on top of the fp32 accumulation's 1e-5 bound; the filter gradient comes back in fp32."""
    e, mq, mn, v, f = shape
    rng = _rng(shape, 3 if family == "exact" else 4)
    nbr_q, nbr_n = C.two_lattice_lists(mq, mn, e, rng)
    vals, W, G = C.operands(family, mq, mn, e, v, f, rng, half=True)
    refs = _references(nbr_q, nbr_n, vals, W, G)
    if family == "exact":
        for k, (ref, bound) in refs.items():
            C.assert_exact_family(bound, ref, half=k != "grad_filter", what=k)
    lib = _lib.load()
    d_q, d_n = _dev(nbr_q), _dev(nbr_n)
    d_vals, d_W, d_G = (_dev(x.astype(np.float16)) for x in (vals, W, G))
    out, gv, gw = _nan(mq, f, torch.float16), _nan(mn, v, torch.float16), _nan(e * v, f)
    q = lib.ln_conv_grad_filter_f16_workspace_bytes(mq, e, v, f)
    ws = _workspace(q)
    rcs = [lib.ln_conv_forward_f16(_lib.ptr(d_q), _lib.ptr(d_vals), _lib.ptr(d_W), mq, e, v, f, 0, _lib.ptr(out), None),
           lib.ln_conv_forward_f16(_lib.ptr(d_n), _lib.ptr(d_G), _lib.ptr(d_W), mn, e, f, v, FLIP_WT, _lib.ptr(gv), None),
           lib.ln_conv_grad_filter_f16(_lib.ptr(d_q), _lib.ptr(d_vals), _lib.ptr(d_G), mq, e, v, f, _lib.ptr(gw), _lib.ptr(ws), q, None)]
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
    print("FILTER_EXTENTS f16 random %s: worst error / allowance: %s" % (_id(shape), " ".join(f"{k} {s:.3g}" for k, s in shares.items())))
    for k in refs:
        C.within(got[k], *refs[k], RTOL, f"{_id(shape)} fp16 {k}", rel=rel[k])


def test_f16_refuses_a_filter_extent_of_one():
    """The fp16 kernels are built for E >= 3.  At E = 1 both entry points return an error code with a message and launch nothing:
    a refusal, not a silently wrong answer."""
    mq, v, f = 300, 64, 64
    rng = np.random.default_rng(9)
    nbr_q, _ = C.permutation_lists(mq, 211, rng)
    d_q = _dev(nbr_q)
    d_vals, d_W, d_G = (_dev(rng.standard_normal(s).astype(np.float16)) for s in ((211, v), (v, f), (mq, f)))
    lib = _lib.load()
    out, gw = _nan(mq, f, torch.float16), _nan(v, f)
    q = lib.ln_conv_grad_filter_f16_workspace_bytes(mq, 1, v, f)
    ws = _workspace(q)
    rc = lib.ln_conv_forward_f16(_lib.ptr(d_q), _lib.ptr(d_vals), _lib.ptr(d_W), mq, 1, v, f, 0, _lib.ptr(out), None)
    assert rc != 0 and lib.ln_last_error_string(), rc
    rc = lib.ln_conv_grad_filter_f16(_lib.ptr(d_q), _lib.ptr(d_vals), _lib.ptr(d_G), mq, 1, v, f, _lib.ptr(gw), _lib.ptr(ws), q, None)
    assert rc != 0 and lib.ln_last_error_string(), rc
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(gw).all()), "a refused call wrote its output"
    assert bool((ws == 0xA5).all()), "a refused call wrote its workspace"


@pytest.mark.parametrize("d,sigma,n", [(2, 0.02, 60000), (4, 0.22, 20000)])
def test_convolution_on_real_lattices_of_other_dimensions(d, sigma, n):
    """64 -> 64 ConvIm2RowLattice forward + backward through autograd on a d = 2 (E = 7) and a d = 4 (E = 11) lattice above
    LN_CONV_B3_MIN_ROWS, against fp64 through the oracle's neighbour list: that the list the library builds at these extents is the
    one its forward AND its backward are fed is what the synthetic lists above cannot show."""
    from lattice_net_amd import ConvIm2RowLattice, Lattice
    from lattice_net_amd.synthetic import cube_cloud
    from oracle import lattice_oracle as O
    from tests.test_gpu_parity import close_terms, oracle_build
    pos_np = cube_cloud(n, 3, d=d)
    lat = Lattice(sigmas=[float(sigma)] * d, capacity=400000, device=torch.device("cuda", 0))
    lat.begin_splat()
    lat.just_create_verts(_dev(pos_np), False)
    m, e = lat.nr_lattice_vertices(), 2 * (d + 1) + 1
    assert 4096 <= m <= 36672, m
    v = f = 64
    rng = np.random.default_rng(d)
    vals = torch.tensor(rng.standard_normal((m, v)).astype(np.float32), device="cuda", requires_grad=True)
    W = torch.tensor((rng.standard_normal((e * v, f)) / np.sqrt(e * v)).astype(np.float32), device="cuda", requires_grad=True)
    G = torch.tensor(rng.standard_normal((m, f)).astype(np.float32), device="cuda")
    lat.set_values(vals.detach())
    out, _ = ConvIm2RowLattice.apply(vals, lat, W, 1)
    (out * G).sum().backward()
    t, _, _, _ = oracle_build(pos_np, sigma, 400000)
    assert t.nr_filled == m
    nbr = torch.from_numpy(O.neighbour_rows(t.keys[:m], t, 1, 1, 1, False).astype(np.int64))
    assert nbr.shape == (m, e)

    def graph(x, w, g):
        padded = torch.cat([x, torch.zeros((1, x.shape[1]), dtype=x.dtype)], 0)
        o = padded[torch.where(nbr >= 0, nbr, torch.full_like(nbr, m))].reshape(m, -1) @ w
        (o * g).sum().backward()
        return o.detach().numpy(), x.grad.numpy(), w.grad.numpy()

    def leaves(absolute):
        ts = [t_.detach().cpu().double() for t_ in (vals, W)]
        return [(t_.abs() if absolute else t_).requires_grad_(True) for t_ in ts]

    ref = graph(*leaves(False), G.cpu().double())
    bound = graph(*leaves(True), G.cpu().double().abs())  # the same graph on the absolute values of every operand
    got = [t_.detach().cpu().numpy() for t_ in (out, vals.grad, W.grad)]
    for name, g, r, b in zip(("values", "grad values", "grad W"), got, ref, bound):
        assert g.shape == r.shape, name
        close_terms(g, r, b, ops=1)
