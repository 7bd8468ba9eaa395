"""GPU parity tests (run on a real MI355X: `pytest -m gpu`).  Every call goes through the C ABI
(liblatticenet_hip.so via lattice_net_amd.Lattice).  Checkers: the golden vectors produced by the
reference kernels (tests/golden) and the CPU oracle (oracle/lattice_oracle.py).

Bars (BASELINE.json north_star): lattice keys, splat indices and neighbour lists bit-exact; fp32
features within 1e-5 relative.  Outputs whose summation order is fixed (slice, gather, im2row,
row2im, barycentric weights) are additionally required to be bit-exact.
"""
import numpy as np
import pytest
import torch

from oracle import lattice_oracle as O
from tests.point_reference import assert_sc_parameter_gradients
from tests.test_gpu_segment_reduce import assert_reduce_close, row_counts

pytestmark = pytest.mark.gpu

RTOL = 1e-5


def dev():
    return torch.device("cuda", 0)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def N(t):
    return t.detach().cpu().numpy()


def make_lattice(sigma, capacity, d=3):
    from lattice_net_amd import Lattice
    return Lattice(sigmas=[float(sigma)] * d, capacity=int(capacity), device=dev())


def close(a, b, scale=None, rtol=RTOL):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    s = float(np.max(np.abs(b))) if scale is None else scale
    np.testing.assert_allclose(a, b, rtol=rtol, atol=rtol * max(s, 1e-30))


def close_terms(a, ref, bound, rtol=RTOL, ops=1):
    """Per-element form of "1e-5 relative": |a - ref| <= ops * rtol * bound element by element, where bound[i] = the sum of the
    absolute values of the terms that make up element i (what an fp32 evaluation in ANY order can be off by, to first order) and
    `ops` the number of chained accumulations between the inputs and this output."""
    a, ref, bound = (np.asarray(x, np.float64) for x in (a, ref, bound))
    err = np.abs(a - ref)
    lim = ops * rtol * bound + 1e-30
    worst = np.unravel_index(np.argmax(err - lim), err.shape) if err.size else ()
    assert np.all(err <= lim), f"element {worst}: |{a[worst]} - {ref[worst]}| = {err[worst]:.3e} > {lim[worst]:.3e}"


def oracle_build(pos_raw, sigma, cap, write=True):
    d = pos_raw.shape[1]
    pos = O.scale_positions(pos_raw, np.full((d,), sigma, np.float32))
    t = O.OracleHashTable(cap, d)
    idx, w = O.build_splat(t, pos, write)
    return t, pos, idx, w


def test_library_is_the_hip_build():
    import lattice_net_amd as L
    assert b"gfx950" in L.load_library().ln_version()
    assert torch.cuda.is_available()


@pytest.mark.parametrize("name", ["F1_config1", "F2_boundary", "F9_lidar", "F5_distribute", "F6_slice_classify"])
def test_build_indices_weights_keys_bit_exact(golden, name):
    g = golden(name)
    lat = make_lattice(g["sigma"], g["capacity"])
    lat.begin_splat()
    idx, w = lat.just_create_verts(T(g["pos_raw"]), True)
    m = lat.nr_lattice_vertices()
    assert m == int(g["nr_filled"])
    np.testing.assert_array_equal(N(idx), g["idx"])
    np.testing.assert_array_equal(N(w), g["w"])
    if "keys" in g:
        np.testing.assert_array_equal(N(lat.hash_table().m_keys_tensor[:m]), g["keys"])
        assert int(lat.hash_table().m_keys_tensor[m:].abs().sum()) == 0
    assert int(lat.hash_table().m_nr_filled_tensor.item()) == m


def test_f1_splat_slice_gather_and_backwards(golden):
    g = golden("F1_config1")
    from lattice_net_amd import SplatLattice
    lat = make_lattice(g["sigma"], g["capacity"])
    pos = T(g["pos_raw"])
    vals = T(g["vals"])
    n, v = g["vals"].shape
    lv, wrap, idx, w = SplatLattice.apply(lat, pos, vals)
    m = lat.nr_lattice_vertices()
    assert lv.shape[0] == int(g["capacity"])  # splat leaves the table CAP rows tall (HashTable.cu:32)
    np.testing.assert_array_equal(N(idx), g["idx"])
    absacc = np.zeros((m, v), np.float32)  # per element: the sum of |value x weight| over the vertex's tokens
    O.splat_accumulate(absacc, np.abs(g["vals"]), g["idx"], np.abs(g["w"]))
    close_terms(N(lv[:m]), g["values"], absacc)  # accumulation order differs
    assert float(lv[m:].abs().max()) == 0.0
    # from here on use the golden vertex values so downstream comparisons can be bit-exact
    lat.set_values(T(g["values"]))
    sl = lat.slice_standalone_with_precomputation(pos, idx, w)
    np.testing.assert_array_equal(N(sl), g["slice"])
    ga = lat.gather_standalone_with_precomputation(pos, idx, w)
    np.testing.assert_array_equal(N(ga), g["gather"])
    sl2, i2, w2 = lat.slice_standalone_no_precomputation(T(g["qpos_raw"]))
    np.testing.assert_array_equal(N(i2), g["idx_nopre"])
    np.testing.assert_array_equal(N(w2), g["w_nopre"])
    np.testing.assert_array_equal(N(sl2), g["slice_nopre"])
    lat.slice_backwards_standalone_with_precomputation_no_homogeneous(pos, T(g["grad_sliced"]), idx, w)
    close_terms(N(lat.values()), g["slice_bwd"], O.slice_backwards(np.abs(g["grad_sliced"]), g["idx"], np.abs(g["w"]), m))
    lat.gather_backwards_standalone_with_precomputation(pos, T(g["grad_gathered"]), idx, w)
    close_terms(N(lat.values()), g["gather_bwd"], O.gather_backwards(np.abs(g["grad_gathered"]), g["idx"], np.abs(g["w"]), m, 3))


@pytest.mark.parametrize("name,dil,v", [("F1_config1", 1, 4), ("F4_dilation2", 2, 2), ("F9_lidar", 1, 1)])
def test_neighbour_lists_im2row_row2im_bit_exact(golden, name, dil, v):
    g = golden(name)
    lat = make_lattice(g["sigma"], g["capacity"])
    lat.begin_splat()
    lat.just_create_verts(T(g["pos_raw"]), False)
    m = lat.nr_lattice_vertices()
    vals = g["values"] if "values" in g else np.zeros((m, v), np.float32)
    lat.set_values(T(vals))
    E = lat.get_filter_extent(1)
    assert E == 9
    suffix = f"_d{dil}"
    np.testing.assert_array_equal(N(lat.im2rowindices(lat, E, dil, False)), g["im2rowindices" + suffix])
    if "im2row" + suffix in g:
        np.testing.assert_array_equal(N(lat.im2row(lat, E, dil, False)), g["im2row" + suffix])
    if "im2row" + suffix + "_flip" in g:
        np.testing.assert_array_equal(N(lat.im2row(lat, E, dil, True)), g["im2row" + suffix + "_flip"])
    if "row2im" + suffix in g:
        out = lat.row2im(T(g["grad_rowified"]), dil, E, 0, lat)
        np.testing.assert_array_equal(N(out), g["row2im" + suffix])


def test_f3_two_levels(golden):
    g = golden("F3_two_level")
    pos = T(g["pos_raw"])
    fine = make_lattice(g["sigma"], g["capacity"])
    fine.begin_splat()
    fine.splat_standalone(pos, T(g["vals"]))
    mf = fine.nr_lattice_vertices()
    assert mf == int(g["fine_nr"])
    np.testing.assert_array_equal(N(fine.hash_table().m_keys_tensor[:mf]), g["fine_keys"])
    fine.set_values(T(g["fine_values"]))
    coarse = fine.create_coarse_verts_naive(pos)
    mc = coarse.nr_lattice_vertices()
    assert mc == int(g["coarse_nr"]) and coarse.lvl() == 2
    np.testing.assert_array_equal(N(coarse.hash_table().m_keys_tensor[:mc]), g["coarse_keys"])
    kc = fine.create_coarse_verts()
    assert kc.nr_lattice_vertices() == int(g["keycoarse_nr"])
    np.testing.assert_array_equal(N(kc.hash_table().m_keys_tensor[: kc.nr_lattice_vertices()]), g["keycoarse_keys"])
    assert tuple(kc.values().shape) == (kc.nr_lattice_vertices(), 4)
    coarse.set_values(T(g["coarse_values"]))
    for flip in (False, True):
        s = "_flip" if flip else ""
        np.testing.assert_array_equal(N(coarse.im2rowindices(fine, 9, 1, flip)), g["idx_coarse_from_fine" + s])
        np.testing.assert_array_equal(N(coarse.im2row(fine, 9, 1, flip)), g["row_coarse_from_fine" + s])
        np.testing.assert_array_equal(N(fine.im2rowindices(coarse, 9, 1, flip)), g["idx_fine_from_coarse" + s])
        np.testing.assert_array_equal(N(fine.im2row(coarse, 9, 1, flip)), g["row_fine_from_coarse" + s])


def test_f5_distribute(golden):
    g = golden("F5_distribute")
    lat = make_lattice(g["sigma"], g["capacity"])
    lat.begin_splat()
    new, dist, idx, w = lat.distribute(T(g["pos_raw"]), T(g["vals"]), True)
    assert new.nr_lattice_vertices() == int(g["nr_filled"])
    np.testing.assert_array_equal(N(idx), g["idx"])
    np.testing.assert_array_equal(N(w), g["w"])
    np.testing.assert_array_equal(N(dist), g["distributed"])
    assert lat.pos_dim() == 3 and lat.val_dim() == 2


def assert_slice_classify_value_gradient(gv, grad_logits, values, delta_w, lin_w, lin_b, idx, w):
    """The lattice-value gradient element by element against the oracle: the C-term dot product in front of the segment reduce, the
    reduce (tests/test_gpu_segment_reduce.py), and the fp32 rounding of the oracle's result, all against sum |terms|."""
    n, c = grad_logits.shape
    idx, w = N(idx), N(w)
    ref = O.slice_classify_backwards(grad_logits, values, delta_w, lin_w, lin_b, idx, w, n)[0]
    mag = O.slice_classify_backwards(np.abs(grad_logits), values, np.zeros_like(delta_w), np.abs(lin_w), lin_b, idx,
                                     np.abs(w + delta_w.reshape(-1)), n)[0]
    assert_reduce_close(gv, ref, mag, row_counts(idx, ref.shape[0]), what="lattice-value gradient", extra=c + 1)


@pytest.mark.parametrize("v", [64, 32])
def test_f11_slice_classify_kitti_head(golden, v):
    """The wave-tiled kernels (ln_classify.hip: 64-point tiles forward, 16-point MFMA tiles backward; n = 1111 leaves both ragged)
    against the reference's own kernels at the SemanticKITTI head's shape, C = 20: logits bit for bit, gradients 1e-5."""
    g = golden("F11_slice_classify_kitti_head")
    lat = make_lattice(g["sigma"], g["capacity"])
    pos = T(g["pos_raw"])
    lat.begin_splat()
    idx, w = lat.just_create_verts(pos, True)
    np.testing.assert_array_equal(N(idx), g["idx"])
    lat.set_values(T(g[f"lattice_values_{v}"]))
    dw, lw, lb = T(g["delta_w"]), T(g[f"lin_w_{v}"]), T(g[f"lin_b_{v}"])
    logits = lat.slice_classify_with_precomputation(pos, dw, lw, lb, 20, idx, w)
    np.testing.assert_array_equal(N(logits), g[f"logits_{v}"])
    gv = torch.zeros_like(lat.values())
    gdw, glw, glb = torch.zeros_like(dw), torch.zeros_like(lw), torch.zeros_like(lb)
    lat.slice_classify_backwards_with_precomputation(T(g["grad_logits"]), pos, lat.values(), dw, lw, lb, 20, gv, gdw, glw, glb, idx, w)
    close(N(gv), g[f"g_values_{v}"])
    assert_slice_classify_value_gradient(gv, g["grad_logits"], g[f"lattice_values_{v}"], g["delta_w"], g[f"lin_w_{v}"], g[f"lin_b_{v}"], idx, w)
    close(N(gdw), g[f"g_delta_w_{v}"])
    close(N(glw), g[f"g_lin_w_{v}"])
    close(N(glb), g[f"g_lin_b_{v}"])
    assert_sc_parameter_gradients(gdw, glw, glb, g["grad_logits"], g[f"lattice_values_{v}"], g["delta_w"], g[f"lin_w_{v}"], idx, w, 3, what=f"F11 V={v}")


def test_f6_slice_classify(golden):
    g = golden("F6_slice_classify")
    lat = make_lattice(g["sigma"], g["capacity"])
    pos = T(g["pos_raw"])
    lat.begin_splat()
    idx, w = lat.just_create_verts(pos, True)
    lat.set_values(T(g["lattice_values"]))
    dw, lw, lb = T(g["delta_w"]), T(g["lin_w"]), T(g["lin_b"])
    logits = lat.slice_classify_with_precomputation(pos, dw, lw, lb, 5, idx, w)
    np.testing.assert_array_equal(N(logits), g["logits"])
    gv = torch.zeros_like(lat.values())
    gdw, glw, glb = torch.zeros_like(dw), torch.zeros_like(lw), torch.zeros_like(lb)
    lat.slice_classify_backwards_with_precomputation(T(g["grad_logits"]), pos, lat.values(), dw, lw, lb, 5, gv, gdw, glw, glb, idx, w)
    close(N(gv), g["g_values"])
    assert_slice_classify_value_gradient(gv, g["grad_logits"], g["lattice_values"], g["delta_w"], g["lin_w"], g["lin_b"], idx, w)
    close(N(gdw), g["g_delta_w"])
    close(N(glw), g["g_lin_w"])
    close(N(glb), g["g_lin_b"])
    assert_sc_parameter_gradients(gdw, glw, glb, g["grad_logits"], g["lattice_values"], g["delta_w"], g["lin_w"], idx, w, 3, what="F6")


def test_f8_pos_dim_2(golden):
    g = golden("F8_posdim2")
    pos = T(g["pos_raw"])
    fine = make_lattice(g["sigma"], g["capacity"], d=2)
    fine.begin_splat()
    idx, w = fine.splat_standalone(pos, T(g["vals"]))
    mf = fine.nr_lattice_vertices()
    assert mf == int(g["fine_nr"])
    np.testing.assert_array_equal(N(idx), g["idx"])
    np.testing.assert_array_equal(N(w), g["w"])
    np.testing.assert_array_equal(N(fine.hash_table().m_keys_tensor[:mf]), g["fine_keys"])
    fine.set_values(T(g["fine_values"]))
    E = fine.get_filter_extent(1)
    assert E == 7
    np.testing.assert_array_equal(N(fine.im2rowindices(fine, E, 1, False)), g["idx_same"])
    np.testing.assert_array_equal(N(fine.im2row(fine, E, 1, False)), g["row_same"])
    coarse = fine.create_coarse_verts_naive(pos)
    mc = coarse.nr_lattice_vertices()
    np.testing.assert_array_equal(N(coarse.hash_table().m_keys_tensor[:mc]), g["coarse_keys"])
    coarse.set_values(T(g["coarse_values"]))
    np.testing.assert_array_equal(N(coarse.im2rowindices(fine, E, 1, False)), g["idx_coarse_from_fine"])
    np.testing.assert_array_equal(N(fine.im2rowindices(coarse, E, 1, False)), g["idx_fine_from_coarse"])
    np.testing.assert_array_equal(N(fine.im2row(coarse, E, 1, False)), g["row_fine_from_coarse"])


def test_f7_near_full_table_every_vertex_is_inserted(golden):
    """Load 0.97: insertion has no probe cap (HashTableGPU.cuh:443), so numbering must still be canonical."""
    g = golden("F7_near_full")
    lat = make_lattice(g["sigma"], g["capacity"])
    lat.begin_splat()
    idx, w = lat.just_create_verts(T(g["pos_raw"]), True)
    assert lat.nr_lattice_vertices() == int(g["nr_filled"])
    np.testing.assert_array_equal(N(idx), g["idx"])
    np.testing.assert_array_equal(N(lat.hash_table().m_keys_tensor[: int(g["nr_filled"])]), g["keys"])
    # retrieval under the 300-probe cap depends on the (race-dependent) slot layout: only require that
    # a found vertex is the right one
    lat.set_values(T(g["lattice_values"]))
    _, i2, _ = lat.slice_standalone_no_precomputation(T(g["pos_raw"]))
    i2 = N(i2)
    found = i2 >= 0
    np.testing.assert_array_equal(i2[found], g["idx"][found])
    assert found.mean() > 0.5


def test_table_overflow_is_reported():
    from lattice_net_amd import LatticeNetHipError
    from lattice_net_amd.synthetic import cube_cloud
    lat = make_lattice(0.05, 500)
    lat.begin_splat()
    lat.just_create_verts(T(cube_cloud(2000, 1)), False)
    with pytest.raises(LatticeNetHipError, match="overflow"):
        lat.nr_lattice_vertices()


def test_key_range_overflow_is_reported():
    from lattice_net_amd import LatticeNetHipError
    lat = make_lattice(1e-6, 1000)
    lat.begin_splat()
    lat.just_create_verts(T(np.array([[1.0, 2.0, 3.0], [5.0, 5.0, 5.0]], np.float32)), False)
    with pytest.raises(LatticeNetHipError, match="packed"):
        lat.nr_lattice_vertices()


def test_duplicate_points_contention():
    """Every point identical: 4 slots take all the insertions (worst-case atomic contention)."""
    n = 50000
    pos = np.tile(np.array([[0.3, -0.2, 0.7]], np.float32), (n, 1))
    lat = make_lattice(0.5, 1000)
    lat.begin_splat()
    vals = np.ones((n, 2), np.float32)
    idx, w = lat.splat_standalone(T(pos), T(vals))
    assert lat.nr_lattice_vertices() == 4
    idx = N(idx).reshape(n, 4)
    assert np.all(idx == np.arange(4)[None, :])
    wsum = N(w).reshape(n, 4)[0].astype(np.float64)
    close(N(lat.values()[:4, 0]), wsum * n, rtol=2e-3)  # 50k-term fp32 running sums: rounding grows with the count


def test_incremental_build_keeps_existing_rows():
    from lattice_net_amd.synthetic import cube_cloud
    a, b = cube_cloud(700, 3), cube_cloud(900, 4)
    lat = make_lattice(0.2, 40000)
    lat.begin_splat()
    ia, _ = lat.just_create_verts(T(a), True)
    ma = lat.nr_lattice_vertices()
    ib, _ = lat.just_create_verts(T(b), True)
    t = O.OracleHashTable(40000, 3)
    sig = np.full((3,), 0.2, np.float32)
    oa, _ = O.build_splat(t, O.scale_positions(a, sig))
    assert t.nr_filled == ma
    ob, _ = O.build_splat(t, O.scale_positions(b, sig))
    assert lat.nr_lattice_vertices() == t.nr_filled
    np.testing.assert_array_equal(N(ia), oa)
    np.testing.assert_array_equal(N(ib), ob)
    np.testing.assert_array_equal(N(lat.hash_table().m_keys_tensor[: t.nr_filled]), t.keys[: t.nr_filled])


@pytest.mark.parametrize("v,f", [(32, 32), (64, 32), (32, 64), (16, 16), (8, 16), (128, 64), (4, 8), (5, 3), (1, 32),
                                 # the LNN shapes (models.py:125-190 with the SemanticKITTI cfg) and other multiples of 16:
                                 # column-chunked launches of the MFMA kernels
                                 (96, 96), (128, 128), (64, 128), (48, 80), (192, 48), (256, 32), (32, 160)])
def test_conv_forward_and_filter_gradient(v, f):
    from lattice_net_amd.synthetic import cube_cloud
    pos = cube_cloud(3000, 5)
    lat = make_lattice(0.15, 60000)
    lat.begin_splat()
    lat.just_create_verts(T(pos), False)
    m = lat.nr_lattice_vertices()
    rng = np.random.default_rng(v * 100 + f)
    vals = rng.standard_normal((m, v)).astype(np.float32)
    W = (rng.standard_normal((9 * v, f)) / np.sqrt(9 * v)).astype(np.float32)
    G = rng.standard_normal((m, f)).astype(np.float32)
    t, _, _, _ = oracle_build(pos, 0.15, 60000)
    assert t.nr_filled == m
    lat.set_values(T(vals))
    for flip in (False, True):
        nbr = O.neighbour_rows(t.keys[:m], t, 1, 1, 1, flip)
        conv = lat.convolve_im2row_standalone(T(W), 1, lat, flip)
        rows = O.im2row(nbr, vals).astype(np.float64)
        ref = rows @ W.astype(np.float64)
        close_terms(N(conv.values()), ref, np.abs(rows) @ np.abs(W.astype(np.float64)))
        assert conv.val_dim() == f and conv.nr_lattice_vertices() == m
    nbr = O.neighbour_rows(t.keys[:m], t, 1, 1, 1, False)
    rows = O.im2row(nbr, vals).astype(np.float64)
    gf = lat.convolve_im2row_grad_filter(T(G), 1, lat, 9)
    ref = rows.T @ G.astype(np.float64)
    close_terms(N(gf), ref, np.abs(rows).T @ np.abs(G.astype(np.float64)))


@pytest.mark.parametrize("v,f", [(32, 32), (64, 64), (128, 128), (96, 32), (64, 128), (32, 96), (256, 64), (48, 80), (192, 192)])
def test_conv_small_integer_operands_are_exact(v, f):
    """Small-integer values, filter bank and upstream gradient: every product and every partial sum is an integer below 2^24, so
    the convolution, the filter gradient and the value gradient are exact in fp32 whatever the summation order, the slab
    reduction or the operand split (a bf16x3 split of a small integer is the integer) — any difference from the int64 result is
    a wrong operand, not rounding.  Covers the fused 32 x 32 kernels, the per-slot kernels and k_grad_filter_b3."""
    from lattice_net_amd import ConvIm2RowLattice
    from lattice_net_amd.synthetic import cube_cloud
    lat = make_lattice(0.05, 200000)
    lat.begin_splat()
    lat.just_create_verts(T(cube_cloud(30000, 11)), False)
    m = lat.nr_lattice_vertices()
    rng = np.random.default_rng(7 * v + f)
    vals_np = rng.integers(-7, 8, (m, v)).astype(np.float32)
    W_np = rng.integers(-3, 4, (9 * v, f)).astype(np.float32)
    G_np = (rng.integers(-3, 4, (m, f)) * (rng.random((m, 1)) < 0.25)).astype(np.float32)   # 3/4 of the rows carry no gradient
    vals = T(vals_np).requires_grad_(True)
    W = T(W_np).requires_grad_(True)
    out, _ = ConvIm2RowLattice.apply(vals, lat, W, 1)
    (out * T(G_np)).sum().backward()
    lat.set_values(T(vals_np))
    # float64 BLAS products of integers below 2^53 are exact
    rows = N(lat.im2row(lat, 9, 1, False)).astype(np.float64)
    nbr = torch.from_numpy(N(lat.neighbours(lat, 1, False)).astype(np.int64))
    W64, G64 = W_np.astype(np.float64), G_np.astype(np.float64)
    assert np.array_equal(N(out.detach()).astype(np.float64), rows @ W64)
    gw = rows.T @ G64
    assert float(np.max(np.abs(gw))) < 2 ** 24
    assert np.array_equal(N(W.grad).astype(np.float64), gw)
    # value gradient = row2im of G W^T: scatter-add of the per-slot products to the neighbour rows
    gr = torch.from_numpy((G64 @ W64.T).reshape(m, 9, v))
    gx = torch.zeros((m, v), dtype=torch.float64)
    for e in range(9):
        ok = nbr[:, e] >= 0
        gx.index_add_(0, nbr[ok, e], gr[ok, e])
    assert np.array_equal(N(vals.grad).astype(np.float64), gx.numpy())


@pytest.mark.parametrize("lo,hi", [(4096, 16384), (16385, 32768), (32769, 49152)])
def test_fused_32_channel_kernels_exact_at_every_subtile_count(lo, hi):
    """k_conv_forward_b3<T> / k_conv_backward_fused_b3<T> (the headline chain's convolution, V = F = 32) are instantiated for T = 1, 2, 3
    sub-tiles of 64 vertices per workgroup, chosen from the vertex count (ln_bwd_subtiles, rounds of 256 workgroups x (T + 1): <= 16 384 /
    <= 32 768 / above at 256 CUs).
    Small-integer operands: forward, value gradient and filter gradient must equal the float64 (exact) result bit for bit."""
    from lattice_net_amd import ConvIm2RowLattice
    from lattice_net_amd.synthetic import cube_cloud
    pos = T(cube_cloud(30000, 5))
    lat, sigma = None, 0.4
    while sigma > 0.02:                                       # finer lattice -> more vertices: take the first sigma that lands in range
        cand = make_lattice(sigma, 200000)
        cand.begin_splat()
        cand.just_create_verts(pos, False)
        if lo <= cand.nr_lattice_vertices() <= hi:
            lat = cand
            break
        sigma /= 1.12
    assert lat is not None, "no sigma puts the cube cloud's vertex count into the range"
    m, v, f = lat.nr_lattice_vertices(), 32, 32
    rng = np.random.default_rng(m)
    vals_np = rng.integers(-7, 8, (m, v)).astype(np.float32)
    W_np = rng.integers(-3, 4, (9 * v, f)).astype(np.float32)
    G_np = (rng.integers(-3, 4, (m, f)) * (rng.random((m, 1)) < 0.25)).astype(np.float32)
    vals = T(vals_np).requires_grad_(True)
    W = T(W_np).requires_grad_(True)
    out, _ = ConvIm2RowLattice.apply(vals, lat, W, 1)
    (out * T(G_np)).sum().backward()
    lat.set_values(T(vals_np))
    rows = N(lat.im2row(lat, 9, 1, False)).astype(np.float64)
    nbr = torch.from_numpy(N(lat.neighbours(lat, 1, False)).astype(np.int64))
    W64, G64 = W_np.astype(np.float64), G_np.astype(np.float64)
    assert np.array_equal(N(out.detach()).astype(np.float64), rows @ W64)
    assert np.array_equal(N(W.grad).astype(np.float64), rows.T @ G64)
    gr = torch.from_numpy((G64 @ W64.T).reshape(m, 9, v))
    gx = torch.zeros((m, v), dtype=torch.float64)
    for e in range(9):
        ok = nbr[:, e] >= 0
        gx.index_add_(0, nbr[ok, e], gr[ok, e])
    assert np.array_equal(N(vals.grad).astype(np.float64), gx.numpy())


@pytest.mark.parametrize("sigma", [0.05, 0.09])
@pytest.mark.parametrize("v", [32, 64, 96, 128, 160, 192, 256])
def test_conv_one_hot_bank_every_instance(v, sigma):
    """Every instantiation of the per-slot kernels (gathered width v; column chunks of 128 / 64 / 32 / 16 filters; both neighbour
    orders; one and three sub-tiles per workgroup = the two lattice sizes) against a bank with ONE non-zero entry per filter and small-integer values: the result is exact whatever the kernel,
    and a single mis-packed operand half shows as a wrong integer.  (hipcc 7.2 has mis-assigned the operands of the split's
    pack instructions when loop-carried registers were undefined on a path — DESIGN.md §4.3; the random-value tests above see
    that as a 1e-1 error, this one names the channel.)"""
    from lattice_net_amd.synthetic import cube_cloud
    lat = make_lattice(sigma, 200000)
    lat.begin_splat()
    lat.just_create_verts(T(cube_cloud(30000, 11)), False)
    m = lat.nr_lattice_vertices()
    # the bf16x3 per-slot kernel runs with three 64-row sub-tiles per workgroup from (m / 192) x column chunks >= 192 on, with one below
    assert (m >= 36864) if sigma == 0.05 else (4096 <= m <= 36672), m
    rng = np.random.default_rng(v)
    vals = rng.integers(-7, 8, (m, v)).astype(np.float32)
    lat.set_values(T(vals))
    # 16-row kernels: 128 + 64 + 32 + 16 | 64 | 32 + 16 | 16 columns per launch; wide form (k_conv_rows32_b3, from 96 channels and
    # multiples of 32 filters on): 128 + 96 (the 96 on the split-K pairs, k_conv_rows32sk_b3) | 128 + 32 | 96 | 64 | 32
    for f in (240, 64, 48, 16) + ((224, 160, 96, 32) if v >= 96 else ()):
        for flip in (False, True):
            slot = rng.integers(0, 9, f)
            chan = rng.integers(0, v, f)
            gain = rng.integers(1, 4, f).astype(np.float32)
            bank = np.zeros((9, v, f), np.float32)
            bank[slot, chan, np.arange(f)] = gain
            got = N(lat.convolve_im2row_standalone(T(bank.reshape(9 * v, f)), 1, lat, flip).values())
            rows = N(lat.im2row(lat, 9, 1, flip)).reshape(m, 9, v)
            exp = rows[:, slot, chan] * gain[None, :]
            bad = np.argwhere(got != exp)
            assert bad.size == 0, (f, flip, bad[:8].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])


@pytest.mark.parametrize("d,sigma,n,three_subtiles", [(2, 0.008, 60000, True), (4, 0.22, 20000, False), (2, 0.02, 60000, False), (4, 0.1, 20000, True)])
def test_conv_one_hot_bank_other_dimensions(d, sigma, n, three_subtiles):
    """The bf16x3 per-slot kernel takes the filter extent at run time (7 slots for d = 2, 11 for d = 4; neighbour ids staged in LDS for
    E <= 16): large lattices in two and four dimensions, one and three sub-tiles per workgroup, one-hot bank, exact."""
    from lattice_net_amd.synthetic import cube_cloud
    lat = make_lattice(sigma, 400000, d)
    lat.begin_splat()
    lat.just_create_verts(T(cube_cloud(n, 3, d=d)), False)
    m, E = lat.nr_lattice_vertices(), 2 * (d + 1) + 1
    assert (m >= 36864) if three_subtiles else (4096 <= m <= 36672), m
    rng = np.random.default_rng(d)
    for v, f in ((64, 80), (128, 64), (32, 48)):
        vals = rng.integers(-7, 8, (m, v)).astype(np.float32)
        lat.set_values(T(vals))
        for flip in (False, True):
            slot = rng.integers(0, E, f)
            chan = rng.integers(0, v, f)
            gain = rng.integers(1, 4, f).astype(np.float32)
            bank = np.zeros((E, v, f), np.float32)
            bank[slot, chan, np.arange(f)] = gain
            got = N(lat.convolve_im2row_standalone(T(bank.reshape(E * v, f)), 1, lat, flip).values())
            rows = N(lat.im2row(lat, E, 1, flip)).reshape(m, E, v)
            exp = rows[:, slot, chan] * gain[None, :]
            bad = np.argwhere(got != exp)
            assert bad.size == 0, (d, m, v, f, flip, bad[:8].tolist())


@pytest.mark.parametrize("v,f", [(32, 32), (64, 32), (96, 96), (128, 64), (128, 128), (32, 80), (64, 64), (64, 192), (96, 32), (32, 64), (32, 96),
                                 (160, 96), (64, 128), (192, 48), (256, 64)])
def test_conv_large_lattice_split_bf16_path(v, f):
    """Lattices of >= 4096 vertices with a channel count that is a multiple of 32 take the kernels on the bf16 matrix cores with
    exactly 3-way split operands (ln_conv.hip: k_conv_mfma_b3 per slot; k_conv_forward_b3 / k_conv_backward_fused_b3 at V = F = 32);
    same 1e-5 bar against fp64 as the fp32-MFMA kernels, forward (both neighbour orders), filter gradient (per element) and value
    gradient (the flipped, transposed bank)."""
    from lattice_net_amd import ConvIm2RowLattice
    from lattice_net_amd.synthetic import cube_cloud
    pos = cube_cloud(30000, 11)
    lat = make_lattice(0.05, 200000)
    lat.begin_splat()
    lat.just_create_verts(T(pos), False)
    m = lat.nr_lattice_vertices()
    assert m >= 4096
    rng = np.random.default_rng(v + f)
    # values with a wide dynamic range: the split has to be exact for every exponent, not just for N(0, 1)
    vals_np = (rng.standard_normal((m, v)) * np.exp(rng.uniform(-6, 6, (m, 1)))).astype(np.float32)
    W_np = (rng.standard_normal((9 * v, f)) / np.sqrt(9 * v)).astype(np.float32)
    G_np = rng.standard_normal((m, f)).astype(np.float32)
    vals = T(vals_np).requires_grad_(True)
    W = T(W_np).requires_grad_(True)
    lat.set_values(vals.detach())
    rows = N(lat.im2row(lat, 9, 1, False)).astype(np.float64)       # a pure copy by the neighbour list (bit-exact, tested above)
    for flip in (False, True):
        conv = lat.convolve_im2row_standalone(T(W_np), 1, lat, flip)
        r = N(lat.im2row(lat, 9, 1, flip)).astype(np.float64)
        ref = r @ W_np.astype(np.float64)
        scale = np.abs(r) @ np.abs(W_np.astype(np.float64))         # per-element bound of the terms summed
        err = np.abs(N(conv.values()).astype(np.float64) - ref)
        assert np.all(err <= RTOL * np.maximum(scale, 1e-30)), float(np.max(err / np.maximum(scale, 1e-30)))
    out, _ = ConvIm2RowLattice.apply(vals, lat, W, 1)
    (out * T(G_np)).sum().backward()
    ref_gw = rows.T @ G_np.astype(np.float64)
    bound_gw = np.abs(rows).T @ np.abs(G_np.astype(np.float64))
    close(N(W.grad), ref_gw, scale=float(np.max(bound_gw)))
    # per element as well: both dimensions multiples of 64 take the bf16x3 filter-gradient kernel (k_grad_filter_mfma_b3)
    assert np.all(np.abs(N(W.grad).astype(np.float64) - ref_gw) <= RTOL * np.maximum(bound_gw, 1e-30))
    # value gradient = row2im of G W^T: check through the adjoint identity <conv(x), G> = <x, grad_x> for a second x
    x2 = rng.standard_normal((m, v)).astype(np.float32)
    lat.set_values(T(x2))
    r2 = N(lat.im2row(lat, 9, 1, False)).astype(np.float64)
    lhs = float(np.sum((r2 @ W_np.astype(np.float64)) * G_np))
    rhs = float(np.sum(x2.astype(np.float64) * N(vals.grad).astype(np.float64)))
    bound = float(np.sum(np.abs(r2) @ np.abs(W_np.astype(np.float64)) * np.abs(G_np)))
    assert abs(lhs - rhs) <= RTOL * bound


@pytest.mark.parametrize("n_points,subtiles", [(1500, 1), (5000, 2), (12000, 3), (30000, 4), (45000, 5)])
def test_conv_backward_fused_same_lattice(n_points, subtiles):
    """Backward of a same-lattice V = F = 32 convolution: one launch computes both gradients from one gather per (vertex, slot)
    (ln_conv.hip: k_conv_backward_fused, 1..4 sub-tiles of 64 vertices per workgroup, one or more rounds of 256 workgroups).  Checked against fp64 through the explicit im2row matrix, 1e-5 of the per-element sum of magnitudes."""
    from lattice_net_amd import ConvIm2RowLattice
    from lattice_net_amd.synthetic import cube_cloud
    v = f = 32
    lat = make_lattice(0.05, 400000)
    lat.begin_splat()
    pos_np = cube_cloud(n_points, 11)
    lat.just_create_verts(T(pos_np), False)
    m = lat.nr_lattice_vertices()
    assert -(-(-(-m // 64)) // 256) == subtiles, m
    rng = np.random.default_rng(n_points)
    vals_np = rng.standard_normal((m, v)).astype(np.float32)
    W_np = (rng.standard_normal((9 * v, f)) / np.sqrt(9 * v)).astype(np.float32)
    G_np = rng.standard_normal((m, f)).astype(np.float32)
    G_np[rng.random(m) < 0.1] = 0.0
    vals = T(vals_np).requires_grad_(True)
    W = T(W_np).requires_grad_(True)
    out, _ = ConvIm2RowLattice.apply(vals, lat, W, 1)
    out.backward(T(G_np))
    # reference: the ORACLE's table and neighbour list (same canonical numbering), fp64 arithmetic, both gradients per element
    t, _, _, _ = oracle_build(pos_np, 0.05, 400000, write=False)
    assert t.nr_filled == m
    nbr = O.neighbour_rows(t.keys[:m], t, 1, 1, 1, False)
    ok = nbr >= 0
    G64, W64 = G_np.astype(np.float64), W_np.astype(np.float64)
    rows = np.zeros((m, 9, v))
    rows[ok] = vals_np.astype(np.float64)[nbr[ok]]
    rows = rows.reshape(m, 9 * v)
    ref_gw = rows.T @ G64  # lattice_funcs.py:302
    bound_gw = np.abs(rows).T @ np.abs(G64)
    assert np.all(np.abs(N(W.grad) - ref_gw) <= RTOL * np.maximum(bound_gw, 1e-30))
    # grad_values = row2im(G W^T) (LatticeGPU.cuh:2187-2284): the adjoint of the gather, accumulated in fp64
    gr = (G64 @ W64.T).reshape(m, 9, v)
    gr_abs = (np.abs(G64) @ np.abs(W64).T).reshape(m, 9, v)
    ref_gv, bound_gv = np.zeros((m, v)), np.zeros((m, v))
    np.add.at(ref_gv, nbr[ok], gr[ok])
    np.add.at(bound_gv, nbr[ok], gr_abs[ok])
    assert np.all(np.abs(N(vals.grad) - ref_gv) <= RTOL * np.maximum(bound_gv, 1e-30))


@pytest.mark.parametrize("n_points,aggressor", [(5000, "fused"), (12000, "fused"), (45000, "fused"), (12000, "per-slot bf16x3")])
def test_other_streams_unharmed_beside_fused_backward(n_points, aggressor):
    """Two streams: one loops the fused convolution backward, the other the segment reduce of a slice backward on fixed inputs.
    Every result of the reduce must equal its first one.  (The one- / two-sub-tile bf16x3 forms of the fused backward left room
    on their CUs for waves of other kernels, and a segment reduce running there came back with wrong rows in 96 % of the
    iterations, as it did beside the per-slot bf16x3 convolution — tools/probes/pair_probe.py, DESIGN.md §4.4: packed fp32
    instructions of the reduce beside K = 32 matrix instructions; the library is compiled without them now.)"""
    from lattice_net_amd import SplatLattice
    from lattice_net_amd.synthetic import cube_cloud
    v = 32
    rng = np.random.default_rng(n_points)
    W = T((rng.standard_normal((9 * v, v)) / 17).astype(np.float32))
    scans = []
    for seed in (1, 2):
        lat = make_lattice(0.05, 400000)
        pos = T(cube_cloud(n_points, seed))
        _, _, idx, w = SplatLattice.apply(lat, pos, torch.randn((n_points, v), device=dev()))
        m = lat.nr_lattice_vertices()
        lat.neighbours(lat, 1, False)
        scans.append(dict(lat=lat, idx=idx, w=w, m=m, G=torch.randn((m, v), device=dev()), P=torch.randn((n_points, v), device=dev())))
    A, B = scans
    if aggressor != "fused":
        W64 = T((rng.standard_normal((9 * 64, 64)) / 24).astype(np.float32))
        A["lat"].set_values(torch.randn((A["m"], 64), device=dev()))
        assert A["m"] >= 4096  # the bf16x3 gate of the per-slot kernel

    def reduce():
        gv = torch.zeros((B["m"], v), device=dev())
        B["lat"]._scatter_rows(B["P"], B["idx"], B["w"], gv, v, 4, v)
        return gv

    ref = reduce().clone()
    scale = float(ref.abs().max())
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    bad = torch.zeros((), device=dev(), dtype=torch.int64)
    for _ in range(150):
        with torch.cuda.stream(sa):
            if aggressor == "fused":
                A["lat"].convolve_im2row_backward(A["G"], W, 1, None, None)
            else:
                A["lat"].convolve_im2row_standalone(W64, 1, A["lat"], False)
        with torch.cuda.stream(sb):
            bad += ((reduce() - ref).abs().max() / scale > 1e-4).long()
    torch.cuda.synchronize()
    assert int(bad) == 0


@pytest.mark.parametrize("v,f", [(32, 32), (96, 64), (128, 128), (48, 96)])
def test_conv_autograd_matches_dense_reference(v, f):
    """ConvIm2RowLattice fwd+bwd against autograd through the explicit im2row matrix (fp64)."""
    from lattice_net_amd import ConvIm2RowLattice
    from lattice_net_amd.synthetic import cube_cloud
    pos = cube_cloud(2000, 6)
    lat = make_lattice(0.15, 60000)
    lat.begin_splat()
    lat.just_create_verts(T(pos), False)
    m = lat.nr_lattice_vertices()
    rng = np.random.default_rng(0)
    vals = torch.tensor(rng.standard_normal((m, v)).astype(np.float32), device=dev(), requires_grad=True)
    W = torch.tensor((rng.standard_normal((9 * v, f)) / 17).astype(np.float32), device=dev(), requires_grad=True)
    G = torch.tensor(rng.standard_normal((m, f)).astype(np.float32), device=dev())
    out, wrap = ConvIm2RowLattice.apply(vals, lat, W, 1)
    (out * G).sum().backward()
    t, _, _, _ = oracle_build(pos, 0.15, 60000)
    nbr = torch.from_numpy(O.neighbour_rows(t.keys[:m], t, 1, 1, 1, False).astype(np.int64))
    v64 = vals.detach().cpu().double().requires_grad_(True)
    w64 = W.detach().cpu().double().requires_grad_(True)
    padded = torch.cat([v64, torch.zeros((1, v), dtype=torch.float64)], 0)
    rows = padded[torch.where(nbr >= 0, nbr, torch.full_like(nbr, m))].reshape(m, 9 * v)
    ref = rows @ w64
    (ref * G.cpu().double()).sum().backward()
    # per-element bounds: the same graph evaluated on the absolute values of every operand
    va = vals.detach().cpu().double().abs().requires_grad_(True)
    wa = W.detach().cpu().double().abs().requires_grad_(True)
    rows_a = torch.cat([va, torch.zeros((1, v), dtype=torch.float64)], 0)[torch.where(nbr >= 0, nbr, torch.full_like(nbr, m))].reshape(m, 9 * v)
    ref_a = rows_a @ wa
    (ref_a * G.cpu().double().abs()).sum().backward()
    close_terms(N(out), ref.detach().numpy(), ref_a.detach().numpy())
    close_terms(N(vals.grad), v64.grad.numpy(), va.grad.numpy())
    close_terms(N(W.grad), w64.grad.numpy(), wa.grad.numpy())


def test_coarsen_finefy_autograd():
    from lattice_net_amd import CoarsenLattice, FinefyLattice
    from lattice_net_amd.synthetic import cube_cloud
    pos_np = cube_cloud(1500, 7)
    pos = T(pos_np)
    fine = make_lattice(0.2, 30000)
    fine.begin_splat()
    fine.just_create_verts(pos, False)
    fine.set_positions(pos)
    mf = fine.nr_lattice_vertices()
    v, f = 16, 32
    rng = np.random.default_rng(1)
    fv = torch.tensor(rng.standard_normal((mf, v)).astype(np.float32), device=dev(), requires_grad=True)
    W1 = torch.tensor((rng.standard_normal((9 * v, f)) / 12).astype(np.float32), device=dev(), requires_grad=True)
    cv, cwrap = CoarsenLattice.apply(fv, fine, W1)
    coarse = cwrap.lattice
    mc = coarse.nr_lattice_vertices()
    W2 = torch.tensor((rng.standard_normal((9 * f, v)) / 17).astype(np.float32), device=dev(), requires_grad=True)
    up, _ = FinefyLattice.apply(cv, coarse, fine, W2)
    G = torch.tensor(rng.standard_normal((mf, v)).astype(np.float32), device=dev())
    (up * G).sum().backward()
    # fp64 reference through explicit neighbour matrices from the oracle
    tf, _, _, _ = oracle_build(pos_np, 0.2, 30000)
    tc, _, _, _ = oracle_build(pos_np, 0.4, 30000, write=False)
    assert tf.nr_filled == mf and tc.nr_filled == mc
    n_cf = torch.from_numpy(O.neighbour_rows(tc.keys[:mc], tf, 2, 1, 1, False).astype(np.int64))
    n_fc = torch.from_numpy(O.neighbour_rows(tf.keys[:mf], tc, 1, 2, 1, False).astype(np.int64))

    def rowify(vals, nbr, rows_in):
        padded = torch.cat([vals, torch.zeros((1, vals.shape[1]), dtype=vals.dtype)], 0)
        return padded[torch.where(nbr >= 0, nbr, torch.full_like(nbr, rows_in))].reshape(nbr.shape[0], -1)

    fv64 = fv.detach().cpu().double().requires_grad_(True)
    w1 = W1.detach().cpu().double().requires_grad_(True)
    w2 = W2.detach().cpu().double().requires_grad_(True)
    c64 = rowify(fv64, n_cf, mf) @ w1
    u64 = rowify(c64, n_fc, mc) @ w2
    (u64 * G.cpu().double()).sum().backward()
    # per-element bounds: the same two-stage graph on the absolute values of every operand (ops = accumulations chained up to the output)
    fa = fv.detach().cpu().double().abs().requires_grad_(True)
    w1a = W1.detach().cpu().double().abs().requires_grad_(True)
    w2a = W2.detach().cpu().double().abs().requires_grad_(True)
    ca = rowify(fa, n_cf, mf) @ w1a
    ua = rowify(ca, n_fc, mc) @ w2a
    (ua * G.cpu().double().abs()).sum().backward()
    close_terms(N(cv), c64.detach().numpy(), ca.detach().numpy())
    close_terms(N(up), u64.detach().numpy(), ua.detach().numpy(), ops=2)
    close_terms(N(fv.grad), fv64.grad.numpy(), fa.grad.numpy(), ops=2)
    close_terms(N(W1.grad), w1.grad.numpy(), w1a.grad.numpy(), ops=2)
    close_terms(N(W2.grad), w2.grad.numpy(), w2a.grad.numpy(), ops=2)


def test_full_size_c3_scan_against_oracle():
    """BASELINE config C3 at full size: 120k LiDAR-like points, sigma 0.9, capacity 100k."""
    from lattice_net_amd.synthetic import lidar_cloud
    pos_np = lidar_cloud(120000, 0)
    lat = make_lattice(0.9, 100000)
    pos = T(pos_np)
    v = 32
    vals_np = np.random.default_rng(0).standard_normal((120000, v)).astype(np.float32)
    lat.begin_splat()
    idx, w = lat.splat_standalone(pos, T(vals_np))
    m = lat.nr_lattice_vertices()
    t, _, oidx, ow = oracle_build(pos_np, 0.9, 100000)
    assert m == t.nr_filled
    np.testing.assert_array_equal(N(idx), oidx)
    np.testing.assert_array_equal(N(w), ow)
    np.testing.assert_array_equal(N(lat.hash_table().m_keys_tensor[:m]), t.keys[:m])
    ov = np.zeros((m, v), np.float32)
    O.splat_accumulate(ov, vals_np, oidx, ow)
    absacc = np.zeros((m, v), np.float32)
    O.splat_accumulate(absacc, np.abs(vals_np), oidx, ow)
    lv = N(lat.values()[:m])
    assert np.all(np.abs(lv.astype(np.float64) - ov) <= 1e-5 * absacc + 1e-30)
    nbr = O.neighbour_rows(t.keys[:m], t, 1, 1, 1, False)
    lat.set_values(lat.values()[:m].contiguous())
    np.testing.assert_array_equal(N(lat.neighbours(lat, 1, False)), nbr)
    # slice(splat(x)) round trip: size-independent properties
    sl = lat.slice_standalone_with_precomputation(pos, idx, w)
    np.testing.assert_array_equal(N(sl), O.slice_with_precomputation(lv, oidx, ow, 120000))
    _, i2, w2 = lat.slice_standalone_no_precomputation(pos)
    np.testing.assert_array_equal(N(i2), oidx)  # slicing at the splat positions finds the splat vertices
    np.testing.assert_array_equal(N(w2), ow)


@pytest.mark.parametrize("d", [1, 2, 4, 5, 6])
def test_other_position_dimensions_against_oracle(d):
    """pos_dim is a template parameter of the reference kernels (any d); the goldens cover d = 2, 3, the generic
    oracle covers the rest."""
    rng = np.random.default_rng(100 + d)
    n = 1500
    pos_np = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    sigma = 0.5 if d >= 4 else 0.1
    cap = 60000
    lat = make_lattice(sigma, cap, d=d)
    lat.begin_splat()
    vals_np = rng.standard_normal((n, 3)).astype(np.float32)
    idx, w = lat.splat_standalone(T(pos_np), T(vals_np))
    m = lat.nr_lattice_vertices()
    t, _, oidx, ow = oracle_build(pos_np, sigma, cap)
    assert m == t.nr_filled
    np.testing.assert_array_equal(N(idx), oidx)
    np.testing.assert_array_equal(N(w), ow)
    np.testing.assert_array_equal(N(lat.hash_table().m_keys_tensor[:m]), t.keys[:m])
    E = 2 * (d + 1) + 1
    assert lat.get_filter_extent(1) == E
    lat.set_values(lat.values()[:m].contiguous())
    for flip in (False, True):
        np.testing.assert_array_equal(N(lat.neighbours(lat, 1, flip)), O.neighbour_rows(t.keys[:m], t, 1, 1, 1, flip))
    coarse = lat.create_coarse_verts_naive(T(pos_np))
    tc, _, _, _ = oracle_build(pos_np, 2 * sigma, cap, write=False)
    mc = coarse.nr_lattice_vertices()
    assert mc == tc.nr_filled
    coarse.set_values(torch.zeros((mc, 3), device=dev()))
    np.testing.assert_array_equal(N(coarse.neighbours(lat, 1, False)), O.neighbour_rows(tc.keys[:mc], t, 2, 1, 1, False))
    np.testing.assert_array_equal(N(lat.neighbours(coarse, 1, False)), O.neighbour_rows(t.keys[:m], tc, 1, 2, 1, False))
    # generic-shape convolution through the C ABI for this filter extent
    W = (rng.standard_normal((E * 3, 5)) / 4).astype(np.float32)
    conv = lat.convolve_im2row_standalone(T(W), 1, lat, False)
    ov = np.zeros((m, 3), np.float32)
    O.splat_accumulate(ov, vals_np, oidx, ow)
    rows = O.im2row(O.neighbour_rows(t.keys[:m], t, 1, 1, 1, False), N(lat.values())).astype(np.float64)
    ref = rows @ W.astype(np.float64)
    close(N(conv.values()), ref, scale=float(np.max(np.abs(rows) @ np.abs(W.astype(np.float64)))))


def test_build_is_deterministic_across_runs():
    """Canonical numbering: repeated builds of the same cloud give bit-identical indices, keys and neighbour lists
    (the reference's CUDA build numbers vertices by thread arrival order and differs run to run)."""
    from lattice_net_amd.synthetic import lidar_cloud
    pos = T(lidar_cloud(60000, 5))
    ref = None
    for _ in range(8):
        lat = make_lattice(0.9, 100000)
        lat.begin_splat()
        idx, w = lat.just_create_verts(pos, True)
        m = lat.nr_lattice_vertices()
        lat.set_values(torch.zeros((m, 1), device=dev()))
        cur = (N(idx), N(w), N(lat.hash_table().m_keys_tensor[:m]), N(lat.neighbours(lat, 1, False)))
        if ref is None:
            ref = cur
        else:
            for a, b in zip(ref, cur):
                np.testing.assert_array_equal(a, b)


def test_c5_aggregated_scans_size():
    """C5-sized input: 4 aggregated LiDAR-like scans (480k points), capacity 400000, V = 64 (fp32 here)."""
    from lattice_net_amd.synthetic import lidar_cloud
    parts = [lidar_cloud(120000, s) + np.array([3.0 * s, -2.0 * s, 0.0], np.float32) for s in range(4)]
    pos_np = np.ascontiguousarray(np.concatenate(parts, 0))
    lat = make_lattice(0.9, 400000)
    lat.begin_splat()
    vals = torch.randn((pos_np.shape[0], 64), device=dev())
    idx, w = lat.splat_standalone(T(pos_np), vals)
    m = lat.nr_lattice_vertices()
    t, _, oidx, ow = oracle_build(pos_np, 0.9, 400000)
    assert m == t.nr_filled
    np.testing.assert_array_equal(N(idx), oidx)
    np.testing.assert_array_equal(N(w), ow)
    lat.set_values(lat.values()[:m].contiguous())
    W = torch.randn((9 * 64, 64), device=dev()) / 24
    conv = lat.convolve_im2row_standalone(W, 1, lat, False)
    nbr = O.neighbour_rows(t.keys[:m], t, 1, 1, 1, False)
    np.testing.assert_array_equal(N(lat.neighbours(lat, 1, False)), nbr)
    # spot-check 2000 output rows of the 64x64 convolution in fp64
    rng = np.random.default_rng(0)
    pick = rng.choice(m, 2000, replace=False)
    lv = N(lat.values()).astype(np.float64)
    rows = np.zeros((2000, 9, 64))
    for e in range(9):
        ok = nbr[pick, e] >= 0
        rows[ok, e] = lv[nbr[pick[ok], e]]
    ref = rows.reshape(2000, -1) @ N(W).astype(np.float64)
    scale = float(np.max(np.abs(rows.reshape(2000, -1)) @ np.abs(N(W).astype(np.float64))))
    close(N(conv.values())[pick], ref, scale=scale)


@pytest.mark.parametrize("v,f", [(128, 128), (256, 256), (192, 192), (256, 128), (128, 256), (128, 64), (96, 96)])
def test_conv_on_a_mid_size_lattice_wide_form_with_slot_split(v, f):
    """Coarse levels of a U-net (5-30 k rows, 128+ channels): the wide convolution form with the filter slots split over gridDim.z and
    the partial sums added behind it (ln_conv_wide_split).  Forward, flipped forward and both gradients against fp64 with the
    per-element bound, on level 2 of the SemanticKITTI lattice (11.4 k rows)."""
    from lattice_net_amd import ConvIm2RowLattice
    from lattice_net_amd.synthetic import lidar_cloud
    pos_np = lidar_cloud(120000, 0)
    lat = make_lattice(1.8, 100000)  # (sigma doubled: the level-2 lattice of the network, built directly)
    lat.begin_splat()
    lat.just_create_verts(T(pos_np), False)
    m = lat.nr_lattice_vertices()
    assert 8000 < m < 16000
    t, _, _, _ = oracle_build(pos_np, 1.8, 100000, write=False)
    assert t.nr_filled == m
    rng = np.random.default_rng(v + f)
    vals = torch.tensor(rng.standard_normal((m, v)).astype(np.float32), device=dev(), requires_grad=True)
    W = torch.tensor((rng.standard_normal((9 * v, f)) / np.sqrt(9 * v)).astype(np.float32), device=dev(), requires_grad=True)
    G = torch.tensor(rng.standard_normal((m, f)).astype(np.float32), device=dev())
    lat.set_values(vals.detach())
    nbr_np = O.neighbour_rows(t.keys[:m], t, 1, 1, 1, False)
    nbr_f = O.neighbour_rows(t.keys[:m], t, 1, 1, 1, True)
    rows_f = O.im2row(nbr_f, vals.detach().cpu().numpy()).astype(np.float64)
    conv_f = lat.convolve_im2row_standalone(W.detach(), 1, lat, True)
    close_terms(N(conv_f.values()), rows_f @ W.detach().cpu().double().numpy(), np.abs(rows_f) @ np.abs(W.detach().cpu().double().numpy()))
    out, _ = ConvIm2RowLattice.apply(vals, lat, W, 1)
    (out * G).sum().backward()
    nbr = torch.from_numpy(nbr_np.astype(np.int64))

    def graph(v64, w64, g64):
        padded = torch.cat([v64, torch.zeros((1, v), dtype=torch.float64)], 0)
        rows = padded[torch.where(nbr >= 0, nbr, torch.full_like(nbr, m))].reshape(m, 9 * v)
        ref = rows @ w64
        (ref * g64).sum().backward()
        return ref.detach().numpy()
    v64, w64 = vals.detach().cpu().double().requires_grad_(True), W.detach().cpu().double().requires_grad_(True)
    ref = graph(v64, w64, G.cpu().double())
    va, wa = vals.detach().cpu().double().abs().requires_grad_(True), W.detach().cpu().double().abs().requires_grad_(True)
    ref_a = graph(va, wa, G.cpu().double().abs())
    close_terms(N(out), ref, ref_a)
    close_terms(N(vals.grad), v64.grad.numpy(), va.grad.numpy())
    close_terms(N(W.grad), w64.grad.numpy(), wa.grad.numpy())
