"""LN_CONV_OVERLAPPED: under the hint the fused 32-channel convolutions (V = F = 32, E = 9, d = 3) run as narrow workgroups of
256 T threads that walk C consecutive chunks of 64 T rows behind one staging of the split filter bank (ln_conv.hip:
k_conv_forward_b3_rows<T, C>, k_conv_backward_fused_b3_rows<T, C>; the shape is ln_conv_plan.h's LN_CONV_OVL_T / LN_CONV_OVL_C).  Per row the
arithmetic is that of the whole-CU forms, so the forward output and the value gradient must not change by a bit; only the grouping of
rows into filter-gradient slabs changes, so the filter gradient is held to fp64 with the bound of the other convolution tests.

Row counts: the smallest that reach the bf16x3 forms (LN_CONV_B3_MIN_ROWS = 4096) around one multiple of the 64 T C rows a workgroup
covers — the multiple, the multiple +- 1, a last workgroup with fewer than C chunks, a last chunk with a partial sub-tile, and the
minimum itself.  The lists are the first m rows of one lattice built from a synthetic cloud, neighbours beyond m marked absent (which
keeps the list symmetric, as the fused backward needs it)."""
import numpy as np
import pytest
import torch

from lattice_net_amd import _lib
from tests.test_gpu_parity import T as to_dev, close_terms, dev, make_lattice

pytestmark = pytest.mark.gpu

OVL_T, OVL_C, OVL_MAX_ROWS = 2, 2, 98304  # the instance the library ships and the row count it is taken up to (tests/test_conv_plan_overlapped.py
                                          # holds these against the plan header)
TILE = 64 * OVL_T              # rows of a chunk
UNIT = TILE * OVL_C            # rows of a workgroup
BASE = (4096 // UNIT + 1) * UNIT  # first multiple above LN_CONV_B3_MIN_ROWS (so that BASE - 1 still takes the narrow form)
# the minimum; the multiple and +- 1; a last workgroup with fewer than C chunks (one, C - 1); a last chunk with a partial sub-tile (as the
# only chunk of its workgroup, behind a full chunk, behind full sub-tiles of its own chunk)
ROW_COUNTS = list(dict.fromkeys([4096, BASE, BASE - 1, BASE + 1, BASE + TILE, BASE + UNIT - TILE, BASE + 17, BASE + TILE + 17, BASE + UNIT - 47]))
E, V, F = 9, 32, 32
SENTINEL = 1234.5


@pytest.fixture(scope="module")
def lattice_rows():
    """One lattice from a small cube cloud: its neighbour list (device, int32 [m, 9]) and row count."""
    from lattice_net_amd.synthetic import cube_cloud
    lat = make_lattice(0.05, 100000)
    lat.begin_splat()
    lat.just_create_verts(to_dev(cube_cloud(3500, 7)), False)
    m = lat.nr_lattice_vertices()
    assert m >= max(ROW_COUNTS), m
    nbr = lat.neighbours(lat, 1, False)[:m].contiguous()
    return nbr, m


_cases = {}


def case(lattice_rows, m):
    """Inputs of row count m, and what the unflagged library computes from them (computed once, shared by the tests)."""
    if m in _cases:
        return _cases[m]
    nbr_full, _ = lattice_rows
    nbr = nbr_full[:m].clone()
    nbr[nbr >= m] = -1
    assert int((nbr[:, :E - 1] < 0).sum()) > m // 10, "the list should have absent neighbours"
    g = torch.Generator(device="cpu").manual_seed(m)
    vals = torch.randn((m, V), generator=g).to(dev())
    W = (torch.randn((E * V, F), generator=g) / np.sqrt(E * V)).to(dev())
    G = torch.randn((m, F), generator=g)
    G[torch.rand((m,), generator=g) < 0.1] = 0.0
    G = G.to(dev())
    # a row partition as a build leaves it (first row of each of the 8 regions, then the row count), regions of unequal sizes
    cuts = np.array([0, 0.05, 0.2, 0.3, 0.55, 0.6, 0.8, 0.95, 1.0]) * m
    part = torch.tensor(cuts.astype(np.int32), dtype=torch.int32, device=dev())
    c = dict(m=m, nbr=nbr, vals=vals, W=W, G=G, part=part)
    c["off"] = {p: run(c, 0, c["part"] if p else None) for p in (False, True)}
    _cases[m] = c
    return c


def run(c, flags, part):
    """Forward and fused backward through the C ABI with sentinels behind every output: (out, grad_values, grad_filter)"""
    lib = _lib.load()
    m = c["m"]
    out_buf = torch.full((m * F + 4096,), SENTINEL, device=dev())
    gv_buf = torch.full((m * V + 4096,), SENTINEL, device=dev())
    wsb = int(lib.ln_conv_backward_workspace_bytes(m, m, E, V, F))
    ws = torch.full((wsb + 65536,), 0xA5, dtype=torch.uint8, device=dev())
    gw = torch.full((E * V, F), SENTINEL, device=dev())
    torch.cuda.synchronize()
    _lib.check(lib.ln_conv_forward_ws(_lib.ptr(c["nbr"]), _lib.ptr(c["vals"]), _lib.ptr(c["W"]), m, E, V, F, flags, _lib.ptr(out_buf), None, 0,
                                      _lib.ptr(part), None), "ln_conv_forward_ws")
    _lib.check(lib.ln_conv_backward_flags(_lib.ptr(c["nbr"]), _lib.ptr(c["nbr"]), _lib.ptr(c["vals"]), _lib.ptr(c["G"]), _lib.ptr(c["W"]), m, m, E,
                                          V, F, flags, _lib.ptr(gv_buf), _lib.ptr(gw), _lib.ptr(ws), wsb, _lib.ptr(part), None),
               "ln_conv_backward_flags")
    torch.cuda.synchronize()
    assert bool((out_buf[m * F:] == SENTINEL).all()), "the forward wrote behind `out`"
    assert bool((gv_buf[m * V:] == SENTINEL).all()), "the backward wrote behind `grad_values`"
    assert bool((ws[wsb:] == 0xA5).all()), "the backward wrote behind the slab workspace"
    return out_buf[:m * F].view(m, F).clone(), gv_buf[:m * V].view(m, V).clone(), gw


@pytest.mark.parametrize("with_partition", [False, True])
@pytest.mark.parametrize("m", ROW_COUNTS)
def test_flag_changes_no_bit_of_output_and_value_gradient(lattice_rows, m, with_partition):
    c = case(lattice_rows, m)
    out0, gv0, _ = c["off"][with_partition]
    out1, gv1, _ = run(c, _lib.LN_CONV_OVERLAPPED, c["part"] if with_partition else None)
    assert torch.equal(out0.view(torch.int32), out1.view(torch.int32))
    assert torch.equal(gv0.view(torch.int32), gv1.view(torch.int32))
    assert float(out0.abs().max()) > 0 and float(gv0.abs().max()) > 0


@pytest.mark.parametrize("with_partition", [False, True])
@pytest.mark.parametrize("m", ROW_COUNTS)
def test_filter_gradient_against_fp64_and_run_to_run(lattice_rows, m, with_partition):
    c = case(lattice_rows, m)
    part = c["part"] if with_partition else None
    _, _, gw1 = run(c, _lib.LN_CONV_OVERLAPPED, part)
    _, _, gw2 = run(c, _lib.LN_CONV_OVERLAPPED, part)
    assert torch.equal(gw1.view(torch.int32), gw2.view(torch.int32)), "two runs on the same inputs differ"
    # fp64 gather-GEMM on the same neighbour list: grad_filter = im2row(values)^T @ grad_out
    nbr = c["nbr"].long()
    rows = c["vals"].double()[nbr.clamp(min=0)] * (nbr >= 0).unsqueeze(-1)
    rows = rows.reshape(m, E * V)
    G64 = c["G"].double()
    ref = rows.T @ G64
    bound = rows.abs().T @ G64.abs()
    close_terms(gw1.cpu().numpy(), ref.cpu().numpy(), bound.cpu().numpy())


@pytest.mark.parametrize("n_points", [5000, 12000, 45000])
def test_other_streams_unharmed_beside_narrow_fused_backward(n_points):
    """tests/test_gpu_parity.py::test_other_streams_unharmed_beside_fused_backward with several scans declared in flight: the narrow
    forms leave room on their CUs for waves of other kernels, the situation that test guards (packed fp32 instructions of a segment
    reduce beside K = 32 matrix instructions).  Every result of the reduce must equal its first one."""
    from lattice_net_amd import SplatLattice, lattice
    from lattice_net_amd.synthetic import cube_cloud
    v = 32
    rng = np.random.default_rng(n_points)
    W = to_dev((rng.standard_normal((9 * v, v)) / 17).astype(np.float32))
    scans = []
    for seed in (1, 2):
        lat = make_lattice(0.05, 400000)
        pos = to_dev(cube_cloud(n_points, seed))
        _, _, idx, w = SplatLattice.apply(lat, pos, torch.randn((n_points, v), device=dev()))
        m = lat.nr_lattice_vertices()
        lat.neighbours(lat, 1, False)
        scans.append(dict(lat=lat, idx=idx, w=w, m=m, G=torch.randn((m, v), device=dev()), P=torch.randn((n_points, v), device=dev())))
    A, B = scans
    assert 4096 <= A["m"] <= OVL_MAX_ROWS  # the rows at which the plan takes the narrow form

    def reduce():
        gv = torch.zeros((B["m"], v), device=dev())
        B["lat"]._scatter_rows(B["P"], B["idx"], B["w"], gv, v, 4, v)
        return gv

    ref = reduce().clone()
    scale = float(ref.abs().max())
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    bad = torch.zeros((), device=dev(), dtype=torch.int64)
    prev = lattice.set_scans_in_flight(4)
    try:
        for _ in range(150):
            with torch.cuda.stream(sa):
                A["lat"].convolve_im2row_backward(A["G"], W, 1, None, None)
            with torch.cuda.stream(sb):
                bad += ((reduce() - ref).abs().max() / scale > 1e-4).long()
        torch.cuda.synchronize()
    finally:
        lattice.set_scans_in_flight(prev)
    assert int(bad) == 0
