"""Cloud batches of unequal sizes (Lattice.set_cloud_batch([...]), LnTableClouds.batch_point_starts) on the device (`pytest -m gpu`): every
cloud of the batch against a build / run of that cloud alone.

Lengths (300, 173, 41) at d = 3: the cloud boundary at point 300 lies inside the second 256-point group of the key pass, so the binary
search on the starts takes both sides within one workgroup and one wave.  Lengths (1, 0, 64, 65): a one-point cloud, an empty cloud and a
boundary on a wave's edge.  Structure comparisons are integer- or bit-exact; the bound of the value comparisons is the project's 1e-4 of
the largest magnitude (tests/test_gpu_lnn_cloud_batch.py)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIG = [0.9, 0.9, 0.9]
CAP = 20000
BOUND = 1e-4
LENGTHS = [(300, 173, 41), (1, 0, 64, 65)]


def dev():
    return torch.device("cuda", 0)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def starts_of(lengths):
    return [0] + [int(x) for x in np.cumsum(lengths)]


def clouds_of(lengths, seed=5):
    """Cloud-major positions: cloud c is (2 + 0.7 c) wide, so that the clouds have different lattices."""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-1.0, 1.0, (n, 3)) * (2.0 + 0.7 * c) for c, n in enumerate(lengths)]).astype(np.float32)


def lattice(batch=None, **kw):
    from lattice_net_amd import Lattice
    lat = Lattice(sigmas=SIG, capacity=CAP, device=dev())
    if batch is not None:
        lat.set_cloud_batch(batch, **kw)
    return lat


@pytest.fixture
def deterministic_mode():
    from lattice_net_amd import lattice as L
    prev = L.set_deterministic(True)  # (canonical rows: the suite's conftest)
    yield
    L.set_deterministic(prev)


def bits(t):
    return t.contiguous().view(torch.int32)


def keys_of(lat):
    return lat.m_hash_table.m_keys_tensor[:lat.nr_lattice_vertices()].clone()


def build_by(how, lat, pos):
    """(lattice that holds the vertices, idx, w) of one of the three builds from positions."""
    if how == "just_create_verts":
        idx, w = lat.just_create_verts(pos, True)
        return lat, idx, w
    vals = torch.ones((pos.shape[0], 1), device=dev())
    if how == "splat":
        idx, w = lat.splat_standalone(pos, vals)
        return lat, idx, w
    new, _, idx, w = lat.distribute(pos, vals)
    return new, idx, w


def assert_cloud_is_the_single_build(batch_lat, idx, w, single, b, s, e, row_starts, key_step, d=3):
    """Cloud b (points [s, e)) of the batch against `single` = (lattice, idx, w) of the cloud built alone; row_starts on the host."""
    r0, r1 = row_starts[b], row_starts[b + 1]
    if single is None:  # the empty cloud
        assert r0 == r1
        return 0
    slat, sidx, sw = single
    m = slat.nr_lattice_vertices()
    assert r1 - r0 == m, (b, r0, r1, m)
    tok = slice(s * (d + 1), e * (d + 1))
    assert torch.equal(idx[tok] - r0, sidx), f"splat indices of cloud {b}"
    assert torch.equal(bits(w[tok]), bits(sw)), f"barycentric weights of cloud {b}"
    k = keys_of(batch_lat)[r0:r1].clone()
    k[:, 0] -= b * key_step
    assert torch.equal(k, keys_of(slat)), f"keys of cloud {b}"
    nb = batch_lat.neighbours(batch_lat, 1, False)[r0:r1]
    nb = torch.where(nb >= 0, nb - r0, nb)
    assert torch.equal(nb, slat.neighbours(slat, 1, False)[:m]), f"neighbour lists of cloud {b}"
    return m


@pytest.mark.parametrize("how", ["splat", "distribute", "just_create_verts"])
@pytest.mark.parametrize("lengths", LENGTHS)
def test_build_is_every_cloud_built_alone(lengths, how):
    pos = T(clouds_of(lengths))
    st = starts_of(lengths)
    lat, idx, w = build_by(how, lattice(list(lengths)), pos)
    total = lat.nr_lattice_vertices()
    rows = lat.cloud_row_starts().tolist()
    step = lat.m_hash_table._batch[1]
    assert lat.cloud_lengths() == list(lengths) and len(rows) == len(lengths) + 1 and rows[0] == 0 and rows[-1] == total
    assert lat.cloud_row_order_flag().tolist() == [0]
    counted = 0
    for b, n in enumerate(lengths):
        single = build_by(how, lattice(), pos[st[b]:st[b + 1]].contiguous()) if n else None
        counted += assert_cloud_is_the_single_build(lat, idx, w, single, b, st[b], st[b + 1], rows, step)
    assert counted == total  # cumulative single-cloud vertex counts: no vertex is shared, none is lost
    # one coarser level from the same positions: the same point ranges, half the key step
    lat.set_values(torch.zeros((total, 1), device=dev()))
    coarse = lat.create_coarse_verts_naive(pos)
    crow = coarse.cloud_row_starts().tolist()
    assert coarse.cloud_lengths() == list(lengths) and coarse.m_hash_table._batch[1] * 2 == step
    ckeys, cnb = keys_of(coarse), coarse.neighbours(coarse, 1, False)
    for b, n in enumerate(lengths):
        if not n:
            assert crow[b] == crow[b + 1]
            continue
        sl = lattice()
        sl.just_create_verts(pos[st[b]:st[b + 1]].contiguous(), False)
        sl.set_values(torch.zeros((sl.nr_lattice_vertices(), 1), device=dev()))
        sc = sl.create_coarse_verts_naive(pos[st[b]:st[b + 1]].contiguous())
        mc = sc.nr_lattice_vertices()
        assert crow[b + 1] - crow[b] == mc
        k = ckeys[crow[b]:crow[b + 1]].clone()
        k[:, 0] -= b * coarse.m_hash_table._batch[1]
        assert torch.equal(k, keys_of(sc)), f"coarse keys of cloud {b}"
        nb = cnb[crow[b]:crow[b + 1]]
        assert torch.equal(torch.where(nb >= 0, nb - crow[b], nb), sc.neighbours(sc, 1, False)[:mc]), f"coarse neighbours of cloud {b}"


def chain(lat, pos, vals, bank, grad):
    """splat -> ConvIm2RowLattice -> slice; (output, filter gradient, idx, w)."""
    import lattice_net_amd as L
    W = bank.clone().requires_grad_(True)
    lv, _, idx, w = L.SplatLattice.apply(lat, pos, vals)
    m = lat.nr_lattice_vertices()
    cv, cw = L.ConvIm2RowLattice.apply(lv[:m].contiguous(), lat, W, 1)
    out = L.SliceLattice.apply(cv, cw.lattice, pos, idx, w)
    if grad is not None:
        out.backward(grad)
    return out.detach(), None if grad is None else W.grad.detach(), idx, w


@pytest.mark.parametrize("lengths", LENGTHS)
def test_operators_are_the_single_cloud_runs(lengths, deterministic_mode):
    v, f = 8, 8
    rng = np.random.default_rng(3)
    n = sum(lengths)
    st = starts_of(lengths)
    pos, vals, grad = T(clouds_of(lengths)), T(rng.standard_normal((n, v)).astype(np.float32)), T(rng.standard_normal((n, f)).astype(np.float32))
    bank = T((rng.standard_normal((9 * v, f)) / np.sqrt(9 * v)).astype(np.float32))
    out, gw, _, _ = chain(lattice(list(lengths)), pos, vals, bank, grad)
    gw_sum = torch.zeros_like(gw, dtype=torch.float64)
    for b, nb in enumerate(lengths):
        if not nb:
            continue
        sl = slice(st[b], st[b + 1])
        sout, sgw, _, _ = chain(lattice(), pos[sl].contiguous(), vals[sl].contiguous(), bank, grad[sl].contiguous())
        assert torch.equal(bits(out[sl]), bits(sout)), f"rows of cloud {b}"
        gw_sum += sgw.double()
    worst = float((gw.double() - gw_sum).abs().max()) / float(gw_sum.abs().max())
    print(f"ragged batch {lengths}: filter gradient against the sum over the clouds, worst ratio to the largest magnitude {worst:.3e}")
    assert worst <= BOUND


def test_equal_sizes_as_a_list_are_the_int_form(deterministic_mode):
    from tests.golden import make_cloud_batch_fixture as M
    pos, vals, bank = M.inputs()
    as_int, as_list = M.chain(pos, vals, bank, 100), M.chain(pos, vals, bank, [100, 100, 100])
    for name, a, b in zip(("idx", "w", "keys", "out"), as_int, as_list):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name


@pytest.mark.parametrize("name,batch", [("batch", 100), ("single", None)])
def test_int_form_and_no_batch_are_what_they_were(golden, name, batch, deterministic_mode):
    """Regression: bit for bit what the commit before per-cloud point ranges computed (tests/golden/make_cloud_batch_fixture.py)."""
    from tests.golden import make_cloud_batch_fixture as M
    fx = golden("F14_cloud_batch_int_form")
    pos, vals, bank = M.inputs()
    assert all(np.array_equal(a, fx[k]) for a, k in zip((pos, vals, bank), ("pos", "vals", "bank")))
    for key, got in zip(("idx", "w", "keys", "out"), M.chain(pos, vals, bank, batch)):
        want = fx[f"{name}_{key}"]
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (name, key)


# ---------------------------------------------------------------------------------------------------------------- band check
def band_clouds(scale1):
    lengths = (300, 173, 0, 41)
    rng = np.random.default_rng(7)
    scales = (2.0, scale1, 1.0, 2.0)
    return lengths, np.concatenate([rng.uniform(-1.0, 1.0, (n, 3)) * s for n, s in zip(lengths, scales)]).astype(np.float32)


def test_band_check_takes_each_clouds_own_range():
    from lattice_net_amd import LatticeNetHipError
    from tests import cloud_band_reference as R
    lengths, inside = band_clouds(2.0)
    _, outside = band_clouds(24.0)
    st = starts_of(lengths)
    ext = {}
    for tag, pos_np in (("inside", inside), ("outside", outside)):
        lat = lattice(list(lengths), quotient_step=16, check_band=True, guard=0)
        lat.just_create_verts(T(pos_np), True)
        ref = [R.cloud_key_extents(pos_np[st[b]:st[b + 1]], np.asarray(SIG, np.float32), max(lengths[b], 1))[0].tolist() if lengths[b]
               else [2 ** 31 - 1, -2 ** 31] for b in range(len(lengths))]
        if tag == "inside":
            assert lat.nr_lattice_vertices() > 0  # nobody raises: not the empty cloud either
        else:
            with pytest.raises(LatticeNetHipError, match=r"cloud 1 has first key coordinates \[%d, %d\]" % tuple(ref[1])):
                lat.nr_lattice_vertices()
        ext[tag] = lat.cloud_key_extents().tolist()
        assert ext[tag] == ref, tag
    assert ext["inside"][2] == [2 ** 31 - 1, -2 ** 31]  # the empty cloud: the empty extent
    for b in (0, 2, 3):
        assert ext["inside"][b] == ext["outside"][b]
    assert ext["inside"][1] != ext["outside"][1]


def test_suggest_quotient_step_takes_lengths():
    from lattice_net_amd import suggest_quotient_step
    lengths, pos_np = band_clouds(24.0)
    q = suggest_quotient_step(T(pos_np), SIG, list(lengths))
    lat = lattice(list(lengths), quotient_step=q, check_band=True)
    lat.just_create_verts(T(pos_np), True)
    assert lat.nr_lattice_vertices() > 0
    lat = lattice(list(lengths), quotient_step=q - 16, check_band=True)
    lat.just_create_verts(T(pos_np), True)
    with pytest.raises(Exception, match="cloud 1"):
        lat.nr_lattice_vertices()


# ---------------------------------------------------------------------------------------------------------------- starts check
GUARD = 0x5A5A5A5A


@pytest.mark.parametrize("starts,n,bad", [([0, 300, 473, 514], 514, False), ([0, 300, 299, 514], 514, True), ([0, 300, 473, 513], 514, True),
                                          ([1, 300, 473, 514], 514, True), ([0, 0, 0, 0], 0, False), ([0, 5, 5, 9], 9, False)])
def test_starts_check_on_the_device(starts, n, bad):
    from lattice_net_amd import LatticeNetHipError, _lib
    lat = lattice()
    lat.just_create_verts(T(clouds_of((50,))), False)
    assert lat.nr_lattice_vertices() > 0
    ht = lat.m_hash_table
    buf = torch.tensor([GUARD, GUARD] + starts + [GUARD, GUARD], dtype=torch.int32, device=dev())
    counters_before = ht._counters.tolist()
    rc = _lib.load().ln_cloud_point_starts_check(buf.data_ptr() + 8, len(starts) - 1, n, ht._counters.data_ptr() + 4, _lib.stream_ptr(dev()))
    assert rc == 0
    torch.cuda.synchronize()
    assert buf.tolist() == [GUARD, GUARD] + starts + [GUARD, GUARD]
    nr, status = ht._counters.tolist()
    assert nr == counters_before[0] and status == (counters_before[1] | (_lib.LN_STATUS_CLOUD_STARTS if bad else 0))
    ht.m_nr_filled_is_dirty = True  # the next count read looks at the device words again
    if bad:
        with pytest.raises(LatticeNetHipError, match="point starts"):
            lat.nr_lattice_vertices()
    else:
        assert lat.nr_lattice_vertices() == nr


def test_status_word_has_guards_of_its_own():
    """The status word between two guard words: only the bit is raised."""
    from lattice_net_amd import _lib
    words = torch.tensor([GUARD, 2, GUARD], dtype=torch.int32, device=dev())
    starts = torch.tensor([0, 3, 2, 7], dtype=torch.int32, device=dev())
    assert _lib.load().ln_cloud_point_starts_check(starts.data_ptr(), 3, 7, words.data_ptr() + 4, _lib.stream_ptr(dev())) == 0
    torch.cuda.synchronize()
    assert words.tolist() == [GUARD, 2 | _lib.LN_STATUS_CLOUD_STARTS, GUARD]


def test_a_list_overwritten_on_the_device_is_reported_with_the_build():
    """The Python layer queues the check in front of the band check: starts broken on the device surface at the first count read, and
    the build itself stays inside its buffers (the search never reads outside the list)."""
    from lattice_net_amd import LatticeNetHipError
    lengths = (300, 173, 41)
    lat = lattice(list(lengths), check_band=True)
    lat.m_hash_table._cloud_starts[2] = 100  # 0, 300, 100, 514: not ascending
    lat.just_create_verts(T(clouds_of(lengths)), True)
    with pytest.raises(LatticeNetHipError, match="point starts"):
        lat.nr_lattice_vertices()


# ---------------------------------------------------------------------------------------------------------------- the whole network
NET_LENGTHS, CLASSES = (300, 173, 41), 20
CFG = """
model: { positions_mode: "xyz"  values_mode: "none"  pointnet_layers: [16,32]  pointnet_start_nr_channels: 32  nr_downsamples: 1
    nr_blocks_down_stage: [1]  nr_blocks_bottleneck: 1  nr_blocks_up_stage: [1]  nr_levels_down_with_normal_resnet: 3
    nr_levels_up_with_normal_resnet: 3  compression_factor: 1.0  dropout_last_layer: 0.0 }
lattice_gpu: { hash_table_capacity: 20000  nr_sigmas: 1  sigma_0: "0.9 3" }
"""


def net_loss(lp, y, ranges):
    from lattice_net_amd.losses import nll_loss_gather
    return sum(nll_loss_gather(lp[s:e], y[s:e]) for s, e in ranges if e > s)


def net_run(d, batch, sl=slice(None), lattice_=None):
    """Log-probabilities and parameter gradients of the summed per-cloud NLL loss; `batch`: None (one cloud, the rows `sl`), or the
    argument of set_cloud_batch for the whole batch."""
    from lattice_net_amd import Lattice
    lat = lattice_
    if lat is None:
        lat = Lattice.create(d["cfg"], "lattice")
        if batch is not None:
            lat.set_cloud_batch(batch, per_cloud_norm=True, per_cloud_invalid_vertex=True)
    pos, vals, y = d["pos"][sl].contiguous(), d["vals"][sl].contiguous(), d["y"][sl]
    lp, _ = d["net"](lat, pos, vals)
    ranges = d["ranges"] if batch is not None else [(0, pos.shape[0])]
    params = d.get("params") or list(d["net"].parameters())
    grads = torch.autograd.grad(net_loss(lp, y, ranges), params, allow_unused=True)
    return lp.detach(), [None if t is None else t.detach() for t in grads]


@pytest.fixture(scope="module")
def net(tmp_path_factory):
    """The clouds, the network (GroupNorm parameters moved off 1 / 0) and the reference: every cloud run alone, gradients summed."""
    from lattice_net_amd import Lattice, ModelParams
    from lattice_net_amd import lattice as L
    from lattice_net_amd.models import LNN
    path = tmp_path_factory.mktemp("lnn_ragged") / "lnn.cfg"
    path.write_text(CFG)
    rng = np.random.default_rng(0)
    clouds = []
    for c, n in enumerate(NET_LENGTHS):
        p = rng.uniform(-1.0, 1.0, (n, 3)) * (2.0 + 0.7 * c)
        p[1:8] = p[0] + 1e-3 * 0.9 * rng.standard_normal((7, 3))  # the first vertex of every cloud passes PointNet's four-point rule
        clouds.append(p.astype(np.float32))
    n = sum(NET_LENGTHS)
    st = starts_of(NET_LENGTHS)
    torch.manual_seed(0)
    Lattice.create(str(path), "lattice")
    d = {"cfg": str(path), "net": LNN(CLASSES, ModelParams.create(str(path)), device=dev()), "pos": T(np.concatenate(clouds)),
         "vals": torch.zeros((n, 1), device=dev()), "y": T(rng.integers(0, CLASSES, n).astype(np.int64)),
         "ranges": list(zip(st[:-1], st[1:]))}
    prev_order, prev_det = L.set_row_order("canonical"), L.set_deterministic(True)
    try:
        net_run(d, None, sl=slice(0, NET_LENGTHS[0]))  # (layers that size themselves from their first input exist from here on)
        with torch.no_grad():
            for name, p in d["net"].named_parameters():
                if ".gn." in name or name.endswith("norm.weight") or name.endswith("norm.bias"):
                    p.add_(0.3 * torch.randn_like(p))
        d["params"] = list(d["net"].parameters())
        outs, grads = [], None
        for s, e in d["ranges"]:
            out, gr = net_run(d, None, sl=slice(s, e))
            outs.append(out)
            grads = gr if grads is None else [a if b is None else a + b for a, b in zip(grads, gr)]
        d["ref_out"], d["ref_grads"] = torch.cat(outs), grads
    finally:
        L.set_row_order(prev_order)
        L.set_deterministic(prev_det)
    assert sum(x is not None for x in grads) > 20
    return d


def rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def net_figures(d, out, grads):
    figures = {f"out cloud {c}": rel(out[s:e], d["ref_out"][s:e]) for c, (s, e) in enumerate(d["ranges"])}
    for (name, _), got, ref in zip(d["net"].named_parameters(), grads, d["ref_grads"]):
        assert (got is None) == (ref is None), name
        if ref is not None:
            figures[f"grad {name}"] = rel(got, ref)
    return figures


def test_lnn_on_a_ragged_batch_is_the_clouds_one_at_a_time(net, deterministic_mode):
    out, grads = net_run(net, list(NET_LENGTHS))
    figures = net_figures(net, out, grads)
    print(f"LNN on the ragged batch {NET_LENGTHS}, both per-cloud switches, against single-cloud runs (relative to the largest "
          f"magnitude): worst {max(figures.values()):.3e} ({max(figures, key=figures.get)})")
    bad = {k: v for k, v in figures.items() if not v <= BOUND}
    assert not bad, bad


def test_lnn_with_the_int_form_on_the_same_points_is_not(net, deterministic_mode):
    """set_cloud_batch(300) cuts the 514 points at 300 only: cloud 0 is what it is alone, clouds 1 and 2 share one lattice."""
    out, _ = net_run(net, 300)
    figures = {c: rel(out[s:e], net["ref_out"][s:e]) for c, (s, e) in enumerate(net["ranges"])}
    print("LNN with set_cloud_batch(300) on the ragged points, outputs against single-cloud runs: " + ", ".join(f"{v:.3e}" for v in figures.values()))
    assert figures[0] <= BOUND, figures
    assert figures[1] > BOUND and figures[2] > BOUND, figures


def test_lnn_on_a_ragged_batch_as_a_graph(net, deterministic_mode):
    """The same step through CapturedNetworkStep with its default flags: two replays are equal bit for bit, non-zero, and within the
    bound of the eager step."""
    from lattice_net_amd import CapturedNetworkStep, Lattice
    eager_out, eager_grads = net_run(net, list(NET_LENGTHS))
    lat = Lattice.create(net["cfg"], "lattice")
    lat.set_cloud_batch(list(NET_LENGTHS), per_cloud_norm=True, per_cloud_invalid_vertex=True)
    params = net["params"]

    def step():
        lp, _ = net["net"](lat, net["pos"], net["vals"])
        net_loss(lp, net["y"], net["ranges"]).backward()
        return lp.detach()

    threads = torch.autograd.is_multithreading_enabled()
    torch.autograd.set_multithreading_enabled(False)
    try:
        cap = CapturedNetworkStep(step, lat, params)
        replays = []
        with torch.cuda.stream(cap.stream):
            for _ in range(2):
                out = cap.launch()
                cap.stream.synchronize()
                counts = cap.check()
                assert all(0 < counts[k] <= cap.bounds[k] for k in counts), (counts, cap.bounds)
                replays.append([out.clone()] + [None if g is None else g.clone() for g in cap.grads])
        torch.cuda.synchronize()
    finally:
        torch.autograd.set_multithreading_enabled(threads)
        lat.set_static_rows(None)
        for p in params:
            p.grad = None
    for a, b in zip(*replays):
        assert (a is None and b is None) or torch.equal(a, b), "two replays differ"
    assert bool(replays[0][0].abs().sum() > 0)
    pairs = [(replays[0][0], eager_out)] + [(a, b) for a, b in zip(replays[0][1:], eager_grads) if b is not None]
    worst = max(rel(a, b) for a, b in pairs)
    print(f"LNN on the ragged batch as a graph: replays against the eager step, worst {worst:.3e}")
    assert worst <= BOUND, worst
