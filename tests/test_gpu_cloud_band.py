"""Band check of a cloud batch on the device (ln_cloud_key_extents, Lattice.set_cloud_batch(check_band=True)) against
tests/cloud_band_reference.py (`pytest -m gpu`).  Every comparison is integer-exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cloud_band_reference as R

pytestmark = pytest.mark.gpu

INT_MAX = R.INT_MAX
SENTINEL = 0x5A5A5A5A
BAND_BIT = 8


def dev():
    return torch.device("cuda", 0)


def c_table(d, batch_points, key_step, counters):
    """An LnTable for the check alone: nr_filled / status are counters[0], counters[1]; no host report."""
    from lattice_net_amd import _lib
    return _lib.LnTable(1, d, None, None, None, None, None, counters.data_ptr(), counters.data_ptr() + 4, None, 0, _lib.LN_KEYS_LATTICE, 0,
                        None, 0, batch_points, key_step, None)


def run_abi(pos, sigmas, n0, key_step, guard, clouds=None, n=None, null=()):
    """One call through the C ABI with sentinel words around both outputs.  Returns (rc, extents [B, 2], first_bad, status, words)."""
    from lattice_net_amd import _lib
    lib = _lib.load()
    n = pos.shape[0] if n is None else n
    d = pos.shape[1]
    B = max(1, -(-pos.shape[0] // max(n0, 1))) if clouds is None else clouds
    words = torch.full((2 * B + 5,), SENTINEL, dtype=torch.int32, device=dev())  # S | extents | S S | first_bad | S
    counters = torch.tensor([123, 0], dtype=torch.int32, device=dev())
    t = c_table(d, n0, key_step, counters)
    base = words.data_ptr()
    args = {"t": C.byref(t), "pos": pos.data_ptr(), "sig": _lib.host_floats(sigmas), "ext": base + 4, "bad": base + 4 * (2 * B + 3)}
    for k in null:
        args[k] = None
    rc = lib.ln_cloud_key_extents(args["t"], args["pos"], args["sig"], n, guard, args["ext"], args["bad"], _lib.stream_ptr(dev()))
    torch.cuda.synchronize()
    w = words.cpu().numpy()
    cnt = counters.tolist()
    assert cnt[0] == 123
    return rc, w[1:1 + 2 * B].reshape(B, 2), int(w[2 * B + 3]), cnt[1], w


def sentinels_intact(w, B):
    return all(int(w[i]) == SENTINEL for i in (0, 2 * B + 1, 2 * B + 2, 2 * B + 4))


def clouds_of(rng, d, n, n0):
    """Cloud c is (1 + 3 c) times as wide as cloud 0: the first passes the band below, later ones need not."""
    pos = rng.uniform(-1.0, 1.0, (n, d))
    pos *= (1.0 + 3.0 * (np.arange(n) // n0))[:, None]
    return pos.astype(np.float32)


@pytest.mark.parametrize("n0", [1, 63, 64, 65, 256, 257])
@pytest.mark.parametrize("d", [2, 3, 6])
def test_extents_and_verdict_are_the_reference_bit_for_bit(d, n0):
    rng = np.random.default_rng(100 * d + n0)
    sig = [0.5 + 0.1 * i for i in range(d)]
    key_step, guard = 16 * (d + 1), 3  # quotient_step 16: half a step is 8 (d + 1) key units
    sizes = [n0, 3 * n0] + ([3 * n0 - (n0 + 1) // 2] if n0 > 1 else [])  # B = 1, B = 3, B = 3 with a shorter last cloud
    verdicts = set()
    for n in sizes:
        pos = clouds_of(rng, d, n, n0)
        B = -(-n // n0)
        ref = R.cloud_key_extents(pos, np.asarray(sig, np.float32), n0)
        ref_bad, ref_bit = R.band_verdict(ref, key_step, guard)
        tpos = torch.from_numpy(pos).to(dev())
        rc, ext, bad, status, w = run_abi(tpos, sig, n0, key_step, guard)
        assert rc == 0
        assert sentinels_intact(w, B), w
        assert ext.tolist() == ref.tolist(), (d, n0, n)
        assert bad == ref_bad and status == (BAND_BIT if ref_bit else 0), (bad, ref_bad, status)
        _, _, _, _, w2 = run_abi(tpos, sig, n0, key_step, guard)
        assert w.tobytes() == w2.tobytes(), "two runs differ"
        verdicts.add(ref_bit)
    if n0 >= 63:
        assert verdicts == {False, True}, "the shapes should exercise both verdicts"


def test_an_empty_cloud_is_inside_its_band():
    """Extents as the init kernel leaves them for a cloud no workgroup touched: n = 0 writes nothing at all, and the verdict kernel
    treats (INT_MAX, INT_MIN) as inside (n0 = 4, n = 5: cloud 1 has one point, grid.x = 1 covers it; nothing is empty on the device, so
    the empty case is the reference's and n = 0)."""
    pos = torch.zeros((5, 3), device=dev())
    rc, ext, bad, status, w = run_abi(pos, [1.0] * 3, 4, 16 * 4 * 2, 0, clouds=2, n=0)
    assert rc == 0 and status == 0 and all(int(x) == SENTINEL for x in w)
    rc, ext, bad, status, w = run_abi(pos, [1.0] * 3, 4, 16 * 4 * 2, 0)
    assert rc == 0 and ext.tolist() == [[0, 3], [0, 3]] and bad == INT_MAX and status == 0


def test_refusals_write_nothing():
    from lattice_net_amd import _lib
    pos = torch.zeros((8, 3), device=dev())
    sig = [1.0] * 3
    step = 16 * 4 * 4  # half = 128
    cases = [
        (dict(n0=0), -1, "no batch"),
        (dict(null="pos"), -1, "null"), (dict(null="sig"), -1, "null"), (dict(null="ext"), -1, "null"), (dict(null="bad"), -1, "null"),
        (dict(null="t"), -1, "null table"),
        (dict(guard=-1), -1, "guard"), (dict(guard=128), -1, "guard"), (dict(guard=1 << 20), -1, "guard"),
        (dict(n=-1), -1, "n < 0"),
        (dict(n0=1, n=65536), -2, "clouds"),
    ]
    for kw, code, text in cases:
        rc, _, _, status, w = run_abi(pos, sig, kw.get("n0", 4), step, kw.get("guard", 0), clouds=2, n=kw.get("n"), null=[kw["null"]] if "null" in kw else ())
        assert rc == code, (kw, rc)
        assert text in _lib.load().ln_last_error_string().decode(), (kw, _lib.load().ln_last_error_string())
        assert status == 0 and all(int(x) == SENTINEL for x in w), kw
    rc, _, _, _, _ = run_abi(pos, sig, 4, step, 127, clouds=2)  # the largest guard that is accepted
    assert rc == 0


# ---------------------------------------------------------------------------------------------------------------- the Python layer
CLOUDS, N0 = 3, 300
SIG = [0.9, 0.9, 0.9]


def three_clouds(scale1):
    rng = np.random.default_rng(7)
    cl = [rng.uniform(-1.0, 1.0, (N0, 3)) * s for s in (2.0, scale1, 2.0)]
    return np.concatenate(cl).astype(np.float32)


def lattice(**batch):
    from lattice_net_amd import Lattice
    lat = Lattice(sigmas=SIG, capacity=20000)
    if batch:
        lat.set_cloud_batch(N0, **batch)
    return lat


def build(lat, pos):
    idx, w = lat.just_create_verts(pos, True)
    return idx, w


def test_a_cloud_that_crosses_into_its_neighbours_band():
    """3 clouds x 300 points, d = 3, quotient_step 16 (a key step of 64, bands of +-32 key units): cloud 1, 12 times as wide as the
    others, reaches far into the bands of clouds 0 and 2.  Unchecked, the batch silently has fewer vertices than the clouds alone, or
    row ranges that are not the clouds' vertex counts; checked, the first vertex-count read raises and names cloud 1."""
    from lattice_net_amd import LatticeNetHipError
    pos_np = three_clouds(24.0)
    ref = R.cloud_key_extents(pos_np, np.asarray(SIG, np.float32), N0)
    assert R.band_verdict(ref, 64, 0) == (1, True) and ref[1, 1] >= 32 + 32 and ref[1, 0] < -32 - 32, ref  # beyond the bands' middles
    pos = torch.from_numpy(pos_np).to(dev())
    singles = []
    for c in range(CLOUDS):
        lat = lattice()
        build(lat, pos[c * N0:(c + 1) * N0].contiguous())
        singles.append(lat.nr_lattice_vertices())
    lat = lattice(quotient_step=16)
    build(lat, pos)
    total = lat.nr_lattice_vertices()
    starts = lat.cloud_row_starts().tolist()
    ranges = [b - a for a, b in zip(starts[:-1], starts[1:])]
    print(f"unchecked: {total} vertices in the batch, {sum(singles)} in the single builds; row ranges {ranges}, single counts {singles}, "
          f"order flag {lat.cloud_row_order_flag().tolist()}")
    assert total < sum(singles) or ranges != singles
    lat = lattice(quotient_step=16, check_band=True, guard=0)
    build(lat, pos)
    with pytest.raises(LatticeNetHipError, match=r"cloud 1 has first key coordinates \[%d, %d\].*quotient_step 16" % (ref[1, 0], ref[1, 1])):
        lat.nr_lattice_vertices()
    assert lat.cloud_key_extents().tolist() == ref.tolist()
    with pytest.raises(LatticeNetHipError, match="cloud 1"):  # (the count stays unread: the error does not go away)
        lat.nr_lattice_vertices()


def test_checked_build_with_a_fitting_step_is_the_unchecked_build():
    from lattice_net_amd import Lattice
    pos = torch.from_numpy(three_clouds(24.0)).to(dev())
    out = []
    for check in (False, True):
        lat = lattice(quotient_step=8192, check_band=check)
        idx, w = build(lat, pos)
        out.append((idx.clone(), w.clone(), lat.nr_lattice_vertices(), lat.cloud_row_starts().clone()))
        if check:
            assert lat.cloud_key_extents().tolist() == R.cloud_key_extents(pos.cpu().numpy(), np.asarray(SIG, np.float32), N0).tolist()
        else:
            with pytest.raises(Exception, match="no checked build"):
                lat.cloud_key_extents()
    (i0, w0, n0, r0), (i1, w1, n1, r1) = out
    assert torch.equal(i0, i1) and torch.equal(w0.view(torch.int32), w1.view(torch.int32)) and n0 == n1 and torch.equal(r0, r1)
    assert Lattice.decode_report((BAND_BIT << 32) | 17) == (17, BAND_BIT)


def test_the_guard_reports_a_cloud_near_the_edge():
    from lattice_net_amd import LatticeNetHipError
    pos_np = three_clouds(24.0)
    ref = R.cloud_key_extents(pos_np, np.asarray(SIG, np.float32), N0)
    reach = int(max(ref[:, 1].max() + 1, -ref[:, 0].min()))
    q = 16 * (-(-reach // 32))  # the smallest step whose half, 2 q key units, holds every cloud: within 32 < 64 key units of the edge
    half = 2 * q
    assert half > 64 and R.band_verdict(ref, 4 * q, 0) == (INT_MAX, False) and R.band_verdict(ref, 4 * q, 64) == (1, True)
    pos = torch.from_numpy(pos_np).to(dev())
    lat = lattice(quotient_step=q, check_band=True)  # the default guard: 16 (d + 1) = 64
    build(lat, pos)
    with pytest.raises(LatticeNetHipError, match="cloud 1"):
        lat.nr_lattice_vertices()
    lat = lattice(quotient_step=q, check_band=True, guard=0)
    build(lat, pos)
    assert lat.nr_lattice_vertices() > 0


def test_suggest_quotient_step_is_the_smallest_that_passes():
    from lattice_net_amd import LatticeNetHipError, suggest_quotient_step
    pos_np = three_clouds(24.0)
    pos = torch.from_numpy(pos_np).to(dev())
    q = suggest_quotient_step(pos, SIG, N0)
    ref = R.cloud_key_extents(pos_np, np.asarray(SIG, np.float32), N0)
    assert q % 16 == 0 and q > 48
    assert R.band_verdict(ref, 4 * q, 64) == (INT_MAX, False) and R.band_verdict(ref, 4 * (q - 16), 64) == (1, True)
    lat = lattice(quotient_step=q, check_band=True)
    build(lat, pos)
    assert lat.nr_lattice_vertices() > 0
    lat = lattice(quotient_step=q - 16, check_band=True)
    build(lat, pos)
    with pytest.raises(LatticeNetHipError, match="cloud 1"):
        lat.nr_lattice_vertices()
    assert suggest_quotient_step(pos, SIG, N0, guard=0) <= q


def test_static_rows_report_the_band():
    """Under set_static_rows nothing reads the device after the build: static_build_report() after a synchronise carries the bit."""
    from lattice_net_amd import LatticeNetHipError, _lib
    good, bad = (torch.from_numpy(three_clouds(s)).to(dev()) for s in (2.5, 24.0))
    lat = lattice(quotient_step=64, check_band=True)
    lat.set_static_rows(8192)
    pos = good.clone()
    for cloud, fails in ((good, False), (bad, True), (good, False)):
        pos.copy_(cloud)
        lat.begin_splat()
        build(lat, pos)
        torch.cuda.synchronize()
        if fails:
            with pytest.raises(LatticeNetHipError, match="cloud 1"):
                lat.static_build_report()
        else:
            assert lat.static_build_report()[1] & _lib.LN_STATUS_CLOUD_BAND == 0


CFG = """
model: { positions_mode: "xyz"  values_mode: "none"  pointnet_layers: [16,32]  pointnet_start_nr_channels: 32  nr_downsamples: 1
    nr_blocks_down_stage: [1]  nr_blocks_bottleneck: 1  nr_blocks_up_stage: [1]  nr_levels_down_with_normal_resnet: 3
    nr_levels_up_with_normal_resnet: 3  compression_factor: 1.0  dropout_last_layer: 0.0 }
lattice_gpu: { hash_table_capacity: 20000  nr_sigmas: 1  sigma_0: "0.9 3" }
"""


def test_captured_network_step_reports_the_band_per_replay(tmp_path):
    """The 3 x 300 LNN of tests/test_gpu_lnn_cloud_batch.py as one graph with the check on: a replay over good clouds passes check(), the
    inputs overwritten in place with cloud 1 moved out of its band make check() raise after the replay, and good clouds pass again."""
    from lattice_net_amd import CapturedNetworkStep, Lattice, LatticeNetHipError, ModelParams
    from lattice_net_amd import lattice as L
    from lattice_net_amd.models import LNN
    classes = 20
    path = tmp_path / "lnn.cfg"
    path.write_text(CFG)
    rng = np.random.default_rng(0)
    good_np = np.concatenate([rng.uniform(-1.0, 1.0, (N0, 3)) * (2.0 + 0.7 * c) for c in range(CLOUDS)]).astype(np.float32)
    bad_np = good_np.copy()
    bad_np[N0:2 * N0, 0] += 32.0  # cloud 1 moved along x: about +82 key units on the first coordinate, the band is [-64, 64)
    sig = np.full(3, 0.9, np.float32)
    assert R.band_verdict(R.cloud_key_extents(good_np, sig, N0), 256, 64) == (INT_MAX, False)
    assert R.band_verdict(R.cloud_key_extents(bad_np, sig, N0), 256, 64) == (1, True)
    good, bad = torch.from_numpy(good_np).to(dev()), torch.from_numpy(bad_np).to(dev())
    pos, vals = good.clone(), torch.zeros((CLOUDS * N0, 1), device=dev())
    g = torch.from_numpy(rng.standard_normal((CLOUDS * N0, classes)).astype(np.float32)).to(dev())
    torch.manual_seed(0)
    lat = Lattice.create(str(path), "lattice")
    net = LNN(classes, ModelParams.create(str(path)), device=dev())
    lat.set_cloud_batch(N0, quotient_step=64, per_cloud_norm=True, per_cloud_invalid_vertex=True, check_band=True)
    prev_det = L.set_deterministic(True)

    def step():
        logsoftmax, _ = net(lat, pos, vals)
        (logsoftmax * g).sum().backward()
        return logsoftmax.detach()

    threads = torch.autograd.is_multithreading_enabled()
    torch.autograd.set_multithreading_enabled(False)
    try:
        step()  # (layers that size themselves from their first input exist from here on)
        params = list(net.parameters())
        for p in params:
            p.grad = None
        cap = CapturedNetworkStep(step, lat, params)
        with torch.cuda.stream(cap.stream):
            for cloud, fails in ((good, False), (bad, True), (good, False)):
                pos.copy_(cloud)
                cap.launch()
                cap.stream.synchronize()
                if fails:
                    with pytest.raises(LatticeNetHipError, match="cloud 1 has first key"):
                        cap.check()
                else:
                    counts = cap.check()
                    assert sorted(counts) == [1, 2]
        torch.cuda.synchronize()
    finally:
        torch.autograd.set_multithreading_enabled(threads)
        L.set_deterministic(prev_det)
        lat.set_static_rows(None)
        for p in net.parameters():
            p.grad = None
