"""The per-cloud Lovasz-Softmax loss (ln_lovasz_forward_clouds, csrc/ln_lovasz.hip) against the fp64 per-cloud reference and the counted
bounds of tests/lovasz_clouds_reference.py, bit for bit against ln_lovasz_forward on every cloud's slice, and through
losses.LovaszSoftmax(points_per_cloud=)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from . import lovasz_clouds_reference as RC
from . import lovasz_reference as R

pytestmark = pytest.mark.gpu

TILE = R.LN_LV_TILE
NO_LABEL = -(1 << 62)
IGNORE = 0
# (n0, clouds, points of the last cloud, classes): every n0 of the tile edges, every B in 1..5, last cloud full / 1 point / n0 - 1
SHAPES = [(1, 1, 1, 2), (1, 5, 1, 3), (65, 3, 65, 3), (65, 4, 1, 20), (65, 2, 64, 2), (TILE - 1, 2, TILE - 2, 3), (TILE, 2, TILE, 2),
          (TILE, 3, 1, 3), (TILE + 1, 2, TILE + 1, 20), (TILE + 1, 5, TILE, 3), (2 * TILE + 903, 3, 1, 20),
          (2 * TILE + 903, 4, 2 * TILE + 902, 2), (3, 700, 3, 20)]
WORST = {}


@pytest.fixture(autouse=True)
def fused_lovasz(monkeypatch):
    """LovaszSoftmax takes the kernels here whatever the module's default is."""
    from lattice_net_amd import losses
    monkeypatch.setattr(losses, "FUSED_LOVASZ", True)


def dev():
    return torch.device("cuda", 0)


def _lib():
    from lattice_net_amd import _lib
    return _lib, _lib.load()


@functools.lru_cache(maxsize=None)
def case(shape, family, red="mean"):
    """(logp, labels, fp64 reference): computed once per case, shared, never written to."""
    n0, clouds, last, c = shape
    lp, y = RC.batch(n0, clouds, last, c, 5, family)
    ref = RC.reference(lp, y, n0, IGNORE, red)
    for a in (lp, y) + tuple(ref[1:]):
        a.setflags(write=False)
    return lp, y, ref


def forward_clouds(lp, y, n0, ignore, red, outputs=True):
    """((loss, per_cloud, per_class, dloss_dlogp) as NumPy, dloss_dlogp on the device).  Every output starts as NaN and carries one
    sentinel row of 7 behind it: the call has to overwrite the former completely and leave the latter alone."""
    L, lib = _lib()
    n, c = lp.shape
    clouds = len(RC.cloud_ranges(n, n0))
    x = torch.from_numpy(np.array(lp)).to(dev())
    t = torch.from_numpy(np.array(y)).to(dev())
    ws = torch.empty((lib.ln_lovasz_clouds_workspace_bytes(n, n0, c),), dtype=torch.uint8, device=dev())
    loss = torch.full((2,), float("nan"), device=dev())
    pcl = torch.full((clouds + 1,), float("nan"), device=dev())
    pc = torch.full((clouds + 1, c), float("nan"), device=dev())
    dl = torch.full((n + 1, c), float("nan"), device=dev())
    for a in (loss, pcl, pc, dl):
        a[-1] = 7.0
    L.check(lib.ln_lovasz_forward_clouds(L.ptr(x), L.ptr(t), n, n0, c, NO_LABEL if ignore is None else ignore, 0 if red == "mean" else 1,
                                         L.ptr(ws), ws.numel(), L.ptr(loss), L.ptr(pcl) if outputs else None, L.ptr(pc) if outputs else None,
                                         L.ptr(dl), L.stream_ptr(dev())), "ln_lovasz_forward_clouds")
    torch.cuda.synchronize()
    for a in (loss, pcl, pc, dl):
        assert bool((a[-1] == 7.0).all()), "sentinel row overwritten"
    assert not bool(torch.isnan(dl[:-1]).any()) and not bool(torch.isnan(loss[0])), "an output element was not written"
    if outputs:
        assert not bool(torch.isnan(pcl[:-1]).any()) and not bool(torch.isnan(pc[:-1]).any())
    return (loss[0].cpu().numpy(), pcl[:-1].cpu().numpy() if outputs else None, pc[:-1].cpu().numpy() if outputs else None,
            dl[:-1].cpu().numpy()), dl[:-1]


def forward_single(lp, y, ignore, red):
    L, lib = _lib()
    n, c = lp.shape
    x = torch.from_numpy(np.array(lp)).to(dev())
    t = torch.from_numpy(np.array(y)).to(dev())
    ws = torch.empty((lib.ln_lovasz_workspace_bytes(n, c),), dtype=torch.uint8, device=dev())
    loss, pc, dl = torch.empty((1,), device=dev()), torch.empty((c,), device=dev()), torch.empty((n, c), device=dev())
    L.check(lib.ln_lovasz_forward(L.ptr(x), L.ptr(t), n, c, NO_LABEL if ignore is None else ignore, 0 if red == "mean" else 1, L.ptr(ws),
                                  ws.numel(), L.ptr(loss), L.ptr(pc), L.ptr(dl), L.stream_ptr(dev())), "ln_lovasz_forward")
    return loss.cpu().numpy()[0], pc.cpu().numpy(), dl.cpu().numpy()


def forward_module(lp, y, n0, ignore, red, grad_scale=1.0):
    from lattice_net_amd import losses
    assert losses.FUSED_LOVASZ
    x = torch.from_numpy(np.array(lp)).to(dev()).requires_grad_(True)
    loss = losses.LovaszSoftmax(ignore, red, points_per_cloud=n0)(x, torch.from_numpy(np.array(y)).to(dev()))
    (loss * grad_scale).backward()
    return loss.detach().cpu().numpy(), None, None, x.grad.cpu().numpy()


def note(what, ratios):
    WORST[what] = np.maximum(WORST.get(what, np.zeros(4)), ratios)
    print(f"\n[lovasz clouds gpu] {what}: worst error/bound loss {WORST[what][0]:.3f} per cloud {WORST[what][1]:.3f} "
          f"per class {WORST[what][2]:.3f} gradient {WORST[what][3]:.3f}")


@pytest.mark.parametrize("shape", SHAPES)
def test_value_and_gradient_against_fp64_and_bitwise_against_the_single_cloud_call(shape):
    n0, clouds, last, c = shape
    for family, red, gradient in (("separated", "mean", True), ("separated", "sum", True), ("ties_mixed", "mean", True),
                                  ("ties_right", "mean", True), ("ties_wrong", "sum", True), ("softmax", "mean", False)):
        lp, y, ref = case(shape, family, red)
        if family == "separated":  # a condition of the test: fp32 and fp64 must order the errors of a class alike
            for lo, hi in RC.cloud_ranges(len(y), n0)[:5]:
                assert hi - lo == 1 or R.separation(lp[lo:hi], y[lo:hi]) >= 0.25 / (hi - lo + 1) > 2.0 ** -20
        got, _ = forward_clouds(lp, y, n0, IGNORE, red)
        note(f"{family}", RC.check(got, lp, y, n0, IGNORE, red, f"{shape} {family} {red}", gradient=gradient, ref=ref))
        if family == "separated":
            # exact zeros where a class does not count in a cloud, and only there: cloud 2 holds the ignore label alone (loss 0),
            # class 1 is absent from cloud 1 and present next door
            assert np.array_equal(got[3] != 0, ref[3] != 0) and np.array_equal(got[2] != 0, ref[2] != 0)
            if clouds > 2:
                assert got[1][2] == 0.0 and not got[3][2 * n0:3 * n0].any()
            if clouds > 1 and c > 2:
                assert not got[3][n0:2 * n0, 1].any()
        ranges = RC.cloud_ranges(len(y), n0)
        picks = range(clouds) if clouds <= 5 else (0, 1, 2, 3, 350, 699)
        for b in picks:
            lo, hi = ranges[b]
            one = forward_single(lp[lo:hi], y[lo:hi], IGNORE, red)
            assert got[1][b].tobytes() == one[0].tobytes() and got[2][b].tobytes() == one[1].tobytes(), (shape, family, b)
            if RC.is_power_of_two(clouds):
                assert got[3][lo:hi].tobytes() == (one[2] * np.float32(1.0 / clouds)).tobytes(), (shape, family, b)


def test_one_cloud_is_the_single_cloud_call_bit_for_bit():
    for n, c in ((65, 3), (2 * TILE + 903, 20)):
        lp, y = R.softmax_random(n, c, n), R.labels(n, c, 3, out_of_range=True)
        for red in ("mean", "sum"):
            one = forward_single(lp, y, IGNORE, red)
            for n0 in (n, n + 1, 1 << 40):
                got, _ = forward_clouds(lp, y, n0, IGNORE, red)
                assert got[0].tobytes() == one[0].tobytes() and got[1][0].tobytes() == one[0].tobytes()
                assert got[2][0].tobytes() == one[1].tobytes() and got[3].tobytes() == one[2].tobytes()


def test_module_forward_and_backward_with_a_grad_loss():
    scale = float(np.float32(-0.37))
    for shape in ((65, 3, 65, 3), (TILE + 1, 5, TILE, 3), (2 * TILE + 903, 4, 2 * TILE + 902, 2)):
        n0 = shape[0]
        lp, y, ref = case(shape, "separated", "mean")
        abi, _ = forward_clouds(lp, y, n0, IGNORE, "mean", outputs=False)
        got = forward_module(lp, y, n0, IGNORE, "mean", grad_scale=scale)
        assert got[0].tobytes() == abi[0].tobytes(), "LovaszSoftmax(points_per_cloud=) did not take the kernels"
        note("module", RC.check(got, lp, y, n0, IGNORE, "mean", f"module {shape}", through_backward=True, grad_scale=scale, ref=ref))
        again = forward_module(lp, y, n0, IGNORE, "mean", grad_scale=scale)
        assert again[0].tobytes() == got[0].tobytes() and again[3].tobytes() == got[3].tobytes()
    from lattice_net_amd import losses
    with pytest.raises(ValueError):
        losses.LovaszSoftmax(0, "none", points_per_cloud=65)
    x64 = torch.from_numpy(np.array(lp)).double().to(dev())  # float64: the torch form
    assert abs(losses.LovaszSoftmax(IGNORE, points_per_cloud=n0)(x64, torch.from_numpy(np.array(y)).to(dev())).item() - ref[0]) < 1e-12


def test_captured_lovasz_clouds_plus_nll_step_replays_bitwise():
    from lattice_net_amd.losses import LovaszSoftmax, nll_loss_gather
    n0, clouds, last, c = TILE + 1, 3, 903, 20
    inputs = [RC.batch(n0, clouds, last, c, s, "softmax") for s in (0, 1, 2)]
    lov = LovaszSoftmax(ignore_index=0, points_per_cloud=n0)
    x = torch.from_numpy(inputs[0][0]).to(dev()).requires_grad_(True)
    t = torch.from_numpy(inputs[0][1]).to(dev())
    st = {}

    def step(xx, tt):
        loss = 0.5 * lov(xx, tt) + 0.5 * nll_loss_gather(xx, tt, ignore_index=0)
        grad, = torch.autograd.grad(loss, xx)
        return loss.detach(), grad

    eager = [step(torch.from_numpy(lp).to(dev()).requires_grad_(True), torch.from_numpy(y).to(dev())) for lp, y in inputs]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(x, t)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st["loss"], st["grad"] = step(x, t)
    for k in (1, 2):
        with torch.no_grad():
            x.copy_(torch.from_numpy(inputs[k][0]))
        t.copy_(torch.from_numpy(inputs[k][1]))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(st["loss"], eager[k][0]) and torch.equal(st["grad"], eager[k][1]), k
    assert not torch.equal(eager[1][1], eager[2][1])


def _launches(call):
    _, lib = _lib()
    assert lib.ln_profile_begin(b"*", 64) == 0
    rc = call()
    ms, count = C.c_double(), C.c_int()
    assert lib.ln_profile_end(C.byref(ms), C.byref(count)) == 0
    return rc, count.value


def test_argument_errors_launch_nothing_and_write_nothing():
    L, lib = _lib()
    n, n0, c = 130, 65, 3
    x = torch.zeros((n, c), device=dev())
    t = torch.zeros((n,), dtype=torch.int64, device=dev())
    need = lib.ln_lovasz_clouds_workspace_bytes(n, n0, c)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev())
    outs = [torch.full(s, 7.0, device=dev()) for s in ((1,), (2,), (2, c), (n, c))]
    loss, pcl, pc, dl = outs
    sp = L.stream_ptr(dev())

    def fwd(nn, pp, cc, ws_bytes, red=0):
        return lambda: lib.ln_lovasz_forward_clouds(L.ptr(x), L.ptr(t), nn, pp, cc, 0, red, L.ptr(ws), ws_bytes, L.ptr(loss), L.ptr(pcl),
                                                    L.ptr(pc), L.ptr(dl), sp)

    for call, text in ((fwd(n, 0, c, need), b"points_per_cloud"), (fwd(n, n0, 0, need), b"bad sizes"), (fwd(n, n0, 1025, need), b"bad sizes"),
                       (fwd((1 << 31) // c + 1, n0, c, need), b"2^31"), (fwd(RC.MAX_CLOUDS + 1, 1, 2, need), b"at most 65535"),
                       (fwd(2 * RC.MAX_CLOUDS + 1, 2, 2, need), b"at most 65535"), (fwd(n, n0, c, need, red=2), b"reduction"),
                       (fwd(n, n0, c, need - 1), b"workspace"), (fwd(-1, n0, c, need), b"bad sizes")):
        rc, launches = _launches(call)
        assert rc == -1 and launches == 0 and text in lib.ln_last_error_string(), (rc, launches, lib.ln_last_error_string())
    torch.cuda.synchronize()
    assert all(bool((a == 7.0).all()) for a in outs)
    rc, launches = _launches(fwd(n, n0, c, need))  # the good call: one launch more than the 17 of ln_lovasz_forward, none per cloud
    assert rc == 0 and launches == 18
    rc, launches = _launches(fwd(0, n0, c, need))  # no points: loss 0, no sort
    torch.cuda.synchronize()
    assert rc == 0 and launches == 0 and float(loss[0]) == 0.0
    ws1 = torch.empty((lib.ln_lovasz_workspace_bytes(n, c),), dtype=torch.uint8, device=dev())
    rc, launches = _launches(lambda: lib.ln_lovasz_forward(L.ptr(x), L.ptr(t), n, c, 0, 0, L.ptr(ws1), ws1.numel(), L.ptr(loss), None,
                                                           L.ptr(dl), sp))
    assert rc == 0 and launches == 17  # the single-cloud call keeps its launch count


def test_workspace_size_is_a_total_host_function_and_kernels_are_listed():
    _, lib = _lib()
    for n in (0, 1, TILE - 1, TILE + 1, 120000, (1 << 31) - 1):
        for n0 in (1, 7500, (1 << 31) - 1):
            for c in (0, 1, 20, 1024):
                assert lib.ln_lovasz_clouds_workspace_bytes(n, n0, c) >= 256 + 16 * n * c
                assert lib.ln_lovasz_clouds_workspace_bytes(n, n0, c) >= lib.ln_lovasz_workspace_bytes(min(n, n0), c)
    assert lib.ln_lovasz_clouds_workspace_bytes(-5, -5, -5) >= 256
    names = lib.ln_kernel_names().decode().split(",")
    for k in ("k_lovasz_cloud_mean", "k_lovasz_keys", "k_lovasz_hist", "k_lovasz_scan", "k_lovasz_scatter", "k_lovasz_fg_count", "k_lovasz_dot",
              "k_lovasz_finish", "k_lovasz_backward"):
        assert k in names


def test_more_than_2_to_22_segments():
    """65 535 clouds of one point at 65 classes: B x C = 4 259 775 >= 2^22 segments, where a one-dimensional grid of one 1024-thread
    workgroup per segment has 2^32 work-items and cannot be launched — the scans run on a (classes, clouds) grid.  A cloud of one
    point has a closed form: its label's class counts unless it is the ignore class, e = 1 - p, g = 1 / U = 1, loss = 1 - p,
    d loss / d logp = -p at the label and 0 elsewhere."""
    clouds, c = RC.MAX_CLOUDS, 65
    assert clouds * c >= 1 << 22
    lp, y = R.softmax_random(clouds, c, 1, spread=1.0), R.labels(clouds, c, 2)
    got, _ = forward_clouds(lp, y, 1, IGNORE, "mean")
    at = np.arange(clouds)
    pick = lp.astype(np.float64)[at, y]
    counts = y != IGNORE
    per_cloud = np.where(counts, np.abs(np.expm1(pick)), 0.0)
    per_class = np.zeros((clouds, c))
    per_class[at, y] = per_cloud
    grad = np.zeros((clouds, c))
    grad[at, y] = np.where(counts, -np.exp(pick), 0.0) / clouds
    pcb = R.r_total(1, c) * R.EPS32 * per_cloud  # lovasz_reference.loss_bound of a cloud of one point with one counting class
    ratios = (R.worst_ratio(got[0], per_cloud.sum() / clouds, RC.loss_bound(per_cloud, pcb)), R.worst_ratio(got[1], per_cloud, pcb),
              R.worst_ratio(got[2], per_class, R.r_loss(1) * R.EPS32 * per_class),
              R.worst_ratio(got[3], grad, R.grad_bound(grad, RC.r_grad(clouds))))
    note("65535 clouds x 65 classes", ratios)
    assert max(ratios) <= 1.0, ratios
    for b in (0, 1, clouds // 2, clouds - 1):
        one = forward_single(lp[b:b + 1], y[b:b + 1], IGNORE, "mean")
        assert got[1][b].tobytes() == one[0].tobytes() and got[2][b].tobytes() == one[1].tobytes()
