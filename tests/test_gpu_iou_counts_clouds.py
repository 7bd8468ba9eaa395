"""Per-cloud intersection / union counts (ln_iou_counts_clouds, csrc/ln_iou.hip) against the NumPy reference of
tests/lovasz_clouds_reference.py — integers, so every comparison is exact — and through losses.Scores.accumulate_scores."""
import ctypes as C

import numpy as np
import pytest
import torch

from . import lovasz_clouds_reference as RC
from . import lovasz_reference as R

pytestmark = pytest.mark.gpu

TILE = R.LN_LV_TILE
# (n0, clouds, points of the last cloud, classes): rows per workgroup is 256; C <= 64 takes a thread per row, C > 64 a wave per row
SHAPES = [(1, 1, 1, 2), (1, 5, 1, 20), (65, 3, 65, 2), (65, 4, 1, 20), (65, 2, 64, 1024), (255, 3, 254, 65), (256, 2, 256, 64),
          (257, 5, 1, 20), (TILE - 1, 2, TILE - 2, 2), (TILE + 1, 3, TILE, 20), (2 * TILE + 903, 4, 1, 20), (300, 3, 299, 1024),
          (3, 700, 3, 20)]


def dev():
    return torch.device("cuda", 0)


def _lib():
    from lattice_net_amd import _lib
    return _lib, _lib.load()


def inputs(shape, seed=4):
    n0, clouds, last, c = shape
    n = n0 * (clouds - 1) + last
    s, y = RC.iou_inputs(n, c, seed)
    if clouds > 1 and c > 1:  # class 1 is missing from the ground truth of cloud 1 and predicted there
        second = y[n0:2 * n0]
        second[(second == 1) | (second >= c)] = 0
        s[n0, :] = 0.0
        s[n0, 1] = 9.0
    if c > 2:  # the maximum repeated at a higher index: the lower one wins
        s[::5, 1] = 8.0
        s[::5, c - 1] = 8.0
    return s, y


def counts(s, y, n0, unlabeled, start=(0, 0), calls=1):
    """(intersection, union) as NumPy after `calls` calls onto accumulators that start at `start`, with a sentinel behind each."""
    L, lib = _lib()
    n, c = s.shape
    x = torch.from_numpy(np.ascontiguousarray(s)).to(dev())
    t = torch.from_numpy(np.ascontiguousarray(y)).to(dev())
    ws = torch.empty((lib.ln_iou_counts_clouds_workspace_bytes(n, n0, c),), dtype=torch.uint8, device=dev())
    inter = torch.full((c + 1,), start[0], dtype=torch.int64, device=dev())
    union = torch.full((c + 1,), start[1], dtype=torch.int64, device=dev())
    inter[-1] = union[-1] = -77
    for _ in range(calls):
        L.check(lib.ln_iou_counts_clouds(L.ptr(x), L.ptr(t), n, n0, c, -1 if unlabeled is None else unlabeled, L.ptr(ws), ws.numel(),
                                         L.ptr(inter), L.ptr(union), L.stream_ptr(dev())), "ln_iou_counts_clouds")
    torch.cuda.synchronize()
    assert int(inter[-1]) == -77 and int(union[-1]) == -77, "sentinel overwritten"
    return inter[:-1].cpu().numpy(), union[:-1].cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES)
def test_counts_are_exact(shape):
    n0, _, _, c = shape
    s, y = inputs(shape)
    for unlabeled in (0, c - 1, None, c + 4, -3):
        ref_i, ref_u = RC.iou_counts(s, y, n0, unlabeled)
        got_i, got_u = counts(s, y, n0, unlabeled)
        assert np.array_equal(got_i, ref_i) and np.array_equal(got_u, ref_u), (shape, unlabeled)
    got_i, got_u = counts(s, y, n0, 0, start=(5, 9), calls=2)  # two calls add twice, onto what was there
    ref_i, ref_u = RC.iou_counts(s, y, n0, 0)
    assert np.array_equal(got_i, 5 + 2 * ref_i) and np.array_equal(got_u, 9 + 2 * ref_u)
    one_i, one_u = RC.iou_counts(s, y, len(y), 0)  # one cloud: points_per_cloud >= n
    got_i, got_u = counts(s, y, len(y) + 3, 0)
    assert np.array_equal(got_i, one_i) and np.array_equal(got_u, one_u)


def test_lowest_index_wins_and_the_batch_differs_from_the_whole():
    s = np.array([[1, 1, 1], [0, 2, 2], [3, 0, 3], [0, 0, 1]], np.float32)
    y = np.array([0, 1, 0, 2], np.int64)
    got_i, got_u = counts(s, y, 4, None)
    assert got_i.tolist() == [2, 1, 1] and got_u.tolist() == [2, 1, 1]
    shape = (65, 3, 65, 20)
    s, y = inputs(shape)
    whole = RC.iou_counts(s, y, len(y), 0)
    per_cloud = counts(s, y, 65, 0)
    assert not np.array_equal(whole[1], per_cloud[1])


def test_capture_and_two_replays_add_twice():
    L, lib = _lib()
    shape = (TILE + 1, 3, TILE, 20)
    s, y = inputs(shape)
    n, c = s.shape
    x, t = torch.from_numpy(s).to(dev()), torch.from_numpy(y).to(dev())
    ws = torch.empty((lib.ln_iou_counts_clouds_workspace_bytes(n, shape[0], c),), dtype=torch.uint8, device=dev())
    inter = torch.zeros((c,), dtype=torch.int64, device=dev())
    union = torch.zeros((c,), dtype=torch.int64, device=dev())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L.check(lib.ln_iou_counts_clouds(L.ptr(x), L.ptr(t), n, shape[0], c, 0, L.ptr(ws), ws.numel(), L.ptr(inter), L.ptr(union),
                                         L.stream_ptr(dev())), "ln_iou_counts_clouds")
    inter.zero_()
    union.zero_()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    ref_i, ref_u = RC.iou_counts(s, y, shape[0], 0)
    assert np.array_equal(inter.cpu().numpy(), 2 * ref_i) and np.array_equal(union.cpu().numpy(), 2 * ref_u)


def test_scores_takes_the_kernel_and_equals_the_cpu_result_cloud_by_cloud():
    from lattice_net_amd import losses
    assert losses.FUSED_IOU_COUNTS
    for shape in ((65, 4, 1, 20), (300, 3, 299, 1024)):
        n0 = shape[0]
        s, y = inputs(shape)
        cpu = losses.Scores()
        for lo, hi in RC.cloud_ranges(len(y), n0):
            cpu.accumulate_scores(torch.from_numpy(s[lo:hi]), torch.from_numpy(y[lo:hi]), 0)
        _, lib = _lib()
        assert lib.ln_profile_begin(b"k_iou_counts_clouds", 8) == 0
        gpu = losses.Scores()
        gpu.accumulate_scores(torch.from_numpy(s).to(dev()), torch.from_numpy(y).to(dev()), 0, points_per_cloud=n0)
        ms, count = C.c_double(), C.c_int()
        assert lib.ln_profile_end(C.byref(ms), C.byref(count)) == 0 and count.value == 1, "Scores did not take the kernel"
        torch_form = losses.Scores()  # float64 scores: the torch form, on the device
        torch_form.accumulate_scores(torch.from_numpy(s).double().to(dev()), torch.from_numpy(y).to(dev()), 0, points_per_cloud=n0)
        for got in (gpu, torch_form):
            assert torch.equal(got.intersection_per_class.cpu(), cpu.intersection_per_class)
            assert torch.equal(got.union_per_class.cpu(), cpu.union_per_class)
            assert got.compute_stats() == cpu.compute_stats()


def test_argument_errors_launch_nothing_and_write_nothing():
    L, lib = _lib()
    n, n0, c = 130, 65, 3
    x = torch.zeros((n, c), device=dev())
    t = torch.zeros((n,), dtype=torch.int64, device=dev())
    need = lib.ln_iou_counts_clouds_workspace_bytes(n, n0, c)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev())
    inter = torch.full((c,), 7, dtype=torch.int64, device=dev())
    union = torch.full((c,), 7, dtype=torch.int64, device=dev())
    sp = L.stream_ptr(dev())

    def run(nn, pp, cc, ws_bytes):
        assert lib.ln_profile_begin(b"*", 64) == 0
        rc = lib.ln_iou_counts_clouds(L.ptr(x), L.ptr(t), nn, pp, cc, 0, L.ptr(ws), ws_bytes, L.ptr(inter), L.ptr(union), sp)
        ms, count = C.c_double(), C.c_int()
        assert lib.ln_profile_end(C.byref(ms), C.byref(count)) == 0
        return rc, count.value

    for args, text in (((n, 0, c, need), b"bad sizes"), ((n, n0, 0, need), b"bad sizes"), ((n, n0, 1025, need), b"bad sizes"),
                       ((-1, n0, c, need), b"bad sizes"), (((1 << 31) // c + 1, n0, c, need), b"2^31"),
                       ((RC.MAX_CLOUDS + 1, 1, 2, need), b"at most 65535"), ((n, n0, c, need - 1), b"workspace")):
        rc, launches = run(*args)
        assert rc == -1 and launches == 0 and text in lib.ln_last_error_string(), (args, rc, launches, lib.ln_last_error_string())
    torch.cuda.synchronize()
    assert bool((inter == 7).all()) and bool((union == 7).all())
    assert run(n, n0, c, need) == (0, 2) and run(0, n0, c, need) == (0, 0)
    for nn in (0, 1, TILE - 1, TILE + 1, 120000, (1 << 31) - 1):
        for pp in (1, 7500, (1 << 31) - 1):
            for cc in (0, 1, 20, 1024):
                assert lib.ln_iou_counts_clouds_workspace_bytes(nn, pp, cc) >= 256 + 12 * -(-nn // pp) * cc
    names = lib.ln_kernel_names().decode().split(",")
    assert "k_iou_counts_clouds" in names and "k_iou_finish_clouds" in names
