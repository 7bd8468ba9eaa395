#!/usr/bin/env python3
"""Kernel time of the per-cloud "invalid vertex" entry points against the ones they stand in for, in one process:
ln_distribute_centre_clouds vs ln_distribute_centre and ln_pointnet_reduce_forward_clouds vs ln_pointnet_reduce_forward at the
SemanticKITTI network's sizes (120 000 LiDAR-like points, 480 000 tokens, width 5, 32 channels), as 1 cloud and as 16 clouds.

    python tools/bench_invalid_vertex.py [--reps 40]      # one JSON line

The two entry points of a pair alternate call by call; every call is timed on its own with ln_profile_begin("*") / ln_profile_end
(the summed durations of the dispatches of that call: zero fill + segment max + decode for the reduction), and the medians are
reported in microseconds with their ratio."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lattice_net_amd as L  # noqa: E402
from lattice_net_amd import _lib, synthetic  # noqa: E402
from lattice_net_amd import lattice as LL  # noqa: E402
from lattice_net_amd.lattice_funcs import DistributeLattice  # noqa: E402

N, CH, WIDTH, POS_DIM = 120000, 32, 5, 3


def timed(lib, fn):
    if lib.ln_profile_begin(b"*", 64) != 0:
        raise RuntimeError(lib.ln_last_error_string())
    fn()
    torch.cuda.synchronize()
    ms, cnt = C.c_double(0.0), C.c_int(0)
    if lib.ln_profile_end(C.byref(ms), C.byref(cnt)) != 0:
        raise RuntimeError(lib.ln_last_error_string())
    return ms.value * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    args = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    LL.set_row_order("canonical")
    pos = torch.from_numpy(synthetic.lidar_cloud(N, 0)).to(dev)
    vals = torch.zeros((N, 1), device=dev)
    src = torch.randn((N * (POS_DIM + 1), CH), device=dev)
    result = {"points": N, "tokens": N * (POS_DIM + 1), "width": WIDTH, "channels": CH, "reps": args.reps, "unit": "us"}
    for clouds in (1, 16):
        n0 = N // clouds
        lat = L.Lattice(sigmas=[0.9] * 3, capacity=8 * N // 4, device=dev)
        lat.set_cloud_batch(n0, per_cloud_invalid_vertex=True)
        wrap, d, idx, _ = DistributeLattice.apply(lat, pos, vals, True)
        dl = wrap.lattice
        rows, tokens = dl.nr_lattice_vertices(), idx.numel()
        starts = dl.per_cloud_invalid_row_starts()
        assert starts.numel() == clouds + 1
        counts = dl.vertex_point_counts(idx)
        sums = torch.zeros((rows, POS_DIM), device=dev)
        dl._scatter_rows(d, idx, torch.ones((tokens,), device=dev), sums, POS_DIM, 1, WIDTH)
        out = torch.empty_like(d)
        _, csr, max_seg, grp_row, _ = dl._csr(idx)
        ws = torch.empty((lib.ln_pointnet_reduce_workspace_bytes(rows, CH),), dtype=torch.uint8, device=dev)
        red = torch.empty((rows, 2 * CH), device=dev)
        arg = torch.empty((rows, CH), dtype=torch.int32, device=dev)
        st = _lib.stream_ptr(dev)
        head_d = (_lib.ptr(d), _lib.ptr(idx), _lib.ptr(sums), _lib.ptr(counts), tokens, WIDTH, POS_DIM)
        head_r = (C.byref(csr), _lib.ptr(grp_row), max_seg, _lib.ptr(src), CH, d.data_ptr() + 4 * (WIDTH - 1), WIDTH, rows, 4, _lib.ptr(ws),
                  ws.numel(), _lib.ptr(red), _lib.ptr(arg))
        calls = {
            "ln_distribute_centre": lambda: _lib.check(lib.ln_distribute_centre(*head_d, _lib.ptr(out), st)),
            "ln_distribute_centre_clouds": lambda: _lib.check(lib.ln_distribute_centre_clouds(*head_d, n0 * (POS_DIM + 1), _lib.ptr(starts), clouds,
                                                                                              _lib.ptr(out), st)),
            "ln_pointnet_reduce_forward": lambda: _lib.check(lib.ln_pointnet_reduce_forward(*head_r, st)),
            "ln_pointnet_reduce_forward_clouds": lambda: _lib.check(lib.ln_pointnet_reduce_forward_clouds(*head_r, _lib.ptr(starts), clouds, st)),
        }
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.2:  # the chip needs tens of ms of load to reach its busy clocks
            for fn in calls.values():
                fn()
            torch.cuda.synchronize()
        entry = {"rows": rows}
        for old, new in (("ln_distribute_centre", "ln_distribute_centre_clouds"), ("ln_pointnet_reduce_forward", "ln_pointnet_reduce_forward_clouds")):
            t_old, t_new = [], []
            for _ in range(args.reps):
                t_old.append(timed(lib, calls[old]))
                t_new.append(timed(lib, calls[new]))
            a, b = statistics.median(t_old), statistics.median(t_new)
            entry[old] = round(a, 2)
            entry[new] = round(b, 2)
            entry[new + "/" + old] = round(b / a, 3)
        result[f"clouds_{clouds}"] = entry
    print(json.dumps(result))


if __name__ == "__main__":
    np.random.seed(0)
    main()
