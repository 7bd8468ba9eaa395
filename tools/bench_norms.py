#!/usr/bin/env python3
"""Time of BatchNorm + ReLU, forward + backward, on lattice-value matrices of the sizes the networks see ([46 500, 64] and
[120 000, 32]): the HIP kernels (lattice_blocks.FUSED_BATCH_NORM on) against torch.nn.BatchNorm1d followed by relu.

What is measured is the wall-clock time of 200 eager forward + backward calls between two device synchronisations, divided by 200:
kernels plus the Python and autograd overhead of either path, which is what a training loop in eager mode pays.  Five runs of each,
alternating.  The rule for switching FUSED_BATCH_NORM on: the median of the five native runs below the fastest torch
run.  (Both paths are in training mode: every call also moves the module's running statistics and num_batches_tracked, part of
either path's work and of no consequence here.)

--ranges B [B ...]: instead, GroupNorm + ReLU forward + backward per row range at [46 080, 64] and [11 520, 128], B equal ranges
(ln_group_norm_forward_many_segments / _backward_many_segments: up to 64 ranges the accumulator-slab kernels, beyond one workgroup per
range) against the whole-matrix GroupNorm on the same tensor, through the C ABI on buffers allocated once, the alternating accumulator
pair as the modules use it.  A window is 200 forward + backward pairs queued between two device synchronisations, divided by 200: the
kernels of a pair when they take longer than their launches.  Five windows of each form, alternating; median, fastest and slowest.

--f16: GroupNorm + ReLU forward + backward per row range (4 equal ranges) at [46 500, 64] and [120 000, 32] through the C ABI, windows as
for --ranges: the fp16 kernels (ln_group_norm_forward_segments_f16 / _backward_segments_f16) next to the fp32 kernels on the same numbers,
and the ratio of their medians."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lattice_net_amd import lattice_blocks  # noqa: E402
from lattice_net_amd.lattice_blocks import batch_norm_rows  # noqa: E402

SHAPES = ((46500, 64), (120000, 32))
RUNS, WARMUP, ITERS = 5, 10, 200


def run(x, gy, bn):
    """Microseconds per BnRelu forward + backward on the path FUSED_BATCH_NORM selects."""

    def once():
        x.grad = None
        batch_norm_rows(x, bn, True).backward(gy)

    for _ in range(WARMUP):
        once()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        once()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / ITERS * 1e6


RANGE_SHAPES = ((46080, 64), (11520, 128))


def range_windows(m, c, ranges_list, dev):
    from lattice_net_amd import _lib
    lib, p = _lib.load(), _lib.ptr
    groups = 32
    x, gy = torch.randn((m, c), device=dev), torch.randn((m, c), device=dev)
    w, b = torch.rand((c,), device=dev) + 0.5, torch.randn((c,), device=dev)
    y, dx, dw, db = torch.empty_like(x), torch.empty_like(x), torch.empty_like(w), torch.empty_like(w)
    stream = _lib.stream_ptr(dev)
    forms = {}
    for segs in ranges_list:  # 0: the whole matrix
        n = max(segs, 1)
        nbytes = int(lib.ln_group_norm_segments_workspace_bytes(c, segs) if segs else lib.ln_group_norm_workspace_bytes(c))
        ws = [torch.zeros((nbytes // 8,), dtype=torch.float64, device=dev) for _ in range(2)]
        mr, ss = torch.empty((n, 2 * groups), device=dev), torch.empty((n, 2 * c), device=dev)
        starts = torch.tensor([m * i // n for i in range(n + 1)], dtype=torch.int32, device=dev)
        tail = (p(starts), segs, stream) if segs else (stream,)
        fwd = lib.ln_group_norm_forward_many_segments if segs else lib.ln_group_norm_forward_rows
        bwd = lib.ln_group_norm_backward_many_segments if segs else lib.ln_group_norm_backward_rows

        def pair(ws=ws, mr=mr, ss=ss, tail=tail, fwd=fwd, bwd=bwd, nbytes=nbytes, keep=starts):
            _lib.check(fwd(p(x), p(w), p(b), m, c, groups, 1e-5, 1, p(y), p(mr), p(ss), p(ws[0]), nbytes, p(ws[1]), nbytes, None, *tail), "forward")
            _lib.check(bwd(p(x), p(gy), p(w), p(mr), p(ss), m, c, groups, 1, p(dx), p(dw), p(db), p(ws[1]), nbytes, p(ws[0]), nbytes, None, *tail),
                       "backward")
        forms[segs] = pair
    times = {segs: [] for segs in forms}
    for _ in range(RUNS):
        for segs, pair in forms.items():
            for _ in range(WARMUP):
                pair()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(ITERS):
                pair()
            torch.cuda.synchronize()
            times[segs].append((time.perf_counter() - t0) / ITERS * 1e6)
    whole = statistics.median(times[0])
    for segs, t in times.items():
        t = sorted(t)
        name = "whole matrix" if not segs else f"{segs:4d} ranges ({'slab form' if segs <= 64 else 'range owners'})"
        print(f"GnRelu fwd+bwd [{m}, {c}] {name:28s} median {statistics.median(t):7.1f} us  fastest {t[0]:7.1f}  slowest {t[-1]:7.1f}  "
              f"median / whole matrix {statistics.median(t) / whole:.2f}")


def f16_windows(m, c, dev):
    """C ABI, 4 equal row ranges: fp16 kernels against fp32 kernels on the same numbers."""
    from lattice_net_amd import _lib
    lib, p = _lib.load(), _lib.ptr
    groups = 32
    x32, gy32 = torch.randn((m, c), device=dev).half().float(), torch.randn((m, c), device=dev).half().float()
    w, b = torch.rand((c,), device=dev) + 0.5, torch.randn((c,), device=dev)
    dw, db = torch.empty_like(w), torch.empty_like(w)
    segs = 4
    mr, ss = torch.empty((segs, 2 * groups), device=dev), torch.empty((segs, 2 * c), device=dev)
    starts = torch.tensor([m * i // segs for i in range(segs + 1)], dtype=torch.int32, device=dev)
    nbytes = int(lib.ln_group_norm_segments_workspace_bytes(c, segs))
    ws = [torch.zeros((nbytes // 8,), dtype=torch.float64, device=dev) for _ in range(2)]
    stream = _lib.stream_ptr(dev)
    forms = {}
    for name, dtype, fwd, bwd in (("fp32 kernels", torch.float32, lib.ln_group_norm_forward_segments, lib.ln_group_norm_backward_segments),
                                  ("fp16 kernels", torch.float16, lib.ln_group_norm_forward_segments_f16, lib.ln_group_norm_backward_segments_f16)):
        x, gy = x32.to(dtype), gy32.to(dtype)
        y, dx = torch.empty_like(x), torch.empty_like(x)

        def pair(x=x, gy=gy, y=y, dx=dx, fwd=fwd, bwd=bwd):
            _lib.check(fwd(p(x), p(w), p(b), m, c, groups, 1e-5, 1, p(y), p(mr), p(ss), p(ws[0]), nbytes, p(ws[1]), nbytes, None, p(starts), segs, stream), "forward")
            _lib.check(bwd(p(x), p(gy), p(w), p(mr), p(ss), m, c, groups, 1, p(dx), p(dw), p(db), p(ws[1]), nbytes, p(ws[0]), nbytes, None, p(starts), segs, stream),
                       "backward")
        forms[name] = pair
    times = {name: [] for name in forms}
    for _ in range(RUNS):
        for name, pair in forms.items():
            for _ in range(WARMUP):
                pair()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(ITERS):
                pair()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / ITERS * 1e6)
    for name, t in times.items():
        t = sorted(t)
        print(f"GnRelu fwd+bwd [{m}, {c}] 4 ranges, C ABI {name}  median {statistics.median(t):7.1f} us  fastest {t[0]:7.1f}  slowest {t[-1]:7.1f}")
    print(f"GnRelu fwd+bwd [{m}, {c}] 4 ranges, C ABI fp16 / fp32 medians {statistics.median(times['fp16 kernels']) / statistics.median(times['fp32 kernels']):.2f}")


def main():
    dev = torch.device("cuda", 0)
    if "--f16" in sys.argv:
        for m, c in SHAPES:
            f16_windows(m, c, dev)
        return
    if "--ranges" in sys.argv:
        ranges = [int(a) for a in sys.argv[sys.argv.index("--ranges") + 1:]]
        for m, c in RANGE_SHAPES:
            range_windows(m, c, [0] + ranges, dev)
        return
    default = lattice_blocks.FUSED_BATCH_NORM
    try:
        for m, c in SHAPES:
            x = torch.randn((m, c), device=dev, requires_grad=True)
            gy = torch.randn((m, c), device=dev)
            bn = torch.nn.BatchNorm1d(c).to(dev)
            times = {True: [], False: []}
            for _ in range(RUNS):  # alternating, so that both see the same clocks
                for fused in (True, False):
                    lattice_blocks.FUSED_BATCH_NORM = fused
                    times[fused].append(run(x, gy, bn))
            native, plain = sorted(times[True]), sorted(times[False])
            print(f"BnRelu fwd+bwd [{m}, {c}] HIP kernels  median {statistics.median(native):7.1f} us  (runs {' '.join(f'{t:.1f}' for t in native)})")
            print(f"BnRelu fwd+bwd [{m}, {c}] torch        fastest {plain[0]:7.1f} us  (runs {' '.join(f'{t:.1f}' for t in plain)})")
    finally:
        lattice_blocks.FUSED_BATCH_NORM = default


if __name__ == "__main__":
    main()
