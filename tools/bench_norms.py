#!/usr/bin/env python3
"""Time of BatchNorm + ReLU, forward + backward, on lattice-value matrices of the sizes the networks see ([46 500, 64] and
[120 000, 32]): the HIP kernels (lattice_blocks.FUSED_BATCH_NORM on) against torch.nn.BatchNorm1d followed by relu.

What is measured is the wall-clock time of 200 eager forward + backward calls between two device synchronisations, divided by 200:
kernels plus the Python and autograd overhead of either path, which is what a training loop in eager mode pays.  Five runs of each,
alternating.  The rule for switching FUSED_BATCH_NORM on: the median of the five native runs below the fastest torch
run.  (Both paths are in training mode: every call also moves the module's running statistics and num_batches_tracked, part of
either path's work and of no consequence here.)"""
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


def main():
    dev = torch.device("cuda", 0)
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
