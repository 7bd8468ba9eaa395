#!/usr/bin/env python3
"""One C2-shaped line for a cloud batch of unequal sizes: splat -> convolution -> slice, forward and backward, V = F = 32, sigma 0.05,
16 box-surface clouds in one lattice, as one captured graph (CapturedStep, no regions), replayed on one stream.

    python tools/bench_ragged_batch.py [--steps 200] [--warmup 20] [--repeats 3]

Prints one JSON line with the rate in Mpoints/s of three forms on the same 120 000 points' worth of clouds:
  ragged      lengths drawn once (seed 0) from 5 000 .. 10 000 and scaled to sum to 120 000, set_cloud_batch([...])
  equal_list  16 x 7 500 as a list, set_cloud_batch([7500] * 16)   (the binary search on the starts, equal sizes)
  equal_int   16 x 7 500 as an int, set_cloud_batch(7500)          (the division, what bench.py --workload C2 runs)
Each rate is the median of --repeats windows of --steps replays, the forms taken in turn; the spread is (max - min) / median."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CLOUDS, TOTAL, V, F, SIGMA = 16, 120000, 32, 32, 0.05


def ragged_lengths():
    rng = np.random.default_rng(0)
    raw = rng.integers(5000, 10001, CLOUDS).astype(np.float64)
    lengths = np.floor(raw * TOTAL / raw.sum()).astype(np.int64)
    lengths[: TOTAL - int(lengths.sum())] += 1  # the rounding's remainder, one point each
    assert int(lengths.sum()) == TOTAL and lengths.min() >= 5000 * TOTAL // int(raw.sum()) - 1
    return [int(x) for x in lengths]


class Form:
    def __init__(self, name, lengths, batch, dev):
        import lattice_net_amd as L
        from lattice_net_amd import CapturedStep, synthetic
        self.name, self.n = name, sum(lengths)
        rng = np.random.default_rng(1)
        pos = np.concatenate([synthetic.box_surface_cloud(n, 100 + b) for b, n in enumerate(lengths)], 0)
        self.pos = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float32)).to(dev)
        self.vals = torch.from_numpy(rng.standard_normal((self.n, V)).astype(np.float32)).to(dev)
        self.G = torch.from_numpy(rng.standard_normal((self.n, F)).astype(np.float32)).to(dev)
        self.W = torch.from_numpy((rng.standard_normal((9 * V, F)) / np.sqrt(9 * V)).astype(np.float32)).to(dev).requires_grad_(True)
        self.lat = L.Lattice(sigmas=[SIGMA] * 3, capacity=60000 * CLOUDS, device=dev)
        self.lat.set_cloud_batch(batch)
        self.state = {}

        def step():
            self.W.grad = None
            lv, _, idx, w = L.SplatLattice.apply(self.lat, self.pos, self.vals)
            m = self.lat.nr_lattice_vertices()
            lv = lv[:m].requires_grad_(True)
            cv, cw = L.ConvIm2RowLattice.apply(lv, self.lat, self.W, 1)
            out = L.SliceLattice.apply(cv, cw.lattice, self.pos, idx, w)
            out.backward(self.G)
            self.state.update(out=out, m=m)

        self.cap = CapturedStep(step, [self.lat], regions=False, before_capture=self.state.clear)

    def window(self, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.cap.launch(0)
        torch.cuda.synchronize()
        return self.n * steps / (time.perf_counter() - t0) / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lengths = ragged_lengths()
    equal = [TOTAL // CLOUDS] * CLOUDS
    forms = [Form("ragged", lengths, lengths, dev), Form("equal_list", equal, equal, dev), Form("equal_int", equal, TOTAL // CLOUDS, dev)]
    for f in forms:
        f.window(args.warmup)
    rates = {f.name: [] for f in forms}
    for _ in range(args.repeats):
        for f in forms:
            rates[f.name].append(f.window(args.steps))
    for f in forms:
        f.cap.check()
    out = {"workload": "C2-shaped ragged batch", "clouds": CLOUDS, "points": TOTAL, "lengths": lengths, "steps": args.steps}
    for name, r in rates.items():
        med = statistics.median(r)
        out[name] = {"mpoints_per_s": round(med, 1), "spread": round((max(r) - min(r)) / med, 4), "windows": [round(x, 1) for x in r]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
