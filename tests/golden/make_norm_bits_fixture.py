"""Records tests/golden/F15_norm_bits.npz: the uint32 bits of every output of the GroupNorm and BatchNorm kernels (csrc/ln_norm.hip) on
random inputs from fixed seeds, forward and backward.  tests/test_gpu_norm_bits.py holds the library to it bit for bit: the fixture was
taken on the commit BEFORE the kernels of ln_norm.hip were rebuilt on shared device bodies, so the comparison shows that no sum changed
its order and no intermediate its precision.

The fp64 atomics of the statistics kernels make a result depend on the order of arrival in general.  It does not where the statistics
grid of a range has at most LN_GN_REPLICAS = 32 workgroups: every accumulator replica then receives one add onto zero, and the sum over
the replicas runs in replica order.  Every case here stays below that (stats_grids(); the test asserts it).

Call paths (PATHS), each at 4, 32, 96 and 1024 channels over 3 statistics workgroups + 3 rows:
    gn            group_norm_rows
    gn_relu       ... with the fused ReLU
    gn_rows       ... with a rows_dev smaller than the tensor
    gn_ranges     ... with row_starts of 4 ranges: a single row, an empty range, two ranges of two workgroups, two rows behind the last
    bn_train      batch_norm_rows in training (running statistics moved)
    bn_eval_rows  batch_norm_rows in evaluation with a rows_dev
and gn_relu once more at 32 channels with all 32 statistics workgroups (`full`).  A GroupNorm case whose apply grid reaches its cap of
2048 workgroups does not exist under that condition, at any channel count: 32 statistics workgroups cover at most 32 * 16 * 256 float4
and the apply grid takes 1024 float4 per workgroup, 128 workgroups at the most.  So that case is left out.

An output of at most ARRAY_BYTES is stored as its uint32 words ("<case>/<output>"), a larger one as the SHA-256 of its bytes
("<case>/<output>.sha256"); the inputs are not stored, inputs() rebuilds them from the seed.  mean_rstd / scale_shift of an empty range
are not written by the kernels: run() returns zeros there.  Run on a GPU from the repository root of the commit to record:

    python tests/golden/make_norm_bits_fixture.py OUT.npz
"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import dense_reference as R  # noqa: E402

CHANNELS = (4, 32, 96, 1024)
PATHS = ("gn", "gn_relu", "gn_rows", "gn_ranges", "bn_train", "bn_eval_rows")
ARRAY_BYTES = 4096
EPS = 1e-5


def slab(c):
    """Rows of one statistics workgroup."""
    return R.gn_rows_per_pass(c) * R.LN_GN_PASSES


def cases():
    """name -> (path, channels, tensor rows, live rows or None, row_starts or None)."""
    out = {}
    for c in CHANNELS:
        m = 3 * slab(c) + 3
        for path in PATHS:
            live = m - slab(c) // 2 - 1 if path.endswith("_rows") else None
            starts = [0, 1, 1, slab(c) + 8, m - 2] if path == "gn_ranges" else None
            out[f"{path}_c{c}"] = (path, c, m, live, starts)
    out["gn_relu_c32_full"] = ("gn_relu", 32, R.LN_GN_REPLICAS * slab(32) - 5, None, None)
    return out


def stats_grids(case):
    """Workgroups that add into the accumulators of each range of the case (the whole matrix is one range)."""
    _, c, m, live, starts = case
    lengths = [b - a for a, b in zip(starts[:-1], starts[1:])] if starts else [m if live is None else live]
    return [-(-n // slab(c)) for n in lengths]


def inputs(name, case):
    _, c, m, _, _ = case
    seed = sorted(cases()).index(name)
    rng = np.random.default_rng(1500 + seed)
    gamma, beta = R.gn_params(c, True, seed)
    return {"x": (0.3 + 1.5 * rng.standard_normal((m, c))).astype(np.float32), "gy": rng.standard_normal((m, c)).astype(np.float32),
            "gamma": gamma, "beta": beta, "running_mean": (0.5 * rng.standard_normal(c)).astype(np.float32),
            "running_var": rng.uniform(0.5, 2.0, c).astype(np.float32)}


def run(name, case):
    """Every output of the case's forward and backward call as float32 NumPy arrays."""
    from lattice_net_amd import lattice_blocks as LB
    path, c, m, live, starts = case
    dev = torch.device("cuda", 0)
    inp = {k: torch.from_numpy(v).to(dev) for k, v in inputs(name, case).items()}
    x = inp["x"].requires_grad_(True)
    rows_dev = None if live is None else torch.tensor([live], dtype=torch.int32, device=dev)
    relu = path != "gn"
    if path.startswith("gn"):
        mod = torch.nn.GroupNorm(32 if c % 32 == 0 else c // 2, c, eps=EPS).to(dev)
        row_starts = None if starts is None else torch.tensor(starts, dtype=torch.int32, device=dev)
        call = lambda: LB.group_norm_rows(x, mod, relu, rows_dev, row_starts)  # noqa: E731
    else:
        mod = torch.nn.BatchNorm1d(c, eps=EPS, momentum=0.1).to(dev).train(path == "bn_train")
        with torch.no_grad():
            mod.running_mean.copy_(inp["running_mean"])
            mod.running_var.copy_(inp["running_var"])
        call = lambda: LB.batch_norm_rows(x, mod, relu, rows_dev)  # noqa: E731
    with torch.no_grad():
        mod.weight.copy_(inp["gamma"])
        mod.bias.copy_(inp["beta"])
    fused, LB.FUSED_BATCH_NORM = LB.FUSED_BATCH_NORM, True  # (without a rows_dev batch_norm_rows takes the kernels only when this is set)
    try:
        y = call()
    finally:
        LB.FUSED_BATCH_NORM = fused
    want = "GroupNormSegmentsFunction" if starts else "GroupNormReluFunction" if path.startswith("gn") else "BatchNormFunction"
    assert type(y.grad_fn).__name__.startswith(want), type(y.grad_fn).__name__
    mean_rstd, scale_shift = (t.detach().clone() for t in y.grad_fn.saved_tensors[2:4])
    if starts:
        for s in range(len(starts) - 1):
            if starts[s + 1] == starts[s]:
                mean_rstd[s] = 0.0
                scale_shift[s] = 0.0
    y.backward(inp["gy"])
    out = {"y": y, "mean_rstd": mean_rstd, "scale_shift": scale_shift, "grad_x": x.grad, "grad_gamma": mod.weight.grad, "grad_beta": mod.bias.grad}
    if path == "bn_train":
        out["running_mean"], out["running_var"] = mod.running_mean, mod.running_var
    torch.cuda.synchronize()
    return {k: np.ascontiguousarray(v.detach().cpu().numpy(), dtype=np.float32) for k, v in out.items()}


def record(case_name, outputs):
    """The fixture's entries for one case: uint32 words, or the SHA-256 of the bytes of an output above ARRAY_BYTES."""
    data = {}
    for key, arr in outputs.items():
        if arr.nbytes <= ARRAY_BYTES:
            data[f"{case_name}/{key}"] = arr.view(np.uint32).copy()
        else:
            data[f"{case_name}/{key}.sha256"] = np.array(hashlib.sha256(arr.tobytes()).hexdigest())
    return data


def main(path):
    data = {}
    for name, case in cases().items():
        assert max(stats_grids(case)) <= R.LN_GN_REPLICAS, (name, stats_grids(case))
        first, again = run(name, case), run(name, case)
        assert all(first[k].tobytes() == again[k].tobytes() for k in first), f"{name}: two runs differ, nothing to record"
        data.update(record(name, first))
    np.savez_compressed(path, **data)
    print("recorded", path, len(data), "entries,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
