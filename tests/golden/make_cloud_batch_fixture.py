"""Records tests/golden/F14_cloud_batch_int_form.npz: what a build and a splat -> convolution -> slice chain give for 300 points at d = 3
with set_cloud_batch(100) and with no batch at all, canonical rows, deterministic mode.  tests/test_gpu_ragged_cloud_batch.py compares
the int form and the no-batch form with it bit for bit: the fixture was taken on the commit BEFORE per-cloud point ranges existed, so the
comparison shows that neither form changed.  Run on a GPU from the repository root of the commit to record:

    python tests/golden/make_cloud_batch_fixture.py OUT.npz
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

N, V, F, SIGMA, CAP = 300, 8, 8, 0.9, 20000


def inputs():
    rng = np.random.default_rng(14)
    pos = np.concatenate([rng.uniform(-1.0, 1.0, (100, 3)) * (2.0 + 0.7 * c) for c in range(3)]).astype(np.float32)
    vals = rng.standard_normal((N, V)).astype(np.float32)
    bank = (rng.standard_normal((9 * V, F)) / np.sqrt(9 * V)).astype(np.float32)
    return pos, vals, bank


def chain(pos, vals, bank, batch):
    """(idx, w, keys, out) of the chain on a new lattice; `batch`: None, or the argument of set_cloud_batch."""
    import lattice_net_amd as L
    dev = torch.device("cuda", 0)
    lat = L.Lattice(sigmas=[SIGMA] * 3, capacity=CAP, device=dev)
    if batch is not None:
        lat.set_cloud_batch(batch)
    p, v, w_bank = (torch.from_numpy(a).to(dev) for a in (pos, vals, bank))
    lv, _, idx, w = L.SplatLattice.apply(lat, p, v)
    m = lat.nr_lattice_vertices()
    cv, cw = L.ConvIm2RowLattice.apply(lv[:m].contiguous(), lat, w_bank, 1)
    out = L.SliceLattice.apply(cv, cw.lattice, p, idx, w)
    torch.cuda.synchronize()
    keys = lat.m_hash_table.m_keys_tensor[:m]
    return [t.detach().cpu().numpy() for t in (idx, w, keys, out)]


def main(path):
    from lattice_net_amd import lattice as LT
    prev = LT.set_row_order("canonical"), LT.set_deterministic(True)
    try:
        pos, vals, bank = inputs()
        data = {"pos": pos, "vals": vals, "bank": bank}
        for name, batch in (("batch", 100), ("single", None)):
            for key, arr in zip(("idx", "w", "keys", "out"), chain(pos, vals, bank, batch)):
                data[f"{name}_{key}"] = arr
    finally:
        LT.set_row_order(prev[0])
        LT.set_deterministic(prev[1])
    np.savez_compressed(path, **data)
    print("recorded", path, {k: v.shape for k, v in data.items()})


if __name__ == "__main__":
    main(sys.argv[1])
