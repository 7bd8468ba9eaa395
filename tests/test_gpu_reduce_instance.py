"""The chain-width instances of the CSR segment reduce (ln_csr.hip: ln_reduce_chunk<..., L8 = 8, CHAIN>, picked by ln_chain_fits for
128-byte source rows shared by 4 tokens: 32 fp32 or 64 fp16 channels in three dimensions) through the public operators
(`pytest -m gpu`): the splat accumulate (k_reduce_and_neighbours) and the slice backward (k_csr_reduce_segments) against an fp64
NumPy scatter over the lattice's own idx / w, element by element within close_terms of tests/test_gpu_parity.py —
|a - ref| <= 1e-5 * sum |value x weight| over the vertex's tokens (one chained accumulation: ops = 1).

The shapes are the smallest that reach every path of the instance: one partly filled wave (no two lane groups share a row: the
combine is skipped), hundreds of tokens on the vertices of one cell (runs over several lane groups, waves and workgroups: every
combine round and the atomic path), a LiDAR-like cloud (mixed), a last batch of a segment padded by re-reading its last entry with
weight 0, fp16 rows of 64 channels under the dense hint (the workgroup-combining instance), and 24 channels, which the instance does
not take.  fp32 cases run without the dense hint: with it a row of 32 floats goes to the generic workgroup-combining instance.

fp16: the splat accumulates fp16 rows into fp32 vertex values (bound as above, reference over the exact fp16 inputs).  The slice
backward returns the gradient in fp16: the fp32 sum is rounded once, which adds half an fp16 ulp — 2^-11 |ref| (2^-25 below the normal
range) — to the bound of that one comparison; the fp32 accumulator itself is held to the plain bound through Lattice._scatter_rows."""
import numpy as np
import pytest
import torch

from tests.test_gpu_parity import close_terms
from tests.test_gpu_segment_reduce import reduce_mode

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def N(t):
    return t.detach().cpu().numpy()


def scatter64(src, idx, w, rows, src_div=4):
    """fp64 scatter: out[idx[t]] += src[t // src_div] * w[t]; returns (sum, sum of |terms|).  idx < 0 is skipped."""
    src, idx, w = np.asarray(src, np.float64), np.asarray(idx, np.int64), np.asarray(w, np.float64)
    t = np.nonzero(idx >= 0)[0]
    with np.errstate(invalid="ignore"):
        terms = src[t // src_div] * w[t][:, None]
    ref = np.zeros((rows, src.shape[1]), np.float64)
    mag = np.zeros_like(ref)
    with np.errstate(invalid="ignore"):
        np.add.at(ref, idx[t], terms)
    np.add.at(mag, idx[t], np.abs(np.where(np.isfinite(terms), terms, 0.0)))
    return ref, mag


def rounded_sum_limit(ref, mag):
    """The bound of an fp32 sum of terms returned in fp16: the plain bound of the sum (close_terms: 1e-5 * sum |terms|) plus its one
    rounding, half an fp16 ulp — 2^-11 |ref|, 2^-25 below the normal range."""
    return 1e-5 * mag + np.maximum(2.0 ** -11 * np.abs(ref), 2.0 ** -25)


def lidar(n, seed=3):
    from lattice_net_amd.synthetic import lidar_cloud
    return np.ascontiguousarray(lidar_cloud(n, seed), dtype=np.float32)


def one_cell(n, seed=5):
    """n points within 0.04 of one position: the 4 vertices of its simplex (and a few next to it) carry hundreds of tokens each."""
    rng = np.random.default_rng(seed)
    return (np.array([[3.3, -1.7, 0.4]]) + rng.uniform(-0.04, 0.04, (n, 3))).astype(np.float32)


CLOUDS = {"wave7": lambda: lidar(7), "cell600": lambda: one_cell(600), "lidar3000": lambda: lidar(3000), "padded5": lambda: lidar(5)}
_CACHE = {}


def cloud(name):
    if name not in _CACHE:
        _CACHE[name] = CLOUDS[name]()
    return _CACHE[name]


def splat_and_slice_backward(pos_np, v, dtype, seed, builds=1):
    """SplatLattice of random rows, then SliceLattice's backward of a random gradient, each against scatter64 of the same idx / w."""
    import lattice_net_amd as L
    n = len(pos_np)
    rng = np.random.default_rng(seed)
    pos = torch.from_numpy(pos_np).to(dev())
    vals = torch.from_numpy(rng.standard_normal((n, v)).astype(np.float32)).to(dev()).to(dtype)
    grad = torch.from_numpy(rng.standard_normal((n, v)).astype(np.float32)).to(dev()).to(dtype)
    lat = L.Lattice(sigmas=[1.0] * 3, capacity=max(64, 8 * n), device=dev())
    for _ in range(builds):  # (the dense hint follows the vertex count of the previous build)
        lv, _, idx, w = L.SplatLattice.apply(lat, pos, vals)
    m = lat.nr_lattice_vertices()
    idx_np, w_np = N(idx), N(w)
    assert lv.dtype == torch.float32 and 0 < m <= 4 * n and idx_np.min() >= 0 and idx_np.max() == m - 1
    counts = np.bincount(idx_np, minlength=m)

    ref, mag = scatter64(N(vals.float()), idx_np, w_np, lv.shape[0])
    close_terms(N(lv), ref, mag)

    acc = torch.zeros((m, v), dtype=torch.float32, device=dev())  # the fp32 accumulator of the slice backward
    lat._scatter_rows(grad, idx, w, acc, v, 4, v)
    gref, gmag = scatter64(N(grad.float()), idx_np, w_np, m)
    close_terms(N(acc), gref, gmag)

    values = torch.from_numpy(rng.standard_normal((m, v)).astype(np.float32)).to(dev()).to(dtype).requires_grad_(True)
    out = L.SliceLattice.apply(values, lat, pos, idx, w)
    out.backward(grad)
    got = N(values.grad.float())
    if dtype == torch.float16:  # the fp32 sum rounded to fp16 once
        err = np.abs(got - gref)
        lim = rounded_sum_limit(gref, gmag)
        assert np.all(err <= lim), float(np.max(err - lim))
    else:
        close_terms(got, gref, gmag)
    return counts


@pytest.mark.parametrize("name", ["wave7", "cell600", "lidar3000", "padded5"])
def test_chain_instance_fp32_matches_fp64(name):
    with reduce_mode("plain"):
        counts = splat_and_slice_backward(cloud(name), 32, torch.float32, seed=len(name))
    if name == "wave7":
        assert counts.sum() == 28 and counts.max() <= 16  # every row is one segment: the last wave is partly filled, nothing to combine
    if name == "cell600":
        assert counts.max() > 16 * 8 * 4  # one row over more segments than a workgroup holds: combine rounds, wave ends, atomics
    if name == "lidar3000":
        assert counts.max() > 32 and (counts == 1).any()
    if name == "padded5":
        assert (counts % 4 != 0).any()  # a last batch of fewer than 4 entries


def test_chain_instance_fp16_x64_dense_matches_fp64():
    """64 fp16 channels, 600 points in one cell, second build: the dense hint is set (k_reduce_and_neighbours<8, 3, true, true, 8, CHAIN>,
    k_csr_reduce_segments<8, true, true, 8, CHAIN>); the first build's splat (no hint yet) takes the generic instance."""
    counts = splat_and_slice_backward(cloud("cell600"), 64, torch.float16, seed=11, builds=2)
    assert 2400 >= 16 * len(counts)
    splat_and_slice_backward(cloud("cell600"), 64, torch.float16, seed=12, builds=1)


def test_24_channels_fall_back_to_the_generic_instance():
    for name in ("cell600", "lidar3000"):
        with reduce_mode("plain"):
            splat_and_slice_backward(cloud(name), 24, torch.float32, seed=24)


def test_chain_and_generic_instances_agree_bit_for_bit_in_deterministic_mode():
    """Deterministic mode fixes the order of every sum.  The same rows at a row stride of 36 floats are not chain-shaped and run the
    generic eight-lane instance: splat values (fused launch, chain), the chain reduce and the generic reduce must be identical bits."""
    import lattice_net_amd as L
    pos_np = cloud("lidar3000")
    n, v = len(pos_np), 32
    rng = np.random.default_rng(7)
    with reduce_mode("deterministic"):
        pos = torch.from_numpy(pos_np).to(dev())
        vals = torch.from_numpy(rng.standard_normal((n, v)).astype(np.float32)).to(dev())
        lat = L.Lattice(sigmas=[1.0] * 3, capacity=8 * n, device=dev())
        lv, _, idx, w = L.SplatLattice.apply(lat, pos, vals)
        rows = lv.shape[0]
        chain = torch.zeros((rows, v), dtype=torch.float32, device=dev())
        lat._scatter_rows(vals, idx, w, chain, v, 4, v)
        wide = torch.zeros((n, v + 4), dtype=torch.float32, device=dev())
        wide[:, :v] = vals
        generic = torch.zeros((rows, v), dtype=torch.float32, device=dev())
        lat._scatter_rows(wide, idx, w, generic, v, 4, v + 4)
        assert torch.equal(chain, generic)
        assert torch.equal(lv, generic)
        assert float(generic.abs().max()) > 0


def test_an_infinite_point_row_reaches_its_own_vertices_only():
    """+-Inf in one point's features (alternating sign by channel): its vertices get +-Inf channel by channel as the fp64 scatter does,
    every other row stays finite and within the bound — the NaN of a 0 x Inf on a padded entry would show here (the SAFE re-run)."""
    import lattice_net_amd as L
    pos_np = cloud("lidar3000")
    n, v = len(pos_np), 32
    rng = np.random.default_rng(13)
    vals_np = rng.standard_normal((n, v)).astype(np.float32)
    with reduce_mode("plain"):
        pos = torch.from_numpy(pos_np).to(dev())
        lat = L.Lattice(sigmas=[1.0] * 3, capacity=8 * n, device=dev())
        lat.begin_splat()
        idx0, w0 = lat.just_create_verts(pos, True)
        idx_np, w_np = N(idx0), N(w0)
        counts = np.bincount(idx_np)
        # a point whose four weights are positive and one of whose vertices has a count that is no multiple of 4 (a padded batch)
        ok = (w_np.reshape(n, 4) > 0).all(1) & (counts[idx_np.reshape(n, 4)] % 4 != 0).any(1)
        p = int(np.nonzero(ok)[0][0])
        vals_np[p] = np.where(np.arange(v) % 2 == 0, np.inf, -np.inf)
        vals = torch.from_numpy(vals_np).to(dev())
        lv, _, idx, w = L.SplatLattice.apply(lat, pos, vals)
        assert np.array_equal(N(idx), idx_np)
        m = lat.nr_lattice_vertices()
        acc = torch.zeros((m, v), dtype=torch.float32, device=dev())
        lat._scatter_rows(vals, idx, w, acc, v, 4, v)
    ref, mag = scatter64(vals_np, idx_np, w_np, lv.shape[0])
    hit = np.zeros(lv.shape[0], bool)
    hit[idx_np[4 * p:4 * p + 4]] = True
    assert np.isinf(ref[hit]).all() and np.isfinite(ref[~hit]).all()
    for got, r, g in ((N(lv), ref, mag), (N(acc), ref[:m], mag[:m])):
        assert np.array_equal(np.isposinf(got), np.isposinf(r)) and np.array_equal(np.isneginf(got), np.isneginf(r))
        assert not np.isnan(got).any()
        fin = np.isfinite(r)
        close_terms(np.where(fin, got, 0.0), np.where(fin, r, 0.0), g)
