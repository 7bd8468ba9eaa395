"""The invalid vertex of every cloud beyond 64 clouds (`pytest -m gpu`): ln_pointnet_reduce_forward_many_clouds (beyond 64 clouds
k_pointnet_reduce_decode_many_clouds: the starts in LDS, a binary search per row) and ln_distribute_centre_many_clouds against the
NumPy restatement of tests/cloud_invalid_vertex_reference.py, bit for bit, on row ranges written by hand through the C ABI; and
Lattice.cloud_row_starts() of a lattice built from 130 clouds (set_cloud_batch(many_clouds=True)) against the clouds built alone.

Select, copy, subtract and divide kernels: every comparison is exact.  A library without the many-clouds forms has none of these
entry points: every case fails."""
import numpy as np
import pytest
import torch

from tests import cloud_invalid_vertex_reference as V
from tests import test_gpu_cloud_invalid_vertex as T

pytestmark = pytest.mark.gpu

POS_DIM = T.POS_DIM


def many(fn, *args, **kw):
    """T.centre / T.reduce with the *_many_clouds entry points in the place of the *_clouds ones they call (same arguments)."""
    from lattice_net_amd import _lib
    lib = _lib.load()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(lib, "ln_distribute_centre_clouds", lib.ln_distribute_centre_many_clouds)
        mp.setattr(lib, "ln_pointnet_reduce_forward_clouds", lib.ln_pointnet_reduce_forward_many_clouds)
        return fn(*args, **kw)


def ragged_sizes():
    """130 clouds of 0 ... 40 rows, empty ones at the front, in the middle (two neighbours) and at the end."""
    sizes = np.random.default_rng(130).integers(0, 41, 130)
    sizes[[0, 1, 64, 65, 129]] = 0
    sizes[[2, 128]] = (40, 1)
    return [int(v) for v in sizes]


HAND_MADE = {
    "65 clouds of 1-9 rows": (list(np.random.default_rng(65).integers(1, 10, 65)), 0),
    "130 clouds of 24 rows": ([24] * 130, 3),
    "130 ragged clouds": (ragged_sizes(), 5),
    "1024 clouds of 0-3 rows": (list(np.random.default_rng(1024).integers(0, 4, 1024)), 2),  # (the LDS copy is full: 1025 starts)
}


@pytest.mark.parametrize("case", list(HAND_MADE))
@pytest.mark.parametrize("channels", [32, 5])  # (at 5 channels a workgroup's 256 elements span 52 rows, at 32 eight)
def test_hand_made_row_starts_beyond_64_clouds(case, channels):
    sizes, extra = HAND_MADE[case]
    tpc = 48
    h = V.make_batch(sizes, tpc, ch=channels, seed=len(sizes) + channels, short_last=11)
    rows = h["rows"] + extra
    import lattice_net_amd as L
    lat = L.Lattice(sigmas=[T.SIGMA] * 3, capacity=20000, device=T.dev())  # (reduce() takes the token adjacency builder from a built lattice; its row bound is the capacity)
    lat.just_create_verts(T.gpu(np.random.default_rng(0).uniform(-1.0, 1.0, (50, 3)).astype(np.float32)), False)
    b = dict(lat=lat, d=T.gpu(h["d"]), idx=T.gpu(h["idx"], torch.int32), rows=rows, tokens=h["tokens"],
             sums=T.gpu(np.concatenate([h["sums"], np.ones((extra, POS_DIM), np.float32)])),
             counts=T.gpu(np.concatenate([h["counts"], np.zeros(extra, np.int64)]), torch.int32))
    starts = T.gpu(h["starts"], torch.int32)
    clouds = len(sizes)
    rc, got = many(T.centre, b, starts, tpc, clouds)
    assert T.centre(b, starts, tpc, clouds)[0] == -2  # (the entry point that existed keeps its limit, and launched nothing)
    exp = V.distribute_centre(h["d"], h["idx"], b["sums"].cpu().numpy(), b["counts"].cpu().numpy(), POS_DIM, tpc, h["starts"])
    assert rc == 0 and np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    rc, out, arg = many(T.reduce, b, T.gpu(h["src"]), starts, clouds, rows=rows)
    eo, ea, ec = V.pointnet_reduce(h["src"], h["idx"], h["d"][:, -1], rows, 4, h["starts"])
    assert rc == 0 and np.array_equal(out.view(np.uint32), eo.view(np.uint32)) and np.array_equal(arg, ea)
    first = np.array([s for s, m in zip(h["starts"][:-1], sizes) if m > 0])
    assert (ec[first] >= 4).all() and not out[first].any() and (arg[first] == -1).all()  # (else the rule is invisible)
    assert not out[h["rows"]:].any() and (arg[h["rows"]:] == -1).all()
    kept = (ec >= 4) & ~V.invalid_rows(h["starts"], rows)
    assert out[kept].any() or not kept.any()
    # the instance for up to 64 clouds on the first 64 of them marks the same rows there
    if clouds > 64:
        rc, out64, arg64 = T.reduce(b, T.gpu(h["src"]), T.gpu(h["starts"][:65], torch.int32), 64, rows=rows)
        upto = int(h["starts"][64])
        assert rc == 0 and np.array_equal(out64[:upto].view(np.uint32), out[:upto].view(np.uint32)) and np.array_equal(arg64[:upto], arg[:upto])


@pytest.mark.parametrize("ragged", [False, True], ids=["130x24", "ragged"])
def test_cloud_row_starts_of_130_clouds(ragged):
    """d = 3, canonical rows (the suite's conftest), quotient_step from suggest_quotient_step: the ranges of the batch are the row
    counts of the sampled clouds built alone, and the order flag is 0."""
    import lattice_net_amd as L
    rng = np.random.default_rng(7)
    lengths = [24] * 130
    if ragged:
        lengths = [int(v) for v in rng.integers(1, 41, 130)]
        for i in (0, 1, 70, 129):
            lengths[i] = 0
    clouds = [(rng.uniform(-1.0, 1.0, (n, 3)) * (0.5 + 0.01 * c)).astype(np.float32) for c, n in enumerate(lengths)]
    pos = T.gpu(np.concatenate(clouds))
    sigma = 0.25
    from lattice_net_amd import lattice as LL
    step = LL.suggest_quotient_step(pos, [sigma] * 3, lengths if ragged else 24)
    assert LL.max_clouds_in_key_range(3, step) >= 130
    lat = L.Lattice(sigmas=[sigma] * 3, capacity=40000, device=T.dev())
    lat.set_cloud_batch(lengths if ragged else 24, quotient_step=step, per_cloud_norm=True, per_cloud_invalid_vertex=True, many_clouds=True)
    lat.just_create_verts(pos, False)
    starts = lat.cloud_row_starts().cpu().numpy()
    assert starts.shape == (131,) and starts[0] == 0 and starts[-1] == lat.nr_lattice_vertices()
    assert int(lat.cloud_row_order_flag().item()) == 0
    nonempty = [c for c, n in enumerate(lengths) if n]
    sample = sorted({nonempty[0], nonempty[-1], min(nonempty, key=lengths.__getitem__), max(nonempty, key=lengths.__getitem__), 69, 71, 33, 101})
    for c in sample:
        if not lengths[c]:
            continue
        alone = L.Lattice(sigmas=[sigma] * 3, capacity=40000, device=T.dev())
        alone.just_create_verts(T.gpu(clouds[c]), False)
        assert alone.nr_lattice_vertices() == starts[c + 1] - starts[c], c
    for c, n in enumerate(lengths):
        assert n or starts[c + 1] == starts[c], c


# ------------------------------------------------------------------------------------------ 130 clouds through the modules and models.LNN
from tests import test_gpu_lnn_cloud_batch as K  # noqa: E402  (its cfg, runner and bound)

CLOUDS = 130
NET_SIGMA = 0.9  # (K.CFG)


def batch_lengths(ragged):
    """130 clouds of 24 points, or of 0 ... 40 with empty clouds at the front, in the middle (two neighbours) and at the end."""
    if not ragged:
        return [24] * CLOUDS
    lengths = np.random.default_rng(11).integers(1, 41, CLOUDS)
    lengths[[0, 1, 64, 65, CLOUDS - 1]] = 0
    lengths[[2, 40]] = (40, 1)
    return [int(v) for v in lengths]


def batch_positions(lengths, sigma, seed):
    """Clouds of unequal extent around the origin; the first 8 points of a cloud share a simplex, so that its first vertex passes
    PointNet's four-point rule and only the invalid-vertex rule can drop it."""
    rng = np.random.default_rng(seed)
    clouds = []
    for c, n in enumerate(lengths):
        p = rng.uniform(-1.0, 1.0, (n, 3)) * (2.0 + 0.01 * c)
        if n > 1:
            p[1:8] = p[0] + 1e-3 * sigma * rng.standard_normal((len(p[1:8]), 3))
        clouds.append(p.astype(np.float32))
    return clouds


def sample_of(lengths):
    """8 clouds: first, last, shortest and longest that hold points, the two around the empty pair in the middle, two more."""
    nonempty = [c for c, n in enumerate(lengths) if n]
    around = [max(c for c in nonempty if c < 64), min(c for c in nonempty if c > 65)]
    picked = [nonempty[0], nonempty[-1], min(nonempty, key=lengths.__getitem__), max(nonempty, key=lengths.__getitem__), *around, 33, 101]
    for c in nonempty:  # (a cloud named twice: the next ones that hold points)
        if len(set(picked)) == 8:
            break
        picked.append(c)
    return sorted(set(picked))


@pytest.mark.parametrize("ragged", [False, True], ids=["130x24", "ragged"])
def test_reduce_and_centre_of_sampled_clouds_are_those_of_the_cloud_alone(ragged):
    """The batch built by DistributeLattice in one lattice, 8 of its clouds in lattices of their own: PointNet reduce (and, for equal
    clouds, the centring pass) of the batch through the *_many_clouds entry points are, on the rows and tokens of a sampled cloud, bit
    for bit what the single-cloud entry points give on that cloud's own lattice."""
    import lattice_net_amd as L
    from lattice_net_amd import lattice as LL
    lengths = batch_lengths(ragged)
    clouds = batch_positions(lengths, T.SIGMA, 3)
    pos = np.concatenate(clouds)
    vals = np.random.default_rng(4).standard_normal((pos.shape[0], 1)).astype(np.float32)
    point_starts = np.concatenate([[0], np.cumsum(lengths)])
    prev_order, prev_det = LL.set_row_order("canonical"), LL.set_deterministic(True)
    try:
        step = LL.suggest_quotient_step(T.gpu(pos), [T.SIGMA] * 3, lengths if ragged else 24)
        lat = L.Lattice(sigmas=[T.SIGMA] * 3, capacity=40000, device=T.dev())
        lat.set_cloud_batch(lengths if ragged else 24, quotient_step=step, per_cloud_invalid_vertex=True, many_clouds=True)
        b = T.distribute(lat, T.gpu(pos), T.gpu(vals))
        starts_dev = b["lat"].per_cloud_invalid_row_starts()
        starts = starts_dev.cpu().numpy()
        assert starts.shape == (CLOUDS + 1,) and starts[-1] == b["rows"]
        src = T.gpu(np.random.default_rng(5).standard_normal((b["tokens"], 16)).astype(np.float32).round(1))
        rc, out, arg = many(T.reduce, b, src, starts_dev, CLOUDS)
        assert rc == 0
        got = many(T.centre, b, starts_dev, 24 * (POS_DIM + 1), CLOUDS)[1] if not ragged else None
        idx = b["idx"].cpu().numpy()
        eo, ea, _ = V.pointnet_reduce(src.cpu().numpy(), idx, b["d"].cpu().numpy()[:, -1], b["rows"], 4, starts)
        assert np.array_equal(out.view(np.uint32), eo.view(np.uint32)) and np.array_equal(arg, ea)
        for c in sample_of(lengths):
            s = T.distribute(L.Lattice(sigmas=[T.SIGMA] * 3, capacity=40000, device=T.dev()), T.gpu(clouds[c]),
                             T.gpu(vals[point_starts[c]:point_starts[c + 1]]))
            t0 = int(point_starts[c]) * (POS_DIM + 1)
            t1, r0, r1 = t0 + s["tokens"], starts[c], starts[c + 1]
            assert s["rows"] == r1 - r0, c
            rc, so, sa = T.reduce(s, src[t0:t1].contiguous())
            assert rc == 0 and np.array_equal(out[r0:r1].view(np.uint32), so.view(np.uint32)), f"cloud {c}"
            assert np.array_equal(arg[r0:r1], np.where(sa >= 0, sa + t0, -1)), f"cloud {c}"
            if got is not None:
                rc, alone = T.centre(s)
                assert rc == 0 and np.array_equal(got[t0:t1].view(np.uint32), alone.view(np.uint32)), f"cloud {c}"
    finally:
        LL.set_row_order(prev_order)
        LL.set_deterministic(prev_det)


@pytest.fixture(scope="module")
def net(tmp_path_factory):
    """K's small LNN, GroupNorm parameters moved off their initial 1 / 0 (made once, never changed)."""
    from lattice_net_amd import Lattice, ModelParams
    from lattice_net_amd import lattice as LL
    from lattice_net_amd.models import LNN
    path = tmp_path_factory.mktemp("lnn_many_clouds") / "lnn.cfg"
    path.write_text(K.CFG)
    torch.manual_seed(0)
    Lattice.create(str(path), "lattice")
    model = LNN(K.CLASSES, ModelParams.create(str(path)), device=T.dev())
    warm = batch_positions([300], NET_SIGMA, 0)[0]
    d = {"cfg": str(path), "net": model, "pos": T.gpu(warm), "vals": torch.zeros((300, 1), device=T.dev()),
         "g": torch.zeros((300, K.CLASSES), device=T.dev())}
    prev_order, prev_det = LL.set_row_order("canonical"), LL.set_deterministic(True)
    try:
        K.run(d, None)  # (layers that size themselves from their first input exist from here on)
    finally:
        LL.set_row_order(prev_order)
        LL.set_deterministic(prev_det)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if ".gn." in name or name.endswith("norm.weight") or name.endswith("norm.bias"):
                p.add_(0.3 * torch.randn_like(p))
    d["params"] = list(model.parameters())
    return d


@pytest.mark.parametrize("static", [False, True], ids=["eager", "static_rows"])
@pytest.mark.parametrize("ragged", [False, True], ids=["130x24", "ragged"])
def test_lnn_on_130_clouds_is_the_sampled_clouds_one_at_a_time(net, ragged, static):
    """models.LNN on the batch with both per-cloud switches (many_clouds=True), the scalar a weighted sum of the log-probabilities of
    the 8 sampled clouds' points only: their log-probabilities and every parameter gradient are within K.BOUND (1e-4 of the largest
    magnitude of the single-cloud figures) of the 8 clouds run alone, gradients summed.  With per_cloud_norm off the log-probabilities
    must leave the bound (the sibling test reports 0.064 - 0.15 without the other switch), so the test cannot pass vacuously."""
    from lattice_net_amd import Lattice
    from lattice_net_amd import lattice as LL
    lengths = batch_lengths(ragged)
    pos = T.gpu(np.concatenate(batch_positions(lengths, NET_SIGMA, 1)))
    n = pos.shape[0]
    point_starts = np.concatenate([[0], np.cumsum(lengths)])
    sample = sample_of(lengths)
    g = np.zeros((n, K.CLASSES), np.float32)
    rng = np.random.default_rng(2)
    for c in sample:
        g[point_starts[c]:point_starts[c + 1]] = rng.standard_normal((lengths[c], K.CLASSES))
    d = dict(net, pos=pos, vals=torch.zeros((n, 1), device=T.dev()), g=T.gpu(g))
    prev_order, prev_det = LL.set_row_order("canonical"), LL.set_deterministic(True)
    try:
        step = LL.suggest_quotient_step(pos, [NET_SIGMA] * 3, lengths if ragged else 24)
        assert LL.max_clouds_in_key_range(3, step) >= CLOUDS

        def lattice(norm, invalid):
            lat = Lattice.create(d["cfg"], "lattice")
            lat.set_cloud_batch(lengths if ragged else 24, quotient_step=step, per_cloud_norm=norm, per_cloud_invalid_vertex=invalid, many_clouds=True)
            if static:
                lat.set_static_rows(16384, coarse_bounds=[8192])
            return lat

        ref_out, ref_grads = {}, None
        for c in sample:
            out, gr = K.run(d, None, sl=slice(int(point_starts[c]), int(point_starts[c + 1])))
            ref_out[c] = out
            ref_grads = gr if ref_grads is None else [a if b is None else a + b for a, b in zip(ref_grads, gr)]
        out, grads = K.run(d, None, lattice=lattice(True, True))
        off, _ = K.run(d, None, lattice=lattice(False, True))
    finally:
        LL.set_row_order(prev_order)
        LL.set_deterministic(prev_det)
    figures, without = {}, {}
    for c in sample:
        sl = slice(int(point_starts[c]), int(point_starts[c + 1]))
        figures[f"out cloud {c}"] = K.rel(out[sl], ref_out[c])
        without[c] = K.rel(off[sl], ref_out[c])
    for (name, _), got, ref in zip(d["net"].named_parameters(), grads, ref_grads):
        assert (got is None) == (ref is None), name
        if ref is not None:
            figures[f"grad {name}"] = K.rel(got, ref)
    print(f"LNN on 130 clouds ({'ragged' if ragged else '130x24'}, {'static rows' if static else 'eager'}) against single-cloud runs: worst "
          f"{max(figures.values()):.3e} ({max(figures, key=figures.get)}); without per_cloud_norm, outputs: "
          f"{min(without.values()):.3e} ... {max(without.values()):.3e}")
    bad = {k: v for k, v in figures.items() if not v <= K.BOUND}
    assert not bad, bad
    assert max(without.values()) > K.BOUND, without
