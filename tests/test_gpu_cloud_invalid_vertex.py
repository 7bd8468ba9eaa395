"""The per-cloud "invalid vertex" of a batch of clouds in one lattice (`pytest -m gpu`): ln_distribute_centre_clouds and
ln_pointnet_reduce_forward_clouds against the NumPy restatement (tests/cloud_invalid_vertex_reference.py) and against the
single-cloud entry points run on every cloud's own lattice, ln_pointnet_reduce_backward on the batch's winners, hand-made row
ranges through the C ABI, and the switch Lattice.set_cloud_batch(per_cloud_invalid_vertex=True) at the modules.

Select, copy, subtract and divide kernels: every comparison is bit for bit.  The position sums are an INPUT of the centring entry
points; they are formed on the host here (fp64, rounded once), so that the batch and the single clouds are handed the same numbers."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cloud_batch_reference as B
from tests import cloud_invalid_vertex_reference as V

pytestmark = pytest.mark.gpu

N0, LAST, CLOUDS, SIGMA = 200, 37, 5, 0.3
WIDTH, POS_DIM, SENTINEL = 5, 3, 777.0


def dev():
    return torch.device("cuda", 0)


def gpu(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev()) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev(), dtype)


def host_sums(d, idx, rows):
    sums = np.zeros((rows, POS_DIM))
    np.add.at(sums, idx[idx >= 0], d[idx >= 0, :POS_DIM].astype(np.float64))
    return sums.astype(np.float32)


def distribute(lat, pos, vals):
    """(lattice, distributed [tokens, 5], idx, rows, sums, counts) of a build of `pos` in `lat`."""
    from lattice_net_amd.lattice_funcs import DistributeLattice
    wrap, distributed, idx, _ = DistributeLattice.apply(lat, pos, vals, True)
    dl = wrap.lattice
    rows = dl.nr_lattice_vertices()
    counts = dl.vertex_point_counts(idx)
    sums = gpu(host_sums(distributed.cpu().numpy(), idx.cpu().numpy(), rows))
    return dict(lat=dl, d=distributed, idx=idx, rows=rows, sums=sums, counts=counts, tokens=idx.numel())


def centre(b, row_starts=None, tokens_per_cloud=0, clouds=0):
    """ln_distribute_centre / _clouds into a buffer with four sentinel rows behind it."""
    from lattice_net_amd import _lib
    lib = _lib.load()
    out = torch.full((b["tokens"] + 4, WIDTH), SENTINEL, device=dev())
    head = (_lib.ptr(b["d"]), _lib.ptr(b["idx"]), _lib.ptr(b["sums"]), _lib.ptr(b["counts"]), b["tokens"], WIDTH, POS_DIM)
    if row_starts is None:
        rc = lib.ln_distribute_centre(*head, _lib.ptr(out), _lib.stream_ptr(dev()))
    else:
        rc = lib.ln_distribute_centre_clouds(*head, tokens_per_cloud, _lib.ptr(row_starts), clouds, _lib.ptr(out), _lib.stream_ptr(dev()))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[b["tokens"]:] == SENTINEL).all(), "rows behind the output were written"
    return rc, out[:b["tokens"]]


def reduce(b, src, row_starts=None, clouds=0, rows=None):
    """ln_pointnet_reduce_forward / _clouds over the token adjacency of b["idx"], sentinel rows behind out and out_arg."""
    from lattice_net_amd import _lib
    lib = _lib.load()
    rows = b["rows"] if rows is None else rows
    c = src.shape[1]
    _, csr, max_seg, grp_row, _ = b["lat"]._csr(b["idx"])
    ws = torch.empty((lib.ln_pointnet_reduce_workspace_bytes(rows, c),), dtype=torch.uint8, device=dev())
    out = torch.full((rows + 4, 2 * c), SENTINEL, device=dev())
    arg = torch.full((rows + 4, c), 12345, dtype=torch.int32, device=dev())
    head = (C.byref(csr), _lib.ptr(grp_row), max_seg, _lib.ptr(src), c, b["d"].data_ptr() + 4 * (WIDTH - 1), WIDTH, rows, 4, _lib.ptr(ws),
            ws.numel(), _lib.ptr(out), _lib.ptr(arg))
    if row_starts is None:
        rc = lib.ln_pointnet_reduce_forward(*head, _lib.stream_ptr(dev()))
    else:
        rc = lib.ln_pointnet_reduce_forward_clouds(*head, _lib.ptr(row_starts), clouds, _lib.stream_ptr(dev()))
    torch.cuda.synchronize()
    out, arg = out.cpu().numpy(), arg.cpu().numpy()
    assert (out[rows:] == SENTINEL).all() and (arg[rows:] == 12345).all(), "rows behind the outputs were written"
    return rc, out[:rows], arg[:rows]


def backward(grad_out, arg, idx, tokens, c):
    from lattice_net_amd import _lib
    g = torch.full((tokens + 4, c), SENTINEL, device=dev())
    rc = _lib.load().ln_pointnet_reduce_backward(_lib.ptr(grad_out), grad_out.shape[1], _lib.ptr(arg), _lib.ptr(idx), tokens, c, _lib.ptr(g),
                                                 _lib.stream_ptr(dev()))
    torch.cuda.synchronize()
    g = g.cpu().numpy()
    assert rc == 0 and (g[tokens:] == SENTINEL).all()
    return g[:tokens]


@pytest.fixture(scope="module")
def data():
    """d = 3; 4 clouds x 200 points and a fifth of 37 (n is no multiple of n0); the first 8 points of every cloud are its point 0
    displaced by 1e-3 sigma, so that every cloud's first vertex holds at least 4 tokens and the rule shows.  The batch in one lattice,
    every cloud in a lattice of its own (computed once, never changed)."""
    import lattice_net_amd as L
    from lattice_net_amd import lattice as LL
    rng = np.random.default_rng(5)
    clouds = []
    for c in range(CLOUDS):
        n = N0 if c < CLOUDS - 1 else LAST
        p = rng.uniform(-1.0, 1.0, (n, 3)) * (0.6 + 0.3 * c)
        p[1:8] = p[0] + 1e-3 * SIGMA * rng.standard_normal((7, 3))
        clouds.append(p.astype(np.float32))
    pos = np.concatenate(clouds)
    vals = rng.standard_normal((pos.shape[0], 1)).astype(np.float32)
    prev_order, prev_det = LL.set_row_order("canonical"), LL.set_deterministic(True)
    try:
        lat = L.Lattice(sigmas=[SIGMA] * 3, capacity=20000, device=dev())
        lat.set_cloud_batch(N0, per_cloud_invalid_vertex=True)
        batch = distribute(lat, gpu(pos), gpu(vals))
        batch["starts"] = batch["lat"].per_cloud_invalid_row_starts()
        assert batch["lat"].per_cloud_norm_row_starts() is None  # (the two switches are independent)
        singles = []
        for c in range(CLOUDS):
            sl = slice(c * N0, min((c + 1) * N0, pos.shape[0]))
            singles.append(distribute(L.Lattice(sigmas=[SIGMA] * 3, capacity=20000, device=dev()), gpu(pos[sl]), gpu(vals[sl])))
        torch.cuda.synchronize()
    finally:
        LL.set_row_order(prev_order)
        LL.set_deterministic(prev_det)
    src = {c: gpu(rng.standard_normal((batch["tokens"], c)).astype(np.float32).round(1)) for c in (16, 32, 5)}
    return dict(batch=batch, singles=singles, src=src, tpc=N0 * (POS_DIM + 1), pos=gpu(pos), vals=gpu(vals))


def test_the_batch_is_what_the_rule_needs(data):
    """The ranges the device wrote are the ranges of the splat indices; every cloud's first vertex holds at least 4 tokens (else the
    rule is invisible); every cloud's own lattice is the batch's range, rebased, with the same token rows."""
    b = data["batch"]
    starts = b["starts"].cpu().numpy()
    idx = b["idx"].cpu().numpy()
    exp, flag = B.row_starts_of_splat_indices(idx, N0, POS_DIM + 1, CLOUDS, b["rows"])
    assert flag == 0 and list(starts) == list(exp) and starts[-1] == b["rows"]
    counts = b["counts"].cpu().numpy()
    assert (counts[starts[:-1]] >= 4).all(), counts[starts[:-1]]
    assert b["lat"].points_per_cloud() == N0
    for c, s in enumerate(data["singles"]):
        t0 = c * data["tpc"]
        assert s["rows"] == starts[c + 1] - starts[c]
        si = s["idx"].cpu().numpy()
        assert np.array_equal(np.where(si >= 0, si + starts[c], -1), idx[t0:t0 + s["tokens"]])
        assert torch.equal(s["d"], b["d"][t0:t0 + s["tokens"]]) and torch.equal(s["sums"], b["sums"][starts[c]:starts[c + 1]])
        assert torch.equal(s["counts"], b["counts"][starts[c]:starts[c + 1]])


def test_distribute_centre_clouds_on_a_batch(data):
    b = data["batch"]
    rc, got = centre(b, b["starts"], data["tpc"], CLOUDS)
    assert rc == 0
    starts = b["starts"].cpu().numpy()
    idx = b["idx"].cpu().numpy()
    exp = V.distribute_centre(b["d"].cpu().numpy(), idx, b["sums"].cpu().numpy(), b["counts"].cpu().numpy(), POS_DIM, data["tpc"], starts)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    for c, s in enumerate(data["singles"]):
        t0 = c * data["tpc"]
        rc, alone = centre(s)
        assert rc == 0 and np.array_equal(got[t0:t0 + s["tokens"]].view(np.uint32), alone.view(np.uint32)), f"cloud {c}"
        first = idx[t0:t0 + s["tokens"]] == starts[c]
        assert first.sum() >= 4 and not got[t0:t0 + s["tokens"]][first].any()
    # the row-0 rule on the batch keeps the tokens of the first vertices of clouds >= 1: what the switch changes
    rc, row0 = centre(b)
    later = np.isin(idx, starts[1:-1])
    assert rc == 0 and row0[later].any() and not got[later].any() and np.array_equal(row0[~later], got[~later])


@pytest.mark.parametrize("channels", [16, 32, 5])  # vec4 segment max (16, 32), scalar (5)
def test_pointnet_reduce_clouds_on_a_batch(data, channels):
    b, src = data["batch"], data["src"][channels]
    rc, out, arg = reduce(b, src, b["starts"], CLOUDS)
    assert rc == 0
    starts = b["starts"].cpu().numpy()
    idx = b["idx"].cpu().numpy()
    eo, ea, ec = V.pointnet_reduce(src.cpu().numpy(), idx, b["d"].cpu().numpy()[:, -1], b["rows"], 4, starts)
    assert np.array_equal(ec, b["counts"].cpu().numpy())
    assert np.array_equal(out.view(np.uint32), eo.view(np.uint32)) and np.array_equal(arg, ea)
    assert not out[starts[:-1]].any() and (arg[starts[:-1]] == -1).all()
    kept = (ec >= 4) & ~V.invalid_rows(starts, b["rows"])
    assert kept.sum() > CLOUDS and (arg[kept] >= 0).all() and out[kept].any(axis=1).all()
    rng = np.random.default_rng(channels)
    grad_out = gpu(rng.standard_normal((b["rows"], 2 * channels)).astype(np.float32))
    grad = backward(grad_out, gpu(arg), b["idx"], b["tokens"], channels)
    assert np.array_equal(grad, V.pointnet_reduce_backward(grad_out.cpu().numpy(), arg, idx, b["tokens"]))
    assert grad.any() and not grad[np.isin(idx, starts[:-1])].any()  # every token of every dropped vertex: exactly zero
    for c, s in enumerate(data["singles"]):
        t0, t1 = c * data["tpc"], c * data["tpc"] + s["tokens"]
        r0, r1 = starts[c], starts[c + 1]
        rc, so, sa = reduce(s, src[t0:t1].contiguous())
        assert rc == 0 and np.array_equal(out[r0:r1].view(np.uint32), so.view(np.uint32)), f"cloud {c}"
        assert np.array_equal(arg[r0:r1], np.where(sa >= 0, sa + t0, -1)), f"cloud {c}"
        sg = backward(grad_out[r0:r1].contiguous(), gpu(sa), s["idx"], s["tokens"], channels)
        assert np.array_equal(grad[t0:t1].view(np.uint32), sg.view(np.uint32)), f"cloud {c}"
    # the row-0 rule on the batch keeps the first vertices of clouds >= 1
    rc, out0, arg0 = reduce(b, src)
    assert rc == 0 and out0[starts[1:-1]].any(axis=1).all() and (arg0[starts[1:-1]] >= 0).all()
    rest = np.ones(b["rows"], bool)
    rest[starts[1:-1]] = False
    assert np.array_equal(out0[rest], out[rest]) and np.array_equal(arg0[rest], arg[rest])


HAND_MADE = {
    "empty, one-row and a short end": ([5, 0, 1, 7, 0, 3], 6),   # empty ranges, a range of one row, 6 rows behind row_starts[B]
    "64 ranges of 1-9 rows": (list(np.random.default_rng(64).integers(1, 10, 64)), 0),
    "one range": ([23], 2),
}


@pytest.mark.parametrize("case", list(HAND_MADE))
@pytest.mark.parametrize("channels", [32, 5])
def test_hand_made_row_starts(data, case, channels):
    """row_starts written by hand, through the C ABI: tokens of a range point into it or nowhere; the rows from row_starts[B] on have no
    token and come out as zeros."""
    sizes, extra = HAND_MADE[case]
    tpc = 96
    h = V.make_batch(sizes, tpc, ch=channels, seed=len(sizes) + channels, short_last=11)
    rows = h["rows"] + extra
    b = dict(lat=data["batch"]["lat"], d=gpu(h["d"]), idx=gpu(h["idx"], torch.int32), rows=rows, tokens=h["tokens"],
             sums=gpu(np.concatenate([h["sums"], np.ones((extra, POS_DIM), np.float32)])),
             counts=gpu(np.concatenate([h["counts"], np.zeros(extra, np.int64)]), torch.int32))
    starts = gpu(h["starts"], torch.int32)
    clouds = len(sizes)
    rc, got = centre(b, starts, tpc, clouds)
    exp = V.distribute_centre(h["d"], h["idx"], b["sums"].cpu().numpy(), b["counts"].cpu().numpy(), POS_DIM, tpc, h["starts"])
    assert rc == 0 and np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    src = gpu(h["src"])
    rc, out, arg = reduce(b, src, starts, clouds, rows=rows)
    eo, ea, ec = V.pointnet_reduce(h["src"], h["idx"], h["d"][:, -1], rows, 4, h["starts"])
    assert rc == 0 and np.array_equal(out.view(np.uint32), eo.view(np.uint32)) and np.array_equal(arg, ea)
    first = np.array([s for s, m in zip(h["starts"][:-1], sizes) if m > 0])
    assert (ec[first] >= 4).all() and not out[first].any() and (arg[first] == -1).all()
    assert not out[h["rows"]:].any() and (arg[h["rows"]:] == -1).all()
    assert out.any() or max(sizes) == 1
    grad_out = gpu(np.random.default_rng(1).standard_normal((rows, 2 * channels)).astype(np.float32))
    grad = backward(grad_out, gpu(arg), b["idx"], b["tokens"], channels)
    assert np.array_equal(grad, V.pointnet_reduce_backward(grad_out.cpu().numpy(), arg, h["idx"], h["tokens"]))
    assert not grad[np.isin(h["idx"], first)].any()


def test_more_than_64_clouds_is_refused_and_launches_nothing(data):
    b = data["batch"]
    starts = gpu(np.arange(66), torch.int32)
    rc, got = centre(b, starts, 4, 65)
    assert rc == -2 and (got == SENTINEL).all()
    rc, out, arg = reduce(b, data["src"][16], starts, 65)
    assert rc == -2 and (out == SENTINEL).all() and (arg == 12345).all()


def modules(pos, vals, per_cloud, grad_through_distributed=False):
    """DistributeLatticeModule -> PointNetModule on the batch: (centred token rows, splat indices, the reduced rows entering the last
    convolution, the row ranges)."""
    import lattice_net_amd as L
    import lattice_net_amd.lattice_modules as M
    lat = L.Lattice(sigmas=[SIGMA] * 3, capacity=20000, device=dev())
    lat.set_cloud_batch(N0, per_cloud_invalid_vertex=per_cloud)
    dl, distributed, idx, _ = M.DistributeLatticeModule()(lat, pos, vals)
    if grad_through_distributed:
        distributed = distributed.clone().requires_grad_(True)
    torch.manual_seed(0)
    pn = M.PointNetModule([16, 32], 32, nr_input_channels=WIDTH - 1, device=dev())
    seen = {}
    pn.last_conv.register_forward_pre_hook(lambda mod, args: seen.__setitem__("in", args[0].detach().clone()))
    pn(dl, distributed, idx)
    return distributed.detach().cpu().numpy(), idx.cpu().numpy(), seen["in"].cpu().numpy(), dl.cloud_row_starts().cpu().numpy()


@pytest.fixture
def deterministic_mode():
    from lattice_net_amd import lattice as L
    prev = L.set_deterministic(True)  # (position sums in a fixed order: two runs of the module agree bit for bit)
    yield
    L.set_deterministic(prev)


def test_the_switch_at_the_modules(data, deterministic_mode):
    """Off: the first vertices of clouds >= 1 keep their tokens' rows and their PointNet feature (what the code computed before the
    switch existed).  On: they are zero, like cloud 0's.  Everything else is the same bit for bit."""
    import lattice_net_amd.lattice_modules as M
    pos, vals = data["pos"], data["vals"]
    d_off, idx, red_off, starts = modules(pos, vals, False)
    d_on, idx_on, red_on, starts_on = modules(pos, vals, True)
    assert np.array_equal(idx, idx_on) and np.array_equal(starts, starts_on) and len(starts) == CLOUDS + 1
    later = starts[1:-1]
    counts = np.bincount(idx[idx >= 0], minlength=starts[-1])
    assert (counts[starts[:-1]] >= 4).all()
    assert red_off[later].any(axis=1).all() and d_off[np.isin(idx, later)].any(axis=1).all()
    assert not red_on[starts[:-1]].any() and not d_on[np.isin(idx, starts[:-1])].any()
    assert not red_off[0].any() and not d_off[idx == 0].any()  # cloud 0's first vertex is row 0: dropped either way
    rest = np.ones(red_on.shape[0], bool)
    rest[later] = False
    assert np.array_equal(red_on[rest], red_off[rest]) and np.array_equal(d_on[~np.isin(idx, later)], d_off[~np.isin(idx, later)])
    # the rule lives in the fused kernels only: where a module cannot take them it says so
    for entry in ("distribute", "pointnet"):
        M.FUSED_GLUE = {"weight_norm", "distribute", "pointnet"} - {entry}
        try:
            with pytest.raises(ValueError, match="per_cloud_invalid_vertex"):
                modules(pos, vals, True)
            modules(pos, vals, False)  # the torch chains stay as they are
        finally:
            M.FUSED_GLUE = {"weight_norm", "distribute", "pointnet"}
    with pytest.raises(ValueError, match="per_cloud_invalid_vertex"):
        modules(pos, vals, True, grad_through_distributed=True)
