"""GroupNorm per row range (csrc/ln_norm.hip: k_gn_stats_segments, k_gn_apply_segments, k_gn_backward_apply_segments,
k_gn_param_grads_segments) against fp64, and the row ranges of a batch lattice (k_cloud_row_starts) against the host (`pytest -m gpu`).

The reference is dense_reference's GroupNorm reference applied to the rows of each range alone, with its bounds (the path has the same
roundings: a range is blocked from its own first row); grad_gamma / grad_beta are sums over the ranges and get the sum of the ranges'
bounds.  Each test prints its worst error / bound ratios (`pytest -s`); nothing is asserted on those figures."""
import numpy as np
import pytest
import torch

from tests import cloud_batch_reference as B
from tests import dense_reference as R

pytestmark = pytest.mark.gpu

HEIGHT = 400
ROW_STARTS = [0, 1, 38, 38, 337]  # a one-row cloud, an empty cloud, edges inside a thread's 16 rows and inside a pass, 63 padding rows
CHANNELS = (4, 32, 64, 1024)
SENTINEL = 777.0


def dev():
    return torch.device("cuda", 0)


def gpu(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev()).requires_grad_(grad)


def starts_dev(row_starts):
    return torch.tensor([int(v) for v in row_starts], dtype=torch.int32, device=dev())


def gn_module(c, groups, eps, params):
    gn = torch.nn.GroupNorm(groups, c, eps=eps, affine=params[0] is not None).to(dev())
    if params[0] is not None:
        with torch.no_grad():
            gn.weight.copy_(gpu(params[0]))
            gn.bias.copy_(gpu(params[1]))
    return gn


def run(x_np, gy_np, gn, relu, row_starts, rows=None):
    """group_norm_rows over the ranges, forward and backward; every output as NumPy (mean_rstd [B, 2 groups], scale_shift [B, 2 C])."""
    from lattice_net_amd.lattice_blocks import group_norm_rows
    x = gpu(x_np, grad=True)
    rows_dev = None if rows is None else torch.tensor([rows], dtype=torch.int32, device=dev())
    y = group_norm_rows(x, gn, relu, rows_dev, starts_dev(row_starts))
    assert type(y.grad_fn).__name__.startswith("GroupNormSegmentsFunction")
    _, _, mean_rstd, scale_shift = y.grad_fn.saved_tensors
    for p in gn.parameters():
        p.grad = None
    y.backward(gpu(gy_np))
    out = {"y": y, "mean_rstd": mean_rstd, "scale_shift": scale_shift, "grad_x": x.grad}
    if gn.affine:
        out["grad_gamma"], out["grad_beta"] = gn.weight.grad, gn.bias.grad
    return {k: v.detach().cpu().numpy().copy() for k, v in out.items()}


def check_random(x, gy, groups, relu, row_starts, affine=True, eps=1e-5, rows=None, what="", seed=0):
    m, c = x.shape
    gamma, beta = R.gn_params(c, affine, seed)
    got = run(x, gy, gn_module(c, groups, eps, (gamma, beta)), relu, row_starts, rows)
    ratios = B.check_forward(x, got["y"], got["mean_rstd"], got["scale_shift"], gamma, beta, groups, eps, relu, row_starts, rows, what)
    ref, bound = B.backward_reference(x, gy, got["y"], got["mean_rstd"], gamma, groups, relu, row_starts, rows)
    _, live = B.segments(row_starts, m, rows)
    assert not got["grad_x"][live:].any(), f"{what}: grad_x is not zero behind row {live}"
    for name, r_, b_ in zip(("grad_x", "grad_gamma", "grad_beta"), ref, bound):
        if name in got:
            R.assert_within(got[name], r_, b_, f"{what} {name}")
            ratios[name] = R.worst_ratio(got[name], r_, b_)
    return ratios, got


def exact_groups(c):
    """The module's groups where a group then holds an even number of channels (the integer run needs an even number of elements per
    group, and the ranges here have odd numbers of rows), else C / 2."""
    g = B.module_groups(c)
    return g if (c // g) % 2 == 0 else c // 2


def check_exact(c, relu, row_starts, height, what=""):
    """Integers (dense_reference.gn_exact_input per range, the group means of range s moved by s): mean, rstd = 1/2, scale, shift, y and
    the parameter gradients are the integer results bit for bit, grad_x within its bound (it divides by the element count)."""
    groups = exact_groups(c)
    cg = c // groups
    segs, live = B.segments(row_starts, height)
    x, gy = np.full((height, c), 3e30, np.float32), np.full((height, c), -2e30, np.float32)
    gy[:live] = R.gn_exact_grad(live, c)
    for s, (lo, hi) in enumerate(segs):
        x[lo:hi] = R.gn_exact_input(hi - lo, c, groups) + (s % 3)
    gamma, beta = R.gn_exact_params(c)
    got = run(x, gy, gn_module(c, groups, 0.0, (gamma, beta)), relu, row_starts)
    y_ref, dg, db = np.zeros((height, c)), np.zeros(c), np.zeros(c)
    for s, (lo, hi) in enumerate(segs):
        if hi == lo:
            continue
        mean = (np.arange(groups) % 5 - 2 + (s % 3)).astype(np.float64)
        w = f"{what} range {s}"
        R.assert_exact(got["mean_rstd"][s][:groups], mean, f"{w} mean")
        R.assert_exact(got["mean_rstd"][s][groups:] * 2, np.ones(groups), f"{w} 2 rstd")
        a = R.f64(gamma) / 2
        b = R.f64(beta) - np.repeat(mean, cg) * a
        R.assert_exact(got["scale_shift"][s], np.concatenate([a, b]), f"{w} scale_shift")
        y_ref[lo:hi] = R.f64(x[lo:hi]) * a + b
        if relu:
            y_ref[lo:hi] = np.maximum(y_ref[lo:hi], 0)
        g = R.f64(gy[lo:hi]) * ((y_ref[lo:hi] > 0) if relu else 1.0)
        dg += (g * (R.f64(x[lo:hi]) - np.repeat(mean, cg))).sum(0) / 2
        db += g.sum(0)
    R.assert_exact(got["y"], y_ref, f"{what} y")
    R.assert_exact(got["grad_gamma"], dg, f"{what} grad_gamma")
    R.assert_exact(got["grad_beta"], db, f"{what} grad_beta")
    ref, bound = B.backward_reference(x, gy, got["y"], got["mean_rstd"], gamma, groups, relu, row_starts)
    R.assert_within(got["grad_x"], ref[0], bound[0], f"{what} grad_x")
    assert not got["grad_x"][live:].any()


def inputs(m, c, seed, row_starts):
    """Every range with its own mean and spread; garbage behind the last range."""
    x, gy = R.gn_input(m, c, 0.5, 2.0, seed), R.gn_input(m, c, 0.0, 1.0, seed + 1)
    segs, live = B.segments(row_starts, m)
    for s, (lo, hi) in enumerate(segs):
        x[lo:hi] = x[lo:hi] * np.float32(1 + s % 4) + np.float32(3 * (s % 5) - 4)
    x[live:] = 3e30 * np.where(np.arange(c) % 2, -1, 1)
    gy[live:] = -1e30
    return x, gy


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("c", CHANNELS)
def test_segments_random(c, relu):
    x, gy = inputs(HEIGHT, c, 10 * c, ROW_STARTS)
    worst = {}
    for groups, affine in ((B.module_groups(c), True), (1, False)):
        r, _ = check_random(x, gy, groups, relu, ROW_STARTS, affine, what=f"c={c} groups={groups} relu={relu}", seed=c)
        worst.update({k: max(v, worst.get(k, 0.0)) for k, v in r.items()})
    print(f"GroupNorm segments c={c} relu={relu}: worst error / bound {worst}")


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("c", CHANNELS)
def test_segments_exact(c, relu):
    check_exact(c, relu, ROW_STARTS, HEIGHT, what=f"c={c} relu={relu}")


def many_small_ranges():
    sizes = np.random.default_rng(64).integers(1, 10, size=64)
    return [0] + [int(v) for v in np.cumsum(sizes)]


@pytest.mark.parametrize("c", [32, 64])
def test_64_ranges_of_1_to_9_rows(c):
    starts = many_small_ranges()
    height = starts[-1] + 7
    x, gy = inputs(height, c, 5 * c, starts)
    r, _ = check_random(x, gy, B.module_groups(c), True, starts, what=f"64 ranges c={c}", seed=3)
    check_exact(c, True, starts, height, what=f"64 ranges exact c={c}")
    print(f"GroupNorm 64 ranges c={c}: worst error / bound {r}")


@pytest.mark.parametrize("rows", [0, 1, 200, 336, 400])
def test_segments_under_a_device_row_count(rows):
    """rows_dev below row_starts[B]: the ranges end there, everything behind is zero, nothing is read from the dead rows."""
    c = 64
    x, gy = inputs(HEIGHT, c, 7, ROW_STARTS)
    live = min(rows, ROW_STARTS[-1])
    x[live:] = 3e30 * np.where(np.arange(c) % 2, -1, 1)
    gy[live:] = -1e30
    r, got = check_random(x, gy, 32, True, ROW_STARTS, rows=rows, what=f"rows_dev={rows}", seed=5)
    for name in ("y", "grad_x", "grad_gamma", "grad_beta"):
        assert np.isfinite(got[name]).all(), f"rows_dev={rows}: {name} is not finite"
    print(f"GroupNorm segments rows_dev={rows}: worst error / bound {r}")


@pytest.mark.parametrize("c", [32, 1024])
def test_one_cloud_cannot_move_the_others(c):
    """The rows of one cloud multiplied by 1000 and moved by 3000 standard deviations: every output of every other cloud keeps its bits."""
    starts = [0, 150, 151, 300, 300, 389]
    x, gy = inputs(HEIGHT, c, 21, starts)
    groups = B.module_groups(c)
    params = R.gn_params(c, True, 2)
    base = run(x, gy, gn_module(c, groups, 1e-5, params), True, starts)
    segs, live = B.segments(starts, HEIGHT)
    for victim in (0, 1, 4):
        lo, hi = segs[victim]
        x2 = x.copy()
        x2[lo:hi] = x2[lo:hi] * np.float32(1000.0) + np.float32(3000.0 * x[lo:hi].std() * 1000.0)
        got = run(x2, gy, gn_module(c, groups, 1e-5, params), True, starts)
        for s, (a, b) in enumerate(segs):
            if s == victim or a == b:
                continue
            for name in ("y", "grad_x"):
                R.assert_equal_bits(got[name][a:b], base[name][a:b], f"victim {victim}: {name} of range {s}")
            for name in ("mean_rstd", "scale_shift"):
                R.assert_equal_bits(got[name][s], base[name][s], f"victim {victim}: {name} of range {s}")
        assert not np.array_equal(got["y"][lo:hi], base["y"][lo:hi]) or hi - lo == 1  # (a one-row range of one channel per group is beta either way)
        # the statistics over ALL rows do move: what the operator is for
        from lattice_net_amd.lattice_blocks import group_norm_rows
        gn = gn_module(c, groups, 1e-5, params)
        whole = [group_norm_rows(gpu(v[:live]), gn, True).detach().cpu().numpy() for v in (x, x2)]
        other = next(s for s in range(len(segs)) if s != victim and segs[s][1] - segs[s][0] > 1)
        a, b = segs[other]
        assert not np.array_equal(whole[0][a:b], whole[1][a:b])


@pytest.mark.parametrize("c", [32, 96])
def test_one_range_is_the_whole_matrix(c):
    """B = 1, row_starts = [0, M]: within the bounds of the reference the ln_group_norm_forward_rows path is held to — the same meaning."""
    m = 5 * R.gn_rows_per_pass(c) * R.LN_GN_PASSES + 3
    x, gy = R.gn_input(m, c, 0.5, 2.0, 1), R.gn_input(m, c, 0.0, 1.0, 2)
    groups = B.module_groups(c)
    gamma, beta = R.gn_params(c, True, 4)
    got = run(x, gy, gn_module(c, groups, 1e-5, (gamma, beta)), True, [0, m])
    ratios = {"rstd": R.assert_gn_statistics(got["mean_rstd"][0], x, groups, 1e-5, None, "B=1")}
    R.assert_gn_scale_shift(got["scale_shift"][0], got["mean_rstd"][0], gamma, beta, c, groups, "B=1")
    ratios["y"] = R.assert_gn_apply(got["y"], x, got["scale_shift"][0], True, None, "B=1")
    ref, bound = R.gn_backward_reference(x, gy, got["y"] > 0, gamma, got["mean_rstd"][0], groups)
    for name, r_, b_ in zip(("grad_x", "grad_gamma", "grad_beta"), ref, bound):
        R.assert_within(got[name], r_, b_, f"B=1 {name}")
        ratios[name] = R.worst_ratio(got[name], r_, b_)
    # and the existing path on the same input, held to the same reference
    from lattice_net_amd.lattice_blocks import group_norm_rows
    gn = gn_module(c, groups, 1e-5, (gamma, beta))
    xg = gpu(x, grad=True)
    y = group_norm_rows(xg, gn, True)
    _, _, mean_rstd, scale_shift = y.grad_fn.saved_tensors
    y.backward(gpu(gy))
    R.assert_gn_statistics(mean_rstd, x, groups, 1e-5, None, "rows path")
    R.assert_gn_apply(y, x, scale_shift, True, None, "rows path")
    ref, bound = R.gn_backward_reference(x, gy, (y.detach() > 0).cpu().numpy(), gamma, mean_rstd, groups)
    for g_, r_, b_ in zip((xg.grad, gn.weight.grad, gn.bias.grad), ref, bound):
        R.assert_within(g_, r_, b_, "rows path gradients")
    print(f"GroupNorm one range c={c}: worst error / bound {ratios}")


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
def test_sentinels_behind_every_output(relu):
    """The C ABI on buffers with sentinel elements behind every output (and in the mean_rstd / scale_shift rows of the empty range): none
    is touched; the call without next_workspace (its own zero fill) gives the numbers of the alternating protocol."""
    from lattice_net_amd import _lib
    lib = _lib.load()
    c, groups, segs = 64, 32, len(ROW_STARTS) - 1
    x_np, gy_np = inputs(HEIGHT, c, 3, ROW_STARTS)
    gamma, beta = R.gn_params(c, True, 9)
    x, gy, w, b, starts = gpu(x_np), gpu(gy_np), gpu(gamma), gpu(beta), starts_dev(ROW_STARTS)

    def buf(n):
        return torch.full((n + 64,), SENTINEL, dtype=torch.float32, device=dev())

    y, dx, mr, ss, dg, db = buf(HEIGHT * c), buf(HEIGHT * c), buf(segs * 2 * groups), buf(segs * 2 * c), buf(c), buf(c)
    nbytes = int(lib.ln_group_norm_segments_workspace_bytes(c, segs))
    ws = torch.full((nbytes // 8 + 8,), 5.0, dtype=torch.float64, device=dev())  # (dirty: the call zero-fills what it accumulates into)
    stream = _lib.stream_ptr(dev())
    _lib.check(lib.ln_group_norm_forward_segments(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), HEIGHT, c, groups, 1e-5, int(relu), _lib.ptr(y), _lib.ptr(mr),
                                                  _lib.ptr(ss), _lib.ptr(ws), nbytes, None, 0, None, _lib.ptr(starts), segs, stream), "forward")
    _lib.check(lib.ln_group_norm_backward_segments(_lib.ptr(x), _lib.ptr(gy), _lib.ptr(w), _lib.ptr(mr), _lib.ptr(ss), HEIGHT, c, groups, int(relu),
                                                   _lib.ptr(dx), _lib.ptr(dg), _lib.ptr(db), _lib.ptr(ws), nbytes, None, 0, None, _lib.ptr(starts),
                                                   segs, stream), "backward")
    torch.cuda.synchronize()
    for name, t, n in (("y", y, HEIGHT * c), ("grad_x", dx, HEIGHT * c), ("mean_rstd", mr, segs * 2 * groups), ("scale_shift", ss, segs * 2 * c),
                       ("grad_gamma", dg, c), ("grad_beta", db, c)):
        assert bool((t[n:] == SENTINEL).all()), f"{name}: a sentinel behind the output was overwritten"
    assert bool((ws[nbytes // 8:] == 5.0).all()), "the workspace was written behind its size"
    assert bool((mr[2 * 2 * groups:3 * 2 * groups] == SENTINEL).all()) and bool((ss[2 * 2 * c:3 * 2 * c] == SENTINEL).all()), \
        "the empty range wrote statistics"
    got = {"y": y[:HEIGHT * c].view(HEIGHT, c), "grad_x": dx[:HEIGHT * c].view(HEIGHT, c), "mean_rstd": mr[:segs * 2 * groups].view(segs, -1),
           "scale_shift": ss[:segs * 2 * c].view(segs, -1), "grad_gamma": dg[:c], "grad_beta": db[:c]}
    got = {k: v.cpu().numpy() for k, v in got.items()}
    B.check_forward(x_np, got["y"], got["mean_rstd"], got["scale_shift"], gamma, beta, groups, 1e-5, relu, ROW_STARTS, None, "raw")
    ref, bound = B.backward_reference(x_np, gy_np, got["y"], got["mean_rstd"], gamma, groups, relu, ROW_STARTS)
    for name, r_, b_ in zip(("grad_x", "grad_gamma", "grad_beta"), ref, bound):
        R.assert_within(got[name], r_, b_, f"raw {name}")


@pytest.mark.parametrize("calls", [3, 4])
def test_alternating_workspaces_with_and_without_ranges(calls):
    """Calls over ranges and over the whole matrix share the accumulator pair of the stream: each one zeroes what the other dirtied."""
    from lattice_net_amd.lattice_blocks import group_norm_rows
    c, groups = 64, 32
    x_np, gy_np = inputs(HEIGHT, c, 13, ROW_STARTS)
    params = R.gn_params(c, True, 1)
    for k in range(calls):
        check_random(x_np, gy_np, groups, True, ROW_STARTS, what=f"call {k}", seed=1)
        gn = gn_module(c, groups, 1e-5, params)
        xg = gpu(x_np[:337], grad=True)
        y = group_norm_rows(xg, gn, True)
        _, _, mean_rstd, scale_shift = y.grad_fn.saved_tensors
        R.assert_gn_statistics(mean_rstd, x_np[:337], groups, 1e-5, None, f"whole matrix after call {k}")
        R.assert_gn_apply(y, x_np[:337], scale_shift, True, None, f"whole matrix after call {k}")
        if k % 2:
            y.backward(gpu(gy_np[:337]))  # (an odd number of launches in between)


def test_group_norm_rows_refuses_ranges_it_cannot_run():
    from lattice_net_amd.lattice_blocks import group_norm_rows
    gn = torch.nn.GroupNorm(3, 6).to(dev())
    with pytest.raises(ValueError, match="per row range"):
        group_norm_rows(torch.zeros((10, 6), device=dev()), gn, False, None, starts_dev([0, 10]))  # channels % 4
    gn = torch.nn.GroupNorm(4, 8).to(dev())
    with pytest.raises(ValueError, match="per row range"):
        group_norm_rows(torch.zeros((10, 8), device=dev()), gn, False, None, torch.tensor([0, 10], device=dev()))  # int64
    with pytest.raises(ValueError, match="per row range"):
        group_norm_rows(torch.zeros((10, 8), device=dev()), gn, False, None, starts_dev(range(67)))  # more than 64 ranges


# ------------------------------------------------------------------------------------------------------------------ ranges of a batch lattice
def batch_clouds(clouds, n0, seed):
    """Clouds of unequal extent around the origin."""
    rng = np.random.default_rng(seed)
    return np.concatenate([(rng.uniform(-1.0, 1.0, (n0, 3)) * (0.6 + 0.7 * c)).astype(np.float32) for c in range(clouds)])


@pytest.mark.parametrize("static", [False, True], ids=["eager", "static_rows"])
def test_cloud_row_starts_of_every_level(static):
    """4 clouds x 200 points, d = 3, canonical rows (the suite's conftest), three levels: cloud_row_starts() of every level equals the ranges the host computes from the splat
    indices of that level copied back, and from the keys; the order flag is 0."""
    import lattice_net_amd as L
    clouds, n0 = 4, 200
    pos = gpu(batch_clouds(clouds, n0, 0))
    lat = L.Lattice(sigmas=[0.25] * 3, capacity=20000, device=dev())
    lat.set_cloud_batch(n0, per_cloud_norm=True)
    if static:
        lat.set_static_rows(6144, coarse_bounds=[4096, 4096])
    level, sizes = lat, []
    for lvl in range(3):
        if lvl == 0:
            level.just_create_verts(pos, False)
        else:
            level = level.create_coarse_verts_naive(pos)
        starts = level.cloud_row_starts()
        assert starts.dtype == torch.int32 and tuple(starts.shape) == (clouds + 1,) and starts.is_cuda
        assert level.cloud_row_starts().data_ptr() == starts.data_ptr(), "not cached with the table structure"
        assert level.per_cloud_norm_row_starts().data_ptr() == starts.data_ptr() and level.cloud_segments() == clouds
        got = starts.cpu().numpy()
        m = int(level.m_hash_table.m_nr_filled_tensor.item())
        assert got[0] == 0 and got[-1] == m and int(level.cloud_row_order_flag().item()) == 0
        # the ranges from the splat indices: a retrieval of the same positions on this level (every point finds its d + 1 vertices)
        clone = L.Lattice._clone_of(level)
        clone.m_hash_table.m_values_tensor = torch.zeros((level.nr_lattice_vertices(), 4), device=dev())
        _, idx, _ = clone.slice_standalone_no_precomputation(pos)
        want, flag = B.row_starts_of_splat_indices(idx.cpu().numpy(), n0, 4, clouds, m)
        assert flag == 0 and np.array_equal(got, want), (lvl, got, want)
        # and from the keys, the way the kernel reads them
        keys = level.m_hash_table.m_keys_tensor[:m].cpu().numpy()
        step = level.m_hash_table._batch[1]
        want_k, flag_k = B.row_starts_of_clouds(B.cloud_of_key(keys[:, 0], step, clouds), clouds)
        assert flag_k == 0 and np.array_equal(got, want_k)
        sizes.append(np.diff(got))
    assert all((s > 0).all() for s in sizes) and len({tuple(s) for s in sizes}) == 3, sizes  # (unequal clouds, every level its own ranges)


def test_cloud_row_starts_needs_first_occurrence_rows():
    """With the default row order the call raises on the host."""
    from lattice_net_amd import _lib
    from lattice_net_amd import lattice as L
    from lattice_net_amd.lattice_blocks import GroupNormLatticeModule
    prev = L.set_row_order("slot")  # (the shipped default; the suite's conftest runs everything else under "canonical")
    try:
        lat = L.Lattice(sigmas=[0.25] * 3, capacity=20000, device=dev())
        lat.set_cloud_batch(200, per_cloud_norm=True)
        lat.just_create_verts(gpu(batch_clouds(4, 200, 0)), False)
        with pytest.raises(_lib.LatticeNetHipError, match="canonical"):
            lat.cloud_row_starts()
        gn = GroupNormLatticeModule(32, device=dev())
        with pytest.raises(_lib.LatticeNetHipError, match="canonical"):
            gn(torch.zeros((lat.nr_lattice_vertices(), 32), device=dev()), lat)
    finally:
        L.set_row_order(prev)
