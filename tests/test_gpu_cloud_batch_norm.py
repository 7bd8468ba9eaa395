"""A small Gn-block network on a batch of clouds in one lattice with per-cloud GroupNorm (Lattice.set_cloud_batch(n0,
per_cloud_norm=True)) against the same clouds run one at a time with the same parameters (`pytest -m gpu`).

splat -> GnReluConv -> ResnetBlock -> GnReluCoarsen -> BottleneckBlock -> GnReluFinefy -> SliceLatticeModule, 32 channels, two lattice
levels; no Distribute / PointNet (their "vertex 0 is the invalid bucket" rule names row 0 of the table: out of scope of the per-cloud
norm).  Per-point outputs of every cloud, and parameter gradients against the sum of the single-cloud runs, agree within 1e-4 of the
largest magnitude of the tensor (the project's whole-network bound, README Parity); with per_cloud_norm=False they must not."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CLOUDS, N0, CH = 3, 300, 32
BOUND = 1e-4


def dev():
    return torch.device("cuda", 0)


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        from lattice_net_amd import lattice_blocks as blocks
        from lattice_net_amd.lattice_modules import SliceLatticeModule, SplatLatticeModule
        self.splat, self.slice = SplatLatticeModule(), SliceLatticeModule()
        self.conv = blocks.GnReluConv(CH, CH, 1, False, False, device=dev())
        self.res = blocks.ResnetBlock(CH, CH, [1, 1], [False, False], False, device=dev())
        self.coarsen = blocks.GnReluCoarsen(CH, CH, device=dev())
        self.bottleneck = blocks.BottleneckBlock(CH, CH, [False, False, False], device=dev())
        self.finefy = blocks.GnReluFinefy(CH, CH, device=dev())

    def forward(self, lattice, pos, vals):
        lv, ls, idx, w = self.splat(lattice, pos, vals)
        lv = lv[:ls.nr_lattice_vertices()].contiguous()
        ls.set_values(lv)
        lv, ls = self.conv(lv, ls)
        lv, fine = self.res(lv, ls)
        lvc, lsc = self.coarsen(lv, fine)
        lvc, lsc = self.bottleneck(lvc, lsc)
        lv, ls = self.finefy(lvc, lsc, fine)
        return self.slice(lv, ls, pos, idx, w)


@pytest.fixture(scope="module")
def data():
    """Three clouds of unequal extent and feature scale, the network (GroupNorm parameters moved off their initial 1 / 0), the weights
    of the scalar the gradients are taken of, and the reference: every cloud run alone (computed once, never changed)."""
    from lattice_net_amd import lattice as L
    rng = np.random.default_rng(0)
    pos = np.concatenate([(rng.uniform(-1.0, 1.0, (N0, 3)) * (0.5 + 0.6 * c)).astype(np.float32) for c in range(CLOUDS)])
    vals = np.concatenate([(rng.standard_normal((N0, CH)) * (1 + 2 * c) + c).astype(np.float32) for c in range(CLOUDS)])
    g = rng.standard_normal((CLOUDS * N0, CH)).astype(np.float32)
    torch.manual_seed(0)
    new_lattice(None, False)  # (the filter banks are sized from the position dimensions of the lattices in use)
    net = Net()
    with torch.no_grad():
        for name, p in net.named_parameters():
            if ".gn." in name:
                p.add_(0.3 * torch.randn_like(p))
    d = {"net": net, "pos": torch.from_numpy(pos).to(dev()), "vals": torch.from_numpy(vals).to(dev()), "g": torch.from_numpy(g).to(dev())}
    prev_order, prev_det = L.set_row_order("canonical"), L.set_deterministic(True)
    try:
        outs, grads = [], None
        for c in range(CLOUDS):
            sl = slice(c * N0, (c + 1) * N0)
            out, gr = run(d, None, False, sl)
            outs.append(out)
            grads = gr if grads is None else [a + b for a, b in zip(grads, gr)]
        d["ref_out"], d["ref_grads"] = torch.cat(outs), grads
    finally:
        L.set_row_order(prev_order)
        L.set_deterministic(prev_det)
    return d


def new_lattice(batch, per_cloud_norm):
    import lattice_net_amd as L
    lat = L.Lattice(sigmas=[0.3] * 3, capacity=20000, device=dev())
    if batch:
        lat.set_cloud_batch(batch, per_cloud_norm=per_cloud_norm)
    return lat


def run(d, batch, per_cloud_norm, sl=slice(None), lattice=None):
    lat = lattice if lattice is not None else new_lattice(batch, per_cloud_norm)
    out = d["net"](lat, d["pos"][sl].contiguous(), d["vals"][sl].contiguous())
    grads = torch.autograd.grad((out * d["g"][sl]).sum(), list(d["net"].parameters()))
    return out.detach(), [t.detach() for t in grads]


def rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def worst_against_reference(d, out, grads):
    figures = {f"out cloud {c}": rel(out[c * N0:(c + 1) * N0], d["ref_out"][c * N0:(c + 1) * N0]) for c in range(CLOUDS)}
    for (name, _), got, ref in zip(d["net"].named_parameters(), grads, d["ref_grads"]):
        figures[f"grad {name}"] = rel(got, ref)
    return figures


@pytest.fixture
def deterministic_mode():
    from lattice_net_amd import lattice as L
    prev = L.set_deterministic(True)  # (canonical rows: the suite's conftest)
    yield
    L.set_deterministic(prev)


def test_batch_with_per_cloud_norm_is_the_clouds_one_at_a_time(data, deterministic_mode):
    out, grads = run(data, N0, True)
    figures = worst_against_reference(data, out, grads)
    print(f"cloud batch, per-cloud GroupNorm, against single-cloud runs (relative to the largest magnitude): worst {max(figures.values()):.3e}")
    bad = {k: v for k, v in figures.items() if not v <= BOUND}
    assert not bad, bad


def test_batch_without_per_cloud_norm_mixes_the_clouds(data, deterministic_mode):
    """Statistics over all rows: every cloud's output and the gradients leave the bound (what the switch is for; this is what the
    code computed before the switch existed)."""
    out, grads = run(data, N0, False)
    figures = worst_against_reference(data, out, grads)
    print(f"cloud batch, GroupNorm over all rows, against single-cloud runs: {min(figures.values()):.3e} .. {max(figures.values()):.3e}")
    assert all(figures[f"out cloud {c}"] > BOUND for c in range(CLOUDS)), figures
    assert max(v for k, v in figures.items() if k.startswith("grad")) > BOUND, figures


def test_batch_with_per_cloud_norm_as_a_graph(data, deterministic_mode):
    """Under set_static_rows, forward + backward captured on one stream (a private accumulator pair sized for the clouds, reset first, as
    CapturedNetworkStep does) and replayed twice: the replays are equal bit for bit and within the bound of the eager result."""
    import lattice_net_amd as L
    from lattice_net_amd.lattice_blocks import new_gn_workspace, reset_gn_workspaces, use_gn_workspace
    lat = new_lattice(N0, True)
    L.Lattice.start_level_trace()
    eager_out, eager_grads = run(data, N0, True, lattice=lat)
    levels = L.Lattice.stop_level_trace()
    assert sorted(levels) == [1, 2]
    bound = lambda m: (int(m * 1.07) + 255) // 256 * 256
    lat.set_static_rows(bound(levels[1]), coarse_bounds=[bound(levels[2])])
    assert lat.cloud_segments() == CLOUDS
    entry = new_gn_workspace(dev(), segments=lat.cloud_segments())

    def step():
        reset_gn_workspaces()
        return run(data, N0, True, lattice=lat)

    threads = torch.autograd.is_multithreading_enabled()
    torch.autograd.set_multithreading_enabled(False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    try:
        with torch.cuda.stream(side), use_gn_workspace(entry):
            for _ in range(2):  # warm-up: table buffers, pinned counters and workspaces exist before the capture
                out, grads = step()
            side.synchronize()
            figures = worst_against_reference(data, out, grads)
            assert max(figures.values()) <= BOUND, ("static rows, eager", figures)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                out, grads = step()
        torch.cuda.synchronize()
        replays = []
        with torch.cuda.stream(side):
            for _ in range(2):
                graph.replay()
                side.synchronize()
                replays.append([out.clone()] + [t.clone() for t in grads])
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
    finally:
        torch.autograd.set_multithreading_enabled(threads)
        lat.set_static_rows(None)
    for a, b in zip(*replays):
        assert torch.equal(a, b), "two replays differ"
    assert bool(replays[0][0].abs().sum() > 0)
    worst = max([rel(replays[0][0], eager_out)] + [rel(a, b) for a, b in zip(replays[0][1:], eager_grads)])
    print(f"cloud batch as a graph: replays against the eager step, worst {worst:.3e}")
    assert worst <= BOUND, worst
