"""models.LNN on a batch of clouds in one lattice (Lattice.set_cloud_batch(n0, per_cloud_norm=True, per_cloud_invalid_vertex=True))
against the same clouds run one at a time with the same parameters (`pytest -m gpu`).

distribute -> PointNet -> ResnetBlock -> CoarsenAct -> BottleneckBlock -> GnReluFinefy -> ResnetBlock -> slice-classify, two lattice
levels, 3 clouds x 300 points of unequal extent; the first 8 points of every cloud share a simplex, so that the first vertex of every
cloud passes PointNet's four-point rule and only the "invalid vertex" rule can drop it.  The scalar the gradients are taken of is a
weighted sum of the log-probabilities, additive over the clouds: the reference gradients are the sums of the single-cloud ones.
Per-point log-probabilities of every cloud and every parameter gradient agree within 1e-4 of the largest magnitude of the tensor (the
project's whole-network bound, README Parity) with both switches on; with per_cloud_invalid_vertex off, clouds 1 and 2 must not."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CLOUDS, N0, CLASSES = 3, 300, 20
BOUND = 1e-4

CFG = """
model: { positions_mode: "xyz"  values_mode: "none"  pointnet_layers: [16,32]  pointnet_start_nr_channels: 32  nr_downsamples: 1
    nr_blocks_down_stage: [1]  nr_blocks_bottleneck: 1  nr_blocks_up_stage: [1]  nr_levels_down_with_normal_resnet: 3
    nr_levels_up_with_normal_resnet: 3  compression_factor: 1.0  dropout_last_layer: 0.0 }
lattice_gpu: { hash_table_capacity: 20000  nr_sigmas: 1  sigma_0: "0.9 3" }
"""


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """The clouds, the network (GroupNorm parameters moved off their initial 1 / 0), the weights of the scalar, and the reference: every
    cloud run alone, gradients summed (computed once, never changed)."""
    from lattice_net_amd import Lattice, ModelParams
    from lattice_net_amd import lattice as L
    from lattice_net_amd.models import LNN
    path = tmp_path_factory.mktemp("lnn_cloud_batch") / "lnn.cfg"
    path.write_text(CFG)
    rng = np.random.default_rng(0)
    clouds = []
    for c in range(CLOUDS):
        p = rng.uniform(-1.0, 1.0, (N0, 3)) * (2.0 + 0.7 * c)
        p[1:8] = p[0] + 1e-3 * 0.9 * rng.standard_normal((7, 3))
        clouds.append(p.astype(np.float32))
    pos = np.concatenate(clouds)
    g = rng.standard_normal((CLOUDS * N0, CLASSES)).astype(np.float32)
    torch.manual_seed(0)
    Lattice.create(str(path), "lattice")  # (the filter banks are sized from the position dimensions of the lattices in use)
    net = LNN(CLASSES, ModelParams.create(str(path)), device=dev())
    d = {"cfg": str(path), "net": net, "pos": torch.from_numpy(pos).to(dev()), "vals": torch.zeros((CLOUDS * N0, 1), device=dev()),
         "g": torch.from_numpy(g).to(dev())}
    prev_order, prev_det = L.set_row_order("canonical"), L.set_deterministic(True)
    try:
        run(d, None, sl=slice(0, N0))  # (layers that size themselves from their first input exist from here on)
        with torch.no_grad():
            for name, p in net.named_parameters():
                if ".gn." in name or name.endswith("norm.weight") or name.endswith("norm.bias"):
                    p.add_(0.3 * torch.randn_like(p))
        d["params"] = [p for p in net.parameters()]
        outs, grads = [], None
        for c in range(CLOUDS):
            out, gr = run(d, None, sl=slice(c * N0, (c + 1) * N0))
            outs.append(out)
            grads = gr if grads is None else [a if b is None else a + b for a, b in zip(grads, gr)]
        d["ref_out"], d["ref_grads"] = torch.cat(outs), grads
    finally:
        L.set_row_order(prev_order)
        L.set_deterministic(prev_det)
    assert sum(x is not None for x in grads) > 20
    return d


def new_lattice(d, switches):
    from lattice_net_amd import Lattice
    lat = Lattice.create(d["cfg"], "lattice")
    if switches is not None:
        lat.set_cloud_batch(N0, per_cloud_norm=switches[0], per_cloud_invalid_vertex=switches[1])
    return lat


def run(d, switches, sl=slice(None), lattice=None):
    lat = lattice if lattice is not None else new_lattice(d, switches)
    logsoftmax, _ = d["net"](lat, d["pos"][sl].contiguous(), d["vals"][sl].contiguous())
    params = d.get("params") or list(d["net"].parameters())
    grads = torch.autograd.grad((logsoftmax * d["g"][sl]).sum(), params, allow_unused=True)
    return logsoftmax.detach(), [None if t is None else t.detach() for t in grads]


def rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def worst_against_reference(d, out, grads):
    figures = {f"out cloud {c}": rel(out[c * N0:(c + 1) * N0], d["ref_out"][c * N0:(c + 1) * N0]) for c in range(CLOUDS)}
    for (name, _), got, ref in zip(d["net"].named_parameters(), grads, d["ref_grads"]):
        assert (got is None) == (ref is None), name
        if ref is not None:
            figures[f"grad {name}"] = rel(got, ref)
    return figures


@pytest.fixture
def deterministic_mode():
    from lattice_net_amd import lattice as L
    prev = L.set_deterministic(True)  # (canonical rows: the suite's conftest)
    yield
    L.set_deterministic(prev)


def test_lnn_on_a_batch_is_the_clouds_one_at_a_time(data, deterministic_mode):
    lat = new_lattice(data, (True, True))
    out, grads = run(data, None, lattice=lat)
    figures = worst_against_reference(data, out, grads)
    print(f"LNN on a cloud batch, both per-cloud switches, against single-cloud runs (relative to the largest magnitude): worst "
          f"{max(figures.values()):.3e} ({max(figures, key=figures.get)})")
    bad = {k: v for k, v in figures.items() if not v <= BOUND}
    assert not bad, bad


def test_lnn_on_a_batch_with_row_zero_as_the_only_invalid_vertex(data, deterministic_mode):
    """per_cloud_norm alone (what the code computed before the second switch existed): cloud 0, whose first vertex is row 0, is still
    what it is alone; clouds 1 and 2 keep the PointNet feature of their first vertex and leave the bound."""
    out, grads = run(data, (True, False))
    figures = worst_against_reference(data, out, grads)
    print("LNN on a cloud batch, per-cloud GroupNorm only, outputs against single-cloud runs: " +
          ", ".join(f"{figures[f'out cloud {c}']:.3e}" for c in range(CLOUDS)))
    assert figures["out cloud 0"] <= BOUND, figures
    assert figures["out cloud 1"] > BOUND and figures["out cloud 2"] > BOUND, figures


def test_lnn_on_a_batch_as_a_graph(data, deterministic_mode):
    """The same step through CapturedNetworkStep, replayed twice on its capture stream: the replays are equal bit for bit, non-zero,
    within the bound of the eager batch step, and every level stayed inside its row bound."""
    from lattice_net_amd import CapturedNetworkStep, _lib
    eager_out, eager_grads = run(data, (True, True))
    lat = new_lattice(data, (True, True))
    params = data["params"]

    def step():
        logsoftmax, _ = data["net"](lat, data["pos"], data["vals"])
        (logsoftmax * data["g"]).sum().backward()
        return logsoftmax.detach()

    threads = torch.autograd.is_multithreading_enabled()
    torch.autograd.set_multithreading_enabled(False)
    try:
        cap = CapturedNetworkStep(step, lat, params)
        # (distribute builds into a new lattice object: the accumulators are sized from the lattices the calibration step built)
        assert cap._gn_entry["bufs"][0].numel() * 8 >= _lib.load().ln_group_norm_segments_workspace_bytes(1024, CLOUDS)
        assert sorted(cap.bounds) == [1, 2]
        replays = []
        with torch.cuda.stream(cap.stream):
            for _ in range(2):
                out = cap.launch()
                cap.stream.synchronize()
                counts = cap.check()
                assert sorted(counts) == [1, 2] and all(0 < counts[k] <= cap.bounds[k] for k in counts), (counts, cap.bounds)
                replays.append([out.clone()] + [None if g is None else g.clone() for g in cap.grads])
        torch.cuda.synchronize()
    finally:
        torch.autograd.set_multithreading_enabled(threads)
        lat.set_static_rows(None)
        for p in params:
            p.grad = None
    for a, b in zip(*replays):
        assert (a is None and b is None) or torch.equal(a, b), "two replays differ"
    assert bool(replays[0][0].abs().sum() > 0)
    pairs = [(replays[0][0], eager_out)] + [(a, b) for a, b in zip(replays[0][1:], eager_grads) if b is not None]
    assert all(a is not None for a, _ in pairs)
    worst = max(rel(a, b) for a, b in pairs)
    print(f"LNN on a cloud batch as a graph: replays against the eager step, worst {worst:.3e}")
    assert worst <= BOUND, worst
