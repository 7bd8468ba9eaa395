"""The training loss of a batch of clouds in one lattice against the clouds run one at a time (`pytest -m gpu`): the set-up of
test_gpu_lnn_cloud_batch.py (3 clouds x 300 points, per_cloud_norm and per_cloud_invalid_vertex on), labels of which 0 %, 40 % and 90 %
are the ignored class, and the step's loss  0.5 LovaszSoftmax + 0.5 NLLLoss(ignore_index=unlabeled)  (ln_train.py:128-158), without and
with LNN.compute_class_weights.

The reference runs every cloud alone with the same parameters and takes the loss the reference project takes on one cloud —
LovaszSoftmax(ignore_index) and torch.nn.functional.nll_loss(weight=, ignore_index=) —; its loss and parameter gradients are the means
over the clouds.  On the batch, LovaszSoftmax(points_per_cloud=) + NLLLoss(points_per_cloud=) must give that loss and those gradients
within the bound of test_gpu_lnn_cloud_batch.py (1e-4 of the largest magnitude of the tensor); with the batch-wide nll_loss_gather in
place of NLLLoss(points_per_cloud=) they must not — the cloud without ignored labels weighs 3.5 times its share there."""
import numpy as np
import pytest
import torch

from .test_gpu_lnn_cloud_batch import BOUND, CLASSES, CLOUDS, N0, data, deterministic_mode, dev, new_lattice, rel  # noqa: F401

pytestmark = pytest.mark.gpu

IGNORE = 0
SHARES = (0.0, 0.4, 0.9)


def labels_and_weights(net):
    rng = np.random.default_rng(11)
    y = rng.integers(1, CLASSES, CLOUDS * N0).astype(np.int64)
    for c, share in enumerate(SHARES):
        part = y[c * N0:(c + 1) * N0]
        part[rng.permutation(N0)[:int(round(share * N0))]] = IGNORE
    freq = np.bincount(y, minlength=CLASSES) / y.size
    return torch.from_numpy(y).to(dev()), net.compute_class_weights(freq, IGNORE)


@pytest.fixture(scope="module")
def setup(data):
    """Labels, class weights and, for weights absent and present, the reference: every cloud alone, loss and gradients averaged (computed
    once, never changed)."""
    from lattice_net_amd import lattice as L
    from lattice_net_amd.losses import LovaszSoftmax
    y, weights = labels_and_weights(data["net"])
    assert weights.dtype == torch.float32 and weights.device.type == "cuda" and float(weights[IGNORE]) == float(np.float32(1e-8))
    counted = [(y[c * N0:(c + 1) * N0] != IGNORE).sum().item() for c in range(CLOUDS)]
    assert counted == [N0, N0 - int(round(0.4 * N0)), N0 - int(round(0.9 * N0))]
    refs = {}
    prev_order, prev_det = L.set_row_order("canonical"), L.set_deterministic(True)
    try:
        for key, w in (("plain", None), ("weighted", weights)):
            total, grads = 0.0, None
            for c in range(CLOUDS):
                sl = slice(c * N0, (c + 1) * N0)
                out, _ = data["net"](new_lattice(data, None), data["pos"][sl].contiguous(), data["vals"][sl].contiguous())
                loss = 0.5 * LovaszSoftmax(IGNORE)(out, y[sl]) + 0.5 * torch.nn.functional.nll_loss(out, y[sl], weight=w, ignore_index=IGNORE)
                gr = torch.autograd.grad(loss, data["params"], allow_unused=True)
                total = total + loss.detach()
                grads = list(gr) if grads is None else [a if b is None else a + b for a, b in zip(grads, gr)]
            refs[key] = (total / CLOUDS, [None if g is None else g / CLOUDS for g in grads])
    finally:
        L.set_row_order(prev_order)
        L.set_deterministic(prev_det)
    return {"y": y, "weights": {"plain": None, "weighted": weights}, "refs": refs}


def batch_loss(data, setup, key, out, per_cloud_nll=True):
    from lattice_net_amd.losses import LovaszSoftmax, NLLLoss, nll_loss_gather
    lovasz = LovaszSoftmax(IGNORE, points_per_cloud=N0)(out, setup["y"])
    if per_cloud_nll:
        nll = NLLLoss(weight=setup["weights"][key], ignore_index=IGNORE, points_per_cloud=N0).to(dev())(out, setup["y"])
    else:
        nll = nll_loss_gather(out, setup["y"], IGNORE)  # the mean over all counted labels of the batch
    return 0.5 * lovasz + 0.5 * nll


def figures_against_reference(data, setup, key, loss, grads):
    ref_loss, ref_grads = setup["refs"][key]
    figures = {"loss": rel(loss.reshape(1), ref_loss.reshape(1))}
    for (name, _), got, ref in zip(data["net"].named_parameters(), grads, ref_grads):
        if ref is not None:
            assert got is not None, name
            figures[f"grad {name}"] = rel(got, ref)
    return figures


@pytest.mark.parametrize("fused", (True, False))
@pytest.mark.parametrize("key", ("plain", "weighted"))
def test_batched_training_loss_is_the_mean_of_the_clouds_steps(data, setup, deterministic_mode, monkeypatch, key, fused):
    from lattice_net_amd import losses
    monkeypatch.setattr(losses, "FUSED_NLL_CLOUDS", fused)
    out, _ = data["net"](new_lattice(data, (True, True)), data["pos"], data["vals"])
    loss = batch_loss(data, setup, key, out)
    figures = figures_against_reference(data, setup, key, loss.detach(), torch.autograd.grad(loss, data["params"], allow_unused=True))
    print(f"\nLNN on a cloud batch, 0.5 Lovasz + 0.5 NLL per cloud ({key}, {'kernels' if fused else 'torch form'}) against single-cloud steps: "
          f"worst {max(figures.values()):.3e} ({max(figures, key=figures.get)}), loss {figures['loss']:.3e}")
    bad = {k: v for k, v in figures.items() if not v <= BOUND}
    assert not bad, bad


def test_batch_wide_nll_is_not_the_mean_of_the_clouds_steps(data, setup, deterministic_mode):
    """What the step computed before NLLLoss(points_per_cloud=): every counted label of the batch weighs the same, so the cloud with no
    ignored label has 300 / 510 of the loss instead of a third."""
    out, _ = data["net"](new_lattice(data, (True, True)), data["pos"], data["vals"])
    loss = batch_loss(data, setup, "plain", out, per_cloud_nll=False)
    figures = figures_against_reference(data, setup, "plain", loss.detach(), torch.autograd.grad(loss, data["params"], allow_unused=True))
    over = [k for k, v in figures.items() if v > BOUND]
    print(f"\nLNN on a cloud batch, batch-wide NLL against single-cloud steps: worst {max(figures.values()):.3e}, loss {figures['loss']:.3e}, "
          f"{len(over)} of {len(figures)} figures over the bound")
    assert max(v for k, v in figures.items() if k != "loss") > BOUND, figures  # (the loss moves too, by how far the clouds' losses differ)


def test_batched_training_step_as_a_graph(data, setup, deterministic_mode, monkeypatch):
    """The weighted step through CapturedNetworkStep: two replays equal bit for bit, and within the bound of the reference."""
    from lattice_net_amd import CapturedNetworkStep, losses
    monkeypatch.setattr(losses, "FUSED_NLL_CLOUDS", True)
    lat = new_lattice(data, (True, True))
    params = data["params"]

    def step():
        out, _ = data["net"](lat, data["pos"], data["vals"])
        loss = batch_loss(data, setup, "weighted", out)
        loss.backward()
        return loss.detach()

    threads = torch.autograd.is_multithreading_enabled()
    torch.autograd.set_multithreading_enabled(False)
    try:
        cap = CapturedNetworkStep(step, lat, params)
        replays = []
        with torch.cuda.stream(cap.stream):
            for _ in range(2):
                out = cap.launch()
                cap.stream.synchronize()
                cap.check()
                replays.append([out.clone()] + [None if g is None else g.clone() for g in cap.grads])
        torch.cuda.synchronize()
    finally:
        torch.autograd.set_multithreading_enabled(threads)
        lat.set_static_rows(None)
        for p in params:
            p.grad = None
    for a, b in zip(*replays):
        assert (a is None and b is None) or torch.equal(a, b), "two replays differ"
    assert float(replays[0][0]) > 0
    figures = figures_against_reference(data, setup, "weighted", replays[0][0], replays[0][1:])
    print(f"\nLNN on a cloud batch, the weighted step as a graph against single-cloud steps: worst {max(figures.values()):.3e}")
    assert max(figures.values()) <= BOUND, figures
