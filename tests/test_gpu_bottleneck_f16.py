"""BottleneckBlock, GnRelu1x1 and Conv1x1 on fp16 lattice values with fp32 parameters (`pytest -m gpu`), in the setting of
test_gpu_gn_blocks_f16.py::test_per_cloud_form_is_every_cloud_alone: 3 x 200 points at d = 3, set_cloud_batch(200, per_cloud_norm=True),
deterministic mode, 64 channels (the middle width of the bottleneck is 16).  Before the fp16 linear layer (csrc/ln_linear_f16.hip)
these raised torch's dtype error in GnRelu1x1.  The kernels' precision is what test_gpu_linear_f16.py holds; the fp16 / fp32 comparison
here is a sanity condition against a wrong route."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CH = 64
N0, CLOUDS = 200, 3


def dev():
    return torch.device("cuda", 0)


def _positions():
    rng = np.random.default_rng(1)
    return np.concatenate([(rng.uniform(-1.0, 1.0, (N0, 3)) * (0.5 + 0.6 * c)).astype(np.float32) for c in range(CLOUDS)])


def _lattice(points):
    import lattice_net_amd as L
    lat = L.Lattice(sigmas=[0.3] * 3, capacity=20000, device=dev())
    lat.set_cloud_batch(N0, per_cloud_norm=True)  # (a cloud alone is a batch of one: the same kernels over one range)
    lat.begin_splat()
    lat.just_create_verts(torch.from_numpy(points).to(dev()), False)
    m = lat.nr_lattice_vertices()
    return lat, m, lat.cloud_row_starts().cpu().numpy()


def _run(net, lat, vals, g):
    """(output, value gradient, parameter gradients) of sum(out * g)"""
    lv = vals.clone().requires_grad_(True)
    lat.set_values(lv)
    out, _ = net(lv, lat)
    grads = torch.autograd.grad((out.float() * g.float()).sum(), [lv] + list(net.parameters()))
    return out.detach(), grads[0], list(grads[1:])


@pytest.fixture(scope="module")
def setting():
    from lattice_net_amd import lattice as LM
    from lattice_net_amd import lattice_blocks as blocks
    prev = LM.set_deterministic(True)
    order = LM.set_row_order("canonical")  # (what the suite's conftest sets around every test: this fixture is built once, ahead of it)
    try:
        pos = _positions()
        lat, m, starts = _lattice(pos)
        torch.manual_seed(1)
        net = blocks.BottleneckBlock(CH, CH, [False, False, True], device=dev())  # (behind the first lattice: filter banks are sized from the lattices in use)
        vals = torch.from_numpy((np.random.default_rng(2).standard_normal((m, CH)) * 2).astype(np.float16)).to(dev())
        g = torch.from_numpy(np.random.default_rng(3).standard_normal((m, CH)).astype(np.float16)).to(dev())
        yield {"pos": pos, "lat": lat, "m": m, "starts": starts, "net": net, "vals": vals, "g": g}
    finally:
        LM.set_row_order(order)
        LM.set_deterministic(prev)


def test_bottleneck_f16_is_every_cloud_alone(setting):
    """fp16 output and value gradient, fp32 parameter gradients; every cloud's output rows and value-gradient rows bitwise those of the
    cloud run alone; parameter gradients within 1e-4 of the largest magnitude of the sum over the single-cloud runs (the project's bound
    for that comparison: the batch sums the same terms in another order)."""
    s = setting
    net, lat, vals, g, starts = s["net"], s["lat"], s["vals"], s["g"], s["starts"]
    out, gv, gp = _run(net, lat, vals, g)
    assert out.dtype == torch.float16 and gv.dtype == torch.float16 and all(t.dtype == torch.float32 for t in gp)
    assert len(gp) == len(list(net.parameters())) and bool(torch.isfinite(out).all()) and float(out.float().abs().max()) > 0
    assert starts[-1] == s["m"]
    summed = [torch.zeros_like(t, dtype=torch.float64) for t in gp]
    for c in range(CLOUDS):
        lo, hi = int(starts[c]), int(starts[c + 1])
        one, m1, _ = _lattice(s["pos"][c * N0:(c + 1) * N0])
        assert m1 == hi - lo
        alone, gv1, gp1 = _run(net, one, vals[lo:hi].contiguous(), g[lo:hi].contiguous())
        assert torch.equal(out[lo:hi], alone), f"cloud {c}: the batch rows differ from the cloud run alone"
        assert torch.equal(gv[lo:hi], gv1), f"cloud {c}: the value gradient differs from the cloud run alone"
        for acc, t in zip(summed, gp1):
            acc += t.double()
    for (name, _), got, want in zip(net.named_parameters(), gp, summed):
        scale = float(want.abs().max())
        err = float((got.double() - want).abs().max())
        print(f"BOTTLENECK_F16 {name}: |batch - sum of clouds| {err:.3e}, largest magnitude {scale:.3e}")
        assert err <= 1e-4 * scale, (name, err, scale)


def test_bottleneck_f16_against_the_fp32_block(setting):
    """The same block on .float() values: relative L2 difference of the outputs printed, asserted below 2^-6 only - a
    dropped residual or a transposed weight gives O(1)."""
    s = setting
    out16, _, _ = _run(s["net"], s["lat"], s["vals"], s["g"])
    out32, gv32, gp32 = _run(s["net"], s["lat"], s["vals"].float(), s["g"])
    assert out32.dtype == torch.float32 and gv32.dtype == torch.float32
    rel = float((out16.float() - out32).norm() / out32.norm())
    print(f"BOTTLENECK_F16 fp16 against fp32 block: relative L2 difference of the outputs {rel:.3e}")
    assert rel < 2.0 ** -6, rel


def test_bottleneck_fp32_is_the_hand_composed_block(setting):
    """fp32 values take the route they took: bitwise `lv + identity` composed by hand from the block's own sub-modules."""
    s = setting
    net, lat = s["net"], s["lat"]
    vals = s["vals"].float()
    with torch.no_grad():
        lat.set_values(vals)
        got, _ = net(vals, lat)
        lat.set_values(vals)
        lv, ls = net.contract(vals, lat)
        lv, ls = net.conv(lv, ls)
        lv, ls = net.expand(lv, ls)
        want = lv + vals
    assert got.dtype == torch.float32 and torch.equal(got, want)


def test_gn_relu_1x1_and_conv_1x1_take_fp16_rows(setting):
    """GnRelu1x1 and Conv1x1 (with bias) on fp16 rows: fp16 out, fp16 gradient w.r.t. the input, fp32 gradients w.r.t. the parameters;
    the route is the fp16 GEMM."""
    from lattice_net_amd import lattice_blocks as blocks
    s = setting
    lat, vals, g = s["lat"], s["vals"], s["g"]
    torch.manual_seed(2)
    gn1x1 = blocks.GnRelu1x1(CH, 32, True, device=dev())
    out, gv, gp = _run(gn1x1, lat, vals, g[:, :32].contiguous())
    assert out.dtype == torch.float16 and out.shape == (s["m"], 32) and gv.dtype == torch.float16 and gv.shape == vals.shape
    assert len(gp) == 4 and all(t.dtype == torch.float32 and bool(torch.isfinite(t).all()) for t in gp)
    conv = blocks.Conv1x1(48, True, in_channels=CH, device=dev())
    x = vals.clone().requires_grad_(True)
    y = conv(x)
    assert y.dtype == torch.float16 and type(y.grad_fn).__name__.startswith("LinearF16Function")
    grads = torch.autograd.grad((y.float() * g[:, :48].float()).sum(), [x, conv.linear.weight, conv.linear.bias])
    assert grads[0].dtype == torch.float16 and grads[1].dtype == torch.float32 and grads[2].dtype == torch.float32
    # against torch on the fp16-rounded weights in fp64: the tolerance of one fp16 rounding on values of this size
    want = x.detach().double() @ conv.linear.weight.detach().half().double().t() + conv.linear.bias.detach().double()
    assert float((y.detach().double() - want).abs().max()) <= 2.0 ** -10 * float(want.abs().max())
    # fp32 rows still go through torch.nn.Linear
    y32 = conv(vals.float())
    assert y32.dtype == torch.float32 and torch.equal(y32, torch.nn.functional.linear(vals.float(), conv.linear.weight, conv.linear.bias))
