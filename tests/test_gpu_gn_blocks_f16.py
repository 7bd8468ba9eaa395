"""GroupNorm on fp16 lattice values with fp32 parameters through group_norm_rows and a Gn block (`pytest -m gpu`): fp16 rows are taken per
row range (up to 64 ranges, 65 are a ValueError), every other fp16 call is what it was; GnReluConv on a batch of clouds with per-cloud
statistics, forward and backward, against every cloud alone.  fp16 rows under set_static_rows are not taken: DESIGN.md 4.6."""
import numpy as np
import pytest
import torch

from tests import dense_reference as R
from tests.test_gpu_group_norm_f16 import check_rows, half_input

pytestmark = pytest.mark.gpu

CH = 32


def dev():
    return torch.device("cuda", 0)


def gn_module(c, groups, seed):
    gn = torch.nn.GroupNorm(groups, c).to(dev())
    gamma, beta = R.gn_params(c, True, seed)
    with torch.no_grad():
        gn.weight.copy_(torch.from_numpy(gamma))
        gn.bias.copy_(torch.from_numpy(beta))
    return gn


def test_ranges_take_fp16_rows_and_static_rows_still_refuse():
    """Per row range fp16 rows take the kernels (this raised ValueError before the fp16 kernels existed); 65 ranges on fp16 rows are a
    ValueError that says so; with a device row count fp16 rows are refused as before."""
    from lattice_net_amd.lattice_blocks import group_norm_rows
    gn = gn_module(CH, 32, 1)
    x = torch.from_numpy(half_input(400, CH, 0.5, 2.0, 1)).to(dev()).requires_grad_(True)
    starts = torch.tensor([0, 1, 1, 150, 400], dtype=torch.int32, device=dev())
    y = group_norm_rows(x, gn, True, None, starts, many_ranges=True)
    assert y.dtype == torch.float16 and type(y.grad_fn).__name__.startswith("GroupNormSegmentsFunction")
    y.sum().backward()
    assert x.grad.dtype == torch.float16 and gn.weight.grad.dtype == torch.float32 and gn.bias.grad.dtype == torch.float32
    with pytest.raises(ValueError, match="float16 rows takes at most 64 ranges"):
        group_norm_rows(x, gn, True, None, torch.arange(0, 66, dtype=torch.int32, device=dev()), many_ranges=True)
    with pytest.raises(ValueError, match="static-rows mode needs the HIP GroupNorm"):
        group_norm_rows(x, gn, True, torch.tensor([350], dtype=torch.int32, device=dev()))


def test_plain_fp16_calls_are_torch_as_before():
    """Without row ranges fp16 rows never reach the kernels: torch.nn.GroupNorm on the transposed view (+ relu), bit for bit."""
    from lattice_net_amd.lattice_blocks import group_norm_rows
    gn = gn_module(CH, 32, 2).half()
    x = torch.from_numpy(half_input(400, CH, 0.5, 2.0, 2)).to(dev())
    for relu in (False, True):
        got = group_norm_rows(x, gn, relu)
        want = gn(x.t().unsqueeze(0)).squeeze(0).t()
        want = torch.relu(want) if relu else want
        assert got.dtype == torch.float16 and torch.equal(got, want)


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
def test_ranges_through_group_norm_rows_are_within_the_kernel_bounds(relu):
    """group_norm_rows with row ranges on fp16 rows and fp32 parameters, forward + backward: every range within the bounds of
    tests/test_gpu_group_norm_f16.py, the parameter gradients within the summed bounds of the ranges."""
    from lattice_net_amd.lattice_blocks import group_norm_rows
    from tests import cloud_batch_reference as B
    m, c, groups = 700, 64, 32
    starts = [0, 1, 1, 150, 700]
    x_np, gy_np = half_input(m, c, 0.5, 2.0, 3), half_input(m, c, 0.0, 1.0, 4)
    gn = gn_module(c, groups, 5)
    gamma, beta = R.gn_params(c, True, 5)
    x = torch.from_numpy(x_np).to(dev()).requires_grad_(True)
    y = group_norm_rows(x, gn, relu, None, torch.tensor(starts, dtype=torch.int32, device=dev()))
    assert type(y.grad_fn).__name__.startswith("GroupNormSegmentsFunction")
    _, _, mean_rstd, scale_shift = y.grad_fn.saved_tensors
    y.backward(torch.from_numpy(gy_np).to(dev()))
    got = {"y": y, "grad_x": x.grad, "mean_rstd": mean_rstd, "scale_shift": scale_shift, "grad_gamma": gn.weight.grad, "grad_beta": gn.bias.grad}
    got = {k: v.detach().cpu().numpy() for k, v in got.items()}
    assert got["y"].dtype == np.float16 and got["grad_x"].dtype == np.float16 and got["grad_gamma"].dtype == np.float32
    worst = {}
    dg, b_dg, db, b_db = np.zeros(c), np.zeros(c), np.zeros(c), np.zeros(c)
    for s_, (lo, hi) in enumerate(B.segments(starts, m)[0]):
        if hi == lo:
            continue
        part = {"y": got["y"][lo:hi], "grad_x": got["grad_x"][lo:hi], "mean_rstd": got["mean_rstd"][s_], "scale_shift": got["scale_shift"][s_]}
        for k, v in check_rows(part, x_np[lo:hi], gy_np[lo:hi], gamma, beta, groups, gn.eps, relu, None, f"range {s_}").items():
            worst[k] = max(v, worst.get(k, 0.0))
        mask = (R.gn_apply_fp32(x_np[lo:hi].astype(np.float32), got["scale_shift"][s_], True) > 0) if relu else None
        refs, bounds = R.gn_backward_reference(x_np[lo:hi], gy_np[lo:hi], mask, gamma, got["mean_rstd"][s_], groups)
        dg, b_dg, db, b_db = dg + refs[1], b_dg + bounds[1], db + refs[2], b_db + bounds[2]
    R.assert_within(got["grad_gamma"], dg, b_dg, "grad_gamma")
    R.assert_within(got["grad_beta"], db, b_db, "grad_beta")
    print(f"group_norm_rows fp16 per range, relu={relu}: worst error / bound {worst}")


def test_per_cloud_form_is_every_cloud_alone():
    """set_cloud_batch(200, per_cloud_norm=True) on 3 x 200 points, GnReluConv on fp16 values with fp32 parameters, forward and backward,
    against every cloud run alone as a batch of one (deterministic mode; canonical rows: the suite's conftest): the output rows and the
    rows of the value gradient of every cloud are bitwise those of the cloud alone; fp16 out and value gradient, fp32 parameter
    gradients."""
    import lattice_net_amd as L
    from lattice_net_amd import lattice as LM
    from lattice_net_amd import lattice_blocks as blocks
    n0, clouds = 200, 3
    rng = np.random.default_rng(1)
    pos = np.concatenate([(rng.uniform(-1.0, 1.0, (n0, 3)) * (0.5 + 0.6 * c)).astype(np.float32) for c in range(clouds)])
    prev = LM.set_deterministic(True)
    try:
        def run(points, batch):
            lat = L.Lattice(sigmas=[0.3] * 3, capacity=20000, device=dev())
            lat.set_cloud_batch(n0, per_cloud_norm=True)  # (a cloud alone is a batch of one: the same kernels over one range)
            lat.begin_splat()
            lat.just_create_verts(torch.from_numpy(points).to(dev()), False)
            m = lat.nr_lattice_vertices()
            return lat, m, lat.cloud_row_starts().cpu().numpy()

        def block(net, lat, vals, g):
            lv = vals.clone().requires_grad_(True)
            lat.set_values(lv)
            out, _ = net(lv, lat)
            grads = torch.autograd.grad((out.float() * g.float()).sum(), [lv] + list(net.parameters()))
            assert out.dtype == torch.float16 and grads[0].dtype == torch.float16 and all(t.dtype == torch.float32 for t in grads[1:])
            return out.detach(), grads[0]

        lat, m, starts = run(pos, True)
        torch.manual_seed(1)
        net = blocks.GnReluConv(CH, CH, 1, False, False, device=dev())  # (behind the first lattice: filter banks are sized from the lattices in use)
        vals = torch.from_numpy((np.random.default_rng(2).standard_normal((m, CH)) * 2).astype(np.float16)).to(dev())
        g = torch.from_numpy(np.random.default_rng(3).standard_normal((m, CH)).astype(np.float16)).to(dev())
        out, gv = block(net, lat, vals, g)
        assert starts[-1] == m
        for c in range(clouds):
            lo, hi = int(starts[c]), int(starts[c + 1])
            one, m1, _ = run(pos[c * n0:(c + 1) * n0], False)
            assert m1 == hi - lo
            alone, gv1 = block(net, one, vals[lo:hi].contiguous(), g[lo:hi].contiguous())
            assert torch.equal(out[lo:hi], alone), f"cloud {c}: the batch rows differ from the cloud run alone"
            assert torch.equal(gv[lo:hi], gv1), f"cloud {c}: the value gradient differs from the cloud run alone"
    finally:
        LM.set_deterministic(prev)
