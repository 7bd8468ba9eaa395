"""SURVEY.md §8f-2 on the GPU: the unmodified LNN definition (distribute -> PointNet -> U-Net over lattice levels ->
DeformSlice head) runs end to end on the HIP backend, is differentiable through every operator, and learns."""
import textwrap

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = textwrap.dedent("""
    model: {
        positions_mode: "xyz"
        values_mode: "none"
        pointnet_layers: [16,32]
        pointnet_start_nr_channels: 32
        nr_downsamples: 2
        nr_blocks_down_stage: [1,1]
        nr_blocks_bottleneck: 1
        nr_blocks_up_stage: [1,1]
        nr_levels_down_with_normal_resnet: 1
        nr_levels_up_with_normal_resnet: 1
        compression_factor: 1.0
        dropout_last_layer: 0.0
    }
    lattice_gpu: {
        hash_table_capacity: 60000
        nr_sigmas: 1
        sigma_0: "0.08 3"
    }
""")


class Cloud:
    pass


def make_case(tmp_path, n=4000, nr_classes=6, seed=0):
    from lattice_net_amd import Lattice, ModelParams
    from lattice_net_amd.models import LNN, prepare_cloud
    from lattice_net_amd.synthetic import box_surface_cloud
    p = tmp_path / "net.cfg"
    p.write_text(CFG)
    torch.manual_seed(seed)
    mp = ModelParams.create(str(p))
    lattice = Lattice.create(str(p), "lattice")
    net = LNN(nr_classes, mp)
    cloud = Cloud()
    cloud.V = box_surface_cloud(n, seed)
    # labels that depend on position, so that there is something to learn
    cloud.L_gt = (np.floor((cloud.V[:, 0] + 0.5) * 2.999).astype(np.int64) + 3 * (cloud.V[:, 2] > 0)).reshape(-1, 1) % nr_classes
    positions, values, target = prepare_cloud(cloud, mp)
    return net, lattice, positions, values, target


def test_lnn_forward_backward_reaches_every_parameter(tmp_path):
    net, lattice, positions, values, target = make_case(tmp_path)
    logsoftmax, logits = net(lattice, positions, values)
    assert logsoftmax.shape == (positions.shape[0], 6) and logits.shape == logsoftmax.shape
    assert torch.isfinite(logsoftmax).all()
    torch.testing.assert_close(logsoftmax.exp().sum(1), torch.ones(positions.shape[0], device=positions.device), rtol=1e-4, atol=1e-4)
    loss = torch.nn.functional.nll_loss(logsoftmax, target)
    loss.backward()
    missing = [n for n, p in net.named_parameters() if p.grad is None]
    assert not missing, f"no gradient for {missing}"
    bad = [n for n, p in net.named_parameters() if not torch.isfinite(p.grad).all()]
    assert not bad, f"non-finite gradient for {bad}"
    dead = [n for n, p in net.named_parameters() if p.grad.abs().sum() == 0 and "bias" not in n and "beta" not in n]
    assert not dead, f"all-zero gradient for {dead}"


def test_lnn_lattice_levels_shrink_and_forward_is_reproducible(tmp_path):
    net, lattice, positions, values, _ = make_case(tmp_path)
    net.eval()
    sizes = []
    hooks = [c.register_forward_hook(lambda m, i, o: sizes.append((i[1].nr_lattice_vertices(), o[1].nr_lattice_vertices(), o[1].lvl())))
             for c in net.coarsens_list]
    with torch.no_grad():
        a, _ = net(lattice, positions, values)
        first = list(sizes)
        b, _ = net(lattice, positions, values)
    for h in hooks:
        h.remove()
    assert first[0][1] < first[0][0] and first[1][1] < first[1][0] and first[0][1] == first[1][0]
    assert [s[2] for s in first] == [2, 3]  # coarse levels are numbered from the finest = 1 (Lattice.cu:679-682)
    assert sizes[2:] == first                # same vertex counts on the second pass: canonical, race-free numbering
    torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)  # scatter sums may reassociate between runs


def test_lnn_overfits_one_cloud(tmp_path):
    net, lattice, positions, values, target = make_case(tmp_path, n=3000, seed=1)
    opt = torch.optim.AdamW(net.parameters(), lr=3e-3, weight_decay=1e-4, amsgrad=True)  # ln_train.py:165
    losses = []
    for _ in range(40):
        logsoftmax, _ = net(lattice, positions, values)
        loss = torch.nn.functional.nll_loss(logsoftmax, target)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert np.isfinite(losses).all()
    assert losses[-1] < 0.6 * losses[0], losses
    acc = float((logsoftmax.argmax(1) == target).float().mean())
    assert acc > 0.5, acc


@pytest.mark.parametrize("m,c,relu", [(5000, 32, False), (46538, 96, True), (777, 128, True), (100, 48, False), (3, 8, True),
                                      (20000, 64, True), (901, 320, False)])
def test_group_norm_kernels_match_torch(m, c, relu):
    """ln_group_norm_forward / _backward on the [M, C] layout against torch.nn.functional.group_norm (fp64 reference)."""
    from lattice_net_amd.lattice_blocks import GroupNormLatticeModule
    torch.manual_seed(m + c)
    dev = torch.device("cuda", 0)
    mod = GroupNormLatticeModule(c)
    with torch.no_grad():
        mod.gn.weight.uniform_(0.5, 2.0)
        mod.gn.bias.uniform_(-1.0, 1.0)
    x = (torch.randn((m, c), device=dev) * 2 + 0.5).requires_grad_(True)
    gy = torch.randn((m, c), device=dev)
    y, _ = mod(x, None, do_set_values=False, fuse_relu=relu)
    y.backward(gy)
    x64 = x.detach().double().cpu().requires_grad_(True)
    w64 = mod.gn.weight.detach().double().cpu().requires_grad_(True)
    b64 = mod.gn.bias.detach().double().cpu().requires_grad_(True)
    ref = torch.nn.functional.group_norm(x64.t().unsqueeze(0), mod.gn.num_groups, w64, b64, mod.gn.eps).squeeze(0).t()
    if relu:
        # the mask of the fused ReLU is the kernel's own (an element on the kink within rounding may fall on either side of it): with
        # it every element of every gradient is compared (tests/test_gpu_dense_layers.py derives the bounds element by element)
        torch.testing.assert_close(y.detach().cpu().double(), torch.relu(ref).detach(), rtol=1e-4, atol=1e-5)
        ref = ref * (y.detach() > 0).cpu().double()
    ref.backward(gy.double().cpu())
    torch.testing.assert_close(y.detach().cpu().double(), ref.detach(), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(x.grad.cpu().double(), x64.grad, rtol=1e-3, atol=1e-4)
    torch.testing.assert_close(mod.gn.weight.grad.cpu().double(), w64.grad, rtol=2e-4, atol=2e-4 * float(w64.grad.abs().max()))
    torch.testing.assert_close(mod.gn.bias.grad.cpu().double(), b64.grad, rtol=2e-4, atol=2e-4 * float(b64.grad.abs().max()))


@pytest.mark.parametrize("rows,cin,cout,with_gx,slope", [(48000, 4, 16, False, 0.2), (48000, 16, 32, True, 0.2), (1000, 5, 8, False, 0.2),
                                                         (333, 32, 64, True, 0.2), (7, 64, 64, True, 0.2), (48000, 9, 1, True, -1.0),
                                                         (501, 7, 3, True, 0.1), (20000, 96, 96, True, -1.0), (5000, 96, 48, True, -1.0)])
def test_linear_leaky_relu_kernels_match_torch(rows, cin, cout, with_gx, slope):
    """ln_linear_act_forward / _backward (the PointNet per-token MLP) against torch linear + leaky_relu in fp64."""
    from lattice_net_amd.lattice_modules import linear_leaky_relu
    torch.manual_seed(rows + cin)
    dev = torch.device("cuda", 0)
    x = torch.randn((rows, cin), device=dev, requires_grad=with_gx)
    w = (torch.randn((cout, cin), device=dev) / cin ** 0.5).requires_grad_(True)
    b = torch.randn((cout,), device=dev, requires_grad=True)
    gy = torch.randn((rows, cout), device=dev)
    y = linear_leaky_relu(x, w, b, slope)
    y.backward(gy)
    x64 = x.detach().double().cpu().requires_grad_(with_gx)
    w64 = w.detach().double().cpu().requires_grad_(True)
    b64 = b.detach().double().cpu().requires_grad_(True)
    ref = torch.nn.functional.linear(x64, w64, b64)
    if slope >= 0:
        ref = torch.nn.functional.leaky_relu(ref, slope)
    ref.backward(gy.double().cpu())
    torch.testing.assert_close(y.detach().cpu().double(), ref.detach(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(w.grad.cpu().double(), w64.grad, rtol=1e-4, atol=1e-4 * float(w64.grad.abs().max()))
    torch.testing.assert_close(b.grad.cpu().double(), b64.grad, rtol=1e-4, atol=1e-4 * float(b64.grad.abs().max()))
    if with_gx:
        torch.testing.assert_close(x.grad.cpu().double(), x64.grad, rtol=1e-4, atol=1e-5)


def test_remaining_reference_blocks_run_forward_and_backward():
    """Blocks of lattice_modules.py that LNN does not use (Conv1x1WN(Act), TwoConv, ResnetBlock2, DensenetBlock, ConvAct,
    GnGeluConv, BnReluConv, Gn*Coarsen / *Finefy variants, ConvLatticeModule, ExpandLatticeModule): shapes and gradients."""
    from lattice_net_amd import Lattice
    from lattice_net_amd import lattice_blocks as B
    from lattice_net_amd.lattice_modules import ConvLatticeModule, ExpandLatticeModule
    from lattice_net_amd.synthetic import cube_cloud
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    pos = torch.from_numpy(cube_cloud(3000, 3)).to(dev)
    lat = Lattice(sigmas=[0.2] * 3, capacity=40000, device=dev)
    lat.begin_splat()
    lat.just_create_verts(pos, False)
    lat.set_positions(pos)
    m = lat.nr_lattice_vertices()
    c = 16
    for block in [B.Conv1x1WN(c, c, True), B.Conv1x1WNAct(c, c, False), B.TwoConv(c, c, [1, 1], [False, True], False),
                  B.ResnetBlock2(c, c, [1, 2], [True, True], False), B.ConvAct(c, c, 1, True, False), B.GnGeluConv(c, c, 1, False, False),
                  B.BnReluConv(c, c, 1, False), B.GnGelu1x1(c, c, True), B.Gn(c), ConvLatticeModule(c, 1)]:
        lv = torch.randn((m, c), device=dev, requires_grad=True)
        out, ls = block(lv, lat)
        assert out.shape == (m, c) and torch.isfinite(out).all(), type(block).__name__
        out.sum().backward()
        assert lv.grad is not None and torch.isfinite(lv.grad).all(), type(block).__name__
    dn = B.DensenetBlock(8, [1, 1, 1], 3, in_channels=c)
    lv = torch.randn((m, c), device=dev, requires_grad=True)
    out, _ = dn(lv, lat)
    assert out.shape == (m, 24)
    out.sum().backward()
    # level-changing variants
    for cls_c, cls_f in [(B.GnCoarsen, B.GnFinefy), (B.GnGeluCoarsen, B.GnGeluFinefy), (B.GnReluCoarsen, B.FinefyAct)]:
        lv = torch.randn((m, c), device=dev, requires_grad=True)
        cv, cs = cls_c(c, 2 * c)(lv, lat)
        assert cs.lvl() == lat.lvl() + 1 and cv.shape == (cs.nr_lattice_vertices(), 2 * c)
        fv, fs = cls_f(2 * c, c)(cv, cs, lat)
        assert fv.shape == (m, c)
        fv.sum().backward()
        assert torch.isfinite(lv.grad).all() and lv.grad.abs().sum() > 0
    ex = ExpandLatticeModule(2, 0.05, True)
    lv = torch.randn((m, c), device=dev)
    ev, es = ex(lv, lat, pos)
    assert es.nr_lattice_vertices() >= m and ev.shape == (es.nr_lattice_vertices(), c)


SHAPENET_CFG = textwrap.dedent("""
    model: {
        positions_mode: "xyz"
        values_mode: "none"
        pointnet_channels_per_layer: [16,32,64]
        pointnet_start_nr_channels: 32
        nr_downsamples: 3
        nr_blocks_down_stage: [4,4,4]
        nr_blocks_bottleneck: 3
        nr_blocks_up_stage: [2,2,2]
        nr_levels_down_with_normal_resnet: 3
        nr_levels_up_with_normal_resnet: 2
        compression_factor: 1.0
        dropout_last_layer: 0.0
        experiment: "none"
    }
    lattice_gpu: {
        hash_table_capacity: 60000
        nr_sigmas: 1
        sigma_0: "0.05 3"
    }
""")


def test_lnn_with_the_shapenet_model_shape(tmp_path):
    """BASELINE.json configs[1] (ln_train_shapenet_example.cfg:19-31,45-50): 3 downsamples, 4 blocks per level, bottleneck
    blocks in the decoder, channel widths up to 256, a 2.5k-point surface cloud.  Forward + backward through all of it."""
    from lattice_net_amd import Lattice, ModelParams
    from lattice_net_amd.models import LNN
    from lattice_net_amd.synthetic import box_surface_cloud
    p = tmp_path / "shapenet.cfg"
    p.write_text(SHAPENET_CFG)
    torch.manual_seed(0)
    mp = ModelParams.create(str(p))
    lattice = Lattice.create(str(p), "lattice")
    net = LNN(50, mp)  # ShapeNet part segmentation: 50 part labels
    dev = torch.device("cuda", 0)
    pos = torch.from_numpy(box_surface_cloud(2500, 0)).to(dev)
    vals = torch.zeros((2500, 1), device=dev)
    target = torch.randint(0, 50, (2500,), device=dev)
    assert net.slice_fast_cuda.in_channels == 128
    assert [c.coarse.weight.shape[1] for c in net.coarsens_list] == [64, 128, 256]
    logsoftmax, logits = net(lattice, pos, vals)
    assert logsoftmax.shape == (2500, 50) and torch.isfinite(logsoftmax).all()
    torch.nn.functional.nll_loss(logsoftmax, target).backward()
    bad = [n for n, q in net.named_parameters() if q.grad is None or not torch.isfinite(q.grad).all()]
    assert not bad, bad


SCANNET_CFG = textwrap.dedent("""
    model: {
        positions_mode: "xyz"
        values_mode: "rgb+height"
        pointnet_layers: [16,32,64]
        pointnet_start_nr_channels: 32
        nr_downsamples: 3
        nr_blocks_down_stage: [6,6,8]
        nr_blocks_bottleneck: 8
        nr_blocks_up_stage: [2,2,2]
        nr_levels_down_with_normal_resnet: 3
        nr_levels_up_with_normal_resnet: 3
        compression_factor: 1.0
        dropout_last_layer: 0.0
        experiment: "none"
    }
    lattice_gpu: {
        hash_table_capacity: 5000000
        nr_sigmas: 1
        sigma_0: "0.08 3" //default
    }
""")


def test_lnn_with_the_scannet_model_shape(tmp_path):
    """BASELINE.json configs[3] (lnn_train_scannet.cfg:22-48): rgb+height values (7 PointNet input channels), 5M-slot tables,
    3 downsamples with 6/6/8 blocks and 8 bottleneck blocks, 21 classes; a 60k-point scene of planes."""
    from lattice_net_amd import Lattice, ModelParams
    from lattice_net_amd.models import LNN, prepare_cloud
    from lattice_net_amd.synthetic import planes_cloud
    p = tmp_path / "scannet.cfg"
    p.write_text(SCANNET_CFG)
    torch.manual_seed(0)
    mp = ModelParams.create(str(p))
    lattice = Lattice.create(str(p), "lattice")
    net = LNN(21, mp)
    cloud = Cloud()
    cloud.V = planes_cloud(60000, 0)
    rng = np.random.default_rng(0)
    cloud.C = rng.random((60000, 3)).astype(np.float32)
    cloud.L_gt = rng.integers(0, 21, (60000, 1))
    positions, values, target = prepare_cloud(cloud, mp)
    assert values.shape == (60000, 4) and net.point_net.layers[0].weight_v.shape == (16, 7)
    logsoftmax, _ = net(lattice, positions, values)
    assert logsoftmax.shape == (60000, 21) and torch.isfinite(logsoftmax).all()
    torch.nn.functional.nll_loss(logsoftmax, target).backward()
    bad = [n for n, q in net.named_parameters() if q.grad is None or not torch.isfinite(q.grad).all()]
    assert not bad, bad


def test_alternating_clouds_through_one_lattice_leave_no_stale_state(tmp_path):
    """One Lattice object and one network see a stream of clouds of different sizes (ln_train.py:143-154 reuses the lattice
    for every batch).  Neighbour lists, CSR layouts, workspaces and the pinned vertex-count readback are cached per build:
    cloud A must give the same logits and gradients before and after clouds B and C went through."""
    from lattice_net_amd.synthetic import box_surface_cloud, planes_cloud
    net, lattice, pos_a, val_a, target_a = make_case(tmp_path, n=4000)
    dev = pos_a.device
    others = [torch.from_numpy(box_surface_cloud(9000, 5)).to(dev), torch.from_numpy(planes_cloud(1500, 6) * 0.1).to(dev),
              torch.from_numpy(box_surface_cloud(300, 7)).to(dev)]

    def run(pos, val, target=None):
        net.zero_grad()
        ls, _ = net(lattice, pos, val)
        if target is not None:
            torch.nn.functional.nll_loss(ls, target).backward()
        else:
            ls.sum().backward()
        return ls.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters()}

    ls0, g0 = run(pos_a, val_a, target_a)
    for pos in others:
        ls, _ = run(pos, torch.zeros((pos.shape[0], 1), device=dev))
        assert ls.shape[0] == pos.shape[0] and torch.isfinite(ls).all()
        ls1, g1 = run(pos_a, val_a, target_a)
        torch.testing.assert_close(ls1, ls0, rtol=1e-4, atol=1e-5)
        # Gradients: run-to-run rounding noise upstream (atomic sum order) moves a handful of activations across a ReLU kink, and
        # one flipped element shows up at the 1e-2 level in the tensors it feeds, so the comparison is in norm.  Stale state
        # (a neighbour list or CSR layout of the other cloud) gives O(1) errors.
        for k in g0:
            err = float((g1[k] - g0[k]).norm() / (g0[k].norm() + 1e-30))
            assert err < 5e-2, f"{k}: relative L2 difference {err:.3e}"


@pytest.mark.parametrize("n,k,c", [(120000, 4, 9), (1000, 4, 9), (777, 3, 5), (50, 7, 16), (1, 4, 9), (3000, 8, 64), (2049, 2, 1)])
def test_max_centre_kernels_match_torch(n, k, c):
    """ln_max_centre_forward / _backward (the max-centring of the DeformSlice head, mods:525-529) against the torch broadcasting
    expression in fp64."""
    from lattice_net_amd.lattice_blocks import MaxCentreFunction
    torch.manual_seed(n + k + c)
    dev = torch.device("cuda", 0)
    x = torch.randn((n, k, c), device=dev, requires_grad=True)
    gamma = (torch.rand((c,), device=dev) + 0.5).requires_grad_(True)
    beta = torch.randn((c,), device=dev, requires_grad=True)
    g = torch.randn((n, k, c), device=dev)
    out = MaxCentreFunction.apply(x, gamma, beta)
    out.backward(g)
    x64, ga64, be64 = (t.detach().double().requires_grad_(True) for t in (x, gamma, beta))
    ref = x64 - (ga64 * x64.max(1, keepdim=True)[0] + be64)
    ref.backward(g.double())
    torch.testing.assert_close(out.detach().double(), ref.detach(), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(x.grad.double(), x64.grad, rtol=1e-5, atol=1e-5)
    scale = max(float(ga64.grad.abs().max()), float(be64.grad.abs().max()), 1.0)
    torch.testing.assert_close(gamma.grad.double(), ga64.grad, rtol=1e-4, atol=1e-5 * scale)
    torch.testing.assert_close(beta.grad.double(), be64.grad, rtol=1e-4, atol=1e-5 * scale)
    # fixed summation order: bit-identical on a second run
    x.grad = gamma.grad = beta.grad = None
    MaxCentreFunction.apply(x, gamma, beta).backward(g)
    g1 = gamma.grad.clone()
    x.grad = gamma.grad = beta.grad = None
    MaxCentreFunction.apply(x, gamma, beta).backward(g)
    assert torch.equal(g1, gamma.grad)


@pytest.mark.parametrize("rows,cin,cout", [(46538, 96, 96), (46538, 96, 48), (11407, 128, 32), (11407, 32, 128), (500, 16, 64), (64, 64, 16),
                                           (3001, 48, 192)])
def test_per_vertex_linear_layers_on_the_convolution_kernels(rows, cin, cout):
    """Bias-free 1x1 layers run as a lattice convolution with a filter extent of 1 over the identity neighbour list
    (LinearMfmaFunction); forward and both gradients against torch in fp64, 1e-5 relative like the convolution itself."""
    from lattice_net_amd.lattice_modules import LinearMfmaFunction, linear_leaky_relu
    torch.manual_seed(rows + cin + cout)
    dev = torch.device("cuda", 0)
    x = torch.randn((rows, cin), device=dev, requires_grad=True)
    w = (torch.randn((cout, cin), device=dev) / cin ** 0.5).requires_grad_(True)
    g = torch.randn((rows, cout), device=dev)
    y = linear_leaky_relu(x, w, None, -1.0)
    assert y.grad_fn is not None and type(y.grad_fn).__name__.startswith("LinearMfmaFunction")
    y.backward(g)
    x64, w64 = x.detach().double().requires_grad_(True), w.detach().double().requires_grad_(True)
    ref = x64 @ w64.t()
    ref.backward(g.double())
    for got, want in ((y.detach(), ref.detach()), (x.grad, x64.grad), (w.grad, w64.grad)):
        torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=1e-5 * float(want.abs().max()))


def test_training_steps_leave_no_cycles_holding_device_memory(tmp_path):
    """With Python's cycle collector off (how the step is timed, and a common setting in training loops) a step must give all
    of its device memory back through reference counts alone: a lattice storage cached inside itself, or a replay closure
    kept after the build was accepted, would leak ~20 MB per step here."""
    import gc
    net, lattice, positions, values, target = make_case(tmp_path, n=4000)
    opt = None
    def train():
        nonlocal opt
        ls, _ = net(lattice, positions, values)
        loss = torch.nn.functional.nll_loss(ls, target)
        if opt is None:
            opt = torch.optim.AdamW(net.parameters(), lr=1e-3)
        opt.zero_grad()
        loss.backward()
        opt.step()
    for _ in range(3):
        train()
    gc.collect()
    gc.disable()
    try:
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        for _ in range(5):
            train()
        torch.cuda.synchronize()
        grown = torch.cuda.memory_allocated() - before
    finally:
        gc.enable()
    assert grown < (1 << 20), f"{grown / 2**20:.1f} MiB of device memory held by reference cycles after 5 steps"
