"""The DeformSlice head on fp16 lattice values through autograd (`pytest -m gpu`): GatherLattice, SliceClassifyLattice and
SliceFastCUDALatticeModule.  The kernels are held bit for bit to their fp32 forms by test_gpu_slice_classify_f16.py; here the routes:
fp16 `lv` against `lv.float()` on a real d = 3 lattice in deterministic mode (the fp32 accumulation order of the segment reduce is
then fixed), forwards and parameter gradients bitwise equal, the value gradient fp16 and bitwise the fp32 run's rounded once.  Before
the fp16 entry points existed these calls handed fp16 storage to `const float*` kernels."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, V, C = 300, 32, 20
N0, CLOUDS, CH = 300, 3, 64


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def deterministic():
    from lattice_net_amd import lattice as LM
    prev = LM.set_deterministic(True)
    order = LM.set_row_order("canonical")  # (what the suite's conftest sets around every test: module fixtures are built ahead of it)
    try:
        yield
    finally:
        LM.set_row_order(order)
        LM.set_deterministic(prev)


@pytest.fixture(scope="module")
def one_cloud(deterministic):
    import lattice_net_amd as L
    rng = np.random.default_rng(11)
    pos = torch.from_numpy(rng.uniform(-1.0, 1.0, (N, 3)).astype(np.float32)).to(dev())
    lat = L.Lattice(sigmas=[0.3] * 3, capacity=20000, device=dev())
    lat.begin_splat()
    idx, w = lat.just_create_verts(pos, True)
    m = lat.nr_lattice_vertices()
    vals = torch.from_numpy(rng.standard_normal((m, V)).astype(np.float16)).to(dev())
    return {"lat": lat, "pos": pos, "idx": idx, "w": w, "m": m, "vals": vals, "rng": rng}


def _t(rng, *shape, scale=1.0):
    return torch.from_numpy((scale * rng.standard_normal(shape)).astype(np.float32)).to(dev())


def test_gather_lattice_on_fp16_values(one_cloud):
    from lattice_net_amd.lattice_funcs import GatherLattice
    s = one_cloud
    g = _t(np.random.default_rng(12), N, 4 * (V + 1))
    res = {}
    for name, vals in (("f16", s["vals"]), ("f32", s["vals"].float())):
        lv = vals.clone().requires_grad_(True)
        out = GatherLattice.apply(lv, s["lat"], s["pos"], s["idx"], s["w"])
        (gv,) = torch.autograd.grad((out * g).sum(), [lv])
        res[name] = (out.detach(), gv)
    assert res["f16"][0].dtype == torch.float32 and res["f16"][0].shape == (N, 4 * (V + 1))
    assert torch.equal(res["f16"][0].view(torch.int32), res["f32"][0].view(torch.int32)), "gathered rows differ from the fp32 run"
    assert res["f16"][1].dtype == torch.float16 and res["f32"][1].dtype == torch.float32
    assert torch.equal(res["f16"][1].view(torch.int16), res["f32"][1].half().view(torch.int16)), "value gradient is not the fp32 one rounded once"
    assert float(res["f32"][1].abs().max()) > 0


def test_slice_classify_lattice_on_fp16_values(one_cloud):
    from lattice_net_amd.lattice_funcs import SliceClassifyLattice
    s = one_cloud
    rng = np.random.default_rng(13)
    g = _t(rng, N, C)
    dw0, lw0, lb0 = _t(rng, N, 4, scale=0.1), _t(rng, C, V), _t(rng, C)
    res = {}
    for name, vals in (("f16", s["vals"]), ("f32", s["vals"].float())):
        lv = vals.clone().requires_grad_(True)
        dw, lw, lb = (t.clone().requires_grad_(True) for t in (dw0, lw0, lb0))
        logits = SliceClassifyLattice.apply(lv, s["lat"], s["pos"], dw, lw, lb, C, s["idx"], s["w"])
        grads = torch.autograd.grad((logits * g).sum(), [lv, dw, lw, lb])
        res[name] = (logits.detach(), grads)
    l16, g16 = res["f16"]
    l32, g32 = res["f32"]
    assert l16.dtype == torch.float32 and torch.equal(l16.view(torch.int32), l32.view(torch.int32)), "logits differ from the fp32 run"
    for k, name in ((1, "grad_delta_weights"), (2, "grad_linear_clasify_weight"), (3, "grad_linear_clasify_bias")):
        assert g16[k].dtype == torch.float32 and torch.equal(g16[k].view(torch.int32), g32[k].view(torch.int32)), f"{name} differs from the fp32 run"
    assert g16[0].dtype == torch.float16 and g16[0].shape == (s["m"], V) and g32[0].dtype == torch.float32
    assert torch.equal(g16[0].view(torch.int16), g32[0].half().view(torch.int16)), "value gradient is not the fp32 one rounded once"
    assert float(g32[0].abs().max()) > 0 and bool(torch.isfinite(l16).all())


# ------------------------------------------------------------------------------------------------------------------ the module
def _batch_lattice(points):
    import lattice_net_amd as L
    lat = L.Lattice(sigmas=[0.3] * 3, capacity=20000, device=dev())
    lat.set_cloud_batch(N0, per_cloud_norm=True)  # (a cloud alone is a batch of one: the same kernels over one range)
    lat.begin_splat()
    idx, w = lat.just_create_verts(torch.from_numpy(points).to(dev()), True)
    return lat, idx, w, lat.nr_lattice_vertices(), lat.cloud_row_starts().cpu().numpy()


def _run_head(net, lat, vals, pos, idx, w, g):
    lv = vals.clone().requires_grad_(True)
    lat.set_values(lv)
    logits = net(lv, lat, pos, idx, w)
    grads = torch.autograd.grad((logits * g).sum(), [lv] + list(net.parameters()))
    return logits.detach(), grads[0], list(grads[1:])


def test_slice_fast_module_on_fp16_values(deterministic):
    """3 clouds x 300 points with per-cloud GroupNorm in canonical row order (the setting in which GnRelu1x1 keeps fp16 rows): fp32 finite
    logits, fp16 value gradient, fp32 parameter gradients, every cloud's logits bitwise those of the cloud run alone, and the logits
    within 2^-6 of the largest logit magnitude of the fp32 module on the widened input (a sanity bound against a wrong route only: the
    step-downs run fp16 GEMMs and fp16 GroupNorm)."""
    from lattice_net_amd import lattice_blocks as blocks
    rng = np.random.default_rng(21)
    pos_np = np.concatenate([(rng.uniform(-1.0, 1.0, (N0, 3)) * (0.5 + 0.6 * c)).astype(np.float32) for c in range(CLOUDS)])
    lat, idx, w, m, starts = _batch_lattice(pos_np)
    pos = torch.from_numpy(pos_np).to(dev())
    torch.manual_seed(3)
    net = blocks.SliceFastCUDALatticeModule(CH, C, 0.0, "none", device=dev())
    vals = torch.from_numpy((rng.standard_normal((m, CH)) * 2).astype(np.float16)).to(dev())
    g = _t(rng, CLOUDS * N0, C)
    logits, gv, gp = _run_head(net, lat, vals, pos, idx, w, g)
    assert logits.dtype == torch.float32 and logits.shape == (CLOUDS * N0, C) and bool(torch.isfinite(logits).all())
    assert gv.dtype == torch.float16 and gv.shape == vals.shape and bool(torch.isfinite(gv.float()).all())
    assert len(gp) == len(list(net.parameters())) and all(t.dtype == torch.float32 and bool(torch.isfinite(t).all()) for t in gp)
    assert starts[-1] == m
    for c in range(CLOUDS):
        lo, hi = int(starts[c]), int(starts[c + 1])
        one, idx1, w1, m1, _ = _batch_lattice(pos_np[c * N0:(c + 1) * N0])
        assert m1 == hi - lo
        alone, _, _ = _run_head(net, one, vals[lo:hi].contiguous(), pos[c * N0:(c + 1) * N0].contiguous(), idx1, w1, g[c * N0:(c + 1) * N0].contiguous())
        assert torch.equal(logits[c * N0:(c + 1) * N0].view(torch.int32), alone.view(torch.int32)), f"cloud {c}: the batch logits differ from the cloud run alone"
    logits32, gv32, _ = _run_head(net, lat, vals.float(), pos, idx, w, g)
    assert logits32.dtype == torch.float32 and gv32.dtype == torch.float32
    diff, scale = float((logits - logits32).abs().max()), float(logits32.abs().max())
    print(f"HEAD_F16 fp16 against fp32 module: largest logit difference {diff:.3e}, largest logit magnitude {scale:.3e}, ratio {diff / scale:.3e}")
    assert diff < 2.0 ** -6 * scale, (diff, scale)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_in_python(one_cloud):
    import lattice_net_amd as L
    from lattice_net_amd.lattice_funcs import GatherLattice, SliceClassifyLattice
    s = one_cloud
    rng = np.random.default_rng(31)
    lat, pos, idx, w, m = s["lat"], s["pos"], s["idx"], s["w"], s["m"]

    def classify(vals, v):
        return SliceClassifyLattice.apply(vals, lat, pos, _t(rng, N, 4, scale=0.1), _t(rng, C, v), _t(rng, C), C, idx, w)

    six = torch.zeros((m, 6), dtype=torch.float16, device=dev())
    with pytest.raises(ValueError, match="val_dim % 4 == 0"):
        classify(six, 6)
    bf = torch.zeros((m, V), dtype=torch.bfloat16, device=dev())
    lat.set_values(bf)
    with pytest.raises(ValueError, match="float32 or float16"):
        lat.slice_classify_with_precomputation(pos, _t(rng, N, 4), _t(rng, C, V), _t(rng, C), C, idx, w)
    with pytest.raises(ValueError, match="float32 or float16"):
        lat.gather_standalone_with_precomputation(pos, idx, w)
    lat.set_values(s["vals"])
    # static-rows mode: like the rest of the fp16 path, eager only
    static = L.Lattice(sigmas=[0.3] * 3, capacity=20000, device=dev())
    static.begin_splat()
    idx2, w2 = static.just_create_verts(pos, True)
    m2 = static.nr_lattice_vertices()
    static.set_static_rows(m2)
    vals2 = torch.zeros((m2, V), dtype=torch.float16, device=dev())
    with pytest.raises(RuntimeError, match="set_static_rows"):
        SliceClassifyLattice.apply(vals2, static, pos, _t(rng, N, 4, scale=0.1), _t(rng, C, V), _t(rng, C), C, idx2, w2)
    with pytest.raises(RuntimeError, match="set_static_rows"):
        GatherLattice.apply(vals2, static, pos, idx2, w2)
    static.set_static_rows(None)
