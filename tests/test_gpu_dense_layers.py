"""The dense network-layer kernels against fp64, element by element (`pytest -m gpu`): GroupNorm + ReLU (csrc/ln_norm.hip), the
per-token linear + LeakyReLU (csrc/ln_mlp.hip) and the max-centring of the DeformSlice head (csrc/ln_centre.hip).

References, bounds and their counting arguments live in tests/dense_reference.py (checked on the CPU by test_dense_reference.py).
Every operator runs twice:
- random: each finite element within its derived bound of the fp64 result, NaN / +-Inf exactly where fp64 has them; the mask of a
  fused activation is the kernel's own (y > 0), so no element of a gradient is left out of the comparison;
- exact: small integers, parameters that are small integers or powers of two: every partial sum is exact in fp32 and the result is
  the integer result bit for bit in any summation order — one row dropped or read twice shows whatever its magnitude.
Each test prints its worst error / bound ratio (`pytest -s`); nothing is asserted on that figure."""

import numpy as np
import pytest
import torch

from tests import dense_reference as R

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def gpu(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev()).requires_grad_(grad)


# ------------------------------------------------------------------------------------------------------------------ GroupNorm
def gn_module(c, groups, eps, affine, params):
    gn = torch.nn.GroupNorm(groups, c, eps=eps, affine=affine).to(dev())
    if affine:
        with torch.no_grad():
            gn.weight.copy_(gpu(params[0]))
            gn.bias.copy_(gpu(params[1]))
    return gn


def gn_forward(x_np, gn, relu, rows=None):
    """group_norm_rows on the kernels, with the tensors the forward saves for the backward (mean_rstd, scale_shift)."""
    from lattice_net_amd.lattice_blocks import group_norm_rows
    x = gpu(x_np, grad=True)
    rows_dev = None if rows is None else torch.tensor([rows], dtype=torch.int32, device=dev())
    y = group_norm_rows(x, gn, relu, rows_dev)
    assert type(y.grad_fn).__name__.startswith("GroupNormReluFunction")
    _, _, mean_rstd, scale_shift = y.grad_fn.saved_tensors
    return x, y, mean_rstd, scale_shift


gn_params = R.gn_params


def gn_check_random(x_np, gy_np, groups, relu, affine=True, eps=1e-5, rows=None, what="", seed=0):
    """Statistics, scale / shift, apply, and the backward with the kernel's own mask, each against fp64.  Returns the worst ratios."""
    m, c = x_np.shape
    gamma, beta = gn_params(c, affine, seed)
    gn = gn_module(c, groups, eps, affine, (gamma, beta))
    x, y, mean_rstd, scale_shift = gn_forward(x_np, gn, relu, rows)
    y.backward(gpu(gy_np))
    ratios = {"rstd": R.assert_gn_statistics(mean_rstd, x_np, groups, eps, rows, what)}
    R.assert_gn_scale_shift(scale_shift, mean_rstd, gamma, beta, c, groups, what)
    ratios["y"] = R.assert_gn_apply(y, x_np, scale_shift, relu, rows, what)
    mask = (y.detach() > 0).cpu().numpy() if relu else None
    ref, bound = R.gn_backward_reference(x_np, gy_np, mask, gamma, mean_rstd, groups, rows)
    got = (x.grad, gn.weight.grad if affine else None, gn.bias.grad if affine else None)
    for name, g_, r_, b_ in zip(("grad_x", "grad_gamma", "grad_beta"), got, ref, bound):
        if g_ is None:
            continue
        R.assert_within(g_, r_, b_, f"{what} {name}")
        ratios[name] = R.worst_ratio(g_, r_, b_)
    return ratios


def gn_check_exact(m, c, groups, relu, rows=None, what=""):
    """Integer run (dense_reference.gn_exact_input): mean an integer and rstd = 1/2 bit for bit, y and the two parameter gradients the
    integer results.  grad_x = g' gamma rstd + x c2 + c3 divides by the element count of the group: where that count is a power of
    two (up to 2^15: every term then sits on one binary grid of fewer than 24 bits) grad_x is the fp64 result bit for bit, elsewhere
    it is held to its bound.  Returns (y, mean_rstd)."""
    live = m if rows is None else max(0, min(rows, m))
    cg = c // groups
    assert live * cg % 2 == 0 and live > 0, "the exact run needs an even number of elements per group"
    x_np, gy_np = R.gn_exact_input(m, c, groups), R.gn_exact_grad(m, c)
    if live < m:
        x_np[live:], gy_np[live:] = 3e30, -2e30
    gamma, beta = R.gn_exact_params(c)
    gn = gn_module(c, groups, 0.0, True, (gamma, beta))
    x, y, mean_rstd, scale_shift = gn_forward(x_np, gn, relu, rows)
    y.backward(gpu(gy_np))
    mean = (np.arange(groups) % 5 - 2).astype(np.float64)
    R.assert_exact(mean_rstd[:groups], mean, f"{what} mean")
    R.assert_exact(mean_rstd[groups:] * 2, np.ones(groups), f"{what} 2 rstd")
    a = R.f64(gamma) / 2
    b = R.f64(beta) - np.repeat(mean, cg) * a
    R.assert_exact(scale_shift, np.concatenate([a, b]), f"{what} scale_shift")
    y_ref = np.zeros((m, c))
    y_ref[:live] = R.f64(x_np[:live]) * a + b
    if relu:
        y_ref = np.maximum(y_ref, 0)
    R.assert_exact(y, y_ref, f"{what} y")
    mask = (y_ref > 0) if relu else None
    g = R.f64(gy_np[:live]) * (mask[:live] if relu else 1.0)
    R.assert_exact(gn.weight.grad, (g * (R.f64(x_np[:live]) - np.repeat(mean, cg))).sum(0) / 2, f"{what} grad_gamma")
    R.assert_exact(gn.bias.grad, g.sum(0), f"{what} grad_beta")
    ref, bound = R.gn_backward_reference(x_np, gy_np, mask, gamma, mean_rstd, groups, rows)
    R.assert_within(x.grad, ref[0], bound[0], f"{what} grad_x")
    cnt = live * cg
    if cnt & (cnt - 1) == 0 and cnt <= 2 ** 15:
        assert np.array_equal(ref[0].astype(np.float32).astype(np.float64), ref[0]), f"{what}: grad_x is not exact in fp32"
        R.assert_within(x.grad, ref[0], 0.0, f"{what} grad_x (exact)")
        EXACT_GRAD_X.append(what)
    return y, mean_rstd


EXACT_GRAD_X = []  # the exact runs whose grad_x was compared bit for bit


def gn_slab(c):
    return R.gn_rows_per_pass(c) * R.LN_GN_PASSES


def gn_groups(c):
    """1, C, 32 where it divides, C / 2."""
    return sorted({1, c, c // 2} | ({32} if c % 32 == 0 else set()))


# rows_per_pass: 4 -> 256, 8 -> 128, 32 -> 32, 48 -> 21 (252 threads live), 96 -> 10 (240), 128 -> 8, 320 -> 3 (240), 516 and 1024 -> 1
GN_CHANNELS = (4, 8, 32, 48, 96, 128, 320, 516, 1024)


@pytest.mark.parametrize("c", GN_CHANNELS)
def test_group_norm_random(c):
    """Rows 1, 2, rows_per_pass * 16 - 1 / + 1 (one workgroup's slab of rows), more than 32 slabs (every accumulator replica), over
    groups 1, C, 32, C / 2, with and without ReLU and affine parameters."""
    slab = gn_slab(c)
    worst = {}
    case = 0
    for groups in gn_groups(c):
        for m in (1, 2, slab - 1, slab + 1, 33 * slab + 5):
            case += 1
            relu, affine = case % 2 == 1, case % 5 != 0
            x = R.gn_input(m, c, 0.5, 2.0, 1000 * c + case)
            gy = R.gn_input(m, c, 0.0, 1.0, 2000 * c + case)
            r = gn_check_random(x, gy, groups, relu, affine, what=f"c={c} groups={groups} m={m} relu={relu} affine={affine}", seed=case)
            worst = {k: max(v, worst.get(k, 0.0)) for k, v in r.items()}
    print(f"GroupNorm c={c}: worst error / bound {worst}")


@pytest.mark.parametrize("c", GN_CHANNELS)
def test_group_norm_exact(c):
    """The same rows and groups with integers, where the group holds an even number of elements."""
    slab = gn_slab(c)
    ran = 0
    for groups in gn_groups(c):
        cg = c // groups
        for m in (1, 2, slab - 1, slab + 1, 33 * slab + 5, 33 * slab + 6, slab, 2 * slab):
            if m * cg % 2:
                continue
            for relu in (False, True):
                gn_check_exact(m, c, groups, relu, what=f"c={c} groups={groups} m={m} relu={relu}")
                ran += 1
    assert ran >= 20
    if c & (c - 1) == 0:  # (slab rows x a power-of-two group: grad_x bit for bit)
        assert any(w.startswith(f"c={c} ") for w in EXACT_GRAD_X)


def test_group_norm_grid_stride_apply():
    """More than 2048 apply workgroups of 1024 elements: the grid-stride loops of k_gn_apply / k_gn_backward_apply."""
    m, c = 70000, 128
    assert m * c // 4 > 2048 * 256 * 4
    r = gn_check_random(R.gn_input(m, c, -1.0, 3.0, 1), R.gn_input(m, c, 0.0, 1.0, 2), 32, True, what="grid-stride")
    gn_check_exact(m, c, 32, True, what="grid-stride exact")
    print(f"GroupNorm grid-stride: worst error / bound {r}")


@pytest.mark.parametrize("m,c", [(46538, 96), (5000, 32), (901, 320)])
@pytest.mark.parametrize("mean,std", [(0.25, 1.0), (100.0, 1.0), (1000.0, 1.0), (30.0, 0.01)], ids=["0.25", "100", "1000", "30+0.01N"])
def test_group_norm_conditioning(m, c, mean, std):
    """Inputs mean + std * N(0, 1) with |mean| up to 3000 std: every rstd within 1e-5 relative, every mean within
    1e-6 (|mean| + std) (dense_reference.assert_gn_statistics; torch's fp32 native_group_norm meets the same on the same inputs:
    test_dense_reference.py), and the apply and the backward within their bounds."""
    groups = 32 if c % 32 == 0 else c // 2
    x = R.gn_conditioning_input(m, c, mean, std)
    gy = R.gn_input(m, c, 0.0, 1.0, m + c + 1)
    r = gn_check_random(x, gy, groups, True, what=f"{m}x{c} {mean}+{std}N")
    print(f"GroupNorm conditioning {m}x{c} {mean}+{std}N: worst error / bound {r}")


@pytest.mark.parametrize("shift", [30.0, 100.0, 3000.0])
@pytest.mark.parametrize("row", [0, 2500])
def test_group_norm_outlier_row(row, shift):
    """One row 30, 100, 3000 standard deviations from the rest — row 0 (the "invalid" vertex of a lattice) or a row in the middle,
    with and without a static row bound: the statistics keep the conditioning requirement and every gradient its bound (a row is the
    pivot of one thread's 16 rows, never of the whole tensor)."""
    worst = {}
    for m, c, groups, rows in ((5000, 4, 1, None), (5000, 4, 4, None), (5000, 32, 32, None), (46538, 32, 32, None), (5000, 32, 8, 4000)):
        x, gy = R.gn_outlier_input(m, c, row, shift, 7), R.gn_input(m, c, 0.0, 1.0, 8)
        if rows is not None:
            x[rows:], gy[rows:] = 3e30, -1e30
        r = gn_check_random(x, gy, groups, True, rows=rows, what=f"{m}x{c} groups={groups} rows_dev={rows} row {row} at {shift} sigma", seed=1)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in r.items()}
    print(f"GroupNorm outlier row {row} at {shift} sigma: worst error / bound {worst}")


def test_group_norm_constant_group():
    """A group whose channels hold one constant: variance 0, rstd = eps^-1/2, y = beta where the group is."""
    m, c, groups = 700, 32, 8
    x = R.gn_input(m, c, 0.5, 2.0, 3)
    x[:, 4:8] = 7.25
    gn = gn_module(c, groups, 1e-5, True, gn_params(c, True, 0))
    _, y, mean_rstd, scale_shift = gn_forward(x, gn, False)
    assert float(mean_rstd[1]) == 7.25
    assert float(mean_rstd[groups + 1]) == float(np.float32(1.0 / np.sqrt(np.float64(np.float32(1e-5)))))
    R.assert_gn_statistics(mean_rstd, x, groups, 1e-5, what="constant group")
    R.assert_gn_apply(y, x, scale_shift, False, what="constant group")
    R.assert_within(y[:, 4:8], np.broadcast_to(R.f64(gn.bias)[4:8], (m, 4)), 3 * R.EPS32 * 7.25 * np.abs(R.f64(scale_shift[4:8])), "constant group y")


@pytest.mark.parametrize("calls", [3, 5])
def test_group_norm_odd_number_of_launches(calls):
    """The alternating-workspace protocol hands every call zeroed accumulators: `calls` forwards in a row on one stream (an odd number
    of launches) each stay within the bounds, and in the exact run they are equal bit for bit."""
    m, c, groups = 5000, 96, 48
    x = R.gn_input(m, c, 3.0, 2.0, 5)
    gn = gn_module(c, groups, 1e-5, True, gn_params(c, True, 1))
    outs = [gn_forward(x, gn, True) for _ in range(calls)]
    for k, (_, y, mean_rstd, scale_shift) in enumerate(outs):
        R.assert_gn_statistics(mean_rstd, x, groups, 1e-5, what=f"call {k}")
        R.assert_gn_apply(y, x, scale_shift, True, what=f"call {k}")
    gn_e = gn_module(c, groups, 0.0, True, R.gn_exact_params(c))
    runs = [gn_forward(R.gn_exact_input(m, c, groups), gn_e, True) for _ in range(calls)]
    for k in range(1, calls):
        R.assert_equal_bits(runs[k][1], runs[0][1], f"y of call {k}")
        R.assert_equal_bits(runs[k][2], runs[0][2], f"mean_rstd of call {k}")
    gn_check_exact(m, c, groups, True, what=f"exact after {calls} calls")


def test_group_norm_after_a_rejected_call():
    """A call the library rejects (6 channels: not a multiple of 4) launches nothing and leaves the accumulators as they were: the next
    valid call is right."""
    from lattice_net_amd import _lib
    lib = _lib.load()
    m, c, groups = 3000, 32, 16
    x_np = R.gn_input(m, c, 2.0, 1.5, 11)
    gn = gn_module(c, groups, 1e-5, True, gn_params(c, True, 2))
    gn_forward(x_np, gn, False)  # (the pair of this stream exists and is in its steady state)
    x6 = torch.zeros((m, 6), device=dev())
    y6, mr, ss = torch.empty_like(x6), torch.empty((12,), device=dev()), torch.empty((12,), device=dev())
    ws = torch.zeros((int(lib.ln_group_norm_workspace_bytes(8)) // 8,), dtype=torch.float64, device=dev())
    rc = lib.ln_group_norm_forward_rows(_lib.ptr(x6), None, None, m, 6, 3, 1e-5, 0, _lib.ptr(y6), _lib.ptr(mr), _lib.ptr(ss),
                                        _lib.ptr(ws), ws.numel() * 8, None, 0, None, _lib.stream_ptr(dev()))
    assert rc != 0
    for k in range(2):
        _, y, mean_rstd, scale_shift = gn_forward(x_np, gn, False)
        R.assert_gn_statistics(mean_rstd, x_np, groups, 1e-5, what=f"after the rejected call, {k}")
        R.assert_gn_apply(y, x_np, scale_shift, False, what=f"after the rejected call, {k}")


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
def test_group_norm_static_rows(relu):
    """rows_device holding 0, 1, m - 1, m and a value above m on a tensor whose dead rows hold large finite garbage: statistics and
    parameter gradients of the live rows only, y and grad_x exactly zero in the dead rows, everything finite for 0 rows."""
    m, c, groups = 1100, 64, 32
    for rows in (0, 1, m - 1, m, m + 77):
        live = min(rows, m)
        x = R.gn_input(m, c, 1.0, 2.0, 20 + rows % 7)
        gy = R.gn_input(m, c, 0.0, 1.0, 30 + rows % 7)
        x[live:] = 3e30 * np.where(np.arange(c) % 2, -1, 1)
        gy[live:] = -1e30
        what = f"rows_dev={rows}"
        gamma, beta = gn_params(c, True, rows)
        gn = gn_module(c, groups, 1e-5, True, (gamma, beta))
        xg, y, mean_rstd, scale_shift = gn_forward(x, gn, relu, rows)
        y.backward(gpu(gy))
        for name, t in (("y", y), ("mean_rstd", mean_rstd), ("scale_shift", scale_shift), ("grad_x", xg.grad), ("grad_gamma", gn.weight.grad),
                        ("grad_beta", gn.bias.grad)):
            assert bool(torch.isfinite(t).all()), f"{what}: {name} is not finite"
        assert not bool(xg.grad[live:].any()), f"{what}: grad_x is not zero in the dead rows"
        R.assert_gn_statistics(mean_rstd, x, groups, 1e-5, rows, what)
        R.assert_gn_apply(y, x, scale_shift, relu, rows, what)
        mask = (y.detach() > 0).cpu().numpy() if relu else None
        ref, bound = R.gn_backward_reference(x, gy, mask, gamma, mean_rstd, groups, rows)
        for name, g_, r_, b_ in zip(("grad_x", "grad_gamma", "grad_beta"), (xg.grad, gn.weight.grad, gn.bias.grad), ref, bound):
            R.assert_within(g_, r_, b_, f"{what} {name}")
        if live > 0 and live % 2 == 0:
            gn_check_exact(m, c, groups, relu, rows, what=f"{what} exact")


# ------------------------------------------------------------------------------------------------------------------ linear + LeakyReLU
MLP_CASES = R.MLP_CASES


def mlp_run(x_np, w_np, b_np, gy_np, slope, with_gx):
    from lattice_net_amd.lattice_modules import linear_leaky_relu
    x, w = gpu(x_np, grad=with_gx), gpu(w_np, grad=True)
    b = None if b_np is None else gpu(b_np, grad=True)
    y = linear_leaky_relu(x, w, b, slope)
    assert type(y.grad_fn).__name__.startswith("LinearLeakyReluFunction"), type(y.grad_fn).__name__
    y.backward(gpu(gy_np))
    return y.detach(), x.grad, w.grad, None if b is None else b.grad


@pytest.mark.parametrize("case", list(MLP_CASES), ids=list(MLP_CASES))
def test_linear_leaky_relu_random(case):
    rows, cin, cout, slope, bias, with_gx = MLP_CASES[case]
    assert "forward_grid_stride" not in case or rows * (cout // 4) > 4096 * 256
    rng = np.random.default_rng(rows + 131 * cin + cout)
    x = rng.standard_normal((rows, cin)).astype(np.float32)
    w = (rng.standard_normal((cout, cin)) / np.sqrt(cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32) if bias else None
    gy = rng.standard_normal((rows, cout)).astype(np.float32)
    y, gx, gw, gb = mlp_run(x, w, b, gy, slope, with_gx)
    ref, bound, mask = R.mlp_forward_reference(x, w, b, slope, y)
    R.assert_within(y, ref, bound, f"{case} y")
    worst = {"y": R.worst_ratio(y, ref, bound)}
    refs, bounds = R.mlp_backward_reference(x, w, gy, mask, slope)
    for name, g_, r_, b_ in zip(("grad_x", "grad_w", "grad_b"), (gx, gw, gb), refs, bounds):
        if g_ is None:
            assert (name == "grad_x" and not with_gx) or (name == "grad_b" and not bias)
            continue
        R.assert_within(g_, r_, b_, f"{case} {name}")
        worst[name] = R.worst_ratio(g_, r_, b_)
    print(f"linear {case}: worst error / bound {worst}")


@pytest.mark.parametrize("case", list(MLP_CASES), ids=list(MLP_CASES))
def test_linear_leaky_relu_exact(case):
    """Integers (slope 0.2 becomes 0.5 with even operands): y, grad_x, grad_w and grad_b are the integer results."""
    rows, cin, cout, slope, bias, with_gx = MLP_CASES[case]
    slope = 0.5 if slope > 0 else slope
    x, w, b, gy = R.mlp_exact_case(rows, cin, cout, slope)
    if not bias:
        b = None
    y, gx, gw, gb = mlp_run(x, w, b, gy, slope, with_gx)
    pre = R.f64(x) @ R.f64(w).T + (0 if b is None else R.f64(b))
    mask = None if slope < 0 else pre > 0
    R.assert_exact(y, pre if slope < 0 else np.where(mask, pre, pre * slope), f"{case} y")
    refs, _ = R.mlp_backward_reference(x, w, gy, mask, slope)
    for name, g_, r_ in zip(("grad_x", "grad_w", "grad_b"), (gx, gw, gb), refs):
        if g_ is not None:
            R.assert_exact(g_, r_, f"{case} {name}")


def test_linear_dispatch():
    """Which implementation a shape takes: 128 -> 128 with a bias has 16384 (o, i) pairs, more than the streaming backward holds: torch;
    96 -> 96 with a bias: the streaming kernels; 96 -> 96 without bias or activation: the MFMA convolution from 64 rows on."""
    from lattice_net_amd.lattice_modules import linear_leaky_relu

    def fn(rows, cin, cout, bias, slope):
        x = torch.randn((rows, cin), device=dev(), requires_grad=True)
        w = torch.randn((cout, cin), device=dev(), requires_grad=True)
        b = torch.randn((cout,), device=dev(), requires_grad=True) if bias else None
        return type(linear_leaky_relu(x, w, b, slope).grad_fn).__name__

    assert fn(500, 128, 128, True, 0.2) == "LeakyReluBackward0"
    assert fn(500, 128, 128, True, -1.0) == "AddmmBackward0"
    assert fn(500, 96, 96, True, -1.0).startswith("LinearLeakyReluFunction")
    assert fn(64, 96, 96, False, -1.0).startswith("LinearMfmaFunction")
    assert fn(63, 96, 96, False, -1.0).startswith("LinearLeakyReluFunction")
    assert fn(64, 96, 96, False, 0.2).startswith("LinearLeakyReluFunction")


def test_linear_backward_of_no_rows_zeroes_the_parameter_gradients():
    from lattice_net_amd import _lib
    lib = _lib.load()
    cin, cout = 16, 32
    gw = torch.full((cout, cin), 7.0, device=dev())
    gb = torch.full((cout,), 7.0, device=dev())
    ws = torch.empty((int(lib.ln_linear_act_backward_workspace_bytes(cin, cout)),), dtype=torch.uint8, device=dev())
    _lib.check(lib.ln_linear_act_backward(None, None, None, None, 0, cin, cout, 0.2, None, _lib.ptr(gw), _lib.ptr(gb), _lib.ptr(ws),
                                          ws.numel(), _lib.stream_ptr(dev())), "ln_linear_act_backward")
    assert not bool(gw.any()) and not bool(gb.any())


# ------------------------------------------------------------------------------------------------------------------ max-centre
MC_CHANNELS = (1, 5, 9, 16, 33, 64)  # live point lanes 256 // C: 252 threads at C = 9, 231 at 33
MC_KINDS = ("randn", "relu", "neginf", "nan", "exact")


def mc_run(x_np, gamma_np, beta_np, g_np):
    from lattice_net_amd.lattice_blocks import MaxCentreFunction, max_centre_rows
    x, gamma, beta = gpu(x_np, grad=True), gpu(gamma_np, grad=True), gpu(beta_np, grad=True)
    out = max_centre_rows(x, gamma, beta)
    assert type(out.grad_fn).__name__.startswith(MaxCentreFunction.__name__)
    out.backward(gpu(g_np))
    return out.detach(), x.grad, gamma.grad, beta.grad


def mc_check(n, K, c, kind, seed, worst):
    what = f"n={n} K={K} C={c} {kind}"
    rng = np.random.default_rng(seed)
    x = R.mc_input(n, K, c, kind, seed)
    if kind == "exact":
        gamma, beta = np.array([1.0, 2.0, -1.0, 0.5], np.float32)[np.arange(c) % 4], (np.arange(c) % 5 - 2).astype(np.float32)
        g = (2 * rng.integers(-3, 4, (n, K, c))).astype(np.float32)
    else:
        gamma, beta = (rng.random(c) + 0.5).astype(np.float32), rng.standard_normal(c).astype(np.float32)
        g = rng.standard_normal((n, K, c)).astype(np.float32)
    out, gx, ggamma, gbeta = mc_run(x, gamma, beta, g)
    ref, bound, mx, am = R.mc_reference(x, gamma, beta)
    (r_gx, r_gg, r_gb), (b_gx, b_gg, b_gb) = R.mc_backward_reference(g, mx, am, gamma)
    if kind == "exact":
        for name, got, want in (("out", out, ref), ("grad_x", gx, r_gx), ("grad_gamma", ggamma, r_gg), ("grad_beta", gbeta, r_gb)):
            R.assert_exact(R.f64(got) * 2, want * 2, f"{what} 2 {name}")  # (gamma = 1/2 in every fourth channel: halves)
    else:
        R.assert_within(out, ref, bound, f"{what} out")
        R.assert_within(gx, r_gx, b_gx, f"{what} grad_x")
        R.assert_within(gbeta, r_gb, b_gb, f"{what} grad_beta")
        # grad_gamma = -sum_n s max: NaN / +Inf / -Inf exactly where fp64 has them.  Under a +-Inf maximum the sign of s = sum_k g
        # decides which; only a channel where such an s lies within its own rounding of zero is left out (none on these inputs)
        s, sa = R.f64(g).sum(1), np.abs(R.f64(g)).sum(1)
        sure = ~(np.isinf(mx) & (np.abs(s) <= K * R.EPS32 * sa)).any(0)
        assert sure.all() or kind == "neginf", what
        got_gg = R.f64(ggamma)
        R.assert_within(got_gg[sure], r_gg[sure], b_gg[sure], f"{what} grad_gamma")
        fin = np.isfinite(r_gg)
        for name, got, want, b_ in (("out", out, ref, bound), ("grad_x", gx, r_gx, b_gx), ("grad_beta", gbeta, r_gb, b_gb),
                                    ("grad_gamma", got_gg[fin], r_gg[fin], b_gg[fin])):
            worst[name] = max(worst.get(name, 0.0), R.worst_ratio(got, want, b_))
    # fixed summation order: bit-identical on a second run
    again = mc_run(x, gamma, beta, g)
    for name, a, b in zip(("out", "grad_x", "grad_gamma", "grad_beta"), (out, gx, ggamma, gbeta), again):
        R.assert_equal_bits(a, b, f"{what} {name} on a second run")


@pytest.mark.parametrize("kind", MC_KINDS)
@pytest.mark.parametrize("c", MC_CHANNELS)
def test_max_centre(c, kind):
    """K = 1 .. 8, n around a whole number of workgroups (lanes * LN_MC_ITERS points each) - 1 / + 0 / + 1."""
    lanes = 256 // c
    worst = {}
    for K in range(1, 9):
        whole = lanes * R.LN_MC_ITERS * (K % 3 + 1)
        for n in (whole - 1, whole, whole + 1):
            mc_check(n, K, c, kind, 100 * c + K, worst)
    print(f"max-centre C={c} {kind}: worst error / bound {worst}")


@pytest.mark.parametrize("kind", ["randn", "relu", "exact"])
def test_max_centre_many_workgroups(kind):
    """The DeformSlice head's shape, 4 vertices x 9 channels, over 120000 points: more than 1000 slabs through the slab sum."""
    worst = {}
    mc_check(100000 if kind == "exact" else 120000, 4, 9, kind, 9, worst)
    print(f"max-centre 4x9 {kind}, many workgroups: worst error / bound {worst}")


def test_max_centre_no_points():
    out, gx, ggamma, gbeta = mc_run(np.zeros((0, 4, 9), np.float32), np.ones(9, np.float32), np.zeros(9, np.float32), np.zeros((0, 4, 9), np.float32))
    assert out.shape == (0, 4, 9) and gx.shape == (0, 4, 9)
    assert not bool(ggamma.any()) and not bool(gbeta.any())


def test_max_centre_first_maximum_and_nan_by_hand():
    """Ties and NaN by hand: the first of equal maxima takes the gradient; a NaN is the maximum, the first NaN takes the gradient."""
    nan, inf = float("nan"), float("inf")
    x = np.array([[[1.0], [3.0], [3.0], [2.0]], [[0.0], [0.0], [0.0], [0.0]], [[5.0], [nan], [7.0], [nan]], [[-inf], [-inf], [-inf], [-inf]],
                  [[nan], [inf], [1.0], [2.0]]], np.float32)
    g = np.ones_like(x)
    out, gx, _, _ = mc_run(x, np.array([1.0], np.float32), np.array([0.0], np.float32), g)
    for p, k in enumerate([1, 0, 1, 0, 0]):
        want = np.ones(4)
        want[k] = 1.0 - 4.0
        assert np.array_equal(R.f64(gx[p, :, 0]), want), (p, gx[p, :, 0])
    assert np.array_equal(R.f64(out[0, :, 0]), [-2.0, 0.0, 0.0, -1.0])
    assert bool(torch.isnan(out[2]).all()) and bool(torch.isnan(out[3]).all()) and bool(torch.isnan(out[4]).all())
