"""CPU checks of tests/dense_reference.py, the references and bounds test_gpu_dense_layers.py holds the HIP kernels to.

For each operator: torch's own fp32 CPU implementation of the same operation passes every bound on the random cases (the bounds are
satisfiable and the inputs legitimate), and planted faults are caught on CPU data: one row's contribution removed from a parameter
gradient, one output element off by 16 times its bound, one activation-mask bit flipped."""
import numpy as np
import pytest
import torch

from tests import dense_reference as R
from tests.dense_reference import MLP_CASES, gn_params


def raises(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


# ------------------------------------------------------------------------------------------------------------------ the primitives
def test_assert_within_compares_non_finite_patterns_and_every_element():
    ref = np.array([1.0, np.nan, np.inf, -np.inf, 0.0])
    R.assert_within(ref.copy(), ref, 0.0)
    for i, v in ((1, 0.0), (2, -np.inf), (3, np.nan), (0, np.inf), (4, 1e-30)):
        got = ref.copy()
        got[i] = v
        raises(R.assert_within, got, ref, 0.0)
    R.assert_within(np.array([1.0 + 1e-7]), np.array([1.0]), 2e-7)
    raises(R.assert_within, np.array([1.0 + 3e-7]), np.array([1.0]), 2e-7)
    raises(R.assert_within, np.array([1.0]), np.array([1.0]), np.nan)


def test_assert_exact_wants_integers_below_2_pow_24():
    R.assert_exact(np.array([3.0, -7.0], np.float32), np.array([3.0, -7.0]))
    raises(R.assert_exact, np.array([3.0]), np.array([3.5]))
    raises(R.assert_exact, np.array([2.0 ** 24]), np.array([2.0 ** 24]))
    raises(R.assert_exact, np.array([3.0, -6.0]), np.array([3.0, -7.0]))
    raises(R.assert_equal_bits, np.array([0.0], np.float32), np.array([-0.0], np.float32))


# ------------------------------------------------------------------------------------------------------------------ GroupNorm
def torch_group_norm(x_np, gamma, beta, groups, eps):
    """torch's fp32 CPU GroupNorm on the [1, C, M] layout: (mean_rstd as the kernels publish it, x as a leaf of that layout)."""
    x = torch.from_numpy(x_np).t().contiguous().unsqueeze(0)
    m, c = x_np.shape
    g = None if gamma is None else torch.from_numpy(gamma)
    b = None if beta is None else torch.from_numpy(beta)
    _, mean, rstd = torch.native_group_norm(x, g, b, 1, c, m, groups, eps)
    return torch.cat([mean.reshape(-1), rstd.reshape(-1)]).numpy()


@pytest.mark.parametrize("m,c", [(46538, 96), (5000, 32), (901, 320)])
@pytest.mark.parametrize("mean,std", [(0.25, 1.0), (100.0, 1.0), (1000.0, 1.0), (30.0, 0.01)], ids=["0.25", "100", "1000", "30+0.01N"])
def test_torch_fp32_group_norm_meets_the_conditioning_requirement(m, c, mean, std):
    """The inputs of test_gpu_dense_layers.test_group_norm_conditioning (same seeds): rstd within 1e-5 relative and mean within
    1e-6 (|mean| + std) is what a careful fp32 implementation delivers."""
    groups = 32 if c % 32 == 0 else c // 2
    x = R.gn_conditioning_input(m, c, mean, std)
    R.assert_gn_statistics(torch_group_norm(x, None, None, groups, 1e-5), x, groups, 1e-5, what=f"{m}x{c} {mean}+{std}N")


def test_naive_fp32_moments_miss_the_conditioning_requirement():
    """E[x^2] - mean^2 over fp32 sums, the form the requirement rules out."""
    x = R.gn_input(5000, 32, 1000.0, 1.0, 5032)
    xg = x.reshape(5000, 32, 1)
    s = xg.sum(axis=(0, 2), dtype=np.float32) / np.float32(5000)
    ss = (xg * xg).sum(axis=(0, 2), dtype=np.float32) / np.float32(5000)
    rstd = 1.0 / np.sqrt(np.maximum(ss - s * s, 0) + np.float32(1e-5))
    raises(R.assert_gn_statistics, np.concatenate([s, rstd]), x, 32, 1e-5)


def gn_cpu_case(m, c, groups, relu, affine, mean=0.5, std=2.0, seed=0, rows=None):
    """What the kernels would hand back if they computed like torch's fp32 CPU GroupNorm: its statistics, the scale / shift and y formed
    from them the way k_gn_apply does, and torch's fp32 gradients under the mask of that y."""
    x = R.gn_input(m, c, mean, std, seed)
    gy = R.gn_input(m, c, 0.0, 1.0, seed + 1)
    gamma, beta = gn_params(c, affine, seed)
    live = m if rows is None else rows
    mean_rstd = torch_group_norm(x[:live], gamma, beta, groups, 1e-5)
    cg = c // groups
    mr = mean_rstd.astype(np.float64).reshape(2, groups)
    a = ((np.ones(c, np.float32) if gamma is None else gamma) * np.repeat(mr[1], cg).astype(np.float32)).astype(np.float32)
    b = ((0.0 if beta is None else beta.astype(np.float64)) - np.repeat(mr[0], cg) * a.astype(np.float64)).astype(np.float32)
    scale_shift = np.concatenate([a, b])
    y = R.gn_apply_fp32(x, scale_shift, relu, rows)
    mask = (y > 0) if relu else None
    xt = torch.from_numpy(x[:live]).requires_grad_(True)
    gt = None if gamma is None else torch.from_numpy(gamma).requires_grad_(True)
    bt = None if beta is None else torch.from_numpy(beta).requires_grad_(True)
    out = torch.nn.functional.group_norm(xt.t().unsqueeze(0), groups, gt, bt, 1e-5).squeeze(0).t()
    if relu:
        out = out * torch.from_numpy(mask[:live].astype(np.float32))
    out.backward(torch.from_numpy(gy[:live]))
    gx = np.zeros_like(x)
    gx[:live] = xt.grad.numpy()
    grads = (gx, None if gt is None else gt.grad.numpy(), None if bt is None else bt.grad.numpy())
    return dict(x=x, gy=gy, gamma=gamma, beta=beta, mean_rstd=mean_rstd, scale_shift=scale_shift, y=y, mask=mask, grads=grads, groups=groups,
                relu=relu, rows=rows)


def gn_check(k, backward=True):
    c = k["x"].shape[1]
    R.assert_gn_statistics(k["mean_rstd"], k["x"], k["groups"], 1e-5, k["rows"])
    R.assert_gn_scale_shift(k["scale_shift"], k["mean_rstd"], k["gamma"], k["beta"], c, k["groups"])
    R.assert_gn_apply(k["y"], k["x"], k["scale_shift"], k["relu"], k["rows"])
    ref, bound = R.gn_backward_reference(k["x"], k["gy"], k["mask"], k["gamma"], k["mean_rstd"], k["groups"], k["rows"])
    for name, g_, r_, b_ in zip(("grad_x", "grad_gamma", "grad_beta"), k["grads"], ref, bound):
        if g_ is not None and (backward or name == "grad_beta"):
            R.assert_within(g_, r_, b_, name)
    return ref, bound


@pytest.mark.parametrize("c", [4, 8, 32, 48, 96, 128, 320, 516, 1024])
def test_torch_fp32_group_norm_passes_the_bounds(c):
    """The groups of test_gpu_dense_layers.test_group_norm_random and its rows up to 3 slabs.  torch refuses a group of one element.  Its
    backward forms sum gy (x - mean) as ds - db * mean from unshifted fp32 sums, whose error grows with |x|, not with |x - mean| as the
    bounds here do (they count the roundings of sums of differences of rows): with one or two rows, where x - mean is a small
    difference of the rows themselves, and far from zero (next test) its grad_x and grad_gamma are compared no further than
    grad_beta; test_shifted_fp32_sums_pass_every_bound shows those bounds satisfiable in fp32 on the CPU."""
    slab = R.gn_rows_per_pass(c) * R.LN_GN_PASSES
    case = 0
    for groups in sorted({1, c, c // 2} | ({32} if c % 32 == 0 else set())):
        for m in (1, 2, slab - 1, slab + 1, 3 * slab + 5):
            case += 1
            if m * (c // groups) > 1:
                gn_check(gn_cpu_case(m, c, groups, case % 2 == 1, case % 5 != 0, seed=1000 * c + case), backward=m > 2)


@pytest.mark.parametrize("mean,std", [(100.0, 1.0), (1000.0, 1.0)])
def test_torch_fp32_group_norm_passes_the_bounds_far_from_zero(mean, std):
    """(At 30 + 0.01 N torch's fp32 Welford sits at the requirement itself, 0.5e-5 .. 1.2e-5 from seed to seed: it is held to it on the
    seeded inputs of the requirement only, above.)"""
    gn_check(gn_cpu_case(901, 320, 32, True, True, mean, std, seed=7), backward=False)
    gn_check(gn_cpu_case(1100, 64, 32, True, True, mean, std, seed=8, rows=700), backward=False)


def gn_emulate(x, gy, gamma, beta, groups, eps, relu, rows=None):
    """The arithmetic of csrc/ln_norm.hip in NumPy, fp32 where the kernels are fp32: per thread the chain of LN_GN_PASSES terms of
    x - pivot (the thread's first row), the pivot put back in fp64, fp64 moments; scale / shift, y and the backward as the apply
    kernels form them.  Same dictionary as gn_cpu_case."""
    f4, f8 = np.float32, np.float64
    m, c = x.shape
    live = m if rows is None else max(0, min(rows, m))
    cg = c // groups
    rpp = R.gn_rows_per_pass(c)
    slab = rpp * R.LN_GN_PASSES
    nb = max(1, -(-live // slab))

    def blocks(a):
        pad = np.zeros((nb * slab, c), f4)
        pad[:live] = a[:live]
        return pad.reshape(nb, R.LN_GN_PASSES, rpp, c)

    def chain(t):
        acc = np.zeros(t[:, 0].shape, f4)
        for k in range(R.LN_GN_PASSES):
            acc = (acc + t[:, k]).astype(f4)
        return acc

    def group(v):
        return np.repeat(v.reshape(groups, cg).sum(1), cg)

    valid = (np.arange(nb * slab) < live).reshape(nb, R.LN_GN_PASSES, rpp, 1)
    n = valid.sum(1)
    xb = blocks(x)
    piv = xb[:, 0].astype(f8)
    with np.errstate(all="ignore"):
        d = np.where(valid, xb - xb[:, :1], 0).astype(f4)
        s1, s2 = chain(d).astype(f8), chain((d * d).astype(f4)).astype(f8)
        sx, sxx = (s1 + n * piv).sum((0, 1)), (s2 + 2 * piv * s1 + n * piv * piv).sum((0, 1))
        cnt = max(live, 1) * cg
        mean = sx.reshape(groups, cg).sum(1) / cnt
        var = np.maximum(sxx.reshape(groups, cg).sum(1) / cnt - mean * mean, 0)
        mean_rstd = np.concatenate([mean, 1 / np.sqrt(var + f8(f4(eps)))]).astype(f4)
        mean_c, rstd_c = (np.repeat(v, cg) for v in mean_rstd.astype(f8).reshape(2, groups))
        g32 = np.ones(c, f4) if gamma is None else gamma
        a = (g32 * np.repeat(mean_rstd[groups:], cg)).astype(f4)
        b = ((0.0 if beta is None else beta.astype(f8)) - np.repeat(mean, cg) * a.astype(f8)).astype(f4)
        scale_shift = np.concatenate([a, b])
        y = R.gn_apply_fp32(x, scale_shift, relu, rows)
        mask = (y > 0) if relu else None
        g = (gy * mask).astype(f4) if relu else gy
        gb = blocks(g)
        s, q = chain((gb * d).astype(f4)).astype(f8), chain(gb).astype(f8)
        ds, db = (s + piv * q).sum((0, 1)), q.sum((0, 1))
        sum1, sum2 = group(ds * g32), group(db * g32)
        c2 = (sum2 * mean_c - sum1) * rstd_c ** 3 / cnt
        c3 = -c2 * mean_c - sum2 * rstd_c / cnt
        gx = np.zeros_like(x)
        gr = (g32 * rstd_c.astype(f4)).astype(f4)
        gx[:live] = ((g[:live] * gr).astype(f4) + (x[:live] * c2.astype(f4)).astype(f4)).astype(f4) + c3.astype(f4)
        grads = (gx, None if gamma is None else ((ds - db * mean_c) * rstd_c).astype(f4), None if beta is None else db.astype(f4))
    return dict(x=x, gy=gy, gamma=gamma, beta=beta, mean_rstd=mean_rstd, scale_shift=scale_shift, y=y, mask=mask, grads=grads, groups=groups,
                relu=relu, rows=rows)


@pytest.mark.parametrize("c", [4, 8, 32, 48, 96, 128, 320, 516, 1024])
def test_shifted_fp32_sums_pass_every_bound(c):
    """gn_emulate on the rows (up to 3 slabs) and groups of test_gpu_dense_layers.test_group_norm_random, one and two rows and a group of
    one element included, and far from zero: statistics, apply and all three gradients."""
    slab = R.gn_rows_per_pass(c) * R.LN_GN_PASSES
    case = 0
    for groups in sorted({1, c, c // 2} | ({32} if c % 32 == 0 else set())):
        for m in (1, 2, slab - 1, slab + 1, 3 * slab + 5):
            case += 1
            mean, std = ((0.5, 2.0), (100.0, 1.0), (1000.0, 1.0), (30.0, 0.01))[case % 4]
            gamma, beta = gn_params(c, case % 5 != 0, case)
            x, gy = R.gn_input(m, c, mean, std, 1000 * c + case), R.gn_input(m, c, 0.0, 1.0, 2000 * c + case)
            gn_check(gn_emulate(x, gy, gamma, beta, groups, 1e-5, case % 2 == 1))


@pytest.mark.parametrize("m,c", [(46538, 96), (5000, 32), (901, 320)])
@pytest.mark.parametrize("mean,std", [(0.25, 1.0), (100.0, 1.0), (1000.0, 1.0), (30.0, 0.01)], ids=["0.25", "100", "1000", "30+0.01N"])
def test_shifted_fp32_sums_meet_the_conditioning_requirement(m, c, mean, std):
    groups = 32 if c % 32 == 0 else c // 2
    gamma, beta = gn_params(c, True, 0)
    gn_check(gn_emulate(R.gn_conditioning_input(m, c, mean, std), R.gn_input(m, c, 0.0, 1.0, m + c + 1), gamma, beta, groups, 1e-5, True))


@pytest.mark.parametrize("shift", [30.0, 100.0, 3000.0])
@pytest.mark.parametrize("row", [0, 2500])
def test_an_outlier_row_does_not_spoil_the_statistics(row, shift):
    """One row far from the rest, row 0 (the "invalid" vertex of a lattice) or any other: the requirement holds for the shifted sums
    (the row is the pivot of one thread's 16 rows only) and for torch; with ONE pivot row for the whole tensor it would not."""
    for m, c, groups, rows in ((5000, 4, 1, None), (5000, 4, 4, None), (5000, 32, 32, None), (5000, 32, 8, 4000)):
        x, gy = R.gn_outlier_input(m, c, row, shift, 7), R.gn_input(m, c, 0.0, 1.0, 8)
        gamma, beta = gn_params(c, True, 1)
        gn_check(gn_emulate(x, gy, gamma, beta, groups, 1e-5, True, rows))
        live = m if rows is None else rows
        R.assert_gn_statistics(torch_group_norm(x[:live], None, None, groups, 1e-5), x, groups, 1e-5, rows)
    if row == 0 and shift >= 100.0:
        x = R.gn_outlier_input(5000, 4, 0, shift, 7)
        d = (x - x[0]).astype(np.float32)
        s1, s2 = d.sum(0, dtype=np.float32).astype(np.float64), (d * d).sum(0, dtype=np.float32).astype(np.float64)
        p = x[0].astype(np.float64)
        mean = (s1 + 5000 * p).sum() / 20000
        var = (s2 - 2 * (mean - p) * s1 + 5000 * (mean - p) ** 2).sum() / 20000
        raises(R.assert_gn_statistics, np.array([mean, 1 / np.sqrt(var + 1e-5)]), x, 1, 1e-5)


def test_group_norm_planted_faults_are_caught():
    k = gn_cpu_case(3000, 32, 8, True, True, seed=3)
    ref, bound = gn_check(k)
    x, gy, mask = k["x"].astype(np.float64), k["gy"].astype(np.float64), k["mask"]
    c = 32
    mean, rstd = (np.repeat(v, 4) for v in k["mean_rstd"].astype(np.float64).reshape(2, 8))
    # one row's contribution removed from the parameter gradients
    row = int(np.argmax(np.abs(gy * mask).min(1)))
    for i, contrib in ((1, gy[row] * mask[row] * (x[row] - mean) * rstd), (2, gy[row] * mask[row])):
        raises(R.assert_within, k["grads"][i] - contrib, ref[i], bound[i])
    # one element 16 bounds off
    for i in range(3):
        got = k["grads"][i].astype(np.float64).copy()
        idx = (5, 7) if i == 0 else (7,)
        got[idx] += 16 * bound[i][idx]
        raises(R.assert_within, got, ref[i], bound[i])
    y = k["y"].astype(np.float64).copy()
    y[11, 3] += 16 * 3 * R.EPS32 * (abs(x[11, 3] * k["scale_shift"][3]) + abs(k["scale_shift"][c + 3])) + 1e-30
    raises(R.assert_gn_apply, y, k["x"], k["scale_shift"], True)
    # one mask bit flipped: in y (a positive element written as zero, a zero written as positive) and in the backward
    on, off = np.argwhere(k["y"] > 0)[17], np.argwhere(k["y"] == 0)[17]
    for idx, v in ((on, 0.0), (off, 1e-3)):
        y = k["y"].copy()
        y[tuple(idx)] = v
        raises(R.assert_gn_apply, y, k["x"], k["scale_shift"], True)
    flipped = mask.copy()
    flipped[tuple(on)] = False
    wrong, _ = R.gn_backward_reference(k["x"], k["gy"], flipped, k["gamma"], k["mean_rstd"], 8)
    for i in range(3):
        raises(R.assert_within, wrong[i], ref[i], bound[i])
    # a dead row that is not zero, statistics that count a dead row
    ks = gn_cpu_case(1100, 64, 32, False, True, seed=9, rows=700)
    y = ks["y"].copy()
    y[900, 5] = 1e-20
    raises(R.assert_gn_apply, y, ks["x"], ks["scale_shift"], False, 700)
    raises(R.assert_gn_statistics, ks["mean_rstd"], ks["x"], 32, 1e-5, 701)


def test_group_norm_exact_inputs_have_integer_moments():
    for m, c, groups in ((6, 8, 2), (4095, 4, 1), (50, 48, 24), (2, 1024, 1024)):
        x = R.gn_exact_input(m, c, groups)
        mean, rstd, _ = R.gn_statistics(x, groups, 0.0)
        assert np.array_equal(mean, np.arange(groups) % 5 - 2) and np.array_equal(rstd, np.full(groups, 0.5))
        assert float(np.abs(x - x[0]).max()) <= 4
        gy = R.gn_exact_grad(m, c)
        assert np.array_equal(gy % 2, np.zeros_like(gy)) and len(np.unique(gy)) >= 6
    # one row less: the mean is no integer any more
    for drop in (0, 1, 2000, 4093):
        mean, rstd, _ = R.gn_statistics(np.delete(R.gn_exact_input(4095, 4, 1), drop, axis=0), 1, 0.0)
        assert mean[0] != round(mean[0]) and rstd[0] != 0.5


# ------------------------------------------------------------------------------------------------------------------ linear + LeakyReLU
def mlp_cpu_case(case):
    rows, cin, cout, slope, bias, _ = MLP_CASES[case]
    rng = np.random.default_rng(rows + 131 * cin + cout)
    x = rng.standard_normal((rows, cin)).astype(np.float32)
    w = (rng.standard_normal((cout, cin)) / np.sqrt(cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32) if bias else None
    gy = rng.standard_normal((rows, cout)).astype(np.float32)
    xt, wt = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(w).requires_grad_(True)
    bt = None if b is None else torch.from_numpy(b).requires_grad_(True)
    y = torch.nn.functional.linear(xt, wt, bt)
    if slope >= 0:
        y = torch.nn.functional.leaky_relu(y, slope)
    y.backward(torch.from_numpy(gy))
    return x, w, b, gy, slope, y.detach().numpy(), (xt.grad.numpy(), wt.grad.numpy(), None if bt is None else bt.grad.numpy())


@pytest.mark.parametrize("case", list(MLP_CASES), ids=list(MLP_CASES))
def test_torch_fp32_linear_passes_the_bounds(case):
    x, w, b, gy, slope, y, grads = mlp_cpu_case(case)
    ref, bound, mask = R.mlp_forward_reference(x, w, b, slope, y)
    R.assert_within(y, ref, bound, "y")
    refs, bounds = R.mlp_backward_reference(x, w, gy, mask, slope)
    for name, g_, r_, b_ in zip(("grad_x", "grad_w", "grad_b"), grads, refs, bounds):
        if g_ is not None:
            R.assert_within(g_, r_, b_, name)


def test_linear_planted_faults_are_caught():
    x, w, b, gy, slope, y, grads = mlp_cpu_case("16to32-w_256_to_1024_pairs")
    ref, bound, mask = R.mlp_forward_reference(x, w, b, slope, y)
    refs, bounds = R.mlp_backward_reference(x, w, gy, mask, slope)
    g = gy.astype(np.float64) * np.where(mask, 1.0, slope)
    row = int(np.argmax(np.abs(g).min(1) * np.abs(x).min(1)))
    raises(R.assert_within, grads[1] - np.outer(g[row], x[row]), refs[1], bounds[1])
    raises(R.assert_within, grads[2] - g[row], refs[2], bounds[2])
    for got, r_, b_, idx in ((y, ref, bound, (77, 5)), (grads[0], refs[0], bounds[0], (77, 5)), (grads[1], refs[1], bounds[1], (3, 9)),
                             (grads[2], refs[2], bounds[2], (3,))):
        bad = got.astype(np.float64).copy()
        bad[idx] += 16 * b_[idx]
        raises(R.assert_within, bad, r_, b_)
    # the activation takes the wrong branch for one element: in y, and in the gradients
    pre = x.astype(np.float64) @ w.astype(np.float64).T + b
    idx = tuple(np.argwhere(pre > 0.5)[5])
    bad = y.copy()
    bad[idx] = -bad[idx]
    raises(R.mlp_forward_reference, x, w, b, slope, bad)
    flipped = mask.copy()
    flipped[idx] = False
    wrong, _ = R.mlp_backward_reference(x, w, gy, flipped, slope)
    for i in range(3):
        raises(R.assert_within, wrong[i], refs[i], bounds[i])
    # the exact run sees one row dropped or read twice, whatever its size
    xe, we, be, ge = R.mlp_exact_case(64 * 512 + 1, 4, 16, 0.0)
    pre = xe.astype(np.float64) @ we.T + be
    refs, _ = R.mlp_backward_reference(xe, we, ge, pre > 0, 0.0)
    R.assert_exact(refs[1].astype(np.float32), refs[1])
    g = ge * (pre > 0)
    row = int(np.argmax((np.abs(g).sum(1) > 0) & (np.abs(xe).sum(1) > 0)))
    raises(R.assert_exact, refs[1] - np.outer(g[row], xe[row]), refs[1])
    raises(R.assert_exact, refs[1] + np.outer(g[row], xe[row]), refs[1])


@pytest.mark.parametrize("slope", [0.5, 0.0, -1.0])
def test_linear_exact_case_is_exact_in_fp32(slope):
    x, w, b, gy = R.mlp_exact_case(70000, 127, 80, slope)
    pre = x.astype(np.float64) @ w.T + b
    y = pre if slope < 0 else np.where(pre > 0, pre, pre * slope)
    refs, _ = R.mlp_backward_reference(x, w, gy, None if slope < 0 else pre > 0, slope)
    for v in (y,) + refs:
        R.assert_exact(v.astype(np.float32), v)
    assert (pre > 0).mean() > 0.2 and (pre <= 0).mean() > 0.2


# ------------------------------------------------------------------------------------------------------------------ max-centre
def mc_cpu_case(n, K, c, kind, seed):
    rng = np.random.default_rng(seed)
    x = R.mc_input(n, K, c, kind, seed)
    gamma, beta = (rng.random(c) + 0.5).astype(np.float32), rng.standard_normal(c).astype(np.float32)
    g = rng.standard_normal((n, K, c)).astype(np.float32)
    xt, gt, bt = (torch.from_numpy(a).requires_grad_(True) for a in (x, gamma, beta))
    out = xt - (gt * xt.max(1, keepdim=True)[0] + bt)
    out.backward(torch.from_numpy(g))
    return x, gamma, beta, g, out.detach().numpy(), (xt.grad.numpy(), gt.grad.numpy(), bt.grad.numpy())


@pytest.mark.parametrize("kind", ["randn", "relu", "neginf", "nan"])
@pytest.mark.parametrize("c", [1, 5, 9, 16, 33, 64])
def test_torch_fp32_max_centre_passes_the_bounds(c, kind):
    """The torch expression on the CPU.  Which of several equal maxima (or NaNs) torch's backward picks is its own business: grad_x is
    compared on inputs without ties (randn), the forward and the parameter gradients everywhere they are finite."""
    for K in range(1, 9):
        n = (256 // c) * R.LN_MC_ITERS * (K % 3 + 1) + 1
        x, gamma, beta, g, out, grads = mc_cpu_case(n, K, c, kind, 100 * c + K)
        ref, bound, mx, am = R.mc_reference(x, gamma, beta)
        R.assert_within(out, ref, bound, f"K={K} out")
        refs, bounds = R.mc_backward_reference(g, mx, am, gamma)
        if kind == "randn":
            R.assert_within(grads[0], refs[0], bounds[0], f"K={K} grad_x")
        R.assert_within(grads[2], refs[2], bounds[2], f"K={K} grad_beta")
        if kind in ("randn", "relu"):
            R.assert_within(grads[1], refs[1], bounds[1], f"K={K} grad_gamma")


def test_max_centre_reference_follows_the_rule():
    nan, inf = np.nan, np.inf
    x = np.array([[1, 3, 3, 2], [0, 0, 0, 0], [5, nan, 7, nan], [-inf, -inf, -inf, -inf], [nan, inf, 1, 2], [2, inf, inf, 0]], np.float32)[:, :, None]
    out, _, mx, am = R.mc_reference(x, np.ones(1, np.float32), np.zeros(1, np.float32))
    assert am[:, 0].tolist() == [1, 0, 1, 0, 0, 1]
    assert np.array_equal(mx[:, 0], [3, 0, nan, -inf, nan, inf], equal_nan=True)
    assert np.array_equal(out[0, :, 0], [-2, 0, 0, -1]) and np.isnan(out[2:5]).all()
    (gx, _, _), (b_gx, _, _) = R.mc_backward_reference(np.ones_like(x), mx, am, np.ones(1))
    assert np.array_equal(gx[0, :, 0], [1, -3, 1, 1]) and np.array_equal(b_gx[0, :, 0] > 0, [False, True, False, False])
    assert R.mc_reference(np.zeros((0, 4, 9), np.float32), np.ones(9), np.zeros(9))[0].shape == (0, 4, 9)


def test_max_centre_planted_faults_are_caught():
    x, gamma, beta, g, out, grads = mc_cpu_case(3000, 4, 9, "randn", 1)
    ref, bound, mx, am = R.mc_reference(x, gamma, beta)
    refs, bounds = R.mc_backward_reference(g, mx, am, gamma)
    s = g.astype(np.float64).sum(1)
    p = int(np.argmax(np.abs(s).min(1)))
    raises(R.assert_within, grads[1] + s[p] * mx[p], refs[1], bounds[1])  # one point dropped
    raises(R.assert_within, grads[2] + s[p], refs[2], bounds[2])
    bad = out.astype(np.float64).copy()
    bad[5, 2, 3] += 16 * bound[5, 2, 3]
    raises(R.assert_within, bad, ref, bound)
    bad = grads[0].astype(np.float64).copy()
    bad[5, (am[5, 3] + 1) % 4, 3] += 1e-7  # off the arg-max the gradient is g itself: any change shows
    raises(R.assert_within, bad, refs[0], bounds[0])
    # the gradient sent to the second of two equal maxima (the mask bit of this operator)
    xr, gamma, beta, g, _, _ = mc_cpu_case(500, 4, 9, "relu", 2)
    _, _, mx, am = R.mc_reference(xr, gamma, beta)
    refs, bounds = R.mc_backward_reference(g, mx, am, gamma)
    tied = np.argwhere((xr == mx[:, None, :]).sum(1) > 1)[0]
    am2 = am.copy()
    am2[tuple(tied)] = np.argwhere(xr[tied[0], :, tied[1]] == mx[tuple(tied)])[1, 0]
    wrong, _ = R.mc_backward_reference(g, mx, am2, gamma)
    raises(R.assert_within, wrong[0], refs[0], bounds[0])
    # a NaN that is skipped
    xn = R.mc_input(300, 4, 9, "nan", 3)
    ref, bound, _, _ = R.mc_reference(xn, gamma, beta)
    skipped = xn - (gamma * np.nanmax(np.where(np.isnan(xn).all(1, keepdims=True), 0, xn), axis=1, keepdims=True) + beta)
    raises(R.assert_within, skipped, ref, bound)
