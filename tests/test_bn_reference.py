"""tests/bn_reference.py checked on the CPU (no GPU, no marker): the fp64 reference agrees with torch.nn.BatchNorm1d in float64, the
n < 2 rule is what the reference defines, a faithful emulation of the kernels' arithmetic passes every bound, and planted faults
(biased variance in the running update, a missing (1 - mom) factor, a padding row counted, evaluation mode on batch statistics) do
not."""
import numpy as np
import pytest
import torch

from tests import bn_reference as B
from tests import dense_reference as R

MOM, EPS = 0.1, 1e-5


def torch_layer(c, affine, gamma, beta, running_mean, running_var, training):
    bn = torch.nn.BatchNorm1d(c, eps=EPS, momentum=MOM, affine=affine).double()
    with torch.no_grad():
        if affine:
            bn.weight.copy_(torch.from_numpy(R.f64(gamma)))
            bn.bias.copy_(torch.from_numpy(R.f64(beta)))
        bn.running_mean.copy_(torch.from_numpy(R.f64(running_mean)))
        bn.running_var.copy_(torch.from_numpy(R.f64(running_var)))
    return bn.train(training)


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("training", [True, False], ids=["training", "evaluation"])
def test_reference_agrees_with_torch_float64(affine, training):
    """y, all three gradients and the running statistics after three consecutive calls (momentum 0.1) on different inputs: 1e-12."""
    m, c = 301, 8
    gamma, beta = R.gn_params(c, affine, 3)
    rm, rv = np.linspace(-1.0, 2.0, c), np.linspace(0.5, 3.0, c)
    bn = torch_layer(c, affine, gamma, beta, rm, rv, training)
    for step in range(3):
        x_np, gy_np = R.gn_input(m, c, 0.7, 1.9, 10 + step), R.gn_input(m, c, 0.0, 1.0, 20 + step)
        x = torch.from_numpy(R.f64(x_np)).requires_grad_(True)
        bn.zero_grad()
        y = bn(x)
        y.backward(torch.from_numpy(R.f64(gy_np)))
        y_ref, (dx, dgamma, dbeta), (rm, rv) = B.bn_layer_reference(x_np, gy_np, gamma, beta, rm, rv, MOM, EPS, training)
        what = f"step {step}"
        R.assert_within(y, y_ref, 1e-12, f"{what} y")
        R.assert_within(x.grad, dx, 1e-12, f"{what} grad_x")
        if affine:
            R.assert_within(bn.weight.grad, dgamma, 1e-12 * m, f"{what} grad_gamma")
            R.assert_within(bn.bias.grad, dbeta, 1e-12 * m, f"{what} grad_beta")
        R.assert_within(bn.running_mean, rm, 1e-12, f"{what} running_mean")
        R.assert_within(bn.running_var, rv, 1e-12, f"{what} running_var")
    assert int(bn.num_batches_tracked) == (3 if training else 0)


def test_reference_relu_and_static_rows_agree_with_torch_on_the_live_rows():
    """Fused ReLU and a row bound: torch on x[:rows] followed by relu is the same layer; the rows beyond are zeros."""
    m, c, rows = 120, 8, 77
    gamma, beta = R.gn_params(c, True, 1)
    rm, rv = np.zeros(c), np.ones(c)
    x_np, gy_np = R.gn_input(m, c, -0.3, 1.2, 1), R.gn_input(m, c, 0.0, 1.0, 2)
    x_np[rows:], gy_np[rows:] = 3e30, -1e30
    for training in (True, False):
        bn = torch_layer(c, True, gamma, beta, rm, rv, training)
        x = torch.from_numpy(R.f64(x_np[:rows])).requires_grad_(True)
        y = torch.relu(bn(x))
        y.backward(torch.from_numpy(R.f64(gy_np[:rows])))
        y_ref, (dx, dgamma, dbeta), (rm1, rv1) = B.bn_layer_reference(x_np, gy_np, gamma, beta, rm, rv, MOM, EPS, training, relu=True, rows=rows)
        R.assert_within(y, y_ref[:rows], 1e-12, "y")
        R.assert_within(x.grad, dx[:rows], 1e-12, "grad_x")
        R.assert_within(bn.weight.grad, dgamma, 1e-10, "grad_gamma")
        R.assert_within(bn.bias.grad, dbeta, 1e-10, "grad_beta")
        R.assert_within(bn.running_mean, rm1, 1e-12, "running_mean")
        R.assert_within(bn.running_var, rv1, 1e-12, "running_var")
        assert not y_ref[rows:].any() and not dx[rows:].any()


def test_fewer_than_two_rows_rule():
    """n < 2 (torch refuses one value per channel in training; the kernels decide on the device): the running statistics keep their
    bits, the single live row has variance 0 and rstd = 1 / sqrt(eps), y = act(beta); n = 0: zeros only."""
    m, c = 9, 8
    gamma, beta = R.gn_params(c, True, 5)
    rm, rv = np.linspace(-1.0, 1.0, c).astype(np.float32), np.linspace(0.5, 2.0, c).astype(np.float32)
    x, gy = R.gn_input(m, c, 3.0, 2.0, 1), R.gn_input(m, c, 0.0, 1.0, 2)
    for rows in (0, 1):
        (rm1, rv1), (b_rm, b_rv) = B.bn_running_reference(x, rm, rv, MOM, EPS, rows)
        assert np.array_equal(rm1, R.f64(rm)) and np.array_equal(rv1, R.f64(rv)) and not b_rm.any() and not b_rv.any()
        for relu in (False, True):
            y, (dx, dgamma, dbeta), stats = B.bn_layer_reference(x, gy, gamma, beta, rm, rv, MOM, EPS, True, relu=relu, rows=rows)
            assert np.array_equal(stats[0], R.f64(rm)) and np.array_equal(stats[1], R.f64(rv))
            assert not y[rows:].any() and not dx[rows:].any()
            if rows == 1:
                want = R.f64(beta)
                assert np.array_equal(y[0], np.maximum(want, 0) if relu else want)
        B.assert_bn_running(rm, rv, x, rm, rv, MOM, EPS, rows, "unchanged")
        with pytest.raises(AssertionError):
            B.assert_bn_running(np.nextafter(rm, np.float32(9)), rv, x, rm, rv, MOM, EPS, rows, "one ulp moved")
    mean, rstd, std = B.bn_statistics(x, EPS, 1)
    assert np.array_equal(mean, R.f64(x[0])) and not std.any() and np.allclose(rstd, 1.0 / np.sqrt(EPS), rtol=1e-15)


# ---- an emulation of the kernels' arithmetic, and the same with one fault planted ------------------------------------------------
def emulate(x, gy, gamma, beta, rm, rv, training, relu, rows, fault=None):
    """What the kernels compute, in NumPy: moments in fp64 (the fp32 part of k_gn_stats is dense_reference's subject), everything
    else with the kernels' roundings.  `fault`: biased_var | no_decay | padding_row | eval_batch_stats."""
    m, c = x.shape
    live = B.live_rows(m, rows)
    n_stat = live + 1 if fault == "padding_row" else live
    x64 = R.f64(x)
    g32 = np.ones(c, np.float32) if gamma is None else R.f32(gamma)
    b64 = np.zeros(c) if beta is None else R.f64(beta)
    batch = training or fault == "eval_batch_stats"
    new_rm, new_rv = R.f32(rm).copy(), R.f32(rv).copy()
    if batch:
        mean = x64[:n_stat].mean(0)
        var = ((x64[:n_stat] - mean) ** 2).mean(0)
        rstd = (1.0 / np.sqrt(var + np.float64(np.float32(EPS)))).astype(np.float32)
        if training and n_stat >= 2:
            keep = 1.0 if fault == "no_decay" else 1.0 - MOM
            unbias = 1.0 if fault == "biased_var" else n_stat / (n_stat - 1.0)
            new_rm = (keep * R.f64(rm) + MOM * mean).astype(np.float32)
            new_rv = (keep * R.f64(rv) + MOM * var * unbias).astype(np.float32)
    else:
        mean = R.f64(rm)
        rstd = (1.0 / np.sqrt(R.f64(rv) + np.float64(np.float32(EPS)))).astype(np.float32)
    a = g32 * rstd  # one fp32 product
    b = (b64 - mean * R.f64(a)).astype(np.float32)
    mean_rstd = np.concatenate([mean.astype(np.float32), rstd])
    scale_shift = np.concatenate([a, b])
    y = R.gn_apply_fp32(x, scale_shift, relu, rows)
    g = R.f64(gy[:live]) * ((y[:live] > 0) if relu else 1.0)
    dx = np.zeros((m, c), np.float32)
    if batch:
        (dx64, dgamma, dbeta), _ = B.bn_training_backward_reference(x, gy, (y > 0) if relu else None, gamma, mean_rstd, rows)
        dx = dx64.astype(np.float32)
    else:
        dx[:live] = (g.astype(np.float32) * a).astype(np.float32)
        dgamma = ((g * (x64[:live] - R.f64(mean_rstd[:c]))).sum(0) * R.f64(rstd))
        dbeta = g.sum(0)
    return dict(y=y, mean_rstd=mean_rstd, scale_shift=scale_shift, dx=dx, dgamma=dgamma.astype(np.float32), dbeta=dbeta.astype(np.float32),
                rm=new_rm, rv=new_rv)


def hold_to_reference(out, x, gy, gamma, beta, rm, rv, training, relu, rows):
    """Every check test_gpu_batch_norm.py applies to one call of the kernels."""
    mask = (out["y"] > 0) if relu else None
    if training:
        B.assert_bn_training_forward(out["y"], out["mean_rstd"], out["scale_shift"], x, gamma, beta, EPS, relu, rows, "emulation")
        ref, bound = B.bn_training_backward_reference(x, gy, mask, gamma, out["mean_rstd"], rows)
        B.assert_bn_running(out["rm"], out["rv"], x, rm, rv, MOM, EPS, rows, "emulation")
    else:
        B.assert_bn_eval_forward(out["y"], out["mean_rstd"], out["scale_shift"], x, gamma, beta, rm, rv, EPS, relu, rows, "emulation")
        ref, bound = B.bn_eval_backward_reference(x, gy, mask, out["mean_rstd"], out["scale_shift"], rows)
        R.assert_equal_bits(out["rm"], rm, "emulation running_mean")
        R.assert_equal_bits(out["rv"], rv, "emulation running_var")
    for name, r_, b_ in zip(("dx", "dgamma", "dbeta"), ref, bound):
        R.assert_within(out[name], r_, b_, f"emulation {name}")


def bound_case():
    m, c, rows = 300, 8, 299
    x, gy = R.gn_input(m, c, 1.5, 2.0, 4), R.gn_input(m, c, 0.0, 1.0, 5)
    x[rows:] = 50.0  # a padding row that is not even far away
    gamma, beta = R.gn_params(c, True, 6)
    rm, rv = np.linspace(1.0, 2.0, c).astype(np.float32), np.linspace(0.5, 3.0, c).astype(np.float32)
    return x, gy, gamma, beta, rm, rv, rows


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("training", [True, False], ids=["training", "evaluation"])
def test_faithful_emulation_is_within_every_bound(training, relu):
    x, gy, gamma, beta, rm, rv, rows = bound_case()
    hold_to_reference(emulate(x, gy, gamma, beta, rm, rv, training, relu, rows), x, gy, gamma, beta, rm, rv, training, relu, rows)
    hold_to_reference(emulate(x, gy, None, None, rm, rv, training, relu, None), x, gy, None, None, rm, rv, training, relu, None)


@pytest.mark.parametrize("fault,training", [("biased_var", True), ("no_decay", True), ("padding_row", True), ("eval_batch_stats", False)])
def test_planted_faults_are_caught(fault, training):
    x, gy, gamma, beta, rm, rv, rows = bound_case()
    out = emulate(x, gy, gamma, beta, rm, rv, training, False, rows, fault)
    with pytest.raises(AssertionError):
        hold_to_reference(out, x, gy, gamma, beta, rm, rv, training, False, rows)
    if fault in ("biased_var", "no_decay"):  # the forward is right, it is the running update that is held
        B.assert_bn_training_forward(out["y"], out["mean_rstd"], out["scale_shift"], x, gamma, beta, EPS, False, rows, fault)
        with pytest.raises(AssertionError):
            B.assert_bn_running(out["rm"], out["rv"], x, rm, rv, MOM, EPS, rows, fault)
