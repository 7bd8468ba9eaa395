"""The BatchNorm kernels (csrc/ln_norm.hip: ln_batch_norm_forward / _backward) against fp64, element by element (`pytest -m gpu`).

References, bounds and their counting arguments live in tests/bn_reference.py and tests/dense_reference.py (checked on the CPU by
test_bn_reference.py / test_dense_reference.py).  Training mode is GroupNorm at one channel per group and is held to GroupNorm's own
bounds; the running statistics, the evaluation mode and the n < 2 rule are held to the bounds of bn_reference.  The fp64 accumulator
atomics make the training statistics order-dependent in their last fp64 bits, so results are compared with bounds, and bit for bit
only where the operands are integers.  Each test prints its worst error / bound ratios (`pytest -s`); nothing is asserted on them.

A slab is the rows one workgroup of the statistics pass takes: rows_per_pass * 16 with rows_per_pass = 256 / (c / 4): 4096 rows at
c = 4, 256 at c = 64, 16 at c = 1024; more than 32 slabs wrap the 32 accumulator replicas."""
import numpy as np
import pytest
import torch

from tests import bn_reference as B
from tests import dense_reference as R

pytestmark = pytest.mark.gpu

MOM, EPS = 0.1, 1e-5
SENTINEL = -777.25
TAIL = 64  # sentinel rows / elements behind every output of a raw call


def dev():
    return torch.device("cuda", 0)


def gpu(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev()).requires_grad_(grad)


@pytest.fixture(autouse=True)
def native_path(monkeypatch):
    """Without a row count the module takes the kernels only with FUSED_BATCH_NORM: these tests are about the kernels."""
    from lattice_net_amd import lattice_blocks
    monkeypatch.setattr(lattice_blocks, "FUSED_BATCH_NORM", True)


def slab(c):
    return R.gn_rows_per_pass(c) * R.LN_GN_PASSES


def running_init(c, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-2.0, 2.0, c).astype(np.float32), rng.uniform(0.3, 3.0, c).astype(np.float32)


def bn_module(c, affine, params, stats, training, eps=EPS, momentum=MOM):
    bn = torch.nn.BatchNorm1d(c, eps=eps, momentum=momentum, affine=affine, track_running_stats=stats is not None).to(dev())
    with torch.no_grad():
        if affine:
            bn.weight.copy_(gpu(params[0]))
            bn.bias.copy_(gpu(params[1]))
        if stats is not None:
            bn.running_mean.copy_(gpu(stats[0]))
            bn.running_var.copy_(gpu(stats[1]))
    return bn.train(training)


def bn_forward(x_np, bn, relu, rows=None):
    """batch_norm_rows on the kernels, with the tensors the forward saves for the backward (mean_rstd, scale_shift)."""
    from lattice_net_amd.lattice_blocks import batch_norm_rows
    x = gpu(x_np, grad=True)
    rows_dev = None if rows is None else torch.tensor([rows], dtype=torch.int32, device=dev())
    y = batch_norm_rows(x, bn, relu, rows_dev)
    assert type(y.grad_fn).__name__.startswith("BatchNormFunction"), type(y.grad_fn).__name__
    _, _, mean_rstd, scale_shift = y.grad_fn.saved_tensors
    return x, y, mean_rstd, scale_shift


def merge(worst, ratios):
    for k, v in ratios.items():
        worst[k] = max(v, worst.get(k, 0.0))


def check_call(x_np, gy_np, gamma, beta, stats, training, relu, rows=None, eps=EPS, momentum=MOM, what=""):
    """One forward + backward through the Python layer, every output held to its bound.  Returns (worst ratios, new running stats)."""
    m, c = x_np.shape
    affine = gamma is not None
    bn = bn_module(c, affine, (gamma, beta), stats, training, eps, momentum)
    x, y, mean_rstd, scale_shift = bn_forward(x_np, bn, relu, rows)
    y.backward(gpu(gy_np))
    mask = (y.detach() > 0).cpu().numpy() if relu else None
    ratios = {}
    if training or stats is None:
        ratios.update(B.assert_bn_training_forward(y, mean_rstd, scale_shift, x_np, gamma, beta, eps, relu, rows, what))
        ref, bound = B.bn_training_backward_reference(x_np, gy_np, mask, gamma, mean_rstd, rows)
        if stats is not None:
            ratios["running_mean"], ratios["running_var"] = B.assert_bn_running(bn.running_mean, bn.running_var, x_np, stats[0], stats[1],
                                                                                momentum, eps, rows, what)
            assert int(bn.num_batches_tracked) == 1, what
    else:
        r = B.assert_bn_eval_forward(y, mean_rstd, scale_shift, x_np, gamma, beta, stats[0], stats[1], eps, relu, rows, what)
        ratios.update({"eval_a": r["a"], "eval_y": r["y"]})
        ref, bound = B.bn_eval_backward_reference(x_np, gy_np, mask, mean_rstd, scale_shift, rows)
        R.assert_equal_bits(bn.running_mean, stats[0], f"{what}: evaluation wrote running_mean")
        R.assert_equal_bits(bn.running_var, stats[1], f"{what}: evaluation wrote running_var")
        assert int(bn.num_batches_tracked) == 0, what
    got = (x.grad, bn.weight.grad if affine else None, bn.bias.grad if affine else None)
    for name, g_, r_, b_ in zip(("grad_x", "grad_gamma", "grad_beta"), got, ref, bound):
        if g_ is None:
            continue
        R.assert_within(g_, r_, b_, f"{what} {name}")
        ratios[("" if training else "eval_") + name] = R.worst_ratio(g_, r_, b_)
    new_stats = None if stats is None else (R.f32(bn.running_mean), R.f32(bn.running_var))
    return ratios, new_stats


# ------------------------------------------------------------------------------------------------------------------ random
@pytest.mark.parametrize("training", [True, False], ids=["training", "evaluation"])
@pytest.mark.parametrize("c", [4, 32, 64, 1024])
def test_batch_norm_random(c, training):
    """Rows 2, slab - 1, slab, slab + 1 and 33 slabs + 3 (every accumulator replica, the first one twice), affine on and off, ReLU on
    and off: every output, gradient, mean_rstd, scale_shift and running statistic within its bound, element by element."""
    s = slab(c)
    worst = {}
    case = 0
    for m in (2, s - 1, s, s + 1, 33 * s + 3):
        x = R.gn_input(m, c, 0.5, 2.0, 1000 * c + m)
        gy = R.gn_input(m, c, 0.0, 1.0, 2000 * c + m)
        for affine in (True, False):
            for relu in (False, True):
                case += 1
                gamma, beta = R.gn_params(c, affine, case)
                r, _ = check_call(x, gy, gamma, beta, running_init(c, case), training, relu,
                                  what=f"c={c} m={m} affine={affine} relu={relu} training={training}")
                merge(worst, r)
    print(f"BatchNorm random c={c} {'training' if training else 'evaluation'}: worst error / bound {worst}")


def test_batch_norm_without_running_statistics():
    """track_running_stats=False: batch statistics in training and in evaluation mode, nothing to update."""
    m, c = 777, 32
    x, gy = R.gn_input(m, c, -1.0, 1.5, 1), R.gn_input(m, c, 0.0, 1.0, 2)
    gamma, beta = R.gn_params(c, True, 3)
    for training in (True, False):
        r, _ = check_call(x, gy, gamma, beta, None, training, True, what=f"no running statistics, training={training}")
    print(f"BatchNorm without running statistics: worst error / bound {r}")


# ------------------------------------------------------------------------------------------------------------------ exact
def exact_stats(c):
    """Integer running means, running variance 4 (rstd = 1/2 with eps = 0)."""
    return ((np.arange(c) % 3) - 1).astype(np.float32), np.full(c, 4.0, np.float32)


def check_exact(m, c, relu, training, rows=None, what=""):
    """dense_reference.gn_exact_input at one channel per group: mean[ch] = ch % 5 - 2, variance 4, rstd = 1/2 bit for bit with eps = 0.
    Training: y, dgamma, dbeta the integer results and, with momentum 1/2 and integer running means, the new running mean bit for bit;
    dx = g' gamma rstd + x c2 + c3 divides by the row count: bit for bit where that is a power of two (as the GroupNorm exact run),
    within its bound elsewhere.  Evaluation with running_var = 4: everything bit for bit."""
    live = B.live_rows(m, rows)
    assert live % 2 == 0 and live > 0
    x_np, gy_np = R.gn_exact_input(m, c, c), R.gn_exact_grad(m, c)
    if live < m:
        x_np[live:], gy_np[live:] = 3e30, -2e30
    gamma, beta = R.gn_exact_params(c)
    rm, rv = exact_stats(c)
    bn = bn_module(c, True, (gamma, beta), (rm, rv), training, eps=0.0, momentum=0.5)
    x, y, mean_rstd, scale_shift = bn_forward(x_np, bn, relu, rows)
    y.backward(gpu(gy_np))
    mean = (np.arange(c) % 5 - 2).astype(np.float64) if training else R.f64(rm)
    R.assert_exact(mean_rstd[:c], mean, f"{what} mean")
    R.assert_exact(mean_rstd[c:] * 2, np.ones(c), f"{what} 2 rstd")
    a = R.f64(gamma) / 2
    b = R.f64(beta) - mean * a
    R.assert_exact(scale_shift, np.concatenate([a, b]), f"{what} scale_shift")
    y_ref = np.zeros((m, c))
    y_ref[:live] = R.f64(x_np[:live]) * a + b
    if relu:
        y_ref = np.maximum(y_ref, 0)
    R.assert_exact(y, y_ref, f"{what} y")
    mask = (y_ref > 0) if relu else None
    g = R.f64(gy_np[:live]) * (mask[:live] if relu else 1.0)
    R.assert_exact(bn.weight.grad, (g * (R.f64(x_np[:live]) - mean)).sum(0) / 2, f"{what} grad_gamma")
    R.assert_exact(bn.bias.grad, g.sum(0), f"{what} grad_beta")
    if training:
        R.assert_exact(bn.running_mean * 2, R.f64(rm) + mean, f"{what} 2 running_mean")
        B.assert_bn_running(bn.running_mean, bn.running_var, x_np, rm, rv, 0.5, 0.0, rows, what)
        ref, bound = B.bn_training_backward_reference(x_np, gy_np, mask, gamma, mean_rstd, rows)
        R.assert_within(x.grad, ref[0], bound[0], f"{what} grad_x")
        if live & (live - 1) == 0 and live <= 2 ** 15:
            assert np.array_equal(ref[0].astype(np.float32).astype(np.float64), ref[0]), f"{what}: grad_x is not exact in fp32"
            R.assert_within(x.grad, ref[0], 0.0, f"{what} grad_x (exact)")
            return True
    else:
        dx = np.zeros((m, c))
        dx[:live] = g * a
        R.assert_exact(x.grad, dx, f"{what} grad_x")
        R.assert_equal_bits(bn.running_mean, rm, f"{what} running_mean")
        R.assert_equal_bits(bn.running_var, rv, f"{what} running_var")
        return True
    return False


@pytest.mark.parametrize("c", [4, 32, 64, 1024])
def test_batch_norm_exact(c):
    s = slab(c)
    bitwise_dx = 0
    for m in (2, s, s + 2, 2 * s, 33 * s + 4):
        for relu in (False, True):
            bitwise_dx += check_exact(m, c, relu, True, what=f"exact training c={c} m={m} relu={relu}")
            check_exact(m, c, relu, False, what=f"exact evaluation c={c} m={m} relu={relu}")
    assert bitwise_dx >= 6  # (2, slab and 2 slabs of rows are powers of two)


# ------------------------------------------------------------------------------------------------------------------ static rows
def tail_buffer(rows, cols=None):
    """(whole buffer, the part the kernel may write): TAIL sentinel rows / elements behind it."""
    whole = torch.full((rows + TAIL,) if cols is None else (rows + TAIL, cols), SENTINEL, dtype=torch.float32, device=dev())
    return whole, whole[:rows]


def raw_call(x_np, gy_np, gamma, beta, stats, training, relu, rows, eps=EPS, momentum=MOM):
    """ln_batch_norm_forward + _backward on buffers of the test's own, each with sentinels behind it, one zeroed workspace per call and
    no next_workspace (the library then zero-fills itself).  Returns the outputs, the return codes and the sentinel check."""
    from lattice_net_amd import _lib
    lib = _lib.load()
    m, c = x_np.shape
    x, gy = gpu(x_np), gpu(gy_np)
    g_, b_ = (None, None) if gamma is None else (gpu(gamma), gpu(beta))
    bufs = {"y": tail_buffer(m, c), "grad_x": tail_buffer(m, c), "mean_rstd": tail_buffer(2 * c), "scale_shift": tail_buffer(2 * c),
            "grad_gamma": tail_buffer(c), "grad_beta": tail_buffer(c), "running_mean": tail_buffer(c), "running_var": tail_buffer(c)}
    bufs["running_mean"][1].copy_(gpu(stats[0]))
    bufs["running_var"][1].copy_(gpu(stats[1]))
    rows_dev = None if rows is None else torch.tensor([rows], dtype=torch.int32, device=dev())
    ws = torch.full((int(lib.ln_batch_norm_workspace_bytes(c)) // 8,), 1e300, dtype=torch.float64, device=dev())  # (dirty on purpose)
    o = {k: v[1] for k, v in bufs.items()}
    stream = _lib.stream_ptr(dev())
    rc_f = lib.ln_batch_norm_forward(_lib.ptr(x), _lib.ptr(g_), _lib.ptr(b_), _lib.ptr(o["running_mean"]), _lib.ptr(o["running_var"]), m, c, eps,
                                     momentum, int(training), int(relu), _lib.ptr(o["y"]), _lib.ptr(o["mean_rstd"]), _lib.ptr(o["scale_shift"]),
                                     _lib.ptr(ws), ws.numel() * 8, None, 0, _lib.ptr(rows_dev), stream)
    rc_b = lib.ln_batch_norm_backward(_lib.ptr(x), _lib.ptr(gy), _lib.ptr(g_), _lib.ptr(o["mean_rstd"]), _lib.ptr(o["scale_shift"]), m, c,
                                      int(training), int(relu), _lib.ptr(o["grad_x"]), _lib.ptr(o["grad_gamma"]) if gamma is not None else None,
                                      _lib.ptr(o["grad_beta"]) if gamma is not None else None, _lib.ptr(ws), ws.numel() * 8, None, 0,
                                      _lib.ptr(rows_dev), stream)
    torch.cuda.synchronize()

    def sentinels_intact():
        for name, (whole, part) in bufs.items():
            assert bool((whole[part.shape[0]:] == SENTINEL).all()), f"{name}: the sentinels behind it were overwritten"

    return o, (rc_f, rc_b), sentinels_intact


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("training", [True, False], ids=["training", "evaluation"])
def test_batch_norm_static_rows(training, relu):
    """rows_device holding 0, 1, 2, m - 1, m, m + 5 on a tensor whose dead rows hold large finite garbage: statistics and gradients of
    the live rows only, exact zeros beyond them, the running statistics bitwise unchanged at 0 and 1 rows (and in evaluation mode
    always), the sentinels behind every output intact."""
    m, c = 1100, 64
    worst = {}
    for rows in (0, 1, 2, m - 1, m, m + 5):
        live = min(rows, m)
        x = R.gn_input(m, c, 1.0, 2.0, 20 + rows % 7)
        gy = R.gn_input(m, c, 0.0, 1.0, 30 + rows % 7)
        x[live:] = 3e30 * np.where(np.arange(c) % 2, -1, 1)
        gy[live:] = -1e30
        gamma, beta = R.gn_params(c, True, rows)
        stats = running_init(c, rows)
        what = f"rows_dev={rows} training={training} relu={relu}"
        o, rcs, sentinels_intact = raw_call(x, gy, gamma, beta, stats, training, relu, rows)
        assert rcs == (0, 0), what
        sentinels_intact()
        for name in ("y", "mean_rstd", "scale_shift", "grad_x", "grad_gamma", "grad_beta", "running_mean", "running_var"):
            assert bool(torch.isfinite(o[name]).all()), f"{what}: {name} is not finite"
        assert not bool(o["y"][live:].any()) and not bool(o["grad_x"][live:].any()), f"{what}: not zero in the dead rows"
        mask = (o["y"] > 0).cpu().numpy() if relu else None
        if training:
            merge(worst, B.assert_bn_training_forward(o["y"], o["mean_rstd"], o["scale_shift"], x, gamma, beta, EPS, relu, rows, what))
            ref, bound = B.bn_training_backward_reference(x, gy, mask, gamma, o["mean_rstd"], rows)
            r = B.assert_bn_running(o["running_mean"], o["running_var"], x, stats[0], stats[1], MOM, EPS, rows, what)
            merge(worst, {"running_mean": r[0], "running_var": r[1]})
            if live < 2:
                R.assert_equal_bits(o["running_mean"], stats[0], f"{what} running_mean")
                R.assert_equal_bits(o["running_var"], stats[1], f"{what} running_var")
        else:
            B.assert_bn_eval_forward(o["y"], o["mean_rstd"], o["scale_shift"], x, gamma, beta, stats[0], stats[1], EPS, relu, rows, what)
            ref, bound = B.bn_eval_backward_reference(x, gy, mask, o["mean_rstd"], o["scale_shift"], rows)
            R.assert_equal_bits(o["running_mean"], stats[0], f"{what} running_mean")
            R.assert_equal_bits(o["running_var"], stats[1], f"{what} running_var")
        for name, r_, b_ in zip(("grad_x", "grad_gamma", "grad_beta"), ref, bound):
            R.assert_within(o[name], r_, b_, f"{what} {name}")
            merge(worst, {name: R.worst_ratio(o[name], r_, b_)})
        if live > 0 and live % 2 == 0:
            check_exact(m, c, relu, training, rows, what=f"{what} exact")
    print(f"BatchNorm static rows training={training} relu={relu}: worst error / bound {worst}")


def test_batch_norm_one_live_row_is_beta():
    """n = 1: variance 0, rstd = 1 / sqrt(eps), y = act(beta) up to the rounding of x a + (beta - x a)."""
    m, c = 40, 32
    x, gy = R.gn_input(m, c, 2.0, 1.0, 1), R.gn_input(m, c, 0.0, 1.0, 2)
    gamma, beta = R.gn_params(c, True, 4)
    o, rcs, sentinels_intact = raw_call(x, gy, gamma, beta, running_init(c, 1), True, False, 1)
    assert rcs == (0, 0)
    sentinels_intact()
    R.assert_equal_bits(o["mean_rstd"][:c], x[0], "mean of one row")
    want = np.float32(1.0 / np.sqrt(np.float64(np.float32(EPS))))
    R.assert_equal_bits(o["mean_rstd"][c:], np.full(c, want), "rstd of one row")
    a = R.f64(o["scale_shift"][:c])
    R.assert_within(o["y"][0], R.f64(beta), 3 * R.EPS32 * (np.abs(R.f64(x[0]) * a) + np.abs(R.f64(o["scale_shift"][c:]))), "y of one row")


# ------------------------------------------------------------------------------------------------------------------ conditioning
@pytest.mark.parametrize("m,c", [(5000, 32), (901, 320)])
@pytest.mark.parametrize("mean,std", [(0.25, 1.0), (100.0, 1.0), (1000.0, 1.0), (30.0, 0.01)], ids=["0.25", "100", "1000", "30+0.01N"])
def test_batch_norm_conditioning(m, c, mean, std):
    """Inputs mean + std N(0, 1) with |mean| up to 3000 std: rstd within 1e-5 relative, mean within 1e-6 (|mean| + std), and the
    running variance within the allowance that follows from them."""
    x = R.gn_conditioning_input(m, c, mean, std)
    gy = R.gn_input(m, c, 0.0, 1.0, m + c + 1)
    gamma, beta = R.gn_params(c, True, 1)
    r, _ = check_call(x, gy, gamma, beta, running_init(c, 2), True, True, what=f"{m}x{c} {mean}+{std}N")
    print(f"BatchNorm conditioning {m}x{c} {mean}+{std}N: worst error / bound {r}")


@pytest.mark.parametrize("row", [0, 2500])
def test_batch_norm_outlier_row(row):
    """One row 3000 standard deviations from the rest — row 0 (the "invalid" vertex of a lattice) or one in the middle, with and
    without a static row bound."""
    worst = {}
    for m, c, rows in ((5000, 4, None), (5000, 32, None), (5000, 32, 4000)):
        x, gy = R.gn_outlier_input(m, c, row, 3000.0, 7), R.gn_input(m, c, 0.0, 1.0, 8)
        if rows is not None:
            x[rows:], gy[rows:] = 3e30, -1e30
        gamma, beta = R.gn_params(c, True, 1)
        r, _ = check_call(x, gy, gamma, beta, running_init(c, 3), True, True, rows=rows, what=f"{m}x{c} rows_dev={rows} row {row} at 3000 sigma")
        merge(worst, r)
    print(f"BatchNorm outlier row {row}: worst error / bound {worst}")


# ------------------------------------------------------------------------------------------------------------------ sequence
def test_batch_norm_evaluation_writes_no_statistics():
    """Evaluation forward + backward, several times, with and without ReLU: running statistics and the batch counter keep their bits."""
    m, c = 3000, 64
    stats = running_init(c, 9)
    bn = bn_module(c, True, R.gn_params(c, True, 2), stats, False)
    for k in range(3):
        x, y, _, _ = bn_forward(R.gn_input(m, c, 5.0, 3.0, k), bn, k % 2 == 1, rows=None if k == 0 else m - k)
        y.backward(gpu(R.gn_input(m, c, 0.0, 1.0, 10 + k)))
    R.assert_equal_bits(bn.running_mean, stats[0], "running_mean after evaluation calls")
    R.assert_equal_bits(bn.running_var, stats[1], "running_var after evaluation calls")
    assert int(bn.num_batches_tracked) == 0


@pytest.mark.parametrize("calls", [3, 5])
def test_batch_norm_sequence_of_training_calls(calls):
    """`calls` training forwards in a row on different inputs, on one stream and without a backward (an odd number of launches on the
    alternating workspace pair): every call within its bounds, the running statistics follow the fp64 recurrence — each step from
    the kernel's own previous value within the one-step bound, and the whole chain from the start with the bounds carried along
    (bound' = (1 - mom) bound + step bound) — and num_batches_tracked counts."""
    m, c = 5000, 96
    gamma, beta = R.gn_params(c, True, 1)
    start = running_init(c, 4)
    bn = bn_module(c, True, (gamma, beta), start, True)
    xs = [R.gn_input(m, c, 3.0 - k, 2.0 + 0.5 * k, 50 + k) for k in range(calls)]
    outs, stats = [], []
    for k in range(calls):
        outs.append(bn_forward(xs[k], bn, True))
        stats.append((bn.running_mean.clone(), bn.running_var.clone()))
    worst = {}
    chain, chain_bound = (R.f64(start[0]), R.f64(start[1])), (np.zeros(c), np.zeros(c))
    prev = start
    for k, (_, y, mean_rstd, scale_shift) in enumerate(outs):
        merge(worst, B.assert_bn_training_forward(y, mean_rstd, scale_shift, xs[k], gamma, beta, EPS, True, None, f"call {k}"))
        r = B.assert_bn_running(stats[k][0], stats[k][1], xs[k], prev[0], prev[1], MOM, EPS, None, f"call {k}")
        merge(worst, {"running_mean": r[0], "running_var": r[1]})
        chain, step_bound = B.bn_running_reference(xs[k], chain[0], chain[1], MOM, EPS)
        chain_bound = tuple((1.0 - MOM) * cb + sb for cb, sb in zip(chain_bound, step_bound))
        R.assert_within(stats[k][0], chain[0], chain_bound[0], f"call {k} running_mean against the fp64 recurrence")
        R.assert_within(stats[k][1], chain[1], chain_bound[1], f"call {k} running_var against the fp64 recurrence")
        prev = (R.f32(stats[k][0]), R.f32(stats[k][1]))
    assert int(bn.num_batches_tracked) == calls
    for relu in (False, True):  # the pair is still sound: integers come out as integers
        check_exact(2 * slab(c), c, relu, True, what=f"exact after {calls} calls")
    print(f"BatchNorm {calls} training calls: worst error / bound {worst}")


def test_batch_norm_after_a_rejected_call():
    """6 channels (not a multiple of 4) and an x 4 bytes off 16-byte alignment are refused with their error codes and launch nothing:
    outputs and running statistics keep their contents, and the next valid calls are right."""
    from lattice_net_amd import _lib
    lib = _lib.load()
    m, c = 3000, 32
    x_np, gy_np = R.gn_input(m, c, 2.0, 1.5, 11), R.gn_input(m, c, 0.0, 1.0, 12)
    gamma, beta = R.gn_params(c, True, 2)
    check_call(x_np, gy_np, gamma, beta, running_init(c, 5), True, False, what="before")  # (this stream's pair is in its steady state)
    stream = _lib.stream_ptr(dev())
    ws = torch.zeros((int(lib.ln_batch_norm_workspace_bytes(32)) // 8,), dtype=torch.float64, device=dev())
    for channels, offset, code in ((6, 0, -2), (32, 1, -1)):  # LN_ERR_UNSUPPORTED, LN_ERR_ARG
        x = torch.zeros((m * channels + 4,), device=dev())[offset:offset + m * channels]
        y, mr, ss = torch.full((m * channels,), SENTINEL, device=dev()), torch.full((2 * channels,), SENTINEL, device=dev()), \
            torch.full((2 * channels,), SENTINEL, device=dev())
        rm, rv = torch.full((channels,), 0.5, device=dev()), torch.full((channels,), 1.5, device=dev())
        for training in (1, 0):
            rc = lib.ln_batch_norm_forward(_lib.ptr(x), None, None, _lib.ptr(rm), _lib.ptr(rv), m, channels, EPS, MOM, training, 0, _lib.ptr(y),
                                           _lib.ptr(mr), _lib.ptr(ss), _lib.ptr(ws), ws.numel() * 8, None, 0, None, stream)
            assert rc == code, (channels, offset, training, rc)
            rc = lib.ln_batch_norm_backward(_lib.ptr(x), _lib.ptr(x), None, _lib.ptr(mr), _lib.ptr(ss), m, channels, training, 0, _lib.ptr(y), None,
                                            None, _lib.ptr(ws), ws.numel() * 8, None, 0, None, stream)
            assert rc == code, (channels, offset, training, rc)
        torch.cuda.synchronize()
        assert bool((y == SENTINEL).all()) and bool((mr == SENTINEL).all()) and bool((ss == SENTINEL).all())
        assert bool((rm == 0.5).all()) and bool((rv == 1.5).all()) and not bool(ws.any())
    # evaluation mode without running statistics is an argument error
    x = torch.zeros((m, c), device=dev())
    rc = lib.ln_batch_norm_forward(_lib.ptr(x), None, None, None, None, m, c, EPS, MOM, 0, 0, _lib.ptr(x), _lib.ptr(ws), _lib.ptr(ws), _lib.ptr(ws),
                                   ws.numel() * 8, None, 0, None, stream)
    assert rc == -1
    for k in range(2):
        check_call(x_np, gy_np, gamma, beta, running_init(c, 6 + k), k == 0, True, what=f"after the rejected calls, {k}")


# ------------------------------------------------------------------------------------------------------------------ module
def test_batch_norm_modules_under_static_rows():
    """BatchNormLatticeModule and BnReluConv on a small lattice under set_static_rows(bound) (they raised there before the kernels
    existed): the norm agrees with the fp64 reference on the live rows and is zero beyond them, in training and in evaluation mode;
    the state_dict keys are torch.nn.BatchNorm1d's; a plain BatchNorm1d loaded with them gives the same evaluation output;
    num_batches_tracked counts."""
    from lattice_net_amd import Lattice
    from lattice_net_amd import lattice_blocks as blocks
    from lattice_net_amd.synthetic import cube_cloud
    torch.manual_seed(0)
    pos = torch.from_numpy(cube_cloud(2000, 3)).to(dev())
    lat = Lattice(sigmas=[0.2] * 3, capacity=40000, device=dev())
    lat.begin_splat()
    lat.just_create_verts(pos, False)
    lat.set_positions(pos)
    live = lat.nr_lattice_vertices()
    bound = (int(live * 1.07) + 255) // 256 * 256
    lat.set_static_rows(bound)
    lat.begin_splat()
    lat.just_create_verts(pos, False)
    lat.set_positions(pos)
    assert lat.nr_lattice_vertices() == bound and int(lat.rows_device()) == live and live < bound
    c = 16
    x_np, gy_np = R.gn_input(bound, c, 0.8, 1.7, 1), R.gn_input(bound, c, 0.0, 1.0, 2)
    x_np[live:], gy_np[live:] = 3e30, -1e30
    worst = {}

    mod = blocks.BatchNormLatticeModule(c, device=dev())
    assert set(mod.state_dict()) == {"bn.weight", "bn.bias", "bn.running_mean", "bn.running_var", "bn.num_batches_tracked"}
    gamma, beta = R.gn_params(c, True, 1)
    with torch.no_grad():
        mod.bn.weight.copy_(gpu(gamma))
        mod.bn.bias.copy_(gpu(beta))
    stats = (R.f32(mod.bn.running_mean), R.f32(mod.bn.running_var))
    for k in range(2):  # two training calls
        x = gpu(x_np, grad=True)
        y, ls = mod(x, lat)
        assert ls is lat and y.shape == (bound, c)
        _, _, mean_rstd, scale_shift = y.grad_fn.saved_tensors
        y.backward(gpu(gy_np))
        merge(worst, B.assert_bn_training_forward(y, mean_rstd, scale_shift, x_np, gamma, beta, mod.bn.eps, False, live, f"module call {k}"))
        r = B.assert_bn_running(mod.bn.running_mean, mod.bn.running_var, x_np, stats[0], stats[1], 0.1, mod.bn.eps, live, f"module call {k}")
        merge(worst, {"running_mean": r[0], "running_var": r[1]})
        ref, bnd = B.bn_training_backward_reference(x_np, gy_np, None, gamma, mean_rstd, live)
        for name, g_, r_, b_ in zip(("grad_x", "grad_gamma", "grad_beta"), (x.grad, mod.bn.weight.grad, mod.bn.bias.grad), ref, bnd):
            R.assert_within(g_, r_, b_, f"module call {k} {name}")
        mod.zero_grad()
        stats = (R.f32(mod.bn.running_mean), R.f32(mod.bn.running_var))
    assert int(mod.bn.num_batches_tracked) == 2
    assert set(mod.state_dict()) == {"bn.weight", "bn.bias", "bn.running_mean", "bn.running_var", "bn.num_batches_tracked"}

    mod.eval()
    y, _ = mod(gpu(x_np), lat, fuse_relu=True)
    plain = torch.nn.BatchNorm1d(c).to(dev())
    plain.load_state_dict({k[3:]: v for k, v in mod.state_dict().items()})
    plain.eval()
    with torch.no_grad():
        y_plain = torch.relu(plain(gpu(x_np[:live])))
    assert not bool(y[live:].any())
    # Both are within their own roundings of the fp64 value: the kernel 3 (fl(fl(x a) + b), one spare) on |x a| + |b|; torch's
    # ((x - mean) invstd) w + b at most 5 on |x a| + |mean a| (the subtraction, invstd, two products, the sum) and 1 on |beta|.
    rstd, a, b = B.bn_eval_affine_reference(gamma, beta, stats[0], stats[1], mod.bn.eps)
    xa = np.abs(R.f64(x_np[:live]) * a)
    tol = R.EPS32 * (3 * (xa + np.abs(b)) + 6 * (xa + np.abs(R.f64(stats[0]) * a) + np.abs(R.f64(beta))))
    y_ref = np.maximum(R.f64(x_np[:live]) * a + b, 0)
    R.assert_within(y[:live], y_ref, tol, "module evaluation against fp64")
    R.assert_within(y_plain, y_ref, tol, "torch evaluation against fp64")
    R.assert_within(y[:live], R.f64(y_plain), tol, "module evaluation against a plain BatchNorm1d with the same state")
    assert int(mod.bn.num_batches_tracked) == 2

    # BnReluConv: the norm + ReLU it hands to its convolution
    block = blocks.BnReluConv(c, c, 1, False, device=dev())
    seen = {}
    block.conv.register_forward_pre_hook(lambda module, args: seen.__setitem__("lv", args[0]))
    x = gpu(x_np, grad=True)
    out, _ = block(x, lat)
    assert out.shape == (bound, c) and bool(torch.isfinite(out).all())
    lv = seen["lv"]
    assert type(lv.grad_fn).__name__.startswith("BatchNormFunction"), "BnReluConv did not fuse its ReLU into the norm"
    _, _, mean_rstd, scale_shift = lv.grad_fn.saved_tensors
    merge(worst, B.assert_bn_training_forward(lv, mean_rstd, scale_shift, x_np, R.f32(block.bn.bn.weight), R.f32(block.bn.bn.bias), block.bn.bn.eps,
                                              True, live, "BnReluConv"))
    out.backward(gpu(np.where(np.arange(bound)[:, None] < live, gy_np, 0.0).astype(np.float32)))
    assert bool(torch.isfinite(x.grad).all()) and not bool(x.grad[live:].any()) and bool(x.grad[:live].any())
    assert int(block.bn.bn.num_batches_tracked) == 1
    lat.set_static_rows(None)
    print(f"BatchNorm modules under static rows: worst error / bound {worst}")


def test_batch_norm_static_rows_still_refuses_what_the_kernels_cannot_take():
    from lattice_net_amd.lattice_blocks import batch_norm_rows
    rows_dev = torch.tensor([5], dtype=torch.int32, device=dev())
    for c, dtype, momentum in ((6, torch.float32, 0.1), (8, torch.float64, 0.1), (8, torch.float32, None)):
        bn = torch.nn.BatchNorm1d(c, momentum=momentum).to(dev()).to(dtype)
        with pytest.raises(ValueError):
            batch_norm_rows(torch.zeros((10, c), dtype=dtype, device=dev()), bn, False, rows_dev)


# ------------------------------------------------------------------------------------------------------------------ graph replay
def test_batch_norm_graph_replay():
    """Forward + backward of BatchNormFunction with a device row count, captured on one side stream with a private accumulator pair
    (reset first, as CapturedNetworkStep does; one stream, so the graph has no parallel branches).  Two warm-up steps and three replays,
    the input overwritten in place and the row count changed between them: outputs of every replay within their bounds, running
    statistics following the reference for warm-ups + replays steps (the capture itself runs nothing)."""
    from lattice_net_amd.lattice_blocks import BatchNormFunction, new_gn_workspace, reset_gn_workspaces, use_gn_workspace
    m, c = 2000, 32
    gamma, beta = R.gn_params(c, True, 3)
    start = running_init(c, 8)
    w, b = gpu(gamma, grad=True), gpu(beta, grad=True)
    rm, rv = gpu(start[0]), gpu(start[1])
    x = torch.zeros((m, c), device=dev(), requires_grad=True)
    gy = torch.zeros((m, c), device=dev())
    rows_dev = torch.zeros((1,), dtype=torch.int32, device=dev())
    steps = [(R.gn_input(m, c, 1.0 + k, 1.0 + 0.3 * k, 70 + k), R.gn_input(m, c, 0.0, 1.0, 80 + k), rows) for k, rows in enumerate((m, m - 7, m, 1500, m + 9))]
    for x_np, gy_np, rows in steps:
        x_np[min(rows, m):], gy_np[min(rows, m):] = 3e30, -1e30
    entry = new_gn_workspace(dev())

    def load(k):
        with torch.no_grad():
            x.copy_(gpu(steps[k][0]))
            gy.copy_(gpu(steps[k][1]))
            rows_dev.fill_(steps[k][2])

    def step():
        reset_gn_workspaces()
        y = BatchNormFunction.apply(x, w, b, (rm, rv), MOM, EPS, True, True, rows_dev)
        _, _, mean_rstd, scale_shift = y.grad_fn.saved_tensors  # (tensors of the graph's pool, rewritten by every replay)
        return (y, mean_rstd, scale_shift) + torch.autograd.grad(y, (x, w, b), gy)

    prev, worst = start, {}

    def check(k, outs):
        nonlocal prev
        x_np, gy_np, rows = steps[k]
        y, mean_rstd, scale_shift, gx, gw, gb = outs
        what = f"step {k} (rows_dev={rows})"
        live = min(rows, m)
        assert not bool(gx[live:].any()), what
        merge(worst, B.assert_bn_training_forward(y, mean_rstd, scale_shift, x_np, gamma, beta, EPS, True, rows, what))
        ref, bound = B.bn_training_backward_reference(x_np, gy_np, (y > 0).cpu().numpy(), gamma, mean_rstd, rows)
        for name, g_, r_, b_ in zip(("grad_x", "grad_gamma", "grad_beta"), (gx, gw, gb), ref, bound):
            R.assert_within(g_, r_, b_, f"{what} {name}")
            merge(worst, {name: R.worst_ratio(g_, r_, b_)})
        r = B.assert_bn_running(rm, rv, x_np, prev[0], prev[1], MOM, EPS, rows, what)
        merge(worst, {"running_mean": r[0], "running_var": r[1]})
        prev = (R.f32(rm), R.f32(rv))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), use_gn_workspace(entry):
        for k in range(2):  # warm-up
            load(k)
            outs = step()
            side.synchronize()
            check(k, outs)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            static = step()
    torch.cuda.synchronize()
    R.assert_equal_bits(rm, prev[0], "the capture itself moved running_mean")
    with torch.cuda.stream(side):
        for k in range(2, 5):
            load(k)
            graph.replay()
            side.synchronize()
            check(k, static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    print(f"BatchNorm graph replay (2 warm-ups + 3 replays): worst error / bound {worst}")
