"""The per-cloud, class-weighted NLL loss as HIP kernels (ln_nll_forward_clouds / ln_nll_backward_clouds, csrc/ln_nll.hip) against the
fp64 reference and the counted bounds of tests/nll_clouds_reference.py: every output element by element at every kernel form (a wave per
cloud, one workgroup per cloud, partials + finish fused or on a grid), cloud by cloud bit for bit against the call on the slice and
against ln_nll_forward / ln_nll_backward, exact runs against the fp32 emulation, reproducibility (also under graph replay), guard words,
refusals, and through losses.NLLLoss / nll_loss_gather."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from . import nll_clouds_reference as R

pytestmark = pytest.mark.gpu

NO_LABEL = R.NO_LABEL
GUARD = 64  # guard words behind every buffer
CLASSES = (1, 3, 20)
POINTS_PER_CLOUD = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)  # 64: a wave per cloud up to here; 1024: one workgroup per cloud
CLOUDS = (1, 2, 3, 64)
SHARES = (0.0, 0.5, 0.99, 1.0)  # ignored labels, cloud after cloud
WEIGHTS = (None, "random", "frequency")
WORST = {}


def ignore_modes(c):
    """inside the class range, outside it, none"""
    return (c // 2, c + 7, None)


def dev():
    return torch.device("cuda", 0)


def _lib():
    from lattice_net_amd import _lib
    return _lib, _lib.load()


def note(what, ratios):
    w = WORST.setdefault(what, {})
    for k, v in ratios.items():
        w[k] = max(w.get(k, 0.0), v)
    print(f"\n[nll clouds gpu] {what}: worst error/bound " + " ".join(f"{k} {v:.3f}" for k, v in w.items()))


@functools.lru_cache(maxsize=None)
def case(n, n0, c, variant, poison=True):
    """(lp, labels, ignore_index, weight, fp64 reference at grad_loss -0.37): computed once per case, shared, never written to.  With
    `poison`, NaN / -inf stand in every log-probability and every class weight the kernels must not read."""
    ignore = ignore_modes(c)[variant % 3]
    kind = WEIGHTS[(variant // 3) % 3]
    y = R.labels_case(n, n0, c, ignore, SHARES, 3 * n + c + variant)
    lp = R.log_probs_case(n, c, 31 * n + c + variant)
    w = R.weights_case(kind, c, n + variant, y, ignore)
    if poison:
        lp, w = R.poisoned(lp, y, ignore, w)
    ref = R.reference(lp, y, n0, ignore, w, grad_loss=GRAD_LOSS)
    for a in (lp, y, w) + tuple(ref.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return lp, y, ignore, w, ref


GRAD_LOSS = float(np.float32(-0.37))


def guarded(shape, fill):
    t = torch.full((int(np.prod(shape)) + GUARD,), fill, dtype=torch.float32, device=dev())
    t[-GUARD:] = 7.0
    return t


def run(lp, y, n0, ignore, weight=None, grad_loss=GRAD_LOSS, backward=True):
    """ln_nll_forward_clouds + ln_nll_backward_clouds through the C ABI.  Every output starts as NaN and carries guard words behind it,
    as does the workspace: the calls overwrite the former completely and leave the latter alone.  Returns the outputs as NumPy."""
    L, lib = _lib()
    n, c = lp.shape
    clouds = len(R.cloud_ranges(n, n0))
    x = torch.from_numpy(np.array(lp)).to(dev())
    t = torch.from_numpy(np.array(y, dtype=np.int64)).to(dev())
    w = None if weight is None else torch.from_numpy(np.array(weight, dtype=np.float32)).to(dev())
    need = lib.ln_nll_clouds_workspace_bytes(n, n0)
    ws = torch.full((need + 4 * GUARD,), 0xA5, dtype=torch.uint8, device=dev())
    nan = float("nan")
    loss, pcl, wsum, grad = guarded((1,), nan), guarded((clouds,), nan), guarded((clouds,), nan), guarded((n, c), nan)
    g = torch.tensor([grad_loss], dtype=torch.float32, device=dev())
    sp = L.stream_ptr(dev())
    ign = NO_LABEL if ignore is None else ignore
    L.check(lib.ln_nll_forward_clouds(L.ptr(x), L.ptr(t), n, n0, c, ign, L.ptr(w), L.ptr(ws), need, L.ptr(loss), L.ptr(pcl), L.ptr(wsum), sp),
            "ln_nll_forward_clouds")
    if backward:
        L.check(lib.ln_nll_backward_clouds(L.ptr(t), L.ptr(g), L.ptr(wsum), n, n0, c, ign, L.ptr(w), L.ptr(grad), sp), "ln_nll_backward_clouds")
    torch.cuda.synchronize()
    for a in (loss, pcl, wsum, grad):
        assert bool((a[-GUARD:] == 7.0).all()), "guard words overwritten"
    assert bool((ws[need:] == 0xA5).all()), "guard bytes behind the workspace overwritten"
    out = dict(loss=loss[:1].cpu().numpy()[0], per_cloud=pcl[:-GUARD].cpu().numpy(), weight_sum=wsum[:-GUARD].cpu().numpy())
    if backward:
        out["grad"] = grad[:-GUARD].view(n, c).cpu().numpy()
    for k, v in out.items():
        assert not np.isnan(v).any(), f"{k}: an element was not written, or a value that must not be read reached it"
    return out


def run_single(lp, y, ignore, grad_loss=GRAD_LOSS):
    """The existing ln_nll_forward + ln_nll_backward on one cloud: (loss_count [2], grad [n, C])."""
    L, lib = _lib()
    n, c = lp.shape
    x = torch.from_numpy(np.array(lp)).to(dev())
    t = torch.from_numpy(np.array(y, dtype=np.int64)).to(dev())
    ws = torch.empty((lib.ln_nll_workspace_bytes(),), dtype=torch.uint8, device=dev())
    lc = torch.empty((2,), device=dev())
    grad = torch.empty((n, c), device=dev())
    g = torch.tensor([grad_loss], dtype=torch.float32, device=dev())
    sp = L.stream_ptr(dev())
    ign = NO_LABEL if ignore is None else ignore
    L.check(lib.ln_nll_forward(L.ptr(x), L.ptr(t), n, c, ign, L.ptr(ws), ws.numel(), L.ptr(lc), sp), "ln_nll_forward")
    L.check(lib.ln_nll_backward(L.ptr(t), L.ptr(g), L.ptr(lc), n, c, ign, L.ptr(grad), sp), "ln_nll_backward")
    torch.cuda.synchronize()
    return lc.cpu().numpy(), grad.cpu().numpy()


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def check_case(n, n0, c, variant, what, slices=True):
    """One batch against fp64, then cloud by cloud bit for bit: the same entry point on the slice, and without weights ln_nll_forward /
    ln_nll_backward on the slice (the gradient times 1 / B when B is a power of two)."""
    lp, y, ignore, w, ref = case(n, n0, c, variant)
    got = run(lp, y, n0, ignore, w)
    note(what, R.check(got, lp, y, n0, ignore, w, f"n={n} n0={n0} C={c} variant {variant}", grad_loss=GRAD_LOSS, ref=ref))
    ranges = R.cloud_ranges(n, n0)
    nb = len(ranges)
    assert got["per_cloud"].shape == (nb,)
    for b in range(nb):
        lo, hi = ranges[b]
        if not (y[lo:hi] != (NO_LABEL if ignore is None else ignore)).any():  # all ignored: 0, the divisor 1, no gradient
            assert got["per_cloud"][b] == 0.0 and got["weight_sum"][b] == 1.0 and not got["grad"][lo:hi].any()
    for b in sorted({0, 1 % nb, nb - 1}) if slices else ():
        lo, hi = ranges[b]
        one = run(lp[lo:hi], y[lo:hi], hi - lo, ignore, w)
        assert same_bits(got["per_cloud"][b], one["per_cloud"][0]) and same_bits(got["weight_sum"][b], one["weight_sum"][0]), (what, n, n0, c, b)
        if w is None:
            lc, grad = run_single(lp[lo:hi], y[lo:hi], ignore)
            assert same_bits(got["per_cloud"][b], lc[0]) and same_bits(got["weight_sum"][b], lc[1]), (what, n, n0, c, b, "ln_nll_forward")
            if nb & (nb - 1) == 0:
                assert same_bits(got["grad"][lo:hi], grad * np.float32(1.0 / nb)), (what, n, n0, c, b, "ln_nll_backward")
    return got


@pytest.mark.parametrize("c", CLASSES)
def test_every_form_against_fp64_and_cloud_by_cloud_bit_for_bit(c):
    k = 0
    for n0 in POINTS_PER_CLOUD:
        for nb in CLOUDS:
            # every second batch of more than one cloud ends in a cloud of one row
            n = n0 * nb if (nb == 1 or n0 == 1 or k % 2) else n0 * (nb - 1) + 1
            check_case(n, n0, c, k, "every form", slices=(nb < 64 or n0 in (1, 64, 65, 1025)))
            k += 1
    assert k >= 9  # every (ignore_index, weights) pair was used


def test_wide_rows_one_cloud_and_the_three_launch_form():
    check_case(65 * 3, 65, 1024, 4, "C = 1024")
    check_case(300, 1 << 40, 20, 3, "points_per_cloud >= n")  # one cloud
    check_case(300, 300, 20, 5, "points_per_cloud >= n")
    # more than LN_NLLC_FUSED_CLOUDS clouds of more than 1024 rows: the per-cloud finish on a grid, the mean in a launch of its own
    assert R.LN_NLLC_FUSED_CLOUDS == 64
    check_case(1025 * 64 + 1, 1025, 3, 0, "65 clouds of 1025 rows")
    check_case(1025 * 64 + 1, 1025, 3, 4, "65 clouds of 1025 rows")


def test_one_long_cloud_past_the_grid_cap():
    n, c = 524288 + 1027, 2  # 512 workgroups, a full further trip of the grid-stride loop and a ragged one
    assert R.nll_blocks(n) == R.LN_NLL_BLOCKS and R.depth(n) == 5 + 23
    check_case(n, n, c, 2, "past the grid cap")        # no weights, no ignore_index: bitwise ln_nll_forward
    check_case(n, n, c, 3, "past the grid cap")        # random weights
    check_case(n + 100, n, c, 6, "past the grid cap")  # two clouds: the long one and a short one


def test_65535_clouds_of_one_point():
    n, c = R.MAX_CLOUDS, 3
    got = check_case(n, 1, c, 3, "65535 clouds", slices=False)
    lp, y, ignore, w, ref = case(n, 1, c, 3)
    counted = y != ignore
    assert 0 < counted.sum() < n and (got["weight_sum"][~counted] == 1.0).all() and not got["grad"][~counted].any()
    assert same_bits(got["weight_sum"][counted], w[np.clip(y[counted], 0, c - 1)])  # one label: its weight
    wc, lpc = w[np.clip(y[counted], 0, c - 1)], lp[counted, np.clip(y[counted], 0, c - 1)]
    assert same_bits(got["per_cloud"][counted], -(wc * lpc) / wc)  # (fp32 NumPy: the product, the division)


def test_zero_weight_class_as_the_only_label_of_a_cloud():
    n0, c = 65, 4
    lp = np.array(R.log_probs_case(3 * n0, c, 5))
    y = np.random.default_rng(6).integers(0, c, 3 * n0).astype(np.int64)
    y[n0:2 * n0] = 2
    w = np.array([0.5, 2.0, 0.0, 3.0], dtype=np.float32)
    got = run(lp, y, n0, None, w)
    note("zero weight", R.check(got, lp, y, n0, None, w, "zero weight", grad_loss=GRAD_LOSS))
    assert got["per_cloud"][1] == 0.0 and got["weight_sum"][1] == 1.0 and not got["grad"][n0:2 * n0].any()
    assert got["per_cloud"][0] > 0 and got["per_cloud"][2] > 0


def test_integer_inputs_and_power_of_two_weights_bit_for_bit():
    for n, n0, c, weighted in ((1000, 300, 3, True), (1000, 300, 20, False), (2100, 1025, 5, True), (640, 64, 3, True), (257, 1, 2, True),
                               (524288 + 1027, 524288 + 1027, 2, True)):
        lp, y, w, g = R.exact_case(n, n0, c, weighted)
        got, want = run(lp, y, n0, -100, w, grad_loss=g), R.emulate(lp, y, n0, -100, w, g)
        for k in R.OUTPUTS:
            assert same_bits(got[k], want[k]), (n, n0, c, weighted, k)
        note("exact", R.check(got, lp, y, n0, -100, w, "exact", grad_loss=g))


def test_another_clouds_inputs_leave_a_clouds_gradient_unchanged():
    n, n0, c, moved = 1000, 300, 20, 1
    lp, y, ignore, w, _ = case(n, n0, c, 4, poison=False)
    base = run(lp, y, n0, ignore, w)
    lo, hi = R.cloud_ranges(n, n0)[moved]
    rows = np.r_[0:lo, hi:n]
    others = [b for b in range(4) if b != moved]
    lp2 = np.array(lp)
    lp2[lo:hi] *= np.float32(2.0)
    y2 = np.array(y)
    y2[lo:hi] = np.where(y[lo:hi] == ignore, 0, ignore)  # what counted is ignored now and the other way round
    for lpx, yx, what in ((lp2, y, "scaled"), (lp, y2, "labels")):
        got = run(lpx, yx, n0, ignore, w)
        for key in ("per_cloud", "weight_sum"):
            assert same_bits(got[key][others], base[key][others]), (what, key)
        assert not same_bits(got["per_cloud"][moved], base["per_cloud"][moved]), what
        assert same_bits(got["grad"][rows], base["grad"][rows]), what
        assert not same_bits(got["loss"], base["loss"]), what
    assert not same_bits(got["grad"][lo:hi], base["grad"][lo:hi]) and not same_bits(got["weight_sum"][moved], base["weight_sum"][moved])


def test_two_runs_are_bitwise_equal():
    for n, n0, c, v in ((1000, 300, 20, 4), (64 * 63, 63, 3, 3), (1025 * 3 + 1, 1025, 20, 5)):
        lp, y, ignore, w, _ = case(n, n0, c, v)
        a, b = run(lp, y, n0, ignore, w), run(lp, y, n0, ignore, w)
        assert all(same_bits(a[k], b[k]) for k in R.OUTPUTS), (n, n0, c)


@pytest.fixture
def fused(monkeypatch):
    """NLLLoss / nll_loss_gather(weight=, points_per_cloud=) take the kernels whatever the module's default is."""
    from lattice_net_amd import losses
    monkeypatch.setattr(losses, "FUSED_NLL_CLOUDS", True)
    return losses


def test_module_takes_the_kernels_and_matches_the_c_abi(fused):
    for n, n0, c, v in ((1000, 300, 20, 4), (1000, 300, 20, 0), (640, 64, 3, 5), (2100, 1025, 20, 3)):
        lp, y, ignore, w, _ = case(n, n0, c, v)
        abi = run(lp, y, n0, ignore, w, grad_loss=1.0)
        x = torch.from_numpy(np.array(lp)).to(dev()).requires_grad_(True)
        wt = None if w is None else torch.from_numpy(np.array(w))
        loss = fused.NLLLoss(weight=wt, ignore_index=ignore, points_per_cloud=n0).to(dev())(x, torch.from_numpy(np.array(y)).to(dev()))
        assert type(loss.grad_fn).__name__ == "_NllCloudsFunctionBackward"
        loss.backward()
        assert same_bits(loss.detach().cpu().numpy(), abi["loss"]) and same_bits(x.grad.cpu().numpy(), abi["grad"]), (n, n0, c, v)
        one = fused.nll_loss_gather(x.detach()[:n0], torch.from_numpy(np.array(y[:n0])).to(dev()), ignore, weight=wt)  # weight alone: one cloud
        assert same_bits(one.cpu().numpy(), abi["per_cloud"][0])
    # float64 on the device: the torch form
    x64 = torch.from_numpy(np.array(lp)).double().to(dev())
    got = fused.NLLLoss(weight=wt, ignore_index=ignore, points_per_cloud=n0)(x64, torch.from_numpy(np.array(y)).to(dev()))
    assert got.dtype == torch.float64 and abs(got.item() - R.reference(lp, y, n0, ignore, w)["loss"]) < 1e-12


def test_default_path_is_unchanged(fused):
    """Neither weight nor points_per_cloud: _NllFunction, bitwise the loss_count and the gradient of ln_nll_forward / ln_nll_backward."""
    assert fused.FUSED_NLL
    for n, c, v in ((1000, 20, 0), (1025, 3, 1), (300, 20, 2)):
        lp, y, ignore, _, _ = case(n, n, c, v, poison=False)
        lc, grad = run_single(lp, y, ignore, grad_loss=1.0)
        for call in (lambda x, t: fused.nll_loss_gather(x, t, ignore), lambda x, t: fused.NLLLoss(ignore_index=ignore)(x, t)):
            x = torch.from_numpy(np.array(lp)).to(dev()).requires_grad_(True)
            loss = call(x, torch.from_numpy(np.array(y)).to(dev()))
            assert type(loss.grad_fn).__name__ == "_NllFunctionBackward"
            loss.backward()
            assert same_bits(loss.detach().cpu().numpy(), lc[0]) and same_bits(x.grad.cpu().numpy(), grad)


def test_batched_loss_is_the_mean_of_the_clouds_losses_not_the_batch_mean(fused):
    lp, y, n0, ignore = R.skewed_case()
    n = len(y)
    x, t = torch.from_numpy(lp).to(dev()), torch.from_numpy(y).to(dev())
    batched = fused.NLLLoss(ignore_index=ignore, points_per_cloud=n0)(x, t).item()
    ranges = R.cloud_ranges(n, n0)
    singles = [fused.NLLLoss(ignore_index=ignore, points_per_cloud=hi - lo)(x[lo:hi], t[lo:hi]).item() for lo, hi in ranges]
    gather = [fused.nll_loss_gather(x[lo:hi], t[lo:hi], ignore).item() for lo, hi in ranges]
    assert singles == gather  # the single-cloud loss of the training step
    ref = R.reference(lp, y, n0, ignore)
    bnd = R.bounds(ref, n, n0, False)
    mean = float(np.mean(np.array(singles, dtype=np.float64)))
    print(f"\n[nll clouds gpu] skewed batch: per-cloud mean {batched!r}, mean of the single-cloud losses {mean!r}, fp64 {ref['loss']!r}, bound "
          f"{bnd['loss']:.3e}")
    assert abs(batched - ref["loss"]) <= bnd["loss"] and abs(mean - ref["loss"]) <= float(np.mean(bnd["per_cloud"]))
    assert abs(batched - mean) <= bnd["loss"] + float(np.mean(bnd["per_cloud"]))
    whole = fused.nll_loss_gather(x, t, ignore).item()
    assert abs(whole - batched) > 1e-3 * abs(batched), (whole, batched)


def test_captured_forward_and_backward_replay_bitwise(fused):
    n, n0, c = 1000, 300, 20
    inputs = [case(n, n0, c, 4 + 9 * s) for s in (0, 1, 2)]  # the same (ignore_index, weights) pair, other seeds
    ignore = inputs[0][2]
    loss_fn = fused.NLLLoss(weight=torch.from_numpy(np.array(inputs[0][3])), ignore_index=ignore, points_per_cloud=n0).to(dev())
    x = torch.from_numpy(np.array(inputs[0][0])).to(dev()).requires_grad_(True)
    t = torch.from_numpy(np.array(inputs[0][1])).to(dev())
    st = {}

    def step(xx, tt):
        loss = loss_fn(xx, tt)
        grad, = torch.autograd.grad(loss, xx)
        return loss.detach(), grad

    eager = []
    for lp, y, _, w, _ in inputs:
        loss_fn.weight.copy_(torch.from_numpy(np.array(w)))
        eager.append(step(torch.from_numpy(np.array(lp)).to(dev()).requires_grad_(True), torch.from_numpy(np.array(y)).to(dev())))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(x, t)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st["loss"], st["grad"] = step(x, t)
    for k in (1, 2, 2):
        with torch.no_grad():
            x.copy_(torch.from_numpy(np.array(inputs[k][0])))
        t.copy_(torch.from_numpy(np.array(inputs[k][1])))
        loss_fn.weight.copy_(torch.from_numpy(np.array(inputs[k][3])))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(st["loss"], eager[k][0]) and torch.equal(st["grad"], eager[k][1]), k
    assert not torch.equal(eager[1][1], eager[2][1])


def _launches(call):
    _, lib = _lib()
    assert lib.ln_profile_begin(b"*", 64) == 0
    rc = call()
    ms, count = C.c_double(), C.c_int()
    assert lib.ln_profile_end(C.byref(ms), C.byref(count)) == 0
    return rc, count.value


def test_refusals_launch_nothing_and_write_nothing():
    L, lib = _lib()
    n, n0, c = 130, 65, 3
    x = torch.zeros((n, c), device=dev())
    t = torch.zeros((n,), dtype=torch.int64, device=dev())
    need = lib.ln_nll_clouds_workspace_bytes(2100, 1025)
    assert need > lib.ln_nll_clouds_workspace_bytes(n, n0) >= 256 and lib.ln_nll_clouds_workspace_bytes(-5, 0) >= 256
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=dev())
    outs = [torch.full(s, 7.0, device=dev()) for s in ((1,), (3,), (3,), (2100, c))]
    loss, pcl, wsum, grad = outs
    big = torch.zeros((2100, c), device=dev())
    bigt = torch.zeros((2100,), dtype=torch.int64, device=dev())
    g = torch.ones((1,), device=dev())
    sp = L.stream_ptr(dev())

    def fwd(nn, pp, cc, ws_bytes, xx=x, tt=t, out=loss, pc=pcl, wsm=wsum, wsp=ws):
        return lambda: lib.ln_nll_forward_clouds(L.ptr(xx), L.ptr(tt), nn, pp, cc, 0, None, L.ptr(wsp), ws_bytes, L.ptr(out), L.ptr(pc), L.ptr(wsm), sp)

    def bwd(nn, pp, cc, tt=t, gg=g, wsm=wsum, out=grad):
        return lambda: lib.ln_nll_backward_clouds(L.ptr(tt), L.ptr(gg), L.ptr(wsm), nn, pp, cc, 0, None, L.ptr(out), sp)

    E, U = R.LN_ERR_ARG, R.LN_ERR_UNSUPPORTED
    for call, rc_want, text in ((fwd(2100, 1025, c, need - 1, big, bigt), E, b"workspace"), (fwd(n, n0, 0, need), E, b"bad sizes"),
                                (fwd(-1, n0, c, need), E, b"bad sizes"), (fwd(n, 0, c, need), E, b"points_per_cloud"),
                                (fwd(R.MAX_CLOUDS + 1, 1, 2, need), U, b"at most 65535"), (fwd(2 * R.MAX_CLOUDS + 1, 2, 2, need), U, b"at most 65535"),
                                (fwd((1 << 31) // c + 1, n0, c, need), U, b"2^31"), (fwd(n, n0, c, need, xx=None), E, b"null"),
                                (fwd(n, n0, c, need, tt=None), E, b"null"), (fwd(n, n0, c, need, out=None), E, b"null"),
                                (fwd(n, n0, c, need, pc=None), E, b"null"), (fwd(n, n0, c, need, wsm=None), E, b"null"),
                                (fwd(n, n0, c, need, wsp=None), E, b"null"),
                                (bwd(n, n0, 0), E, b"bad sizes"), (bwd(-1, n0, c), E, b"bad sizes"), (bwd(n, 0, c), E, b"points_per_cloud"),
                                (bwd(R.MAX_CLOUDS + 1, 1, 2), U, b"at most 65535"), (bwd((1 << 31) // c + 1, n0, c), U, b"2^31"),
                                (bwd(n, n0, c, tt=None), E, b"null"), (bwd(n, n0, c, gg=None), E, b"null"), (bwd(n, n0, c, wsm=None), E, b"null"),
                                (bwd(n, n0, c, out=None), E, b"null")):
        rc, launches = _launches(call)
        assert rc == rc_want and launches == 0 and text in lib.ln_last_error_string(), (rc, launches, lib.ln_last_error_string())
    torch.cuda.synchronize()
    assert all(bool((a == 7.0).all()) for a in outs) and bool((ws == 0xA5).all())
    rc, launches = _launches(fwd(n, n0, c, need))  # one workgroup per cloud and the mean
    assert rc == 0 and launches == 2
    rc, launches = _launches(fwd(2100, 1025, c, need, big, bigt))  # partials, and one finishing workgroup
    assert rc == 0 and launches == 2
    rc, launches = _launches(bwd(n, n0, c))
    assert rc == 0 and launches == 1
    rc, launches = _launches(bwd(0, n0, c))  # no points: nothing to write
    assert rc == 0 and launches == 0
    loss.fill_(7.0)
    rc, launches = _launches(fwd(0, n0, c, need))  # no points, no cloud: the loss is 0
    torch.cuda.synchronize()
    assert rc == 0 and launches == 0 and float(loss[0]) == 0.0
    names = set(lib.ln_kernel_names().decode().split(","))
    assert {"k_nll_clouds_wave", "k_nll_clouds_partials", "k_nll_clouds_finish", "k_nll_clouds_backward"} <= names
