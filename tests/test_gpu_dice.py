"""The generalized soft Dice loss as HIP kernels (ln_dice_forward / ln_dice_backward, csrc/ln_dice.hip), one cloud and per cloud, against
the fp64 reference and the counted bounds of tests/dice_reference.py: every output element by element, exact runs, cloud by cloud bit
for bit, reproducibility (also under graph replay), guard words and refusals, and through losses.GeneralizedSoftDiceLoss."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from . import dice_reference as R

pytestmark = pytest.mark.gpu

NO_LABEL = -(1 << 62)
GUARD = 64  # guard words behind every buffer
NS = (1, 63, 64, 65, 255, 256, 257, 1000)
CLASSES = (1, 2, 19, 20, 32, 33, 64, 255, 256, 257, 1024)  # 255, 256, 257: both lane mappings and the boundary between them
# (family of log-probabilities, kind of labels, ignore_index as a function of C)
VARIANTS = (("softmax", "random", lambda c: None), ("softmax", "wild", lambda c: 0), ("onehot", "absent", lambda c: c + 3),
            ("softmax", "one", lambda c: c - 1), ("onehot", "wild", lambda c: None), ("softmax", "absent", lambda c: 0))
# one shape just past the tile cap of k_dice_partials per lane mapping: LN_DICE_MAX_TILES tiles of LN_DICE_STEPS steps no longer cover
# the cloud and the tiles grow (dice_reference.rows_past_the_tile_cap: 256 / C * 16 * 512 + 1 rows, 16 * 512 + 1 for C > 256)
PAST_THE_CAP = ((R.rows_past_the_tile_cap(64), 64), (R.rows_past_the_tile_cap(257), 257))
# (n, n0): n0 = 1, 7 and 300 with a shorter last cloud where n0 allows one, one cloud, n0 > n, 64 clouds of 1 - 9 points
CLOUD_SHAPES = ((13, 1), (1000, 7), (1000, 300), (257, 257), (257, 1 << 40), (64, 1), (63 * 5 + 2, 5), (63 * 9 + 1, 9))
CLOUD_CLASSES = (1, 20, 33, 256, 257)
WORST = {}


def dev():
    return torch.device("cuda", 0)


def _lib():
    from lattice_net_amd import _lib
    return _lib, _lib.load()


def note(what, ratios):
    w = WORST.setdefault(what, {})
    for k, v in ratios.items():
        w[k] = max(w.get(k, 0.0), v)
    print(f"\n[dice gpu] {what}: worst error/bound " + " ".join(f"{k} {v:.3f}" for k, v in w.items()))


@functools.lru_cache(maxsize=None)
def case(n, c, n0, variant, seed=0):
    """(logp, labels, ignore_index, fp64 reference): computed once per case, shared, never written to."""
    family, kind, ign = VARIANTS[variant]
    lp, y, ignore = R.inputs(n, c, 31 * n + c + seed, family), R.labels(n, c, n + seed, kind), ign(c)
    ref = R.reference(lp, y, n0, ignore)
    for a in (lp, y) + tuple(v for v in ref.values() if isinstance(v, np.ndarray)):
        a.setflags(write=False)
    return lp, y, ignore, ref


def guarded(shape, fill):
    """A flat buffer of prod(shape) elements `fill` with GUARD words of 7 behind it."""
    t = torch.full((int(np.prod(shape)) + GUARD,), fill, dtype=torch.float32, device=dev())
    t[-GUARD:] = 7.0
    return t


def run(lp, y, n0, ignore, grad_loss=1.0, optional=True):
    """ln_dice_forward + ln_dice_backward through the C ABI.  Every output starts as NaN and carries guard words behind it, as does the
    workspace: the calls have to overwrite the former completely and leave the latter alone.  Returns the outputs as NumPy."""
    L, lib = _lib()
    n, c = lp.shape
    pp = n if n0 is None else n0
    clouds = len(R.cloud_ranges(n, pp))
    x = torch.from_numpy(np.array(lp)).to(dev())
    t = torch.from_numpy(np.array(y, dtype=np.int64)).to(dev())
    need = lib.ln_dice_workspace_bytes(n, pp, c)
    ws = torch.full((need + 4 * GUARD,), 0xA5, dtype=torch.uint8, device=dev())
    nan = float("nan")
    loss, pcl, st, coef, grad = guarded((1,), nan), guarded((clouds,), nan), guarded((clouds, 3, c), nan), guarded((clouds, 2, c), nan), \
        guarded((n, c), nan)
    g = torch.tensor([grad_loss], dtype=torch.float32, device=dev())
    sp = L.stream_ptr(dev())
    L.check(lib.ln_dice_forward(L.ptr(x), L.ptr(t), n, pp, c, NO_LABEL if ignore is None else ignore, L.ptr(ws), need, L.ptr(loss),
                                L.ptr(pcl) if optional else None, L.ptr(st) if optional else None, L.ptr(coef), sp), "ln_dice_forward")
    L.check(lib.ln_dice_backward(L.ptr(x), L.ptr(t), L.ptr(coef), L.ptr(g), n, pp, c, L.ptr(grad), sp), "ln_dice_backward")
    torch.cuda.synchronize()
    for a in (loss, pcl, st, coef, grad):
        assert bool((a[-GUARD:] == 7.0).all()), "guard words overwritten"
    assert bool((ws[need:] == 0xA5).all()), "guard bytes behind the workspace overwritten"
    out = dict(loss=loss[:1].cpu().numpy()[0], coef=coef[:-GUARD].view(clouds, 2, c).cpu().numpy(), grad=grad[:-GUARD].view(n, c).cpu().numpy())
    if optional:
        out.update(per_cloud=pcl[:-GUARD].cpu().numpy(), stats=st[:-GUARD].view(clouds, 3, c).cpu().numpy())
    else:
        assert bool(torch.isnan(pcl[:-GUARD]).all()) and bool(torch.isnan(st[:-GUARD]).all())
    for k, v in out.items():
        assert not np.isnan(v).any(), f"{k}: an element was not written"
    return out


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("c", CLASSES)
def test_one_cloud_against_fp64_element_by_element(c):
    scale = float(np.float32(-0.37))
    for k, n in enumerate(NS):
        for j in range(3):  # three of the six variants per n, every variant four times per C
            v = (k + 2 * j) % len(VARIANTS)
            lp, y, ignore, ref = case(n, c, None, v)
            got = run(lp, y, None, ignore, grad_loss=scale, optional=(j != 2))
            note("one cloud", R.check(got, lp, y, None, ignore, f"n={n} C={c} variant {v}", grad_loss=scale, ref=ref))
            if "stats" in got:
                assert same_bits(got["stats"][0, 2], ref["stats"][0, 2].astype(np.float32)), "G is exact"
            assert np.array_equal(got["coef"] == 0, ref["coef"] == 0)  # the ignore class, and only it, has a = b = 0 (b = 0 also where I = 0)


@pytest.mark.parametrize("n,c", PAST_THE_CAP)
def test_past_the_tile_cap_against_fp64(n, c):
    assert R.tiling(n - 1, c)[1] == R.tiling(1, c)[0] * R.LN_DICE_STEPS < R.tiling(n, c)[1] and R.tiling(n - 1, c)[2] == R.LN_DICE_MAX_TILES
    lp, y, ignore, ref = case(n, c, None, 1)
    note("past the tile cap", R.check(run(lp, y, None, ignore), lp, y, None, ignore, f"n={n} C={c}", ref=ref))
    n0 = n  # two clouds: one past the cap, a short one that is cut as a cloud of its own length
    lp, y, ignore, ref = case(n + 100, c, n0, 0)
    got = run(lp, y, n0, ignore)
    note("past the tile cap", R.check(got, lp, y, n0, ignore, f"n={n + 100} n0={n0} C={c}", ref=ref))
    one = run(lp[n0:], y[n0:], None, ignore)
    assert same_bits(got["per_cloud"][1], one["per_cloud"][0]) and same_bits(got["stats"][1], one["stats"][0])


@pytest.mark.parametrize("c", CLOUD_CLASSES)
def test_per_cloud_against_fp64_and_cloud_by_cloud_bit_for_bit(c):
    for k, (n, n0) in enumerate(CLOUD_SHAPES):
        v = k % len(VARIANTS)
        lp, y, ignore, ref = case(n, c, n0, v)
        got = run(lp, y, n0, ignore)
        note("per cloud", R.check(got, lp, y, n0, ignore, f"n={n} n0={n0} C={c} variant {v}", ref=ref))
        ranges = R.cloud_ranges(n, n0)
        nb = len(ranges)
        assert got["per_cloud"].shape == (nb,)
        for b in sorted({0, 1 % nb, nb // 2, nb - 1}):
            lo, hi = ranges[b]
            one = run(lp[lo:hi], y[lo:hi], None, ignore)
            assert same_bits(got["per_cloud"][b], one["per_cloud"][0]) and same_bits(got["stats"][b], one["stats"][0]), (n, n0, c, b)
            if nb & (nb - 1) == 0:  # the 1 / B inside a and b is a change of exponent
                assert same_bits(got["grad"][lo:hi], one["grad"] * np.float32(1.0 / nb)), (n, n0, c, b)
            else:
                # a = fl(a_1 / B): 1 rounding; b = fl(fl(a I) / D) against fl(fl(a_1 I) / D) / B: 5; a - b, p t, grad_loss (p t) on
                # either side: 6 — on the magnitude p (a [y = c] + b) of the fp64 reference
                a, bb = ref["coef"][b]
                mag = np.exp(lp[lo:hi].astype(np.float64)) * (a * (y[lo:hi, None] == np.arange(c)[None, :]) + bb)
                diff = np.abs(got["grad"][lo:hi].astype(np.float64) - one["grad"].astype(np.float64) / nb)
                assert (diff <= R.gamma(12) * mag + 4 * R.TINY32).all(), (n, n0, c, b)
        if nb == 1:
            whole = run(lp, y, None, ignore)
            assert all(same_bits(got[key], whole[key]) for key in R.OUTPUTS), "one cloud is the single-cloud call"


def test_scaling_one_cloud_leaves_the_others_unchanged():
    n, n0, c, moved = 1000, 300, 20, 1
    lp, y, ignore, _ = case(n, c, n0, 1)
    base = run(lp, y, n0, ignore)
    lp2 = np.array(lp)
    lo, hi = R.cloud_ranges(n, n0)[moved]
    lp2[lo:hi] = R.log_softmax64(2.0 * lp[lo:hi].astype(np.float64)).astype(np.float32)
    got = run(lp2, y, n0, ignore)
    others = [b for b in range(4) if b != moved]
    rows = np.r_[0:lo, hi:n]
    for key in ("per_cloud", "stats", "coef"):
        assert same_bits(got[key][others], base[key][others]), key
        assert not same_bits(got[key][moved], base[key][moved]), key
    assert same_bits(got["grad"][rows], base["grad"][rows]) and not same_bits(got["grad"][lo:hi], base["grad"][lo:hi])
    assert not same_bits(got["loss"], base["loss"])


def test_exact_runs():
    """log_probs entries 0 or -inf: p is exactly 1 or 0, every sum is a sum of small integers — stats are the integer counts bit for
    bit, and the gradient of a -inf entry is exactly 0, not NaN."""
    for n, c, n0, kind in ((1000, 3, None, "random"), (1000, 20, 300, "wild"), (257, 257, 7, "random"), (65, 1, None, "random")):
        lp, y = R.inputs(n, c, n, "exact"), R.labels(n, c, n, kind)
        got = run(lp, y, n0, 0)
        ref = R.reference(lp, y, n0, 0)
        assert same_bits(got["stats"], ref["stats"].astype(np.float32)), (n, c, n0)
        assert (got["grad"][np.isneginf(lp)] == 0.0).all() and not np.isnan(got["grad"]).any()
        note("exact", R.check(got, lp, y, n0, 0, f"exact n={n} C={c}", ref=ref))


def test_two_runs_are_bitwise_equal():
    for n, c, n0 in ((1000, 20, None), (1000, 33, 7), (PAST_THE_CAP[0][0], 64, None)):
        lp, y, ignore, _ = case(n, c, n0, 1)
        a, b = run(lp, y, n0, ignore, grad_loss=0.5), run(lp, y, n0, ignore, grad_loss=0.5)
        assert all(same_bits(a[k], b[k]) for k in R.OUTPUTS), (n, c, n0)


@pytest.fixture
def fused_dice(monkeypatch):
    """GeneralizedSoftDiceLoss takes the kernels whatever the module's default is."""
    from lattice_net_amd import losses
    monkeypatch.setattr(losses, "FUSED_DICE", True)
    return losses


def test_captured_forward_and_backward_replay_bitwise(fused_dice):
    n0, c = 300, 20
    inputs = [(np.array(case(1000, c, n0, 1, seed=s)[0]), np.array(case(1000, c, n0, 1, seed=s)[1])) for s in (0, 1, 2)]
    dice = fused_dice.GeneralizedSoftDiceLoss(ignore_index=0, points_per_cloud=n0)
    x = torch.from_numpy(inputs[0][0]).to(dev()).requires_grad_(True)
    t = torch.from_numpy(inputs[0][1]).to(dev())
    st = {}

    def step(xx, tt):
        loss = dice(torch.log_softmax(xx, 1), tt)
        grad, = torch.autograd.grad(loss, xx)
        return loss.detach(), grad

    eager = [step(torch.from_numpy(lp).to(dev()).requires_grad_(True), torch.from_numpy(y).to(dev())) for lp, y in inputs]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(x, t)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st["loss"], st["grad"] = step(x, t)
    for k in (1, 2):
        with torch.no_grad():
            x.copy_(torch.from_numpy(inputs[k][0]))
        t.copy_(torch.from_numpy(inputs[k][1]))
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
    need = lib.ln_dice_workspace_bytes(n, n0, c)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=dev())
    outs = [torch.full(s, 7.0, device=dev()) for s in ((1,), (2,), (2, 3, c), (2, 2, c), (n, c))]
    loss, pcl, st, coef, grad = outs
    g = torch.ones((1,), device=dev())
    sp = L.stream_ptr(dev())

    def fwd(nn, pp, cc, ws_bytes):
        return lambda: lib.ln_dice_forward(L.ptr(x), L.ptr(t), nn, pp, cc, 0, L.ptr(ws), ws_bytes, L.ptr(loss), L.ptr(pcl), L.ptr(st),
                                           L.ptr(coef), sp)

    def bwd(nn, pp, cc):
        return lambda: lib.ln_dice_backward(L.ptr(x), L.ptr(t), L.ptr(coef), L.ptr(g), nn, pp, cc, L.ptr(grad), sp)

    for call, text in ((fwd(n, n0, c, need - 1), b"workspace"), (fwd(n, n0, 0, need), b"bad sizes"), (fwd(n, n0, 1025, need), b"bad sizes"),
                       (fwd(n, 0, c, need), b"points_per_cloud"), (fwd(R.MAX_CLOUDS + 1, 1, 2, need), b"at most 65535"),
                       (fwd(2 * R.MAX_CLOUDS + 1, 2, 2, need), b"at most 65535"), (fwd((1 << 31) // c + 1, n0, c, need), b"2^31"),
                       (fwd(-1, n0, c, need), b"bad sizes"), (bwd(n, n0, 0), b"bad sizes"), (bwd(n, n0, 1025), b"bad sizes"),
                       (bwd(n, 0, c), b"points_per_cloud"), (bwd(R.MAX_CLOUDS + 1, 1, 2), b"at most 65535")):
        rc, launches = _launches(call)
        assert rc == -1 and launches == 0 and text in lib.ln_last_error_string(), (rc, launches, lib.ln_last_error_string())
    torch.cuda.synchronize()
    assert all(bool((a == 7.0).all()) for a in outs) and bool((ws == 0xA5).all())
    rc, launches = _launches(fwd(n, n0, c, need))  # the good call: partial sums and the finishing workgroup
    assert rc == 0 and launches == 2
    rc, launches = _launches(bwd(n, n0, c))
    assert rc == 0 and launches == 1
    rc, launches = _launches(bwd(0, n0, c))  # no points: nothing to write
    assert rc == 0 and launches == 0
    loss.fill_(7.0)
    rc, launches = _launches(fwd(0, n0, c, need))  # no points, no cloud: the loss is 0
    torch.cuda.synchronize()
    assert rc == 0 and launches == 0 and float(loss[0]) == 0.0
    names = lib.ln_kernel_names().decode().split(",")
    assert {"k_dice_partials", "k_dice_finish", "k_dice_backward"} <= set(names)


def test_module_matches_f13_with_and_without_points_per_cloud(fused_dice, golden):
    f = golden("F13_losses")
    for name in [str(x) for x in f["case_names"]]:
        lp, labels, ignore = f[f"{name}/logp"].astype(np.float32), f[f"{name}/labels"], int(f[f"{name}/ignore"])
        n = lp.shape[0]
        abi = run(lp, labels, None, ignore)
        ref, g_ref = float(f[f"{name}/dice"]), f[f"{name}/dice_grad"].astype(np.float64)
        for pp in (None, n, n + 5):
            x = torch.from_numpy(lp).to(dev()).requires_grad_(True)
            loss = fused_dice.GeneralizedSoftDiceLoss(ignore_index=ignore, points_per_cloud=pp)(x, torch.from_numpy(labels.astype(np.int64)).to(dev()))
            loss.backward()
            assert same_bits(loss.detach().cpu().numpy(), abi["loss"]), "GeneralizedSoftDiceLoss did not take the kernels"
            assert abs(float(loss) - ref) <= 5e-6 * max(abs(ref), 1.0), (name, pp, float(loss), ref)
            assert np.max(np.abs(x.grad.double().cpu().numpy() - g_ref)) <= 1e-5 * max(np.max(np.abs(g_ref)), 1e-30), (name, pp)


def test_module_autograd_through_log_softmax(fused_dice):
    """d loss / d logits through torch's log_softmax backward, gx = g - exp(lp) sum_c g with g = d loss / d lp from ln_dice_backward.
    The reference evaluates the SAME fp32 log-probabilities in fp64, so only the loss is under test.  Bound: that of g (dice_reference),
    carried through the row sum (at most C - 1 additions in any order: gamma(C) on the sum of magnitudes), torch's exp (2 ulp allowed:
    4 units), the product and the subtraction (one unit each)."""
    scale = float(np.float32(1.7))
    for n, c, n0, v in ((1000, 20, None, 1), (1000, 20, 300, 1), (257, 257, 7, 0), (63 * 9 + 1, 33, 9, 5)):
        logits = np.random.default_rng(n + c).uniform(-6.0, 6.0, (n, c)).astype(np.float32)
        _, y, ignore, _ = case(n, c, n0, v)
        x = torch.from_numpy(logits).to(dev()).requires_grad_(True)
        lp_t = torch.log_softmax(x, 1)
        loss = fused_dice.GeneralizedSoftDiceLoss(ignore_index=ignore, points_per_cloud=n0)(lp_t, torch.from_numpy(np.array(y)).to(dev()))
        (loss * scale).backward()
        lp = lp_t.detach().cpu().numpy()
        ref = R.reference(lp, y, n0, ignore)
        bnd = R.bounds(ref, lp, y, n0, ignore, grad_loss=scale)
        ratios = {"loss": R.worst_ratio(loss.detach().cpu().numpy(), ref["loss"], bnd["loss"])}
        g, e_g, p = ref["grad"] * scale, bnd["grad"], np.exp(lp.astype(np.float64))
        s, e_s = g.sum(1, keepdims=True), e_g.sum(1, keepdims=True) + R.gamma(c) * (np.abs(g) + e_g).sum(1, keepdims=True)
        e_prod = p * e_s + R.gamma(5) * p * (np.abs(s) + e_s)
        bound = e_g + e_prod + R.EPS32 * (np.abs(g) + p * np.abs(s) + e_g + e_prod) + 2 * R.TINY32
        ratios["grad through log_softmax"] = R.worst_ratio(x.grad.cpu().numpy(), g - p * s, bound)
        note("module", ratios)
        assert max(ratios.values()) <= 1.0, (n, c, n0, ratios)
    x64 = torch.from_numpy(lp).double().to(dev())  # float64: the torch form
    got = fused_dice.GeneralizedSoftDiceLoss(ignore_index=0, points_per_cloud=n0)(x64, torch.from_numpy(np.array(y).clip(0, c - 1)).to(dev()))
    assert abs(got.item() - R.reference(lp, np.array(y).clip(0, c - 1), n0, 0)["loss"]) < 1e-12
