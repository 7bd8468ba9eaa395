"""The per-cloud losses over clouds of UNEQUAL sizes (the _ranges entry points of csrc/ln_nll.hip, ln_dice.hip,
ln_lovasz.hip) through the C ABI: every cloud bit for bit against the existing one-cloud call on its rows, loss and gradient
against the fp64 per-slice references and their counted bounds, equal lengths bit for bit against the equal-size entry points,
independence of the clouds, reproducibility (also under graph replay), guard words, refusals."""
import functools

import numpy as np
import pytest
import torch

from . import dice_reference as D
from . import lovasz_clouds_reference as LC
from . import lovasz_reference as LV
from . import nll_clouds_reference as N

pytestmark = pytest.mark.gpu

NO_LABEL = N.NO_LABEL
GUARD = 64
GRAD_LOSS = float(np.float32(-0.37))
NAN = float("nan")


def dev():
    return torch.device("cuda", 0)


def _lib():
    from lattice_net_amd import _lib
    return _lib, _lib.load()


def slices(lengths):
    s = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return [(int(a), int(b)) for a, b in zip(s[:-1], s[1:])]


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def guarded(count, fill=NAN, dtype=torch.float32):
    t = torch.full((int(count) + GUARD,), fill, dtype=dtype, device=dev())
    t[int(count):] = 7
    return t


def to_dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.array(a, dtype=dtype)).to(dev())


def starts_of(lengths):
    return torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32, device=dev())


class Call:
    """One family's forward (+ backward) through the C ABI on guarded, NaN-filled outputs: `launch()` queues the calls on the current
    stream, `read()` checks the guard words and returns the outputs as NumPy."""

    def __init__(self, outputs, workspace_bytes):
        self.out = {k: (guarded(int(np.prod(shape))), shape) for k, shape in outputs.items()}
        self.need = workspace_bytes
        self.ws = torch.full((workspace_bytes + 4 * GUARD,), 0xA5, dtype=torch.uint8, device=dev())
        self.g = torch.tensor([GRAD_LOSS], dtype=torch.float32, device=dev())

    def p(self, k):
        L, _ = _lib()
        return L.ptr(self.out[k][0])

    def read(self, written=True):
        torch.cuda.synchronize()
        assert bool((self.ws[self.need:] == 0xA5).all()), "guard bytes behind the workspace overwritten"
        res = {}
        for k, (t, shape) in self.out.items():
            n = int(np.prod(shape))
            assert bool((t[n:] == 7).all()), f"{k}: guard words overwritten"
            res[k] = t[:n].cpu().numpy().reshape(shape)
        return res


# ---------------------------------------------------------------------------------------------------------------------------- NLL
def nll_call(lp, y, cut, ignore, w):
    """cut: a list of lengths (ln_nll_forward_ranges) or an int (ln_nll_forward_clouds)."""
    L, lib = _lib()
    n, c = lp.shape
    ranged = not isinstance(cut, int)
    B = len(cut) if ranged else len(N.cloud_ranges(n, cut))
    x, t, wd = to_dev(lp), to_dev(y, np.int64), to_dev(w, np.float32)
    ign = NO_LABEL if ignore is None else ignore
    if ranged:
        st, longest = starts_of(cut), int(max(cut))
        call = Call(dict(loss=(1,), per_cloud=(B,), weight_sum=(B,), grad=(n, c)), lib.ln_nll_ranges_workspace_bytes(n, B, longest))
    else:
        call = Call(dict(loss=(1,), per_cloud=(B,), weight_sum=(B,), grad=(n, c)), lib.ln_nll_clouds_workspace_bytes(n, cut))

    def launch():
        sp = L.stream_ptr(dev())
        if ranged:
            L.check(lib.ln_nll_forward_ranges(L.ptr(x), L.ptr(t), n, L.ptr(st), B, longest, c, ign, L.ptr(wd), L.ptr(call.ws), call.need,
                                              call.p("loss"), call.p("per_cloud"), call.p("weight_sum"), sp), "ln_nll_forward_ranges")
            L.check(lib.ln_nll_backward_ranges(L.ptr(t), L.ptr(call.g), call.p("weight_sum"), n, L.ptr(st), B, longest, c, ign, L.ptr(wd),
                                               call.p("grad"), sp), "ln_nll_backward_ranges")
        else:
            L.check(lib.ln_nll_forward_clouds(L.ptr(x), L.ptr(t), n, cut, c, ign, L.ptr(wd), L.ptr(call.ws), call.need, call.p("loss"),
                                              call.p("per_cloud"), call.p("weight_sum"), sp), "ln_nll_forward_clouds")
            L.check(lib.ln_nll_backward_clouds(L.ptr(t), L.ptr(call.g), call.p("weight_sum"), n, cut, c, ign, L.ptr(wd), call.p("grad"), sp),
                    "ln_nll_backward_clouds")
    call.launch = launch
    call.keep = (x, t, wd, st if ranged else None)
    return call


def run(call):
    call.launch()
    out = call.read()
    for k, v in out.items():
        assert not np.isnan(v).any(), f"{k}: an element was not written"
    return out


NLL_C = 5
NLL_BATCHES = {
    "wave per cloud": (1, 0, 64, 37),
    "one block per cloud": (300, 0, 1024, 65, 1),
    "partials of 2 and 3 blocks": (1025, 0, 3, 2049, 64),
    "66 clouds, phase 1 on a grid": tuple(int(v) for v in np.random.default_rng(3).integers(1, 10, 40)) + (1025,) + tuple(
        int(v) for v in np.random.default_rng(4).integers(1, 10, 25)),
    "empty first, last and neighbours": (0, 70, 0, 0, 5, 130, 0),
}
assert len(NLL_BATCHES["66 clouds, phase 1 on a grid"]) == 66 > N.LN_NLLC_FUSED_CLOUDS


@functools.lru_cache(maxsize=None)
def nll_case(name, weighted):
    lengths = NLL_BATCHES[name]
    n = sum(lengths)
    ignore = 2
    lp = N.log_probs_case(n, NLL_C, 7 + n)
    y = np.random.default_rng(n).integers(0, NLL_C, n).astype(np.int64)
    y[::5] = ignore
    y[3::17] = NLL_C + 4  # clamped
    w = N.weights_case("random", NLL_C, n) if weighted else None
    for a in (lp, y, w):
        if a is not None:
            a.setflags(write=False)
    return lengths, lp, y, ignore, w


def nll_expected(lengths, lp, y, ignore, w):
    """fp64 per slice with n0 = len, and the bounds of nll_clouds_reference put together as its own `bounds` does for a batch."""
    B = len(lengths)
    pc, ws, e_pc = np.zeros(B), np.ones(B), np.zeros(B)
    grad, e_grad = np.zeros(lp.shape), np.zeros(lp.shape)
    for b, (lo, hi) in enumerate(slices(lengths)):
        if hi == lo:
            continue
        ref = N.reference(lp[lo:hi], y[lo:hi], hi - lo, ignore, w, grad_loss=GRAD_LOSS)
        bnd = N.bounds(ref, hi - lo, hi - lo, w is not None, GRAD_LOSS)
        pc[b], ws[b], e_pc[b] = ref["per_cloud"][0], ref["weight_sum"][0], bnd["per_cloud"][0]
        grad[lo:hi] = ref["grad"] / B
        e_grad[lo:hi] = np.where(ref["grad"] != 0, bnd["grad"] / B + N.TINY32, 0.0)  # (relative bounds: they scale with the 1 / B)
    loss = pc.sum() / B
    e_loss = (e_pc.sum() + N.loss_depth(B) * N.EPS32 * np.sum(np.abs(pc) + e_pc)) / B
    return dict(loss=loss, per_cloud=pc, weight_sum=ws, grad=grad), dict(loss=e_loss, per_cloud=e_pc, grad=e_grad)


def ratio(got, ref, bound):
    return D.worst_ratio(got, ref, bound)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", sorted(NLL_BATCHES))
def test_nll_every_form(name, weighted):
    lengths, lp, y, ignore, w = nll_case(name, weighted)
    got = run(nll_call(lp, y, list(lengths), ignore, w))
    for b, (lo, hi) in enumerate(slices(lengths)):
        if hi == lo:
            assert got["per_cloud"][b] == 0.0 and got["weight_sum"][b] == 1.0
            continue
        one = run(nll_call(lp[lo:hi], y[lo:hi], 1 << 40, ignore, w))  # every cloud
        assert same_bits(got["per_cloud"][b], one["per_cloud"][0]) and same_bits(got["weight_sum"][b], one["weight_sum"][0]), (name, b)
    ref, bnd = nll_expected(lengths, lp, y, ignore, w)
    r = {k: ratio(got[k].reshape(np.shape(ref[k])), ref[k], bnd[k]) for k in ("loss", "per_cloud", "grad")}
    print(f"\n[ragged nll] {name} weighted={weighted}: worst error/bound " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, r
    assert np.count_nonzero(got["grad"]) > 0


# ---------------------------------------------------------------------------------------------------------------------------- Dice
def dice_call(lp, y, cut, ignore):
    L, lib = _lib()
    n, c = lp.shape
    ranged = not isinstance(cut, int)
    B = len(cut) if ranged else len(D.cloud_ranges(n, cut))
    x, t = to_dev(lp), to_dev(y, np.int64)
    ign = NO_LABEL if ignore is None else ignore
    outs = dict(loss=(1,), per_cloud=(B,), stats=(B, 3, c), coef=(B, 2, c), grad=(n, c))
    if ranged:
        st, longest = starts_of(cut), int(max(cut))
        call = Call(outs, lib.ln_dice_ranges_workspace_bytes(n, B, longest, c))
    else:
        call = Call(outs, lib.ln_dice_workspace_bytes(n, cut, c))

    def launch():
        sp = L.stream_ptr(dev())
        if ranged:
            L.check(lib.ln_dice_forward_ranges(L.ptr(x), L.ptr(t), n, L.ptr(st), B, longest, c, ign, L.ptr(call.ws), call.need, call.p("loss"),
                                               call.p("per_cloud"), call.p("stats"), call.p("coef"), sp), "ln_dice_forward_ranges")
            L.check(lib.ln_dice_backward_ranges(L.ptr(x), L.ptr(t), call.p("coef"), L.ptr(call.g), n, L.ptr(st), B, longest, c, call.p("grad"),
                                                sp), "ln_dice_backward_ranges")
        else:
            L.check(lib.ln_dice_forward(L.ptr(x), L.ptr(t), n, cut, c, ign, L.ptr(call.ws), call.need, call.p("loss"), call.p("per_cloud"),
                                        call.p("stats"), call.p("coef"), sp), "ln_dice_forward")
            L.check(lib.ln_dice_backward(L.ptr(x), L.ptr(t), call.p("coef"), L.ptr(call.g), n, cut, c, call.p("grad"), sp), "ln_dice_backward")
    call.launch = launch
    call.keep = (x, t, st if ranged else None)
    return call


DICE_CASES = {"C = 20": (20, (193, 0, 12, 500, 1)), "C = 300, the wide form": (300, (17, 0, 1, 40))}


@functools.lru_cache(maxsize=None)
def dice_case(name):
    c, lengths = DICE_CASES[name]
    n = sum(lengths)
    assert [D.tiling(m, c)[2] for m in lengths] == ([2, 0, 1, 3, 1] if c == 20 else [2, 0, 1, 3])
    lp, y = D.inputs(n, c, 5 + c), D.labels(n, c, 9 + c)
    lp.setflags(write=False)
    y.setflags(write=False)
    return c, lengths, lp, y, 3


@pytest.mark.parametrize("name", sorted(DICE_CASES))
def test_dice_every_form(name):
    c, lengths, lp, y, ignore = dice_case(name)
    B = len(lengths)
    got = run(dice_call(lp, y, list(lengths), ignore))
    pc, e_pc, worst = np.zeros(B), np.zeros(B), 0.0
    for b, (lo, hi) in enumerate(slices(lengths)):
        if hi == lo:  # the one-cloud formula on no rows: every class that is not ignored contributes 1 / C
            assert same_bits(got["per_cloud"][b], np.float32(c - 1) / np.float32(c)) and not got["stats"][b].any()
            pc[b], e_pc[b] = (c - 1) / c, D.EPS32 * (c - 1) / c
            continue
        one = run(dice_call(lp[lo:hi], y[lo:hi], 1 << 40, ignore))
        assert same_bits(got["per_cloud"][b], one["per_cloud"][0]) and same_bits(got["stats"][b], one["stats"][0]), (name, b)
        # coef carries the 1 / B: times B it is the one-cloud row bit for bit only when B is a power of two (C = 300: B = 4); otherwise the
        # division rounds (C = 20: B = 5) and the row is held by its bound below
        assert same_bits(got["coef"][b] * np.float32(B), one["coef"][0]) or B & (B - 1), (name, b)
        ref = D.reference(lp[lo:hi], y[lo:hi], hi - lo, ignore)
        ref["coef"], ref["grad"] = ref["coef"] / B, ref["grad"] / B  # what cloud b of B clouds carries
        bnd = D.bounds(ref, lp[lo:hi], y[lo:hi], hi - lo, ignore, GRAD_LOSS)
        pc[b], e_pc[b] = ref["per_cloud"][0], bnd["per_cloud"][0]
        worst = max(worst, ratio(got["grad"][lo:hi], ref["grad"] * GRAD_LOSS, bnd["grad"]), ratio(got["coef"][b], ref["coef"][0], bnd["coef"][0]))
    e_loss = e_pc.mean() + D.gamma(D.cloud_sum_depth(B) + 1) * (np.abs(pc) + e_pc).mean()
    r = dict(loss=ratio(got["loss"][0], pc.sum() / B, e_loss), per_cloud=ratio(got["per_cloud"], pc, e_pc), grad_coef=worst)
    print(f"\n[ragged dice] {name}: worst error/bound " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, r


# ---------------------------------------------------------------------------------------------------------------------------- Lovasz
def lovasz_call(lp, y, cut, ignore, reduction):
    """cut: a list of lengths (ln_lovasz_forward_ranges), an int (ln_lovasz_forward_clouds) or None (ln_lovasz_forward)."""
    L, lib = _lib()
    n, c = lp.shape
    ranged = isinstance(cut, list)
    B = len(cut) if ranged else (1 if cut is None else len(LC.cloud_ranges(n, cut)))
    x, t = to_dev(lp), to_dev(y, np.int64)
    ign = NO_LABEL if ignore is None else ignore
    red = 0 if reduction == "mean" else 1
    outs = dict(loss=(1,), per_cloud=(B,), per_class=(B, c), dloss=(n, c), grad=(n, c))
    if ranged:
        st, longest = starts_of(cut), int(max(cut))
        call = Call(outs, lib.ln_lovasz_ranges_workspace_bytes(n, B, longest, c))
    else:
        call = Call(outs, lib.ln_lovasz_workspace_bytes(n, c) if cut is None else lib.ln_lovasz_clouds_workspace_bytes(n, cut, c))

    def launch():
        sp = L.stream_ptr(dev())
        if ranged:
            L.check(lib.ln_lovasz_forward_ranges(L.ptr(x), L.ptr(t), n, L.ptr(st), B, longest, c, ign, red, L.ptr(call.ws), call.need,
                                                 call.p("loss"), call.p("per_cloud"), call.p("per_class"), call.p("dloss"), sp),
                    "ln_lovasz_forward_ranges")
        elif cut is None:
            L.check(lib.ln_lovasz_forward(L.ptr(x), L.ptr(t), n, c, ign, red, L.ptr(call.ws), call.need, call.p("loss"), call.p("per_class"),
                                          call.p("dloss"), sp), "ln_lovasz_forward")
        else:
            L.check(lib.ln_lovasz_forward_clouds(L.ptr(x), L.ptr(t), n, cut, c, ign, red, L.ptr(call.ws), call.need, call.p("loss"),
                                                 call.p("per_cloud"), call.p("per_class"), call.p("dloss"), sp), "ln_lovasz_forward_clouds")
        L.check(lib.ln_lovasz_backward(call.p("dloss"), L.ptr(call.g), n, c, call.p("grad"), sp), "ln_lovasz_backward")
    call.launch = launch
    call.keep = (x, t, st if ranged else None)
    return call


def run_lovasz(call, one_cloud=False):
    call.launch()
    out = call.read()
    if one_cloud:
        out.pop("per_cloud")  # (ln_lovasz_forward has no such output)
    for k, v in out.items():
        assert not np.isnan(v).any(), f"{k}: an element was not written"
    return out


LOVASZ_C = 4
LOVASZ_LENGTHS = (2049, 0, 1, 300, 2048)  # two tiles, none, one, one, one


@functools.lru_cache(maxsize=None)
def lovasz_case():
    # the separated family, cloud by cloud as lovasz_clouds_reference.batch draws it: inside a class all errors of a cloud differ by at
    # least 0.5 / (len + 1), so the fp32 sort and the fp64 reference rank the points alike and the gradient can be held element by element
    n = sum(LOVASZ_LENGTHS)
    lp = np.concatenate([LV.separated(m, LOVASZ_C, 11 + 31 * b) for b, m in enumerate(LOVASZ_LENGTHS)])
    y = LV.labels(n, LOVASZ_C, 12, out_of_range=True)
    lp.setflags(write=False)
    y.setflags(write=False)
    return lp, y, 1  # ignore_index inside the classes


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_lovasz_every_form(reduction):
    lp, y, ignore = lovasz_case()
    lengths, B, c = LOVASZ_LENGTHS, len(LOVASZ_LENGTHS), LOVASZ_C
    assert [LV.tiles(m) for m in lengths] == [2, 0, 1, 1, 1]
    got = run_lovasz(lovasz_call(lp, y, list(lengths), ignore, reduction))
    pc, e_pc, grad = np.zeros(B), np.zeros(B), np.zeros(lp.shape)
    for b, (lo, hi) in enumerate(slices(lengths)):
        if hi == lo:
            assert same_bits(got["per_cloud"][b], np.float32(0)) and same_bits(got["per_class"][b], np.zeros(c, np.float32))
            continue
        one = run_lovasz(lovasz_call(lp[lo:hi], y[lo:hi], None, ignore, reduction), one_cloud=True)
        assert same_bits(got["per_cloud"][b], one["loss"][0]) and same_bits(got["per_class"][b], one["per_class"][0]), (reduction, b)
        loss_b, per_class_b, grad_b = LV.reference(lp[lo:hi], y[lo:hi], ignore, reduction)
        pc[b], grad[lo:hi] = loss_b, grad_b / B
        e_pc[b] = LV.loss_bound(per_class_b, hi - lo, reduction, LV.counting_classes(y[lo:hi], c, ignore))
    want_grad = grad * GRAD_LOSS
    r = dict(loss=ratio(got["loss"][0], pc.sum() / B, LC.loss_bound(pc, e_pc)), per_cloud=ratio(got["per_cloud"], pc, e_pc),
             grad=LV.worst_ratio(got["grad"], want_grad, LV.grad_bound(want_grad, LC.r_grad(B, through_backward=True))))
    print(f"\n[ragged lovasz] {reduction}: worst error/bound " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, r
    assert np.count_nonzero(got["grad"]) > 0


# ---------------------------------------------------------------------------------------------- properties of all three loss families
def family_calls():
    """(name, call over lengths-or-int, lp, y, lengths, equal-size n0 and lengths (n0, .., n0, rest))"""
    lengths, lp, y, ignore, w = nll_case("partials of 2 and 3 blocks", True)
    yield "nll", (lambda x, cut: nll_call(x, y, cut, ignore, w)), lp, lengths, 1025
    yield "nll wave", (lambda x, cut: nll_call(x, y, cut, ignore, w)), lp, lengths, 37
    c, dl, dlp, dy, dig = dice_case("C = 20")
    yield "dice", (lambda x, cut: dice_call(x, dy, cut, dig)), dlp, dl, 193
    llp, ly, lig = lovasz_case()
    yield "lovasz", (lambda x, cut: lovasz_call(x, ly, cut, lig, "mean")), llp, LOVASZ_LENGTHS, 2049


def outputs(call):
    call.launch()
    return call.read()


def assert_same(a, b, what, skip=()):
    for k in a:
        if k not in skip:
            assert same_bits(a[k], b[k]), (what, k)


def test_equal_lengths_are_the_equal_size_entry_points_bit_for_bit():
    for name, make, lp, lengths, n0 in family_calls():
        n = lp.shape[0]
        eq = [n0] * (n // n0) + ([n % n0] if n % n0 else [])
        new, old = outputs(make(lp, eq)), outputs(make(lp, n0))
        assert not any(np.isnan(v).any() for v in new.values()), name
        assert_same(new, old, name)  # loss, per-cloud outputs, every gradient element


def test_scaling_one_cloud_leaves_the_others_unchanged():
    for name, make, lp, lengths, _ in family_calls():
        ranges = slices(lengths)
        base = outputs(make(lp, list(lengths)))
        lo, hi = ranges[3]
        moved = np.array(lp)
        moved[lo:hi] *= np.float32(1.5)
        got = outputs(make(moved, list(lengths)))
        changed = False
        for k, v in base.items():
            if k == "loss":
                continue
            rows = v.shape[0]
            if rows == lp.shape[0]:  # per point: the gradient rows of the other clouds
                keep = np.ones(rows, bool)
                keep[lo:hi] = False
            else:  # per cloud
                keep = np.arange(rows) != 3
            assert same_bits(v[keep], got[k][keep]), (name, k)
            changed = changed or not same_bits(v[~keep], got[k][~keep])
        assert changed, name


def test_two_runs_and_two_graph_replays_are_bitwise_equal():
    for name, make, lp, lengths, _ in family_calls():
        first, second = outputs(make(lp, list(lengths))), outputs(make(lp, list(lengths)))
        assert_same(first, second, name)
        call = make(lp, list(lengths))
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            call.launch()  # (warm-up outside the capture)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call.launch()
        replays = []
        for _ in range(2):
            for t, _shape in call.out.values():
                t[:-GUARD] = NAN
            graph.replay()
            replays.append(call.read())
        assert_same(replays[0], replays[1], name + " replay")
        assert_same(replays[0], first, name + " replay against the eager run")


def test_every_refusal_returns_its_code_and_writes_nothing():
    """Each of the five entry points on real buffers (NaN-filled outputs, guard words, a guarded workspace): a null list, clouds < 1,
    clouds > 65 535, longest < 0, longest > n and the size limits return the family's code, name the entry point and leave every output
    element and the workspace as they were."""
    L, lib = _lib()
    lengths, lp, y, ignore, _ = nll_case("wave per cloud", False)
    n, c = lp.shape
    B = len(lengths)
    x, t, st = to_dev(lp), to_dev(y, np.int64), starts_of(lengths)
    g = torch.tensor([GRAD_LOSS], dtype=torch.float32, device=dev())
    ws = torch.full((1 << 20,), 0xA5, dtype=torch.uint8, device=dev())
    outs = {k: guarded(m) for k, m in dict(loss=1, per_cloud=B, side=B * 3 * c, coef=B * 2 * c, grad=n * c).items()}
    o = {k: L.ptr(v) for k, v in outs.items()}
    X, T, S, W, G = L.ptr(x), L.ptr(t), L.ptr(st), L.ptr(ws), L.ptr(g)
    entries = {
        "ln_nll_forward_ranges": (-2, lambda n_, s_, b_, lg, c_: lib.ln_nll_forward_ranges(X, T, n_, s_, b_, lg, c_, ignore, None, W, ws.numel(), o["loss"],
                                                                                             o["per_cloud"], o["side"], None)),
        "ln_nll_backward_ranges": (-2, lambda n_, s_, b_, lg, c_: lib.ln_nll_backward_ranges(T, G, o["side"], n_, s_, b_, lg, c_, ignore, None, o["grad"],
                                                                                               None)),
        "ln_dice_forward_ranges": (-1, lambda n_, s_, b_, lg, c_: lib.ln_dice_forward_ranges(X, T, n_, s_, b_, lg, c_, ignore, W, ws.numel(), o["loss"],
                                                                                               o["per_cloud"], o["side"], o["coef"], None)),
        "ln_dice_backward_ranges": (-1, lambda n_, s_, b_, lg, c_: lib.ln_dice_backward_ranges(X, T, o["coef"], G, n_, s_, b_, lg, c_, o["grad"], None)),
        "ln_lovasz_forward_ranges": (-1, lambda n_, s_, b_, lg, c_: lib.ln_lovasz_forward_ranges(X, T, n_, s_, b_, lg, c_, ignore, 0, W, ws.numel(), o["loss"],
                                                                                                   o["per_cloud"], o["side"], o["grad"], None)),
    }
    longest = max(lengths)
    checked = 0
    for name, (limit, call) in entries.items():
        for args, code in (((n, None, B, longest, c), -1), ((n, S, 0, longest, c), -1), ((n, S, -3, longest, c), -1),
                           ((n, S, 65536, longest, c), limit), ((n, S, B, -1, c), -1), ((n, S, B, n + 1, c), -1), ((-1, S, B, 0, c), -1),
                           ((n, S, B, longest, 0), -1), ((1 << 29, S, B, longest, c), limit)):
            assert call(*args) == code, (name, args)
            assert name.encode() in lib.ln_last_error_string(), (name, args)
            checked += 1
    assert lib.ln_lovasz_forward_ranges(X, T, n, S, B, longest, c, ignore, 2, W, ws.numel(), o["loss"], o["per_cloud"], o["side"], o["grad"], None) == -1
    assert lib.ln_nll_forward_ranges(X, T, n, S, B, longest, c, ignore, None, W, 8, o["loss"], o["per_cloud"], o["side"], None) == -1
    assert lib.ln_dice_forward_ranges(X, T, n, S, B, longest, c, ignore, W, 8, o["loss"], o["per_cloud"], o["side"], o["coef"], None) == -1
    torch.cuda.synchronize()
    assert checked == 45
    for k, v in outs.items():
        assert bool(torch.isnan(v[:-GUARD]).all()) and bool((v[-GUARD:] == 7).all()), k
    assert bool((ws == 0xA5).all())
