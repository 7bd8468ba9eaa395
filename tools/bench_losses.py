#!/usr/bin/env python3
"""Time of the training losses on a [120k, 20] prediction: NLL (then with class weights and per cloud: ln_nll_forward_clouds against
ln_nll_forward, torch's nll_loss(weight=) and the torch gather form; `--nll` stops after these lines), Lovasz-Softmax (HIP kernels, and the torch form with
losses.FUSED_LOVASZ off), soft Dice (HIP kernels, and the torch form with losses.FUSED_DICE off; then per cloud); forward + backward.  Then the same matrix as a batch of 16 clouds x 7 500 points: the per-cloud
loss (ln_lovasz_forward_clouds against 16 calls of ln_lovasz_forward and against the batched torch form) and the per-cloud IoU
counts (ln_iou_counts_clouds against Scores.accumulate_scores cloud by cloud).  `--ragged` runs only the C-ABI lines of clouds of unequal
sizes (the _ranges entry points, which losses.py does not call yet): forward + backward calls alone, no log-softmax, 16 clouds of 5 068 to
9 825 points against the equal-size entry points at 16 x 7 500 and at one cloud of 120 000."""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lattice_net_amd import losses
from lattice_net_amd.losses import GeneralizedSoftDiceLoss, LovaszSoftmax, nll_loss_gather
dev = torch.device("cuda", 0)
n, c = 120000, 20
logits = torch.randn((n, c), device=dev, requires_grad=True)
target = torch.randint(0, c, (n,), device=dev)
lov, dice = LovaszSoftmax(ignore_index=0), GeneralizedSoftDiceLoss(ignore_index=0)
def run(fn):
    for _ in range(3):
        logits.grad = None
        fn(torch.log_softmax(logits, 1)).backward()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        logits.grad = None
        fn(torch.log_softmax(logits, 1)).backward()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / 20 * 1e3
print(f"log_softmax + nll   {run(lambda lp: nll_loss_gather(lp, target, 0)):6.3f} ms")

# ---- NLL with class weights and per cloud (ln_nll_forward_clouds) against the torch forms, one cloud and 16 clouds x 7 500 points ---------
# Every line: windows of 200 steps (log_softmax + loss forward + backward), 21 windows per variant taken in turn, variant after
# variant, so that a drift of the clock hits all of them alike (a round before them is dropped); median, fastest and slowest window.  FUSED_NLL_CLOUDS goes on only when
# the kernels' median is below the torch form's by more than the spread (slowest - fastest window) of either, at BOTH shapes.
def nll_section():
    weight = (1.0 / torch.log(1.05 + torch.bincount(target, minlength=c).float() / n)).to(dev)
    weight[0] = 1e-8
    def window(fn, steps=200):
        for _ in range(3):
            logits.grad = None
            fn(torch.log_softmax(logits, 1)).backward()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            logits.grad = None
            fn(torch.log_softmax(logits, 1)).backward()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3
    def with_switch(fused, weight, n0):  # (the function form on every line: no Module.__call__ on one side only)
        def fn(lp):
            losses.FUSED_NLL_CLOUDS = fused
            return nll_loss_gather(lp, target, 0, weight=weight, points_per_cloud=n0)
        return fn
    one, one_w, per, per_w = (None, n), (weight, n), (None, 7500), (weight, 7500)
    variants = [
        ("120000 x 20, one cloud: ln_nll_forward / _backward (no weights)           ", lambda lp: nll_loss_gather(lp, target, 0)),
        ("120000 x 20, one cloud: ln_nll_forward_clouds / _backward_clouds, no weights", with_switch(True, *one)),
        ("120000 x 20, one cloud: ln_nll_forward_clouds / _backward_clouds, weights   ", with_switch(True, *one_w)),
        ("120000 x 20, one cloud: torch.nn.functional.nll_loss(weight=)               ",
         lambda lp: torch.nn.functional.nll_loss(lp, target, weight=weight, ignore_index=0)),
        ("120000 x 20, one cloud: torch gather form, weights                          ", with_switch(False, *one_w)),
        ("16 x 7500 x 20: ln_nll_forward_clouds / _backward_clouds, no weights        ", with_switch(True, *per)),
        ("16 x 7500 x 20: ln_nll_forward_clouds / _backward_clouds, weights           ", with_switch(True, *per_w)),
        ("16 x 7500 x 20: batched torch gather form per cloud, no weights             ", with_switch(False, *per)),
        ("16 x 7500 x 20: batched torch gather form per cloud, weights                ", with_switch(False, *per_w)),
    ]
    default = losses.FUSED_NLL_CLOUDS
    times = [[] for _ in variants]
    for r in range(22):  # (the first round warms the clocks and is dropped)
        for k, (_, fn) in enumerate(variants):
            t = window(fn)
            if r:
                times[k].append(t)
    losses.FUSED_NLL_CLOUDS = default
    for (name, _), t in zip(variants, times):
        t.sort()
        print(f"{name} median {t[len(t) // 2]:6.4f} ms, fastest {t[0]:6.4f} ms, slowest {t[-1]:6.4f} ms")

# ---- clouds of unequal sizes through the C ABI: 21 windows of 200 forward + backward calls per variant, taken in turn (a round dropped) ----
def ragged_section():
    import random
    from lattice_net_amd import _lib
    lib, P = _lib.load(), _lib.ptr
    lengths = None
    for seed in range(1000):  # (bounded: a seed whose 16th length fits the range)
        rng = random.Random(seed)
        ls = [rng.randint(5068, 9825) for _ in range(15)]
        if 5068 <= n - sum(ls) <= 9825:
            lengths = ls + [n - sum(ls)]
            break
    if lengths is None:
        sys.exit("no seed below 1000 gives 16 lengths in 5068 .. 9825 that sum to %d" % n)
    B, longest = len(lengths), max(lengths)
    starts = torch.tensor([sum(lengths[:k]) for k in range(B + 1)], dtype=torch.int32, device=dev)
    print(f"ragged batch: {B} clouds of {min(lengths)} .. {max(lengths)} points, {n} in all")
    lp = torch.log_softmax(logits.detach(), 1).contiguous()
    g = torch.ones((1,), device=dev)
    ws = torch.empty((max(lib.ln_lovasz_ranges_workspace_bytes(n, B, longest, c), lib.ln_lovasz_clouds_workspace_bytes(n, 7500, c),
                          lib.ln_lovasz_workspace_bytes(n, c)),), dtype=torch.uint8, device=dev)
    loss, pc, side, coef = (torch.empty((k,), device=dev) for k in (1, B, B * 3 * c, B * 2 * c))
    dl, grad = torch.empty((n, c), device=dev), torch.empty((n, c), device=dev)
    sp = _lib.stream_ptr(dev)
    W, nb = P(ws), ws.numel()
    def nll(n0):
        def f():
            if n0 is None:
                lib.ln_nll_forward_ranges(P(lp), P(target), n, P(starts), B, longest, c, 0, None, W, nb, P(loss), P(pc), P(side), sp)
                lib.ln_nll_backward_ranges(P(target), P(g), P(side), n, P(starts), B, longest, c, 0, None, P(grad), sp)
            else:
                lib.ln_nll_forward_clouds(P(lp), P(target), n, n0, c, 0, None, W, nb, P(loss), P(pc), P(side), sp)
                lib.ln_nll_backward_clouds(P(target), P(g), P(side), n, n0, c, 0, None, P(grad), sp)
        return f
    def dice(n0):
        def f():
            if n0 is None:
                lib.ln_dice_forward_ranges(P(lp), P(target), n, P(starts), B, longest, c, 0, W, nb, P(loss), None, None, P(coef), sp)
                lib.ln_dice_backward_ranges(P(lp), P(target), P(coef), P(g), n, P(starts), B, longest, c, P(grad), sp)
            else:
                lib.ln_dice_forward(P(lp), P(target), n, n0, c, 0, W, nb, P(loss), None, None, P(coef), sp)
                lib.ln_dice_backward(P(lp), P(target), P(coef), P(g), n, n0, c, P(grad), sp)
        return f
    def lovasz(n0):
        def f():
            if n0 is None:
                lib.ln_lovasz_forward_ranges(P(lp), P(target), n, P(starts), B, longest, c, 0, 0, W, nb, P(loss), None, None, P(dl), sp)
            else:
                lib.ln_lovasz_forward_clouds(P(lp), P(target), n, n0, c, 0, 0, W, nb, P(loss), None, None, P(dl), sp)
            lib.ln_lovasz_backward(P(dl), P(g), n, c, P(grad), sp)
        return f
    def window(fn, steps=200):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3
    variants = [(f"{name}, {shape}", make(n0)) for name, make in (("nll   ", nll), ("dice  ", dice), ("lovasz", lovasz))
                for shape, n0 in (("16 x 7500 ", 7500), ("1 x 120000", n), ("16 ragged ", None))]
    times = [[] for _ in variants]
    for r in range(22):
        for k, (_, fn) in enumerate(variants):
            t = window(fn)
            if r:
                times[k].append(t)
    for (name, _), t in zip(variants, times):
        t.sort()
        print(f"{name} median {t[len(t) // 2]:6.4f} ms, fastest {t[0]:6.4f} ms, slowest {t[-1]:6.4f} ms")
if "--ragged" in sys.argv:  # (only these lines)
    ragged_section()
    sys.exit(0)
nll_section()
if "--nll" in sys.argv:  # (only the lines above)
    sys.exit(0)

def run_lovasz(fused):
    losses.FUSED_LOVASZ = fused
    return run(lambda lp: lov(lp, target))
default = losses.FUSED_LOVASZ
# median of five runs of 20 steps and the fastest of the five: FUSED_LOVASZ goes on only when the kernels' median is below the torch
# form's fastest run
def five(fn):
    t = sorted(fn() for _ in range(5))
    return f"median {t[2]:6.3f} ms, fastest {t[0]:6.3f} ms"
print(f"log_softmax + lovasz (HIP kernels) {five(lambda: run_lovasz(True))}")
print(f"log_softmax + lovasz (torch form)  {five(lambda: run_lovasz(False))}")
losses.FUSED_LOVASZ = default
# soft Dice, one cloud and 16 clouds x 7 500 points: FUSED_DICE goes on only when the kernels' median is below the torch form's fastest
# run in BOTH pairs
def run_dice(fused, loss):
    losses.FUSED_DICE = fused
    return run(lambda lp: loss(lp, target))
default_dice = losses.FUSED_DICE
dice_clouds = GeneralizedSoftDiceLoss(ignore_index=0, points_per_cloud=7500)
print(f"log_softmax + dice (torch form)                          {five(lambda: run_dice(False, dice))}")
print(f"log_softmax + dice (HIP kernels)                         {five(lambda: run_dice(True, dice))}")
print(f"16 x 7500: log_softmax + dice per cloud (torch form)     {five(lambda: run_dice(False, dice_clouds))}")
print(f"16 x 7500: log_softmax + dice per cloud (HIP kernels)    {five(lambda: run_dice(True, dice_clouds))}")
losses.FUSED_DICE = default_dice

# ---- a batch of clouds: 16 clouds x 7 500 points, the per-cloud loss and the per-cloud IoU counts -----------------------------------
# (each line: five(), as above)
clouds, n0 = 16, 7500
lov_clouds = LovaszSoftmax(ignore_index=0, points_per_cloud=n0)
def per_cloud_calls(lp):
    return sum(lov(lp[b * n0:(b + 1) * n0], target[b * n0:(b + 1) * n0]) for b in range(clouds)) / clouds
def run_clouds(fused, fn):
    losses.FUSED_LOVASZ = fused
    return run(fn)
print(f"16 x 7500: log_softmax + lovasz per cloud (ln_lovasz_forward_clouds)   {five(lambda: run_clouds(True, lambda lp: lov_clouds(lp, target)))}")
print(f"16 x 7500: log_softmax + lovasz per cloud (16 x ln_lovasz_forward)     {five(lambda: run_clouds(True, per_cloud_calls))}")
print(f"16 x 7500: log_softmax + lovasz per cloud (batched torch form)         {five(lambda: run_clouds(False, lambda lp: lov_clouds(lp, target)))}")
print(f"16 x 7500: log_softmax + lovasz whole batch (torch form, for scale)    {five(lambda: run_clouds(False, lambda lp: lov(lp, target)))}")
losses.FUSED_LOVASZ = default
probs = torch.softmax(logits.detach(), 1)
def run_scores(per_cloud_kernel):
    s = losses.Scores()
    def once():
        if per_cloud_kernel:
            s.accumulate_scores(probs, target, 0, points_per_cloud=n0)
        else:
            for b in range(clouds):
                s.accumulate_scores(probs[b * n0:(b + 1) * n0], target[b * n0:(b + 1) * n0], 0)
    for _ in range(3):
        once()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        once()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / 20 * 1e3
print(f"16 x 7500: IoU counts (ln_iou_counts_clouds)                           {five(lambda: run_scores(True))}")
print(f"16 x 7500: IoU counts (accumulate_scores cloud by cloud)               {five(lambda: run_scores(False))}")
