#!/usr/bin/env python3
"""Time of the training losses on a [120k, 20] prediction: NLL, Lovasz-Softmax (HIP kernels, and the torch form with
losses.FUSED_LOVASZ off), soft Dice (HIP kernels, and the torch form with losses.FUSED_DICE off; then per cloud); forward + backward.  Then the same matrix as a batch of 16 clouds x 7 500 points: the per-cloud
loss (ln_lovasz_forward_clouds against 16 calls of ln_lovasz_forward and against the batched torch form) and the per-cloud IoU
counts (ln_iou_counts_clouds against Scores.accumulate_scores cloud by cloud)."""
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
