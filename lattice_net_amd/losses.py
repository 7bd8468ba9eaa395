"""Training-side pieces of SURVEY.md §8f-4: the Lovasz-Softmax loss used next to NLL (ln_train.py:128-157, reference
latticenet_py/lattice/lovasz_loss.py:17-57) and the intersection-over-union bookkeeping (callbacks/scores.py).

The loss is the Lovasz extension of the per-class Jaccard index (Berman et al., CVPR 2018): for class c the errors
e_i = |1[y_i = c] - p_i(c)| are sorted in decreasing order and dotted with the discrete gradient of the Jaccard loss
along that order; classes absent from the cloud and the ignore class are skipped, the rest averaged.  All classes are
processed at once with no host synchronisation — the reference loops over classes and reads one scalar per class back to
the host.  With FUSED_LOVASZ set, float32 CUDA inputs take the HIP kernels of csrc/ln_lovasz.hip; everything else, and everything while
the flag is off, the torch form ([C, N] sort / cumsum).

A batch of clouds in one lattice (Lattice.set_cloud_batch) hands its log-probabilities over as one cloud-major [N, C] matrix.  The
reference's step and its validation work on ONE cloud: LovaszSoftmax(points_per_cloud=) and Scores.accumulate_scores(points_per_cloud=)
take the loss and the counts per cloud (Berman's per_image=True), so that a batched step is the mean of the clouds' reference steps.
"""
from __future__ import annotations

import os

import torch

__all__ = ["GeneralizedSoftDiceLoss", "LovaszSoftmax", "NLLLoss", "Scores", "SegmentationLoss", "log_softmax", "nll_loss_gather"]


_NO_LABEL = -(1 << 62)  # "no ignore_index": a value no label takes
FUSED_NLL = True
FUSED_IOU_COUNTS = True  # Scores.accumulate_scores(points_per_cloud=): integer-exact either way, and the torch form of one cloud synchronises
FUSED_LOVASZ = False  # off until tools/bench_losses.py has shown the kernels below the torch form on an MI355X
FUSED_DICE = True  # by the rule FUSED_LOVASZ states: tools/bench_losses.py on an MI355X has csrc/ln_dice.hip below the torch form, one cloud and per cloud
FUSED_NLL_CLOUDS = True  # nll_loss_gather(weight=, points_per_cloud=) / NLLLoss: by the rule FUSED_LOVASZ states, tools/bench_losses.py on an MI355X has csrc/ln_nll.hip below the torch forms, one cloud and per cloud
_LOVASZ_MAX_CLASSES = 1024 # limits of ln_lovasz_forward (include/latticenet_hip.h)
_LOVASZ_MAX_ELEMENTS = 1 << 31
_LOVASZ_MAX_CLOUDS = 65535  # of ln_lovasz_forward_clouds and ln_iou_counts_clouds


def _label_or_none(ignore_index) -> int:
    """ignore_index as the kernels take it."""
    return _NO_LABEL if ignore_index is None else int(ignore_index)


def _checked_points_per_cloud(points_per_cloud):
    """The points_per_cloud argument of a loss's constructor: None or an int >= 1."""
    if points_per_cloud is None:
        return None
    if int(points_per_cloud) < 1:
        raise ValueError("points_per_cloud >= 1")
    return int(points_per_cloud)


def _clouds_ok(n, points_per_cloud) -> bool:
    """The batch has no more clouds than the kernels take (None: one cloud)."""
    return points_per_cloud is None or -(-n // points_per_cloud) <= _LOVASZ_MAX_CLOUDS


def _lovasz_fused_ok(inputs, targets) -> bool:
    """The inputs LovaszSoftmax hands to the kernels (reduction "mean" or "sum"), while FUSED_LOVASZ is set."""
    return FUSED_LOVASZ and _kernel_inputs(inputs, targets)


def _kernel_inputs(inputs, targets) -> bool:
    return inputs.is_cuda and inputs.dtype == torch.float32 and inputs.is_contiguous() and targets.is_cuda and \
        targets.dtype == torch.int64 and targets.numel() == inputs.shape[0] and inputs.shape[0] >= 1 and \
        1 <= inputs.shape[1] <= _LOVASZ_MAX_CLASSES and inputs.numel() < _LOVASZ_MAX_ELEMENTS


def _dice_fused_ok(inputs, targets) -> bool:
    """The inputs GeneralizedSoftDiceLoss hands to the kernels (the limits of ln_dice_forward are the Lovasz ones), while FUSED_DICE is set."""
    return FUSED_DICE and inputs.dim() == 2 and _kernel_inputs(inputs, targets)


class _NllFunction(torch.autograd.Function):
    """csrc/ln_nll.hip, its one-cloud entry without class weights: at most two launches forward (partial sums in a fixed order, one
    finishing workgroup), one backward that writes the whole [n, C] gradient — instead of gather / mean and the zero fill + scatter of
    their autograd."""

    @staticmethod
    def forward(ctx, log_probs, target, ignore_index):
        from . import _lib
        lib = _lib.load()
        lp = log_probs.contiguous()
        n, c = lp.shape
        dev = lp.device
        ws = torch.empty((lib.ln_nll_workspace_bytes(),), dtype=torch.uint8, device=dev)
        loss_count = torch.empty((2,), dtype=torch.float32, device=dev)
        _lib.check(lib.ln_nll_forward(_lib.ptr(lp), _lib.ptr(target), n, c, ignore_index, _lib.ptr(ws), ws.numel(), _lib.ptr(loss_count),
                                      _lib.stream_ptr(dev)), "ln_nll_forward")
        ctx.save_for_backward(target, loss_count)
        ctx.shape, ctx.ignore_index = (n, c), ignore_index
        return loss_count[0]

    @staticmethod
    def backward(ctx, grad_loss):
        from . import _lib
        target, loss_count = ctx.saved_tensors
        n, c = ctx.shape
        g = grad_loss.contiguous().float()
        grad = torch.empty((n, c), dtype=torch.float32, device=g.device)
        _lib.check(_lib.load().ln_nll_backward(_lib.ptr(target), _lib.ptr(g), _lib.ptr(loss_count), n, c, ctx.ignore_index, _lib.ptr(grad),
                                               _lib.stream_ptr(g.device)), "ln_nll_backward")
        return grad, None, None


class _LovaszFunction(torch.autograd.Function):
    """csrc/ln_lovasz.hip: per-class stable radix sort of the errors, Jaccard gradient in closed form, sums in a fixed order.  The
    forward call leaves d loss / d log_probs in memory; backward is one elementwise launch."""

    @staticmethod
    def forward(ctx, log_probs, target, ignore_index, reduction):
        from . import _lib
        lib = _lib.load()
        n, c = log_probs.shape
        dev = log_probs.device
        ws = torch.empty((lib.ln_lovasz_workspace_bytes(n, c),), dtype=torch.uint8, device=dev)
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        dloss = torch.empty((n, c), dtype=torch.float32, device=dev)
        _lib.check(lib.ln_lovasz_forward(_lib.ptr(log_probs), _lib.ptr(target), n, c, ignore_index, reduction, _lib.ptr(ws), ws.numel(),
                                         _lib.ptr(loss), None, _lib.ptr(dloss), _lib.stream_ptr(dev)), "ln_lovasz_forward")
        ctx.save_for_backward(dloss)
        return loss[0]

    @staticmethod
    def backward(ctx, grad_loss):
        from . import _lib
        dloss, = ctx.saved_tensors
        n, c = dloss.shape
        g = grad_loss.contiguous().float()
        grad = torch.empty_like(dloss)
        _lib.check(_lib.load().ln_lovasz_backward(_lib.ptr(dloss), _lib.ptr(g), n, c, _lib.ptr(grad), _lib.stream_ptr(g.device)),
                   "ln_lovasz_backward")
        return grad, None, None, None


class _LovaszCloudsFunction(torch.autograd.Function):
    """ln_lovasz_forward_clouds: the same kernels over (cloud, class) segments, the mean over the clouds; d loss / d log_probs carries
    the 1 / clouds, so the backward is that of _LovaszFunction."""

    @staticmethod
    def forward(ctx, log_probs, target, ignore_index, reduction, points_per_cloud):
        from . import _lib
        lib = _lib.load()
        n, c = log_probs.shape
        dev = log_probs.device
        ws = torch.empty((lib.ln_lovasz_clouds_workspace_bytes(n, points_per_cloud, c),), dtype=torch.uint8, device=dev)
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        dloss = torch.empty((n, c), dtype=torch.float32, device=dev)
        _lib.check(lib.ln_lovasz_forward_clouds(_lib.ptr(log_probs), _lib.ptr(target), n, points_per_cloud, c, ignore_index, reduction,
                                                _lib.ptr(ws), ws.numel(), _lib.ptr(loss), None, None, _lib.ptr(dloss), _lib.stream_ptr(dev)),
                   "ln_lovasz_forward_clouds")
        ctx.save_for_backward(dloss)
        return loss[0]

    @staticmethod
    def backward(ctx, grad_loss):
        return _LovaszFunction.backward(ctx, grad_loss) + (None,)


class _DiceFunction(torch.autograd.Function):
    """csrc/ln_dice.hip: two launches forward (per-tile partial sums of I, S, G in a fixed order, one finishing workgroup that leaves
    the coefficients a, b per (cloud, class)), one backward that writes the whole [n, C] gradient.  points_per_cloud >= n: one cloud."""

    @staticmethod
    def forward(ctx, log_probs, target, ignore_index, points_per_cloud):
        from . import _lib
        lib = _lib.load()
        n, c = log_probs.shape
        dev = log_probs.device
        clouds = -(-n // points_per_cloud)
        ws = torch.empty((lib.ln_dice_workspace_bytes(n, points_per_cloud, c),), dtype=torch.uint8, device=dev)
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        coef = torch.empty((clouds, 2, c), dtype=torch.float32, device=dev)
        _lib.check(lib.ln_dice_forward(_lib.ptr(log_probs), _lib.ptr(target), n, points_per_cloud, c, ignore_index, _lib.ptr(ws), ws.numel(),
                                       _lib.ptr(loss), None, None, _lib.ptr(coef), _lib.stream_ptr(dev)), "ln_dice_forward")
        ctx.save_for_backward(log_probs, target, coef)
        ctx.points_per_cloud = points_per_cloud
        return loss[0]

    @staticmethod
    def backward(ctx, grad_loss):
        from . import _lib
        log_probs, target, coef = ctx.saved_tensors
        n, c = log_probs.shape
        g = grad_loss.contiguous().float()
        grad = torch.empty_like(log_probs)
        _lib.check(_lib.load().ln_dice_backward(_lib.ptr(log_probs), _lib.ptr(target), _lib.ptr(coef), _lib.ptr(g), n, ctx.points_per_cloud, c,
                                                _lib.ptr(grad), _lib.stream_ptr(g.device)), "ln_dice_backward")
        return grad, None, None, None


class _NllCloudsFunction(torch.autograd.Function):
    """csrc/ln_nll.hip: the class-weighted NLL of every cloud of a cloud-major batch and the mean over the clouds — two launches forward
    (the clouds' sums, each cut and added by the kernels that serve ln_nll_forward on a cloud's rows, then the mean in a fixed order), one backward
    that writes the whole [n, C] gradient.  weight None: every class 1.  points_per_cloud >= n: one cloud."""

    @staticmethod
    def forward(ctx, log_probs, target, ignore_index, weight, points_per_cloud):
        from . import _lib
        lib = _lib.load()
        lp = log_probs.contiguous()
        n, c = lp.shape
        dev = lp.device
        clouds = -(-n // points_per_cloud)
        ws = torch.empty((lib.ln_nll_clouds_workspace_bytes(n, points_per_cloud),), dtype=torch.uint8, device=dev)
        out = torch.empty((1 + 2 * clouds,), dtype=torch.float32, device=dev)  # loss, per_cloud [B], weight_sum [B]: one allocation, addressed
        p = out.data_ptr()
        _lib.check(lib.ln_nll_forward_clouds(_lib.ptr(lp), _lib.ptr(target), n, points_per_cloud, c, ignore_index,
                                             None if weight is None else _lib.ptr(weight), _lib.ptr(ws), ws.numel(), p, p + 4, p + 4 + 4 * clouds,
                                             _lib.stream_ptr(dev)), "ln_nll_forward_clouds")
        ctx.save_for_backward(target, out, weight)
        ctx.shape, ctx.ignore_index, ctx.points_per_cloud = (n, c), ignore_index, points_per_cloud
        return out[0]

    @staticmethod
    def backward(ctx, grad_loss):
        from . import _lib
        target, out, weight = ctx.saved_tensors
        n, c = ctx.shape
        g = grad_loss.contiguous().float()
        grad = torch.empty((n, c), dtype=torch.float32, device=g.device)
        _lib.check(_lib.load().ln_nll_backward_clouds(_lib.ptr(target), _lib.ptr(g), out.data_ptr() + 2 * (out.numel() + 1), n, ctx.points_per_cloud, c,
                                                      ctx.ignore_index, None if weight is None else _lib.ptr(weight), _lib.ptr(grad),
                                                      _lib.stream_ptr(g.device)), "ln_nll_backward_clouds")
        return grad, None, None, None, None


def log_softmax(logits: torch.Tensor) -> torch.Tensor:
    """torch.log_softmax(logits, 1) of [N, C] logits: the one place where the losses of this module turn logits into log-probabilities."""
    return torch.log_softmax(logits, 1)


def _nll_clouds_torch(log_probs, target, ignore_index, weight, points_per_cloud):
    """The formula of ln_nll_forward_clouds in torch operators: gather, `where`, sums over a [B, n0] view padded behind a shorter last
    cloud.  Shapes depend on sizes only and nothing is read back: any device, any float dtype, inside a stream capture."""
    n, c = log_probs.shape
    if n == 0:
        return log_probs.sum() * 0.0
    n0 = min(points_per_cloud, n)
    clouds = -(-n // n0)
    clamped = target.clamp(0, c - 1)
    picked = log_probs.gather(1, clamped.unsqueeze(1)).squeeze(1)
    zero = torch.zeros_like(picked)
    w = torch.ones_like(picked) if weight is None else weight.to(device=picked.device, dtype=picked.dtype)[clamped]
    if ignore_index is not None:
        keep = target != int(ignore_index)
        # (selected, not multiplied by a 0 / 1 mask: a -inf or NaN in an ignored row, or in the weight of a class that only ignored labels
        # carry, must reach neither the loss nor the gradient — w is selected first, so that the product's gradient is 0 * 0 there)
        w = torch.where(keep, w, zero)
        terms = torch.where(keep, w * picked, zero)
    else:
        terms = w * picked
    pad = clouds * n0 - n
    if pad:
        terms, w = torch.nn.functional.pad(terms, (0, pad)), torch.nn.functional.pad(w, (0, pad))
    weight_sum = w.reshape(clouds, n0).sum(1)
    per_cloud = -terms.reshape(clouds, n0).sum(1) / torch.where(weight_sum != 0, weight_sum, torch.ones_like(weight_sum))
    return per_cloud.sum() / clouds


def nll_loss_gather(log_probs: torch.Tensor, target: torch.Tensor, ignore_index=None, *, weight=None, points_per_cloud=None) -> torch.Tensor:
    """Mean negative log-likelihood, as torch.nn.NLLLoss(ignore_index=...) (ln_train.py:130).  float32 CUDA inputs take the fused
    kernels; everything else is written as gather + masked mean (torch's nll_loss kernels reduce a [120 k, C] input in a single
    workgroup: 0.14 ms forward, 0.09 ms backward on MI355X).

    weight ([C] class weights, torch.nn.NLLLoss(weight=): the loss is sum w[y_i] lp[i, y_i] / sum w[y_i]) and points_per_cloud (the
    [N, C] input is a cloud-major batch of ceil(N / n0) clouds, the last possibly shorter; the result is the MEAN OVER THE CLOUDS of
    each cloud's own loss, a cloud without a counted label contributing 0, as LovaszSoftmax(points_per_cloud=)) go through
    ln_nll_forward_clouds on float32 CUDA inputs while FUSED_NLL_CLOUDS is set, and through the torch form otherwise.  With both left at
    None nothing changes: the same Function, the same kernels, the same bits."""
    target = target.reshape(-1)
    if weight is not None or points_per_cloud is not None:
        if log_probs.dim() != 2 or target.shape[0] != log_probs.shape[0]:
            raise ValueError("nll_loss_gather(weight=, points_per_cloud=) expects [N, C] log-probabilities and N labels")
        n, c = log_probs.shape
        if weight is not None and weight.numel() != c:
            raise ValueError("weight: one value per class")
        n0 = max(n, 1) if points_per_cloud is None else int(points_per_cloud)
        if n0 < 1:
            raise ValueError("points_per_cloud >= 1")
        if FUSED_NLL_CLOUDS and log_probs.is_cuda and log_probs.dtype == torch.float32 and target.is_cuda and target.dtype == torch.int64 and \
                n > 0 and log_probs.numel() < _LOVASZ_MAX_ELEMENTS and _clouds_ok(n, n0):
            w = weight
            if w is not None and not (w.device == log_probs.device and w.dtype == torch.float32 and w.dim() == 1 and w.is_contiguous() and
                                      not w.requires_grad):  # (the buffer of NLLLoss on the model's device passes as it is)
                w = w.detach().to(device=log_probs.device, dtype=torch.float32).reshape(-1).contiguous()
            return _NllCloudsFunction.apply(log_probs, target.contiguous(), _label_or_none(ignore_index), w, n0)
        return _nll_clouds_torch(log_probs, target, ignore_index, None if weight is None else weight.detach().reshape(-1), n0)
    if FUSED_NLL and log_probs.is_cuda and log_probs.dtype == torch.float32 and log_probs.dim() == 2 and target.is_cuda and \
            target.dtype == torch.int64 and target.shape[0] == log_probs.shape[0] and log_probs.shape[0] > 0 and \
            log_probs.numel() < _LOVASZ_MAX_ELEMENTS:  # (the limit of ln_nll_forward; beyond it the torch form)
        return _NllFunction.apply(log_probs, target.contiguous(), _label_or_none(ignore_index))
    picked = log_probs.gather(1, target.clamp(0, log_probs.shape[1] - 1).unsqueeze(1)).squeeze(1)
    if ignore_index is None:
        return -picked.mean()
    keep = target != ignore_index
    # (selected, not multiplied by a 0 / 1 mask: the kernels never read an ignored row, so a -inf or NaN there must not reach the loss)
    return -torch.where(keep, picked, torch.zeros_like(picked)).sum() / keep.sum().clamp(min=1).to(picked.dtype)


class NLLLoss(torch.nn.Module):
    """torch.nn.NLLLoss(weight=, ignore_index=, reduction="mean") of the training step (ln_train.py:130) over log-probabilities [N, C],
    with the class weights of LNN.compute_class_weights and, for a batch of clouds in one lattice, per cloud.

    points_per_cloud=None: the loss of one cloud.  points_per_cloud=n0 (what Lattice.points_per_cloud() returns for a batch set up with
    set_cloud_batch): the rows are a cloud-major batch of ceil(N / n0) clouds of n0 points, the last possibly shorter, and the result
    is the MEAN OVER THE CLOUDS of each cloud's own loss  -sum w[y_i] lp[i, y_i] / sum w[y_i]  over the cloud's labels that differ from
    ignore_index — not the loss of the whole batch, in which a cloud with fewer ignored labels weighs more.  A cloud without a counted
    label contributes 0 and still counts in the mean, as in LovaszSoftmax(points_per_cloud=).  ignore_index=None ignores no label
    (torch's default is -100).  Labels outside [0, C) are clamped, as in nll_loss_gather.  With neither weight nor points_per_cloud this
    is nll_loss_gather(log_probs, target, ignore_index)."""

    def __init__(self, weight=None, ignore_index=None, points_per_cloud=None):
        super().__init__()
        self.register_buffer("weight", None if weight is None else torch.as_tensor(weight).detach().clone().reshape(-1))
        self.ignore_index = ignore_index
        self.points_per_cloud = _checked_points_per_cloud(points_per_cloud)

    def forward(self, log_probs: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if log_probs.dim() != 2:
            raise ValueError("NLLLoss expects [N, C] log-probabilities")
        return nll_loss_gather(log_probs, target, self.ignore_index, weight=self.weight, points_per_cloud=self.points_per_cloud)


class GeneralizedSoftDiceLoss(torch.nn.Module):
    """The alternative to Lovasz-Softmax that ln_train.py:127 keeps at hand (reference latticenet_py/lattice/diceloss.py:172-209):
    with p = exp(log_probs) [N, C] and labels [N], per class  dice_c = 2 sum_i p_ic [y_i = c] / (sum_i p_ic + #{y_i = c} + 1e-6);
    loss = sum_c w_c (1 - dice_c) / C with w = 1 except w[ignore_index] = 0 (the division keeps all C classes, as there).
    No one-hot matrix is built: the intersection is a gather + index_add over the labels.

    points_per_cloud=None: the loss of one cloud, the reference's.  points_per_cloud=n0 (what Lattice.points_per_cloud() returns for a
    batch set up with set_cloud_batch): the [N, C] input is a cloud-major batch of ceil(N / n0) clouds of n0 points, the last possibly
    shorter, and the result is the MEAN OVER THE CLOUDS of each cloud's own loss (a ratio of sums: not the loss of the whole batch).
    With FUSED_DICE set, float32 CUDA inputs within the limits of ln_dice_forward take the kernels of csrc/ln_dice.hip (bitwise
    reproducible; a label outside [0, C) belongs to no class there); everything else, and everything while the flag is off, the torch
    form, which faults on such a label as the reference does."""

    def __init__(self, p=1, smooth=1, reduction="mean", weight=1, ignore_index=None, points_per_cloud=None):
        super().__init__()
        self.p, self.smooth, self.reduction = p, smooth, reduction  # accepted and unused, as in the reference
        self.ignore_index = ignore_index
        self.points_per_cloud = _checked_points_per_cloud(points_per_cloud)

    def _forward_clouds_torch(self, output, target):
        """The single-cloud form batched as [B_full, C, n0] plus a [1, C, rest] term for a shorter last cloud; shapes depend on sizes
        only and nothing is read back: runs on the CPU and inside a stream capture."""
        n, c = output.shape
        n0 = min(self.points_per_cloud, max(n, 1))
        full, rest = divmod(n, n0)
        clouds = full + (1 if rest else 0)
        if clouds == 0:
            return output.sum() * 0.0
        total = None
        for lo, hi, b in ((0, full * n0, full), (full * n0, n, 1 if rest else 0)):
            if b == 0:
                continue
            probs = output[lo:hi].exp().reshape(b, (hi - lo) // b, c).transpose(1, 2)  # [b, C, points]
            labels = target[lo:hi].reshape(b, 1, (hi - lo) // b)
            picked = probs.gather(1, labels).squeeze(1)  # [b, points]
            intersection = torch.zeros((b, c), dtype=probs.dtype, device=probs.device).scatter_add_(1, labels.squeeze(1), picked)
            counts = torch.zeros((b, c), dtype=probs.dtype, device=probs.device).scatter_add_(1, labels.squeeze(1), torch.ones_like(picked))
            loss_per_class = 1.0 - 2.0 * intersection / (probs.sum(2) + counts + 1e-6)
            if self.ignore_index is not None:
                loss_per_class = loss_per_class * (torch.arange(c, device=probs.device) != int(self.ignore_index)).to(probs.dtype)
            per_cloud = loss_per_class.sum(1) / c
            total = per_cloud.sum() if total is None else total + per_cloud.sum()
        return total / clouds

    def forward(self, output: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        target = target.reshape(-1)
        if _dice_fused_ok(output, target) and _clouds_ok(output.shape[0], self.points_per_cloud):
            return _DiceFunction.apply(output, target.contiguous(), _label_or_none(self.ignore_index),
                                       output.shape[0] if self.points_per_cloud is None else self.points_per_cloud)
        if self.points_per_cloud is not None:
            if output.dim() != 2:
                raise ValueError("GeneralizedSoftDiceLoss(points_per_cloud=) expects [N, C] log-probabilities")
            return self._forward_clouds_torch(output, target)
        nr_classes = output.shape[1]
        probs = output.exp()
        picked = probs.gather(1, target.unsqueeze(1)).squeeze(1)
        intersection = torch.zeros(nr_classes, dtype=probs.dtype, device=probs.device).index_add_(0, target, picked)
        counts = torch.zeros(nr_classes, dtype=probs.dtype, device=probs.device).index_add_(0, target, torch.ones_like(picked))
        union = probs.sum(0) + counts
        loss_per_class = 1.0 - 2.0 * intersection / (union + 1e-6)
        if self.ignore_index is not None:
            weight = (torch.arange(nr_classes, device=probs.device) != int(self.ignore_index)).to(probs.dtype)
            loss_per_class = loss_per_class * weight
        return loss_per_class.sum() / nr_classes


def _lovasz_per_class(errors_sorted, order, onehot):
    """Class-major rows along the last axis ([C, N], or [B, C, n0] for a batch of clouds): the Jaccard gradient along each row's sorted
    order dotted with the sorted errors, and the rows' foreground counts."""
    fg_sorted = torch.gather(onehot, -1, order)
    # gradient of the Jaccard loss along the sorted order: J_k = 1 - (G - cumsum fg) / (G + cumsum (1 - fg))
    gts = fg_sorted.sum(-1, keepdim=True)
    intersection = gts - fg_sorted.cumsum(-1)
    union = gts + (1.0 - fg_sorted).cumsum(-1)
    jaccard = 1.0 - intersection / union
    grad = torch.cat((jaccard[..., :1], jaccard[..., 1:] - jaccard[..., :-1]), -1)
    return (errors_sorted * grad).sum(-1), gts.squeeze(-1)


class LovaszSoftmax(torch.nn.Module):
    """points_per_cloud=None: the loss of one cloud, the reference's.  points_per_cloud=n0 (what Lattice.points_per_cloud() returns for
    a batch set up with set_cloud_batch; reduction "mean" or "sum"): the [N, C] input is a cloud-major batch of ceil(N / n0) clouds of
    n0 points, the last possibly shorter, and the result is the MEAN OVER THE CLOUDS of each cloud's own loss — its own sort, its own
    Jaccard index, its own set of present classes.  The kernels (FUSED_LOVASZ) take at most 65 535 clouds, the limit of
    ln_lovasz_forward_clouds; a batch of more clouds is computed by the torch form, like every other input the kernels do not take."""

    def __init__(self, ignore_index, reduction: str = "mean", points_per_cloud=None):
        super().__init__()
        if points_per_cloud is not None and reduction not in ("mean", "sum"):
            raise ValueError("LovaszSoftmax(points_per_cloud=) needs reduction 'mean' or 'sum': the classes present differ from cloud to cloud")
        self.ignore_index = ignore_index
        self.reduction = reduction
        self.points_per_cloud = _checked_points_per_cloud(points_per_cloud)

    def _keep(self, c, device):
        """[C] mask of the classes that may count, or None (no host scalar: safe inside a stream capture)"""
        if self.ignore_index is not None and 0 <= int(self.ignore_index) < c:
            return torch.arange(c, device=device) != int(self.ignore_index)
        return None

    def _forward_clouds_torch(self, inputs, targets):
        """The [C, N] form batched as [B_full, C, n0] plus a [1, C, rest] term for a shorter last cloud; shapes depend on sizes only."""
        n, c = inputs.shape
        n0 = min(self.points_per_cloud, max(n, 1))
        full, rest = divmod(n, n0)
        clouds = full + (1 if rest else 0)
        if clouds == 0:
            return inputs.sum() * 0.0
        keep = self._keep(c, inputs.device)
        total = None
        for lo, hi, b in ((0, full * n0, full), (full * n0, n, 1 if rest else 0)):
            if b == 0:
                continue
            probs = inputs[lo:hi].exp().reshape(b, (hi - lo) // b, c).transpose(1, 2)  # [b, C, points]
            onehot = torch.zeros((hi - lo, c), dtype=probs.dtype, device=probs.device).scatter_(1, targets[lo:hi].clamp(0, c - 1).unsqueeze(1), 1.0)
            onehot = onehot.reshape(b, (hi - lo) // b, c).transpose(1, 2).contiguous()
            errors_sorted, order = torch.sort((onehot - probs).abs(), dim=2, descending=True)
            per_class, gts = _lovasz_per_class(errors_sorted, order, onehot)
            present = gts > 0
            if keep is not None:
                present = present & keep
            per_cloud = (per_class * present).sum(1)
            if self.reduction == "mean":
                per_cloud = per_cloud / present.sum(1).clamp(min=1)
            total = per_cloud.sum() if total is None else total + per_cloud.sum()
        return total / clouds

    def forward(self, inputs, targets):
        """inputs: log-probabilities [N, C] (the model's log-softmax, ln_train.py:156); targets: int64 [N]."""
        if inputs.dim() != 2:
            raise ValueError("LovaszSoftmax expects [N, C] log-probabilities")
        if self.points_per_cloud is not None:
            if self.reduction not in ("mean", "sum"):  # (also when it was reassigned after construction)
                raise ValueError("LovaszSoftmax(points_per_cloud=) needs reduction 'mean' or 'sum'")
            if _lovasz_fused_ok(inputs, targets) and _clouds_ok(inputs.shape[0], self.points_per_cloud):
                return _LovaszCloudsFunction.apply(inputs, targets.reshape(-1).contiguous(), _label_or_none(self.ignore_index),
                                                   0 if self.reduction == "mean" else 1, self.points_per_cloud)
            return self._forward_clouds_torch(inputs, targets.reshape(-1))
        if self.reduction in ("mean", "sum") and _lovasz_fused_ok(inputs, targets):
            # equal errors are ordered by point index and the Jaccard gradient is taken in closed form (csrc/ln_lovasz.hip)
            return _LovaszFunction.apply(inputs, targets.reshape(-1).contiguous(), _label_or_none(self.ignore_index),
                                         0 if self.reduction == "mean" else 1)
        probs = inputs.exp()
        n, c = probs.shape
        targets = targets.reshape(-1)
        onehot = torch.zeros((n, c), dtype=probs.dtype, device=probs.device).scatter_(1, targets.clamp(0, c - 1).unsqueeze(1), 1.0)
        # class-major [C, N] so that every class is one contiguous row: row-wise sort / cumsum are far faster than
        # column-wise ones on an [N, C] matrix
        onehot = onehot.t().contiguous()
        errors = (onehot - probs.t()).abs()
        if errors.is_cuda and torch.cuda.is_current_stream_capturing() and os.environ.get("LN_LOVASZ_ROW_SORT"):
            # (kept as a switch: for a while the captured [C, N] sort looked unsafe to replay — the faults were those of training loops
            # that joined replays and eager kernels across streams; on the capture stream the matrix sort replays fine)
            parts = [torch.sort(errors[k], descending=True) for k in range(c)]
            errors_sorted = torch.stack([p[0] for p in parts])
            order = torch.stack([p[1] for p in parts])
        else:
            errors_sorted, order = torch.sort(errors, dim=1, descending=True)
        per_class, gts = _lovasz_per_class(errors_sorted, order, onehot)
        present = gts > 0
        keep = self._keep(c, probs.device)
        if keep is not None:
            present = present & keep
        if self.reduction == "none":
            return per_class[present]
        total = (per_class * present).sum()
        if self.reduction == "sum":
            return total
        return total / present.sum().clamp(min=1)


class SegmentationLoss(torch.nn.Module):
    """The loss of the training step from LOGITS [N, C] (ln_train.py:128-158):
        lovasz_weight LovaszSoftmax(ignore_index)(lp, t) + nll_weight NLLLoss(weight=class_weight, ignore_index=)(lp, t),  lp = log_softmax(logits),
    points_per_cloud as in the two modules: the mean over the clouds of a cloud-major batch.  A loss whose weight is 0 is not computed.
    LovaszSoftmax and NLLLoss are composed over losses.log_softmax, so each takes its kernels wherever it does on its own; any device,
    any float dtype, inside a stream capture."""

    def __init__(self, ignore_index, lovasz_weight=0.5, nll_weight=0.5, class_weight=None, points_per_cloud=None):
        super().__init__()
        self.ignore_index = ignore_index
        self.lovasz_weight, self.nll_weight = float(lovasz_weight), float(nll_weight)
        self.points_per_cloud = _checked_points_per_cloud(points_per_cloud)
        self.lovasz = LovaszSoftmax(ignore_index, "mean", points_per_cloud=points_per_cloud)
        self.nll = NLLLoss(weight=class_weight, ignore_index=ignore_index, points_per_cloud=points_per_cloud)

    def forward(self, logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if logits.dim() != 2:
            raise ValueError("SegmentationLoss expects [N, C] logits")
        target = target.reshape(-1)
        lp = log_softmax(logits)
        total = None
        if self.lovasz_weight != 0:
            total = self.lovasz_weight * self.lovasz(lp, target)
        if self.nll_weight != 0:
            term = self.nll_weight * self.nll(lp, target)
            total = term if total is None else total + term
        return lp.sum() * 0.0 if total is None else total


class Scores:
    """Per-class intersection / union accumulated over clouds (callbacks/scores.py): IoU_c = I_c / U_c over the classes
    that occur (union > 0), mean over those.  Counts stay on the device; `all_reduce(dist)` sums them over ranks."""

    def __init__(self):
        self.clear()

    def clear(self):
        self.start_fresh_eval()
        self.best_iou = -99999999
        self.best_iou_dict = {}

    def start_fresh_eval(self):
        self.intersection_per_class = None
        self.union_per_class = None
        self.nr_classes = None

    def accumulate_scores(self, pred_softmax, gt, unlabeled_idx, points_per_cloud=None):
        """points_per_cloud=None: one cloud.  points_per_cloud=n0 (Lattice.points_per_cloud() of a batch set up with set_cloud_batch):
        the rows are a cloud-major batch of ceil(N / n0) clouds and every cloud is scored on its own — only the classes present in
        THAT cloud's ground truth count there, as when the clouds are handed over one by one.  No host synchronisation on float32
        CUDA scores (ln_iou_counts_clouds): usable inside a captured step."""
        c = pred_softmax.shape[1]
        gt = gt.detach().reshape(-1)
        if self.intersection_per_class is None:
            self.nr_classes = c
            self.intersection_per_class = torch.zeros(c, dtype=torch.int64, device=gt.device)
            self.union_per_class = torch.zeros(c, dtype=torch.int64, device=gt.device)
        if points_per_cloud is not None:
            self._accumulate_clouds(pred_softmax.detach(), gt, unlabeled_idx, int(points_per_cloud))
            return
        pred = pred_softmax.detach().argmax(1)
        hit = torch.bincount(gt[pred == gt], minlength=c)[:c]
        n_gt = torch.bincount(gt.clamp(0, c - 1), minlength=c)[:c]
        n_pred = torch.bincount(pred, minlength=c)[:c]
        in_gt = n_gt > 0  # the reference only scores the classes present in this cloud's ground truth
        if unlabeled_idx is not None and 0 <= int(unlabeled_idx) < c:
            in_gt[int(unlabeled_idx)] = False
        self.intersection_per_class += hit * in_gt
        self.union_per_class += (n_gt + n_pred - hit) * in_gt

    def _accumulate_clouds(self, scores, gt, unlabeled_idx, n0):
        if n0 < 1:
            raise ValueError("points_per_cloud >= 1")
        n, c = scores.shape
        clouds = -(-n // n0)
        if FUSED_IOU_COUNTS and scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 2 and gt.is_cuda and \
                gt.dtype == torch.int64 and gt.numel() == n and 1 <= c <= _LOVASZ_MAX_CLASSES and scores.numel() < _LOVASZ_MAX_ELEMENTS and \
                _clouds_ok(n, n0) and self.intersection_per_class.is_cuda:
            from . import _lib
            lib = _lib.load()
            scores, gt = scores.contiguous(), gt.contiguous()
            ws = torch.empty((lib.ln_iou_counts_clouds_workspace_bytes(n, n0, c),), dtype=torch.uint8, device=scores.device)
            _lib.check(lib.ln_iou_counts_clouds(_lib.ptr(scores), _lib.ptr(gt), n, n0, c, -1 if unlabeled_idx is None else int(unlabeled_idx),
                                                _lib.ptr(ws), ws.numel(), _lib.ptr(self.intersection_per_class), _lib.ptr(self.union_per_class),
                                                _lib.stream_ptr(scores.device)), "ln_iou_counts_clouds")
            return
        if n == 0:
            return
        # per-cloud histograms through the offset label cloud * C + class; a miss goes to a bin of its own (no boolean-mask index)
        pred = scores.argmax(1)
        base = (torch.arange(n, device=gt.device) // n0) * c
        ones = torch.ones(n, dtype=torch.int64, device=gt.device)

        def hist(idx):
            return torch.zeros(clouds * c + 1, dtype=torch.int64, device=gt.device).scatter_add_(0, idx, ones)[:clouds * c].view(clouds, c)

        hit = hist(torch.where(pred == gt, base + pred, torch.full_like(base, clouds * c)))
        n_gt = hist(base + gt.clamp(0, c - 1))
        n_pred = hist(base + pred)
        in_gt = n_gt > 0
        if unlabeled_idx is not None and 0 <= int(unlabeled_idx) < c:
            in_gt = in_gt & (torch.arange(c, device=gt.device) != int(unlabeled_idx))
        self.intersection_per_class += (hit * in_gt).sum(0)
        self.union_per_class += ((n_gt + n_pred - hit) * in_gt).sum(0)

    def all_reduce(self, dist):
        if dist is not None and self.intersection_per_class is not None:
            dist.all_reduce(self.intersection_per_class, op=dist.ReduceOp.SUM)
            dist.all_reduce(self.union_per_class, op=dist.ReduceOp.SUM)

    def compute_stats(self, print_per_class_iou=False):
        inter = self.intersection_per_class.tolist()
        union = self.union_per_class.tolist()
        iou_dict = {i: inter[i] / union[i] for i in range(self.nr_classes) if union[i] > 0}
        if print_per_class_iou:
            for i, v in iou_dict.items():
                print("class iou for idx", i, " is ", v)
        avg = sum(iou_dict.values()) / max(len(iou_dict), 1)
        return avg, iou_dict

    def avg_class_iou(self, print_per_class_iou=False):
        return self.compute_stats(print_per_class_iou)[0]

    def iou_per_class(self, print_per_class_iou=False):
        return self.compute_stats(print_per_class_iou)[1]

    def update_best(self):
        avg, d = self.compute_stats()
        if avg > self.best_iou:
            self.best_iou, self.best_iou_dict = avg, d
