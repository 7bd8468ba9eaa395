"""fp64 reference of the training head from logits, for losses.SegmentationLoss (test_head_reference.py): per row of [n, C]
    log-softmax            lp[c] = (x[c] - m) - log(sum_c exp(x[c] - m)),  m = max_c x[c]
    its backward           dx[c] = g[c] - exp(lp[c]) sum_c g[c]
and inputs.  The Lovasz and NLL halves are those of lovasz_reference.py and nll_clouds_reference.py."""
import numpy as np


def f64(a):
    return np.asarray(a, dtype=np.float64)


def forward_reference(x):
    """lp in fp64; a row without a finite maximum, or with a NaN, is a row of NaN (torch.log_softmax's result)."""
    x = f64(x)
    with np.errstate(all="ignore"):
        m = np.max(x, axis=1, keepdims=True)
        d = x - m
        lp = d - np.log(np.exp(d).sum(1, keepdims=True))
    lp[~np.isfinite(m[:, 0]) | np.isnan(x).any(1)] = np.nan
    return lp


def backward_reference(lp, g):
    lp, g = f64(lp), f64(g)
    return g - np.exp(lp) * g.sum(1, keepdims=True)


def logits_case(n, c, seed, spread=4.0):
    return (np.random.default_rng(seed).standard_normal((n, c)) * spread).astype(np.float32)


def labels_case(n, c, seed, ignore_index=None, share=0.3):
    rng = np.random.default_rng(seed + 17)
    y = rng.integers(0, c, n).astype(np.int64)
    if ignore_index is not None:
        y[rng.random(n) < share] = ignore_index
    return y


def weights_case(c, seed):
    """class weights with a zero and a large one among them"""
    w = (0.25 + np.random.default_rng(seed + 5).random(c) * 4.0).astype(np.float32)
    if c >= 3:
        w[1] = 0.0
        w[2] = 20.5
    return w
