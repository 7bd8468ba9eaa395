"""The Lovasz-Softmax kernels (csrc/ln_lovasz.hip) against the fp64 reference and the counted bounds of tests/lovasz_reference.py,
through the C ABI (ln_lovasz_forward / ln_lovasz_backward) and through losses.LovaszSoftmax."""
import ctypes as C

import numpy as np
import pytest
import torch

from . import lovasz_reference as R

pytestmark = pytest.mark.gpu

TILE = R.LN_LV_TILE
SIZES = [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 903]
NO_LABEL = -(1 << 62)


@pytest.fixture(autouse=True)
def fused_lovasz(monkeypatch):
    """LovaszSoftmax takes the kernels here whatever the module's default is."""
    from lattice_net_amd import losses
    monkeypatch.setattr(losses, "FUSED_LOVASZ", True)


def dev():
    return torch.device("cuda", 0)


def _lib():
    from lattice_net_amd import _lib
    return _lib, _lib.load()


def forward_abi(lp, y, ignore, red, with_per_class=True):
    """(loss, per_class or None, dloss_dlogp) as NumPy, and the device tensor of dloss_dlogp."""
    L, lib = _lib()
    n, c = lp.shape
    x = torch.from_numpy(np.ascontiguousarray(lp)).to(dev())
    t = torch.from_numpy(np.ascontiguousarray(y)).to(dev())
    ws = torch.empty((lib.ln_lovasz_workspace_bytes(n, c),), dtype=torch.uint8, device=dev())
    loss = torch.full((1,), float("nan"), device=dev())
    pc = torch.full((c,), float("nan"), device=dev()) if with_per_class else None
    dl = torch.full((n, c), float("nan"), device=dev())
    L.check(lib.ln_lovasz_forward(L.ptr(x), L.ptr(t), n, c, NO_LABEL if ignore is None else ignore, 0 if red == "mean" else 1, L.ptr(ws),
                                  ws.numel(), L.ptr(loss), L.ptr(pc), L.ptr(dl), L.stream_ptr(dev())), "ln_lovasz_forward")
    torch.cuda.synchronize()
    return (loss.cpu().numpy()[0], None if pc is None else pc.cpu().numpy(), dl.cpu().numpy()), dl


def forward_module(lp, y, ignore, red, grad_scale=1.0):
    from lattice_net_amd import losses
    assert losses.FUSED_LOVASZ
    x = torch.from_numpy(np.ascontiguousarray(lp)).to(dev()).requires_grad_(True)
    loss = losses.LovaszSoftmax(ignore_index=ignore, reduction=red)(x, torch.from_numpy(y).to(dev()))
    (loss * grad_scale).backward()
    return loss.detach().cpu().numpy(), None, x.grad.cpu().numpy()


CASES = (  # classes, ignore_index, reduction, per_class given, labels outside [0, C)
    (1, None, "mean", True, False),
    (2, 0, "sum", False, False),
    (3, 7, "mean", True, True),      # ignore_index out of range
    (20, 0, "mean", True, False),
    (20, 19, "sum", False, True),
)


@pytest.mark.parametrize("n", SIZES)
def test_separated_errors_value_and_gradient(n):
    worst = np.zeros(3)
    for c, ignore, red, with_pc, oor in CASES:
        y = R.labels(n, c, n + c, out_of_range=oor)
        lp = R.separated(n, c, 11 * n + c)
        # a condition of the test: the errors of a class are far enough apart that fp32 and fp64 must order them alike
        assert n == 1 or R.separation(lp, y) >= 0.25 / (n + 1) > 2.0 ** -20
        got, _ = forward_abi(lp, y, ignore, red, with_pc)
        worst = np.maximum(worst, R.check(got, lp, y, ignore, red, f"C ABI n={n} c={c}"))
        via_module = forward_module(lp, y, ignore, red)
        R.check(via_module, lp, y, ignore, red, f"LovaszSoftmax n={n} c={c}", r_grad=R.R_GRAD_BACKWARD)
        assert via_module[0] == got[0], "LovaszSoftmax did not take the kernels"
    print(f"\n[lovasz gpu] n={n}: worst error/bound loss {worst[0]:.3f} per class {worst[1]:.3f} gradient {worst[2]:.3f}")


def test_absent_class_single_class_and_ignored_class():
    n, c = 2 * TILE + 903, 3
    lp = R.separated(n, c, 5)
    for y, ignore, what in ((R.labels(n, c, 1, absent=1), 0, "class 1 absent"), (R.labels(n, c, 1, all_one=2), None, "all points in class 2"),
                            (R.labels(n, c, 1, all_one=0), 0, "all points in the ignore class")):
        for red in ("mean", "sum"):
            got, _ = forward_abi(lp, y, ignore, red)
            R.check(got, lp, y, ignore, red, what)
            R.check(forward_module(lp, y, ignore, red), lp, y, ignore, red, what + " (module)", r_grad=R.R_GRAD_BACKWARD)
    got, _ = forward_abi(lp, R.labels(n, c, 1, all_one=0), 0, "mean")
    assert got[0] == 0.0 and not got[1].any() and not got[2].any()  # no class counts: loss 0, gradient 0


@pytest.mark.parametrize("mode", ["right", "wrong", "mixed"])
def test_exact_ties_follow_the_point_index(mode):
    for n, c in ((1, 2), (65, 3), (TILE + 1, 3), (2 * TILE + 903, 20)):
        lp, y = R.ties(n, c, n, mode)
        for red in ("mean", "sum"):
            got, _ = forward_abi(lp, y, 0, red)
            R.check(got, lp, y, 0, red, f"ties {mode} n={n} c={c} {red}")
        R.check(forward_module(lp, y, None, "mean"), lp, y, None, "mean", f"ties {mode} n={n} c={c} (module)", r_grad=R.R_GRAD_BACKWARD)


def test_softmax_of_random_logits_loss_value():
    for n, c in ((65, 3), (2 * TILE + 903, 20)):
        lp, y = R.softmax_random(n, c, n), R.labels(n, c, 3)
        for red in ("mean", "sum"):
            got, _ = forward_abi(lp, y, 0, red)
            R.check(got, lp, y, 0, red, f"softmax n={n} c={c}", gradient=False)


def test_backward_scales_by_grad_loss():
    L, lib = _lib()
    n, c = TILE + 1, 3
    lp, y = R.separated(n, c, 8), R.labels(n, c, 8)
    scale = float(np.float32(-0.37))
    _, dl = forward_abi(lp, y, 0, "mean")
    g = torch.tensor([scale], device=dev())
    out = torch.full((n, c), float("nan"), device=dev())
    L.check(lib.ln_lovasz_backward(L.ptr(dl), L.ptr(g), n, c, L.ptr(out), L.stream_ptr(dev())), "ln_lovasz_backward")
    _, _, ref_grad = R.reference(lp, y, 0, "mean")
    assert R.worst_ratio(out.cpu().numpy(), ref_grad * scale, R.grad_bound(ref_grad * scale, R.R_GRAD_BACKWARD)) <= 1.0
    assert torch.equal(out, dl * scale)
    got = forward_module(lp, y, 0, "mean", grad_scale=scale)
    R.check(got, lp, y, 0, "mean", "module, grad_loss != 1", r_grad=R.R_GRAD_BACKWARD, grad_scale=scale)


def test_two_runs_are_bitwise_equal():
    n, c = 2 * TILE + 903, 20
    lp, y = R.softmax_random(n, c, 1), R.labels(n, c, 1)
    a, _ = forward_abi(lp, y, 0, "mean")
    b, _ = forward_abi(lp, y, 0, "mean")
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    ga, gb = forward_module(lp, y, 0, "mean", 0.5), forward_module(lp, y, 0, "mean", 0.5)
    assert ga[0].tobytes() == gb[0].tobytes() and ga[2].tobytes() == gb[2].tobytes()


def test_captured_lovasz_plus_nll_step_replays_bitwise():
    """0.5 Lovasz + 0.5 NLL (ln_train.py:156-158), forward and backward, captured on one stream and replayed on fresh inputs."""
    from lattice_net_amd.losses import LovaszSoftmax, nll_loss_gather
    n, c = 2 * TILE + 903, 20
    inputs = [(R.softmax_random(n, c, s), R.labels(n, c, s)) for s in (0, 1, 2)]
    lov = LovaszSoftmax(ignore_index=0)
    x = torch.from_numpy(inputs[0][0]).to(dev()).requires_grad_(True)
    t = torch.from_numpy(inputs[0][1]).to(dev())
    st = {}

    def step(xx, tt):
        loss = 0.5 * lov(xx, tt) + 0.5 * nll_loss_gather(xx, tt, ignore_index=0)
        grad, = torch.autograd.grad(loss, xx)
        return loss.detach(), grad

    eager = []
    for lp, y in inputs:
        eager.append(step(torch.from_numpy(lp).to(dev()).requires_grad_(True), torch.from_numpy(y).to(dev())))
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
    """Return code of `call()` and the number of kernel launches of the library it made."""
    _, lib = _lib()
    assert lib.ln_profile_begin(b"*", 64) == 0
    rc = call()
    ms, count = C.c_double(), C.c_int()
    assert lib.ln_profile_end(C.byref(ms), C.byref(count)) == 0
    return rc, count.value


def test_argument_errors_launch_nothing():
    L, lib = _lib()
    n, c = 65, 3
    x = torch.zeros((n, c), device=dev())
    t = torch.zeros((n,), dtype=torch.int64, device=dev())
    need = lib.ln_lovasz_workspace_bytes(n, c)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev())
    loss = torch.full((1,), 7.0, device=dev())
    dl = torch.full((n, c), 7.0, device=dev())
    sp = L.stream_ptr(dev())

    def fwd(nn, cc, ws_bytes):
        return lambda: lib.ln_lovasz_forward(L.ptr(x), L.ptr(t), nn, cc, 0, 0, L.ptr(ws), ws_bytes, L.ptr(loss), None, L.ptr(dl), sp)

    for call, text in ((fwd(n, c, need - 1), b"workspace"), (fwd(n, 0, need), b"bad sizes"), (fwd(n, 1025, need), b"bad sizes"),
                       (fwd((1 << 31) // c + 1, c, need), b"2^31"), (fwd(-1, c, need), b"bad sizes"),
                       (lambda: lib.ln_lovasz_forward(L.ptr(x), L.ptr(t), n, c, 0, 2, L.ptr(ws), need, L.ptr(loss), None, L.ptr(dl), sp), b"reduction"),
                       (lambda: lib.ln_lovasz_backward(L.ptr(dl), L.ptr(loss), (1 << 31) // c + 1, c, L.ptr(dl), sp), b"bad sizes")):
        rc, launches = _launches(call)
        assert rc == -1 and launches == 0 and text in lib.ln_last_error_string(), (rc, launches, lib.ln_last_error_string())
    torch.cuda.synchronize()
    assert float(loss[0]) == 7.0 and bool((dl == 7.0).all())
    rc, launches = _launches(fwd(n, c, need))  # and the good call does launch
    assert rc == 0 and launches >= 5
    rc, _ = _launches(fwd(0, c, need))  # no points: loss 0
    torch.cuda.synchronize()
    assert rc == 0 and float(loss[0]) == 0.0


def test_workspace_size_is_a_total_host_function_and_kernels_are_listed():
    _, lib = _lib()
    for n in (0, 1, 2047, 2048, 2049, 120000, (1 << 31) - 1):
        for c in (0, 1, 3, 20, 1024):
            assert lib.ln_lovasz_workspace_bytes(n, c) >= 256 + 16 * n * c
    names = lib.ln_kernel_names().decode().split(",")
    for k in ("k_lovasz_keys", "k_lovasz_hist", "k_lovasz_scan", "k_lovasz_scatter", "k_lovasz_fg_count", "k_lovasz_dot", "k_lovasz_finish",
              "k_lovasz_backward"):
        assert k in names


def test_other_inputs_keep_the_torch_form():
    from lattice_net_amd import losses
    n, c = 65, 3
    lp, y = R.softmax_random(n, c, 2), R.labels(n, c, 2)
    x64 = torch.from_numpy(lp).double().to(dev())
    t = torch.from_numpy(y).to(dev())
    ref_loss, ref_pc, _ = R.reference(lp, y, 0, "mean")
    assert abs(float(losses.LovaszSoftmax(0)(x64, t)) - ref_loss) < 1e-12  # float64: torch form
    none = losses.LovaszSoftmax(0, reduction="none")(x64.float(), t)          # data-dependent shape: torch form
    assert none.shape[0] == int((ref_pc > 0).sum())
