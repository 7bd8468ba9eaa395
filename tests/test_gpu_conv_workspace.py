"""Degraded-workspace paths of the convolution plan (csrc/ln_conv_plan.h) on the GPU: ln_conv_forward_ws with the queried workspace,
with none, with one byte less than queried, and with sentinel bytes behind the queried size; ln_linear_backward with grad_x null
and non-null (the filter gradient's slab sum rides in the grad_x convolution's bank split, or is launched on its own);
ln_conv_backward in each of its forms inside exactly ln_conv_backward_workspace_bytes.
4500 rows: the smallest lattices above LN_CONV_B3_MIN_ROWS, where 128 channels take the wide form with its slots split.  Operands
are small integers, so every form (fp32, bf16x3, split slots + partial sums) is exact and the outputs are compared bit for bit."""
import numpy as np
import pytest
import torch

from lattice_net_amd import _lib

pytestmark = pytest.mark.gpu
M, E = 4500, 9
SENTINEL = 0xA5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _workspaces(q):
    """(buffer, bytes passed, bytes of the buffer the call may touch) for: queried, none, one byte short, queried + sentinels"""
    def buf(n):
        return torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")
    return [("queried", buf(q), q), ("none", None, 0), ("one byte short", buf(q), q - 1), ("sentinels", buf(q + 4096), q)]


@pytest.fixture(scope="module")
def nbr():
    rng = np.random.default_rng(5)
    n = rng.integers(-1, M, (M, E)).astype(np.int32)  # -1: absent neighbour
    n[:, E - 1] = np.arange(M)
    return n


@pytest.mark.parametrize("v,f", [(128, 128), (64, 64)])
def test_conv_forward_is_exact_with_any_workspace(nbr, v, f):
    lib = _lib.load()
    rng = np.random.default_rng(v + f)
    vals = rng.integers(-3, 4, (M, v)).astype(np.float32)
    W = rng.integers(-2, 3, (E * v, f)).astype(np.float32)
    rows = np.where(nbr[:, :, None] >= 0, vals[np.maximum(nbr, 0)], 0.0).reshape(M, E * v).astype(np.float64)
    want = rows @ W.astype(np.float64)  # integers below 2^24: exact in fp64 and in fp32
    assert float(np.max(np.abs(want))) < 2 ** 24
    d_nbr, d_vals, d_W = _dev(nbr), _dev(vals), _dev(W)
    q = lib.ln_conv_forward_workspace_bytes(M, E, v, f)
    for name, ws, nbytes in _workspaces(q):
        out = torch.full((M, f), float("nan"), device="cuda")
        rc = lib.ln_conv_forward_ws(_lib.ptr(d_nbr), _lib.ptr(d_vals), _lib.ptr(d_W), M, E, v, f, 0, _lib.ptr(out), _lib.ptr(ws), nbytes, None, None)
        torch.cuda.synchronize()
        assert rc == 0, (name, lib.ln_last_error_string())
        assert np.array_equal(out.cpu().numpy().astype(np.float64), want), name
        if ws is not None:
            assert bool((ws[nbytes:] == SENTINEL).all()), f"{name}: bytes behind the workspace were written"


@pytest.mark.parametrize("cin,cout", [(128, 128), (64, 64)])
@pytest.mark.parametrize("with_grad_x", [False, True])
def test_linear_backward_is_exact_whether_the_slab_sum_rides_or_not(cin, cout, with_grad_x):
    lib = _lib.load()
    rng = np.random.default_rng(cin + 2 * cout + with_grad_x)
    x = rng.integers(-3, 4, (M, cin)).astype(np.float32)
    gy = rng.integers(-3, 4, (M, cout)).astype(np.float32)
    w = rng.integers(-2, 3, (cout, cin)).astype(np.float32)
    want_w = gy.astype(np.float64).T @ x.astype(np.float64)
    want_x = gy.astype(np.float64) @ w.astype(np.float64)
    assert float(np.max(np.abs(want_w))) < 2 ** 24
    ident = _dev(np.arange(M, dtype=np.int32).reshape(M, 1))
    d_x, d_gy, d_w = _dev(x), _dev(gy), _dev(w)
    q = lib.ln_linear_backward_workspace_bytes(M, cin, cout)
    for name, ws, nbytes in _workspaces(q):
        gx = torch.full((M, cin), float("nan"), device="cuda") if with_grad_x else None
        gw = torch.full((cout, cin), float("nan"), device="cuda")
        rc = lib.ln_linear_backward(_lib.ptr(ident), _lib.ptr(d_x), _lib.ptr(d_gy), _lib.ptr(d_w), M, cin, cout, _lib.ptr(gx), _lib.ptr(gw),
                                    _lib.ptr(ws), nbytes, None)
        torch.cuda.synchronize()
        if nbytes < q:  # this call requires its workspace: an error, and nothing launched
            assert rc == -4, name
            assert bool(torch.isnan(gw).all()), name
            continue
        assert rc == 0, (name, lib.ln_last_error_string())
        assert np.array_equal(gw.cpu().numpy().astype(np.float64), want_w), name
        if with_grad_x:
            assert np.array_equal(gx.cpu().numpy().astype(np.float64), want_x), name
        assert bool((ws[nbytes:] == SENTINEL).all()), f"{name}: bytes behind the workspace were written"


def _symmetric_list(m, rng):
    """Neighbour list of one lattice: nbr(a, e) = b  <=>  nbr(b, e ^ 1) = a, some neighbours absent, the centre in the last slot"""
    n = np.full((m, E), -1, np.int32)
    for e in range(0, E - 1, 2):
        to = rng.permutation(m).astype(np.int32)
        have = rng.random(m) < 0.8
        n[have, e] = to[have]
        n[to[have], e + 1] = np.nonzero(have)[0]
    n[:, E - 1] = np.arange(m)
    return n


def _random_list(rows, into, rng):
    n = rng.integers(-1, into, (rows, E)).astype(np.int32)
    n[:, E - 1] = np.minimum(np.arange(rows), into - 1)
    return n


# one shape per LnBwdForm (csrc/ln_conv_plan.h; which form a shape takes is ln_conv_backward_plan's answer, asked through
# tests/cabi/conv_plan_check.cpp's header): fused = same list, 32 -> 32; full sum = a bank that fits LDS whole, two lattices; two calls =
# 128 -> 128 at few rows, where the value-gradient convolution splits over the filter slots and parks its slabs behind the filter
# gradient's
@pytest.mark.parametrize("form,mq,mn,v,f", [("fused", 1000, 1000, 32, 32), ("full sum", 1500, 1100, 32, 16), ("two calls", 700, 650, 128, 128)])
def test_conv_backward_is_exact_inside_its_queried_workspace(form, mq, mn, v, f):
    lib = _lib.load()
    rng = np.random.default_rng(mq + v + f)
    if form == "fused":
        nbr_q = nbr_n = _symmetric_list(mq, rng)
    else:
        nbr_q, nbr_n = _random_list(mq, mn, rng), _random_list(mn, mq, rng)
    vals = rng.integers(-3, 4, (mn, v)).astype(np.float32)
    G = rng.integers(-3, 4, (mq, f)).astype(np.float32)
    W = rng.integers(-2, 3, (E * v, f)).astype(np.float32)
    rows = np.where(nbr_q[:, :, None] >= 0, vals[np.maximum(nbr_q, 0)], 0.0).reshape(mq, E * v).astype(np.float64)
    want_w = rows.T @ G.astype(np.float64)
    flip = [e ^ 1 for e in range(E - 1)] + [E - 1]
    nf = nbr_n[:, flip]
    g_rows = np.where(nf[:, :, None] >= 0, G[np.maximum(nf, 0)], 0.0).astype(np.float64)  # [mn, E, f]
    want_v = np.einsum("nef,evf->nv", g_rows, W.astype(np.float64).reshape(E, v, f))
    assert max(float(np.max(np.abs(want_w))), float(np.max(np.abs(want_v)))) < 2 ** 24  # integers: exact in fp64 and in fp32
    d_q = _dev(nbr_q)
    d_n = d_q if nbr_n is nbr_q else _dev(nbr_n)
    d_vals, d_G, d_W = _dev(vals), _dev(G), _dev(W)
    q = lib.ln_conv_backward_workspace_bytes(mq, mn, E, v, f)
    ws = torch.full((q + 4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    gv = torch.full((mn, v), float("nan"), device="cuda")
    gw = torch.full((E * v, f), float("nan"), device="cuda")
    rc = lib.ln_conv_backward(_lib.ptr(d_q), _lib.ptr(d_n), _lib.ptr(d_vals), _lib.ptr(d_G), _lib.ptr(d_W), mq, mn, E, v, f, _lib.ptr(gv),
                              _lib.ptr(gw), _lib.ptr(ws), q, None, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.ln_last_error_string()
    assert bool((ws[q:] == SENTINEL).all()), "bytes behind the workspace were written"
    assert np.array_equal(gw.cpu().numpy().astype(np.float64), want_w)
    assert np.array_equal(gv.cpu().numpy().astype(np.float64), want_v)
