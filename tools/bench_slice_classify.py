#!/usr/bin/env python3
"""Kernel time of the fused slice + classifier head (forward, backward) at the SemanticKITTI LNN shape.
Usage: python tools/bench_slice_classify.py [--f16] [points] [val_dim] [classes]

--f16: times ln_slice_classify_forward / _backward and their _f16 forms through the C ABI on the same tokens and the same values
(fp16, and those widened), alternating the four calls window by window: 15 windows of 500 calls each per call, device events around
each window, median and range of the per-call time over the windows."""
import ctypes as C, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lattice_net_amd as L
from lattice_net_amd import synthetic
lib = L.load_library()
dev = torch.device("cuda", 0)
F16 = "--f16" in sys.argv
sys.argv = [a for a in sys.argv if a != "--f16"]
n = int(sys.argv[1]) if len(sys.argv) > 1 else 120000
v = int(sys.argv[2]) if len(sys.argv) > 2 else 96
c = int(sys.argv[3]) if len(sys.argv) > 3 else 20
pos = torch.from_numpy(synthetic.lidar_cloud(n, 0)).to(dev)
lat = L.Lattice(sigmas=[0.9] * 3, capacity=100000, device=dev)
lat.begin_splat()
idx, w = lat.just_create_verts(pos, True)
m = lat.nr_lattice_vertices()
vals = torch.randn((m, v), device=dev, requires_grad=True)
dw = (torch.randn((n, 4), device=dev) * 0.01).requires_grad_(True)
lw = torch.randn((c, v), device=dev, requires_grad=True)
lb = torch.zeros((c,), device=dev, requires_grad=True)
g = torch.randn((n, c), device=dev)
if F16:
    from lattice_net_amd import _lib
    st = _lib.stream_ptr(dev)
    v16 = vals.detach().half()
    v32 = v16.float()
    logits = torch.empty((n, c), device=dev)
    gdw, glw, glb = torch.zeros((n, 4), device=dev), torch.zeros((c, v), device=dev), torch.zeros((c,), device=dev)
    gs, weff = torch.empty((n, v), device=dev), torch.empty((n * 4,), device=dev)
    ws = torch.empty((lib.ln_slice_classify_backward_workspace_bytes(n, 3, v, c),), dtype=torch.uint8, device=dev)
    p = lambda t: t.data_ptr()
    def fwd(fn, x):
        return lambda: _lib.check(fn(p(x), p(dw), p(lw), p(lb), p(idx), p(w), n, 3, v, c, p(logits), st), "forward")
    def bwd(fn, x):
        return lambda: _lib.check(fn(p(g), p(x), p(dw), p(lw), p(idx), p(w), n, 3, v, c, None, p(gdw), p(glw), p(glb), p(gs), p(weff), p(ws),
                                     ws.numel(), st), "backward")
    calls = {"forward fp32": fwd(lib.ln_slice_classify_forward, v32), "forward fp16": fwd(lib.ln_slice_classify_forward_f16, v16),
             "backward fp32": bwd(lib.ln_slice_classify_backward, v32), "backward fp16": bwd(lib.ln_slice_classify_backward_f16, v16)}
    WINDOWS, CALLS = 15, 500
    for f in calls.values():
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(WINDOWS):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / CALLS * 1e3)
    print(f"n={n} V={v} C={c} m={m}: per-call time over {WINDOWS} windows of {CALLS} calls, us")
    for k, t in times.items():
        print(f"{k:14s} median {np.median(t):7.1f}  range {min(t):7.1f} .. {max(t):7.1f}")
    sys.exit(0)
def step():
    for t in (vals, dw, lw, lb):
        t.grad = None
    L.SliceClassifyLattice.apply(vals, lat, pos, dw, lw, lb, c, idx, w).backward(g)
for _ in range(3):
    step()
for k in ("k_slice_classify_forward", "k_slice_classify_backward", "k_sc_reduce_slabs", "k_csr_reduce_segments"):
    lib.ln_profile_begin(k.encode(), 64)
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    ms, cnt = C.c_double(0.0), C.c_int(0)
    lib.ln_profile_end(C.byref(ms), C.byref(cnt))
    print(f"{k:28s} {ms.value / max(cnt.value, 1) * 1e3:7.1f} us x{cnt.value // 5}")
