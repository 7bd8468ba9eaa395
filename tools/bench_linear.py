#!/usr/bin/env python3
"""Per-shape timing of the streaming linear (+LeakyReLU) kernels of csrc/ln_mlp.hip: forward, backward (x and w parts via
the library's own per-kernel event hooks).  Usage: python tools/bench_linear.py

python tools/bench_linear.py --f16: forward + backward of the per-vertex linear layer on fp16 rows (ln_linear_forward_f16 +
ln_linear_backward_f16, csrc/ln_linear_f16.hip) through the C ABI at the rows and widths of the bottlenecks of the SemanticKITTI network
(contract and expand of each level), against the fp32 path on the same shapes (ln_conv_forward_ws over the identity list +
ln_linear_backward).  Windows of 20 forward + backward pairs, the two paths alternating, nine windows each: median and fastest -
slowest window per path.  No ratio is asserted: these launches may be bound by latency."""
import ctypes as C, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lattice_net_amd as L
from lattice_net_amd import _lib
from lattice_net_amd.lattice_modules import LinearLeakyReluFunction, LinearMfmaFunction, _MFMA_LINEAR_WIDTHS
lib = L.load_library()
dev = torch.device("cuda", 0)


def bench_f16(windows=9, iters=20):
    shapes = [(46538, 32, 8), (46538, 8, 32), (11407, 64, 16), (11407, 16, 64), (2577, 128, 32), (2577, 32, 128)]
    p = _lib.ptr
    for rows, cin, cout in shapes:
        x32, w, g32 = torch.randn((rows, cin), device=dev), torch.randn((cout, cin), device=dev) / cin ** 0.5, torch.randn((rows, cout), device=dev)
        x16, g16 = x32.half(), g32.half()
        y16, gx16 = torch.empty((rows, cout), dtype=torch.float16, device=dev), torch.empty((rows, cin), dtype=torch.float16, device=dev)
        y32, gx32, gw = torch.empty((rows, cout), device=dev), torch.empty((rows, cin), device=dev), torch.empty((cout, cin), device=dev)
        ident = torch.arange(rows, dtype=torch.int32, device=dev).unsqueeze(1)
        ws16 = torch.empty((lib.ln_linear_backward_f16_workspace_bytes(rows, cin, cout),), dtype=torch.uint8, device=dev)
        wsf = torch.empty((max(int(lib.ln_conv_forward_workspace_bytes(rows, 1, cin, cout)), 256),), dtype=torch.uint8, device=dev)
        wsb = torch.empty((lib.ln_linear_backward_workspace_bytes(rows, cin, cout),), dtype=torch.uint8, device=dev)

        def f16():
            return (lib.ln_linear_forward_f16(p(x16), p(w), None, None, rows, cin, cout, p(y16), None) or
                    lib.ln_linear_backward_f16(p(x16), p(g16), p(w), rows, cin, cout, p(gx16), p(gw), None, p(ws16), ws16.numel(), None))

        def f32():
            return (lib.ln_conv_forward_ws(p(ident), p(x32), p(w), rows, 1, cin, cout, 2, p(y32), p(wsf), wsf.numel(), None, None) or
                    lib.ln_linear_backward(p(ident), p(x32), p(g32), p(w), rows, cin, cout, p(gx32), p(gw), p(wsb), wsb.numel(), None))

        paths = {"fp16": f16, "fp32": f32}
        for name in list(paths):
            rc = paths[name]()
            torch.cuda.synchronize()
            if rc != 0:
                print(f"rows={rows:6d} {cin:3d}->{cout:3d}: {name} path refused (rc {rc}): {lib.ln_last_error_string().decode()}", flush=True)
                del paths[name]
        times = {name: [] for name in paths}
        for _ in range(windows):
            for name, step in paths.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(iters):
                    step()
                b.record()
                b.synchronize()
                times[name].append(a.elapsed_time(b) / iters * 1e3)
        out = []
        for name, t in times.items():
            t = sorted(t)
            out.append(f"{name} median {t[len(t) // 2]:6.1f} us ({t[0]:.1f} - {t[-1]:.1f})")
        print(f"rows={rows:6d} {cin:3d}->{cout:3d} forward + backward: " + "   ".join(out), flush=True)


if "--f16" in sys.argv:
    bench_f16()
    sys.exit(0)
shapes = [(480000, 4, 16, 0.2), (480000, 16, 32, 0.2), (480000, 9, 1, -1.0), (46538, 96, 96, -1.0), (46538, 96, 48, -1.0), (46538, 48, 8, -1.0),
          (11407, 128, 32, -1.0), (11407, 32, 128, -1.0)]
for rows, cin, cout, slope in shapes:
    x = torch.randn((rows, cin), device=dev, requires_grad=True)
    w = torch.randn((cout, cin), device=dev, requires_grad=True)
    b = torch.randn((cout,), device=dev, requires_grad=True)
    g = torch.randn((rows, cout), device=dev)
    def step():
        x.grad = w.grad = b.grad = None
        LinearLeakyReluFunction.apply(x, w, b, slope).backward(g)
    for _ in range(3):
        step()
    out = []
    for k in ("k_linear_act_forward", "k_linear_act_backward_x", "k_linear_act_backward_w", "k_linear_reduce_slabs"):
        lib.ln_profile_begin(k.encode(), 64)
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        ms, cnt = C.c_double(0.0), C.c_int(0)
        lib.ln_profile_end(C.byref(ms), C.byref(cnt))
        out.append(f"{k[13:]} {ms.value / max(cnt.value, 1) * 1e3:6.1f}us x{cnt.value // 5}")
    print(f"rows={rows:7d} {cin:3d}->{cout:3d}: " + "  ".join(out), flush=True)
    if cin in _MFMA_LINEAR_WIDTHS and cout in _MFMA_LINEAR_WIDTHS:  # the same layer (without bias) as an extent-1 convolution
        def step2():
            x.grad = w.grad = None
            LinearMfmaFunction.apply(x, w).backward(g)
        for _ in range(3):
            step2()
        out = []
        for k in ("k_conv_mfma", "k_grad_filter_mfma", "k_reduce_slabs"):
            lib.ln_profile_begin(k.encode(), 64)
            for _ in range(5):
                step2()
            torch.cuda.synchronize()
            ms, cnt = C.c_double(0.0), C.c_int(0)
            lib.ln_profile_end(C.byref(ms), C.byref(cnt))
            out.append(f"{k} {ms.value / max(cnt.value, 1) * 1e3:6.1f}us x{cnt.value // 5}")
        print(" " * 24 + "as 1x1 convolution: " + "  ".join(out), flush=True)
