"""The convolution dispatch as a CPU test: lattice_net_amd/csrc/ln_conv_plan.h is plain C++ (no HIP), so tests/cabi/conv_plan_check.cpp
is built with the host compiler under AddressSanitizer + UBSan and checks, over shapes around every boundary of the dispatch, that
each plan covers every output column once, keeps its bank regions and slabs inside the layout it reports and the layout inside the
workspace offered, degrades to no bank / no slot split without a usable workspace, and that at most one launch carries a pending
slab sum.  The sizes it derives from the plan are compared here with what the library's C ABI returns."""
import os
import shutil
import subprocess

import pytest

from lattice_net_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("plan") / "conv_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "lattice_net_amd", "csrc"), os.path.join(ROOT, "tests", "cabi", "conv_plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def _run(exe, b3):
    r = subprocess.run([exe, "1" if b3 else "0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:] + r.stderr[-4000:])
    assert "PLANS OK" in r.stdout
    return [tuple(int(x) for x in line.split()[1:]) for line in r.stdout.splitlines() if line.startswith("Q ")]


def test_plans_hold_their_invariants_with_the_exact_f32_switch(plan_check):
    assert len(_run(plan_check, False)) > 20000


def test_plan_sizes_are_the_c_abi_queries(plan_check):
    lib = _lib.load()
    b3 = os.environ.get("LN_CONV_EXACT_F32", "")[:1] != "1"  # (the library reads the switch once per process)
    rows = _run(plan_check, b3)
    assert len(rows) > 20000
    for m, e, v, f, fwd, bank, gf, lin, *bwd in rows:
        assert lib.ln_conv_forward_workspace_bytes(m, e, v, f) == fwd, (m, e, v, f)
        assert lib.ln_conv_bank_workspace_bytes(m, e, v, f) == bank, (m, e, v, f)
        assert lib.ln_conv_grad_filter_workspace_bytes(m, e, v, f) == gf, (m, e, v, f)
        if e == 1:
            assert lib.ln_linear_backward_workspace_bytes(m, f, v) == lin, (m, v, f)
        assert len(bwd) == 3
        for mn, want in zip((m, m // 2 + 1, 2 * m), bwd):
            assert lib.ln_conv_backward_workspace_bytes(m, mn, e, v, f) == want, (m, mn, e, v, f)
