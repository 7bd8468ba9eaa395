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


def _two_lattice_plans(exe, shapes, e, b3=True):
    """{shape: {"FWD" / "VG": [(kernel, nt, t, nsplit, cols)], "GF": (form, vs, fs, tile), "BWD": form}} from `conv_plan_check plan`"""
    args = [str(x) for mq, mn, v, f in shapes for x in (mq, mn, e, v, f)]
    r = subprocess.run([exe, "plan", "1" if b3 else "0"] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:] + r.stderr[-4000:])
    plans, cur = {}, None
    for line in r.stdout.splitlines():
        tag, *rest = line.split()
        if tag == "PLAN":
            mq, mn, _, v, f = (int(x) for x in rest)
            cur = plans.setdefault((mq, mn, v, f), {"FWD": [], "VG": []})
        elif tag in ("FWD", "VG"):
            cur[tag].append((rest[0],) + tuple(int(x) for x in rest[1:]))
        elif tag == "GF":
            cur["GF"] = (rest[0],) + tuple(int(x) for x in rest[1:])
        else:
            assert tag == "BWD", line
            cur["BWD"] = rest[0]
    assert len(plans) == len(set(shapes))
    return plans


def two_lattice_forms(plans):
    """{form: [shapes that take it]} over the forms a convolution between two lattices can take: every forward kernel (as forward or as
    value gradient), the per-slot kernels as a flipped, transposed value gradient, every filter-gradient form and block, and the
    backward's forms that are not same-list by definition"""
    def conv(kernel, where=("FWD", "VG"), t=None, split=None):
        def takes(p):
            return any(k == kernel and t in (None, lt) and split in (None, nsplit > 1) for w in where for k, _, lt, nsplit, _ in p[w])
        return takes
    forms = {
        "LN_K_FORWARD_B3": conv("LN_K_FORWARD_B3"), "LN_K_FULL": conv("LN_K_FULL"), "LN_K_MFMA": conv("LN_K_MFMA"),
        "LN_K_MFMA_B3 t == 1": conv("LN_K_MFMA_B3", t=1), "LN_K_MFMA_B3 t == 3": conv("LN_K_MFMA_B3", t=3),
        "LN_K_ROWS32 unsplit": conv("LN_K_ROWS32", split=False), "LN_K_ROWS32 nsplit > 1": conv("LN_K_ROWS32", split=True),
        "LN_K_ROWS32SK unsplit": conv("LN_K_ROWS32SK", split=False), "LN_K_ROWS32SK nsplit > 1": conv("LN_K_ROWS32SK", split=True),
        "LN_K_SUM_PARTIALS": conv("LN_K_SUM_PARTIALS"), "LN_K_GENERIC": conv("LN_K_GENERIC"),
        "LN_K_MFMA_B3 as value gradient": conv("LN_K_MFMA_B3", where=("VG",)), "LN_K_ROWS32 as value gradient": conv("LN_K_ROWS32", where=("VG",)),
        "LN_K_MFMA as value gradient": conv("LN_K_MFMA", where=("VG",)),
        "LN_GF_GENERIC": lambda p: p["GF"][0] == "LN_GF_GENERIC", "LN_GF_F32": lambda p: p["GF"][0] == "LN_GF_F32",
        "LN_BWD_FULL_SUM, fp32 filter gradient": lambda p: p["BWD"] == "LN_BWD_FULL_SUM" and p["GF"][0] == "LN_GF_F32",
        "LN_BWD_FULL_SUM, bf16x3 filter gradient": lambda p: p["BWD"] == "LN_BWD_FULL_SUM" and p["GF"][0] == "LN_GF_B3",
        "LN_BWD_TWO_CALLS": lambda p: p["BWD"] == "LN_BWD_TWO_CALLS",
    }
    for vs, fs in ((128, 128), (64, 64), (32, 96), (96, 32), (32, 64), (64, 32), (32, 32)):
        forms["LN_GF_B3 %d x %d" % (vs, fs)] = lambda p, b=("LN_GF_B3", vs, fs): p["GF"][:3] == b
    return {name: [s for s, p in plans.items() if takes(p)] for name, takes in forms.items()}


def test_two_lattice_shapes_reach_every_form(plan_check):
    """The shape table of tests/test_gpu_conv_two_lattices.py, asked of the plan with the library's own inputs (queried workspace, aligned
    buffers, no bank left by an earlier call): every form above is taken by at least one case with mq != mn.  A tuning change that moves
    a boundary fails here, on the CPU, and names the form that lost its case."""
    from tests.test_gpu_conv_two_lattices import E, SHAPES
    assert all(mq != mn and mq % 64 and mq % 192 and mn % 64 and mn % 192 for mq, mn, _, _ in SHAPES)
    reached = two_lattice_forms(_two_lattice_plans(plan_check, SHAPES, E))
    for name, shapes in reached.items():
        print("%-42s %s" % (name, " ".join("%dx%d:%d->%d" % s for s in shapes)))
    missing = [name for name, shapes in reached.items() if not shapes]
    assert not missing, missing
