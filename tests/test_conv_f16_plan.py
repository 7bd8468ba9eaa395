"""The fp16 convolution's dispatch as a CPU test: lattice_net_amd/csrc/ln_conv_f16_plan.h is plain C++ (no HIP), so
tests/cabi/conv_f16_plan_check.cpp is built with the host compiler under AddressSanitizer + UBSan and checks, over shapes, row counts
and pointer alignments around every boundary of the dispatch, that the per-slot chunks cover every output column once within 32 KB of
LDS, that the tiled form is taken only where its kernel is built and its grid covers the rows, that the generic form is taken exactly
when neither other is, that the filter gradient's tiles partition V x F and its fallback is refused exactly when its rows exceed
64 KB of LDS.  The workspace size it derives is compared here with what the library's C ABI returns, and the case table of
tests/test_gpu_conv_f16_forms.py is asked of the plan: every form of the dispatch is taken by at least one case."""
import os
import shutil
import subprocess

import pytest

from lattice_net_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_checker(directory, sanitize):
    """conv_f16_plan_check built with the host compiler; `sanitize`: under ASan + UBSan (the CPU tests here).  Without, the same program
    as a plain tool that prints plans: what a test marked `gpu` may run."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(directory), "conv_f16_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    cmd += ["-I", os.path.join(ROOT, "lattice_net_amd", "csrc"), os.path.join(ROOT, "tests", "cabi", "conv_f16_plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    return build_checker(tmp_path_factory.mktemp("plan_f16"), sanitize=True)


@pytest.fixture(scope="module")
def grid_walk(plan_check):
    r = subprocess.run([plan_check], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:] + r.stderr[-4000:])
    return r.stdout.splitlines()


def test_f16_plans_hold_their_invariants(grid_walk):
    assert grid_walk[-1].startswith("PLANS OK ") and int(grid_walk[-1].split()[2]) > 1000000, grid_walk[-1]


def test_f16_plan_workspace_is_the_c_abi_query(grid_walk):
    lib = _lib.load()
    rows = [tuple(int(x) for x in line.split()[1:]) for line in grid_walk if line.startswith("Q ")]
    assert len(rows) > 20000
    for m, e, v, f, want in rows:
        assert lib.ln_conv_grad_filter_f16_workspace_bytes(m, e, v, f) == want, (m, e, v, f)
    for m in (0, -1):
        assert lib.ln_conv_grad_filter_f16_workspace_bytes(m, 9, 64, 64) == 256


def f16_plans(exe, cases, e):
    """{case: {"FWD" / "VG": {form, V, nt, t, line, kstep, launches, chunks [(nt, f_off)]}, "GF": {form, launches, gridz, lds, tiles
    [(vt, ft, v_off, f_off)]}}} from `conv_f16_plan_check plan`; cases: (mq, mn, V, F, values_off, grad_out_off)"""
    args = [str(x) for c in cases for x in (c[0], c[1], e, c[2], c[3], c[4], c[5])]
    r = subprocess.run([exe, "plan"] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:] + r.stderr[-4000:])
    plans, cur = {}, None
    for line in r.stdout.splitlines():
        tag, *rest = line.split()
        if tag == "PLAN":
            mq, mn, ext, v, f, voff, goff = (int(x) for x in rest)
            assert ext == e
            cur = plans.setdefault((mq, mn, v, f, voff, goff), {})
        elif tag in ("FWD", "VG"):
            v, nt, t, line_, kstep, n = (int(x) for x in rest[1:7])
            cur[tag] = {"form": rest[0], "V": v, "nt": nt, "t": t, "line": bool(line_), "kstep": kstep, "launches": n,
                        "chunks": [tuple(int(x) for x in c.split(":")) for c in rest[7:]]}
        else:
            assert tag == "GF", line
            cur["GF"] = {"form": rest[0], "launches": int(rest[1]), "gridz": int(rest[2]), "lds": int(rest[3]),
                         "tiles": [tuple(int(x) for x in c.split(":")) for c in rest[4:]]}
    assert len(plans) == len(set(cases)) and set(plans) == set(cases)
    return plans


def f16_forms():
    """{form: predicate over (case, plan)}: every form of the fp16 dispatch that tests/test_gpu_conv_f16_forms.py must reach"""
    forms = {}

    def conv(where, **want):
        return lambda c, p: any(all(p[w][k] == x for k, x in want.items()) for w in where)

    both = ("FWD", "VG")
    for v, f in ((32, 32), (32, 64), (64, 32), (64, 64)):
        forms["tiled %d -> %d, T = 1" % (v, f)] = conv(both, form="TILED", V=v, nt=f // 16, t=1)
    for t in (2, 3, 4):
        forms["tiled T = %d, line-shaped gather (V = 64)" % t] = conv(both, form="TILED", t=t, line=True, V=64)
        forms["tiled T = %d, fragment gather (V = 32)" % t] = conv(both, form="TILED", t=t, line=False, V=32)
        forms["tiled T = %d as flipped, transposed value gradient" % t] = conv(("VG",), form="TILED", t=t)
    for v in (16, 32, 64, 96, 128, 256):
        forms["per-slot V = %d as forward" % v] = conv(("FWD",), form="SLOTS", V=v)
        forms["per-slot V = %d as value gradient" % v] = conv(("VG",), form="SLOTS", V=v)
    forms["per-slot K = 16 step"] = conv(both, form="SLOTS", kstep=16)
    forms["per-slot K = 32 step"] = conv(both, form="SLOTS", kstep=32)
    for nt in (8, 4, 2, 1):
        forms["per-slot chunk of %d columns at a nonzero f_off" % (16 * nt)] = \
            lambda c, p, nt=nt: any(p[w]["form"] == "SLOTS" and any(n == nt and off > 0 for n, off in p[w]["chunks"]) for w in both)
    forms["per-slot chunks 8, 4, 2, 1 in one launch sequence"] = \
        lambda c, p: any(p[w]["form"] == "SLOTS" and [n for n, _ in p[w]["chunks"]] == [8, 4, 2, 1] for w in both)
    forms["per-slot V = 256, F = 128: two chunks of 64"] = \
        lambda c, p: any(p[w]["form"] == "SLOTS" and p[w]["V"] == 256 and p[w]["chunks"] == [(4, 0), (4, 64)] for w in both)
    forms["per-slot V = 256, F = 112: chunks 4, 2, 1"] = \
        lambda c, p: any(p[w]["form"] == "SLOTS" and p[w]["V"] == 256 and p[w]["chunks"] == [(4, 0), (2, 64), (1, 96)] for w in both)
    forms["per-slot at a tiled shape, values 8 bytes off"] = lambda c, p: c[2:5] == (64, 64, 8) and p["FWD"]["form"] == "SLOTS"
    forms["generic: V = 48"] = lambda c, p: c[2] == 48 and c[3] % 16 == 0 and c[4] == 0 and p["FWD"]["form"] == "GENERIC"
    forms["generic: F no multiple of 16"] = lambda c, p: c[3] % 16 != 0 and p["FWD"]["form"] == "GENERIC"
    forms["generic: a matrix-core shape, values 2 bytes off"] = \
        lambda c, p: c[2] in (16, 32, 64, 96, 128, 256) and c[3] % 16 == 0 and c[4] == 2 and p["FWD"]["form"] == "GENERIC"
    forms["generic: a per-slot shape as value gradient, grad_out 4 bytes off"] = \
        lambda c, p: c[3] in (16, 32, 64, 96, 128, 256) and c[2] % 16 == 0 and c[5] == 4 and p["VG"]["form"] == "GENERIC"
    for vt in (1, 2, 4):
        for ft in (1, 2, 4):
            forms["filter gradient tile (%d, %d)" % (vt, ft)] = \
                lambda c, p, t=(vt, ft): p["GF"]["form"] == "MFMA" and any(x[:2] == t for x in p["GF"]["tiles"])
    for nt in (2, 1):
        forms["filter gradient tile of %d channels at a nonzero v_off" % (16 * nt)] = \
            lambda c, p, nt=nt: p["GF"]["form"] == "MFMA" and any(x[0] == nt and x[2] > 0 for x in p["GF"]["tiles"])
        forms["filter gradient tile of %d filters at a nonzero f_off" % (16 * nt)] = \
            lambda c, p, nt=nt: p["GF"]["form"] == "MFMA" and any(x[1] == nt and x[3] > 0 for x in p["GF"]["tiles"])
    forms["filter gradient tile (2, 1) with both offsets nonzero"] = \
        lambda c, p: p["GF"]["form"] == "MFMA" and any(x[:2] == (2, 1) and x[2] > 0 and x[3] > 0 for x in p["GF"]["tiles"])
    forms["filter gradient fallback, gridDim.z = 1"] = lambda c, p: p["GF"]["form"] == "FALLBACK" and p["GF"]["gridz"] == 1
    forms["filter gradient fallback, gridDim.z > 1"] = lambda c, p: p["GF"]["form"] == "FALLBACK" and p["GF"]["gridz"] > 1 and c[4:] == (0, 0)
    forms["filter gradient fallback by a grad_out 4 bytes off, gridDim.z > 1"] = \
        lambda c, p: p["GF"]["form"] == "FALLBACK" and p["GF"]["gridz"] > 1 and c[2] % 16 == 0 and c[3] % 16 == 0 and c[5] == 4
    return forms


def test_f16_table_reaches_every_form(plan_check):
    """The case table of tests/test_gpu_conv_f16_forms.py, asked of the plan with the pointer offsets the cases pass: every form above is
    taken by at least one case.  A tuning change that moves a boundary fails here, on the CPU, and names the form that lost its case."""
    from tests.test_gpu_conv_f16_forms import CASES, E
    assert len(CASES) <= 30 and len(set(CASES)) == len(CASES)
    assert all(mq != mn and mq % 64 and mn % 64 and max(mq, mn) <= 98400 for mq, mn, *_ in CASES)
    plans = f16_plans(plan_check, CASES, E)
    reached = {name: [c for c in CASES if takes(c, plans[c])] for name, takes in f16_forms().items()}
    for name, cases in reached.items():
        print("%-70s %s" % (name, " ".join("%dx%d:%d->%d%s" % (c[:4] + ("+%d/%d" % c[4:] if c[4:] != (0, 0) else "",)) for c in cases)))
    missing = [name for name, cases in reached.items() if not cases]
    assert not missing, missing
    # the sub-tile counts above 1 are met just above their boundaries (multiples of 16 384 rows: the checker's grid walk asserts them)
    for c in CASES:
        for w, rows in (("FWD", c[0]), ("VG", c[1])):
            if plans[c][w]["form"] == "TILED" and plans[c][w]["t"] > 1:
                assert 0 < rows % 16384 < 64, (c, w)
    # no case asks for the refusal: it has a test of its own
    assert all(p["GF"]["form"] != "UNSUPPORTED" for p in plans.values())
