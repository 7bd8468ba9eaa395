"""The fp16 linear layer's dispatch as a CPU test: lattice_net_amd/csrc/ln_linear_f16_plan.h is plain C++ (no HIP), so
tests/cabi/linear_f16_plan_check.cpp is built with the host compiler under AddressSanitizer + UBSan and checks, over shapes, row
counts and pointer alignments around every boundary of the dispatch, that the column chunks cover every output column once within
64 KB of LDS, that the row tiles are shared out over at most 512 workgroups with none empty, that the element-wise forms are taken
exactly when the matrix-core ones are not, that the weight gradient's tiles partition cout x cin and sum every bias element once, and
the refusal rules.  The workspace size it derives from the slabs is compared here with what the library's C ABI returns, and the case
table of tests/test_gpu_linear_f16.py is asked of the plan: every form of the dispatch is taken by at least one case."""
import os
import shutil
import subprocess

import pytest

from lattice_net_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_checker(directory, sanitize):
    """linear_f16_plan_check built with the host compiler; `sanitize`: under ASan + UBSan (the CPU tests here).  Without, the same
    program as a plain tool that prints plans: what a test marked `gpu` may run."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(directory), "linear_f16_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    cmd += ["-I", os.path.join(ROOT, "lattice_net_amd", "csrc"), os.path.join(ROOT, "tests", "cabi", "linear_f16_plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    return build_checker(tmp_path_factory.mktemp("plan_lin16"), sanitize=True)


@pytest.fixture(scope="module")
def grid_walk(plan_check):
    r = subprocess.run([plan_check], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:] + r.stderr[-4000:])
    return r.stdout.splitlines()


def test_linear_f16_plans_hold_their_invariants_and_refusal_rules(grid_walk):
    assert grid_walk[-1].startswith("PLANS OK ") and int(grid_walk[-1].split()[2]) > 100000, grid_walk[-1]


def test_linear_f16_plan_workspace_is_the_c_abi_query(grid_walk):
    lib = _lib.load()
    rows = [tuple(int(x) for x in line.split()[1:]) for line in grid_walk if line.startswith("Q ")]
    assert len(rows) > 10000
    for m, cin, cout, want in rows:
        assert lib.ln_linear_backward_f16_workspace_bytes(m, cin, cout) == want, (m, cin, cout)
    for m in (0, -1):
        assert lib.ln_linear_backward_f16_workspace_bytes(m, 64, 64) == 256


def linear_f16_plans(exe, cases):
    """{case: {"FWD" / "GX": {form, kstep, nt, tiles_per_wg, launches, grid, chunks [(nt, off)]}, "GW": {form, launches, chunks, gridy,
    tiles [(vt, ft, v_off, f_off)]}}} from `linear_f16_plan_check plan`; cases: (rows, cin, cout, x_off)"""
    args = [str(x) for c in cases for x in c]
    r = subprocess.run([exe, "plan"] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:] + r.stderr[-4000:])
    plans, cur = {}, None
    for line in r.stdout.splitlines():
        tag, *rest = line.split()
        if tag == "PLAN":
            cur = plans.setdefault(tuple(int(x) for x in rest), {})
        elif tag in ("FWD", "GX"):
            kstep, nt, tpw, n, grid = (int(x) for x in rest[1:6])
            cur[tag] = {"form": rest[0], "kstep": kstep, "nt": nt, "tiles_per_wg": tpw, "launches": n, "grid": grid,
                        "chunks": [tuple(int(x) for x in c.split(":")) for c in rest[6:]]}
        else:
            assert tag == "GW", line
            cur["GW"] = {"form": rest[0], "launches": int(rest[1]), "chunks": int(rest[2]), "gridy": int(rest[3]),
                         "tiles": [tuple(int(x) for x in c.split(":")) for c in rest[4:]]}
    assert len(plans) == len(set(cases)) and set(plans) == set(cases)
    return plans


def linear_f16_forms():
    """{form: predicate over (case, plan)}: every form of the dispatch that tests/test_gpu_linear_f16.py must reach"""
    forms = {}
    both = ("FWD", "GX")
    for w in both:
        for kstep in (32, 16):
            forms["%s matrix-core, K = %d steps" % (w, kstep)] = lambda c, p, w=w, kstep=kstep: p[w]["form"] == "MFMA" and p[w]["kstep"] == kstep
        forms["%s matrix-core in more than one column chunk" % w] = lambda c, p, w=w: p[w]["form"] == "MFMA" and p[w]["launches"] > 1
        forms["%s one thread per element" % w] = lambda c, p, w=w: p[w]["form"] == "GENERIC"
    for nt in (16, 8, 4, 2, 1):
        forms["matrix-core chunk of %d columns" % (16 * nt)] = \
            lambda c, p, nt=nt: any(p[w]["form"] == "MFMA" and any(n == nt for n, _ in p[w]["chunks"]) for w in both)
    for nt in (8, 4, 2, 1):
        forms["matrix-core chunk of %d columns at a nonzero offset" % (16 * nt)] = \
            lambda c, p, nt=nt: any(p[w]["form"] == "MFMA" and any(n == nt and off > 0 for n, off in p[w]["chunks"]) for w in both)
    forms["matrix-core chunks 8, 4, 2, 1 in one launch sequence"] = \
        lambda c, p: any(p[w]["form"] == "MFMA" and [n for n, _ in p[w]["chunks"]] == [8, 4, 2, 1] for w in both)
    forms["the largest bank, 256 x 256: two chunks of 128 columns each way"] = \
        lambda c, p: c[1:3] == (256, 256) and all(p[w]["form"] == "MFMA" and p[w]["chunks"] == [(8, 0), (8, 128)] for w in both)
    forms["matrix-core, a second tile behind one staging of the bank"] = \
        lambda c, p: any(p[w]["form"] == "MFMA" and p[w]["tiles_per_wg"] > 1 for w in both)
    forms["matrix-core, one row"] = lambda c, p: c[0] == 1 and p["FWD"]["form"] == "MFMA"
    forms["one thread per element: columns no multiple of 16"] = lambda c, p: c[2] % 16 != 0 and p["FWD"]["form"] == "GENERIC"
    forms["one thread per element: a contraction length no multiple of 16"] = \
        lambda c, p: c[1] % 16 != 0 and p["FWD"]["form"] == "GENERIC"
    forms["one thread per element: a matrix-core shape, x 2 bytes off"] = \
        lambda c, p: c[1] % 16 == 0 and c[2] % 16 == 0 and c[3] == 2 and p["FWD"]["form"] == "GENERIC" and p["GX"]["form"] == "MFMA"
    for vt in (1, 2, 4):
        for ft in (1, 2, 4):
            forms["weight gradient tile (%d, %d)" % (vt, ft)] = \
                lambda c, p, t=(vt, ft): p["GW"]["form"] == "MFMA" and any(x[:2] == t for x in p["GW"]["tiles"])
    forms["weight gradient tile at nonzero v_off and f_off"] = \
        lambda c, p: p["GW"]["form"] == "MFMA" and any(x[2] > 0 and x[3] > 0 for x in p["GW"]["tiles"])
    forms["weight gradient, bias summed by more than one launch"] = \
        lambda c, p: p["GW"]["form"] == "MFMA" and sum(1 for x in p["GW"]["tiles"] if x[3] == 0) > 1
    for n in (1, 2, 3):
        forms["weight gradient matrix-core, %d slab%s" % (n, "s" if n > 1 else "")] = lambda c, p, n=n: p["GW"]["form"] == "MFMA" and p["GW"]["chunks"] == n
        forms["weight gradient fallback, %d slab%s" % (n, "s" if n > 1 else "")] = lambda c, p, n=n: p["GW"]["form"] == "FALLBACK" and p["GW"]["chunks"] == n
    forms["weight gradient fallback, gridDim.y > 1"] = lambda c, p: p["GW"]["form"] == "FALLBACK" and p["GW"]["gridy"] > 1
    forms["weight gradient fallback by an x 2 bytes off"] = lambda c, p: p["GW"]["form"] == "FALLBACK" and c[1] % 16 == 0 and c[2] % 16 == 0 and c[3] == 2
    return forms


def test_linear_f16_table_reaches_every_form(plan_check):
    """The case table of tests/test_gpu_linear_f16.py, asked of the plan with the pointer offsets the cases pass: every form above is
    taken by at least one case.  A tuning change that moves a boundary fails here, on the CPU, and names the form that lost its case."""
    from tests.test_gpu_linear_f16 import CASES, ISSUE_ROWS, ISSUE_WIDTHS
    assert len(CASES) <= 30 and len(set(CASES)) == len(CASES)
    # the row counts and the widths the issue names are all in the table
    assert set(ISSUE_ROWS) <= {c[0] for c in CASES} and set(ISSUE_WIDTHS) <= {c[1:3] for c in CASES}
    plans = linear_f16_plans(plan_check, CASES)
    reached = {name: [c for c in CASES if takes(c, plans[c])] for name, takes in linear_f16_forms().items()}
    for name, cases in reached.items():
        print("%-80s %s" % (name, " ".join("%d:%d->%d%s" % (c[:3] + ("+%d" % c[3] if c[3] else "",)) for c in cases)))
    missing = [name for name, cases in reached.items() if not cases]
    assert not missing, missing
    assert all(p["GW"]["form"] != "UNSUPPORTED" for p in plans.values())
