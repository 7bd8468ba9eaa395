"""LN_CONV_OVERLAPPED in the convolution plans, as a CPU test: tests/cabi/conv_plan_overlap_check.cpp is built with the host compiler
under AddressSanitizer + UBSan against lattice_net_amd/csrc/ln_conv_plan.h and walks a sweep of row counts at V = F = 32, E = 9 — the
small sizes tests/test_gpu_conv_overlapped.py runs, the C3 and C4 sizes of the benchmark, the boundaries of the whole-CU cost model.
Without the flag every plan and size query is, field for field, what tests/golden/conv_plan_unflagged.txt recorded from the plan header
before the flag existed; with it the workgroups cover the rows, write no more slabs than without it, and the one workspace query covers
them."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_plan_unflagged.txt")


@pytest.fixture(scope="module")
def overlap_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("plan_ovl") / "conv_plan_overlap_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "lattice_net_amd", "csrc"), os.path.join(ROOT, "tests", "cabi", "conv_plan_overlap_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def test_unflagged_plans_are_the_recorded_ones_and_flagged_plans_hold_their_invariants(overlap_check):
    want = [line for line in open(GOLDEN).read().splitlines() if line.startswith("U ")]
    ms = [line.split()[1] for line in want]
    assert len(ms) > 150 and {"4096", "46538", "129024"} <= set(ms)
    r = subprocess.run([overlap_check] + ms, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:] + r.stderr[-4000:])
    assert "OVERLAP PLANS OK" in r.stdout
    have = [line for line in r.stdout.splitlines() if line.startswith("U ")]
    assert len(have) == len(want)
    for h, w in zip(have, want):
        assert h == w
    flagged = {int(m): (int(t), int(c), int(g)) for _, m, _, t, _, c, _, g in (line.split() for line in r.stdout.splitlines() if line.startswith("O "))}
    assert len(flagged) == len(ms)
    # the hint changes the shape from LN_CONV_B3_MIN_ROWS up to two rounds of whole-CU workgroups (2 x 256 x 192 rows) and nowhere else
    (ovl_t, ovl_c, lo, hi), = [tuple(int(x) for x in line.split()[1:]) for line in r.stdout.splitlines() if line.startswith("SHAPE ")]
    assert (lo, hi) == (4096, 98304)
    assert all(c == 1 for m, (_, c, _) in flagged.items() if m < lo or m > hi)
    assert all(c > 1 for m, (_, c, _) in flagged.items() if lo <= m <= hi)
    assert any(m > hi for m in flagged) and any(lo <= m <= hi for m in flagged)
    assert {(t, c) for m, (t, c, _) in flagged.items() if lo <= m <= hi} == {(ovl_t, ovl_c)}  # one narrow instance is built
    # ... and it is the one the GPU test lays its row counts out for (read from its text: this test stays free of torch and the GPU modules)
    gpu_test = open(os.path.join(ROOT, "tests", "test_gpu_conv_overlapped.py")).read()
    assert re.search(r"^OVL_T, OVL_C, OVL_MAX_ROWS = (\d+), (\d+), (\d+)\b", gpu_test, re.M).groups() == (str(ovl_t), str(ovl_c), str(hi))
