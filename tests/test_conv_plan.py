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


def _two_lattice_plans(exe, shapes, e=None, b3=True):
    """{shape: {"FWD" / "VG": [(kernel, nt, t, nsplit, cols, e_per)], "GF": (form, vs, fs, tile), "BWD": form}} from `conv_plan_check plan`.
    shapes: (mq, mn, v, f) at the one extent `e`, or (e, mq, mn, v, f) with an extent per shape (`e` None)"""
    per_shape = e is None
    args = [str(x) for s in shapes for x in ((s[1], s[2], s[0], s[3], s[4]) if per_shape else (s[0], s[1], e, s[2], s[3]))]
    r = subprocess.run([exe, "plan", "1" if b3 else "0"] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:] + r.stderr[-4000:])
    plans, cur = {}, None
    for line in r.stdout.splitlines():
        tag, *rest = line.split()
        if tag == "PLAN":
            mq, mn, ext, v, f = (int(x) for x in rest)
            cur = plans.setdefault((ext, mq, mn, v, f) if per_shape else (mq, mn, v, f), {"FWD": [], "VG": []})
        elif tag in ("FWD", "VG"):
            cur[tag].append((rest[0],) + tuple(int(x) for x in rest[1:]))
        elif tag == "GF":
            cur["GF"] = (rest[0],) + tuple(int(x) for x in rest[1:])
        else:
            assert tag == "BWD", line
            cur["BWD"] = rest[0]
    assert len(plans) == len(set(shapes)) and set(plans) == set(shapes)
    return plans


def _conv_takes(kernel, where=("FWD", "VG"), t=None, split=None):
    def takes(p):
        return any(k == kernel and t in (None, lt) and split in (None, nsplit > 1) for w in where for k, _, lt, nsplit, _, _ in p[w])
    return takes


def _form_predicates():
    conv = _conv_takes
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
    return forms


def two_lattice_forms(plans):
    """{form: [shapes that take it]} over the forms a convolution between two lattices can take: every forward kernel (as forward or as
    value gradient), the per-slot kernels as a flipped, transposed value gradient, every filter-gradient form and block, and the
    backward's forms that are not same-list by definition"""
    return {name: [s for s, p in plans.items() if takes(p)] for name, takes in _form_predicates().items()}


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


# kernels that stage the neighbour ids of a tile in LDS (s_nbr[R * LN_CONV_LDS_E]: extents up to 16)
LDS_ID_KERNELS = ("LN_K_MFMA_B3", "LN_K_ROWS32", "LN_K_ROWS32SK")
# forms built for E == 9 alone
E9_ONLY_KERNELS = ("LN_K_FORWARD_B3", "LN_K_FULL")
B3_MIN_ROWS = 4096  # LN_CONV_B3_MIN_ROWS


def other_extent_forms(plans):
    """{form: [shapes that take it]} over the forms a convolution at an extent other than 9 can take"""
    forms = {name: takes for name, takes in _form_predicates().items()
             if not name.startswith(("LN_K_FORWARD_B3", "LN_K_FULL", "LN_BWD_", "LN_GF_B3", "LN_K_MFMA", "LN_GF_F32"))}
    conv = _conv_takes
    forms.update({
        "LN_K_MFMA unsplit": conv("LN_K_MFMA", split=False), "LN_K_MFMA nsplit > 1": conv("LN_K_MFMA", split=True),
        "LN_K_MFMA_B3 t == 1": conv("LN_K_MFMA_B3", t=1), "LN_K_MFMA_B3 t == 3": conv("LN_K_MFMA_B3", t=3),
        "LN_K_MFMA_B3 as value gradient": conv("LN_K_MFMA_B3", where=("VG",)), "LN_K_MFMA as value gradient": conv("LN_K_MFMA", where=("VG",)),
    })
    for tile in (4, 2, 1):
        forms["LN_GF_F32 tile %d" % tile] = lambda p, b=("LN_GF_F32", tile): (p["GF"][0], p["GF"][3]) == b
    return {name: [s for s, p in plans.items() if takes(p)] for name, takes in forms.items()}


def test_other_extent_shapes_reach_every_form(plan_check):
    """The shape table of tests/test_gpu_conv_filter_extents.py, asked of the plan with the library's own inputs: every form an extent
    other than 9 can take is taken by a case with E != 9 and mq != mn; a split whose last part holds fewer slots occurs in the 16-row
    and in the wide form; E = 1 above LN_CONV_B3_MIN_ROWS reaches the bf16x3 kernels and the unsplit wide form; E = 17 stays off the
    kernels that keep their ids in LDS; and no E != 9 case plans a form built for E == 9.  Whoever opens one of those forms to other
    extents fails here and finds the table to extend."""
    from tests.test_gpu_conv_filter_extents import LINEAR_SHAPES, SHAPES
    assert all(e != 9 and mq != mn and mq % 64 and mq % 192 and mn % 64 and mn % 192 and max(mq, mn) <= 24400 for e, mq, mn, _, _ in SHAPES)
    assert len(SHAPES) <= 30 and len(set(SHAPES)) == len(SHAPES)
    plans = _two_lattice_plans(plan_check, SHAPES)
    reached = other_extent_forms(plans)
    for name, shapes in reached.items():
        print("%-42s %s" % (name, " ".join("E%d:%dx%d:%d->%d" % s for s in shapes)))
    missing = [name for name, shapes in reached.items() if not shapes]
    assert not missing, missing

    def launches(s, where=("FWD", "VG")):
        return [l for w in where for l in plans[s][w]]
    # each extent in a matrix-core forward, a value gradient and a filter gradient
    for e in (1, 5, 7, 11, 13, 15):
        rows = [s for s in SHAPES if s[0] == e]
        assert any(k != "LN_K_GENERIC" for s in rows for k, *_ in launches(s, ("FWD",))), e
        assert any(k != "LN_K_GENERIC" for s in rows for k, *_ in launches(s, ("VG",))), e
        assert any(plans[s]["GF"][0] == "LN_GF_F32" for s in rows), e
    # a split whose last part holds fewer slots than the others, in the 16-row form (fp32 and bf16x3) and in the wide form
    uneven = {k for s in SHAPES for k, _, _, nsplit, _, e_per in launches(s) if nsplit > 1 and s[0] % e_per != 0}
    print("uneven last split:", " ".join(sorted(uneven)))
    assert {"LN_K_MFMA", "LN_K_MFMA_B3", "LN_K_ROWS32", "LN_K_ROWS32SK", "LN_K_SUM_PARTIALS"} <= uneven, uneven
    for s in SHAPES:  # (what the tool's own CHECKs hold for every plan, restated for the table: e_per is the slots of a full part)
        for k, _, _, nsplit, _, e_per in launches(s):
            assert (nsplit - 1) * e_per < s[0] <= nsplit * e_per, (s, k, nsplit, e_per)
    # E = 1 above LN_CONV_B3_MIN_ROWS: the sizes of the network's level-0 and level-1 1 x 1 layers
    e1 = [s for s in SHAPES if s[0] == 1 and s[1] >= B3_MIN_ROWS]
    assert any(k == "LN_K_MFMA_B3" for s in e1 for k, *_ in launches(s, ("FWD",)))
    assert any(k == "LN_K_ROWS32" and nsplit == 1 for s in e1 for k, _, _, nsplit, _, _ in launches(s, ("FWD",)))
    assert all(nsplit == 1 for s in SHAPES if s[0] == 1 for _, _, _, nsplit, _, _ in launches(s)), "E < 2 turns the slot split off"
    # E = 17 and its E = 15 twin
    for s in (s for s in SHAPES if s[0] == 17):
        twin = (15,) + s[1:]
        assert twin in plans and any(k == "LN_K_MFMA_B3" for k, *_ in launches(twin, ("FWD",))), twin
        assert not any(k in LDS_ID_KERNELS or k.startswith("LN_K_SPLIT_BANK") for k, *_ in launches(s)), (s, launches(s))
    assert any(s[0] == 17 for s in SHAPES)
    assert not any(k in LDS_ID_KERNELS for s in SHAPES if s[0] > 16 for k, *_ in launches(s))
    # the E == 9 forms stay closed
    for s in SHAPES:
        assert not any(k in E9_ONLY_KERNELS for k, *_ in launches(s)), s
        assert plans[s]["GF"][0] != "LN_GF_B3" and plans[s]["BWD"] == "LN_BWD_TWO_CALLS", (s, plans[s]["GF"], plans[s]["BWD"])
    # ln_linear_backward: grad_x is the plain forward over (rows, 1, cout -> cin); the grad_w slab sum rides in its bank split where it has one
    lin = _two_lattice_plans(plan_check, [(1, rows, rows + 1, cout, cin) for rows, cin, cout in LINEAR_SHAPES])
    rides = {s[1:2] + s[3:]: any(k.startswith("LN_K_SPLIT_BANK") for k, *_ in p["FWD"]) and p["GF"][0] == "LN_GF_F32" for s, p in lin.items()}
    print("linear backward, slab sum rides:", rides)
    assert any(rides.values()) and not all(rides.values())
    assert any(not r and p["GF"][0] == "LN_GF_F32" for r, p in zip(rides.values(), lin.values())), "no case launches the slab sum on its own"
