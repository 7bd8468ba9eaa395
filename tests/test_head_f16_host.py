"""Host side of the fp16 DeformSlice head (csrc/ln_classify_f16.hip), no GPU: the four entry points are declared, exported and bound,
the workspace query is a pure host function that is total over odd shapes and equals the fp32 query, and the form table the fp16 GPU
test derives its cases from (tests/point_reference.py) says what the header says about coverage."""
import itertools
import os
import re

from lattice_net_amd import _lib
from tests import point_reference as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ln_gather_forward_f16", "ln_slice_classify_forward_f16", "ln_slice_classify_backward_f16",
         "ln_slice_classify_backward_f16_workspace_bytes")


def test_the_four_symbols_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "latticenet_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in latticenet_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    # the argument lists are those of the fp32 entry points
    for name in NAMES:
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("_f16", "")], name


def test_the_new_launch_labels_are_listed():
    names = _lib.load().ln_kernel_names().decode().split(",")
    for k in ("k_gather_forward_f16", "k_slice_classify_forward_f16", "k_slice_classify_backward_f16"):
        assert k in names, k


def test_workspace_query_is_total_and_equals_the_fp32_query():
    lib = _lib.load()
    for n, d, v, c in itertools.product([0, 1, 69, 1000, 120000], [1, 2, 3, 4, 6], [1, 5, 8, 30, 32, 64, 96, 128, 160, 512, 777], [1, 3, 13, 20, 32, 50]):
        got = lib.ln_slice_classify_backward_f16_workspace_bytes(n, d, v, c)
        assert got > 0
        assert got == lib.ln_slice_classify_backward_workspace_bytes(n, d, v, c), (n, d, v, c)


def test_null_and_bad_arguments_are_reported_without_a_gpu():
    lib = _lib.load()
    assert lib.ln_gather_forward_f16(None, None, None, -1, 3, 8, None, None) == -1
    assert lib.ln_gather_forward_f16(None, None, None, 5, 3, 8, None, None) == -1
    assert b"null buffer" in lib.ln_last_error_string()
    assert lib.ln_gather_forward_f16(None, None, None, 0, 3, 8, None, None) == 0
    assert lib.ln_slice_classify_forward_f16(None, None, None, None, None, None, 5, 3, 32, 0, None, None) == -1
    assert lib.ln_slice_classify_forward_f16(None, None, None, None, None, None, 0, 3, 5, 3, None, None) == 0
    # a non-NULL g_values is an argument error before anything else is looked at
    assert lib.ln_slice_classify_backward_f16(None, None, None, None, None, None, 0, 3, 32, 20, 16, None, None, None, None, None, None, 0, None) == -1
    assert b"g_values must be NULL" in lib.ln_last_error_string()
    assert lib.ln_slice_classify_backward_f16(None, None, None, None, None, None, 0, 3, 32, 20, None, None, None, None, None, None, None, 0, None) == 0


def test_covered_shapes_are_the_wave_and_v4_forms_of_the_reference_table():
    """What the header promises, recomputed from point_reference: a form that is not scalar exists only at V % 4 == 0, and the pairs
    (form, PB) a V % 4 == 0 shape can take are wave, v4 64 / 32 / 16 forward and wave, v4 64 / 32 / 16 / 8 backward."""
    fwd, bwd = set(), set()
    for d, v, c in itertools.product(range(1, 7), range(1, 1025), (1, 3, 8, 13, 20, 21, 32, 33, 40, 50, 64)):
        f, b = P.sc_forward_form(d, v, c), P.sc_backward_form(d, v, c)
        if v % 4:
            assert f is None or f[0] == "scalar"
            assert b is None or b[0] == "scalar"
            continue
        if f is not None and f[0] != "scalar":
            fwd.add((f[0], f[1] if f[0] == "v4" else None))
        if b is not None and b[0] != "scalar":
            bwd.add((b[0], b[1] if b[0] == "v4" else None))
    assert fwd == {("wave", None), ("v4", 64), ("v4", 32), ("v4", 16)}
    assert bwd == {("wave", None), ("v4", 64), ("v4", 32), ("v4", 16), ("v4", 8)}
