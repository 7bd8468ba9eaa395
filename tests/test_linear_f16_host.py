"""Host side of the fp16 linear layer, without a GPU: the header, the ctypes signatures and the build list agree on the three entry
points, the argument checks answer before any device call, and linear_leaky_relu takes fp32 CPU input exactly where it took it."""
import ctypes as C
import os
import re

import pytest
import torch

from lattice_net_amd import _lib, build_ext
from lattice_net_amd.lattice_modules import LinearF16Function, linear_leaky_relu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPES = {"int": C.c_int, "size_t": C.c_size_t, "const void*": C.c_void_p, "void*": C.c_void_p, "const float*": C.c_void_p, "float*": C.c_void_p}


def _declaration(name):
    text = open(os.path.join(ROOT, "include", "latticenet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"(\w[\w ]*?)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared in latticenet_hip.h"
    args = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*") for a in m.group(2).split(",")]
    return m.group(1).strip(), args


@pytest.mark.parametrize("name", ["ln_linear_forward_f16", "ln_linear_backward_f16_workspace_bytes", "ln_linear_backward_f16"])
def test_header_and_signatures_agree(name):
    res, args = _declaration(name)
    want_res, want_args = _lib.SIGNATURES[name]
    assert CTYPES[res] is want_res
    assert [CTYPES[a] for a in args] == list(want_args), (args, want_args)
    assert hasattr(_lib.load(), name)


def test_sources_and_kernel_names():
    assert "ln_linear_f16.hip" in build_ext.SOURCES
    assert os.path.exists(os.path.join(build_ext.CSRC, "ln_linear_f16.hip")) and os.path.exists(os.path.join(build_ext.CSRC, "ln_linear_f16_plan.h"))
    names = _lib.load().ln_kernel_names().decode().split(",")
    for k in ("k_linear_mfma_f16", "k_linear_generic_f16", "k_linear_grad_w_mfma_f16", "k_linear_grad_w_f16"):
        assert k in names


def test_argument_errors_answer_on_the_host():
    lib = _lib.load()
    assert lib.ln_linear_forward_f16(None, None, None, None, -1, 16, 16, None, None) == -1
    assert b"ln_linear_forward_f16" in lib.ln_last_error_string()
    assert lib.ln_linear_forward_f16(None, None, None, None, 5, 16, 16, None, None) == -1
    assert lib.ln_linear_backward_f16(None, None, None, 5, 0, 16, None, None, None, None, 0, None) == -1
    assert lib.ln_linear_backward_f16(None, None, None, 5, 16, 16, None, None, None, None, 0, None) == -1  # null grad_w
    assert b"ln_linear_backward_f16" in lib.ln_last_error_string()
    assert lib.ln_linear_backward_f16_workspace_bytes(1300, 64, 16) == (3 * 64 * 16 + 3 * 16) * 4 + 256
    assert lib.ln_linear_backward_f16_workspace_bytes(0, 64, 16) == 256


@pytest.mark.parametrize("slope", [-1.0, 0.2])
@pytest.mark.parametrize("bias", [False, True])
def test_fp32_cpu_input_is_bitwise_what_it_was(slope, bias):
    torch.manual_seed(0)
    x, w = torch.randn(70, 24), torch.randn(20, 24)
    b = torch.randn(20) if bias else None
    got = linear_leaky_relu(x, w, b, slope)
    want = torch.nn.functional.linear(x, w, b)
    want = torch.nn.functional.leaky_relu(want, slope) if slope >= 0 else want
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert not type(got.grad_fn).__name__.startswith("LinearF16Function")


def test_fp16_cpu_input_and_activations_do_not_take_the_new_branch():
    """the branch is for CUDA rows: fp16 CPU rows with fp16 weights go through torch as before, and a residual is refused off the branch"""
    x, w = torch.randn(8, 16).half(), torch.randn(4, 16).half()
    got = linear_leaky_relu(x, w, None, -1.0)
    assert got.dtype == torch.float16 and torch.equal(got, torch.nn.functional.linear(x, w))
    with pytest.raises(ValueError, match="residual"):
        linear_leaky_relu(torch.randn(8, 16), torch.randn(4, 16), None, -1.0, residual=torch.zeros(8, 4))
    assert LinearF16Function.apply is not None
