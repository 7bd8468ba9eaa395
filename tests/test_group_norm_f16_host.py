"""Host-side checks of the fp16 GroupNorm entry points (no GPU): the two symbols are declared in the header, bound with the argument
lists of their fp32 twins and named in the kernel list; the 65-range refusal of group_norm_rows on fp16 rows
fires on shapes and dtypes alone.  That last part runs here on CPU tensors with the library loader replaced by one that fails the test:
the ValueError is raised before any device or library call, so it needs no mocked CUDA and is not skipped."""
import os
import re

import pytest
import torch

from lattice_net_amd import _lib, lattice_blocks

PAIRS = {"ln_group_norm_forward_segments_f16": "ln_group_norm_forward_segments",
         "ln_group_norm_backward_segments_f16": "ln_group_norm_backward_segments"}


def test_symbols_are_declared_and_bound():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "latticenet_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for half, single in PAIRS.items():
        assert re.search(r"\bint\s+%s\s*\(\s*const void\*\s*x\b" % half, header), f"{half} is not declared with a const void* x"
        assert hasattr(lib, half)
        assert _lib.SIGNATURES[half] == _lib.SIGNATURES[single], f"{half} does not mirror {single} argument for argument"
    names = lib.ln_kernel_names().decode().split(",")
    for k in ("k_gn_stats_segments", "k_gn_apply_segments", "k_gn_backward_apply_segments"):
        assert k in names and k + "_f16" in names
    assert "k_gn_param_grads_segments_f16" not in names  # (no row access: one instance serves both)


def test_null_and_misaligned_arguments_are_refused_on_the_host():
    """Argument checks run before any launch: a null x is LN_ERR_ARG, and so is an x 2 bytes off (8-byte alignment is asked of fp16
    matrices, 16 of fp32 ones: an address 8 bytes off passes the first and not the second).  Addresses only; nothing is dereferenced."""
    lib = _lib.load()
    big = 1 << 30
    fwd16 = lambda x, c=8, g=2, segs=1: lib.ln_group_norm_forward_segments_f16(x, None, None, 10, c, g, 1e-5, 0, 4096, 4096, 4096, 4096, big, None, 0,
                                                                               None, 4096, segs, None)
    fwd32 = lambda x: lib.ln_group_norm_forward_segments(x, None, None, 10, 8, 2, 1e-5, 0, 4096, 4096, 4096, 4096, big, None, 0, None, 4096, 1, None)
    assert fwd16(None) == -1 and fwd16(4096 + 2) == -1
    assert b"8-byte aligned" in lib.ln_last_error_string()
    assert fwd32(4096 + 8) == -1 and b"16-byte aligned" in lib.ln_last_error_string()
    assert fwd16(4096, 6, 3) == -2 and fwd16(4096, segs=65) == -2


def test_65_ranges_on_fp16_rows_raise_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(_lib, "load", no_library)
    gn = torch.nn.GroupNorm(4, 8)
    x = torch.zeros((100, 8), dtype=torch.float16)
    with pytest.raises(ValueError, match="float16 rows takes at most 64 ranges"):
        lattice_blocks.group_norm_rows(x, gn, False, None, torch.arange(0, 66, dtype=torch.int32))
    with pytest.raises(ValueError, match="float16 rows takes at most 64 ranges"):
        lattice_blocks.group_norm_rows(x, gn, True, None, torch.arange(0, 66, dtype=torch.int32), many_ranges=True)
