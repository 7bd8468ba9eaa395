"""The HIP sources carry no experiment switches: LN_CONV_EXACT_F32 is the one runtime choice, and A/B builds go through
build_ext.build(variant=..., extra_flags=...).  A switch read from the environment selects a path that no test runs, and a stray
variable on a user's machine would select it silently."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lattice_net_amd", "csrc")

REMOVED = [
    # runtime switches
    "LN_DEBUG_MASK", "LN_BWD_T", "LN_FWD_T", "LN_CONV_B3_T", "LN_CONV_WIDE_SPLIT", "LN_CONV_ROWS32", "LN_CONV_R32_SK", "LN_GFB_WIDE",
    "LN_BWD_SLAB_SUM_IN_SPLIT", "LN_BKT_NARROW", "LN_REDUCE_L8", "LN_F16_T", "LN_F16_PER_SLOT",
    # compile-time alternates
    "LN_FWD_LINE", "LN_BWD_LINE", "LN_BWD_SWZ", "LN_MFMA_B3_LINE", "LN_F16_LINE", "LN_CONV_R32_PIN", "LN_CONV_R32_SPREAD",
    "LN_CONV_R32_PRIO", "LN_CONV_R32_SKEW",
    # ablation and investigation builds
    "LN_CONV_PROBE", "LN_CONV_R32_PROBE", "LN_GFB_PROBE", "LN_CONV_PROBE_NO_MFMA", "LN_SCW_PROBE", "LN_SCB_PROBE", "LN_SEGMAX_PLAIN",
    "LN_PROBE_NO_CLEAR", "LN_TR_CHECK", "ln_dbg", "ln_debug_dump", "dbg_plain",
]


def _sources():
    paths = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert len(paths) >= 10, paths
    return {os.path.basename(p): open(p, encoding="utf-8").read() for p in paths}


def test_the_only_environment_switch_is_exact_f32():
    names = set()
    for name, text in _sources().items():
        calls = re.findall(r"\bgetenv\s*\(", text)
        literal = re.findall(r"\bgetenv\s*\(\s*\"([^\"]+)\"\s*\)", text)
        assert len(calls) == len(literal), f"{name}: getenv with a name that is not a string literal"
        names.update(literal)
    assert names == {"LN_CONV_EXACT_F32"}


def test_no_debug_mask():
    for name, text in _sources().items():
        assert "ln_debug_mask" not in text, name


def test_no_removed_switch_is_named():
    for name, text in _sources().items():
        found = [s for s in REMOVED if re.search(r"\b%s\b" % s, text)]
        assert not found, f"{name}: {found}"
