"""Host side of the per-cloud losses over clouds of unequal sizes (the _ranges entry points of csrc/ln_nll.hip, ln_dice.hip, ln_lovasz.hip):
the workspace functions are total and every refusal that needs no device returns its code and names its entry point.  No GPU is touched."""
from lattice_net_amd import _lib


def test_ranges_workspace_functions_are_total():
    lib = _lib.load()
    for n in (-5, 0, 1, 514, 120000, 1 << 31, 1 << 40):
        for clouds in (-1, 0, 1, 16, 65535, 1 << 30):
            for longest in (-3, 0, 1, 300, 1 << 33):
                assert lib.ln_nll_ranges_workspace_bytes(n, clouds, longest) >= 256
                for classes in (-1, 0, 1, 20, 300, 5000):
                    assert lib.ln_dice_ranges_workspace_bytes(n, clouds, longest, classes) >= 256
                    assert lib.ln_lovasz_ranges_workspace_bytes(n, clouds, longest, classes) >= 256


def test_ranges_entry_points_refuse_before_they_touch_anything():
    """Every refusal that needs no device: pointers are never followed (16 stands for any non-null address)."""
    lib = _lib.load()
    P = 16
    calls = {
        "ln_nll_forward_ranges": lambda n, st, b, lg, c: lib.ln_nll_forward_ranges(P, P, n, st, b, lg, c, -1, None, P, 1 << 30, P, P, P, None),
        "ln_nll_backward_ranges": lambda n, st, b, lg, c: lib.ln_nll_backward_ranges(P, P, P, n, st, b, lg, c, -1, None, P, None),
        "ln_dice_forward_ranges": lambda n, st, b, lg, c: lib.ln_dice_forward_ranges(P, P, n, st, b, lg, c, -1, P, 1 << 30, P, P, P, P, None),
        "ln_dice_backward_ranges": lambda n, st, b, lg, c: lib.ln_dice_backward_ranges(P, P, P, P, n, st, b, lg, c, P, None),
        "ln_lovasz_forward_ranges": lambda n, st, b, lg, c: lib.ln_lovasz_forward_ranges(P, P, n, st, b, lg, c, -1, 0, P, 1 << 30, P, P, P, P, None),
    }
    for name, call in calls.items():
        limit = -2 if "nll" in name else -1  # LN_ERR_UNSUPPORTED in the NLL family, as in its equal-size entries
        for args, code in (((100, None, 3, 50, 5), -1), ((100, P, 0, 50, 5), -1), ((100, P, 65536, 50, 5), limit), ((100, P, 3, -1, 5), -1),
                           ((100, P, 3, 101, 5), -1), ((-1, P, 3, 0, 5), -1), ((100, P, 3, 50, 0), -1), ((1 << 29, P, 3, 50, 5), limit)):
            assert call(*args) == code, (name, args)
            assert name.encode() in lib.ln_last_error_string(), (name, args, lib.ln_last_error_string())
        if "nll" not in name:
            assert call(100, P, 3, 50, 1025) == -1 and name.encode() in lib.ln_last_error_string()
    assert lib.ln_lovasz_forward_ranges(P, P, 100, P, 3, 50, 5, -1, 2, P, 1 << 30, P, P, P, P, None) == -1
    assert lib.ln_nll_forward_ranges(P, P, 100, P, 3, 50, 5, -1, None, P, 8, P, P, P, None) == -1 and b"workspace" in lib.ln_last_error_string()
    assert lib.ln_nll_forward_ranges(P, P, 100, P, 3, 50, 5, -1, None, P, 1 << 30, None, P, P, None) == -1
    assert lib.ln_nll_backward_ranges(P, P, P, 0, P, 3, 0, 5, -1, None, P, None) == 0  # no row: nothing to do
    assert lib.ln_dice_backward_ranges(P, P, P, P, 0, P, 3, 0, 5, P, None) == 0
