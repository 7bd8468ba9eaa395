"""The cloud-count limits of the per-cloud entry points on the host (no GPU).  The entry points that existed keep their limit of 64
clouds; their *_many siblings take 1024: 1024 row ranges / clouds pass the count check of every one of them, 1025 are
LN_ERR_UNSUPPORTED before anything is launched, and the workspace of the per-range GroupNorm keeps
its size up to 64 ranges and is the B x 2 C fp64 parameter-gradient terms beyond (the range-owner form of csrc/ln_norm.hip)."""
import ctypes as C

import pytest

from lattice_net_amd import _lib
from lattice_net_amd.lattice import Lattice

UNSUPPORTED, ARG = -2, -1
BIG = 1 << 40
LN_GN_REPLICAS = 32  # (include/latticenet_hip.h: the accumulator slab of a range is LN_GN_REPLICAS x 2 x C doubles)


def entry_points(lib, many=True):
    """name -> call(clouds) of the *_many entry points (many=False: of the entry points they extend) with every buffer a non-null dummy except ONE that is checked behind the cloud count: a call that gets past
    the count fails on it with LN_ERR_ARG and launches nothing."""
    csr = _lib.LnCsr(16, 16, 16, 16, 0, None, 0)
    t = _lib.LnTable(100, 3, 1, 1, 1, 1, 1, 1, 1)
    t.batch_points, t.batch_key_step = 10, 64
    f = {k: getattr(lib, k.replace("MANY_", "many_" if many else "")) for k in (
        "ln_group_norm_forward_MANY_segments", "ln_group_norm_backward_MANY_segments", "ln_pointnet_reduce_forward_MANY_clouds",
        "ln_distribute_centre_MANY_clouds", "ln_distribute_centre_MANY_cloud_starts")}
    f["ln_cloud_row_starts"] = lib.ln_cloud_row_starts_many if many else lib.ln_cloud_row_starts
    return {
        "ln_group_norm_forward_segments": lambda b: f["ln_group_norm_forward_MANY_segments"](16, None, None, 100, 8, 2, 1e-5, 0, 16, 16, 16, 16, BIG, None,
                                                                                       0, None, None, b, None),  # null row_starts
        "ln_group_norm_backward_segments": lambda b: f["ln_group_norm_backward_MANY_segments"](16, 16, None, 16, 16, 100, 8, 2, 0, 16, None, None, 16, BIG,
                                                                                         None, 0, None, None, b, None),  # null row_starts
        "ln_pointnet_reduce_forward_clouds": lambda b: f["ln_pointnet_reduce_forward_MANY_clouds"](C.byref(csr), None, 5, 16, 8, 16, 5, 10, 4, 16, 1 << 20, 16,
                                                                                             16, None, b, None),  # null row_starts
        "ln_distribute_centre_clouds": lambda b: f["ln_distribute_centre_MANY_clouds"](16, 16, 16, 16, 10, 5, 3, 4, None, b, 16, None),  # null row_starts
        "ln_distribute_centre_cloud_starts": lambda b: f["ln_distribute_centre_MANY_cloud_starts"](16, 16, 16, 16, 10, 5, 3, 4, None, 16, b, 16, None),
        "ln_cloud_row_starts": lambda b: f["ln_cloud_row_starts"](C.byref(t), 10, b, None, 16, None),  # null output
    }


def test_1025_clouds_are_refused_and_1024_pass_the_count_check():
    lib = _lib.load()
    for name, call in entry_points(lib).items():
        assert call(1025) == UNSUPPORTED, name
        message = lib.ln_last_error_string()
        assert b"1024" in message and b"1025" in message, (name, message)
        assert call(0) == UNSUPPORTED, name
        for clouds in (65, 1024):
            assert call(clouds) == ARG, (name, clouds)  # past the count, stopped by the null buffer
            assert b"null" in lib.ln_last_error_string(), (name, clouds, lib.ln_last_error_string())


def test_the_entry_points_that_existed_keep_their_limit():
    lib = _lib.load()
    for name, call in entry_points(lib, many=False).items():
        assert call(65) == UNSUPPORTED and call(1024) == UNSUPPORTED, name
        assert b"64" in lib.ln_last_error_string(), name
        assert call(64) == ARG, name


def test_new_kernels_are_registered():
    names = _lib.load().ln_kernel_names().decode().split(",")
    for k in ("k_gn_forward_range_owner", "k_gn_backward_range_owner", "k_pointnet_reduce_decode_many_clouds"):
        assert k in names


@pytest.mark.parametrize("c", [4, 32, 64, 1024])
def test_workspace_of_the_per_range_group_norm(c):
    lib = _lib.load()
    slab = LN_GN_REPLICAS * 2 * c * 8
    assert lib.ln_group_norm_workspace_bytes(c) == slab
    for s in range(1, 65):  # the header's formula: `segments` slabs, then segments x 2 C doubles
        assert lib.ln_group_norm_segments_workspace_bytes(c, s) == s * (slab + 2 * c * 8), s
    prev = 0
    for s in range(65, 1025):  # the range-owner form: segments x 2 C doubles, no slab
        got = lib.ln_group_norm_segments_workspace_bytes(c, s)
        assert got >= s * 2 * c * 8 and got >= prev, s
        prev = got
    # what the feature is for: no 32 KB slab per range to zero at 1024 ranges
    assert lib.ln_group_norm_segments_workspace_bytes(c, 1024) < lib.ln_group_norm_segments_workspace_bytes(c, 64)


def test_a_too_small_workspace_is_refused_at_many_ranges():
    lib = _lib.load()
    need = lib.ln_group_norm_segments_workspace_bytes(8, 200)
    call = lambda nbytes: lib.ln_group_norm_backward_many_segments(16, 16, None, 16, 16, 100, 8, 2, 0, 16, None, None, 16, nbytes, None, 0, None, 16, 200,
                                                              None)
    assert call(need - 1) == ARG and b"workspace" in lib.ln_last_error_string()


def test_set_cloud_batch_names_the_limit():
    """many_clouds=True lifts the limit of the per-cloud switches from 64 to 1024; without it a call is what it was."""
    assert Lattice.MAX_BATCH_CLOUDS == 1024 and Lattice.DEFAULT_MAX_BATCH_CLOUDS == 64
    lat = Lattice(sigmas=[0.9, 0.9, 0.9], capacity=1000)
    for switch in ("per_cloud_norm", "per_cloud_invalid_vertex"):
        with pytest.raises(ValueError, match="at most 1024"):
            lat.set_cloud_batch([1] * 1025, many_clouds=True, **{switch: True})
        with pytest.raises(ValueError, match="at most 64 .1024 with many_clouds=True"):
            lat.set_cloud_batch([1] * 65, **{switch: True})
        lat.set_cloud_batch([1] * 1024, many_clouds=True, **{switch: True})  # accepted
        assert len(lat.cloud_lengths()) == 1024 and lat.m_hash_table._many_clouds
        assert Lattice._clone_of(lat).m_hash_table._many_clouds  # (coarser levels and clones inherit it)
        lat.set_cloud_batch([1] * 65, many_clouds=True, **{switch: True})
        assert len(lat.cloud_lengths()) == 65
        lat.set_cloud_batch([1] * 3, **{switch: True})
        assert not lat.m_hash_table._many_clouds
