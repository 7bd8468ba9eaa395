"""Row ranges of a batch of clouds, without a GPU: the NumPy restatement the GPU tests hold k_cloud_row_starts to
(tests/cloud_batch_reference.py) against brute force, the per-point ranges, the host-side refusals of Lattice.cloud_row_starts()
(no device work), and the ABI of the per-range GroupNorm (argument errors are reported by the host half of the library)."""
import numpy as np
import pytest

from tests import cloud_batch_reference as B


def brute_force_starts(cloud_of_row, clouds):
    rows = len(cloud_of_row)
    return [next((r for r in range(rows) if cloud_of_row[r] >= c), rows) for c in range(clouds + 1)]


@pytest.mark.parametrize("sizes", [[3, 1, 4], [0, 5, 0, 0, 2, 0], [0, 0, 0], [1], [7, 0, 1, 0]])
def test_row_starts_of_cloud_major_rows(sizes):
    """Clouds without a vertex start where the next one does; the last entry is the row count; the flag is 0."""
    cloud_of_row = np.repeat(np.arange(len(sizes)), sizes)
    starts, flag = B.row_starts_of_clouds(cloud_of_row, len(sizes))
    assert flag == 0
    assert list(starts) == brute_force_starts(cloud_of_row, len(sizes)) == list(np.concatenate([[0], np.cumsum(sizes)]))


def test_rows_that_are_not_cloud_major_raise_the_flag():
    assert B.row_starts_of_clouds([0, 0, 1, 0, 2], 3) == (None, 1)
    assert B.row_starts_of_clouds([2, 2, 2], 3)[1] == 0
    assert B.row_starts_of_clouds([1, 0], 2)[1] == 1


def test_cloud_of_key_at_every_level():
    """Cloud c sits at c * step with the cloud within half a step of the origin; a coarser level halves keys and step alike."""
    step, clouds = (1 << 13) * 4, 5
    rng = np.random.default_rng(0)
    for lvl in range(4):
        st = step >> lvl
        local = rng.integers(-(st // 2) + 1, st // 2, size=1000)  # strictly inside half a step
        c = rng.integers(0, clouds, size=1000)
        assert np.array_equal(B.cloud_of_key(local + c * st, st, clouds), c)
    assert list(B.cloud_of_key([-1, 0, step // 2 - 1, step // 2, step, -step], step, clouds)) == [0, 0, 0, 1, 1, 0]  # (clamped into the batch)


def test_row_starts_of_splat_indices():
    # 3 clouds x 2 points x 2 tokens; cloud 1 touches no vertex of its own (all -1)
    idx = [0, 1, 1, 2, -1, -1, -1, -1, 3, 3, 4, 3]
    starts, flag = B.row_starts_of_splat_indices(idx, 2, 2, 3, 5)
    assert flag == 0 and list(starts) == [0, 3, 3, 5]
    with pytest.raises(AssertionError, match="shared"):
        B.row_starts_of_splat_indices([0, 1, 1, 2], 1, 2, 2, 3)


def test_segments_are_clamped_like_the_kernels():
    assert B.segments([0, 1, 38, 38, 337], 400) == ([(0, 1), (1, 38), (38, 38), (38, 337)], 337)
    assert B.segments([0, 1, 38, 38, 337], 400, rows=200) == ([(0, 1), (1, 38), (38, 38), (38, 200)], 200)
    assert B.segments([0, 50, 40, 500], 100) == ([(0, 50), (50, 50), (40, 100)], 100)  # (whatever row_starts holds: lo <= hi, inside the tensor)


def test_cloud_point_ranges():
    from lattice_net_amd.lattice import cloud_point_ranges
    assert cloud_point_ranges(900, 300) == [0, 300, 600, 900]
    assert cloud_point_ranges(900, 300, 4) == [0, 1200, 2400, 3600]
    assert cloud_point_ranges(700, 300) == [0, 300, 600, 700]  # (the last cloud takes what is left)
    assert cloud_point_ranges(0, 300) == [0]
    n0, k = 7, 3
    for n in range(0, 30):
        got = np.array(cloud_point_ranges(n, n0, k))
        cloud_of_row = np.repeat(np.arange(n) // n0, k)
        assert list(got) == brute_force_starts(cloud_of_row, -(-n // n0))
    with pytest.raises(ValueError):
        cloud_point_ranges(10, 0)


def test_cloud_row_starts_refuses_on_the_host():
    """No batch, or a lattice that was never built from a batch of positions: an error before anything touches a device."""
    import lattice_net_amd as L
    from lattice_net_amd import _lib
    lat = L.Lattice(sigmas=[1.0, 1.0, 1.0], capacity=1000, device="cpu")
    with pytest.raises(_lib.LatticeNetHipError, match="no cloud batch"):
        lat.cloud_row_starts()
    assert lat.per_cloud_norm_row_starts() is None and lat.cloud_segments() == 1
    lat.set_cloud_batch(100, per_cloud_norm=True)
    assert lat.m_hash_table._per_cloud_norm and lat.m_hash_table._batch == (100, (1 << 13) * 4)
    with pytest.raises(_lib.LatticeNetHipError, match="not built from a batch"):
        lat.cloud_row_starts()
    lat.set_cloud_batch(100)  # the default keeps today's behaviour
    assert not lat.m_hash_table._per_cloud_norm and lat.per_cloud_norm_row_starts() is None
    lat.set_cloud_batch(None, per_cloud_norm=True)  # no batch: nothing to normalise per cloud
    assert not lat.m_hash_table._per_cloud_norm


def test_segment_entry_points_reject_bad_sizes():
    from lattice_net_amd import _lib
    lib = _lib.load()
    assert lib.ln_group_norm_segments_workspace_bytes(64, 1) == lib.ln_group_norm_workspace_bytes(64) + 2 * 64 * 8
    assert lib.ln_group_norm_segments_workspace_bytes(64, 16) == 16 * lib.ln_group_norm_segments_workspace_bytes(64, 1)
    big = 1 << 40
    fwd = lambda m, c, groups, segs, ws=16, starts=16: lib.ln_group_norm_forward_segments(16, None, None, m, c, groups, 1e-5, 0, 16, 16, 16, ws, big, None, 0,
                                                                                          None, starts, segs, None)
    bwd = lambda m, c, groups, segs: lib.ln_group_norm_backward_segments(16, 16, None, 16, 16, m, c, groups, 0, 16, None, None, 16, big, None, 0, None, 16,
                                                                         segs, None)
    for call in (fwd, bwd):
        assert call(100, 6, 3, 2) == -2 and call(100, 1028, 2, 2) == -2 and call(0, 8, 2, 2) == -2  # channels % 4, <= 1024, rows >= 1
        assert call(100, 8, 3, 2) == -1  # groups do not divide the channels
        assert call(100, 8, 2, 0) == -2 and call(100, 8, 2, 65) == -2  # 1 <= row ranges <= 64
        assert b"row ranges" in lib.ln_last_error_string()
    assert fwd(100, 8, 2, 2, starts=None) == -1 and fwd(100, 8, 2, 2, ws=None) == -1
    assert lib.ln_group_norm_forward_segments(16, None, None, 100, 8, 2, 1e-5, 0, 16, 16, 16, 16, 8, None, 0, None, 16, 2, None) == -1  # workspace too small
    t = _lib.LnTable(100, 3, 1, 1, 1, 1, 1, 1, 1)
    import ctypes as C
    assert lib.ln_cloud_row_starts(C.byref(t), 10, 2, 16, 16, None) == -1 and b"no batch" in lib.ln_last_error_string()
    t.batch_points, t.batch_key_step = 10, 64
    assert lib.ln_cloud_row_starts(C.byref(t), 10, 65, 16, 16, None) == -2
    assert lib.ln_cloud_row_starts(C.byref(t), 10, 2, None, 16, None) == -1
    names = lib.ln_kernel_names().decode().split(",")
    for k in ("k_cloud_row_starts", "k_gn_stats_segments", "k_gn_apply_segments", "k_gn_backward_apply_segments", "k_gn_param_grads_segments"):
        assert k in names
