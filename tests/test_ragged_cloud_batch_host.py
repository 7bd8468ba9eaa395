"""Host side of cloud batches of unequal sizes (Lattice.set_cloud_batch([...]), LnTableClouds.batch_point_starts): row ranges, argument checks
and the C ABI's refusals.  No GPU is touched."""
import ctypes as C

import pytest
import torch

from lattice_net_amd import Lattice, _lib
from lattice_net_amd.lattice import cloud_point_ranges


def plain_ranges(lengths, k):
    out, at = [0], 0
    for length in lengths:
        at += length
        out.append(at * k)
    return out


@pytest.mark.parametrize("lengths", [(300, 173, 41), (1, 0, 64, 65), (0, 0, 5), (7,), (0,), (3, 0, 0)])
@pytest.mark.parametrize("k", [1, 4])  # per-point rows, and the d + 1 = 4 token rows of a point at d = 3
def test_ragged_ranges_against_a_plain_loop(lengths, k):
    got = cloud_point_ranges(sum(lengths), list(lengths), k)
    assert got == plain_ranges(lengths, k)
    assert len(got) == len(lengths) + 1 and got[0] == 0 and got[-1] == sum(lengths) * k
    assert cloud_point_ranges(sum(lengths), tuple(lengths), k) == got


def test_ragged_ranges_refuse_a_wrong_sum_and_bad_lengths():
    with pytest.raises(ValueError, match="sum to 514"):
        cloud_point_ranges(515, [300, 173, 41])
    with pytest.raises(ValueError):
        cloud_point_ranges(5, [6, -1])
    with pytest.raises(ValueError):
        cloud_point_ranges(0, [])
    with pytest.raises(ValueError):
        cloud_point_ranges(3, [1.5, 1.5])
    assert cloud_point_ranges(10, 4) == [0, 4, 8, 10]  # the int form is what it was
    assert cloud_point_ranges(10, 4, 4) == [0, 16, 32, 40]


def new_lattice():
    return Lattice(sigmas=[0.9, 0.9, 0.9], capacity=1000)


def test_set_cloud_batch_checks_the_lengths():
    lat = new_lattice()
    with pytest.raises(ValueError, match="lengths"):
        lat.set_cloud_batch([300, -1, 41])
    with pytest.raises(ValueError, match="lengths"):
        lat.set_cloud_batch([])
    with pytest.raises(ValueError, match="at most 64"):
        lat.set_cloud_batch([1] * 65, per_cloud_norm=True)
    with pytest.raises(ValueError, match="at most 64"):
        lat.set_cloud_batch([1] * 65, per_cloud_invalid_vertex=True)
    with pytest.raises(ValueError, match="quotient_step"):
        lat.set_cloud_batch([3, 4], quotient_step=100)
    assert lat.cloud_lengths() == [] and lat.points_per_cloud() == 0  # nothing was set by a refused call


def test_ragged_batch_has_lengths_and_no_stride():
    lat = new_lattice()
    lat.set_cloud_batch([300, 173, 41])
    assert lat.cloud_lengths() == [300, 173, 41]
    with pytest.raises(ValueError, match=r"cloud_lengths\(\)"):
        lat.points_per_cloud()
    lat.set_cloud_batch([1] * 65)  # more than 64 clouds are fine without a per-cloud switch
    assert len(lat.cloud_lengths()) == 65
    lat.set_cloud_batch(100)  # the int form: a stride again
    assert lat.points_per_cloud() == 100 and lat.cloud_lengths(250) == [100, 100, 50]
    lat.set_cloud_batch(None)
    assert lat.points_per_cloud() == 0 and lat.cloud_lengths() == []


def test_positions_must_hold_the_whole_batch():
    lat = new_lattice()
    lat.set_cloud_batch([300, 173, 41])
    values = torch.zeros((513, 1))
    with pytest.raises(ValueError, match="sum to 514 points but the positions have 513 rows"):
        lat.just_create_verts(torch.zeros((513, 3)), False)
    with pytest.raises(ValueError, match="sum to 514 points but the positions have 513 rows"):
        lat.splat_standalone(torch.zeros((513, 3)), values)
    with pytest.raises(ValueError, match="sum to 514 points but the positions have 513 rows"):
        lat.distribute(torch.zeros((513, 3)), values)


def test_new_symbols_and_the_zero_table():
    lib = _lib.load()
    assert hasattr(lib, "ln_cloud_point_starts_check") and hasattr(lib, "ln_distribute_centre_cloud_starts")
    names = lib.ln_kernel_names().decode().split(",")
    for k in ("k_cloud_point_starts_check", "k_cloud_key_extents_ranges", "k_distribute_centre_cloud_starts"):
        assert k in names
    # LnTable keeps its layout; the starts live behind it in an LnTableClouds, whose head is tagged
    assert C.sizeof(_lib.LnTable) == 120 and _lib.LnTableClouds.table.offset == 0
    assert _lib.LnTableClouds.batch_point_starts.offset == 120 and _lib.LnTableClouds.batch_clouds.offset == 128
    assert C.sizeof(_lib.LnTableClouds) == 136
    assert _lib.LnTable().batch_points == 0  # a zero-initialised LnTable is a plain table: nothing behind it is read
    c = _lib.LnTableClouds()
    assert c.batch_point_starts is None and c.batch_clouds == 0 and c.table.batch_points == _lib.LN_BATCH_POINT_STARTS == -1
    c = _lib.LnTableClouds((100, 3, 1, 1, 1, 1, 1, 1, 1), 4096, 3)
    head = c.table
    head.host_seq = 7  # the head is a view of the struct's memory, not a copy
    assert (c.table.capacity, c.table.pos_dim, c.table.host_seq, c.batch_point_starts, c.batch_clouds) == (100, 3, 7, 4096, 3)
    assert C.addressof(head) == C.addressof(c)
    assert _lib.LN_STATUS_CLOUD_STARTS == 16


def test_refusals_launch_nothing():
    lib = _lib.load()
    assert lib.ln_cloud_point_starts_check(None, 3, 10, 16, None) == -1 and b"null" in lib.ln_last_error_string()
    assert lib.ln_cloud_point_starts_check(16, 3, 10, None, None) == -1
    assert lib.ln_cloud_point_starts_check(16, 0, 10, 16, None) == -1
    assert lib.ln_cloud_point_starts_check(16, 3, -1, 16, None) == -1
    dc = lib.ln_distribute_centre_cloud_starts
    assert dc(16, 16, 16, 16, 40, 5, 3, 4, None, 16, 3, 16, None) == -1 and b"point_starts" in lib.ln_last_error_string()
    assert dc(16, 16, 16, 16, 40, 5, 3, 0, 16, 16, 3, 16, None) == -1
    assert dc(16, 16, 16, 16, 40, 5, 3, 4, 16, 16, 65, 16, None) == -2
    assert dc(16, 16, 16, 16, 40, 5, 3, 4, 16, 16, 0, 16, None) == -2
    assert dc(16, 16, 16, 16, 0, 5, 3, 4, 16, 16, 3, 16, None) == 0  # no token: nothing to do
    for starts, clouds in ((16, 0), (None, 3)):  # a tagged table must bring a list and at least one cloud
        c = _lib.LnTableClouds((100, 3, 1, 1, 1, 1, 1, 1, 1), starts, clouds)
        c.table.batch_key_step = 64
        assert lib.ln_cloud_key_extents(C.byref(c.table), 16, _lib.host_floats([1, 1, 1]), 10, 0, 16, 16, None) == -1
        assert b"LN_BATCH_POINT_STARTS" in lib.ln_last_error_string()
        assert lib.ln_slice_no_precomputation(C.byref(c.table), 16, 16, _lib.host_floats([1, 1, 1]), 10, 1, 16, 16, 16, None) == -1
