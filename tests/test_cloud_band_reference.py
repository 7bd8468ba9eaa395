"""CPU checks of tests/cloud_band_reference.py (the reference the GPU band-check tests compare with) against hand-built cases, and of the
host-side key-range arithmetic of set_cloud_batch(check_band=True)."""
import numpy as np
import pytest

from tests import cloud_band_reference as R

INT_MAX, INT_MIN = R.INT_MAX, R.INT_MIN


def test_origin_has_the_keys_zero_to_d():
    """Position 0: elevated 0, remainder-0 point 0, all differences tie so rank[i] = i; vertex r has first key r: extent (0, d)."""
    for d in (1, 2, 3, 6):
        ext = R.cloud_key_extents(np.zeros((1, d), np.float32), np.ones(d), 1)
        assert ext.tolist() == [[0, d]]


def test_extents_are_min_and_max_per_cloud_of_the_oracle_keys():
    from oracle import lattice_oracle as O
    rng = np.random.default_rng(0)
    pos = (rng.uniform(-3, 3, (10, 3)) * np.array([1.0, 1.0, 1.0])).astype(np.float32)
    sig = np.array([0.5, 0.7, 0.9], np.float32)
    ext = R.cloud_key_extents(pos, sig, 4)  # clouds of 4, 4 and 2 points
    assert ext.shape == (3, 2) and ext.dtype == np.int32
    rem0, rank, _ = O.simplex(O.scale_positions(pos, sig))
    keys = O.simplex_keys(rem0, rank)
    for c, rows in enumerate((range(0, 4), range(4, 8), range(8, 10))):
        firsts = [int(keys[p, r, 0]) for p in rows for r in range(4)]
        assert ext[c].tolist() == [min(firsts), max(firsts)]


def one_point(x, d=3):
    p = np.zeros((1, d), np.float32)
    p[0, 0] = x
    return p


@pytest.mark.parametrize("x", [7.3, -7.3])
def test_verdict_at_the_edges_of_the_band(x):
    """One point; the band is laid around its measured extent (lo, hi).  hi < half - guard is strict, -half + guard <= lo is not."""
    (lo, hi), = R.cloud_key_extents(one_point(x), np.ones(3), 1).tolist()
    assert lo < hi and (hi > 8 if x > 0 else lo < -8)
    half = 4096
    if x > 0:
        assert R.band_verdict([[lo, hi]], 2 * half, half - hi) == (0, True)        # exactly on half - guard: outside
        assert R.band_verdict([[lo, hi]], 2 * half, half - hi - 1) == (INT_MAX, False)  # one key unit inside
        assert R.band_verdict([[lo, hi]], 2 * half, half - hi + 1) == (0, True)    # one key unit outside
    else:
        assert R.band_verdict([[lo, hi]], 2 * half, half + lo) == (INT_MAX, False)  # exactly on -half + guard: inside
        assert R.band_verdict([[lo, hi]], 2 * half, half + lo - 1) == (INT_MAX, False)
        assert R.band_verdict([[lo, hi]], 2 * half, half + lo + 1) == (0, True)     # one key unit outside


def test_first_offender_is_the_smallest_cloud_and_empty_clouds_pass():
    ext = [[-10, 10], [-200, 5], [INT_MAX, INT_MIN], [-300, 300]]
    assert R.band_verdict(ext, 256, 0) == (1, True)
    assert R.band_verdict(ext[:1] + ext[2:3], 256, 0) == (INT_MAX, False)
    # half = 128: hi = 10 < 128 - guard holds up to guard 117 (lo = -10 >= -128 + guard up to 118)
    assert R.band_verdict(ext[:1], 256, 117) == (INT_MAX, False) and R.band_verdict(ext[:1], 256, 118) == (0, True)


def test_empty_last_cloud_and_single_cloud():
    pos = np.concatenate([one_point(1.0), one_point(-2.0)])
    ext = R.cloud_key_extents(pos, np.ones(3), 2)
    assert ext.shape == (1, 2)  # B = 1
    a, b = R.cloud_key_extents(pos[:1], np.ones(3), 1)[0], R.cloud_key_extents(pos[1:], np.ones(3), 1)[0]
    assert ext[0].tolist() == [min(a[0], b[0]), max(a[1], b[1])]
    assert R.cloud_key_extents(np.zeros((0, 3), np.float32), np.ones(3), 5).shape == (0, 2)
    # a shorter last cloud: 3 points in clouds of 2
    ext = R.cloud_key_extents(np.concatenate([pos, one_point(5.0)]), np.ones(3), 2)
    assert ext.shape == (2, 2) and ext[1].tolist() == R.cloud_key_extents(one_point(5.0), np.ones(3), 1)[0].tolist()


@pytest.mark.parametrize("d, bits", [(3, 20), (4, 15), (6, 10)])
def test_host_key_range_arithmetic(d, bits):
    """README 'Key range': min(32, 60 // d) bits per quotient.  The product's closed form against the reference's search, and the
    ValueError of the check names the largest batch that fits."""
    from lattice_net_amd.lattice import _BandCheck, max_clouds_in_key_range
    assert min(32, 60 // d) == bits
    for q in (16, 32, 48, 1024, 8192, 1 << 14, 1 << 20):
        fits = R.max_clouds_in_key_range(d, q)
        assert max_clouds_in_key_range(d, q) == fits, (d, q)
        reach = 2 ** (bits - 1)
        # by hand: cloud c reaches c q + q / 2; the last one that fits has (B - 1) q + q / 2 <= 2^(bits - 1)
        assert fits == (0 if q // 2 > reach else (reach - q // 2) // q + 1)
        if fits:
            _BandCheck.check_key_range(d, q, fits)
        with pytest.raises(ValueError, match=f"largest batch that fits is {fits} clouds"):
            _BandCheck.check_key_range(d, q, fits + 1)
    assert R.max_clouds_in_key_range(3, 8192) == 64 and R.max_clouds_in_key_range(4, 8192) == 2 and R.max_clouds_in_key_range(6, 8192) == 0


def test_set_cloud_batch_checks_the_range_and_the_guard_on_the_host():
    from lattice_net_amd import Lattice
    lat = Lattice(sigmas=[1.0] * 6, capacity=1000)
    with pytest.raises(ValueError, match="largest batch that fits is 0 clouds"):
        lat.set_cloud_batch(100, check_band=True)  # 8192 cells: half a band is beyond the 512 quotients of d = 6
    lat.set_cloud_batch(100)  # unchecked: as before
    lat.set_cloud_batch(100, quotient_step=64, check_band=True)
    assert lat.m_hash_table._band.guard == 16 * 7
    with pytest.raises(ValueError, match="guard"):
        lat.set_cloud_batch(100, quotient_step=32, check_band=True)  # half = 112 key units = the default guard
    with pytest.raises(ValueError, match="guard"):
        lat.set_cloud_batch(100, quotient_step=64, check_band=True, guard=-1)
    lat.set_cloud_batch(None)
    assert lat.m_hash_table._band is None
