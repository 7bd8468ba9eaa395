"""NumPy reference of the band check of a cloud batch (ln_cloud_key_extents): per-cloud extents of the first key coordinate from the
oracle's key computation (oracle/lattice_oracle.py: scale, elevate, simplex, simplex_keys), the verdict, and the host-side key-range
arithmetic.  Everything is integer-exact."""
import numpy as np

from oracle import lattice_oracle as O

INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


def cloud_key_extents(positions_raw, sigmas, points_per_cloud):
    """int32 [B, 2]: smallest and largest first key coordinate over the d + 1 simplex vertices of every point of cloud c (rows
    c n0 ... of the positions), before the cloud's shift; (INT_MAX, INT_MIN) for a cloud without a point.  B = ceil(n / n0)."""
    pos = np.asarray(positions_raw, dtype=np.float32)
    n, d = pos.shape
    n0 = int(points_per_cloud)
    clouds = -(-n // n0)
    out = np.empty((clouds, 2), dtype=np.int32)
    out[:, 0], out[:, 1] = INT_MAX, INT_MIN
    if n == 0:
        return out
    rem0, rank, _ = O.simplex(O.scale_positions(pos, np.asarray(sigmas, dtype=np.float32)))
    k0 = O.simplex_keys(rem0, rank)[:, :, 0]  # [n, d + 1]
    for c in range(clouds):
        k = k0[c * n0:(c + 1) * n0]
        if k.size:
            out[c] = (k.min(), k.max())
    return out


def band_verdict(extents, key_step, guard):
    """(first offending cloud or INT_MAX, status bit set?): cloud c is inside when -half + guard <= lo and hi < half - guard, half =
    key_step >> 1; an empty cloud is inside."""
    half = int(key_step) >> 1
    for c, (lo, hi) in enumerate(np.asarray(extents).tolist()):
        if lo > hi:
            continue
        if not (-half + guard <= lo and hi < half - guard):
            return c, True
    return INT_MAX, False


def max_clouds_in_key_range(pos_dim, quotient_step):
    """Largest B with every quotient of clouds 0..B-1, [c q - q / 2, c q + q / 2), packable: |quotient| <= 2^(bits - 1) with bits =
    min(32, 60 // d) (README 'Key range'), and the key (d + 1) x quotient inside int32.  By search, not by the closed form."""
    d, q = int(pos_dim), int(quotient_step)
    reach = min(2 ** (min(32, 60 // d) - 1), 2 ** 31 // (d + 1))
    fits = 0
    while fits * q + q // 2 <= reach and fits < 1 << 20:
        fits += 1
    return fits

