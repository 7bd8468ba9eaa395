"""Host side of tests/test_gpu_key_coarsen.py and tests/test_gpu_position_lookup.py: the clouds of every case, the oracle's tables for
them (built once per process), an exact integer restatement of the key-built coarse level that can stop after a number of fine rows,
and the conditions that keep the cases from being vacuous.  tests/test_table_reference.py evaluates all of it without a GPU.

The key-built coarse level (LatticeGPU.cuh:2348-2511, oracle `coarsen_keys`): every fine vertex whose d + 1 coordinates (the d stored
ones and the implied -sum) are all even is a seed.  A seed hands out up to 2 (d + 1) + 1 tokens, in this order: the centre key / 2, then
per axis the coarse neighbour `np` (+1 everywhere, -d on the axis) if the FINE np neighbour exists, then `nm` (-1 everywhere, +d on the
axis) if the fine nm neighbour exists.  Coarse row r is the r-th first occurrence of a key in (fine row, token) order.  `coarsen_rows`
works on integers and a set of the fine keys, so it takes the fine rows in ANY numbering: handed the keys as the device numbered
them, it gives the coarse order that numbering must produce."""
import functools

import numpy as np

from oracle import lattice_oracle as O

F32 = np.float32
CAP = 60000  # slots of the oracle's tables and of the device tables of the main cases (loads of a few per cent: no probe limit in sight)
RAW_BITS = {d: min(32, 63 // d) for d in range(1, 7)}  # bits per coordinate of the raw key format (csrc/ln_common.h, KeyPack<D>::BITS)


def sigmas(d, sigma):
    return np.full((d,), sigma, F32)


def oracle_build(pos, sigma, cap=CAP, table=None):
    """(table, idx, w) of the oracle's serial build; `table`: insert into an existing one (incremental build)"""
    d = pos.shape[1]
    t = O.OracleHashTable(cap, d) if table is None else table
    idx, w = O.build_splat(t, O.scale_positions(pos, sigmas(d, sigma)))
    return t, idx, w


def keys_of(t):
    return t.keys[: t.nr_filled]


def raw_range(d):
    b = RAW_BITS[d]
    return -(1 << (b - 1)), (1 << (b - 1)) - 1


# ------------------------------------------------------------------------------------------------------------------ coarsening
def coarsen_rows(fine_keys, rows=None):
    """The key-built coarse level of the fine rows [0, rows) (all of them by default), lookups answered by the WHOLE fine table.
    Returns a dict: keys [mc, d] int32 in first-occurrence order, tokens (fine row, token, coarse key), seeds, with_existing /
    with_missing (seeds with at least one existing / missing np or nm neighbour), shared (coarse keys that two different fine rows
    produce)."""
    fk = np.asarray(fine_keys, np.int64)
    m, d = fk.shape
    rows = m if rows is None else max(0, min(int(rows), m))
    present = set(map(tuple, fk.tolist()))
    full = np.concatenate([fk, -fk.sum(axis=1, keepdims=True)], axis=1)
    seeds = np.nonzero(~((full[:rows] & 1).any(axis=1)))[0]
    tokens, with_existing, with_missing = [], 0, 0
    for r in seeds.tolist():
        k = full[r]
        half = k // 2  # exact: every coordinate is even
        tokens.append((r, 0, tuple(half[:d].tolist())))
        found = 0
        for a in range(d + 1):
            for j, s in ((1 + 2 * a, 1), (2 + 2 * a, -1)):
                nk = k + s
                nk[a] = k[a] - s * d
                if tuple(nk[:d].tolist()) in present:
                    ck = half + s
                    ck[a] = half[a] - s * d
                    tokens.append((r, j, tuple(ck[:d].tolist())))
                    found += 1
        with_existing += found > 0
        with_missing += found < 2 * (d + 1)
    first, producers = {}, {}
    for r, _, ck in tokens:
        first.setdefault(ck, len(first))
        producers.setdefault(ck, set()).add(r)
    keys = np.asarray(list(first), np.int32).reshape(len(first), d)
    return dict(keys=keys, tokens=tokens, seeds=len(seeds), with_existing=with_existing, with_missing=with_missing,
                shared=sum(len(p) > 1 for p in producers.values()))


def fits_raw_format(keys):
    """Every stored coordinate of every key inside the raw key format of its dimension"""
    keys = np.asarray(keys)
    lo, hi = raw_range(keys.shape[1])
    return bool(keys.size == 0 or (keys.min() >= lo and keys.max() <= hi))


def oracle_coarse(t_fine, cap=CAP):
    """The oracle's own serial coarsening of an oracle table -> coarse oracle table"""
    tc = O.OracleHashTable(cap, t_fine.pos_dim)
    O.coarsen_keys(t_fine, tc)
    return tc


def table_of_keys(keys, cap=CAP):
    """Oracle table holding `keys` in this order (row r = keys[r])"""
    keys = np.asarray(keys, np.int32)
    t = O.OracleHashTable(cap, keys.shape[1])
    rows = t.insert(keys)
    assert np.array_equal(rows, np.arange(len(keys))), "the keys must be distinct"
    return t


def assert_coarsen_conditions(c, what=""):
    """What keeps a comparison of coarse levels from being vacuous (asserted on the CPU and again in the GPU test)"""
    assert len(c["keys"]) >= 20, (what, "fewer than 20 coarse vertices", len(c["keys"]))
    assert c["with_existing"] >= 1, (what, "no seed with an existing np / nm neighbour")
    assert c["with_missing"] >= 1, (what, "no seed with a missing np / nm neighbour")
    assert c["shared"] >= 1, (what, "no coarse key produced by two fine rows: the first-occurrence rule is idle")


def row_permutation(keys_a, keys_b):
    """perm[row of a] = row of b; asserts that both hold the same set of keys"""
    keys_a, keys_b = np.asarray(keys_a), np.asarray(keys_b)
    assert keys_a.shape == keys_b.shape, (keys_a.shape, keys_b.shape)
    oa, ob = np.lexsort(keys_a.T[::-1]), np.lexsort(keys_b.T[::-1])
    assert np.array_equal(keys_a[oa], keys_b[ob]), "vertex sets differ"
    perm = np.empty(len(oa), np.int64)
    perm[oa] = ob
    return perm


# ------------------------------------------------------------------------------------------------------------------ the clouds
# d -> (points, half extent of the box, sigma): a fine level of a few thousand vertices; about one in 2^d of them is a seed, so the
# higher dimensions pack their points into fewer cells
MAIN = {1: (1500, 300.0, 0.3), 2: (2500, 6.0, 0.3), 3: (1500, 1.8, 0.3), 4: (3000, 1.1, 0.3), 5: (1000, 0.6, 0.3), 6: (3000, 0.55, 0.3)}


@functools.lru_cache(maxsize=None)
def main_cloud(d):
    n, extent, sigma = MAIN[d]
    rng = np.random.default_rng(700 + d)
    return rng.uniform(-extent, extent, (n, d)).astype(F32), sigma


@functools.lru_cache(maxsize=None)
def main_oracle(d):
    """(fine table, idx, w, coarse table) of the main cloud"""
    pos, sigma = main_cloud(d)
    t, idx, w = oracle_build(pos, sigma)
    return t, idx, w, oracle_coarse(t)


def simplex_keys_of(points, sigma):
    """[n, d + 1, d] keys of the simplex vertices of raw points"""
    pts = np.asarray(points, F32)
    rem0, rank, _ = O.simplex(O.scale_positions(pts, sigmas(pts.shape[1], sigma)))
    return O.simplex_keys(rem0, rank)


def seeds_of(keys):
    """mask of the all-even keys ([..., d] stored coordinates; the implied one is -sum)"""
    keys = np.asarray(keys, np.int64)
    return ~((keys & 1).any(axis=-1) | ((keys.sum(axis=-1) & 1) != 0))


# a vertex of remainder r has stored coordinates (d + 1) q + r: for even d + 1 (d = 1, 3, 5) every coordinate of the remainder-0 vertex
# of ANY simplex is even, so only the even dimensions have points without a seed
NO_SEED_DIMS = (2, 4, 6)


@functools.lru_cache(maxsize=None)
def no_seed_points(d, count):
    """`count` points of the main cloud none of whose simplex vertices is all-even"""
    pos, sigma = main_cloud(d)
    ok = ~seeds_of(simplex_keys_of(pos, sigma)).any(axis=1)
    assert ok.sum() >= count, (d, "no point without a seed")
    return pos[np.nonzero(ok)[0][:count]].copy(), sigma


@functools.lru_cache(maxsize=None)
def one_point_with_a_seed(d):
    pos, sigma = main_cloud(d)
    has = seeds_of(simplex_keys_of(pos, sigma)).any(axis=1)
    return pos[np.nonzero(has)[0][:1]].copy(), sigma


CLAMP_DIMS = (1, 3, 6)      # dimensions of the fine_rows_upper cases
TWO_LEVEL_DIMS = (2, 3)     # a second coarsening, of a fine table in the raw key format
ONE_POINT_DIMS = (1, 3)     # the smallest fine level: the d + 1 vertices of one point
BLOCK_EDGE_COUNTS = (255, 256, 257)  # fine vertex counts around the 256-row workgroup of k_insert_coarse (d = 3)


@functools.lru_cache(maxsize=None)
def points_for_vertex_count(target, d=3):
    """A subset of the main cloud (in cloud order) whose fine level has exactly `target` vertices: a point is taken while its new
    vertices still fit under the target"""
    pos, sigma = main_cloud(d)
    keys = simplex_keys_of(pos, sigma)
    have, take = set(), []
    for p in range(len(pos)):
        new = {tuple(k) for k in keys[p].tolist()} - have
        if len(have) + len(new) <= target:
            have |= new
            take.append(p)
        if len(have) == target:
            break
    assert len(have) == target, (target, len(have))
    return pos[take].copy(), sigma


# wide clouds (the recipe of test_lattice_key_format_covers_wide_clouds): (d, reach) -> whether the halved keys fit the raw format
WIDE = {(5, 3500): True, (5, 4600): False, (6, 900): True, (6, 1150): False}
WIDE_CAP = 40000
WIDE_POINTS = {5: 600, 6: 3000}  # (at d = 5 every second vertex is a seed: fewer points keep the oracle's serial loop short)


@functools.lru_cache(maxsize=None)
def wide_cloud(d, reach):
    """WIDE_POINTS[d] points stretched so that the largest lattice coordinate of the fine level lands near `reach` units: beyond the raw key
    format (+-2048 at d = 5, +-512 at d = 6), inside the lattice format.  Returns (positions, fine oracle table, idx, w); sigma is 1."""
    rng = np.random.default_rng(50 + d)
    unit = rng.uniform(-1.0, 1.0, (WIDE_POINTS[d], d)).astype(F32)
    t0 = O.OracleHashTable(WIDE_CAP, d)
    O.build_splat(t0, O.scale_positions(unit * 100.0, np.ones((d,), F32)), False)
    spread = 100.0 * reach / float(np.abs(keys_of(t0)).max())
    pos = (unit * spread).astype(F32)
    t, idx, w = oracle_build(pos, 1.0, WIDE_CAP)
    return pos, t, idx, w


@functools.lru_cache(maxsize=None)
def wide_oracle_coarse(d, reach):
    return oracle_coarse(wide_cloud(d, reach)[1], WIDE_CAP)


# ------------------------------------------------------------------------------------------------------------------ position lookups
LOOKUP_CASES = [(1, 1, 1500), (2, 3, 1500), (3, 64, 1500), (4, 65, 1500), (5, 1, 1500), (6, 3, 1500),
                (1, 65, 0), (2, 64, 1), (3, 3, 256), (4, 1, 257), (5, 64, 257), (6, 65, 256)]  # (d, value width, queries)
KINDS = ("cloud", "shell", "far")


def queries(pos, sigma, n, seed, extent=None):
    """n query points of three kinds in one array, shuffled: points of the build cloud; shell points (every second one a cloud point
    pushed through a face of the cloud's box by up to 1.5 sigma, the others a cloud point moved by 0.9 sigma along one axis, into a
    neighbouring simplex: some simplex vertices absent); points 40 sigma and more beyond the box along every axis (all absent).
    Returns (q [n, d], kind [n])."""
    pos = np.asarray(pos, F32)
    d = pos.shape[1]
    rng = np.random.default_rng(seed)
    extent = float(np.abs(pos).max()) if extent is None else float(extent)
    kind = np.arange(n) % 3
    rng.shuffle(kind)
    q = pos[rng.integers(0, len(pos), n)].copy()
    shell = np.nonzero(kind == 1)[0]
    axis = rng.integers(0, d, len(shell))
    side = rng.choice(np.array([-1.0, 1.0], F32), len(shell))
    pushed = side * (extent + rng.uniform(0.0, 1.5, len(shell)).astype(F32) * F32(sigma))
    moved = q[shell, axis] + side * F32(0.9 * sigma)
    q[shell, axis] = np.where(np.arange(len(shell)) % 2 == 0, pushed, moved).astype(F32)
    far = np.nonzero(kind == 2)[0]
    q[far] = side_sign(rng, len(far), d) * (F32(extent + 40.0 * sigma) + rng.uniform(0.0, extent, (len(far), d)).astype(F32))
    return np.ascontiguousarray(q, F32), kind


def lookup_calls(d, n):
    """The calls of a lookup case with n queries: one call of the three kinds mixed; n = 1: three calls, one query of each kind; n = 0:
    one empty call.  [(q, kind)]"""
    pos, sigma = main_cloud(d)
    extent = MAIN[d][1]
    if n == 0:
        return [(np.zeros((0, d), F32), np.zeros((0,), np.int64))]
    if n == 1:
        q, kind = queries(pos, sigma, 3, 31 * d + 1, extent)
        return [(q[i:i + 1].copy(), kind[i:i + 1].copy()) for i in range(3)]
    return [queries(pos, sigma, n, 31 * d + n, extent)]


def side_sign(rng, n, d):
    """one sign per query, the same along every axis: a far query sits on a diagonal of the box"""
    return np.repeat(rng.choice(np.array([-1.0, 1.0], F32), (n, 1)), d, axis=1)


def found_per_query(idx, d):
    return (np.asarray(idx).reshape(-1, d + 1) >= 0).sum(axis=1)


def assert_query_kinds(idx, kind, d, what=""):
    """Each kind is there, the cloud's own points find their whole simplex, some shell query finds part of its simplex, no far query
    finds anything.  Returns the counts (cloud, shell, far, shell queries with a partly absent simplex)."""
    found = found_per_query(idx, d)
    counts = [int((kind == k).sum()) for k in range(3)]
    partial = int(((found > 0) & (found < d + 1) & (kind == 1)).sum())
    if len(kind) >= 3:
        assert min(counts) >= 1, (what, counts)
    assert np.all(found[kind == 0] == d + 1), (what, "a point of the build cloud misses a vertex of its own simplex")
    assert np.all(found[kind == 2] == 0), (what, "a far query found a vertex")
    if counts[1] >= 20:
        assert partial >= 1, (what, "no shell query with a partly absent simplex")
    return counts + [partial]


def oracle_lookup(t, values, q, sigma):
    """O.slice_no_precomputation of raw query points (also of none) -> (sliced, idx, w)"""
    d = t.pos_dim
    if len(q) == 0:
        return np.zeros((0, values.shape[1]), F32), np.zeros((0,), np.int32), np.zeros((0,), F32)
    return O.slice_no_precomputation(t, values, O.scale_positions(q, sigmas(d, sigma)))


def slice_fp64(values, idx, w, n):
    """(sum_r value_r w_r, sum_r |value_r w_r|) over the found vertices in fp64 -> [n, v] each"""
    v = values.shape[1]
    dp1 = (len(idx) // n) if n else 1
    idx2, w2 = np.asarray(idx).reshape(n, dp1), np.asarray(w, np.float64).reshape(n, dp1)
    out, mag = np.zeros((n, v)), np.zeros((n, v))
    vals = np.asarray(values, np.float64)
    for r in range(dp1):
        ok = idx2[:, r] >= 0
        term = vals[idx2[ok, r]] * w2[ok, r][:, None]
        out[ok] += term
        mag[ok] += np.abs(term)
    return out, mag


def slice_bound(mag, d):
    """fp32 evaluation of a (d + 1)-term sum of products, any order: gamma_(d+1) sum |terms|"""
    u = (d + 1) * 2.0 ** -24
    return u / (1.0 - u) * mag


def scatter_fp64(grad, idx, w, m):
    """Gradient of the slice towards the lattice values in fp64, absent vertices with weight 0: (sum, sum of |terms|, tokens per row)"""
    n, v = grad.shape
    dp1 = (len(idx) // n) if n else 1
    idx2, w2 = np.asarray(idx).reshape(n, dp1), np.asarray(w, np.float64).reshape(n, dp1)
    out, mag, count = np.zeros((m, v)), np.zeros((m, v)), np.zeros((m,), np.int64)
    g = np.asarray(grad, np.float64)
    for r in range(dp1):
        ok = idx2[:, r] >= 0
        term = g[ok] * w2[ok, r][:, None]
        np.add.at(out, idx2[ok, r], term)
        np.add.at(mag, idx2[ok, r], np.abs(term))
        np.add.at(count, idx2[ok, r], 1)
    return out, mag, count


@functools.lru_cache(maxsize=None)
def lookup_oracle(d):
    """(positions, sigma, oracle table, idx, w) of the table the lookups of dimension d run against: the main cloud"""
    pos, sigma = main_cloud(d)
    t, idx, w, _ = main_oracle(d)
    return pos, sigma, t, idx, w


def rehash_queries(d):
    _, second, sigma = rehash_clouds(d)[:3]
    return queries(second, sigma, 257, 50 + d, 3 * MAIN[d][1])


def wide_queries(d, reach):
    return queries(wide_cloud(d, reach)[0], 1.0, 256, 70 + d)


def loaded_queries(d):
    pos, sigma = main_cloud(d)
    return queries(pos, sigma, 1500, 90 + d, MAIN[d][1])


REHASH_DIMS = (1, 2, 4, 6)
REHASH_CAP = 100000


@functools.lru_cache(maxsize=None)
def rehash_clouds(d):
    """A first cloud of 400 points (its build hashes into 16384 of the 100000 slots) and a second one of 3000 points over a
    box three times as wide, inserted without a reset: (first, second, sigma, oracle table after both, (idx, w) of each build,
    vertex count after the first)"""
    pos, sigma = main_cloud(d)
    extent = MAIN[d][1]
    rng = np.random.default_rng(900 + d)
    first = pos[:400].copy()
    second = rng.uniform(-3 * extent, 3 * extent, (3000, d)).astype(F32)
    t, i1, w1 = oracle_build(first, sigma, REHASH_CAP)
    m1 = t.nr_filled
    _, i2, w2 = oracle_build(second, sigma, table=t)
    return first, second, sigma, t, (i1, w1), (i2, w2), m1


LOADED_DIMS = (2, 3, 5)
PROBE_MARGIN = 150  # half the 300-probe retrieval limit


@functools.lru_cache(maxsize=None)
def loaded_table(d):
    """The main cloud in a table at load 0.8: (capacity, oracle table, idx, w).  The reference's hash spreads lattice keys well for some
    moduli and poorly for others, so the capacity is the first one from vertices / 0.8 upwards at which the oracle's longest run of
    occupied slots stays below half the 300-probe retrieval limit."""
    pos, sigma = main_cloud(d)
    base = int(main_oracle(d)[0].nr_filled / 0.8) + 1
    for cap in range(base, base + 40):
        t, idx, w = oracle_build(pos, sigma, cap)
        if longest_probe_run(t) < PROBE_MARGIN:
            return cap, t, idx, w
    raise AssertionError((d, "no capacity near load 0.8 keeps the probe chains short"))


def longest_probe_run(t):
    """Longest run of occupied slots of an oracle table (circular): what the longest probe chain of a lookup can be"""
    occ = t.entries >= 0
    if occ.all():
        return len(occ)
    start = int(np.argmin(occ))  # an empty slot: unroll the circle there
    run = best = 0
    for x in np.roll(occ, -start).tolist():
        run = run + 1 if x else 0
        best = max(best, run)
    return best


EXPAND_CASES = [(d, mult, ev) for d in (2, 5) for mult in (1, 3) for ev in (True, False)]
EXPAND_CAP = 60000
EXPAND_NOISE = 0.2


@functools.lru_cache(maxsize=None)
def expand_cloud(d):
    pos, sigma = main_cloud(d)
    return pos[:500].copy(), sigma
