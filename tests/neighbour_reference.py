"""Exact reference of the neighbour traversal (csrc/ln_neighbours.h: ln_neighbours_body) and the clouds its tests run on.  Plain NumPy and
a Python dict on the CPU: test_neighbour_reference.py checks this module without a GPU (against oracle.lattice_oracle.neighbour_rows,
which imitates the float arithmetic of the traversal step by step, and against seeded wrong traversals), test_gpu_neighbour_forms.py
holds every form of the kernel to it, entry for entry.

The function.  A table is a dict {key tuple (first d coordinates) -> row}.  A query vertex with the key k (d + 1 integer coordinates, the
last one minus the sum of the others) is scaled by s = 2^(query level - neighbour level), s in {1/2, 1, 2}; its neighbours along axis a are
    np_a = s k + t (1, .., 1, -d, 1, .., 1)        nm_a = s k - t (1, .., 1, -d, 1, .., 1)        (-d at coordinate a)
with the step t = min(s, 1) * dilation.  List slots: np_a -> 2 a + flip, nm_a -> 2 a + 1 - flip, the vertex s k itself -> E - 1, E = 2 (d + 1) + 1.
Entries: row >= 0, ABSENT (-1) looked up and not there, NOT_VISITED (-2) never looked up.  At s >= 1 everything is looked up.  At s = 1/2:
    the centre is looked up only when all d + 1 coordinates of s k are integers;
    the neighbours are looked up only when they are not all integers;
    for odd d + 1 a neighbour is looked up only when its own d + 1 coordinates are all integers.
What is looked up with a coordinate that is no integer (even d + 1 at s = 1/2: all coordinates of s k are then half-integers, and an even
dilation leaves them so) is rounded half away from zero, as roundf does.  Everything is computed on DOUBLED coordinates 2 s k and 2 t, which
are integers at every s: "is an integer" is "is even", nothing is ever rounded but that one half, and no float occurs.  A key the
table's packed format cannot hold is in no table, i.e. in no dict: absent.

The float forms of the kernel and the oracle are exact while every coordinate of every vertex and neighbour stays below 2^24 in magnitude
(`largest_coordinate` gives the figure to assert on); beyond that this module is still exact and they are not."""
import functools

import numpy as np

from oracle import lattice_oracle as O

ABSENT, NOT_VISITED = -1, -2
WRONG = ("swap_np_nm_on_one_axis", "step_d_plus_1", "no_odd_rule", "no_centre_rule", "one_row_shifted")
INT_FORM_COORD = 1 << 22     # the integer form of the kernel is taken below this coordinate magnitude ...
INT_FORM_DILATION = 1 << 18  # ... and below this dilation
FLOAT_EXACT = 1 << 24


def extent(d):
    return 2 * (d + 1) + 1


def rows_per_workgroup(d):
    """vertices per workgroup of k_neighbours / of the traversal part of the fused launch"""
    return 256 // extent(d)


def swap_axis(d):
    """the axis of the seeded np / nm swap (and the one the far clusters lie along)"""
    return (d + 1) // 2


def table_dict(keys):
    """{key tuple: row} of the first len(keys) rows of a table's keys [M, d]"""
    return {t: r for r, t in enumerate(map(tuple, np.asarray(keys, np.int64).tolist()))}


def full_keys(keys):
    """[M, d + 1] int64: the keys with the (d + 1)-th coordinate"""
    k = np.asarray(keys, np.int64)
    return np.concatenate([k, -k.sum(axis=1, keepdims=True)], axis=1)


def _doubled(lvl_diff, dilation):
    """(factor from k to the doubled scaled coordinate, doubled step)"""
    assert lvl_diff in (-1, 0, 1) and dilation >= 1
    return {-1: 1, 0: 2, 1: 4}[lvl_diff], int(dilation) * (1 if lvl_diff < 0 else 2)


def _halve_rounding_half_away(k2):
    """doubled coordinate -> the integer roundf gives for its half"""
    odd = k2 % 2  # 0 / 1, for negative numbers too
    return (k2 + np.sign(k2) * odd) // 2


def _lookup(table, k2, d):
    keys = _halve_rounding_half_away(k2)[:, :d]
    return np.fromiter((table.get(t, ABSENT) for t in map(tuple, keys.tolist())), np.int64, count=len(keys))


def neighbour_list(query_keys, table, lvl_diff, dilation, flip, wrong=None):
    """[M, E] int32 list of the query vertices `query_keys` [M, d] in `table` (a dict), lvl_diff = query level - neighbour level.
    `wrong` (one of WRONG): the same with one seeded mistake, for the tests that show the reference would notice it."""
    assert wrong is None or wrong in WRONG
    flip = 1 if flip else 0
    k = full_keys(query_keys)
    m, dp1 = k.shape
    d, E = dp1 - 1, 2 * dp1 + 1
    factor, step2 = _doubled(lvl_diff, dilation)
    k2 = k * factor
    half = lvl_diff < 0
    all_int = np.all(k2 % 2 == 0, axis=1)
    out = np.full((m, E), NOT_VISITED, np.int64)
    visit_centre = all_int if (half and wrong != "no_centre_rule") else np.ones(m, bool)
    visit_nbrs = ~all_int if half else np.ones(m, bool)
    out[visit_centre, E - 1] = _lookup(table, k2[visit_centre], d)
    big = step2 * ((d + 1) if wrong == "step_d_plus_1" else d)
    for a in range(dp1):
        swap = 1 if (wrong == "swap_np_nm_on_one_axis" and a == swap_axis(d)) else 0
        for sign, slot in ((1, 2 * a + (flip ^ swap)), (-1, 2 * a + 1 - (flip ^ swap))):
            n2 = k2 + sign * step2
            n2[:, a] = k2[:, a] - sign * big
            visit = visit_nbrs
            if half and dp1 % 2 == 1 and wrong != "no_odd_rule":
                visit = visit & np.all(n2 % 2 == 0, axis=1)
            out[visit, slot] = _lookup(table, n2[visit], d)
    if wrong == "one_row_shifted":
        rows = np.nonzero(np.any(out >= 0, axis=1))[0]
        r = rows[len(rows) // 2]
        out[r] = np.roll(out[r], 1)
    return out.astype(np.int32)


def largest_coordinate(query_keys, lvl_diff, dilation):
    """Largest magnitude among the d + 1 scaled coordinates of every query vertex and of every neighbour the traversal forms (whether it
    looks it up or not), as a float: the float form is exact while this stays below 2^24."""
    k = full_keys(query_keys)
    d = k.shape[1] - 1
    factor, step2 = _doubled(lvl_diff, dilation)
    reach = np.abs(k * factor).max() + step2 * d  # |s k_a -+ t d| <= |s k_a| + t d, and t <= t d
    return float(reach) / 2.0


def shares(nbr):
    """Fractions the vacuity conditions are about: hits / absent / never visited among the non-centre entries, never visited on the centre"""
    nbr = np.asarray(nbr)
    side, centre = nbr[:, :-1], nbr[:, -1]
    return {"hits": float(np.mean(side >= 0)), "absent": float(np.mean(side == ABSENT)), "unvisited": float(np.mean(side == NOT_VISITED)),
            "centre_unvisited": float(np.mean(centre == NOT_VISITED)), "hit_count": int(np.sum(side >= 0))}


def assert_same_level_not_vacuous(nbr, what=""):
    s = shares(nbr)
    assert s["hits"] >= 0.05 and s["absent"] >= 0.05, (what, s)


# ------------------------------------------------------------------------------------------------------------------------------------
# clouds.  Every cloud is (positions [n, d] float32, sigma); all of them are a few hundred to 3000 points, 10^3 .. 10^4 vertices.
# ------------------------------------------------------------------------------------------------------------------------------------
CAPACITY = 1 << 16  # slots of every table of these tests


def _elevation(d):
    """[d + 1, d]: the linear map from (sigma-scaled) positions to lattice coordinates"""
    return O.elevate(np.eye(d, dtype=np.float32)).astype(np.float64).T


def axis_direction(d, a):
    """The position step that moves a lattice vertex onto its np neighbour of axis a at dilation 1 (times sigma)"""
    v = np.ones(d + 1)
    v[a] = -d
    return np.linalg.lstsq(_elevation(d), v, rcond=None)[0]


LINE_HALF_LENGTH = 9  # in neighbour steps: longer than the largest small dilation (5)


@functools.lru_cache(maxsize=None)
def lines_cloud(d):
    """A blob at the origin and a line of points through it along every one of the d + 1 neighbour directions, 2 * LINE_HALF_LENGTH steps
    long: a vertex on a line has its neighbours of that axis at every dilation up to 5 (hits), and none along most other axes (absent).
    The points are sparse enough along the lines to leave gaps (at d = 1, where there is nothing but the line, the gaps are the absents)."""
    rng = np.random.default_rng(7100 + d)
    per_line = {1: 14, 2: 60, 3: 90, 4: 90, 5: 80, 6: 70}[d]
    noise = {1: 0.0, 2: 0.5, 3: 0.45, 4: 0.35, 5: 0.3, 6: 0.25}[d]
    parts = [rng.standard_normal((40 * d, d)) * 1.2]
    for a in range(d + 1):
        t = rng.uniform(-LINE_HALF_LENGTH, LINE_HALF_LENGTH, (per_line * (d + 1) // 2, 1))
        parts.append(t * axis_direction(d, a)[None, :] + rng.standard_normal((len(t), d)) * noise)
    if d == 1:  # one direction only: a longer, gappy line
        parts = [rng.uniform(-260, 260, (430, 1))]
    pos = np.concatenate(parts).astype(np.float32)
    return pos[rng.permutation(len(pos))], 1.0


@functools.lru_cache(maxsize=None)
def crossing_cloud(d):
    """lines_cloud plus isolated points far from everything: the coarse level made from the fine vertices (create_coarse_verts) holds the
    coarse neighbours of every fine vertex that has fine neighbours, so only isolated simplices give the fine -> coarse list absents."""
    pos, sigma = lines_cloud(d)
    rng = np.random.default_rng(7400 + d)
    extra = rng.uniform(300, 6300, (300, 1)) if d == 1 else rng.uniform(-40, 40, (300, d))
    return np.concatenate([pos, extra.astype(np.float32)]), sigma


def fine_to_coarse_conditions(d, dilation):
    """Which of the four 1 % conditions of a fine -> coarse list (hits, absent, never-visited neighbour slots, never-visited centres) CAN
    hold, with the reason for each that cannot; the test asserts what replaces it.
      odd d + 1, even dilation: a neighbour is s k +- dilation / 2 * (1, .., -d, ..), an integer vector away from s k, so it is all-integer
        exactly when s k is, and then the neighbours are not looked up: NO neighbour slot is ever visited.  Asserted: every one reads -2.
      d = 1, dilation 1: every vertex of a table built from points comes with the other vertex of its segment; the odd one of the two looks
        up the halves of its two even neighbours, and the coarsening inserts both (the half of the even partner, and, because the odd
        vertex is that partner's fine neighbour, the coarse vertex on its other side): nothing is absent.  Asserted: no -1.
      d = 6: a neighbour slot is looked up for one of the 2^6 parity patterns of the vertex only, 1 / 64 = 1.6 % of the entries, so hits and
        absents cannot both reach 1 %.  Asserted: 1 % hits and at least 100 absent entries."""
    odd_even = (d + 1) % 2 == 1 and dilation % 2 == 0
    return {"looked_up": not odd_even, "absent": not odd_even and not (d == 1 and dilation == 1), "absent_share": d != 6}


def assert_fine_to_coarse_conditions(nbr, d, dilation, what=""):
    s, can = shares(nbr), fine_to_coarse_conditions(d, dilation)
    assert s["unvisited"] >= 0.01 and s["centre_unvisited"] >= 0.01 and float(np.mean(nbr[:, -1] >= 0)) >= 0.01, (what, s)
    if not can["looked_up"]:
        assert s["unvisited"] == 1.0, (what, s)
        return
    assert s["hits"] >= 0.01, (what, s)
    if not can["absent"]:
        assert s["absent"] == 0.0, (what, s)
    elif can["absent_share"]:
        assert s["absent"] >= 0.01, (what, s)
    else:
        assert int(np.sum(nbr[:, :-1] == ABSENT)) >= 100, (what, s)


def _key_per_unit(d):
    """lattice coordinate 0 per unit of position coordinate 0 (sigma 1)"""
    return float(_elevation(d)[0, 0])


@functools.lru_cache(maxsize=None)
def offset_cloud(d, kind):
    """d in (1, 2).  kind "beyond": every vertex has a coordinate beyond +-2^22 (the float form of the same-level traversal everywhere);
    "straddle": the cloud lies across the threshold, both forms in one launch, within one workgroup where the rows of the two sides meet."""
    assert d in (1, 2) and kind in ("beyond", "straddle")
    rng = np.random.default_rng(7200 + 10 * d + (kind == "straddle"))
    x0 = INT_FORM_COORD / _key_per_unit(d)
    if d == 1:
        lo, hi = (x0 + 2000, x0 + 2900) if kind == "beyond" else (x0 - 450, x0 + 450)
        pos = rng.uniform(lo, hi, (700, 1))
    else:
        lo, hi = (x0 + 500, x0 + 545) if kind == "beyond" else (x0 - 22, x0 + 23)
        pos = np.stack([rng.uniform(lo, hi, 1500), rng.uniform(-10, 10, 1500)], axis=1)
    return pos.astype(np.float32), 1.0


@functools.lru_cache(maxsize=None)
def far_clusters_cloud(d):
    """Two copies of one blob 2^18 neighbour steps of axis swap_axis(d) apart, each several steps wide, so that dilation 2^18 and 2^18 + 1 find hits
    from one copy into the other along that axis (and nothing along the others: absent, or beyond what the key format packs)"""
    rng = np.random.default_rng(7300 + d)
    blob = rng.uniform(-120, 120, (400, 1)) if d == 1 else rng.standard_normal((500, d)) * 2.0
    far = INT_FORM_DILATION * axis_direction(d, swap_axis(d))[None, :]
    return np.concatenate([blob, blob + far + rng.standard_normal(blob.shape) * 0.2]).astype(np.float32), 1.0


def cloud(kind, d):
    return {"lines": lines_cloud, "crossing": crossing_cloud, "far": far_clusters_cloud}[kind](d) if kind in ("lines", "crossing", "far") \
        else offset_cloud(d, kind)


def oracle_table(pos, sigma):
    """The oracle's table of a cloud (canonical row numbering)"""
    d = pos.shape[1]
    t = O.OracleHashTable(CAPACITY, d)
    O.build_splat(t, O.scale_positions(pos, np.full((d,), sigma, np.float32)))
    return t


def oracle_coarse_table(fine):
    """The key-based coarse level of an oracle table (what Lattice.create_coarse_verts builds)"""
    c = O.OracleHashTable(CAPACITY, fine.pos_dim)
    O.coarsen_keys(fine, c)
    return c


def beyond_threshold(keys):
    """per vertex: some coordinate at or beyond +-2^22 (the vertex takes the float form of the same-level traversal)"""
    return np.any(np.abs(full_keys(keys)) >= INT_FORM_COORD, axis=1)


# the cases of test_gpu_neighbour_forms.py: (cloud kind, d, direction, dilation); direction "same", "fine_to_coarse" (scale 1/2) or
# "coarse_to_fine" (scale 2), the coarse level made from the fine one by the key-based coarsening
SMALL_DILATIONS = (1, 2, 3, 5)
CROSSING_DILATIONS = (1, 2)
FLOAT_COORD_DILATIONS = (1, 2)
FAR_DILATIONS = (INT_FORM_DILATION, INT_FORM_DILATION + 1)
LVL_DIFF = {"same": 0, "fine_to_coarse": -1, "coarse_to_fine": 1}


def cases():
    out = [("lines", d, "same", dil) for d in range(1, 7) for dil in SMALL_DILATIONS]
    out += [(kind, d, "same", dil) for d in (1, 2) for kind in ("beyond", "straddle") for dil in FLOAT_COORD_DILATIONS]
    out += [("far", d, "same", dil) for d in (1, 3) for dil in FAR_DILATIONS]
    out += [("crossing", d, way, dil) for d in range(1, 7) for way in ("fine_to_coarse", "coarse_to_fine") for dil in CROSSING_DILATIONS]
    return out


@functools.lru_cache(maxsize=None)
def oracle_tables(kind, d):
    """(fine table, coarse table or None) of a cloud, built by the oracle"""
    fine = oracle_table(*cloud(kind, d))
    return fine, (oracle_coarse_table(fine) if kind == "crossing" else None)


def sides(fine_keys, coarse_keys, direction):
    """(query keys, keys of the neighbour table) of a case"""
    return {"same": (fine_keys, fine_keys), "fine_to_coarse": (fine_keys, coarse_keys), "coarse_to_fine": (coarse_keys, fine_keys)}[direction]


def wrong_applies(wrong, d, direction, dilation):
    """Whether a seeded mistake can change the list of a case at all: the two rules exist at scale 1 / 2 only (the odd one for odd d + 1),
    and where no neighbour slot is ever looked up (fine_to_coarse_conditions) nothing about the neighbours can show."""
    half = direction == "fine_to_coarse"
    if wrong == "no_centre_rule":
        return half
    if wrong == "no_odd_rule":
        return half and (d + 1) % 2 == 1
    if wrong in ("swap_np_nm_on_one_axis", "step_d_plus_1"):
        return not half or fine_to_coarse_conditions(d, dilation)["looked_up"]
    return True
