"""Looking positions up in an existing table (ln_slice_no_precomputation: k_retrieve_points<D, false>, then ln_slice_forward; reached
through Lattice.slice_standalone_no_precomputation and SliceLattice.apply without indices), the re-hash of a table that grows
(ln_rehash: k_rehash_rows<D>) and Lattice.expand, at every position dimension 1 .. 6 against the oracle (`pytest -m gpu`).

Every call mixes three kinds of query: points of the build cloud (whole simplex present), points pushed through a face of the cloud's
box (part of the simplex absent), points far away (nothing present).  Indices and weights are compared bit for bit (-1 / -1.0 for an
absent vertex), the sliced rows bit for bit with the oracle's ordered fp32 evaluation AND element by element within
(d + 1) 2^-24 / (1 - (d + 1) 2^-24) * sum_r |value_r w_r| of an fp64 evaluation; rows of far queries are +0.0 exactly.  The gradient
towards the lattice values is held to the segment-reduce bound of tests/test_gpu_segment_reduce.py against an fp64 scatter in which
absent vertices weigh 0: an absent vertex that contributed anywhere would show.  The clouds and their conditions live in
tests/table_reference.py (checked without a GPU by tests/test_table_reference.py).

Worst |slice - fp64| / bound per case, measured on an MI355X (`pytest -s` prints them with the number of queries of each kind;
asserted <= 1):
  d = 1: 0.741 (V = 1, n = 1500), 0 (V = 65, n = 0)       d = 2: 0.645 (V = 3, n = 1500), 0.677 (V = 64, n = 1: three calls)
  d = 3: 0.688 (V = 64, n = 1500), 0.425 (V = 3, n = 256)   d = 4: 0.604 (V = 65, n = 1500), 0.290 (V = 1, n = 257)
  d = 5: 0.387 (V = 1, n = 1500), 0.423 (V = 64, n = 257)   d = 6: 0.327 (V = 3, n = 1500), 0.403 (V = 65, n = 256)
"""
import numpy as np
import pytest
import torch

from tests import table_reference as R
from tests.test_gpu_segment_reduce import assert_reduce_close

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def N(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def new_lattice(d, sigma, cap):
    from lattice_net_amd import Lattice
    return Lattice(sigmas=[float(sigma)] * d, capacity=int(cap), device=dev())


def build(pos, sigma, cap):
    lat = new_lattice(pos.shape[1], sigma, cap)
    lat.begin_splat()
    idx, w = lat.just_create_verts(T(pos), True)
    m = lat.nr_lattice_vertices()
    assert int(N(lat.m_hash_table._counters)[1]) == 0, "the build reported a status bit"
    return lat, idx, w, m


_TABLES = {}


def main_table(d):
    """(lattice, oracle table) of the main cloud of dimension d, built once per module"""
    if d not in _TABLES:
        pos, sigma, t, oidx, ow = R.lookup_oracle(d)
        lat, idx, w, m = build(pos, sigma, R.CAP)
        assert m == t.nr_filled and np.array_equal(N(idx), oidx) and np.array_equal(N(w), ow)
        assert np.array_equal(N(lat.m_hash_table.m_keys_tensor)[:m], R.keys_of(t))
        _TABLES[d] = (lat, t)
    return _TABLES[d]


def assert_lookup(lat, t, sigma, q, kind, v, seed, what, gradient=True):
    """One call with the queries q against the oracle; returns (worst error / bound against fp64, counts per kind)"""
    from lattice_net_amd import SliceLattice
    d, m, n = t.pos_dim, t.nr_filled, len(q)
    rng = np.random.default_rng(seed)
    vals_np = rng.standard_normal((m, v)).astype(np.float32)
    lat.set_values(T(vals_np))
    out, idx, w = lat.slice_standalone_no_precomputation(T(q))
    out, idx, w = N(out), N(idx), N(w)
    o_out, o_idx, o_w = R.oracle_lookup(t, vals_np, q, sigma)
    assert out.shape == (n, v) and idx.shape == (n * (d + 1),) and w.shape == (n * (d + 1),)
    assert np.array_equal(idx, o_idx), (what, "indices", int((idx != o_idx).sum()))
    assert np.array_equal(bits(w), bits(o_w)), (what, "weights", int((bits(w) != bits(o_w)).sum()))
    assert np.all(w[idx < 0] == -1.0) and np.all(w[idx >= 0] != -1.0)
    counts = R.assert_query_kinds(idx, kind, d, what)
    assert np.array_equal(bits(out), bits(o_out)), (what, "sliced rows against the ordered fp32 evaluation", int((bits(out) != bits(o_out)).sum()))
    ref, mag = R.slice_fp64(vals_np, idx, w, n)
    bound = R.slice_bound(mag, d)
    err = np.abs(out.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.max(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)))) if err.size else 0.0
    assert np.all(err <= bound), (what, "sliced rows against fp64", ratio)
    assert np.all(bits(out[kind == 2]) == 0), (what, "rows of far queries must be +0.0 exactly")
    if gradient:
        g_np = rng.standard_normal((n, v)).astype(np.float32)
        vals = T(vals_np).requires_grad_(True)
        out2 = SliceLattice.apply(vals, lat, T(q))
        assert np.array_equal(bits(N(out2)), bits(o_out)), (what, "SliceLattice.apply without indices")
        out2.backward(T(g_np))
        gref, gmag, count = R.scatter_fp64(g_np, idx, w, m)
        assert tuple(vals.grad.shape) == (m, v)
        assert_reduce_close(vals.grad, gref, gmag, count, what=f"{what} lattice-value gradient")
        untouched = count == 0
        assert np.all(bits(N(vals.grad)[untouched]) == 0), (what, "a row without a found vertex received a gradient")
    return ratio, counts


@pytest.mark.parametrize("d,v,n", R.LOOKUP_CASES)
def test_lookups_against_the_oracle(d, v, n):
    lat, t = main_table(d)
    sigma = R.MAIN[d][2]
    worst, total = 0.0, np.zeros(4, np.int64)
    for k, (q, kind) in enumerate(R.lookup_calls(d, n)):
        ratio, counts = assert_lookup(lat, t, sigma, q, kind, v, 100 * d + k, f"d={d} V={v} n={n} call {k}")
        worst, total = max(worst, ratio), total + counts
    print(f"d={d} V={v} n={n}: worst |slice - fp64| / bound {worst:.3f}; queries cloud {total[0]} shell {total[1]} (partly absent {total[3]}) far {total[2]}")
    assert worst <= 1.0


@pytest.mark.parametrize("d", R.REHASH_DIMS)
def test_every_vertex_is_found_after_a_rehash(d):
    """A first cloud hashed into 16384 of the table's slots, then begin_splat(reset_hashmap=False) and a larger cloud: the table is
    re-hashed into all its slots (ln_rehash) before the second build.  Looking up the first cloud's own positions afterwards returns
    exactly the indices and weights its build returned, and so does looking up the second cloud's: every vertex kept its row and is
    found by its key."""
    first, second, sigma, t, (oi1, ow1), (oi2, ow2), m1 = R.rehash_clouds(d)
    lat = new_lattice(d, sigma, R.REHASH_CAP)
    lat.begin_splat()
    i1, w1 = lat.just_create_verts(T(first), True)
    assert lat.nr_lattice_vertices() == m1
    st = lat.m_hash_table._storage
    assert st.hashed() == 16384 < R.REHASH_CAP
    lat.begin_splat(reset_hashmap=False)
    i2, w2 = lat.just_create_verts(T(second), True)
    m2 = lat.nr_lattice_vertices()
    assert st.hashed() == R.REHASH_CAP, "the incremental build must have re-hashed the table into all its slots"
    assert m2 == t.nr_filled and int(N(lat.m_hash_table._counters)[1]) == 0
    for got, want in ((i1, oi1), (w1, ow1), (i2, oi2), (w2, ow2)):
        assert np.array_equal(N(got), want)
    assert np.array_equal(N(lat.m_hash_table.m_keys_tensor)[:m2], R.keys_of(t))
    vals_np = np.random.default_rng(d).standard_normal((m2, 3)).astype(np.float32)
    lat.set_values(T(vals_np))
    for name, pts, bi, bw in (("first", first, i1, w1), ("second", second, i2, w2)):
        out, qi, qw = lat.slice_standalone_no_precomputation(T(pts))
        assert torch.equal(qi, bi), (d, name, "indices of the build", int((qi != bi).sum()))
        assert torch.equal(qw, bw), (d, name, "weights of the build")
        assert int(qi.min()) >= 0
        o_out, _, _ = R.oracle_lookup(t, vals_np, pts, sigma)
        assert np.array_equal(bits(N(out)), bits(o_out)), (d, name)
    # and the mixed queries of the lookup cases, against the grown table
    q, kind = R.rehash_queries(d)
    assert_lookup(lat, t, sigma, q, kind, 3, 60 + d, f"after the re-hash, d={d}", gradient=False)


@pytest.mark.parametrize("d,reach", [c for c in R.WIDE if R.WIDE[c]])
def test_lookups_in_a_wide_table_in_the_lattice_key_format(d, reach):
    pos, t, oidx, ow = R.wide_cloud(d, reach)
    lat, idx, w, m = build(pos, 1.0, R.WIDE_CAP)
    assert m == t.nr_filled and lat.m_hash_table._storage.key_format == 1 and not R.fits_raw_format(R.keys_of(t))
    assert np.array_equal(N(idx), oidx) and np.array_equal(N(w), ow)
    vals_np = np.random.default_rng(d).standard_normal((m, 3)).astype(np.float32)
    lat.set_values(T(vals_np))
    out, qi, qw = lat.slice_standalone_no_precomputation(T(pos))
    assert torch.equal(qi, idx) and torch.equal(qw, w) and int(qi.min()) >= 0
    o_out, o_idx, o_w = R.oracle_lookup(t, vals_np, pos, 1.0)
    assert np.array_equal(N(qi), o_idx) and np.array_equal(bits(N(qw)), bits(o_w)) and np.array_equal(bits(N(out)), bits(o_out))
    # the three kinds around this cloud too: far queries leave the packable range of the lattice format altogether at d = 6
    q, kind = R.wide_queries(d, reach)
    assert_lookup(lat, t, 1.0, q, kind, 3, 80 + d, f"wide d={d} reach {reach}", gradient=False)


@pytest.mark.parametrize("d", R.LOADED_DIMS)
def test_lookups_in_a_table_at_load_0_8(d):
    """Capacity from the oracle's vertex count (tests/table_reference.py: loaded_table), the oracle's probe chains below half the
    300-probe retrieval limit"""
    pos, sigma = R.main_cloud(d)
    cap, t, oidx, ow = R.loaded_table(d)
    assert R.longest_probe_run(t) < R.PROBE_MARGIN
    lat, idx, w, m = build(pos, sigma, cap)
    assert m == t.nr_filled and lat.m_hash_table._storage.hashed() == cap and 0.78 <= m / cap <= 0.8
    assert np.array_equal(N(idx), oidx) and np.array_equal(N(w), ow)
    q, kind = R.loaded_queries(d)
    assert_lookup(lat, t, sigma, q, kind, 3, 95 + d, f"load 0.8, d={d}")


@pytest.mark.parametrize("d,multiplier,expand_values", R.EXPAND_CASES)
def test_expand_at_other_dimensions(d, multiplier, expand_values):
    """Lattice.expand: the positions repeated `multiplier` times plus Gaussian jitter, inserted into a copy of the table.  The jitter is
    reproducible under torch.manual_seed, so the expanded table is the oracle's incremental build on exactly those positions."""
    pos_np, sigma = R.expand_cloud(d)
    pos = T(pos_np)
    n, v = len(pos_np), 3
    lat = new_lattice(d, sigma, R.EXPAND_CAP)
    lat.begin_splat()
    lat.splat_standalone(pos, T(np.random.default_rng(d).standard_normal((n, v)).astype(np.float32)))
    m = lat.nr_lattice_vertices()
    lat.set_values(lat.values()[:m].contiguous())
    keys_before, values_before = N(lat.m_hash_table.m_keys_tensor).copy(), N(lat.values()).copy()
    torch.manual_seed(d)
    ex = lat.expand(pos, multiplier, R.EXPAND_NOISE, expand_values)
    m2 = ex.nr_lattice_vertices()
    # the same jitter again (repeat, then + randn * stddev), then the oracle's serial insertion order
    torch.manual_seed(d)
    rep = pos.repeat(multiplier, 1)
    jittered = N(rep + torch.randn_like(rep) * R.EXPAND_NOISE)
    t, _, _ = R.oracle_build(pos_np, sigma, R.EXPAND_CAP)
    assert t.nr_filled == m and np.array_equal(R.keys_of(t), keys_before[:m])
    R.oracle_build(jittered, sigma, table=t)
    assert m2 == t.nr_filled and m2 > m, "the jitter must add vertices"
    ek = N(ex.m_hash_table.m_keys_tensor)
    assert np.array_equal(ek[:m2], R.keys_of(t)), "keys in order: old rows keep their ids, new ones follow in insertion order"
    assert not ek[m2:].any()
    if expand_values:
        assert tuple(ex.values().shape) == (m2, v)
        assert np.array_equal(bits(N(ex.values())[:m]), bits(values_before)), "old rows keep their values"
        assert np.all(bits(N(ex.values())[m:]) == 0), "new rows are zero"
    else:
        assert ex.values().shape[1] == v and not bool(ex.values().any())
    # the source lattice is untouched
    assert lat.nr_lattice_vertices() == m and lat.m_hash_table._storage is not ex.m_hash_table._storage
    assert np.array_equal(N(lat.m_hash_table.m_keys_tensor), keys_before)
    assert np.array_equal(bits(N(lat.values())), bits(values_before))
    # the expanded table answers lookups of old and new positions like the oracle's
    ex.set_values(torch.zeros((m2, v), device=dev()))
    for pts in (pos_np, jittered[:300]):
        _, qi, qw = ex.slice_standalone_no_precomputation(T(pts))
        _, oi, ow = R.oracle_lookup(t, np.zeros((m2, v), np.float32), pts, sigma)
        assert np.array_equal(N(qi), oi) and np.array_equal(bits(N(qw)), bits(ow)) and oi.min() >= 0
