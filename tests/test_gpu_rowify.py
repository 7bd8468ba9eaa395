"""k_im2row<VEC>, k_im2rowindices and k_row2im<VEC> (csrc/ln_rows.hip) through the C ABI over synthetic neighbour lists (`pytest -m gpu`):
lists between two lattices (query rows != gathered rows, ids up to the last gathered row), about 30 % of the entries absent (-1), some never
visited (-2), on the centre slot too.  Filter extents 5, 9, 15 x widths on either side of a multiple of 4 (both VEC instances) x row counts
whose work is no multiple of a 256-thread workgroup.  Outputs are pre-filled (NaN / an integer sentinel) and have sentinels behind them.

im2row and im2rowindices move or recode entries: bitwise / integer equality.  row2im adds at most E terms per element in a fixed order:
against the fp64 sum of the same terms within E * 2^-24 * sum |terms| (at most E - 1 fp32 additions, each within half an ulp, 2^-24
relative, of a partial sum no larger than the sum of the magnitudes), and bitwise on small integers, where every partial sum is exact."""
import numpy as np
import pytest
import torch

from oracle import lattice_oracle as O

pytestmark = pytest.mark.gpu
EXTENTS = (5, 9, 15)
WIDTHS = (1, 3, 4, 5, 8, 33, 64)
ROWS = (1, 257, 1000)
INT_SENTINEL = -7777
TAIL = 67


def dev():
    return torch.device("cuda", 0)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def N(t):
    return t.detach().cpu().numpy()


def two_lattice_list(m, mn, E, rng, lo=0):
    """[m, E] int32: ids in [lo, mn) drawn independently, ~30 % -1, ~8 % -2 (on every slot, the centre included); planted: the ids lo and
    mn - 1, a -2 and a -1 on the centre slot, one row wholly absent (from two rows on)"""
    nbr = rng.integers(lo, mn, (m, E)).astype(np.int32)
    u = rng.random((m, E))
    nbr[u < 0.30] = -1
    nbr[u > 0.92] = -2
    if m > 2:
        nbr[m - 1] = -1
        nbr[1, E - 1] = -2
        nbr[2, E - 1] = -1
        nbr[m - 2, 1] = lo
    nbr[0, 0], nbr[0, E - 1] = mn - 1, lo
    return nbr


def sizes(m):
    """rows of the gathered side: never the query row count"""
    return m + 37


def call(name, *args):
    from lattice_net_amd import _lib
    rc = getattr(_lib.load(), name)(*[_lib.ptr(a) if isinstance(a, torch.Tensor) else a for a in args], _lib.stream_ptr(dev()))
    torch.cuda.synchronize()
    assert rc == 0, (name, rc)


def out_buffer(elems, dtype):
    """pre-filled output with sentinels behind it -> (tensor, check of the tail)"""
    if dtype == torch.float32:
        buf = torch.full((elems + TAIL,), float("nan"), dtype=dtype, device=dev())
        buf[elems:] = 12345.0
        return buf, lambda: bool(torch.all(buf[elems:] == 12345.0))
    buf = torch.full((elems + TAIL,), INT_SENTINEL, dtype=dtype, device=dev())
    return buf, lambda: bool(torch.all(buf[elems:] == INT_SENTINEL))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def gather_rows(nbr, vals):
    """[m, E, V]: rows by id, a zero row for every id < 0"""
    return np.where((nbr >= 0)[:, :, None], vals[np.maximum(nbr, 0)], np.float32(0.0)).astype(np.float32)


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("V", WIDTHS)
@pytest.mark.parametrize("E", EXTENTS)
def test_im2row_is_a_bitwise_gather(E, V, m):
    rng = np.random.default_rng(1000 * E + 10 * V + m)
    mn = sizes(m)
    nbr = two_lattice_list(m, mn, E, rng, lo=1)
    vals = rng.standard_normal((mn, V)).astype(np.float32)
    vals[0] = np.nan  # row 0 is named by no entry: a negative id must give a zero row, not row 0 (or row 0 times zero)
    vals[mn - 1, 0] = -0.0
    out, tail_ok = out_buffer(m * E * V, torch.float32)
    call("ln_im2row", T(nbr), T(vals), m, E, V, out)
    got = N(out)[: m * E * V].reshape(m, E, V)
    assert np.array_equal(bits(got), bits(gather_rows(nbr, vals)))
    assert tail_ok()


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("V", WIDTHS)
@pytest.mark.parametrize("E", EXTENTS)
def test_im2rowindices_fill_rules(E, V, m):
    """-2 -> 0; a negative centre -> 0; -1 kept on neighbour slots; every entry V times"""
    rng = np.random.default_rng(2000 * E + 10 * V + m)
    nbr = two_lattice_list(m, sizes(m), E, rng)
    ref = nbr.copy()
    ref[ref == -2] = 0
    ref[ref[:, E - 1] < 0, E - 1] = 0
    ref = np.repeat(ref, V, axis=1)
    assert np.array_equal(ref, O.im2rowindices(nbr, V))
    assert m < 3 or ((ref[:, : (E - 1) * V] == -1).any() and (nbr[:, E - 1] == -1).any() and (nbr[:, E - 1] == -2).any() and not (ref[:, (E - 1) * V:] < 0).any())
    out, tail_ok = out_buffer(m * E * V, torch.int32)
    call("ln_im2rowindices", T(nbr), m, E, V, out)
    assert np.array_equal(N(out)[: m * E * V].reshape(m, E * V), ref)
    assert tail_ok()


def row2im_terms(nbr, rows):
    """[m, E, V] fp64: the terms of every output row in the kernel's order (np_a reads slot 2a + 1, nm_a slot 2a, then the centre), zero
    where the entry is negative"""
    m, E = nbr.shape
    rows = rows.reshape(rows.shape[0], E, -1).astype(np.float64)
    slot = [e ^ 1 for e in range(E - 1)] + [E - 1]
    terms = np.zeros((m, E, rows.shape[2]))
    for e in range(E):
        ok = nbr[:, e] >= 0
        terms[ok, e] = rows[nbr[ok, e], slot[e]]
    return terms


@pytest.mark.parametrize("family", ["random", "small_integers"])
@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("V", WIDTHS)
@pytest.mark.parametrize("E", EXTENTS)
def test_row2im(E, V, m, family):
    rng = np.random.default_rng(3000 * E + 10 * V + m)
    mr = sizes(m)
    nbr = two_lattice_list(m, mr, E, rng, lo=1)
    if family == "random":
        rows = (rng.standard_normal((mr, E * V)) * np.exp(rng.uniform(-6, 6, (mr, 1)))).astype(np.float32)
    else:
        rows = rng.integers(-1000, 1001, (mr, E * V)).astype(np.float32)
    terms = row2im_terms(nbr, rows)  # (before row 0 is poisoned: no entry names it)
    assert not (nbr == 0).any()
    rows[0] = np.where(rng.random(E * V) < 0.5, np.inf, np.nan)  # an absent entry contributes no term, not 0 * x
    ref, mag = terms.sum(axis=1), np.abs(terms).sum(axis=1)
    out, tail_ok = out_buffer(m * V, torch.float32)
    call("ln_row2im", T(nbr), T(rows), m, E, V, out)
    got = N(out)[: m * V].reshape(m, V)
    assert np.all(np.isfinite(got))
    if family == "small_integers":
        assert float(mag.max()) < 2 ** 24
        assert np.array_equal(bits(got), bits(ref.astype(np.float32)))
    else:
        err = np.abs(got.astype(np.float64) - ref)
        assert np.all(err <= E * 2.0 ** -24 * mag), float(np.max(err / np.maximum(E * 2.0 ** -24 * mag, 1e-300)))
        assert np.array_equal(bits(got), bits(O.row2im(nbr, rows_without_poison(rows), V)))
    assert tail_ok()


def rows_without_poison(rows):
    r = rows.copy()
    r[0] = 0.0
    return r


@pytest.mark.parametrize("name,dil,v", [("F1_config1", 1, 4), ("F4_dilation2", 2, 2), ("F9_lidar", 1, 1)])
def test_the_goldens_through_the_c_abi(golden, name, dil, v):
    """The three kernels on the oracle's list of a golden cloud, against the golden's recorded rows"""
    g = golden(name)
    d = g["pos_raw"].shape[1]
    t = O.OracleHashTable(int(g["capacity"]), d)
    O.build_splat(t, O.scale_positions(g["pos_raw"], np.full((d,), float(g["sigma"]), np.float32)))
    m, E = t.nr_filled, 2 * (d + 1) + 1
    nbr = O.neighbour_rows(t.keys[:m], t, 1, 1, dil, False)
    suffix = f"_d{dil}"
    out, tail_ok = out_buffer(m * E * v, torch.int32)
    call("ln_im2rowindices", T(nbr), m, E, v, out)
    assert np.array_equal(N(out)[: m * E * v].reshape(m, E * v), g["im2rowindices" + suffix]) and tail_ok()
    if "im2row" + suffix in g:
        out, tail_ok = out_buffer(m * E * v, torch.float32)
        call("ln_im2row", T(nbr), T(g["values"]), m, E, v, out)
        assert np.array_equal(bits(N(out)[: m * E * v].reshape(m, E * v)), bits(g["im2row" + suffix])) and tail_ok()
    if "row2im" + suffix in g:
        out, tail_ok = out_buffer(m * v, torch.float32)
        call("ln_row2im", T(nbr), T(g["grad_rowified"]), m, E, v, out)
        assert np.array_equal(bits(N(out)[: m * v].reshape(m, v)), bits(g["row2im" + suffix])) and tail_ok()
