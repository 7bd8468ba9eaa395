"""The per-cloud "invalid vertex" rule of a batch of clouds, without a GPU: the NumPy restatement the GPU tests hold
ln_distribute_centre_clouds / ln_pointnet_reduce_forward_clouds to (tests/cloud_invalid_vertex_reference.py) against its own
definitions — one cloud is the row-0 rule, a batch is its clouds done alone with rebased indices — the host switch
Lattice.set_cloud_batch(per_cloud_invalid_vertex=True) (no device work), and the argument checks of the two entry points (reported by
the host half of the library)."""
import numpy as np
import pytest

from tests import cloud_invalid_vertex_reference as V


def test_cloud_of_token():
    assert list(V.cloud_of_token(np.arange(10), 4, 3)) == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2]
    assert list(V.cloud_of_token(np.arange(10), 4, 2)) == [0, 0, 0, 0, 1, 1, 1, 1, 1, 1]  # the last cloud takes what is left
    assert list(V.cloud_of_token([0, 7, 8, 800], 8, 64)) == [0, 0, 1, 63]
    assert list(V.cloud_of_token(np.arange(5), 1000, 1)) == [0] * 5


def test_invalid_rows():
    assert list(np.flatnonzero(V.invalid_rows([0, 3, 4, 8], 8))) == [0, 3, 4]
    # empty clouds have none: cloud 0 ([0, 0)) and clouds 2, 3 ([5, 5)) are empty; row 0 is cloud 1's first vertex
    assert list(np.flatnonzero(V.invalid_rows([0, 0, 5, 5, 5, 9], 9))) == [0, 5]
    # row_starts[B] below the row count: row 6 is no cloud's vertex
    assert list(np.flatnonzero(V.invalid_rows([0, 2, 6], 10))) == [0, 2]
    assert list(np.flatnonzero(V.invalid_rows([0, 1, 2, 3], 3))) == [0, 1, 2]  # one-row clouds: their only row
    assert not V.invalid_rows([0, 0, 0], 4).any()


def test_one_cloud_is_the_row_zero_rule():
    b = V.make_batch([40], 300)
    a = V.distribute_centre(b["d"], b["idx"], b["sums"], b["counts"], 3, 300, [0, 40])
    e = V.distribute_centre(b["d"], b["idx"], b["sums"], b["counts"], 3)
    assert np.array_equal(a, e) and not a[b["idx"] <= 0].any() and a[b["idx"] > 0].all()
    got = V.pointnet_reduce(b["src"], b["idx"], b["d"][:, -1], 40, 4, [0, 40])
    exp = V.pointnet_reduce(b["src"], b["idx"], b["d"][:, -1], 40, 4)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    assert got[2][0] >= 4 and not got[0][0].any() and (got[1][0] == -1).all()
    # brute force of one kept row: first maximum, its barycentric weight
    r = int(np.flatnonzero(got[2] >= 4)[1])
    toks = np.flatnonzero(b["idx"] == r)
    for c in range(b["src"].shape[1]):
        t = toks[np.argmax(b["src"][toks, c])]
        assert got[1][r, c] == t and got[0][r, c] == b["src"][t, c] and got[0][r, 6 + c] == b["d"][t, -1]
    few = got[2] < 4
    assert few.any() and not got[0][few].any() and (got[1][few] == -1).all()


@pytest.mark.parametrize("sizes,short_last", [([30, 17, 25], 0), ([12, 0, 9, 1, 20], 0), ([0, 8, 8], 0), ([20, 20, 11], 130)])
def test_a_batch_is_its_clouds_done_alone(sizes, short_last):
    """Centred rows, maxima, winners (after adding the cloud's token offset) and gradients of the batch equal those of every cloud done
    alone under the row-0 rule with its indices rebased to its own first row."""
    tpc = 200
    b = V.make_batch(sizes, tpc, short_last=short_last)
    starts, idx = b["starts"], b["idx"]
    clouds = len(sizes)
    dist = V.distribute_centre(b["d"], idx, b["sums"], b["counts"], 3, tpc, starts)
    out, arg, counts = V.pointnet_reduce(b["src"], idx, b["d"][:, -1], b["rows"] + 3, 4, starts)  # (3 rows behind row_starts[B]: no tokens)
    assert not out[b["rows"]:].any() and (arg[b["rows"]:] == -1).all()
    rng = np.random.default_rng(1)
    grad_out = rng.standard_normal(out.shape).astype(np.float32)
    grad = V.pointnet_reduce_backward(grad_out, arg, idx, b["tokens"])
    for c in range(clouds):
        t0, t1 = c * tpc, min((c + 1) * tpc, b["tokens"])
        r0, r1 = int(starts[c]), int(starts[c + 1])
        local = np.where(idx[t0:t1] >= 0, idx[t0:t1] - r0, -1)
        assert ((local >= 0) <= (local < r1 - r0)).all()
        e = V.distribute_centre(b["d"][t0:t1], local, b["sums"][r0:r1], b["counts"][r0:r1], 3) if r1 > r0 else np.zeros_like(b["d"][t0:t1])
        assert np.array_equal(dist[t0:t1], e)
        if r1 == r0:
            assert not grad[t0:t1].any()
            continue
        eo, ea, ec = V.pointnet_reduce(b["src"][t0:t1], local, b["d"][t0:t1, -1], r1 - r0, 4)
        assert ec[0] >= 4, "the rule would be invisible"
        assert np.array_equal(out[r0:r1], eo) and np.array_equal(arg[r0:r1], np.where(ea >= 0, ea + t0, -1))
        assert not out[r0].any() and (arg[r0] == -1).all()
        eg = V.pointnet_reduce_backward(grad_out[r0:r1], ea, local, t1 - t0)
        assert np.array_equal(grad[t0:t1], eg)
        assert not grad[t0:t1][local == 0].any()  # every token of the dropped vertex: exactly zero
    assert grad.any()


def test_the_switch_on_the_host():
    """Default off, off when no batch is set, inherited by clones of the table state; asking for the ranges of a lattice that was never
    built from a batch raises what cloud_row_starts() raises, before anything touches a device."""
    import lattice_net_amd as L
    from lattice_net_amd import _lib
    lat = L.Lattice(sigmas=[1.0, 1.0, 1.0], capacity=1000, device="cpu")
    assert not lat.m_hash_table._per_cloud_invalid_vertex and lat.per_cloud_invalid_row_starts() is None and lat.points_per_cloud() == 0
    lat.set_cloud_batch(100, per_cloud_invalid_vertex=True)
    assert lat.m_hash_table._per_cloud_invalid_vertex and not lat.m_hash_table._per_cloud_norm and lat.points_per_cloud() == 100
    assert lat.per_cloud_norm_row_starts() is None and lat.cloud_segments() == 1
    with pytest.raises(_lib.LatticeNetHipError, match="not built from a batch"):
        lat.per_cloud_invalid_row_starts()
    lat.set_cloud_batch(100, per_cloud_norm=True)  # the default keeps today's behaviour
    assert not lat.m_hash_table._per_cloud_invalid_vertex and lat.per_cloud_invalid_row_starts() is None
    lat.set_cloud_batch(None, per_cloud_invalid_vertex=True)  # no batch: row 0 is the only invalid vertex
    assert not lat.m_hash_table._per_cloud_invalid_vertex and lat.per_cloud_invalid_row_starts() is None
    lat.set_cloud_batch(100, per_cloud_norm=True, per_cloud_invalid_vertex=True)
    assert lat.m_hash_table._per_cloud_invalid_vertex and lat.m_hash_table._per_cloud_norm
    clone = L.Lattice._clone_of(lat)  # (coarser levels: tests/test_gpu_lnn_cloud_batch.py, they need a device)
    assert clone.m_hash_table._per_cloud_invalid_vertex and clone.m_hash_table._per_cloud_norm and clone.points_per_cloud() == 100
    lat.set_cloud_batch(100)
    assert not L.Lattice._clone_of(lat).m_hash_table._per_cloud_invalid_vertex


def test_entry_points_reject_bad_arguments_on_the_host():
    import ctypes as C
    from lattice_net_amd import _lib
    lib = _lib.load()
    dc = lambda tokens=10, width=5, pos_dim=3, tpc=4, starts=16, clouds=2, out=16: lib.ln_distribute_centre_clouds(
        16, 16, 16, 16, tokens, width, pos_dim, tpc, starts, clouds, out, None)
    assert dc(clouds=65) == -2 and b"clouds" in lib.ln_last_error_string()
    assert dc(clouds=0) == -2
    assert dc(tpc=0) == -1 and dc(pos_dim=6) == -1 and dc(starts=None) == -1 and dc(out=None) == -1
    assert dc(tokens=0) == 0  # nothing to do, nothing launched
    csr = _lib.LnCsr(16, 16, 16, 16, 0, None, 0)
    pr = lambda rows=10, clouds=2, starts=16, ws_bytes=1 << 20, ch=8: lib.ln_pointnet_reduce_forward_clouds(
        C.byref(csr), None, 5, 16, ch, 16, 5, rows, 4, 16, ws_bytes, 16, 16, starts, clouds, None)
    assert pr(clouds=65) == -2 and b"clouds" in lib.ln_last_error_string()
    assert pr(clouds=0) == -2
    assert pr(starts=None) == -1 and pr(ch=0) == -1
    assert pr(ws_bytes=8) != 0 and b"workspace" in lib.ln_last_error_string()
    assert pr(rows=0) == 0
    names = lib.ln_kernel_names().decode().split(",")
    assert "k_distribute_centre_clouds" in names and "k_pointnet_reduce_decode_clouds" in names
