"""tests/conv_reference.py on the CPU: the lists hold what they promise, the three references agree with an independent evaluation (a
torch fp64 autograd graph through the padded gather of test_conv_autograd_matches_dense_reference), and the comparisons reject every
seeded mistake a two-lattice convolution kernel can make that a single lattice hides.  One small shape: mq = 200 query rows, mn = 131
gathered rows, E = 9, 8 -> 16 channels."""
import numpy as np
import pytest
import torch

from tests import conv_reference as C

MQ, MN, E, V, F = 200, 131, 9, 8, 16
RTOL = 1e-5


def _padded_rows(x, nbr, absent_reads_row0=False):
    """[rows, E, channels]: rows of x by id, the zero row appended behind x for an absent neighbour"""
    nbr = torch.from_numpy(np.asarray(nbr).astype(np.int64))
    padded = torch.cat([x, torch.zeros((1, x.shape[1]), dtype=x.dtype)], 0)
    return padded[torch.where(nbr >= 0, nbr, torch.full_like(nbr, 0 if absent_reads_row0 else x.shape[0]))]


def _flipped(nbr, mistake=None):
    """the list as the value gradient reads it"""
    nbr = np.asarray(nbr)
    rows, e = nbr.shape
    if mistake == "not flipped":
        return nbr
    if mistake == "last slot flipped":  # e ^ 1 at every slot: the last one reads the first slot of the next row (nothing behind the list)
        flat = np.concatenate([nbr.reshape(-1), [-1]])
        return flat[np.arange(rows)[:, None] * e + (np.arange(e) ^ 1)[None, :]]
    return nbr[:, C.flip_slots(e)]


def _autograd_products(nbr_q, nbr_n, vals, W, G, mistake=None):
    """(out, gW, gv) in fp64 from torch autograd; `mistake`: one of the seeded ones"""
    r0 = mistake == "absent reads row 0"
    if mistake == "ids clamped":  # to the list's own row count, as on a single lattice
        nbr_q, nbr_n = np.minimum(nbr_q, nbr_q.shape[0] - 1), np.minimum(nbr_n, nbr_n.shape[0] - 1)
    v64 = torch.from_numpy(C.f64(vals))
    w64 = torch.from_numpy(C.f64(W)).requires_grad_(True)
    g64 = torch.from_numpy(C.f64(G))
    out = _padded_rows(v64, nbr_q, r0).reshape(nbr_q.shape[0], -1) @ w64
    (out * g64).sum().backward()
    # value gradient: d/dx of sum_n <x[n], sum_e B_e^T G[nbr_n[n, flip e]]> with B_e = W[e V:(e + 1) V, :]
    x = torch.zeros((nbr_n.shape[0], v64.shape[1]), dtype=torch.float64, requires_grad=True)
    ev, f = W.shape
    e = nbr_n.shape[1]
    bank = w64.detach().reshape(e, ev // e, f)
    if mistake == "bank transposed whole":  # the [F, E V] transpose of the whole bank read as E slots of [F, V]
        bank = w64.detach().t().contiguous().reshape(e, f, ev // e).transpose(1, 2)
    g_rows = _padded_rows(g64, _flipped(nbr_n, mistake), r0)  # [mn, E, F]
    torch.einsum("nef,evf,nv->", g_rows, bank, x).backward()
    return out.detach().numpy(), w64.grad.numpy(), x.grad.numpy()


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(7)
    nbr_q, nbr_n = C.two_lattice_lists(MQ, MN, E, rng)
    vals, W, G = C.operands("random", MQ, MN, E, V, F, rng)
    refs = (C.forward(nbr_q, vals, W), C.grad_filter(nbr_q, vals, G), C.grad_values(nbr_n, G, W))
    return nbr_q, nbr_n, vals, W, G, refs


@pytest.fixture(scope="module")
def exact_case():
    rng = np.random.default_rng(8)
    nbr_q, nbr_n = C.two_lattice_lists(MQ, MN, E, rng)
    vals, W, G = C.operands("exact", MQ, MN, E, V, F, rng)
    refs = (C.forward(nbr_q, vals, W), C.grad_filter(nbr_q, vals, G), C.grad_values(nbr_n, G, W))
    return nbr_q, nbr_n, vals, W, G, refs


@pytest.mark.parametrize("mq,mn", [(MQ, MN), (MN, MQ), (4500, 1300)])
@pytest.mark.parametrize("unreferenced", [False, True])
def test_lists_hold_every_planted_case(mq, mn, unreferenced):
    nbr_q, nbr_n = C.two_lattice_lists(mq, mn, E, np.random.default_rng(mq), unreferenced)
    assert nbr_q.shape == (mq, E) and nbr_n.shape == (mn, E) and nbr_q.dtype == nbr_n.dtype == np.int32
    for nbr, into in ((nbr_q, mn), (nbr_n, mq)):
        p = C.list_properties(nbr, into)
        assert p["in_range"] and p["all_absent_rows"] >= 1 and p["full_rows"] >= 1 and p["has_largest"] and p["hot"] >= 64, p
        assert p["has_zero"] == (not unreferenced), p
        assert bool(np.all(nbr[-1] == -1)), "the wholly absent row sits in the partial last tile"
        assert not np.array_equal(nbr[:, E - 1], np.minimum(np.arange(nbr.shape[0]), into - 1)), "no identity slot"


def test_references_agree_with_autograd_through_the_padded_gather(case):
    nbr_q, nbr_n, vals, W, G, refs = case
    got = _autograd_products(nbr_q, nbr_n, vals, W, G)
    for name, g, (ref, bound) in zip(("forward", "grad_filter", "grad_values"), got, refs):
        assert C.within(g, ref, bound, 1e-13, name) <= 1.0  # two fp64 evaluations in different orders
        assert np.all(bound >= np.abs(ref))
    assert np.all(refs[0][0][-1] == 0) and np.all(refs[0][1][-1] == 0)  # the wholly absent row: zero, and nothing allowed


def test_value_gradient_is_the_adjoint_on_mutual_lists():
    """Where the two lists ARE mutual (nbr_q[a, e] = b <=> nbr_n[b, e ^ 1] = a, the last slot its own partner) grad_values is the
    gradient of `forward` with respect to vals: the flip and the per-slot transpose are the right ones."""
    rng = np.random.default_rng(3)
    nbr_q, nbr_n = np.full((MQ, E), -1, np.int32), np.full((MN, E), -1, np.int32)
    for e, partner in enumerate(C.flip_slots(E)):
        k = int(0.7 * MN)
        a, b = rng.permutation(MQ)[:k], rng.permutation(MN)[:k]
        nbr_q[a, e] = b
        nbr_n[b, partner] = a
    vals, W, G = C.operands("random", MQ, MN, E, V, F, rng)
    v64 = torch.from_numpy(C.f64(vals)).requires_grad_(True)
    out = _padded_rows(v64, nbr_q).reshape(MQ, -1) @ torch.from_numpy(C.f64(W))
    (out * torch.from_numpy(C.f64(G))).sum().backward()
    ref, bound = C.grad_values(nbr_n, G, W)
    C.within(v64.grad.numpy(), ref, bound, 1e-13, "grad_values on mutual lists")


# which of the three products each mistake must show in
@pytest.mark.parametrize("mistake,shows_in", [("not flipped", [2]), ("last slot flipped", [2]), ("bank transposed whole", [2]),
                                              ("absent reads row 0", [0, 1, 2]), ("ids clamped", [2])])
def test_wrong_formulas_are_rejected(case, mistake, shows_in):
    nbr_q, nbr_n, vals, W, G, refs = case
    got = _autograd_products(nbr_q, nbr_n, vals, W, G, mistake)
    for k, name in enumerate(("forward", "grad_filter", "grad_values")):
        if k in shows_in:
            with pytest.raises(AssertionError):
                C.within(got[k], refs[k][0], refs[k][1], RTOL, f"{mistake}: {name}")
        else:
            C.within(got[k], refs[k][0], refs[k][1], RTOL, f"{mistake}: {name}")


def test_wrong_formulas_are_rejected_in_the_exact_family(exact_case):
    nbr_q, nbr_n, vals, W, G, refs = exact_case
    for (ref, bound) in refs:
        C.assert_exact_family(bound)
    for g, (ref, _) in zip(_autograd_products(nbr_q, nbr_n, vals, W, G), refs):
        C.exact(g, ref)
    for mistake in ("not flipped", "last slot flipped", "bank transposed whole", "absent reads row 0", "ids clamped"):
        got = _autograd_products(nbr_q, nbr_n, vals, W, G, mistake)
        with pytest.raises(AssertionError):
            C.exact(got[2], refs[2][0], mistake)


def test_ids_clamped_to_the_own_row_count_show_in_the_forward_of_the_swapped_pair(case):
    """mn > mq seen from the forward: 131 query rows gathering from 200"""
    nbr_q, nbr_n, vals, W, G, _ = case
    ref, bound = C.forward(nbr_n, G, W.reshape(E, V, F).transpose(0, 2, 1).reshape(E * F, V))
    wrong, _ = C.forward(np.minimum(nbr_n, MN - 1), G, W.reshape(E, V, F).transpose(0, 2, 1).reshape(E * F, V))
    with pytest.raises(AssertionError):
        C.within(wrong, ref, bound, RTOL)


def test_unwritten_tail_rows_are_rejected(case, exact_case):
    assert MQ % 64 == 8
    for nbr_q, nbr_n, vals, W, G, refs in (case, exact_case):
        ref, bound = refs[0]
        for fill in (np.nan, np.inf, 0.0):  # NaN pre-fill left in place; or a buffer that happened to hold zeros
            got = ref.copy()
            got[MQ - MQ % 64:MQ - 1] = fill  # (row MQ - 1 is the wholly absent one: zero is right there)
            with pytest.raises(AssertionError):
                C.within(got, ref, bound, RTOL)
            with pytest.raises(AssertionError):
                C.exact(got, ref)


def test_one_element_off_is_rejected(case, exact_case):
    for k in range(3):
        ref, bound = case[5][k]
        i = np.unravel_index(int(np.argmax(bound)), bound.shape)
        got = ref.copy()
        got[i] += 0.5 * RTOL * bound[i]
        assert 0.49 < C.within(got, ref, bound, RTOL) < 0.51
        got[i] = ref[i] - 16 * RTOL * bound[i]
        with pytest.raises(AssertionError, match="16"):
            C.within(got, ref, bound, RTOL)
        ref, _ = exact_case[5][k]
        got = ref.copy()
        got[i] += 1
        with pytest.raises(AssertionError):
            C.exact(got, ref)
    # fp16 results: one rounding of the result on top
    ref, bound = case[5][0]
    half = ref.astype(np.float16).astype(np.float64)
    C.within(half, ref, bound, RTOL, rel=2.0 ** -11)
    with pytest.raises(AssertionError):
        C.within(half, ref, bound, RTOL)


def test_exact_family_conditions():
    rng = np.random.default_rng(0)
    for half in (False, True):
        vals, W, G = C.operands("exact", MQ, MN, E, 256, 256, rng, half)
        for x in (vals, W, G):
            assert np.array_equal(x, np.round(x)) and np.abs(x).max() <= 3
        nbr_q, nbr_n = C.two_lattice_lists(MQ, MN, E, rng)
        ref, bound = C.forward(nbr_q, vals, W)
        C.assert_exact_family(bound, ref, half)
    with pytest.raises(AssertionError):
        C.assert_exact_family(np.full((2, 2), 2.0 ** 24))
    with pytest.raises(AssertionError):
        C.assert_exact_family(np.ones((2, 2)), np.full((2, 2), 2048.0), True)
    vals, W, G = C.operands("random", MQ, MN, E, V, F, rng, half=True)
    for x in (vals, W, G):
        assert np.array_equal(x, x.astype(np.float16).astype(np.float32))


@pytest.mark.parametrize("extent", [1, 5, 7, 11, 13, 15, 17])
@pytest.mark.parametrize("unreferenced", [False, True])
def test_lists_hold_every_planted_case_at_every_extent(extent, unreferenced):
    """What the lists plant at E = 9 they plant at every extent from 1 on (at E = 1 the repeats of one id sit in slot 0, the only one)"""
    for mq, mn in ((MQ, MN), (MN, MQ), (4500, 1300)):
        nbr_q, nbr_n = C.two_lattice_lists(mq, mn, extent, np.random.default_rng(mq + extent), unreferenced)
        assert nbr_q.shape == (mq, extent) and nbr_n.shape == (mn, extent) and nbr_q.dtype == nbr_n.dtype == np.int32
        for nbr, into in ((nbr_q, mn), (nbr_n, mq)):
            p = C.list_properties(nbr, into)
            assert p["in_range"] and p["all_absent_rows"] >= 1 and p["full_rows"] >= 2 and p["has_largest"] and p["hot"] >= C.HOT_ROWS, p
            assert p["has_zero"] == (not unreferenced), p
            assert int(nbr.min()) == -1 and int(nbr[nbr >= 0].min()) == (1 if unreferenced else 0), "the smallest id is named"
            assert bool(np.all(nbr[-1] == -1)), "the wholly absent row sits in the partial last tile"
            assert bool(np.all(nbr[0] >= 0)) and bool(np.all(nbr[-2] >= 0)), "rows 0 and rows - 2 are whole"
            hot = nbr[3:3 + C.HOT_ROWS, min(1, extent - 1)]
            assert bool(np.all(hot == into - 1)) and 3 < 64 < 3 + C.HOT_ROWS, "the repeats cross a 64-row tile boundary"
            assert not np.array_equal(nbr[:, extent - 1], np.minimum(np.arange(nbr.shape[0]), into - 1)), "no identity slot"


@pytest.mark.parametrize("unreferenced", [False, True])
def test_permutation_lists_are_injective_with_absent_entries(unreferenced):
    for mq, mn in ((MQ, MN), (4500, 1300), (1300, 4500)):
        nbr_q, nbr_n = C.permutation_lists(mq, mn, np.random.default_rng(mq), unreferenced)
        for nbr, into in ((nbr_q, mn), (nbr_n, mq)):
            assert nbr.shape[1] == 1 and nbr.dtype == np.int32
            ids = nbr[nbr >= 0]
            p = C.list_properties(nbr, into)
            assert p["in_range"] and p["hot"] == 1 and ids.size == np.unique(ids).size, "every id at most once"
            assert p["has_largest"] and p["has_zero"] == (not unreferenced) and int(ids.min()) == (1 if unreferenced else 0)
            assert nbr[-1, 0] == -1 and nbr[0, 0] >= 0 and nbr[-2, 0] >= 0 and int(np.sum(nbr < 0)) >= nbr.shape[0] // 10
            assert ids.size >= min(nbr.shape[0], into) // 2
            assert not np.array_equal(nbr[:, 0], np.arange(nbr.shape[0])), "not the identity"


def test_the_flip_is_the_identity_at_an_extent_of_one():
    assert C.flip_slots(1) == [0]
    assert C.flip_slots(5) == [1, 0, 3, 2, 4] and C.flip_slots(9) == [1, 0, 3, 2, 5, 4, 7, 6, 8]
    rng = np.random.default_rng(11)
    for lists in (C.two_lattice_lists, lambda mq, mn, e, r: C.permutation_lists(mq, mn, r)):
        nbr_q, nbr_n = lists(MQ, MN, 1, rng)
        vals, W, G = C.operands("random", MQ, MN, 1, V, F, rng)
        for transposed, x, nbr, bank in ((False, vals, nbr_q, W), (True, G, nbr_n, W)):
            plain, flipped = C.forward(nbr, x, bank, flip=False, transposed=transposed), C.forward(nbr, x, bank, flip=True, transposed=transposed)
            assert np.array_equal(plain[0], flipped[0]) and np.array_equal(plain[1], flipped[1])
    # ... and nowhere else: at E = 5 the flipped forward differs
    nbr_q, _ = C.two_lattice_lists(MQ, MN, 5, rng)
    vals, W, _ = C.operands("random", MQ, MN, 5, V, F, rng)
    assert not np.array_equal(C.forward(nbr_q, vals, W, flip=True)[0], C.forward(nbr_q, vals, W)[0])


@pytest.mark.parametrize("extent", [1, 7, 17])
def test_references_agree_with_autograd_at_other_extents(extent):
    rng = np.random.default_rng(extent)
    nbr_q, nbr_n = C.two_lattice_lists(MQ, MN, extent, rng)
    vals, W, G = C.operands("random", MQ, MN, extent, V, F, rng)
    refs = (C.forward(nbr_q, vals, W), C.grad_filter(nbr_q, vals, G), C.grad_values(nbr_n, G, W))
    for name, g, (ref, bound) in zip(("forward", "grad_filter", "grad_values"), _autograd_products(nbr_q, nbr_n, vals, W, G), refs):
        assert C.within(g, ref, bound, 1e-13, name) <= 1.0


@pytest.mark.parametrize("unreferenced", [False, True])
def test_small_list_holds_what_it_plants_from_one_row_on(unreferenced):
    """C.small_list at the row counts of the kernels' tile edges: the first row complete, the last row wholly absent where there is
    more than one, the largest id named, every id in range, and the references take such a list (one row gives one full row)."""
    into = 37
    for rows in (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 511, 512, 513, 577):
        for e in (1, 9):
            nbr = C.small_list(rows, into, e, np.random.default_rng(rows + e), unreferenced)
            assert nbr.shape == (rows, e) and nbr.dtype == np.int32
            p = C.list_properties(nbr, into)
            assert p["in_range"] and p["has_largest"] and bool(np.all(nbr[0] >= 0)) and nbr[0, e - 1] == into - 1, p
            assert not (unreferenced and p["has_zero"]), p
            if rows > 1:
                assert bool(np.all(nbr[-1] == -1)) and p["all_absent_rows"] >= 1
            else:
                assert p["all_absent_rows"] == 0 and p["full_rows"] == 1
            if rows >= 15 and e == 9:  # about one entry in eight: absent neighbours inside the tile, not only in the planted last row
                inner = nbr[1:-1]
                assert 0.04 < float(np.mean(inner < 0)) < 0.25, float(np.mean(inner < 0))
    nbr = C.small_list(1, into, E, np.random.default_rng(0))
    vals, W, G = C.operands("exact", 1, into, E, V, F, np.random.default_rng(1))
    ref, bound = C.forward(nbr, vals, W)
    assert ref.shape == (1, F) and np.array_equal(ref[0], sum(vals[nbr[0, e]].astype(np.float64) @ W[e * V:(e + 1) * V] for e in range(E)))
    gw, _ = C.grad_filter(nbr, vals, G)
    assert np.array_equal(gw, np.concatenate([np.outer(vals[nbr[0, e]], G[0]) for e in range(E)]).astype(np.float64))
