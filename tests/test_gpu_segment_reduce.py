"""The CSR segment reduce (ln_csr.hip: k_csr_reduce_segments, k_reduce_and_neighbours) against an fp64 scatter, element by
element (`pytest -m gpu`).

Every scatter onto lattice vertices goes through this kernel: the splat accumulate (fused with the same-level neighbour traversal),
the slice, gather and slice-classify backwards (Lattice._scatter_rows), with fp32 and with fp16 source rows.  The dispatch
(ln_csr_reduce_rows_impl, ln_splat_tail_impl) picks a template instance <VEC, HALF, WG, L8> from the row width, the source dtype and
alignment, the dense hint (LnCsr.dense & 1) and deterministic mode (LnCsr.dense & 2); the widths and modes below reach every
instance, over every origin of the CSR: the bucketed build in slot and in canonical row order, the atomic build path, eight kd
regions under both slot orders, and ln_csr_build from a synthetic index with chosen token counts per row.

Each case runs twice:
- random sources and weights: every finite element within (LN_CSR_SEG + nseg(row) + 1) * 2^-24 * sum|x * w| of the fp64 scatter (the
  fma chain of one segment, then the combination of the row's segments), and NaN / +Inf / -Inf exactly where the fp64 scatter has them;
- integer sources with unit weights: every partial sum is exact in fp32, so the result must equal the integer sum bit for bit in any
  summation order — a token that is dropped, duplicated or sent to another row shows whatever its magnitude."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LN_CSR_SEG = 16  # csrc/ln_csr.h: CSR entries per segment (the sequential fma chain of one lane group)
EPS32 = 2.0 ** -24
MODES = ("plain", "dense", "deterministic")
ORIGINS = ("slot", "canonical", "atomic", "regions_hash", "regions_space", "csr_build")
WIDTHS = {torch.float32: (1, 3, 4, 12, 28, 32, 36, 96, 256, 264),  # 264: more float4 chunks than 64 lanes
          torch.float16: (5, 32, 60, 64, 72, 520)}
# token counts of the rows of the synthetic index: around the batches of 4 entries, the segments of 16, a wave's worth of segments
# (8 lanes per segment: 8 segments = 128 entries), a workgroup (32 segments), and one row over many workgroups
EDGE_COUNTS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 128, 256, 512, 1024, 4100)


def dev():
    return torch.device("cuda", 0)


# ---------------------------------------------------------------------------------------------------------- reference and bounds
def reduce_reference(src, idx, w, rows, val_dim, src_div, src_stride):
    """fp64 scatter on the CPU: dst[row, j] = sum over the row's tokens t of x[t // src_div, j] * w[t], x[r, j] = src[r * src_stride + j].
    Returns (sum, sum |x * w|, tokens per row); ids outside [0, rows) are ignored.  fp16 sources are converted exactly."""
    idx = idx.detach().cpu().long().reshape(-1)
    w = w.detach().cpu().double().reshape(-1)
    flat = src.detach().reshape(-1).cpu().double()
    nsrc = (flat.numel() - val_dim) // src_stride + 1
    x = torch.as_strided(flat, (nsrc, val_dim), (src_stride, 1))
    t = torch.arange(idx.numel())
    ok = (idx >= 0) & (idx < rows)
    t, r = t[ok], idx[ok]
    ij = torch.stack([r, t // src_div])

    def spmm(vals, xs):
        return torch.sparse.mm(torch.sparse_coo_tensor(ij, vals, (rows, nsrc)).coalesce(), xs)

    # (|x * w| summed over tokens = |x| times the sum of |w| over the tokens of one (row, source row) pair)
    return spmm(w[t], x), spmm(w[t].abs(), x.abs()), torch.bincount(r, minlength=rows)


def reduce_bound(mag, count, deterministic=False, extra=0):
    """Per-element error bound of the reduce: (LN_CSR_SEG + nseg(row) + 1) * 2^-24 * sum|x * w|.  A segment is a chain of at most
    LN_CSR_SEG fmas; the nseg(row) partial sums of a row then combine through shuffles, LDS and atomics in any order.  In deterministic
    mode one lane group walks the whole row: a single chain of count(row) fmas.  `extra`: roundings the source rows already carry
    (e.g. the C-term dot product in front of the slice-classify backward), counted against the same sum |x * w|."""
    count = count.double()
    nseg = torch.ceil(count / LN_CSR_SEG)
    k = (count + 1 if deterministic else LN_CSR_SEG + nseg + 1) + extra
    return k[:, None] * EPS32 * mag


def row_counts(idx, rows):
    """Tokens per row of a splat-index array (ids outside [0, rows) ignored)."""
    idx = torch.as_tensor(np.asarray(idx.detach().cpu() if torch.is_tensor(idx) else idx)).long().reshape(-1)
    return torch.bincount(idx[(idx >= 0) & (idx < rows)], minlength=rows)


def _first(mask):
    return tuple(int(i) for i in torch.nonzero(mask)[0])


def assert_reduce_close(got, ref, mag, count, deterministic=False, what="", extra=0):
    """Element by element: the same NaN / +Inf / -Inf pattern as the fp64 reference, finite elements within reduce_bound (compared on
    got's device).  Tensors or NumPy arrays; ref and mag in fp64."""
    got = (got.detach() if torch.is_tensor(got) else torch.as_tensor(np.asarray(got))).double()
    ref, mag, count = (torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(got.device) for a in (ref, mag, count))
    ref, mag = ref.double(), mag.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    for f in (torch.isnan, torch.isposinf, torch.isneginf):
        bad = f(got) != f(ref)
        if bad.any():
            i = _first(bad)
            raise AssertionError(f"{what}: {f.__name__} differs in {int(bad.sum())} elements, first {i}: got {float(got[i])!r}, "
                                 f"fp64 {float(ref[i])!r}")
    fin = torch.isfinite(ref)
    bound = reduce_bound(mag, count, deterministic, extra)
    err = torch.where(fin, (got - ref).abs(), torch.zeros_like(ref))
    bad = err > torch.where(fin, bound, torch.zeros_like(bound))
    if bad.any():
        i = _first(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside the bound, first {i}: got {float(got[i])!r}, fp64 {float(ref[i])!r}, "
                             f"bound {float(bound[i]):.3e}, tokens {int(count[i[0]])}")


def assert_exact(got, ref, what=""):
    """Integer sources, unit weights: the fp32 result is the integer sum itself."""
    assert bool(torch.all(ref == torch.round(ref))) and float(ref.abs().max()) < 2 ** 24, what
    got = got.detach().double()
    ref = ref.to(got.device)
    bad = got != ref
    if bad.any():
        i = _first(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} elements differ from the integer sum, first {i}: got {float(got[i])!r}, "
                             f"exact {float(ref[i])!r}")


# ---------------------------------------------------------------------------------------------------------- sources, CSR origins, modes
def make_src(nrows, stride, dtype, form, rng):
    """Flat source of nrows rows of `stride` elements: N(0, 1) values, or integers (r % 251) - 125 + j (exact in fp16 up to 2048)."""
    if form == "exact":
        r = torch.arange(nrows, device=dev())[:, None]
        return ((r % 251) - 125 + torch.arange(stride, device=dev())[None, :]).reshape(-1).to(dtype)
    g = torch.Generator(device=dev())
    g.manual_seed(int(rng.integers(2 ** 62)))
    return torch.randn((nrows * stride,), generator=g, device=dev()).to(dtype)


def make_w(tokens, form, rng):
    if form == "exact":
        return torch.ones((tokens,), device=dev())
    return torch.from_numpy(rng.uniform(-1.0, 1.0, tokens).astype(np.float32)).to(dev())


@contextlib.contextmanager
def reduce_mode(mode):
    """plain: no dense hint (what a table that has not reported a vertex count gets); dense: LnCsr.dense & 1 (workgroup combining);
    deterministic: sorted token lists, one lane group per row (set_deterministic)."""
    from lattice_net_amd import lattice as LL
    saved = LL._DENSE_TOKENS_PER_VERTEX
    prev = LL.set_deterministic(mode == "deterministic")
    LL._DENSE_TOKENS_PER_VERTEX = 0.0 if mode == "dense" else 1e9
    try:
        yield
    finally:
        LL._DENSE_TOKENS_PER_VERTEX = saved
        LL.set_deterministic(prev)


SPAN = {1: 300.0, 2: 40.0, 3: 8.0, 4: 4.0, 6: 2.0}  # half-width of the uniform part of hot_cloud: mostly rows of a few tokens


def hot_cloud(d, seed, n_uniform=2500, n_dup=25, copies=40, n_hot=2500):
    """Uniform points + 25 points repeated 40 times + one point repeated 2500 times (its d + 1 vertices carry 2500+ tokens: about 160
    segments, several workgroups of them)."""
    rng = np.random.default_rng(seed)
    parts = [rng.uniform(-SPAN[d], SPAN[d], (n_uniform, d)), np.repeat(rng.uniform(-2, 2, (n_dup, d)), copies, 0),
             np.tile(rng.uniform(-0.5, 0.5, (1, d)), (n_hot, 1))]
    pos = np.concatenate(parts, 0).astype(np.float32)
    return np.ascontiguousarray(pos[rng.permutation(len(pos))])


def csr_seg_count(lat, idx):
    from lattice_net_amd import _lib
    buf = lat._csr(idx)[0]
    return buf[-(_lib.LN_XCD_GROUPS + 2):].cpu().numpy()


def build_origin(origin, pos_np, sigma, cap):
    """A lattice over pos_np and the splat indices whose CSR the reduce will walk (the build's own, or ln_csr_build's for a synthetic
    index).  Settings are restored before returning; the CSR stays cached with the index tensor."""
    import lattice_net_amd as L
    from lattice_net_amd import lattice as LL
    prev_order, prev_slot, prev_atomic = LL.get_row_order(), LL.set_slot_order("hash"), LL._FORCE_ATOMIC_BUILD
    try:
        LL.set_row_order("canonical" if origin == "canonical" else "slot")
        LL._FORCE_ATOMIC_BUILD = origin == "atomic"
        lat = L.Lattice(sigmas=[sigma] * pos_np.shape[1], capacity=cap, device=dev())
        pos = torch.from_numpy(pos_np).to(dev())
        lat.begin_splat()
        idx, _ = lat.just_create_verts(pos, True)
        lat.nr_lattice_vertices()
        if origin.startswith("regions"):
            LL.set_slot_order(origin.split("_")[1])
            planes, shares = lat.balanced_region_planes(idx, return_shares=True)
            lat.set_region_planes(planes, shares)
            lat.begin_splat()
            idx, _ = lat.just_create_verts(pos, True)
            lat.nr_lattice_vertices()
            assert csr_seg_count(lat, idx)[LL._lib.LN_XCD_GROUPS] == 8, "the build did not file its segments under 8 regions"
    finally:
        LL.set_row_order(prev_order)
        LL.set_slot_order(prev_slot)
        LL._FORCE_ATOMIC_BUILD = prev_atomic
    if origin == "csr_build":
        idx = synthetic_index(cap, seed=7)
    return lat, idx


def synthetic_index(rows_upper, seed):
    """int32 ids: rows with EDGE_COUNTS tokens, 3000 rows with 1..40, ids of -1 and >= rows_upper (ignored); tokens in random order."""
    rng = np.random.default_rng(seed)
    rows = rng.choice(rows_upper, len(EDGE_COUNTS) + 3000, replace=False)
    counts = np.concatenate([EDGE_COUNTS, rng.integers(1, 41, 3000)])
    counts[int(np.argmax(rows))] = 33  # (the highest row in use: 33 tokens)
    ids = np.concatenate([np.repeat(rows, counts), np.full(40, -1), rows_upper + rng.integers(0, 1000, 40), np.full(3, 2 ** 31 - 1)])
    return torch.from_numpy(ids[rng.permutation(len(ids))].astype(np.int32)).to(dev())


# ---------------------------------------------------------------------------------------------------------- one width, every path
def check_width(lat, idx, src_div, dtype, v, form, mode, rng, what, paths=("scatter", "fused", "offset", "gather")):
    """The reduce of `idx` at width v through _scatter_rows (rows of src_div tokens' source, stride v), the fused splat tail, a source
    view offset by one element (scalar lanes), and the gather-backward form (one (v + 1)-wide source row per token)."""
    rows = lat.m_hash_table.capacity()
    tokens = idx.numel()
    det = mode == "deterministic"
    w = make_w(tokens, form, rng)

    def check(dst, ref, tag):
        if form == "exact":
            assert_exact(dst, ref[0], f"{what} v={v} {tag}")
        else:
            assert_reduce_close(dst, *ref, deterministic=det, what=f"{what} v={v} {tag}")

    nsrc = -(-tokens // src_div)
    src = make_src(nsrc, v, dtype, form, rng)
    ref = reduce_reference(src, idx, w, rows, v, src_div, v)
    for path in paths:
        dst = torch.zeros((rows, v), dtype=torch.float32, device=dev())
        if path == "scatter":
            lat._scatter_rows(src.view(nsrc, v), idx, w, dst, v, src_div, v)
        elif path == "fused":
            lat._accumulate_and_prefetch(src.view(nsrc, v), idx, w, dst, v, src_div, tokens)
        elif path == "offset":
            buf = torch.empty((src.numel() + 1,), dtype=dtype, device=dev())
            buf[1:] = src
            lat._scatter_rows(buf[1:], idx, w, dst, v, src_div, v)
        else:
            continue
        check(dst, ref, path)
    if "gather" in paths:
        src = make_src(tokens, v + 1, dtype, form, rng)
        ref = reduce_reference(src, idx, w, rows, v, 1, v + 1)
        dst = torch.zeros((rows, v), dtype=torch.float32, device=dev())
        lat._scatter_rows(src.view(tokens, v + 1), idx, w, dst, v, 1, v + 1)
        check(dst, ref, "gather")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("origin", ORIGINS)
def test_segment_reduce_matches_fp64_scatter(origin, mode, dtype):
    """Every width of WIDTHS[dtype] through every path of check_width, random and integer-exact, over one CSR origin in one mode."""
    rng = np.random.default_rng(6 * ORIGINS.index(origin) + 2 * MODES.index(mode) + (dtype == torch.float16))
    with reduce_mode(mode):
        lat, idx = build_origin(origin, hot_cloud(3, seed=1), 0.5, 20000)
        if origin != "csr_build":
            counts = torch.bincount(idx[idx >= 0].long())
            assert int(counts.max()) >= 2500 and int((counts >= 40).sum()) >= 25  # hot rows over several segments / workgroups
        for v in WIDTHS[dtype]:
            for form in ("random", "exact"):
                check_width(lat, idx, 4, dtype, v, form, mode, rng, f"{origin}/{mode}/{form}")


@pytest.mark.parametrize("d", [1, 2, 4, 6])
def test_fused_splat_tail_other_dimensions(d):
    """k_reduce_and_neighbours<VEC, D, ...> for the other position dimensions (D = 3 runs above): src_div = d + 1 a power of two (d = 1)
    and not (d = 2, 4, 6); fp32 rows of 3, 32 and 96 channels and fp16 rows of 64, plain and dense."""
    rng = np.random.default_rng(d)
    for mode in ("plain", "dense"):
        with reduce_mode(mode):
            lat, idx = build_origin("slot", hot_cloud(d, seed=d, n_hot=1200), 0.6, 40000)
            for dtype, widths in ((torch.float32, (3, 32, 96)), (torch.float16, (64,))):
                for v in widths:
                    for form in ("random", "exact"):
                        check_width(lat, idx, d + 1, dtype, v, form, mode, rng, f"d={d}/{mode}/{form}", paths=("scatter", "fused"))


# ---------------------------------------------------------------------------------------------------------- the public splat
@pytest.mark.parametrize("dtype,v", [(torch.float32, 32), (torch.float16, 64), (torch.float16, 32)], ids=["f32x32", "f16x64", "f16x32"])
def test_splat_values_first_and_steady_state_build(dtype, v):
    """SplatLattice twice on the same lattice: the first build (no vertex count known yet: no dense hint) and the second, which the dense
    hint of the first count steers to the workgroup-combining instances on a dense cloud (the C5 steady state: k_reduce_and_neighbours
    <8, 3, true, true, 8> at fp16 x 64)."""
    import lattice_net_amd as L
    from lattice_net_amd.synthetic import lidar_cloud
    n = 60000
    pos = torch.from_numpy(lidar_cloud(n, 9)).to(dev())
    rng = np.random.default_rng(v)
    vals = torch.from_numpy(rng.standard_normal((n, v)).astype(np.float32)).to(dev()).to(dtype)
    lat = L.Lattice(sigmas=[2.0] * 3, capacity=100000, device=dev())  # coarse cells: about 30 tokens per vertex
    for step in range(2):
        lv, _, idx, w = L.SplatLattice.apply(lat, pos, vals)
        m = lat.nr_lattice_vertices()
        assert 4 * n >= 16 * m
        ref = reduce_reference(vals, idx, w, lv.shape[0], v, 4, v)
        assert_reduce_close(lv, *ref, what=f"splat {step}")


# ---------------------------------------------------------------------------------------------------------- non-finite sources
def poison(idx, rows, tokens, stride, dtype, rng):
    """Random finite sources (one row per token) with +-Inf / NaN on chosen tokens: every token of rows whose count is 1, 2 or 3 mod 4
    (so that the last entry of every segment is non-finite), the last (largest) token of other such rows, a middle token of rows of
    5+ tokens (NaN in one channel, -Inf in all), and token 0."""
    ids = idx.cpu().numpy()
    src = rng.standard_normal((tokens, stride)).astype(np.float32)
    ok = (ids >= 0) & (ids < rows)
    order = np.argsort(np.where(ok, ids, rows), kind="stable")
    order = order[:int(ok.sum())]
    starts = np.searchsorted(ids[order], np.arange(rows + 1))
    cnt = np.diff(starts)
    for res, val in ((1, np.inf), (2, -np.inf), (3, np.inf)):
        sel = np.nonzero((cnt % 4 == res) & (cnt > 0))[0]
        rng.shuffle(sel)
        for r in sel[:12]:
            src[order[starts[r]:starts[r + 1]]] = val
        for r in sel[12:24]:
            src[order[starts[r]:starts[r + 1]].max()] = -val
    mid = np.nonzero(cnt >= 5)[0]
    rng.shuffle(mid)
    for k, r in enumerate(mid[:16]):
        toks = np.sort(order[starts[r]:starts[r + 1]])
        t = toks[len(toks) // 2]
        if k % 2:
            src[t, k % stride] = np.nan
        else:
            src[t] = -np.inf
    src[0] = np.inf
    return torch.from_numpy(src.reshape(-1)).to(dev()).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("origin", ORIGINS)
def test_non_finite_sources_propagate_like_the_fp64_scatter(origin, dtype):
    """+-Inf and NaN in source rows reach exactly the elements an fp64 (or atomicAdd) scatter puts them in: a row whose tokens are all
    +Inf sums to +Inf, not NaN, whatever padding the kernel's last batch of 4 entries needs; other rows stay finite."""
    rng = np.random.default_rng(ORIGINS.index(origin))
    widths = (3, 32, 96) if dtype == torch.float32 else (5, 64, 72)
    for mode in MODES:
        with reduce_mode(mode):
            lat, idx = build_origin(origin, hot_cloud(3, seed=2, n_hot=600), 0.5, 20000)
            rows, tokens = lat.m_hash_table.capacity(), idx.numel()
            w = torch.from_numpy(rng.uniform(0.25, 1.0, tokens).astype(np.float32)).to(dev())
            for v in widths:
                src = poison(idx, rows, tokens, v, dtype, rng)
                ref = reduce_reference(src, idx, w, rows, v, 1, v)
                assert bool(torch.isnan(ref[0]).any()) and bool(torch.isposinf(ref[0]).any()) and bool(torch.isneginf(ref[0]).any())
                assert int(torch.isfinite(ref[0]).all(1).sum()) > rows - 200
                for path in ("scatter", "fused"):
                    dst = torch.zeros((rows, v), dtype=torch.float32, device=dev())
                    if path == "scatter":
                        lat._scatter_rows(src.view(tokens, v), idx, w, dst, v, 1, v)
                    else:
                        lat._accumulate_and_prefetch(src.view(tokens, v), idx, w, dst, v, 1, tokens)
                    assert_reduce_close(dst, *ref, deterministic=mode == "deterministic", what=f"{origin}/{mode} v={v} {path}")


# ---------------------------------------------------------------------------------------------------------- source offsets past 2^31
@pytest.mark.parametrize("dtype,v", [(torch.float32, 8), (torch.float16, 64)], ids=["f32", "f16"])
def test_source_rows_beyond_2_pow_31_elements(dtype, v):
    """Integer rows read at element offsets up to 2^31 + 2^27 (src_div = 1, src_stride = 2^27): the offset must be computed in 64 bits.
    Only the rows that are read are written."""
    import lattice_net_amd as L
    stride, tokens = 2 ** 27, 18
    numel = (tokens - 1) * stride + v
    need = numel * torch.finfo(dtype).bits // 8
    free, _ = torch.cuda.mem_get_info(dev())
    if free < need + (2 << 30):
        pytest.skip(f"needs {need / 2 ** 30:.1f} GiB of free device memory")
    lat = L.Lattice(sigmas=[1.0] * 3, capacity=64, device=dev())
    lat.begin_splat()
    lat.just_create_verts(torch.zeros((1, 3), device=dev()), True)  # (a table: _scatter_rows caches its CSR there)
    idx = torch.arange(tokens, dtype=torch.int32, device=dev()) % 3
    w = torch.ones((tokens,), device=dev())
    src = torch.empty((numel,), dtype=dtype, device=dev())
    rows = torch.from_numpy(((np.arange(tokens)[:, None] * 37) % 251 - 125 + np.arange(v)[None, :]).astype(np.float32))
    for t in range(tokens):
        src[t * stride:t * stride + v] = rows[t].to(dev()).to(dtype)
    assert (tokens - 1) * stride >= 2 ** 31
    ref = torch.zeros((64, v), dtype=torch.float64)
    ref.index_add_(0, idx.cpu().long(), rows.double())
    dst = torch.zeros((64, v), dtype=torch.float32, device=dev())
    lat._scatter_rows(src, idx, w, dst, v, 1, stride)
    assert_exact(dst, ref, "offsets past 2^31")
    del src
    torch.cuda.empty_cache()
