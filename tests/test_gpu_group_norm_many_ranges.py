"""GroupNorm over 65 ... 1024 row ranges (csrc/ln_norm.hip: k_gn_forward_range_owner, k_gn_backward_range_owner, one workgroup per range)
against fp64, through ln_group_norm_forward_many_segments / _backward_many_segments (`pytest -m gpu`).

The reference and the bounds are those of tests/test_gpu_group_norm_segments.py: dense_reference's GroupNorm reference on the rows of each
range alone (the owner blocks a range from its own first row in the slabs of the other forms, so the fp32 roundings are the same),
grad_gamma / grad_beta within the sum of the ranges' bounds.  The calls go through the C ABI on buffers with sentinels behind every
output.  Each test prints its worst error / bound ratios (`pytest -s`); nothing is asserted on those figures.  A library without
the range-owner form has none of these entry points: every case fails."""
import numpy as np
import pytest
import torch

from tests import cloud_batch_reference as B
from tests import dense_reference as R
from tests import test_gpu_group_norm_segments as S

pytestmark = pytest.mark.gpu

SENTINEL = 777.0
LENGTHS = (0, 1, 2, 3, 9, 40)
PAD = 7  # garbage rows behind the last range: zeros in y and grad_x


def starts_of(count, seed):
    """`count` ranges with lengths drawn from LENGTHS; range 0, the last range and two neighbours in the middle are empty."""
    sizes = np.random.default_rng(seed).choice(LENGTHS, size=count)
    sizes[[0, count // 2, count // 2 + 1, count - 1]] = 0
    sizes[[1, count - 2]] = (40, 1)  # (and the first and the last range that hold rows are not all alike)
    return [0] + [int(v) for v in np.cumsum(sizes)]


def buf(n, fill=SENTINEL, dtype=torch.float32):
    return torch.full((n + 64,), fill, dtype=dtype, device=S.dev())


class Call:
    """The buffers of one forward + backward pair through the C ABI, allocated once (a stream capture replays `launch`)."""

    def __init__(self, x_np, gy_np, gamma, beta, row_starts, groups, relu, eps=1e-5, rows=None, use_next=False):
        from lattice_net_amd import _lib
        self.lib, self._lib = _lib.load(), _lib
        self.m, self.c = x_np.shape
        self.groups, self.relu, self.eps, self.segs = groups, int(relu), eps, len(row_starts) - 1
        self.x, self.gy = S.gpu(x_np), S.gpu(gy_np)
        self.w = None if gamma is None else S.gpu(gamma)
        self.b = None if beta is None else S.gpu(beta)
        self.starts = S.starts_dev(row_starts)
        self.rows = None if rows is None else torch.tensor([rows], dtype=torch.int32, device=S.dev())
        m, c, segs = self.m, self.c, self.segs
        self.sizes = {"y": m * c, "grad_x": m * c, "mean_rstd": segs * 2 * groups, "scale_shift": segs * 2 * c, "grad_gamma": c, "grad_beta": c}
        self.out = {k: buf(n) for k, n in self.sizes.items()}
        self.nbytes = int(self.lib.ln_group_norm_segments_workspace_bytes(c, segs))
        self.ws = buf(self.nbytes // 8, 5.0, torch.float64)  # (dirty: this form accumulates into nothing)
        self.next_count = 3000 if use_next else 0  # doubles of the next call's accumulators to zero on the way out
        self.next = buf(self.next_count, 5.0, torch.float64) if use_next else None

    def launch(self):
        p, o, lib = self._lib.ptr, self.out, self.lib
        stream = self._lib.stream_ptr(S.dev())
        nxt = (p(self.next), self.next_count * 8) if self.next is not None else (None, 0)
        self._lib.check(lib.ln_group_norm_forward_many_segments(p(self.x), p(self.w), p(self.b), self.m, self.c, self.groups, self.eps, self.relu, p(o["y"]),
                                                           p(o["mean_rstd"]), p(o["scale_shift"]), p(self.ws), self.nbytes, *nxt, p(self.rows),
                                                           p(self.starts), self.segs, stream), "forward")
        self._lib.check(lib.ln_group_norm_backward_many_segments(p(self.x), p(self.gy), p(self.w), p(o["mean_rstd"]), p(o["scale_shift"]), self.m, self.c,
                                                            self.groups, self.relu, p(o["grad_x"]), p(o["grad_gamma"]), p(o["grad_beta"]), p(self.ws),
                                                            self.nbytes, *nxt, p(self.rows), p(self.starts), self.segs, stream), "backward")

    def results(self, what=""):
        """Every output as NumPy, after the sentinel checks."""
        torch.cuda.synchronize()
        for name, n in self.sizes.items():
            assert bool((self.out[name][n:] == SENTINEL).all()), f"{what}: a sentinel behind {name} was overwritten"
        assert bool((self.ws[self.nbytes // 8:] == 5.0).all()), f"{what}: the workspace was written behind its size"
        if self.next is not None:
            assert not bool(self.next[:self.next_count].any()), f"{what}: the next call's accumulators are not zero"
            assert bool((self.next[self.next_count:] == 5.0).all()), f"{what}: the next workspace was written behind its size"
        m, c, segs = self.m, self.c, self.segs
        shapes = {"y": (m, c), "grad_x": (m, c), "mean_rstd": (segs, -1), "scale_shift": (segs, -1), "grad_gamma": (c,), "grad_beta": (c,)}
        return {k: self.out[k][:self.sizes[k]].view(*shapes[k]).cpu().numpy().copy() for k in self.sizes}


def run(x, gy, gamma, beta, row_starts, groups, relu, **kw):
    call = Call(x, gy, gamma, beta, row_starts, groups, relu, **kw)
    call.launch()
    return call.results(), call


def check(x, gy, row_starts, groups, relu, affine=True, rows=None, use_next=False, what="", seed=0):
    """One call against the fp64 reference of every range; the statistics rows of empty ranges keep their sentinels."""
    m, c = x.shape
    gamma, beta = R.gn_params(c, affine, seed)
    got, call = run(x, gy, gamma, beta, row_starts, groups, relu, rows=rows, use_next=use_next)
    segs, live = B.segments(row_starts, m, rows)
    for s, (lo, hi) in enumerate(segs):
        if hi == lo:
            assert (got["mean_rstd"][s] == SENTINEL).all() and (got["scale_shift"][s] == SENTINEL).all(), f"{what}: empty range {s} wrote statistics"
    ratios = B.check_forward(x, got["y"], got["mean_rstd"], got["scale_shift"], gamma, beta, groups, 1e-5, relu, row_starts, rows, what)
    ref, bound = B.backward_reference(x, gy, got["y"], got["mean_rstd"], gamma, groups, relu, row_starts, rows)
    assert not got["grad_x"][live:].any(), f"{what}: grad_x is not zero behind row {live}"
    for name, r_, b_ in zip(("grad_x", "grad_gamma", "grad_beta"), ref, bound):
        if not affine and name != "grad_x":
            continue  # (no parameters: the sibling test holds no gradient of them either)
        R.assert_within(got[name], r_, b_, f"{what} {name}")
        ratios[name] = R.worst_ratio(got[name], r_, b_)
    return ratios, got


CASES = [(65, 4), (65, 32), (65, 64), (65, 1024), (200, 4), (200, 32), (200, 64), (1024, 4), (1024, 32), (1024, 64)]


@pytest.mark.parametrize("count,c", CASES)
def test_many_ranges_random(count, c):
    """Groups of 32 (the module's rule where 32 does not divide C) with ReLU and the alternating workspaces, groups of C / 2 without
    either and without affine parameters."""
    starts = starts_of(count, count + c)
    x, gy = S.inputs(starts[-1] + PAD, c, 3 * c + count, starts)
    worst = {}
    for groups, relu, affine, use_next in ((B.module_groups(c), True, True, True), (c // 2, False, False, False)):
        r, _ = check(x, gy, starts, groups, relu, affine, use_next=use_next, what=f"{count} ranges c={c} groups={groups} relu={relu}", seed=c)
        worst.update({k: max(v, worst.get(k, 0.0)) for k, v in r.items()})
    print(f"GroupNorm {count} ranges c={c}: worst error / bound {worst}")


@pytest.mark.parametrize("c", [4, 64, 1024])
def test_the_other_switch_settings(c):
    """ReLU without next_workspace, and no ReLU with it, at 65 ranges."""
    starts = starts_of(65, c)
    x, gy = S.inputs(starts[-1] + PAD, c, c, starts)
    for relu, use_next in ((True, False), (False, True)):
        check(x, gy, starts, B.module_groups(c), relu, use_next=use_next, what=f"c={c} relu={relu} next={use_next}", seed=1)


@pytest.mark.parametrize("c", [64, 1024])
def test_one_long_range_among_64_short_ones(c):
    """A range of 3 000 rows: the owner's loop takes 12 slabs of 256 rows at 64 channels, 188 of 16 rows at 1024."""
    sizes = [int(v) for v in np.random.default_rng(c).choice(LENGTHS[1:], size=64)]
    sizes.insert(31, 3000)
    starts = [0] + [int(v) for v in np.cumsum(sizes)]
    x, gy = S.inputs(starts[-1] + PAD, c, 11, starts)
    r, _ = check(x, gy, starts, B.module_groups(c), True, what=f"long range c={c}", seed=2)
    print(f"GroupNorm 64 short ranges and one of 3000 rows c={c}: worst error / bound {r}")


@pytest.mark.parametrize("c", [32, 64])
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
def test_many_ranges_exact(c, relu, monkeypatch):
    """Integer inputs through group_norm_rows(..., many_ranges=True): statistics, y and the parameter gradients bit for bit (the sibling
    test's check, whose runner imports group_norm_rows at every call)."""
    import functools
    from lattice_net_amd import lattice_blocks
    monkeypatch.setattr(lattice_blocks, "group_norm_rows", functools.partial(lattice_blocks.group_norm_rows, many_ranges=True))
    starts = starts_of(200, 7)
    S.check_exact(c, relu, starts, starts[-1] + PAD, what=f"200 ranges exact c={c} relu={relu}")


@pytest.mark.parametrize("rows", ["below_last_start", -5])
def test_under_a_device_row_count(rows):
    """*rows_dev below the start of the last range that holds rows: the ranges end there; a negative count is no row at all."""
    c = 64
    starts = starts_of(130, 4)
    if rows == "below_last_start":
        rows = starts[-3] - 1  # (ranges -1 is empty, -2 holds one row: inside the range in front of it)
    height = starts[-1] + PAD
    x, gy = S.inputs(height, c, 9, starts)
    live = max(min(rows, starts[-1]), 0)
    x[live:] = 3e30 * np.where(np.arange(c) % 2, -1, 1)
    gy[live:] = -1e30
    r, got = check(x, gy, starts, 32, True, rows=rows, what=f"rows_dev={rows}", seed=5)
    for name in ("y", "grad_x", "grad_gamma", "grad_beta"):
        assert np.isfinite(got[name]).all(), f"rows_dev={rows}: {name} is not finite"
    if rows < 0:
        assert not got["y"].any() and not got["grad_x"].any() and not got["grad_gamma"].any() and not got["grad_beta"].any()
    print(f"GroupNorm 130 ranges rows_dev={rows}: worst error / bound {r}")


@pytest.mark.parametrize("c", [32, 1024])
def test_one_range_cannot_move_the_others(c):
    """The rows of one range multiplied by 1000 and moved by 3000 standard deviations: every output of every other range keeps its bits."""
    starts = starts_of(65 if c == 1024 else 200, 12)
    x, gy = S.inputs(starts[-1] + PAD, c, 21, starts)
    groups = B.module_groups(c)
    gamma, beta = R.gn_params(c, True, 2)
    base, _ = run(x, gy, gamma, beta, starts, groups, True)
    segs, _ = B.segments(starts, x.shape[0])
    for victim in (1, next(s for s in range(len(segs) // 3, len(segs)) if segs[s][1] > segs[s][0])):
        lo, hi = segs[victim]
        x2 = x.copy()
        x2[lo:hi] = x2[lo:hi] * np.float32(1000.0) + np.float32(3000.0 * x[lo:hi].std() * 1000.0)
        got, _ = run(x2, gy, gamma, beta, starts, groups, True)
        keep = np.ones(x.shape[0], bool)
        keep[lo:hi] = False
        for name in ("y", "grad_x"):
            R.assert_equal_bits(got[name][keep], base[name][keep], f"victim {victim}: {name} of the other ranges")
        others = [s for s in range(len(segs)) if s != victim]
        for name in ("mean_rstd", "scale_shift"):
            R.assert_equal_bits(got[name][others], base[name][others], f"victim {victim}: {name} of the other ranges")
        assert not np.array_equal(got["mean_rstd"][victim], base["mean_rstd"][victim])


def test_runs_and_graph_replays_agree_bit_for_bit():
    """Two eager runs and two replays of a captured forward + backward pair: every output has the same bits (fixed summation order)."""
    c, groups = 64, 32
    starts = starts_of(1024, 3)
    x, gy = S.inputs(starts[-1] + PAD, c, 17, starts)
    gamma, beta = R.gn_params(c, True, 6)
    first, _ = run(x, gy, gamma, beta, starts, groups, True)
    second, _ = run(x, gy, gamma, beta, starts, groups, True)
    for k in first:
        R.assert_equal_bits(second[k], first[k], f"second run: {k}")
    call = Call(x, gy, gamma, beta, starts, groups, True)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call.launch()  # (warm-up on the capture stream)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            call.launch()
    for replay in range(2):
        for t in call.out.values():
            t.fill_(SENTINEL)
        graph.replay()
        got = call.results(f"replay {replay}")
        for k in first:
            R.assert_equal_bits(got[k], first[k], f"replay {replay}: {k}")


def test_group_norm_rows_takes_more_than_64_ranges_only_when_asked():
    from lattice_net_amd.lattice_blocks import group_norm_rows
    gn = torch.nn.GroupNorm(4, 8).to(S.dev())
    x = torch.zeros((10, 8), device=S.dev())
    with pytest.raises(ValueError, match="B <= 64"):
        group_norm_rows(x, gn, False, None, S.starts_dev(range(67)))
    with pytest.raises(ValueError, match="B <= 1024"):
        group_norm_rows(x, gn, False, None, S.starts_dev(range(1026)), many_ranges=True)
    y = group_norm_rows(x, gn, False, None, S.starts_dev(range(67)), many_ranges=True)  # 66 ranges, the ones behind row 10 empty
    assert tuple(y.shape) == (10, 8) and bool(torch.isfinite(y).all())
