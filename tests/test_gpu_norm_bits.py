"""The GroupNorm and BatchNorm kernels of csrc/ln_norm.hip against tests/golden/F15_norm_bits.npz, bit for bit (`pytest -m gpu`): every
output of every call path, forward and backward, as the commit before the kernels were rebuilt on shared device bodies computed it
(tests/golden/make_norm_bits_fixture.py holds the cases, their inputs and the calls).  No tolerance: a sum taken in another order or an
intermediate kept at another precision shows as a differing word."""
import hashlib

import numpy as np
import pytest

from tests import dense_reference as R
from tests.golden import make_norm_bits_fixture as M

pytestmark = pytest.mark.gpu

CASES = M.cases()


def test_the_cases_are_the_issues():
    """4, 32, 96 and 1024 channels over three statistics workgroups + 3 rows on every path; four ranges with an empty one and a single row."""
    for c in M.CHANNELS:
        for path in M.PATHS:
            _, _, m, live, starts = CASES[f"{path}_c{c}"]
            assert m == 3 * (256 // (c // 4)) * 16 + 3
            assert (live is not None and 0 < live < m) == path.endswith("_rows")
            if path == "gn_ranges":
                lengths = np.diff(starts)
                assert len(lengths) == 4 and 0 in lengths and 1 in lengths
    assert M.stats_grids(CASES["gn_relu_c32_full"]) == [R.LN_GN_REPLICAS]


@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_are_what_they_were(golden, name):
    fx = golden("F15_norm_bits")
    case = CASES[name]
    # the condition of the comparison: one add onto zero per accumulator replica, so the fp64 atomics leave no freedom of order
    grids = M.stats_grids(case)
    assert max(grids) <= R.LN_GN_REPLICAS, f"{name}: {grids} statistics workgroups per range, more than the accumulator replicas"
    got = M.run(name, case)
    want_keys = sorted(k.split("/", 1)[1].replace(".sha256", "") for k in fx if k.startswith(name + "/"))
    assert sorted(got) == want_keys, (name, sorted(got), want_keys)
    for key, arr in got.items():
        if f"{name}/{key}" in fx:
            want = fx[f"{name}/{key}"]
            assert want.dtype == np.uint32 and want.shape == arr.shape, (name, key, want.dtype, want.shape, arr.shape)
            R.assert_equal_bits(arr, want.view(np.float32), f"{name} {key}")
        else:
            assert arr.nbytes > M.ARRAY_BYTES
            assert hashlib.sha256(arr.tobytes()).hexdigest() == str(fx[f"{name}/{key}.sha256"]), f"{name} {key}: SHA-256 of the bytes differs"
