"""oracle_np.numpy_row_sum restates the order in which np.sum(a, axis=1) adds a C-contiguous row -- the sum whose zero test
decides find_argmax_nonzero_value (utils/indexing.py:9-32) and which k_argmax_nonzero reproduces.  Checked bit for bit
against numpy itself on rows that cancel, so a numpy that changed its order fails here, without a GPU."""
import numpy as np
import pytest

from oracle import oracle_np

WIDTHS = list(range(1, 301)) + [511, 512, 513, 1000]


def _cancelling_rows(rng, C, dtype):
    rows = [
        rng.integers(-3, 4, C) * 0.1,                                    # multiples of 0.1: sums near zero, either sign
        rng.normal(0, 1, C) * np.exp(rng.uniform(-20, 20)),
        np.full(C, -0.0),
    ]
    half = rng.normal(0, 1, (C + 1) // 2) * 10.0 ** rng.integers(-8, 9, (C + 1) // 2)
    pm = np.concatenate([half, -half])[:C]                               # x and -x, shuffled: exact zero left to right
    rows.append(pm[rng.permutation(C)])
    a = np.stack(rows).astype(dtype)
    if C >= 3:
        a = np.concatenate([a, np.array([[1e8, 1.0, -1e8] + [0.0] * (C - 3)], dtype=dtype)])
    return np.ascontiguousarray(a)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_numpy_row_sum_is_numpys_order_bit_for_bit(dtype):
    rng = np.random.default_rng(12)
    uint = np.uint64 if dtype == np.float64 else np.uint32
    disagree_left_to_right = 0
    for C in WIDTHS:
        a = _cancelling_rows(rng, C, dtype)
        want = np.sum(a, axis=1)
        got = np.array([oracle_np.numpy_row_sum(r, dtype) for r in a], dtype=dtype)
        assert want.dtype == dtype
        np.testing.assert_array_equal(got.view(uint), want.view(uint), err_msg=f"C={C} {np.dtype(dtype).name}")
        naive = np.cumsum(a, axis=1)[:, -1]  # left to right
        disagree_left_to_right += int(np.sum((naive == 0) != (want == 0)))
    # the rows are chosen so that the order matters: a left-to-right sum disagrees with numpy about zero on some of them
    assert disagree_left_to_right > 0


def test_the_issues_two_rows_sum_to_numpys_values():
    a = np.array([[0.2, 0.3, -0.1, -0.3, 0.3, -0.3, -0.3, 0.2], [-0.2, -0.1, -0.2, 0.3, 1.0, -0.3, -0.3, -0.2]])
    assert oracle_np.numpy_row_sum(a[0], np.float64) == 0.0 == np.sum(a, axis=1)[0]
    assert oracle_np.numpy_row_sum(a[1], np.float64) == np.sum(a, axis=1)[1] != 0.0
    f = np.array([[1e8, 1.0, -1e8]], dtype=np.float32)
    assert oracle_np.numpy_row_sum(f[0], np.float32) == np.sum(f, axis=1)[0] == 0.0
