"""CPU tests of the checker itself: tests/szh_ref.py's independent Huffman cost, which the GPU tests hold the device's code books to."""
import numpy as np
import pytest

import szh_ref


def test_huffman_cost_of_known_distributions():
    assert szh_ref.huffman_cost([1, 1, 2, 4]) == (14, 3)        # code lengths 3, 3, 2, 1
    assert szh_ref.huffman_cost([0, 5, 0, 5, 0]) == (10, 1)     # empty bins take no part
    assert szh_ref.huffman_cost([7]) == (0, 0)                  # one symbol: no bits
    assert szh_ref.huffman_cost([1, 1, 1, 1]) == (8, 2)
    fib = [1, 1, 2, 3, 5, 8, 13, 21]                             # Fibonacci counts: the deepest tree, 7 levels for 8 symbols
    cost, height = szh_ref.huffman_cost(fib)
    assert height == 7 and cost == sum(f * l for f, l in zip(fib, [7, 7, 6, 5, 4, 3, 2, 1]))


def test_assert_book_optimal_accepts_the_optimum_and_rejects_a_worse_book():
    freq = np.array([1, 1, 2, 4])
    szh_ref.assert_book_optimal(freq, np.array([3, 3, 2, 1], np.uint8), 16)
    with pytest.raises(AssertionError):
        szh_ref.assert_book_optimal(freq, np.array([2, 2, 2, 2], np.uint8), 16)
    # beyond the length limit: within 0.2 % of the unlimited code passes, more does not
    fib = np.array([1, 1, 2, 3, 5, 8, 13, 21] + [10 ** 6] * 2)
    cost, height = szh_ref.huffman_cost(fib)
    lens = np.array([9, 9, 8, 7, 6, 5, 4, 3, 1, 2])  # (the unlimited code; the limit below makes it "length-limited")
    assert int((fib * lens).sum()) == cost and height == 9
    szh_ref.assert_book_optimal(fib, lens, 8)
    with pytest.raises(AssertionError):
        szh_ref.assert_book_optimal(fib, np.array([9, 9, 8, 7, 6, 5, 4, 3, 2, 2]) + 1, 8)
