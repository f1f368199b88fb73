"""The test entry of the block LDL^T (include/epsilon_hip.h eps_test_block_solve): the argument
checks.  They fail before any device work: they need the built library, not a GPU."""

import os

import numpy as np
import pytest

from epsilon_amd import _solve, ir


@pytest.fixture(scope="module")
def lib_built():
    if not os.path.exists(_solve.LIB_PATH):
        pytest.fail("libepsilon_hip.so is not built")
    return _solve


B = np.arange(10.0).reshape(5, 2)


def blocks():
    """[[I_5, B], [B^T, I_2]] on the keys "one" and "two" """
    return [("one", "one", ir.identity(5)), ("one", "two", ir.dense_matrix(B)),
            ("two", "one", ir.transpose(ir.dense_matrix(B))), ("two", "two", ir.identity(2))]


@pytest.mark.parametrize("given", [None, []])
def test_null_or_empty_block_list(lib_built, given):
    with pytest.raises(_solve.error, match="eps_test_block_solve: blocks is null or empty"):
        _solve.block_solve(given, {"one": np.ones(5)})


@pytest.mark.parametrize("mode", ["fill", "factor", "solve"])
def test_rhs_key_the_matrix_lacks(lib_built, mode):
    with pytest.raises(_solve.error, match="rhs key three is not a key of the matrix"):
        _solve.block_solve(blocks(), {"one": np.ones(5), "three": np.ones(2)}, mode=mode)


def test_rhs_key_the_substitution_order_lacks(lib_built):
    L = [("two", "one", ir.dense_matrix(B.T))]
    with pytest.raises(_solve.error, match="rhs key three is not in keys"):
        _solve.block_solve(L, {"three": np.ones(2)}, mode="forward", keys=["one", "two"])
    with pytest.raises(_solve.error, match="block key one is not in keys"):
        _solve.block_solve(L, {"two": np.ones(2)}, mode="back", keys=["two"])
    with pytest.raises(_solve.error, match="mode forward needs the key order in keys"):
        _solve.block_solve(L, {"two": np.ones(2)}, mode="forward")


def test_rhs_of_another_length(lib_built):
    with pytest.raises(_solve.error, match="rhs two has 5 entries, the matrix 2"):
        _solve.block_solve(blocks(), {"two": np.ones(5)})


def test_pair_given_twice(lib_built):
    twice = blocks() + [("one", "two", ir.dense_matrix(B))]
    with pytest.raises(_solve.error, match=r"block \(one, two\) is given twice"):
        _solve.block_solve(twice, {"one": np.ones(5)})


@pytest.mark.parametrize("mode", ["", "Factor", "cholesky"])
def test_unknown_mode(lib_built, mode):
    with pytest.raises(_solve.error, match="mode must be fill, factor, solve, forward or back, got %s" % mode):
        _solve.block_solve(blocks(), {"one": np.ones(5)}, mode=mode)


def test_truncated_linear_map_payload(lib_built):
    given = blocks()
    payload = given[1][2].proto.SerializeToString()
    given[1] = ("one", "two", payload[:-1])  # cuts the nested Constant short
    with pytest.raises(_solve.error, match=r"block \(one, two\): malformed LinearMap: .*truncated"):
        _solve.block_solve(given, {"one": np.ones(5)})
    given[1] = ("one", "two", b"")
    with pytest.raises(_solve.error, match=r"block \(one, two\) has an empty LinearMap payload"):
        _solve.block_solve(given, {"one": np.ones(5)})


def test_blocks_that_do_not_fit(lib_built):
    given = blocks()[:2] + blocks()[3:]  # (two, one) left out
    with pytest.raises(_solve.error, match=r"block \(one, two\) has no transpose \(two, one\)"):
        _solve.block_solve(given)
    given = blocks()
    given[3] = ("two", "two", ir.identity(3))
    with pytest.raises(_solve.error, match="block 3 gives key two the size 3, an earlier block 2"):
        _solve.block_solve(given)


def test_every_check_comes_before_device_work(lib_built):
    """With arguments that pass, the call goes on to the device: without one it fails there (no
    fallback), with one it answers."""
    if _solve.device_count() > 0:
        assert _solve.block_solve(blocks(), mode="fill")["fill"] == {"one": 4, "two": 25}
    else:
        with pytest.raises(_solve.error, match="no HIP device"):
            _solve.block_solve(blocks(), mode="fill")
