"""Argument checks of the batched solve (_solve.solve_batch / eps_solve_batch) that fail before
any device work: they need the built library, not a GPU."""

import pytest

from epsilon_amd import _solve, problems, wire


@pytest.fixture(scope="module")
def lib_built():
    import os
    if not os.path.exists(_solve.LIB_PATH):
        pytest.fail("libepsilon_hip.so is not built")
    return _solve


def test_empty_batch_is_an_error(lib_built):
    sb = wire.SolverParams().SerializeToString()
    with pytest.raises(_solve.error, match="count is 0"):
        _solve.solve_batch([], None, sb, {})


def test_parameter_lists_must_match_problems(lib_built):
    prob, _ = problems.lasso(8, 20, seed=0)
    sb = wire.SolverParams().SerializeToString()
    with pytest.raises(_solve.error, match="2 problems but 1 parameter lists"):
        _solve.solve_batch([prob.SerializeToString()] * 2, [[]], sb, prob.expression_data())


def test_malformed_instance_is_named(lib_built):
    prob, _ = problems.lasso(8, 20, seed=0)
    pb = prob.SerializeToString()
    sb = wire.SolverParams().SerializeToString()
    with pytest.raises(_solve.error, match="instance 2"):
        _solve.solve_batch([pb, pb, b"\xff\xff\xff\xff"], None, sb, prob.expression_data())
    with pytest.raises(_solve.error, match="instance 0"):
        _solve.solve_batch([b"\x0a\xff"], None, sb, {})
