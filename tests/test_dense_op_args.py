"""The test entry of the dense mat-vec layer (include/epsilon_hip.h eps_test_dense_op): the
argument checks.  They fail before any device work: they need the built library, not a GPU."""

import os

import numpy as np
import pytest

from epsilon_amd import _solve


@pytest.fixture(scope="module")
def lib_built():
    if not os.path.exists(_solve.LIB_PATH):
        pytest.fail("libepsilon_hip.so is not built")
    return _solve


A = np.arange(15.0).reshape(5, 3)  # 5 x 3, passed column-major
X3, Y5 = np.ones(3), np.ones(5)


def gemv_n(**kw):
    args = dict(rows=5, cols=3, a=A.flatten(order="F"), x=X3, y=Y5)
    args.update(kw)
    return _solve.dense_op("gemv_n", **args)


@pytest.mark.parametrize("op", ["", "gemv", "GEMV_N", "symv_pack", "nrm2"])
def test_unknown_op(lib_built, op):
    with pytest.raises(_solve.error, match="eps_test_dense_op: op must be gemv_n, gemv_t, symv, symv_packed, "
                                           "reduce_partials, sumsq, sumsq_diff, dot, axpby or diag_mul, got %s$" % op):
        _solve.dense_op(op, rows=5, cols=3, a=A, x=X3, y=Y5)


def test_null_op(lib_built):
    with pytest.raises(_solve.error, match="eps_test_dense_op: op is null"):
        _solve.dense_op(None, rows=5, cols=3, a=A, x=X3, y=Y5)


@pytest.mark.parametrize("missing", ["a", "x", "y"])
def test_null_operand_gemv(lib_built, missing):
    with pytest.raises(_solve.error, match="eps_test_dense_op: %s is null" % missing):
        gemv_n(**{missing: None})


def test_null_operands_of_the_other_ops(lib_built):
    with pytest.raises(_solve.error, match="eps_test_dense_op: a is null"):
        _solve.dense_op("symv", rows=3, x=X3, y=X3)
    with pytest.raises(_solve.error, match="eps_test_dense_op: add is null"):
        _solve.dense_op("reduce_partials", rows=5, nparts=3, a=A, y=Y5, with_add=True)
    with pytest.raises(_solve.error, match="eps_test_dense_op: x is null"):
        _solve.dense_op("sumsq", rows=5)
    with pytest.raises(_solve.error, match="eps_test_dense_op: y is null"):
        _solve.dense_op("dot", rows=5, x=Y5)
    with pytest.raises(_solve.error, match="eps_test_dense_op: x is null"):
        _solve.dense_op("axpby", rows=5, y=Y5)
    with pytest.raises(_solve.error, match="eps_test_dense_op: a is null"):
        _solve.dense_op("diag_mul", rows=5, x=Y5, y=Y5)


@pytest.mark.parametrize("op", ["gemv_n", "gemv_t", "symv", "symv_packed"])
def test_lda_below_rows(lib_built, op):
    with pytest.raises(_solve.error, match="eps_test_dense_op: lda 4 < rows 5"):
        _solve.dense_op(op, rows=5, cols=3, lda=4, a=A, x=X3, y=Y5)


def test_operand_lengths(lib_built):
    with pytest.raises(_solve.error, match="a has 15 entries, the dimensions need 17"):
        gemv_n(lda=6)  # (cols - 1) * lda + rows
    with pytest.raises(_solve.error, match="x has 5 entries, the dimensions need 3"):
        gemv_n(x=Y5)
    with pytest.raises(_solve.error, match="y has 3 entries, the dimensions need 5"):
        gemv_n(y=X3)
    with pytest.raises(_solve.error, match="x has 3 entries, the dimensions need 5"):
        _solve.dense_op("gemv_t", rows=5, cols=3, a=A, x=X3, y=X3)
    with pytest.raises(_solve.error, match="y has 5 entries, the dimensions need 3"):
        _solve.dense_op("gemv_t", rows=5, cols=3, a=A, x=Y5, y=Y5)
    with pytest.raises(_solve.error, match="a has 15 entries, the dimensions need 9"):
        _solve.dense_op("symv", rows=3, a=A, x=X3, y=X3)
    with pytest.raises(_solve.error, match="a has 9 entries, the dimensions need 11"):
        _solve.dense_op("symv_packed", rows=3, lda=4, a=np.ones(9), x=X3, y=X3)
    with pytest.raises(_solve.error, match="a has 15 entries, the dimensions need 20"):
        _solve.dense_op("reduce_partials", rows=5, nparts=4, a=A, y=Y5)
    with pytest.raises(_solve.error, match="add has 3 entries, the dimensions need 5"):
        _solve.dense_op("reduce_partials", rows=5, nparts=3, a=A, y=Y5, add=X3)
    with pytest.raises(_solve.error, match="x has 3 entries, the dimensions need 5"):
        _solve.dense_op("sumsq", rows=5, x=X3)
    with pytest.raises(_solve.error, match="y has 3 entries, the dimensions need 5"):
        _solve.dense_op("sumsq_diff", rows=5, x=Y5, y=X3)
    with pytest.raises(_solve.error, match="x has 3 entries, the dimensions need 5"):
        _solve.dense_op("axpby", rows=5, x=X3, y=Y5)
    with pytest.raises(_solve.error, match="a has 3 entries, the dimensions need 5"):
        _solve.dense_op("diag_mul", rows=5, a=X3, x=Y5, y=Y5)


def test_negative_sizes(lib_built):
    with pytest.raises(_solve.error, match="eps_test_dense_op: rows is negative: -5"):
        gemv_n(rows=-5)
    with pytest.raises(_solve.error, match="eps_test_dense_op: cols is negative: -3"):
        gemv_n(cols=-3)
    with pytest.raises(_solve.error, match="eps_test_dense_op: rows is negative: -1"):
        _solve.dense_op("dot", rows=-1, x=Y5, y=Y5)
    for name in ("a", "x", "y", "add"):
        with pytest.raises(_solve.error, match="eps_test_dense_op: %s_off is negative: -1" % name):
            gemv_n(**{name + "_off": -1})


@pytest.mark.parametrize("nparts", [0, -1])
def test_nparts_below_one(lib_built, nparts):
    with pytest.raises(_solve.error, match="eps_test_dense_op: nparts must be at least 1, got %d" % nparts):
        _solve.dense_op("reduce_partials", rows=5, nparts=nparts, a=np.zeros(0), y=Y5)


def test_every_check_comes_before_device_work(lib_built):
    """With arguments that pass, the call goes on to the device: without one it fails there (no
    fallback), with one it answers."""
    if _solve.device_count() > 0:
        out = gemv_n()
        G = _solve.DENSE_OP_GUARD
        assert np.array_equal(out[G:-G], A.sum(axis=1))
        assert np.all(out[:G] == _solve.DENSE_OP_SENTINEL) and np.all(out[-G:] == _solve.DENSE_OP_SENTINEL)
    else:
        for op, kw in [("gemv_n", dict(rows=5, cols=3, a=A, x=X3, y=Y5)),
                       ("symv_packed", dict(rows=3, a=np.eye(3), x=X3, y=X3)),
                       ("reduce_partials", dict(rows=5, nparts=3, a=A, y=Y5, add=Y5)),
                       ("dot", dict(rows=5, x=Y5, y=Y5)), ("axpby", dict(rows=5, y=Y5, alias_xy=True)),
                       ("diag_mul", dict(rows=5, a=Y5, x=Y5, y=Y5))]:
            with pytest.raises(_solve.error, match="no HIP device"):
                _solve.dense_op(op, **kw)
