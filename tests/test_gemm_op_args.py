"""The test entry of the dense mat-mat layer (include/epsilon_hip.h eps_test_gemm_op): the argument
checks.  They fail before any device work: they need the built library, not a GPU."""

import os

import numpy as np
import pytest

from epsilon_amd import _solve


@pytest.fixture(scope="module")
def lib_built():
    if not os.path.exists(_solve.LIB_PATH):
        pytest.fail("libepsilon_hip.so is not built")
    return _solve


A = np.arange(15.0).reshape(5, 3)   # 5 x 3, passed column-major
B = np.arange(12.0).reshape(3, 4)   # 3 x 4
C = np.zeros((5, 4))
OPS = "gemm, gemm_batched, mat_copy, add_diag, symmetrize, col_abs_sums or kron"


def gemm(op="gemm", **kw):
    args = dict(M=5, N=4, K=3, a=A.flatten(order="F"), b=B.flatten(order="F"), c=C.flatten(order="F"))
    args.update(kw)
    return _solve.gemm_op(op, **args)


@pytest.mark.parametrize("op", ["", "GEMM", "gemv_n", "syrk", "matcopy"])
def test_unknown_op(lib_built, op):
    with pytest.raises(_solve.error, match="eps_test_gemm_op: op must be %s, got %s$" % (OPS, op)):
        gemm(op)


def test_null_op(lib_built):
    with pytest.raises(_solve.error, match="eps_test_gemm_op: op is null"):
        gemm(None)


@pytest.mark.parametrize("op", ["gemm", "gemm_batched"])
@pytest.mark.parametrize("missing", ["a", "b", "c"])
def test_null_operand_gemm(lib_built, op, missing):
    with pytest.raises(_solve.error, match="eps_test_gemm_op: %s is null" % missing):
        gemm(op, **{missing: None})


def test_null_operands_of_the_helpers(lib_built):
    with pytest.raises(_solve.error, match="eps_test_gemm_op: a is null"):
        _solve.gemm_op("mat_copy", M=5, N=3, c=np.zeros(15))
    with pytest.raises(_solve.error, match="eps_test_gemm_op: c is null"):
        _solve.gemm_op("mat_copy", M=5, N=3, a=A)
    with pytest.raises(_solve.error, match="eps_test_gemm_op: c is null"):
        _solve.gemm_op("add_diag", M=3)
    with pytest.raises(_solve.error, match="eps_test_gemm_op: c is null"):
        _solve.gemm_op("symmetrize", M=3)
    with pytest.raises(_solve.error, match="eps_test_gemm_op: a is null"):
        _solve.gemm_op("col_abs_sums", M=5, N=3)
    with pytest.raises(_solve.error, match="eps_test_gemm_op: b is null"):
        _solve.gemm_op("kron", M=5, N=3, K=3, batch=4, a=A, c=np.zeros(180))


@pytest.mark.parametrize("name", ["M", "N", "K"])
def test_negative_sizes(lib_built, name):
    with pytest.raises(_solve.error, match="eps_test_gemm_op: %s is negative: -2" % name):
        gemm(**{name: -2})


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_negative_offsets(lib_built, name):
    with pytest.raises(_solve.error, match="eps_test_gemm_op: %s_off is negative: -1" % name):
        gemm(**{name + "_off": -1})


def test_leading_dimension_below_the_rows_it_holds(lib_built):
    with pytest.raises(_solve.error, match="eps_test_gemm_op: lda 4 < rows 5"):
        gemm(lda=4)
    with pytest.raises(_solve.error, match="eps_test_gemm_op: lda 2 < rows 3"):
        gemm(trans_a=True, lda=2)   # a transposed A is stored K x M
    with pytest.raises(_solve.error, match="eps_test_gemm_op: ldb 2 < rows 3"):
        gemm(ldb=2)
    with pytest.raises(_solve.error, match="eps_test_gemm_op: ldb 3 < rows 4"):
        gemm(trans_b=True, ldb=3)   # a transposed B is stored N x K
    with pytest.raises(_solve.error, match="eps_test_gemm_op: ldc 4 < rows 5"):
        gemm(ldc=4)
    with pytest.raises(_solve.error, match="eps_test_gemm_op: lda 2 < rows 3"):
        _solve.gemm_op("mat_copy", M=5, N=3, trans_a=True, lda=2, a=A, c=np.zeros(15))
    with pytest.raises(_solve.error, match="eps_test_gemm_op: ldc 2 < rows 3"):
        _solve.gemm_op("add_diag", M=3, ldc=2, c=np.zeros(9))
    with pytest.raises(_solve.error, match="eps_test_gemm_op: ldc 2 < rows 3"):
        _solve.gemm_op("symmetrize", M=3, ldc=2, c=np.zeros(9))
    with pytest.raises(_solve.error, match="eps_test_gemm_op: lda 4 < rows 5"):
        _solve.gemm_op("col_abs_sums", M=5, N=3, lda=4, a=A)


def test_operand_lengths(lib_built):
    with pytest.raises(_solve.error, match="a has 15 entries, the dimensions need 17"):
        gemm(lda=6)  # (cols - 1) * lda + rows
    with pytest.raises(_solve.error, match="a has 15 entries, the dimensions need 19"):
        gemm(trans_a=True, lda=4)  # stored 3 x 5: 4 * 4 + 3
    with pytest.raises(_solve.error, match="b has 12 entries, the dimensions need 15"):
        gemm(ldb=4)
    with pytest.raises(_solve.error, match="c has 20 entries, the dimensions need 23"):
        gemm(ldc=6)
    with pytest.raises(_solve.error, match="b has 15 entries, the dimensions need 12"):
        gemm(b=A)
    with pytest.raises(_solve.error, match="a has 15 entries, the dimensions need 0"):
        gemm(K=0)    # an empty contraction reads nothing of A
    with pytest.raises(_solve.error, match="a has 15 entries, the dimensions need 12"):
        _solve.gemm_op("mat_copy", M=4, N=3, a=A, c=np.zeros(12))
    with pytest.raises(_solve.error, match="c has 12 entries, the dimensions need 15"):
        _solve.gemm_op("mat_copy", M=5, N=3, a=A, c=np.zeros(12))
    with pytest.raises(_solve.error, match="c has 9 entries, the dimensions need 11"):
        _solve.gemm_op("add_diag", M=3, ldc=4, c=np.zeros(9))
    with pytest.raises(_solve.error, match="d has 5 entries, the dimensions need 3"):
        _solve.gemm_op("add_diag", M=3, c=np.zeros(9), d=np.ones(5))
    with pytest.raises(_solve.error, match="c has 9 entries, the dimensions need 11"):
        _solve.gemm_op("symmetrize", M=3, ldc=4, c=np.zeros(9))
    with pytest.raises(_solve.error, match="a has 15 entries, the dimensions need 17"):
        _solve.gemm_op("col_abs_sums", M=5, N=3, lda=6, a=A)
    with pytest.raises(_solve.error, match="c has 179 entries, the dimensions need 180"):
        _solve.gemm_op("kron", M=5, N=3, K=3, batch=4, a=A, b=B, c=np.zeros(179))


def test_batch_lengths_follow_the_strides(lib_built):
    ok = dict(batch=3, outer=2, sA=16, sB=12, sC=24, sA2=50, sB2=40)  # 2 * 16 + 50 + 15, 2 * 12 + 40 + 12, 5 * 24 + 20
    a, b, c = np.zeros(97), np.zeros(76), np.zeros(140)
    with pytest.raises(_solve.error, match="a has 96 entries, the dimensions need 97"):
        gemm("gemm_batched", a=a[:96], b=b, c=c, **ok)
    with pytest.raises(_solve.error, match="b has 75 entries, the dimensions need 76"):
        gemm("gemm_batched", a=a, b=b[:75], c=c, **ok)
    with pytest.raises(_solve.error, match="c has 139 entries, the dimensions need 140"):
        gemm("gemm_batched", a=a, b=b, c=c[:139], **ok)
    with pytest.raises(_solve.error, match="a has 97 entries, the dimensions need 65"):
        gemm("gemm_batched", a=a, b=b, c=c, **dict(ok, sA=0))   # a shared operand: (outer - 1) sA2 + 15
    with pytest.raises(_solve.error, match="sC 19 < the 20 entries of one result: the results overlap"):
        gemm("gemm_batched", a=a, b=b, c=c, **dict(ok, sC=19))
    for name in ("sA", "sB", "sC", "sA2", "sB2"):
        with pytest.raises(_solve.error, match="eps_test_gemm_op: %s must be 0..2\\^40, got -4" % name):
            gemm("gemm_batched", a=a, b=b, c=c, **dict(ok, **{name: -4}))
    for name in ("batch", "outer"):
        with pytest.raises(_solve.error, match="eps_test_gemm_op: %s must be 1..255, got 0" % name):
            gemm("gemm_batched", a=a, b=b, c=c, **dict(ok, **{name: 0}))


@pytest.mark.parametrize("op", ["gemm", "gemm_batched"])
def test_lower_only_needs_a_square_result(lib_built, op):
    with pytest.raises(_solve.error, match="eps_test_gemm_op: lower_only needs M == N, got 5 x 4"):
        gemm(op, lower_only=True)


def test_every_check_comes_before_device_work(lib_built):
    """With arguments that pass, the call goes on to the device: without one it fails there (no
    fallback), with one it answers."""
    if _solve.device_count() > 0:
        out, route = gemm()
        G = _solve.DENSE_OP_GUARD
        assert np.array_equal(out[G:-G].reshape((5, 4), order="F"), A.dot(B)) and route == "small"
        assert np.all(out[:G] == _solve.DENSE_OP_SENTINEL) and np.all(out[-G:] == _solve.DENSE_OP_SENTINEL)
    else:
        for op, kw in [("gemm", dict(M=5, N=4, K=3, a=A, b=B, c=C)),
                       ("gemm_batched", dict(M=5, N=4, K=3, a=A, b=B, c=C, batch=1, outer=1)),
                       ("mat_copy", dict(M=3, N=5, trans_a=True, a=A, c=np.zeros(15))),
                       ("add_diag", dict(M=3, c=np.eye(3), d=np.ones(3))), ("add_diag", dict(M=3, c=np.eye(3))),
                       ("symmetrize", dict(M=3, c=np.eye(3))), ("col_abs_sums", dict(M=5, N=3, a=A)),
                       ("kron", dict(M=5, N=3, K=3, batch=4, a=A, b=B, c=np.zeros(180)))]:
            with pytest.raises(_solve.error, match="no HIP device"):
                _solve.gemm_op(op, **kw)
