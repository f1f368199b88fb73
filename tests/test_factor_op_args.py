"""The test entry of the dense factor layer (include/epsilon_hip.h eps_test_factor_op): the argument
checks.  They fail before any device work: they need the built library, not a GPU."""

import ctypes
import os

import numpy as np
import pytest

from epsilon_amd import _solve


@pytest.fixture(scope="module")
def lib_built():
    if not os.path.exists(_solve.LIB_PATH):
        pytest.fail("libepsilon_hip.so is not built")
    return _solve


A = np.eye(5) + 0.125 * np.ones((5, 5))   # 5 x 5, symmetric positive definite
OPS = "spd_inverse or spd_inverse_columns"
BOTH = ["spd_inverse", "spd_inverse_columns"]


def factor(op="spd_inverse", **kw):
    args = dict(n=5, a=A.flatten(order="F"))
    args.update(kw)
    return _solve.factor_op(op, **args)


@pytest.mark.parametrize("op", ["", "SPD_INVERSE", "potrf", "spd_inverse_column", "spd_inverse "])
def test_unknown_op(lib_built, op):
    with pytest.raises(_solve.error, match="eps_test_factor_op: op must be %s, got %s$" % (OPS, op)):
        factor(op)


def test_null_op(lib_built):
    with pytest.raises(_solve.error, match="eps_test_factor_op: op is null"):
        factor(None)


@pytest.mark.parametrize("op", BOTH)
def test_null_matrix(lib_built, op):
    with pytest.raises(_solve.error, match="eps_test_factor_op: a is null"):
        factor(op, a=None)


@pytest.mark.parametrize("op", BOTH)
def test_null_result(lib_built, op):
    """The binding always passes a result: the C entry is called directly."""
    L = _solve.lib()
    L.eps_test_factor_op.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    a = A.flatten(order="F")
    g = _solve._FactorOp()
    g.op, g.n, g.form = op.encode(), 5, -1
    g.a, g.a_len = a.ctypes.data_as(ctypes.c_void_p), a.size
    assert L.eps_test_factor_op(ctypes.byref(g), None, None) != 0
    assert "eps_test_factor_op: out is null" in L.eps_last_error().decode()
    assert L.eps_test_factor_op(None, None, None) != 0
    assert "eps_test_factor_op: args is null" in L.eps_last_error().decode()


@pytest.mark.parametrize("op", BOTH)
def test_negative_size(lib_built, op):
    with pytest.raises(_solve.error, match="eps_test_factor_op: n is negative: -2"):
        factor(op, n=-2)


@pytest.mark.parametrize("op", BOTH)
def test_matrix_length(lib_built, op):
    with pytest.raises(_solve.error, match="eps_test_factor_op: a has 25 entries, the dimensions need 16"):
        factor(op, n=4)
    with pytest.raises(_solve.error, match="eps_test_factor_op: a has 25 entries, the dimensions need 36"):
        factor(op, n=6)
    with pytest.raises(_solve.error, match="eps_test_factor_op: a has 25 entries, the dimensions need 0"):
        factor(op, n=0)


@pytest.mark.parametrize("op", BOTH)
def test_negative_offset(lib_built, op):
    with pytest.raises(_solve.error, match="eps_test_factor_op: a_off is negative: -1"):
        factor(op, a_off=-1)


@pytest.mark.parametrize("op", BOTH)
@pytest.mark.parametrize("form", [-2, 2, 7])
def test_form_outside_its_range(lib_built, op, form):
    with pytest.raises(_solve.error, match="eps_test_factor_op: form must be -1, 0 or 1, got %d" % form):
        factor(op, form=form)


def test_column_slab(lib_built):
    cols = "spd_inverse_columns"
    with pytest.raises(_solve.error, match="eps_test_factor_op: lo is negative: -1"):
        factor(cols, lo=-1, cnt=1)
    with pytest.raises(_solve.error, match="eps_test_factor_op: cnt is negative: -1"):
        factor(cols, lo=1, cnt=-1, out_cols=0)
    with pytest.raises(_solve.error, match=r"eps_test_factor_op: lo \+ cnt > n: 3 \+ 3 > 5"):
        factor(cols, lo=3, cnt=3)
    with pytest.raises(_solve.error, match=r"eps_test_factor_op: lo \+ cnt > n: 6 \+ 0 > 5"):
        factor(cols, lo=6, cnt=0)
    with pytest.raises(_solve.error, match=r"eps_test_factor_op: lo \+ cnt > n: 0 \+ 6 > 5"):
        factor(cols, lo=0, cnt=6)
    with pytest.raises(_solve.error, match="eps_test_factor_op: out_cols 2 < cnt 3"):
        factor(cols, lo=0, cnt=3, out_cols=2)
    with pytest.raises(_solve.error, match="eps_test_factor_op: out_cols -1 < cnt 0"):
        factor(cols, lo=0, cnt=0, out_cols=-1)


def test_what_an_op_has_no_use_for_must_not_be_given(lib_built):
    """Both ops have a second result (X = L^-1, the factor), so no out2 is ever refused; the slab
    arguments belong to spd_inverse_columns alone."""
    for name in ("lo", "cnt", "out_cols"):
        with pytest.raises(_solve.error, match=r"eps_test_factor_op: %s is given \(2\), spd_inverse has no column slab" % name):
            factor("spd_inverse", **{name: 2})


def test_every_check_comes_before_device_work(lib_built):
    """With arguments that pass, the call goes on to the device: without one it fails there (no
    fallback), with one it answers."""
    calls = [("spd_inverse", dict()), ("spd_inverse", dict(want_out2=True, a_off=1, form=1)),
             ("spd_inverse_columns", dict(lo=2, cnt=3, out_cols=4, want_out2=True)),
             ("spd_inverse_columns", dict(lo=5, cnt=0)), ("spd_inverse", dict(n=0, a=np.zeros(0)))]
    if _solve.device_count() > 0:
        G = _solve.DENSE_OP_GUARD
        for dtype in ("f64", "f32"):
            _solve.set_option("dtype", dtype)
            try:
                for op, kw in calls:
                    out, _ = factor(op, **kw)
                    assert np.all(out[:G] == _solve.DENSE_OP_SENTINEL) and np.all(out[-G:] == _solve.DENSE_OP_SENTINEL)
                out, _ = factor()
                np.testing.assert_allclose(out[G:-G].reshape((5, 5), order="F"), np.linalg.inv(A), rtol=1e-5)
            finally:
                _solve.set_option("dtype", "f32")
    else:
        for op, kw in calls:
            with pytest.raises(_solve.error, match="no HIP device"):
                factor(op, **kw)
