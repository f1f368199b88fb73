"""Host-side checks of the segmented TV-1D prox: what the problem builders put on the wire, the
argument validation of `_solve.tv1d_batch` (which needs no library), and the alternating-prox
reference that tests/test_gpu_tv_segments.py holds the 2-D problem against."""
import numpy as np
import pytest

from epsilon_amd import _solve, ir, problems, wire
from epsilon_amd.wire import ProxFunction


def tv_slices(V, lam, axis):
    """The DP oracle on every column (axis 0) or row (axis 1) of V."""
    from oracle import c_oracle
    V = np.asarray(V, dtype=np.float64)
    out = np.empty_like(V)
    if axis == 0:
        for j in range(V.shape[1]):
            out[:, j] = c_oracle.tv1d(V[:, j], lam)
    else:
        for i in range(V.shape[0]):
            out[i, :] = c_oracle.tv1d(V[i, :], lam)
    return out


def dykstra_tv2d(B, lam_cols, lam_rows, max_iter=20000):
    """argmin 1/2 ||X - B||^2 + lam_cols TV(columns of X) + lam_rows TV(rows of X) by Dykstra's
    alternating prox (Bauschke & Combettes 2008), the DP oracle per column and per row, until the
    objective changes by less than 1e-10 relative.  Returns (X, objective, iterations)."""
    def objective(X):
        return float(0.5 * np.sum((X - B) ** 2) + lam_cols * np.abs(np.diff(X, axis=0)).sum() +
                     lam_rows * np.abs(np.diff(X, axis=1)).sum())
    X = np.array(B, dtype=np.float64)
    P, Q = np.zeros_like(X), np.zeros_like(X)
    prev = objective(X)
    for it in range(1, max_iter + 1):
        Y = tv_slices(X + P, lam_cols, 0)
        P = X + P - Y
        X = tv_slices(Y + Q, lam_rows, 1)
        Q = Y + Q - X
        obj = objective(X)
        if abs(obj - prev) < 1e-10 * max(abs(obj), 1e-300):
            return X, obj, it
        prev = obj
    raise AssertionError("Dykstra did not settle in %d iterations" % max_iter)


def roundtrip(expr_proto):
    return wire.Expression.FromString(expr_proto.SerializeToString())


@pytest.mark.parametrize("axis", [0, 1])
def test_tv_prox_expr_on_the_wire(axis):
    e = roundtrip(problems.tv_prox_expr(12, 7, axis, lam_alpha=2.5).proto)
    f = e.prox_function
    assert e.expression_type == wire.Expression.PROX_FUNCTION
    assert f.prox_function_type == ProxFunction.TOTAL_VARIATION_1D
    assert f.has_axis and f.axis == axis and f.alpha == 2.5
    assert [list(s.dim) for s in f.arg_size] == [[12, 7]]
    assert ir.get_variables(e) and list(ir.get_variables(e)) == ["var:X"]


def test_tv_1d_prox_expr_keeps_no_axis():
    f = roundtrip(problems.tv_1d_prox_expr(9).proto).prox_function
    assert not f.has_axis


def test_tv_2d_on_the_wire():
    prob, info = problems.tv_2d(6, 5, seed=1)
    assert info["B"].shape == (6, 5) and info["lam"] > 0
    p = wire.Problem.FromString(prob.SerializeToString())
    terms = list(p.objective.arg)
    assert len(terms) == 3 and len(p.constraint) == 2
    kinds = [t.prox_function.prox_function_type for t in terms]
    assert kinds == [ProxFunction.SUM_SQUARE, ProxFunction.TOTAL_VARIATION_1D, ProxFunction.TOTAL_VARIATION_1D]
    assert not terms[0].prox_function.has_axis
    for t, axis in ((terms[1], 0), (terms[2], 1)):
        f = t.prox_function
        assert f.has_axis and f.axis == axis and f.alpha == info["lam"]
        assert [list(s.dim) for s in f.arg_size] == [[6, 5]]
    # the row term keeps X itself, the other two work on copies
    assert list(ir.get_variables(terms[2])) == ["var:X"]
    assert set(ir.get_variables(p)) == {"var:X", "separate:var:X:sum_square", "separate:var:X:tv_axis0"}
    assert all(tuple(sz) == (6, 5) for sz in ir.get_variables(p).values())
    # the image is constant data of the problem, column-major
    assert any(np.array_equal(np.frombuffer(v), info["B"].reshape(-1, order="F"))
               for v in prob.expression_data().values() if len(v) == 8 * 30)


def test_tv_2d_objective():
    B = np.zeros((2, 3))
    X = np.array([[0.0, 1.0, 1.0], [2.0, 1.0, 4.0]])
    # 1/2 ||X||^2 = 11.5, column jumps 2 + 0 + 3, row jumps 1 + 0 + 1 + 3
    assert problems.tv_2d_objective(B, 2.0, X) == 11.5 + 2.0 * 5 + 2.0 * 5


def test_tv1d_batch_validates_before_loading_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_solve, "lib", no_library)
    for bad in (np.zeros(5), np.zeros((2, 3, 4)), 3.0):
        with pytest.raises(_solve.error, match="2-D"):
            _solve.tv1d_batch(bad, 1.0)
    for axis in (2, -1, None):
        with pytest.raises(_solve.error, match="axis"):
            _solve.tv1d_batch(np.zeros((3, 4)), 1.0, axis=axis)


def test_dykstra_helper_is_the_column_dp_without_a_row_term():
    rng = np.random.RandomState(4)
    B = np.repeat(rng.randn(4, 9), 5, axis=0) + 0.3 * rng.randn(20, 9)
    X, obj, it = dykstra_tv2d(B, 0.8, 0.0)
    want = tv_slices(B, 0.8, 0)
    np.testing.assert_allclose(X, want, rtol=1e-12, atol=1e-12)
    assert it <= 3
    assert obj == pytest.approx(sum(problems.tv_1d_objective(B[:, j], 0.8, want[:, j]) for j in range(9)), rel=1e-12)
    # and with both terms it does not leave the columns alone
    X2, obj2, _ = dykstra_tv2d(B, 0.8, 0.8)
    assert np.abs(X2 - want).max() > 1e-3
    assert obj2 >= obj
