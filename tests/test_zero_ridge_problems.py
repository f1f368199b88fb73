"""The graph-form problems with a ridge penalty on x (problems.hinge_l2, svr_l2, logreg_l2): their
structure - the variables and keys of hinge_l1, the terms in the order loss, SUM_SQUARE, ZERO - and
that the CPU oracle solves these forms.  No GPU, no built library.

Figures measured on the oracle: the logistic stationarity ratio ||C^T sigma(C x) + 2 lam x|| /
||2 lam x|| at abs_tol = rel_tol = 1e-6 is 1.3e-5 at (603, 260) and 2.0e-5 at (260, 601); the
hinge_l2 objective at the default tolerances is 0.31 % above the one at 1e-7 at (603, 260) with
lam = 0.1 and 0.88 % at (260, 601) with lam = 1.0."""

import numpy as np
import pytest

from epsilon_amd import ir, problems, wire
from epsilon_amd.wire import ProxFunction
from oracle import epsilon_oracle as orc

BUILDERS = {
    "hinge_l2": (problems.hinge_l2, ProxFunction.SUM_HINGE),
    "svr_l2": (problems.svr_l2, ProxFunction.SUM_DEADZONE),
    "logreg_l2": (problems.logreg_l2, ProxFunction.SUM_LOGISTIC),
}


def solve(prob, **kw):
    st, x = orc.solve(prob.SerializeToString(), [], wire.SolverParams(**kw).SerializeToString(),
                      prob.expression_data())
    return wire.SolverStatus.FromString(st), {k: np.frombuffer(v) for k, v in x.items()}


def term_keys(prob, term):
    """the keys of a term's block factorisation in the oracle, in elimination order"""
    s = orc.create_solver(wire.Problem.FromString(prob.SerializeToString()), dict(prob.expression_data()),
                          wire.SolverParams(max_iterations=1))
    s.solve()
    return list(s.prox[term].chol.p)


@pytest.mark.parametrize("kind", sorted(BUILDERS))
@pytest.mark.parametrize("shape", [(12, 5), (5, 12)])
def test_structure_is_hinge_l1_with_a_ridge_term(kind, shape):
    build, loss = BUILDERS[kind]
    prob, info = build(*shape, lam=0.1)
    ref = problems.hinge_l1(*shape)[0]
    p = prob.proto()
    assert [t.prox_function.prox_function_type for t in p.objective.arg] == [
        loss, ProxFunction.SUM_SQUARE, ProxFunction.ZERO]
    assert p.objective.arg[1].prox_function.alpha == 0.1 and info["lam"] == 0.1
    assert ir.get_variables(p) == ir.get_variables(ref.proto())
    assert len(p.constraint) == len(ref.proto().constraint) == 2
    keys = term_keys(prob, 2)
    assert len(keys) == 5 and sorted(keys) == sorted(term_keys(ref, 2))
    # the order the fused routes' descriptor accepts for the ridge term (prox.cc)
    assert term_keys(prob, 1) == ["arg:0", "constraint:0", "var:x"]
    m, n = shape
    assert info["A"].shape == (m, n) and info["b"].shape == (m,)
    np.testing.assert_allclose(np.sum(info["A"] ** 2, 0), 1.0, rtol=1e-12)


def test_data_follows_the_stated_draws():
    m, n = 9, 4
    rng = np.random.RandomState(3)
    A = rng.randn(m, n)
    A /= np.sqrt(np.sum(A ** 2, 0))
    x0, e = rng.randn(n), rng.randn(m)
    y = np.sign(A.dot(x0) + 0.05 * e)
    h = problems.hinge_l2(m, n, seed=3)[1]
    r = problems.svr_l2(m, n, seed=3)[1]
    g = problems.logreg_l2(m, n, seed=3)[1]
    assert np.array_equal(h["C"], y[:, None] * A) and np.array_equal(h["b"], y) and h["lam"] == 1.0
    assert np.array_equal(r["A"], A) and np.array_equal(r["b"], A.dot(x0) + e) and r["M"] == 0.5
    assert np.array_equal(g["C"], -y[:, None] * A) and g["lam"] == 1.0


@pytest.mark.parametrize("shape", [(603, 260), (260, 601)])
def test_oracle_solves_logreg_l2_to_stationarity(shape):
    prob, info = problems.logreg_l2(*shape, lam=0.1)
    S, x = solve(prob, abs_tol=1e-6, rel_tol=1e-6, max_iterations=5000)
    assert S.state == wire.SolverStatus.OPTIMAL
    C, lam, xv = info["C"], info["lam"], x["var:x"]
    grad = C.T.dot(1.0 / (1.0 + np.exp(-C.dot(xv)))) + 2 * lam * xv
    ratio = np.linalg.norm(grad) / np.linalg.norm(2 * lam * xv)
    print(shape, "stationarity ratio %.3g at %d" % (ratio, S.num_iterations))
    assert ratio <= 1e-4


@pytest.mark.parametrize("shape", [(603, 260), (260, 601)])
def test_oracle_hinge_l2_objective_at_default_tolerances(shape):
    prob, info = problems.hinge_l2(*shape, lam=0.1 if shape[0] > shape[1] else 1.0)
    S, x = solve(prob)
    S7, x7 = solve(prob, abs_tol=1e-7, rel_tol=1e-7, max_iterations=20000)
    assert S.state == S7.state == wire.SolverStatus.OPTIMAL
    obj = problems.hinge_l2_objective(info["C"], info["lam"], x["var:x"])
    obj7 = problems.hinge_l2_objective(info["C"], info["lam"], x7["var:x"])
    print(shape, "objective %.8g at %d, %.8g at %d: %.3g %%" % (
        obj, S.num_iterations, obj7, S7.num_iterations, 100 * (obj / obj7 - 1)))
    assert abs(obj - obj7) <= 1e-2 * abs(obj7)


def test_objectives():
    rng = np.random.RandomState(0)
    C, x, b = rng.randn(6, 3), rng.randn(3), rng.randn(6)
    z = C.dot(x)
    assert np.isclose(problems.hinge_l2_objective(C, 0.3, x), np.maximum(1 - z, 0).sum() + 0.3 * x.dot(x))
    assert np.isclose(problems.svr_l2_objective(C, b, 0.3, 0.5, x),
                      np.maximum(np.abs(z - b) - 0.5, 0).sum() + 0.3 * x.dot(x))
    assert np.isclose(problems.logreg_l2_objective(C, 0.3, x), np.log1p(np.exp(z)).sum() + 0.3 * x.dot(x))
