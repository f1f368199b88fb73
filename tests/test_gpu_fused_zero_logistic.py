"""l1-regularised logistic regression on the fused sweep of ZERO-term problems:
problems.logreg_l1, seed 0, runs as one pass over the data matrix (tag "zero_fused"), one row
kernel with the logistic prox in it (tag "zero_fused_rows") and the apply of the cached inverse.

Tolerances are the project's own: against the oracle f64 rtol 1e-6, atol 1e-8; f32 rtol = atol =
5e-3, equal state and stopping sweep.

Shapes: (256, 601) the row floor, whole 64-row workgroups of the row kernel; (260, 601) and
(1028, 2051) a last workgroup of 4 rows, the latter with the tile-packed symmetric apply.

Oracle facts the tests rest on (asserted where they are used).  After 60 sweeps x has 17-753
non-zeros of both signs and |z| spans 0.3-7.8, so both thresholds on x and the curved part of the
logistic prox are exercised.  Default stopping rule, r / eps_pri at the stopping check and at the
check before, s / eps_dual: (256, 601) stops at 60 with 0.838 after 1.256, <= 0.50; (260, 601) at
60 with 0.863 after 1.268, <= 0.47 - margins f32 rounding cannot cross; (1028, 2051) at 120 with
0.953 after 1.046, <= 0.20: f64 alone."""

import numpy as np
import pytest

from epsilon_amd import problems, wire
from oracle import epsilon_oracle as orc
from tests import route_support as rs

pytestmark = pytest.mark.gpu

SHAPES = [(256, 601), (260, 601), (1028, 2051)]
FIXED = dict(max_iterations=60, abs_tol=0.0, rel_tol=0.0)
KEYS = ["separate:var:x:zero", "separate:var:z:zero", "var:x", "var:z"]
# routes.solve(prob, dtype, route, fused, **solver params): the options of a solve here
ROUTE_OPTIONS = (("route", "fused_zero", "auto"), ("fused", "fused", "1"))
ON = rs.switched_on(ROUTE_OPTIONS)  # nothing: the route is the library's default


def zero_tags(c):
    return sorted(t for t in c if t.startswith("zero_fused"))


@pytest.fixture
def routes(solve_mod):
    return rs.Routes(solve_mod, ROUTE_OPTIONS)


# kind "default": the default lambda, 0.1 max|C^T 1/2|; "small": a tenth of it
make = rs.memoised({
    "default": lambda m, n: problems.logreg_l1(m, n)[0],
    "small": lambda m, n: problems.logreg_l1(m, n, lam=0.01 * rs.lam_scale("logreg_l1", m, n))[0],
})
oracle = rs.oracle_of(make)


def assert_route(c, st, shape):
    """one pass and one row kernel per sweep (the checks are not pipelined: nothing is discarded),
    the packed symmetric apply from 1024 rows"""
    assert c.get("zero_fused", 0) == rs.sweeps(st), (zero_tags(c), c.get("zero_fused"), rs.sweeps(st))
    assert c.get("zero_fused_rows", 0) == rs.sweeps(st), (c.get("zero_fused_rows"), rs.sweeps(st))
    assert "lasso_fused" not in c
    if shape[0] >= 1024:
        assert c.get("symv_packed", 0) >= rs.sweeps(st), sorted(c)


# ---- 1. fixed 60 sweeps, every variable against the oracle -----------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", ["default", "small"])
def test_sixty_sweeps_match_the_oracle(routes, kind, shape, dtype):
    so, xo = oracle(kind, shape, **FIXED)
    assert so.state == wire.SolverStatus.MAX_ITERATIONS_REACHED and so.num_iterations == 60
    assert sorted(xo) == KEYS
    x, z = xo["var:x"], np.abs(xo["var:z"])
    print(kind, "x > 0:", int((x > 0).sum()), "x < 0:", int((x < 0).sum()), "of", x.size,
          "|z| in [%.3g, %.3g]" % (z.min(), z.max()))
    assert (x > 0).sum() > 0 and (x < 0).sum() > 0 and (x == 0).sum() > 0
    assert z.min() < 3 and z.max() > 4.5  # rows on the bend of the logistic loss and far out in its tails
    st, x, c = routes.solve(make(kind, shape), dtype, **FIXED)
    assert_route(c, st, shape)
    rs.assert_matches_oracle(st, x, so, xo, dtype)


# ---- 2. default stopping rule -------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dtype,stop,ratio", [
    ((256, 601), "f32", 60, 0.838),
    ((256, 601), "f64", 60, 0.838),
    ((260, 601), "f32", 60, 0.863),
    ((260, 601), "f64", 60, 0.863),
    ((1028, 2051), "f64", 120, 0.953),
])
def test_stops_with_the_oracle(routes, shape, dtype, stop, ratio):
    so, xo = oracle("default", shape)
    assert so.state == wire.SolverStatus.OPTIMAL and so.num_iterations == stop
    assert abs(so.residuals.r_norm / so.residuals.epsilon_primal - ratio) < 1e-3
    assert so.residuals.s_norm <= 0.5 * so.residuals.epsilon_dual
    st, x, c = routes.solve(make("default", shape), dtype)
    assert_route(c, st, shape)
    rs.assert_matches_oracle(st, x, so, xo, dtype)


# ---- 3. fused against generic, f64 --------------------------------------------------------------------
def test_fused_equals_generic_to_rounding_f64(routes):
    """both routes run the same fp64 ProxElem, the prox is 1-Lipschitz, and only the order of the
    sums differs"""
    shape = (260, 601)
    prob = make("default", shape)
    st, x, c = routes.solve(prob, "f64", "auto", **FIXED)
    st0, x0, c0 = routes.solve(prob, "f64", "0", **FIXED)
    assert_route(c, st, shape)
    assert not zero_tags(c0)
    assert rs.status(st).num_iterations == rs.status(st0).num_iterations == 60
    assert sorted(x) == sorted(x0) == KEYS
    for k in x0:
        diff, ref = np.abs(x[k] - x0[k]).max(), np.abs(x0[k]).max()
        print(k, "max |fused - generic| %.3g, max |generic| %.3g" % (diff, ref))
    for k in x0:
        assert np.abs(x[k] - x0[k]).max() <= 1e-9 * np.abs(x0[k]).max(), k


# ---- 4. sweep boundaries and warm start -------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_a_solve_can_stop_after_any_sweep(solve_mod, dtype):
    """the head the row kernel carries from one sweep to the next survives the end of a run call"""
    prob = make("default", (256, 601))
    params = dict(max_iterations=1000, abs_tol=0.0, rel_tol=0.0)
    st_a, xa, ca = rs.run_handle(solve_mod, prob, dtype, [30], ON, **params)
    st_b, xb, cb = rs.run_handle(solve_mod, prob, dtype, [1, 7, 22], ON, **params)
    assert ca.get("zero_fused") == cb.get("zero_fused") == 30
    assert ca.get("zero_fused_rows") == cb.get("zero_fused_rows") == 30
    assert sorted(xa) == sorted(xb) == KEYS
    rs.assert_same_arrays(xa, xb)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_warm_start_takes_the_state_over(solve_mod, dtype):
    """two solves of 30 sweeps on one handle, the second warm-started, against the oracle doing
    the same on one solver object: the first head of the second solve comes from the adopted state"""
    prob = make("default", (256, 601))
    sp = wire.SolverParams(warm_start=True, max_iterations=30, abs_tol=0.0, rel_tol=0.0)
    pb, data = prob.SerializeToString(), prob.expression_data()
    with rs.handle(solve_mod, prob, dtype, sp, **ON) as s:
        s.init()
        s.run(-1)
        s.init()
        s.run(-1)
        c = rs.base_counts(solve_mod.profile_dump())
        st, x = s.result()
    assert c.get("zero_fused") == c.get("zero_fused_rows") == 60
    osolver = orc.create_solver(wire.Problem.FromString(pb), dict(data), sp)
    osolver.solve()
    xo = osolver.solve()
    assert rs.status(st).num_iterations == osolver.status.num_iterations == 30
    x = rs.arrays(x)
    xo = {k: np.asarray(xo(k), dtype=np.float64).ravel() for k in x}
    # the second solve went on from the first: in the oracle it is not the cold solve's iterate,
    # by far more than the tolerances
    cold = oracle("default", (256, 601), max_iterations=30, abs_tol=0.0, rel_tol=0.0)[1]
    print("oracle: max |warm - cold| in z %.3g" % np.abs(xo["var:z"] - cold["var:z"]).max())
    assert np.abs(xo["var:z"] - cold["var:z"]).max() > 0.1
    rs.assert_close(x, xo, dtype)


# ---- 5. determinism ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_two_solves_return_the_same_bytes(routes, dtype):
    shape = (1028, 2051)
    prob = make("default", shape)
    st1, x1, c1 = routes.solve(prob, dtype, **FIXED)
    st2, x2, c2 = routes.solve(prob, dtype, **FIXED)
    assert_route(c1, st1, shape)
    assert_route(c2, st2, shape)
    assert sorted(x1) == sorted(x2) == KEYS
    rs.assert_same_arrays(x1, x2)


# ---- 6. what keeps the generic path ---------------------------------------------------------------------
@pytest.mark.parametrize("shape,dtype,params,fused", [
    ((252, 601), "f64", {}, "1"),             # below the row floor
    ((300, 100), "f32", {}, "1"),             # tall: the order ends in x'
    ((256, 601), "f32", {"solver": 1}, "1"),  # two-block driver
    ((256, 601), "f32", {}, "0"),             # the fused routes switched off altogether
])
def test_fall_backs_are_the_generic_path(routes, shape, dtype, params, fused):
    prob = make("default", shape)
    params = dict(max_iterations=30, **params)
    st, x, c = routes.solve(prob, dtype, "auto", fused, **params)
    st0, x0, c0 = routes.solve(prob, dtype, "0", fused, **params)
    assert not zero_tags(c) and not zero_tags(c0)
    assert sorted(x) == sorted(x0) == KEYS
    rs.assert_same_bytes(st, x, st0, x0)
