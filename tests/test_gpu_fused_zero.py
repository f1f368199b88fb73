"""The fused sweep of ZERO-term problems (option "fused_zero"): basis pursuit and
hinge / deadzone loss with an l1 penalty in graph form run as one pass over the data matrix (tag
"zero_fused"), one row kernel (tag "zero_fused_rows"; basis pursuit has none) and the apply of the
cached inverse.  Problems: problems.basis_pursuit, problems.hinge_l1, problems.deadzone_l1, seed 0.

Tolerances are the project's own: against the oracle as in test_more_benchmark_problems
(test_gpu_parity.py: f64 rtol 1e-6, atol 1e-8; f32 rtol = atol = 5e-3, equal state and stopping
sweep).

Shapes: (256, 601) the row floor, 64 live threads of the pass, odd n with a trailing unpaired
column; (260, 601) rows past a wave boundary; (1028, 2051) a second, ragged row chunk per thread
and the tile-packed symmetric apply of the inverse.

The basis pursuit shapes stop with a margin on both sides in the oracle (r / eps_pri <= 0.852 at
the stopping check, >= 1.027 at the check before, s / eps_dual <= 0.33 throughout), so f32 rounding
cannot move the stopping sweep; hinge_l1(256, 601) stops at 270 with 0.899 after 1.002, enough for
f64 alone."""

import numpy as np
import pytest

from epsilon_amd import problems, wire
from oracle import epsilon_oracle as orc
from tests import route_support as rs

pytestmark = pytest.mark.gpu

SHAPES = [(256, 601), (260, 601), (1028, 2051)]
FIXED = dict(max_iterations=60, abs_tol=0.0, rel_tol=0.0)
# routes.solve(prob, dtype, route, fused, **solver params): the options of a solve here
ROUTE_OPTIONS = (("route", "fused_zero", "auto"), ("fused", "fused", "1"))
ON = rs.switched_on(ROUTE_OPTIONS)  # nothing: the route is the library's default


def zero_tags(c):
    return sorted(t for t in c if t.startswith("zero_fused"))


@pytest.fixture
def routes(solve_mod):
    return rs.Routes(solve_mod, ROUTE_OPTIONS)


make = rs.memoised({
    "bp": lambda m, n: problems.basis_pursuit(m, n)[0],
    "deadzone": lambda m, n: problems.deadzone_l1(m, n)[0],
    "hinge_default": lambda m, n: problems.hinge_l1(m, n)[0],
    "hinge": lambda m, n: problems.hinge_l1(m, n, lam=0.01 * rs.lam_scale("hinge_l1", m, n))[0],
    "hinge_tall": lambda m, n: problems.hinge_l1(m, n)[0],
    "lp": lambda m, n: problems.lp(m, n)[0],
    "lad": lambda m, n: problems.least_abs_dev(m, n)[0],
})
oracle = rs.oracle_of(make)


def assert_route(c, st, rows, shape):
    """one pass per sweep (the checks are not pipelined: nothing is discarded), the row kernel
    with it where the problem has a z block, the packed symmetric apply from 1024 rows"""
    assert c.get("zero_fused", 0) == rs.sweeps(st), (zero_tags(c), c.get("zero_fused"), rs.sweeps(st))
    assert c.get("zero_fused_rows", 0) == (rs.sweeps(st) if rows else 0), (c.get("zero_fused_rows"), rs.sweeps(st))
    assert "lasso_fused" not in c
    if shape[0] >= 1024:
        assert c.get("symv_packed", 0) >= rs.sweeps(st), sorted(c)


# ---- 1. basis pursuit, default stopping rule -------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("shape,stop", list(zip(SHAPES, [60, 60, 50])))
def test_basis_pursuit_stops_with_the_oracle(routes, dtype, shape, stop):
    so, xo = oracle("bp", shape)
    assert so.state == wire.SolverStatus.OPTIMAL and so.num_iterations == stop
    st, x, c = routes.solve(make("bp", shape), dtype)
    rs.assert_matches_oracle(st, x, so, xo, dtype)
    assert_route(c, st, False, shape)


# ---- 2. fixed 60 sweeps, every variable against the oracle -----------------------------------------
def assert_both_sides(kind, xo):
    """on the oracle's result alone: the 60-sweep iterate has entries on both sides of every
    threshold of the two chains"""
    x = xo["var:x"]
    print(kind, "x nonzero", int((x != 0).sum()), "of", x.size)
    assert 0 < (x != 0).sum() < x.size
    if kind == "hinge":
        h = 1.0 - xo["var:z"]
        print("hinge: 1 - z < 0 on", int((h < 0).sum()), "rows, == 0 on", int((h == 0).sum()))
        assert (h < 0).sum() > 0 and (h == 0).sum() > 0 and (h < 0).sum() + (h == 0).sum() == h.size
    if kind == "deadzone":
        z, M = xo["var:z"], 0.5
        cls = [(np.abs(z) < M).sum(), (z == M).sum(), (z == -M).sum(), (z > M).sum(), (z < -M).sum()]
        print("deadzone: inside, on +, on -, beyond +, beyond -:", [int(v) for v in cls])
        assert all(v > 0 for v in cls)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", ["hinge", "deadzone", "bp"])
def test_sixty_sweeps_match_the_oracle(routes, kind, shape, dtype):
    so, xo = oracle(kind, shape, **FIXED)
    assert so.state == wire.SolverStatus.MAX_ITERATIONS_REACHED and so.num_iterations == 60
    assert sorted(xo) == (["separate:var:x:zero", "var:x"] if kind == "bp" else
                          ["separate:var:x:zero", "separate:var:z:zero", "var:x", "var:z"])
    assert_both_sides(kind, xo)
    st, x, c = routes.solve(make(kind, shape), dtype, **FIXED)
    assert_route(c, st, kind != "bp", shape)
    rs.assert_matches_oracle(st, x, so, xo, dtype)


# ---- 3. hinge, default stopping rule, f64 -----------------------------------------------------------
def test_hinge_stops_with_the_oracle_f64(routes):
    shape = (256, 601)
    so, xo = oracle("hinge_default", shape)
    assert so.state == wire.SolverStatus.OPTIMAL and so.num_iterations == 270
    st, x, c = routes.solve(make("hinge_default", shape), "f64")
    assert_route(c, st, True, shape)
    rs.assert_matches_oracle(st, x, so, xo, "f64")


# ---- 4. fused against generic, f64 --------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hinge", "deadzone", "bp"])
def test_fused_equals_generic_to_rounding_f64(routes, kind):
    shape = (260, 601)
    prob = make(kind, shape)
    st, x, c = routes.solve(prob, "f64", "auto", **FIXED)
    st0, x0, c0 = routes.solve(prob, "f64", "0", **FIXED)
    assert_route(c, st, kind != "bp", shape)
    assert not zero_tags(c0)
    assert rs.status(st).num_iterations == rs.status(st0).num_iterations == 60
    for k in x0:
        diff, ref = np.abs(x[k] - x0[k]).max(), np.abs(x0[k]).max()
        print(k, "max |fused - generic| %.3g, max |generic| %.3g" % (diff, ref))
        assert diff <= 1e-9 * ref, k


# ---- 5. what keeps the generic path ---------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,dtype,params,fused", [
    ("bp", (252, 601), "f64", {}, "1"),           # below the row floor
    ("bp", (258, 601), "f32", {}, "1"),           # rows not a multiple of 4
    ("hinge_tall", (300, 100), "f32", {}, "1"),   # tall: the order ends in x'
    ("lp", (256, 601), "f32", {}, "1"),           # AFFINE / NON_NEGATIVE terms
    ("lad", (300, 40), "f32", {}, "1"),           # x lives in the ZERO term alone
    ("hinge", (256, 601), "f32", {"solver": 1}, "1"),  # two-block driver
    ("hinge", (256, 601), "f32", {}, "0"),        # the fused routes switched off altogether
])
def test_fall_backs_are_the_generic_path(routes, kind, shape, dtype, params, fused):
    prob = make(kind, shape)
    params = dict(max_iterations=30, **params)
    st, x, c = routes.solve(prob, dtype, "auto", fused, **params)
    st0, x0, c0 = routes.solve(prob, dtype, "0", fused, **params)
    assert not zero_tags(c) and not zero_tags(c0)
    rs.assert_same_bytes(st, x, st0, x0)


def test_rows_multiple_of_two_take_the_route_in_f64(routes):
    st, x, c = routes.solve(make("bp", (258, 601)), "f64", max_iterations=30)
    assert_route(c, st, False, (258, 601))


# ---- 6. sweep boundaries and warm start -------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_a_solve_can_stop_after_any_sweep(solve_mod, dtype):
    prob = make("hinge_default", (256, 601))
    params = dict(max_iterations=1000, abs_tol=0.0, rel_tol=0.0)
    st_a, xa, ca = rs.run_handle(solve_mod, prob, dtype, [30], ON, **params)
    st_b, xb, cb = rs.run_handle(solve_mod, prob, dtype, [1, 9, 20], ON, **params)
    assert ca.get("zero_fused") == cb.get("zero_fused") == 30
    assert ca.get("zero_fused_rows") == cb.get("zero_fused_rows") == 30
    assert len(xa) == 4
    rs.assert_same_arrays(xa, xb)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_warm_start_takes_the_state_over(solve_mod, dtype):
    """two solves of 30 sweeps on one handle, the second warm-started, against the oracle doing
    the same on one solver object"""
    prob = make("hinge_default", (256, 601))
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
    rs.assert_close(x, {k: np.asarray(xo(k), dtype=np.float64).ravel() for k in x}, dtype)
    # the second solve went on from the first: it is not the cold solve's iterate (in the oracle
    # the two differ by 0.94 in z, far above the tolerances)
    cold = oracle("hinge_default", (256, 601), max_iterations=30, abs_tol=0.0, rel_tol=0.0)[1]
    assert np.abs(x["var:z"] - cold["var:z"]).max() > 0.1


# ---- 7. determinism ------------------------------------------------------------------------------------
def test_two_solves_return_the_same_bytes(routes):
    prob = make("deadzone", (1028, 2051))
    st1, x1, c1 = routes.solve(prob, "f32", **FIXED)
    st2, x2, c2 = routes.solve(prob, "f32", **FIXED)
    assert_route(c1, st1, True, (1028, 2051))
    assert c1.get("zero_fused") == c2.get("zero_fused")
    rs.assert_same_arrays(x1, x2)
