"""The fused sweep of ZERO-term problems with tall C (DESIGN.md 3.11 "Tall C", option
"fused_zero_tall"): hinge / deadzone loss with an l1 penalty in graph form with more rows than
columns run as one pass over a transposed copy of the data matrix (tag "zero_tall"), one kernel on
the x side (tag "zero_tall_cols") and the apply of the cached n x n inverse.  Problems:
problems.hinge_l1, problems.deadzone_l1, seed 0.  Every solve here sets "fused_zero_tall" = "1" (or
"0" where it says so) and puts "auto" back.

Tolerances are the project's own: against the oracle as in test_more_benchmark_problems
(test_gpu_parity.py: f64 rtol 1e-6, atol 1e-8; f32 rtol = atol = 5e-3, equal state and stopping
sweep); fused against generic in f64 the fat route's bound, 1e-9 of the largest magnitude.

Shapes: (601, 256) the column floor, 64 live threads of the pass, odd m with a trailing unpaired
streamed column, one column pair per workgroup; (603, 260) columns past a wave boundary;
(2051, 1028) a second, ragged chunk per thread, several pairs per workgroup and the tile-packed
symmetric apply of the inverse.

hinge_l1 with its default lambda stops in the oracle at 250 for (601, 256) - r / eps_pri 0.945
there, 1.016 at the check before - and at 200 for (603, 260) - 0.929 after 1.010: margins that
carry f64 rounding, not f32, so the stopping rule is tested in f64 alone.  The default lambda
leaves x = 0 after 60 sweeps at (2051, 1028); the fixed-sweep tests use lambda = 0.01 max|sum_i C_i|."""

import numpy as np
import pytest

from epsilon_amd import problems, wire
from oracle import epsilon_oracle as orc
from tests import route_support as rs

pytestmark = pytest.mark.gpu

SHAPES = [(601, 256), (603, 260), (2051, 1028)]
FIXED = dict(max_iterations=60, abs_tol=0.0, rel_tol=0.0)
# routes.solve(prob, dtype, tall, fused, fused_zero, **solver params): the options of a solve here
ROUTE_OPTIONS = (("tall", "fused_zero_tall", "1"), ("fused", "fused", "1"), ("fused_zero", "fused_zero", "auto"))
ON = rs.switched_on(ROUTE_OPTIONS)  # fused_zero_tall = "1": what the handles and the batch set


def tall_tags(c):
    return sorted(t for t in c if t.startswith("zero_tall"))


@pytest.fixture
def routes(solve_mod):
    return rs.Routes(solve_mod, ROUTE_OPTIONS)


make = rs.memoised({
    "deadzone": lambda m, n: problems.deadzone_l1(m, n)[0],
    "hinge_default": lambda m, n: problems.hinge_l1(m, n)[0],
    "hinge": lambda m, n: problems.hinge_l1(m, n, lam=0.01 * rs.lam_scale("hinge_l1", m, n))[0],
    "logreg": lambda m, n: problems.logreg_l1(m, n)[0],
})
oracle = rs.oracle_of(make)


def assert_route(c, st, shape):
    """one pass and one x-side launch per sweep (the checks are not pipelined: nothing is
    discarded), no launch of the fat route or of the lasso route, the packed symmetric apply from
    1024 columns"""
    assert c.get("zero_tall", 0) == rs.sweeps(st), (tall_tags(c), c.get("zero_tall"), rs.sweeps(st))
    assert c.get("zero_tall_cols", 0) == rs.sweeps(st), (c.get("zero_tall_cols"), rs.sweeps(st))
    assert not [t for t in c if t.startswith("zero_fused")], sorted(c)
    assert "lasso_fused" not in c
    if shape[1] >= 1024:
        assert c.get("symv_packed", 0) >= rs.sweeps(st), sorted(c)


def assert_generic(c):
    assert not tall_tags(c) and not [t for t in c if t.startswith("zero_fused")], sorted(c)


# ---- 1. fixed 60 sweeps, every variable against the oracle -----------------------------------------
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
@pytest.mark.parametrize("kind", ["hinge", "deadzone"])
def test_sixty_sweeps_match_the_oracle(routes, kind, shape, dtype):
    so, xo = oracle(kind, shape, **FIXED)
    assert so.state == wire.SolverStatus.MAX_ITERATIONS_REACHED and so.num_iterations == 60
    assert sorted(xo) == ["separate:var:x:zero", "separate:var:z:zero", "var:x", "var:z"]
    assert_both_sides(kind, xo)
    st, x, c = routes.solve(make(kind, shape), dtype, **FIXED)
    assert_route(c, st, shape)
    rs.assert_matches_oracle(st, x, so, xo, dtype)


# ---- 2. hinge, default stopping rule, f64 -----------------------------------------------------------
@pytest.mark.parametrize("shape,stop", [((601, 256), 250), ((603, 260), 200)])
def test_hinge_stops_with_the_oracle_f64(routes, shape, stop):
    """The oracle stops (601, 256) at 250 with r / eps_pri = 0.945 after 1.016 at the check before,
    (603, 260) at 200 with 0.929 after 1.010: enough for f64, not for f32."""
    so, xo = oracle("hinge_default", shape)
    assert so.state == wire.SolverStatus.OPTIMAL and so.num_iterations == stop
    st, x, c = routes.solve(make("hinge_default", shape), "f64")
    assert_route(c, st, shape)
    rs.assert_matches_oracle(st, x, so, xo, "f64")


# ---- 3. fused against generic, f64 --------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hinge", "deadzone"])
def test_fused_equals_generic_to_rounding_f64(routes, kind):
    shape = (603, 260)
    prob = make(kind, shape)
    st, x, c = routes.solve(prob, "f64", "1", **FIXED)
    st0, x0, c0 = routes.solve(prob, "f64", "0", **FIXED)
    assert_route(c, st, shape)
    assert_generic(c0)
    assert rs.status(st).num_iterations == rs.status(st0).num_iterations == 60
    for k in x0:
        diff, ref = np.abs(x[k] - x0[k]).max(), np.abs(x0[k]).max()
        print(k, "max |fused - generic| %.3g, max |generic| %.3g" % (diff, ref))
        assert diff <= 1e-9 * ref, k


# ---- 4. sweep boundaries and warm start -------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_a_solve_can_stop_after_any_sweep(solve_mod, dtype):
    prob = make("hinge", (601, 256))
    params = dict(max_iterations=1000, abs_tol=0.0, rel_tol=0.0)
    st_a, xa, ca = rs.run_handle(solve_mod, prob, dtype, [30], ON, **params)
    st_b, xb, cb = rs.run_handle(solve_mod, prob, dtype, [1, 9, 20], ON, **params)
    assert ca.get("zero_tall") == cb.get("zero_tall") == 30
    assert ca.get("zero_tall_cols") == cb.get("zero_tall_cols") == 30
    assert len(xa) == 4
    rs.assert_same_arrays(xa, xb)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_warm_start_takes_the_state_over(solve_mod, dtype):
    """two solves of 30 sweeps on one handle, the second warm-started, against the oracle doing
    the same on one solver object"""
    shape = (601, 256)
    prob = make("hinge", shape)
    sp = wire.SolverParams(warm_start=True, max_iterations=30, abs_tol=0.0, rel_tol=0.0)
    pb, data = prob.SerializeToString(), prob.expression_data()
    with rs.handle(solve_mod, prob, dtype, sp, **ON) as s:
        s.init()
        s.run(-1)
        s.init()
        s.run(-1)
        c = rs.base_counts(solve_mod.profile_dump())
        st, x = s.result()
    assert c.get("zero_tall") == c.get("zero_tall_cols") == 60
    osolver = orc.create_solver(wire.Problem.FromString(pb), dict(data), sp)
    osolver.solve()
    xo = osolver.solve()
    assert rs.status(st).num_iterations == osolver.status.num_iterations == 30
    x = rs.arrays(x)
    xw = {k: np.asarray(xo(k), dtype=np.float64).ravel() for k in x}
    # on the oracle alone: the second solve went on from the first, its iterate is not the cold
    # solve's by far more than the tolerances, so a route that dropped the state would not pass
    cold = oracle("hinge", shape, max_iterations=30, abs_tol=0.0, rel_tol=0.0)[1]
    print("oracle: max |warm - cold| in z %.3g" % np.abs(xw["var:z"] - cold["var:z"]).max())
    assert np.abs(xw["var:z"] - cold["var:z"]).max() > 0.1
    rs.assert_close(x, xw, dtype)


# ---- 5. what keeps the generic path under "1" -------------------------------------------------------
@pytest.mark.parametrize("kind,shape,dtype,params,fused,fused_zero", [
    ("logreg", (601, 256), "f32", {}, "1", "auto"),          # a smooth z term
    ("hinge", (600, 252), "f32", {}, "1", "auto"),           # below the column floor
    ("hinge", (601, 258), "f32", {}, "1", "auto"),           # columns not a multiple of 4
    ("hinge", (601, 256), "f32", {"solver": 1}, "1", "auto"),  # two-block driver
    ("hinge", (601, 256), "f32", {}, "0", "auto"),           # the fused routes switched off altogether
    ("hinge", (601, 256), "f32", {}, "1", "0"),              # the ZERO-term routes switched off
])
def test_fall_backs_are_the_generic_path(routes, kind, shape, dtype, params, fused, fused_zero):
    prob = make(kind, shape)
    params = dict(max_iterations=30, **params)
    st, x, c = routes.solve(prob, dtype, "1", fused, fused_zero, **params)
    st0, x0, c0 = routes.solve(prob, dtype, "0", fused, fused_zero, **params)
    assert_generic(c)
    assert_generic(c0)
    rs.assert_same_bytes(st, x, st0, x0)


def test_option_zero_is_the_generic_path(routes):
    """"0" at a shape the route takes: no tall launch, and the bytes of the solve with every fused
    route off"""
    prob = make("hinge", (601, 256))
    st, x, c = routes.solve(prob, "f32", "0", max_iterations=30)
    st0, x0, c0 = routes.solve(prob, "f32", "0", "0", max_iterations=30)
    st1, x1, c1 = routes.solve(prob, "f32", "1", max_iterations=30)
    assert_generic(c)
    assert_generic(c0)
    assert_route(c1, st1, (601, 256))
    rs.assert_same_bytes(st, x, st0, x0)


def test_auto_takes_the_route_from_the_measured_floor(routes):
    """the 4n x n ladder has the fused sweep ahead from its first cell, n = 256, so
    "auto" takes the route wherever "1" does"""
    st, x, c = routes.solve(make("hinge", (601, 256)), "f32", "auto", max_iterations=30)
    st1, x1, c1 = routes.solve(make("hinge", (601, 256)), "f32", "1", max_iterations=30)
    assert_route(c, st, (601, 256))
    rs.assert_same_bytes(st, x, st1, x1)


# ---- 6. batch ---------------------------------------------------------------------------------------
def test_batch_members_are_their_own_solves(solve_mod):
    """three tall hinge members on one C: the route has no batched form, every member is solved
    by itself on it and returns its own solve bit for bit"""
    m, n = 601, 256
    scale = np.abs(problems.hinge_l1(m, n)[1]["C"].sum(axis=0)).max()
    probs = [problems.hinge_l1(m, n, lam=f * scale)[0] for f in (0.05, 0.02, 0.01)]
    pbs, data = [p.SerializeToString() for p in probs], rs.union_data(probs)
    sb = wire.SolverParams(max_iterations=60).SerializeToString()
    with rs.options(solve_mod, **ON):
        batch, tags = rs.profiled(solve_mod, lambda: solve_mod.solve_batch(pbs, None, sb, data))
        single = [solve_mod.solve(pb, [], sb, data) for pb in pbs]
    cb = rs.base_counts(tags)
    assert cb.get("zero_tall", 0) == cb.get("zero_tall_cols", 0) == sum(rs.sweeps(st) for st, _ in batch), cb
    assert not [t for t in cb if t.startswith("batch_zero")], sorted(cb)
    assert len(batch) == len(single) == 3
    rs.assert_identical(batch, single)
