"""l1-regularised logistic regression with tall C on the fused sweep of ZERO-term problems
(DESIGN.md 3.11 "Tall C", option "fused_zero_tall_smooth"): problems.logreg_l1 with more rows than
columns, seed 0, runs as five launches per sweep - the dot products over a transposed copy of the
data matrix (tag "zero_tall_dot"), one kernel over the samples with the logistic prox in it (tag
"zero_tall_samples"), the forward product over the same copy (tag "zero_tall_acc"), the x side (tag
"zero_tall_cols") and the apply of the cached n x n inverse.  Every solve here sets
"fused_zero_tall_smooth" (and "fused_zero_tall" = "1") for one call and puts "auto" back.

Tolerances are the project's own: against the oracle f64 rtol 1e-6, atol 1e-8; f32 rtol = atol =
5e-3, equal state and stopping sweep; fused against generic in f64 1e-9 of the largest magnitude.

Shapes: (601, 256) the column floor, 64 live threads of the passes, odd m with a trailing unpaired
streamed column, a last workgroup of 89 samples in the sample kernel; (603, 260) columns past a wave
boundary; (2051, 1028) a second, ragged chunk per thread, several pairs per workgroup and the
tile-packed symmetric apply of the inverse.

Oracle facts the tests rest on (asserted where they are used).  After 60 sweeps x has entries of
both signs and zeros and |z| spans the bend of the logistic loss and its tails (the table in
test_sixty_sweeps_match_the_oracle).  Default stopping rule, r / eps_pri at the stopping check and at
the check before: (603, 260) stops at 60 with 0.930 after 1.150 - a margin f32 rounding cannot
cross; (601, 256) at 70 with 0.829 after 1.0245 and (2051, 1028) at 120 with 0.965 after 1.060: f64
alone; s / eps_dual at most 0.30 in all three."""

import numpy as np
import pytest

from epsilon_amd import problems, wire
from oracle import epsilon_oracle as orc
from tests import route_support as rs

pytestmark = pytest.mark.gpu

SHAPES = [(601, 256), (603, 260), (2051, 1028)]
FIXED = dict(max_iterations=60, abs_tol=0.0, rel_tol=0.0)
KEYS = ["separate:var:x:zero", "separate:var:z:zero", "var:x", "var:z"]
SMOOTH_TAGS = ["zero_tall_dot", "zero_tall_samples", "zero_tall_acc", "zero_tall_cols"]
# routes.solve(prob, dtype, smooth, tall, fused, fused_zero, **solver params): the options of a solve
ROUTE_OPTIONS = (("smooth", "fused_zero_tall_smooth", "1"), ("tall", "fused_zero_tall", "1"),
                 ("fused", "fused", "1"), ("fused_zero", "fused_zero", "auto"))
ON = rs.switched_on(ROUTE_OPTIONS)  # the two tall options = "1": what the handles and the batch set


def route_tags(c):
    return sorted(t for t in c if t.startswith("zero_tall") or t.startswith("zero_fused"))


@pytest.fixture
def routes(solve_mod):
    return rs.Routes(solve_mod, ROUTE_OPTIONS)


# kind "default": the default lambda, 0.1 max|C^T 1/2|; "small": a tenth of it; "hinge":
# problems.hinge_l1 with lambda = 0.01 max|sum_i C_i|
make = rs.memoised({
    "default": lambda m, n: problems.logreg_l1(m, n)[0],
    "small": lambda m, n: problems.logreg_l1(m, n, lam=0.01 * rs.lam_scale("logreg_l1", m, n))[0],
    "hinge": lambda m, n: problems.hinge_l1(m, n, lam=0.01 * rs.lam_scale("hinge_l1", m, n))[0],
})
oracle = rs.oracle_of(make)


def assert_route_counts(c, count, shape):
    """the five launches, `count` times each (the checks are not pipelined: nothing is discarded);
    no launch of the one-pass tall form, of the fat route or of the lasso route; the packed symmetric
    apply from 1024 columns"""
    for t in SMOOTH_TAGS:
        assert c.get(t, 0) == count, (t, c.get(t), count, route_tags(c))
    assert "zero_tall" not in c, route_tags(c)
    assert not [t for t in c if t.startswith("zero_fused")], route_tags(c)
    assert "lasso_fused" not in c
    if shape[1] >= 1024:
        assert c.get("symv_packed", 0) >= count, sorted(c)


def assert_route(c, st, shape):
    assert_route_counts(c, rs.sweeps(st), shape)


def assert_generic(c):
    assert not route_tags(c), route_tags(c)


# ---- 1. fixed 60 sweeps, every variable against the oracle -----------------------------------------
# the oracle's 60-sweep iterate: entries of x above, below and at zero, the range of |z|
SIXTY = {
    ((601, 256), "default"): (26, 20, 210, 0.004, 8.9),
    ((601, 256), "small"): (103, 112, 41, 0.06, 14.0),
    ((603, 260), "default"): (24, 29, 207, 0.03, 7.9),
    ((603, 260), "small"): (111, 100, 49, 0.47, 11.6),
    ((2051, 1028), "default"): (5, 6, 1017, 0.03, 11.8),
    ((2051, 1028), "small"): (304, 318, 406, 0.43, 14.3),
}


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", ["default", "small"])
def test_sixty_sweeps_match_the_oracle(routes, kind, shape, dtype):
    so, xo = oracle(kind, shape, **FIXED)
    assert so.state == wire.SolverStatus.MAX_ITERATIONS_REACHED and so.num_iterations == 60
    assert sorted(xo) == KEYS
    x, z = xo["var:x"], np.abs(xo["var:z"])
    print(kind, "x > 0:", int((x > 0).sum()), "x < 0:", int((x < 0).sum()), "x = 0:", int((x == 0).sum()),
          "|z| in [%.3g, %.3g]" % (z.min(), z.max()))
    pos, neg, zero, zlo, zhi = SIXTY[(shape, kind)]
    assert ((x > 0).sum(), (x < 0).sum(), (x == 0).sum()) == (pos, neg, zero)
    assert pos > 0 and neg > 0 and zero > 0
    assert z.min() < 3 and z.max() > 4.5  # rows on the bend of the logistic loss and far out in its tails
    assert abs(z.min() - zlo) <= 0.1 * zlo + 0.005 and abs(z.max() - zhi) <= 0.01 * zhi
    st, x, c = routes.solve(make(kind, shape), dtype, **FIXED)
    assert_route(c, st, shape)
    rs.assert_matches_oracle(st, x, so, xo, dtype)


# ---- 2. default stopping rule -------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dtype,stop,ratio", [
    ((603, 260), "f32", 60, 0.930),
    ((603, 260), "f64", 60, 0.930),
    ((601, 256), "f64", 70, 0.829),
    ((2051, 1028), "f64", 120, 0.965),
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
    shape = (603, 260)
    prob = make("default", shape)
    st, x, c = routes.solve(prob, "f64", "1", **FIXED)
    st0, x0, c0 = routes.solve(prob, "f64", "0", **FIXED)
    assert_route(c, st, shape)
    assert_generic(c0)
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
    """the head the sample kernel carries from one sweep to the next survives the end of a run call"""
    shape = (601, 256)
    prob = make("default", shape)
    params = dict(max_iterations=1000, abs_tol=0.0, rel_tol=0.0)
    st_a, xa, ca = rs.run_handle(solve_mod, prob, dtype, [30], ON, **params)
    st_b, xb, cb = rs.run_handle(solve_mod, prob, dtype, [1, 7, 22], ON, **params)
    assert_route_counts(ca, 30, shape)
    assert_route_counts(cb, 30, shape)
    assert sorted(xa) == sorted(xb) == KEYS
    rs.assert_same_arrays(xa, xb)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_warm_start_takes_the_state_over(solve_mod, dtype):
    """two solves of 30 sweeps on one handle, the second warm-started, against the oracle doing
    the same on one solver object: the first head of the second solve comes from the adopted state"""
    shape = (601, 256)
    prob = make("default", shape)
    sp = wire.SolverParams(warm_start=True, max_iterations=30, abs_tol=0.0, rel_tol=0.0)
    with rs.handle(solve_mod, prob, dtype, sp, **ON) as s:
        s.init()
        s.run(-1)
        s.init()
        s.run(-1)
        c = rs.base_counts(solve_mod.profile_dump())
        st, x = s.result()
    assert_route_counts(c, 60, shape)
    osolver = orc.create_solver(wire.Problem.FromString(prob.SerializeToString()), dict(prob.expression_data()), sp)
    osolver.solve()
    xo = osolver.solve()
    assert rs.status(st).num_iterations == osolver.status.num_iterations == 30
    x = rs.arrays(x)
    xo = {k: np.asarray(xo(k), dtype=np.float64).ravel() for k in x}
    # the second solve went on from the first: in the oracle it is not the cold solve's iterate,
    # by far more than the tolerances (1.84 in z)
    cold = oracle("default", shape, max_iterations=30, abs_tol=0.0, rel_tol=0.0)[1]
    print("oracle: max |warm - cold| in z %.3g" % np.abs(xo["var:z"] - cold["var:z"]).max())
    assert np.abs(xo["var:z"] - cold["var:z"]).max() > 0.1
    rs.assert_close(x, xo, dtype)


# ---- 5. determinism ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_two_solves_return_the_same_bytes(routes, dtype):
    shape = (2051, 1028)
    prob = make("default", shape)
    st1, x1, c1 = routes.solve(prob, dtype, **FIXED)
    st2, x2, c2 = routes.solve(prob, dtype, **FIXED)
    assert_route(c1, st1, shape)
    assert_route(c2, st2, shape)
    assert sorted(x1) == sorted(x2) == KEYS
    rs.assert_same_arrays(x1, x2)


# ---- 6. what keeps the generic path ---------------------------------------------------------------------
@pytest.mark.parametrize("shape,smooth,tall,fused,fused_zero,params", [
    ((601, 256), "auto", "1", "1", "auto", {}),          # the default at the column floor
    ((601, 256), "0", "1", "1", "auto", {}),
    ((601, 256), "1", "0", "1", "auto", {}),             # the tall route switched off
    ((601, 256), "1", "1", "1", "0", {}),                # the ZERO-term routes switched off
    ((601, 256), "1", "1", "0", "auto", {}),             # the fused routes switched off altogether
    ((601, 256), "1", "1", "1", "auto", {"solver": 1}),  # two-block driver
    ((600, 252), "1", "1", "1", "auto", {}),             # below the column floor
    ((601, 258), "1", "1", "1", "auto", {}),             # columns not a multiple of 4
])
def test_fall_backs_are_the_generic_path(routes, shape, smooth, tall, fused, fused_zero, params):
    prob = make("default", shape)
    params = dict(max_iterations=30, **params)
    st, x, c = routes.solve(prob, "f32", smooth, tall, fused, fused_zero, **params)
    st0, x0, c0 = routes.solve(prob, "f32", "0", "1", "1", "auto", **params)
    assert_generic(c)
    assert_generic(c0)
    rs.assert_same_bytes(st, x, st0, x0)


def test_the_option_leaves_tall_hinge_alone(routes):
    """a zone on z keeps the one-pass tall form and its bytes whatever the option says"""
    prob = make("hinge", (601, 256))
    st1, x1, c1 = routes.solve(prob, "f32", "1", max_iterations=30)
    st0, x0, c0 = routes.solve(prob, "f32", "0", max_iterations=30)
    for c, st in ((c1, st1), (c0, st0)):
        assert c.get("zero_tall", 0) == c.get("zero_tall_cols", 0) == rs.sweeps(st), route_tags(c)
        assert route_tags(c) == ["zero_tall", "zero_tall_cols"]
    rs.assert_same_bytes(st1, x1, st0, x0)


def test_auto_takes_the_route_from_the_measured_floor(routes):
    """the 4n x n ladder has the fused sweep ahead from n = 512, so "auto" takes the
    route there as "1" does; at the column floor it keeps the generic path (the first fall-back)"""
    shape = (2051, 1028)
    st, x, c = routes.solve(make("default", shape), "f32", "auto", max_iterations=30)
    st1, x1, c1 = routes.solve(make("default", shape), "f32", "1", max_iterations=30)
    assert_route(c, st, shape)
    assert_route(c1, st1, shape)
    rs.assert_same_bytes(st, x, st1, x1)


# ---- 7. batch ---------------------------------------------------------------------------------------
def test_batch_members_are_their_own_solves(solve_mod):
    """three tall logistic members on one C: the route has no batched form, every member is solved
    by itself on it and returns its own solve bit for bit"""
    m, n = 601, 256
    scale = np.abs(problems.logreg_l1(m, n)[1]["C"].T.dot(np.full(m, 0.5))).max()
    probs = [problems.logreg_l1(m, n, lam=f * scale)[0] for f in (0.1, 0.05, 0.02)]
    pbs, data = [p.SerializeToString() for p in probs], rs.union_data(probs)
    sb = wire.SolverParams(max_iterations=60).SerializeToString()
    # in the oracle the second member stops by the rule at 40, the other two run into the cap
    ost = [rs.status(orc.solve(pb, [], sb, data)[0]) for pb in pbs]
    assert [(s.state, s.num_iterations) for s in ost] == [
        (wire.SolverStatus.MAX_ITERATIONS_REACHED, 60), (wire.SolverStatus.OPTIMAL, 40),
        (wire.SolverStatus.MAX_ITERATIONS_REACHED, 60)]
    with rs.options(solve_mod, **ON):
        batch, tags = rs.profiled(solve_mod, lambda: solve_mod.solve_batch(pbs, None, sb, data))
        single = [solve_mod.solve(pb, [], sb, data) for pb in pbs]
    cb = rs.base_counts(tags)
    assert_route_counts(cb, sum(rs.sweeps(st) for st, _ in batch), (m, n))
    assert not [t for t in cb if t.startswith("batch_zero")], sorted(cb)
    assert len(batch) == len(single) == 3
    rs.assert_identical(batch, single)
