"""A linear term on x and the non-negative cone on z on the fused ZERO-term routes (DESIGN.md 3.11 "A
linear term on x, a cone on z", option "fused_zero_lp"): linear programs in graph form (problems.lp,
seed 0: affine(c^T x) + non_negative(s), s = b - A x) run on the fat route (tags "zero_fused",
"zero_fused_rows") and on the tall one (tags "zero_tall", "zero_tall_cols") with the two new heads in
the thresholds' places.  The heads are per side, so the same option carries the polyhedron problems
(problems.polyhedron: ||x||_1 or lam ||x||_2^2 over A x <= b, the cone with the old x heads) and a
linear cost with a hinge or logistic loss (the linear term with the old z heads).  Every solve here sets
"fused_zero_lp" (to "1" unless it says otherwise) and puts "0", the library's default, back; with it
"fused_zero_ridge" and "fused_zero_check", put back to "auto" and "0"; route_support's scope sets the
other options, the tall ones to "1".

Tolerances are the project's own: against the oracle rs.TOLERANCES (f64 rtol 1e-6, atol 1e-8; f32
rtol = atol = 5e-3, equal state and stopping sweep); fused against generic in f64 the bound of the
other ZERO-route tests, 1e-9 of the largest magnitude.

Shapes.  Fat: (256, 601) the row floor; (260, 601) rows past a wave boundary.  Tall: (601, 256) the
column floor, odd m; (603, 260) columns past a wave boundary; (2051, 1028) a second, ragged chunk per
thread and the tile-packed symmetric apply.

Fixed sweeps, on the CPU oracle (entries of var:s that are zero / positive): tall lp after 60 sweeps
258 / 343 at (601, 256) and 258 / 345 at (603, 260), so both branches of the cone in the pass decide
entries.  Fat lp converges to s = 0 within 20 sweeps (256 of 256 zero at 60), so it is compared after 5
sweeps: 253 / 3 at (256, 601), 256 / 4 at (260, 601).  The polyhedron problems cover the cone in the
rows after 60 sweeps: l1 135 / 121 and ridge 130 / 126 at (256, 601).

Stopping rule, on the CPU oracle: lp stops OPTIMAL at the check of iteration 40 on all three tall
shapes; r / eps_pri at the stop: 0.914 at (601, 256), 0.809 at (603, 260), 0.710 at (2051, 1028), after
1.286, 1.133 and 1.068 at the check of iteration 30 as oracle_checks below reads them (1.345, 1.192 and
1.108 were noted when the cells were chosen); s / eps_dual < 0.08 at both checks.  (603, 260) and (2051, 1028) run in both types, (601, 256) in f64 alone: its 0.914 does not
carry f32 rounding by the margin the project has used.  With the route's own check
(test_the_one_launch_check_...) the same two tall cells, and fat lp (256, 601), which stops at the check
of iteration 10 with both ratios below 1e-3 after 99 and 5.6 at the check of iteration 0."""

import contextlib
import os

import numpy as np
import pytest
import scipy.sparse as sp

from epsilon_amd import ir, problems, wire
from epsilon_amd.wire import ProxFunction
from oracle import epsilon_oracle as orc
from tests import route_support as rs

pytestmark = pytest.mark.gpu

FAT = [(256, 601), (260, 601)]
TALL = [(601, 256), (603, 260), (2051, 1028)]
FIXED = dict(max_iterations=60, abs_tol=0.0, rel_tol=0.0)
FIXED5 = dict(max_iterations=5, abs_tol=0.0, rel_tol=0.0)
VARIABLES = ["separate:var:s:zero", "separate:var:x:zero", "var:s", "var:x"]
# routes.solve(prob, dtype, lp, ridge, check, **options by name, **solver params)
ROUTE_OPTIONS = (("tall", "fused_zero_tall", "1"), ("tall_smooth", "fused_zero_tall_smooth", "1"),
                 ("fused", "fused", "1"), ("fused_zero", "fused_zero", "auto"))
ON = rs.switched_on(ROUTE_OPTIONS)  # what the handles and the batches set beside this module's own options


def is_tall(shape):
    return shape[0] > shape[1]


# ---- the options of this module: route_support's scope has no row for them ---------------------------
@contextlib.contextmanager
def lp_option(mod, value, ridge="auto", check="0"):
    """"fused_zero_lp" = value for the block (None: the variable unset), "fused_zero_ridge" and
    "fused_zero_check" with it; "0", "auto" and "0", the library's defaults, on every way out"""
    try:
        mod.set_option("fused_zero_ridge", ridge)
        mod.set_option("fused_zero_check", check)
        if value is None:
            mod.set_option("fused_zero_lp", "0")
            os.unsetenv("EPSILON_HIP_FUSED_ZERO_LP")  # (the library reads the process environment)
        else:
            mod.set_option("fused_zero_lp", value)
        yield
    finally:
        mod.set_option("fused_zero_lp", "0")
        mod.set_option("fused_zero_check", "0")
        mod.set_option("fused_zero_ridge", "auto")


class Routes(rs.Routes):
    def solve(self, prob, dtype="f32", lp="1", ridge="auto", check="0", **params):
        with lp_option(self.mod, lp, ridge, check):
            return super(Routes, self).solve(prob, dtype, **params)


@pytest.fixture
def routes(solve_mod):
    return Routes(solve_mod, ROUTE_OPTIONS)


def lp_of(A, b, c, c_map=ir.dense_matrix):
    """problems.lp's graph form on given data; `c_map`: how the 1 x n map of the cost is stored"""
    def terms(x, s):
        return [ir.prox(ProxFunction.AFFINE, ir.linear_map(c_map(c.reshape(1, -1)), x)),
                ir.prox(ProxFunction.NON_NEGATIVE, s)]
    return problems._graph_form(terms, -A, b, z_key="var:s")


def sparse_cost(m, n):
    """lp with the cost's 1 x n argument map stored as a sparse matrix: not one dense row"""
    info = problems.lp(m, n)[1]
    return lp_of(info["A"], info["b"], info["c"], c_map=lambda c: ir.sparse_matrix(sp.csr_matrix(c)))


def linear_with_loss(loss):
    """a linear cost on x with a hinge or logistic loss on z = C x, C of problems.hinge_l1: the linear
    head with an old z head.  (Whether it is bounded is not asked: fixed sweeps are compared.)"""
    def build(m, n):
        C = problems.hinge_l1(m, n)[1]["C"]
        c = -C.T.dot(np.random.RandomState(5).rand(m)) / m

        def terms(x, z):
            if loss == "hinge":
                arg = ir.add(ir.linear_map(ir.scalar(-1, m), z), ir.scalar_constant(1.0, (m, 1)))
                fz = ir.prox(ProxFunction.SUM_HINGE, arg)
            else:
                fz = ir.prox(ProxFunction.SUM_LOGISTIC, z, alpha=1.0)
            return [fz, ir.prox(ProxFunction.AFFINE, ir.linear_map(ir.dense_matrix(c.reshape(1, -1)), x))]
        return problems._graph_form(terms, C, None)
    return build


def second_lp(m, n):
    """lp(m, n) with another right-hand side on the same A and c"""
    info = problems.lp(m, n)[1]
    return lp_of(info["A"], info["b"] + np.random.RandomState(7).rand(m), info["c"])


make = rs.memoised({
    "lp": lambda m, n: problems.lp(m, n)[0],
    "lp_b2": second_lp,
    "poly_l1": lambda m, n: problems.polyhedron(m, n, norm="l1")[0],
    "poly_l2": lambda m, n: problems.polyhedron(m, n, norm="l2")[0],
    "lin_hinge": linear_with_loss("hinge"),
    "lin_logistic": linear_with_loss("logistic"),
    "sparse_cost": sparse_cost,
    "hinge_l1": lambda m, n: problems.hinge_l1(m, n, lam=0.01 * rs.lam_scale("hinge_l1", m, n))[0],
})
oracle = rs.oracle_of(make)


def zero_tags(c):
    return sorted(t for t in c if t.startswith(("zero_", "batch_zero")))


def sweep_tags(kind, shape):
    if not is_tall(shape):
        return ("zero_fused", "zero_fused_rows")
    if kind == "lin_logistic":
        return ("zero_tall_dot", "zero_tall_samples", "zero_tall_acc", "zero_tall_cols")
    return ("zero_tall", "zero_tall_cols")


def assert_route(c, st, kind, shape, norms=None):
    """one launch of every kernel of the route per sweep, nothing generic in their place, nothing of the
    other route, of the lasso route or of a batch; `norms`: that many launches of the route's own check;
    the packed symmetric apply from a pivot of order 1024"""
    n = rs.sweeps(st)
    want = {t: n for t in sweep_tags(kind, shape)}
    if norms:
        want["zero_tall_norms" if is_tall(shape) else "zero_fused_norms"] = norms
    # (the first head of a smooth term, "zero_fused_head" / "zero_tall_head", belongs to Init)
    got = {t: c[t] for t in zero_tags(c) if not t.endswith("_head")}
    assert got == want, (got, want)
    assert "lasso_fused" not in c and not [t for t in c if t.startswith("batch_")], sorted(c)
    if min(shape) >= 1024:
        assert c.get("symv_packed", 0) >= n, sorted(c)


def assert_generic(c):
    assert not zero_tags(c) and "lasso_fused" not in c, sorted(c)


# ---- 1. route tags --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FAT + TALL)
def test_lp_takes_the_route_with_the_option(routes, shape):
    st, x, c = routes.solve(make("lp", shape), "f32", "1", max_iterations=30)
    assert_route(c, st, "lp", shape)
    assert sorted(x) == VARIABLES


@pytest.mark.parametrize("lp", [None, "0"])
@pytest.mark.parametrize("shape", [(256, 601), (601, 256)])
def test_the_default_is_the_generic_path(routes, shape, lp):
    """the variable unset, and "0": no ZERO launch, and the bytes of the solve with every fused route off"""
    prob = make("lp", shape)
    st, x, c = routes.solve(prob, "f32", lp, max_iterations=30)
    st0, x0, c0 = routes.solve(prob, "f32", lp, fused="0", max_iterations=30)
    assert_generic(c)
    assert_generic(c0)
    rs.assert_same_bytes(st, x, st0, x0)


# ---- 2. fixed sweeps, every variable against the oracle ------------------------------------------------
def assert_both_branches(kind, shape, xo):
    """on the oracle's result alone: var:s has entries on the cone's boundary and inside it, so both
    branches of max(., 0) decide entries of the iterate, and x is not zero"""
    s = xo["var:s"]
    cls = [int((s == 0).sum()), int((s > 0).sum())]
    print(kind, shape, "s == 0, s > 0 on", cls, "rows")
    assert all(v > 0 for v in cls) and not (s < 0).any()
    assert np.abs(xo["var:x"]).max() > 0.1


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kind,shape,params", (
    [("lp", shape, FIXED) for shape in TALL] + [("lp", shape, FIXED5) for shape in FAT] +
    [(kind, shape, FIXED) for kind in ("poly_l1", "poly_l2") for shape in (FAT[0], TALL[1])]))
def test_fixed_sweeps_match_the_oracle(routes, kind, shape, params, dtype):
    so, xo = oracle(kind, shape, **params)
    assert so.state == wire.SolverStatus.MAX_ITERATIONS_REACHED and so.num_iterations == params["max_iterations"]
    assert sorted(xo) == VARIABLES
    assert_both_branches(kind, shape, xo)
    st, x, c = routes.solve(make(kind, shape), dtype, **params)
    assert_route(c, st, kind, shape)
    rs.assert_matches_oracle(st, x, so, xo, dtype)


# ---- 3. default stopping rule on tall C ----------------------------------------------------------------
_checks = {}


def oracle_checks(kind, shape):
    """the oracle's solve under the default stopping rule with r / eps_pri and s / eps_dual at every
    check: (decoded status, arrays, {iteration: (r ratio, s ratio)})"""
    if (kind, shape) not in _checks:
        prob, ratios = make(kind, shape), {}

        def at_check(it, solver):
            if it % solver.params.epoch_iterations == 0:
                solver.compute_residuals()
                r = solver.status.residuals
                ratios[it] = (r.r_norm / r.epsilon_primal, r.s_norm / r.epsilon_dual)
        st, x = orc.solve(prob.SerializeToString(), [], wire.SolverParams().SerializeToString(),
                          prob.expression_data(), trace=at_check)
        _checks[kind, shape] = (rs.status(st), rs.arrays(x), ratios)
    return _checks[kind, shape]


@pytest.mark.parametrize("shape,dtype", [((603, 260), "f32"), ((603, 260), "f64"), ((2051, 1028), "f32"),
                                         ((2051, 1028), "f64"), ((601, 256), "f64")])
def test_stops_with_the_oracle(routes, shape, dtype):
    so, xo, ratios = oracle_checks("lp", shape)
    assert so.state == wire.SolverStatus.OPTIMAL and so.num_iterations == 40
    (r0, s0), (r1, s1) = ratios[30], ratios[40]
    print("oracle: r / eps_pri %.3f then %.3f, s / eps_dual %.3f then %.3f" % (r0, r1, s0, s1))
    # the primal residual decides; the f32 cells are at least 6 % away from the threshold on either side
    assert r0 > 1.0 > r1 and max(s0, s1) < 0.08
    if dtype == "f32":
        assert r0 >= 1.06 and r1 <= 0.9
    st, x, c = routes.solve(make("lp", shape), dtype)
    assert_route(c, st, "lp", shape)
    rs.assert_matches_oracle(st, x, so, xo, dtype)


# ---- 4. fused against generic, f64 ----------------------------------------------------------------------
def assert_equal_to_rounding(x, x0):
    """every variable within 1e-9 of its largest magnitude on the generic path, the bound of the other
    ZERO-route tests.  A variable that has itself converged to zero gives no scale: fat lp ends at s = 0
    (exactly, in var:s), and the copy s' = v_s - e w is then the rounding of the O(1) terms it is the
    difference of - 4.4e-15 on the generic path, 6.8e-15 fused at (260, 601).  Such a variable - largest
    magnitude below 1e-9 of the solve's own, the resolution of the bound - is held to 1e-9 of the largest
    magnitude among the solve's variables instead."""
    solve_scale = max(np.abs(v).max() for v in x0.values())
    for k in x0:
        diff, ref = np.abs(x[k] - x0[k]).max(), np.abs(x0[k]).max()
        print(k, "max |fused - generic| %.3g, max |generic| %.3g (the solve's %.3g)" % (diff, ref, solve_scale))
    for k in x0:
        ref = np.abs(x0[k]).max()
        scale = ref if ref >= 1e-9 * solve_scale else solve_scale
        assert np.abs(x[k] - x0[k]).max() <= 1e-9 * scale, k


@pytest.mark.parametrize("kind,shape", [(kind, shape) for kind in ("lp", "poly_l1", "poly_l2")
                                        for shape in ((260, 601), (603, 260))])
def test_fused_equals_generic_to_rounding_f64(routes, kind, shape):
    prob = make(kind, shape)
    st, x, c = routes.solve(prob, "f64", "1", **FIXED)
    st0, x0, c0 = routes.solve(prob, "f64", "0", **FIXED)
    assert_route(c, st, kind, shape)
    assert_generic(c0)
    assert rs.status(st).num_iterations == rs.status(st0).num_iterations == 60
    assert sorted(x) == sorted(x0) == VARIABLES
    assert_equal_to_rounding(x, x0)


# ---- 5. the heads are independent -----------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(256, 601), (601, 256)])
@pytest.mark.parametrize("kind", ["poly_l1", "poly_l2"])
def test_the_cone_runs_with_the_old_x_heads(routes, kind, shape):
    prob = make(kind, shape)
    st, x, c = routes.solve(prob, "f32", "1", "1", max_iterations=30)
    assert_route(c, st, kind, shape)
    # the ridge term beside the cone is the ridge option's: with "0" the l2 problem stays generic
    st0, x0, c0 = routes.solve(prob, "f32", "1", "0", max_iterations=30)
    if kind == "poly_l2":
        assert_generic(c0)
    else:
        assert_route(c0, st0, kind, shape)
        rs.assert_same_bytes(st, x, st0, x0)
    # and without the cone's option either stays generic
    st0, x0, c0 = routes.solve(prob, "f32", "0", "1", max_iterations=30)
    assert_generic(c0)


@pytest.mark.parametrize("shape", [(256, 601), (601, 256)])
@pytest.mark.parametrize("kind", ["lin_hinge", "lin_logistic"])
def test_the_linear_term_runs_with_the_old_z_heads(routes, kind, shape):
    """a linear cost with a hinge loss (a zone on z) and with a logistic loss (a smooth term: the carried
    head fat, the sample kernel tall): on the route, and the generic path's iterate to rounding"""
    prob = make(kind, shape)
    st, x, c = routes.solve(prob, "f64", "1", **FIXED)
    st0, x0, c0 = routes.solve(prob, "f64", "0", **FIXED)
    assert_route(c, st, kind, shape)
    assert_generic(c0)
    assert rs.status(st).num_iterations == rs.status(st0).num_iterations == 60
    assert sorted(x) == sorted(x0) and len(x0) == 4
    for k in x0:
        diff, ref = np.abs(x[k] - x0[k]).max(), np.abs(x0[k]).max()
        print(k, "max |fused - generic| %.3g, max |generic| %.3g" % (diff, ref))
    for k in x0:
        assert np.abs(x0[k]).max() > 0
        assert np.abs(x[k] - x0[k]).max() <= 1e-9 * np.abs(x0[k]).max(), k


def test_l1_problems_are_untouched(routes):
    for shape in ((601, 256), (256, 601)):
        prob = make("hinge_l1", shape)
        st0, x0, c0 = routes.solve(prob, "f32", "0", max_iterations=30)
        st1, x1, c1 = routes.solve(prob, "f32", "1", max_iterations=30)
        assert c0.get("zero_tall" if is_tall(shape) else "zero_fused", 0) == rs.sweeps(st0), sorted(c0)
        assert c0 == c1, (c0, c1)
        rs.assert_same_bytes(st1, x1, st0, x0)


# ---- 6. what keeps the generic path with the option on -------------------------------------------------
@pytest.mark.parametrize("kind,shape,options", [
    ("lp", (601, 256), {"solver": 1}),              # two-block driver
    ("lp", (256, 601), {"solver": 1}),
    ("lp", (601, 256), {"fused_zero": "0"}),        # the ZERO-term routes switched off
    ("lp", (256, 601), {"fused_zero": "0"}),
    ("lp", (601, 256), {"fused": "0"}),             # the fused routes switched off altogether
    ("lp", (256, 601), {"fused": "0"}),
    ("lp", (601, 256), {"tall": "0"}),              # the tall route switched off
    ("lp", (600, 252), {}),                         # below the column floor
    ("lp", (252, 601), {}),                         # below the row floor
    ("sparse_cost", (601, 256), {}),                # an AFFINE term whose argument map is not one dense row
    ("sparse_cost", (256, 601), {}),
])
def test_fall_backs_are_the_generic_path(routes, kind, shape, options):
    prob = make(kind, shape)
    params = dict(max_iterations=30, **options)
    st, x, c = routes.solve(prob, "f32", "1", **params)
    st0, x0, c0 = routes.solve(prob, "f32", "0", **params)
    assert_generic(c)
    assert_generic(c0)
    rs.assert_same_bytes(st, x, st0, x0)


# ---- 7. sweep boundaries and warm start -----------------------------------------------------------------
BOUNDARY = [("lp", (601, 256)), ("poly_l1", (256, 601))]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kind,shape", BOUNDARY)
def test_a_solve_can_stop_after_any_sweep(solve_mod, kind, shape, dtype):
    prob = make(kind, shape)
    params = dict(max_iterations=1000, abs_tol=0.0, rel_tol=0.0)
    with lp_option(solve_mod, "1"):
        st_a, xa, ca = rs.run_handle(solve_mod, prob, dtype, [30], ON, **params)
        st_b, xb, cb = rs.run_handle(solve_mod, prob, dtype, [1, 9, 20], ON, **params)
    for tag in sweep_tags(kind, shape):
        assert ca.get(tag) == cb.get(tag) == 30, (tag, ca.get(tag), cb.get(tag))
    assert sorted(xa) == VARIABLES
    rs.assert_same_arrays(xa, xb)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kind,shape", BOUNDARY)
def test_warm_start_takes_the_state_over(solve_mod, kind, shape, dtype):
    """two solves of 30 sweeps on one handle, the second warm-started, against the oracle doing
    the same on one solver object"""
    prob = make(kind, shape)
    sp_ = wire.SolverParams(warm_start=True, max_iterations=30, abs_tol=0.0, rel_tol=0.0)
    pb, data = prob.SerializeToString(), prob.expression_data()
    with lp_option(solve_mod, "1"), rs.handle(solve_mod, prob, dtype, sp_, **ON) as s:
        s.init()
        s.run(-1)
        s.init()
        s.run(-1)
        c = rs.base_counts(solve_mod.profile_dump())
        st, x = s.result()
    for tag in sweep_tags(kind, shape):
        assert c.get(tag) == 60, (tag, c.get(tag))
    osolver = orc.create_solver(wire.Problem.FromString(pb), dict(data), sp_)
    osolver.solve()
    xo = osolver.solve()
    assert rs.status(st).num_iterations == osolver.status.num_iterations == 30
    x = rs.arrays(x)
    xw = {k: np.asarray(xo(k), dtype=np.float64).ravel() for k in x}
    # on the oracle alone: the second solve went on from the first - in some variable its iterate is
    # off the cold solve's by more than twice what the f32 tolerances allow, so a route that dropped
    # the state would not pass
    cold = oracle(kind, shape, max_iterations=30, abs_tol=0.0, rel_tol=0.0)[1]
    tol = rs.TOLERANCES["f32"]
    room = max(np.abs(xw[k] - cold[k]).max() / (tol["atol"] + tol["rtol"] * np.abs(cold[k]).max()) for k in cold)
    print("oracle: max |warm - cold| is %.3g x the f32 tolerance" % room)
    assert room > 2.0
    rs.assert_close(x, xw, dtype)


# ---- 8. the route's own residual check -------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kind,shape", [("lp", (603, 260)), ("lp", (2051, 1028)), ("lp", (256, 601))])
def test_the_one_launch_check_stops_where_the_generic_one_does(routes, kind, shape, dtype):
    """"fused_zero_check" = "1": the same stopping sweep and the same bytes as with the generic check (the
    check writes no state), one launch per check under the route's own tag"""
    prob = make(kind, shape)
    st, x, c = routes.solve(prob, dtype, "1", "auto", "1", max_iterations=200)
    st0, x0, c0 = routes.solve(prob, dtype, "1", "auto", "0", max_iterations=200)
    sg = rs.status(st)
    print(kind, shape, dtype, "state %d at %d" % (sg.state, sg.num_iterations))
    assert sg.state == wire.SolverStatus.OPTIMAL
    tag = "zero_tall_norms" if is_tall(shape) else "zero_fused_norms"
    assert c.get(tag, 0) >= sg.num_iterations // 10 + 1 and tag not in c0, (c.get(tag), sorted(c0))
    assert_route(c0, st0, kind, shape)
    # the sweeps behind the stopping check are enqueued before it is read and dropped after it
    for t in sweep_tags(kind, shape):
        assert c.get(t, 0) >= rs.sweeps(st), (t, c.get(t))
    rs.assert_same_bytes(st, x, st0, x0)


# ---- 9. batch --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(601, 256), (256, 601)])
def test_batch_members_are_their_own_solves(solve_mod, shape):
    """two lp members on one matrix (different b): the batched kernels have neither head, so every
    member is solved by itself on its route and returns its own solve bit for bit"""
    probs = [make("lp", shape), make("lp_b2", shape)]
    with lp_option(solve_mod, "1"):
        batch, tagsb, single, _ = rs.run_both(solve_mod, probs, "f32", dict(ON, batch_zero_tall="1"),
                                              max_iterations=60)
    cb = rs.base_counts(tagsb)
    total = sum(rs.sweeps(st) for st, _ in batch)
    for tag in sweep_tags("lp", shape):
        assert cb.get(tag, 0) == total, (tag, cb.get(tag), total)
    assert not [t for t in cb if t.startswith("batch_")], sorted(cb)
    assert len(batch) == len(single) == 2
    rs.assert_identical(batch, single)
