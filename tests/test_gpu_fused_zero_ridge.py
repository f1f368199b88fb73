"""A ridge term on x on the fused ZERO-term routes (DESIGN.md 3.11 "A ridge term on x", option
"fused_zero_ridge"): the hinge, deadzone and logistic losses with lam ||x||_2^2 in graph form
(problems.hinge_l2, svr_l2, logreg_l2, seed 0) run on the fat route (tags "zero_fused",
"zero_fused_rows") and on the tall one (tags "zero_tall", "zero_tall_cols"; logistic: "zero_tall_dot",
"zero_tall_samples", "zero_tall_acc", "zero_tall_cols") with the ridge prox - two multiplies, the block
solve's own - in the threshold's place.  Every solve here sets "fused_zero_ridge" (to "1" unless it
says otherwise) and puts "auto" back; the tall solves set "fused_zero_tall" and
"fused_zero_tall_smooth" to "1" as well.

Tolerances are the project's own: against the oracle as in test_more_benchmark_problems
(test_gpu_parity.py: f64 rtol 1e-6, atol 1e-8; f32 rtol = atol = 5e-3, equal state and stopping
sweep); fused against generic in f64 the bound of the other ZERO-route tests, 1e-9 of the largest
magnitude.

Shapes.  Tall: (601, 256) the column floor and a trailing unpaired streamed column; (603, 260)
columns past a wave boundary; (2051, 1028) a ragged second chunk per thread and the tile-packed
symmetric apply.  Fat: the same transposed.  Weights: lam = 0.1 on tall shapes; on fat shapes 1.0 for
hinge and SVR (at 0.1 a class of the zone is empty after 60 sweeps) and 0.1 for logistic.

Stopping rule, on the oracle: hinge_l2 (603, 260) stops at 30 with s / eps_dual = 0.39 after 1.11 at
the check before (r / eps_pri 0.21 after 0.54); logreg_l2 (260, 601) stops at 40 with 0.45 after 1.26
(r / eps_pri below 0.02 at both)."""

import contextlib

import numpy as np
import pytest

from epsilon_amd import ir, problems, wire
from epsilon_amd.wire import ProxFunction
from oracle import epsilon_oracle as orc
from tests import route_support as rs

pytestmark = pytest.mark.gpu

TALL = [(601, 256), (603, 260), (2051, 1028)]
FAT = [(256, 601), (260, 601), (1028, 2051)]
KINDS = ["hinge", "svr", "logreg"]
FIXED = dict(max_iterations=60, abs_tol=0.0, rel_tol=0.0)
# routes.solve(prob, dtype, ridge, **options by name, **solver params)
ROUTE_OPTIONS = (("tall", "fused_zero_tall", "1"), ("tall_smooth", "fused_zero_tall_smooth", "1"),
                 ("fused", "fused", "1"), ("fused_zero", "fused_zero", "auto"))
ON = rs.switched_on(ROUTE_OPTIONS)  # what the handles and the batches set beside "fused_zero_ridge"


def is_tall(shape):
    return shape[0] > shape[1]


def lam_of(kind, shape):
    return 0.1 if is_tall(shape) or kind == "logreg" else 1.0


# ---- the option of this module: route_support's scope has no row for it ------------------------------
@contextlib.contextmanager
def ridge_option(mod, value):
    """"fused_zero_ridge" = value for the block; "auto", the library's default, on every way out"""
    try:
        mod.set_option("fused_zero_ridge", value)
        yield
    finally:
        mod.set_option("fused_zero_ridge", "auto")


class Routes(rs.Routes):
    def solve(self, prob, dtype="f32", ridge="1", **params):
        with ridge_option(self.mod, ridge):
            return super(Routes, self).solve(prob, dtype, **params)


@pytest.fixture
def routes(solve_mod):
    return Routes(solve_mod, ROUTE_OPTIONS)


GENERATORS = {"hinge": problems.hinge_l2, "svr": problems.svr_l2, "logreg": problems.logreg_l2}


def offset_ridge(m, n):
    """hinge_l2 with a constant added to the ridge term's argument: lam ||x + c||^2"""
    C = problems.hinge_l2(m, n)[1]["C"]
    c = np.linspace(-1.0, 1.0, n)

    def terms(x, z):
        arg = ir.add(ir.linear_map(ir.scalar(-1, m), z), ir.scalar_constant(1.0, (m, 1)))
        return [ir.prox(ProxFunction.SUM_HINGE, arg),
                ir.prox(ProxFunction.SUM_SQUARE, ir.add(x, ir.constant(c)), alpha=0.1)]
    return problems._graph_form(terms, C, None)


def elastic_net(m, n):
    """hinge loss with an l1 and a ridge term on x, each on a copy of its own"""
    C = problems.hinge_l2(m, n)[1]["C"]
    x, z = ir.variable(n, 1, "var:x"), ir.variable(m, 1, "var:z")
    xr = ir.variable(n, 1, "separate:var:x:sum_square")
    xp, zp = ir.variable(n, 1, "separate:var:x:zero"), ir.variable(m, 1, "separate:var:z:zero")
    arg = ir.add(ir.linear_map(ir.scalar(-1, m), z), ir.scalar_constant(1.0, (m, 1)))
    terms = [ir.prox(ProxFunction.SUM_HINGE, arg), ir.prox(ProxFunction.NORM_1, x, alpha=0.05),
             ir.prox(ProxFunction.SUM_SQUARE, xr, alpha=0.1),
             ir.prox(ProxFunction.ZERO, ir.add(ir.linear_map(ir.dense_matrix(C), xp),
                                               ir.linear_map(ir.scalar(-1, m), zp)))]
    cons = [ir.zero(ir.add(xp, ir.linear_map(ir.scalar(-1, n), x))),
            ir.zero(ir.add(xr, ir.linear_map(ir.scalar(-1, n), x))),
            ir.zero(ir.add(zp, ir.linear_map(ir.scalar(-1, m), z)))]
    return ir.Problem(terms, cons)


make = rs.memoised(dict(
    {k: (lambda m, n, k=k: GENERATORS[k](m, n, lam=lam_of(k, (m, n)))[0]) for k in KINDS},
    offset=offset_ridge, elastic=elastic_net,
    hinge_l1=lambda m, n: problems.hinge_l1(m, n, lam=0.01 * rs.lam_scale("hinge_l1", m, n))[0]))
oracle = rs.oracle_of(make)


def zero_tags(c):
    return sorted(t for t in c if t.startswith("zero_"))


def assert_route(c, st, kind, shape):
    """one launch of every kernel of the route per sweep, nothing of the other route, of the lasso
    route or of a batch, the packed symmetric apply from a pivot of order 1024"""
    n = rs.sweeps(st)
    if not is_tall(shape):
        want = {"zero_fused": n, "zero_fused_rows": n}
    elif kind == "logreg":
        want = {"zero_tall_dot": n, "zero_tall_samples": n, "zero_tall_acc": n, "zero_tall_cols": n}
    else:
        want = {"zero_tall": n, "zero_tall_cols": n}
    # (the first head of a smooth term, "zero_fused_head" / "zero_tall_head", belongs to Init)
    got = {t: c[t] for t in zero_tags(c) if not t.endswith("_head")}
    assert got == want, (got, want)
    assert "lasso_fused" not in c and not [t for t in c if t.startswith("batch_")], sorted(c)
    if min(shape) >= 1024:
        assert c.get("symv_packed", 0) >= n, sorted(c)


def assert_generic(c):
    assert not zero_tags(c) and "lasso_fused" not in c, sorted(c)


# ---- 1. fixed 60 sweeps, every variable against the oracle -----------------------------------------
def assert_every_class(kind, xo):
    """on the oracle's result alone: the 60-sweep iterate has rows in every class of the loss's zone
    (logistic: arguments of both signs), and x is not zero"""
    x, z = xo["var:x"], xo["var:z"]
    assert np.abs(x).max() > 0.1
    if kind == "hinge":
        h = 1.0 - z
        cls = [(h < 0).sum(), (h == 0).sum(), (h > 0).sum()]
        print("hinge: 1 - z < 0, == 0, > 0 on", [int(v) for v in cls], "rows")
    elif kind == "svr":
        M = 0.5
        cls = [(np.abs(z) < M).sum(), (z == M).sum(), (z == -M).sum(), (z > M).sum(), (z < -M).sum()]
        print("deadzone: inside, on +, on -, beyond +, beyond -:", [int(v) for v in cls])
    else:
        # (no zone: the Newton solve runs at arguments spread over the curved part of the loss; on fat
        # C the classes separate and every z = -y a^T x is negative)
        cls = [(z < -2.0).sum(), (np.abs(z) < 1.0).sum()]
        print("logistic: z < -2, |z| < 1 on", [int(v) for v in cls], "rows; z in [%.3g, %.3g]" % (z.min(), z.max()))
    assert all(v > 0 for v in cls)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("shape", TALL + FAT)
@pytest.mark.parametrize("kind", KINDS)
def test_sixty_sweeps_match_the_oracle(routes, kind, shape, dtype):
    so, xo = oracle(kind, shape, **FIXED)
    assert so.state == wire.SolverStatus.MAX_ITERATIONS_REACHED and so.num_iterations == 60
    assert sorted(xo) == ["separate:var:x:zero", "separate:var:z:zero", "var:x", "var:z"]
    assert_every_class(kind, xo)
    st, x, c = routes.solve(make(kind, shape), dtype, **FIXED)
    assert_route(c, st, kind, shape)
    rs.assert_matches_oracle(st, x, so, xo, dtype)


# ---- 2. default stopping rule ------------------------------------------------------------------------
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


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kind,shape,stop", [("hinge", (603, 260), 30), ("logreg", (260, 601), 40)])
def test_stops_with_the_oracle(routes, kind, shape, stop, dtype):
    so, xo, ratios = oracle_checks(kind, shape)
    assert so.state == wire.SolverStatus.OPTIMAL and so.num_iterations == stop
    (r0, s0), (r1, s1) = ratios[stop - 10], ratios[stop]
    print("oracle: r / eps_pri %.3f then %.3f, s / eps_dual %.3f then %.3f" % (r0, r1, s0, s1))
    # the dual residual decides, and both checks are at least 10 % away from the threshold
    assert s0 >= 1.1 and s1 <= 0.9 and r0 <= 0.9 and r1 <= 0.9
    st, x, c = routes.solve(make(kind, shape), dtype)
    assert_route(c, st, kind, shape)
    rs.assert_matches_oracle(st, x, so, xo, dtype)


# ---- 3. fused against generic, f64 --------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(603, 260), (260, 601)])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_equals_generic_to_rounding_f64(routes, kind, shape):
    prob = make(kind, shape)
    st, x, c = routes.solve(prob, "f64", "1", **FIXED)
    st0, x0, c0 = routes.solve(prob, "f64", "0", **FIXED)
    assert_route(c, st, kind, shape)
    assert_generic(c0)
    assert rs.status(st).num_iterations == rs.status(st0).num_iterations == 60
    for k in x0:
        diff, ref = np.abs(x[k] - x0[k]).max(), np.abs(x0[k]).max()
        print(k, "max |fused - generic| %.3g, max |generic| %.3g" % (diff, ref))
    for k in x0:
        assert np.abs(x[k] - x0[k]).max() <= 1e-9 * np.abs(x0[k]).max(), k


# ---- 4. sweep boundaries and warm start -------------------------------------------------------------
BOUNDARY = [("hinge", (601, 256)), ("logreg", (256, 601))]


def sweep_tags(kind, shape):
    return ("zero_tall", "zero_tall_cols") if is_tall(shape) else ("zero_fused", "zero_fused_rows")


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kind,shape", BOUNDARY)
def test_a_solve_can_stop_after_any_sweep(solve_mod, kind, shape, dtype):
    prob = make(kind, shape)
    params = dict(max_iterations=1000, abs_tol=0.0, rel_tol=0.0)
    with ridge_option(solve_mod, "1"):
        st_a, xa, ca = rs.run_handle(solve_mod, prob, dtype, [30], ON, **params)
        st_b, xb, cb = rs.run_handle(solve_mod, prob, dtype, [1, 9, 20], ON, **params)
    for tag in sweep_tags(kind, shape):
        assert ca.get(tag) == cb.get(tag) == 30, (tag, ca.get(tag), cb.get(tag))
    assert len(xa) == 4
    rs.assert_same_arrays(xa, xb)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kind,shape", BOUNDARY)
def test_warm_start_takes_the_state_over(solve_mod, kind, shape, dtype):
    """two solves of 30 sweeps on one handle, the second warm-started, against the oracle doing
    the same on one solver object"""
    prob = make(kind, shape)
    sp = wire.SolverParams(warm_start=True, max_iterations=30, abs_tol=0.0, rel_tol=0.0)
    pb, data = prob.SerializeToString(), prob.expression_data()
    with ridge_option(solve_mod, "1"), rs.handle(solve_mod, prob, dtype, sp, **ON) as s:
        s.init()
        s.run(-1)
        s.init()
        s.run(-1)
        c = rs.base_counts(solve_mod.profile_dump())
        st, x = s.result()
    for tag in sweep_tags(kind, shape):
        assert c.get(tag) == 60, (tag, c.get(tag))
    osolver = orc.create_solver(wire.Problem.FromString(pb), dict(data), sp)
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


# ---- 5. what keeps the generic path under "1" -------------------------------------------------------
@pytest.mark.parametrize("kind,shape,ridge,options", [
    ("hinge", (601, 256), "0", {}),                       # the option's "0", tall
    ("svr", (256, 601), "0", {}),                         # the option's "0", fat
    ("logreg", (601, 256), "0", {}),                      # the option's "0", tall smooth
    ("hinge", (256, 601), "1", {"fused_zero": "0"}),      # the ZERO-term routes switched off
    ("hinge", (601, 256), "1", {"fused_zero": "0"}),
    ("hinge", (601, 256), "1", {"tall": "0"}),            # the tall route switched off
    ("logreg", (601, 256), "1", {"tall_smooth": "0"}),    # the smooth tall form switched off
    ("hinge", (601, 256), "1", {"solver": 1}),            # two-block driver
    ("hinge", (256, 601), "1", {"solver": 1}),
    ("hinge", (600, 252), "1", {}),                       # below the column floor
    ("hinge", (252, 601), "1", {}),                       # below the row floor
    ("offset", (601, 256), "1", {}),                      # a ridge term with an offset
    ("offset", (256, 601), "1", {}),
    ("elastic", (601, 256), "1", {}),                     # an l1 term on x beside the ridge term
    ("elastic", (256, 601), "1", {}),
])
def test_fall_backs_are_the_generic_path(routes, kind, shape, ridge, options):
    prob = make(kind, shape)
    params = dict(max_iterations=30, **options)
    st, x, c = routes.solve(prob, "f32", ridge, **params)
    params["fused"] = "0"
    st0, x0, c0 = routes.solve(prob, "f32", ridge, **params)
    assert_generic(c)
    assert_generic(c0)
    rs.assert_same_bytes(st, x, st0, x0)


# ---- 6. the option touches nothing but problems with a ridge term -----------------------------------
@pytest.mark.parametrize("shape", [(601, 256), (256, 601)])
def test_l1_problems_are_untouched(routes, shape):
    prob = make("hinge_l1", shape)
    st0, x0, c0 = routes.solve(prob, "f32", "0", max_iterations=30)
    assert c0.get("zero_tall" if is_tall(shape) else "zero_fused", 0) == rs.sweeps(st0), sorted(c0)
    for word in ("1", "auto"):
        st, x, c = routes.solve(prob, "f32", word, max_iterations=30)
        assert {t: c[t] for t in zero_tags(c)} == {t: c0[t] for t in zero_tags(c0)}
        rs.assert_same_bytes(st, x, st0, x0, word)


# ---- 8. "auto" ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,on,below", [
    ("hinge", (601, 256), (600, 252)),    # tall, one pass: the floor is 256 columns
    ("logreg", (601, 256), (600, 252)),   # tall, the pass in halves: 256 columns
    ("svr", (256, 601), (252, 601)),      # fat: 256 rows
])
def test_auto_follows_the_measured_floors(routes, kind, on, below):
    """every measured cell is ahead of the generic path, so each floor of "auto" is its
    route's first cell: at it "auto" returns the bytes of "1" on the route, below it those of "0"."""
    st, x, c = routes.solve(make(kind, on), "f32", "auto", max_iterations=30)
    st1, x1, c1 = routes.solve(make(kind, on), "f32", "1", max_iterations=30)
    assert_route(c, st, kind, on)
    assert_route(c1, st1, kind, on)
    rs.assert_same_bytes(st, x, st1, x1)
    st, x, c = routes.solve(make(kind, below), "f32", "auto", max_iterations=30)
    st0, x0, c0 = routes.solve(make(kind, below), "f32", "0", max_iterations=30)
    assert_generic(c)
    assert_generic(c0)
    rs.assert_same_bytes(st, x, st0, x0)


# ---- 7. batch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,lams,tall_groups", [
    ((601, 256), (0.2, 0.1, 0.05), "0"),
    ((601, 256), (0.2, 0.1, 0.05), "1"),
    ((256, 601), (1.0, 0.7, 0.5), "0"),
])
def test_batch_members_are_their_own_solves(solve_mod, shape, lams, tall_groups):
    """three hinge_l2 members on one C: the batched kernels have no ridge head, so every member is
    solved by itself on its route and returns its own solve bit for bit"""
    probs = [problems.hinge_l2(*shape, lam=lam)[0] for lam in lams]
    with ridge_option(solve_mod, "1"):
        batch, tagsb, single, _ = rs.run_both(solve_mod, probs, "f32", dict(ON, batch_zero_tall=tall_groups),
                                              max_iterations=60)
    cb = rs.base_counts(tagsb)
    total = sum(rs.sweeps(st) for st, _ in batch)
    for tag in sweep_tags("hinge", shape):
        assert cb.get(tag, 0) == total, (tag, cb.get(tag), total)
    assert not [t for t in cb if t.startswith("batch_")], sorted(cb)
    assert len(batch) == len(single) == 3
    rs.assert_identical(batch, single)
