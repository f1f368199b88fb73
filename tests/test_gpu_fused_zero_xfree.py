"""The fused sweep of tall ZERO-term problems whose x lives in the ZERO term alone (DESIGN.md 3.11
"x in the ZERO term alone", option "fused_zero_xfree"): least absolute deviations and quantile
regression in graph form (problems.least_abs_dev, problems.quantile with tau = 0.3, seed 0) run as
the pass over the transposed copy of the data matrix (tag "zero_tall"), one kernel on the x side
that sums the partials and keeps x (tag "zero_tall_free_cols") and the apply of the cached n x n
inverse.  Every solve here sets "fused_zero_xfree" (to "1" unless it says otherwise) and puts "0",
the library's default, back; route_support's scope sets the other options.

Tolerances are the project's own: against the oracle as in test_more_benchmark_problems
(test_gpu_parity.py: f64 rtol 1e-6, atol 1e-8; f32 rtol = atol = 5e-3, equal state and stopping
sweep); fused against generic in f64 the bound of the other ZERO-route tests, 1e-9 of the largest
magnitude.

Shapes: (601, 256) the column floor, odd m; (603, 260) columns past a wave boundary; (2051, 1028) a
second, ragged chunk per thread and the tile-packed symmetric apply of the inverse.

Stopping rule, on the CPU oracle (stop; r / eps_pri, s / eps_dual at the stop after those one check
earlier): lad (601, 256) 40; 0.765, 0.875 after 1.062, 1.163 - margins that carry f32 rounding.
lad (603, 260) 40; 0.701, 0.681 after 0.968, 1.014 and quantile (603, 260) 80; 0.198, 0.917 after
0.273, 1.020 - f64 alone.  quantile (601, 256) is not used: its dual ratio at the stop is 0.999.

No test solves a fat problem of these kinds: C^T C is singular there on every path."""

import contextlib
import os

import numpy as np
import pytest

from epsilon_amd import ir, problems, wire
from epsilon_amd.wire import ProxFunction
from oracle import epsilon_oracle as orc
from tests import route_support as rs

pytestmark = pytest.mark.gpu

SHAPES = [(601, 256), (603, 260), (2051, 1028)]
KINDS = ["lad", "quantile"]
FIXED = dict(max_iterations=60, abs_tol=0.0, rel_tol=0.0)
VARIABLES = ["separate:var:z:zero", "var:x", "var:z"]
# routes.solve(prob, dtype, xfree, **options by name, **solver params)
ROUTE_OPTIONS = (("tall", "fused_zero_tall", "1"), ("fused", "fused", "1"), ("fused_zero", "fused_zero", "auto"))
ON = rs.switched_on(ROUTE_OPTIONS)  # what the handles and the batches set beside "fused_zero_xfree"
TAUS3 = (0.1, 0.5, 0.9)
TAUS9 = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9)


# ---- the option of this module: route_support's scope has no row for it ------------------------------
@contextlib.contextmanager
def xfree_option(mod, value):
    """"fused_zero_xfree" = value for the block (None: the variable unset); "0", the library's
    default, on every way out"""
    try:
        if value is None:
            mod.set_option("fused_zero_xfree", "0")
            os.unsetenv("EPSILON_HIP_FUSED_ZERO_XFREE")  # (the library reads the process environment)
        else:
            mod.set_option("fused_zero_xfree", value)
        yield
    finally:
        mod.set_option("fused_zero_xfree", "0")


class Routes(rs.Routes):
    def solve(self, prob, dtype="f32", xfree="1", **params):
        with xfree_option(self.mod, xfree):
            return super(Routes, self).solve(prob, dtype, **params)


@pytest.fixture
def routes(solve_mod):
    return Routes(solve_mod, ROUTE_OPTIONS)


def free_logistic(m, n):
    """plain logistic regression, no penalty: sum_logistic(z) with z = C x, x in the ZERO term alone"""
    C = problems.logreg_l1(m, n)[1]["C"]
    return problems._graph_form(lambda x, z: [ir.prox(ProxFunction.SUM_LOGISTIC, z, alpha=1.0)], C, None,
                                x_in_terms=False)


def hinge_on_quantile_data(m, n):
    """hinge loss + l1 on the data matrix and offset of problems.quantile(m, n): a member with a
    copied x on the very matrix of the tau path"""
    info = problems.quantile(m, n)[1]
    A, b = info["A"], info["b"]
    lam = 0.05 * np.abs(A.sum(axis=0)).max()

    def terms(x, z):
        arg = ir.add(ir.linear_map(ir.scalar(-1, m), z), ir.scalar_constant(1.0, (m, 1)))
        return [ir.prox(ProxFunction.SUM_HINGE, arg), ir.prox(ProxFunction.NORM_1, x, alpha=lam)]
    return problems._graph_form(terms, A, -b)


make = rs.memoised({
    "lad": lambda m, n: problems.least_abs_dev(m, n)[0],
    "quantile": lambda m, n: problems.quantile(m, n)[0],
    "logistic": free_logistic,
    "hinge_l1": lambda m, n: problems.hinge_l1(m, n, lam=0.01 * rs.lam_scale("hinge_l1", m, n))[0],
    "lasso": lambda m, n: problems.lasso(m, n, seed=0)[0],
    "hinge_on_quantile": hinge_on_quantile_data,
})
oracle = rs.oracle_of(make)


def tau_path(shape, taus):
    return [problems.quantile(shape[0], shape[1], tau=tau)[0] for tau in taus]


def zero_tags(c):
    return sorted(t for t in c if t.startswith(("zero_", "batch_zero")))


def assert_route(c, st, shape):
    """one pass and one free-x launch per sweep, no x-side chain, nothing of the fat route, of the
    lasso route or of a batch, the packed symmetric apply from 1024 columns"""
    n = rs.sweeps(st)
    got = {t: c[t] for t in zero_tags(c)}
    assert got == {"zero_tall": n, "zero_tall_free_cols": n}, (got, n)
    assert "zero_tall_cols" not in c and not [t for t in c if t.startswith("zero_fused")], sorted(c)
    assert "lasso_fused" not in c
    if shape[1] >= 1024:
        assert c.get("symv_packed", 0) >= n, sorted(c)


def assert_generic(c):
    assert not zero_tags(c) and "lasso_fused" not in c, sorted(c)


# ---- 1. fixed 60 sweeps, every variable against the oracle -----------------------------------------
def assert_every_class(kind, shape, xo):
    """on the oracle's result alone: after 60 sweeps z has entries on the kink of the loss, above it
    and below it, so the zone's three branches all decide entries of the iterate"""
    z = xo["var:z"]
    cls = [int((z == 0).sum()), int((z > 0).sum()), int((z < 0).sum())]
    print(kind, shape, "z == 0, > 0, < 0 on", cls, "rows")
    assert all(v > 0 for v in cls)
    assert np.abs(xo["var:x"]).max() > 0.1


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_sixty_sweeps_match_the_oracle(routes, kind, shape, dtype):
    so, xo = oracle(kind, shape, **FIXED)
    assert so.state == wire.SolverStatus.MAX_ITERATIONS_REACHED and so.num_iterations == 60
    assert sorted(xo) == VARIABLES
    assert_every_class(kind, shape, xo)
    st, x, c = routes.solve(make(kind, shape), dtype, **FIXED)
    assert_route(c, st, shape)
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


@pytest.mark.parametrize("kind,shape,stop,dtype", [
    ("lad", (601, 256), 40, "f32"),
    ("lad", (601, 256), 40, "f64"),
    ("lad", (603, 260), 40, "f64"),
    ("quantile", (603, 260), 80, "f64"),
])
def test_stops_with_the_oracle(routes, kind, shape, stop, dtype):
    so, xo, ratios = oracle_checks(kind, shape)
    assert so.state == wire.SolverStatus.OPTIMAL and so.num_iterations == stop
    (r0, s0), (r1, s1) = ratios[stop - 10], ratios[stop]
    print("oracle: r / eps_pri %.3f then %.3f, s / eps_dual %.3f then %.3f" % (r0, r1, s0, s1))
    st, x, c = routes.solve(make(kind, shape), dtype)
    assert_route(c, st, shape)
    rs.assert_matches_oracle(st, x, so, xo, dtype)


# ---- 3. fused against generic, f64 --------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_fused_equals_generic_to_rounding_f64(routes, kind):
    shape = (603, 260)
    prob = make(kind, shape)
    st, x, c = routes.solve(prob, "f64", "1", **FIXED)
    st0, x0, c0 = routes.solve(prob, "f64", "0", **FIXED)
    assert_route(c, st, shape)
    assert_generic(c0)
    assert rs.status(st).num_iterations == rs.status(st0).num_iterations == 60
    assert sorted(x) == sorted(x0) == VARIABLES
    for k in x0:
        diff, ref = np.abs(x[k] - x0[k]).max(), np.abs(x0[k]).max()
        print(k, "max |fused - generic| %.3g, max |generic| %.3g" % (diff, ref))
    for k in x0:
        assert np.abs(x[k] - x0[k]).max() <= 1e-9 * np.abs(x0[k]).max(), k


# ---- 4. sweep boundaries and warm start -------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_a_solve_can_stop_after_any_sweep(solve_mod, dtype):
    prob = make("lad", (601, 256))
    params = dict(max_iterations=1000, abs_tol=0.0, rel_tol=0.0)
    with xfree_option(solve_mod, "1"):
        st_a, xa, ca = rs.run_handle(solve_mod, prob, dtype, [30], ON, **params)
        st_b, xb, cb = rs.run_handle(solve_mod, prob, dtype, [1, 9, 20], ON, **params)
    assert ca.get("zero_tall") == cb.get("zero_tall") == 30
    assert ca.get("zero_tall_free_cols") == cb.get("zero_tall_free_cols") == 30
    assert sorted(xa) == VARIABLES
    rs.assert_same_arrays(xa, xb)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_warm_start_takes_the_state_over(solve_mod, dtype):
    """two solves of 30 sweeps on one handle, the second warm-started, against the oracle doing
    the same on one solver object"""
    shape = (601, 256)
    prob = make("lad", shape)
    sp = wire.SolverParams(warm_start=True, max_iterations=30, abs_tol=0.0, rel_tol=0.0)
    pb, data = prob.SerializeToString(), prob.expression_data()
    with xfree_option(solve_mod, "1"), rs.handle(solve_mod, prob, dtype, sp, **ON) as s:
        s.init()
        s.run(-1)
        s.init()
        s.run(-1)
        c = rs.base_counts(solve_mod.profile_dump())
        st, x = s.result()
    assert c.get("zero_tall") == c.get("zero_tall_free_cols") == 60
    osolver = orc.create_solver(wire.Problem.FromString(pb), dict(data), sp)
    osolver.solve()
    xo = osolver.solve()
    assert rs.status(st).num_iterations == osolver.status.num_iterations == 30
    x = rs.arrays(x)
    xw = {k: np.asarray(xo(k), dtype=np.float64).ravel() for k in x}
    # on the oracle alone: the second solve went on from the first - in some variable its iterate is
    # off the cold solve's by more than twice what the f32 tolerances allow, so a route that dropped
    # the state would not pass
    cold = oracle("lad", shape, max_iterations=30, abs_tol=0.0, rel_tol=0.0)[1]
    tol = rs.TOLERANCES["f32"]
    room = max(np.abs(xw[k] - cold[k]).max() / (tol["atol"] + tol["rtol"] * np.abs(cold[k]).max()) for k in cold)
    print("oracle: max |warm - cold| is %.3g x the f32 tolerance" % room)
    assert room > 2.0
    rs.assert_close(x, xw, dtype)


# ---- 5. what keeps the generic path -----------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,options", [
    ("lad", (600, 252), {}),                          # below the column floor
    ("quantile", (600, 252), {}),
    ("lad", (601, 258), {}),                          # columns not a multiple of 4
    ("lad", (601, 256), {"solver": 1}),               # two-block driver
    ("lad", (601, 256), {"fused": "0"}),              # the fused routes switched off altogether
    ("lad", (601, 256), {"fused_zero": "0"}),         # the ZERO-term routes switched off
    ("quantile", (601, 256), {"tall": "0"}),          # the tall route switched off
    ("logistic", (601, 256), {}),                     # a smooth z term with free x
])
def test_fall_backs_are_the_generic_path(routes, kind, shape, options):
    prob = make(kind, shape)
    params = dict(max_iterations=30, **options)
    st, x, c = routes.solve(prob, "f32", "1", **params)
    st0, x0, c0 = routes.solve(prob, "f32", "0", **params)
    assert_generic(c)
    assert_generic(c0)
    rs.assert_same_bytes(st, x, st0, x0)


@pytest.mark.parametrize("xfree", [None, "0"])
@pytest.mark.parametrize("kind", KINDS)
def test_the_default_is_the_generic_path(routes, kind, xfree):
    """the variable unset, and "0", at a shape the route takes under "1": no tall launch, and the
    bytes of the solve with every fused route off"""
    prob = make(kind, (601, 256))
    st, x, c = routes.solve(prob, "f32", xfree, max_iterations=30)
    st0, x0, c0 = routes.solve(prob, "f32", xfree, fused="0", max_iterations=30)
    st1, x1, c1 = routes.solve(prob, "f32", "1", max_iterations=30)
    assert_generic(c)
    assert_generic(c0)
    assert_route(c1, st1, (601, 256))
    rs.assert_same_bytes(st, x, st0, x0)


# ---- 6. the option touches nothing but problems with free x -----------------------------------------
@pytest.mark.parametrize("kind,tag", [("hinge_l1", "zero_tall_cols"), ("lasso", "lasso_tall_cols")])
def test_other_problems_are_untouched(routes, kind, tag):
    prob = make(kind, (601, 256))
    st0, x0, c0 = routes.solve(prob, "f32", "0", max_iterations=30)
    st1, x1, c1 = routes.solve(prob, "f32", "1", max_iterations=30)
    assert c0.get(tag, 0) == rs.sweeps(st0), sorted(c0)
    assert "zero_tall_free_cols" not in c0 and "zero_tall_free_cols" not in c1
    assert c0 == c1, (c0, c1)
    rs.assert_same_bytes(st1, x1, st0, x0)


# ---- 7. batch: a tau path ----------------------------------------------------------------------------
GROUP = ("batch_zero_tall_pass", "batch_zero_tall_free_cols")
SINGLE = ("zero_tall", "zero_tall_free_cols")


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("shape,taus", [((601, 256), TAUS3), ((603, 260), TAUS9)])
def test_a_tau_path_is_one_group(solve_mod, shape, taus, dtype):
    """members that differ in tau alone share C, its transposed copy and the inverse: one group,
    every member its own solve bit for bit; nine f32 members at one chunk per thread are passes of 8
    and 1"""
    probs = tau_path(shape, taus)
    with xfree_option(solve_mod, "1"):
        batch, tagsb, single, tags1 = rs.run_both(solve_mod, probs, dtype, dict(ON, batch_zero_tall="1"),
                                                  max_iterations=150)
    cb, c1 = rs.base_counts(tagsb), rs.base_counts(tags1)
    print(dtype, shape, [(rs.status(st).state, rs.status(st).num_iterations) for st, _ in single])
    assert_route(c1, single[0][0], shape)
    longest = max(rs.sweeps(st) for st, _ in batch)
    assert cb.get("batch_zero_tall_free_cols") == longest, (cb, longest)
    assert cb.get("batch_zero_tall_pass", 0) >= longest, cb
    if dtype == "f32" and len(taus) == 9:
        assert cb.get("batch_zero_tall_pass") > longest, cb  # more than one pass per sweep while 9 are active
    assert not [t for t in cb if t.startswith("zero_")] and "batch_zero_tall_cols" not in cb, sorted(cb)
    assert cb.get("transpose_copy") == 1, sorted(cb)
    assert len(batch) == len(single) == len(taus)
    rs.assert_identical(batch, single)


def test_without_the_batch_option_every_member_runs_alone(solve_mod):
    probs = tau_path((601, 256), TAUS3)
    with xfree_option(solve_mod, "1"):
        batch, tagsb, single, _ = rs.run_both(solve_mod, probs, "f32", dict(ON, batch_zero_tall="0"),
                                              max_iterations=60)
    cb = rs.base_counts(tagsb)
    total = sum(rs.sweeps(st) for st, _ in batch)
    assert cb.get("zero_tall", 0) == cb.get("zero_tall_free_cols", 0) == total, (cb, total)
    assert not [t for t in cb if t.startswith("batch_zero")], sorted(cb)
    rs.assert_identical(batch, single)


def test_a_hinge_member_joins_no_quantile_group(solve_mod):
    """a hinge + l1 member on the path's own matrix has a copied x and its own x-side chain: it is
    solved by itself, the three quantile members form their group"""
    shape = (601, 256)
    quant = tau_path(shape, TAUS3)
    probs = [quant[0], make("hinge_on_quantile", shape), quant[1], quant[2]]
    with xfree_option(solve_mod, "1"):
        batch, tagsb, single, _ = rs.run_both(solve_mod, probs, "f32", dict(ON, batch_zero_tall="1"),
                                              max_iterations=60)
    cb = rs.base_counts(tagsb)
    hinge_sweeps = rs.sweeps(single[1][0])
    group_sweeps = max(rs.sweeps(single[i][0]) for i in (0, 2, 3))
    assert cb.get("zero_tall") == cb.get("zero_tall_cols") == hinge_sweeps, (cb, hinge_sweeps)
    assert "zero_tall_free_cols" not in cb and "batch_zero_tall_cols" not in cb, sorted(cb)
    assert cb.get("batch_zero_tall_free_cols") == cb.get("batch_zero_tall_pass") == group_sweeps, (cb, group_sweeps)
    rs.assert_identical(batch, single)
