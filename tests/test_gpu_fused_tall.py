"""The fused sweep of the lasso structure with tall A (option "fused_tall"): least
squares + a scaled-zone penalty with more rows than columns never reads A inside a sweep - the tile
launch of the packed n x n inverse and the cols kernel (tag "lasso_tall_cols") from 1024 columns,
the dense apply and the cols kernel below.  Problems: problems.lasso(m, n, seed=0) and the deadzone /
quantile forms of route_support.fused_problem on the same data.

route_support.options has no default for "fused_tall", so this module brings its own scope
(`fused_tall`): it sets the option and puts "auto" back on every way out.

Tolerances are the project's own: against the oracle route_support.TOLERANCES with equal state and
stopping sweep; fused against generic in f64 the tall ZERO route's bound, 1e-9 of the largest
magnitude.

Shapes: (601, 256) the floor, dense apply, two whole workgroups; (603, 259) odd n, a ragged last
workgroup; (2051, 1027) the packed apply with nb = 9, a last tile 3 rows wide and the short loop of
the tiles' sum; (2305, 2181) nb = 18, the eight-at-a-time loop and its remainder.

On the oracle (asserted first): after 60 fixed sweeps x has 78 / 256, 61 / 259, 339 / 1027 and
501 / 2181 non-zero entries; under the default stopping rule all four stop OPTIMAL at 20 with
r / eps_pri 0.14 to 0.56 there - a margin that f32 carries, so the stopping sweep is tested in both
dtypes."""

import contextlib

import numpy as np
import pytest

from epsilon_amd import ir, problems, wire
from oracle import epsilon_oracle as orc
from tests import route_support as rs

pytestmark = pytest.mark.gpu

SHAPES = [(601, 256), (603, 259), (2051, 1027), (2305, 2181)]
NONZERO = {(601, 256): 78, (603, 259): 61, (2051, 1027): 339, (2305, 2181): 501}
FIXED = dict(max_iterations=60, abs_tol=0.0, rel_tol=0.0)
ROUTE_OPTIONS = (("fused", "fused", "1"),)
# kLassoTallAutoMinCols (csrc/fused_route.cc): the measured floor of "auto"; 0: "auto" is "0"
AUTO_FLOOR = 256


@contextlib.contextmanager
def fused_tall(mod, value):
    try:
        mod.set_option("fused_tall", value)
        yield
    finally:
        mod.set_option("fused_tall", "auto")


@pytest.fixture
def routes(solve_mod):
    """solve(prob, dtype, tall, fused, **solver params) -> (status, arrays, {full tag: (count, ms)})"""
    r = rs.Routes(solve_mod, ROUTE_OPTIONS, raw_tags=True)

    def solve(prob, dtype="f32", tall="1", fused="1", **params):
        with fused_tall(solve_mod, tall):
            return r.solve(prob, dtype, fused, **params)
    return solve


def zone_problem(kind):
    def build(m, n):
        A, b = problems.regression_data(m, n, seed=0)
        rng = np.random.RandomState(2)
        qvec = (0.2 + rng.rand(n), 0.2 + rng.rand(n))
        return rs.fused_problem(ir.dense_matrix(A), m, n, ir.constant(b), 0.2 * np.abs(A.T.dot(b)).max(), kind, qvec)
    return build


def parameter_problem(m, n):
    A, b = problems.regression_data(m, n, seed=0)
    return problems.lasso_ir(ir.dense_matrix(A), ir.parameter(m, 1, "param:b"), 0.2 * np.abs(A.T.dot(b)).max(), n)


make = rs.memoised({
    "lasso": lambda m, n: problems.lasso(m, n, seed=0)[0],
    "deadzone": zone_problem("deadzone"),
    "quantile": zone_problem("quantile"),
    "matrix": lambda m, n: problems.mv_lasso(m, n, 3)[0],
    "param_b": parameter_problem,
})
oracle = rs.oracle_of(make)


def route_tags(tags):
    c = rs.base_counts(tags)
    return sorted(t for t in c if "lasso_tall" in t or t.startswith("lasso_fused") or t.endswith("_fused"))


def data_products(tags, shape):
    """launches of a mat-vec with A's shape"""
    return sum(c for t, (c, _) in tags.items() if t.startswith("gemv") and t.endswith(":%dx%d" % shape))


def assert_route(tags, nsweeps, shape, inits=1):
    """one cols launch per sweep (the checks are not pipelined into discarded sweeps), the tile
    launch with it from 1024 columns, A read once per Init - for c - and never in a sweep, no launch
    of the fat route"""
    c = rs.base_counts(tags)
    assert c.get("lasso_tall_cols", 0) == nsweeps, (route_tags(tags), c.get("lasso_tall_cols"), nsweeps)
    assert c.get("lasso_tall_rhs", 0) == inits, route_tags(tags)
    assert data_products(tags, shape) == inits, sorted(tags)
    assert not [t for t in c if t.startswith("lasso_fused") or t.endswith("_fused")], sorted(c)
    if shape[1] >= 1024:
        assert c.get("symv_packed_tiles", 0) == nsweeps, sorted(c)


def assert_generic(tags):
    assert route_tags(tags) == [], route_tags(tags)


# ---- 1. fixed 60 sweeps against the oracle -----------------------------------------------------------
CASES = [("lasso", s) for s in SHAPES] + [(k, s) for k in ("deadzone", "quantile") for s in SHAPES[1:3]]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kind,shape", CASES)
def test_sixty_sweeps_match_the_oracle(routes, kind, shape, dtype):
    so, xo = oracle(kind, shape, **FIXED)
    assert so.state == wire.SolverStatus.MAX_ITERATIONS_REACHED and so.num_iterations == 60
    x = xo[problems.LASSO_VAR]
    print(kind, shape, "x nonzero", int((x != 0).sum()), "of", x.size)
    if kind == "lasso":
        assert int((x != 0).sum()) == NONZERO[shape]
    st, x, tags = routes(make(kind, shape), dtype, **FIXED)
    assert_route(tags, 60, shape)
    rs.assert_matches_oracle(st, x, so, xo, dtype)


# ---- 2. default stopping rule ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES)
def test_stops_with_the_oracle(routes, shape, dtype):
    so, xo = oracle("lasso", shape)
    assert so.state == wire.SolverStatus.OPTIMAL and so.num_iterations == 20
    ratio = so.residuals.r_norm / so.residuals.epsilon_primal
    print(shape, "oracle r / eps_pri at the stop %.3g" % ratio)
    assert ratio <= 0.56 + 0.005
    st, x, tags = routes(make("lasso", shape), dtype)
    assert rs.base_counts(tags).get("lasso_tall_cols", 0) >= rs.sweeps(st)  # (pipelined checks: sweeps past the stop)
    assert_generic({t: v for t, v in tags.items() if "lasso_tall" not in t})
    rs.assert_matches_oracle(st, x, so, xo, dtype)


# ---- 3. fused against generic, f64 -------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES[1:3])
def test_fused_equals_generic_to_rounding_f64(routes, shape):
    prob = make("lasso", shape)
    st, x, tags = routes(prob, "f64", "1", **FIXED)
    st0, x0, tags0 = routes(prob, "f64", "0", **FIXED)
    assert_route(tags, 60, shape)
    assert_generic(tags0)
    assert rs.status(st).num_iterations == rs.status(st0).num_iterations == 60
    for k in x0:
        diff, ref = np.abs(x[k] - x0[k]).max(), np.abs(x0[k]).max()
        print(k, "max |fused - generic| %.3g, max |generic| %.3g" % (diff, ref))
        assert diff <= 1e-9 * ref, k


# ---- 4. sweep boundaries, 5. warm start -------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("shape", [(603, 259), (2051, 1027)])
def test_a_solve_can_stop_after_any_sweep(solve_mod, shape, dtype):
    prob = make("lasso", shape)
    params = dict(max_iterations=1000, abs_tol=0.0, rel_tol=0.0)
    with fused_tall(solve_mod, "1"):
        st_a, xa, ca = rs.run_handle(solve_mod, prob, dtype, [30], {}, **params)
        st_b, xb, cb = rs.run_handle(solve_mod, prob, dtype, [1, 9, 20], {}, **params)
    assert ca.get("lasso_tall_cols") == cb.get("lasso_tall_cols") == 30
    assert len(xa) == 2
    rs.assert_same_arrays(xa, xb)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_warm_start_takes_the_state_over(solve_mod, dtype):
    """two solves of 30 sweeps on one handle, the second warm-started, against the oracle doing the
    same on one solver object.  On the oracle the warm iterate is 4.3e-4 off the cold 30-sweep one in
    x' (the problem is close to its fixed point by then): 100 times the f64 tolerance and below the
    f32 one, so in either dtype the route's own warm - cold gap must also be the oracle's to within a
    factor of two - f32 rounding of the iterates is some 1e-6, far below the gap - which a route
    that dropped the state (gap 0) or restarted part of it does not pass."""
    shape = (603, 259)
    prob = make("lasso", shape)
    fixed = dict(max_iterations=30, abs_tol=0.0, rel_tol=0.0)
    sp = wire.SolverParams(warm_start=True, **fixed)
    pb, data = prob.SerializeToString(), prob.expression_data()
    osolver = orc.create_solver(wire.Problem.FromString(pb), dict(data), sp)
    osolver.solve()
    xo = osolver.solve()
    cold = oracle("lasso", shape, **fixed)[1]
    xw = {k: np.asarray(xo(k), dtype=np.float64).ravel() for k in cold}
    key = problems.LASSO_COPY
    gap = np.abs(xw[key] - cold[key]).max()
    tol64 = rs.TOLERANCES["f64"]
    print("oracle: max |warm - cold| in x' %.3g" % gap)
    assert gap > 100 * (tol64["atol"] + tol64["rtol"] * np.abs(cold[key]).max())
    with fused_tall(solve_mod, "1"):
        with rs.handle(solve_mod, prob, dtype, sp) as s:
            s.init()
            s.run(-1)
            s.init()
            s.run(-1)
            tags = solve_mod.profile_dump()
            st, x = s.result()
        _, xc, _ = rs.run_handle(solve_mod, prob, dtype, [30], {}, **fixed)
    assert_route(tags, 60, shape, inits=2)
    assert rs.status(st).num_iterations == osolver.status.num_iterations == 30
    x = rs.arrays(x)
    rs.assert_close(x, xw, dtype)
    own = np.abs(x[key] - xc[key]).max()
    print("route: max |warm - cold| in x' %.3g" % own)
    assert 0.5 * gap <= own <= 2 * gap


# ---- 6. re-bound b -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("shape", [(603, 259), (2051, 1027)])
def test_each_bound_b_is_its_own_solve(solve_mod, shape, dtype):
    """two solves sharing A (and so the cached inverse) with "param:b" bound to different vectors:
    a c = L(var, arg) rhs_arg kept from the first would fail the second"""
    m, n = shape
    prob = make("param_b", shape)
    b = problems.regression_data(m, n, seed=0)[1]
    bs = [b, 0.5 * b + 0.3 * np.random.RandomState(5).randn(m)]
    pb, sb = prob.SerializeToString(), wire.SolverParams(**FIXED).SerializeToString()
    got, want = [], []
    for bi in bs:
        params, data = rs.bind_b(bi)
        data.update(prob.expression_data())
        so, xo = orc.solve(pb, params, sb, data)
        want.append((rs.status(so), rs.arrays(xo)))
        with fused_tall(solve_mod, "1"), rs.options(solve_mod, dtype=dtype):
            (st, x), tags = rs.profiled(solve_mod, lambda: solve_mod.solve(pb, params, sb, data))
        assert_route(tags, 60, shape)
        got.append((st, rs.arrays(x)))
    tol = rs.TOLERANCES[dtype]
    xa, xb = want[0][1][problems.LASSO_VAR], want[1][1][problems.LASSO_VAR]
    print("oracle: max |x(b0) - x(b1)| %.3g" % np.abs(xa - xb).max())
    assert np.abs(xa - xb).max() > 10 * (tol["atol"] + tol["rtol"] * np.abs(xb).max())
    for (st, x), (so, xo) in zip(got, want):
        rs.assert_matches_oracle(st, x, so, xo, dtype)


# ---- 7. what keeps the generic path under "1" -------------------------------------------------------
@pytest.mark.parametrize("kind,shape,params,fused", [
    ("lasso", (600, 252), {}, "1"),               # below the column floor
    ("lasso", (601, 256), {"solver": 1}, "1"),    # two-block driver
    ("matrix", (601, 256), {}, "1"),              # a matrix variable with tall A
    ("lasso", (601, 256), {}, "0"),               # the fused routes switched off altogether
])
def test_fall_backs_are_the_generic_path(routes, kind, shape, params, fused):
    prob = make(kind, shape)
    params = dict(max_iterations=30, **params)
    st, x, tags = routes(prob, "f32", "1", fused, **params)
    st0, x0, tags0 = routes(prob, "f32", "0", fused, **params)
    assert_generic(tags)
    assert_generic(tags0)
    rs.assert_same_bytes(st, x, st0, x0)


def test_option_zero_is_the_generic_path(routes):
    shape = (601, 256)
    prob = make("lasso", shape)
    st, x, tags = routes(prob, "f32", "0", max_iterations=30)
    st0, x0, tags0 = routes(prob, "f32", "0", "0", max_iterations=30)
    st1, x1, tags1 = routes(prob, "f32", "1", max_iterations=30)
    assert_generic(tags)
    assert_generic(tags0)
    assert rs.base_counts(tags1).get("lasso_tall_cols", 0) >= rs.sweeps(st1)
    rs.assert_same_bytes(st, x, st0, x0)


@pytest.mark.parametrize("shape", [(601, 256), (2051, 1027)])
def test_auto_follows_the_measured_floor(routes, shape):
    """ "auto" is "1" from AUTO_FLOOR columns and "0" below (0: "0" everywhere)"""
    prob = make("lasso", shape)
    same = "1" if AUTO_FLOOR and shape[1] >= AUTO_FLOOR else "0"
    st, x, tags = routes(prob, "f32", "auto", **FIXED)
    st1, x1, tags1 = routes(prob, "f32", same, **FIXED)
    assert route_tags(tags) == route_tags(tags1) and bool(route_tags(tags)) == (same == "1")
    rs.assert_same_bytes(st, x, st1, x1)


# ---- 8. batch ----------------------------------------------------------------------------------------
def lambda_path(shape, fracs):
    m, n = shape
    A, b = problems.regression_data(m, n, seed=0)
    lmax = np.abs(A.T.dot(b)).max()
    return [problems.lasso_ir(ir.dense_matrix(A), ir.constant(b), f * lmax, n) for f in fracs]


def oracle_stops(probs, data):
    out = []
    for p in probs:
        st, _ = orc.solve(p.SerializeToString(), [], wire.SolverParams().SerializeToString(), data)
        out.append(rs.status(st))
    return out


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_a_lambda_path_runs_as_one_group(solve_mod, dtype):
    """(0.4, 0.2, 0.1, 0.02) max|A^T b| at (2051, 1027): the oracle stops the members at 20, 10, 10,
    20 with every ratio <= 0.33 at the stop (0.05 is left out: its s / eps_dual is 0.93 at the
    stop)"""
    shape = (2051, 1027)
    probs = lambda_path(shape, (0.4, 0.2, 0.1, 0.02))
    stops = oracle_stops(probs, rs.union_data(probs))
    assert [s.num_iterations for s in stops] == [20, 10, 10, 20]
    for s in stops:
        assert s.state == wire.SolverStatus.OPTIMAL
        assert s.residuals.r_norm <= 0.33 * s.residuals.epsilon_primal
        assert s.residuals.s_norm <= 0.33 * s.residuals.epsilon_dual
    with fused_tall(solve_mod, "1"):
        batch, tagsb, single, tags1 = rs.run_both(solve_mod, probs, dtype, {})
    rs.assert_identical(batch, single)
    cb = rs.base_counts(tagsb)
    most = max(rs.sweeps(st) for st, _ in batch)
    assert cb.get("batch_lasso_tall_cols", 0) == cb.get("batch_symv_packed_tiles", 0) == most, cb
    assert "lasso_tall_cols" not in cb and cb.get("lasso_tall_rhs", 0) == len(probs), sorted(cb)
    setup = rs.setup_counts(tagsb, ("spd_inverse", "pack_inverse"))
    assert sorted(setup.values()) == [1, 1], setup
    assert rs.base_counts(tags1).get("lasso_tall_cols", 0) >= rs.sweeps(single[0][0])


def test_two_right_hand_sides_share_a_group(solve_mod):
    shape = (2051, 1027)
    m, n = shape
    A, b = problems.regression_data(m, n, seed=0)
    b2 = 0.5 * b + 0.3 * np.random.RandomState(5).randn(m)
    probs = [problems.lasso_ir(ir.dense_matrix(A), ir.constant(v), 0.2 * np.abs(A.T.dot(v)).max(), n) for v in (b, b2)]
    with fused_tall(solve_mod, "1"):
        batch, tagsb, single, _ = rs.run_both(solve_mod, probs, "f32", {}, max_iterations=40)
    rs.assert_identical(batch, single)
    cb = rs.base_counts(tagsb)
    assert cb.get("batch_lasso_tall_cols", 0) == max(rs.sweeps(st) for st, _ in batch), cb
    assert not np.array_equal(np.frombuffer(batch[0][1][problems.LASSO_VAR]),
                              np.frombuffer(batch[1][1][problems.LASSO_VAR]))


def test_below_the_packed_floor_members_are_solved_singly(solve_mod):
    probs = lambda_path((601, 256), (0.4, 0.2, 0.1))
    with fused_tall(solve_mod, "1"):
        batch, tagsb, single, _ = rs.run_both(solve_mod, probs, "f32", {}, max_iterations=40)
    rs.assert_identical(batch, single)
    cb = rs.base_counts(tagsb)
    assert "batch_lasso_tall_cols" not in cb, sorted(cb)
    assert cb.get("lasso_tall_cols", 0) >= sum(rs.sweeps(st) for st, _ in batch), cb
