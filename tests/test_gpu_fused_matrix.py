"""The fused sweep for matrix variables (option "fused_matrix"): the k columns of
X (n x k) under the data map I_k (x) A run as k members of the batched pass or of the wide kernels
inside ONE solve, with the joint stopping test; for group lasso the threshold couples the members
of a row.  Problems: problems.mv_lasso(m, n, k, rho) and problems.group_lasso(m, n, k), seed 0.

Tolerances are the project's own: against the oracle as in test_more_benchmark_problems
(test_gpu_parity.py: f64 rtol 1e-6, atol 1e-8; f32 rtol = atol = 5e-3, equal state and stopping
sweep), whitened against explicit as in test_gpu_fused_whiten.py (atol 2e-4 max|x|).

The mv shapes stop with a margin on both sides in the oracle (r / eps_pri <= 0.82 at the stopping
check, >= 1.15 at the check before), so f32 rounding cannot move the stopping sweep."""

import math

import numpy as np
import pytest

from epsilon_amd import ir, problems, wire
from tests import route_support as rs

pytestmark = pytest.mark.gpu

BATCH_TAGS = {"batch_fused_pass", "batch_reduce_partials", "batch_symv_packed"}
WIDE_TAGS = {"wide_back", "wide_forward", "wide_reduce"}
X, XP = "var:X", "separate:var:X:sum_square"
SETUP = ("gemm", "syrk", "spd_inverse")  # what setup_counts counts here
# routes.solve(prob, dtype, route, fused, **solver params): the options of a solve here
ROUTE_OPTIONS = (("route", "fused_matrix", "auto"), ("fused", "fused", "1"))


def assert_launches(c, tag, st, per_sweep):
    """`per_sweep` launches of `tag` in every sweep.  A residual check that is far from the
    tolerances has the next epoch's sweeps enqueued behind it (Solver::Run); when that check says
    OPTIMAL they are discarded and not counted, so up to one epoch of 10 sweeps more was launched."""
    n = c.get(tag, 0)
    assert n % per_sweep == 0 and n // per_sweep in (rs.sweeps(st), rs.sweeps(st) + 10), (tag, n, rs.sweeps(st), per_sweep)


@pytest.fixture
def routes(solve_mod):
    return rs.Routes(solve_mod, ROUTE_OPTIONS, raw_tags=True)


def make(kind, shape):
    if kind == "mv":
        m, n, k, rho = shape
        return problems.mv_lasso(m, n, k, rho=rho)[0]
    if kind == "group":
        m, n, k = shape
        return problems.group_lasso(m, n, k)[0]
    m, n, k, frac = shape  # "group_at": the same data, weight frac * the default one
    lam = problems.group_lasso(m, n, k)[1]["lam"]
    return problems.group_lasso(m, n, k, lam=frac * lam)[0]


oracle = rs.oracle_of(make)


# ---- 1. mv lasso, pass route, against the oracle -----------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("shape,stop", [((256, 301, 3, 0.1), 20),    # odd n, ragged column pair, nk < width
                                        ((256, 301, 10, 0.1), 30)])  # two launches: 8 + 2
def test_mv_pass_route_matches_oracle(routes, dtype, shape, stop):
    so, xo = oracle("mv", shape)
    assert so.state == wire.SolverStatus.OPTIMAL and so.num_iterations == stop
    st, x, tags = routes.solve(make("mv", shape), dtype, "pass")
    c = rs.base_counts(tags)
    assert_launches(c, "batch_fused_pass", st, math.ceil(shape[2] / 8))
    assert not WIDE_TAGS & set(c) and "lasso_fused" not in c, sorted(c)
    rs.assert_matches_oracle(st, x, so, xo, dtype)


# ---- 2. mv lasso, wide route, f32, against the oracle ------------------------------------------------
@pytest.mark.parametrize("shape,route", [((256, 301, 10, 0.1), "auto"),    # the default takes it from k = 8
                                         ((256, 301, 17, 0.01), "wide")])  # two tiles, n no multiple of 4
def test_mv_wide_route_matches_oracle(routes, shape, route):
    so, xo = oracle("mv", shape)
    assert so.state == wire.SolverStatus.OPTIMAL and so.num_iterations == 30
    st, x, tags = routes.solve(make("mv", shape), "f32", route)
    c = rs.base_counts(tags)
    assert_launches(c, "wide_back", st, 1)
    assert WIDE_TAGS <= set(c), sorted(c)
    assert "batch_fused_pass" not in c and "lasso_fused" not in c, sorted(c)
    rs.assert_matches_oracle(st, x, so, xo, "f32")


# ---- 3. the forms of the inverse apply, against the generic path in the same process -----------------
@pytest.mark.parametrize("shape,dtype,route,form", [
    ((1024, 1500, 3, 0.05), "f32", "pass", "batch_symv_packed"),  # packed inverse
    ((1024, 1500, 3, 0.05), "f64", "pass", "batch_symv_packed"),
    ((2052, 3000, 7, 0.05), "f32", "pass", "batch_symv_packed"),  # width 6: launches 6 + 1
    ((2048, 4100, 5, 0.05), "f32", "pass", "whitened"),
    ((2048, 4100, 9, 0.05), "f32", "wide", "whitened")])
def test_inverse_apply_forms_match_generic_path(routes, shape, dtype, route, form):
    prob = make("mv", shape)
    st, x, tags = routes.solve(prob, dtype, route)
    sg, xg, tg = routes.solve(prob, dtype, route, fused="0")
    c, cg = rs.base_counts(tags), rs.base_counts(tg)
    assert not (BATCH_TAGS | WIDE_TAGS) & set(cg), sorted(cg)
    if route == "pass":
        width = 6 if shape[0] == 2052 else 8  # four 16-byte chunks per thread from m = 2049 on
        assert_launches(c, "batch_fused_pass", st, math.ceil(shape[2] / width))
    else:
        assert_launches(c, "wide_back", st, 1)
    if form == "whitened":
        assert not any(t.startswith(("symv", "batch_symv")) for t in c), sorted(c)
    else:
        assert c.get(form, 0) > 0, sorted(c)
    a, g = rs.status(st), rs.status(sg)
    print("fused: state %d at %d | generic: state %d at %d" % (a.state, a.num_iterations, g.state, g.num_iterations))
    assert a.state == g.state
    assert sorted(x) == sorted(xg)
    for k in xg:
        scale = np.abs(xg[k]).max()
        print(k, "max |fused - generic| %.3g, max |generic| %.3g" % (np.abs(x[k] - xg[k]).max(), scale))
        if form == "whitened":
            np.testing.assert_allclose(x[k], xg[k], rtol=0, atol=2e-4 * scale, err_msg=k)
        elif dtype == "f64":
            np.testing.assert_allclose(x[k], xg[k], rtol=1e-6, atol=1e-8, err_msg=k)
        else:
            np.testing.assert_allclose(x[k], xg[k], rtol=5e-3, atol=5e-3, err_msg=k)


# ---- 4. group lasso -----------------------------------------------------------------------------------
def row_norms(x, k):
    return np.sqrt((x.reshape(-1, k, order="F") ** 2).sum(axis=1))


GROUP_CASES = [("f32", 3, "pass", "batch_fused_pass"), ("f64", 3, "pass", "batch_fused_pass"),
               ("f32", 8, "pass", "batch_fused_pass"), ("f64", 8, "pass", "batch_fused_pass"),  # k = width
               ("f64", 9, "auto", None),  # more columns than one launch carries: the generic path
               ("f32", 9, "auto", "wide_back"), ("f32", 20, "auto", "wide_back")]


def check_group(routes, kind, shape, dtype, route, tag):
    so, xo = oracle(kind, shape, max_iterations=60)
    assert so.state == wire.SolverStatus.MAX_ITERATIONS_REACHED
    st, x, tags = routes.solve(make(kind, shape), dtype, route, max_iterations=60)
    c = rs.base_counts(tags)
    if tag is None:
        assert not (BATCH_TAGS | WIDE_TAGS) & set(c), sorted(c)
    else:
        assert c.get(tag) == 60 and "lasso_fused" not in c, c
    rs.assert_matches_oracle(st, x, so, xo, dtype)
    k = shape[2]
    zero_g, zero_o = row_norms(x[X], k) == 0, row_norms(xo[X], k) == 0
    print("rows exactly zero: gpu %d, oracle %d of %d" % (zero_g.sum(), zero_o.sum(), zero_o.size))
    return zero_g, zero_o


@pytest.mark.parametrize("dtype,k,route,tag", GROUP_CASES)
def test_group_lasso_matches_oracle(routes, dtype, k, route, tag):
    """problems.group_lasso(256, 301, k) with its default weight, 60 sweeps.  The oracle ends in
    MAX_ITERATIONS_REACHED with EVERY row of X exactly zero here (k = 3, 8, 9, 20: 301 of 301;
    the first non-zero rows appear well after sweep 60, 29 of them by sweep 300 at k = 3), so these
    cases exercise the zero branch of the shrink only; the rows the GPU result zeroes must be the
    oracle's.  test_group_lasso_both_branches covers the other branch."""
    zero_g, zero_o = check_group(routes, "group", (256, 301, k), dtype, route, tag)
    assert np.array_equal(zero_g, zero_o)


@pytest.mark.parametrize("dtype,k,route,tag", GROUP_CASES)
def test_group_lasso_both_branches(routes, dtype, k, route, tag):
    """The same data at 0.3 of the default weight: after 60 sweeps the oracle has some rows of X
    non-zero and most exactly zero, so both branches of the shrink are exercised; both must occur in
    the GPU result.  (A row whose norm lies within rounding of the weight may fall on either side
    in f32, so the sets are compared in f64 only.)"""
    zero_g, zero_o = check_group(routes, "group_at", (256, 301, k, 0.3), dtype, route, tag)
    assert 0 < (~zero_o).sum() < zero_o.sum()
    assert (~zero_g).sum() > 0 and zero_g.sum() > 0
    if dtype == "f64":
        assert np.array_equal(zero_g, zero_o)


# ---- 5. route and setup, by profile tags ----------------------------------------------------------------
@pytest.mark.parametrize("shape,route", [((256, 301, 3, 0.1), "pass"), ((256, 301, 10, 0.1), "pass"),
                                         ((256, 301, 10, 0.1), "wide")])
def test_route_and_setup_tags(routes, shape, route):
    """25 sweeps without the stopping test, so that every launched sweep counts."""
    m, n, k, rho = shape
    fixed = dict(max_iterations=25, ignore_stopping_criteria=True)
    prob, info = problems.mv_lasso(m, n, k, rho=rho)
    st, x, tags = routes.solve(prob, "f32", route, **fixed)
    assert rs.sweeps(st) == 25
    c = rs.base_counts(tags)
    assert "lasso_fused" not in c, sorted(c)
    if route == "pass":
        assert c.get("batch_fused_pass") == rs.sweeps(st) * math.ceil(k / 8), c
        assert c.get("batch_reduce_partials") == rs.sweeps(st) and not WIDE_TAGS & set(c), c
    else:
        assert c.get("wide_back") == c.get("wide_forward") == c.get("wide_reduce") == rs.sweeps(st), c
        assert not BATCH_TAGS & set(c), sorted(c)
    # the Gram product and the inverse are formed once for all k columns: the setup of ONE vector lasso
    vec = problems.lasso_ir(ir.dense_matrix(info["A"]), ir.constant(info["B"][:, 0]), info["lam"], n)
    _, _, tv = routes.solve(vec, "f32", **fixed)
    assert "lasso_fused" in rs.base_counts(tv)
    setup = rs.setup_counts(tags, SETUP)
    if route == "wide":
        # the wide sweep's own product, the cached inverse times the panel of 64 members (once at
        # Init, once per sweep and contraction range), carries the gemm tag too: not setup
        panel = [t for t in setup if t not in rs.setup_counts(tv, SETUP)]
        assert panel and all(t.startswith("gemm:%dx" % (64 * m)) for t in panel), panel
        assert all(setup.pop(t) % (rs.sweeps(st) + 1) == 0 for t in panel), rs.setup_counts(tags, SETUP)
    assert rs.setup_counts(tv, SETUP) and setup == rs.setup_counts(tv, SETUP), (setup, rs.setup_counts(tv, SETUP))
    _, x0, t0 = routes.solve(prob, "f32", "0", **fixed)
    assert not (BATCH_TAGS | WIDE_TAGS | {"lasso_fused"}) & set(rs.base_counts(t0)), sorted(rs.base_counts(t0))


# ---- 6. below the floor of 256 rows -----------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape", [("mv", (30, 40, 3, 0.1)), ("group", (30, 20, 3))])
def test_small_problems_keep_the_generic_path(routes, kind, shape):
    st, x, tags = routes.solve(make(kind, shape), "f64", max_iterations=60)
    c = rs.base_counts(tags)
    assert c and not (BATCH_TAGS | WIDE_TAGS | {"lasso_fused"}) & set(c), sorted(c)
    # ... and the routes themselves are taken from 256 rows on (what fails without the fused sweep)
    big = {"mv": (256, 301, 3, 0.1), "group": (256, 301, 3)}[kind]
    _, _, tb = routes.solve(make(kind, big), "f64", max_iterations=20)
    assert "batch_fused_pass" in rs.base_counts(tb), sorted(rs.base_counts(tb))


# ---- 7. handles: two runs continue where one would ---------------------------------------------------------
def handle_run(mod, prob, route, chunks):
    with rs.options(mod, fused_matrix=route):
        s = mod.Solver(prob.SerializeToString(), wire.SolverParams().SerializeToString(), prob.expression_data())
        try:
            s.init()
            for n in chunks:
                assert s.run(n) == n
            st, x = s.result()
        finally:
            s.close()
    return st, x


@pytest.mark.parametrize("route", ["pass", "wide"])
def test_two_runs_continue_where_one_would(solve_mod, route):
    prob = make("mv", (256, 301, 10, 0.1))
    _, two = handle_run(solve_mod, prob, route, [5, 5])
    _, one = handle_run(solve_mod, prob, route, [10])
    assert sorted(one) == sorted(two) == sorted([X, XP])
    rs.assert_same_arrays(one, two)


# ---- 8. the same solve twice ----------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["pass", "wide"])
def test_same_solve_twice_same_bytes(routes, route):
    prob = make("mv", (256, 301, 10, 0.1))
    sa, xa, _ = routes.solve(prob, "f32", route)
    sb, xb, _ = routes.solve(prob, "f32", route)
    assert rs.status(sa).num_iterations == rs.status(sb).num_iterations
    rs.assert_same_arrays(xa, xb)


# ---- 9. inside a batch the matrix-variable problem runs alone ---------------------------------------------------
def test_in_a_batch_the_mv_problem_runs_alone(solve_mod):
    m, n, k = 256, 301, 3
    mv, info = problems.mv_lasso(m, n, k, rho=0.1)
    A, B, lam = info["A"], info["B"], info["lam"]
    lassos = [problems.lasso_ir(ir.dense_matrix(A), ir.constant(B[:, c]), f * lam, n) for c, f in ((0, 1.0), (1, 0.7))]
    probs = [mv] + lassos
    data = rs.union_data(probs)
    sb = wire.SolverParams().SerializeToString()
    pbs = [p.SerializeToString() for p in probs]
    batch = solve_mod.solve_batch(pbs, None, sb, data)
    st, x = solve_mod.solve(pbs[0], [], sb, data)
    rs.assert_same_bytes(batch[0][0], batch[0][1], st, x)
    for i in (1, 2):  # the two vector problems still form their group
        sti, xi = solve_mod.solve(pbs[i], [], sb, data)
        rs.assert_same_arrays(batch[i][1], xi, i)
