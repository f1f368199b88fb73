"""A census of route recognition (csrc/fused_route.cc): ONE table of problem, dtype, driver and
options -> the route the solve takes.  Every accepted form of every fused route has a row, and so has
every neighbour that must keep the generic operator path: a gate that grows too wide moves a
"generic" row onto a kernel, one that shrinks moves a fused row off it - and the second kind passes
every "fused equals generic" test of the route modules.

A row is solved for five sweeps (one residual check) with the profile on, and its route is read from
the launch tags of the sweep, the tags the route's own module asserts (test_gpu_fused_tall.py,
test_gpu_fused_matrix.py, test_gpu_fused_zero*.py).  Shapes are the smallest of those modules: fat
256 x 601, tall 601 x 256, the tall logistic form under "auto" 1201 x 512, and 252 rows / columns for
"just below a floor" (252 still meets the pass's shape conditions: a multiple of 4).  A fat lasso of
256 rows is below the whitening floor (2048 rows), so its rows are the explicit-inverse form of the
lasso route.

Every row sets the four route options it can depend on ("auto", the library's default, unless the row
says otherwise) and puts them back."""

import contextlib

import numpy as np
import pytest

from epsilon_amd import ir, problems
from epsilon_amd.wire import ProxFunction
from tests import route_support as rs

pytestmark = pytest.mark.gpu

FAT, TALL, TALL_SMOOTH = (256, 601), (601, 256), (1201, 512)
FAT_BELOW, TALL_BELOW = (252, 601), (600, 252)
SWEEPS = dict(max_iterations=5, epoch_iterations=5)

# the sweep's launches by route; a tag of this universe that a row's route does not name must be absent
ROUTES = {
    "generic": (),
    "lasso": ("lasso_fused",),              # the pass over A (two-block driver: kChainTwoBlock, the same tag)
    "lasso_tall": ("lasso_tall_cols",),
    "matrix": ("batch_fused_pass",),        # the columns of a matrix variable as members of the batched pass
    "basis_pursuit": ("zero_fused",),       # no z block: the partials go through the reduction
    "zero_fat": ("zero_fused", "zero_fused_rows"),
    "zero_tall": ("zero_tall", "zero_tall_cols"),
    "zero_tall_smooth": ("zero_tall_dot", "zero_tall_samples", "zero_tall_acc", "zero_tall_cols"),
}
SWEEP_TAGS = sorted({t for tags in ROUTES.values() for t in tags} | {"wide_back", "batch_zero_pass", "batch_zero_rows"})

# the options of the tall routes and of the ridge term; route_support's scope has no row for two of them
ROUTE_OPTIONS = ("fused_tall", "fused_zero_tall", "fused_zero_tall_smooth", "fused_zero_ridge")


@contextlib.contextmanager
def route_options(mod, values):
    try:
        for key in ROUTE_OPTIONS:
            mod.set_option(key, values.get(key, "auto"))
        yield
    finally:
        for key in ROUTE_OPTIONS:
            mod.set_option(key, "auto")


# ---- problems ------------------------------------------------------------------------------------------
def offset_lasso(m, n):
    """the lasso with a constant in the penalty's argument: lam ||x + c||_1"""
    A, b = problems.regression_data(m, n, seed=0)
    x, y = ir.variable(n, 1, problems.LASSO_COPY), ir.variable(n, 1, problems.LASSO_VAR)
    f0 = ir.prox(ProxFunction.SUM_SQUARE, ir.add(ir.linear_map(ir.dense_matrix(A), x),
                                                 ir.linear_map(ir.scalar(-1, m), ir.constant(b))), alpha=1.0)
    f1 = ir.prox(ProxFunction.NORM_1, ir.add(y, ir.constant(np.linspace(-0.1, 0.1, n))),
                 alpha=0.2 * np.abs(A.T.dot(b)).max())
    return ir.Problem([f0, f1], [ir.zero(ir.add(x, ir.linear_map(ir.scalar(-1, n), y)))])


def hinge_groups(m, n):
    """hinge_l1 with the penalty on x as a group norm of its rows (NORM_2, axis 1, on the n x 1
    variable): the nearest form to a group-lasso term that a ZERO-term problem can carry"""
    C, lam = [problems.hinge_l1(m, n)[1][k] for k in ("C", "lam")]

    def terms(x, z):
        arg = ir.add(ir.linear_map(ir.scalar(-1, m), z), ir.scalar_constant(1.0, (m, 1)))
        return [ir.prox(ProxFunction.SUM_HINGE, arg), ir.prox(ProxFunction.NORM_2, x, alpha=lam, has_axis=True, axis=1)]
    return problems._graph_form(terms, C, None)


def deadzone_penalty(m, n):
    """the lasso's data with a deadzone penalty on 2 x: a zone with M and a map that is not the identity"""
    A, b = problems.regression_data(m, n, seed=0)
    return rs.fused_problem(ir.dense_matrix(A), m, n, ir.constant(b), 0.2 * np.abs(A.T.dot(b)).max(), "deadzone")


def first(generator, *fixed):
    return lambda m, n: generator(m, n, *fixed)[0]


make = rs.memoised({
    "lasso": first(problems.lasso),
    "deadzone_penalty": deadzone_penalty,
    "offset_lasso": offset_lasso,
    "mv_lasso": first(problems.mv_lasso, 3),
    "group_lasso": first(problems.group_lasso, 3),
    "basis_pursuit": first(problems.basis_pursuit),
    "hinge_l1": first(problems.hinge_l1),
    "deadzone_l1": first(problems.deadzone_l1),
    "logreg_l1": first(problems.logreg_l1),
    "hinge_l2": first(problems.hinge_l2),
    "svr_l2": first(problems.svr_l2),
    "logreg_l2": first(problems.logreg_l2),
    "hinge_groups": hinge_groups,
    "least_abs_dev": first(problems.least_abs_dev),
    "quantile": first(problems.quantile),
    "lp": first(problems.lp),
    "fused_lasso": lambda m, n: problems.fused_lasso(m, 3, n // 3)[0],
})

# ---- the table -----------------------------------------------------------------------------------------
MULTI, TWO_BLOCK = 0, 1  # SolverParams.solver
ON = {"fused_zero_tall_smooth": "1"}
BOTH = ("f32", "f64")


def rows(problem, shape, route, options=None, driver=MULTI, dtypes=("f32",)):
    return [(problem, shape, dt, driver, dict(options or {}), route) for dt in dtypes]


CENSUS = (
    # -- the lasso route: zone without offset, or row groups with cols > 1
    rows("lasso", FAT, "lasso", dtypes=BOTH)
    + rows("deadzone_penalty", FAT, "lasso", dtypes=BOTH)
    + rows("lasso", TALL, "lasso_tall", dtypes=BOTH)
    + rows("deadzone_penalty", TALL, "lasso_tall", dtypes=BOTH)
    + rows("mv_lasso", FAT, "matrix", dtypes=BOTH)
    + rows("group_lasso", FAT, "matrix", dtypes=BOTH)
    # -- the two-block route: zone without offset
    + rows("lasso", FAT, "lasso", driver=TWO_BLOCK, dtypes=BOTH)
    # -- the ZERO route: x zone without offset or ridge; z zone with optional offset, or smooth
    + rows("basis_pursuit", FAT, "basis_pursuit", dtypes=BOTH)
    + rows("hinge_l1", FAT, "zero_fat", dtypes=BOTH)       # z: a zone with an offset
    + rows("deadzone_l1", FAT, "zero_fat", dtypes=BOTH)    # z: a zone without one
    + rows("logreg_l1", FAT, "zero_fat", dtypes=BOTH)      # z: smooth
    + rows("hinge_l1", TALL, "zero_tall", dtypes=BOTH)
    + rows("deadzone_l1", TALL, "zero_tall", dtypes=BOTH)
    + rows("logreg_l1", TALL_SMOOTH, "zero_tall_smooth", dtypes=BOTH)        # "auto": from 512 columns
    + rows("logreg_l1", TALL, "zero_tall_smooth", ON, dtypes=BOTH)           # "1": from 256
    + rows("hinge_l2", FAT, "zero_fat", dtypes=BOTH)
    + rows("svr_l2", FAT, "zero_fat", dtypes=BOTH)
    + rows("logreg_l2", FAT, "zero_fat", dtypes=BOTH)
    + rows("hinge_l2", TALL, "zero_tall", dtypes=BOTH)
    + rows("svr_l2", TALL, "zero_tall", dtypes=BOTH)
    + rows("logreg_l2", TALL, "zero_tall_smooth", ON, dtypes=BOTH)
    + rows("logreg_l2", TALL_SMOOTH, "zero_tall_smooth", dtypes=BOTH)
    # -- forms no route accepts
    + rows("offset_lasso", FAT, "generic")
    + rows("offset_lasso", TALL, "generic")
    + rows("offset_lasso", FAT, "generic", driver=TWO_BLOCK)
    + rows("mv_lasso", FAT, "generic", driver=TWO_BLOCK)
    + rows("mv_lasso", TALL, "generic")                    # the tall form takes vector variables alone
    + rows("group_lasso", TALL, "generic")
    + rows("hinge_groups", FAT, "generic")
    + rows("hinge_groups", TALL, "generic")
    + rows("hinge_l1", FAT, "generic", driver=TWO_BLOCK)
    + rows("hinge_l2", FAT, "generic", driver=TWO_BLOCK)
    + rows("lasso", TALL, "generic", driver=TWO_BLOCK)
    # (x lives in the ZERO term alone in the first two: with fat A its system is singular, so tall only)
    + rows("least_abs_dev", TALL, "generic")
    + rows("quantile", TALL, "generic")
    + [row for problem in ("lp", "fused_lasso") for shape in (FAT, TALL) for row in rows(problem, shape, "generic")]
    # -- each tall route, and the ridge term, with its option "0"
    + rows("lasso", TALL, "generic", {"fused_tall": "0"})
    + rows("hinge_l1", TALL, "generic", {"fused_zero_tall": "0"})
    + rows("logreg_l1", TALL_SMOOTH, "generic", {"fused_zero_tall": "0"})
    + rows("logreg_l1", TALL_SMOOTH, "generic", {"fused_zero_tall_smooth": "0"})
    + rows("hinge_l2", FAT, "generic", {"fused_zero_ridge": "0"})
    + rows("hinge_l2", TALL, "generic", {"fused_zero_ridge": "0"})
    + rows("logreg_l2", TALL_SMOOTH, "generic", {"fused_zero_ridge": "0"})
    + rows("logreg_l2", TALL_SMOOTH, "generic", {"fused_zero_tall_smooth": "0"})
    # -- each floor of "auto" from just below
    + rows("lasso", TALL_BELOW, "generic")
    + rows("hinge_l1", TALL_BELOW, "generic")
    + rows("hinge_l1", FAT_BELOW, "generic")
    + rows("logreg_l1", TALL, "generic")                   # the smooth form's floor is 512 columns
    + rows("logreg_l2", TALL, "generic")
    + rows("hinge_l2", TALL_BELOW, "generic")
    + rows("svr_l2", FAT_BELOW, "generic")
    + rows("logreg_l2", TALL_BELOW, "generic", ON)
)


def row_id(row):
    problem, shape, dtype, driver, options, route = row
    words = ["%s=%s" % (k.replace("fused_", ""), v) for k, v in sorted(options.items())]
    return "-".join([problem, "%dx%d" % shape, dtype, "two_block" if driver == TWO_BLOCK else "multi"] + words)


def route_of(counts):
    return {t: counts[t] for t in SWEEP_TAGS if t in counts}


@pytest.mark.parametrize("row", CENSUS, ids=row_id)
def test_route(solve_mod, row):
    problem, shape, dtype, driver, options, route = row
    with route_options(solve_mod, options):
        st, _, counts = rs.Routes(solve_mod, ()).solve(make(problem, shape), dtype, solver=driver, **SWEEPS)
    n = rs.sweeps(st)
    got = route_of(counts)
    print(row_id(row), "ran", n, "sweeps:", got)
    assert n == 5
    assert got == {t: n for t in ROUTES[route]}, (route, got)


@pytest.mark.parametrize("shape,route", [(FAT, "zero_fat"), (TALL, "zero_tall")])
def test_a_ridge_member_of_a_batch_is_solved_by_itself(solve_mod, shape, route):
    """the batched kernels have no ridge head: the members' launches are their single solves' own"""
    probs = [problems.hinge_l2(*shape, lam=lam)[0] for lam in (1.0, 0.5)]
    with route_options(solve_mod, {}):
        batch, tagsb, single, tags1 = rs.run_both(solve_mod, probs, "f32", {"batch_zero_tall": "1"}, **SWEEPS)
    cb, c1 = rs.base_counts(tagsb), rs.base_counts(tags1)
    assert route_of(c1) == {t: 5 for t in ROUTES[route]}, route_of(c1)
    assert route_of(cb) == {t: 2 * c for t, c in route_of(c1).items()}, route_of(cb)
    assert not [t for t in cb if t.startswith("batch_")], sorted(cb)
    rs.assert_identical(batch, single)
