"""The one-launch residual check of the fused ZERO-term routes (DESIGN.md 3.11 "The residual check",
option "fused_zero_check"): with the option "1" a check is ONE launch (tag "zero_fused_norms" on the
fat route, "zero_tall_norms" on the tall ones) that sums, per constraint side, five squares in double;
the host finishes the closed form, and the driver pipelines the next epoch's sweeps behind the check
and restores a snapshot when the check says OPTIMAL.  Every solve here sets "fused_zero_check" through
`check_option`, which puts "0", the library's default, back; the routes themselves are switched on by
"fused_zero_tall" = "fused_zero_tall_smooth" = "fused_zero_ridge" = "fused_zero_xfree" = "1".

Kinds (seed 0): hinge_l1 with lambda = 0.01 max|sum_i C_i| and deadzone_l1 with frac = 0.005 (two
sides, zones); basis_pursuit (fat, the x side alone); least_abs_dev and quantile with tau = 0.5 (tall,
free x: the z side alone); logreg_l1 (a carried head; tall: lambda = 0.05 of the generator's scale,
fat: its default 0.1); hinge_l2 (a ridge term on x; lambda 0.1 tall, 1.0 fat).  Shapes: tall
(601, 256) - the x side below one workgroup's stride of the norms kernel, the z side ragged - and
(2051, 1028) - two and three workgroups, ragged tails, the packed apply; fat (256, 601), the row
floor, and (260, 1031).  Every kind runs in f32 and f64.

Tolerances are the project's own: against the oracle rs.TOLERANCES; the four residual fields with the
option on against the same solve with it off in f64 within 1e-9 relative, the bound of the other
fused-against-generic ZERO tests, and in f32 within rs.TOLERANCES["f32"].

Stopping rule (default tolerances, epoch 10), chosen on the CPU oracle: both r / eps_pri and
s / eps_dual are outside [0.95, 1.05] at the stopping check and at the check before it.  Cell: stop;
(r, s ratios) at the stop | at the check before.  15 cells, at least one per kind:
  hinge_l1      (2051, 1028): 50; (0.895, 0.589) | (1.090, 0.765)
  hinge_l1      (260, 1031):  50; (0.840, 0.350) | (1.124, 0.438)
  deadzone_l1   (601, 256):   40; (0.801, 0.295) | (1.143, 0.452)
  deadzone_l1   (256, 601):   50; (0.572, 0.886) | (0.677, 1.146)
  basis_pursuit (256, 601):   60; (0.831, 0.297) | (1.239, 0.331)
  basis_pursuit (260, 1031):  70; (0.828, 0.324) | (1.091, 0.350)
  least_abs_dev (601, 256):   40; (0.765, 0.875) | (1.062, 1.163)
  quantile      (601, 256):   60; (0.270, 0.840) | (0.322, 1.092)
  logreg_l1     (601, 256):   40; (0.902, 0.886) | (1.279, 1.275)
  logreg_l1     (2051, 1028): 70; (0.926, 0.318) | (1.078, 0.380)
  logreg_l1     (256, 601):   60; (0.838, 0.358) | (1.238, 0.470)
  logreg_l1     (260, 1031):  80; (0.902, 0.200) | (1.141, 0.275)
  hinge_l2      (601, 256):   30; (0.200, 0.427) | (0.488, 1.070)
  hinge_l2      (2051, 1028): 30; (0.181, 0.410) | (0.486, 1.131)
  hinge_l2      (260, 1031):  10; (0.873, 0.285) | (43.4, 136) at the check after sweep 0
Not used, a ratio inside the window: hinge_l1 (601, 256) 0.977 and (256, 601) 0.954 at the stop;
least_abs_dev (2051, 1028) 0.995 before; quantile (2051, 1028) 0.940 at the stop is kept out as too
close; hinge_l2 (256, 601) 0.981 at the stop.  test_stops_with_the_oracle asserts the window on the
oracle's own ratios, so a cell that drifts into it fails there.  hinge_l2 (260, 1031) stops at the
first check after the one at sweep 0, which is far from optimal: its ten speculative sweeps are
discarded there, the default epoch's own case of a restore.

Speculation and restore: with epoch_iterations = E the check after sweep 0 is far from optimal (a
ratio above 4, the driver's bound), the driver enqueues the next E sweeps behind it, and the check at iteration E is the
cell's stopping check above (its ratios do not depend on the epoch): OPTIMAL, the snapshot is restored.
Cells and E: least_abs_dev (601, 256) 40; deadzone_l1 (601, 256) 40 and hinge_l1 (260, 1031) 50 (two
sides); logreg_l1 (601, 256) 40 and (256, 601) 60 (the head is in the snapshot).

Groups (abs_tol = rel_tol = 1e-2, three hinge_l1 members with lambda = f max|sum_i C_i|): stop;
ratios at the stop | before.  (601, 256): f = 0.05: 60; (0.872, 0.325) | (1.068, 0.357); 0.02: 30;
(0.930, 0.758) | (1.297, 1.087); 0.01: 40; (0.503, 0.695) | (0.598, 1.091).  (256, 601): 0.05: 60;
(0.940, 0.146) | (1.135, 0.160); 0.02: 30; (0.738, 0.281) | (1.174, 0.311); 0.01: 20; (0.545, 0.292) |
(1.188, 0.360)."""

import contextlib

import numpy as np
import pytest

from epsilon_amd import problems, wire
from oracle import epsilon_oracle as orc
from tests import route_support as rs

pytestmark = pytest.mark.gpu

T1, T2, F1, F2 = (601, 256), (2051, 1028), (256, 601), (260, 1031)
FIXED = dict(max_iterations=23, abs_tol=0.0, rel_tol=0.0)
FIXED_CHECKS = 4  # after sweeps 0, 10 and 20, and the final one of a solve that ends on max_iterations
# routes.solve(prob, dtype, check, **options by name, **solver params)
ROUTE_OPTIONS = (("tall", "fused_zero_tall", "1"), ("tall_smooth", "fused_zero_tall_smooth", "1"),
                 ("fused", "fused", "1"), ("fused_zero", "fused_zero", "auto"))
ON = rs.switched_on(ROUTE_OPTIONS)  # what the handles and the batches set beside this module's own options
NORMS = ("zero_fused_norms", "zero_tall_norms")


def is_tall(shape):
    return shape[0] > shape[1]


# ---- the options of this module: route_support's scope has no row for them ---------------------------
@contextlib.contextmanager
def check_option(mod, value):
    """"fused_zero_check" = value for the block; "0", the library's default, on every way out.  With it
    "fused_zero_ridge" = "fused_zero_xfree" = "1", put back to "auto" and "0", theirs."""
    try:
        mod.set_option("fused_zero_ridge", "1")
        mod.set_option("fused_zero_xfree", "1")
        mod.set_option("fused_zero_check", value)
        yield
    finally:
        mod.set_option("fused_zero_check", "0")
        mod.set_option("fused_zero_xfree", "0")
        mod.set_option("fused_zero_ridge", "auto")


class Routes(rs.Routes):
    def solve(self, prob, dtype="f32", check="1", **params):
        with check_option(self.mod, check):
            return super(Routes, self).solve(prob, dtype, **params)


@pytest.fixture
def routes(solve_mod):
    return Routes(solve_mod, ROUTE_OPTIONS)


def hinge_member(m, n, f):
    return problems.hinge_l1(m, n, lam=f * rs.lam_scale("hinge_l1", m, n))[0]


make = rs.memoised({
    "hinge_l1": lambda m, n: hinge_member(m, n, 0.01),
    "deadzone_l1": lambda m, n: problems.deadzone_l1(m, n, frac=0.005)[0],
    "basis_pursuit": lambda m, n: problems.basis_pursuit(m, n)[0],
    "least_abs_dev": lambda m, n: problems.least_abs_dev(m, n)[0],
    "quantile": lambda m, n: problems.quantile(m, n, tau=0.5)[0],
    "logreg_l1": lambda m, n: (problems.logreg_l1(m, n, lam=0.05 * rs.lam_scale("logreg_l1", m, n))[0] if m > n else
                               problems.logreg_l1(m, n)[0]),
    "hinge_l2": lambda m, n: problems.hinge_l2(m, n, lam=0.1 if m > n else 1.0)[0],
})
oracle = rs.oracle_of(make)

SHAPES_OF = {
    "hinge_l1": (T1, T2, F1, F2), "deadzone_l1": (T1, T2, F1, F2), "basis_pursuit": (F1, F2),
    "least_abs_dev": (T1, T2), "quantile": (T1, T2), "logreg_l1": (T1, T2, F1, F2), "hinge_l2": (T1, T2, F1, F2),
}
CELLS = [(kind, shape) for kind, shapes in SHAPES_OF.items() for shape in shapes]
FREE_X = ("least_abs_dev", "quantile")


def sweep_tags(kind, shape):
    """the route's own launches of one sweep, as the existing modules' assert_route helpers have them"""
    if not is_tall(shape):
        return ("zero_fused",) if kind == "basis_pursuit" else ("zero_fused", "zero_fused_rows")
    if kind in FREE_X:
        return ("zero_tall", "zero_tall_free_cols")
    if kind == "logreg_l1":
        return ("zero_tall_dot", "zero_tall_samples", "zero_tall_acc", "zero_tall_cols")
    return ("zero_tall", "zero_tall_cols")


def norms_tag(shape):
    return NORMS[1] if is_tall(shape) else NORMS[0]


def zero_counts(c):
    """the ZERO-route launches of a profile, without the first head of a smooth term (Init's)"""
    return {t: v for t, v in c.items() if t.startswith("zero_") and not t.endswith("_head")}


def assert_route(c, st, kind, shape, checks, discarded=0):
    """every kernel of the route once per sweep (`discarded`: sweeps that ran behind the last check
    and were dropped); `checks` launches of the route's norms kernel under its own tag (0: neither
    tag), nothing of the other route, of the lasso route or of a batch"""
    n = rs.sweeps(st) + discarded
    want = {t: n for t in sweep_tags(kind, shape)}
    if checks:
        want[norms_tag(shape)] = checks
    assert zero_counts(c) == want, (zero_counts(c), want)
    assert "lasso_fused" not in c and not [t for t in c if t.startswith("batch_")], sorted(c)


def residuals(st):
    r = rs.status(st).residuals
    return {f: getattr(r, f) for f in rs.STATUS_FIELDS}


def assert_residuals_close(st, st0, dtype):
    """the four residual fields of `st` (option on) against `st0` (off)"""
    a, b = residuals(st), residuals(st0)
    for f in rs.STATUS_FIELDS:
        print("%s: on %.17g, off %.17g, relative difference %.3g" % (
            f, a[f], b[f], abs(a[f] - b[f]) / abs(b[f]) if b[f] else abs(a[f])))
    for f in rs.STATUS_FIELDS:
        if dtype == "f64":
            assert abs(a[f] - b[f]) <= 1e-9 * abs(b[f]), f
        else:
            np.testing.assert_allclose(a[f], b[f], err_msg=f, **rs.TOLERANCES["f32"])


# ---- 1. values: the closed form against the generic check -------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kind,shape", CELLS)
def test_the_check_has_the_generic_values(routes, kind, shape, dtype):
    """23 sweeps with the tolerances at zero: two epoch checks are passed and the final check lands off
    the epoch.  The same again under the default tolerances with the stopping rule ignored, where the
    two tolerances are not zero: they carry max_norm and ||A^T u||."""
    prob = make(kind, shape)
    so, xo = oracle(kind, shape, **FIXED)
    assert so.state == wire.SolverStatus.MAX_ITERATIONS_REACHED and so.num_iterations == 23
    assert so.residuals.r_norm > 0 and so.residuals.s_norm > 0
    for params in (FIXED, dict(max_iterations=23, ignore_stopping_criteria=True)):
        st, x, c = routes.solve(prob, dtype, "1", **params)
        st0, x0, c0 = routes.solve(prob, dtype, "0", **params)
        assert_route(c, st, kind, shape, FIXED_CHECKS)
        assert_route(c0, st0, kind, shape, 0)
        rs.assert_same_bytes(st, x, st0, x0, params)  # the check writes no state
        assert_residuals_close(st, st0, dtype)
        if params is not FIXED:
            assert residuals(st0)["epsilon_primal"] > 0 and residuals(st0)["epsilon_dual"] > 0
    st, x, _ = routes.solve(prob, dtype, "1", **FIXED)
    rs.assert_matches_oracle(st, x, so, xo, dtype)


# ---- 2. launches: one per check, nothing else between sweeps ----------------------------------------
def loop_profiles(mod, prob, dtype, check, pieces):
    """the launches of each piece of a solve of FIXED on a handle, Init's left out: [base_counts]"""
    out = []
    with check_option(mod, check), rs.handle(mod, prob, dtype, wire.SolverParams(**FIXED), **ON) as s:
        s.init()
        for part in pieces:
            mod.profile_reset()
            assert s.run(part) == part
            out.append(rs.base_counts(mod.profile_dump()))
        st, _ = s.result()
    assert rs.status(st).num_iterations == 23
    return out


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kind,shape", CELLS)
def test_a_check_is_one_launch(solve_mod, kind, shape, dtype):
    """Sweep 0 with its check, sweeps 1 to 9 without one, sweeps 10 to 22 with the checks at 10 and 20
    and the final one: beside the sweeps' own launches - those of the nine sweeps that no check
    follows - the profile holds one norms launch per check and nothing else.  With the option off the
    profile is the sweeps' launches alone, as on the route before the option existed: neither norms tag."""
    prob = make(kind, shape)
    first, nine, rest = loop_profiles(solve_mod, prob, dtype, "1", (1, 9, 13))
    tag = norms_tag(shape)
    assert set(sweep_tags(kind, shape)) <= set(nine) and not set(NORMS) & set(nine), sorted(nine)
    assert all(v % 9 == 0 for v in nine.values()), nine
    per = {t: v // 9 for t, v in nine.items()}
    assert all(per[t] == 1 for t in sweep_tags(kind, shape)), per
    assert first == dict(per, **{tag: 1}), (first, per)
    assert rest == dict({t: 13 * v for t, v in per.items()}, **{tag: 3}), (rest, per)
    first0, nine0, rest0 = loop_profiles(solve_mod, prob, dtype, "0", (1, 9, 13))
    assert nine0 == nine, (nine0, nine)
    # (the generic check's vector launches carry no profile tag: the sweeps' own are all there is)
    for got, sweeps in ((first0, 1), (rest0, 13)):
        assert got == {t: sweeps * v for t, v in per.items()}, (got, per)


# ---- 3. stopping sweep --------------------------------------------------------------------------------
_checks = {}


def oracle_checks(kind, shape, make_prob=None, **params):
    """the oracle's solve with r / eps_pri and s / eps_dual at every check: (decoded status, arrays,
    {iteration: (r ratio, s ratio)})"""
    key = (kind, shape, tuple(sorted(params.items())))
    if key not in _checks:
        prob, ratios = (make_prob or (lambda: make(kind, shape)))(), {}

        def at_check(it, solver):
            if it % solver.params.epoch_iterations == 0:
                solver.compute_residuals()
                r = solver.status.residuals
                ratios[it] = (r.r_norm / r.epsilon_primal, r.s_norm / r.epsilon_dual)
        st, x = orc.solve(prob.SerializeToString(), [], wire.SolverParams(**params).SerializeToString(),
                          prob.expression_data(), trace=at_check)
        _checks[key] = (rs.status(st), rs.arrays(x), ratios)
    return _checks[key]


def outside_the_window(ratios, its):
    return all(not 0.95 <= v <= 1.05 for it in its for v in ratios[it])


STOPS = [
    ("hinge_l1", T2, 50), ("hinge_l1", F2, 50), ("deadzone_l1", T1, 40), ("deadzone_l1", F1, 50),
    ("basis_pursuit", F1, 60), ("basis_pursuit", F2, 70), ("least_abs_dev", T1, 40), ("quantile", T1, 60),
    ("logreg_l1", T1, 40), ("logreg_l1", T2, 70), ("logreg_l1", F1, 60), ("logreg_l1", F2, 80),
    ("hinge_l2", T1, 30), ("hinge_l2", T2, 30), ("hinge_l2", F2, 10),
]


def test_every_kind_has_a_stopping_cell():
    assert {kind for kind, _, _ in STOPS} == set(SHAPES_OF)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kind,shape,stop", STOPS)
def test_stops_with_the_oracle(routes, kind, shape, stop, dtype):
    so, xo, ratios = oracle_checks(kind, shape)
    assert so.state == wire.SolverStatus.OPTIMAL and so.num_iterations == stop
    print("oracle: (r / eps_pri, s / eps_dual) at %d: %s, at %d: %s" % (
        stop - 10, ratios[stop - 10], stop, ratios[stop]))
    assert outside_the_window(ratios, (stop - 10, stop)), ratios
    # the driver speculates behind a check while the check before it was beyond 4 x a tolerance
    discarded = 10 if max(ratios[stop - 10]) > 4 else 0
    assert discarded == (10 if (kind, shape) == ("hinge_l2", F2) else 0)
    for check in ("1", "0"):
        st, x, c = routes.solve(make(kind, shape), dtype, check)
        if check == "1":
            assert_route(c, st, kind, shape, stop // 10 + 1, discarded)
        else:
            assert_route(c, st, kind, shape, 0)
        rs.assert_matches_oracle(st, x, so, xo, dtype)


# ---- 4. speculation and restore ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kind,shape,epoch", [
    ("least_abs_dev", T1, 40), ("deadzone_l1", T1, 40), ("hinge_l1", F2, 50), ("logreg_l1", T1, 40),
    ("logreg_l1", F1, 60),
])
def test_a_discarded_epoch_leaves_the_stopping_iterate(routes, kind, shape, epoch, dtype):
    """The check after sweep 0 is far from optimal, so the next `epoch` sweeps run behind it; so do
    `epoch` more behind the check at iteration `epoch`, which says OPTIMAL: they are discarded and the
    snapshot is restored.  The variables are those of `epoch` + 1 sweeps with no speculation at the end."""
    so, xo, ratios = oracle_checks(kind, shape, epoch_iterations=epoch)
    assert so.state == wire.SolverStatus.OPTIMAL and so.num_iterations == epoch and sorted(ratios) == [0, epoch]
    print("oracle: (r / eps_pri, s / eps_dual) at 0: %s, at %d: %s" % (ratios[0], epoch, ratios[epoch]))
    assert max(ratios[0]) > 4 and outside_the_window(ratios, (epoch,)), ratios
    prob = make(kind, shape)
    st, x, c = routes.solve(prob, dtype, "1", epoch_iterations=epoch)
    s = rs.status(st)
    assert s.state == wire.SolverStatus.OPTIMAL and s.num_iterations == epoch, s
    # the sweeps launched: 1 + epoch counted and epoch discarded
    assert c.get(sweep_tags(kind, shape)[0]) == 2 * epoch + 1 and c.get(norms_tag(shape)) == 2, c
    plain = dict(max_iterations=epoch + 1, abs_tol=0.0, rel_tol=0.0)
    for check in ("1", "0"):
        st1, x1, c1 = routes.solve(prob, dtype, check, **plain)
        assert c1.get(sweep_tags(kind, shape)[0]) == epoch + 1, c1
        rs.assert_same_arrays(x, x1, check)
    rs.assert_matches_oracle(st, x, so, xo, dtype)


# ---- 5. handles in pieces -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kind,shape", CELLS)
def test_a_solve_in_pieces_is_the_same_solve(solve_mod, kind, shape, dtype):
    prob = make(kind, shape)
    with check_option(solve_mod, "1"):
        st_a, xa, ca = rs.run_handle(solve_mod, prob, dtype, [23], ON, **FIXED)
        st_b, xb, cb = rs.run_handle(solve_mod, prob, dtype, [7, 10, 6], ON, **FIXED)
    for c in (ca, cb):
        assert c.get(sweep_tags(kind, shape)[0]) == 23 and c.get(norms_tag(shape)) == FIXED_CHECKS, c
    assert rs.status(st_a).state == wire.SolverStatus.MAX_ITERATIONS_REACHED
    rs.assert_same_bytes_and_residuals((st_a, xa), (st_b, xb))


# ---- 6. groups ----------------------------------------------------------------------------------------
GROUP_TOL = dict(abs_tol=1e-2, rel_tol=1e-2)
GROUP_FRACS = (0.05, 0.02, 0.01)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("shape,stops,sweep_tag", [
    (T1, (60, 30, 40), "batch_zero_tall_cols"), (F1, (60, 30, 20), "batch_zero_rows"),
])
def test_a_group_checks_each_member_with_one_launch(solve_mod, shape, stops, sweep_tag, dtype):
    """a three-member hinge lambda path that stops, by the oracle, at three different checks: each
    member is its own solve with the option on, bit for bit, frozen from its stop on while the others
    go on, and every check of the group is one norms launch per member still active"""
    probs = [hinge_member(shape[0], shape[1], f) for f in GROUP_FRACS]
    for f, prob, stop in zip(GROUP_FRACS, probs, stops):
        so, _, ratios = oracle_checks("hinge_member %g" % f, shape, make_prob=lambda prob=prob: prob, **GROUP_TOL)
        print("oracle, f = %g: stop %d, ratios before %s, at the stop %s" % (
            f, so.num_iterations, ratios[stop - 10], ratios[stop]))
        assert so.state == wire.SolverStatus.OPTIMAL and so.num_iterations == stop
        assert outside_the_window(ratios, (stop - 10, stop)), ratios
    opts = dict(ON, batch_zero_tall="1")
    with check_option(solve_mod, "1"):
        batch, tagsb, single, tags1 = rs.run_both(solve_mod, probs, dtype, opts, **GROUP_TOL)
    cb, c1 = rs.base_counts(tagsb), rs.base_counts(tags1)
    got = [(rs.status(st).state, rs.status(st).num_iterations) for st, _ in batch]
    assert got == [(wire.SolverStatus.OPTIMAL, stop) for stop in stops], got
    rs.assert_identical(batch, single)
    tag = norms_tag(shape)
    assert cb.get(sweep_tag) == max(stops) + 1, cb                     # one group, as long as its last member
    assert cb.get(tag) == sum(stop // 10 + 1 for stop in stops), cb    # a member is checked until it stops
    assert c1.get(tag) == stops[0] // 10 + 1, c1
    # nothing else between the sweeps of a group: 20, 21 and 30 sweeps with the tolerances at zero have
    # 3, 4 and 4 checks per member, so 21 against 20 is one sweep and one check of every member, and 30
    # against 21 nine sweeps
    pbs, data = [p.SerializeToString() for p in probs], rs.union_data(probs)
    counts = {}
    for check, lengths in (("1", (20, 20, 21, 30)), ("0", (20,))):  # (the first call: a warm-up)
        for sweeps in lengths:
            sb = wire.SolverParams(max_iterations=sweeps, abs_tol=0.0, rel_tol=0.0).SerializeToString()
            with check_option(solve_mod, check), rs.options(solve_mod, dtype=dtype, **opts):
                _, tags = rs.profiled(solve_mod, lambda: solve_mod.solve_batch(pbs, None, sb, data))
            counts[check, sweeps] = rs.base_counts(tags)
    c20, c21, c30 = (counts["1", k] for k in (20, 21, 30))
    nine = {t: c30[t] - c21.get(t, 0) for t in c30 if c30[t] != c21.get(t, 0)}
    assert nine.get(sweep_tag) == 9 and all(v % 9 == 0 for v in nine.values()) and tag not in nine, nine
    one = {t: c21[t] - c20.get(t, 0) for t in c21 if c21[t] != c20.get(t, 0)}
    assert one == dict({t: v // 9 for t, v in nine.items()}, **{tag: len(probs)}), (one, nine)
    assert not set(NORMS) & set(counts["0", 20]) and counts["0", 20].get(sweep_tag) == 20, sorted(counts["0", 20])


# ---- 7. run to run ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kind,shape", [("hinge_l1", T2), ("logreg_l1", F2), ("least_abs_dev", T2),
                                        ("basis_pursuit", F2)])
def test_two_solves_give_the_same_bits(routes, kind, shape, dtype):
    prob = make(kind, shape)
    a = routes.solve(prob, dtype, "1", **FIXED)
    b = routes.solve(prob, dtype, "1", **FIXED)
    rs.assert_same_bytes_and_residuals(a[:2], b[:2])
    assert residuals(a[0])["r_norm"] > 0 and residuals(a[0])["s_norm"] > 0
