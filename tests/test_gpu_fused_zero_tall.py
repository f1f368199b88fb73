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

pytestmark = pytest.mark.gpu

SHAPES = [(601, 256), (603, 260), (2051, 1028)]
FIXED = dict(max_iterations=60, abs_tol=0.0, rel_tol=0.0)


def status(st):
    return wire.SolverStatus.FromString(st)


def sweeps(st):
    s = status(st)
    return s.num_iterations + 1 if s.state == wire.SolverStatus.OPTIMAL else s.num_iterations


def base_counts(tags):
    out = {}
    for t, (c, _) in tags.items():
        out[t.split(":")[0]] = out.get(t.split(":")[0], 0) + c
    return out


def tall_tags(c):
    return sorted(t for t in c if t.startswith("zero_tall"))


class Routes(object):
    """solves with the options set for one call and put back after it"""

    def __init__(self, mod):
        self.mod = mod

    def solve(self, prob, dtype="f32", tall="1", fused="1", fused_zero="auto", **params):
        pb, data = prob.SerializeToString(), prob.expression_data()
        sb = wire.SolverParams(**params).SerializeToString()
        mod = self.mod
        mod.set_option("dtype", dtype)
        mod.set_option("fused_zero_tall", tall)
        mod.set_option("fused_zero", fused_zero)
        mod.set_option("fused", fused)
        mod.profile_reset()
        mod.profile_enable(True)
        try:
            st, x = mod.solve(pb, [], sb, data)
            tags = mod.profile_dump()
        finally:
            mod.profile_enable(False)
            mod.set_option("fused", "1")
            mod.set_option("fused_zero", "auto")
            mod.set_option("fused_zero_tall", "auto")
            mod.set_option("dtype", "f32")
        return st, {k: np.frombuffer(v).copy() for k, v in x.items()}, base_counts(tags)


@pytest.fixture
def routes(solve_mod):
    return Routes(solve_mod)


_made = {}


def make(kind, shape):
    key = (kind, shape)
    if key not in _made:
        m, n = shape
        if kind == "deadzone":
            _made[key] = problems.deadzone_l1(m, n)[0]
        elif kind == "hinge_default":
            _made[key] = problems.hinge_l1(m, n)[0]
        elif kind == "hinge":
            C = problems.hinge_l1(m, n)[1]["C"]
            _made[key] = problems.hinge_l1(m, n, lam=0.01 * np.abs(C.sum(axis=0)).max())[0]
        else:
            assert kind == "logreg"
            _made[key] = problems.logreg_l1(m, n)[0]
    return _made[key]


_oracle = {}


def oracle(kind, shape, **params):
    """the CPU oracle's solve of one problem, computed once per module"""
    key = (kind, shape, tuple(sorted(params.items())))
    if key not in _oracle:
        prob = make(kind, shape)
        st, x = orc.solve(prob.SerializeToString(), [], wire.SolverParams(**params).SerializeToString(),
                          prob.expression_data())
        _oracle[key] = (status(st), {k: np.frombuffer(v).copy() for k, v in x.items()})
    return _oracle[key]


def assert_close(x, xo, dtype):
    tol = dict(rtol=1e-6, atol=1e-8) if dtype == "f64" else dict(rtol=5e-3, atol=5e-3)
    assert sorted(x) == sorted(xo)
    for k in xo:
        print(k, "max |gpu - oracle| %.3g, max |oracle| %.3g" % (np.abs(x[k] - xo[k]).max(), np.abs(xo[k]).max()))
    for k in xo:
        np.testing.assert_allclose(x[k], xo[k], err_msg=k, **tol)


def assert_matches_oracle(st, x, so, xo, dtype):
    sg = status(st)
    print("gpu: state %d at %d, r %.6g eps %.6g | oracle: state %d at %d, r %.6g eps %.6g" % (
        sg.state, sg.num_iterations, sg.residuals.r_norm, sg.residuals.epsilon_primal,
        so.state, so.num_iterations, so.residuals.r_norm, so.residuals.epsilon_primal))
    assert sg.state == so.state and sg.num_iterations == so.num_iterations
    assert_close(x, xo, dtype)


def assert_route(c, st, shape):
    """one pass and one x-side launch per sweep (the checks are not pipelined: nothing is
    discarded), no launch of the fat route or of the lasso route, the packed symmetric apply from
    1024 columns"""
    assert c.get("zero_tall", 0) == sweeps(st), (tall_tags(c), c.get("zero_tall"), sweeps(st))
    assert c.get("zero_tall_cols", 0) == sweeps(st), (c.get("zero_tall_cols"), sweeps(st))
    assert not [t for t in c if t.startswith("zero_fused")], sorted(c)
    assert "lasso_fused" not in c
    if shape[1] >= 1024:
        assert c.get("symv_packed", 0) >= sweeps(st), sorted(c)


def assert_generic(c):
    assert not tall_tags(c) and not [t for t in c if t.startswith("zero_fused")], sorted(c)


def assert_same_bytes(st, x, st0, x0):
    assert (status(st).state, status(st).num_iterations) == (status(st0).state, status(st0).num_iterations)
    assert sorted(x) == sorted(x0)
    for k in x0:
        assert x[k].tobytes() == x0[k].tobytes(), k


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
    assert_matches_oracle(st, x, so, xo, dtype)


# ---- 2. hinge, default stopping rule, f64 -----------------------------------------------------------
@pytest.mark.parametrize("shape,stop", [((601, 256), 250), ((603, 260), 200)])
def test_hinge_stops_with_the_oracle_f64(routes, shape, stop):
    """The oracle stops (601, 256) at 250 with r / eps_pri = 0.945 after 1.016 at the check before,
    (603, 260) at 200 with 0.929 after 1.010: enough for f64, not for f32."""
    so, xo = oracle("hinge_default", shape)
    assert so.state == wire.SolverStatus.OPTIMAL and so.num_iterations == stop
    st, x, c = routes.solve(make("hinge_default", shape), "f64")
    assert_route(c, st, shape)
    assert_matches_oracle(st, x, so, xo, "f64")


# ---- 3. fused against generic, f64 --------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hinge", "deadzone"])
def test_fused_equals_generic_to_rounding_f64(routes, kind):
    shape = (603, 260)
    prob = make(kind, shape)
    st, x, c = routes.solve(prob, "f64", "1", **FIXED)
    st0, x0, c0 = routes.solve(prob, "f64", "0", **FIXED)
    assert_route(c, st, shape)
    assert_generic(c0)
    assert status(st).num_iterations == status(st0).num_iterations == 60
    for k in x0:
        diff, ref = np.abs(x[k] - x0[k]).max(), np.abs(x0[k]).max()
        print(k, "max |fused - generic| %.3g, max |generic| %.3g" % (diff, ref))
        assert diff <= 1e-9 * ref, k


# ---- 4. sweep boundaries and warm start -------------------------------------------------------------
def run_handle(mod, prob, dtype, splits, **params):
    mod.set_option("dtype", dtype)
    mod.set_option("fused_zero_tall", "1")
    s = mod.Solver(prob.SerializeToString(), wire.SolverParams(**params).SerializeToString(),
                   prob.expression_data())
    mod.profile_reset()
    mod.profile_enable(True)
    try:
        s.init()
        for part in splits:
            assert s.run(part) == part
        c = base_counts(mod.profile_dump())
        st, x = s.result()
    finally:
        mod.profile_enable(False)
        s.close()
        mod.set_option("fused_zero_tall", "auto")
        mod.set_option("dtype", "f32")
    return st, {k: np.frombuffer(v).copy() for k, v in x.items()}, c


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_a_solve_can_stop_after_any_sweep(solve_mod, dtype):
    prob = make("hinge", (601, 256))
    params = dict(max_iterations=1000, abs_tol=0.0, rel_tol=0.0)
    st_a, xa, ca = run_handle(solve_mod, prob, dtype, [30], **params)
    st_b, xb, cb = run_handle(solve_mod, prob, dtype, [1, 9, 20], **params)
    assert ca.get("zero_tall") == cb.get("zero_tall") == 30
    assert ca.get("zero_tall_cols") == cb.get("zero_tall_cols") == 30
    assert sorted(xa) == sorted(xb) and len(xa) == 4
    for k in xa:
        assert xa[k].tobytes() == xb[k].tobytes(), k


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_warm_start_takes_the_state_over(solve_mod, dtype):
    """two solves of 30 sweeps on one handle, the second warm-started, against the oracle doing
    the same on one solver object"""
    shape = (601, 256)
    prob = make("hinge", shape)
    sp = wire.SolverParams(warm_start=True, max_iterations=30, abs_tol=0.0, rel_tol=0.0)
    pb, data = prob.SerializeToString(), prob.expression_data()
    solve_mod.set_option("dtype", dtype)
    solve_mod.set_option("fused_zero_tall", "1")
    s = solve_mod.Solver(pb, sp.SerializeToString(), data)
    solve_mod.profile_reset()
    solve_mod.profile_enable(True)
    try:
        s.init()
        s.run(-1)
        s.init()
        s.run(-1)
        c = base_counts(solve_mod.profile_dump())
        st, x = s.result()
    finally:
        solve_mod.profile_enable(False)
        s.close()
        solve_mod.set_option("fused_zero_tall", "auto")
        solve_mod.set_option("dtype", "f32")
    assert c.get("zero_tall") == c.get("zero_tall_cols") == 60
    osolver = orc.create_solver(wire.Problem.FromString(pb), dict(data), sp)
    osolver.solve()
    xo = osolver.solve()
    assert status(st).num_iterations == osolver.status.num_iterations == 30
    x = {k: np.frombuffer(v) for k, v in x.items()}
    xw = {k: np.asarray(xo(k), dtype=np.float64).ravel() for k in x}
    # on the oracle alone: the second solve went on from the first, its iterate is not the cold
    # solve's by far more than the tolerances, so a route that dropped the state would not pass
    cold = oracle("hinge", shape, max_iterations=30, abs_tol=0.0, rel_tol=0.0)[1]
    print("oracle: max |warm - cold| in z %.3g" % np.abs(xw["var:z"] - cold["var:z"]).max())
    assert np.abs(xw["var:z"] - cold["var:z"]).max() > 0.1
    assert_close(x, xw, dtype)


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
    assert_same_bytes(st, x, st0, x0)


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
    assert_same_bytes(st, x, st0, x0)


def test_auto_takes_the_route_from_the_measured_floor(routes):
    """the 4n x n ladder has the fused sweep ahead from its first cell, n = 256, so
    "auto" takes the route wherever "1" does"""
    st, x, c = routes.solve(make("hinge", (601, 256)), "f32", "auto", max_iterations=30)
    st1, x1, c1 = routes.solve(make("hinge", (601, 256)), "f32", "1", max_iterations=30)
    assert_route(c, st, (601, 256))
    assert_same_bytes(st, x, st1, x1)


# ---- 6. batch ---------------------------------------------------------------------------------------
def test_batch_members_are_their_own_solves(solve_mod):
    """three tall hinge members on one C: the route has no batched form, every member is solved
    by itself on it and returns its own solve bit for bit"""
    m, n = 601, 256
    scale = np.abs(problems.hinge_l1(m, n)[1]["C"].sum(axis=0)).max()
    probs = [problems.hinge_l1(m, n, lam=f * scale)[0] for f in (0.05, 0.02, 0.01)]
    data = {}
    for p in probs:
        data.update(p.expression_data())
    pbs = [p.SerializeToString() for p in probs]
    sb = wire.SolverParams(max_iterations=60).SerializeToString()
    solve_mod.set_option("fused_zero_tall", "1")
    solve_mod.profile_reset()
    solve_mod.profile_enable(True)
    try:
        batch = solve_mod.solve_batch(pbs, None, sb, data)
        cb = base_counts(solve_mod.profile_dump())
        solve_mod.profile_enable(False)
        single = [solve_mod.solve(pb, [], sb, data) for pb in pbs]
    finally:
        solve_mod.profile_enable(False)
        solve_mod.set_option("fused_zero_tall", "auto")
    assert cb.get("zero_tall", 0) == cb.get("zero_tall_cols", 0) == sum(sweeps(st) for st, _ in batch), cb
    assert not [t for t in cb if t.startswith("batch_zero")], sorted(cb)
    assert len(batch) == len(single) == 3
    for k, ((stb, xb), (sts, xs)) in enumerate(zip(batch, single)):
        a, s = status(stb), status(sts)
        assert a.state == s.state and a.num_iterations == s.num_iterations, (k, a, s)
        for f in ("r_norm", "s_norm", "epsilon_primal", "epsilon_dual"):
            assert getattr(a.residuals, f) == getattr(s.residuals, f), (k, f)
        assert sorted(xb) == sorted(xs)
        for v in xs:
            assert np.array_equal(np.frombuffer(xb[v]), np.frombuffer(xs[v])), (k, v)
