"""The wide route of batched solves (option "batch_wide", kernels_fused_wide.hip):
groups of 8 or more f32 instances that share the data matrix run their sweeps as two matrix
products on the f32 matrix instruction.  Its contract is not bit identity with the single solve:
the same state, the same stopping check except where a residual sits within rounding of its
threshold, variables and residuals within f32 rounding - plus two invariants: identical bytes from
run to run, and an instance's bytes do not depend on its partners or its position.

References for values are f64: the oracle at the small shape, the library's own f64 single solve
(held to the oracle at 1e-7 by test_gpu_batch.py / test_gpu_parity.py) at the larger ones."""

import functools
import os
import sys

import numpy as np
import pytest

# torch first: it carries its own HIP runtime (see test_gpu_full_size.py)
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from epsilon_amd import _solve, ir, problems, wire  # noqa: E402
from oracle import epsilon_oracle as orc  # noqa: E402
from tests import route_support as rs  # noqa: E402

pytestmark = pytest.mark.gpu

RESIDUAL_NORMS = ("r_norm", "s_norm")
SMALL = (256, 768)  # the oracle is the reference here
FIXED = wire.SolverParams(max_iterations=100, ignore_stopping_criteria=True).SerializeToString()
# the oracle does not know ignore_stopping_criteria: zero tolerances run the same 100 sweeps
ORACLE_FIXED = wire.SolverParams(max_iterations=100, abs_tol=0.0, rel_tol=0.0).SerializeToString()
DEFAULT = wire.SolverParams().SerializeToString()
EPOCH = wire.SolverParams().epoch_iterations


def fracs_of(k):
    return [float(f) for f in np.geomspace(0.6, 0.04, k)]


@functools.lru_cache(maxsize=None)
def regression(m, n, seed):
    A, b = problems.regression_data(m, n, seed=seed)
    return A, b, float(np.abs(A.T.dot(b)).max()), ir.dense_matrix(A), ir.constant(b)


def lasso_path(m, n, seed, fracs):
    """(serialized problems, data) of a lambda path on regression_data(m, n, seed)"""
    A, b, lmax, Aexpr, bexpr = regression(m, n, seed)
    probs = [problems.lasso_ir(Aexpr, bexpr, f * lmax, n) for f in fracs]
    return [p.SerializeToString() for p in probs], rs.union_data(probs)


def f32_singles(pbs, params, sb, data):
    with rs.options(_solve, dtype="f32"):
        return [_solve.solve(pb, ps, sb, data) for pb, ps in zip(pbs, params)]


def f64_reference(shape, pbs, params, sb, data):
    """the oracle at the small shape, the library's f64 single solve above it"""
    if tuple(shape) == SMALL:
        sb = ORACLE_FIXED if sb == FIXED else sb
        return [orc.solve(pb, ps, sb, data) for pb, ps in zip(pbs, params)]
    with rs.options(_solve, dtype="f64"):
        return [_solve.solve(pb, ps, sb, data) for pb, ps in zip(pbs, params)]


def wide_batch(pbs, params, sb, data):
    with rs.options(_solve, dtype="f32"):
        return _solve.solve_batch(pbs, params, sb, data, wide=True)


def tags_of(fn):
    """(fn(), the set of tag names it launched)"""
    out, tags = rs.profiled(_solve, fn)
    return out, set(rs.base_counts(tags))


def assert_values_within_bound(label, wide, single, ref, residuals=True):
    """For every instance and variable, with e(.) the largest absolute distance from the f64
    reference and scale = max|x_ref|: e(wide) <= max(2 e(single f32 solve), 2e-5 scale) - the wide
    route may not be meaningfully worse than the route users already trust; the floor is the atol
    of test_fused_sweep_matches_generic_and_oracle (test_gpu_parity.py), whose residual tolerance
    (rtol 3e-3, atol 1e-5) holds the residual norms to the reference."""
    assert len(wide) == len(single) == len(ref)
    failures = []
    for k, ((stw, xw), (sts, xs), (str_, xr)) in enumerate(zip(wide, single, ref)):
        assert sorted(xw) == sorted(xr)
        for v in xr:
            r = np.frombuffer(xr[v])
            scale = np.abs(r).max()
            ew = np.abs(np.frombuffer(xw[v]) - r).max()
            es = np.abs(np.frombuffer(xs[v]) - r).max()
            bound = max(2 * es, 2e-5 * scale)
            print("%s inst %d %s: e(wide) %.3e e(single) %.3e scale %.3e bound %.3e" % (label, k, v, ew, es, scale, bound))
            if not ew <= bound:
                failures.append((k, v, ew, es, scale))
        if residuals:
            a, s, o = rs.status(stw), rs.status(sts), rs.status(str_)
            assert a.num_iterations == s.num_iterations == o.num_iterations == 100
            for f in RESIDUAL_NORMS:
                gw, gs, go = (getattr(z.residuals, f) for z in (a, s, o))
                print("%s inst %d %s: wide %.6e single %.6e ref %.6e" % (label, k, f, gw, gs, go))
                if not abs(gw - go) <= 1e-5 + 3e-3 * abs(go):
                    failures.append((k, f, gw, gs, go))
    assert not failures, failures


# ---- 1. route taken ------------------------------------------------------------------------------
def test_route_taken(solve_mod):
    pbs, data = lasso_path(*SMALL, 21, fracs_of(24))
    with rs.options(solve_mod, dtype="f32"):
        _, on = tags_of(lambda: solve_mod.solve_batch(pbs, None, FIXED, data, wide=True))
        _, off = tags_of(lambda: solve_mod.solve_batch(pbs, None, FIXED, data, wide=False))
    assert {"wide_back", "wide_forward", "wide_reduce"} <= on and "batch_fused_pass" not in on, sorted(on)
    assert "batch_fused_pass" in off and not {"wide_back", "wide_forward", "wide_reduce"} & off, sorted(off)


# ---- 2. fixed sweeps, the three forms of the inverse apply ---------------------------------------
@pytest.mark.parametrize("shape,seed,k", [((256, 768), 21, 24),      # inverse applied as a product
                                          ((1024, 3000), 5, 24),     # the packed-inverse form
                                          ((2048, 4608), 11, 32)])   # whitened
def test_fixed_sweeps_within_bound(solve_mod, shape, seed, k):
    pbs, data = lasso_path(*shape, seed, fracs_of(k))
    none = [[]] * k
    wide = wide_batch(pbs, None, FIXED, data)
    single = f32_singles(pbs, none, FIXED, data)
    ref = f64_reference(shape, pbs, none, FIXED, data)
    assert all(rs.status(st).num_iterations == 100 for st, _ in wide)
    assert_values_within_bound("fixed %dx%d" % shape, wide, single, ref)


# ---- 3. stopping ---------------------------------------------------------------------------------
def ratio(st):
    r = rs.status(st).residuals
    return max(r.r_norm / r.epsilon_primal, r.s_norm / r.epsilon_dual)


def reference_stops(shape, pbs, data):
    """per instance: (stopping check of the f64 reference, close?) - close when the residual ratio
    at the stopping check exceeds 0.95 or at the check before is below 1.05"""
    k = len(pbs)
    full = f64_reference(shape, pbs, [[]] * k, DEFAULT, data)
    out = []
    for pb, (st, _) in zip(pbs, full):
        s = rs.status(st)
        assert s.state == wire.SolverStatus.OPTIMAL
        stop = s.num_iterations
        close = ratio(st) > 0.95
        if stop >= EPOCH:
            # the check before: MAX_ITERATIONS_REACHED after stop - EPOCH + 1 sweeps reports the
            # residuals of exactly that iterate
            sb = wire.SolverParams(max_iterations=stop - EPOCH + 1).SerializeToString()
            (stp, _), = f64_reference(shape, [pb], [[]], sb, data)
            assert rs.status(stp).state == wire.SolverStatus.MAX_ITERATIONS_REACHED
            close = close or ratio(stp) < 1.05
        out.append((stop, close))
    return out


@pytest.mark.parametrize("shape,seed,k", [((256, 768), 21, 24), ((2048, 4608), 11, 32)])
def test_stopping_matches_reference(solve_mod, shape, seed, k):
    pbs, data = lasso_path(*shape, seed, fracs_of(k))
    stops = reference_stops(shape, pbs, data)
    nclose = sum(1 for _, c in stops if c)
    print("reference stops", stops)
    assert nclose <= k // 4, "inconclusive: %d of %d instances within rounding of a threshold" % (nclose, k)
    assert len({s for s, _ in stops}) >= 2  # members leave their panel at different checks
    wide = wide_batch(pbs, None, DEFAULT, data)
    got = [rs.status(st) for st, _ in wide]
    print("wide stops", [s.num_iterations for s in got])
    assert all(s.state == wire.SolverStatus.OPTIMAL for s in got)
    for i, (s, (stop, close)) in enumerate(zip(got, stops)):
        if close:
            assert abs(s.num_iterations - stop) <= EPOCH, (i, s.num_iterations, stop)
        else:
            assert s.num_iterations == stop, (i, s.num_iterations, stop)
    # MAX_ITERATIONS_REACHED beside OPTIMAL in one group
    slowest = max(s for s, _ in stops)
    cap = slowest - EPOCH + 1
    sb = wire.SolverParams(max_iterations=cap).SerializeToString()
    capped = [rs.status(st) for st, _ in wide_batch(pbs, None, sb, data)]
    states = {s.state for s in capped}
    assert states == {wire.SolverStatus.OPTIMAL, wire.SolverStatus.MAX_ITERATIONS_REACHED}, states
    for i, (s, (stop, close)) in enumerate(zip(capped, stops)):
        if close:
            continue
        if stop < cap:
            assert s.state == wire.SolverStatus.OPTIMAL and s.num_iterations == stop, (i, s, stop)
        else:
            assert s.state == wire.SolverStatus.MAX_ITERATIONS_REACHED, (i, s, stop)


# ---- 4. what may differ per instance ---------------------------------------------------------------
def check_wide_group(label, shape, probs, params, data):
    pbs = [p.SerializeToString() for p in probs]
    data = dict(data)
    data.update(rs.union_data(probs))
    wide, tags = tags_of(lambda: wide_batch(pbs, params, FIXED, data))
    assert "wide_back" in tags and not {"batch_fused_pass", "lasso_fused"} & tags, sorted(tags)
    single = f32_singles(pbs, params, FIXED, data)
    ref = f64_reference(shape, pbs, params, FIXED, data)
    assert_values_within_bound(label, wide, single, ref)


def test_rhs_bindings_with_different_lambda(solve_mod):
    m, n = 1024, 2100
    A, b, lmax, Aexpr, _ = regression(m, n, 8)
    rng = np.random.RandomState(2)
    bs = [b, b + 0.05 * rng.randn(m), 0.5 * b]
    probs, params, data = [], [], {}
    for i, f in enumerate(fracs_of(18)):
        probs.append(problems.lasso_ir(Aexpr, ir.parameter(m, 1, "param:b"), f * lmax, n))
        p, d = rs.bind_b(bs[i % 3])
        params.append(p)
        data.update(d)
    check_wide_group("param:b", (m, n), probs, params, data)


@pytest.mark.parametrize("kind", ["deadzone", "hinge", "quantile"])
def test_scaled_zone_kinds(solve_mod, kind):
    m, n = 1024, 2100
    A, b, lmax, Aexpr, bexpr = regression(m, n, 8)
    rng = np.random.RandomState(3)
    probs = []
    for f in fracs_of(16):
        qvec = (0.2 + rng.rand(n), 0.2 + rng.rand(n))  # per-column alpha / beta, per instance
        probs.append(rs.fused_problem(Aexpr, m, n, bexpr, f * lmax, kind, qvec))
    check_wide_group(kind, (m, n), probs, [[]] * 16, {})


# ---- 5. invariants ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,seed", [((256, 768), 21), ((2048, 4608), 11)])
def test_bits_do_not_depend_on_run_partners_or_position(solve_mod, shape, seed):
    path = fracs_of(24)
    pbs, data = lasso_path(*shape, seed, path)
    first = wide_batch(pbs, None, DEFAULT, data)
    assert len({rs.status(st).num_iterations for st, _ in first}) >= 2
    again = wide_batch(pbs, None, DEFAULT, data)
    for i in range(24):
        rs.assert_same_bytes_and_residuals(again[i], first[i], ("again", i))
    rev = wide_batch(pbs[::-1], None, DEFAULT, data)
    for i in range(24):
        rs.assert_same_bytes_and_residuals(rev[23 - i], first[i], ("reversed", i))
    head = wide_batch(pbs[:17], None, DEFAULT, data)
    for i in range(17):
        rs.assert_same_bytes_and_residuals(head[i], first[i], ("first 17", i))
    # 70 members, two panels: the path's first half in panel 0, its second half across the boundary
    others = [float(f) for f in np.geomspace(0.55, 0.05, 46)]
    opbs, odata = lasso_path(*shape, seed, others)
    big = opbs[:20] + pbs[:12] + opbs[20:] + pbs[12:]
    where = list(range(20, 32)) + list(range(58, 70))
    bdata = dict(data)
    bdata.update(odata)
    out, tags = tags_of(lambda: wide_batch(big, None, DEFAULT, bdata))
    assert "wide_back" in tags and "batch_fused_pass" not in tags
    for i, w in enumerate(where):
        assert big[w] is pbs[i]
        rs.assert_same_bytes_and_residuals(out[w], first[i], ("of 70", i))


# ---- 6. nothing else moves -------------------------------------------------------------------------
def assert_identical_to_single(batch, single):
    assert len(batch) == len(single)
    for k, (a, b) in enumerate(zip(batch, single)):
        rs.assert_same_bytes_and_residuals(a, b, k)


def test_f64_batch_keeps_its_route(solve_mod):
    pbs, data = lasso_path(*SMALL, 21, fracs_of(24))
    sb = wire.SolverParams(max_iterations=300).SerializeToString()
    with rs.options(solve_mod, dtype="f64"):
        batch, tags = tags_of(lambda: solve_mod.solve_batch(pbs, None, sb, data, wide=True))
        single = [solve_mod.solve(pb, [], sb, data) for pb in pbs]
    assert "batch_fused_pass" in tags and "wide_back" not in tags, sorted(tags)
    assert_identical_to_single(batch, single)


def test_two_block_batch_and_small_group_keep_their_routes(solve_mod):
    pbs, data = lasso_path(*SMALL, 21, fracs_of(24))
    sb2 = wire.SolverParams(max_iterations=200, solver=1).SerializeToString()
    batch, tags = tags_of(lambda: wide_batch(pbs, None, sb2, data))
    assert "wide_back" not in tags, sorted(tags)
    assert_identical_to_single(batch, f32_singles(pbs, [[]] * 24, sb2, data))
    sb = wire.SolverParams(max_iterations=300).SerializeToString()
    batch, tags = tags_of(lambda: wide_batch(pbs[:3], None, sb, data))
    assert "batch_fused_pass" in tags and "wide_back" not in tags, sorted(tags)
    assert_identical_to_single(batch, f32_singles(pbs[:3], [[]] * 3, sb, data))


def test_mixed_batch(solve_mod):
    """sparse, hinge, logistic and other-matrix instances beside a wide group: every instance that
    is not in the wide group returns the bits of its single solve."""
    rng = np.random.RandomState(6)
    wpbs, wdata = lasso_path(*SMALL, 21, fracs_of(16))
    opbs, odata = lasso_path(300, 650, 7, (0.3, 0.2))  # another matrix: a group of two
    ms, ns = 60, 150
    S = __import__("scipy.sparse", fromlist=["random"]).random(ms, ns, density=0.15, random_state=rng, format="csc")
    bs = S.dot(np.where(rng.rand(ns) < 0.1, rng.randn(ns), 0)) + 0.01 * rng.randn(ms)
    sparse = problems.lasso_ir(ir.sparse_matrix(S), ir.constant(bs), 0.1 * np.abs(S.T.dot(bs)).max(), ns)
    hinge, _ = problems.hinge_l1(80, 40, seed=1)
    logreg, _ = problems.logreg_l1(80, 40, seed=2)
    extra = [sparse, hinge, logreg]
    pbs = wpbs[:8] + [extra[0].SerializeToString(), opbs[0]] + wpbs[8:] + \
        [extra[1].SerializeToString(), opbs[1], extra[2].SerializeToString()]
    wide_at = list(range(8)) + list(range(10, 18))
    data = dict(wdata)
    data.update(odata)
    data.update(rs.union_data(extra))
    batch, tags = tags_of(lambda: wide_batch(pbs, None, FIXED, data))
    assert {"wide_back", "batch_fused_pass"} <= tags, sorted(tags)
    single = f32_singles(pbs, [[]] * len(pbs), FIXED, data)
    for i in range(len(pbs)):
        if i not in wide_at:
            rs.assert_same_bytes_and_residuals(batch[i], single[i], i)
    wp = [pbs[i] for i in wide_at]
    ref = f64_reference(SMALL, wp, [[]] * 16, FIXED, data)
    assert_values_within_bound("mixed", [batch[i] for i in wide_at], [single[i] for i in wide_at], ref)


# ---- 7. full size ------------------------------------------------------------------------------------
def test_full_size_path_of_32(solve_mod):
    """config 2 (10^4 x 5 * 10^4, fp32, whitened), K = 32, 30 sweeps: every instance within
    atol = 2e-4 * scale of its single whitened solve, the tolerance of the full-size checks
    (test_gpu_full_size.py, test_gpu_fused_whiten.py)."""
    import bench
    At, b, lam = bench.make_instance(10000, 50000, torch.device("cuda", 0))
    try:
        lmax = 2.0 * lam  # make_instance returns 0.5 lambda_max
        probs = [bench.build_problem(At, b, f * lmax) for f in fracs_of(32)]
        pbs, data = [p.SerializeToString() for p in probs], rs.union_data(probs)
        sb = wire.SolverParams(max_iterations=30, ignore_stopping_criteria=True).SerializeToString()
        wide, tags = tags_of(lambda: wide_batch(pbs, None, sb, data))
        single = f32_singles(pbs, [[]] * 32, sb, data)
    finally:
        del At
        torch.cuda.empty_cache()
    assert "wide_back" in tags and "batch_fused_pass" not in tags, sorted(tags)
    for k, ((stw, xw), (sts, xs)) in enumerate(zip(wide, single)):
        assert rs.status(stw).num_iterations == rs.status(sts).num_iterations == 30
        for v in xs:
            s = np.frombuffer(xs[v])
            scale = np.abs(s).max()
            err = np.abs(np.frombuffer(xw[v]) - s).max()
            print("full size inst %d %s: |wide - single| %.3e scale %.3e" % (k, v, err, scale))
            assert err <= 2e-4 * scale, (k, v, err, scale)
