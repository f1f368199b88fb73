"""Batched solves (include/epsilon_hip.h eps_solve_batch, _solve.solve_batch): K instances that
share one data map and one SolverParams.  The contract is that result k is exactly what
_solve.solve returns for instance k alone - the same status (timing aside) and the same bits in
every variable - whether the instance ran in a batched group (kernels_fused_batch.hip) or alone."""

import math

import numpy as np
import pytest

from epsilon_amd import ir, problems, wire
from oracle import epsilon_oracle as orc
from tests import route_support as rs

pytestmark = pytest.mark.gpu

PATH = (0.5, 0.35, 0.25, 0.18, 0.12)  # fractions of lambda_max of the lambda paths below
SETUP = ("gemm", "syrk", "spd_inverse")  # what setup_counts counts here: Gram products, explicit inverses
dtype = rs.dtype_fixture(("f32", "f64"))


def lambda_path(m, n, seed, fracs=PATH):
    A, b = problems.regression_data(m, n, seed=seed)
    lmax = np.abs(A.T.dot(b)).max()
    probs = [problems.lasso_ir(ir.dense_matrix(A), ir.constant(b), f * lmax, n) for f in fracs]
    return probs, A, b


def singles(solve_mod, pbs, params, sb, data):
    return [solve_mod.solve(pb, ps, sb, data) for pb, ps in zip(pbs, params)]


def max_iterations_splitting(solve_mod, pbs, data, **kw):
    """A max_iterations that some instances reach OPTIMAL within (at different sweeps) and the
    slowest does not."""
    sb = wire.SolverParams(max_iterations=3000, **kw).SerializeToString()
    its = sorted(rs.status(st).num_iterations for st, _ in singles(solve_mod, pbs, [[]] * len(pbs), sb, data))
    assert its[-1] > its[0], its
    return its[-1] - 1


@pytest.mark.parametrize("shape", [(200, 500), (1024, 3000)])
def test_lambda_path_bit_identical(solve_mod, dtype, shape):
    probs, A, b = lambda_path(*shape, seed=3)
    pbs, data = [p.SerializeToString() for p in probs], rs.union_data(probs)
    tight = dict(epoch_iterations=1, rel_tol=1e-4, abs_tol=1e-6)  # a check after every sweep
    max_it = max_iterations_splitting(solve_mod, pbs, data, **tight)
    sb = wire.SolverParams(max_iterations=max_it, **tight).SerializeToString()
    single = singles(solve_mod, pbs, [[]] * len(pbs), sb, data)
    states = [rs.status(st).state for st, _ in single]
    assert wire.SolverStatus.MAX_ITERATIONS_REACHED in states
    assert len({rs.status(st).num_iterations for st, _ in single}) >= 3  # stops at different checks
    batch = solve_mod.solve_batch(pbs, None, sb, data)
    rs.assert_identical(batch, single)


def test_lambda_path_matches_oracle_f64(solve_mod):
    with rs.options(solve_mod, dtype="f64"):
        probs, A, b = lambda_path(200, 500, seed=4, fracs=PATH[:4])
        pbs, data = [p.SerializeToString() for p in probs], rs.union_data(probs)
        sb = wire.SolverParams(max_iterations=400).SerializeToString()
        batch = solve_mod.solve_batch(pbs, None, sb, data)
    for pb, (stb, xb) in zip(pbs, batch):
        sto, xo = orc.solve(pb, [], sb, data)
        a, o = rs.status(stb), rs.status(sto)
        assert a.state == o.state and a.num_iterations == o.num_iterations
        for v in xo:
            np.testing.assert_allclose(np.frombuffer(xb[v]), np.frombuffer(xo[v]), rtol=1e-7, atol=1e-9)


def test_parameters_and_scaled_zone_kinds(solve_mod, dtype):
    m, n = 1024, 2100
    A, b = problems.regression_data(m, n, seed=8)
    lmax = np.abs(A.T.dot(b)).max()
    rng = np.random.RandomState(2)
    bs = [b, b + 0.05 * rng.randn(m), 0.5 * b]
    probs, params, data = [], [], {}
    # per-instance bindings of param:b, with lambda varying too
    for i, (bi, f) in enumerate(zip(bs, (0.3, 0.3, 0.2))):
        probs.append(problems.lasso_ir(ir.dense_matrix(A), ir.parameter(m, 1, "param:b"), f * lmax, n))
        p, d = rs.bind_b(bi)
        params.append(p)
        data.update(d)
    qvec = (0.2 + rng.rand(n), 0.2 + rng.rand(n))
    for kind in ("deadzone", "hinge", "quantile", "quantile"):
        lam = (0.3 if len(probs) % 2 else 0.2) * lmax
        probs.append(rs.fused_problem(ir.dense_matrix(A), m, n, ir.constant(b), lam, kind, qvec))
        params.append([])
    data.update(rs.union_data(probs))
    pbs = [p.SerializeToString() for p in probs]
    sb = wire.SolverParams(max_iterations=300).SerializeToString()
    single = singles(solve_mod, pbs, params, sb, data)
    batch = solve_mod.solve_batch(pbs, params, sb, data)
    rs.assert_identical(batch, single)


def expected_passes(results, width):
    sw = [rs.sweeps(st) for st, _ in results]
    return sum(math.ceil(sum(1 for s in sw if s > i) / width) for i in range(max(sw)))


@pytest.mark.parametrize("dt,shape,k,width", [("f32", (1024, 3000), 5, 8),    # one pass per sweep
                                              ("f64", (1024, 3000), 13, 8)])  # two passes
def test_shared_setup_and_pass_counts(solve_mod, dt, shape, k, width):
    """Widths per (m, dtype): DESIGN.md 3.6 (f32 and f64 at m = 1024 run two 16-byte chunks per
    thread, 8 instances per pass)."""
    with rs.options(solve_mod, dtype=dt):
        fracs = [0.5 * 0.9 ** i for i in range(k)]
        probs, A, b = lambda_path(*shape, seed=5, fracs=fracs)
        pbs, data = [p.SerializeToString() for p in probs], rs.union_data(probs)
        sb = wire.SolverParams(max_iterations=250).SerializeToString()
        one, tags1 = rs.profiled(solve_mod, lambda: solve_mod.solve(pbs[0], [], sb, data))
        batch, tagsb = rs.profiled(solve_mod, lambda: solve_mod.solve_batch(pbs, None, sb, data))
        single = singles(solve_mod, pbs, [[]] * k, sb, data)
    rs.assert_identical(batch, single)
    s1, sb_ = rs.setup_counts(tags1, SETUP), rs.setup_counts(tagsb, SETUP)
    assert s1 and sb_ == s1, (tags1, tagsb)
    c1, cb = rs.base_counts(tags1), rs.base_counts(tagsb)
    assert "lasso_fused" in c1 and "lasso_fused" not in cb, sorted(tagsb)
    assert cb["batch_fused_pass"] == expected_passes(batch, width), (cb, [rs.sweeps(s) for s, _ in batch])
    assert cb["batch_symv_packed"] > 0 and cb["batch_reduce_partials"] == cb["batch_fused_pass"] // math.ceil(k / width) or k > width


def test_fallbacks_are_exact(solve_mod, dtype):
    rng = np.random.RandomState(6)
    fused, A, b = lambda_path(300, 700, seed=6, fracs=(0.4, 0.2))
    other_A, _, _ = lambda_path(300, 650, seed=7, fracs=(0.3,))  # another matrix: alone
    ms, ns = 60, 150
    S = __import__("scipy.sparse", fromlist=["random"]).random(ms, ns, density=0.15, random_state=rng, format="csc")
    bs = S.dot(np.where(rng.rand(ns) < 0.1, rng.randn(ns), 0)) + 0.01 * rng.randn(ms)
    sparse = problems.lasso_ir(ir.sparse_matrix(S), ir.constant(bs), 0.1 * np.abs(S.T.dot(bs)).max(), ns)
    hinge, _ = problems.hinge_l1(80, 40, seed=1)
    logreg, _ = problems.logreg_l1(80, 40, seed=2)
    probs = [fused[0], sparse, hinge, fused[1], other_A[0], logreg]
    pbs, data = [p.SerializeToString() for p in probs], rs.union_data(probs)
    sb = wire.SolverParams(max_iterations=200).SerializeToString()
    rs.assert_identical(solve_mod.solve_batch(pbs, None, sb, data), singles(solve_mod, pbs, [[]] * 6, sb, data))
    # the two-block driver: solved one by one, the same bits
    sb2 = wire.SolverParams(max_iterations=200, solver=1).SerializeToString()
    pbs2 = [p.SerializeToString() for p in fused]
    rs.assert_identical(solve_mod.solve_batch(pbs2, None, sb2, data), singles(solve_mod, pbs2, [[]] * 2, sb2, data))


def test_errors_leave_the_library_usable(solve_mod):
    probs, A, b = lambda_path(100, 300, seed=1, fracs=(0.5, 0.3))
    pbs, data = [p.SerializeToString() for p in probs], rs.union_data(probs)
    sb = wire.SolverParams(max_iterations=100).SerializeToString()
    good = solve_mod.solve_batch(pbs, None, sb, data)

    def check_ok():
        rs.assert_identical(solve_mod.solve_batch(pbs, None, sb, data), good)

    with pytest.raises(solve_mod.error, match="count is 0"):
        solve_mod.solve_batch([], None, sb, data)
    check_ok()
    with pytest.raises(solve_mod.error):
        solve_mod.solve_batch(pbs, [[]], sb, data)
    check_ok()
    with pytest.raises(solve_mod.error, match="instance 1"):
        solve_mod.solve_batch([pbs[0], b"\xff\xff\xff", pbs[1]], None, sb, data)
    check_ok()
    unbound = problems.lasso_ir(ir.dense_matrix(A), ir.parameter(100, 1, "param:b"), 1.0, 300)
    with pytest.raises(solve_mod.error, match="instance 2.*param:b"):
        solve_mod.solve_batch(pbs + [unbound.SerializeToString()], None, sb, data)
    check_ok()


def test_full_size_lambda_path(solve_mod):
    """config 2 (10^4 x 5 * 10^4, fp32), a lambda path of 4."""
    probs, A, b = lambda_path(10000, 50000, seed=0, fracs=(0.5, 0.35, 0.25, 0.18))
    del A, b
    pbs, data = [p.SerializeToString() for p in probs], rs.union_data(probs)
    sb = wire.SolverParams().SerializeToString()
    with rs.options(solve_mod, dtype="f32"):
        batch = solve_mod.solve_batch(pbs, None, sb, data)
        single = singles(solve_mod, pbs, [[]] * 4, sb, data)
    rs.assert_identical(batch, single)
    assert all(rs.status(st).state == wire.SolverStatus.OPTIMAL for st, _ in batch)
