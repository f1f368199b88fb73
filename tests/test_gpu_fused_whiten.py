"""The whitened route of the fused lasso sweep: f32, m >= 2048, one GPU.  The pass
streams A_hat = X A (X = L^-1 of the cached inverse's Cholesky factor) and its partials reduce
to X p directly, so no inverse apply runs in the sweep.  EPSILON_HIP_FUSED_WHITEN=0 keeps the
explicit inverse apply; it is read once per process, so that side runs in a child process
(this file run as a script)."""

import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

# torch first: it carries its own HIP runtime (see test_gpu_full_size.py)
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from epsilon_amd import problems, wire  # noqa: E402

pytestmark = pytest.mark.gpu

STATUS_FIELDS = ("r_norm", "s_norm", "epsilon_primal", "epsilon_dual")


def bench_instance(m, n):
    import bench
    At, b, lam = bench.make_instance(m, n, torch.device("cuda", 0))
    prob = bench.build_problem(At, b, lam)
    return At, prob


def run_sweeps(solve_mod, pb, data, sweeps):
    """`sweeps` fused sweeps from a fresh Init, the tags of one profiled sweep after them"""
    solve_mod.set_option("dtype", "f32")
    params = wire.SolverParams(max_iterations=10 ** 9, ignore_stopping_criteria=True)
    s = solve_mod.Solver(pb, params.SerializeToString(), data)
    s.init()
    assert s.run(sweeps - 1) == sweeps - 1
    solve_mod.profile_reset()
    solve_mod.profile_enable(True)
    try:
        assert s.run(1) == 1
        tags = solve_mod.profile_dump()
    finally:
        solve_mod.profile_enable(False)
    st, x = s.result()
    s.close()
    st = wire.SolverStatus.FromString(st)
    return st, {k: np.frombuffer(v).copy() for k, v in x.items()}, tags


def explicit_route(m, n, sweeps):
    """the same sweeps with EPSILON_HIP_FUSED_WHITEN=0, in a child process"""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "explicit.npz")
        env = dict(os.environ, EPSILON_HIP_FUSED_WHITEN="0")
        subprocess.run([sys.executable, os.path.abspath(__file__), str(m), str(n), str(sweeps), out],
                       env=env, cwd=ROOT, check=True, timeout=600)
        z = np.load(out)
        res = {f: float(z["res_" + f]) for f in ("r_norm", "s_norm")}
        x = {k[2:]: z[k] for k in z.files if k.startswith("x_")}
        symv = bool(z["symv"])
    return res, x, symv


def has_symv(tags):
    return any(t.split(":")[0].startswith(("symv", "batch_symv")) for t in tags)


@pytest.mark.parametrize("m,n", [(2048, 8192), (10000, 50000)])
def test_whitened_sweeps_match_explicit_apply(solve_mod, m, n):
    """30 sweeps on either route agree to the tolerances of the fused-vs-generic full-size check
    (test_gpu_full_size.py); the whitened sweep launches no symmetric inverse apply."""
    At, prob = bench_instance(m, n)
    try:
        st, x, tags = run_sweeps(solve_mod, prob.SerializeToString(), prob.expression_data(), 30)
    finally:
        del At
        torch.cuda.empty_cache()
    names = {t.split(":")[0] for t in tags}
    assert "lasso_fused" in names and "reduce_partials" in names, sorted(tags)
    assert not has_symv(tags), sorted(tags)
    res_e, x_e, symv_e = explicit_route(m, n, 30)
    assert symv_e  # the switch does select the explicit apply
    assert sorted(x) == sorted(x_e)
    for k in x_e:
        scale = max(np.abs(x_e[k]).max(), 1e-3)
        np.testing.assert_allclose(x[k], x_e[k], rtol=0, atol=2e-4 * scale, err_msg=k)
    for f in ("r_norm", "s_norm"):
        np.testing.assert_allclose(getattr(st.residuals, f), res_e[f], rtol=2e-3)


def test_whitened_full_size_reaches_optimal(solve_mod):
    At, prob = bench_instance(10000, 50000)
    try:
        solve_mod.set_option("dtype", "f32")
        st, _ = solve_mod.solve(prob.SerializeToString(), [], wire.SolverParams(max_iterations=2000).SerializeToString(),
                                prob.expression_data())
    finally:
        del At
        torch.cuda.empty_cache()
    assert wire.SolverStatus.FromString(st).state == wire.SolverStatus.OPTIMAL


def whitening_tag(m, n):
    return "gemm_f16split_krange:%dx%d" % (m * n, m)


def test_lambda_path_batch_shares_whitened_matrix(solve_mod):
    """A lambda path at 2048 x 8192 in one batch: the bits of its single solves, one whitening
    product for all members and no inverse apply in the sweeps."""
    m, n = 2048, 8192
    A, b = problems.regression_data(m, n, seed=11)
    lmax = np.abs(A.T.dot(b)).max()
    from epsilon_amd import ir
    probs = [problems.lasso_ir(ir.dense_matrix(A), ir.constant(b), f * lmax, n) for f in (0.5, 0.3, 0.2)]
    pbs = [p.SerializeToString() for p in probs]
    data = {}
    for p in probs:
        data.update(p.expression_data())
    sb = wire.SolverParams(max_iterations=300).SerializeToString()
    solve_mod.set_option("dtype", "f32")
    solve_mod.profile_reset()
    solve_mod.profile_enable(True)
    try:
        batch = solve_mod.solve_batch(pbs, None, sb, data)
        tags = solve_mod.profile_dump()
    finally:
        solve_mod.profile_enable(False)
    single = [solve_mod.solve(pb, [], sb, data) for pb in pbs]
    assert tags.get(whitening_tag(m, n), (0, 0))[0] == 1, sorted(tags)
    assert not has_symv(tags), sorted(tags)
    assert "batch_fused_pass" in {t.split(":")[0] for t in tags}, sorted(tags)
    for (stb, xb), (sts, xs) in zip(batch, single):
        a, s = wire.SolverStatus.FromString(stb), wire.SolverStatus.FromString(sts)
        assert a.state == s.state and a.num_iterations == s.num_iterations
        for f in STATUS_FIELDS:
            assert getattr(a.residuals, f) == getattr(s.residuals, f), f
        assert sorted(xb) == sorted(xs)
        for v in xs:
            assert np.array_equal(np.frombuffer(xb[v]), np.frombuffer(xs[v])), v


def test_warm_reinit_issues_no_product(solve_mod):
    """Re-binding the rhs and re-running Init finds the inverse, its factor and A_hat cached: no
    product is formed, the sweeps stay on the whitened route and the warm solve converges."""
    from epsilon_amd import ir
    m, n = 2048, 8192
    A, b = problems.regression_data(m, n, seed=12)
    lam = 0.3 * np.abs(A.T.dot(b)).max()
    prob = problems.lasso_ir(ir.dense_matrix(A), ir.parameter(m, 1, "param:b"), lam, n)
    b2 = b + 0.05 * np.random.RandomState(0).randn(m)

    def bind(v):
        d = {}
        c = ir.store(np.asarray(v, dtype=np.float64).reshape(-1, 1), d)
        return ("param:b", c.SerializeToString()), d

    (p1, d1), (p2, d2) = bind(b), bind(b2)
    data = dict(prob.expression_data())
    data.update(d1)
    data.update(d2)
    pb = prob.SerializeToString()
    sb = wire.SolverParams(warm_start=True).SerializeToString()
    solve_mod.set_option("dtype", "f32")
    s = solve_mod.Solver(pb, sb, data)
    try:
        s.set_parameter(*p1)
        solve_mod.profile_reset()
        solve_mod.profile_enable(True)
        s.init()
        tags1 = solve_mod.profile_dump()
        solve_mod.profile_enable(False)
        s.run(-1)
        s.set_parameter(*p2)
        solve_mod.profile_reset()
        solve_mod.profile_enable(True)
        s.init()
        tags2 = solve_mod.profile_dump()
        s.run(3)
        tags_sweep = solve_mod.profile_dump()
        solve_mod.profile_enable(False)
        s.run(-1)
        st2, _ = s.result()
    finally:
        solve_mod.profile_enable(False)
        s.close()
    assert tags1.get(whitening_tag(m, n), (0, 0))[0] == 1, sorted(tags1)
    assert not any(t.startswith(("syrk", "gemm", "spd_inverse")) for t in tags2), sorted(tags2)
    assert not has_symv(tags_sweep), sorted(tags_sweep)
    assert wire.SolverStatus.FromString(st2).state == wire.SolverStatus.OPTIMAL


def _child(m, n, sweeps, out):
    from epsilon_amd import _solve
    At, prob = bench_instance(m, n)
    st, x, tags = run_sweeps(_solve, prob.SerializeToString(), prob.expression_data(), sweeps)
    z = {"x_" + k: v for k, v in x.items()}
    for f in ("r_norm", "s_norm"):
        z["res_" + f] = np.float64(getattr(st.residuals, f))
    z["symv"] = np.bool_(has_symv(tags))
    np.savez(out, **z)


if __name__ == "__main__":
    _child(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
