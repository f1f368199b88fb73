"""The resident share of the fused pass (DESIGN.md 3.7 "Residency", option "fused_resident"): the
pass loads a part of the data matrix with the default cache policy, so that it stays in the
Infinity Cache from sweep to sweep, and streams the rest with non-temporal loads.  Only the cache
policy bits of the loads differ, so the claim under test is that NO bit of an iterate depends on the
budget: 25 sweeps from a fresh Init under four budgets - 0 (everything streamed), a cut inside row
chunk 0, one whole chunk plus a cut inside chunk 1, more than the matrix - give the same bytes in
every variable and the same four residuals.

A row chunk is what one load instruction of the workgroup covers: 4 KB of a column at 256 threads,
8 KB at 512.  Rows 2560 (f32: 2.5 chunks, f64: 5) with an odd number of columns (a trailing unpaired
column), 4 (one chunk, smaller than a workgroup), 10244 (the 512-thread form), the two-block driver
and basis pursuit (kChainTwoBlock and kChainZeroCols) on small shapes, and a 3-member lambda path
through solve_batch at 2048 x 4100 (the batched pass, on the whitened route)."""

import ctypes

import numpy as np
import pytest

from epsilon_amd import problems, wire
from tests import route_support as rs

pytestmark = pytest.mark.gpu

RESIDUALS = ("r_norm", "s_norm", "epsilon_primal", "epsilon_dual")
SWEEPS = 25


def rule(mod, m, n, dtype, budget_bytes):
    q, j, b = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
    mod._check(mod.lib().eps_fused_residency(ctypes.c_int64(m), ctypes.c_int64(n), ctypes.c_int(dtype == "f64"),
                                             ctypes.c_int64(budget_bytes), ctypes.byref(q), ctypes.byref(j),
                                             ctypes.byref(b)))
    return q.value, j.value, b.value


def last_share(mod):
    """the (qfull, jcut) the most recent launch of the pass received"""
    q, j = ctypes.c_int(), ctypes.c_int64()
    mod._check(mod.lib().eps_fused_residency_last(ctypes.byref(q), ctypes.byref(j)))
    return q.value, j.value


def chunk_bytes(m, dtype):
    """a row chunk of one column: 16 bytes per thread, 512 threads where 256 cannot own the rows"""
    return 16 * (512 if m > (5120 if dtype == "f64" else 10240) else 256)


def budgets_kib(mod, m, n, dtype):
    """[0, a cut inside chunk 0, chunk 0 whole and a cut inside chunk 1, more than the matrix] in
    KiB, with the (qfull, jcut) each gives"""
    elem = 8 if dtype == "f64" else 4
    whole = rule(mod, m, n, dtype, m * n * elem)
    chunk0 = min(chunk_bytes(m, dtype), m * elem) * n  # bytes of chunk 0 over all columns
    kib = [0, max(1, int(0.4 * chunk0) // 1024), max(1, int(1.4 * chunk0) // 1024), m * n * elem // 1024 + 1024]
    cuts = [rule(mod, m, n, dtype, k * 1024)[:2] for k in kib]
    print("shape %d x %d %s: budgets (KiB) %s -> (qfull, jcut) %s, whole matrix %s" % (m, n, dtype, kib, cuts, whole))
    assert cuts[0] == (0, 0) and cuts[3] == whole[:2]
    return kib, cuts


def tag_counts(mod):
    out = {}
    for t, (c, _) in mod.profile_dump().items():
        out[t.split(":")[0]] = out.get(t.split(":")[0], 0) + c
    return out


def runs(mod, prob, dtype, budgets, tag, shares=None, **params):
    """25 sweeps from a fresh Init under each budget, on one handle (the data and the factorisation
    are shared, the option is read at every Init): [(residuals, {variable: bytes})].  shares: the
    (qfull, jcut) the pass has to receive under each budget - the iterates cannot show that the
    option reached the kernel."""
    sb = wire.SolverParams(max_iterations=SWEEPS, ignore_stopping_criteria=True, **params).SerializeToString()
    mod.set_option("dtype", dtype)
    s = mod.Solver(prob.SerializeToString(), sb, prob.expression_data())
    out = []
    try:
        for budget in budgets:
            mod.set_option("fused_resident", budget)
            mod.profile_reset()
            mod.profile_enable(True)
            s.init()
            s.run(-1)
            tags = tag_counts(mod)
            mod.profile_enable(False)
            st, x = s.result()
            assert rs.status(st).num_iterations == SWEEPS
            if tag is not None:
                assert tags.get(tag, 0) >= SWEEPS, (budget, tags)  # the fused pass ran every sweep
                if shares is not None:
                    assert last_share(mod) == shares[len(out)], (budget, last_share(mod), shares)
            else:
                assert not any(t.endswith("_fused") for t in tags), (budget, tags)
            out.append((tuple(getattr(rs.status(st).residuals, f) for f in RESIDUALS), {k: bytes(v) for k, v in x.items()}))
    finally:
        mod.profile_enable(False)
        s.close()
        mod.set_option("fused_resident", "auto")
        mod.set_option("dtype", "f32")
    return out


def assert_same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    assert sorted(a[1]) == sorted(b[1])
    for k in a[1]:
        assert a[1][k] == b[1][k], (what, k)


_made = {}


def make(kind, m, n):
    if (kind, m, n) not in _made:
        _made[(kind, m, n)] = (problems.basis_pursuit(m, n) if kind == "bp" else problems.lasso(m, n, seed=2))[0]
    return _made[(kind, m, n)]


# The multi-block driver eliminates a tall least-squares term (m > n) to the n x n Gram and keeps it
# on the operator path (test_gpu_parity.py), so each tall shape has a fat one with the same rows
# beside it that does take the pass; the tall ones run too: the option must not change them either.
CASES = [
    ("lasso", 2560, 301, "f32", {}, None),
    ("lasso", 2560, 301, "f64", {}, None),
    ("lasso", 4, 3, "f32", {}, None),
    ("lasso", 10244, 64, "f32", {}, None),
    ("lasso", 2560, 2701, "f32", {}, "lasso_fused"),    # last row chunk half filled, trailing unpaired column
    ("lasso", 2560, 2701, "f64", {}, "lasso_fused"),
    ("lasso", 4, 7, "f32", {}, "lasso_fused"),          # one chunk, smaller than a workgroup
    ("lasso", 10244, 10261, "f32", {}, "lasso_fused"),  # the 512-thread form
    ("lasso", 1536, 1601, "f32", {"solver": 1}, "lasso_fused"),  # two-block driver: kChainTwoBlock
    ("bp", 1536, 2051, "f32", {}, "zero_fused"),                 # ZERO route: kChainZeroCols
]


@pytest.mark.parametrize("kind,m,n,dtype,params,tag", CASES)
def test_iterates_do_not_depend_on_the_budget(solve_mod, kind, m, n, dtype, params, tag):
    prob = make(kind, m, n)
    kib, cuts = budgets_kib(solve_mod, m, n, dtype)
    if m * (8 if dtype == "f64" else 4) > chunk_bytes(m, dtype):  # more than one chunk per column
        assert cuts[1][0] == 0 and cuts[1][1] > 0 and cuts[2][0] == 1 and cuts[2][1] > 0, cuts
    got = runs(solve_mod, prob, dtype, kib, tag, shares=cuts, **params)
    assert any(np.frombuffer(v).any() for v in got[0][1].values())
    for k, r in zip(kib[1:], got[1:]):
        assert_same(r, got[0], "budget %d KiB" % k)


def test_auto_gives_the_bytes_of_budget_zero(solve_mod):
    """2560 x 2701: smaller than any budget "auto" leaves, and n < 2m keeps the explicit inverse
    apply (whose bytes "auto" subtracts)"""
    m, n = 2560, 2701
    whole = rule(solve_mod, m, n, "f32", m * n * 4)[:2]
    auto, zero = runs(solve_mod, make("lasso", m, n), "f32", ["auto", 0], "lasso_fused", shares=[whole, (0, 0)])
    assert_same(auto, zero, "auto")


def test_batch_members_equal_their_single_solves_under_every_budget(solve_mod):
    m, n = 2048, 4100
    A, b = problems.regression_data(m, n, seed=5)
    lmax = np.abs(A.T.dot(b)).max()
    from epsilon_amd import ir
    probs = [problems.lasso_ir(ir.dense_matrix(A), ir.constant(b), f * lmax, n) for f in (0.5, 0.3, 0.15)]
    pbs = [p.SerializeToString() for p in probs]
    data = {}
    for p in probs:
        data.update(p.expression_data())
    sb = wire.SolverParams(max_iterations=SWEEPS, ignore_stopping_criteria=True).SerializeToString()
    kib, cuts = budgets_kib(solve_mod, m, n, "f32")

    def result(st, x):
        s = rs.status(st)
        assert s.num_iterations == SWEEPS
        return tuple(getattr(s.residuals, f) for f in RESIDUALS), {k: bytes(v) for k, v in x.items()}

    base = None
    for k in kib:
        solve_mod.set_option("fused_resident", k)
        solve_mod.profile_reset()
        solve_mod.profile_enable(True)
        try:
            batch = [result(*r) for r in solve_mod.solve_batch(pbs, None, sb, data)]
            tags = tag_counts(solve_mod)
            assert last_share(solve_mod) == cuts[kib.index(k)], (k, last_share(solve_mod), cuts)
            single = [result(*solve_mod.solve(pb, [], sb, data)) for pb in pbs]
        finally:
            solve_mod.profile_enable(False)
            solve_mod.set_option("fused_resident", "auto")
        assert tags.get("batch_fused_pass", 0) >= SWEEPS, tags
        for i in range(len(pbs)):
            assert_same(batch[i], single[i], "budget %d KiB, member %d against its single solve" % (k, i))
        if base is None:
            base = single
        for i in range(len(pbs)):
            assert_same(single[i], base[i], "budget %d KiB, member %d against budget 0" % (k, i))
