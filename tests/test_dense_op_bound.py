"""Self-check of the reference and the forward error bounds of tests/test_gpu_dense_ops.py, on the
CPU: every case of the GPU case table is evaluated in the tested precision, once with numpy's own
products and sums in that precision (BLAS order, possibly fused) and once by a plain sequential loop
over the contraction index, and both must stay inside the bound the GPU tests hold the kernels to.
A bound or a reference that a correct evaluation can miss shows here, before any kernel is blamed."""

import math

import numpy as np
import pytest

from tests import test_gpu_dense_ops as gd

GROUPS = {
    "gemv_n": gd.GEMV_N_CASES, "gemv_t": gd.GEMV_T_CASES, "symv": gd.SYMV_CASES + gd.SYMV_PACKED_CASES,
    "reduce_partials": gd.RP_CASES + gd.RP_ALIGN_CASES, "reductions": gd.RED_CASES,
    "elementwise": gd.AXPBY_CASES + gd.DIAG_MUL_CASES,
}


def test_groups_cover_the_case_table():
    assert sum(len(g) for g in GROUPS.values()) == len(gd.ALL_CASES)
    assert all(c.note for c in gd.ALL_CASES)  # every row names its branch


def finish(c, d, s, T):
    """alpha s + beta y (+ add) in the precision T, as the epilogues do."""
    out = T(c.alpha) * s
    if c.beta != 0:
        out = out + T(c.beta) * d["y"].astype(T)
    if c.add:
        out = out + d["add"].astype(T)
    assert out.dtype == T
    return out.astype(np.float64)


def evaluate(c, d, dtype, sequential):
    T = gd.NP_DT[dtype]
    if c.op in ("sumsq", "sumsq_diff", "dot"):
        # fp64 accumulation of exact (f32) or once-rounded (f64) terms, in either dtype
        x = d["x"]
        terms = x * x if c.op == "sumsq" else (x - d["y"]) ** 2 if c.op == "sumsq_diff" else x * d["y"]
        if sequential:
            total = float(np.cumsum(terms)[-1]) if terms.size else 0.0
        else:
            total = float(np.sum(terms))  # pairwise
        return (gd.PRESET if c.acc else 0.0) + total
    if c.op in ("axpby", "diag_mul"):
        x, y = d["x"].astype(T), d["y"].astype(T)
        if sequential:  # every operation rounded
            t = T(c.alpha) * x if c.op == "axpby" else T(c.alpha) * (d["A"].astype(T) * x)
            out = t + T(c.beta) * y if c.beta != 0 else t
            assert out.dtype == T
            return out.astype(np.float64)
        # the other extreme: one rounding of the exact-in-fp64 expression (contracted forms)
        t = c.alpha * d["x"] if c.op == "axpby" else c.alpha * d["A"] * d["x"]
        return (t + (c.beta * d["y"] if c.beta != 0 else 0.0)).astype(T).astype(np.float64)
    M, v, k = gd.contraction(c, d)
    rows = M.shape[0]
    if not sequential:
        MT = M.astype(T)
        s = MT.sum(axis=1, dtype=T) if v is None else MT.dot(v.astype(T))
    else:
        cols_of_M = np.ascontiguousarray(M.T.astype(T))  # k x rows
        s = np.zeros(rows, dtype=T)
        if v is None:
            for j in range(k):
                s += cols_of_M[j]
        else:
            vT = v.astype(T)
            for j in range(k):
                s += cols_of_M[j] * vT[j]
    assert s.dtype == T
    return finish(c, d, s, T)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_tested_precision_stays_inside_the_bound(group, dtype):
    worst = 0.0
    for c in GROUPS[group]:
        d = gd.make_data(c, dtype)
        ref, tol = gd.reference(c, d, dtype)
        for sequential in (False, True):
            got = evaluate(c, d, dtype, sequential)
            err = np.abs(got - ref)
            assert np.all(np.isfinite(got)) and np.all(err <= tol), "%s (%s, %s): error %r over the bound %r" % (
                gd.case_id(c), dtype, "sequential" if sequential else "numpy", np.max(err), np.max(tol))
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(np.asarray(tol) > 0, err / tol, 0.0)
            worst = max(worst, float(np.max(ratio)) if np.size(ratio) else 0.0)
    assert worst <= 1.0
    print("%s %s: largest error / bound over the table: %.3g" % (group, dtype, worst))


def test_the_bound_needs_the_add_term():
    """tol = gamma(k + 8) (|alpha| (|A| |x|) + |beta| |y|) alone is not a bound for
    y = (alpha sum + beta y) + add: the last addition rounds relative to |add| too.  A plain f32
    evaluation misses it where the sum is small against add, so the bound carries |add_i|."""
    c = gd.case("reduce_partials", 4096, nparts=1, add=True, ab=(1.0, 0.0))
    d = gd.make_data(c, "f32")
    ref, tol = gd.reference(c, d, "f32")
    got = evaluate(c, d, "f32", True)
    without_add = gd.gamma(c.nparts + 8, gd.U["f32"]) * abs(c.alpha) * np.abs(d["A"]).sum(axis=0)
    err = np.abs(got - ref)
    assert np.all(err <= tol)
    assert np.any(err > without_add)


def test_reference_is_exact_where_it_can_be():
    """On small integers every product and sum is exact in f32: reference, numpy and the sequential
    loop agree to the bit, whatever the order."""
    c = gd.case("gemv_n", 257, 65, ab=(1.25, 0.5))
    rng = np.random.RandomState(0)
    d = {"A": rng.randint(-8, 9, size=(257, 65)).astype(np.float64), "x": rng.randint(-8, 9, size=65).astype(np.float64),
         "y": rng.randint(-8, 9, size=257).astype(np.float64) * 4}
    ref, tol = gd.reference(c, d, "f32")
    for sequential in (False, True):
        assert np.array_equal(evaluate(c, d, "f32", sequential), ref)
    assert np.all(tol >= 0) and math.isclose(gd.gamma(73, 2.0 ** -24), 73 * 2.0 ** -24, rel_tol=1e-5)
