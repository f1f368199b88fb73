"""Self-check of the references, the bounds and M_SPREAD of tests/test_gpu_factor_ops.py, on the CPU.
Every row of the GPU table is evaluated in the tested dtype three times - LAPACK potrf + potri; LAPACK
potrf + trtri + X^T X; a numpy emulation of the order of csrc/kernels_factor.hip (64-column
left-looking steps inside 256-panels, a right-looking trailing update, 64-block inverses grown by
X21 = -X22 (L21 X11), X^T X) - and a slab row a fourth time, potrs on the unit columns.  Each must
factor without failure and stay inside the bounds (a), (b) and (c) of the GPU tests with its own L, X
and W: a bound or a reference that a correct evaluation can miss shows here, before any kernel is
blamed.  (b) is a theorem for substitution only; that the emulated doubling stays inside it on every
row is what makes it a fair condition on these inputs.

M_SPREAD, the factor of the end-to-end check (d), is measured here among the CPU evaluations alone:
the largest ratio between two of them over the whole table, rounded up to a power of two, at least 2."""

import math

import numpy as np
import pytest

from tests import test_gpu_factor_ops as gf

GROUPS = ("one block", "doubling", "outer panel", "512-block", "four panels", "kappa", "slab")


def test_groups_cover_the_case_table():
    assert sum(len([r for r in gf.ALL_ROWS if r.group == g]) for g in GROUPS) == len(gf.ALL_ROWS)
    assert all(r.note for r in gf.ALL_ROWS)  # every row names its branch
    ids = [gf.row_id(r) for r in gf.ALL_ROWS]
    assert len(set(ids)) == len(ids)
    assert all(r.dtypes and set(r.dtypes) <= set(gf.BOTH) for r in gf.ALL_ROWS)
    for r in gf.SLAB_ROWS:
        assert 0 <= r.lo and 0 <= r.cnt and r.lo + r.cnt <= r.n
    # the table of the issue, row for row
    assert [r.n for r in gf.SIZE_ROWS if r.kappa == 1e2] == [1, 2, 63, 64, 65, 128, 129, 192, 193, 255, 256, 257,
                                                             320, 321, 512, 513, 577, 1026, 1090]
    assert sorted((r.n, r.kappa, r.dtypes) for r in gf.SIZE_ROWS if r.kappa != 1e2) == [
        (321, 1e4, gf.BOTH), (321, 1e8, ("f64",)), (577, 1e4, gf.BOTH), (577, 1e8, ("f64",))]
    assert [(r.n, r.lo, r.cnt) for r in gf.SLAB_ROWS] == [
        (65, 0, 65), (65, 64, 1), (300, 0, 0), (577, 0, 16), (577, 0, 17), (577, 500, 77), (577, 512, 65),
        (577, 576, 1), (1090, 1030, 17), (1090, 0, 1090)]


def test_inputs_are_symmetric_f32_values_of_the_stated_conditioning():
    for r in gf.ALL_ROWS:
        A = gf.make_matrix(r)
        assert np.array_equal(A, A.T) and np.array_equal(A, A.astype(np.float32).astype(np.float64))
        if r.n >= 63:
            d = 1.0 / np.sqrt(np.diag(A))
            w = np.linalg.eigvalsh(A * d[:, None] * d[None, :])
            assert w[0] > 0
            rows = np.sqrt(np.diag(A))
            assert rows.max() / rows.min() > 10  # rows of very different scale


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("group", GROUPS)
def test_tested_precision_stays_inside_the_bounds(group, dtype):
    worst = {"a": 0.0, "b": 0.0, "c": 0.0}
    for r in gf.ALL_ROWS:
        if r.group != group or dtype not in r.dtypes:
            continue
        A = gf.make_matrix(r)
        for name, e, stat in gf.cpu_evaluations(r, dtype):  # (factors without failure, or raises)
            what = "%s %s %s" % (gf.row_id(r), dtype, name)
            ra = gf.ratio_factor(e["L"], A, dtype)
            assert np.array_equal(np.triu(e["L"], 1), np.zeros_like(A))
            assert ra <= 1.0, "%s (a): %.3g x the bound" % (what, ra)
            worst["a"] = max(worst["a"], ra)
            if e["X"] is not None:
                assert np.array_equal(np.triu(e["X"], 1), np.zeros_like(A))
                rb, rc = gf.ratio_inverse(e["X"], e["L"], dtype), gf.ratio_product(e["W"], e["X"], dtype)
                assert rb <= 1.0, "%s (b): %.3g x the bound" % (what, rb)
                assert rc <= 1.0, "%s (c): %.3g x the bound" % (what, rc)
                worst["b"], worst["c"] = max(worst["b"], rb), max(worst["c"], rc)
            assert np.isfinite(stat)
    print("%s %s: largest error / bound over the rows: (a) %.3g (b) %.3g (c) %.3g" % (
        group, dtype, worst["a"], worst["b"], worst["c"]))


def spread(r, dtype):
    stats = [gf.floored(s, dtype) for _, _, s in gf.cpu_evaluations(r, dtype)]
    return max(stats) / min(stats)


def test_m_spread_is_the_spread_among_the_cpu_evaluations():
    worst = {}
    for dtype in gf.BOTH:
        ratios = [(spread(r, dtype), gf.row_id(r)) for r in gf.ALL_ROWS if dtype in r.dtypes]
        worst[dtype] = max(ratios)
        print("%s: largest ratio between two CPU evaluations %.3g at %s" % ((dtype,) + worst[dtype]))
    largest = max(w[0] for w in worst.values())
    M = max(2, 2 ** int(math.ceil(math.log(largest, 2))))
    assert gf.M_SPREAD == M, "the CPU evaluations spread by %.3g: M_SPREAD must be %d" % (largest, M)


def test_the_emulation_is_a_faithful_order():
    """On a matrix whose factor, inverse and product are exact in f32 every order gives the same
    bits; and the emulation with the sign of X21 dropped leaves the bounds (the checks can fail)."""
    n = 130
    L = np.eye(n) * 2.0 + np.tril(np.ones((n, n)), -1) * (np.arange(n)[:, None] % 2 == 0) * (np.arange(n)[None, :] % 64 == 0)
    A = L.dot(L.T)
    for name, fn in gf.EVALUATIONS:
        assert np.array_equal(fn(A, np.float32)["L"], L), name
    r = gf.SIZE_ROWS[6]  # n = 129
    bad = gf.eval_emulated(gf.make_matrix(r), np.float32, sign=1.0)
    bad = {k: v.astype(np.float64) for k, v in bad.items()}
    assert gf.ratio_inverse(bad["X"], bad["L"], "f32") > 1.0
    assert gf.statistic(bad["W"], gf.inv64(r.n, r.kappa)) > gf.end_to_end_bound(r, "f32")


def test_not_positive_definite_inputs_fail_in_every_evaluation():
    for name, make in gf.NOT_PD:
        for T in (np.float32, np.float64):
            for ename, fn in gf.EVALUATIONS:
                if "nan" in name and fn is not gf.eval_emulated:
                    continue  # what a LAPACK build makes of a NaN pivot is its own business
                with pytest.raises(gf.NotPositiveDefinite):
                    fn(make(), T)
