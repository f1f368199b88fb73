"""Self-check of the reference and the forward error bounds of tests/test_gpu_gemm_ops.py, on the
CPU: every row of the GPU case table is evaluated in the tested precision in three orders - numpy's
own product in that dtype (BLAS order, possibly fused), a plain sequential loop over k, and sums of
32-term chunks added in order (the shape of the slabbed and split-K orders) - and all three must stay
inside the bound the GPU tests hold the kernels to.  A bound or a reference that a correct evaluation
can miss shows here, before any kernel is blamed."""

import numpy as np
import pytest

from tests import test_gpu_gemm_ops as gg

GROUPS = {
    "small": gg.SMALL_CASES, "generic": gg.GENERIC_CASES, "mfma_f32": gg.MFMA_F32_CASES,
    "mfma_f64": gg.MFMA_F64_CASES, "mfma_f32_pipe": gg.PIPE_F32_CASES, "mfma_f64_pipe": gg.PIPE_F64_CASES,
    "split_k": gg.SPLIT_K_CASES, "multi_gemv": gg.MULTI_CASES, "f16_edge": gg.F16_EDGE_CASES,
    "variants": gg.VARIANT_CASES, "lower_only": gg.LOWER_CASES, "batched": gg.BATCHED_CASES,
    "mat_copy": gg.MAT_COPY_CASES, "add_diag": gg.ADD_DIAG_CASES, "symmetrize": gg.SYMMETRIZE_CASES,
    "col_abs_sums": gg.COL_ABS_SUMS_CASES, "kron": gg.KRON_CASES,
}
HELPERS = ("mat_copy", "add_diag", "symmetrize", "col_abs_sums", "kron")
ORDERS = ("numpy", "sequential", "chunks of 32")


def test_groups_cover_the_case_table():
    assert sum(len(g) for g in GROUPS.values()) == len(gg.ALL_CASES)
    assert all(c.note for c in gg.ALL_CASES)  # every row names its branch
    for c in gg.GEMM_CASES:  # and its route, in every dtype it runs in
        assert c.routes and all(c.routes.values()), gg.case_id(c)
    for name, group in GROUPS.items():
        ids = [gg.case_id(c) for c in group]
        assert len(set(ids)) == len(ids), name


def test_the_variant_subset_has_an_interior_and_a_ragged_shape_per_kernel():
    for mode, V, dtypes, shapes, route, fallback in gg.VARIANT_SHAPES:
        if route == "split_k":
            continue  # one shape: its parts are whole products of their own
        assert any(M % 32 == 0 and N % 32 == 0 for M, N, K in shapes) and any(M % 32 and N % 32 for M, N, K in shapes)


def product(A, B, T, order):
    """A B in the precision T, A M x K and B K x N given as float64 arrays of T-representable values."""
    A, B = A.astype(T), B.astype(T)
    M, K = A.shape
    N = B.shape[1]
    if order == "numpy":
        s = A.dot(B)
    elif order == "sequential":
        s = np.zeros((M, N), dtype=T)
        cols = np.ascontiguousarray(A.T)
        for k in range(K):
            s += cols[k][:, None] * B[k][None, :]
    else:
        s = np.zeros((M, N), dtype=T)
        for k0 in range(0, K, 32):
            s += A[:, k0:k0 + 32].dot(B[k0:k0 + 32])
    assert s.dtype == T
    return s


def evaluate(c, d, z, T, order):
    s = product(gg.op_of(d["A"][z], c.ta), gg.op_of(d["B"][z], c.tb), T, order)
    out = T(c.alpha) * s
    if c.beta != 0:
        out = out + T(c.beta) * d["C"][z].astype(T)
    assert out.dtype == T
    return out.astype(np.float64)


def evaluate_helper(c, h, T, order):
    kw = h["kw"]
    if c.op == "mat_copy":
        src = kw["a"][gg.cells(0, c.N if c.ta else c.M, c.M if c.ta else c.N, kw["lda"])].astype(T)
        return (T(c.alpha) * gg.op_of(src, c.ta)).astype(np.float64)
    if c.op == "add_diag":
        W = h["W"].astype(T)
        inc = T(c.alpha) * kw["d"].astype(T) if kw["d"] is not None else np.full(c.M, T(c.alpha))
        return (W + np.diag(inc)).astype(np.float64)
    if c.op == "symmetrize":
        L = np.tril(h["W"]).astype(T)
        return (L + np.tril(L, -1).T).astype(np.float64)
    if c.op == "col_abs_sums":  # fp64 sums whatever the dtype
        A = np.abs(kw["a"][gg.cells(0, c.M, c.N, kw["lda"])])
        return np.cumsum(A, axis=0)[-1] if order == "sequential" else A.sum(axis=0)
    A = kw["a"].reshape((c.M, c.N), order="F").astype(T)
    B = kw["b"].reshape((c.K, c.batch), order="F").astype(T)
    out = np.kron(A, B)
    assert out.dtype == T
    return out.astype(np.float64)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_tested_precision_stays_inside_the_bound(group, dtype):
    T = gg.NP_DT[dtype]
    worst = 0.0
    for c in GROUPS[group]:
        if group in HELPERS:
            h = gg.helper_data(c, dtype)
            pairs = [(h["ref"], h["tol"], lambda order: evaluate_helper(c, h, T, order), None)]
        elif dtype not in c.routes:
            continue
        else:
            d = gg.make_data(c, dtype)
            low = np.arange(c.M)[:, None] >= np.arange(c.N)[None, :] if c.lower else None
            pairs = []
            for z in range(c.batch * c.outer):
                ref, mag = gg.reference(c, d, z)
                pairs.append((ref, gg.tolerance(c, mag, dtype), lambda order, z=z: evaluate(c, d, z, T, order), low))
        for ref, tol, run, where in pairs:
            for order in ORDERS:
                got = run(order)
                gg.check_entries(c, "%s, %s" % (dtype, order), got, ref, tol, where)
                with np.errstate(invalid="ignore", divide="ignore"):
                    ratio = np.where(np.asarray(tol) > 0, np.abs(got - ref) / tol, 0.0)
                worst = max(worst, float(np.max(ratio)) if np.size(ratio) else 0.0)
    assert worst <= 1.0
    print("%s %s: largest error / bound over the table: %.3g" % (group, dtype, worst))


def test_reference_is_exact_where_it_can_be():
    """On small integers every product and sum is exact in f32: reference and the three orders agree
    to the bit, whatever the order."""
    c = gg.case("gemm", "auto", 33, 31, 33, tt=(1, 0), ab=(1.25, 0.5), route="small", note="exact")
    rng = np.random.RandomState(0)
    d = {"A": [rng.randint(-8, 9, size=(33, 33)).astype(np.float64)],
         "B": [rng.randint(-8, 9, size=(33, 31)).astype(np.float64)],
         "C": [rng.randint(-8, 9, size=(33, 31)).astype(np.float64) * 4]}
    ref, mag = gg.reference(c, d, 0)
    for order in ORDERS:
        assert np.array_equal(evaluate(c, d, 0, np.float32, order), ref)
    assert np.all(gg.tolerance(c, mag, "f32") >= 0)


def test_layouts_keep_batch_members_apart():
    """The strides of every batched row: past the contiguous values, distinct, those of A and B
    multiples of 4, and no two results share an element."""
    for c in gg.BATCHED_CASES + [c for c in gg.LOWER_CASES if c.op == "gemm_batched"]:
        L = gg.layout(c)
        ar, ac, br, bc = gg.stored(c)
        assert L["sC"] > L["ldc"] * c.N and all(L[s] % 4 == 0 for s in ("sA", "sB", "sA2", "sB2"))
        if c.batch * c.outer == 6:
            assert L["sA"] in (0, ) or L["sA"] > L["lda"] * ac
            assert L["sB"] > L["ldb"] * bc and L["sA2"] not in (c.batch * L["sA"],) and L["sA2"] > 0
            assert (L["sB2"] == 0) == (c.shared == "sB20") and (L["sA"] == 0) == (c.shared == "sA0")
            assert L["sB2"] != c.batch * L["sB"]
        d = gg.make_data(c, "f32")
        seen = np.concatenate([i.reshape(-1) for i in d["idx"]])
        assert len(np.unique(seen)) == seen.size == c.batch * c.outer * c.M * c.N
