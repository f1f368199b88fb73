"""On the CPU: (1) the self-check of the reference and the forward error bounds of
tests/test_gpu_sparse_ops.py - every case of its tables is evaluated in the tested precision in
several summation orders (forward, reversed, pairwise, and dealt to 1, 2, ..., 64 and 256 lanes that
are then folded as the kernels fold them), and each must stay inside the bound the GPU tests hold the
kernels to: the bound, not luck, decides the outcome; (2) the host CSC algebra of csrc/sparse.cc through
eps_test_csc_op, on integer-valued matrices (fp64 sums and products are exact in any order) compared
exactly with dense numpy / scipy references, every result checked against the HostCsc invariants."""

import os

import numpy as np
import pytest
import scipy.sparse as sp

from epsilon_amd import _solve
from tests import test_gpu_sparse_ops as gs

LANES = (1, 2, 4, 8, 16, 32, 64, 256)
ORDERS = ["forward", "reversed", "pairwise"] + ["lanes%d" % n for n in LANES]


def test_the_tables_name_their_branches():
    assert all(c.note for c in gs.ALL_CASES)
    assert len({c.name for c in gs.ALL_CASES}) == len(gs.ALL_CASES)
    assert {gs.lanes_of(c.lens) for c in gs.SPMV_CASES} == set(LANES)
    # both sides of every switch of Spmv: avg L | L + 1 for each LANES, and 1023 | 1024
    assert {gs.avg_of(c.lens) for c in gs.SPMV_CASES} >= {0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 1023, 1024}
    for c in gs.SPMV_CASES:
        if "-edge" in c.name or "-above" in c.name:
            assert len(set(c.lens)) > 2 and 0 in c.lens and max(c.lens) > gs.lanes_of(c.lens) % 256


# ---- summation orders, vectorised over the output entries: P holds one sum per row, zero-padded (adding
# a zero is exact, so the padding changes no partial sum)

def fold(P):
    """Sequential sum of the columns of P, in P's precision."""
    s = np.zeros(P.shape[0], dtype=P.dtype)
    for j in range(P.shape[1]):
        s = s + P[:, j]
    return s


def pairwise(P):
    while P.shape[1] > 1:
        if P.shape[1] % 2:
            P = np.concatenate([P, np.zeros((P.shape[0], 1), dtype=P.dtype)], axis=1)
        P = P[:, 0::2] + P[:, 1::2]
    return P[:, 0] if P.shape[1] else np.zeros(P.shape[0], dtype=P.dtype)


def by_lanes(P, lanes):
    """Entry p goes to lane p % lanes, each lane sums its own in order; the lanes are folded as the
    shuffle loops fold them (lane i += lane i + off, off = lanes / 2 ... 1).  256: four waves of 64
    folded that way, then added in order (SpmvCsrBlockKernel)."""
    part = np.stack([fold(P[:, lane::lanes]) for lane in range(lanes)], axis=1)
    width = min(lanes, 64)
    off = width // 2
    while off:
        for base in range(0, lanes, width):
            part[:, base:base + off] = part[:, base:base + off] + part[:, base + off:base + 2 * off]
        off //= 2
    return fold(part[:, ::width])


def summed(P, order):
    if order == "forward":
        return fold(P)
    if order == "reversed":
        return fold(P[:, ::-1])
    if order == "pairwise":
        return pairwise(P)
    return by_lanes(P, int(order[5:]))


def products(c, d, T):
    """(P, live): the rounded products of every output entry with at least one term, one row of P
    each, zero-padded; live: the (row of S, column of X) of each."""
    S, X = gs.contraction(c, d)
    lens = np.asarray(c.lens)
    rows = np.nonzero(lens)[0]
    kmax = int(lens.max()) if lens.size else 0
    N = X.shape[1]
    if rows.size == 0:
        return np.zeros((0, 0), dtype=T), rows, N
    pos = d["ptr"][rows].astype(np.int64)[:, None] + np.arange(kmax)[None, :]
    mask = np.arange(kmax)[None, :] < lens[rows][:, None]
    pos = np.where(mask, pos, 0)
    V = np.where(mask, d["val"][pos], 0.0).astype(T)          # rows x kmax
    J = d["idx"][pos]                                          # rows x kmax
    XT = X.astype(T)
    P = np.concatenate([V * np.where(mask, XT[J, j], T(0)) for j in range(N)], axis=0)  # column j after j - 1
    assert P.dtype == T
    return P, rows, N


def evaluate(c, d, dtype, order, P, rows, N):
    T = gs.NP_DT[dtype]
    s = np.zeros((c.rows, N), dtype=T)
    if rows.size:
        s[rows, :] = summed(P, order).reshape(N, rows.size).T
    out = T(c.alpha) * s
    if c.beta != 0:
        out = out + T(c.beta) * d["y"].astype(T).reshape(-1, 1)
    assert out.dtype == T
    return gs.device_layout(c, out.astype(np.float64))


GROUPS = {"spmv": gs.SPMV_CASES, "spmm_csr_dense": gs.SPMM_CASES, "dense_spmm_csc": gs.DSPMM_CASES,
          "limit": gs.LIMIT_CASES}


def test_groups_cover_the_case_table():
    assert sum(len(g) for g in GROUPS.values()) + len(gs.SCATTER_CASES) == len(gs.ALL_CASES)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_tested_precision_stays_inside_the_bound(group, dtype):
    worst = 0.0
    for c in GROUPS[group]:
        d = gs.make_data(c, dtype)
        ref, tol = gs.reference(c, dtype)
        P, rows, N = products(c, d, gs.NP_DT[dtype])
        for order in ORDERS:
            got = evaluate(c, d, dtype, order, P, rows, N)
            err = np.abs(got - ref)
            assert np.all(np.isfinite(got)) and np.all(err <= tol), "%s (%s, %s): error %r over the bound %r" % (
                c.name, dtype, order, np.max(err), np.max(tol))
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(tol > 0, err / tol, 0.0)
            worst = max(worst, float(np.max(ratio)) if ratio.size else 0.0)
    assert worst <= 1.0
    print("%s %s: largest error / bound over the table: %.3g" % (group, dtype, worst))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_scatter_stays_inside_the_bound(dtype):
    """W + alpha v with both operations rounded, and with one rounding of the exact sum (FMA)."""
    T = gs.NP_DT[dtype]
    for c in gs.SCATTER_CASES:
        d = gs.make_data(c, dtype)
        ref, tol = gs.reference(c, dtype)
        add = np.zeros((c.cols, c.rows))
        add[d["idx"], np.repeat(np.arange(c.rows), c.lens)] = d["val"]
        two = d["W"].astype(T) + T(c.alpha) * add.astype(T)
        assert two.dtype == T
        ext = np.longdouble
        one = (d["W"].astype(ext) + ext(c.alpha) * add.astype(ext)).astype(T)
        for got in (two, one):
            err = np.abs(got.astype(np.float64).flatten(order="F") - ref).astype(np.float64)
            assert np.all(err <= tol), "%s (%s): error %r over the bound" % (c.name, dtype, np.max(err))
            assert np.array_equal(got[add == 0], d["W"][add == 0])


def test_reference_is_exact_where_it_can_be():
    """On small integers every product and sum is exact in f32: the reference and every summation
    order agree to the bit."""
    c = next(c for c in gs.SPMV_CASES if c.name.startswith("spmv-L16-edge") and c.beta != 0)
    rng = np.random.RandomState(0)
    d = dict(gs.make_data(c, "f32"))
    d["val"] = rng.randint(-8, 9, size=d["val"].size).astype(np.float64)
    d["x"] = rng.randint(-8, 9, size=c.cols).astype(np.float64)
    d["y"] = rng.randint(-8, 9, size=c.rows).astype(np.float64) * 4
    S, X = gs.contraction(c, d)
    ref = c.alpha * np.asarray(S.dot(X)).reshape(-1) + c.beta * d["y"]
    P, rows, N = products(c, d, np.float32)
    for order in ORDERS:
        assert np.array_equal(evaluate(c, d, "f32", order, P, rows, N), ref), order


# ---- the host CSC algebra through csc_op ---------------------------------------------------------------

@pytest.fixture(scope="module")
def csc_op():
    if not os.path.exists(_solve.LIB_PATH):
        pytest.fail("libepsilon_hip.so is not built")
    return _solve.csc_op


def operand(M):
    """A scipy matrix (or a dense array) as a csc_op operand, canonical form."""
    M = sp.csc_matrix(M)
    M.sort_indices()
    return (M.shape[0], M.shape[1], M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(np.float64))


def check_invariants(res):
    m, n, colptr, rowidx, val = res
    assert colptr.shape == (n + 1,) and colptr[0] == 0 and colptr[-1] == len(rowidx) == len(val)
    assert np.all(np.diff(colptr) >= 0)
    assert np.all((rowidx >= 0) & (rowidx < m)) if len(rowidx) else True
    inner = np.ones(len(rowidx), dtype=bool)
    inner[colptr[:-1][np.diff(colptr) > 0]] = False  # the first entry of every column
    assert np.all(np.diff(rowidx.astype(np.int64))[inner[1:]] > 0), "row indices not strictly ascending in a column"
    return res


def as_scipy(res):
    m, n, colptr, rowidx, val = check_invariants(res)
    return sp.csc_matrix((val, rowidx, colptr), shape=(m, n))


def dense_of(res):
    return np.asarray(as_scipy(res).todense())


def int_matrix(rng, m, n, density):
    """Small non-zero integers at a `density` share of the entries."""
    mask = rng.rand(m, n) < density
    return np.where(mask, rng.randint(1, 9, size=(m, n)) * rng.choice([-1, 1], size=(m, n)), 0).astype(np.float64)


def same_bits(res, M):
    """res is the canonical CSC form of the scipy matrix M, structure and values."""
    want = operand(M)
    assert res[0] == want[0] and res[1] == want[1]
    for got, exp in zip(res[2:], want[2:]):
        assert np.array_equal(got, exp)


def test_transpose(csc_op):
    rng = np.random.RandomState(1)
    A = int_matrix(rng, 9, 13, 0.3)
    A[:, 4] = 0
    A[:, 12] = 0
    A[0, :] = 0
    A[5, :] = 0
    shapes = [np.zeros((4, 6)), np.zeros((0, 3)), np.zeros((3, 0)), A, int_matrix(rng, 1, 17, 0.5),
              int_matrix(rng, 17, 1, 0.5)]
    for M in shapes:
        a = operand(M)
        t = csc_op("transpose", a=a)
        same_bits(check_invariants(t), sp.csc_matrix(M).T)
        back = csc_op("transpose", a=t)
        for got, exp in zip(back, a):  # twice: the input bit for bit
            assert np.array_equal(got, exp)


def test_add(csc_op):
    rng = np.random.RandomState(2)
    A = int_matrix(rng, 11, 8, 0.35)
    even = (np.add.outer(np.arange(11), np.arange(8)) % 2 == 0)
    cases = {"disjoint": (A * even, int_matrix(rng, 11, 8, 0.5) * ~even),
             "identical": (A, A),
             "interleaved": (A, int_matrix(rng, 11, 8, 0.35))}
    for name, (X, Y) in cases.items():
        res = csc_op("add", a=operand(X), b=operand(Y))
        assert np.array_equal(dense_of(res), X + Y), name
        # the structure is the union, cancellation or not
        assert len(res[3]) == np.count_nonzero((X != 0) | (Y != 0)), name
    res = csc_op("add", a=operand(A), b=operand(-A))
    assert np.array_equal(dense_of(res), np.zeros_like(A))
    assert len(res[3]) == np.count_nonzero(A) and np.all(res[4] == 0)  # explicit zeros stay


def test_multiply(csc_op):
    rng = np.random.RandomState(3)
    A = int_matrix(rng, 7, 9, 0.4)
    B = int_matrix(rng, 9, 6, 0.4)
    B[:, 2] = 0                 # empty columns in B
    B[:, 5] = 0
    A[3, :] = [1, -2, 3, 1, 0, 2, -1, 1, 4]   # a dense row of A ...
    B[:, 0] = [1, 1, -1, 2, 0, 1, 3, -2, 1]   # ... met by a dense column of B: row 3 reached 8 times
    res = csc_op("multiply", a=operand(A), b=operand(B))
    assert np.array_equal(dense_of(res), A.dot(B))
    assert res[2][3] == res[2][2] and res[2][6] == res[2][5]  # the empty columns stay empty
    C = int_matrix(rng, 6, 14, 0.3)
    D = int_matrix(rng, 14, 1, 0.6)
    chain = operand(A)
    want = A
    for M in (B, C, D):  # 7 x 9 . 9 x 6 . 6 x 14 . 14 x 1
        chain = csc_op("multiply", a=chain, b=operand(M))
        want = want.dot(M)
        assert np.array_equal(dense_of(chain), want)
    assert chain[:2] == (7, 1)


def test_kron(csc_op):
    rng = np.random.RandomState(4)
    A = int_matrix(rng, 3, 4, 0.6)
    B = int_matrix(rng, 5, 3, 0.5)
    A[:, 1] = 0  # an empty column in either factor
    B[:, 2] = 0
    for X, Y in ((A, B), (B, A), (A, np.zeros((2, 2))), (np.eye(3), B)):
        res = csc_op("kron", a=operand(X), b=operand(Y))
        assert np.array_equal(dense_of(res), np.kron(X, Y))
        assert len(res[3]) == np.count_nonzero(X) * np.count_nonzero(Y)


def test_scale_rows_and_cols(csc_op):
    rng = np.random.RandomState(5)
    A = int_matrix(rng, 6, 9, 0.4)
    r = rng.randint(-4, 5, size=6).astype(np.float64)
    c = rng.randint(-4, 5, size=9).astype(np.float64)
    assert np.array_equal(dense_of(csc_op("scale_rows", a=operand(A), d=r)), r[:, None] * A)
    assert np.array_equal(dense_of(csc_op("scale_cols", a=operand(A), d=c)), A * c[None, :])
    for op in ("scale_rows", "scale_cols"):
        res = csc_op(op, a=operand(A), d=[-3.0])
        assert np.array_equal(dense_of(res), -3.0 * A)
        assert np.array_equal(res[3], operand(A)[3])  # the structure is the input's
    S = int_matrix(rng, 6, 6, 0.5)  # size 1 means a scalar even where 1 == m would not tell
    assert np.array_equal(dense_of(csc_op("scale_rows", a=operand(S[:1]), d=[2.0])), 2.0 * S[:1])


def test_from_dense(csc_op):
    """Exact zeros are dropped; -0.0 compares equal to 0.0 (`v != 0.0` in CscFromDense) and is dropped
    as well; everything else, denormals included, is kept."""
    rng = np.random.RandomState(6)
    D = int_matrix(rng, 7, 5, 0.5)
    D[2, 1], D[3, 1], D[4, 3] = -0.0, 5e-324, -1e-300
    D[:, 4] = 0
    res = csc_op("from_dense", m=7, n=5, d=D.flatten(order="F"))
    kept = D != 0
    assert not kept[2, 1] and kept[3, 1]
    assert len(res[3]) == np.count_nonzero(kept)
    got = dense_of(res)
    assert np.array_equal(got, D) and not np.signbit(got[2, 1])
    same_bits(res, sp.csc_matrix(D))
    assert csc_op("from_dense", m=0, n=3, d=np.zeros(0))[:2] == (0, 3)


def blob_of(colptr, rowidx, val):
    return (np.asarray(colptr, dtype=np.int32).tobytes() + np.asarray(rowidx, dtype=np.int32).tobytes() +
            np.asarray(val, dtype=np.float64).tobytes())


def from_blob(csc_op, m, n, colptr, rowidx, val):
    return csc_op("from_blob", m=m, n=n, nnz=len(val), blob=blob_of(colptr, rowidx, val))


def test_from_blob(csc_op):
    rng = np.random.RandomState(7)
    A = int_matrix(rng, 9, 7, 0.5)
    A[:, 3] = 0
    m, n, colptr, rowidx, val = operand(A)
    res = from_blob(csc_op, m, n, colptr, rowidx, val)  # sorted: returned as it is
    for got, exp in zip(res, (m, n, colptr, rowidx, val)):
        assert np.array_equal(got, exp)
    # one column with its indices reversed
    j = int(np.argmax(np.diff(colptr)))
    sl = slice(colptr[j], colptr[j + 1])
    r2, v2 = rowidx.copy(), val.copy()
    r2[sl], v2[sl] = rowidx[sl][::-1], val[sl][::-1]
    same_bits(check_invariants(from_blob(csc_op, m, n, colptr, r2, v2)), sp.csc_matrix(A))
    # one duplicated index: the values are summed
    assert colptr[-1] > colptr[-2]
    r3, v3 = np.append(rowidx, rowidx[-1]), np.append(val, 5.0)
    c3 = colptr.copy()
    c3[-1] += 1
    want = A.copy()
    want[rowidx[-1], n - 1] += 5.0
    res = from_blob(csc_op, m, n, c3, r3, v3)
    assert np.array_equal(dense_of(res), want) and len(res[3]) == len(rowidx)
    # duplicates in several columns, unsorted, some cancelling: every column shuffled and doubled
    cols = []
    for j in range(n):
        r, v = rowidx[colptr[j]:colptr[j + 1]], val[colptr[j]:colptr[j + 1]]
        extra = rng.randint(-3, 4, size=len(v)).astype(np.float64)
        extra[:1] = -v[:1]  # the first entry of the column cancels to an explicit zero
        p = rng.permutation(2 * len(r))
        cols.append((np.concatenate([r, r])[p], np.concatenate([v, extra])[p]))
    c4 = np.concatenate(([0], np.cumsum([len(r) for r, _ in cols])))
    res = from_blob(csc_op, m, n, c4, np.concatenate([r for r, _ in cols]), np.concatenate([v for _, v in cols]))
    want = np.zeros_like(A)
    for j, (r, v) in enumerate(cols):
        np.add.at(want[:, j], r, v)
    assert np.array_equal(dense_of(res), want)
    assert np.array_equal(res[2], colptr) and np.array_equal(res[3], rowidx)  # the structure of A, zeros explicit
    # rejected
    bad = rowidx.copy()
    bad[2] = m
    with pytest.raises(_solve.error, match="sparse blob: row index out of range"):
        from_blob(csc_op, m, n, colptr, bad, val)
    bad[2] = -1
    with pytest.raises(_solve.error, match="sparse blob: row index out of range"):
        from_blob(csc_op, m, n, colptr, bad, val)
    down = colptr.copy()
    down[2], down[3] = colptr[3] + 1, colptr[2]
    with pytest.raises(_solve.error, match="sparse blob: column pointers not monotone"):
        from_blob(csc_op, m, n, down, rowidx, val)
    past = colptr.copy()
    past[1] = len(val) + 3  # monotone up to here, but past the arrays
    with pytest.raises(_solve.error, match="sparse blob: column pointers not monotone"):
        from_blob(csc_op, m, n, past, rowidx, val)
    with pytest.raises(_solve.error, match="sparse blob: bad column pointers"):
        from_blob(csc_op, m, n, colptr + 1, rowidx, val)
    with pytest.raises(_solve.error, match="sparse blob 'blob' has %d bytes for 9 x 7 nnz=%d" % (
            len(blob_of(colptr, rowidx, val)) - 4, len(val))):
        csc_op("from_blob", m=m, n=n, nnz=len(val), blob=blob_of(colptr, rowidx, val)[:-4])


# ---- the threaded forms: from 2^20 entries -------------------------------------------------------------

BIG_NNZ = (1 << 20) + 3


def big_matrix(m, n, empty_leading):
    """m x n with BIG_NNZ entries, integer-valued, the first `empty_leading` columns empty (the first
    threads of CscFromBlob's validation, which deals out equal shares of the columns, get no entry at
    all; the first chunk of CscTranspose, which deals out equal shares of the entries, starts with all
    of them) and an empty row."""
    rng = np.random.RandomState(m)
    live = n - empty_leading
    per = BIG_NNZ // live
    lens = np.full(live, per)
    lens[:BIG_NNZ - per * live] += 1
    assert lens.max() <= m - 1 and lens.sum() == BIG_NNZ
    # column j: `lens[j]` distinct rows of 1..m-1 (row 0 stays empty): a random start, stride 1, wrapped
    start = rng.randint(0, m - 1, size=live)
    colptr = np.concatenate((np.zeros(empty_leading + 1, dtype=np.int64), np.cumsum(lens)))
    within = np.arange(BIG_NNZ) - np.repeat(colptr[empty_leading:-1], lens)
    rowidx = 1 + (np.repeat(start, lens) + within) % (m - 1)
    val = rng.randint(1, 100, size=BIG_NNZ).astype(np.float64)
    S = sp.csc_matrix((val, rowidx, colptr), shape=(m, n))
    S.sort_indices()
    assert S.nnz == BIG_NNZ
    return S


@pytest.mark.parametrize("m, n, empty_leading, note", [
    (2048, 1200, 300, "nt stays at the host thread count: nt m <= 16 * 2048 <= nnz / 4"),
    (100000, 2000, 700, "the halving loop: nt m <= nnz / 4 = 262144 leaves nt = 2"),
], ids=["2048rows", "100000rows"])
def test_threaded_transpose_and_blob_validation(csc_op, m, n, empty_leading, note):
    S = big_matrix(m, n, empty_leading)
    a = operand(S)
    same_bits(check_invariants(csc_op("transpose", a=a)), S.T)
    _, _, colptr, rowidx, val = a
    res = from_blob(csc_op, m, n, colptr, rowidx, val)  # sorted: the threaded validation, returned as it is
    for got, exp in zip(res, a):
        assert np.array_equal(got, exp)
    # one swapped pair at the very end: only the last thread's chunk sees it
    assert colptr[-1] - colptr[-2] >= 2
    r2, v2 = rowidx.copy(), val.copy()
    r2[-2:], v2[-2:] = rowidx[-2:][::-1], val[-2:][::-1]
    res = check_invariants(from_blob(csc_op, m, n, colptr, r2, v2))
    for got, exp in zip(res, a):
        assert np.array_equal(got, exp)
    # an index out of range in the middle
    r2[BIG_NNZ // 2] = m
    with pytest.raises(_solve.error, match="sparse blob: row index out of range"):
        from_blob(csc_op, m, n, colptr, r2, v2)
