"""The sparse layer on the device, launcher by launcher, through the test entry eps_test_sparse_op
(epsilon_amd._solve.sparse_op): SpmvCsr, SpmmCsrDense, DenseSpmmCsc and ScatterAddCsc of
csrc/kernels_sparse.hip; and sparse map handles (transposed, scaled, both) as operands of the
products and sums of csrc/linear_map.cc, through eps_test_sparse_handle_op and eps_linear_map_apply.

Every case is the smallest shape at which one branch of a launcher is entered; the tables below name
the branch per row, read from the launchers' conditions (256 threads per workgroup; SpMV:
avg = ceil(nnz / rows), LANES = 1, 2, 4, 8, 16, 32 for avg <= LANES, 64 above, 256 / LANES rows per
workgroup, the workgroup-per-row kernel from avg = 1024).  Every case asserts:

  * the result is inside the forward error bound (below) of the fp64 reference,
  * the guard elements on both sides of the output are untouched,
  * with beta == 0 (and for the products, which have no beta) the output, pre-filled with NaN, comes
    back finite (it is never read),
  * NaN in the padding rows of the dense operand leaves the result finite (they are never read),
  * a second identical call returns identical bits (fixed summation orders, no atomics).

Reference and bound.  Values and dense operands are rounded to the tested dtype first; the reference
is the fp64 product on the rounded inputs (scipy's CSR product, a sequential fp64 sum per entry).
alpha and beta are exact in f32.  Per output entry

    tol_i = gamma(k_i + 8) * (|alpha| (|S| |x|)_i + |beta| |y_i|),  gamma(q) = q u / (1 - q u),

u = 2^-24 (f32) / 2^-53 (f64), k_i the stored length of the row of S that entry sums over (the
column of the sparse factor for dense_spmm_csc): the standard forward bound, valid for any summation
order, with or without FMA; the + 8 covers the scaling and the beta term.  An empty row has the bound
|beta y_i| gamma(8), exactly 0 for beta == 0.  The scatter is elementwise, at most two roundings:
4 u (|w| + |alpha v|), against a reference in extended precision; entries no stored value addresses
must come back bit for bit.  No tolerance here is measured, none is widened by a factor;
tests/test_sparse_op_bound.py checks on the CPU that evaluations of every case in the tested
precision, in several summation orders, stay inside these bounds.
"""

import collections
import functools
import zlib

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

G = 8               # _solve.DENSE_OP_GUARD
SENTINEL = -777.25  # _solve.DENSE_OP_SENTINEL
U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
NP_DT = {"f32": np.float32, "f64": np.float64}

# name (the test id), op, the CSR operand (rows, cols, lens: stored entries per row), alpha, beta,
# n (columns of B / rows of A), pad (ld - rows of the dense operand), the branch the row enters
Case = collections.namedtuple("Case", "name op rows cols lens alpha beta n pad note")

AB4 = [(1.0, 0.0), (-0.75, 0.0), (1.25, 0.5), (-1.0, 1.0)]
AB2 = [AB4[0], AB4[2]]


def case(name, op, lens, cols, ab=(1.0, 0.0), n=0, pad=0, note=""):
    lens = tuple(int(v) for v in lens)
    assert all(0 <= v <= cols for v in lens)
    name = "%s-%s-a%g-b%g" % (op, name, ab[0], ab[1])
    return Case(name, op, len(lens), cols, lens, float(ab[0]), float(ab[1]), n, pad, note)


def avg_of(lens):
    """ceil(nnz / rows), the figure Spmv picks its kernel from."""
    return -(-sum(lens) // len(lens))


def lanes_of(lens):
    """The kernel Spmv launches: LANES, or 256 for the workgroup-per-row kernel."""
    avg = avg_of(lens)
    if avg >= 1024:
        return 256
    for lanes in (1, 2, 4, 8, 16, 32):
        if avg <= lanes:
            return lanes
    return 64


def edge_lens(rows, avg):
    """rows >= 5 row lengths with nnz == rows * avg exactly (so ceil(nnz / rows) == avg, the upper
    end of what gives this avg): row 0 holds 2 avg + 1 entries (longer than any LANES chosen for avg,
    not a multiple of it: the stride loop runs up to three times, unevenly across the lanes), row 1 is
    empty, rows 2, 3 and 4 hold avg - 1, avg + 1 and avg - 1, the others avg."""
    assert rows >= 5 and avg >= 1
    lens = [avg] * rows
    lens[0], lens[1], lens[2], lens[3], lens[4] = 2 * avg + 1, 0, avg - 1, avg + 1, avg - 1
    assert sum(lens) == rows * avg and min(lens) >= 0
    return lens


# ---- SpMV -------------------------------------------------------------------------------------------
def spmv_cases():
    out = []

    def add(name, lens, expect, note, abs_=AB2):
        lens = list(lens)
        assert lanes_of(lens) == expect, (name, avg_of(lens), lanes_of(lens), expect)
        cols = max(max(lens), 1) + 5  # every row's column indices are distinct; never a round number
        for ab in abs_:
            out.append(case(name, "spmv", lens, cols, ab=ab, note=note))

    for lanes in (1, 2, 4, 8, 16, 32):
        add("L%d-edge" % lanes, edge_lens(256 // lanes + 1, lanes), lanes,
            "avg = %d, the largest with LANES = %d; %d rows per workgroup, rows = %d: the second workgroup has one "
            "live row group; row 0 has %d entries (3 stride passes, the last with one lane), row 1 none"
            % (lanes, lanes, 256 // lanes, 256 // lanes + 1, 2 * lanes + 1),
            abs_=AB4 if lanes in (1, 16) else AB2)
        nxt = 2 * lanes
        add("L%d-above" % lanes, edge_lens(256 // lanes + 1, lanes + 1), nxt,
            "avg = %d, one above the edge of LANES = %d: LANES = %d, %d rows per workgroup, %d workgroups, the last "
            "with one live row group" % (lanes + 1, lanes, nxt, 256 // nxt, -(-(256 // lanes + 1) // (256 // nxt))))
    add("L64-edge", edge_lens(5, 1023), 64,
        "avg = 1023, the largest with LANES = 64 (one below the workgroup-per-row kernel); 4 rows per workgroup, "
        "rows = 5: the second workgroup has one live wave; row 1 empty")
    add("L64-above", edge_lens(5, 1024), 256,
        "avg = 1024: the workgroup-per-row kernel, 5 workgroups, one on an empty row")
    for lanes, ln in ((1, 1), (2, 2), (4, 3), (8, 7), (16, 13), (32, 29), (64, 100)):
        add("L%d-1row" % lanes, [ln], lanes,
            "rows = 1 with %d entries: LANES = %d, one live row group in the only workgroup%s"
            % (ln, lanes, "; two stride passes, the second with 36 lanes" if lanes == 64 else ""))
    add("skew-one-long-row", [0] * 1500 + [3000] + [0] * 1500, 1,
        "avg = 1 with one row of 3000 entries among 3000 empty ones: LANES = 1, one lane walks the long row; "
        "12 workgroups, the last with 185 live rows")
    add("skew-half-empty", [0, 75, 0, 90, 0, 64, 0, 101, 0, 70], 64,
        "avg = 40 > 32 with every other row empty: LANES = 64, 4 rows per workgroup, 3 workgroups, the last with two "
        "live waves")
    add("nnz0", [0] * 5, 1, "nnz == 0 with rows > 0: avg = 0, LANES = 1; y = beta y, zeros over NaN for beta == 0")
    add("block-2rows-2047", [1500, 547], 256,
        "rows = 2, nnz = 2047: avg = 1024 enters the workgroup-per-row kernel; 5 full passes of 256 and a tail of "
        "220 / 2 passes and a tail of 35", abs_=AB4)
    add("L64-2rows-2046", [1500, 546], 64,
        "rows = 2, nnz = 2046: avg = 1023 stays on LANES = 64, one workgroup with two live waves")
    add("block-3rows-middle-empty", [200, 0, 2900], 256,
        "workgroup-per-row kernel, avg = 1034: a row shorter than 256 (56 idle lanes), an empty row, a row of "
        "11 * 256 + 84 entries")
    return out


SPMV_CASES = spmv_cases()


# ---- SpmmCsrDense: thread per row of S, blockIdx.x = block of 256 rows, blockIdx.y = column of B (slabs of
# 65535 columns per launch); C has the column stride rows.
def row_pattern(rows, cols):
    """Row lengths that differ, every seventh row empty; a single row is not empty."""
    if rows == 1:
        return [min(5, cols)]
    return [(3 * i + 2) % 7 if i % 7 else 0 for i in range(rows)]


SPMM_ROWS = [(1, "one thread of one workgroup live: the i >= rows tail takes 255"),
             (256, "one full workgroup, no tail"),
             (257, "grid.x = 2: a second row block with one live thread")]
SPMM_CASES = [case("%dx23-N%d-ld+%d" % (rows, n, pad), "spmm_csr_dense", row_pattern(rows, 23), 23, ab=(alpha, 0.0),
                   n=n, pad=pad, note="%s; grid.y = %d; ldb = cols%s; rows of %s entries" % (
                       note, n, " + 3, NaN in the padding rows of B" if pad else "", "0..6" if rows > 1 else "5"))
              for rows, note in SPMM_ROWS for n in (1, 3) for pad in (0, 3) for alpha in (1.0, -0.75)]

# ---- DenseSpmmCsc: thread per row of A, blockIdx.x = block of 256 rows of A, blockIdx.y = column of the
# sparse factor F (= row of the CSR operand; slabs of 65535 per launch); C has the column stride M.
DSPMM_LENS = [3, 0, 40, 1, 5, 2, 7]  # the columns of F: an empty one, one with 40 of the 45 rows
DSPMM_CASES = [case("M%d-45x7-ld+%d" % (m, pad), "dense_spmm_csc", DSPMM_LENS, 45, ab=(alpha, 0.0), n=m, pad=pad,
                    note="%s; grid.y = 7 columns of 3, 0, 40, 1, 5, 2, 7 entries; lda = M%s" % (
                        note.replace("rows", "M"), " + 3, NaN in the padding rows of A" if pad else ""))
               for m, note in SPMM_ROWS for pad in (0, 3) for alpha in (1.0, -0.75)]

# ---- ScatterAddCsc: one wave per column of F (= row of the CSR operand), 4 columns per workgroup, the 64 lanes
# stride over the column's entries; nnz == 0 returns before any launch.  W is ld x columns with ld = 137.
SCATTER_LD = 137
SCATTER_COLS = [
    ("c1-n1", [1], "one column of one entry: one lane of wave 0, waves 1..3 leave at j >= cols"),
    ("c1-n130", [130], "one column of 130 entries: three stride passes, the last with 2 lanes"),
    ("c4", [130, 0, 65, 64], "4 columns: one full workgroup; 130 (three passes), an empty column, 65 (a second "
                             "pass with one lane), 64 (exactly one pass)"),
    ("c5", [0, 1, 64, 65, 130], "5 columns: a second workgroup with one live wave (its column has 130 entries)"),
    ("c5-nnz0", [0] * 5, "nnz == 0: no launch, W and the guards keep their bits"),
]
SCATTER_CASES = [case(name, "scatter_add_csc", lens, SCATTER_LD, ab=(alpha, 0.0), note=note)
                 for name, lens, note in SCATTER_COLS for alpha in (1.0, -0.75)]

# ---- more than 65535 values of blockIdx.y: a second slab of one column
LIMIT_CASES = [
    case("M1-3x65536", "dense_spmm_csc", [(i + 1) % 3 for i in range(65536)], 3, ab=(-0.75, 0.0), n=1,
         note="M = 1 and 65536 sparse columns: two launches, grid.y = 65535 and 1, colptr and C advanced"),
    case("1x3-N65536", "spmm_csr_dense", [2], 3, ab=(-0.75, 0.0), n=65536,
         note="one sparse row, N = 65536: two launches, grid.y = 65535 and 1, B and C advanced"),
]

ALL_CASES = SPMV_CASES + SPMM_CASES + DSPMM_CASES + SCATTER_CASES + LIMIT_CASES


# ---- data, reference and bound ---------------------------------------------------------------------

def gamma(q, u):
    return q * u / (1.0 - q * u)


def seed_of(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def csr_structure(rng, lens, cols):
    """ptr and idx of a CSR matrix with the given row lengths: distinct, ascending columns per row."""
    ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    idx = np.concatenate([np.sort(rng.choice(cols, size=k, replace=False)) for k in lens] +
                         [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    return ptr, idx


@functools.lru_cache(maxsize=None)
def make_data(c, dtype):
    """The operands of case c, seeded by its name, rounded to the tested dtype (held as float64).
    Computed once per (case, dtype); nobody changes them."""
    rng = np.random.RandomState(seed_of(c.name))

    def randn(*shape):
        return rng.randn(*shape).astype(NP_DT[dtype]).astype(np.float64)

    d = {}
    d["ptr"], d["idx"] = csr_structure(rng, c.lens, c.cols)
    d["val"] = randn(int(d["ptr"][-1]))
    if c.op == "spmv":
        d["x"], d["y"] = randn(c.cols), randn(c.rows)
    elif c.op == "spmm_csr_dense":
        d["B"] = randn(c.cols, c.n)
    elif c.op == "dense_spmm_csc":
        d["A"] = randn(c.n, c.cols)
    elif c.op == "scatter_add_csc":
        w = randn(c.cols, c.rows)
        d["W"] = np.where(w == 0, 1.0, w)  # pre-filled with non-zero values
    else:
        raise ValueError(c.op)
    for v in d.values():
        v.setflags(write=False)
    return d


def contraction(c, d):
    """(S, X): the case's sums are the rows of S X - S the CSR operand as a scipy matrix, X dense with
    S.cols rows.  The device output is (S X) column-major, except for dense_spmm_csc: C = A F = (S A^T)^T."""
    S = sp.csr_matrix((d["val"], d["idx"], d["ptr"]), shape=(c.rows, c.cols))
    if c.op == "spmv":
        return S, d["x"].reshape(-1, 1)
    if c.op == "spmm_csr_dense":
        return S, d["B"]
    return S, d["A"].T


def device_layout(c, R):
    """The rows x N array R = S X as the flat output of the launcher."""
    return R.reshape(-1) if c.op == "dense_spmm_csc" else R.flatten(order="F")


@functools.lru_cache(maxsize=None)
def reference(c, dtype):
    """(reference, tolerance) per entry of the flat output."""
    d = make_data(c, dtype)
    if c.op == "scatter_add_csc":
        ext = np.longdouble
        add = np.zeros((c.cols, c.rows), dtype=ext)
        row_of = np.repeat(np.arange(c.rows), c.lens)
        add[d["idx"], row_of] = ext(c.alpha) * d["val"].astype(ext)
        ref = d["W"].astype(ext) + add
        tol = 4 * U[dtype] * (np.abs(d["W"]) + np.abs(add).astype(np.float64))
        return ref.flatten(order="F"), tol.flatten(order="F")
    S, X = contraction(c, d)
    R = np.asarray(S.dot(X))
    mag = np.asarray(abs(S).dot(np.abs(X)))
    k = np.asarray(c.lens, dtype=np.float64).reshape(-1, 1)
    ref = c.alpha * R
    bound = abs(c.alpha) * mag
    if c.beta != 0:
        ref = ref + c.beta * d["y"].reshape(-1, 1)
        bound = bound + abs(c.beta) * np.abs(d["y"]).reshape(-1, 1)
    tol = gamma(k + 8, U[dtype]) * bound
    return device_layout(c, ref), device_layout(c, tol)


def device_operands(c, d):
    """The keyword arguments of sparse_op for case c: the operands as the device gets them - NaN in
    everything the launcher must not read (y under beta == 0, the output of the products, the padding
    rows of the dense operand)."""
    kw = dict(rows=c.rows, cols=c.cols, ptr=d["ptr"], idx=d["idx"], val=d["val"], alpha=c.alpha, beta=c.beta)
    if c.op == "spmv":
        kw["d"] = d["x"]
        kw["y"] = np.full(c.rows, np.nan) if c.beta == 0 else d["y"]
    elif c.op == "scatter_add_csc":
        kw["y"] = d["W"].flatten(order="F")
    else:
        D = d["B"] if c.op == "spmm_csr_dense" else d["A"]
        held, count = D.shape
        ld = held + c.pad
        P = np.full((ld, count), np.nan)
        P[:held] = D
        kw["d"] = P.flatten(order="F")[:max((count - 1) * ld + held, 0)]
        kw["ld"], kw["n"] = ld, c.n
        kw["y"] = np.full(c.rows * c.n, np.nan)
    return kw


# ---- the checks -------------------------------------------------------------------------------------

@pytest.fixture(params=["f64", "f32"])
def dtype(request, solve_mod):
    solve_mod.set_option("dtype", request.param)
    yield request.param
    solve_mod.set_option("dtype", "f32")


def split_guards(name, out):
    assert out.shape == (len(out),) and len(out) >= 2 * G
    lo, body, hi = out[:G], out[G:len(out) - G], out[len(out) - G:]
    assert np.array_equal(lo, np.full(G, SENTINEL)), "%s: store below the output: %r" % (name, lo)
    assert np.array_equal(hi, np.full(G, SENTINEL)), "%s: store past the output: %r" % (name, hi)
    return body


def check_inside(name, note, got, ref, tol):
    got = np.asarray(got).reshape(-1)
    ref, tol = np.asarray(ref).reshape(-1), np.asarray(tol).reshape(-1)
    assert got.shape == ref.shape, "%s: %r values, the reference has %r" % (name, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), "%s (%s): %d entries not finite (something that must not be read was)" % (
        name, note, np.count_nonzero(~np.isfinite(got)))
    err = np.abs(got - ref).astype(np.float64)
    bad = np.nonzero(err > tol)[0]
    assert bad.size == 0, "%s (%s): %d entries outside the bound, first at %d: got %r, reference %r, bound %r" % (
        name, note, bad.size, bad[0], got[bad[0]], ref[bad[0]], tol[bad[0]])


def run_case(solve_mod, c, dtype):
    d = make_data(c, dtype)
    ref, tol = reference(c, dtype)
    kw = device_operands(c, d)
    first = solve_mod.sparse_op(c.op, **kw)
    again = solve_mod.sparse_op(c.op, **kw)
    got = split_guards(c.name, first)
    check_inside(c.name, c.note, got, ref, tol)
    assert np.array_equal(first, again), "%s (%s): two runs differ in %d entries" % (
        c.name, c.note, np.count_nonzero(first != again))
    return got


def params(cases):
    return pytest.mark.parametrize("c", cases, ids=[c.name for c in cases])


def test_tables_name_their_branches():
    """Every row has a note, unique ids, and the SpMV rows cover every kernel at both ends."""
    assert all(c.note for c in ALL_CASES)
    assert len({c.name for c in ALL_CASES}) == len(ALL_CASES)
    assert {lanes_of(c.lens) for c in SPMV_CASES} == {1, 2, 4, 8, 16, 32, 64, 256}
    assert {avg_of(c.lens) for c in SPMV_CASES} >= {0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 1023, 1024}


@params(SPMV_CASES)
def test_spmv(solve_mod, dtype, c):
    got = run_case(solve_mod, c, dtype)
    if sum(c.lens) == 0:  # y = beta y, and beta = 0.5 scales without rounding
        assert np.array_equal(got, c.beta * make_data(c, dtype)["y"])


@params(SPMM_CASES)
def test_spmm_csr_dense(solve_mod, dtype, c):
    run_case(solve_mod, c, dtype)


@params(DSPMM_CASES)
def test_dense_spmm_csc(solve_mod, dtype, c):
    run_case(solve_mod, c, dtype)


@params(SCATTER_CASES)
def test_scatter_add_csc(solve_mod, dtype, c):
    got = run_case(solve_mod, c, dtype)
    d = make_data(c, dtype)
    untouched = np.ones((c.cols, c.rows), dtype=bool)
    untouched[d["idx"], np.repeat(np.arange(c.rows), c.lens)] = False
    w = d["W"].flatten(order="F")
    keep = untouched.flatten(order="F")
    assert np.array_equal(got[keep], w[keep]), "%s: entries that no stored value addresses changed" % c.name
    if sum(c.lens) == 0:
        assert np.array_equal(got, w)


@params(LIMIT_CASES)
def test_more_columns_than_one_launch_takes(solve_mod, dtype, c):
    run_case(solve_mod, c, dtype)


# ---- map level: a sparse handle that is transposed, scaled or both, as an operand ---------------------

MAP_M, MAP_N = 300, 270  # more than one row block of 256 in either direction
SCALE = -0.75
HANDLES = [("plain", False, None), ("transposed", True, None), ("scaled", False, SCALE),
           ("scaled-transposed", True, SCALE)]


@functools.lru_cache(maxsize=None)
def map_data(dtype):
    """S (300 x 270, about 4 % filled, with empty rows and columns), dense operands for both sides of
    either orientation, vectors; all rounded to the tested dtype."""
    rng = np.random.RandomState(20)
    T = NP_DT[dtype]
    stored = rng.rand(MAP_M, MAP_N) < 0.04
    stored[:, 7] = False
    stored[11, :] = False
    S = sp.csc_matrix(np.where(stored, rng.randn(MAP_M, MAP_N).astype(T).astype(np.float64), 0.0))
    S.sort_indices()
    dense = {shape: rng.randn(*shape).astype(T).astype(np.float64)
             for shape in [(MAP_N, 5), (MAP_M, 5), (3, MAP_M), (3, MAP_N), (MAP_M, MAP_N), (MAP_N, MAP_M)]}
    vec = {n: rng.randn(n).astype(T).astype(np.float64) for n in (MAP_M, MAP_N)}
    return S, dense, vec


def handle_matrix(S, transpose, scale):
    """(H0, s): the handle is s H0, H0 = S or S^T in CSR form."""
    H0 = sp.csr_matrix(S.T if transpose else S)
    H0.sort_indices()
    return H0, 1.0 if scale is None else scale


def product_bound(H0, s, D, dtype, left):
    """Reference and bound of s H0 D (left) or D (s H0): k is the row (column) length of H0."""
    if left:
        ref, mag = H0.dot(D), abs(H0).dot(np.abs(D))
        k = np.diff(H0.indptr).reshape(-1, 1)
    else:
        ref, mag = H0.T.dot(D.T).T, abs(H0).T.dot(np.abs(D).T).T
        k = np.diff(sp.csc_matrix(H0).indptr).reshape(1, -1)
    return s * np.asarray(ref), gamma(k + 8.0, U[dtype]) * abs(s) * np.asarray(mag)


@pytest.mark.parametrize("handle", HANDLES, ids=[h[0] for h in HANDLES])
def test_sparse_handle_products_and_sums(solve_mod, dtype, handle):
    """Sparse x Dense (SpmmCsrDense on csr()), Dense x Sparse (DenseSpmmCsc on csr_of_transpose()) and
    Sparse + Dense in both orders (ScatterAddCsc on csr_of_transpose()): the factor of a scaled handle
    is in the result exactly once, a transposed handle takes the other CSR copy."""
    from epsilon_amd import ir
    name, transpose, scale = handle
    S, dense, _ = map_data(dtype)
    A = ir.sparse_matrix(S)
    H0, s = handle_matrix(S, transpose, scale)
    hm, hn = H0.shape
    D = dense[(hn, 5)]
    got = solve_mod.sparse_handle_op("sparse_dense", A, D, transpose=transpose, scale=scale)
    check_inside(name + " x dense", "", got.flatten(order="F"), *[v.flatten(order="F") for v in product_bound(
        H0, s, D, dtype, True)])
    D = dense[(3, hm)]
    got = solve_mod.sparse_handle_op("dense_sparse", A, D, transpose=transpose, scale=scale)
    check_inside("dense x " + name, "", got.flatten(order="F"), *[v.flatten(order="F") for v in product_bound(
        H0, s, D, dtype, False)])
    D = dense[(hm, hn)]
    ext = np.longdouble
    add = ext(s) * np.asarray(H0.todense()).astype(ext)
    ref = D.astype(ext) + add
    tol = 4 * U[dtype] * (np.abs(D) + np.abs(add).astype(np.float64))
    stored = np.asarray(abs(H0).todense()) != 0
    for op in ("sparse_plus_dense", "dense_plus_sparse"):
        got = solve_mod.sparse_handle_op(op, A, D, transpose=transpose, scale=scale)
        check_inside(op + " " + name, "", got.flatten(order="F"), ref.flatten(order="F"), tol.flatten(order="F"))
        assert np.array_equal(got[~stored], D[~stored]), "%s %s: entries outside the structure changed" % (op, name)


def spmv_bound(H0, s, x, dtype):
    k = np.diff(H0.indptr)
    return s * H0.dot(x), gamma(k + 8.0, U[dtype]) * abs(s) * abs(H0).dot(np.abs(x))


@pytest.mark.parametrize("handle", HANDLES, ids=[h[0] for h in HANDLES])
def test_sparse_handle_apply_and_adjoint(solve_mod, dtype, handle):
    """Apply and adjoint of every handle; and with the map as built applied FIRST, so that the core
    holds the CSR copy of the plain direction before the handle asks for its own: both cached copies
    serve the right direction."""
    from epsilon_amd import ir
    name, transpose, scale = handle
    S, _, vec = map_data(dtype)
    A = ir.sparse_matrix(S)
    H0, s = handle_matrix(S, transpose, scale)
    hm, hn = H0.shape
    Ht = sp.csr_matrix(H0.T)
    Ht.sort_indices()
    plain_ref, plain_tol = spmv_bound(sp.csr_matrix(S), 1.0, vec[MAP_N], dtype)
    for p in (None, vec[MAP_N]):
        for op, M, x in (("apply", H0, vec[hn]), ("adjoint", Ht, vec[hm])):
            got = solve_mod.sparse_handle_op(op, A, x, transpose=transpose, scale=scale, p=p)
            if p is not None:
                got, plain = got
                check_inside("plain first, then %s of %s" % (op, name), "", plain, plain_ref, plain_tol)
            check_inside("%s of %s" % (op, name), "plain first" if p is not None else "", got,
                         *spmv_bound(M, s, x, dtype))


def test_unsorted_blob_applies_like_its_canonical_form(solve_mod, dtype):
    """A sparse map built from a wire blob with a reversed column and a duplicated entry (CscFromBlob's
    sort-and-combine path) applies, in both directions, like the sorted matrix with the duplicate
    summed: inside the bound of the canonical structure, and with the canonical map's bits."""
    from epsilon_amd import ir
    from epsilon_amd.wire import Constant, LinearMap
    S, _, vec = map_data(dtype)
    T = NP_DT[dtype]
    colptr, rowidx, val = S.indptr.astype(np.int32), S.indices.astype(np.int32).copy(), S.data.copy()
    lens = np.diff(colptr)
    j = int(np.argmax(lens))  # the longest column, reversed
    assert lens[j] >= 3
    sl = slice(colptr[j], colptr[j + 1])
    rowidx[sl], val[sl] = rowidx[sl][::-1].copy(), val[sl][::-1].copy()
    # one more entry at the end of the last non-empty column, on the row of its first entry
    jd = int(np.nonzero(lens)[0][-1])
    extra = 0.5
    rowidx = np.insert(rowidx, colptr[jd + 1], rowidx[colptr[jd]])
    val = np.insert(val, colptr[jd + 1], extra)
    colptr = colptr.copy()
    colptr[jd + 1:] += 1
    blob = colptr.tobytes() + rowidx.astype(np.int32).tobytes() + val.tobytes()
    c = Constant(constant_type=Constant.SPARSE_MATRIX, m=MAP_M, n=MAP_N, nnz=len(val), data_location="/mem/unsorted")
    raw = ir.LMap(LinearMap(linear_map_type=LinearMap.SPARSE_MATRIX, m=MAP_M, n=MAP_N, constant=c),
                  {"/mem/unsorted": blob})
    canon = sp.csc_matrix(S)
    canon[rowidx[colptr[jd]], jd] += extra  # summed in fp64 on the host, rounded at the upload
    canon.data = canon.data.astype(T).astype(np.float64)
    canon.sort_indices()
    canonical = ir.sparse_matrix(canon)
    for transpose, x in ((False, vec[MAP_N]), (True, vec[MAP_M])):
        got = solve_mod.linear_map_apply(raw, x, transpose=transpose)
        H0 = sp.csr_matrix(canon.T if transpose else canon)
        check_inside("unsorted blob, transpose=%r" % transpose, "", got, *spmv_bound(H0, 1.0, x, dtype))
        assert np.array_equal(got, solve_mod.linear_map_apply(canonical, x, transpose=transpose))
