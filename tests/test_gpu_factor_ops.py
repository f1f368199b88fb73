"""The dense factor layer on the device, launcher by launcher, through the test entry
eps_test_factor_op (epsilon_amd._solve.factor_op): SpdInverseInPlace and SpdInverseColumns of
csrc/kernels_factor.hip - the blocked Cholesky, X = L^-1 by recursive doubling, the X^T X product and
the slab solve behind every cached explicit inverse.

Kernels and the condition that enters each (NB = 64, outer panel OB = 256, BS = 512):

  PotrfFusedStepKernel     f32 with form 0 (the default without the potrf_two_kernels option): one
                           launch per 64-column step, ceil(rem / 64) workgroups - ONE dead workgroup
                           when rem = n - (k0 + kb) is 0, which still factors the diagonal block.
                           Every workgroup re-derives the factor of the diagonal block; workgroup 0
                           writes it to a side buffer, scattered into W after the last step.
  PotrfDiagStepKernel<T>   f64 always, f32 with form 1: the diagonal block of a step - the update
                           with the K0..k0 columns of the outer panel (none in the panel's first
                           step), then CholRows in one wave; kb < 64 is padded with the identity.
  PotrfPanelStepKernel<T>  the same forms, launched only when rows lie below the block: the same
                           update, then forward substitution against the new block.
  Gemm, lower_only         the rank-KB update of the trailing matrix after each outer panel that has
                           rows below it (n > 256).
  ScatterDiagBlocksKernel  the fused form's side buffer into W; the 64 x 64 inverses into X.
  TrtriDiagBlocksKernel<T> always: the inverse of every diagonal block, ragged last one included.
  DoublingInverse          levels sz = 64, 128, ... < cap (cap = n, or 512 for the slab solve): the
                           n / (2 sz) full pairs of a level in two GemmBatched launches, a ragged
                           last pair (s2 = min(sz, n - r0 - sz) rows) in two Gemm calls, a lone last
                           block left as it is.
  X^T X                    Gemm(T, N, lower_only) per 1024-row block of X (two blocks from n = 1025),
                           then SymmetrizeFromLower.
  SpdInverseColumns        Fill + AddDiag place the unit columns; forward over the 512-blocks from
                           lo / 512, backward over all of them, two Gemm calls (MultiGemv at cnt <= 16
                           on aligned f32 operands) and a 2-D copy per block.

Sizes (SIZE_ROWS; every row runs in f32 with forms 0 and 1 and in f64 with form -1, kappa = 1e2):

  n = 1, 2, 63, 64, 65       one block: ragged kb; a one-row panel; the fused step's dead workgroup
  n = 128, 129, 192, 193     doubling: a full pair; a full pair plus a lone block; a ragged pair, s2 = 1
  n = 255, 256, 257, 320, 321  one outer panel exactly; a trailing update of 1 row, 64 rows, 65 rows
  n = 512, 513, 577          the 512-block edge of SpdInverseColumns; a last block of 1 row, of 65 rows
  n = 1026, 1090             four outer panels plus a ragged one; two X^T X row blocks; odd and even
                             block counts; an even ld for the f64 pipe kernel
  n = 321, 577 at kappa = 1e4 (both dtypes) and 1e8 (f64 only)

Column slabs (SLAB_ROWS: n, lo, cnt; each with out_cols = cnt and cnt + 3, kappa = 1e2):

  (65, 0, 65), (65, 64, 1)   every column; the last column alone, in the one-row block
  (300, 0, 0)                cnt == 0: the pure-Cholesky entry, nothing written
  (577, 0, 16), (577, 0, 17) either side of the MultiGemv width
  (577, 500, 77)             lo inside block 0, the slab crossing row 512
  (577, 512, 65)             the forward loop starts at block 1
  (577, 576, 1)              the last column alone
  (1090, 1030, 17)           the forward loop starts at block 2
  (1090, 0, 1090)            every column of three 512-blocks

Each row's `note` names the branch it is the smallest shape for.  The routes that start at n >= 2048 -
the split-f16 X^T X (SyrkSplitF16LowerTriangular), GemmSplitF16KRange, nsplit > 1 and the unbatched
doubling levels from 4096 - stay with tests/test_gpu_parity.py (n = 4200) and
tests/test_gpu_under_load.py.

Inputs.  A = D Q diag(ev) Q^T D: Q orthogonal from a seeded QR, ev geometric from 1 to kappa,
D = diag(exp(U(-2, 2))) so that rows of small scale are not masked by large ones; symmetrised, then
rounded to f32 in BOTH dtypes, so both see the same exactly symmetric, exactly representable matrix.

What every case asserts, with u = 2^-24 / 2^-53 and gamma(q) = q u / (1 - q u); every product below is
evaluated in fp64 from the returned values:

  (a) the factor: L^ is the lower triangle of the columns op's out2 with cnt = 0; on i >= j
      |L^ L^T - A| <= gamma(n + 8) (|L^| |L^|^T) - the componentwise backward bound of Cholesky
      (Higham, Accuracy and Stability of Numerical Algorithms, Thm 10.3, gamma_{n+1}), which holds for
      any order of the subtractions and so for the 64 / 256 blocking; + 8 is the project's slack
      convention.
  (b) the triangular inverse: X^ (spd_inverse's out2) is exactly zero strictly above the diagonal,
      and |X^ L^ - I| <= gamma(n + 8) (|X^| |L^|) per entry.  A theorem for the substitution forms,
      not for the recursive doubling: a condition on the inputs, which tests/test_factor_op_bound.py
      checks with a numpy emulation of the doubling on every row.
  (c) the product: on i >= j |W^ - X^T X^| <= gamma(n + 8) (|X^|^T |X^|), the forward bound of a sum
      of n products with the returned X^ as operand; and W^ is bitwise symmetric.
  (d) end to end, for W^ and for the slab: max_ij |W^ - inv64(A)|_ij / sqrt(inv_ii inv_jj) <=
      M_SPREAD x the largest value of the same statistic among the CPU evaluations of that case in
      the tested dtype (cpu_evaluations: LAPACK potrf + potri; potrf + trtri + X^T X; a numpy
      emulation of the kernels' own order; for a slab also potrs on the unit columns).  M_SPREAD is
      the largest ratio between two CPU evaluations over the whole table, a power of two: the
      kernels' summation order is one more sample of the spread that equally valid orders show among
      themselves.  It is measured among references only (tests/test_factor_op_bound.py asserts it).
      A statistic below STAT_FLOOR counts as STAT_FLOOR: at n = 1 the chain sqrt, reciprocal, square
      is (1 + d)^5 and inv64 is itself rounded, so an evaluation that happens to be exact sets no
      bound.
  (e) only the lower triangle is read: with the strict upper triangle of A replaced by NaN, and again
      by unrelated finite values, every output is bit-identical to the symmetric input's (of the
      columns op's out2 the lower triangle: the rest is scratch).
  (f) a second identical call returns identical bits, the factor included - which is what lets (b)
      pair X^ with L^; both guards are intact at a_off = 0 and 1; the padded columns cnt .. out_cols
      are bit-identical to what was placed; the lower triangle of the columns op's out2 equals the
      cnt = 0 factor.

Not positive definite (NOT_PD): every input raises the launcher's own message in both dtypes, both
forms and both ops (cnt = 0 included), and a valid n = 65 case afterwards still satisfies (a) to (d).

The largest matrix is 1090 x 1090; the CPU evaluations are cached per case and dtype.
"""

import collections
import functools
import zlib

import numpy as np
import pytest
from scipy.linalg import lapack

pytestmark = pytest.mark.gpu

G = 8               # _solve.DENSE_OP_GUARD
SENTINEL = -777.25  # _solve.DENSE_OP_SENTINEL
U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
NP_DT = {"f32": np.float32, "f64": np.float64}
BOTH = ("f32", "f64")
FORMS = {"f32": (0, 1), "f64": (-1,)}
NOT_PD_MSG = "dense inverse: matrix is not positive definite"
# (d): the spread among the CPU evaluations; asserted by tests/test_factor_op_bound.py
M_SPREAD = 4
# (d): five roundings of the n = 1 chain and the rounding of inv64 itself
STAT_FLOOR = {"f32": 5 * U["f32"] + U["f64"], "f64": 6 * U["f64"]}

# n, kappa, the dtypes it runs in, lo, cnt (None: a size row), the group of the table, the branch
Row = collections.namedtuple("Row", "n kappa dtypes lo cnt group note")


def size_row(n, group, note, kappa=1e2, dtypes=BOTH):
    return Row(n, kappa, dtypes, None, None, group, note)


SIZE_ROWS = [
    size_row(1, "one block", "kb = 1: one live row, 63 of identity padding; nothing below - the fused step's dead workgroup"),
    size_row(2, "one block", "kb = 2: the smallest block with an off-diagonal entry"),
    size_row(63, "one block", "kb = 63: ragged by one row"),
    size_row(64, "one block", "one whole 64-block, nothing below it"),
    size_row(65, "one block", "two steps: a one-row panel below the first, a last block of kb = 1; one ragged doubling pair"),
    size_row(128, "doubling", "one full pair at sz = 64: the two batched launches, no level above"),
    size_row(129, "doubling", "a full pair plus a lone one-row block at sz = 64; a ragged pair with s2 = 1 at sz = 128"),
    size_row(192, "doubling", "a full pair plus a lone whole block at sz = 64; a ragged pair with s2 = 64 at sz = 128"),
    size_row(193, "doubling", "a full pair and a ragged pair with s2 = 1 at sz = 64; s2 = 65 at sz = 128"),
    size_row(255, "outer panel", "one outer panel, ragged by one: four steps, the last with kb = 63, no trailing update"),
    size_row(256, "outer panel", "one outer panel exactly: no trailing update"),
    size_row(257, "outer panel", "a trailing rank-256 update of 1 row; a second outer panel of one row"),
    size_row(320, "outer panel", "a trailing update of 64 rows"),
    size_row(321, "outer panel", "a trailing update of 65 rows; the second panel has a step with a one-row panel below"),
    size_row(512, "512-block", "the 512-block edge of SpdInverseColumns: one block, the doubling to cap 512 is all of X"),
    size_row(513, "512-block", "a last 512-block of 1 row; two trailing updates, the second of 1 row"),
    size_row(577, "512-block", "a last 512-block of 65 rows"),
    size_row(1026, "four panels", "four outer panels plus one of 2 rows; a second X^T X row block of 2 rows; 17 blocks "
                                  "(odd); an even ld for the f64 pipe kernel"),
    size_row(1090, "four panels", "four outer panels plus one of 66 rows; a second X^T X row block of 66 rows; 18 blocks "
                                  "(even); an even ld"),
    size_row(321, "kappa", "kappa = 1e4: the bounds (a) to (c) scale with |L| and |X|, not with kappa", kappa=1e4),
    size_row(577, "kappa", "kappa = 1e4 across the 512-block edge", kappa=1e4),
    size_row(321, "kappa", "kappa = 1e8, f64 only", kappa=1e8, dtypes=("f64",)),
    size_row(577, "kappa", "kappa = 1e8 across the 512-block edge, f64 only", kappa=1e8, dtypes=("f64",)),
]

SLAB_ROWS = [Row(n, 1e2, BOTH, lo, cnt, "slab", note) for n, lo, cnt, note in [
    (65, 0, 65, "every column of a two-block matrix: one 512-block of 65 rows"),
    (65, 64, 1, "the last column alone: the unit entry sits in the one-row 64-block"),
    (300, 0, 0, "cnt == 0: the pure-Cholesky entry returns right after the factorisation"),
    (577, 0, 16, "cnt = 16: the widest MultiGemv product"),
    (577, 0, 17, "cnt = 17: one past the MultiGemv width"),
    (577, 500, 77, "lo inside block 0, the slab crossing row 512"),
    (577, 512, 65, "lo / 512 = 1: the forward loop skips block 0, whose rows of Y stay zero"),
    (577, 576, 1, "the last column alone"),
    (1090, 1030, 17, "lo / 512 = 2: the forward loop starts at the last, ragged block"),
    (1090, 0, 1090, "every column, three 512-blocks"),
]]
SLAB_PADS = (0, 3)  # out_cols - cnt

ALL_ROWS = SIZE_ROWS + SLAB_ROWS


def row_id(r):
    s = "n%d-kappa1e%d" % (r.n, int(round(np.log10(r.kappa))))
    return s if r.cnt is None else s + "-lo%d-cnt%d" % (r.lo, r.cnt)


# ---- inputs -----------------------------------------------------------------------------------------

def gamma(q, u):
    return q * u / (1.0 - q * u)


@functools.lru_cache(maxsize=None)
def _matrix(n, kappa):
    rng = np.random.RandomState(zlib.crc32(("factor-%d-%g" % (n, kappa)).encode()) & 0x7FFFFFFF)
    Q, _ = np.linalg.qr(rng.randn(n, n))
    ev = np.geomspace(1.0, kappa, n)
    D = np.exp(rng.uniform(-2.0, 2.0, n))
    A = (Q * ev).dot(Q.T)
    A = D[:, None] * A * D[None, :]
    A = 0.5 * (A + A.T)
    A = A.astype(np.float32).astype(np.float64)
    assert np.array_equal(A, A.T)
    A.setflags(write=False)
    return A


def make_matrix(r):
    """The matrix of a row (shared by the rows of one n and kappa; read-only)."""
    return _matrix(r.n, r.kappa)


def upper_replaced(A, what):
    """A with its strict upper triangle replaced by NaN or by unrelated f32-representable values."""
    n = A.shape[0]
    up = np.triu(np.ones((n, n), dtype=bool), 1)
    if what == "nan":
        return np.where(up, np.nan, A)
    rng = np.random.RandomState(n + 12345)
    junk = (1e3 * rng.randn(n, n)).astype(np.float32).astype(np.float64)
    return np.where(up, junk, A)


# ---- the CPU evaluations ----------------------------------------------------------------------------

class NotPositiveDefinite(Exception):
    pass


def _lapack(name, T):
    return getattr(lapack, ("s" if T == np.float32 else "d") + name)


def _potrf(A, T):
    c, info = _lapack("potrf", T)(np.asfortranarray(A.astype(T)), lower=1, clean=1)
    if info != 0:
        raise NotPositiveDefinite("potrf: info = %d" % info)
    assert c.dtype == T
    return c


def eval_potri(A, T):
    """1. LAPACK potrf + potri."""
    c = _potrf(A, T)
    w, info = _lapack("potri", T)(c, lower=1)
    assert info == 0 and w.dtype == T
    return dict(L=c, X=None, W=np.tril(w) + np.tril(w, -1).T)


def eval_trtri(A, T):
    """2. LAPACK potrf + trtri, then X^T X in the dtype."""
    c = _potrf(A, T)
    x, info = _lapack("trtri", T)(c, lower=1)
    assert info == 0
    x = np.tril(x)
    w = x.T.dot(x)
    assert x.dtype == T and w.dtype == T
    return dict(L=c, X=x, W=w)


def eval_emulated(A, T, sign=-1.0):
    """3. The order of csrc/kernels_factor.hip in numpy, every operation in the dtype: 64-column
    left-looking steps inside 256-panels (the diagonal block right-looking, as CholRows; the rows
    below by forward substitution), a right-looking trailing update per panel, the 64-block inverses
    in trti2 order grown by X21 = -X22 (L21 X11), and X^T X."""
    NB, OB = 64, 256
    n = A.shape[0]
    W = np.tril(A).astype(T)
    for K0 in range(0, n, OB):
        KB = min(OB, n - K0)
        for k0 in range(K0, K0 + KB, NB):
            kb = min(NB, n - k0)
            P = W[k0:k0 + kb, K0:k0]
            D = np.tril(W[k0:k0 + kb, k0:k0 + kb] - P.dot(P.T))
            for j in range(kb):
                if not D[j, j] > 0:
                    raise NotPositiveDefinite("pivot %d" % (k0 + j))
                D[j, j] = np.sqrt(D[j, j])
                D[j + 1:, j] /= D[j, j]
                D[j + 1:, j + 1:] -= np.tril(np.outer(D[j + 1:, j], D[j + 1:, j]))
            W[k0:k0 + kb, k0:k0 + kb] = D
            if k0 + kb < n:
                Tm = W[k0 + kb:, k0:k0 + kb] - W[k0 + kb:, K0:k0].dot(P.T)
                for j in range(kb):
                    Tm[:, j] = (Tm[:, j] - Tm[:, :j].dot(D[j, :j])) / D[j, j]
                W[k0 + kb:, k0:k0 + kb] = Tm
        if K0 + KB < n:
            L21 = W[K0 + KB:, K0:K0 + KB]
            W[K0 + KB:, K0 + KB:] -= L21.dot(L21.T)
    L = np.tril(W)
    X = np.zeros((n, n), dtype=T)
    for k0 in range(0, n, NB):
        kb = min(NB, n - k0)
        Lb, Xb = L[k0:k0 + kb, k0:k0 + kb], np.zeros((kb, kb), dtype=T)
        for j in range(kb - 1, -1, -1):
            Xb[j, j] = T(1) / Lb[j, j]
            Xb[j + 1:, j] = -(Xb[j + 1:, j + 1:].dot(Lb[j + 1:, j])) * Xb[j, j]
        X[k0:k0 + kb, k0:k0 + kb] = Xb
    sz = NB
    while sz < n:
        for r0 in range(0, n, 2 * sz):
            if r0 + sz < n:
                s2 = min(sz, n - r0 - sz)
                a, b, c = r0, r0 + sz, r0 + sz + s2
                X[b:c, a:b] = T(sign) * X[b:c, b:c].dot(L[b:c, a:b].dot(X[a:b, a:b]))
        sz *= 2
    Wi = X.T.dot(X)
    assert L.dtype == T and X.dtype == T and Wi.dtype == T
    return dict(L=L, X=X, W=Wi)


def eval_potrs(A, T, lo, cnt):
    """4. (slabs) LAPACK potrf + potrs on the unit columns lo .. lo + cnt."""
    c = _potrf(A, T)
    E = np.zeros((A.shape[0], cnt), dtype=T, order="F")
    E[lo + np.arange(cnt), np.arange(cnt)] = 1
    x, info = _lapack("potrs", T)(c, E, lower=1)
    assert info == 0 and x.dtype == T
    return dict(L=c, X=None, W=None, S=x)


EVALUATIONS = (("potrf + potri", eval_potri), ("potrf + trtri + X^T X", eval_trtri), ("emulated", eval_emulated))


def statistic(W, inv, lo=0):
    """(d): max_ij |W - inv|_ij / sqrt(inv_ii inv_jj) over the columns lo .. lo + W.shape[1] of inv."""
    if W.size == 0:
        return 0.0
    d = np.sqrt(np.diag(inv))
    cols = slice(lo, lo + W.shape[1])
    return float(np.max(np.abs(W - inv[:, cols]) / (d[:, None] * d[None, cols])))


@functools.lru_cache(maxsize=None)
def inv64(n, kappa):
    inv = np.linalg.inv(_matrix(n, kappa))
    inv = 0.5 * (inv + inv.T)
    inv.setflags(write=False)
    return inv


@functools.lru_cache(maxsize=None)
def cpu_evaluations(r, dtype):
    """The CPU evaluations of a row in the tested dtype: [(name, result as float64 arrays, its
    end-to-end statistic)], computed once per row and dtype.  A slab row's statistic is over its
    columns."""
    A, T, inv = make_matrix(r), NP_DT[dtype], inv64(r.n, r.kappa)
    out = []
    for name, fn in EVALUATIONS:
        e = {k: (None if v is None else v.astype(np.float64)) for k, v in fn(A, T).items()}
        W = e["W"] if r.cnt is None else e["W"][:, r.lo:r.lo + r.cnt]
        out.append((name, e, statistic(W, inv, r.lo or 0)))
    if r.cnt:  # (no right-hand side at cnt == 0)
        e = eval_potrs(A, T, r.lo, r.cnt)
        e = {k: (None if v is None else v.astype(np.float64)) for k, v in e.items()}
        out.append(("potrf + potrs", e, statistic(e["S"], inv, r.lo)))
    return out


def floored(stat, dtype):
    return max(stat, STAT_FLOOR[dtype])


def end_to_end_bound(r, dtype):
    return M_SPREAD * max(floored(s, dtype) for _, _, s in cpu_evaluations(r, dtype))


# ---- the checks -------------------------------------------------------------------------------------

def _ratio(err, bound, where):
    """The largest err / bound over `where`; an entry whose bound is 0 must have no error."""
    err, bound = err[where], bound[where]
    if err.size == 0:
        return 0.0
    assert np.all(np.isfinite(err)), "a value is not finite"
    zero = bound == 0
    if np.any(err[zero] != 0):
        return np.inf
    return float(np.max(err[~zero] / bound[~zero])) if np.any(~zero) else 0.0


def ratio_factor(L, A, dtype):
    """(a): the largest |L L^T - A| / (gamma(n + 8) |L| |L|^T) over i >= j."""
    n = A.shape[0]
    low = np.tril(np.ones((n, n), dtype=bool))
    return _ratio(np.abs(L.dot(L.T) - A), gamma(n + 8, U[dtype]) * np.abs(L).dot(np.abs(L).T), low)


def ratio_inverse(X, L, dtype):
    """(b): the largest |X L - I| / (gamma(n + 8) |X| |L|) over all entries."""
    n = L.shape[0]
    return _ratio(np.abs(X.dot(L) - np.eye(n)), gamma(n + 8, U[dtype]) * np.abs(X).dot(np.abs(L)),
                  np.ones((n, n), dtype=bool))


def ratio_product(W, X, dtype):
    """(c): the largest |W - X^T X| / (gamma(n + 8) |X|^T |X|) over i >= j."""
    n = X.shape[0]
    low = np.tril(np.ones((n, n), dtype=bool))
    return _ratio(np.abs(W - X.T.dot(X)), gamma(n + 8, U[dtype]) * np.abs(X).T.dot(np.abs(X)), low)


def same_bits(x, y):
    """Elementwise: equal, NaN counting as equal to NaN."""
    return (x == y) | (np.isnan(x) & np.isnan(y))


def assert_same(what, x, y):
    same = same_bits(x, y)
    assert np.all(same), "%s: %d entries differ, first at flat index %d" % (what, np.count_nonzero(~same), np.argmin(same))


def split_guards(what, out, n):
    assert out.shape == (n + 2 * G,), "%s: %d values returned, %d expected" % (what, out.size, n + 2 * G)
    lo, body, hi = out[:G], out[G:G + n], out[G + n:]
    assert np.array_equal(lo, np.full(G, SENTINEL)), "%s: store below the result: %r" % (what, lo)
    assert np.array_equal(hi, np.full(G, SENTINEL)), "%s: store past the result: %r" % (what, hi)
    return body


class Configured(object):
    """The dtype for one case, restored on the way out."""

    def __init__(self, solve_mod, dtype):
        self.s, self.dtype = solve_mod, dtype

    def __enter__(self):
        self.s.set_option("dtype", self.dtype)

    def __exit__(self, *exc):
        self.s.set_option("dtype", "f32")


def call_factor(solve_mod, what, A, form, a_off):
    """The cnt = 0 columns op: (the factor's lower triangle, the raw result)."""
    n = A.shape[0]
    out, w = solve_mod.factor_op("spd_inverse_columns", n=n, a=A.flatten(order="F"), a_off=a_off, form=form,
                                 lo=0, cnt=0, want_out2=True)
    split_guards(what + " factor", out, 0)
    return np.tril(w.reshape((n, n), order="F"))


def call_inverse(solve_mod, what, A, form, a_off):
    n = A.shape[0]
    out, x = solve_mod.factor_op("spd_inverse", n=n, a=A.flatten(order="F"), a_off=a_off, form=form, want_out2=True)
    W = split_guards(what + " inverse", out, n * n).reshape((n, n), order="F")
    return W, x.reshape((n, n), order="F")


def call_columns(solve_mod, what, A, form, a_off, lo, cnt, pad):
    """(the n x cnt slab, the lower triangle of W afterwards); guards and padded columns checked."""
    n = A.shape[0]
    out, w = solve_mod.factor_op("spd_inverse_columns", n=n, a=A.flatten(order="F"), a_off=a_off, form=form,
                                 lo=lo, cnt=cnt, out_cols=cnt + pad, want_out2=True)
    body = split_guards(what + " slab", out, n * (cnt + pad)).reshape((n, cnt + pad), order="F")
    assert np.array_equal(body[:, cnt:], np.full((n, pad), SENTINEL)), "%s: the padded columns changed" % what
    return body[:, :cnt], np.tril(w.reshape((n, n), order="F"))


def check_abcd(what, A, inv, L, X, W, dtype, bound_d):
    """(a) to (d) of one factor / inverse pair; every figure is printed before it is asserted."""
    n = A.shape[0]
    ra, rb, rc = ratio_factor(L, A, dtype), ratio_inverse(X, L, dtype), ratio_product(W, X, dtype)
    sd = statistic(W, inv)
    print("FIGURES %s: (a) %.3g (b) %.3g (c) %.3g of the bound; (d) %.3g against %.3g = %.3g of the bound" % (
        what, ra, rb, rc, sd, bound_d, sd / bound_d))
    assert ra <= 1.0, "%s (a): |L L^T - A| is %.3g x its bound" % (what, ra)
    assert np.array_equal(np.triu(X, 1), np.zeros((n, n))), "%s (b): X is not exactly zero above the diagonal" % what
    assert rb <= 1.0, "%s (b): |X L - I| is %.3g x its bound" % (what, rb)
    assert rc <= 1.0, "%s (c): |W - X^T X| is %.3g x its bound" % (what, rc)
    assert np.array_equal(W, W.T), "%s (c): W is not bitwise symmetric" % what
    assert sd <= bound_d, "%s (d): the end-to-end statistic %.3g is past %d x the CPU evaluations' %.3g" % (
        what, sd, M_SPREAD, bound_d / M_SPREAD)


def run_size_row(solve_mod, r, dtype, form):
    A, inv = make_matrix(r), inv64(r.n, r.kappa)
    bound_d = end_to_end_bound(r, dtype)
    with Configured(solve_mod, dtype):
        for a_off in (0, 1):
            what = "%s %s form %d a_off %d" % (row_id(r), dtype, form, a_off)
            L = call_factor(solve_mod, what, A, form, a_off)
            W, X = call_inverse(solve_mod, what, A, form, a_off)
            check_abcd(what, A, inv, L, X, W, dtype, bound_d)
            # (f) a second identical call
            assert_same(what + " (f) the factor of a second call", call_factor(solve_mod, what, A, form, a_off), L)
            W2, X2 = call_inverse(solve_mod, what, A, form, a_off)
            assert_same(what + " (f) W of a second call", W2, W)
            assert_same(what + " (f) X of a second call", X2, X)
            # (e) only the lower triangle is read
            for fill in ("nan", "finite"):
                Au = upper_replaced(A, fill)
                tag = "%s (e) upper triangle %s: " % (what, fill)
                assert_same(tag + "the factor", call_factor(solve_mod, what, Au, form, a_off), L)
                Wu, Xu = call_inverse(solve_mod, what, Au, form, a_off)
                assert_same(tag + "W", Wu, W)
                assert_same(tag + "X", Xu, X)


def run_slab_row(solve_mod, r, dtype, form, pad):
    A, inv = make_matrix(r), inv64(r.n, r.kappa)
    bound_d = end_to_end_bound(r, dtype)
    with Configured(solve_mod, dtype):
        for a_off in (0, 1):
            what = "%s+%d %s form %d a_off %d" % (row_id(r), pad, dtype, form, a_off)
            L = call_factor(solve_mod, what, A, form, a_off)
            S, Ls = call_columns(solve_mod, what, A, form, a_off, r.lo, r.cnt, pad)
            ra, sd = ratio_factor(L, A, dtype), statistic(S, inv, r.lo)
            print("FIGURES %s: (a) %.3g of the bound; (d) %.3g against %.3g = %.3g of the bound" % (
                what, ra, sd, bound_d, sd / bound_d))
            assert ra <= 1.0, "%s (a): |L L^T - A| is %.3g x its bound" % (what, ra)
            assert np.all(np.isfinite(S)), "%s: the slab is not finite" % what
            assert sd <= bound_d, "%s (d): the slab's statistic %.3g is past %d x the CPU evaluations' %.3g" % (
                what, sd, M_SPREAD, bound_d / M_SPREAD)
            assert_same(what + " (f) the factor left in W against the cnt = 0 factor", Ls, L)
            S2, L2 = call_columns(solve_mod, what, A, form, a_off, r.lo, r.cnt, pad)
            assert_same(what + " (f) the slab of a second call", S2, S)
            assert_same(what + " (f) the factor of a second call", L2, L)
            for fill in ("nan", "finite"):
                Su, Lu = call_columns(solve_mod, what, upper_replaced(A, fill), form, a_off, r.lo, r.cnt, pad)
                assert_same("%s (e) upper triangle %s: the slab" % (what, fill), Su, S)
                assert_same("%s (e) upper triangle %s: the factor" % (what, fill), Lu, L)


def params(rows, extra=()):
    """One test per row, dtype and form (and out_cols - cnt for the slabs)."""
    ps, ids = [], []
    for r in rows:
        for dtype in r.dtypes:
            for form in FORMS[dtype]:
                for x in (extra or (None,)):
                    ps.append((r, dtype, form) + (() if x is None else (x,)))
                    ids.append("%s%s-%s-form%d" % (row_id(r), "" if x is None else "+%d" % x, dtype, form))
    return pytest.mark.parametrize("r,dtype,form" + (",pad" if extra else ""), ps, ids=ids)


@params(SIZE_ROWS)
def test_factor_inverse_product(solve_mod, r, dtype, form):
    run_size_row(solve_mod, r, dtype, form)


@params(SLAB_ROWS, SLAB_PADS)
def test_inverse_columns(solve_mod, r, dtype, form, pad):
    run_slab_row(solve_mod, r, dtype, form, pad)


# ---- not positive definite --------------------------------------------------------------------------

def _eye_with(n, i, v):
    A = np.eye(n)
    A[i, i] = v
    return A


def _nan_in_the_second_block():
    A = np.array(_matrix(129, 1e2))
    A[70, 66] = np.nan  # lower triangle of the second diagonal block; the mirror entry stays finite
    return A


NOT_PD = [
    ("zero-1x1", lambda: np.zeros((1, 1))),
    ("minus-identity-5", lambda: -np.eye(5)),
    ("ones-2x2", lambda: np.ones((2, 2))),  # an exact zero pivot
    ("ragged-last-block-130", lambda: _eye_with(130, 129, -1.0)),
    ("second-outer-panel-300", lambda: _eye_with(300, 290, -1.0)),  # after a trailing update
    ("nan-in-the-second-block-129", _nan_in_the_second_block),
]
VALID_AFTER = size_row(65, "one block", "the valid case after a failure")


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("name,make", NOT_PD, ids=[n for n, _ in NOT_PD])
def test_not_positive_definite_is_an_error_and_the_next_call_is_clean(solve_mod, name, make, dtype):
    B = make()
    n = B.shape[0]
    b = B.flatten(order="F")
    A, inv = make_matrix(VALID_AFTER), inv64(VALID_AFTER.n, VALID_AFTER.kappa)
    bound_d = end_to_end_bound(VALID_AFTER, dtype)
    calls = [("spd_inverse", dict()), ("spd_inverse", dict(want_out2=True)),
             ("spd_inverse_columns", dict(lo=0, cnt=0)), ("spd_inverse_columns", dict(lo=n - 1, cnt=1)),
             ("spd_inverse_columns", dict(lo=0, cnt=n, out_cols=n + 3, want_out2=True))]
    with Configured(solve_mod, dtype):
        for form in (-1, 0, 1):  # both forms in both dtypes (f64 has one: the option is not read)
            for op, kw in calls:
                with pytest.raises(solve_mod.error, match=NOT_PD_MSG):
                    solve_mod.factor_op(op, n=n, a=b, form=form, **kw)
                what = "%s after %s %s %r form %d" % (dtype, name, op, kw, form)
                L = call_factor(solve_mod, what, A, form, 0)
                W, X = call_inverse(solve_mod, what, A, form, 0)
                check_abcd(what, A, inv, L, X, W, dtype, bound_d)


def test_the_valid_matrices_are_accepted_where_a_failure_is_one_entry_away(solve_mod):
    """The identities of the not-positive-definite cases without their bad entry: exact results."""
    for dtype in BOTH:
        with Configured(solve_mod, dtype):
            for n in (130, 300):
                for form in FORMS[dtype]:
                    W, X = call_inverse(solve_mod, "identity %d" % n, _eye_with(n, n - 1, 4.0), form, 0)
                    want = _eye_with(n, n - 1, 0.25)
                    assert np.array_equal(W, want) and np.array_equal(X, _eye_with(n, n - 1, 0.5))
