"""The block LDL^T (csrc/block.cc: ComputeFill, NextKey, ForwardSub, BackSub, BlockCholesky) on the
device, through the test entry eps_test_block_solve.

Every matrix is built twice from the same numpy arrays: with `ir` maps for the device and with the
oracle's LM / BlockMatrix.  Fill bounds, elimination order and factor types depend on structure
only: they are compared with the oracle AND with literal values, identical for both dtypes.
Numbers are compared with numpy fp64 on the assembled dense matrix (BlockMatrix.as_dense +
np.linalg.solve); the error of a solve is max|x - x_ref| / max|x_ref| over all keys, bounded by the
project's tolerances for explicit inverses (test_dense_inverse): 1e-9 in f64, 2e-3 in f32.  All the
well-conditioned systems here have cond_2 <= 20.
"""

import functools
import json
import math
import os

import numpy as np
import pytest
import scipy.sparse as sp

from epsilon_amd import ir
from oracle import epsilon_oracle as orc
from oracle.epsilon_oracle import LM
from tests import route_support as rs

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                     "reference_known_answers.json")))
TOL = {"f64": 1e-9, "f32": 2e-3}
MAX = "MAX"  # a key without a diagonal block
dtype = rs.dtype_fixture(("f64", "f32"), refine="auto")


# ---- one description of a block, two representations ------------------------------------------------
# ("dense", array) ("sparse", matrix) ("diag", vector) ("scalar", alpha, n) ("kron", spec, spec)
# ("T", spec)


def to_ir(s):
    if s[0] == "dense":
        return ir.dense_matrix(s[1])
    if s[0] == "sparse":
        return ir.sparse_matrix(s[1])
    if s[0] == "diag":
        return ir.diagonal_matrix(s[1])
    if s[0] == "scalar":
        return ir.scalar(s[1], s[2])
    if s[0] == "kron":
        return ir.kronecker_product(to_ir(s[1]), to_ir(s[2]))
    assert s[0] == "T"
    return to_ir(s[1]) if s[1][0] in ("diag", "scalar") else ir.transpose(to_ir(s[1]))


def to_lm(s):
    if s[0] == "dense":
        return LM.dense(s[1])
    if s[0] == "sparse":
        return LM.sparse(s[1])
    if s[0] == "diag":
        return LM.diagonal(s[1])
    if s[0] == "scalar":
        return LM.scalar(s[1], s[2])
    if s[0] == "kron":
        return LM.kron(to_lm(s[1]), to_lm(s[2]))
    assert s[0] == "T"
    return to_lm(s[1]).T()


def scaled(alpha, s):
    """alpha * block, as the scalar row of the multiply table forms it"""
    if s[0] in ("dense", "sparse", "diag"):
        return (s[0], alpha * s[1])
    if s[0] == "scalar":
        return ("scalar", alpha * s[1], s[2])
    assert s[0] == "kron"
    return ("kron", scaled(alpha, s[1]), scaled(1.0, s[2]))


def rows_of(s):
    if s[0] in ("dense", "sparse"):
        return s[1].shape[0]
    if s[0] == "diag":
        return len(s[1])
    if s[0] == "scalar":
        return s[2]
    return rows_of(s[1]) * rows_of(s[2])


def kkt(H, A, alpha, identity_of):
    """The blocks of  alpha (H + H^T) + (A + A^T) - sum of LeftIdentity of `identity_of`,
    written out block by block: {(row, col): spec}."""
    M = {}
    for (r, c), s in H.items():
        M[(r, c)] = scaled(alpha, s)
        M[(c, r)] = ("T", scaled(alpha, s))
    for (r, c), s in A.items():
        M[(r, c)] = s
        M[(c, r)] = ("T", s)
    for B in identity_of:
        for (r, c), s in B.items():
            M[(r, r)] = ("scalar", -1.0, rows_of(s))
    return M


def oracle_matrix(specs):
    M = orc.BlockMatrix()
    for (r, c), s in specs.items():
        M.set(r, c, to_lm(s))
    return M


def algebra_sum_square(H, A, alpha):  # prox.cc SumSquareProx::Init
    H, A = oracle_matrix(H), oracle_matrix(A)
    return (H + H.T()).scaled(alpha) + (A + A.T()) - H.left_identity() - A.left_identity()


def algebra_zero(H, A):  # prox.cc ZeroProx::Init
    H, A = oracle_matrix(H), oracle_matrix(A)
    return H + H.T() + A + A.T() - A.left_identity()


def assert_same_matrix(M, N):
    """the block-by-block KKT matrix is the one the constructors' algebra gives: keys, types, values"""
    assert sorted((r, c) for r, c, _ in M.entries()) == sorted((r, c) for r, c, _ in N.entries())
    for r, c, v in M.entries():
        w = N.get(r, c)
        assert v.type == w.type, (r, c, v, w)
        assert np.array_equal(v.as_dense(), w.as_dense()), (r, c)


class Case(object):
    """A KKT system with its oracle factorisation, elimination trace and dense fp64 form."""

    def __init__(self, name, specs, algebra=None, factor=True):
        self.name = name
        self.specs = specs
        self.M = oracle_matrix(specs)
        if algebra is not None:
            assert_same_matrix(self.M, algebra)
        self.keys = self.M.col_keys()
        self.dim = {c: self.M.col(c)[0][1].n for c in self.keys}
        self.dense = self.M.as_dense(self.keys, self.keys)
        assert np.array_equal(self.dense, self.dense.T)
        self.trace = []  # [({key: fill}, pivot)], replayed with next_key / remove_key
        A = self.M.copy()
        self.L, self.D_inv = orc.BlockMatrix(), orc.BlockMatrix()
        for _ in self.keys:
            fills = {k: orc.compute_fill(A, k) for k in A.col_keys()}
            key = orc.next_key(A)
            self.trace.append(({k: (MAX if f == orc.FILL_MAX else f) for k, f in fills.items()}, key))
            if factor:
                Di = orc.BlockMatrix()
                Di.set(key, key, A.get(key, key).inverse())
                V = orc.remove_key(A, key)
                self.L = self.L + (V @ Di)
                self.D_inv = self.D_inv + Di
                A = A - (V @ Di @ V.T())
            else:  # the large case: the order is structural, the values are not compared
                break
        self.order = [p for _, p in self.trace]

    def blocks(self):
        return [(r, c, to_ir(s)) for (r, c), s in sorted(self.specs.items())]

    def rhs(self, seed, keys=None):
        rng = np.random.RandomState(seed)
        full = {k: rng.uniform(-1, 1, self.dim[k]) for k in self.keys}
        return {k: full[k] for k in (keys or self.keys)}

    def reference(self, rhs):
        b = np.concatenate([rhs.get(k, np.zeros(self.dim[k])) for k in self.keys])
        x = np.linalg.solve(self.dense, b)
        off = np.cumsum([0] + [self.dim[k] for k in self.keys])
        return {k: x[off[i]:off[i + 1]] for i, k in enumerate(self.keys)}


def rel_error(x, ref):
    assert sorted(x) == sorted(ref), (sorted(x), sorted(ref))
    return max(np.abs(x[k] - ref[k]).max() for k in ref) / max(np.abs(ref[k]).max() for k in ref)


def uniform(seed, *shape):
    return np.random.RandomState(seed).uniform(-1, 1, size=shape)


def lasso_blocks(Hd):
    n = Hd.shape[1]
    return {("arg:0", "var:x"): ("dense", Hd)}, {("constraint:0", "var:x"): ("scalar", 1.0, n)}


@functools.lru_cache(maxsize=None)
def lasso_case(m, n, factor=True):
    # entries ~ 1/sqrt(max(m, n)): ||H|| stays O(1), the pivot I + 2 H H^T well conditioned
    H, A = lasso_blocks(uniform(100 + m, m, n) / math.sqrt(max(m, n)))
    alpha = math.sqrt(2)
    alg = algebra_sum_square(H, A, alpha) if factor else None
    return Case("lasso-%dx%d" % (m, n), kkt(H, A, alpha, [H, A]), alg, factor)


@functools.lru_cache(maxsize=None)
def mixed_case():
    rng = np.random.RandomState(7)
    m, n, q, alpha = 40, 30, 25, 1.3
    H = {("arg:0", "var:a"): ("dense", rng.uniform(-1, 1, (m, n)) / math.sqrt(m)),
         ("arg:0", "var:b"): ("diag", rng.uniform(0.5, 1.5, m)),
         ("arg:1", "var:c"): ("dense", rng.uniform(-1, 1, (33, q)) / math.sqrt(33))}
    S = sp.random(q, n, 0.2, random_state=rng, format="csc")
    A = {("constraint:0", "var:a"): ("sparse", S),
         ("constraint:0", "var:c"): ("scalar", -1.0, q),
         ("constraint:1", "var:b"): ("scalar", 1.0, m),
         ("constraint:2", "var:a"): ("scalar", 1.0, n)}
    return Case("mixed", kkt(H, A, alpha, [H, A]), algebra_sum_square(H, A, alpha))


@functools.lru_cache(maxsize=None)
def tie_case():
    H = {("arg:0", "var:p"): ("dense", uniform(11, 12, 9) / math.sqrt(3)),
         ("arg:1", "var:q"): ("dense", uniform(12, 12, 9) / math.sqrt(3))}
    A = {("constraint:0", "var:p"): ("scalar", 1.0, 9), ("constraint:0", "var:q"): ("scalar", -1.0, 9)}
    return Case("tie", kkt(H, A, 1.0, [H, A]), algebra_sum_square(H, A, 1.0))


@functools.lru_cache(maxsize=None)
def matrix_case():
    H = {("arg:0", "var:X"): ("kron", ("scalar", 1.0, 3), ("dense", uniform(13, 10, 14) / math.sqrt(14)))}
    A = {("constraint:0", "var:X"): ("scalar", 1.0, 42)}
    alpha = math.sqrt(2)
    return Case("matrix", kkt(H, A, alpha, [H, A]), algebra_sum_square(H, A, alpha))


@functools.lru_cache(maxsize=None)
def zero_case():
    H, A = lasso_blocks(uniform(14, 6, 15) / math.sqrt(15))
    return Case("zero", kkt(H, A, 1.0, [A]), algebra_zero(H, A))


LASSO_SHAPES = [(8, 20), (20, 8), (65, 130), (130, 65), (300, 301)]
CASES = dict([("lasso-%dx%d" % s, functools.partial(lasso_case, *s)) for s in LASSO_SHAPES] +
             [("mixed", mixed_case), ("tie", tie_case), ("matrix", matrix_case), ("zero", zero_case)])

# the literal expectations: first-step fill bounds and elimination order
LITERAL = {
    "mixed": ({"arg:0": 3340, "arg:1": 625, "constraint:0": 2401, "constraint:1": 1, "constraint:2": 1,
               "var:a": MAX, "var:b": MAX, "var:c": MAX},
              ["constraint:1", "constraint:2", "var:b", "arg:1", "var:c", "arg:0", "var:a", "constraint:0"]),
    "tie": ({"arg:0": 81, "arg:1": 81, "constraint:0": 4, "var:p": MAX, "var:q": MAX},
            ["constraint:0", "arg:0", "arg:1", "var:p", "var:q"]),
    "matrix": ({"arg:0": 1764, "constraint:0": 1, "var:X": MAX}, ["constraint:0", "var:X", "arg:0"]),
    "zero": ({"arg:0": MAX, "constraint:0": 1, "var:x": MAX}, ["constraint:0", "var:x", "arg:0"]),
}
for (_m, _n) in LASSO_SHAPES:
    LITERAL["lasso-%dx%d" % (_m, _n)] = (
        {"arg:0": _n * _n, "constraint:0": 1, "var:x": MAX},
        ["constraint:0", "var:x", "arg:0"] if _m < _n else ["constraint:0", "arg:0", "var:x"])


def device_fills(fills, solve_mod):
    return {k: (MAX if f == solve_mod.FILL_MAX else f) for k, f in fills.items()}


def device_type(kind):
    return kind[0] if isinstance(kind, tuple) else kind


_factor_cache = {}


def factored(solve_mod, dtype, name, seed=1):
    """One device factorisation + solve per (case, dtype), shared by the tests that read it."""
    key = (name, dtype)
    if key not in _factor_cache:
        case = CASES[name]()
        rhs = case.rhs(seed)
        _factor_cache[key] = (case, rhs, solve_mod.block_solve(case.blocks(), rhs, mode="factor"))
    return _factor_cache[key]


# ---- 1. the reference's own four tests (vector/block_cholesky_test.cc) ------------------------------


def test_reference_compute_fill_4_and_25(solve_mod, dtype):
    A0 = uniform(0, 5, 2)
    blocks = [("one", "one", ir.identity(5)), ("one", "two", ir.dense_matrix(A0)),
              ("two", "one", ir.transpose(ir.dense_matrix(A0))), ("two", "two", ir.identity(2))]
    want = GOLDEN["compute_fill"]["fill_when_eliminating"]
    assert (want["one"], want["two"]) == (4, 25)
    got = solve_mod.block_solve(blocks, mode="fill")["fill"]
    assert got == {"one": want["one"], "two": want["two"]}


def test_reference_forward_and_back_sub(solve_mod, dtype):
    rng = np.random.RandomState(0)
    L0, b1, b2 = rng.uniform(-1, 1, (5, 2)), rng.uniform(-1, 1, 2), rng.uniform(-1, 1, 5)
    rhs, keys = {"one": b1, "two": b2}, ["one", "two"]
    # b - sum of at most 5 products of numbers in [-1, 1], u = 2^-53 / 2^-24: the operands are
    # rounded to the dtype (3u per product with its own rounding, u for b), each of the 5 additions
    # rounds a partial sum of at most 6: 15u + u + 30u = 46u
    tol = {"f64": 1e-14, "f32": 3e-6}[dtype]
    x = solve_mod.block_solve([("two", "one", ir.dense_matrix(L0))], rhs, mode="forward", keys=keys)["x"]
    assert sorted(x) == keys
    np.testing.assert_allclose(x["one"], b1, rtol=0, atol=tol)
    np.testing.assert_allclose(x["two"], b2 - L0 @ b1, rtol=0, atol=tol)
    LT = [("one", "two", ir.transpose(ir.dense_matrix(L0)))]
    x = solve_mod.block_solve(LT, rhs, mode="back", keys=keys)["x"]
    np.testing.assert_allclose(x["one"], b1 - L0.T @ b2, rtol=0, atol=tol)
    np.testing.assert_allclose(x["two"], b2, rtol=0, atol=tol)
    # an absent source is skipped, a target the rhs lacks is created (as -L b)
    x = solve_mod.block_solve([("two", "one", ir.dense_matrix(L0))], {"one": b1}, mode="forward", keys=keys)["x"]
    np.testing.assert_allclose(x["two"], -L0 @ b1, rtol=0, atol=tol)
    x = solve_mod.block_solve([("two", "one", ir.dense_matrix(L0))], {"two": b2}, mode="forward", keys=keys)["x"]
    assert sorted(x) == ["two"] and np.allclose(x["two"], b2, rtol=0, atol=tol)


def test_reference_scalar_dense_solve(solve_mod, dtype):
    A12 = uniform(0, 5, 2)
    specs = {("one", "one"): ("scalar", 10.0, 5), ("one", "two"): ("dense", A12),
             ("two", "one"): ("T", ("dense", A12)), ("two", "two"): ("scalar", 10.0, 2)}
    case = Case("ten", specs)
    rhs = case.rhs(0)
    out = solve_mod.block_solve(case.blocks(), rhs, mode="solve")
    err = rel_error(out["x"], case.reference(rhs))
    print("reference scalar/dense solve %s: error %.3g" % (dtype, err))
    assert out["order"] == case.order
    assert err <= TOL[dtype]


# ---- 2. order, trace and factor types ---------------------------------------------------------------


@pytest.mark.parametrize("name", sorted(CASES))
def test_fill_order_and_types(solve_mod, dtype, name):
    case, _, out = factored(solve_mod, dtype, name)
    first, order = LITERAL[name]
    fills = device_fills(solve_mod.block_solve(case.blocks(), mode="fill")["fill"], solve_mod)
    assert fills == first
    assert case.trace[0][0] == first and case.order == order  # the oracle agrees with the literals
    assert out["order"] == order
    trace = [(device_fills(f, solve_mod), p) for f, p in out["trace"]]
    assert trace == case.trace
    for name_, got, want in (("L", out["L"], case.L), ("D_inv", out["D_inv"], case.D_inv)):
        assert sorted(got) == sorted((r, c) for r, c, _ in want.entries()), name_
        for r, c, v in want.entries():
            assert device_type(got[(r, c)][0]) == v.type, (name_, r, c, got[(r, c)][0], v)
            if v.type == orc.KRONECKER:
                assert got[(r, c)][0] == (orc.KRONECKER, v.KA.type, v.KB.type), (name_, r, c)


@pytest.mark.parametrize("name", ["lasso-8x20", "lasso-65x130", "lasso-300x301", "matrix"])
def test_types_the_fused_pattern_reads(solve_mod, dtype, name):
    """SumSquareProx::DescribeLeastSquares: order [constraint, var, arg], L(var, constraint) = -1,
    D_inv(constraint) = -1, D_inv(var) = 1, no L(arg, constraint), L(arg, var) and D_inv(arg) dense
    or, for a matrix variable, kron(scalar, dense)."""
    _, _, out = factored(solve_mod, dtype, name)
    ck, vk, ak = out["order"]
    assert (ck, ak) == ("constraint:0", "arg:0") and vk in ("var:x", "var:X")
    L, D = out["L"], out["D_inv"]
    n = L[(vk, ck)][1].shape[0]
    for blk, value in ((L[(vk, ck)], -1.0), (D[(ck, ck)], -1.0), (D[(vk, vk)], 1.0)):
        assert blk[0] == orc.SCALAR
        assert np.array_equal(blk[1], value * np.eye(n))
    assert (ak, ck) not in L
    big = (orc.KRONECKER, orc.SCALAR, orc.DENSE) if name == "matrix" else orc.DENSE
    assert L[(ak, vk)][0] == big and D[(ak, ak)][0] == big


# ---- 3. numbers -------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", sorted(CASES))
def test_factors_and_solution(solve_mod, dtype, name):
    case, rhs, out = factored(solve_mod, dtype, name)
    worst = 0.0
    for got, want in ((out["L"], case.L), (out["D_inv"], case.D_inv)):
        for r, c, v in want.entries():
            ref = v.as_dense()
            assert got[(r, c)][1].shape == ref.shape
            worst = max(worst, np.abs(got[(r, c)][1] - ref).max() / np.abs(ref).max())
    ref = case.reference(rhs)
    err = rel_error(out["x"], ref)
    cond = np.linalg.cond(case.dense)
    print("%s %s: cond_2 %.3g, factors %.3g, solution %.3g" % (name, dtype, cond, worst, err))
    assert cond <= 20
    assert worst <= TOL[dtype]
    assert err <= TOL[dtype]
    # a second solve on the same factorisation: the same bytes
    assert sorted(out["x_again"]) == sorted(out["x"])
    for k in out["x"]:
        assert out["x"][k].tobytes() == out["x_again"][k].tobytes(), k


def test_solution_through_the_symmetric_apply(solve_mod, dtype):
    """lasso structure at (1030, 1300): D_inv(arg:0) has 1030 rows, its apply inside the
    substitution is the symmetric kernel used from 1024 rows.  The solution only."""
    case = lasso_case(1030, 1300, False)
    assert case.order[0] == "constraint:0"
    rhs = case.rhs(2)
    out = solve_mod.block_solve(case.blocks(), rhs, mode="solve")
    assert out["order"] == ["constraint:0", "var:x", "arg:0"]
    err = rel_error(out["x"], case.reference(rhs))
    print("lasso-1030x1300 %s: solution %.3g, refine_steps %d, estimate %.3g" % (
        dtype, err, out["refine_steps"], out["condition_estimate"]))
    assert err <= TOL[dtype]
    for k in out["x"]:
        assert out["x"][k].tobytes() == out["x_again"][k].tobytes(), k


@pytest.mark.parametrize("name,present", [("lasso-8x20", ["var:x"]), ("lasso-20x8", ["arg:0"]),
                                          ("lasso-65x130", ["constraint:0"]),
                                          ("mixed", ["var:a", "arg:1"]), ("matrix", ["var:X"])])
def test_rhs_that_lacks_keys(solve_mod, dtype, name, present):
    """Substitute skips absent sources and creates the targets: the solution has every key."""
    case = CASES[name]()
    rhs = case.rhs(3, present)
    out = solve_mod.block_solve(case.blocks(), rhs, mode="solve")
    err = rel_error(out["x"], case.reference(rhs))
    print("%s %s rhs on %s: solution %.3g" % (name, dtype, present, err))
    assert err <= TOL[dtype]


# ---- 4. ill-conditioned pivot and refinement --------------------------------------------------------


@functools.lru_cache(maxsize=None)
def ill_case(sigma_max):
    m, n = 40, 70
    rng = np.random.RandomState(5)
    U, _ = np.linalg.qr(rng.randn(m, m))
    V, _ = np.linalg.qr(rng.randn(n, m))
    sigma = np.logspace(-2, math.log10(sigma_max), m)
    Hd = (U * sigma) @ V.T
    H, A = lasso_blocks(Hd)
    case = Case("ill-%g" % sigma_max, kkt(H, A, math.sqrt(2), [H, A]), algebra_sum_square(H, A, math.sqrt(2)))
    pivot = -(np.eye(m) + 2 * Hd @ Hd.T)
    return case, np.linalg.cond(pivot, 2), np.linalg.cond(pivot, 1)


# kappa_2 of the arg:0 pivot -(I + 2 A A^T), (1 + 2 sigma_max^2) / (1 + 2e-4), and the RefineStepsFor
# band of an estimate between kappa_2 and 1.5 kappa_2; kappa_1 (about 3e4 and 2e6: it depends on U)
# is taken from numpy
ILL = {50: (5.0e3, 1), 400: (3.2e5, 2)}


@pytest.mark.parametrize("sigma_max", sorted(ILL))
def test_ill_conditioned_pivot_f64(solve_mod, sigma_max):
    case, _, _ = ill_case(sigma_max)
    solve_mod.set_option("dtype", "f64")
    try:
        rhs = case.rhs(4)
        out = solve_mod.block_solve(case.blocks(), rhs, mode="solve")
    finally:
        solve_mod.set_option("dtype", "f32")
    err = rel_error(out["x"], case.reference(rhs))
    print("ill sigma_max=%g f64: error %.3g" % (sigma_max, err))
    assert out["order"] == ["constraint:0", "var:x", "arg:0"]
    assert out["refine_steps"] == 0
    assert err <= 1e-9


@pytest.mark.parametrize("sigma_max", sorted(ILL))
def test_ill_conditioned_pivot_f32_refinement(solve_mod, sigma_max):
    """Measured on an MI355X (errors against numpy fp64, not against the library):
         sigma_max  50: estimate 6649   (kappa_2 5000,  kappa_1 3.37e4), 1 step,
                        error 1.48e-6 refined, 8.06e-5 unrefined (ratio 55)
         sigma_max 400: estimate 4.54e5 (kappa_2 3.2e5, kappa_1 2.18e6), 2 steps,
                        error 6.9e-6 refined, 3.07e-3 unrefined (ratio 445)"""
    k2_said, steps = ILL[sigma_max]
    case, k2, k1 = ill_case(sigma_max)
    assert abs(k2 / k2_said - 1) < 0.01 and 6 * k2 < k1 < 8 * k2, (k2, k1)
    assert np.linalg.cond(case.dense) < 1000
    rhs = case.rhs(4)
    ref = case.reference(rhs)
    solve_mod.set_option("dtype", "f32")
    try:
        solve_mod.set_option("refine", "auto")
        solve_mod.block_solve_stats(reset=True)
        refined = solve_mod.block_solve(case.blocks(), rhs, mode="solve")
        stats = solve_mod.block_solve_stats(reset=True)
        solve_mod.set_option("refine", "0")
        plain = solve_mod.block_solve(case.blocks(), rhs, mode="solve")
    finally:
        solve_mod.set_option("refine", "auto")
    e_ref, e_plain = rel_error(refined["x"], ref), rel_error(plain["x"], ref)
    est = refined["condition_estimate"]
    print("ill sigma_max=%g f32: kappa_2 %.4g kappa_1 %.4g estimate %.4g (band %.4g..%.4g) steps %d; "
          "error refined %.3g unrefined %.3g ratio %.3g" % (
              sigma_max, k2, k1, est, k2, 1.5 * k2, refined["refine_steps"], e_ref, e_plain,
              e_plain / e_ref))
    assert plain["refine_steps"] == 0
    assert refined["refine_steps"] == steps
    assert stats == (est, steps)  # BlockSolveStats records the test entry's factorisation too
    assert math.isfinite(est) and est <= k1 * (1 + 1e-3)
    if not k2 <= est <= 1.5 * k2:
        print("FINDING: ConditionEstimate %.4g outside [kappa_2, 1.5 kappa_2]" % est)
    assert e_ref < e_plain
    assert e_ref <= 2e-3


def test_well_conditioned_f32_is_not_refined(solve_mod):
    solve_mod.set_option("dtype", "f32")
    solve_mod.set_option("refine", "auto")
    case = lasso_case(65, 130)
    out = solve_mod.block_solve(case.blocks(), case.rhs(1), mode="solve")
    print("lasso-65x130 f32: estimate %.4g" % out["condition_estimate"])
    assert out["refine_steps"] == 0


# ---- 5. failure is an error, not an abort -----------------------------------------------------------


def test_no_diagonal_block_is_an_error(solve_mod, dtype):
    B = uniform(20, 6, 4)
    blocks = [("one", "two", ir.dense_matrix(B)), ("two", "one", ir.transpose(ir.dense_matrix(B)))]
    with pytest.raises(solve_mod.error, match="no key with a diagonal block"):
        solve_mod.block_solve(blocks, {"one": np.ones(6)}, mode="solve")
    assert solve_mod.block_solve(blocks, mode="fill")["fill"] == {"one": solve_mod.FILL_MAX,
                                                                  "two": solve_mod.FILL_MAX}
    case = lasso_case(8, 20)
    rhs = case.rhs(1)
    out = solve_mod.block_solve(case.blocks(), rhs, mode="solve")
    assert rel_error(out["x"], case.reference(rhs)) <= TOL[dtype]
