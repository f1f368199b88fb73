"""Batched solves of ZERO-term problems: members of _solve.solve_batch on the
fused ZERO-term route that share the data matrix run as one group - per sweep one batched pass with
the ZERO column chain per `width` members (tag "batch_zero_pass"), ONE row launch for all of them
("batch_zero_rows"; basis pursuit has none: "batch_reduce_partials") and one batched apply of the
packed inverse ("batch_symv_packed", from 1024 rows).  The contract is test_gpu_batch.py's: result k
is exactly what _solve.solve returns for member k alone - status, residual fields, every variable.

Shapes (test_gpu_fused_zero.py's floors): (256, 601) the row floor, 64 live threads of the pass, odd
n with an unpaired last column; (260, 601) rows past a wave boundary; (1028, 2051) a ragged second
row chunk and the packed symmetric apply.  Members of one kind and shape come from one seed, so
their matrices have equal content-hashed data keys and the blobs merge into one."""

import math

import numpy as np
import pytest

from epsilon_amd import ir, problems, wire
from oracle import epsilon_oracle as orc
from tests import route_support as rs

pytestmark = pytest.mark.gpu

FIXED = dict(abs_tol=0.0, rel_tol=0.0)
SETUP = ("gemm", "syrk", "spd_inverse", "pack_inverse")  # what setup_counts counts here
ON = {}  # options of a call here beside "dtype": none, the group is the library's default


# ---- 1. lambda paths, members stopping at different checks ---------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("shape", [(256, 601), (260, 601)])
@pytest.mark.parametrize("kind", ["hinge", "deadzone", "logreg"])
def test_paths_are_bit_identical_with_mixed_stopping(solve_mod, kind, shape, dtype):
    """The CPU oracle in f64 stops the full-length solves at hinge 1000 (not converged) / 520 / 270 /
    130 / 60, logreg 430 / 120 / 60 / 40 / 80, deadzone 470 / 530 / 380: under the cap members stop
    at distinct checks and (hinge, logreg) some reach it."""
    max_it = 500 if kind == "deadzone" else 300
    batch, tagsb, single, _ = rs.run_both(solve_mod, rs.members(kind, shape), dtype, ON, max_iterations=max_it)
    st = [rs.status(s) for s, _ in single]
    print(kind, shape, dtype, [(s.state, s.num_iterations) for s in st])
    assert len({s.num_iterations for s in st}) >= 2
    if kind != "deadzone":
        assert wire.SolverStatus.MAX_ITERATIONS_REACHED in [s.state for s in st]
    cb = rs.base_counts(tagsb)
    assert cb.get("batch_zero_pass", 0) > 0 and cb.get("batch_zero_rows", 0) > 0 and "zero_fused" not in cb, sorted(cb)
    rs.assert_identical(batch, single)


# ---- 2. basis pursuit, several right-hand sides ---------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_basis_pursuit_with_several_right_hand_sides(solve_mod, dtype):
    batch, tagsb, single, _ = rs.run_both(solve_mod, rs.members("bp", (256, 601)), dtype, ON, max_iterations=200)
    cb = rs.base_counts(tagsb)
    assert cb.get("batch_zero_pass", 0) > 0 and cb.get("batch_reduce_partials", 0) > 0, sorted(cb)
    assert "batch_zero_rows" not in cb and "zero_fused" not in cb, sorted(cb)
    rs.assert_identical(batch, single)


# ---- 3. launch counts and the shared setup --------------------------------------------------------
@pytest.mark.parametrize("dt,kind,k,width", [("f32", "hinge", 5, 8),    # one pass per sweep
                                             ("f64", "logreg", 7, 6)])  # two passes
def test_launch_counts_and_shared_setup(solve_mod, dt, kind, k, width):
    """Widths of the ZERO chain per (chunks per thread, dtype): DESIGN.md 3.6 (m = 1028 is two
    16-byte chunks per thread in f32, width 8, and three, run as four, in f64, width 6)."""
    shape, n_sweeps = (1028, 2051), 60
    batch, tagsb, single, tags1 = rs.run_both(solve_mod, rs.members(kind, shape, k), dt, ON, max_iterations=n_sweeps,
                                              **FIXED)
    assert all(rs.sweeps(st) == n_sweeps for st, _ in batch)
    c1, cb = rs.base_counts(tags1), rs.base_counts(tagsb)
    assert c1.get("zero_fused") == n_sweeps and "zero_fused" not in cb, (sorted(c1), sorted(cb))
    assert cb.get("batch_zero_pass") == n_sweeps * math.ceil(k / width), cb
    assert cb.get("batch_zero_rows") == n_sweeps and cb.get("batch_symv_packed") == n_sweeps, cb
    assert "zero_fused_rows" not in cb, sorted(cb)
    s1, sb = rs.setup_counts(tags1, SETUP), rs.setup_counts(tagsb, SETUP)
    assert any("pack_inverse" in t for t in s1) and any("spd_inverse" in t for t in s1), sorted(tags1)
    assert sb == s1, (s1, sb)
    rs.assert_identical(batch, single)


# ---- 4. more members than one launch holds --------------------------------------------------------
def test_more_members_than_one_launch_holds(solve_mod):
    """f32 at one chunk per thread: width 8, so 9 members are launches of 8 and 1"""
    k, n_sweeps = 9, 30
    batch, tagsb, single, _ = rs.run_both(solve_mod, rs.members("hinge", (256, 601), k), "f32", ON,
                                          max_iterations=n_sweeps, **FIXED)
    cb = rs.base_counts(tagsb)
    assert cb.get("batch_zero_pass") == 2 * n_sweeps and cb.get("batch_zero_rows") == n_sweeps, cb
    rs.assert_identical(batch, single)


# ---- 5. against the CPU oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hinge", "logreg", "bp"])
def test_batch_matches_the_oracle_f64(solve_mod, kind):
    probs = rs.members(kind, (256, 601))[:3]
    pbs, data = [p.SerializeToString() for p in probs], rs.union_data(probs)
    sb = wire.SolverParams(max_iterations=60, **FIXED).SerializeToString()
    with rs.options(solve_mod, dtype="f64"):
        batch, tagsb = rs.profiled(solve_mod, lambda: solve_mod.solve_batch(pbs, None, sb, data))
    assert rs.base_counts(tagsb).get("batch_zero_pass") == 60, sorted(tagsb)
    for pb, (stb, xb) in zip(pbs, batch):
        sto, xo = orc.solve(pb, [], sb, data)
        rs.assert_matches_oracle(stb, rs.arrays(xb), rs.status(sto), rs.arrays(xo), "f64")


# ---- 6. a mixed batch, and the route switched off ---------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_mixed_batch_and_fallbacks(solve_mod, dtype):
    shape = (256, 601)
    m, n = shape
    on_c1 = rs.members("hinge", shape)[1:3]
    # a deadzone member on the hinge members' matrix: C of hinge_l1, the rows' offset from a vector b
    C = problems.hinge_l1(m, n)[1]["C"]
    b = np.random.RandomState(3).randn(m)
    lam = 0.3 * np.abs(C.T.dot(np.sign(b))).max()
    deadzone = problems._graph_form(
        lambda x, z: [ir.prox(wire.ProxFunction.SUM_DEADZONE, z, scaled_zone_params=wire.ProxScaledZoneParams(m=0.5)),
                      ir.prox(wire.ProxFunction.NORM_1, x, alpha=lam)], C, -b)
    other = problems.hinge_l1(m, n, seed=1)[0]
    small = problems.hinge_l1(80, 40, seed=1)[0]
    lasso = rs.lasso_pair(300, 700, seed=6)
    probs = [on_c1[0], lasso[0], other, deadzone, small, on_c1[1], lasso[1]]
    zero_only = [on_c1[0], other, deadzone, small, on_c1[1]]
    batch, tagsb, single, _ = rs.run_both(solve_mod, probs, dtype, ON, max_iterations=120)
    cb = rs.base_counts(tagsb)
    assert cb.get("batch_fused_pass", 0) > 0 and cb.get("batch_zero_pass", 0) > 0, sorted(cb)
    # the member on another matrix runs alone on the single route, and it is the only one that does:
    # the deadzone member shares the hinge members' group (one row launch per sweep for the three)
    assert cb.get("zero_fused") == rs.sweeps(single[2][0]), (cb, rs.sweeps(single[2][0]))
    assert cb["batch_zero_rows"] == cb["batch_zero_pass"] == max(rs.sweeps(single[i][0]) for i in (0, 3, 5)), cb
    rs.assert_identical(batch, single)

    batch0, tags0, single0, _ = rs.run_both(solve_mod, zero_only, dtype, dict(fused_zero="0"), max_iterations=120)
    assert not [t for t in rs.base_counts(tags0) if t.startswith(("batch_zero", "zero_fused"))], sorted(tags0)
    rs.assert_identical(batch0, single0)
