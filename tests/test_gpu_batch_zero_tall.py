"""Batched solves of tall ZERO-term problems (DESIGN.md 3.6 "Tall members", option "batch_zero_tall"):
members of _solve.solve_batch on the tall ZERO-term route (3.11 "Tall C") that share the data matrix
run as one group.  Hinge / deadzone members: per sweep one batched pass over the transposed copy per
`width` members (tag "batch_zero_tall_pass"), ONE x-side launch for all ("batch_zero_tall_cols") and
one batched apply of the packed n x n inverse ("batch_symv_packed", from 1024 columns).  Logistic
members: the pass in halves ("batch_zero_tall_dot", "batch_zero_tall_acc") around ONE launch over the
samples of all ("batch_zero_tall_samples").  The contract is test_gpu_batch.py's: result k is exactly
what _solve.solve returns for member k alone - status, residual fields, every variable.

Every call here sets "batch_zero_tall" = "1", "fused_zero_tall" = "1" and "fused_zero_tall_smooth" =
"1" (the logistic form's "auto" starts at 512 columns, above two of the shapes) and puts "0", "auto",
"auto" back.

Shapes (test_gpu_fused_zero_tall.py's floors): (601, 256) the column floor, 64 live threads of the
pass, odd m with an unpaired last streamed column; (603, 260) columns past a wave boundary;
(2051, 1028) a ragged second chunk per thread and the packed symmetric apply.  Members of one kind
and shape come from one seed, so their matrices have equal content-hashed data keys, the blobs
merge into one and the members find one transposed copy in the batch's cache."""

import math

import numpy as np
import pytest

from epsilon_amd import ir, problems, wire
from oracle import epsilon_oracle as orc
from tests import route_support as rs

pytestmark = pytest.mark.gpu

FIXED = dict(abs_tol=0.0, rel_tol=0.0)
# options of every call here beside "dtype" (the module docstring)
ON = dict(batch_zero_tall="1", fused_zero_tall="1", fused_zero_tall_smooth="1")
# what a sweep of the single tall route launches ("zero_tall_head" is an Init launch of a logistic
# member, in a group as alone)
SINGLE_SWEEP = ("zero_tall", "zero_tall_cols", "zero_tall_dot", "zero_tall_samples", "zero_tall_acc")
ZONE_GROUP = ("batch_zero_tall_pass", "batch_zero_tall_cols")
LOGISTIC_GROUP = ("batch_zero_tall_dot", "batch_zero_tall_samples", "batch_zero_tall_acc", "batch_zero_tall_cols")


def group_tags(kind):
    return LOGISTIC_GROUP if kind == "logreg" else ZONE_GROUP


# ---- 1. lambda paths, members stopping at different checks ---------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("shape", [(601, 256), (603, 260)])
@pytest.mark.parametrize("kind", ["hinge", "deadzone", "logreg"])
def test_paths_are_bit_identical_with_mixed_stopping(solve_mod, kind, shape, dtype):
    """The CPU oracle in f64 stops these solves under the cap (300, deadzone 500) at
    (601, 256): hinge 300 (cap), 300 (cap), 250, 100, 50; logreg 300 (cap), 130, 70, 40, 100;
    deadzone 420, 480, 440;  (603, 260): hinge 300, 300, 200, 100, 40; logreg 300, 120, 60, 40, 100;
    deadzone 410, 470, 450 - members stop at distinct checks and (hinge, logreg) some reach the cap."""
    max_it = 500 if kind == "deadzone" else 300
    batch, tagsb, single, _ = rs.run_both(solve_mod, rs.members(kind, shape), dtype, ON, max_iterations=max_it)
    st = [rs.status(s) for s, _ in single]
    print(kind, shape, dtype, [(s.state, s.num_iterations) for s in st])
    assert len({s.num_iterations for s in st}) >= 2
    if kind != "deadzone":
        assert wire.SolverStatus.MAX_ITERATIONS_REACHED in [s.state for s in st]
    cb = rs.base_counts(tagsb)
    assert all(cb.get(t, 0) > 0 for t in group_tags(kind)), sorted(cb)
    assert not [t for t in SINGLE_SWEEP if t in cb], sorted(cb)
    rs.assert_identical(batch, single)


# ---- 2. launch counts and the shared setup --------------------------------------------------------
@pytest.mark.parametrize("dt,kind,k,widths", [("f32", "hinge", 5, {"pass": 8}),
                                              ("f64", "logreg", 7, {"dot": 12, "acc": 12})])
def test_launch_counts_and_shared_setup(solve_mod, dt, kind, k, widths):
    """Widths of the tall chains per (chunks per thread, dtype): DESIGN.md 3.6 (n = 1028 is two
    16-byte chunks per thread in f32, kChainZeroTall: width 8; three, run as four, in f64, the two
    halves of the tall pass: width 12)."""
    shape, n_sweeps = (2051, 1028), 60
    batch, tagsb, single, tags1 = rs.run_both(solve_mod, rs.members(kind, shape, k), dt, ON, max_iterations=n_sweeps,
                                              **FIXED)
    assert all(rs.sweeps(st) == n_sweeps for st, _ in batch)
    c1, cb = rs.base_counts(tags1), rs.base_counts(tagsb)
    first_pass = "zero_tall" if kind == "hinge" else "zero_tall_dot"
    assert c1.get(first_pass) == n_sweeps and c1.get("zero_tall_cols") == n_sweeps, sorted(c1)
    assert not [t for t in SINGLE_SWEEP if t in cb], sorted(cb)
    for half, width in widths.items():
        assert cb.get("batch_zero_tall_" + half) == n_sweeps * math.ceil(k / width), (half, cb)
    assert cb.get("batch_zero_tall_cols") == n_sweeps and cb.get("batch_symv_packed") == n_sweeps, cb
    assert cb.get("batch_zero_tall_samples", 0) == (n_sweeps if kind == "logreg" else 0), cb
    s1, sb = rs.setup_counts(tags1), rs.setup_counts(tagsb)
    assert any("pack_inverse" in t for t in s1) and any("spd_inverse" in t for t in s1), sorted(tags1)
    assert sb == s1, (s1, sb)
    assert rs.base_counts(tags1).get("transpose_copy") == 1 and cb.get("transpose_copy") == 1, (sorted(c1), sorted(cb))
    rs.assert_identical(batch, single)


# ---- 3. more members than one launch holds --------------------------------------------------------
def test_more_members_than_one_launch_holds(solve_mod):
    """f32 at one chunk per thread: kChainZeroTall has width 8, so 9 members are launches
    of 8 and 1"""
    k, n_sweeps = 9, 30
    batch, tagsb, single, _ = rs.run_both(solve_mod, rs.members("hinge", (601, 256), k), "f32", ON,
                                          max_iterations=n_sweeps, **FIXED)
    cb = rs.base_counts(tagsb)
    assert cb.get("batch_zero_tall_pass") == 2 * n_sweeps and cb.get("batch_zero_tall_cols") == n_sweeps, cb
    rs.assert_identical(batch, single)


# ---- 4. against the CPU oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hinge", "logreg"])
def test_batch_matches_the_oracle_f64(solve_mod, kind):
    probs = rs.members(kind, (601, 256))[:3]
    pbs, data = [p.SerializeToString() for p in probs], rs.union_data(probs)
    sb = wire.SolverParams(max_iterations=60, **FIXED).SerializeToString()
    with rs.options(solve_mod, dtype="f64", **ON):
        batch, tagsb = rs.profiled(solve_mod, lambda: solve_mod.solve_batch(pbs, None, sb, data))
    cb = rs.base_counts(tagsb)
    assert all(cb.get(t) == 60 for t in group_tags(kind)), sorted(cb)
    for pb, (stb, xb) in zip(pbs, batch):
        sto, xo = orc.solve(pb, [], sb, data)
        rs.assert_matches_oracle(stb, rs.arrays(xb), rs.status(sto), rs.arrays(xo), "f64")


# ---- 5. a mixed batch, and the group switched off ---------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_mixed_batch_and_fallbacks(solve_mod, dtype):
    shape = (601, 256)
    m, n = shape
    on_c1 = rs.members("hinge", shape)[1:3]
    # a deadzone member and a logistic pair on the hinge members' matrix: C of hinge_l1
    C = problems.hinge_l1(m, n)[1]["C"]
    b = np.random.RandomState(3).randn(m)
    lam = 0.3 * np.abs(C.T.dot(np.sign(b))).max()
    deadzone = problems._graph_form(
        lambda x, z: [ir.prox(wire.ProxFunction.SUM_DEADZONE, z, scaled_zone_params=wire.ProxScaledZoneParams(m=0.5)),
                      ir.prox(wire.ProxFunction.NORM_1, x, alpha=lam)], C, -b)
    llam = np.abs(C.T.dot(np.full(m, 0.5))).max()
    logreg = [problems._graph_form(
        lambda x, z, f=f: [ir.prox(wire.ProxFunction.SUM_LOGISTIC, z, alpha=1.0),
                           ir.prox(wire.ProxFunction.NORM_1, x, alpha=f * llam)], C, None) for f in (0.1, 0.05)]
    other = problems.hinge_l1(m, n, seed=1)[0]
    fat = members_fat()
    lasso = rs.lasso_pair(300, 700, seed=6)
    probs = [on_c1[0], lasso[0], logreg[0], other, fat[0], deadzone, on_c1[1], logreg[1], lasso[1], fat[1]]
    zone, logi, alone = (0, 5, 6), (2, 7), 3
    tall_only = [on_c1[0], logreg[0], other, deadzone, on_c1[1], logreg[1]]
    batch, tagsb, single, _ = rs.run_both(solve_mod, probs, dtype, ON, max_iterations=120)
    cb = rs.base_counts(tagsb)
    assert cb.get("batch_fused_pass", 0) > 0 and cb.get("batch_zero_pass", 0) > 0, sorted(cb)
    # the hinge member on another matrix runs alone on the single route, and it is the only one that
    # does; the deadzone member shares the hinge members' group (one x-side launch per sweep for the
    # three), the logistic pair forms its own (one sample launch per sweep for the two)
    assert cb.get("zero_tall") == cb.get("zero_tall_cols") == rs.sweeps(single[alone][0]), (cb, rs.sweeps(single[alone][0]))
    assert not [t for t in SINGLE_SWEEP[2:] if t in cb], sorted(cb)
    zone_sweeps = max(rs.sweeps(single[i][0]) for i in zone)
    logi_sweeps = max(rs.sweeps(single[i][0]) for i in logi)
    assert cb["batch_zero_tall_pass"] == zone_sweeps, (cb, zone_sweeps)
    assert cb["batch_zero_tall_dot"] == cb["batch_zero_tall_samples"] == cb["batch_zero_tall_acc"] == logi_sweeps, cb
    assert cb["batch_zero_tall_cols"] == zone_sweeps + logi_sweeps, cb
    rs.assert_identical(batch, single)

    for off in ("batch_zero_tall", "fused_zero_tall"):
        batch0, tags0, single0, _ = rs.run_both(solve_mod, tall_only, dtype, dict(ON, **{off: "0"}), max_iterations=120)
        assert not [t for t in rs.base_counts(tags0) if t.startswith("batch_zero_tall")], (off, sorted(tags0))
        rs.assert_identical(batch0, single0)


def members_fat():
    """a fat hinge pair on one matrix: a "batch_zero_pass" group beside the tall ones"""
    m, n = 256, 601
    return [problems.hinge_l1(m, n, lam=f * rs.lam_scale("hinge_l1", m, n))[0] for f in (0.2, 0.1)]
