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

pytestmark = pytest.mark.gpu

FRACS = (0.5, 0.2, 0.1, 0.05, 0.02)  # of the generators' own lambda scale (their default: 0.1)
DEADZONE_FRACS = (0.5, 0.3, 0.15)
STATUS_FIELDS = ("r_norm", "s_norm", "epsilon_primal", "epsilon_dual")
FIXED = dict(abs_tol=0.0, rel_tol=0.0)
# what a sweep of the single tall route launches ("zero_tall_head" is an Init launch of a logistic
# member, in a group as alone)
SINGLE_SWEEP = ("zero_tall", "zero_tall_cols", "zero_tall_dot", "zero_tall_samples", "zero_tall_acc")
ZONE_GROUP = ("batch_zero_tall_pass", "batch_zero_tall_cols")
LOGISTIC_GROUP = ("batch_zero_tall_dot", "batch_zero_tall_samples", "batch_zero_tall_acc", "batch_zero_tall_cols")


def status(st):
    return wire.SolverStatus.FromString(st)


def sweeps(st):
    s = status(st)
    return s.num_iterations + 1 if s.state == wire.SolverStatus.OPTIMAL else s.num_iterations


def union_data(probs):
    data = {}
    for p in probs:
        data.update(p.expression_data())
    return data


def assert_identical(batch, single):
    assert len(batch) == len(single)
    for k, ((stb, xb), (sts, xs)) in enumerate(zip(batch, single)):
        a, s = status(stb), status(sts)
        assert a.state == s.state and a.num_iterations == s.num_iterations, (k, a, s)
        for f in STATUS_FIELDS:
            assert getattr(a.residuals, f) == getattr(s.residuals, f), (k, f)
        assert sorted(xb) == sorted(xs)
        for v in xs:
            assert np.array_equal(np.frombuffer(xb[v]), np.frombuffer(xs[v])), (k, v)


def tags_of(solve_mod, fn):
    solve_mod.profile_reset()
    solve_mod.profile_enable(True)
    try:
        out = fn()
        return out, solve_mod.profile_dump()
    finally:
        solve_mod.profile_enable(False)


def base_counts(tags):
    """launch counts by tag name (the profile appends the shape: "name:AxB")"""
    out = {}
    for t, (c, _) in tags.items():
        out[t.split(":")[0]] = out.get(t.split(":")[0], 0) + c
    return out


def setup_counts(tags):
    """Gram products, factorisations / explicit inverses, packed and transposed copies of an Init"""
    return {t: c for t, (c, _) in tags.items()
            if any(w in t for w in ("gemm", "syrk", "spd_inverse", "pack_inverse", "transpose_copy"))}


_scale = {}


def lam_scale(kind, m, n):
    """what the generator multiplies by 0.1 for its default lambda"""
    if (kind, m, n) not in _scale:
        C = getattr(problems, kind)(m, n)[1]["C"]
        _scale[kind, m, n] = (np.abs(C.sum(axis=0)).max() if kind == "hinge_l1" else
                              np.abs(C.T.dot(np.full(m, 0.5))).max())
    return _scale[kind, m, n]


_members = {}


def members(kind, shape, count=None):
    """a path of one kind on one matrix (seed 0); `count`: that many members, lambda falling by 0.8
    from half the scale"""
    key = (kind, shape, count)
    if key not in _members:
        m, n = shape
        if kind == "deadzone":
            fr = DEADZONE_FRACS if count is None else [0.5 * 0.8 ** i for i in range(count)]
            _members[key] = [problems.deadzone_l1(m, n, frac=f)[0] for f in fr]
        else:
            gen = "hinge_l1" if kind == "hinge" else "logreg_l1"
            fr = FRACS if count is None else [0.5 * 0.8 ** i for i in range(count)]
            _members[key] = [getattr(problems, gen)(m, n, lam=f * lam_scale(gen, m, n))[0] for f in fr]
    return _members[key]


class Options(object):
    """the options of a call, put back after it"""

    ON = (("batch_zero_tall", "1", "0"), ("fused_zero_tall", "1", "auto"), ("fused_zero_tall_smooth", "1", "auto"))

    def __init__(self, mod, dtype, **other):
        self.mod, self.dtype, self.other = mod, dtype, other

    def __enter__(self):
        self.mod.set_option("dtype", self.dtype)
        for key, on, _ in self.ON:
            self.mod.set_option(key, self.other.get(key, on))

    def __exit__(self, *exc):
        for key, _, default in self.ON:
            self.mod.set_option(key, default)
        self.mod.set_option("dtype", "f32")


def run_both(solve_mod, probs, dtype, options=None, **params):
    """(batch, its tags, singles, the first single's tags); `options`: values other than "1" """
    pbs, data = [p.SerializeToString() for p in probs], union_data(probs)
    sb = wire.SolverParams(**params).SerializeToString()
    with Options(solve_mod, dtype, **(options or {})):
        batch, tagsb = tags_of(solve_mod, lambda: solve_mod.solve_batch(pbs, None, sb, data))
        first, tags1 = tags_of(solve_mod, lambda: solve_mod.solve(pbs[0], [], sb, data))
        single = [first] + [solve_mod.solve(pb, [], sb, data) for pb in pbs[1:]]
    return batch, tagsb, single, tags1


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
    batch, tagsb, single, _ = run_both(solve_mod, members(kind, shape), dtype, max_iterations=max_it)
    st = [status(s) for s, _ in single]
    print(kind, shape, dtype, [(s.state, s.num_iterations) for s in st])
    assert len({s.num_iterations for s in st}) >= 2
    if kind != "deadzone":
        assert wire.SolverStatus.MAX_ITERATIONS_REACHED in [s.state for s in st]
    cb = base_counts(tagsb)
    assert all(cb.get(t, 0) > 0 for t in group_tags(kind)), sorted(cb)
    assert not [t for t in SINGLE_SWEEP if t in cb], sorted(cb)
    assert_identical(batch, single)


# ---- 2. launch counts and the shared setup --------------------------------------------------------
@pytest.mark.parametrize("dt,kind,k,widths", [("f32", "hinge", 5, {"pass": 8}),
                                              ("f64", "logreg", 7, {"dot": 12, "acc": 12})])
def test_launch_counts_and_shared_setup(solve_mod, dt, kind, k, widths):
    """Widths of the tall chains per (chunks per thread, dtype): DESIGN.md 3.6 (n = 1028 is two
    16-byte chunks per thread in f32, chain 3: width 8; three, run as four, in f64, chains 4 and 5:
    width 12)."""
    shape, n_sweeps = (2051, 1028), 60
    batch, tagsb, single, tags1 = run_both(solve_mod, members(kind, shape, k), dt, max_iterations=n_sweeps, **FIXED)
    assert all(sweeps(st) == n_sweeps for st, _ in batch)
    c1, cb = base_counts(tags1), base_counts(tagsb)
    first_pass = "zero_tall" if kind == "hinge" else "zero_tall_dot"
    assert c1.get(first_pass) == n_sweeps and c1.get("zero_tall_cols") == n_sweeps, sorted(c1)
    assert not [t for t in SINGLE_SWEEP if t in cb], sorted(cb)
    for half, width in widths.items():
        assert cb.get("batch_zero_tall_" + half) == n_sweeps * math.ceil(k / width), (half, cb)
    assert cb.get("batch_zero_tall_cols") == n_sweeps and cb.get("batch_symv_packed") == n_sweeps, cb
    assert cb.get("batch_zero_tall_samples", 0) == (n_sweeps if kind == "logreg" else 0), cb
    s1, sb = setup_counts(tags1), setup_counts(tagsb)
    assert any("pack_inverse" in t for t in s1) and any("spd_inverse" in t for t in s1), sorted(tags1)
    assert sb == s1, (s1, sb)
    assert base_counts(tags1).get("transpose_copy") == 1 and cb.get("transpose_copy") == 1, (sorted(c1), sorted(cb))
    assert_identical(batch, single)


# ---- 3. more members than one launch holds --------------------------------------------------------
def test_more_members_than_one_launch_holds(solve_mod):
    """f32 at one chunk per thread: chain 3 has width 8, so 9 members are launches
    of 8 and 1"""
    k, n_sweeps = 9, 30
    batch, tagsb, single, _ = run_both(solve_mod, members("hinge", (601, 256), k), "f32", max_iterations=n_sweeps,
                                       **FIXED)
    cb = base_counts(tagsb)
    assert cb.get("batch_zero_tall_pass") == 2 * n_sweeps and cb.get("batch_zero_tall_cols") == n_sweeps, cb
    assert_identical(batch, single)


# ---- 4. against the CPU oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hinge", "logreg"])
def test_batch_matches_the_oracle_f64(solve_mod, kind):
    probs = members(kind, (601, 256))[:3]
    pbs, data = [p.SerializeToString() for p in probs], union_data(probs)
    sb = wire.SolverParams(max_iterations=60, **FIXED).SerializeToString()
    with Options(solve_mod, "f64"):
        batch, tagsb = tags_of(solve_mod, lambda: solve_mod.solve_batch(pbs, None, sb, data))
    cb = base_counts(tagsb)
    assert all(cb.get(t) == 60 for t in group_tags(kind)), sorted(cb)
    for pb, (stb, xb) in zip(pbs, batch):
        sto, xo = orc.solve(pb, [], sb, data)
        a, o = status(stb), status(sto)
        assert a.state == o.state and a.num_iterations == o.num_iterations
        assert sorted(xb) == sorted(xo)
        for v in xo:
            np.testing.assert_allclose(np.frombuffer(xb[v]), np.frombuffer(xo[v]), rtol=1e-6, atol=1e-8, err_msg=v)


# ---- 5. a mixed batch, and the group switched off ---------------------------------------------------
def lasso_pair(m, n, seed):
    A, b = problems.regression_data(m, n, seed=seed)
    lmax = np.abs(A.T.dot(b)).max()
    return [problems.lasso_ir(ir.dense_matrix(A), ir.constant(b), f * lmax, n) for f in (0.4, 0.2)]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_mixed_batch_and_fallbacks(solve_mod, dtype):
    shape = (601, 256)
    m, n = shape
    on_c1 = members("hinge", shape)[1:3]
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
    lasso = lasso_pair(300, 700, seed=6)
    probs = [on_c1[0], lasso[0], logreg[0], other, fat[0], deadzone, on_c1[1], logreg[1], lasso[1], fat[1]]
    zone, logi, alone = (0, 5, 6), (2, 7), 3
    tall_only = [on_c1[0], logreg[0], other, deadzone, on_c1[1], logreg[1]]
    batch, tagsb, single, _ = run_both(solve_mod, probs, dtype, max_iterations=120)
    cb = base_counts(tagsb)
    assert cb.get("batch_fused_pass", 0) > 0 and cb.get("batch_zero_pass", 0) > 0, sorted(cb)
    # the hinge member on another matrix runs alone on the single route, and it is the only one that
    # does; the deadzone member shares the hinge members' group (one x-side launch per sweep for the
    # three), the logistic pair forms its own (one sample launch per sweep for the two)
    assert cb.get("zero_tall") == cb.get("zero_tall_cols") == sweeps(single[alone][0]), (cb, sweeps(single[alone][0]))
    assert not [t for t in SINGLE_SWEEP[2:] if t in cb], sorted(cb)
    zone_sweeps = max(sweeps(single[i][0]) for i in zone)
    logi_sweeps = max(sweeps(single[i][0]) for i in logi)
    assert cb["batch_zero_tall_pass"] == zone_sweeps, (cb, zone_sweeps)
    assert cb["batch_zero_tall_dot"] == cb["batch_zero_tall_samples"] == cb["batch_zero_tall_acc"] == logi_sweeps, cb
    assert cb["batch_zero_tall_cols"] == zone_sweeps + logi_sweeps, cb
    assert_identical(batch, single)

    for off in ("batch_zero_tall", "fused_zero_tall"):
        batch0, tags0, single0, _ = run_both(solve_mod, tall_only, dtype, options={off: "0"}, max_iterations=120)
        assert not [t for t in base_counts(tags0) if t.startswith("batch_zero_tall")], (off, sorted(tags0))
        assert_identical(batch0, single0)


def members_fat():
    """a fat hinge pair on one matrix: a "batch_zero_pass" group beside the tall ones"""
    m, n = 256, 601
    return [problems.hinge_l1(m, n, lam=f * lam_scale("hinge_l1", m, n))[0] for f in (0.2, 0.1)]
