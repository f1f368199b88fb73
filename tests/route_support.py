"""What the tests of the fused and batched routes share (`from tests import route_support as rs`):
decoding a status and counting launches, ONE scope that sets options and puts them back, ONE
profiled call, one solve-with-route and one solver handle built on the two, memoised problems and
oracle solves, and the assertions with their tolerances.  A test module keeps what it is about: its
shapes, its tags, which options its solves set, and its route checks.

`mod` is the ctypes binding (the session-scoped `solve_mod` fixture), so an option left set would
hold for every later test of the process: nothing here or in those modules calls set_option outside
`options`."""

import contextlib

import numpy as np
import pytest

from epsilon_amd import ir, problems, wire
from epsilon_amd.wire import ProxFunction
from oracle import epsilon_oracle as orc

# ---- decoding and counting -------------------------------------------------------------------------
STATUS_FIELDS = ("r_norm", "s_norm", "epsilon_primal", "epsilon_dual")
SETUP_WORDS = ("gemm", "syrk", "spd_inverse", "pack_inverse", "transpose_copy")


def status(st):
    return wire.SolverStatus.FromString(st)


def sweeps(st):
    """sweeps a solve ran: a check at iteration i follows sweep i (0-based), so a solve that the
    check at num_iterations ended ran one sweep more than one that ran into max_iterations"""
    s = status(st)
    return s.num_iterations + 1 if s.state == wire.SolverStatus.OPTIMAL else s.num_iterations


def base_counts(tags):
    """launch counts by tag name (the profile appends the shape: "name:AxB")"""
    out = {}
    for t, (c, _) in tags.items():
        out[t.split(":")[0]] = out.get(t.split(":")[0], 0) + c
    return out


def setup_counts(tags, words=SETUP_WORDS):
    """launch counts, by full tag, of what an Init forms once: Gram products, factorisations /
    explicit inverses, packed and transposed copies.  `words`: a module that counts fewer kinds
    passes its own list."""
    return {t: c for t, (c, _) in tags.items() if any(w in t for w in words)}


def union_data(probs):
    data = {}
    for p in probs:
        data.update(p.expression_data())
    return data


def arrays(x):
    """{variable: bytes} of a result as f64 arrays of their own"""
    return {k: np.frombuffer(v).copy() for k, v in x.items()}


# ---- one option scope --------------------------------------------------------------------------------
# The library's value of each option while nothing is set (csrc/options.cc: the `unset` word of the
# row; "fused" is on unless "0"; "refine" "auto" unsets; "dtype": capi.cc).  A test can set only what
# has a row here, so every option set has a stated way back.
DEFAULTS = {
    "dtype": "f32",
    "fused": "1",
    "fused_matrix": "auto",
    "fused_zero": "auto",
    "fused_zero_tall": "auto",
    "fused_zero_tall_smooth": "auto",
    "batch_zero_tall": "0",
    "refine": "auto",
}


@contextlib.contextmanager
def options(mod, **values):
    """Sets `values` in the order given; on every way out puts each key it set (or began to set)
    back to its default, last set first - callers name "dtype" first, so it is restored last.
    (Each key writes a variable of its own, opt::Set, so the order decides nothing.)"""
    unknown = sorted(k for k in values if k not in DEFAULTS)
    if unknown:
        raise KeyError("no default to put back for option(s) %s" % ", ".join(unknown))
    began = []
    try:
        for key, value in values.items():
            began.append(key)
            mod.set_option(key, value)
        yield
    finally:
        for key in reversed(began):
            mod.set_option(key, DEFAULTS[key])


def dtype_fixture(order, **also):
    """the `dtype` fixture of a module: its tests run once per entry of `order`, with the option
    (and `also`) set for the test"""
    @pytest.fixture(params=list(order))
    def dtype(request, solve_mod):
        with options(solve_mod, dtype=request.param, **also):
            yield request.param
    return dtype


# ---- one profiled call -------------------------------------------------------------------------------
def profiled(mod, fn):
    """(fn(), {tag: (count, ms)} of the launches it made)"""
    mod.profile_reset()
    mod.profile_enable(True)
    try:
        out = fn()
        return out, mod.profile_dump()
    finally:
        mod.profile_enable(False)


# ---- one solve with a route, one handle --------------------------------------------------------------
def switched_on(route_options):
    """{option: value} of the rows of a module's `route_options` that differ from the library's
    default: what its handles and batches set to be on the module's route"""
    return {key: value for _, key, value in route_options if value != DEFAULTS[key]}


class Routes(object):
    """Solves with a module's options set for one call and put back after it.  `route_options`:
    (argument name of `solve`, option, value unless given) in the order of the positional
    arguments after `dtype`.  `raw_tags`: return the profile's {tag: (count, ms)}, not base_counts
    of it."""

    def __init__(self, mod, route_options, raw_tags=False):
        self.mod, self.route_options, self.raw_tags = mod, tuple(route_options), raw_tags

    def solve(self, prob, dtype="f32", *words, **params):
        names = [name for name, _, _ in self.route_options]
        assert len(words) <= len(names) and not set(names[:len(words)]) & set(params), (words, sorted(params))
        params.update(zip(names, words))
        opts = {key: params.pop(name, value) for name, key, value in self.route_options}
        pb, data = prob.SerializeToString(), prob.expression_data()
        sb = wire.SolverParams(**params).SerializeToString()
        with options(self.mod, dtype=dtype, **opts):
            (st, x), tags = profiled(self.mod, lambda: self.mod.solve(pb, [], sb, data))
        return st, arrays(x), tags if self.raw_tags else base_counts(tags)


@contextlib.contextmanager
def handle(mod, prob, dtype, solver_params, **opts):
    """A solver handle with `opts` set, profiled from after its construction: Init reads the options,
    and the profile starts empty behind the constructor.  On every way out: profile off, close(),
    options back."""
    with options(mod, dtype=dtype, **opts):
        s = mod.Solver(prob.SerializeToString(), solver_params.SerializeToString(), prob.expression_data())
        try:
            mod.profile_reset()
            mod.profile_enable(True)
            yield s
        finally:
            mod.profile_enable(False)
            s.close()


def run_handle(mod, prob, dtype, splits, opts, **params):
    """one solve on a handle, run in pieces of `splits` sweeps: (status, arrays, base_counts)"""
    with handle(mod, prob, dtype, wire.SolverParams(**params), **opts) as s:
        s.init()
        for part in splits:
            assert s.run(part) == part
        c = base_counts(mod.profile_dump())
        st, x = s.result()
    return st, arrays(x), c


def run_both(mod, probs, dtype, opts, **params):
    """a batch and the single solves of its members under the same options: (batch, its tags,
    singles, the first single's tags)"""
    pbs, data = [p.SerializeToString() for p in probs], union_data(probs)
    sb = wire.SolverParams(**params).SerializeToString()
    with options(mod, dtype=dtype, **opts):
        batch, tagsb = profiled(mod, lambda: mod.solve_batch(pbs, None, sb, data))
        first, tags1 = profiled(mod, lambda: mod.solve(pbs[0], [], sb, data))
        single = [first] + [mod.solve(pb, [], sb, data) for pb in pbs[1:]]
    return batch, tagsb, single, tags1


# ---- memoised problems and oracle solves -------------------------------------------------------------
def memoised(builders):
    """make(kind, shape) over a module's own {kind: builder(*shape)}, each problem built once.  The
    memo belongs to the table: a kind name means what its module says."""
    made = {}

    def make(kind, shape):
        if (kind, shape) not in made:
            made[kind, shape] = builders[kind](*shape)
        return made[kind, shape]
    return make


def oracle_of(make):
    """oracle(kind, shape, **params): the CPU oracle's solve of make(kind, shape), computed once, as
    (decoded status, arrays)"""
    solved = {}

    def oracle(kind, shape, **params):
        key = (kind, shape, tuple(sorted(params.items())))
        if key not in solved:
            prob = make(kind, shape)
            st, x = orc.solve(prob.SerializeToString(), [], wire.SolverParams(**params).SerializeToString(),
                              prob.expression_data())
            solved[key] = (status(st), arrays(x))
        return solved[key]
    return oracle


# members of the ZERO-term batches
FRACS = (0.5, 0.2, 0.1, 0.05, 0.02)  # of the generators' own lambda scale (their default: 0.1)
DEADZONE_FRACS = (0.5, 0.3, 0.15)
_scale, _members = {}, {}


def lam_scale(kind, m, n):
    """what the generator multiplies by 0.1 for its default lambda"""
    if (kind, m, n) not in _scale:
        C = getattr(problems, kind)(m, n)[1]["C"]
        _scale[kind, m, n] = (np.abs(C.sum(axis=0)).max() if kind == "hinge_l1" else
                              np.abs(C.T.dot(np.full(m, 0.5))).max())
    return _scale[kind, m, n]


def members(kind, shape, count=None):
    """a path of one kind ("hinge", "logreg", "deadzone"; "bp": right-hand sides) on one matrix
    (seed 0); `count`: that many members, lambda falling by 0.8 from half the scale"""
    key = (kind, shape, count)
    if key not in _members:
        m, n = shape
        if kind == "deadzone":
            fr = DEADZONE_FRACS if count is None else [0.5 * 0.8 ** i for i in range(count)]
            _members[key] = [problems.deadzone_l1(m, n, frac=f)[0] for f in fr]
        elif kind == "bp":
            A, b = [problems.basis_pursuit(m, n)[1][k] for k in ("A", "b")]
            rng = np.random.RandomState(11)
            bs = [b] + [A.dot(rng.randn(n) * (rng.rand(n) < 0.2)) for _ in range((count or 4) - 1)]
            _members[key] = [problems.basis_pursuit(m, n, b=bi)[0] for bi in bs]
        else:
            gen = {"hinge": "hinge_l1", "logreg": "logreg_l1"}[kind]
            fr = FRACS if count is None else [0.5 * 0.8 ** i for i in range(count)]
            _members[key] = [getattr(problems, gen)(m, n, lam=f * lam_scale(gen, m, n))[0] for f in fr]
    return _members[key]


def lasso_pair(m, n, seed):
    A, b = problems.regression_data(m, n, seed=seed)
    lmax = np.abs(A.T.dot(b)).max()
    return [problems.lasso_ir(ir.dense_matrix(A), ir.constant(b), f * lmax, n) for f in (0.4, 0.2)]


def bind_b(b):
    """(parameters binding "param:b" to b, the data they need)"""
    data = {}
    c = ir.store(np.asarray(b, dtype=np.float64).reshape(-1, 1), data)
    return [("param:b", c.SerializeToString())], data


def fused_problem(Aexpr, m, n, b_expr, lam, kind, qvec=None):
    """sum_square(A x' - b) + lam * g(x)  s.t.  x' - x = 0 with g a scaled-zone function."""
    x = ir.variable(n, 1, problems.LASSO_COPY)
    y = ir.variable(n, 1, problems.LASSO_VAR)
    f0 = ir.prox(ProxFunction.SUM_SQUARE, ir.add(ir.linear_map(Aexpr, x),
                                                 ir.linear_map(ir.scalar(-1, m), b_expr)), alpha=1.0)
    if kind == "deadzone":
        f1 = ir.prox(ProxFunction.SUM_DEADZONE, ir.linear_map(ir.scalar(2.0, n), y), alpha=lam,
                     scaled_zone_params=wire.ProxScaledZoneParams(m=0.05))
    elif kind == "hinge":
        f1 = ir.prox(ProxFunction.SUM_HINGE, y, alpha=lam)
    else:  # quantile with per-column alpha / beta from data vectors
        assert kind == "quantile"
        qa, qb = ir.constant(qvec[0]), ir.constant(qvec[1])
        qd = dict(qa.data)
        qd.update(qb.data)
        f1 = ir.prox(ProxFunction.SUM_QUANTILE, y, alpha=lam, data=qd,
                     scaled_zone_params=wire.ProxScaledZoneParams(alpha_expr=qa.proto, beta_expr=qb.proto))
    return ir.Problem([f0, f1], [ir.zero(ir.add(x, ir.linear_map(ir.scalar(-1, n), y)))])


# ---- assertions ----------------------------------------------------------------------------------------
# against the CPU oracle, as in test_more_benchmark_problems (test_gpu_parity.py)
TOLERANCES = {"f64": dict(rtol=1e-6, atol=1e-8), "f32": dict(rtol=5e-3, atol=5e-3)}


def assert_close(x, xo, dtype):
    assert sorted(x) == sorted(xo), (sorted(x), sorted(xo))
    for k in xo:
        print(k, "max |gpu - oracle| %.3g, max |oracle| %.3g" % (np.abs(x[k] - xo[k]).max(), np.abs(xo[k]).max()))
    for k in xo:
        np.testing.assert_allclose(x[k], xo[k], err_msg=k, **TOLERANCES[dtype])


def assert_matches_oracle(st, x, so, xo, dtype):
    """equal state and stopping sweep, every variable within the tolerances of `dtype`"""
    sg = status(st)
    print("gpu: state %d at %d, r %.6g eps %.6g | oracle: state %d at %d, r %.6g eps %.6g" % (
        sg.state, sg.num_iterations, sg.residuals.r_norm, sg.residuals.epsilon_primal,
        so.state, so.num_iterations, so.residuals.r_norm, so.residuals.epsilon_primal))
    assert sg.state == so.state and sg.num_iterations == so.num_iterations, (sg, so)
    assert_close(x, xo, dtype)


def _raw(v):
    return v.tobytes() if isinstance(v, np.ndarray) else bytes(v)


def assert_same_arrays(x, x0, what=None):
    """the same variables with the same bytes; values are arrays or the bytes of a result"""
    assert sorted(x) == sorted(x0), (what, sorted(x), sorted(x0))
    for k in x0:
        assert _raw(x[k]) == _raw(x0[k]), (what, k)


def assert_same_bytes(st, x, st0, x0, what=None):
    """two solves: equal state and iteration, the same bytes in every variable"""
    p, q = status(st), status(st0)
    assert (p.state, p.num_iterations) == (q.state, q.num_iterations), (what, p, q)
    assert_same_arrays(x, x0, what)


def assert_same_bytes_and_residuals(a, b, what=None):
    """two results (status, variables): assert_same_bytes, and the four residual fields equal"""
    assert_same_bytes(a[0], a[1], b[0], b[1], what)
    p, q = status(a[0]), status(b[0])
    for f in STATUS_FIELDS:
        assert getattr(p.residuals, f) == getattr(q.residuals, f), (what, f)


def assert_identical(batch, single):
    """the contract of a batched solve: result k is what the single solve of member k returns -
    state, iteration, the four residual fields, every variable as f64 values"""
    assert len(batch) == len(single)
    for k, ((stb, xb), (sts, xs)) in enumerate(zip(batch, single)):
        a, s = status(stb), status(sts)
        assert a.state == s.state and a.num_iterations == s.num_iterations, (k, a, s)
        for f in STATUS_FIELDS:
            assert getattr(a.residuals, f) == getattr(s.residuals, f), (k, f)
        assert sorted(xb) == sorted(xs), (k, sorted(xb), sorted(xs))
        for v in xs:
            assert np.array_equal(np.frombuffer(xb[v]), np.frombuffer(xs[v])), (k, v)
