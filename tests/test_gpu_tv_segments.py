"""Segmented TV-1D prox (k::Tv1dSeg, kernels_tv3.hip): many signals with one lam in one pass,
through the C ABI (`tv1d_batch`), the operator (`eval_prox` with an axis) and the ADMM driver.

Reference: the DP oracle (oracle/c_oracle.tv1d) slice by slice, and the KKT certificate per
slice.  Tolerances are those of test_gpu_parity.test_tv1d_parallel_kernel, applied per slice:
f64 rtol = atol = 1e-9 and the KKT triple below 1e-7; f32 rtol = 1e-4, atol = 1e-4 max(1, max|v|)
of the slice, the input rounded to f32 first."""
import ctypes

import numpy as np
import pytest

# torch first: it carries its own HIP runtime, and the one that is loaded first in a process is
# the one every later library binds to (tests/test_gpu_full_size.py imports in the same order);
# it only provides the device buffers of the device entry's tests
torch = pytest.importorskip("torch")

from epsilon_amd import ir, problems, wire  # noqa: E402
from epsilon_amd.wire import ProxFunction  # noqa: E402
from oracle import epsilon_oracle as orc  # noqa: E402
from tests import route_support as rs  # noqa: E402
from tests.test_tv_segments_args import dykstra_tv2d, tv_slices  # noqa: E402

pytestmark = pytest.mark.gpu
dtype = rs.dtype_fixture(("f64", "f32"))


def as_dtype(V, dtype):
    return V.astype(np.float32).astype(np.float64) if dtype == "f32" else V


def check_slices(got, V, lam, dtype, axis=0):
    """Every slice of `got` against the DP of the same slice of V, and its KKT certificate."""
    want = tv_slices(V, lam, axis)
    assert got.shape == V.shape
    G, W, Vs = (got.T, want.T, V.T) if axis == 0 else (got, want, V)
    for k in range(G.shape[0]):
        if dtype == "f64":
            tol = dict(rtol=1e-9, atol=1e-9)
        else:
            tol = dict(rtol=1e-4, atol=1e-4 * max(1.0, np.abs(Vs[k]).max()))
        np.testing.assert_allclose(G[k], W[k], err_msg="slice %d" % k, **tol)
        if dtype == "f64":
            bound, jump, end = orc.tv1d_kkt_violation(G[k], Vs[k], lam)
            assert bound < 1e-7 and jump < 1e-7 and end < 1e-7, "slice %d" % k
    return want


def make_batch(kind, length, count, seed):
    """(V of shape (length, count): one signal per column, lam).  The columns cycle through four
    amplitudes, the first of them so small that the column comes out constant while the larger
    ones split many times under the same lam."""
    rng = np.random.RandomState(seed)
    if kind == "noise":
        V, lam = rng.randn(length, count), 0.7
    elif kind == "ties":
        V, lam = rng.randn(length, count) * 2, 1.0
    else:  # steps: plateaus of 20 samples plus a little noise
        base = rng.randn((length + 19) // 20, count)
        V, lam = np.repeat(base, 20, axis=0)[:length] + 0.1 * rng.randn(length, count), 3.0
    V = V * np.array([1e-4, 1.0, 5.0, 0.3])[np.arange(count) % 4]
    if kind == "ties":
        V = np.round(V)
    return V, lam


SHAPES = [(1, 5), (2, 3), (7, 300), (2048, 3), (2047, 5), (2049, 5), (300, 7), (5000, 130), (100000, 2)]


@pytest.mark.parametrize("kind", ["noise", "ties", "steps"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_slice_parity(solve_mod, dtype, shape, kind):
    """Check 1.  (1, 5) is the copy, (2, 3) a region of two samples, (7, 300) several heads per
    8-sample chunk at level 0, 2048 the tile length, 2047 / 2049 boundaries that drift through
    the tiles, (5000, 130) more than 256 tiles with heads in most of them, (100000, 2) two long
    slices."""
    length, count = shape
    V, lam = make_batch(kind, length, count, seed=length + count)
    V = as_dtype(V, dtype)
    got = solve_mod.tv1d_batch(V, lam, axis=0)
    check_slices(got, V, lam, dtype)
    if length == 1:
        assert np.array_equal(got, V)
    distinct = [len(np.unique(got[:, k])) for k in range(count)]
    if length >= 2:  # the quiet columns are constant ...
        assert any(np.ptp(got[:, k]) == 0 for k in range(count))
    if length >= 300:  # ... and a loud one has many pieces (a slice of 2 or 7 samples cannot)
        assert max(distinct) > 10


@pytest.mark.parametrize("shape", [(100, 4), (37, 6), (1100, 2)], ids=lambda s: "%dx%d" % s)
def test_no_coupling_across_boundaries(solve_mod, dtype, shape):
    """Check 2: slice k = noise + 1000 k, lam = 5.  A boundary term between neighbouring slices
    would move the ends of every slice by about lam.

    The shapes keep the sum over the whole batch near 10^6 or below: region means are differences
    of ONE fp64 prefix sum over the concatenation, whose values near P are spaced 2^-52 P apart, so
    a region of one or two samples behind a prefix of P = 2 10^7 (2049 x 5 with these offsets,
    spacing 3.7e-9) cannot meet atol = 1e-9 - measured there: 2 of 2049 samples of the slice with
    offset 0 off by 1.12e-9 when it comes last, everything else inside.  At P <= 1.1 10^6 the
    spacing is 2.3e-10.  (1100, 2) puts the boundary inside the first of two tiles; slice
    boundaries that move through many tiles are held by test_slice_parity."""
    length, count = shape
    rng = np.random.RandomState(5)
    V = as_dtype(rng.randn(length, count) + 1000.0 * np.arange(count), dtype)
    lam = 5.0
    got = solve_mod.tv1d_batch(V, lam, axis=0)
    check_slices(got, V, lam, dtype)
    # the same slices in the opposite order: the same result per slice (to the tolerance, not to
    # the bit: region means are differences of prefix sums over the whole batch)
    rev = solve_mod.tv1d_batch(V[:, ::-1], lam, axis=0)
    check_slices(rev, V[:, ::-1], lam, dtype)
    for k in range(count):
        tol = dict(rtol=1e-9, atol=1e-9) if dtype == "f64" else dict(rtol=1e-4, atol=1e-4 * np.abs(V[:, k]).max())
        np.testing.assert_allclose(rev[:, count - 1 - k], got[:, k], **tol)


@pytest.mark.parametrize("shape", [(300, 7), (5000, 130)], ids=lambda s: "%dx%d" % s)
def test_constant_batch_is_returned_exactly(solve_mod, dtype, shape):
    """Check 2, third item.  2.5 and its multiples are exact in both formats, so the prefix sums
    and with them every region mean are exact: the result is the input, bit for bit, and the
    recursion stops after the level that found no cut."""
    length, count = shape
    V = np.full((length, count), 2.5)
    assert np.array_equal(solve_mod.tv1d_batch(V, 3.0, axis=0), V)
    tdt = torch.float32 if dtype == "f32" else torch.float64
    v = torch.full((length * count,), 2.5, dtype=tdt, device="cuda:0")
    x = torch.zeros_like(v)
    torch.cuda.synchronize()
    lev = ctypes.c_int(-1)
    solve_mod._check(solve_mod.lib().eps_tv1d_batch_device(
        ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(x.data_ptr()), ctypes.c_size_t(length),
        ctypes.c_size_t(count), ctypes.c_int(1 if dtype == "f32" else 2), ctypes.c_double(3.0), ctypes.byref(lev)))
    assert lev.value == 1
    assert bool((x == v).all())


def test_device_entry_matches_host_entry(solve_mod, dtype):
    """eps_tv1d_batch_device on device pointers gives the bytes of eps_tv1d_batch, and reports
    the depth of the deepest slice."""
    V, lam = make_batch("steps", 2049, 5, seed=8)
    V = as_dtype(V, dtype)
    host = solve_mod.tv1d_batch(V, lam, axis=0)
    tdt = torch.float32 if dtype == "f32" else torch.float64
    v = torch.from_numpy(np.ascontiguousarray(V.T)).to(tdt).to("cuda:0")
    x = torch.zeros_like(v)
    torch.cuda.synchronize()
    lev = ctypes.c_int(-1)
    solve_mod._check(solve_mod.lib().eps_tv1d_batch_device(
        ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(x.data_ptr()), ctypes.c_size_t(2049), ctypes.c_size_t(5),
        ctypes.c_int(1 if dtype == "f32" else 2), ctypes.c_double(lam), ctypes.byref(lev)))
    assert np.array_equal(x.double().cpu().numpy().T, host)
    assert lev.value > 1


@pytest.mark.parametrize("shape", [(5000, 130), (7, 300)], ids=lambda s: "%dx%d" % s)
def test_run_to_run_identity(solve_mod, dtype, shape):
    """Check 3."""
    V, lam = make_batch("noise", shape[0], shape[1], seed=3)
    a = solve_mod.tv1d_batch(V, lam, axis=0)
    b = solve_mod.tv1d_batch(V, lam, axis=0)
    assert a.tobytes() == b.tobytes()


def eval_tv(solve_mod, expr, lam, V):
    got = solve_mod.eval_prox(expr.proto.SerializeToString(), lam, expr.data,
                              {"var:X": np.asarray(V, dtype=np.float64).tobytes(order="F")})
    assert set(got) == {"var:X"}
    return np.frombuffer(got["var:X"]).reshape(V.shape, order="F")


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("shape", [(12, 7), (7, 12), (40, 25), (1, 5), (5, 1), (300, 2100), (65, 130)],
                         ids=lambda s: "%dx%d" % s)
def test_axis_through_eval_prox(solve_mod, dtype, shape, axis):
    """Check 4: the operator with has_axis against the DP per column (axis 0) or per row (axis 1)
    of the column-major argument, to the tolerances test_eval_prox_vs_oracle uses for its tv_1d
    case.  (300, 2100) has only full 64 x 64 transpose tiles on one side and ragged ones on the
    other, (65, 130) ragged ones on both."""
    rows, cols = shape
    rng = np.random.RandomState(rows * 7 + cols)
    V = np.repeat(rng.randn(rows, (cols + 4) // 5), 5, axis=1)[:, :cols] + 0.5 * rng.randn(rows, cols)
    lam, alpha = 0.6, 1.5
    got = eval_tv(solve_mod, problems.tv_prox_expr(rows, cols, axis, lam_alpha=alpha), lam, V)
    want = tv_slices(V, lam * alpha, axis)
    tol = dict(rtol=1e-10, atol=1e-11) if dtype == "f64" else dict(rtol=5e-4, atol=5e-5)
    np.testing.assert_allclose(got, want, **tol)


@pytest.mark.parametrize("shape", [(300, 2100), (65, 130), (12, 7)], ids=lambda s: "%dx%d" % s)
def test_batch_axis1_is_axis0_of_the_transpose(solve_mod, dtype, shape):
    rng = np.random.RandomState(shape[0])
    V = rng.randn(*shape)
    a = solve_mod.tv1d_batch(V, 0.8, axis=1)
    b = solve_mod.tv1d_batch(V.T, 0.8, axis=0).T
    assert a.shape == V.shape and a.tobytes() == np.ascontiguousarray(b).tobytes()
    check_slices(a, as_dtype(V, dtype), 0.8, dtype, axis=1)


def test_unsegmented_operator_is_untouched(solve_mod, dtype):
    """Check 5.  lam = 1 keeps every scaling of eval_prox exactly 1, so the operator hands
    the prox the very input `tv1d` does."""
    rng = np.random.RandomState(2)
    V = rng.randn(40, 25)
    X = ir.variable(40, 25, "var:X")
    plain = eval_tv(solve_mod, ir.prox(ProxFunction.TOTAL_VARIATION_1D, X, alpha=0.75), 1.0, V)
    flat = solve_mod.tv1d(V.reshape(-1, order="F"), 0.75)
    assert plain.reshape(-1, order="F").tobytes() == flat.tobytes()
    cols = eval_tv(solve_mod, problems.tv_prox_expr(40, 25, 0, lam_alpha=0.75), 1.0, V)
    assert not np.array_equal(cols, plain)
    # the chain through all columns couples every column's last sample to the next one's first
    assert np.abs(cols - plain)[[0, -1], :].max() > 1e-3


def in_band(obj, opt):
    return obj <= opt * (1 + 1e-2) + 1e-4 and obj >= opt * (1 - 1e-6) - 1e-9


def solve(solve_mod, prob, **kw):
    st, x = solve_mod.solve(prob.SerializeToString(), [], wire.SolverParams(**kw).SerializeToString(),
                            prob.expression_data())
    return wire.SolverStatus.FromString(st), {k: np.frombuffer(v) for k, v in x.items()}


def test_column_tv_through_the_driver(solve_mod, dtype):
    """Check 6, first problem: 0.5 sum_square(X' - B) + lam TV_axis0(X) at (60, 9); the optimum
    is the DP of every column of B."""
    rows, cols, lam = 60, 9, 2.0
    rng = np.random.RandomState(6)
    B = np.repeat(3 * rng.randn(6, cols), 10, axis=0) + rng.randn(rows, cols)
    n = rows * cols
    Xs = ir.variable(rows, cols, "separate:var:X:sum_square")
    X = ir.variable(rows, cols, "var:X")
    f0 = ir.prox(ProxFunction.SUM_SQUARE,
                 ir.add(ir.reshape(Xs, n, 1), ir.linear_map(ir.scalar(-1, n), ir.constant(B.reshape(-1, 1, order="F")))),
                 alpha=0.5, arg_size=[(n, 1)])
    f1 = ir.prox(ProxFunction.TOTAL_VARIATION_1D, X, alpha=lam, has_axis=True, axis=0)
    c = ir.zero(ir.add(ir.reshape(Xs, n, 1), ir.linear_map(ir.scalar(-1, n), ir.reshape(X, n, 1))))
    S, x = solve(solve_mod, ir.Problem([f0, f1], [c]), max_iterations=3000)
    assert S.state == wire.SolverStatus.OPTIMAL

    def objective(Z):
        return float(0.5 * np.sum((Z - B) ** 2) + lam * np.abs(np.diff(Z, axis=0)).sum())
    obj = objective(x["var:X"].reshape((rows, cols), order="F"))
    opt = objective(tv_slices(B, lam, 0))
    print("column TV through the driver: obj %.9g opt %.9g iterations %d" % (obj, opt, S.num_iterations))
    assert in_band(obj, opt)


def test_tv_2d_through_the_driver(solve_mod, dtype):
    """Check 6, second problem: anisotropic 2-D TV as a three-term problem, against Dykstra's
    alternating prox with the DP per column and per row."""
    prob, info = problems.tv_2d(24, 40)
    S, x = solve(solve_mod, prob, max_iterations=3000)
    assert S.state == wire.SolverStatus.OPTIMAL
    B, lam = info["B"], info["lam"]
    obj = problems.tv_2d_objective(B, lam, x["var:X"].reshape((24, 40), order="F"))
    _, opt, it = dykstra_tv2d(B, lam, lam)
    print("tv_2d through the driver: obj %.9g opt %.9g (Dykstra, %d rounds) iterations %d"
          % (obj, opt, it, S.num_iterations))
    assert in_band(obj, opt)


def test_errors_are_raised_not_fatal(solve_mod):
    """Check 7.  The size limit is checked on the counts alone: the pointers are never read."""
    L = solve_mod.lib()
    small = np.zeros(8)
    p = small.ctypes.data_as(ctypes.c_void_p)
    for length, count in ((2 ** 20, 2 ** 11), (2 ** 31 - 1, 1), (3, 2 ** 30), (2 ** 40, 2 ** 40)):
        with pytest.raises(solve_mod.error, match="below 2\\^31"):
            solve_mod._check(L.eps_tv1d_batch(p, ctypes.c_size_t(length), ctypes.c_size_t(count),
                                              ctypes.c_double(1.0), p))
        with pytest.raises(solve_mod.error, match="below 2\\^31"):
            solve_mod._check(L.eps_tv1d_batch_device(p, p, ctypes.c_size_t(length), ctypes.c_size_t(count),
                                                     ctypes.c_int(1), ctypes.c_double(1.0), None))
    V = np.zeros((6, 4))
    X = ir.variable(6, 4, "var:X")
    bad_size = ir.prox(ProxFunction.TOTAL_VARIATION_1D, X, has_axis=True, axis=0, arg_size=[(5, 4)])
    with pytest.raises(solve_mod.error, match="arg_size"):
        eval_tv(solve_mod, bad_size, 1.0, V)
    bad_axis = ir.prox(ProxFunction.TOTAL_VARIATION_1D, X, has_axis=True, axis=2)
    with pytest.raises(solve_mod.error, match="axis"):
        eval_tv(solve_mod, bad_axis, 1.0, V)
    with pytest.raises(solve_mod.error, match="axis"):
        solve_mod.tv1d_batch(V, 1.0, axis=2)
    with pytest.raises(solve_mod.error, match="2-D"):
        solve_mod.tv1d_batch(np.zeros(5), 1.0)
    # the library is still usable afterwards
    assert np.array_equal(solve_mod.tv1d_batch(np.full((3, 2), 1.0), 1.0), np.full((3, 2), 1.0))


def device_levels(solve_mod, dtype, v, lam, length=None, count=None):
    """(x, levels) of eps_tv1d_device, or of eps_tv1d_batch_device when length / count are given,
    on a device copy of v."""
    L = solve_mod.lib()
    d = torch.from_numpy(np.ascontiguousarray(v)).to(torch.float32 if dtype == "f32" else torch.float64).to("cuda:0")
    x = torch.zeros_like(d)
    torch.cuda.synchronize()
    lev = ctypes.c_int(-1)
    kind = ctypes.c_int(1 if dtype == "f32" else 2)
    pv, px = ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(x.data_ptr())
    if length is None:
        solve_mod._check(L.eps_tv1d_device(pv, px, ctypes.c_size_t(d.numel()), kind, ctypes.c_double(lam),
                                           ctypes.byref(lev)))
    else:
        solve_mod._check(L.eps_tv1d_batch_device(pv, px, ctypes.c_size_t(length), ctypes.c_size_t(count), kind,
                                                 ctypes.c_double(lam), ctypes.byref(lev)))
    return x.cpu().numpy(), d.cpu().numpy(), lev.value


def noisy_steps(n, seed):
    rng = np.random.RandomState(seed)
    return np.repeat(2.0 * rng.randn((n + 19) // 20), 20)[:n] + 0.3 * rng.randn(n)


@pytest.mark.parametrize("n", [2, 63, 65, 2049, 524289])
def test_single_signal_is_a_batch_of_one(solve_mod, dtype, n):
    """One signal is the segmented prox with one slice: `tv1d`, a one-column batch and a one-row
    batch give the same bytes, and the single and the batch device entry report the same depth.
    63 and 65 straddle the width of the init kernel's lane group, 2049 is one tile plus a sample,
    524289 the first size with more than 256 tiles (aggregate scans as launches of their own)."""
    v, lam = noisy_steps(n, seed=n), 1.5
    one = solve_mod.tv1d(v, lam)
    col = solve_mod.tv1d_batch(v[:, None], lam, axis=0)
    row = solve_mod.tv1d_batch(v[None, :], lam, axis=1)
    assert col.shape == (n, 1) and row.shape == (1, n)
    assert one.tobytes() == col.tobytes() == row.tobytes()
    xs, _, lev_single = device_levels(solve_mod, dtype, v, lam)
    xb, _, lev_batch = device_levels(solve_mod, dtype, v, lam, length=n, count=1)
    assert xs.tobytes() == xb.tobytes() == one.astype(xs.dtype).tobytes()
    assert lev_single == lev_batch and lev_single >= 1


def test_trivial_calls_report_depth_zero(solve_mod, dtype):
    """The depth belongs to the call: lam = 0 and n = 1 are copies and report 0 levels, whatever
    the call before them reported."""
    v = noisy_steps(300, seed=4)
    _, _, lev = device_levels(solve_mod, dtype, v, 1.5)
    assert lev >= 1
    x, d, lev = device_levels(solve_mod, dtype, v, 0.0)
    assert lev == 0 and np.array_equal(x, d)
    _, _, lev = device_levels(solve_mod, dtype, v, 1.5)
    assert lev >= 1
    x, d, lev = device_levels(solve_mod, dtype, v[:1], 1.5)
    assert lev == 0 and np.array_equal(x, d)
