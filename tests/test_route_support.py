"""tests/route_support.py decides pass or fail for the tests of the fused and batched routes, so its
scopes and assertions are tested here, on the CPU, against a stub of the binding that records the
set_option / profile_* calls and raises where it is told to."""

import numpy as np
import pytest

from epsilon_amd import wire
from tests import route_support as rs


class Boom(Exception):
    pass


class StubSolver(object):
    def __init__(self, mod):
        self.mod = mod

    def init(self):
        self.mod.call("init")

    def close(self):
        self.mod.call("close")


class StubMod(object):
    """records every call as a tuple; raises Boom at the calls listed in `fail`"""

    def __init__(self, *fail):
        self.calls, self.fail = [], fail

    def call(self, *what):
        self.calls.append(what)
        if what in self.fail:
            raise Boom(what)

    def set_option(self, key, value):
        self.call("set_option", key, value)

    def profile_reset(self):
        self.call("profile_reset")

    def profile_enable(self, on):
        self.call("profile_enable", on)

    def profile_dump(self):
        return {"a:3x4": (2, 0.5)}

    def Solver(self, pb, sb, data):
        self.call("Solver")
        return StubSolver(self)

    def options_now(self):
        """the value every option holds after the recorded calls"""
        now = dict(rs.DEFAULTS)
        now.update({c[1]: c[2] for c in self.calls if c[0] == "set_option"})
        return now

    def profile_is_on(self):
        return [c[1] for c in self.calls if c[0] == "profile_enable"][-1]


class StubMessage(object):
    def SerializeToString(self):
        return b""

    def expression_data(self):
        return {}


# ---- options ---------------------------------------------------------------------------------------
def test_options_sets_in_order_and_restores_last_first():
    mod = StubMod()
    with rs.options(mod, dtype="f64", fused_zero_tall="1", fused="0"):
        assert mod.options_now() == dict(rs.DEFAULTS, dtype="f64", fused_zero_tall="1", fused="0")
    assert [c[1:] for c in mod.calls] == [("dtype", "f64"), ("fused_zero_tall", "1"), ("fused", "0"),
                                          ("fused", "1"), ("fused_zero_tall", "auto"), ("dtype", "f32")]


def test_options_restores_when_the_body_raises():
    mod = StubMod()
    with pytest.raises(Boom):
        with rs.options(mod, dtype="f64", batch_zero_tall="1"):
            raise Boom()
    assert mod.options_now() == rs.DEFAULTS


def test_options_restores_when_a_later_set_raises():
    mod = StubMod(("set_option", "fused_zero_tall", "1"))
    with pytest.raises(Boom):
        with rs.options(mod, dtype="f64", fused_zero="0", fused_zero_tall="1", fused="0"):
            pytest.fail("the body must not run")
    assert mod.options_now() == rs.DEFAULTS
    assert ("set_option", "fused", "0") not in mod.calls
    # the key whose set raised is put back too: the library may have taken the value before it threw
    assert mod.calls[-3:] == [("set_option", "fused_zero_tall", "auto"), ("set_option", "fused_zero", "auto"),
                              ("set_option", "dtype", "f32")]


def test_options_refuses_a_key_without_a_default():
    mod = StubMod()
    with pytest.raises(KeyError, match="fused_resident"):
        with rs.options(mod, dtype="f64", fused_resident="0"):
            pytest.fail("the body must not run")
    assert mod.calls == []


def test_switched_on_names_what_differs_from_the_default():
    rows = (("smooth", "fused_zero_tall_smooth", "1"), ("fused", "fused", "1"), ("route", "fused_zero", "auto"))
    assert rs.switched_on(rows) == {"fused_zero_tall_smooth": "1"}


# ---- profiled, handle ------------------------------------------------------------------------------
def test_profiled_returns_the_tags_and_disables_when_fn_raises():
    mod = StubMod()
    assert rs.profiled(mod, lambda: 7) == (7, {"a:3x4": (2, 0.5)})
    assert mod.calls == [("profile_reset",), ("profile_enable", True), ("profile_enable", False)]

    def fn():
        raise Boom()
    mod = StubMod()
    with pytest.raises(Boom):
        rs.profiled(mod, fn)
    assert mod.profile_is_on() is False


def test_handle_order_of_entry_and_exit():
    mod = StubMod()
    with rs.handle(mod, StubMessage(), "f64", StubMessage(), fused_zero_tall="1") as s:
        s.init()
    assert mod.calls == [("set_option", "dtype", "f64"), ("set_option", "fused_zero_tall", "1"), ("Solver",),
                         ("profile_reset",), ("profile_enable", True), ("init",), ("profile_enable", False),
                         ("close",), ("set_option", "fused_zero_tall", "auto"), ("set_option", "dtype", "f32")]


def test_handle_closes_and_restores_when_init_raises():
    mod = StubMod(("init",))
    with pytest.raises(Boom):
        with rs.handle(mod, StubMessage(), "f64", StubMessage(), fused_zero_tall="1") as s:
            s.init()
    assert ("close",) in mod.calls and mod.profile_is_on() is False
    assert mod.options_now() == rs.DEFAULTS


def test_handle_restores_when_the_constructor_raises():
    mod = StubMod(("Solver",))
    with pytest.raises(Boom):
        with rs.handle(mod, StubMessage(), "f64", StubMessage(), fused_zero_tall="1"):
            pytest.fail("the body must not run")
    assert mod.options_now() == rs.DEFAULTS
    assert ("close",) not in mod.calls and ("profile_enable", True) not in mod.calls


# ---- decoding and counting -------------------------------------------------------------------------
def result(state=wire.SolverStatus.OPTIMAL, num_iterations=40, x=(1.0, -2.0, 0.0), **residuals):
    """(status bytes, {variable: bytes}) as the binding returns them"""
    r = dict(r_norm=0.25, s_norm=0.125, epsilon_primal=0.5, epsilon_dual=0.75)
    r.update(residuals)
    st = wire.SolverStatus(state=state, num_iterations=num_iterations, residuals=wire.Residuals(**r))
    return st.SerializeToString(), {"var:x": np.asarray(x, dtype=np.float64).tobytes(), "var:z": b"\0" * 16}


def test_sweeps_counts_the_sweep_before_the_stopping_check():
    assert rs.sweeps(result(wire.SolverStatus.OPTIMAL, 40)[0]) == 41
    assert rs.sweeps(result(wire.SolverStatus.MAX_ITERATIONS_REACHED, 40)[0]) == 40


def test_counts_fold_the_shape_suffix():
    tags = {"a:3x4": (2, 0.1), "a:5x6": (3, 0.1), "gemm:7x7": (1, 0.2), "pack_inverse:7": (4, 0.3), "b": (5, 0.0)}
    assert rs.base_counts(tags) == {"a": 5, "gemm": 1, "pack_inverse": 4, "b": 5}
    assert rs.setup_counts(tags) == {"gemm:7x7": 1, "pack_inverse:7": 4}
    assert rs.setup_counts(tags, ("gemm", "syrk")) == {"gemm:7x7": 1}


def test_arrays_are_copies():
    st, x = result()
    a = rs.arrays(x)
    assert a["var:x"].tolist() == [1.0, -2.0, 0.0] and a["var:x"].flags.writeable


# ---- assertions ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,rtol,atol", [("f64", 1e-6, 1e-8), ("f32", 5e-3, 5e-3)])
def test_assert_close_holds_the_tolerance_of_the_dtype(dtype, rtol, atol):
    ref = np.array([0.0, 1.0, -3.0])
    tol = atol + rtol * np.abs(ref)
    rs.assert_close({"v": ref + np.array([atol, 0.999 * tol[1], -0.999 * tol[2]])}, {"v": ref}, dtype)  # [0]: exactly at it
    for i, off in enumerate([np.nextafter(atol, 1.0), 1.001 * tol[1], -1.001 * tol[2]]):
        x = ref.copy()
        x[i] += off
        with pytest.raises(AssertionError):
            rs.assert_close({"v": x}, {"v": ref}, dtype)


def test_assert_close_fails_on_a_missing_key_and_an_unknown_dtype():
    ref = {"v": np.zeros(2), "w": np.zeros(2)}
    with pytest.raises(AssertionError):
        rs.assert_close({"v": np.zeros(2)}, ref, "f64")
    with pytest.raises(AssertionError):
        rs.assert_close(dict(ref, u=np.zeros(2)), ref, "f64")
    with pytest.raises(KeyError):
        rs.assert_close(ref, ref, "f16")


def test_assert_matches_oracle_compares_state_and_stopping_sweep():
    st, x = result()
    so, xo = rs.status(st), rs.arrays(x)
    rs.assert_matches_oracle(st, rs.arrays(x), so, xo, "f64")
    for other in (result(num_iterations=50), result(state=wire.SolverStatus.MAX_ITERATIONS_REACHED)):
        with pytest.raises(AssertionError):
            rs.assert_matches_oracle(other[0], rs.arrays(x), so, xo, "f64")


ONE_ULP_OFF = [result(x=(np.nextafter(1.0, 2.0), -2.0, 0.0))] + [
    result(**{f: np.nextafter(result_value, 1.0)})
    for f, result_value in (("r_norm", 0.25), ("s_norm", 0.125), ("epsilon_primal", 0.5), ("epsilon_dual", 0.75))]


def test_bit_identity_checks_pass_on_equal_results():
    a, b = result(), result()
    rs.assert_identical([a, a], [b, b])
    rs.assert_same_bytes_and_residuals(a, b)
    rs.assert_same_bytes(a[0], rs.arrays(a[1]), b[0], rs.arrays(b[1]))
    rs.assert_same_arrays(a[1], rs.arrays(b[1]))  # bytes of a result against arrays


@pytest.mark.parametrize("other", ONE_ULP_OFF, ids=["value", "r_norm", "s_norm", "epsilon_primal", "epsilon_dual"])
def test_one_ulp_fails_the_bit_identity_checks(other):
    a = result()
    with pytest.raises(AssertionError):
        rs.assert_identical([a, a], [a, other])
    with pytest.raises(AssertionError):
        rs.assert_same_bytes_and_residuals(a, other)


def test_same_bytes_fails_on_values_state_iteration_and_keys():
    a = result()
    with pytest.raises(AssertionError):
        rs.assert_same_bytes(a[0], a[1], *ONE_ULP_OFF[0])
    with pytest.raises(AssertionError):
        rs.assert_same_arrays(rs.arrays(a[1]), rs.arrays(ONE_ULP_OFF[0][1]))
    for other in (result(num_iterations=41), result(state=wire.SolverStatus.MAX_ITERATIONS_REACHED)):
        with pytest.raises(AssertionError):
            rs.assert_same_bytes(a[0], a[1], *other)
    with pytest.raises(AssertionError):
        rs.assert_same_arrays(a[1], {"var:x": a[1]["var:x"]})
    with pytest.raises(AssertionError):
        rs.assert_identical([a], [a, a])
