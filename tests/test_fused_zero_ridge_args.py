"""The "fused_zero_ridge" option (include/epsilon_hip.h eps_set_option): the fused sweep of ZERO-term
problems whose term on x is a ridge penalty.  Checks that fail before any device work: they need the
built library, not a GPU."""

import ctypes
import os

import pytest

from epsilon_amd import _solve


@pytest.fixture(scope="module")
def lib_built():
    if not os.path.exists(_solve.LIB_PATH):
        pytest.fail("libepsilon_hip.so is not built")
    return _solve


def stored(name="EPSILON_HIP_FUSED_ZERO_RIDGE"):
    """the option as the library reads it: the process environment"""
    libc = ctypes.CDLL(None)
    libc.getenv.restype = ctypes.c_char_p
    libc.getenv.argtypes = [ctypes.c_char_p]
    v = libc.getenv(name.encode())
    return None if v is None else v.decode()


@pytest.fixture
def option_auto(lib_built):
    _solve.set_option("fused_zero_ridge", "auto")
    yield
    _solve.set_option("fused_zero_ridge", "auto")


@pytest.mark.parametrize("value", ["0", "1", "auto"])
def test_option_accepts_the_three_values(option_auto, value):
    _solve.set_option("fused_zero_ridge", value)
    assert stored() == value


@pytest.mark.parametrize("value,text", [(0, "0"), (1, "1")])
def test_option_accepts_numbers(option_auto, value, text):
    _solve.set_option("fused_zero_ridge", value)
    assert stored() == text


@pytest.mark.parametrize("value", ["2", "on", "Auto", "", "pass"])
def test_option_rejects_other_values_by_name(option_auto, value):
    _solve.set_option("fused_zero_ridge", "0")
    with pytest.raises(_solve.error, match="fused_zero_ridge must be 0, 1 or auto, got %s" % value):
        _solve.set_option("fused_zero_ridge", value)
    assert stored() == "0"


def test_the_other_zero_options_keep_their_values(option_auto):
    """the new option leaves "fused_zero" and "fused_zero_tall", their values and error texts as they were"""
    for key, name, words, bad in (("fused_zero", "EPSILON_HIP_FUSED_ZERO", "0 or auto", "1"),
                                  ("fused_zero_tall", "EPSILON_HIP_FUSED_ZERO_TALL", "0, 1 or auto", "2")):
        _solve.set_option(key, "auto")
        try:
            with pytest.raises(_solve.error, match="%s must be %s, got %s" % (key, words, bad)):
                _solve.set_option(key, bad)
            assert stored(name) == "auto"
        finally:
            _solve.set_option(key, "auto")
