"""The "fused_zero_tall_smooth" option (include/epsilon_hip.h eps_set_option): the fused sweep of tall
ZERO-term problems whose z term is smooth (l1 logistic regression with more rows than columns).
Checks that fail before any device work: they need the built library, not a GPU."""

import ctypes

import pytest

from epsilon_amd import _solve

OPTION, VARIABLE = "fused_zero_tall_smooth", "EPSILON_HIP_FUSED_ZERO_TALL_SMOOTH"


@pytest.fixture(scope="module")
def lib_built():
    import os
    if not os.path.exists(_solve.LIB_PATH):
        pytest.fail("libepsilon_hip.so is not built")
    return _solve


def stored(name=VARIABLE):
    """the option as the library reads it: the process environment"""
    libc = ctypes.CDLL(None)
    libc.getenv.restype = ctypes.c_char_p
    libc.getenv.argtypes = [ctypes.c_char_p]
    v = libc.getenv(name.encode())
    return None if v is None else v.decode()


@pytest.fixture
def option_auto(lib_built):
    _solve.set_option(OPTION, "auto")
    yield
    _solve.set_option(OPTION, "auto")


@pytest.mark.parametrize("value", ["0", "1", "auto"])
def test_option_accepts_the_three_values(option_auto, value):
    _solve.set_option(OPTION, value)
    assert stored() == value


@pytest.mark.parametrize("value,text", [(0, "0"), (1, "1")])
def test_option_accepts_numbers(option_auto, value, text):
    _solve.set_option(OPTION, value)
    assert stored() == text


@pytest.mark.parametrize("value", ["2", "on", "Auto", "", "pass"])
def test_option_rejects_other_values_by_name(option_auto, value):
    _solve.set_option(OPTION, "0")
    with pytest.raises(_solve.error, match="fused_zero_tall_smooth must be 0, 1 or auto, got %s" % value):
        _solve.set_option(OPTION, value)
    assert stored() == "0"


def test_fused_zero_tall_keeps_its_values_and_text(option_auto):
    """the new option leaves "fused_zero_tall", its variable and its error text as they were"""
    _solve.set_option("fused_zero_tall", "auto")
    try:
        _solve.set_option(OPTION, "1")
        assert stored("EPSILON_HIP_FUSED_ZERO_TALL") == "auto"
        with pytest.raises(_solve.error, match="fused_zero_tall must be 0, 1 or auto, got pass"):
            _solve.set_option("fused_zero_tall", "pass")
        assert stored("EPSILON_HIP_FUSED_ZERO_TALL") == "auto" and stored() == "1"
    finally:
        _solve.set_option("fused_zero_tall", "auto")
