"""The "fused_zero" option (include/epsilon_hip.h eps_set_option): the fused sweep of ZERO-term
problems.  Checks that fail before any device work: they need the built library, not a GPU."""

import ctypes

import pytest

from epsilon_amd import _solve


@pytest.fixture(scope="module")
def lib_built():
    import os
    if not os.path.exists(_solve.LIB_PATH):
        pytest.fail("libepsilon_hip.so is not built")
    return _solve


def stored():
    """the option as the library reads it: the process environment"""
    libc = ctypes.CDLL(None)
    libc.getenv.restype = ctypes.c_char_p
    libc.getenv.argtypes = [ctypes.c_char_p]
    v = libc.getenv(b"EPSILON_HIP_FUSED_ZERO")
    return None if v is None else v.decode()


@pytest.fixture
def option_auto(lib_built):
    _solve.set_option("fused_zero", "auto")
    yield
    _solve.set_option("fused_zero", "auto")


@pytest.mark.parametrize("value", ["0", "auto"])
def test_option_accepts_the_two_values(option_auto, value):
    _solve.set_option("fused_zero", value)
    assert stored() == value


def test_option_accepts_the_number_zero(option_auto):
    _solve.set_option("fused_zero", 0)
    assert stored() == "0"


@pytest.mark.parametrize("value", ["1", "on", "Auto", ""])
def test_option_rejects_other_values_by_name(option_auto, value):
    _solve.set_option("fused_zero", "0")
    with pytest.raises(_solve.error, match="fused_zero must be 0 or auto, got %s" % value):
        _solve.set_option("fused_zero", value)
    assert stored() == "0"
