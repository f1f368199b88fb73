"""The "fused_matrix" option (include/epsilon_hip.h eps_set_option): the route of the fused sweep
for matrix variables.  Checks that fail before any device work: they need the built library, not
a GPU."""

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
    v = libc.getenv(b"EPSILON_HIP_FUSED_MATRIX")
    return None if v is None else v.decode()


@pytest.fixture
def option_auto(lib_built):
    _solve.set_option("fused_matrix", "auto")
    yield
    _solve.set_option("fused_matrix", "auto")


@pytest.mark.parametrize("value", ["0", "pass", "wide", "auto"])
def test_option_accepts_the_four_values(option_auto, value):
    _solve.set_option("fused_matrix", value)
    assert stored() == value


def test_option_accepts_the_number_zero(option_auto):
    _solve.set_option("fused_matrix", 0)
    assert stored() == "0"


@pytest.mark.parametrize("value", ["1", "on", "Wide", ""])
def test_option_rejects_other_values_by_name(option_auto, value):
    _solve.set_option("fused_matrix", "pass")
    with pytest.raises(_solve.error, match="fused_matrix must be 0, pass, wide or auto, got %s" % value):
        _solve.set_option("fused_matrix", value)
    assert stored() == "pass"
