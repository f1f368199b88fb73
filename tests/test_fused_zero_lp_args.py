"""The "fused_zero_lp" option (include/epsilon_hip.h eps_set_option): the fused sweep of ZERO-term
problems with a linear term on x or the non-negative cone on z (linear programs in graph form).  Its
words are "0" and "1"; unset means "0".  Checks that fail before any device work: they need the built
library, not a GPU."""

import ctypes
import os

import pytest

from epsilon_amd import _solve

KEY, NAME = "fused_zero_lp", "EPSILON_HIP_FUSED_ZERO_LP"


@pytest.fixture(scope="module")
def lib_built():
    if not os.path.exists(_solve.LIB_PATH):
        pytest.fail("libepsilon_hip.so is not built")
    return _solve


def stored(name=NAME):
    """the option as the library reads it: the process environment"""
    libc = ctypes.CDLL(None)
    libc.getenv.restype = ctypes.c_char_p
    libc.getenv.argtypes = [ctypes.c_char_p]
    v = libc.getenv(name.encode())
    return None if v is None else v.decode()


@pytest.fixture
def option_off(lib_built):
    _solve.set_option(KEY, "0")
    yield
    _solve.set_option(KEY, "0")


@pytest.mark.parametrize("value", ["0", "1"])
def test_option_accepts_its_two_words(option_off, value):
    _solve.set_option(KEY, value)
    assert stored() == value


@pytest.mark.parametrize("value,text", [(0, "0"), (1, "1")])
def test_option_accepts_numbers(option_off, value, text):
    _solve.set_option(KEY, value)
    assert stored() == text


@pytest.mark.parametrize("start", ["0", "1"])
@pytest.mark.parametrize("value", ["auto", "2", "", "on"])
def test_option_rejects_other_values_by_name(option_off, value, start):
    _solve.set_option(KEY, start)
    with pytest.raises(_solve.error, match="fused_zero_lp must be 0 or 1, got %s$" % value):
        _solve.set_option(KEY, value)
    assert stored() == start


def test_the_other_zero_options_keep_their_values(option_off):
    """the new option leaves the other ZERO options, their words and error texts as they were"""
    for key, name, words, bad, default in (
            ("fused_zero", "EPSILON_HIP_FUSED_ZERO", "0 or auto", "1", "auto"),
            ("fused_zero_tall", "EPSILON_HIP_FUSED_ZERO_TALL", "0, 1 or auto", "2", "auto"),
            ("fused_zero_tall_smooth", "EPSILON_HIP_FUSED_ZERO_TALL_SMOOTH", "0, 1 or auto", "2", "auto"),
            ("fused_zero_ridge", "EPSILON_HIP_FUSED_ZERO_RIDGE", "0, 1 or auto", "2", "auto"),
            ("fused_zero_xfree", "EPSILON_HIP_FUSED_ZERO_XFREE", "0 or 1", "auto", "0"),
            ("fused_zero_check", "EPSILON_HIP_FUSED_ZERO_CHECK", "0 or 1", "auto", "0"),
            ("batch_zero_tall", "EPSILON_HIP_BATCH_ZERO_TALL", "0 or 1", "auto", "0")):
        _solve.set_option(key, default)
        try:
            with pytest.raises(_solve.error, match="%s must be %s, got %s" % (key, words, bad)):
                _solve.set_option(key, bad)
            assert stored(name) == default
            for word in words.replace(" or ", ", ").split(", "):
                _solve.set_option(key, word)
                assert stored(name) == word
        finally:
            _solve.set_option(key, default)
