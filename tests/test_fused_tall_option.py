"""The option "fused_tall" (csrc/options.cc; the tall lasso route) at the boundary:
every word is accepted and stored in EPSILON_HIP_FUSED_TALL, any other value raises the generated
text and stores nothing.  Needs the built library, not a GPU.  The environment is put back."""

import ctypes
import os

import pytest

from epsilon_amd import _solve

KEY, NAME, WORDS = "fused_tall", "EPSILON_HIP_FUSED_TALL", ["0", "1", "auto"]


def libc():
    c = ctypes.CDLL(None)
    c.getenv.restype = ctypes.c_char_p
    c.getenv.argtypes = [ctypes.c_char_p]
    c.setenv.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]
    c.unsetenv.argtypes = [ctypes.c_char_p]
    return c


def stored():
    """the option as the library reads it: the process environment"""
    v = libc().getenv(NAME.encode())
    return None if v is None else v.decode()


@pytest.fixture
def environment_kept():
    if not os.path.exists(_solve.LIB_PATH):
        pytest.fail("libepsilon_hip.so is not built")
    before = stored()
    yield
    if before is None:
        libc().unsetenv(NAME.encode())
    else:
        libc().setenv(NAME.encode(), before.encode(), 1)
    assert stored() == before


def test_every_word_is_accepted_and_stored(environment_kept):
    for word in WORDS:
        _solve.set_option(KEY, word)
        assert stored() == word


def test_other_values_raise_the_generated_text_and_store_nothing(environment_kept):
    for keep in WORDS:
        _solve.set_option(KEY, keep)
        for value in ["", "AUTO", "2", "pass", "wide", "on", "auto "]:
            with pytest.raises(_solve.error) as info:
                _solve.set_option(KEY, value)
            text = "fused_tall must be 0, 1 or auto, got %s" % value
            assert str(info.value).endswith(": " + text), (value, str(info.value))
            assert stored() == keep
