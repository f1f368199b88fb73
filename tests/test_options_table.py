"""The option table (epsilon_amd/csrc/options.{h,cc}): what eps_set_option does for every key that
is stored in the process environment, that this unit alone touches the environment, and that the
table and README.md's list of variables name the same variables.  Needs the built library, not a
GPU."""

import ctypes
import os
import re

import pytest

from epsilon_amd import _solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "epsilon_amd", "csrc")

# key -> (variable, words in index order): the options with a choice of words
WORDS = {
    "fused_zero": ("EPSILON_HIP_FUSED_ZERO", ["0", "auto"]),
    "fused_zero_tall": ("EPSILON_HIP_FUSED_ZERO_TALL", ["0", "1", "auto"]),
    "fused_zero_tall_smooth": ("EPSILON_HIP_FUSED_ZERO_TALL_SMOOTH", ["0", "1", "auto"]),
    "fused_matrix": ("EPSILON_HIP_FUSED_MATRIX", ["0", "pass", "wide", "auto"]),
    "batch_wide": ("EPSILON_HIP_BATCH_WIDE", ["0", "1"]),
}
FREE = {"device": "EPSILON_HIP_DEVICE", "gemm": "EPSILON_HIP_GEMM", "fused": "EPSILON_HIP_FUSED"}
VARIABLES = [v for v, _ in WORDS.values()] + list(FREE.values()) + ["EPSILON_HIP_REFINE"]


def libc():
    c = ctypes.CDLL(None)
    c.getenv.restype = ctypes.c_char_p
    c.getenv.argtypes = [ctypes.c_char_p]
    c.setenv.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]
    c.unsetenv.argtypes = [ctypes.c_char_p]
    return c


def stored(name):
    """the option as the library reads it: the process environment"""
    v = libc().getenv(name.encode())
    return None if v is None else v.decode()


@pytest.fixture
def environment_kept():
    """the library must be there; whatever a test stores is put back as it was"""
    if not os.path.exists(_solve.LIB_PATH):
        pytest.fail("libepsilon_hip.so is not built")
    before = {name: stored(name) for name in VARIABLES}
    wide = _solve._options.get("batch_wide")
    yield
    for name, value in before.items():
        if value is None:
            libc().unsetenv(name.encode())
        else:
            libc().setenv(name.encode(), value.encode(), 1)
    _solve._options.pop("batch_wide", None)
    if wide is not None:
        _solve._options["batch_wide"] = wide


def words_text(words):
    """the list as the error spells it: "0 or auto", "0, 1 or auto" """
    return ", ".join(words[:-1]) + " or " + words[-1]


@pytest.mark.parametrize("key", sorted(WORDS))
def test_every_word_is_accepted_and_stored(environment_kept, key):
    name, words = WORDS[key]
    for word in words:
        _solve.set_option(key, word)
        assert stored(name) == word


@pytest.mark.parametrize("key", sorted(WORDS))
def test_other_values_raise_the_generated_text_and_store_nothing(environment_kept, key):
    name, words = WORDS[key]
    foreign = sorted({w for _, ws in WORDS.values() for w in ws} - set(words))  # words of other options
    wrong_case = [w.upper() for w in words if w.upper() != w] or ["AUTO"]
    for keep in words:
        _solve.set_option(key, keep)
        for value in [""] + wrong_case + foreign:
            text = "%s must be %s, got %s" % (key, words_text(words), value)
            with pytest.raises(_solve.error) as info:
                _solve.set_option(key, value)
            assert str(info.value).endswith(": " + text), (value, str(info.value))
            assert stored(name) == keep


def test_the_four_shapes_of_the_word_list():
    assert {words_text(w) for _, w in WORDS.values()} == {"0 or auto", "0, 1 or auto", "0, pass, wide or auto", "0 or 1"}


def test_unknown_key(environment_kept):
    """(the table's rows without a key, such as EPSILON_HIP_SVD's, are no options either)"""
    for key in ("nosuch", "svd", "EPSILON_HIP_SVD", ""):
        with pytest.raises(_solve.error) as info:
            _solve.set_option(key, "1")
        assert str(info.value).endswith(": unknown option " + key)


def test_refine_auto_unsets(environment_kept):
    _solve.set_option("refine", "2")
    assert stored("EPSILON_HIP_REFINE") == "2"
    _solve.set_option("refine", "auto")
    assert stored("EPSILON_HIP_REFINE") is None
    _solve.set_option("refine", "auto")  # (unsetting an unset variable is no error)
    assert stored("EPSILON_HIP_REFINE") is None


@pytest.mark.parametrize("key", sorted(FREE))
def test_unvalidated_keys_store_any_string(environment_kept, key):
    for value in ["0", "off", "", "Auto", "no such value 7"]:
        _solve.set_option(key, value)
        assert stored(FREE[key]) == value


def sources():
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".cc", ".h", ".hip")):
            with open(os.path.join(CSRC, f)) as fh:
                yield f, fh.read()


def test_one_unit_touches_the_environment():
    users = {f for f, text in sources() if re.search(r"\b(getenv|setenv|unsetenv)\s*\(", text)}
    assert users == {"options.cc"}


def test_table_and_readme_name_the_same_variables():
    with open(os.path.join(CSRC, "options.cc")) as fh:
        table = set(re.findall(r'"(EPSILON_HIP_[A-Z0-9_]+)"', fh.read()))
    with open(os.path.join(ROOT, "README.md")) as fh:
        readme = fh.read()
    start = readme.index("| variable | effect |")
    rows = readme[start:].split("\n\n")[0]
    documented = set(re.findall(r"EPSILON_HIP_[A-Z0-9_]+", rows))
    assert len(table) >= 48
    assert table - documented == set(), "in options.cc, not in README.md's table"
    assert documented - table == set(), "in README.md's table, not in options.cc"


def test_no_variable_is_named_outside_the_table():
    """a site names its knob by the enum: no other unit spells a variable in a string"""
    for f, text in sources():
        if f != "options.cc":
            assert re.findall(r'"EPSILON_HIP_[A-Z0-9_]+"', text) == [], f
