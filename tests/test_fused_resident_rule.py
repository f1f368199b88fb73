"""The residency rule of the fused pass (include/epsilon_hip.h eps_fused_residency; option
"fused_resident"): a pure host function of (m, n, dtype, budget) that needs no device.  Row chunk q
of column j stays in the Infinity Cache iff q < qfull or (q == qfull and j < jcut); the resident
bytes are the largest total of this form within the budget."""

import ctypes
import re

import pytest

from epsilon_amd import _solve


def rule(m, n, dtype, budget):
    q, j, b = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
    _solve._check(_solve.lib().eps_fused_residency(ctypes.c_int64(m), ctypes.c_int64(n), ctypes.c_int(dtype == "f64"),
                                                   ctypes.c_int64(budget), ctypes.byref(q), ctypes.byref(j),
                                                   ctypes.byref(b)))
    return q.value, j.value, b.value


def pieces(m, dtype):
    """bytes of every row chunk of one column: 16 bytes per thread of the workgroup (512 threads
    where 256 cannot own the rows), the last chunk as far as the rows go"""
    elem = 8 if dtype == "f64" else 4
    chunk = 16 * (512 if m > (5120 if dtype == "f64" else 10240) else 256)
    col = m * elem
    return [min(chunk, col - at) for at in range(0, col, chunk)]


def resident_bytes(m, n, dtype, qfull, jcut):
    p = pieces(m, dtype)
    assert 0 <= qfull <= len(p) and 0 <= jcut < max(n, 1) + (qfull == len(p)) and (qfull < len(p) or jcut == 0)
    return n * sum(p[:qfull]) + (jcut * p[qfull] if jcut else 0)


SHAPES = [(4, 3), (4, 1), (1024, 1), (2560, 301), (2562, 301), (10000, 50000), (10244, 64), (20480, 7), (2048, 8192)]


# (the f64 pass ends at 10240 rows)
CASES = [(m, n, dt) for m, n in SHAPES for dt in ("f32", "f64") if dt == "f32" or m <= 10240]


@pytest.mark.parametrize("m,n,dtype", CASES)
def test_largest_share_within_the_budget(m, n, dtype):
    elem = 8 if dtype == "f64" else 4
    p = pieces(m, dtype)
    total = m * n * elem
    assert n * sum(p) == total
    budgets = {0, 1, 15, 16, p[0] - 1, p[0], p[0] + 1, p[0] * n - 1, p[0] * n, p[0] * n + p[-1], total // 3,
               total // 2 + 5, total - 1, total, total + 1, 4 * total, 200 << 20, 256 << 20}
    for budget in sorted(budgets):
        qfull, jcut, got = rule(m, n, dtype, budget)
        assert got == resident_bytes(m, n, dtype, qfull, jcut), (budget, qfull, jcut, got)
        assert got <= budget, (budget, qfull, jcut, got)
        if budget >= total:
            assert (qfull, jcut, got) == (len(p), 0, total)  # a matrix that fits is resident as a whole
        else:
            assert qfull < len(p) and jcut < n
            assert got + p[qfull] > budget, (budget, qfull, jcut, got)  # one more chunk-column would not fit
    assert rule(m, n, dtype, 0) == (0, 0, 0) and rule(m, n, dtype, -5) == (0, 0, 0)


def test_the_share_grows_with_the_budget():
    m, n = 10000, 50000
    last = (0, 0, 0)
    for mib in (0, 64, 128, 160, 192, 208, 224, 240, 2048):
        cur = rule(m, n, "f32", mib << 20)
        assert (cur[0], cur[1]) >= (last[0], last[1]) and cur[2] >= last[2]
        last = cur
    assert last == (10, 0, m * n * 4)


def test_bad_arguments_are_errors():
    for m, n in ((0, 5), (5, 0)):
        with pytest.raises(_solve.error, match="eps_fused_residency"):
            rule(m, n, "f32", 100)


# ---- the option ("fused_resident"): checks that fail before any device work -----------------------
def stored():
    """the option as the library reads it: the process environment"""
    libc = ctypes.CDLL(None)
    libc.getenv.restype = ctypes.c_char_p
    libc.getenv.argtypes = [ctypes.c_char_p]
    v = libc.getenv(b"EPSILON_HIP_FUSED_RESIDENT_KB")
    return None if v is None else v.decode()


@pytest.fixture
def option_auto():
    _solve.set_option("fused_resident", "auto")
    yield
    _solve.set_option("fused_resident", "auto")


@pytest.mark.parametrize("value", ["auto", "0", "1", "204800", 65536])
def test_option_accepts_auto_and_kib(option_auto, value):
    _solve.set_option("fused_resident", value)
    assert stored() == str(value)


@pytest.mark.parametrize("value", ["-1", "on", "Auto", "", "12MB", "1.5", "+5", " 5"])
def test_option_rejects_other_values_by_name(option_auto, value):
    _solve.set_option("fused_resident", "0")
    with pytest.raises(_solve.error, match="fused_resident must be auto or a number of KiB, got " + re.escape(value) + "$"):
        _solve.set_option("fused_resident", value)
    assert stored() == "0"


def test_option_clamps_a_huge_number(option_auto):
    _solve.set_option("fused_resident", "9" * 40)  # no overflow into a negative budget: accepted
    assert stored() == "9" * 40
