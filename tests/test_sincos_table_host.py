"""The remainder table of Box-Muller's 20-bit angle (klara.jl_amd/csrc/detmath.h), without a GPU.

kd_sincos2pi_bits is kd_sincos_rem (sin y and cos y - 1 of the angle's remainder) followed by kd_sincos_rotate (the (C, S) table entry and four
fmas).  For the angle of kd_normal_pair_w, 1 + (k + 1/2) 2^-20, the remainder depends on m = k & 0xfff alone, so the kernels that run many
transitions per launch read (sin y, cos y - 1) from a 4,096-entry table T[m] that they fill with kd_sincos_rem_entry.  Here tests/sincos_table_ref.c
is compiled against the header (gcc, -ffp-contract=off) and, for all 2^20 angles, kd_sincos_rotate(j, T[m]) is compared with the arithmetic form
bit for bit."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import oracle_ffi as O

ROOT = Path(__file__).resolve().parent.parent
SRC = Path(__file__).resolve().parent / "sincos_table_ref.c"
N = 1 << 20


@pytest.fixture(scope="module")
def ref():
    so = O.build_c("sincos_table_ref", ["-O2", "-std=gnu11", "-ffp-contract=off", "-fPIC", "-shared", *O.INC], sources=[SRC],
                   hashed=[O.CSRC / "detmath.h", O.CSRC / "detmath_tables.h"])
    lib = C.CDLL(str(so))
    lib.st_fill.argtypes = [C.c_void_p]
    lib.st_fill.restype = None
    lib.st_compare.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.st_compare.restype = C.c_int64
    lib.st_compare_double_form.argtypes = [C.c_void_p]
    lib.st_compare_double_form.restype = C.c_int64
    table = np.full((4096, 2), np.nan)
    lib.st_fill(table.ctypes.data)
    return lib, table


def test_table_form_equals_arithmetic_form_at_every_angle(ref):
    lib, table = ref
    assert np.isfinite(table).all()
    for low12 in (0, 1):                                   # the 12 bits below the angle belong to the radius: they must not matter
        sy, dc = np.empty(N), np.empty(N)
        first = C.c_int64(-2)
        bad = lib.st_compare(table.ctypes.data, low12, sy.ctypes.data, dc.ctypes.data, C.byref(first))
        assert bad == 0, f"{bad} of {N} angles differ, the first at k = {first.value}"
        # the values the table replaces: 4,096 distinct (sin y, cos y - 1) pairs, pair m at every k with k & 0xfff == m
        pairs = np.stack([sy, dc], axis=1).view(np.uint64)
        assert np.unique(pairs, axis=0).shape[0] == 4096
        assert np.array_equal(pairs.reshape(256, 4096, 2), np.broadcast_to(table.view(np.uint64), (256, 4096, 2)))


def test_table_entries_are_what_they_stand_for(ref):
    """T[m] against sin y and cos y - 1 in extended precision, y = 2 pi ((m + 1/2 - 2048) 2^-20 + 2^-53), |y| <= 0.0123; the polynomials'
    dropped terms are below 2e-20 relative.  sin y = fma(y z (...), y): y's rounding and the fma's, everything else scaled by y^2 < 2e-4 — one
    ulp, and the bound is two ulps of the largest entry (2 x 2^-59, |sin y| < 2^-6).  cos y - 1 = z * poly(z) with z = y * y: six roundings
    reach it at full weight (y's twice through the square, z's, the polynomial's last fma, the product, and one for the reference's own
    argument), so the bound is 6 x 2^-53 relative to |cos y - 1| < 2^-13.  Both doubled where long double is no wider than double.
    (The reference takes cos y - 1 as -2 sin^2(y/2): the difference itself would cancel 13 bits.)"""
    _, table = ref
    m = np.arange(4096, dtype=np.longdouble)
    twopi = np.longdouble(8) * np.arctan(np.longdouble(1))
    y = twopi * ((m + np.longdouble(0.5) - 2048) * np.longdouble(2.0 ** -20) + np.longdouble(2.0 ** -53))
    wide = 1 if np.finfo(np.longdouble).eps < 1e-18 else 2
    assert np.max(np.abs(y)) < 0.0123 and np.max(np.abs(table[:, 0])) < 2.0 ** -6 and np.max(np.abs(table[:, 1])) < 2.0 ** -13
    assert np.max(np.abs(table[:, 0].astype(np.longdouble) - np.sin(y))) < wide * 2 * 2.0 ** -59
    assert np.max(np.abs(table[:, 1].astype(np.longdouble) - (-2 * np.sin(y / 2) ** 2))) < wide * 6 * 2.0 ** -53 * 2.0 ** -13


def test_double_argument_form_hits_the_same_bits(ref):
    """kd_sincos2pi((k + 1/2) 2^-20) — ops 2 / 3 of the device selftest — forms u + (1 - 2^-53): a tie that rounds to the even neighbour
    1 + (k + 1/2) 2^-20, the 20-bit angle's own bits, so it too equals the table form at every k (tests/test_gpu_sincos_table.py relies on it)."""
    lib, table = ref
    k = np.arange(N, dtype=np.float64)
    uu = (k + 0.5) * 2.0 ** -20 + float.fromhex("0x1.fffffffffffffp-1")
    assert np.array_equal(uu.view(np.uint64), ((0x3FF00000 | np.arange(N, dtype=np.uint64)) << np.uint64(32)) | np.uint64(0x80000000))
    assert lib.st_compare_double_form(table.ctypes.data) == 0
