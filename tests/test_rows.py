"""The row layout of the per-cell arrays (hybrid9_amd/csrc/h9g_rows.h) on the
host (tests/csrc/host_rows.cpp, test-only): its packed <-> rows transposition
against oracle/refcase.unpack_state, the layout stated independently of the
header, and a load-then-store round trip of its per-cell helpers through
St<L> and a FlatStore<L>."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from oracle import refcase
from tests.helpers import BUILD, ROOT

FP = C.POINTER(C.c_float)
_lib = None


def rows_lib():
    global _lib
    if _lib is None:
        src = ROOT / "tests" / "csrc" / "host_rows.cpp"
        out = BUILD / "libhost_rows.so"
        deps = [src] + list((ROOT / "hybrid9_amd" / "csrc").glob("*.h"))
        if not out.exists() or out.stat().st_mtime < max(d.stat().st_mtime for d in deps):
            BUILD.mkdir(exist_ok=True)
            subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-fPIC", "-shared",
                            str(src), "-o", str(out)], check=True)
        _lib = C.CDLL(str(out))
        _lib.h9k_rows_unpack.argtypes = _lib.h9k_rows_pack.argtypes = [C.c_int, C.c_int, FP, FP]
        _lib.h9k_rows_unpack_params.argtypes = [C.c_int, C.c_int, FP, FP]
        _lib.h9k_rows_roundtrip.argtypes = [C.c_int, C.c_int, FP, FP, FP, FP, C.c_int, C.c_int]
    return _lib


def same_bits(a, b):
    """Equal bit patterns, NaN payloads and the sign of zero included."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def distinct(k, start=1):
    """k float32 with distinct bit patterns (an arange viewed as float32:
    denormals, no NaN)."""
    return np.arange(start, start + k, dtype=np.uint32).view(np.float32)


def special(buf):
    """... with a quiet and a signalling NaN payload and a -0.0 in it."""
    b = buf.copy().view(np.uint32)
    b[1], b[b.size // 2], b[-2] = 0x7FC12345, 0x7F800123, 0x80000000
    return b.view(np.float32)


def unpack(L, n, packed):
    rows = np.full((4 * L + 9, n), np.float32(-7.0))
    rows_lib().h9k_rows_unpack(L, n, packed.ctypes.data_as(FP), rows.ctypes.data_as(FP))
    return rows


def expected_rows(L, n, packed):
    """The rows as oracle/refcase.py states the packed layout: field by field,
    value i of cell c of a field in row (field's first row + i), column c."""
    st = refcase.unpack_state(packed, n, L)
    return np.concatenate([np.asarray(st[name]).reshape(n, w).T for name, w in refcase.state_fields(L)])


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("L", [8, 10])
def test_unpack_is_refcase_layout_and_pack_inverts_it(L, n):
    assert rows_lib().h9k_rows_state_size(L) == 4 * L + 9
    for packed in (distinct((4 * L + 9) * n), special(distinct((4 * L + 9) * n))):
        rows = unpack(L, n, packed)
        assert same_bits(rows, expected_rows(L, n, packed))
        back = np.zeros_like(packed)
        rows_lib().h9k_rows_pack(L, n, rows.ctypes.data_as(FP), back.ctypes.data_as(FP))
        assert same_bits(back, packed)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("L", [8, 10])
def test_unpack_params_layout(L, n):
    packed = special(distinct((4 * L + 1) * n, start=5000))
    rows = np.zeros((4 * L + 1, n), np.float32)
    rows_lib().h9k_rows_unpack_params(L, n, packed.ctypes.data_as(FP), rows.ctypes.data_as(FP))
    exp = np.concatenate([packed[k * n * L:(k + 1) * n * L].reshape(n, L).T for k in range(4)]
                         + [packed[4 * n * L:].reshape(1, n)])
    assert same_bits(rows, exp)


@pytest.mark.parametrize("nscalars,rootr", [(8, 1), (8, 0), (4, 0)])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("L", [8, 10])
def test_load_store_roundtrip(L, n, nscalars, rootr):
    """Loading a cell and storing it returns every row it is meant to store,
    bit for bit (NaN payloads, -0.0), and touches no other: h2o_ma never, the
    rootr rows only with `rootr` (the last one then holds rootr_col(Nlevgrnd) =
    0), pm pfm plen rdepth not in the four-scalar store of the site path."""
    st = special(distinct((4 * L + 9) * n)).reshape(4 * L + 9, n)
    par = special(distinct((4 * L + 1) * n, start=9000)).reshape(4 * L + 1, n)
    mark = np.float32(-7.0)
    st_out, par_out = np.full_like(st, mark), np.full_like(par, mark)
    rc = rows_lib().h9k_rows_roundtrip(L, n, par.ctypes.data_as(FP), st.ctypes.data_as(FP), par_out.ctypes.data_as(FP),
                                       st_out.ctypes.data_as(FP), nscalars, rootr)
    assert rc == 0
    assert same_bits(par_out, par)
    exp = np.full_like(st, mark)
    exp[0:L] = st[0:L]                           # h2o
    exp[2 * L:3 * L] = st[2 * L:3 * L]           # smp
    if rootr:
        exp[3 * L:4 * L] = st[3 * L:4 * L]
        exp[4 * L] = 0.0
    exp[4 * L + 1:4 * L + 1 + nscalars] = st[4 * L + 1:4 * L + 1 + nscalars]
    assert same_bits(st_out, exp)
    assert same_bits(st_out[L:2 * L], np.full((L, n), mark))          # h2o_ma untouched
    if nscalars == 4:
        assert same_bits(st_out[4 * L + 5:], np.full((4, n), mark))   # pm pfm plen rdepth untouched
