"""Shared by tests/test_dayquant_host.py and tests/test_gpu_dayquant.py: the
order statistics of include/h9g.h (h9g_get_dayquant) stated a third time, as a
plain per-cell loop that sorts (key, value) pairs (``order_stats_loop``; the
header's contract and hybrid9_amd.day_order_stats are the other two); the host
build of hybrid9_amd/csrc/h9g_quant.h (tests/csrc/host_quant.cpp) with every
year cut wherever the caller says and every digit width the kernel is built
with; and hand-made records of three years built to go wrong where a selection
by key can go wrong."""
from __future__ import annotations

import ctypes as C
import math
import struct
import subprocess

import numpy as np

import hybrid9_amd as h
from tests.daystat_helpers import handmade, random_records
from tests.helpers import BUILD, ROOT

F = np.float32
D = np.float64
# unsorted, with a repeat; 0.2 * 365 is a whole number (m = 366: g = j exactly)
QP = (0.0, 0.05, 0.5, 0.95, 1.0, 0.5, 0.2)
BITS = (2, 4, 8)         # the digit widths h9g_dayquant_kernel is built with
WS = (4, 8, 16)          # ... and its workgroups (waves = slices of a year)
NSERIES = len(h.DAYQUANT_SERIES)
HAND_NT = (365, 366, 365)

_lib = None


# ---- the contract, as a loop over cells that sorts (key, value) pairs ---------
def _key(x: float) -> int:
    (u,) = struct.unpack("<Q", struct.pack("<d", x))
    return u ^ (0xFFFFFFFFFFFFFFFF if u >> 63 else 1 << 63)


def order_stats_loop(records_by_year, *, series, p, pooled=False):
    """list of (nday_y, 7, n) float32 -> (nres, 1 + 2 len(p), n) float64, cell
    by cell.  Python floats are IEEE doubles and hold every float32 exactly, so
    the subtraction is the one float64 subtraction of the contract."""
    yrs = [np.asarray(r, F) for r in records_by_year]
    n = yrs[0].shape[2]
    s = h.DAYQUANT_SERIES.index(series) if isinstance(series, str) else int(series)
    p = [float(v) for v in np.atleast_1d(p)]
    groups = [list(range(len(yrs)))] if pooled else [[y] for y in range(len(yrs))]
    out = np.empty((len(groups), 1 + 2 * len(p), n), D)
    nan = float("nan")
    for res, ys in enumerate(groups):
        for c in range(n):
            pairs = []
            for y in ys:
                col = yrs[y][:, s, c].astype(D).tolist()         # (exact)
                for d, v in enumerate(col):
                    x = v - (col[d - 1] if d > 0 else 0.0) if s < 2 else v
                    if not math.isnan(x):
                        pairs.append((_key(x), x))
            pairs.sort(key=lambda kv: kv[0])
            m = len(pairs)
            out[res, 0, c] = m
            for i, pi in enumerate(p):
                if m == 0:
                    lo = hi = nan
                else:
                    g = pi * float(m - 1)
                    j = int(math.floor(g))
                    lo, hi = pairs[j][1], pairs[min(j + 1, m - 1)][1]
                out[res, 1 + 2 * i, c] = lo
                out[res, 2 + 2 * i, c] = hi
    return out


# ---- the host build of h9g_quant.h ------------------------------------------------
def quant_lib():
    global _lib
    if _lib is None:
        src = ROOT / "tests" / "csrc" / "host_quant.cpp"
        out = BUILD / "libhost_quant.so"
        deps = [src, ROOT / "include" / "h9g.h"] + list((ROOT / "hybrid9_amd" / "csrc").glob("*.h"))
        if not out.exists() or out.stat().st_mtime < max(d.stat().st_mtime for d in deps):
            BUILD.mkdir(exist_ok=True)
            subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-fPIC", "-shared",
                            str(src), "-o", str(out)], check=True)
        _lib = C.CDLL(str(out))
        ip = C.POINTER(C.c_int)
        _lib.h9k_host_quant.argtypes = [C.c_int, C.c_int, ip, C.POINTER(C.c_float), C.c_int, ip, C.c_int, C.c_int,
                                        C.c_int, C.POINTER(h._QuantOpts), C.POINTER(C.c_double)]
        _lib.h9k_host_quant_cuts.argtypes = [C.c_int, C.c_int, ip]
        _lib.h9k_host_quant_opts_ok.argtypes = [C.POINTER(h._QuantOpts)]
    return _lib


def pack_years(records_by_year):
    """list of (nday_y, 7, n) -> (nt int32 (nyears), records (nyears, ntmax, 7, n) float32, NaN padded)."""
    yrs = [np.asarray(r, F) for r in records_by_year]
    nt = np.array([r.shape[0] for r in yrs], np.int32)
    rec = np.full((len(yrs), int(nt.max()), 7, yrs[0].shape[2]), np.nan, F)
    for y, r in enumerate(yrs):
        rec[y, :r.shape[0]] = r
    return nt, rec


def host_quant(records_by_year, *, series, p, pooled=False, cuts=(), rev=False, bits=4, key64=False):
    """quant_cand / quant_digit / quant_step / quant_needs_succ on the host:
    every year cut at `cuts` (strictly increasing days > 0), the slices visited
    in order (rev: last to first), digits of `bits` bits, the 64-bit key for
    every series with key64 -> (nres, 1 + 2 len(p), n)."""
    nt, rec = pack_years(records_by_year)
    o = h.dayquant_opts(series=series, p=p, pooled=pooled)
    cu = np.ascontiguousarray(cuts, np.int32)
    out = np.empty((1 if pooled else nt.size, 1 + 2 * o.nq, rec.shape[3]), D)
    ip = C.POINTER(C.c_int)
    rc = quant_lib().h9k_host_quant(rec.shape[3], nt.size, nt.ctypes.data_as(ip),
                                    rec.ctypes.data_as(C.POINTER(C.c_float)), cu.size, cu.ctypes.data_as(ip),
                                    int(rev), int(bits), int(key64), C.byref(o),
                                    out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0, "h9k_host_quant refused its arguments"
    return out


def kernel_cuts(nt, nseg):
    """The cuts of h9g_dayquant_kernel's nseg slices of a year of nt days."""
    cu = np.zeros(max(nseg, 1), np.int32)
    m = quant_lib().h9k_host_quant_cuts(int(nt), int(nseg), cu.ctypes.data_as(C.POINTER(C.c_int)))
    return cu[:m].copy()


def cut_sets(nt, seed=0, nrandom=4):
    """The cuts the tests compare: none, the kernel's for every W built, every
    day on its own, and a few random ones."""
    rng = np.random.default_rng(seed)
    sets = [("one slice", np.zeros(0, np.int32))]
    sets += [(f"W = {w}", kernel_cuts(nt, w)) for w in WS]
    sets.append(("single days", np.arange(1, nt, dtype=np.int32)))
    for k in range(nrandom):
        m = int(rng.integers(1, 40))
        sets.append((f"random {k}", np.sort(rng.choice(np.arange(1, nt), size=m, replace=False)).astype(np.int32)))
    return sets


# ---- hand-made records -----------------------------------------------------------------
def handmade3():
    """Three years (365, 366, 365 days) x 13 cells, every value exact in float32.
    Cells 0..7 are daystat_helpers.handmade()'s (ties of extremes, -0 among +0
    in q and e of cell 1 and in zwt of cell 4, negative LAI with -0 and +0 in
    cell 5, cell 6 stopping on day 3 of the first year, cell 7 with no day);
    year 0 is its first 365 days, year 1 all 366, year 2 year 0 run backwards
    (the same values on other days).  Then:
      8   every value of every series equal (q and e too: sums of a constant)
      9   values that differ only in the lowest bit of the key: theta1 between
          0.3f and the next float32 (32-bit key), q between 1 and 1 + 2^-52
          (64-bit key: sums alternating between -1 and 2^-52) and their negatives
      10  zwt all +0 with -0 among them; soil water with the smallest denormals
          of either sign; a denormal first runoff sum; LAI with +inf one day
      11  a runoff sum that is +inf for one day (q = +inf, then -inf) and for
          two days running (inf - inf: a NaN candidate from records that are not NaN)
      12  one day only: a STOP on day 1 of the first year"""
    base = handmade()                              # (366, 7, 8)
    n = 13
    yrs = []
    for y, nt in enumerate(HAND_NT):
        d = np.arange(nt)
        rec = np.zeros((nt, 7, n), F)
        rec[:, :, :8] = base[:nt]
        q = (1 + (d * 7 + y) % 5).astype(D)
        e = (1 + (d * 3 + y) % 4).astype(D) * 0.5
        for c in range(8, n):
            rec[:, 0, c] = np.cumsum(q)
            rec[:, 1, c] = np.cumsum(e)
            rec[:, 2, c] = 300 + (d * 11 + 5 * y) % 37
            rec[:, 3, c] = 0.3 + 0.03125 * ((d * 5 + y) % 3)
            rec[:, 4, c] = 400 + 8 * ((d * 13 + y) % 29)
            rec[:, 5, c] = 4000 + d
            rec[:, 6, c] = 0.5 + 0.0625 * ((d * 3 + y) % 17)
        rec[:, 0, 8] = 3.0 * (d + 1)               # cell 8
        rec[:, 1, 8] = 0.5 * (d + 1)
        rec[:, 2:, 8] = np.array([310, 0.25, 1200, 4100, 2.5], F)[None, :]
        lo, up = F(0.3), np.nextafter(F(0.3), F(1))            # cell 9
        rec[:, 3, 9] = np.where((d * 7) % 3 == 0, up, lo)
        s9 = np.where(d % 2 == 1, -1.0, 2.0 ** -52)
        s9[0] = 1.0
        rec[:, 0, 9] = s9
        rec[:, 4, 10] = 0.0                        # cell 10
        rec[(d * 5) % 7 == 0, 4, 10] = -0.0
        tiny = np.float32(1.0e-45)
        rec[:, 2, 10] = np.where(d % 3 == 0, tiny, np.where(d % 3 == 1, -tiny, 0.0))
        rec[0, 0, 10] = tiny
        rec[50, 6, 10] = np.inf
        rec[200, 0, 11] = np.inf                   # cell 11
        rec[300:302, 0, 11] = np.inf
        rec[1:, :, 12] = np.nan                    # cell 12
        yrs.append(rec)
    yrs[2][:, 2:, :8] = yrs[2][::-1, 2:, :8].copy()
    for y in (1, 2):                               # a stopped cell stays stopped
        yrs[y][:, :, 6] = np.nan
        yrs[y][:, :, 12] = np.nan
    assert np.isnan(yrs[0][3:, :, 6]).all() and np.isnan(yrs[0][:, :, 7]).all()
    return yrs


def check_handmade3(per_year, pooled, series):
    """What the hand-made records were made for, on the results for QP of one
    series: per_year (3, 15, 13), pooled (1, 15, 13)."""
    m, mp = per_year[:, 0], pooled[0, 0]
    assert (m[:, 7] == 0).all() and mp[7] == 0 and np.isnan(per_year[:, 1:, 7]).all() and np.isnan(pooled[0, 1:, 7]).all()
    assert list(m[:, 6]) == [3, 0, 0] and mp[6] == 3
    assert list(m[:, 12]) == [1, 0, 0] and mp[12] == 1
    one = per_year[0, 1:, 12]
    assert (one == one[0]).all()                   # m = 1: every order statistic is that day
    assert mp[8] == sum(HAND_NT) and (np.diff(pooled[0, 1:, 8]) == 0).all()       # all equal
    sign = np.signbit
    i_min, i_max, i_med = 1, 1 + 2 * 4, 1 + 2 * 2
    if series == 0:
        assert pooled[0, i_min, 1] == 0 and sign(pooled[0, i_min, 1])            # -0 first ...
        assert pooled[0, i_min + 1, 1] == 0 and sign(pooled[0, i_min + 1, 1])    # (one a year)
        assert pooled[0, i_max, 1] == 0 and not sign(pooled[0, i_max, 1])        # ... +0 last
        v = np.unique(per_year[1, 1:, 9])
        assert {1.0, 1.0 + 2.0 ** -52} <= set(v) and (v < 0).any()
        assert per_year[0, 0, 10] == 365 and per_year[0, i_min, 10] == 2.0 ** -149
        assert per_year[0, i_max, 11] == np.inf and per_year[0, i_min, 11] == -np.inf
        assert per_year[0, 0, 11] == 365 - 1       # inf - inf is skipped
    if series == 3:
        lo, up = F(0.3), np.nextafter(F(0.3), F(1))
        assert per_year[0, i_min, 9] == D(lo) and per_year[0, i_max, 9] == D(up)
        assert per_year[0, i_med, 9] in (D(lo), D(up))
    if series == 4:
        assert sign(pooled[0, i_min, 10]) and not sign(pooled[0, i_max, 10]) and (pooled[0, 1:, 10] == 0).all()
        assert sign(per_year[1, i_min, 4]) and per_year[1, i_min, 4] == 0        # -0 below +0 below 5
        assert per_year[1, i_min + 1, 4] == 0 and not sign(per_year[1, i_min + 1, 4])
    if series == 2:
        assert per_year[0, i_min, 10] == -(2.0 ** -149) and per_year[0, i_max, 10] == 2.0 ** -149
    if series == 6:
        assert per_year[0, i_max, 10] == np.inf and np.isfinite(per_year[0, i_max - 2, 10])
        assert pooled[0, i_min, 5] == -1 and pooled[0, i_max, 5] == 0 and not sign(pooled[0, i_max, 5])


def random_years(n, seed):
    """Three years (365, 366, 365) of daystat_helpers.random_records: few
    distinct values (many ties), NaN tails of random length.  Cell 0 has no day
    in any year and cell 1 every day of every year (a complete cell's days)."""
    yrs = [random_records(n, nt, seed + y) for y, nt in enumerate(HAND_NT)]
    for r in yrs:
        whole = np.flatnonzero(~np.isnan(r).any(axis=(0, 1)))
        r[:, :, 1] = r[:, :, whole[0]]
        r[:, :, 0] = np.nan
    return yrs
