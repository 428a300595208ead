"""Day statistics on the host (no GPU): the three statements of the table of
include/h9g.h -- hybrid9_amd.day_stats (numpy), daystat_helpers.day_stats_loop
(a plain double loop) and the host build of hybrid9_amd/csrc/h9g_stat.h, the
lines h9g_daystat_kernel runs -- agree bit for bit on the oracle's day records
and on hand-made ones; the rows do not depend on how the year is cut into
segments; the argument checks that need no device; the sxy file.  Every
comparison is conftest.same_bits: no tolerance."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import hybrid9_amd as h
from tests.conftest import same_bits
from tests.daystat_helpers import (HAND_THR, NS, WS, check_handmade, check_meaningful, cut_sets, day_stats_loop,
                                   golden_records, handmade, host_stat, kernel_cuts, random_records, thresholds_of)
from tests.helpers import BUILD, ROOT

GOLDENS = ("c1_2yr_leap", "stop_ns24", "edge")


def _years(name):
    """(year, records (nt, 7, n)) of every year of a golden."""
    inp, rec = golden_records(name)
    return [(inp["year0"] + y, rec[y, :h.days_in_year(inp["year0"] + y)]) for y in range(inp["nyears"])]


# ---- 1-3. three statements, one answer, on the oracle's records -------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_three_statements_agree_on_oracle_records(name):
    inp, rec = golden_records(name)
    thr = thresholds_of(name, rec)
    stats = []
    for year, r in _years(name):
        a, b, c = h.day_stats(r, **thr), day_stats_loop(r, **thr), host_stat(r, **thr)
        assert a.shape == (NS, r.shape[2]) and a.dtype == np.float64
        for i, k in enumerate(h.DAYSTAT_FIELDS):
            assert same_bits(a[i], b[i]), f"{name} {year}: day_stats and the loop differ in {k}"
            assert same_bits(c[i], b[i]), f"{name} {year}: the host build and the loop differ in {k}"
        stats.append(b)
    check_meaningful(name, np.stack(stats))
    if name == "c1_2yr_leap":
        assert [r.shape[0] for _, r in _years(name)] == [365, 366]
        assert (stats[0][0] == 365).all() and (stats[1][0] == 366).all()
    if name == "stop_ns24":
        s = stats[0]
        stopped = np.flatnonzero((s[0] > 0) & (s[0] < 365))
        assert stopped.size == 1 and s[0, 2] == 0                # one cell stops; cell 2 is masked
        c = int(stopped[0])
        assert np.isnan(rec[0, int(s[0, c]):, :, c]).all()
        assert np.isnan(s[[1, 3, 5, 6, 8, 9, 12, 14], 2]).all() and (s[[2, 7, 15], 2] == -1).all()
        assert (s[[4, 10, 11, 13, 16], 2] == 0).all()


# ---- 4. the cut does not matter ----------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS + ("handmade", "random365"))
def test_rows_do_not_depend_on_the_cut(name):
    if name == "handmade":
        years, thr = [(0, handmade())], HAND_THR
    elif name == "random365":
        years, thr = [(0, random_records(40, 365, 3))], HAND_THR
    else:
        years, thr = _years(name), thresholds_of(name, golden_records(name)[1])
    seen = set()
    for year, r in years:
        nt = r.shape[0]
        seen.add(nt)
        one = host_stat(r, **thr)
        assert same_bits(one, day_stats_loop(r, **thr))
        for label, cuts in cut_sets(nt, seed=nt):
            for tree in (False, True):
                got = host_stat(r, cuts, tree=tree, **thr)
                assert same_bits(got, one), f"{name} {year}: cut '{label}' (tree {tree}) changes " \
                    f"{[h.DAYSTAT_FIELDS[i] for i in range(NS) if not same_bits(got[i], one[i])]}"
    if name == "c1_2yr_leap":
        assert seen == {365, 366}


def test_kernel_cuts_are_even_slices():
    for nt in (365, 366):
        for w in WS:
            cu = kernel_cuts(nt, w)
            edges = np.concatenate([[0], cu, [nt]])
            assert cu.size == w - 1 and set(np.diff(edges)) <= {nt // w, nt // w + 1}
    assert kernel_cuts(3, 16).size == 2           # more slices than days: the empty ones vanish


# ---- 5. hand-made records ---------------------------------------------------------------
def test_handmade_records():
    rec = handmade()
    a, b, c = h.day_stats(rec, **HAND_THR), day_stats_loop(rec, **HAND_THR), host_stat(rec, **HAND_THR)
    assert same_bits(a, b) and same_bits(c, b)
    check_handmade(b)
    for w in WS:
        assert same_bits(host_stat(rec, kernel_cuts(366, w), **HAND_THR), b)


def test_random_records_with_nan_tails():
    for nt in (365, 366):
        rec = random_records(60, nt, nt)
        a, b = h.day_stats(rec, **HAND_THR), day_stats_loop(rec, **HAND_THR)
        assert same_bits(a, b) and same_bits(host_stat(rec, **HAND_THR), b)
        assert (b[0] == 0).any() and (b[0] == nt).any() and ((b[0] > 0) & (b[0] < nt)).any()


def test_short_years():
    """Fewer than seven days: no q7; one day: every extreme is that day's."""
    rec = handmade()
    for nt in (1, 6, 7):
        a, b = h.day_stats(rec[:nt], **HAND_THR), day_stats_loop(rec[:nt], **HAND_THR)
        assert same_bits(a, b) and same_bits(host_stat(rec[:nt], **HAND_THR), b)
        assert np.isnan(b[3]).all() == (nt < 7)


# ---- 6. argument checks that need no device ------------------------------------------------
def test_argument_checks_without_a_device():
    lb = h.lib()
    dp = C.POINTER(C.c_double)
    out = np.zeros((NS, 8), np.float64)
    rec = np.ascontiguousarray(handmade())
    ok = h.daystat_opts(**HAND_THR)
    EINVAL = -1
    # h9g_get_daystats: a null context, null options, a null result
    assert lb.h9g_get_daystats(None, 0, 1, C.byref(ok), out.ctypes.data_as(dp)) == EINVAL
    fake = C.c_void_p(1)                          # (never dereferenced: the options are checked first)
    assert lb.h9g_get_daystats(fake, 0, 1, None, out.ctypes.data_as(dp)) == EINVAL
    assert lb.h9g_get_daystats(fake, 0, 1, C.byref(ok), None) == EINVAL
    self_args = (0, 8, 366, 0, h._fp(rec))
    assert lb.h9g_daystat_selftest(*self_args, None, out.ctypes.data_as(dp)) == EINVAL
    assert lb.h9g_daystat_selftest(*self_args, C.byref(ok), None) == EINVAL
    assert lb.h9g_daystat_selftest(0, 8, 366, 0, None, C.byref(ok), out.ctypes.data_as(dp)) == EINVAL
    assert lb.h9g_daystat_selftest(0, 8, 366, 17, h._fp(rec), C.byref(ok), out.ctypes.data_as(dp)) == EINVAL
    assert lb.h9g_daystat_selftest(0, 0, 366, 0, h._fp(rec), C.byref(ok), out.ctypes.data_as(dp)) == EINVAL
    for k in h.DAYSTAT_THRESHOLDS:
        bad = h.daystat_opts(**dict(HAND_THR, **{k: np.nan}))
        assert lb.h9g_get_daystats(fake, 0, 1, C.byref(bad), out.ctypes.data_as(dp)) == EINVAL
        assert lb.h9g_daystat_selftest(*self_args, C.byref(bad), out.ctypes.data_as(dp)) == EINVAL
    for i in range(4):
        bad = h.daystat_opts(**HAND_THR)
        bad.reserved[i] = 1
        assert lb.h9g_get_daystats(fake, 0, 1, C.byref(bad), out.ctypes.data_as(dp)) == EINVAL
        assert lb.h9g_daystat_selftest(*self_args, C.byref(bad), out.ctypes.data_as(dp)) == EINVAL
    with pytest.raises(TypeError, match="unknown"):
        h.daystat_opts(q_threshold=1.0)
    with pytest.raises(ValueError):
        h.day_stats(np.zeros((3, 6, 2), np.float32))
    assert h.NDAYSTAT == NS == len(h.DAYSTAT_FIELDS)


# ---- 7. the sxy file ------------------------------------------------------------------------
def test_write_sxy_nc_round_trip(tmp_path):
    from scipy.io import netcdf_file
    rec = handmade()
    stats = h.day_stats(rec, **HAND_THR)
    nx, ny = 6, 4
    gid = np.array([0, 3, 5, 7, 11, 12, 18, 23], np.int64)
    path = tmp_path / "sxy1904.nc"
    h.write_sxy_nc(path, stats, gid, 1904, nx=nx, ny=ny, **HAND_THR)
    assert path.read_bytes()[:4] == b"CDF\x02"
    units = dict(zip(h.DAYSTAT_FIELDS, ("days", "mm/day", "day of year (0-based)", "mm/7 days", "days", "mm/day",
                                        "mm", "day of year (0-based)", "mm", "mm^3/mm^3", "days", "days", "mm",
                                        "days", "m^2/m^2", "day of year (0-based)", "days")))
    other = np.setdiff1d(np.arange(nx * ny), gid)
    with netcdf_file(path, "r", mmap=False) as nc:
        assert dict(nc.dimensions) == {"latitude": ny, "longitude": nx}
        assert list(nc.variables) == ["latitude", "longitude", *h.DAYSTAT_FIELDS]
        assert nc.variables["latitude"].units.decode() == "degrees_north"
        assert np.allclose(nc.variables["latitude"][:], 90 - 180 / ny * (np.arange(ny) + 0.5))
        for i, k in enumerate(h.DAYSTAT_FIELDS):
            v = nc.variables[k]
            assert v.dimensions == ("latitude", "longitude") and v.data.dtype == np.dtype(">f8")
            assert v.units.decode() == units[k] and np.isnan(v._FillValue)
            flat = np.array(v[:], np.float64).reshape(-1)
            assert same_bits(flat[gid], stats[i]), k
            assert np.isnan(flat[other]).all()
        assert int(nc.year) == 1904
        for k, want in HAND_THR.items():
            assert np.float32(getattr(nc, k)) == np.float32(want)
    lb = h.lib()
    o = h.daystat_opts(**HAND_THR)
    assert lb.h9g_write_sxy_nc(None, nx, ny, 0, None, 1904, C.byref(o), None) == -1
    assert lb.h9g_write_sxy_nc(str(path).encode(), nx, ny, 0, None, 1904, None, None) == -1
    bad = np.array([nx * ny], np.int64)
    assert lb.h9g_write_sxy_nc(str(path).encode(), nx, ny, 1, bad.ctypes.data_as(C.POINTER(C.c_int64)), 1904,
                               C.byref(o), stats.ctypes.data_as(C.POINTER(C.c_double))) == -1


# ---- a sanitizer build of the same lines, as a program of its own ---------------------------
def test_host_stat_program_under_sanitizers():
    """tests/csrc/host_stat.cpp with its own main, built with
    -fsanitize=address,undefined and run on the CPU: hand-made records through
    one slice, the kernel's cuts and single days."""
    src = ROOT / "tests" / "csrc" / "host_stat.cpp"
    exe = BUILD / "san_host_stat"
    BUILD.mkdir(exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-DHOST_STAT_MAIN", str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 of 8 cuts differ" in r.stdout
