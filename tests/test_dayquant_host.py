"""Day quantiles on the host (no GPU): the three statements of the contract of
include/h9g.h -- hybrid9_amd.day_order_stats (numpy), dayquant_helpers.
order_stats_loop (a per-cell loop that sorts (key, value) pairs) and the host
build of hybrid9_amd/csrc/h9g_quant.h, the lines h9g_dayquant_kernel runs --
agree bit for bit on hand-made records, on random ones and on the oracle's day
records, however the days are cut, for every digit width built and for either
key; the ties to the day statistics; the argument checks that need no device;
the qxy file.  Every comparison is conftest.same_bits: no tolerance."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import hybrid9_amd as h
from tests.conftest import same_bits
from tests.daystat_helpers import golden_records
from tests.dayquant_helpers import (BITS, HAND_NT, NSERIES, QP, check_handmade3, cut_sets, handmade3, host_quant,
                                    kernel_cuts, order_stats_loop, quant_lib, random_years)
from tests.helpers import BUILD, ROOT

GOLDENS = ("c1_2yr_leap", "stop_ns24")
NROWS = 1 + 2 * len(QP)


def _golden_years(name):
    inp, rec = golden_records(name)
    return [rec[y, :h.days_in_year(inp["year0"] + y)] for y in range(inp["nyears"])]


def _three(years, series, pooled, p=QP):
    a = h.day_order_stats(years, series=series, p=p, pooled=pooled)
    b = order_stats_loop(years, series=series, p=p, pooled=pooled)
    c = host_quant(years, series=series, p=p, pooled=pooled)
    assert a.dtype == np.float64 and a.shape == (1 if pooled else len(years), 1 + 2 * len(p), years[0].shape[2])
    assert same_bits(a, b), f"series {series} pooled {pooled}: day_order_stats and the loop differ"
    assert same_bits(c, b), f"series {series} pooled {pooled}: the host build and the loop differ"
    return b


# ---- 1. three statements, one answer, on hand-made records --------------------------
@pytest.mark.parametrize("series", range(NSERIES))
def test_three_statements_agree_on_handmade_records(series):
    years = handmade3()
    assert tuple(r.shape[0] for r in years) == HAND_NT
    per_year, pooled = _three(years, series, False), _three(years, series, True)
    check_handmade3(per_year, pooled, series)
    assert same_bits(pooled[0, 0], per_year[:, 0].sum(axis=0))
    # by name as by number
    assert same_bits(h.day_order_stats(years, series=h.DAYQUANT_SERIES[series], p=QP), per_year)


@pytest.mark.parametrize("series", (0, 3, 4))
def test_cut_digit_width_and_key_do_not_matter(series):
    """Every digit width built, both keys for the record rows, the kernel's
    cuts for every workgroup built, single days, random cuts, slices visited
    in either order: the same bits."""
    years = handmade3()
    for pooled in (False, True):
        want = order_stats_loop(years, series=series, p=QP, pooled=pooled)
        for bits in BITS:
            for key64 in (False, True):
                for label, cuts in cut_sets(366, seed=series, nrandom=2):
                    for rev in (False, True):
                        got = host_quant(years, series=series, p=QP, pooled=pooled, cuts=cuts, rev=rev, bits=bits,
                                         key64=key64)
                        assert same_bits(got, want), (series, pooled, bits, key64, label, rev)


def test_kernel_cuts_are_even_slices():
    for nt in (365, 366):
        for w in (4, 8, 16):
            cu = kernel_cuts(nt, w)
            edges = np.concatenate([[0], cu, [nt]])
            assert cu.size == w - 1 and set(np.diff(edges)) <= {nt // w, nt // w + 1}
    assert kernel_cuts(3, 16).size == 2           # more slices than days: the empty ones vanish


def test_short_years_and_single_quantiles():
    years = handmade3()
    for nt in (1, 2, 6):
        short = [r[:nt] for r in years]
        for series in (0, 2):
            for pooled in (False, True):
                _three(short, series, pooled)
    for p in ((0.0,), (1.0,), (0.5,), tuple(np.linspace(0, 1, 16))):
        _three(years, 0, True, p)
        _three(years, 6, False, p)


# ---- 2. random records: many ties, NaN tails --------------------------------------------
@pytest.mark.parametrize("pooled", (False, True))
def test_random_records_with_nan_tails(pooled):
    years = random_years(40, 11)
    for series in range(NSERIES):
        b = _three(years, series, pooled)
        nt = sum(HAND_NT) if pooled else HAND_NT[0]
        assert (b[0, 0] == 0).any() and (b[0, 0] == nt).any() and ((b[0, 0] > 0) & (b[0, 0] < nt)).any()
    for bits in BITS:
        for key64 in (False, True):
            got = host_quant(years, series=4, p=QP, pooled=pooled, cuts=kernel_cuts(366, 8), bits=bits, key64=key64)
            assert same_bits(got, order_stats_loop(years, series=4, p=QP, pooled=pooled))


# ---- 3. the oracle's records ----------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_three_statements_agree_on_oracle_records(name):
    years = _golden_years(name)
    med = 1 + 2 * QP.index(0.5)
    for series in range(NSERIES):
        per_year = _three(years, series, False)
        pooled = _three(years, series, True)
        assert same_bits(pooled[0, 0], per_year[:, 0].sum(axis=0))
        if h.DAYQUANT_SERIES[series] in ("q", "theta1", "zwt", "LAI"):
            # the goldens show something: the median lies strictly between the extremes
            ran = per_year[:, 0] > 0
            mid = ran & (per_year[:, med] > per_year[:, 1]) & (per_year[:, med] < per_year[:, 1 + 2 * QP.index(1.0)])
            print(f"{name}: median of {h.DAYQUANT_SERIES[series]} strictly between min and max in "
                  f"{int(mid.sum())} of {int(ran.sum())} cell-years")
            assert mid.sum() * 2 >= ran.sum() > 0
    if name == "c1_2yr_leap":
        assert [r.shape[0] for r in years] == [365, 366]
    if name == "stop_ns24":
        m = h.day_order_stats(years, series=0, p=QP)[0, 0]
        stopped = np.flatnonzero((m > 0) & (m < 365))
        assert stopped.size == 1 and m[2] == 0                   # one cell stops; cell 2 is masked


# ---- 4. ties to the day statistics --------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS + ("random",))
def test_extreme_quantiles_are_the_day_statistics(name):
    """Per year, p = 0 and p = 1 reproduce day_stats' extremes bit for bit; on
    product records m equals ndays."""
    years = random_years(30, 5) if name == "random" else _golden_years(name)
    f = {k: i for i, k in enumerate(h.DAYSTAT_FIELDS)}
    ties = (("q", 1, "q_max"), ("e", 1, "e_max"), ("soil_water", 0, "w_min"), ("soil_water", 1, "w_max"),
            ("theta1", 0, "theta1_min"), ("zwt", 0, "zwt_min"), ("LAI", 1, "lai_max"))
    for y, r in enumerate(years):
        st = h.day_stats(r)
        for series, p, row in ties:
            q = h.day_order_stats([r], series=series, p=(float(p),))[0]
            assert same_bits(q[1], st[f[row]]), (name, y, series, row)
            assert p == 0 or same_bits(q[2], st[f[row]]), (name, y, series, row)      # (above the largest: itself)
            if name != "random":
                assert same_bits(q[0], st[f["ndays"]])


# ---- 5. the host interpolation --------------------------------------------------------------
def test_day_quantiles_interpolates_as_numpy_does():
    rng = np.random.default_rng(2)
    rec = np.zeros((365, 7, 6), np.float32)
    rec[:, 3] = rng.random((365, 6))
    p = (0.05, 0.5, 0.95, 0.0, 1.0, 0.2)
    q = h.day_order_stats([rec], series="theta1", p=p)
    v = h.day_quantiles(q, p)
    assert v.shape == (1, len(p), 6)
    want = np.quantile(rec[:, 3].astype(np.float64), p, axis=0)
    # both are one multiply-add from the same two order statistics: a few ulp of values in (0, 1)
    assert np.abs(v[0] - want).max() <= 4 * np.finfo(np.float64).eps
    exact = [p.index(0.0), p.index(1.0)]
    assert same_bits(v[0][exact], want[exact])
    # an infinite order statistic stays one; no candidate: NaN
    q2 = np.array([[[4.0, 0.0]], [[np.inf, np.nan]], [[np.inf, np.nan]]]).reshape(1, 3, 2)
    assert h.day_quantiles(q2, (0.5,))[0, 0, 0] == np.inf and np.isnan(h.day_quantiles(q2, (0.5,))[0, 0, 1])


# ---- 6. argument checks that need no device ------------------------------------------------
def _bad_opts():
    ok = dict(series=0, p=(0.5,), pooled=False)
    bad = []
    for s in (-1, 7):
        o = h.dayquant_opts(**ok)
        o.series = s
        bad.append((f"series {s}", o))
    for nq in (0, 17, -3):
        o = h.dayquant_opts(**ok)
        o.nq = nq
        bad.append((f"nq {nq}", o))
    for p in (-0.001, 1.001, np.nan, np.inf):
        o = h.dayquant_opts(series=0, p=(0.2, 0.5, 0.7))
        o.p[2] = p
        bad.append((f"p {p}", o))
    for v in (2, -1):
        o = h.dayquant_opts(**ok)
        o.pooled = v
        bad.append((f"pooled {v}", o))
    o = h.dayquant_opts(**ok)
    o.reserved = 1
    bad.append(("reserved", o))
    return bad


def test_argument_checks_without_a_device():
    lb = h.lib()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    nt = np.array([2, 3], np.int32)
    rec = np.zeros((2, 3, 7, 4), np.float32)
    out = np.zeros((2, 3, 4), np.float64)
    ok = h.dayquant_opts(series=0, p=(0.5,))
    EINVAL = -1
    fake = C.c_void_p(1)                          # (never dereferenced: the options are checked first)
    self_args = (0, 4, 2, nt.ctypes.data_as(ip), 0, h._fp(rec))
    assert quant_lib().h9k_host_quant_opts_ok(C.byref(ok)) == 1
    for what, bad in _bad_opts():
        assert quant_lib().h9k_host_quant_opts_ok(C.byref(bad)) == 0, what
        assert lb.h9g_get_dayquant(fake, 0, 1, C.byref(bad), out.ctypes.data_as(dp)) == EINVAL, what
        assert lb.h9g_dayquant_selftest(*self_args, C.byref(bad), out.ctypes.data_as(dp)) == EINVAL, what
    assert lb.h9g_get_dayquant(None, 0, 1, C.byref(ok), out.ctypes.data_as(dp)) == EINVAL
    assert lb.h9g_get_dayquant(fake, 0, 1, None, out.ctypes.data_as(dp)) == EINVAL
    assert lb.h9g_get_dayquant(fake, 0, 1, C.byref(ok), None) == EINVAL
    assert lb.h9g_dayquant_selftest(*self_args, None, out.ctypes.data_as(dp)) == EINVAL
    assert lb.h9g_dayquant_selftest(*self_args, C.byref(ok), None) == EINVAL
    assert lb.h9g_dayquant_selftest(0, 4, 2, None, 0, h._fp(rec), C.byref(ok), out.ctypes.data_as(dp)) == EINVAL
    assert lb.h9g_dayquant_selftest(0, 4, 2, nt.ctypes.data_as(ip), 0, None, C.byref(ok),
                                    out.ctypes.data_as(dp)) == EINVAL
    for n, ny, nseg in ((0, 2, 0), (4, 0, 0), (4, 513, 0), (4, 2, 17), (4, 2, -1)):
        assert lb.h9g_dayquant_selftest(0, n, ny, nt.ctypes.data_as(ip), nseg, h._fp(rec), C.byref(ok),
                                        out.ctypes.data_as(dp)) == EINVAL, (n, ny, nseg)
    zero = np.array([2, 0], np.int32)
    assert lb.h9g_dayquant_selftest(0, 4, 2, zero.ctypes.data_as(ip), 0, h._fp(rec), C.byref(ok),
                                    out.ctypes.data_as(dp)) == EINVAL
    assert lb.h9g_last_dayquant_ms(None) == 0.0
    with pytest.raises(ValueError, match="unknown day-quantile series"):
        h.dayquant_opts(series="runoff", p=(0.5,))
    with pytest.raises(ValueError):
        h.dayquant_opts(series=0, p=np.linspace(0, 1, 17))
    with pytest.raises(ValueError):
        h.day_order_stats([np.zeros((3, 6, 2), np.float32)], series=0, p=(0.5,))
    assert h.NQUANT_MAX == 16 and len(h.DAYQUANT_SERIES) == NSERIES == h.NDAYREC


def test_symbols_are_declared_exported_and_bound():
    names = ("h9g_get_dayquant", "h9g_last_dayquant_ms", "h9g_dayquant_selftest", "h9g_write_qxy_nc")
    declared = h.exported_symbols()
    f90 = (ROOT / "hybrid9_amd" / "fortran" / "h9_gpu.f90").read_text()
    for name in names:
        assert name in declared
        assert getattr(h.lib(), name).argtypes is not None
        assert re.search(rf"BIND\(C,\s*NAME='{name}'\)", f90), name
    hdr = (ROOT / "include" / "h9g.h").read_text()
    assert "#define H9G_NQUANT_MAX 16" in hdr and "h9g_dayquant_opts" in f90
    assert C.sizeof(h._QuantOpts) == 16 + 8 * 16


# ---- 7. the qxy file ------------------------------------------------------------------------
@pytest.mark.parametrize("pooled", (False, True))
def test_write_qxy_nc_round_trip(tmp_path, pooled):
    from scipy.io import netcdf_file
    years = handmade3()
    quant = h.day_order_stats(years, series="zwt", p=QP, pooled=pooled)[0]
    n = quant.shape[1]
    nx, ny = 6, 4
    gid = np.array([0, 3, 5, 7, 11, 12, 18, 23, 1, 2, 4, 6, 8], np.int64)
    path = tmp_path / ("qxy1901_1903.nc" if pooled else "qxy1901.nc")
    h.write_qxy_nc(path, quant, gid, 1901, 1903 if pooled else None, nx=nx, ny=ny, series="zwt", p=QP, pooled=pooled)
    assert path.read_bytes()[:4] == b"CDF\x02"
    other = np.setdiff1d(np.arange(nx * ny), gid)
    value = h.day_quantiles(quant, QP)
    with netcdf_file(path, "r", mmap=False) as nc:
        assert dict(nc.dimensions) == {"quantile": len(QP), "latitude": ny, "longitude": nx}
        assert list(nc.variables) == ["latitude", "longitude", "p", "count", "lower", "upper", "value"]
        assert nc.variables["latitude"].units.decode() == "degrees_north"
        assert np.allclose(nc.variables["latitude"][:], 90 - 180 / ny * (np.arange(ny) + 0.5))
        assert same_bits(np.array(nc.variables["p"][:], np.float64), np.array(QP))
        cnt = nc.variables["count"]
        assert cnt.dimensions == ("latitude", "longitude") and cnt.data.dtype == np.dtype(">f8")
        flat = np.array(cnt[:], np.float64).reshape(-1)
        assert same_bits(flat[gid], quant[0]) and np.isnan(flat[other]).all()
        for k, want in (("lower", quant[1::2]), ("upper", quant[2::2]), ("value", value)):
            v = nc.variables[k]
            assert v.dimensions == ("quantile", "latitude", "longitude") and v.data.dtype == np.dtype(">f8")
            assert v.units.decode() == "mm" and np.isnan(v._FillValue)
            got = np.array(v[:], np.float64).reshape(len(QP), -1)
            assert same_bits(got[:, gid], want), k
            assert np.isnan(got[:, other]).all()
        assert nc.series.decode() == "zwt" and int(nc.year_first) == 1901
        assert int(nc.year_last) == (1903 if pooled else 1901) and int(nc.pooled) == int(pooled)
    lb = h.lib()
    o = h.dayquant_opts(series="zwt", p=QP)
    dp = C.POINTER(C.c_double)
    assert lb.h9g_write_qxy_nc(None, nx, ny, 0, None, 1901, 1901, C.byref(o), None) == -1
    assert lb.h9g_write_qxy_nc(str(path).encode(), nx, ny, 0, None, 1901, 1901, None, None) == -1
    assert lb.h9g_write_qxy_nc(str(path).encode(), nx, ny, 0, None, 1902, 1901, C.byref(o), None) == -1
    bad = np.array([nx * ny], np.int64)
    assert lb.h9g_write_qxy_nc(str(path).encode(), nx, ny, 1, bad.ctypes.data_as(C.POINTER(C.c_int64)), 1901, 1901,
                               C.byref(o), quant.ctypes.data_as(dp)) == -1
    assert n == gid.size


# ---- a sanitizer build of the same lines, as a program of its own ---------------------------
def test_host_quant_program_under_sanitizers():
    """tests/csrc/host_quant.cpp with its own main, built with
    -fsanitize=address,undefined and run on the CPU: three years of records,
    every series, per year and pooled, every digit width, both keys, several cuts."""
    src = ROOT / "tests" / "csrc" / "host_quant.cpp"
    exe = BUILD / "san_host_quant"
    BUILD.mkdir(exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-DHOST_QUANT_MAIN", str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"host_quant: 0 of \d+ runs differ", r.stdout)
