"""Monthly output without a GPU: the host build of cell_year_pair with the
Months policy (tests/csrc/host_monthly.cpp) against the month-end snapshots
rebuilt from the oracle's per-substep trace, bit for bit; the year-end
invariant (snapshot 11 divided as HYBRID9.f90:263-290 is the annual means);
the STOP and mask conventions; monthly_means; write_mxy_nc read back."""
import ctypes as C

import numpy as np
import pytest

import hybrid9_amd as h
from oracle import port, refcase
from tests.conftest import load_golden, same_bits
from tests.daily_helpers import stop_mask_inputs
from tests.monthly_helpers import (NM, R_NPP, R_PM, R_RNF, annual_from_final, check_year_end, host_monthly, l10_inputs,
                                   month_ends, monthly_lib, port_snapshots, trace_rows)

F = np.float32


@pytest.fixture(scope="module")
def leap():
    """c1_2yr_leap (17 cells, 1903-1904): inputs, golden, the oracle's trace
    rebuilt into snapshots, and the oracle's run."""
    meta, inp, exp = load_golden("c1_2yr_leap")
    snap, ref = port_snapshots(**inp)
    return meta, inp, exp, snap, ref


def test_month_end_calendar():
    """month_end of h9g_pair.h, from nt alone: the month that ends with each day."""
    me = monthly_lib().h9k_month_end
    for y, nt in ((1903, 365), (1904, 366)):
        ends = month_ends(y)
        assert ends[0] == 31 and ends[1] == (60 if nt == 366 else 59) and ends[11] == nt
        for d1 in range(1, nt + 1):
            assert me(d1, nt) == (ends.index(d1) if d1 in ends else -1), (d1, nt)


def test_trace_rebuild_reproduces_the_oracles_annual_means(leap):
    """The helper first: its year-end sums, divided as :263-290, are the
    oracle's annual means (= the golden) in the rows the trace determines."""
    meta, inp, exp, snap, ref = leap
    assert ref["rc"] == 0 and same_bits(ref["annual"], exp["annual"])
    rows = trace_rows(meta["L"])
    for y in range(2):
        a = annual_from_final(snap[y, NM - 1], inp["year0"] + y, inp["nisurf"])
        assert same_bits(a[rows], ref["annual"][y][rows])


@pytest.mark.parametrize("const_geo", [1, 0])
def test_host_snapshots_match_trace_leap(leap, const_geo):
    meta, inp, exp, snap, ref = leap
    out = host_monthly(const_geo=const_geo, **inp)
    assert out["rc"] == 0
    assert same_bits(out["annual"], exp["annual"]) and same_bits(out["state"], exp["state"])
    rows = trace_rows(meta["L"])
    assert same_bits(out["monthly"][:, :, rows], snap[:, :, rows])
    check_year_end(out["monthly"], out["annual"], inp["year0"], inp["nisurf"])
    # 1904 uses the leap month ends: its February snapshot holds 60 days of
    # forcing, 1903's 59 (tas, summed in float32 day by day)
    tas = np.asarray(inp["forcing"], F)[0]
    for y, d0, nd in ((0, 0, 59), (1, 365, 60)):
        s = np.zeros(tas.shape[1], F)
        for d in range(nd):
            s = (s + tas[d0 + d]).astype(F)
        assert same_bits(out["monthly"][y, 1, 4], s)


@pytest.mark.parametrize("const_geo", [1, 0])
def test_host_snapshots_golden_edge(const_geo):
    meta, inp, exp = load_golden("edge")
    out = host_monthly(const_geo=const_geo, **inp)
    assert out["rc"] == 0
    assert same_bits(out["annual"], exp["annual"]) and same_bits(out["state"], exp["state"])
    check_year_end(out["monthly"], out["annual"], inp["year0"], inp["nisurf"])
    snap, ref = port_snapshots(**inp)
    rows = trace_rows(meta["L"])
    assert same_bits(out["monthly"][:, :, rows], snap[:, :, rows])


@pytest.mark.parametrize("const_geo", [1, 0])
def test_host_snapshots_l10_ns24(const_geo):
    inp = l10_inputs()
    snap, ref = port_snapshots(**inp)
    out = host_monthly(const_geo=const_geo, **inp)
    assert ref["rc"] == out["rc"] == 0
    assert same_bits(out["annual"], ref["annual"])
    assert same_bits(out["state"], refcase.pack_state(ref["state"], 10))
    rows = trace_rows(10)
    assert same_bits(out["monthly"][:, :, rows], snap[:, :, rows])
    check_year_end(out["monthly"], out["annual"], 1903, 24)


def test_host_snapshots_without_grow(leap):
    """grow_on = 0: npp_sum stays 0, and plant_mass_sum is the sequential
    float32 sum of the (constant) plant mass."""
    meta, inp, exp, _, _ = leap
    inp = dict(inp, grow_on=0)
    ref = port.run(**{k: v for k, v in inp.items() if k != "state0"}, nthreads=8)
    out = host_monthly(**inp)
    assert ref["rc"] == out["rc"] == 0 and same_bits(out["annual"], ref["annual"])
    check_year_end(out["monthly"], out["annual"], inp["year0"], inp["nisurf"])
    mon = out["monthly"]
    assert same_bits(mon[:, :, R_NPP], np.zeros_like(mon[:, :, R_NPP]))
    pm = refcase.unpack_state(port.init_state(inp["params"], inp["zi"]), meta["ncell"], meta["L"])["plant_mass"]
    pm = np.asarray(pm, F).reshape(-1)
    for y in range(2):
        s, m = np.zeros_like(pm), 0
        ends = month_ends(inp["year0"] + y)
        for d in range(ends[-1]):
            s = (s + pm).astype(F)
            if d + 1 == ends[m]:
                assert same_bits(mon[y, m, R_PM], s)
                m += 1


def test_host_stop_and_masked_cell():
    """A cell that reaches a reference STOP has NaN in all twelve months of
    that year (and later ones); a masked cell throughout; the others complete."""
    meta, inp = stop_mask_inputs()
    s = meta["stop"]
    out = host_monthly(**inp)
    c = s["cell"]
    assert out["rc"] == s["code"] and out["err"][c, 0] == s["code"]
    ys = out["err"][c, 1]
    mon = out["monthly"]
    assert np.isnan(mon[ys:, :, :, c]).all() and not np.isnan(mon[:ys, :, :, c]).any()
    assert np.isnan(mon[:, :, :, 2]).all()
    others = [k for k in range(meta["ncell"]) if k not in (c, 2)]
    assert np.isfinite(mon[:, :, :, others]).all()
    check_year_end(mon, out["annual"], inp["year0"], inp["nisurf"])
    ref = port.run(**{k: v for k, v in inp.items() if k != "state0"}, nthreads=8)
    assert same_bits(out["annual"][:, :, others], ref["annual"][:, :, others])


# ---- monthly_means --------------------------------------------------------
def _snap(L=8, n=5, seed=3):
    r = np.random.default_rng(seed)
    return np.cumsum(r.uniform(0.5, 40.0, (NM, 12 + L, n)), axis=0).astype(F)


@pytest.mark.parametrize("jyear", [1903, 1904, 1900, 2000])
def test_monthly_means_against_float64_restatement(jyear):
    s, nisurf = _snap(), 48
    got = h.monthly_means(s, jyear, nisurf)
    assert got.dtype == np.float32 and got.shape == s.shape
    ends = month_ends(jyear)
    for m in range(NM):
        days = ends[m] - (ends[m - 1] if m else 0)
        for k in range(s.shape[1]):
            prev = s[m - 1, k].astype(np.float64) if m else 0.0
            div = 1.0 if k == R_NPP else float(days * nisurf) if k == R_RNF else float(days)
            assert same_bits(got[m, k], ((s[m, k].astype(np.float64) - prev) / div).astype(F))


def test_monthly_means_telescope_to_the_year():
    """The twelve differences sum back to snapshot 11.  With integer-valued
    snapshots every difference and every partial sum is exact, so the monthly
    totals of row npp (divisor 1) and the means times their divisors add up
    to the year's final sums exactly."""
    r = np.random.default_rng(5)
    s = np.cumsum(r.integers(1, 4000, (NM, 20, 6)), axis=0).astype(F)
    jyear, nisurf = 1904, 48
    got = h.monthly_means(s, jyear, nisurf).astype(np.float64)
    assert np.array_equal(got[:, R_NPP].sum(axis=0), s[NM - 1, R_NPP].astype(np.float64))
    d = np.diff(s.astype(np.float64), axis=0, prepend=0.0)
    assert np.array_equal(d.sum(axis=0), s[NM - 1].astype(np.float64))
    # the other rows: mean * divisor rounds back to the (integer) difference
    days = np.diff(np.array([0] + month_ends(jyear))).astype(np.float64)
    back = np.rint(got[:, 4:] * days[:, None, None])
    assert np.array_equal(back.sum(axis=0), s[NM - 1, 4:].astype(np.float64))


def test_monthly_means_leap_february():
    s = np.zeros((NM, 20, 1), F)
    s[1:] = F(58.0)                     # everything arrives in February
    for jyear, days in ((1903, 28), (1904, 29)):
        got = h.monthly_means(s, jyear, 48)
        assert same_bits(got[1, 4], np.array([np.float64(58.0) / days], np.float64).astype(F))
        assert same_bits(got[1, R_RNF], np.array([np.float64(58.0) / (days * 48)], np.float64).astype(F))
        assert same_bits(got[1, R_NPP], np.array([58.0], F))
        assert same_bits(got[2:], np.zeros_like(got[2:]))
    with pytest.raises(ValueError):
        h.monthly_means(s[:11], 1903, 48)


def test_write_mxy_nc_roundtrip(tmp_path):
    from scipy.io import netcdf_file
    nx, ny, L, nisurf, jyear = 12, 6, 8, 48, 1904
    gid = np.array([3, 17, 40, 71], np.int64)
    s = _snap(L, gid.size)
    s[:, :, 2] = np.nan                 # a stopped cell
    zc = np.arange(1, L + 1, dtype=F) * F(10.5)
    path = tmp_path / "mxy1904.nc"
    h.write_mxy_nc(path, s, gid, zc, jyear, nisurf, nx=nx, ny=ny)
    mean = h.monthly_means(s, jyear, nisurf)
    names = {"net primary production": ("g[DM]/m^2/month", 0), "plant mass": ("g[DM]", 1), "runoff": ("mm/s", 2),
             "evaporation": ("mm/s", 3), "temperature": ("K", 4), "specific_humidity": ("kg[water]/kg[air]", 7),
             "air_pressure": ("Pa", 8), "precipitation": ("kg/m^2/s", 9), "relative_humidity": ("percent", 10),
             "soil_water": ("mm", 11 + L)}
    with netcdf_file(path, "r", mmap=False) as nc:
        assert nc.version_byte == 2
        assert list(nc.dimensions.items()) == [("month", 12), ("latitude", ny), ("longitude", nx),
                                               ("layer_centre_depth", L)]
        assert set(nc.variables) == set(names) | {"latitude", "longitude", "layer_centre_depth", "soil_water_layers"}
        assert same_bits(nc.variables["layer_centre_depth"][:], zc)
        other = np.setdiff1d(np.arange(nx * ny), gid)
        for name, (units, row) in names.items():
            v = nc.variables[name]
            assert v.dimensions == ("month", "latitude", "longitude") and v.units.decode() == units
            assert np.isnan(v._FillValue)
            flat = v[:].reshape(NM, -1)
            assert same_bits(flat[:, gid], mean[:, row]) and np.isnan(flat[:, other]).all()
        v = nc.variables["soil_water_layers"]
        assert v.dimensions == ("month", "latitude", "longitude", "layer_centre_depth")
        assert v.units.decode() == "mm^3/mm^3" and np.isnan(v._FillValue)
        lay = v[:].reshape(NM, nx * ny, L)
        assert same_bits(lay[:, gid], mean[:, 11:11 + L].transpose(0, 2, 1)) and np.isnan(lay[:, other]).all()
    # the annual file's schema is untouched by the shared writer
    axy = tmp_path / "axy1904.nc"
    h.write_axy_nc(axy, s[NM - 1], gid, zc, nx=nx, ny=ny)
    with netcdf_file(axy, "r", mmap=False) as nc:
        assert list(nc.dimensions) == ["latitude", "longitude", "layer_centre_depth"]
        assert nc.variables["net primary production"].units.decode() == "g[DM]/m^2/yr"
        assert same_bits(nc.variables["runoff"][:].reshape(-1)[gid], s[NM - 1, 2])


def test_monthly_entry_points_reject_no_context():
    """Host-only: without a context nothing can have been recorded.  (That
    h9g_get_monthly answers H9G_ESTATE on a context before any run needs a GPU
    to create one: tests/test_gpu_monthly.py.)"""
    lb = h.lib()
    out = np.zeros(4, F)
    assert lb.h9g_get_monthly(None, 0, out.ctypes.data_as(C.POINTER(C.c_float))) == -1
    assert lb.h9g_set_monthly(None, 1) == -1
    assert lb.h9g_write_mxy_nc(None, 4, 4, 8, None, 0, None, 1901, 48, None) == -1
