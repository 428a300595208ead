"""Day records without a GPU: the host build of cell_year_pair with the day
kernels' policies (tests/csrc/host_days.cpp) against the day record of
include/h9g.h restated in numpy float32 over the oracle's per-substep trace
(tests/days_helpers.py), bit for bit on all seven rows; the forced-re-run
build; the ties of rows 0 and 1 to the annual means and the month-end
snapshots; the STOP and mask conventions; day_values against a plain double
loop; write_dxy_nc read back."""
import numpy as np
import pytest

import hybrid9_amd as h
from oracle import port
from tests.conftest import load_golden, same_bits
from tests.daily_helpers import stop_mask_inputs
from tests.days_helpers import MAXD, ND, check_ties, day_values_loop, host_days, port_days
from tests.evap_helpers import host_evap
from tests.monthly_helpers import l10_inputs

F = np.float32


@pytest.fixture(scope="module")
def leap():
    """c1_2yr_leap (17 cells, 1903-1904, GROW on): inputs, the records from the
    oracle's trace, and the oracle's run."""
    meta, inp, exp = load_golden("c1_2yr_leap")
    rec, ref = port_days(**inp)
    return meta, inp, exp, rec, ref


def land_of(inp):
    return np.array([port._mask_sum(t) > F(1.0e-8) for t in inp["params"]["theta_s"]])


def check_against(out, rec, base, inp):
    """out (host_days) has the records rec on every land cell and NaN on the
    others; annual means, snapshots, state and STOP records are the ET host
    build's (base); the two ties hold."""
    assert out["rc"] == base["rc"] == 0
    assert out["days"].shape == rec.shape == (inp["nyears"], MAXD, ND, land_of(inp).size)
    land = land_of(inp)
    for r in range(ND):
        assert same_bits(out["days"][:, :, r][..., land], rec[:, :, r][..., land]), f"row {r}"
    assert np.isnan(out["days"][..., ~land]).all()
    assert same_bits(out["annual"], base["annual"]) and same_bits(out["monthly"], base["monthly"])
    assert same_bits(out["state"], base["state"]) and np.array_equal(out["err"], base["err"])
    assert check_ties(out["days"], out["annual"], out["monthly"], inp["year0"], inp["nisurf"]) > 0


@pytest.mark.parametrize("const_geo", [1, 0])
def test_host_days_match_trace_leap(leap, const_geo):
    meta, inp, exp, rec, ref = leap
    assert ref["rc"] == 0 and same_bits(ref["annual"], exp["annual"])
    out = host_days(const_geo=const_geo, **inp)
    check_against(out, rec, host_evap(const_geo=const_geo, **inp), inp)
    assert same_bits(out["state"], exp["state"])
    # 1903 has 365 days, 1904 has 366: day 366 exists in the leap year only
    assert np.isnan(out["days"][0, 365]).all() and np.isfinite(out["days"][1, 365]).all()
    # GROW is on: the LAI of the records moves, and the records hold what the
    # issue describes (cumulative sums that grow, a water table below ground)
    d = out["days"]
    assert (np.ptp(d[0, :365, 6], axis=0) > 0).any()
    assert (d[1, 365, 1] > 100.0).all() and (d[1, 365, 1] > d[1, 30, 1]).all()


def test_host_days_without_monthly_rows(leap):
    """M = null (no monthly recording): the same records."""
    meta, inp, exp, rec, ref = leap
    out = host_days(monthly=False, **inp)
    assert out["rc"] == 0 and out["monthly"] is None
    assert same_bits(out["days"], rec) and same_bits(out["state"], exp["state"])


@pytest.mark.parametrize("const_geo", [1, 0])
def test_host_days_golden_edge(const_geo):
    meta, inp, exp = load_golden("edge")
    rec, ref = port_days(**inp)
    out = host_days(const_geo=const_geo, **inp)
    check_against(out, rec, host_evap(const_geo=const_geo, **inp), inp)


@pytest.mark.parametrize("const_geo", [1, 0])
def test_host_days_l10_ns24(const_geo):
    inp = l10_inputs(4)
    rec, ref = port_days(**inp)
    assert ref["rc"] == 0
    out = host_days(const_geo=const_geo, **inp)
    check_against(out, rec, host_evap(const_geo=const_geo, **inp), inp)


@pytest.mark.parametrize("case", ["leap", "l10"])
def test_forced_rerun_build_gives_the_same_records(leap, case):
    """-DH9G_FORCE_RERUN=5: the exact replay from the day snapshot runs in
    about every other eligible substep; the records are taken after the day's
    last substep and are every bit the ordinary build's."""
    inp = leap[1] if case == "leap" else l10_inputs(4)
    a = host_days(**inp)
    b = host_days(rerun=5, **inp)
    assert a["rc"] == b["rc"] == 0
    # as tests/test_evap_host.py: the forced build must replay, and often
    n = inp["params"]["fmax"].size
    print("exact re-runs (runs, substeps): ordinary", a["exact"], "forced", b["exact"])
    assert b["exact"][0] >= 10 * n and b["exact"][0] > 10 * a["exact"][0], (a["exact"], b["exact"])
    assert b["exact"][1] > b["exact"][0]
    assert same_bits(a["days"], b["days"])
    assert same_bits(a["annual"], b["annual"]) and same_bits(a["monthly"], b["monthly"])
    assert same_bits(a["state"], b["state"])


def test_host_days_stop_and_masked_cell():
    """Finite before the STOP day, NaN from it on and in the later year; the
    masked cell NaN throughout; the other cells complete."""
    meta, inp = stop_mask_inputs()
    s = meta["stop"]
    out = host_days(**inp)
    c = s["cell"]
    assert out["rc"] == s["code"] and out["err"][c, 0] == s["code"]
    ys, e = out["err"][c, 1], out["err"][c, 2]
    d = out["days"]
    assert np.isfinite(d[:ys, :365, :, c]).all() and np.isfinite(d[ys, :e, :, c]).all()
    assert np.isnan(d[ys, e:, :, c]).all() and np.isnan(d[ys + 1:, :, :, c]).all()
    assert e > 0 or ys > 0, "the fixture must leave some records before the STOP"
    assert np.isnan(d[..., 2]).all()
    rest = [k for k in range(meta["ncell"]) if k not in (c, 2)]
    for y in range(inp["nyears"]):
        nt = port._days(inp["year0"] + y)
        assert np.isfinite(d[y, :nt][..., rest]).all() and np.isnan(d[y, nt:]).all()
    base = host_evap(**inp)
    assert same_bits(out["annual"], base["annual"]) and np.array_equal(out["err"], base["err"])
    assert check_ties(d, out["annual"], out["monthly"], inp["year0"], inp["nisurf"]) > 0


# ---- day_values, write_dxy_nc --------------------------------------------------
def _records(nday=366, n=5, seed=5):
    r = np.random.default_rng(seed)
    rec = r.uniform(0.5, 40.0, (nday, ND, n)).astype(F)
    rec[:, :2] = np.cumsum(r.uniform(0.0, 9.0, (nday, 2, n)), axis=0).astype(F)
    return rec


def test_day_values_against_a_plain_double_loop():
    rec = _records(40)
    rec[25:, :, 3] = np.nan              # a cell that stopped on day 25
    got = h.day_values(rec)
    assert got.dtype == np.float32 and got.shape == rec.shape
    assert same_bits(got, day_values_loop(rec))
    assert same_bits(got[:, 2:], rec[:, 2:])
    assert same_bits(got[0, :2], rec[0, :2])          # S[-1] = 0
    assert np.isnan(got[25:, :, 3]).all() and np.isfinite(got[:25, :, 3]).all()
    with pytest.raises(ValueError):
        h.day_values(rec[:, :5])


@pytest.mark.parametrize("jyear,nday", [(1904, 366), (1903, 365)])
def test_write_dxy_nc_roundtrip(tmp_path, jyear, nday):
    from scipy.io import netcdf_file
    nx, ny, L = 10, 10, 8
    gid = np.array([3, 17, 40, 71, 99], np.int64)
    rec = _records(nday, gid.size)
    rec[200:, :, 2] = np.nan             # a cell that stopped on day 200
    zc = np.arange(1, L + 1, dtype=F) * F(10.5)
    path = tmp_path / f"dxy{jyear}.nc"
    h.write_dxy_nc(path, rec, gid, zc, jyear, nx=nx, ny=ny)
    val = h.day_values(rec)
    rows = {"runoff": (0, "mm/day"), "evapotranspiration": (1, "mm/day"), "soil_water": (2, "mm"),
            "soil_water_top_layer": (3, "mm^3/mm^3"), "water_table_depth": (4, "mm"), "aquifer_water": (5, "mm"),
            "LAI": (6, "m^2/m^2")}
    assert path.read_bytes()[:4] == b"CDF\x02"
    with netcdf_file(path, "r", mmap=False) as nc:
        assert nc.dimensions["time"] == nday and nc.dimensions["latitude"] == ny and nc.dimensions["longitude"] == nx
        assert nc.variables["time"].units.decode() == f"days since {jyear}-01-01"
        assert same_bits(nc.variables["time"][:], np.arange(nday, dtype=F))
        assert nc.variables["latitude"].units.decode() == "degrees_north"
        assert same_bits(nc.variables["layer_centre_depth"][:], zc)
        other = np.setdiff1d(np.arange(nx * ny), gid)
        for name, (row, units) in rows.items():
            v = nc.variables[name]
            assert v.units.decode() == units and np.isnan(v._FillValue)
            assert v.dimensions == ("time", "latitude", "longitude")
            flat = np.array(v[:]).reshape(nday, -1)
            assert same_bits(flat[:, gid], val[:, row]), name
            assert np.isnan(flat[:, other]).all()
    lb = h.lib()
    assert lb.h9g_write_dxy_nc(None, 4, 4, 8, None, 0, None, 1901, 365, None) == -1
    assert lb.h9g_write_dxy_nc(str(path).encode(), nx, ny, L, None, 0, None, 1903, 366, None) == -1   # no day 366


def test_days_entry_points_reject_null():
    lb = h.lib()
    assert lb.h9g_set_days(None, 1) == -1
    assert lb.h9g_get_days(None, 0, None) == -1
    assert h.NDAYREC == ND == len(h.DAY_FIELDS)
