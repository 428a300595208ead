"""Evapotranspiration output without a GPU: the host build of cell_year_pair
with the ET policies (tests/csrc/host_evap.cpp) against the definition of the
evaporation sum restated in numpy float32 over the oracle's per-substep trace
(tests/evap_helpers.py), bit for bit; the other rows, the state and the STOP
record against the Months host build; the forced-re-run build (the day
snapshot's SV_EVAP); the STOP and mask conventions; water-balance closure;
monthly_means(evap=True); write_mxy_nc(evap=True) read back."""
import numpy as np
import pytest

import hybrid9_amd as h
from oracle import port
from tests.conftest import load_golden, same_bits
from tests.daily_helpers import stop_mask_inputs
from tests.evap_helpers import R_EVAP, host_evap, others, port_evap, water_balance_residual
from tests.monthly_helpers import NM, host_monthly, l10_inputs, month_ends

F = np.float32


@pytest.fixture(scope="module")
def leap():
    """c1_2yr_leap (17 cells, 1903-1904): inputs, the definition over the
    oracle's trace (annual row 3, month-end row 3), and the oracle's run."""
    meta, inp, exp = load_golden("c1_2yr_leap")
    ea, em, ref = port_evap(**inp)
    return meta, inp, exp, ea, em, ref


def check_against(out, ea, em, base, L, year0, nisurf):
    """out (host_evap) has rows 3 = (ea, em), snapshot 11 of row 3 divided by
    nt * nisurf = annual row 3, and everything else = base (host_monthly)."""
    assert out["rc"] == base["rc"]
    assert same_bits(out["annual"][:, R_EVAP], ea)
    assert same_bits(out["monthly"][:, :, R_EVAP], em)
    for y in range(out["annual"].shape[0]):
        nt = port._days(year0 + y)
        assert same_bits((out["monthly"][y, NM - 1, R_EVAP] / F(nt * nisurf)).astype(F), out["annual"][y, R_EVAP])
    o = others(L)
    assert same_bits(out["annual"][:, o], base["annual"][:, o])
    assert same_bits(out["monthly"][:, :, o], base["monthly"][:, :, o])
    assert same_bits(out["state"], base["state"]) and np.array_equal(out["err"], base["err"])


@pytest.mark.parametrize("const_geo", [1, 0])
def test_host_evap_matches_trace_leap(leap, const_geo):
    meta, inp, exp, ea, em, ref = leap
    assert ref["rc"] == 0 and same_bits(ref["annual"], exp["annual"])
    out = host_evap(const_geo=const_geo, **inp)
    check_against(out, ea, em, host_monthly(const_geo=const_geo, **inp), meta["L"], inp["year0"], inp["nisurf"])
    assert same_bits(out["state"], exp["state"])
    # the field is what the issue measured: no negative sum, hundreds of mm a year
    tot = out["monthly"][:, NM - 1, R_EVAP].astype(np.float64)
    assert (tot > 100.0).all() and (tot < 1000.0).all()
    # 1904's leap month ends: February's snapshot is the sum after day 60
    assert not same_bits(out["monthly"][1, 1, R_EVAP], out["monthly"][0, 1, R_EVAP])


def test_host_evap_without_monthly_rows(leap):
    """mon = null (ET without monthly recording): the same annual rows."""
    meta, inp, exp, ea, em, ref = leap
    out = host_evap(monthly=False, **inp)
    assert out["rc"] == 0 and out["monthly"] is None
    assert same_bits(out["annual"][:, R_EVAP], ea) and same_bits(out["state"], exp["state"])


@pytest.mark.parametrize("const_geo", [1, 0])
def test_host_evap_golden_edge(const_geo):
    meta, inp, exp = load_golden("edge")
    ea, em, ref = port_evap(**inp)
    out = host_evap(const_geo=const_geo, **inp)
    check_against(out, ea, em, host_monthly(const_geo=const_geo, **inp), meta["L"], inp["year0"], inp["nisurf"])


@pytest.mark.parametrize("const_geo", [1, 0])
def test_host_evap_l10_ns24(const_geo):
    inp = l10_inputs()
    ea, em, ref = port_evap(**inp)
    out = host_evap(const_geo=const_geo, **inp)
    assert ref["rc"] == out["rc"] == 0
    check_against(out, ea, em, host_monthly(const_geo=const_geo, **inp), 10, 1903, 24)


def test_host_evap_without_grow(leap):
    meta, inp, exp, _, _, _ = leap
    inp = dict(inp, grow_on=0)
    ea, em, ref = port_evap(**inp)
    out = host_evap(**inp)
    assert ref["rc"] == out["rc"] == 0
    check_against(out, ea, em, host_monthly(**inp), meta["L"], inp["year0"], inp["nisurf"])


@pytest.mark.parametrize("case", ["leap", "l10"])
def test_forced_rerun_build_gives_the_same_bits(leap, case):
    """-DH9G_FORCE_RERUN=5: the exact replay from the day snapshot runs in
    about every other eligible substep and must hand the evaporation sum over
    (SV_EVAP) like the runoff sum: every bit of the ordinary build's."""
    inp = leap[1] if case == "leap" else l10_inputs()
    a = host_evap(**inp)
    b = host_evap(rerun=5, **inp)
    assert a["rc"] == b["rc"] == 0
    # the test means something only if the forced build replays, and often: at
    # least ten re-runs per cell (it forces one in every fifth substep of a day
    # whose water table is in the column), several substeps long among them,
    # where the ordinary build has next to none
    n = inp["params"]["fmax"].size
    print("exact re-runs (runs, substeps): ordinary", a["exact"], "forced", b["exact"])
    assert b["exact"][0] >= 10 * n and b["exact"][0] > 10 * a["exact"][0], (a["exact"], b["exact"])
    assert b["exact"][1] > b["exact"][0]
    assert same_bits(a["annual"], b["annual"]) and same_bits(a["monthly"], b["monthly"])
    assert same_bits(a["state"], b["state"])


def test_host_evap_stop_and_masked_cell():
    """Row 3 is NaN from the STOP year on and for the masked cell, finite before."""
    meta, inp = stop_mask_inputs()
    s = meta["stop"]
    out = host_evap(**inp)
    c = s["cell"]
    assert out["rc"] == s["code"] and out["err"][c, 0] == s["code"]
    ys = out["err"][c, 1]
    for rows in (out["annual"][:, R_EVAP], out["monthly"][:, :, R_EVAP]):
        assert np.isnan(rows[ys:, ..., c]).all() and np.isfinite(rows[:ys, ..., c]).all()
        assert np.isnan(rows[..., 2]).all()
        rest = [k for k in range(meta["ncell"]) if k not in (c, 2)]
        assert np.isfinite(rows[..., rest]).all() and (rows[..., rest] > 0).all()
    base = host_monthly(**inp)
    o = others(meta["L"])
    assert same_bits(out["annual"][:, o], base["annual"][:, o]) and np.array_equal(out["err"], base["err"])


def test_water_balance_closes_1904(leap):
    """|P - R - E - dS| <= 2 mm per cell over 1904, from the host build's annual
    rows and the states before and after the year.  (The oracle's trace closes
    to 0.99 mm; the bound allows as much again for f32 sums of 17,568 terms.
    Without either flux the residual is hundreds of mm in vegetated cells.)"""
    meta, inp, exp, _, _, _ = leap
    nd = port._days(1903)
    y1 = host_evap(**dict(inp, nyears=1, forcing=np.ascontiguousarray(inp["forcing"][:, :nd])))
    y2 = host_evap(**inp)
    assert y1["rc"] == y2["rc"] == 0 and same_bits(y1["annual"][0], y2["annual"][0])
    res = water_balance_residual(y2["annual"][1], y1["state"], y2["state"], meta["L"], 1904, inp["nisurf"])
    print("water balance residual 1904, mm per cell:", np.round(res, 3))
    assert np.abs(res).max() <= 2.0
    zero = np.array(y2["annual"][1])
    zero[R_EVAP] = 0
    assert np.abs(water_balance_residual(zero, y1["state"], y2["state"], meta["L"], 1904, inp["nisurf"])).min() > 100.0


# ---- monthly_means, write_mxy_nc ---------------------------------------------
def _snap(L=8, n=5, seed=3):
    r = np.random.default_rng(seed)
    return np.cumsum(r.uniform(0.5, 40.0, (NM, 12 + L, n)), axis=0).astype(F)


@pytest.mark.parametrize("jyear", [1903, 1904, 1900, 2000])
def test_monthly_means_evap_against_float64_restatement(jyear):
    s, nisurf = _snap(), 48
    got = h.monthly_means(s, jyear, nisurf, evap=True)
    assert got.dtype == np.float32 and got.shape == s.shape
    ends = month_ends(jyear)
    for m in range(NM):
        days = ends[m] - (ends[m - 1] if m else 0)
        for k in range(s.shape[1]):
            prev = s[m - 1, k].astype(np.float64) if m else 0.0
            div = 1.0 if k == 0 else float(days * nisurf) if k in (2, R_EVAP) else float(days)
            assert same_bits(got[m, k], ((s[m, k].astype(np.float64) - prev) / div).astype(F))
    # the default keeps today's divisors, and only row 3 differs
    off = h.monthly_means(s, jyear, nisurf)
    assert same_bits(off, h.monthly_means(s, jyear, nisurf, evap=False))
    o = others(s.shape[1] - 12)
    assert same_bits(off[:, o], got[:, o])
    d3 = np.diff(s[:, R_EVAP].astype(np.float64), axis=0, prepend=0.0)
    days = np.diff(np.array([0] + month_ends(jyear))).astype(np.float64)
    assert same_bits(off[:, R_EVAP], (d3 / days[:, None]).astype(F))


def test_write_mxy_nc_evap_roundtrip(tmp_path):
    from scipy.io import netcdf_file
    nx, ny, L, nisurf, jyear = 12, 6, 8, 48, 1904
    gid = np.array([3, 17, 40, 71], np.int64)
    s = _snap(L, gid.size)
    s[:, :, 2] = np.nan                 # a stopped cell
    zc = np.arange(1, L + 1, dtype=F) * F(10.5)
    rows = {"net primary production": 0, "plant mass": 1, "runoff": 2, "evaporation": 3, "temperature": 4,
            "soil_water": 11 + L}
    got = {}
    for evap in (False, True):
        path = tmp_path / f"mxy1904_{int(evap)}.nc"
        h.write_mxy_nc(path, s, gid, zc, jyear, nisurf, nx=nx, ny=ny, evap=evap)
        mean = h.monthly_means(s, jyear, nisurf, evap=evap)
        with netcdf_file(path, "r", mmap=False) as nc:
            assert nc.variables["evaporation"].units.decode() == "mm/s"
            for name, row in rows.items():
                flat = nc.variables[name][:].reshape(NM, -1)
                assert same_bits(flat[:, gid], mean[:, row])
            got[evap] = {k: np.array(v[:]) for k, v in nc.variables.items()}
    assert set(got[False]) == set(got[True])
    for k in got[False]:
        assert same_bits(got[False][k], got[True][k]) == (k != "evaporation"), k


def test_evap_entry_points_reject_null():
    lb = h.lib()
    assert lb.h9g_set_evap(None, 1) == -1
    assert lb.h9g_write_mxy_nc_evap(None, 4, 4, 8, None, 0, None, 1901, 48, None) == -1
