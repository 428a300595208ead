"""The daily diagnostics line (HYBRID9.f90:221-229) without a GPU: the host
build of cell_focus (tests/csrc/host_focus.cpp) against the reference golden
daily_c1 (tests/golden/make_daily_golden.py) and against the oracle's
per-substep trace, bit for bit; and site.focus_window against INIT.f90:220-236.
tests/test_gpu_daily.py then holds the device build to this host build."""
import numpy as np
import pytest

from hybrid9_amd import site, synth
from oracle import port
from tests.conftest import load_golden, same_bits
from tests.daily_helpers import (F, LINE_INDEX, fT_of, host_focus, load_daily_golden, port_daily8, stop_mask_inputs,
                                 w_i_of)

IDX = list(LINE_INDEX)


@pytest.fixture(scope="module")
def golden():
    meta, inp, exp = load_daily_golden()
    return meta, inp, exp, host_focus(**inp)


def test_host_focus_matches_reference_golden(golden):
    """The eight columns the reference's trace determines, all 730 days."""
    meta, inp, exp, out = golden
    assert out["rc"] == 0 and not out["code"].any()
    d = out["daily"]
    assert d.shape == (730, 11, 8)
    for j, k in enumerate(IDX):
        assert same_bits(d[:, k], exp["daily8"][:, j]), meta["columns"][j]


def test_host_focus_fT_and_theta_ma(golden):
    """fT is plain arithmetic on tas (GROW.f90:67-71); theta_ma(1) =
    h2osoi_liq_ma(1) / dz(1) of the state (HYDROLOGY.f90:149), constant."""
    meta, inp, exp, out = golden
    d = out["daily"]
    assert same_bits(d[:, 10], fT_of(inp["forcing"][0]))
    L, n = meta["L"], meta["ncell"]
    zi = inp["zi"]
    ma1 = port.init_state(inp["params"], zi)[n * L:2 * n * L].reshape(n, L)[:, 0]
    want = (ma1 / F(zi[1] - zi[0])).astype(F)
    assert same_bits(d[:, 6], np.broadcast_to(want, (730, n)))


def test_host_focus_w_i_on_the_first_day_of_each_year(golden):
    """w_i (GROW.f90:55-62) from the day's end-of-day smp (the oracle's trace,
    which equals the reference's) and rootr_col as GROW finds it: the start
    state's on day 1 of 1901, the oracle's state after 1901 on day 1 of 1902.
    (Later days' rootr_col are not observable from the oracle; LAI matching
    every day pins them.)"""
    meta, inp, exp, out = golden
    L, n, ns = meta["L"], meta["ncell"], meta["nisurf"]
    kw = {k: inp[k] for k in ("zi", "params", "nisurf", "grow_on")}
    r2 = port.run(forcing=inp["forcing"], year0=1901, nyears=2, trace_cells=tuple(range(n)), nthreads=8, **kw)
    r1 = port.run(forcing=np.ascontiguousarray(inp["forcing"][:, :365]), year0=1901, nyears=1, nthreads=8, **kw)
    root0 = port.init_state(inp["params"], inp["zi"])[3 * n * L:3 * n * L + n * (L + 1)].reshape(n, L + 1)[:, :L]
    for day, root in ((0, root0), (365, r1["state"]["rootr_col"][:, :L])):
        smp = r2["trace"][:, (day + 1) * ns - 1, L:2 * L]
        assert same_bits(out["daily"][day, 9], w_i_of(smp, root)), day
    assert (out["daily"][:, 9] >= 0).all() and (out["daily"][:, 9] <= 1).all()


def _against_port(inp, const_geo=1):
    d8, ref = port_daily8(**inp)
    out = host_focus(const_geo=const_geo, **inp)
    return d8, ref, out


@pytest.mark.parametrize("const_geo", [1, 0])
def test_host_focus_matches_port_on_edge_cells(const_geo):
    meta, inp, _ = load_golden("edge")
    d8, ref, out = _against_port(inp, const_geo)
    assert ref["rc"] == out["rc"] == 0
    assert same_bits(out["daily"][:, IDX], d8)
    assert same_bits(out["daily"][:, 10], fT_of(inp["forcing"][0]))


def test_host_focus_matches_port_l10_ns24():
    g = synth.land_cells(synth.NX025, synth.NY025, synth.NLAND025)[11::1601][:4]
    p = synth.make_params(g, 10)
    f = synth.make_forcing(g, synth.cell_lat(g, synth.NX025, synth.NY025), synth.year_day0(1903), 365)
    inp = dict(zi=synth.ZI_L10, params=p, forcing=f, nisurf=24, year0=1903, nyears=1, grow_on=1)
    d8, ref, out = _against_port(inp)
    assert ref["rc"] == out["rc"] == 0
    assert same_bits(out["daily"][:, IDX], d8)


def test_host_focus_stop_and_masked_cell():
    """NaN from the recorded STOP day on for the failing cell (the reference
    ends before writing that day's line), NaN on every day for a masked cell,
    the other cells complete and equal to the oracle."""
    meta, inp = stop_mask_inputs()
    s = meta["stop"]
    d8, ref, out = _against_port(inp)
    c, day = s["cell"], s["day"]
    assert ref["rc"] == out["rc"] == s["code"] and out["code"][c] == s["code"]
    assert ref["errors"]["day"][c] == day
    d = out["daily"]
    assert np.isnan(d[day:, :, c]).all() and not np.isnan(d[:day, :, c]).any()
    assert np.isnan(d[:, :, 2]).all()
    ok = [k for k in range(meta["ncell"]) if k not in (2, c)]
    assert not np.isnan(d[:, :, ok]).any()
    assert same_bits(d[:, IDX][:, :, ok], d8[:, :, ok])
    # the failing cell before its STOP (LAI after GROW comes from the next
    # day's first substep, so one day less)
    assert same_bits(d[:day, IDX[:6], c], d8[:day, :6, c])
    assert same_bits(d[:day - 1, IDX[6:], c], d8[:day - 1, 6:, c])


def test_host_focus_cell_stopped_before_the_run_has_no_line():
    meta, inp, _ = load_golden("c1_10x10")
    sel = np.arange(0, 100, 33)
    p = {k: v[sel] for k, v in inp["params"].items()}
    f = np.ascontiguousarray(inp["forcing"][:, :, sel])
    out = host_focus(**dict(inp, params=p, forcing=f), failed=[0, 1, 0, 0])
    assert np.isnan(out["daily"][:, :, 1]).all() and not np.isnan(out["daily"][:, :, [0, 2, 3]]).any()


def test_host_focus_without_grow():
    """grow_on = 0: w_i = fT = 0, LAI and LAI_litter stay (the site path's convention)."""
    meta, inp, _ = load_daily_golden()
    f = np.ascontiguousarray(inp["forcing"][:, :365])
    out = host_focus(**dict(inp, forcing=f, nyears=1, grow_on=0))
    d = out["daily"]
    assert (d[:, 9] == 0).all() and (d[:, 10] == 0).all()
    assert same_bits(d[:, 7], np.broadcast_to(d[0, 7], d[:, 7].shape))
    assert same_bits(d[:, 8], np.broadcast_to(d[0, 8], d[:, 8].shape))


def test_write_window_csv_layout(tmp_path):
    """The reference's header (INIT.f90:888-890, A200), line format
    (2(I5,A1),10(F10.4,A1),F10.4) and order decade -> cell -> year -> day; a
    cell's NaN lines (from its STOP on) are not written."""
    r = np.random.default_rng(3)
    d = r.uniform(-2, 50, (365 + 365 + 365, 11, 2)).astype(np.float32)
    d[365 + 100:, :, 1] = np.nan                       # cell 1 stops on day 101 of 1910
    path = tmp_path / "daily_diag.csv"
    site.write_window_csv(path, d, [[1909, 1910], [1911]], 2)
    lines = path.read_text().split("\n")
    assert lines[0] == site.DAILY_HEADER and len(lines[0]) == 200 and lines[0].endswith("lai_litter, w_i, fT")
    rows = lines[1:-1]
    key = [(int(v[0]), int(v[1])) for v in (ln.split(",") for ln in rows)]
    dec1 = [(y, k) for y in (1909, 1910) for k in range(1, 366)]
    assert key == dec1 + dec1[:365 + 100] + [(1911, k) for k in range(1, 366)]
    assert all(len(ln) == 132 for ln in rows)
    assert rows[0] == "%5d,%5d," % (1909, 1) + ",".join("%10.4f" % x for x in d[0, :, 0])
    assert rows[730] == "%5d,%5d," % (1909, 1) + ",".join("%10.4f" % x for x in d[0, :, 1])


def test_focus_window_indices():
    """INIT.f90:224-234 at 0.5 deg: b_lon = 2, a_lon = 360.5, b_lat = -2,
    a_lat = 180.5, so NINT(118.6) and NINT(103.68)."""
    lon_s, lat_s, gids = site.focus_window(-120.95, 38.41, 1, 1)
    assert (lon_s, lat_s) == (119, 104)
    assert gids.tolist() == [103 * 720 + 118]


def test_focus_window_lists_cells_in_y_x_order():
    lon_s, lat_s, gids = site.focus_window(-120.95, 38.41, 2, 3)
    assert (lon_s, lat_s) == (119, 104)
    assert gids.tolist() == [(y - 1) * 720 + (x - 1) for y in (104, 105, 106) for x in (119, 120)]
    # a small grid: 20 x 10 cells of 18 degrees, centres -171 .. 171 and 81 .. -81
    lon_s, lat_s, gids = site.focus_window(-9.0, 9.0, 2, 2, nx=20, ny=10)
    assert (lon_s, lat_s) == (10, 5)
    assert gids.tolist() == [4 * 20 + 9, 4 * 20 + 10, 5 * 20 + 9, 5 * 20 + 10]
