"""Day quantiles on the GPU: h9g_dayquant_kernel gives, for hand-made records
and for the records of both run modes, the order statistics of include/h9g.h
as the per-cell sorting loop (dayquant_helpers.order_stats_loop) and
hybrid9_amd.day_order_stats give them, bit for bit, however a year is cut into
slices; and calling it changes nothing else.  Every comparison is
conftest.same_bits: no tolerance.  Runs on an MI355X only."""
import subprocess

import numpy as np
import pytest

import hybrid9_amd as h
from oracle import refcase
from tests.conftest import load_golden, same_bits
from tests.daily_helpers import stop_mask_inputs
from tests.daystat_helpers import golden_records
from tests.dayquant_helpers import (BITS, HAND_NT, NSERIES, QP, check_handmade3, handmade3, order_stats_loop,
                                    random_years)

pytestmark = pytest.mark.gpu

NROWS = 1 + 2 * len(QP)
NSEGS = (0, 1, 3, 4, 8, 16)
_cache = {}


def _once(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _want(name, years, series, pooled):
    return _once((name, series, pooled), lambda: order_stats_loop(years, series=series, p=QP, pooled=pooled))


# ---- 1. the kernel on the hand-made three years ----------------------------------
@pytest.mark.parametrize("series", range(NSERIES))
def test_selftest_handmade_records(series):
    years = handmade3()
    per_year, pooled = _want("hand", years, series, False), _want("hand", years, series, True)
    check_handmade3(per_year, pooled, series)
    for pool, want in ((False, per_year), (True, pooled)):
        for nseg in NSEGS:
            got = h.dayquant_selftest(years, series=series, p=QP, pooled=pool, nseg=nseg)
            assert got.shape == want.shape and got.dtype == np.float64
            assert same_bits(got, want), f"series {series} pooled {pool} nseg {nseg}: rows " \
                f"{[i for i in range(NROWS) if not same_bits(got[:, i], want[:, i])]}"


def test_selftest_short_years_and_empty_slices():
    years = handmade3()
    for nt in (1, 2, 6):                          # fewer days than slices: empty slices
        short = [r[:nt] for r in years]
        for series in (0, 3):
            for pool in (False, True):
                want = order_stats_loop(short, series=series, p=QP, pooled=pool)
                for nseg in (0, 1, 16):
                    got = h.dayquant_selftest(short, series=series, p=QP, pooled=pool, nseg=nseg)
                    assert same_bits(got, want), (nt, series, pool, nseg)
    uneven = [years[0][:1], years[1][:6], years[2][:2]]          # years of unequal lengths
    for pool in (False, True):
        assert same_bits(h.dayquant_selftest(uneven, series=0, p=QP, pooled=pool, nseg=16),
                         order_stats_loop(uneven, series=0, p=QP, pooled=pool))
    with pytest.raises(ValueError):
        h.dayquant_selftest(years, series=0, p=QP, nseg=17)


def test_selftest_every_variant_built(monkeypatch):
    """Every digit width built, and the 64-bit key for a record row: the same bits."""
    years = handmade3()
    for series in (0, 4):
        for pool in (False, True):
            want = _want("hand", years, series, pool)
            for bits in BITS:
                for key64 in ("0", "1"):
                    monkeypatch.setenv("H9G_DAYQUANT_BITS", str(bits))
                    monkeypatch.setenv("H9G_DAYQUANT_KEY64", key64)
                    for nseg in (0, 16):
                        got = h.dayquant_selftest(years, series=series, p=QP, pooled=pool, nseg=nseg)
                        assert same_bits(got, want), (series, pool, bits, key64, nseg)
    # more ranks than a launch selects at once
    p16 = tuple(np.linspace(0, 1, 16))
    for bits in BITS:
        monkeypatch.setenv("H9G_DAYQUANT_BITS", str(bits))
        monkeypatch.setenv("H9G_DAYQUANT_KEY64", "0")
        assert same_bits(h.dayquant_selftest(years, series=6, p=p16, pooled=True),
                         order_stats_loop(years, series=6, p=p16, pooled=True)), bits


@pytest.mark.parametrize("pooled", (False, True))
def test_selftest_random_cells_and_tail_workgroups(pooled):
    """200 cells with NaN tails of random length; n = 1, 63, 64, 65, 200: a lone
    lane, a workgroup one lane short, full, one lane into the next, several."""
    years = random_years(200, 21)
    for series in (0, 4):
        want = _want("rand", years, series, pooled)
        nt = sum(HAND_NT) if pooled else HAND_NT[0]
        assert (want[0, 0] == 0).any() and (want[0, 0] == nt).any() and ((want[0, 0] > 0) & (want[0, 0] < nt)).any()
        for n in (1, 63, 64, 65, 200):
            sub = [np.ascontiguousarray(r[:, :, :n]) for r in years]
            for nseg in (0, 3):
                got = h.dayquant_selftest(sub, series=series, p=QP, pooled=pooled, nseg=nseg)
                assert same_bits(got, want[:, :, :n]), (series, n, nseg)


# ---- 2. isolated mode ------------------------------------------------------------------
def test_isolated_years_match_records_and_oracle():
    meta, inp, _ = load_golden("c1_2yr_leap")
    _, rec = golden_records("c1_2yr_leap")
    n = meta["ncell"]
    f = {k: i for i, k in enumerate(h.DAYSTAT_FIELDS)}
    with h.Context(n, inp["zi"], nisurf=inp["nisurf"]) as ctx:
        ctx.set_params(inp["params"])
        ctx.init_state()
        ctx.set_evap(True)
        ctx.set_days(True)
        with pytest.raises(h.H9GError, match="nothing recorded"):
            ctx.get_dayquant(series="q", p=QP)
        assert ctx.last_dayquant_ms() == 0.0
        d0 = 0
        for y in range(2):
            nt = h.days_in_year(inp["year0"] + y)
            ctx.push_forcing(y, inp["forcing"][:, d0:d0 + nt])
            ctx.run_year(y, inp["year0"] + y)
            ctx.sync()
            d0 += nt
            days = ctx.get_days()
            assert days.shape[0] == nt
            st = ctx.get_daystats()[0]
            for series in range(NSERIES):
                got = ctx.get_dayquant(series=series, p=QP)
                assert got.shape == (1, NROWS, n) and got.dtype == np.float64
                assert same_bits(got, h.day_order_stats([days], series=series, p=QP)), (y, series)
                assert same_bits(got, order_stats_loop([rec[y, :nt]], series=series, p=QP)), (y, series)
                assert (got[0, 0] == nt).all() and same_bits(got[0, 0], st[f["ndays"]])
                assert same_bits(ctx.get_dayquant(series=series, p=QP, pooled=True), got)     # a span of one year
            i0, i1 = 1 + 2 * QP.index(0.0), 1 + 2 * QP.index(1.0)
            for series, i, row in (("q", i1, "q_max"), ("e", i1, "e_max"), ("soil_water", i0, "w_min"),
                                   ("soil_water", i1, "w_max"), ("theta1", i0, "theta1_min"), ("zwt", i0, "zwt_min"),
                                   ("LAI", i1, "lai_max")):
                assert same_bits(ctx.get_dayquant(series=series, p=QP)[0, i], st[f[row]]), (y, series, row)
            for span in ((0, 2), (1, 1), (-1, 1), (0, 0)):
                with pytest.raises(ValueError, match="H9G_EINVAL"):
                    ctx.get_dayquant(*span, series="q", p=QP)
            assert ctx.last_dayquant_ms() > 0
    out = h.run(dayquant=dict(series="zwt", p=QP), **inp)
    assert "days" not in out and out["dayquant"].shape == (2, NROWS, n)
    for y in range(2):
        want = order_stats_loop([rec[y, :h.days_in_year(inp["year0"] + y)]], series="zwt", p=QP)
        assert same_bits(out["dayquant"][y], want[0])
    with pytest.raises(ValueError, match="pooled"):
        h.run(dayquant=dict(series="zwt", p=QP, pooled=True), **inp)


# ---- 3. ordered mode -------------------------------------------------------------------
def test_ordered_span_per_year_and_pooled():
    meta, inp, _ = load_golden("co_c1_30yr")
    ny = 12
    nd = sum(h.days_in_year(y) for y in range(1901, 1901 + ny))
    n, L = meta["ncell"], meta["L"]
    assert inp["year0"] == 1901 and n == 100
    p = (0.05, 0.5, 0.95)
    with h.Context(n, inp["zi"], nlayers=L, nisurf=inp["nisurf"], grow_on=inp["grow_on"], nslots=ny) as ctx:
        ctx.set_params(inp["params"])
        ctx.init_state()
        ctx.set_evap(True)
        ctx.set_days(True)
        d0 = 0
        for k in range(ny):
            nt = h.days_in_year(1901 + k)
            ctx.push_forcing(k, inp["forcing"][:, d0:d0 + nt])
            d0 += nt
        assert d0 == nd
        ctx.run_ordered(list(range(ny)), 1901)
        days = [ctx.get_days(k) for k in range(ny)]
        for series in ("q", "zwt"):
            got = ctx.get_dayquant(0, ny, series=series, p=p)
            assert got.shape == (ny, 7, n)
            assert same_bits(got, h.day_order_stats(days, series=series, p=p)), series
            assert {int(v) for v in got[:, 0].ravel()} == {365, 366}
            assert same_bits(ctx.get_dayquant(3, 4, series=series, p=p), got[3:7])
            pooled = ctx.get_dayquant(0, ny, series=series, p=p, pooled=True)
            assert pooled.shape == (1, 7, n)
            assert same_bits(pooled, h.day_order_stats(days, series=series, p=p, pooled=True)), series
            assert same_bits(pooled[0, 0], got[:, 0].sum(axis=0)) and (pooled[0, 0] == nd).all()
            part = ctx.get_dayquant(3, 4, series=series, p=p, pooled=True)
            assert same_bits(part, h.day_order_stats(days[3:7], series=series, p=p, pooled=True)), series
            assert not same_bits(part, pooled)
        for span in ((0, 13), (12, 1), (-1, 2), (5, 0), (11, 2)):
            for pool in (False, True):
                with pytest.raises(ValueError, match="H9G_EINVAL"):
                    ctx.get_dayquant(*span, series="q", p=p, pooled=pool)
        want_py, want_pool = ctx.get_dayquant(0, ny, series="q", p=p), ctx.get_dayquant(0, ny, series="q", p=p,
                                                                                        pooled=True)
    inp12 = dict(inp, nyears=ny, forcing=np.ascontiguousarray(inp["forcing"][:, :nd]))
    out = h.run_cell_order(dayquant=dict(series="q", p=p), **inp12)
    assert out["rc"] == 0 and "days" not in out and same_bits(out["dayquant"], want_py)
    out = h.run_cell_order(dayquant=dict(series="q", p=p, pooled=True), **inp12)
    assert out["rc"] == 0 and same_bits(out["dayquant"], want_pool)


# ---- 4. STOP and mask conventions ------------------------------------------------------
def test_stop_and_masked_cell_rows():
    meta, inp = stop_mask_inputs()
    _, rec = golden_records("stop_ns24")
    s = meta["stop"]
    out = h.run(stop_on_error=False, days=True, dayquant=dict(series="theta1", p=QP), **inp)
    assert out["rc"] == s["code"]
    q = out["dayquant"][0]
    assert same_bits(q, h.day_order_stats([out["days"][0, :365]], series="theta1", p=QP)[0])
    assert same_bits(q, order_stats_loop([rec[0, :365]], series="theta1", p=QP)[0])
    c = s["cell"]
    assert q[0, c] == s["day"] and 0 < s["day"] < 365            # the days before the STOP count
    assert np.isfinite(q[:, c]).all()
    assert q[0, 2] == 0 and np.isnan(q[1:, 2]).all()             # the masked cell: no day at all
    rest = [k for k in range(meta["ncell"]) if k not in (c, 2)]
    assert (q[0, rest] == 365).all() and np.isfinite(q[:, rest]).all()


# ---- 5. off means off --------------------------------------------------------------------
def test_a_call_changes_nothing_else():
    meta, inp, _ = load_golden("c1_2yr_leap")
    with h.Context(meta["ncell"], inp["zi"], nisurf=inp["nisurf"]) as ctx:
        ctx.set_params(inp["params"])
        ctx.init_state()
        ctx.set_evap(True)
        ctx.set_monthly(True)
        ctx.set_days(True)
        ctx.push_forcing(0, inp["forcing"][:, :365])
        ctx.run_year(0, inp["year0"])
        ctx.sync()

        def everything():
            ls = ctx.launch_stats()
            return (ctx.get_annual(), ctx.get_state(), ctx.get_days(), ctx.get_monthly(),
                    {k: (v["launches"], v["cell_years"], v["ms"]) for k, v in ls.items()}, ctx.kernel_name(),
                    ctx.total_kernel_ms())

        before = everything()
        a = ctx.get_dayquant(series="q", p=QP)
        b = ctx.get_dayquant(series="zwt", p=(0.5,), pooled=True)
        after = everything()
        assert a.shape[1] == NROWS and b.shape[1] == 3 and not same_bits(a[0, 1], b[0, 1])   # (the calls did run)
        for x, y in zip(before[:4], after[:4]):
            assert same_bits(x, y)
        assert before[4] == after[4] and sum(v[0] for v in after[4].values()) == 1    # one year launch, still
        assert before[5:] == after[5:]
        # ... and the next year runs as if no quantiles had been taken
        ctx.push_forcing(1, inp["forcing"][:, 365:])
        ctx.run_year(1, inp["year0"] + 1)
        ctx.sync()
        ann, state, days = ctx.get_annual(), ctx.get_state(), ctx.get_days()
    ref = h.run(days=True, monthly=True, **inp)
    assert same_bits(ann, ref["annual"][1]) and same_bits(state, ref["state"]) and same_bits(days, ref["days"][1])


# ---- 6. the Fortran host --------------------------------------------------------------------
def _read_qxy(path, n):
    from scipy.io import netcdf_file
    with netcdf_file(path, "r", mmap=False) as nc:
        nq = nc.dimensions["quantile"]
        rows = [np.array(nc.variables["count"][:], np.float64).reshape(-1)[:n]]
        lower = np.array(nc.variables["lower"][:], np.float64).reshape(nq, -1)[:, :n]
        upper = np.array(nc.variables["upper"][:], np.float64).reshape(nq, -1)[:, :n]
        for i in range(nq):
            rows += [lower[i], upper[i]]
        value = np.array(nc.variables["value"][:], np.float64).reshape(nq, -1)[:, :n]
        return (np.stack(rows), value, np.array(nc.variables["p"][:], np.float64), nc.series.decode(),
                int(nc.year_first), int(nc.year_last))


def test_fortran_host_writes_qxy(tmp_path):
    from tests.test_fortran_host import _build
    exe = _build()
    meta, inp, exp = load_golden("c1_10x10")
    n = meta["ncell"]
    p = (0.05, 0.5, 0.95, 0.2)
    for cell_order in (False, True):
        work = tmp_path / f"co{int(cell_order)}"
        work.mkdir()
        case = work / "case"
        refcase.write_case(case, zi=inp["zi"], params=inp["params"], forcing=inp["forcing"], nisurf=inp["nisurf"],
                           year0=inp["year0"], nyears=inp["nyears"], grow_on=inp["grow_on"], state0=None,
                           cell_order=cell_order)
        nml = work / "h9gpu.nml"
        nml.write_text(f"&h9gpu\n input_mode='case', case_dir='{case}', out_dir='{work}', dayquant=1,\n"
                       f" quant_series=4, quant_p(1)=0.05, quant_p(2)=0.5, quant_p(3)=0.95, quant_p(5)=0.2,"
                       f" quant_pool={int(cell_order)}\n/\n")
        r = subprocess.run([str(exe), str(work / "no_driver.txt"), str(nml)], capture_output=True, text=True,
                           timeout=600)
        assert "completed successfully" in r.stdout, r.stdout + r.stderr
        y0, ny = inp["year0"], meta["nyears"]
        if cell_order:
            out = h.run_cell_order(days=True, **inp)
            assert out["rc"] == 0
            years = [out["days"][y, :h.days_in_year(y0 + y)] for y in range(ny)]
            want = h.day_order_stats(years, series="zwt", p=p, pooled=True)[0]
            got, value, pp, name, first, last = _read_qxy(work / f"qxy{y0}_{y0 + ny - 1}.nc", n)
            assert same_bits(got, want) and same_bits(value, h.day_quantiles(want, p))
            assert same_bits(pp, np.array(p)) and name == "zwt" and (first, last) == (y0, y0 + ny - 1)
            assert not (work / f"qxy{y0}.nc").exists()
        else:
            out = h.run(days=True, **inp)
            for y in range(ny):
                jy = y0 + y
                want = h.day_order_stats([out["days"][y, :h.days_in_year(jy)]], series="zwt", p=p)[0]
                assert not (work / f"dxy{jy}.nc").exists()        # days = 1 was not set
                got, value, pp, name, first, last = _read_qxy(work / f"qxy{jy}.nc", n)
                assert same_bits(got, want) and same_bits(value, h.day_quantiles(want, p)), jy
                assert name == "zwt" and (first, last) == (jy, jy)
    # pooled quantiles need the ordered mode (case.nml's cell_order governs a case)
    work = tmp_path / "co0"
    case, nml = work / "case", work / "h9gpu.nml"
    nml.write_text(f"&h9gpu\n input_mode='case', case_dir='{case}', out_dir='{work}', dayquant=1, quant_pool=1,"
                   f" cell_order=0\n/\n")
    r = subprocess.run([str(exe), str(work / "no_driver.txt"), str(nml)], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "quant_pool = 1 needs cell_order = 1" in r.stdout + r.stderr
