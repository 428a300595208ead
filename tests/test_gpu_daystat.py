"""Day statistics on the GPU: h9g_daystat_kernel gives, for hand-made records
and for the records of both run modes, the rows of the table of include/h9g.h
as the plain loop (daystat_helpers.day_stats_loop) and hybrid9_amd.day_stats
give them, bit for bit, however the year is cut into slices; and calling it
changes nothing else.  Every comparison is conftest.same_bits: no tolerance.
Runs on an MI355X only."""
import subprocess

import numpy as np
import pytest

import hybrid9_amd as h
from oracle import refcase
from tests.conftest import load_golden, same_bits
from tests.daily_helpers import stop_mask_inputs
from tests.daystat_helpers import (HAND_THR, NS, WS, check_handmade, day_stats_loop, golden_records, handmade,
                                   random_records, thresholds_of)

pytestmark = pytest.mark.gpu

_cache = {}


def _once(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


NSEGS = (0, 1, 3, *WS)


# ---- 1. the kernel on hand-made records ------------------------------------------
def test_selftest_handmade_records():
    rec = handmade()
    want = _once("hand", lambda: day_stats_loop(rec, **HAND_THR))
    check_handmade(want)
    for nseg in NSEGS:
        got = h.daystat_selftest(rec, nseg=nseg, **HAND_THR)
        assert same_bits(got, want), f"nseg {nseg}: " \
            f"{[h.DAYSTAT_FIELDS[i] for i in range(NS) if not same_bits(got[i], want[i])]}"
    for nseg in (2, 5, 7, 9, 15, 16):             # every kernel built, with empty trailing slices too
        assert same_bits(h.daystat_selftest(rec, nseg=nseg, **HAND_THR), want), nseg
    for nt in (1, 6, 7, 13):                      # fewer days than slices, and than a 7-day window
        w = day_stats_loop(rec[:nt], **HAND_THR)
        for nseg in (0, 1, 16):
            assert same_bits(h.daystat_selftest(rec[:nt], nseg=nseg, **HAND_THR), w), (nt, nseg)
    with pytest.raises(ValueError):
        h.daystat_selftest(rec, nseg=17, **HAND_THR)


@pytest.mark.parametrize("nt", [365, 366])
def test_selftest_random_cells_and_tail_workgroups(nt):
    """200 cells with NaN tails of random length; n = 1, 63, 64, 65, 200: a lone
    lane, a workgroup one lane short, full, one lane into the next, several."""
    rec = random_records(200, nt, nt)
    want = _once(("rand", nt), lambda: day_stats_loop(rec, **HAND_THR))
    assert (want[0] == 0).any() and (want[0] == nt).any() and ((want[0] > 0) & (want[0] < nt)).any()
    for n in (1, 63, 64, 65, 200):
        sub = np.ascontiguousarray(rec[:, :, :n])
        for nseg in NSEGS:
            got = h.daystat_selftest(sub, nseg=nseg, **HAND_THR)
            assert same_bits(got, want[:, :n]), f"n {n}, nseg {nseg}: " \
                f"{[h.DAYSTAT_FIELDS[i] for i in range(NS) if not same_bits(got[i], want[i, :n])]}"


# ---- 2. isolated mode ------------------------------------------------------------------
def test_isolated_years_match_records_and_oracle():
    meta, inp, _ = load_golden("c1_2yr_leap")
    _, rec = golden_records("c1_2yr_leap")
    thr = thresholds_of("c1_2yr_leap", rec)
    with h.Context(meta["ncell"], inp["zi"], nisurf=inp["nisurf"]) as ctx:
        ctx.set_params(inp["params"])
        ctx.init_state()
        ctx.set_evap(True)
        ctx.set_days(True)
        with pytest.raises(h.H9GError, match="nothing recorded"):
            ctx.get_daystats(**thr)
        d0 = 0
        for y in range(2):
            nt = h.days_in_year(inp["year0"] + y)
            ctx.push_forcing(y, inp["forcing"][:, d0:d0 + nt])
            ctx.run_year(y, inp["year0"] + y)
            ctx.sync()
            d0 += nt
            got = ctx.get_daystats(**thr)
            assert got.shape == (1, NS, meta["ncell"]) and got.dtype == np.float64
            days = ctx.get_days()
            assert days.shape[0] == nt
            assert same_bits(got[0], h.day_stats(days, **thr))
            assert same_bits(got[0], day_stats_loop(rec[y, :nt], **thr))
            assert (got[0, 0] == nt).all()
            for span in ((0, 2), (1, 1), (-1, 1), (0, 0)):
                with pytest.raises(ValueError, match="H9G_EINVAL"):
                    ctx.get_daystats(*span, **thr)
            assert ctx.last_daystat_ms() > 0
    out = h.run(daystats=thr, **inp)
    assert "days" not in out and out["daystats"].shape == (2, NS, meta["ncell"])
    for y in range(2):
        assert same_bits(out["daystats"][y], day_stats_loop(rec[y, :h.days_in_year(inp["year0"] + y)], **thr))


# ---- 3. ordered mode -------------------------------------------------------------------
def test_ordered_span_in_one_call():
    meta, inp, _ = load_golden("co_c1_30yr")
    ny = 12
    nd = sum(h.days_in_year(y) for y in range(1901, 1901 + ny))
    n, L = meta["ncell"], meta["L"]
    assert inp["year0"] == 1901 and n == 100
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
        # thresholds from the records themselves, as the host tests take them
        thr = thresholds_of("co_c1_30yr", np.stack([np.pad(d, ((0, 366 - d.shape[0]), (0, 0), (0, 0)),
                                                           constant_values=np.nan) for d in days]))
        got = ctx.get_daystats(0, ny, **thr)
        assert got.shape == (ny, NS, n)
        for k in range(ny):
            assert same_bits(got[k], h.day_stats(days[k], **thr)), f"year {1901 + k}"
        assert {int(v) for v in got[:, 0].ravel()} == {365, 366}
        assert same_bits(ctx.get_daystats(3, 4, **thr), got[3:7])
        assert same_bits(ctx.get_daystats(11, 1, **thr), got[11:])
        for span in ((0, 13), (12, 1), (-1, 2), (5, 0), (11, 2)):
            with pytest.raises(ValueError, match="H9G_EINVAL"):
                ctx.get_daystats(*span, **thr)
        # the counts are not trivial on these years
        for r in (4, 10, 13, 16):
            mid = (got[:, r] > 0) & (got[:, r] < got[:, 0])
            print(f"co_c1_30yr 1901-{1900 + ny}: {h.DAYSTAT_FIELDS[r]} strictly between 0 and ndays in "
                  f"{int(mid.sum())} of {mid.size} cell-years")
            assert mid.any()
    inp12 = dict(inp, nyears=ny, forcing=np.ascontiguousarray(inp["forcing"][:, :nd]))
    out = h.run_cell_order(daystats=thr, **inp12)
    assert out["rc"] == 0 and "days" not in out and same_bits(out["daystats"], got)


# ---- 4. STOP and mask conventions ------------------------------------------------------
def test_stop_and_masked_cell_rows():
    meta, inp = stop_mask_inputs()
    _, rec = golden_records("stop_ns24")
    thr = thresholds_of("stop_ns24", rec)
    s = meta["stop"]
    out = h.run(stop_on_error=False, days=True, daystats=thr, **inp)
    assert out["rc"] == s["code"]
    st = out["daystats"][0]
    assert same_bits(st, h.day_stats(out["days"][0, :365], **thr))
    assert same_bits(st, day_stats_loop(rec[0, :365], **thr))
    c = s["cell"]
    assert st[0, c] == s["day"] and 0 < s["day"] < 365          # the days before the STOP count
    assert np.isfinite(st[:, c]).all() == (s["day"] >= 7)       # (a 7-day window needs seven of them)
    assert st[0, 2] == 0                                         # the masked cell: no day at all
    assert np.isnan(st[[1, 3, 5, 6, 8, 9, 12, 14], 2]).all() and (st[[2, 7, 15], 2] == -1).all()
    assert (st[[4, 10, 11, 13, 16], 2] == 0).all()
    rest = [k for k in range(meta["ncell"]) if k not in (c, 2)]
    assert (st[0, rest] == 365).all() and np.isfinite(st[:, rest]).all()


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
        a = ctx.get_daystats(**HAND_THR)
        b = ctx.get_daystats(q_thr=0.5)
        after = everything()
        assert not same_bits(a, b)                # (other thresholds, other counts: the call did run)
        for x, y in zip(before[:4], after[:4]):
            assert same_bits(x, y)
        assert before[4] == after[4] and sum(v[0] for v in after[4].values()) == 1    # one year launch, still
        assert before[5:] == after[5:]
        # ... and the next year runs as if no statistics had been taken
        ctx.push_forcing(1, inp["forcing"][:, 365:])
        ctx.run_year(1, inp["year0"] + 1)
        ctx.sync()
        ann, state, days = ctx.get_annual(), ctx.get_state(), ctx.get_days()
    ref = h.run(days=True, monthly=True, **inp)
    assert same_bits(ann, ref["annual"][1]) and same_bits(state, ref["state"]) and same_bits(days, ref["days"][1])


# ---- 6. the Fortran host --------------------------------------------------------------------
def test_fortran_host_writes_sxy(tmp_path):
    from scipy.io import netcdf_file
    from tests.test_fortran_host import _build
    exe = _build()
    meta, inp, exp = load_golden("c1_10x10")
    n = meta["ncell"]
    case = tmp_path / "case"
    refcase.write_case(case, zi=inp["zi"], params=inp["params"], forcing=inp["forcing"], nisurf=inp["nisurf"],
                       year0=inp["year0"], nyears=inp["nyears"], grow_on=inp["grow_on"], state0=None, cell_order=False)
    thr = dict(q_thr=0.5, theta_thr=0.25, zwt_thr=2000.0, lai_thr=1.25)
    nml = tmp_path / "h9gpu.nml"
    nml.write_text(f"&h9gpu\n input_mode='case', case_dir='{case}', out_dir='{tmp_path}', daystats=1,\n"
                   f" q_thr={thr['q_thr']}, theta_thr={thr['theta_thr']}, zwt_thr={thr['zwt_thr']},"
                   f" lai_thr={thr['lai_thr']}\n/\n")
    r = subprocess.run([str(exe), str(tmp_path / "no_driver.txt"), str(nml)], capture_output=True, text=True,
                       timeout=600)
    assert "completed successfully" in r.stdout, r.stdout + r.stderr
    out = h.run(days=True, **inp)
    for y in range(meta["nyears"]):
        jy = inp["year0"] + y
        want = h.day_stats(out["days"][y, :h.days_in_year(jy)], **thr)
        assert not (tmp_path / f"dxy{jy}.nc").exists()            # days = 1 was not set
        with netcdf_file(tmp_path / f"sxy{jy}.nc", "r", mmap=False) as nc:
            for i, k in enumerate(h.DAYSTAT_FIELDS):
                assert same_bits(np.array(nc.variables[k][:], np.float64).reshape(-1)[:n], want[i]), (jy, k)
            assert int(nc.year) == jy and np.float32(nc.theta_thr) == np.float32(thr["theta_thr"])
