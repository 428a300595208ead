"""Day records on the GPU: the day year kernels (every kind the dispatch can
choose) store the host build's records bit for bit, in both run modes, and
leave annual means, month-end snapshots, state and STOP records exactly as an
ET run without day recording leaves them.  Every comparison is
conftest.same_bits: no tolerance.  Runs on an MI355X only."""
import subprocess

import numpy as np
import pytest

import hybrid9_amd as h
from hybrid9_amd import synth
from oracle import port, refcase
from tests.conftest import load_golden, same_bits
from tests.daily_helpers import stop_mask_inputs
from tests.days_helpers import ND, cell_order_days, check_ties, host_days, port_days
from tests.monthly_helpers import l10_inputs

pytestmark = pytest.mark.gpu

_cache = {}


def _once(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _same_errors(a, b):
    return all(same_bits(a[k], b[k]) for k in ("code", "day", "substep", "value"))


# ---- 1. the contract of h9g_set_days / h9g_get_days -------------------------
def test_days_contract():
    meta, inp, _ = load_golden("c1_2yr_leap")
    with h.Context(meta["ncell"], inp["zi"], nisurf=inp["nisurf"]) as ctx:
        lb, hd = ctx._lib, ctx._h
        with pytest.raises(h.H9GError, match="nothing recorded"):
            ctx.get_days()
        assert lb.h9g_set_days(hd, 1) == -4            # H9G_ESTATE: needs ET recording
        with pytest.raises(h.H9GError, match="set_evap"):
            ctx.set_days(True)
        ctx.set_evap(True)
        assert "_et_kernel" in ctx.kernel_name()
        ctx.set_days(True)
        assert "_day_kernel" in ctx.kernel_name() and "_et_kernel" not in ctx.kernel_name()
        assert lb.h9g_set_evap(hd, 0) == -4            # ... and ET stays on while days are recorded
        with pytest.raises(h.H9GError, match="nothing recorded"):
            ctx.get_days()
        ctx.set_days(False)
        assert "_et_kernel" in ctx.kernel_name()
        ctx.set_params(inp["params"])
        ctx.init_state()
        ctx.push_forcing(0, inp["forcing"][:, :365])
        ctx.run_year(0, 1903)
        ctx.sync()
        with pytest.raises(h.H9GError, match="nothing recorded"):
            ctx.get_days()
        ctx.set_days(True)
        ctx.push_forcing(1, inp["forcing"][:, 365:])
        ctx.run_year(1, 1904)
        ctx.sync()
        assert ctx.get_days(0).shape == (366, ND, meta["ncell"])
        for k in (-1, 1):
            with pytest.raises(h.H9GError, match="failed with -1"):
                ctx.get_days(k)
        with pytest.raises(h.H9GError, match="H9G_ESTATE"):     # spin-up records nothing
            ctx.spinup([1], 1904, max_cycles=1)
        ctx.set_days(False)
        ctx.set_evap(False)


# ---- 2. c1_2yr_leap on the L = 8 kinds ---------------------------------------
@pytest.mark.parametrize("kernel", ["pair", "pair11", "pair1"])
def test_leap_years_match_host_and_trace(kernel, monkeypatch):
    meta, inp, exp = load_golden("c1_2yr_leap")
    host = _once("leap_host", lambda: host_days(**inp))
    rec, _ = _once("leap_trace", lambda: port_days(**inp))
    monkeypatch.setenv("H9G_KERNEL", kernel)
    off = h.run(evap=True, **inp)
    on = h.run(days=True, **inp)
    both = h.run(days=True, monthly=True, **inp)
    o = [k for k in range(12 + meta["L"]) if k != 3]
    for r in (on, both):
        assert r["rc"] == off["rc"] == 0
        assert same_bits(r["annual"], off["annual"]) and same_bits(r["annual"][:, o], exp["annual"][:, o])
        assert same_bits(r["state"], off["state"]) and same_bits(r["state"], exp["state"])
        assert _same_errors(r["errors"], off["errors"])
        assert same_bits(r["days"], host["days"]) and same_bits(r["days"], rec)
    assert same_bits(both["monthly"], host["monthly"])
    assert check_ties(on["days"], on["annual"], None, inp["year0"], inp["nisurf"]) == 2 * meta["ncell"]
    assert check_ties(both["days"], both["annual"], both["monthly"], inp["year0"], inp["nisurf"]) == 2 * meta["ncell"]


# ---- 3. L = 10, NS = 24 on solo, pair2 and both halves of mixed ---------------
@pytest.mark.parametrize("kernel", ["solo", "pair2", "mixed"])
def test_l10_kinds_match_host(kernel, monkeypatch):
    inp = l10_inputs(30)
    host = _once("l10_host", lambda: host_days(**inp))
    assert host["rc"] == 0
    monkeypatch.setenv("H9G_KERNEL", kernel)
    monkeypatch.setenv("H9G_SPLIT", "17")           # mixed: cells [0, 17) solo, [17, 30) pair
    off = h.run(evap=True, **inp)
    on = h.run(days=True, **inp)
    assert on["rc"] == off["rc"] == 0
    assert same_bits(on["annual"], off["annual"]) and same_bits(on["annual"], host["annual"])
    assert same_bits(on["state"], off["state"]) and same_bits(on["state"], host["state"])
    assert same_bits(on["days"], host["days"])
    assert check_ties(on["days"], on["annual"], None, inp["year0"], inp["nisurf"]) == 30


# ---- 4. ragged, several workgroups: sort, slot-ordered I/O, un-permute --------
LISTS = ((3, 1), (0, 3), (120, 5))         # tests/test_gpu_monthly.py


def _strided():
    gid = synth.land_cells()[::331][:200]
    lat = synth.cell_lat(gid, synth.NX05, synth.NY05)
    inp = dict(zi=synth.ZI_L8, params=synth.make_params(gid, 8),
               forcing=synth.make_forcing(gid, lat, synth.year_day0(1901), 365 + 365), nisurf=48, year0=1901,
               nyears=2, grow_on=1)
    return inp, host_days(**inp)


def _sub(inp, lo, n):
    return dict(inp, params={k: v[lo:lo + n] for k, v in inp["params"].items()},
                forcing=np.ascontiguousarray(inp["forcing"][:, :, lo:lo + n]))


def test_strided_cells_on_pair_match_host(monkeypatch):
    inp, host = _once("strided", _strided)
    assert host["rc"] == 0
    monkeypatch.setenv("H9G_KERNEL", "pair")
    on = h.run(days=True, monthly=True, **inp)
    assert on["rc"] == 0
    assert same_bits(on["annual"], host["annual"]) and same_bits(on["state"], host["state"])
    assert same_bits(on["monthly"], host["monthly"])
    assert same_bits(on["days"], host["days"])
    assert check_ties(on["days"], on["annual"], on["monthly"], 1901, 48) == 400


@pytest.mark.parametrize("lo,n", LISTS)
def test_strided_lists_on_pair1_match_host(lo, n, monkeypatch):
    inp, host = _once("strided", _strided)
    monkeypatch.setenv("H9G_KERNEL", "pair1")
    on = h.run(days=True, **_sub(inp, lo, n))
    assert on["rc"] == 0
    assert same_bits(on["annual"], host["annual"][:, :, lo:lo + n])
    assert same_bits(on["days"], host["days"][:, :, :, lo:lo + n])


# ---- 5. STOP and mask conventions -----------------------------------------------
@pytest.mark.parametrize("kernel", ["pair", "solo"])
def test_stop_and_masked_cell(kernel, monkeypatch):
    meta, inp = stop_mask_inputs()
    s = meta["stop"]
    host = _once("stop_host", lambda: host_days(**inp))
    monkeypatch.setenv("H9G_KERNEL", kernel)
    off = h.run(stop_on_error=False, evap=True, **inp)
    on = h.run(stop_on_error=False, days=True, **inp)
    assert on["rc"] == off["rc"] == s["code"]
    assert same_bits(on["annual"], off["annual"]) and same_bits(on["state"], off["state"])
    assert _same_errors(on["errors"], off["errors"])
    c, d = s["cell"], on["days"]
    ys, e = int(host["err"][c, 1]), int(host["err"][c, 2])
    assert np.isfinite(d[:ys, :365, :, c]).all() and np.isfinite(d[ys, :e, :, c]).all()
    assert np.isnan(d[ys, e:, :, c]).all() and np.isnan(d[ys + 1:, :, :, c]).all()
    assert np.isnan(d[..., 2]).all()
    assert same_bits(d, host["days"])
    assert check_ties(d, on["annual"], None, inp["year0"], inp["nisurf"]) > 0


# ---- 6. the tie to the focus line ------------------------------------------------
def test_days_tie_to_the_daily_line(monkeypatch):
    """Rows 3 and 6 of the day records are columns theta(1) and LAI of
    h9g_get_daily (HYBRID9.f90:226-227, HYDROLOGY.f90:1233), bit for bit."""
    meta, inp, exp = load_golden("c1_2yr_leap")
    sel = [0, 3, 7, 11, 16]
    on = h.run(days=True, daily_cells=sel, **inp)
    assert on["rc"] == 0
    d0 = 0
    for y in range(inp["nyears"]):
        nt = h.days_in_year(inp["year0"] + y)
        line = on["daily"][d0:d0 + nt]
        assert same_bits(on["days"][y, :nt, 3][:, sel], line[:, 2])
        assert same_bits(on["days"][y, :nt, 6][:, sel], line[:, 7])
        d0 += nt


# ---- 7. the reference's order, small ---------------------------------------------
def _co16():
    meta, inp, _ = load_golden("co_c1_30yr")
    nd = sum(h.days_in_year(y) for y in range(1901, 1921))
    return dict(inp, nyears=20, params={k: v[:16] for k, v in inp["params"].items()},
                forcing=np.ascontiguousarray(inp["forcing"][:, :nd, :16]))


def test_cell_order_small_matches_trace():
    """16 cells as their own chain over 1901-1920: the second decade re-runs
    cells, some for one year only (an early merge); both APIs give the records
    the oracle's traced cell-order loop gives, with monthly recording or a daily
    selection beside them."""
    inp = _co16()
    kw = {k: v for k, v in inp.items() if k != "state0"}
    ref = port.run_cell_order(**kw)
    rec, st, ann = cell_order_days(**kw)
    assert ref["rc"] == 0 and same_bits(ann, ref["annual"])
    # the combinations ride along: monthly recording in the pipelined call
    # (the decades stay overlapped), a daily selection in the per-decade one
    sel = [1, 6, 15]
    a = h.run_cell_order(pipelined=True, days=True, monthly=True, **inp)
    b = h.run_cell_order(pipelined=False, days=True, daily_cells=sel, **inp)
    L = inp["params"]["theta_s"].shape[1]
    o = [k for k in range(12 + L) if k != 3]
    for r in (a, b):
        assert r["rc"] == 0
        assert same_bits(r["annual"][:, o], ref["annual"][:, o])
        assert same_bits(r["state"], refcase.pack_state(ref["state"], L))
    assert same_bits(a["days"], b["days"])
    assert same_bits(a["days"], rec)
    assert check_ties(a["days"], a["annual"], a["monthly"], 1901, inp["nisurf"]) == 20 * 16
    d0 = 0
    for y in range(20):                      # rows 3 and 6 against the daily line, as in isolated mode
        nt = h.days_in_year(1901 + y)
        assert same_bits(b["days"][y, :nt, 3][:, sel], b["daily"][d0:d0 + nt, 2])
        assert same_bits(b["days"][y, :nt, 6][:, sel], b["daily"][d0:d0 + nt, 7])
        d0 += nt
    w = b["work"][1]                         # decade 2 of the per-decade run (h9g_decade_stats)
    print(f"co16: decade 2 re-ran {w['rerun_cells']} cells, {w['rerun_cell_years']} cell-years; passes {b['passes']}")
    assert w["rerun_cells"] > 0 and w["rerun_cell_years"] < 10 * w["rerun_cells"]


# ---- 8. the reference's order, re-runs riding ---------------------------------------
def test_cell_order_band_riding():
    meta, inp, exp = load_golden("co_c2_band")
    nd = sum(h.days_in_year(y) for y in range(1901, 1921))
    inp = dict(inp, nyears=20, forcing=np.ascontiguousarray(inp["forcing"][:, :nd]))
    a = h.run_cell_order(pipelined=True, days=True, **inp)
    b = h.run_cell_order(pipelined=False, days=True, **inp)
    L = inp["params"]["theta_s"].shape[1]
    o = [k for k in range(12 + L) if k != 3]
    for r in (a, b):
        assert r["rc"] == 0
        assert same_bits(r["annual"][:, o], exp["annual"][:20][:, o])
    assert same_bits(a["annual"], b["annual"]) and same_bits(a["state"], b["state"])
    assert same_bits(a["days"], b["days"])
    check_ties(a["days"], a["annual"], None, 1901, inp["nisurf"])
    print(f"co_c2_band 1901-1920: overlap {a['overlap']}")
    assert a["overlap"]["rerun_years_riding"] > 0


# ---- 9. a STOP inside the reference's order ---------------------------------------
def test_cell_order_stop():
    meta, inp, _ = load_golden("co_stop")
    off = h.run_cell_order(pipelined=False, evap=True, **inp)
    on = h.run_cell_order(pipelined=False, days=True, **inp)
    s = meta["stop"]
    assert on["rc"] == off["rc"] == s["code"]
    assert on["err"] == off["err"] and _same_errors(on["errors"], off["errors"])
    assert same_bits(on["annual"], off["annual"]) and same_bits(on["state"], off["state"])
    check_ties(on["days"], on["annual"], None, inp["year0"], inp["nisurf"])
    c, d = s["cell"], on["days"]
    ys, e = on["err"]["year"] - inp["year0"], on["err"]["day"]
    assert on["err"]["cell"] == c
    assert np.isnan(d[ys, e:, :, c]).all() and np.isnan(d[ys + 1:, :, :, c]).all()
    assert np.isfinite(d[ys, :e, :, c]).all() and np.isfinite(d[:ys, :365, :, c]).all()


# ---- 10. one context, several calls: the recording buffers' lifetime ---------------
def test_recordings_across_calls_on_one_context():
    """A context that is reused -- an ordered call with months, a longer one
    with day records switched on beside them (the retained buffers of both
    regrow; the day records' decade buffers come after the ordered mode's own),
    then months off and a single year -- gives after every call the months and
    day records a fresh context gives for the same years from the same start,
    bit for bit, and refuses the year one past the last."""
    meta, inp, _ = load_golden("co_c1_30yr")
    n, L = 8, inp["params"]["theta_s"].shape[1]
    assert inp.get("state0") is None
    params = {k: v[:n] for k, v in inp["params"].items()}
    d0 = np.concatenate([[0], np.cumsum([h.days_in_year(y) for y in range(1901, 1907)])])

    def context(state, monthly, days):
        ctx = h.Context(n, inp["zi"], nlayers=L, nisurf=inp["nisurf"], grow_on=inp.get("grow_on", True), nslots=3)
        ctx.set_params(params)
        ctx.set_evap(True)
        ctx.set_monthly(monthly)
        ctx.set_days(days)
        ctx.init_state() if state is None else ctx.set_state(state)
        return ctx

    def run(ctx, years, ordered, monthly, days):
        """Runs the years; the recorded (months, day records) of each."""
        for k, y in enumerate(years):
            ctx.push_forcing(k, inp["forcing"][:, d0[y - 1901]:d0[y - 1900], :n])
        if ordered:
            ctx.run_ordered(list(range(len(years))), years[0])
        else:
            ctx.run_year(0, years[0])
            ctx.sync()
        for get, on in ((ctx.get_monthly, monthly), (ctx.get_days, days)):
            if on:
                with pytest.raises(h.H9GError, match="failed with -1"):     # H9G_EINVAL
                    get(len(years))
        return ([ctx.get_monthly(k) for k in range(len(years))] if monthly else [],
                [ctx.get_days(k) for k in range(len(years))] if days else [])

    steps = (((1901, 1902), True, True, False),               # years, ordered, monthly, days
             ((1903, 1904, 1905), True, True, True),
             ((1906,), False, False, True))
    with context(None, True, False) as reused:
        for years, ordered, monthly, days in steps:
            start = reused.get_state()
            assert not reused.get_errors()["code"].any()       # (a fresh context's STOP records: none)
            reused.set_monthly(monthly)
            reused.set_days(days)
            got = run(reused, years, ordered, monthly, days)
            with context(start, monthly, days) as fresh:
                want = run(fresh, years, ordered, monthly, days)
                assert same_bits(reused.get_state(), fresh.get_state())
            for g, w in zip(got, want):
                assert len(g) == len(w) == (len(years) if len(w) else 0)
                assert all(a.shape == b.shape and same_bits(a, b) for a, b in zip(g, w))
            assert [d.shape[0] for d in got[1]] == [h.days_in_year(y) for y in years if days]
        with pytest.raises(h.H9GError, match="nothing recorded"):
            reused.get_monthly()
        assert reused.get_days(0).shape == (365, ND, n)


# ---- 11. the Fortran host ----------------------------------------------------------
def test_fortran_host_writes_dxy(tmp_path):
    from tests.test_fortran_host import _build
    exe = _build()
    meta, inp, exp = load_golden("c1_10x10")
    n, L = meta["ncell"], meta["L"]
    case = tmp_path / "case"
    refcase.write_case(case, zi=inp["zi"], params=inp["params"], forcing=inp["forcing"], nisurf=inp["nisurf"],
                       year0=inp["year0"], nyears=inp["nyears"], grow_on=inp["grow_on"], state0=None, cell_order=False)
    nml = tmp_path / "h9gpu.nml"
    nml.write_text(f"&h9gpu\n input_mode='case', case_dir='{case}', out_dir='{tmp_path}', days=1\n/\n")
    r = subprocess.run([str(exe), str(tmp_path / "no_driver.txt"), str(nml)], capture_output=True, text=True,
                       timeout=600)
    assert "completed successfully" in r.stdout, r.stdout + r.stderr
    out = h.run(days=True, **inp)
    ann = np.fromfile(tmp_path / "annual.f32", np.float32).reshape(meta["nyears"], 12 + L, n)
    assert same_bits(ann, out["annual"])
    zi = np.asarray(inp["zi"], np.float32)
    zc = (zi[1:L + 1] - (zi[1:L + 1] - zi[:L]) / np.float32(2.0)).astype(np.float32)
    for y in range(meta["nyears"]):
        jy = inp["year0"] + y
        mine = tmp_path / f"py_dxy{jy}.nc"
        h.write_dxy_nc(mine, out["days"][y, :h.days_in_year(jy)], np.arange(n), zc, jy, nx=n, ny=1)
        assert (tmp_path / f"dxy{jy}.nc").read_bytes() == mine.read_bytes()
