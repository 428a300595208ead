"""Monthly output on the GPU: the monthly year kernels (every kind the
dispatch can choose) store the host build's month-end snapshots bit for bit,
in both run modes, and leave annual means, state and STOP records exactly as
a run with recording off leaves them.  Every comparison is
conftest.same_bits: no tolerance.  Runs on an MI355X only."""
import subprocess

import numpy as np
import pytest

import hybrid9_amd as h
from hybrid9_amd import synth
from oracle import port, refcase
from tests.conftest import load_golden, same_bits
from tests.daily_helpers import stop_mask_inputs
from tests.monthly_helpers import (NM, cell_order_snapshots, check_year_end, host_monthly, l10_inputs, port_snapshots,
                                   trace_rows)

pytestmark = pytest.mark.gpu

_cache = {}


def _once(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _same_errors(a, b):
    return all(same_bits(a[k], b[k]) for k in ("code", "day", "substep", "value"))


def test_nothing_recorded_is_estate():
    """h9g_get_monthly's contract is h9g_get_daily's: H9G_ESTATE before any
    recording run (also with recording switched on, and after a run with it
    off), H9G_EINVAL for a bad k."""
    meta, inp, _ = load_golden("c1_2yr_leap")
    with h.Context(meta["ncell"], inp["zi"], nisurf=inp["nisurf"]) as ctx:
        with pytest.raises(h.H9GError, match="nothing recorded"):
            ctx.get_monthly()
        ctx.set_monthly(True)
        with pytest.raises(h.H9GError, match="nothing recorded"):
            ctx.get_monthly()
        ctx.set_monthly(False)
        ctx.set_params(inp["params"])
        ctx.init_state()
        ctx.push_forcing(0, inp["forcing"][:, :365])
        ctx.run_year(0, 1903)
        ctx.sync()
        with pytest.raises(h.H9GError, match="nothing recorded"):
            ctx.get_monthly()
        ctx.set_monthly(True)
        ctx.push_forcing(1, inp["forcing"][:, 365:])
        ctx.run_year(1, 1904)
        ctx.sync()
        assert ctx.get_monthly(0).shape == (NM, 12 + meta["L"], meta["ncell"])
        for k in (-1, 1):
            with pytest.raises(h.H9GError, match="failed with -1"):
                ctx.get_monthly(k)


# ---- 1. c1_2yr_leap on the L = 8 kinds -----------------------------------
@pytest.mark.parametrize("kernel", ["pair", "pair11", "pair1"])
def test_leap_years_match_host_and_trace(kernel, monkeypatch):
    meta, inp, exp = load_golden("c1_2yr_leap")
    host = _once("leap_host", lambda: host_monthly(**inp))
    snap, _ = _once("leap_trace", lambda: port_snapshots(**inp))
    monkeypatch.setenv("H9G_KERNEL", kernel)
    off = h.run(**inp)
    on = h.run(monthly=True, **inp)
    assert on["rc"] == off["rc"] == 0
    assert same_bits(on["annual"], off["annual"]) and same_bits(on["annual"], exp["annual"])
    assert same_bits(on["state"], off["state"]) and same_bits(on["state"], exp["state"])
    assert _same_errors(on["errors"], off["errors"])
    assert same_bits(on["monthly"], host["monthly"])
    rows = trace_rows(meta["L"])
    assert same_bits(on["monthly"][:, :, rows], snap[:, :, rows])
    check_year_end(on["monthly"], on["annual"], inp["year0"], inp["nisurf"])


# ---- 2. L = 10, NS = 24 on solo, pair2 and both halves of mixed -----------
@pytest.mark.parametrize("kernel", ["solo", "pair2", "mixed"])
def test_l10_kinds_match_host(kernel, monkeypatch):
    inp = l10_inputs(30)
    host = _once("l10_host", lambda: host_monthly(**inp))
    assert host["rc"] == 0
    monkeypatch.setenv("H9G_KERNEL", kernel)
    monkeypatch.setenv("H9G_SPLIT", "17")           # mixed: cells [0, 17) solo, [17, 30) pair
    off = h.run(**inp)
    on = h.run(monthly=True, **inp)
    assert on["rc"] == off["rc"] == 0
    assert same_bits(on["annual"], off["annual"]) and same_bits(on["annual"], host["annual"])
    assert same_bits(on["state"], off["state"]) and same_bits(on["state"], host["state"])
    assert same_bits(on["monthly"], host["monthly"])
    check_year_end(on["monthly"], on["annual"], inp["year0"], inp["nisurf"])


# ---- 3. ragged, several workgroups: sort, slot-ordered I/O, un-permute ----
LISTS = ((3, 1), (0, 3), (120, 5))         # tests/test_gpu_pair1_flux.py


def _strided():
    gid = synth.land_cells()[::331][:200]
    lat = synth.cell_lat(gid, synth.NX05, synth.NY05)
    inp = dict(zi=synth.ZI_L8, params=synth.make_params(gid, 8),
               forcing=synth.make_forcing(gid, lat, synth.year_day0(1901), 365 + 365), nisurf=48, year0=1901,
               nyears=2, grow_on=1)
    return inp, host_monthly(**inp)


def _sub(inp, lo, n):
    return dict(inp, params={k: v[lo:lo + n] for k, v in inp["params"].items()},
                forcing=np.ascontiguousarray(inp["forcing"][:, :, lo:lo + n]))


def test_strided_cells_on_pair_match_host(monkeypatch):
    inp, host = _once("strided", _strided)
    assert host["rc"] == 0
    monkeypatch.setenv("H9G_KERNEL", "pair")
    on = h.run(monthly=True, **inp)
    assert on["rc"] == 0
    assert same_bits(on["annual"], host["annual"]) and same_bits(on["state"], host["state"])
    assert same_bits(on["monthly"], host["monthly"])
    check_year_end(on["monthly"], on["annual"], 1901, 48)


@pytest.mark.parametrize("lo,n", LISTS)
def test_strided_lists_on_pair1_match_host(lo, n, monkeypatch):
    inp, host = _once("strided", _strided)
    monkeypatch.setenv("H9G_KERNEL", "pair1")
    on = h.run(monthly=True, **_sub(inp, lo, n))
    assert on["rc"] == 0
    assert same_bits(on["annual"], host["annual"][:, :, lo:lo + n])
    assert same_bits(on["monthly"], host["monthly"][:, :, :, lo:lo + n])


# ---- 4. STOP and mask conventions -----------------------------------------
@pytest.mark.parametrize("kernel", ["pair", "solo"])
def test_stop_and_masked_cell(kernel, monkeypatch):
    meta, inp = stop_mask_inputs()
    s = meta["stop"]
    host = _once("stop_host", lambda: host_monthly(**inp))
    monkeypatch.setenv("H9G_KERNEL", kernel)
    off = h.run(stop_on_error=False, **inp)
    on = h.run(stop_on_error=False, monthly=True, **inp)
    assert on["rc"] == off["rc"] == s["code"]
    assert same_bits(on["annual"], off["annual"]) and same_bits(on["state"], off["state"])
    assert _same_errors(on["errors"], off["errors"])
    c, mon = s["cell"], on["monthly"]
    ys = int(host["err"][c, 1])
    assert np.isnan(mon[ys:, :, :, c]).all() and not np.isnan(mon[:ys, :, :, c]).any()
    assert np.isnan(mon[:, :, :, 2]).all()
    assert same_bits(mon, host["monthly"])
    check_year_end(mon, on["annual"], inp["year0"], inp["nisurf"])


# ---- 5. the reference's order, small ---------------------------------------
def _co16():
    meta, inp, _ = load_golden("co_c1_30yr")
    nd = sum(h.days_in_year(y) for y in range(1901, 1921))
    return dict(inp, nyears=20, params={k: v[:16] for k, v in inp["params"].items()},
                forcing=np.ascontiguousarray(inp["forcing"][:, :nd, :16]))


def test_cell_order_small_matches_trace():
    """16 cells as their own chain over 1901-1920: the second decade re-runs
    cells, some for one year only (an early merge), one through the decade;
    both APIs give the snapshots the oracle's traced cell-order loop gives."""
    inp = _co16()
    kw = {k: v for k, v in inp.items() if k != "state0"}
    ref = port.run_cell_order(**kw)
    snap, st, ann = cell_order_snapshots(**kw)
    assert ref["rc"] == 0 and same_bits(ann, ref["annual"])
    a = h.run_cell_order(pipelined=True, monthly=True, **inp)
    b = h.run_cell_order(pipelined=False, monthly=True, **inp)
    off = h.run_cell_order(pipelined=True, **inp)
    L = inp["params"]["theta_s"].shape[1]
    for o in (a, b, off):
        assert o["rc"] == 0
        assert same_bits(o["annual"], ref["annual"])
        assert same_bits(o["state"], refcase.pack_state(ref["state"], L))
    assert same_bits(a["monthly"], b["monthly"])
    rows = trace_rows(L)
    assert same_bits(a["monthly"][:, :, rows], snap[:, :, rows])
    check_year_end(a["monthly"], a["annual"], 1901, inp["nisurf"])
    w = b["work"][1]                         # decade 2 of the per-decade run (h9g_decade_stats)
    print(f"co16: decade 2 re-ran {w['rerun_cells']} cells, {w['rerun_cell_years']} cell-years; passes {b['passes']}")
    assert w["rerun_cells"] > 0 and w["rerun_cell_years"] < 10 * w["rerun_cells"]


# ---- 6. the reference's order, re-runs riding ------------------------------
def test_cell_order_band_riding():
    meta, inp, exp = load_golden("co_c2_band")
    nd = sum(h.days_in_year(y) for y in range(1901, 1921))
    inp = dict(inp, nyears=20, forcing=np.ascontiguousarray(inp["forcing"][:, :nd]))
    a = h.run_cell_order(pipelined=True, monthly=True, **inp)
    b = h.run_cell_order(pipelined=False, monthly=True, **inp)
    for o in (a, b):
        assert o["rc"] == 0
        assert same_bits(o["annual"], exp["annual"][:20])
    assert same_bits(a["state"], b["state"])
    assert same_bits(a["monthly"], b["monthly"])
    check_year_end(a["monthly"], a["annual"], 1901, inp["nisurf"])
    print(f"co_c2_band 1901-1920: overlap {a['overlap']}")
    assert a["overlap"]["rerun_years_riding"] > 0


# ---- 7. a STOP inside the reference's order -------------------------------
def test_cell_order_stop():
    meta, inp, _ = load_golden("co_stop")
    off = h.run_cell_order(pipelined=False, **inp)
    on = h.run_cell_order(pipelined=False, monthly=True, **inp)
    assert on["rc"] == off["rc"] == meta["stop"]["code"]
    assert on["err"] == off["err"] and _same_errors(on["errors"], off["errors"])
    assert same_bits(on["annual"], off["annual"]) and same_bits(on["state"], off["state"])
    ny = on["annual"].shape[0]
    check_year_end(on["monthly"][:ny], on["annual"], inp["year0"], inp["nisurf"])
    assert np.isnan(on["monthly"][:, :, :, meta["stop"]["cell"]]).any()


# ---- 8. the Fortran host ---------------------------------------------------
def test_fortran_host_writes_mxy(tmp_path):
    from tests.test_fortran_host import _build
    exe = _build()
    meta, inp, exp = load_golden("c1_10x10")
    n, L = meta["ncell"], meta["L"]
    case = tmp_path / "case"
    refcase.write_case(case, zi=inp["zi"], params=inp["params"], forcing=inp["forcing"], nisurf=inp["nisurf"],
                       year0=inp["year0"], nyears=inp["nyears"], grow_on=inp["grow_on"], state0=None, cell_order=False)
    nml = tmp_path / "h9gpu.nml"
    nml.write_text(f"&h9gpu\n input_mode='case', case_dir='{case}', out_dir='{tmp_path}', monthly=1\n/\n")
    r = subprocess.run([str(exe), str(tmp_path / "no_driver.txt"), str(nml)], capture_output=True, text=True,
                       timeout=600)
    assert "completed successfully" in r.stdout, r.stdout + r.stderr
    ann = np.fromfile(tmp_path / "annual.f32", np.float32).reshape(meta["nyears"], 12 + L, n)
    assert same_bits(ann, exp["annual"])
    out = h.run(monthly=True, **inp)
    zi = np.asarray(inp["zi"], np.float32)
    zc = (zi[1:L + 1] - (zi[1:L + 1] - zi[:L]) / np.float32(2.0)).astype(np.float32)
    for y in range(meta["nyears"]):
        mine = tmp_path / f"py_mxy{inp['year0'] + y}.nc"
        h.write_mxy_nc(mine, out["monthly"][y], np.arange(n), zc, inp["year0"] + y, inp["nisurf"], nx=n, ny=1)
        assert (tmp_path / f"mxy{inp['year0'] + y}.nc").read_bytes() == mine.read_bytes()
