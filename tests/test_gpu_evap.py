"""Evapotranspiration output on the GPU: the ET year kernels (every kind the
dispatch can choose, both run modes) fill row evap of the annual means and of
the month-end snapshots with the year's evaporation sum -- the definition
restated over the oracle's per-substep trace (tests/evap_helpers.py) and the
host build of the same code (tests/csrc/host_evap.cpp), bit for bit -- and
leave every other row, the state and the STOP records exactly as a run with
recording off leaves them.  Every comparison is conftest.same_bits: no
tolerance.  Runs on an MI355X only."""
import subprocess

import numpy as np
import pytest

import hybrid9_amd as h
from hybrid9_amd import synth
from oracle import refcase
from tests.conftest import load_golden, same_bits
from tests.daily_helpers import stop_mask_inputs
from tests.evap_helpers import R_EVAP, cell_order_evap, host_evap, others, port_evap
from tests.monthly_helpers import NM, l10_inputs

pytestmark = pytest.mark.gpu

_cache = {}


def _once(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _same_errors(a, b):
    return all(same_bits(a[k], b[k]) for k in ("code", "day", "substep", "value"))


def _run(inp, evap, monthly):
    """hybrid9_amd.run on one context, with the name of the kernel its years ran on."""
    L = inp["params"]["theta_s"].shape[1]
    n = inp["params"]["fmax"].size
    with h.Context(n, inp["zi"], nlayers=L, nisurf=inp["nisurf"], grow_on=inp["grow_on"]) as ctx:
        ctx.set_params(inp["params"])
        if inp.get("state0") is None:
            ctx.init_state()
        else:
            ctx.set_state(inp["state0"])
        ctx.set_monthly(monthly)
        ctx.set_evap(evap)
        ann, mon, d0 = [], [], 0
        for y in range(inp["nyears"]):
            nt = h.days_in_year(inp["year0"] + y)
            ctx.push_forcing(y % 2, inp["forcing"][:, d0:d0 + nt, :])
            ctx.run_year(y % 2, inp["year0"] + y)
            rc = ctx.sync(raise_on_stop=False)
            ann.append(ctx.get_annual())
            if monthly:
                mon.append(ctx.get_monthly())
            d0 += nt
        return dict(rc=rc, annual=np.stack(ann), monthly=np.stack(mon) if monthly else None, state=ctx.get_state(),
                    errors=ctx.get_errors(), name=ctx.kernel_name())


def _check_on_off(on, off, L, monthly):
    """Everything but row evap is the ET-off run's; row evap there is +0."""
    o = others(L)
    assert on["rc"] == off["rc"]
    assert same_bits(on["annual"][:, o], off["annual"][:, o])
    assert same_bits(on["state"], off["state"]) and _same_errors(on["errors"], off["errors"])
    ran = ~np.isnan(off["annual"][:, R_EVAP])
    assert same_bits(off["annual"][:, R_EVAP][ran], np.zeros(int(ran.sum()), np.float32))
    if monthly:
        assert same_bits(on["monthly"][:, :, o], off["monthly"][:, :, o])


# ---- 1. c1_2yr_leap on the L = 8 kinds ---------------------------------------
@pytest.mark.parametrize("monthly", [False, True], ids=["annual", "monthly"])
@pytest.mark.parametrize("kernel", ["pair", "pair11", "pair1"])
def test_leap_years_match_trace_and_host(kernel, monthly, monkeypatch):
    meta, inp, exp = load_golden("c1_2yr_leap")
    ea, em, _ = _once("leap_trace", lambda: port_evap(**inp))
    host = _once("leap_host", lambda: host_evap(**inp))
    monkeypatch.setenv("H9G_KERNEL", kernel)
    off = _run(inp, False, monthly)
    on = _run(inp, True, monthly)
    assert on["rc"] == 0 and same_bits(off["annual"], exp["annual"]) and same_bits(on["state"], exp["state"])
    assert on["name"].split("<")[0].endswith("_et_kernel"), on["name"]
    assert on["name"].split("<")[0] == off["name"].split("<")[0].replace("_kernel", "_et_kernel")
    _check_on_off(on, off, meta["L"], monthly)
    assert same_bits(on["annual"][:, R_EVAP], ea) and same_bits(on["annual"], host["annual"])
    if monthly:
        assert same_bits(on["monthly"][:, :, R_EVAP], em) and same_bits(on["monthly"], host["monthly"])


def test_off_again_is_the_reference_zero(monkeypatch):
    """set_evap(False) after set_evap(True): the plain kernel and +0 again."""
    meta, inp, exp = load_golden("c1_2yr_leap")
    with h.Context(meta["ncell"], inp["zi"], nisurf=inp["nisurf"], grow_on=inp["grow_on"]) as ctx:
        plain = ctx.kernel_name()
        ctx.set_evap(True)
        assert ctx.kernel_name() == plain.replace("_kernel", "_et_kernel")
        ctx.set_evap(False)
        assert ctx.kernel_name() == plain
        ctx.set_params(inp["params"])
        ctx.init_state()
        ctx.push_forcing(0, inp["forcing"][:, :365])
        ctx.run_year(0, 1903)
        ctx.sync()
        assert same_bits(ctx.get_annual(), exp["annual"][0])


# ---- 2. L = 10, NS = 24 on solo, pair2 and both halves of mixed --------------
@pytest.mark.parametrize("kernel", ["solo", "pair2", "mixed"])
def test_l10_kinds_match_host(kernel, monkeypatch):
    inp = l10_inputs(30)
    host = _once("l10_host", lambda: host_evap(**inp))
    assert host["rc"] == 0
    monkeypatch.setenv("H9G_KERNEL", kernel)
    monkeypatch.setenv("H9G_SPLIT", "17")           # mixed: cells [0, 17) solo, [17, 30) pair
    off = h.run(monthly=True, **inp)
    on = h.run(monthly=True, evap=True, **inp)
    assert on["rc"] == off["rc"] == 0
    _check_on_off(on, off, 10, True)
    assert same_bits(on["annual"], host["annual"]) and same_bits(on["state"], host["state"])
    assert same_bits(on["monthly"], host["monthly"])


# ---- 3. the single-wave one-column kernel -------------------------------------
def _synth_et(gid):
    lat = synth.cell_lat(gid, synth.NX05, synth.NY05)
    with h.Context(gid.size, synth.ZI_L8, nlayers=8, nisurf=48, grow_on=False) as ctx:
        ctx.set_cells(gid, lat)
        ctx.synth_params(synth.SEED)
        ctx.init_state()
        ctx.set_evap(True)
        before = ctx.kernel_name()
        ctx.synth_forcing(0, synth.SEED, synth.year_day0(1901), 365)
        ctx.run_year(0, 1901)
        ctx.sync(raise_on_stop=False)
        return ctx.get_annual(), ctx.get_state(), ctx.get_errors(), ctx.kernel_name(), before


@pytest.mark.parametrize("n", [512, 513])
def test_pair1_shapes_match_the_pair_kernel(n, monkeypatch):
    """513 cells run on the single-wave h9g_pair1_et_kernel, 512 on the two-wave
    h9g_pair1f_et_kernel (a build without it, H9G_P1_FRONT=0: the single-wave
    kernel at both sizes); the shape is read from the launch record."""
    monkeypatch.setenv("H9G_KERNEL", "pair")
    gid = synth.land_cells()[::131][:513]
    ann_all, st_all, err_all, name_all, _ = _once("big", lambda: _synth_et(gid))
    assert name_all.startswith("h9g_pair_et_kernel<"), name_all
    monkeypatch.setenv("H9G_KERNEL", "pair1")
    ann, st, err, name, before = _synth_et(gid[:n])
    front = _once("front", lambda: _synth_et(gid[:1])[4].startswith("h9g_pair1f_et_kernel<"))
    want = "h9g_pair1f_et_kernel<" if front and n <= 512 else "h9g_pair1_et_kernel<"
    print(f"built with the two-wave shape: {front}; {n} cells ran on {name}")
    assert name.startswith(want), (name, want)
    assert same_bits(ann, ann_all[:, :n]) and (ann[R_EVAP] != 0).all()
    assert all(same_bits(np.asarray(err[k]), np.asarray(err_all[k])[:n]) for k in ("code", "day", "substep", "value"))
    full, part = refcase.unpack_state(st_all, gid.size, 8), refcase.unpack_state(st, n, 8)
    for k in part:
        assert same_bits(part[k], full[k][:n]), k


# ---- 4. runtime geometry --------------------------------------------------------
def test_runtime_geometry_matches_host_geor():
    """NISURF = 36 (neither 24 nor 48): the GeoR kernels, dt = 2400 s."""
    meta, inp, _ = load_golden("c1_2yr_leap")
    inp = dict(inp, nisurf=36, nyears=1, params={k: v[:4] for k, v in inp["params"].items()},
               forcing=np.ascontiguousarray(inp["forcing"][:, :365, :4]))
    host = host_evap(const_geo=0, **inp)
    ea, em, ref = port_evap(**inp)
    assert host["rc"] == ref["rc"] == 0
    on = _run(inp, True, True)
    assert "GeoR" in on["name"] and on["name"].split("<")[0].endswith("_et_kernel"), on["name"]
    assert on["rc"] == 0
    assert same_bits(on["annual"], host["annual"]) and same_bits(on["monthly"], host["monthly"])
    assert same_bits(on["state"], host["state"])
    assert same_bits(on["annual"][:, R_EVAP], ea) and same_bits(on["monthly"][:, :, R_EVAP], em)


# ---- 5. STOP and mask conventions -----------------------------------------------
@pytest.mark.parametrize("kernel", ["pair", "solo"])
def test_stop_and_masked_cell(kernel, monkeypatch):
    meta, inp = stop_mask_inputs()
    s = meta["stop"]
    host = _once("stop_host", lambda: host_evap(**inp))
    monkeypatch.setenv("H9G_KERNEL", kernel)
    off = h.run(stop_on_error=False, monthly=True, **inp)
    on = h.run(stop_on_error=False, monthly=True, evap=True, **inp)
    assert on["rc"] == off["rc"] == s["code"]
    _check_on_off(on, off, meta["L"], True)
    c = s["cell"]
    ys = int(host["err"][c, 1])
    for rows in (on["annual"][:, R_EVAP], on["monthly"][:, :, R_EVAP]):
        assert np.isnan(rows[ys:, ..., c]).all() and np.isfinite(rows[:ys, ..., c]).all()
        assert np.isnan(rows[..., 2]).all()
    assert same_bits(on["annual"], host["annual"]) and same_bits(on["monthly"], host["monthly"])


# ---- 6. the reference's order, small ---------------------------------------------
def _co16():
    meta, inp, _ = load_golden("co_c1_30yr")
    nd = sum(h.days_in_year(y) for y in range(1901, 1921))
    return dict(inp, nyears=20, params={k: v[:16] for k, v in inp["params"].items()},
                forcing=np.ascontiguousarray(inp["forcing"][:, :nd, :16]))


@pytest.mark.parametrize("nchains", [1, 2])
def test_cell_order_small_matches_trace(nchains):
    """The 16 cells and two decades of test_gpu_monthly's small cell-order test,
    as one chain and as two, with ET and monthly recording on: rows 3 of every
    year and month against the cell-order loop restated over full traces."""
    inp = _co16()
    chains = None if nchains == 1 else np.repeat(np.arange(2), 8)
    kw = {k: v for k, v in inp.items() if k != "state0"}
    ea, em, st, ann = cell_order_evap(chains=chains, **kw)
    a = h.run_cell_order(pipelined=True, monthly=True, evap=True, chains=chains, **inp)
    b = h.run_cell_order(pipelined=False, monthly=True, evap=True, chains=chains, **inp)
    off = h.run_cell_order(pipelined=True, monthly=True, chains=chains, **inp)
    L = inp["params"]["theta_s"].shape[1]
    o = others(L)
    assert same_bits(off["annual"], ann) and same_bits(off["state"], refcase.pack_state(st, L))
    for r in (a, b):
        assert r["rc"] == 0
        assert same_bits(r["annual"][:, o], off["annual"][:, o]) and same_bits(r["state"], off["state"])
        assert same_bits(r["monthly"][:, :, o], off["monthly"][:, :, o])
        assert same_bits(r["annual"][:, R_EVAP], ea)
        assert same_bits(r["monthly"][:, :, R_EVAP], em)
    w = b["work"][1]
    print(f"co16, {nchains} chain(s): decade 2 re-ran {w['rerun_cells']} cells, {w['rerun_cell_years']} cell-years; "
          f"passes {b['passes']}")
    assert w["rerun_cells"] > 0


# ---- 7. the reference's order, re-runs riding ---------------------------------------
def test_cell_order_band_riding(monkeypatch):
    meta, inp, exp = load_golden("co_c2_band")
    nd = sum(h.days_in_year(y) for y in range(1901, 1921))
    inp = dict(inp, nyears=20, forcing=np.ascontiguousarray(inp["forcing"][:, :nd]))
    a = h.run_cell_order(pipelined=True, monthly=True, evap=True, **inp)
    b = h.run_cell_order(pipelined=False, monthly=True, evap=True, **inp)
    o = others(meta["L"])
    for r in (a, b):
        assert r["rc"] == 0
        assert same_bits(r["annual"][:, o], exp["annual"][:20][:, o])
    assert same_bits(a["annual"], b["annual"]) and same_bits(a["monthly"], b["monthly"])
    assert same_bits(a["state"], b["state"])
    ev = a["annual"][:, R_EVAP]
    assert np.isfinite(ev).all() and (ev != 0).all()
    print(f"co_c2_band 1901-1920 with ET: overlap {a['overlap']}")
    assert a["overlap"]["rerun_years_riding"] > 0 and a["overlap"]["probed"] > 0
    monkeypatch.setenv("H9G_NO_PROBE", "1")
    c = h.run_cell_order(pipelined=True, monthly=True, evap=True, **inp)
    assert c["rc"] == 0 and c["overlap"]["probed"] == 0
    assert same_bits(c["annual"], a["annual"]) and same_bits(c["monthly"], a["monthly"])
    assert same_bits(c["state"], a["state"])


# ---- 8. a STOP inside the reference's order ----------------------------------------
def test_cell_order_stop():
    meta, inp, _ = load_golden("co_stop")
    off = h.run_cell_order(pipelined=False, **inp)
    on = h.run_cell_order(pipelined=False, evap=True, **inp)
    assert on["rc"] == off["rc"] == meta["stop"]["code"]
    assert on["err"] == off["err"] and _same_errors(on["errors"], off["errors"])
    o = others(meta["L"])
    assert same_bits(on["annual"][:, o], off["annual"][:, o]) and same_bits(on["state"], off["state"])
    c = meta["stop"]["cell"]
    ev = on["annual"][:, R_EVAP]
    assert np.isnan(ev[:, c]).any()
    done = ~np.isnan(off["annual"][:, 0])              # the cell-years that completed
    assert np.isnan(ev[~done]).all() and np.isfinite(ev[done]).all() and (ev[done] != 0).all()


# ---- 9. the Fortran host --------------------------------------------------------------
def test_fortran_host_evap(tmp_path):
    """evap = 1 on the golden of test_fortran_host_writes_mxy.  A case's cells
    form no grid, so the host writes no axyYYYY.nc for it: the annual means it
    would hand to h9g_write_axy_nc are annual.f32, held to the Python run's, and
    mxyYYYY.nc is the file write_mxy_nc(evap=True) writes."""
    from scipy.io import netcdf_file
    from tests.test_fortran_host import _build
    exe = _build()
    meta, inp, exp = load_golden("c1_10x10")
    n, L = meta["ncell"], meta["L"]
    case = tmp_path / "case"
    refcase.write_case(case, zi=inp["zi"], params=inp["params"], forcing=inp["forcing"], nisurf=inp["nisurf"],
                       year0=inp["year0"], nyears=inp["nyears"], grow_on=inp["grow_on"], state0=None, cell_order=False)
    nml = tmp_path / "h9gpu.nml"
    nml.write_text(f"&h9gpu\n input_mode='case', case_dir='{case}', out_dir='{tmp_path}', monthly=1, evap=1\n/\n")
    r = subprocess.run([str(exe), str(tmp_path / "no_driver.txt"), str(nml)], capture_output=True, text=True,
                       timeout=600)
    assert "completed successfully" in r.stdout, r.stdout + r.stderr
    out = h.run(monthly=True, evap=True, **inp)
    ann = np.fromfile(tmp_path / "annual.f32", np.float32).reshape(meta["nyears"], 12 + L, n)
    assert same_bits(ann, out["annual"]) and (ann[:, R_EVAP] > 0).all()
    assert same_bits(ann[:, others(L)], exp["annual"][:, others(L)])
    zi = np.asarray(inp["zi"], np.float32)
    zc = (zi[1:L + 1] - (zi[1:L + 1] - zi[:L]) / np.float32(2.0)).astype(np.float32)
    for y in range(meta["nyears"]):
        jy = inp["year0"] + y
        mine = tmp_path / f"py_mxy{jy}.nc"
        h.write_mxy_nc(mine, out["monthly"][y], np.arange(n), zc, jy, inp["nisurf"], nx=n, ny=1, evap=True)
        assert (tmp_path / f"mxy{jy}.nc").read_bytes() == mine.read_bytes()
        with netcdf_file(tmp_path / f"mxy{jy}.nc", "r", mmap=False) as nc:
            got = np.array(nc.variables["evaporation"][:]).reshape(NM, n)
        assert same_bits(got, h.monthly_means(out["monthly"][y], jy, inp["nisurf"], evap=True)[:, R_EVAP])
        assert (got > 0).all()
