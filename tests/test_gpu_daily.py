"""The daily diagnostics line (HYBRID9.f90:221-229) on the GPU: the shadow
kernel h9g_focus_kernel behind h9g_set_daily / h9g_get_daily against the host
build of cell_focus, the reference golden daily_c1 and the oracle's trace, bit
for bit, in both run modes (isolated cells and the reference's own order), and
through the Fortran host (daily = 1, INTERACTIVE = .T.)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import hybrid9_amd as h
from hybrid9_amd import site, synth
from oracle import port, refcase
from tests.conftest import load_golden, same_bits
from tests.daily_helpers import (F, LINE_INDEX, cell_order_daily8, host_focus, load_daily_golden, port_daily8,
                                 stop_mask_inputs)

pytestmark = pytest.mark.gpu
IDX = list(LINE_INDEX)
I32P = C.POINTER(C.c_int32)


def _years(ctx, forcing, year0, nyears, stop=True):
    """nyears through run_year; (annual, daily or None, rc)."""
    ann, daily, d0, rc = [], [], 0, 0
    for y in range(nyears):
        nt = h.days_in_year(year0 + y)
        ctx.push_forcing(y % 2, forcing[:, d0:d0 + nt, :])
        ctx.run_year(y % 2, year0 + y)
        rc = ctx.sync(raise_on_stop=False)
        ann.append(ctx.get_annual())
        if getattr(ctx, "_nsel", 0):
            daily.append(ctx.get_daily())
        d0 += nt
    return np.stack(ann), (np.concatenate(daily) if daily else None), rc


def test_gpu_daily_golden_isolated_mode():
    meta, inp, exp = load_daily_golden()
    n, L = meta["ncell"], meta["L"]
    host = host_focus(**inp)["daily"]
    with h.Context(n, inp["zi"], nlayers=L, nisurf=inp["nisurf"], grow_on=True) as ctx:
        ctx.set_params(inp["params"])
        ctx.init_state()
        ctx.set_daily(range(n))
        ann, daily, rc = _years(ctx, inp["forcing"], 1901, 2)
        st = ctx.get_state()
        # the same context without a selection
        ctx.init_state()
        ctx.set_daily([])
        ann0, none, rc0 = _years(ctx, inp["forcing"], 1901, 2)
        st0 = ctx.get_state()
    assert rc == rc0 == 0 and none is None
    assert daily.shape == (730, 11, n)
    assert same_bits(daily, host)                                  # all 11 columns
    assert same_bits(daily[:, IDX], exp["daily8"])                 # the reference's eight
    assert same_bits(ann, exp["annual"]) and same_bits(st, exp["state"])
    assert same_bits(ann, ann0) and same_bits(st, st0)
    # the shadow run follows the year kernel's trajectory: the year kernel's
    # annual theta(i) is the f32 running sum of the daily theta(i) over nt
    d0 = 0
    for y, nt in enumerate((365, 365)):
        for i in range(4):
            s = np.zeros(n, F)
            for d in range(d0, d0 + nt):
                s = (s + daily[d, 2 + i]).astype(F)
            assert same_bits((s / F(nt)).astype(F), ann[y, 11 + i]), (y, i)
        d0 += nt


def test_gpu_daily_selection_shapes():
    """A lone lane (nsel = 1) and two waves, the second with one lane
    (nsel = 65), against the oracle's trace; and the API's refusals."""
    g = synth.land_cells()[3::517][:130]
    assert g.size == 130
    p = synth.make_params(g, 8)
    f = synth.make_forcing(g, synth.cell_lat(g), synth.year_day0(1901), 365)
    inp = dict(zi=synth.ZI_L8, params=p, forcing=f, nisurf=24, year0=1901, nyears=1, grow_on=1)
    even = list(range(0, 130, 2))
    traced = sorted(set(even) | {77})
    d8, ref = port_daily8(cells=traced, **inp)
    assert ref["rc"] == 0
    with h.Context(130, synth.ZI_L8, nisurf=24) as ctx:
        lib, hd = ctx._lib, ctx._h
        ctx.set_params(p)
        ctx.init_state()
        st0 = ctx.get_state()
        buf = np.empty((366, 11, 130), np.float32)
        fp = buf.ctypes.data_as(C.POINTER(C.c_float))
        assert lib.h9g_get_daily(hd, 0, fp) == -4                  # H9G_ESTATE: no selection
        for bad in ([5, 3], [3, 3], [-1, 2], [0, 130]):
            a = np.asarray(bad, np.int32)
            assert lib.h9g_set_daily(hd, a.size, a.ctypes.data_as(I32P)) == -1, bad   # H9G_EINVAL
            with pytest.raises(ValueError):
                ctx.set_daily(bad)
        assert lib.h9g_set_daily(hd, 131, np.arange(131, dtype=np.int32).ctypes.data_as(I32P)) == -1
        ctx.set_daily([77])
        assert lib.h9g_get_daily(hd, 0, fp) == -4                  # selected, but nothing run yet
        ann1, one, rc = _years(ctx, f, 1901, 1)
        assert rc == 0 and one.shape == (365, 11, 1)
        assert same_bits(one[:, IDX, 0], d8[:, :, traced.index(77)])
        assert lib.h9g_get_daily(hd, 1, fp) == -1                  # a bad k
        ctx.set_state(st0)
        ctx.set_daily(even)
        ann65, many, rc = _years(ctx, f, 1901, 1)
        assert rc == 0 and many.shape == (365, 11, 65)
        assert same_bits(many[:, IDX], d8[:, :, [traced.index(c) for c in even]])
        assert same_bits(ann1, ann65) and same_bits(ann1, ref["annual"])
        ctx.set_state(st0)
        ctx.set_daily([])                                          # off again
        _years(ctx, f, 1901, 1)
        assert lib.h9g_get_daily(hd, 0, fp) == -4


def test_gpu_daily_stop_and_masked_cell():
    """NaN from the STOP day on, NaN for a masked cell, as the host build; the
    STOP record is the same with and without a selection."""
    meta, inp = stop_mask_inputs()
    s = meta["stop"]
    host = host_focus(**inp)
    kw = dict(inp, stop_on_error=False)
    out = h.run(daily_cells=range(meta["ncell"]), **kw)
    plain = h.run(**kw)
    assert out["rc"] == plain["rc"] == s["code"]
    assert out["err"] == plain["err"] and out["err"]["cell"] == s["cell"] and out["err"]["day"] == s["day"]
    assert all(np.array_equal(out["errors"][k], plain["errors"][k]) for k in ("code", "day", "substep"))
    assert same_bits(out["errors"]["value"], plain["errors"]["value"])
    assert same_bits(out["annual"], plain["annual"]) and same_bits(out["state"], plain["state"])
    d = out["daily"]
    assert same_bits(d, host["daily"])
    assert np.isnan(d[s["day"]:, :, s["cell"]]).all() and not np.isnan(d[:s["day"], :, s["cell"]]).any()
    assert np.isnan(d[:, :, 2]).all()


@pytest.mark.parametrize("chains", [None, [0, 0, 0, 1, 1, 1]], ids=["one_chain", "two_chains"])
def test_gpu_daily_reference_order(chains):
    """Two decades of two years (1909-1910, 1911-1912) in the reference's own
    order: the replay must start every cell from the smp its predecessor in
    the chain hands it.  The isolated-mode lines of the same cells differ, so
    a replay that ignored the carried smp would fail."""
    g = synth.land_cells()[::11003][:6]
    p = synth.make_params(g, 8)
    nd = sum(h.days_in_year(y) for y in range(1909, 1913))
    f = synth.make_forcing(g, synth.cell_lat(g), synth.year_day0(1909), nd)
    inp = dict(zi=synth.ZI_L8, params=p, forcing=f, nisurf=48, year0=1909, nyears=4, grow_on=1)
    d8, st, ann = cell_order_daily8(chains=chains, **inp)
    ref = port.run_cell_order(chains=chains, **inp)
    assert ref["rc"] == 0 and same_bits(ann, ref["annual"])
    assert all(same_bits(st[k], ref["state"][k]) for k in st)
    sel = list(range(6))
    per_decade = h.run_cell_order(chains=chains, pipelined=False, daily_cells=sel, **inp)
    one_call = h.run_cell_order(chains=chains, pipelined=True, daily_cells=sel, **inp)
    for out in (per_decade, one_call):
        assert out["rc"] == 0
        assert same_bits(out["annual"], ref["annual"])
        assert same_bits(out["state"], refcase.pack_state(ref["state"], 8))
        assert out["daily"].shape == (nd, 11, 6)
        assert same_bits(out["daily"][:, IDX], d8)
    assert same_bits(per_decade["daily"], one_call["daily"])
    if chains is None:
        iso = h.run(daily_cells=sel, **inp)
        differ = iso["daily"][:, IDX].view(np.uint32) != d8.view(np.uint32)
        assert differ.any(axis=(0, 1)).sum() == 5, differ.sum()   # 5 of the 6 cells (the oracle on the CPU)
        # without a selection the ordered call is as before
        plain = h.run_cell_order(pipelined=True, **inp)
        assert same_bits(plain["annual"], one_call["annual"]) and same_bits(plain["state"], one_call["state"])
        assert "daily" not in plain


def test_gpu_daily_l10_ns24():
    g = synth.land_cells(synth.NX025, synth.NY025, synth.NLAND025)[11::1601][:4]
    p = synth.make_params(g, 10)
    f = synth.make_forcing(g, synth.cell_lat(g, synth.NX025, synth.NY025), synth.year_day0(1903), 365)
    inp = dict(zi=synth.ZI_L10, params=p, forcing=f, nisurf=24, year0=1903, nyears=1, grow_on=1)
    d8, ref = port_daily8(**inp)
    out = h.run(daily_cells=range(4), **inp)
    assert ref["rc"] == out["rc"] == 0
    assert same_bits(out["daily"][:, IDX], d8)
    assert same_bits(out["daily"], host_focus(**inp)["daily"])
    assert same_bits(out["annual"], ref["annual"])


def test_gpu_daily_runtime_geometry():
    """A NISURF that has no compile-time geometry (the GeoR instantiation)."""
    meta, inp, _ = load_daily_golden()
    f = np.ascontiguousarray(inp["forcing"][:, :365, :3])
    p = {k: v[:3] for k, v in inp["params"].items()}
    kw = dict(inp, params=p, forcing=f, nisurf=12, nyears=1)
    out = h.run(daily_cells=[0, 2], **kw)
    assert out["rc"] == 0
    assert same_bits(out["daily"], host_focus(const_geo=0, **kw)["daily"][:, :, [0, 2]])


def _host_exe():
    from tests.test_fortran_host import _build
    return _build()


def test_gpu_daily_fortran_host_case_mode(tmp_path):
    """h9gpu namelist daily = 1: <out_dir>/daily.f32 (cell fastest, 11, total
    days) equals the Python API's lines."""
    exe = _host_exe()
    meta, inp, exp = load_golden("c1_10x10")
    n, L = meta["ncell"], meta["L"]
    case = tmp_path / "case"
    refcase.write_case(case, zi=inp["zi"], params=inp["params"], forcing=inp["forcing"], nisurf=inp["nisurf"],
                       year0=inp["year0"], nyears=inp["nyears"], grow_on=inp["grow_on"])
    nml = tmp_path / "h9gpu.nml"
    nml.write_text(f"&h9gpu\n input_mode='case', case_dir='{case}', out_dir='{tmp_path}', daily=1\n/\n")
    r = subprocess.run([str(exe), str(tmp_path / "no_driver.txt"), str(nml)], capture_output=True, text=True,
                       timeout=600)
    assert "completed successfully" in r.stdout, r.stdout + r.stderr
    nd = inp["forcing"].shape[1]
    got = np.fromfile(tmp_path / "daily.f32", np.float32).reshape(nd, 11, n)
    api = h.run(daily_cells=range(n), **inp)
    assert same_bits(got, api["daily"])
    assert same_bits(np.fromfile(tmp_path / "annual.f32", np.float32).reshape(meta["nyears"], 12 + L, n),
                     exp["annual"])


def test_gpu_daily_fortran_host_interactive(tmp_path):
    """INTERACTIVE = .T. in driver.txt on a small synthetic grid: the land
    list is cut to the 2 x 2 focus window and LCLIM/daily_diag.csv has the
    reference's header and one line per (cell, year, day) in its order
    decade -> cell -> year -> day, each number the API's value to the 4
    decimals F10.4 prints."""
    exe = _host_exe()
    nx, ny, nland = 20, 10, 48
    gid = synth.land_cells(nx, ny, nland)
    land = set(gid.tolist())
    # the 2 x 2 window with the most land cells (first such in raster order)
    best = max(((sum(((y + dy) * nx + x + dx) in land for dy in (0, 1) for dx in (0, 1)), -y, -x)
                for y in range(ny - 1) for x in range(nx - 1)))
    y0, x0 = -best[1], -best[2]
    lon_w, lat_w = -180.0 + (x0 + 0.5) * 360.0 / nx, 90.0 - (y0 + 0.5) * 180.0 / ny
    lon_s, lat_s, wg = site.focus_window(lon_w, lat_w, 2, 2, nx=nx, ny=ny)
    assert (lon_s, lat_s) == (x0 + 1, y0 + 1)
    cells = np.asarray([c for c in wg.tolist() if c in land], np.int64)      # (y, x) order
    assert cells.size == best[0] >= 2
    drv = tmp_path / "driver.txt"
    drv.write_text(f"'{tmp_path}'\n48\n.T.\n 1\n 1\n.T.\n .F.\n 'a'\n 'b'\n 1901\n 1902\n 0\n{lon_w}\n{lat_w}\n 2\n 2\n" +
                   "".join(f"{v}\n" for v in synth.ZI_L8[:10]))
    nml = tmp_path / "h9gpu.nml"
    nml.write_text(f"&h9gpu\n input_mode='synth', out_dir='{tmp_path}', grow_on=1, nyears=2, nc_out=0,\n"
                   f" gnx={nx}, gny={ny}, gnland={nland}\n/\n")
    r = subprocess.run([str(exe), str(drv), str(nml)], capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert "completed successfully" in r.stdout, r.stdout + r.stderr
    assert "in cell order" in r.stdout
    # the Python mirror: the window's cells alone, the reference's order
    m = int(cells.size)
    with h.Context(m, synth.ZI_L8, nisurf=48, nslots=2) as ctx:
        ctx.set_cells(cells, synth.cell_lat(cells, nx, ny))
        ctx.synth_params(synth.SEED)
        ctx.init_state()
        ctx.synth_forcing(0, synth.SEED, 0, 365)
        ctx.synth_forcing(1, synth.SEED, 365, 365)
        ctx.set_daily(range(m))
        ctx.run_decade_ordered([0, 1], 1901)
        api = np.concatenate([ctx.get_daily(0), ctx.get_daily(1)])
    assert not np.isnan(api).any()
    lines = (tmp_path / "LCLIM" / "daily_diag.csv").read_text().split("\n")
    assert lines[0] == site.DAILY_HEADER and lines[-1] == ""
    rows = lines[1:-1]
    assert len(rows) == m * 730
    k = 0
    for c in range(m):
        for yi, year in enumerate((1901, 1902)):
            for doy in range(1, 366):
                v = rows[k].split(",")
                assert len(rows[k]) == 2 * 6 + 10 * 11 + 10 and len(v) == 13
                assert (int(v[0]), int(v[1])) == (year, doy), (k, rows[k])
                got = np.asarray([float(t) for t in v[2:]])
                assert np.all(np.abs(got - api[yi * 365 + doy - 1, :, c].astype(np.float64)) <= 0.5e-4), rows[k]
                k += 1
    # and the same lines as daily.f32, bit for bit
    assert same_bits(np.fromfile(tmp_path / "daily.f32", np.float32).reshape(730, 11, m), api)
