"""Runtime layer geometry on the GPU: every kernel kind, the monthly and ET
siblings, both one-column shapes, ragged waves, the ordered mode, the focus
kernel, the site kernel and the NaN-parameter paths, all on the GeoR
instantiations at layer interfaces other than the two compile-time sets --
against the reference's goldens of kind `geo` and co_geo_a
(tests/golden/make_golden.py main_geo), the host build with runtime geometry
and the oracle (itself pinned to the same goldens by tests/test_geo.py).
What only the device build has -- the s_zt table in LDS (fill_zt) and the GeoR
kernel argument of each kernel -- is compared here and nowhere else.  Every
comparison is conftest.same_bits: no tolerance.  Every test first asserts that
its context names a GeoR kernel.  Runs on an MI355X only."""
import numpy as np
import pytest

import hybrid9_amd as h
from hybrid9_amd import synth
from oracle import port, refcase
from tests.conftest import load_golden, same_bits
from tests.daily_helpers import LINE_INDEX, host_focus, port_daily8
from tests.evap_helpers import R_EVAP, host_evap, others, port_evap
from tests.geo_helpers import first_cells, load_geo_golden
from tests.golden.make_golden import LCLIM_EVENTS_2004, ZI_GEO_A, ZI_GEO_C, site_inputs
from tests.monthly_helpers import host_monthly

pytestmark = pytest.mark.gpu

NTHREADS = 16   # oracle threads on the GPU box (its CPU share)
IDX = list(LINE_INDEX)
_cache = {}


def _once(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _geo_name(n, zi, nisurf, grow_on=True):
    """The kernel a context of this configuration runs its years on (under the
    H9G_KERNEL of the moment); must be a GeoR instantiation."""
    zi = np.asarray(zi, np.float32)
    with h.Context(n, zi, nlayers=zi.size - 2, nisurf=nisurf, grow_on=bool(grow_on)) as ctx:
        name = ctx.kernel_name()
    assert "GeoR" in name and "GeoC" not in name, name
    return name


def _name_of(inp):
    return _geo_name(inp["params"]["fmax"].size, inp["zi"], inp["nisurf"], inp["grow_on"])


def _same_errors(a, b, sel=slice(None)):
    return all(same_bits(np.asarray(a[k]), np.asarray(b[k])[sel]) for k in ("code", "day", "substep", "value"))


# ---- 1. isolated mode, every kind, against the reference ---------------------
CASES = ([(g, k) for g in ("geo_a_ns36", "geo_b_ns12") for k in ("pair", "pair11", "pair1", "solo", "mixed")]
         + [("geo_c_ns24", k) for k in ("pair", "pair2", "pair11", "pair1", "solo", "mixed")])


@pytest.mark.parametrize("name,kernel", CASES)
def test_every_kind_matches_reference_geo(name, kernel, monkeypatch):
    """32 cells x 1903-1904: one full 22-column wave and a ragged one, three
    11-column waves, 32 one-column workgroups, a 13 | 19 mixed split."""
    monkeypatch.setenv("H9G_KERNEL", kernel)
    monkeypatch.setenv("H9G_SPLIT", "13")
    meta, inp, exp = load_geo_golden(name)
    kname = _name_of(inp)
    stems = {"mixed": ("h9g_solo_kernel<",), "pair1": ("h9g_pair1_kernel<", "h9g_pair1f_kernel<")}
    assert kname.startswith(stems.get(kernel, (f"h9g_{kernel}_kernel<",))), kname
    out = h.run(**inp)
    assert out["rc"] == 0, out["err"]
    assert same_bits(out["annual"], exp["annual"])
    assert same_bits(out["state"], exp["state"])


# ---- 2. the dispatch boundary --------------------------------------------------
ZI_L8_LAST = synth.ZI_L8.copy()
ZI_L8_LAST[9] = 4400.0        # only zi(L+1) differs from the compile-time set


@pytest.mark.parametrize("kernel,zi,nisurf,cells,want", [
    ("pair", ZI_L8_LAST, 48, 3, "h9g_pair_kernel<8,GeoR>"),
    ("pair2", ZI_GEO_C, 24, 30, "h9g_pair2_kernel<10,GeoR>"),
    ("pair11", ZI_GEO_A, 48, 3, "h9g_pair11_kernel<8,GeoR>"),
], ids=["zi9_ns48", "setC_ns24_pair2", "setA_pair11"])
def test_kernel_name_at_the_geometry_boundary(kernel, zi, nisurf, cells, want, monkeypatch):
    """A single interface off the compile-time set, or a NISURF the compile-time
    sets have with other layers, is runtime geometry: before any year and after one."""
    monkeypatch.setenv("H9G_KERNEL", kernel)
    L = zi.size - 2
    gid = synth.land_cells()[::331][:cells]
    with h.Context(gid.size, zi, nlayers=L, nisurf=nisurf, grow_on=False) as ctx:
        assert ctx.kernel_name() == want
        ctx.set_cells(gid, synth.cell_lat(gid, synth.NX05, synth.NY05))
        ctx.synth_params(synth.SEED)
        ctx.init_state()
        ctx.synth_forcing(0, synth.SEED, synth.year_day0(1903), synth.days_in_year(1903))
        ctx.run_year(0, 1903)
        ctx.sync()
        assert ctx.kernel_name() == want


# ---- 3. the monthly and ET siblings ---------------------------------------------
@pytest.mark.parametrize("name,kernel", [("geo_a_ns36", k) for k in ("pair", "pair11", "pair1", "solo")]
                         + [("geo_c_ns24", k) for k in ("pair2", "mixed")])
def test_monthly_and_et_siblings_geo(name, kernel, monkeypatch):
    meta, inp, exp = load_geo_golden(name)
    L = meta["L"]
    o = others(L)
    hm = _once(("host_monthly", name), lambda: host_monthly(const_geo=0, **inp))
    he = _once(("host_evap", name), lambda: host_evap(const_geo=0, **inp))
    ea, em, ref = _once(("port_evap", name), lambda: port_evap(**inp))
    assert hm["rc"] == he["rc"] == ref["rc"] == 0
    monkeypatch.setenv("H9G_KERNEL", kernel)
    monkeypatch.setenv("H9G_SPLIT", "13")
    _name_of(inp)
    mon = h.run(monthly=True, **inp)
    et = h.run(monthly=True, evap=True, **inp)
    for out in (mon, et):
        assert out["rc"] == 0, out["err"]
        assert same_bits(out["annual"][:, o], exp["annual"][:, o])
        assert same_bits(out["state"], exp["state"])
    assert same_bits(mon["annual"], hm["annual"]) and same_bits(mon["monthly"], hm["monthly"])
    assert same_bits(mon["annual"], exp["annual"])
    assert same_bits(et["annual"], he["annual"]) and same_bits(et["monthly"], he["monthly"])
    assert same_bits(et["annual"][:, R_EVAP], ea) and same_bits(et["monthly"][:, :, R_EVAP], em)
    assert (et["annual"][:, R_EVAP] != 0).all()


# ---- 4./5. device-generated inputs at layers A: 513 cells ---------------------------
def _synth_a(gid, year=1903):
    """Cells gid at layers A, NISURF 36, GROW on, one year, inputs made on the device."""
    lat = synth.cell_lat(gid, synth.NX05, synth.NY05)
    with h.Context(gid.size, ZI_GEO_A, nlayers=8, nisurf=36, grow_on=True) as ctx:
        assert "GeoR" in ctx.kernel_name(), ctx.kernel_name()
        ctx.set_cells(gid, lat)
        ctx.synth_params(synth.SEED)
        ctx.init_state()
        ctx.synth_forcing(0, synth.SEED, synth.year_day0(year), synth.days_in_year(year))
        ctx.run_year(0, year)
        ctx.sync(raise_on_stop=False)
        name = ctx.kernel_name()
        assert "GeoR" in name, name
        return ctx.get_annual(), ctx.get_state(), ctx.get_errors(), name


def _big(monkeypatch):
    monkeypatch.setenv("H9G_KERNEL", "pair")
    gid = synth.land_cells()[::131][:513]
    assert gid.size == 513
    return (gid,) + _once("big", lambda: _synth_a(gid))


def _check_part(part, n, big, lo):
    ann, st, err, _ = part
    _, ann_all, st_all, err_all, _ = big
    assert same_bits(ann, ann_all[:, lo:lo + n]), (lo, n)
    assert _same_errors(err, err_all, slice(lo, lo + n)), (lo, n)
    full, got = refcase.unpack_state(st_all, ann_all.shape[1], 8), refcase.unpack_state(st, n, 8)
    for k in got:
        assert same_bits(got[k], full[k][lo:lo + n]), (lo, n, k)


def test_pair_kernel_513_cells_sampled_against_oracle(monkeypatch):
    gid, ann, st, err, name = _big(monkeypatch)
    assert name == "h9g_pair_kernel<8,GeoR>"
    sample = np.arange(7, 513, 32)
    assert sample.size == 16
    g = gid[sample]
    p = synth.make_params(g, 8)
    f = synth.make_forcing(g, synth.cell_lat(g), synth.year_day0(1903), 365)
    ref = port.run(zi=ZI_GEO_A, params=p, forcing=f, nisurf=36, year0=1903, nyears=1, grow_on=1, nthreads=NTHREADS)
    assert same_bits(ann[:, sample], ref["annual"][0])
    assert np.array_equal(np.asarray(err["code"])[sample], ref["errors"]["code"])
    got = refcase.unpack_state(st, gid.size, 8)
    for k, v in ref["state"].items():
        assert same_bits(got[k][sample], v), k


@pytest.mark.parametrize("n", [512, 513])
def test_pair1_shapes_match_the_pair_kernel_geo(n, monkeypatch):
    """512 cells: the two-wave shape (where the library has it), 513: the
    single-wave kernel; the shape is read from the launch record."""
    big = _big(monkeypatch)
    monkeypatch.setenv("H9G_KERNEL", "pair1")
    front = _geo_name(1, ZI_GEO_A, 36).startswith("h9g_pair1f_kernel<")
    part = _synth_a(big[0][:n])
    want = "h9g_pair1f_kernel<8,GeoR>" if front and n <= 512 else "h9g_pair1_kernel<8,GeoR>"
    assert part[3] == want, (part[3], want)
    _check_part(part, n, big, 0)


@pytest.mark.parametrize("kernel", ["pair", "pair11"])
def test_spare_lanes_in_ragged_waves_geo(kernel, monkeypatch):
    """Waves of 1, 3, 9 and 22 + 1 (11 + 11 + 1) columns: the helper lanes
    read the geometry table for the pairs they serve."""
    big = _big(monkeypatch)
    monkeypatch.setenv("H9G_KERNEL", kernel)
    for lo, n in ((0, 1), (5, 3), (101, 9), (300, 23)):
        part = _synth_a(big[0][lo:lo + n])
        assert part[3] == f"h9g_{kernel}_kernel<8,GeoR>", part[3]
        _check_part(part, n, big, lo)


# ---- 6. the ordered mode -----------------------------------------------------------
@pytest.mark.parametrize("pipelined", [True, False], ids=["pipelined", "per_decade"])
def test_cell_order_matches_reference_geo(pipelined):
    meta, inp, exp = load_golden("co_geo_a")
    _name_of(inp)
    out = h.run_cell_order(pipelined=pipelined, **inp)
    assert out["rc"] == 0, out["err"]
    assert same_bits(out["annual"], exp["annual"])
    assert same_bits(out["state"], exp["state"])
    reran = sum(w["rerun_cell_years"] for w in out["work"])
    print(f"co_geo_a pipelined={pipelined}: re-ran {reran} cell-years, passes {out['passes']}")
    assert reran > 0


def _oracle_chains(inp, chains):
    """port.run_cell_order(chains=chains), every chain on a thread of its own:
    chains exchange nothing (each reference rank is its own chain), so a
    chain's cells run alone give what they give beside the other chains."""
    from concurrent.futures import ThreadPoolExecutor
    kw = {k: v for k, v in inp.items() if k not in ("state0", "params", "forcing")}
    sels = [np.flatnonzero(chains == r) for r in np.unique(chains)]

    def one(sel):
        return port.run_cell_order(chains=chains[sel], params={k: v[sel] for k, v in inp["params"].items()},
                                   forcing=np.ascontiguousarray(inp["forcing"][:, :, sel]), **kw)
    with ThreadPoolExecutor(len(sels)) as ex:
        parts = list(ex.map(one, sels))
    n, L = chains.size, inp["params"]["theta_s"].shape[1]
    ann = np.full((inp["nyears"], 12 + L, n), np.nan, np.float32)
    st = {k: np.zeros((n,) + v.shape[1:], v.dtype) for k, v in parts[0]["state"].items()}
    for sel, r in zip(sels, parts):
        ann[:, :, sel] = r["annual"]
        for k, v in r["state"].items():
            st[k][sel] = v
    return dict(annual=ann, state=st, rc=max(r["rc"] for r in parts))


@pytest.mark.parametrize("split", ["halves", "alternating"])
def test_cell_order_two_chains_match_oracle_geo(split):
    """Two chains against the oracle's restatement of the order (pinned to the
    reference at these layers by co_geo_a on one chain).  Cut into halves, the
    cells end with the one-chain bits (the oracle, on the CPU); alternating
    chains hand every cell another predecessor and move the second decade."""
    meta, inp, exp = load_golden("co_geo_a")
    _name_of(inp)
    chains = np.array([0] * 20 + [1] * 20) if split == "halves" else np.arange(40) % 2
    ref = _oracle_chains(inp, chains)
    assert ref["rc"] == 0
    assert same_bits(ref["annual"], exp["annual"]) == (split == "halves")
    for pipelined in (True, False):
        out = h.run_cell_order(pipelined=pipelined, chains=chains, **inp)
        assert out["rc"] == 0, out["err"]
        assert same_bits(out["annual"], ref["annual"])
        assert same_bits(out["state"], refcase.pack_state(ref["state"], meta["L"]))


# ---- 7. the daily focus window -------------------------------------------------------
def test_daily_focus_geo():
    meta, inp, exp = load_geo_golden("geo_a_ns36")
    inp = first_cells(inp, meta["ncell"])
    sel = [0, 5, 31]
    _name_of(inp)
    host = host_focus(const_geo=0, **inp)
    d8, ref = port_daily8(cells=sel, **inp)
    out = h.run(daily_cells=sel, **inp)
    assert out["rc"] == host["rc"] == ref["rc"] == 0
    assert out["daily"].shape == (365, 11, 3)
    assert same_bits(out["daily"], host["daily"][:, :, sel])
    assert same_bits(out["daily"][:, IDX], d8)
    assert same_bits(out["annual"], exp["annual"][:1])


# ---- 8. the site path ------------------------------------------------------------------
def test_site_path_geo():
    from tests.test_site import _gpu_site
    gid = synth.land_cells()[4321::7000][:4]
    p, sub, daily, lai = site_inputs(gid, 8, 36, (2004,), LCLIM_EVENTS_2004)
    inp = dict(zi=ZI_GEO_A, params=p, sub=sub, daily=daily, lai=lai, nisurf=36)
    _geo_name(4, ZI_GEO_A, 36, False)
    ref = port.site(**inp, nthreads=NTHREADS)
    assert ref["rc"] == 0 and not np.isnan(ref["daily"]).any()
    diag, st = _gpu_site(inp)
    assert same_bits(diag, ref["daily"])
    assert same_bits(st, refcase.pack_state(ref["state"], 8))


# ---- 9. NaN-parameter cells --------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["pair", "pair1", "solo"])
def test_nan_parameter_cells_match_oracle_geo(kernel, monkeypatch):
    """Cells with missing soil data run the year with NaN state, so every
    deferred special-case check and every redo path runs under GeoR, in the
    same waves as normal cells."""
    monkeypatch.setenv("H9G_KERNEL", kernel)
    meta, inp, _ = load_geo_golden("geo_a_ns36")
    inp = first_cells(inp, meta["ncell"])
    p = {k: v.copy() for k, v in inp["params"].items()}
    p["fmax"][::7] = np.nan
    p["psi_s"][3::11, 2] = np.nan
    p["hksat"][5::13, 0] = np.nan
    p["bsw"][8::17, 6] = np.nan
    kw = dict(inp, params=p)
    _name_of(kw)
    ref = _once("nan_ref", lambda: port.run(**{k: v for k, v in kw.items() if k != "state0"}, nthreads=NTHREADS))
    gpu = h.run(stop_on_error=False, **kw)
    assert np.isnan(ref["annual"][0]).any(axis=0).sum() > 5
    assert np.array_equal(gpu["errors"]["code"], ref["errors"]["code"])
    assert same_bits(gpu["annual"], ref["annual"])
    assert same_bits(gpu["state"], refcase.pack_state(ref["state"], meta["L"]))
