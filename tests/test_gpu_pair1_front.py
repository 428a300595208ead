"""The one-column kernel's two waves per column (h9g_pair1f_kernel; h9g_pair.h
front_year_pair) against the 22-column pair kernel and the goldens, bit for bit
(conftest.same_bits: no tolerance anywhere).

Lists of at most 512 cells run a workgroup per cell: the main wave without the
front of the substep, the front wave beside it, two workgroup barriers per
substep.  With H9G_KERNEL=pair1 a context of n cells runs every year as such a
launch (n <= 512) or on the single-wave kernel (n > 512).

  - lists of 1, 2, 3 and 5 cells, 1903-1904 (1904 has 366 days), L = 8 at
    NISURF = 48 and L = 10 at NISURF = 24, GROW on and off, against the same
    cells inside one 200-cell run of the pair kernel: every annual mean, the end
    state, the STOP records;
  - a mid-year STOP: stop_ns24's STOP cell and its neighbour, in both orders --
    both waves of the STOP cell's workgroup leave, the neighbour's finish -- and
    a second year on top, in which the STOP cell returns early (its record is
    set) beside a non-land (NaN theta_s) cell and ordinary ones;
  - the exact re-run from the day snapshot: the `edge` golden's 16 cells;
  - the boundary: 512 cells take the two-wave shape, 513 the single-wave kernel,
    and both match the pair kernel.  The shape is read from the launch record: a
    one-column context's kernel_name() is, once a year has run, the kernel that
    launch was dispatched to (run_year_impl).  Before any year it says what the
    library was built with: a build without the two-wave shape (H9G_P1_FRONT=0)
    names the single-wave kernel for a context of few cells, and then the
    512-cell list must have run on that kernel, with the same bits;
  - the monthly sibling: three cells with monthly recording on, dispatched to
    the two-wave monthly kernel, month-end snapshots against the pair kernel's.
Runs on an MI355X only."""
import numpy as np
import pytest

import hybrid9_amd as h
from hybrid9_amd import synth
from oracle import refcase
from tests.conftest import load_golden, same_bits

pytestmark = pytest.mark.gpu

LISTS = ((3, 1), (40, 2), (0, 3), (120, 5))        # (first cell, cells) within the 200
YEARS = (1903, 1904)
_full = {}
_big = {}


def _synth_run(gid, L, nisurf, grow, years, monthly=None):
    """monthly: a list that receives the month-end snapshots of each year."""
    lat = synth.cell_lat(gid, synth.NX05, synth.NY05)
    zi = synth.ZI_L8 if L == 8 else synth.ZI_L10
    anns = []
    with h.Context(gid.size, zi, nlayers=L, nisurf=nisurf, grow_on=grow) as ctx:
        ctx.set_cells(gid, lat)
        ctx.synth_params(synth.SEED)
        ctx.init_state()
        if monthly is not None:
            ctx.set_monthly(True)
        for k, y in enumerate(years):
            ctx.synth_forcing(k % 2, synth.SEED, synth.year_day0(y), synth.days_in_year(y))
            ctx.run_year(k % 2, y)
            ctx.sync(raise_on_stop=False)
            anns.append(ctx.get_annual())
            if monthly is not None:
                monthly.append(ctx.get_monthly())
        return np.stack(anns), ctx.get_state(), ctx.get_errors(), ctx.kernel_name()


def _built_with_front(monkeypatch):
    """What the library says it was built with: before any year has run, a
    one-column context of few cells names the two-wave kernel, or, in a build
    without it, the single-wave one."""
    monkeypatch.setenv("H9G_KERNEL", "pair1")
    with h.Context(1, synth.ZI_L8, nlayers=8, nisurf=48, grow_on=False) as ctx:
        name = ctx.kernel_name()
    assert name.startswith(("h9g_pair1f_kernel<", "h9g_pair1_kernel<")), name
    return name.startswith("h9g_pair1f_kernel<")


def _same_errors(a, b, sel=slice(None)):
    return all(same_bits(np.asarray(a[k]), np.asarray(b[k])[sel]) for k in ("code", "day", "substep", "value"))


@pytest.mark.parametrize("grow", [True, False], ids=["grow", "nogrow"])
@pytest.mark.parametrize("L,nisurf", [(8, 48), (10, 24)])
def test_two_wave_lists_match_the_pair_kernel(L, nisurf, grow, monkeypatch):
    key = (L, nisurf, grow)
    if key not in _full:
        monkeypatch.setenv("H9G_KERNEL", "pair")
        gid = synth.land_cells()[::331][:200]
        _full[key] = (gid,) + _synth_run(gid, L, nisurf, grow, YEARS)
    gid, ann_all, st_all, err_all, name_all = _full[key]
    assert "pair1" not in name_all, name_all
    assert synth.days_in_year(YEARS[1]) == 366
    full = refcase.unpack_state(st_all, gid.size, L)
    monkeypatch.setenv("H9G_KERNEL", "pair1")
    for lo, n in LISTS:
        ann, st, err, name = _synth_run(gid[lo:lo + n], L, nisurf, grow, YEARS)
        assert "pair1" in name, name                # (the boundary test below pins the shape)
        assert same_bits(ann, ann_all[:, :, lo:lo + n]), (lo, n)
        assert _same_errors(err, err_all, slice(lo, lo + n)), (lo, n)
        part = refcase.unpack_state(st, n, L)
        for k in part:
            assert same_bits(part[k], full[k][lo:lo + n]), (lo, n, k)


def _two_years(inp, cells, params=None):
    """The golden's cells `cells`, its year twice (1901, then 1902 on the same
    forcing): annual means of both years, end state, STOP records, kernel name."""
    p = inp["params"] if params is None else params
    p = {k: np.ascontiguousarray(v[cells]) for k, v in p.items()}
    f = np.ascontiguousarray(inp["forcing"][:, :, cells])
    anns = []
    with h.Context(len(cells), inp["zi"], nisurf=inp["nisurf"], grow_on=bool(inp["grow_on"])) as ctx:
        ctx.set_params(p)
        ctx.init_state()
        ctx.push_forcing(0, f)
        for y in (1901, 1902):
            ctx.run_year(0, y)
            ctx.sync(raise_on_stop=False)
            anns.append(ctx.get_annual())
        return np.stack(anns), ctx.get_state(), ctx.get_errors(), ctx.kernel_name()


def test_a_mid_year_stop_and_the_early_returns(monkeypatch):
    meta, inp, _ = load_golden("stop_ns24")
    s, n, L = meta["stop"], meta["ncell"], meta["L"]
    c = s["cell"]
    p = {k: np.array(v, copy=True) for k, v in inp["params"].items()}
    p["theta_s"][2] = np.nan                                   # a non-land cell
    monkeypatch.setenv("H9G_KERNEL", "pair")
    ann_all, st_all, err_all, name_all = _two_years(inp, list(range(n)), p)
    assert "pair1" not in name_all
    # the pair kernel's record of the STOP cell is the golden's; its substep is the yardstick's
    assert (err_all["code"][c], err_all["day"][c]) == (s["code"], s["day"])
    assert f"{err_all['value'][c]:.9g}" == f"{s['value']:.9g}"
    assert np.array_equal(np.nonzero(err_all["code"])[0], [c])
    full = refcase.unpack_state(st_all, n, L)
    monkeypatch.setenv("H9G_KERNEL", "pair1")
    nb = c - 1
    for cells in ([c, nb], [nb, c], [2, c, nb, 0], [0, nb, c, 2, 1]):
        ann, st, err, name = _two_years(inp, cells, p)
        assert "pair1" in name, name                # (the boundary test below pins the shape)
        k = cells.index(c)
        assert (err["code"][k], err["day"][k], err["substep"][k]) == (s["code"], s["day"], err_all["substep"][c]), cells
        assert f"{err['value'][k]:.9g}" == f"{s['value']:.9g}", cells
        assert _same_errors(err, err_all, cells), cells
        assert same_bits(ann, ann_all[:, :, cells]), cells          # NaN for the STOP cell and the non-land cell
        assert not np.isnan(ann[:, :, cells.index(nb)]).any(), cells   # the neighbour's years completed
        part = refcase.unpack_state(st, len(cells), L)
        for f in part:
            assert same_bits(part[f], full[f][cells]), (cells, f)


def test_the_exact_rerun_matches_the_edge_golden(monkeypatch):
    monkeypatch.setenv("H9G_KERNEL", "pair1")
    meta, inp, exp = load_golden("edge")
    out = h.run(zi=inp["zi"], params=inp["params"], forcing=inp["forcing"], nisurf=inp["nisurf"],
                year0=inp["year0"], nyears=inp["nyears"], grow_on=bool(inp["grow_on"]), state0=inp["state0"])
    assert out["rc"] == 0, out["err"]
    assert same_bits(out["annual"], exp["annual"])
    assert same_bits(out["state"], exp["state"])


@pytest.mark.parametrize("n", [512, 513])
def test_the_boundary_between_the_two_shapes(n, monkeypatch):
    front = _built_with_front(monkeypatch)
    if not _big:
        monkeypatch.setenv("H9G_KERNEL", "pair")
        gid = synth.land_cells()[::131][:513]
        _big["run"] = (gid,) + _synth_run(gid, 8, 48, False, (1901,))
    gid, ann_all, st_all, err_all, _ = _big["run"]
    assert gid.size == 513
    monkeypatch.setenv("H9G_KERNEL", "pair1")
    ann, st, err, name = _synth_run(gid[:n], 8, 48, False, (1901,))
    # the kernel the year was dispatched to
    want = "h9g_pair1f_kernel<" if front and n <= 512 else "h9g_pair1_kernel<"
    print(f"built with the two-wave shape: {front}; {n} cells ran on {name}")
    assert name.startswith(want), (name, want)
    assert same_bits(ann, ann_all[:, :, :n])
    assert _same_errors(err, err_all, slice(0, n))
    full, part = refcase.unpack_state(st_all, gid.size, 8), refcase.unpack_state(st, n, 8)
    for k in part:
        assert same_bits(part[k], full[k][:n]), k


def test_the_monthly_sibling_takes_the_same_shape(monkeypatch):
    front = _built_with_front(monkeypatch)
    monkeypatch.setenv("H9G_KERNEL", "pair")
    gid = synth.land_cells()[::331][:24]
    mon_all = []
    ann_all, st_all, err_all, _ = _synth_run(gid, 8, 48, True, (1904,), mon_all)
    monkeypatch.setenv("H9G_KERNEL", "pair1")
    mon = []
    ann, st, err, name = _synth_run(gid[5:8], 8, 48, True, (1904,), mon)
    assert name.startswith("h9g_pair1f_kernel<" if front else "h9g_pair1_kernel<"), name
    assert not np.isnan(mon[0]).any()
    assert same_bits(mon[0], mon_all[0][:, :, 5:8])
    assert same_bits(ann, ann_all[:, :, 5:8])
    assert _same_errors(err, err_all, slice(5, 8))
    full, part = refcase.unpack_state(st_all, gid.size, 8), refcase.unpack_state(st, 3, 8)
    for k in part:
        assert same_bits(part[k], full[k][5:8]), k
