"""The water-table chain on the second wave of the one-column kernel's two-wave
shape (H9G_P1_SIDE; h9g_pair.h hydrology_pair ROLE_MAINS / ROLE_CHAIN,
front_year_pair) against the 22-column pair kernel, bit for bit
(conftest.same_bits: no tolerance anywhere).

In a substep that starts with the water table in the column (jwt < L) the
second wave evaluates recharge, the water table, baseflow and drainage beside
the main wave's tridiagonal sweep and hands zwt, wa, rsub_top, jwt, the
re-run flag, STOP 3 and the h2osoi_liq additions over behind a third barrier;
a substep that starts below the column (jwt == L) keeps the main wave's own
chain.  With H9G_KERNEL=pair1 a context of at most 512 cells runs every year
on that shape.

  - lists of 1, 2, 3 and 5 cells, 1903-1904 (1904 has 366 days), L = 8 at
    NISURF = 48 and L = 10 at NISURF = 24, GROW on and off, against the same
    cells inside one 200-cell run of the pair kernel: every annual mean, the end
    state, the STOP records;
  - the `edge` golden's 16 cells, its year twice (1901, then 1902 on the same
    forcing), against the pair kernel: water table at the surface, inside
    layers 3 and 8 and at an interface, near the 80 m clamp, a saturated column,
    the aquifer near its 5,000 mm cap.  Counted with the C oracle (oracle.port,
    test_the_edge_cells_hold_every_kind_of_substep, a CPU test) over the 16
    cells and those two years: 270,020 wave-substeps start with jwt < L (the
    second wave's chain), 290,620 with jwt == L (the main wave's), 6,012 change
    from one kind to the other, and 1,129 end in another layer of the column
    than they started in, which takes a second layer visit.  No kind is
    missing, so no hand-built cell is added;
  - a mid-year STOP: stop_ns24's STOP cell and its neighbour, in both orders,
    then a second year in which the STOP cell returns early beside a non-land
    cell: both waves of the STOP cell's workgroup leave, the neighbour's finish;
  - the monthly sibling: three cells with monthly recording on, against the pair
    kernel's month-end snapshots;
  - the launch record: after its years every one-column context of this file
    must name h9g_pair1f_kernel, the two-wave kernel, whatever the library was
    built with.  A build without the chain on the second wave (H9G_P1_SIDE=0)
    is round 9's kernel under the same name and passes this file with the same
    bits; a build without the two-wave shape (H9G_P1_FRONT=0) fails it.  The
    name cannot tell the second wave's chain from round 9's kernel: that the
    product holds it is in the code-object and timing records.
The GPU tests run on an MI355X only."""
import numpy as np
import pytest

import hybrid9_amd as h
from hybrid9_amd import synth
from oracle import port, refcase
from tests.conftest import load_golden, same_bits

gpu = pytest.mark.gpu

LISTS = ((3, 1), (40, 2), (0, 3), (120, 5))        # (first cell, cells) within the 200
YEARS = (1903, 1904)
_full = {}


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


TWO_WAVE = "h9g_pair1f_kernel<"     # the launch record of every list in this file (at most 512 cells)


def _same_errors(a, b, sel=slice(None)):
    return all(same_bits(np.asarray(a[k]), np.asarray(b[k])[sel]) for k in ("code", "day", "substep", "value"))


@gpu
@pytest.mark.parametrize("grow", [True, False], ids=["grow", "nogrow"])
@pytest.mark.parametrize("L,nisurf", [(8, 48), (10, 24)])
def test_lists_match_the_pair_kernel(L, nisurf, grow, monkeypatch):
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
        assert name.startswith(TWO_WAVE), name          # the launch record
        assert same_bits(ann, ann_all[:, :, lo:lo + n]), (lo, n)
        assert _same_errors(err, err_all, slice(lo, lo + n)), (lo, n)
        part = refcase.unpack_state(st, n, L)
        for k in part:
            assert same_bits(part[k], full[k][lo:lo + n]), (lo, n, k)


def _two_years(inp, cells, params=None):
    """The golden's cells `cells`, its year twice (1901, then 1902 on the same
    forcing), from the golden's start state where it has one: annual means of
    both years, end state, STOP records, kernel name."""
    p = inp["params"] if params is None else params
    n_all = p["fmax"].size
    p = {k: np.ascontiguousarray(v[cells]) for k, v in p.items()}
    f = np.ascontiguousarray(inp["forcing"][:, :, cells])
    L = p["theta_s"].shape[1]
    anns = []
    with h.Context(len(cells), inp["zi"], nisurf=inp["nisurf"], grow_on=bool(inp["grow_on"])) as ctx:
        ctx.set_params(p)
        ctx.init_state()
        if inp.get("state0") is not None:
            s0 = refcase.unpack_state(inp["state0"], n_all, L)
            ctx.set_state(refcase.pack_state({k: np.asarray(v)[cells] for k, v in s0.items()}, L))
        ctx.push_forcing(0, f)
        for y in (1901, 1902):
            ctx.run_year(0, y)
            ctx.sync(raise_on_stop=False)
            anns.append(ctx.get_annual())
        return np.stack(anns), ctx.get_state(), ctx.get_errors(), ctx.kernel_name()


def _jwt(zwt, zi, L):
    """HYDROLOGY.f90:499-508 for float32 zwt: the layers whose bottom lies above the water table."""
    zim = np.asarray(zi[1:L + 1], np.float32) / np.float32(1000.0)
    return (np.asarray(zwt, np.float32)[..., None] > zim).sum(-1)


def test_the_edge_cells_hold_every_kind_of_substep():
    """CPU, the C oracle: the edge golden's 16 cells over the two years of the
    GPU test below hold substeps of every kind the hand-over distinguishes."""
    meta, inp, _ = load_golden("edge")
    L, n, ns = meta["L"], meta["ncell"], inp["nisurf"]
    s0 = refcase.unpack_state(inp["state0"], n, L)
    inside = below = change = cross = 0
    for y in (1901, 1902):
        r = port.run(zi=inp["zi"], params=inp["params"], forcing=inp["forcing"], nisurf=ns, year0=y, nyears=1,
                     grow_on=inp["grow_on"], state0=s0, trace_cells=tuple(range(n)), nthreads=8)
        assert r["rc"] == 0
        zend = r["trace"][:, :, 3 * L]                              # zwt after each substep
        zstart = np.concatenate([np.asarray(s0["zwt"], np.float32).reshape(n, 1), zend[:, :-1]], axis=1)
        j0, j1 = _jwt(zstart, inp["zi"], L), _jwt(zend, inp["zi"], L)
        inside += int((j0 < L).sum())
        below += int((j0 == L).sum())
        change += int(((j0 < L) != (j1 < L)).sum())
        cross += int(((j0 < L) & (j1 < L) & (j0 != j1)).sum())      # another layer of the column: a second visit
        s0 = r["state"]
    print(f"jwt < L: {inside}, jwt == L: {below}, changes: {change}, second layer visits: {cross}")
    assert (inside, below, change, cross) == (270020, 290620, 6012, 1129)


@gpu
def test_the_edge_cells_two_years(monkeypatch):
    meta, inp, exp = load_golden("edge")
    n, L = meta["ncell"], meta["L"]
    monkeypatch.setenv("H9G_KERNEL", "pair")
    ann_all, st_all, err_all, name_all = _two_years(inp, list(range(n)))
    assert "pair1" not in name_all, name_all
    assert same_bits(ann_all[:1], exp["annual"])                 # the golden's year
    assert not err_all["code"].any()
    monkeypatch.setenv("H9G_KERNEL", "pair1")
    ann, st, err, name = _two_years(inp, list(range(n)))
    assert name.startswith(TWO_WAVE), name
    assert same_bits(ann, ann_all)
    assert _same_errors(err, err_all)
    full, part = refcase.unpack_state(st_all, n, L), refcase.unpack_state(st, n, L)
    for k in part:
        assert same_bits(part[k], full[k]), k


@gpu
def test_a_mid_year_stop_and_the_early_returns(monkeypatch):
    meta, inp, _ = load_golden("stop_ns24")
    s, n, L = meta["stop"], meta["ncell"], meta["L"]
    c = s["cell"]
    p = {k: np.array(v, copy=True) for k, v in inp["params"].items()}
    p["theta_s"][2] = np.nan                                   # a non-land cell
    monkeypatch.setenv("H9G_KERNEL", "pair")
    ann_all, st_all, err_all, name_all = _two_years(inp, list(range(n)), p)
    assert "pair1" not in name_all
    assert (err_all["code"][c], err_all["day"][c]) == (s["code"], s["day"])
    assert f"{err_all['value'][c]:.9g}" == f"{s['value']:.9g}"
    assert np.array_equal(np.nonzero(err_all["code"])[0], [c])
    full = refcase.unpack_state(st_all, n, L)
    monkeypatch.setenv("H9G_KERNEL", "pair1")
    nb = c - 1
    for cells in ([c, nb], [nb, c], [2, c, nb, 0]):
        ann, st, err, name = _two_years(inp, cells, p)
        assert name.startswith(TWO_WAVE), name
        k = cells.index(c)
        assert (err["code"][k], err["day"][k], err["substep"][k]) == (s["code"], s["day"], err_all["substep"][c]), cells
        assert f"{err['value'][k]:.9g}" == f"{s['value']:.9g}", cells
        assert _same_errors(err, err_all, cells), cells
        assert same_bits(ann, ann_all[:, :, cells]), cells          # NaN for the STOP cell and the non-land cell
        assert not np.isnan(ann[:, :, cells.index(nb)]).any(), cells   # the neighbour's years completed
        part = refcase.unpack_state(st, len(cells), L)
        for f in part:
            assert same_bits(part[f], full[f][cells]), (cells, f)


@gpu
def test_the_monthly_sibling(monkeypatch):
    monkeypatch.setenv("H9G_KERNEL", "pair")
    gid = synth.land_cells()[::331][:24]
    mon_all = []
    ann_all, st_all, err_all, _ = _synth_run(gid, 8, 48, True, (1904,), mon_all)
    monkeypatch.setenv("H9G_KERNEL", "pair1")
    mon = []
    ann, st, err, name = _synth_run(gid[5:8], 8, 48, True, (1904,), mon)
    assert name.startswith(TWO_WAVE), name
    assert not np.isnan(mon[0]).any()
    assert same_bits(mon[0], mon_all[0][:, :, 5:8])
    assert same_bits(ann, ann_all[:, :, 5:8])
    assert _same_errors(err, err_all, slice(5, 8))
    full, part = refcase.unpack_state(st_all, gid.size, 8), refcase.unpack_state(st, 3, 8)
    for k in part:
        assert same_bits(part[k], full[k][5:8]), k
