"""The pair kernels' split flux phase (the tridiagonal system's interface
fluxes, half of them on each lane of a pair: hydrology_pair `kFluxSplit`,
h9g_pair.h) against the solo kernel, bit for bit.

The solo kernel runs one lane per column and evaluates every interface on it,
from a text the split does not touch.  The 200 strided cells
synth.land_cells()[::331][:200] run two years, a launch each, with GROW on
and off, at (L = 8, NISURF = 48) and (L = 10, NISURF = 24), on the 22-column
kernel (`pair`), the 11-column kernel (`pair11`) and, at L = 10, the
two-wave-per-SIMD kernel (`pair2`); every annual mean of both years and the end
state must equal the solo kernel's (conftest.same_bits: no tolerance).

The smallest shapes at which the split can go wrong run as lists of the same
cells and are compared with the 200-cell run:
    (3, 1)     one cell: a wave with one pair (below the column: the aquifer
               interface on its odd lane)
    (0, 23)    a full 22-column wave plus a one-pair wave
    (100, 89)  a full four-wave workgroup plus one
Rows L and L+1 of the system have two shapes, with the water table inside the
column or below it.  tests/test_gpu_pair1_flux.py records which of these cells
are which (0 and 2 inside, 1 rising into it, 3 below; 120 and 123 inside, 121,
122 and 124 below): the lists of 23 and 89 cells hold both, in one wave, so
`any_aq` is set while some pairs are not `aq`.  The test asserts that from the
kernel's own year-end zwt against zi(L), and that no compared cell STOPped.
Runs on an MI355X only."""
import numpy as np
import pytest

import hybrid9_amd as h
from hybrid9_amd import synth
from oracle import refcase
from tests.conftest import same_bits

pytestmark = pytest.mark.gpu

LISTS = ((3, 1), (0, 23), (100, 89))       # (first cell, cells) within the 200
KIND = {"pair": 1, "solo": 2, "pair2": 4, "pair11": 5}
_solo = {}


def _run(gid, L, nisurf, grow):
    """Two years, a launch each: the annual means, the year-end states, the
    STOP records and the kernel kind."""
    lat = synth.cell_lat(gid, synth.NX05, synth.NY05)
    zi = synth.ZI_L8 if L == 8 else synth.ZI_L10
    anns, sts = [], []
    with h.Context(gid.size, zi, nlayers=L, nisurf=nisurf, grow_on=grow) as ctx:
        ctx.set_cells(gid, lat)
        ctx.synth_params(synth.SEED)
        ctx.init_state()
        for y in range(2):
            nt = synth.days_in_year(1901 + y)
            ctx.synth_forcing(y % 2, synth.SEED, synth.year_day0(1901 + y), nt)
            ctx.run_year(y % 2, 1901 + y)
            ctx.sync(raise_on_stop=False)
            anns.append(ctx.get_annual())
            sts.append(np.array(ctx.get_state(), copy=True))
        return np.stack(anns), sts, ctx.get_errors(), ctx.kind_id()


def _solo_run(L, nisurf, grow, monkeypatch):
    """The 200-cell run of the solo kernel, once per case."""
    key = (L, nisurf, grow)
    if key not in _solo:
        monkeypatch.setenv("H9G_KERNEL", "solo")
        gid = synth.land_cells()[::331][:200]
        _solo[key] = (gid,) + _run(gid, L, nisurf, grow)
    return _solo[key]


def _inside(sts, n, L, cells, zi):
    """Per year end and compared cell: is the water table inside the column?"""
    zwt_mm = np.stack([refcase.unpack_state(s, n, L)["zwt"][cells] * np.float32(1000.0) for s in sts])
    return zwt_mm < zi[L], zwt_mm


CASES = [(8, 48, "pair"), (8, 48, "pair11"), (10, 24, "pair"), (10, 24, "pair11"), (10, 24, "pair2")]


@pytest.mark.parametrize("grow", [True, False], ids=["grow", "nogrow"])
@pytest.mark.parametrize("L,nisurf,kernel", CASES)
def test_split_fluxes_match_the_solo_kernel(L, nisurf, kernel, grow, monkeypatch):
    gid, ann_solo, sts_solo, err_solo, kind_solo = _solo_run(L, nisurf, grow, monkeypatch)
    assert gid.size == 200 and kind_solo == KIND["solo"], kind_solo
    zi = synth.ZI_L8 if L == 8 else synth.ZI_L10
    monkeypatch.setenv("H9G_KERNEL", kernel)
    ann, sts, err, kind = _run(gid, L, nisurf, grow)
    assert kind == KIND[kernel], (kernel, kind)
    # both shapes of rows L, L+1, by this kernel's own states: among all compared cells, and
    # within the one-wave-plus and the one-workgroup-plus lists (mixed waves)
    for lo, n in ((0, 200),) + LISTS[1:]:
        cells = np.arange(lo, lo + n)
        inside, zwt_mm = _inside(sts, 200, L, cells, zi)
        print(f"L={L} {kernel} grow={grow}: cells [{lo}, {lo + n}): {int(inside[-1].sum())} inside the column, "
              f"{int((~inside[-1]).sum())} below it at the end; zi(L) = {zi[L]}")
        assert inside.any(), f"no cell of [{lo}, {lo + n}) has its water table inside the column"
        assert (~inside).any(), f"no cell of [{lo}, {lo + n}) has its water table below the column"
    assert not err["code"].any() and not err_solo["code"].any()   # no compared cell STOPped
    assert same_bits(ann, ann_solo)
    full_solo = refcase.unpack_state(sts_solo[-1], 200, L)
    full = refcase.unpack_state(sts[-1], 200, L)
    for k in full:
        assert same_bits(full[k], full_solo[k]), k
    for lo, n in LISTS:
        ann_l, sts_l, err_l, kind_l = _run(gid[lo:lo + n], L, nisurf, grow)
        assert kind_l == KIND[kernel], (lo, n, kind_l)
        assert not err_l["code"].any(), (lo, n)
        assert same_bits(ann_l, ann[:, :, lo:lo + n]), (lo, n)
        part = refcase.unpack_state(sts_l[-1], n, L)
        for k in part:
            assert same_bits(part[k], full[k][lo:lo + n]), (lo, n, k)
