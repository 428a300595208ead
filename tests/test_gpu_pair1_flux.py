"""The one-column kernel's round C (the tridiagonal system's interface fluxes
on the task lanes, hydrology_pair `kTask`, h9g_pair.h) and its shorter
quotient chains, against the 22-column pair kernel, bit for bit.

h9g_pair1_kernel runs lists of 1, 3 and 5 cells (one wave, a ragged
workgroup, a full four-wave workgroup plus one wave) over two years, with
GROW on and off, at (L = 8, NISURF = 48) and (L = 10, NISURF = 24); every
annual mean of each year and the end state must equal those of the same cells
inside one 200-cell run of the pair kernel (conftest.same_bits: no tolerance).

Rows L and L+1 of the system have two shapes, with the water table inside the
column or below it (the aquifer interface).  The cells were chosen on the
host, by running the 200 strided cells of synth.land_cells()[::331] through
oracle.port.run and reading zwt at each year's end against zi(L), the same
in all four cases:
    list (3, 1)    cell 3: below the column in both years (the aquifer rows)
    list (0, 3)    cells 0 and 2 inside the column; cell 1 starts below it and
                   rises into it (L = 8, GROW on: 5.38 m, then 2.2959 m
                   against zi(L) = 2.296 m), so both shapes within one run
    list (120, 5)  cells 120 and 123 inside, 121, 122 and 124 below
The test asserts, from the pair kernel's own year-end states, that the
compared cells hold both kinds and that none of them STOPped.  Runs on an
MI355X only."""
import numpy as np
import pytest

import hybrid9_amd as h
from hybrid9_amd import synth
from oracle import refcase
from tests.conftest import same_bits

pytestmark = pytest.mark.gpu

LISTS = ((3, 1), (0, 3), (120, 5))         # (first cell, cells) within the 200
_full = {}


def _run(gid, L, nisurf, grow):
    """Two years, a launch each: the annual means, the year-end states, the
    STOP records and the kernel's name."""
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
        return np.stack(anns), sts, ctx.get_errors(), ctx.kernel_name()


def _pair_run(L, nisurf, grow, monkeypatch):
    """The 200-cell reference run of the 22-column kernel, once per case."""
    key = (L, nisurf, grow)
    if key not in _full:
        monkeypatch.setenv("H9G_KERNEL", "pair")
        gid = synth.land_cells()[::331][:200]
        _full[key] = (gid,) + _run(gid, L, nisurf, grow)
    return _full[key]


@pytest.mark.parametrize("grow", [True, False], ids=["grow", "nogrow"])
@pytest.mark.parametrize("L,nisurf", [(8, 48), (10, 24)])
def test_one_column_fluxes_match_the_pair_kernel(L, nisurf, grow, monkeypatch):
    gid, ann_all, sts_all, err_all, name_all = _pair_run(L, nisurf, grow, monkeypatch)
    assert gid.size == 200 and "pair1" not in name_all, name_all
    zi = synth.ZI_L8 if L == 8 else synth.ZI_L10
    ends = [refcase.unpack_state(s, gid.size, L) for s in sts_all]
    full = ends[-1]
    # both shapes of rows L, L+1 among the compared cells, by the pair kernel's own states
    cells = np.concatenate([np.arange(lo, lo + n) for lo, n in LISTS])
    zwt_mm = np.stack([e["zwt"][cells] * np.float32(1000.0) for e in ends])
    print(f"L={L} grow={grow}: zwt (mm) at the year ends of cells {cells.tolist()}: {zwt_mm.tolist()}; zi(L) = {zi[L]}")
    assert (zwt_mm < zi[L]).any(), "no compared cell has its water table inside the column"
    assert (zwt_mm >= zi[L]).any(), "no compared cell has its water table below the column"
    assert not err_all["code"][cells].any()                        # no compared cell STOPped
    monkeypatch.setenv("H9G_KERNEL", "pair1")
    for lo, n in LISTS:
        ann, sts, err, name = _run(gid[lo:lo + n], L, nisurf, grow)
        assert "pair1" in name, name
        assert not err["code"].any(), (lo, n)
        assert same_bits(ann, ann_all[:, :, lo:lo + n]), (lo, n)
        part = refcase.unpack_state(sts[-1], n, L)
        for k in part:
            assert same_bits(part[k], full[k][lo:lo + n]), (lo, n, k)
