"""The one-column kernel's task rounds (hydrology_pair `kTask`, h9g_pair.h)
against the 22-column pair kernel, bit for bit.

h9g_pair1_kernel runs lists of 1, 3 and 5 cells (one wave per cell: a ragged
workgroup, and with 5 cells a full four-wave workgroup plus a one-wave one)
over two years with GROW on; every annual mean and the end state must equal
those of the same cells inside one 200-cell run of the pair kernel, which the
goldens of test_gpu_parity.py pin to the reference.  No tolerance is involved
(conftest.same_bits).  Runs on an MI355X only."""
import numpy as np
import pytest

import hybrid9_amd as h
from hybrid9_amd import synth
from oracle import refcase
from tests.conftest import same_bits

pytestmark = pytest.mark.gpu

LISTS = ((0, 1), (17, 3), (120, 5))        # (first cell, cells) within the 200
_full = {}


def _run(gid, L, nisurf):
    lat = synth.cell_lat(gid, synth.NX05, synth.NY05)
    zi = synth.ZI_L8 if L == 8 else synth.ZI_L10
    anns = []
    with h.Context(gid.size, zi, nlayers=L, nisurf=nisurf, grow_on=True) as ctx:
        ctx.set_cells(gid, lat)
        ctx.synth_params(synth.SEED)
        ctx.init_state()
        for y in range(2):
            nt = synth.days_in_year(1901 + y)
            ctx.synth_forcing(y % 2, synth.SEED, synth.year_day0(1901 + y), nt)
            ctx.run_year(y % 2, 1901 + y)
            ctx.sync(raise_on_stop=False)
            anns.append(ctx.get_annual())
        return np.stack(anns), ctx.get_state(), ctx.get_errors(), ctx.kernel_name()


def _pair_run(L, nisurf, monkeypatch):
    """The 200-cell reference run of the 22-column kernel, once per shape."""
    if (L, nisurf) not in _full:
        monkeypatch.setenv("H9G_KERNEL", "pair")
        gid = synth.land_cells()[::331][:200]
        _full[(L, nisurf)] = (gid,) + _run(gid, L, nisurf)
    return _full[(L, nisurf)]


@pytest.mark.parametrize("L,nisurf", [(8, 48), (10, 24)])
def test_one_column_lists_match_the_pair_kernel(L, nisurf, monkeypatch):
    gid, ann_all, st_all, err_all, _ = _pair_run(L, nisurf, monkeypatch)
    assert gid.size == 200
    full = refcase.unpack_state(st_all, gid.size, L)
    monkeypatch.setenv("H9G_KERNEL", "pair1")
    for lo, n in LISTS:
        assert not err_all["code"][lo:lo + n].any(), (lo, n)      # no compared cell STOPped
        ann, st, err, name = _run(gid[lo:lo + n], L, nisurf)
        assert "pair1" in name, name
        assert not err["code"].any(), (lo, n)
        assert same_bits(ann, ann_all[:, :, lo:lo + n]), (lo, n)
        part = refcase.unpack_state(st, n, L)
        for k in part:
            assert same_bits(part[k], full[k][lo:lo + n]), (lo, n, k)
