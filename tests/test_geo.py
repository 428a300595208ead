"""Runtime layer geometry without a GPU.  The goldens of kind `geo`
(tests/golden/make_golden.py main_geo) are the reference itself run at layer
interfaces other than the two sets the kernels hold at compile time, at
NISURF 36, 12 and 24.  The oracle (oracle/h9_oracle.c) and the kernel body
built for the host with runtime geometry (const_geo = 0: make_geo_r) must
reproduce them bit for bit, so that a layer depth, a node spacing, zi(L) or
zi(L+1) baked into either shows; co_geo_a does the same for the reference's own
cell order, stop_geo_ns36 (kind `stop`: tests/test_oracle_golden.py) for a STOP
record.  tests/test_gpu_geo.py then holds the device build to these."""
import numpy as np
import pytest

from oracle import port, refcase
from tests.conftest import load_golden, same_bits
from tests.daily_helpers import LINE_INDEX, host_focus, port_daily8
from tests.evap_helpers import R_EVAP, host_evap, others, port_evap
from tests.geo_helpers import GEO_GOLDENS, first_cells, load_geo_golden
from tests.monthly_helpers import NM, annual_from_final, check_year_end, host_monthly
from tests.test_kernel_host import host_run

IDX = list(LINE_INDEX)


@pytest.mark.parametrize("name", GEO_GOLDENS)
def test_oracle_matches_reference_geo(name):
    meta, inp, exp = load_geo_golden(name)
    out = port.run(**{k: v for k, v in inp.items() if k != "state0"}, nthreads=4)
    assert out["rc"] == 0, out["err"]
    assert same_bits(out["annual"], exp["annual"])
    assert same_bits(refcase.pack_state(out["state"], meta["L"]), exp["state"])


@pytest.mark.parametrize("name", GEO_GOLDENS)
def test_kernel_body_matches_reference_geo(name):
    meta, inp, exp = load_geo_golden(name)
    out = host_run(const_geo=0, **inp)
    assert out["rc"] == 0
    assert same_bits(out["annual"], exp["annual"])
    assert same_bits(out["state"], exp["state"])


def test_kernel_body_reproduces_reference_stop_geo():
    """The STOP the reference prints at layers A, NISURF 36 (kind `stop`: the
    oracle's leg is tests/test_oracle_golden.py's)."""
    meta, inp, _ = load_golden("stop_geo_ns36")
    assert meta["nisurf"] == 36 and meta["zi"][1] == 30.0
    out = host_run(const_geo=0, **inp)
    s = meta["stop"]
    c = s["cell"]
    assert out["rc"] == s["code"]
    assert out["err"][c, 0] == s["code"] and out["err"][c, 2] == s["day"]
    assert np.array_equal(np.nonzero(out["err"][:, 0])[0], [c])


def test_geo_goldens_end_in_both_water_table_regimes():
    """What the generator asserted on the reference's output, read back from
    the fixtures: the water table ends inside the column for at least 4 cells
    and below it for at least 4, and nothing is NaN."""
    for name in GEO_GOLDENS:
        meta, inp, exp = load_geo_golden(name)
        L, n = meta["L"], meta["ncell"]
        assert n == 32 and not np.isnan(exp["annual"]).any() and not np.isnan(exp["state"]).any()
        zwt = refcase.unpack_state(exp["state"], n, L)["zwt"]
        inside = int((zwt * np.float32(1000.0) < inp["zi"][L]).sum())
        assert inside >= 4 and n - inside >= 4, (name, inside)


def test_oracle_cell_order_matches_reference_geo():
    """The reference's own cell order at layers A, NISURF 36, two decades: the
    carry changes the second decade (meta: at least 20 cell-years)."""
    meta, inp, exp = load_golden("co_geo_a")
    assert meta["isolated_vs_cell_order"]["cell_years_differing"] >= 20
    out = port.run_cell_order(**{k: v for k, v in inp.items() if k != "state0"})
    assert out["rc"] == 0
    assert same_bits(out["annual"], exp["annual"])
    assert same_bits(refcase.pack_state(out["state"], meta["L"]), exp["state"])


# ---- the host siblings at layers A, NISURF 36: 8 cells, 1903 -----------------
@pytest.fixture(scope="module")
def a8():
    meta, inp, exp = load_geo_golden("geo_a_ns36")
    return meta, first_cells(inp, 8), exp["annual"][:1, :, :8]


def test_host_monthly_geo(a8):
    meta, inp, ann = a8
    out = host_monthly(const_geo=0, **inp)
    assert out["rc"] == 0
    assert same_bits(out["annual"], ann)
    check_year_end(out["monthly"], out["annual"], inp["year0"], inp["nisurf"])
    assert same_bits(annual_from_final(out["monthly"][0, NM - 1], inp["year0"], inp["nisurf"]), ann[0])


def test_host_evap_geo(a8):
    meta, inp, ann = a8
    o = others(meta["L"])
    out = host_evap(const_geo=0, **inp)
    assert out["rc"] == 0
    assert same_bits(out["annual"][:, o], ann[:, o])
    fin = annual_from_final(out["monthly"][0, NM - 1], inp["year0"], inp["nisurf"])
    assert same_bits(fin[o], ann[0][o]) and same_bits(fin[R_EVAP], out["annual"][0, R_EVAP])
    ea, em, ref = port_evap(**inp)
    assert ref["rc"] == 0
    assert same_bits(out["annual"][:, R_EVAP], ea) and same_bits(out["monthly"][:, :, R_EVAP], em)


def test_host_focus_geo(a8):
    meta, inp, ann = a8
    d8, ref = port_daily8(**inp)
    out = host_focus(const_geo=0, **inp)
    assert ref["rc"] == out["rc"] == 0 and same_bits(ref["annual"], ann)
    assert same_bits(out["daily"][:, IDX], d8)
