"""Spin-up to equilibrium without a GPU: the host build of the per-cell test
(hybrid9_amd/csrc/h9g_spin.h through tests/csrc/host_spin.cpp) against the
rule restated in numpy on the oracle's states (tests/spinup_helpers.py), bit
for bit; its edge cases; and what h9g_spinup validates with no device."""
import ctypes as C
import re

import numpy as np
import pytest

import hybrid9_amd as h
from oracle import refcase
from tests.conftest import load_golden, same_bits
from tests.daily_helpers import stop_mask_inputs
from tests.spinup_helpers import (D, F, check_meaningful, drift_of, drifts, emulate, histogram, host_soil, host_spin,
                                  issue_tolerances, keys_of, land_of, max_of, met_of, trajectory)

K = 6


def _traj(name):
    if name == "stop_mask":
        meta, inp = stop_mask_inputs()
    else:
        meta, inp, _ = load_golden(name)
    return meta, inp, trajectory((name, 1, K), inp, 1, K)


@pytest.mark.parametrize("name", ["c1_10x10", "stop_ns24"])
def test_host_build_equals_the_restated_rule_on_oracle_states(name):
    """Keys, drifts, decisions and maxima of every cycle of the oracle's
    trajectory: the header's lines against the numpy restatement."""
    meta, inp, tr = _traj(name)
    L = tr["L"]
    tol = issue_tolerances(tr, plant=True)
    for k in range(1, K + 1):
        a, b = tr["states"][k - 1], tr["states"][k]
        got = host_spin(refcase.pack_state(a, L), refcase.pack_state(b, L), L, k, min_cycles=2, **tol)
        ka, kb = keys_of(a, L), keys_of(b, L)
        d = drift_of(ka, kb)
        assert same_bits(got["keys"][0], np.stack(ka)) and same_bits(got["keys"][1], np.stack(kb))
        assert same_bits(got["drift"], np.stack(d))
        assert np.array_equal(got["met"], met_of(d, k, 2, **tol))
        every = np.ones(tr["n"], bool)
        assert same_bits(got["maxima"], np.array([max_of(x, every) for x in d]))
    assert np.array_equal(host_soil(inp["params"]), land_of(inp["params"]))


@pytest.mark.parametrize("plant", [False, True])
@pytest.mark.parametrize("name", ["c1_10x10", "stop_ns24"])
def test_issue_tolerances_retire_cells_at_different_cycles(name, plant):
    """The tolerances chosen from the oracle's own drifts spread the settling
    over the cycles (the histograms the issue reports for tol_plant = +inf)."""
    meta, inp, tr = _traj(name)
    em = emulate(tr, max_cycles=K, freeze=True, **issue_tolerances(tr, plant))
    print(name, "plant" if plant else "inf", histogram(em, K), em["history"][:, :3].tolist())
    check_meaningful(em)
    if not plant:
        want = {"c1_10x10": [36, 2, 33, 13, 7, 6, 3], "stop_ns24": [1, 0, 2, 2, 1, 0, 1]}[name]
        assert histogram(em, K) == want
    if name == "stop_ns24":
        assert (em["cell_cycle"] == -2).sum() == 1 and em["rc"] == meta["stop"]["code"]
    # freeze = 0 records the same first-met cycles for the cells freeze = 1 retires
    em0 = emulate(tr, max_cycles=K, freeze=False, **issue_tolerances(tr, plant))
    assert np.array_equal(em0["cell_cycle"], em["cell_cycle"])
    assert (em0["last"][em0["cell_cycle"] >= 0] == em0["cycles"]).all()


def _two(L=8, **fields):
    """Two packed states of 4 cells that differ only in the given fields
    (name=(prev, cur) arrays)."""
    n = 4
    base = {f: np.zeros((n, w) if w > 1 else n, F) for f, w in refcase.state_fields(L)}
    base["h2osoi_liq"][:] = 30.0
    base["wa"][:] = 4800.0
    base["zwt"][:] = 3000.0
    base["plant_mass"][:] = 2.0
    a = {f: np.array(v, copy=True) for f, v in base.items()}
    b = {f: np.array(v, copy=True) for f, v in base.items()}
    for f, (x, y) in fields.items():
        a[f][:] = np.asarray(x, F)
        b[f][:] = np.asarray(y, F)
    return refcase.pack_state(a, L), refcase.pack_state(b, L)


def test_plant_drift_edge_cases():
    """pm_k == pm_{k-1} == 0 is no drift; a zero pm_{k-1} gives +inf, which
    only tol_plant = +inf accepts; a NaN never settles; neither does +inf != +inf."""
    a, b = _two(plant_mass=([0.0, 0.0, 2.0, np.nan], [0.0, 1.5, 2.0, np.nan]))
    got = host_spin(a, b, 8, 1, tol_water=0.0, tol_zwt=0.0, tol_plant=0.0)
    assert same_bits(got["drift"][2], np.array([0.0, np.inf, 0.0, np.nan]))
    assert got["met"].tolist() == [True, False, True, False]
    assert same_bits(got["maxima"], np.array([0.0, 0.0, np.inf]))
    got = host_spin(a, b, 8, 1, tol_water=0.0, tol_zwt=0.0, tol_plant=np.inf)
    assert got["met"].tolist() == [True, True, True, False]
    # pm_{k-1} = +inf: inf - 1 = inf, inf / inf = NaN
    a, b = _two(plant_mass=([np.inf] * 4, [1.0, np.inf, -np.inf, 1.0]))
    got = host_spin(a, b, 8, 1, tol_plant=np.inf)
    assert got["met"].tolist() == [False, True, False, False]


def test_nan_water_and_zwt_do_not_settle_and_are_not_counted():
    a, b = _two(wa=([4800.0] * 4, [4800.0, np.nan, 4801.0, 4800.0]),
                zwt=([3000.0] * 4, [3000.0, 3000.0, 3000.0, np.nan]))
    got = host_spin(a, b, 8, 3)            # every tolerance +inf: only a NaN keeps a cell active
    assert got["met"].tolist() == [True, False, True, False]
    assert same_bits(got["maxima"], np.array([1.0, 0.0, 0.0]))
    assert np.isnan(got["drift"][0][1]) and np.isnan(got["drift"][1][3])


def test_water_key_adds_the_layers_in_order_in_double():
    """W is the float64 sum in layer order, then wa -- not a float32 sum and
    not a pairwise one."""
    r = np.random.default_rng(5)
    L, n = 10, 4
    st = {f: r.uniform(1.0, 300.0, (n, w) if w > 1 else n).astype(F) for f, w in refcase.state_fields(L)}
    p = refcase.pack_state(st, L)
    got = host_spin(p, p, L, 1)
    w = np.zeros(n, D)
    for i in range(L):
        w = w + st["h2osoi_liq"][:, i].astype(D)
    w = w + st["wa"].astype(D)
    assert same_bits(got["keys"][0][0], w)
    assert not same_bits(w, st["h2osoi_liq"].sum(axis=1, dtype=F).astype(D) + st["wa"])
    assert got["met"].all() and same_bits(got["drift"], np.zeros((3, n)))


def test_min_cycles_holds_every_cell_back():
    a, b = _two()
    assert not host_spin(a, b, 8, 2, min_cycles=3, tol_water=0.0, tol_zwt=0.0, tol_plant=0.0)["met"].any()
    assert host_spin(a, b, 8, 3, min_cycles=3, tol_water=0.0, tol_zwt=0.0, tol_plant=0.0)["met"].all()
    meta, inp, tr = _traj("c1_10x10")
    tol = issue_tolerances(tr, False)
    em = emulate(tr, max_cycles=K, min_cycles=4, **tol)
    assert not ((em["cell_cycle"] > 0) & (em["cell_cycle"] < 4)).any() and (em["cell_cycle"] == 4).sum() > 10
    assert em["history"][:3, 1].sum() == 0


def test_zero_tolerance_is_a_bit_exact_fixed_point():
    a, b = _two(wa=([4800.0] * 4, [4800.0, np.nextafter(F(4800.0), F(5000.0)), 4800.0, 4800.0]))
    got = host_spin(a, b, 8, 1, tol_water=0.0, tol_zwt=0.0, tol_plant=0.0)
    assert got["met"].tolist() == [True, False, True, True]


# ---- the entry points, no GPU -------------------------------------------------
def _opts(**kw):
    return h.spin_opts(**dict(dict(max_cycles=3), **kw))


def test_spinup_rejects_null_and_bad_options():
    lb = h.lib()
    i32 = C.POINTER(C.c_int32)
    slots = (C.c_int32 * 1)(0)
    assert lb.h9g_spinup(None, slots, 1901, 1, C.byref(_opts()), None, None, None) == -1
    st = np.zeros(4 * 8 + 9, F)
    lst, cc, stats = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(7, D)

    def selftest(o, k=1, n=1, L=8):
        return lb.h9g_spin_selftest(0, n, L, st.ctypes.data_as(C.POINTER(C.c_float)),
                                    st.ctypes.data_as(C.POINTER(C.c_float)), None, C.byref(o) if o else None, k,
                                    lst.ctypes.data_as(i32), cc.ctypes.data_as(i32),
                                    stats.ctypes.data_as(C.POINTER(C.c_double)))
    # the options are validated before a device is touched (H9G_EINVAL = -1)
    bad = [dict(max_cycles=0), dict(min_cycles=0), dict(min_cycles=4), dict(tol_water=-1.0), dict(tol_zwt=np.nan),
           dict(tol_plant=-0.5), dict(tol_water=-np.inf)]
    for kw in bad:
        assert selftest(_opts(**kw)) == -1, kw
    o = _opts()
    o.reserved = 1
    assert selftest(o) == -1
    o = _opts()
    o.freeze = 2
    assert selftest(o) == -1
    assert selftest(None) == -1
    assert selftest(_opts(), k=0) == -1 and selftest(_opts(), n=0) == -1 and selftest(_opts(), L=9) == -1


def test_spinup_is_declared_exported_and_bound():
    syms = h.exported_symbols()
    assert "h9g_spinup" in syms and "h9g_spin_selftest" in syms
    lb = h.lib()
    assert lb.h9g_spinup.argtypes and lb.h9g_spin_selftest.argtypes
    src = (h.HERE / "fortran" / "h9_gpu.f90").read_text()
    bound = set(re.findall(r"NAME='(h9g_[a-z_0-9]+)'", src))
    assert {"h9g_spinup", "h9g_spin_selftest"} <= bound
    hdr = (h.HERE.parent / "include" / "h9g.h").read_text()
    assert "#define H9G_NSPIN 6" in hdr and h.NSPIN == 6 and len(h.SPIN_HISTORY) == 6
    assert C.sizeof(h._SpinOpts) == 40
    host = (h.HERE / "fortran" / "h9_host.f90").read_text()
    for key in ("spinup_cycles", "spinup_years", "spinup_min_cycles", "spinup_freeze", "spinup_tol_water",
                "spinup_tol_zwt", "spinup_tol_plant"):
        assert key in host


def test_config_bytes_does_not_count_spinup_buffers():
    """The call's buffers are allocated by the call: h9g_config_bytes is what
    it was (67,420 cells, L = 8, two slots: the figure of the parent commit)."""
    zi = [0.0, 45.0, 91.0, 166.0, 289.0, 493.0, 829.0, 1383.0, 2296.0, 5000.0]
    assert h.config_bytes(h.make_config(67420, zi)) == 3438806184
    zi10 = [0.0, 18.0, 45.0, 91.0, 166.0, 289.0, 493.0, 829.0, 1383.0, 2296.0, 3500.0, 5000.0]
    assert h.config_bytes(h.make_config(1000, zi10, nlayers=10, nisurf=24, nslots=3)) == 94845432
    assert h.Context.spinup.__doc__ and "spinup" in h.run.__doc__
