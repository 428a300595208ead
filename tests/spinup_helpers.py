"""Shared by tests/test_spinup_host.py and tests/test_gpu_spinup.py: the rule
of h9g_spinup (include/h9g.h) restated in numpy over the CPU oracle.

``trajectory`` runs ``oracle.port.run`` cycle by cycle for ALL cells: isolated
cells are independent, so a cell that settles at cycle k is expected to hold
its state at the end of cycle k of that trajectory, whatever the others do.
The stopped set is carried across the cycles here (the oracle itself would
run a stopped cell again).  ``emulate`` then applies the rule to the
trajectory: W = the layers added one by one in float64, then wa; d_w, d_z,
d_p; the decision; cell_cycle, the history rows and what the call must leave
behind.  ``host_spin`` is the host build of hybrid9_amd/csrc/h9g_spin.h
(tests/csrc/host_spin.cpp), the lines the kernel runs per cell."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np

from oracle import port, refcase
from tests.helpers import BUILD, ROOT

F = np.float32
D = np.float64
NTHREADS = 16
_lib = None
_traj = {}


def spin_lib():
    global _lib
    if _lib is None:
        src = ROOT / "tests" / "csrc" / "host_spin.cpp"
        out = BUILD / "libhost_spin.so"
        deps = [src] + list((ROOT / "hybrid9_amd" / "csrc").glob("*.h"))
        if not out.exists() or out.stat().st_mtime < max(d.stat().st_mtime for d in deps):
            BUILD.mkdir(exist_ok=True)
            subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-fPIC", "-shared",
                            str(src), "-o", str(out)], check=True)
        _lib = C.CDLL(str(out))
        fp, dp, ip = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int)
        _lib.h9k_host_spin.argtypes = [C.c_int, C.c_int, fp, fp, C.c_int, C.c_int, C.c_double, C.c_double,
                                       C.c_double, dp, dp, ip, dp]
        _lib.h9k_host_spin_soil.argtypes = [C.c_int, C.c_int, fp, ip]
        _lib.h9k_host_spin_soil.restype = None
    return _lib


def host_spin(prev, cur, L, k, *, min_cycles=1, tol_water=np.inf, tol_zwt=np.inf, tol_plant=np.inf):
    """spin_key / spin_drift / spin_settled / spin_max on the host for packed
    states prev, cur: dict(keys (2, 3, n), drift (3, n), met (n), maxima (3))."""
    a, b = np.ascontiguousarray(prev, F).ravel(), np.ascontiguousarray(cur, F).ravel()
    n = a.size // (4 * L + 9)
    keys, drift = np.zeros((2, 3, n), D), np.zeros((3, n), D)
    met, mx = np.zeros(n, np.int32), np.zeros(3, D)
    fp, dp, ip = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int)
    rc = spin_lib().h9k_host_spin(n, L, a.ctypes.data_as(fp), b.ctypes.data_as(fp), int(k), int(min_cycles),
                                  float(tol_water), float(tol_zwt), float(tol_plant), keys.ctypes.data_as(dp),
                                  drift.ctypes.data_as(dp), met.ctypes.data_as(ip), mx.ctypes.data_as(dp))
    assert rc == 0
    return dict(keys=keys, drift=drift, met=met.astype(bool), maxima=mx)


def host_soil(params):
    L = params["theta_s"].shape[1]
    n = params["fmax"].size
    pp = port.pack_params(params)
    out = np.zeros(n, np.int32)
    spin_lib().h9k_host_spin_soil(n, L, pp.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_int)))
    return out.astype(bool)


# ---- the rule, restated ------------------------------------------------------
def keys_of(st, L):
    """(W, zwt, pm) in float64 of a state dict: the layers added in a Python
    loop, in order, then wa."""
    h = np.asarray(st["h2osoi_liq"], F)
    w = np.zeros(h.shape[0], D)
    for i in range(L):
        w = w + h[:, i].astype(D)
    w = w + np.asarray(st["wa"], F).astype(D)
    return w, np.asarray(st["zwt"], F).astype(D), np.asarray(st["plant_mass"], F).astype(D)


def drift_of(prev, now):
    """(d_w, d_z, d_p) from keys one cycle apart."""
    with np.errstate(all="ignore"):
        d_w = np.abs(now[0] - prev[0])
        d_z = np.abs(now[1] - prev[1])
        d_p = np.where(now[2] == prev[2], 0.0, np.abs(now[2] - prev[2]) / np.abs(prev[2]))
    return d_w, d_z, d_p


def met_of(d, k, min_cycles, tol_water, tol_zwt, tol_plant):
    with np.errstate(invalid="ignore"):
        return (k >= min_cycles) & (d[0] <= tol_water) & (d[1] <= tol_zwt) & (d[2] <= tol_plant)


def max_of(x, sel):
    """The maximum over the selected cells: 0 with none, a NaN not counted."""
    return float(np.fmax.reduce(x[sel], initial=0.0)) if sel.any() else 0.0


def land_of(params):
    return np.array([port._mask_sum(t) > F(1.0e-8) for t in params["theta_s"]])


def trajectory(key, inp, years, cycles):
    """The oracle's states after cycles 0..cycles of the first `years` years of
    inp, every cell running every cycle until it stops.  Cached by `key`: the
    reference is computed once and shared.  Returns dict(L, n, land, states
    [cycles+1] (dicts), annual [cycles+1] (12+L, n: the last year of the
    cycle), err (4, n) int32 records with the value's bits, stop_cycle (n; 0:
    none), stop_year (n), ran0 (n): land and not stopped at the start."""
    if key in _traj:
        return _traj[key]
    p, zi = inp["params"], inp["zi"]
    L, n = p["theta_s"].shape[1], p["fmax"].size
    nd = sum(port._days(inp["year0"] + y) for y in range(years))
    fo = np.ascontiguousarray(inp["forcing"][:, :nd])
    st = refcase.unpack_state(port.init_state(p, zi) if inp.get("state0") is None
                              else np.asarray(inp["state0"], F), n, L)
    st = {k: np.array(v, copy=True) for k, v in st.items()}
    land = land_of(p)
    states, annual = [st], [np.full((12 + L, n), np.nan, F)]
    err = np.zeros((4, n), np.int32)
    stop_cycle, stop_year = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for k in range(1, cycles + 1):
        r = port.run(zi=zi, params=p, forcing=fo, nisurf=inp["nisurf"], year0=inp["year0"], nyears=years,
                     grow_on=int(inp["grow_on"]), state0=st, nthreads=NTHREADS)
        e = r["errors"]
        new = land & (stop_cycle == 0) & (e["code"] != 0)
        for c in np.nonzero(new)[0]:
            err[:, c] = (e["code"][c], e["day"][c], e["substep"][c], e["value"][c:c + 1].view(np.int32)[0])
            stop_cycle[c] = k
            y = 0                      # the first year whose means it did not complete
            while y < years - 1 and not np.isnan(r["annual"][y, 0, c]):
                y += 1
            stop_year[c] = inp["year0"] + y
        st = {f: np.array(v, copy=True) for f, v in r["state"].items()}
        ann = np.array(r["annual"][years - 1], copy=True)
        gone = stop_cycle > 0
        ann[:, gone] = np.nan
        states.append(st)
        annual.append(ann)
    _traj[key] = dict(L=L, n=n, land=land, states=states, annual=annual, err=err, stop_cycle=stop_cycle,
                      stop_year=stop_year, years=years, year0=inp["year0"])
    return _traj[key]


def drifts(traj):
    """Per cycle k = 1..K: (d_w, d_z, d_p, tested) of the cells that ran cycle
    k and did not stop in it."""
    out = []
    for k in range(1, len(traj["states"])):
        d = drift_of(keys_of(traj["states"][k - 1], traj["L"]), keys_of(traj["states"][k], traj["L"]))
        sc = traj["stop_cycle"]
        out.append((*d, traj["land"] & ((sc == 0) | (sc > k))))
    return out


def issue_tolerances(traj, plant):
    """The issue's choice, from the oracle's own drifts: tol_water the median
    of cycle-3 d_w over the running cells, tol_zwt four times the median of
    cycle-3 d_z, tol_plant +inf or the median of cycle-4 d_p."""
    d = drifts(traj)
    w3, z3, _, t3 = d[2]
    _, _, p4, t4 = d[3]
    return dict(tol_water=float(np.median(w3[t3])), tol_zwt=float(4.0 * np.median(z3[t3])),
                tol_plant=float(np.median(p4[t4])) if plant else np.inf)


def emulate(traj, *, max_cycles, min_cycles=1, tol_water=np.inf, tol_zwt=np.inf, tol_plant=np.inf, freeze=True):
    """h9g_spinup over the trajectory: dict(cycles, cell_cycle, history
    (cycles, 6), state (dict: every cell after the last cycle it ran), annual
    (12+L, n), err (4, n), ok (n: never stopped), last (n: the last cycle each
    cell ran), rc, first_stop (cell, year) or None)."""
    L, n, land, sc = traj["L"], traj["n"], traj["land"], traj["stop_cycle"]
    assert max_cycles < len(traj["states"])
    cc = np.where(land, 0, -1).astype(np.int32)
    last = np.zeros(n, np.int32)
    hist, cycles = [], 0
    active = cc == 0
    for k in range(1, max_cycles + 1):
        if not active.any():
            break
        ran = (cc == 0) if freeze else (cc >= 0)
        stopped = ran & (sc == k)
        tested = ran & ~stopped
        d = drift_of(keys_of(traj["states"][k - 1], L), keys_of(traj["states"][k], L))
        met = tested & met_of(d, k, min_cycles, tol_water, tol_zwt, tol_plant)
        first = met & (cc == 0)
        cc[first] = k
        cc[stopped] = -2
        last[ran] = k
        hist.append([ran.sum(), first.sum(), stopped.sum(), max_of(d[0], tested), max_of(d[1], tested),
                     max_of(d[2], tested)])
        active = tested & ~met
        cycles = k
    state = {f: np.array(v, copy=True) for f, v in traj["states"][0].items()}
    annual = np.full((12 + L, n), np.nan, F)
    for c in range(n):
        for f in state:
            state[f][c] = traj["states"][last[c]][f][c]
        annual[:, c] = traj["annual"][last[c]][:, c]
    err = np.array(traj["err"], copy=True)
    err[:, cc != -2] = 0
    stops = np.nonzero(cc == -2)[0]
    return dict(cycles=cycles, cell_cycle=cc, history=np.array(hist, D).reshape(-1, 6), state=state, annual=annual,
                err=err, ok=cc != -2, last=last, rc=int(err[0, stops[0]]) if stops.size else 0,
                first_stop=(int(stops[0]), int(traj["stop_year"][stops[0]])) if stops.size else None)


def check_meaningful(em):
    """A test that retires nothing, or everything at once, shows nothing: at
    least three distinct settling cycles, one cell settled before the last
    cycle, one still active at the end."""
    cc = em["cell_cycle"]
    settled = cc[cc > 0]
    assert np.unique(settled).size >= 3, np.bincount(settled)
    assert (settled < em["cycles"]).any()
    assert (cc == 0).any()


def histogram(em, K):
    """[active at the end, settled at cycle 1, ..., cycle K]"""
    cc = em["cell_cycle"]
    return [int((cc == 0).sum())] + [int((cc == k).sum()) for k in range(1, K + 1)]
