"""Shared by tests/test_evap_host.py and tests/test_gpu_evap.py: the host build
of cell_year_pair with the ET policies (tests/csrc/host_evap.cpp, and its
forced-re-run variant), and the definition of the evaporation sum restated in
numpy float32 over the oracle's full per-substep trace:

    evap_sum = 0 at the start of the year                      (HYBRID9.f90:137)
    after every substep: evap_sum = evap_sum + (evg + tran) * dt

with tran the trace's column 3L+2, evg its column 3L+3 (qflx_evap_grnd after
the MIN(em1, .) of HYDROLOGY.f90:396-400) and dt = 86400 / NISURF.  Annual row
3 is evap_sum / FLOAT(nt * NISURF), month-end row 3 the sum as it stands."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np

from oracle import port, refcase
from tests.helpers import BUILD, ROOT
from tests.monthly_helpers import NM, month_ends

F = np.float32
R_RNF, R_EVAP, R_PR = 2, 3, 9

_libs = {}


def evap_lib(rerun=0):
    """libhost_evap.so, or with rerun = k the -DH9G_FORCE_RERUN=k build."""
    if rerun not in _libs:
        src = ROOT / "tests" / "csrc" / "host_evap.cpp"
        out = BUILD / (f"libhost_evap_rerun{rerun}.so" if rerun else "libhost_evap.so")
        deps = [src] + list((ROOT / "hybrid9_amd" / "csrc").glob("*.h"))
        if not out.exists() or out.stat().st_mtime < max(d.stat().st_mtime for d in deps):
            BUILD.mkdir(exist_ok=True)
            extra = [f"-DH9G_FORCE_RERUN={rerun}"] if rerun else []
            subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-std=c++17", "-fPIC",
                            "-shared", *extra, str(src), "-o", str(out)], check=True)
        lb = C.CDLL(str(out))
        fp = C.POINTER(C.c_float)
        lb.h9k_host_evap.argtypes = [C.c_int] * 7 + [fp, fp, fp, fp, fp, fp, C.POINTER(C.c_int)]
        lb.h9k_evap_exact.argtypes = [C.POINTER(C.c_longlong)]
        lb.h9k_evap_exact.restype = None
        _libs[rerun] = lb
    return _libs[rerun]


def host_evap(*, zi, params, forcing, nisurf, year0, nyears, grow_on, state0=None, const_geo=1, rerun=0,
              monthly=True):
    """cell_year_pair<..., EvapProf, MonthsEt> on the host for every cell:
    dict(rc, annual (nyears, 12+L, n), monthly (nyears, 12, 12+L, n) or None,
    state (packed), err (n, 4), exact (re-runs, substeps replayed)); NaN as
    monthly_helpers.host_monthly."""
    L = params["theta_s"].shape[1]
    n = params["fmax"].size
    zi = np.ascontiguousarray(zi, F)
    pp = port.pack_params(params)
    fo = np.ascontiguousarray(forcing, F)
    st = port.init_state(params, zi) if state0 is None else np.array(state0, F)
    ann = np.full((nyears, 12 + L, n), np.nan, F)
    mon = np.full((nyears, NM, 12 + L, n), np.nan, F) if monthly else None
    err = np.zeros(4 * n, np.int32)
    fp = C.POINTER(C.c_float)
    lb = evap_lib(rerun)
    ex = (C.c_longlong * 2)()
    lb.h9k_evap_exact(ex)
    rc = lb.h9k_host_evap(n, L, nisurf, int(grow_on), year0, nyears, int(const_geo), zi.ctypes.data_as(fp),
                          pp.ctypes.data_as(fp), fo.ctypes.data_as(fp), st.ctypes.data_as(fp),
                          ann.ctypes.data_as(fp), mon.ctypes.data_as(fp) if monthly else None,
                          err.ctypes.data_as(C.POINTER(C.c_int)))
    lb.h9k_evap_exact(ex)
    return dict(rc=rc, annual=ann, monthly=mon, state=st, err=err.reshape(n, 4), exact=(int(ex[0]), int(ex[1])))


def evap_from_trace(trace, L, nisurf, year0, nyears):
    """The definition over a full trace (ncells, ndays*nisurf, 3L+7) ->
    (annual row 3 (nyears, ncells), month-end row 3 (nyears, 12, ncells))."""
    tr = np.asarray(trace, F)
    n = tr.shape[0]
    dt = F(F(86400.0) / F(nisurf))
    # one term per substep; np.add.accumulate adds them one after another in
    # float32, from the first (0 + term is the term)
    term = ((tr[:, :, 3 * L + 3] + tr[:, :, 3 * L + 2]).astype(F) * dt).astype(F)
    ann = np.zeros((nyears, n), F)
    mon = np.zeros((nyears, NM, n), F)
    k = 0
    for y in range(nyears):
        nt = port._days(year0 + y)
        run = np.add.accumulate(term[:, k:k + nt * nisurf], axis=1, dtype=F)
        for m, d1 in enumerate(month_ends(year0 + y)):
            mon[y, m] = run[:, d1 * nisurf - 1]
        ann[y] = run[:, -1] / F(nt * nisurf)
        k += nt * nisurf
    assert k == tr.shape[1]
    return ann, mon


def port_evap(*, zi, params, forcing, nisurf, year0, nyears, grow_on, state0=None):
    """The oracle with every cell traced -> (annual row 3, month-end row 3, run)."""
    L = params["theta_s"].shape[1]
    n = params["fmax"].size
    s0 = None if state0 is None else refcase.unpack_state(np.asarray(state0, F), n, L)
    r = port.run(zi=zi, params=params, forcing=forcing, nisurf=nisurf, year0=year0, nyears=nyears,
                 grow_on=grow_on, state0=s0, trace_cells=tuple(range(n)), nthreads=8)
    a, m = evap_from_trace(r["trace"], L, nisurf, year0, nyears)
    return a, m, r


def cell_order_evap(*, zi, params, forcing, nisurf, year0, nyears, grow_on, chains=None):
    """Rows 3 of the reference's own order: port.run_cell_order's loop restated
    (decade -> cell -> year, smp carried from cell to cell, HYBRID9.f90:93-130;
    as tests/monthly_helpers.cell_order_snapshots) with every per-cell port.run
    traced in full.  Returns (annual row 3 (nyears, n), month-end row 3
    (nyears, 12, n), end state, annual); NaN for a masked cell."""
    L = params["theta_s"].shape[1]
    n = params["fmax"].size
    fo = np.ascontiguousarray(forcing, dtype=F)
    st = refcase.unpack_state(port.init_state(params, zi), n, L)
    st = {k: np.array(v, copy=True) for k, v in st.items()}
    ann = np.full((nyears, 12 + L, n), np.nan, dtype=F)
    ea = np.full((nyears, n), np.nan, dtype=F)
    em = np.full((nyears, NM, n), np.nan, dtype=F)
    land = [c for c in range(n) if port._mask_sum(params["theta_s"][c]) > F(1.0e-8)]
    cid = np.zeros(n, np.int64) if chains is None else np.asarray(chains, np.int64)
    groups = [[c for c in land if cid[c] == r] for r in sorted(set(cid[land].tolist()))]
    day0 = 0
    for y0, ny in port.decades(year0, nyears):
        nd = sum(port._days(y0 + k) for k in range(ny))
        carry = {grp[0]: st["smp"][grp[-1]].copy() for grp in groups}
        prev = {b: a for grp in groups for a, b in zip(grp, grp[1:])}
        k0 = y0 - year0
        for c in land:
            s1 = {k: v[c:c + 1].copy() for k, v in st.items()}
            s1["smp"][0] = carry[c] if c in carry else st["smp"][prev[c]].copy()
            f1 = np.ascontiguousarray(fo[:, day0:day0 + nd, c:c + 1])
            r = port.run(zi=zi, params={k: v[c:c + 1] for k, v in params.items()}, forcing=f1, nisurf=nisurf,
                         year0=y0, nyears=ny, grow_on=grow_on, state0=s1, trace_cells=(0,))
            assert r["rc"] == 0
            a, m = evap_from_trace(r["trace"], L, nisurf, y0, ny)
            ea[k0:k0 + ny, c] = a[:, 0]
            em[k0:k0 + ny, :, c] = m[:, :, 0]
            for k in st:
                st[k][c] = r["state"][k][0]
            ann[k0:k0 + ny, :, c] = r["annual"][:, :, 0]
        day0 += nd
    return ea, em, st, ann


def others(L):
    """Every row of the 12+L but evap."""
    return [k for k in range(12 + L) if k != R_EVAP]


def water_balance_residual(ann, state0, state1, L, jyear, nisurf):
    """P - R - E - dS per cell for one year, in float64: P the year's rain
    (row pr is its mean in kg/m^2/s = mm/s), R and E rows rnf and evap times
    nt * nisurf (mm), S = sum of h2osoi_liq + wa from the packed states before
    and after the year."""
    n = ann.shape[1]
    nt = port._days(jyear)
    a = np.asarray(ann, np.float64)
    P = a[R_PR] * nt * 86400.0
    R = a[R_RNF] * nt * nisurf
    E = a[R_EVAP] * nt * nisurf
    s0, s1 = (refcase.unpack_state(np.asarray(s, F), n, L) for s in (state0, state1))
    S = [s["h2osoi_liq"].astype(np.float64).sum(axis=1) + s["wa"].astype(np.float64) for s in (s0, s1)]
    return P - R - E - (S[1] - S[0])
