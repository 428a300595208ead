"""Shared by tests/test_days_host.py and tests/test_gpu_days.py: the host build
of cell_year_pair with the day kernels' policies (tests/csrc/host_days.cpp,
and its forced-re-run variant), and the day record of include/h9g.h restated
in numpy float32 over the oracle's full per-substep trace (3L+7 columns per
substep, oracle/h9_oracle.c:712-726):

    row 0  rnf_sum          column 3L+4 of the day's last substep
    row 1  evap_sum         evap_helpers.evap_from_trace's f32 accumulation,
                            read at the day's last substep
    row 2  W                columns 0..L-1 of the day's last substep, added in
                            that order
    row 3  theta(1)         column 2L of the day's last substep
    row 4  zwt              column 3L
    row 5  wa               column 3L+1
    row 6  LAI after GROW   column 3L+5 of the next day's first substep; for
                            the run's last day the end state's LAI

and the two ties of the records to the annual means and month-end snapshots."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np

from oracle import port, refcase
from tests.helpers import BUILD, ROOT
from tests.monthly_helpers import NM, month_ends

F = np.float32
ND = 7                   # H9G_NDAYREC
MAXD = 366
R_RNF, R_EVAP = 2, 3     # rows of the annual means and of a snapshot

_libs = {}


def days_lib(rerun=0):
    """libhost_days.so, or with rerun = k the -DH9G_FORCE_RERUN=k build."""
    if rerun not in _libs:
        src = ROOT / "tests" / "csrc" / "host_days.cpp"
        out = BUILD / (f"libhost_days_rerun{rerun}.so" if rerun else "libhost_days.so")
        deps = [src] + list((ROOT / "hybrid9_amd" / "csrc").glob("*.h"))
        if not out.exists() or out.stat().st_mtime < max(d.stat().st_mtime for d in deps):
            BUILD.mkdir(exist_ok=True)
            extra = [f"-DH9G_FORCE_RERUN={rerun}"] if rerun else []
            subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-std=c++17", "-fPIC",
                            "-shared", *extra, str(src), "-o", str(out)], check=True)
        lb = C.CDLL(str(out))
        fp = C.POINTER(C.c_float)
        lb.h9k_host_days.argtypes = [C.c_int] * 7 + [fp, fp, fp, fp, fp, fp, fp, C.POINTER(C.c_int)]
        lb.h9k_days_exact.argtypes = [C.POINTER(C.c_longlong)]
        lb.h9k_days_exact.restype = None
        _libs[rerun] = lb
    return _libs[rerun]


def host_days(*, zi, params, forcing, nisurf, year0, nyears, grow_on, state0=None, const_geo=1, rerun=0,
              monthly=True):
    """cell_year_pair<..., EvapProf, DaysEt> on the host for every cell:
    dict(rc, annual (nyears, 12+L, n), monthly (nyears, 12, 12+L, n) or None,
    days (nyears, 366, 7, n), state (packed), err (n, 4), exact (re-runs,
    substeps replayed)).  days: NaN for a masked cell, from its STOP day on for
    a cell that stops, and on day 366 of a 365-day year."""
    L = params["theta_s"].shape[1]
    n = params["fmax"].size
    zi = np.ascontiguousarray(zi, F)
    pp = port.pack_params(params)
    fo = np.ascontiguousarray(forcing, F)
    st = port.init_state(params, zi) if state0 is None else np.array(state0, F)
    ann = np.full((nyears, 12 + L, n), np.nan, F)
    mon = np.full((nyears, NM, 12 + L, n), np.nan, F) if monthly else None
    days = np.full((nyears, MAXD, ND, n), np.nan, F)
    err = np.zeros(4 * n, np.int32)
    fp = C.POINTER(C.c_float)
    lb = days_lib(rerun)
    ex = (C.c_longlong * 2)()
    lb.h9k_days_exact(ex)
    rc = lb.h9k_host_days(n, L, nisurf, int(grow_on), year0, nyears, int(const_geo), zi.ctypes.data_as(fp),
                          pp.ctypes.data_as(fp), fo.ctypes.data_as(fp), st.ctypes.data_as(fp),
                          ann.ctypes.data_as(fp), mon.ctypes.data_as(fp) if monthly else None,
                          days.ctypes.data_as(fp), err.ctypes.data_as(C.POINTER(C.c_int)))
    lb.h9k_days_exact(ex)
    return dict(rc=rc, annual=ann, monthly=mon, days=days, state=st, err=err.reshape(n, 4),
                exact=(int(ex[0]), int(ex[1])))


def records_from_trace(trace, end_lai, L, nisurf, year0, nyears):
    """The table above over a full trace (ncells, ndays*nisurf, 3L+7) of cells
    that did not stop, and their end-state LAI (ncells) -> (nyears, 366, 7,
    ncells); day 366 of a 365-day year is NaN."""
    tr = np.asarray(trace, F)
    n = tr.shape[0]
    last = tr[:, nisurf - 1::nisurf]          # the days' last substeps (ncells, ndays, 3L+7)
    first = tr[:, ::nisurf]                   # ... and first ones
    ndays = last.shape[1]
    dt = F(F(86400.0) / F(nisurf))
    term = ((tr[:, :, 3 * L + 3] + tr[:, :, 3 * L + 2]).astype(F) * dt).astype(F)
    w = last[:, :, 0].astype(F)
    for i in range(1, L):
        w = (w + last[:, :, i]).astype(F)
    lai = np.empty((n, ndays), F)
    lai[:, :-1] = first[:, 1:, 3 * L + 5]
    lai[:, -1] = np.asarray(end_lai, F)
    out = np.full((nyears, MAXD, ND, n), np.nan, F)
    d0 = 0
    for y in range(nyears):
        nt = port._days(year0 + y)
        sl = slice(d0, d0 + nt)
        # the year's sum from zero, one term per substep added one after another in float32
        run = np.add.accumulate(term[:, d0 * nisurf:(d0 + nt) * nisurf], axis=1, dtype=F)
        out[y, :nt, 0] = last[:, sl, 3 * L + 4].T
        out[y, :nt, 1] = run[:, nisurf - 1::nisurf].T
        out[y, :nt, 2] = w[:, sl].T
        out[y, :nt, 3] = last[:, sl, 2 * L].T
        out[y, :nt, 4] = last[:, sl, 3 * L].T
        out[y, :nt, 5] = last[:, sl, 3 * L + 1].T
        out[y, :nt, 6] = lai[:, sl].T
        d0 += nt
    assert d0 == ndays
    return out


def port_days(*, zi, params, forcing, nisurf, year0, nyears, grow_on, state0=None):
    """The oracle with every cell traced -> (records_from_trace, run)."""
    L = params["theta_s"].shape[1]
    n = params["fmax"].size
    s0 = None if state0 is None else refcase.unpack_state(np.asarray(state0, F), n, L)
    r = port.run(zi=zi, params=params, forcing=forcing, nisurf=nisurf, year0=year0, nyears=nyears,
                 grow_on=grow_on, state0=s0, trace_cells=tuple(range(n)), nthreads=8)
    return records_from_trace(r["trace"], r["state"]["LAI"], L, nisurf, year0, nyears), r


def check_ties(days, annual, monthly, year0, nisurf):
    """For every cell-year that did not stop (finite annual rows rnf and evap):
    rows 0 and 1 of the year's last day, divided by FLOAT(nt * NISURF) in f32,
    are annual rows rnf and evap; rows 0 and 1 at each month's last day are
    rows 2 and 3 of that month's snapshot (monthly may be None).  Returns the
    number of cell-years checked."""
    from tests.conftest import same_bits
    days, annual = np.asarray(days), np.asarray(annual)
    seen = 0
    for y in range(annual.shape[0]):
        nt = port._days(year0 + y)
        ran = np.isfinite(annual[y, R_RNF]) & np.isfinite(annual[y, R_EVAP])
        seen += int(ran.sum())
        for r, row in ((0, R_RNF), (1, R_EVAP)):
            assert same_bits((days[y, nt - 1, r][ran] / F(nt * nisurf)).astype(F), annual[y, row][ran]), \
                f"year {year0 + y}: row {r} of the last day is not annual row {row}"
            if monthly is not None:
                for m, d1 in enumerate(month_ends(year0 + y)):
                    assert same_bits(days[y, d1 - 1, r][ran], np.asarray(monthly)[y, m, row][ran]), \
                        f"year {year0 + y}, month {m}: row {r} is not snapshot row {row}"
        assert np.isnan(days[y, nt:]).all(), f"year {year0 + y}: a record past the year's last day"
    return seen


def day_values_loop(rec):
    """hybrid9_amd.day_values as a plain double loop over (nday, 7, n)."""
    rec = np.asarray(rec, F)
    out = np.array(rec, F)
    for r in (0, 1):
        for c in range(rec.shape[2]):
            prev = 0.0
            for d in range(rec.shape[0]):
                cur = float(rec[d, r, c])
                out[d, r, c] = F(cur - prev)
                prev = cur
    return out


def cell_order_days(*, zi, params, forcing, nisurf, year0, nyears, grow_on, chains=None):
    """The day records of the reference's own order: port.run_cell_order's loop
    restated (decade -> cell -> year, smp carried from cell to cell,
    HYBRID9.f90:93-130; as tests/monthly_helpers.cell_order_snapshots) with
    every per-cell port.run traced in full.  Returns (records (nyears, 366, 7,
    n), end state, annual); NaN for a masked cell."""
    L = params["theta_s"].shape[1]
    n = params["fmax"].size
    fo = np.ascontiguousarray(forcing, dtype=F)
    st = refcase.unpack_state(port.init_state(params, zi), n, L)
    st = {k: np.array(v, copy=True) for k, v in st.items()}
    ann = np.full((nyears, 12 + L, n), np.nan, dtype=F)
    rec = np.full((nyears, MAXD, ND, n), np.nan, dtype=F)
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
            rec[k0:k0 + ny, :, :, c] = records_from_trace(r["trace"], r["state"]["LAI"], L, nisurf, y0, ny)[..., 0]
            for k in st:
                st[k][c] = r["state"][k][0]
            ann[k0:k0 + ny, :, c] = r["annual"][:, :, 0]
        day0 += nd
    return rec, st, ann
