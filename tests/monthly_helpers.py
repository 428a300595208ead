"""Shared by tests/test_monthly_host.py and tests/test_gpu_monthly.py: the host
build of cell_year_pair with the Months policy (tests/csrc/host_monthly.cpp),
the month-end snapshots rebuilt from the oracle's per-substep trace, and the
year-end invariant that ties the twelfth snapshot to the annual means.

A snapshot (include/h9g.h, h9g_get_monthly) is the year's 12+L running sums
as they stand after a month's last day, undivided, in h9g_get_annual's row
order.  The trace determines rows rnf, tas..rhs, theta(1..L) and theta_total
(TRACE_ROWS); plant mass and NPP are not in it."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np

from hybrid9_amd import synth
from oracle import port, refcase
from tests.helpers import BUILD, ROOT

F = np.float32
NM = 12
R_NPP, R_PM, R_RNF, R_EVAP, R_TAS = 0, 1, 2, 3, 4

_lib = None


def trace_rows(L):
    """The snapshot rows the oracle's trace determines."""
    return [R_RNF] + list(range(R_TAS, R_TAS + 7)) + list(range(11, 12 + L))


def month_ends(jyear):
    """Last day (1-based) of each month, INIT.f90:844-859: restated here, not
    taken from the package."""
    leap = port._days(jyear) == 366
    return [31, 59 + leap, 90 + leap, 120 + leap, 151 + leap, 181 + leap, 212 + leap, 243 + leap, 273 + leap,
            304 + leap, 334 + leap, 365 + leap]


def monthly_lib():
    global _lib
    if _lib is None:
        src = ROOT / "tests" / "csrc" / "host_monthly.cpp"
        out = BUILD / "libhost_monthly.so"
        deps = [src] + list((ROOT / "hybrid9_amd" / "csrc").glob("*.h"))
        if not out.exists() or out.stat().st_mtime < max(d.stat().st_mtime for d in deps):
            BUILD.mkdir(exist_ok=True)
            subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp",
                            "-std=c++17", "-fPIC", "-shared", str(src), "-o", str(out)], check=True)
        _lib = C.CDLL(str(out))
        fp = C.POINTER(C.c_float)
        _lib.h9k_host_monthly.argtypes = [C.c_int] * 7 + [fp, fp, fp, fp, fp, fp, C.POINTER(C.c_int)]
        _lib.h9k_month_end.argtypes = [C.c_int, C.c_int]
    return _lib


def host_monthly(*, zi, params, forcing, nisurf, year0, nyears, grow_on, state0=None, const_geo=1):
    """cell_year_pair<..., Months> on the host for every cell: dict(rc, annual
    (nyears, 12+L, n), monthly (nyears, 12, 12+L, n), state (packed), err (n, 4));
    NaN for a masked cell, and from the year of its STOP on for a cell that stops."""
    L = params["theta_s"].shape[1]
    n = params["fmax"].size
    zi = np.ascontiguousarray(zi, F)
    pp = port.pack_params(params)
    fo = np.ascontiguousarray(forcing, F)
    st = port.init_state(params, zi) if state0 is None else np.array(state0, F)
    ann = np.full((nyears, 12 + L, n), np.nan, F)
    mon = np.full((nyears, NM, 12 + L, n), np.nan, F)
    err = np.zeros(4 * n, np.int32)
    fp = C.POINTER(C.c_float)
    rc = monthly_lib().h9k_host_monthly(n, L, nisurf, int(grow_on), year0, nyears, int(const_geo),
                                        zi.ctypes.data_as(fp), pp.ctypes.data_as(fp), fo.ctypes.data_as(fp),
                                        st.ctypes.data_as(fp), ann.ctypes.data_as(fp), mon.ctypes.data_as(fp),
                                        err.ctypes.data_as(C.POINTER(C.c_int)))
    return dict(rc=rc, annual=ann, monthly=mon, state=st, err=err.reshape(n, 4))


def l10_inputs(ncell=4):
    """Config-5 cells at L = 10, NS = 24: the 4 of test_host_focus_matches_port_l10_ns24,
    then further strided ones."""
    g = synth.land_cells(synth.NX025, synth.NY025, synth.NLAND025)[11::1601][:ncell]
    p = synth.make_params(g, 10)
    f = synth.make_forcing(g, synth.cell_lat(g, synth.NX025, synth.NY025), synth.year_day0(1903), 365)
    return dict(zi=synth.ZI_L10, params=p, forcing=f, nisurf=24, year0=1903, nyears=1, grow_on=1)


def snapshots_from_trace(trace, forcing, L, nisurf, year0, nyears):
    """Month-end snapshots (nyears, 12, 12+L, ncells) from the oracle's trace
    (ncells, ndays*nisurf, 3L+7; oracle.port.run(trace_cells=...)) and those
    cells' forcing (7, ndays, ncells): oracle/h9_oracle.c:730-742 restated in
    float32 -- day by day the seven forcing sums, then for i = 1..L
    theta_sum(i) += theta(i) and h2osoi_sum_total += h2o(i), from the day's
    last substep (theta at 2L+i, h2o at i), and the running rnf_sum (3L+4) as
    that substep left it.  Rows npp and plant_mass are NaN (not in the trace),
    row evap is +0."""
    return snapshots_from_last(day_last(trace, nisurf), forcing, L, year0, nyears)


def day_last(trace, nisurf):
    """The last substep of every day of a trace: (ncells, ndays, 3L+7)."""
    return trace[:, nisurf - 1::nisurf]


def snapshots_from_last(last, forcing, L, year0, nyears):
    """snapshots_from_trace from the days' last substeps (day_last)."""
    n = last.shape[0]
    fo = np.asarray(forcing, F)
    out = np.full((nyears, NM, 12 + L, n), np.nan, F)
    d0 = 0
    for y in range(nyears):
        nt = port._days(year0 + y)
        tr = last[:, d0:d0 + nt]
        ends = month_ends(year0 + y)
        fsum = np.zeros((7, n), F)
        theta_sum = np.zeros((L, n), F)
        h2o_total = np.zeros(n, F)
        m = 0
        for d in range(nt):
            fsum = (fsum + fo[:, d0 + d]).astype(F)
            for i in range(L):
                theta_sum[i] = (theta_sum[i] + tr[:, d, 2 * L + i]).astype(F)
                h2o_total = (h2o_total + tr[:, d, i]).astype(F)
            if d + 1 == ends[m]:
                s = out[y, m]
                s[R_RNF] = tr[:, d, 3 * L + 4]
                s[R_EVAP] = F(0.0)
                s[R_TAS:R_TAS + 7] = fsum
                s[11:11 + L] = theta_sum
                s[11 + L] = h2o_total
                m += 1
        assert m == NM
        d0 += nt
    return out


def annual_from_final(s11, jyear, nisurf):
    """The year's final sums (12+L, n) divided as HYBRID9.f90:263-290 divides
    them, in float32: the annual means."""
    nt = port._days(jyear)
    a = np.array(s11, F)
    a[R_PM] = a[R_PM] / F(nt)
    a[R_RNF] = a[R_RNF] / F(nt * nisurf)
    a[R_EVAP] = a[R_EVAP] / F(nt * nisurf)
    a[R_TAS:] = a[R_TAS:] / F(nt)
    return a


def check_year_end(monthly, annual, year0, nisurf):
    """The year-end invariant for monthly (nyears, 12, 12+L, n) against annual
    (nyears, 12+L, n): where a cell-year's annual means are finite, snapshot 11
    divided as :263-290 equals them bit for bit and row evap is +0 in all
    twelve months; where they are NaN, all twelve months are NaN."""
    from tests.conftest import same_bits
    monthly, annual = np.asarray(monthly), np.asarray(annual)
    assert monthly.shape[0] == annual.shape[0] and monthly.shape[1] == NM
    for y in range(annual.shape[0]):
        fin = np.isfinite(annual[y]).all(axis=0)
        nan = np.isnan(annual[y]).all(axis=0)      # masked, or stopped in or before this year
        ran = ~nan                                  # (golden `edge` has a cell whose sums of two rows are NaN
        #                                             without a STOP: it ran, and same_bits holds NaN to NaN)
        assert np.isnan(monthly[y][:, :, nan]).all(), f"year {year0 + y}: months of a NaN cell-year are not all NaN"
        assert np.isfinite(monthly[y][:, :, fin]).all(), f"year {year0 + y}: a NaN month in a finite cell-year"
        assert same_bits(annual_from_final(monthly[y, NM - 1][:, ran], year0 + y, nisurf), annual[y][:, ran]), \
            f"year {year0 + y}: snapshot 11 divided as :263-290 is not the annual means"
        ev = monthly[y][:, R_EVAP][:, ran]
        assert same_bits(ev, np.zeros_like(ev)), f"year {year0 + y}: row evap is not +0"


def port_snapshots(*, zi, params, forcing, nisurf, year0, nyears, grow_on, state0=None):
    """The oracle with every cell traced -> (snapshots from the trace, run)."""
    L = params["theta_s"].shape[1]
    n = params["fmax"].size
    s0 = None if state0 is None else refcase.unpack_state(np.asarray(state0, F), n, L)
    r = port.run(zi=zi, params=params, forcing=forcing, nisurf=nisurf, year0=year0, nyears=nyears,
                 grow_on=grow_on, state0=s0, trace_cells=tuple(range(n)), nthreads=8)
    return snapshots_from_trace(r["trace"], forcing, L, nisurf, year0, nyears), r


def cell_order_snapshots(*, zi, params, forcing, nisurf, year0, nyears, grow_on, chains=None):
    """The snapshots of the reference's own order: port.run_cell_order's loop
    restated (decade -> cell -> year, smp carried from cell to cell,
    HYBRID9.f90:93-130; as tests/daily_helpers.cell_order_daily8) with every
    per-cell port.run traced.  Returns (snapshots (nyears, 12, 12+L, n), end
    state, annual); the caller holds the end state to port.run_cell_order's."""
    L = params["theta_s"].shape[1]
    n = params["fmax"].size
    fo = np.ascontiguousarray(forcing, dtype=F)
    st = refcase.unpack_state(port.init_state(params, zi), n, L)
    st = {k: np.array(v, copy=True) for k, v in st.items()}
    ann = np.full((nyears, 12 + L, n), np.nan, dtype=F)
    snap = np.full((nyears, NM, 12 + L, n), np.nan, dtype=F)
    land = [c for c in range(n) if port._mask_sum(params["theta_s"][c]) > F(1.0e-8)]
    cid = np.zeros(n, np.int64) if chains is None else np.asarray(chains, np.int64)
    groups = [[c for c in land if cid[c] == r] for r in sorted(set(cid[land].tolist()))]
    day0 = 0
    for y0, ny in port.decades(year0, nyears):
        nd = sum(port._days(y0 + k) for k in range(ny))
        carry = {grp[0]: st["smp"][grp[-1]].copy() for grp in groups}
        prev = {b: a for grp in groups for a, b in zip(grp, grp[1:])}
        last = np.zeros((n, nd, 3 * L + 7), F)
        for c in land:
            s1 = {k: v[c:c + 1].copy() for k, v in st.items()}
            s1["smp"][0] = carry[c] if c in carry else st["smp"][prev[c]].copy()
            f1 = np.ascontiguousarray(fo[:, day0:day0 + nd, c:c + 1])
            r = port.run(zi=zi, params={k: v[c:c + 1] for k, v in params.items()}, forcing=f1, nisurf=nisurf,
                         year0=y0, nyears=ny, grow_on=grow_on, state0=s1, trace_cells=(0,))
            assert r["rc"] == 0
            k0 = y0 - year0
            last[c] = day_last(r["trace"], nisurf)[0]
            for k in st:
                st[k][c] = r["state"][k][0]
            ann[k0:k0 + ny, :, c] = r["annual"][:, :, 0]
        sn = snapshots_from_last(last[land], fo[:, day0:day0 + nd][:, :, land], L, y0, ny)
        snap[k0:k0 + ny][:, :, :, land] = sn
        day0 += nd
    return snap, st, ann
