"""hybrid9_amd -- MI355X-native HYBRID9 per-cell hydrology/vegetation hot path.

Python host mirror of the C-ABI in ``include/h9g.h`` (``lib/libh9g.so``,
built by ``hybrid9_amd.build``).  The reference has no Python surface: its
only "interface" is the driver loop ``HYBRID9.f90:120-295`` around the
argument-less ``SUBROUTINE HYDROLOGY``/``GROW``.  ``Context`` exposes that
loop one calendar year at a time, with the reference's array layouts and
STOP conditions (raised as :class:`ReferenceStop` carrying the first failing
cell, like the reference's diagnostics block ``HYDROLOGY.f90:1244-1274``).

There is no CPU fallback: if the HIP library is missing or cannot reach a
GPU, every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
LIB_PATH = HERE / "lib" / "libh9g.so"
if os.environ.get("H9G_LIB"):          # alternative build (e.g. the H9G_STAMPS profiling build)
    LIB_PATH = Path(os.environ["H9G_LIB"]).resolve()
NFORCING = 7
NANNUAL_SCALARS = 11
NDIAG = 12
NDAILY = 11              # H9G_NDAILY: the daily diagnostics line (site.DIAG_FIELDS)
NMONTHS = 12             # H9G_NMONTHS
NDAYREC = 7              # H9G_NDAYREC: the day record (DAY_FIELDS)
# The rows of a day record (Context.get_days); rnf_sum and evap_sum are the
# year's running sums (day_values differences them).
DAY_FIELDS = ("rnf_sum", "evap_sum", "soil_water", "theta1", "zwt", "wa", "LAI")
NDAYSTAT = 17            # H9G_NDAYSTAT: the day statistics (DAYSTAT_FIELDS)
# The rows of Context.get_daystats / day_stats, per cell and year.
DAYSTAT_FIELDS = ("ndays", "q_max", "q_max_day", "q7_min", "q_days", "e_max", "w_min", "w_min_day", "w_max",
                  "theta1_min", "dry_days", "dry_spell", "zwt_min", "wet_days", "lai_max", "lai_max_day",
                  "green_days")
# Thresholds of the counting rows where the caller names none: a runoff day has
# q >= q_thr (mm/day), a dry day theta(1) < theta_thr (mm3/mm3), a wet day
# zwt <= zwt_thr (mm), a green day LAI >= lai_thr.
DAYSTAT_THRESHOLDS = dict(q_thr=1.0, theta_thr=0.2, zwt_thr=1000.0, lai_thr=1.0)
ANNUAL_SCALARS = ("npp", "plant_mass", "rnf", "evap", "tas", "rlds", "rsds",
                  "huss", "ps", "pr", "rhs")
DIAG_NAMES = ("cells", "rnf_sum", "theta_total_sum", "zwt_sum", "wa_sum",
              "npp_sum", "plant_mass_sum", "lai_sum", "theta1_sum", "tas_sum",
              "pr_sum", "failed_cells")
STOP_MESSAGES = {  # HYDROLOGY.f90 STOP sites
    1: "Problem with tridiagonal 1.",            # :806-812
    2: "Problem with tridiagonal 2.",            # :818-825
    3: "rsub_top_tot is positive in drainage",   # :1068-1072
    4: "Problem in HYDROLOGY: Water imbalance > 0.1 mm",  # :1244-1274
    5: "internal: exact re-run requested with no day snapshot",   # H9G_ERR_NOSNAP (not a reference STOP)
}
LMAX = 10
MAX_SLOTS = 512          # H9G_MAX_SLOTS


class H9GError(RuntimeError):
    """API / HIP failure (negative return codes)."""


class ReferenceStop(RuntimeError):
    """A cell hit one of the reference's STOP conditions."""

    def __init__(self, err: dict):
        self.err = err
        msg = STOP_MESSAGES.get(err["code"], f"code {err['code']}")
        super().__init__(f"{msg} cell={err['cell']} year={err['year']} "
                         f"day={err['day']} substep={err['substep']} value={err['value']}")


class _Config(C.Structure):
    _fields_ = [("ncell", C.c_int32), ("nlayers", C.c_int32), ("nisurf", C.c_int32),
                ("grow_on", C.c_int32), ("max_days", C.c_int32), ("nslots", C.c_int32),
                ("zi", C.c_float * (LMAX + 2))]


class _Error(C.Structure):
    _fields_ = [("code", C.c_int32), ("cell", C.c_int32), ("year", C.c_int32),
                ("day", C.c_int32), ("substep", C.c_int32), ("value", C.c_float)]


class _SpinOpts(C.Structure):
    _fields_ = [("max_cycles", C.c_int32), ("min_cycles", C.c_int32), ("freeze", C.c_int32),
                ("reserved", C.c_int32), ("tol_water", C.c_double), ("tol_zwt", C.c_double),
                ("tol_plant", C.c_double)]


class _StatOpts(C.Structure):
    _fields_ = [("q_thr", C.c_float), ("theta_thr", C.c_float), ("zwt_thr", C.c_float), ("lai_thr", C.c_float),
                ("reserved", C.c_int32 * 4)]


def daystat_opts(**thresholds) -> _StatOpts:
    """The ``h9g_daystat_opts`` of Context.get_daystats: q_thr, theta_thr,
    zwt_thr, lai_thr (DAYSTAT_THRESHOLDS where not given), as float32."""
    bad = set(thresholds) - set(DAYSTAT_THRESHOLDS)
    if bad:
        raise TypeError(f"unknown day-statistics thresholds {sorted(bad)}: {sorted(DAYSTAT_THRESHOLDS)}")
    t = dict(DAYSTAT_THRESHOLDS, **thresholds)
    return _StatOpts(float(t["q_thr"]), float(t["theta_thr"]), float(t["zwt_thr"]), float(t["lai_thr"]))


NQUANT_MAX = 16          # H9G_NQUANT_MAX: quantiles of one Context.get_dayquant call
# The daily series Context.get_dayquant orders: the day's runoff and
# evapotranspiration (differences of the running sums, as day_stats' q and e)
# and rows 2..6 of the day record.
DAYQUANT_SERIES = ("q", "e", "soil_water", "theta1", "zwt", "wa", "LAI")


class _QuantOpts(C.Structure):
    _fields_ = [("series", C.c_int32), ("nq", C.c_int32), ("pooled", C.c_int32), ("reserved", C.c_int32),
                ("p", C.c_double * NQUANT_MAX)]


def dayquant_opts(*, series, p, pooled=False) -> _QuantOpts:
    """The ``h9g_dayquant_opts`` of Context.get_dayquant.  series: one of
    DAYQUANT_SERIES or its index; p: 1 .. 16 probabilities in [0, 1], in any
    order (hydrology's "Q95", the flow exceeded 95 % of the time, is p = 0.05)."""
    if isinstance(series, str):
        if series not in DAYQUANT_SERIES:
            raise ValueError(f"unknown day-quantile series {series!r}: {DAYQUANT_SERIES}")
        series = DAYQUANT_SERIES.index(series)
    p = np.atleast_1d(np.asarray(p, dtype=np.float64))
    if p.ndim != 1 or not 1 <= p.size <= NQUANT_MAX:
        raise ValueError(f"day quantiles: 1 .. {NQUANT_MAX} probabilities")
    o = _QuantOpts(int(series), int(p.size), int(pooled), 0)
    for i, v in enumerate(p):
        o.p[i] = float(v)
    return o


NSPIN = 6                # H9G_NSPIN: a cycle's history row
SPIN_HISTORY = ("cells_run", "settled", "stopped", "max_d_water", "max_d_zwt", "max_d_plant")


def spin_opts(*, max_cycles, min_cycles=1, tol_water=np.inf, tol_zwt=np.inf, tol_plant=np.inf,
              freeze=True) -> _SpinOpts:
    """The ``h9g_spinup_opts`` of Context.spinup."""
    return _SpinOpts(int(max_cycles), int(min_cycles), int(bool(freeze)), 0, float(tol_water), float(tol_zwt),
                     float(tol_plant))


_lib = None
_FP = C.POINTER(C.c_float)
_DP = C.POINTER(C.c_double)
_I64P = C.POINTER(C.c_int64)


def lib() -> C.CDLL:
    """Load libh9g.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise H9GError(f"{LIB_PATH} not built: run `python -m hybrid9_amd.build` "
                       "(or __graft_entry__.build())")
    L = C.CDLL(str(LIB_PATH))
    vp = C.c_void_p
    sig = {
        "h9g_abi_version": (C.c_int, []),
        "h9g_device_count": (C.c_int, []),
        "h9g_create": (vp, [C.POINTER(_Config), C.c_int]),
        "h9g_create_error": (C.c_char_p, []),
        "h9g_config_check": (C.c_int, [C.POINTER(_Config), C.c_char_p, C.c_int]),
        "h9g_config_bytes": (C.c_size_t, [C.POINTER(_Config)]),
        "h9g_destroy": (None, [vp]),
        "h9g_set_params": (C.c_int, [vp, _FP, _FP, _FP, _FP, _FP]),
        "h9g_init_state": (C.c_int, [vp]),
        "h9g_state_size": (C.c_int, [C.c_int]),
        "h9g_set_state": (C.c_int, [vp, _FP]),
        "h9g_get_state": (C.c_int, [vp, _FP]),
        "h9g_push_forcing": (C.c_int, [vp, C.c_int, C.c_int, _FP, C.c_int]),
        "h9g_push_forcing_device": (C.c_int, [vp, C.c_int, C.c_int, vp]),
        "h9g_forcing_slot": (vp, [vp, C.c_int]),
        "h9g_host_alloc": (vp, [C.c_size_t]),
        "h9g_host_free": (None, [vp]),
        "h9g_run_year": (C.c_int, [vp, C.c_int, C.c_int]),
        "h9g_run_decade_ordered": (C.c_int, [vp, C.POINTER(C.c_int32), C.c_int, C.c_int, _FP,
                                             C.POINTER(C.c_int32)]),
        "h9g_run_ordered": (C.c_int, [vp, C.POINTER(C.c_int32), C.c_int, C.c_int, _FP, C.POINTER(C.c_int32)]),
        "h9g_decade_stats": (C.c_int, [vp, C.POINTER(C.c_int64), C.c_int]),
        "h9g_ordered_stats": (C.c_int, [vp, C.POINTER(C.c_int64), C.c_int]),
        "h9g_launch_stats": (C.c_int, [vp, _DP, C.c_int, C.c_int]),
        "h9g_set_chains": (C.c_int, [vp, C.POINTER(C.c_int32)]),
        "h9g_sync": (C.c_int, [vp]),
        "h9g_last_error": (C.c_int, [vp, C.POINTER(_Error)]),
        "h9g_get_errors": (C.c_int, [vp, C.POINTER(C.c_int32)]),
        "h9g_get_annual": (C.c_int, [vp, _FP]),
        "h9g_get_diagnostics": (C.c_int, [vp, _DP, vp]),
        "h9g_get_diagnostics_async": (C.c_int, [vp, vp, vp]),
        "h9g_set_cells": (C.c_int, [vp, _I64P, _FP]),
        "h9g_synth_params": (C.c_int, [vp, C.c_uint64]),
        "h9g_synth_forcing": (C.c_int, [vp, C.c_int, C.c_uint64, C.c_int, C.c_int]),
        "h9g_last_kernel_ms": (C.c_float, [vp]),
        "h9g_total_kernel_ms": (C.c_double, [vp, C.c_int]),
        "h9g_kernel_name": (C.c_char_p, [vp]),
        "h9g_build_id": (C.c_char_p, []),
        "h9g_math_selftest": (C.c_int, [C.c_int, C.c_int, _FP, _FP, _FP]),
        "h9g_div_selftest": (C.c_int, [C.c_int, C.c_int, _FP, _FP, _FP, C.POINTER(C.c_int)]),
        "h9g_pace_probe": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_uint)]),
        "h9g_math_fast_selftest": (C.c_int, [C.c_int, C.c_int, _FP, _FP, _FP, C.POINTER(C.c_int)]),
        "h9g_synth_host": (C.c_int, [C.c_uint64, C.c_int, C.c_int, _I64P, _FP, C.c_int,
                                     C.c_int, _FP, _FP]),
        "h9g_land_cells": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_uint64, _I64P, _FP]),
        "h9g_write_axy_nc": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, _FP, C.c_int, _I64P, _FP]),
        "h9g_write_mxy_nc": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, _FP, C.c_int, _I64P, C.c_int, C.c_int,
                                       _FP]),
        "h9g_write_mxy_nc_evap": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, _FP, C.c_int, _I64P, C.c_int,
                                            C.c_int, _FP]),
        "h9g_nc_forcing_read": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, _I64P,
                                          C.c_int, C.c_int, _FP]),
        "h9g_nc_ntimes": (C.c_int, [C.c_char_p]),
        "h9g_nc_read_stats": (C.c_int, [C.POINTER(C.c_double), C.c_int]),
        "h9g_nc_forcing_prefetch": (C.c_int, [vp, C.c_int, C.POINTER(C.c_char_p), C.c_int, C.c_int,
                                              C.c_int, C.c_int]),
        "h9g_soil_layer": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int]),
        "h9g_soil_fmax": (C.c_int, [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int]),
        "h9g_last_soil_ms": (C.c_float, [vp]),
        "h9g_last_soil_slow": (C.c_int, [vp]),
        "h9g_get_params": (C.c_int, [vp, _FP, _FP, _FP, _FP, _FP]),
        "h9g_run_site": (C.c_int, [vp, C.c_int, _FP, _FP, _FP, _FP]),
        "h9g_set_daily": (C.c_int, [vp, C.c_int, C.POINTER(C.c_int32)]),
        "h9g_get_daily": (C.c_int, [vp, C.c_int, _FP]),
        "h9g_set_monthly": (C.c_int, [vp, C.c_int]),
        "h9g_set_evap": (C.c_int, [vp, C.c_int]),
        "h9g_get_monthly": (C.c_int, [vp, C.c_int, _FP]),
        "h9g_set_days": (C.c_int, [vp, C.c_int]),
        "h9g_get_days": (C.c_int, [vp, C.c_int, _FP]),
        "h9g_write_dxy_nc": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, _FP, C.c_int, _I64P, C.c_int, C.c_int,
                                       _FP]),
        "h9g_spinup": (C.c_int, [vp, C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(_SpinOpts),
                                 C.POINTER(C.c_int32), C.POINTER(C.c_int32), _DP]),
        "h9g_spin_selftest": (C.c_int, [C.c_int, C.c_int, C.c_int, _FP, _FP, C.POINTER(C.c_int32),
                                        C.POINTER(_SpinOpts), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                        _DP]),
        "h9g_get_daystats": (C.c_int, [vp, C.c_int, C.c_int, C.POINTER(_StatOpts), _DP]),
        "h9g_last_daystat_ms": (C.c_float, [vp]),
        "h9g_daystat_selftest": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _FP, C.POINTER(_StatOpts), _DP]),
        "h9g_write_sxy_nc": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, _I64P, C.c_int, C.POINTER(_StatOpts),
                                       _DP]),
        "h9g_get_dayquant": (C.c_int, [vp, C.c_int, C.c_int, C.POINTER(_QuantOpts), _DP]),
        "h9g_last_dayquant_ms": (C.c_float, [vp]),
        "h9g_dayquant_selftest": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, _FP,
                                            C.POINTER(_QuantOpts), _DP]),
        "h9g_write_qxy_nc": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, _I64P, C.c_int, C.c_int,
                                       C.POINTER(_QuantOpts), _DP]),
        "h9g_host_expf": (C.c_float, [C.c_float]),
        "h9g_host_powf": (C.c_float, [C.c_float, C.c_float]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    if L.h9g_abi_version() != 1:
        raise H9GError("libh9g ABI mismatch")
    _lib = L
    return L


def build_id() -> str:
    """Digest of the sources and flags the loaded libh9g.so was built from
    (hybrid9_amd/build.py build_id); needs no GPU."""
    return lib().h9g_build_id().decode()


def exported_symbols():
    """Names every C-ABI entry point declared in include/h9g.h."""
    import re
    hdr = (HERE.parent / "include" / "h9g.h").read_text()
    return sorted(set(re.findall(r"\b(h9g_[a-z_0-9]+)\s*\(", hdr)))


def _fp(a):
    return a.ctypes.data_as(_FP)


def _check(rc, what):
    if rc < 0:
        raise H9GError(f"{what} failed with {rc}")
    return rc


def days_in_year(y: int) -> int:
    """INIT.f90:844-859 calendar (Gregorian)."""
    if y % 4:
        return 365
    if y % 100:
        return 366
    if y % 400:
        return 365
    return 366


def state_size(L: int) -> int:
    return 4 * L + 9


def make_config(ncell: int, zi, *, nlayers: int = 8, nisurf: int = 48, grow_on: bool = True,
                max_days: int = 366, nslots: int = 2) -> _Config:
    """The ``h9g_config`` of a context, validated on the host by
    ``h9g_config_check`` (no GPU needed); raises ValueError with its reason."""
    zi = np.asarray(zi, dtype=np.float32)
    if zi.size != nlayers + 2:
        raise ValueError(f"zi must hold zi(0:L+1) = {nlayers + 2} values")
    cfg = _Config()
    cfg.ncell, cfg.nlayers, cfg.nisurf = int(ncell), int(nlayers), int(nisurf)
    cfg.grow_on, cfg.max_days, cfg.nslots = int(bool(grow_on)), int(max_days), int(nslots)
    for i, v in enumerate(zi):
        cfg.zi[i] = float(v)
    why = C.create_string_buffer(256)
    if lib().h9g_config_check(C.byref(cfg), why, 256):
        raise ValueError(f"invalid h9g_config: {why.value.decode()}")
    return cfg


def config_bytes(cfg: _Config) -> int:
    """Device bytes a context of ``cfg`` allocates (h9g_config_bytes)."""
    return int(lib().h9g_config_bytes(C.byref(cfg)))


def spin_selftest(state_prev, state, L: int, k: int, *, err=None, device: int = 0, **opts) -> dict:
    """One cycle's test of Context.spinup on hand-made packed states one cycle
    apart, through the same kernel (h9g_spin_selftest): dict(list (the cells
    still active, increasing), cell_cycle, stats (the history row))."""
    a = np.ascontiguousarray(state_prev, dtype=np.float32).ravel()
    b = np.ascontiguousarray(state, dtype=np.float32).ravel()
    n = a.size // state_size(L)
    assert a.size == b.size == n * state_size(L)
    i32 = C.POINTER(C.c_int32)
    e = None if err is None else np.ascontiguousarray(err, dtype=np.int32)
    lst, cc = np.full(n, -1, np.int32), np.zeros(n, np.int32)
    st = np.zeros(NSPIN + 1, np.float64)
    o = spin_opts(**opts)
    rc = lib().h9g_spin_selftest(int(device), n, int(L), _fp(a), _fp(b), None if e is None else e.ctypes.data_as(i32),
                                 C.byref(o), int(k), lst.ctypes.data_as(i32), cc.ctypes.data_as(i32),
                                 st.ctypes.data_as(_DP))
    _check(rc, "h9g_spin_selftest")
    return dict(list=lst[:int(st[NSPIN])].copy(), cell_cycle=cc, stats=st[:NSPIN].copy())


def daystat_selftest(records, *, nseg: int = 0, device: int = 0, **thresholds) -> np.ndarray:
    """Context.get_daystats on hand-made records (nday, 7, ncell), through the
    same kernel, with no context and no year run (h9g_daystat_selftest) ->
    (17, ncell) float64.  nseg = 0: the product's cut of the year into slices;
    nseg > 0: that many slices (1 .. 16) through the same code."""
    r = np.ascontiguousarray(records, dtype=np.float32)
    if r.ndim != 3 or r.shape[1] != NDAYREC:
        raise ValueError("daystat_selftest: records must be (nday, 7, ncell)")
    out = np.empty((NDAYSTAT, r.shape[2]), dtype=np.float64)
    o = daystat_opts(**thresholds)
    rc = lib().h9g_daystat_selftest(int(device), r.shape[2], r.shape[0], int(nseg), _fp(r), C.byref(o),
                                    out.ctypes.data_as(_DP))
    if rc == -1:
        raise ValueError("daystat_selftest: empty records, nseg outside 0 .. 16 or a NaN threshold")
    _check(rc, "h9g_daystat_selftest")
    return out


def _quant_years(records_by_year):
    """A list of years' records (nday_y, 7, ncell) -> (list of float32 arrays, ncell)."""
    yrs = [np.asarray(r, dtype=np.float32) for r in records_by_year]
    if not yrs or any(r.ndim != 3 or r.shape[1] != NDAYREC or r.shape[0] < 1 or r.shape[2] != yrs[0].shape[2]
                      for r in yrs):
        raise ValueError("day quantiles: a list of years' records, each (nday, 7, ncell)")
    return yrs, yrs[0].shape[2]


def dayquant_selftest(records_by_year, *, series, p, pooled=False, nseg: int = 0, device: int = 0) -> np.ndarray:
    """Context.get_dayquant on hand-made records, a list of years each (nday_y,
    7, ncell), through the same kernel, with no context and no year run
    (h9g_dayquant_selftest) -> (nres, 1 + 2 len(p), ncell) float64.  nseg = 0:
    the product's cut of a year into slices; nseg > 0: that many slices
    (1 .. 16) through the same code."""
    yrs, n = _quant_years(records_by_year)
    o = dayquant_opts(series=series, p=p, pooled=pooled)
    nt = np.array([r.shape[0] for r in yrs], dtype=np.int32)
    rec = np.full((len(yrs), int(nt.max()), NDAYREC, n), np.nan, dtype=np.float32)
    for y, r in enumerate(yrs):
        rec[y, :r.shape[0]] = r
    out = np.empty((1 if pooled else len(yrs), 1 + 2 * o.nq, n), dtype=np.float64)
    rc = lib().h9g_dayquant_selftest(int(device), n, len(yrs), nt.ctypes.data_as(C.POINTER(C.c_int32)), int(nseg),
                                     _fp(rec), C.byref(o), out.ctypes.data_as(_DP))
    if rc == -1:
        raise ValueError("dayquant_selftest: nseg outside 0 .. 16, more than 512 years, or options that "
                         "h9g_get_dayquant refuses (H9G_EINVAL)")
    _check(rc, "h9g_dayquant_selftest")
    return out


class Context:
    """One GPU, one shard of land cells (C-ABI ``h9g_ctx``)."""

    def __init__(self, ncell: int, zi, *, nlayers: int = 8, nisurf: int = 48,
                 grow_on: bool = True, max_days: int = 366, nslots: int = 2,
                 device: int = 0):
        lb = lib()
        zi = np.asarray(zi, dtype=np.float32)
        if zi.size != nlayers + 2:
            raise ValueError(f"zi must hold zi(0:L+1) = {nlayers + 2} values")
        cfg = make_config(ncell, zi, nlayers=nlayers, nisurf=nisurf, grow_on=grow_on,
                          max_days=max_days, nslots=nslots)
        self._lib = lb
        self.ncell, self.L, self.nisurf, self.grow_on = int(ncell), int(nlayers), int(nisurf), bool(grow_on)
        self.zi = zi
        self.device = device
        self._keep = {}
        self._h = lb.h9g_create(C.byref(cfg), int(device))
        if not self._h:
            why = (lb.h9g_create_error() or b"").decode() or "unknown"
            raise H9GError(f"h9g_create failed (ncell={ncell}, L={nlayers}, nslots={nslots}, "
                           f"device={device}): {why}")

    # -- lifetime ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.h9g_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- parameters & state -----------------------------------------------
    def set_params(self, params: dict):
        """params: theta_s, hksat, bsw, psi_s as (ncell, L); fmax (ncell)."""
        arrs = [np.ascontiguousarray(params[k], dtype=np.float32)
                for k in ("theta_s", "hksat", "bsw", "psi_s", "fmax")]
        for a in arrs[:4]:
            assert a.shape == (self.ncell, self.L), a.shape
        assert arrs[4].shape == (self.ncell,)
        _check(self._lib.h9g_set_params(self._h, *[_fp(a) for a in arrs]), "h9g_set_params")

    def get_params(self) -> dict:
        out = {k: np.empty((self.ncell, self.L), np.float32) for k in ("theta_s", "hksat", "bsw", "psi_s")}
        out["fmax"] = np.empty(self.ncell, np.float32)
        _check(self._lib.h9g_get_params(self._h, *[_fp(out[k]) for k in
                                                   ("theta_s", "hksat", "bsw", "psi_s", "fmax")]),
               "h9g_get_params")
        return out

    def soil_layer(self, layer: int, ts, ks, lm, ps, nx: int, ny: int):
        """INIT.f90:575-631 for one layer: 30" fields as (ny*60, nx*60) float32
        host arrays, or device pointers (ints, e.g. tensor.data_ptr())."""
        if all(isinstance(a, int) for a in (ts, ks, lm, ps)):
            ptrs, dev = [C.c_void_p(a) for a in (ts, ks, lm, ps)], 1
        else:
            arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in (ts, ks, lm, ps)]
            for a in arrs:
                assert a.shape == (ny * 60, nx * 60), a.shape
            ptrs, dev = [a.ctypes.data_as(C.c_void_p) for a in arrs], 0
        _check(self._lib.h9g_soil_layer(self._h, layer, *ptrs, nx, ny, dev), "h9g_soil_layer")
        return float(self._lib.h9g_last_soil_ms(self._h)), int(self._lib.h9g_last_soil_slow(self._h))

    def soil_fmax(self, soil_tex, fmax, nx: int, ny: int):
        """INIT.f90:661-680 (0.5 deg integer grids (ny, nx)); completes the parameters."""
        t = np.ascontiguousarray(soil_tex, dtype=np.int32)
        f = np.ascontiguousarray(fmax, dtype=np.int32)
        assert t.size == f.size == nx * ny
        i32 = C.POINTER(C.c_int32)
        _check(self._lib.h9g_soil_fmax(self._h, t.ctypes.data_as(i32), f.ctypes.data_as(i32), nx, ny),
               "h9g_soil_fmax")

    def init_state(self):
        _check(self._lib.h9g_init_state(self._h), "h9g_init_state")

    def set_state(self, packed: np.ndarray):
        packed = np.ascontiguousarray(packed, dtype=np.float32)
        assert packed.size == state_size(self.L) * self.ncell
        _check(self._lib.h9g_set_state(self._h, _fp(packed)), "h9g_set_state")

    def get_state(self) -> np.ndarray:
        out = np.empty(state_size(self.L) * self.ncell, dtype=np.float32)
        _check(self._lib.h9g_get_state(self._h, _fp(out)), "h9g_get_state")
        return out

    # -- forcing ----------------------------------------------------------
    def push_forcing(self, slot: int, forcing: np.ndarray, async_: bool = False):
        """forcing: (7, nday, ncell) float32 in READ_PGF order."""
        forcing = np.ascontiguousarray(forcing, dtype=np.float32)
        assert forcing.shape[0] == NFORCING and forcing.shape[2] == self.ncell, forcing.shape
        self._keep[slot] = forcing        # async copies read it after return
        _check(self._lib.h9g_push_forcing(self._h, slot, forcing.shape[1], _fp(forcing),
                                          int(async_)), "h9g_push_forcing")

    def nc_prefetch(self, slot: int, paths, nx: int, ny: int, t0: int, nt: int):
        """Async PGF prefetch from NetCDF files (READ_PGF.f90) into `slot`:
        days [t0, t0+nt) of the 7 files, needs set_cells."""
        _check(self._lib.h9g_nc_forcing_prefetch(self._h, slot, _paths(paths), nx, ny, t0, nt),
               "h9g_nc_forcing_prefetch")

    def push_forcing_device(self, slot: int, nday: int, dev_ptr: int):
        _check(self._lib.h9g_push_forcing_device(self._h, slot, nday, C.c_void_p(dev_ptr)),
               "h9g_push_forcing_device")

    def set_cells(self, gid, lat):
        gid = np.ascontiguousarray(gid, dtype=np.int64)
        lat = np.ascontiguousarray(lat, dtype=np.float32)
        assert gid.size == lat.size == self.ncell
        _check(self._lib.h9g_set_cells(self._h, gid.ctypes.data_as(_I64P), _fp(lat)),
               "h9g_set_cells")

    def synth_params(self, seed: int):
        _check(self._lib.h9g_synth_params(self._h, C.c_uint64(seed)), "h9g_synth_params")

    def synth_forcing(self, slot: int, seed: int, day0: int, nday: int):
        _check(self._lib.h9g_synth_forcing(self._h, slot, C.c_uint64(seed), day0, nday),
               "h9g_synth_forcing")

    # -- hot path ---------------------------------------------------------
    def run_year(self, slot: int, jyear: int):
        _check(self._lib.h9g_run_year(self._h, slot, jyear), "h9g_run_year")
        self.daily_years = [jyear]

    def run_decade_ordered(self, slots, jyear0: int, raise_on_stop: bool = True, annual: bool = True):
        """One decade of the reference's own cell order (h9g_run_decade_ordered:
        smp carried from cell to cell, HYBRID9.f90:93-130); synchronous.
        Returns (annual (nyears, 12+L, ncell) or None, passes);
        self.decade_rc holds the STOP code."""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        out = np.empty((sl.size, 12 + self.L, self.ncell), dtype=np.float32) if annual else None
        np_ = C.c_int32(0)
        self.daily_years = [jyear0 + k for k in range(sl.size)]
        rc = _check(self._lib.h9g_run_decade_ordered(self._h, sl.ctypes.data_as(C.POINTER(C.c_int32)), jyear0,
                                                     sl.size, _fp(out) if annual else None, C.byref(np_)),
                    "h9g_run_decade_ordered")
        self.decade_rc = rc
        if rc and raise_on_stop:
            raise ReferenceStop(self.last_error())
        return out, int(np_.value)

    def run_ordered(self, slots, jyear0: int, raise_on_stop: bool = True, annual: bool = True):
        """Years jyear0 .. jyear0+len(slots)-1 in the reference's own cell
        order, cut into its decades, which overlap on the device
        (h9g_run_ordered; bit-identical to run_decade_ordered per decade);
        synchronous.  Every year's slot must stay resident for the call.
        Returns (annual (nyears, 12+L, ncell) or None, passes per decade);
        self.decade_rc holds the STOP code."""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        out = np.empty((sl.size, 12 + self.L, self.ncell), dtype=np.float32) if annual else None
        np_ = (C.c_int32 * max(1, len(decades(jyear0, sl.size))))()
        self.daily_years = [jyear0 + k for k in range(sl.size)]
        rc = _check(self._lib.h9g_run_ordered(self._h, sl.ctypes.data_as(C.POINTER(C.c_int32)), jyear0, sl.size,
                                              _fp(out) if annual else None, np_), "h9g_run_ordered")
        self.decade_rc = rc
        if rc and raise_on_stop:
            raise ReferenceStop(self.last_error())
        return out, [int(v) for v in np_][:len(decades(jyear0, sl.size))]

    def spinup(self, slots, jyear0: int, *, max_cycles: int, min_cycles: int = 1, tol_water=np.inf,
               tol_zwt=np.inf, tol_plant=np.inf, freeze: bool = True, raise_on_stop: bool = True) -> dict:
        """Spin-up to equilibrium (h9g_spinup): repeats years jyear0 ..
        jyear0+len(slots)-1 (isolated cells, the forcing of year jyear0+k
        resident in slots[k]) and tests every cell after each cycle against
        its own state one cycle earlier: a cell settles once its column water
        (mm), water table (mm) and relative plant-mass drifts are within the
        tolerances (inf: criterion off; 0: a bit-exact fixed point).  freeze:
        a settled cell leaves the later cycles (bit-exact for the others, cells
        being independent); else every cell runs every cycle.  Synchronous.
        Returns dict(cycles, cell_cycle (ncell int32: k > 0 settled at cycle k,
        0 still active, -1 masked or stopped before, -2 stopped during the
        call), history (cycles, 6: SPIN_HISTORY), rc (the STOP code))."""
        sl = np.ascontiguousarray(slots, dtype=np.int32).ravel()
        opts = spin_opts(max_cycles=max_cycles, min_cycles=min_cycles, tol_water=tol_water, tol_zwt=tol_zwt,
                         tol_plant=tol_plant, freeze=freeze)
        cyc = C.c_int32(0)
        cc = np.zeros(self.ncell, dtype=np.int32)
        hist = np.zeros((max(int(max_cycles), 1), NSPIN), dtype=np.float64)
        i32 = C.POINTER(C.c_int32)
        rc = self._lib.h9g_spinup(self._h, sl.ctypes.data_as(i32), int(jyear0), int(sl.size), C.byref(opts),
                                  C.byref(cyc), cc.ctypes.data_as(i32), hist.ctypes.data_as(_DP))
        if rc == -1:
            raise ValueError("spinup: bad slots (distinct, resident, one per year), years or options")
        if rc == -4:
            raise H9GError("h9g_spinup: H9G_ESTATE: spin-up records nothing (turn daily, monthly and day "
                           "recording off) and needs parameters and a state")
        _check(rc, "h9g_spinup")
        if rc and raise_on_stop:
            raise ReferenceStop(self.last_error())
        return dict(cycles=int(cyc.value), cell_cycle=cc, history=hist[:cyc.value].copy(), rc=rc)

    def ordered_stats(self) -> dict:
        """How the last ordered call overlapped its decades (h9g_ordered_stats)."""
        out = (C.c_int64 * 64)()
        m = _check(self._lib.h9g_ordered_stats(self._h, out, 64), "h9g_ordered_stats")
        keys = ("decades", "first_pass_launches", "rerun_years_riding", "rerun_cell_years_riding",
                "rerun_years_alone", "rerun_cell_years_alone", "cells_left_out_of_first_pass",
                "probed", "probe_kept")
        d = {k: int(out[i]) for i, k in enumerate(keys)}
        d["passes"] = [int(out[i]) for i in range(len(keys), m)]
        return d

    def launch_stats(self, reset: bool = False) -> dict:
        """Year launches per kernel kind since the last reset
        (h9g_launch_stats): launches, cell-years, device ms."""
        out = (C.c_double * 21)()
        m = _check(self._lib.h9g_launch_stats(self._h, out, 21, int(reset)), "h9g_launch_stats")
        names = ("pair", "solo", "mixed", "pair2", "pair11", "pair1", "probe")
        return {nm: dict(launches=int(out[3 * i]), cell_years=int(out[3 * i + 1]), ms=float(out[3 * i + 2]))
                for i, nm in enumerate(names) if 3 * i + 2 < m and out[3 * i] > 0}

    def set_chains(self, chain=None):
        """Independent cell-order chains, one per reference rank
        (h9g_set_chains; shard.reference_blocks gives the reference's).
        None: one chain."""
        if chain is None:
            _check(self._lib.h9g_set_chains(self._h, None), "h9g_set_chains")
            return
        ch = np.ascontiguousarray(chain, dtype=np.int32)
        assert ch.size == self.ncell
        _check(self._lib.h9g_set_chains(self._h, ch.ctypes.data_as(C.POINTER(C.c_int32))), "h9g_set_chains")

    def decade_stats(self) -> dict:
        """Work of the last run_decade_ordered (h9g_decade_stats)."""
        out = (C.c_int64 * 64)()
        m = _check(self._lib.h9g_decade_stats(self._h, out, 64), "h9g_decade_stats")
        return dict(passes=int(out[0]), rerun_cells=int(out[1]), rerun_cell_years=int(out[2]),
                    rerun_launches=int(out[3]), launch_cells=[int(out[i]) for i in range(4, m)])

    def run_site(self, sub, daily, lai, raise_on_stop: bool = True) -> np.ndarray:
        """LCLIM site path (HYBRID9.f90:339-480) over nday days, synchronous.

        sub (nday*nisurf, 5, ncell): tak (degC), rh, Rnet, PAR, ppt (mm per
        substep); daily (nday, 2, ncell): huss, ps; lai (nday, 3, ncell):
        (LAI, a, b), NaN = unchanged.  Returns the daily diagnostics
        (nday, 11, ncell), site.DIAG_FIELDS (NaN for masked/failed cells)."""
        daily = np.ascontiguousarray(daily, dtype=np.float32)
        nday = daily.shape[0]
        sub = np.ascontiguousarray(sub, dtype=np.float32)
        lai = np.ascontiguousarray(lai, dtype=np.float32)
        if (sub.shape != (nday * self.nisurf, 5, self.ncell) or daily.shape != (nday, 2, self.ncell)
                or lai.shape != (nday, 3, self.ncell)):
            raise ValueError("run_site: shapes must be sub (nday*nisurf, 5, ncell), "
                             "daily (nday, 2, ncell), lai (nday, 3, ncell)")
        out = np.empty((nday, 11, self.ncell), dtype=np.float32)
        rc = _check(self._lib.h9g_run_site(self._h, nday, _fp(sub), _fp(daily), _fp(lai), _fp(out)),
                    "h9g_run_site")
        if rc and raise_on_stop:
            raise ReferenceStop(self.last_error())
        self.site_rc = rc
        return out

    # -- daily diagnostics of selected cells ------------------------------
    def set_daily(self, cells=()):
        """Selects the cells (context indices, strictly increasing) whose
        daily line (HYBRID9.f90:221-229, site.DIAG_FIELDS) the next run_year,
        run_decade_ordered or run_ordered records (h9g_set_daily); an empty
        list turns it off.  The year kernels are untouched: the selected
        cells are run once more by a small shadow kernel."""
        c = np.ascontiguousarray(cells if cells is not None else (), dtype=np.int32).ravel()
        rc = self._lib.h9g_set_daily(self._h, int(c.size), c.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc == -1:
            raise ValueError("set_daily: cells must be strictly increasing context indices in [0, ncell)")
        _check(rc, "h9g_set_daily")
        self._nsel = int(c.size)
        self._daily_days = []

    def get_daily(self, k: int = 0) -> np.ndarray:
        """The daily lines of year k (0-based) of the last run_year (k = 0)
        or ordered call: (ndays, 11, nsel), selection order (h9g_get_daily).
        The year is the k-th of that call (``daily_years`` names them)."""
        years = getattr(self, "daily_years", [])
        nsel = getattr(self, "_nsel", 0)
        nt = days_in_year(years[k]) if 0 <= k < len(years) else 366
        out = np.empty((nt, NDAILY, max(nsel, 1)), dtype=np.float32)
        rc = self._lib.h9g_get_daily(self._h, int(k), _fp(out))
        if rc == -4:
            raise H9GError("h9g_get_daily: nothing recorded (H9G_ESTATE): select cells with set_daily, then run")
        _check(rc, "h9g_get_daily")
        return out[:, :, :nsel]

    # -- monthly output: month-end running sums ---------------------------
    def set_monthly(self, on: bool = True):
        """Turns monthly recording on or off (h9g_set_monthly; off by
        default).  With it on, the next run_year, run_decade_ordered or
        run_ordered runs the monthly year kernels, which also store the
        year's 12+L running sums at every month end; annual means, state,
        STOP records and daily lines are the same bit for bit either way."""
        _check(self._lib.h9g_set_monthly(self._h, int(bool(on))), "h9g_set_monthly")

    def set_evap(self, on: bool = True):
        """Turns evapotranspiration recording on or off (h9g_set_evap; off by
        default).  With it on every year launch runs the ET year kernels, and
        row evap (3) of the annual means and of the month-end snapshots is the
        year's evaporation sum, sum over the substeps of (qflx_evap_grnd +
        qflx_tran_veg_col) * dt in float32, in mm: divided by nt * nisurf in
        the annual means like row rnf, as it stands in a snapshot.  Every
        other row, the state, the STOP records and the daily lines are the
        same bits either way."""
        _check(self._lib.h9g_set_evap(self._h, int(bool(on))), "h9g_set_evap")

    def get_monthly(self, k: int = 0) -> np.ndarray:
        """The month-end snapshots of year k (0-based) of the last run_year
        (k = 0) or ordered call: (12, 12+L, ncell) float32, the undivided
        running sums in get_annual's row order (h9g_get_monthly; NaN for a
        cell that stopped or is masked).  ``monthly_means`` derives the
        months' means from them."""
        out = np.empty((NMONTHS, 12 + self.L, self.ncell), dtype=np.float32)
        rc = self._lib.h9g_get_monthly(self._h, int(k), _fp(out))
        if rc == -4:
            raise H9GError("h9g_get_monthly: nothing recorded (H9G_ESTATE): set_monthly(), then run")
        _check(rc, "h9g_get_monthly")
        return out

    # -- day records: day-end records of every cell -------------------------
    def set_days(self, on: bool = True):
        """Turns day recording on or off (h9g_set_days; off by default).  It
        rides on evapotranspiration recording: set_evap() first (H9G_ESTATE
        otherwise, and from set_evap(False) while it is on).  With it on every
        year launch runs the day year kernels, which also store NDAYREC values
        per cell and day (DAY_FIELDS); annual means, month-end snapshots,
        state, STOP records and daily lines are the bits of an ET run."""
        rc = self._lib.h9g_set_days(self._h, int(bool(on)))
        if rc == -4:
            raise H9GError("h9g_set_days: H9G_ESTATE: day recording needs set_evap() first")
        _check(rc, "h9g_set_days")

    def get_days(self, k: int = 0) -> np.ndarray:
        """The day records of year k (0-based) of the last run_year (k = 0)
        or ordered call: (nday_k, 7, ncell) float32 in DAY_FIELDS' order
        (h9g_get_days; NaN from a cell's STOP day on and for a masked cell).
        ``day_values`` turns the two running sums into the days' amounts."""
        years = getattr(self, "daily_years", [])
        nt = days_in_year(years[k]) if 0 <= k < len(years) else 366
        out = np.empty((nt, NDAYREC, self.ncell), dtype=np.float32)
        rc = self._lib.h9g_get_days(self._h, int(k), _fp(out))
        if rc == -4:
            raise H9GError("h9g_get_days: nothing recorded (H9G_ESTATE): set_evap(), set_days(), then run")
        _check(rc, "h9g_get_days")
        return out

    # -- day statistics: per-cell annual indices from the day records --------
    def get_daystats(self, k0: int = 0, nk: int = 1, **thresholds) -> np.ndarray:
        """The day statistics of years k0 .. k0+nk-1 (0-based) of the last
        run_year (k0 = 0, nk = 1) or ordered call that recorded days: (nk, 17,
        ncell) float64 in DAYSTAT_FIELDS' order, reduced on the device from the
        day records where they lie (h9g_get_daystats; ``day_stats`` states the
        definition).  thresholds: q_thr, theta_thr, zwt_thr, lai_thr
        (DAYSTAT_THRESHOLDS).  Synchronises, as get_days does."""
        o = daystat_opts(**thresholds)
        out = np.empty((max(int(nk), 1), NDAYSTAT, self.ncell), dtype=np.float64)
        rc = self._lib.h9g_get_daystats(self._h, int(k0), int(nk), C.byref(o), out.ctypes.data_as(_DP))
        if rc == -4:
            raise H9GError("h9g_get_daystats: nothing recorded (H9G_ESTATE): set_evap(), set_days(), then run")
        if rc == -1:
            raise ValueError("get_daystats: years outside those the last call recorded, or a NaN threshold "
                             "(H9G_EINVAL)")
        _check(rc, "h9g_get_daystats")
        return out

    def last_daystat_ms(self) -> float:
        """Device time of the last get_daystats' launches (h9g_last_daystat_ms)."""
        return float(self._lib.h9g_last_daystat_ms(self._h))

    def get_dayquant(self, k0: int = 0, nk: int = 1, *, series, p, pooled: bool = False) -> np.ndarray:
        """Order statistics of one daily series (DAYQUANT_SERIES) of years k0 ..
        k0+nk-1 of what the last run_year (k0 = 0, nk = 1), run_decade_ordered
        or run_ordered call recorded -> (nk, or 1 when pooled, 1 + 2 len(p),
        ncell) float64: row 0 the number m of days that count, rows 1 + 2i and
        2 + 2i the order statistics x_(j) and x_(min(j+1, m-1)) around p[i], j
        = floor(p[i] (m - 1)); selected on the device from the day records where
        they lie (h9g_get_dayquant; ``day_order_stats`` states the same in
        numpy, bit for bit; ``day_quantiles`` interpolates).  pooled: one
        result over all days of the span's years.  Synchronises, as get_days does."""
        o = dayquant_opts(series=series, p=p, pooled=pooled)
        out = np.empty((1 if pooled else max(int(nk), 1), 1 + 2 * o.nq, self.ncell), dtype=np.float64)
        rc = self._lib.h9g_get_dayquant(self._h, int(k0), int(nk), C.byref(o), out.ctypes.data_as(_DP))
        if rc == -4:
            raise H9GError("h9g_get_dayquant: nothing recorded (H9G_ESTATE): set_evap(), set_days(), then run")
        if rc == -1:
            raise ValueError("get_dayquant: years outside those the last call recorded, a series outside 0 .. 6 or "
                             "a probability outside [0, 1] (H9G_EINVAL)")
        _check(rc, "h9g_get_dayquant")
        return out

    def last_dayquant_ms(self) -> float:
        """Device time of the last get_dayquant's launches (h9g_last_dayquant_ms)."""
        return float(self._lib.h9g_last_dayquant_ms(self._h))

    def sync(self, raise_on_stop: bool = True) -> int:
        rc = _check(self._lib.h9g_sync(self._h), "h9g_sync")
        if rc and raise_on_stop:
            raise ReferenceStop(self.last_error())
        return rc

    def last_error(self) -> dict:
        e = _Error()
        _check(self._lib.h9g_last_error(self._h, C.byref(e)), "h9g_last_error")
        return dict(code=e.code, cell=e.cell, year=e.year, day=e.day, substep=e.substep,
                    value=e.value)

    def get_errors(self) -> dict:
        """Every cell's STOP record: code (0: none), day, substep, value."""
        rec = np.empty((4, self.ncell), dtype=np.int32)
        _check(self._lib.h9g_get_errors(self._h, rec.ctypes.data_as(C.POINTER(C.c_int32))), "h9g_get_errors")
        return dict(code=rec[0].copy(), day=rec[1].copy(), substep=rec[2].copy(),
                    value=rec[3].view(np.float32).copy())

    def get_annual(self) -> np.ndarray:
        out = np.empty((12 + self.L, self.ncell), dtype=np.float32)
        _check(self._lib.h9g_get_annual(self._h, _fp(out)), "h9g_get_annual")
        return out

    def get_diagnostics(self, dev_ptr: int | None = None) -> np.ndarray:
        out = np.empty(NDIAG, dtype=np.float64)
        _check(self._lib.h9g_get_diagnostics(self._h, out.ctypes.data_as(_DP),
                                             C.c_void_p(dev_ptr) if dev_ptr else None),
               "h9g_get_diagnostics")
        return out

    def diagnostics_async(self, dev_ptr: int, stream: int | None):
        """Copy the diagnostics into device buffer dev_ptr, ordered on the
        hipStream_t `stream` (e.g. torch's current stream before an RCCL
        all-reduce) with no host synchronisation."""
        _check(self._lib.h9g_get_diagnostics_async(self._h, C.c_void_p(dev_ptr),
                                                   C.c_void_p(stream) if stream else None),
               "h9g_get_diagnostics_async")

    def last_kernel_ms(self) -> float:
        return float(self._lib.h9g_last_kernel_ms(self._h))

    def total_kernel_ms(self, reset: bool = False) -> float:
        return float(self._lib.h9g_total_kernel_ms(self._h, int(reset)))

    def kernel_name(self) -> str:
        return self._lib.h9g_kernel_name(self._h).decode()

    def kind_id(self) -> int:
        """The context's year kernel as h9g_launch_stats numbers it: 1 pair,
        2 solo, 3 solo rounds + pair, 4 pair2, 5 pair11, 6 pair1."""
        name = self.kernel_name()
        if "+" in name:
            return 3
        for prefix, k in (("h9g_solo_", 2), ("h9g_pair2_", 4), ("h9g_pair11_", 5), ("h9g_pair1_", 6)):
            if name.startswith(prefix):
                return k
        return 1


PGF_VARS = ("tas", "rlds", "rsds", "huss", "ps", "pr", "rhs")   # READ_PGF.f90 order


def _paths(paths):
    paths = [str(p).encode() for p in paths]
    if len(paths) != NFORCING:
        raise ValueError("need the 7 PGF files in READ_PGF order " + " ".join(PGF_VARS))
    return (C.c_char_p * NFORCING)(*paths)


def pgf_paths(directory, decade: str, suffix: str = "nc4"):
    """READ_PGF.f90:22-106 file names: <var>_pgfv2.1_<decade>.<suffix>."""
    return [str(Path(directory) / f"{v}_pgfv2.1_{decade}.{suffix}") for v in PGF_VARS]


def nc_ntimes(path) -> int:
    """NTIMES of a PGF file (its 'time' dimension, READ_NET_CDF_0D.f90)."""
    return _check(lib().h9g_nc_ntimes(str(path).encode()), "h9g_nc_ntimes")


IO_STATS = ("wall_s", "setup_s", "threads", "jobs", "pread_s", "inflate_s", "gather_s", "other_s",
            "bytes_read", "bytes_decoded", "values", "pool_wall_s")


def nc_read_stats() -> dict:
    """Stage profile of the last forcing read (h9g_nc_read_stats): wall and
    setup seconds, then thread-seconds per stage summed over the pool."""
    out = (C.c_double * len(IO_STATS))()
    m = _check(lib().h9g_nc_read_stats(out, len(IO_STATS)), "h9g_nc_read_stats")
    return {k: float(out[i]) for i, k in enumerate(IO_STATS[:m])}


def nc_forcing_read(paths, nx: int, ny: int, gid, t0: int, nt: int) -> np.ndarray:
    """Days [t0, t0+nt) of the 7 PGF files at grid ids gid -> (7, nt, ncell)."""
    gid = np.ascontiguousarray(gid, dtype=np.int64)
    out = np.empty((NFORCING, nt, gid.size), dtype=np.float32)
    _check(lib().h9g_nc_forcing_read(_paths(paths), nx, ny, gid.size, gid.ctypes.data_as(_I64P), t0, nt,
                                     _fp(out)), "h9g_nc_forcing_read")
    return out


def write_axy_nc(path, annual, gid, zc, nx: int = 720, ny: int = 360):
    """WRITE_NET_CDF_3DR.f90: one year of annual means (12+L, ncell) of the
    cells gid to axyYYYY.nc (netCDF classic, the reference's schema)."""
    annual = np.ascontiguousarray(annual, dtype=np.float32)
    gid = np.ascontiguousarray(gid, dtype=np.int64)
    zc = np.ascontiguousarray(zc, dtype=np.float32)
    L = annual.shape[0] - 12
    assert annual.shape[1] == gid.size and zc.size == L
    _check(lib().h9g_write_axy_nc(str(path).encode(), nx, ny, L, _fp(zc), gid.size,
                                  gid.ctypes.data_as(_I64P), _fp(annual)), "h9g_write_axy_nc")


def write_mxy_nc(path, snapshots, gid, zc, jyear: int, nisurf: int, nx: int = 720, ny: int = 360, evap=False):
    """One year of monthly means, derived as ``monthly_means`` derives them
    from the month-end snapshots (12, 12+L, ncell) of the cells gid, to
    mxyYYYY.nc: write_axy_nc's variables under a leading dimension month
    (h9g_write_mxy_nc; netCDF classic).  evap: the snapshots of an ET run
    (Context.set_evap), row evap divided like row rnf (h9g_write_mxy_nc_evap)."""
    snapshots = np.ascontiguousarray(snapshots, dtype=np.float32)
    gid = np.ascontiguousarray(gid, dtype=np.int64)
    zc = np.ascontiguousarray(zc, dtype=np.float32)
    L = snapshots.shape[1] - 12
    assert snapshots.shape == (NMONTHS, 12 + L, gid.size) and zc.size == L
    name = "h9g_write_mxy_nc_evap" if evap else "h9g_write_mxy_nc"
    _check(getattr(lib(), name)(str(path).encode(), nx, ny, L, _fp(zc), gid.size, gid.ctypes.data_as(_I64P),
                                int(jyear), int(nisurf), _fp(snapshots)), name)


def day_values(records) -> np.ndarray:
    """A year's day records (nday, 7, ncell) (Context.get_days) with the two
    running sums turned into the days' amounts: rows 0 (runoff) and 1
    (evapotranspiration) become, in float64, S[d] - S[d-1] with S[-1] = 0,
    rounded to float32, in mm per day; rows 2..6 are unchanged.  Derived from
    the reference's f32 running sums: deterministic, but not a reference
    quantity.  NaN days (a STOP, a masked cell) stay NaN."""
    r = np.asarray(records, dtype=np.float32)
    if r.ndim != 3 or r.shape[1] != NDAYREC:
        raise ValueError("day_values: records must be (nday, 7, ncell)")
    out = np.array(r, dtype=np.float32)
    s = r[:, :2].astype(np.float64)
    out[:, :2] = np.diff(s, axis=0, prepend=np.zeros_like(s[:1])).astype(np.float32)
    return out


def _first_extreme(v, largest: bool):
    """Per column of v (nday, n): the largest (smallest) value that is not NaN
    and the row of its first occurrence, as float64; (NaN, -1) with none."""
    n = v.shape[1]
    if v.shape[0] == 0:
        return np.full(n, np.nan), np.full(n, -1.0)
    ok = ~np.isnan(v)
    key = np.where(ok, v, -np.inf if largest else np.inf)
    i = key.argmax(axis=0) if largest else key.argmin(axis=0)     # (the first of equal values; -0 == +0)
    # (every candidate an infinity of the padding's sign: the first candidate)
    i = np.where(np.take_along_axis(ok, i[None], axis=0)[0], i, ok.argmax(axis=0))
    some = ok.any(axis=0)
    val = np.take_along_axis(v, i[None], axis=0)[0].astype(np.float64)
    return np.where(some, val, np.nan), np.where(some, i, -1).astype(np.float64)


def day_stats(records, **thresholds) -> np.ndarray:
    """One year's day statistics from its day records (nday, 7, ncell)
    (Context.get_days) -> (17, ncell) float64 in DAYSTAT_FIELDS' order: the
    numpy statement of what Context.get_daystats computes on the device, bit
    for bit.  With R the records, S = R[:, 0] in float64 and S[-1] = 0:
    q[d] = S[d] - S[d-1] (the day's runoff, day_values' difference before its
    rounding), e[d] the same from row 1, q7[d] = S[d] - S[d-7] for d >= 6.

        ndays                  days none of whose seven values is NaN
        q_max, q_max_day       largest q; 0-based day of its first occurrence
        q7_min                 smallest q7
        q_days                 days with q >= q_thr (in float64)
        e_max                  largest e
        w_min, w_min_day       smallest soil_water (row 2); first day
        w_max                  largest soil_water
        theta1_min             smallest theta1 (row 3)
        dry_days               days with theta1 < theta_thr (in float32)
        dry_spell              longest run of consecutive dry days
        zwt_min                smallest zwt (row 4)
        wet_days               days with zwt <= zwt_thr
        lai_max, lai_max_day   largest LAI (row 6); first day
        green_days             days with LAI >= lai_thr

    A NaN is never a candidate and never counted (a STOP day and later, a
    masked cell), and ends a dry run; with no candidate an extreme is NaN and
    its day -1.  Of equal extremes the first day is kept.  thresholds: q_thr,
    theta_thr, zwt_thr, lai_thr (DAYSTAT_THRESHOLDS), taken as float32.
    Derived from the reference's f32 running sums: deterministic, but not a
    reference quantity."""
    r = np.asarray(records, dtype=np.float32)
    if r.ndim != 3 or r.shape[1] != NDAYREC:
        raise ValueError("day_stats: records must be (nday, 7, ncell)")
    o = daystat_opts(**thresholds)
    nt, _, n = r.shape
    s = r[:, :2].astype(np.float64)
    d = np.diff(s, axis=0, prepend=np.zeros_like(s[:1]))
    q, e = d[:, 0], d[:, 1]
    before = np.concatenate([np.zeros((1, n)), s[:-7, 0]]) if nt >= 7 else np.zeros((0, n))
    q7 = s[6:, 0] - before
    out = np.empty((NDAYSTAT, n), dtype=np.float64)
    out[0] = (~np.isnan(r).any(axis=1)).sum(axis=0)
    out[1], out[2] = _first_extreme(q, True)
    out[3] = _first_extreme(q7, False)[0]
    out[4] = (q >= np.float64(np.float32(o.q_thr))).sum(axis=0)
    out[5] = _first_extreme(e, True)[0]
    out[6], out[7] = _first_extreme(r[:, 2], False)
    out[8] = _first_extreme(r[:, 2], True)[0]
    out[9] = _first_extreme(r[:, 3], False)[0]
    dry = r[:, 3] < np.float32(o.theta_thr)
    out[10] = dry.sum(axis=0)
    day1 = np.arange(1, nt + 1)[:, None]
    run = np.where(dry, day1 - np.maximum.accumulate(np.where(dry, 0, day1), axis=0), 0)
    out[11] = run.max(axis=0)
    out[12] = _first_extreme(r[:, 4], False)[0]
    out[13] = (r[:, 4] <= np.float32(o.zwt_thr)).sum(axis=0)
    out[14], out[15] = _first_extreme(r[:, 6], True)
    out[16] = (r[:, 6] >= np.float32(o.lai_thr)).sum(axis=0)
    return out


def write_sxy_nc(path, stats, gid, jyear: int, nx: int = 720, ny: int = 360, **thresholds):
    """One year of day statistics (17, ncell) float64 (Context.get_daystats,
    day_stats) of the cells gid to sxyYYYY.nc: 17 float64 variables named as
    DAYSTAT_FIELDS on write_axy_nc's latitude / longitude grid, NaN fill, the
    thresholds they were taken with as global attributes (h9g_write_sxy_nc;
    netCDF classic, 64-bit offsets)."""
    stats = np.ascontiguousarray(stats, dtype=np.float64)
    gid = np.ascontiguousarray(gid, dtype=np.int64)
    assert stats.shape == (NDAYSTAT, gid.size)
    o = daystat_opts(**thresholds)
    _check(lib().h9g_write_sxy_nc(str(path).encode(), nx, ny, gid.size, gid.ctypes.data_as(_I64P), int(jyear),
                                  C.byref(o), stats.ctypes.data_as(_DP)), "h9g_write_sxy_nc")


def day_order_stats(records_by_year, *, series, p, pooled=False) -> np.ndarray:
    """Order statistics of one daily series from day records, a list of years
    each (nday_y, 7, ncell) (Context.get_days) -> (nres, 1 + 2 len(p), ncell)
    float64, nres = 1 when pooled, else one result per year: the numpy statement
    of what Context.get_dayquant selects on the device, bit for bit.

    Candidates: for series q and e the day's amount, S[d] - S[d-1] in float64
    with S the year's running sum (row 0 or 1) and S[-1] = 0 in every year (as
    day_stats' q and e); for the other series the record's row widened to
    float64.  A NaN is no candidate; m candidates are left (row 0).  They are
    ordered by their bits (the sign-magnitude pattern mapped to a monotone
    unsigned key, so -0 comes before +0; np.sort on the floats would leave
    those two in any order): x_(0) <= ... <= x_(m-1).  For p[i], g = p[i] *
    float64(m - 1) and j = floor(g): row 1 + 2i is x_(j), row 2 + 2i is
    x_(min(j + 1, m - 1)); both NaN where m = 0.  ``day_quantiles``
    interpolates between the two."""
    yrs, n = _quant_years(records_by_year)
    o = dayquant_opts(series=series, p=p, pooled=pooled)
    top = np.uint64(1) << np.uint64(63)
    keys = []
    for r in yrs:
        x = r[:, o.series].astype(np.float64)
        if o.series < 2:
            with np.errstate(invalid="ignore"):                   # (inf - inf: a NaN, no candidate)
                x = np.diff(x, axis=0, prepend=np.zeros_like(x[:1]))
        u = np.ascontiguousarray(x).view(np.uint64)
        k = u ^ np.where(u >> np.uint64(63) != 0, ~np.uint64(0), top)
        keys.append(np.where(np.isnan(x), ~np.uint64(0), k))      # (no candidate has that key: it is a NaN's)
    groups = [np.concatenate(keys)] if o.pooled else keys
    out = np.empty((len(groups), 1 + 2 * o.nq, n), dtype=np.float64)
    for res, k in enumerate(groups):
        m = (k != ~np.uint64(0)).sum(axis=0)
        ks = np.sort(k, axis=0)                                   # unsigned order: the candidates first
        out[res, 0] = m
        last = np.maximum(m, 1) - 1
        for i in range(o.nq):
            g = np.float64(o.p[i]) * last.astype(np.float64)
            j = np.floor(g).astype(np.int64)
            for row, idx in ((1 + 2 * i, j), (2 + 2 * i, np.minimum(j + 1, last))):
                kk = np.take_along_axis(ks, idx[None], axis=0)[0]
                u = kk ^ np.where(kk >> np.uint64(63) != 0, top, ~np.uint64(0))
                out[res, row] = np.where(m > 0, u.view(np.float64), np.nan)
    return out


def day_quantiles(quant, p) -> np.ndarray:
    """The quantiles of Context.get_dayquant's / day_order_stats' result
    (..., 1 + 2 len(p), ncell) -> (..., len(p), ncell) float64: with m = row 0,
    g = p[i] * float64(m - 1) and j = floor(g), lo + (hi - lo) * (g - j) in
    float64 between the two order statistics (numpy's default "linear"
    quantile); where they are equal, or g is whole, the lower one itself (an
    infinite value does not turn into NaN).  Deterministic and derived, like
    the monthly means."""
    q = np.asarray(quant, dtype=np.float64)
    p = np.atleast_1d(np.asarray(p, dtype=np.float64))
    if q.shape[-2] != 1 + 2 * p.size:
        raise ValueError("day_quantiles: quant must be (..., 1 + 2 len(p), ncell)")
    m = q[..., 0, :]
    out = np.empty(q.shape[:-2] + (p.size, q.shape[-1]), dtype=np.float64)
    for i in range(p.size):
        g = p[i] * (np.maximum(m, 1.0) - 1.0)
        t = g - np.floor(g)
        lo, hi = q[..., 1 + 2 * i, :], q[..., 2 + 2 * i, :]
        with np.errstate(invalid="ignore"):
            v = lo + (hi - lo) * t
        out[..., i, :] = np.where((t == 0.0) | (lo == hi), lo, v)
    return out


def write_qxy_nc(path, quant, gid, year_first: int, year_last: int | None = None, nx: int = 720, ny: int = 360, *,
                 series, p, pooled=False):
    """One result of Context.get_dayquant / day_order_stats, (1 + 2 len(p),
    ncell) float64, of the cells gid to qxyYYYY.nc (or qxyYYYY_YYYY.nc for a
    pooled span): dimension quantile with coordinate p, count(lat, lon), and
    lower, upper, value(quantile, lat, lon) -- value is day_quantiles'
    interpolation -- float64 with NaN fill on write_axy_nc's latitude /
    longitude grid; the series' name and the years are global attributes
    (h9g_write_qxy_nc; netCDF classic, 64-bit offsets)."""
    o = dayquant_opts(series=series, p=p, pooled=pooled)
    quant = np.ascontiguousarray(quant, dtype=np.float64)
    gid = np.ascontiguousarray(gid, dtype=np.int64)
    assert quant.shape == (1 + 2 * o.nq, gid.size)
    _check(lib().h9g_write_qxy_nc(str(path).encode(), nx, ny, gid.size, gid.ctypes.data_as(_I64P), int(year_first),
                                  int(year_first if year_last is None else year_last), C.byref(o),
                                  quant.ctypes.data_as(_DP)), "h9g_write_qxy_nc")


def write_dxy_nc(path, records, gid, zc, jyear: int, nx: int = 720, ny: int = 360):
    """One year of day records (nday, 7, ncell) of the cells gid, as
    ``day_values`` derives them, to dxyYYYY.nc: seven variables under a leading
    dimension time on write_axy_nc's grid (h9g_write_dxy_nc; netCDF classic,
    64-bit offsets)."""
    records = np.ascontiguousarray(records, dtype=np.float32)
    gid = np.ascontiguousarray(gid, dtype=np.int64)
    zc = np.ascontiguousarray(zc, dtype=np.float32)
    assert records.ndim == 3 and records.shape[1:] == (NDAYREC, gid.size)
    _check(lib().h9g_write_dxy_nc(str(path).encode(), nx, ny, zc.size, _fp(zc), gid.size, gid.ctypes.data_as(_I64P),
                                  int(jyear), records.shape[0], _fp(records)), "h9g_write_dxy_nc")


def month_ends(jyear: int) -> np.ndarray:
    """The last day (1-based) of each month of jyear, INIT.f90:844-859."""
    e = np.array([31, 59, 90, 120, 151, 181, 212, 243, 273, 304, 334, 365])
    if days_in_year(jyear) == 366:
        e[1:] += 1
    return e


def monthly_means(snapshots, jyear: int, nisurf: int, evap=False) -> np.ndarray:
    """Monthly means from one year's month-end snapshots (12, 12+L, ncell)
    (Context.get_monthly): in float64, (S[m] - S[m-1]) / days_m with
    S[-1] = 0, rounded to float32; the divisor is days_m * nisurf for rnf
    (row 2) and 1 for npp (row 0, a monthly total, as the annual row is a
    yearly total).  Row evap (3) is the reference's zero; evap: the
    snapshots of an ET run (Context.set_evap), whose row evap is a sum over
    the substeps like rnf: its divisor is then days_m * nisurf too.  Derived from the
    reference's f32 running sums: deterministic, but not a reference
    quantity (the reference writes annual means only)."""
    s = np.asarray(snapshots, dtype=np.float32).astype(np.float64)
    if s.ndim != 3 or s.shape[0] != NMONTHS:
        raise ValueError("monthly_means: snapshots must be (12, 12+L, ncell)")
    d = np.diff(s, axis=0, prepend=np.zeros_like(s[:1]))
    days = np.diff(month_ends(jyear), prepend=0).astype(np.float64)
    div = np.repeat(days[:, None], s.shape[1], axis=1)
    div[:, 0] = 1.0
    div[:, 2] = days * float(nisurf)
    if evap:
        div[:, 3] = days * float(nisurf)
    return (d / div[:, :, None]).astype(np.float32)


def decades(year0: int, nyears: int):
    """The reference's decades (HYBRID9.f90:93-113: 1901-1910, 1911-1920,
    ...) cut to [year0, year0 + nyears): list of (first year, years)."""
    out, y, end = [], year0, year0 + nyears
    while y < end:
        e = min(1901 + 10 * ((y - 1901) // 10) + 10, end)
        out.append((y, e - y))
        y = e
    return out


def run_cell_order(*, zi, params, forcing, nisurf=48, year0=1901, nyears=1, grow_on=True,
                   state0: np.ndarray | None = None, device=0, chains=None, pipelined=True, daily_cells=None,
                   monthly=False, evap=False, days=False, daystats: dict | None = None,
                   dayquant: dict | None = None):
    """``run`` in the reference's own cell order (smp carried from cell to
    cell, cells in the given order; chains: a reference rank per cell, each
    rank its own chain, shard.reference_blocks).  pipelined: one
    ``Context.run_ordered`` over all the years (every year's forcing
    resident, the decades overlapping on the device); else decade by decade
    through ``Context.run_decade_ordered``.  Returns dict(annual, state, rc,
    err, errors, passes (per decade), work (decade_stats per call),
    overlap (ordered_stats, pipelined)).  daily_cells: the cells whose daily
    line is recorded (Context.set_daily) -> out["daily"] (ndays, 11, nsel); the
    decades then run one after another.  monthly: the month-end snapshots
    (Context.set_monthly) -> out["monthly"] (nyears, 12, 12+L, n); the decades
    stay overlapped.  evap: evapotranspiration recording (Context.set_evap):
    row evap of annual and monthly is the year's evaporation sum.  days: day
    records (Context.set_days; turns evap on) -> out["days"] (nyears, 366, 7,
    n), day 366 of a 365-day year NaN; the decades stay overlapped.  daystats:
    dict of thresholds (may be empty; DAYSTAT_THRESHOLDS): the day statistics
    (Context.get_daystats; turns evap and day recording on) ->
    out["daystats"] (nyears, 17, n), one call over the years of an ordered
    call; the records themselves are copied out only with days.  dayquant:
    dict(series=, p=, pooled=False), the keywords of Context.get_dayquant (turns
    evap and day recording on) -> out["dayquant"], one call over the years of
    an ordered call: (nyears, 1 + 2 len(p), n), or with pooled (1, ...) over the
    whole span (decade by decade: one result per decade)."""
    want_days, days = days, days or daystats is not None or dayquant is not None
    evap = evap or days
    L = params["theta_s"].shape[1]
    n = params["fmax"].size
    with Context(n, zi, nlayers=L, nisurf=nisurf, grow_on=grow_on, device=device,
                 nslots=nyears if pipelined else 10) as ctx:
        ctx.set_chains(chains)
        ctx.set_params(params)
        if daily_cells is not None:
            ctx.set_daily(daily_cells)
        if monthly:
            ctx.set_monthly(True)
        if evap:
            ctx.set_evap(True)
        if days:
            ctx.set_days(True)
        if state0 is None:
            ctx.init_state()
        else:
            ctx.set_state(state0)
        ann = np.full((nyears, 12 + L, n), np.nan, dtype=np.float32)
        d0, rc, err, passes, work = 0, 0, None, [], []
        if pipelined:
            for k in range(nyears):
                nt = days_in_year(year0 + k)
                ctx.push_forcing(k, forcing[:, d0:d0 + nt, :])
                d0 += nt
            a, passes = ctx.run_ordered(list(range(nyears)), year0, raise_on_stop=False)
            rc = ctx.decade_rc
            if not rc or len(decades(year0, nyears)) == 1:
                out = dict(annual=a, state=ctx.get_state(), rc=rc, err=ctx.last_error() if rc else None,
                           errors=ctx.get_errors(), passes=passes, work=[ctx.decade_stats()],
                           overlap=ctx.ordered_stats())
                if daily_cells is not None:
                    out["daily"] = np.concatenate([ctx.get_daily(k) for k in range(nyears)])
                if monthly:
                    out["monthly"] = np.stack([ctx.get_monthly(k) for k in range(nyears)])
                if want_days:
                    out["days"] = _days_years(ctx, nyears)
                if daystats is not None:
                    out["daystats"] = ctx.get_daystats(0, nyears, **daystats)
                if dayquant is not None:
                    out["dayquant"] = ctx.get_dayquant(0, nyears, **dayquant)
                return out
    if pipelined:
        # a STOP: the reference program ends in that decade, while run_ordered
        # goes on with the other cells; the decade-by-decade form stops there
        return run_cell_order(zi=zi, params=params, forcing=forcing, nisurf=nisurf, year0=year0, nyears=nyears,
                              grow_on=grow_on, state0=state0, device=device, chains=chains, pipelined=False,
                              daily_cells=daily_cells, monthly=monthly, evap=evap, days=want_days,
                              daystats=daystats, dayquant=dayquant)
    with Context(n, zi, nlayers=L, nisurf=nisurf, grow_on=grow_on, device=device, nslots=10) as ctx:
        ctx.set_chains(chains)
        ctx.set_params(params)
        if daily_cells is not None:
            ctx.set_daily(daily_cells)
        if monthly:
            ctx.set_monthly(True)
        if evap:
            ctx.set_evap(True)
        if days:
            ctx.set_days(True)
        if state0 is None:
            ctx.init_state()
        else:
            ctx.set_state(state0)
        ann = np.full((nyears, 12 + L, n), np.nan, dtype=np.float32)
        mon = np.full((nyears, NMONTHS, 12 + L, n), np.nan, dtype=np.float32)
        rec = np.full((nyears, 366, NDAYREC, n), np.nan, dtype=np.float32) if want_days else None
        stats = np.full((nyears, NDAYSTAT, n), np.nan, dtype=np.float64)
        d0, rc, err, passes, work, daily, quant = 0, 0, None, [], [], [], []
        for y0, ny in decades(year0, nyears):
            for k in range(ny):
                nt = days_in_year(y0 + k)
                ctx.push_forcing(k, forcing[:, d0:d0 + nt, :])
                d0 += nt
            a, p = ctx.run_decade_ordered(list(range(ny)), y0, raise_on_stop=False)
            ann[y0 - year0:y0 - year0 + ny] = a
            passes.append(p)
            work.append(ctx.decade_stats())
            if daily_cells is not None:
                daily += [ctx.get_daily(k) for k in range(ny)]
            if monthly:
                for k in range(ny):
                    mon[y0 - year0 + k] = ctx.get_monthly(k)
            if want_days:
                rec[y0 - year0:y0 - year0 + ny] = _days_years(ctx, ny)
            if daystats is not None:
                stats[y0 - year0:y0 - year0 + ny] = ctx.get_daystats(0, ny, **daystats)
            if dayquant is not None:
                quant.append(ctx.get_dayquant(0, ny, **dayquant))
            rc = ctx.decade_rc
            if rc:
                err = ctx.last_error()
                break
        out = dict(annual=ann, state=ctx.get_state(), rc=rc, err=err, errors=ctx.get_errors(), passes=passes,
                   work=work)
        if daily_cells is not None:
            out["daily"] = np.concatenate(daily)
        if monthly:
            out["monthly"] = mon
        if want_days:
            out["days"] = rec
        if daystats is not None:
            out["daystats"] = stats
        if dayquant is not None:
            out["dayquant"] = np.concatenate(quant)
        return out


def _days_years(ctx, nyears: int) -> np.ndarray:
    """Years 0 .. nyears-1 of the context's day records as (nyears, 366, 7, n)."""
    rec = np.full((nyears, 366, NDAYREC, ctx.ncell), np.nan, dtype=np.float32)
    for k in range(nyears):
        d = ctx.get_days(k)
        rec[k, :d.shape[0]] = d
    return rec


def run(*, zi, params, forcing, nisurf=48, year0=1901, nyears=1, grow_on=True,
        state0: np.ndarray | None = None, device=0, stop_on_error=True, daily_cells=None, monthly=False,
        evap=False, spinup: dict | None = None, days=False, daystats: dict | None = None,
        dayquant: dict | None = None):
    """Run ``nyears`` years from ``year0`` for every cell (HYBRID9.f90:120-290).

    Same contract as ``oracle.port.run`` / ``oracle.refcase.run_case``:
    forcing is (7, ndays_total, ncell); returns dict(annual (nyears, 12+L,
    ncell), state (packed), rc, err, errors).  A cell reaching one of the
    reference's STOPs stops (NaN means); with stop_on_error the run ends
    after that year, as the reference program would, else the other cells
    go on.  ``errors`` holds every cell's STOP record (Context.get_errors).
    daily_cells: the cells whose daily line is recorded (Context.set_daily)
    -> out["daily"] (ndays of the years run, 11, nsel).  monthly: the month-end
    snapshots (Context.set_monthly) -> out["monthly"] (nyears, 12, 12+L, n).
    evap: evapotranspiration recording (Context.set_evap): row evap (3) of
    annual and monthly is the year's evaporation sum instead of the
    reference's zero.  days: day records (Context.set_days; turns evap on)
    -> out["days"] (nyears, 366, 7, n) in DAY_FIELDS' order, day 366 of a
    365-day year NaN.  daystats: dict of thresholds (may be empty;
    DAYSTAT_THRESHOLDS): the day statistics of every year
    (Context.get_daystats; turns evap and day recording on) ->
    out["daystats"] (nyears, 17, n) in DAYSTAT_FIELDS' order; the records
    themselves are copied out only with days.  dayquant: dict(series=, p=), the
    keywords of Context.get_dayquant (turns evap and day recording on) ->
    out["dayquant"] (nyears, 1 + 2 len(p), n); pooled is a ValueError here, since
    an isolated run retains one year.  spinup: dict(years=Y, max_cycles=..., and the other
    keywords of Context.spinup): the first Y years of ``forcing``, resident in
    Y slots, are cycled to equilibrium before the run proper (Context.spinup;
    nothing is recorded meanwhile) -> out["spinup"]; the years of the run
    proper are unchanged and start from the spun-up state.  A STOP during
    spin-up takes that cell out of the run and is reported in out["spinup"]
    (rc) and in ``errors``."""
    if dayquant is not None and dayquant.get("pooled"):
        raise ValueError("run: pooled day quantiles need an ordered call (run_cell_order); an isolated run "
                         "retains one year")
    want_days, days = days, days or daystats is not None or dayquant is not None
    evap = evap or days
    L = params["theta_s"].shape[1]
    n = params["fmax"].size
    spin = dict(spinup) if spinup else None
    spin_years = int(spin.pop("years")) if spin else 0
    if spin and not 1 <= spin_years <= nyears:
        raise ValueError("run: spinup['years'] must be between 1 and nyears")
    with Context(n, zi, nlayers=L, nisurf=nisurf, grow_on=grow_on, device=device,
                 nslots=max(2, spin_years)) as ctx:
        ctx.set_params(params)
        if state0 is None:
            ctx.init_state()
        else:
            ctx.set_state(state0)
        if evap:
            ctx.set_evap(True)
        spun = None
        if spin:
            d0 = 0
            for k in range(spin_years):
                nt = days_in_year(year0 + k)
                ctx.push_forcing(k, forcing[:, d0:d0 + nt, :])
                d0 += nt
            spun = ctx.spinup(list(range(spin_years)), year0, raise_on_stop=False, **spin)
        if daily_cells is not None:
            ctx.set_daily(daily_cells)
        if monthly:
            ctx.set_monthly(True)
        if days:
            ctx.set_days(True)
        ann = np.full((nyears, 12 + L, n), np.nan, dtype=np.float32)
        mon = np.full((nyears, NMONTHS, 12 + L, n), np.nan, dtype=np.float32)
        rec = np.full((nyears, 366, NDAYREC, n), np.nan, dtype=np.float32) if want_days else None
        stats = np.full((nyears, NDAYSTAT, n), np.nan, dtype=np.float64)
        quant = [] if dayquant is None else np.full((nyears, 1 + 2 * dayquant_opts(**dayquant).nq, n), np.nan)
        d0, rc, err, daily = 0, 0, None, []
        for y in range(nyears):
            nt = days_in_year(year0 + y)
            ctx.push_forcing(y % 2, forcing[:, d0:d0 + nt, :])
            ctx.run_year(y % 2, year0 + y)
            rc = ctx.sync(raise_on_stop=False)
            ann[y] = ctx.get_annual()
            if daily_cells is not None:
                daily.append(ctx.get_daily())
            if monthly:
                mon[y] = ctx.get_monthly()
            if want_days:
                rec[y, :nt] = ctx.get_days()
            if daystats is not None:
                stats[y] = ctx.get_daystats(**daystats)[0]
            if dayquant is not None:
                quant[y] = ctx.get_dayquant(**dayquant)[0]
            d0 += nt
            if rc:
                err = ctx.last_error()
                if stop_on_error:
                    break
        out = dict(annual=ann, state=ctx.get_state(), rc=rc, err=err, errors=ctx.get_errors())
        if daily_cells is not None:
            out["daily"] = np.concatenate(daily)
        if monthly:
            out["monthly"] = mon
        if want_days:
            out["days"] = rec
        if daystats is not None:
            out["daystats"] = stats
        if dayquant is not None:
            out["dayquant"] = quant
        if spun is not None:
            out["spinup"] = spun
        return out
