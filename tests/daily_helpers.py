"""Shared by tests/test_daily_host.py and tests/test_gpu_daily.py: the host
build of cell_focus (tests/csrc/host_focus.cpp), and the oracle's per-substep
trace turned into the columns of the daily diagnostics line that it
determines (tests/golden/make_daily_golden.py)."""
from __future__ import annotations

import ctypes as C
import json
import subprocess

import numpy as np

from oracle import port, refcase
from tests.conftest import GOLDEN
from tests.golden.make_daily_golden import LINE_INDEX, daily_from_trace
from tests.helpers import BUILD, ROOT

_lib = None
F = np.float32
TF = F(273.16)


def focus_lib():
    global _lib
    if _lib is None:
        src = ROOT / "tests" / "csrc" / "host_focus.cpp"
        out = BUILD / "libhost_focus.so"
        deps = [src] + list((ROOT / "hybrid9_amd" / "csrc").glob("*.h"))
        if not out.exists() or out.stat().st_mtime < max(d.stat().st_mtime for d in deps):
            BUILD.mkdir(exist_ok=True)
            subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp",
                            "-std=c++17", "-fPIC", "-shared", str(src), "-o", str(out)], check=True)
        _lib = C.CDLL(str(out))
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
        _lib.h9k_host_focus.argtypes = [C.c_int] * 7 + [fp, fp, fp, fp, ip, fp, ip]
    return _lib


def host_focus(*, zi, params, forcing, nisurf, year0, nyears, grow_on, state0=None, const_geo=1, failed=None):
    """cell_focus on the host for every cell: dict(daily (ndays, 11, n), code (n), rc)."""
    L = params["theta_s"].shape[1]
    n = params["fmax"].size
    zi = np.ascontiguousarray(zi, np.float32)
    pp = port.pack_params(params)
    fo = np.ascontiguousarray(forcing, np.float32)
    st = port.init_state(params, zi) if state0 is None else np.ascontiguousarray(state0, np.float32)
    ndays = fo.shape[1]
    assert ndays == sum(port._days(year0 + k) for k in range(nyears)), "forcing must hold whole years"
    out = np.full((ndays, 11, n), -1.0, np.float32)
    code = np.zeros(n, np.int32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    fl = None if failed is None else np.ascontiguousarray(failed, np.int32)
    rc = focus_lib().h9k_host_focus(n, L, nisurf, int(grow_on), year0, nyears, int(const_geo), zi.ctypes.data_as(fp),
                                    pp.ctypes.data_as(fp), fo.ctypes.data_as(fp), st.ctypes.data_as(fp),
                                    None if fl is None else fl.ctypes.data_as(ip), out.ctypes.data_as(fp),
                                    code.ctypes.data_as(ip))
    return dict(daily=out, code=code, rc=rc)


def port_daily8(*, zi, params, forcing, nisurf, year0, nyears, grow_on, state0=None, cells=None):
    """The oracle (oracle.port.run, every cell traced) -> (daily8 (ndays, 8,
    ncells), run): the eight columns LINE_INDEX of the line, for the traced
    cells (all by default).  Rows from a cell's STOP day on are meaningless."""
    L = params["theta_s"].shape[1]
    n = params["fmax"].size
    cells = tuple(range(n)) if cells is None else tuple(cells)
    s0 = None if state0 is None else refcase.unpack_state(np.asarray(state0, np.float32), n, L)
    r = port.run(zi=zi, params=params, forcing=forcing, nisurf=nisurf, year0=year0, nyears=nyears,
                 grow_on=grow_on, state0=s0, trace_cells=cells, nthreads=8)
    ndays = np.asarray(forcing).shape[1]
    sel = np.asarray(sorted(cells))
    end = {k: r["state"][k][sel] for k in ("LAI", "LAI_litter")}
    return daily_from_trace(r["trace"], end, L, nisurf, ndays), r


def fT_of(tas):
    """GROW.f90:67-71 restated in float32 (plain arithmetic)."""
    tas = np.asarray(tas, F)
    x = (tas - TF).astype(F)
    d = np.abs((x - F(18.0)).astype(F))
    hi = (F(1.0) - ((d / F(21.0)).astype(F) ** 2).astype(F)).astype(F)
    a = (d / F(25.0)).astype(F)
    lo = (F(1.0) - (a * a).astype(F)).astype(F)
    lo = np.where(F(0.0) > lo, F(0.0), lo)       # MAX(zero, fT)
    lo = np.where(F(1.0) < lo, F(1.0), lo)       # MIN(one, fT)
    return np.where(x > F(18.0), hi, lo).astype(F)


def w_i_of(smp, rootr):
    """GROW.f90:55-62 restated in float32: smp, rootr (n, L) -> (n)."""
    w_i = np.zeros(smp.shape[0], F)
    for i in range(smp.shape[1]):
        w = ((F(-150000.0) - smp[:, i].astype(F)).astype(F) / (F(-150000.0) - F(-50000.0))).astype(F)
        w = np.where(F(0.0) > w, F(0.0), w)
        w = np.where(F(1.0) < w, F(1.0), w)
        w_i = (w_i + (rootr[:, i].astype(F) * w).astype(F)).astype(F)
    return w_i


def load_daily_golden(name="daily_c1"):
    """(meta, inputs, expected) of the daily golden; the synthetic inputs are
    regenerated and checked against the stored sha256."""
    from hybrid9_amd import synth
    from tests.golden.make_golden import digest, packed_params, synth_inputs
    z = np.load(GOLDEN / f"{name}.npz")
    meta = json.loads(str(z["meta"]))
    gid = np.asarray(meta["gid"], dtype=np.int64)
    p, f = synth_inputs(gid, meta["year0"], meta["nyears"], meta["L"], meta["seed"])
    assert digest(packed_params(p), f) == meta["input_sha256"], "synthetic inputs drifted"
    inputs = dict(zi=np.asarray(meta["zi"], np.float32), params=p, forcing=f, nisurf=meta["nisurf"],
                  year0=meta["year0"], nyears=meta["nyears"], grow_on=meta["grow_on"], state0=None)
    assert tuple(meta["line_index"]) == tuple(LINE_INDEX)
    return meta, inputs, dict(daily8=z["daily8"], annual=z["annual"], state=z["state"])


def stop_mask_inputs():
    """The stop_ns24 golden's inputs with cell 2 masked (theta_s = 0)."""
    from tests.conftest import load_golden
    meta, inp, _ = load_golden("stop_ns24")
    p = {k: np.array(v, copy=True) for k, v in inp["params"].items()}
    p["theta_s"][2] = 0.0
    return meta, dict(inp, params=p)


def cell_order_daily8(*, zi, params, forcing, nisurf, year0, nyears, grow_on, chains=None):
    """The daily lines of the reference's own order: port.run_cell_order's
    loop restated (decade -> cell -> year, smp carried from cell to cell,
    HYBRID9.f90:93-130) with every per-cell port.run traced.  Returns
    (daily8 (ndays, 8, n), end state, annual); the caller holds the end state
    to port.run_cell_order's."""
    L = params["theta_s"].shape[1]
    n = params["fmax"].size
    fo = np.ascontiguousarray(forcing, dtype=np.float32)
    st = refcase.unpack_state(port.init_state(params, zi), n, L)
    st = {k: np.array(v, copy=True) for k, v in st.items()}
    ann = np.full((nyears, 12 + L, n), np.nan, dtype=np.float32)
    d8 = np.full((fo.shape[1], 8, n), np.nan, dtype=np.float32)
    land = [c for c in range(n) if port._mask_sum(params["theta_s"][c]) > np.float32(1.0e-8)]
    cid = np.zeros(n, np.int64) if chains is None else np.asarray(chains, np.int64)
    groups = [[c for c in land if cid[c] == r] for r in sorted(set(cid[land].tolist()))]
    day0 = 0
    for y0, ny in port.decades(year0, nyears):
        nd = sum(port._days(y0 + k) for k in range(ny))
        carry = {grp[0]: st["smp"][grp[-1]].copy() for grp in groups}
        prev = {b: a for grp in groups for a, b in zip(grp, grp[1:])}
        for c in land:
            s1 = {k: v[c:c + 1].copy() for k, v in st.items()}
            s1["smp"][0] = carry[c] if c in carry else st["smp"][prev[c]].copy()
            r = port.run(zi=zi, params={k: v[c:c + 1] for k, v in params.items()},
                         forcing=np.ascontiguousarray(fo[:, day0:day0 + nd, c:c + 1]), nisurf=nisurf,
                         year0=y0, nyears=ny, grow_on=grow_on, state0=s1, trace_cells=(0,))
            assert r["rc"] == 0
            d8[day0:day0 + nd, :, c] = daily_from_trace(r["trace"], r["state"], L, nisurf, nd)[:, :, 0]
            for k in st:
                st[k][c] = r["state"][k][0]
            ann[y0 - year0:y0 - year0 + ny, :, c] = r["annual"][:, :, 0]
        day0 += nd
    return d8, st, ann
