#!/usr/bin/env python3
"""Generate tests/golden/daily_c1.npz from the REFERENCE itself: the daily
diagnostics line of its INTERACTIVE mode (HYBRID9.f90:221-229) for eight
synthetic 0.5 deg cells over 1901-1902, NISURF = 48, GROW on.

Runs ``oracle/_ref/h9ref`` (the unmodified reference HYDROLOGY.f90 / GROW.f90
behind the harness oracle/ref/h9ref_main.f90) with every cell traced and
derives, from the harness's per-substep trace, the eight columns of the line
the trace determines:

  evap_day, evap_grnd_day   the f32 sums of HYBRID9.f90:207-209 over the day's
                            substeps, from the trace's qflx_tran_veg_col and
                            qflx_evap_grnd, starting from zero
  theta(1:4)                of the day's last substep (HYDROLOGY.f90:1233)
  LAI, LAI_litter           after the day's GROW: the next day's first substep,
                            and the end state for the last day

(theta_ma(1), w_i and fT are not in the trace; tests/test_daily_host.py
restates them.)  Needs the reference sources to build h9ref; the fixture is
data and travels with the repository.

    python tests/golden/make_daily_golden.py

daily_c1.npz holds: meta (json string, kind "daily", with the inputs' sha256),
daily8 (730, 8, 8) = (day, column, cell), annual (2, 20, 8), state (packed).
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from hybrid9_amd import synth  # noqa: E402
from oracle import refcase  # noqa: E402
from tests.golden.make_golden import digest, packed_params, synth_inputs  # noqa: E402

OUT = Path(__file__).resolve().parent
COLUMNS = ("evap_day", "evap_grnd_day", "theta1", "theta2", "theta3", "theta4", "LAI", "LAI_litter")
# where they sit in the 11-value line (hybrid9_amd.site.DIAG_FIELDS)
LINE_INDEX = (0, 1, 2, 3, 4, 5, 7, 8)


def daily_gid():
    return synth.land_cells(720, 360, 67420, synth.SEED)[::8431][:8]


def daily_from_trace(trace, end_state, L, nisurf, ndays):
    """(ndays, 8, ncell) from a trace (ncell, ndays*nisurf, 3L+7) and the end
    state's LAI and LAI_litter."""
    f = np.float32
    n = trace.shape[0]
    tr = trace.reshape(n, ndays, nisurf, 3 * L + 7)
    dt = f(86400.0) / f(nisurf)                                # INIT.f90:214
    tran, evg = tr[..., 3 * L + 2], tr[..., 3 * L + 3]
    ev = np.zeros((n, ndays), f)
    evgd = np.zeros((n, ndays), f)
    for k in range(nisurf):                                    # HYBRID9.f90:207-209
        ev = (ev + ((evg[:, :, k] + tran[:, :, k]).astype(f) * dt).astype(f)).astype(f)
        evgd = (evgd + (evg[:, :, k] * dt).astype(f)).astype(f)
    out = np.empty((ndays, 8, n), f)
    out[:, 0] = ev.T
    out[:, 1] = evgd.T
    for i in range(4):
        out[:, 2 + i] = tr[:, :, nisurf - 1, 2 * L + i].T
    out[:-1, 6] = tr[:, 1:, 0, 3 * L + 5].T
    out[:-1, 7] = tr[:, 1:, 0, 3 * L + 6].T
    out[-1, 6] = end_state["LAI"]
    out[-1, 7] = end_state["LAI_litter"]
    return out


def main():
    gid = np.asarray(daily_gid(), dtype=np.int64)
    L, nisurf, year0, nyears = 8, 48, 1901, 2
    p, f = synth_inputs(gid, year0, nyears)
    n = int(gid.size)
    out = refcase.run_case(zi=synth.ZI_L8, params=p, forcing=f, nisurf=nisurf, year0=year0, nyears=nyears,
                           grow_on=1, trace_cells=tuple(range(n)))
    ndays = f.shape[1]
    d8 = daily_from_trace(out["trace"], out["state"], L, nisurf, ndays)
    meta = dict(name="daily_c1", kind="daily", seed=synth.SEED, gid=gid.tolist(), L=L, ncell=n, year0=year0,
                nyears=nyears, nisurf=nisurf, grow_on=1, zi=synth.ZI_L8.tolist(), columns=list(COLUMNS),
                line_index=list(LINE_INDEX), input_sha256=digest(packed_params(p), f),
                generator="oracle/_ref/h9ref (reference HYDROLOGY.f90/GROW.f90, amdflang -O2), per-substep trace")
    path = OUT / "daily_c1.npz"
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), daily8=d8, annual=out["annual"],
                        state=refcase.pack_state(out["state"], L))
    print(f"daily_c1: {n} cells x {nyears} yr, {path.stat().st_size / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
