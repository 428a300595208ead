#!/usr/bin/env python3
"""Cost of the daily diagnostics' shadow run (h9g_set_daily) on
the config-2 grid: wall ms per run_year (host clock around run_year + sync,
the state reset to the same start before every run) for selections of
nsel = 0, 1, 64, 1024 cells spread evenly over the grid.

    python tools/daily_cost.py [--nsel 0,1,64,1024] [--reps 7] [--root DIR] [--out FILE.json]

--root: the tree whose hybrid9_amd package (and library) is measured, so that
two builds can be alternated from a shell loop; a build without h9g_set_daily
can be measured at nsel = 0 only.  The shadow kernel's own device time comes
from a separate run of this script under a kernel trace (--reps 1), as the
durations of the h9g_focus_kernel dispatches in launch order."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nsel", default="0,1,64,1024")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--root", default=str(Path(__file__).resolve().parents[1]))
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import numpy as np
    import hybrid9_amd as h
    from hybrid9_amd import synth

    gid = synth.land_cells()
    n = int(gid.size)
    res = dict(label=a.label, root=a.root, build_id=h.build_id(), ncell=n, nisurf=48, grow_on=False, year=1901,
               reps=a.reps, series=[])
    with h.Context(n, synth.ZI_L8, nisurf=48, grow_on=False) as ctx:
        ctx.set_cells(gid, synth.cell_lat(gid))
        ctx.synth_params(synth.SEED)
        ctx.init_state()
        st0 = ctx.get_state()
        ctx.synth_forcing(0, synth.SEED, 0, 365)
        ctx.sync()
        res["kernel"] = ctx.kernel_name()
        for nsel in [int(v) for v in a.nsel.split(",")]:
            if nsel:
                ctx.set_daily(np.linspace(0, n - 1, nsel).astype(np.int64) if nsel > 1 else [n // 2])
            elif hasattr(ctx, "set_daily"):
                ctx.set_daily([])
            wall, dev = [], []
            for r in range(a.reps + 1):             # the first run warms up
                ctx.set_state(st0)
                ctx.sync()
                t0 = time.perf_counter()
                ctx.run_year(0, 1901)
                ctx.sync(raise_on_stop=False)
                t1 = time.perf_counter()
                if r:
                    wall.append((t1 - t0) * 1e3)
                    dev.append(ctx.last_kernel_ms())
            row = dict(nsel=nsel, wall_ms=wall, wall_ms_median=statistics.median(wall), wall_ms_min=min(wall),
                       wall_ms_max=max(wall), year_kernel_ms_median=statistics.median(dev))
            res["series"].append(row)
            print(f"{a.label} nsel={nsel:5d}: wall ms/run_year median {row['wall_ms_median']:.2f} "
                  f"(min {row['wall_ms_min']:.2f}, max {row['wall_ms_max']:.2f}, {a.reps} runs); "
                  f"year kernel {row['year_kernel_ms_median']:.2f} ms", flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
