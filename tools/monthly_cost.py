#!/usr/bin/env python3
"""Cost of monthly recording (h9g_set_monthly) on the config-2
grid (67,420 cells, L = 8, NISURF = 48, GROW off).

    python tools/monthly_cost.py [--mode year|ordered] [--monthly 0,1] [--reps 7]
                                 [--root DIR] [--label TEXT] [--out FILE.json]

year     wall ms per run_year (host clock around run_year + sync, the state
         reset to the same start before every run; the first run warms up)
         and the year kernel's device ms, with recording off (0) and on (1).
ordered  what bench.py times, once per setting: the reference's cell order
         over 1911-1930 (h9g_run_ordered, whole decades) after an untimed
         1901-1910, every year's synthetic forcing resident; wall ms per
         simulated year.

--root: the tree whose hybrid9_amd package (and library) is measured, so that
two builds can be alternated from a shell loop; a build without
h9g_set_monthly is measured with recording off only."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="year", choices=("year", "ordered"))
    ap.add_argument("--monthly", default="0,1")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--root", default=str(Path(__file__).resolve().parents[1]))
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import hybrid9_amd as h
    from hybrid9_amd import synth

    gid = synth.land_cells()
    n = int(gid.size)
    ordered = a.mode == "ordered"
    res = dict(label=a.label, root=a.root, mode=a.mode, build_id=h.build_id(), ncell=n, nisurf=48, grow_on=False,
               reps=a.reps, series=[])
    with h.Context(n, synth.ZI_L8, nisurf=48, grow_on=False, nslots=30 if ordered else 2) as ctx:
        ctx.set_cells(gid, synth.cell_lat(gid))
        ctx.synth_params(synth.SEED)
        ctx.init_state()
        st0 = ctx.get_state()
        for k in range(30 if ordered else 1):
            ctx.synth_forcing(k, synth.SEED, synth.year_day0(1901 + k), synth.days_in_year(1901 + k))
        ctx.sync()
        res["kernel"] = ctx.kernel_name()
        for on in [int(v) for v in a.monthly.split(",")]:
            if hasattr(ctx, "set_monthly"):
                ctx.set_monthly(bool(on))
            elif on:
                print(f"{a.label} monthly=1: this build has no h9g_set_monthly", flush=True)
                continue
            if ordered:
                ctx.set_state(st0)
                ctx.run_ordered(list(range(10)), 1901, raise_on_stop=False, annual=False)
                t0 = time.perf_counter()
                ctx.run_ordered(list(range(10, 30)), 1911, raise_on_stop=False, annual=False)
                t1 = time.perf_counter()
                row = dict(monthly=on, wall_ms_per_year=(t1 - t0) * 1e3 / 20, overlap=ctx.ordered_stats())
                print(f"{a.label} ordered 1911-1930 monthly={on}: {row['wall_ms_per_year']:.2f} ms per simulated year",
                      flush=True)
            else:
                wall, dev = [], []
                for r in range(a.reps + 1):
                    ctx.set_state(st0)
                    ctx.sync()
                    t0 = time.perf_counter()
                    ctx.run_year(0, 1901)
                    ctx.sync(raise_on_stop=False)
                    t1 = time.perf_counter()
                    if r:
                        wall.append((t1 - t0) * 1e3)
                        dev.append(ctx.last_kernel_ms())
                row = dict(monthly=on, wall_ms=wall, wall_ms_median=statistics.median(wall), wall_ms_min=min(wall),
                           wall_ms_max=max(wall), year_kernel_ms_median=statistics.median(dev))
                print(f"{a.label} run_year monthly={on}: wall ms median {row['wall_ms_median']:.2f} "
                      f"(min {row['wall_ms_min']:.2f}, max {row['wall_ms_max']:.2f}, {a.reps} runs); "
                      f"year kernel {row['year_kernel_ms_median']:.2f} ms", flush=True)
            res["series"].append(row)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
