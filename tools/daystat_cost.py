#!/usr/bin/env python3
"""Cost of the day statistics (h9g_get_daystats) on the config-2
grid (67,420 cells, L = 8, NISURF = 48, GROW off), beside what they replace.

    python tools/daystat_cost.py [--mode year|ordered] [--reps 12] [--out FILE.json]

year     one recorded year (h9g_run_year with day recording on).  For every
         workgroup h9g_daystat_kernel is built with (W = 4, 8, 16 waves, chosen
         through H9G_DAYSTAT_W): the kernel's device ms (HIP events around the
         launch, h9g_last_daystat_ms; median of --reps calls after two warm-up
         calls), the bytes of the year's records divided by that time, and the
         wall ms of the whole get_daystats call (launch, synchronisation and
         the copy of the 17 rows).  Beside them the path it replaces: the wall
         ms of get_days for the same year, and of hybrid9_amd.day_stats over
         the copy on 16 host threads (the cells cut into 16 blocks).  The rows
         of the two paths are compared bit for bit.
ordered  the reference's cell order over 1901-1920 (h9g_run_ordered), every
         year's records retained: get_daystats(0, 20) in one call, timed once,
         beside twenty calls of one year each."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
WS = (4, 8, 16)
THREADS = 16


def host_stats(h, rec, thr):
    n = rec.shape[2]
    cuts = np.linspace(0, n, THREADS + 1).astype(int)
    with ThreadPoolExecutor(THREADS) as ex:
        parts = list(ex.map(lambda i: h.day_stats(rec[:, :, cuts[i]:cuts[i + 1]], **thr), range(THREADS)))
    return np.concatenate(parts, axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="year", choices=("year", "ordered"))
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import hybrid9_amd as h
    from hybrid9_amd import synth

    gid = synth.land_cells()
    n = int(gid.size)
    ny = 20 if a.mode == "ordered" else 1
    thr = dict(h.DAYSTAT_THRESHOLDS)
    res = dict(mode=a.mode, build_id=h.build_id(), ncell=n, nisurf=48, grow_on=False, reps=a.reps, series=[])
    with h.Context(n, synth.ZI_L8, nisurf=48, grow_on=False, nslots=max(ny, 2)) as ctx:
        ctx.set_cells(gid, synth.cell_lat(gid))
        ctx.synth_params(synth.SEED)
        ctx.init_state()
        for k in range(ny):
            ctx.synth_forcing(k, synth.SEED, synth.year_day0(1901 + k), synth.days_in_year(1901 + k))
        ctx.sync()
        ctx.set_evap(True)
        ctx.set_days(True)
        if a.mode == "year":
            ctx.run_year(0, 1901)
            ctx.sync(raise_on_stop=False)
            nt = 365
            nbytes = nt * h.NDAYREC * n * 4
            got = {}
            for w in WS:
                os.environ["H9G_DAYSTAT_W"] = str(w)
                dev, wall = [], []
                for r in range(a.reps + 2):
                    t0 = time.perf_counter()
                    got[w] = ctx.get_daystats(**thr)
                    t1 = time.perf_counter()
                    if r >= 2:
                        dev.append(ctx.last_daystat_ms())
                        wall.append((t1 - t0) * 1e3)
                row = dict(W=w, device_ms=dev, device_ms_median=statistics.median(dev), device_ms_min=min(dev),
                           read_bytes=nbytes, tb_per_s=nbytes / (statistics.median(dev) * 1e-3) / 1e12,
                           wall_ms_median=statistics.median(wall), wall_ms_min=min(wall), wall_ms_max=max(wall))
                res["series"].append(row)
                print(f"W = {w:2d}: h9g_daystat_kernel device ms median {row['device_ms_median']:.3f} (min "
                      f"{row['device_ms_min']:.3f}, {a.reps} calls); {nbytes / 1e6:.1f} MB of records -> "
                      f"{row['tb_per_s']:.2f} TB/s; get_daystats wall ms median {row['wall_ms_median']:.2f} "
                      f"(min {row['wall_ms_min']:.2f}, max {row['wall_ms_max']:.2f})", flush=True)
            os.environ.pop("H9G_DAYSTAT_W")
            same = all(np.array_equal(got[w].view(np.uint64), got[WS[0]].view(np.uint64)) for w in WS)
            copy, host = [], []
            for r in range(4):
                t0 = time.perf_counter()
                rec = ctx.get_days()
                t1 = time.perf_counter()
                st = host_stats(h, rec, thr)
                t2 = time.perf_counter()
                if r:
                    copy.append((t1 - t0) * 1e3)
                    host.append((t2 - t1) * 1e3)
            nan = np.isnan(st) & np.isnan(got[WS[0]][0])
            eq = bool(np.all((st.view(np.uint64) == got[WS[0]][0].view(np.uint64)) | nan))
            res["replaced"] = dict(get_days_wall_ms=copy, get_days_wall_ms_median=statistics.median(copy),
                                   day_stats_16_threads_wall_ms=host,
                                   day_stats_16_threads_wall_ms_median=statistics.median(host),
                                   same_bits_as_device=eq, same_bits_across_W=same)
            print(f"replaced: get_days wall ms median {statistics.median(copy):.1f} (min {min(copy):.1f}); "
                  f"day_stats on {THREADS} host threads {statistics.median(host):.1f} ms; rows equal to the "
                  f"device's bit for bit: {eq}; the same for every W: {same}", flush=True)
        else:
            t0 = time.perf_counter()
            ctx.run_ordered(list(range(ny)), 1901, raise_on_stop=False, annual=False)
            t1 = time.perf_counter()
            ctx.get_daystats(0, 1, **thr)                      # (the first call allocates)
            ctx.get_daystats(0, ny, **thr)
            t2 = time.perf_counter()
            one = ctx.get_daystats(0, ny, **thr)
            t3 = time.perf_counter()
            dev_one = ctx.last_daystat_ms()
            dev_each, each = [], []
            for k in range(ny):
                each.append(ctx.get_daystats(k, 1, **thr)[0])
                dev_each.append(ctx.last_daystat_ms())
            t4 = time.perf_counter()
            nbytes = sum(synth.days_in_year(1901 + k) for k in range(ny)) * h.NDAYREC * n * 4
            eq = bool(np.array_equal(np.stack(each).view(np.uint64), one.view(np.uint64)))
            res["ordered"] = dict(years=ny, run_ordered_wall_s=t1 - t0, one_call_wall_ms=(t3 - t2) * 1e3,
                                  one_call_device_ms=dev_one, per_year_calls_wall_ms=(t4 - t3) * 1e3,
                                  per_year_calls_device_ms=sum(dev_each), read_bytes=nbytes,
                                  one_call_tb_per_s=nbytes / (dev_one * 1e-3) / 1e12, same_bits=eq)
            print(f"ordered 1901-{1900 + ny}: run_ordered {t1 - t0:.1f} s; get_daystats(0, {ny}) wall "
                  f"{(t3 - t2) * 1e3:.1f} ms, device {dev_one:.2f} ms ({nbytes / 1e9:.2f} GB -> "
                  f"{res['ordered']['one_call_tb_per_s']:.2f} TB/s); {ny} calls of one year: wall "
                  f"{(t4 - t3) * 1e3:.1f} ms, device {sum(dev_each):.2f} ms; the same bits: {eq}", flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
