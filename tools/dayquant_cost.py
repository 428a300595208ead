#!/usr/bin/env python3
"""Cost of the day quantiles (h9g_get_dayquant) on the config-2
grid (67,420 cells, L = 8, NISURF = 48, GROW off), beside what they replace:
series q at p = 0.05, 0.5, 0.95.

    python tools/dayquant_cost.py [--mode year|ordered] [--reps 8] [--out FILE.json]

year     one recorded year (h9g_run_year with day recording on).  For every
         variant h9g_dayquant_kernel is built with (digits of 2, 4 and 8 bits,
         W = 4, 8, 16 waves, chosen through H9G_DAYQUANT_BITS and
         H9G_DAYQUANT_W): the device ms of the call's launches (HIP events,
         h9g_last_dayquant_ms; median of --reps calls after two warm-up
         calls), the bytes it reads (one row of the year per pass, 64 / bits
         + 1 passes per group of ranks), those bytes at the part's streaming
         read rate (6.0 TB/s) as the yardstick, and the wall ms
         of the whole get_dayquant call.  Beside them the path it replaces:
         the wall ms of get_days for the same year, and of np.partition over
         the copy on 16 host threads (the cells cut into 16 blocks).  The
         results of all variants and of hybrid9_amd.day_order_stats are
         compared bit for bit.  Also the 32-bit key path (series zwt) of the
         product's variant.
ordered  the reference's cell order over 1901-1920 (h9g_run_ordered), every
         year's records retained: get_dayquant(0, 20) per year and pooled, for
         every variant, and the host route (20 get_days, np.partition of the
         pooled series on 16 threads).
profile  the recorded year and three get_dayquant calls of the product's
         variant and nothing else: the program to run under a counter
         collection (rocprofv3 --pmc ..., counters in a run of their own)."""
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
BITS = (2, 4, 8)
WS = (4, 8, 16)
GROUP = {2: 4, 4: 4, 8: 1}       # ranks a launch selects at once (h9g_quant.hip quant_group)
THREADS = 16
STREAM_TBS = 6.0                 # the part's measured streaming read rate (6.0-6.3 TB/s)
P = (0.05, 0.5, 0.95)


def passes(bits, nq, key_bits=64):
    groups = -(-nq // GROUP[bits])
    return groups * (key_bits // bits + 1)


def host_partition(days_by_year):
    """The host route for series q at P: the days' amounts of every year, pooled, np.partition per block of cells."""
    n = days_by_year[0].shape[2]
    cuts = np.linspace(0, n, THREADS + 1).astype(int)

    def block(i):
        sl = slice(cuts[i], cuts[i + 1])
        q = np.concatenate([np.diff(r[:, 0, sl].astype(np.float64), axis=0, prepend=0.0) for r in days_by_year])
        m = q.shape[0]
        ks = sorted({int(np.floor(p * (m - 1))) for p in P} | {min(int(np.floor(p * (m - 1))) + 1, m - 1) for p in P})
        part = np.partition(q, ks, axis=0)
        return part[ks]

    with ThreadPoolExecutor(THREADS) as ex:
        return np.concatenate(list(ex.map(block, range(THREADS))), axis=1)


def timed(ctx, reps, **kw):
    dev, wall, got = [], [], None
    for r in range(reps + 2):
        t0 = time.perf_counter()
        got = ctx.get_dayquant(**kw)
        t1 = time.perf_counter()
        if r >= 2:
            dev.append(ctx.last_dayquant_ms())
            wall.append((t1 - t0) * 1e3)
    return got, dev, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="year", choices=("year", "ordered", "profile"))
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import hybrid9_amd as h
    from hybrid9_amd import synth

    gid = synth.land_cells()
    n = int(gid.size)
    ny = 20 if a.mode == "ordered" else 1
    res = dict(mode=a.mode, build_id=h.build_id(), ncell=n, nisurf=48, grow_on=False, reps=a.reps, series="q", p=P,
               stream_tb_per_s=STREAM_TBS, variants=[])
    with h.Context(n, synth.ZI_L8, nisurf=48, grow_on=False, nslots=max(ny, 2)) as ctx:
        ctx.set_cells(gid, synth.cell_lat(gid))
        ctx.synth_params(synth.SEED)
        ctx.init_state()
        for k in range(ny):
            ctx.synth_forcing(k, synth.SEED, synth.year_day0(1901 + k), synth.days_in_year(1901 + k))
        ctx.sync()
        ctx.set_evap(True)
        ctx.set_days(True)
        if a.mode in ("year", "profile"):
            ctx.run_year(0, 1901)
            ctx.sync(raise_on_stop=False)
        else:
            t0 = time.perf_counter()
            ctx.run_ordered(list(range(ny)), 1901, raise_on_stop=False, annual=False)
            res["run_ordered_wall_s"] = time.perf_counter() - t0
        if a.mode == "profile":
            for _ in range(3):
                ctx.get_dayquant(series="q", p=P)
            print(f"profile: three get_dayquant calls of the product's variant, device ms {ctx.last_dayquant_ms():.3f}")
            return
        ndays = sum(synth.days_in_year(1901 + k) for k in range(ny))
        row_bytes = ndays * n * 4                       # one row of the span: what a pass reads
        pools = (False,) if a.mode == "year" else (False, True)
        got = {}
        for bits in BITS:
            for w in WS:
                os.environ["H9G_DAYQUANT_BITS"], os.environ["H9G_DAYQUANT_W"] = str(bits), str(w)
                for pooled in pools:
                    q, dev, wall = timed(ctx, a.reps, k0=0, nk=ny, series="q", p=P, pooled=pooled)
                    got[bits, w, pooled] = q
                    np_ = passes(bits, len(P))
                    ideal = np_ * row_bytes / (STREAM_TBS * 1e12) * 1e3
                    med = statistics.median(dev)
                    row = dict(bits=bits, W=w, pooled=pooled, passes=np_, read_bytes=np_ * row_bytes,
                               yardstick_ms=ideal, device_ms=dev, device_ms_median=med, device_ms_min=min(dev),
                               tb_per_s=np_ * row_bytes / (med * 1e-3) / 1e12, share_of_yardstick=ideal / med,
                               wall_ms_median=statistics.median(wall), wall_ms_min=min(wall), wall_ms_max=max(wall))
                    res["variants"].append(row)
                    print(f"bits {bits} W {w:2d} pooled {int(pooled)}: {np_} passes, {np_ * row_bytes / 1e9:.2f} GB; "
                          f"device ms median {med:.3f} (min {min(dev):.3f}) -> {row['tb_per_s']:.2f} TB/s, "
                          f"{100 * row['share_of_yardstick']:.0f} % of the yardstick ({ideal:.3f} ms); wall ms median "
                          f"{row['wall_ms_median']:.2f} (min {row['wall_ms_min']:.2f}, max {row['wall_ms_max']:.2f})",
                          flush=True)
        os.environ.pop("H9G_DAYQUANT_BITS")
        os.environ.pop("H9G_DAYQUANT_W")
        first = {pooled: got[BITS[0], WS[0], pooled] for pooled in pools}
        same = all(np.array_equal(v.view(np.uint64), first[k[2]].view(np.uint64)) for k, v in got.items())
        # the product's variant: the 32-bit key path, and sixteen ranks
        for label, kw in (("zwt, 32-bit key", dict(series="zwt", p=P)),
                          ("q, 16 quantiles", dict(series="q", p=tuple(np.linspace(0, 1, 16))))):
            for pooled in pools:
                _, dev, wall = timed(ctx, a.reps, k0=0, nk=ny, pooled=pooled, **kw)
                res.setdefault("product", []).append(dict(what=label, pooled=pooled, device_ms=dev, wall_ms=wall))
                print(f"product variant, {label}, pooled {int(pooled)}: device ms median "
                      f"{statistics.median(dev):.3f}, wall ms median {statistics.median(wall):.2f}", flush=True)
        # the host route
        copy, host = [], []
        for r in range(3 if a.mode == "year" else 1):
            t0 = time.perf_counter()
            days = [ctx.get_days(k) for k in range(ny)]
            t1 = time.perf_counter()
            host_partition(days)
            t2 = time.perf_counter()
            copy.append((t1 - t0) * 1e3)
            host.append((t2 - t1) * 1e3)
        if a.mode == "year":
            ref = h.day_order_stats(days, series="q", p=P)
            eq = bool(np.array_equal(ref.view(np.uint64), first[False].view(np.uint64)))
        else:
            eq = None
        res["replaced"] = dict(get_days_wall_ms=copy, get_days_wall_ms_min=min(copy), partition_16_threads_wall_ms=host,
                               same_bits_as_numpy=eq, same_bits_across_variants=same)
        print(f"replaced: get_days of {ny} year(s) wall ms {['%.1f' % c for c in copy]}; np.partition on {THREADS} host "
              f"threads {['%.1f' % c for c in host]} ms; device rows equal to day_order_stats bit for bit: {eq}; the "
              f"same for every variant: {same}", flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
