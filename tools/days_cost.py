#!/usr/bin/env python3
"""Cost of day recording (h9g_set_days) on the config-2 grid
(67,420 cells, L = 8, NISURF = 48, GROW off), against ET recording alone.

    python tools/days_cost.py [--mode year|ordered|meta] [--set 0,1] [--reps 7]
                              [--root DIR] [--label TEXT] [--out FILE.json]

year     wall ms per run_year (host clock around run_year + sync, the state
         reset to the same start before every run; the first run warms up)
         and the year kernel's device ms, per setting: 0 = ET recording alone
         (the baseline: the ET kernels), 1 = ET and day recording (the day
         kernels).
ordered  what bench.py times, once per setting: the reference's cell order
         over 1911-1930 (h9g_run_ordered, whole decades) after an untimed
         1901-1910, every year's synthetic forcing resident; wall ms per
         simulated year.
meta     no GPU: registers, spills, scratch, LDS and code size
         (tools/kernel_meta.py) of every day kernel beside its ET sibling, from
         the built library of --root.

--root: the tree whose hybrid9_amd package (and library) is measured, so that
two builds can be alternated from a shell loop; a build without h9g_set_days
(the parent commit's) is measured with ET recording alone."""
from __future__ import annotations

import argparse
import json
import re
import statistics
import sys
import tempfile
import time
from pathlib import Path


def meta(root: Path):
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    import kernel_meta
    lib = root / "hybrid9_amd" / "lib" / "libh9g.so"
    with tempfile.TemporaryDirectory() as t:
        ks, sizes = [], {}
        for co in kernel_meta.code_objects(lib, Path(t)):
            ks += kernel_meta.kernels(co)
            sizes.update(kernel_meta.code_sizes(co))
    names = kernel_meta.demangle([k["name"] for k in ks])
    rows = {}
    for k, nm in zip(ks, names):
        m = re.search(r"h9g_(\w+?)(_mon|_et|_day)?_kernel<(.*?)\s*>\(", nm.replace("h9k::", ""))
        if m and m.group(1) in ("pair", "pair2", "pair11", "pair1", "pair1f", "solo") and m.group(2) in ("_et", "_day"):
            rows.setdefault((m.group(1), m.group(3)), {})[m.group(2)] = dict(k, code_bytes=sizes.get(k["name"], 0))
    print(f"{'kernel':8s} {'<L, geometry>':22s} " + " ".join(f"{v:>34s}" for v in ("_et", "_day")))
    print(f"{'':31s} " + " ".join(f"{'VGPR vsp ssp scrB   LDS B  code B':>34s}" for _ in range(2)))
    out = []
    for (stem, targs), d in sorted(rows.items()):
        cells = []
        for v in ("_et", "_day"):
            k = d.get(v)
            cells.append("-" if k is None else f"{k.get('vgpr', 0):4d} {k.get('vgpr_spill', 0):3d} "
                         f"{k.get('sgpr_spill', 0):3d} {k.get('private_bytes', 0):4d} {k.get('lds_bytes', 0):7d} "
                         f"{k.get('code_bytes', 0):7d}")
            if k is not None:
                out.append(dict(stem=stem, targs=targs, variant=v, **{x: k.get(x, 0) for x in (
                    "vgpr", "sgpr", "vgpr_spill", "sgpr_spill", "private_bytes", "lds_bytes", "code_bytes")}))
        print(f"{stem:8s} {targs:22s} " + " ".join(f"{c:>34s}" for c in cells))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="year", choices=("year", "ordered", "meta"))
    ap.add_argument("--set", default="0,1")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--root", default=str(Path(__file__).resolve().parents[1]))
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if a.mode == "meta":
        res = dict(label=a.label, root=a.root, mode="meta", kernels=meta(Path(a.root)))
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text(json.dumps(res, indent=1))
        return
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
        ctx.set_evap(True)
        for em in a.set.split(","):
            dy = int(em)
            if dy and not hasattr(ctx, "set_days"):
                print(f"{a.label} {em}: this build has no h9g_set_days", flush=True)
                continue
            if hasattr(ctx, "set_days"):
                ctx.set_days(bool(dy))
            if ordered:
                ctx.set_state(st0)
                ctx.run_ordered(list(range(10)), 1901, raise_on_stop=False, annual=False)
                t0 = time.perf_counter()
                ctx.run_ordered(list(range(10, 30)), 1911, raise_on_stop=False, annual=False)
                t1 = time.perf_counter()
                row = dict(evap=1, days=dy, wall_ms_per_year=(t1 - t0) * 1e3 / 20, overlap=ctx.ordered_stats())
                print(f"{a.label} ordered 1911-1930 evap=1 days={dy}: {row['wall_ms_per_year']:.2f} ms per "
                      f"simulated year", flush=True)
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
                row = dict(evap=1, days=dy, kernel=ctx.kernel_name(), wall_ms=wall,
                           wall_ms_median=statistics.median(wall), wall_ms_min=min(wall), wall_ms_max=max(wall),
                           year_kernel_ms_median=statistics.median(dev))
                print(f"{a.label} run_year evap=1 days={dy} ({row['kernel']}): wall ms median "
                      f"{row['wall_ms_median']:.2f} (min {row['wall_ms_min']:.2f}, max {row['wall_ms_max']:.2f}, "
                      f"{a.reps} runs); year kernel {row['year_kernel_ms_median']:.2f} ms", flush=True)
            res["series"].append(row)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
