#!/usr/bin/env python3
"""Cost of spin-up to equilibrium (h9g_spinup) on the config-2
grid (67,420 cells, L = 8, NISURF = 48, GROW on), year 1901 repeated.

    python tools/spinup_cost.py [--mode loop|retire] [--reps 5] [--cycles N]
                                [--root DIR] [--label TEXT] [--out FILE.json]

loop    the cost of the loop itself: wall ms of `cycles` (default 5) one-year
        cycles of h9g_spinup with every tolerance 0 and freeze = 1 (nothing is
        expected to settle: every cycle the every-cell launch, plus the spin
        kernel and one small read-back) against the same number of run_year
        calls and one sync, alternated `reps` times in one process from the
        same start state; the first pair warms up.  A tree without h9g_spinup
        (--root, e.g. the parent commit's) measures the run_year leg alone, so
        that two builds can be alternated from a shell loop.
retire  what retiring cells buys: the tolerances at the medians of the cycle-3
        drifts (tol_water, 4 x tol_zwt) and of cycle 4 (tol_plant), computed
        in numpy from the states after cycles 2, 3 and 4 of a plain run_year
        loop; then `cycles` (default 10) cycles with freeze = 1 and freeze = 0
        from the cold start: wall ms, cell-years and launches per kernel kind
        (h9g_launch_stats), cells run / settled per cycle."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np


def keys(h, st, n, L):
    """(W, zwt, pm) in float64 from a packed state (the layers added in order, then wa)."""
    off = 0
    f = {}
    for name, w in (("h2o", L), ("ma", L), ("smp", L), ("rootr", L + 1), ("zwt", 1), ("wa", 1), ("LAI", 1),
                    ("LAIl", 1), ("pm", 1)):
        f[name] = st[off:off + n * w].reshape(n, w)
        off += n * w
    w = np.zeros(n)
    for i in range(L):
        w = w + f["h2o"][:, i].astype(np.float64)
    w = w + f["wa"][:, 0].astype(np.float64)
    return w, f["zwt"][:, 0].astype(np.float64), f["pm"][:, 0].astype(np.float64)


def drift(a, b):
    with np.errstate(all="ignore"):
        return (np.abs(b[0] - a[0]), np.abs(b[1] - a[1]),
                np.where(b[2] == a[2], 0.0, np.abs(b[2] - a[2]) / np.abs(a[2])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="loop", choices=("loop", "retire"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cycles", type=int, default=0)
    ap.add_argument("--root", default=str(Path(__file__).resolve().parents[1]))
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import hybrid9_amd as h
    from hybrid9_amd import synth

    gid = synth.land_cells()
    n, L = int(gid.size), 8
    cycles = a.cycles or (5 if a.mode == "loop" else 10)
    res = dict(label=a.label, root=a.root, mode=a.mode, build_id=h.build_id(), ncell=n, nisurf=48, grow_on=True,
               cycles=cycles)
    with h.Context(n, synth.ZI_L8, nisurf=48, grow_on=True) as ctx:
        ctx.set_cells(gid, synth.cell_lat(gid))
        ctx.synth_params(synth.SEED)
        ctx.init_state()
        st0 = ctx.get_state()
        ctx.synth_forcing(0, synth.SEED, synth.year_day0(1901), synth.days_in_year(1901))
        ctx.sync()
        have = hasattr(ctx, "spinup")
        if a.mode == "loop":
            plain, spin = [], []
            for r in range(a.reps + 1):
                ctx.set_state(st0)
                ctx.sync()
                t0 = time.perf_counter()
                for _ in range(cycles):
                    ctx.run_year(0, 1901)
                ctx.sync(raise_on_stop=False)
                t1 = time.perf_counter()
                if r:
                    plain.append((t1 - t0) * 1e3)
                if not have:
                    continue
                ctx.set_state(st0)
                ctx.sync()
                t0 = time.perf_counter()
                out = ctx.spinup([0], 1901, max_cycles=cycles, tol_water=0.0, tol_zwt=0.0, tol_plant=0.0,
                                 freeze=True, raise_on_stop=False)
                t1 = time.perf_counter()
                if r:
                    spin.append((t1 - t0) * 1e3)
            res.update(run_year_ms=plain, run_year_ms_median=statistics.median(plain))
            print(f"{a.label} {cycles} x run_year + sync: wall ms median {statistics.median(plain):.2f} "
                  f"(min {min(plain):.2f}, max {max(plain):.2f}, {a.reps} runs)", flush=True)
            if have:
                res.update(spinup_ms=spin, spinup_ms_median=statistics.median(spin), settled=int(out["history"][:, 1].sum()),
                           cycles_run=out["cycles"])
                print(f"{a.label} h9g_spinup, {cycles} cycles, tolerances 0: wall ms median {statistics.median(spin):.2f} "
                      f"(min {min(spin):.2f}, max {max(spin):.2f}); settled {res['settled']}; difference of medians "
                      f"{statistics.median(spin) - statistics.median(plain):+.2f} ms", flush=True)
        else:
            sts = []
            for k in range(4):
                ctx.run_year(0, 1901)
                ctx.sync(raise_on_stop=False)
                sts.append(ctx.get_state())
            code = ctx.get_errors()["code"]
            ok = (code == 0) & ~np.isnan(ctx.get_annual()[2])
            d3 = drift(keys(h, sts[1], n, L), keys(h, sts[2], n, L))
            d4 = drift(keys(h, sts[2], n, L), keys(h, sts[3], n, L))
            tol = dict(tol_water=float(np.median(d3[0][ok])), tol_zwt=float(4.0 * np.median(d3[1][ok])),
                       tol_plant=float(np.median(d4[2][ok])))
            res["tolerances"] = tol
            print(f"{a.label} tolerances (medians of cycles 3 and 4 over {int(ok.sum())} cells): {tol}", flush=True)
            for freeze in (True, False):
                ctx.set_state(st0)
                ctx.launch_stats(reset=True)
                ctx.sync()
                t0 = time.perf_counter()
                out = ctx.spinup([0], 1901, max_cycles=cycles, freeze=freeze, raise_on_stop=False, **tol)
                t1 = time.perf_counter()
                stats = ctx.launch_stats()
                row = dict(freeze=int(freeze), wall_ms=(t1 - t0) * 1e3, cycles=out["cycles"], rc=out["rc"],
                           cell_years=int(sum(s["cell_years"] for s in stats.values())), launch_stats=stats,
                           history=out["history"].tolist(), active_at_end=int((out["cell_cycle"] == 0).sum()))
                res.setdefault("runs", []).append(row)
                print(f"{a.label} freeze={int(freeze)}: wall {row['wall_ms']:.1f} ms, {row['cycles']} cycles, "
                      f"{row['cell_years']} cell-years, active at the end {row['active_at_end']}", flush=True)
                print("   per kind: " + ", ".join(f"{k} {s['launches']} launches {s['cell_years']} cell-years "
                                                   f"{s['ms']:.1f} ms" for k, s in stats.items()), flush=True)
                print("   cells run / settled per cycle: " +
                      " ".join(f"{int(r[0])}/{int(r[1])}" for r in out["history"]), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
