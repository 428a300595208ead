"""Where the water table of tools/tail_probe.py's cells is, from day records:
per simulated year the share of cell-days that end with the water table below
the column (zwt > zi(L)/1000, jwt == L).  A substep that starts there keeps
the water-table chain on the one-column kernel's main wave (h9g_pair.h
front_year_pair, H9G_P1_SIDE); one that starts in the column hands it to the
second wave.  Day resolution: a day's 48 substeps are counted by the day's
last one, so a cell that crosses the column's bottom within a day is off by
part of that day.

    python tools/tail_share.py [ncell] [years]     (env: H9G_KERNEL, H9G_LIB)
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import bench  # noqa: E402
import hybrid9_amd as h  # noqa: E402
from hybrid9_amd import synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 128
ny = int(sys.argv[2]) if len(sys.argv) > 2 else 6
pl = bench.plan("config2", 0, ny)
idx = [(k * 7919) % pl["gid"].size for k in range(n)]      # tail_probe.py's cells
gid, lat = pl["gid"][idx], pl["lat"][idx]
L = pl["L"]
bottom = np.float32(pl["zi"][L]) / np.float32(1000.0)
ctx = h.Context(n, pl["zi"], nlayers=L, nisurf=pl["ns"], grow_on=pl["grow_on"], nslots=pl["nslots"])
ctx.set_cells(gid, lat)
ctx.synth_params(pl["seed"])
ctx.init_state()
ctx.set_evap(True)
ctx.set_days(True)
for slot, y in enumerate(pl["slot_year"]):
    ctx.synth_forcing(slot, pl["seed"], synth.year_day0(y), synth.days_in_year(y))
ctx.sync()
print(f"tail share: {n} cells, kernel {ctx.kernel_name()}, column bottom {bottom} m", flush=True)
for s, y in enumerate(pl["years"]):
    ctx.run_year(pl["slot_of_step"][s], y)
    ctx.sync(raise_on_stop=False)
    zwt = ctx.get_days(0)[:, 4, :]
    ok = ~np.isnan(zwt)
    below = (zwt > bottom) & ok
    per_cell = below.sum(0) / np.maximum(ok.sum(0), 1)
    print(f"{y} below the column: {below.sum() / ok.sum():.3f} of {int(ok.sum())} cell-days; cells always in the column "
          f"{int((per_cell == 0).sum())}, always below {int((per_cell == 1).sum())}, both {int(((per_cell > 0) & (per_cell < 1)).sum())}",
          flush=True)
