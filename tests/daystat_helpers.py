"""Shared by tests/test_daystat_host.py and tests/test_gpu_daystat.py: the day
statistics of include/h9g.h (h9g_get_daystats) stated a third time, as a plain
double loop (``day_stats_loop``; the header's table and hybrid9_amd.day_stats
are the other two); the host build of hybrid9_amd/csrc/h9g_stat.h
(tests/csrc/host_stat.cpp) with the year cut wherever the caller says; the
oracle's day records of three goldens with thresholds taken from the records
themselves; and hand-made records built to go wrong where a merge of segments
can go wrong."""
from __future__ import annotations

import ctypes as C
import math
import subprocess

import numpy as np

import hybrid9_amd as h
from oracle import port
from tests.helpers import BUILD, ROOT

F = np.float32
D = np.float64
NS = 17                  # H9G_NDAYSTAT
COUNT_ROWS = (4, 10, 11, 13, 16)     # q_days, dry_days, dry_spell, wet_days, green_days
WS = (4, 8, 16)          # the workgroups h9g_daystat_kernel is built with (waves = slices of a year)
HAND_THR = dict(q_thr=2.0, theta_thr=0.25, zwt_thr=500.0, lai_thr=1.0)

_lib = None
_cache = {}


# ---- the table, as a double loop ------------------------------------------------
def day_stats_loop(records, *, q_thr, theta_thr, zwt_thr, lai_thr):
    """(nday, 7, n) float32 -> (17, n) float64, cell by cell and day by day.
    Python floats are IEEE doubles and hold every float32 exactly, so a
    comparison of two of them is the float32 comparison."""
    rec = np.asarray(records, F)
    nt, _, n = rec.shape
    q_thr, theta_thr, zwt_thr, lai_thr = (float(F(v)) for v in (q_thr, theta_thr, zwt_thr, lai_thr))
    out = np.empty((NS, n), D)
    nan = float("nan")
    for c in range(n):
        col = rec[:, :, c].astype(D).tolist()        # (exact)
        ndays = q_days = dry_days = wet_days = green_days = 0
        spell = run = 0
        q_max = q7_min = e_max = w_min = w_max = t_min = z_min = l_max = nan
        q_max_day = w_min_day = l_max_day = -1
        for d in range(nt):
            r = col[d]
            if not any(math.isnan(v) for v in r):
                ndays += 1
            q = r[0] - (col[d - 1][0] if d > 0 else 0.0)
            e = r[1] - (col[d - 1][1] if d > 0 else 0.0)
            if not math.isnan(q):
                if math.isnan(q_max) or q > q_max:
                    q_max, q_max_day = q, d
                if q >= q_thr:
                    q_days += 1
            if d >= 6:
                q7 = r[0] - (col[d - 7][0] if d > 6 else 0.0)
                if not math.isnan(q7) and (math.isnan(q7_min) or q7 < q7_min):
                    q7_min = q7
            if not math.isnan(e) and (math.isnan(e_max) or e > e_max):
                e_max = e
            w, t, z, lai = r[2], r[3], r[4], r[6]
            if not math.isnan(w):
                if math.isnan(w_min) or w < w_min:
                    w_min, w_min_day = w, d
                if math.isnan(w_max) or w > w_max:
                    w_max = w
            if not math.isnan(t) and (math.isnan(t_min) or t < t_min):
                t_min = t
            if not math.isnan(t) and t < theta_thr:
                dry_days += 1
                run += 1
                spell = max(spell, run)
            else:
                run = 0
            if not math.isnan(z):
                if math.isnan(z_min) or z < z_min:
                    z_min = z
                if z <= zwt_thr:
                    wet_days += 1
            if not math.isnan(lai):
                if math.isnan(l_max) or lai > l_max:
                    l_max, l_max_day = lai, d
                if lai >= lai_thr:
                    green_days += 1
        out[:, c] = (ndays, q_max, q_max_day, q7_min, q_days, e_max, w_min, w_min_day, w_max, t_min, dry_days, spell,
                     z_min, wet_days, l_max, l_max_day, green_days)
    return out


# ---- the host build of h9g_stat.h -------------------------------------------------
def stat_lib():
    global _lib
    if _lib is None:
        src = ROOT / "tests" / "csrc" / "host_stat.cpp"
        out = BUILD / "libhost_stat.so"
        deps = [src, ROOT / "include" / "h9g.h"] + list((ROOT / "hybrid9_amd" / "csrc").glob("*.h"))
        if not out.exists() or out.stat().st_mtime < max(d.stat().st_mtime for d in deps):
            BUILD.mkdir(exist_ok=True)
            subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-fPIC", "-shared",
                            str(src), "-o", str(out)], check=True)
        _lib = C.CDLL(str(out))
        ip = C.POINTER(C.c_int)
        _lib.h9k_host_stat.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, ip, C.c_int,
                                       C.POINTER(h._StatOpts), C.POINTER(C.c_double)]
        _lib.h9k_host_stat_cuts.argtypes = [C.c_int, C.c_int, ip]
    return _lib


def host_stat(records, cuts=(), tree=False, **thr):
    """stat_day / stat_merge / stat_rows on the host: the year cut at `cuts`
    (strictly increasing days in (0, nday)), every slice summarised on its own
    and the summaries merged left to right (tree: right to left) -> (17, n)."""
    rec = np.ascontiguousarray(records, F)
    nt, _, n = rec.shape
    cu = np.ascontiguousarray(cuts, np.int32)
    out = np.empty((NS, n), D)
    o = h.daystat_opts(**thr)
    rc = stat_lib().h9k_host_stat(n, nt, rec.ctypes.data_as(C.POINTER(C.c_float)), cu.size,
                                  cu.ctypes.data_as(C.POINTER(C.c_int)), int(tree), C.byref(o),
                                  out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0, "h9k_host_stat refused its arguments"
    return out


def kernel_cuts(nt, nseg):
    """The cuts of h9g_daystat_kernel's nseg slices of a year of nt days."""
    cu = np.zeros(max(nseg, 1), np.int32)
    m = stat_lib().h9k_host_stat_cuts(int(nt), int(nseg), cu.ctypes.data_as(C.POINTER(C.c_int)))
    return cu[:m].copy()


def cut_sets(nt, seed=0):
    """The cuts the associativity tests compare: none, the kernel's for every W
    built, every day on its own, and 20 random ones."""
    rng = np.random.default_rng(seed)
    sets = [("one slice", np.zeros(0, np.int32))]
    sets += [(f"W = {w}", kernel_cuts(nt, w)) for w in WS]
    sets.append(("single days", np.arange(1, nt, dtype=np.int32)))
    for k in range(20):
        m = int(rng.integers(1, 40))
        sets.append((f"random {k}", np.sort(rng.choice(np.arange(1, nt), size=m, replace=False)).astype(np.int32)))
    return sets


# ---- the oracle's records ----------------------------------------------------------
def golden_records(name):
    """The oracle's day records (days_helpers.port_days) of a golden ->
    (inputs, records (nyears, 366, 7, n)).  "stop_ns24" is the golden with cell
    2 masked (daily_helpers.stop_mask_inputs); the oracle's trace knows no
    convention for the cell that stops and the masked one, so theirs is put
    on here (include/h9g.h: NaN from the STOP day on; NaN throughout)."""
    if name not in _cache:
        from tests.conftest import load_golden
        from tests.daily_helpers import stop_mask_inputs
        from tests.days_helpers import port_days
        if name == "stop_ns24":
            meta, inp = stop_mask_inputs()
        else:
            meta, inp, _ = load_golden(name)
        rec, ref = port_days(**inp)
        if name == "stop_ns24":
            s = meta["stop"]
            assert ref["rc"] == s["code"] and ref["err"]["cell"] == s["cell"] and inp["nyears"] == 1
            rec[0, ref["err"]["day"]:, :, s["cell"]] = np.nan
            land = np.array([port._mask_sum(t) > F(1.0e-8) for t in inp["params"]["theta_s"]])
            assert not land[2] and land.sum() == land.size - 1
            rec[..., ~land] = np.nan
        else:
            assert ref["rc"] == 0
        _cache[name] = (inp, rec)
    return _cache[name]


# The quantile of each threshold's row over the golden's cells and days: the
# median for rows 3, 4 and 6 and the 90th percentile of q, as a rule.
QUANTILES = dict(q_thr=0.9, theta_thr=0.5, zwt_thr=0.5, lai_thr=0.5)
# Where a golden cannot meet check_meaningful for a row at that quantile, the
# row takes the quantile named here (the assertion stays as it is):
#   c1_2yr_leap, q: runoff is concentrated in a few of its 17 cells -- 70 % of
#   its cell-days run off less than 4e-4 mm, and the 90th percentile (7.3
#   mm/day) is reached in only 8 of the 34 cell-years (0.24 of them); at the
#   70th percentile half of the cell-years have runoff days and days without.
QUANTILES_OF = {"c1_2yr_leap": dict(q_thr=0.7)}


def thresholds_of(name, rec):
    """The golden's thresholds, from its own records (finite values of every
    year): QUANTILES of q, theta1, zwt and LAI.  Printed."""
    qs = dict(QUANTILES, **QUANTILES_OF.get(name, {}))
    rec = np.asarray(rec, F)
    s = rec[:, :, 0].astype(D)
    q = np.diff(s, axis=1, prepend=np.zeros_like(s[:, :1]))
    pools = dict(q_thr=q, theta_thr=rec[:, :, 3], zwt_thr=rec[:, :, 4], lai_thr=rec[:, :, 6])
    thr = {}
    for k, v in pools.items():
        v = np.asarray(v, D)
        thr[k] = float(F(np.quantile(v[np.isfinite(v)], qs[k])))
    print(f"{name}: thresholds {thr} (quantiles {qs})")
    return thr


def check_meaningful(name, stats):
    """A count that is 0 or every day in every cell shows nothing: each of the
    five counting rows is neither 0 nor ndays in at least a quarter of the
    cells that ran (ndays > 0), over the golden's years."""
    stats = np.asarray(stats)                     # (nyears, 17, n)
    ran = stats[:, 0] > 0
    assert ran.any()
    for r in COUNT_ROWS:
        mid = ran & (stats[:, r] > 0) & (stats[:, r] < stats[:, 0])
        share = mid.sum() / ran.sum()
        print(f"{name}: row {r} ({h.DAYSTAT_FIELDS[r]}) strictly between 0 and ndays in {mid.sum()} of "
              f"{ran.sum()} cell-years")
        assert share >= 0.25, (name, h.DAYSTAT_FIELDS[r], share)


# ---- hand-made records ---------------------------------------------------------------
def handmade():
    """8 cells x 366 days (thresholds HAND_THR), every value exact in float32:
      0  dry runs across every slice boundary of W = 4, 8 and 16, the longest
         (days 170..199) across the middle of the year
      1  dry all year; q and e tied at zero, with a -0 among the +0
      2  equal maxima of q on days 182 and 183 (a boundary of W = 4), of LAI on
         days 90 and 91, equal minima of W on days 273 and 274
      3  q largest on day 0; LAI largest and W smallest on the last day
      4  q7 smallest in the first window (d = 6); zwt tied at +0 then -0
      5  q7 smallest in the window of days 180..186, across the boundary 183;
         LAI tied at -0 then +0
      6  a STOP on day 3: no 7-day window
      7  a STOP on day 0: no day at all"""
    nt, n = 366, 8
    d = np.arange(nt)
    rec = np.zeros((nt, 7, n), F)
    q = (1 + (d * 7) % 5).astype(D)               # 1..5 mm a day
    e = (1 + (d * 3) % 4).astype(D) * 0.5
    for c in range(n):
        rec[:, 0, c] = np.cumsum(q)
        rec[:, 1, c] = np.cumsum(e)
        rec[:, 2, c] = 300 + (d * 11) % 37
        rec[:, 3, c] = 0.3 + 0.03125 * ((d * 5) % 3)
        rec[:, 4, c] = 400 + 8 * ((d * 13) % 29)
        rec[:, 5, c] = 4000 + d
        rec[:, 6, c] = 0.5 + 0.0625 * ((d * 3) % 17)
    bounds = sorted({int(b) for w in WS for b in kernel_cuts(nt, w)})
    assert 183 in bounds and 91 in bounds and 274 in bounds and len(bounds) == 15
    for b in bounds:                              # cell 0
        rec[b - 2:b + 2, 3, 0] = 0.125
    rec[170:200, 3, 0] = 0.125
    rec[:, 3, 1] = 0.125                          # cell 1
    rec[:, 0, 1] = 0.0
    rec[100, 0, 1] = -0.0
    rec[:, 1, 1] = 0.0
    rec[0, 1, 1] = -0.0
    q2 = q.copy()                                 # cell 2
    q2[182] = q2[183] = 50.0
    rec[:, 0, 2] = np.cumsum(q2)
    rec[90, 6, 2] = rec[91, 6, 2] = 7.0
    rec[273, 2, 2] = rec[274, 2, 2] = 100.0
    q3 = q.copy()                                 # cell 3
    q3[0] = 100.0
    rec[:, 0, 3] = np.cumsum(q3)
    rec[365, 6, 3] = 9.0
    rec[365, 2, 3] = 50.0
    q4 = q.copy() + 1.0                           # cell 4
    q4[:7] = 0.0
    rec[:, 0, 4] = np.cumsum(q4)
    rec[:, 4, 4] = 5.0
    rec[10, 4, 4] = 0.0
    rec[200, 4, 4] = -0.0
    q5 = q.copy() + 1.0                           # cell 5
    q5[180:187] = 0.0
    rec[:, 0, 5] = np.cumsum(q5)
    rec[:, 6, 5] = -1.0
    rec[50, 6, 5] = -0.0
    rec[300, 6, 5] = 0.0
    rec[3:, :, 6] = np.nan                        # cell 6
    rec[:, :, 7] = np.nan                         # cell 7
    assert np.array_equal(rec[:, 0, :6].astype(D), np.round(rec[:, 0, :6].astype(D)))   # (the sums stayed exact)
    return rec


def check_handmade(stats):
    """What the hand-made records were made for, on their 17 rows (17, 8)."""
    s = np.asarray(stats)
    f = {k: s[i] for i, k in enumerate(h.DAYSTAT_FIELDS)}
    sign = np.signbit
    assert f["dry_spell"][0] == 30 and f["dry_days"][0] == 30 + 4 * 14
    assert f["dry_spell"][1] == 366 and f["dry_days"][1] == 366
    assert f["q_max"][1] == 0 and not sign(f["q_max"][1]) and f["q_max_day"][1] == 0
    assert f["e_max"][1] == 0 and sign(f["e_max"][1])
    assert f["q_max"][2] == 50 and f["q_max_day"][2] == 182
    assert f["lai_max"][2] == 7 and f["lai_max_day"][2] == 90
    assert f["w_min"][2] == 100 and f["w_min_day"][2] == 273
    assert f["q_max"][3] == 100 and f["q_max_day"][3] == 0
    assert f["lai_max_day"][3] == 365 and f["w_min_day"][3] == 365
    assert f["q7_min"][4] == 0 and f["zwt_min"][4] == 0 and not sign(f["zwt_min"][4])
    assert f["q7_min"][5] == 0 and f["lai_max"][5] == 0 and sign(f["lai_max"][5]) and f["lai_max_day"][5] == 50
    assert f["ndays"][6] == 3 and np.isnan(f["q7_min"][6]) and f["q_max_day"][6] in (0, 1, 2)
    assert f["ndays"][7] == 0
    ext = [i for i, k in enumerate(h.DAYSTAT_FIELDS) if not k.endswith("_days") and k not in ("ndays", "dry_spell")]
    for i in ext:
        want_day = h.DAYSTAT_FIELDS[i].endswith("_day")
        assert (s[i, 7] == -1) if want_day else np.isnan(s[i, 7]), h.DAYSTAT_FIELDS[i]
    assert (s[list(COUNT_ROWS), 7] == 0).all()


def random_records(n, nt, seed):
    """n cells x nt days of few distinct values (many ties), with NaN tails of
    random length (some cells none, some the whole year)."""
    rng = np.random.default_rng(seed)
    rec = np.empty((nt, 7, n), F)
    rec[:, 0] = np.cumsum(rng.integers(0, 6, (nt, n)), axis=0)
    rec[:, 1] = np.cumsum(rng.integers(0, 4, (nt, n)) * 0.25, axis=0)
    rec[:, 2] = 300 + rng.integers(0, 12, (nt, n))
    rec[:, 3] = 0.125 * rng.integers(0, 5, (nt, n))
    rec[:, 4] = 100.0 * rng.integers(0, 9, (nt, n))
    rec[:, 5] = 4000 + rng.integers(0, 100, (nt, n))
    rec[:, 6] = 0.25 * rng.integers(0, 9, (nt, n))
    stop = rng.integers(0, 2 * nt, n)              # (about half of the cells complete the year)
    stop[rng.integers(0, n, max(n // 20, 1))] = 0
    for c in range(n):
        rec[stop[c]:, :, c] = np.nan
    return rec
