"""Spin-up to equilibrium on the GPU (h9g_spinup, h9g_spin_kernel): everything
the call leaves -- state, annual means, STOP records, cell_cycle, history --
against the rule restated in numpy over the CPU oracle's trajectory
(tests/spinup_helpers.py), bit for bit; the list paths the environment
switches select; freeze = 0 against a plain loop of run_year; the ordered
compaction at awkward sizes through h9g_spin_selftest; recording; the layers
above.  The tolerances are chosen at test time from the oracle's own drifts
(spinup_helpers.issue_tolerances), and every test first asserts on the
emulation alone that cells retire at different cycles.  Runs on an MI355X."""
import subprocess

import numpy as np
import pytest

import hybrid9_amd as h
from oracle import port, refcase
from tests.conftest import load_golden, same_bits
from tests.daily_helpers import stop_mask_inputs
from tests.spinup_helpers import (D, F, check_meaningful, drift_of, emulate, histogram, issue_tolerances, keys_of,
                                  max_of, met_of, trajectory)

pytestmark = pytest.mark.gpu

K = 6


def _case(name, years=1):
    if name == "stop_mask":
        meta, inp = stop_mask_inputs()
    else:
        meta, inp, _ = load_golden(name)
    return meta, inp, trajectory((name, years, K), inp, years, K)


def gpu_spin(inp, years, *, evap=False, slots=None, **opts):
    """Context.spinup on the first `years` years of inp: everything it leaves."""
    p = inp["params"]
    L, n = p["theta_s"].shape[1], p["fmax"].size
    with h.Context(n, inp["zi"], nlayers=L, nisurf=inp["nisurf"], grow_on=bool(inp["grow_on"]),
                   nslots=max(2, years)) as ctx:
        ctx.set_params(p)
        if inp.get("state0") is None:
            ctx.init_state()
        else:
            ctx.set_state(inp["state0"])
        if evap:
            ctx.set_evap(True)
        d0 = 0
        for k in range(years):
            nt = h.days_in_year(inp["year0"] + k)
            ctx.push_forcing(k, inp["forcing"][:, d0:d0 + nt])
            d0 += nt
        ctx.launch_stats(reset=True)
        res = ctx.spinup(list(range(years)) if slots is None else slots, inp["year0"], raise_on_stop=False, **opts)
        return dict(res, state=ctx.get_state(), annual=ctx.get_annual(), errors=ctx.get_errors(),
                    last_error=ctx.last_error(), stats=ctx.launch_stats(), diag=ctx.get_diagnostics(),
                    kernel=ctx.kernel_name())


def check_against(out, em, tr, evap=False):
    """Everything the call left equals the emulation."""
    L, n = tr["L"], tr["n"]
    print("cycles", out["cycles"], "histogram", histogram(em, K))
    print("history (GPU):\n", out["history"])
    assert out["cycles"] == em["cycles"]
    assert np.array_equal(out["cell_cycle"], em["cell_cycle"])
    assert same_bits(out["history"], em["history"])
    assert out["rc"] == em["rc"]
    e = out["errors"]
    got = np.stack([e["code"], e["day"], e["substep"], e["value"].view(np.int32)])
    assert np.array_equal(got, em["err"])
    rows = [r for r in range(12 + L) if not (evap and r == 3)]
    assert same_bits(out["annual"][rows], em["annual"][rows])
    ran = tr["land"] & em["ok"]          # (a stopped cell's state: as tests/test_gpu_parity.py, not compared)
    st = refcase.unpack_state(out["state"], n, L)
    for f, v in em["state"].items():
        assert same_bits(st[f][ran], v[ran]), f
    if em["first_stop"] is not None:
        c, year = em["first_stop"]
        le = out["last_error"]
        assert (le["code"], le["cell"], le["year"], le["day"], le["substep"]) == \
               (int(em["err"][0, c]), c, year, int(em["err"][1, c]), int(em["err"][2, c]))
        assert np.float32(le["value"]).view(np.int32) == em["err"][3, c]
    # the diagnostics, recomputed over the rows the call left (FP64 sums of n values: n * 2^-53 relative)
    a = out["annual"].astype(D)
    live = (e["code"] == 0) & ~np.isnan(a[2])
    assert out["diag"][0] == live.sum() and out["diag"][11] == (e["code"] != 0).sum()
    terms = [a[2], a[11 + L], st["zwt"].astype(D), st["wa"].astype(D), a[0], a[1], st["LAI"].astype(D)]
    for got_sum, x in zip(out["diag"][1:8], terms):
        assert abs(got_sum - x[live].sum()) <= 1e-12 * np.abs(x[live]).sum()


LIST_PATHS = {"default": ({}, "pair1"),
              "no_pair1": ({"H9G_NO_PAIR1": "1"}, "pair11"),
              "no_pair1_no_pair11": ({"H9G_NO_PAIR1": "1", "H9G_NO_PAIR11": "1"}, "pair"),
              "solo": ({"H9G_KERNEL": "solo"}, "solo")}


@pytest.mark.parametrize("path,plant", [("default", False), ("no_pair1", False), ("no_pair1_no_pair11", False),
                                        ("solo", False), ("default", True)])
def test_c1_10x10_freeze_on_every_list_path(path, plant, monkeypatch):
    """100 cells (more than one wave, no multiple of 64), six one-year cycles:
    cycle 1 the every-cell launch, the later ones lists of the active cells."""
    env, list_kind = LIST_PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    meta, inp, tr = _case("c1_10x10")
    tol = issue_tolerances(tr, plant)
    em = emulate(tr, max_cycles=K, freeze=True, **tol)
    check_meaningful(em)
    out = gpu_spin(inp, 1, max_cycles=K, freeze=True, **tol)
    check_against(out, em, tr)
    # launches: the every-cell year of cycle 1 (and of every cycle before a cell left), then lists
    hist = em["history"]
    left = np.concatenate([[0], np.cumsum(hist[:, 1] + hist[:, 2])[:-1]])      # cells gone before cycle k
    total = int(hist[:, 0].sum())
    stats = out["stats"]
    print("launch stats", stats)
    assert sum(s["cell_years"] for s in stats.values()) == total
    assert sum(s["launches"] for s in stats.values()) == em["cycles"]
    lists = int(hist[left > 0, 0].sum())
    assert lists > 0 and (left == 0).sum() >= 1
    every = "solo" if path == "solo" else "pair"
    if list_kind != every:
        assert stats[list_kind]["cell_years"] == lists and stats[list_kind]["launches"] == (left > 0).sum()
        assert stats[every]["cell_years"] == total - lists
    else:
        assert set(stats) == {every}


def test_c1_10x10_no_freeze_equals_a_plain_loop():
    meta, inp, tr = _case("c1_10x10")
    tol = issue_tolerances(tr, False)
    em = emulate(tr, max_cycles=K, freeze=False, **tol)
    em1 = emulate(tr, max_cycles=K, freeze=True, **tol)
    check_meaningful(em1)
    assert np.array_equal(em["cell_cycle"], em1["cell_cycle"])     # the first-met cycle
    out = gpu_spin(inp, 1, max_cycles=K, freeze=False, **tol)
    check_against(out, em, tr)
    assert set(out["stats"]) == {"pair"} and out["stats"]["pair"]["launches"] == out["cycles"]
    # a second context: cycles x run_year
    p = inp["params"]
    with h.Context(tr["n"], inp["zi"], nisurf=inp["nisurf"], grow_on=bool(inp["grow_on"])) as ctx:
        ctx.set_params(p)
        ctx.init_state()
        ctx.push_forcing(0, inp["forcing"][:, :h.days_in_year(inp["year0"])])
        for _ in range(out["cycles"]):
            ctx.run_year(0, inp["year0"])
        ctx.sync()
        assert same_bits(ctx.get_state(), out["state"])
        assert same_bits(ctx.get_annual(), out["annual"])
        assert same_bits(ctx.get_diagnostics(), out["diag"])


@pytest.mark.parametrize("plant", [False, True])
def test_two_year_cycle_with_a_leap_year(plant):
    """c1_2yr_leap: 1903 and 1904 (366 days) in two resident slots."""
    meta, inp, tr = _case("c1_2yr_leap", years=2)
    tol = issue_tolerances(tr, plant)
    em = emulate(tr, max_cycles=K, **tol)
    check_meaningful(em)
    if not plant:
        assert histogram(em, K) == [3, 2, 7, 0, 2, 2, 1]
    out = gpu_spin(inp, 2, max_cycles=K, **tol)
    check_against(out, em, tr)
    assert sum(s["cell_years"] for s in out["stats"].values()) == 2 * int(em["history"][:, 0].sum())
    if plant:
        return
    with pytest.raises(ValueError):
        gpu_spin(inp, 2, slots=[1, 1], max_cycles=K, **tol)
    with pytest.raises(ValueError):
        gpu_spin(inp, 2, slots=[0, 2], max_cycles=K, **tol)
    with pytest.raises(ValueError):
        gpu_spin(inp, 2, max_cycles=2, min_cycles=3)


def test_stop_and_masked_cell():
    """8 cells, cell 2 masked, one that STOPs: the codes -1 and -2, the return
    code and h9g_last_error; the other cells go on."""
    meta, inp, tr = _case("stop_mask")
    tol = issue_tolerances(tr, False)
    em = emulate(tr, max_cycles=K, **tol)
    s = meta["stop"]
    assert em["cell_cycle"][2] == -1 and em["cell_cycle"][s["cell"]] == -2 and em["rc"] == s["code"]
    assert np.unique(em["cell_cycle"][em["cell_cycle"] > 0]).size >= 3 and (em["cell_cycle"] == 0).any()
    out = gpu_spin(inp, 1, max_cycles=K, **tol)
    check_against(out, em, tr)
    assert out["rc"] == s["code"] and out["last_error"]["cell"] == s["cell"]
    assert out["last_error"]["day"] == s["day"] and out["last_error"]["year"] == inp["year0"]
    assert f"{out['last_error']['value']:.9g}" == f"{s['value']:.9g}"
    assert out["cycles"] > int(tr["stop_cycle"][s["cell"]])
    assert np.isnan(out["annual"][:, [2, s["cell"]]]).all()
    with pytest.raises(h.ReferenceStop):
        p = inp["params"]
        with h.Context(tr["n"], inp["zi"], nisurf=inp["nisurf"], grow_on=bool(inp["grow_on"])) as ctx:
            ctx.set_params(p)
            ctx.init_state()
            ctx.push_forcing(0, inp["forcing"][:, :h.days_in_year(inp["year0"])])
            ctx.spinup([0], inp["year0"], max_cycles=2)


@pytest.mark.parametrize("plant", [False, True])
def test_c5_l10_sample(plant):
    """L = 10, NS = 24, a STOP in cycle 1: the other layer set and its kernels."""
    meta, inp, tr = _case("c5_l10_sample")
    tol = issue_tolerances(tr, plant)
    em = emulate(tr, max_cycles=K, **tol)
    check_meaningful(em)
    # (the medians are over the 48 cells that run cycle 3, without the stopped one: [16, 1, 19, 4, 2, 4, 2] for
    # tol_plant = +inf; with the oracle's continued run of the stopped cell in the median it is [17, 1, 19, 4, 2, 2, 3])
    assert (em["cell_cycle"] == -2).sum() == 1 and em["history"][0, 2] == 1
    out = gpu_spin(inp, 1, max_cycles=K, **tol)
    check_against(out, em, tr)
    assert "<10," in out["kernel"]


# ---- the kernel alone: ordered compaction at awkward sizes --------------------
def _states(n, L, active, seed=11):
    """Two packed states one cycle apart: the cells `active` drift above the
    tolerances used below, the others by less; returns (prev, cur, dicts)."""
    r = np.random.default_rng(seed + n)
    a = {f: r.uniform(1.0, 300.0, (n, w) if w > 1 else n).astype(F) for f, w in refcase.state_fields(L)}
    b = {f: np.array(v, copy=True) for f, v in a.items()}
    b["wa"] = np.where(active, a["wa"] + F(2.0) + r.uniform(0.0, 5.0, n).astype(F), a["wa"]).astype(F)
    b["zwt"] = (a["zwt"] + r.uniform(0.0, 0.25, n).astype(F)).astype(F)
    b["plant_mass"] = (a["plant_mass"] * F(1.001)).astype(F)
    return refcase.pack_state(a, L), refcase.pack_state(b, L), a, b


def _expect(a, b, L, k, stopped, tol, min_cycles=1):
    n = a["wa"].size
    d = drift_of(keys_of(a, L), keys_of(b, L))
    tested = ~stopped
    met = tested & met_of(d, k, min_cycles, **tol)
    cc = np.where(stopped, -2, np.where(met, k, 0)).astype(np.int32)
    stats = np.array([n, met.sum(), stopped.sum(), max_of(d[0], tested), max_of(d[1], tested), max_of(d[2], tested)], D)
    return np.nonzero(tested & ~met)[0].astype(np.int32), cc, stats


TOL = dict(tol_water=1.0, tol_zwt=0.5, tol_plant=0.01)


@pytest.mark.parametrize("L", [8, 10])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_selftest_list_counts_and_maxima(n, L):
    """Sizes across the wave (64) and chunk (1,024) boundaries; every third
    cell drifts above tolerance, every 50th stopped in the cycle."""
    active = np.arange(n) % 3 == 0
    stopped = np.arange(n) % 50 == 7
    prev, cur, a, b = _states(n, L, active)
    want_list, want_cc, want_stats = _expect(a, b, L, 4, stopped, TOL)
    assert n < 3 or (0 < want_list.size < n)
    got = h.spin_selftest(prev, cur, L, 4, err=np.where(stopped, 4, 0), max_cycles=9, **TOL)
    assert np.array_equal(got["list"], want_list) and (np.diff(got["list"]) > 0).all()
    assert np.array_equal(got["cell_cycle"], want_cc)
    assert same_bits(got["stats"], want_stats)


@pytest.mark.parametrize("case", ["none", "all", "last", "min_cycles"])
@pytest.mark.parametrize("n", [65, 1025, 2049])
def test_selftest_none_all_and_only_the_last_cell_active(n, case):
    active = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "last": np.arange(n) == n - 1,
              "min_cycles": np.zeros(n, bool)}[case]
    prev, cur, a, b = _states(n, 8, active)
    mc = 5 if case == "min_cycles" else 1           # (k = 4 < min_cycles: every cell stays active)
    want_list, want_cc, want_stats = _expect(a, b, 8, 4, np.zeros(n, bool), TOL, mc)
    assert want_list.size == {"none": 0, "all": n, "last": 1, "min_cycles": n}[case]
    got = h.spin_selftest(prev, cur, 8, 4, max_cycles=9, min_cycles=mc, **TOL)
    assert np.array_equal(got["list"], want_list)
    assert np.array_equal(got["cell_cycle"], want_cc)
    assert same_bits(got["stats"], want_stats)


def test_selftest_nan_and_inf_drifts():
    n, L = 130, 8
    prev, cur, a, b = _states(n, L, np.zeros(n, bool))
    a["plant_mass"][5], b["plant_mass"][5] = 0.0, 0.0          # no drift
    a["plant_mass"][70], b["plant_mass"][70] = 0.0, 1.0        # +inf
    b["wa"][129] = np.nan                                      # never settles, not in the maximum
    prev, cur = refcase.pack_state(a, L), refcase.pack_state(b, L)
    for tol in (TOL, dict(TOL, tol_plant=np.inf)):
        want_list, want_cc, want_stats = _expect(a, b, L, 2, np.zeros(n, bool), tol)
        assert want_list.tolist() == ([70, 129] if tol is TOL else [129]) and want_stats[5] == np.inf
        got = h.spin_selftest(prev, cur, L, 2, max_cycles=9, **tol)
        assert np.array_equal(got["list"], want_list) and np.array_equal(got["cell_cycle"], want_cc)
        assert same_bits(got["stats"], want_stats)


# ---- recording ----------------------------------------------------------------
def test_recording_is_refused_and_evap_is_allowed():
    meta, inp, tr = _case("c1_10x10")
    tol = issue_tolerances(tr, False)
    em = emulate(tr, max_cycles=K, **tol)
    p = inp["params"]
    nt = h.days_in_year(inp["year0"])
    with h.Context(tr["n"], inp["zi"], nisurf=inp["nisurf"], grow_on=bool(inp["grow_on"])) as ctx:
        ctx.set_params(p)
        ctx.init_state()
        ctx.push_forcing(0, inp["forcing"][:, :nt])
        ctx.set_monthly(True)
        with pytest.raises(h.H9GError, match="H9G_ESTATE"):
            ctx.spinup([0], inp["year0"], max_cycles=2)
        ctx.set_monthly(False)
        ctx.set_daily([3, 40])
        with pytest.raises(h.H9GError, match="H9G_ESTATE"):
            ctx.spinup([0], inp["year0"], max_cycles=2)
        ctx.set_daily([])
        # a plain ET loop: row evap after every cycle
        ctx.set_evap(True)
        rows = []
        for _ in range(em["cycles"]):
            ctx.run_year(0, inp["year0"])
            ctx.sync()
            rows.append(ctx.get_annual()[3])
    out = gpu_spin(inp, 1, evap=True, max_cycles=K, **tol)
    check_against(out, em, tr, evap=True)
    assert "_et_kernel" in out["kernel"]
    want = np.array([rows[em["last"][c] - 1][c] for c in range(tr["n"])], F)
    assert same_bits(out["annual"][3], want) and (want > 0).all()


# ---- the layers above ----------------------------------------------------------
def _rounded(tol):
    """Tolerances a namelist carries exactly: six significant digits."""
    return {k: float(f"{v:.6g}") for k, v in tol.items()}


def test_run_with_spinup_and_the_fortran_host(tmp_path):
    from tests.test_fortran_host import _build
    meta, inp, tr = _case("c1_10x10")
    tol = _rounded(issue_tolerances(tr, True))
    em = emulate(tr, max_cycles=K, **tol)
    check_meaningful(em)
    common = dict(zi=inp["zi"], params=inp["params"], forcing=inp["forcing"], nisurf=inp["nisurf"],
                  year0=inp["year0"], nyears=inp["nyears"], grow_on=bool(inp["grow_on"]))
    out = h.run(spinup=dict(years=1, max_cycles=K, **tol), **common)
    sp = out["spinup"]
    assert sp["cycles"] == em["cycles"] and np.array_equal(sp["cell_cycle"], em["cell_cycle"])
    assert same_bits(sp["history"], em["history"]) and sp["rc"] == 0 and out["rc"] == 0
    # the run proper: its years from the spun-up state, as the oracle runs them
    ref = port.run(zi=inp["zi"], params=inp["params"], forcing=inp["forcing"], nisurf=inp["nisurf"],
                   year0=inp["year0"], nyears=inp["nyears"], grow_on=int(inp["grow_on"]), state0=em["state"],
                   nthreads=16)
    assert same_bits(out["annual"], ref["annual"])
    assert same_bits(out["state"], refcase.pack_state(ref["state"], tr["L"]))
    plain = h.run(**common)
    assert "spinup" not in plain and not same_bits(plain["state"], out["state"])
    # the Fortran host on the same case
    exe = _build()
    case = tmp_path / "case"
    refcase.write_case(case, zi=inp["zi"], params=inp["params"], forcing=inp["forcing"], nisurf=inp["nisurf"],
                       year0=inp["year0"], nyears=inp["nyears"], grow_on=inp["grow_on"], state0=None)
    nml = tmp_path / "h9gpu.nml"
    nml.write_text(f"&h9gpu\n input_mode='case', case_dir='{case}', out_dir='{tmp_path}', cell_order=0,\n"
                   f" spinup_cycles={K}, spinup_years=1, spinup_min_cycles=1, spinup_freeze=1,\n"
                   f" spinup_tol_water={tol['tol_water']:.6g}d0, spinup_tol_zwt={tol['tol_zwt']:.6g}d0,\n"
                   f" spinup_tol_plant={tol['tol_plant']:.6g}d0\n/\n")
    r = subprocess.run([str(exe), str(tmp_path / "no_driver.txt"), str(nml)], capture_output=True, text=True,
                       timeout=600)
    assert "completed successfully" in r.stdout, r.stdout + r.stderr
    assert same_bits(np.fromfile(tmp_path / "state_end.f32", F), out["state"])
    assert np.array_equal(np.fromfile(tmp_path / "spinup_cycle.i32", np.int32), sp["cell_cycle"])
    assert same_bits(np.fromfile(tmp_path / "annual.f32", F).reshape(out["annual"].shape), out["annual"])
    lines = [ln.split() for ln in (tmp_path / "spinup.txt").read_text().splitlines()]
    assert len(lines) == sp["cycles"]
    got = np.array([[float(v) for v in ln[1:]] for ln in lines])
    assert [int(ln[0]) for ln in lines] == list(range(1, sp["cycles"] + 1))
    assert same_bits(got, sp["history"])
