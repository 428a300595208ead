"""The hand-over of the one-column kernel's two waves per column
(front_year_pair and cell_year_pair, h9g_pair.h; h9g_pair1f_kernel), restated
and checked on the host for L = 8 and 10.

A workgroup is one column: the main wave runs today's one-column substep
without its front, the front wave the front.  They share the column's LDS
block and meet at two workgroup barriers per substep:

  interval          main wave                         front wave
  (b2, b1]  "post"  writes smp(1..L), h2o(1), zwt,    reads nothing, writes nothing
                    go; day constants, plant state,
                    rootr at a day's start and end
  (b1, b2]  "eval"  reads none of the words below;    reads the posted words and the
                    writes theta(1..L)                block's fields; writes FrontRes
  after b2          reads FrontRes                    --

The front wave has no trip counts: after every barrier 1 it reads go and
leaves when it is set, which the main wave does at each exit of its year loop
(a STOP code, H9G_ERR_NOSNAP_K, a STOP of the exact re-run, the year's end).
This file is the protocol written down a second time, as tests/test_pair1_tasks.py
writes down the task map: a model in Python, checked for consistency with
itself.  Only the order of the hand-over words is read from the header; the
model cannot notice the device code posting another word, moving barrier 2 or
raising a STOP before it.  That the device code keeps the protocol is what
tests/test_gpu_pair1_front.py checks, by results and by not hanging.
The model's checks: the words are distinct and lie behind theta in the block, in the
header's order; in no interval does one wave write a word the other reads or
writes; and for every way a year can end both waves pass the same number of
barriers, the front wave never evaluating a substep the main wave does not
run."""
from __future__ import annotations

import re
from pathlib import Path

import pytest

LS = (8, 10)
HEADER = Path(__file__).resolve().parents[1] / "hybrid9_amd" / "csrc" / "h9g_pair.h"
RES = ("HO_SURF", "HO_TRAN", "HO_EVG", "HO_INFL")            # FrontRes: qflx_surf, tran, evg, qflx_infl


def words(L):
    """name -> float offset from the end of the block's theta rows."""
    w = {f"HO_SMP{i}": i - 1 for i in range(1, L + 1)}
    k = L
    for name in ("HO_H2O1", "HO_ZWT", "HO_GO", "HO_PAD", *RES):
        w[name] = k
        k += 1
    w["HO_END"] = k
    return w


POSTED = lambda L: [f"HO_SMP{i}" for i in range(1, L + 1)] + ["HO_H2O1", "HO_ZWT", "HO_GO"]   # noqa: E731
# the block's own fields the front reads (written by the main wave's day_consts, GROW, park)
DAY_FIELDS = ["PS_DAY", "PS_DR", "PF_ROOTR", "PS_LAI"]


def accesses(L):
    """interval -> wave -> (reads, writes)."""
    posted, res = POSTED(L), list(RES)
    return {
        "post": {"main": (set(res), set(posted) | set(DAY_FIELDS)), "front": (set(), set())},
        "eval": {"main": (set(), {"TH0"}), "front": (set(posted) | set(DAY_FIELDS), set(res))},
    }


@pytest.mark.parametrize("L", LS)
def test_words_are_distinct_whole_rows_in_the_headers_order(L):
    w = words(L)
    offs = [v for k, v in w.items() if k != "HO_END"]
    assert sorted(offs) == list(range(w["HO_END"]))            # dense, no word twice
    assert w["HO_END"] % 2 == 0                                 # whole rows of the two-lane block
    assert w["HO_END"] == L + 8
    text = HEADER.read_text()
    m = re.search(r"HO_SMP = TH0 \+ L,(.*?)HO_END", text, re.S)
    assert m, "the hand-over enum of PairStore"
    names = ["HO_SMP"] + re.findall(r"(HO_[A-Z0-9]+)", m.group(1))
    assert names == ["HO_SMP", "HO_H2O1", "HO_SMP", "HO_ZWT", "HO_GO", "HO_PAD", *RES]   # (HO_H2O1 = HO_SMP + L)
    mine = [k for k in w if not k.startswith("HO_SMP") and k != "HO_END"]
    assert mine == ["HO_H2O1", "HO_ZWT", "HO_GO", "HO_PAD", *RES]


@pytest.mark.parametrize("L", LS)
def test_no_interval_has_a_word_written_by_one_wave_and_touched_by_the_other(L):
    for name, iv in accesses(L).items():
        (mr, mw), (fr, fw) = iv["main"], iv["front"]
        assert not (mw & (fr | fw)), (name, mw & (fr | fw))
        assert not (fw & (mr | mw)), (name, fw & (mr | mw))
    a = accesses(L)
    # every word one wave reads was written by the other in the interval before
    assert a["eval"]["front"][0] <= a["post"]["main"][1]
    assert a["post"]["main"][0] <= a["eval"]["front"][1]
    # the front's inputs: the previous substep's smp of every layer, h2osoi_liq(1), zwt
    assert len(POSTED(L)) == L + 3


def main_wave(nsub, stop_at):
    """The main wave's barriers over a year of nsub substeps; stop_at: the
    substep (0-based) whose code ends the year, or None."""
    seq = []
    for k in range(nsub):
        seq += [("b1", 0), ("b2", None)]                        # front_post (go = 0), barrier 1; barrier 2
        if stop_at == k:                                        # a code, known after barrier 2
            break
    seq.append(("b1", 1))                                       # front_done
    return seq


def front_wave(go_words):
    """The front wave's barriers, following the go words it reads after each
    barrier 1; the substeps it evaluated."""
    seq, done = [], 0
    for go in go_words:
        seq.append("b1")
        if go:
            return seq, done
        done += 1
        seq.append("b2")
    raise AssertionError("the front wave waits at a barrier 1 the main wave never reaches")


@pytest.mark.parametrize("nsub", [1, 2, 24 * 365, 48 * 366])
def test_both_waves_pass_the_same_barriers_on_every_exit(nsub):
    stops = [None, 0, nsub - 1] + ([1, nsub // 2] if nsub > 2 else [])
    for stop_at in stops:
        m = main_wave(nsub, stop_at)
        f, done = front_wave([go for b, go in m if b == "b1"])
        assert [b for b, _ in m] == f, stop_at
        ran = nsub if stop_at is None else stop_at + 1
        assert done == ran, stop_at
        assert m[-1] == ("b1", 1) and [go for b, go in m if b == "b1"].count(1) == 1
