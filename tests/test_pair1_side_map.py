"""The hand-over of the water-table chain between the one-column kernel's two
waves per column (H9G_P1_SIDE; hydrology_pair ROLE_MAINS / ROLE_CHAIN,
front_year_pair and cell_year_pair in h9g_pair.h), restated and checked on the
host for L = 8 and 10, in the manner of tests/test_pair1_front_map.py, whose
two-barrier protocol this one extends.

Three workgroup barriers per substep.  Both waves decide from the posted zwt
whose the substep's chain (recharge through the zwt clamps) is: the second
wave's when the substep starts with the water table in the column (jwt < L),
the main wave's when it starts below it (jwt == L).

  interval          main wave                          second wave
  (b3, b1]  "post"  reads the chain's results (jwt <   reads nothing, writes nothing
                    L); writes smp, h2o(1), zwt, go
                    and HS_WA; the day's fields
  (b1, b2]  "eval"  writes theta, then the chain's     reads the posted words, the
                    operands HS_P0 .. HS_RZQ           day's fields; writes FrontRes
  (b2, b3]  "side"  reads FrontRes; the sweep; its     reads HS_WA .. HS_RZQ, zwt, the
                    own chain when jwt == L            parameter fields; writes the
                                                       results HS_ZWT .. HS_R1

A STOP of the main wave between barriers 2 and 3 (the sweep's STOPs 1 and 2)
passes barrier 3 on its way out; the second wave's STOP 3 travels in HS_CODE
and HS_ERRV and is returned by the main wave after barrier 3; every other
code (the balance's STOP 4, H9G_ERR_NOSNAP_K, a STOP of the exact re-run) is
known after barrier 3.  Every exit then passes front_done: go = 1, barrier 1.

This file is a model in Python, checked for consistency with itself; only the
order of the new words is read from the header.  That the device code keeps
the protocol is what tests/test_gpu_pair1_side.py checks, by results and by
not hanging.  The model's checks: the new words are distinct, start at HO_END
and fill whole rows; in no interval does one wave write a word the other reads
or writes, and every word a wave reads was written by the other in an earlier
interval of the same substep cycle; and for every way a year can end, and both
kinds of substep, both waves pass the same barriers."""
from __future__ import annotations

import itertools
import re
from pathlib import Path

import pytest

from tests.test_pair1_front_map import DAY_FIELDS, POSTED, RES, words as front_words

LS = (8, 10)
HEADER = Path(__file__).resolve().parents[1] / "hybrid9_amd" / "csrc" / "h9g_pair.h"
OPERANDS = ["HS_WA", "HS_P0", "HS_PY", "HS_RSMP", "HS_RZQ"]                 # main -> second wave
RESULTS = ["HS_ZWT", "HS_WAO", "HS_RSUB", "HS_JWT", "HS_FLAG", "HS_CODE", "HS_ERRV",
           "HS_I0", "HS_R0", "HS_I1", "HS_R1"]                              # second wave -> main
ORDER = [*OPERANDS, "HS_PAD0", *RESULTS, "HS_PAD1"]
PARAMS = ["PF_TS", "PF_HKS", "PF_PSI", "PF_NINVB", "PF_RPSI0", "PF_RPSI1", "ZT"]   # written before the year only


def words(L):
    """name -> float offset from the end of the block's theta rows, the front's words first."""
    w = front_words(L)
    k = w.pop("HO_END")
    for name in ORDER:
        w[name] = k
        k += 1
    w["HS_END"] = k
    return w


def accesses(L):
    """interval -> wave -> (reads, writes), for a substep of either kind: the
    union over jwt < L and jwt == L (a word one kind leaves alone is free in
    the other too)."""
    posted, res = set(POSTED(L)), set(RES)
    return {
        "post": {"main": (set(RESULTS), posted | {"HS_WA"} | set(DAY_FIELDS)), "side": (set(), set())},
        "eval": {"main": (set(), {"TH0", "HS_P0", "HS_PY", "HS_RSMP", "HS_RZQ"}),
                 "side": (posted | set(DAY_FIELDS), res)},
        "side": {"main": (res | set(PARAMS), set()),
                 "side": (set(OPERANDS) | {"HO_ZWT"} | set(PARAMS), set(RESULTS))},
    }


@pytest.mark.parametrize("L", LS)
def test_the_new_words_are_distinct_whole_rows_after_the_fronts(L):
    w, f = words(L), front_words(L)
    mine = [k for k in w if k.startswith("HS_") and k != "HS_END"]
    assert mine == ORDER and len(set(ORDER)) == len(ORDER)
    assert [w[k] for k in mine] == list(range(f["HO_END"], w["HS_END"]))     # dense, from HO_END, no word twice
    assert (w["HS_END"] - f["HO_END"]) % 2 == 0                              # whole rows of the two-lane block
    assert w["HS_I1"] == w["HS_I0"] + 2 and w["HS_R1"] == w["HS_R0"] + 2     # visit k's pair: HS_I0 + 2k, HS_R0 + 2k
    text = HEADER.read_text()
    m = re.search(r"HS_WA = HO_END,(.*?)HS_END", text, re.S)
    assert m, "the chain's enum of PairStore"
    assert ["HS_WA"] + re.findall(r"(HS_[A-Z0-9]+)", m.group(1)) == ORDER
    # the front's enum is as tests/test_pair1_front_map.py reads it: the new words are not in it
    m = re.search(r"HO_SMP = TH0 \+ L,(.*?)HO_END", text, re.S)
    assert m and "HS_" not in m.group(1)


@pytest.mark.parametrize("L", LS)
def test_no_interval_has_a_word_written_by_one_wave_and_touched_by_the_other(L):
    a = accesses(L)
    for name, iv in a.items():
        (mr, mw), (sr, sw) = iv["main"], iv["side"]
        assert not (mw & (sr | sw)), (name, mw & (sr | sw))
        assert not (sw & (mr | mw)), (name, sw & (mr | mw))
    # what a wave reads of the other's, the other wrote in an earlier interval of the cycle post, eval, side, post
    main_w = a["post"]["main"][1] | a["eval"]["main"][1]
    assert a["eval"]["side"][0] <= a["post"]["main"][1]
    assert a["side"]["side"][0] - set(PARAMS) <= main_w
    assert a["side"]["main"][0] - set(PARAMS) <= a["eval"]["side"][1]
    assert a["post"]["main"][0] <= a["side"]["side"][1]
    # the chain's operands: the two single powers, smp and zq of layer max(jwt, 1), wa (zwt is the front's word)
    assert len(OPERANDS) == 5 and "HO_ZWT" in POSTED(L)


# ways a substep can end the year
AFTER_B3 = "after_b3"      # a code known after barrier 3: STOP 3 from HS_CODE, STOP 4, NOSNAP, the exact re-run's
MID = "mid"                # the sweep's STOP 1 or 2, between barriers 2 and 3


def main_wave(kinds, stop_at, how):
    """The main wave's barriers over a year whose substep k starts with the
    water table in the column (kinds[k]) or below it; stop_at: the substep
    (0-based) whose code ends the year, or None; how: AFTER_B3 or MID."""
    seq = []
    for k, inside in enumerate(kinds):
        seq += [("b1", 0), ("b2", None)]                        # front_post (go = 0), barrier 1; barrier 2
        if stop_at == k and how == MID:
            seq.append(("b3", None))                            # STOP_RET: the barrier on the way out
            break
        # the sweep; its own chain when not inside; then barrier 3, and the rows when inside
        seq.append(("b3", None))
        if stop_at == k:
            break
    seq.append(("b1", 1))                                       # front_done
    return seq


def second_wave(go_words, kinds):
    """The second wave's barriers, following the go words it reads after each
    barrier 1; the substeps whose front and whose chain it evaluated."""
    seq, fronts, chains = [], 0, 0
    for k, go in enumerate(go_words):
        seq.append("b1")
        if go:
            return seq, fronts, chains
        fronts += 1
        seq.append("b2")
        if kinds[k]:
            chains += 1                                         # a STOP 3 here is posted, not returned
        seq.append("b3")
    raise AssertionError("the second wave waits at a barrier 1 the main wave never reaches")


def _kinds(nsub, pattern):
    if pattern == "inside":
        return [True] * nsub
    if pattern == "below":
        return [False] * nsub
    return [(k // 3) % 2 == 0 for k in range(nsub)]             # years that cross between the two


@pytest.mark.parametrize("pattern", ["inside", "below", "mixed"])
@pytest.mark.parametrize("nsub", [1, 2, 24 * 365, 48 * 366])
def test_both_waves_pass_the_same_barriers_on_every_exit(nsub, pattern):
    kinds = _kinds(nsub, pattern)
    stops = [None, 0, nsub - 1] + ([1, nsub // 2] if nsub > 2 else [])
    for stop_at, how in itertools.product(stops, (AFTER_B3, MID)):
        m = main_wave(kinds, stop_at, how)
        s, fronts, chains = second_wave([go for b, go in m if b == "b1"], kinds)
        assert [b for b, _ in m] == s, (stop_at, how)
        ran = nsub if stop_at is None else stop_at + 1
        assert fronts == ran and chains == sum(kinds[:ran]), (stop_at, how)
        assert m[-1] == ("b1", 1) and [go for b, go in m if b == "b1"].count(1) == 1
        assert len(m) == 3 * ran + 1                            # three barriers a substep, whatever its kind
