"""The task map of the one-column wave's two task rounds (hydrology_pair,
h9g_pair.h: `kTask`), restated and checked on the host for L = 8 and 10.

A wave of h9g_pair1_kernel holds one column: pair lanes 0 and 1, 62 helper
lanes.  Its powers of the equilibrium profile, the conductivity phase, the
single-power round and the aquifer node run as two rounds, a power per lane:

  round A (level 0: reads only the substep's starting state)
    lane 4(i-1)+k   layer i = 1..L, kind k = 0 b0^expo, 1 bi^expo,
                    2 s1^(2b+2), 3 s_node^(-b)
    lane 4L, 4L+1   the two single powers (kinds 4, 5)
  round B (level 1: reads round A's results), on the lane that holds the operand
    lane 4(i-1)+1   (vol_eq(i)/ts(i))^(-b(i)): vol_eq from the lane's own
                    bi^expo and lane 4(i-1)'s b0^expo (DPP quad_perm [0,0,2,2])
    lane 4L, 4L+1   the aquifer node's two powers

Lanes past 4L+1 repeat the last task; the lanes of kinds 0, 2 and 3 repeat
kind 1's expressions in round B and are never read.  Both pair lanes read
every layer's results from the lanes that hold them (zq from kind 1, hk and
dhkdw from kind 2, smp and dsmpdw from kind 3); the tasks' flags come by
ballot, masked by kind.

tests/test_helper_lanes.py's (L, 1) rows describe the former map of this wave
shape (one helper round per phase), which the one-column kernel still
compiles when the task rounds are switched off (H9G_P1_TASKS=0) and which
the 11- and 22-column kernels keep."""
from __future__ import annotations

import pytest

LS = (8, 10)
KINDS_A = ("b0", "bi", "s1", "s_node")


def decode(L, ln):
    """(kind, layer) of lane ln, as the device decodes it; the layer of kinds
    4 and 5 is a runtime value (jwt + 1, or L below the column): None."""
    NA = 4 * L + 2
    ta = min(ln, NA - 1)
    if ta < 4 * L:
        return ta & 3, (ta >> 2) + 1
    return ta - 4 * L + 4, None


def round_a(L):
    out = {}
    for ln in range(64):
        k, i = decode(L, ln)
        out[ln] = ("A", i, KINDS_A[k] if k < 4 else "single%d" % (k - 4))
    return out


def round_b(L):
    """lane -> the task whose result is read from it (None: unread)."""
    out = {}
    for ln in range(64):
        k, i = decode(L, ln)
        if ln >= 4 * L + 2:
            out[ln] = None                               # a repeat of the last task
        elif k == 1:
            out[ln] = ("B", i, "zq")
        elif k >= 4:
            out[ln] = ("B", L, "aquifer%d" % (k - 4))
        else:
            out[ln] = None
    return out


def all_tasks(L):
    a = [("A", i, k) for i in range(1, L + 1) for k in KINDS_A] + [("A", None, "single0"), ("A", None, "single1")]
    b = [("B", i, "zq") for i in range(1, L + 1)] + [("B", L, "aquifer0"), ("B", L, "aquifer1")]
    return a, b


@pytest.mark.parametrize("L", LS)
def test_a_lane_per_task(L):
    assert 4 * L + 2 <= 64 and L + 2 <= 64
    a, b = all_tasks(L)
    assert len(a) == 4 * L + 2 and len(b) == L + 2


@pytest.mark.parametrize("L", LS)
def test_every_task_is_evaluated_once(L):
    ta, tb = all_tasks(L)
    la, lb = round_a(L), round_b(L)
    live_a = [la[ln] for ln in range(4 * L + 2)]
    assert sorted(live_a, key=str) == sorted(ta, key=str) and len(set(live_a)) == len(live_a)
    live_b = [v for v in lb.values() if v is not None]
    assert sorted(live_b, key=str) == sorted(tb, key=str) and len(set(live_b)) == len(live_b)


@pytest.mark.parametrize("L", LS)
def test_idle_lanes_repeat_a_valid_task(L):
    """Every lane decodes to a kind 0..5 and a layer 1..L (or the runtime
    layer of the single powers), so no lane forms an address outside the
    column's block; lanes past the last task repeat it."""
    ta, _ = all_tasks(L)
    la = round_a(L)
    for ln in range(64):
        k, i = decode(L, ln)
        assert 0 <= k <= 5 and (i is None or 1 <= i <= L)
        assert la[ln] in ta
    for ln in range(4 * L + 2, 64):
        assert decode(L, ln) == decode(L, 4 * L + 1)


@pytest.mark.parametrize("L", LS)
def test_round_b_runs_where_its_operands_are(L):
    """vol_eq(i) needs b0^expo and bi^expo of layer i: the kind-1 lane holds
    the second and takes the first from the even lane of its lane pair."""
    la, lb = round_a(L), round_b(L)
    for i in range(1, L + 1):
        ln = 4 * (i - 1) + 1
        assert lb[ln] == ("B", i, "zq")
        assert la[ln] == ("A", i, "bi")
        assert la[ln & ~1] == ("A", i, "b0")             # quad_perm [0,0,2,2]: lane & ~1
    # the aquifer node: zq(L+1) from the first single power (its temp0), smp1 from theta(L)
    assert la[4 * L] == ("A", None, "single0") and lb[4 * L] == ("B", L, "aquifer0")
    assert la[4 * L + 1] == ("A", None, "single1") and lb[4 * L + 1] == ("B", L, "aquifer1")


@pytest.mark.parametrize("L", LS)
def test_pair_lanes_read_the_lanes_that_ran_their_tasks(L):
    la, lb = round_a(L), round_b(L)
    for i in range(1, L + 1):
        base = 4 * (i - 1)
        assert lb[base + 1] == ("B", i, "zq")             # zq(i)
        assert la[base + 2] == ("A", i, "s1")             # hk(i), dhkdw(i)
        assert la[base + 3] == ("A", i, "s_node")         # smp(i), dsmpdw(i)
        assert base + 3 < 64
    assert 4 * L + 1 < 64


@pytest.mark.parametrize("L", LS)
def test_flag_masks_select_the_kinds(L):
    """The ballot bits that re-run eq_exact (kinds 0, 1 of round A, kind 1 of
    round B), hk_exact (kinds 2, 3) and the pick rounds (lanes 4L, 4L+1)."""
    la, lb = round_a(L), round_b(L)
    all_a = (1 << (4 * L)) - 1
    eq_a, eq_b, hk_a = 0x3333333333333333 & all_a, 0x2222222222222222 & all_a, 0xCCCCCCCCCCCCCCCC & all_a
    for ln in range(64):
        _, i, kind = la[ln]
        assert bool((eq_a >> ln) & 1) == (ln < 4 * L and kind in ("b0", "bi"))
        assert bool((hk_a >> ln) & 1) == (ln < 4 * L and kind in ("s1", "s_node"))
        assert bool((eq_b >> ln) & 1) == (lb[ln] is not None and lb[ln][2] == "zq")
        picks = bool(((3 << (4 * L)) >> ln) & 1)
        assert picks == (ln in (4 * L, 4 * L + 1))
        assert picks == (lb[ln] is not None and lb[ln][2].startswith("aquifer"))
    assert eq_a | hk_a == all_a and eq_a & hk_a == 0
