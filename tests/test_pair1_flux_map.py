"""The map of the one-column wave's round C (hydrology_pair, h9g_pair.h:
`kTask`, after rounds A and B), restated and checked on the host for L = 8
and 10.

Round C evaluates the tridiagonal system's interface fluxes qo(i), d1(i),
d2(i) once, a lane per interface, instead of on both pair lanes:

  interface i = 1..L-1   on lane 4(i-1)+2, layer i's kind-2 lane, which holds
                         hk(i), dhkdw(i); it takes
                           smp(i),   dsmpdw(i)    from lane ln+1 (kind 3 of i)
                           smp(i+1), dsmpdw(i+1)  from lane ln+5 (kind 3 of i+1)
                           zq(i)                  from lane ln-1 (kind 1 of i)
                           zq(i+1)                from lane ln+3 (kind 1 of i+1)
  aquifer interface L    on lane 4(L-1)+2 (read only below the column):
                           smp(L), dsmpdw(L), zq(L) as above,
                           smp1, dsmpdw1          from lane 4L+1 (round B, aquifer1)
                           zq(L+1)                from lane 4L   (round B, aquifer0)

The pair lanes then read qo, d1, d2 of every interface from its lane and smp
of every layer from its kind-3 lane; hk, dhkdw, dsmpdw and zq(1..L) travel
only when a flag sends the wave-substep to the pair lanes' own flux block."""
from __future__ import annotations

import pytest

from tests.test_pair1_tasks import decode, round_a, round_b

LS = (8, 10)
OPERANDS = ("hk", "dhkdw", "smp_i", "dsmpdw_i", "smp_n", "dsmpdw_n", "zq_i", "zq_n")


def flux_lane(L, i):
    """The lane that evaluates interface i (i = L: the aquifer interface)."""
    return 4 * (i - 1) + 2


def flux_sources(L, ln):
    """lane ln's operand lanes in round C, as the device forms them (every
    lane forms them; only the interface lanes' results are read)."""
    _, i = decode(L, ln)
    top = i == L
    return {
        "hk": ln, "dhkdw": ln,
        "smp_i": (ln + 1) & 63, "dsmpdw_i": (ln + 1) & 63,
        "smp_n": (4 * L + 1 if top else ln + 5) & 63, "dsmpdw_n": (4 * L + 1 if top else ln + 5) & 63,
        "zq_i": (ln + 63) & 63, "zq_n": (4 * L if top else ln + 3) & 63,
    }


def holds(L, ln, what, layer):
    """Does lane ln hold `what` of `layer` after rounds A and B?"""
    la, lb = round_a(L), round_b(L)
    if what in ("hk", "dhkdw"):
        return la[ln] == ("A", layer, "s1")
    if what in ("smp", "dsmpdw"):
        return la[ln] == ("A", layer, "s_node")
    if what == "zq":
        return lb[ln] == ("B", layer, "zq")
    if what in ("smp1", "dsmpdw1"):
        return ln == 4 * L + 1 and lb[ln] == ("B", L, "aquifer1")
    if what == "zq_aq":
        return ln == 4 * L and lb[ln] == ("B", L, "aquifer0")
    raise KeyError(what)


def gather_list(L):
    """(value, index, lane) of everything the pair lanes read after round C
    on the fast path; the aquifer interface's fluxes only below the column."""
    out = []
    for i in range(1, L + 1):
        out.append(("smp", i, 4 * (i - 1) + 3))
        for v in ("qo", "d1", "d2"):
            out.append((v, i, flux_lane(L, i)))
    return out


@pytest.mark.parametrize("L", LS)
def test_every_interface_has_one_lane(L):
    lanes = [flux_lane(L, i) for i in range(1, L + 1)]
    assert len(set(lanes)) == L
    for i, ln in enumerate(lanes, start=1):
        assert decode(L, ln) == (2, i)                   # the layer's kind-2 lane
        # no other lane decodes to (kind 2, layer i)
        assert [x for x in range(64) if decode(L, x) == (2, i)] == [ln]


@pytest.mark.parametrize("L", LS)
def test_operands_come_from_the_lanes_that_hold_them(L):
    for i in range(1, L):
        src = flux_sources(L, flux_lane(L, i))
        assert holds(L, src["hk"], "hk", i) and holds(L, src["dhkdw"], "dhkdw", i)
        assert holds(L, src["smp_i"], "smp", i) and holds(L, src["dsmpdw_i"], "dsmpdw", i)
        assert holds(L, src["smp_n"], "smp", i + 1) and holds(L, src["dsmpdw_n"], "dsmpdw", i + 1)
        assert holds(L, src["zq_i"], "zq", i) and holds(L, src["zq_n"], "zq", i + 1)
    src = flux_sources(L, flux_lane(L, L))               # the aquifer interface
    assert holds(L, src["hk"], "hk", L) and holds(L, src["dhkdw"], "dhkdw", L)
    assert holds(L, src["smp_i"], "smp", L) and holds(L, src["dsmpdw_i"], "dsmpdw", L)
    assert holds(L, src["zq_i"], "zq", L)
    assert holds(L, src["smp_n"], "smp1", L) and holds(L, src["dsmpdw_n"], "dsmpdw1", L)
    assert holds(L, src["zq_n"], "zq_aq", L)
    assert (src["smp_n"], src["zq_n"]) == (4 * L + 1, 4 * L)


@pytest.mark.parametrize("L", LS)
def test_no_lane_index_reaches_64(L):
    for ln in range(64):                                 # every lane forms its sources, read or not
        src = flux_sources(L, ln)
        assert set(src) == set(OPERANDS)
        assert all(0 <= s < 64 for s in src.values())
    for i in range(1, L + 1):                            # the interface lanes' need no wrap
        ln = flux_lane(L, i)
        assert 1 <= ln and ln + 5 < 64 and 4 * L + 1 < 64
    assert all(0 <= ln < 64 for _, _, ln in gather_list(L))
    for jwt in range(0, L):                              # the recharge section's smp, zq of layer max(jwt, 1)
        lm = 4 * (max(jwt, 1) - 1)
        assert holds(L, lm + 3, "smp", max(jwt, 1)) and holds(L, lm + 1, "zq", max(jwt, 1))


@pytest.mark.parametrize("L", LS)
def test_the_gather_covers_every_flux_and_every_smp_once(L):
    g = gather_list(L)
    keys = [(v, i) for v, i, _ in g]
    assert len(set(keys)) == len(keys) == 4 * L
    want = [(v, i) for i in range(1, L + 1) for v in ("qo", "d1", "d2", "smp")]
    assert sorted(keys) == sorted(want)
    for v, i, ln in g:
        if v == "smp":
            assert holds(L, ln, "smp", i)
        else:
            assert ln == flux_lane(L, i)
    assert 4 * L < 5 * L + 5                             # against the five per-layer arrays and the aquifer node
