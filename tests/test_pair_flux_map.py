"""The map of the pair kernels' split flux phase (hydrology_pair, h9g_pair.h:
`kFluxSplit`, H9G_FLUX_SPLIT), restated and checked on the host for L = 8
and 10.

After the equilibrium and conductivity phases lane h (0 even, 1 odd) of a pair
holds, in slot t = 0..L/2-1, hk, dhkdw, smp, dsmpdw and zq of its own layer
2t+1+h.  The tridiagonal system's interface i lies between layers i and i+1
(i = L: the aquifer interface, between layer L and the aquifer node).  The
split phase evaluates every interface once per pair:

  lane h, slot t         interface i = 2t+1+h
    own-layer operands   the lane's own slot t (layer i)
    next-layer operands  layer i+1 = the partner's slot t (h = 0) or t+1 (h = 1):
      smp, zq            from the exchanged arrays at index i+1, selected on h
      dsmpdw             by one pair_swap: a lane sends its slot t+1 (h = 0) or
                         t (h = 1) and takes what its partner sends
    odd lane, last slot  the aquifer interface L: smp1, dsmpdw1 and zq(L+1),
                         which both lanes hold

and exchanges qo, d1, d2 of every interface to both lanes."""
from __future__ import annotations

import pytest

LS = (8, 10)
AQ = "aquifer"                                           # the aquifer node's smp1, dsmpdw1, zq(L+1)


def own_layer(L, h, t):
    """The layer whose results lane h holds in slot t."""
    assert 0 <= t < L // 2 and h in (0, 1)
    return 2 * t + 1 + h


def flux_slot(L, i):
    """(lane parity, slot) that evaluates interface i."""
    assert 1 <= i <= L
    return (i - 1) % 2, (i - 1) // 2


def array_index_next(L, h, t):
    """Index into the exchanged arrays smp[], zq[] of the next-layer operand,
    as the device selects it: sel(h, a[2t+2], a[2t+3]); the last slot's odd
    lane takes smp1 (zq[L+1] is the aquifer node's entry of zq[] itself)."""
    return 2 * t + 2 + h


def swap_sent(L, h, t):
    """The slot whose dsmpdw lane h sends in the exchange of slot t: the even
    lane its slot t+1, the odd lane its slot t; the even lane's last send is
    its last slot again, unread (the odd lane selects dsmpdw1 there)."""
    NT = L // 2
    if t == NT - 1:
        return NT - 1
    return t + 1 if h == 0 else t


def next_sources(L, h, t):
    """Where lane h's slot-t interface takes smp, dsmpdw and zq of the layer
    above the interface from: (partner parity, partner slot), or AQ."""
    NT = L // 2
    if h == 1 and t == NT - 1:
        return {"smp": AQ, "dsmpdw": AQ, "zq": AQ}
    layer = array_index_next(L, h, t)
    holder = flux_slot(L, layer)                          # layer k is held where interface k is evaluated
    return {"smp": holder, "zq": holder, "dsmpdw": (1 - h, swap_sent(L, 1 - h, t))}


@pytest.mark.parametrize("L", LS)
def test_every_interface_is_evaluated_exactly_once_per_pair(L):
    done = [own_layer(L, h, t) for h in (0, 1) for t in range(L // 2)]
    assert sorted(done) == list(range(1, L + 1))
    assert [i for i in done if i % 2 == 1] == list(range(1, L, 2))      # even lane: 1, 3, .., L-1
    assert [i for i in done if i % 2 == 0] == list(range(2, L + 1, 2))  # odd lane: 2, 4, .., L-2, then L


@pytest.mark.parametrize("L", LS)
def test_interface_2t_1_h_is_on_lane_h_slot_t(L):
    for h in (0, 1):
        for t in range(L // 2):
            assert flux_slot(L, 2 * t + 1 + h) == (h, t)
            assert own_layer(L, *flux_slot(L, 2 * t + 1 + h)) == 2 * t + 1 + h
    assert flux_slot(L, L) == (1, L // 2 - 1)             # the aquifer interface: odd lane, last slot
    assert flux_slot(L, L - 1) == (0, L // 2 - 1)


@pytest.mark.parametrize("L", LS)
def test_next_layer_operands_come_from_the_slot_that_holds_them(L):
    NT = L // 2
    for i in range(1, L):
        h, t = flux_slot(L, i)
        src = next_sources(L, h, t)
        for what in ("smp", "dsmpdw", "zq"):
            ph, pt = src[what]
            assert ph == 1 - h                            # the partner's
            assert pt == (t if h == 0 else t + 1)         # slot t for the even lane, t+1 for the odd one
            assert 0 <= pt < NT
            assert own_layer(L, ph, pt) == i + 1          # ... which holds layer i+1
        assert array_index_next(L, h, t) == i + 1 <= L


@pytest.mark.parametrize("L", LS)
def test_the_swap_pairs_what_one_lane_sends_with_what_the_other_needs(L):
    NT = L // 2
    for t in range(NT):
        even_gets = own_layer(L, 1, swap_sent(L, 1, t))   # the odd lane's send
        assert even_gets == own_layer(L, 0, t) + 1
        if t < NT - 1:
            odd_gets = own_layer(L, 0, swap_sent(L, 0, t))
            assert odd_gets == own_layer(L, 1, t) + 1
        assert 0 <= swap_sent(L, 0, t) < NT and 0 <= swap_sent(L, 1, t) < NT


@pytest.mark.parametrize("L", LS)
def test_the_aquifer_interface_takes_the_aquifer_node(L):
    h, t = flux_slot(L, L)
    assert next_sources(L, h, t) == {"smp": AQ, "dsmpdw": AQ, "zq": AQ}
    assert array_index_next(L, h, t) == L + 1             # zq(L+1): the aquifer node's entry
    for i in range(1, L):                                 # and no other interface does
        assert AQ not in next_sources(L, *flux_slot(L, i)).values()
