"""The packed state through the device rows (hybrid9_amd/csrc/h9g_rows.h):
h9g_set_state then h9g_get_state returns the packed block bit for bit, and
h9g_init_kernel's rows read back as the oracle's init_state."""
import numpy as np
import pytest

import hybrid9_amd as h
from hybrid9_amd import synth
from oracle import port
from tests.test_rows import distinct, same_bits, special

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("L,nisurf", [(8, 48), (10, 24)])
def test_state_roundtrip_and_init_rows(L, nisurf):
    n = 3
    if L == 8:
        g, zi = synth.land_cells()[7::389][:n], synth.ZI_L8
    else:
        g, zi = synth.land_cells(synth.NX025, synth.NY025, synth.NLAND025)[11::1601][:n], synth.ZI_L10
    p = synth.make_params(g, L)
    packed = special(distinct((4 * L + 9) * n))
    with h.Context(n, zi, nlayers=L, nisurf=nisurf, grow_on=True) as ctx:
        ctx.set_params(p)
        ctx.set_state(packed)
        back = ctx.get_state()
        ctx.init_state()
        init = ctx.get_state()
    assert same_bits(back, packed)              # distinct values, NaN payloads, -0.0
    assert same_bits(init, port.init_state(p, zi))
