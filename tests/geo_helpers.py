"""Shared by tests/test_geo.py and tests/test_gpu_geo.py: the goldens of kind
`geo` (tests/golden/make_golden.py main_geo) -- the reference run at layer
interfaces other than the two sets the kernels hold at compile time, so every
run of them goes through the runtime-geometry (GeoR) instantiations."""
from __future__ import annotations

import json

import numpy as np

from tests.conftest import GOLDEN

GEO_GOLDENS = ("geo_a_ns36", "geo_b_ns12", "geo_c_ns24")
_cache = {}


def load_geo_golden(name):
    """(meta, inputs, expected) of a `geo` golden, in the shape
    conftest.load_golden returns; the synthetic inputs are regenerated
    (synth_inputs at L = 8, l10_inputs at L = 10) and checked against the
    stored sha256.  Loaded once per session: treat the arrays as read-only."""
    if name in _cache:
        return _cache[name]
    from tests.golden.make_golden import digest, l10_inputs, packed_params, synth_inputs
    z = np.load(GOLDEN / f"{name}.npz")
    meta = json.loads(str(z["meta"]))
    assert meta["kind"] == "geo", (name, meta["kind"])
    L = meta["L"]
    gid = np.asarray(meta["gid"], dtype=np.int64)
    if L == 10:
        p, f = l10_inputs(gid, meta["year0"], meta["nyears"], meta["seed"])
    else:
        p, f = synth_inputs(gid, meta["year0"], meta["nyears"], L, meta["seed"])
    assert digest(packed_params(p), f) == meta["input_sha256"], "synthetic inputs drifted"
    zi = np.asarray(meta["zi"], np.float32)
    assert zi.size == L + 2
    inputs = dict(zi=zi, params=p, forcing=f, nisurf=meta["nisurf"], year0=meta["year0"], nyears=meta["nyears"],
                  grow_on=meta["grow_on"], state0=None)
    for a in (zi, f, *p.values()):
        a.setflags(write=False)
    _cache[name] = (meta, inputs, dict(annual=z["annual"], state=z["state"]))
    return _cache[name]


def first_cells(inp, n, nyears=1):
    """The first n cells and the first nyears years of a golden's inputs."""
    from oracle import port
    nd = sum(port._days(inp["year0"] + k) for k in range(nyears))
    return dict(inp, nyears=nyears, params={k: np.ascontiguousarray(v[:n]) for k, v in inp["params"].items()},
                forcing=np.ascontiguousarray(inp["forcing"][:, :nd, :n]))
