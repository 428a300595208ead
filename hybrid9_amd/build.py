"""Build the gfx950 HIP library ``hybrid9_amd/lib/libh9g.so`` in-tree.

``python -m hybrid9_amd.build`` (also called by ``__graft_entry__.build()``).
hipcc cross-compiles for gfx950 without a GPU.  Numerics flags are part of
the parity contract: ``-ffp-contract=off`` (the reference executes no FMA;
h9_math.h issues its FMAs explicitly) and HIP's default correctly-rounded
f32 division/sqrt and f32 denormal support are kept (no fast-math).
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
CSRC = HERE / "csrc"
# The translation units and the flags each gets beyond FLAGS.  ID: the build-id
# flag, for the unit that defines h9g_build_id alone (a digest of every unit:
# with it a unit is recompiled whenever any other changes).
ID = object()
UNITS = [
    (CSRC / "h9g.hip", []),         # host runtime: context, forcing, the year launch, recording; its small kernels
    (CSRC / "h9g_ord.hip", []),     # host runtime: the ordered mode and its small kernels
    (CSRC / "h9g_spin.hip", []),    # host runtime: spin-up to equilibrium and its kernel
    (CSRC / "h9g_stat.hip", []),    # host runtime: day statistics from the day records and their kernel
    (CSRC / "h9g_quant.hip", []),   # host runtime: day quantiles from the day records and their kernel
    (CSRC / "h9g_aux.hip", []),     # soil build, synthetic inputs, self-tests
    (CSRC / "h9g_plain.hip", []),   # the plain year kernels (h9g_year.h)
    (CSRC / "h9g_mon.hip", []),     # the monthly kernels: the same kernels with the Months policy
    (CSRC / "h9g_et.hip", []),      # the ET kernels: the same kernels with the EvapProf and MonthsEt policies
    (CSRC / "h9g_day.hip", []),     # the day-record kernels: the same kernels with the EvapProf and DaysEt policies
    (CSRC / "h9g_cols.hip", []),    # the other geometry-templated kernels: init, sort, site, focus
    (CSRC / "h9g_io.cpp", [ID]),    # host-only NetCDF I/O, and h9g_build_id
]
_INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', re.M)


def unit_deps(src: Path) -> list[Path]:
    """A unit and the headers it reaches through quoted #includes, transitively
    (whatever an #if around them says): what its object is compiled from."""
    seen, todo = [], [src]
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.append(f)
        todo += [(f.parent / m).resolve() for m in _INCLUDE.findall(f.read_text())]
    return [seen[0], *sorted(seen[1:])]


def deps() -> list[Path]:
    """Every file the library is compiled from: the units in UNITS' order, then their headers."""
    per = [unit_deps(src) for src, _ in UNITS]
    return [u[0] for u in per] + sorted({h for u in per for h in u[1:]})


OUT = HERE / "lib" / "libh9g.so"
ARCH = os.environ.get("H9G_ARCH", "gfx950")

FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-fPIC", "-shared",
         "-Wall", "-Wno-unused-value"]


def hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and Path(c).exists():
            return c
    raise FileNotFoundError("hipcc not found")


def build_id(extra=()) -> str:
    """Digest of everything the library is compiled from: the sources, the
    flags and the target.  It is compiled into the library (h9g_build_id)
    and recorded with every profile (tools/pmc_summary.py), so bench.py
    attaches counters only to the build they were measured on."""
    import hashlib
    hs = hashlib.sha256()
    for d in deps():
        hs.update(d.name.encode() + b"\0" + d.read_bytes() + b"\0")
    hs.update(" ".join([ARCH, *FLAGS, *extra]).encode())
    return hs.hexdigest()[:16]


def id_flag(extra=()) -> str:
    return f'-DH9G_BUILD_ID="{build_id(extra)}"'


def up_to_date() -> bool:
    if not OUT.exists():
        return False
    t = OUT.stat().st_mtime
    return all(d.stat().st_mtime <= t for d in deps())


def _run(cmd, verbose):
    if verbose:
        print(" ".join(cmd))
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed:\n{r.stderr[-4000:]}")


def build(force: bool = False, verbose: bool = False, extra=()) -> Path:
    """Compiles the translation units of UNITS to objects, side by side, each
    only when its own inputs changed (keyed by the digest of its flags, its
    source and the headers it includes), and links libh9g.so.  The four units
    of year kernels take minutes each and h9g_cols.hip about one; the host
    runtime's units and the I/O take seconds, so a change there is a short build."""
    if not force and up_to_date():
        return OUT
    OUT.parent.mkdir(parents=True, exist_ok=True)
    obj = OUT.parent / "obj"
    obj.mkdir(exist_ok=True)
    import hashlib
    flags = [f"--offload-arch={ARCH}", *FLAGS, *extra]
    objs, jobs = [], []
    for src, own in UNITS:
        flags_u = flags + [id_flag(extra) if f is ID else f for f in own]
        hs = hashlib.sha256(" ".join(flags_u).encode())
        for d in unit_deps(src):
            hs.update(d.read_bytes())
        o = obj / f"{src.stem}_{hs.hexdigest()[:16]}.o"
        if force or not o.exists():
            # this unit's stale objects (the digest is what follows the stem: "h9g_*" would be every unit's)
            for old in obj.glob(f"{src.stem}_{'[0-9a-f]' * 16}.o"):
                old.unlink()
            tmp = o.with_suffix(".o.tmp")
            jobs.append(([hipcc(), *[f for f in flags_u if f != "-shared"], "-c", str(src), "-o", str(tmp)], tmp, o))
        objs.append(str(o))
    if jobs:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(min(len(jobs), 16)) as ex:
            for _ in ex.map(lambda j: (_run(j[0], verbose), os.replace(j[1], j[2])), jobs):
                pass
    tmp = OUT.with_suffix(".so.tmp")
    _run([hipcc(), f"--offload-arch={ARCH}", "-fPIC", "-shared", *objs, "-o", str(tmp)], verbose)
    os.replace(tmp, OUT)
    return OUT


if __name__ == "__main__":
    p = build(force="--force" in sys.argv, verbose=True)
    print(p)
