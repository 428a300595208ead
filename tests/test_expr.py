"""The layer expressions that every lane mapping of hydrology_pair shares
(hybrid9_amd/csrc/h9g_expr.h) on the host (tests/csrc/host_expr.cpp,
test-only): the fast forms equal the exact forms bit for bit wherever they
raise no flag, and they flag what lies outside their range.  The inputs are
chosen so that the exact forms alone give finite results on all of them."""
import ctypes as C
import subprocess

import numpy as np

from tests.helpers import BUILD, ROOT

FP = C.POINTER(C.c_float)
IP = C.POINTER(C.c_int)
_lib = None


def expr_lib():
    global _lib
    if _lib is None:
        src = ROOT / "tests" / "csrc" / "host_expr.cpp"
        out = BUILD / "libhost_expr.so"
        deps = [src] + list((ROOT / "hybrid9_amd" / "csrc").glob("*.h"))
        if not out.exists() or out.stat().st_mtime < max(d.stat().st_mtime for d in deps):
            BUILD.mkdir(exist_ok=True)
            subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-fPIC", "-shared",
                            str(src), "-o", str(out)], check=True)
        _lib = C.CDLL(str(out))
        _lib.h9k_expr_s1.argtypes = [C.c_int, FP, FP, FP, FP, FP, FP, IP, FP, FP]
        _lib.h9k_expr_vol_in.argtypes = [C.c_int, FP, FP, FP, FP, FP, FP, FP, IP, FP]
    return _lib


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def f32(x):
    return np.ascontiguousarray(x, np.float32)


def pow2(rng, lo, hi, n):
    """n float32 with a random significand and an exponent in [lo, hi)."""
    return f32(np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(lo, hi, n)))


LO, HI = np.float32(2.0 ** -60), np.float32(2.0 ** 60)       # s1_mk's range [2^-60, 2^60)
BELOW_LO, BELOW_HI = np.nextafter(LO, np.float32(0)), np.nextafter(HI, np.float32(0))


def s1(sa, sb):
    """The two forms of s1 for a = theta(i) + theta(ip) = sa, b = ts(i) +
    ts(ip) = sb (each as two equal halves: their sum is exact)."""
    sa, sb = f32(sa), f32(sb)
    n = sa.size
    h = np.float32(0.5)
    th, ts = f32(sa * h), f32(sb * h)
    out = [np.empty(n, np.float32) for _ in range(4)]
    flag = np.empty(n, np.int32)
    expr_lib().h9k_expr_s1(n, th.ctypes.data_as(FP), th.ctypes.data_as(FP), ts.ctypes.data_as(FP),
                           ts.ctypes.data_as(FP), out[0].ctypes.data_as(FP), out[1].ctypes.data_as(FP),
                           flag.ctypes.data_as(IP), out[2].ctypes.data_as(FP), out[3].ctypes.data_as(FP))
    fast, fast_min, exact, exact_min = out
    assert np.isfinite(exact).all() and np.isfinite(exact_min).all()
    assert np.isin(flag, (0, 3)).all()          # s1_quot_mk and s1_mk flag alike
    return fast, fast_min, flag != 0, exact, exact_min


def test_s1_mk_is_the_exact_quotient_in_its_range():
    rng = np.random.default_rng(5)
    n = 4000
    # the soil's range, the whole accepted range, and both edges either side
    sa = np.concatenate([f32(rng.uniform(0.02, 1.3, n)), pow2(rng, -60, 60, n)])
    sb = np.concatenate([f32(rng.uniform(0.5, 1.4, n)), pow2(rng, -60, 60, n)])
    edges = np.array([LO, BELOW_HI, np.nextafter(LO, np.float32(1)), np.float32(1.0), np.float32(0.75)], np.float32)
    ea, eb = np.meshgrid(edges, edges)
    sa, sb = np.concatenate([sa, ea.ravel()]), np.concatenate([sb, eb.ravel()])
    fast, fast_min, flagged, exact, exact_min = s1(sa, sb)
    assert not flagged.any()
    assert same_bits(fast, exact)
    assert same_bits(fast_min, exact_min)
    assert (exact > 1).any() and (exact < 1).any()            # the clamp is exercised both ways


def test_s1_mk_flags_outside_its_range():
    rng = np.random.default_rng(6)
    n = 1000
    mid = pow2(rng, -20, 20, n)
    out = np.concatenate([pow2(rng, -100, -61, n // 2), pow2(rng, 60, 100, n // 2)])
    edge_out = np.array([BELOW_LO, HI, np.float32(0.0), np.float32(-0.5)], np.float32)
    one = np.ones(edge_out.size, np.float32)
    # the dividend outside (zero and negative among it), then the divisor
    # outside (nonzero: the exact quotient stays finite)
    sa = np.concatenate([out, mid, edge_out, one, np.array([BELOW_LO, HI], np.float32)])
    sb = np.concatenate([mid, out, one, np.where(edge_out == 0, BELOW_LO, edge_out), np.array([HI, BELOW_LO], np.float32)])
    fast, fast_min, flagged, exact, exact_min = s1(sa, sb)
    assert flagged.all()
    # one operand at the last value inside, the other outside: still flagged
    _, _, fl, _, _ = s1(np.array([LO, BELOW_HI, BELOW_LO, HI], np.float32),
                        np.array([BELOW_LO, HI, LO, BELOW_HI], np.float32))
    assert fl.all()


def vol_in(pte, ts, temp0, zw, zlo, zhi):
    a = [f32(v) for v in (pte, ts, temp0, zw, zlo, zhi)]
    n = a[0].size
    fast, exact, flag = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, np.int32)
    expr_lib().h9k_expr_vol_in(n, *[v.ctypes.data_as(FP) for v in a], fast.ctypes.data_as(FP),
                               flag.ctypes.data_as(IP), exact.ctypes.data_as(FP))
    assert np.isfinite(exact).all()
    return fast, flag != 0, exact


def test_fast_in_layer_vol_eq_is_the_exact_form():
    rng = np.random.default_rng(7)
    n = 4000
    zlo = f32(rng.uniform(0.0, 3000.0, n))
    zhi = f32(zlo + rng.uniform(10.0, 1500.0, n))
    zw = f32(zlo + (zhi - zlo) * rng.uniform(0.0, 1.0, n))
    # the water table one float above the layer's top and one below its bottom
    zw[:50] = np.nextafter(zlo[:50], np.float32(np.inf))
    zw[50:100] = np.nextafter(zhi[50:100], np.float32(-np.inf))
    inside = (zw > zlo) & (zw < zhi)
    ts = f32(rng.uniform(0.3, 0.6, n))
    bsw = rng.uniform(2.5, 15.0, n)
    pte = f32(-rng.uniform(10.0, 1000.0, n) * ts / (1.0 - 1.0 / bsw))      # psi ts / (1 - 1/b), psi < 0
    temp0 = f32(rng.uniform(1.0, 8.0, n) ** (1.0 - 1.0 / bsw))            # ((-psi + zw - zlo) / -psi)^(1 - 1/b)
    a = [v[inside] for v in (pte, ts, temp0, zw, zlo, zhi)]
    assert a[0].size > 3900
    fast, flagged, exact = vol_in(*a)
    assert not flagged.any()
    assert same_bits(fast, exact)
    assert (exact == a[1]).any() and ((exact > 0) & (exact < a[1])).any()  # both sides of the clamp to ts


def test_fast_in_layer_vol_eq_flags_a_subnormal_quotient():
    """PTE / (zw - zlo) below the normal range: the double-reciprocal quotient
    may round differently there, so the lane is flagged for the exact form."""
    k = 8
    pte = np.full(k, -2.0 ** -120, np.float32)
    fast, flagged, exact = vol_in(pte, np.full(k, 0.4), np.full(k, 1.5), np.linspace(300.0, 900.0, k),
                                  np.full(k, 100.0), np.full(k, 1000.0))
    assert flagged.all()
