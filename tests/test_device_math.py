"""The scalar functions that the kernels and the CPU oracle share, held to each other bit for bit.

Every image-level parity test rests on one assumption: include/ct_fmath.h and the device-only variants of
csrc/ct_device.hpp give the same bits under hipcc for gfx950 as under gcc on the host.  This file checks that directly,
function by function: ct_debug_math_eval evaluates one function `fn` of the device code on given operands, orc_math_eval
(oracle/ct_oracle.c) is its host twin with the same numbering.

Input sets (built once per function, deterministic, at most 2^22 items) = a strided sweep of the domain by bit pattern
+ every float within 4096 ulp of each breakpoint of the function + the special values.

CPU half (no GPU): the oracle on these sets against float64 numpy (within the bounds ct_fmath.h states) or against exact
numpy restatements; the same translation unit compiled by ROCm's clang for the host against the gcc build, bit for bit.
GPU half (marked gpu): device == oracle bit for bit on every set, the four exhaustive self-tests of the device-only variants,
the new entry point's refusals, and one rendered frame at an optical depth per step just under the limit of 80.
"""
import ctypes as C
import subprocess
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import _oracle as O
import deepestscatter_amd as ds
from deepestscatter_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
CLANG = Path("/opt/rocm/llvm/bin/clang")

FN = {0: "ct_expf", 1: "ct_logf", 2: "ct_log2f", 3: "ct_powf", 4: "ct_sincosf", 5: "expf_inrange", 6: "logf_above_one", 7: "div_",
      8: "u24_to_float", 9: "tea4", 10: "lcg24", 11: "floor_to_int", 12: "fract_", 13: "tex_weight<false>", 14: "tex_weight<true>"}
INT_RESULT = {9: (True, True), 10: (True, True), 11: (True, True)}   # both result words are integers (strict comparison)
WIN = 4096           # ulps on either side of a breakpoint
CAP = 1 << 22        # items per set
TARGET = 1 << 21     # items of a strided sweep, about
FRAC_MAX = np.float32(1.0 - 2.0 ** -24)     # 0x1.fffffep-1f

NANS = [0x7fc00000, 0x7fc01234, 0xffc00001, 0x7f800001]
FINITE_SPECIALS = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff]   # +-0, smallest / largest subnormal
SPECIALS = FINITE_SPECIALS + [0x7f800000, 0xff800000] + NANS


# ---- bit patterns ---------------------------------------------------------------------------------------------------
def f2b(x):
    return np.ascontiguousarray(x, np.float32).reshape(-1).view(np.uint32)


def b2f(u):
    return np.ascontiguousarray(u, np.uint32).reshape(-1).view(np.float32)


def _key(bits):
    """Monotone integer key of a float's bit pattern (-0 and +0 share key 0)."""
    b = np.asarray(bits, np.uint32).astype(np.int64)
    return np.where(b < 2**31, b, 2**31 - b)


def _unkey(k):
    k = np.clip(np.asarray(k, np.int64), -0x7f800000, 0x7f800000)      # stay within [-inf, inf]
    return np.where(k >= 0, k, 2**31 - k).astype(np.uint32)


def window(centres, n=WIN):
    """Every float within n ulp on either side of each centre."""
    c = _key(f2b(np.asarray(centres, np.float64).astype(np.float32)))
    return _unkey((c[:, None] + np.arange(-n, n + 1, dtype=np.int64)[None, :]).reshape(-1))


def span(lo, hi):
    """Every float of [lo, hi]."""
    a, b = (int(_key(f2b(np.float32(v)))[0]) for v in (lo, hi))
    return _unkey(np.arange(a, b + 1, dtype=np.int64))


def sweep(ranges, target=TARGET):
    """Strided sweep by bit pattern over inclusive ranges of bit patterns, one odd stride for about `target` items."""
    total = sum(hi - lo + 1 for lo, hi in ranges)
    stride = max(1, total // target) | 1
    return np.concatenate([np.arange(lo, hi + 1, stride, dtype=np.int64) for lo, hi in ranges]).astype(np.uint32)


def bits_of(x):
    return int(f2b(np.float32(x))[0])


def union(*parts):
    out = np.unique(np.concatenate([np.asarray(p, np.uint32).reshape(-1) for p in parts]))
    assert 0 < out.size <= CAP, out.size
    return out


def union_pairs(*parts):
    a = np.concatenate([np.asarray(p[0], np.uint32).reshape(-1) for p in parts])
    b = np.concatenate([np.asarray(p[1], np.uint32).reshape(-1) for p in parts])
    ab = np.unique(np.stack([a, b], axis=1), axis=0)
    assert 0 < len(ab) <= CAP, len(ab)
    return np.ascontiguousarray(ab[:, 0]), np.ascontiguousarray(ab[:, 1])


# ---- the input sets -------------------------------------------------------------------------------------------------
LOG2E = float(np.float32(1.44269504088896341))
SQRT_HALF = 0.70710678


@lru_cache(maxsize=None)
def exp_set():
    # [-90, 90]; the sweep is a little thinner than elsewhere: the 254 rintf breakpoints alone are 2^21 items
    sw = sweep([(0, bits_of(90.0)), (0x80000000, bits_of(-90.0))], target=15 << 17)
    ties = [(n + 0.5) / LOG2E for n in range(-126, 128)]          # x * log2e crosses a half-integer: rintf steps
    return union(sw, window([-87.0, 88.0]), window(ties), span(-87.0, -86.6), SPECIALS)


@lru_cache(maxsize=None)
def log_set():
    sw = sweep([(1, 0x7f7fffff)])                                  # every positive float, subnormals included
    split = [SQRT_HALF * 2.0 ** e for e in (-126, -64, -1, 0, 1, 64, 127)]
    negatives = f2b(np.array([-1.0, -0.5, -3e38, -1e-30], np.float32))
    return union(sw, window(split), window([1.0]), window([2.0 ** -126]), window([0.0]), [0x7f7fffff], negatives, SPECIALS)


@lru_cache(maxsize=None)
def sincos_set():
    sw = sweep([(0, bits_of(8.0)), (0x80000000, bits_of(-8.0))])
    octants = [s * k * np.pi / 4 for k in range(1, 11) for s in (1, -1)]   # 10 pi/4 = 7.85 is the last one below 8
    return union(sw, window(octants), window([0.0, 8.0, -8.0]), SPECIALS)


@lru_cache(maxsize=None)
def pow_set():
    g = bits_of(1 / 2.2)
    bases = union(sweep([(1, 0x3f800000)]), window([1.0, 1e-4]), f2b(np.array([-1.0, -1e-30, 2.0, 1e30], np.float32)), SPECIALS)
    tonemap = (bases, np.full(bases.size, g, np.uint32))
    lods = f2b((np.arange(-2 * 64, 12 * 64 + 1) / 64.0).astype(np.float32))     # 2^lod of the descriptor
    two = (np.full(lods.size, bits_of(2.0), np.uint32), lods)
    ys = np.array(SPECIALS + [bits_of(1.0), bits_of(-1.0), bits_of(200.0)], np.uint32)
    some = np.array([bits_of(0.5), bits_of(2.0), 0, bits_of(1.0), bits_of(-2.0)], np.uint32)
    cross = (np.repeat(some, ys.size), np.tile(ys, some.size))
    return union_pairs(tonemap, two, cross)


@lru_cache(maxsize=None)
def div_set():
    rng = np.random.default_rng(20240607)
    n = 1 << 19
    anything = (rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32), rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32))
    # the march's back-off xi / T: xi a 24-bit random over 2^24, T in [1e-45, 1] -- subnormal T included
    xi = f2b((rng.integers(0, 1 << 24, n).astype(np.float64) / 2.0 ** 24).astype(np.float32))
    t_any = rng.integers(1, 0x3f800000 + 1, n).astype(np.uint32)
    t_sub = rng.integers(1, 0x00800000, n // 4).astype(np.uint32)
    thick = (np.concatenate([xi, xi[:n // 4]]), np.concatenate([t_any, t_sub]))
    # quotients around the overflow threshold: x = FLT_MAX * y * (1 +- a few ulp)
    y = b2f(rng.integers(bits_of(2.0 ** -100), 0x3f800000, n // 4).astype(np.uint32)).astype(np.float64)
    fmax = float(np.finfo(np.float32).max)
    x = (fmax * y * (1.0 + rng.integers(-16, 17, y.size) * 2.0 ** -24)).astype(np.float32)
    big = (f2b(x), f2b(y.astype(np.float32)))
    sp = np.array(SPECIALS + [bits_of(1.0), bits_of(-3.0), 0x7f7fffff], np.uint32)
    cross = (np.repeat(sp, sp.size), np.tile(sp, sp.size))
    return union_pairs(anything, thick, big, cross)


@lru_cache(maxsize=None)
def u24_set():
    return union(np.arange(0, 1 << 24, 7, dtype=np.uint32), [0, (1 << 24) - 1, (1 << 24) - 2, 1, 1 << 23])


@lru_cache(maxsize=None)
def tea_set():
    rng = np.random.default_rng(7)
    n = 1 << 20
    px, py = np.meshgrid(np.arange(0, 4096, 37, dtype=np.uint32), np.arange(0, 4096, 41, dtype=np.uint32))
    seeds = (px * np.uint32(4096) + py).reshape(-1)                   # the estimators' v0 = x * 4096 + y, v1 = subframe
    edge = np.array([0, 1, 0xffffffff, 0x80000000], np.uint32)
    return union_pairs((rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32), rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)),
                       (seeds, (np.arange(seeds.size) % 1025).astype(np.uint32)), (np.repeat(edge, 4), np.tile(edge, 4)))


@lru_cache(maxsize=None)
def lcg_set():
    rng = np.random.default_rng(8)
    return union(rng.integers(0, 2**32, 1 << 20, dtype=np.uint64).astype(np.uint32), [0, 1, 0xffffffff, 0x80000000, 0x00ffffff, 0x01000000])


@lru_cache(maxsize=None)
def texel_set():
    """Texel coordinates: the domain of floor_to_int, fract_ and the two filter weights (finite values only)."""
    lim = bits_of(2.0 ** 24)
    sw = sweep([(0, lim), (0x80000000, 0x80000000 | lim)])
    k = np.arange(0, 513, dtype=np.float32)
    around = np.concatenate([np.nextafter(k, np.float32(np.inf)), np.nextafter(k, np.float32(-np.inf)), k, -k, k - np.float32(0.5)])
    # the ties of the 1.8 fixed-point weight, (2k+1)/512, on several integers (all exact), each with its two neighbours
    tie = (2.0 * np.arange(256) + 1.0) / 512.0
    ties = np.concatenate([(base + tie).astype(np.float32) for base in (0.0, 1.0, 7.0, 100.0, 4095.0, -1.0, -3.0, -256.0)])
    ties = np.concatenate([ties, np.nextafter(ties, np.float32(np.inf)), np.nextafter(ties, np.float32(-np.inf))])
    # fractions above 255.5/256, which round to a weight of exactly 1.0; the fraction of a tiny negative x is clamped below 1
    top = window([255.5 / 256, 1.0, 3.0 + 255.5 / 256, 4.0, -2.0 + 255.5 / 256, -1.0, -1e-10, 0.0])
    return union(sw, f2b(around), f2b(ties), top, FINITE_SPECIALS)


@lru_cache(maxsize=None)
def inputs(fn):
    """(a, b): the operand bit patterns of function fn; b is None for a function of one operand."""
    if fn == 0:
        return exp_set(), None
    if fn == 5:      # the range ct_expf's checks leave: -87 < x <= 88 (callers pass (-87, 0])
        x = b2f(exp_set())
        return exp_set()[(x > -87.0) & (x <= 88.0)], None
    if fn in (1, 2):
        return log_set(), None
    if fn == 6:      # positive normal floats (callers pass xi / T > 1 and 1 - u >= 2^-24)
        s = log_set()
        return s[(s >= 0x00800000) & (s <= 0x7f7fffff)], None
    if fn == 3:
        return pow_set()
    if fn == 4:
        return sincos_set(), None
    if fn == 7:
        return div_set()
    if fn == 8:
        return u24_set(), None
    if fn == 9:
        return tea_set()
    if fn == 10:
        return lcg_set(), None
    if fn == 11:     # (int32_t)floorf(x) is defined for -2^31 <= x < 2^31 only: the range's ends stand in for inf and NaN
        return union(texel_set(), f2b(np.array([-2.0 ** 31, 2.0 ** 30, -2.0 ** 30], np.float32)), [0x4effffff, 0xceffffff]), None
    # 12, 13, 14: finite texel coordinates.  At +-inf and NaN the two sides differ and no caller can get there (a texel
    # coordinate is a finite position times a finite scale): test_fract_outside_the_finite_floats_is_as_documented
    return texel_set(), None


@lru_cache(maxsize=None)
def host(fn):
    """The oracle's results on inputs(fn), computed once."""
    a, b = inputs(fn)
    return O.math_eval(fn, a, b)


def is_nan_bits(u):
    return (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)


def assert_same_bits(fn, got, ref, who):
    """got == ref word for word; two NaNs of a float result count as equal -- except where the function hands its NaN
    argument back (ct_expf): there the payload must be the same too."""
    a, b = inputs(fn)
    for k in (0, 1):
        g, r = got[k], ref[k]
        bad = g != r
        if not INT_RESULT.get(fn, (False, False))[k] and fn != 0:
            bad &= ~(is_nan_bits(g) & is_nan_bits(r))
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            ops = f"a = 0x{int(a[i]):08x}" + (f", b = 0x{int(b[i]):08x}" if b is not None else "")
            raise AssertionError(f"fn {fn} ({FN[fn]}), result {k}: {int(bad.sum())} of {a.size} differ; first at {ops}: "
                                 f"{who[0]} 0x{int(g[i]):08x}, {who[1]} 0x{int(r[i]):08x}")


# =====================================================================================================================
# CPU half
# =====================================================================================================================
def test_sets_are_deterministic_and_bounded():
    for fn in FN:
        a, b = inputs(fn)
        assert a.dtype == np.uint32 and 0 < a.size <= CAP and (b is None or b.shape == a.shape), fn
    assert np.array_equal(exp_set.__wrapped__(), exp_set())
    for x, y in zip(div_set.__wrapped__(), div_set()):
        assert np.array_equal(x, y)


def _ulps(got_bits, ref64):
    got = b2f(got_bits).astype(np.float64)
    with np.errstate(over="ignore"):
        unit = np.abs(np.spacing(ref64.astype(np.float32))).astype(np.float64)
    return np.abs(got - ref64) / unit


def test_expf_against_float64(oracle_lib):
    a, _ = inputs(0)
    x = b2f(a)
    got = host(0)[0]
    with np.errstate(over="ignore", invalid="ignore"):
        ref = np.exp(x.astype(np.float64))
    inrange = np.isfinite(x) & (x > -87.0) & (x <= 88.0)
    normal = inrange & (ref >= 2.0 ** -126) & (ref <= float(np.finfo(np.float32).max))
    err = _ulps(got[normal], ref[normal])
    print(f"ct_expf: {int(normal.sum())} normal results, max error {err.max():.4f} ulp at x = {x[normal][err.argmax()]!r}")
    assert err.max() <= 2.0                                   # the bound ct_fmath.h states
    # e^-87 = 1.6e-38 is above 2^-126 = 1.18e-38: no in-range result is subnormal; the smallest scale, 2^-126 at
    # n = -126, meets a polynomial value of 1.36 or more
    assert not (inrange & ~normal).any()
    assert a[inrange & (x < -86.99)].size > 1000 and np.all(got[inrange] >= 0x00800000)     # (n = -126 is in the set)
    # range checks and special values
    assert np.all(got[np.isfinite(x) & (x <= -87.0)] == 0) and np.all(got[x == -np.inf] == 0)
    assert np.all(got[x > 88.0] == 0x7f800000)
    nan = np.isnan(x)
    assert nan.sum() == len(NANS) and np.array_equal(got[nan], a[nan])     # a NaN comes back as it went in
    assert got[a == 0][0] == bits_of(1.0) and got[a == 0x80000000][0] == bits_of(1.0)


def _check_log_specials(a, got):
    x = b2f(a)
    assert np.all(got[x == 0] == 0xff800000)                  # -inf for both zeros
    assert is_nan_bits(got[(x < 0) | np.isnan(x)]).all()
    assert np.all(got[x == np.inf] == 0x7f800000)
    return np.isfinite(x) & (x > 0)


def test_logf_against_float64(oracle_lib):
    a, _ = inputs(1)
    got = host(1)[0]
    pos = _check_log_specials(a, got)
    x = b2f(a)[pos]
    ref = np.log(x.astype(np.float64))
    err = _ulps(got[pos], ref)
    print(f"ct_logf: {int(pos.sum())} positive arguments, max error {err.max():.4f} ulp at x = {x[err.argmax()]!r}")
    assert err.max() <= 2.0                                   # the bound ct_fmath.h states
    assert got[a == bits_of(1.0)][0] == 0


def test_log2f_against_float64(oracle_lib):
    a, _ = inputs(2)
    got = host(2)[0]
    pos = _check_log_specials(a, got)
    x = b2f(a)[pos]
    ref = np.log2(x.astype(np.float64))
    rel = np.abs(b2f(got[pos]).astype(np.float64) - ref) / np.maximum(np.abs(ref), 1e-300)
    print(f"ct_log2f: max relative error {rel.max() / 2.0 ** -23:.4f} x 2^-23 at x = {x[rel.argmax()]!r}")
    # ct_logf within 2 ulp (<= 2 * 2^-23 relative), the float constant 1/ln 2 within 2^-24, one rounding of the product
    # within 2^-24: 3 * 2^-23, and the second-order terms
    assert rel.max() <= 3.01 * 2.0 ** -23


def test_powf_against_float64(oracle_lib):
    a, b = inputs(3)
    got = host(3)[0]
    x = b2f(a)
    sel = (x >= np.float32(1e-4)) & (x <= 1.0) & (b == bits_of(1 / 2.2))
    assert sel.sum() > 100000
    ref = x[sel].astype(np.float64) ** float(np.float32(1 / 2.2))
    rel = np.abs(b2f(got[sel]).astype(np.float64) / ref - 1.0)
    print(f"ct_powf: {int(sel.sum())} tonemap arguments in [1e-4, 1], max relative error {rel.max():.3e}")
    assert rel.max() < 2e-6                                   # the bound of test_fmath_accuracy, on its range only
    assert np.all(got[x == 0] == 0)
    assert is_nan_bits(got[(x < 0) | np.isnan(x)]).all()


def test_sincosf_against_float64(oracle_lib):
    a, _ = inputs(4)
    s, c = host(4)
    x = b2f(a)
    dom = np.abs(x) <= 8.0                                    # the documented domain
    x64 = x[dom].astype(np.float64)
    es = np.abs(b2f(s[dom]).astype(np.float64) - np.sin(x64))
    ec = np.abs(b2f(c[dom]).astype(np.float64) - np.cos(x64))
    print(f"ct_sincosf: {int(dom.sum())} arguments in [-8, 8], max absolute error sin {es.max():.3e}, cos {ec.max():.3e}")
    assert es.max() < 2e-7 and ec.max() < 2e-7                # the bound of test_fmath_accuracy
    assert s[a == 0][0] == 0 and c[a == 0][0] == bits_of(1.0)


def _tea4_numpy(v0, v1):
    v0, v1 = v0.astype(np.uint32), v1.astype(np.uint32)
    s0 = np.uint32(0)
    with np.errstate(over="ignore"):
        for _ in range(4):
            s0 = np.uint32((int(s0) + 0x9e3779b9) & 0xffffffff)
            v0 = v0 + ((((v1 << np.uint32(4)) + np.uint32(0xa341316c)) ^ (v1 + s0)) ^ ((v1 >> np.uint32(5)) + np.uint32(0xc8013ea4)))
            v1 = v1 + ((((v0 << np.uint32(4)) + np.uint32(0xad90777d)) ^ (v0 + s0)) ^ ((v0 >> np.uint32(5)) + np.uint32(0x7e95761e)))
    return v0


@pytest.mark.parametrize("fn", [7, 8, 9, 10, 11, 12, 13, 14])
def test_exact_functions_against_numpy(oracle_lib, fn):
    """Division, the integer functions, floor and the filter weights are single IEEE operations or integer arithmetic:
    numpy's float32 / uint32 arithmetic is an independent exact reference for the oracle's side of the GPU comparison."""
    a, b = inputs(fn)
    got = host(fn)
    x = b2f(a)
    with np.errstate(all="ignore"):
        if fn == 7:
            want = (f2b(x / b2f(b)), None)
        elif fn == 8:
            want = (f2b((a.astype(np.float64) / 2.0 ** 24).astype(np.float32)), None)
        elif fn == 9:
            want = (_tea4_numpy(a, b), None)
        elif fn == 10:
            state = ((a.astype(np.uint64) * np.uint64(1664525) + np.uint64(1013904223)) & np.uint64(0xffffffff)).astype(np.uint32)
            want = (state & np.uint32(0x00ffffff), state)
        elif fn == 11:
            want = (np.floor(x.astype(np.float64)).astype(np.int64).astype(np.int32).view(np.uint32), None)
        else:
            frac = np.where(np.isfinite(x), np.minimum(x - np.floor(x), FRAC_MAX), FRAC_MAX)
            if fn == 14:
                frac = np.rint(frac * np.float32(256.0)) * np.float32(1.0 / 256.0)
            want = (f2b(frac.astype(np.float32)), None)
    for k in (0, 1):
        w = want[k] if want[k] is not None else np.zeros(a.size, np.uint32)
        bad = got[k] != w
        if fn == 7:
            bad &= ~(is_nan_bits(got[k]) & is_nan_bits(w))
        assert not bad.any(), (fn, FN[fn], k, hex(int(a[bad][0])), hex(int(got[k][bad][0])), hex(int(w[bad][0])))
    if fn == 7:   # a subnormal denominator and a subnormal quotient are computed, not flushed
        one, tiny = bits_of(1.0), 0x00000001
        r0, _ = O.math_eval(7, np.array([tiny, one], np.uint32), np.array([one, tiny], np.uint32))
        assert r0[0] == tiny and r0[1] == 0x7f800000
    if fn == 14:  # a fraction above 255.5/256 becomes a weight of exactly 1.0
        with np.errstate(invalid="ignore"):
            top = (x - np.floor(x) > np.float32(255.5 / 256)) & (x > 0)
        assert top.sum() > 4096 and np.all(got[0][top] == bits_of(1.0))


@pytest.fixture(scope="module")
def clang_oracle(tmp_path_factory):
    if not CLANG.exists():
        pytest.skip(f"{CLANG} is not installed")
    so = tmp_path_factory.mktemp("clang_oracle") / "libct_oracle_clang.so"
    subprocess.run([str(CLANG), "-std=gnu11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-fvisibility=hidden",
                    "-o", str(so), str(ROOT / "oracle" / "ct_oracle.c"), "-lm"], check=True)
    return O.bind_math_eval(C.CDLL(str(so)))


@pytest.mark.parametrize("fn", sorted(FN))
def test_clang_host_build_agrees_with_gcc(oracle_lib, clang_oracle, fn):
    """The same translation unit under ROCm's clang, for the host, with the device build's floating-point flags: bit for
    bit the gcc build.  A GPU mismatch that this test does not share is the device's, not the compiler front end's."""
    a, b = inputs(fn)
    got = O.math_eval(fn, a, b, L=clang_oracle)
    ref = host(fn)
    for k in (0, 1):
        bad = got[k] != ref[k]
        assert not bad.any(), (fn, FN[fn], k, int(bad.sum()), hex(int(a[bad][0])), hex(int(got[k][bad][0])), hex(int(ref[k][bad][0])))


THICK_MFP = 7000.0 / 512.0 / 79.9      # cloud_size_m / mean_free_path_m * sample_step = 79.9 with the default size and step


def test_create_refuses_an_optical_depth_per_step_of_80(product_lib):
    tex = np.full((8, 8, 8), 255, np.uint8)
    mfp = 7000.0 / 512.0 / 80.0        # 175/1024, exact: the depth per step is exactly 80.0f
    assert np.float32(7000.0) / np.float32(mfp) * np.float32(1.0 / 512.0) == np.float32(80.0)
    with pytest.raises(_lib.CloudTraceError) as e:
        ds.CloudTracer(tex, width=16, height=16, mean_free_path_m=mfp)
    assert e.value.code == _lib.CT_E_INVAL and "optical depth per step" in e.value.message
    depth = np.float32(7000.0) / np.float32(THICK_MFP) * np.float32(1.0 / 512.0)
    assert 79.89 < float(depth) < 79.91


# =====================================================================================================================
# GPU half
# =====================================================================================================================
@pytest.fixture(scope="module")
def tracer():
    tr = ds.CloudTracer(np.zeros((4, 4, 4), np.uint8), width=8, height=8)
    yield tr
    tr.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fn", sorted(FN))
def test_device_function_equals_host_bit_for_bit(tracer, fn):
    a, b = inputs(fn)
    got = tracer.debug_math_eval(fn, a, b)
    assert_same_bits(fn, got, host(fn), ("device", "host"))


# (which, ranges of bit patterns [lo, hi]): the tested count is computed here from the bounds
EXHAUSTIVE = {
    2: [(0x80000000, bits_of(-87.0) - 1), (0x00000000, 0x00000000)],           # -87 < x <= -0.0f, and +0.0f
    3: [(0x00800000, 0x7f7fffff)],                                             # every positive normal float
    4: [(0x00000000, bits_of(2.0 ** 31) - 1), (0x80000000, bits_of(-2.0 ** 31))],  # -2^31 <= x < 2^31
    5: [(0x00000000, 0x7f7fffff), (0x80000000, 0xff7fffff)],                   # every finite float
}


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(EXHAUSTIVE))
def test_device_only_variants_exhaustively(tracer, which):
    """expf_inrange == ct_expf, logf_above_one == ct_logf, floor_to_int == (int32_t)floorf, fract_ == the oracle's fracf
    for EVERY float of the stated range, compared on the device in one pass."""
    r = tracer.debug_math_selftest(which)
    want = sum(hi - lo + 1 for lo, hi in EXHAUSTIVE[which])
    assert r["tested"] == want and r["mismatches"] == 0, (which, want, r, hex(r["first_bad_bits"]))


@pytest.mark.gpu
def test_fract_outside_the_finite_floats_is_as_documented(tracer):
    """The one region where a device function and its host twin differ, outside what any caller passes: for +-inf and NaN
    the fract instruction returns a NaN, while the oracle's fracf() -- fminf(NaN, 1 - 2^-24) -- returns the clamp, and the
    fixed-point weight rounds that to 1.0.  Every FINITE float agrees (self-test 5).  Pinned here so that the comment at
    fract_ in ct_device.hpp stays true."""
    a = np.array([0x7f800000, 0xff800000] + NANS, np.uint32)
    for fn in (12, 13, 14):
        dev, _ = tracer.debug_math_eval(fn, a)
        hst, _ = O.math_eval(fn, a)
        assert is_nan_bits(dev).all(), (fn, dev)
        assert np.all(hst == (bits_of(1.0) if fn == 14 else bits_of(FRAC_MAX))), (fn, hst)


@pytest.mark.gpu
def test_math_eval_refuses_bad_arguments(tracer):
    L, h = tracer.L, tracer.h
    buf = np.zeros(8, np.uint32)
    p = buf.ctypes.data_as(C.c_void_p)
    for args in ((0, p, 0, p), (0, p, (1 << 24) + 1, p), (0, None, 4, p), (0, p, 4, None), (-1, p, 4, p), (len(FN), p, 4, p)):
        assert L.ct_debug_math_eval(h, *args) == _lib.CT_E_INVAL, args
    assert L.ct_debug_math_eval(None, 0, p, 4, p) == _lib.CT_E_INVAL
    with pytest.raises(_lib.CloudTraceError) as e:
        tracer.debug_math_eval(0, np.zeros(0, np.uint32))
    assert e.value.code == _lib.CT_E_INVAL
    for which in (-1, 6):
        with pytest.raises(_lib.CloudTraceError) as e:
            tracer.debug_math_selftest(which)
        assert e.value.code == _lib.CT_E_INVAL
    # the handle still works, and the last item of a block-sized and of a ragged count is written
    for n in (1, 256, 257):
        r0, r1 = tracer.debug_math_eval(10, np.arange(n, dtype=np.uint32))
        w0, w1 = O.math_eval(10, np.arange(n, dtype=np.uint32))
        assert np.array_equal(r0, w0) and np.array_equal(r1, w1)


@pytest.mark.gpu
@pytest.mark.parametrize("estimator", [0, 1])
def test_optical_depth_per_step_just_under_the_limit(estimator):
    """ct_create accepts a depth per step below 80 and expf_inrange is valid down to -87: at 79.9 on a volume of 255s a
    full step multiplies the transmittance T by e^-79.9 ~ 2e-35 and a second one takes it below the normal range: the
    back-off's xi / T then divides by a tiny or subnormal T.  Radiance and counters equal the oracle's, one subframe per mode."""
    tex = np.full((8, 8, 8), 255, np.uint8)
    for mode in (0, 1, 2):
        tr = ds.CloudTracer(tex, width=16, height=16, mode=mode, estimator=estimator, mean_free_path_m=THICK_MFP)
        orc = O.Oracle(tex, 16, 16, mode=mode, fast=True, estimator=estimator, mean_free_path_m=THICK_MFP)
        tr.render_subframe(1)
        got, ref = tr.frame(), orc.render_subframe(1)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (estimator, mode)
        assert tr.counters() == orc.counters.as_dict(), (estimator, mode)
        assert tr.counters()["scatter_events"] > 0
        tr.close()
