"""The image kernels -- accumulate_batch_kernel, reinhard_fused_kernel, converged_kernel, converged_freeze_kernel
(csrc/ct_kernels.hip) -- on SYNTHETIC frames: caller-owned buffers of every awkward shape, value range and count, not the
narrow range of values a rendered cloud produces.

Two references:

1. the CPU oracle (O.reinhard, O.is_converged, O.accumulate), which the kernels must equal bit for bit, NaNs included;
2. a plain float64 restatement in numpy, written below from reinhard.cu:20-84, progressive.cu:17-27 and Camera.cpp:232-268
   as the kernels' comments quote them.  It shares no code and no ct_fmath.h arithmetic with oracle or product, and is
   what catches a misreading that oracle and kernels have in common.

The tolerances against (2) are measured on the CPU -- oracle against float64, on the very inputs (same seeds) the GPU
tests use -- by the tests without a `gpu` mark in this file; the GPU tests apply the same constants to the product.
"""
import zlib

import numpy as np
import pytest

import _oracle as O
from conftest import sphere_volume

gpu = pytest.mark.gpu

SHAPES = [(1, 1), (3, 5), (4, 1), (37, 21), (33, 9), (31, 7), (64, 1024), (64, 1030), (5, 2049), (8, 4096), (1028, 8),
          (2048, 3), (4100, 2), (257, 2049), (1024, 1024)]                       # (width, height)
FAMILIES = ["uniform", "lognormal", "render_like", "black", "equal", "bright", "ramp"]
EXPOSURES = [0.4, 0.05, 3.0, 1e-6, 1e4]

# ---------------------------------------------------------------------------------------------------------------------
# Tolerances of the float64 reference.  Each is the worst figure of the ORACLE against float64 over the inputs of this
# file (test_oracle_against_float64_* print and bound them), times the factor named.
# ---------------------------------------------------------------------------------------------------------------------
# avg luminance, relative error: measured worst 4.72e-5 (8x4096 ramp: 4096 float32 additions in a row; 2.5e-5 at 257x2049,
# 1.4e-5 at 1024x1024, below 1e-6 under 1000 rows), x 4
AVG_RTOL = 1.9e-4
# a screen byte may differ from floor(v64) by one only where v64 lies within SCREEN_D of an integer: measured worst distance
# 3.29e-4 (12288x2 lognormal, exposure 3; 3.4e-5 over the shapes of SHAPES), x 4
SCREEN_D = 1.32e-3
# share of the bytes of one image that may be off by one: 0.5 %.  The oracle's worst share is 0.11 % (4100x2 ramp; the ramp
# puts one pixel in 512 on a boundary on purpose), 0.012 % on any other family: under the 0.25 % this cap presupposes
SCREEN_OFF_SHARE = 0.005
SCREEN_OFF_SHARE_ORACLE = 0.0025
# Welford after N samples: |mean32 - mean64| <= C_MEAN * N * 2^-24 * max|x| + N * 2^-149, and
# |M2_32 - M2_64| <= C_M2 * N * 2^-24 * max|x|^2 + N * 2^-149 (for a run that continues an uploaded state: N = its
# length, max|x| taken over the samples and the state's mean, and the state's |M2| added to max|x|^2).  The second term is
# the spacing of float32 subnormals: a denormal sample has no relative precision for the first term to scale.
# measured worst ratios: mean 0.672 (the three ids round 2^24; 0.073 from id 1), M2 5.29 (31x7 uniform, 4096 ids), x 4
C_MEAN = 2.69
C_M2 = 21.2
# convergence: a pixel whose float64 rel_ci or abs_ci lies within this relative distance of its threshold may fall either way
CI_BAND = 1e-5

LUM = (0.265068, 0.67023428, 0.06409157)      # reinhard.cu's luminance weights (alpha weighs 0)


def _seed(*parts):
    return zlib.crc32(":".join(str(p) for p in parts).encode())


# ---------------------------------------------------------------------------------------------------------------------
# float64 restatements
# ---------------------------------------------------------------------------------------------------------------------
def reinhard64(mean, exposure):
    """reinhard.cu:20-84 in float64: -> (v [H,W,3] = the channel values before truncation to a byte, avg)."""
    m = mean.astype(np.float64)
    lum = m[..., 0] * LUM[0] + m[..., 1] * LUM[1] + m[..., 2] * LUM[2]
    avg = float(np.mean(lum + 1e-5))                                      # firstPass + secondPass
    with np.errstate(all="ignore"):
        ld = lum * float(exposure) / avg                                  # applyReinhard
        ld = ld / (1.0 + ld)
        c = m[..., :3] * (ld / lum)[..., None]
        c = np.where(np.isnan(c), 1.0, np.clip(c, 0.0, 1.0))              # optix clamp: fmaxf(0, fminf(NaN, 1)) = 1
        v = c ** (1.0 / 2.2) * 255.0
    return v, avg


def welford64(samples):
    """Two passes over float64 samples [N, ...]: -> (mean, sum of squared deviations)."""
    x = samples.astype(np.float64)
    with np.errstate(all="ignore"):
        mean = x.sum(axis=0) / x.shape[0]
        m2 = ((x - mean) ** 2).sum(axis=0)
    return mean, m2


def converged64(mean, m2, n):
    """Camera.cpp:232-268 in float64: -> (fewest, most) pixels outside the interval, the difference being the pixels
    whose confidence interval lies within CI_BAND of a threshold."""
    mx, vx = mean[..., 0].astype(np.float64).ravel(), m2[..., 0].astype(np.float64).ravel()
    with np.errstate(all="ignore"):
        sigma = np.sqrt(vx / float(n))
        abs_ci = 1.96 * sigma / np.sqrt(float(n))
        rel_ci = abs_ci / (mx + 2.0 ** -23)                               # FLT_EPSILON
        surely = (rel_ci < 0.02 * (1 - CI_BAND)) | (abs_ci < 1e-2 * (1 - CI_BAND))
        maybe = (rel_ci < 0.02 * (1 + CI_BAND)) | (abs_ci < 1e-2 * (1 + CI_BAND))
    return int(mx.size - maybe.sum()), int(mx.size - surely.sum())


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def ramp_image(w, h, exposure):
    """Grey pixels whose tonemapped value lands on a byte boundary k, and the float32 neighbours of that input on either
    side; the rest of the frame is black.  For a grey pixel g the screen value is (ld / (1 + ld) / S) ** (1 / 2.2) * 255
    with ld = g * S * exposure / avg and S the sum of the luminance weights: inverted for ld, and avg follows from
    avg = mean(lum) + 1e-5 = avg * sum(ld) / (P * exposure) + 1e-5.  About half of such bytes come out one lower in
    float32, so that the off-by-one share of the image stays a fifth of its cap the boundaries take one pixel in 512: m = P / 1536
    values of k spread over 1 .. kmax, three pixels each (every k from 1 to 255 in a frame of 400 k pixels; none in a frame
    of fewer than 1536 pixels, which is simply black).  kmax is the largest that keeps sum(ld) / (P * exposure) below 1/2."""
    P, S = w * h, sum(LUM)
    img = np.zeros((P, 4), np.float32)
    img[:, 3] = 1.0
    m = min(255, P // 1536)
    if m == 0:
        return img.reshape(h, w, 4)
    for kmax in range(255, 0, -1):
        k = np.repeat(np.unique(np.rint(np.linspace(1, kmax, min(m, kmax))).astype(np.int64)), 3)
        st = S * (k / 255.0) ** 2.2
        ld = st / (1.0 - st)
        r = ld.sum() / P / exposure
        if r <= 0.5:
            break
    else:
        raise AssertionError("no ramp fits this frame and exposure")
    avg = 1e-5 / (1.0 - r)
    g = (ld * avg / exposure / S).astype(np.float32)
    which = np.arange(len(k)) % 3
    g = np.where(which == 1, np.nextafter(g, np.float32(0)), np.where(which == 2, np.nextafter(g, np.float32(np.inf)), g))
    img[:len(g), :3] = g[:, None]
    return img.reshape(h, w, 4)


def make_image(w, h, family, exposure):
    """float32 [H, W, 4], alpha 1 (the product's case)."""
    rng = np.random.default_rng(_seed("image", w, h, family))
    img = np.zeros((h, w, 4), np.float32)
    if family == "uniform":
        img[..., :3] = rng.random((h, w, 3), dtype=np.float32)
    elif family == "lognormal":                                          # about 12 decades
        img[..., :3] = (10.0 ** rng.uniform(-6, 6, (h, w, 1)) * rng.uniform(0.2, 1.0, (h, w, 3))).astype(np.float32)
    elif family == "render_like":                                        # half the pixels exactly black
        img[..., :3] = rng.random((h, w, 3), dtype=np.float32) * 0.3 * (rng.random((h, w, 1)) < 0.5)
    elif family == "black":
        pass
    elif family == "equal":
        img[..., :3] = (0.25, 0.5, 0.125)
    elif family == "bright":
        img[h // 2, w // 2, :3] = (300.0, 200.0, 100.0)
    elif family == "ramp":
        return ramp_image(w, h, exposure)
    else:
        raise ValueError(family)
    img[..., 3] = 1.0
    return img


def tonemap_cases():
    """A third of shapes x families (every shape at least twice, every family five times), the exposures dealt round."""
    out = []
    for i, (w, h) in enumerate(SHAPES):
        for j, family in enumerate(FAMILIES):
            if (i + j) % 3 == 0:
                out.append((w, h, family, EXPOSURES[(i + 2 * j) % len(EXPOSURES)]))
    return out + [(257, 2049, "ramp", 0.4), (1024, 1024, "ramp", 3.0)]      # (the frames that hold every boundary)


TONEMAP_CASES = tonemap_cases()
WIDEST_CASES = [(w, h, family, exposure) for w, h in ((12288, 1), (12288, 2)) for family, exposure in (("uniform", 0.4), ("lognormal", 3.0))]
_case_id = lambda c: f"{c[0]}x{c[1]}-{c[2]}-{c[3]:g}"


def conv_inputs(w, h, n):
    """(mean, M2) whose confidence intervals spread over four decades round both thresholds; the channels the rule does
    not read hold NaNs and noise."""
    rng = np.random.default_rng(_seed("conv", w, h, n))
    mean = rng.standard_normal((h, w, 4)).astype(np.float32)
    m2 = rng.standard_normal((h, w, 4)).astype(np.float32)
    mean[..., 1:][rng.random((h, w, 3)) < 0.1] = np.nan
    m2[..., 1:][rng.random((h, w, 3)) < 0.1] = np.nan
    mu = 10.0 ** rng.uniform(-3, 1, (h, w))
    ci = 10.0 ** rng.uniform(-4, 0, (h, w))                              # the absolute interval aimed at
    sigma = ci * np.sqrt(float(n)) / 1.96
    mean[..., 0] = mu
    m2[..., 0] = sigma * sigma * float(n)
    return mean, m2


def exact_bad_inputs(w, h, n, k, seed=0):
    """mean 1, M2 0 (inside the interval) everywhere but on exactly k pixels, the last one of the frame among them, whose
    interval is far outside: abs_ci = 1.96."""
    rng = np.random.default_rng(_seed("exact", w, h, n, k, seed))
    P = w * h
    mean = np.ones((P, 4), np.float32)
    m2 = np.zeros((P, 4), np.float32)
    where = rng.choice(P - 1, k - 1, replace=False)
    m2[where, 0] = float(n) * float(n)
    m2[P - 1, 0] = float(n) * float(n)
    return mean.reshape(h, w, 4), m2.reshape(h, w, 4)


def step32(x, steps):
    x = np.float32(x)
    for _ in range(abs(steps)):
        x = np.nextafter(x, np.float32(np.inf if steps > 0 else -np.inf))
    return x


def threshold_inputs(w, h, n):
    """Pixels on the per-pixel boundaries: the float32 neighbours (M2 stepped with nextafter) of rel_ci = 0.02 at mean 1
    (abs_ci = 0.02 does not pass) and of abs_ci = 0.01 at mean 0.1 (rel_ci = 0.1 does not pass), and the special values.
    -> (mean, M2)."""
    P = w * h
    mean = np.ones((P, 4), np.float32)
    m2 = np.zeros((P, 4), np.float32)
    nf = float(np.float32(n))
    rows = []
    for mu, ci in ((1.0, 0.02 * (1.0 + 2.0 ** -23)), (0.1, 0.01)):
        centre = np.float32((ci * np.sqrt(nf) / 1.96) ** 2 * nf)
        for s in range(-12, 13):
            rows.append((mu, step32(centre, s)))
    for mu, v in ((0.0, 0.0), (0.0, 1e-12), (0.0, 1e9), (-2.0 ** -23, 0.0), (-2.0 ** -23, 1.0), (-3.0, 1e9), (1.0, np.inf),
                  (1.0, -1.0), (1.0, -0.0), (1.0, -1e-30), (1.0, np.nan), (np.nan, 0.0), (np.nan, 1e9), (np.inf, 1e9), (1.0, 1e-45)):
        rows.append((mu, v))
    rows = (rows * (P // len(rows) + 1))[:min(P, 4 * len(rows))]
    at = np.random.default_rng(_seed("threshold", w, h)).choice(P, len(rows), replace=False)
    mean[at, 0] = [r[0] for r in rows]
    m2[at, 0] = [r[1] for r in rows]
    return mean.reshape(h, w, 4), m2.reshape(h, w, 4)


SPECIALS = ["nan_once", "inf_once", "ninf_once", "denormal", "denormal_difference", "huge", "flt_max"]


def caller_frames(w, h, family, first, count, arbitrary_alpha=True):
    """float32 [count, H, W, 4] caller-owned samples for the ids first .. first + count - 1, with special values sprinkled
    in at fixed (pixel, channel) places: -> (frames, kind [H, W, 4] = index into SPECIALS or -1)."""
    rng = np.random.default_rng(_seed("frames", w, h, family, first, count))
    if family == "uniform":
        x = rng.random((count, h, w, 4), dtype=np.float32)
    elif family == "lognormal":
        x = (10.0 ** rng.uniform(-6, 6, (count, h, w, 4)) * rng.choice([-1.0, 1.0], (count, h, w, 4))).astype(np.float32)
    elif family == "render_like":
        x = (rng.random((count, h, w, 4), dtype=np.float32) * 0.3 * (rng.random((1, h, w, 1)) < 0.5)).astype(np.float32)
    else:
        raise ValueError(family)
    if not arbitrary_alpha:
        x[..., 3] = 1.0
    kind = np.full((h, w, 4), -1, np.int64)
    n_special = min(h * w * 4, max(len(SPECIALS), h * w * 4 // 8))
    at = rng.choice(h * w * 4, n_special, replace=False)
    kind.reshape(-1)[at] = np.arange(n_special) % len(SPECIALS)
    u = rng.random((count, h, w, 4), dtype=np.float32) + np.float32(0.5)
    when = rng.integers(0, count, (h, w, 4))                             # the one sample of the *_once kinds
    once = np.arange(count)[:, None, None, None] == when[None]
    for i, name in enumerate(SPECIALS):
        sel = np.broadcast_to(kind == i, x.shape)
        if name == "nan_once":
            x[sel & once] = np.nan
        elif name == "inf_once":
            x[sel & once] = np.inf
        elif name == "ninf_once":
            x[sel & once] = -np.inf
        elif name == "denormal":
            x[sel] = (u * np.float32(1e-40))[sel]
        elif name == "denormal_difference":                              # normal numbers that differ by a subnormal
            x[sel] = (np.float32(2e-38) + (u * np.float32(3e-42)))[sel]
        elif name == "huge":                                             # (nr - mu) * (nr - nm) overflows
            x[sel] = (u * np.float32(1e30))[sel]
        elif name == "flt_max":
            x[sel] = np.where(once, np.float32(3.4028235e38), u)[sel]
    return x, kind


def oracle_accumulate(frames, first, mean=None, m2=None):
    mean = np.zeros(frames.shape[1:], np.float32) if mean is None else mean.copy()
    m2 = np.zeros(frames.shape[1:], np.float32) if m2 is None else m2.copy()
    for i in range(frames.shape[0]):
        O.accumulate(np.ascontiguousarray(frames[i]), mean, m2, first + i)
    return mean, m2


# ---------------------------------------------------------------------------------------------------------------------
# comparisons (used for oracle and product alike); each returns the figures the tolerance constants were taken from
# ---------------------------------------------------------------------------------------------------------------------
def same_values(a, b):
    """Equal, NaNs included and in the same places."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a, b, equal_nan=True)


def check_tonemap_against_float64(screen, avg, image, exposure, share_cap=SCREEN_OFF_SHARE):
    v64, avg64 = reinhard64(image, exposure)
    avg_err = abs(avg - avg64) / avg64
    diff = screen[..., :3].astype(np.int64) - np.floor(v64).astype(np.int64)
    off = diff != 0
    dist = np.abs(v64 - np.rint(v64))
    worst_dist = float(dist[off].max()) if off.any() else 0.0
    share = float(off.mean())
    print(f"avg rel err {avg_err:.3e}  bytes off {int(off.sum())} ({share:.3e})  worst distance {worst_dist:.3e}")
    assert avg_err <= AVG_RTOL, (avg, avg64)
    assert np.abs(diff).max() <= 1, "a byte is off by more than one"
    assert worst_dist <= SCREEN_D, "a byte is off by one where float64 is not next to an integer"
    assert share <= share_cap
    assert (screen[..., 3] == 255).all()
    return avg_err, worst_dist, share


def check_welford_against_float64(mean, m2, mean64, m2_64, count, scale, m2_scale, finite):
    """`finite`: the elements all of whose samples are finite and below 1e18 (whose squares float32 can hold)."""
    floor = count * 2.0 ** -149
    unit = count * 2.0 ** -24
    with np.errstate(all="ignore"):
        e_mean = np.abs(mean.astype(np.float64) - mean64)[finite]
        e_m2 = np.abs(m2.astype(np.float64) - m2_64)[finite]
        assert np.isfinite(e_mean).all() and np.isfinite(e_m2).all(), "a non-finite value where every sample is finite"
        r_mean = np.max(np.maximum(e_mean - floor, 0.0) / np.maximum(unit * scale[finite], 1e-300), initial=0.0)
        r_m2 = np.max(np.maximum(e_m2 - floor, 0.0) / np.maximum(unit * m2_scale[finite], 1e-300), initial=0.0)
    print(f"welford: N {count}  mean ratio {r_mean:.3f}  M2 ratio {r_m2:.3f}")
    assert r_mean <= C_MEAN and r_m2 <= C_M2
    return float(r_mean), float(r_m2)


def check_caller_run(mean, m2, frames, kind):
    """A run from id 1 against two-pass float64, and the non-finite samples staying where they are."""
    x = frames.astype(np.float64)
    finite_samples = np.isfinite(frames).all(axis=0)
    mx = np.abs(np.where(np.isfinite(x), x, 0.0)).max(axis=0)
    finite = finite_samples & (mx < 1e18)
    # a non-finite sample makes its own channel of its own pixel non-finite for good, and no other
    assert np.array_equal(np.isfinite(mean), finite_samples)
    assert np.isfinite(m2[finite]).all()
    for name in ("nan_once", "inf_once", "ninf_once"):
        assert not np.isfinite(mean[kind == SPECIALS.index(name)]).any()
    mean64, m2_64 = welford64(np.where(finite[None], x, 0.0))
    return check_welford_against_float64(mean, m2, mean64, m2_64, frames.shape[0], mx, mx * mx, finite)


def high_id_run(w, h):
    """A state after 2^24 - 2 samples and the three frames that follow it."""
    rng = np.random.default_rng(_seed("high", w, h))
    mean0 = rng.random((h, w, 4), dtype=np.float32)
    m2_0 = rng.random((h, w, 4), dtype=np.float32) * np.float32(2 ** 24 * 0.08)
    frames = rng.random((3, h, w, 4), dtype=np.float32)
    return mean0, m2_0, frames, 2 ** 24 - 1


def check_high_id_run(mean, m2, mean0, m2_0, frames, first):
    mu, var = mean0.astype(np.float64), m2_0.astype(np.float64)
    for i in range(frames.shape[0]):                                     # progressive.cu:17-27 in float64, exact counts
        x = frames[i].astype(np.float64)
        nm = mu + (x - mu) / float(first + i)
        var = var + (x - mu) * (x - nm)
        mu = nm
    scale = np.maximum(np.abs(frames).max(axis=0), np.abs(mean0)).astype(np.float64)
    everywhere = np.ones(mean.shape, bool)
    return check_welford_against_float64(mean, m2, mu, var, frames.shape[0], scale, scale * scale + np.abs(m2_0), everywhere)


ACCUMULATE_RUNS = [(33, 9, "uniform", 40), (31, 7, "lognormal", 40), (1, 1, "uniform", 40), (37, 21, "render_like", 40),
                   (3, 5, "lognormal", 40), (31, 7, "uniform", 4096), (1, 1, "lognormal", 4096)]
CONVERGED_COUNTS = [99, 100, 101, 1000, 2 ** 24 + 1]


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the oracle against float64 (fixes the tolerances; no GPU)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TONEMAP_CASES + WIDEST_CASES, ids=_case_id)
def test_oracle_against_float64_tonemap(case):
    w, h, family, exposure = case
    image = make_image(w, h, family, exposure)
    screen, avg = O.reinhard(image, exposure)
    check_tonemap_against_float64(screen, avg, image, exposure, share_cap=SCREEN_OFF_SHARE_ORACLE)


def test_ramp_reaches_the_byte_boundaries():
    """The ramp does what it is for: at 1024x1024, exposure 3, float64 puts a value within 1e-4 of every k = 1 .. 255."""
    v64, _ = reinhard64(ramp_image(1024, 1024, 3.0), 3.0)
    grey = v64.reshape(-1, 3)[:765:3, 0]
    assert np.abs(grey - np.arange(1, 256)).max() < 1e-4


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_oracle_against_float64_converged(shape):
    w, h = shape
    for n in CONVERGED_COUNTS:
        mean, m2 = conv_inputs(w, h, n)
        ok, bad = O.is_converged(mean, m2, n)
        if n < 100:
            assert (ok, bad) == (False, w * h)
            continue
        lo, hi = converged64(mean, m2, n)
        assert hi - lo == 0 or (hi - lo) * 1000 < w * h, "too many undecided pixels: change the inputs"
        assert lo <= bad <= hi and ok == (bad < 500)
        mean, m2 = threshold_inputs(w, h, n)                             # (no float64 here: these sit ON the thresholds)
        assert O.is_converged(mean, m2, n)[1] <= w * h
    if w * h > 501:
        for k in (499, 500, 501):
            mean, m2 = exact_bad_inputs(w, h, 100, k)
            assert converged64(mean, m2, 100) == (k, k)
            assert O.is_converged(mean, m2, 100) == (k < 500, k)


@pytest.mark.parametrize("run", ACCUMULATE_RUNS, ids=lambda r: f"{r[0]}x{r[1]}-{r[2]}-{r[3]}")
def test_oracle_against_float64_accumulate(run):
    w, h, family, count = run
    frames, kind = caller_frames(w, h, family, 1, count)
    mean, m2 = oracle_accumulate(frames, 1)
    check_caller_run(mean, m2, frames, kind)


def test_oracle_against_float64_accumulate_high_ids():
    mean0, m2_0, frames, first = high_id_run(33, 9)
    mean, m2 = oracle_accumulate(frames, first, mean0, m2_0)
    check_high_id_run(mean, m2, mean0, m2_0, frames, first)


def test_oracle_counts_nan_and_negative_m2_as_unconverged():
    mean, m2 = np.ones((8, 100, 4), np.float32), np.zeros((8, 100, 4), np.float32)
    m2[0, :7, 0] = np.nan
    m2[3, :5, 0] = -1.0
    mean[5, :3, 0] = np.nan            # (with M2 = 0 the absolute interval is 0 and passes whatever the mean)
    m2[5, :3, 0] = 1e9
    assert O.is_converged(mean, m2, 100) == (True, 15)
    assert converged64(mean, m2, 100) == (15, 15)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
_handles = {}


def handle(w, h, shard_index=0, shard_count=1):
    """One handle per frame size, on a volume that costs nothing to set up."""
    import deepestscatter_amd as ds
    key = (w, h, shard_index, shard_count)
    if key not in _handles:
        _handles[key] = ds.CloudTracer(sphere_volume(8), width=w, height=h, shard_index=shard_index, shard_count=shard_count)
    return _handles[key]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for tr in _handles.values():
        tr.close()
    _handles.clear()


def to_device(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def from_device(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def tonemap_three_ways(tr, image, dev, exposure):
    from deepestscatter_amd import _lib
    a = tr.tonemap_buffer(dev.data_ptr(), exposure)
    tr.upload(_lib.CT_BUF_MEAN, image)
    b = tr.tonemap(exposure)
    tr.tonemap_async(exposure)
    tr.synchronize()
    c = tr.download(_lib.CT_BUF_SCREEN)
    return a, b, c


@gpu
@pytest.mark.parametrize("case", TONEMAP_CASES, ids=_case_id)
def test_tonemap_buffer(case):
    w, h, family, exposure = case
    image = make_image(w, h, family, exposure)
    tr = handle(w, h)
    dev = to_device(image)
    (screen, avg), (screen_b, avg_b), screen_c = tonemap_three_ways(tr, image, dev, exposure)
    ref_screen, ref_avg = O.reinhard(image, exposure)
    assert same_values(np.float32(avg), np.float32(ref_avg)), (avg, ref_avg)
    assert np.array_equal(screen, ref_screen), f"{int((screen != ref_screen).sum())} bytes differ from the oracle"
    check_tonemap_against_float64(screen, avg, image, exposure)
    assert np.array_equal(screen_b, screen) and same_values(np.float32(avg_b), np.float32(avg))
    assert np.array_equal(screen_c, screen)


@gpu
def test_tonemap_repeats_and_interleaves():
    """The grid barrier's counter runs on from launch to launch, one per handle: 50 launches through the three entry
    points, three handles of different sizes (and block counts) taking turns."""
    from deepestscatter_amd import _lib
    sizes = [(37, 21, "uniform", 0.4), (64, 1030, "lognormal", 3.0), (1028, 8, "render_like", 0.05)]
    trs, devs, firsts = [], [], []
    for w, h, family, exposure in sizes:
        image = make_image(w, h, family, exposure)
        tr = handle(w, h)
        tr.upload(_lib.CT_BUF_MEAN, image)
        trs.append(tr)
        devs.append(to_device(image))
        ref_screen, ref_avg = O.reinhard(image, exposure)
        firsts.append((ref_screen, np.float32(ref_avg)))
    for launch in range(50):
        i = (launch * 2 + launch // 7) % 3
        tr, exposure, (want_screen, want_avg) = trs[i], sizes[i][3], firsts[i]
        way = (launch + launch // 3) % 3
        if way == 0:
            screen, avg = tr.tonemap_buffer(devs[i].data_ptr(), exposure)
        elif way == 1:
            screen, avg = tr.tonemap(exposure)
        else:
            tr.tonemap_async(exposure)
            tr.synchronize()
            screen, avg = tr.download(_lib.CT_BUF_SCREEN), want_avg
        assert np.array_equal(screen, want_screen) and np.float32(avg) == want_avg, (launch, i, way)


@gpu
def test_widest_frame():
    """12288 pixels: the widest frame ct_create accepts (include/cloudtrace.h).  The tonemap kernel keeps a row of column
    sums in dynamic LDS beside 16 KiB + 4 B of its own, 65540 bytes in all at this width."""
    import deepestscatter_amd as ds
    from deepestscatter_amd import _lib
    for w, h, family, exposure in WIDEST_CASES:
        image = make_image(w, h, family, exposure)
        tr = handle(w, h)
        (screen, avg), (screen_b, avg_b), screen_c = tonemap_three_ways(tr, image, to_device(image), exposure)
        ref_screen, ref_avg = O.reinhard(image, exposure)
        assert np.float32(avg) == np.float32(ref_avg) and np.array_equal(screen, ref_screen)
        check_tonemap_against_float64(screen, avg, image, exposure)
        assert np.array_equal(screen_b, screen) and np.float32(avg_b) == np.float32(avg) and np.array_equal(screen_c, screen)
    for w, h in ((12289, 1), (8, 4097), (0, 8)):
        with pytest.raises(_lib.CloudTraceError) as e:
            ds.CloudTracer(sphere_volume(8), width=w, height=h)
        assert e.value.code == _lib.CT_E_INVAL


def converged_buffers(tr, mean, m2, n):
    a, b = to_device(mean), to_device(m2)                                # (both alive until the call has returned)
    return tr.is_converged_buffers(a.data_ptr(), b.data_ptr(), n)


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_converged_buffers(shape):
    w, h = shape
    tr = handle(w, h)
    for n in CONVERGED_COUNTS:
        mean, m2 = conv_inputs(w, h, n)
        got = converged_buffers(tr, mean, m2, n)
        assert got == O.is_converged(mean, m2, n), n
        if n >= 100:
            lo, hi = converged64(mean, m2, n)
            assert lo <= got[1] <= hi and got[0] == (got[1] < 500)
        mean, m2 = threshold_inputs(w, h, n)
        got = converged_buffers(tr, mean, m2, n)
        assert got == O.is_converged(mean, m2, n), ("per-pixel thresholds", n)
    nans = to_device(np.full((h, w, 4), np.nan, np.float32))
    for n in (0, 1, 99):
        assert tr.is_converged_buffers(nans.data_ptr(), nans.data_ptr(), n) == (False, w * h)
    assert tr.is_converged_buffers(nans.data_ptr(), nans.data_ptr(), 100) == (w * h < 500, w * h)


@gpu
@pytest.mark.parametrize("shape", [(64, 1030), (257, 2049)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_converged_buffers_decide_at_500(shape):
    """Camera.cpp:267: converged when FEWER than 500 pixels lie outside the interval."""
    w, h = shape
    tr = handle(w, h)
    for n in (100, 1000):
        for k in (499, 500, 501):
            mean, m2 = exact_bad_inputs(w, h, n, k)
            assert converged64(mean, m2, n) == (k, k)
            assert converged_buffers(tr, mean, m2, n) == (k < 500, k)
    # NaN and negative M2 count as outside the interval: that is what the !(a || b) form of the rule is for
    mean, m2 = np.ones((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    m2.reshape(-1, 4)[-300:, 0] = np.nan
    m2.reshape(-1, 4)[:150, 0] = -1.0
    mean.reshape(-1, 4)[1000:1050, 0] = np.nan
    m2.reshape(-1, 4)[1000:1050, 0] = 1e9              # (with M2 = 0 the absolute interval is 0 and passes whatever the mean)
    assert converged_buffers(tr, mean, m2, 100) == (False, 500)
    m2.reshape(-1, 4)[0, 0] = 0.0
    assert converged_buffers(tr, mean, m2, 100) == (True, 499)


def freeze_frames(w, h, noisy):
    """Two frames to alternate: 1 everywhere, but 0 and 2 in turn on `noisy` pixels (the last of the frame among them)."""
    P = w * h
    rng = np.random.default_rng(_seed("freeze", w, h, noisy))
    frames = np.ones((2, P, 4), np.float32)
    if noisy:
        at = np.append(rng.choice(P - 1, noisy - 1, replace=False), P - 1)
        frames[0, at, 0] = 0.0
        frames[1, at, 0] = 2.0
    return frames.reshape(2, h, w, 4)


@gpu
@pytest.mark.parametrize("min_subframes", [100, 7])
@pytest.mark.parametrize("cadence", [1, 3, 10])
def test_freeze_through_ct_accumulate(cadence, min_subframes):
    """ct_set_stop_when_converged on a handle that is fed through ct_accumulate: the test runs behind every cadence-th id
    from min_subframes on, freezes the image when fewer than 500 pixels lie outside the interval, and a frozen image
    ignores what is accumulated afterwards."""
    from deepestscatter_amd import _lib
    w, h = 37, 21
    tr = handle(w, h)
    first_tested = -(-min_subframes // cadence) * cadence
    for noisy in (0, 500, 499):
        tr.set_stop_when_converged(0, 0)
        tr.reset()
        tr.set_stop_when_converged(cadence, min_subframes)
        frames = freeze_frames(w, h, noisy)
        dev = to_device(frames)
        mean, m2 = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
        last = first_tested + 2 * cadence
        frozen = None
        for sid in range(1, last + 1):
            tr.accumulate(sid, dev[sid % 2].data_ptr())
            if frozen is None:
                O.accumulate(frames[sid % 2], mean, m2, sid)
            at = tr.converged_at()
            if sid < first_tested:
                assert at == (0, 0, 0), (sid, at)
            elif noisy == 500:
                assert at == (0, sid - sid % cadence, 500), (sid, at)
            else:
                assert at == (first_tested, first_tested, noisy), (sid, at)
                frozen = first_tested
        assert converged64(mean, m2, frozen or last) == (noisy, noisy)
        assert same_values(tr.mean(), mean) and same_values(tr.m2(), m2)
        if noisy == 500:
            continue
        loud = to_device(np.full((h, w, 4), 1e6, np.float32))
        for sid in range(last + 1, last + 6):
            tr.accumulate(sid, loud.data_ptr())
            assert tr.converged_at() == (first_tested, first_tested, noisy)
        assert same_values(tr.mean(), mean) and same_values(tr.m2(), m2)
        if first_tested >= 100:
            assert tr.is_converged() == O.is_converged(mean, m2, first_tested)
        tr.reset()                                                       # thaws it
        assert tr.converged_at() == (0, 0, 0)
        tr.accumulate(1, loud.data_ptr())
        assert (tr.mean() == np.float32(1e6)).all() and (tr.m2() == 0).all()
    tr.set_stop_when_converged(0, 0)
    tr.reset()


def device_accumulate(tr, frames, first):
    dev = to_device(frames)
    for i in range(frames.shape[0]):
        tr.accumulate(first + i, dev[i].data_ptr())
    return tr.mean(), tr.m2()


@gpu
@pytest.mark.parametrize("run", ACCUMULATE_RUNS, ids=lambda r: f"{r[0]}x{r[1]}-{r[2]}-{r[3]}")
def test_accumulate_caller_frames(run):
    w, h, family, count = run
    frames, kind = caller_frames(w, h, family, 1, count)
    tr = handle(w, h)
    tr.reset()
    mean, m2 = device_accumulate(tr, frames, 1)
    ref_mean, ref_m2 = oracle_accumulate(frames, 1)
    assert same_values(mean, ref_mean) and same_values(m2, ref_m2)
    check_caller_run(mean, m2, frames, kind)
    assert tr.subframes == count
    tr.reset()


@gpu
def test_accumulate_high_ids():
    """Ids round 2^24, where (float)subframe_id stops being exact, on a state set with ct_upload + ct_set_subframes."""
    from deepestscatter_amd import _lib
    w, h = 33, 9
    mean0, m2_0, frames, first = high_id_run(w, h)
    tr = handle(w, h)
    tr.upload(_lib.CT_BUF_MEAN, mean0)
    tr.upload(_lib.CT_BUF_M2, m2_0)
    tr.set_subframes(first - 1)
    mean, m2 = device_accumulate(tr, frames, first)
    ref_mean, ref_m2 = oracle_accumulate(frames, first, mean0, m2_0)
    assert same_values(mean, ref_mean) and same_values(m2, ref_m2)
    check_high_id_run(mean, m2, mean0, m2_0, frames, first)
    tr.reset()


@gpu
@pytest.mark.parametrize("shape", [(33, 9), (37, 21)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_accumulate_sharded_handles_leave_foreign_tiles_zero(shape):
    """A shard accumulates its own 8x8 tiles only, whatever the caller's frame holds elsewhere: the sum over the shards is
    the unsharded image bit for bit, which is what the RCCL sum-merge rests on."""
    import deepestscatter_amd as ds
    w, h = shape
    frames = np.random.default_rng(_seed("shards", w, h)).random((5, h, w, 4), dtype=np.float32) + np.float32(0.5)
    whole = handle(w, h)
    whole.reset()
    want_mean, want_m2 = device_accumulate(whole, frames, 1)
    ref_mean, ref_m2 = oracle_accumulate(frames, 1)
    assert same_values(want_mean, ref_mean) and same_values(want_m2, ref_m2)
    for count in (2, 3):
        sum_mean, sum_m2 = np.zeros_like(want_mean), np.zeros_like(want_m2)
        for index in range(count):
            tr = handle(w, h, index, count)
            tr.reset()
            mean, m2 = device_accumulate(tr, frames, 1)
            own = ds.shard_mask(w, h, index, count)
            assert own.any() and not own.all()
            assert (mean[~own] == 0).all() and (m2[~own] == 0).all(), "a foreign tile was written"
            assert np.array_equal(mean[own], want_mean[own]) and np.array_equal(m2[own], want_m2[own])
            sum_mean += mean
            sum_m2 += m2
        assert np.array_equal(sum_mean, want_mean) and np.array_equal(sum_m2, want_m2)
    whole.reset()


@gpu
def test_rendered_frames_fed_back():
    """ct_render_subframe into caller-owned buffers, those buffers through a fresh handle's ct_accumulate: the dense
    accumulate kernel and the list kernel of ct_render_accumulate make the same image of the same samples, misses included."""
    import torch
    import deepestscatter_amd as ds
    tex = sphere_volume(24, seed=5)
    w, h, spp = 40, 24, 6
    kw = dict(width=w, height=h, cloud_size_m=3000.0, max_depth=200)
    a, b, c = (ds.CloudTracer(tex, **kw) for _ in range(3))
    bufs = torch.zeros((spp, h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for i in range(spp):
        a.render_subframe(i + 1, bufs[i].data_ptr())
    for i in range(spp):
        b.accumulate(i + 1, bufs[i].data_ptr())
    c.render_accumulate(1, spp)
    frames = from_device(bufs)
    assert (frames[..., 3] == 1).all() and (frames[..., :3] > 0).any() and (frames[..., :3].sum(axis=(0, 3)) == 0).any()
    assert same_values(b.mean(), c.mean()) and same_values(b.m2(), c.m2())
    ref_mean, ref_m2 = oracle_accumulate(frames, 1)
    assert same_values(b.mean(), ref_mean) and same_values(b.m2(), ref_m2)
    for tr in (a, b, c):
        tr.close()
