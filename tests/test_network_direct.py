"""CT_NET_ADD_SINGLE_SCATTER: ct_network_render_* with the sun's single-scatter term added (include/cloudtrace.h, "the
scattering network as a renderer").

Per pixel and subframe  mode 0 = mode 2 + (multiple scatter from the first-scatter point): the network predicts the second
summand, the flag adds the first, D -- exactly what a CT_MODE_SUN_SINGLE_SCATTER handle renders for that pixel and subframe.
So every reference here is made of things that already exist: ct_render_subframe of a mode-2 MARCH handle on the same cloud,
the flagless network frame, the CPU oracle's mode-2 frame, and the loop network_render_subframe + accumulate.

Everything is compared with np.array_equal on the float values: bit for bit, except that +0 and -0 compare equal (0 + (-0) is
+0, so the sign of a zero direct term need not survive the sum).  No tolerance of this file's own.

Scene: make_procedural_cloud(64), 24 x 16, the default pose, SCALE = (0.5, 2.0, 3.0); the seeded (200, 1, 3) and (32, 1, 1)
weights of tests/test_network_render.py (helpers copied, not imported).  Subframe 3 has 79 records in rows 4 .. 12; under the
default light 47 of them have a non-zero single-scatter value and the rest lie in full shadow, under LIGHT2 25 are lit: the
CPU test asserts these numbers on the oracle, so the GPU tests are known to see lit records, records with a direct term of
exactly 0, and pixels without a record."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _oracle as O
import deepestscatter_amd as ds
from deepestscatter_amd import _lib
from deepestscatter_amd import network as N

ROOT = Path(__file__).resolve().parents[1]
W, H, SID = 24, 16, 3
SCALE = (0.5, 2.0, 3.0)
LIGHT2 = (0.586, -0.766, -0.271)
FLAGSHIP, SMALL = N.NetworkShape(200, 1, 3), N.NetworkShape(32, 1, 1)
FLAG = 0x100
MODE2 = _lib.CT_MODE_SUN_SINGLE_SCATTER


# ------------------------------------------------------------------------------ helpers of tests/test_network_render.py
def seeded_weights(shape: N.NetworkShape, seed: int) -> np.ndarray:
    """Every matrix and bias uniform in +-1/sqrt(fan_in), in the flat array's order."""
    rng = np.random.default_rng(seed)
    dims = []
    for k in range(N.BLOCKS):
        dims += [(shape.width, shape.fan_in(k)), (shape.width, shape.width)]
    dims += [(shape.width, shape.width)] * (shape.head_layers - 1) + [(1, shape.width)]
    parts = []
    for rows, cols in dims:
        bound = 1.0 / np.sqrt(cols)
        parts.append(rng.uniform(-bound, bound, rows * cols).astype(np.float32))
        parts.append(rng.uniform(-bound, bound, rows).astype(np.float32))
    flat = np.concatenate(parts)
    assert flat.size == shape.weight_count()
    return flat


def weights(shape, negated=False):
    """The seeded weights of a case, with outputs of both signs on this scene's records (seed 1 with the output bias raised by
    0.056 for (200, 1, 3), seed 13 for (32, 1, 1)); negated: the last layer (v, d) times -1, so out becomes -out exactly."""
    w = seeded_weights(shape, {FLAGSHIP: 1, SMALL: 13}[shape])
    if shape == FLAGSHIP:
        w[-1] += np.float32(0.056)
    if negated:
        w[-(shape.width + 1):] *= np.float32(-1)
    return w


def dark_weights(shape=SMALL):
    """Every weight 0, the output bias d = -1: out = -1 for every record, so g = 0 under both transforms."""
    w = np.zeros(shape.weight_count(), np.float32)
    w[-1] = -1
    return w


def cloud():
    return ds.make_procedural_cloud(64)


# ------------------------------------------------------------------------------ the restatement of tests/test_descriptor_frame.py
F = np.float32


def _norm(v):
    """optix::normalize: v * (1 / sqrtf(dot(v, v)))"""
    inv = F(1) / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return (v[0] * inv, v[1] * inv, v[2] * inv)


def record_pixels(orc, subframe_id):
    """-> the pixel indices (y * width + x, row-major) that have a first-scatter record, for the oracle scene `orc`: the primary
    ray, the box test and the first flight restated in numpy float32 with the oracle's texture unit and expf / logf."""
    L = O.lib(False)
    u = orc.derived_uniforms()
    bbox = (F(u[0]), F(u[1]), F(u[2]))
    dm, step = F(u[6]), F(u[15])
    s = orc.scene
    width, height = int(s.width), int(s.height)
    eye = tuple(F(v) for v in s.eye)
    U, V, Wv = (tuple(F(v) for v in a) for a in (s.U, s.V, s.W))
    nz, ny, nx = orc.density.shape
    dims = (C.c_uint32 * 3)(nx, ny, nz)
    texels = orc.density.ctypes.data_as(C.c_void_p)
    p3 = (C.c_float * 3)()
    lo, hi = F(-0.01), tuple(b + F(0.01) for b in bbox)
    half = tuple(b * F(0.5) for b in bbox)

    def in_box(p):
        return bool(p[0] >= lo and p[1] >= lo and p[2] >= lo and p[0] <= hi[0] and p[1] <= hi[1] and p[2] <= hi[2])

    def tex(p):
        p3[0], p3[1], p3[2] = float(p[0]), float(p[1]), float(p[2])
        return F(L.orc_tex3d(texels, dims, p3))

    def intersect_box(o, d):
        bmin = tuple(-b / F(2) for b in bbox)
        bmax = tuple(b / F(2) for b in bbox)
        with np.errstate(divide="ignore", invalid="ignore"):
            t0 = tuple((bmin[i] - o[i]) / d[i] for i in range(3))
            t1 = tuple((bmax[i] - o[i]) / d[i] for i in range(3))
        tmin = np.fmax(np.fmax(np.fmin(t0[0], t1[0]), np.fmin(t0[1], t1[1])), np.fmin(t0[2], t1[2]))
        tmax = np.fmin(np.fmin(np.fmax(t0[0], t1[0]), np.fmax(t0[1], t1[1])), np.fmax(t0[2], t1[2]))
        if tmin <= tmax:
            if tmin > F(0) and tmin < F(1e27):
                return F(tmin)
            return F(0.000001)
        return None

    def flight(xi, pos, d):
        sx, sy, sz = d[0] * step, d[1] * step, d[2] * step
        T = F(1)
        while in_box(pos):
            pos = (pos[0] + sx, pos[1] + sy, pos[2] + sz)
            density = tex(pos) * dm
            extinction = density * step
            T = T * F(L.orc_expf(-extinction))
            if xi > T:
                lg = F(L.orc_logf(xi / T))
                inv = F(1) / density
                return True, (pos[0] - d[0] * lg * inv, pos[1] - d[1] * lg * inv, pos[2] - d[2] * lg * inv)
        return False, pos

    pix = []
    for y in range(height):
        for x in range(width):
            dx = F(x) / F(width) * F(2) - F(1)
            dy = F(y) / F(height) * F(2) - F(1)
            d1 = _norm(tuple(U[i] * dx + V[i] * dy + Wv[i] for i in range(3)))
            t_hit = intersect_box(eye, d1)
            if t_hit is None:
                continue
            pos = tuple(eye[i] + d1[i] * t_hit + half[i] for i in range(3))
            d2 = _norm(d1)
            seed = C.c_uint32(L.orc_tea4((x * 4096 + y) & 0xFFFFFFFF, subframe_id))
            xi = F(L.orc_rnd(C.byref(seed)))
            scattered, sp = flight(xi, pos, d2)
            if scattered and in_box(sp):
                pix.append(y * width + x)
    return np.array(pix, np.int64)


# ------------------------------------------------------------------------------ oracle frames, computed once
_ORACLE = {}


def oracle_single(light=None, fast=False):
    """The mode-2 oracle of the scene under a light (None: the default one)."""
    key = ("orc", light, fast)
    if key not in _ORACLE:
        extra = {"light_direction": light} if light else {}
        _ORACLE[key] = O.Oracle(cloud(), W, H, mode=2, fast=fast, **extra)
    return _ORACLE[key]


def oracle_single_frame(sid, light=None, fast=False):
    key = ("frame", sid, light, fast)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_single(light, fast).render_subframe(sid)
    return _ORACLE[key]


# ---------------------------------------------------------------------------------------------------- CPU
def test_constant_parameters_and_the_null_handle(product_lib):
    assert _lib.CT_NET_ADD_SINGLE_SCATTER == FLAG
    header = (ROOT / "include" / "cloudtrace.h").read_text()
    assert int(re.search(r"#define CT_NET_ADD_SINGLE_SCATTER (0x[0-9a-fA-F]+)", header).group(1), 16) == FLAG
    assert C.sizeof(_lib.CtNetworkRender) == 24
    params = ds.CloudTracer._network_render_params
    p = params("expm1", SCALE, 48, direct=True)
    assert p.transform == 0x101 and p.band_pixels == 48 and tuple(p.rgb_scale) == SCALE and p.abi_version == _lib.CT_ABI_VERSION
    assert params("linear", SCALE, 0, direct=True).transform == FLAG
    assert params("expm1", SCALE, 48).transform == _lib.CT_NET_OUT_EXPM1 and params("linear", SCALE, 0).transform == _lib.CT_NET_OUT_LINEAR
    assert params("expm1", SCALE, 48, direct=False).transform == 1
    assert params(0x101, SCALE, 0).transform == 0x101 and params(-1, SCALE, 0).transform == -1     # an integer passes through
    for transform in (FLAG, FLAG | 1):
        q = _lib.CtNetworkRender(_lib.CT_ABI_VERSION, transform, (C.c_float * 3)(1, 1, 1), 0)
        assert product_lib.ct_network_render_subframe(None, None, C.byref(q), 1, None) == _lib.CT_E_INVAL
        assert product_lib.ct_network_render_accumulate(None, None, C.byref(q), 1, 1) == _lib.CT_E_INVAL


def test_cli_names_the_option():
    from deepestscatter_amd import build
    r = subprocess.run([str(build.build_cli())], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "[--net-direct]" in r.stderr
    src = (ROOT / "deepestscatter_amd" / "host" / "main.cpp").read_text()
    assert src.count("--net-direct") >= 3                          # header comment, usage line and the option itself


def test_total_radiance_is_single_scatter_plus_the_rest_on_the_oracle():
    single = oracle_single()
    total = O.Oracle(cloud(), W, H, mode=0, inscatter=single.inscatter)          # one shadow volume for both
    greater, records = [], {}
    for sid in (1, 2, 3):
        f0, f2 = total.render_subframe(sid), oracle_single_frame(sid)
        assert np.all(f0[..., :3] >= f2[..., :3]), sid
        greater.append(int((f0[..., :3] > f2[..., :3]).any(axis=2).sum()))
        records[sid] = record_pixels(single, sid)
        none = np.ones(W * H, bool)
        none[records[sid]] = False
        assert not f2.reshape(-1, 4)[none, :3].any(), sid                        # no record, no single scatter
    assert greater == [48, 53, 50]                                               # strictly greater somewhere, in every subframe
    pix = records[SID]
    rows = np.bincount(pix // W, minlength=H)
    assert len(pix) == 79 and rows[:4].sum() == 0 and rows[13:].sum() == 0 and np.all(rows[4:13] > 0)
    lit = oracle_single_frame(SID).reshape(-1, 4)[pix, :3].any(axis=1)
    assert int(lit.sum()) == 47
    lit2 = oracle_single_frame(SID, LIGHT2).reshape(-1, 4)[pix, :3].any(axis=1)
    assert int(lit2.sum()) == 25
    assert not np.array_equal(oracle_single_frame(SID, LIGHT2), oracle_single_frame(SID))


def test_render_values_with_a_direct_term():
    rng = np.random.default_rng(5)
    out = rng.uniform(-1, 1, 40).astype(np.float32)
    direct = rng.uniform(0, 1, (40, 3)).astype(np.float32)
    direct[::4] = 0
    plain = N.render_values(out, "linear", SCALE)
    got = N.render_values(out, "linear", SCALE, direct=direct)
    assert got.dtype == np.float32 and got.shape == (40, 4) and np.all(got[:, 3] == 1)
    assert np.array_equal(got[:, :3], plain[:, :3] + direct) and (plain[:, :3] + direct).dtype == np.float32
    assert not np.array_equal(got, plain)
    assert np.array_equal(N.render_values(out, "linear", SCALE, direct=None), plain)
    assert np.array_equal(N.render_values(out, "linear", SCALE, direct=direct.astype(np.float64).tolist()), got)   # cast to float32 first
    expf = lambda v: float(np.exp(np.float32(v)))
    assert np.array_equal(N.render_values(out, "expm1", SCALE, expf=expf, direct=direct)[:, :3],
                          N.render_values(out, "expm1", SCALE, expf=expf)[:, :3] + direct)


# ---------------------------------------------------------------------------------------------------- GPU
class Pair:
    """A handle for the network (mode 0) and a CT_MODE_SUN_SINGLE_SCATTER MARCH handle on the same cloud: the reference of D."""

    def __init__(self, flags=0, estimator=_lib.CT_EST_MARCH):
        tex = cloud()
        self.net_tracer = ds.CloudTracer(tex, width=W, height=H, flags=flags, estimator=estimator)
        self.single = ds.CloudTracer(tex, width=W, height=H, mode=MODE2, estimator=_lib.CT_EST_MARCH, flags=flags)
        self.nets = {}
        self._single = {}

    def net(self, shape=SMALL, kind="seeded"):
        if (shape, kind) not in self.nets:
            w = dark_weights(shape) if kind == "dark" else weights(shape, kind == "negated")
            self.nets[(shape, kind)] = N.Network(self.net_tracer, w, shape.width, shape.aux, shape.head_layers)
        return self.nets[(shape, kind)]

    def single_frame(self, sid):
        """ct_render_subframe of the mode-2 handle, once per subframe (forget() after a new light)."""
        if sid not in self._single:
            self.single.render_subframe(sid)
            self._single[sid] = self.single.frame()
        return self._single[sid]

    def set_light(self, direction):
        self.net_tracer.set_light(direction)
        self.single.set_light(direction)
        self._single.clear()

    def close(self):
        for n in self.nets.values():
            n.close()
        self.net_tracer.close()
        self.single.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


@pytest.fixture(scope="module")
def pair():
    """The module's pair as it is created: default pose, default light, nothing accumulated on the network's handle.  Tests that
    change a light or accumulate make a Pair of their own."""
    with Pair() as p:
        yield p


def direct_frame(p, net, sid, **kw):
    return p.net_tracer.network_render_subframe(net, sid, direct=True, **kw).cpu().numpy()


def check_dark(p, oracle_fast=False):
    """Subframes 1 .. 5, both transforms: the dark network's direct frame IS the mode-2 handle's frame; subframe 3 also the oracle's."""
    net = p.net(SMALL, "dark")
    for sid in range(1, 6):
        want = p.single_frame(sid)
        for transform in ("linear", "expm1"):
            got = direct_frame(p, net, sid, transform=transform, rgb_scale=SCALE)
            assert np.array_equal(got, want), (sid, transform)
    want = p.single_frame(SID)
    assert np.array_equal(want, oracle_single_frame(SID, fast=oracle_fast))
    assert want[..., :3].any() and np.all(want[..., 3] == 1)
    # without the flag the dark network's frame is dark
    plain = p.net_tracer.network_render_subframe(net, SID, rgb_scale=SCALE).cpu().numpy()
    assert not plain[..., :3].any() and np.all(plain[..., 3] == 1)


@pytest.mark.gpu
def test_a_dark_network_shows_the_single_scatter_image(pair):
    check_dark(pair)
    # lit records, records in full shadow, pixels without a record: all three are in the frame that was compared
    pix = pair.net_tracer.descriptor_frame(SID)[3].cpu().numpy().astype(np.int64)
    lit = pair.single_frame(SID).reshape(-1, 4)[pix, :3].any(axis=1)
    assert len(pix) == 79 and int(lit.sum()) == 47


@pytest.mark.gpu
def test_a_dark_network_with_fixed8_texture_weights():
    with Pair(flags=_lib.CT_FLAG_TEX_FIXED8) as p:
        check_dark(p, oracle_fast="fixed8")


@pytest.mark.gpu
def test_a_dark_network_on_a_delta_handle(pair):
    """The flight and D ignore the handle's estimator: the reference stays the MARCH mode-2 handle."""
    with Pair(estimator=_lib.CT_EST_DELTA) as p:
        check_dark(p)
        assert np.array_equal(p.single_frame(SID), pair.single_frame(SID))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [FLAGSHIP, SMALL], ids=["200-1-3", "32-1-1"])
@pytest.mark.parametrize("transform", ["linear", "expm1"])
def test_the_sum_rule(pair, transform, shape):
    import torch
    tr = pair.net_tracer
    single = pair.single_frame(SID)
    for kind in ("seeded", "negated"):
        net = pair.net(shape, kind)
        plain = tr.network_render_subframe(net, SID, transform=transform, rgb_scale=SCALE).cpu().numpy()
        assert plain[..., :3].any()                                            # the network's summand is there ...
        want = plain.copy()
        want[..., :3] = plain[..., :3].astype(np.float32) + single[..., :3].astype(np.float32)
        assert want.dtype == np.float32 and not np.array_equal(want, plain)    # ... and so is the sun's
        got = direct_frame(pair, net, SID, transform=transform, rgb_scale=SCALE)
        assert np.array_equal(got[..., :3], want[..., :3]), kind
        assert np.all(got[..., 3] == 1)
        assert np.array_equal(tr.download(_lib.CT_BUF_FRAME), got)
        mine = torch.full((H, W, 4), -7.0, dtype=torch.float32, device=torch.device("cuda", tr.params.device))   # a caller's tensor
        assert tr.network_render_subframe(net, SID, transform=transform, rgb_scale=SCALE, out=mine, direct=True) is mine
        assert np.array_equal(mine.cpu().numpy(), want)
        assert np.array_equal(tr.download(_lib.CT_BUF_FRAME), mine.cpu().numpy())


@pytest.mark.gpu
def test_a_new_light(pair):
    with Pair() as p:
        net = p.net(SMALL, "dark")
        old = direct_frame(p, net, SID, rgb_scale=SCALE)
        assert np.array_equal(old, pair.single_frame(SID))                      # the handles of the dark-network test
        p.set_light(LIGHT2)
        lit = direct_frame(p, net, SID, rgb_scale=SCALE)
        assert np.array_equal(lit, p.single_frame(SID))
        assert lit[..., :3].any() and not np.array_equal(lit, old)
        assert np.array_equal(lit, oracle_single_frame(SID, LIGHT2))


def _progressive(tr):
    return tr.mean(), tr.m2(), tr.subframes


@pytest.mark.gpu
@pytest.mark.parametrize("stop", [False, True])
def test_fused_equals_the_loop(stop):
    tex = cloud()
    kw = dict(transform="linear", rgb_scale=SCALE, direct=True)
    with ds.CloudTracer(tex, width=W, height=H) as a, ds.CloudTracer(tex, width=W, height=H) as b:
        na, nb = N.Network(a, weights(FLAGSHIP), 200, 1, 3), N.Network(b, weights(FLAGSHIP), 200, 1, 3)
        try:
            if stop:
                a.set_stop_when_converged(2, 2)
                b.set_stop_when_converged(2, 2)
            a.network_render_accumulate(na, 1, 5, band_pixels=48, **kw)
            for sid in range(1, 6):
                b.network_render_subframe(nb, sid, out=False, **kw)
                b.accumulate(sid)
            sa, sb = _progressive(a), _progressive(b)
            assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1]) and sa[2] == sb[2] == 5
            assert sa[0][..., :3].any() and sa[1][..., :3].any()
            assert np.all(sa[0][..., 3] == 1) and np.all(sa[1][..., 3] == 0)
            assert a.converged_at() == b.converged_at()
            if stop:
                assert a.converged_at()[:2] == (2, 2)          # 384 pixels are fewer than 500: frozen at the first test
            # the flag is in the mean: the flagless render of the same subframes differs
            mean_direct = sa[0]
            a.reset()
            if stop:
                a.set_stop_when_converged(2, 2)
            a.network_render_accumulate(na, 1, 5, band_pixels=48, transform="linear", rgb_scale=SCALE)
            assert not np.array_equal(a.mean(), mean_direct)
        finally:
            na.close()
            nb.close()


@pytest.mark.gpu
def test_the_image_does_not_depend_on_the_bands(pair):
    net = pair.net(SMALL)
    want = direct_frame(pair, net, SID, rgb_scale=SCALE, band_pixels=W * H)
    plain = pair.net_tracer.network_render_subframe(net, SID, rgb_scale=SCALE).cpu().numpy()
    sum_ = plain.copy()
    sum_[..., :3] = plain[..., :3] + pair.single_frame(SID)[..., :3]
    assert np.array_equal(want, sum_)
    pix = pair.net_tracer.descriptor_frame(SID)[3].cpu().numpy()
    per_row = np.bincount(pix // W, minlength=H)
    assert (per_row == 0).any() and (per_row > 0).any()              # one-row bands: some without a record, some with
    for band in (1, 24, 25, 120, 0):
        assert np.array_equal(direct_frame(pair, net, SID, rgb_scale=SCALE, band_pixels=band), want), band


def _state(tr):
    return tr.mean(), tr.m2(), tr.subframes, tr.counters(), tr.fetch_counters()


@pytest.mark.gpu
@pytest.mark.parametrize("ahead", [False, True])
def test_render_subframe_with_the_flag_has_no_side_effects_on_a_progressive_render(ahead, pair):
    tex = cloud()
    states = []
    for with_call in (True, False):
        with ds.CloudTracer(tex, width=W, height=H) as tr:
            if ahead:
                tr.set_render_ahead(8)
                tr.render_accumulate_async(1, 2)
            else:
                tr.render_accumulate(1, 2)
            if with_call:
                rendered = tr.rendered_subframes()
                with N.Network(tr, dark_weights(SMALL), 32, 1, 1) as net:
                    frame = tr.network_render_subframe(net, SID, rgb_scale=SCALE, band_pixels=48, direct=True)
                    assert np.array_equal(frame.cpu().numpy(), pair.single_frame(SID))
                assert tr.rendered_subframes() == rendered and tr.subframes == 2     # nothing rendered ahead was dropped
            if ahead:
                tr.render_accumulate_async(3, 2)
                tr.synchronize()
            else:
                tr.render_accumulate(3, 2)
            states.append(_state(tr))
    x, y = states
    assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[0].any()
    assert x[2:] == y[2:] and x[2] == 4


def _code(fn, *a, **kw):
    with pytest.raises(_lib.CloudTraceError) as e:
        fn(*a, **kw)
    return e.value.code


@pytest.mark.gpu
def test_unknown_bits_are_refused_and_the_handle_renders_afterwards(pair):
    tr, net = pair.net_tracer, pair.net(SMALL, "dark")
    want = pair.single_frame(SID)
    for bad in (0x200, 0x102, 0x100 | 2, 0x1100):
        assert _code(tr.network_render_subframe, net, SID, transform=bad) == _lib.CT_E_INVAL, hex(bad)
        assert b"transform" in tr.L.ct_last_error(tr.h)
        assert _code(tr.network_render_accumulate, net, 1, 1, transform=bad) == _lib.CT_E_INVAL, hex(bad)
        assert _code(tr.network_render_subframe, net, SID, transform=bad, direct=True) == _lib.CT_E_INVAL, hex(bad)
        assert tr.subframes == 0 and not tr.mean().any()
        assert np.array_equal(direct_frame(pair, net, SID, rgb_scale=SCALE), want), hex(bad)
    # the flag as an integer transform is the keyword
    assert np.array_equal(tr.network_render_subframe(net, SID, transform=0x101, rgb_scale=SCALE).cpu().numpy(), want)


@pytest.mark.gpu
def test_the_direct_scratch_is_kept_and_reused(pair):
    net0 = pair.net(SMALL)
    plain = pair.net_tracer.network_render_subframe(net0, SID, rgb_scale=SCALE).cpu().numpy()
    flagged = plain.copy()
    flagged[..., :3] = plain[..., :3] + pair.single_frame(SID)[..., :3]
    assert not np.array_equal(flagged, plain)
    with ds.CloudTracer(cloud(), width=W, height=H) as tr, N.Network(tr, weights(SMALL), 32, 1, 1) as net:
        # the handle's first call carries the flag; then without it on a larger band (only the flagless temporaries grow); then
        # with it on that band (the direct temporary grows); then warm calls of both kinds on small bands
        for direct, band in ((True, 24), (False, 0), (True, 0), (True, 48), (False, 24), (True, 24)):
            got = tr.network_render_subframe(net, SID, rgb_scale=SCALE, band_pixels=band, direct=direct).cpu().numpy()
            assert np.array_equal(got, flagged if direct else plain), (direct, band)
            times = tr.network_render_time()
            assert all(np.isfinite(t) and t >= 0 for t in times) and times[0] > 0


@pytest.mark.gpu
def test_cli_renders_with_the_network_and_the_direct_term(tmp_path):
    """cloudtrace --network --net-direct: the written images are Python's mean after network_render_accumulate(1, 4, direct=True)
    under the same lights, for both of the job's suns."""
    from deepestscatter_amd import build
    cli = build.build_cli()
    N.save_weights(tmp_path / "w.bin", weights(FLAGSHIP), FLAGSHIP)
    r = subprocess.run([str(cli), "procedural:64", "--network", str(tmp_path / "w.bin"), "--net-direct", "--size", f"{W}x{H}", "--spp", "4",
                        "--format", "pfm", "--out", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "rendering subframe 4" in r.stdout
    with ds.CloudTracer(cloud(), width=W, height=H, light_direction=ds.LIGHT_DIRECTIONS["Side"]) as tr:
        with N.Network(tr, weights(FLAGSHIP), 200, 1, 3) as net:
            images, flagless = {}, {}
            for light in ("Side", "Back"):
                tr.set_light(ds.LIGHT_DIRECTIONS[light])
                tr.reset()
                tr.network_render_accumulate(net, 1, 4, direct=True)
                images[light] = tr.mean()[..., :3]
                tr.reset()
                tr.network_render_accumulate(net, 1, 4)
                flagless[light] = tr.mean()[..., :3]
    assert not np.array_equal(images["Side"], images["Back"])
    for light, want in images.items():
        raw = (tmp_path / f"procedural_64.{light}.PT.pfm").read_bytes()
        header_end = 0
        for _ in range(3):
            header_end = raw.index(b"\n", header_end) + 1
        assert raw[:header_end].split() == [b"PF", str(W).encode(), str(H).encode(), b"-1.0"]
        img = np.frombuffer(raw[header_end:], "<f4").reshape(H, W, 3)
        assert want.any() and np.array_equal(img, want), light
        assert not np.array_equal(want, flagless[light]), light            # the option is in the picture
