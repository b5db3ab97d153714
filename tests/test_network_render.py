"""ct_network_render_subframe / ct_network_render_accumulate: the scattering network as a progressive renderer
(include/cloudtrace.h, "the scattering network as a renderer").

Everything is compared BIT FOR BIT: the reference of a frame is built from entry points that already exist --
descriptor_frame, the device's own aux (network_aux, itself held to its numpy restatement within 2 ulp), Network.eval,
network.render_values (numpy; "expm1" through the oracle's orc_expf) and a scatter by the pixel list -- and the reference of
the fused accumulation is the loop network_render_subframe + accumulate.  No tolerance of this file's own.

Scene: the fixtures of tests/test_network.py -- make_procedural_cloud(64), 24 x 16, the default pose -- whose subframe 3 has
79 records in rows 4 .. 12 and none in rows 0 .. 3 and 13 .. 15 (the CPU test below restates that with the restatement of
tests/test_descriptor_frame.py, so one-row bands take both paths: with records and without).  Weights: the seeded (200, 1, 3)
and (32, 1, 1) cases, chosen so that the outputs have both signs (see `weights`); every frame test runs the weights as they
are and with the last layer (v, d) negated, which negates every output exactly.

ct_create gives every handle the default pose, so "no camera pose" (CT_E_STATE) cannot be provoked through the ABI: the
order-error test covers the statuses a live handle can produce."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

import _oracle as O
import deepestscatter_amd as ds
from deepestscatter_amd import _lib
from deepestscatter_amd import network as N

W, H, SID = 24, 16, 3
SCALE = (0.5, 2.0, 3.0)
LIGHT2 = (0.586, -0.766, -0.271)
FLAGSHIP, SMALL = N.NetworkShape(200, 1, 3), N.NetworkShape(32, 1, 1)


def seeded_weights(shape: N.NetworkShape, seed: int) -> np.ndarray:
    """Every matrix and bias uniform in +-1/sqrt(fan_in), in the flat array's order (as tests/test_network.py)."""
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
    """The seeded weights of a case, chosen so that the outputs on this scene's records have BOTH signs (a frame test with
    outputs of one sign is blind in one of its two runs).  A random network is nearly constant over the records: of the seeds
    1 .. 399 none gives the (200, 1, 3) network outputs of both signs (seed 1, the case of tests/test_network.py: -0.063 ..
    -0.046 on subframe 3), so that case keeps seed 1 and its output bias d is raised by 0.056, which leaves 15 to 22 of the
    78 to 81 records of subframes 1 .. 5 positive; the (32, 1, 1) case uses seed 13, the first whose outputs are mixed (16 of
    79 positive on subframe 3).  Both were chosen with reference_forward on the restated records, on the CPU."""
    w = seeded_weights(shape, {FLAGSHIP: 1, SMALL: 13}[shape])
    if shape == FLAGSHIP:
        w[-1] += np.float32(0.056)
    if negated:
        w[-(shape.width + 1):] *= np.float32(-1)       # the last layer (v, d): out becomes -out, exactly
    return w


def cloud():
    return ds.make_procedural_cloud(64)


# ---------------------------------------------------------------------------------------------------- CPU
def test_symbols_resolve_and_answer_null_arguments(product_lib):
    names = ["ct_network_render_subframe", "ct_network_render_accumulate", "ct_debug_network_aux", "ct_debug_network_render_time"]
    for name in names:
        assert hasattr(product_lib, name) and name in _lib.EXPORTS
    p = _lib.CtNetworkRender(_lib.CT_ABI_VERSION, _lib.CT_NET_OUT_LINEAR, (C.c_float * 3)(1, 1, 1), 0)
    assert product_lib.ct_network_render_subframe(None, None, C.byref(p), 1, None) == _lib.CT_E_INVAL
    assert product_lib.ct_network_render_subframe(None, None, None, 1, None) == _lib.CT_E_INVAL
    assert product_lib.ct_network_render_accumulate(None, None, C.byref(p), 1, 1) == _lib.CT_E_INVAL
    assert product_lib.ct_network_render_accumulate(None, None, None, 1, 1) == _lib.CT_E_INVAL
    assert product_lib.ct_debug_network_aux(None, None, 0, None) == _lib.CT_E_INVAL
    assert product_lib.ct_debug_network_render_time(None, None) == _lib.CT_E_INVAL
    assert C.sizeof(_lib.CtNetworkRender) == 24


def test_weight_file_round_trip(tmp_path):
    import torch
    for shape in (SMALL, N.NetworkShape(16, 0, 4)):
        w = seeded_weights(shape, 4)
        path = tmp_path / f"w{shape.width}.bin"
        N.save_weights(path, w, shape)
        raw = path.read_bytes()
        assert len(raw) == 32 + 4 * w.size and raw[:4] == b"CTNW"
        assert struct.unpack("<IIIIIQ", raw[4:32]) == (1, 10, shape.width, shape.aux, shape.head_layers, w.size)
        got, got_shape = N.load_weights(path)
        assert got_shape == shape and got.dtype == np.float32 and got.tobytes() == w.tobytes()
    torch.manual_seed(3)
    module = N.ScatterNet(16, 1, 2)
    N.save_weights(tmp_path / "m.bin", module)
    got, got_shape = N.load_weights(tmp_path / "m.bin")
    assert got_shape == module.shape and got.tobytes() == N.pack_weights(module).tobytes()
    with pytest.raises(ValueError):
        N.save_weights(tmp_path / "x.bin", seeded_weights(SMALL, 4)[:-1], SMALL)


def malformed_files(tmp_path):
    """-> {case: path}: a wrong magic, a wrong version, a count that does not match the shapes, a short file."""
    good = tmp_path / "good.bin"
    N.save_weights(good, seeded_weights(SMALL, 4), SMALL)
    raw = good.read_bytes()
    cases = {
        "magic": b"CTNX" + raw[4:],
        "version": raw[:4] + struct.pack("<I", 2) + raw[8:],
        "count": raw[:24] + struct.pack("<Q", SMALL.weight_count() + 1) + raw[32:] + b"\0\0\0\0",
        "short": raw[:-4],
        "header": raw[:20],
    }
    out = {}
    for name, data in cases.items():
        out[name] = tmp_path / f"{name}.bin"
        out[name].write_bytes(data)
    return out


def test_malformed_weight_files_raise_and_stop_the_cli_before_any_device(tmp_path, product_lib):
    from deepestscatter_amd import build
    cli = build.build_cli()
    for name, path in malformed_files(tmp_path).items():
        with pytest.raises(ValueError):
            N.load_weights(path)
        r = subprocess.run([str(cli), "procedural:16", "--network", str(path), "--size", "24x16", "--spp", "1", "--out", str(tmp_path)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode != 0, name
        assert path.name in r.stdout and "Loading volume" not in r.stdout, (name, r.stdout)      # a message, and no scene was set up
        assert not list(tmp_path.glob("*.exr"))
    # a network with another number of aux inputs is refused there too
    N.save_weights(tmp_path / "aux0.bin", seeded_weights(N.NetworkShape(16, 0, 1), 4), N.NetworkShape(16, 0, 1))
    r = subprocess.run([str(cli), "procedural:16", "--network", str(tmp_path / "aux0.bin"), "--out", str(tmp_path)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "aux" in r.stdout and "Loading volume" not in r.stdout


def test_render_values(oracle_lib):
    x = np.array([np.nan, -np.inf, -3.5, -0.0, 0.0, 1e-30, 0.25, 2.0, 87.5, np.inf], np.float32)
    lin = N.render_values(x, "linear", SCALE)
    assert lin.shape == (len(x), 4) and lin.dtype == np.float32 and np.all(lin[:, 3] == 1)
    assert np.all(lin[:6 - 1, :3] == 0)                                     # NaN, negative values and zero give 0
    want = np.where(x > 0, x, np.float32(0)).astype(np.float32)
    assert np.array_equal(lin[:, :3], want[:, None] * np.array(SCALE, np.float32)[None, :])
    assert np.array_equal(N.render_values(x, "linear")[:, 0], want)        # the linear transform is the identity on positive values
    expf = lambda v: oracle_lib.orc_expf(v)
    e = N.render_values(x, "expm1", (1, 1, 1), expf=expf)
    L = np.array([oracle_lib.orc_expf(float(v)) for v in x], np.float32) - np.float32(1)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(e[:, 0], np.where(L > 0, L, np.float32(0)).astype(np.float32))
    assert e[0, 0] == 0 and e[2, 0] == 0 and e[6, 0] > 0 and np.isinf(e[9, 0])
    assert e[6, 0] == np.float32(oracle_lib.orc_expf(0.25)) - np.float32(1)
    with pytest.raises(ValueError):
        N.render_values(x, "expm1")
    with pytest.raises(ValueError):
        N.render_values(x, "log")


def test_the_scene_has_rows_with_and_without_records():
    """The restatement of tests/test_descriptor_frame.py on this file's scene: which rows of subframe 3 hold records."""
    from test_descriptor_frame import restate
    orc = O.Oracle(cloud(), W, H, mode=2, inscatter="none")                 # (the light does not enter the flight)
    pix, _, _ = restate(orc, SID)
    rows = np.bincount(pix // W, minlength=H)
    assert len(pix) == 79 and rows[:4].sum() == 0 and rows[13:].sum() == 0 and np.all(rows[4:13] > 0)


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def tracer():
    with ds.CloudTracer(cloud(), width=W, height=H) as tr:
        yield tr


# Networks made for the module tracer.  The `nets` fixture closes them at its teardown, before the tracer's (a network goes
# before its handle).
_NETS = []


def make_net(tr, shape=FLAGSHIP, negated=False):
    net = N.Network(tr, weights(shape, negated), shape.width, shape.aux, shape.head_layers)
    _NETS.append(net)
    return net


@pytest.fixture(scope="module")
def nets(tracer):
    """The module tracer's networks: (shape, negated) -> Network, created once."""
    made = {}

    def get(shape=FLAGSHIP, negated=False):
        if (shape, negated) not in made:
            made[(shape, negated)] = make_net(tracer, shape, negated)
        return made[(shape, negated)]
    yield get
    for n in _NETS:
        n.close()
    _NETS.clear()


def definition(tr, net, sid, transform="linear", scale=SCALE, expf=None):
    """-> (frame float32 [H, W, 4], out [n], pixels [n]) from descriptor_frame, the device's aux, eval and render_values."""
    import torch
    desc, _, view, pix = tr.descriptor_frame(sid)
    count = int(pix.shape[0])
    aux = tr.network_aux(view)
    out = torch.empty((count,), dtype=torch.float32, device=desc.device)
    torch.cuda.synchronize()
    if count:
        net.eval(desc.data_ptr(), aux.data_ptr(), count, out.data_ptr())
    o, p = out.cpu().numpy(), pix.cpu().numpy().astype(np.int64)
    frame = np.zeros((tr.height * tr.width, 4), np.float32)
    frame[:, 3] = 1
    frame[p] = N.render_values(o, transform, scale, expf=expf)
    return frame.reshape(tr.height, tr.width, 4), o, p


# Reference frames of the MODULE tracer as it is created: default pose, default light, nothing accumulated.  No test may move
# its camera, change its light or accumulate on it -- tests that do any of that make tracers of their own -- or these
# frames would go stale.
_FRAMES = {}


def reference_frame(tracer, nets, sid=SID, shape=FLAGSHIP):
    """The definition's linear frame of the module tracer, computed once per (subframe, shape)."""
    if (sid, shape) not in _FRAMES:
        _FRAMES[(sid, shape)] = definition(tracer, nets(shape), sid)[0]
    return _FRAMES[(sid, shape)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [FLAGSHIP, SMALL], ids=["200-1-3", "32-1-1"])
@pytest.mark.parametrize("transform", ["linear", "expm1"])
def test_frame_equals_its_definition(tracer, nets, oracle_lib, transform, shape):
    import torch
    expf = lambda v: oracle_lib.orc_expf(v)
    positive = []
    for negated in (False, True):
        net = nets(shape, negated)
        want, out, pix = definition(tracer, net, SID, transform, SCALE, expf)
        assert 0 < len(pix) < W * H
        got = tracer.network_render_subframe(net, SID, transform=transform, rgb_scale=SCALE)
        assert got.shape == (H, W, 4) and got.dtype == torch.float32
        assert np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(tracer.download(_lib.CT_BUF_FRAME), want)
        mine = torch.full((H, W, 4), -7.0, dtype=torch.float32, device=got.device)           # a caller's frame_rgba_dev
        assert tracer.network_render_subframe(net, SID, transform=transform, rgb_scale=SCALE, out=mine) is mine
        assert np.array_equal(mine.cpu().numpy(), want)
        g = want.reshape(-1, 4)[pix]
        positive.append(g[:, 1] > 0)
        assert positive[-1].any()                                  # the run is not blind
        assert np.array_equal(g[:, 0] * 4, g[:, 1]) and np.array_equal(g[:, 0] * 6, g[:, 2])   # the channels by their scales
        miss = np.ones(W * H, bool)
        miss[pix] = False
        assert np.all(want.reshape(-1, 4)[miss] == np.array([0, 0, 0, 1], np.float32))
    assert np.all(positive[0] ^ positive[1])                       # together: every record is positive in exactly one run


@pytest.mark.gpu
def test_aux_is_the_dot_product_with_the_light(tracer):
    import torch
    _, _, view, _ = tracer.descriptor_frame(SID)
    got = tracer.network_aux(view).cpu().numpy()
    d, l = view.cpu().numpy(), tracer.light_direction()
    terms = d * l[None, :]
    want = (terms[:, 0] + terms[:, 1]) + terms[:, 2]
    assert want.dtype == np.float32 and len(got) == len(want) > 0
    bound = 2 * np.spacing(np.abs(terms).max(axis=1))
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= bound)
    assert np.abs(got).max() > 0.1
    empty = tracer.network_aux(torch.empty((0, 3), dtype=torch.float32, device=view.device))      # count == 0 is OK
    assert tuple(empty.shape) == (0,)
    assert tracer.L.ct_debug_network_aux(tracer.h, None, 5, None) == _lib.CT_E_INVAL


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [FLAGSHIP, SMALL], ids=["200-1-3", "32-1-1"])
def test_the_image_does_not_depend_on_the_bands(tracer, nets, shape):
    want = reference_frame(tracer, nets, SID, shape)
    rows = (want[..., :3] != 0).any(axis=(1, 2))                    # rows with a positive record
    pix = tracer.descriptor_frame(SID)[3].cpu().numpy()
    per_row = np.bincount(pix // W, minlength=H)
    assert (per_row == 0).any() and (per_row > 0).any() and rows.any()   # one-row bands: some without a record, some with
    for band in (24, 1, 120, 0, 25, 384, 1 << 30):
        got = tracer.network_render_subframe(nets(shape), SID, rgb_scale=SCALE, band_pixels=band)
        assert np.array_equal(got.cpu().numpy(), want), band


@pytest.mark.gpu
def test_a_frame_of_more_than_2_to_the_20_pixels():
    """1040 x 1024 is more than one descriptor_frame rect holds, so band_pixels = 0 makes two bands (1008 rows and 16).  The
    definition is assembled from two rects of 512 rows.  A distant eye and a coarse step keep the records few and the flights
    short, as in tests/test_descriptor_frame.py."""
    import torch
    from conftest import sphere_volume
    w, h = 1040, 1024
    eye = (9.0, -1.5, 0.5)
    U, V, Wv = O.camera_variables(eye, aspect=w / h)
    with ds.CloudTracer(sphere_volume(32, seed=13), width=w, height=h, cloud_size_m=700.0, sample_step=1.0 / 128.0) as tr:
        tr.set_camera(eye, U, V, Wv)
        lit = []
        for negated in (False, True):           # (out and -out: one of the two frames has light whatever this scene's signs are)
            with N.Network(tr, weights(SMALL, negated), 32, 1, 1) as net:
                want = np.zeros((h * w, 4), np.float32)
                want[:, 3] = 1
                total = 0
                for y0 in (0, 512):
                    desc, _, view, pix = tr.descriptor_frame(2, rect=(0, y0, w, y0 + 512), capacity=1 << 16)
                    count = int(pix.shape[0])
                    out = torch.empty((count,), dtype=torch.float32, device=desc.device)
                    aux = tr.network_aux(view)
                    torch.cuda.synchronize()
                    net.eval(desc.data_ptr(), aux.data_ptr(), count, out.data_ptr())
                    want[pix.cpu().numpy().astype(np.int64)] = N.render_values(out.cpu().numpy(), "linear", SCALE)
                    total += count
                assert 500 < total < w * h // 8
                want = want.reshape(h, w, 4)
                for band in (0, 1 << 19):
                    got = tr.network_render_subframe(net, 2, rgb_scale=SCALE, band_pixels=band)
                    assert np.array_equal(got.cpu().numpy(), want), band
                tr.reset()
                tr.network_render_accumulate(net, 1, 1, rgb_scale=SCALE)
                tr.network_render_subframe(net, 1, rgb_scale=SCALE, out=False)
                assert tr.subframes == 1 and np.array_equal(tr.mean(), tr.frame()) and not tr.m2().any()
                lit.append(bool(want[..., :3].any()))
        assert any(lit)


def _progressive(tr):
    return tr.mean(), tr.m2(), tr.subframes


@pytest.mark.gpu
@pytest.mark.parametrize("stop", [False, True])
def test_fused_equals_the_unfused_loop(stop, oracle_lib):
    tex = cloud()
    kw = dict(transform="linear", rgb_scale=SCALE)
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
            assert sa[0].any() and sa[1].any()
            assert np.all(sa[0][..., 3] == 1) and np.all(sa[1][..., 3] == 0)          # alpha: mean 1, M2 0
            assert a.converged_at() == b.converged_at()
            if stop:
                assert a.converged_at()[:2] == (2, 2)          # 384 pixels are fewer than 500: frozen at the first test
            ta, tb = a.tonemap(), b.tonemap()
            assert np.array_equal(ta[0], tb[0]) and ta[1] == tb[1] and ta[0][..., :3].any()
            assert a.is_converged() == b.is_converged()
            # in two calls: (1, 2) then (3, 3)
            a.reset()
            if stop:
                a.set_stop_when_converged(2, 2)
            a.network_render_accumulate(na, 1, 2, **kw)
            assert a.subframes == 2
            a.network_render_accumulate(na, 3, 3, band_pixels=24, **kw)
            sa = _progressive(a)
            assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1]) and sa[2] == 5
            assert a.converged_at() == b.converged_at()
            # the other transform, fused against its own loop
            expm = dict(transform="expm1", rgb_scale=SCALE)
            a.reset()
            b.reset()
            a.network_render_accumulate(na, 1, 3, **expm)
            for sid in range(1, 4):
                b.network_render_subframe(nb, sid, out=False, **expm)
                b.accumulate(sid)
            sa, sb2 = _progressive(a), _progressive(b)
            assert np.array_equal(sa[0], sb2[0]) and np.array_equal(sa[1], sb2[1]) and sa[2] == sb2[2] == 3
            assert sa[0][..., :3].any() and not np.array_equal(sa[0], sb[0])
        finally:
            na.close()
            nb.close()


def _code(fn, *a, **kw):
    with pytest.raises(_lib.CloudTraceError) as e:
        fn(*a, **kw)
    return e.value.code


@pytest.mark.gpu
def test_order_errors_leave_the_handle_usable():
    with ds.CloudTracer(cloud(), width=W, height=H) as tr:
        net = N.Network(tr, weights(SMALL), 32, 1, 1)
        try:
            assert _code(tr.network_render_accumulate, net, 2, 1) == _lib.CT_E_STATE       # first != subframes + 1
            assert b"subframes are accumulated" in tr.L.ct_last_error(tr.h)
            assert _code(tr.network_render_accumulate, net, 1, 0) == _lib.CT_E_INVAL       # count == 0
            assert _code(tr.network_render_accumulate, net, 0, 1) == _lib.CT_E_INVAL       # ids are 1-based
            assert _code(tr.network_render_subframe, net, 0) == _lib.CT_E_INVAL
            assert tr.subframes == 0 and not tr.mean().any()
            tr.network_render_accumulate(net, 1, 2, rgb_scale=SCALE)
            assert tr.subframes == 2
            assert _code(tr.network_render_accumulate, net, 2, 1) == _lib.CT_E_STATE
            assert _code(tr.network_render_accumulate, net, 4, 1) == _lib.CT_E_STATE
            assert _code(tr.render_accumulate, 4, 1) == _lib.CT_E_STATE                    # (the estimator's answer to the same mistake)
            before = tr.mean()
            tr.network_render_accumulate(net, 3, 1, rgb_scale=SCALE)
            assert tr.subframes == 3 and not np.array_equal(tr.mean(), before)
        finally:
            net.close()


@pytest.mark.gpu
def test_invalid_arguments_leave_the_handle_usable(tracer, nets):
    want = reference_frame(tracer, nets)
    net = nets()
    L, h = tracer.L, tracer.h

    def still_renders():
        assert np.array_equal(tracer.network_render_subframe(net, SID, rgb_scale=SCALE).cpu().numpy(), want)

    def params(abi=_lib.CT_ABI_VERSION, transform=0, scale=(1, 1, 1)):
        return _lib.CtNetworkRender(abi, transform, (C.c_float * 3)(*scale), 0)

    for shape in (N.NetworkShape(32, 0, 1), N.NetworkShape(16, 2, 1)):                       # aux 0, aux 2
        with N.Network(tracer, seeded_weights(shape, 2), shape.width, shape.aux, shape.head_layers) as other:
            assert _code(tracer.network_render_subframe, other, SID) == _lib.CT_E_INVAL
            assert _code(tracer.network_render_accumulate, other, 1, 1) == _lib.CT_E_INVAL
        still_renders()
    for bad in (dict(transform=2), dict(transform=-1), dict(transform="log"), dict(rgb_scale=(1, np.nan, 1)), dict(rgb_scale=(np.inf, 1, 1)),
                dict(rgb_scale=(1, 1, -np.inf))):
        assert _code(tracer.network_render_subframe, net, SID, **bad) == _lib.CT_E_INVAL, bad
        assert _code(tracer.network_render_accumulate, net, 1, 1, **bad) == _lib.CT_E_INVAL, bad
        still_renders()
    p = params(abi=_lib.CT_ABI_VERSION + 1)
    assert L.ct_network_render_subframe(h, net.n, C.byref(p), SID, None) == _lib.CT_E_INVAL
    assert L.ct_network_render_accumulate(h, net.n, C.byref(p), 1, 1) == _lib.CT_E_INVAL
    assert b"abi_version" in L.ct_last_error(h)
    p = params()
    assert L.ct_network_render_subframe(h, None, C.byref(p), SID, None) == _lib.CT_E_INVAL
    assert L.ct_network_render_subframe(h, net.n, None, SID, None) == _lib.CT_E_INVAL
    assert L.ct_network_render_accumulate(h, None, C.byref(p), 1, 1) == _lib.CT_E_INVAL
    assert L.ct_network_render_accumulate(h, net.n, None, 1, 1) == _lib.CT_E_INVAL
    assert L.ct_debug_network_render_time(h, None) == _lib.CT_E_INVAL
    assert tracer.subframes == 0 and not tracer.mean().any()                                # nothing was accumulated by any of them
    still_renders()
    # a shard of a multi-GPU job: refused with a message that says so, and the shard goes on rendering its tiles
    with ds.CloudTracer(cloud(), width=W, height=H, shard_index=0, shard_count=2) as shard:
        with N.Network(shard, weights(SMALL), 32, 1, 1) as sn:
            assert _code(shard.network_render_subframe, sn, SID) == _lib.CT_E_INVAL
            assert b"shard" in shard.L.ct_last_error(shard.h)
            assert _code(shard.network_render_accumulate, sn, 1, 1) == _lib.CT_E_INVAL
        shard.render_accumulate(1, 1)
        assert shard.subframes == 1 and shard.mean().any()
    still_renders()


def _state(tr):
    return tr.mean(), tr.m2(), tr.subframes, tr.counters(), tr.fetch_counters()


@pytest.mark.gpu
@pytest.mark.parametrize("ahead", [False, True])
def test_render_subframe_has_no_side_effects_on_a_progressive_render(ahead):
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
                with N.Network(tr, weights(SMALL), 32, 1, 1) as net:
                    frame = tr.network_render_subframe(net, SID, rgb_scale=SCALE, band_pixels=48)
                    assert bool((frame[..., :3] != 0).any())
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


@pytest.mark.gpu
def test_other_estimators_layouts_and_a_new_light(tracer, nets):
    want = reference_frame(tracer, nets, SID, SMALL)

    def frame_of(tr):
        with N.Network(tr, weights(SMALL), 32, 1, 1) as net:
            got = tr.network_render_subframe(net, SID, rgb_scale=SCALE).cpu().numpy()
            return got, definition(tr, net, SID)[0]

    for kw in (dict(estimator=_lib.CT_EST_DELTA), dict(flags=_lib.CT_FLAG_SPARSE_BRICKS)):
        with ds.CloudTracer(cloud(), width=W, height=H, **kw) as tr:
            assert np.array_equal(frame_of(tr)[0], want), kw
    with ds.CloudTracer(cloud(), width=W, height=H, flags=_lib.CT_FLAG_TEX_FIXED8) as tr:
        got, own = frame_of(tr)                                     # its own records: the flag changes flight and gather
        assert np.array_equal(got, own) and got[..., :3].any()
    with ds.CloudTracer(cloud(), width=W, height=H) as tr:
        old, own = frame_of(tr)
        assert np.array_equal(old, want) and np.array_equal(own, want)
        tr.set_light(LIGHT2)
        lit, own = frame_of(tr)
        assert np.array_equal(lit, own) and lit[..., :3].any() and not np.array_equal(lit, old)


@pytest.mark.gpu
def test_scratch_is_reused_grown_and_kept(tracer, nets):
    want = {sid: reference_frame(tracer, nets, sid, SMALL) for sid in (1, SID)}
    with ds.CloudTracer(cloud(), width=W, height=H) as tr, N.Network(tr, weights(SMALL), 32, 1, 1) as net:
        assert tr.network_render_time() == (0.0, 0.0, 0.0, 0.0)
        for band in (24, 24, 0, 48, 24):          # a first call, a warm one, a larger band (growth), smaller ones again
            assert np.array_equal(tr.network_render_subframe(net, SID, rgb_scale=SCALE, band_pixels=band).cpu().numpy(), want[SID]), band
            times = tr.network_render_time()
            assert len(times) == 4 and all(np.isfinite(t) and t >= 0 for t in times) and times[2] > 0 and times[0] > 0
            # one accumulated subframe IS its frame: mean = 0 + (x - 0) * 1, M2 = 0 + (x - 0) * (x - x)
            tr.reset()
            tr.network_render_accumulate(net, 1, 1, rgb_scale=SCALE, band_pixels=band)
            assert np.array_equal(tr.mean(), want[1]) and not tr.m2().any() and tr.subframes == 1, band
            times = tr.network_render_time()
            assert all(np.isfinite(t) and t >= 0 for t in times) and times[2] > 0
            tr.reset()


@pytest.mark.gpu
def test_a_band_in_pieces_gives_the_same_bits(tracer, nets, monkeypatch):
    """When the descriptor array cannot hold a band's records (the device refused its growth, or CT_NET_DESC_RECORDS caps
    it, as here), the records go through gather, aux and network in pieces of the array's size.  16: subframe 3's 79 records
    make five pieces, the last of 15; 1: one record per piece; 79 and 1000: the whole band at once."""
    want = {sid: reference_frame(tracer, nets, sid, SMALL) for sid in (1, SID)}
    for cap in ("16", "1", "79", "1000"):
        monkeypatch.setenv("CT_NET_DESC_RECORDS", cap)
        with ds.CloudTracer(cloud(), width=W, height=H) as tr, N.Network(tr, weights(SMALL), 32, 1, 1) as net:
            for band in (0, 72):
                got = tr.network_render_subframe(net, SID, rgb_scale=SCALE, band_pixels=band)
                assert np.array_equal(got.cpu().numpy(), want[SID]), (cap, band)
            tr.network_render_accumulate(net, 1, 1, rgb_scale=SCALE)
            assert np.array_equal(tr.mean(), want[1]) and not tr.m2().any(), cap
            assert tr.network_render_time()[2] > 0


@pytest.mark.gpu
def test_cli_renders_with_the_network(tmp_path):
    """cloudtrace --network: the written images are Python's mean after network_render_accumulate(1, 4) under the same light
    and pose, for both of the job's suns (the second through ct_set_light, as for the estimator)."""
    from deepestscatter_amd import build
    cli = build.build_cli()
    N.save_weights(tmp_path / "w.bin", weights(FLAGSHIP), FLAGSHIP)
    r = subprocess.run([str(cli), "procedural:64", "--network", str(tmp_path / "w.bin"), "--size", f"{W}x{H}", "--spp", "4", "--format", "pfm",
                        "--net-scale", "0.5,2,3", "--out", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "rendering subframe 4" in r.stdout
    with ds.CloudTracer(cloud(), width=W, height=H, light_direction=ds.LIGHT_DIRECTIONS["Side"]) as tr:
        with N.Network(tr, weights(FLAGSHIP), 200, 1, 3) as net:
            images = {}
            for light in ("Side", "Back"):
                tr.set_light(ds.LIGHT_DIRECTIONS[light])
                tr.reset()
                tr.network_render_accumulate(net, 1, 4, rgb_scale=SCALE)
                images[light] = tr.mean()[..., :3]
    assert not np.array_equal(images["Side"], images["Back"])
    for light, want in images.items():
        raw = (tmp_path / f"procedural_64.{light}.PT.pfm").read_bytes()
        header_end = 0
        for _ in range(3):
            header_end = raw.index(b"\n", header_end) + 1
        assert raw[:header_end].split() == [b"PF", str(W).encode(), str(H).encode(), b"-1.0"]
        img = np.frombuffer(raw[header_end:], "<f4").reshape(H, W, 3)
        assert want.any() and np.array_equal(img, want), light
