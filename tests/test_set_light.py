"""ct_set_light: a live handle re-lit in place (the GPU cases run with -m gpu on an MI355X).

The reference for everything here is a handle freshly created with the target light -- code the verb does not touch: after
`set_light` the device state (shadow volume, its apron bricks, the march bricks with their shadow-zero flags, the twin bricks'
shadow half) must be that handle's byte for byte, and after `reset()` the rendered frame and the counters must be its too.
"Equal" is np.array_equal / equal dicts throughout.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import _oracle as O
import deepestscatter_amd as ds
from deepestscatter_amd import _lib

gpu = pytest.mark.gpu

W, H, SPP = 40, 32, 3
BASE = dict(width=W, height=H, cloud_size_m=20000.0)
LIGHTS = dict(ds.LIGHT_DIRECTIONS, Axis=(0.0, -1.0, 0.0))
LAYOUTS = ("density_bricks", "shadow_bricks", "march_bricks", "march_rows", "march_coarse", "twin_bricks")

_TEX = []
_FRESH = {}


def cloud():
    if not _TEX:
        _TEX.append(ds.make_procedural_cloud(64))
    return _TEX[0]


def make(monkeypatch, env, **kw):
    """A handle on the test cloud, created with `env` (CT_* knobs are read once, at ct_create) in the environment."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tr = ds.CloudTracer(cloud(), **{**BASE, **kw})
    for k in env:
        monkeypatch.delenv(k)
    return tr


def layouts(tr):
    out = {}
    for name in LAYOUTS:
        try:
            out[name] = tr.layout(name)[0]
        except _lib.CloudTraceError as e:      # a layout this kind of handle does not have
            assert e.code == _lib.CT_E_INVAL
    return out


def device_state(tr):
    mm = tr.march_meta()
    return {"inscatter": tr.inscatter(), "layouts": layouts(tr), "radius": mm["radius"], "meta": mm["meta"], "sparse": mm["sparse"]}


def rendered(tr):
    """The frame of SPP subframes from a clean image, and every counter."""
    tr.reset()
    tr.render_accumulate(1, SPP)
    return {"mean": tr.mean(), "m2": tr.m2(), "counters": tr.counters(), "fetch": tr.fetch_counters()}


def fresh(monkeypatch, env, **kw):
    """State and frame of a handle freshly created with `kw` under `env`: computed once, shared, never modified."""
    key = repr((sorted(env.items()), sorted(kw.items())))
    if key not in _FRESH:
        tr = make(monkeypatch, env, **kw)
        _FRESH[key] = {**device_state(tr), **rendered(tr)}
        tr.close()
    return _FRESH[key]


def same_state(got, want):
    assert np.array_equal(got["inscatter"], want["inscatter"])
    assert got["radius"] == want["radius"] and got["sparse"] == want["sparse"]
    assert (got["meta"] is None) == (want["meta"] is None)
    if want["meta"] is not None:
        assert np.array_equal(got["meta"], want["meta"])
    assert got["layouts"].keys() == want["layouts"].keys()
    for name, ref in want["layouts"].items():
        assert np.array_equal(got["layouts"][name], ref), name


def same_frame(got, want, fetch=True):
    assert np.array_equal(got["mean"], want["mean"])
    assert np.array_equal(got["m2"], want["m2"])
    assert got["counters"] == want["counters"]
    if fetch:
        assert got["fetch"] == want["fetch"]


def relit_equals_fresh(monkeypatch, src, dst, env=None, **kw):
    """create(src) -> set_light(dst) must be create(dst) in device state and in the frame it renders."""
    env = env or {}
    tr = make(monkeypatch, env, light_direction=LIGHTS[src], **kw)
    before = layouts(tr)
    tr.render_accumulate(1, 2)                    # the handle has rendered under the old light
    tr.set_light(LIGHTS[dst])
    want = fresh(monkeypatch, env, light_direction=LIGHTS[dst], **kw)
    got = device_state(tr)
    same_state(got, want)
    assert np.array_equal(got["layouts"]["density_bricks"], before["density_bricks"])
    frame = rendered(tr)
    same_frame(frame, want)
    return tr, before, got, frame


# ---- CPU ---------------------------------------------------------------------------------------------------------------------

def test_null_handle_and_null_group_are_invalid_arguments(product_lib):
    d = np.array(LIGHTS["Back"], np.float32)
    p = d.ctypes.data_as(C.c_void_p)
    assert product_lib.ct_set_light(None, p, None, 1e6) == _lib.CT_E_INVAL
    assert product_lib.ct_group_set_light(None, p, None, 1e6) == _lib.CT_E_INVAL


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("src,dst", [("Side", "Back"), ("Back", "Front"), ("Side", "Axis")])
def test_relight_equals_fresh(monkeypatch, src, dst):
    tr, _, got, frame = relit_equals_fresh(monkeypatch, src, dst)
    assert not got["sparse"] and got["radius"] >= 1 and (got["meta"] & 0x40).any()
    if (src, dst) == ("Side", "Back"):
        orc = O.Oracle(cloud(), W, H, fast=True, light_direction=LIGHTS[dst], cloud_size_m=20000.0)
        assert np.array_equal(got["inscatter"], orc.inscatter)
        ref_mean, ref_m2 = orc.render(SPP)
        assert np.array_equal(frame["mean"], ref_mean) and np.array_equal(frame["m2"], ref_m2)
        assert frame["counters"] == orc.counters.as_dict()
    tr.close()


@gpu
def test_stale_shadow_zero_flags_are_cleared(monkeypatch):
    side = fresh(monkeypatch, {}, light_direction=LIGHTS["Side"])
    back = fresh(monkeypatch, {}, light_direction=LIGHTS["Back"])
    fs, fb = (side["meta"] & 0x40) != 0, (back["meta"] & 0x40) != 0
    assert (fs & ~fb).any() and (fb & ~fs).any()      # else a kernel that only ever sets bit 6 would pass
    tr = make(monkeypatch, {}, light_direction=LIGHTS["Side"])
    tr.set_light(LIGHTS["Back"])
    tr.set_light(LIGHTS["Side"])
    same_state(device_state(tr), side)
    same_frame(rendered(tr), side)
    tr.close()


@gpu
def test_sparse_bricks(monkeypatch):
    tr, _, got, _ = relit_equals_fresh(monkeypatch, "Side", "Back", env={"CT_SPARSE": "1"})
    assert got["sparse"] and tr.march_meta()["sparse"]
    assert {"march_bricks", "march_rows", "march_coarse"} <= got["layouts"].keys()
    # and the walk over the stored bricks writes the dense walk's bytes
    assert np.array_equal(got["inscatter"], fresh(monkeypatch, {}, light_direction=LIGHTS["Back"])["inscatter"])
    tr.close()


@gpu
@pytest.mark.parametrize("nee", ["0", "1", "2"])
def test_delta(monkeypatch, nee):
    tr, before, got, _ = relit_equals_fresh(monkeypatch, "Side", "Back", env={"CT_DELTA_NEE": nee}, estimator=1)
    assert tr.delta_grid()["nee"] == int(nee)
    assert ("twin_bricks" in got["layouts"]) == (nee == "2")
    if nee == "2":
        twin = got["layouts"]["twin_bricks"]
        assert np.array_equal(twin[..., :64], before["twin_bricks"][..., :64])           # the density half was left alone
        assert not np.array_equal(twin[..., 64:], before["twin_bricks"][..., 64:])
    tr.close()


@gpu
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_tex_fixed8_and_modes(monkeypatch, mode):
    tr, _, _, _ = relit_equals_fresh(monkeypatch, "Back", "Side", flags=_lib.CT_FLAG_TEX_FIXED8, mode=mode)
    tr.close()


@gpu
@pytest.mark.parametrize("invariants", [False, True])
def test_nothing_of_the_old_light_survives_in_flight(monkeypatch, invariants):
    env = {"CT_DEBUG_INVARIANTS": "1"} if invariants else {}
    tr = make(monkeypatch, env, light_direction=LIGHTS["Side"])
    tr.set_render_ahead(8)
    for k in range(3):
        tr.render_accumulate_async(1 + 2 * k, 2)          # rendered ahead, paths suspended, nothing waited for
    tr.set_light(LIGHTS["Back"])
    assert tr.rendered_subframes() == tr.subframes == 6
    want = fresh(monkeypatch, {}, light_direction=LIGHTS["Back"])
    same_state(device_state(tr), want)
    same_frame(rendered(tr), want)
    if invariants:
        iv = tr.debug_invariants()
        assert iv["armed"] and iv["checks"] > 0 and iv["violations"] == 0
    tr.close()


@gpu
def test_normalisation(monkeypatch):
    long_back = tuple(2.5 * v for v in LIGHTS["Back"])
    tr = make(monkeypatch, {}, light_direction=LIGHTS["Side"])
    tr.set_light(long_back)
    want = fresh(monkeypatch, {}, light_direction=long_back)
    same_state(device_state(tr), want)
    same_frame(rendered(tr), want)
    tr.close()
    # CT_FLAG_LIGHT_NORMALIZED: the vector is used as given (here: once-normalised in float64, not what two float32 passes give)
    v = np.array(LIGHTS["Back"], np.float64)
    given = tuple(float(x) for x in (v / np.linalg.norm(v)).astype(np.float32))
    tr = make(monkeypatch, {}, light_direction=LIGHTS["Side"], flags=_lib.CT_FLAG_LIGHT_NORMALIZED)
    tr.set_light(given)
    want = fresh(monkeypatch, {}, light_direction=given, flags=_lib.CT_FLAG_LIGHT_NORMALIZED)
    same_state(device_state(tr), want)
    same_frame(rendered(tr), want)
    tr.close()


@gpu
def test_colour_and_intensity(monkeypatch):
    colour = (0.5, 1.0, 2.0)
    tr = make(monkeypatch, {}, light_direction=LIGHTS["Side"])
    tr.set_light(LIGHTS["Back"], color=colour, intensity=3e5)
    want = fresh(monkeypatch, {}, light_direction=LIGHTS["Back"], light_color=colour, light_intensity=3e5)
    same_state(device_state(tr), want)
    same_frame(rendered(tr), want)
    assert not np.array_equal(want["mean"], fresh(monkeypatch, {}, light_direction=LIGHTS["Back"])["mean"])
    # color=None keeps the colour; the intensity is always set
    tr.set_light(LIGHTS["Front"], intensity=1e6)
    want = fresh(monkeypatch, {}, light_direction=LIGHTS["Front"], light_color=colour)
    same_state(device_state(tr), want)
    same_frame(rendered(tr), want)
    # an infinite intensity: no shadow-zero skip, every flag clear, as a fresh handle has it
    tr.set_light(LIGHTS["Back"], intensity=float("inf"))
    mm = tr.march_meta()
    assert mm["radius"] == 0 and not (mm["meta"] & 0x40).any()
    tr.close()
    inf = make(monkeypatch, {}, light_direction=LIGHTS["Back"], light_color=colour, light_intensity=float("inf"))
    ref = inf.march_meta()
    assert ref["radius"] == 0 and np.array_equal(ref["meta"], mm["meta"])
    inf.close()


@gpu
def test_other_consumers_of_the_light(monkeypatch):
    def consumers(tr):
        pos, view = tr.generate_scatter_samples(256, batch_seed=3)
        tasks = tr.point_radiance_launch(ds.make_point_tasks(pos[:64], view[:64]), 1, 2)
        return pos, view, tasks.tobytes(), tr.collect_descriptors(pos[:32], view[:32])

    kw = dict(mode=1)
    tr = make(monkeypatch, {}, light_direction=LIGHTS["Side"], **kw)
    old = consumers(tr)
    tr.set_light(LIGHTS["Back"])
    got = consumers(tr)
    new = make(monkeypatch, {}, light_direction=LIGHTS["Back"], **kw)
    want = consumers(new)
    for g, w in zip(got, want):
        assert np.array_equal(g, w) if isinstance(w, np.ndarray) else g == w
    assert got[2] != old[2] and not np.array_equal(got[3], old[3])     # radiance and descriptor frame do follow the light
    tr.close()
    new.close()


@gpu
def test_rejected_calls_change_nothing(monkeypatch):
    tr = make(monkeypatch, {}, light_direction=LIGHTS["Side"])
    for bad in ((0.0, 0.0, 0.0), (float("nan"), -1.0, 0.0), (0.0, float("inf"), 0.0), None):
        with pytest.raises(_lib.CloudTraceError) as e:
            tr.set_light(bad, color=(9.0, 9.0, 9.0), intensity=7.0)
        assert e.value.code == _lib.CT_E_INVAL
    want = fresh(monkeypatch, {}, light_direction=LIGHTS["Side"])
    same_state(device_state(tr), want)
    same_frame(rendered(tr), want)
    tr.close()


@gpu
def test_group(monkeypatch):
    g = ds.TracerGroup(cloud(), devices=[0, 0], **{**BASE, "light_direction": LIGHTS["Side"]})
    g.render_accumulate(1, 2)
    g.mean()                                            # merged under the old light: must go stale
    g.set_light(LIGHTS["Back"])
    g.reset()
    g.render_accumulate(1, SPP)
    want = fresh(monkeypatch, {}, light_direction=LIGHTS["Back"])
    assert np.array_equal(g.mean(), want["mean"]) and np.array_equal(g.m2(), want["m2"])
    assert g.counters() == want["counters"]
    with pytest.raises(_lib.CloudTraceError) as e:
        g.set_light((0.0, 0.0, 0.0))
    assert e.value.code == _lib.CT_E_INVAL
    g.close()


@gpu
def test_cli_renders_two_lights_on_one_context(tmp_path):
    """cloudtrace --light Side --light Back re-lights the first task's renderer for the second: same files as two runs."""
    from deepestscatter_amd import build
    cli = build.build_cli()

    def run(out, *lights):
        out.mkdir()
        args = [a for l in lights for a in ("--light", l)]
        r = subprocess.run([str(cli), "procedural:64", "--size", f"{W}x{H}", "--spp", str(SPP), "--size-m", "20000", "--out", str(out), *args],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return {p.name: p.read_bytes() for p in out.iterdir()}

    both = run(tmp_path / "both", "Side", "Back")
    assert sorted(both) == ["procedural_64.Back.PT.exr", "procedural_64.Side.PT.exr"]
    assert both["procedural_64.Back.PT.exr"] != both["procedural_64.Side.PT.exr"]
    for light in ("Side", "Back"):
        assert run(tmp_path / light, light) == {f"procedural_64.{light}.PT.exr": both[f"procedural_64.{light}.PT.exr"]}
