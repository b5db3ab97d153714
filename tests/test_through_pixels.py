"""Through pixels (run with -m gpu on an MI355X): a pixel whose primary ray crosses the box without meeting a non-zero
density footprint is classified once per pose and never rendered -- the host books its samples' counters, the accumulate
kernel its constant sample (0,0,0,1).

Nothing may change by a bit: mean, M2 and the six CtCounters are held against the CPU oracle, the classification against
the oracle's one-pixel windows, and ct_fetch_counters against the same handle with CT_THROUGH_PIXELS=0.

Two cases of the plan cannot be asked of the library and are held as what it answers instead: max_depth == 1 is refused by
ct_create (max_depth 2..65535), and a handle's density cannot be replaced (ct_upload takes the running mean and M2 only), so
"cloud in front of former through pixels" is a second handle with the fuller volume under the same pose.
"""
import numpy as np
import pytest

import _oracle as O
import deepestscatter_amd as ds
from deepestscatter_amd import _lib

pytestmark = pytest.mark.gpu

F8 = _lib.CT_FLAG_TEX_FIXED8
N, W, H, SPP = 96, 160, 128, 8
ORACLE_KEYS = ("mode", "cloud_size_m", "sample_step", "max_depth", "light_direction")
OFF = {"CT_THROUGH_PIXELS": "0"}
_VOL = {}
_SHADOW = {}
_REF = {}


def volume(name="cloud"):
    if name not in _VOL:
        if name == "cloud":
            v = ds.make_procedural_cloud(N)
        elif name == "empty":
            v = np.zeros((32, 32, 32), np.uint8)
        elif name == "full":
            v = np.full((32, 32, 32), 2, np.uint8)
        elif name == "fuller":
            # the cloud plus a thin slab across the whole box: cloud in front of (or behind) every former through pixel
            v = ds.make_procedural_cloud(N).copy()
            v[:, N // 2, :] = np.maximum(v[:, N // 2, :], 1)
        v.setflags(write=False)
        _VOL[name] = v
    return _VOL[name]


def pose(eye, lookat, w, h, fov=60.0):
    return (eye,) + tuple(ds.calculate_camera_variables(eye, lookat, (0, 1, 0), fov, w / h))


def oracle(vol, w, h, camera=None, f8=False, **kw):
    kw = {k: v for k, v in kw.items() if k in ORACLE_KEYS}
    # (the shadow volume does not depend on the frame, the pose, the mode or the depth cap: computed once, never modified)
    key = repr((vol, f8, sorted((k, v) for k, v in kw.items() if k not in ("mode", "max_depth"))))
    orc = O.Oracle(volume(vol), w, h, fast="fixed8" if f8 else True, inscatter=_SHADOW.get(key), **kw)
    if key not in _SHADOW:
        orc.inscatter.setflags(write=False)
        _SHADOW[key] = orc.inscatter
    if camera is not None:
        orc.set_camera(*pose(*camera, w, h))
    return orc


def reference(vol="cloud", w=W, h=H, spp=SPP, camera=None, f8=False, **kw):
    """(mean, M2, counters) of the oracle: computed once per scene and pose, shared, never modified."""
    key = repr((vol, w, h, spp, camera, f8, sorted(kw.items())))
    if key not in _REF:
        orc = oracle(vol, w, h, camera, f8, **kw)
        mean, m2 = orc.render(spp)
        for a in (mean, m2):
            a.setflags(write=False)
        _REF[key] = (mean, m2, orc.counters.as_dict())
    return _REF[key]


def tracer(monkeypatch, vol="cloud", w=W, h=H, env=None, camera=None, **kw):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    tr = ds.CloudTracer(volume(vol), width=w, height=h, **kw)
    for k in (env or {}):
        monkeypatch.delenv(k)
    if camera is not None:
        tr.set_camera(*pose(*camera, w, h))
    return tr


def holds(tr, ref):
    mean, m2, counters = ref
    assert np.array_equal(tr.mean(), mean)
    assert np.array_equal(tr.m2(), m2)
    assert tr.counters() == counters


def run_case(monkeypatch, vol="cloud", w=W, h=H, spp=SPP, env=None, camera=None, f8=False, **kw):
    """One frame against the oracle -> (pixel classes, fetch counters)."""
    with tracer(monkeypatch, vol, w, h, env=env, camera=camera, flags=F8 if f8 else 0, **kw) as tr:
        tr.render_accumulate(1, spp)
        holds(tr, reference(vol, w, h, spp, camera=camera, f8=f8, **kw))
        return tr.debug_pixel_classes(), tr.fetch_counters()


def all_three(cls, w=W, h=H):
    assert cls["misses"] > 0 and cls["listed"] > 0 and cls["through"] > 0 and cls["through_steps"] >= cls["through"], cls
    assert cls["misses"] + cls["listed"] + cls["through"] == w * h


# ---- parity ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1, 2])
def test_every_mode(monkeypatch, mode):
    cls, _ = run_case(monkeypatch, mode=mode)
    if mode == 1:
        # (the direction is drawn before the first flight: no sample takes the prefix, nothing is classified)
        assert cls["through"] == 0 and cls["through_steps"] == 0 and cls["misses"] > 0 and cls["listed"] > 0
    else:
        all_three(cls)


@pytest.mark.parametrize("max_depth", [1, 2])
def test_at_the_depth_cap(monkeypatch, max_depth):
    if max_depth == 1:
        # a sample capped before its first flight makes no lookup, so no pixel could be a through pixel: ct_create does not
        # take such a scene at all
        with pytest.raises(_lib.CloudTraceError) as e:
            ds.CloudTracer(volume(), width=W, height=H, max_depth=1)
        assert e.value.code == _lib.CT_E_INVAL and "max_depth 2..65535" in e.value.message
        return
    cls, _ = run_case(monkeypatch, max_depth=max_depth)
    all_three(cls)
    assert reference(max_depth=max_depth)[2]["depth_capped"] > 0


def test_sparse_bricks(monkeypatch):
    all_three(run_case(monkeypatch, env={"CT_SPARSE": "1"})[0])


def test_fixed8_filter(monkeypatch):
    all_three(run_case(monkeypatch, f8=True)[0])


def test_knob_off_and_what_the_kernels_fetched(monkeypatch):
    off, fetched_off = run_case(monkeypatch, env=OFF)
    on, fetched_on = run_case(monkeypatch)
    all_three(on)
    assert off["through"] == 0 and off["through_steps"] == 0
    assert off["misses"] == on["misses"] and off["listed"] == on["listed"] + on["through"]
    # a sample of a through pixel issues one fetch: its prefix ends before the decisive step
    assert fetched_on["density_fetches"] == fetched_off["density_fetches"] - on["through"] * SPP


def test_no_advance_lists_every_hit(monkeypatch):
    cls, _ = run_case(monkeypatch, env={"CT_NO_ADVANCE": "1"})
    assert cls["through"] == 0 and cls["listed"] > 0


def test_two_shards_make_the_unsharded_frame(monkeypatch):
    mean, m2, counters = reference()
    total_mean, total_m2, ctr, classes = np.zeros_like(mean), np.zeros_like(m2), None, None
    for i in range(2):
        with tracer(monkeypatch, shard_index=i, shard_count=2) as sh:
            sh.render_accumulate(1, SPP)
            m = sh.mean()
            assert np.all(m[~ds.shard_mask(W, H, i, 2)] == 0)
            total_mean += m
            total_m2 += sh.m2()
            c, k = sh.counters(), sh.debug_pixel_classes()
            assert k["through"] > 0
            ctr = c if ctr is None else {x: ctr[x] + c[x] for x in c}
            classes = k if classes is None else {x: classes[x] + k[x] for x in k}
    assert np.array_equal(total_mean, mean) and np.array_equal(total_m2, m2)
    assert ctr == counters
    with tracer(monkeypatch) as whole:
        assert whole.debug_pixel_classes() == classes


# ---- classification ----------------------------------------------------------------------------------------------------------

def near_cloud(w, h, eye=(2.5, -0.4, 0.0)):
    """Per pixel: does the primary ray pass within a texel of a non-zero footprint?  (float64 positions every half step and
    footprints widened by a texel each way, so whatever the float32 march meets is found.)"""
    vol = volume()
    occ = np.pad(vol > 0, 2)
    wide = np.zeros_like(vol, bool)
    for dz in range(4):
        for dy in range(4):
            for dx in range(4):   # texels i-1 .. i+2 of the footprint's base texel i
                wide |= occ[1 + dz:1 + dz + N, 1 + dy:1 + dy + N, 1 + dx:1 + dx + N]
    U, V, Wv = (np.asarray(v, np.float64) for v in O.camera_variables(eye, aspect=w / h))
    ys, xs = np.mgrid[0:h, 0:w]
    d = (xs / w * 2 - 1)[..., None] * U + (ys / h * 2 - 1)[..., None] * V + Wv
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    out = np.zeros((h, w), bool)
    for t in np.arange(1.5, 3.6, 1.0 / 1024.0):             # (the box lies 1.67 .. 3.41 from the eye)
        p = np.asarray(eye) + d * t + 0.5                       # box coordinates, [0, 1]^3
        inside = np.all((p >= -0.02) & (p <= 1.02), axis=-1)
        i = np.clip(np.floor(p * N - 0.5).astype(int), 0, N - 1)
        out |= inside & wide[i[..., 2], i[..., 1], i[..., 0]]
    return out


def test_classes_against_the_oracle(monkeypatch):
    with tracer(monkeypatch) as tr:
        cls, steps = tr.debug_pixel_class_plane()
        counts = tr.debug_pixel_classes()
    all_three(counts)
    assert [(cls == k).sum() for k in range(3)] == [counts["misses"], counts["listed"], counts["through"]]
    assert int(steps[cls == 2].sum()) == counts["through_steps"] and np.all(steps[cls != 2] == 0)
    assert np.all(steps[cls == 2] > 0)
    # every listed pixel has cloud on its primary ray
    assert np.all(near_cloud(W, H)[cls == 1])
    # 24 pixels of each class, spread over the class: the oracle's one-pixel window over 4 subframes
    orc = oracle("cloud", W, H)
    for k in (1, 2):
        ys, xs = np.nonzero(cls == k)
        pick = np.linspace(0, len(ys) - 1, 24).astype(int)
        assert len(set(pick)) >= 16
        scattered = 0
        for y, x in zip(ys[pick], xs[pick]):
            orc.counters = O.OrcCounters()
            orc.render(4, window=(int(x), int(y), int(x) + 1, int(y) + 1))
            c = orc.counters.as_dict()
            assert c["box_hits"] == 4
            if k == 2:
                assert c["scatter_events"] == 0 and c["density_lookups"] == 4 * int(steps[y, x]), (x, y, c)
            else:
                scattered += c["scatter_events"] > 0
        assert k == 2 or scattered > 0


# ---- edges -------------------------------------------------------------------------------------------------------------------

def test_empty_volume_two_batches(monkeypatch):
    w, h = 40, 32
    with tracer(monkeypatch, "empty", w, h) as tr:
        tr.render_accumulate(1, 3)
        tr.render_accumulate(4, 2)
        holds(tr, reference("empty", w, h, 5))
        cls = tr.debug_pixel_classes()
        assert cls["listed"] == 0 and cls["through"] > 0 and cls["misses"] > 0
        assert tr.fetch_counters() == {"density_fetches": 0, "inscatter_fetches": 0}
        assert tr.counters()["density_lookups"] == cls["through_steps"] * 5


def test_density_in_every_texel(monkeypatch):
    w, h = 40, 32
    cls, _ = run_case(monkeypatch, "full", w, h, 2, max_depth=4)
    assert cls["through"] == 0 and cls["listed"] > 0 and cls["misses"] > 0


def test_listed_pixels_do_not_fill_the_last_group(monkeypatch):
    w, h = 150, 117
    cls, _ = run_case(monkeypatch, w=w, h=h, spp=3)
    all_three(cls, w, h)
    assert cls["listed"] % 64 != 0


# ---- pipelines ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ahead", [False, True])
def test_enqueued_batches_equal_one_waited_for(monkeypatch, ahead):
    kw = dict(cloud_size_m=30000.0, max_depth=300)
    with tracer(monkeypatch, **kw) as sync, tracer(monkeypatch, env={"CT_DEBUG_INVARIANTS": "1"}, **kw) as tr:
        sync.render_accumulate(1, 7)
        if ahead:
            tr.set_render_ahead(4)
        tr.render_accumulate_async(1, 3)
        tr.render_accumulate_async(4, 1)
        tr.render_accumulate_async(5, 3)
        tr.synchronize()
        assert np.array_equal(tr.mean(), sync.mean()) and np.array_equal(tr.m2(), sync.m2())
        assert tr.counters() == sync.counters()
        iv = tr.debug_invariants()
        assert iv["armed"] == 1 and iv["violations"] == 0 and iv["samples_without_alpha_1"] == 0, iv
        assert iv["dealt"] == iv["written"] == sync.counters()["box_hits"], iv
        assert tr.debug_pixel_classes()["through"] > 0


# ---- reclassification --------------------------------------------------------------------------------------------------------

def test_new_pose_on_the_same_handle(monkeypatch):
    near = ((1.2, 0.3, -0.8), (0.0, 0.0, 0.0))
    with tracer(monkeypatch) as tr, tracer(monkeypatch, camera=near) as fresh:
        tr.render_accumulate(1, 2)
        first = tr.debug_pixel_classes()
        tr.set_camera(*pose(*near, W, H))
        tr.reset()
        tr.render_accumulate(1, 3)
        fresh.render_accumulate(1, 3)
        assert np.array_equal(tr.mean(), fresh.mean()) and np.array_equal(tr.m2(), fresh.m2())
        assert tr.counters() == fresh.counters() and tr.fetch_counters()["density_fetches"] == fresh.fetch_counters()["density_fetches"]
        assert tr.debug_pixel_classes() == fresh.debug_pixel_classes() != first
        holds(tr, reference(spp=3, camera=near))


def test_cloud_in_front_of_former_through_pixels(monkeypatch):
    with tracer(monkeypatch) as thin, tracer(monkeypatch, "fuller") as full:
        a, _ = thin.debug_pixel_class_plane()
        b, _ = full.debug_pixel_class_plane()
        assert np.array_equal(a == 0, b == 0)
        assert ((a == 2) & (b == 1)).sum() > 0 and not ((a == 1) & (b == 2)).any()
        full.render_accumulate(1, 2)
        holds(full, reference("fuller", spp=2))


def test_new_light_keeps_the_classes(monkeypatch):
    with tracer(monkeypatch, light_direction=ds.LIGHT_DIRECTIONS["Back"]) as tr:
        tr.render_accumulate(1, 2)
        before = tr.debug_pixel_class_plane()
        tr.set_light(ds.LIGHT_DIRECTIONS["Side"])
        tr.reset()
        tr.render_accumulate(1, 3)
        after = tr.debug_pixel_class_plane()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        holds(tr, reference(spp=3, light_direction=ds.LIGHT_DIRECTIONS["Side"]))
