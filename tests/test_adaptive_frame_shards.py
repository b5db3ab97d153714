"""Adaptive frames on sharded handles and on a CtGroup: ct_adaptive_frame_create_shard and ct_group_adaptive_frame_*
(include/cloudtrace.h).

A shard's frame runs the adaptive frame's rounds over the shard's own pixels only; the union of the shards' frames is the whole
frame's, bit for bit, and the group's merge -- the unsigned maximum of every 32-bit word -- is that union.  Every comparison is on
the bits (tobytes()).  The CPU tests hold the shard references to the whole reference over the CPU oracle and assert there the
conditions the cases were chosen for; the GPU tests hold every shard frame and every group to a whole-frame ct_adaptive_frame on
an unsharded handle of the same scene, which tests/test_adaptive_frame.py holds to the uniform images (and one test here too).

Scene: test_adaptive_frame's -- sphere_volume(32, seed=12), default camera and light, set A (mode 0, R = 4, min 8, cap 96, rel
0.7, abs 1e-2) and set C (mode 2, rel 0.5).  Every group is a rehearsal on one device (devices = [0] * N).

Cases (frame, N): own pixels, paths and capped pixels per shard, as the reference gives them on the oracle with fast=True:
  24 x 16, 2   192 / 192                    5008 / 4512                             19 / 21
  24 x 16, 3   128 / 128 / 128              1496 / 6356 / 1668                      5 / 34 / 1
  24 x 16, 8   64 x 6, 0, 0                 780, 3000, 872, 716, 3356, 796, 0, 0    3, 19, 1, 2, 15, 0, 0, 0
  20 x 12, 3   96 / 96 / 48 (partial tiles) 1792 / 4208 / 712                       10 / 17 / 2
   9 x 17, 5   64, 16, 1, 64, 8             864, 128, 8, 1096, 64                   3, 0, 0, 3, 0"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import _oracle as O
import deepestscatter_amd as ds
import test_adaptive_frame as T
from deepestscatter_amd import _lib
from deepestscatter_amd import adaptive as ad
from deepestscatter_amd import cloudtrace as ct
from deepestscatter_amd import exr

R = 4
CASES = {
    (24, 16, 2): dict(own=[192, 192], paths=[5008, 4512], capped=[19, 21]),
    (24, 16, 3): dict(own=[128, 128, 128], paths=[1496, 6356, 1668], capped=[5, 34, 1]),
    (24, 16, 8): dict(own=[64] * 6 + [0, 0], paths=[780, 3000, 872, 716, 3356, 796, 0, 0], capped=[3, 19, 1, 2, 15, 0, 0, 0]),
    (20, 12, 3): dict(own=[96, 96, 48], paths=[1792, 4208, 712], capped=[10, 17, 2]),
    (9, 17, 5): dict(own=[64, 16, 1, 64, 8], paths=[864, 128, 8, 1096, 64], capped=[3, 0, 0, 3, 0]),
}
WHOLE = {(24, 16): dict(rounds=24, paths=9520, capped=40), (20, 12): dict(rounds=24, paths=6712, capped=29), (9, 17): dict(paths=2160, capped=6)}
CASE_IDS = [f"{w}x{h}-{n}" for w, h, n in CASES]
NAMES = ("ct_adaptive_frame_create_shard", "ct_group_adaptive_frame_create", "ct_group_adaptive_frame_update", "ct_group_adaptive_frame_raise_cap",
         "ct_group_adaptive_frame_info", "ct_group_adaptive_frame_shard", "ct_group_adaptive_frame_merge", "ct_group_adaptive_frame_download",
         "ct_group_adaptive_frame_device_ptr", "ct_group_adaptive_frame_destroy")


def own_pixels(w, h, i, n):
    return ad.shard_pixels_reference(w, h, i, n)


def rounds_of(counts, own):
    """The rounds a shard runs: every pixel that is live in its last round holds rounds * R samples."""
    return int(counts.reshape(-1)[own].max()) // R if len(own) else 0


# ---------------------------------------------------------------------------------------------------- CPU
def test_symbols_resolve_and_answer_null_arguments(product_lib):
    L = product_lib
    assert len(NAMES) == 10
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.EXPORTS
    d = _lib.CtAdaptiveFrameDesc(_lib.CT_ABI_VERSION, 4, 8, 96, 0.1, 0.1, 0, 0)
    out, info = C.c_void_p(), _lib.CtAdaptiveFrameInfo()
    assert L.ct_adaptive_frame_create_shard(None, C.byref(d), C.byref(out)) == _lib.CT_E_INVAL
    assert L.ct_group_adaptive_frame_create(None, C.byref(d), C.byref(out)) == _lib.CT_E_INVAL and not out.value
    assert L.ct_group_adaptive_frame_update(None, 1) == _lib.CT_E_INVAL
    assert L.ct_group_adaptive_frame_raise_cap(None, 100) == _lib.CT_E_INVAL
    assert L.ct_group_adaptive_frame_info(None, C.byref(info)) == _lib.CT_E_INVAL
    assert L.ct_group_adaptive_frame_shard(None, 0, C.byref(out)) == _lib.CT_E_INVAL
    assert L.ct_group_adaptive_frame_merge(None) == _lib.CT_E_INVAL
    assert L.ct_group_adaptive_frame_download(None, 0, None, 0) == _lib.CT_E_INVAL
    assert L.ct_group_adaptive_frame_device_ptr(None, 0, C.byref(out)) == _lib.CT_E_INVAL
    assert L.ct_group_adaptive_frame_destroy(None) == _lib.CT_OK
    assert b"null" in L.ct_group_last_error(None)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("w, h", [(24, 16), (20, 12), (9, 17), (8, 8), (1, 1)])
def test_own_pixel_lists_are_the_tile_rule_and_partition_the_frame(w, h, n):
    lists = [own_pixels(w, h, i, n) for i in range(n)]
    for i, own in enumerate(lists):
        assert np.issubdtype(own.dtype, np.integer)
        assert own.tobytes() == np.flatnonzero(ct.shard_mask(w, h, i, n)).astype(own.dtype).tobytes()
        assert (np.diff(own) > 0).all()
    assert sorted(np.concatenate(lists).tolist()) == list(range(w * h))
    with pytest.raises(ValueError):
        ad.shard_pixels_reference(w, h, n, n)


_SNAPSHOTS = {}


def oracle_snapshots(w, h, name):
    """snapshot(c) of the whole w x h frame over the CPU oracle for the counts set `name` asks for, rendered once and kept."""
    key = (w, h, name)
    if key not in _SNAPSHOTS:
        orc = O.Oracle(T.volume(), w, h, mode=T.SETS[name]["mode"], fast=True)
        mean, m2 = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
        kept = {}

        def snapshot(c):
            for s in range(len(kept) * R + 1, c + 1):
                O.accumulate(orc.render_subframe(s), mean, m2, s)
                if s % R == 0:
                    kept[s] = (mean.copy(), m2.copy())
            return kept[c]

        _SNAPSHOTS[key] = snapshot
    return _SNAPSHOTS[key]


_REFERENCES = {}


def oracle_reference(w, h, name, pixels=None, key=None):
    k = (w, h, name, key)
    if k not in _REFERENCES:
        _REFERENCES[k] = ad.adaptive_frame_reference(oracle_snapshots(w, h, name), w, h, pixels=pixels, **T.params_of(name))
    return _REFERENCES[k]


def shard_references(w, h, n, name="A"):
    return [oracle_reference(w, h, name, own_pixels(w, h, i, n), (i, n)) for i in range(n)]


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def assert_shard_of(shard, whole, w, h, own):
    """(mean, m2, counts) of a shard: the whole frame's on the own pixels, zero bits elsewhere."""
    foreign = np.ones(w * h, bool)
    foreign[own] = False
    for a, b, width in zip(shard[:3], whole[:3], (4, 4, 1)):
        a, b = np.asarray(a).reshape(w * h, width), np.asarray(b).reshape(w * h, width)
        assert bits(a[own]) == bits(b[own])
        assert not a[foreign].view(np.uint32).any()


@pytest.mark.parametrize("w, h, n", list(CASES), ids=CASE_IDS)
def test_shards_on_the_oracle_are_the_whole_reference_and_have_the_histories_they_were_chosen_for(w, h, n):
    case = CASES[(w, h, n)]
    whole = oracle_reference(w, h, "A")
    if (w, h) == (24, 16):
        T.check_history("A", whole)
    shards = shard_references(w, h, n)
    for i, s in enumerate(shards):
        own = own_pixels(w, h, i, n)
        assert_shard_of(s, whole, w, h, own)
        assert len(s[3]) == rounds_of(whole[2], own)
        assert sorted(s[4]) == sorted(set(whole[4]) & set(own))
    merged = ad.merge_reference([s[:3] for s in shards])
    assert [bits(a) for a in merged] == [bits(a) for a in whole[:3]]
    assert [len(own_pixels(w, h, i, n)) for i in range(n)] == case["own"]
    assert [int(s[2].sum()) for s in shards] == case["paths"] and sum(case["paths"]) == int(whole[2].sum())
    assert [len(s[4]) for s in shards] == case["capped"] and sum(case["capped"]) == len(whole[4])
    want = WHOLE[(w, h)]
    assert (int(whole[2].sum()), len(whole[4])) == (want["paths"], want["capped"]) and len(whole[3]) == want.get("rounds", len(whole[3]))
    for k in range(len(whole[3])):                                            # per round, the shards' lists sum to the whole frame's
        assert sum(s[3][k][0] for s in shards if k < len(s[3])) == whole[3][k][0]
    live = [[a for a, _ in s[3]] for s in shards]
    if (w, h, n) == (24, 16, 3):
        assert live[0][2] == 7 and all(a <= 7 for a in live[0][2:]) and live[2][-1] == 1
    if (w, h, n) == (24, 16, 8):
        assert len(live[5]) == 23 and case["capped"][5] == 0 and live[6] == live[7] == []
        assert all(len(l) == 24 for l in live[:5])
    if (w, h) == (20, 12):
        assert [a for a, _ in whole[3]][:3] == [240, 240, 99] and whole[3][-1][0] == 32
        assert w % 8 and h % 8                                                # (partial tiles on both edges)
    if (w, h, n) == (9, 17, 5):
        assert case["own"].count(1) == 1 and sum(len(l) == 2 for l in live) == 3


def test_set_c_on_two_shards_one_needs_four_rounds_and_the_other_two():
    whole = oracle_reference(24, 16, "C")
    T.check_history("C", whole)
    shards = shard_references(24, 16, 2, "C")
    assert sorted(len(s[3]) for s in shards) == [2, 4]
    for i, s in enumerate(shards):
        assert_shard_of(s, whole, 24, 16, own_pixels(24, 16, i, 2))
    assert [bits(a) for a in ad.merge_reference([s[:3] for s in shards])] == [bits(a) for a in whole[:3]]


def test_merge_reference_keeps_every_bit_pattern():
    patterns = np.array([0x80000000, 0x7FC12345, 0xFFC00001, 0x00000001, 0x807FFFFF, 0x4B800000], np.uint32)   # -0.0, NaNs with payloads, denormals, 2^24 as a float
    mean = [np.zeros((2, 3, 4), np.float32) for _ in range(3)]
    m2 = [np.zeros((2, 3, 4), np.float32) for _ in range(3)]
    counts = [np.zeros((2, 3), np.uint32) for _ in range(3)]
    for p in range(6):                                                        # pixel p belongs to shard p % 3
        mean[p % 3].reshape(6, 4).view(np.uint32)[p] = np.roll(patterns, p)[:4]
        m2[p % 3].reshape(6, 4).view(np.uint32)[p] = np.roll(patterns, p + 2)[:4]
        counts[p % 3].reshape(6)[p] = (1 << 24, 1, 0xFFFFFFFF)[p % 3]
    got = ad.merge_reference(list(zip(mean, m2, counts)))
    assert got[0].dtype == np.float32 and got[0].shape == (2, 3, 4) and got[2].dtype == np.uint32 and got[2].shape == (2, 3)
    for p in range(6):
        assert got[0].reshape(6, 4).view(np.uint32)[p].tolist() == np.roll(patterns, p)[:4].tolist()
        assert got[1].reshape(6, 4).view(np.uint32)[p].tolist() == np.roll(patterns, p + 2)[:4].tolist()
        assert got[2].reshape(6)[p] == (1 << 24, 1, 0xFFFFFFFF)[p % 3]
    assert np.signbit(got[0].reshape(-1)[0]) and got[0].reshape(-1)[0] == 0 and np.isnan(got[0].reshape(-1)[1])
    alone = ad.merge_reference([(mean[0], m2[0], counts[0])])
    assert [bits(a) for a in alone] == [bits(mean[0]), bits(m2[0]), bits(counts[0])]


# ---------------------------------------------------------------------------------------------------- GPU
MARCH, DELTA = _lib.CT_EST_MARCH, _lib.CT_EST_DELTA
UPDATE, RAISE = "update", "raise_cap"


class Borrowed(ds.CloudTracer):
    """A CloudTracer's verbs on a handle somebody else owns (a group's shard)."""

    def __init__(self, L, h, width, height):
        self.L, self.h, self.width, self.height = L, h, width, height

    def close(self):
        self.h = None


def tracer(w, h, **kw):
    return ds.CloudTracer(T.volume(), **{**dict(width=w, height=h, mode=0), **kw})


def group(w, h, n, **kw):
    return ds.TracerGroup(T.volume(), [0] * n, **{**dict(width=w, height=h, mode=0), **kw})


def handles(g, n):
    return [Borrowed(g.L, g.handle(i), g.width, g.height) for i in range(n)]


def state(f):
    info = {k: v for k, v in f.info().items() if not k.endswith("_ms")}
    return f.mean(), f.m2(), f.counts(), info


def run(f, calls):
    """The states behind every call of `calls`: (UPDATE, rounds) or (RAISE, cap)."""
    out = []
    for verb, arg in calls:
        getattr(f, verb)(arg)
        out.append(state(f))
    return out


_WHOLE = {}


def whole_frame(w, h, calls=((UPDATE, 0),), name="A", tracer_kw=(), **params):
    """The whole-frame ct_adaptive_frame on an unsharded handle driven by `calls`, once per key: -> the states, the paths counted."""
    key = (w, h, tuple(calls), name, tuple(tracer_kw), tuple(sorted(params.items())))
    if key not in _WHOLE:
        with tracer(w, h, mode=T.SETS[name]["mode"], **dict(tracer_kw)) as tr:
            before = tr.counters()["paths"]
            with tr.adaptive_frame(**T.params_of(name, **params)) as f:
                states = run(f, calls)
            _WHOLE[key] = states, tr.counters()["paths"] - before
    return _WHOLE[key]


def assert_same_frame(got, want):
    for a, b in zip(got[:3], want[:3]):
        assert bits(a) == bits(b)
    assert got[3] == want[3]


def shard_states(w, h, n, calls=((UPDATE, 0),), name="A", tracer_kw=(), **params):
    """Every shard's frame from ct_adaptive_frame_create_shard on a sharded handle of its own, driven by `calls`: -> per shard the
    last state and the handle's paths delta."""
    out = []
    for i in range(n):
        with tracer(w, h, mode=T.SETS[name]["mode"], shard_index=i, shard_count=n, **dict(tracer_kw)) as tr:
            before = tr.counters()["paths"]
            with tr.adaptive_frame(shard=True, **T.params_of(name, **params)) as f:
                last = run(f, calls)[-1]
            out.append((last, tr.counters()["paths"] - before))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("w, h, n", list(CASES), ids=CASE_IDS)
def test_shard_frames_are_the_whole_frame_on_their_own_pixels(w, h, n):
    case = CASES[(w, h, n)]
    (whole,), whole_paths = whole_frame(w, h)
    if (w, h, n) == (24, 16, 3):                                              # the chain to the uniform images, in this file too
        ref = T.gpu_reference("A")
        T.check_history("A", ref)
        assert [bits(a) for a in whole[:3]] == [bits(a) for a in ref[:3]]
    shards = shard_states(w, h, n)
    for i, (s, paths) in enumerate(shards):
        own = own_pixels(w, h, i, n)
        assert_shard_of(s, whole, w, h, own)
        info = s[3]
        assert (info["width"], info["height"], info["pixels"], info["max_samples"]) == (w, h, case["own"][i], 96)
        assert (info["paths"], info["capped"], info["live"]) == (case["paths"][i], case["capped"][i], 0)
        assert info["converged"] == case["own"][i] - case["capped"][i] and info["rounds"] == rounds_of(whole[2], own)
        assert paths == info["paths"] == int(s[2].sum())
    total = {k: sum(s[3][k] for s, _ in shards) for k in ("pixels", "live", "converged", "capped", "paths")}
    assert total == {k: whole[3][k] for k in total} and sum(p for _, p in shards) == whole_paths
    assert max(s[3]["rounds"] for s, _ in shards) == whole[3]["rounds"]
    merged = ad.merge_reference([s[:3] for s, _ in shards])
    assert [bits(a) for a in merged] == [bits(a) for a in whole[:3]]


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, _lib.CT_FLAG_TEX_FIXED8], ids=["plain", "fixed8"])
@pytest.mark.parametrize("estimator", [MARCH, DELTA], ids=["march", "delta"])
def test_shards_equal_the_whole_frame_on_both_estimators_and_with_fixed8(estimator, flags):
    kw = (("estimator", estimator), ("flags", flags))
    (whole,), whole_paths = whole_frame(24, 16, tracer_kw=kw)
    assert 0 < whole[3]["converged"] < 384
    shards = shard_states(24, 16, 3, tracer_kw=kw)
    for i, (s, _) in enumerate(shards):
        assert_shard_of(s, whole, 24, 16, own_pixels(24, 16, i, 3))
    assert sum(p for _, p in shards) == whole_paths == whole[3]["paths"]


@pytest.mark.gpu
@pytest.mark.parametrize("w, h, n", list(CASES), ids=CASE_IDS)
def test_the_first_live_list_is_the_shards_own_pixels(w, h, n):
    """Through update(1)'s counts: exactly the own pixels hold R, all others 0 -- and so do mean and M2 hold nothing elsewhere."""
    for i, (s, paths) in enumerate(shard_states(w, h, n, calls=((UPDATE, 1),))):
        own = own_pixels(w, h, i, n)
        want = np.zeros(w * h, np.uint32)
        want[own] = R
        assert bits(s[2]) == bits(want)
        assert not s[0].reshape(w * h, 4)[want == 0].view(np.uint32).any() and not s[1].reshape(w * h, 4)[want == 0].view(np.uint32).any()
        assert (s[3]["pixels"], s[3]["live"], s[3]["rounds"], s[3]["paths"]) == (len(own), len(own), 1 if len(own) else 0, R * len(own))
        assert paths == R * len(own)


GROUPS = [(24, 16, 1), (24, 16, 2), (24, 16, 3), (24, 16, 8), (9, 17, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("w, h, n", GROUPS, ids=[f"{w}x{h}-{n}" for w, h, n in GROUPS])
def test_a_group_frame_is_the_whole_frame_after_the_same_calls(w, h, n):
    calls = ((UPDATE, 3), (UPDATE, 0))
    want, _ = whole_frame(w, h, calls)
    with group(w, h, n) as g, g.adaptive_frame(**T.params_of("A")) as gf:
        first = state(gf)                                                     # before any round: everything live, nothing held
        assert first[3]["pixels"] == first[3]["live"] == w * h and not first[2].any() and first[3]["rounds"] == 0
        for got, ref in zip(run(gf, calls), want):
            assert_same_frame(got, ref)
        hs = handles(g, n)
        launches = [t.kernel_time()[2] for t in hs]
        counters = g.counters()
        assert counters["paths"] == want[-1][3]["paths"]
        gf.update()                                                           # finished: CT_OK, nothing launched
        gf.update(2)
        assert_same_frame(state(gf), want[-1])
        assert [t.kernel_time()[2] for t in hs] == launches and g.counters() == counters
        for i in range(n):                                                    # ... and shard(i) is that shard's frame
            s = gf.shard(i)
            assert s.info()["pixels"] == len(own_pixels(w, h, i, n))
            assert_shard_of((s.mean(), s.m2(), s.counts()), want[-1], w, h, own_pixels(w, h, i, n))
    calls = ((UPDATE, 0), (RAISE, 96), (UPDATE, 0))
    want, _ = whole_frame(w, h, calls, max_samples=48)
    assert want[0][3]["capped"] > 0 and want[1][3]["live"] == want[0][3]["capped"] and want[1][3]["max_samples"] == 96
    with group(w, h, n) as g, g.adaptive_frame(**T.params_of("A", max_samples=48)) as gf:
        for got, ref in zip(run(gf, calls), want):
            assert_same_frame(got, ref)
    assert_same_frame(want[-1], whole_frame(w, h)[0][-1])                     # the higher cap's frame, as f-16 promises


@pytest.mark.gpu
def test_chunks_and_passes_do_not_change_a_groups_bits():
    (want,), _ = whole_frame(24, 16)
    with group(24, 16, 3) as g, g.adaptive_frame(**T.params_of("A", chunk_pixels=64, pass_subframes=1)) as gf:
        gf.update()
        assert_same_frame(state(gf), want)
        assert handles(g, 3)[1].kernel_time()[2] >= 2 * 4 + 23                # shard 1, round 1: 128 pixels in 2 chunks, 4 passes


@pytest.mark.gpu
def test_tonemap_buffer_takes_the_merged_mean():
    calls = ((UPDATE, 6),)
    with tracer(24, 16) as tr, tr.adaptive_frame(**T.params_of("A")) as f:
        f.update(6)
        want, want_avg = f.tonemap(0.4)
    with group(24, 16, 3) as g, g.adaptive_frame(**T.params_of("A")) as gf:
        gf.update(6)
        screen, avg = gf.tonemap(0.4)
        assert bits(screen) == bits(want) and avg == want_avg and screen[..., :3].any()
        again, _ = handles(g, 3)[0].tonemap_buffer(gf.device_ptr(), 0.4)
        assert bits(again) == bits(want)
        ptrs = [gf.device_ptr(k) for k in (_lib.CT_ADAPTIVE_MEAN, _lib.CT_ADAPTIVE_M2, _lib.CT_ADAPTIVE_COUNTS)]
        assert ptrs[1] - ptrs[0] == 24 * 16 * 16 and ptrs[2] - ptrs[1] == 24 * 16 * 16    # [mean | M2 | counts]
        assert_same_frame(state(gf), whole_frame(24, 16, calls)[0][0])


@pytest.mark.gpu
def test_the_groups_image_is_left_alone():
    with group(24, 16, 3) as g, tracer(24, 16) as fresh:
        g.render_accumulate(1, 2)
        before = (g.mean(), g.m2())
        with g.adaptive_frame(**T.params_of("A")) as gf:
            assert gf.update(4)["rounds"] == 4
            gf.merge()
            after = (g.mean(), g.m2())
        assert [bits(a) for a in before] == [bits(a) for a in after] and before[0].any()
        g.render_accumulate(3, 2)                                             # ... and the render goes on to an unsharded handle's bits
        g.merge()
        fresh.render_accumulate(1, 4)
        assert bits(g.mean()) == bits(fresh.mean()) and bits(g.m2()) == bits(fresh.m2())


def _code(call):
    with pytest.raises(_lib.CloudTraceError) as e:
        call()
    return e.value.code, e.value.message


@pytest.mark.gpu
@pytest.mark.parametrize("change", ["camera", "light"])
def test_a_new_pose_or_light_is_a_state_error_and_download_still_works(change):
    with group(24, 16, 3) as g, g.adaptive_frame(**T.params_of("A", max_samples=8)) as gf:
        gf.update(2)
        before = state(gf)
        assert before[3]["capped"] > 0
        if change == "camera":
            other = (2.0, 0.3, 0.5)
            g.set_camera(other, *ds.calculate_camera_variables(other, (0, 0, 0), (0, 1, 0), 30.0, 24 / 16))
        else:
            g.set_light((0.3, -0.8, 0.2))
        for call in (lambda: gf.update(), lambda: gf.raise_cap(16)):
            code, message = _code(call)
            assert code == _lib.CT_E_STATE and change in message and "shard 0" in message
        assert_same_frame(state(gf), before)
        assert gf.device_ptr() != 0
        g.render_accumulate(1, 1)                                             # the group stays usable


@pytest.mark.gpu
def test_argument_errors_leave_the_group_and_the_frames_as_they_were():
    with group(24, 16, 3) as g, g.adaptive_frame(**T.params_of("A")) as gf:
        gf.update(3)
        L = g.L
        before, counters, allocations = state(gf), g.counters(), ct.debug_allocations()

        def message():
            return L.ct_group_last_error(g.g).decode()

        out, info = C.c_void_p(1), _lib.CtAdaptiveFrameInfo()
        desc = _lib.CtAdaptiveFrameDesc(_lib.CT_ABI_VERSION, 4, 8, 96, 0.7, 1e-2, 0, 0)
        assert L.ct_group_adaptive_frame_create(g.g, None, C.byref(out)) == _lib.CT_E_INVAL and not out.value
        assert L.ct_group_adaptive_frame_create(g.g, C.byref(desc), None) == _lib.CT_E_INVAL
        for field, value, word in (("abi_version", _lib.CT_ABI_VERSION + 1, "abi_version"), ("round_samples", 0, "round_samples"),
                                   ("max_samples", 98, "max_samples"), ("min_samples", 6, "min_samples"), ("rel_tol", -1.0, "rel_tol"),
                                   ("chunk_pixels", 96, "chunk_pixels"), ("pass_subframes", 5, "pass_subframes")):
            bad = _lib.CtAdaptiveFrameDesc(_lib.CT_ABI_VERSION, 4, 8, 96, 0.7, 1e-2, 0, 0)
            setattr(bad, field, value)
            out = C.c_void_p(1)
            assert L.ct_group_adaptive_frame_create(g.g, C.byref(bad), C.byref(out)) == _lib.CT_E_INVAL and not out.value
            assert word in message() and "shard 0" in message() and "ct_adaptive_frame_create_shard" in message()
        for cap in (44, 96, 98, 2 ** 24 + 4):                                 # lower, equal, no multiple of R, too high
            code, text = _code(lambda: gf.raise_cap(cap))
            assert code == _lib.CT_E_INVAL and "max_samples" in text
        assert L.ct_group_adaptive_frame_info(gf.gf, None) == _lib.CT_E_INVAL
        for index in (3, 4, 2 ** 32 - 1):
            assert L.ct_group_adaptive_frame_shard(gf.gf, index, C.byref(out)) == _lib.CT_E_INVAL
        assert L.ct_group_adaptive_frame_shard(gf.gf, 0, None) == _lib.CT_E_INVAL
        assert L.ct_group_adaptive_frame_device_ptr(gf.gf, 3, C.byref(out)) == _lib.CT_E_INVAL
        assert L.ct_group_adaptive_frame_device_ptr(gf.gf, 0, None) == _lib.CT_E_INVAL
        buf = np.zeros(384 * 4 + 1, np.float32)
        for which, nbytes in ((3, 384 * 16), (0, 384 * 16 - 4), (0, 384 * 16 + 4), (2, 384 * 16), (1, 0)):
            assert L.ct_group_adaptive_frame_download(gf.gf, which, buf.ctypes.data_as(C.c_void_p), nbytes) == _lib.CT_E_INVAL
            assert "ct_group_adaptive_frame_download" in message()
        assert L.ct_group_adaptive_frame_download(gf.gf, 0, None, 384 * 16) == _lib.CT_E_INVAL
        assert not buf.any() and ct.debug_allocations() == allocations
        assert_same_frame(state(gf), before)
        assert g.counters() == counters
        gf.update()                                                           # ... and the frame goes on to what set A gives
        assert_same_frame(state(gf), whole_frame(24, 16)[0][0])
    with group(24, 16, 2, flags=_lib.CT_FLAG_SIMPLE_KERNEL) as simple:
        code, text = _code(lambda: simple.adaptive_frame(**T.params_of("A")))
        assert code == _lib.CT_E_INVAL and "persistent kernel" in text
        simple.render_accumulate(1, 1)                                        # ... which stays usable
    with tracer(24, 16, shard_index=1, shard_count=2) as shard:               # the whole-frame create keeps refusing a shard
        code, text = _code(lambda: shard.adaptive_frame(**T.params_of("A")))
        assert code == _lib.CT_E_INVAL and "shard 1 of 2" in text


@pytest.mark.gpu
def test_every_allocation_is_given_back():
    start = ct.debug_allocations()
    with tracer(24, 16, shard_index=1, shard_count=3) as tr:
        held = ct.debug_allocations()
        with tr.adaptive_frame(shard=True, **T.params_of("A")) as f:
            inside = ct.debug_allocations()
            # mean, M2, counts, the wave counts of the frame's pixels, two live lists of the 128 own pixels
            assert inside["device_buffers"] == held["device_buffers"] + 6
            assert inside["device_bytes"] == held["device_bytes"] + 384 * 36 + (384 // 64 + 1) * 4 + 2 * 128 * 4
            f.update()                                                        # (the handle's point buffers grow here, and stay with it)
        assert ct.debug_allocations()["device_bytes"] >= held["device_bytes"]
    assert ct.debug_allocations() == start
    with tracer(24, 16, shard_index=7, shard_count=8) as tr:                  # a shard that owns nothing has no lists
        held = ct.debug_allocations()
        with tr.adaptive_frame(shard=True, **T.params_of("A")) as f:
            assert ct.debug_allocations()["device_buffers"] == held["device_buffers"] + 4
            assert f.update()["pixels"] == 0
        assert ct.debug_allocations() == held
    assert ct.debug_allocations() == start
    with group(24, 16, 3) as g:
        held = ct.debug_allocations()
        with g.adaptive_frame(**T.params_of("A")) as gf:
            inside = ct.debug_allocations()
            assert inside["device_buffers"] == held["device_buffers"] + 3 * 6 + 3 + 1     # + a staging buffer per shard and the landing buffer
            gf.update(2)
            gf.merge()
        other = (2.0, 0.3, 0.5)                                               # a create whose second shard fails: its handle alone was moved
        pose = [np.asarray(v, np.float32) for v in (other, *ds.calculate_camera_variables(other, (0, 0, 0), (0, 1, 0), 30.0, 24 / 16))]
        h1 = g.handle(1)
        assert g.L.ct_set_camera(h1, *[v.ctypes.data_as(C.c_void_p) for v in pose]) == _lib.CT_OK
        held = ct.debug_allocations()
        code, text = _code(lambda: g.adaptive_frame(**T.params_of("A")))
        assert code == _lib.CT_E_STATE and "shard 1" in text
        assert ct.debug_allocations() == held
        g.render_accumulate(1, 1)                                             # the group is left as it was
    assert ct.debug_allocations() == start


@pytest.mark.gpu
def test_the_armed_invariants_report_no_violation_over_set_a_on_a_group(monkeypatch):
    monkeypatch.setenv("CT_DEBUG_INVARIANTS", "1")
    (want,), _ = whole_frame(24, 16)
    with group(24, 16, 3) as g, g.adaptive_frame(**T.params_of("A")) as gf:
        gf.update()
        assert_same_frame(state(gf), want)
        for i, t in enumerate(handles(g, 3)):
            iv = t.debug_invariants()
            assert iv["armed"] == 1 and iv["checks"] > 0 and iv["violations"] == 0 and iv["samples_without_alpha_1"] == 0
            assert iv["dealt"] == iv["written"] == CASES[(24, 16, 3)]["paths"][i]


@pytest.mark.gpu
def test_cli_adaptive_gpus_writes_the_python_whole_frame_paths_files(tmp_path):
    from deepestscatter_amd import build
    cli = build.build_cli()
    w, h = 24, 16
    counts_file = tmp_path / "counts.u32"
    r = subprocess.run([str(cli), "procedural:32", "--size", f"{w}x{h}", "--light", "Side", "--out", str(tmp_path),
                        "--adaptive", "4,96,8,0.7,0.01", "--adaptive-gpus", "0,0,0", "--adaptive-counts", str(counts_file)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with ds.CloudTracer(ds.make_procedural_cloud(32), width=w, height=h, mode=0, light_direction=ds.LIGHT_DIRECTIONS["Side"]) as tr, \
            tr.adaptive_frame(**T.params_of("A")) as f:
        info = f.update()
        mean, counts = f.mean(), f.counts()
    assert 0 < info["converged"] < w * h
    assert (f'adaptive {{"rounds": {info["rounds"]}, "pixels": {w * h}, "converged": {info["converged"]}, "capped": {info["capped"]}, '
            f'"paths": {info["paths"]}}}') in r.stdout
    assert np.fromfile(counts_file, "<u4").tobytes() == counts.tobytes()
    rgb = exr.read_exr(tmp_path / "procedural_32.Side.PT.exr")
    assert rgb.shape == (h, w, 3) and rgb.tobytes() == np.ascontiguousarray(mean[..., :3]).tobytes()
    for args in (["--adaptive-gpus", "0,0"], ["--adaptive", "4,96", "--adaptive-gpus", "2", "--display"],
                 ["--adaptive", "4,96", "--adaptive-gpus", "2", "--network", "none.bin"],
                 ["--adaptive", "4,96", "--adaptive-gpus", "2", "--traced-bake", "4,4,4,4,2", "--bake-samples", "4"]):
        r = subprocess.run([str(cli), "procedural:32", *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--adaptive" in r.stdout
