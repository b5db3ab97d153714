"""ct_adaptive_frame_*: the progressive image with the stopping rule applied per pixel (include/cloudtrace.h, "the adaptive
frame").

Everything is held bit for bit (tobytes()) to adaptive.adaptive_frame_reference -- the loop over uniform images -- over the CPU
oracle (the CPU tests) or over a second handle of the same scene stepped with ct_render_accumulate (the GPU tests).

Scene: conftest.sphere_volume(32, seed=12), a 24 x 16 frame (384 pixels, six waves), default camera and light.  Parameter sets
(histories as the reference gives them on the oracle with fast=True):
  A  mode 0, R = 4, min 8, cap 96, rel 0.7, abs 1e-2: 24 rounds, live 384, 384, 135, 124, .. 42, 42, 41; pixels leave in all but
     rounds 1 and 22, the live count is never again a multiple of 64 and below one wave from round 15 on, 249 pixels leave at the
     first tested count, 40 end capped, the counts sum to 9520
  C  set A with mode 2 and rel 0.5: history (384, 0), (384, 383), (1, 0), (1, 1): one pixel is live in rounds 3 and 4, the frame
     completes in round 4, the counts sum to 3080"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import _oracle as O
import deepestscatter_amd as ds
from deepestscatter_amd import _lib
from deepestscatter_amd import adaptive as ad
from deepestscatter_amd import cloudtrace as ct
from deepestscatter_amd import exr
from conftest import sphere_volume

W, H = 24, 16
SETS = {
    "A": dict(mode=0, round_samples=4, min_samples=8, max_samples=96, rel_tol=0.7, abs_tol=1e-2),
    "C": dict(mode=2, round_samples=4, min_samples=8, max_samples=96, rel_tol=0.5, abs_tol=1e-2),
}
LIVE_A = [384, 384, 135, 124, 114, 105, 98, 95, 88, 79, 75, 70, 67, 65, 62, 58, 55, 54, 50, 47, 46, 42, 42, 41]
HISTORY_C = [(384, 0), (384, 383), (1, 0), (1, 1)]


def volume():
    return sphere_volume(32, seed=12)


def params_of(name, **kw):
    p = {k: v for k, v in SETS[name].items() if k != "mode"}
    p.update(kw)
    return p


def check_history(name, ref, cap=96):
    """The conditions the parameter sets were chosen for, on the REFERENCE's run: a device run is compared with it afterwards."""
    mean, m2, counts, history, capped = ref
    live = [n for n, _ in history]
    assert live[0] == W * H and all(a - left == b for (a, left), b in zip(history, live[1:]))
    assert counts.sum() == 4 * sum(live) and counts.min() >= 8
    if name == "A" and cap == 96:
        assert live == LIVE_A and len(history) == 24
        assert [k + 1 for k, (_, left) in enumerate(history) if not left] == [1, 22]
        assert all(n % 64 for n in live[2:]) and all(n < 64 for n in live[14:]) and live[13] >= 64
        assert history[1][1] == 249 and len(capped) == 40 and counts.sum() == 9520
        assert (counts == 96).sum() == 41 and history[-1] == (41, 41)         # one pixel passes at the cap itself
    elif name == "A":
        assert cap == 48 and live == LIVE_A[:12] and len(capped) == 67 and history[-1][0] == 70
    elif name == "C":
        assert history == HISTORY_C and len(capped) == 0 and counts.sum() == 3080 and 1 in live
        assert counts.max() == 16 and (counts == 16).sum() == 1


class Stepper:
    """snapshot(c) of adaptive_frame_reference over something that renders and accumulates the subframes first .. first + n - 1
    of the whole frame: step(first, n) -> (mean, m2).  Asked with ascending c."""

    def __init__(self, step):
        self.step, self.done, self.state = step, 0, None

    def __call__(self, c):
        assert c > self.done
        self.state = self.step(self.done + 1, c - self.done)
        self.done = c
        return self.state


# ---------------------------------------------------------------------------------------------------- CPU
_ORACLE_RUNS = {}


def oracle_run(name):
    if name not in _ORACLE_RUNS:
        orc = O.Oracle(volume(), W, H, mode=SETS[name]["mode"], fast=True)
        mean, m2 = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)

        def step(first, n):
            for s in range(first, first + n):
                O.accumulate(orc.render_subframe(s), mean, m2, s)
            return mean.copy(), m2.copy()

        _ORACLE_RUNS[name] = ad.adaptive_frame_reference(Stepper(step), W, H, **params_of(name))
    return _ORACLE_RUNS[name]


NAMES = ("ct_adaptive_frame_create", "ct_adaptive_frame_update", "ct_adaptive_frame_raise_cap", "ct_adaptive_frame_info",
         "ct_adaptive_frame_download", "ct_adaptive_frame_device_ptr", "ct_adaptive_frame_destroy")


def test_symbols_resolve_and_answer_null_arguments(product_lib):
    L = product_lib
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.EXPORTS
    d = _lib.CtAdaptiveFrameDesc(_lib.CT_ABI_VERSION, 4, 8, 96, 0.1, 0.1, 0, 0)
    out, info = C.c_void_p(), _lib.CtAdaptiveFrameInfo()
    assert L.ct_adaptive_frame_create(None, C.byref(d), C.byref(out)) == _lib.CT_E_INVAL
    assert L.ct_adaptive_frame_update(None, 1) == _lib.CT_E_INVAL
    assert L.ct_adaptive_frame_raise_cap(None, 100) == _lib.CT_E_INVAL
    assert L.ct_adaptive_frame_info(None, C.byref(info)) == _lib.CT_E_INVAL
    assert L.ct_adaptive_frame_download(None, 0, None, 0) == _lib.CT_E_INVAL
    assert L.ct_adaptive_frame_device_ptr(None, 0, C.byref(out)) == _lib.CT_E_INVAL
    assert L.ct_adaptive_frame_destroy(None) == _lib.CT_OK
    assert (_lib.CT_ADAPTIVE_MEAN, _lib.CT_ADAPTIVE_M2, _lib.CT_ADAPTIVE_COUNTS) == (0, 1, 2)


def test_struct_layout_matches_the_header():
    import tempfile
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    desc = ["abi_version", "round_samples", "min_samples", "max_samples", "rel_tol", "abs_tol", "chunk_pixels", "pass_subframes"]
    info = ["width", "height", "round_samples", "min_samples", "max_samples", "rounds", "rel_tol", "abs_tol", "pixels", "live", "converged",
            "capped", "paths", "trace_ms", "fold_ms", "test_ms"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "cloudtrace.h"\nint main(){printf("%zu %zu %d %d %d", sizeof(CtAdaptiveFrameDesc), '
           'sizeof(CtAdaptiveFrameInfo), CT_ADAPTIVE_MEAN, CT_ADAPTIVE_M2, CT_ADAPTIVE_COUNTS);'
           + "".join(f'printf(" %zu", offsetof(CtAdaptiveFrameDesc, {f}));' for f in desc)
           + "".join(f'printf(" %zu", offsetof(CtAdaptiveFrameInfo, {f}));' for f in info) + "return 0;}")
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "p.c").write_text(src)
        subprocess.run(["gcc", "-I", str(root / "include"), "-o", f"{d}/p", f"{d}/p.c"], check=True)
        out = [int(v) for v in subprocess.run([f"{d}/p"], capture_output=True, text=True, check=True).stdout.split()]
    assert out[:2] == [32, 96] == [C.sizeof(_lib.CtAdaptiveFrameDesc), C.sizeof(_lib.CtAdaptiveFrameInfo)]
    assert out[2:5] == [0, 1, 2]
    assert out[5:13] == [getattr(_lib.CtAdaptiveFrameDesc, f).offset for f in desc] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert out[13:] == [getattr(_lib.CtAdaptiveFrameInfo, f).offset for f in info] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64, 72, 80, 88]


def test_pixel_rule_with_the_references_constants_is_is_converged():
    """pixel_converged_reference(.., 2e-2, 1e-2) fails exactly the pixels Camera::isConverged counts, on oracle images of 100
    and 108 subframes, and on made-up statistics with zeros, a negative mean and NaNs."""
    orc = O.Oracle(volume(), W, H, mode=0, fast=True)
    mean, m2 = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
    seen = set()
    for s in range(1, 109):                                                   # (Camera::isConverged tests nothing below 100)
        O.accumulate(orc.render_subframe(s), mean, m2, s)
        if s in (100, 108):
            bad = int((~ad.pixel_converged_reference(mean[..., 0], m2[..., 0], s, 2e-2, 1e-2)).sum())
            assert bad == O.is_converged(mean, m2, s)[1]
            seen.add(bad)
    assert all(0 < b < W * H for b in seen)
    rng = np.random.default_rng(3)
    mean = (rng.random((8, 8, 4), dtype=np.float32) - 0.1) * 5
    m2 = rng.random((8, 8, 4), dtype=np.float32) * 40
    mean[0, :4, 0], m2[1, :4, 0], m2[2, 0, 0], mean[2, 1, 0] = 0, 0, np.nan, np.nan
    bad = int((~ad.pixel_converged_reference(mean[..., 0], m2[..., 0], 100, 2e-2, 1e-2)).sum())
    assert bad == O.is_converged(mean, m2, 100)[1] and 2 <= bad < 64


@pytest.mark.parametrize("name", ["A", "C"])
def test_the_parameter_sets_have_the_histories_they_were_chosen_for(name):
    ref = oracle_run(name)
    check_history(name, ref)
    mean, m2, counts, history, capped = ref
    p = SETS[name]
    failing = ~ad.pixel_converged_reference(mean[..., 0], m2[..., 0], 96, p["rel_tol"], p["abs_tol"]).reshape(-1)
    assert sorted(capped) == sorted(np.flatnonzero((counts.reshape(-1) == 96) & failing))
    if name == "A":                                                           # 74 % of the uniform 96-spp job's paths are saved
        assert 0.74 <= 1 - counts.sum() / (96 * W * H) < 0.75


def test_a_run_cut_into_rounds_is_the_start_of_the_whole_run():
    whole = oracle_run("C")
    orc = O.Oracle(volume(), W, H, mode=2, fast=True)
    mean, m2, counts, history, capped = ad.adaptive_frame_reference(
        Stepper(lambda first, n: orc.render(first + n - 1)), W, H, rounds=2, **params_of("C"))
    assert history == HISTORY_C[:2] and (counts == 8).all()
    left = whole[2] == 8
    assert left.sum() == 383 and mean[left].tobytes() == whole[0][left].tobytes() and m2[left].tobytes() == whole[1][left].tobytes()


def test_the_python_layer_refuses_contradicting_arguments():
    ok = dict(round_samples=4, max_samples=96, min_samples=8, rel_tol=0.1, abs_tol=0.1)
    ad.check_params(**ok)
    for kw in (dict(round_samples=0), dict(round_samples=65536), dict(max_samples=98), dict(max_samples=2 ** 24 + 4), dict(max_samples=0),
               dict(min_samples=6), dict(min_samples=100), dict(min_samples=0), dict(rel_tol=-1.0), dict(rel_tol=float("nan")),
               dict(abs_tol=float("inf")), dict(chunk_pixels=96), dict(chunk_pixels=-64), dict(pass_subframes=5), dict(pass_subframes=-1)):
        with pytest.raises(ValueError):
            ad.check_params(**{**ok, **kw})
    with pytest.raises(ValueError):                                           # before anything of the tracer is touched
        ad.AdaptiveFrame(None, round_samples=4, max_samples=98, min_samples=8)
    with pytest.raises(ValueError):
        ad.adaptive_frame_reference(lambda c: None, W, H, round_samples=4, max_samples=96, min_samples=7, rel_tol=0.1, abs_tol=0.1)


# ---------------------------------------------------------------------------------------------------- GPU
MARCH, DELTA = _lib.CT_EST_MARCH, _lib.CT_EST_DELTA
_GPU_RUNS = {}


def tracer(**kw):
    return ds.CloudTracer(volume(), **{**dict(width=W, height=H, mode=0), **kw})


def gpu_reference(name, **kw):
    """adaptive_frame_reference over a handle of its own that is stepped with ct_render_accumulate(.., R) and downloaded after
    every round, once per (set, parameters): -> (mean, m2, counts, history, capped)."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _GPU_RUNS:
        with tracer(mode=SETS[name]["mode"]) as tr:
            def step(first, n):
                tr.render_accumulate(first, n)
                return tr.mean(), tr.m2()
            _GPU_RUNS[key] = ad.adaptive_frame_reference(Stepper(step), W, H, **params_of(name, **kw))
    return _GPU_RUNS[key]


def assert_equals_reference(f, ref, cap=96, W=W, H=H):
    mean, m2, counts, history, capped = ref
    assert f.counts().tobytes() == counts.tobytes()
    assert f.mean().tobytes() == mean.tobytes()
    assert f.m2().tobytes() == m2.tobytes()
    info = f.info()
    at_cap = bool(history) and history[-1][0] > 0 and counts.max() == cap
    live = 0 if at_cap or not history else history[-1][0] - history[-1][1]
    assert (info["width"], info["height"], info["pixels"], info["rounds"]) == (W, H, W * H, len(history))
    assert (info["live"], info["capped"], info["converged"]) == (live, len(capped), W * H - live - len(capped))
    assert info["paths"] == int(counts.sum()) and info["max_samples"] == cap


def device_run(tr, name, split=(0,), **kw):
    f = tr.adaptive_frame(**params_of(name, **kw))
    for k in split:
        f.update(k)
    return f


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, _lib.CT_FLAG_TEX_FIXED8], ids=["plain", "fixed8"])
@pytest.mark.parametrize("estimator", [MARCH, DELTA], ids=["march", "delta"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_path_equality_every_pixel_is_the_uniform_images(mode, estimator, flags):
    """rel 0, abs 0: nothing converges, every count is the cap, and the frame is the uniform handle's after 12 subframes."""
    kw = dict(mode=mode, estimator=estimator, flags=flags)
    with tracer(**kw) as uniform:
        uniform.render_accumulate(1, 12)
        mean, m2, paths = uniform.mean(), uniform.m2(), uniform.counters()["paths"]
    assert mean[..., 0].any() and paths == 12 * W * H
    with tracer(**kw) as tr, tr.adaptive_frame(round_samples=4, max_samples=12, min_samples=4, rel_tol=0.0, abs_tol=0.0) as f:
        info = f.update()
        assert (f.counts() == 12).all()
        assert f.mean().tobytes() == mean.tobytes()
        assert f.m2().tobytes() == m2.tobytes()
        assert (info["rounds"], info["live"], info["converged"], info["capped"], info["paths"]) == (3, 0, 0, W * H, 12 * W * H)
        assert tr.counters()["paths"] == paths


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "C"])
def test_adaptive_frame_equals_the_loop_over_uniform_images(name):
    ref = gpu_reference(name)
    check_history(name, ref)
    with tracer(mode=SETS[name]["mode"]) as tr:
        before = tr.counters()["paths"]
        with device_run(tr, name) as f:
            assert_equals_reference(f, ref)
            assert tr.counters()["paths"] - before == int(ref[2].sum())


@pytest.mark.gpu
def test_the_split_of_rounds_over_calls_does_not_matter_and_a_finished_frame_launches_nothing():
    ref = gpu_reference("A")
    check_history("A", ref)
    with tracer() as tr, device_run(tr, "A", split=(5, 7, 0)) as f:
        assert_equals_reference(f, ref)
    with tracer() as tr, device_run(tr, "A", split=(5,)) as f:                # ... and a run stopped early is the reference's start
        assert_equals_reference(f, gpu_reference("A", rounds=5))
    ref = gpu_reference("C")
    check_history("C", ref)
    with tracer(mode=2) as tr, device_run(tr, "C", split=(3, 100)) as f:      # stops at completion, in round 4
        assert_equals_reference(f, ref)
        counters, launches = tr.counters(), tr.kernel_time()
        f.update()                                                            # CT_OK, nothing launched
        f.update(3)
        assert_equals_reference(f, ref)
        assert tr.counters() == counters and tr.kernel_time() == launches


@pytest.mark.gpu
@pytest.mark.parametrize("chunk_pixels, pass_subframes", [(64, 1), (128, 3)])
def test_chunks_and_passes_do_not_change_the_bits(chunk_pixels, pass_subframes):
    ref = gpu_reference("A")
    check_history("A", ref)
    with tracer() as tr, device_run(tr, "A", chunk_pixels=chunk_pixels, pass_subframes=pass_subframes) as f:
        assert_equals_reference(f, ref)
        # round 1: 384 pixels in chunks of chunk_pixels, 4 subframes in passes of pass_subframes, one estimator launch each
        assert tr.kernel_time()[2] >= (384 // chunk_pixels) * -(-4 // pass_subframes) + 23


@pytest.mark.gpu
def test_raise_cap_continues_to_the_bits_of_the_higher_cap():
    low = gpu_reference("A", max_samples=48)
    check_history("A", low, cap=48)
    ref = gpu_reference("A")
    check_history("A", ref)
    with tracer() as tr, device_run(tr, "A", max_samples=48) as f:
        assert_equals_reference(f, low, cap=48)
        assert f.info()["capped"] == 67
        for cap in (44, 48, 50, 2 ** 24 + 4):                                 # lower, equal, no multiple of R, too high
            with pytest.raises(_lib.CloudTraceError) as e:
                f.raise_cap(cap)
            assert e.value.code == _lib.CT_E_INVAL and "max_samples" in e.value.message
        assert_equals_reference(f, low, cap=48)
        f.raise_cap(96)
        assert (f.info()["live"], f.info()["capped"], f.info()["max_samples"]) == (67, 0, 96)
        f.update()
        assert_equals_reference(f, ref)


@pytest.mark.gpu
def test_tonemap_buffer_works_on_the_adaptive_mean():
    import torch
    with tracer() as tr, device_run(tr, "A", split=(6,)) as f:
        mean = f.mean()
        screen, avg = f.tonemap(0.4)
        up = torch.from_numpy(mean).cuda()
        torch.cuda.synchronize()
        want, want_avg = tr.tonemap_buffer(up.data_ptr(), 0.4)
        assert screen.tobytes() == want.tobytes() and avg == want_avg and screen[..., :3].any()
        assert f.device_ptr(_lib.CT_ADAPTIVE_M2) != f.device_ptr() != f.device_ptr(_lib.CT_ADAPTIVE_COUNTS)


@pytest.mark.gpu
def test_the_handles_image_is_left_alone():
    with tracer() as tr, tracer() as fresh:
        tr.render_accumulate(1, 2)
        before = (tr.mean(), tr.m2(), tr.frame(), tr.subframes, tr.rendered_subframes())
        with device_run(tr, "A", split=(4,)) as f:
            assert f.info()["rounds"] == 4
            after = (tr.mean(), tr.m2(), tr.frame(), tr.subframes, tr.rendered_subframes())
        for x, y in zip(before[:3], after[:3]):
            assert x.tobytes() == y.tobytes()
        assert before[0].any() and before[3:] == after[3:] == (2, 2)
        tr.render_accumulate(3, 2)                                            # ... and the render goes on to a fresh handle's bits
        fresh.render_accumulate(1, 4)
        assert tr.subframes == 4 and tr.mean().tobytes() == fresh.mean().tobytes() and tr.m2().tobytes() == fresh.m2().tobytes()


def _state(f):
    return (f.mean().tobytes(), f.m2().tobytes(), f.counts().tobytes(), {k: v for k, v in f.info().items() if not k.endswith("_ms")})


@pytest.mark.gpu
def test_a_new_pose_or_light_is_a_state_error_and_download_still_works():
    eye = (2.5, -0.4, 0.0)
    same = ds.calculate_camera_variables(eye, (0, 0, 0), (0, 1, 0), 30.0, W / H)
    for change in ("camera", "light"):
        with tracer() as tr, device_run(tr, "A", split=(2,), max_samples=8) as f:
            state = _state(f)
            assert state[3]["capped"] > 0
            tr.set_camera(eye, *same)                                         # the pose it has: nothing changes
            f.update(1)
            if change == "camera":
                other = (2.0, 0.3, 0.5)
                tr.set_camera(other, *ds.calculate_camera_variables(other, (0, 0, 0), (0, 1, 0), 30.0, W / H))
            else:
                tr.set_light((0.3, -0.8, 0.2))
            for call in (lambda: f.update(), lambda: f.raise_cap(16)):
                with pytest.raises(_lib.CloudTraceError) as e:
                    call()
                assert e.value.code == _lib.CT_E_STATE and change in e.value.message
            assert _state(f) == state and f.device_ptr() != 0
            tr.render_accumulate(1, 1)                                        # the handle stays usable
            assert tr.subframes == 1


@pytest.mark.gpu
def test_argument_errors_leave_the_handle_and_the_frame_as_they_were():
    with tracer() as tr, device_run(tr, "A", split=(3,)) as f:
        L, h = tr.L, tr.h
        state, counters, allocations = _state(f), tr.counters(), ct.debug_allocations()

        def message(handle=h):
            return L.ct_last_error(handle).decode()

        def create(handle=h, abi=_lib.CT_ABI_VERSION, R=4, lo=8, cap=96, rel=0.7, abs_tol=1e-2, chunk=0, passes=0, with_desc=True, with_out=True):
            desc = _lib.CtAdaptiveFrameDesc(abi, R, lo, cap, rel, abs_tol, chunk, passes)
            out = C.c_void_p(1)
            rc = L.ct_adaptive_frame_create(handle, C.byref(desc) if with_desc else None, C.byref(out) if with_out else None)
            assert rc != _lib.CT_OK and (not with_out or not out.value or handle is None)
            return rc

        assert create(handle=None) == _lib.CT_E_INVAL
        for kw in (dict(with_desc=False), dict(with_out=False)):
            assert create(**kw) == _lib.CT_E_INVAL and "ct_adaptive_frame_create" in message(), kw
        for kw, word in ((dict(abi=_lib.CT_ABI_VERSION + 1), "abi_version"), (dict(R=0), "round_samples"), (dict(R=65536, lo=65536, cap=65536), "round_samples"),
                         (dict(cap=0), "max_samples"), (dict(cap=98), "max_samples"), (dict(cap=2 ** 24 + 4), "max_samples"),
                         (dict(lo=0), "min_samples"), (dict(lo=6), "min_samples"), (dict(lo=100), "min_samples"),
                         (dict(rel=-1.0), "rel_tol"), (dict(rel=float("inf")), "rel_tol"), (dict(abs_tol=float("nan")), "abs_tol"), (dict(abs_tol=-0.5), "abs_tol"),
                         (dict(chunk=96), "chunk_pixels"), (dict(passes=5), "pass_subframes")):
            assert create(**kw) == _lib.CT_E_INVAL, kw
            assert word in message() and "ct_adaptive_frame_create" in message(), (word, message())
        with tracer(flags=_lib.CT_FLAG_SIMPLE_KERNEL) as simple, tracer(shard_index=1, shard_count=2) as shard:
            assert create(handle=simple.h) == _lib.CT_E_INVAL and "persistent kernel" in message(simple.h)
            assert create(handle=shard.h) == _lib.CT_E_INVAL and "shard 1 of 2" in message(shard.h)
            for other in (simple, shard):                                     # ... which stay usable
                other.render_accumulate(1, 1)
                assert other.subframes == 1
        info, ptr = _lib.CtAdaptiveFrameInfo(), C.c_void_p()
        assert L.ct_adaptive_frame_info(f.f, None) == _lib.CT_E_INVAL
        assert L.ct_adaptive_frame_device_ptr(f.f, 3, C.byref(ptr)) == _lib.CT_E_INVAL
        assert L.ct_adaptive_frame_device_ptr(f.f, 0, None) == _lib.CT_E_INVAL
        buf = np.zeros(W * H * 4 + 1, np.float32)
        for which, nbytes in ((3, W * H * 16), (0, W * H * 16 - 4), (0, W * H * 16 + 4), (2, W * H * 16), (1, 0)):
            assert L.ct_adaptive_frame_download(f.f, which, buf.ctypes.data_as(C.c_void_p), nbytes) == _lib.CT_E_INVAL
            assert "ct_adaptive_frame_download" in message()
        assert L.ct_adaptive_frame_download(f.f, 0, None, W * H * 16) == _lib.CT_E_INVAL
        assert not buf.any() and ct.debug_allocations() == allocations
        assert _state(f) == state and tr.counters() == counters
        f.update()                                                            # ... and the frame goes on to what set A gives
        assert_equals_reference(f, gpu_reference("A"))


@pytest.mark.gpu
def test_every_allocation_is_given_back():
    start = ct.debug_allocations()
    with tracer() as tr:
        held = ct.debug_allocations()
        with device_run(tr, "A", split=(1,)) as f:
            inside = ct.debug_allocations()
            assert inside["device_buffers"] >= held["device_buffers"] + 6     # mean, M2, counts, two live lists, wave counts
            f.update()
            assert ct.debug_allocations()["device_buffers"] == inside["device_buffers"]   # (the point buffers hold 384 entries already)
        after = ct.debug_allocations()
        assert after["device_buffers"] == inside["device_buffers"] - 6
        assert after["device_bytes"] == inside["device_bytes"] - (W * H * (16 + 16 + 4 + 4 + 4) + (W * H // 64 + 1) * 4)
    assert ct.debug_allocations() == start


@pytest.mark.gpu
def test_the_armed_invariants_report_no_violation_over_set_a(monkeypatch):
    monkeypatch.setenv("CT_DEBUG_INVARIANTS", "1")
    ref = gpu_reference("A")
    with tracer() as tr, device_run(tr, "A") as f:
        assert_equals_reference(f, ref)
        iv = tr.debug_invariants()
        assert iv["armed"] == 1 and iv["checks"] > 0 and iv["violations"] == 0 and iv["samples_without_alpha_1"] == 0
        assert iv["dealt"] == iv["written"] == int(ref[2].sum())


@pytest.mark.gpu
def test_cli_adaptive_writes_the_python_paths_mean_and_counts(tmp_path):
    from deepestscatter_amd import build
    cli = build.build_cli()
    counts_file = tmp_path / "counts.u32"
    r = subprocess.run([str(cli), "procedural:32", "--size", f"{W}x{H}", "--light", "Side", "--out", str(tmp_path),
                        "--adaptive", "4,96,8,0.7,0.01", "--adaptive-counts", str(counts_file)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with ds.CloudTracer(ds.make_procedural_cloud(32), width=W, height=H, mode=0, light_direction=ds.LIGHT_DIRECTIONS["Side"]) as tr, \
            tr.adaptive_frame(**params_of("A")) as f:
        info = f.update()
        mean, counts = f.mean(), f.counts()
    assert 0 < info["converged"] < W * H and info["paths"] < 96 * W * H
    assert (f'adaptive {{"rounds": {info["rounds"]}, "pixels": {W * H}, "converged": {info["converged"]}, "capped": {info["capped"]}, '
            f'"paths": {info["paths"]}}}') in r.stdout
    assert np.fromfile(counts_file, "<u4").tobytes() == counts.tobytes()
    rgb = exr.read_exr(tmp_path / "procedural_32.Side.PT.exr")
    assert rgb.shape == (H, W, 3) and rgb.tobytes() == np.ascontiguousarray(mean[..., :3]).tobytes()
    for extra in (["--gpus", "1"], ["--display"], ["--traced-bake", "4,4,4,4,2", "--bake-samples", "4"], ["--network", "none.bin"]):
        r = subprocess.run([str(cli), "procedural:32", "--adaptive", "4,96", *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--adaptive" in r.stdout
