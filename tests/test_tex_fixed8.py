"""CT_FLAG_TEX_FIXED8: the kernels filter with the reference's texture-unit weights -- every linear / trilinear weight rounded
to 1.8 fixed point, rint(frac * 256) / 256 -- and are bit-exact against the oracle build that does the same
(libct_oracle_fixed8.so, -DORC_TEX_FIXED8).  The GPU tests mirror tests/test_gpu_parity.py with the flag on both sides; the
last GPU test checks that the flag changes the result, so a flag that is dropped on the way cannot pass."""
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import _oracle as O
import deepestscatter_amd as ds
from deepestscatter_amd import _lib
from conftest import sphere_volume

ROOT = Path(__file__).resolve().parents[1]
F8 = _lib.CT_FLAG_TEX_FIXED8
ORACLE_KEYS = ("cloud_size_m", "mean_free_path_m", "sample_step", "max_depth", "light_direction", "light_color", "light_intensity",
               "estimator")


def make_pair8(tex, w, h, mode=0, flags=0, **kw):
    tr = ds.CloudTracer(tex, width=w, height=h, mode=mode, flags=F8 | flags, **kw)
    orc = O.Oracle(tex, w, h, mode=mode, fast="fixed8", **{k: v for k, v in kw.items() if k in ORACLE_KEYS})
    return tr, orc


# ---------------------------------------------------------------------------------------------------- CPU
def test_header_constant_equals_the_python_binding():
    header = (ROOT / "include" / "cloudtrace.h").read_text()
    m = re.search(r"#define CT_FLAG_TEX_FIXED8 (\d+)u", header)
    assert m and int(m.group(1)) == F8 == 16
    others = [int(v) for v in re.findall(r"#define CT_FLAG_(?!TEX_FIXED8)\w+ (\d+)u", header)]
    assert F8 & ~0 and not any(F8 & v for v in others)          # a bit of its own


def test_cli_usage_lists_the_flag():
    from deepestscatter_amd import build
    cli = build.build_cli()
    r = subprocess.run([str(cli)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "[--tex-fixed8]" in r.stderr
    src = (ROOT / "deepestscatter_amd" / "host" / "main.cpp").read_text()
    assert src.count("--tex-fixed8") >= 3                         # header comment (render and collect) and the option itself


def test_fixed8_oracle_cdf_bisection_equals_the_default_over_every_input():
    """The guide table of the scatter direction (getNewDirection) is not touched by the flag: tex1D of the CDF at j/65536 has
    weights ((j - 8) & 15) / 16, which 1.8 fixed point holds exactly.  Pinned over all 2^24 random numbers."""
    n = 1 << 24
    assert np.array_equal(O.cdf_bisect_k(0, n, fast="fixed8"), O.cdf_bisect_k(0, n, fast=True))


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("dims", [(32, 32, 32), (20, 28, 36), (40, 24, 16)])
def test_shadow_volume_bit_exact(dims):
    tex = sphere_volume(dims=dims, seed=2)
    tr, orc = make_pair8(tex, 8, 8)
    assert np.array_equal(tr.inscatter(), orc.inscatter)
    tr.close()
    tr, orc = make_pair8(sphere_volume(dims=dims, seed=4), 8, 8, light_direction=(0.586, -0.766, -0.271), sample_step=1.0 / 128.0,
                         cloud_size_m=3000.0)
    assert np.array_equal(tr.inscatter(), orc.inscatter)
    tr.close()


@pytest.mark.gpu
def test_shadow_volume_texel_exact_at_512():
    tex = ds.make_procedural_cloud(512)
    tr = ds.CloudTracer(tex, width=8, height=8, flags=F8)
    got = tr.inscatter()
    tr.close()
    orc = O.Oracle(tex, 8, 8, fast="fixed8", inscatter="none")
    rng = np.random.default_rng(5)
    nz, ny, nx = tex.shape
    xyz = rng.integers(0, [nx, ny, nz], (400000, 3))
    inside = xyz[tex[xyz[:, 2], xyz[:, 1], xyz[:, 0]] > 0]      # texels in the cloud (the ones the NEE reads most) and anywhere
    xyz = np.concatenate([inside[:30000], xyz[:10000]]).astype(np.uint32)
    assert len(xyz) > 20000
    want = orc.inscatter_texels(xyz)
    assert np.array_equal(got[xyz[:, 2], xyz[:, 1], xyz[:, 0]], want)
    assert len(np.unique(want)) > 10


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_subframe_radiance_mean_m2_and_counters_all_modes(mode, monkeypatch):
    tex = sphere_volume(32, seed=1)
    w, h = 32, 24
    tr, orc = make_pair8(tex, w, h, mode=mode)
    for sid in (1, 2, 7):
        tr.render_subframe(sid)
        assert np.array_equal(tr.frame(), orc.render_subframe(sid)), (mode, sid)
    assert tr.counters() == orc.counters.as_dict()
    tr.close()
    tr, orc = make_pair8(tex, w, h, mode=mode)
    mean, m2 = orc.render(9)
    tr.render_accumulate(1, 4)
    tr.render_accumulate(5, 5)
    assert np.array_equal(tr.mean(), mean) and np.array_equal(tr.m2(), m2)
    assert tr.counters() == orc.counters.as_dict()
    tr.close()
    # the diagnostics build of the kernel (CT_DEBUG_INVARIANTS) samples the same way
    monkeypatch.setenv("CT_DEBUG_INVARIANTS", "1")
    tr = ds.CloudTracer(tex, width=w, height=h, mode=mode, flags=F8)
    tr.render_accumulate(1, 9)
    assert np.array_equal(tr.mean(), mean) and np.array_equal(tr.m2(), m2)
    assert tr.debug_invariants()["violations"] == 0
    tr.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nee", ["0", "1", "2"])
def test_delta_fetch_layouts(nee, monkeypatch):
    monkeypatch.setenv("CT_DELTA_NEE", nee)
    rng = np.random.default_rng(7)
    cases = [
        (sphere_volume(dims=(23, 31, 17), seed=5), 40, 28, dict(mode=0, cloud_size_m=9000.0)),
        (rng.integers(0, 256, (14, 19, 26)).astype(np.uint8), 33, 21, dict(mode=0, cloud_size_m=300.0, max_depth=60)),   # no border
        (sphere_volume(dims=(40, 40, 40), radius=0.45, seed=9), 36, 36, dict(mode=1, cloud_size_m=4000.0, max_depth=300)),
        (sphere_volume(dims=(29, 29, 29), seed=11), 32, 24, dict(mode=2)),
    ]
    for invariants in ("0", "1"):                                   # the product's kernel and the diagnostics build
        monkeypatch.setenv("CT_DEBUG_INVARIANTS", invariants)
        for tex, w, h, kw in cases:
            tr, orc = make_pair8(tex, w, h, estimator=1, **kw)
            assert tr.delta_grid()["nee"] == int(nee)
            tr.render_accumulate_async(1, 3)
            tr.render_accumulate(4, 4)
            tr.render_accumulate_async(8, 5)
            mean, m2 = orc.render(12)
            assert np.array_equal(tr.mean(), mean) and np.array_equal(tr.m2(), m2), (nee, invariants, tex.shape, kw)
            assert tr.counters() == orc.counters.as_dict(), (nee, invariants, tex.shape, kw)
            tr.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nee", ["1", "2"])
def test_delta_interior_kernel(nee, monkeypatch):
    monkeypatch.setenv("CT_DELTA_NEE", nee)
    rng = np.random.default_rng(23)
    tex = np.zeros((28, 28, 28), np.uint8)
    tex[6:22, 6:22, 6:22] = rng.integers(1, 256, (16, 16, 16)).astype(np.uint8)
    for mode in (0, 1, 2):
        tr, orc = make_pair8(tex, 40, 30, mode=mode, cloud_size_m=600.0, max_depth=200, estimator=1)
        assert tr.delta_grid()["interior"] is True
        tr.render_accumulate_async(1, 4)
        tr.render_accumulate(5, 3)
        tr.render_accumulate_async(8, 5)
        mean, m2 = orc.render(12)
        assert np.array_equal(tr.mean(), mean) and np.array_equal(tr.m2(), m2), mode
        assert tr.counters() == orc.counters.as_dict() and tr.counters()["scatter_events"] > 0, mode
        tr.close()


@pytest.mark.gpu
def test_sparse_bricks_and_simple_kernel(monkeypatch):
    tex = sphere_volume(dims=(96, 72, 80), radius=0.12, seed=21)
    w, h = 40, 32
    for flags in (_lib.CT_FLAG_SPARSE_BRICKS, _lib.CT_FLAG_SIMPLE_KERNEL):
        tr, orc = make_pair8(tex, w, h, flags=flags)
        if flags == _lib.CT_FLAG_SPARSE_BRICKS:
            assert tr.debug_memory()["sparse"] == 1
        mean, m2 = orc.render(3)
        tr.render_accumulate(1, 3)
        assert np.array_equal(tr.mean(), mean) and np.array_equal(tr.m2(), m2), flags
        assert tr.counters() == orc.counters.as_dict(), flags
        tr.close()
    # the sparse diagnostics kernel
    monkeypatch.setenv("CT_DEBUG_INVARIANTS", "1")
    tr = ds.CloudTracer(tex, width=w, height=h, flags=F8 | _lib.CT_FLAG_SPARSE_BRICKS)
    tr.render_accumulate(1, 3)
    assert np.array_equal(tr.mean(), mean) and np.array_equal(tr.m2(), m2)
    tr.close()


@pytest.mark.gpu
def test_enqueued_batches_with_path_continuation():
    tex = sphere_volume(48, radius=0.42, seed=17)
    w, h = 256, 192
    kw = dict(mode=0, cloud_size_m=30000.0, max_depth=300)
    tr = ds.CloudTracer(tex, width=w, height=h, flags=F8, **kw)
    ref = ds.CloudTracer(tex, width=w, height=h, flags=F8, **kw)
    first = 1
    for n in (4, 3, 5, 2, 6, 4):
        tr.render_accumulate_async(first, n)
        ref.render_accumulate(first, n)
        first += n
    tr.synchronize()
    assert tr.debug_suspended() > 1000
    assert np.array_equal(tr.mean(), ref.mean()) and np.array_equal(tr.m2(), ref.m2())
    assert tr.counters() == ref.counters()
    orc = O.Oracle(tex, w, h, fast="fixed8", **kw)
    win = (112, 80, 144, 112)
    mean, m2 = orc.render(first - 1, window=win)
    sl = np.s_[win[1]:win[3], win[0]:win[2]]
    assert np.array_equal(tr.mean()[sl], mean[sl]) and np.array_equal(tr.m2()[sl], m2[sl])
    tr.close()
    ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("estimator", [0, 1])
def test_pixel_tile_shards_sum_to_the_whole(estimator):
    tex = sphere_volume(32, seed=10)
    w, h = 40, 24
    whole, orc = make_pair8(tex, w, h, estimator=estimator)
    whole.render_accumulate(1, 3)
    mean, m2 = orc.render(3)
    assert np.array_equal(whole.mean(), mean) and np.array_equal(whole.m2(), m2)
    total_mean = np.zeros((h, w, 4), np.float32)
    total_m2 = np.zeros_like(total_mean)
    for i in range(3):
        sh = ds.CloudTracer(tex, width=w, height=h, estimator=estimator, shard_index=i, shard_count=3, flags=F8)
        sh.render_accumulate_async(1, 2)
        sh.render_accumulate(3, 1)
        total_mean += sh.mean()
        total_m2 += sh.m2()
        sh.close()
    assert np.array_equal(total_mean, mean) and np.array_equal(total_m2, m2)
    whole.close()


@pytest.mark.gpu
def test_descriptors_point_radiance_and_scatter_samples():
    for dims, size_m in (((40, 40, 40), 700.0), ((36, 52, 44), 3000.0)):
        tex = sphere_volume(dims=dims, seed=31)
        tr, orc = make_pair8(tex, 8, 8, cloud_size_m=size_m)
        pos, view = tr.generate_scatter_samples(48, batch_seed=5)
        opos, oview = orc.generate_scatter_samples(48, batch_seed=5)
        assert pos.tobytes() == opos.tobytes() and view.tobytes() == oview.tobytes()
        rng = np.random.default_rng(9)
        extra = rng.uniform(-0.75, 0.75, (16, 3)).astype(np.float32)
        extra_v = rng.normal(size=(16, 3)).astype(np.float32)
        extra_v /= np.linalg.norm(extra_v, axis=1, keepdims=True)
        pos, view = np.concatenate([pos, extra]), np.concatenate([view, extra_v])
        got = tr.collect_descriptors(pos, view)
        assert np.array_equal(got, orc.collect_descriptors(pos, view)) and got.any()
        tr.close()
    tex = sphere_volume(32, seed=35)
    rng = np.random.default_rng(3)
    pos = (rng.random((100, 3), dtype=np.float32) - 0.5) * 0.5
    d = rng.normal(size=(100, 3)).astype(np.float32)
    for estimator in (0, 1):
        tr, orc = make_pair8(tex, 8, 8, mode=1, estimator=estimator)
        got = tr.point_radiance_launch(ds.make_point_tasks(pos, d), 1, 5)
        ref = orc.point_radiance_launch(ds.make_point_tasks(pos, d), 1, 5)
        assert got.tobytes() == ref.tobytes(), estimator
        tr.close()


@pytest.mark.gpu
def test_north_star_window_after_1024_spp_in_the_references_texture_arithmetic():
    """configs[2] (512^3 / 1024^2 / 1024 spp, rendered the way bench.py does) with the flag: a 16x16 window is bit-identical
    to the fixed8 oracle, which integrates its own shadow volume for every texel its paths touch; those texels equal the
    product's shadow volume one by one."""
    tex = ds.make_procedural_cloud(512)
    w = h = 1024
    tr = ds.CloudTracer(tex, width=w, height=h, flags=F8)
    first = 1
    for _ in range(4):
        tr.render_accumulate_async(first, 256)
        first += 256
    tr.synchronize()
    mean, m2 = tr.mean(), tr.m2()
    orc = O.Oracle(tex, w, h, fast="fixed8", inscatter="lazy")
    x0, y0 = 500, 520
    ref_mean, ref_m2 = orc.render(1024, window=(x0, y0, x0 + 16, y0 + 16))
    sl = np.s_[y0:y0 + 16, x0:x0 + 16]
    assert ref_mean[sl][..., 0].mean() > 0.5
    assert np.array_equal(mean[sl], ref_mean[sl]) and np.array_equal(m2[sl], ref_m2[sl])
    touched = orc.inscatter_valid.astype(bool)
    assert touched.sum() > 1_000_000
    assert np.array_equal(tr.inscatter()[touched], orc.inscatter[touched])
    tr.close()


@pytest.mark.gpu
def test_cli_render_and_collect_with_the_flag(tmp_path):
    from deepestscatter_amd import build, exr
    from deepestscatter_amd import collector as col
    cli = build.build_cli()
    tex = ds.make_procedural_cloud(32)
    want = {}
    for flags in (0, F8):
        tr = ds.CloudTracer(tex, width=40, height=24, light_direction=ds.LIGHT_DIRECTIONS["Back"], flags=flags)
        tr.render_accumulate(1, 5)
        want[flags] = tr.mean()[..., :3]
        tr.close()
    assert not np.array_equal(want[0], want[F8])
    out = tmp_path / "r"
    out.mkdir()
    r = subprocess.run([str(cli), "procedural:32", "--size", "40x24", "--spp", "5", "--light", "Back", "--tex-fixed8", "--out", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(exr.read_exr(out / "procedural_32.Back.PT.exr"), want[F8])
    # collect: scatter samples, point radiance and descriptors of one batch, as the Python pipeline computes them with the flag
    batch, scene_id = 32, 1
    out = tmp_path / "tables"
    r = subprocess.run([str(cli), "collect", "procedural:48", "--batch", str(batch), "--scene-id", str(scene_id), "--light", "Back",
                        "--tex-fixed8", "--out", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    tr = ds.CloudTracer(ds.make_procedural_cloud(48), width=64, height=64, mode=1, light_direction=ds.LIGHT_DIRECTIONS["Back"], flags=F8)
    start = scene_id * batch
    pos, view = tr.generate_scatter_samples(batch, start)
    samples = [(start + i, col.encode_scatter_sample(scene_id, pos[i], view[i])) for i in range(batch)]
    assert col.read_flat_dataset(out / "ScatterSample.flat") == ("ScatterSample", samples)
    rc = col.RadianceCollector(tr.point_radiance_launch, pos, view, batch_start_id=start)
    while not rc.is_completed():
        rc.update()
    assert col.read_flat_dataset(out / "Result.flat") == ("Result", rc.results())
    dc = col.DisneyDescriptorCollector(tr.collect_descriptors, [s for _, s in samples], batch_start_id=start)
    assert col.read_flat_dataset(out / "DisneyDescriptor.flat") == ("DisneyDescriptor", dc.results())
    tr.close()


@pytest.mark.gpu
@pytest.mark.parametrize("estimator", [0, 1])
def test_the_flag_changes_the_shadow_volume_and_the_frames(estimator):
    tex = sphere_volume(32, seed=1)
    a = ds.CloudTracer(tex, width=32, height=24, estimator=estimator)
    b = ds.CloudTracer(tex, width=32, height=24, estimator=estimator, flags=F8)
    assert not np.array_equal(a.inscatter(), b.inscatter())
    a.render_accumulate(1, 4)
    b.render_accumulate(1, 4)
    assert not np.array_equal(a.mean(), b.mean())
    # ... and it is the oracle's default build that the flag-less handle equals
    orc = O.Oracle(tex, 32, 24, fast=True, estimator=estimator)
    assert np.array_equal(a.mean(), orc.render(4)[0])
    a.close()
    b.close()


@pytest.mark.gpu
def test_the_exchange_kernels_refuse_the_flag():
    """The experiments build's path-exchange kernels filter with the exact weights only: ct_create says so instead of
    ignoring the flag (child process: this one keeps the product's library)."""
    from deepestscatter_amd import build
    build.build_variant("exp")
    code = ("import numpy as np; import deepestscatter_amd as ds; from deepestscatter_amd import _lib\n"
            "tex = np.zeros((16, 16, 16), np.uint8); tex[4:12, 4:12, 4:12] = 200\n"
            "ds.CloudTracer(tex, width=16, height=16, estimator=1).close()\n"
            "try:\n    ds.CloudTracer(tex, width=16, height=16, estimator=1, flags=_lib.CT_FLAG_TEX_FIXED8)\n"
            "except _lib.CloudTraceError as e:\n    print('refused', e.code == _lib.CT_E_INVAL, 'TEX_FIXED8' in e.message)\n")
    env = dict(os.environ, CT_LIBRARY="libcloudtrace_exp.so", CT_EXCHANGE="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert r.returncode == 0 and "refused True True" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
