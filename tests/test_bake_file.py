"""Bake files: ct_bake_save, ct_bake_file_info, ct_bake_load (include/cloudtrace.h, "bake files").

Every comparison is on the bits.  A loaded bake is held to the bake that was saved -- every accessor, every lookup, every frame --
the saved bytes to network.write_bake_file_reference of the downloads, and a continued loaded bake to an uninterrupted one.

Scene: sphere_volume(32, seed=12), 24 x 16 (and 27 x 13 on 3 shards), grids 5 x 4 x 3 x 4 with 3 and 2 polar nodes.  On that
volume the mask of a 5 x 4 x 3 grid has all 60 nodes active (margin 4 texels of 32), so the kinds that keep a mask run a second
time on SMALL, sphere_volume(48, radius=0.12, seed=12), whose mask is a proper subset: 36 of 60 nodes (test_the_masks_of_the_two_volumes).
Traced bakes take 4 samples; adaptive ones R = 4, cap 8 raised to 16, rel_tol 0.7."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import deepestscatter_amd as ds
from deepestscatter_amd import _lib
from deepestscatter_amd import cloudtrace as ct
from deepestscatter_amd import network as N
from conftest import sphere_volume

ROOT = Path(__file__).resolve().parents[1]
W, H, SID = 24, 16, 3
SCALE = (0.5, 2.0, 3.0)
LIGHT2 = (0.586, -0.766, -0.271)
GRID3 = ((5, 4, 3), 4, 3)
GRID2 = ((5, 4, 3), 4, 2)
SAMPLES = 4
P = dict(round_samples=4, max_samples=8, rel_tol=0.7, abs_tol=1e-4, zero_samples=7)
STEP = ds.SceneParams().sample_step
MARCH, DELTA = 0, 1
f32 = np.float32


def volume(small=False):
    return sphere_volume(48, radius=0.12, seed=12) if small else sphere_volume(32, seed=12)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _code(fn, *a, **kw):
    with pytest.raises(_lib.CloudTraceError) as e:
        fn(*a, **kw)
    return e.value.code


def header_of(kind=0, fmt=0, traced=0, adaptive=0, grid=(5, 4, 3), nphi=4, nc=3, active=None, **over):
    """A consistent header for a 32^3 volume, as a dict for write_bake_file_reference."""
    nodes = grid[0] * grid[1] * grid[2]
    active = nodes if kind == 0 else (23 if active is None else active)
    block = nphi * nc
    h = dict(kind=kind, format=fmt, traced=traced, adaptive=adaptive, grid=grid, azimuths=nphi, cosines=nc, margin_texels=0 if kind == 0 else 4,
             entries=nodes * block, stored_entries=(active + 1) * block if kind == 2 else nodes * block, active_nodes=active,
             light=(0, 0, 1), axis_a=(1, 0, 0), axis_b=(0, 1, 0), dims=(32, 32, 32), sample_step_bits=int(np.array(STEP, f32).view(np.uint32)),
             mean_free_path_bits=int(np.array(10, f32).view(np.uint32)), cloud_size_bits=int(np.array(7000, f32).view(np.uint32)),
             estimator=1, tex_fixed8=1, light_color_bits=(0x3F800000,) * 3, light_intensity_bits=0x49742400, volume_hash=0x0123456789ABCDEF)
    if traced:
        h.update(samples=8, paths=8 * active * block)
    if adaptive:
        h.update(round_samples=4, max_samples=8, zero_samples=7, rel_tol_bits=int(np.array(0.7, f32).view(np.uint32)),
                 abs_tol_bits=int(np.array(1e-4, f32).view(np.uint32)), rounds=2, capped=17, converged=active * block - 17)
    h.update(over)
    return h


def payload_of(h, seed=3):
    rng = np.random.default_rng(seed)
    nodes = h["grid"][0] * h["grid"][1] * h["grid"][2]
    stored = h["stored_entries"]
    out = {"table": rng.integers(0, 0x7BFF, stored).astype(np.uint16) if h["format"] else rng.random(stored, dtype=f32)}
    if h["kind"]:
        mask = np.zeros(nodes, np.uint8)
        mask[rng.permutation(nodes)[:h["active_nodes"]]] = 1
        out["nodes"] = mask
    if h["adaptive"]:
        out["m2"] = rng.random(stored, dtype=f32)
        out["counts"] = rng.integers(0, 9, stored).astype(np.uint32)
    return out


def write(tmp_path, data, name="f.bake"):
    p = tmp_path / name
    p.write_bytes(data)
    return p


def reseal(data):
    data = bytes(data)[:-8]
    return data + np.array(N.fnv1a64_reference(data), "<u8").tobytes()


# ---------------------------------------------------------------------------------------------------- CPU
def test_symbols_resolve_and_answer_null_arguments(product_lib, tmp_path):
    L = product_lib
    for name in ("ct_bake_save", "ct_bake_file_info", "ct_bake_load", "ct_debug_volume_hash"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    out, info = C.c_void_p(1), _lib.CtBakeFileInfo()
    assert L.ct_bake_save(None, b"x") == _lib.CT_E_INVAL and L.ct_bake_save(None, None) == _lib.CT_E_INVAL
    assert L.ct_bake_load(None, b"x", C.byref(out)) == _lib.CT_E_INVAL
    assert L.ct_bake_file_info(None, C.byref(info)) == _lib.CT_E_INVAL and L.ct_bake_file_info(b"x", None) == _lib.CT_E_INVAL
    assert L.ct_debug_volume_hash(None, None) == _lib.CT_E_INVAL
    assert L.ct_bake_file_info(os.fsencode(tmp_path / "missing.bake"), C.byref(info)) == _lib.CT_E_INVAL
    assert "cannot open" in L.ct_last_error(None).decode()


def test_struct_layout_matches_the_header():
    import tempfile
    names = [n for n, _ in _lib.CtBakeFileHeader._fields_]
    tail = [n for n, _ in _lib.CtBakeFileInfo._fields_[1:]]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "cloudtrace.h"\nint main(){printf("%zu %zu %d %d %u", sizeof(CtBakeFileHeader), '
           'sizeof(CtBakeFileInfo), CT_BAKE_F32, CT_BAKE_F16, CT_BAKE_FILE_VERSION);'
           + "".join(f'printf(" %zu", offsetof(CtBakeFileHeader, {f}));' for f in names)
           + "".join(f'printf(" %zu", offsetof(CtBakeFileInfo, {f}));' for f in tail) + 'printf(" %s", CT_BAKE_FILE_MAGIC);return 0;}')
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "p.c").write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", f"{d}/p", f"{d}/p.c"], check=True)
        raw = subprocess.run([f"{d}/p"], capture_output=True, check=True).stdout
    out = [int(v) for v in raw.split()[:5 + len(names) + len(tail)]]
    assert out[:5] == [256, 312, 0, 1, 1] and raw.endswith(b" CTBAKE\r\n")
    pinned = [0, 8, 12, 16, 20, 24, 28, 32, 44, 48, 52, 56, 64, 72, 80, 92, 104, 116, 128, 132, 136, 140, 144, 148, 160, 164, 168, 176, 184, 188,
              192, 196, 200, 204, 208, 216, 224]
    assert out[5:5 + len(names)] == pinned == [getattr(_lib.CtBakeFileHeader, f).offset for f in names]
    assert pinned == [N.bake_file_dtype.fields[f][1] for f in names] and N.bake_file_dtype.itemsize == 256
    assert out[5 + len(names):] == [256, 264, 272, 280, 288, 296, 304] == [getattr(_lib.CtBakeFileInfo, f).offset for f in tail]
    assert _lib.CT_BAKE_FILE_MAGIC == N.BAKE_FILE_MAGIC == b"CTBAKE\r\n"


def test_the_masks_of_the_two_volumes():
    full = N.bake_mask_reference(volume(), (5, 4, 3), STEP)
    small = N.bake_mask_reference(volume(small=True), (5, 4, 3), STEP)
    assert full[2] == small[2] == 4
    assert int(full[1].sum()) == 60                     # every node of the grid is active on sphere_volume(32, seed=12)
    assert int(small[1].sum()) == 36                    # SMALL: a proper subset


def test_volume_hash_reference():
    a = volume()
    b = a.copy()
    z, y, x = np.argwhere(a > 3)[0]
    b[z, y, x] -= 1
    assert N.volume_hash_reference(a) != N.volume_hash_reference(b)
    c = a.copy().reshape(-1)
    i, j = np.flatnonzero(c == c.max())[0], np.flatnonzero(c == 0)[0]     # two unequal texels, swapped
    c[i], c[j] = c[j], c[i]
    assert N.volume_hash_reference(c) != N.volume_hash_reference(a)
    want = 0                                                                # the formula, in Python integers
    for k, t in enumerate(a.reshape(-1)[:4096].tolist()):
        want = (want + (t + 1) * (((k + 1) * 0x9E3779B97F4A7C15) % 2 ** 64)) % 2 ** 64
    assert N.volume_hash_reference(a.reshape(-1)[:4096]) == want
    assert N.fnv1a64_reference(b"") == 0xCBF29CE484222325 and N.fnv1a64_reference(b"a") == 0xAF63DC4C8601EC8C


CASES = [(kind, fmt, traced, adaptive) for kind in (0, 1, 2) for fmt in (0, 1) for traced, adaptive in ((0, 0), (1, 0), (1, 1))
         if not (fmt and adaptive)]


@pytest.mark.parametrize("kind, fmt, traced, adaptive", CASES)
def test_file_info_returns_the_header(tmp_path, kind, fmt, traced, adaptive):
    h = header_of(kind, fmt, traced, adaptive)
    parts = payload_of(h)
    data = N.write_bake_file_reference(h, **parts)
    info = N.bake_file_info(write(tmp_path, data))
    for name, value in h.items():
        assert np.array_equal(np.asarray(info[name]), np.asarray(value, np.asarray(info[name]).dtype)), name
    assert info["magic"] == N.BAKE_FILE_MAGIC and info["version"] == 1 and info["header_bytes"] == 256 and not info["reserved"].any()
    assert info["file_bytes"] == len(data) and info["checksum_offset"] == len(data) - 8
    assert info["checksum"] == N.fnv1a64_reference(data[:-8])
    back = N.read_bake_file_reference(data)
    for name, a in parts.items():
        at = info[f"{name}_offset"]
        assert at % 16 == 0 and at >= 256
        assert np.array_equal(back[name].view(np.uint8), np.ascontiguousarray(a).view(np.uint8)), name
        assert data[at:at + a.nbytes] == a.tobytes()
    assert (info["nodes_offset"] == 0) == (kind == 0) and (info["m2_offset"] == 0) == (not adaptive) == (info["counts_offset"] == 0)
    assert info["table_offset"] + h["stored_entries"] * (2 if fmt else 4) <= info["checksum_offset"]


def test_every_refusal_of_file_info(tmp_path, product_lib):
    L = product_lib

    def refused(data, word, name="bad.bake"):
        info = _lib.CtBakeFileInfo()
        assert L.ct_bake_file_info(os.fsencode(write(tmp_path, data, name)), C.byref(info)) == _lib.CT_E_INVAL, word
        message = L.ct_last_error(None).decode()
        assert word in message and "ct_bake_file_info" in message, (word, message)

    h = header_of(2, 0, 1, 1)
    parts = payload_of(h)
    good = N.write_bake_file_reference(h, **parts)
    info = N.bake_file_info(write(tmp_path, good))
    # each truncated section, the header and the checksum
    refused(good[:100], "shorter")
    for at, word in ((info["nodes_offset"] + 30, "the node bytes"), (info["table_offset"] + 5, "the table"), (info["m2_offset"] + 9, "m2"),
                     (info["counts_offset"] + 3, "the counts"), (len(good) - 1, "the checksum")):
        refused(good[:at], "truncated in " + word)
    refused(good + b"\0", "behind the checksum")
    # a flipped payload byte in every section, a flipped header byte
    for at in (info["nodes_offset"] + 3, info["table_offset"] + 11, info["m2_offset"] + 2, info["counts_offset"] + 6, 170):
        bad = bytearray(good)
        bad[at] ^= 0x10
        refused(bad, "checksum")

    def with_header(**over):
        hh = dict(h, **over)
        raw = bytearray(N.write_bake_file_reference(h, **parts))
        rec = np.frombuffer(bytes(raw[:256]), N.bake_file_dtype, 1).copy()
        for name, value in over.items():
            rec[name] = value
        raw[:256] = rec.tobytes()
        return reseal(raw), hh

    refused(with_header(magic=b"CTBAKX\r\n")[0], "magic")
    refused(with_header(version=2)[0], "version 2")
    refused(with_header(header_bytes=260)[0], "header")
    refused(with_header(kind=3)[0], "kind")
    refused(with_header(format=2)[0], "format")
    refused(with_header(azimuths=6)[0], "azimuths")
    refused(with_header(cosines=65)[0], "cosines")
    refused(with_header(grid=(1, 4, 3))[0], "grid[0] = 1")
    refused(with_header(grid=(5, 257, 3))[0], "grid[1] = 257")
    refused(with_header(entries=h["entries"] + 1)[0], "entries")
    refused(with_header(stored_entries=h["stored_entries"] + 12)[0], "stored entries")
    refused(with_header(active_nodes=61, stored_entries=62 * 12)[0], "active nodes")
    refused(with_header(traced=0)[0], "adaptive")
    refused(with_header(format=1)[0], "adaptive")
    refused(with_header(samples=2 ** 24 + 1)[0], "samples")
    refused(with_header(round_samples=0)[0], "round_samples")
    refused(with_header(max_samples=10)[0], "max_samples")
    refused(with_header(rel_tol_bits=0x7FC00000)[0], "rel_tol")
    refused(with_header(rounds=3)[0], "rounds")
    refused(with_header(capped=10 ** 6)[0], "capped")
    refused(with_header(dims=(32, 0, 32))[0], "dims[1]")
    refused(with_header(estimator=2)[0], "estimator")
    refused(with_header(tex_fixed8=2)[0], "tex_fixed8")
    refused(with_header(reserved=np.arange(32, dtype=np.uint8))[0], "reserved")
    # a header too large for its file: 2^26 stored entries announced, 276 stored
    big = with_header(grid=(256, 256, 16), azimuths=8, cosines=8, entries=2 ** 26, active_nodes=2 ** 20 - 1, stored_entries=2 ** 26,
                      converged=(2 ** 20 - 1) * 64 - 17)[0]
    refused(big, "truncated")
    refused(with_header(grid=(256, 256, 32), azimuths=8, cosines=8, entries=2 ** 27, active_nodes=2 ** 21 - 1, stored_entries=2 ** 27)[0], "2^26")
    # a stored_entries that agrees with active_nodes but not with the node bytes, and a node byte that is neither 0 nor 1
    one_more = dict(parts, nodes=parts["nodes"].copy())
    one_more["nodes"][np.flatnonzero(parts["nodes"] == 0)[0]] = 1
    refused(N.write_bake_file_reference(h, **one_more), "node bytes are set")
    two = dict(parts, nodes=parts["nodes"].copy())
    two["nodes"][np.flatnonzero(parts["nodes"])[0]] = 2
    refused(N.write_bake_file_reference(h, **two), "not 0 or 1")
    gap = bytearray(good)
    assert info["table_offset"] > info["nodes_offset"] + 60
    gap[info["nodes_offset"] + 60] = 1
    refused(reseal(gap), "gap")
    # a dense network file with traced fields
    d = header_of(0, 0, 0, 0)
    refused(N.write_bake_file_reference(dict(d, samples=4), **payload_of(d)), "network")
    refused(N.write_bake_file_reference(dict(d, rounds=1), **payload_of(d)), "adaptive parameters")
    refused(N.write_bake_file_reference(dict(d, margin_texels=4), **payload_of(d)), "margin")
    # ... and the numpy reader refuses what it can see
    for bad in (good[:-1], good[:100], bytes(gap)):
        with pytest.raises(ValueError):
            N.read_bake_file_reference(bad)


def test_the_parser_under_the_sanitizers():
    """tests/sanitize_bakefile: the device-free parser, a valid file of every kind and a few thousand seeded mutations, built with
    -fsanitize=address,undefined and run as a plain child process."""
    here = ROOT / "tests" / "sanitize_bakefile"
    subprocess.run(["make", "-C", str(here), "_build/bakefile_asan"], check=True, capture_output=True)
    r = subprocess.run([str(here / "_build" / "bakefile_asan")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    word, inputs, accepted = r.stdout.split()
    assert word == "ok" and int(inputs) >= 4000 and 15 <= int(accepted) < int(inputs)


# ---------------------------------------------------------------------------------------------------- GPU
def tracer(small=False, w=W, h=H, **kw):
    return ds.CloudTracer(volume(small), width=w, height=h, **kw)


def small_net(tr):
    from test_network_render import SMALL, weights
    return N.Network(tr, weights(SMALL), 32, 1, 1)


def make(tr, what, kind, grid=GRID3, net=None, p=P):
    kw = {"sparse": kind == "sparse", "compact": kind == "compact"}
    if what == "net":
        return tr.network_bake(net, *grid, **kw)
    if what == "traced":
        return tr.traced_bake(*grid, SAMPLES, **kw)
    return tr.traced_bake_adaptive(*grid, **p, **kw)


def records(tr, n, seed=5, nan=True):
    """n lookup records: inside and outside the box, a NaN position, a NaN direction and a zero direction."""
    rng = np.random.default_rng(seed)
    box = np.array(tr.dims, f32) / f32(max(tr.dims))
    pos = (rng.uniform(-0.7, 0.7, (n, 3)) * box).astype(f32)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    pos[0] = 0
    if n > 4:
        d[3] = 0
        pos[4] = (2.0, -3.0, 0.9)
        if nan:                                                             # (fmaxf takes a NaN to cell 0; numpy's maximum keeps it)
            pos[1, 0], d[2, 1] = np.nan, np.nan
    return pos, d


def lookups(tr, bake):
    import torch
    out = []
    for n in (1, 63, 65, 257):
        pos, d = records(tr, n)
        out.append(tr.bake_lookup(bake, torch.from_numpy(pos).cuda(), torch.from_numpy(d).cuda()).cpu().numpy())
    return out


def frames(tr, bake, shard=False):
    sub = tr.baked_render_shard_subframe if shard else tr.baked_render_subframe
    acc = tr.baked_render_shard_accumulate if shard else tr.baked_render_accumulate
    out = []
    for direct in (False, True):
        out.append(sub(bake, SID, rgb_scale=SCALE, direct=direct).cpu().numpy())
        tr.reset()
        acc(bake, 1, 3, rgb_scale=SCALE, direct=direct)
        assert tr.subframes == 3
        out += [tr.mean(), tr.m2()]
        tr.reset()
    return out


MS = ("gather_ms", "network_ms", "mask_ms", "trace_ms", "fold_ms", "test_ms")


def accessors(bake):
    """Everything the contract lists, as {name: array or number}; the ms fields apart."""
    out, ms = {}, {}
    for prefix, d in (("info", bake.info), ("sparse", bake.sparse_info), ("storage", bake.storage_info), ("trace", bake.trace_info()),
                      ("adaptive", bake.adaptive_info())):
        for k, v in d.items():
            (ms if k in MS else out)[f"{prefix}.{k}"] = v
    out["format"] = bake.format
    out["mask"] = bake.mask()
    pos, d = bake.probes()
    out["probes.pos"], out["probes.dir"], out["directions"], out["table"] = pos, d, bake.directions(), bake.table()
    if out["storage.compact"]:
        out["slots"], out["stored"] = bake.slots(), bake.stored_table()
    if out["adaptive.adaptive"]:
        out["counts"], out["m2"] = bake.counts(), bake.m2()
    if bake.format == _lib.CT_BAKE_F16:
        out["half"] = bake.half_table()
    return out, ms


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.atleast_1d(a[k]), np.atleast_1d(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, k
        assert np.array_equal(x.view(np.uint8) if x.dtype.kind == "f" else x, y.view(np.uint8) if y.dtype.kind == "f" else y), k


def reference_bytes(tr, bake, density):
    """write_bake_file_reference of the downloads and the scene: what ct_bake_save must write."""
    i, sp, st, ti, ai = bake.info, bake.sparse_info, bake.storage_info, bake.trace_info(), bake.adaptive_info()
    p = tr.params
    kind = 2 if st["compact"] else 1 if sp["sparse"] else 0
    word = lambda v: int(np.array(v, f32).view(np.uint32))
    h = dict(kind=kind, format=bake.format, traced=int(ti["traced"]), adaptive=int(ai["adaptive"]), grid=i["grid"], azimuths=i["azimuths"],
             cosines=i["cosines"], margin_texels=sp["margin_texels"], entries=i["entries"], stored_entries=st["stored_entries"],
             active_nodes=sp["active_nodes"], light=i["light"], axis_a=i["axis_a"], axis_b=i["axis_b"], dims=tr.dims,
             sample_step_bits=word(p.sample_step), mean_free_path_bits=word(p.mean_free_path_m), cloud_size_bits=word(p.cloud_size_m),
             estimator=p.estimator, tex_fixed8=int(bool(p.flags & _lib.CT_FLAG_TEX_FIXED8)), light_color_bits=[word(c) for c in p.light_color],
             light_intensity_bits=word(p.light_intensity), samples=ti["samples"], paths=ti["paths"], volume_hash=N.volume_hash_reference(density))
    if ai["adaptive"]:
        h.update(round_samples=ai["round_samples"], max_samples=ai["max_samples"], zero_samples=ai["zero_samples"], rel_tol_bits=word(ai["rel_tol"]),
                 abs_tol_bits=word(ai["abs_tol"]), rounds=ai["rounds"], converged=ai["converged"], capped=ai["capped"])
    half = bake.format == _lib.CT_BAKE_F16
    table = bake.half_table() if half else bake.stored_table() if kind == 2 else bake.table()
    return N.write_bake_file_reference(h, table, nodes=bake.mask() if kind else None, m2=bake.m2() if ai["adaptive"] else None,
                                       counts=bake.counts() if ai["adaptive"] else None)


def round_trip(tmp_path, what, kind, small=False, grid=GRID3, **kw):
    """save on one handle, load on a second handle of the same scene: accessors, lookups, frames, bytes."""
    path = tmp_path / "a.bake"
    with tracer(small, **kw) as tr, tracer(small, **kw) as other:
        net = small_net(tr) if what == "net" else None
        try:
            with make(tr, what, kind, grid, net) as bake:
                tr.render_accumulate(1, 2)
                image = (tr.mean(), tr.m2(), tr.subframes, tr.counters())
                bake.save(path)
                assert (tr.subframes, tr.counters()) == image[2:] and np.array_equal(bits(tr.mean()), bits(image[0]))
                tr.reset()
                data = path.read_bytes()
                assert data == reference_bytes(tr, bake, volume(small))
                assert sorted(p.name for p in tmp_path.iterdir()) == ["a.bake"]          # no temporary file is left
                want, want_ms = accessors(bake)
                want_look, want_frames = lookups(tr, bake), frames(tr, bake)
                assert tr.volume_hash() == N.volume_hash_reference(volume(small)) == N.bake_file_info(path)["volume_hash"]
                other.render_accumulate(1, 1)
                before = (other.mean(), other.subframes, other.counters())
                with other.load_bake(path) as loaded:
                    assert (other.subframes, other.counters()) == before[1:] and np.array_equal(bits(other.mean()), bits(before[0]))
                    other.reset()
                    got, got_ms = accessors(loaded)
                    same(got, want)
                    assert got["info.current"] and all(v == 0 for v in got_ms.values()) and got_ms.keys() == want_ms.keys()
                    for a, b in zip(lookups(other, loaded), want_look):
                        assert np.array_equal(bits(a), bits(b))
                    for a, b in zip(frames(other, loaded), want_frames):
                        assert np.array_equal(bits(a), bits(b))
                    assert want_frames[0][..., :3].any() or what == "net"            # (a network's outputs may all be clamped to 0)
                    assert want_frames[3][..., :3].any() and want_frames[4].any()     # with the sun's single scatter: lit pixels
                    loaded.save(tmp_path / "b.bake")
                    assert (tmp_path / "b.bake").read_bytes() == data
                    if what == "net":                                                    # a loaded network bake takes ct_bake_update
                        with small_net(other) as net2:
                            loaded.update(net2)
                            assert np.array_equal(bits(loaded.table()), bits(want["table"]))
                return want
        finally:
            if net is not None:
                net.close()


@pytest.mark.gpu
@pytest.mark.parametrize("what, kind, small", [("net", "dense", False), ("net", "compact", False), ("traced", "dense", False), ("traced", "sparse", False),
                                               ("traced", "compact", False), ("adaptive", "sparse", False), ("adaptive", "compact", False),
                                               ("net", "compact", True), ("traced", "sparse", True), ("adaptive", "compact", True)])
def test_a_loaded_bake_is_the_saved_bake(tmp_path, what, kind, small):
    want = round_trip(tmp_path, what, kind, small)
    assert want["sparse.active_nodes"] == (36 if small else 60)
    assert want["table"].any()


@pytest.mark.gpu
def test_two_polar_nodes_and_the_other_estimator(tmp_path):
    round_trip(tmp_path, "traced", "compact", small=True, grid=GRID2, estimator=DELTA)


@pytest.mark.gpu
def test_shard_frames_of_a_loaded_bake(tmp_path):
    files, seen = [], []
    for index in range(3):
        kw = dict(small=True, w=27, h=13, shard_index=index, shard_count=3)
        with tracer(**kw) as tr, tracer(**kw) as other, make(tr, "traced", "compact") as bake:
            path = tmp_path / f"s{index}.bake"
            bake.save(path)
            files.append(path.read_bytes())
            want = frames(tr, bake, shard=True)
            with other.load_bake(path) as loaded:
                for a, b in zip(frames(other, loaded, shard=True), want):
                    assert np.array_equal(bits(a), bits(b))
            seen.append(any(b.any() for b in want))
    assert any(seen)
    assert files[0] == files[1] == files[2]                                             # point tasks are not pixels


@pytest.mark.gpu
@pytest.mark.parametrize("estimator, flags", [(MARCH, 0), (DELTA, 0), (MARCH, _lib.CT_FLAG_TEX_FIXED8)], ids=["march", "delta", "march-fixed8"])
def test_a_loaded_bake_continues_to_the_bits_of_an_uninterrupted_one(tmp_path, estimator, flags):
    """The sets the adaptive continuation needs, measured on the device (MARCH / DELTA) with network.point_converged_reference on
    the downloaded state: on sphere_volume(32, seed=12) with rel_tol 0.7, 451 / 461 / 452 (fixed8) entries converge by 8
    experiments, 269 / 259 / 268 stop at the cap of 8, and 9 / 9 / 8 of those converge by 16; on SMALL the same tolerance leaves
    none of the capped entries converging by 16, so SMALL (the proper-subset mask) runs with rel_tol 1.5: 408 / 409 / 408
    converged, 24 / 23 / 24 capped, 6 / 5 / 6 of those by 16.  The test asserts only that the three sets are not empty."""
    kw = dict(estimator=estimator, flags=flags)
    with tracer(True, **kw) as tr, tracer(True, **kw) as other:
        # traced(4), save, load, trace_more(3) = traced(7)
        with tr.traced_bake(*GRID3, 4, compact=True) as first, tr.traced_bake(*GRID3, 7, compact=True) as whole:
            first.save(tmp_path / "t.bake")
            with other.load_bake(tmp_path / "t.bake") as loaded:
                loaded.trace_more(3)
                assert np.array_equal(bits(loaded.stored_table()), bits(whole.stored_table())) and whole.stored_table().any()
                assert not np.array_equal(bits(first.stored_table()), bits(whole.stored_table()))
                assert loaded.trace_info()["samples"] == 7 and loaded.trace_info()["paths"] == whole.trace_info()["paths"]
    # adaptive(cap 8), save, load, trace_adaptive_more(16) = adaptive(cap 16)
    for kind, small, tol in (("sparse", False, 0.7), ("compact", False, 0.7), ("sparse", True, 1.5), ("compact", True, 1.5)):
        k, p = {kind: True}, {**P, "rel_tol": tol}
        with tracer(small, **kw) as tr, tracer(small, **kw) as other, tr.traced_bake_adaptive(*GRID3, **p, **k) as first, \
                tr.traced_bake_adaptive(*GRID3, **{**p, "max_samples": 16}, **k) as whole:
            get = (lambda b: b.stored_table()) if kind == "compact" else (lambda b: b.table())
            count = first.counts().reshape(-1)
            live = np.repeat(first.mask().reshape(-1) != 0, 12) if kind == "sparse" else np.arange(count.size) >= 12
            ok = N.point_converged_reference(get(first), first.m2(), first.counts(), tol, p["abs_tol"], p["zero_samples"]).reshape(-1)
            ok16 = N.point_converged_reference(get(whole), whole.m2(), whole.counts(), tol, p["abs_tol"], p["zero_samples"]).reshape(-1)
            at8, final = live & ~ok, whole.counts().reshape(-1)
            assert (final[at8] > 8).all() and (final[live & ok] <= 8).all() and (count[at8] == 8).all()
            sets = (int((live & ok).sum()), int(at8.sum()), int((at8 & ok16).sum()))
            print(f"adaptive sets ({kind}, small {small}, estimator {estimator}, flags {flags}): converged by 8, capped at 8, of those converged by 16 =", sets)
            assert all(v > 0 for v in sets), sets
            assert first.adaptive_info()["capped"] == sets[1]
            first.save(tmp_path / "a.bake")
            with other.load_bake(tmp_path / "a.bake") as loaded:
                assert loaded.adaptive_info()["capped"] == sets[1]
                loaded.trace_adaptive_more(16)
                assert np.array_equal(bits(get(loaded)), bits(get(whole))) and np.array_equal(bits(loaded.m2()), bits(whole.m2()))
                assert np.array_equal(loaded.counts(), whole.counts())
                for key in ("rounds", "converged", "capped", "paths", "max_samples", "entries_active"):
                    assert loaded.adaptive_info()[key] == whole.adaptive_info()[key], key
                assert not np.array_equal(first.counts(), whole.counts())


@pytest.mark.gpu
def test_every_load_refusal(tmp_path):
    path = tmp_path / "t.bake"
    with tracer(small=True) as tr, tr.traced_bake(*GRID3, SAMPLES, sparse=True) as bake:
        bake.save(path)
        want = bake.table()
        start = ct.debug_allocations()

        def refused(other, word, file=path, code=_lib.CT_E_INVAL):
            held = ct.debug_allocations()
            out = C.c_void_p(1)
            assert other.L.ct_bake_load(other.h, os.fsencode(file), C.byref(out)) == code and not out.value
            message = other.L.ct_last_error(other.h).decode()
            assert word in message and "ct_bake_load" in message, (word, message)
            assert ct.debug_allocations() == held                                      # nothing is kept of a refused load

        changed = volume(True).copy()
        z, y, x = np.argwhere(changed > 3)[0]
        changed[z, y, x] -= 1
        for other, word in ((ds.CloudTracer(changed, width=W, height=H), "volume hash"),
                            (ds.CloudTracer(sphere_volume(dims=(48, 48, 50), radius=0.12, seed=12), width=W, height=H), "dims[0]"),
                            (tracer(True, sample_step=1.0 / 256.0), "sample_step"), (tracer(True, estimator=DELTA), "estimator"),
                            (tracer(True, flags=_lib.CT_FLAG_TEX_FIXED8), "CT_FLAG_TEX_FIXED8"), (tracer(True, mean_free_path_m=11.0), "mean_free_path_m"),
                            (tracer(True, cloud_size_m=7001.0), "cloud_size_m"), (tracer(True, flags=_lib.CT_FLAG_SIMPLE_KERNEL), "persistent kernel")):
            with other:
                refused(other, word)
                if word != "persistent kernel":
                    assert "another cloud / estimator" in other.L.ct_last_error(other.h).decode()
        with tracer(True) as other:
            # node bytes edited, the count kept, the checksum put right
            data = bytearray(path.read_bytes())
            info = N.bake_file_info(path)
            mask = np.frombuffer(bytes(data), np.uint8, 60, info["nodes_offset"]).copy()
            on, off = np.flatnonzero(mask)[0], np.flatnonzero(mask == 0)[0]
            mask[on], mask[off] = 0, 1
            data[info["nodes_offset"]:info["nodes_offset"] + 60] = mask.tobytes()
            refused(other, "mask", write(tmp_path, reseal(data), "edited.bake"))
            # what ct_bake_file_info refuses, ct_bake_load refuses
            refused(other, "truncated", write(tmp_path, path.read_bytes()[:-9], "short.bake"))
            refused(other, "cannot open", tmp_path / "missing.bake")
            out = C.c_void_p()
            assert other.L.ct_bake_load(other.h, None, C.byref(out)) == _lib.CT_E_INVAL and other.L.ct_bake_load(other.h, b"x", None) == _lib.CT_E_INVAL
            assert other.L.ct_bake_save(bake.b, os.fsencode(tmp_path / "no" / "such" / "dir.bake")) == _lib.CT_E_INVAL
            assert not (tmp_path / "no").exists()
            # an adaptive file whose capped count is not what its state gives
            with other.traced_bake_adaptive(*GRID3, **P, compact=True) as ad:
                ad.save(tmp_path / "ad.bake")
            raw = bytearray((tmp_path / "ad.bake").read_bytes())
            rec = np.frombuffer(bytes(raw[:256]), N.bake_file_dtype, 1).copy()
            assert rec["capped"][0] > 0
            rec["capped"] -= 1
            rec["converged"] += 1
            raw[:256] = rec.tobytes()
            refused(other, "capped", write(tmp_path, reseal(raw), "ad2.bake"))
            # another light: loads, is not current, renders CT_E_STATE, and ct_bake_retrace makes it current
            other.set_light(LIGHT2)
            with other.load_bake(path) as stale:
                assert not stale.info["current"] and np.array_equal(bits(stale.table()), bits(want))
                assert _code(other.baked_render_subframe, stale, SID) == _lib.CT_E_STATE
                assert _code(stale.trace_more, 1) == _lib.CT_E_STATE
                stale.retrace(SAMPLES)
                assert stale.info["current"] and np.array_equal(stale.info["light"], other.light_direction())
                with other.traced_bake(*GRID3, SAMPLES, sparse=True) as fresh:
                    assert np.array_equal(bits(stale.table()), bits(fresh.table())) and not np.array_equal(bits(fresh.table()), bits(want))
                assert other.baked_render_subframe(stale, SID, rgb_scale=SCALE).cpu().numpy()[..., :3].any()
            # ... and so does another light colour or intensity, with the direction kept
        with tracer(True, light_intensity=2e6) as other, other.load_bake(path) as stale:
            assert not stale.info["current"]
        assert ct.debug_allocations() == start
        assert np.array_equal(bits(bake.table()), bits(want))


@pytest.mark.gpu
def test_every_allocation_of_a_load_is_given_back(tmp_path):
    start = ct.debug_allocations()
    with tracer(True) as tr:
        with tr.traced_bake_adaptive(*GRID3, **P, compact=True) as bake:
            bake.save(tmp_path / "a.bake")
        held = ct.debug_allocations()
        with tr.load_bake(tmp_path / "a.bake") as loaded:
            inside = ct.debug_allocations()
            # nodes, list, slots, table, probe and direction tables, m2, counts, two live lists, wave counts
            assert inside["device_buffers"] == held["device_buffers"] + 11
            loaded.trace_adaptive_more(16)
            assert ct.debug_allocations()["device_buffers"] == inside["device_buffers"]
        assert ct.debug_allocations() == held
    assert ct.debug_allocations() == start


def cli_common(tmp_path):
    from deepestscatter_amd import build
    return [str(build.build_cli()), "procedural:32", "--size", f"{W}x{H}", "--spp", "4", "--net-scale", "0.5,2,3", "--light", "Back", "--net-direct",
            "--out", str(tmp_path)]


@pytest.mark.gpu
def test_cli_saves_a_bake_and_renders_from_the_file(tmp_path):
    from deepestscatter_amd import exr
    common, file, image = cli_common(tmp_path), tmp_path / "cloud.bake", tmp_path / "procedural_32.Back.PT.exr"
    r = subprocess.run(common + ["--traced-bake", "5,4,3,4,3", "--bake-samples", "4", "--net-bake-compact", "--bake-out", str(file)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    first = image.read_bytes()
    image.unlink()
    info = N.bake_file_info(file)
    assert (info["kind"], info["format"], info["traced"], info["samples"], tuple(info["grid"])) == (2, 0, 1, 4, (5, 4, 3))
    r = subprocess.run(common + ["--bake-in", str(file)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert image.read_bytes() == first and exr.read_exr(image).any()
    with ds.CloudTracer(ds.make_procedural_cloud(32), width=W, height=H, light_direction=ds.LIGHT_DIRECTIONS["Back"]) as tr, tr.load_bake(file) as bake:
        tr.baked_render_accumulate(bake, 1, 4, rgb_scale=SCALE, direct=True)
        assert np.array_equal(bits(exr.read_exr(image)), bits(tr.mean()[..., :3]))
    # contradictions stop before any device
    for extra, word in ((["--bake-in", str(file), "--traced-bake", "5,4,3,4,3"], "--traced-bake"), (["--bake-out", str(file)], "--bake-out"),
                        (["--bake-in", str(file), "--bake-out", str(file)], "same file"), (["--bake-in", str(tmp_path / "none.bake")], "cannot open")):
        r = subprocess.run(common + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and word in r.stdout + r.stderr, (extra, r.stdout + r.stderr)
