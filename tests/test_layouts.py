"""The volume layouts that ct_create builds on the device, byte for byte (run with -m gpu on an MI355X).

The oracle marches every step and has none of these structures, so a frame that equals the oracle's says nothing about a
value in them that is too conservative, and little about one that is too generous where no sampled path went.  Here every
layout is read back (ct_debug_layout) and compared, with exact integer equality, with a numpy reference written from the
definitions in the DevScene comments of csrc/ct_device.hpp:

  apron bricks (density, shadow)  texels, majorant byte, free-space distance and interior flag
  march bricks, dense             texels, and per row the clearance (bits 0-5) and the interior flag (bit 7) of the meta byte
                                  (bit 6, shadow-zero, is tests/test_nee_skip.py's)
  march bricks, sparse            row table, compact bricks, coarse clearance grid
  twin bricks                     both halves
  majorant grid (DELTA)           geometry, cells, codes, the zero cells outside the stored box, the magic division

The clearances are also held to the two properties that define them, stated on a summed-area table of the blocked base
texels and not on the distance transform: a row's clearance is safe, and one more texel would not be.
"""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
import deepestscatter_amd as ds
from deepestscatter_amd import _lib

pytestmark = pytest.mark.gpu

CLEAR_CAP = 63        # a row's clearance: 6 bits
STEP = 1.0 / 512.0    # the reference's sample step


# ---- volumes: the smallest at which each thing can go wrong --------------------------------------------------------------
def _blobs(shape, seed, count, rmax, margin):
    rng = np.random.default_rng(seed)
    vol = np.zeros(shape, np.uint8)
    zz, yy, xx = np.ogrid[0:shape[0], 0:shape[1], 0:shape[2]]
    for _ in range(count):
        c = [int(rng.integers(margin, n - margin)) for n in shape]
        r = float(rng.uniform(1.0, rmax))
        m = (zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= r * r
        vol[m] = rng.integers(1, 256, int(m.sum())).astype(np.uint8)
    return vol


def _vol_blobs():
    """No dimension is a multiple of 3 or 4; blobs with free space between them."""
    return _blobs((37, 41, 50), 3, 7, 5.0, 5)


def _vol_faces():
    """Non-zero texels on every face (and free space inside): clamp addressing, the interior flags, out-of-grid = blocked."""
    rng = np.random.default_rng(5)
    vol = _blobs((20, 28, 36), 4, 2, 3.0, 6)
    vol[0, 3:9, 4:12] = rng.integers(1, 256, (6, 8))
    vol[-1, 15:25, 20:35] = rng.integers(1, 256, (10, 15))
    vol[2:7, 0, 10:30] = rng.integers(1, 256, (5, 20))
    vol[12:19, -1, 0:9] = rng.integers(1, 256, (7, 9))
    vol[8:12, 5:11, 0] = rng.integers(1, 256, (4, 6))
    vol[1:6, 20:27, -1] = rng.integers(1, 256, (5, 7))
    vol[-1, -1, -1] = 255
    vol[0, 0, 0] = 1
    return vol


def _vol_zero():
    return np.zeros((14, 17, 22), np.uint8)


def _vol_one_texel():
    vol = np.zeros((14, 17, 22), np.uint8)
    vol[1, 1, 1] = 200
    return vol


def _vol_cap():
    """136^3, empty but for a blob at one corner: the clearance cap of 63 needs 64 free base texels on both sides of a base on
    every axis, i.e. axes of 130 texels or more."""
    vol = np.zeros((136, 136, 136), np.uint8)
    vol[2:6, 2:6, 2:6] = np.random.default_rng(6).integers(1, 256, (4, 4, 4))
    return vol


def _vol_long():
    """Long in x: large x indices, the march bricks' own x bias, a long majorant grid."""
    rng = np.random.default_rng(8)
    vol = np.zeros((12, 12, 2048), np.uint8)
    for x0, x1 in ((3, 7), (1000, 1009), (2040, 2045)):
        vol[4:8, 3:7, x0:x1] = rng.integers(1, 256, (4, 4, x1 - x0))
    vol[5, 5, 1500] = 9
    return vol


def _vol_big():
    """(192, 200, 208): more than 65536 * 256 bytes of apron and of twin bricks, so their launchers' grid-stride loops run a second
    trip.  A quarter of its 16^3 cells, faces included, hold a pattern in which neighbouring texels differ."""
    shape = (192, 200, 208)
    rng = np.random.default_rng(9)
    cells = rng.random((12, 13, 13)) < 0.25
    cells[0, 0, 0] = cells[-1, -1, -1] = cells[0, 6, 12] = cells[11, 0, 5] = True
    mask = np.repeat(np.repeat(np.repeat(cells, 16, 0), 16, 1), 16, 2)[:shape[0], :shape[1], :shape[2]]
    z, y, x = np.ogrid[0:shape[0], 0:shape[1], 0:shape[2]]
    return (((z * 131 + y * 31 + x * 7) % 251 + 1) * mask).astype(np.uint8)


# name -> (builder, sample step).  The apron around a volume grows with its longest axis; the long volume takes one texel
# per step so that its short axes are not all apron.
VOLUMES = {
    "blobs": (_vol_blobs, STEP), "faces": (_vol_faces, STEP), "zero": (_vol_zero, STEP), "one_texel": (_vol_one_texel, STEP),
    "cap": (_vol_cap, STEP), "long": (_vol_long, 1.0 / 2048.0), "big": (_vol_big, STEP),
    "cloud128": (lambda: ds.make_procedural_cloud(128), STEP), "cloud224": (lambda: ds.make_procedural_cloud(224), STEP),
}
_cache = {}


def volume(name):
    if ("vol", name) not in _cache:
        v = np.ascontiguousarray(VOLUMES[name][0](), np.uint8)
        v.setflags(write=False)
        _cache["vol", name] = v
    return _cache["vol", name]


def tracer(name, **kw):
    return ds.CloudTracer(volume(name), width=16, height=16, sample_step=VOLUMES[name][1], **kw)


# ---- numpy building blocks ----------------------------------------------------------------------------------------------
def expand(vol, lo, length):
    """The clamp-to-edge texels [lo, lo + length) per axis (z, y, x)."""
    idx = [np.clip(np.arange(l, l + m), 0, n - 1) for l, m, n in zip(lo, length, vol.shape)]
    return vol[np.ix_(*idx)]


def windows(a, axis, stride, width, count, op):
    """out[c] = op over k < width of a[stride * c + k], along one axis."""
    out = None
    for k in range(width):
        sl = [slice(None)] * a.ndim
        sl[axis] = slice(k, k + stride * (count - 1) + 1, stride)
        s = a[tuple(sl)]
        out = s.copy() if out is None else op(out, s)
    return out


def erode(a):
    """a[p] and all of its 26 neighbours; positions outside the array count as False."""
    for axis in range(3):
        b = a.copy()
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        b[tuple(hi)] &= a[tuple(lo)]
        b[tuple(lo)] &= a[tuple(hi)]
        first = [slice(None)] * 3
        last = [slice(None)] * 3
        first[axis], last[axis] = 0, -1
        b[tuple(first)] = False
        b[tuple(last)] = False
        a = b
    return a


def capped_chebyshev(free, cap):
    """min(cap, Chebyshev distance to the nearest position that is not free); positions outside the array are not free.
    Brute force from the definition: the distance exceeds k exactly when everything within k is free."""
    dist = np.zeros(free.shape, np.int32)
    cur = free.copy()
    for _ in range(cap):
        if not cur.any():
            break
        dist += cur
        cur = erode(cur)
    return dist


def interior_axis(lo, hi, n):
    return (lo >= 1) & (hi <= n - 3)


def outer_and(z, y, x):
    return z[:, None, None] & y[None, :, None] & x[None, None, :]


def blocked_bases(vol):
    """A base texel is blocked when it is not in [1, N-3]^3 or its 2x2x2 footprint holds a non-zero texel."""
    nz, ny, nx = vol.shape
    s = vol != 0
    f = s.copy()
    f[:, :, :-1] |= s[:, :, 1:]
    g = f.copy()
    g[:, :-1, :] |= f[:, 1:, :]
    f = g.copy()
    f[:-1, :, :] |= g[1:, :, :]
    inside = outer_and(*[interior_axis(np.arange(n), np.arange(n), n) for n in (nz, ny, nx)])
    return f | ~inside, inside


def base_tables(name):
    """Per base texel of a volume: blocked, interior, and the clearance max(0, min(64, distance to a blocked base) - 1).
    Computed once per volume and shared."""
    if ("bases", name) not in _cache:
        blocked, inside = blocked_bases(volume(name))
        dist = capped_chebyshev(~blocked, CLEAR_CAP + 1)
        clear = np.maximum(dist - 1, 0).astype(np.uint8)
        for a in (blocked, inside, clear):
            a.setflags(write=False)
        _cache["bases", name] = (blocked, inside, clear)
    return _cache["bases", name]


def padded(a, lo, shape):
    """`a` (indexed by texel) in an array that covers the texels [lo, lo + shape) per axis; zero / False outside the volume."""
    out = np.zeros(shape, a.dtype)
    out[tuple(slice(-l, -l + n) for l, n in zip(lo, a.shape))] = a
    return out


# ---- references ----------------------------------------------------------------------------------------------------------
def apron_texels_reference(vol, g):
    """Byte lz*25 + ly*5 + lx of brick b = the clamp-to-edge texel 4b - bias + l; bytes 125..127 zero."""
    gx, gy, gz = g["bricks"]
    e = expand(vol, (-g["bias"],) * 3, (4 * gz + 1, 4 * gy + 1, 4 * gx + 1))
    out = np.zeros((gz, gy, gx, 128), np.uint8)
    for lz in range(5):
        for ly in range(5):
            for lx in range(5):
                out[..., lz * 25 + ly * 5 + lx] = e[lz:lz + 4 * gz - 3:4, ly:ly + 4 * gy - 3:4, lx:lx + 4 * gx - 3:4]
    return out


def density_meta_reference(vol, g):
    """(byte 125, byte 126) of every density brick: free-space distance | interior << 7, majorant."""
    gx, gy, gz = g["bricks"]
    bias = g["bias"]
    m = expand(vol, (-bias - 1,) * 3, (4 * gz + 3, 4 * gy + 3, 4 * gx + 3))      # texels [lo - 1, lo + 5] of brick b at 4b .. 4b + 6
    for axis, n in enumerate((gz, gy, gx)):
        m = windows(m, axis, 4, 7, n, np.maximum)
    inter = outer_and(*[interior_axis(4 * np.arange(n) - bias, 4 * np.arange(n) - bias + 3, t) for n, t in zip((gz, gy, gx), vol.shape)])
    dist = capped_chebyshev((m == 0) & inter, 127)
    return (dist | (inter.astype(np.int32) << 7)).astype(np.uint8), m, int(dist.max())


def march_reference(name, g):
    """The dense march bricks without bit 6 of the meta bytes, and the rows' clearance and interior flag [z, y, brick x]."""
    vol = volume(name)
    gx, gy, gz = g["bricks"]
    bias, bias_x = g["bias"], g["bias_x"]
    _, inside, clear = base_tables(name)
    e = expand(vol, (-bias, -bias, -bias_x), (4 * gz + 1, 4 * gy + 1, 3 * gx + 1))
    out = np.zeros((gz, gy, gx, 128), np.uint8)
    for lz in range(5):
        for ly in range(5):
            for lx in range(4):     # texels of the columns 3bx - bias_x + lx
                out[..., lz * 25 + ly * 5 + lx] = e[lz:lz + 4 * gz - 3:4, ly:ly + 4 * gy - 3:4, lx:lx + 3 * gx - 2:3]
    lo, shape = (-bias, -bias, -bias_x), (4 * gz, 4 * gy, 3 * gx)
    row_clear = padded(clear, lo, shape).reshape(4 * gz, 4 * gy, gx, 3).min(-1)          # a base outside the volume gives 0
    row_inter = padded(inside, lo, shape).reshape(4 * gz, 4 * gy, gx, 3).all(-1)
    meta = row_clear | (row_inter.astype(np.uint8) << 7)
    for lz in range(4):
        for ly in range(4):
            out[..., lz * 25 + ly * 5 + 4] = meta[lz::4, ly::4, :]
    return out, row_clear, row_inter


def row_meta(bricks):
    """[z, y, brick x] meta bytes of dense march bricks [bz, by, bx, 128]."""
    gz, gy, gx, _ = bricks.shape
    meta = np.zeros((4 * gz, 4 * gy, gx), np.uint8)
    for lz in range(4):
        for ly in range(4):
            meta[lz::4, ly::4, :] = bricks[..., lz * 25 + ly * 5 + 4]
    return meta


META_BYTES = np.array([o < 125 and o % 5 == 4 and o % 25 < 20 and o < 100 for o in range(128)])
TEXEL_BYTES = np.array([o < 125 and o % 5 != 4 for o in range(128)])


def boxes_clear(blocked, z, y, x0, r):
    """For rows of base texels (x0 .. x0 + 2, y, z) and a radius r per row: True where every base within Chebyshev distance r of
    the row's bases lies in the volume and is not blocked (its footprint is all zero and it is interior).  Counted on a
    summed-area table."""
    nz, ny, nx = blocked.shape
    sat = np.zeros((nz + 1, ny + 1, nx + 1), np.int64)
    sat[1:, 1:, 1:] = blocked.astype(np.int64).cumsum(0).cumsum(1).cumsum(2)
    zl, zh, yl, yh, xl, xh = z - r, z + r + 1, y - r, y + r + 1, x0 - r, x0 + r + 3       # [l, h)
    inside = (zl >= 0) & (yl >= 0) & (xl >= 0) & (zh <= nz) & (yh <= ny) & (xh <= nx)
    zl, zh = np.clip(zl, 0, nz), np.clip(zh, 0, nz)
    yl, yh = np.clip(yl, 0, ny), np.clip(yh, 0, ny)
    xl, xh = np.clip(xl, 0, nx), np.clip(xh, 0, nx)
    count = (sat[zh, yh, xh] - sat[zl, yh, xh] - sat[zh, yl, xh] - sat[zh, yh, xl]
             + sat[zl, yl, xh] + sat[zl, yh, xl] + sat[zh, yl, xl] - sat[zl, yl, xl])
    return inside & (count == 0)


def twin_reference(vol, shadow, g):
    """Bytes lz*16 + ly*4 + lx of brick b = the clamp-to-edge DENSITY texel 3b - bias + l, bytes 64.. the shadow volume's."""
    gx, gy, gz = g["bricks"]
    out = np.zeros((gz, gy, gx, 128), np.uint8)
    for half, v in enumerate((vol, shadow)):
        e = expand(v, (-g["bias"],) * 3, (3 * gz + 1, 3 * gy + 1, 3 * gx + 1))
        for lz in range(4):
            for ly in range(4):
                for lx in range(4):
                    out[..., 64 * half + lz * 16 + ly * 4 + lx] = e[lz:lz + 3 * gz - 2:3, ly:ly + 3 * gy - 2:3, lx:lx + 3 * gx - 2:3]
    return out


def majorant_reference(vol, cell, bias, origin, count):
    """(max, code) of the cells origin .. origin + count of the virtual grid (x, y, z): over the clamped texels [lo - 1, lo + C + 1]^3,
    lo = C * cell index - bias; code = min(3, 4 * min // max), 0 for an all-zero cell."""
    lo = [cell * o - bias - 1 for o in origin[::-1]]
    n = count[::-1]
    e = expand(vol, lo, [cell * c + 3 for c in n])
    hi, low = e, e
    for axis in range(3):
        hi = windows(hi, axis, cell, cell + 3, n[axis], np.maximum)
        low = windows(low, axis, cell, cell + 3, n[axis], np.minimum)
    code = np.minimum(3, 4 * low.astype(np.int32) // np.maximum(hi, 1))
    return hi, np.where(hi > 0, code, 0).astype(np.uint8)


# ---- apron bricks --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["blobs", "faces", "zero", "one_texel", "cap", "long", "big"])
def test_apron_bricks(name):
    """Density and shadow apron bricks: every texel byte, the majorant byte 126, the free-space distance and the interior
    flag of byte 125, and the zero bytes.  The brick distance is capped at 64 bricks, which only a volume of about 520^3 can
    reach: the cap is left out, and the test asserts that no reference distance comes near it."""
    vol = volume(name)
    tr = tracer(name)
    dens, g = tr.layout("density_bricks")
    shad, gs = tr.layout("shadow_bricks")
    shadow = tr.inscatter()
    tr.close()
    assert gs == g and g["bias"] % 4 == 0 and g["bias"] > 0
    assert all(4 * b >= n + 2 * g["bias"] for b, n in zip(g["bricks"], vol.shape[::-1]))
    assert dens.shape == shad.shape == (*g["bricks"][::-1], 128)
    ref = apron_texels_reference(vol, g)
    assert np.array_equal(dens[..., :125], ref[..., :125])
    assert np.array_equal(shad, apron_texels_reference(shadow, g))        # bytes 125..127 of the shadow bricks: 0
    meta, majorant, dmax = density_meta_reference(vol, g)
    assert dmax < 64
    assert np.array_equal(dens[..., 126], majorant)
    assert np.array_equal(dens[..., 125] >> 7, meta >> 7)
    assert np.array_equal(dens[..., 125] & 0x7f, meta & 0x7f)
    assert not dens[..., 127].any()
    if name == "big":
        assert dens.size > 65536 * 256


# ---- march bricks --------------------------------------------------------------------------------------------------------
MARCH_VOLUMES = ["blobs", "faces", "zero", "one_texel", "cap", "long"]


@pytest.mark.parametrize("name", MARCH_VOLUMES)
def test_march_bricks_dense(name):
    """Texel bytes, and bits 0-5 and 7 of every row's meta byte, against the brute-force capped Chebyshev transform; then the
    two properties that define a clearance c, on the device's own bytes: SAFE -- every base within Chebyshev distance c of
    the row's three bases lies in the volume, is interior and has an all-zero footprint; OPTIMAL -- for c < 63 that fails at
    c + 1.  (c = 0 promises nothing, so safety is asserted for c >= 1.)"""
    vol = volume(name)
    tr = tracer(name)
    bricks, g = tr.layout("march_bricks")
    tr.close()
    gx, gy, gz = g["bricks"]
    assert not g["sparse"] and g["bias_x"] % 3 == 0 and g["bias"] % 4 == 0 and bricks.shape == (gz, gy, gx, 128)
    assert 3 * gx >= vol.shape[2] + 2 * g["bias_x"]
    ref, row_clear, row_inter = march_reference(name, g)
    assert np.array_equal(bricks[..., TEXEL_BYTES], ref[..., TEXEL_BYTES])
    assert not bricks[..., ~(TEXEL_BYTES | META_BYTES)].any()
    meta = row_meta(bricks)
    clear = (meta & 0x3f).astype(np.int64)
    assert np.array_equal(meta >> 7, row_inter.astype(np.uint8))
    if name == "cap":
        assert (row_clear == CLEAR_CAP).any() and np.array_equal(clear == CLEAR_CAP, row_clear == CLEAR_CAP)
    assert np.array_equal(clear, row_clear)
    assert not ((meta & 0x40) != 0)[clear != 0].any()              # shadow-zero is given to rows of clearance 0 only
    blocked, _, _ = base_tables(name)
    z = (np.arange(4 * gz) - g["bias"])[:, None, None]
    y = (np.arange(4 * gy) - g["bias"])[None, :, None]
    x0 = (3 * np.arange(gx) - g["bias_x"])[None, None, :]
    safe = boxes_clear(blocked, z, y, x0, clear)
    assert safe[clear >= 1].all()
    further = boxes_clear(blocked, z, y, x0, clear + 1)
    assert not further[clear < CLEAR_CAP].any()


@pytest.mark.parametrize("name", MARCH_VOLUMES)
def test_march_bricks_sparse(name, monkeypatch):
    """CT_SPARSE=1 next to a dense handle of the same volume: the row table holds the first brick and the number of bricks up
    to the last one with a non-zero texel byte, starts are the prefix sums, an empty row is (start, 0); the compact array is
    the dense one inside the extents, in order; a coarse cell holds the minimum clearance and the AND of the interior flags
    of its 8^3 base texels, a base outside the volume being blocked and not interior."""
    vol = volume(name)
    tr = tracer(name)
    dense, g = tr.layout("march_bricks")
    with pytest.raises(_lib.CloudTraceError) as e:
        tr.layout("march_rows")
    assert e.value.code == _lib.CT_E_INVAL
    with pytest.raises(_lib.CloudTraceError) as e:
        tr.layout("march_coarse")
    assert e.value.code == _lib.CT_E_INVAL
    tr.close()
    monkeypatch.setenv("CT_SPARSE", "1")
    sp = tracer(name)
    compact, gs = sp.layout("march_bricks")
    rows, gr = sp.layout("march_rows")
    coarse, gc = sp.layout("march_coarse")
    sp.close()
    gx, gy, gz = g["bricks"]
    assert gs == {**g, "sparse": True} and gr["rows"] == (gy, gz) and rows.shape == (gz, gy, 2)
    ref, _, _ = march_reference(name, g)
    nonzero = (ref[..., TEXEL_BYTES] != 0).any(-1)                   # [bz, by, bx]
    has = nonzero.any(-1)
    first = np.where(has, nonzero.argmax(-1), 0)
    last = np.where(has, gx - 1 - nonzero[..., ::-1].argmax(-1), -1)
    count = np.where(has, last - first + 1, 0)
    start = np.concatenate([[0], np.cumsum(count.ravel())[:-1]]).reshape(gz, gy)
    assert np.array_equal(rows[..., 0], start)
    assert np.array_equal(rows[..., 1], np.where(has, first | (count << 16), 0))
    bx = np.arange(gx)
    stored = (bx >= first[..., None]) & (bx < (first + count)[..., None])
    assert compact.shape == (int(count.sum()), 128)
    assert np.array_equal(compact, dense[stored])
    assert not dense[~stored][:, TEXEL_BYTES].any()                  # what is left out holds no texel
    # the coarse clearance grid
    _, inside, clear = base_tables(name)
    edge = 1 << gc["shift"]
    cx, cy, cz = gc["cells"]
    assert edge == 8 and gc["bias"] == g["bias"] and coarse.shape == (cz, cy, cx)
    assert all(edge * c >= n + 2 * g["bias"] for c, n in zip((cz, cy, cx), vol.shape))
    lo, shape = (-g["bias"],) * 3, (edge * cz, edge * cy, edge * cx)
    want_clear = padded(clear, lo, shape).reshape(cz, edge, cy, edge, cx, edge).min((1, 3, 5))
    want_inter = padded(inside, lo, shape).reshape(cz, edge, cy, edge, cx, edge).all((1, 3, 5))
    assert np.array_equal(coarse & 0x3f, want_clear)
    assert np.array_equal(coarse >> 6, want_inter.astype(np.uint8) << 1)


# ---- twin bricks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["blobs", "faces", "one_texel", "big"])
def test_twin_bricks(name, monkeypatch):
    """DELTA handle with the twin layout forced (CT_DELTA_NEE=2): both 64-byte halves against the clamped density and the
    clamped shadow volume."""
    monkeypatch.setenv("CT_DELTA_NEE", "2")
    vol = volume(name)
    tr = tracer(name, estimator=1)
    assert tr.delta_grid()["nee"] == 2
    twin, g = tr.layout("twin_bricks")
    shadow = tr.inscatter()
    tr.close()
    assert g["bias"] % 3 == 0 and g["bias"] > 0 and twin.shape == (*g["bricks"][::-1], 128)
    assert all(3 * b >= n + 2 * g["bias"] for b, n in zip(g["bricks"], vol.shape[::-1]))
    assert np.array_equal(twin, twin_reference(vol, shadow, g))
    if name == "big":
        assert twin.size > 65536 * 256


def test_layouts_a_handle_does_not_have(monkeypatch):
    """Twin bricks and the majorant grid on a MARCH handle, twin bricks on a DELTA handle with another fetch layout, an unknown
    layout and a capacity that is too small answer CT_E_INVAL; a NULL destination returns size and geometry only."""
    tr = tracer("blobs")
    for which in ("twin_bricks", "majorant_cells", "majorant_codes", 9, -1):
        with pytest.raises(_lib.CloudTraceError) as e:
            tr.layout(which)
        assert e.value.code == _lib.CT_E_INVAL
    geom, n = np.zeros(16, np.uint32), C.c_size_t(0)
    assert tr.L.ct_debug_layout(tr.h, _lib.CT_LAYOUT_DENSITY_BRICKS, geom.ctypes.data_as(C.c_void_p), None, 0, C.byref(n)) == _lib.CT_OK
    assert n.value == 128 * int(geom[1]) * int(geom[2]) * int(geom[3]) > 0
    buf = np.full(n.value, 0xAB, np.uint8)
    rc = tr.L.ct_debug_layout(tr.h, _lib.CT_LAYOUT_DENSITY_BRICKS, geom.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p),
                              n.value - 1, C.byref(n))
    assert rc == _lib.CT_E_INVAL and (buf == 0xAB).all()
    tr.close()
    monkeypatch.setenv("CT_DELTA_NEE", "1")
    tr = tracer("blobs", estimator=1)
    with pytest.raises(_lib.CloudTraceError) as e:
        tr.layout("twin_bricks")
    assert e.value.code == _lib.CT_E_INVAL
    tr.close()


# ---- the DELTA estimator's majorant grid ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["blobs", "faces", "zero", "one_texel", "long", "cloud128", "cloud224"])
def test_majorant_grid(name):
    """Geometry = orc_majorant_grid; cells and codes = orc_build_majorants = numpy's max and min(3, 4 * min // max) over
    [lo - 1, lo + C + 1]^3; every virtual cell outside the stored box reads zeros only; and the kernel's division by the cell edge,
    (x * mc_div) >> 20 with a 24-bit multiply, is exact for every texel index of the grid.
    The procedural cloud at 128^3 has cells with all four codes, but its stored box fits with 4-texel cells (25 x 18 x 22), as
    does every size up to 208^3; 224^3 is the smallest whose cell edge, 5, is no power of two, so that mc_div is a real magic
    number: that is asserted there as a precondition."""
    vol = volume(name)
    step = VOLUMES[name][1]
    tr = tracer(name, estimator=1)
    cells, g = tr.layout("majorant_cells")
    codes, gc = tr.layout("majorant_codes")
    apron_bias = tr.layout("density_bricks")[1]["bias"]
    tr.close()
    L = O.lib(True)
    dims = np.array(vol.shape[::-1], np.uint32)
    grid = np.zeros(11, np.int32)
    L.orc_majorant_grid(O._ptr(vol), O._ptr(dims), step, O._ptr(grid))
    cell, bias = g["cell"], g["bias"]
    assert gc == g and bias == apron_bias
    assert (bias, cell, g["origin"], g["stored"], g["virtual"]) == (int(grid[0]), int(grid[1]), tuple(int(v) for v in grid[2:5]),
                                                                    tuple(int(v) for v in grid[5:8]), tuple(int(v) for v in grid[8:11]))
    if name == "cloud224":
        assert cell not in (4, 8, 16)
    sx, sy, sz = g["stored"]
    assert cells.shape == codes.shape == (sz, sy, sx)
    origin = np.ascontiguousarray(grid[2:5])
    orc_cells, orc_codes = np.empty_like(cells), np.empty_like(codes)
    L.orc_build_majorants(O._ptr(vol), O._ptr(dims), bias, cell, O._ptr(origin), sx, sy, sz, O._ptr(orc_cells), O._ptr(orc_codes))
    assert np.array_equal(cells, orc_cells) and np.array_equal(codes, orc_codes)
    want_cells, want_codes = majorant_reference(vol, cell, bias, g["origin"], g["stored"])
    assert np.array_equal(cells, want_cells) and np.array_equal(codes, want_codes)
    # the virtual grid covers [-bias, n + bias); outside the stored box everything a cell can read is zero
    assert all(cell * v >= n + 2 * bias for v, n in zip(g["virtual"], vol.shape[::-1]))
    assert all(o + s <= v for o, s, v in zip(g["origin"], g["stored"], g["virtual"]))
    everything, _ = majorant_reference(vol, cell, bias, (0, 0, 0), g["virtual"])
    ox, oy, oz = g["origin"]
    outside = np.ones(everything.shape, bool)
    outside[oz:oz + sz, oy:oy + sy, ox:ox + sx] = False
    assert not everything[outside].any()
    if vol.any():      # ... and the box is tight: its six outer layers of cells each read a non-zero texel
        assert all(cells.take(i, axis).any() for axis in range(3) for i in (0, -1))
    # (x * mc_div) >> 20 == x // mc_cell, in 64 bits; then what __umul24 and a 32-bit product need
    div = g["div"]
    x = np.arange(max(vol.shape) + 2 * bias, dtype=np.int64)
    assert np.array_equal((x * div) >> 20, x // cell)
    assert int(x[-1]) * div < 2 ** 32 and int(x[-1]) < 2 ** 24 and div < 2 ** 24
