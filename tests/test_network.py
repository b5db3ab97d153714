"""ct_network_eval: the scattering network (include/cloudtrace.h, "the scattering network") run on descriptor records by one
fused bf16 MFMA kernel.

The device is held to `reference_forward(accumulate=np.float64)` of deepestscatter_amd/network.py, the rounded model in numpy.
Tolerance, per case: with R64 that reference and R32 the same restatement summing in float32,
    e_ref = max |R32 - R64| / (1 + |R64|)        and the device must satisfy      max |dev - R64| / (1 + |R64|) <= 8 e_ref.
The device sums a layer in another order than numpy, and a differing float32 sum can flip a bf16 rounding that later layers
carry on; 8 x covers that and still catches a wrong column, which moves outputs by orders of magnitude more.
Weights are seeded uniform in +-1/sqrt(fan_in), inputs random bytes from a fixed seed; references are computed once per
process and shared."""
import ctypes as C

import numpy as np
import pytest

import deepestscatter_amd as ds
from deepestscatter_amd import _lib
from deepestscatter_amd import network as N

SENTINEL = -12345.0
TIES = [0.0, -0.0, 1.0, 1.00390625, 1.01171875, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20,
        1.0 + 2.0 ** -8 - 2.0 ** -20, -1.00390625, -1.01171875, 255.5, 256.5 * 2, 3.4028234663852886e38, 1e-40, 2.0 ** -133,
        float("inf"), float("-inf")]
# what round-to-nearest-even gives for the first eleven, by hand: 1 + 2^-8 is a tie between 1 and 1 + 2^-7 whose even
# neighbour is 1; 1 + 3 * 2^-8 a tie between 1 + 2^-7 (odd) and 1 + 2^-6 (even)
TIES_ROUNDED = [0.0, -0.0, 1.0, 1.0, 1.015625, 1.0, 1.015625, 1.0078125, 1.0, -1.0, -1.015625]


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


_CACHE = {}


def case(width, aux, head, count, seed=1, kind="random"):
    """-> (shape, weights, bytes [count, 2250], aux [count, A], R64, R32), computed once."""
    key = (width, aux, head, count, seed, kind)
    if key not in _CACHE:
        shape = N.NetworkShape(width, aux, head)
        w = seeded_weights(shape, seed)
        rng = np.random.default_rng(1000 + seed)
        if kind == "random":
            b = rng.integers(0, 256, (count, N.RECORD_BYTES), dtype=np.uint8)
        elif kind == "onehot":
            assert count == N.RECORD_BYTES
            b = np.zeros((count, N.RECORD_BYTES), np.uint8)
            b[np.arange(count), np.arange(count)] = 255
        else:
            b = np.zeros((count, N.RECORD_BYTES), np.uint8)
        a = rng.uniform(-1, 1, (count, aux)).astype(np.float32)
        r64 = N.reference_forward(w, shape, b, a, accumulate=np.float64)
        r32 = N.reference_forward(w, shape, b, a, accumulate=np.float32)
        _CACHE[key] = (shape, w, b, a, r64, r32)
    return _CACHE[key]


def rel_err(x, r64):
    return float(np.max(np.abs(np.asarray(x, np.float64) - r64) / (1.0 + np.abs(r64))))


def flagship(count):
    """The first `count` records of the one (200, 1, 3) case of 1000 records (records are independent of each other)."""
    shape, w, b, a, r64, r32 = case(200, 1, 3, 1000)
    return shape, w, b[:count], a[:count], r64[:count], r32[:count]


# ---------------------------------------------------------------------------------------------------- CPU
def test_reference_without_rounding_is_the_torch_module():
    """Packing order and architecture: the numpy restatement with its rounding switched off is ScatterNet.forward."""
    import torch
    for width, aux, head in [(200, 1, 3), (32, 0, 1), (16, 8, 4)]:
        torch.manual_seed(5)
        net = N.ScatterNet(width, aux, head)
        rng = np.random.default_rng(3)
        b = rng.integers(0, 256, (7, 10, 9, 5, 5), dtype=np.uint8)
        a = rng.uniform(-1, 1, (7, aux)).astype(np.float32)
        flat = N.pack_weights(net)
        got = N.reference_forward(flat, net.shape, b, a, accumulate=np.float64, rounding=False)
        with torch.no_grad():
            want = net.double()(torch.from_numpy(b), torch.from_numpy(a).double() if aux else None).numpy()
        assert want.shape == (7,) and np.abs(want).max() > 1e-3
        assert rel_err(got, want) <= 1e-12


def test_pack_weights_length_is_the_formula():
    for width, aux, head in [(200, 1, 3), (32, 0, 1), (16, 8, 4)]:
        n = (width * (225 + aux) + 9 * width * (width + 225 + aux) + 10 * (width * width + 2 * width)
             + (head - 1) * (width * width + width) + width + 1)
        assert N.NetworkShape(width, aux, head).weight_count() == n
        assert N.pack_weights(N.ScatterNet(width, aux, head)).shape == (n,)
    # a state dict round-trips by the documented names
    names = set(N.ScatterNet(16, 0, 2).state_dict())
    assert {"blocks.0.fc1.weight", "blocks.9.fc2.bias", "head.0.weight", "out.bias"} <= names


def test_bf16_helper_rounds_to_nearest_even():
    got = N.bf16_round(np.array(TIES, np.float32))
    assert np.array_equal(got[:len(TIES_ROUNDED)], np.array(TIES_ROUNDED, np.float32))
    assert np.array_equal(np.signbit(got[:2]), [False, True])
    assert got[11] == 255.0 + 1.0 and got[12] == 512.0                      # 255.5 -> 256 (a tie, 256 is even), 513 -> 512
    assert np.isinf(got[13])                                                # the largest float32 rounds up to infinity
    assert np.isinf(got[16]) and np.isinf(got[17]) and got[17] < 0
    assert np.isnan(N.bf16_round(np.array([np.nan], np.float32))[0])
    assert np.all((got.view(np.uint32) & 0xFFFF) == 0)


def test_bf16_round_of_the_library_equals_the_helper(product_lib):
    rng = np.random.default_rng(17)
    x = np.concatenate([rng.integers(0, 2 ** 32, 10000, dtype=np.uint64).astype(np.uint32).view(np.float32),
                        np.array(TIES, np.float32)])
    want = N.bf16_round(x)
    got = np.array([product_lib.ct_debug_bf16_round(float(v)) for v in x], np.float32)
    nan = np.isnan(x)
    assert nan.any() and np.isnan(got[nan]).all() and np.isnan(want[nan]).all()
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


ZERO_CASE = dict(width=200, aux=0, head=3, count=65, seed=2, kind="zero")


def test_reference_errors_are_not_zero():
    """Every e_ref the GPU tests multiply by 8 is a positive number, and 8 e_ref is no tighter than what storing the output as
    a float32 costs (half an ulp of it) -- a bound below that would test the output format, not the kernel.  The all-zero
    case is one record 65 times, so its e_ref hangs on one number: of the seeds 1, 2, 3 ... it uses the first that meets both
    conditions (seed 1 at widths 32 and 200 gives an e_ref of exactly 0 or below the float32 half-ulp)."""
    def ok(r64, r32):
        half_ulp = np.max(np.spacing(np.abs(r64).astype(np.float32)).astype(np.float64) / 2 / (1 + np.abs(r64)))
        return rel_err(r32, r64) > 0 and 8 * rel_err(r32, r64) > half_ulp

    for count in COUNTS:
        assert ok(*flagship(count)[4:]), count
    for width, aux, head in SHAPES:
        assert ok(*case(width, aux, head, 65)[4:]), (width, aux, head)
    assert ok(*case(200, 1, 3, N.RECORD_BYTES, kind="onehot")[4:])
    assert not ok(*case(**dict(ZERO_CASE, seed=1))[4:])
    assert ok(*case(**ZERO_CASE)[4:])


def test_null_arguments_are_invalid_without_a_device(product_lib):
    n = C.c_void_p()
    d = _lib.CtNetworkDesc(_lib.CT_ABI_VERSION, 10, 16, 0, 1, None, 0)
    assert product_lib.ct_network_create(None, C.byref(d), C.byref(n)) == _lib.CT_E_INVAL
    assert product_lib.ct_network_eval(None, None, None, None, 0, None) == _lib.CT_E_INVAL
    assert product_lib.ct_network_destroy(None) == _lib.CT_OK
    assert product_lib.ct_debug_network_time(None, None) == _lib.CT_E_INVAL
    for name in ("ct_network_create", "ct_network_destroy", "ct_network_eval", "ct_debug_network_time"):
        assert name in _lib.EXPORTS


# ---------------------------------------------------------------------------------------------------- GPU
COUNTS = [1, 31, 32, 33, 65, 1000]
SHAPES = [(32, 0, 1), (16, 8, 4), (256, 1, 2)]


@pytest.fixture(scope="module")
def tracer():
    with ds.CloudTracer(ds.make_procedural_cloud(64), width=24, height=16) as tr:
        yield tr


_NETS = {}


@pytest.fixture(scope="module")
def nets(tracer):
    """Network of a case's weights on the module's tracer, created once."""
    def get(shape, w):
        key = (shape, w.tobytes()[:64], w.size)
        if key not in _NETS:
            _NETS[key] = N.Network(tracer, w, shape.width, shape.aux, shape.head_layers)
        return _NETS[key]
    yield get
    for n in _NETS.values():
        n.close()
    _NETS.clear()


def run(net, b, a, count=None):
    """eval on device copies of the arrays, out allocated with 64 extra floats preset to a sentinel that must survive."""
    import torch
    count = len(b) if count is None else count
    dev = torch.device("cuda", 0)
    desc = torch.from_numpy(np.ascontiguousarray(b)).to(dev)
    aux = torch.from_numpy(np.ascontiguousarray(a)).to(dev) if net.shape.aux else None
    out = torch.full((count + 64,), SENTINEL, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    net.eval(desc.data_ptr(), aux.data_ptr() if aux is not None else None, count, out.data_ptr())
    res = out.cpu().numpy()
    assert np.all(res[count:] == np.float32(SENTINEL)), "wrote past out_dev[count)"
    return res[:count]


def check(dev, r64, r32, what):
    e_ref, e_dev = rel_err(r32, r64), rel_err(dev, r64)
    print(f"{what}: e_ref = {e_ref:.3e}, device = {e_dev:.3e} ({e_dev / e_ref:.2f} x)")
    assert e_ref > 0
    assert np.isfinite(dev).all() and e_dev <= 8 * e_ref, (what, e_dev, e_ref)


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
def test_flagship_shape_at_the_tile_edges(nets, count):
    shape, w, b, a, r64, r32 = flagship(count)
    dev = run(nets(shape, w), b, a)
    check(dev, r64, r32, f"(200,1,3) x {count}")
    if count in (1, 33, 1000):
        assert np.array_equal(dev, run(nets(shape, w), b, a))       # the same call, the same bits


@pytest.mark.gpu
@pytest.mark.parametrize("width,aux,head", SHAPES)
def test_other_shapes(nets, width, aux, head):
    shape, w, b, a, r64, r32 = case(width, aux, head, 65)
    check(run(nets(shape, w), b, a), r64, r32, f"({width},{aux},{head}) x 65")


@pytest.mark.gpu
def test_one_hot_sweep_reaches_every_descriptor_column(nets):
    shape, w, b, a, r64, r32 = case(200, 1, 3, N.RECORD_BYTES, kind="onehot")
    assert len(np.unique(r64)) == N.RECORD_BYTES         # the reference tells every column from every other
    check(run(nets(shape, w), b, a), r64, r32, "one-hot sweep")


@pytest.mark.gpu
def test_zero_input_gives_every_record_the_same_bits(nets):
    shape, w, b, a, r64, r32 = case(**ZERO_CASE)
    dev = run(nets(shape, w), b, a)
    assert np.all(dev.view(np.uint32) == dev.view(np.uint32)[0])
    check(dev, r64, r32, "zero input")


@pytest.mark.gpu
def test_count_zero_is_ok_and_writes_nothing(nets):
    shape, w, b, a, _, _ = flagship(1)
    assert run(nets(shape, w), b, a, count=0).shape == (0,)


@pytest.mark.gpu
def test_invalid_arguments(tracer, nets):
    L, h = tracer.L, tracer.h
    shape = N.NetworkShape(16, 1, 2)
    w = seeded_weights(shape, 2)

    def create(weights=w, ptr=True, out=True, **kw):
        f = dict(abi_version=_lib.CT_ABI_VERSION, blocks=10, width=16, aux=1, head_layers=2, weight_count=weights.size)
        f.update(kw)
        d = _lib.CtNetworkDesc(f["abi_version"], f["blocks"], f["width"], f["aux"], f["head_layers"],
                               weights.ctypes.data_as(C.c_void_p) if ptr else None, f["weight_count"])
        n = C.c_void_p()
        return L.ct_network_create(h, C.byref(d), C.byref(n) if out else None), n

    assert L.ct_network_create(h, None, C.byref(C.c_void_p())) == _lib.CT_E_INVAL
    bad = [dict(ptr=False), dict(out=False), dict(abi_version=_lib.CT_ABI_VERSION + 1), dict(blocks=9), dict(blocks=11),
           dict(width=8), dict(width=20), dict(width=264), dict(aux=9), dict(head_layers=0), dict(head_layers=5),
           dict(weight_count=w.size - 1), dict(weight_count=w.size + 1), dict(width=24)]
    for kw in bad:
        assert create(**kw)[0] == _lib.CT_E_INVAL, kw
    for poison in (np.nan, np.inf, -np.inf):
        wp = w.copy()
        wp[wp.size // 2] = poison
        assert create(weights=wp)[0] == _lib.CT_E_INVAL, poison
    assert b"finite" in L.ct_last_error(h)
    rc, n = create()
    assert rc == _lib.CT_OK and n.value
    try:
        import torch
        dev = torch.device("cuda", 0)
        desc = torch.zeros((4, N.RECORD_BYTES), dtype=torch.uint8, device=dev)
        aux = torch.zeros((4,), dtype=torch.float32, device=dev)
        out = torch.zeros((4,), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        p = lambda t: C.c_void_p(t.data_ptr())
        assert L.ct_network_eval(h, n, p(desc), p(aux), 4, p(out)) == _lib.CT_OK
        assert L.ct_network_eval(h, None, p(desc), p(aux), 4, p(out)) == _lib.CT_E_INVAL
        assert L.ct_network_eval(None, n, p(desc), p(aux), 4, p(out)) == _lib.CT_E_INVAL
        assert L.ct_network_eval(h, n, None, p(aux), 4, p(out)) == _lib.CT_E_INVAL
        assert L.ct_network_eval(h, n, p(desc), None, 4, p(out)) == _lib.CT_E_INVAL          # A == 1 needs aux
        assert L.ct_network_eval(h, n, p(desc), p(aux), 4, None) == _lib.CT_E_INVAL
        assert L.ct_network_eval(h, n, p(desc), p(aux), (1 << 20) + 1, p(out)) == _lib.CT_E_INVAL
        shape0, w0, _, _, _, _ = case(32, 0, 1, 65)
        assert L.ct_network_eval(h, nets(shape0, w0).n, p(desc), p(aux), 4, p(out)) == _lib.CT_E_INVAL   # A == 0 takes none
        assert L.ct_network_eval(h, n, p(desc), p(aux), 4, p(out)) == _lib.CT_OK            # and the handle goes on working
        ms = C.c_double(-1)
        assert L.ct_debug_network_time(n, C.byref(ms)) == _lib.CT_OK and ms.value > 0
    finally:
        assert L.ct_network_destroy(n) == _lib.CT_OK


def _state(tr):
    return tr.mean(), tr.m2(), tr.subframes, tr.counters()


@pytest.mark.gpu
@pytest.mark.parametrize("ahead", [False, True])
def test_no_side_effects_on_a_progressive_render(ahead):
    shape, w, b, a, r64, r32 = flagship(33)
    tex = ds.make_procedural_cloud(64)
    states = []
    for with_call in (True, False):
        with ds.CloudTracer(tex, width=24, height=16) as tr:
            if ahead:
                tr.set_render_ahead(8)
                tr.render_accumulate_async(1, 2)
            else:
                tr.render_accumulate(1, 2)
            if with_call:
                rendered = tr.rendered_subframes()
                with N.Network(tr, w, shape.width, shape.aux, shape.head_layers) as net:
                    check(run(net, b, a), r64, r32, "mid-render")
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
def test_network_frame(tracer, nets):
    import torch
    w_, h_, sid = tracer.width, tracer.height, 3
    shape, w, _, _, _, _ = flagship(1)
    net = nets(shape, w)
    desc, pos, view, pix = tracer.descriptor_frame(sid)
    count = len(pix)
    assert 0 < count < w_ * h_
    image, n = tracer.network_frame(net, sid)
    assert n == count and image.shape == (h_, w_) and image.dtype == torch.float32
    # eval of the same records, with the aux input network_frame documents
    light = torch.tensor(tracer.light_direction(), device=view.device)
    aux = (view * light).sum(dim=1).contiguous()
    out = torch.empty((count,), dtype=torch.float32, device=view.device)
    torch.cuda.synchronize()
    net.eval(desc.data_ptr(), aux.data_ptr(), count, out.data_ptr())
    flat = image.reshape(-1).cpu().numpy()
    valid = np.zeros(w_ * h_, bool)
    valid[pix.cpu().numpy()] = True
    got = out.cpu().numpy()
    assert np.all(got != 0)                       # (so that "0 at exactly the invalid pixels" can be read off the image)
    assert np.array_equal(flat != 0, valid)
    assert np.array_equal(flat[pix.cpu().numpy()], got)
    # ... which are the reference's values for these records
    r64 = N.reference_forward(w, shape, desc.cpu().numpy().reshape(count, -1), aux.cpu().numpy().reshape(count, 1))
    r32 = N.reference_forward(w, shape, desc.cpu().numpy().reshape(count, -1), aux.cpu().numpy().reshape(count, 1), accumulate=np.float32)
    check(got, r64, r32, "network_frame records")
    rect = (5, 3, 19, 12)
    sub, n_sub = tracer.network_frame(net, sid, rect=rect)
    assert sub.shape == (9, 14) and n_sub == int(valid.reshape(h_, w_)[3:12, 5:19].sum())
    assert torch.equal(sub, image[3:12, 5:19])
    # another number of aux inputs is refused
    shape0, w0, _, _, _, _ = case(32, 0, 1, 65)
    with pytest.raises(ValueError):
        tracer.network_frame(nets(shape0, w0), sid)
