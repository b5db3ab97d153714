// ct_network.hip -- ct_network_*: the scattering network evaluated on descriptor records, one fused MFMA kernel (gfx950).
//
// The network is defined in include/cloudtrace.h ("the scattering network"); this file packs its weights on the host and runs it.
//
// Tiling.  Records sit on the MFMA's column index: every layer is Y[out][record] = W[out][in] * X[in][record] with
// v_mfma_f32_32x32x16_bf16, W the A operand and the activations the B operand.  A wave owns 32 records and carries them through
// all 10 blocks and the head; a block is 4 waves = 128 records.  With the width padded to NT tiles of 32 rows a wave holds
//     acc[NT]   the layer's float32 accumulators, 16 registers each (column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5))
//     z[2 NT]   the state as bf16 B fragments, one per k-step of 16 (4 registers each)
//     h[2 NT]   the block's hidden layer, likewise
// An accumulator tile IS the next layer's B operand: registers 8 s .. 8 s + 7 of tile t, rounded to bf16 in pairs, are the
// fragment of k-step 2 t + s, whose element j on lane half g is input feature 32 t + 16 s + 8 (j >> 2) + 4 g + (j & 3).  That
// permutation of k is folded into the weights when they are packed, so activations never move between lanes or through LDS,
// and the residual z + W2 h adds fragment element j to accumulator register 8 s + j of the same lane.
// The descriptor bytes of a layer are 14 k-steps in natural order (lane half g of k-step s holds bytes 16 s + 8 g .. + 7 of its
// record, read from global memory as aligned words and converted in registers) and a 15th that holds byte 224 on lane half 0 and
// the aux inputs on lane half 1.
//
// Weights.  The host packs every matrix into the A fragments the kernel will ask for, in the order it asks: a k-step is NT
// chunks of 1 KiB (64 lanes x 8 bf16, tile after tile), and the whole network is one stream of k-steps
//     block 0: W1 bytes+aux (15), W2 (2 NT);  blocks 1..9: W1 state (2 NT), W1 bytes+aux (15), W2 (2 NT);
//     head: H - 1 times V (2 NT), then v (2 NT, of which only tile 0 is used),
// padded with zeros to whole groups of kGroupSteps k-steps.  A block streams it through a ring of three groups in LDS: on
// entering group g all waves meet at one barrier, each thread then requests its 16-byte pieces of group g + 2 from L2 into
// registers, the wave multiplies through group g reading its A fragments lane-linearly (ds_read_b128), and on leaving the group
// the pieces are written to the slot that group g - 1 has left.  The data of a group is therefore in LDS one full group before
// it is needed, and there is one barrier per 4 NT MFMAs of a wave.  At width 200 (NT = 7) the stream is 3.2 MB and stays in the
// L2 of the XCD.
//
// No atomics, no inline assembly; the only global store is out[record].
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "ct_devmem.hpp"
#include "ct_network.hpp"

namespace {

constexpr uint32_t kBlocks = CT_DESCRIPTOR_LAYERS;
constexpr uint32_t kLayerBytes = CT_DESCRIPTOR_LAYER_SIZE;   // 225
constexpr uint32_t kRecordBytes = CT_DESCRIPTOR_BYTES;       // 2250
constexpr uint32_t kByteSteps = 15;      // k-steps of a layer's bytes and the aux inputs: 14 of bytes, 1 of byte 224 | aux
constexpr uint32_t kGroupSteps = 4;      // k-steps per staged group
constexpr uint32_t kRing = 3;            // groups in LDS
constexpr uint32_t kWaves = 4;           // waves per block
constexpr uint32_t kTileRecords = 32;    // records per wave
constexpr uint32_t kChunk = 512;         // bf16 of one A fragment set (64 lanes x 8)
constexpr uint32_t kMaxCount = 1u << 20;

// ---------------------------------------------------------------------------------------------- rounding and packing (host)
// float32 -> bf16, round to nearest even; a NaN stays a (quiet) NaN.  The one rounding routine: ct_debug_bf16_round exports it.
uint16_t bf16_bits(float x)
{
    uint32_t u;
    memcpy(&u, &x, sizeof u);
    if ((u & 0x7fffffffu) > 0x7f800000u) {
        return (uint16_t)((u >> 16) | 0x40u);
    }
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

struct Geometry {
    uint32_t width, aux, head, nt;
    uint32_t in0() const { return kLayerBytes + aux; }            // fan-in of W1_0
    uint32_t in1() const { return width + kLayerBytes + aux; }    // fan-in of W1_k, k >= 1
    size_t weight_count() const
    {
        const size_t w = width, sq = w * w + w;
        return (w * in0() + w + sq) + (size_t)(kBlocks - 1) * (w * in1() + w + sq) + (size_t)(head - 1) * sq + w + 1;
    }
    uint32_t steps() const
    {
        return (kByteSteps + 2 * nt) + (kBlocks - 1) * (4 * nt + kByteSteps) + (head - 1) * 2 * nt + 2 * nt;
    }
    uint32_t groups() const { return (steps() + kGroupSteps - 1) / kGroupSteps; }
    uint32_t bias_layers() const { return 2 * kBlocks + head; }
};

struct Packer {
    const Geometry &g;
    std::vector<uint16_t> stream;
    std::vector<float> bias;

    // One k-step of the matrix W[rows][ld]: element j of lane half `half` is column col(half, j) of W (a negative column is a
    // zero), divided by 255 where by255(half, j) says so.
    template <class Col, class By255>
    void step(const float *W, uint32_t rows, uint32_t ld, Col col, By255 by255)
    {
        const size_t base = stream.size();
        stream.resize(base + (size_t)g.nt * kChunk, 0);
        for (uint32_t t = 0; t < g.nt; t++) {
            for (uint32_t lane = 0; lane < 64; lane++) {
                const uint32_t row = 32 * t + (lane & 31), half = lane >> 5;
                if (row >= rows) {
                    continue;
                }
                for (uint32_t j = 0; j < 8; j++) {
                    const int c = col(half, j);
                    if (c >= 0) {
                        const float w = W[(size_t)row * ld + (uint32_t)c];
                        stream[base + ((size_t)t * 64 + lane) * 8 + j] = bf16_bits(by255(half, j) ? w / 255.0f : w);
                    }
                }
            }
        }
    }

    // The 2 NT k-steps over `width` features that arrive as packed accumulator tiles, columns first .. first + width of W.
    void state_steps(const float *W, uint32_t rows, uint32_t ld, uint32_t first)
    {
        for (uint32_t s = 0; s < 2 * g.nt; s++) {
            step(W, rows, ld,
                 [&](uint32_t half, uint32_t j) {
                     const uint32_t f = 16 * s + 8 * (j >> 2) + 4 * half + (j & 3);
                     return f < g.width ? (int)(first + f) : -1;
                 },
                 [](uint32_t, uint32_t) { return false; });
        }
    }

    // The 15 k-steps of a layer's bytes (columns first .. first + 225 of W) and the aux inputs (the columns after them).
    void byte_steps(const float *W, uint32_t rows, uint32_t ld, uint32_t first)
    {
        for (uint32_t s = 0; s + 1 < kByteSteps; s++) {
            step(W, rows, ld, [&](uint32_t half, uint32_t j) { return (int)(first + 16 * s + 8 * half + j); },
                 [](uint32_t, uint32_t) { return true; });
        }
        step(W, rows, ld,
             [&](uint32_t half, uint32_t j) {
                 if (half == 0) {
                     return j == 0 ? (int)(first + kLayerBytes - 1) : -1;
                 }
                 return j < g.aux ? (int)(first + kLayerBytes + j) : -1;
             },
             [](uint32_t half, uint32_t) { return half == 0; });
    }

    void bias_layer(const float *b, uint32_t rows)
    {
        const size_t base = bias.size();
        bias.resize(base + (size_t)g.nt * 32, 0.0f);
        memcpy(bias.data() + base, b, rows * sizeof(float));
    }

    void pack(const float *w)
    {
        const uint32_t wd = g.width;
        for (uint32_t k = 0; k < kBlocks; k++) {
            const uint32_t in = k ? g.in1() : g.in0();
            const float *W1 = w, *c1 = W1 + (size_t)wd * in, *W2 = c1 + wd, *c2 = W2 + (size_t)wd * wd;
            w = c2 + wd;
            if (k) {
                state_steps(W1, wd, in, 0);
            }
            byte_steps(W1, wd, in, k ? wd : 0);
            bias_layer(c1, wd);
            state_steps(W2, wd, wd, 0);
            bias_layer(c2, wd);
        }
        for (uint32_t i = 0; i + 1 < g.head; i++) {
            state_steps(w, wd, wd, 0);
            bias_layer(w + (size_t)wd * wd, wd);
            w += (size_t)wd * wd + wd;
        }
        state_steps(w, 1, wd, 0);
        bias_layer(w + wd, 1);
        stream.resize((size_t)g.groups() * kGroupSteps * g.nt * kChunk, 0);
    }
};

// ------------------------------------------------------------------------------------------------------------ the kernel
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // (a native vector: an array of them stays in registers)

struct NetArgs {
    const u32x4 *stream;
    const float *bias;
    const uint8_t *desc;
    const float *aux;
    float *out;
    uint32_t count, aux_n, head, groups;
};

// The weight stream of a block: see "Weights" above.
template <int NT>
struct Pipe {
    static constexpr uint32_t kGroupU4 = kGroupSteps * NT * 64;   // 16-byte pieces per group = NT per thread
    const u32x4 *src;
    u32x4 *ring;
    uint32_t groups;
    uint32_t q;          // k-steps consumed

    __device__ __forceinline__ void load(u32x4 (&stage)[NT], uint32_t g) const
    {
        const u32x4 *p = src + (size_t)g * kGroupU4 + threadIdx.x;
#pragma unroll
        for (int i = 0; i < NT; i++) {
            stage[i] = p[i * 256];
        }
    }
    __device__ __forceinline__ void store(const u32x4 (&stage)[NT], uint32_t g) const
    {
        u32x4 *p = ring + (g % kRing) * kGroupU4 + threadIdx.x;
#pragma unroll
        for (int i = 0; i < NT; i++) {
            p[i * 256] = stage[i];
        }
    }
    __device__ __forceinline__ void prologue(u32x4 (&stage)[NT])
    {
        q = 0;
        load(stage, 0);
        store(stage, 0);
        load(stage, 1);   // (a network has more than two groups)
        store(stage, 1);
    }
    // -> this lane's A fragment of tile 0 of the next k-step; tile t is 64 pieces further on
    __device__ __forceinline__ const u32x4 *begin_step(u32x4 (&stage)[NT])
    {
        const uint32_t g = q / kGroupSteps, s = q % kGroupSteps;
        if (s == 0) {
            __syncthreads();   // group g is in LDS (written while g - 2 or g - 1 ran), and nobody reads group g - 1 any more
            if (g + 2 < groups) {
                load(stage, g + 2);
            }
        }
        return ring + (g % kRing) * kGroupU4 + s * (NT * 64) + (threadIdx.x & 63u);
    }
    __device__ __forceinline__ void end_step(const u32x4 (&stage)[NT])
    {
        const uint32_t g = q / kGroupSteps;
        if (q % kGroupSteps == kGroupSteps - 1 && g + 2 < groups) {
            store(stage, g + 2);      // into the slot of group g - 1
        }
        q++;
    }
};

__device__ __forceinline__ bf16x8 as_fragment(u32x4 v)
{
    return __builtin_bit_cast(bf16x8, v);
}

template <int NT>
__device__ __forceinline__ void mma_step(Pipe<NT> &pipe, u32x4 (&stage)[NT], f32x16 (&acc)[NT], bf16x8 b)
{
    const u32x4 *a = pipe.begin_step(stage);
#pragma unroll
    for (int t = 0; t < NT; t++) {
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_fragment(a[t * 64]), b, acc[t], 0, 0, 0);
    }
    pipe.end_step(stage);
}

// acc = the layer's bias: register 4 i + e of tile t is row 32 t + 8 i + 4 half + e
template <int NT>
__device__ __forceinline__ void load_bias(f32x16 (&acc)[NT], const float *bias, uint32_t half)
{
#pragma unroll
    for (int t = 0; t < NT; t++) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float4 v = *reinterpret_cast<const float4 *>(bias + 32 * t + 8 * i + 4 * half);
            acc[t][4 * i + 0] = v.x;
            acc[t][4 * i + 1] = v.y;
            acc[t][4 * i + 2] = v.z;
            acc[t][4 * i + 3] = v.w;
        }
    }
}

// f = bf16(relu(acc)): the accumulator tiles as the next layer's B fragments
template <int NT>
__device__ __forceinline__ void pack_relu(const f32x16 (&acc)[NT], bf16x8 (&f)[2 * NT])
{
#pragma unroll
    for (int t = 0; t < NT; t++) {
#pragma unroll
        for (int s = 0; s < 2; s++) {
#pragma unroll
            for (int j = 0; j < 8; j++) {
                f[2 * t + s][j] = (__bf16)fmaxf(acc[t][8 * s + j], 0.0f);
            }
        }
    }
}

// The aligned word at byte `off` of the records, of which nothing at or past `total` is read (the missing bytes are 0).
__device__ __forceinline__ uint32_t word_within(const uint8_t *base, uint64_t off, uint64_t total)
{
    if (off + 4 <= total) {
        return *reinterpret_cast<const uint32_t *>(base + off);
    }
    uint32_t v = 0;
    for (uint32_t b = 0; b < 4; b++) {
        if (off + b < total) {
            v |= (uint32_t)base[off + b] << (8 * b);
        }
    }
    return v;
}

// The 8 bytes at `off` (any alignment; off + 8 <= total) from two or three aligned words.
__device__ __forceinline__ uint2 bytes8(const uint8_t *base, uint64_t off, uint64_t total)
{
    const uint64_t a = off & ~(uint64_t)3;
    const uint32_t m = (uint32_t)off & 3u;
    const uint32_t d0 = word_within(base, a, total), d1 = word_within(base, a + 4, total);
    const uint32_t d2 = m ? word_within(base, a + 8, total) : 0u;
    return make_uint2(__builtin_amdgcn_alignbyte(d1, d0, m), __builtin_amdgcn_alignbyte(d2, d1, m));
}

// 8 bytes -> 8 bf16 (0 .. 255 are exact in bf16)
__device__ __forceinline__ bf16x8 bytes_fragment(uint2 v)
{
    bf16x8 f;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        f[j] = (__bf16)(float)((v.x >> (8 * j)) & 0xffu);
        f[4 + j] = (__bf16)(float)((v.y >> (8 * j)) & 0xffu);
    }
    return f;
}

template <int NT>
__global__ __launch_bounds__(kWaves * 64) void network_kernel(NetArgs a)
{
    __shared__ u32x4 ring[kRing * Pipe<NT>::kGroupU4];
    const uint32_t lane = threadIdx.x & 63u, half = lane >> 5, wave = threadIdx.x >> 6;
    const uint32_t rec = (blockIdx.x * kWaves + wave) * kTileRecords + (lane & 31u);
    const bool valid = rec < a.count;          // a record past the end computes on zeros and stores nothing
    const uint64_t total = (uint64_t)a.count * kRecordBytes;
    const uint64_t rec_off = (uint64_t)rec * kRecordBytes;

    Pipe<NT> pipe;
    pipe.src = a.stream;
    pipe.ring = ring;
    pipe.groups = a.groups;
    u32x4 stage[NT];   // this thread's pieces of the group after next, on their way from L2 to LDS
    pipe.prologue(stage);

    bf16x8 zero;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        zero[j] = (__bf16)0.0f;
    }
    bf16x8 auxf = zero;                         // lane half 1 of the last byte step
    if (valid && half == 1u) {
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) {
            if (j < a.aux_n) {
                auxf[j] = (__bf16)a.aux[(uint64_t)rec * a.aux_n + j];
            }
        }
    }

    f32x16 acc[NT];
    bf16x8 z[2 * NT], h[2 * NT];
#pragma unroll
    for (int s = 0; s < 2 * NT; s++) {
        z[s] = zero;
    }
    const float *bias = a.bias;
    const uint2 none = make_uint2(0u, 0u);

    for (uint32_t k = 0; k < kBlocks; k++) {
        const uint64_t layer = rec_off + (uint64_t)kLayerBytes * k + 8u * half;   // this lane's bytes of k-step 0
        uint2 next0 = valid ? bytes8(a.desc, layer, total) : none;
        uint2 next1 = valid ? bytes8(a.desc, layer + 16, total) : none;
        const uint32_t last = valid && half == 0u ? a.desc[rec_off + (uint64_t)kLayerBytes * k + (kLayerBytes - 1)] : 0u;

        // h = relu(W1 [z | b | a] + c1)
        load_bias(acc, bias, half);
        bias += NT * 32;
        if (k) {
#pragma unroll
            for (int s = 0; s < 2 * NT; s++) {
                mma_step(pipe, stage, acc, z[s]);
            }
        }
        for (uint32_t s = 0; s + 1 < kByteSteps; s++) {
            const uint2 cur = next0;
            next0 = next1;
            next1 = valid && s + 3 < kByteSteps ? bytes8(a.desc, layer + 16 * (s + 2), total) : none;
            mma_step(pipe, stage, acc, bytes_fragment(cur));
        }
        bf16x8 tail = auxf;
        if (half == 0u) {
            tail = zero;
            tail[0] = (__bf16)(float)last;
        }
        mma_step(pipe, stage, acc, tail);
        pack_relu(acc, h);

        // z = relu(z + W2 h + c2)
        load_bias(acc, bias, half);
        bias += NT * 32;
#pragma unroll
        for (int s = 0; s < 2 * NT; s++) {
            mma_step(pipe, stage, acc, h[s]);
        }
#pragma unroll
        for (int t = 0; t < NT; t++) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                acc[t][r] += (float)z[2 * t + (r >> 3)][r & 7];   // (z_0 is all zeros)
            }
        }
        pack_relu(acc, z);
    }

    for (uint32_t i = 0; i + 1 < a.head; i++) {
        load_bias(acc, bias, half);
        bias += NT * 32;
#pragma unroll
        for (int s = 0; s < 2 * NT; s++) {
            mma_step(pipe, stage, acc, z[s]);
        }
        pack_relu(acc, z);
    }

    // out = v z + d: row 0 of tile 0, which is register 0 of lane half 0
    f32x16 o[1];
    load_bias(o, bias, half);
#pragma unroll
    for (int s = 0; s < 2 * NT; s++) {
        const u32x4 *w = pipe.begin_step(stage);
        o[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_fragment(w[0]), z[s], o[0], 0, 0, 0);
        pipe.end_step(stage);
    }
    if (valid && half == 0u) {
        a.out[rec] = o[0][0];
    }
}

template <int NT>
hipError_t launch(const NetArgs &a, uint32_t blocks, hipStream_t stream)
{
    hipLaunchKernelGGL(network_kernel<NT>, dim3(blocks), dim3(kWaves * 64), 0, stream, a);
    return hipGetLastError();
}

int failf(int code, char *err, size_t err_len, const char *fmt, ...) __attribute__((format(printf, 4, 5)));
int failf(int code, char *err, size_t err_len, const char *fmt, ...)
{
    if (err && err_len) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, err_len, fmt, ap);
        va_end(ap);
    }
    return code;
}

} // namespace

struct CtNetwork_ {
    int device = 0;
    Geometry geo{};
    ct::DevBuf<uint16_t> d_stream;
    ct::DevBuf<float> d_bias;
    ct::Event ev[2];
    double last_ms = 0;
};

namespace ct {

int network_validate(const CtNetworkDesc *d, CtNetwork *out, char *err, size_t err_len)
{
    if (!d || !out || !d->weights_host) {
        return failf(CT_E_INVAL, err, err_len, "ct_network_create: need a description, its weights and out");
    }
    if (d->abi_version != CT_ABI_VERSION) {
        return failf(CT_E_INVAL, err, err_len, "ct_network_create: abi_version %u, this library is %u", d->abi_version, CT_ABI_VERSION);
    }
    if (d->blocks != kBlocks || d->width < 16 || d->width > 256 || d->width % 8 != 0 || d->aux > 8 || d->head_layers < 1 ||
        d->head_layers > 4) {
        return failf(CT_E_INVAL, err, err_len,
                     "ct_network_create: need blocks == %u, a width that is a multiple of 8 in [16, 256], aux <= 8 and 1 to 4 head "
                     "layers (got %u, %u, %u, %u)", kBlocks, d->blocks, d->width, d->aux, d->head_layers);
    }
    const Geometry g{ d->width, d->aux, d->head_layers, (d->width + 31) / 32 };
    if (d->weight_count != g.weight_count()) {
        return failf(CT_E_INVAL, err, err_len, "ct_network_create: these shapes have %zu weights, not %zu", g.weight_count(),
                     d->weight_count);
    }
    for (size_t i = 0; i < d->weight_count; i++) {
        if (!std::isfinite(d->weights_host[i])) {
            return failf(CT_E_INVAL, err, err_len, "ct_network_create: weight %zu is not finite", i);
        }
    }
    return CT_OK;
}

int network_create(int device, const CtNetworkDesc *d, CtNetwork *out, char *err, size_t err_len)
{
    const int rc = network_validate(d, out, err, err_len);
    if (rc != CT_OK) {
        return rc;
    }
    *out = nullptr;
    CtNetwork n = new (std::nothrow) CtNetwork_;
    if (!n) {
        return failf(CT_E_NOMEM, err, err_len, "ct_network_create: out of host memory");
    }
    n->device = device;
    n->geo = Geometry{ d->width, d->aux, d->head_layers, (d->width + 31) / 32 };
    Packer p{ n->geo, {}, {} };
    try {
        p.pack(d->weights_host);
    } catch (const std::bad_alloc &) {
        delete n;
        return failf(CT_E_NOMEM, err, err_len, "ct_network_create: out of host memory");
    }
    const size_t sbytes = p.stream.size() * sizeof(uint16_t), bbytes = p.bias.size() * sizeof(float);
    hipError_t e = n->d_stream.alloc(p.stream.size());
    e = e == hipSuccess ? n->d_bias.alloc(p.bias.size()) : e;
    e = e == hipSuccess ? hipMemcpy(n->d_stream, p.stream.data(), sbytes, hipMemcpyHostToDevice) : e;
    e = e == hipSuccess ? hipMemcpy(n->d_bias, p.bias.data(), bbytes, hipMemcpyHostToDevice) : e;
    e = e == hipSuccess ? n->ev[0].create() : e;
    e = e == hipSuccess ? n->ev[1].create() : e;
    if (e != hipSuccess) {
        ct_network_destroy(n);
        return failf(e == hipErrorOutOfMemory ? CT_E_NOMEM : CT_E_HIP, err, err_len, "ct_network_create: %s", hipGetErrorString(e));
    }
    *out = n;
    return CT_OK;
}

int network_device(CtNetwork n)
{
    return n->device;
}

uint32_t network_aux_inputs(CtNetwork n)
{
    return n->geo.aux;
}

int network_eval(CtNetwork n, hipStream_t stream, const uint8_t *descriptors_dev, const float *aux_dev, uint32_t count,
                 float *out_dev, char *err, size_t err_len)
{
    if (count > kMaxCount) {
        return failf(CT_E_INVAL, err, err_len, "ct_network_eval: at most 2^20 records per call, not %u", count);
    }
    if (count == 0) {
        return CT_OK;
    }
    if (!descriptors_dev || !out_dev || (aux_dev == nullptr) != (n->geo.aux == 0)) {
        return failf(CT_E_INVAL, err, err_len, "ct_network_eval: need descriptors, out, and aux exactly when the network has aux inputs");
    }
    if (((uintptr_t)descriptors_dev & 3u) || ((uintptr_t)aux_dev & 3u) || ((uintptr_t)out_dev & 3u)) {
        return failf(CT_E_INVAL, err, err_len, "ct_network_eval: the device arrays must be 4-byte aligned");
    }
    NetArgs a{ reinterpret_cast<const u32x4 *>(n->d_stream.get()), n->d_bias, descriptors_dev, aux_dev, out_dev, count, n->geo.aux,
               n->geo.head, n->geo.groups() };
    const uint32_t blocks = (count + kWaves * kTileRecords - 1) / (kWaves * kTileRecords);
    n->last_ms = 0;
    hipError_t e = hipEventRecord(n->ev[0], stream);
    if (e == hipSuccess) {
        switch (n->geo.nt) {
        case 1: e = launch<1>(a, blocks, stream); break;
        case 2: e = launch<2>(a, blocks, stream); break;
        case 3: e = launch<3>(a, blocks, stream); break;
        case 4: e = launch<4>(a, blocks, stream); break;
        case 5: e = launch<5>(a, blocks, stream); break;
        case 6: e = launch<6>(a, blocks, stream); break;
        case 7: e = launch<7>(a, blocks, stream); break;
        default: e = launch<8>(a, blocks, stream); break;
        }
    }
    e = e == hipSuccess ? hipEventRecord(n->ev[1], stream) : e;
    const hipError_t es = hipStreamSynchronize(stream);   // (also after a failure: the call returns with the stream idle)
    e = e == hipSuccess ? es : e;
    float ms = 0;
    e = e == hipSuccess ? hipEventElapsedTime(&ms, n->ev[0], n->ev[1]) : e;
    if (e != hipSuccess) {
        return failf(CT_E_HIP, err, err_len, "ct_network_eval: %s", hipGetErrorString(e));
    }
    n->last_ms = ms;
    return CT_OK;
}

} // namespace ct

extern "C" int ct_network_destroy(CtNetwork n)
{
    if (!n) {
        return CT_OK;
    }
    int prev = 0;
    const bool switched = hipGetDevice(&prev) == hipSuccess && prev != n->device && hipSetDevice(n->device) == hipSuccess;
    delete n;   // (its buffers and events: on its device)
    if (switched) {
        hipSetDevice(prev);
    }
    return CT_OK;
}

extern "C" int ct_debug_network_time(CtNetwork n, double *ms_out)
{
    if (!n || !ms_out) {
        return CT_E_INVAL;
    }
    *ms_out = n->last_ms;
    return CT_OK;
}

extern "C" float ct_debug_bf16_round(float x)
{
    const uint32_t u = (uint32_t)bf16_bits(x) << 16;
    float r;
    memcpy(&r, &u, sizeof r);
    return r;
}
