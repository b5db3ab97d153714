// ct_api.cpp -- the C ABI of include/cloudtrace.h on top of the gfx950 kernels.
//
// Host-side restatement of what the reference's scene items publish to OptiX before a
// launch (Scene::init Scene.cpp:36-46, Sun::init Sun.cpp:13-18, VDBCloud::init
// VDBCloud.cpp:15-137, Mie.cpp:8206-8297, Camera::init Camera.cpp:22-66), then thin launch
// wrappers.  No exception leaves this file and nothing here falls back to a CPU path: if
// HIP or the device is missing every entry point reports CT_E_NODEVICE / CT_E_HIP.
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <map>
#include <vector>

#include "../../include/cloudtrace.h"
#include "ct_handle.hpp"
#include "ct_plan.hpp"

static_assert(plan::kTile == kTile && plan::kQueues == kQueues && plan::kMaxRegions == CtHandle_::kMaxRegions,
              "ct_plan.hpp plans for the kernels' tile and queue counts and the handle's ring");

static thread_local std::string g_create_error;

int ct::fail(CtHandle h, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) {
        h->error = buf;
    } else {
        g_create_error = buf;
    }
    return code;
}

// CT_TRACE=1: host-side phases of a new pose (rebuild_queue, tune_order, build_jobs) with their durations on stderr.
struct TracePhase {
    const char *name;
    std::chrono::steady_clock::time_point t0;
    bool on;
    TracePhase(CtHandle h, const char *n);
    ~TracePhase()
    {
        if (on) {
            fprintf(stderr, "[cloudtrace] %s %.2f ms\n", name,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
    }
};

inline TracePhase::TracePhase(CtHandle h, const char *n) : name(n), t0(std::chrono::steady_clock::now()), on(h && h->tune.TRACE) {}

static int check_invariants(CtHandle h);

static void v3_normalize_twice(const float in[3], float out[3])
{
    float v[3] = { in[0], in[1], in[2] };
    for (int pass = 0; pass < 2; pass++) { // installers.cpp:74-78 then SceneDescription.h:16
        const float inv = 1.0f / sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        v[0] *= inv;
        v[1] *= inv;
        v[2] *= inv;
    }
    out[0] = v[0];
    out[1] = v[1];
    out[2] = v[2];
}

// Mie.cpp:8206-8243: phase / mean(phase), float32 running sum in index order.
static void mie_phase_texture(const float *raw, uint32_t n, std::vector<float> &out)
{
    out.resize(n);
    float average = 0;
    for (uint32_t i = 0; i < n; i++) {
        average += raw[i];
    }
    average /= (float)n;
    for (uint32_t i = 0; i < n; i++) {
        out[i] = raw[i] / average;
    }
}

// Mie.cpp:8245-8282: running sum of phase / sum(phase).
static void mie_integral_texture(const float *raw, uint32_t n, std::vector<float> &out)
{
    out.resize(n);
    float sum = 0;
    for (uint32_t i = 0; i < n; i++) {
        sum += raw[i];
    }
    float integral = 0;
    for (uint32_t i = 0; i < n; i++) {
        integral += raw[i] / sum;
        out[i] = integral;
    }
}

// guide[b] = #{ i : cdf[i] < b / 4096 }, b = 0..4096 (+1 pad): brackets the texel search of
// sample_cos_theta for every 24-bit random whose top 12 bits are b.
static void build_guide(const std::vector<float> &cdf, std::vector<uint16_t> &guide)
{
    guide.assign(kGuideN + 2, 0);
    uint32_t t = 0;
    for (uint32_t b = 0; b <= (uint32_t)kGuideN; b++) {
        const float edge = (float)b / (float)kGuideN;
        while (t < cdf.size() && cdf[t] < edge) {
            t++;
        }
        guide[b] = (uint16_t)t;
    }
    guide[kGuideN + 1] = guide[kGuideN];
}

// ---- shadow-zero rows (DevScene::mbricks bit 6, DevScene::nee_reach; launch_nee_skip_flags) ---------------------------------
// render_persistent_kernel skips the NEE of a collision whose march-brick row has bit 6 set and whose back-off
// t = fl(lg * inv) is <= nee_reach.  Its scatter position is pos_s = fl(pos - fl(fl(dir * lg) * inv)), |dir_a| <= 1 + 2^-22, so
// per axis |pos - pos_s| <= lg * inv * (1 + 2^-20) <= nee_reach * (1 + 2^-20) plus the rounding of the subtraction, and in texel
// coordinates f = fl(fma(p, s_a, -0.5)) the two positions differ by at most
//     D_a = nee_reach * s_a * (1 + 2^-20) + 2^-22 * (s_a + 1)
// (three roundings of magnitude <= 2^-24 * (1.1 s_a + 0.5): |p| <= 1.1 wherever a collision happens, the box being at most
// [-0.01, 1.01]).  Integers floor(f_c) - floor(f_s) < D_a + 1, so the NEE's base texel is within ceil(D_a) of the collision's
// on every axis: the radius r of the flag.  The back-off lg / density is at most one step up to rounding, but that rounding is
// unbounded relative to a tiny density * step (T's last bits); nee_reach is a little under one step, so that at one texel per
// step -- the benchmark's setting -- r is 1, and the few back-offs beyond it (about 0.4 % of the collisions, and the rare
// long ones) evaluate their NEE.
constexpr int kNeeSkipMaxR = 8;   // beyond this the flags are left clear (the distance transform's cost grows with r)

static float nee_skip_reach(const DevScene &d)
{
    return d.sample_step * (1.0f - 1.0f / 256.0f);
}

// The flags' radius in texels, or 0: no skip.  The skip needs in_scattering_finish of a zero footprint to be +-0 (finite light,
// sun ratio and phase tables) -- rad + (+-0) is rad then, rad never being -0.
static int nee_skip_radius(const DevScene &d, bool mie_finite)
{
    if (!mie_finite || !std::isfinite(d.lr) || !std::isfinite(d.lg) || !std::isfinite(d.lb) || !std::isfinite(d.sun_ratio) ||
        !(d.sample_step > 0.0f) || !std::isfinite(d.sample_step)) {
        return 0;
    }
    const double reach = (double)nee_skip_reach(d);
    int r = 0;
    for (const float s : { d.sx, d.sy, d.sz }) {
        const double D = reach * s * (1.0 + std::ldexp(1.0, -20)) + std::ldexp(1.0, -22) * (s + 1.0);
        if (!(D < kNeeSkipMaxR)) {
            return 0;
        }
        r = std::max(r, (int)std::ceil(D));
    }
    return std::max(r, 1);
}

static void release(CtHandle h)
{
    if (!h) {
        return;
    }
    hipSetDevice(h->device);
    if (h->stream) {
        hipStreamSynchronize(h->stream);
    }
#ifdef CT_EXPERIMENTS
    if (h->vmm.va) {
        // the march bricks live in a reserved virtual range: unmap, release the physical chunks, free the range
        hipMemUnmap(h->vmm.va, h->vmm.size);
        for (auto &hd : h->vmm.handles) {
            hipMemRelease(hd);
        }
        hipMemAddressFree(h->vmm.va, h->vmm.size);
        h->vmm.va = nullptr;
        (void)h->d_mbricks.release();   // (not a hipMalloc pointer: nothing to free)
    }
#endif
    // Every buffer and event is a member that frees itself.  The handle's own stream goes after them: after the delete.
    const hipStream_t own_stream = h->own_stream;
    delete h;
    if (own_stream) {
        hipStreamDestroy(own_stream);
    }
}

#ifdef CT_EXPERIMENTS
// EXPERIMENTS BUILD ONLY (measured and rejected in round 4: a gather over memory mapped in 2-MiB pieces runs at 0.55 of the speed of
// the same gather over one hipMalloc, whatever the layout -- DESIGN.md 4.3 item 7b, profiles/r04f, r04g).
// CT_FLAG_VMM_BRICKS / CT_SPARSE=2 (BASELINE.json configs[4], "sparse brick-compressed density"): the dense march-brick array
// h->d_mbricks is replaced by a reserved VIRTUAL range of the same size and layout in which chunks of the virtual-memory
// granularity (2 MiB) SHARE memory wherever they may.  A chunk with a non-zero texel byte gets a copy of its own.  A chunk
// without one is described by its meta bytes alone, and a clearance may be rounded down without changing a result (the exact
// free-space skip gets shorter, nothing else): the clearances are quantised to {0, 4, 8, 16, 32, 64, 127} texels, and all
// chunks whose quantised bytes are equal are mapped onto ONE piece of memory.  For that to happen chunk boundaries must fall
// on brick-row boundaries, so this layout pads a brick row to a power of two bricks (build_march_layouts).  The estimator's kernel is
// the dense one, unchanged -- same address arithmetic, one more level of sharing in the page tables -- and its results are
// identical (tests/test_gpu_parity.py: test_vmm_backed_march_bricks..., the knob test with CT_SPARSE=2; tests/test_configs.py).
static int vmm_back_mbricks(CtHandle h)
{
    const size_t dense_bytes = h->mbricks_dense_bytes;
    hipMemAllocationProp prop{};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = h->device;
    size_t gran = 0;
    HIPCHK(h, hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended));
    const size_t chunk = std::max<size_t>(gran, (size_t)2 << 20);
    if (chunk % 128 != 0 || (chunk & (chunk - 1)) != 0) {
        return fail(h, CT_E_HIP, "virtual-memory granularity %zu is not a power of two", chunk);
    }
    const size_t n_chunks = (dense_bytes + chunk - 1) / chunk;
    const size_t va_size = n_chunks * chunk;
    DevBuf<uint4> d_class;
    HIPCHK(h, d_class.alloc(n_chunks));
    std::vector<uint4> cls(n_chunks);
    const uint8_t *dense = h->d_mbricks;
    void *va = nullptr;
    std::vector<hipMemGenericAllocationHandle_t> handles;
    auto undo = [&]() {
        if (va) {
            hipMemUnmap(va, va_size);
            for (auto &hd : handles) {
                hipMemRelease(hd);
            }
            hipMemAddressFree(va, va_size);
        }
    };
#define VMMCHK(expr)                                                                                       \
    do {                                                                                                   \
        const hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) {                                                                            \
            undo();                                                                                        \
            return fail(h, CT_E_HIP, "virtual-memory bricks: %s failed: %s", #expr, hipGetErrorString(e_)); \
        }                                                                                                  \
    } while (0)
    VMMCHK(launch_mbrick_chunk_class(dense, (int64_t)dense_bytes, (int64_t)chunk, d_class, h->stream));
    VMMCHK(hipMemcpyAsync(cls.data(), d_class, n_chunks * sizeof(uint4), hipMemcpyDeviceToHost, h->stream));
    VMMCHK(hipStreamSynchronize(h->stream));
    VMMCHK(hipMemAddressReserve(&va, va_size, chunk, nullptr, 0));
    // owner[c] = the chunk whose memory chunk c uses (itself: memory of its own)
    std::vector<size_t> owner(n_chunks);
    std::vector<hipMemGenericAllocationHandle_t> of_chunk(n_chunks);
    std::map<uint64_t, size_t> first_with;
    size_t own = 0, with_data = 0;
    for (size_t c = 0; c < n_chunks; c++) {
        const bool whole = (c + 1) * chunk <= dense_bytes;   // (the last, partial chunk always gets memory of its own)
        owner[c] = c;
        if (whole && cls[c].x == 0u) {
            const uint64_t key = (uint64_t)cls[c].z | (uint64_t)cls[c].w << 32;
            const auto it = first_with.find(key);
            if (it != first_with.end()) {
                owner[c] = it->second;
            } else {
                first_with[key] = c;
            }
        } else {
            with_data += 1;
        }
        void *at = (uint8_t *)va + c * chunk;
        if (owner[c] == c) {
            hipMemGenericAllocationHandle_t hd;
            VMMCHK(hipMemCreate(&hd, chunk, &prop, 0));
            handles.push_back(hd);
            of_chunk[c] = hd;
            own += 1;
        } else {
            of_chunk[c] = of_chunk[owner[c]];
        }
        VMMCHK(hipMemMap(at, chunk, 0, of_chunk[c], 0));
    }
    hipMemAccessDesc acc{};
    acc.location = prop.location;
    acc.flags = hipMemAccessFlagsProtReadWrite;
    VMMCHK(hipMemSetAccess(va, va_size, &acc, 1));
    for (size_t c = 0; c < n_chunks; c++) {
        if (owner[c] != c) {
            continue;
        }
        uint8_t *at = (uint8_t *)va + c * chunk;
        const size_t n = std::min(chunk, dense_bytes - c * chunk);
        VMMCHK(hipMemcpyAsync(at, dense + c * chunk, n, hipMemcpyDeviceToDevice, h->stream));
        if (n < chunk) {
            VMMCHK(hipMemsetAsync(at + n, 0, chunk - n, h->stream));
        } else if (cls[c].x == 0u) {
            VMMCHK(launch_mbrick_chunk_quantize(at, (int64_t)chunk, h->stream));   // others are mapped onto these bytes
        }
    }
    VMMCHK(hipStreamSynchronize(h->stream));
#undef VMMCHK
    HIPCHK(h, h->d_mbricks.reset());
    h->d_mbricks.hold((uint8_t *)va, va_size);   // (release() detaches the range again)
    h->dev.mbricks = h->d_mbricks;
    h->vmm.va = va;
    h->vmm.size = va_size;
    h->vmm.chunk = chunk;
    h->vmm.handles = std::move(handles);
    h->vmm.real_chunks = with_data;
    h->vmm.shared_chunks = own - with_data;
    h->vmm.mapped_chunks = n_chunks - own;
    h->mbricks_bytes = own * chunk;
    if (h->tune.STATS) {
        fprintf(stderr, "[cloudtrace] march bricks, dense addressing with sparse backing: %zu chunks of %zu KiB, %zu with texels, %zu distinct "
                        "empty ones, %zu mapped onto those: %.3f GB behind %.3f GB of addresses\n", n_chunks, chunk >> 10, with_data, own - with_data,
                n_chunks - own, (double)(own * chunk) / 1e9, (double)va_size / 1e9);
    }
    return CT_OK;
}
#endif

// ---- ct_create's layout stages: each builds one layout into the handle or returns a CT_* code (create_impl calls them in order)

#define CT_TRY(expr)            \
    do {                        \
        const int rc_ = (expr); \
        if (rc_ != CT_OK) {     \
            return rc_;         \
        }                       \
    } while (0)

// A brick grid is addressed with 32-bit brick indices whose xy plane has 24 bits (apron, march and twin bricks alike).
static bool brick_indices_fit(int64_t gx, int64_t gy, int64_t gz)
{
    return gx * gy * gz < (1ll << 31) && gx * gy < (1ll << 24);
}

// Volumes far larger than the caches -- at 1024^3 nine fetches in ten miss L2 -- get schedules of their own.
static bool beyond_caches(const CtScene *s)
{
    return (uint64_t)s->dims[0] * s->dims[1] * s->dims[2] >= 768ull * 768ull * 768ull;
}

// Bounding box [lo, hi] of the non-zero texels; an empty volume leaves lo = n, hi = -1.
static void density_bbox(const uint8_t *t, const int32_t n[3], int32_t lo[3], int32_t hi[3])
{
    for (int a = 0; a < 3; a++) {
        lo[a] = n[a];
        hi[a] = -1;
    }
    for (int32_t z = 0; z < n[2]; z++) {
        for (int32_t y = 0; y < n[1]; y++) {
            const uint8_t *row = t + ((size_t)z * n[1] + y) * n[0];
            int32_t x0 = 0, x1 = n[0] - 1;
            while (x0 <= x1 && row[x0] == 0) {
                x0++;
            }
            if (x0 > x1) {
                continue;
            }
            while (row[x1] == 0) {
                x1--;
            }
            lo[0] = std::min(lo[0], x0);
            hi[0] = std::max(hi[0], x1);
            lo[1] = std::min(lo[1], y);
            hi[1] = std::max(hi[1], y);
            lo[2] = std::min(lo[2], z);
            hi[2] = std::max(hi[2], z);
        }
    }
}

// Majorant cells of the DELTA grid (orc_majorant_grid / orc_build_majorants in the oracle, same rule).  A VIRTUAL grid of cubic
// cells of C texels covers [-bias, n + bias); stored -- and copied to LDS by every block -- is only the box of cells that can have a
// non-zero majorant: per axis the cells whose clamped read interval [clamp(lo - 1), clamp(lo + C + 1)] meets the bounding interval
// of the non-zero texels.  C = the smallest value >= 4 whose box fits the kernel's LDS array: the benchmark cloud at 512^3 gets
// 10-texel cells where a grid over the whole volume allowed 16 (round 4).
struct MajorantCells {
    int32_t C = 4, div = 0, origin[3] = { 0, 0, 0 }, stored[3] = { 1, 1, 1 }, virt[3] = { 1, 1, 1 };
};

static MajorantCells majorant_cells(const int32_t n[3], int32_t bbias, const int32_t lo[3], const int32_t hi[3])
{
    MajorantCells m;
    for (;; m.C++) {
        const int32_t C = m.C;
        int64_t cells = 1;
        for (int a = 0; a < 3; a++) {
            const int32_t v = (n[a] + 2 * bbias + C - 1) / C;
            int32_t c0 = v, c1 = -1;
            for (int32_t c = 0; c < v; c++) {
                const int32_t r0 = std::min(std::max(C * c - bbias - 1, 0), n[a] - 1), r1 = std::min(std::max(C * c - bbias + C + 1, 0), n[a] - 1);
                if (r0 <= hi[a] && r1 >= lo[a]) {
                    c0 = std::min(c0, c);
                    c1 = c;
                }
            }
            if (c1 < c0) {   // an empty volume: one stored cell, whose majorant will be 0
                c0 = c1 = 0;
            }
            m.origin[a] = c0;
            m.stored[a] = c1 - c0 + 1;
            m.virt[a] = v;
            cells *= (int64_t)m.stored[a];
        }
        if (cells <= kMajCellsMax) {
            break;
        }
    }
    m.div = (int32_t)(((1u << 20) + (uint32_t)m.C - 1u) / (uint32_t)m.C);
    return m;
}

// x / C as (x * div) >> 20 for every texel index of the grid (dda_begin): checked, not argued
static bool majorant_div_exact(const MajorantCells &m)
{
    for (int32_t x = 0; x < (std::max({ m.virt[0], m.virt[1], m.virt[2] }) + 1) * m.C; x++) {
        if ((int32_t)(((uint32_t)x * (uint32_t)m.div) >> 20) != x / m.C || (uint64_t)x * (uint64_t)m.div >= (1ull << 32)) {
            return false;
        }
    }
    return true;
}

// DevScene::delta_interior (render_delta_kernel drops the texel clamp), first half:
// (a real collision has a non-zero texel in its footprint, i.e. its texel coordinate is within one texel of the non-zero
// texels' bounding box: two texels of margin put it inside the box whatever the rounding; CT_DELTA_INTERIOR=0: always test)
// (and a tentative collision lies in a stored cell -- to a hundredth of a texel: the error of the crossings' sums -- so
// when the stored box, grown by one texel, is inside the brick grid its texel index needs no clamp)
static bool cells_inside_apron(const int32_t lo[3], const int32_t hi[3], const int32_t n[3], const MajorantCells &m, const int32_t bg[3])
{
    for (int a = 0; a < 3; a++) {
        if (lo[a] < 2 || hi[a] > n[a] - 3 || m.C * m.origin[a] < 1 || m.C * (m.origin[a] + m.stored[a]) > 4 * bg[a] - 1) {
            return false;
        }
    }
    return true;
}

// (delta_interior's second half for the twin layout: the stored cells, grown by a texel, inside the TWIN grid)
static bool cells_inside_twin(const DevScene &d)
{
    const int32_t tg[3] = { d.t_gx, d.t_gy, d.t_gz }, o[3] = { d.mc_x0, d.mc_y0, d.mc_z0 }, st[3] = { d.mc_gx, d.mc_gy, d.mc_gz };
    for (int a = 0; a < 3; a++) {
        if (d.mc_cell * o[a] - d.brick_bias - 1 < -d.t_bias || d.mc_cell * (o[a] + st[a]) - d.brick_bias > 3 * tg[a] - 1 - d.t_bias) {
            return false;
        }
    }
    return true;
}

// Which of the volume's six boundary layers are empty (launch_inscatter: a march that leaves through one of those is over):
// bit 2 * axis for the layer at 0, bit 2 * axis + 1 for the last one.
static uint32_t zero_faces(const uint8_t *t, uint32_t nx, uint32_t ny, uint32_t nz)
{
    const uint32_t n[3] = { nx, ny, nz };
    uint32_t faces = 0;
    for (uint32_t f = 0; f < 6; f++) {
        const uint32_t axis = f / 2, u_axis = (axis + 1) % 3, v_axis = (axis + 2) % 3;
        uint32_t c[3];
        c[axis] = (f & 1) ? n[axis] - 1 : 0;
        bool zero = true;
        for (c[v_axis] = 0; zero && c[v_axis] < n[v_axis]; c[v_axis]++) {
            for (c[u_axis] = 0; zero && c[u_axis] < n[u_axis]; c[u_axis]++) {
                zero = t[((size_t)c[2] * ny + c[1]) * nx + c[0]] == 0;
            }
        }
        faces |= (zero ? 1u : 0u) << f;
    }
    return faces;
}

// How the march bricks are stored.  CT_FLAG_SPARSE_BRICKS / CT_FLAG_VMM_BRICKS choose; CT_SPARSE, set to anything, overrides both
// (0 dense, 1 row extents, 2 virtual memory, 3 its padded rows alone, 4 virtual memory without them).
struct MarchStorage {
    bool sparse;         // compacted to the extents of the brick rows (compact_march_bricks; MARCH only)
    bool vmm;            // dense addressing with sparse backing (vmm_back_mbricks; MARCH only, experiments build)
    bool pad_rows;       // brick rows padded to a power of two bricks (for the virtual-memory chunks)
    bool experimental;   // one of the virtual-memory layouts: the product build refuses them
};

static MarchStorage march_storage(const CtScene *s, const Knob &sparse_knob)
{
    bool sparse = (s->flags & CT_FLAG_SPARSE_BRICKS) != 0, vmm = (s->flags & CT_FLAG_VMM_BRICKS) != 0, pad_only = false, no_pad = false;
    if (const char *env = sparse_knob.get()) {
        const int v = atoi(env);
        sparse = v == 1;
        vmm = v == 2 || v == 4;
        pad_only = v == 3;   // (A/B: the padded rows of the virtual-memory layout in ordinary memory)
        no_pad = v == 4;     // (A/B: the mapping without the padded rows)
    }
    const bool march = s->estimator == CT_EST_MARCH;
    vmm = vmm && march;
    return { sparse && march, vmm && !sparse, (vmm && !no_pad) || pad_only, vmm || pad_only };
}

static int open_device(const CtScene *s, CtHandle h)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        return fail(h, CT_E_NODEVICE, "no HIP device visible (libcloudtrace has no CPU fallback)");
    }
    if (s->device < 0 || s->device >= ndev) {
        return fail(h, CT_E_INVAL, "device %d out of range (0..%d)", s->device, ndev - 1);
    }
    HIPCHK(h, hipSetDevice(s->device));
    (void)hipGetLastError(); // (see NEED_NOFLUSH)
    HIPCHK(h, hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    for (auto &e : h->ev) {
        HIPCHK(h, e.create());
    }
    return CT_OK;
}

// The schedule (launch shapes, scheduler constants, job queues, pipeline): defaults by estimator and volume size, then the knobs.
static int choose_schedule(const CtScene *s, CtHandle h)
{
    const CtTuning &t = h->tune;
    DevScene &d = h->dev;
    const bool delta = s->estimator == CT_EST_DELTA, big = beyond_caches(s);
    // (persistent_shape takes CT_BLOCKS_PER_CU from 1 to 8 and ignores other values)
    h->shape = persistent_shape(s->device, delta, knob_int(t.BLOCKS_PER_CU, INT_MIN, INT_MAX, 0));
    h->debug_invariants = knob_flag(t.DEBUG_INVARIANTS, h->debug_invariants);
    h->shape.stats = t.STATS.get() != nullptr || h->debug_invariants;
    h->exchange = delta ? knob_int(t.EXCHANGE, 0, 2, 0) : 0;
#ifdef CT_EXPERIMENTS
    if (h->exchange && (s->flags & CT_FLAG_TEX_FIXED8)) {
        // (the path-exchange kernels are measured-and-rejected experiments: they filter with the exact weights only)
        return fail(h, CT_E_INVAL, "CT_EXCHANGE has no CT_FLAG_TEX_FIXED8 kernels");
    }
    if (h->exchange) {
        h->xshape = h->exchange == 2 ? wave_exchange_shape(s->device) : exchange_shape(s->device);
        h->xshape.stats = h->shape.stats;
    }
#else
    if (h->exchange) {
        // the product's library holds the product's kernels only; the measured-and-rejected ones live in the experiments build
        return fail(h, CT_E_INVAL, "CT_EXCHANGE needs the experiments build (python -m deepestscatter_amd.build --variant exp; "
                                   "CT_LIBRARY=libcloudtrace_exp.so)");
    }
#endif
    // measured (profiles/README.md, burst sweep): 1207 Msamples/s without bursts, 1453 with 8/32/32
    // (re-swept on the final kernel, 512 spp per launch: burst_scatter 48 -> 40 is worth +3 %, 2871 -> 2963)
    // DELTA: a tracking visit ends in a real collision 6 times out of 10: short bursts and an early refill
    // (sweep at 512^3/1024^2: 8/16 -> 2300 Msamples/s, 1/16 -> 2700, 1/4 -> 2870, 3/4 -> 3460)
    // (round 2, on the final kernel: 3/4 with scatter phases as soon as one lane waits 4200; the scatter phase held back
    // until 16 lanes wait 4241; that with bursts of 2: 4295 -- profiles/r02e/delta_scatter_min_sweep.log)
    // Beyond the caches every fetch is an L2 miss and longer bursts pay: 1914 vs 1855 Msamples/s at 1024^3.
    d.march_burst = (uint32_t)knob_int(t.MARCH_BURST, 1, 1024, delta ? 2 : 8);
    // (round 6, with the bounded free-space replay, CT_MARCH_REPLAY_MAX = 4: burst_scatter 24 / 28 / 32 / 36 / 40 / 48 ->
    // 3825 / 3880 / 3895 / 3862 / 3766 / 3481 Msamples/s; the parent's loop: 3725 / 3790 / 3827 / 3823 / 3763 / 3532; profiles/r06a)
    // (round 10, on the list without through pixels, 512^3 / 1024^2, Msamples/s, the other knobs at their defaults; profiles/r10a:
    //    march_burst      1 / 2 / 4 / 6 / 8 / 12 / 16 / 32 / 64   2996 / 3867 / 4097 / 4086 / 4081 / 4069 / 4065 / 4052 / 4045
    //    burst_scatter    8 / 16 / 24 / 28 / 32 / 36 / 40 / 48 / 65   3079 / 3674 / 4009 / 4066 / 4081 / 4032 / 3933 / 3613 / 3419
    //    burst_idle       4 / 8 / 16 / 32 / 48 / 65   3411 / 4081 / 4084 / 4081 / 4083 / 4084
    //    burst_march_min  1 / 4 / 8 / 16 / 32   4081 / 4082 / 4082 / 4081 / 4075
    //    tail_burst       2 / 8 / 32   4081 / 4081 / 4080
    //  march_burst 4 is +0.3-0.4 % with and without the refill at 4 lanes -- twice the run-to-run spread, not ten times: 8 stays;
    //  83 % of the bursts end at burst_scatter after 3.4 steps, 3 % at their step count, none for idle lanes -- the MARCH kernel
    //  no longer has that rule, burst_idle is the DELTA kernel's)
    d.burst_scatter = (uint32_t)knob_int(t.BURST_SCATTER, 1, 65, delta || big ? 48 : 32);
    d.burst_idle = (uint32_t)knob_int(t.BURST_IDLE, 1, 65, 32);   // (render_delta_kernel only)
    d.burst_march_min = (uint32_t)knob_int(t.BURST_MARCH_MIN, 1, 64, 1);
    d.tail_burst = (uint32_t)knob_int(t.TAIL_BURST, 1, 1024, 8);
    // (re-swept on the final kernel: 8 instead of 16 is worth +1.4 % at 512^3 and +5 % at 256^3; 16 stays best at 1024^3)
    // (round 10: every sample a wave takes is now a path of some 56 bounces, a lane idles only when such a path ends, and a
    // regeneration hands out 8 of them after an average of 11 idle lanes per scheduler visit.  Refilling at 4:
    //    regen_min  1 / 2 / 3 / 4 / 5 / 6 / 8 / 12 / 16 / 24 / 32
    //    no priority   4030 / 4099 / - / 4130 / - / 4110 / 4081 / 3990 / 3875 / 3594 / 3358
    //    with phase priority   - / - / 4182 / 4182 / 4177 / - / 4135 / ...     (+1.1-1.2 % either way; profiles/r10a)
    //  the >= 768^3 value and the short batches' 16 were not swept again)
    d.regen_min = (uint32_t)knob_int(t.REGEN_MIN, 1, 64, delta ? 4 : big ? 16 : 4);
    // measured: running the scatter phase as soon as any lane needs it beats waiting for a fuller
    // phase (927 vs 877 Msamples/s); a waiting lane is latency added to a serial path
    // (DELTA: 16 until the tracking burst followed the scatter phase in one iteration; 8 / 12 / 16 / 24 / 32: 5284 / 5290 / 5273
    // / 5168 / 5104, profiles/r04h, r04i)
    // (round 10, MARCH: scatter_min 1 / 2 / 4 / 8 / 16 -> 4081 / 4072 / 4074 / 4069 / 4069; entry ratio 0 / 1/8 / 1/4 / 1/2 -> 4081 / 4081 /
    // 4081 / 4080: a scatter phase has 30 lanes as it is, because the bursts end at burst_scatter)
    d.scatter_min = (uint32_t)knob_int(t.SCATTER_MIN, 1, 64, delta ? 12 : 1);
    d.scatter_num = 0;
    d.scatter_den = 1;
    if (const char *e = t.SCATTER_RATIO.get()) { // "num/den"
        unsigned a = 1, b = 1;
        if (sscanf(e, "%u/%u", &a, &b) == 2 && b > 0 && a < 1000 && b < 1000) {
            d.scatter_num = a;
            d.scatter_den = b;
        }
    }
    d.hint_period = 64;
    if (const char *e = t.HINT_PERIOD.get()) {
        const int v = atoi(e);
        d.hint_period = (v > 0 && (v & (v - 1)) == 0) ? (uint32_t)v : 0u;
    }
    if (delta) {
        // measured at 512^3 / 1024^2 (profiles/r04b, r04c): 0 -> 5020 Msamples/s, 1 -> 5125 (+2.1 %: 2.8 % fewer vector
        // instructions, the NEE miss off the bounce's critical path), 2 -> 5100 (+1.6 % although the launch moves 32 % fewer
        // bytes: the kernel is bound by instruction issue, not by line fills -- DESIGN.md 4.2 "Round 4")
        // ... and at 1024^3 / 2048^2, where nine fetches in ten miss L2 and the volume is four times the Infinity Cache, the
        // twin bricks win: 0 -> 3841, 1 -> 3914, 2 -> 4562 Msamples/s (+19 %; profiles/r04d)
        // (CT_DELTA_NEE, render_delta_kernel<.., NEE>: where a collision's two lookups come from)
        d.delta_nee = (uint32_t)knob_int(t.DELTA_NEE, 0, 2, big ? 2 : 1);
        h->job_work = 48.f;     // (its cost unit is a bounce; 16 measured 0.4 % slower there)
    }
    // measured (profiles/README.md): regional queues raise the L2 hit rate from 67 % to 77 % but not
    // the speed (the kernel is bound by the L1 gather rate and by instruction issue, not by L2
    // misses), and any imbalance between regions costs more than that: off unless asked for
    // ... unless the volume is far larger than the caches: at 1024^3 (2.7 GB of march bricks) the regional
    // queues are worth +4.5 % (1824 -> 1906 Msamples/s at 2048^2); at 512^3 they cost 0.5-2 %
    h->queues_enabled = knob_flag(t.XCD_QUEUES, big);
    h->regions = (uint32_t)knob_int(t.XCD_REGIONS, 1, 65536, (int)h->regions);
    if (const char *e = t.SHARED_DEPTH.get()) {
        h->shared_depth = (float)atof(e);
    }
    h->job_max = (uint32_t)knob_int(t.JOB_MAX, 1, 4096, (int)h->job_max);
    if (const char *e = t.JOB_WORK.get()) {
        h->job_work = (float)std::max(1.0, atof(e));
    }
    h->no_advance = knob_flag(t.NO_ADVANCE, h->no_advance);
    h->point_order = knob_flag(t.POINT_ORDER, h->point_order);
    h->continuation = knob_flag(t.CONTINUATION, h->continuation) && !h->exchange;   // (the exchange kernels run every path to its end)
    h->chunk_interleave = knob_flag(t.CHUNK_INTERLEAVE, h->chunk_interleave);
    if (const char *e = t.TILE_ORDER.get()) {
        h->tile_hilbert = strcmp(e, "hilbert") == 0;
    }
    h->chunk_morton = knob_flag(t.CHUNK_MORTON, h->chunk_morton);
    h->serpentine = knob_flag(t.SERPENTINE, h->serpentine);
    h->hand_on_jobs = knob_flag(t.HAND_ON_JOBS, h->hand_on_jobs);
    h->max_age_override = knob_int(t.MAX_AGE, 0, CtHandle_::kMaxRegions - 1, h->max_age_override);
    h->ahead = (uint32_t)knob_int(t.RENDER_AHEAD, 0, 65535, (int)h->ahead);
    return CT_OK;
}

// ---- uniforms: VDBCloud::setupVolumeVariables (VDBCloud.cpp:98-111), Sun::init (Sun.cpp:13-18)
// The light's share of them (ct_create and ct_set_light): nlx/nly/nlz and lr/lg/lb.
static void light_uniforms(const CtScene *s, DevScene &d)
{
    float l[3] = { s->light_direction[0], s->light_direction[1], s->light_direction[2] };
    if (!(s->flags & CT_FLAG_LIGHT_NORMALIZED)) {
        v3_normalize_twice(s->light_direction, l);
    }
    d.nlx = -l[0];
    d.nly = -l[1];
    d.nlz = -l[2];
    d.lr = s->light_color[0] * s->light_intensity;
    d.lg = s->light_color[1] * s->light_intensity;
    d.lb = s->light_color[2] * s->light_intensity;
}

static void scene_uniforms(const CtScene *s, DevScene &d)
{
    const uint32_t nx = s->dims[0], ny = s->dims[1], nz = s->dims[2];
    const float fx = (float)nx, fy = (float)ny, fz = (float)nz;
    const float maxs = fmaxf(fmaxf(fx, fy), fz);
    d.nx = (int32_t)nx;
    d.ny = (int32_t)ny;
    d.nz = (int32_t)nz;
    d.bx = fx / maxs;
    d.by = fy / maxs;
    d.bz = fz / maxs;
    d.hx = d.bx + 0.01f;
    d.hy = d.by + 0.01f;
    d.hz = d.bz + 0.01f;
    d.tsx = maxs / fx;
    d.tsy = maxs / fy;
    d.tsz = maxs / fz;
    d.sx = (maxs / fx) * fx; // textureScale * N
    d.sy = (maxs / fy) * fy;
    d.sz = (maxs / fz) * fz;
    d.density_multiplier = s->cloud_size_m / s->mean_free_path_m;
    d.sample_step = s->sample_step;
    light_uniforms(s, d);
    {
        // cloud.cuh:148-151 evaluated once on the host, in float like the device code.
        const float sunAngularRadiusDeg = 0.53f / 2;
        const float sphereArea = 4 * kPi;
        const float sunArea = 2 * kPi * (1 - cosf(sunAngularRadiusDeg * kPi / 180.0f));
        d.sun_ratio = sunArea / sphereArea;
    }
    d.width = s->width;
    d.height = s->height;
    d.max_depth = s->max_depth;
    d.mode = s->mode;
    d.tex_fixed8 = (s->flags & CT_FLAG_TEX_FIXED8) ? 1u : 0u;   // every launcher picks its kernel by it (the shadow volume's too)
    d.tiles_x = (s->width + kTile - 1) / kTile;
    d.tiles_y = (s->height + kTile - 1) / kTile;
}

// The apron bricks' grid (4^3 texels each).  apron: the farthest texel a marching path can address -- slack box + the steps it
// fetches speculatively in one scheduler visit (kSpec in ct_kernels.hip, 8 allowed for here).
static int apron_grid(const CtScene *s, CtHandle h, int &apron)
{
    DevScene &d = h->dev;
    const uint32_t nx = s->dims[0], ny = s->dims[1], nz = s->dims[2];
    apron = (int)ceilf((0.01f + 8.0f * s->sample_step) * fmaxf(fmaxf(d.sx, d.sy), d.sz) + 0.5f) + 1;
    if (apron > 160) {
        return fail(h, CT_E_INVAL, "sample_step %g too coarse for a %u^3 volume", (double)s->sample_step,
                    (unsigned)std::max({ nx, ny, nz }));
    }
    // brick coordinates = (texel index + bias) / 4, bias a multiple of 4 covering the apron
    const int bbias = ((apron + 3) / 4) * 4;
    const int64_t bgx = ((int64_t)nx + 2 * bbias + 3) / 4 + 1, bgy = ((int64_t)ny + 2 * bbias + 3) / 4 + 1,
                  bgz = ((int64_t)nz + 2 * bbias + 3) / 4 + 1;
    if (!brick_indices_fit(bgx, bgy, bgz)) {
        return fail(h, CT_E_INVAL, "volume too large for 32-bit brick indices");
    }
    d.brick_bias = bbias;
    d.nee_cache = (bgx * bgy * bgz < (1ll << 25) && knob_flag(h->tune.NEE_CACHE, true)) ? 1u : 0u;
    d.brick_gx = (int32_t)bgx;
    d.brick_gxy = (int32_t)(bgx * bgy);
    d.brick_gy = (int32_t)bgy;
    d.brick_gz = (int32_t)bgz;
    return CT_OK;
}

// ---- Mie textures (Mie.cpp:8206-8297) + guide table.  mie_finite: both phase tables are finite (nee_skip_radius).
static int upload_mie(const CtScene *s, CtHandle h, bool &mie_finite)
{
    std::vector<float> mie_tex, chopped_tex, cdf_tex;
    std::vector<uint16_t> guide;
    mie_phase_texture(s->mie_host, s->mie_count, mie_tex);
    mie_phase_texture(s->chopped_mie_host, s->mie_count, chopped_tex);
    mie_integral_texture(s->chopped_mie_host, s->mie_count, cdf_tex);
    build_guide(cdf_tex, guide);
    HIPCHK(h, h->d_mie.alloc(kMieN));
    HIPCHK(h, h->d_chopped.alloc(kMieN));
    HIPCHK(h, h->d_cdf.alloc(kMieN));
    HIPCHK(h, h->d_guide.alloc(kGuideN + 2));
    HIPCHK(h, hipMemcpyAsync(h->d_mie, mie_tex.data(), kMieN * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_chopped, chopped_tex.data(), kMieN * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_cdf, cdf_tex.data(), kMieN * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_guide, guide.data(), (kGuideN + 2) * sizeof(uint16_t), hipMemcpyHostToDevice,
                             h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream)); // the vectors die at scope exit
    mie_finite = true;
    for (int i = 0; i < kMieN; i++) {
        mie_finite = mie_finite && std::isfinite(mie_tex[i]) && std::isfinite(chopped_tex[i]);
    }
    h->dev.mie = h->d_mie;
    h->dev.chopped = h->d_chopped;
    h->dev.cdf = h->d_cdf;
    h->dev.guide = h->d_guide;
    return CT_OK;
}

// ---- density -> corner cells, with the free-space distance field on the brick grid itself embedded as the bricks' meta byte;
// shadow volume (VDBCloud::InitInScatter) -> corner cells: allocated here, built once it is marched (build_march_layouts)
static int build_apron_bricks(const CtScene *s, CtHandle h)
{
    DevScene &d = h->dev;
    const uint32_t nx = s->dims[0], ny = s->dims[1], nz = s->dims[2];
    const size_t texels = h->volume_bytes;
    const int bbias = d.brick_bias;
    const int64_t bgx = d.brick_gx, bgy = d.brick_gy, bgz = d.brick_gz;
    const size_t brick_bytes = (size_t)(bgx * bgy * bgz) * 128;
    HIPCHK(h, h->d_density.alloc(texels));
    HIPCHK(h, h->d_inscatter.alloc(texels));
    HIPCHK(h, h->d_dbricks.alloc(brick_bytes));
    HIPCHK(h, h->d_ibricks.alloc(brick_bytes));
    HIPCHK(h, hipMemcpyAsync(h->d_density, s->density_host, texels, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, launch_build_bricks(h->d_density, nx, ny, nz, bbias, (int)bgx, (int)bgy, (int)bgz, h->d_dbricks, h->stream));
    d.dbricks = h->d_dbricks;
    d.ibricks = h->d_ibricks;
    const size_t nb = (size_t)(bgx * bgy * bgz);
    HIPCHK(h, h->d_dist.alloc(nb));
    HIPCHK(h, h->d_dist_tmp.alloc(nb));
    HIPCHK(h, h->d_majorant.alloc(nb));
    HIPCHK(h, launch_build_dist(h->d_density, nx, ny, nz, bbias, (int)bgx, (int)bgy, (int)bgz, h->d_dist,
                                h->d_dist_tmp, h->d_majorant, h->stream));
    HIPCHK(h, launch_brick_meta(h->d_dist, h->d_majorant, nx, ny, nz, bbias, (int)bgx, (int)bgy, (int)bgz,
                                h->d_dbricks, h->stream));
    return CT_OK;
}

// The DELTA estimator's majorant grid (majorant_cells) and the first half of delta_interior.
static int build_majorant_grid(const CtScene *s, CtHandle h)
{
    DevScene &d = h->dev;
    const uint32_t nx = s->dims[0], ny = s->dims[1], nz = s->dims[2];
    const int32_t n[3] = { (int32_t)nx, (int32_t)ny, (int32_t)nz };
    const int bbias = d.brick_bias;
    int32_t lo[3], hi[3];
    density_bbox(s->density_host, n, lo, hi);
    const MajorantCells m = majorant_cells(n, bbias, lo, hi);
    if (!majorant_div_exact(m)) {
        return fail(h, CT_E_INVAL, "volume too large for the majorant grid's index arithmetic");
    }
    const auto &[C, div, origin, stored, virt] = m;
    const size_t cells = (size_t)stored[0] * stored[1] * stored[2];
    HIPCHK(h, h->d_maj_cells.alloc((cells + 3) & ~(size_t)3)); // the kernel copies whole words
    HIPCHK(h, hipMemsetAsync(h->d_maj_cells, 0, (cells + 3) & ~(size_t)3, h->stream));
    HIPCHK(h, h->d_maj_codes.alloc((cells + 3) & ~(size_t)3));
    HIPCHK(h, hipMemsetAsync(h->d_maj_codes, 0, (cells + 3) & ~(size_t)3, h->stream));
    HIPCHK(h, launch_majorant_cells(h->d_density, nx, ny, nz, bbias, C, origin, stored[0], stored[1], stored[2], h->d_maj_cells,
                                    h->d_maj_codes, h->stream));
    d.maj_cells = h->d_maj_cells;
    d.maj_codes = h->d_maj_codes;
    d.mc_cell = C;
    d.mc_div = div;
    d.mc_gx = stored[0];
    d.mc_gy = stored[1];
    d.mc_gz = stored[2];
    d.mc_x0 = origin[0];
    d.mc_y0 = origin[1];
    d.mc_z0 = origin[2];
    d.mc_vx = virt[0];
    d.mc_vy = virt[1];
    d.mc_vz = virt[2];
    const int32_t bg[3] = { d.brick_gx, d.brick_gy, d.brick_gz };
    d.delta_interior = (cells_inside_apron(lo, hi, n, m, bg) && knob_flag(h->tune.DELTA_INTERIOR, true)) ? 1u : 0u;
    return CT_OK;
}

// Twin bricks (DevScene::tbricks): density and shadow volume of 3^3 base texels in one line, over the texel range of the apron
// bricks (which is that of the majorant cells: every position a flight can reach).  The grid; build_march_layouts fills it.
static int twin_grid(CtHandle h)
{
    DevScene &d = h->dev;
    const int bbias = d.brick_bias, tbias = ((bbias + 2) / 3) * 3;
    const int64_t tgx = ((int64_t)d.nx + bbias + tbias + 2) / 3 + 1, tgy = ((int64_t)d.ny + bbias + tbias + 2) / 3 + 1,
                  tgz = ((int64_t)d.nz + bbias + tbias + 2) / 3 + 1;
    if (!brick_indices_fit(tgx, tgy, tgz) || (int64_t)std::max({ d.nx, d.ny, d.nz }) + 2 * tbias >= (1 << 15)) {
        return fail(h, CT_E_INVAL, "volume too large for 32-bit brick indices");
    }
    if (h->d_tbricks.alloc((size_t)(tgx * tgy * tgz) * 128) != hipSuccess) {
        return fail(h, CT_E_NOMEM, "out of device memory (twin bricks)");
    }
    d.tbricks = h->d_tbricks;
    d.t_bias = tbias;
    d.t_gx = (int32_t)tgx;
    d.t_gy = (int32_t)tgy;
    d.t_gz = (int32_t)tgz;
    if (!cells_inside_twin(d)) {
        d.delta_interior = 0u;
    }
    return CT_OK;
}

// Sparse storage (BASELINE.json configs[4]: "1024^3 sparse brick-compressed density"): CT_FLAG_SPARSE_BRICKS, or
// CT_SPARSE=0/1 in the environment.  Not the default at any size: measured at 1024^3 / 2048^2 the stored bricks
// shrink from 3.41 GB to 0.36 GB, but the march runs 20 % slower (1670 vs 2083 Msamples/s,
// profiles/r02c/ab_sparse_1024.log) -- the row-extent lookup is one more dependent load in a gather that is bound
// by latency and by the L1's address rate, and only 5 % of the fetches land outside the stored extents, so there
// are few line fills to save.  With 288 GB of HBM the dense array is the faster choice; this is the option for
// when capacity matters.
// Each brick row keeps its bricks from the first to the last one with a texel; the cells outside those extents get a coarse
// clearance from the distance volume tmp_b.
static int compact_march_bricks(CtHandle h, const uint8_t *tmp_b)
{
    DevScene &d = h->dev;
    const uint32_t nx = (uint32_t)d.nx, ny = (uint32_t)d.ny, nz = (uint32_t)d.nz;
    const int bbias = d.brick_bias;
    const int64_t bgx = d.brick_gx, bgy = d.brick_gy, bgz = d.brick_gz, mgx = d.m_gx;
    const size_t rows = (size_t)(bgy * bgz);
    DevBuf<uint32_t> d_x0, d_x1;
    DevBuf<uint8_t> compact;
    auto run = [&]() -> int {
        HIPCHK(h, d_x0.alloc(rows));
        HIPCHK(h, d_x1.alloc(rows));
        HIPCHK(h, hipMemsetAsync(d_x0, 0xff, rows * sizeof(uint32_t), h->stream));
        HIPCHK(h, hipMemsetAsync(d_x1, 0, rows * sizeof(uint32_t), h->stream));
        HIPCHK(h, launch_mbrick_extent(h->d_mbricks, (int)mgx, (int)bgy, (int)bgz, d_x0, d_x1, h->stream));
        std::vector<uint32_t> x0(rows), x1(rows);
        HIPCHK(h, hipMemcpyAsync(x0.data(), d_x0, rows * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(x1.data(), d_x1, rows * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        std::vector<uint2> ri(rows);
        uint64_t lines = 0;
        for (size_t r = 0; r < rows; r++) {
            const uint32_t cnt = x1[r] > x0[r] ? x1[r] - x0[r] : 0u;
            ri[r] = make_uint2((uint32_t)lines, cnt ? (x0[r] | (cnt << 16)) : 0u);
            lines += cnt;
        }
        if (lines >= (1ull << 32)) {
            return fail(h, CT_E_INVAL, "volume too large for 32-bit brick indices");
        }
        HIPCHK(h, h->d_mrows.alloc(rows));
        HIPCHK(h, hipMemcpyAsync(h->d_mrows, ri.data(), rows * sizeof(uint2), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, compact.alloc(std::max<size_t>((size_t)lines, 1) * 128));
        HIPCHK(h, launch_mbrick_compact(h->d_mbricks, (int)mgx, (int)bgy, (int)bgz, h->d_mrows, compact, h->stream));
        // clearance of the cells outside the extents: cubic cells of 8 texels over the brick grid's texel range
        const int cshift = 3;
        const int64_t cgx = (4 * bgx + 7) >> cshift, cgy = (4 * bgy + 7) >> cshift, cgz = (4 * bgz + 7) >> cshift;
        HIPCHK(h, h->d_mcoarse.alloc((size_t)(cgx * cgy * cgz)));
        HIPCHK(h, launch_coarse_clearance(tmp_b, nx, ny, nz, bbias, cshift, (int)cgx, (int)cgy, (int)cgz, h->d_mcoarse,
                                          h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream)); // `ri` dies at scope exit; the dense array is freed below
        HIPCHK(h, h->d_mbricks.reset());
        h->d_mbricks = std::move(compact);
        d.mbricks = h->d_mbricks;
        h->mbricks_bytes = (size_t)lines * 128;
        d.m_rows = h->d_mrows;
        d.m_coarse = h->d_mcoarse;
        d.m_cshift = cshift;
        d.m_cgx = (int32_t)cgx;
        d.m_cgxy = (int32_t)(cgx * cgy);
        return CT_OK;
    };
    const int rc = run();
    if (rc != CT_OK) {
        hipStreamSynchronize(h->stream);   // (before the temporaries go)
    }
    return rc;
}

// March bricks (3x4x4 texels, one meta byte per row; DevScene::mbricks) and what is built over them up to the compaction (in the
// order create_impl states).  A launch error skips the launches that follow and is reported after the stream synchronise.
static int build_march_layouts(const CtScene *s, CtHandle h, int apron, const MarchStorage &ms, uint32_t zero_faces, bool mie_finite)
{
    DevScene &d = h->dev;
    const uint32_t nx = s->dims[0], ny = s->dims[1], nz = s->dims[2];
    const size_t texels = h->volume_bytes;
    const int bbias = d.brick_bias;
    const int64_t bgx = d.brick_gx, bgy = d.brick_gy, bgz = d.brick_gz;
#ifndef CT_EXPERIMENTS
    if (ms.experimental) {
        return fail(h, CT_E_INVAL, "march bricks behind virtual memory (CT_FLAG_VMM_BRICKS, CT_SPARSE=2..4) were measured and rejected "
                                   "(DESIGN.md 4.3 item 7b): they exist in the experiments build only (build --variant exp; CT_LIBRARY=libcloudtrace_exp.so)");
    }
#endif
    const int mbias = ((apron + 2) / 3) * 3;
    int64_t mgx = ((int64_t)nx + 2 * mbias + 2) / 3 + 1;
    if (ms.pad_rows) {
        // dense addressing with sparse backing (vmm_back_mbricks): chunks of 2 MiB = 2^14 bricks must hold whole brick rows for
        // empty chunks to have equal bytes, so a row is padded to a power of two bricks (addresses cost nothing)
        int64_t p2 = 1;
        while (p2 < mgx) {
            p2 <<= 1;
        }
        mgx = p2;
    }
    if (!brick_indices_fit(mgx, bgy, bgz) || (int64_t)nx + 2 * mbias >= (1 << 17)) {
        return fail(h, CT_E_INVAL, "volume too large for 32-bit brick indices");
    }
    const size_t dense_bytes = (size_t)(mgx * bgy * bgz) * 128;
    h->mbricks_dense_bytes = h->mbricks_bytes = dense_bytes;
    // The MARCH kernel addresses footprints with 32-bit byte offsets while the march bricks and the shadow volume's bricks are
    // each at most 4 GiB (1024^3: 3.4 GB and 2.2 GB), else with 64-bit ones.  CT_WIDE_OFFSETS=1 forces those (tests).
    const size_t ibricks_bytes = (size_t)(bgx * bgy * bgz) * 128;
    h->shape.wide = std::max(dense_bytes, ibricks_bytes) > (1ull << 32) || knob_flag(h->tune.WIDE_OFFSETS, false);
    HIPCHK(h, h->d_mbricks.alloc(dense_bytes));
    d.mbricks = h->d_mbricks;
    d.m_bias_x = mbias;
    d.m_gx = (int32_t)mgx;
    d.m_gxy = (int32_t)(mgx * bgy);
    DevBuf<uint8_t> tmp_a, tmp_b, tmp_c;
    HIPCHK(h, tmp_a.alloc(texels));
    if (tmp_b.alloc(texels) != hipSuccess) {
        return fail(h, CT_E_NOMEM, "out of device memory (distance transform scratch)");
    }
    hipError_t e = launch_build_mbricks(h->d_density, nx, ny, nz, mbias, bbias, (int)mgx, (int)bgy, (int)bgz,
                                        tmp_a, tmp_b, h->d_mbricks, h->stream);
    if (e == hipSuccess) {
        // the shadow volume (VDBCloud::InitInScatter): its march towards the sun walks the (dense) march bricks
        e = launch_inscatter(d, h->d_inscatter, zero_faces, h->stream);
    }
    if (e == hipSuccess) {
        e = launch_build_bricks(h->d_inscatter, nx, ny, nz, bbias, (int)bgx, (int)bgy, (int)bgz, h->d_ibricks, h->stream);
    }
    const int nee_r = s->estimator == CT_EST_MARCH ? nee_skip_radius(d, mie_finite) : 0;
    if (e == hipSuccess && nee_r > 0) {
        // shadow-zero rows (bit 6 of the march bricks' meta bytes)
        e = tmp_c.alloc(texels);
        if (e == hipSuccess) {
            e = launch_nee_skip_flags(h->d_inscatter, nx, ny, nz, nee_r, mbias, bbias, (int)mgx, (int)bgy, (int)bgz, tmp_a, tmp_c,
                                      h->d_mbricks, h->stream);
            d.nee_reach = nee_skip_reach(d);
            h->nee_skip_r = nee_r;
        }
    }
    if (e == hipSuccess && s->estimator == CT_EST_DELTA && d.delta_nee == 2u) {
        CT_TRY(twin_grid(h));
        e = launch_build_twin_bricks(h->d_density, h->d_inscatter, nx, ny, nz, d.t_bias, d.t_gx, d.t_gy, d.t_gz, h->d_tbricks, h->stream);
    }
    const hipError_t e2 = hipStreamSynchronize(h->stream);
    HIPCHK(h, e);
    HIPCHK(h, e2);
    return ms.sparse ? compact_march_bricks(h, tmp_b) : CT_OK;
}

// ---- Camera::init buffers (Camera.cpp:45-48) + reset (:77-86), and the pipeline of enqueued batches
static int frame_buffers(const CtScene *s, CtHandle h)
{
    const size_t pixels = (size_t)s->width * s->height;
    HIPCHK(h, h->d_frame.alloc(pixels));
    HIPCHK(h, h->d_mean.alloc(pixels));
    HIPCHK(h, h->d_m2.alloc(pixels));
    HIPCHK(h, h->d_screen.alloc(pixels));
    HIPCHK(h, h->d_colsum.alloc(s->width));
    HIPCHK(h, h->d_avg.alloc(2)); // average luminance + the fused tonemap kernel's grid barrier
    HIPCHK(h, h->d_queue.alloc(kQueueWords));
    HIPCHK(h, h->d_cont_count.alloc(6));
    HIPCHK(h, hipMemsetAsync(h->d_cont_count, 0, 6 * sizeof(uint32_t), h->stream));
    // a lane suspends at most one path per launch, and a launch resumes up to 64 paths per wave: the same number
    h->cont_capacity = (size_t)h->shape.blocks * h->shape.threads;
    HIPCHK(h, h->ev_flush0.create());
    HIPCHK(h, h->ev_flush1.create());
    if (h->tune.TIMELINE.get()) {
        const size_t waves = (size_t)h->shape.blocks * h->shape.threads / 64u;
        HIPCHK(h, h->d_timeline.alloc(4 * waves));
        HIPCHK(h, hipMemsetAsync(h->d_timeline, 0, 4 * waves * sizeof(unsigned long long), h->stream));
    }
    HIPCHK(h, h->d_cont_total.alloc(1));
    HIPCHK(h, hipMemsetAsync(h->d_cont_total, 0, sizeof(unsigned long long), h->stream));
    for (auto &c : h->cont) {
        HIPCHK(h, c.alloc(h->cont_capacity * (s->estimator == CT_EST_DELTA ? kContWordsDelta : kContWords)));
    }
    h->left_capacity = h->cont_capacity / 64;   // a wave hands on at most the one job it is working on
    for (auto &c : h->left) {
        HIPCHK(h, c.alloc(h->left_capacity * kLeftWords));
    }
    for (auto &sl : h->slots) {
        HIPCHK(h, sl.queue.alloc(kQueueWords));
        for (Event *e : { &sl.ev_in, &sl.ev_start, &sl.ev_done, &sl.ev_acc0, &sl.ev_acc1 }) {
            HIPCHK(h, e->create());
        }
    }
    HIPCHK(h, h->d_counters.alloc(kCounterCount + 1 + kStatCount));
    HIPCHK(h, h->d_freeze.alloc(8));
    HIPCHK(h, hipMemsetAsync(h->d_freeze, 0, 8 * sizeof(uint32_t), h->stream));
    HIPCHK(h, h->freeze_host.alloc(4));
    memset(h->freeze_host, 0, 4 * sizeof(uint32_t));
    HIPCHK(h, hipMemsetAsync(h->d_frame, 0, pixels * sizeof(float4), h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_mean, 0, pixels * sizeof(float4), h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_m2, 0, pixels * sizeof(float4), h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_screen, 0, pixels * sizeof(uchar4), h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_counters, 0, (kCounterCount + 1 + kStatCount) * sizeof(unsigned long long), h->stream));

    HIPCHK(h, h->d_primary.alloc(2 * pixels));
    HIPCHK(h, h->d_advance.alloc((s->estimator == CT_EST_DELTA ? 4 : 1) * pixels));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CT_OK;
}

// The stages in order.  The order is the dependencies between them:
//  - the shadow volume marches over the DENSE march bricks: after them, before the sparse compaction;
//  - the shadow-zero (NEE-skip) flags follow the shadow volume and precede the compaction, which copies the meta bytes;
//  - the twin bricks hold the shadow volume, so they follow it;
//  - delta_interior's second half needs the twin grid (twin_grid re-evaluates it);
//  - the compaction's coarse clearance reads the distance volume in tmp_b, which lives until the compaction is done.
static int create_impl(const CtScene *s, CtHandle h)
{
    h->scene = *s;
    h->device = s->device;
    h->volume_bytes = (size_t)s->dims[0] * s->dims[1] * s->dims[2];
    h->tune = CtTuning::from_env();
    CT_TRY(open_device(s, h));
    CT_TRY(choose_schedule(s, h));
    scene_uniforms(s, h->dev);
    int apron = 0;
    CT_TRY(apron_grid(s, h, apron));
    CT_TRY(upload_mie(s, h, h->mie_finite));
    CT_TRY(build_apron_bricks(s, h));
    if (s->estimator == CT_EST_DELTA) {
        CT_TRY(build_majorant_grid(s, h));
    }
    const MarchStorage ms = march_storage(s, h->tune.SPARSE);
    h->zero_faces = zero_faces(s->density_host, s->dims[0], s->dims[1], s->dims[2]);
    CT_TRY(build_march_layouts(s, h, apron, ms, h->zero_faces, h->mie_finite));
#ifdef CT_EXPERIMENTS
    if (ms.vmm) {
        CT_TRY(vmm_back_mbricks(h));
    }
#endif
    CT_TRY(frame_buffers(s, h));

    // ---- default pose: Camera.cpp:37-39 through sutil::calculateCameraVariables
    const float eye[3] = { 2.5f, -0.4f, 0.f }, lookat[3] = { 0, 0, 0 }, up[3] = { 0, 1, 0 };
    float U[3], V[3], W[3];
    ct_calculate_camera_variables(eye, lookat, up, 30.0f, (float)s->width / (float)s->height, U, V, W);
    return ct_set_camera(h, eye, U, V, W);
}

extern "C" int ct_create(const CtScene *s, CtHandle *out)
{
    if (!out) {
        return fail(nullptr, CT_E_INVAL, "out is NULL");
    }
    *out = nullptr;
    if (!s) {
        return fail(nullptr, CT_E_INVAL, "scene is NULL");
    }
    if (s->abi_version != CT_ABI_VERSION) {
        return fail(nullptr, CT_E_INVAL, "abi_version %u, library is %u", s->abi_version, CT_ABI_VERSION);
    }
    if (!s->density_host || s->dims[0] < 2 || s->dims[1] < 2 || s->dims[2] < 2 || s->dims[0] > 2048 ||
        s->dims[1] > 2048 || s->dims[2] > 2048) {
        return fail(nullptr, CT_E_INVAL, "density volume missing or dims out of range [2,2048]");
    }
    if (s->mode < 0 || s->mode > 2) {
        return fail(nullptr, CT_E_INVAL, "Invalid Render Mode %d", s->mode); // CloudMaterial.cpp:62
    }
    if (s->estimator != CT_EST_MARCH && s->estimator != CT_EST_DELTA) {
        return fail(nullptr, CT_E_INVAL, "unknown estimator %d", s->estimator);
    }
    if (s->estimator == CT_EST_DELTA && (s->flags & CT_FLAG_SIMPLE_KERNEL)) {
        return fail(nullptr, CT_E_INVAL, "the one-thread-per-pixel cross-check kernel only implements MARCH");
    }
    if (!s->mie_host || !s->chopped_mie_host || s->mie_count != (uint32_t)kMieN) {
        return fail(nullptr, CT_E_INVAL, "Mie tables must be %d floats each", kMieN);
    }
    if (s->width == 0 || s->height == 0 || s->width > 12288 || s->height > 4096) {   // (width: the tonemap kernel keeps a row of column sums in LDS)
        return fail(nullptr, CT_E_INVAL, "frame %ux%u out of range (seed packing x*4096+y needs H <= 4096)", s->width,
                    s->height);
    }
    if (!(s->sample_step > 0.f) || !(s->sample_step <= 0.03125f) || !(s->cloud_size_m > 0.f) ||
        !(s->mean_free_path_m > 0.f) || s->max_depth < 2 || s->max_depth > 65535) {
        // (a suspended path carries its depth in 16 bits: BatchArgs::cont_out)
        return fail(nullptr, CT_E_INVAL, "sample_step/cloud_size_m/mean_free_path_m/max_depth out of range (max_depth 2..65535)");
    }
    if (!(s->cloud_size_m / s->mean_free_path_m * s->sample_step < 80.f)) {
        return fail(nullptr, CT_E_INVAL, "optical depth per step %g too large (must be < 80)",
                    (double)(s->cloud_size_m / s->mean_free_path_m * s->sample_step));
    }
    const float ll = s->light_direction[0] * s->light_direction[0] + s->light_direction[1] * s->light_direction[1] +
                     s->light_direction[2] * s->light_direction[2];
    if (!(ll > 0.f)) {
        return fail(nullptr, CT_E_INVAL, "light_direction is zero");
    }
    if (s->shard_count == 0 || s->shard_index >= s->shard_count) {
        return fail(nullptr, CT_E_INVAL, "shard %u of %u", s->shard_index, s->shard_count);
    }
    CtHandle h = new (std::nothrow) CtHandle_();
    if (!h) {
        return fail(nullptr, CT_E_NOMEM, "out of host memory");
    }
    const int rc = create_impl(s, h);
    if (rc != CT_OK) {
        g_create_error = h->error;
        release(h);
        return rc;
    }
    // host pointers are not retained
    h->scene.density_host = nullptr;
    h->scene.mie_host = nullptr;
    h->scene.chopped_mie_host = nullptr;
    *out = h;
    return CT_OK;
}

extern "C" int ct_destroy(CtHandle h)
{
    release(h);
    return CT_OK;
}

extern "C" const char *ct_last_error(CtHandle h)
{
    return h ? h->error.c_str() : g_create_error.c_str();
}

extern "C" int ct_set_stream(CtHandle h, void *hip_stream)
{
    NEED(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    return CT_OK;
}

extern "C" int ct_set_camera(CtHandle h, const float eye[3], const float U[3], const float V[3], const float W[3])
{
    NEED(h);
    if (!eye || !U || !V || !W) {
        return fail(h, CT_E_INVAL, "camera vectors must not be NULL");
    }
    DevScene &d = h->dev;
    d.ex = eye[0]; d.ey = eye[1]; d.ez = eye[2];
    d.ux = U[0]; d.uy = U[1]; d.uz = U[2];
    d.vx = V[0]; d.vy = V[1]; d.vz = V[2];
    d.wx = W[0]; d.wy = W[1]; d.wz = W[2];
    h->camera_set = true;
    h->queue_dirty = true; // primary rays and the work queue depend on the pose
    discard_ahead(h);      // (and so does every sample rendered ahead of the calls)
    return CT_OK;
}

// What depends on the light, rebuilt in place in the order create_impl documents: the uniforms, the shadow volume (marched over
// the march bricks as they are stored: dense, or sparse through the row table), its apron bricks, bit 6 of the march bricks'
// clearance-0 rows (MARCH), the shadow half of the twin bricks (DELTA, delta_nee == 2).  Every temporary is allocated before
// anything of the handle changes, so an allocation failure leaves the old light in place.  Nothing is in flight (the caller
// has flushed); the stream is idle on return.
static int relight(CtHandle h, const CtScene &s)
{
    DevScene d = h->dev;
    light_uniforms(&s, d);
    const bool march = s.estimator == CT_EST_MARCH;
    const int nee_r = march ? nee_skip_radius(d, h->mie_finite) : 0;
    DevBuf<uint8_t> tmp_a, tmp_c;   // the Chebyshev passes' two scratch volumes
    if (nee_r > 0 && (tmp_a.alloc(h->volume_bytes) != hipSuccess || tmp_c.alloc(h->volume_bytes) != hipSuccess)) {
        (void)hipGetLastError();
        return fail(h, CT_E_NOMEM, "out of device memory (shadow-zero flags scratch); the light is unchanged");
    }
    d.nee_reach = nee_r > 0 ? nee_skip_reach(d) : 0.0f;
    h->scene = s;
    h->dev = d;
    h->nee_skip_r = nee_r;
    discard_ahead(h);   // (samples rendered ahead of the calls saw the old light)
    // A new light is a new scene setup: the next render call starts as a fresh handle's first one does, with the pose's primary
    // rays, pixel list and job order rebuilt and its costs measured again.  The job list decides which samples a lane runs one
    // after the other, and with them what its one-entry footprint cache serves: ct_fetch_counters would otherwise depend on what
    // the handle rendered under the old light.
    h->queue_dirty = true;
    h->tile_deepest.clear();
    const int nx = d.nx, ny = d.ny, nz = d.nz, bbias = d.brick_bias;
    hipError_t e = launch_inscatter(d, h->d_inscatter, h->zero_faces, h->stream);
    if (e == hipSuccess) {
        e = launch_build_bricks(h->d_inscatter, nx, ny, nz, bbias, d.brick_gx, d.brick_gy, d.brick_gz, h->d_ibricks, h->stream);
    }
    if (e == hipSuccess && march) {
        e = launch_shadow_zero_rows(h->d_inscatter, nx, ny, nz, nee_r, d.m_bias_x, bbias, d.m_gx, d.brick_gy, d.brick_gz, tmp_a, tmp_c,
                                    h->d_mbricks, h->d_mrows, h->stream);
    }
    if (e == hipSuccess && h->d_tbricks) {
        e = launch_twin_shadow_half(h->d_inscatter, nx, ny, nz, d.t_bias, d.t_gx, d.t_gy, d.t_gz, h->d_tbricks, h->stream);
    }
    const hipError_t e2 = hipStreamSynchronize(h->stream);   // (before the temporaries go)
    HIPCHK(h, e);
    HIPCHK(h, e2);
    return CT_OK;
}

extern "C" int ct_set_light(CtHandle h, const float direction[3], const float color[3], float intensity)
{
    NEED_NOFLUSH(h);
    // (arguments first: a rejected call leaves the handle exactly as it was, batches in flight included)
    if (!direction) {
        return fail(h, CT_E_INVAL, "light direction must not be NULL");
    }
    if (!std::isfinite(direction[0]) || !std::isfinite(direction[1]) || !std::isfinite(direction[2])) {
        return fail(h, CT_E_INVAL, "light direction is not finite");
    }
    if (!(direction[0] * direction[0] + direction[1] * direction[1] + direction[2] * direction[2] > 0.f)) {
        return fail(h, CT_E_INVAL, "light_direction is zero");
    }
    if (h->vmm.va) {
        // (experiments build: chunks of the virtual range share memory by their meta bytes, bit 6 included)
        return fail(h, CT_E_INVAL, "ct_set_light: march bricks behind virtual memory cannot be re-lit");
    }
    const int rc = flush(h);
    if (rc != CT_OK) {
        return rc;
    }
    CtScene s = h->scene;
    for (int a = 0; a < 3; a++) {
        s.light_direction[a] = direction[a];
        if (color) {
            s.light_color[a] = color[a];
        }
    }
    s.light_intensity = intensity;
    h->light_epoch++;   // (a CtBake made under the old light is stale from here on, whatever relight answers)
    return relight(h, s);
}

// Does the handle keep start records (BatchArgs::start)?  The MARCH kernel's image launches read them; CT_START_RECORDS=0: none (A/B).
static bool start_records(CtHandle h)
{
    return h->scene.estimator == CT_EST_MARCH && !(h->scene.flags & CT_FLAG_SIMPLE_KERNEL) && knob_flag(h->tune.START_RECORDS, true);
}

// Are through pixels settled without a path?  Only where every sample of a pixel takes the pre-walked prefix and runs the
// decisive iteration itself: MARCH's persistent kernel, not mode 1 (the direction is drawn first), not CT_NO_ADVANCE; and not
// at max_depth == 1 outside mode 2, where a sample is capped before its first flight (no lookups, depth_capped + 1).
// CT_THROUGH_PIXELS=0: every box-hitting pixel is listed (A/B, tests).
static bool through_on(CtHandle h)
{
    return h->scene.estimator == CT_EST_MARCH && !(h->scene.flags & CT_FLAG_SIMPLE_KERNEL) && h->scene.mode != 1 && !h->no_advance &&
           (h->scene.max_depth > 1 || h->scene.mode == 2) && knob_flag(h->tune.THROUGH_PIXELS, true);
}

// Primary rays of the current pose + the list of this shard's pixels whose samples need a path (they hit the box and are
// no through pixels), in tile-Morton order, cut into groups of 64 (one wave's worth).
// ... and, from those, the start record of every slot of the list.
static int rebuild_queue(CtHandle h)
{
    TracePhase trace(h, "rebuild_queue");
    const uint32_t W = h->scene.width, H = h->scene.height;
    const size_t pixels = (size_t)W * H;
    const bool through = through_on(h);
    HIPCHK(h, launch_primary_rays(h->dev, h->d_primary, h->stream));
    if (h->scene.estimator == CT_EST_DELTA) {
        HIPCHK(h, launch_primary_advance_delta(h->dev, h->d_primary, h->d_advance, h->stream));
    } else {
        HIPCHK(h, launch_primary_advance(h->dev, h->d_primary, h->d_advance, through, h->stream));
    }
    // (the class plane and, behind it, the word of the through pixels' steps: one download)
    const size_t sum_at = (pixels + 7u) & ~(size_t)7u, plane_bytes = sum_at + sizeof(unsigned long long);
    HIPCHK(h, h->d_hit.reserve(plane_bytes));   // (the same size at every call: allocated at the first)
    HIPCHK(h, h->hit_host.reserve(plane_bytes));
    HIPCHK(h, hipMemsetAsync(h->d_hit + sum_at, 0, sizeof(unsigned long long), h->stream));
    HIPCHK(h, launch_hit_flags(h->d_primary, through ? h->d_advance : nullptr, h->d_hit, (uint32_t)pixels, W, h->scene.shard_index,
                               h->scene.shard_count, (unsigned long long *)(h->d_hit + sum_at), h->stream));
    HIPCHK(h, hipMemcpyAsync(h->hit_host, h->d_hit, plane_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const uint32_t tiles_x = h->dev.tiles_x, tiles_y = h->dev.tiles_y;
    std::vector<uint32_t> list;
    list.reserve(pixels / std::max(1u, h->scene.shard_count) + 64);
    const plan::PixelCounts n = plan::list_pixels(
        h->hit_host, W, H, tiles_x, tiles_y, h->tile_hilbert,
        [&](uint32_t tx, uint32_t ty) { return tile_owner(tx, ty, h->scene.shard_count) == h->scene.shard_index; }, list, h->group_tile);
    plan::seed_group_order(h->group_tile, h->tile_deepest, (size_t)tiles_x * tiles_y, h->group_order);
    h->own_pixels = n.own;
    h->listed_pixels = n.listed;
    h->through_pixels = n.through;
    h->hit_pixels = n.listed + n.through;
    h->miss_pixels = n.own - h->hit_pixels;
    {
        unsigned long long steps = 0;
        memcpy(&steps, h->hit_host + sum_at, sizeof steps);
        h->through_steps = steps;
    }
    h->n_groups = (uint32_t)(list.size() / 64);
    // (the old contents are dead: free, then allocate)
    HIPCHK(h, h->d_pixels.reserve((size_t)h->n_groups * 64));
    HIPCHK(h, h->d_cost.reserve(2 * (size_t)h->n_groups));
    HIPCHK(h, h->d_group_rank.reserve((size_t)h->n_groups));
    HIPCHK(h, h->d_group_order.reserve((size_t)h->n_groups));
    if (start_records(h)) {
        HIPCHK(h, h->d_start.reserve(2 * (size_t)h->n_groups * 64));
    }
    h->group_depth.assign(h->n_groups, 0.f);
    if (h->n_groups) {
        HIPCHK(h, hipMemcpyAsync(h->d_pixels, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                                 h->stream));
        HIPCHK(h, hipMemsetAsync(h->d_cost, 0, 2 * (size_t)h->n_groups * sizeof(uint32_t), h->stream));
        if (h->d_start) {
            // (this function alone writes d_primary, d_advance and d_pixels, so the records are as fresh as those)
            const bool prefix = h->scene.mode != 1 && !h->no_advance;
            HIPCHK(h, launch_start_records(h->dev, h->d_pixels, h->n_groups * 64u, h->d_primary, prefix ? h->d_advance : nullptr, h->d_start,
                                           h->stream));
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    h->queue_dirty = false;
    h->order_tuned = false;
    h->jobs_S = 0; // force a new job list
    return CT_OK;
}

static bool short_batch(CtHandle h, uint32_t S)
{
    return plan::short_batch(h->scene.estimator == CT_EST_DELTA, S, h->hit_pixels);
}

// What the handle and the knobs decide about a job list for batches of S subframes.
static plan::JobPolicy job_policy(CtHandle h, uint32_t S)
{
    plan::JobPolicy p;
    p.unit = (h->scene.estimator == CT_EST_DELTA) ? 1.f : 16.f;
    p.brief = short_batch(h, S);
    // (per-XCD queues are cut at equal shares of the MEASURED cost: before anything is measured they would be equal shares of
    // pixels, and the XCD that got the cloud's body would finish long after the others)
    const bool queues = (h->queues_enabled || (p.brief && !h->tune.XCD_QUEUES.get())) && !(h->scene.flags & CT_FLAG_SIMPLE_KERNEL) &&
                        (h->order_tuned || h->tune.XCD_QUEUES_UNTUNED.get());
    p.nq = (queues && h->n_groups >= (uint32_t)kQueues) ? (uint32_t)kQueues : 1u;
    p.regions_wanted = (p.brief && !h->queues_enabled && !h->tune.XCD_REGIONS.get()) ? 16u : h->regions;
    p.job_work = (p.brief && !h->tune.JOB_WORK.get()) ? 4.f : h->job_work;
    p.job_max = h->job_max;
    p.shared_depth = h->shared_depth;
    p.order_tuned = h->order_tuned;
    p.chunk_interleave = h->chunk_interleave;
    p.chunk_morton = h->chunk_morton;
    return p;
}

// Job list for batches of S subframes, in chunks of chunk_groups pixel groups (plan::fill_jobs).
static int build_jobs(CtHandle h, uint32_t S, uint32_t chunk_groups)
{
    chunk_groups = plan::clamp_chunk_groups(chunk_groups, h->n_groups);
    if (h->jobs_S >= S && h->jobs_brief == short_batch(h, S) && h->chunk_groups == chunk_groups) {
        return CT_OK; // a list for a larger batch serves a smaller one (the kernel clips the jobs)
    }
    TracePhase trace(h, "build_jobs");
    if (h->order_tuned) {
        S = std::max(S, h->jobs_hint);   // (the cost-measuring launch gets a list of its own: one-subframe jobs, its few subframes only)
    }
    const plan::JobPolicy policy = job_policy(h, S);
    const size_t total_jobs = plan::count_jobs(policy, h->group_depth, S);
    HIPCHK(h, h->jobs_host_g.reserve(total_jobs, total_jobs / 4 + 1024));
    HIPCHK(h, h->jobs_host_s.reserve(total_jobs, total_jobs / 4 + 1024));
    plan::JobPlan jp;
    plan::fill_jobs(policy, h->group_depth, h->group_order, S, chunk_groups, h->jobs_host_g, h->jobs_host_s, jp);
    if (h->tune.STATS.get()) {
        fprintf(stderr, "[cloudtrace] job queues (S=%u, %u chunk(s) of %u groups):", S, jp.n_chunks, chunk_groups);
        for (int x = 0; x <= kQueues; x++) {
            fprintf(stderr, " q%d weight %.0f;", x, jp.q_weight[x]);
        }
        fprintf(stderr, "\n");
    }
    h->job_order = std::move(jp.job_order);
    h->chunk_q_begin = std::move(jp.chunk_q_begin);
    if (h->n_groups) {
        HIPCHK(h, hipMemcpyAsync(h->d_group_rank, jp.rank.data(), jp.rank.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->d_group_order, h->job_order.data(), h->job_order.size() * sizeof(uint32_t),
                                 hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    h->chunk_groups = chunk_groups;
    h->n_chunks = jp.n_chunks;
    h->n_jobs = (uint32_t)jp.n_jobs;
    HIPCHK(h, h->d_job_group.reserve(h->n_jobs, h->n_jobs / 4));
    HIPCHK(h, h->d_job_sub.reserve(h->n_jobs, h->n_jobs / 4));
    if (h->n_jobs) {
        HIPCHK(h, hipMemcpyAsync(h->d_job_group, h->jobs_host_g, jp.n_jobs * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->d_job_sub, h->jobs_host_s, jp.n_jobs * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));   // (the pinned list is rewritten by the next build)
    }
    h->jobs_S = S;
    h->jobs_brief = policy.brief;
    return CT_OK;
}

// The group order and depths from what the cost-measuring launch of a pose has booked (plan::tune_groups).
static int tune_order(CtHandle h, uint32_t measured_subframes)
{
    TracePhase trace(h, "tune_order");
    h->order_tuned = true;
    if (h->n_groups < 2 || measured_subframes == 0) {
        return CT_OK;
    }
    std::vector<uint32_t> cost(2 * (size_t)h->n_groups);
    HIPCHK(h, hipMemcpyAsync(cost.data(), h->d_cost, cost.size() * sizeof(uint32_t), hipMemcpyDeviceToHost,
                             h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    plan::tune_groups(cost.data(), h->n_groups, measured_subframes, h->group_tile, (size_t)h->dev.tiles_x * h->dev.tiles_y, h->group_order,
                      h->group_depth, h->tile_deepest);
    if (h->tune.STATS.get()) {
        const plan::CostShare cs = plan::cost_share(cost.data(), h->n_groups);
        fprintf(stderr, "[cloudtrace] cost share by deepest-path class (2^(k-1) <= depth < 2^k):");
        for (int k = 0; k < 34; k++) {
            if (cs.count[k]) {
                fprintf(stderr, " k=%d groups %u share %.1f%%;", k, cs.count[k], 100.0 * cs.share[k] / std::max(cs.total, 1.0));
            }
        }
        fprintf(stderr, "\n");
    }
    h->jobs_S = 0; // rebuild the job list with the new order
    return CT_OK;
}

// Entries of one subframe in the batch scratch: the columns of a chunk's pixel groups (compact) or the frame (simple).
static size_t frame_stride(CtHandle h)
{
    if (h->scene.flags & CT_FLAG_SIMPLE_KERNEL) {
        return (size_t)h->scene.width * h->scene.height;
    }
    return (size_t)std::max(h->chunk_groups, 1u) * 64;
}

static int wanted_regions(CtHandle h, uint64_t need, uint64_t budget_float4)
{
    return plan::wanted_regions(h->max_age_override, need, budget_float4);
}

static uint64_t scratch_slot_bytes(CtHandle h)
{
    if (h && h->scratch_cap_bytes) {
        return h->scratch_cap_bytes;   // (the device could not give more: ensure_frames failed with less)
    }
    // CT_SCRATCH_GIB sets the size of one of the two regions a long batch uses.  Default 16: the 1024-spp job of a 1024^2
    // frame is then ONE launch, 14 GB, instead of two of 512 -- a launch costs a few ms besides its samples -- and 28 GB of
    // scratch are a tenth of this GPU's memory.  Allocated as needed; a device that cannot give that much gets less (below).
    if (h->tune.SCRATCH_MIB) {   // (tests: chunks of a few pixel groups on small frames)
        return (uint64_t)knob_int(h->tune.SCRATCH_MIB, 1, 65536, 0) << 20;
    }
    return (uint64_t)knob_int(h->tune.SCRATCH_GIB, 1, 64, 16) << 30;
}

static uint32_t groups_per_chunk(CtHandle h, uint32_t S)
{
    if (h->scene.flags & CT_FLAG_SIMPLE_KERNEL) {
        return std::max(h->n_groups, 1u);
    }
    return plan::groups_per_chunk(scratch_slot_bytes(h) / sizeof(float4), S, h->n_groups);
}

// At least `total` float4 of per-sample scratch (nothing may be in flight when it grows: the caller has flushed).
static int reserve_frames(CtHandle h, size_t total)
{
    if (total <= h->d_frames_all.capacity()) {
        return CT_OK;
    }
    // free, then allocate: the scratch is several GB, and two of them may not fit
    h->slot_capacity = 0;
    HIPCHK(h, h->d_frames_all.reset());
    const hipError_t e = h->d_frames_all.alloc(total);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, e == hipErrorOutOfMemory ? CT_E_NOMEM : CT_E_HIP, "per-sample scratch of %.1f GB: %s", (double)total * 16e-9,
                    hipGetErrorString(e));
    }
    // touch it now: the first launch that writes a fresh part of a large allocation has been seen to
    // take 30 ms longer (measured on the 3.5 GB scratch of a 256-subframe batch)
    HIPCHK(h, hipMemsetAsync(h->d_frames_all, 0, total * sizeof(float4), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CT_OK;
}

// The per-sample scratch laid out for launches of S subframes over chunks of h->chunk_groups pixel groups: regions of
// S * stride entries each.  Nothing may be in flight when the layout changes (the caller has flushed).
static int ensure_frames(CtHandle h, uint32_t S, bool relayout)
{
    const size_t need = std::max<size_t>((size_t)S * frame_stride(h), 1);
    if (!relayout && need <= h->slot_capacity) {
        return CT_OK;   // (a waited-for batch, the cost-measuring launch: any region that is large enough will do)
    }
    discard_ahead(h);
    const uint64_t budget = 2 * scratch_slot_bytes(h) / sizeof(float4);
    // (a waited-for batch needs one region; the others are allocated when batches are first enqueued)
    const int regions = relayout ? wanted_regions(h, need, std::max<uint64_t>(budget, 2 * need)) : 1;
    size_t total = (size_t)regions * need;
    if (total > 0xffffffffull) {
        if ((relayout ? 2 : 1) * need > 0xffffffffull) {
            return fail(h, CT_E_INVAL, "batch of %u subframes is too large for 32-bit result indices", S);
        }
        total = (0xffffffffull / need) * need;
    }
    {
        const int rc = reserve_frames(h, total);
        if (rc != CT_OK) {
            return rc;
        }
    }
    h->slot_capacity = need;
    h->n_regions = (int)std::min<size_t>((size_t)regions, h->d_frames_all.capacity() / need);
    h->layout_S = S;
    h->next_slot = 0;
    return CT_OK;
}

static float4 *slot_frames(CtHandle h, int slot)
{
    return h->d_frames_all + (size_t)slot * h->slot_capacity;
}

// Waits for one slot's launch (and its accumulate kernel, if enqueued) and books the kernel times.
static int collect(CtHandle h, CtHandle_::Slot &sl)
{
    if (!sl.pending) {
        return CT_OK;
    }
    sl.pending = false;
    HIPCHK(h, hipEventSynchronize(sl.accumulated ? sl.ev_acc1 : sl.ev_done));
    float ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, sl.ev_start, sl.ev_done));
    h->render_ms += ms;
    if (h->tune.TRACE.get()) {
        uint32_t cnt[3] = { 0, 0, 0 };
        hipMemcpy(cnt, h->d_cont_count, sizeof cnt, hipMemcpyDeviceToHost);
        fprintf(stderr, "[cloudtrace] estimator launch %.2f ms (suspended paths per buffer now: %u %u, cursor %u)\n", ms,
                cnt[0], cnt[1], cnt[2]);
    }
    if (sl.accumulated) {
        HIPCHK(h, hipEventElapsedTime(&ms, sl.ev_acc0, sl.ev_acc1));
        h->accum_ms += ms;
    }
    h->launches += 1;
    return CT_OK;
}

// The convergence test on the running mean after `subframes` subframes, and its outcome copied to where the host can
// read it without waiting (ct_converged_at).
int ct::enqueue_convergence_test(CtHandle h, uint32_t subframes)
{
    HIPCHK(h, launch_converged_freeze(h->d_mean, h->d_m2, subframes, (uint64_t)h->scene.width * h->scene.height, 500u /* Camera.cpp:267 */,
                                      h->d_freeze, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->freeze_host, h->d_freeze, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    return CT_OK;
}

// The accumulate kernel(s) for subframes [sl.acc_done, sl.acc_done + n) of a slot's batch.  With stop-when-converged they
// are cut at the multiples of its cadence and each is followed by the test (a batch rendered in several chunks of pixel
// groups is a whole image only after its last chunk: it is tested there, if it ends on a multiple).
static int enqueue_accumulate(CtHandle h, CtHandle_::Slot &sl, const float4 *frames, bool dense, uint32_t n)
{
    const bool simple = (h->scene.flags & CT_FLAG_SIMPLE_KERNEL) != 0;
    const bool chunked = !(simple || dense) && h->n_chunks > 1;
    const uint32_t cadence = h->stop_cadence;
    const uint32_t *frozen = cadence ? h->d_freeze : nullptr;
    HIPCHK(h, hipEventRecord(sl.ev_acc0, h->stream));
    while (n != 0u) {
        const uint32_t off = sl.acc_done, next = sl.first + off;   // (next: the subframe id of the first sample of this piece)
        uint32_t piece = n;
        if (cadence && !chunked) {
            piece = std::min(n, cadence - (next - 1u) % cadence);
        }
        if (simple || dense) {
            HIPCHK(h, launch_accumulate_batch(frames + (size_t)off * h->scene.width * h->scene.height, h->d_mean, h->d_m2, next, piece,
                                              h->scene.width, h->scene.height, h->scene.shard_index, h->scene.shard_count,
                                              h->d_counters + 8, frozen, h->stream));
        } else {
            HIPCHK(h, launch_accumulate_list(frames + (size_t)off * frame_stride(h), (uint32_t)frame_stride(h), h->d_pixels, sl.groups * 64u,
                                             h->n_chunks <= 1 ? nullptr : h->d_group_order, sl.rank_base,
                                             sl.with_misses, h->d_hit, h->d_mean, h->d_m2, next, piece, h->scene.width,
                                             h->scene.height, h->scene.shard_index, h->scene.shard_count, h->d_counters + 8, frozen,
                                             h->stream));
        }
        sl.acc_done += piece;
        n -= piece;
        const uint32_t upto = sl.first + sl.acc_done - 1u;
        const bool whole_image = !chunked || (sl.last_chunk && sl.acc_done == sl.S);
        if (cadence && whole_image && upto % cadence == 0u && upto >= h->stop_min) {
            const int rc = enqueue_convergence_test(h, upto);
            if (rc != CT_OK) {
                return rc;
            }
        }
    }
    HIPCHK(h, hipEventRecord(sl.ev_acc1, h->stream));   // (of several partial accumulates the last one is the one whose time is booked)
    sl.accumulated = true;
    return CT_OK;
}

// How far the running mean may follow: everything that is complete, or -- with render-ahead -- the calls minus the lag that
// lets every call find its share complete (see CtHandle_::ahead).
static uint32_t accumulate_target(CtHandle h)
{
    if (h->ahead == 0) {
        return 0xffffffffu;
    }
    const uint64_t lag = (uint64_t)std::max(h->n_regions - 1, 1) * h->ahead;
    return h->subframes > lag ? (uint32_t)(h->subframes - lag) : 0u;
}

// Enqueues the accumulate kernels of the complete batches, oldest first, up to subframe `target`.
static int advance_accumulate(CtHandle h, uint32_t target)
{
    while (!h->waiting.empty()) {
        const int w = h->waiting.front();
        CtHandle_::Slot &sl = h->slots[w];
        if (!sl.complete) {
            break;
        }
        const uint32_t next = sl.first + sl.acc_done, last = sl.first + sl.S - 1u;
        const uint32_t upto = std::min(last, target);
        if (upto >= next && sl.acc_done < sl.S) {
            const int rc = enqueue_accumulate(h, sl, slot_frames(h, w), false, upto - next + 1u);
            if (rc != CT_OK) {
                return rc;
            }
        }
        if (sl.acc_done < sl.S) {
            break;
        }
        sl.awaits_accumulate = false;
        h->waiting.erase(h->waiting.begin());
    }
    return CT_OK;
}

// Forgets the subframes that were rendered ahead of the calls (the pose, the layout of the scratch or the count of
// subframes changes).  Nothing may be in flight: the caller has flushed, so what is left in `waiting` is exactly that.
void ct::discard_ahead(CtHandle h)
{
    for (int w : h->waiting) {
        h->slots[w].awaits_accumulate = false;
    }
    h->waiting.clear();
    h->rendered = h->subframes;
}

// The estimator launch itself: the kernel that fits the handle and the batch.
static int launch_estimator(CtHandle h, const BatchArgs &ba)
{
    DevScene sc = h->dev;
    if (ba.S != 0 && short_batch(h, ba.S) && !h->tune.REGEN_MIN.get()) {
        sc.regen_min = 16;   // (see short_batch)
    }
    bool launched = false;
#ifdef CT_EXPERIMENTS
    if (h->exchange && !ba.cost && !ba.cont_in && !ba.cont_out && h->scene.estimator == CT_EST_DELTA) {
        if (h->exchange == 2) {
            HIPCHK(h, launch_render_delta_w(sc, ba, h->xshape, h->stream));
        } else {
            HIPCHK(h, launch_render_delta_x(sc, ba, h->xshape, h->stream));
        }
        launched = true;
    }
#endif
    if (launched) {
        // (an experiments-build kernel rendered the batch)
    } else if (h->scene.estimator == CT_EST_DELTA) {
        HIPCHK(h, launch_render_delta(sc, ba, h->shape, h->stream));
    } else {
        HIPCHK(h, launch_render_persistent(sc, ba, h->shape, h->stream));
    }
    return CT_OK;
}

// Enqueues one launch of the estimator over S subframes.  `frames` is the dense frame buffer
// (ct_render_subframe) or NULL for the slot's region of the scratch.  With `suspend` the launch hands its
// surviving paths to the next one and the batch's accumulate kernel follows the launch that is max_age = n_regions - 1
// batches younger; the paths the previous launch suspended are resumed in any case.  Does not wait.
static int submit_batch(CtHandle h, int slot, float4 *dense_frames, uint32_t first, uint32_t S, bool accumulate,
                        bool suspend, uint32_t chunk)
{
    CtHandle_::Slot &sl = h->slots[slot];
    const bool simple = (h->scene.flags & CT_FLAG_SIMPLE_KERNEL) != 0;
    const bool dense = dense_frames != nullptr;
    const uint32_t max_age = (uint32_t)(h->n_regions - 1);
    const uint32_t rank_base = chunk * h->chunk_groups;
    const uint32_t chunk_n = h->n_groups > rank_base ? std::min(h->chunk_groups, h->n_groups - rank_base) : 0u;
    BatchArgs ba{};
    ba.frames = dense ? dense_frames : (simple ? slot_frames(h, slot) : h->d_frames_all);
    ba.frame_stride = (simple || dense) ? 0u : (uint32_t)frame_stride(h);
    ba.out_offset = (simple || dense) ? 0u : (uint32_t)((size_t)slot * h->slot_capacity);
    ba.primary = h->d_primary;
    ba.advance = h->no_advance ? nullptr : h->d_advance;
    ba.pixels = h->d_pixels;
    ba.start = dense ? nullptr : h->d_start;   // (a dense frame is indexed by pixel, which a start record does not hold)
    ba.group_rank = (simple || dense || h->n_chunks <= 1) ? nullptr : h->d_group_rank;   // (one chunk: column g * 64, as ever)
    ba.rank_base = rank_base;
    ba.job_group = h->d_job_group;
    ba.job_sub = h->d_job_sub;
    // the cost-measuring launch of a pose: every path leaves what it cost beside its result, summed per group below
    const bool measure = !h->order_tuned && !simple && !dense && chunk_n != 0u;
    if (measure) {
        const size_t entries = (size_t)S * frame_stride(h);
        HIPCHK(h, h->d_cost_plane.reserve(entries, entries / 4));
        HIPCHK(h, hipMemsetAsync(h->d_cost_plane, 0, entries * sizeof(uint2), h->stream));
        ba.cost = h->d_cost_plane;
    }
    static const std::array<uint32_t, kQueues + 2> no_jobs{};
    const auto &qb = chunk < h->chunk_q_begin.size() ? h->chunk_q_begin[chunk] : no_jobs;   // (the simple kernel has no job list)
    ba.n_jobs = qb[kQueues + 1];            // (absolute index of the chunk's end: the job that raises the "list empty" flag)
    for (int x = 0; x <= kQueues + 1; x++) {
        ba.q_begin[x] = qb[x];
    }
    const uint32_t chunk_jobs = qb[kQueues + 1] - qb[0];
    ba.first_subframe = first;
    ba.S = S;
    ba.queue = sl.queue;
    ba.counters = h->d_counters;
    ba.stats = h->d_counters + kCounterCount + 1;
    ba.timeline = h->d_timeline;
    ba.touched_density = h->d_touched[0];
    ba.touched_shadow = h->d_touched[1];
    if (suspend && short_batch(h, S) && h->serpentine) {
        ba.reverse = (uint32_t)(h->launch_no & 1u);
    }
    const int buf_out = (int)(h->launch_no & 1u), buf_in = buf_out ^ 1;
    ZeroList zero;
    if (h->cont_live) {
        ba.cont_in = h->cont[buf_in];
        ba.cont_in_count = h->d_cont_count + buf_in;
        ba.cont_cursor = h->d_cont_count + 2;
        ba.left_in = h->left[buf_in];
        ba.left_in_count = h->d_cont_count + 3 + buf_in;
        ba.left_cursor = h->d_cont_count + 5;
        zero.add(h->d_cont_count + 2, 1);
        zero.add(h->d_cont_count + 5, 1);
    }
    if (suspend) {
        ba.cont_out = h->cont[buf_out];
        ba.cont_out_count = h->d_cont_count + buf_out;
        ba.cont_capacity = (uint32_t)h->cont_capacity;
        ba.max_age = std::max(1u, max_age);
        ba.cont_total = h->d_cont_total;
        if (h->hand_on_jobs) {
            ba.left_out = h->left[buf_out];
            ba.left_out_count = h->d_cont_count + 3 + buf_out;
            ba.left_capacity = (uint32_t)h->left_capacity;
        }
        zero.add(h->d_cont_count + buf_out, 1);
        zero.add(h->d_cont_count + 3 + buf_out, 1);
    }
    zero.add(sl.queue, kQueueWords);
    HIPCHK(h, launch_zero_words(zero, h->stream));
    if (h->debug_invariants && !simple && !dense && h->n_groups != 0) {
        // NaNs (with a NaN alpha) wherever this batch is going to write: a sample that is never written cannot
        // pass for the one an earlier batch left there
        HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)slot_frames(h, slot), 0x7fc0deadu, (size_t)S * frame_stride(h) * 4u,
                                    h->stream));
    }
    HIPCHK(h, hipEventRecord(sl.ev_start, h->stream));
    if (simple) {
        h->host_paths += h->own_pixels * S;
        h->host_hits += h->hit_pixels * S;
        for (uint32_t s = 0; s < S; s++) {
            BatchArgs one = ba;
            one.frames = ba.frames + (size_t)s * h->scene.width * h->scene.height;
            one.first_subframe = first + s;
            one.S = 1;
            HIPCHK(h, launch_render_simple(h->dev, one, h->scene.shard_index, h->scene.shard_count, h->stream));
        }
    } else {
        if (chunk_jobs != 0 || ba.cont_in) {
            const int rc = launch_estimator(h, ba);
            if (rc != CT_OK) {
                return rc;
            }
            if (measure) {
                HIPCHK(h, launch_cost_reduce(h->d_cost_plane, (uint32_t)frame_stride(h), S, chunk_n,
                                             h->n_chunks <= 1 ? nullptr : h->d_group_order, rank_base, h->d_cost,
                                             h->d_cost + h->n_groups, h->stream));
            }
        }
        // (every group is full but the last one of the pixel list, which padding completes; it sits somewhere in the job order)
        uint64_t chunk_hits = 0;
        for (uint32_t r = rank_base; r < rank_base + chunk_n; r++) {
            chunk_hits += (h->job_order[r] + 1u == h->n_groups) ? 64u - (uint64_t)((uint64_t)h->n_groups * 64u - h->listed_pixels) : 64u;
        }
        if (chunk == 0) {
            h->host_paths += h->own_pixels * S;
            // (the samples of through pixels, which no kernel runs: a box hit and the pixel's lookups each)
            h->host_hits += h->through_pixels * S;
            h->host_lookups += h->through_steps * S;
            h->host_settled += h->through_pixels * S;
        }
        h->host_hits += chunk_hits * S;
        h->iv_expected_dealt += chunk_hits * S;
    }
    HIPCHK(h, hipEventRecord(sl.ev_done, h->stream));
    h->launch_no += 1;
    h->cont_live = suspend && !simple;
    sl.first = first;
    sl.S = S;
    sl.rank_base = rank_base;
    sl.groups = chunk_n;
    sl.with_misses = chunk == 0;
    sl.last_chunk = simple || dense || chunk + 1u >= std::max(h->n_chunks, 1u);
    sl.pending = true;
    sl.accumulated = false;
    sl.awaits_accumulate = false;
    sl.complete = false;
    sl.acc_done = 0;
    if (accumulate) {
        if (suspend) {
            sl.awaits_accumulate = true;
            h->waiting.push_back(slot);
            // every batch that max_age launches have followed is complete: its accumulate kernels may go behind this launch
            uint32_t younger = 0;
            for (size_t i = h->waiting.size(); i-- > 0;) {
                CtHandle_::Slot &w = h->slots[h->waiting[i]];
                if (!w.complete && ++younger > max_age) {
                    w.complete = true;
                }
            }
            return advance_accumulate(h, accumulate_target(h));
        } else {
            sl.complete = true;
            const int rc = enqueue_accumulate(h, sl, dense ? dense_frames : slot_frames(h, slot), dense, S);
            if (rc != CT_OK) {
                return rc;
            }
        }
    }
    return CT_OK;
}

// Nothing is in flight: the conservation identities of CtHandle_::debug_invariants must hold.
static int check_invariants(CtHandle h)
{
    unsigned long long iv[4] = { 0, 0, 0, 0 }, bad = 0;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(iv, h->d_counters + kCounterCount + 1 + 64, sizeof iv, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(&bad, h->d_counters + 8, sizeof bad, hipMemcpyDeviceToHost));
    h->iv_checks += 1;
    const unsigned long long dealt = iv[0], resumed = iv[1], written = iv[2], suspended = iv[3];
    const bool simple = (h->scene.flags & CT_FLAG_SIMPLE_KERNEL) != 0;
    const bool ok = simple || (dealt + resumed == written + suspended && resumed == suspended && dealt == h->iv_expected_dealt &&
                               bad == 0);
    if (!ok) {
        h->iv_violations += 1;
        fprintf(stderr, "[cloudtrace] INVARIANT VIOLATED: dealt %llu (host expects %llu) resumed %llu written %llu suspended %llu, "
                        "samples without alpha 1 seen by accumulate: %llu\n",
                dealt, (unsigned long long)h->iv_expected_dealt, resumed, written, suspended, bad);
        return fail(h, CT_E_STATE, "invariant violated: dealt %llu (expected %llu) resumed %llu written %llu suspended %llu bad samples %llu",
                    dealt, (unsigned long long)h->iv_expected_dealt, resumed, written, suspended, bad);
    }
    return CT_OK;
}

// Every batch in flight has finished when this returns.  Batches that still wait for suspended paths get ONE launch that
// only resumes them (no jobs, no suspension: everything runs to its end), then their accumulate kernels in order.
int ct::flush(CtHandle h)
{
    if (h->cont_live) {
        BatchArgs ba{};
        ba.frames = h->d_frames_all;
        ba.frame_stride = (uint32_t)frame_stride(h);   // (unused: resumed paths and handed-on jobs carry their own places)
        ba.primary = h->d_primary;
        ba.advance = h->no_advance ? nullptr : h->d_advance;
        ba.pixels = h->d_pixels;
        ba.start = h->d_start;
        ba.job_group = h->d_job_group;
        ba.job_sub = h->d_job_sub;
        ba.n_jobs = 0;                  // q_begin stays all zero: every queue is empty
        ba.first_subframe = 1;
        ba.S = 0;
        ba.queue = h->d_queue;
        ba.counters = h->d_counters;
        ba.stats = h->d_counters + kCounterCount + 1;
        const int buf_in = (int)((h->launch_no & 1u) ^ 1u);
        ba.cont_in = h->cont[buf_in];
        ba.cont_in_count = h->d_cont_count + buf_in;
        ba.cont_cursor = h->d_cont_count + 2;
        ba.left_in = h->left[buf_in];
        ba.left_in_count = h->d_cont_count + 3 + buf_in;
        ba.left_cursor = h->d_cont_count + 5;
        HIPCHK(h, hipMemsetAsync(h->d_cont_count + 2, 0, sizeof(uint32_t), h->stream));
        HIPCHK(h, hipMemsetAsync(h->d_cont_count + 5, 0, sizeof(uint32_t), h->stream));
        HIPCHK(h, hipMemsetAsync(h->d_queue, 0, kQueueWords * sizeof(uint32_t), h->stream));
        HIPCHK(h, hipEventRecord(h->ev_flush0, h->stream));
        const int rc = launch_estimator(h, ba);
        if (rc != CT_OK) {
            return rc;
        }
        HIPCHK(h, hipEventRecord(h->ev_flush1, h->stream));
        h->launch_no += 1;
        h->cont_live = false;
        HIPCHK(h, hipEventSynchronize(h->ev_flush1));
        float ms = 0;
        HIPCHK(h, hipEventElapsedTime(&ms, h->ev_flush0, h->ev_flush1));
        h->render_ms += ms; // the launch that only resumes belongs to the estimator's time
        if (h->tune.TRACE.get()) {
            fprintf(stderr, "[cloudtrace] resume-only launch %.2f ms\n", ms);
        }
    }
    for (int w : h->waiting) {
        h->slots[w].complete = true;
    }
    {
        // everything the caller has asked for; what was rendered ahead of the calls stays in its region for the next ones
        const int rc = advance_accumulate(h, h->ahead ? h->subframes : 0xffffffffu);
        if (rc != CT_OK) {
            return rc;
        }
    }
    for (int k = 0; k < CtHandle_::kMaxRegions; k++) {
        const int rc = collect(h, h->slots[k]);
        if (rc != CT_OK) {
            return rc;
        }
    }
    return h->debug_invariants ? check_invariants(h) : CT_OK;
}

// Job list etc. for batches of S subframes; everything in flight is waited for when it has to change.
static int prepare_batches(CtHandle h, uint32_t S)
{
    const bool simple = (h->scene.flags & CT_FLAG_SIMPLE_KERNEL) != 0;
    if (simple) {
        h->chunk_groups = std::max(h->n_groups, 1u);
        h->n_chunks = 1;
        return CT_OK;
    }
    if (h->queue_dirty) {
        int rc = flush(h);
        discard_ahead(h);
        if (rc == CT_OK) {
            rc = rebuild_queue(h);
        }
        if (rc != CT_OK) {
            return rc;
        }
    }
    const uint32_t want = groups_per_chunk(h, S);
    if (h->jobs_S < S || h->jobs_brief != short_batch(h, S) || h->chunk_groups != want || h->chunk_q_begin.empty()) {
        const int rc = flush(h);   // the job list (and with it the layout of the scratch) changes: nothing may be in flight
        discard_ahead(h);
        return rc == CT_OK ? build_jobs(h, S, want) : rc;
    }
    return CT_OK;
}

// One batch of S subframes (every chunk of the pixel groups, + optional accumulate), waited for, every path run to its
// end.  `dense_frames` is the frame buffer of ct_render_subframe or NULL for the batch scratch.
static int run_batch(CtHandle h, float4 *dense_frames, uint32_t first, uint32_t S, bool accumulate)
{
    int rc = flush(h);
    discard_ahead(h);   // (slot 0 is about to be reused)
    if (rc == CT_OK) {
        rc = prepare_batches(h, S);
    }
    if (rc == CT_OK && !dense_frames) {
        rc = ensure_frames(h, S, false);
    }
    if (rc != CT_OK) {
        return rc;
    }
    for (uint32_t c = 0; c < std::max(h->n_chunks, 1u) && rc == CT_OK; c++) {
        rc = submit_batch(h, 0, dense_frames, first, S, accumulate, false, c);
        if (rc == CT_OK) {
            rc = collect(h, h->slots[0]);
        }
    }
    if (rc != CT_OK) {
        return rc;
    }
    const bool simple = (h->scene.flags & CT_FLAG_SIMPLE_KERNEL) != 0;
    if (!simple && !h->order_tuned && !dense_frames) {   // (a dense frame -- ct_render_subframe -- measures nothing)
        return tune_order(h, S);
    }
    return CT_OK;
}

extern "C" int ct_render_subframe(CtHandle h, uint32_t subframe_id, float *frame_rgba_dev)
{
    NEED(h);
    if (!h->camera_set) {
        return fail(h, CT_E_STATE, "ct_set_camera has not been called");
    }
    const size_t bytes = (size_t)h->scene.width * h->scene.height * sizeof(float4);
    // own pixels start as a miss (0,0,0,1); pixels of other shards stay (0,0,0,0)
    HIPCHK(h, launch_fill_frame(h->d_frame, h->scene.width, h->scene.height, h->scene.shard_index,
                                h->scene.shard_count, h->stream));
    const int rc = run_batch(h, h->d_frame, subframe_id, 1, false);
    if (rc != CT_OK) {
        return rc;
    }
    if (frame_rgba_dev) {
        HIPCHK(h, hipMemcpyAsync(frame_rgba_dev, h->d_frame, bytes, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return CT_OK;
}

extern "C" int ct_accumulate(CtHandle h, uint32_t subframe_id, const float *frame_rgba_dev)
{
    NEED(h);
    if (subframe_id == 0) {
        return fail(h, CT_E_INVAL, "subframe ids are 1-based (Camera.cpp:191)");
    }
    const float4 *src = frame_rgba_dev ? (const float4 *)frame_rgba_dev : h->d_frame;
    HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    // (no alpha check here: the caller may accumulate frames of its own)
    HIPCHK(h, launch_accumulate_batch(src, h->d_mean, h->d_m2, subframe_id, 1, h->scene.width, h->scene.height,
                                      h->scene.shard_index, h->scene.shard_count, nullptr, h->stop_cadence ? h->d_freeze : nullptr,
                                      h->stream));
    if (h->stop_cadence && subframe_id % h->stop_cadence == 0u && subframe_id >= h->stop_min) {
        const int rc = enqueue_convergence_test(h, subframe_id);
        if (rc != CT_OK) {
            return rc;
        }
    }
    HIPCHK(h, hipEventRecord(h->ev[2], h->stream));
    HIPCHK(h, hipEventSynchronize(h->ev[2]));
    float ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[1], h->ev[2]));
    h->accum_ms += ms;
    h->subframes = subframe_id;
    discard_ahead(h);
    return CT_OK;
}

// Subframes of the launch that measures the job costs of a new pose.
// (16 since round 3 -- 32 before: a waited-for launch of 32 subframes lasted 48 ms, most of it the wait for its longest paths.
// The order 16 subframes yield is as good as that of 32 -- long launches 349 ms either way, 10-subframe display updates 4.49 vs
// 4.52 ms -- while 8 subframes cost the display cadence 2-3 %: 4.61 ms, 3.70 instead of 3.62 with render-ahead.)
constexpr uint32_t kTuneSubframes = 16;
// (Also tried in round 3: the cost-measuring launch ENQUEUED -- it ends when its job list is empty, its survivors go to the next
// launch booking what they have cost so far, times 1..4 -- 18 ms instead of 26-48.  The order made from paths cut short is worse:
// the launches that follow take 352-359 ms per 1024 subframes instead of 349 for as long as the pose lasts, and the first image of
// a pose needs its longest path either way.  Removed.)
static uint32_t tune_subframes(CtHandle h)
{
    return (uint32_t)knob_int(h->tune.TUNE_SUBFRAMES, 1, 1024, (int)kTuneSubframes);   // (A/B: how short may the cost-measuring launch be?)
}

static int render_accumulate_impl(CtHandle h, uint32_t first_subframe_id, uint32_t count, bool wait)
{
    if (!h->camera_set) {
        return fail(h, CT_E_STATE, "ct_set_camera has not been called");
    }
    if (first_subframe_id != h->subframes + 1) {
        return fail(h, CT_E_STATE, "first_subframe_id %u but %u subframes are accumulated", first_subframe_id,
                    h->subframes);
    }
    if (count == 0) {
        return wait ? flush(h) : CT_OK;
    }
    const bool simple = (h->scene.flags & CT_FLAG_SIMPLE_KERNEL) != 0;
    if (h->rendered > h->subframes) {
        // some of these subframes were rendered ahead of the calls: their samples wait in the scratch
        const uint32_t covered = std::min(count, h->rendered - h->subframes);
        h->subframes += covered;
        first_subframe_id += covered;
        count -= covered;
        if (count == 0) {
            const int rc = advance_accumulate(h, accumulate_target(h));
            return rc != CT_OK ? rc : (wait ? flush(h) : CT_OK);
        }
    }
    // (from here on every rendered subframe has been asked for)
    const uint32_t asked_end = h->subframes + count;
    if (!wait && h->ahead > count && !simple && h->continuation && h->order_tuned && !h->queue_dirty &&
        groups_per_chunk(h, h->ahead) >= h->n_groups) {
        count = h->ahead;   // the launch renders ahead of the calls; this call accumulates its own share
    }
    if (h->queue_dirty && !simple) {
        int rc = flush(h);
        if (rc == CT_OK) {
            rc = rebuild_queue(h);
        }
        if (rc != CT_OK) {
            return rc;
        }
    }
    // A call is cut by SUBFRAMES only where it must be (the subframe offset of a job has 16 bits); what does not fit the
    // scratch is cut by PIXEL GROUPS: every launch renders all the subframes of one chunk of groups (prepare_batches).
    const uint64_t cap = 0xffffull;
    uint32_t done = 0;
    // job lists are built for the size of the call's batches, not for the remainder that follows the short
    // cost-measuring launch (the next call of the same size would rebuild them)
    h->jobs_hint = (uint32_t)((count + (count + cap - 1) / cap - 1) / ((count + cap - 1) / cap));
    if (!simple) {
        // the scratch is sized for the call's batches now, not grown when the first of them follows the short cost-measuring
        // launch (freeing and allocating tens of GB takes hundreds of milliseconds)
        for (;;) {
            const uint32_t gc = groups_per_chunk(h, h->jobs_hint);
            // (reserved for a pose in which EVERY pixel of this shard hits the box, if a region holds that: the pixel list grows
            // and shrinks as the camera moves, and every growth of the scratch would be a hipFree + hipMalloc of tens of GB --
            // 25 ms when the driver has the pages at hand, a second when it has not)
            const uint64_t all_groups = (h->own_pixels + 63u) / 64u;
            const uint64_t region_groups = plan::region_groups(scratch_slot_bytes(h) / sizeof(float4), h->jobs_hint);
            const uint32_t gc_reserve = (gc >= h->n_groups && all_groups <= region_groups) ? (uint32_t)std::max<uint64_t>(all_groups, gc) : gc;
            const size_t need = (size_t)h->jobs_hint * gc_reserve * 64;
            const bool enqueue = !wait || gc < h->n_groups;
            const uint64_t budget = 2 * scratch_slot_bytes(h) / sizeof(float4);
            const size_t total = std::min<size_t>((size_t)(enqueue ? wanted_regions(h, need, std::max<uint64_t>(budget, 2 * need)) : 1) * need,
                                                  (0xffffffffull / std::max<size_t>(need, 1)) * need);
            if (total <= h->d_frames_all.capacity()) {
                break;
            }
            int rc = flush(h);
            if (rc == CT_OK) {
                rc = reserve_frames(h, total);
            }
            if (rc == CT_E_NOMEM && scratch_slot_bytes(h) > (64ull << 20)) {
                h->scratch_cap_bytes = scratch_slot_bytes(h) / 2;   // the device cannot give that much: smaller chunks
                continue;
            }
            if (rc != CT_OK) {
                return rc;
            }
            break;
        }
    }
    while (done < count) {
        const uint64_t left = count - done, parts = (left + cap - 1) / cap;
        uint32_t S = (uint32_t)((left + parts - 1) / parts);
        int rc;
        if (!simple && !h->order_tuned) {
            // the first launch of a pose measures the job costs (two atomics per path, jobs in image
            // order): it is kept short, waited for, then the order is set
            // (a call of a display update's size is the cost-measuring launch as a whole: 10 subframes waited for cost 27 ms, 8 of
            // them 26 and the other 2 a launch and a flush of their own)
            S = std::min(S, h->jobs_hint <= tune_subframes(h) + tune_subframes(h) / 2u ? std::max(h->jobs_hint, 1u) : tune_subframes(h));
            rc = run_batch(h, nullptr, first_subframe_id + done, S, true);
        } else {
            const bool trace = h->tune.TRACE.get() != nullptr;
            const auto t0 = std::chrono::steady_clock::now();
            rc = prepare_batches(h, S);
            // several chunks: they are enqueued like batches (paths pass from chunk to chunk) and a waited-for call waits at the end
            const bool enqueue = !wait || (h->n_chunks > 1 && h->continuation && !simple);
            // (laid out for the call's batch size, not for the remainder that follows the short cost-measuring launch: the next
            // call of the same size then finds its layout, and nothing has to be flushed for it)
            uint32_t layout = S;
            if (enqueue && h->n_chunks <= 1 && 2 * (uint64_t)std::max(S, h->jobs_hint) * frame_stride(h) <= 0xffffffffull) {
                layout = std::max(S, h->jobs_hint);   // (one chunk only: a chunk's size was chosen for S)
            }
            const size_t need = (size_t)layout * frame_stride(h);
            // (an enqueued batch may use the regions of a layout made for larger ones, as long as the ring is long enough for it)
            const bool ring_too_short = enqueue && (h->n_regions < 2 ||
                                                    (layout != h->layout_S && h->n_regions < wanted_regions(h, need, 2 * scratch_slot_bytes(h) / sizeof(float4))));
            if (rc == CT_OK && (need > h->slot_capacity || ring_too_short)) {
                rc = flush(h); // the layout of the scratch changes: nothing may be in flight
                if (rc == CT_OK) {
                    rc = ensure_frames(h, layout, enqueue);
                }
                if (rc == CT_E_NOMEM && scratch_slot_bytes(h) > (64ull << 20)) {
                    h->scratch_cap_bytes = scratch_slot_bytes(h) / 2;   // the device cannot give that much: smaller chunks
                    continue;
                }
            }
            const auto t1 = std::chrono::steady_clock::now();
            if (!enqueue) {
                rc = rc == CT_OK ? flush(h) : rc;
                h->next_slot = 0; // a synchronous batch uses one region and runs every path to its end
            }
            for (uint32_t c = 0; c < std::max(h->n_chunks, 1u) && rc == CT_OK; c++) {
                const int slot = h->next_slot;
                if (rc == CT_OK && h->slots[slot].awaits_accumulate) {
                    // the region's previous batch: with render-ahead its last share is due now at the latest
                    h->subframes = std::min(h->rendered + S, asked_end);
                    rc = advance_accumulate(h, accumulate_target(h));
                    h->subframes = std::min(h->rendered, asked_end);
                    if (rc == CT_OK && h->slots[slot].awaits_accumulate) {
                        rc = fail(h, CT_E_STATE, "internal: scratch region %d is reused before its batch is accumulated", slot);
                    }
                }
                rc = rc == CT_OK ? collect(h, h->slots[slot]) : rc; // book the launch that used this region n_regions launches ago
                const auto t2 = std::chrono::steady_clock::now();
                if (rc == CT_OK) {
                    const bool suspend = enqueue && h->continuation && !simple;
                    rc = submit_batch(h, slot, nullptr, first_subframe_id + done, S, true, suspend, c);
                }
                if (trace) {
                    const auto t3 = std::chrono::steady_clock::now();
                    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
                    fprintf(stderr, "[cloudtrace] batch first=%u S=%u chunk %u of %u, region %d of %d: prepare %.2f ms, slot %.2f ms, submit %.2f ms\n",
                            first_subframe_id + done, S, c, h->n_chunks, slot, h->n_regions, ms(t0, t1), ms(t1, t2), ms(t2, t3));
                }
                if (enqueue) {
                    h->next_slot = (h->next_slot + 1) % h->n_regions;
                } else if (rc == CT_OK) {
                    rc = collect(h, h->slots[slot]);
                }
            }
        }
        if (rc != CT_OK) {
            flush(h);
            return rc;
        }
        done += S;
        h->rendered += S;
        h->subframes = std::min(h->rendered, asked_end);
        if (h->ahead && rc == CT_OK) {
            rc = advance_accumulate(h, accumulate_target(h));   // (the launch was enqueued before the count moved)
            if (rc != CT_OK) {
                flush(h);
                return rc;
            }
        }
    }
    return wait ? flush(h) : CT_OK;
}

extern "C" int ct_render_accumulate(CtHandle h, uint32_t first_subframe_id, uint32_t count)
{
    NEED(h);
    return render_accumulate_impl(h, first_subframe_id, count, true);
}

extern "C" int ct_render_accumulate_async(CtHandle h, uint32_t first_subframe_id, uint32_t count)
{
    NEED_NOFLUSH(h);
    return render_accumulate_impl(h, first_subframe_id, count, false);
}

extern "C" int ct_set_render_ahead(CtHandle h, uint32_t subframes)
{
    NEED(h);
    if (subframes > 0xffffu) {
        return fail(h, CT_E_INVAL, "render-ahead of %u subframes (a launch holds at most 65535)", subframes);
    }
    discard_ahead(h);
    h->ahead = subframes;
    return CT_OK;
}

extern "C" int ct_set_stop_when_converged(CtHandle h, uint32_t cadence, uint32_t min_subframes)
{
    NEED(h);
    if (cadence != 0u && h->scene.shard_count > 1u) {
        return fail(h, CT_E_INVAL, "stop-when-converged is a whole-frame decision: this handle renders shard %u of %u "
                                   "(test the merged frame with ct_is_converged_buffers)", h->scene.shard_index, h->scene.shard_count);
    }
    h->stop_cadence = cadence;
    h->stop_min = min_subframes;
    HIPCHK(h, hipMemsetAsync(h->d_freeze, 0, 8 * sizeof(uint32_t), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    memset(h->freeze_host, 0, 4 * sizeof(uint32_t));
    return CT_OK;
}

extern "C" int ct_converged_at(CtHandle h, uint32_t *subframes_out, uint32_t *tested_at_out, uint64_t *unconverged_pixels_out)
{
    NEED_NOFLUSH(h);
    // (written by the copies that follow the tests in stream order; read without waiting)
    const volatile uint32_t *st = h->freeze_host;
    if (subframes_out) {
        *subframes_out = st[0];
    }
    if (tested_at_out) {
        *tested_at_out = st[1];
    }
    if (unconverged_pixels_out) {
        *unconverged_pixels_out = st[2];
    }
    return CT_OK;
}

extern "C" int ct_rendered_subframes(CtHandle h, uint32_t *count_out)
{
    NEED_NOFLUSH(h);
    if (count_out) {
        *count_out = std::max(h->rendered, h->subframes);
    }
    return CT_OK;
}

extern "C" int ct_synchronize(CtHandle h)
{
    NEED(h);
    const int rc = flush(h);
    if (rc != CT_OK) {
        return rc;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CT_OK;
}

static_assert(sizeof(CtPointRadianceTask) == 40, "Gpu::PointRadianceTask is 40 bytes (PointRadianceTask.h:70-77)");

// The launch half of ct_point_radiance_launch, which the traced bake (ct_bake.cpp) shares: `launches` experiments, frames
// first_frame_id .., of the `count` point tasks whose rays `rays` enqueues into h->pt.primary / h->pt.pixels (grown to
// pad64(count) entries by then).  The results are h->pt.frames[f * pad64(count) + i]; `fold` enqueues what consumes them.
// Waits for the stream, books the estimator's time and the paths.  sc: the scene the estimator runs with.
int ct::point_launch(CtHandle h, const DevScene &sc, uint32_t count, uint32_t first_frame_id, uint32_t launches,
                     const std::function<int()> &rays, const std::function<int()> &fold)
{
    const uint32_t n_pad = (count + 63u) & ~63u, n_groups = n_pad / 64u;
    // ---- job list.  A job = (group of 64 tasks, range of frames).  A collector's call is small -- 20480 tasks x 100
    // frames are 32000 wave-jobs of 64 experiments for the chip's 6144 resident waves -- and most of its work is in the few
    // tasks deep inside the cloud, whose every experiment runs to the depth cap (2000 bounces): jobs are single frames
    // unless the call is large, in one queue, frame-major, so that the deep groups are spread evenly over the list and over
    // the waves.  (What bounds such a call is the serial latency of those paths, ~6 us per bounce: DESIGN.md section 8 f-1.)
    // Several collectors at once (cloudtrace collect --jobs K: one handle and one host thread per scene setup) each launch a
    // persistent grid, and a grid that fills every CU leaves the others waiting for its last, longest paths.  A call that
    // finds others in flight launches a share of the grid instead -- blocks per CU divided by the calls in flight, at least
    // one -- so that the kernels are resident side by side: 8.72 -> 7.86 ms per update with four setups in flight, 7.76 with six
    // (profiles/r03y).  Alone, a call keeps the whole chip.  (The schedule only: results do not depend on the grid.)
    struct InFlight {
        std::atomic<int> &n;
        int mine;
        explicit InFlight(std::atomic<int> &c) : n(c), mine(c.fetch_add(1) + 1) {}
        ~InFlight() { n.fetch_sub(1); }
    };
    static std::atomic<int> point_calls_in_flight[64];   // (per device: cloudtrace collect --gpus deals the setups to several)
    const InFlight in_flight(point_calls_in_flight[(uint32_t)h->device & 63u]);
    LaunchShape shape = h->shape;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) == hipSuccess && cus > 0) {
            const int per_cu = std::max(1, shape.blocks / cus);
            const int share = std::max(1, per_cu / std::max(1, in_flight.mine));
            shape.blocks = knob_int(h->tune.POINT_BLOCKS_PER_CU, 1, per_cu, share) * cus;   // (CT_POINT_BLOCKS_PER_CU: A/B)
        }
    }
    const uint32_t waves = (uint32_t)shape.blocks * (uint32_t)shape.threads / 64u;
    const uint32_t chunk = h->point_order
                               ? (uint32_t)std::min<uint64_t>(8, std::max<uint64_t>(1, (uint64_t)n_groups * launches / (16ull * std::max(waves, 1u))))
                               : 8u;
    std::vector<uint32_t> jg, js;
    jg.reserve((size_t)n_groups * ((launches + chunk - 1) / chunk));
    js.reserve(jg.capacity());
    if (h->point_order) {
        for (uint32_t s0 = 0; s0 < launches; s0 += chunk) {
            for (uint32_t g = 0; g < n_groups; g++) {
                jg.push_back(g);
                js.push_back(s0 | (std::min(chunk, launches - s0) << 16));
            }
        }
    } else {
        for (uint32_t g = 0; g < n_groups; g++) {
            for (uint32_t s0 = 0; s0 < launches; s0 += chunk) {
                jg.push_back(g);
                js.push_back(s0 | (std::min(chunk, launches - s0) << 16));
            }
        }
    }
    CtHandle_::PointBuffers &pt = h->pt;
    auto run = [&]() -> int {
        HIPCHK(h, pt.primary.reserve(2 * (size_t)n_pad));
        HIPCHK(h, pt.pixels.reserve(n_pad));
        HIPCHK(h, pt.frames.reserve((size_t)n_pad * launches));
        HIPCHK(h, pt.jg.reserve(jg.size()));
        HIPCHK(h, pt.js.reserve(js.size()));
        HIPCHK(h, hipMemcpyAsync(pt.jg, jg.data(), jg.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(pt.js, js.data(), js.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemsetAsync(h->d_queue, 0, kQueueWords * sizeof(uint32_t), h->stream));
        int rc = rays();
        if (rc != CT_OK) {
            return rc;
        }
        BatchArgs ba{};
        ba.frames = pt.frames;
        ba.frame_stride = n_pad;
        ba.primary = pt.primary;
        ba.pixels = pt.pixels;
        ba.job_group = pt.jg;
        ba.job_sub = pt.js;
        ba.cost = nullptr;
        ba.n_jobs = (uint32_t)jg.size();
        if (h->point_order) {
            // one queue: the order above is the order the chip's waves take the jobs in
            ba.q_begin[0] = 0;
            for (int x = 1; x <= kQueues + 1; x++) {
                ba.q_begin[x] = ba.n_jobs;
            }
        } else {
            split_queues_evenly(ba);
        }
        ba.first_subframe = first_frame_id;
        ba.S = launches;
        ba.queue = h->d_queue;
        ba.counters = h->d_counters;
        ba.stats = h->d_counters + kCounterCount + 1;
        HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
        if (h->scene.estimator == CT_EST_DELTA) {
            HIPCHK(h, launch_render_delta(sc, ba, shape, h->stream));
        } else {
            HIPCHK(h, launch_render_persistent(sc, ba, shape, h->stream));
        }
        HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
        rc = fold();
        if (rc != CT_OK) {
            return rc;
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        float ms = 0;
        HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
        h->render_ms += ms;
        h->launches += 1;
        h->host_paths += (unsigned long long)count * launches;
        h->iv_expected_dealt += (unsigned long long)count * launches;
        if (pt.frames.capacity() > ((size_t)64 << 20)) {
            // an unusually large call (> 1 GiB of per-experiment results): do not keep that much for the handle's life
            HIPCHK(h, pt.frames.reset());
        }
        return CT_OK;
    };
    const int rc = run();
    if (rc != CT_OK) {
        hipStreamSynchronize(h->stream);
    }
    return rc;
}

extern "C" int ct_point_radiance_launch(CtHandle h, CtPointRadianceTask *tasks_host, uint32_t count,
                                        uint32_t first_frame_id, uint32_t launches)
{
    NEED(h);
    if (!tasks_host || count == 0 || launches == 0 || launches > 0xffffu || count > (1u << 24)) {
        return fail(h, CT_E_INVAL, "ct_point_radiance_launch: need 1..2^24 tasks and 1..65535 launches");
    }
    if (h->scene.flags & CT_FLAG_SIMPLE_KERNEL) {
        return fail(h, CT_E_INVAL, "point radiance tasks need the persistent kernel");
    }
    // A zero direction, or a direction or origin with a component that is not finite, has no ray, but can still "hit" the box
    // (fmaxf drops the NaN slabs; 0 / 0 needs only an origin inside): the path would then march with NaN coordinates, which
    // neither the estimators' brick addressing nor the DELTA estimator's cell walk is written for.  No ray of the reference is such.
    for (uint32_t i = 0; i < count; i++) {
        const float *d = tasks_host[i].direction, *o = tasks_host[i].position;
        if (!(std::isfinite(d[0]) && std::isfinite(d[1]) && std::isfinite(d[2])) || (d[0] == 0.f && d[1] == 0.f && d[2] == 0.f)) {
            return fail(h, CT_E_INVAL, "ct_point_radiance_launch: task %u has a zero or non-finite direction", i);
        }
        if (!(std::isfinite(o[0]) && std::isfinite(o[1]) && std::isfinite(o[2]))) {
            return fail(h, CT_E_INVAL, "ct_point_radiance_launch: task %u has a non-finite position", i);
        }
    }
    const uint32_t n_pad = (count + 63u) & ~63u;
    if ((uint64_t)n_pad * launches > 0xffffffffull) {
        return fail(h, CT_E_INVAL, "too many task-launches for one call");
    }
    CtHandle_::PointBuffers &pt = h->pt;
    return point_launch(
        h, h->dev, count, first_frame_id, launches,
        [&]() -> int {
            HIPCHK(h, pt.tasks.reserve(count));
            HIPCHK(h, hipMemcpyAsync(pt.tasks, tasks_host, (size_t)count * sizeof(CtPointRadianceTask), hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, launch_point_rays(h->dev, pt.tasks, count, n_pad, pt.primary, pt.pixels, h->stream));
            return CT_OK;
        },
        [&]() -> int {
            HIPCHK(h, launch_point_accumulate(pt.frames, n_pad, pt.tasks, count, launches, h->stream));
            HIPCHK(h, hipMemcpyAsync(tasks_host, pt.tasks, (size_t)count * sizeof(CtPointRadianceTask), hipMemcpyDeviceToHost, h->stream));
            return CT_OK;
        });
}

// ---- the radiance collector on the device (ct_collector_*): RadianceCollector's loop over point_launch -------------------
// Kernels: ct_collect.hip.  All device memory is allocated in ct_collector_create; an update reads back one word, the number of
// survivors, behind the wait point_launch makes anyway.
struct CtCollector_ {
    CtHandle h = nullptr;
    int device = 0;
    CtCollectorDesc d{};
    uint32_t batch = 0;
    uint32_t n_live = 0;      // tasks in live[cur]
    int cur = 0;
    uint32_t count = 0;       // experiments every live task holds
    uint32_t updates = 0, frame_id = 0;
    uint64_t paths = 0, epoch = 0;
    double trace_ms = 0, fold_ms = 0, test_ms = 0;
    DevBuf<float> positions, directions, mean, m2;
    DevBuf<uint32_t> counts, converged_update, live[2], waves;
    Event ev[5];              // around the rays kernel, the fold kernel, and behind the compaction
};

static_assert(sizeof(CtCollectorDesc) == 24 && sizeof(CtCollectorInfo) == 64, "include/cloudtrace.h states these sizes");

extern "C" int ct_collector_create(CtHandle h, const CtCollectorDesc *d, const float *positions_host, const float *directions_host,
                                   uint32_t count, CtCollector *out)
{
    if (!h) {
        return fail(nullptr, CT_E_INVAL, "null handle");
    }
    if (out) {
        *out = nullptr;
    }
    if (!d || !positions_host || !directions_host || !out) {
        return fail(h, CT_E_INVAL, "ct_collector_create: need a description, positions, directions and out");
    }
    if (d->abi_version != CT_ABI_VERSION) {
        return fail(h, CT_E_INVAL, "ct_collector_create: abi_version %u, this library is %u", d->abi_version, CT_ABI_VERSION);
    }
    if (d->max_thread_count == 0u || d->max_thread_count > (1u << 24)) {
        return fail(h, CT_E_INVAL, "ct_collector_create: max_thread_count %u, a collector has 1 .. 2^24 threads", d->max_thread_count);
    }
    if (d->launches_per_update == 0u || d->launches_per_update > 0xffffu) {
        return fail(h, CT_E_INVAL, "ct_collector_create: launches_per_update %u, an update traces 1 .. 65535 frames", d->launches_per_update);
    }
    if (!std::isfinite(d->rel_tol) || !std::isfinite(d->abs_tol) || d->rel_tol < 0.f || d->abs_tol < 0.f) {
        return fail(h, CT_E_INVAL, "ct_collector_create: rel_tol and abs_tol must be finite and not negative");
    }
    if (count == 0u || count > d->max_thread_count) {
        return fail(h, CT_E_INVAL, "ct_collector_create: %u tasks for %u threads; need 1 .. max_thread_count", count, d->max_thread_count);
    }
    if ((uint64_t)((d->max_thread_count + 63u) & ~63u) * d->launches_per_update > 0xffffffffull) {
        return fail(h, CT_E_INVAL, "ct_collector_create: too many task-launches for one update");
    }
    for (uint32_t i = 0; i < count; i++) {   // (ct_point_radiance_launch's test of its tasks)
        const float *dir = directions_host + 3 * (size_t)i, *o = positions_host + 3 * (size_t)i;
        if (!(std::isfinite(dir[0]) && std::isfinite(dir[1]) && std::isfinite(dir[2])) || (dir[0] == 0.f && dir[1] == 0.f && dir[2] == 0.f)) {
            return fail(h, CT_E_INVAL, "ct_collector_create: task %u has a zero or non-finite direction", i);
        }
        if (!(std::isfinite(o[0]) && std::isfinite(o[1]) && std::isfinite(o[2]))) {
            return fail(h, CT_E_INVAL, "ct_collector_create: task %u has a non-finite position", i);
        }
    }
    if (h->scene.flags & CT_FLAG_SIMPLE_KERNEL) {
        return fail(h, CT_E_INVAL, "ct_collector_create: point radiance tasks need the persistent kernel");
    }
    NEED(h);
    CtCollector_ *c = new CtCollector_();
    c->h = h;
    c->device = h->device;
    c->d = *d;
    c->batch = c->n_live = count;
    c->epoch = h->light_epoch;
    const size_t B = count;
    if (c->positions.alloc(3 * B) != hipSuccess || c->directions.alloc(3 * B) != hipSuccess || c->mean.alloc(B) != hipSuccess ||
        c->m2.alloc(B) != hipSuccess || c->counts.alloc(B) != hipSuccess || c->converged_update.alloc(B) != hipSuccess ||
        c->live[0].alloc(B) != hipSuccess || c->live[1].alloc(B) != hipSuccess || c->waves.alloc(B + 1u) != hipSuccess) {
        (void)hipGetLastError();
        delete c;
        return fail(h, CT_E_NOMEM, "ct_collector_create: no device memory for the state and live lists of %u tasks", count);
    }
    std::vector<uint32_t> ids(B);
    for (uint32_t i = 0; i < count; i++) {
        ids[i] = i;
    }
    auto fill = [&]() -> int {
        for (Event &e : c->ev) {
            HIPCHK(h, e.create());
        }
        HIPCHK(h, hipMemcpyAsync(c->positions, positions_host, 3 * B * sizeof(float), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(c->directions, directions_host, 3 * B * sizeof(float), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(c->live[0], ids.data(), B * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemsetAsync(c->mean, 0, B * sizeof(float), h->stream));
        HIPCHK(h, hipMemsetAsync(c->m2, 0, B * sizeof(float), h->stream));
        HIPCHK(h, hipMemsetAsync(c->counts, 0, B * sizeof(uint32_t), h->stream));
        HIPCHK(h, hipMemsetAsync(c->converged_update, 0, B * sizeof(uint32_t), h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return CT_OK;
    };
    const int rc = fill();
    if (rc != CT_OK) {
        hipStreamSynchronize(h->stream);
        delete c;
        return rc;
    }
    *out = c;
    return CT_OK;
}

extern "C" int ct_collector_update(CtHandle h, CtCollector c, uint32_t updates)
{
    if (!h) {
        return fail(nullptr, CT_E_INVAL, "null handle");
    }
    if (!c) {
        return fail(h, CT_E_INVAL, "ct_collector_update: null collector");
    }
    if (c->h != h) {
        return fail(h, CT_E_INVAL, "ct_collector_update: the collector belongs to another handle");
    }
    if (updates == 0u) {
        return fail(h, CT_E_INVAL, "ct_collector_update: need at least one update");
    }
    NEED(h);
    if (c->epoch != h->light_epoch) {
        return fail(h, CT_E_STATE, "ct_collector_update: the handle's light has changed since ct_collector_create");
    }
    c->trace_ms = c->fold_ms = c->test_ms = 0;
    CtHandle_::PointBuffers &pt = h->pt;
    const uint32_t L = c->d.launches_per_update;
    for (uint32_t k = 0; k < updates && c->n_live != 0u; k++) {
        const uint32_t n = c->n_live, r = c->d.max_thread_count / n, threads = n * r;
        if ((uint64_t)c->count + (uint64_t)r * L > 0xffffffffull) {
            return fail(h, CT_E_STATE, "ct_collector_update: update %u would carry the tasks' experiment count (%u) beyond 2^32 - 1", c->updates + 1u, c->count);
        }
        if ((uint64_t)c->frame_id + L > 0xffffffffull) {
            return fail(h, CT_E_STATE, "ct_collector_update: the frame ids of update %u would wrap", c->updates + 1u);
        }
        CollectArgs a{};
        a.live = c->live[c->cur];
        a.positions = c->positions;
        a.directions = c->directions;
        a.mean = c->mean;
        a.m2 = c->m2;
        a.counts = c->counts;
        a.converged_update = c->converged_update;
        a.n = n;
        a.r = r;
        a.n_pad = (threads + 63u) & ~63u;
        a.rel_tol = c->d.rel_tol;
        a.abs_tol = c->d.abs_tol;
        a.zero_samples = c->d.zero_samples;
        uint32_t survivors = 0;
        const double render_before = h->render_ms;
        const int rc = point_launch(
            h, h->dev, threads, c->frame_id + 1u, L,
            [&]() -> int {
                HIPCHK(h, hipEventRecord(c->ev[0], h->stream));
                HIPCHK(h, launch_collect_rays(h->dev, a, pt.primary, pt.pixels, h->stream));
                HIPCHK(h, hipEventRecord(c->ev[1], h->stream));
                return CT_OK;
            },
            [&]() -> int {
                HIPCHK(h, hipEventRecord(c->ev[2], h->stream));
                HIPCHK(h, launch_collect_fold(a, pt.frames, a.n_pad, L, c->count, c->updates + 1u, c->waves, h->stream));
                HIPCHK(h, hipEventRecord(c->ev[3], h->stream));
                HIPCHK(h, launch_collect_compact(a, c->waves, c->live[c->cur ^ 1], h->stream));
                HIPCHK(h, hipEventRecord(c->ev[4], h->stream));
                HIPCHK(h, hipMemcpyAsync(&survivors, c->waves + collect_groups(a), sizeof survivors, hipMemcpyDeviceToHost, h->stream));
                return CT_OK;
            });
        if (rc != CT_OK) {
            return rc;
        }
        float ms0 = 0, ms1 = 0, ms2 = 0;
        HIPCHK(h, hipEventElapsedTime(&ms0, c->ev[0], c->ev[1]));
        HIPCHK(h, hipEventElapsedTime(&ms1, c->ev[2], c->ev[3]));
        HIPCHK(h, hipEventElapsedTime(&ms2, c->ev[3], c->ev[4]));
        c->trace_ms += h->render_ms - render_before;
        c->fold_ms += (double)ms0 + (double)ms1;
        c->test_ms += (double)ms2;
        if (survivors > n) {
            return fail(h, CT_E_HIP, "internal: an update of %u live tasks counted %u survivors", n, survivors);
        }
        c->count += r * L;
        c->frame_id += L;
        c->updates += 1u;
        c->paths += (uint64_t)threads * L;
        c->cur ^= 1;
        c->n_live = survivors;
    }
    return CT_OK;
}

extern "C" int ct_collector_info(CtCollector c, CtCollectorInfo *out)
{
    if (!c || !out) {
        return fail(c ? c->h : nullptr, CT_E_INVAL, "ct_collector_info: need a collector and out");
    }
    *out = CtCollectorInfo{};
    out->batch = c->batch;
    out->remaining = c->n_live;
    out->converged = c->batch - c->n_live;
    out->updates = c->updates;
    out->frame_id = c->frame_id;
    out->repeat_count = c->n_live ? c->d.max_thread_count / c->n_live : 0u;
    out->threads = c->n_live * out->repeat_count;
    out->completed = c->n_live == 0u ? 1u : 0u;
    out->paths = c->paths;
    out->trace_ms = c->trace_ms;
    out->fold_ms = c->fold_ms;
    out->test_ms = c->test_ms;
    return CT_OK;
}

extern "C" int ct_collector_download(CtCollector c, CtPointRadianceTask *tasks_host_out, uint32_t *converged_update_host_out, uint32_t count)
{
    if (!c) {
        return fail(nullptr, CT_E_INVAL, "ct_collector_download: null collector");
    }
    CtHandle h = c->h;
    if (!tasks_host_out || count != c->batch) {
        return fail(h, CT_E_INVAL, "ct_collector_download: need an array of exactly %u tasks", c->batch);
    }
    NEED(h);
    const size_t B = c->batch;
    std::vector<float> pos(3 * B), dir(3 * B), mean(B), m2(B);
    std::vector<uint32_t> counts(B), conv(B);
    HIPCHK(h, hipMemcpy(pos.data(), c->positions, 3 * B * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(dir.data(), c->directions, 3 * B * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(mean.data(), c->mean, B * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(m2.data(), c->m2, B * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(counts.data(), c->counts, B * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(conv.data(), c->converged_update, B * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < B; i++) {
        CtPointRadianceTask &t = tasks_host_out[i];
        t.id = (int32_t)i;
        t.experimentCount = counts[i];
        t.radiance = mean[i];
        t.runningVariance = m2[i];
        for (int k = 0; k < 3; k++) {
            t.position[k] = pos[3 * i + k];
            t.direction[k] = dir[3 * i + k];
        }
        if (converged_update_host_out) {
            converged_update_host_out[i] = conv[i];
        }
    }
    return CT_OK;
}

extern "C" int ct_collector_destroy(CtCollector c)
{
    if (!c) {
        return CT_OK;
    }
    hipSetDevice(c->device);
    delete c;
    return CT_OK;
}

// ---- the adaptive frame (ct_adaptive_frame_*): the progressive image in rounds that go to the unconverged pixels only ----------
// Kernels: ct_adaptive.hip.  The scheme is bake_trace_adaptive's (ct_bake.cpp): a round's live list goes through point_launch in
// chunks of whole groups of 64 and passes, the fold of the round's last pass counts the survivors per wave, a scan and a ranked
// write compact them into the other list, and the host reads one word per round behind the wait point_launch makes anyway.
struct CtAdaptiveFrame_ {
    CtHandle h = nullptr;
    int device = 0;
    CtAdaptiveFrameDesc d{};
    uint32_t width = 0, height = 0, pixels = 0;
    uint32_t own = 0;         // the pixels the frame renders: all of them, or (ct_adaptive_frame_create_shard) the shard's own
    uint32_t n_live = 0;      // entries of the live list: live[cur], or every pixel of the frame while !listed
    uint32_t n_capped = 0;    // n_live == 0: the entries of live[cur] that failed the rule at the cap
    bool listed = false;
    int cur = 0;
    uint32_t count = 0;       // samples every live (or capped) pixel holds
    uint32_t cap = 0, rounds = 0;
    uint64_t paths = 0, epoch = 0;
    float pose[12] = {};
    double trace_ms = 0, fold_ms = 0, test_ms = 0;
    DevBuf<float4> mean, m2;
    DevBuf<uint32_t> counts, live[2], waves;
    Event ev[6];              // around the rays kernel, the fold kernel and the compaction
};

static_assert(sizeof(CtAdaptiveFrameDesc) == 32 && sizeof(CtAdaptiveFrameInfo) == 96, "include/cloudtrace.h states these sizes");

// The twelve floats ct_set_camera sets.
static void adaptive_pose(const DevScene &d, float out[12])
{
    const float v[12] = { d.ex, d.ey, d.ez, d.ux, d.uy, d.uz, d.vx, d.vy, d.vz, d.wx, d.wy, d.wz };
    memcpy(out, v, sizeof v);
}

// Is the frame still the image of the handle's pose and light?  (update and raise_cap; sets the handle's error)
static int adaptive_current(CtAdaptiveFrame f, const char *who)
{
    CtHandle h = f->h;
    if (f->epoch != h->light_epoch) {
        return fail(h, CT_E_STATE, "%s: the handle's light has changed since ct_adaptive_frame_create", who);
    }
    float pose[12];
    adaptive_pose(h->dev, pose);
    if (memcmp(pose, f->pose, sizeof pose) != 0) {
        return fail(h, CT_E_STATE, "%s: the handle's camera pose has changed since ct_adaptive_frame_create", who);
    }
    return CT_OK;
}

// ct_group_adaptive_frame_create (ct_group.hip): were two shards' frames created for the same camera pose and light?  Shards
// of one image must be; a caller that moved one handle of a group on its own is told so.
namespace ct {
bool adaptive_same_view(CtAdaptiveFrame a, CtAdaptiveFrame b)
{
    const CtScene &sa = a->h->scene, &sb = b->h->scene;
    return memcmp(a->pose, b->pose, sizeof a->pose) == 0 && memcmp(sa.light_direction, sb.light_direction, sizeof sa.light_direction) == 0 &&
           memcmp(sa.light_color, sb.light_color, sizeof sa.light_color) == 0 && sa.light_intensity == sb.light_intensity;
}
} // namespace ct

// ct_adaptive_frame_create (shard == false: a whole frame, a shard of a multi-GPU job is refused) and
// ct_adaptive_frame_create_shard (shard == true: the handle's own pixels, any shard_count).
static int adaptive_create(CtHandle h, const CtAdaptiveFrameDesc *d, CtAdaptiveFrame *out, const char *who, bool shard)
{
    if (!h) {
        return fail(nullptr, CT_E_INVAL, "null handle");
    }
    if (out) {
        *out = nullptr;
    }
    if (!d || !out) {
        return fail(h, CT_E_INVAL, "%s: need a description and out", who);
    }
    if (d->abi_version != CT_ABI_VERSION) {
        return fail(h, CT_E_INVAL, "%s: abi_version %u, this library is %u", who, d->abi_version, CT_ABI_VERSION);
    }
    const uint32_t R = d->round_samples;
    if (R == 0u || R > 0xffffu) {
        return fail(h, CT_E_INVAL, "%s: round_samples %u, a round traces 1 .. 65535 subframes per pixel", who, R);
    }
    if (d->max_samples == 0u || d->max_samples % R != 0u || d->max_samples > (1u << 24)) {
        return fail(h, CT_E_INVAL, "%s: max_samples %u; a multiple of round_samples (%u), at most 2^24", who, d->max_samples, R);
    }
    if (d->min_samples == 0u || d->min_samples % R != 0u || d->min_samples > d->max_samples) {
        return fail(h, CT_E_INVAL, "%s: min_samples %u; a multiple of round_samples (%u), at most max_samples (%u)", who, d->min_samples, R,
                    d->max_samples);
    }
    if (!std::isfinite(d->rel_tol) || !std::isfinite(d->abs_tol) || d->rel_tol < 0.f || d->abs_tol < 0.f) {
        return fail(h, CT_E_INVAL, "%s: rel_tol and abs_tol must be finite and not negative", who);
    }
    if (d->chunk_pixels % 64u != 0u) {
        return fail(h, CT_E_INVAL, "%s: chunk_pixels %u; 0 or a multiple of 64", who, d->chunk_pixels);
    }
    if (d->pass_subframes > R) {
        return fail(h, CT_E_INVAL, "%s: pass_subframes %u; 0 or 1 .. round_samples (%u)", who, d->pass_subframes, R);
    }
    if (h->scene.flags & CT_FLAG_SIMPLE_KERNEL) {
        return fail(h, CT_E_INVAL, "%s: an adaptive frame needs the persistent kernel", who);
    }
    if (!shard && h->scene.shard_count > 1u) {
        return fail(h, CT_E_INVAL, "%s: this handle renders shard %u of %u; an adaptive frame is a whole frame", who, h->scene.shard_index,
                    h->scene.shard_count);
    }
    NEED(h);
    const bool listed = h->scene.shard_count > 1u;   // (one shard of one: the whole frame, ct_adaptive_frame_create's object)
    CtAdaptiveFrame_ *f = new CtAdaptiveFrame_();
    f->h = h;
    f->device = h->device;
    f->d = *d;
    f->width = h->scene.width;
    f->height = h->scene.height;
    f->pixels = f->own = f->n_live = f->width * f->height;   // (at most 12288 x 4096: ct_create)
    f->cap = d->max_samples;
    f->epoch = h->light_epoch;
    adaptive_pose(h->dev, f->pose);
    const size_t P = f->pixels;
    auto no_memory = [&]() {
        (void)hipGetLastError();
        delete f;
        return fail(h, CT_E_NOMEM, "%s: no device memory for the state and live lists of %zu pixels", who, P);
    };
    if (f->mean.alloc(P) != hipSuccess || f->m2.alloc(P) != hipSuccess || f->counts.alloc(P) != hipSuccess ||
        (!listed && (f->live[0].alloc(P) != hipSuccess || f->live[1].alloc(P) != hipSuccess)) ||
        f->waves.alloc((P + 63u) / 64u + 1u) != hipSuccess) {
        return no_memory();
    }
    const AdaptiveShard own{ f->width, f->pixels, h->scene.shard_index, h->scene.shard_count };
    uint32_t n_own = 0;
    auto fill = [&]() -> int {
        for (Event &e : f->ev) {
            HIPCHK(h, e.create());
        }
        HIPCHK(h, hipMemsetAsync(f->mean, 0, P * sizeof(float4), h->stream));
        HIPCHK(h, hipMemsetAsync(f->m2, 0, P * sizeof(float4), h->stream));
        HIPCHK(h, hipMemsetAsync(f->counts, 0, P * sizeof(uint32_t), h->stream));
        if (listed) {   // the wave counts of the tile rule and their scan; the total sizes the two lists
            HIPCHK(h, launch_adaptive_own_count(own, f->waves, h->stream));
            HIPCHK(h, hipMemcpyAsync(&n_own, f->waves + (P + 63u) / 64u, sizeof n_own, hipMemcpyDeviceToHost, h->stream));
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return CT_OK;
    };
    int rc = fill();
    if (rc == CT_OK && listed) {
        if (n_own > P) {
            rc = fail(h, CT_E_HIP, "internal: %u of %zu pixels counted as the shard's own", n_own, P);
        } else if (n_own != 0u && (f->live[0].alloc(n_own) != hipSuccess || f->live[1].alloc(n_own) != hipSuccess)) {
            return no_memory();
        } else {
            f->own = f->n_live = n_own;
            f->listed = true;
            auto list = [&]() -> int {
                if (n_own != 0u) {
                    HIPCHK(h, launch_adaptive_own_list(own, f->waves, f->live[0], h->stream));
                    HIPCHK(h, hipStreamSynchronize(h->stream));
                }
                return CT_OK;
            };
            rc = list();
        }
    }
    if (rc != CT_OK) {
        hipStreamSynchronize(h->stream);
        delete f;
        return rc;
    }
    *out = f;
    return CT_OK;
}

extern "C" int ct_adaptive_frame_create(CtHandle h, const CtAdaptiveFrameDesc *d, CtAdaptiveFrame *out)
{
    return adaptive_create(h, d, out, "ct_adaptive_frame_create", false);
}

extern "C" int ct_adaptive_frame_create_shard(CtHandle h, const CtAdaptiveFrameDesc *d, CtAdaptiveFrame *out)
{
    return adaptive_create(h, d, out, "ct_adaptive_frame_create_shard", true);
}

extern "C" int ct_adaptive_frame_update(CtAdaptiveFrame f, uint32_t rounds)
{
    const char *const who = "ct_adaptive_frame_update";
    if (!f) {
        return fail(nullptr, CT_E_INVAL, "%s: null frame", who);
    }
    CtHandle h = f->h;
    NEED(h);
    const int current = adaptive_current(f, who);
    if (current != CT_OK) {
        return current;
    }
    f->trace_ms = f->fold_ms = f->test_ms = 0;
    CtHandle_::PointBuffers &pt = h->pt;
    const uint32_t R = f->d.round_samples;
    const double render_before = h->render_ms;
    for (uint32_t k = 0; (rounds == 0u || k < rounds) && f->n_live != 0u; k++) {
        const uint32_t c = f->count, L = f->n_live;
        uint32_t chunk = std::min(L, f->d.chunk_pixels ? f->d.chunk_pixels : 1u << 20);
        if (chunk >= 64u) {
            chunk &= ~63u;   // (whole groups of 64: a chunk's waves are the live list's)
        }
        const uint32_t *live_in = f->listed ? (const uint32_t *)f->live[f->cur] : nullptr;
        uint32_t *live_out = f->live[f->listed ? f->cur ^ 1 : 0];
        uint32_t survivors = 0;
        AdaptiveArgs a{};
        a.live = live_in;
        a.mean = f->mean;
        a.m2 = f->m2;
        a.counts = f->counts;
        a.rel_tol = f->d.rel_tol;
        a.abs_tol = f->d.abs_tol;
        a.min_samples = f->d.min_samples;
        for (uint32_t first = 0; first < L; first += chunk) {
            a.first = first;
            a.n = std::min(chunk, L - first);
            a.n_pad = (a.n + 63u) & ~63u;
            // at most 2^24 results per launch: 256 MiB of pt.frames, which point_launch keeps from call to call
            const uint32_t fit = std::max(1u, (1u << 24) / a.n_pad);
            const uint32_t per_pass = std::min(f->d.pass_subframes ? f->d.pass_subframes : R, std::min(fit, 0xffffu));
            for (uint32_t at = 0; at < R; at += per_pass) {
                const uint32_t passes = std::min(per_pass, R - at), done = c + at;
                const bool last_pass = at + passes == R, last = last_pass && first + a.n == L;
                AdaptiveArgs whole = a;   // the compaction's view: the whole list
                whole.first = 0;
                whole.n = L;
                whole.n_pad = (L + 63u) & ~63u;
                const int rc = point_launch(
                    h, h->dev, a.n, done + 1u, passes,
                    [&]() -> int {
                        HIPCHK(h, hipEventRecord(f->ev[0], h->stream));
                        HIPCHK(h, launch_adaptive_rays(h->dev, a, pt.primary, pt.pixels, h->stream));
                        HIPCHK(h, hipEventRecord(f->ev[1], h->stream));
                        return CT_OK;
                    },
                    [&]() -> int {
                        HIPCHK(h, hipEventRecord(f->ev[2], h->stream));
                        HIPCHK(h, launch_adaptive_fold(a, pt.frames, a.n_pad, passes, done, last_pass ? (uint32_t *)f->waves : nullptr, h->stream));
                        HIPCHK(h, hipEventRecord(f->ev[3], h->stream));
                        if (last) {
                            HIPCHK(h, hipEventRecord(f->ev[4], h->stream));
                            HIPCHK(h, launch_adaptive_compact(whole, f->waves, live_out, h->stream));
                            HIPCHK(h, hipEventRecord(f->ev[5], h->stream));
                            HIPCHK(h, hipMemcpyAsync(&survivors, f->waves + (L + 63u) / 64u, sizeof survivors, hipMemcpyDeviceToHost, h->stream));
                        }
                        return CT_OK;
                    });
                if (rc != CT_OK) {
                    return rc;
                }
                float ms0 = 0, ms1 = 0, ms2 = 0;
                HIPCHK(h, hipEventElapsedTime(&ms0, f->ev[0], f->ev[1]));
                HIPCHK(h, hipEventElapsedTime(&ms1, f->ev[2], f->ev[3]));
                if (last) {
                    HIPCHK(h, hipEventElapsedTime(&ms2, f->ev[4], f->ev[5]));
                }
                f->fold_ms += (double)ms0 + (double)ms1;
                f->test_ms += (double)ms2;
                f->trace_ms = h->render_ms - render_before;
            }
        }
        if (survivors > L) {
            return fail(h, CT_E_HIP, "internal: a round of %u live pixels counted %u survivors", L, survivors);
        }
        f->count = c + R;
        f->rounds += 1u;
        f->paths += (uint64_t)L * R;
        f->cur = f->listed ? f->cur ^ 1 : 0;
        f->listed = true;
        if (f->count >= f->cap) {   // the survivors fail the rule at the cap: kept for ct_adaptive_frame_raise_cap
            f->n_capped = survivors;
            f->n_live = 0;
        } else {
            f->n_live = survivors;
        }
    }
    return CT_OK;
}

extern "C" int ct_adaptive_frame_raise_cap(CtAdaptiveFrame f, uint32_t max_samples)
{
    const char *const who = "ct_adaptive_frame_raise_cap";
    if (!f) {
        return fail(nullptr, CT_E_INVAL, "%s: null frame", who);
    }
    CtHandle h = f->h;
    if (max_samples <= f->cap || max_samples % f->d.round_samples != 0u || max_samples > (1u << 24)) {
        return fail(h, CT_E_INVAL, "%s: max_samples %u; a multiple of round_samples (%u) above the cap (%u), at most 2^24", who, max_samples,
                    f->d.round_samples, f->cap);
    }
    NEED(h);
    const int current = adaptive_current(f, who);
    if (current != CT_OK) {
        return current;
    }
    f->cap = max_samples;
    if (f->n_capped != 0u) {   // (they all hold the old cap's count, as f->count says)
        f->n_live = f->n_capped;
        f->n_capped = 0;
    }
    return CT_OK;
}

extern "C" int ct_adaptive_frame_info(CtAdaptiveFrame f, CtAdaptiveFrameInfo *out)
{
    if (!f || !out) {
        return fail(f ? f->h : nullptr, CT_E_INVAL, "ct_adaptive_frame_info: need a frame and out");
    }
    *out = CtAdaptiveFrameInfo{};
    out->width = f->width;
    out->height = f->height;
    out->round_samples = f->d.round_samples;
    out->min_samples = f->d.min_samples;
    out->max_samples = f->cap;
    out->rounds = f->rounds;
    out->rel_tol = f->d.rel_tol;
    out->abs_tol = f->d.abs_tol;
    out->pixels = f->own;
    out->live = f->n_live;
    out->capped = f->n_capped;
    out->converged = (uint64_t)f->own - f->n_live - f->n_capped;
    out->paths = f->paths;
    out->trace_ms = f->trace_ms;
    out->fold_ms = f->fold_ms;
    out->test_ms = f->test_ms;
    return CT_OK;
}

// The device array `which` names and its size; nullptr: no such array.
static void *adaptive_array(CtAdaptiveFrame f, uint32_t which, size_t &bytes)
{
    switch (which) {
    case CT_ADAPTIVE_MEAN:
        bytes = (size_t)f->pixels * sizeof(float4);
        return (float4 *)f->mean;
    case CT_ADAPTIVE_M2:
        bytes = (size_t)f->pixels * sizeof(float4);
        return (float4 *)f->m2;
    case CT_ADAPTIVE_COUNTS:
        bytes = (size_t)f->pixels * sizeof(uint32_t);
        return (uint32_t *)f->counts;
    default:
        bytes = 0;
        return nullptr;
    }
}

extern "C" int ct_adaptive_frame_download(CtAdaptiveFrame f, uint32_t which, void *host, size_t bytes)
{
    const char *const who = "ct_adaptive_frame_download";
    if (!f) {
        return fail(nullptr, CT_E_INVAL, "%s: null frame", who);
    }
    CtHandle h = f->h;
    size_t need = 0;
    void *src = adaptive_array(f, which, need);
    if (!src) {
        return fail(h, CT_E_INVAL, "%s: which = %u; CT_ADAPTIVE_MEAN, CT_ADAPTIVE_M2 or CT_ADAPTIVE_COUNTS", who, which);
    }
    if (!host || bytes != need) {
        return fail(h, CT_E_INVAL, "%s: need a host array of exactly %zu bytes", who, need);
    }
    NEED(h);
    HIPCHK(h, hipMemcpy(host, src, need, hipMemcpyDeviceToHost));
    return CT_OK;
}

extern "C" int ct_adaptive_frame_device_ptr(CtAdaptiveFrame f, uint32_t which, void **out)
{
    const char *const who = "ct_adaptive_frame_device_ptr";
    if (!f) {
        return fail(nullptr, CT_E_INVAL, "%s: null frame", who);
    }
    size_t bytes = 0;
    void *p = adaptive_array(f, which, bytes);
    if (!p || !out) {
        return fail(f->h, CT_E_INVAL, "%s: need CT_ADAPTIVE_MEAN, CT_ADAPTIVE_M2 or CT_ADAPTIVE_COUNTS and out", who);
    }
    *out = p;
    return CT_OK;
}

extern "C" int ct_adaptive_frame_destroy(CtAdaptiveFrame f)
{
    if (!f) {
        return CT_OK;
    }
    hipSetDevice(f->device);
    delete f;
    return CT_OK;
}

extern "C" int ct_generate_scatter_samples(CtHandle h, uint32_t count, uint32_t batch_seed,
                                           float *positions_host_out, float *directions_host_out)
{
    NEED(h);
    if (!positions_host_out || !directions_host_out || count == 0 || count > (1u << 20)) {
        return fail(h, CT_E_INVAL, "ct_generate_scatter_samples: need 1..2^20 samples and two output arrays");
    }
    DevBuf<float> d_pos, d_dir;
    auto run = [&]() -> int {
        HIPCHK(h, d_pos.alloc(3 * (size_t)count));
        HIPCHK(h, d_dir.alloc(3 * (size_t)count));
        HIPCHK(h, launch_scatter_samples(h->dev, count, batch_seed, d_pos, d_dir, h->stream));
        HIPCHK(h, hipMemcpyAsync(positions_host_out, d_pos, 3 * (size_t)count * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(directions_host_out, d_dir, 3 * (size_t)count * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return CT_OK;
    };
    const int rc = run();
    if (rc != CT_OK) {
        hipStreamSynchronize(h->stream);
    }
    return rc;
}

extern "C" int ct_reset(CtHandle h)
{
    NEED(h);
    const size_t pixels = (size_t)h->scene.width * h->scene.height;
    HIPCHK(h, hipMemsetAsync(h->d_frame, 0, pixels * sizeof(float4), h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_mean, 0, pixels * sizeof(float4), h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_m2, 0, pixels * sizeof(float4), h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_counters, 0, (kCounterCount + 1 + kStatCount) * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_freeze, 0, 8 * sizeof(uint32_t), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    memset(h->freeze_host, 0, 4 * sizeof(uint32_t));
    h->subframes = 0;
    discard_ahead(h);
    h->render_ms = h->accum_ms = 0;
    h->launches = 0;
    h->host_paths = h->host_hits = 0;
    h->host_lookups = h->host_settled = 0;
    h->iv_expected_dealt = 0;
    return CT_OK;
}

static int tonemap_impl(CtHandle h, const float4 *mean, float exposure, uint8_t *rgba_host, float *avg_luminance_out)
{
    HIPCHK(h, launch_reinhard(mean, h->scene.width, h->scene.height, exposure, h->d_colsum, h->d_avg,
                              h->d_screen, &h->reinhard_generation, h->device, h->stream));
    if (rgba_host) {
        HIPCHK(h, hipMemcpyAsync(rgba_host, h->d_screen, (size_t)h->scene.width * h->scene.height * sizeof(uchar4),
                                 hipMemcpyDeviceToHost, h->stream));
    }
    if (avg_luminance_out) {
        HIPCHK(h, hipMemcpyAsync(avg_luminance_out, h->d_avg, sizeof(float), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CT_OK;
}

extern "C" int ct_tonemap(CtHandle h, float exposure, uint8_t *rgba_host, float *avg_luminance_out)
{
    NEED(h);
    return tonemap_impl(h, h->d_mean, exposure, rgba_host, avg_luminance_out);
}

extern "C" int ct_tonemap_async(CtHandle h, float exposure)
{
    NEED_NOFLUSH(h);
    // (behind whatever is enqueued: the running mean of the batches whose accumulate kernels precede it on the stream)
    HIPCHK(h, launch_reinhard(h->d_mean, h->scene.width, h->scene.height, exposure, h->d_colsum, h->d_avg, h->d_screen, &h->reinhard_generation,
                              h->device, h->stream));
    return CT_OK;
}

extern "C" int ct_tonemap_buffer(CtHandle h, const float *mean_rgba_dev, float exposure, uint8_t *rgba_host,
                                 float *avg_luminance_out)
{
    NEED(h);
    if (!mean_rgba_dev) {
        return fail(h, CT_E_INVAL, "mean_rgba_dev is NULL");
    }
    return tonemap_impl(h, (const float4 *)mean_rgba_dev, exposure, rgba_host, avg_luminance_out);
}

static int converged_impl(CtHandle h, const float4 *mean, const float4 *m2, uint32_t subframes, int32_t *converged_out,
                          uint64_t *unconverged_pixels_out)
{
    if (!converged_out) {
        return fail(h, CT_E_INVAL, "converged_out is NULL");
    }
    const uint64_t pixels = (uint64_t)h->scene.width * h->scene.height;
    if (subframes < 100) { // Camera.cpp:234-237
        *converged_out = 0;
        if (unconverged_pixels_out) {
            *unconverged_pixels_out = pixels;
        }
        return CT_OK;
    }
    unsigned long long *d_cnt = h->d_counters + kCounterCount;
    HIPCHK(h, hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long), h->stream));
    HIPCHK(h, launch_converged(mean, m2, subframes, pixels, d_cnt, h->stream));
    unsigned long long bad = 0;
    HIPCHK(h, hipMemcpyAsync(&bad, d_cnt, sizeof bad, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *converged_out = bad < 500 ? 1 : 0; // Camera.cpp:267
    if (unconverged_pixels_out) {
        *unconverged_pixels_out = bad;
    }
    return CT_OK;
}

extern "C" int ct_is_converged(CtHandle h, int32_t *converged_out, uint64_t *unconverged_pixels_out)
{
    NEED(h);
    // (a running mean that stop-when-converged froze is the image after that many subframes, whatever was asked for since)
    const uint32_t frozen_at = h->stop_cadence ? h->freeze_host[0] : 0u;
    return converged_impl(h, h->d_mean, h->d_m2, frozen_at ? frozen_at : h->subframes, converged_out, unconverged_pixels_out);
}

extern "C" int ct_is_converged_buffers(CtHandle h, const float *mean_rgba_dev, const float *m2_rgba_dev, uint32_t subframes,
                                       int32_t *converged_out, uint64_t *unconverged_pixels_out)
{
    NEED(h);
    if (!mean_rgba_dev || !m2_rgba_dev) {
        return fail(h, CT_E_INVAL, "mean_rgba_dev / m2_rgba_dev is NULL");
    }
    return converged_impl(h, (const float4 *)mean_rgba_dev, (const float4 *)m2_rgba_dev, subframes, converged_out,
                          unconverged_pixels_out);
}

static int buffer_info(CtHandle h, int32_t which, void **ptr, size_t *bytes)
{
    const size_t pixels = (size_t)h->scene.width * h->scene.height;
    switch (which) {
    case CT_BUF_MEAN: *ptr = h->d_mean; *bytes = pixels * sizeof(float4); return CT_OK;
    case CT_BUF_M2: *ptr = h->d_m2; *bytes = pixels * sizeof(float4); return CT_OK;
    case CT_BUF_FRAME: *ptr = h->d_frame; *bytes = pixels * sizeof(float4); return CT_OK;
    case CT_BUF_SCREEN: *ptr = h->d_screen; *bytes = pixels * sizeof(uchar4); return CT_OK;
    case CT_BUF_INSCATTER: *ptr = h->d_inscatter; *bytes = h->volume_bytes; return CT_OK;
    case CT_BUF_DENSITY: *ptr = h->d_density; *bytes = h->volume_bytes; return CT_OK;
    default: return fail(h, CT_E_INVAL, "unknown buffer %d", which);
    }
}

extern "C" int ct_buffer_bytes(CtHandle h, int32_t which, size_t *bytes_out)
{
    NEED(h);
    void *p;
    size_t b = 0;
    const int rc = buffer_info(h, which, &p, &b);
    if (rc == CT_OK && bytes_out) {
        *bytes_out = b;
    }
    return rc;
}

extern "C" int ct_download(CtHandle h, int32_t which, void *dst_host, size_t dst_bytes)
{
    NEED(h);
    void *p;
    size_t b = 0;
    const int rc = buffer_info(h, which, &p, &b);
    if (rc != CT_OK) {
        return rc;
    }
    if (!dst_host || dst_bytes != b) {
        return fail(h, CT_E_INVAL, "ct_download: need %zu bytes, got %zu", b, dst_bytes);
    }
    HIPCHK(h, hipMemcpyAsync(dst_host, p, b, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CT_OK;
}

// The image changes under the convergence rule's feet (ct_upload, ct_set_subframes: a checkpoint is loaded): whatever
// ct_set_stop_when_converged had frozen was the OLD image -- left in place, the flag would make every later accumulate
// kernel return early and the new image's samples would be dropped without a word.  As in ct_reset.
static int clear_freeze(CtHandle h)
{
    HIPCHK(h, hipMemsetAsync(h->d_freeze, 0, 8 * sizeof(uint32_t), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    memset(h->freeze_host, 0, 4 * sizeof(uint32_t));
    return CT_OK;
}

extern "C" int ct_upload(CtHandle h, int32_t which, const void *src_host, size_t src_bytes)
{
    NEED(h);
    if (which != CT_BUF_MEAN && which != CT_BUF_M2) {
        return fail(h, CT_E_INVAL, "ct_upload: only the running mean and M2 can be set (buffer %d)", which);
    }
    void *p;
    size_t b = 0;
    const int rc = buffer_info(h, which, &p, &b);
    if (rc != CT_OK) {
        return rc;
    }
    if (!src_host || src_bytes != b) {
        return fail(h, CT_E_INVAL, "ct_upload: need %zu bytes, got %zu", b, src_bytes);
    }
    discard_ahead(h);   // (what was rendered ahead belongs to the image that is being replaced)
    HIPCHK(h, hipMemcpyAsync(p, src_host, b, hipMemcpyHostToDevice, h->stream));
    return clear_freeze(h);
}

extern "C" int ct_copy_to_device(CtHandle h, int32_t which, void *dst_dev, size_t dst_bytes)
{
    NEED(h);
    void *p;
    size_t b = 0;
    const int rc = buffer_info(h, which, &p, &b);
    if (rc != CT_OK) {
        return rc;
    }
    if (!dst_dev || dst_bytes != b) {
        return fail(h, CT_E_INVAL, "ct_copy_to_device: need %zu bytes, got %zu", b, dst_bytes);
    }
    HIPCHK(h, hipMemcpyAsync(dst_dev, p, b, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CT_OK;
}

extern "C" int ct_copy_to_device_async(CtHandle h, int32_t which, void *dst_dev, size_t dst_bytes)
{
    NEED_NOFLUSH(h);
    void *p;
    size_t b = 0;
    const int rc = buffer_info(h, which, &p, &b);
    if (rc != CT_OK) {
        return rc;
    }
    if (!dst_dev || dst_bytes != b) {
        return fail(h, CT_E_INVAL, "ct_copy_to_device_async: need %zu bytes, got %zu", b, dst_bytes);
    }
    HIPCHK(h, hipMemcpyAsync(dst_dev, p, b, hipMemcpyDeviceToDevice, h->stream));
    return CT_OK;
}

extern "C" int ct_device_ptr(CtHandle h, int32_t which, void **ptr_out)
{
    NEED(h);
    size_t b = 0;
    if (!ptr_out) {
        return fail(h, CT_E_INVAL, "ptr_out is NULL");
    }
    return buffer_info(h, which, ptr_out, &b);
}

extern "C" int ct_subframes(CtHandle h, uint32_t *count_out)
{
    NEED_NOFLUSH(h); // host-side count of the subframes submitted so far
    if (count_out) {
        *count_out = h->subframes;
    }
    return CT_OK;
}

extern "C" int ct_set_subframes(CtHandle h, uint32_t count)
{
    NEED(h);
    h->subframes = count;
    discard_ahead(h);
    return clear_freeze(h);
}

extern "C" int ct_counters(CtHandle h, CtCounters *out)
{
    NEED(h);
    if (!out) {
        return fail(h, CT_E_INVAL, "out is NULL");
    }
    unsigned long long c[kCounterCount];
    HIPCHK(h, hipMemcpyAsync(c, h->d_counters, sizeof c, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    out->paths = c[0] + h->host_paths;
    out->box_hits = c[1] + h->host_hits;
    out->density_lookups = c[2] + h->host_lookups;
    out->inscatter_lookups = c[3];
    out->scatter_events = c[4];
    out->depth_capped = c[5];
    return CT_OK;
}

extern "C" int ct_fetch_counters(CtHandle h, CtFetchCounters *out)
{
    NEED(h);
    if (!out) {
        return fail(h, CT_E_INVAL, "out is NULL");
    }
    unsigned long long c[kCounterCount];
    HIPCHK(h, hipMemcpyAsync(c, h->d_counters, sizeof c, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    out->density_fetches = c[6];
    out->inscatter_fetches = c[7];
    return CT_OK;
}

extern "C" int ct_debug_invariants(CtHandle h, uint64_t out[8])
{
    NEED(h);
    if (!out) {
        return fail(h, CT_E_INVAL, "out is NULL");
    }
    unsigned long long iv[4] = { 0, 0, 0, 0 }, bad = 0;
    HIPCHK(h, hipMemcpyAsync(iv, h->d_counters + kCounterCount + 1 + 64, sizeof iv, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&bad, h->d_counters + 8, sizeof bad, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    out[0] = h->debug_invariants ? 1 : 0;
    out[1] = h->iv_checks;
    out[2] = h->iv_violations;
    out[3] = bad;
    // (dealt and written count every sample of a box-hitting pixel, whoever settles it: those of through pixels are the host's)
    const uint64_t settled = h->debug_invariants ? h->host_settled : 0;
    out[4] = iv[0] + settled;
    out[5] = iv[1];
    out[6] = iv[2] + settled;
    out[7] = iv[3];
    return CT_OK;
}

extern "C" int ct_debug_pixel_classes(CtHandle h, uint64_t out[4])
{
    NEED(h);
    if (!out) {
        return fail(h, CT_E_INVAL, "out is NULL");
    }
    if (!h->camera_set) {
        return fail(h, CT_E_STATE, "ct_set_camera has not been called");
    }
    if (h->scene.flags & CT_FLAG_SIMPLE_KERNEL) {
        return fail(h, CT_E_INVAL, "ct_debug_pixel_classes: the one-thread-per-pixel kernel keeps no pixel list");
    }
    if (h->queue_dirty) {   // (the classes of the current pose, rendered or not)
        int rc = flush(h);
        discard_ahead(h);
        if (rc == CT_OK) {
            rc = rebuild_queue(h);
        }
        if (rc != CT_OK) {
            return rc;
        }
    }
    out[0] = h->miss_pixels;
    out[1] = h->listed_pixels;
    out[2] = h->through_pixels;
    out[3] = h->through_steps;
    return CT_OK;
}

extern "C" int ct_debug_pixel_class_plane(CtHandle h, uint32_t *out, size_t count)
{
    NEED(h);
    const size_t pixels = (size_t)h->scene.width * h->scene.height;
    if (!out || count != pixels) {
        return fail(h, CT_E_INVAL, "ct_debug_pixel_class_plane: need room for %zu pixels", pixels);
    }
    uint64_t counts[4];
    const int rc = ct_debug_pixel_classes(h, counts);   // (brings the pose's classes up to date)
    if (rc != CT_OK) {
        return rc;
    }
    std::vector<float4> advance(through_on(h) ? pixels : 0);   // (class 2 appears on no other handle)
    if (!advance.empty()) {
        HIPCHK(h, hipMemcpy(advance.data(), h->d_advance, pixels * sizeof(float4), hipMemcpyDeviceToHost));
    }
    for (size_t p = 0; p < pixels; p++) {
        const uint32_t cls = h->hit_host[p];
        uint32_t steps = 0;
        if (cls == 2u) {
            memcpy(&steps, &advance[p].w, sizeof steps);
            steps &= 0x3fffffffu;
        }
        out[p] = cls << 30 | steps;
    }
    return CT_OK;
}

extern "C" int ct_kernel_time(CtHandle h, double *render_ms_out, double *accumulate_ms_out, uint64_t *launches_out)
{
    NEED(h);
    if (render_ms_out) {
        *render_ms_out = h->render_ms;
    }
    if (accumulate_ms_out) {
        *accumulate_ms_out = h->accum_ms;
    }
    if (launches_out) {
        *launches_out = h->launches;
    }
    return CT_OK;
}

extern "C" int ct_debug_stats(CtHandle h, uint64_t out[64])
{
    NEED(h);
    if (!out) {
        return fail(h, CT_E_INVAL, "out is NULL");
    }
    unsigned long long c[kStatCount];
    HIPCHK(h, hipMemcpyAsync(c, h->d_counters + kCounterCount + 1, sizeof c, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < 64; i++) { // (the conservation tallies behind them: ct_debug_invariants)
        out[i] = c[i];
    }
    return CT_OK;
}

extern "C" int ct_debug_stats_ex(CtHandle h, uint64_t *out, uint32_t count)
{
    NEED(h);
    if (!out || count > (uint32_t)kStatCount) {
        return fail(h, CT_E_INVAL, "out is NULL or count > %d", kStatCount);
    }
    unsigned long long c[kStatCount];
    HIPCHK(h, hipMemcpyAsync(c, h->d_counters + kCounterCount + 1, sizeof c, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (uint32_t i = 0; i < count; i++) {
        out[i] = c[i];
    }
    return CT_OK;
}

// The estimator's working set: which 128-B lines of the density array it reads (march bricks for MARCH; apron or twin bricks
// for DELTA) and of the shadow volume's apron bricks a launch fetches from.  Needs the diagnostics kernels (CT_STATS=1 or
// CT_DEBUG_INVARIANTS=1 at ct_create).  enable != 0 allocates and clears the two bitmaps; 0 frees them.
extern "C" int ct_debug_track_lines(CtHandle h, int32_t enable)
{
    NEED(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (auto &t : h->d_touched) {
        HIPCHK(h, t.reset());
    }
    if (!enable) {
        return CT_OK;
    }
    if (!h->shape.stats) {
        return fail(h, CT_E_STATE, "ct_debug_track_lines needs the diagnostics kernels (CT_STATS=1 at ct_create)");
    }
    if (h->dev.m_rows) {
        return fail(h, CT_E_STATE, "ct_debug_track_lines: not implemented for sparse march bricks");
    }
    const size_t apron_lines = (size_t)h->dev.brick_gxy * (size_t)h->dev.brick_gz;
    size_t density_lines = apron_lines;
    if (h->scene.estimator == CT_EST_MARCH) {
        density_lines = h->mbricks_dense_bytes / 128;
    } else if (h->dev.delta_nee == 2u && h->dev.tbricks) {
        density_lines = (size_t)h->dev.t_gx * h->dev.t_gy * h->dev.t_gz;
    }
    h->touched_lines[0] = density_lines;
    h->touched_lines[1] = apron_lines;
    for (int k = 0; k < 2; k++) {
        const size_t words = (h->touched_lines[k] + 31) / 32;
        HIPCHK(h, h->d_touched[k].alloc(words));
        HIPCHK(h, hipMemsetAsync(h->d_touched[k], 0, words * sizeof(uint32_t), h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CT_OK;
}

// out[0], out[1] = distinct lines touched in the density / shadow arrays since ct_debug_track_lines(h, 1) (or since the last
// call with clear != 0), out[2], out[3] = the arrays' sizes in lines.  Waits for the batches in flight.
extern "C" int ct_debug_touched_lines(CtHandle h, uint64_t out[4], int32_t clear)
{
    NEED(h);
    if (!out || !h->d_touched[0]) {
        return fail(h, CT_E_STATE, "ct_debug_touched_lines: call ct_debug_track_lines(h, 1) first");
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int k = 0; k < 2; k++) {
        const size_t words = (h->touched_lines[k] + 31) / 32;
        std::vector<uint32_t> bits(words);
        HIPCHK(h, hipMemcpy(bits.data(), h->d_touched[k], words * sizeof(uint32_t), hipMemcpyDeviceToHost));
        uint64_t n = 0;
        for (uint32_t w : bits) {
            n += (uint64_t)__builtin_popcount(w);
        }
        out[k] = n;
        out[2 + k] = h->touched_lines[k];
        if (clear) {
            HIPCHK(h, hipMemset(h->d_touched[k], 0, words * sizeof(uint32_t)));
        }
    }
    return CT_OK;
}

extern "C" int ct_debug_memory(CtHandle h, uint64_t out[8])
{
    NEED(h);
    if (!out) {
        return fail(h, CT_E_INVAL, "out is NULL");
    }
    const size_t brick_bytes = (size_t)h->dev.brick_gxy * (size_t)h->dev.brick_gz * 128;
    out[0] = h->volume_bytes;
    out[1] = brick_bytes;                 // density apron bricks
    out[2] = brick_bytes;                 // shadow-volume apron bricks
    out[3] = h->mbricks_dense_bytes;
    out[4] = h->mbricks_bytes;
    out[5] = h->dev.m_rows ? 1 : (h->vmm.va ? 2 : 0);   // 1 row extents, 2 dense addressing with sparse backing (out[4] = the memory behind it)
    out[6] = h->dev.m_rows ? (size_t)h->dev.brick_gy * h->dev.brick_gz * sizeof(uint2) : 0;
    out[7] = h->dev.m_rows ? (size_t)h->dev.m_cgxy * (size_t)((4 * h->dev.brick_gz + 7) >> h->dev.m_cshift) : 0;
    return CT_OK;
}

extern "C" int ct_debug_delta_grid(CtHandle h, uint32_t out[8])
{
    NEED(h);
    if (!out) {
        return fail(h, CT_E_INVAL, "out is NULL");
    }
    const DevScene &d = h->dev;
    const bool delta = d.maj_cells != nullptr;
    out[0] = delta ? (uint32_t)d.mc_cell : 0u;
    out[1] = delta ? (uint32_t)d.mc_gx : 0u;
    out[2] = delta ? (uint32_t)d.mc_gy : 0u;
    out[3] = delta ? (uint32_t)d.mc_gz : 0u;
    out[4] = delta ? (uint32_t)d.mc_x0 : 0u;
    out[5] = delta ? (uint32_t)d.mc_y0 : 0u;
    out[6] = delta ? (uint32_t)d.mc_z0 : 0u;
    out[7] = delta ? (d.delta_nee | (d.delta_interior ? 0x100u : 0u)) : 0u;
    return CT_OK;
}

extern "C" int ct_debug_march_meta(CtHandle h, uint32_t geom_out[8], uint8_t *meta_out, size_t capacity)
{
    NEED(h);
    if (!geom_out) {
        return fail(h, CT_E_INVAL, "geom_out is NULL");
    }
    const DevScene &d = h->dev;
    const size_t rows = (size_t)d.m_gx * d.brick_gy * d.brick_gz * 16;
    geom_out[0] = (uint32_t)h->nee_skip_r;
    geom_out[1] = (uint32_t)d.m_bias_x;
    geom_out[2] = (uint32_t)d.brick_bias;
    geom_out[3] = (uint32_t)d.m_gx;
    geom_out[4] = (uint32_t)d.brick_gy;
    geom_out[5] = (uint32_t)d.brick_gz;
    geom_out[6] = d.m_rows ? 1u : 0u;
    geom_out[7] = 0u;
    if (!meta_out) {
        return CT_OK;
    }
    if (d.m_rows || h->mbricks_bytes != rows * 8 || capacity < rows) {
        return fail(h, CT_E_INVAL, "ct_debug_march_meta: dense march bricks in ordinary memory only, capacity >= %zu", rows);
    }
    std::vector<uint8_t> bricks(h->mbricks_bytes);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(bricks.data(), h->d_mbricks, bricks.size(), hipMemcpyDeviceToHost));
    const size_t gx = (size_t)d.m_gx, gy = (size_t)d.brick_gy, gz = (size_t)d.brick_gz;
    for (size_t bz = 0; bz < gz; bz++) {
        for (size_t by = 0; by < gy; by++) {
            for (size_t bx = 0; bx < gx; bx++) {
                const uint8_t *b = bricks.data() + (((bz * gy + by) * gx + bx) << 7);
                for (size_t lz = 0; lz < 4; lz++) {
                    for (size_t ly = 0; ly < 4; ly++) {
                        meta_out[((bz * 4 + lz) * gy * 4 + by * 4 + ly) * gx + bx] = b[lz * 25 + ly * 5 + 4];
                    }
                }
            }
        }
    }
    return CT_OK;
}

// The device bytes of one volume layout as stored, and the geometry that indexes it (include/cloudtrace.h).  No kernel: a
// stream synchronise and one copy (CT_LAYOUT_MIP_PYRAMID builds the pyramid first if no descriptor call has yet).
extern "C" int ct_debug_layout(CtHandle h, int32_t which, uint32_t geom_out[16], void *dst_host, size_t capacity, size_t *bytes_out)
{
    NEED(h);
    if (!geom_out || !bytes_out) {
        return fail(h, CT_E_INVAL, "geom_out or bytes_out is NULL");
    }
    const DevScene &d = h->dev;
    uint32_t g[16] = { 0 };
    const void *src = nullptr;
    size_t bytes = 0;
    const size_t apron_bytes = (size_t)d.brick_gxy * (size_t)d.brick_gz * 128;
    switch (which) {
    case CT_LAYOUT_DENSITY_BRICKS:
    case CT_LAYOUT_SHADOW_BRICKS:
        src = which == CT_LAYOUT_DENSITY_BRICKS ? h->d_dbricks : h->d_ibricks;
        bytes = apron_bytes;
        g[0] = (uint32_t)d.brick_bias;
        g[1] = (uint32_t)d.brick_gx;
        g[2] = (uint32_t)d.brick_gy;
        g[3] = (uint32_t)d.brick_gz;
        break;
    case CT_LAYOUT_MARCH_BRICKS:
        src = h->vmm.va ? nullptr : h->d_mbricks;   // (a virtual range with holes cannot be copied)
        bytes = h->mbricks_bytes;
        g[0] = (uint32_t)d.m_bias_x;
        g[1] = (uint32_t)d.brick_bias;
        g[2] = (uint32_t)d.m_gx;
        g[3] = (uint32_t)d.brick_gy;
        g[4] = (uint32_t)d.brick_gz;
        g[5] = d.m_rows ? 1u : 0u;
        break;
    case CT_LAYOUT_MARCH_ROWS:
        src = h->d_mrows;
        bytes = (size_t)d.brick_gy * (size_t)d.brick_gz * sizeof(uint2);
        g[0] = (uint32_t)d.brick_gy;
        g[1] = (uint32_t)d.brick_gz;
        break;
    case CT_LAYOUT_MARCH_COARSE:
        src = h->d_mcoarse;
        if (src) {
            const int32_t cgy = d.m_cgxy / d.m_cgx, cgz = (4 * d.brick_gz + 7) >> d.m_cshift;   // (compact_march_bricks)
            bytes = (size_t)d.m_cgxy * (size_t)cgz;
            g[0] = (uint32_t)d.m_cshift;
            g[1] = (uint32_t)d.m_cgx;
            g[2] = (uint32_t)cgy;
            g[3] = (uint32_t)cgz;
            g[4] = (uint32_t)d.brick_bias;
        }
        break;
    case CT_LAYOUT_TWIN_BRICKS:
        src = h->d_tbricks;
        bytes = (size_t)d.t_gx * (size_t)d.t_gy * (size_t)d.t_gz * 128;
        g[0] = (uint32_t)d.t_bias;
        g[1] = (uint32_t)d.t_gx;
        g[2] = (uint32_t)d.t_gy;
        g[3] = (uint32_t)d.t_gz;
        break;
    case CT_LAYOUT_MAJORANT_CELLS:
    case CT_LAYOUT_MAJORANT_CODES:
        src = which == CT_LAYOUT_MAJORANT_CELLS ? h->d_maj_cells : h->d_maj_codes;
        bytes = (size_t)d.mc_gx * (size_t)d.mc_gy * (size_t)d.mc_gz;
        g[0] = (uint32_t)d.mc_cell;
        g[1] = (uint32_t)d.mc_div;
        g[2] = (uint32_t)d.mc_gx;
        g[3] = (uint32_t)d.mc_gy;
        g[4] = (uint32_t)d.mc_gz;
        g[5] = (uint32_t)d.mc_x0;
        g[6] = (uint32_t)d.mc_y0;
        g[7] = (uint32_t)d.mc_z0;
        g[8] = (uint32_t)d.mc_vx;
        g[9] = (uint32_t)d.mc_vy;
        g[10] = (uint32_t)d.mc_vz;
        g[11] = (uint32_t)d.brick_bias;
        break;
    case CT_LAYOUT_MIP_PYRAMID: {
        const int prc = ensure_pyramid(h);   // (built on first use, as in ct_collect_descriptors; the copy below waits for it)
        if (prc != CT_OK) {
            return prc;
        }
        const MipPyramid &mp = h->pyramid;
        src = h->d_pyramid;
        bytes = (size_t)mp.offset[mp.levels - 1u] + (size_t)mp.nx[mp.levels - 1u] * mp.ny[mp.levels - 1u] * mp.nz[mp.levels - 1u];
        g[0] = mp.levels;
        g[1] = (uint32_t)mp.nx[0];
        g[2] = (uint32_t)mp.ny[0];
        g[3] = (uint32_t)mp.nz[0];
        break;
    }
    default:
        return fail(h, CT_E_INVAL, "ct_debug_layout: unknown layout %d", which);
    }
    if (!src) {
        return fail(h, CT_E_INVAL, "ct_debug_layout: this handle has no layout %d", which);
    }
    memcpy(geom_out, g, sizeof g);
    *bytes_out = bytes;
    if (!dst_host) {
        return CT_OK;
    }
    if (capacity < bytes) {
        return fail(h, CT_E_INVAL, "ct_debug_layout: layout %d has %zu bytes, capacity %zu", which, bytes, capacity);
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (bytes) {
        HIPCHK(h, hipMemcpy(dst_host, src, bytes, hipMemcpyDeviceToHost));
    }
    return CT_OK;
}

extern "C" int ct_debug_timeline(CtHandle h, uint64_t *out, uint32_t waves)
{
    NEED(h);
    const size_t have = (size_t)h->shape.blocks * h->shape.threads / 64u;
    if (!h->d_timeline || !out || waves > have) {
        return fail(h, CT_E_INVAL, "ct_debug_timeline: CT_TIMELINE=1 at ct_create, at most %zu waves", have);
    }
    HIPCHK(h, hipMemcpy(out, h->d_timeline, 4 * (size_t)waves * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return CT_OK;
}

extern "C" int ct_debug_suspended(CtHandle h, uint64_t *paths_out)
{
    NEED(h);
    if (!paths_out) {
        return fail(h, CT_E_INVAL, "paths_out is NULL");
    }
    unsigned long long n = 0;
    HIPCHK(h, hipMemcpy(&n, h->d_cont_total, sizeof n, hipMemcpyDeviceToHost));
    *paths_out = n;
    return CT_OK;
}

extern "C" int ct_debug_fetch_probe(int32_t device, uint32_t log2_lines, uint32_t repeats, uint64_t *sum_out)
{
    if (log2_lines < 10 || log2_lines > 28 || hipSetDevice(device) != hipSuccess) {
        return fail(nullptr, CT_E_INVAL, "ct_debug_fetch_probe: bad device or size");
    }
    DevBuf<uint8_t> buf;
    DevBuf<unsigned long long> sum;
    const size_t bytes = (size_t)128 << log2_lines;
    if (buf.alloc(bytes) != hipSuccess || sum.alloc(1) != hipSuccess) {
        return fail(nullptr, CT_E_NOMEM, "ct_debug_fetch_probe: out of device memory");
    }
    hipMemset(buf, 0, bytes);
    hipMemset(sum, 0, 8);
    hipError_t e = hipSuccess;
    for (uint32_t r = 0; r < repeats && e == hipSuccess; r++) {
        e = launch_fetch_probe(buf, log2_lines, (r & 1u) ? 72u : 25u, sum, nullptr); // odd repeats touch both 64-B halves
    }
    if (e == hipSuccess) {
        e = hipDeviceSynchronize();
    }
    unsigned long long v = 0;
    hipMemcpy(&v, sum, 8, hipMemcpyDeviceToHost);
    if (sum_out) {
        *sum_out = v;
    }
    return e == hipSuccess ? CT_OK : fail(nullptr, CT_E_HIP, "fetch probe failed: %s", hipGetErrorString(e));
}

// The same access shape over a WORKING SET: 2^log2_threads lanes each read one pseudo-random line out of `ws_lines` lines, so
// a set smaller than a cache level is re-read from that level (2^25 lanes over 2^20 lines = 128 MiB: every line 32 times per
// launch, far apart in time) -- the line-fill ceiling of the level the set fits in (L2 4 MiB per XCD, Infinity Cache 256 MiB,
// HBM beyond).  `repeats` launches; time two calls with different repeats and take the difference.
extern "C" int ct_debug_fetch_probe_ws(int32_t device, uint32_t log2_threads, uint64_t ws_lines, uint32_t repeats, uint64_t *sum_out)
{
    if (log2_threads < 10 || log2_threads > 28 || ws_lines < 1024 || ws_lines > (1ull << 28) || hipSetDevice(device) != hipSuccess) {
        return fail(nullptr, CT_E_INVAL, "ct_debug_fetch_probe_ws: bad device or size");
    }
    DevBuf<uint8_t> buf;
    DevBuf<unsigned long long> sum;
    const size_t bytes = (size_t)128 * ws_lines;
    if (buf.alloc(bytes) != hipSuccess || sum.alloc(1) != hipSuccess) {
        return fail(nullptr, CT_E_NOMEM, "ct_debug_fetch_probe_ws: out of device memory");
    }
    hipMemset(buf, 0, bytes);
    hipMemset(sum, 0, 8);
    hipError_t e = hipSuccess;
    for (uint32_t r = 0; r < repeats && e == hipSuccess; r++) {
        e = launch_fetch_probe_ws(buf, log2_threads, (uint32_t)ws_lines, r, sum, nullptr);
    }
    if (e == hipSuccess) {
        e = hipDeviceSynchronize();
    }
    unsigned long long v = 0;
    hipMemcpy(&v, sum, 8, hipMemcpyDeviceToHost);
    if (sum_out) {
        *sum_out = v;
    }
    return e == hipSuccess ? CT_OK : fail(nullptr, CT_E_HIP, "fetch probe failed: %s", hipGetErrorString(e));
}

extern "C" int ct_debug_math_selftest(CtHandle h, int32_t which, uint64_t out[3])
{
    NEED(h);
    if (!out || which < 0 || which > 5) {
        return fail(h, CT_E_INVAL, "ct_debug_math_selftest: which = 0 (reciprocal), 1 (square root), 2 (expf_inrange), 3 (logf_above_one), "
                                   "4 (floor_to_int) or 5 (fract_)");
    }
    // Up to two ranges of bit patterns [lo, hi] per test, both ends included.
    // 0, 1: every float with 2^-60 <= x < 2^61 (positive: both functions are odd / undefined for negative arguments in the same way
    //       as the IEEE operations, and the kernels only pass positive values); the reciprocal also for the negative range
    // 2:    every float with -87 < x <= -0.0f, and +0.0f (the march's argument is -sigma * step)
    // 3:    every positive normal float
    // 4:    every float with -2^31 <= x < 2^31, both zeros and the subnormals included
    // 5:    every finite float
    const uint32_t lo = (127u - 60u) << 23, hi = ((127u + 61u) << 23) - 1u;
    const uint32_t ranges[6][4] = {
        { lo, hi, lo | 0x80000000u, hi | 0x80000000u },
        { lo, hi, 1u, 0u },
        { 0x80000000u, 0xc2adffffu, 0u, 0u },           // -87.0f = 0xc2ae0000
        { 0x00800000u, 0x7f7fffffu, 1u, 0u },
        { 0u, 0x4effffffu, 0x80000000u, 0xcf000000u },  // 2^31 = 0x4f000000
        { 0u, 0x7f7fffffu, 0x80000000u, 0xff7fffffu },
    };
    const uint32_t *rg = ranges[which];
    DevBuf<unsigned long long> d;   // (freed on return, which on every path follows a wait for the stream or the device)
    HIPCHK(h, d.alloc(3));
    const unsigned long long init[3] = { 0, 0, 0xffffffffull };
    hipError_t e = hipMemcpyAsync(d, init, sizeof init, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
        e = launch_math_selftest(which, rg[0], rg[1], d, h->stream);
    }
    if (e == hipSuccess && rg[2] <= rg[3]) {
        e = launch_math_selftest(which, rg[2], rg[3], d, h->stream);
    }
    unsigned long long r[3] = { 0, 0, 0 };
    if (e == hipSuccess) {
        e = hipMemcpyAsync(r, d, sizeof r, hipMemcpyDeviceToHost, h->stream);
    }
    if (e == hipSuccess) {
        e = hipStreamSynchronize(h->stream);
    }
    HIPCHK(h, e);
    out[0] = r[0];
    out[1] = r[1];
    out[2] = r[2];
    return CT_OK;
}

extern "C" int ct_debug_math_eval(CtHandle h, int32_t fn, const uint32_t *in_bits, uint32_t n, uint32_t *out_bits)
{
    NEED(h);
    if (!in_bits || !out_bits || n == 0 || n > (1u << 24) || fn < 0 || fn >= CT_MATH_FN_COUNT) {
        return fail(h, CT_E_INVAL, "ct_debug_math_eval: fn in [0, %d), 1 <= n <= 2^24, two words per item in and out", CT_MATH_FN_COUNT);
    }
    DevBuf<uint32_t> d_in, d_out;
    HIPCHK(h, d_in.alloc(2 * (size_t)n));
    HIPCHK(h, d_out.alloc(2 * (size_t)n));
    const size_t bytes = 2 * (size_t)n * sizeof(uint32_t);
    hipError_t e = hipMemcpyAsync(d_in, in_bits, bytes, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
        e = launch_math_eval(fn, d_in, n, d_out, h->stream);
    }
    if (e == hipSuccess) {
        e = hipMemcpyAsync(out_bits, d_out, bytes, hipMemcpyDeviceToHost, h->stream);
    }
    const hipError_t es = hipStreamSynchronize(h->stream);   // before the temporaries go out of scope, whatever happened
    HIPCHK(h, e);
    HIPCHK(h, es);
    return CT_OK;
}

extern "C" int ct_debug_cdf_inversion(CtHandle h, uint32_t first_u24, uint32_t count, uint32_t *k_host_out)
{
    NEED(h);
    if (!k_host_out || count == 0 || (uint64_t)first_u24 + count > (1ull << 24)) {
        return fail(h, CT_E_INVAL, "range must lie inside [0, 2^24)");
    }
    DevBuf<uint32_t> d_k;
    HIPCHK(h, d_k.alloc(count));
    hipError_t e = launch_cdf_selftest(h->d_cdf, h->d_guide, first_u24, count, d_k, h->stream);
    if (e == hipSuccess) {
        e = hipMemcpyAsync(k_host_out, d_k, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream);
    }
    if (e == hipSuccess) {
        e = hipStreamSynchronize(h->stream);
    }
    HIPCHK(h, e);
    return CT_OK;
}

extern "C" int ct_debug_allocations(uint64_t out[4])
{
    if (!out) {
        return CT_E_INVAL;
    }
    for (int i = 0; i < 4; i++) {
        out[i] = g_live_allocations[i].load();
    }
    return CT_OK;
}

extern "C" uint32_t ct_tile_owner(uint32_t tile_x, uint32_t tile_y, uint32_t shard_count)
{
    return tile_owner(tile_x, tile_y, shard_count);
}

extern "C" int ct_shard_tiles(uint32_t width, uint32_t height, uint32_t shard_index, uint32_t shard_count, uint32_t *tiles_out,
                              uint32_t capacity, uint32_t *count_out)
{
    if (width == 0 || height == 0 || shard_count == 0 || shard_index >= shard_count || !count_out) {
        return CT_E_INVAL;
    }
    const uint32_t tiles_x = (width + kTile - 1) / kTile, tiles_y = (height + kTile - 1) / kTile;
    uint32_t count = 0;
    for (uint32_t ty = 0; ty < tiles_y; ty++) {
        for (uint32_t tx = 0; tx < tiles_x; tx++) {
            if (tile_owner(tx, ty, shard_count) != shard_index) {
                continue;
            }
            if (tiles_out && count < capacity) {
                tiles_out[count] = ty * tiles_x + tx;
            }
            count++;
        }
    }
    *count_out = count;
    return tiles_out && count > capacity ? CT_E_INVAL : CT_OK;
}
