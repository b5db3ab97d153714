// ct_group.hip -- multi-GPU below the C ABI: one process drives the GPUs of one node.
//
// A CtGroup owns one CtHandle per device -- handle i renders the 8x8-pixel tiles of shard i of N (ct_tile_owner) --
// and an RCCL communicator over those devices (ncclCommInitAll).  ct_group_merge stages every shard's running mean and
// M2 (2 x W*H float4, zeros outside the shard's own tiles) and SUM-reduces them to the first device with ONE ncclReduce
// per device inside ncclGroupStart/End: tiles are disjoint, so the sum is the exact merged frame.  Whole-frame
// quantities (Reinhard's average luminance, Camera::isConverged's count) then run on the merged buffers on the first
// device with the single-GPU arithmetic (ct_tonemap_buffer / ct_is_converged_buffers).
//
// The Python host does the same thing with one process per GPU over torch.distributed (deepestscatter_amd/distributed.py:
// that is what bench.py times); this file is what a C or C++ caller -- the reference's own host is one -- uses instead:
// deepestscatter_amd/host/main.cpp --gpus N.
//
// librccl is loaded with dlopen when the first group is created, so libcloudtrace.so itself does not depend on it (and
// a process that already holds a copy, e.g. PyTorch's, shares it).  A missing library is CT_E_RCCL, never a fallback.
// RCCL refuses two ranks on one device; a device list that repeats a device (a rehearsal on a one-GPU box) therefore
// merges with peer copies and an add kernel on the first device instead -- the same sums, no communicator.
//
// The adaptive frame on a group (ct_group_adaptive_frame_*, at the end of the file) has a merge of its own: the unsigned maximum
// of every 32-bit word instead of a float sum, always by peer copies and a kernel on the first device.
//
// Bakes on a group (ct_group_bake_*, behind it): every shard builds a span of the bake and copies bring every shard the rest.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <set>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/cloudtrace.h"
#include "ct_bake_group.hpp"
#include "ct_devmem.hpp"

namespace {

// the part of rccl.h this file needs (the header's own declarations would make the symbols link-time dependencies)
typedef struct ncclComm *ncclComm_t;
typedef int ncclResult_t;
constexpr int kNcclSuccess = 0, kNcclFloat = 7, kNcclSum = 0;

struct Rccl {
    void *lib = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*Reduce)(const void *, void *, size_t, int, int, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    std::string error;

    std::mutex mu;     // two threads may create their first group at once

    bool load()
    {
        std::lock_guard<std::mutex> lock(mu);
        if (lib) {
            return true;
        }
        void *l = nullptr;
        std::string why;
        for (const char *name : { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" }) {
            l = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (l) {
                break;
            }
            const char *e = dlerror();   // (returns the message ONCE and clears it)
            why = e ? e : "?";
        }
        if (!l) {
            error = "cannot load librccl: " + why;
            return false;
        }
        auto sym = [&](const char *n) { return dlsym(l, n); };
        CommInitAll = (decltype(CommInitAll))sym("ncclCommInitAll");
        CommDestroy = (decltype(CommDestroy))sym("ncclCommDestroy");
        Reduce = (decltype(Reduce))sym("ncclReduce");
        GroupStart = (decltype(GroupStart))sym("ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))sym("ncclGroupEnd");
        GetErrorString = (decltype(GetErrorString))sym("ncclGetErrorString");
        if (!CommInitAll || !CommDestroy || !Reduce || !GroupStart || !GroupEnd || !GetErrorString) {
            error = "librccl lacks an expected symbol";
            return false;
        }
        lib = l;
        return true;
    }
};

Rccl g_rccl;

__global__ void add_into_kernel(float4 *__restrict__ dst, const float4 *__restrict__ src, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float4 a = dst[i], b = src[i];
        dst[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    }
}

// ct_group_adaptive_frame_merge: dst = max(dst, src) on every 32-bit word as an unsigned integer.  A pixel's words are non-zero in
// at most one shard's arrays, so the maximum IS that shard's word, whatever its bit pattern.  n4 uint4, then the words % 4 tail.
__global__ void max_into_kernel(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src, size_t words)
{
    const size_t n4 = words / 4, stride = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint4 *__restrict__ dst4 = (uint4 *)dst;
    const uint4 *__restrict__ src4 = (const uint4 *)src;
    for (size_t i = first; i < n4; i += stride) {
        const uint4 a = dst4[i], b = src4[i];
        dst4[i] = make_uint4(max(a.x, b.x), max(a.y, b.y), max(a.z, b.z), max(a.w, b.w));
    }
    for (size_t i = 4 * n4 + first; i < words; i += stride) {
        dst[i] = max(dst[i], src[i]);
    }
}

} // namespace

namespace ct {
bool adaptive_same_view(CtAdaptiveFrame a, CtAdaptiveFrame b);   // ct_api.cpp: the same pose and light at create?
}

struct CtGroup_ {
    std::vector<CtHandle> handles;
    std::vector<int> devices;
    std::vector<ct::DevBuf<float>> staging;     // per shard, on its device: [mean | M2], 2 * W*H float4
    std::vector<hipStream_t> streams;   // per shard: the stream of the merge
    std::vector<ncclComm_t> comms;      // empty in the rehearsal mode (a device appears twice)
    ct::DevBuf<float> scratch;          // rehearsal mode: landing buffer on the first device
    uint32_t width = 0, height = 0, subframes = 0;
    bool merged = false;
    std::string error;
};

static thread_local std::string g_group_create_error;

static int gfail(CtGroup g, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (g) {
        g->error = buf;
    } else {
        g_group_create_error = buf;
    }
    return code;
}

#define GHIP(g, expr)                                                                                           \
    do {                                                                                                        \
        hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) {                                                                                 \
            return gfail((g), e_ == hipErrorOutOfMemory ? CT_E_NOMEM : CT_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
        }                                                                                                       \
    } while (0)

#define GNCCL(g, expr)                                                                        \
    do {                                                                                      \
        ncclResult_t r_ = (expr);                                                             \
        if (r_ != kNcclSuccess) {                                                             \
            return gfail((g), CT_E_RCCL, "%s failed: %s", #expr, g_rccl.GetErrorString(r_)); \
        }                                                                                     \
    } while (0)

// A shard's failure, with its message.
static int shard_fail(CtGroup g, uint32_t i, int rc)
{
    return gfail(g, rc, "shard %u (device %d): %s", i, g->devices[i], ct_last_error(g->handles[i]));
}

extern "C" int ct_group_destroy(CtGroup g)
{
    if (!g) {
        return CT_OK;
    }
    for (ncclComm_t c : g->comms) {
        if (c) {
            g_rccl.CommDestroy(c);
        }
    }
    for (size_t i = 0; i < g->handles.size(); i++) {
        if (i < g->devices.size()) {
            hipSetDevice(g->devices[i]);
        }
        if (i < g->streams.size() && g->streams[i]) {
            hipStreamSynchronize(g->streams[i]);
            hipStreamDestroy(g->streams[i]);
        }
        if (i < g->staging.size()) {
            g->staging[i].reset();   // (on its device, set above)
        }
        ct_destroy(g->handles[i]);
    }
    if (g->scratch) {
        hipSetDevice(g->devices[0]);
        g->scratch.reset();
    }
    delete g;
    return CT_OK;
}

extern "C" int ct_group_create(const CtScene *scene, const int32_t *devices, uint32_t count, CtGroup *out)
{
    if (!out) {
        return gfail(nullptr, CT_E_INVAL, "out is NULL");
    }
    *out = nullptr;
    if (!scene || !devices || count == 0 || count > 64) {
        return gfail(nullptr, CT_E_INVAL, "ct_group_create: need a scene and 1..64 devices");
    }
    CtGroup g = new (std::nothrow) CtGroup_();
    if (!g) {
        return gfail(nullptr, CT_E_NOMEM, "out of host memory");
    }
    auto bail = [&](int rc) {
        g_group_create_error = g->error;
        ct_group_destroy(g);
        return rc;
    };
    g->width = scene->width;
    g->height = scene->height;
    g->devices.assign(devices, devices + count);
    const bool distinct = std::set<int>(g->devices.begin(), g->devices.end()).size() == count;
    const size_t floats = (size_t)2 * scene->width * scene->height * 4;
    for (uint32_t i = 0; i < count; i++) {
        CtScene s = *scene;
        s.device = devices[i];
        s.shard_index = i;
        s.shard_count = count;
        CtHandle h = nullptr;
        const int rc = ct_create(&s, &h);
        if (rc != CT_OK) {
            g->error = std::string("shard ") + std::to_string(i) + ": " + ct_last_error(nullptr);
            return bail(rc);
        }
        g->handles.push_back(h);
        ct::DevBuf<float> st;
        hipStream_t stream = nullptr;
        const bool ok = hipSetDevice(devices[i]) == hipSuccess && st.alloc(floats) == hipSuccess &&
                        hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess;
        g->staging.push_back(std::move(st));
        g->streams.push_back(stream);
        if (!ok) {
            g->error = "out of device memory (merge staging buffer)";
            return bail(CT_E_NOMEM);
        }
    }
    if (distinct) {
        if (!g_rccl.load()) {
            g->error = g_rccl.error;
            return bail(CT_E_RCCL);
        }
        g->comms.assign(count, nullptr);
        const ncclResult_t r = g_rccl.CommInitAll(g->comms.data(), (int)count, g->devices.data());
        if (r != kNcclSuccess) {
            g->comms.clear();
            g->error = std::string("ncclCommInitAll failed: ") + g_rccl.GetErrorString(r);
            return bail(CT_E_RCCL);
        }
    } else {
        // rehearsal: several shards on one device (RCCL refuses that); merge with copies and adds on the first device
        if (hipSetDevice(devices[0]) != hipSuccess || g->scratch.alloc(floats) != hipSuccess) {
            g->error = "out of device memory (merge scratch)";
            return bail(CT_E_NOMEM);
        }
    }
    *out = g;
    return CT_OK;
}

extern "C" const char *ct_group_last_error(CtGroup g)
{
    return g ? g->error.c_str() : g_group_create_error.c_str();
}

extern "C" int ct_group_size(CtGroup g, uint32_t *count_out)
{
    if (!g || !count_out) {
        return gfail(g, CT_E_INVAL, "null argument");
    }
    *count_out = (uint32_t)g->handles.size();
    return CT_OK;
}

extern "C" int ct_group_handle(CtGroup g, uint32_t index, CtHandle *out)
{
    if (!g || !out || index >= g->handles.size()) {
        return gfail(g, CT_E_INVAL, "ct_group_handle: index out of range");
    }
    *out = g->handles[index];
    return CT_OK;
}

extern "C" int ct_group_set_camera(CtGroup g, const float eye[3], const float U[3], const float V[3], const float W[3])
{
    if (!g) {
        return gfail(nullptr, CT_E_INVAL, "null group");
    }
    for (uint32_t i = 0; i < g->handles.size(); i++) {
        const int rc = ct_set_camera(g->handles[i], eye, U, V, W);
        if (rc != CT_OK) {
            return shard_fail(g, i, rc);
        }
    }
    g->merged = false;
    return CT_OK;
}

// ct_set_light on every shard.  The arguments are checked by the first shard before anything changes; a shard that runs out of
// memory keeps its old light while the shards before it have the new one, so the group is re-lit again or destroyed then.
extern "C" int ct_group_set_light(CtGroup g, const float direction[3], const float color[3], float intensity)
{
    if (!g) {
        return gfail(nullptr, CT_E_INVAL, "null group");
    }
    for (uint32_t i = 0; i < g->handles.size(); i++) {
        const int rc = ct_set_light(g->handles[i], direction, color, intensity);
        if (rc != CT_OK) {
            return shard_fail(g, i, rc);
        }
    }
    g->merged = false;
    return CT_OK;
}

// Every shard enqueues its batch (the devices work at the same time), then every shard is waited for.
extern "C" int ct_group_render_accumulate(CtGroup g, uint32_t first_subframe_id, uint32_t count)
{
    if (!g) {
        return gfail(nullptr, CT_E_INVAL, "null group");
    }
    for (uint32_t i = 0; i < g->handles.size(); i++) {
        const int rc = ct_render_accumulate_async(g->handles[i], first_subframe_id, count);
        if (rc != CT_OK) {
            return shard_fail(g, i, rc);
        }
    }
    for (uint32_t i = 0; i < g->handles.size(); i++) {
        const int rc = ct_synchronize(g->handles[i]);
        if (rc != CT_OK) {
            return shard_fail(g, i, rc);
        }
    }
    g->subframes = first_subframe_id + count - 1;
    g->merged = false;
    return CT_OK;
}

// ---- the scattering network on a group ---------------------------------------------------------------------------------
struct CtGroupNetwork_ {
    CtGroup group = nullptr;
    std::vector<CtNetwork> nets;   // per shard, on its device
};

extern "C" int ct_group_network_destroy(CtGroupNetwork gn)
{
    if (!gn) {
        return CT_OK;
    }
    for (CtNetwork n : gn->nets) {
        ct_network_destroy(n);
    }
    delete gn;
    return CT_OK;
}

extern "C" int ct_group_network_create(CtGroup g, const CtNetworkDesc *d, CtGroupNetwork *out)
{
    if (!g) {
        return gfail(nullptr, CT_E_INVAL, "null group");
    }
    if (!out) {
        return gfail(g, CT_E_INVAL, "ct_group_network_create: out is NULL");
    }
    *out = nullptr;
    CtGroupNetwork gn = new (std::nothrow) CtGroupNetwork_();
    if (!gn) {
        return gfail(g, CT_E_NOMEM, "out of host memory");
    }
    gn->group = g;
    for (uint32_t i = 0; i < g->handles.size(); i++) {
        CtNetwork n = nullptr;
        const int rc = ct_network_create(g->handles[i], d, &n);
        if (rc != CT_OK) {
            ct_group_network_destroy(gn);
            return shard_fail(g, i, rc);
        }
        gn->nets.push_back(n);
    }
    *out = gn;
    return CT_OK;
}

// ct_network_render_shard_accumulate waits for every band's record count, so the devices only work at the same time when every
// shard has a host thread: shards 1 .. N-1 on threads of this call, shard 0 on the caller.  Handles are independent, every
// entry point selects its device on the thread it is called on, and a handle's error message is its own.
extern "C" int ct_group_network_render_accumulate(CtGroup g, CtGroupNetwork gn, const CtNetworkRender *p, uint32_t first_subframe_id,
                                                  uint32_t count)
{
    if (!g) {
        return gfail(nullptr, CT_E_INVAL, "null group");
    }
    if (!gn || gn->group != g || gn->nets.size() != g->handles.size()) {
        return gfail(g, CT_E_INVAL, "ct_group_network_render_accumulate: need a CtGroupNetwork of this group");
    }
    const uint32_t shards = (uint32_t)g->handles.size();
    std::vector<int> codes(shards, CT_OK);
    auto shard = [&](uint32_t i) {
        codes[i] = ct_network_render_shard_accumulate(g->handles[i], gn->nets[i], p, first_subframe_id, count);
    };
    std::vector<std::thread> threads;
    threads.reserve(shards);
    for (uint32_t i = 1; i < shards; i++) {
        threads.emplace_back(shard, i);
    }
    shard(0);
    for (std::thread &t : threads) {
        t.join();
    }
    g->merged = false;
    for (uint32_t i = 0; i < shards; i++) {
        if (codes[i] != CT_OK) {
            return shard_fail(g, i, codes[i]);
        }
    }
    g->subframes = first_subframe_id + count - 1;
    return CT_OK;
}

extern "C" int ct_group_reset(CtGroup g)
{
    if (!g) {
        return gfail(nullptr, CT_E_INVAL, "null group");
    }
    for (uint32_t i = 0; i < g->handles.size(); i++) {
        const int rc = ct_reset(g->handles[i]);
        if (rc != CT_OK) {
            return shard_fail(g, i, rc);
        }
    }
    g->subframes = 0;
    g->merged = false;
    return CT_OK;
}

// The frame reduce: [mean | M2] of every shard, summed onto the first device.
extern "C" int ct_group_merge(CtGroup g)
{
    if (!g) {
        return gfail(nullptr, CT_E_INVAL, "null group");
    }
    const size_t n = (size_t)g->width * g->height;       // float4 per buffer
    const size_t bytes = n * sizeof(float4);
    for (uint32_t i = 0; i < g->handles.size(); i++) {
        int rc = ct_copy_to_device(g->handles[i], CT_BUF_MEAN, g->staging[i], bytes);
        if (rc == CT_OK) {
            rc = ct_copy_to_device(g->handles[i], CT_BUF_M2, (float4 *)g->staging[i].get() + n, bytes);
        }
        if (rc != CT_OK) {
            return shard_fail(g, i, rc);
        }
    }
    if (!g->comms.empty()) {
        GNCCL(g, g_rccl.GroupStart());
        for (uint32_t i = 0; i < g->handles.size(); i++) {
            GHIP(g, hipSetDevice(g->devices[i]));
            GNCCL(g, g_rccl.Reduce(g->staging[i], g->staging[i], 2 * n * 4, kNcclFloat, kNcclSum, 0, g->comms[i], g->streams[i]));
        }
        GNCCL(g, g_rccl.GroupEnd());
        for (uint32_t i = 0; i < g->handles.size(); i++) {
            GHIP(g, hipSetDevice(g->devices[i]));
            GHIP(g, hipStreamSynchronize(g->streams[i]));
        }
    } else {
        GHIP(g, hipSetDevice(g->devices[0]));
        (void)hipGetLastError();
        for (uint32_t i = 1; i < g->handles.size(); i++) {
            GHIP(g, hipMemcpyPeerAsync(g->scratch, g->devices[0], g->staging[i], g->devices[i], 2 * bytes, g->streams[0]));
            hipLaunchKernelGGL(add_into_kernel, dim3(1024), dim3(256), 0, g->streams[0], (float4 *)g->staging[0].get(),
                               (const float4 *)g->scratch.get(), 2 * n);
            GHIP(g, hipGetLastError());
        }
        GHIP(g, hipStreamSynchronize(g->streams[0]));
    }
    g->merged = true;
    return CT_OK;
}

static int need_merge(CtGroup g)
{
    if (!g) {
        return gfail(nullptr, CT_E_INVAL, "null group");
    }
    return g->merged ? CT_OK : ct_group_merge(g);
}

extern "C" int ct_group_download(CtGroup g, int32_t which, void *dst_host, size_t dst_bytes)
{
    const int rc = need_merge(g);
    if (rc != CT_OK) {
        return rc;
    }
    const size_t n = (size_t)g->width * g->height, bytes = n * sizeof(float4);
    if ((which != CT_BUF_MEAN && which != CT_BUF_M2) || !dst_host || dst_bytes != bytes) {
        return gfail(g, CT_E_INVAL, "ct_group_download: CT_BUF_MEAN or CT_BUF_M2, %zu bytes", bytes);
    }
    GHIP(g, hipSetDevice(g->devices[0]));
    GHIP(g, hipMemcpy(dst_host, (float4 *)g->staging[0].get() + (which == CT_BUF_M2 ? n : 0), bytes, hipMemcpyDeviceToHost));
    return CT_OK;
}

extern "C" int ct_group_tonemap(CtGroup g, float exposure, uint8_t *rgba_host, float *avg_luminance_out)
{
    int rc = need_merge(g);
    if (rc != CT_OK) {
        return rc;
    }
    rc = ct_tonemap_buffer(g->handles[0], g->staging[0], exposure, rgba_host, avg_luminance_out);
    return rc == CT_OK ? CT_OK : shard_fail(g, 0, rc);
}

extern "C" int ct_group_is_converged(CtGroup g, int32_t *converged_out, uint64_t *unconverged_pixels_out)
{
    int rc = need_merge(g);
    if (rc != CT_OK) {
        return rc;
    }
    const size_t n = (size_t)g->width * g->height;
    rc = ct_is_converged_buffers(g->handles[0], g->staging[0], (float *)((float4 *)g->staging[0].get() + n), g->subframes, converged_out,
                                 unconverged_pixels_out);
    return rc == CT_OK ? CT_OK : shard_fail(g, 0, rc);
}

extern "C" int ct_group_counters(CtGroup g, CtCounters *out)
{
    if (!g || !out) {
        return gfail(g, CT_E_INVAL, "null argument");
    }
    std::memset(out, 0, sizeof *out);
    for (uint32_t i = 0; i < g->handles.size(); i++) {
        CtCounters c;
        const int rc = ct_counters(g->handles[i], &c);
        if (rc != CT_OK) {
            return shard_fail(g, i, rc);
        }
        out->paths += c.paths;
        out->box_hits += c.box_hits;
        out->density_lookups += c.density_lookups;
        out->inscatter_lookups += c.inscatter_lookups;
        out->scatter_events += c.scatter_events;
        out->depth_capped += c.depth_capped;
    }
    return CT_OK;
}

// ---- the adaptive frame on a group (ct_group_adaptive_frame_*) -----------------------------------------------------------
// One shard frame per handle (ct_adaptive_frame_create_shard): every shard runs its own rounds over its own pixels and never
// waits for another.  The merge stages every shard's [mean | M2 | counts] (9 * W*H words) on its device, copies them one after
// the other into a landing buffer on the first device and folds each with max_into_kernel into shard 0's staging buffer -- the
// one path for every device list, the one ct_group_merge takes in a rehearsal; no collective.
struct CtGroupAdaptiveFrame_ {
    CtGroup group = nullptr;
    std::vector<CtAdaptiveFrame> frames;             // per shard, on its device
    std::vector<ct::DevBuf<uint32_t>> staging;       // per shard, on its device: [mean | M2 | counts]
    ct::DevBuf<uint32_t> landing;                    // on the first device
    CtAdaptiveFrameDesc d{};
    uint32_t cap = 0;
    bool merged = false;
};

extern "C" int ct_group_adaptive_frame_destroy(CtGroupAdaptiveFrame gf)
{
    if (!gf) {
        return CT_OK;
    }
    CtGroup g = gf->group;
    for (size_t i = 0; i < g->handles.size(); i++) {
        hipSetDevice(g->devices[i]);
        if (i < gf->staging.size()) {
            gf->staging[i].reset();
        }
        if (i < gf->frames.size()) {
            ct_adaptive_frame_destroy(gf->frames[i]);
        }
    }
    hipSetDevice(g->devices[0]);
    gf->landing.reset();
    delete gf;
    return CT_OK;
}

extern "C" int ct_group_adaptive_frame_create(CtGroup g, const CtAdaptiveFrameDesc *d, CtGroupAdaptiveFrame *out)
{
    const char *const who = "ct_group_adaptive_frame_create";
    if (!g) {
        return gfail(nullptr, CT_E_INVAL, "null group");
    }
    if (out) {
        *out = nullptr;
    }
    if (!d || !out) {
        return gfail(g, CT_E_INVAL, "%s: need a description and out", who);
    }
    CtGroupAdaptiveFrame gf = new (std::nothrow) CtGroupAdaptiveFrame_();
    if (!gf) {
        return gfail(g, CT_E_NOMEM, "out of host memory");
    }
    gf->group = g;
    gf->d = *d;
    gf->cap = d->max_samples;
    const size_t words = (size_t)9 * g->width * g->height;
    for (uint32_t i = 0; i < g->handles.size(); i++) {
        CtAdaptiveFrame f = nullptr;
        int rc = ct_adaptive_frame_create_shard(g->handles[i], d, &f);
        if (rc != CT_OK) {
            rc = shard_fail(g, i, rc);
            ct_group_adaptive_frame_destroy(gf);
            return rc;
        }
        gf->frames.push_back(f);
        if (i != 0 && !ct::adaptive_same_view(gf->frames[0], f)) {
            ct_group_adaptive_frame_destroy(gf);
            return gfail(g, CT_E_STATE, "%s: shard %u (device %d) has another camera pose or light than shard 0; ct_group_set_camera and "
                                        "ct_group_set_light set them on every shard", who, i, g->devices[i]);
        }
        ct::DevBuf<uint32_t> st;
        const bool ok = hipSetDevice(g->devices[i]) == hipSuccess && st.alloc(words) == hipSuccess;
        gf->staging.push_back(std::move(st));
        if (!ok) {
            (void)hipGetLastError();
            ct_group_adaptive_frame_destroy(gf);
            return gfail(g, CT_E_NOMEM, "%s: out of device memory (staging buffer of shard %u)", who, i);
        }
    }
    if (hipSetDevice(g->devices[0]) != hipSuccess || gf->landing.alloc(words) != hipSuccess) {
        (void)hipGetLastError();
        ct_group_adaptive_frame_destroy(gf);
        return gfail(g, CT_E_NOMEM, "%s: out of device memory (landing buffer)", who);
    }
    *out = gf;
    return CT_OK;
}

// ct_adaptive_frame_update waits for every round's survivor count, so -- as in ct_group_network_render_accumulate -- the devices
// only work at the same time when every shard has a host thread: shards 1 .. N-1 on threads of this call, shard 0 on the caller.
extern "C" int ct_group_adaptive_frame_update(CtGroupAdaptiveFrame gf, uint32_t rounds)
{
    if (!gf) {
        return gfail(nullptr, CT_E_INVAL, "ct_group_adaptive_frame_update: null frame");
    }
    CtGroup g = gf->group;
    const uint32_t shards = (uint32_t)gf->frames.size();
    std::vector<int> codes(shards, CT_OK);
    auto shard = [&](uint32_t i) { codes[i] = ct_adaptive_frame_update(gf->frames[i], rounds); };
    std::vector<std::thread> threads;
    threads.reserve(shards);
    for (uint32_t i = 1; i < shards; i++) {
        threads.emplace_back(shard, i);
    }
    shard(0);
    for (std::thread &t : threads) {
        t.join();
    }
    gf->merged = false;
    for (uint32_t i = 0; i < shards; i++) {
        if (codes[i] != CT_OK) {
            return shard_fail(g, i, codes[i]);
        }
    }
    return CT_OK;
}

extern "C" int ct_group_adaptive_frame_raise_cap(CtGroupAdaptiveFrame gf, uint32_t max_samples)
{
    const char *const who = "ct_group_adaptive_frame_raise_cap";
    if (!gf) {
        return gfail(nullptr, CT_E_INVAL, "%s: null frame", who);
    }
    CtGroup g = gf->group;
    if (max_samples <= gf->cap || max_samples % gf->d.round_samples != 0u || max_samples > (1u << 24)) {
        return gfail(g, CT_E_INVAL, "%s: max_samples %u; a multiple of round_samples (%u) above the cap (%u), at most 2^24", who, max_samples,
                     gf->d.round_samples, gf->cap);
    }
    for (uint32_t i = 0; i < gf->frames.size(); i++) {
        const int rc = ct_adaptive_frame_raise_cap(gf->frames[i], max_samples);
        if (rc != CT_OK) {
            return shard_fail(g, i, rc);
        }
    }
    gf->cap = max_samples;
    gf->merged = false;
    return CT_OK;
}

extern "C" int ct_group_adaptive_frame_info(CtGroupAdaptiveFrame gf, CtAdaptiveFrameInfo *out)
{
    if (!gf || !out) {
        return gfail(gf ? gf->group : nullptr, CT_E_INVAL, "ct_group_adaptive_frame_info: need a frame and out");
    }
    CtAdaptiveFrameInfo sum{};
    for (uint32_t i = 0; i < gf->frames.size(); i++) {
        CtAdaptiveFrameInfo s{};
        const int rc = ct_adaptive_frame_info(gf->frames[i], &s);
        if (rc != CT_OK) {
            return shard_fail(gf->group, i, rc);
        }
        if (i == 0) {
            sum = s;   // width, height, R, min, cap and the tolerances: the same on every shard
            continue;
        }
        sum.rounds = s.rounds > sum.rounds ? s.rounds : sum.rounds;
        sum.pixels += s.pixels;
        sum.live += s.live;
        sum.converged += s.converged;
        sum.capped += s.capped;
        sum.paths += s.paths;
        sum.trace_ms = s.trace_ms > sum.trace_ms ? s.trace_ms : sum.trace_ms;   // (the shards run at the same time)
        sum.fold_ms = s.fold_ms > sum.fold_ms ? s.fold_ms : sum.fold_ms;
        sum.test_ms = s.test_ms > sum.test_ms ? s.test_ms : sum.test_ms;
    }
    *out = sum;
    return CT_OK;
}

extern "C" int ct_group_adaptive_frame_shard(CtGroupAdaptiveFrame gf, uint32_t index, CtAdaptiveFrame *out)
{
    if (!gf || !out || index >= gf->frames.size()) {
        return gfail(gf ? gf->group : nullptr, CT_E_INVAL, "ct_group_adaptive_frame_shard: need a frame, out and an index below the group's size");
    }
    *out = gf->frames[index];
    return CT_OK;
}

extern "C" int ct_group_adaptive_frame_merge(CtGroupAdaptiveFrame gf)
{
    if (!gf) {
        return gfail(nullptr, CT_E_INVAL, "ct_group_adaptive_frame_merge: null frame");
    }
    CtGroup g = gf->group;
    const size_t n = (size_t)g->width * g->height, words = 9 * n;
    const size_t at[3] = { 0, 4 * n, 8 * n }, size[3] = { 4 * n, 4 * n, n };   // in words: mean, M2, counts
    for (uint32_t i = 0; i < gf->frames.size(); i++) {
        GHIP(g, hipSetDevice(g->devices[i]));
        (void)hipGetLastError();
        for (uint32_t which = 0; which < 3; which++) {
            void *src = nullptr;
            const int rc = ct_adaptive_frame_device_ptr(gf->frames[i], which, &src);
            if (rc != CT_OK) {
                return shard_fail(g, i, rc);
            }
            GHIP(g, hipMemcpyAsync(gf->staging[i].get() + at[which], src, size[which] * sizeof(uint32_t), hipMemcpyDeviceToDevice, g->streams[i]));
        }
        GHIP(g, hipStreamSynchronize(g->streams[i]));
    }
    GHIP(g, hipSetDevice(g->devices[0]));
    for (uint32_t i = 1; i < gf->frames.size(); i++) {
        GHIP(g, hipMemcpyPeerAsync(gf->landing, g->devices[0], gf->staging[i], g->devices[i], words * sizeof(uint32_t), g->streams[0]));
        hipLaunchKernelGGL(max_into_kernel, dim3(1024), dim3(256), 0, g->streams[0], gf->staging[0].get(), (const uint32_t *)gf->landing.get(), words);
        GHIP(g, hipGetLastError());
    }
    GHIP(g, hipStreamSynchronize(g->streams[0]));
    gf->merged = true;
    return CT_OK;
}

// The merged array `which` names on the first device and its size; nullptr: no such array.
static uint32_t *group_adaptive_array(CtGroupAdaptiveFrame gf, uint32_t which, size_t &bytes)
{
    const size_t n = (size_t)gf->group->width * gf->group->height;
    switch (which) {
    case CT_ADAPTIVE_MEAN:
        bytes = n * sizeof(float4);
        return gf->staging[0].get();
    case CT_ADAPTIVE_M2:
        bytes = n * sizeof(float4);
        return gf->staging[0].get() + 4 * n;
    case CT_ADAPTIVE_COUNTS:
        bytes = n * sizeof(uint32_t);
        return gf->staging[0].get() + 8 * n;
    default:
        bytes = 0;
        return nullptr;
    }
}

extern "C" int ct_group_adaptive_frame_download(CtGroupAdaptiveFrame gf, uint32_t which, void *host, size_t bytes)
{
    const char *const who = "ct_group_adaptive_frame_download";
    if (!gf) {
        return gfail(nullptr, CT_E_INVAL, "%s: null frame", who);
    }
    CtGroup g = gf->group;
    size_t need = 0;
    const uint32_t *src = group_adaptive_array(gf, which, need);
    if (!src) {
        return gfail(g, CT_E_INVAL, "%s: which = %u; CT_ADAPTIVE_MEAN, CT_ADAPTIVE_M2 or CT_ADAPTIVE_COUNTS", who, which);
    }
    if (!host || bytes != need) {
        return gfail(g, CT_E_INVAL, "%s: need a host array of exactly %zu bytes", who, need);
    }
    if (!gf->merged) {
        const int rc = ct_group_adaptive_frame_merge(gf);
        if (rc != CT_OK) {
            return rc;
        }
    }
    GHIP(g, hipSetDevice(g->devices[0]));
    GHIP(g, hipMemcpy(host, src, need, hipMemcpyDeviceToHost));
    return CT_OK;
}

extern "C" int ct_group_adaptive_frame_device_ptr(CtGroupAdaptiveFrame gf, uint32_t which, void **out)
{
    const char *const who = "ct_group_adaptive_frame_device_ptr";
    if (!gf) {
        return gfail(nullptr, CT_E_INVAL, "%s: null frame", who);
    }
    size_t bytes = 0;
    uint32_t *p = group_adaptive_array(gf, which, bytes);
    if (!p || !out) {
        return gfail(gf->group, CT_E_INVAL, "%s: need CT_ADAPTIVE_MEAN, CT_ADAPTIVE_M2 or CT_ADAPTIVE_COUNTS and out", who);
    }
    if (!gf->merged) {
        const int rc = ct_group_adaptive_frame_merge(gf);
        if (rc != CT_OK) {
            return rc;
        }
    }
    *out = p;
    return CT_OK;
}

// ---- bakes on a group (ct_group_bake_*) -------------------------------------------------------------------------
// One CtBake per shard, on its handle.  A call that builds or continues the bake cuts the nodes it covers into one span per shard
// (ct_bake.cpp: shard i of N takes list positions [i A / N, (i + 1) A / N)), every shard works on its span on a host thread of its
// own -- a bake waits for its chunks as a band of the network renderer does -- and the exchange (ct::bake_exchange: copies, no
// collective) leaves every shard with the whole bake, because a shard's tiles look up anywhere in the table.
struct CtGroupBake_ {
    CtGroup group = nullptr;
    std::vector<CtBake> bakes;   // per shard, on its device
    bool failed = false;         // a shard has failed in a build: good for ct_group_bake_destroy only
    uint64_t exchange_bytes = 0;
    double exchange_ms = 0;      // the last exchange, on the host's clock
};

// f(i) for every shard: shards 1 .. N-1 on threads of this call, shard 0 on the caller.  -> the first failing shard, or N.
template <typename F>
static uint32_t on_every_shard(uint32_t shards, std::vector<int> &codes, F &&f)
{
    codes.assign(shards, CT_OK);
    auto shard = [&](uint32_t i) { codes[i] = f(i); };
    std::vector<std::thread> threads;
    threads.reserve(shards);
    for (uint32_t i = 1; i < shards; i++) {
        threads.emplace_back(shard, i);
    }
    shard(0);
    for (std::thread &t : threads) {
        t.join();
    }
    for (uint32_t i = 0; i < shards; i++) {
        if (codes[i] != CT_OK) {
            return i;
        }
    }
    return shards;
}

static int group_bake_usable(CtGroupBake gb, const char *who)
{
    if (!gb) {
        return gfail(nullptr, CT_E_INVAL, "%s: null group bake", who);
    }
    if (gb->failed) {
        return gfail(gb->group, CT_E_STATE, "%s: a shard of this group bake has failed in a build; it is good for ct_group_bake_destroy only", who);
    }
    return CT_OK;
}

static int group_bake_exchange(CtGroupBake gb, uint64_t paths_before)
{
    char text[512] = "";
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = ct::bake_exchange(gb->bakes.data(), (uint32_t)gb->bakes.size(), paths_before, &gb->exchange_bytes, text, sizeof text);
    gb->exchange_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc != CT_OK) {
        gb->failed = true;
        return gfail(gb->group, rc, "%s", text);
    }
    return CT_OK;
}

extern "C" int ct_group_bake_destroy(CtGroupBake gb)
{
    if (!gb) {
        return CT_OK;
    }
    for (CtBake b : gb->bakes) {
        ct_bake_destroy(b);   // (NULL is a no-op; selects its device)
    }
    delete gb;
    return CT_OK;
}

// The three builds: gn, samples or p says which.
static int group_bake_build(CtGroup g, CtGroupNetwork gn, const CtBakeDesc *d, uint32_t kind, const uint32_t *samples, const CtBakeAdaptive *p,
                            CtGroupBake *out)
{
    const uint32_t shards = (uint32_t)g->handles.size();
    CtGroupBake gb = new (std::nothrow) CtGroupBake_();
    if (!gb) {
        return gfail(g, CT_E_NOMEM, "out of host memory");
    }
    gb->group = g;
    gb->bakes.assign(shards, nullptr);
    std::vector<int> codes;
    const uint32_t bad = on_every_shard(shards, codes, [&](uint32_t i) {
        return ct::bake_create_shard(g->handles[i], gn ? gn->nets[i] : nullptr, d, kind, samples, p, i, shards, &gb->bakes[i]);
    });
    int rc = bad < shards ? shard_fail(g, bad, codes[bad]) : group_bake_exchange(gb, 0);
    if (rc != CT_OK) {
        ct_group_bake_destroy(gb);
        return rc;
    }
    *out = gb;
    return CT_OK;
}

extern "C" int ct_group_network_bake(CtGroup g, CtGroupNetwork gn, const CtBakeDesc *d, uint32_t kind, CtGroupBake *out)
{
    if (!g) {
        return gfail(nullptr, CT_E_INVAL, "null group");
    }
    if (out) {
        *out = nullptr;
    }
    if (!gn || !d || !out) {
        return gfail(g, CT_E_INVAL, "ct_group_network_bake: need a group network, a description and out");
    }
    if (gn->group != g || gn->nets.size() != g->handles.size()) {
        return gfail(g, CT_E_INVAL, "ct_group_network_bake: need a CtGroupNetwork of this group");
    }
    return group_bake_build(g, gn, d, kind, nullptr, nullptr, out);
}

extern "C" int ct_group_bake_traced(CtGroup g, const CtBakeDesc *d, uint32_t kind, uint32_t samples, CtGroupBake *out)
{
    if (!g) {
        return gfail(nullptr, CT_E_INVAL, "null group");
    }
    if (out) {
        *out = nullptr;
    }
    if (!d || !out) {
        return gfail(g, CT_E_INVAL, "ct_group_bake_traced: need a description and out");
    }
    return group_bake_build(g, nullptr, d, kind, &samples, nullptr, out);
}

extern "C" int ct_group_bake_traced_adaptive(CtGroup g, const CtBakeDesc *d, uint32_t kind, const CtBakeAdaptive *p, CtGroupBake *out)
{
    if (!g) {
        return gfail(nullptr, CT_E_INVAL, "null group");
    }
    if (out) {
        *out = nullptr;
    }
    if (!d || !p || !out) {
        return gfail(g, CT_E_INVAL, "ct_group_bake_traced_adaptive: need a description, parameters and out");
    }
    return group_bake_build(g, nullptr, d, kind, nullptr, p, out);
}

// ct_bake_load on every shard: every shard holds the whole bake at once, and is cut for what follows.
extern "C" int ct_group_bake_load(CtGroup g, const char *path, CtGroupBake *out)
{
    if (!g) {
        return gfail(nullptr, CT_E_INVAL, "null group");
    }
    if (out) {
        *out = nullptr;
    }
    if (!path || !out) {
        return gfail(g, CT_E_INVAL, "ct_group_bake_load: need a path and out");
    }
    const uint32_t shards = (uint32_t)g->handles.size();
    CtGroupBake gb = new (std::nothrow) CtGroupBake_();
    if (!gb) {
        return gfail(g, CT_E_NOMEM, "out of host memory");
    }
    gb->group = g;
    gb->bakes.assign(shards, nullptr);
    std::vector<int> codes;
    const uint32_t bad = on_every_shard(shards, codes, [&](uint32_t i) {
        const int rc = ct_bake_load(g->handles[i], path, &gb->bakes[i]);
        return rc != CT_OK ? rc : ct::bake_cut_shard(gb->bakes[i], i, shards);
    });
    if (bad < shards) {
        const int rc = shard_fail(g, bad, codes[bad]);
        ct_group_bake_destroy(gb);
        return rc;
    }
    *out = gb;
    return CT_OK;
}

// A call that continues the bake or builds it again.  The single-GPU call's own checks are passed through from shard 0 before
// any shard works: a refusal leaves everything as it was.  from_zero: the call counts its paths from 0 (retrace).
template <typename F>
static int group_bake_continue(CtGroupBake gb, CtNetwork n0, ct::BakeOp op, uint32_t arg, bool from_zero, F &&call)
{
    CtGroup g = gb->group;
    const uint32_t shards = (uint32_t)gb->bakes.size();
    int rc = ct::bake_op_checks(g->handles[0], n0, gb->bakes[0], op, arg);
    if (rc != CT_OK) {
        return shard_fail(g, 0, rc);
    }
    CtBakeTraceInfo before{};
    rc = ct_bake_trace_info(gb->bakes[0], &before);
    if (rc != CT_OK) {
        return shard_fail(g, 0, rc);
    }
    std::vector<int> codes;
    const uint32_t bad = on_every_shard(shards, codes, call);
    if (bad < shards) {
        gb->failed = true;
        return shard_fail(g, bad, codes[bad]);
    }
    return group_bake_exchange(gb, from_zero ? 0 : before.paths);
}

extern "C" int ct_group_bake_update(CtGroupBake gb, CtGroupNetwork gn)
{
    const char *const who = "ct_group_bake_update";
    const int rc = group_bake_usable(gb, who);
    if (rc != CT_OK) {
        return rc;
    }
    CtGroup g = gb->group;
    if (!gn || gn->group != g || gn->nets.size() != g->handles.size()) {
        return gfail(g, CT_E_INVAL, "%s: need a CtGroupNetwork of the bake's group", who);
    }
    return group_bake_continue(gb, gn->nets[0], ct::BAKE_OP_UPDATE, 0, true,
                               [&](uint32_t i) { return ct_bake_update(g->handles[i], gn->nets[i], gb->bakes[i]); });
}

extern "C" int ct_group_bake_trace_more(CtGroupBake gb, uint32_t samples)
{
    const int rc = group_bake_usable(gb, "ct_group_bake_trace_more");
    if (rc != CT_OK) {
        return rc;
    }
    CtGroup g = gb->group;
    return group_bake_continue(gb, nullptr, ct::BAKE_OP_TRACE_MORE, samples, false,
                               [&](uint32_t i) { return ct_bake_trace_more(g->handles[i], gb->bakes[i], samples); });
}

extern "C" int ct_group_bake_retrace(CtGroupBake gb, uint32_t samples)
{
    const int rc = group_bake_usable(gb, "ct_group_bake_retrace");
    if (rc != CT_OK) {
        return rc;
    }
    CtGroup g = gb->group;
    return group_bake_continue(gb, nullptr, ct::BAKE_OP_RETRACE, samples, true,
                               [&](uint32_t i) { return ct_bake_retrace(g->handles[i], gb->bakes[i], samples); });
}

extern "C" int ct_group_bake_trace_adaptive_more(CtGroupBake gb, uint32_t max_samples)
{
    const int rc = group_bake_usable(gb, "ct_group_bake_trace_adaptive_more");
    if (rc != CT_OK) {
        return rc;
    }
    CtGroup g = gb->group;
    return group_bake_continue(gb, nullptr, ct::BAKE_OP_ADAPTIVE_MORE, max_samples, false,
                               [&](uint32_t i) { return ct_bake_trace_adaptive_more(g->handles[i], gb->bakes[i], max_samples); });
}

extern "C" int ct_group_bake_retrace_adaptive(CtGroupBake gb)
{
    const int rc = group_bake_usable(gb, "ct_group_bake_retrace_adaptive");
    if (rc != CT_OK) {
        return rc;
    }
    CtGroup g = gb->group;
    return group_bake_continue(gb, nullptr, ct::BAKE_OP_RETRACE_ADAPTIVE, 0, true,
                               [&](uint32_t i) { return ct_bake_retrace_adaptive(g->handles[i], gb->bakes[i]); });
}

extern "C" int ct_group_bake_shard(CtGroupBake gb, uint32_t index, CtBake *out)
{
    const char *const who = "ct_group_bake_shard";
    const int rc = group_bake_usable(gb, who);
    if (rc != CT_OK) {
        return rc;
    }
    if (!out || index >= gb->bakes.size()) {
        return gfail(gb->group, CT_E_INVAL, "%s: need out and an index below the group's size", who);
    }
    *out = gb->bakes[index];
    return CT_OK;
}

extern "C" int ct_group_bake_spans(CtGroupBake gb, uint64_t *lo_hi_out, size_t count)
{
    const char *const who = "ct_group_bake_spans";
    const int rc = group_bake_usable(gb, who);
    if (rc != CT_OK) {
        return rc;
    }
    if (!lo_hi_out || count != 2u * gb->bakes.size()) {
        return gfail(gb->group, CT_E_INVAL, "%s: need an array of exactly %zu words, lo and hi per shard", who, 2u * gb->bakes.size());
    }
    for (size_t i = 0; i < gb->bakes.size(); i++) {
        ct::bake_shard_span(gb->bakes[i], lo_hi_out + 2u * i);
    }
    return CT_OK;
}

extern "C" int ct_debug_group_bake_exchange(CtGroupBake gb, uint64_t *bytes_out, double *ms_out)
{
    if (!gb || !bytes_out || !ms_out) {
        return gfail(gb ? gb->group : nullptr, CT_E_INVAL, "ct_debug_group_bake_exchange: need a group bake, bytes_out and ms_out");
    }
    *bytes_out = gb->exchange_bytes;
    *ms_out = gb->exchange_ms;
    return CT_OK;
}

// ct_baked_render_shard_accumulate -- with a depth (1 .. 64), ct_baked_render_hybrid_shard_accumulate -- on every shard, as
// ct_group_network_render_accumulate runs the network renderer.
static int group_baked_accumulate(CtGroup g, CtGroupBake gb, const CtNetworkRender *p, uint32_t depth, bool hybrid, uint32_t first_subframe_id,
                                  uint32_t count)
{
    const char *const who = hybrid ? "ct_group_baked_render_hybrid_accumulate" : "ct_group_baked_render_accumulate";
    if (!g) {
        return gfail(nullptr, CT_E_INVAL, "null group");
    }
    if (!gb || gb->group != g || gb->bakes.size() != g->handles.size()) {
        return gfail(g, CT_E_INVAL, "%s: need a CtGroupBake of this group", who);
    }
    const int rc = group_bake_usable(gb, who);
    if (rc != CT_OK) {
        return rc;
    }
    const uint32_t shards = (uint32_t)g->handles.size();
    std::vector<int> codes;
    const uint32_t bad = on_every_shard(shards, codes, [&](uint32_t i) {
        return hybrid ? ct_baked_render_hybrid_shard_accumulate(g->handles[i], gb->bakes[i], p, depth, first_subframe_id, count)
                      : ct_baked_render_shard_accumulate(g->handles[i], gb->bakes[i], p, first_subframe_id, count);
    });
    g->merged = false;
    if (bad < shards) {
        return shard_fail(g, bad, codes[bad]);
    }
    g->subframes = first_subframe_id + count - 1;
    return CT_OK;
}

extern "C" int ct_group_baked_render_accumulate(CtGroup g, CtGroupBake gb, const CtNetworkRender *p, uint32_t first_subframe_id, uint32_t count)
{
    return group_baked_accumulate(g, gb, p, 0u, false, first_subframe_id, count);
}

extern "C" int ct_group_baked_render_hybrid_accumulate(CtGroup g, CtGroupBake gb, const CtNetworkRender *p, uint32_t depth,
                                                       uint32_t first_subframe_id, uint32_t count)
{
    return group_baked_accumulate(g, gb, p, depth, true, first_subframe_id, count);
}
