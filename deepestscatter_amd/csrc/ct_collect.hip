// ct_collect.hip -- the kernels of the device collector (include/cloudtrace.h, "the radiance collector on the device"; host
// side: ct_api.cpp).  An update of RadianceCollector (RadianceCollector.cpp:73-141) without the host: the rays kernel is
// scheduleTasks' replication (r = T / n threads per live task) as point_rays_kernel would see it, the estimator kernels of
// ct_kernels.hip trace the replicas, the fold kernel folds every replica's results, merges the replicas of a task in order with
// PointRadianceTask::operator+= and tests the stopping rule, and a scan and a ranked write compact the survivors' ids into the
// next update's live list.  The 40-byte replicated task records are never made.
//
// Compile with -ffp-contract=off, like ct_kernels.hip: the bits are those of point_rays_kernel, point_accumulate_kernel and the
// host's merge.
#include "ct_internal.hpp"

namespace ct {

// point_rays_kernel for thread i = t * r + j < n * r: the ray of task live[t], the thread's index as its pixel and in its seed
// base.  Lanes n * r .. n_pad - 1 pad the last group of 64.
__global__ __launch_bounds__(256) void collect_rays_kernel(DevScene sc, CollectArgs a, float4 *__restrict__ primary,
                                                           uint32_t *__restrict__ pixels)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n_pad) {
        return;
    }
    if (i >= a.n * a.r) {
        pixels[i] = 0xffffffffu;
        return;
    }
    pixels[i] = i;
    const uint32_t id = a.live[i / a.r];
    const f3 o = mk3(a.positions[3u * id + 0u], a.positions[3u * id + 1u], a.positions[3u * id + 2u]);
    const f3 d = mk3(a.directions[3u * id + 0u], a.directions[3u * id + 1u], a.directions[3u * id + 2u]);
    float t_hit = 0;
    const bool hit = intersect_box(sc, o, d, t_hit);
    f3 pos = add3(o, scale3(d, t_hit));
    pos = add3(pos, scale3(mk3(sc.bx, sc.by, sc.bz), 0.5f));
    const f3 dir = normalize3(d);
    primary[2 * (size_t)i] = make_float4(pos.x, pos.y, pos.z, hit ? 1.f : 0.f);
    primary[2 * (size_t)i + 1] = make_float4(dir.x, dir.y, dir.z, __uint_as_float(i * 4096u));
}

// PointRadianceTask::addExperimentResult (PointRadianceTask.h:40-51) for thread i's results in frame order, as
// point_accumulate_kernel folds them.
CT_DEV void collect_fold(const float4 *__restrict__ frames, uint32_t stride, uint32_t launches, uint32_t i, float &radiance,
                         float &variance, uint32_t &count)
{
    for (uint32_t f = 0; f < launches; f++) {
        const float new_radiance = frames[(size_t)f * stride + i].x;
        count++;
        const float N = (float)count;
        const float new_weight = (float)(1.0 / (double)N);
        const float previous_mean = radiance;
        const float new_mean = radiance + (new_radiance - previous_mean) * new_weight;
        radiance = new_mean;
        variance += (new_radiance - previous_mean) * (new_radiance - new_mean);
    }
}

// RadianceCollector::update's test (RadianceCollector.cpp:112-118) with the collector's constants: bake_adaptive_converged's
// arithmetic (ct_bake_trace.hip).
CT_DEV bool collect_converged(const CollectArgs &a, float mean, float m2, uint32_t count)
{
    const float N = (float)count;
    const float absolute = div_(1.96f * sqrt_(div_(m2, N)), sqrt_(N));
    const float relative = div_(absolute, mean + 1.1920928955078125e-7f);   // FLT_EPSILON
    bool converged = relative < a.rel_tol || absolute < a.abs_tol;          // (a NaN compares false)
    if (mean < 1.1920928955078125e-7f) {
        converged = count > a.zero_samples;
    }
    return converged;
}

CT_DEV float collect_readlane(float v, uint32_t lane)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (int)lane));
}

// r > 1: wave t is live task t.  Lane l folds replicas l, l + 64, ..: consecutive lanes read consecutive results.  Behind every
// 64 replicas the wave merges them in replica order into the running triple that every lane carries:
//     w = ((float)n1 * 1.0f) / (float)(n0 + n1),  mean = mean + (o.mean - mean) * w,  m2 = m2 + o.m2,  count = n0 + n1
// Every replica but the first holds n1 = launches experiments and n0 = done + j * launches is known without the chain, so lane l
// forms the weight of its own replica beside its fold, and the chain itself is three readlanes, a subtraction, a multiplication
// and two additions per replica: no division, no load, no LDS.  Lane 0 stores the triple and the verdict.
__global__ __launch_bounds__(256) void collect_fold_merge_kernel(CollectArgs a, const float4 *__restrict__ frames, uint32_t stride,
                                                                 uint32_t launches, uint32_t done, uint32_t update,
                                                                 uint32_t *__restrict__ waves)
{
    const uint32_t t = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (t >= a.n) {
        return;   // (the whole wave)
    }
    const uint32_t id = a.live[t], base = t * a.r;
    float mean = 0, m2 = 0;
    for (uint32_t j0 = 0; j0 < a.r; j0 += 64u) {
        const uint32_t j = j0 + lane;
        float radiance = 0, variance = 0, weight = 0;
        if (j < a.r) {
            uint32_t count = 0;
            if (j == 0u) {
                radiance = a.mean[id];
                variance = a.m2[id];
                count = done;
            }
            collect_fold(frames, stride, launches, base + j, radiance, variance, count);
            weight = div_((float)launches * 1.0f, (float)(done + (j + 1u) * launches));
        }
        const uint32_t here = min(64u, a.r - j0);
        uint32_t k = 0;
        if (j0 == 0u) {   // replica 0 is what the others are merged into
            mean = collect_readlane(radiance, 0u);
            m2 = collect_readlane(variance, 0u);
            k = 1;
        }
        for (; k < here; k++) {
            const float o_mean = collect_readlane(radiance, k), o_m2 = collect_readlane(variance, k), w = collect_readlane(weight, k);
            mean = mean + (o_mean - mean) * w;
            m2 = m2 + o_m2;
        }
    }
    if (lane == 0u) {
        const uint32_t count = done + a.r * launches;
        const bool converged = collect_converged(a, mean, m2, count);
        a.mean[id] = mean;
        a.m2[id] = m2;
        a.counts[id] = count;
        if (converged) {
            a.converged_update[id] = update;
        }
        waves[t] = converged ? 0u : 1u;
    }
}

// r == 1: lane t is live task t, its one replica folded from the stored state as point_accumulate_kernel does; wave g counts
// its lanes that fail the rule.  Every lane reaches the ballot.
__global__ __launch_bounds__(256) void collect_fold_single_kernel(CollectArgs a, const float4 *__restrict__ frames, uint32_t stride,
                                                                  uint32_t launches, uint32_t done, uint32_t update,
                                                                  uint32_t *__restrict__ waves)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    bool goes_on = false;
    if (t < a.n) {
        const uint32_t id = a.live[t];
        float radiance = a.mean[id], variance = a.m2[id];
        uint32_t count = done;
        collect_fold(frames, stride, launches, t, radiance, variance, count);
        a.mean[id] = radiance;
        a.m2[id] = variance;
        a.counts[id] = count;
        goes_on = !collect_converged(a, radiance, variance, count);
        if (!goes_on) {
            a.converged_update[id] = update;
        }
    }
    const uint64_t mask = __builtin_amdgcn_ballot_w64(goes_on);
    if ((threadIdx.x & 63u) == 0u && t < a.n) {
        waves[t >> 6] = (uint32_t)__popcll(mask);
    }
}

// bake_adaptive_scan_kernel (ct_bake_trace.hip) over the fold's groups: counts[g] becomes the number of survivors in the groups
// before g, counts[n_groups] their total.  One block.
__global__ __launch_bounds__(1024) void collect_scan_kernel(uint32_t *__restrict__ counts, uint32_t n_groups)
{
    __shared__ uint32_t sums[2][1024];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (n_groups + 1023u) / 1024u;
    const uint32_t begin = min(t * per, n_groups), end = min(begin + per, n_groups);
    uint32_t own = 0;
    for (uint32_t g = begin; g < end; g++) {
        own += counts[g];
    }
    sums[0][t] = own;
    __syncthreads();
    int cur = 0;
    for (uint32_t d = 1; d < 1024u; d *= 2u) {   // Hillis-Steele, inclusive
        sums[cur ^ 1][t] = sums[cur][t] + (t >= d ? sums[cur][t - d] : 0u);
        cur ^= 1;
        __syncthreads();
    }
    uint32_t run = sums[cur][t] - own;
    for (uint32_t g = begin; g < end; g++) {
        const uint32_t c = counts[g];
        counts[g] = run;
        run += c;
    }
    if (t == 1023u) {
        counts[n_groups] = sums[cur][t];
    }
}

// Lane p of the live list: a task that the update has not given a converged_update goes on, and writes its id at its group's
// offset + its rank among the group's survivors (group_shift 0: the group is the task itself; 6: its wave).  live_out is
// ascending like live, whatever order the waves ran in.
__global__ __launch_bounds__(256) void collect_compact_kernel(CollectArgs a, uint32_t group_shift, const uint32_t *__restrict__ offsets,
                                                              uint32_t *__restrict__ live_out)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    bool goes_on = false;
    uint32_t id = 0;
    if (p < a.n) {
        id = a.live[p];
        goes_on = a.converged_update[id] == 0u;
    }
    const uint64_t mask = __builtin_amdgcn_ballot_w64(goes_on);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    if (goes_on) {
        live_out[offsets[p >> group_shift] + (group_shift ? rank : 0u)] = id;
    }
}

hipError_t launch_collect_rays(const DevScene &sc, const CollectArgs &a, float4 *primary, uint32_t *pixels, hipStream_t stream)
{
    hipLaunchKernelGGL(collect_rays_kernel, dim3((a.n_pad + 255u) / 256u), dim3(256), 0, stream, sc, a, primary, pixels);
    return hipGetLastError();
}

hipError_t launch_collect_fold(const CollectArgs &a, const float4 *frames, uint32_t stride, uint32_t launches, uint32_t done,
                               uint32_t update, uint32_t *waves, hipStream_t stream)
{
    if (a.r > 1u) {
        hipLaunchKernelGGL(collect_fold_merge_kernel, dim3((a.n + 3u) / 4u), dim3(256), 0, stream, a, frames, stride, launches, done, update, waves);
    } else {
        hipLaunchKernelGGL(collect_fold_single_kernel, dim3((a.n + 255u) / 256u), dim3(256), 0, stream, a, frames, stride, launches, done, update, waves);
    }
    return hipGetLastError();
}

hipError_t launch_collect_compact(const CollectArgs &a, uint32_t *waves, uint32_t *live_out, hipStream_t stream)
{
    hipLaunchKernelGGL(collect_scan_kernel, dim3(1), dim3(1024), 0, stream, waves, collect_groups(a));
    hipLaunchKernelGGL(collect_compact_kernel, dim3((a.n + 255u) / 256u), dim3(256), 0, stream, a, a.r > 1u ? 0u : 6u, (const uint32_t *)waves, live_out);
    return hipGetLastError();
}

} // namespace ct
