// ct_adaptive.hip -- the kernels of the adaptive frame (include/cloudtrace.h, "the adaptive frame"; host side: ct_api.cpp).  A
// round of the progressive image that goes only to the pixels which have not yet passed Camera::isConverged's test: the rays
// kernel hands the live pixels' primary rays to the estimator kernels of ct_kernels.hip as point tasks that carry the pixel's own
// seed base, the fold kernel is accumulate_list_kernel's Welford update from the pixel's stored state plus the test, and a scan
// and a ranked write compact the survivors into the next round's live list.  No atomics: the same lists every time.
//
// Compile with -ffp-contract=off, like ct_kernels.hip: the bits are those of primary_rays_kernel, welford() and converged_kernel.
#include "ct_internal.hpp"

namespace ct {

// Entry i of a chunk is pixel live[first + i] of the live list, or pixel first + i while the list is still the whole frame.
CT_DEV uint32_t adaptive_pixel(const AdaptiveArgs &a, uint32_t i)
{
    return a.live ? a.live[a.first + i] : a.first + i;
}

// primary_direction (ct_kernels.hip), restated: trace<>, cameraCommon.cuh:18-30.
CT_DEV f3 adaptive_primary_direction(const DevScene &sc, uint32_t x, uint32_t y)
{
    const float dx = (float)x / (float)sc.width * 2.f - 1.f;
    const float dy = (float)y / (float)sc.height * 2.f - 1.f;
    const f3 U = mk3(sc.ux, sc.uy, sc.uz), V = mk3(sc.vx, sc.vy, sc.vz), W = mk3(sc.wx, sc.wy, sc.wz);
    return normalize3(add3(add3(scale3(U, dx), scale3(V, dy)), W));
}

// primary_rays_kernel for the chunk's entries: lane i < n writes the two float4 of its pixel -- seed base x * 4096 + y, so that
// frame id s draws ct_render_subframe's sample of that pixel and subframe s -- at entry i, which is its own "pixel" for the
// estimator.  Lanes n .. n_pad - 1 pad the last group of 64.
__global__ __launch_bounds__(256) void adaptive_rays_kernel(DevScene sc, AdaptiveArgs a, float4 *__restrict__ primary,
                                                            uint32_t *__restrict__ pixels)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n_pad) {
        return;
    }
    if (i >= a.n) {
        pixels[i] = 0xffffffffu;
        return;
    }
    pixels[i] = i;
    const uint32_t p = adaptive_pixel(a, i);
    const uint32_t x = p % sc.width, y = p / sc.width;
    const f3 eye = mk3(sc.ex, sc.ey, sc.ez);
    const f3 d = adaptive_primary_direction(sc, x, y);
    float t_hit = 0;
    const bool hit = intersect_box(sc, eye, d, t_hit);
    f3 pos = add3(eye, scale3(d, t_hit));
    pos = add3(pos, scale3(mk3(sc.bx, sc.by, sc.bz), 0.5f));
    const f3 dir = normalize3(d);
    primary[2 * (size_t)i] = make_float4(pos.x, pos.y, pos.z, hit ? 1.f : 0.f);
    primary[2 * (size_t)i + 1] = make_float4(dir.x, dir.y, dir.z, __uint_as_float(x * 4096u + y));
}

// welford() (ct_kernels.hip), restated: progressive.cu:17-27 on all four channels.
CT_DEV void adaptive_welford(float4 &mu, float4 &var, float4 nr, uint32_t subframe_id)
{
    const float w = 1.0f / (float)subframe_id;
    float4 nm;
    nm.x = mu.x + (nr.x - mu.x) * w;
    nm.y = mu.y + (nr.y - mu.y) * w;
    nm.z = mu.z + (nr.z - mu.z) * w;
    nm.w = mu.w + (nr.w - mu.w) * w;
    var.x = var.x + (nr.x - mu.x) * (nr.x - nm.x);
    var.y = var.y + (nr.y - mu.y) * (nr.y - nm.y);
    var.z = var.z + (nr.z - mu.z) * (nr.z - nm.z);
    var.w = var.w + (nr.w - mu.w) * (nr.w - nm.w);
    mu = nm;
}

// converged_kernel's test (Camera::isConverged, Camera.cpp:232-268) of channel x with the frame's tolerances, in float32 with
// IEEE division and square root.
CT_DEV bool adaptive_converged(const AdaptiveArgs &a, float mean_x, float m2_x, uint32_t count)
{
    const float N = (float)count;
    const float sigma = sqrt_(div_(m2_x, N));
    const float abs_ci = div_(1.96f * sigma, sqrt_(N));
    const float rel_ci = div_(abs_ci, mean_x + 1.1920929e-07f);   // FLT_EPSILON
    return rel_ci < a.rel_tol || abs_ci < a.abs_tol;               // (a NaN compares false)
}

// Does the pixel stay in the list behind a round that left it with `count` samples?  Below min_samples nothing is tested.
CT_DEV bool adaptive_goes_on(const AdaptiveArgs &a, float mean_x, float m2_x, uint32_t count)
{
    return count < a.min_samples || !adaptive_converged(a, mean_x, m2_x, count);
}

// accumulate_list_kernel for the chunk's entries: lane i folds frames[f * stride + i], f < passes -- subframes done + 1 .. done +
// passes, consecutive lanes read consecutive results, eight loads in flight per lane -- onto its pixel's stored mean and M2 and
// stores them with count = done + passes.  With wave_counts (the round's last pass; a.first is a multiple of 64 then, so the
// waves of the chunk are the live list's waves a.first / 64 on) every wave also counts its lanes that fail the rule: every lane
// reaches the ballot.
__global__ __launch_bounds__(256) void adaptive_fold_kernel(AdaptiveArgs a, const float4 *__restrict__ frames, uint32_t stride,
                                                            uint32_t passes, uint32_t done, uint32_t *__restrict__ wave_counts)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool goes_on = false;
    if (i < a.n) {
        const uint32_t p = adaptive_pixel(a, i);
        float4 mu = a.mean[p], var = a.m2[p];
        uint32_t f = 0;
        for (; f + 8 <= passes; f += 8) {
            float4 v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                v[k] = frames[(size_t)(f + k) * stride + i];
            }
#pragma unroll
            for (int k = 0; k < 8; k++) {
                adaptive_welford(mu, var, v[k], done + 1u + f + k);
            }
        }
        for (; f < passes; f++) {
            adaptive_welford(mu, var, frames[(size_t)f * stride + i], done + 1u + f);
        }
        a.mean[p] = mu;
        a.m2[p] = var;
        a.counts[p] = done + passes;
        goes_on = wave_counts != nullptr && adaptive_goes_on(a, mu.x, var.x, done + passes);
    }
    if (wave_counts) {
        const uint64_t mask = __builtin_amdgcn_ballot_w64(goes_on);
        if ((threadIdx.x & 63u) == 0u && i < a.n_pad) {
            wave_counts[(a.first + i) >> 6] = (uint32_t)__popcll(mask);
        }
    }
}

// bake_adaptive_scan_kernel (ct_bake_trace.hip), restated, over the live list's waves: counts[w] becomes the number of survivors
// in the waves before w, counts[n_waves] their total.  One block.
__global__ __launch_bounds__(1024) void adaptive_scan_kernel(uint32_t *__restrict__ counts, uint32_t n_waves)
{
    __shared__ uint32_t sums[2][1024];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (n_waves + 1023u) / 1024u;
    const uint32_t begin = min(t * per, n_waves), end = min(begin + per, n_waves);
    uint32_t own = 0;
    for (uint32_t w = begin; w < end; w++) {
        own += counts[w];
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
    for (uint32_t w = begin; w < end; w++) {
        const uint32_t c = counts[w];
        counts[w] = run;
        run += c;
    }
    if (t == 1023u) {
        counts[n_waves] = sums[cur][t];
    }
}

// Lane q of the whole live list (a.first == 0, a.n == the list's length) tests its pixel's stored state again -- three loads; the
// fold kernel's verdict is not kept -- and a survivor writes its pixel at wave offset + rank: live_out is ascending like the list,
// whatever order the waves ran in.
__global__ __launch_bounds__(256) void adaptive_compact_kernel(AdaptiveArgs a, const uint32_t *__restrict__ wave_offsets,
                                                               uint32_t *__restrict__ live_out)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    bool goes_on = false;
    uint32_t p = 0;
    if (q < a.n) {
        p = adaptive_pixel(a, q);
        goes_on = adaptive_goes_on(a, a.mean[p].x, a.m2[p].x, a.counts[p]);
    }
    const uint64_t mask = __builtin_amdgcn_ballot_w64(goes_on);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    if (goes_on) {
        live_out[wave_offsets[q >> 6] + rank] = p;
    }
}

// ct_adaptive_frame_create_shard: is pixel p of the frame the shard's own?  The tile rule of ct_tile_owner on the pixel's 8 x 8 tile.
CT_DEV bool adaptive_own(const AdaptiveShard &s, uint32_t p)
{
    return tile_owner((p % s.width) >> 3, (p / s.width) >> 3, s.shard_count) == s.shard_index;
}

// The first live list of a shard frame, pass 1: lane p of the frame's pixels tests the tile rule and every wave of 64 consecutive
// pixels writes how many of them are the shard's own.  Every lane reaches the ballot; the last wave's lanes p >= pixels vote no.
__global__ __launch_bounds__(256) void adaptive_own_count_kernel(AdaptiveShard s, uint32_t *__restrict__ wave_counts)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    const bool own = p < s.pixels && adaptive_own(s, p);
    const uint64_t mask = __builtin_amdgcn_ballot_w64(own);
    if ((threadIdx.x & 63u) == 0u && p < s.pixels) {
        wave_counts[p >> 6] = (uint32_t)__popcll(mask);
    }
}

// ... and pass 2, behind adaptive_scan_kernel over those counts: adaptive_compact_kernel's ranked write with the tile rule as the
// predicate.  live_out is the shard's pixels in ascending p, the same list on every run.
__global__ __launch_bounds__(256) void adaptive_own_list_kernel(AdaptiveShard s, const uint32_t *__restrict__ wave_offsets,
                                                                uint32_t *__restrict__ live_out)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    const bool own = p < s.pixels && adaptive_own(s, p);
    const uint64_t mask = __builtin_amdgcn_ballot_w64(own);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    if (own) {
        live_out[wave_offsets[p >> 6] + rank] = p;
    }
}

hipError_t launch_adaptive_own_count(const AdaptiveShard &s, uint32_t *waves, hipStream_t stream)
{
    hipLaunchKernelGGL(adaptive_own_count_kernel, dim3((s.pixels + 255u) / 256u), dim3(256), 0, stream, s, waves);
    hipLaunchKernelGGL(adaptive_scan_kernel, dim3(1), dim3(1024), 0, stream, waves, (s.pixels + 63u) / 64u);
    return hipGetLastError();
}

hipError_t launch_adaptive_own_list(const AdaptiveShard &s, const uint32_t *waves, uint32_t *live_out, hipStream_t stream)
{
    hipLaunchKernelGGL(adaptive_own_list_kernel, dim3((s.pixels + 255u) / 256u), dim3(256), 0, stream, s, waves, live_out);
    return hipGetLastError();
}

hipError_t launch_adaptive_rays(const DevScene &sc, const AdaptiveArgs &a, float4 *primary, uint32_t *pixels, hipStream_t stream)
{
    hipLaunchKernelGGL(adaptive_rays_kernel, dim3((a.n_pad + 255u) / 256u), dim3(256), 0, stream, sc, a, primary, pixels);
    return hipGetLastError();
}

hipError_t launch_adaptive_fold(const AdaptiveArgs &a, const float4 *frames, uint32_t stride, uint32_t passes, uint32_t done,
                                uint32_t *waves, hipStream_t stream)
{
    hipLaunchKernelGGL(adaptive_fold_kernel, dim3((a.n_pad + 255u) / 256u), dim3(256), 0, stream, a, frames, stride, passes, done, waves);
    return hipGetLastError();
}

hipError_t launch_adaptive_compact(const AdaptiveArgs &a, uint32_t *waves, uint32_t *live_out, hipStream_t stream)
{
    hipLaunchKernelGGL(adaptive_scan_kernel, dim3(1), dim3(1024), 0, stream, waves, (a.n + 63u) / 64u);
    hipLaunchKernelGGL(adaptive_compact_kernel, dim3((a.n + 255u) / 256u), dim3(256), 0, stream, a, (const uint32_t *)waves, live_out);
    return hipGetLastError();
}

} // namespace ct
