// ct_bake_trace.hip -- the kernels of the traced bake (include/cloudtrace.h, "the traced bake"; host side: ct_bake.cpp).
// A traced bake fills a probe table with Monte-Carlo means of ct_point_radiance_launch's estimator: the task kernel turns a
// range of the table's stored entries into that entry point's rays, the estimator kernels of ct_kernels.hip trace them, and the
// fold kernel folds the per-experiment results into the table with PointRadianceTask::addExperimentResult's arithmetic.
// The adaptive traced bake ("the adaptive traced bake") traces in rounds: its fold keeps m2 and count beside the mean and tests
// the reference's stopping rule, and a scan and a ranked write compact the entries that go on into the next round's live list.
//
// Compile with -ffp-contract=off, like ct_kernels.hip: the bits are those of point_rays_kernel and point_accumulate_kernel.
#include "ct_internal.hpp"

namespace ct {

// Stored entry s of the bake: a.first + i, or (adaptive) live[a.first + i].  Dense: s is the virtual index e = ((node Nphi) + j) Nc + k.  With a list (sparse and
// compact bakes) s = (r Nphi + j) Nc + k counts through the blocks of the active nodes, node = list[r].  All of it in 64 bits.
struct BakeTraceEntry {
    uint64_t e;          // the virtual index
    uint32_t node, jk;   // jk = j Nc + k
};

// (live: the adaptive bake's list of the stored entries that still take experiments.)
CT_DEV uint64_t bake_trace_stored(const BakeTraceArgs &a, uint32_t i)
{
    return a.live ? (uint64_t)a.live[a.first + i] : a.first + i;
}

CT_DEV BakeTraceEntry bake_trace_entry_of(const BakeTraceArgs &a, uint64_t s)
{
    const uint64_t block = (uint64_t)a.nphi * a.nc;
    const uint64_t r = s / block;
    BakeTraceEntry t;
    t.jk = (uint32_t)(s - r * block);
    t.node = a.list ? a.list[r] : (uint32_t)r;
    t.e = (uint64_t)t.node * block + t.jk;
    return t;
}

CT_DEV BakeTraceEntry bake_trace_entry(const BakeTraceArgs &a, uint32_t i)
{
    return bake_trace_entry_of(a, bake_trace_stored(a, i));
}

// Where stored entry s keeps its value: dense and sparse: [e]; compact: behind the zero block, in list order.
CT_DEV uint64_t bake_trace_address(const BakeTraceArgs &a, uint64_t s)
{
    return a.compact ? (uint64_t)a.nphi * a.nc + s : bake_trace_entry_of(a, s).e;
}

// point_rays_kernel for the entries [first, first + n): the position from the per-axis node tables, the direction from the
// Nphi x Nc direction table, the seed base of the VIRTUAL index (truncated to 32 bits last), the entry's place in the range as
// its pixel.  Lanes n .. n_pad - 1 pad the last group of 64.
__global__ __launch_bounds__(256) void bake_trace_tasks_kernel(DevScene sc, BakeTraceArgs a, float4 *__restrict__ primary,
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
    const BakeTraceEntry t = bake_trace_entry(a, i);
    const uint32_t x = t.node % a.nx, y = t.node / a.nx % a.ny, z = t.node / a.nx / a.ny;
    const f3 o = mk3(a.axes[x], a.axes[a.nx + y], a.axes[a.nx + a.ny + z]);
    const f3 d = mk3(a.directions[3u * t.jk + 0u], a.directions[3u * t.jk + 1u], a.directions[3u * t.jk + 2u]);
    float t_hit = 0;
    const bool hit = intersect_box(sc, o, d, t_hit);
    f3 pos = add3(o, scale3(d, t_hit));
    pos = add3(pos, scale3(mk3(sc.bx, sc.by, sc.bz), 0.5f));
    const f3 dir = normalize3(d);
    primary[2 * (size_t)i] = make_float4(pos.x, pos.y, pos.z, hit ? 1.f : 0.f);
    primary[2 * (size_t)i + 1] = make_float4(dir.x, dir.y, dir.z, __uint_as_float((uint32_t)(t.e * 4096ull)));
}

// point_accumulate_kernel's mean for the same range: the entry's value after `done` experiments is read at its stored address
// -- dense and sparse: table[e]; compact: behind the zero block, in list order -- the pass's results are folded in in frame
// order, and one float goes back.  frames[f * stride + i]: consecutive lanes read consecutive results.
__global__ __launch_bounds__(256) void bake_trace_fold_kernel(BakeTraceArgs a, const float4 *__restrict__ frames, uint32_t stride,
                                                              uint32_t passes, uint32_t done, float *__restrict__ table)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) {
        return;
    }
    const uint64_t at = bake_trace_address(a, bake_trace_stored(a, i));
    float radiance = table[at];
    uint32_t count = done;
    for (uint32_t f = 0; f < passes; f++) {
        const float new_radiance = frames[(size_t)f * stride + i].x;
        count++;
        const float N = (float)count;
        const float new_weight = (float)(1.0 / (double)N);
        radiance = radiance + (new_radiance - radiance) * new_weight;
    }
    table[at] = radiance;
}

// ---- the adaptive traced bake (ct_bake_traced_adaptive): mean, m2 and count per entry, the stopping rule, the compaction -----------
// PointRadianceTask::relativeConfidenceInterval / absoluteConfidenceInterval95 (PointRadianceTask.h:23-36) and the test of
// RadianceCollector::update (RadianceCollector.cpp:112-118) in float32, IEEE division and square root: false = the entry goes on.
CT_DEV bool bake_adaptive_converged(const BakeAdaptiveState &st, float mean, float m2, uint32_t count)
{
    const float N = (float)count;
    const float absolute = div_(1.96f * sqrt_(div_(m2, N)), sqrt_(N));
    const float relative = div_(absolute, mean + 1.1920928955078125e-7f);   // FLT_EPSILON
    bool converged = relative < st.rel_tol || absolute < st.abs_tol;        // (a NaN compares false)
    if (mean < 1.1920928955078125e-7f) {
        converged = count > st.zero_samples;
    }
    return converged;
}

// point_accumulate_kernel for the live entries [first, first + n) of a round: mean, m2 and count at the entry's stored address.
// With wave_counts (the round's last pass) every wave also counts its lanes that fail the rule: every lane reaches the ballot,
// and the waves of a.n_pad lanes -- a.first is a multiple of 64 -- are the live list's waves a.first / 64 on.
__global__ __launch_bounds__(256) void bake_adaptive_fold_kernel(BakeTraceArgs a, const float4 *__restrict__ frames, uint32_t stride,
                                                                 uint32_t passes, uint32_t done, BakeAdaptiveState st,
                                                                 uint32_t *__restrict__ wave_counts)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool goes_on = false;
    if (i < a.n) {
        const uint64_t at = bake_trace_address(a, bake_trace_stored(a, i));
        float radiance = st.table[at], variance = st.m2[at];
        uint32_t count = done;
        for (uint32_t f = 0; f < passes; f++) {
            const float new_radiance = frames[(size_t)f * stride + i].x;
            count++;
            const float N = (float)count;
            const float new_weight = (float)(1.0 / (double)N);
            const float previous_mean = radiance;
            const float new_mean = radiance + (new_radiance - previous_mean) * new_weight;
            radiance = new_mean;
            variance += (new_radiance - previous_mean) * (new_radiance - new_mean);
        }
        st.table[at] = radiance;
        st.m2[at] = variance;
        st.counts[at] = count;
        goes_on = !bake_adaptive_converged(st, radiance, variance, count);
    }
    if (wave_counts) {
        const uint64_t mask = __builtin_amdgcn_ballot_w64(goes_on);
        if ((threadIdx.x & 63u) == 0u && i < a.n_pad) {
            wave_counts[(a.first + i) >> 6] = (uint32_t)__popcll(mask);
        }
    }
}

// ct_bake_load: the fold kernel's count without a fold.  Lane p tests the stored state of stored entry p < n of an active node;
// an entry that stopped by the rule still passes it, so the lanes that fail are the live set the bake was left with.
__global__ __launch_bounds__(256) void bake_adaptive_count_kernel(BakeTraceArgs a, BakeAdaptiveState st, uint32_t n,
                                                                  uint32_t *__restrict__ wave_counts)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    bool goes_on = false;
    if (p < n) {
        const uint64_t at = bake_trace_address(a, p);
        goes_on = !bake_adaptive_converged(st, st.table[at], st.m2[at], st.counts[at]);
    }
    const uint64_t mask = __builtin_amdgcn_ballot_w64(goes_on);
    if ((threadIdx.x & 63u) == 0u && p < ((n + 63u) & ~63u)) {
        wave_counts[p >> 6] = (uint32_t)__popcll(mask);
    }
}

// first_scatter_scan_kernel (ct_kernels.hip) for the live list's waves: counts[w] becomes the number of survivors in the waves
// before w, counts[n_waves] their total.  One block.
__global__ __launch_bounds__(1024) void bake_adaptive_scan_kernel(uint32_t *__restrict__ counts, uint32_t n_waves)
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

// Lane p of the live list tests its entry's stored state again (three loads; the fold kernel's verdict is not kept) and a
// survivor writes its stored index at wave offset + rank: live_out is ascending like live_in, whatever order the waves ran in.
__global__ __launch_bounds__(256) void bake_adaptive_compact_kernel(BakeTraceArgs a, BakeAdaptiveState st, const uint32_t *__restrict__ live_in,
                                                                    uint32_t n_live, const uint32_t *__restrict__ wave_offsets,
                                                                    uint32_t *__restrict__ live_out)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    bool goes_on = false;
    uint32_t s = 0;
    if (p < n_live) {
        s = live_in ? live_in[p] : p;
        const uint64_t at = bake_trace_address(a, s);
        goes_on = !bake_adaptive_converged(st, st.table[at], st.m2[at], st.counts[at]);
    }
    const uint64_t mask = __builtin_amdgcn_ballot_w64(goes_on);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    if (goes_on) {
        live_out[wave_offsets[p >> 6] + rank] = s;
    }
}

// ---- a bake on a group (ct_group_bake_*): a shard's span of the live list ---------------------------------------------------------
// The first round of a shard: live[i] = first + i for i < n, the stored indices of its span (first + n <= 2^26).
__global__ __launch_bounds__(256) void bake_live_iota_kernel(uint32_t *__restrict__ live, uint32_t first, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) {
        live[i] = first + i;
    }
}

// A later call of a shard: bounds[t] = the number of entries of the ascending live[0 .. n) below key t, t < 2.  One block.
__global__ __launch_bounds__(64) void bake_live_bounds_kernel(const uint32_t *__restrict__ live, uint32_t n, uint32_t key_lo, uint32_t key_hi,
                                                              uint32_t *__restrict__ bounds)
{
    if (threadIdx.x >= 2u) {
        return;
    }
    const uint32_t key = threadIdx.x == 0u ? key_lo : key_hi;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (live[mid] < key) {
            lo = mid + 1u;
        } else {
            hi = mid;
        }
    }
    bounds[threadIdx.x] = lo;
}

hipError_t launch_bake_live_iota(uint32_t *live, uint32_t first, uint32_t n, hipStream_t stream)
{
    if (n != 0u) {
        hipLaunchKernelGGL(bake_live_iota_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, live, first, n);
    }
    return hipGetLastError();
}

hipError_t launch_bake_live_bounds(const uint32_t *live, uint32_t n, uint32_t key_lo, uint32_t key_hi, uint32_t *bounds, hipStream_t stream)
{
    hipLaunchKernelGGL(bake_live_bounds_kernel, dim3(1), dim3(64), 0, stream, live, n, key_lo, key_hi, bounds);
    return hipGetLastError();
}

hipError_t launch_bake_adaptive_fold(const BakeTraceArgs &a, const float4 *frames, uint32_t stride, uint32_t passes, uint32_t done,
                                     const BakeAdaptiveState &st, uint32_t *waves, hipStream_t stream)
{
    hipLaunchKernelGGL(bake_adaptive_fold_kernel, dim3((a.n + 255u) / 256u), dim3(256), 0, stream, a, frames, stride, passes, done, st, waves);
    return hipGetLastError();
}

hipError_t launch_bake_adaptive_count(const BakeTraceArgs &a, const BakeAdaptiveState &st, uint32_t n, uint32_t *waves, hipStream_t stream)
{
    hipLaunchKernelGGL(bake_adaptive_count_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, a, st, n, waves);
    return hipGetLastError();
}

hipError_t launch_bake_adaptive_scan(uint32_t *waves, uint32_t n_live, hipStream_t stream)
{
    hipLaunchKernelGGL(bake_adaptive_scan_kernel, dim3(1), dim3(1024), 0, stream, waves, (n_live + 63u) / 64u);
    return hipGetLastError();
}

hipError_t launch_bake_adaptive_compact(const BakeTraceArgs &a, const BakeAdaptiveState &st, const uint32_t *live_in, uint32_t n_live,
                                        const uint32_t *waves, uint32_t *live_out, hipStream_t stream)
{
    hipLaunchKernelGGL(bake_adaptive_compact_kernel, dim3((n_live + 255u) / 256u), dim3(256), 0, stream, a, st, live_in, n_live, waves, live_out);
    return hipGetLastError();
}

hipError_t launch_bake_trace_tasks(const DevScene &sc, const BakeTraceArgs &a, float4 *primary, uint32_t *pixels, hipStream_t stream)
{
    hipLaunchKernelGGL(bake_trace_tasks_kernel, dim3((a.n_pad + 255u) / 256u), dim3(256), 0, stream, sc, a, primary, pixels);
    return hipGetLastError();
}

hipError_t launch_bake_trace_fold(const BakeTraceArgs &a, const float4 *frames, uint32_t stride, uint32_t passes, uint32_t done,
                                  float *table, hipStream_t stream)
{
    hipLaunchKernelGGL(bake_trace_fold_kernel, dim3((a.n + 255u) / 256u), dim3(256), 0, stream, a, frames, stride, passes, done, table);
    return hipGetLastError();
}

} // namespace ct
