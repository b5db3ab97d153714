// ct_bake_trace.hip -- the two kernels of the traced bake (include/cloudtrace.h, "the traced bake"; host side: ct_neural.cpp).
// A traced bake fills a probe table with Monte-Carlo means of ct_point_radiance_launch's estimator: the task kernel turns a
// range of the table's stored entries into that entry point's rays, the estimator kernels of ct_kernels.hip trace them, and the
// fold kernel folds the per-experiment results into the table with PointRadianceTask::addExperimentResult's arithmetic.
//
// Compile with -ffp-contract=off, like ct_kernels.hip: the bits are those of point_rays_kernel and point_accumulate_kernel.
#include "ct_internal.hpp"

namespace ct {

// Stored entry s = a.first + i of the bake.  Dense: s is the virtual index e = ((node Nphi) + j) Nc + k.  With a list (sparse and
// compact bakes) s = (r Nphi + j) Nc + k counts through the blocks of the active nodes, node = list[r].  All of it in 64 bits.
struct BakeTraceEntry {
    uint64_t e;          // the virtual index
    uint32_t node, jk;   // jk = j Nc + k
};

CT_DEV BakeTraceEntry bake_trace_entry(const BakeTraceArgs &a, uint32_t i)
{
    const uint64_t s = a.first + i, block = (uint64_t)a.nphi * a.nc;
    const uint64_t r = s / block;
    BakeTraceEntry t;
    t.jk = (uint32_t)(s - r * block);
    t.node = a.list ? a.list[r] : (uint32_t)r;
    t.e = (uint64_t)t.node * block + t.jk;
    return t;
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
    const uint64_t at = a.compact ? (uint64_t)a.nphi * a.nc + a.first + i : bake_trace_entry(a, i).e;
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
