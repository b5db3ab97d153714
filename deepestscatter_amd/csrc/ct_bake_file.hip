// ct_bake_file.hip -- the two kernels of include/cloudtrace.h, "bake files" and "half tables" (host side: ct_bake.cpp): the
// volume hash that ties a bake file to its cloud, and the float32 -> binary16 conversion of ct_bake_half.  The half lookup itself
// is bake_lookup<COMPACT, HALF> in ct_kernels.hip.
#include <algorithm>

#include "ct_bakefile.hpp"
#include "ct_internal.hpp"

namespace ct {

// H = sum_i (t_i + 1) * ((i + 1) * 0x9E3779B97F4A7C15) mod 2^64.  Integer addition mod 2^64 is exact in any order: a lane sums
// its grid-strided texels, a wave its lanes through shuffles, and one lane per wave adds to *hash.
__global__ __launch_bounds__(256) void volume_hash_kernel(const uint8_t *__restrict__ texels, uint64_t count, unsigned long long *__restrict__ hash)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    unsigned long long sum = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < count; i += stride) {
        sum += ((unsigned long long)texels[i] + 1ull) * ((i + 1ull) * 0x9E3779B97F4A7C15ull);
    }
    for (int d = 32; d > 0; d >>= 1) {
        sum += __shfl_down(sum, d, 64);
    }
    if ((threadIdx.x & 63u) == 0u) {
        atomicAdd(hash, sum);
    }
}

hipError_t launch_volume_hash(const uint8_t *texels, uint64_t count, unsigned long long *hash, hipStream_t stream)
{
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((count + 255u) / 256u, 1024u);
    if (blocks == 0u) {
        return hipSuccess;
    }
    hipLaunchKernelGGL(volume_hash_kernel, dim3(blocks), dim3(256), 0, stream, texels, count, hash);
    return hipGetLastError();
}

// One lane per stored value; the last block's lanes behind `count` do nothing.  A value half_round_bits would turn into an
// infinity or a NaN is counted and its index offered to the minimum; its bits are stored all the same (the bake is refused).
__global__ __launch_bounds__(256) void bake_half_convert_kernel(const float *__restrict__ table, uint32_t count, uint16_t *__restrict__ half,
                                                                uint32_t *__restrict__ refused)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) {
        return;
    }
    const uint32_t bits = __float_as_uint(table[i]);
    half[i] = half_round_bits(bits);
    if (half_refused(bits)) {
        atomicAdd(&refused[0], 1u);
        atomicMin(&refused[1], i);
    }
}

hipError_t launch_bake_half_convert(const float *table, uint32_t count, uint16_t *half, uint32_t *refused, hipStream_t stream)
{
    hipLaunchKernelGGL(bake_half_convert_kernel, dim3((count + 255u) / 256u), dim3(256), 0, stream, table, count, half, refused);
    return hipGetLastError();
}

} // namespace ct
