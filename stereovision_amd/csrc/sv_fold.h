// sv_fold.h — the per-block fold of a launch's range and counts into the spread accumulator
// copies (kFuseSlots), shared by the kernels that report a map's minimum and maximum
// (sv_fuse.hip, sv_flow.hip).
#pragma once
#include "sv_internal.h"

namespace sv {

// order-preserving integer image of a finite float: a < b  <=>  fkey(a) < fkey(b)
__device__ __forceinline__ uint32_t fkey(float v) {
    const uint32_t u = __float_as_uint(v);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// Accumulators of one launch, zero on entry: [0] max of ~fkey (the minimum), [1] max of fkey,
// [2], [3] counts.  Per block: butterfly inside each wave, four partials through LDS, one
// vector atomic per word into slot (block % kFuseSlots): thousands of same-address atomics
// serialise at L2, so the blocks spread over kFuseSlots copies 128 B apart and the host folds
// them (fuse_stats_fold).
__device__ __forceinline__ void fold_stats(uint32_t kmin_inv, uint32_t kmax, uint32_t n0, uint32_t n1,
                                           uint32_t (*red)[4], uint32_t* stats) {
    for (int off = 32; off > 0; off >>= 1) {
        kmin_inv = max(kmin_inv, (uint32_t)__shfl_xor((int)kmin_inv, off));
        kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, off));
        n0 += (uint32_t)__shfl_xor((int)n0, off);
        n1 += (uint32_t)__shfl_xor((int)n1, off);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[wave][0] = kmin_inv;
        red[wave][1] = kmax;
        red[wave][2] = n0;
        red[wave][3] = n1;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        stats += ((blockIdx.y * gridDim.x + blockIdx.x) % kFuseSlots) * kFuseSlotStride;
        const uint32_t a = red[0][k], b = red[1][k], c = red[2][k], d = red[3][k];
        if (k < 2) atomicMax(&stats[k], max(max(a, b), max(c, d)));
        else if (a + b + c + d) atomicAdd(&stats[k], a + b + c + d);
    }
}

}  // namespace sv
