// sv_stencil.h — the small device helpers the stencil kernel families share (sv_harris.hip,
// sv_hog.hip, sv_median.hip through sv_harris_wave.h).
#pragma once
#include "sv_internal.h"

namespace sv {

__device__ __forceinline__ int refl101(int i, int n) {
    if (n == 1) return 0;
    i = i < 0 ? -i : i;
    return i >= n ? 2 * (n - 1) - i : i;
}

// lane j-1 / j+1 through a plain v_mov_b32_dpp wave_shr/shl:1 kept unfolded: folded into
// an ALU op (v_subrev_u32_dpp ... wave_shr:1 bound_ctrl:1, what the compiler emits for
// old = 0) the wave shifts read 0 on every lane on gfx950 (tools/microbench/dpp_check)
__device__ __forceinline__ int dpp_shr1_keep(int v) {   // lane j-1 (lane 0 keeps its own)
    int t = __builtin_amdgcn_update_dpp(v, v, 0x138, 0xF, 0xF, false);
    asm volatile("" : "+v"(t));
    return t;
}
__device__ __forceinline__ int dpp_shl1_keep(int v) {   // lane j+1 (lane 63 keeps its own)
    int t = __builtin_amdgcn_update_dpp(v, v, 0x130, 0xF, 0xF, false);
    asm volatile("" : "+v"(t));
    return t;
}

// 3x3 Sobel pair at (yc, xc) of a staged byte tile; the caller resolves the neighbour rows
// and columns (reflect-101) to tile indices.
template <int COLS>
__device__ __forceinline__ void sobel_tile(const uint8_t (*t)[COLS], int ym, int yc, int yp, int xm, int xc,
                                           int xp, int& gx, int& gy) {
    gx = (t[ym][xp] + 2 * t[yc][xp] + t[yp][xp]) - (t[ym][xm] + 2 * t[yc][xm] + t[yp][xm]);
    gy = (t[yp][xm] + 2 * t[yp][xc] + t[yp][xp]) - (t[ym][xm] + 2 * t[ym][xc] + t[ym][xp]);
}

}  // namespace sv
