// sv_match.hip — the disparity cost-volume + winner-take-all kernel for gfx950.
//
// Replaces the reference's `cv2.StereoSGBM_create(...).compute(gray_left, gray_right)`
// (depth_map.py:894-909, fused_depth_map.py:988-1004) with the build-defined SAD / SSD /
// HOG winner-take-all engine specified in DESIGN.md ("Semantics").  Output: int16 = d*16,
// invalid = (minD-1)*16 outside the matched band [X0, X1).
//
// Work decomposition (one wave = ROWS output rows (1 or 4), one run of output columns):
//   * the wave is split into G = 64/LPG groups of LPG lanes; group g walks its segment of
//     S columns left to right;
//   * lane l of a group owns the DPL consecutive disparities d = minD + l*DPL + k, so the
//     LPG*DPL candidates of one pixel sit across one group, and the argmin is an in-lane
//     min3 chain over (cost << dbits | d) keys + a DPP row reduction (first-min tie-break);
//   * image data is staged ONCE per wave in LDS as "column packs": the window rows of one
//     column packed 4 bytes per dword (zero padded).  One v_sad_u8 sums 4 vertical taps;
//   * the horizontal window is a running sum along x: per step the group adds the column
//     entering the window and subtracts the column leaving it;
//   * the right-image column a lane needs for disparity k at step t is the column it
//     loaded for k-1 at step t-1, so each lane keeps a DPL-deep register ring and loads
//     ONE new right pack per step (plus one for the leaving column);
//   * right packs are stored with a 1-in-DPL slot gap (rslot) so the 16 lanes of a group,
//     whose columns are DPL apart, hit distinct LDS banks, and a lane's reads inside a
//     DPL-step chunk use static offsets;
//   * the per-pixel DPP reductions of a DPL-step chunk are batched (independent chains)
//     before one coalesced store per lane.
// Cost kinds:
//   SAD   1 row/wave, pack = ceil(win/4) byte dwords, ceil(win/4) v_sad_u8 per column cell;
//   SAD4  4 rows/wave for win >= 5: packs of the 2r-2 rows the four windows share + one
//         word per row for its 3 others; the metric configs run the ring kind
//         (sv_match_ring.hip: a register ring of entering-column costs, v_sad_u32 updates);
//   SSD   v_dot4_u32_u8: sum (L-R)^2 = sum L^2 + sum R^2 - 2 sum L*R (squares per pack);
//   HOG   9-bin u16 window histograms as packs compared with v_sad_u16 (no running window).
// The pack shape, the pack builders and the LDS geometry are in sv_match_packs.h.
#include "sv_match_packs.h"

namespace sv {
namespace {

// 4-row kind: full-length segments when the common words are split into their own array
// (24-B packs, r <= 5); half-length for the 28-B packs of r 6..7, which would otherwise
// hold the LDS to 1.5 waves per SIMD.
int seg_mult(int kind, int r) {
    static const int sm4 = env_int("SV_SAD4_SEG", 1, 8);
    if (kind != COST_SAD4) return 4;
    if (sm4) return sm4;
    return (2 * r - 2 + 3) / 4 <= 2 ? 4 : 2;
}
// 4-row kind with r <= 5 (win <= 11): argmin keys are (cost << 16) | idx, maintained with
// v_sad_hi_u8 (cost max 30855: keys incl. the padding offset stay below 2^32).
__host__ __device__ constexpr bool hi_keys(int cost, int r) { return cost == COST_SAD4 && r <= 5; }
// Column cost(s) of one (left pack, right pack) pair: v[0] (v[0..3]: the four rows of SAD4).
template <int COST, int ND, int NW>
__device__ __forceinline__ void ccol(const Pk<NW>& l, const Pk<NW>& r, uint32_t* v) {
    if constexpr (COST == COST_SAD) {
        uint32_t a = 0u;
#pragma unroll
        for (int i = 0; i < ND; ++i) a = __builtin_amdgcn_sad_u8(l.w[i], r.w[i], a);
        v[0] = a;
    } else if constexpr (COST == COST_SAD4) {
        constexpr int NC = NW - 4;
        uint32_t s = 0u;
#pragma unroll
        for (int i = 0; i < NC; ++i) s = __builtin_amdgcn_sad_u8(l.w[i], r.w[i], s);
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = __builtin_amdgcn_sad_u8(l.w[NC + q], r.w[NC + q], s);
    } else if constexpr (COST == COST_SSD) {
        uint32_t dot = 0u;
#pragma unroll
        for (int i = 0; i < ND; ++i) dot = __builtin_amdgcn_udot4(l.w[i], r.w[i], dot, false);
        v[0] = (l.w[ND] + r.w[ND]) - (dot << 1);
    } else {  // HOG: 9 u16 bins in 5 dwords; the cost IS the cell value
        uint32_t a = 0u;
#pragma unroll
        for (int i = 0; i < 5; ++i) a = __builtin_amdgcn_sad_u16(l.w[i], r.w[i], a);
        v[0] = a;
    }
}

// h + d * m (m = 1 << dbits, |d| < 2^23: one column's cost difference) as ONE
// v_mad_i32_i24.  Through the mul24 intrinsic LLVM does not factor the per-step updates
// into running diff sums (which `h += d << s` in plain C gets: an extra add per cell).
__device__ __forceinline__ uint32_t shl_add(uint32_t d, int m, uint32_t h) {
    return h + (uint32_t)__mul24((int)d, m);
}
template <int COST, int ND, int DPL>
__device__ __forceinline__ void match_chunk(
    const int cut, const int dbits, PackPtr<COST, ND> rnb, PackPtr<COST, ND> rob, PackPtr<COST, ND> lnb,
    PackPtr<COST, ND> lob,
    Pk<PackCfg<COST, ND>::NW> (&rn)[DPL], Pk<PackCfg<COST, ND>::NW> (&ro)[DPL],
    uint32_t (&h)[DPL][PackCfg<COST, ND>::ROWS], const uint32_t (&mk)[DPL],
    uint32_t (&bk)[PackCfg<COST, ND>::ROWS][DPL]) {
    constexpr int NW = PackCfg<COST, ND>::NW;
    constexpr int ROWS = PackCfg<COST, ND>::ROWS;
    constexpr bool RUN = COST != COST_HOG;            // running horizontal window
    constexpr bool HI = hi_keys(COST, ND);            // dbits == 16 (plan_match)
#pragma unroll
    for (int u = 0; u < DPL; ++u) {
        // ring slot u receives this step's entering right column; its previous content
        // (k = DPL-1 of the last step) is dead.  Static offsets inside the chunk; `cut` is
        // the wave-uniform phase of the old ring's slot gap.
        rn[u] = ld<COST, ND>(rnb + u);
        const Pk<NW> L = ld<COST, ND>(lnb + u);
        Pk<NW> LO;
        if constexpr (RUN) {
            ro[u] = ld<COST, ND>(rob + (u + (u >= cut ? 1 : 0)));
            LO = ld<COST, ND>(lob + u);
        }
#pragma unroll
        for (int k = 0; k < DPL; ++k) {
            const int sk = (u - k + DPL) % DPL;
            if constexpr (HI) {
                // keys (cost << 16) | idx updated by v_sad_hi_u8, which adds (SAD << 16):
                // m = (old row-q SAD + old common - new common) << 16, then
                // h = h + (new row-q SAD << 16) - m: 2 v_sad + 1 v_sub per cell, 1 v_sub
                // per 4 cells (instead of 2 v_sad + v_sub + v_mad per cell)
                constexpr int NC = PackCfg<COST, ND>::NC;
                uint32_t cn = 0u, co = 0u;
#pragma unroll
                for (int i = 0; i < NC; ++i) {
                    cn = __builtin_amdgcn_sad_hi_u8(L.w[i], rn[sk].w[i], cn);
                    co = __builtin_amdgcn_sad_hi_u8(LO.w[i], ro[sk].w[i], co);
                }
                const uint32_t nch = co - cn;
#pragma unroll
                for (int q = 0; q < ROWS; ++q) {
                    const uint32_t m = __builtin_amdgcn_sad_hi_u8(LO.w[NC + q], ro[sk].w[NC + q], nch);
                    h[k][q] = __builtin_amdgcn_sad_hi_u8(L.w[NC + q], rn[sk].w[NC + q], h[k][q]) - m;
                }
                continue;
            }
            uint32_t vn[ROWS];
            ccol<COST, ND, NW>(L, rn[sk], vn);
            if constexpr (RUN) {
                // running keys: h = (window cost << dbits) + base; one shift-add per cell
                uint32_t vo[ROWS];
                ccol<COST, ND, NW>(LO, ro[sk], vo);
#pragma unroll
                for (int q = 0; q < ROWS; ++q) h[k][q] = shl_add(vn[q] - vo[q], 1 << dbits, h[k][q]);
            } else {
                h[k][0] = (vn[0] << dbits) | mk[k];
            }
        }
#pragma unroll
        for (int q = 0; q < ROWS; ++q) {
            uint32_t b = 0xFFFFFFFFu;
#pragma unroll
            for (int k = 0; k < DPL; ++k) b = min(b, h[k][q]);
            bk[q][u] = b;
        }
        // one scheduling region per step: without it hipcc hoists every step's LDS reads
        // to the top of the chunk and the register file doubles
        __builtin_amdgcn_sched_barrier(0);
    }
}

// Batched per-pixel reductions of one chunk, branch-free per LPG so the independent DPP
// chains interleave.
// The min lands in the group's LAST lane (every lane for LPG = 16): row_ror within 16-lane
// rows, then row_bcast:15 / row_bcast:31 across rows.
template <int LPG, int N>
__device__ __forceinline__ void reduce_batch(uint32_t* v) {
#define SV_ROR_STEP(CTRL)                                                                     \
    _Pragma("unroll") for (int i = 0; i < N; ++i)                                             \
        v[i] = min(v[i], (uint32_t)__builtin_amdgcn_update_dpp(0u, (int)v[i], CTRL, 0xF, 0xF, false));
    SV_ROR_STEP(0x121)  // row_ror:1
    SV_ROR_STEP(0x122)  // row_ror:2
    SV_ROR_STEP(0x124)  // row_ror:4
    SV_ROR_STEP(0x128)  // row_ror:8
#undef SV_ROR_STEP
    if constexpr (LPG >= 32) {
#pragma unroll
        for (int i = 0; i < N; ++i)
            v[i] = min(v[i], (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v[i], 0x142, 0xA, 0xF, false));
    }
    if constexpr (LPG == 64) {
#pragma unroll
        for (int i = 0; i < N; ++i)
            v[i] = min(v[i], (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v[i], 0x143, 0xC, 0xF, false));
    }
}

// Reduce-scatter of 16 keys over the 16 lanes of a row (LPG = 16, ROWS * DPL = 16):
// on return lane l's v[0] is the min over the row of key index l.  Four butterfly steps
// with XOR partners 15, 7, 3, 1 (row_mirror, row_half_mirror, quad perms); at each step a
// lane keeps the half of its keys selected by the partner bit and sends the other half:
// 8+4+2+1 fused v_min_u32_dpp plus 2 selects each, instead of 16 x 4 row_ror steps.
__device__ __forceinline__ void reduce_scatter16(uint32_t (&v)[16], int l) {
#define SV_RS_STEP(HALF, BIT, CTRL)                                                            \
    {                                                                                          \
        const bool hi = (l & (BIT)) != 0;                                                      \
        _Pragma("unroll") for (int k = 0; k < (HALF); ++k) {                                   \
            const uint32_t send = hi ? v[k] : v[k + (HALF)];                                   \
            const uint32_t keep = hi ? v[k + (HALF)] : v[k];                                   \
            v[k] = min(keep, (uint32_t)__builtin_amdgcn_update_dpp(0u, (int)send, CTRL, 0xF, 0xF, false)); \
        }                                                                                      \
    }
    SV_RS_STEP(8, 8, 0x140)   // row_mirror:      partner l ^ 15
    SV_RS_STEP(4, 4, 0x141)   // row_half_mirror: partner l ^ 7
    SV_RS_STEP(2, 2, 0x1B)    // quad_perm 3210:  partner l ^ 3
    SV_RS_STEP(1, 1, 0xB1)    // quad_perm 1032:  partner l ^ 1
#undef SV_RS_STEP
}
// Occupancy target: LDS admits ~3 blocks/CU for the common configs (D <= 128, win <= 11),
// so cap registers at 3 waves/SIMD (<= 168 VGPRs); the widest packs get 2 waves/SIMD.
template <int COST, int ND> struct Occ {
    static constexpr int W = COST == COST_SAD4 ? 2 : (COST == COST_SAD || ND <= 3) ? 3 : 2;
};

template <int COST, int ND, int DPL>
__global__ __launch_bounds__((64 * PackCfg<COST, ND>::WPB), (Occ<COST, ND>::W)) void k_match(MatchParams a) {
    constexpr int NW = PackCfg<COST, ND>::NW;
    constexpr int ROWS = PackCfg<COST, ND>::ROWS;
    extern __shared__ __attribute__((aligned(16))) uint4 smem[];
    if (blockIdx.z) {   // frame batch
        a.L += blockIdx.z * a.fs_in;
        a.R += blockIdx.z * a.fs_in;
        a.out += blockIdx.z * a.fs_out;
        if constexpr (COST == COST_HOG) {
            a.HL += blockIdx.z * a.fs_hist;
            a.HR += blockIdx.z * a.fs_hist;
        }
    }
    const int lane = threadIdx.x & 63;
    const int wid = PackCfg<COST, ND>::WPB == 1 ? 0 : (int)(threadIdx.x >> 6);
    const int LPG = a.lpg;
    const int S = seg_width(LPG, DPL, a.segm);      // segment width per group
    const int WC = wave_cols(LPG, DPL, a.segm);
    const int r = a.r;
    const int W2 = 2 * r + 1;
    SV_MATCH_REGIONS(WC, LPG, DPL, r)
    // per-wave LDS region: [L main | R main | L common | R common] (common arrays: SPLIT)
    using P = PackCfg<COST, ND>;
    uint4* wbase = reinterpret_cast<uint4*>(reinterpret_cast<char*>(smem) + (size_t)wid * (NL + NRphys) * P::SLOT_BYTES);
    typename P::CT* cbase = reinterpret_cast<typename P::CT*>(wbase + (size_t)(NL + NRphys) * P::QX);
    const PackOut<COST, ND> Lw{wbase, cbase};
    const PackOut<COST, ND> Rw{wbase + (size_t)NL * P::QX, cbase + NL};
    const PackPtr<COST, ND> Lp{Lw.x, Lw.c};
    const PackPtr<COST, ND> Rp{Rw.x, Rw.c};

    const int y = a.row0 + ((int)blockIdx.y * PackCfg<COST, ND>::WPB + wid) * ROWS;
    const int yc = min(y, a.row1 - 1);
    const int xw = a.X0 + (int)blockIdx.x * WC;
    const int cL0 = xw - 3 * r - 1;
    const int cR0 = cL0 - a.minD - (LPG * DPL - 1);

    build_all_packs<COST, ND, DPL>(a, yc, cL0, NL, cR0, NRlog, c0, Lw, Rw, lane);

    if (blockIdx.x == 0) {  // columns outside the matched band are invalid
        const int16_t inv = (int16_t)((a.minD - 1) * 16);
#pragma unroll
        for (int q = 0; q < ROWS; ++q) {
            if (y + q >= a.row1) break;
            int16_t* orow = a.out + (size_t)(y + q) * a.opitch;
            for (int x = lane; x < a.X0; x += 64) orow[x] = inv;
            for (int x = a.X1 + lane; x < a.W; x += 64) orow[x] = inv;
        }
    }
    __syncthreads();
    if (y >= a.row1) return;

    const int g = lane >> a.lpg_log2;
    const int l = lane & (LPG - 1);
    // disparity slot of the lane inside its group: lanes of odd 16-lane rows are rotated by
    // 8, which makes the per-step right-pack ds_read_b128 conflict-free across the two
    // groups that share a b128 lane group (the min over a group does not depend on the
    // order; emission uses the physical lane)
    const int sl = l ^ (((lane >> 4) & 1) << 3);
    const int xs = xw + g * S;
    const int iL0 = g * S + 2 * r + 1;                   // L index of the window's first column
    const int iR0 = g * S + 2 * r + (LPG - sl) * DPL;  // R index of (first column, k = 0)
    const uint32_t dmask = (1u << a.dbits) - 1u;
    const int dbits = a.dbits;
    const int j = l - (LPG - 16);                        // emitting lane -> step within a chunk

    // argmin keys (cost << dbits) | idx.  Running kinds keep the key itself in h, starting
    // from its base: idx, or for padding disparities (idx >= D) idx + (cmax + 1) << dbits so
    // they can never win (plan_match checks the range).  HOG forms keys with mk.
    uint32_t mk[DPL];
    uint32_t h[DPL][ROWS], bk[ROWS][DPL];
#pragma unroll
    for (int k = 0; k < DPL; ++k) {
        const int idx = sl * DPL + k;
        mk[k] = idx < a.D ? (uint32_t)idx : 0xFFFFFFFFu;
#pragma unroll
        for (int q = 0; q < ROWS; ++q) h[k][q] = idx < a.D ? (uint32_t)idx : a.pad_key | (uint32_t)idx;
    }

    // ---- prologue: window of output column xs = the W2 columns xs-r .. xs+r, added directly
    for (int t = 0; t < W2; ++t) {
        const Pk<NW> L = ld<COST, ND>(Lp + (iL0 + t));
#pragma unroll
        for (int k = 0; k < DPL; ++k) {
            uint32_t vn[ROWS];
            ccol<COST, ND, NW>(L, ld<COST, ND>(Rp + rslot(iR0 + t - k, c0, DPL)), vn);
            if constexpr (COST == COST_HOG) h[k][0] = (vn[0] << dbits) | mk[k];
            else {
#pragma unroll
                for (int q = 0; q < ROWS; ++q) h[k][q] += vn[q] << dbits;
            }
        }
    }
    {
        const bool emit0 = j == 0 && xs < a.X1;
#pragma unroll
        for (int q = 0; q < ROWS; ++q) {
            uint32_t b = 0xFFFFFFFFu;
#pragma unroll
            for (int k = 0; k < DPL; ++k) b = min(b, h[k][q]);
            if (LPG == 16) reduce_batch<16, 1>(&b);
            else if (LPG == 32) reduce_batch<32, 1>(&b);
            else reduce_batch<64, 1>(&b);
            if (emit0 && y + q < a.row1)
                a.out[(size_t)(y + q) * a.opitch + xs] = key_disp16(b, dmask, a.minD);
        }
    }

    // ---- main loop: step t' adds column xs+r+1+t' and drops column xs-r+t' (output
    // xs+1+t'), in chunks of DPL steps with static ring slots and static LDS offsets.
    // c0 aligns chunk starts with the right-pack slot gaps (see rslot); the leaving
    // column's reads trail by W2 packs, so their gap phase is (-W2) mod DPL for every lane.
    const int phi = (DPL - W2 % DPL) % DPL;
    const int cut = DPL - phi;                           // old slot offsets u >= cut skip a gap
    const int iN = iR0 + W2;                             // R index of the entering column, t' = 0
    Pk<NW> rn[DPL], ro[DPL];
#pragma unroll
    for (int s = 1; s < DPL; ++s) {                      // virtual steps t' = s - DPL
        rn[s] = ld<COST, ND>(Rp + rslot(iN - (DPL - s), c0, DPL));
        if constexpr (COST != COST_HOG) ro[s] = ld<COST, ND>(Rp + rslot(iR0 - (DPL - s), c0, DPL));
    }
    const PackPtr<COST, ND> rn0 = Rp + rslot(iN, c0, DPL);
    const PackPtr<COST, ND> ro0 = Rp + rslot(iR0, c0, DPL);
    const PackPtr<COST, ND> ln0 = Lp + (iL0 + W2);
    const PackPtr<COST, ND> lo0 = Lp + iL0;
    const int T = (S - 1 + DPL - 1) / DPL * DPL;

    for (int t0 = 0, c = 0; t0 < T; t0 += DPL, ++c) {
        match_chunk<COST, ND, DPL>(cut, dbits, rn0 + c * (DPL + 1), ro0 + c * (DPL + 1), ln0 + t0, lo0 + t0, rn,
                                   ro, h, mk, bk);
        if constexpr (ROWS * DPL == 16 || ROWS * DPL == 32) {
            if (LPG == 16) {   // reduce-scatter: lane l ends with key (row l / DPL, step l % DPL)
#pragma unroll
                for (int half = 0; half < ROWS * DPL / 16; ++half) {
                    uint32_t v[16];
#pragma unroll
                    for (int i = 0; i < 16; ++i) v[i] = bk[(16 * half + i) / DPL][i % DPL];
                    reduce_scatter16(v, l);
                    const int q = (16 * half) / DPL + l / DPL, e = t0 + l % DPL + 1, x = xs + e;
                    if (e < S && x < a.X1 && y + q < a.row1)
                        a.out[(size_t)(y + q) * a.opitch + x] = key_disp16(v[0], dmask, a.minD);
                }
                continue;
            }
        }
        if constexpr (ROWS * DPL == 8) {
            // 8 keys (HOG, 1-row SAD/SSD with DPL 8, 2-row SAD2 with DPL 4): bank-masked
            // reduce-scatter over each 16-lane row, then the rows of a group joined by
            // permlane swaps; lanes 2i of the group's first row emit key i
            uint32_t v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = bk[i / DPL][i % DPL];
            reduce_scatter8_bm(v, lane & 15);
            uint32_t key = v[0];
            if (LPG >= 32) {
                const auto p = __builtin_amdgcn_permlane16_swap(key, key, false, false);
                key = min(p[0], p[1]);
            }
            if (LPG == 64) {
                const auto p = __builtin_amdgcn_permlane32_swap(key, key, false, false);
                key = min(p[0], p[1]);
            }
            const int i = (l >> 1) & 7, q = i / DPL, e = t0 + i % DPL + 1, x = xs + e;
            if (l < 16 && (l & 1) == 0 && e < S && x < a.X1 && y + q < a.row1)
                a.out[(size_t)(y + q) * a.opitch + x] = key_disp16(key, dmask, a.minD);
            continue;
        }
        const int e = t0 + j + 1;
        const int x = xs + e;
        const bool emit = j >= 0 && j < DPL && e < S && x < a.X1;
        // ROWS*DPL independent group reductions (ILP instead of a serial DPP chain per step)
        if (LPG == 16) reduce_batch<16, ROWS * DPL>(&bk[0][0]);
        else if (LPG == 32) reduce_batch<32, ROWS * DPL>(&bk[0][0]);
        else reduce_batch<64, ROWS * DPL>(&bk[0][0]);
#pragma unroll
        for (int q = 0; q < ROWS; ++q) {
            uint32_t v = bk[q][0];
#pragma unroll
            for (int u = 1; u < DPL; ++u) v = (j == u) ? bk[q][u] : v;
            if (emit && y + q < a.row1)
                a.out[(size_t)(y + q) * a.opitch + x] = key_disp16(v, dmask, a.minD);
        }
    }
}
__global__ void k_fill_i16(int16_t* out, int opitch, int H, int W, int16_t v) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x < W && y < H) out[(size_t)y * opitch + x] = v;
}

template <int COST, int ND, int DPL>
int launch_one(const MatchParams& a, size_t lds, hipStream_t s) {
    auto fn = k_match<COST, ND, DPL>;
    if (lds > 65536) {  // opt in to > 64 KiB of dynamic LDS (per device, cheap host call)
        hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    const int wc = wave_cols(a.lpg, DPL, a.segm);
    const int rows_per_block = PackCfg<COST, ND>::WPB * PackCfg<COST, ND>::ROWS;
    dim3 grid((a.X1 - a.X0 + wc - 1) / wc, (a.row1 - a.row0 + rows_per_block - 1) / rows_per_block,
              a.nf > 1 ? a.nf : 1);
    hipLaunchKernelGGL(fn, grid, dim3(64 * PackCfg<COST, ND>::WPB), lds, s, a);
    return (int)hipGetLastError();
}

template <int COST, int ND>
int launch_dpl(const MatchParams& a, const MatchPlan& p, size_t lds, hipStream_t s) {
    switch (p.dpl) {
        case 4: return launch_one<COST, ND, 4>(a, lds, s);
        case 6: return launch_one<COST, ND, 6>(a, lds, s);
        case 8: return launch_one<COST, ND, 8>(a, lds, s);
    }
    return (int)hipErrorInvalidValue;
}

template <int COST>
int launch_nd(const MatchParams& a, const MatchPlan& p, size_t lds, hipStream_t s) {
    if constexpr (COST == COST_HOG) {
        return launch_dpl<COST, 5>(a, p, lds, s);
    } else if constexpr (COST == COST_SAD4) {
        switch (p.ndw) {   // = r
            case 2: return launch_dpl<COST, 2>(a, p, lds, s);
            case 3: return launch_dpl<COST, 3>(a, p, lds, s);
            case 4: return launch_dpl<COST, 4>(a, p, lds, s);
            case 5: return launch_dpl<COST, 5>(a, p, lds, s);
            case 6: return launch_dpl<COST, 6>(a, p, lds, s);
            case 7: return launch_dpl<COST, 7>(a, p, lds, s);
        }
        return (int)hipErrorInvalidValue;
    } else {
        switch (p.ndw) {
            case 1: return launch_dpl<COST, 1>(a, p, lds, s);
            case 2: return launch_dpl<COST, 2>(a, p, lds, s);
            case 3: return launch_dpl<COST, 3>(a, p, lds, s);
            case 4: return launch_dpl<COST, 4>(a, p, lds, s);
        }
        return (int)hipErrorInvalidValue;
    }
}

}  // namespace

// HOG: 9 * win^2 * 255 is a deliberately loose bound.  A histogram's bins sum to at most
// win^2 * 191 (the largest magnitude), so true costs stay below 2 * win^2 * 191.
uint64_t max_cost(int win, int cost) {
    return cost == COST_SAD ? (uint64_t)win * win * 255
         : cost == COST_SSD ? (uint64_t)win * win * 255 * 255
                            : (uint64_t)9 * win * win * 255;
}

int plan_match(int num_disp, int win, int cost, MatchPlan* plan) {
    static const int menu[][2] = {{4, 16}, {6, 16}, {8, 16}, {6, 32}, {8, 32}, {6, 64}, {8, 64}};
    if (num_disp <= 0 || win < 1 || (win & 1) == 0 || win > 15) return -22;
    if (cost != COST_SAD && cost != COST_SSD && cost != COST_HOG) return -22;
    int i = 0;
    for (; i < 7; ++i)
        if (menu[i][0] * menu[i][1] >= num_disp) break;
    if (i == 7) return -22;
    plan->dpl = menu[i][0];
    plan->lpg = menu[i][1];
    const int kind = kind_of(cost, win);
    plan->ndw = kind == COST_HOG ? 5 : kind == COST_SAD4 ? win / 2
              : (win + 3) / 4;
    int n = plan->dpl * plan->lpg - 1, bits = 0;
    while (n > 0) { ++bits; n >>= 1; }
    plan->dbits = bits < 1 ? 1 : bits;
    if (hi_keys(kind, win / 2)) plan->dbits = 16;
    const uint64_t cmax = max_cost(win, cost);
    // the other kinds' keys (cost << dbits | idx) must fit 32 bits; padding disparities (idx >=
    // D) carry keys above (cmax + 1) << dbits
    const bool over = (cmax << plan->dbits) >= (1ull << 32) ||
                      (num_disp < plan->dpl * plan->lpg && cost != COST_HOG &&
                       ((2 * cmax + 2) << plan->dbits) >= (1ull << 32));
    plan->mfma_only = 0;
    if (over) {
        // SSD the matrix-core kind holds (centred keys, sv_ssd_mfma.hip): only that kind runs
        // it (launch_match refuses the call where it cannot: unaligned images)
        if (!ssd_mfma(cost, win, num_disp)) return -34;   // ERANGE: key would overflow
        plan->mfma_only = 1;
    }
    return 0;
}

size_t match_lds_bytes(const MatchPlan& p, int r, int cost) {
    const int kind = kind_of(cost, 2 * r + 1);
    const int wpb = kind == COST_SAD4 ? 1 : 4;   // (PackCfg::WPB)
    SV_MATCH_REGIONS(wave_cols(p.lpg, p.dpl, seg_mult(kind, r)), p.lpg, p.dpl, r)
    return (size_t)wpb * (NL + NRphys) * pack_shape(kind, p.ndw).slot_bytes;
}

int launch_fill_i16(int16_t* out, int opitch, int H, int W, int16_t v, hipStream_t s) {
    if (H <= 0 || W <= 0) return 0;
    hipLaunchKernelGGL(k_fill_i16, dim3((W + 255) / 256, H), dim3(256), 0, s, out, opitch, H, W, v);
    return (int)hipGetLastError();
}

bool match_is_ssd_mfma(const MatchParams& a, int cost) {
    return a.row1 > a.row0 && a.X1 > a.X0 && ssd_mfma_fits(a, cost);
}

int launch_match(const MatchParams& a, const MatchPlan& p, int cost, hipStream_t s) {
    if (a.row1 <= a.row0) return 0;
    if (a.X1 <= a.X0) {
        for (int z = 0; z < (a.nf > 1 ? a.nf : 1); ++z) {
            int e = launch_fill_i16(a.out + z * a.fs_out + (size_t)a.row0 * a.opitch, a.opitch,
                                    a.row1 - a.row0, a.W, (int16_t)((a.minD - 1) * 16), s);
            if (e) return e;
        }
        return 0;
    }
    if (match_is_ssd_mfma(a, cost)) return launch_ssd_mfma(a, s);
    if (p.mfma_only) return (int)hipErrorInvalidValue;   // no other kind holds these keys
    // (the ring kind's SAD forms need no place ahead of these two: both concern SSD alone)
    const int e = launch_match_ring(a, cost, s);
    if (e >= 0) return e;
    const size_t lds = match_lds_bytes(p, a.r, cost);
    if (lds > 160 * 1024) return (int)hipErrorInvalidValue;
    MatchParams b = a;
    b.segm = seg_mult(kind_of(cost, a.win), a.r);
    switch (kind_of(cost, a.win)) {
        case COST_SAD: return launch_nd<COST_SAD>(b, p, lds, s);
        case COST_SAD4: return launch_nd<COST_SAD4>(b, p, lds, s);
        case COST_SSD: return launch_nd<COST_SSD>(b, p, lds, s);
        case COST_HOG: return launch_nd<COST_HOG>(b, p, lds, s);
    }
    return (int)hipErrorInvalidValue;
}

}  // namespace sv
