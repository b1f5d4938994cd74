// sv_match_ring.hip — the ring kind of the matcher: SAD (and SSD) windows, four output rows
// per wave, the kernel of the metric configs.  Packs and LDS geometry: sv_match_packs.h.
//
// k_match's four-row kind (sv_match.hip) recomputes the LEAVING column's cost at every step
// (12 v_sad_hi per 4 cells).  Here each lane owns RG_DPL = 4 consecutive disparities and keeps
// the entering column's four row costs (hi-shifted, as in the key) in a register ring of W2 + 1
// = 2r+2 slots, so the leaving column's costs are read back instead of recomputed: a step costs
// 6 v_sad_hi + 4 v_sad_u32 per 4 cells (key = |key - leaving| + entering).  Both rings (the M-slot cost ring and the 4-deep right pack ring) have
// static register indices inside a body of lcm(4, M) unrolled steps.
// The first 2r steps of a segment fill the window and emit nothing: whole chunks of them run
// ahead of the loop in an add-only variant (no leaving cost, no argmin), see `chunk` below.
// Keys are (cost << 16) | idx; padding disparities (idx >= D)
// start at cost 0x8000, above every real window cost (<= 121*255 = 30855 for win 11).
#include "sv_match_packs.h"
#include "sv_xcd.h"

#include <cstdio>

namespace sv {
namespace {

// two u16 lanes of a word (v_pk_add_u16, wrapping mod 2^16)
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_add16(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, a) + __builtin_bit_cast(u16x2, b));
}

// DEFER: a chunk's second step pair is not reduced at the chunk's end (where its DPP /
// permlane chain ran alone before the next basic block) but in the next chunk's step 1,
// beside that chunk's first pair: two independent reduce-scatter chains interleaved, +9
// loop-carried VGPRs (off for r 5, which would spill).
// KEYS (split ring, D > 256): the reduced argmin keys (cost << 16 | idx) go to a.keys as u32
// (the merge kernel picks the smaller of the two passes' keys), no band-edge fill.
// SSD (r <= 4): the same packs and ring with squared differences, Σ(L-R)² = ΣL² + ΣR² - 2ΣLR
// over each output row's window column: v_dot4_u32_u8 on the common and per-row words (the
// packs' zero bytes add nothing), ΣL² once per step, ΣR² per disparity slot; the column cost
// enters pre-shifted by dbits, (ΣL² + ΣR²) << dbits - ΣLR << (dbits + 1) by one
// v_mad_i32_i24, and the window update is the same v_sad_u32.
// LDSMIN (32-lane groups, takes DEFER's place): the cross-lane fold runs through a per-wave
// LDS scratch of 8 keys x 64 lanes (2 KiB at the start of the wave's LDS) instead of the DPP
// reduce-scatter + permlane join.  A pair's 8 keys are stored as [key i][lane] (8
// ds_write_addtid_b32, consecutive lanes on consecutive banks) after its second step; at the
// top of the next step lane r loads the 8 dwords [8r, 8r + 8) = key r >> 3, group (r >> 2) & 1,
// quarter r & 3 as two ds_read_b128, folds them with 3 v_min3 + 1 v_min at that step's end
// and finishes over its quad with two quad-perm DPP mins: 6 VALU per pair.  The block is one
// wave and a wave's LDS operations complete in order, so the store -> load order in the
// program is all the synchronisation there is, and one pair's scratch serves both pairs.
// The two 16-B halves are read in the order (r >> 3) & 1 picks: within a ds_read_b128 lane
// group ({0-3,12-15,20-27}, ...) the lanes' 32-B strides then cover all 64 banks once.
// Afterwards the four lanes of quad m hold key m >> 1 of group m & 1 for both pairs; odd
// lanes take the second pair (one v_cndmask), lanes 0 and 1 of each quad emit: one store per
// chunk, one chunk late, as with DEFER.
typedef uint32_t lds_u32x4 __attribute__((ext_vector_type(4), may_alias));

template <int R, int LPGT, bool DEFER, bool KEYS, bool SSD = false, bool LDSMIN = false>
__global__ __launch_bounds__(64, 2) void k_match_ring(MatchParams a) {
    using P = PackCfg<COST_SAD4, R>;
    constexpr int NW = P::NW, NC = P::NC, W2 = 2 * R + 1;
    static_assert(!LDSMIN || (LPGT == 32 && R <= 5), "the LDS fold is laid out for two 32-lane groups of 32-bit keys");
    // PK (r 6..7): window and column costs of rows 2j, 2j+1 share a register as two u16
    // (a window costs at most 57375; v_pk_add_u16 in the warm-up, v_sad_u32 after it): 15 ring
    // steps x 16 cells fit in 120 VGPRs; the argmin keys (cost << 16) | idx are built per step
    constexpr bool PK = R >= 6;
    static_assert(P::SPLIT && (P::CW == 3) == PK, "ring kind expects split packs (20 B for r 2..3, 24 B for r 4..5, 28 B for r 6..7)");
    extern __shared__ __attribute__((aligned(16))) uint4 smem[];
    // XCD-aware tile order (sv_xcd.h): horizontal and vertical neighbours share 2r of their
    // 2r+4 input rows and most right-image columns; each XCD takes a contiguous tile range
    int bx, by, bz;
    xcd_tile(a.xcd_map != 0, bx, by, bz);
    if (bz) {   // frame batch
        a.L += bz * a.fs_in;
        a.R += bz * a.fs_in;
        a.out += bz * a.fs_out;
        if constexpr (KEYS) a.keys += bz * a.fs_out;
    }
    const int lane = threadIdx.x;
    constexpr int LPG = LPGT;                           // lanes per group (template: no
                                                        // branches between the steps)
    const int S = a.segm;                               // segment width per group (multiple of 4)
    // The window update is ONE v_sad_u32 (key - leaving + entering), which reads the leaving
    // column's cost after the entering one is computed, so the two cannot share a register: the
    // cost ring has M = W2 + 1 slots (the entering cost goes to the slot whose value left the
    // window one step earlier) and keeps static register names.  r 5 fits its 16 more ring
    // VGPRs without the left-pack prefetch (LPF below).
    // PK: the two u16 halves of a cost word update as ONE 32-bit v_sad_u32 as well: each half
    // of the key holds its leaving cost as a summand, so key >= leaving as 32-bit integers with
    // no borrow between the halves, and key - leaving + entering stays below 2^16 per half (no
    // carry): the packed result is exact.
    constexpr int M = W2 + 1;                           // cost ring slots
    constexpr int U = M % 4 == 0 ? M : M % 2 == 0 ? 2 * M : 4 * M;   // lcm(4, M) steps per body
    constexpr int NCH = U / 4;                          // chunks per body
    // steps per segment: S outputs + 2r warm-up, in chunks of 4; whole bodies of U steps,
    // the first body entered at chunk e0 (its first e0 chunks skipped)
    SV_RING_GEOM(LPG, S, R)
    constexpr int c0 = RING_C0;
    const int nit = (Tn + U - 1) / U;
    const int e0 = (nit * U - Tn) >> 2;
    uint4* wbase = smem + ring_scratch_bytes(LDSMIN) / 16;   // the packs follow the scratch
    typename P::CT* cbase = reinterpret_cast<typename P::CT*>(wbase + (size_t)slots);
    const PackOut<COST_SAD4, R> Lw{wbase + RING_PAD_F, cbase + RING_PAD_F};
    const PackOut<COST_SAD4, R> Rw{wbase + NL + RING_PAD_F + RING_PAD_M, cbase + NL + RING_PAD_F + RING_PAD_M};
    const PackPtr<COST_SAD4, R> Lp{Lw.x, Lw.c};
    const PackPtr<COST_SAD4, R> Rp{Rw.x, Rw.c};

    const int y = a.row0 + by * 4;
    const int yc = min(y, a.row1 - 1);
    const int xw = a.X0 + bx * WC;
    const int cL0 = xw - R;                             // L index i -> column cL0 + i
    const int cR0 = cL0 - a.minD - (4 * LPG - 1);       // R index i -> column cR0 + i
    build_ring_packs<R, 3, RG_DPL>(a, yc, cL0, NL, cR0, NRlog, c0, Lw, Rw, lane);

    // columns outside the matched band are invalid (margins_done: an earlier launch into the
    // same map left them so, see MatchParams)
    if (!KEYS && bx == 0 && !a.margins_done) {
        const int16_t inv = (int16_t)((a.minD - 1) * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (y + q >= a.row1) break;
            int16_t* orow = a.out + (size_t)(y + q) * a.opitch;
            for (int x = lane; x < a.X0; x += 64) orow[x] = inv;
            for (int x = a.X1 + lane; x < a.W; x += 64) orow[x] = inv;
        }
    }
    __syncthreads();
    if (y >= a.row1) return;

    const int g = lane / LPG;
    const int l = lane & (LPG - 1);
    const int xs = xw + g * S;                          // first output column of the segment
    // step t enters column xs - r + t; lane l, disparity idx 4l + k reads R index iR0 + t - k
    // r <= 5: padding disparities (idx >= D) start at cost 0x8000, above any real window.
    // r 6..7 (window costs up to 57375, no headroom; D a multiple of 4): padding lanes
    // re-match the last real group D-4..D-1 under their own, larger labels, so on equal
    // costs the real lane wins every tie
    const int dl = PK ? min(4 * l, a.D - 4) : 4 * l;
    const int iR0 = g * S + 4 * (LPG - 1) - dl + 3;
    constexpr int RQ = PK ? 2 : 4;                      // cost words per k (h and ring slots)
    uint32_t h[RG_DPL][RQ], lab[RG_DPL];
#pragma unroll
    for (int k = 0; k < RG_DPL; ++k) {
        const int idx = 4 * l + k;
        const uint32_t base = PK ? 0u : idx < a.D ? (uint32_t)idx : (SSD ? a.pad_key : 0x8000u << 16) | (uint32_t)idx;
        lab[k] = (uint32_t)idx;
#pragma unroll
        for (int q = 0; q < RQ; ++q) h[k][q] = base;
    }
    // No slot is read before a step has written it or the last warm-up chunk has zeroed it
    // (below), so the ring starts with whatever its registers hold: the empty asm gives every
    // element a defined value at no instruction (M * 16 v_mov per wave otherwise).
    uint32_t ring[M][RG_DPL][RQ];
#pragma unroll
    for (int s = 0; s < M; ++s)
#pragma unroll
        for (int k = 0; k < RG_DPL; ++k)
#pragma unroll
            for (int q = 0; q < RQ; ++q) asm volatile("" : "=v"(ring[s][k][q]));
    Pk<NW> rn[RG_DPL];
#pragma unroll
    for (int s = 1; s < RG_DPL; ++s) rn[RG_DPL - s] = ld<COST_SAD4, R, true>(Rp + rslot(iR0 - s, c0, RG_DPL));
    // pointers of body position 0 (chunk e0 of the first body is step 0; the skipped chunks'
    // offsets are never dereferenced)
    PackPtr<COST_SAD4, R> rb = Rp + (rslot(iR0, c0, RG_DPL) - e0 * (RG_DPL + 1));
    PackPtr<COST_SAD4, R> lb = Lp + (g * S - 4 * e0);
    // LPF: the left pack is loaded one step ahead (off for r 5, whose 32-lane body is 4 VGPRs
    // over the 256 a wave of two per SIMD may hold: the 6 registers of the prefetched pack take
    // its spills out of the loop)
    constexpr bool LPF = R != 5;
    Pk<NW> Lnext = ld<COST_SAD4, R, true>(lb + 4 * e0);
    // after the reduce-scatter lane l's key is (row jq, step ju) of the chunk; the first 16
    // lanes of a group emit
    // (32-bit per-lane state only: output offset of step 0 and the emit window)
    const int jq = (lane >> 2) & 3, ju = (lane >> 1) & 1;   // key (l >> 1) & 7 = 2 jq + ju
    // 32-lane groups (D 65..128) join the two DPP rows of a chunk's two step pairs with ONE
    // v_permlane16_swap of the pairs' keys (instead of a mov + swap + min per pair): the
    // rows then hold different pairs, and both rows emit.  Which row receives which pair is
    // read off the swap itself once (pofs = the step offset of the lane's pair in its chunk,
    // folded into eb).  64-lane groups (D 129..256) do the same and then join the wave's
    // halves with one v_permlane32_swap; rows 0 and 1 emit.  (r 5 fits it since LPG is a
    // template parameter and the body has no branches: 244 VGPRs; with a runtime LPG and
    // branches around the reductions the allocator spilled ~1,000.)
    constexpr bool join2 = LPG >= 32;
    int pofs = 0;
    if (join2 && !LDSMIN) {
        const auto p = __builtin_amdgcn_permlane16_swap((uint32_t)lane, (uint32_t)lane + 64u, false, false);
        // min(p[0], p[1]) of a lane comes from the first operand's values iff both p[k] < 64
        pofs = (max(p[0], p[1]) < 64u) ? 0 : 2;
    }
    // step t emits column xs + t + eb (join2: the chunk starting at step t emits the lane's
    // pair at column xs + t + eb)
    // LDSMIN: lane r emits row r >> 4, step (r >> 3) & 1 of pair r & 1, for the segment of
    // group (r >> 2) & 1 (not the group whose costs it computes)
    const int eq = LDSMIN ? lane >> 4 : jq;
    const int exs = LDSMIN ? xw + ((lane >> 2) & 1) * S : xs;
    const int eb = (LDSMIN ? ((lane >> 3) & 1) + 2 * (lane & 1) : ju + pofs) - 2 * R;
    constexpr int OB = KEYS ? 4 : 2;                        // bytes per output element
    const int ooff = OB * ((y + eq) * a.opitch + exs + eb);   // bytes
    // 32-bit buffer offsets from one SGPR descriptor (no 64-bit per-lane addresses to keep)
    const auto orsrc = KEYS ? __builtin_amdgcn_make_buffer_rsrc(a.keys, 0, 0x7FFFFFFF, 0x00020000)
                            : __builtin_amdgcn_make_buffer_rsrc(a.out, 0, 0x7FFFFFFF, 0x00020000);
    const int emax = (LDSMIN ? (lane & 2) == 0 && y + eq < a.row1
                             : (l & 1) == 0 && l < (join2 ? 32 : 16) && y + jq < a.row1)
                         ? max(0, min(S, a.X1 - exs)) : 0;

    // store of a reduced key for the chunk starting at step tt (join2) / of step tt
    auto emit_key = [&](uint32_t key, int tt) {
        // non-emitting lanes store past the buffer's range (dropped by the hardware bounds
        // check, as in composable_kernel): no exec-mask branch
        const int off = (unsigned)(tt + eb) < (unsigned)emax ? ooff + OB * tt : (int)0x80000000u;
        if constexpr (KEYS) __builtin_amdgcn_raw_buffer_store_b32(key, orsrc, off, 0, 0);
        else __builtin_amdgcn_raw_buffer_store_b16(
            (uint16_t)key_disp16(key, SSD ? (1u << a.dbits) - 1u : 0xFFFFu, a.minD), orsrc, off, 0, 0);
    };
    // join2: pair (0,1) in kA, pair (2,3) in kB: one swap joins both
    auto join_pairs = [&](uint32_t kA_, uint32_t kB_) {
        auto p = __builtin_amdgcn_permlane16_swap(kA_, kB_, false, false);
        uint32_t key = min(p[0], p[1]);
        if (LPG == 64) {   // rows 0 and 2 hold the same pair (1 and 3 the other)
            p = __builtin_amdgcn_permlane32_swap(key, key, false, false);
            key = min(p[0], p[1]);
        }
        return key;
    };
    auto join_rows = [&](uint32_t key) {   // !join2: a pair's key over the group's DPP rows
        if (LPG >= 32) {   // rows 0,1 (and 2,3) of the wave: min with lane ^ 16
            const auto p = __builtin_amdgcn_permlane16_swap(key, key, false, false);
            key = min(p[0], p[1]);
        }
        if (LPG == 64) {   // halves: min with lane ^ 32
            const auto p = __builtin_amdgcn_permlane32_swap(key, key, false, false);
            key = min(p[0], p[1]);
        }
        return key;
    };
    // DEFER state: the previous chunk's second pair (8 keys), its first pair's reduced key
    // and its first step (a first chunk has none: the sentinel step stores out of range)
    uint32_t dv[8], kA = 0xFFFFFFFFu;
    int tprev = -(1 << 24);
#pragma unroll
    for (int i = 0; i < 8; ++i) dv[i] = 0xFFFFFFFFu;
    // LDSMIN: the scratch as dwords; a lane stores at scr[64 i + lane] and loads its two
    // 16-B halves at sra and srb (byte offsets 32 lane + 16 s and 32 lane + 16 (1 - s))
    [[maybe_unused]] uint32_t* const scr = reinterpret_cast<uint32_t*>(smem);
    // the scratch's LDS byte address (wave-uniform), the M0 base of the addtid stores
    [[maybe_unused]] const uint32_t scr_m0 = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t*)scr);
    [[maybe_unused]] const lds_u32x4* const sra = reinterpret_cast<const lds_u32x4*>(scr + 8 * lane + 4 * ((lane >> 3) & 1));
    [[maybe_unused]] const lds_u32x4* const srb = reinterpret_cast<const lds_u32x4*>(scr + 8 * lane + 4 * (1 - ((lane >> 3) & 1)));
    auto lds_fold = [&](const lds_u32x4& p, const lds_u32x4& s) {
        uint32_t m = min(min(p.x, p.y), p.z);
        m = min(min(m, p.w), s.x);
        m = min(min(m, s.y), s.z);
        m = min(m, s.w);
        m = min(m, (uint32_t)__builtin_amdgcn_update_dpp(0u, (int)m, 0xB1, 0xF, 0xF, false));   // l ^ 1
        return min(m, (uint32_t)__builtin_amdgcn_update_dpp(0u, (int)m, 0x4E, 0xF, 0xF, false));   // l ^ 2
    };
    [[maybe_unused]] const bool pairB = (lane & 1) != 0;

    // One chunk (4 steps) at body position ch, first step t0, in two compile-time variants.
    // WARM: all four steps lie in the warm-up (t0 + 3 < 2r).  Their argmins would be emitted
    // out of range and the costs leaving their windows are the ring's initial zeros, so the
    // variant only adds the entering costs to the keys and files them in the ring (the same
    // static slots and right-pack names as the normal variant of this position): no read of
    // the ring, no min, no fold, no scratch traffic, no store.  tprev, kA and dv keep their
    // sentinels, so the first normal chunk is the sentinel first chunk.  The last warm-up
    // chunk zeroes the slots that steps 4*nwarm .. 2r read before any step has written them
    // (one step's slot for even r, three for odd r); warm-up steps that share a chunk with
    // output steps (step 8 at r 4) run in the normal variant against those zeros.
    constexpr int NZ = 2 * R - 4 * (2 * R / 4) + 1;
    auto chunk = [&](auto warm_c, const int ch, const int t0) __attribute__((always_inline)) {
            constexpr bool WARM = decltype(warm_c)::value;
            [[maybe_unused]] uint32_t bk[4][2];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                // the entering cost goes to `slot`, the leaving one (entered W2 steps ago)
                // is read from `oslot`
                const int slot = (4 * ch + u) % M, oslot = (4 * ch + u + 1) % M;
                // this step's packs: L (every k) and the entering right column (k = 0 only)
                rn[u] = ld<COST_SAD4, R, true>(rb + (ch * (RG_DPL + 1) + u));
                const Pk<NW> Lc = LPF ? Lnext : ld<COST_SAD4, R, true>(lb + (4 * ch + u));
                if constexpr (LPF) Lnext = ld<COST_SAD4, R, true>(lb + (4 * ch + u + 1));
                // LDSMIN: the pair stored after the previous step (u 0: the previous chunk's
                // second pair, or stale scratch before the first chunk), folded below
                lds_u32x4 fa{}, fb{};
                if constexpr (LDSMIN && !WARM) {
                    if ((u & 1) == 0) { fa = *sra; fb = *srb; }
                }
                // SSD: ΣL² of this step's left pack per output row, pre-shifted by dbits
                uint32_t sqL[4];
                if constexpr (SSD) {
                    uint32_t sc = 0u;
#pragma unroll
                    for (int i = 0; i < NC; ++i) sc = __builtin_amdgcn_udot4(Lc.w[i], Lc.w[i], sc, false);
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        sqL[q] = __builtin_amdgcn_udot4(Lc.w[NC + q], Lc.w[NC + q], sc, false) << a.dbits;
                }
                // k = 0 (the fresh right pack) last
#pragma unroll
                for (int kk = 0; kk < RG_DPL; ++kk) {
                    const int k = RG_DPL - 1 - kk;
                    const Pk<NW>& Rk = rn[(u - k) & 3];
                    if constexpr (PK) {
                        // common rows once, in both halves; row 2j's sad in the low half,
                        // row 2j+1's in the high half
                        uint32_t cn = 0u;
#pragma unroll
                        for (int i = 0; i < NC; ++i) cn = __builtin_amdgcn_sad_u8(Lc.w[i], Rk.w[i], cn);
                        cn |= cn << 16;
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const uint32_t c = __builtin_amdgcn_sad_hi_u8(
                                Lc.w[NC + 2 * j + 1], Rk.w[NC + 2 * j + 1],
                                __builtin_amdgcn_sad_u8(Lc.w[NC + 2 * j], Rk.w[NC + 2 * j], cn));
                            if constexpr (!WARM) sad_u32_acc(h[k][j], ring[oslot][k][j], c);
                            else h[k][j] = pk_add16(h[k][j], c);
                            ring[slot][k][j] = c;
                        }
                    } else if constexpr (SSD) {
                        uint32_t cn = 0u, sr = 0u;
#pragma unroll
                        for (int i = 0; i < NC; ++i) {
                            cn = __builtin_amdgcn_udot4(Lc.w[i], Rk.w[i], cn, false);
                            sr = __builtin_amdgcn_udot4(Rk.w[i], Rk.w[i], sr, false);
                        }
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const uint32_t lr = __builtin_amdgcn_udot4(Lc.w[NC + q], Rk.w[NC + q], cn, false);
                            const uint32_t rr = __builtin_amdgcn_udot4(Rk.w[NC + q], Rk.w[NC + q], sr, false);
                            const uint32_t t = (rr << a.dbits) + sqL[q];
                            const uint32_t c = (uint32_t)__mul24((int)lr, -(2 << a.dbits)) + t;
                            if constexpr (WARM) h[k][q] += c;
                            else sad_u32_acc(h[k][q], ring[oslot][k][q], c);
                            ring[slot][k][q] = c;
                        }
                    } else {
                        uint32_t cn = 0u;
#pragma unroll
                        for (int i = 0; i < NC; ++i) cn = __builtin_amdgcn_sad_hi_u8(Lc.w[i], Rk.w[i], cn);
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const uint32_t c = __builtin_amdgcn_sad_hi_u8(Lc.w[NC + q], Rk.w[NC + q], cn);
                            // key - leaving + entering as ONE v_sad_u32 (|key - leaving|
                            // + entering): the key holds the leaving column's cost as one of
                            // its summands, so key >= leaving and the absolute value is the
                            // plain difference (one VOP3 instead of a VOP2 sub + add)
                            if constexpr (!WARM) sad_u32_acc(h[k][q], ring[oslot][k][q], c);
                            else h[k][q] += c;
                            ring[slot][k][q] = c;
                        }
                    }
                }
                if constexpr (WARM) {
                    __builtin_amdgcn_sched_barrier(0);
                    continue;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    uint32_t kq[RG_DPL];
#pragma unroll
                    for (int k = 0; k < RG_DPL; ++k)
                        kq[k] = !PK ? h[k][q] : (q & 1) ? (h[k][q >> 1] & 0xFFFF0000u) | lab[k] : (h[k][q >> 1] << 16) | lab[k];
                    bk[q][u & 1] = min(min(kq[0], kq[1]), min(kq[2], kq[3]));
                }
                if constexpr (LDSMIN) {
                    if (u == 2) {
                        kA = lds_fold(fa, fb);
                    } else if (u == 0) {   // the previous chunk is complete: one store for its 4 steps
                        const uint32_t kB = lds_fold(fa, fb);
                        emit_key(pairB ? kB : kA, tprev);
                        tprev = t0;
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (LDSMIN) {
                    if (u & 1) {   // steps u-1, u: key (row q, step j) of every lane to scr[2q + j][lane]
                        // ds_write_addtid_b32 (address = M0 + offset + 4 lane: the scratch's own
                        // layout) sends one data VGPR and no address per store, 8 dwords per
                        // pair instead of the 12 of four ds_write2st64_b32 (which gave back most
                        // of the fold's gain); no builtin has it.  The compiler's
                        // lgkmcnt counts do not see these stores: LDS returns in order, so each
                        // count still waits for at least what it meant to
                        asm volatile("s_mov_b32 m0, %8\n\t"
                                     "s_nop 0\n\t"   // SALU write of M0 -> LDS add-TID: 1 wait state
                                     "ds_write_addtid_b32 %0\n\t"
                                     "ds_write_addtid_b32 %1 offset:256\n\t"
                                     "ds_write_addtid_b32 %2 offset:512\n\t"
                                     "ds_write_addtid_b32 %3 offset:768\n\t"
                                     "ds_write_addtid_b32 %4 offset:1024\n\t"
                                     "ds_write_addtid_b32 %5 offset:1280\n\t"
                                     "ds_write_addtid_b32 %6 offset:1536\n\t"
                                     "ds_write_addtid_b32 %7 offset:1792\n\t"
                                     :
                                     : "v"(bk[0][0]), "v"(bk[0][1]), "v"(bk[1][0]), "v"(bk[1][1]), "v"(bk[2][0]),
                                       "v"(bk[2][1]), "v"(bk[3][0]), "v"(bk[3][1]), "s"(scr_m0)
                                     : "memory", "m0");
                        // wavefront scope: no instruction, keeps the next step's loads below
                        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                    }
                    continue;
                }
                // steps u-1, u: 8 keys (row q, step j) at v[2q + j].  Warm-up pairs are reduced
                // too (their keys are not emitted): no branch, so a chunk is one basic block and
                // the scheduler can interleave a reduction's DPP / permlane chain with the next
                // step's independent cost work
                if (DEFER && u == 3) {   // the second pair waits for the next chunk
#pragma unroll
                    for (int i = 0; i < 8; ++i) dv[i] = bk[i >> 1][i & 1];
                } else if (DEFER && u == 1) {   // this chunk's first pair + the previous chunk's second
                    uint32_t v[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[i] = bk[i >> 1][i & 1];
                    reduce_scatter8_bm(v, lane & 15);
                    reduce_scatter8_bm(dv, lane & 15);
                    if (join2) {
                        emit_key(join_pairs(kA, dv[0]), tprev);
                        kA = v[0];
                    } else {
                        emit_key(join_rows(dv[0]), tprev + 2);
                        emit_key(join_rows(v[0]), t0);
                    }
                    tprev = t0;
                } else if (u & 1) {
                    uint32_t v[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[i] = bk[i >> 1][i & 1];
                    reduce_scatter8_bm(v, lane & 15);
                    if (join2) {
                        if (u == 1) kA = v[0];
                        else emit_key(join_pairs(kA, v[0]), t0);
                    } else {
                        emit_key(join_rows(v[0]), t0 + u - 1);
                    }
                }
            }
            if constexpr (WARM) {
                if (t0 + 7 >= 2 * R) {   // the last warm-up chunk
#pragma unroll
                    for (int i = 0; i < NZ; ++i)
#pragma unroll
                        for (int k = 0; k < RG_DPL; ++k)
#pragma unroll
                            for (int q = 0; q < RQ; ++q) ring[(4 * ch + 5 + i) % M][k][q] = 0u;
                }
            }
    };
    // The warm-up chunks run ahead of the loop, one copy per entry chunk e0 (positions past
    // the body's end are the second body's: same slot names, since U is a multiple of M, and
    // the pointers are body 0's).  Inside the loop a third path per chunk made LLVM copy the
    // keys and the pack rings at every merge.
    constexpr int NWARM = 2 * R / 4;
#pragma unroll
    for (int e = 0; e < NCH; ++e) {
        if (e != e0) continue;               // (uniform)
#pragma unroll
        for (int i = 0; i < NWARM; ++i) chunk(std::true_type{}, e + i, 4 * i);
    }
    // whole bodies of U = 4*W2 steps, no exits inside a body (an exit per chunk made LLVM
    // shuffle the rings); the first body skips its first e0 chunks by a uniform branch
    for (int it = 0, t0 = -4 * e0; it < nit; ++it) {
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch, t0 += 4) {
            if (t0 < 4 * NWARM) continue;    // skipped and warm-up chunks of the first bodies (uniform)
            chunk(std::false_type{}, ch, t0);
        }
        rb = rb + NCH * (RG_DPL + 1);
        lb = lb + U;
    }
    if constexpr (LDSMIN) {   // the last chunk's second pair and store
        const uint32_t kB = lds_fold(*sra, *srb);
        emit_key(pairB ? kB : kA, tprev);
    } else if (DEFER) {   // the last chunk's second pair
        reduce_scatter8_bm(dv, lane & 15);
        if (join2) emit_key(join_pairs(kA, dv[0]), tprev);
        else emit_key(join_rows(dv[0]), tprev + 2);
    }
}

// Ring kind eligibility and geometry.  SV_RING=0 disables it (A/B measurements);
bool ring_kind(int cost, int win, int num_disp) {
    static const bool on = env_flag("SV_RING", true);
    return on && kind_of(cost, win) == COST_SAD4 && win >= 5 && num_disp <= 256 &&
           (win <= 11 || (win <= 15 && num_disp % 4 == 0));
}
int ring_lpg(int num_disp) { return num_disp <= 64 ? 16 : num_disp <= 128 ? 32 : 64; }
// LDS argmin fold (k_match_ring's LDSMIN): 32-lane groups at r 4, the SAD ring's disparity
// output.  SV_RING_LDSMIN=0 (A/B) restores the DPP reduce-scatter.  Its 2 KiB scratch counts
// in the wave's LDS: 1080p D=128 win 9 takes 18,144 + 2,048 = 20,192 B, still 8 waves per CU
// (profiles/r07_ldsmin).
bool ring_ldsmin(int lpg, int r, bool keys, bool ssd) {
    static const bool on = env_flag("SV_RING_LDSMIN", true);
    return on && lpg == 32 && r == 4 && !keys && !ssd;
}
size_t ring_lds_bytes(int lpg, int seg, int r, bool ldsmin) {
    SV_RING_GEOM(lpg, seg, r)
    return (size_t)slots * pack_shape(COST_SAD4, r).slot_bytes + ring_scratch_bytes(ldsmin);
}
// Segment width per group: S (a multiple of 4) minimising the steps all waves of a row
// run, ceil(band / (G*S)) * (S + 2r) (idle columns of the last wave + the 2r warm-up steps
// of every segment), among segments whose LDS leaves room for 2 waves per SIMD; ties go to
// the longer segment.  SV_RING_SEG=<S> forces a width (A/B measurements).
int ring_seg(int lpg, int r, int band, bool ldsmin) {
    static const int env = [] {
        const int v = env_int("SV_RING_SEG", 8, 1024);
        return v % 4 == 0 ? v : 0;
    }();
    if (env) return env;
    const int G = 64 / lpg;
    int best = 8;
    long long best_cost = -1;
    for (int S = 8; S <= 1024; S += 4) {
        if (S > 8 && ring_lds_bytes(lpg, S, r, ldsmin) > 20 * 1024) break;
        SV_RING_GEOM(lpg, S, r)
        const long long cost = (long long)((band + G * S - 1) / (G * S)) * Tn;
        if (best_cost < 0 || cost <= best_cost) { best = S; best_cost = cost; }
    }
    return best;
}

template <int R, int LPG, bool KEYS, bool SSD>
int launch_ring_rl(const MatchParams& a, size_t lds, bool ldsmin, hipStream_t s) {
    // SV_RING_DEFER=0 (A/B): every pair reduced inside its own chunk
    static const bool defer = env_flag("SV_RING_DEFER", true);
    void (*fn)(MatchParams);
    if constexpr (SSD) fn = k_match_ring<R, LPG, R != 5, false, true>;
    else if constexpr (KEYS) fn = k_match_ring<R, LPG, R != 5, true>;
    else fn = (defer && R != 5) ? k_match_ring<R, LPG, R != 5, false> : k_match_ring<R, LPG, false, false>;
    if constexpr (R == 4 && LPG == 32 && !KEYS && !SSD) {
        if (ldsmin) fn = k_match_ring<R, LPG, false, false, false, true>;
    }
    if (lds > 65536) {
        hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    const int wc = (64 / a.lpg) * a.segm;
    dim3 grid((a.X1 - a.X0 + wc - 1) / wc, (a.row1 - a.row0 + 3) / 4, a.nf > 1 ? a.nf : 1);
    // SV_RING_OCC=1: print every ring launch's resident waves per CU at its LDS size
    static const bool occ = env_flag("SV_RING_OCC", false);
    if (occ) {
        int nb = -1;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)fn, 64, lds);
        std::fprintf(stderr, "k_match_ring r=%d lpg=%d ldsmin=%d seg=%d lds=%zu B: %d waves/CU\n", R, LPG,
                     (int)ldsmin, a.segm, lds, nb);
    }
    // SV_XCD_MAP=0 (A/B): tiles in plain dispatch order
    static const bool xcd = env_flag("SV_XCD_MAP", true);
    MatchParams b = a;
    b.xcd_map = xcd ? 1 : 0;
    hipLaunchKernelGGL(fn, grid, dim3(64), lds, s, b);
    return (int)hipGetLastError();
}
template <int R, bool KEYS, bool SSD = false>
int launch_ring_r(const MatchParams& a, size_t lds, bool ldsmin, hipStream_t s) {
    switch (a.lpg) {
        case 16: return launch_ring_rl<R, 16, KEYS, SSD>(a, lds, ldsmin, s);
        case 32: return launch_ring_rl<R, 32, KEYS, SSD>(a, lds, ldsmin, s);
        case 64: return launch_ring_rl<R, 64, KEYS, SSD>(a, lds, ldsmin, s);
    }
    return (int)hipErrorInvalidValue;
}

template <bool KEYS, bool SSD = false>
int launch_ring(const MatchParams& a0, hipStream_t s) {
    MatchParams a = a0;
    a.lpg = ring_lpg(a.D);
    a.lpg_log2 = a.lpg == 16 ? 4 : a.lpg == 32 ? 5 : 6;
    a.dbits = SSD ? a.lpg_log2 + 2 : 16;   // SSD keys: (cost << log2(4 LPG)) | idx
    if (SSD) a.pad_key = (uint32_t)((max_cost(a.win, COST_SSD) + 1) << a.dbits);
    const bool ldsmin = ring_ldsmin(a.lpg, a.r, KEYS, SSD);
    a.segm = ring_seg(a.lpg, a.r, a.X1 - a.X0, ldsmin);
    const size_t lds = ring_lds_bytes(a.lpg, a.segm, a.r, ldsmin);
    if (lds > 160 * 1024) return (int)hipErrorInvalidValue;
    if constexpr (SSD) {
        switch (a.r) {
            case 2: return launch_ring_r<2, false, true>(a, lds, ldsmin, s);
            case 3: return launch_ring_r<3, false, true>(a, lds, ldsmin, s);
            case 4: return launch_ring_r<4, false, true>(a, lds, ldsmin, s);
        }
        return (int)hipErrorInvalidValue;
    } else {
        switch (a.r) {
            case 2: return launch_ring_r<2, KEYS>(a, lds, ldsmin, s);
            case 3: return launch_ring_r<3, KEYS>(a, lds, ldsmin, s);
            case 4: return launch_ring_r<4, KEYS>(a, lds, ldsmin, s);
            case 5: return launch_ring_r<5, KEYS>(a, lds, ldsmin, s);
            case 6: return launch_ring_r<6, KEYS>(a, lds, ldsmin, s);
            case 7: return launch_ring_r<7, KEYS>(a, lds, ldsmin, s);
        }
        return (int)hipErrorInvalidValue;
    }
}

// Split ring merge: per pixel the smaller of the two passes' keys (pass B's indices shifted
// past pass A's 256: on equal costs pass A's smaller disparity wins, the first minimum), and
// the band-edge columns' invalid value.  4 pixels per thread (16-B key loads, one 8-B store)
// when the pitch, frame stride and map allow it.
__device__ __forceinline__ int16_t merge_px(uint32_t ka, uint32_t kb, int x, int X0, int X1, int minD) {
    const uint32_t k = min(ka, kb + 256u);
    return (int16_t)(x >= X0 && x < X1 ? ((int)(k & 0xFFFFu) + minD) * 16 : (minD - 1) * 16);
}
__global__ __launch_bounds__(256) void k_merge_ring_keys(const uint32_t* __restrict__ ka,
                                                         const uint32_t* __restrict__ kb, int16_t* __restrict__ out,
                                                         int opitch, long long fs_out, int row0, int W, int X0, int X1,
                                                         int minD, int vec) {
    const int x = 4 * (int)(blockIdx.x * 256 + threadIdx.x);
    if (x >= W) return;
    const size_t i = (size_t)blockIdx.z * fs_out + (size_t)(row0 + (int)blockIdx.y) * opitch + x;
    if (vec && x + 4 <= W) {
        const uint4 a = *reinterpret_cast<const uint4*>(ka + i);
        const uint4 b = *reinterpret_cast<const uint4*>(kb + i);
        const uint32_t lo = (uint16_t)merge_px(a.x, b.x, x, X0, X1, minD) |
                            ((uint32_t)(uint16_t)merge_px(a.y, b.y, x + 1, X0, X1, minD) << 16);
        const uint32_t hi = (uint16_t)merge_px(a.z, b.z, x + 2, X0, X1, minD) |
                            ((uint32_t)(uint16_t)merge_px(a.w, b.w, x + 3, X0, X1, minD) << 16);
        *reinterpret_cast<uint2*>(out + i) = make_uint2(lo, hi);
        return;
    }
    for (int q = 0; q < 4 && x + q < W; ++q) out[i + q] = merge_px(ka[i + q], kb[i + q], x + q, X0, X1, minD);
}

}  // namespace

// D in (256, 512]: the ring kind twice, d in [0, 256) (64-lane groups) and [256, D) (its
// own group width), each into a key plane, then k_merge_ring_keys — the four-row kind it
// replaces ran 2.3x slower per cell (1080p D=320 w7: 2,322 us per 16 frames against 805 for
// D=256, round 4)
// SSD windows 5..9 with D <= 256 take the ring kind's SSD form when the keys (cost << dbits |
// idx, padding lanes above every real key) fit 32 bits
bool ring_ssd(int cost, int win, int num_disp) {
    if (cost != COST_SSD || win < 5 || win > 9 || num_disp < 1 || num_disp > 256) return false;
    if (!ring_kind(COST_SAD, win, num_disp)) return false;   // (SV_RING=0 switches it off too)
    const int lpg = ring_lpg(num_disp), dbits = (lpg == 16 ? 4 : lpg == 32 ? 5 : 6) + 2;
    const uint64_t cmax = max_cost(win, COST_SSD);
    const uint64_t top = num_disp < 4 * lpg ? (2 * cmax + 2) << dbits : (cmax << dbits) + (uint64_t)(4 * lpg);
    return top < (1ull << 32);
}
bool ring_split(int cost, int win, int num_disp) {
    return num_disp > 256 && num_disp <= 512 && ring_kind(cost, win, 256) && ring_kind(cost, win, num_disp - 256);
}
long long ring_split_elems(int nf, long long fs_out, int row1, int opitch) {
    return ((long long)(nf > 1 ? nf - 1 : 0) * fs_out + (long long)(row1 + 3) * opitch + 64 + 3) & ~3LL;
}

int launch_match_ring(const MatchParams& a, int cost, hipStream_t s) {
    // the ring kind stores through one buffer descriptor with 32-bit byte offsets
    // (2 * (row * out_pitch + x) per frame); maps whose last row lies past 2^31 bytes take
    // k_match's size_t-addressed four-row kind instead
    const bool ring_fits = 2LL * ((long long)(a.row1 + 3) * a.opitch + a.W + 64) < 0x7FFFFFFFLL;
    if (ring_kind(cost, a.win, a.D) && ring_fits) return launch_ring<false>(a, s);
    if (ring_ssd(cost, a.win, a.D) && ring_fits) return launch_ring<false, true>(a, s);
    if (ring_split(cost, a.win, a.D) && a.keys) {
        // (key planes: 4-byte elements, so half the 2^31-byte range of the int16 maps)
        if (4LL * ((long long)(a.row1 + 3) * a.opitch + a.W + 64) >= 0x7FFFFFFFLL) return (int)hipErrorInvalidValue;
        MatchParams pa = a, pb = a;
        pa.D = 256;
        pb.minD = a.minD + 256;
        pb.D = a.D - 256;
        pb.keys = a.keys + a.keys_stride;
        int e = launch_ring<true>(pa, s);
        if (!e) e = launch_ring<true>(pb, s);
        if (e) return e;
        const int nf = a.nf > 1 ? a.nf : 1;
        const long long fso = nf > 1 ? a.fs_out : 0LL;
        const int vec = (a.opitch % 4 == 0 && fso % 4 == 0 && a.keys_stride % 4 == 0 &&
                         ((uintptr_t)a.out & 7) == 0 && ((uintptr_t)a.keys & 15) == 0) ? 1 : 0;
        hipLaunchKernelGGL(k_merge_ring_keys, dim3((a.W + 1023) / 1024, a.row1 - a.row0, nf), dim3(256), 0, s, pa.keys,
                           pb.keys, a.out, a.opitch, fso, a.row0, a.W, a.X0, a.X1, a.minD, vec);
        return (int)hipGetLastError();
    }
    return -1;
}

}  // namespace sv
