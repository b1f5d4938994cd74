// sv_match_packs.h — what the matcher's two kernel files share (sv_match.hip: k_match,
// sv_match_ring.hip: k_match_ring): the column packs' shape and their builders, the per-wave
// LDS geometry of both kernels (one definition for the kernel and for the host's byte count),
// the 8-key reduce-scatter, and a few small device and host helpers.
#pragma once
#include "sv_internal.h"

#include <cstdlib>
#include <type_traits>

namespace sv {

constexpr int COST_SAD4 = 4;          // internal kind: SAD, four output rows per wave

// Kind actually launched for a public cost: SAD with win >= 5 runs four rows per wave.
inline int kind_of(int cost, int win) { return cost == COST_SAD && win >= 5 ? COST_SAD4 : cost; }

// ---- pack shape --------------------------------------------------------------------------
// A column pack holds `nw` live dwords.  `nd` is the kind's width parameter: byte dwords (SAD,
// SSD), unused (HOG), the window radius r (SAD4: ceil((2r-2)/4) common dwords + 4 per-row
// dwords).  Unsplit packs take a 16*q-byte slot of the main array.  Split packs keep their `nc`
// common words in a separate array of `cw`-word slots and 4 words in a 16-byte slot:
//   * the 4-row kind: 20-B packs for r 2..3 (one common word, a 4-byte slot), 24 B for r 4..5
//     (instead of a 32-byte slot, so a 4-LPG segment still fits 2 waves per SIMD in LDS), 28 B
//     for r 6..7 (3 common words in a 12-byte slot of their own: the ring kind's LDS holds ~40%
//     longer segments than with a padded 16-byte slot);
//   * HOG and 5-word SSD: word 0 in an 8-byte slot, words 1-4 in a 16-byte slot, so a group's
//     16 lanes (slots DPL+1 apart) read disjoint banks (32-byte slots: 2-way).
struct PackShape {
    int nw;           // live words per pack
    int nc;           // common words (split packs)
    int cw;           // words per common slot: 1, 2 or 3
    bool split;
    int q;            // uint4 per unsplit slot
    int qx;           // uint4 per slot of the main array
    int slot_bytes;   // LDS bytes per pack, both arrays
};
__host__ __device__ constexpr PackShape pack_shape(int kind, int nd) {
    const int nw = kind == COST_SAD ? nd : kind == COST_SSD ? nd + 1 : kind == COST_SAD4 ? (2 * nd - 2 + 3) / 4 + 4 : 5;
    const int nc = kind == COST_SAD4 ? nw - 4 : (kind == COST_HOG || (kind == COST_SSD && nw == 5)) ? 1 : 0;
    const bool split = (kind == COST_SAD4 && nc <= 3) || kind == COST_HOG || (kind == COST_SSD && nw == 5);
    const int cw = (kind == COST_SAD4 && nc == 1) ? 1 : nc <= 2 ? 2 : 3;
    const int q = (nw + 3) / 4, qx = split ? 1 : q;
    return {nw, nc, cw, split, q, qx, 16 * qx + (split ? 4 * cw : 0)};
}

struct Word3 { uint32_t x, y, z; };   // a 12-byte common-word slot (4-byte aligned)

template <int COST, int ND> struct PackCfg {
    static constexpr int NW = pack_shape(COST, ND).nw;
    static constexpr int NC = pack_shape(COST, ND).nc;
    static constexpr int CW = pack_shape(COST, ND).cw;
    static constexpr bool SPLIT = pack_shape(COST, ND).split;
    static constexpr int Q = pack_shape(COST, ND).q;
    static constexpr int QX = pack_shape(COST, ND).qx;
    static constexpr int SLOT_BYTES = pack_shape(COST, ND).slot_bytes;
    static constexpr int ROWS = COST == COST_SAD4 ? 4 : 1;
    // waves per block: the 4-row kind's packs are large, one wave per block lets the LDS
    // hold as many waves as the register file does
    static constexpr int WPB = COST == COST_SAD4 ? 1 : 4;
    using CT = typename std::conditional<CW == 1, uint32_t,
                                         typename std::conditional<CW == 2, uint2, Word3>::type>::type;
};
template <int NW> struct Pk { uint32_t w[NW]; };

// ---- per-wave LDS geometry ---------------------------------------------------------------
// Each kernel's region sizes are written once, as statements that the kernel and the host's
// byte count both expand in place.  (As inlined functions returning a struct the same
// arithmetic left LLVM with other register counts in 30 instantiations.)
// Logical right-pack index i -> LDS slot: one empty slot after every DPL packs, phased by
// c0 so that every DPL-step chunk of a lane's "entering column" reads is DPL consecutive
// slots (static ds_read offsets) and the 16 lanes of a group, DPL packs apart, land DPL+1
// slots apart (DPL+1 odd -> distinct 16-byte bank groups for ds_read_b128).
__device__ __forceinline__ int rslot(int i, int c0, int dpl) { return i + (i + c0) / dpl; }

// k_match.  Segment width per lane group: segm*LPG columns rounded up to a multiple of DPL so
// that every group of a wave shares the same right-pack slot phase; WC = columns per wave.
__host__ __device__ __forceinline__ int seg_width(int lpg, int dpl, int segm) { return (segm * lpg + dpl - 1) / dpl * dpl; }
__host__ __device__ __forceinline__ int wave_cols(int lpg, int dpl, int segm) { return (64 / lpg) * seg_width(lpg, dpl, segm); }
// A wave's region is [L main | R main | L common | R common] (common arrays: split packs) of
// NL + NRphys slots: c0 = slot-gap phase, (iR0 + W2 + c0) % DPL == 0; NL left packs, NRlog
// right packs, NRphys right slots with the gaps.
#define SV_MATCH_REGIONS(WC, lpg, dpl, r)                             \
    const int c0 = ((dpl) - (4 * (r) + 1) % (dpl)) % (dpl);           \
    const int NL = (WC) + 4 * (r) + (dpl) + 1;                        \
    const int NRlog = (WC) + 4 * (r) + (lpg) * (dpl) + (dpl);         \
    const int NRphys = NRlog + (NRlog + c0) / (dpl) + 1;

// k_match_ring (one wave per block, RG_DPL disparities per lane, seg = segment width per group
// in columns): [LDSMIN scratch | main array | common array], each array `slots` long: the two
// regions and the pad slots around them (build_ring_packs).  WC = columns per wave, Tn = steps
// per segment (seg outputs + 2r warm-up, in chunks of 4), NL = left packs (+ the L prefetch
// past the last step), NRlog right packs, NRphys right slots with the gaps.
constexpr int RG_DPL = 4;
constexpr int RING_C0 = 1;            // chunk starts (index = 3 mod 4) meet slot gaps
constexpr int RING_PAD_F = 3, RING_PAD_M = 4, RING_PAD_B = 3;
#define SV_RING_GEOM(lpg, seg, r)                                     \
    const int WC = (64 / (lpg)) * (seg);                              \
    const int Tn = ((seg) + 2 * (r) + 3) & ~3;                        \
    const int NL = WC - (seg) + Tn + 1;                               \
    const int NRlog = WC - (seg) + Tn + 4 * (lpg);                    \
    const int NRphys = NRlog + (NRlog + RING_C0) / RG_DPL + 1;        \
    [[maybe_unused]] const int slots = NL + NRphys + RING_PAD_F + RING_PAD_M + RING_PAD_B;
// the LDS argmin fold's scratch at the start of the wave's LDS: 8 keys x 64 lanes
__host__ __device__ constexpr int ring_scratch_bytes(bool ldsmin) { return ldsmin ? 8 * 64 * 4 : 0; }

// ---- small device helpers ----------------------------------------------------------------
// An argmin key's disparity as the output's int16 = d * 16.
__device__ __forceinline__ int16_t key_disp16(uint32_t key, uint32_t dmask, int minD) {
    return (int16_t)(((int)(key & dmask) + minD) * 16);
}

// Pointer to a column-pack slot (main array + the split common-word array).
template <int COST, int ND, typename X, typename C> struct PackPtrT {
    X* x;
    C* c;
    __device__ __forceinline__ PackPtrT operator+(int s) const {
        return {x + s * PackCfg<COST, ND>::QX, PackCfg<COST, ND>::SPLIT ? c + s : c};
    }
};
template <int COST, int ND>
using PackPtr = PackPtrT<COST, ND, const uint4, const typename PackCfg<COST, ND>::CT>;
template <int COST, int ND> using PackOut = PackPtrT<COST, ND, uint4, typename PackCfg<COST, ND>::CT>;

// B128: the 16-byte slot as one ds_read_b128 (the ring kind, whose 32-lane groups read
// slots 80 B apart: as two dword pairs, lanes l and l+16 of a b32 cycle share banks).  The
// other kinds keep the split dword loads the compiler pairs into ds_read2_b64 (HOG: b128
// measured 518 -> 655 us per 4K frame).
template <int COST, int ND, bool B128 = false>
__device__ __forceinline__ Pk<PackCfg<COST, ND>::NW> ld(PackPtr<COST, ND> p) {
    using P = PackCfg<COST, ND>;
    Pk<P::NW> v;
    if constexpr (P::SPLIT) {
        if constexpr (P::CW == 1) {
            v.w[0] = *p.c;
        } else {
            const typename P::CT c = *p.c;
            v.w[0] = c.x;
            if constexpr (P::NC > 1) v.w[1] = c.y;
            if constexpr (P::NC > 2) v.w[2] = c.z;
        }
        if constexpr (B128) {
            const uint4 m = *p.x;
            v.w[P::NC] = m.x;
            v.w[P::NC + 1] = m.y;
            v.w[P::NC + 2] = m.z;
            v.w[P::NC + 3] = m.w;
        } else {
            const uint32_t* q = reinterpret_cast<const uint32_t*>(__builtin_assume_aligned(p.x, 16));
#pragma unroll
            for (int i = 0; i < 4; ++i) v.w[P::NC + i] = q[i];
        }
    } else {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(__builtin_assume_aligned(p.x, 16));
#pragma unroll
        for (int i = 0; i < P::NW; ++i) v.w[i] = q[i];
    }
    return v;
}

// Store the NW words w[0..NW) of one pack.
template <int COST, int ND>
__device__ __forceinline__ void put(PackOut<COST, ND> p, const uint32_t (&w)[8]) {
    using P = PackCfg<COST, ND>;
    if constexpr (P::SPLIT) {
        if constexpr (P::CW == 1) *p.c = w[0];
        else if constexpr (P::CW == 2) *p.c = make_uint2(w[0], P::NC > 1 ? w[1] : 0u);
        else *p.c = Word3{w[0], w[1], w[2]};
        p.x[0] = make_uint4(w[P::NC], w[P::NC + 1], w[P::NC + 2], w[P::NC + 3]);
    } else {
        p.x[0] = make_uint4(w[0], w[1], w[2], w[3]);
        if constexpr (P::Q > 1) p.x[1] = make_uint4(w[4], w[5], w[6], w[7]);
    }
}
// Store column k of a 4-column group's pack words (build_group, sad4_group_words).
template <int COST, int ND>
__device__ __forceinline__ void put_col(PackOut<COST, ND> p, const uint32_t (&w)[PackCfg<COST, ND>::NW][4], int k) {
    constexpr int NW = PackCfg<COST, ND>::NW;
    uint32_t v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = i < NW ? w[i < NW ? i : 0][k] : 0u;
    put<COST, ND>(p, v);
}

// Build one column pack for logical column c around output row y (replicate-clamped).
template <int COST, int ND>
__device__ __forceinline__ void build_pack(const MatchParams& a, const uint8_t* img,
                                           const uint16_t* hist, int c, int y, PackOut<COST, ND> dst) {
    const int cc = clampi(c, 0, a.W - 1);
    if constexpr (COST == COST_HOG) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(hist + ((size_t)y * a.W + cc) * 10);
        const uint32_t w[8] = {src[0], src[1], src[2], src[3], src[4], 0u, 0u, 0u};
        put<COST, ND>(dst, w);
    } else if constexpr (COST == COST_SAD4) {
        // rows y-r .. y+r+3 (j = 0 .. 2r+3): j in [3, 2r] -> common word (j-3)/4; the 3
        // rows of output q outside the common block -> byte positions of word ND+q
        constexpr int NC = PackCfg<COST, ND>::NW - 4;
        uint32_t w[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        const int r = ND;
        for (int j = 0; j <= 2 * r + 3; ++j) {
            const int yy = clampi(y - r + j, 0, a.H - 1);
            const uint32_t v = img[(size_t)yy * a.pitch + cc];
            if (j >= 3 && j <= 2 * r) {
                const int q = (j - 3) >> 2;
                const uint32_t sh = v << (8 * ((j - 3) & 3));
#pragma unroll
                for (int i = 0; i < NC; ++i) w[i] |= q == i ? sh : 0u;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                // custom rows of output q: j = q .. 2 (before the common block), then
                // j = 2r+1 .. 2r+q (after it); byte position = order within the 3
                const int pos = j <= 2 ? j - q : (j >= 2 * r + 1 ? (3 - q) + (j - 2 * r - 1) : -1);
                const bool in = j <= 2 ? (j >= q) : (j >= 2 * r + 1 && j <= 2 * r + q);
                w[NC + q] |= in ? v << (8 * pos) : 0u;
            }
        }
        put<COST, ND>(dst, w);
    } else {
        uint32_t w[5] = {0u, 0u, 0u, 0u, 0u};
        uint32_t sq = 0;
        for (int j = 0; j < a.win; ++j) {
            const int yy = clampi(y - a.r + j, 0, a.H - 1);
            const uint32_t v = img[(size_t)yy * a.pitch + cc];
            sq += v * v;
            const uint32_t sh = v << (8 * (j & 3));
            const int q = j >> 2;
            w[0] |= q == 0 ? sh : 0u;
            w[1] |= q == 1 ? sh : 0u;
            w[2] |= q == 2 ? sh : 0u;
            w[3] |= q == 3 ? sh : 0u;
        }
        if constexpr (COST == COST_SSD) w[ND] = sq;
        const uint32_t o[8] = {w[0], w[1], w[2], w[3], w[4], 0u, 0u, 0u};
        put<COST, ND>(dst, o);
    }
}

// ---- vectorised pack building: one lane = 4 consecutive in-bounds columns -------------
// Each window row is read as ONE dword (4 columns) and 4 rows x 4 columns are transposed
// with v_perm_b32 into the 4 columns' pack words (8 perms per 16 bytes), instead of one
// clamped byte load + shift/select chain per (row, column).
__device__ __forceinline__ void transpose4(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t (&o)[4]) {
    const uint32_t t0 = __builtin_amdgcn_perm(b, a, 0x05010400u);   // a0 b0 a1 b1
    const uint32_t t1 = __builtin_amdgcn_perm(b, a, 0x07030602u);   // a2 b2 a3 b3
    const uint32_t t2 = __builtin_amdgcn_perm(d, c, 0x05010400u);   // c0 d0 c1 d1
    const uint32_t t3 = __builtin_amdgcn_perm(d, c, 0x07030602u);   // c2 d2 c3 d3
    o[0] = __builtin_amdgcn_perm(t2, t0, 0x05040100u);              // a0 b0 c0 d0
    o[1] = __builtin_amdgcn_perm(t2, t0, 0x07060302u);
    o[2] = __builtin_amdgcn_perm(t3, t1, 0x05040100u);
    o[3] = __builtin_amdgcn_perm(t3, t1, 0x07060302u);
}

// 4-row kind: the pack words of 4 columns from their 2r+4 window rows (one dword = the 4
// columns of a row, rows y-r .. y+r+3); same layout as build_pack.
// The common block is 2r-2 rows, so its last word holds four rows or two: two rows take one
// perm per column straight from the row dwords (selector 0x0c = a zero byte).  The per-row
// words of outputs 0..3 hold rows {0,1,2}, {1,2,2r+1}, {2,2r+1,2r+2}, {2r+1,2r+2,2r+3}: the
// row pairs (1,2) and (2r+1,2r+2) that two neighbouring outputs share are interleaved once
// (2 perms each), and every word is then one perm of a pair against its third row: 24 perms
// for the four words instead of the 32 of four 3-row transposes.
template <int R>
__device__ __forceinline__ void sad4_group_words(const uint32_t (&rw)[2 * R + 4],
                                                 uint32_t (&w)[PackCfg<COST_SAD4, R>::NW][4]) {
    constexpr int NC = PackCfg<COST_SAD4, R>::NW - 4, NCR = 2 * R - 2;
    static_assert(NCR % 4 == 0 || NCR % 4 == 2, "the common block's last word holds 4 or 2 rows");
#pragma unroll
    for (int m = 0; m < NC; ++m) {
        const int b = 3 + 4 * m;
        if (4 * m + 4 <= NCR) {
            transpose4(rw[b], rw[b + 1], rw[b + 2], rw[b + 3], w[m]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)   // a_k b_k 0 0
                w[m][k] = __builtin_amdgcn_perm(rw[b + 1], rw[b], 0x0c0c0400u + 0x0101u * (uint32_t)k);
        }
    }
    constexpr int P = 2 * R + 1;
    const uint32_t pa[2] = {__builtin_amdgcn_perm(rw[2], rw[1], 0x05010400u),    // a0 b0 a1 b1
                            __builtin_amdgcn_perm(rw[2], rw[1], 0x07030602u)};   // a2 b2 a3 b3
    const uint32_t pb[2] = {__builtin_amdgcn_perm(rw[P + 1], rw[P], 0x05010400u),
                            __builtin_amdgcn_perm(rw[P + 1], rw[P], 0x07030602u)};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // column k's pair sits in bytes 2(k&1), 2(k&1)+1 of the pair word k >> 1 (selector 4..7:
        // the first operand); its third row is byte k of the second operand
        const uint32_t p0 = 4u + 2u * (k & 1), p1 = p0 + 1u, s = (uint32_t)k;
        const uint32_t row_pair = 0x0c000000u | (p1 << 16) | (p0 << 8) | s;   // row, pair
        const uint32_t pair_row = 0x0c000000u | (s << 16) | (p1 << 8) | p0;   // pair, row
        w[NC + 0][k] = __builtin_amdgcn_perm(pa[k >> 1], rw[0], row_pair);
        w[NC + 1][k] = __builtin_amdgcn_perm(pa[k >> 1], rw[P], pair_row);
        w[NC + 2][k] = __builtin_amdgcn_perm(pb[k >> 1], rw[2], row_pair);
        w[NC + 3][k] = __builtin_amdgcn_perm(pb[k >> 1], rw[P + 2], pair_row);
    }
}

// Pack words of the 4 columns cg..cg+3 (all inside [0, W), 4-byte aligned rows) around
// output row y; same layout as build_pack.
template <int COST, int ND>
__device__ __forceinline__ void build_group(const MatchParams& a, const uint8_t* img, int cg, int y,
                                            uint32_t (&w)[PackCfg<COST, ND>::NW][4]) {
    const int r = COST == COST_SAD4 ? ND : a.r;
    auto row = [&](int j) -> uint32_t {
        const int yy = clampi(y - r + j, 0, a.H - 1);
        return *reinterpret_cast<const uint32_t*>(img + (size_t)yy * a.pitch + cg);
    };
    if constexpr (COST == COST_SAD4) {
        uint32_t rw[2 * ND + 4];
#pragma unroll
        for (int j = 0; j < 2 * ND + 4; ++j) rw[j] = row(j);
        sad4_group_words<ND>(rw, w);
        return;
    }
    const int nsh = a.win;                                   // transposed rows
#pragma unroll
    for (int q = 0; q < ND; ++q) {
        uint32_t d[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) d[t] = (4 * q + t < nsh) ? row(4 * q + t) : 0u;
        transpose4(d[0], d[1], d[2], d[3], w[q]);
    }
    if constexpr (COST == COST_SSD) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t sq = 0u;
#pragma unroll
            for (int q = 0; q < ND; ++q) sq = __builtin_amdgcn_udot4(w[q][k], w[q][k], sq, false);
            w[ND][k] = sq;
        }
    }
}

// All column packs of one wave: L packs i -> column cL0 + i (slot i), R packs i -> column
// cR0 + i (slot rslot(i)).  Interior 4-column groups take the vectorised path; groups
// touching the image border (replicate clamp), HOG, and unaligned images take build_pack.
template <int COST, int ND, int DPL>
__device__ __forceinline__ void build_all_packs(const MatchParams& a, int y, int cL0, int NL, int cR0,
                                                int NRlog, int c0, PackOut<COST, ND> Lp,
                                                PackOut<COST, ND> Rp, int lane) {
    constexpr int NW = PackCfg<COST, ND>::NW;
    bool aligned = ((reinterpret_cast<uintptr_t>(a.L) | reinterpret_cast<uintptr_t>(a.R) |
                     (uintptr_t)a.pitch) & 3u) == 0;
    if constexpr (COST == COST_HOG) aligned = false;
    if (!aligned) {
        for (int i = lane; i < NL; i += 64) build_pack<COST, ND>(a, a.L, a.HL, cL0 + i, y, Lp + i);
        for (int i = lane; i < NRlog; i += 64)
            build_pack<COST, ND>(a, a.R, a.HR, cR0 + i, y, Rp + rslot(i, c0, DPL));
        return;
    }
    if constexpr (COST != COST_HOG) {
    const int aL = cL0 & ~3, aR = cR0 & ~3;                  // floor to a multiple of 4
    const int gL = (cL0 + NL - aL + 3) >> 2, gR = (cR0 + NRlog - aR + 3) >> 2;
    for (int gi = lane; gi < gL + gR; gi += 64) {
        const bool right = gi >= gL;
        const int cg = right ? aR + 4 * (gi - gL) : aL + 4 * gi;
        const int cfirst = right ? cR0 : cL0, n = right ? NRlog : NL;
        const uint8_t* img = right ? a.R : a.L;
        const PackOut<COST, ND> base = right ? Rp : Lp;
        if (cg >= 0 && cg + 4 <= a.W) {
            uint32_t w[NW][4];
            build_group<COST, ND>(a, img, cg, y, w);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int idx = cg + k - cfirst;
                if (idx < 0 || idx >= n) continue;
                put_col<COST, ND>(base + (right ? rslot(idx, c0, DPL) : idx), w, k);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int idx = cg + k - cfirst;
                if (idx < 0 || idx >= n) continue;
                build_pack<COST, ND>(a, img, nullptr, cg + k, y, base + (right ? rslot(idx, c0, DPL) : idx));
            }
        }
    }
    }
}

// The ring kind's packs (4-row kind, radius R): as build_all_packs, but each lane issues
// the row loads of up to MF of its 4-column groups before it transposes any of them, so a
// wave waits for its global loads once per MF groups instead of once per group (the
// per-group form left ~8% of k_match's time in the segment prologue).  Groups touching the
// image border load nothing and take build_pack afterwards.
// An interior group stores all of its four columns, also those just outside the wave's range
// (indices -3 .. -1 and n .. n + 2), so the regions need unused slots around them: RING_PAD_F
// in front of the left region, RING_PAD_M between the two (the left's 3 rear slots and the
// right's 4 front slots, index -3 sitting in slot -4, are the same ones: both only ever receive
// unread columns) and RING_PAD_B behind the right one.
template <int R, int MF, int DPL>
__device__ __forceinline__ void build_ring_packs(const MatchParams& a, int y, int cL0, int NL, int cR0,
                                                 int NRlog, int c0, PackOut<COST_SAD4, R> Lp,
                                                 PackOut<COST_SAD4, R> Rp, int lane) {
    constexpr int NW = PackCfg<COST_SAD4, R>::NW, NRW = 2 * R + 4;
    const bool aligned = ((reinterpret_cast<uintptr_t>(a.L) | reinterpret_cast<uintptr_t>(a.R) |
                           (uintptr_t)a.pitch) & 3u) == 0;
    // the row loads below address a frame by 32-bit byte offsets
    const bool near = (long long)a.H * (long long)a.pitch < 0x7FFFFFFFLL;
    if (!aligned || !near) {
        build_all_packs<COST_SAD4, R, DPL>(a, y, cL0, NL, cR0, NRlog, c0, Lp, Rp, lane);
        return;
    }
    // Row loads through one buffer descriptor per image: the row offset (wave-uniform) is the
    // scalar offset and the group's first column the only per-lane term, instead of a 64-bit
    // per-lane address for every (group, row).  A wave's m-th groups are the left image's, the
    // right image's or (one m per wave) both: each image's lanes load in a pass of their own,
    // and a pass with no lanes is skipped.
    const auto lsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a.L), 0, 0x7FFFFFFF, 0x00020000);
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a.R), 0, 0x7FFFFFFF, 0x00020000);
    const int aL = cL0 & ~3, aR = cR0 & ~3;                  // floor to a multiple of 4
    const int gL = (cL0 + NL - aL + 3) >> 2, gR = (cR0 + NRlog - aR + 3) >> 2;
    const int G = gL + gR;
    int roff[NRW];                                           // row offsets (wave-uniform)
#pragma unroll
    for (int j = 0; j < NRW; ++j) roff[j] = clampi(y - R + j, 0, a.H - 1) * a.pitch;
    static_assert(DPL == 4, "a 4-column group meets one slot gap at a wave-uniform column");
    for (int g0 = 0; g0 < G; g0 += 64 * MF) {
        uint32_t rw[MF][NRW];
#pragma unroll
        for (int m = 0; m < MF; ++m) {
            const int gi = g0 + lane + 64 * m;
            const bool right = gi >= gL;
            const int cg = right ? aR + 4 * (gi - gL) : aL + 4 * gi;
            const bool in = gi < G && cg >= 0 && cg + 4 <= a.W;   // the others' rw stay unread
            if (in && !right) {
#pragma unroll
                for (int j = 0; j < NRW; ++j) rw[m][j] = __builtin_amdgcn_raw_buffer_load_b32(lsrc, cg, roff[j], 0);
            }
            if (in && right) {
#pragma unroll
                for (int j = 0; j < NRW; ++j) rw[m][j] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, cg, roff[j], 0);
            }
        }
#pragma unroll
        for (int m = 0; m < MF; ++m) {
            const int gi = g0 + lane + 64 * m;
            if (gi >= G) continue;
            const bool right = gi >= gL;
            const int cg = right ? aR + 4 * (gi - gL) : aL + 4 * gi;
            const int cfirst = right ? cR0 : cL0, n = right ? NRlog : NL;
            const PackOut<COST_SAD4, R> base = right ? Rp : Lp;
            if (cg >= 0 && cg + 4 <= a.W) {
                // All four columns, with no range test per column: the up to three columns of a
                // region's first or last group that lie outside [cfirst, cfirst + n) land in
                // the pad slots around the regions, which nothing reads.  Left: consecutive
                // slots from one base.  Right: group j's column k has index 4j + d + k, so its
                // slot is (d + 5j) + k + floor((d + k + c0) / 4): one base per lane and four
                // wave-uniform offsets (d = aR - cR0 is the same for every group of the wave).
                uint32_t w[NW][4];
                sad4_group_words<R>(rw[m], w);
                if (right) {
                    const int d = aR - cR0;                  // -3 .. 0
                    const PackOut<COST_SAD4, R> gb = Rp + (d + ((cg - aR) >> 2) * (DPL + 1));
#pragma unroll
                    for (int k = 0; k < 4; ++k) put_col<COST_SAD4, R>(gb + (k + ((d + k + c0 + DPL) >> 2) - 1), w, k);   // (floor)
                } else {
                    const PackOut<COST_SAD4, R> gb = Lp + (cg - cL0);
#pragma unroll
                    for (int k = 0; k < 4; ++k) put_col<COST_SAD4, R>(gb + k, w, k);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int idx = cg + k - cfirst;
                    if (idx < 0 || idx >= n) continue;
                    build_pack<COST_SAD4, R>(a, right ? a.R : a.L, nullptr, cg + k, y,
                                             base + (right ? rslot(idx, c0, DPL) : idx));
                }
            }
        }
    }
}

// Reduce-scatter of 8 keys over the 16 lanes of a row: on return lanes 2j and 2j+1 hold the
// min over the row of key j = (l >> 1) & 7 in v[0].  Bank-masked DPP for lane bits 3 and 2,
// selects for bit 1, then one all-reduce step with lane l ^ 1: 16 ops for 8 keys.
__device__ __forceinline__ void reduce_scatter8_bm(uint32_t (&v)[8], int l) {
#define SV_BM_PAIR(A, B, CTRL, M0, M1)                                                          \
    "v_min_u32_dpp %" #A ", %" #A ", %" #A " " CTRL " row_mask:0xf bank_mask:" M0 "\n\t"      \
    "v_min_u32_dpp %" #A ", %" #B ", %" #B " " CTRL " row_mask:0xf bank_mask:" M1 "\n\t"
    asm volatile("s_nop 1\n\t"
                 SV_BM_PAIR(0, 4, "row_mirror", "0x3", "0xc") SV_BM_PAIR(1, 5, "row_mirror", "0x3", "0xc")
                 SV_BM_PAIR(2, 6, "row_mirror", "0x3", "0xc") SV_BM_PAIR(3, 7, "row_mirror", "0x3", "0xc")
                 : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3])
                 : "v"(v[4]), "v"(v[5]), "v"(v[6]), "v"(v[7]));
    asm volatile("s_nop 1\n\t"
                 SV_BM_PAIR(0, 2, "row_half_mirror", "0x5", "0xa") SV_BM_PAIR(1, 3, "row_half_mirror", "0x5", "0xa")
                 : "+v"(v[0]), "+v"(v[1])
                 : "v"(v[2]), "v"(v[3]));
#undef SV_BM_PAIR
    const bool hi = (l & 2) != 0;
    const uint32_t send = hi ? v[0] : v[1];
    const uint32_t keep = hi ? v[1] : v[0];
    v[0] = min(keep, (uint32_t)__builtin_amdgcn_update_dpp(0u, (int)send, 0x1B, 0xF, 0xF, false));  // l ^ 3
    v[0] = min(v[0], (uint32_t)__builtin_amdgcn_update_dpp(0u, (int)v[0], 0xB1, 0xF, 0xF, false));  // l ^ 1
}

// sv_match_ring.hip: launches `a` as the ring kind (SAD windows 5..15 and SSD windows 5..9 with
// D <= 256, SAD with 256 < D <= 512 as two passes and a merge) and returns its hipError_t, or
// returns -1 where the launch is k_match's.
int launch_match_ring(const MatchParams& a, int cost, hipStream_t s);

}  // namespace sv
