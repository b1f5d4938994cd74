// sv_harris_wave.h — the register/DPP Harris bands and the one Harris response function.
// sv_harris.hip wraps the bands in kernels of their own; sv_median.hip runs them in the extra
// blocks of k_median_i16<1|2, *>.
#pragma once
#include "sv_stencil.h"

namespace sv {

// Box sums of the gradient products -> response, cornerHarris(3, 3, 0.04) convention: the
// sums are exact integers and every form shares these f32 operations, so the LDS, the 1- and
// the 4-column kernels are bit-identical.
constexpr float kHarrisScale2 = (float)((1.0 / (4.0 * 3.0 * 255.0)) * (1.0 / (4.0 * 3.0 * 255.0)));
__device__ __forceinline__ float harris_response(int sxx, int sxy, int syy) {
    const float a = (float)sxx * kHarrisScale2, b = (float)sxy * kHarrisScale2, c = (float)syy * kHarrisScale2;
    const float t1 = a * c, t2 = b * b, t3 = a + c, t4 = t3 * t3;
    const float rr = t1 - t2;
    const float kt = 0.04f * t4;
    return rr - kt;
}

// ---------------------------------------------------------------------------------------
// Harris, register/DPP form (the default for W, H >= 8): one wave = 64 consecutive columns
// (lane j <-> column x0 - 2 + j, 60 outputs for lanes 2..61) walking down a band of HB output
// rows (PF image rows prefetched); no LDS, no barriers.  Per product row a lane loads ONE image byte (its column of the
// next row, reflect-101), its left/right neighbours come by wave_shr/wave_shl DPP: the Sobel
// column sums and row smooths, the 3 gradient products, their vertical 3-row sums from a
// register ring and the horizontal 3-sums by DPP again; coalesced f32 stores.  Reflect-101
// of the PRODUCT images (cv2.cornerHarris box-filters the products with reflect-101) falls
// out of computing every product from reflect-101 pixels, except the cross product's sign:
// outside the image gx (row) or gy (column) flips, so gxy is negated once per dimension in
// which the position lies outside (gxx, gyy are even).  Sums are exact integers; the float
// epilogue is the LDS kernel's, so outputs are identical.
// One wave's band: output columns x0 .. x0+59, rows y0 .. y0+HB-1 of one frame.
template <int HB, int PF>
__device__ __forceinline__ void harris_wave(const uint8_t* __restrict__ g, int H, int W, int pitch,
                                            float* __restrict__ out, int x0, int y0, int lane) {
    const int c = x0 - 2 + lane;
    const int cc = refl101(clampi(c, -2, W + 1), W);              // loaded column
    const int csign = (c < 0 || c >= W) ? -1 : 1;                  // gxy sign outside the image
    const bool emit = lane >= 2 && lane < 62 && c < W;
    auto ldrow = [&](int r) -> int {   // image row r (reflect-101), this lane's column
        return (int)g[(size_t)refl101(clampi(r, -2, H + 1), H) * pitch + cc];
    };
    auto rowsm = [&](int v) { return dpp_shr1_keep(v) + 2 * v + dpp_shl1_keep(v); };
    // product rows y0-1 .. y0+HB; image rows y0-2 .. y0+HB+1
    // PF image rows in flight ahead of the one being used (the loads are one byte per lane:
    // latency, not bandwidth, is what they cost)
    int im = ldrow(y0 - 2), ic = ldrow(y0 - 1);
    int pre[PF];
#pragma unroll
    for (int k = 0; k < PF; ++k) pre[k] = ldrow(y0 + k);
    int rsm = rowsm(im), rsc = rowsm(ic);
    int pxx[3] = {0, 0, 0}, pxy[3] = {0, 0, 0}, pyy[3] = {0, 0, 0};
    const int rend = min(y0 + HB, H);                               // last output row + 1
    for (int r = y0 - 1; r <= rend; ++r) {
        const int ip = pre[0];
#pragma unroll
        for (int k = 0; k + 1 < PF; ++k) pre[k] = pre[k + 1];
        pre[PF - 1] = ldrow(r + 1 + PF);
        const int rsp = rowsm(ip);
        const int col = im + 2 * ic + ip;
        const int gx = dpp_shl1_keep(col) - dpp_shr1_keep(col);
        const int gy = rsp - rsm;
        const int rsign = (r < 0 || r >= H) ? -csign : csign;
        pxx[0] = pxx[1]; pxx[1] = pxx[2]; pxx[2] = __mul24(gx, gx);
        pyy[0] = pyy[1]; pyy[1] = pyy[2]; pyy[2] = __mul24(gy, gy);
        pxy[0] = pxy[1]; pxy[1] = pxy[2]; pxy[2] = rsign * __mul24(gx, gy);
        im = ic;
        ic = ip;
        rsm = rsc;
        rsc = rsp;
        if (r >= y0 + 1) {   // output row r - 1 from product rows r-2 .. r
            const int vxx = pxx[0] + pxx[1] + pxx[2], vxy = pxy[0] + pxy[1] + pxy[2], vyy = pyy[0] + pyy[1] + pyy[2];
            const int sxx = dpp_shr1_keep(vxx) + vxx + dpp_shl1_keep(vxx);
            const int sxy = dpp_shr1_keep(vxy) + vxy + dpp_shl1_keep(vxy);
            const int syy = dpp_shr1_keep(vyy) + vyy + dpp_shl1_keep(vyy);
            const float resp = harris_response(sxx, sxy, syy);
            if (emit) out[(size_t)(r - 1) * W + c] = resp;
        }
    }
}

// Harris, 4 columns per lane (the default for W >= 1024; any W >= 256 works): lane j holds columns x0-4+4j ..
// x0-1+4j as one dword per image row (interior waves: one aligned dword load per lane-row;
// waves touching an image border or unaligned rows assemble it from 4 reflect-101 byte
// loads), the lane's first/last neighbours come by wave_shr/shl:1 DPP; 248 output columns
// per wave (lanes 1..62), f32x4 stores.  Same arithmetic, same reflect-101 product rule and
// the same float epilogue as harris_wave: bit-identical outputs.
// One wave's band: output columns x0 .. x0+247, rows y0 .. y0+HB-1 of one frame.
template <int HB, int PF>
__device__ __forceinline__ void harris_wave4(const uint8_t* __restrict__ g, int H, int W, int pitch,
                                             float* __restrict__ out, int x0, int y0, int lane) {
    const int c0 = x0 - 4 + 4 * lane;                               // first column of the lane
    // interior: every lane's 4 columns inside the image and dword-aligned rows (uniform)
    const bool fast = x0 >= 4 && x0 + 252 <= W && ((pitch & 3) == 0) && ((((uintptr_t)g) & 3) == 0);
    int cc[4], csg[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + i;
        cc[i] = refl101(clampi(c, -2, W + 1), W);
        csg[i] = (c < 0 || c >= W) ? -1 : 1;
    }
    auto ldrow = [&](int r) -> uint32_t {   // image row r (reflect-101), the lane's 4 columns
        const uint8_t* row = g + (size_t)refl101(clampi(r, -2, H + 1), H) * pitch;
        if (fast) return *reinterpret_cast<const uint32_t*>(row + c0);
        return (uint32_t)row[cc[0]] | ((uint32_t)row[cc[1]] << 8) | ((uint32_t)row[cc[2]] << 16) |
               ((uint32_t)row[cc[3]] << 24);
    };
    auto unpack = [](uint32_t w, int (&p)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) p[i] = (int)((w >> (8 * i)) & 0xffu);
    };
    // row smooth p[i-1] + 2 p[i] + p[i+1] of the lane's 4 columns (neighbour bytes by DPP)
    auto rowsm4 = [&](uint32_t w, int (&o)[4]) {
        int p[4];
        unpack(w, p);
        const int lft = (int)(((uint32_t)dpp_shr1_keep((int)w)) >> 24);
        const int rgt = (int)(((uint32_t)dpp_shl1_keep((int)w)) & 0xffu);
        o[0] = lft + 2 * p[0] + p[1];
        o[1] = p[0] + 2 * p[1] + p[2];
        o[2] = p[1] + 2 * p[2] + p[3];
        o[3] = p[2] + 2 * p[3] + rgt;
    };
    int im[4], ic[4], rsm[4], rsc[4];
    {
        const uint32_t wm = ldrow(y0 - 2), wc = ldrow(y0 - 1);
        unpack(wm, im);
        unpack(wc, ic);
        rowsm4(wm, rsm);
        rowsm4(wc, rsc);
    }
    uint32_t pre[PF];
#pragma unroll
    for (int k = 0; k < PF; ++k) pre[k] = ldrow(y0 + k);
    int pxx[3][4] = {}, pxy[3][4] = {}, pyy[3][4] = {};
    const int rend = min(y0 + HB, H);
    const bool emit_lane = lane >= 1 && lane < 63;
    for (int r = y0 - 1; r <= rend; ++r) {
        const uint32_t wp = pre[0];
#pragma unroll
        for (int k = 0; k + 1 < PF; ++k) pre[k] = pre[k + 1];
        pre[PF - 1] = ldrow(r + 1 + PF);
        int ip[4], rsp[4], col[4];
        unpack(wp, ip);
        rowsm4(wp, rsp);
#pragma unroll
        for (int i = 0; i < 4; ++i) col[i] = im[i] + 2 * ic[i] + ip[i];
        const int cl = dpp_shr1_keep(col[3]), cr = dpp_shl1_keep(col[0]);
        const bool rout = r < 0 || r >= H;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int gx = (i < 3 ? col[i + 1] : cr) - (i > 0 ? col[i - 1] : cl);
            const int gy = rsp[i] - rsm[i];
            const int sg = rout ? -csg[i] : csg[i];
            pxx[0][i] = pxx[1][i]; pxx[1][i] = pxx[2][i]; pxx[2][i] = __mul24(gx, gx);
            pyy[0][i] = pyy[1][i]; pyy[1][i] = pyy[2][i]; pyy[2][i] = __mul24(gy, gy);
            pxy[0][i] = pxy[1][i]; pxy[1][i] = pxy[2][i]; pxy[2][i] = sg * __mul24(gx, gy);
            im[i] = ic[i];
            ic[i] = ip[i];
            rsm[i] = rsc[i];
            rsc[i] = rsp[i];
        }
        if (r >= y0 + 1) {   // output row r - 1
            int vxx[4], vxy[4], vyy[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                vxx[i] = pxx[0][i] + pxx[1][i] + pxx[2][i];
                vxy[i] = pxy[0][i] + pxy[1][i] + pxy[2][i];
                vyy[i] = pyy[0][i] + pyy[1][i] + pyy[2][i];
            }
            const int lxx = dpp_shr1_keep(vxx[3]), rxx = dpp_shl1_keep(vxx[0]);
            const int lxy = dpp_shr1_keep(vxy[3]), rxy = dpp_shl1_keep(vxy[0]);
            const int lyy = dpp_shr1_keep(vyy[3]), ryy = dpp_shl1_keep(vyy[0]);
            float o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int sxx = (i > 0 ? vxx[i - 1] : lxx) + vxx[i] + (i < 3 ? vxx[i + 1] : rxx);
                const int sxy = (i > 0 ? vxy[i - 1] : lxy) + vxy[i] + (i < 3 ? vxy[i + 1] : rxy);
                const int syy = (i > 0 ? vyy[i - 1] : lyy) + vyy[i] + (i < 3 ? vyy[i + 1] : ryy);
                o[i] = harris_response(sxx, sxy, syy);
            }
            if (emit_lane) {
                float* orow = out + (size_t)(r - 1) * W;
                if (c0 + 3 < W && ((W & 3) == 0) && ((((uintptr_t)out) & 15) == 0)) {
                    *reinterpret_cast<float4*>(orow + c0) = make_float4(o[0], o[1], o[2], o[3]);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (c0 + i >= 0 && c0 + i < W) orow[c0 + i] = o[i];
                }
            }
        }
    }
}

}  // namespace sv
