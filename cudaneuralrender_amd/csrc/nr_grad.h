// nr_grad.h -- the network's value and analytic gradient on a wave's 64 points (mlp16_grad): the
// device functions k_grad (nr_grad.hip, nr_mlp_gradient) and k_project (nr_project.hip,
// nr_project_points) share.
//
// Forward: mlp16_fp32_nt (nr_mlp16.h) with its mask output -- nr_mlp_forward's fp32 bits, and for
// every ReLU layer the bits z > 0, 8 per lane, tile and layer in two words per tile.
// Backward: the same matrix-core loop on the transposed kernels (the backward pack, nr_internal.h
// pack_grad_16): 8 k-steps x 2 row tiles of v_mfma_f32_16x16x4_f32 per layer and 16-point tile,
// each dot product one fmaf chain from +0 over the layer's output units ascending.  A masked C
// result is the next layer's B operand with no lane movement (unit 4k + g in register k of lane
// group g, the forward's order); only the last ReLU layer's mask, which the forward holds as
// units 8g + k, is transposed: one 32-bit word per point by two v_permlane swaps per tile.
// Applying a mask costs two VALU per element (v_bfe_i32 to 0 / ~0, v_and_b32) and recording it
// two (v_min_u32, v_lshl_or_b32): a masked element is +0 exactly, the operand the chains are
// specified with.  The input layer's transpose is one more row tile whose rows repeat every 4, so
// that every lane group holds the gradient and a lane selects its own tile's.
//
// A point's outputs depend only on that point: the tiles' columns are independent and the two
// forms (clamped on the scaled pack, add + max beyond F32_INPUT_BOUND) give the same bits.
#pragma once
#include "nr_mlp16.h"

namespace nr {

// The two packs (~61 KB for 7 hidden layers) let two workgroups share a CU.  4-wave workgroups:
// 2 waves per SIMD, whose register budget (256) the four-tile forward + masks + backward fit
// without scratch (207 VGPRs); 8-wave workgroups (4 per SIMD, 128 registers) spilled ~50 of them.
// The forward alone loses ~5 % from 4 to 2 waves per SIMD (profiles/r1_mlp_occupancy_sweep.txt).
#ifndef NR_GRAD_WAVES
#define NR_GRAD_WAVES 4
#endif

// 0 or ~0 from bit `pos` of m (v_bfe_i32)
__device__ __forceinline__ uint32_t bit_fill(uint32_t m, int pos) {
    return (uint32_t)__builtin_amdgcn_sbfe((int)m, (uint32_t)pos, 1u);
}

// value (lane p = point p of the wave) and gradient gr[0..3] (gr[3] = 0 for 3 inputs) on NT tiles.
// s: the forward pack, sb: the backward pack (LDS).
template <int NT, bool CL>
__device__ __forceinline__ float mlp16_grad_nt(const float *__restrict__ s, const float *__restrict__ sb, int in0, int nh,
                                               float fr, float x, float y, float z, float (&gr)[4]) {
    const int lane = lane_id(), g = lane >> 4;
    uint32_t mk[NT][2];
#pragma unroll
    for (int t = 0; t < NT; ++t) mk[t][0] = mk[t][1] = 0u;
    const float value = mlp16_fp32_nt<NT, 0, CL, 0, true>(s, in0, nh, fr, x, y, z, mk);

    // g of the last ReLU layer: its mask as one word per point (bit u = unit u), then the last
    // kernel where the bit is set
    float gq[NT][8];
    {
        const float4 *kl = reinterpret_cast<const float4 *>(sb + gb_last(nh) + g * 8);
        const float4 klo = kl[0], khi = kl[1];
        const float kw[8] = {klo.x, klo.y, klo.z, klo.w, khi.x, khi.y, khi.z, khi.w};
        const int sh = 8 * (nh & 3);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const uint32_t b = ((nh < 4 ? mk[t][0] : mk[t][1]) >> sh) & 0xffu;
            uint32_t w = b << (8 * g);
            auto r = __builtin_amdgcn_permlane32_swap(w, w, false, false);  // [w0 w1 w0 w1], [w2 w3 w2 w3]
            w = r[0] | r[1];
            r = __builtin_amdgcn_permlane16_swap(w, w, false, false);       // [x0 x0 x2 x2], [x1 x1 x3 x3]
            w = (r[0] | r[1]) >> g;
#pragma unroll
            for (int k = 0; k < 8; ++k) gq[t][k] = __uint_as_float(bit_fill(w, 4 * k) & __float_as_uint(kw[k]));
        }
    }
    // hidden layers, last to first: acc[i] = chain over j of K[i][j] g[j], then the mask of layer jl
    f32x4 c[NT][2];
    for (int jl = nh - 1; jl >= 0; --jl) {
        const float *L = sb + jl * 1024;
        float4 wq[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) wq[q] = reinterpret_cast<const float4 *>(L)[q * 64 + lane];
#pragma unroll
        for (int st = 0; st < 8; ++st) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const int m = 2 * st + mt;
                const float4 wv = wq[m >> 2];
                const float w = (m & 3) == 0 ? wv.x : ((m & 3) == 1 ? wv.y : ((m & 3) == 2 ? wv.z : wv.w));
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    c[t][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                        w, gq[t][st], st == 0 ? f32x4{0.0f, 0.0f, 0.0f, 0.0f} : c[t][mt], 0, 0, 0);
            }
        }
        const int sh = 8 * (jl & 3);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const uint32_t mw = (jl < 4 ? mk[t][0] : mk[t][1]) >> sh;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    gq[t][4 * mt + r] = __uint_as_float(bit_fill(mw, 4 * mt + r) & __float_as_uint(c[t][mt][r]));
        }
    }
    // the input layer: one row tile, rows = inputs (repeated every 4)
    {
        const float4 *A = reinterpret_cast<const float4 *>(sb + gb_l0(nh));
        const float4 a0 = A[lane], a1 = A[64 + lane];
        const float w[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        f32x4 d[NT];
#pragma unroll
        for (int st = 0; st < 8; ++st)
#pragma unroll
            for (int t = 0; t < NT; ++t)
                d[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[st], gq[t][st],
                                                            st == 0 ? f32x4{0.0f, 0.0f, 0.0f, 0.0f} : d[t], 0, 0, 0);
        // point p = 16t + j: lane p is lane (j, t) of tile t
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = d[0][r];
            if constexpr (NT > 1) v = g == 1 ? d[1][r] : v;
            if constexpr (NT > 2) v = g == 2 ? d[2][r] : v;
            if constexpr (NT > 3) v = g == 3 ? d[NT > 3 ? 3 : 0][r] : v;
            gr[r] = v;
        }
    }
    return value;
}

// cl (wave-uniform) as mlp16_fp32's: the clamped form on the active tiles, else add + max on four
__device__ __forceinline__ float mlp16_grad(const MlpArgs &M, const float *s, const float *sb, float fr, float x, float y,
                                            float z, uint32_t tmask, float (&gr)[4]) {
    const int nt = 32 - __clz((int)tmask);
    if (M.f32_clamp && inputs_in_bound_f32(x, y, z, fr)) {
        if (nt >= 4) return mlp16_grad_nt<4, true>(s, sb, M.in0, M.nh, fr, x, y, z, gr);
        if (nt == 3) return mlp16_grad_nt<3, true>(s, sb, M.in0, M.nh, fr, x, y, z, gr);
        if (nt == 2) return mlp16_grad_nt<2, true>(s, sb, M.in0, M.nh, fr, x, y, z, gr);
        return mlp16_grad_nt<1, true>(s, sb, M.in0, M.nh, fr, x, y, z, gr);
    }
    return mlp16_grad_nt<4, false>(s, sb, M.in0, M.nh, fr, x, y, z, gr);
}

}  // namespace nr
