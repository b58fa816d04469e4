// nr_fit.hip -- fitting a [3, 32, ..., 32, 1] network to (point, value) pairs (nr_fit_*): the
// weight gradients of the clamped or plain L2 loss (k_fit_grad), their ordered totals, Adam and the
// packs rewritten on the device (k_fit_update).  The arithmetic contract is in
// include/neural_render.h; tests/fit_ref.py restates it in numpy.
//
// k_fit_grad.  A wave owns whole partial sums: wave w of the grid takes partials w, w + waves, ...
// and, for partial s, the 16-point tiles s, s + S, ... in ascending order, so every chain's order is
// fixed by (n, S) alone and no sum is shared between waves.  Per tile, lane (j, g) = (lane & 15,
// lane >> 4) holds point j and the units 4k + g (register k) of every ReLU layer -- the order a
// v_mfma_f32_16x16x4_f32 result is the next layer's B operand in, forward and backward:
//   forward   nr_mlp16.h's loop on the fit pack; the activations a_l go to LDS as [unit][point] and
//             their masks z > 0 into two words; the final 32 -> 1 chain runs in the point's lane over
//             the staged a_nh, units ascending.
//   residual  e and g (lanes 0-15), to LDS.
//   backward  nr_grad.h's loop on the transposed kernels, seeded with K_last[u] * g; every d_l goes
//             to LDS as [unit][point] as well.
//   weight gradient of layer l: GK_l (32 x 32) = sum over points of a_(l-1) (x) d_l is 2 x 2 tiles
//             of v_mfma_f32_16x16x4_f32 whose k index is the point: A = a_(l-1)[unit rt 16 + j][point
//             4q + g], B = d_l[unit ct 16 + j][point 4q + g], k-step q = 0..3.  The MFMA is an fmaf
//             chain over k ascending, so one accumulator's chain runs over the points 4q + k in
//             ascending order, tile after tile.  The [unit][point] staging stores point 4q + g at
//             position 4g + q: a lane's four k-steps are one ds_read_b128, and the 64 lanes of a
//             store or a load cover 64 or 256 consecutive floats (no bank conflict).  That is the
//             one transpose per layer and tile: through LDS, not lane swaps -- the activations have
//             to outlive the backward pass anyway, and held in registers they are 64 more beside
//             the ~130 accumulators.
//             The input layer is one row tile: rows x, y, z and a row of ones, whose result is GB_0
//             (fmaf(1, d, acc) = acc + d in one rounding).
//   bias gradients GB_l (l >= 1), GK_last, GB_last, SS: lane u & 31 sums its unit's 16 staged values in
//             point order on the VALU (16 adds per layer against 8 more MFMAs and 8 more
//             accumulators for a row of ones).
// Accumulators per wave at nh = 7: 7 x 16 + 8 (MFMA tiles) + 7 + 3 = 130 registers per lane, live for
// the whole partial.  One 4-wave workgroup per CU (one wave per SIMD, the whole 512-entry register
// file): the packs (57.6 KB at nh = 7) and four waves' staging (18.4 KB each) are 131 KB of the 160 KB.
#include "nr_mlp16.h"

namespace nr {
namespace {

// the wave's LDS stores before this point are visible to its loads after it (LDS operations of a
// wave complete in order; this keeps the compiler from moving them across)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The masks as nr_mlp16.h and nr_grad.h keep them: an activation is +0 exactly where z <= 0 and
// positive elsewhere, so its bit is min(bits, 1) (v_min_u32, v_lshl_or_b32), and a masked element
// is v AND (0 or ~0 from the bit: v_bfe_i32): +0 exactly.  No constant per bit in a register.
__device__ __forceinline__ uint32_t mark(uint32_t m, float act, int pos) {
    uint32_t b;  // (asm: seen through, the compiler selects between 0 and a constant 1 << pos held in a register)
    asm("v_min_u32_e32 %0, 1, %1" : "=v"(b) : "v"(act));
    return (b << pos) | m;
}
__device__ __forceinline__ float masked(uint32_t m, int pos, float v) {
    return __uint_as_float((uint32_t)__builtin_amdgcn_sbfe((int)m, (uint32_t)pos, 1u) & __float_as_uint(v));
}

// position of point p in a staged row: point 4q + g at 4g + q
__device__ __forceinline__ constexpr int tpos(int p) { return 4 * (p & 3) + (p >> 2); }

__device__ __forceinline__ void load16(const float *p, float (&v)[16]) {
    const float4 *q = reinterpret_cast<const float4 *>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 t = q[i];
        v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
    }
}
__device__ __forceinline__ void load4(const float *p, float (&v)[4]) {
    const float4 t = *reinterpret_cast<const float4 *>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void load8(const float *p, float (&v)[8]) {
    const float4 *q = reinterpret_cast<const float4 *>(p);
    const float4 lo = q[0], hi = q[1];
    v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
}

// one hidden layer's MFMA loop (forward: L = the layer's A operand, b = activations; backward: the
// transposed A operand, b = deltas): c[mt] = rows 16 mt .. 16 mt + 15, chains over k ascending
__device__ __forceinline__ void layer_mfma(const float *L, int lane, const float (&b)[8], f32x4 (&c)[2]) {
    // (an opaque copy of the lane index, tied to the layer's input: the 16 registers of weights are
    // then loaded here -- not hoisted out of the tile loop, and not all layers' at the top of the tile,
    // which is what the scheduler does with a whole register file to itself)
    asm volatile("" : "+v"(lane) : "v"(b[0]));
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
            c[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, b[st], st == 0 ? f32x4{0.0f, 0.0f, 0.0f, 0.0f} : c[mt], 0, 0, 0);
        }
    }
}

template <int NH>
__global__ __launch_bounds__(64 * FIT_WAVES, 1) void k_fit_grad(FitArgs F) {
    constexpr int NHA = NH > 0 ? NH : 1;
    float *sp = reinterpret_cast<float *>(nr_smem16);
    {
        const int4 *src = reinterpret_cast<const int4 *>(F.pack);
        int4 *dst = reinterpret_cast<int4 *>(sp);
        for (int i = threadIdx.x; i < fit_pack_floats(NH) / 4; i += blockDim.x) dst[i] = src[i];
    }
    __syncthreads();
    const float *s = sp, *sb = sp + fit_bwd(NH);
    const int lane = lane_id(), j = lane & 15, g = lane >> 4, u = lane & 31;
    float *AS = sp + fit_pack_floats(NH) + (threadIdx.x >> 6) * fit_wave_floats(NH);
    float *DS = AS + (NH + 1) * 512, *XS = DS + 512, *EG = XS + 64;
    const int pj = 4 * (j & 3) + (j >> 2);  // tpos(j)
    const int st_off = g * 16 + pj;         // + 64 k: unit 4k + g, point j
    const int rd_off = j * 16 + 4 * g;      // + 256 tile: unit 16 tile + j, points 4q + g
    const uint32_t n = (uint32_t)F.n, ntiles = (n + 15u) >> 4, S = (uint32_t)F.S;
    const uint32_t wave =
        (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (uint32_t)FIT_WAVES + (threadIdx.x >> 6)));
    const uint32_t waves = (uint32_t)__builtin_amdgcn_readfirstlane((int)(gridDim.x * (uint32_t)FIT_WAVES));
    const float clampv = F.clamp;
    const int P = fit_params(NH);
    const float *wf = s + pk_final(NH);  // K_last [32], B_last

    for (uint32_t part = wave; part < S; part += waves) {
        f32x4 gk[NHA][2][2], gk0[2];
        float gb[NHA], gkl = 0.0f, gbl = 0.0f, ss = 0.0f;
#pragma unroll
        for (int l = 0; l < NHA; ++l) {
            gb[l] = 0.0f;
#pragma unroll
            for (int q = 0; q < 4; ++q) gk[l][q >> 1][q & 1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
        gk0[0] = gk0[1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

        for (uint32_t t = part; t < ntiles; t += S) {
            const uint32_t p = t * 16u + (uint32_t)j;
            const bool live = p < n;
            float x = 0.0f, y = 0.0f, z = 0.0f, yt = 0.0f;
            if (live) {
                const float *xp = F.X + (size_t)p * 3;
                x = xp[0]; y = xp[1]; z = xp[2];
                yt = F.Y[p];
            }
            // ---- forward
            const float bt = g == 0 ? x : (g == 1 ? y : (g == 2 ? z : 0.0f));  // B[k = g][point j]
            wave_lds_sync();  // (the previous tile's loads of XS, EG, AS, DS)
            XS[g * 16 + pj] = g == 3 ? 1.0f : bt;
            uint32_t mk[2] = {0u, 0u};
            float a[8];
            f32x4 c[2];
            {
                c[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(s[PK_L0W + lane], bt, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
                c[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(s[PK_L0W + 64 + lane], bt, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
                float bias[8];
                load8(s + PK_L0B + g * 8, bias);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    a[k] = fmaxf(c[k >> 2][k & 3] + bias[k], 0.0f);
                    mk[0] = mark(mk[0], a[k], k);
                    AS[64 * k + st_off] = a[k];
                }
            }
#pragma unroll
            for (int jl = 0; jl < NH; ++jl) {
                const float *L = s + PK_HID + jl * PK_HID_STRIDE;
                layer_mfma(L, lane, a, c);
                float bias[8];
                load8(L + 1024 + g * 8, bias);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    a[k] = fmaxf(c[k >> 2][k & 3] + bias[k], 0.0f);
                    mk[(jl + 1) >> 2] = mark(mk[(jl + 1) >> 2], a[k], 8 * ((jl + 1) & 3) + k);
                    AS[(jl + 1) * 512 + 64 * k + st_off] = a[k];
                }
            }
            // (opaque: seen through, the mask words are dropped and the activations themselves are
            // kept in registers until the backward pass, 8 per layer)
            asm volatile("" : "+v"(mk[0]), "+v"(mk[1]));
            wave_lds_sync();
            // the final layer in the point's lane (all four lane groups: the same point, the same bits)
            float v = 0.0f;
            {
                const float *an = AS + NH * 512 + pj;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    float w[4];
                    load4(wf + 4 * q, w);
#pragma unroll
                    for (int i = 0; i < 4; ++i) v = __builtin_fmaf(w[i], an[(4 * q + i) * 16], v);
                }
                v = v + wf[32];
            }
            // ---- residual
            float vc = v;
            bool inside = true;
            if (clampv > 0.0f) {
                vc = fminf(fmaxf(v, -clampv), clampv);
                inside = v > -clampv && v < clampv;
            }
            const float e = live ? vc - yt : 0.0f;
            const float gv = inside ? e : 0.0f;
            if (g == 0) {
                EG[pj] = e;
                EG[16 + pj] = gv;
                if (live && F.value) F.value[p] = v;
            }
            // ---- backward, with each layer's weight gradient as soon as its deltas exist
            float d[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float kg = wf[4 * k + g] * gv;
                d[k] = masked(mk[NH >> 2], 8 * (NH & 3) + k, kg);
            }
#pragma unroll
            for (int l = NH; l >= 0; --l) {
                // d = d_l (unit 4k + g, point j)
                wave_lds_sync();  // (the loads of DS for layer l + 1)
#pragma unroll
                for (int k = 0; k < 8; ++k) DS[64 * k + st_off] = d[k];
                wave_lds_sync();
                // (the operand offset tied to this layer's deltas: the loads of the staged activations
                // are then issued here, not right after the forward pass, 8 registers per layer early)
                int ro = rd_off;
                asm volatile("" : "+v"(ro) : "v"(d[0]));
                float b4[2][4];
                load4(DS + ro, b4[0]);
                load4(DS + 256 + ro, b4[1]);
                if (l == NH) {
                    // the last layer's sums: GK_last[u], GB_last, SS over the tile's points ascending
                    float av[16], ev[16], gg[16];
                    load16(AS + NH * 512 + u * 16, av);
                    load16(EG, ev);
                    load16(EG + 16, gg);
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        gkl = __builtin_fmaf(av[tpos(q)], gg[tpos(q)], gkl);
                        gbl = gbl + gg[tpos(q)];
                        ss = __builtin_fmaf(ev[tpos(q)], ev[tpos(q)], ss);
                    }
                }
                if (l >= 1) {
                    float a4[2][4];
                    load4(AS + (l - 1) * 512 + ro, a4[0]);
                    load4(AS + (l - 1) * 512 + 256 + ro, a4[1]);
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                            for (int ct = 0; ct < 2; ++ct)
                                gk[l >= 1 ? l - 1 : 0][rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                                    a4[rt][q], b4[ct][q], gk[l >= 1 ? l - 1 : 0][rt][ct], 0, 0, 0);
                    float dv[16];
                    load16(DS + u * 16, dv);
#pragma unroll
                    for (int q = 0; q < 16; ++q) gb[l >= 1 ? l - 1 : 0] = gb[l >= 1 ? l - 1 : 0] + dv[tpos(q)];
                    // d_(l-1) = m_(l-1) ? K_l d_l : +0
                    layer_mfma(sb + (l - 1) * 1024, lane, d, c);
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        d[k] = masked(mk[(l - 1) >> 2], 8 * ((l - 1) & 3) + k, c[k >> 2][k & 3]);
                } else {
                    float a4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (j < 4) load4(XS + ro, a4);
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int ct = 0; ct < 2; ++ct)
                            gk0[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[q], b4[ct][q], gk0[ct], 0, 0, 0);
                }
            }
        }

        // ---- flush: partial `part` in flat parameter order, then SS.  (The lane's offset is formed
        // here from an opaque copy of the lane index: hoisted out of the partial loop, the stores'
        // 64-bit offsets held two registers per store for the kernel's life.)
        float *o = F.partial + (size_t)part * (size_t)(P + 1);
        uint32_t fl = (uint32_t)lane;
        asm volatile("" : "+v"(fl));
        const uint32_t fj = fl & 15u, fg = fl >> 4;
        if (fg == 0) {
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
                for (int r = 0; r < 3; ++r) o[fj + (uint32_t)(r * 32 + ct * 16)] = gk0[ct][r];
                o[fj + (uint32_t)(fit_off_b(0) + ct * 16)] = gk0[ct][3];
            }
        }
        const uint32_t fo = fg * 128u + fj;  // row 4g of a row tile, column j of a column tile
#pragma unroll
        for (int l = 1; l <= NH; ++l) {
            float *ol = o + fit_off_k(l);
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) ol[fo + (uint32_t)((rt * 16 + r) * 32 + ct * 16)] = gk[l - 1][rt][ct][r];
            if (fl < 32u) ol[fl + 1024u] = gb[l - 1];
        }
        if (fl < 32u) o[fl + (uint32_t)fit_off_k(NH + 1)] = gkl;
        if (fl == 0u) {
            o[fit_off_k(NH + 1) + 32] = gbl;
            o[P] = ss;
        }
    }
}

// where parameter idx (flat order) lives in the fit pack: one forward slot, and for a hidden
// kernel one backward slot
__device__ __forceinline__ void fit_scatter(float *pack, int nh, int idx, float w) {
    if (idx < 96) {
        const int kk = idx >> 5, uout = idx & 31;
        const int mt = uout >> 4, i = 4 * (uout & 3) + ((uout >> 2) & 3);
        pack[PK_L0W + mt * 64 + kk * 16 + i] = w;
        return;
    }
    if (idx < 128) {
        const int un = idx - 96;
        pack[PK_L0B + (un & 3) * 8 + (un >> 2)] = w;
        return;
    }
    const int r = idx - 128, l = r / 1056;
    if (l < nh) {
        const int q = r - l * 1056;
        if (q < 1024) {
            const int uin = q >> 5, uout = q & 31;
            {
                const int mt = uout >> 4, i = 4 * (uout & 3) + ((uout >> 2) & 3), m = 2 * (uin >> 2) + mt, kk = uin & 3;
                pack[PK_HID + l * PK_HID_STRIDE + ((m >> 2) * 64 + kk * 16 + i) * 4 + (m & 3)] = w;
            }
            {
                const int mt = uin >> 4, i = 4 * (uin & 3) + ((uin >> 2) & 3), m = 2 * (uout >> 2) + mt, kk = uout & 3;
                pack[fit_bwd(nh) + l * 1024 + ((m >> 2) * 64 + kk * 16 + i) * 4 + (m & 3)] = w;
            }
        } else {
            const int un = q - 1024;
            pack[PK_HID + l * PK_HID_STRIDE + 1024 + (un & 3) * 8 + (un >> 2)] = w;
        }
        return;
    }
    pack[pk_final(nh) + (r - nh * 1056)] = w;  // K_last[u] at u, B_last at 32
}

// 16 sums x FIT_CHUNKS chunks per workgroup: thread (chunk c, sum i) adds its chunk's partials in
// ascending order; the threads of chunk 0 then add the chunk sums in ascending order and finish.
__global__ __launch_bounds__(16 * FIT_CHUNKS) void k_fit_update(FitUpdArgs U) {
    __shared__ float cs[FIT_CHUNKS][17];
    const int P = fit_params(U.nh);
    const int i = threadIdx.x & 15, c = threadIdx.x >> 4;
    const int idx = blockIdx.x * 16 + i;
    if (U.mode != FIT_MODE_PACK) {
        const int per = (U.S + FIT_CHUNKS - 1) / FIT_CHUNKS;
        const int s0 = c * per, s1 = min(s0 + per, U.S);
        float acc = 0.0f;
        if (idx <= P) {
            const float *q = U.partial + idx;
            for (int sidx = s0; sidx < s1; ++sidx) acc = acc + q[(size_t)sidx * (size_t)(P + 1)];
        }
        cs[c][i] = acc;
        __syncthreads();
    }
    if (c != 0 || idx > P) return;
    float G = 0.0f;
    if (U.mode != FIT_MODE_PACK) {
        float T = 0.0f;
#pragma unroll
        for (int k = 0; k < FIT_CHUNKS; ++k) T = T + cs[k][i];
        G = T * U.inv_n;
    }
    if (idx == P) {
        if (U.mode != FIT_MODE_PACK && U.loss) U.loss[0] = G;
        return;
    }
    if (U.mode == FIT_MODE_GRADIENT) {
        if (U.grad) U.grad[idx] = G;
        return;
    }
    float th = U.theta[idx];
    if (U.mode == FIT_MODE_ADAM) {
        const float m = U.beta1 * U.m[idx] + U.omb1 * G;
        const float v = U.beta2 * U.v[idx] + U.omb2 * (G * G);
        th = th - (U.a_t * m) / (__builtin_sqrtf(v) + U.eps);
        U.m[idx] = m;
        U.v[idx] = v;
        U.theta[idx] = th;
    }
    fit_scatter(U.pack, U.nh, idx, th);
}

template <int NH>
hipError_t launch_fit_grad_nh(const FitArgs &F, int grid, hipStream_t st) {
    const int sm = fit_lds_bytes(NH);
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_fit_grad<NH>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, sm);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fit_grad<NH>, dim3(grid), dim3(64 * FIT_WAVES), sm, st, F);
    return hipGetLastError();
}

}  // namespace

int fit_lds_bytes(int nh) { return 4 * (fit_pack_floats(nh) + FIT_WAVES * fit_wave_floats(nh)); }

hipError_t launch_fit_grad(const FitArgs &F, int grid, hipStream_t st) {
    switch (F.nh) {
        case 0: return launch_fit_grad_nh<0>(F, grid, st);
        case 1: return launch_fit_grad_nh<1>(F, grid, st);
        case 2: return launch_fit_grad_nh<2>(F, grid, st);
        case 3: return launch_fit_grad_nh<3>(F, grid, st);
        case 4: return launch_fit_grad_nh<4>(F, grid, st);
        case 5: return launch_fit_grad_nh<5>(F, grid, st);
        case 6: return launch_fit_grad_nh<6>(F, grid, st);
        case 7: return launch_fit_grad_nh<7>(F, grid, st);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_fit_update(const FitUpdArgs &U, hipStream_t st) {
    const int grid = (fit_params(U.nh) + 1 + 15) / 16;
    hipLaunchKernelGGL(k_fit_update, dim3(grid), dim3(16 * FIT_CHUNKS), 0, st, U);
    return hipGetLastError();
}

}  // namespace nr
