// nr_light.hip -- ambient occlusion and soft shadows for a frame (nr_render_lit): every pixel of
// the W x H geometry buffer (k_query<true>'s status, position and normal, nr_query.hip) gets an
// occlusion factor and a shadow factor from the same field, and the base colour times the two.
//
// Two kernels after the geometry buffer:
//   k_light_trace    the hot path, k_query's structure: a persistent launch of 4-wave workgroups with
//                    the fp32 pack in LDS, up to 64 shadow rays per wave in its lanes, refilled from
//                    a device-side cursor over the pixel indices (one atomic per wave per refill),
//                    the tail compacted into the lowest tiles.  A lane that takes a pixel that is
//                    not a hit writes ao = shadow = 1 and is free again.  A lane that takes a hit
//                    reads p and n, appends them to a per-wave LDS list for the occlusion pass and
//                    either writes its shadow at once (no shadows wanted, the surface faces away
//                    from the light, the shadow ray misses the bounding sphere) or becomes the
//                    shadow ray o = p + n * bias, d = L.  The ray is marched as k_query marches one
//                    (intersect_bounding, mlp16_fp32, scene_sdf, singleMarch's step) with the running
//                    minimum res of k * ts / (tnear + travel) on top.  d is the same for every ray:
//                    it stays in the kernel's scalar arguments.
//                    The occlusion pass has the normal pass's shape: 16 pixels x 4 samples, lane
//                    4 k + q = sample q of pixel k at p + n * ((q + 1) * ao_step); the quad
//                    broadcasts bring the four terms to lane q = 0, which sums them in order and
//                    writes ao.  It runs when 16 pixels wait or the cursor is drained;
//   k_light_resolve  one thread per pixel: the base colour (shade_color on the geometry buffer's
//                    normal and the pixel's regenerated ray direction) times
//                    f = ao * (ambient + (1 - ambient) * (shadow * ndl)) per channel.
// A pixel writes only its own slots and nothing it computes depends on another pixel, so the
// outputs are the same bits for any grid, occupancy or order in which the pixels are dealt.
#include "nr_mlp16.h"

namespace nr {

// workgroups per CU k_light_trace's registers are allocated for (4 waves each)
#ifndef NR_LIGHT_BPC
#define NR_LIGHT_BPC 3
#endif
// refill once this many lanes are free (k_query's value), or the wave is empty
constexpr int NR_LIGHT_REFILL_MIN = 4;
// hit pixels waiting for their occlusion pass, per wave: a pass leaves at most 15, a refill adds
// at most 64
constexpr int LSTASH = 80;
static_assert(16 - 1 + 64 <= LSTASH, "the per-wave list of hit pixels");

// rule 2: dd = dot3(n, L), ndl = dd > 0 ? dd : 0 (a NaN normal gives 0)
__device__ __forceinline__ float light_ndl(F3 n, const LightArgs &X) {
    const float dd = dot3(n, mk3(X.dir[0], X.dir[1], X.dir[2]));
    return dd > 0.0f ? dd : 0.0f;
}

__global__ __launch_bounds__(256, NR_LIGHT_BPC) void k_light_trace(LightArgs X, MlpArgs M) {
    Smem16 S = stage16<NR_PRECISION_FP32, true>(M);
    __shared__ float4 stash_p[4][LSTASH];  // {p.xyz, pixel}
    __shared__ float4 stash_n[4][LSTASH];  // {n.xyz, -}
    const int lane = lane_id();
    const int wid = threadIdx.x >> 6;
    const int q4 = lane & 3;
    const float fr = (float)X.frame;
    const double zoff = sphere_zoff(X.frame);
    const uint32_t n = (uint32_t)X.n;
    const bool ao_on = X.ao_strength > 0.0f;
    const F3 d = mk3(X.dir[0], X.dir[1], X.dir[2]);  // wave-uniform: scalar registers
    int nstash = 0;
    bool qempty = false;
    F3 p = mk3(0, 0, 0);
    float tfar = 0.0f, tnear = 0.0f, travel = 0.0f, res = 1.0f;
    uint32_t idx = 0;
    int it = -1, maxit = 0;  // it: iterations of the lane's shadow ray; -1: no ray
    uint32_t nsteps = 0;
    while (true) {
        nstash = __builtin_amdgcn_readfirstlane(nstash);
        qempty = __builtin_amdgcn_readfirstlane((int)qempty) != 0;
        // ---- refill free lanes from the pixel cursor
        if (!qempty) {
            const uint64_t freem = __ballot(it < 0);
            const uint32_t nfree = (uint32_t)__popcll(freem);
            if (nfree >= (uint32_t)NR_LIGHT_REFILL_MIN) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(X.cursor, nfree);
                base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                if (base >= n) {
                    qempty = true;
                } else {
                    const uint32_t got = min(nfree, n - base);
                    const uint32_t rank = rank_below(freem);
                    bool surf = false, ray = false;
                    F3 hp = mk3(0, 0, 0), hn = mk3(0, 0, 0);
                    uint32_t i = 0;
                    if (it < 0 && rank < got) {
                        i = base + rank;
                        surf = X.status[i] == NR_RAY_HIT;
                        if (!surf) {  // rule 1
                            X.ao[i] = 1.0f;
                            X.shadow[i] = 1.0f;
                        } else {
                            const float *pp = X.position + (size_t)i * 3, *pn = X.normal + (size_t)i * 3;
                            hp = mk3(pp[0], pp[1], pp[2]);
                            hn = mk3(pn[0], pn[1], pn[2]);
                            if (!ao_on) X.ao[i] = 1.0f;
                            // rule 4: the shadow is known at once, or the lane becomes a shadow ray
                            if (X.shadow_steps == 0) {
                                X.shadow[i] = 1.0f;
                            } else if (!(light_ndl(hn, X) > 0.0f)) {
                                X.shadow[i] = 0.0f;
                            } else {
                                const F3 o = add3(hp, mul3s(hn, X.shadow_bias));
                                float tn, tf;
                                ray = intersect_bounding(o, d, tn, tf);
                                if (ray) {
                                    if (tn < 0.0f) tn = 0.0f;
                                    p = add3(o, mul3s(d, tn));
                                    tfar = tf;  // (the reference does not subtract tnear)
                                    tnear = tn;
                                    travel = 0.0f;
                                    res = 1.0f;
                                    idx = i;
                                    it = 0;
                                } else {
                                    X.shadow[i] = 1.0f;  // MISS
                                }
                            }
                        }
                    }
                    if (ao_on) {
                        const uint64_t sm = __ballot(surf);
                        if (surf) {
                            const int slot = nstash + (int)rank_below(sm);
                            stash_p[wid][slot] = make_float4(hp.x, hp.y, hp.z, __uint_as_float(i));
                            stash_n[wid][slot] = make_float4(hn.x, hn.y, hn.z, 0.0f);
                        }
                        nstash += (int)__popcll(sm);
                    }
                }
            }
        }
        // ---- occlusion of the waiting hit pixels (rule 3): 16 pixels x 4 samples per pass, lane
        // 4 k + q = sample q of pixel k.  A partial pass runs once the cursor is drained: no
        // further pixel can join the list.
        while (nstash >= 16 || (qempty && nstash > 0)) {
            const int nb = min(16, nstash);
            const int k = lane >> 2;
            const int e = nstash - nb + (k < nb ? k : 0);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            const float4 sp = stash_p[wid][e];
            const float4 sn = stash_n[wid][e];
            int qo = q4;
            asm volatile("" : "+v"(qo));
            const float hq = (float)(qo + 1) * X.ao_step;
            const float wq = qo == 0 ? 1.0f : qo == 1 ? 0.5f : qo == 2 ? 0.25f : 0.125f;
            const F3 aq = add3(mk3(sp.x, sp.y, sp.z), mul3s(mk3(sn.x, sn.y, sn.z), hq));
            const uint32_t smask = (1u << ((4 * nb + 15) >> 4)) - 1u;
            const float sdf = mlp16_fp32(M, S.s32, fr, aq.x, aq.y, aq.z, smask);
            const float cq = (hq - scene_sdf(aq, sdf, X.scene, zoff)) * wq;
            const float c1 = quad_bcast<1>(cq), c2 = quad_bcast<2>(cq), c3 = quad_bcast<3>(cq);
            if (k < nb && q4 == 0) {
                const float occ = ((cq + c1) + c2) + c3;
                X.ao[__float_as_uint(sp.w)] = saturatef_(1.0f - X.ao_strength * occ);
            }
            nstash -= nb;
        }
        uint64_t lm = __ballot(it >= 0);
        if (!lm) {
            if (qempty) break;  // (the list is empty: the pass above drained it)
            continue;
        }
        uint32_t tmask = tiles_of(lm);
        // ---- tail: pack the live rays into the lowest tiles
        if (qempty) {
            const int nl = (int)__popcll(lm);
            const int need = (nl + 15) >> 4;
            if (__popc(tmask) > need) {
                const int src = select_bit(lm, lane < nl ? lane : 0);
                p = mk3(__shfl(p.x, src), __shfl(p.y, src), __shfl(p.z, src));
                tfar = __shfl(tfar, src);
                tnear = __shfl(tnear, src);
                travel = __shfl(travel, src);
                res = __shfl(res, src);
                idx = (uint32_t)__shfl((int)idx, src);
                const int it_src = __shfl(it, src);
                it = lane < nl ? it_src : -1;
                if (it < 0) p = mk3(0.0f, 0.0f, 0.0f);
                lm = __ballot(it >= 0);
                tmask = (1u << need) - 1u;
            }
        }
        // ---- the MLP on every live point, then one sphere-trace step per shadow ray
        const float sdf = mlp16_fp32(M, S.s32, fr, p.x, p.y, p.z, tmask);
        nsteps += (uint32_t)__popcll(lm);
        if (nsteps >= (1u << 30)) {
            if (lane == 0) atomicAdd(X.stats + 0, (unsigned long long)nsteps);
            nsteps = 0;
        }
        if (it >= 0) {
            const float ts = scene_sdf(p, sdf, X.scene, zoff);
            // the penumbra term, at the point ts was taken at (dist = 0: the ray's first point when
            // its origin lies inside the bounding sphere -- the bias decides there, not a quotient)
            const float dist = tnear + travel;
            if (dist > 0.0f) {
                const float r = X.shadow_k * ts / dist;
                if (r < res) res = r;
            }
            tfar -= ts;
            float sh = 0.0f;  // HIT and LIMIT: the light is blocked, or not reached
            int used = 0;
            if (tfar <= 0) {  // ESCAPED
                sh = X.shadow_k > 0.0f ? saturatef_(res) : 1.0f;
                used = it + 1;
            } else {
                p = add3(p, mul3s(d, ts));
                travel += ts;
                if (ts < MARCHING_EPSILON) used = it + 1;
                else if (++it >= X.shadow_steps) used = X.shadow_steps;
            }
            if (used) {  // the ray ended
                X.shadow[idx] = sh;
                maxit = max(maxit, used);
                it = -1;
            }
        }
        // a free lane's point stays a finite MLP input
        if (it < 0) p = mk3(0.0f, 0.0f, 0.0f);
    }
    // ---- statistics: one set of atomics per wave
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) maxit = max(maxit, __shfl_xor(maxit, off));
    if (lane == 0) {
        if (nsteps) atomicAdd(X.stats + 0, (unsigned long long)nsteps);
        if (maxit) atomicMax(X.stats + 1, (unsigned long long)maxit);
    }
}

// Rule 5 for every pixel: base(x, y) is shade_color on the geometry buffer's normal and the pixel's
// ray direction (k_query's GBUF arithmetic), which is nr_render's fp32 pixel.
__global__ __launch_bounds__(256) void k_light_resolve(RenderArgs A, LightArgs X) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= X.n) return;
    uint32_t c = 0;
    if (X.status[t] == NR_RAY_HIT) {
        const float *pn = X.normal + (size_t)t * 3;
        const F3 nrm = mk3(pn[0], pn[1], pn[2]);
        const float *V = A.inv_view;
        const int y = (int)udiv_r((uint32_t)t, (uint32_t)A.W, A.inv_w), x = (int)t - y * A.W;
        const float u = pixel_uv(x, A.W, A.rcp_w);
        const float v = pixel_uv(y, A.H, A.rcp_h);
        const F3 dn = normalize3(mk3(u, v, -2.0f));
        const F3 dd = mk3(dot3(dn, mk3(V[0], V[1], V[2])), dot3(dn, mk3(V[4], V[5], V[6])),
                          dot3(dn, mk3(V[8], V[9], V[10])));
        const uint32_t b = shade_color(A, A.normal, nrm, dd);
        const float f = X.ao[t] * (X.ambient + (1.0f - X.ambient) * (X.shadow[t] * light_ndl(nrm, X)));
        c = b & 0xff000000u;
#pragma unroll
        for (int sh = 0; sh < 24; sh += 8) {
            const float ch = (float)((b >> sh) & 0xffu) * f;
            c |= (uint32_t)(ch < 255.0f ? ch : 255.0f) << sh;  // (f > 1 only for a light longer than 1)
        }
    }
    A.out[t] = c;
}

hipError_t launch_light_trace(const LightArgs &X, const MlpArgs &M, int grid, hipStream_t st) {
    const int sm = smem16_bytes(M, NR_PRECISION_FP32, true);
    hipLaunchKernelGGL(k_light_trace, dim3(grid), dim3(256), sm, st, X, M);
    return hipGetLastError();
}

hipError_t launch_light_resolve(const RenderArgs &A, const LightArgs &X, hipStream_t st) {
    hipLaunchKernelGGL(k_light_resolve, dim3((unsigned)((X.n + 255) / 256)), dim3(256), 0, st, A, X);
    return hipGetLastError();
}

}  // namespace nr
