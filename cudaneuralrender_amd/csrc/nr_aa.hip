// nr_aa.hip -- adaptive supersampled antialiasing (nr_render_aa): the edge pixels of a rendered
// W x H frame are resolved from the S x S pixels they cover in the S W x S H frame of the same view.
//
// Sub-sample (0, 0) of pixel (x, y) is pixel (S x, S y) of the large frame and has the ray of pixel
// (x, y) of the small one ((float)(S x) / (float)(S W) and (float)x / (float)W are the correctly
// rounded quotient of the same rational), so the base frame is nr_render's own and supplies that
// sample.  Three kernels after it:
//   k_aa_detect   one thread per pixel: the edge rule on the base frame's 8-neighbourhood, edge
//                 pixels appended to a list (one atomic per workgroup, block_append2);
//   k_aa_trace    the hot path, k_query's structure: a persistent launch of 4-wave workgroups with
//                 the fp32 pack in LDS, up to 64 rays per wave in its lanes, refilled from a
//                 device-side cursor over edge_count x (S S - 1) sample indices, the tail compacted
//                 into the lowest tiles.  A lane generates the ray of pixel (S x + sx, S y + sy) of
//                 the S W x S H view with initMarcher's arithmetic (pixel_uv with that size's
//                 arguments), marches it with mlp16_fp32 / scene_sdf / singleMarch's step, and a
//                 converged ray waits in a per-wave LDS list for its 16-ray x 4-sample normal
//                 pass, whose colour (shade_color) is added to the edge pixel's accumulator: one
//                 64-bit atomic add of four 16-bit channel fields (8 x 8 x 255 < 2^16).  Background
//                 samples add nothing.  Integer sums: the result does not depend on the order;
//   k_aa_resolve  per listed pixel: (base + accumulated + S S / 2) / (S S) per channel, written
//                 over the base colour.
// The list's order depends on atomics; an entry's position only names its accumulator.
#include "nr_mlp16.h"

namespace nr {

// workgroups per CU k_aa_trace's registers are allocated for (4 waves each)
#ifndef NR_AA_BPC
#define NR_AA_BPC 3
#endif
// how the cursor's sample indices are dealt: 0 = a pixel's S S - 1 samples together (neighbouring
// lanes march neighbouring rays and add into the same accumulator), 1 = sample k of every edge
// pixel before sample k + 1 (a pixel's samples spread over waves).  A/B: profiles/aa_bench.txt.
#ifndef NR_AA_SPREAD
#define NR_AA_SPREAD 0
#endif
// refill once this many lanes are free (k_query's value), or the wave is empty
constexpr int NR_AA_REFILL_MIN = 4;
// converged rays waiting for their colour, per wave: a pass leaves at most 15, an iteration adds
// at most 64
constexpr int ASTASH = 80;
static_assert(16 - 1 + 64 <= ASTASH, "the per-wave list of converged rays");

// Rule 2: pixel (x, y) is an edge iff a pixel of its 8-neighbourhood inside the image differs from
// it by more than `contrast` in some channel.
__device__ __forceinline__ int channel_diff(uint32_t a, uint32_t b) {
    int m = 0;
#pragma unroll
    for (int sh = 0; sh < 32; sh += 8) {
        const int d = (int)((a >> sh) & 0xffu) - (int)((b >> sh) & 0xffu);
        m = max(m, d < 0 ? -d : d);
    }
    return m;
}

__global__ __launch_bounds__(256) void k_aa_detect(AaArgs X) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long npix = (long)X.W * X.H;
    bool edge = false;
    if (t < npix) {
        if (X.full) {
            edge = true;
        } else {
            const int y = (int)udiv_r((uint32_t)t, (uint32_t)X.W, X.inv_w), x = (int)(t - (long)y * X.W);
            const uint32_t c = X.out[t];
            int m = 0;
            for (int dy = -1; dy <= 1; ++dy) {
                const int ny = y + dy;
                if (ny < 0 || ny >= X.H) continue;
                for (int dx = -1; dx <= 1; ++dx) {
                    const int nx = x + dx;
                    if (nx < 0 || nx >= X.W) continue;
                    m = max(m, channel_diff(c, X.out[(long)ny * X.W + nx]));
                }
            }
            edge = m > X.contrast;
        }
    }
    const Slots sl = block_append2(edge, X.count, false, nullptr);
    if (edge) X.list[sl.a] = (uint32_t)t;
}

// A: the S W x S H frame's arguments as nr_render builds them (W, H, reciprocals, view, colouring)
__global__ __launch_bounds__(256, NR_AA_BPC) void k_aa_trace(RenderArgs A, AaArgs X, MlpArgs M) {
    Smem16 S = stage16<NR_PRECISION_FP32, true>(M);
    __shared__ float4 stash_p[4][ASTASH];  // {p.xyz, accumulator index}
    __shared__ float4 stash_d[4][ASTASH];  // {d.xyz, -}
    const int lane = lane_id();
    const int wid = threadIdx.x >> 6;
    const int q4 = lane & 3;
    const float fr = (float)A.frame;
    const double zoff = sphere_zoff(A.frame);
    const uint32_t n = X.nsub;
    int nstash = 0;
    bool qempty = false;
    F3 p = mk3(0, 0, 0), d = mk3(0, 0, 0);
    float tfar = 0.0f;
    uint32_t idx = 0;  // the ray's accumulator (its pixel's position in the edge list)
    int it = -1, maxit = 0;  // it: iterations of the lane's ray; -1: no ray
    uint32_t nsteps = 0, nhit = 0, nconv = 0;
    while (true) {
        nstash = __builtin_amdgcn_readfirstlane(nstash);
        qempty = __builtin_amdgcn_readfirstlane((int)qempty) != 0;
        // ---- refill free lanes from the sample cursor
        if (!qempty) {
            // (a wave fills its lowest X.take lanes only: fewer tiles per iteration when the launch has
            // fewer samples than ray slots)
            const uint64_t freem = __ballot(it < 0 && lane < X.take);
            const uint32_t nfree = (uint32_t)__popcll(freem);
            if (nfree >= (uint32_t)NR_AA_REFILL_MIN) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(X.cursor, nfree);
                base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                if (base >= n) {
                    qempty = true;
                } else {
                    const uint32_t got = min(nfree, n - base);
                    const uint32_t rank = rank_below(freem);
                    bool hit = false;
                    if (it < 0 && lane < X.take && rank < got) {
                        // sample i: sub-sample k = 1 .. S S - 1 of the edge list's entry e (a pixel's
                        // samples are dealt together)
                        const uint32_t i = base + rank;
#if NR_AA_SPREAD
                        const uint32_t k0 = udiv_r(i, X.nedge, X.inv_nedge);
                        const uint32_t e = i - k0 * X.nedge, k = k0 + 1u;
#else
                        const uint32_t e = udiv_r(i, (uint32_t)X.per, X.inv_per);
                        const uint32_t k = i - e * (uint32_t)X.per + 1u;
#endif
                        const uint32_t sy = udiv_r(k, (uint32_t)X.S, X.inv_s), sx = k - sy * (uint32_t)X.S;
                        const uint32_t pix = X.list[e];
                        const uint32_t py = udiv_r(pix, (uint32_t)X.W, X.inv_w), px = pix - py * (uint32_t)X.W;
                        const int x = (int)(px * (uint32_t)X.S + sx), y = (int)(py * (uint32_t)X.S + sy);
                        const float *V = A.inv_view;
                        const F3 o = mk3(dot4(0.0f, 0.0f, 0.0f, 1.0f, V + 0), dot4(0.0f, 0.0f, 0.0f, 1.0f, V + 4),
                                         dot4(0.0f, 0.0f, 0.0f, 1.0f, V + 8));
                        const float u = pixel_uv(x, A.W, A.rcp_w);
                        const float v = pixel_uv(y, A.H, A.rcp_h);
                        const F3 dn = normalize3(mk3(u, v, -2.0f));
                        const F3 dd = mk3(dot3(dn, mk3(V[0], V[1], V[2])), dot3(dn, mk3(V[4], V[5], V[6])),
                                          dot3(dn, mk3(V[8], V[9], V[10])));
                        float tn, tf;
                        hit = intersect_bounding(o, dd, tn, tf);
                        if (hit && A.max_steps > 0) {
                            if (tn < 0.0f) tn = 0.0f;
                            p = add3(o, mul3s(dd, tn));
                            d = dd;
                            tfar = tf;  // (the reference does not subtract tnear)
                            idx = e;
                            it = 0;
                        }
                    }
                    nhit += (uint32_t)__popcll(__ballot(hit));
                }
            }
        }
        // ---- colours of the waiting converged rays: 16 rays x 4 tetrahedron samples per pass,
        // lane 4 k + q = sample q of ray k.  Once the cursor is drained a partial pass waits for
        // the wave's last marching ray, as in k_trace.
        const uint64_t lm0 = __ballot(it >= 0);
        while (nstash >= 16 || (qempty && nstash > 0 && !lm0)) {
            const int nb = min(16, nstash);
            const int k = lane >> 2;
            const int e = nstash - nb + (k < nb ? k : 0);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            const float4 sp = stash_p[wid][e];
            // tetrahedron point q (c_tet, :38-43): x = +1 for q = 0, 3; y = +1 for q = 2, 3; z = +1 for q = 1, 3
            int qo = q4;
            asm volatile("" : "+v"(qo));
            const F3 tp = mk3((qo == 0 || qo == 3) ? 1.0f : -1.0f, qo >= 2 ? 1.0f : -1.0f, (qo & 1) ? 1.0f : -1.0f);
            const F3 pq = add3(mk3(sp.x, sp.y, sp.z), mul3s(tp, NORMAL_EPSILON));
            const uint32_t smask = (1u << ((4 * nb + 15) >> 4)) - 1u;
            const float sdf = mlp16_fp32(M, S.s32, fr, pq.x, pq.y, pq.z, smask);
            const F3 cq = mul3s(tp, scene_sdf(pq, sdf, A.scene, zoff));
            const F3 c1 = quad_bcast3_1(cq), c2 = quad_bcast3_2(cq), c3 = quad_bcast3_3(cq);
            if (k < nb && q4 == 0) {
                const F3 nrm = normalize3(add3(add3(add3(cq, c1), c2), c3));
                const float4 sd = stash_d[wid][e];
                const uint32_t c = shade_color(A, A.normal, nrm, mk3(sd.x, sd.y, sd.z));
                // four 16-bit fields r, g, b, a: no field carries into the next below 2^16 / 255 samples
                const unsigned long long f = (unsigned long long)(c & 0xffu) | ((unsigned long long)((c >> 8) & 0xffu) << 16) |
                                             ((unsigned long long)((c >> 16) & 0xffu) << 32) |
                                             ((unsigned long long)(c >> 24) << 48);
                if (f) atomicAdd(X.accum + __float_as_uint(sp.w), f);
            }
            nconv += (uint32_t)nb;
            nstash -= nb;
        }
        uint64_t lm = lm0;
        if (!lm) {
            if (qempty && nstash == 0) break;
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
                d = mk3(__shfl(d.x, src), __shfl(d.y, src), __shfl(d.z, src));
                tfar = __shfl(tfar, src);
                idx = (uint32_t)__shfl((int)idx, src);
                const int it_src = __shfl(it, src);
                it = lane < nl ? it_src : -1;
                if (it < 0) p = mk3(0.0f, 0.0f, 0.0f);
                lm = __ballot(it >= 0);
                tmask = (1u << need) - 1u;
            }
        }
        // ---- the MLP on every live point, then one sphere-trace step per ray
        const float sdf = mlp16_fp32(M, S.s32, fr, p.x, p.y, p.z, tmask);
        nsteps += (uint32_t)__popcll(lm);
        if (nsteps >= (1u << 30)) {
            if (lane == 0) atomicAdd(X.stats + 0, (unsigned long long)nsteps);
            nsteps = 0;
        }
        bool conv = false;
        if (it >= 0) {
            const float ts = scene_sdf(p, sdf, A.scene, zoff);
            tfar -= ts;
            int used = 0;  // iterations this ray consumed, if it ends now (k_trace's count)
            if (tfar <= 0) {
                used = it + 1;  // background: adds nothing
            } else {
                p = add3(p, mul3s(d, ts));
                if (ts < MARCHING_EPSILON) {
                    // converged: coloured by the reference's next iteration when there is one (:446-457)
                    conv = it + 1 < A.max_steps;
                    used = conv ? it + 2 : it + 1;
                } else if (++it >= A.max_steps) {
                    used = A.max_steps;  // iteration cap: adds nothing
                }
            }
            if (used) {  // the ray ended
                maxit = max(maxit, used);
                it = -1;
            }
        }
        const uint64_t cm = __ballot(conv);
        if (conv) {
            const int slot = nstash + (int)rank_below(cm);
            stash_p[wid][slot] = make_float4(p.x, p.y, p.z, __uint_as_float(idx));
            stash_d[wid][slot] = make_float4(d.x, d.y, d.z, 0.0f);
        }
        nstash += (int)__popcll(cm);
        // a free lane's point stays a finite MLP input
        if (it < 0) p = mk3(0.0f, 0.0f, 0.0f);
    }
    // ---- statistics: one set of atomics per wave
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) maxit = max(maxit, __shfl_xor(maxit, off));
    if (lane == 0) {
        if (nsteps) atomicAdd(X.stats + 0, (unsigned long long)nsteps);
        if (nhit) atomicAdd(X.stats + 1, (unsigned long long)nhit);
        if (maxit) atomicMax(X.stats + 2, (unsigned long long)maxit);
        if (nconv) atomicAdd(X.stats + 3, (unsigned long long)nconv);
    }
}

// Rule 3 for the listed pixels: the base colour is sample (0, 0), the accumulator holds the others
__global__ __launch_bounds__(256) void k_aa_resolve(AaArgs X) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= X.nedge) return;
    const uint32_t pix = X.list[e];
    const uint32_t b = X.out[pix];
    const unsigned long long a = X.accum[e];
    const uint32_t ss = (uint32_t)(X.S * X.S);
    uint32_t r = 0;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        const uint32_t sum = ((b >> (8 * ch)) & 0xffu) + (uint32_t)((a >> (16 * ch)) & 0xffffu);
        r |= ((sum + ss / 2) / ss) << (8 * ch);
    }
    X.out[pix] = r;
}

hipError_t launch_aa_detect(const AaArgs &X, hipStream_t st) {
    const long npix = (long)X.W * X.H;
    hipLaunchKernelGGL(k_aa_detect, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, X);
    return hipGetLastError();
}

hipError_t launch_aa_trace(const RenderArgs &A, const AaArgs &X, const MlpArgs &M, int grid, hipStream_t st) {
    const int sm = smem16_bytes(M, NR_PRECISION_FP32, true);
    hipLaunchKernelGGL(k_aa_trace, dim3(grid), dim3(256), sm, st, A, X, M);
    return hipGetLastError();
}

hipError_t launch_aa_resolve(const AaArgs &X, hipStream_t st) {
    hipLaunchKernelGGL(k_aa_resolve, dim3((X.nedge + 255) / 256), dim3(256), 0, st, X);
    return hipGetLastError();
}

}  // namespace nr
