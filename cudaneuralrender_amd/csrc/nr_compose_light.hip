// nr_compose_light.hip -- ambient occlusion and shadows of a composed scene (nr_compose_render_lit):
// every pixel of the W x H geometry buffer k_compose<true> left (status, position, normal) gets an
// occlusion factor and a shadow factor from the composed field, so a part shades the others and a
// cut-out lies in the dark of what is around it.
//
// k_compose_light is k_light_trace (nr_light.hip: lanes refilled from a cursor over the pixel
// indices, hit pixels waiting in a per-wave LDS list for 16-pixel x 4-sample occlusion passes, the
// tail packed into the lowest tiles, the light direction in the kernel's scalar arguments) with the
// composed field (nr_compose_field.h) in the place of one MLP, in k_compose's workgroup: the packs
// staged once into dynamic LDS, 4, 8 or 12 waves, the part loop wave-uniform and a part's network
// run only for the waves with a live lane inside that part's bound.  The shadow ray follows the
// composed ray rule (the world bound's entry, tfar reduced by tnear) with nr_render_lit's running
// minimum on top, and the owner the field returns at the converging step of a ray that ends HIT is
// the part that blocked the light.  The compositing pass is k_light_resolve, unchanged.
// A pixel writes only its own slots and nothing it computes depends on another pixel, so the
// outputs are the same bits for any workgroup size, grid or order in which the pixels are dealt.
#include "nr_compose_field.h"
#include "nr_mlp16.h"

namespace nr {

// refill once this many lanes are free (k_light_trace's value), or the wave is empty
constexpr int NR_CLIGHT_REFILL_MIN = 4;
// hit pixels waiting for their occlusion pass, per wave: a pass leaves at most 15, a refill adds at most 64
constexpr int LSTASH = 80;
static_assert(16 - 1 + 64 <= LSTASH, "the per-wave list of hit pixels");

__global__ __launch_bounds__(NR_COMPOSE_MAX_THREADS) void k_compose_light(ComposeArgs C, ComposeLightArgs X) {
    const float *lds = compose_stage(C);
    const int lane = lane_id();
    const int wid = threadIdx.x >> 6;
    // behind the packs: per wave {p.xyz, pixel}, then {n.xyz, -}
    float4 *stash_p = reinterpret_cast<float4 *>(nr_smem16 + C.pack_bytes) + wid * (2 * LSTASH);
    float4 *stash_n = stash_p + LSTASH;
    const int q4 = lane & 3;
    const float fr = (float)C.frame;
    const uint32_t n = (uint32_t)C.n;
    const bool ao_on = X.ao_strength > 0.0f;
    const F3 d = mk3(X.dir[0], X.dir[1], X.dir[2]);  // wave-uniform: scalar registers
    int nstash = 0;
    bool qempty = false;
    F3 p = mk3(0, 0, 0);
    float tfar = 0.0f, tnear = 0.0f, travel = 0.0f, res = 1.0f;
    uint32_t idx = 0;
    int it = -1, maxit = 0;  // it: iterations of the lane's shadow ray; -1: no ray
    uint32_t nsteps = 0;
    FieldCount march{0, 0, 0}, other{0, 0, 0};
    auto flush = [&]() {
        if (lane == 0) {
            if (nsteps) atomicAdd(C.stats + 0, (unsigned long long)nsteps);
            if (march.pairs) atomicAdd(C.stats + 4, (unsigned long long)march.pairs);
            if (march.evals + other.evals) atomicAdd(C.stats + 5, (unsigned long long)march.evals + other.evals);
            if (march.skips + other.skips) atomicAdd(C.stats + 6, (unsigned long long)march.skips + other.skips);
        }
        nsteps = 0;
        march = FieldCount{0, 0, 0};
        other = FieldCount{0, 0, 0};
    };
    while (true) {
        nstash = __builtin_amdgcn_readfirstlane(nstash);
        qempty = __builtin_amdgcn_readfirstlane((int)qempty) != 0;
        // ---- refill free lanes from the pixel cursor
        if (!qempty) {
            const uint64_t freem = __ballot(it < 0);
            const uint32_t nfree = (uint32_t)__popcll(freem);
            if (nfree >= (uint32_t)NR_CLIGHT_REFILL_MIN) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(C.cursor, nfree);
                base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                if (base >= n) {
                    qempty = true;
                } else {
                    const uint32_t got = min(nfree, n - base);
                    const uint32_t rank = rank_below(freem);
                    bool surf = false;
                    F3 hp = mk3(0, 0, 0), hn = mk3(0, 0, 0);
                    uint32_t i = 0;
                    if (it < 0 && rank < got) {
                        i = base + rank;
                        surf = X.status[i] == NR_RAY_HIT;
                        // the occluder of a pixel is -1 unless its shadow ray ends HIT
                        if (X.occluder) X.occluder[i] = -1;
                        if (!surf) {  // rule 1
                            X.ao[i] = 1.0f;
                            X.shadow[i] = 1.0f;
                        } else {
                            const float *pp = X.position + (size_t)i * 3, *pn = X.normal + (size_t)i * 3;
                            hp = mk3(pp[0], pp[1], pp[2]);
                            hn = mk3(pn[0], pn[1], pn[2]);
                            if (!ao_on) X.ao[i] = 1.0f;
                            // rule 4: the shadow is known at once, or the lane becomes a shadow ray
                            const float dd = dot3(hn, d);
                            if (X.shadow_steps == 0) {
                                X.shadow[i] = 1.0f;
                            } else if (!(dd > 0.0f)) {
                                X.shadow[i] = 0.0f;
                            } else {
                                const F3 o = add3(hp, mul3s(hn, X.shadow_bias));
                                float tn, tf;
                                if (compose_intersect(o, d, C, tn, tf)) {
                                    if (tn < 0.0f) tn = 0.0f;
                                    p = add3(o, mul3s(d, tn));
                                    tfar = tf - tn;  // the remaining interval (the composed ray rule)
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
                            stash_p[slot] = make_float4(hp.x, hp.y, hp.z, __uint_as_float(i));
                            stash_n[slot] = make_float4(hn.x, hn.y, hn.z, 0.0f);
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
            const float4 sp = stash_p[e];
            const float4 sn = stash_n[e];
            int qo = q4;
            asm volatile("" : "+v"(qo));
            const float hq = (float)(qo + 1) * X.ao_step;
            const float wq = qo == 0 ? 1.0f : qo == 1 ? 0.5f : qo == 2 ? 0.25f : 0.125f;
            const F3 aq = add3(mk3(sp.x, sp.y, sp.z), mul3s(mk3(sn.x, sn.y, sn.z), hq));
            int own;
            const float sq = compose_field(C, lds, fr, aq, k < nb, own, other);
            const float cq = (hq - sq) * wq;
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
        // ---- tail: pack the live rays into the lowest tiles
        if (qempty) {
            const int nl = (int)__popcll(lm);
            const int need = (nl + 15) >> 4;
            if (__popc(tiles_of(lm)) > need) {
                const int src = select_bit(lm, lane < nl ? lane : 0);
                p = mk3(__shfl(p.x, src), __shfl(p.y, src), __shfl(p.z, src));
                tfar = __shfl(tfar, src);
                tnear = __shfl(tnear, src);
                travel = __shfl(travel, src);
                res = __shfl(res, src);
                idx = (uint32_t)__shfl((int)idx, src);
                const int it_src = __shfl(it, src);
                it = lane < nl ? it_src : -1;
                lm = __ballot(it >= 0);
            }
        }
        // ---- the field at every live point, then one sphere-trace step per shadow ray
        int own;
        const float ts = compose_field(C, lds, fr, p, it >= 0, own, march);
        nsteps += (uint32_t)__popcll(lm);
        if (nsteps >= (1u << 26)) flush();
        if (it >= 0) {
            // the penumbra term, at the point ts was taken at (dist = 0: the ray's first point when
            // its origin lies inside the bound -- the bias decides there, not a quotient)
            const float dist = tnear + travel;
            if (dist > 0.0f) {
                const float r = X.shadow_k * ts / dist;
                if (r < res) res = r;
            }
            tfar -= ts;
            float sh = 0.0f;  // HIT and LIMIT: the light is blocked, or not reached
            int used = 0, occ = -1;
            if (tfar <= 0) {  // ESCAPED
                sh = X.shadow_k > 0.0f ? saturatef_(res) : 1.0f;
                used = it + 1;
            } else {
                p = add3(p, mul3s(d, ts));
                travel += ts;
                if (ts < MARCHING_EPSILON) {
                    used = it + 1;
                    if (used < X.shadow_steps) occ = own;  // HIT (LIMIT otherwise)
                } else if (++it >= X.shadow_steps) {
                    used = X.shadow_steps;
                }
            }
            if (used) {  // the ray ended
                X.shadow[idx] = sh;
                if (X.occluder && occ >= 0) X.occluder[idx] = occ;
                maxit = max(maxit, used);
                it = -1;
            }
        }
    }
    // ---- statistics: one set of atomics per wave
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) maxit = max(maxit, __shfl_xor(maxit, off));
    flush();
    if (lane == 0 && maxit) atomicMax(C.stats + 2, (unsigned long long)maxit);
}

int compose_light_lds_bytes(const ComposeArgs &C, int threads) {
    return C.pack_bytes + (threads >> 6) * 2 * LSTASH * (int)sizeof(float4);
}

hipError_t launch_compose_light(const ComposeArgs &C, const ComposeLightArgs &X, int grid, int threads, hipStream_t st) {
    const int sm = compose_light_lds_bytes(C, threads);
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_compose_light),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, sm);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_compose_light, dim3(grid), dim3(threads), sm, st, C, X);
    return hipGetLastError();
}

}  // namespace nr
