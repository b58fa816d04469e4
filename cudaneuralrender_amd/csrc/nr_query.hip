// nr_query.hip -- ray queries and geometry buffers: the persistent sphere tracer for rays the
// caller chooses (nr_trace_rays) or the pixel rays of the context's view (nr_render_gbuffer),
// returning per ray the status, the iteration count, the ray parameter, the hit point and the
// world normal instead of a colour.
//
// The arithmetic is k_trace's fp32 instance, through the same device functions (nr_device.h,
// nr_mlp16.h): intersect_bounding for the entry, mlp16_fp32 over the tiles that hold a live lane,
// scene_sdf and singleMarch's step (volumeRender_kernel.cu:416-477), and surfaceNormal's four
// tetrahedral samples (:361-377) in 16-ray x 4-sample passes.  One persistent launch per call:
//   * a wave holds up to 64 rays in its lanes and refills free lanes from a device-side ray
//     cursor (one atomic per wave per refill, the positions dealt by ballot / mbcnt);
//   * a ray writes only its own output slots, and nothing it computes depends on another ray
//     (the MLP's tiles are column-independent, the scene's wave-wide screens choose between
//     bit-identical forms), so the outputs are the same for any grid, ray order or chunking;
//   * converged rays wait in a per-wave LDS list for their normal; a pass runs when 16 wait or
//     the wave drains.  Without a normal output no pass runs at all (occlusion rays).
#include "nr_mlp16.h"

namespace nr {

// workgroups per CU k_query's registers are allocated for (4 waves each)
#ifndef NR_QUERY_BPC
#define NR_QUERY_BPC 3
#endif
// refill once this many lanes are free (k_trace's fp32 value), or the wave is empty
constexpr int NR_QUERY_REFILL_MIN = 4;
// converged rays waiting for their normal, per wave: a pass leaves at most 15, an iteration adds
// at most 64
constexpr int QSTASH = 80;
static_assert(16 - 1 + 64 <= QSTASH, "the per-wave list of converged rays");

// GBUF: ray i is the ray of pixel (i % W, i / W) of the view Q.inv_view (gen_hit's arithmetic,
// initMarcher :293-358) instead of (origins[i], dirs[i]).
template <bool GBUF>
__global__ __launch_bounds__(256, NR_QUERY_BPC) void k_query(QueryArgs Q, MlpArgs M) {
    Smem16 S = stage16<NR_PRECISION_FP32, true>(M);
    __shared__ float4 stash[4][QSTASH];  // {p.xyz, ray index}
    const int lane = lane_id();
    const int wid = threadIdx.x >> 6;
    const int q4 = lane & 3;
    const float fr = (float)Q.frame;
    const double zoff = sphere_zoff(Q.frame);
    const uint32_t n = (uint32_t)Q.n;
    const bool normals = Q.normal != nullptr;
    int nstash = 0;
    bool qempty = false;
    F3 p = mk3(0, 0, 0), d = mk3(0, 0, 0);
    float tfar = 0.0f, tnear = 0.0f, travel = 0.0f;
    uint32_t idx = 0;
    int it = -1, maxit = 0;  // it: iterations of the lane's ray; -1: no ray
    uint32_t nsteps = 0, nhit = 0, nconv = 0;
    // a ray's results; the normal of a hit is written by its normal pass
    auto finish = [&](uint32_t i, int status, int steps, float t, F3 pos) {
        if (Q.status) Q.status[i] = status;
        if (Q.steps) Q.steps[i] = steps;
        if (Q.t) Q.t[i] = t;
        if (Q.position) {
            float *o = Q.position + (size_t)i * 3;
            o[0] = pos.x; o[1] = pos.y; o[2] = pos.z;
        }
        if (Q.normal && status != NR_RAY_HIT) {
            float *o = Q.normal + (size_t)i * 3;
            o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f;
        }
    };
    while (true) {
        nstash = __builtin_amdgcn_readfirstlane(nstash);
        qempty = __builtin_amdgcn_readfirstlane((int)qempty) != 0;
        // ---- refill free lanes from the ray cursor
        if (!qempty) {
            const uint64_t freem = __ballot(it < 0);
            const uint32_t nfree = (uint32_t)__popcll(freem);
            if (nfree >= (uint32_t)NR_QUERY_REFILL_MIN) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(Q.cursor, nfree);
                base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                if (base >= n) {
                    qempty = true;
                } else {
                    const uint32_t got = min(nfree, n - base);
                    const uint32_t rank = rank_below(freem);
                    bool hit = false;
                    if (it < 0 && rank < got) {
                        const uint32_t i = base + rank;
                        F3 o, dd;
                        if constexpr (GBUF) {
                            const float *V = Q.inv_view;
                            const int y = (int)udiv_r(i, (uint32_t)Q.W, Q.inv_w), x = (int)i - y * Q.W;
                            o = mk3(dot4(0.0f, 0.0f, 0.0f, 1.0f, V + 0), dot4(0.0f, 0.0f, 0.0f, 1.0f, V + 4),
                                    dot4(0.0f, 0.0f, 0.0f, 1.0f, V + 8));
                            const float u = pixel_uv(x, Q.W, Q.rcp_w);
                            const float v = pixel_uv(y, Q.H, Q.rcp_h);
                            const F3 dn = normalize3(mk3(u, v, -2.0f));
                            dd = mk3(dot3(dn, mk3(V[0], V[1], V[2])), dot3(dn, mk3(V[4], V[5], V[6])),
                                     dot3(dn, mk3(V[8], V[9], V[10])));
                        } else {
                            const float *po = Q.origins + (size_t)i * 3, *pd = Q.dirs + (size_t)i * 3;
                            o = mk3(po[0], po[1], po[2]);
                            dd = mk3(pd[0], pd[1], pd[2]);
                        }
                        float tn, tf;
                        hit = intersect_bounding(o, dd, tn, tf);
                        if (hit) {
                            if (tn < 0.0f) tn = 0.0f;
                            p = add3(o, mul3s(dd, tn));
                            d = dd;
                            tfar = tf;  // (the reference does not subtract tnear)
                            tnear = tn;
                            travel = 0.0f;
                            idx = i;
                            it = 0;
                        } else {
                            finish(i, NR_RAY_MISS, 0, 0.0f, mk3(0.0f, 0.0f, 0.0f));
                        }
                    }
                    nhit += (uint32_t)__popcll(__ballot(hit));
                }
            }
        }
        // ---- normals of the waiting converged rays: 16 rays x 4 tetrahedron samples per pass,
        // lane 4 k + q = sample q of ray k.  Once the cursor is drained a partial pass waits for
        // the wave's last marching ray, as in k_trace.
        const uint64_t lm0 = __ballot(it >= 0);
        while (nstash >= 16 || (qempty && nstash > 0 && !lm0)) {
            const int nb = min(16, nstash);
            const int k = lane >> 2;
            const int e = nstash - nb + (k < nb ? k : 0);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            const float4 sp = stash[wid][e];
            // tetrahedron point q (c_tet, :38-43): x = +1 for q = 0, 3; y = +1 for q = 2, 3; z = +1 for q = 1, 3
            int qo = q4;
            asm volatile("" : "+v"(qo));
            const F3 tp = mk3((qo == 0 || qo == 3) ? 1.0f : -1.0f, qo >= 2 ? 1.0f : -1.0f, (qo & 1) ? 1.0f : -1.0f);
            const F3 pq = add3(mk3(sp.x, sp.y, sp.z), mul3s(tp, NORMAL_EPSILON));
            const uint32_t smask = (1u << ((4 * nb + 15) >> 4)) - 1u;
            const float sdf = mlp16_fp32(M, S.s32, fr, pq.x, pq.y, pq.z, smask);
            const F3 cq = mul3s(tp, scene_sdf(pq, sdf, Q.scene, zoff));
            const F3 c1 = quad_bcast3_1(cq), c2 = quad_bcast3_2(cq), c3 = quad_bcast3_3(cq);
            if (k < nb && q4 == 0) {
                const F3 nrm = normalize3(add3(add3(add3(cq, c1), c2), c3));
                float *o = Q.normal + (size_t)__float_as_uint(sp.w) * 3;
                o[0] = nrm.x; o[1] = nrm.y; o[2] = nrm.z;
            }
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
                tnear = __shfl(tnear, src);
                travel = __shfl(travel, src);
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
            if (lane == 0) atomicAdd(Q.stats + 0, (unsigned long long)nsteps);
            nsteps = 0;
        }
        bool conv = false;
        if (it >= 0) {
            const float ts = scene_sdf(p, sdf, Q.scene, zoff);
            tfar -= ts;
            int status = -1, used = 0;
            if (tfar <= 0) {
                status = NR_RAY_ESCAPED;
                used = it + 1;
            } else {
                p = add3(p, mul3s(d, ts));
                travel += ts;
                if (ts < MARCHING_EPSILON) {
                    // converged: shaded by the reference's next iteration when there is one (:446-457)
                    status = it + 1 < Q.max_steps ? NR_RAY_HIT : NR_RAY_LIMIT;
                    used = it + 1;
                } else if (++it >= Q.max_steps) {
                    status = NR_RAY_LIMIT;
                    used = Q.max_steps;
                }
            }
            if (status >= 0) {  // the ray ended
                const bool h = status == NR_RAY_HIT;
                finish(idx, status, used, h ? tnear + travel : 0.0f, h ? p : mk3(0.0f, 0.0f, 0.0f));
                conv = h;
                maxit = max(maxit, used);
                it = -1;
            }
        }
        const uint64_t cm = __ballot(conv);
        if (conv && normals) stash[wid][nstash + (int)rank_below(cm)] = make_float4(p.x, p.y, p.z, __uint_as_float(idx));
        if (normals) nstash += (int)__popcll(cm);
        nconv += (uint32_t)__popcll(cm);
        // a free lane's point stays a finite MLP input
        if (it < 0) p = mk3(0.0f, 0.0f, 0.0f);
    }
    // ---- statistics: one set of atomics per wave
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) maxit = max(maxit, __shfl_xor(maxit, off));
    if (lane == 0) {
        if (nsteps) atomicAdd(Q.stats + 0, (unsigned long long)nsteps);
        if (nhit) atomicAdd(Q.stats + 1, (unsigned long long)nhit);
        if (maxit) atomicMax(Q.stats + 2, (unsigned long long)maxit);
        if (nconv) atomicAdd(Q.stats + 3, (unsigned long long)nconv);
    }
}

hipError_t launch_query(const QueryArgs &Q, const MlpArgs &M, int grid, hipStream_t st) {
    const int sm = smem16_bytes(M, NR_PRECISION_FP32, true);
    if (Q.origins) hipLaunchKernelGGL(k_query<false>, dim3(grid), dim3(256), sm, st, Q, M);
    else hipLaunchKernelGGL(k_query<true>, dim3(grid), dim3(256), sm, st, Q, M);
    return hipGetLastError();
}

}  // namespace nr
