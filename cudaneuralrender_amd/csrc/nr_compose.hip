// nr_compose.hip -- composed scenes: several networks, each rotated, moved and scaled, folded by
// union and subtraction into one signed-distance field, and the persistent sphere tracer, the point
// sampler and the colouring pass over that field (nr_compose_*; the contract is in
// include/neural_render.h).
//
// k_compose is k_query's tracer (nr_query.hip: lanes refilled from a ray cursor, the tail packed
// into the lowest tiles, converged rays waiting in a per-wave LDS list for 16-ray x 4-sample normal
// passes, one set of statistics atomics per wave) with the composed field (nr_compose_field.h) in
// the place of one MLP:
//   * every distinct fp32 pack is staged once per workgroup into dynamic LDS, back to back (four of
//     them are about 122 KB: one workgroup per CU, launched with 12 waves so that a SIMD holds three);
//   * the part table is in the kernarg segment, the part loop is wave-uniform, and a part's network
//     runs only when some live lane of the wave is inside that part's bound, on the tiles that hold
//     such a lane: a ray far from a part costs that part no MLP evaluation;
//   * a ray writes only its own slots and nothing it computes depends on another ray (the MLP's
//     tiles are column-independent, its clamped and add + max forms bit-identical within the
//     bound), so the outputs are the same for any workgroup size, grid or ray order.
#include "nr_compose_field.h"
#include "nr_mlp16.h"

namespace nr {

// refill once this many lanes are free (k_query's value), or the wave is empty
constexpr int NR_COMPOSE_REFILL_MIN = 4;
// converged rays waiting for their normal, per wave: a pass leaves at most 15, an iteration adds at most 64
constexpr int CSTASH = 80;
static_assert(16 - 1 + 64 <= CSTASH, "the per-wave list of converged rays");

// k_compose<true>'s copy of the view in LDS
struct ComposeView {
    float V[12];
    float rcp_w, rcp_h;
    int W, H;
    double inv_w;
};

// GBUF: ray i is the ray of pixel (i % W, i / W) of the view C.inv_view (k_query<GBUF>'s ray
// generation) instead of (origins[i], dirs[i]).
template <bool GBUF>
__global__ __launch_bounds__(NR_COMPOSE_MAX_THREADS) void k_compose(ComposeArgs C) {
    // the view and the image size live in LDS behind the per-wave lists, read at a refill: held in
    // scalar registers across the march, they were spilled as register tuples
    ComposeView *sview = reinterpret_cast<ComposeView *>(nr_smem16 + C.pack_bytes + (blockDim.x >> 6) * CSTASH * (int)sizeof(float4));
    if (GBUF && threadIdx.x < 12) sview->V[threadIdx.x] = C.inv_view[threadIdx.x];
    if (GBUF && threadIdx.x == 0) {
        sview->rcp_w = C.rcp_w; sview->rcp_h = C.rcp_h;
        sview->W = C.W; sview->H = C.H;
        sview->inv_w = C.inv_w;
    }
    const float *lds = compose_stage(C);  // (its __syncthreads covers the view)
    const int lane = lane_id();
    const int wid = threadIdx.x >> 6;
    float4 *stash = reinterpret_cast<float4 *>(nr_smem16 + C.pack_bytes) + wid * CSTASH;  // {p.xyz, ray index}
    const int q4 = lane & 3;
    const float fr = (float)C.frame;
    const uint32_t n = (uint32_t)C.n;
    const bool normals = C.normal != nullptr;
    int nstash = 0;
    bool qempty = false;
    F3 p = mk3(0, 0, 0), d = mk3(0, 0, 0);
    float tfar = 0.0f, tnear = 0.0f, travel = 0.0f;
    uint32_t idx = 0;
    int it = -1, maxit = 0;  // it: iterations of the lane's ray; -1: no ray
    uint32_t nsteps = 0, nhit = 0, nconv = 0;
    FieldCount march{0, 0, 0}, other{0, 0, 0};
    // a ray's results; the normal of a hit is written by its normal pass
    auto finish = [&](uint32_t i, int status, int steps, float t, F3 pos, int own) {
        if (C.status) C.status[i] = status;
        if (C.steps) C.steps[i] = steps;
        if (C.t) C.t[i] = t;
        if (C.position) {
            float *o = C.position + (size_t)i * 3;
            o[0] = pos.x; o[1] = pos.y; o[2] = pos.z;
        }
        if (C.normal && status != NR_RAY_HIT) {
            float *o = C.normal + (size_t)i * 3;
            o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f;
        }
        if (C.part) C.part[i] = own;
    };
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
        // ---- refill free lanes from the ray cursor
        if (!qempty) {
            const uint64_t freem = __ballot(it < 0);
            const uint32_t nfree = (uint32_t)__popcll(freem);
            if (nfree >= (uint32_t)NR_COMPOSE_REFILL_MIN) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(C.cursor, nfree);
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
                            const float *V = sview->V;
                            const int W = sview->W, H = sview->H;
                            const int y = (int)udiv_r(i, (uint32_t)W, sview->inv_w), x = (int)i - y * W;
                            o = mk3(dot4(0.0f, 0.0f, 0.0f, 1.0f, V + 0), dot4(0.0f, 0.0f, 0.0f, 1.0f, V + 4),
                                    dot4(0.0f, 0.0f, 0.0f, 1.0f, V + 8));
                            const float u = pixel_uv(x, W, sview->rcp_w);
                            const float v = pixel_uv(y, H, sview->rcp_h);
                            const F3 dn = normalize3(mk3(u, v, -2.0f));
                            dd = mk3(dot3(dn, mk3(V[0], V[1], V[2])), dot3(dn, mk3(V[4], V[5], V[6])),
                                     dot3(dn, mk3(V[8], V[9], V[10])));
                        } else {
                            const float *po = C.origins + (size_t)i * 3, *pd = C.dirs + (size_t)i * 3;
                            o = mk3(po[0], po[1], po[2]);
                            dd = mk3(pd[0], pd[1], pd[2]);
                        }
                        float tn, tf;
                        hit = compose_intersect(o, dd, C, tn, tf);
                        if (hit) {
                            if (tn < 0.0f) tn = 0.0f;
                            p = add3(o, mul3s(dd, tn));
                            d = dd;
                            tfar = tf - tn;  // the remaining interval
                            tnear = tn;
                            travel = 0.0f;
                            idx = i;
                            it = 0;
                        } else {
                            finish(i, NR_RAY_MISS, 0, 0.0f, mk3(0.0f, 0.0f, 0.0f), -1);
                        }
                    }
                    nhit += (uint32_t)__popcll(__ballot(hit));
                }
            }
        }
        // ---- normals of the waiting converged rays: 16 rays x 4 tetrahedron samples per pass,
        // lane 4 k + q = sample q of ray k.  Once the cursor is drained a partial pass waits for
        // the wave's last marching ray, as in k_query.
        const uint64_t lm0 = __ballot(it >= 0);
        while (nstash >= 16 || (qempty && nstash > 0 && !lm0)) {
            const int nb = min(16, nstash);
            const int k = lane >> 2;
            const int e = nstash - nb + (k < nb ? k : 0);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            const float4 sp = stash[e];
            const F3 cq = compose_tet_term(C, lds, fr, mk3(sp.x, sp.y, sp.z), q4, k < nb, other);
            const F3 c1 = quad_bcast3_1(cq), c2 = quad_bcast3_2(cq), c3 = quad_bcast3_3(cq);
            if (k < nb && q4 == 0) {
                const F3 nrm = normalize3(add3(add3(add3(cq, c1), c2), c3));
                float *o = C.normal + (size_t)__float_as_uint(sp.w) * 3;
                o[0] = nrm.x; o[1] = nrm.y; o[2] = nrm.z;
            }
            nstash -= nb;
        }
        uint64_t lm = lm0;
        if (!lm) {
            if (qempty && nstash == 0) break;
            continue;
        }
        // ---- tail: pack the live rays into the lowest tiles
        if (qempty) {
            const int nl = (int)__popcll(lm);
            const int need = (nl + 15) >> 4;
            if (__popc(tiles_of(lm)) > need) {
                const int src = select_bit(lm, lane < nl ? lane : 0);
                p = mk3(__shfl(p.x, src), __shfl(p.y, src), __shfl(p.z, src));
                d = mk3(__shfl(d.x, src), __shfl(d.y, src), __shfl(d.z, src));
                tfar = __shfl(tfar, src);
                tnear = __shfl(tnear, src);
                travel = __shfl(travel, src);
                idx = (uint32_t)__shfl((int)idx, src);
                const int it_src = __shfl(it, src);
                it = lane < nl ? it_src : -1;
                lm = __ballot(it >= 0);
            }
        }
        // ---- the field at every live point, then one sphere-trace step per ray
        int own;
        const float ts = compose_field(C, lds, fr, p, it >= 0, own, march);
        nsteps += (uint32_t)__popcll(lm);
        if (nsteps >= (1u << 26)) flush();
        bool conv = false;
        if (it >= 0) {
            tfar -= ts;
            int status = -1, used = 0;
            if (tfar <= 0) {
                status = NR_RAY_ESCAPED;
                used = it + 1;
            } else {
                p = add3(p, mul3s(d, ts));
                travel += ts;
                if (ts < MARCHING_EPSILON) {
                    status = it + 1 < C.max_steps ? NR_RAY_HIT : NR_RAY_LIMIT;
                    used = it + 1;
                } else if (++it >= C.max_steps) {
                    status = NR_RAY_LIMIT;
                    used = C.max_steps;
                }
            }
            if (status >= 0) {  // the ray ended
                const bool h = status == NR_RAY_HIT;
                finish(idx, status, used, h ? tnear + travel : 0.0f, h ? p : mk3(0.0f, 0.0f, 0.0f), h ? own : -1);
                conv = h;
                maxit = max(maxit, used);
                it = -1;
            }
        }
        const uint64_t cm = __ballot(conv);
        if (conv && normals) stash[nstash + (int)rank_below(cm)] = make_float4(p.x, p.y, p.z, __uint_as_float(idx));
        if (normals) nstash += (int)__popcll(cm);
        nconv += (uint32_t)__popcll(cm);
    }
    // ---- statistics: one set of atomics per wave
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) maxit = max(maxit, __shfl_xor(maxit, off));
    flush();
    if (lane == 0) {
        if (nhit) atomicAdd(C.stats + 1, (unsigned long long)nhit);
        if (maxit) atomicMax(C.stats + 2, (unsigned long long)maxit);
        if (nconv) atomicAdd(C.stats + 3, (unsigned long long)nconv);
    }
}

// value and owner of the field at n points: a wave takes 64 consecutive points at a time
__global__ __launch_bounds__(256, 3) void k_compose_sample(ComposeArgs C) {
    const float *lds = compose_stage(C);
    const int lane = lane_id();
    const float fr = (float)C.frame;
    const long nchunks = (C.n + 63) >> 6;
    const long wave = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long nwaves = (long)gridDim.x * (blockDim.x >> 6);
    FieldCount cnt{0, 0, 0};
    for (long ch = wave; ch < nchunks; ch += nwaves) {
        const long i = (ch << 6) + lane;
        const bool live = i < C.n;
        F3 p = mk3(0.0f, 0.0f, 0.0f);
        if (live) {
            const float *pp = C.points + (size_t)i * 3;
            p = mk3(pp[0], pp[1], pp[2]);
        }
        int own;
        const float v = compose_field(C, lds, fr, p, live, own, cnt);
        if (live) {
            if (C.value) C.value[i] = v;
            if (C.owner) C.owner[i] = own;
        }
        if (cnt.pairs >= (1u << 30)) {
            if (lane == 0) atomicAdd(C.stats + 4, (unsigned long long)cnt.pairs);
            cnt.pairs = 0;
        }
    }
    if (lane == 0) {
        if (cnt.pairs) atomicAdd(C.stats + 4, (unsigned long long)cnt.pairs);
        if (cnt.evals) atomicAdd(C.stats + 5, (unsigned long long)cnt.evals);
        if (cnt.skips) atomicAdd(C.stats + 6, (unsigned long long)cnt.skips);
    }
}

// one thread per pixel: shade_color on the geometry buffer's normal and the pixel's regenerated ray
// direction (k_light_resolve's base colour) for a HIT, 0 for anything else
__global__ __launch_bounds__(256) void k_compose_color(RenderArgs A, const int32_t *status, const float *normal) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)A.W * A.H) return;
    uint32_t c = 0;
    if (status[t] == NR_RAY_HIT) {
        const float *pn = normal + (size_t)t * 3;
        const F3 nrm = mk3(pn[0], pn[1], pn[2]);
        const float *V = A.inv_view;
        const int y = (int)udiv_r((uint32_t)t, (uint32_t)A.W, A.inv_w), x = (int)t - y * A.W;
        const float u = pixel_uv(x, A.W, A.rcp_w);
        const float v = pixel_uv(y, A.H, A.rcp_h);
        const F3 dn = normalize3(mk3(u, v, -2.0f));
        const F3 dd = mk3(dot3(dn, mk3(V[0], V[1], V[2])), dot3(dn, mk3(V[4], V[5], V[6])),
                          dot3(dn, mk3(V[8], V[9], V[10])));
        c = shade_color(A, A.normal, nrm, dd);
    }
    A.out[t] = c;
}

int compose_lds_bytes(const ComposeArgs &C, int threads) { return C.pack_bytes + (threads >> 6) * CSTASH * (int)sizeof(float4) + (int)sizeof(ComposeView); }

hipError_t launch_compose(const ComposeArgs &C, int grid, int threads, hipStream_t st) {
    const int sm = compose_lds_bytes(C, threads);
    const void *fn = C.origins ? reinterpret_cast<const void *>(k_compose<false>) : reinterpret_cast<const void *>(k_compose<true>);
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, sm);
    if (e != hipSuccess) return e;
    if (C.origins) hipLaunchKernelGGL(k_compose<false>, dim3(grid), dim3(threads), sm, st, C);
    else hipLaunchKernelGGL(k_compose<true>, dim3(grid), dim3(threads), sm, st, C);
    return hipGetLastError();
}

hipError_t launch_compose_sample(const ComposeArgs &C, int grid, hipStream_t st) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_compose_sample),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, C.pack_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_compose_sample, dim3(grid), dim3(256), C.pack_bytes, st, C);
    return hipGetLastError();
}

hipError_t launch_compose_color(const RenderArgs &A, const int32_t *status, const float *normal, hipStream_t st) {
    const long n = (long)A.W * A.H;
    hipLaunchKernelGGL(k_compose_color, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, A, status, normal);
    return hipGetLastError();
}

}  // namespace nr
