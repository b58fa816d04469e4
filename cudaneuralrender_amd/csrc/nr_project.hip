// nr_project.hip -- projection of points onto a level set of the network (nr_project_points):
// damped Newton steps along the analytic gradient, p <- p - g (v - iso) / (g . g), iterated in one
// persistent launch until |v - iso| <= tol.
//
// The evaluation is k_grad's (nr_grad.h mlp16_grad: the fp32 forward with its masks and the backward
// pass on the transposed kernels, both packs staged in LDS once per workgroup).  Around it:
//   * a wave holds up to 64 points in its lanes, all state in registers, and refills its free lanes
//     from a device-side point cursor (one atomic per wave per refill, the positions dealt by
//     ballot / mbcnt, as k_query's rays);
//   * a point writes only its own output slots, and nothing it computes depends on another point
//     (the tiles' columns are independent, and the wave-uniform choice between the clamped and the
//     add + max form is between bit-identical forms; free lanes evaluate the finite point 0), so
//     the outputs are the same for any n, order, split into calls, grid or occupancy;
//   * once the cursor is past n a wave packs its live points into the lowest tiles whenever that
//     lowers the tile count (ds_bpermute, the tracer's tail).
// Termination is structural: a point retires after at most max_iters + 1 evaluations, the cursor
// only grows, and a wave ends when the cursor is past n and no lane is live.  No wave waits for
// another.
#include "nr_grad.h"

namespace nr {

// refill once this many lanes are free (k_query's value), or the wave is empty
constexpr int NR_PROJ_REFILL_MIN = 4;

template <int IN0>
__global__ __launch_bounds__(64 * NR_GRAD_WAVES, NR_GRAD_WAVES / 2) void k_project(ProjArgs P, MlpArgs M) {
    {
        const int4 *src = reinterpret_cast<const int4 *>(P.gb);
        int4 *dst = reinterpret_cast<int4 *>(nr_smem16 + M.pk_bytes);
        for (int i = threadIdx.x; i < P.gb_bytes / 16; i += blockDim.x) dst[i] = src[i];
    }
    Smem16 S = stage16<NR_PRECISION_FP32, true>(M);  // (its __syncthreads covers the copy above)
    const float *sb = reinterpret_cast<const float *>(nr_smem16 + M.pk_bytes);
    M.in0 = IN0;
    const int lane = lane_id();
    const uint32_t n = (uint32_t)P.n;
    bool qempty = false;
    F3 p = mk3(0, 0, 0), p0 = mk3(0, 0, 0);
    float w = 0.0f;
    uint32_t idx = 0;
    int it = -1;       // steps the lane's point has taken; -1: no point
    bool neg = false;  // r0 < 0
    uint32_t nevals = 0, nconv = 0;
    int maxev = 0;
    while (true) {
        qempty = __builtin_amdgcn_readfirstlane((int)qempty) != 0;
        // ---- refill free lanes from the point cursor
        if (!qempty) {
            const uint64_t freem = __ballot(it < 0);
            const uint32_t nfree = (uint32_t)__popcll(freem);
            if (nfree >= (uint32_t)NR_PROJ_REFILL_MIN) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(P.cursor, nfree);
                base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                // (the cursor stays below 2^32: every wave stops adding once it has seen a value >= n,
                // n <= 2^30, and a grid has far fewer than 2^25 waves of at most 64 each)
                if (base >= n) {
                    qempty = true;
                } else {
                    const uint32_t got = min(nfree, n - base);
                    const uint32_t rank = rank_below(freem);
                    if (it < 0 && rank < got) {
                        idx = base + rank;
                        const float *xp = P.X + (size_t)idx * IN0;
                        p = mk3(xp[0], xp[1], xp[2]);
                        if constexpr (IN0 == 4) w = xp[3];
                        p0 = p;
                        it = 0;
                    }
                }
            }
        }
        uint64_t lm = __ballot(it >= 0);
        if (!lm) {
            if (qempty) break;
            continue;
        }
        uint32_t tmask = tiles_of(lm);
        // ---- tail: pack the live points into the lowest tiles
        if (qempty && P.compact) {
            const int nl = (int)__popcll(lm);
            const int need = (nl + 15) >> 4;
            if (32 - __clz((int)tmask) > need) {
                const int src = select_bit(lm, lane < nl ? lane : 0);
                p = mk3(__shfl(p.x, src), __shfl(p.y, src), __shfl(p.z, src));
                p0 = mk3(__shfl(p0.x, src), __shfl(p0.y, src), __shfl(p0.z, src));
                if constexpr (IN0 == 4) w = __shfl(w, src);
                idx = (uint32_t)__shfl((int)idx, src);
                neg = __shfl((int)neg, src) != 0;
                const int it_src = __shfl(it, src);
                it = lane < nl ? it_src : -1;
                if (it < 0) { p = mk3(0.0f, 0.0f, 0.0f); w = 0.0f; }
                lm = __ballot(it >= 0);
                tmask = (1u << need) - 1u;
            }
        }
        // ---- value and gradient of every live point, then the test and one Newton step per point
        float g[4];
        const float v = mlp16_grad(M, S.s32, sb, w, p.x, p.y, p.z, tmask, g);
        nevals += (uint32_t)__popcll(lm);
        if (nevals >= (1u << 30)) {
            if (lane == 0) atomicAdd(P.stats + 0, (unsigned long long)nevals);
            nevals = 0;
        }
        bool conv = false;
        if (it >= 0) {
            const F3 gv = mk3(g[0], g[1], g[2]);
            const float r = v - P.iso;
            if (it == 0) neg = r < 0.0f;
            int status = -1;
            if (__builtin_fabsf(r) <= P.tol) {
                status = NR_PROJ_CONVERGED;
            } else if (it == P.max_iters) {
                status = NR_PROJ_LIMIT;
            } else {
                const float gg = dot3(gv, gv);
                if (!(gg > 0.0f)) {
                    status = NR_PROJ_FLAT;
                } else {
                    float t = r / gg;
                    if (P.max_step > 0.0f) {
                        const float m = __builtin_fabsf(r) / sqrtf(gg);
                        if (m > P.max_step) t = t * (P.max_step / m);
                    }
                    p = mk3(p.x - gv.x * t, p.y - gv.y * t, p.z - gv.z * t);
                    ++it;
                }
            }
            if (status >= 0) {  // the point retires: its outputs, all at the final p
                if (P.position) {
                    float *o = P.position + (size_t)idx * 3;
                    o[0] = p.x; o[1] = p.y; o[2] = p.z;
                }
                if (P.value) P.value[idx] = v;
                if (P.normal) {
                    const F3 nrm = normalize3(gv);
                    float *o = P.normal + (size_t)idx * 3;
                    o[0] = nrm.x; o[1] = nrm.y; o[2] = nrm.z;
                }
                if (P.distance) {
                    const F3 dl = mk3(p.x - p0.x, p.y - p0.y, p.z - p0.z);
                    const float d = sqrtf(dot3(dl, dl));
                    P.distance[idx] = neg ? -d : d;
                }
                if (P.iters) P.iters[idx] = it;
                if (P.status) P.status[idx] = status;
                conv = status == NR_PROJ_CONVERGED;
                maxev = max(maxev, it + 1);
                it = -1;
                // a free lane's point stays a finite input of the evaluation
                p = mk3(0.0f, 0.0f, 0.0f);
                w = 0.0f;
            }
        }
        nconv += (uint32_t)__popcll(__ballot(conv));
    }
    // ---- statistics: one set of atomics per wave
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) maxev = max(maxev, __shfl_xor(maxev, off));
    if (lane == 0) {
        if (nevals) atomicAdd(P.stats + 0, (unsigned long long)nevals);
        if (nconv) atomicAdd(P.stats + 1, (unsigned long long)nconv);
        if (maxev) atomicMax(P.stats + 2, (unsigned long long)maxev);
    }
}

int project_lds_bytes(const MlpArgs &M, const ProjArgs &P) { return smem16_bytes(M, NR_PRECISION_FP32, true) + P.gb_bytes; }

hipError_t launch_project(const ProjArgs &P, const MlpArgs &M, int grid, hipStream_t st) {
    const int sm = project_lds_bytes(M, P);
    if (M.in0 == 4) hipLaunchKernelGGL(k_project<4>, dim3(grid), dim3(64 * NR_GRAD_WAVES), sm, st, P, M);
    else hipLaunchKernelGGL(k_project<3>, dim3(grid), dim3(64 * NR_GRAD_WAVES), sm, st, P, M);
    return hipGetLastError();
}

}  // namespace nr
