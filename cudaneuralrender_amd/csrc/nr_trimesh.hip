// nr_trimesh.hip -- signed distance from points to a triangle mesh (nr_trimesh_distance): the closest
// triangle of each point by a walk of the host-built hierarchy (nr_trimesh_host.cpp), the closest point
// and feature on it, and the sign from the feature's pseudonormal.  The arithmetic contract is in
// include/neural_render.h; tests/trimesh_ref.py restates it in numpy.
//
// k_trimesh_distance.  A wave owns chunks of 64 consecutive points (chunk w, w + waves, ...), one
// point per lane, and walks the tree once for all of them:
//   * the walk is wave-uniform: one node index, one stack of pending nodes (a few words of LDS per
//     wave, one entry per level at most), and a node's words and a leaf's triangles are read at
//     wave-uniform addresses -- scalar loads, one copy per wave, operands of every lane's VALU work;
//   * each lane forms its own lower bound to a node's box; the wave enters the node while any live
//     lane has bound <= best, and skips it otherwise (the project's idiom: decide per wave, skip
//     what no lane needs).  Of two wanted children the one more lanes are nearer to is entered at
//     once and the other is pushed; a popped node is tested again, since best has shrunk meanwhile;
//   * a leaf's triangles are evaluated by every lane; the winner is the minimum of (d2, original
//     triangle index), so the order of the walk, the leaf size and the hierarchy itself change no
//     bit.  NR_TRIMESH_BRUTE is the same evaluation over all triangles with no walk;
//   * a lane without a point (the tail) or with a non-finite one is not live: it takes no part in
//     any vote and cannot lengthen the walk.
// Every loop is bounded by a count the host fixed: nodes entered <= nnodes, pops <= the stack size,
// a leaf's triangles <= its count.  The closest point, feature and sign are recomputed once per
// point from the winning triangle by the same code.
#include "nr_device.h"
#include "nr_internal.h"
#include "nr_kernels.h"

namespace nr {
namespace {

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 v3(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 vsub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
// the contract's dot: fmaf(u.z, v.z, fmaf(u.y, v.y, u.x * v.x))
__device__ __forceinline__ float vdot(V3 u, V3 v) { return __builtin_fmaf(u.z, v.z, __builtin_fmaf(u.y, v.y, u.x * v.x)); }
__device__ __forceinline__ V3 vfma(V3 e, float t, V3 b) {
    return V3{__builtin_fmaf(e.x, t, b.x), __builtin_fmaf(e.y, t, b.y), __builtin_fmaf(e.z, t, b.z)};
}

// Ericson's region test: the closest point of triangle (a, b, c) to p and the feature it lies on
// (0 face, 1..3 edges AB, BC, CA, 4..6 vertices A, B, C), the regions tested in the header's order.
__device__ __forceinline__ V3 tri_closest(V3 p, V3 a, V3 b, V3 c, int &feature) {
    const V3 ab = vsub(b, a), ac = vsub(c, a), bc = vsub(c, b);
    const V3 ap = vsub(p, a), bp = vsub(p, b), cp = vsub(p, c);
    const float d1 = vdot(ab, ap), d2 = vdot(ac, ap), d3 = vdot(ab, bp), d4 = vdot(ac, bp), d5 = vdot(ab, cp), d6 = vdot(ac, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float e43 = d4 - d3, e56 = d5 - d6;
    int f = 0;
    if (va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f) f = 2;
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) f = 3;
    if (d6 >= 0.0f && d5 <= d6) f = 6;
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) f = 1;
    if (d3 >= 0.0f && d4 <= d3) f = 5;
    if (d1 <= 0.0f && d2 <= 0.0f) f = 4;
    feature = f;
    V3 r = f == 4 ? a : (f == 5 ? b : c);
    if (f < 4) {
        const float num = f == 1 ? d1 : (f == 3 ? d2 : (f == 2 ? e43 : vb));
        const float den = f == 1 ? d1 - d3 : (f == 3 ? d2 - d6 : (f == 2 ? e43 + e56 : (va + vb) + vc));
        const float t = num / den;
        const V3 e = f == 3 ? ac : (f == 2 ? bc : ab);
        r = vfma(e, t, f == 2 ? b : a);
        if (f == 0) {
            const float w = vc / den;
            r = vfma(ac, w, r);
        }
    }
    return r;
}

__device__ __forceinline__ V3 load_v3(const float4 *q) {
    const float4 t = *q;
    return V3{t.x, t.y, t.z};
}

// a lane's lower bound of its squared distance to an (inflated) box, scaled down by 2^-16 of itself
// against the rounding of the bound and of the distances it is compared with
__device__ __forceinline__ float box_bound(V3 p, float4 lo, float4 hi) {
    const float dx = fmaxf(fmaxf(lo.x - p.x, p.x - hi.x), 0.0f);
    const float dy = fmaxf(fmaxf(lo.y - p.y, p.y - hi.y), 0.0f);
    const float dz = fmaxf(fmaxf(lo.z - p.z, p.z - hi.z), 0.0f);
    return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx)) * 0.9999847412109375f;
}

__global__ __launch_bounds__(256) void k_trimesh_distance(const float4 *__restrict__ nodes, const float4 *__restrict__ tris,
                                                          const float *__restrict__ table, TriMeshArgs A) {
    __shared__ int stacks[4][TRIMESH_STACK];
    int *stack = stacks[threadIdx.x >> 6];
    const int lane = lane_id();
    const uint32_t nchunks = (uint32_t)((A.n + 63) >> 6);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const uint32_t waves = gridDim.x * 4u;
    const float inf = __uint_as_float(0x7f800000u), qnan = __uint_as_float(0x7fc00000u);
    unsigned long long evals = 0;

    for (uint32_t chunk = wave; chunk < nchunks; chunk += waves) {
        const size_t idx = (size_t)chunk * 64 + (size_t)lane;
        const bool have = idx < (size_t)A.n;  // (the tail chunk is masked)
        V3 p = v3(0.0f, 0.0f, 0.0f);
        if (have) {
            const float *xp = A.X + idx * 3;
            p = v3(xp[0], xp[1], xp[2]);
        }
        const bool live = have && __builtin_fabsf(p.x) < inf && __builtin_fabsf(p.y) < inf && __builtin_fabsf(p.z) < inf;
        const uint64_t lm = __ballot(live);
        float best = inf;
        int besti = 0x7fffffff, bestpos = -1;

        // every lane's distance to triangle t of tris; a live lane keeps the minimum of (d2, index)
        auto eval = [&](int t) {
            const float4 q0 = tris[3 * (size_t)t], q1 = tris[3 * (size_t)t + 1], q2 = tris[3 * (size_t)t + 2];
            const int oi = __float_as_int(q0.w);
            int f;
            const V3 c = tri_closest(p, v3(q0.x, q0.y, q0.z), v3(q1.x, q1.y, q1.z), v3(q2.x, q2.y, q2.z), f);
            const V3 d = vsub(p, c);
            const float d2 = vdot(d, d);
            if (live && (d2 < best || (d2 == best && oi < besti))) {
                best = d2;
                besti = oi;
                bestpos = t;
            }
        };

        if (lm != 0) {
            const unsigned long long nlive = (unsigned long long)__popcll(lm);
            if (A.brute) {
                for (int t = 0; t < A.ntl; ++t) eval(t);
                evals += (unsigned long long)A.ntl * nlive;
            } else {
                int sp = 0, node = 0;
                for (int entered = 0; entered < A.nnodes; ++entered) {
                    const float4 n0 = nodes[2 * (size_t)node], n1 = nodes[2 * (size_t)node + 1];
                    const int w3 = __float_as_int(n0.w), w7 = __float_as_int(n1.w);
                    if (w7 <= 0) {
                        const int first = w3, count = -w7;
                        for (int t = first; t < first + count; ++t) eval(t);
                        evals += (unsigned long long)count * nlive;
                        node = -1;
                    } else {
                        const float bl = box_bound(p, nodes[2 * (size_t)w3], nodes[2 * (size_t)w3 + 1]);
                        const float br = box_bound(p, nodes[2 * (size_t)w7], nodes[2 * (size_t)w7 + 1]);
                        const bool want_l = __ballot(live && !(bl > best)) != 0;
                        const bool want_r = __ballot(live && !(br > best)) != 0;
                        const bool left_near = 2ull * (unsigned long long)__popcll(__ballot(live && bl <= br)) >= nlive;
                        const int near = left_near ? w3 : w7, far = left_near ? w7 : w3;
                        const bool want_near = left_near ? want_l : want_r, want_far = left_near ? want_r : want_l;
                        if (want_near) {
                            node = near;
                            if (want_far && sp < TRIMESH_STACK) stack[sp++] = far;
                        } else {
                            node = want_far ? far : -1;
                        }
                    }
                    if (node < 0) {
                        while (sp > 0) {
                            const int cand = __builtin_amdgcn_readfirstlane(stack[--sp]);
                            const float bc = box_bound(p, nodes[2 * (size_t)cand], nodes[2 * (size_t)cand + 1]);
                            if (__ballot(live && !(bc > best)) != 0) {
                                node = cand;
                                break;
                            }
                        }
                        if (node < 0) break;
                    }
                }
            }
        }

        if (have) {
            float sdf = qnan;
            V3 c = v3(qnan, qnan, qnan);
            int ti = -1, fe = -1;
            if (live && bestpos >= 0) {
                const float4 *q = tris + 3 * (size_t)bestpos;
                c = tri_closest(p, load_v3(q), load_v3(q + 1), load_v3(q + 2), fe);
                const V3 d = vsub(p, c);
                const float dist = __builtin_sqrtf(vdot(d, d));
                const float *nrm = table + ((size_t)besti * 7 + (size_t)fe) * 3;
                const float s = vdot(d, v3(nrm[0], nrm[1], nrm[2]));
                sdf = s < 0.0f ? -dist : dist;
                ti = besti;
            }
            if (A.sdf) A.sdf[idx] = sdf;
            if (A.closest) {
                float *o = A.closest + idx * 3;
                o[0] = c.x; o[1] = c.y; o[2] = c.z;
            }
            if (A.tri) A.tri[idx] = ti;
            if (A.feature) A.feature[idx] = fe;
        }
    }
    if (lane == 0 && evals != 0) atomicAdd(A.stats, evals);
}

}  // namespace

hipError_t launch_trimesh_distance(const TriMeshArgs &A, int grid, hipStream_t st) {
    hipLaunchKernelGGL(k_trimesh_distance, dim3(grid), dim3(256), 0, st, reinterpret_cast<const float4 *>(A.nodes),
                       reinterpret_cast<const float4 *>(A.tris), A.table, A);
    return hipGetLastError();
}

}  // namespace nr
