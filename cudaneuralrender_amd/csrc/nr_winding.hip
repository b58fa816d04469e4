// nr_winding.hip -- the generalized winding number of a triangle mesh at points (nr_mesh_winding):
// the signed solid angles of all triangles seen from the point, over 4 pi, summed through the
// host-built hierarchy (nr_trimesh_host.cpp) with a node far from the point replaced by the order-1
// expansion of its moments.  The arithmetic contract is in include/neural_render.h;
// tests/winding_ref.py restates it in numpy.
//
// k_trimesh_winding.  A wave owns chunks of 64 consecutive points, one point per lane, and walks the
// tree once for all of them, as k_trimesh_distance does: one wave-uniform node index, one stack of
// pending nodes in LDS, nodes, moments and a leaf's triangles read at wave-uniform addresses (scalar
// loads).  Unlike a minimum, a sum depends on its order and on what it is made of, so:
//   * the order is fixed: the left child is entered, the right one pushed -- the preorder of the
//     tree, whatever the other lanes of the wave need;
//   * a lane's sum is a function of its own point: a lane for which a node is far adds the node's
//     expansion and is closed for the node's subtree -- the index range [node, end), nodes being in
//     preorder; `end` travels wave-uniformly beside the node (on the stack too), and the lane keeps
//     `resume`, the first node it is open for again;
//   * the wave enters a node's children, or evaluates a leaf's triangles, iff some live lane is open
//     for the node and not far from it, and only those lanes add.
// NR_TRIMESH_BRUTE is the same accumulator over every triangle in position order.  A lane without a
// point or with a non-finite one is not live and takes no part in any vote.  Every loop is bounded
// by a count the host fixed: nodes entered <= nnodes (one pop at most per node entered), the stack
// by TRIMESH_STACK entries, a leaf's triangles by its count.
//
// With A.sdf the kernel also rewrites the magnitudes k_trimesh_distance left there: -|sdf| where
// w >= 0.5f, |sdf| elsewhere, a NaN left as it is.
#include "nr_device.h"
#include "nr_internal.h"
#include "nr_kernels.h"

namespace nr {
namespace {

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 dsub(D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
// the contract's dot and len
__device__ __forceinline__ double ddot(D3 u, D3 v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }
__device__ __forceinline__ double dlen(D3 u) { return (double)__builtin_sqrtf((float)ddot(u, u)); }
__device__ __forceinline__ D3 promote(float4 q) { return D3{(double)q.x, (double)q.y, (double)q.z}; }

// the contract's h(num, den): atan2 from basic operations
__device__ __forceinline__ double half_angle(double num, double den) {
    const double an = __builtin_fabs(num), ad = __builtin_fabs(den);
    const bool swap = an > ad;
    const double t = (an < ad ? an : ad) / (an < ad ? ad : an);
    const bool big = t > 0.41421356237309503;
    const double u = big ? (t - 1.0) / (t + 1.0) : t;
    const double z = u * u;
    double p = -1.0 / 23.0;
    p = p * z + 1.0 / 21.0;
    p = p * z + -1.0 / 19.0;
    p = p * z + 1.0 / 17.0;
    p = p * z + -1.0 / 15.0;
    p = p * z + 1.0 / 13.0;
    p = p * z + -1.0 / 11.0;
    p = p * z + 1.0 / 9.0;
    p = p * z + -1.0 / 7.0;
    p = p * z + 1.0 / 5.0;
    p = p * z + -1.0 / 3.0;
    p = p * z + 1.0;
    double a = (big ? 0.7853981633974483 : 0.0) + u * p;
    if (swap) a = 1.5707963267948966 - a;
    if (den < 0.0) a = 3.141592653589793 - a;
    if (num < 0.0) a = -a;
    const bool finite = __builtin_fabs(t) < __builtin_inf();  // (false for a NaN)
    return num == 0.0 || !finite ? 0.0 : a;
}

// the signed solid angle of triangle (A, B, C) seen from p
__device__ __forceinline__ double solid_angle(D3 p, D3 A, D3 B, D3 C) {
    const D3 a = dsub(A, p), b = dsub(B, p), c = dsub(C, p);
    const double det = (a.x * (b.y * c.z - b.z * c.y) + a.y * (b.z * c.x - b.x * c.z)) + a.z * (b.x * c.y - b.y * c.x);
    const double la = dlen(a), lb = dlen(b), lc = dlen(c);
    const double den = (((la * lb) * lc + ddot(a, b) * lc) + ddot(b, c) * la) + ddot(c, a) * lb;
    return 2.0 * half_angle(det, den);
}

__global__ __launch_bounds__(256) void k_trimesh_winding(const float4 *__restrict__ nodes, const float4 *__restrict__ tris,
                                                         const float4 *__restrict__ moments, TriWindArgs A) {
    __shared__ int stacks[4][TRIMESH_STACK][2];
    int(*stack)[2] = stacks[threadIdx.x >> 6];
    const int lane = lane_id();
    const uint32_t nchunks = (uint32_t)((A.n + 63) >> 6);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const uint32_t waves = gridDim.x * 4u;
    const float inf = __uint_as_float(0x7f800000u), qnan = __uint_as_float(0x7fc00000u);
    const double bb = (double)A.beta * (double)A.beta;
    unsigned long long evals = 0;

    for (uint32_t chunk = wave; chunk < nchunks; chunk += waves) {
        const size_t idx = (size_t)chunk * 64 + (size_t)lane;
        const bool have = idx < (size_t)A.n;  // (the tail chunk is masked)
        float px = 0.0f, py = 0.0f, pz = 0.0f;
        if (have) {
            const float *xp = A.X + idx * 3;
            px = xp[0]; py = xp[1]; pz = xp[2];
        }
        const bool live = have && __builtin_fabsf(px) < inf && __builtin_fabsf(py) < inf && __builtin_fabsf(pz) < inf && A.ntl > 0;
        const uint64_t lm = __ballot(live);
        const D3 p{(double)px, (double)py, (double)pz};
        double W = 0.0;

        auto omega = [&](int t) {
            return solid_angle(p, promote(tris[3 * (size_t)t]), promote(tris[3 * (size_t)t + 1]), promote(tris[3 * (size_t)t + 2]));
        };

        if (lm != 0) {
            if (A.brute) {
                for (int t = 0; t < A.ntl; ++t) {
                    const double o = omega(t);
                    if (live) W += o;
                }
                evals += (unsigned long long)A.ntl * (unsigned long long)__popcll(lm);
            } else {
                int sp = 0, node = 0, end = A.nnodes;
                int resume = 0;  // the lane is open for node i iff i >= resume
                for (int entered = 0; entered < A.nnodes; ++entered) {
                    const float4 n0 = nodes[2 * (size_t)node], n1 = nodes[2 * (size_t)node + 1];
                    const int w3 = __float_as_int(n0.w), w7 = __float_as_int(n1.w);
                    const float4 m0 = moments[4 * (size_t)node];
                    const bool open = live && node >= resume;
                    const D3 r = dsub(promote(m0), p);
                    const double d2 = ddot(r, r);
                    const bool isfar = d2 > bb * (double)m0.w;
                    const uint64_t take = __ballot(open && isfar);
                    if (take != 0) {
                        const float4 m1 = moments[4 * (size_t)node + 1], m2 = moments[4 * (size_t)node + 2], m3 = moments[4 * (size_t)node + 3];
                        const double sxx = (double)m2.x, syy = (double)m2.y, szz = (double)m2.z;
                        const double sxy = (double)m2.w, sxz = (double)m3.x, syz = (double)m3.y;
                        const double d = (double)__builtin_sqrtf((float)d2);
                        const double d3 = d2 * d;
                        const D3 s{(sxx * r.x + sxy * r.y) + sxz * r.z, (sxy * r.x + syy * r.y) + syz * r.z, (sxz * r.x + syz * r.y) + szz * r.z};
                        const double q = ddot(r, s);
                        const double tr = (sxx + syy) + szz;
                        const double E = ddot(promote(m1), r) / d3 + (tr / d3 - (3.0 * q) / (d3 * d2));
                        if (open && isfar) {
                            W += E;
                            resume = end;
                        }
                        evals += (unsigned long long)__popcll(take);
                    }
                    const uint64_t need = __ballot(open && !isfar);
                    int next = -1, next_end = 0;
                    if (need != 0) {
                        if (w7 <= 0) {
                            const int first = w3, count = -w7;
                            for (int t = first; t < first + count; ++t) {
                                const double o = omega(t);
                                if (open && !isfar) W += o;
                            }
                            evals += (unsigned long long)count * (unsigned long long)__popcll(need);
                        } else {
                            next = w3;
                            next_end = w7;
                            if (sp < TRIMESH_STACK) {
                                stack[sp][0] = w7;
                                stack[sp][1] = end;
                                ++sp;
                            }
                        }
                    }
                    if (next < 0) {
                        if (sp == 0) break;
                        --sp;
                        next = __builtin_amdgcn_readfirstlane(stack[sp][0]);
                        next_end = __builtin_amdgcn_readfirstlane(stack[sp][1]);
                    }
                    node = next;
                    end = next_end;
                }
            }
        }

        if (have) {
            const float w = live ? (float)(W * 0.07957747154594767) : qnan;
            if (A.winding) A.winding[idx] = w;
            if (A.sdf) {
                const float m = A.sdf[idx];
                if (m == m) A.sdf[idx] = w >= 0.5f ? -__builtin_fabsf(m) : __builtin_fabsf(m);
            }
        }
    }
    if (lane == 0 && evals != 0) atomicAdd(A.stats, evals);
}

}  // namespace

hipError_t launch_trimesh_winding(const TriWindArgs &A, int grid, hipStream_t st) {
    hipLaunchKernelGGL(k_trimesh_winding, dim3(grid), dim3(256), 0, st, reinterpret_cast<const float4 *>(A.nodes),
                       reinterpret_cast<const float4 *>(A.tris), reinterpret_cast<const float4 *>(A.moments), A);
    return hipGetLastError();
}

}  // namespace nr
