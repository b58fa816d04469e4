// nr_mesh_rays.hip -- rays against a triangle mesh (nr_mesh_trace_rays, nr_mesh_gbuffer,
// nr_mesh_render): the closest hit of each ray, or whether there is any, by a walk of the hierarchy
// nr_trimesh_create built (nr_trimesh_host.cpp).  The arithmetic contract -- Woop, Benthin and Wald's
// watertight shear form -- is in include/neural_render.h; tests/mesh_ray_ref.py restates it in numpy.
//
// k_mesh_rays has the shape of k_trimesh_distance.  A wave owns chunks of 64 rays (chunk w, w + waves,
// ...), one ray per lane -- 64 consecutive caller rays, or one 8 x 8 tile of the view, whose rays are
// generated here with nr_render's arithmetic -- and walks the tree once for all of them:
//   * the walk is wave-uniform: one node index, one stack of pending nodes in LDS, and a node's words
//     and a leaf's triangles are read at wave-uniform addresses (scalar loads);
//   * each lane tests a node's box, widened by its own pad, with its own slab interval; the wave
//     enters the node while any live lane wants it.  Of two wanted children the one more lanes reach
//     sooner is entered at once and the other is pushed; a popped node is tested again, since best has
//     shrunk meanwhile;
//   * the axes of the shear differ per lane: the components are selected with compares, never by
//     indexing, so nothing goes to scratch;
//   * a leaf's triangles are evaluated by every lane up to the edge test; the depth and its division
//     are formed only if some lane of the wave passed it.  The winner is the minimum of (t, original
//     triangle index), so the order of the walk, the leaf size and the hierarchy change no bit.
//     NR_TRIMESH_BRUTE is the same evaluation over all triangles with no walk;
//   * a lane without a ray (the tail, a ragged tile) or with a dead one is not live: it takes no part
//     in any vote and cannot lengthen the walk.  With NR_MESH_RAY_ANY a lane that has its hit leaves
//     the live mask, and the walk ends when the mask is empty.
// Every loop is bounded by a count the host fixed: nodes entered <= nnodes, pops <= the stack size, a
// leaf's triangles <= its count.  The winner's outputs are recomputed once per ray after the walk.
#include "nr_device.h"
#include "nr_internal.h"
#include "nr_kernels.h"

namespace nr {
namespace {

// component k (0, 1, 2) of (x, y, z) by two selects
__device__ __forceinline__ float sel3(float x, float y, float z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

// what a ray keeps for the triangle test: the origin in the order (kx, ky, kz) and the shear
struct Shear {
    int kx, ky, kz;
    float ox, oy, oz;
    float sx, sy, sz;
};

__device__ __forceinline__ Shear make_shear(F3 o, F3 d) {
    Shear s;
    int kz = 0;
    float dk = d.x;
    if (__builtin_fabsf(d.y) > __builtin_fabsf(dk)) { kz = 1; dk = d.y; }
    if (__builtin_fabsf(d.z) > __builtin_fabsf(dk)) { kz = 2; dk = d.z; }
    int kx = kz == 2 ? 0 : kz + 1;
    int ky = kx == 2 ? 0 : kx + 1;
    if (dk < 0.0f) { const int k = kx; kx = ky; ky = k; }
    s.kx = kx; s.ky = ky; s.kz = kz;
    s.ox = sel3(o.x, o.y, o.z, kx); s.oy = sel3(o.x, o.y, o.z, ky); s.oz = sel3(o.x, o.y, o.z, kz);
    s.sx = sel3(d.x, d.y, d.z, kx) / dk;
    s.sy = sel3(d.x, d.y, d.z, ky) / dk;
    s.sz = 1.0f / dk;
    return s;
}

// The edge functions of triangle (a, b, c) and the unscaled depths of its corners (step 2 of the
// header up to det).  A component of a - o does not depend on the order it is selected in.
struct Edges { float U, V, W, det, az, bz, cz; };
__device__ __forceinline__ Edges tri_edges(const Shear &s, float4 a, float4 b, float4 c) {
    Edges e;
    e.az = sel3(a.x, a.y, a.z, s.kz) - s.oz;
    e.bz = sel3(b.x, b.y, b.z, s.kz) - s.oz;
    e.cz = sel3(c.x, c.y, c.z, s.kz) - s.oz;
    const float ax = (sel3(a.x, a.y, a.z, s.kx) - s.ox) - s.sx * e.az, ay = (sel3(a.x, a.y, a.z, s.ky) - s.oy) - s.sy * e.az;
    const float bx = (sel3(b.x, b.y, b.z, s.kx) - s.ox) - s.sx * e.bz, by = (sel3(b.x, b.y, b.z, s.ky) - s.oy) - s.sy * e.bz;
    const float cx = (sel3(c.x, c.y, c.z, s.kx) - s.ox) - s.sx * e.cz, cy = (sel3(c.x, c.y, c.z, s.ky) - s.oy) - s.sy * e.cz;
    e.U = cx * by - cy * bx;
    e.V = ax * cy - ay * cx;
    e.W = bx * ay - by * ax;
    e.det = (e.U + e.V) + e.W;
    return e;
}
__device__ __forceinline__ bool edges_pass(const Edges &e) {
    const bool neg = e.U < 0.0f || e.V < 0.0f || e.W < 0.0f, pos = e.U > 0.0f || e.V > 0.0f || e.W > 0.0f;
    return !(neg && pos) && e.det != 0.0f;
}
__device__ __forceinline__ float edges_t(const Shear &s, const Edges &e) {
    const float az = s.sz * e.az, bz = s.sz * e.bz, cz = s.sz * e.cz;
    const float tn = (e.U * az + e.V * bz) + e.W * cz;
    return tn / e.det;
}

// Whether a ray wants a node: the slab interval [tn, tf] of the stored box widened by pad against
// [tmin, lim]; min and max ignore a NaN (0 * inf of a ray in a face's plane), and a comparison with
// a NaN keeps the node.
__device__ __forceinline__ bool slab_wants(F3 o, F3 inv, float pad, float4 lo, float4 hi, float tmin, float lim, float &tn) {
    const float x1 = ((lo.x - pad) - o.x) * inv.x, x2 = ((hi.x + pad) - o.x) * inv.x;
    const float y1 = ((lo.y - pad) - o.y) * inv.y, y2 = ((hi.y + pad) - o.y) * inv.y;
    const float z1 = ((lo.z - pad) - o.z) * inv.z, z2 = ((hi.z + pad) - o.z) * inv.z;
    tn = fmaxf(fmaxf(fminf(x1, x2), fminf(y1, y2)), fminf(z1, z2));
    const float tf = fminf(fminf(fmaxf(x1, x2), fmaxf(y1, y2)), fmaxf(z1, z2));
    return !(tn > tf) && !(tf < tmin) && !(tn > lim);
}

__device__ __forceinline__ bool finite3(F3 v) {
    const float inf = __uint_as_float(0x7f800000u);
    return __builtin_fabsf(v.x) < inf && __builtin_fabsf(v.y) < inf && __builtin_fabsf(v.z) < inf;
}

// normalise(v) of the header, or the face entry where the squared length is 0 or not finite
__device__ __forceinline__ F3 unit_or(F3 v, F3 face) {
    const float l2 = dot3(v, v);
    if (!(l2 > 0.0f) || !(l2 < __uint_as_float(0x7f800000u))) return face;
    return mul3s(v, 1.0f / sqrtf(l2));
}

__device__ __forceinline__ F3 load3(const float *p) { return mk3(p[0], p[1], p[2]); }
__device__ __forceinline__ void store3(float *p, F3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }

// The kernel's arguments that only a chunk's head (the view) or its tail (the outputs' pointers, the
// colouring) needs are read from the kernel-argument segment there, behind a barrier the compiler
// cannot move the loads across: hoisted out of the chunk loop they would be held in SGPRs through
// the walk, which has none to spare, and be spilled.  KARG_R / KARG_A: where R and A lie behind the
// three pointers of k_mesh_rays.
// *kernarg_late<MeshRayArgs>(KARG_R) and the parameter R are the same bytes, and so are A's: a
// parameter added to k_mesh_rays or moved in it has to move these offsets with it.
constexpr size_t KARG_R = 3 * sizeof(void *), KARG_A = KARG_R + sizeof(MeshRayArgs);
static_assert(KARG_R == sizeof(const float4 *) + sizeof(const float4 *) + sizeof(const float *),
              "k_mesh_rays: R follows the three pointers nodes, tris, table");
static_assert(alignof(MeshRayArgs) == 8 && KARG_R % alignof(MeshRayArgs) == 0, "k_mesh_rays: no padding before R");
static_assert(alignof(RenderArgs) == 8 && sizeof(MeshRayArgs) % alignof(RenderArgs) == 0, "k_mesh_rays: no padding before A");
template <class T>
__device__ __forceinline__ const T *kernarg_late(size_t off) {
    const __attribute__((address_space(4))) char *p = (const __attribute__((address_space(4))) char *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return (const T *)(p + off);
}

// PIX: the rays are the view's, one 8 x 8 tile per chunk; COLOR: the payload is the frame A.out
template <bool PIX, bool COLOR>
__global__ __launch_bounds__(256) void k_mesh_rays(const float4 *__restrict__ nodes, const float4 *__restrict__ tris,
                                                   const float *__restrict__ table, MeshRayArgs R, RenderArgs) {
    __shared__ int stacks[4][TRIMESH_STACK];
    int *stack = stacks[threadIdx.x >> 6];
    const int lane = lane_id();
    const uint32_t nchunks = PIX ? (uint32_t)R.tiles_x * (uint32_t)R.tiles_y : (uint32_t)((R.n + 63) >> 6);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const uint32_t waves = gridDim.x * 4u;
    const float inf = __uint_as_float(0x7f800000u);
    unsigned long long evals = 0, hits = 0;

    for (uint32_t chunk = wave; chunk < nchunks; chunk += waves) {
        size_t idx;
        bool have;
        F3 o, d;
        if constexpr (PIX) {
            const MeshRayArgs &Rv = *kernarg_late<MeshRayArgs>(KARG_R);
            const uint32_t ty = chunk / (uint32_t)R.tiles_x, tx = chunk - ty * (uint32_t)R.tiles_x;
            const int x = (int)(tx * 8u) + (lane & 7), y = (int)(ty * 8u) + (lane >> 3);
            have = x < Rv.W && y < Rv.H;  // (ragged tiles are masked)
            idx = (size_t)y * (size_t)Rv.W + (size_t)x;
            const float *V = Rv.inv_view;
            o = mk3(dot4(0.0f, 0.0f, 0.0f, 1.0f, V + 0), dot4(0.0f, 0.0f, 0.0f, 1.0f, V + 4), dot4(0.0f, 0.0f, 0.0f, 1.0f, V + 8));
            const float u = pixel_uv(x, Rv.W, Rv.rcp_w);
            const float v = pixel_uv(y, Rv.H, Rv.rcp_h);
            const F3 dn = normalize3(mk3(u, v, -2.0f));
            d = mk3(dot3(dn, mk3(V[0], V[1], V[2])), dot3(dn, mk3(V[4], V[5], V[6])), dot3(dn, mk3(V[8], V[9], V[10])));
        } else {
            idx = (size_t)chunk * 64 + (size_t)lane;
            have = idx < (size_t)R.n;  // (the tail chunk is masked)
            o = mk3(0.0f, 0.0f, 0.0f);
            d = o;
            if (have) {
                o = load3(R.origins + idx * 3);
                d = load3(R.dirs + idx * 3);
            }
        }
        const bool live = have && finite3(o) && finite3(d) && (d.x != 0.0f || d.y != 0.0f || d.z != 0.0f);
        const Shear sh = make_shear(o, d);
        const F3 inv = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
        const float pad = 3.814697265625e-06f * (fmaxf(fmaxf(__builtin_fabsf(o.x), __builtin_fabsf(o.y)), __builtin_fabsf(o.z)) + R.scale);
        bool alive = live;  // live, and with NR_MESH_RAY_ANY still without a hit
        float best = inf;
        int besti = 0x7fffffff, bestpos = -1;

        // every lane against triangle t of tris; a live lane keeps the minimum of (t, index)
        auto eval = [&](int t) {
            const float4 q0 = tris[3 * (size_t)t], q1 = tris[3 * (size_t)t + 1], q2 = tris[3 * (size_t)t + 2];
            const int oi = __float_as_int(q0.w);
            const Edges e = tri_edges(sh, q0, q1, q2);
            const bool pass = alive && edges_pass(e);
            evals += (unsigned long long)__popcll(__ballot(alive));
            if (__ballot(pass) != 0) {
                const float th = edges_t(sh, e);
                if (pass && R.tmin <= th && th <= R.tmax) {
                    if (R.any) {
                        alive = false;
                        bestpos = t;
                    } else if (th < best || (th == best && oi < besti)) {
                        best = th;
                        besti = oi;
                        bestpos = t;
                    }
                }
            }
        };

        if (__ballot(live) != 0) {
            if (R.brute) {
                _Pragma("nounroll") for (int t = 0; t < R.ntl; ++t) eval(t);
            } else {
                int sp = 0, node = 0;
                for (int entered = 0; entered < R.nnodes; ++entered) {
                    const float4 n0 = nodes[2 * (size_t)node], n1 = nodes[2 * (size_t)node + 1];
                    const int w3 = __float_as_int(n0.w), w7 = __float_as_int(n1.w);
                    if (w7 <= 0) {
                        const int first = w3, count = -w7;
                        _Pragma("nounroll") for (int t = first; t < first + count; ++t) eval(t);
                        node = -1;
                        if (__ballot(alive) == 0) break;
                    } else {
                        const float lim = fminf(best, R.tmax);
                        float tl, tr;
                        const bool wl = slab_wants(o, inv, pad, nodes[2 * (size_t)w3], nodes[2 * (size_t)w3 + 1], R.tmin, lim, tl);
                        const bool wr = slab_wants(o, inv, pad, nodes[2 * (size_t)w7], nodes[2 * (size_t)w7 + 1], R.tmin, lim, tr);
                        const bool want_l = __ballot(alive && wl) != 0;
                        const bool want_r = __ballot(alive && wr) != 0;
                        const bool left_near = 2 * __popcll(__ballot(alive && tl <= tr)) >= __popcll(__ballot(alive));
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
                            float tc;
                            const bool wc = slab_wants(o, inv, pad, nodes[2 * (size_t)cand], nodes[2 * (size_t)cand + 1], R.tmin,
                                                       fminf(best, R.tmax), tc);
                            if (__ballot(alive && wc) != 0) {
                                node = cand;
                                break;
                            }
                        }
                        if (node < 0) break;
                    }
                }
            }
        }

        const bool hit = live && bestpos >= 0;
        hits += (unsigned long long)__popcll(__ballot(hit));
        if (have) {
            const MeshRayArgs &Ro = *kernarg_late<MeshRayArgs>(KARG_R);
            float th = 0.0f;
            F3 bary = mk3(0.0f, 0.0f, 0.0f), pos = bary, nrm = bary;
            int ti = -1;
            if (hit && !R.any) {
                const float4 *q = tris + 3 * (size_t)bestpos;
                const Edges e = tri_edges(sh, q[0], q[1], q[2]);
                th = edges_t(sh, e);
                bary = mk3(e.U / e.det, e.V / e.det, e.W / e.det);
                pos = mk3(__builtin_fmaf(d.x, th, o.x), __builtin_fmaf(d.y, th, o.y), __builtin_fmaf(d.z, th, o.z));
                ti = besti;
                const float *nt = table + (size_t)besti * 21;
                const F3 face = load3(nt);
                nrm = face;
                if (Ro.smooth) {
                    const F3 na = unit_or(load3(nt + 12), face), nb = unit_or(load3(nt + 15), face), nc = unit_or(load3(nt + 18), face);
                    const F3 m = mk3(__builtin_fmaf(nc.x, bary.z, __builtin_fmaf(nb.x, bary.y, na.x * bary.x)),
                                     __builtin_fmaf(nc.y, bary.z, __builtin_fmaf(nb.y, bary.y, na.y * bary.x)),
                                     __builtin_fmaf(nc.z, bary.z, __builtin_fmaf(nb.z, bary.y, na.z * bary.x)));
                    nrm = unit_or(m, face);
                }
            }
            if constexpr (COLOR) {
                const RenderArgs &A = *kernarg_late<RenderArgs>(KARG_A);
                A.out[idx] = hit ? shade_color(A, A.normal, nrm, d) : 0u;
            } else {
                if (Ro.status) Ro.status[idx] = hit ? NR_RAY_HIT : NR_RAY_MISS;
                if (Ro.t) Ro.t[idx] = th;
                if (Ro.tri) Ro.tri[idx] = ti;
                if (Ro.bary) store3(Ro.bary + idx * 3, bary);
                if (Ro.position) store3(Ro.position + idx * 3, pos);
                if (Ro.normal) store3(Ro.normal + idx * 3, nrm);
            }
        }
    }
    if (lane == 0) {
        if (evals != 0) atomicAdd(R.stats, evals);
        if (hits != 0) atomicAdd(R.stats + 1, hits);
    }
}

}  // namespace

hipError_t launch_mesh_rays(const MeshRayArgs &R, const RenderArgs *color, int grid, hipStream_t st) {
    const float4 *nodes = reinterpret_cast<const float4 *>(R.nodes), *tris = reinterpret_cast<const float4 *>(R.tris);
    if (color) hipLaunchKernelGGL((k_mesh_rays<true, true>), dim3(grid), dim3(256), 0, st, nodes, tris, R.table, R, *color);
    else if (!R.origins) hipLaunchKernelGGL((k_mesh_rays<true, false>), dim3(grid), dim3(256), 0, st, nodes, tris, R.table, R, RenderArgs{});
    else hipLaunchKernelGGL((k_mesh_rays<false, false>), dim3(grid), dim3(256), 0, st, nodes, tris, R.table, R, RenderArgs{});
    return hipGetLastError();
}

}  // namespace nr
