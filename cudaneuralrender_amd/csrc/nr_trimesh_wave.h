// nr_trimesh_wave.h -- the per-wave bodies of the triangle-mesh point queries, one copy for every
// kernel that runs them: the shared walk with tri_closest, the (d2, index) minimum and the
// pseudonormal sign (trimesh_distance_wave: k_trimesh_distance, k_trimesh_grid_distance), and the
// winding sum with its expansion and the in-place sign (trimesh_winding_wave: k_trimesh_winding,
// k_trimesh_grid_winding).  The arithmetic contract is in include/neural_render.h;
// tests/trimesh_ref.py and tests/winding_ref.py restate it in numpy.
//
// A body is a template over a point source: which 64 points a wave takes as chunk c, and where a
// point's results go.  A source has
//     uint32_t nchunks() const
//     bool point(uint32_t chunk, int lane, size_t &idx, float &x, float &y, float &z) const
// point() returns whether the lane has a point; idx is the point's slot in every output array.  A
// lane without a point is not live: it takes part in no vote and writes nothing.  A point's result
// is a function of the point alone (the minimum of (d2, original index); the fixed preorder of the
// sum), so the sources differ in speed only, never in a bit:
//     PointArraySrc     64 consecutive points of a caller's array (nr_trimesh_distance, nr_mesh_winding)
//     LatticeBlockSrc   one 4 x 4 x 4 block of a lattice (nr_mesh_sample_grid, nr_mesh_remesh)
//     CornerBlockSrc    one 4 x 4 x 4 block of the brick-corner lattice (nr_mesh_remesh_sparse)
//     BrickStoreSrc     64 consecutive store points of an active brick (nr_mesh_remesh_sparse)
// The lattice sources form a coordinate from the point's global lattice index,
// origin[a] + (float)idx_a * step[a], never from a block's origin plus an offset.
#pragma once
#include "nr_device.h"
#include "nr_internal.h"
#include "nr_kernels.h"
#include "nr_lattice.h"

namespace nr {

// ---------------------------------------------------------------- point sources
struct PointArraySrc {
    const float *X;  // [n][3]
    long n;
    __device__ __forceinline__ uint32_t nchunks() const { return (uint32_t)((n + 63) >> 6); }
    __device__ __forceinline__ bool point(uint32_t chunk, int lane, size_t &idx, float &x, float &y, float &z) const {
        idx = (size_t)chunk * 64 + (size_t)lane;
        const bool have = idx < (size_t)n;  // (the tail chunk is masked)
        if (have) {
            const float *xp = X + idx * 3;
            x = xp[0]; y = xp[1]; z = xp[2];
        }
        return have;
    }
};

// lane l of block (bi, bj, bk) is lattice point (4 bi + (l & 3), 4 bj + ((l >> 2) & 3), 4 bk + (l >> 4)); the
// point's index is 64-bit.  The blocks are dealt tile by tile -- a tile is 2^tx x 2^ty x 2^tz blocks (8 a
// side where the lattice has as many), tiles and the blocks of a tile both x-fastest -- so that the waves
// running at one time work on a compact part of the lattice and share the nodes and triangles they read
// (measured: profiles/trimesh_grid_bench.txt).  A chunk whose block lies past the lattice (a ragged tile)
// has no point in any lane.  The order changes no bit: a point's value is a function of the point.
struct LatticeBlockSrc {
    LatticeArgs L;
    uint32_t tbx, tbxy, chunks;  // tiles along x, in an xy slab; tiles times blocks per tile
    uint32_t shifts;             // tx | ty << 8 | tz << 16
    __device__ __forceinline__ uint32_t nchunks() const { return chunks; }
    __device__ __forceinline__ bool point(uint32_t chunk, int lane, size_t &idx, float &x, float &y, float &z) const {
        const uint32_t tx = shifts & 255u, ty = (shifts >> 8) & 255u, txy = tx + ty, txyz = txy + (shifts >> 16);
        const uint32_t tile = chunk >> txyz, w = chunk & ((1u << txyz) - 1u);
        const uint32_t tk = tile / tbxy, r = tile - tk * tbxy;  // (once per 64 points: plain division)
        const uint32_t tj = r / tbx, ti = r - tj * tbx;
        const uint32_t bi = (ti << tx) + (w & ((1u << tx) - 1u)), bj = (tj << ty) + ((w >> tx) & ((1u << ty) - 1u)),
                       bk = (tk << (txyz - txy)) + (w >> txy);
        const int i = (int)(4u * bi) + (lane & 3), j = (int)(4u * bj) + ((lane >> 2) & 3), k = (int)(4u * bk) + (lane >> 4);
        const bool have = i < L.nx && j < L.ny && k < L.nz;
        idx = ((size_t)k * (size_t)L.ny + (size_t)j) * (size_t)L.nx + (size_t)i;
        if (have) {
            x = L.origin[0] + (float)i * L.step[0];
            y = L.origin[1] + (float)j * L.step[1];
            z = L.origin[2] + (float)k * L.step[2];
        }
        return have;
    }
};
inline LatticeBlockSrc make_lattice_blocks(const LatticeArgs &L) {
    LatticeBlockSrc S{};
    S.L = L;
    const uint32_t b[3] = {((uint32_t)L.nx + 3u) / 4u, ((uint32_t)L.ny + 3u) / 4u, ((uint32_t)L.nz + 3u) / 4u};  // <= 2^28 each
    uint32_t t[3], tb[3];
    for (int pass = 0; pass < 2; ++pass) {
        for (int a = 0; a < 3; ++a) {
            t[a] = 0;
            while (pass == 0 && t[a] < 3 && (1u << t[a]) < b[a]) ++t[a];
            tb[a] = (b[a] + (1u << t[a]) - 1u) >> t[a];
        }
        // (ragged tiles add chunks without points; should they ever push the count past 32 bits: tiles of one block)
        if ((((unsigned long long)tb[0] * tb[1] * tb[2]) << (t[0] + t[1] + t[2])) < (1ull << 32)) break;
    }
    S.tbx = tb[0]; S.tbxy = tb[0] * tb[1];
    S.chunks = (tb[0] * tb[1] * tb[2]) << (t[0] + t[1] + t[2]);
    S.shifts = t[0] | t[1] << 8 | t[2] << 16;
    return S;
}

// the same blocks over the brick-corner lattice (cx by cy by cz corners): corner (ci, cj, ck) is the
// lattice point min(B c, dim - 1) per axis and slot (ck cy + cj) cx + ci of SparseArgs::coarse
struct CornerBlockSrc {
    SparseLattice L;
    uint32_t cx, cy, cz;
    uint32_t bx, bxy, nblocks;
    __device__ __forceinline__ uint32_t nchunks() const { return nblocks; }
    __device__ __forceinline__ bool point(uint32_t chunk, int lane, size_t &idx, float &x, float &y, float &z) const {
        const uint32_t bk = chunk / bxy, r = chunk - bk * bxy;  // (once per 64 points: plain division)
        const uint32_t bj = r / bx, bi = r - bj * bx;
        const uint32_t ci = 4u * bi + (uint32_t)(lane & 3), cj = 4u * bj + (uint32_t)((lane >> 2) & 3), ck = 4u * bk + (uint32_t)(lane >> 4);
        const bool have = ci < cx && cj < cy && ck < cz;
        idx = ((size_t)ck * cy + cj) * cx + ci;
        if (have) {
            const F3 p = lattice_point(L, min(L.B * (int)ci, L.nx - 1), min(L.B * (int)cj, L.ny - 1), min(L.B * (int)ck, L.nz - 1));
            x = p.x; y = p.y; z = p.z;
        }
        return have;
    }
};
inline CornerBlockSrc make_corner_blocks(const SparseLattice &L) {
    CornerBlockSrc S{};
    S.L = L;
    S.cx = (uint32_t)L.nbx + 1u; S.cy = (uint32_t)L.nby + 1u; S.cz = (uint32_t)L.nbz + 1u;
    const uint32_t bx = (S.cx + 3u) / 4u, by = (S.cy + 3u) / 4u, bz = (S.cz + 3u) / 4u;
    S.bx = bx; S.bxy = bx * by; S.nblocks = bx * by * bz;  // < 2^32 as ncoarse is
    return S;
}

// chunk c = the 64 store points from 64 c: all of brick slot c / (stride / 64), as k_sp_sample deals
// them; a store point past the brick's S^3 or past a ragged brick's extent is no point
struct BrickStoreSrc {
    SparseLattice L;
    const uint32_t *list;  // [nactive]
    uint32_t nactive;
    __device__ __forceinline__ uint32_t nchunks() const { return nactive * (L.stride >> 6); }  // < 2^31 (the host checks)
    __device__ __forceinline__ bool point(uint32_t chunk, int lane, size_t &idx, float &x, float &y, float &z) const {
        const uint32_t wpb = L.stride >> 6;
        const uint32_t a = udiv_r(chunk, wpb, L.inv_wpb);
        const uint32_t r = ((chunk - a * wpb) << 6) + (uint32_t)lane;
        idx = (size_t)a * L.stride + r;
        if (r >= L.P) return false;
        const Brick K = brick_of(L, list[a]);
        int li, lj, lk;
        local_ijk(L, r, li, lj, lk);
        if (!(li <= K.e[0] && lj <= K.e[1] && lk <= K.e[2])) return false;
        const F3 p = lattice_point(L, L.B * K.b[0] + li, L.B * K.b[1] + lj, L.B * K.b[2] + lk);
        x = p.x; y = p.y; z = p.z;
        return true;
    }
};

// ---------------------------------------------------------------- distance
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

// One wave of a 4-wave workgroup: chunks wave, wave + waves, ... of `src`; `stack` is the wave's
// TRIMESH_STACK words of LDS.  A.X and A.n are the source's business, not read here.
template <class Src>
__device__ __forceinline__ void trimesh_distance_wave(const float4 *__restrict__ nodes, const float4 *__restrict__ tris,
                                                      const float *__restrict__ table, const TriMeshArgs &A, const Src &src,
                                                      int *stack) {
    const int lane = lane_id();
    const uint32_t nchunks = src.nchunks();
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const uint32_t waves = gridDim.x * 4u;
    const float inf = __uint_as_float(0x7f800000u), qnan = __uint_as_float(0x7fc00000u);
    unsigned long long evals = 0;

    for (uint32_t chunk = wave; chunk < nchunks; chunk += waves) {
        size_t idx;
        V3 p = v3(0.0f, 0.0f, 0.0f);
        const bool have = src.point(chunk, lane, idx, p.x, p.y, p.z);
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

// ---------------------------------------------------------------- winding
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

// One wave of a 4-wave workgroup, as trimesh_distance_wave; `stack` is the wave's TRIMESH_STACK
// pairs of LDS words.  With A.sdf the magnitudes found there are signed in place.
template <class Src>
__device__ __forceinline__ void trimesh_winding_wave(const float4 *__restrict__ nodes, const float4 *__restrict__ tris,
                                                     const float4 *__restrict__ moments, const TriWindArgs &A, const Src &src,
                                                     int (*stack)[2]) {
    const int lane = lane_id();
    const uint32_t nchunks = src.nchunks();
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const uint32_t waves = gridDim.x * 4u;
    const float inf = __uint_as_float(0x7f800000u), qnan = __uint_as_float(0x7fc00000u);
    const double bb = (double)A.beta * (double)A.beta;
    unsigned long long evals = 0;

    for (uint32_t chunk = wave; chunk < nchunks; chunk += waves) {
        size_t idx;
        float px = 0.0f, py = 0.0f, pz = 0.0f;
        const bool have = src.point(chunk, lane, idx, px, py, pz);
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

}  // namespace nr
