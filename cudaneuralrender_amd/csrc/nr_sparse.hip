// nr_sparse.hip -- brick-culled isosurface extraction (nr_extract_mesh_sparse): nr_mesh_grid's mesh
// of a lattice too large to sample densely, restricted to the bricks of B^3 cells that can hold the
// surface (the contract: include/neural_render.h; the rule, the ownership and what the band proves:
// DESIGN.md).
//
//   k_sp_coarse          the scene's distance at the brick corners (the lattice points min(B b, dim - 1))
//   k_sp_classify_count  a brick is active iff a corner is NaN, the corners differ in insideness or
//   k_mesh_scan            the nearest corner is within `band` of iso; count, scan and
//   k_sp_classify_emit     emit compact the active bricks in ascending index and write the brick -> slot map
//   k_sp_sample          the hot path: the point sets of the active bricks, 64 store points a wave
//                        and pass, into the compact store (SparseLattice, nr_internal.h)
//   k_sp_mesh_count      nr_mesh.hip's three passes over 256-point blocks of the store: a store point
//   k_mesh_scan            contributes the triangles of its cell (every cell lies in one brick) and
//   k_sp_mesh_emit         the vertices of the edges its brick owns
//
// The samplers are k_grid's loop (persistent waves, the fp32 pack staged once per workgroup,
// mlp16_fp32 with a tile mask, scene_sdf) with the coordinate of a point computed from its global
// lattice index, so a value has nr_sample_grid's bits whichever brick evaluates it.  An edge on a
// face, edge or corner shared by bricks is owned by the lowest-indexed active brick whose point set
// holds both its ends (at most 8 candidates in the map; the brick that uses it is one).  No atomic
// decides an order: the output is a pure function of the inputs.
#include "nr_internal.h"
#include "nr_lattice.h"
#include "nr_mesh_rule.h"
#include "nr_mlp16.h"

namespace nr {

// waves per SIMD the samplers' registers are allocated for (as NR_GRID_WPS)
#ifndef NR_SPARSE_WPS
#define NR_SPARSE_WPS 4
#endif

static __constant__ MeshRule c_sp_rule = make_mesh_rule();

// ---------------------------------------------------------------- coarse sampler
__global__ __launch_bounds__(256, NR_SPARSE_WPS) void k_sp_coarse(SparseArgs A, MlpArgs M) {
    Smem16 S = stage16<NR_PRECISION_FP32, true>(M);
    const SparseLattice &L = A.L;
    const int lane = lane_id();
    const float fr = (float)A.frame;
    const double zoff = sphere_zoff(A.frame);
    const uint32_t n = L.ncoarse;
    const uint32_t nchunks = (n + 63u) >> 6;
    const uint32_t cx = (uint32_t)L.nbx + 1u, cxy = cx * ((uint32_t)L.nby + 1u);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const uint32_t waves = (uint32_t)__builtin_amdgcn_readfirstlane((int)(gridDim.x * 4u));
    for (uint32_t c = wave; c < nchunks; c += waves) {
        const uint32_t base = c << 6, idx = base + (uint32_t)lane;
        const bool live = idx < n;
        F3 p = mk3(0.0f, 0.0f, 0.0f);
        if (live) p = corner_point(L, idx, cx, cxy);
        const uint32_t rem = n - base;
        const uint32_t tmask = rem >= 64u ? 0xfu : (1u << ((rem + 15u) >> 4)) - 1u;
        float sdf = mlp16_fp32(M, S.s32, fr, p.x, p.y, p.z, tmask);
        if (!live) sdf = 0.0f;  // (a tile the MLP skipped holds no value)
        const float v = scene_sdf(p, sdf, A.scene, zoff);
        if (live) A.coarse[idx] = v;
    }
}

// ---------------------------------------------------------------- classify: count, (scan,) emit
// One thread per brick, 256 per block.  The block's exclusive scan of (active bricks, their point-set
// sizes) runs on one packed word: at most 256 bricks (bits 0-8) of at most 17^3 points (bits 9-31).
__global__ __launch_bounds__(256) void k_sp_classify_count(SparseArgs A) {
    __shared__ uint32_t wtot[4];
    const SparseLattice &L = A.L;
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    const int lane = lane_id(), wid = threadIdx.x >> 6;
    const bool live = b < L.nbricks;
    bool active = false;
    uint32_t packed = 0;
    if (live) {
        const Brick K = brick_of(L, b);
        const uint32_t cx = (uint32_t)L.nbx + 1u, cxy = cx * ((uint32_t)L.nby + 1u);
        const uint32_t base = (uint32_t)K.b[2] * cxy + (uint32_t)K.b[1] * cx + (uint32_t)K.b[0];
        uint32_t inside = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float s = A.coarse[base + (uint32_t)(c & 1) + ((c & 2) ? cx : 0u) + ((c & 4) ? cxy : 0u)];
            const float d = fabsf(s - A.iso);
            active |= s != s || d <= A.band;
            inside |= (uint32_t)(s < A.iso) << c;
        }
        active |= inside != 0u && inside != 0xffu;
        if (active) packed = 1u | ((uint32_t)((K.e[0] + 1) * (K.e[1] + 1) * (K.e[2] + 1)) << 9);
    }
    uint32_t incl = packed;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    if (lane == 63) wtot[wid] = incl;
    __syncthreads();
    uint32_t before = 0;
    for (int w = 0; w < wid; ++w) before += wtot[w];
    const uint32_t excl = before + incl - packed;
    if (live) A.map[b] = active ? (int32_t)(excl & 0x1ffu) : -1;
    if (threadIdx.x == 255) {
        const uint32_t tot = before + incl;
        A.bcnt[blockIdx.x] = tot & 0x1ffu;
        A.bcnt[A.nblk_b + blockIdx.x] = tot >> 9;
    }
}

__global__ __launch_bounds__(256) void k_sp_classify_emit(SparseArgs A) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= A.L.nbricks) return;
    const int32_t local = A.map[b];
    if (local < 0) return;
    const uint32_t slot = (uint32_t)A.boff[blockIdx.x] + (uint32_t)local;
    A.map[b] = (int32_t)slot;
    A.list[slot] = b;
}

// ---------------------------------------------------------------- brick sampler
// Chunk c = the 64 store points from 64 c: all of brick slot c / (stride / 64).  Store points past
// the brick's S^3, and those past a ragged brick's extent, evaluate the finite point (0, 0, 0) and
// skip the store; every chunk starts below S^3, so its first tile always holds a point.
__global__ __launch_bounds__(256, NR_SPARSE_WPS) void k_sp_sample(SparseArgs A, MlpArgs M) {
    Smem16 S = stage16<NR_PRECISION_FP32, true>(M);
    const SparseLattice &L = A.L;
    const int lane = lane_id();
    const float fr = (float)A.frame;
    const double zoff = sphere_zoff(A.frame);
    const uint32_t wpb = L.stride >> 6;
    const uint32_t nchunks = A.nactive * wpb;  // < 2^31 (the host checks)
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const uint32_t waves = (uint32_t)__builtin_amdgcn_readfirstlane((int)(gridDim.x * 4u));
    for (uint32_t c = wave; c < nchunks; c += waves) {
        const uint32_t a = udiv_r(c, wpb, L.inv_wpb);
        const uint32_t rbase = (c - a * wpb) << 6, r = rbase + (uint32_t)lane;
        const Brick K = brick_of(L, A.list[a]);
        bool live = r < L.P;
        F3 p = mk3(0.0f, 0.0f, 0.0f);
        if (live) {
            int li, lj, lk;
            local_ijk(L, r, li, lj, lk);
            live = li <= K.e[0] && lj <= K.e[1] && lk <= K.e[2];
            if (live) p = lattice_point(L, L.B * K.b[0] + li, L.B * K.b[1] + lj, L.B * K.b[2] + lk);
        }
        const uint32_t rem = L.P - rbase;
        const uint32_t tmask = rem >= 64u ? 0xfu : (1u << ((rem + 15u) >> 4)) - 1u;
        float sdf = mlp16_fp32(M, S.s32, fr, p.x, p.y, p.z, tmask);
        if (r >= L.P) sdf = 0.0f;  // (a tile the MLP skipped holds no value)
        const float v = scene_sdf(p, sdf, A.scene, zoff);
        if (live) A.store[(size_t)a * L.stride + r] = v;
    }
}

// ---------------------------------------------------------------- mesh passes over the store
struct StorePoint {
    uint32_t a, r;  // brick slot, local index
    Brick K;
    int l[3];
    bool live;      // a point of the brick's point set
};

__device__ __forceinline__ StorePoint store_point(const SparseArgs &A, size_t p) {
    const SparseLattice &L = A.L;
    StorePoint Q;
    Q.a = udiv_r((uint32_t)(p >> 6), L.stride >> 6, L.inv_wpb);  // p < 2^37 (the host checks)
    Q.r = (uint32_t)(p - (size_t)Q.a * L.stride);
    Q.live = Q.a < A.nactive && Q.r < L.P;
    if (!Q.live) return Q;
    Q.K = brick_of(L, A.list[Q.a]);
    local_ijk(L, Q.r, Q.l[0], Q.l[1], Q.l[2]);
    Q.live = Q.l[0] <= Q.K.e[0] && Q.l[1] <= Q.K.e[1] && Q.l[2] <= Q.K.e[2];
    return Q;
}

__device__ __forceinline__ uint32_t local_index(const SparseLattice &L, int li, int lj, int lk) {
    return (uint32_t)((lk * L.S + lj) * L.S + li);
}

// mesh_point on the brick's point set: a corner is valid iff it lies in it
__device__ __forceinline__ MeshPoint store_mesh_point(const SparseArgs &A, const StorePoint &Q) {
    const SparseLattice &L = A.L;
    MeshPoint P;
    const bool vx = Q.l[0] < Q.K.e[0], vy = Q.l[1] < Q.K.e[1], vz = Q.l[2] < Q.K.e[2];
    const float *s0 = A.store + (size_t)Q.a * L.stride + Q.r;
    P.valid = 0;
    P.inside = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const bool ok = (!(c & 1) || vx) && (!(c & 2) || vy) && (!(c & 4) || vz);
        const float s = ok ? s0[mesh_corner_offset(c, (uint32_t)L.S, (uint32_t)(L.S * L.S))] : 0.0f;
        P.s[c] = s;
        P.valid |= (uint32_t)ok << c;
        P.inside |= (uint32_t)(ok && s < A.iso) << c;
    }
    mesh_point_masks(c_sp_rule, P);
    return P;
}

// The owner of the edge from local point l of brick K (slot a) along the corner bits e -- both ends
// in K's point set: the lowest-indexed active brick whose point set holds both.  Along an axis the
// edge does not run, a point on a face between two bricks belongs to both; the candidates are the
// subsets of those axes, and stepping down z, then y, then x gives the lower index.  Returns the
// owner's slot and the point's local coordinates there.
struct EdgeOwner {
    uint32_t a;
    int l[3];
};

__device__ __forceinline__ EdgeOwner edge_owner(const SparseArgs &A, const Brick &K, uint32_t a, const int l[3], int e) {
    const SparseLattice &L = A.L;
    const int nb[3] = {L.nbx, L.nby, L.nbz};
    EdgeOwner O;
    O.a = a;
    int ub[3];  // the upper brick of each axis, the point's coordinate in it
    int low = 0, self = 0;  // axes with a lower brick too; those where K is the lower one
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        ub[ax] = K.b[ax];
        O.l[ax] = l[ax];
        if ((e >> ax) & 1) continue;
        if (l[ax] == K.e[ax] && K.b[ax] + 1 < nb[ax]) {
            ub[ax] = K.b[ax] + 1;
            self |= 1 << ax;
        } else if (!(l[ax] == 0 && K.b[ax] > 0)) {
            continue;
        }
        low |= 1 << ax;
    }
    if (!low) return O;  // inside K, or on the lattice's face
    for (int n = 7; n > self; --n) {
        if ((n & low) != n) continue;
        const int32_t s = A.map[brick_index(L, ub[0] - (n & 1), ub[1] - ((n >> 1) & 1), ub[2] - (n >> 2))];
        if (s < 0) continue;
        O.a = (uint32_t)s;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) O.l[ax] = ((n >> ax) & 1) ? L.B : ((self >> ax) & 1) ? 0 : l[ax];
        return O;
    }
    return O;  // no active candidate below K
}

// bit slot: the vertex of the crossing edge on `slot` is K's to write
__device__ __forceinline__ uint32_t owned_mask(const SparseArgs &A, const StorePoint &Q, uint32_t vmask) {
    uint32_t m = 0;
#pragma unroll
    for (int slot = 0; slot < 7; ++slot)
        if ((vmask >> slot) & 1u) m |= (uint32_t)(edge_owner(A, Q.K, Q.a, Q.l, MESH_SLOT_BITS[slot]).a == Q.a) << slot;
    return m;
}

// One thread per store point, 256 per block; the packed block scan of k_mesh_count.
__global__ __launch_bounds__(256) void k_sp_mesh_count(SparseArgs A) {
    __shared__ uint32_t wtot[4];
    const size_t p = (size_t)blockIdx.x * 256u + threadIdx.x;
    const int lane = lane_id(), wid = threadIdx.x >> 6;
    const StorePoint Q = store_point(A, p);
    uint32_t vmask = 0, packed = 0;
    if (Q.live) {
        const MeshPoint P = store_mesh_point(A, Q);
        vmask = owned_mask(A, Q, P.vmask);
        packed = (uint32_t)__popc(vmask) | (P.ntri << 16);
    }
    uint32_t incl = packed;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    if (lane == 63) wtot[wid] = incl;
    __syncthreads();
    uint32_t before = 0;
    for (int w = 0; w < wid; ++w) before += wtot[w];
    const uint32_t excl = before + incl - packed;
    if (Q.live) A.word[p] = vmask | ((excl & 0xffffu) << 7) | ((excl >> 16) << 18);
    if (threadIdx.x == 255) {
        const uint32_t tot = before + incl;
        A.cnt[blockIdx.x] = tot & 0xffffu;
        A.cnt[A.nblk_m + blockIdx.x] = tot >> 16;
    }
}

__global__ __launch_bounds__(256) void k_sp_mesh_emit(SparseArgs A) {
    const SparseLattice &L = A.L;
    const size_t p = (size_t)blockIdx.x * 256u + threadIdx.x;
    const StorePoint Q = store_point(A, p);
    if (!Q.live) return;
    const MeshPoint P = store_mesh_point(A, Q);
    if (!P.vmask && !P.ntri) return;
    const uint32_t w = A.word[p];
    const unsigned long long *offv = A.off, *offt = A.off + A.nblk_m;
    const uint32_t vmask = w & 0x7fu;
    if (vmask) {
        unsigned long long v0 = offv[blockIdx.x] + ((w >> 7) & 0x7ffu);
        const int idx[3] = {L.B * Q.K.b[0] + Q.l[0], L.B * Q.K.b[1] + Q.l[1], L.B * Q.K.b[2] + Q.l[2]};
        const long long index = ((long long)idx[2] * L.ny + idx[1]) * L.nx + idx[0];
        const float sa = P.s[0];
#pragma unroll
        for (int slot = 0; slot < 7; ++slot) {
            if (!((vmask >> slot) & 1u)) continue;
            const int b = MESH_SLOT_BITS[slot];
            const float t = (A.iso - sa) / (P.s[b] - sa);
            float *o = A.vertices + v0 * 3;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const float pa = L.origin[ax] + (float)idx[ax] * L.step[ax];
                const float pb = L.origin[ax] + (float)(idx[ax] + ((b >> ax) & 1)) * L.step[ax];
                o[ax] = mesh_lerp(pa, pb, t);
            }
            if (A.keys) A.keys[v0] = index * 7 + slot;
            ++v0;
        }
    }
    if (!P.ntri) return;
    unsigned long long t0 = offt[blockIdx.x] + (w >> 18);
    for (int t = 0; t < 6; ++t) {
        const uint32_t m = mesh_tet_mask(c_sp_rule, P.inside, t);
        const int pc = __popc(m);
        const int ntri = pc == 2 ? 2 : (pc == 1 || pc == 3) ? 1 : 0;
        for (int q = 0; q < ntri; ++q) {
            const uint32_t code = c_sp_rule.tri[t][m][q];
            int32_t *o = A.triangles + t0 * 3;
            for (int r = 0; r < 3; ++r) {
                const uint32_t cd = (code >> (6 * r)) & 63u;
                const int cor = (int)(cd >> 3), slot = (int)(cd & 7u);
                const int lq[3] = {Q.l[0] + (cor & 1), Q.l[1] + ((cor >> 1) & 1), Q.l[2] + (cor >> 2)};
                const EdgeOwner O = edge_owner(A, Q.K, Q.a, lq, MESH_SLOT_BITS[slot]);
                const size_t qp = (size_t)O.a * L.stride + local_index(L, O.l[0], O.l[1], O.l[2]);
                const uint32_t wq = A.word[qp];
                o[r] = (int32_t)((uint32_t)offv[qp >> 8] + ((wq >> 7) & 0x7ffu) + (uint32_t)__popc(wq & ((1u << slot) - 1u)));
            }
            ++t0;
        }
    }
}

hipError_t launch_sparse_coarse(const SparseArgs &A, const MlpArgs &M, int grid, hipStream_t st) {
    hipLaunchKernelGGL(k_sp_coarse, dim3(grid), dim3(256), smem16_bytes(M, NR_PRECISION_FP32, true), st, A, M);
    return hipGetLastError();
}

hipError_t launch_sparse_classify_count(const SparseArgs &A, hipStream_t st) {
    hipLaunchKernelGGL(k_sp_classify_count, dim3(A.nblk_b), dim3(256), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_sparse_classify_emit(const SparseArgs &A, hipStream_t st) {
    hipLaunchKernelGGL(k_sp_classify_emit, dim3(A.nblk_b), dim3(256), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_sparse_sample(const SparseArgs &A, const MlpArgs &M, int grid, hipStream_t st) {
    hipLaunchKernelGGL(k_sp_sample, dim3(grid), dim3(256), smem16_bytes(M, NR_PRECISION_FP32, true), st, A, M);
    return hipGetLastError();
}

hipError_t launch_sparse_mesh_count(const SparseArgs &A, hipStream_t st) {
    hipLaunchKernelGGL(k_sp_mesh_count, dim3(A.nblk_m), dim3(256), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_sparse_mesh_emit(const SparseArgs &A, hipStream_t st) {
    hipLaunchKernelGGL(k_sp_mesh_emit, dim3(A.nblk_m), dim3(256), 0, st, A);
    return hipGetLastError();
}

}  // namespace nr
