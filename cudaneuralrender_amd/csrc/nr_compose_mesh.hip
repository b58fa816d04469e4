// nr_compose_mesh.hip -- composed scenes on a lattice: the samplers and the vertex pass of
// nr_compose_sample_grid, nr_compose_extract_mesh and nr_compose_extract_mesh_sparse (the contract
// is in include/neural_render.h).  The four kernels of the mesh pipeline that touch a network, with
// compose_field (nr_compose_field.h) in the place of one MLP and its scene:
//
//   k_compose_grid       k_grid: value and / or owner at every point of a dense lattice
//   k_compose_sp_coarse  k_sp_coarse: the value at the brick corners
//   k_compose_sp_sample  k_sp_sample: the point sets of the active bricks into the compact store
//   k_compose_vertex     k_vnormal: the owner and the normal at every vertex of the mesh
//
// The classify, count, scan and emit passes (nr_mesh.hip, nr_sparse.hip) work on values alone and
// run unchanged.  As in k_compose every distinct pack is staged once per workgroup into dynamic LDS
// -- four of them leave room for one workgroup per CU, so the workgroup is k_compose's, up to 12
// waves, and the wave count is read from blockDim -- the part table stays in the kernarg segment,
// the part loop is wave-uniform and a part's network runs only on the tiles that hold a point inside
// its bound: a chunk of 64 lattice points outside every bound costs no MLP evaluation.  A point's
// coordinate comes from its global lattice index (nr_lattice.h) and its value depends on nothing
// else, so the outputs are the same bits for any workgroup size, grid or enclosing lattice.  The only
// atomics are the per-wave statistics adds.
#include "nr_compose_field.h"
#include "nr_lattice.h"

namespace nr {

// this wave's index among the launch's waves, and their number (wave-uniform)
__device__ __forceinline__ uint32_t compose_wave(uint32_t &waves) {
    const uint32_t wpg = blockDim.x >> 6;
    waves = (uint32_t)__builtin_amdgcn_readfirstlane((int)(gridDim.x * wpg));
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * wpg + (threadIdx.x >> 6)));
}

// one set of statistics atomics per wave; pairs: the sampling passes count them, the vertex pass does not
__device__ __forceinline__ void compose_count_flush(const ComposeArgs &C, const FieldCount &cnt, bool pairs) {
    if (lane_id() != 0) return;
    if (pairs && cnt.pairs) atomicAdd(C.stats + 4, (unsigned long long)cnt.pairs);
    if (cnt.evals) atomicAdd(C.stats + 5, (unsigned long long)cnt.evals);
    if (cnt.skips) atomicAdd(C.stats + 6, (unsigned long long)cnt.skips);
}

// a wave's counters stay below 2^32: flushed once any of them passes 2^30 (a chunk adds at most 64 x 16)
__device__ __forceinline__ void compose_count_guard(const ComposeArgs &C, FieldCount &cnt, bool pairs) {
    if ((cnt.pairs | cnt.evals | cnt.skips) >= (1u << 30)) {
        compose_count_flush(C, cnt, pairs);
        cnt = FieldCount{0, 0, 0};
    }
}

// ---------------------------------------------------------------- dense sampler
// k_grid's loop: persistent waves deal the 64-point chunks of the linear index grid-stride.  Lanes
// past the end hold no point (compose_field's `live`): they feed the networks zeros and skip the store.
__global__ __launch_bounds__(NR_COMPOSE_MAX_THREADS) void k_compose_grid(ComposeArgs C, ComposeGridArgs G) {
    const float *lds = compose_stage(C);
    const int lane = lane_id();
    const float fr = (float)C.frame;
    const uint32_t n = (uint32_t)G.L.n;
    const uint32_t nchunks = (n + 63u) >> 6;
    uint32_t waves;
    const uint32_t wave = compose_wave(waves);
    FieldCount cnt{0, 0, 0};
    for (uint32_t c = wave; c < nchunks; c += waves) {
        const uint32_t idx = (c << 6) + (uint32_t)lane;
        const bool live = idx < n;
        F3 p = mk3(0.0f, 0.0f, 0.0f);
        if (live) {
            int i, j, k;
            lattice_ijk(G.L, idx, i, j, k);
            p = mk3(G.L.origin[0] + (float)i * G.L.step[0], G.L.origin[1] + (float)j * G.L.step[1],
                    G.L.origin[2] + (float)k * G.L.step[2]);
        }
        int own;
        const float v = compose_field(C, lds, fr, p, live, own, cnt);
        if (live) {
            if (G.value) G.value[idx] = v;
            if (G.owner) G.owner[idx] = own;
        }
        compose_count_guard(C, cnt, true);
    }
    compose_count_flush(C, cnt, true);
}

// ---------------------------------------------------------------- brick-corner sampler
__global__ __launch_bounds__(NR_COMPOSE_MAX_THREADS) void k_compose_sp_coarse(ComposeArgs C, SparseArgs A) {
    const float *lds = compose_stage(C);
    const SparseLattice &L = A.L;
    const int lane = lane_id();
    const float fr = (float)C.frame;
    const uint32_t n = L.ncoarse;
    const uint32_t nchunks = (n + 63u) >> 6;
    const uint32_t cx = (uint32_t)L.nbx + 1u, cxy = cx * ((uint32_t)L.nby + 1u);
    uint32_t waves;
    const uint32_t wave = compose_wave(waves);
    FieldCount cnt{0, 0, 0};
    for (uint32_t c = wave; c < nchunks; c += waves) {
        const uint32_t idx = (c << 6) + (uint32_t)lane;
        const bool live = idx < n;
        F3 p = mk3(0.0f, 0.0f, 0.0f);
        if (live) p = corner_point(L, idx, cx, cxy);
        int own;
        const float v = compose_field(C, lds, fr, p, live, own, cnt);
        if (live) A.coarse[idx] = v;
        compose_count_guard(C, cnt, true);
    }
    compose_count_flush(C, cnt, true);
}

// ---------------------------------------------------------------- active-brick sampler
// k_sp_sample's chunks: chunk c = the 64 store points from 64 c, all of brick slot c / (stride / 64).
// Store points past the brick's S^3, and those past a ragged brick's extent, hold no point.
__global__ __launch_bounds__(NR_COMPOSE_MAX_THREADS) void k_compose_sp_sample(ComposeArgs C, SparseArgs A) {
    const float *lds = compose_stage(C);
    const SparseLattice &L = A.L;
    const int lane = lane_id();
    const float fr = (float)C.frame;
    const uint32_t wpb = L.stride >> 6;
    const uint32_t nchunks = A.nactive * wpb;  // < 2^31 (the host checks)
    uint32_t waves;
    const uint32_t wave = compose_wave(waves);
    FieldCount cnt{0, 0, 0};
    for (uint32_t c = wave; c < nchunks; c += waves) {
        const uint32_t a = udiv_r(c, wpb, L.inv_wpb);
        const uint32_t r = ((c - a * wpb) << 6) + (uint32_t)lane;
        const Brick K = brick_of(L, A.list[a]);
        bool live = r < L.P;
        F3 p = mk3(0.0f, 0.0f, 0.0f);
        if (live) {
            int li, lj, lk;
            local_ijk(L, r, li, lj, lk);
            live = li <= K.e[0] && lj <= K.e[1] && lk <= K.e[2];
            if (live) p = lattice_point(L, L.B * K.b[0] + li, L.B * K.b[1] + lj, L.B * K.b[2] + lk);
        }
        int own;
        const float v = compose_field(C, lds, fr, p, live, own, cnt);
        if (live) A.store[(size_t)a * L.stride + r] = v;
        compose_count_guard(C, cnt, true);
    }
    compose_count_flush(C, cnt, true);
}

// ---------------------------------------------------------------- vertex pass
// A wave takes 64 consecutive vertices at a time.  With `part`: one field evaluation at the vertices,
// for the owner.  With `normals`: k_compose's normal passes over them, 16 vertices x 4 tetrahedron
// samples each (lane 4 v + q = sample q of the pass's vertex v); the lanes of a short last pass
// repeat its first vertex, as in k_vnormal, and hold no point.
__global__ __launch_bounds__(NR_COMPOSE_MAX_THREADS) void k_compose_vertex(ComposeArgs C, ComposeVertexArgs V) {
    const float *lds = compose_stage(C);
    const int lane = lane_id();
    const int q4 = lane & 3, kv = lane >> 2;
    const float fr = (float)C.frame;
    const uint32_t nv = (uint32_t)V.nv;
    const uint32_t nchunks = (nv + 63u) >> 6;
    uint32_t waves;
    const uint32_t wave = compose_wave(waves);
    FieldCount cnt{0, 0, 0};
    for (uint32_t c = wave; c < nchunks; c += waves) {
        const uint32_t base = c << 6;
        const uint32_t nb64 = min(64u, nv - base);
        if (V.part) {
            const bool live = (uint32_t)lane < nb64;
            F3 p = mk3(0.0f, 0.0f, 0.0f);
            if (live) {
                const float *vp = V.vertices + (size_t)(base + (uint32_t)lane) * 3;
                p = mk3(vp[0], vp[1], vp[2]);
            }
            int own;
            (void)compose_field(C, lds, fr, p, live, own, cnt);
            if (live) V.part[base + (uint32_t)lane] = own;
        }
        if (V.normals) {
            for (uint32_t b16 = 0; b16 < nb64; b16 += 16u) {
                const uint32_t nb = min(16u, nb64 - b16);
                const bool live = (uint32_t)kv < nb;
                const uint32_t vi = base + b16 + (live ? (uint32_t)kv : 0u);
                const float *vp = V.vertices + (size_t)vi * 3;
                const F3 cq = compose_tet_term(C, lds, fr, mk3(vp[0], vp[1], vp[2]), q4, live, cnt);
                const F3 c1 = quad_bcast3_1(cq), c2 = quad_bcast3_2(cq), c3 = quad_bcast3_3(cq);
                if (live && q4 == 0) {
                    const F3 nrm = normalize3(add3(add3(add3(cq, c1), c2), c3));
                    float *o = V.normals + (size_t)vi * 3;
                    o[0] = nrm.x; o[1] = nrm.y; o[2] = nrm.z;
                }
            }
        }
        compose_count_guard(C, cnt, false);
    }
    compose_count_flush(C, cnt, false);
}

// the packs are the workgroup's only dynamic LDS; more than 64 KB of it has to be asked for
template <class K, class X>
static hipError_t compose_mesh_launch(K kernel, const ComposeArgs &C, const X &args, int grid, int threads, hipStream_t st) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             C.pack_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), C.pack_bytes, st, C, args);
    return hipGetLastError();
}

hipError_t launch_compose_grid(const ComposeArgs &C, const ComposeGridArgs &G, int grid, int threads, hipStream_t st) {
    return compose_mesh_launch(k_compose_grid, C, G, grid, threads, st);
}

hipError_t launch_compose_vertex(const ComposeArgs &C, const ComposeVertexArgs &V, int grid, int threads, hipStream_t st) {
    return compose_mesh_launch(k_compose_vertex, C, V, grid, threads, st);
}

hipError_t launch_compose_sp_coarse(const ComposeArgs &C, const SparseArgs &A, int grid, int threads, hipStream_t st) {
    return compose_mesh_launch(k_compose_sp_coarse, C, A, grid, threads, st);
}

hipError_t launch_compose_sp_sample(const ComposeArgs &C, const SparseArgs &A, int grid, int threads, hipStream_t st) {
    return compose_mesh_launch(k_compose_sp_sample, C, A, grid, threads, st);
}

}  // namespace nr
