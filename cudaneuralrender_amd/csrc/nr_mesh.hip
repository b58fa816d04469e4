// nr_mesh.hip -- SDF volume sampling and isosurface extraction (nr_sample_grid, nr_mesh_grid,
// nr_extract_mesh): the scene's distance on a lattice whose points the kernel generates, and
// marching tetrahedra on the Kuhn split of its cells (the rule: include/neural_render.h,
// nr_mesh_rule.h).
//
// k_grid and k_vnormal run the fp32 MLP through the device functions k_trace and k_query use
// (nr_device.h, nr_mlp16.h): mlp16_fp32 on 16-point tiles, then scene_sdf.  A point's value
// depends only on that point -- the MLP's tiles are column-independent and the scene's wave-wide
// screens choose between bit-identical forms -- so the lattice values are the same bits for any
// grid, occupancy or lattice that contains the point.
//
// The extraction is three memory-bound passes over the 4 B/point lattice, in 256-point blocks of
// the linear index: k_mesh_count (each point's vertex mask and its position in its block, the
// block's totals), k_mesh_scan (exclusive scan of the block totals, one workgroup) and k_mesh_emit
// (every point writes its vertices and its cell's triangles at the scanned positions).  No atomic
// decides an order: the output is a pure function of the inputs.
#include "nr_lattice.h"
#include "nr_mesh_rule.h"
#include "nr_mlp16.h"

namespace nr {

// waves per SIMD k_grid / k_vnormal's registers are allocated for
#ifndef NR_GRID_WPS
#define NR_GRID_WPS 4
#endif

static __constant__ MeshRule c_mesh_rule = make_mesh_rule();

// ---------------------------------------------------------------- sampler
// Persistent waves deal the 64-point chunks of the linear index grid-stride; the fp32 pack is staged
// once per workgroup.  The last chunk keeps all 64 lanes running through the scene (its wave-wide
// ballots): lanes past the end evaluate the finite point (0, 0, 0) and skip the store.
__global__ __launch_bounds__(256, NR_GRID_WPS) void k_grid(GridArgs G, MlpArgs M) {
    Smem16 S = stage16<NR_PRECISION_FP32, true>(M);
    const int lane = lane_id();
    const float fr = (float)G.frame;
    const double zoff = sphere_zoff(G.frame);
    const uint32_t n = (uint32_t)G.L.n;
    const uint32_t nchunks = (n + 63u) >> 6;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const uint32_t waves = (uint32_t)__builtin_amdgcn_readfirstlane((int)(gridDim.x * 4u));
    for (uint32_t c = wave; c < nchunks; c += waves) {
        const uint32_t base = c << 6, idx = base + (uint32_t)lane;
        const bool live = idx < n;
        F3 p = mk3(0.0f, 0.0f, 0.0f);
        if (live) {
            int i, j, k;
            lattice_ijk(G.L, idx, i, j, k);
            p = mk3(G.L.origin[0] + (float)i * G.L.step[0], G.L.origin[1] + (float)j * G.L.step[1],
                    G.L.origin[2] + (float)k * G.L.step[2]);
        }
        const uint32_t rem = n - base;
        const uint32_t tmask = rem >= 64u ? 0xfu : (1u << ((rem + 15u) >> 4)) - 1u;
        float sdf = mlp16_fp32(M, S.s32, fr, p.x, p.y, p.z, tmask);
        if (!live) sdf = 0.0f;  // (a tile the MLP skipped holds no value)
        const float v = scene_sdf(p, sdf, G.scene, zoff);
        if (live) G.sdf[idx] = v;
    }
}

// ---------------------------------------------------------------- vertex normals
// nr_trace_rays' hit normal over the vertex list: 16 vertices x 4 tetrahedron samples per pass,
// lane 4 v + q = sample q of the pass's vertex v (k_query's normal pass).  The lanes of a short last
// pass repeat its first vertex.
__global__ __launch_bounds__(256, NR_GRID_WPS) void k_vnormal(VNormalArgs V, MlpArgs M) {
    Smem16 S = stage16<NR_PRECISION_FP32, true>(M);
    const int lane = lane_id();
    const int q4 = lane & 3, kv = lane >> 2;
    const float fr = (float)V.frame;
    const double zoff = sphere_zoff(V.frame);
    const uint32_t nv = (uint32_t)V.nv;
    const uint32_t npass = (nv + 15u) >> 4;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const uint32_t waves = (uint32_t)__builtin_amdgcn_readfirstlane((int)(gridDim.x * 4u));
    for (uint32_t c = wave; c < npass; c += waves) {
        const uint32_t base = c << 4;
        const uint32_t nb = min(16u, nv - base);
        const uint32_t vi = base + ((uint32_t)kv < nb ? (uint32_t)kv : 0u);
        const float *vp = V.vertices + (size_t)vi * 3;
        const F3 sp = mk3(vp[0], vp[1], vp[2]);
        // tetrahedron point q (c_tet): x = +1 for q = 0, 3; y = +1 for q = 2, 3; z = +1 for q = 1, 3
        int qo = q4;
        asm volatile("" : "+v"(qo));
        const F3 tp = mk3((qo == 0 || qo == 3) ? 1.0f : -1.0f, qo >= 2 ? 1.0f : -1.0f, (qo & 1) ? 1.0f : -1.0f);
        const F3 pq = add3(sp, mul3s(tp, NORMAL_EPSILON));
        const uint32_t smask = (1u << ((4u * nb + 15u) >> 4)) - 1u;
        const float sdf = mlp16_fp32(M, S.s32, fr, pq.x, pq.y, pq.z, smask);
        const F3 cq = mul3s(tp, scene_sdf(pq, sdf, V.scene, zoff));
        const F3 c1 = quad_bcast3_1(cq), c2 = quad_bcast3_2(cq), c3 = quad_bcast3_3(cq);
        if ((uint32_t)kv < nb && q4 == 0) {
            const F3 nrm = normalize3(add3(add3(add3(cq, c1), c2), c3));
            float *o = V.normals + (size_t)vi * 3;
            o[0] = nrm.x; o[1] = nrm.y; o[2] = nrm.z;
        }
    }
}

// ---------------------------------------------------------------- count, scan, emit
// One thread per lattice point, 256 per block.  The block's exclusive scan of (vertices, triangles)
// runs on one packed word: a block holds at most 256 x 7 vertices (bits 0-15) and 256 x 12
// triangles (bits 16-31).
__global__ __launch_bounds__(256) void k_mesh_count(MeshArgs A) {
    __shared__ uint32_t wtot[4];
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    const int lane = lane_id(), wid = threadIdx.x >> 6;
    const bool live = p < (uint32_t)A.L.n;
    uint32_t vmask = 0, packed = 0;
    if (live) {
        int i, j, k;
        lattice_ijk(A.L, p, i, j, k);
        const MeshPoint P = mesh_point(c_mesh_rule, A.sdf, p, i, j, k, A.L.nx, A.L.ny, A.L.nz, A.iso);
        vmask = P.vmask;
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
    if (live) A.word[p] = vmask | ((excl & 0xffffu) << 7) | ((excl >> 16) << 18);
    if (threadIdx.x == 255) {
        const uint32_t tot = before + incl;
        A.cnt[blockIdx.x] = tot & 0xffffu;
        A.cnt[A.nblk + blockIdx.x] = tot >> 16;
    }
}

// Exclusive scans of the two rows of block totals, 64-bit, by one workgroup: 1024 blocks per
// step (their sums fit 32 bits), the running totals carried from step to step.
__global__ __launch_bounds__(1024) void k_mesh_scan(MeshArgs A) {
    __shared__ uint32_t wtot[2][16];
    const int lane = lane_id(), wid = threadIdx.x >> 6;
    unsigned long long carry[2] = {0ull, 0ull};
    for (int base = 0; base < A.nblk; base += 1024) {
        const int b = base + (int)threadIdx.x;
        uint32_t v[2], incl[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            v[q] = b < A.nblk ? A.cnt[q * A.nblk + b] : 0u;
            incl[q] = v[q];
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t t = __shfl_up(incl[q], off);
                if (lane >= off) incl[q] += t;
            }
            if (lane == 63) wtot[q][wid] = incl[q];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            uint32_t before = 0, all = 0;
            for (int w = 0; w < 16; ++w) {
                if (w < wid) before += wtot[q][w];
                all += wtot[q][w];
            }
            if (b < A.nblk) A.off[q * A.nblk + b] = carry[q] + before + incl[q] - v[q];
            carry[q] += all;
        }
        __syncthreads();  // wtot is rewritten by the next step
    }
    if (threadIdx.x == 0) {
        A.total[0] = carry[0];
        A.total[1] = carry[1];
    }
}

__global__ __launch_bounds__(256) void k_mesh_emit(MeshArgs A) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= (uint32_t)A.L.n) return;
    int i, j, k;
    lattice_ijk(A.L, p, i, j, k);
    const MeshPoint P = mesh_point(c_mesh_rule, A.sdf, p, i, j, k, A.L.nx, A.L.ny, A.L.nz, A.iso);
    if (!P.vmask && !P.ntri) return;
    const uint32_t w = A.word[p];
    const unsigned long long *offv = A.off, *offt = A.off + A.nblk;
    mesh_emit_point(c_mesh_rule, P, A.L.origin, A.L.step, p, i, j, k, (uint32_t)A.L.nx,
                    (uint32_t)A.L.nx * (uint32_t)A.L.ny, A.iso, A.word, offv, offv[blockIdx.x] + ((w >> 7) & 0x7ffu),
                    offt[blockIdx.x] + (w >> 18), A.vertices, A.triangles);
}

hipError_t launch_grid(const GridArgs &G, const MlpArgs &M, int grid, hipStream_t st) {
    hipLaunchKernelGGL(k_grid, dim3(grid), dim3(256), smem16_bytes(M, NR_PRECISION_FP32, true), st, G, M);
    return hipGetLastError();
}

hipError_t launch_vnormal(const VNormalArgs &V, const MlpArgs &M, int grid, hipStream_t st) {
    hipLaunchKernelGGL(k_vnormal, dim3(grid), dim3(256), smem16_bytes(M, NR_PRECISION_FP32, true), st, V, M);
    return hipGetLastError();
}

hipError_t launch_mesh_count(const MeshArgs &A, hipStream_t st) {
    hipLaunchKernelGGL(k_mesh_count, dim3(A.nblk), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(1024), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_mesh_scan(const MeshArgs &A, hipStream_t st) {
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(1024), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_mesh_emit(const MeshArgs &A, hipStream_t st) {
    hipLaunchKernelGGL(k_mesh_emit, dim3(A.nblk), dim3(256), 0, st, A);
    return hipGetLastError();
}

}  // namespace nr
