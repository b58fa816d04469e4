// nr_trimesh_grid.hip -- a triangle mesh's signed distance on a lattice (nr_mesh_sample_grid,
// nr_mesh_remesh, nr_mesh_remesh_sparse): the point queries' per-wave bodies
// (nr_trimesh_wave.h; no arithmetic of its own) over points generated in the kernel.
//
//   k_trimesh_grid_distance<Src>   trimesh_distance_wave: the value with the pseudonormal sign
//   k_trimesh_grid_winding<Src>    trimesh_winding_wave with sdf: the magnitudes just written, signed in
//                                  place by w >= 0.5f (NR_SAMPLE_SIGN_WINDING; a second launch, as
//                                  nr_mesh_winding's sdf output)
// for the three lattice sources:
//   LatticeBlockSrc   a wave owns 4 x 4 x 4 blocks of the lattice, grid-stride over the blocks: the 64
//                     points of a wave fill a small cube, the best case of the shared walk (few boxes
//                     are near some lane and far from all others); the blocks are dealt in tiles of
//                     8 x 8 x 8, so the waves running together read the same part of the tree;
//   CornerBlockSrc    the same blocks over the brick-corner lattice, into SparseArgs::coarse;
//   BrickStoreSrc     64 consecutive store points of an active brick, into SparseArgs::store.
// A lane of a ragged block that lies outside the lattice is not live, exactly like the tail lanes of
// k_trimesh_distance.  Every loop is the bodies' own: bounded by nnodes, the stack and a leaf's count.
#include <algorithm>

#include "nr_trimesh_wave.h"

namespace nr {
namespace {

// amdgpu_num_sgpr(100): the scalar registers of k_trimesh_distance's 8 waves per SIMD.  A source's
// lattice constants would otherwise stay in scalar registers across the walk and cost a wave; capped,
// a few of them wait in spare vector lanes (no scratch: profiles/trimesh_grid_resources.txt).
template <class Src>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(100))) void k_trimesh_grid_distance(
    const float4 *__restrict__ nodes, const float4 *__restrict__ tris, const float *__restrict__ table, TriMeshArgs A, Src src) {
    __shared__ int stacks[4][TRIMESH_STACK];
    trimesh_distance_wave(nodes, tris, table, A, src, stacks[threadIdx.x >> 6]);
}

template <class Src>
__global__ __launch_bounds__(256) void k_trimesh_grid_winding(const float4 *__restrict__ nodes, const float4 *__restrict__ tris,
                                                              const float4 *__restrict__ moments, TriWindArgs A, Src src) {
    __shared__ int stacks[4][TRIMESH_STACK][2];
    trimesh_winding_wave(nodes, tris, moments, A, src, stacks[threadIdx.x >> 6]);
}

// the distance launch and, with W, the winding launch that signs its values
template <class Src>
hipError_t launch_both(const TriMeshArgs &D, const TriWindArgs *W, const Src &src, int grid, hipStream_t st) {
    hipLaunchKernelGGL(k_trimesh_grid_distance<Src>, dim3(grid), dim3(256), 0, st, reinterpret_cast<const float4 *>(D.nodes),
                       reinterpret_cast<const float4 *>(D.tris), D.table, D, src);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !W) return e;
    hipLaunchKernelGGL(k_trimesh_grid_winding<Src>, dim3(grid), dim3(256), 0, st, reinterpret_cast<const float4 *>(W->nodes),
                       reinterpret_cast<const float4 *>(W->tris), reinterpret_cast<const float4 *>(W->moments), *W, src);
    return hipGetLastError();
}

// a grid-stride over chunks of 64 points: at most 8 four-wave workgroups per CU, as the point calls
int grid_for(size_t chunks, int cus) {
    return (int)std::max<size_t>(1, std::min<size_t>((chunks + 3) / 4, (size_t)cus * 8));
}

}  // namespace

hipError_t launch_trimesh_lattice(const TriMeshArgs &D, const TriWindArgs *W, const LatticeArgs &L, int cus, hipStream_t st) {
    const LatticeBlockSrc src = make_lattice_blocks(L);
    return launch_both(D, W, src, grid_for(src.chunks, cus), st);
}

hipError_t launch_trimesh_sparse(const TriMeshArgs &D, const TriWindArgs *W, const SparseArgs &S, bool store, int cus,
                                 hipStream_t st) {
    if (store) {
        const BrickStoreSrc src{S.L, S.list, S.nactive};
        return launch_both(D, W, src, grid_for((size_t)S.nactive * (S.L.stride >> 6), cus), st);
    }
    const CornerBlockSrc src = make_corner_blocks(S.L);
    return launch_both(D, W, src, grid_for(src.nblocks, cus), st);
}

}  // namespace nr
