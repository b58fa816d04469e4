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
#include "nr_trimesh_wave.h"

namespace nr {
namespace {

// the walk itself: trimesh_distance_wave (nr_trimesh_wave.h), here over chunks of the caller's array
__global__ __launch_bounds__(256) void k_trimesh_distance(const float4 *__restrict__ nodes, const float4 *__restrict__ tris,
                                                          const float *__restrict__ table, TriMeshArgs A) {
    __shared__ int stacks[4][TRIMESH_STACK];
    trimesh_distance_wave(nodes, tris, table, A, PointArraySrc{A.X, A.n}, stacks[threadIdx.x >> 6]);
}

}  // namespace

hipError_t launch_trimesh_distance(const TriMeshArgs &A, int grid, hipStream_t st) {
    hipLaunchKernelGGL(k_trimesh_distance, dim3(grid), dim3(256), 0, st, reinterpret_cast<const float4 *>(A.nodes),
                       reinterpret_cast<const float4 *>(A.tris), A.table, A);
    return hipGetLastError();
}

}  // namespace nr
