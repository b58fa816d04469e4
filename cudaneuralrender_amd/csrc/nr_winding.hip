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
#include "nr_trimesh_wave.h"

namespace nr {
namespace {

// the sum itself: trimesh_winding_wave (nr_trimesh_wave.h), here over chunks of the caller's array
__global__ __launch_bounds__(256) void k_trimesh_winding(const float4 *__restrict__ nodes, const float4 *__restrict__ tris,
                                                         const float4 *__restrict__ moments, TriWindArgs A) {
    __shared__ int stacks[4][TRIMESH_STACK][2];
    trimesh_winding_wave(nodes, tris, moments, A, PointArraySrc{A.X, A.n}, stacks[threadIdx.x >> 6]);
}

}  // namespace

hipError_t launch_trimesh_winding(const TriWindArgs &A, int grid, hipStream_t st) {
    hipLaunchKernelGGL(k_trimesh_winding, dim3(grid), dim3(256), 0, st, reinterpret_cast<const float4 *>(A.nodes),
                       reinterpret_cast<const float4 *>(A.tris), reinterpret_cast<const float4 *>(A.moments), A);
    return hipGetLastError();
}

}  // namespace nr
