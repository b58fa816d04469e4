// nr_grad.hip -- the network's analytic gradient (nr_mlp_gradient): value, d value / d input and
// the normalised gradient of every point, in one launch.  The evaluation (forward with masks, backward
// on the transposed kernels) is mlp16_grad of nr_grad.h.
#include "nr_grad.h"

namespace nr {

// Persistent waves deal the 64-point chunks grid-stride (k_grid's scheme); both packs are staged
// once per workgroup.  Lanes past the end evaluate the finite point 0 and skip their stores.
template <int IN0>
__global__ __launch_bounds__(64 * NR_GRAD_WAVES, NR_GRAD_WAVES / 2) void k_grad(GradArgs G, MlpArgs M) {
    {
        const int4 *src = reinterpret_cast<const int4 *>(G.gb);
        int4 *dst = reinterpret_cast<int4 *>(nr_smem16 + M.pk_bytes);
        for (int i = threadIdx.x; i < G.gb_bytes / 16; i += blockDim.x) dst[i] = src[i];
    }
    Smem16 S = stage16<NR_PRECISION_FP32, true>(M);  // (its __syncthreads covers the copy above)
    const float *sb = reinterpret_cast<const float *>(nr_smem16 + M.pk_bytes);
    M.in0 = IN0;
    const int lane = lane_id();
    const uint32_t n = (uint32_t)G.n;
    const uint32_t nchunks = (n + 63u) >> 6;
    const uint32_t wave =
        (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (uint32_t)NR_GRAD_WAVES + (threadIdx.x >> 6)));
    const uint32_t waves = (uint32_t)__builtin_amdgcn_readfirstlane((int)(gridDim.x * (uint32_t)NR_GRAD_WAVES));
    for (uint32_t c = wave; c < nchunks; c += waves) {
        const uint32_t base = c << 6, idx = base + (uint32_t)lane;
        const bool live = idx < n;
        float x = 0.0f, y = 0.0f, z = 0.0f, f = 0.0f;
        if (live) {
            const float *xp = G.X + (size_t)idx * IN0;
            x = xp[0]; y = xp[1]; z = xp[2];
            if constexpr (IN0 == 4) f = xp[3];
        }
        const uint32_t rem = n - base;
        const uint32_t tmask = rem >= 64u ? 0xfu : (1u << ((rem + 15u) >> 4)) - 1u;
        float gr[4];
        const float v = mlp16_grad(M, S.s32, sb, f, x, y, z, tmask, gr);
        if (live) {
            if (G.value) G.value[idx] = v;
            if (G.grad) {
                float *o = G.grad + (size_t)idx * IN0;
                o[0] = gr[0]; o[1] = gr[1]; o[2] = gr[2];
                if constexpr (IN0 == 4) o[3] = gr[3];
            }
            if (G.normal) {
                const F3 nrm = normalize3(mk3(gr[0], gr[1], gr[2]));
                float *o = G.normal + (size_t)idx * 3;
                o[0] = nrm.x; o[1] = nrm.y; o[2] = nrm.z;
            }
        }
    }
}

int grad_lds_bytes(const MlpArgs &M, const GradArgs &G) { return smem16_bytes(M, NR_PRECISION_FP32, true) + G.gb_bytes; }

hipError_t launch_grad(const GradArgs &G, const MlpArgs &M, int grid, hipStream_t st) {
    const int sm = grad_lds_bytes(M, G);
    if (M.in0 == 4) hipLaunchKernelGGL(k_grad<4>, dim3(grid), dim3(64 * NR_GRAD_WAVES), sm, st, G, M);
    else hipLaunchKernelGGL(k_grad<3>, dim3(grid), dim3(64 * NR_GRAD_WAVES), sm, st, G, M);
    return hipGetLastError();
}

}  // namespace nr
