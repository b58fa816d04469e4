// nr_sample.hip -- seeded fitting samples of a triangle mesh (nr_mesh_sample): points on the surface
// in proportion to triangle area, optionally jittered, and points uniform in a box.  The contract is
// in include/neural_render.h; tests/sample_ref.py restates it in numpy.  Everything that decides a
// bit is an integer or one named f32 operation: Philox4x32-10 words, a binary search of the uint32
// area thresholds (nr_trimesh_host.cpp trimesh_area_table), 24-bit barycentrics and fmaf.
//
// k_mesh_sample.  One sample per lane, grid-stride over the samples; sample i draws from the counter
// (i, stream), so its bits do not depend on the grid.  The threshold table is read with per-lane
// loads (the top levels of the search are the same few lines for every lane: cache), the chosen
// position's record as three 16-byte loads.  No LDS, no scratch.
#include "nr_device.h"
#include "nr_internal.h"
#include "nr_kernels.h"

namespace nr {
namespace {

struct Words { uint32_t w0, w1, w2, w3; };

// Philox4x32-10 (Salmon et al., Random123): counter (c0, c1, c2, c3), key (k0, k1)
__device__ __forceinline__ Words philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1;
        c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Words{c0, c1, c2, c3};
}

// the eight-term uniform sum of a stream's words: unit variance, exact in integers up to the one product
__device__ __forceinline__ float jitter(const Words &w) {
    const int S = (int)((w.w0 & 0xffffu) + (w.w0 >> 16) + (w.w1 & 0xffffu) + (w.w1 >> 16) + (w.w2 & 0xffffu) + (w.w2 >> 16) +
                        (w.w3 & 0xffffu) + (w.w3 >> 16));
    return (float)(S - 262140) * __uint_as_float(0x379cc471u);
}

__global__ __launch_bounds__(256) void k_mesh_sample(const float4 *__restrict__ tris, const uint32_t *__restrict__ thr,
                                                     SampleArgs A) {
    const uint32_t k0 = (uint32_t)A.seed, k1 = (uint32_t)(A.seed >> 32);
    const float inv24 = 5.9604644775390625e-08f;  // 2^-24
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
        const uint32_t i0 = (uint32_t)i, i1 = (uint32_t)((unsigned long long)i >> 32);
        const Words w = philox(i0, i1, 0u, 0u, k0, k1);
        float p[3], bary[3] = {0.0f, 0.0f, 0.0f};
        int32_t tri = -1;
        if (i < A.n_surface) {
            // position = min(#{q : T_q <= w0}, last)
            int lo = 0, hi = A.ntl;
            while (lo < hi) {
                const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
                if (thr[mid] <= w.w0) lo = mid + 1; else hi = mid;
            }
            const int pos = lo < A.last ? lo : A.last;
            const float4 a = tris[(size_t)pos * 3], b = tris[(size_t)pos * 3 + 1], c = tris[(size_t)pos * 3 + 2];
            tri = __float_as_int(a.w);
            uint32_t iu = w.w1 >> 8, iv = w.w2 >> 8;
            if (iu + iv > (1u << 24)) { iu = (1u << 24) - iu; iv = (1u << 24) - iv; }
            const float u = (float)iu * inv24, v = (float)iv * inv24;
            bary[0] = (float)((1u << 24) - iu - iv) * inv24; bary[1] = u; bary[2] = v;
            p[0] = __builtin_fmaf(v, c.x - a.x, __builtin_fmaf(u, b.x - a.x, a.x));
            p[1] = __builtin_fmaf(v, c.y - a.y, __builtin_fmaf(u, b.y - a.y, a.y));
            p[2] = __builtin_fmaf(v, c.z - a.z, __builtin_fmaf(u, b.z - a.z, a.z));
            if (A.sigma > 0.0f) {
#pragma unroll
                for (int k = 0; k < 3; ++k) p[k] = __builtin_fmaf(A.sigma, jitter(philox(i0, i1, 1u + k, 0u, k0, k1)), p[k]);
            }
        } else {
            p[0] = __builtin_fmaf((float)(w.w0 >> 8) * inv24, A.ext[0], A.lo[0]);
            p[1] = __builtin_fmaf((float)(w.w1 >> 8) * inv24, A.ext[1], A.lo[1]);
            p[2] = __builtin_fmaf((float)(w.w2 >> 8) * inv24, A.ext[2], A.lo[2]);
        }
        float *o = A.points + (size_t)i * 3;
        o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
        if (A.tri) A.tri[i] = tri;
        if (A.bary) {
            float *q = A.bary + (size_t)i * 3;
            q[0] = bary[0]; q[1] = bary[1]; q[2] = bary[2];
        }
    }
}

}  // namespace

hipError_t launch_mesh_sample(const SampleArgs &A, int grid, hipStream_t st) {
    hipLaunchKernelGGL(k_mesh_sample, dim3(grid), dim3(256), 0, st, reinterpret_cast<const float4 *>(A.tris), A.thresholds, A);
    return hipGetLastError();
}

}  // namespace nr
