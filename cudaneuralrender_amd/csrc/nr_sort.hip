// nr_sort.hip -- the stable order of a point set (nr_points_order): 32-bit keys (a 30-bit Morton code
// or a seeded Philox word) with the point's index as payload, sorted by a stable LSD radix sort of
// four 8-bit passes, and the gather that applies a permutation.  The contract is in
// include/neural_render.h: perm = the stable ascending argsort of the keys.
//
// A pass is three kernels, and every dependency between workgroups is a kernel boundary -- no
// workgroup ever waits on another, nothing spins on global memory:
//   k_sort_hist     a workgroup counts the 256 digits of its tile of SORT_TILE keys (counts in LDS) and
//                   writes them digit-major: table[digit][block];
//   k_sort_scan     one workgroup scans the table exclusively, SORT_SCAN_STEP entries a step, carrying
//                   the total (nr_mesh.hip k_mesh_scan's pattern): table[digit][block] becomes where
//                   the block's first key of that digit goes;
//   k_sort_scatter  a workgroup ranks its tile stably and writes key and payload to their places.
// The stable rank.  Wave w of a workgroup owns the contiguous keys [512 w, 512 w + 512) of the tile and
// takes them 64 at a time, in order.  The lanes of a wave that hold the same digit are found by eight
// ballots, one per digit bit; a key's rank among them is the count of such lanes below its own.  A
// per-wave, per-digit running count in LDS orders the wave's eight rounds, and the four waves'
// counts are prefix-summed per digit in LDS.  No atomic decides a position: the output is a pure
// function of the keys.  (k_sort_hist adds each group's size to the LDS count once, by its lowest
// lane: the sum does not depend on the order of the adds.)
#include <algorithm>

#include "nr_device.h"
#include "nr_internal.h"
#include "nr_kernels.h"

namespace nr {
namespace {

constexpr int ROUNDS = SORT_TILE / 256;  // 64-key rounds per wave
static_assert(SORT_TILE == 4 * 64 * ROUNDS, "a tile is four waves' rounds");
static_assert(SORT_SCAN_STEP == 4 * 1024, "a scan step is four entries per thread");

// Philox4x32-10, word 0 of counter (i, stream 4) (nr_sample.hip has the generator's four words)
__device__ __forceinline__ uint32_t philox_w0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1;
        c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

__device__ __forceinline__ uint32_t spread10(uint32_t v) {
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    return (v | (v << 2)) & 0x09249249u;
}

// q = 1023 if t >= 1023, (int)t if t > 0, else 0 (a NaN: 0)
__device__ __forceinline__ uint32_t quantise(float x, float lo, float inv) {
    const float t = (x - lo) * inv;
    return t >= 1023.0f ? 1023u : (t > 0.0f ? (uint32_t)(int)t : 0u);
}

__global__ __launch_bounds__(256) void k_sort_keys(SortArgs A) {
    const long stride = (long)gridDim.x * 256;
    const uint32_t k0 = (uint32_t)A.seed, k1 = (uint32_t)(A.seed >> 32);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
        uint32_t key;
        if (A.mode == NR_ORDER_MORTON) {
            const float *p = A.X + (size_t)i * 3;
            key = spread10(quantise(p[0], A.lo[0], A.inv[0])) | (spread10(quantise(p[1], A.lo[1], A.inv[1])) << 1) |
                  (spread10(quantise(p[2], A.lo[2], A.inv[2])) << 2);
        } else {
            key = philox_w0((uint32_t)i, (uint32_t)((unsigned long long)i >> 32), 4u, 0u, k0, k1);
        }
        A.keys[0][i] = key;
        A.vals[0][i] = (uint32_t)i;
    }
}

// the lanes of the wave that are valid and hold digit d (for a valid lane; eight ballots)
__device__ __forceinline__ unsigned long long same_digit(uint32_t d, bool valid) {
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long bb = __ballot(bit);
        m &= bit ? bb : ~bb;
    }
    return m;
}
// how many lanes of m lie below this one
__device__ __forceinline__ uint32_t lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__global__ __launch_bounds__(256) void k_sort_hist(const uint32_t *__restrict__ keys, long n, int shift, uint32_t *__restrict__ table,
                                                   int nblk) {
    __shared__ uint32_t cnt[256];
    cnt[threadIdx.x] = 0u;
    __syncthreads();
    const long base = (long)blockIdx.x * SORT_TILE;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const long idx = base + r * 256 + threadIdx.x;
        const bool valid = idx < n;
        const uint32_t d = valid ? (keys[idx] >> shift) & 255u : 0u;
        const unsigned long long m = same_digit(d, valid);
        if (valid && lanes_below(m) == 0u) atomicAdd(&cnt[d], (uint32_t)__popcll(m));
    }
    __syncthreads();
    table[(size_t)threadIdx.x * nblk + blockIdx.x] = cnt[threadIdx.x];
}

__global__ __launch_bounds__(1024) void k_sort_scan(uint32_t *__restrict__ table, int M) {
    __shared__ uint32_t wtot[16];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t carry = 0u;
    for (int base = 0; base < M; base += SORT_SCAN_STEP) {
        const int i = base + (int)threadIdx.x * 4;  // M is a multiple of 4: the four entries are in or out together
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (i < M) v = *reinterpret_cast<const uint4 *>(table + i);
        const uint32_t s = (v.x + v.y) + (v.z + v.w);
        uint32_t incl = s;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t = __shfl_up(incl, off);
            if (lane >= off) incl += t;
        }
        if (lane == 63) wtot[wid] = incl;
        __syncthreads();
        uint32_t before = 0u, all = 0u;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            if (w < wid) before += wtot[w];
            all += wtot[w];
        }
        const uint32_t ex = carry + before + incl - s;
        if (i < M) *reinterpret_cast<uint4 *>(table + i) = make_uint4(ex, ex + v.x, ex + v.x + v.y, ex + v.x + v.y + v.z);
        carry += all;
        __syncthreads();  // wtot is rewritten by the next step
    }
}

__global__ __launch_bounds__(256) void k_sort_scatter(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals, long n,
                                                      int shift, const uint32_t *__restrict__ table, int nblk,
                                                      uint32_t *__restrict__ keys_out, uint32_t *__restrict__ vals_out) {
    __shared__ uint32_t wcnt[4][256];  // per wave and digit: the running count, then where the wave's first such key goes
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int w = 0; w < 4; ++w) wcnt[w][threadIdx.x] = 0u;
    __syncthreads();
    const long base = (long)blockIdx.x * SORT_TILE + wid * (64 * ROUNDS) + lane;
    uint32_t key[ROUNDS], val[ROUNDS], off[ROUNDS];
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const long idx = base + r * 64;
        const bool valid = idx < n;
        key[r] = valid ? keys[idx] : 0u;
        val[r] = valid ? vals[idx] : 0u;
    }
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const bool valid = base + r * 64 < n;
        const uint32_t d = (key[r] >> shift) & 255u;
        const unsigned long long m = same_digit(d, valid);
        const uint32_t rank = lanes_below(m);
        off[r] = wcnt[wid][d] + rank;
        __syncthreads();  // every lane has read the count before the group's lowest lane moves it on
        if (valid && rank == 0u) wcnt[wid][d] += (uint32_t)__popcll(m);
        __syncthreads();
    }
    {
        const int d = threadIdx.x;
        const uint32_t c0 = wcnt[0][d], c1 = wcnt[1][d], c2 = wcnt[2][d];
        const uint32_t g = table[(size_t)d * nblk + blockIdx.x];
        wcnt[0][d] = g; wcnt[1][d] = g + c0; wcnt[2][d] = g + c0 + c1; wcnt[3][d] = g + c0 + c1 + c2;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const bool valid = base + r * 64 < n;
        const uint32_t d = (key[r] >> shift) & 255u;
        const uint32_t pos = wcnt[wid][d] + off[r];
        if (valid && (long)pos < n) {  // (pos < n by construction; the test keeps a wrong table from writing outside)
            keys_out[pos] = key[r];
            vals_out[pos] = val[r];
        }
    }
}

__global__ __launch_bounds__(256) void k_gather(const float *__restrict__ src, const float *__restrict__ col_src,
                                                const int32_t *__restrict__ perm, long n, float *__restrict__ dst,
                                                float *__restrict__ col_dst) {
    const long stride = (long)gridDim.x * 256;
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < n; j += stride) {
        const uint32_t i = (uint32_t)perm[j];
        if ((long)i >= n) continue;  // (a permutation of 0..n-1 by construction)
        const float *p = src + (size_t)i * 3;
        const float x = p[0], y = p[1], z = p[2];
        float *o = dst + (size_t)j * 3;
        o[0] = x; o[1] = y; o[2] = z;
        if (col_dst) col_dst[j] = col_src[i];
    }
}

int stride_grid(long n) { return (int)std::max<long>(1, std::min<long>((n + 255) / 256, 2048)); }

}  // namespace

hipError_t launch_sort_pairs(uint32_t *const keys[2], uint32_t *const vals[2], long n, uint32_t *table, int nblk,
                             uint32_t *vals_out, hipStream_t st) {
    for (int pass = 0; pass < 4; ++pass) {
        const int in = pass & 1, out = in ^ 1;
        const int shift = 8 * pass;
        hipLaunchKernelGGL(k_sort_hist, dim3(nblk), dim3(256), 0, st, keys[in], n, shift, table, nblk);
        hipLaunchKernelGGL(k_sort_scan, dim3(1), dim3(1024), 0, st, table, 256 * nblk);
        hipLaunchKernelGGL(k_sort_scatter, dim3(nblk), dim3(256), 0, st, keys[in], vals[in], n, shift, table, nblk, keys[out],
                           pass == 3 && vals_out ? vals_out : vals[out]);
    }
    return hipGetLastError();
}

hipError_t launch_points_order(const SortArgs &A, hipStream_t st) {
    hipLaunchKernelGGL(k_sort_keys, dim3(stride_grid(A.n)), dim3(256), 0, st, A);
    return launch_sort_pairs(A.keys, A.vals, A.n, A.table, A.nblk, reinterpret_cast<uint32_t *>(A.perm), st);
}

hipError_t launch_gather(const float *src, const float *col_src, const int32_t *perm, long n, float *dst, float *col_dst,
                         hipStream_t st) {
    hipLaunchKernelGGL(k_gather, dim3(stride_grid(n)), dim3(256), 0, st, src, col_src, perm, n, dst, col_dst);
    return hipGetLastError();
}

}  // namespace nr
