// mfma_peak.hip -- sustained rate of back-to-back independent v_mfma_f32_16x16x4_f32 (the
// fp32 MLP's instruction) and v_mfma_f32_32x32x16_bf16, waves per SIMD 1..4, no VALU work:
// the practical ceiling the MLP kernels are measured against.  Prints TFLOP/s.
// Then the unit-skip section: v_mfma_f32_32x32x1_2b_f32 (K = 1, two 32-point blocks) with
// independent accumulators, as one dependent accumulate chain, with a wave-uniform "is this
// unit +0 in every live lane" test and branch between instances (8, 16 or 32 tests ahead of their
// branches), with its weight operand read from LDS (a wide read issued ahead, or a 4-byte read in
// front of the instruction), and with v_permlane32_swap
// beside it; every figure as median [min, max] of 7 timed launches, next to the 16x16x4
// stream timed the same way.  It also checks the instruction's D layout with exact integers.
// build: hipcc --offload-arch=gfx950 -O3 mfma_peak.hip -o bin/mfma_peak
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__global__ void k_f32(float *out, int iters, float a0, float b0) {
    f32x4 c[8];
    for (int i = 0; i < 8; ++i) c[i] = f32x4{0, 0, 0, 0};
    const float a = a0 + threadIdx.x * 1e-9f, b = b0;
    for (int it = 0; it < iters; ++it)
#pragma unroll
        for (int i = 0; i < 8; ++i) c[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c[i], 0, 0, 0);
    float s = 0;
    for (int i = 0; i < 8; ++i) s += c[i][0] + c[i][3];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

// the same f32 MFMA stream with NV independent v_add_f32 after every MFMA (the VALU work an
// MLP epilogue or a marching phase adds to the issue port)
template <int NV>
__global__ void k_f32_valu(float *out, int iters, float a0, float b0) {
    f32x4 c[8];
    for (int i = 0; i < 8; ++i) c[i] = f32x4{0, 0, 0, 0};
    const float a = a0 + threadIdx.x * 1e-9f, b = b0;
    float v[8];
    for (int i = 0; i < 8; ++i) v[i] = a * (float)(i + 1);
    for (int it = 0; it < iters; ++it)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            c[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c[i], 0, 0, 0);
#pragma unroll
            for (int q = 0; q < NV; ++q) asm volatile("v_add_f32 %0, %0, %1" : "+v"(v[(i + q) & 7]) : "v"(b));
        }
    float s = 0;
    for (int i = 0; i < 8; ++i) s += c[i][0] + c[i][3] + v[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

__global__ void k_bf16(float *out, int iters, float a0, float b0) {
    f32x16 c[4];
    for (int i = 0; i < 4; ++i) c[i] = f32x16{};
    bf16x8 a, b;
    for (int i = 0; i < 8; ++i) { a[i] = (__bf16)(a0 + threadIdx.x * 1e-3f); b[i] = (__bf16)b0; }
    for (int it = 0; it < iters; ++it)
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c[i], 0, 0, 0);
    float s = 0;
    for (int i = 0; i < 4; ++i) s += c[i][0] + c[i][15];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

typedef float f32x32 __attribute__((ext_vector_type(32)));

// v_mfma_f32_32x32x1_2b_f32, NACC independent accumulators (NACC = 1: one dependent chain)
template <int NACC>
__global__ void k_u(float *out, int iters, float a0, float b0) {
    f32x32 c[NACC];
    for (int i = 0; i < NACC; ++i) c[i] = f32x32{};
    const float a = a0 + threadIdx.x * 1e-9f, b = b0;
    for (int it = 0; it < iters; ++it)
#pragma unroll
        for (int i = 0; i < 8; ++i) c[i % NACC] = __builtin_amdgcn_mfma_f32_32x32x1f32(a, b, c[i % NACC], 0, 0, 0);
    float s = 0;
    for (int i = 0; i < NACC; ++i) s += c[i][0] + c[i][31];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

// one dependent chain over 8 "units" per iteration: unit k is issued only if its activation
// av[k] has a nonzero bit pattern in some live lane.  The empty asm keeps the compiler from
// hoisting the loop-invariant test out of the loop.  MODE 0: compare, scalar and, scalar branch
// in front of each instance; 1: the eight compares and ands first (as after a layer's
// epilogue), then a scalar test and branch per instance; 2: compare and and per instance, no
// branch (every unit issued): the cost of the test without the branch
template <int MODE>
__global__ void k_u_skip(float *out, int iters, float b0, const float *av, unsigned long long live) {
    f32x32 c = f32x32{};
    const int lane = threadIdx.x & 63;
    unsigned a[8];
    for (int k = 0; k < 8; ++k) a[k] = __float_as_uint(av[k * 64 + lane]);
    float w = b0 + lane * 1e-9f;
    asm volatile("" : "+v"(w));
    unsigned long long any = 0;
    for (int it = 0; it < iters; ++it) {
        if constexpr (MODE == 1) {
            unsigned long long m[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                asm volatile("" : "+v"(a[k]));
                m[k] = __builtin_amdgcn_ballot_w64(a[k] != 0u) & live;
                asm volatile("" : "+s"(m[k]));
            }
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (m[k]) c = __builtin_amdgcn_mfma_f32_32x32x1f32(w, __uint_as_float(a[k]), c, 0, 0, 0);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                asm volatile("" : "+v"(a[k]));
                const unsigned long long m = __builtin_amdgcn_ballot_w64(a[k] != 0u) & live;
                if constexpr (MODE == 2) {
                    any |= m;
                    c = __builtin_amdgcn_mfma_f32_32x32x1f32(w, __uint_as_float(a[k]), c, 0, 0, 0);
                } else if (m) {
                    c = __builtin_amdgcn_mfma_f32_32x32x1f32(w, __uint_as_float(a[k]), c, 0, 0, 0);
                }
            }
        }
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = c[0] + c[31] + (float)(unsigned)(any >> 40);
}

// NT tests (8, 16 or 32: the units of one, two or four iterations of k_u_skip<1>) ahead of their
// branches: what forming all of a layer's masks before its first branch costs in scalar registers
template <int NT>
__global__ void k_u_tests(float *out, int iters, float b0, const float *av, unsigned long long live) {
    f32x32 c = f32x32{};
    const int lane = threadIdx.x & 63;
    unsigned a[8];
    for (int k = 0; k < 8; ++k) a[k] = __float_as_uint(av[k * 64 + lane]);
    float w = b0 + lane * 1e-9f;
    asm volatile("" : "+v"(w));
    for (int it = 0; it < iters; it += NT / 8) {
        unsigned long long m[NT];
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            asm volatile("" : "+v"(a[k & 7]));
            m[k] = __builtin_amdgcn_ballot_w64(a[k & 7] != 0u) & live;
            asm volatile("" : "+s"(m[k]));
        }
#pragma unroll
        for (int k = 0; k < NT; ++k)
            if (m[k]) c = __builtin_amdgcn_mfma_f32_32x32x1f32(w, __uint_as_float(a[k & 7]), c, 0, 0, 0);
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = c[0] + c[31];
}

// one dependent chain of 8 units per iteration whose weight operand comes from LDS, [k >> 2][row 32][k & 3]
// as the unit pack holds it.  MODE 0: one ds_read_b128 per four units, issued (inline asm) while
// the four before run and waited for by hand, as the kernel does; 1: a 4-byte read directly in
// front of each instance
template <int MODE>
__global__ void k_u_lds(float *out, int iters, float b0) {
    __shared__ f32x4 wl[2][32];
    const int lane = threadIdx.x & 63, row = lane & 31;
    if (threadIdx.x < 64) wl[threadIdx.x >> 5][row] = f32x4{1.0f, 1.0f, 1.0f, 1.0f} * (1.0f + threadIdx.x * 1e-9f);
    __syncthreads();
    unsigned addr = (unsigned)(size_t)(const __attribute__((address_space(3))) f32x4 *)&wl[0][row];
    asm volatile("" : "+v"(addr));
    f32x32 c = f32x32{};
    float b = b0;
    asm volatile("" : "+v"(b));
    if constexpr (MODE == 0) {
        f32x4 w, n;
        asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(w) : "v"(addr));
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (q == 0) asm volatile("ds_read_b128 %0, %1 offset:512" : "=&v"(n) : "v"(addr));
                else asm volatile("ds_read_b128 %0, %1" : "=&v"(n) : "v"(addr));
#pragma unroll
                for (int i = 0; i < 4; ++i) c = __builtin_amdgcn_mfma_f32_32x32x1f32(w[i], b, c, 0, 0, 0);
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(n));
                w = n;
            }
        }
    } else {
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                float w;
                if (k < 4) asm volatile("ds_read_b32 %0, %1 offset:%2\n\ts_waitcnt lgkmcnt(0)" : "=&v"(w) : "v"(addr), "n"(4 * (k & 3)));
                else asm volatile("ds_read_b32 %0, %1 offset:%2\n\ts_waitcnt lgkmcnt(0)" : "=&v"(w) : "v"(addr), "n"(512 + 4 * (k & 3)));
                c = __builtin_amdgcn_mfma_f32_32x32x1f32(w, b, c, 0, 0, 0);
            }
        }
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = c[0] + c[31];
}

// one dependent chain with NS v_permlane32_swap (independent registers) after every instance
template <int NS>
__global__ void k_u_swap(float *out, int iters, float a0, float b0) {
    f32x32 c = f32x32{};
    const float a = a0 + threadIdx.x * 1e-9f, b = b0;
    unsigned v[8];
    for (int i = 0; i < 8; ++i) v[i] = threadIdx.x * 8u + i;
    for (int it = 0; it < iters; ++it)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            c = __builtin_amdgcn_mfma_f32_32x32x1f32(a, b, c, 0, 0, 0);
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                const int x = (2 * (i + q)) & 7;
                auto r = __builtin_amdgcn_permlane32_swap(v[x], v[x + 1], false, false);
                v[x] = r[0];
                v[x + 1] = r[1];
            }
        }
    unsigned s = 0;
    for (int i = 0; i < 8; ++i) s += v[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = c[0] + c[31] + (float)s;
}

// D layout: A = 1 + row + 100 * block in lane 32 * block + row, B = 1 + 3 * column + 1000 * block
// in lane 32 * block + column (asymmetric, exact in f32); every lane dumps its 32 registers
__global__ void k_u_layout(float *out) {
    const int lane = threadIdx.x & 63;
    const float a = 1.0f + (lane & 31) + 100.0f * (lane >> 5);
    const float b = 1.0f + 3.0f * (lane & 31) + 1000.0f * (lane >> 5);
    f32x32 c = __builtin_amdgcn_mfma_f32_32x32x1f32(a, b, f32x32{}, 0, 0, 0);
    for (int r = 0; r < 32; ++r) out[lane * 32 + r] = c[r];
}

template <class F>
static bool timed(const char *name, int wps, double flop, double peak, F launch) {
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) || hipEventCreate(&e1)) return false;
    launch();
    if (hipDeviceSynchronize()) return false;
    std::vector<double> tf;
    for (int r = 0; r < 7; ++r) {
        if (hipEventRecord(e0, 0)) return false;
        launch();
        if (hipEventRecord(e1, 0) || hipEventSynchronize(e1)) return false;
        float ms = 0;
        if (hipEventElapsedTime(&ms, e0, e1)) return false;
        tf.push_back(flop / (ms * 1e-3) / 1e12);
    }
    std::sort(tf.begin(), tf.end());
    printf("%-58s waves/SIMD %d: %6.1f TF/s [%6.1f, %6.1f]  (%.3f of %.1f)\n", name, wps, tf[3], tf[0], tf[6], tf[3] / peak, peak);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return true;
}

static int unit_skip_section(int cus, float *out) {
    printf("# unit skip: v_mfma_f32_32x32x1_2b_f32, median [min, max] of 7 launches; a skipped unit counts as issued FLOP\n");
    // D layout first: block b = reg / 16, column = lane % 32, row = (reg % 4) + 8 * ((reg % 16) / 4) + 4 * (lane / 32)
    {
        std::vector<float> h(64 * 32);
        hipLaunchKernelGGL(k_u_layout, dim3(1), dim3(64), 0, 0, out);
        if (hipMemcpy(h.data(), out, h.size() * 4, hipMemcpyDeviceToHost)) return 1;
        int bad = 0;
        for (int lane = 0; lane < 64; ++lane)
            for (int r = 0; r < 32; ++r) {
                const int blk = r / 16, col = lane % 32, row = (r % 4) + 8 * ((r % 16) / 4) + 4 * (lane / 32);
                const float want = (1.0f + row + 100.0f * blk) * (1.0f + 3.0f * col + 1000.0f * blk);
                bad += h[lane * 32 + r] != want;
            }
        printf("D layout (block = reg / 16, column = lane %% 32, row = reg %% 4 + 8 * (reg %% 16 / 4) + 4 * (lane / 32)): %d of 2048 wrong\n", bad);
    }
    float *av;
    if (hipMalloc(&av, 3 * 8 * 64 * 4)) return 1;
    {
        // pattern 0: every unit nonzero in every lane; 1: units 1, 4, 6 are +0 in all lanes;
        // 2: the same three units nonzero in lane 63 only, which the live mask leaves out
        std::vector<float> h(3 * 8 * 64);
        for (int p = 0; p < 3; ++p)
            for (int k = 0; k < 8; ++k)
                for (int l = 0; l < 64; ++l) {
                    const bool dead = k == 1 || k == 4 || k == 6;
                    h[(p * 8 + k) * 64 + l] = p == 0 || !dead ? 1e-3f : (p == 2 && l == 63 ? 1e-3f : 0.0f);
                }
        if (hipMemcpy(av, h.data(), h.size() * 4, hipMemcpyHostToDevice)) return 1;
    }
    const int iters = 2048;
    for (int wps = 1; wps <= 4; wps += 3) {
        const int grid = cus * wps;
        const double f16 = (double)grid * 4 * iters * 2 * 8.0 * 2 * 16 * 16 * 4, fu = (double)grid * 4 * iters * 8.0 * 2 * 32 * 32 * 2;
        bool ok = true;
        ok &= timed("16x16x4 f32, 8 independent accumulators", wps, f16, 157.3,
                    [&] { hipLaunchKernelGGL(k_f32, dim3(grid), dim3(256), 0, 0, out, 2 * iters, 1.0f, 1e-3f); });
        ok &= timed("32x32x1_2b f32, 2 independent accumulators", wps, fu, 157.3,
                    [&] { hipLaunchKernelGGL(k_u<2>, dim3(grid), dim3(256), 0, 0, out, iters, 1.0f, 1e-3f); });
        ok &= timed("32x32x1_2b f32, one dependent chain", wps, fu, 157.3,
                    [&] { hipLaunchKernelGGL(k_u<1>, dim3(grid), dim3(256), 0, 0, out, iters, 1.0f, 1e-3f); });
        ok &= timed("chain + test and branch per unit, 8 of 8 issued", wps, fu, 157.3,
                    [&] { hipLaunchKernelGGL(k_u_skip<0>, dim3(grid), dim3(256), 0, 0, out, iters, 1e-3f, av, ~0ull); });
        ok &= timed("chain + test and branch per unit, 5 of 8 issued", wps, fu, 157.3,
                    [&] { hipLaunchKernelGGL(k_u_skip<0>, dim3(grid), dim3(256), 0, 0, out, iters, 1e-3f, av + 512, ~0ull); });
        ok &= timed("chain + test and branch, 5 of 8, stale lane 63 masked off", wps, fu, 157.3,
                    [&] { hipLaunchKernelGGL(k_u_skip<0>, dim3(grid), dim3(256), 0, 0, out, iters, 1e-3f, av + 1024, ~0ull >> 1); });
        ok &= timed("chain, 8 tests first, then branch per unit, 8 of 8 issued", wps, fu, 157.3,
                    [&] { hipLaunchKernelGGL(k_u_skip<1>, dim3(grid), dim3(256), 0, 0, out, iters, 1e-3f, av, ~0ull); });
        ok &= timed("chain, 8 tests first, then branch per unit, 5 of 8 issued", wps, fu, 157.3,
                    [&] { hipLaunchKernelGGL(k_u_skip<1>, dim3(grid), dim3(256), 0, 0, out, iters, 1e-3f, av + 512, ~0ull); });
        ok &= timed("chain + test per unit, no branch, 8 of 8 issued", wps, fu, 157.3,
                    [&] { hipLaunchKernelGGL(k_u_skip<2>, dim3(grid), dim3(256), 0, 0, out, iters, 1e-3f, av, ~0ull); });
        ok &= timed("chain, 16 tests first, then branch per unit, 5 of 8 issued", wps, fu, 157.3,
                    [&] { hipLaunchKernelGGL(k_u_tests<16>, dim3(grid), dim3(256), 0, 0, out, iters, 1e-3f, av + 512, ~0ull); });
        ok &= timed("chain, 32 tests first, then branch per unit, 5 of 8 issued", wps, fu, 157.3,
                    [&] { hipLaunchKernelGGL(k_u_tests<32>, dim3(grid), dim3(256), 0, 0, out, iters, 1e-3f, av + 512, ~0ull); });
        ok &= timed("chain, weights by ds_read_b128 four units ahead", wps, fu, 157.3,
                    [&] { hipLaunchKernelGGL(k_u_lds<0>, dim3(grid), dim3(256), 0, 0, out, iters, 1e-3f); });
        ok &= timed("chain, weight by ds_read_b32 in front of each instance", wps, fu, 157.3,
                    [&] { hipLaunchKernelGGL(k_u_lds<1>, dim3(grid), dim3(256), 0, 0, out, iters, 1e-3f); });
        ok &= timed("chain + 1 v_permlane32_swap per instance", wps, fu, 157.3,
                    [&] { hipLaunchKernelGGL(k_u_swap<1>, dim3(grid), dim3(256), 0, 0, out, iters, 1.0f, 1e-3f); });
        ok &= timed("chain + 2 v_permlane32_swap per instance", wps, fu, 157.3,
                    [&] { hipLaunchKernelGGL(k_u_swap<2>, dim3(grid), dim3(256), 0, 0, out, iters, 1.0f, 1e-3f); });
        if (!ok) return 1;
    }
    (void)hipFree(av);
    return 0;
}

int main() {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0)) return 1;
    const int cus = prop.multiProcessorCount;
    float *out;
    if (hipMalloc(&out, (size_t)cus * 16 * 256 * 4)) return 1;
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) || hipEventCreate(&e1)) return 1;
    for (int kind = 0; kind < 2; ++kind)
        for (int wps = 1; wps <= 4; ++wps) {
            const int iters = kind == 0 ? 4096 : 8192;
            const int grid = cus * wps;  // 256 threads = 4 waves = one per SIMD, wps blocks per CU
            auto launch = [&]() {
                if (kind == 0) hipLaunchKernelGGL(k_f32, dim3(grid), dim3(256), 0, 0, out, iters, 1.0f, 1e-3f);
                else hipLaunchKernelGGL(k_bf16, dim3(grid), dim3(256), 0, 0, out, iters, 1.0f, 1e-3f);
            };
            launch();
            if (hipDeviceSynchronize()) return 1;
            if (hipEventRecord(e0, 0)) return 1;
            for (int r = 0; r < 5; ++r) launch();
            if (hipEventRecord(e1, 0) || hipEventSynchronize(e1)) return 1;
            float ms = 0;
            if (hipEventElapsedTime(&ms, e0, e1)) return 1;
            ms /= 5;
            const double flop = (double)grid * 4 * iters * (kind == 0 ? 8.0 * 2 * 16 * 16 * 4 : 4.0 * 2 * 32 * 32 * 16);
            const double tf = flop / (ms * 1e-3) / 1e12;
            printf("%s  waves/SIMD %d: %.3f ms  %.1f TF/s  (%.3f of %s)\n", kind == 0 ? "16x16x4 f32  " : "32x32x16 bf16", wps,
                   ms, tf, tf / (kind == 0 ? 157.3 : 2516.6), kind == 0 ? "157.3" : "2516.6");
        }
    for (int nv = 1; nv <= 6; ++nv)
        for (int wps = 1; wps <= 3; wps += 2) {
            const int iters = 4096, grid = cus * wps;
            auto launch = [&]() {
                switch (nv) {
                    case 1: hipLaunchKernelGGL(k_f32_valu<1>, dim3(grid), dim3(256), 0, 0, out, iters, 1.0f, 1e-3f); break;
                    case 2: hipLaunchKernelGGL(k_f32_valu<2>, dim3(grid), dim3(256), 0, 0, out, iters, 1.0f, 1e-3f); break;
                    case 3: hipLaunchKernelGGL(k_f32_valu<3>, dim3(grid), dim3(256), 0, 0, out, iters, 1.0f, 1e-3f); break;
                    case 4: hipLaunchKernelGGL(k_f32_valu<4>, dim3(grid), dim3(256), 0, 0, out, iters, 1.0f, 1e-3f); break;
                    case 5: hipLaunchKernelGGL(k_f32_valu<5>, dim3(grid), dim3(256), 0, 0, out, iters, 1.0f, 1e-3f); break;
                    default: hipLaunchKernelGGL(k_f32_valu<6>, dim3(grid), dim3(256), 0, 0, out, iters, 1.0f, 1e-3f); break;
                }
            };
            launch();
            if (hipDeviceSynchronize()) return 1;
            if (hipEventRecord(e0, 0)) return 1;
            for (int r = 0; r < 5; ++r) launch();
            if (hipEventRecord(e1, 0) || hipEventSynchronize(e1)) return 1;
            float ms = 0;
            if (hipEventElapsedTime(&ms, e0, e1)) return 1;
            ms /= 5;
            const double tf = (double)grid * 4 * iters * 8.0 * 2 * 16 * 16 * 4 / (ms * 1e-3) / 1e12;
            printf("16x16x4 f32 + %d v_add_f32 per MFMA, waves/SIMD %d: %.1f TF/s (%.3f of 157.3)\n", nv, wps, tf, tf / 157.3);
        }
    return unit_skip_section(cus, out);
}
