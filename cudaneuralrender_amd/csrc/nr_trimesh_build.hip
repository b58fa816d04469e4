// nr_trimesh_build.hip -- a nr_trimesh built on the device (nr_mesh_create_device): the pseudonormal
// table, the Morton order of the live triangles, the balanced tree over that order with its boxes and
// moments, and the area table, from vertices and triangles in device memory.  The contract of a
// device-built mesh is in include/neural_render.h; tests/trimesh_device_ref.py restates it in numpy.
//
// Every dependency between workgroups is a kernel boundary; no workgroup waits on another.  No atomic
// decides a position or the order of a sum: the atomics here are integer min / max / or / add of
// values whose result does not depend on the order (the bound, the flags, the live count, R2's
// maximum, the last rising threshold).  Every sum is sequential in one thread, in the order the
// contract names.  f64 throughout the table, the moments and the area table, one rounding per
// operation (-ffp-contract=off); the only square root is the correctly rounded f32 one.
//
//   k_tb_head      the read-back record's start values
//   k_tb_bound     the vertices' bound, largest |coordinate| and finiteness
//   k_tb_faces     per triangle: index check, f64 face normal, liveness, centroid, Morton key; the
//                  corner keys (vertex index, payload 3 t + corner)
//   (nr_sort.hip)  the stable sort of the triangle keys -> order; of the corner keys -> incidence lists
//   k_tb_vertex    per incidence list, by its first entry: the angle-weighted vertex sum
//   k_tb_edge      per triangle edge: the uses of the edge, found in the list of its smaller endpoint
//   k_tb_gather    d_tris and |A_p| by position
//   k_tb_leaves    per leaf: the exact box and the raw sums, sequential in position order
//   k_tb_level     per inner node of one level: left + right
//   k_tb_finish    per node: the centre, N, S, the grown box, the links
//   k_tb_r2        per position, down its path from the root: the largest squared corner distance
//   k_tb_r2_fin    R2 rounded up
//   k_tb_area_*    the running sums in blocks of 256, the blocks' exclusive sums, the thresholds
#include <algorithm>

#include "nr_trimesh_wave.h"

namespace nr {
namespace {

__device__ __forceinline__ uint32_t tb_encode(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}
__device__ __forceinline__ float tb_decode_dev(uint32_t e) { return __uint_as_float((e & 0x80000000u) ? e ^ 0x80000000u : ~e); }

// nr_sort.hip's Morton cell (header: "Order keys")
__device__ __forceinline__ uint32_t tb_spread10(uint32_t v) {
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    return (v | (v << 2)) & 0x09249249u;
}
__device__ __forceinline__ uint32_t tb_quantise(float x, float lo, float inv) {
    const float t = (x - lo) * inv;
    return t >= 1023.0f ? 1023u : (t > 0.0f ? (uint32_t)(int)t : 0u);
}

__device__ __forceinline__ D3 dcross(D3 u, D3 v) { return D3{u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x}; }
__device__ __forceinline__ D3 dvert(const float *V, int32_t i) {
    const float *p = V + (size_t)i * 3;
    return D3{(double)p[0], (double)p[1], (double)p[2]};
}
__device__ __forceinline__ bool dfinite(double x) { return __builtin_fabs(x) < __builtin_inf(); }

// wave-wide minimum / maximum of a 32-bit word
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, off));
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, off));
    return v;
}

int stride_grid(long n) { return (int)std::max<long>(1, std::min<long>((n + 255) / 256, 2048)); }
int flat_grid(long n) { return (int)std::max<long>(1, (n + 255) / 256); }

__global__ void k_tb_head(TriBuildHead *h) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        TriBuildHead z{};
        for (int a = 0; a < 3; ++a) { z.lo[a] = 0xffffffffu; z.hi[a] = 0u; }
        z.area_last = -1;
        *h = z;
    }
}

__global__ __launch_bounds__(256) void k_tb_bound(const float *__restrict__ V, long nv, TriBuildHead *h) {
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u}, ma = 0u, bad = 0u;
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += stride) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = V[(size_t)i * 3 + a];
            const uint32_t mag = __float_as_uint(v) & 0x7fffffffu;
            if (mag >= 0x7f800000u) { bad = 2u; continue; }
            const uint32_t e = tb_encode(v);
            lo[a] = min(lo[a], e);
            hi[a] = max(hi[a], e);
            ma = max(ma, mag);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = wave_min(lo[a]); hi[a] = wave_max(hi[a]); }
    ma = wave_max(ma);
    bad = wave_max(bad);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { atomicMin(&h->lo[a], lo[a]); atomicMax(&h->hi[a], hi[a]); }
        atomicMax(&h->maxabs, ma);
        if (bad) atomicOr(&h->err, bad);
    }
}

__global__ __launch_bounds__(256) void k_tb_faces(TriBuildArgs A) {
    float lo[3], inv[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = tb_decode_dev(A.head->lo[a]);
        inv[a] = 1023.0f / (tb_decode_dev(A.head->hi[a]) - lo[a]);
    }
    const long stride = (long)gridDim.x * 256;
    // (every lane runs the same number of rounds: the ballot below counts the wave's live triangles)
    for (long base = (long)blockIdx.x * 256; base < A.nt; base += stride) {
        const long t = base + threadIdx.x;
        bool live = false;
        if (t < A.nt) {
            const int32_t i0 = A.T[3 * t], i1 = A.T[3 * t + 1], i2 = A.T[3 * t + 2];
            const bool ok = i0 >= 0 && i1 >= 0 && i2 >= 0 && (long)i0 < A.nv && (long)i1 < A.nv && (long)i2 < A.nv;
            D3 f{0.0, 0.0, 0.0};
            uint32_t key = 1u << 30;
            if (!ok) {
                atomicOr(&A.head->err, 1u);
            } else {
                const float *pa = A.V + (size_t)i0 * 3, *pb = A.V + (size_t)i1 * 3, *pc = A.V + (size_t)i2 * 3;
                const D3 a{(double)pa[0], (double)pa[1], (double)pa[2]}, b{(double)pb[0], (double)pb[1], (double)pb[2]},
                    c{(double)pc[0], (double)pc[1], (double)pc[2]};
                const D3 n = dcross(dsub(b, a), dsub(c, a));
                live = (n.x != 0.0 || n.y != 0.0 || n.z != 0.0) && dfinite(n.x) && dfinite(n.y) && dfinite(n.z);
                if (live) {
                    const double s = fmax(fmax(__builtin_fabs(n.x), __builtin_fabs(n.y)), __builtin_fabs(n.z));
                    const D3 m{n.x / s, n.y / s, n.z / s};
                    const double l = dlen(m);
                    f = D3{m.x / l, m.y / l, m.z / l};
                    const float cx = ((pa[0] + pb[0]) + pc[0]) / 3.0f, cy = ((pa[1] + pb[1]) + pc[1]) / 3.0f,
                                cz = ((pa[2] + pb[2]) + pc[2]) / 3.0f;
                    key = tb_spread10(tb_quantise(cx, lo[0], inv[0])) | (tb_spread10(tb_quantise(cy, lo[1], inv[1])) << 1) |
                          (tb_spread10(tb_quantise(cz, lo[2], inv[2])) << 2);
                }
            }
            A.fn[3 * t] = f.x; A.fn[3 * t + 1] = f.y; A.fn[3 * t + 2] = f.z;
            float *o = A.table + (size_t)t * 21;
            o[0] = (float)f.x; o[1] = (float)f.y; o[2] = (float)f.z;
            A.tkeys[0][t] = key;
            A.tvals[0][t] = (uint32_t)t;
            A.ckeys[0][3 * t] = (uint32_t)i0; A.ckeys[0][3 * t + 1] = (uint32_t)i1; A.ckeys[0][3 * t + 2] = (uint32_t)i2;
            A.cvals[0][3 * t] = (uint32_t)(3 * t); A.cvals[0][3 * t + 1] = (uint32_t)(3 * t + 1); A.cvals[0][3 * t + 2] = (uint32_t)(3 * t + 2);
        }
        const unsigned long long m = __ballot(live);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(&A.head->ntl, (uint32_t)__popcll(m));
    }
}

// One thread per sorted corner.  The corners of a vertex are consecutive, in ascending (triangle,
// corner); the first of them sums the list and writes the sum to every member.  rank[3 t + c] = the
// corner's place, ghead[place] = the list's first place (k_tb_edge finds the list by them).
__global__ __launch_bounds__(256) void k_tb_vertex(TriBuildArgs A) {
    const long n3 = 3 * A.nt;
    const uint32_t *keys = A.ckeys[0], *vals = A.cvals[0];
    uint32_t *rank = A.ckeys[1], *ghead = A.cvals[1];
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n3) return;
    const uint32_t key = keys[i];
    rank[vals[i]] = (uint32_t)i;
    if (i > 0 && keys[i - 1] == key) return;
    const D3 o = dvert(A.V, (int32_t)key);
    D3 s{0.0, 0.0, 0.0};
    long end = i;
    for (long j = i; j < n3 && keys[j] == key; ++j) {
        end = j + 1;
        const uint32_t t = vals[j] / 3u, c = vals[j] % 3u;
        const D3 n{A.fn[3 * (size_t)t], A.fn[3 * (size_t)t + 1], A.fn[3 * (size_t)t + 2]};
        if (n.x != 0.0 || n.y != 0.0 || n.z != 0.0) {
            const D3 u = dsub(dvert(A.V, A.T[3 * (size_t)t + (c + 1u) % 3u]), o), v = dsub(dvert(A.V, A.T[3 * (size_t)t + (c + 2u) % 3u]), o);
            const double ang = half_angle(dlen(dcross(u, v)), ddot(u, v));
            s = D3{s.x + ang * n.x, s.y + ang * n.y, s.z + ang * n.z};
        }
    }
    for (long j = i; j < end; ++j) {
        const uint32_t t = vals[j] / 3u, c = vals[j] % 3u;
        float *w = A.table + ((size_t)t * 7 + 4 + c) * 3;
        w[0] = (float)s.x; w[1] = (float)s.y; w[2] = (float)s.z;
        ghead[j] = (uint32_t)i;
    }
}

// One thread per triangle edge (t, slot).  Every use of the undirected edge {lo, hi} shows in the
// incidence list of lo: at an entry (t', c') as slot c' when the next corner is hi (the edge leaves
// lo), and, for lo < hi, as slot c' + 2 when the previous corner is hi (the edge arrives at lo).
__global__ __launch_bounds__(256) void k_tb_edge(TriBuildArgs A) {
    const long n3 = 3 * A.nt;
    const uint32_t *keys = A.ckeys[0], *vals = A.cvals[0];
    const uint32_t *rank = A.ckeys[1], *ghead = A.cvals[1];
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n3) return;
    const uint32_t t = (uint32_t)(e / 3), s = (uint32_t)(e % 3);
    const uint32_t i = (uint32_t)A.T[3 * (size_t)t + s], j = (uint32_t)A.T[3 * (size_t)t + (s + 1u) % 3u];
    const uint32_t lo = i <= j ? i : j, hi = i <= j ? j : i;
    const uint32_t cl = i <= j ? s : (s + 1u) % 3u;
    D3 sum{0.0, 0.0, 0.0};
    int leave = 0, arrive = 0;
    for (long q = ghead[rank[3 * t + cl]]; q < n3 && keys[q] == lo; ++q) {
        const uint32_t t2 = vals[q] / 3u, c2 = vals[q] % 3u;
        const uint32_t next = (uint32_t)A.T[3 * (size_t)t2 + (c2 + 1u) % 3u], prev = (uint32_t)A.T[3 * (size_t)t2 + (c2 + 2u) % 3u];
        const int uses = (next == hi ? 1 : 0) + (prev == hi && lo < hi ? 1 : 0);
        leave += next == hi ? 1 : 0;
        arrive += prev == hi && lo < hi ? 1 : 0;
        const D3 n{A.fn[3 * (size_t)t2], A.fn[3 * (size_t)t2 + 1], A.fn[3 * (size_t)t2 + 2]};
        for (int k = 0; k < uses; ++k) sum = D3{sum.x + n.x, sum.y + n.y, sum.z + n.z};
    }
    float *w = A.table + ((size_t)t * 7 + 1 + s) * 3;
    w[0] = (float)sum.x; w[1] = (float)sum.y; w[2] = (float)sum.z;
    if (!(leave == 1 && arrive == 1)) atomicOr(&A.head->open, 1u);
}

// the contract's per-position values from the corners as stored in tris
struct TbTri {
    D3 A;         // 0.5 (b - a) x (c - a)
    double area;  // (double)sqrtf((float)((A.x A.x + A.y A.y) + A.z A.z))
    D3 x;         // ((a + b) + c) / 3.0
};
__device__ __forceinline__ TbTri tb_tri(const float *q) {
    const D3 a{(double)q[0], (double)q[1], (double)q[2]}, b{(double)q[4], (double)q[5], (double)q[6]}, c{(double)q[8], (double)q[9], (double)q[10]};
    const D3 n = dcross(dsub(b, a), dsub(c, a));
    TbTri r;
    r.A = D3{0.5 * n.x, 0.5 * n.y, 0.5 * n.z};
    r.area = dlen(r.A);
    r.x = D3{((a.x + b.x) + c.x) / 3.0, ((a.y + b.y) + c.y) / 3.0, ((a.z + b.z) + c.z) / 3.0};
    return r;
}

__global__ __launch_bounds__(256) void k_tb_gather(TriBuildArgs A) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= A.ntl) return;
    const uint32_t t = A.tvals[0][p];
    float q[12];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float *v = A.V + (size_t)A.T[3 * (size_t)t + c] * 3;
        q[4 * c] = v[0]; q[4 * c + 1] = v[1]; q[4 * c + 2] = v[2];
        q[4 * c + 3] = 0.0f;
    }
    q[3] = __uint_as_float(t);
    float4 *o = reinterpret_cast<float4 *>(A.tris + (size_t)p * 12);
    o[0] = make_float4(q[0], q[1], q[2], q[3]);
    o[1] = make_float4(q[4], q[5], q[6], q[7]);
    o[2] = make_float4(q[8], q[9], q[10], q[11]);
    A.area[p] = tb_tri(q).area;
}

__global__ __launch_bounds__(256) void k_tb_leaves(TriBuildArgs A) {
    const long li = (long)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.nleaves) return;
    const int node = A.list[li];
    const int first = A.first[node], count = A.count[node];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    double s[19];
#pragma unroll
    for (int k = 0; k < 19; ++k) s[k] = 0.0;
    for (int p = first; p < first + count; ++p) {
        const float *q = A.tris + (size_t)p * 12;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = fminf(lo[a], q[4 * c + a]);
                hi[a] = fmaxf(hi[a], q[4 * c + a]);
            }
        const TbTri r = tb_tri(q);
        const double x[3] = {r.x.x, r.x.y, r.x.z}, Av[3] = {r.A.x, r.A.y, r.A.z};
        s[0] += r.area;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            s[1 + a] += r.area * x[a];
            s[4 + a] += x[a];
            s[7 + a] += Av[a];
#pragma unroll
            for (int b = 0; b < 3; ++b) s[10 + 3 * a + b] += Av[a] * x[b];
        }
    }
    double *o = A.sums + (size_t)node * 19;
#pragma unroll
    for (int k = 0; k < 19; ++k) o[k] = s[k];
    float *bx = A.box + (size_t)node * 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) { bx[a] = lo[a]; bx[3 + a] = hi[a]; }
}

__global__ __launch_bounds__(256) void k_tb_level(TriBuildArgs A, int begin, int end) {
    const long k = (long)begin + (long)blockIdx.x * 256 + threadIdx.x;
    if (k >= end) return;
    const int node = A.list[k];
    const int l = A.w3[node], r = A.w7[node];
    const double *sl = A.sums + (size_t)l * 19, *sr = A.sums + (size_t)r * 19;
    double *o = A.sums + (size_t)node * 19;
#pragma unroll
    for (int q = 0; q < 19; ++q) o[q] = sl[q] + sr[q];
    const float *bl = A.box + (size_t)l * 6, *br = A.box + (size_t)r * 6;
    float *bx = A.box + (size_t)node * 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) { bx[a] = fminf(bl[a], br[a]); bx[3 + a] = fmaxf(bl[3 + a], br[3 + a]); }
}

// x - slack rounded down / x + slack rounded up to f32: to nearest, then one ulp outward, on the bits,
// where the result lies on the wrong side
__device__ __forceinline__ float tb_round_down(double x) {
    float f = (float)x;
    if ((double)f > x) {
        const uint32_t b = __float_as_uint(f);
        f = __uint_as_float((b & 0x7fffffffu) == 0u ? 0x80000001u : ((b & 0x80000000u) ? b + 1u : b - 1u));
    }
    return f;
}
__device__ __forceinline__ float tb_round_up(double x) {
    float f = (float)x;
    if ((double)f < x) {
        const uint32_t b = __float_as_uint(f);
        f = __uint_as_float((b & 0x7fffffffu) == 0u ? 0x00000001u : ((b & 0x80000000u) ? b - 1u : b + 1u));
    }
    return f;
}

__global__ __launch_bounds__(256) void k_tb_finish(TriBuildArgs A) {
    const long node = (long)blockIdx.x * 256 + threadIdx.x;
    if (node >= A.nnodes) return;
    const double *s = A.sums + (size_t)node * 19;
    const float *bx = A.box + (size_t)node * 6;
    float *nd = A.nodes + (size_t)node * 8, *rec = A.moments + (size_t)node * 16;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        nd[a] = tb_round_down((double)bx[a] - A.slack);
        nd[4 + a] = tb_round_up((double)bx[3 + a] + A.slack);
    }
    nd[3] = __int_as_float(A.w3[node]);
    nd[7] = __int_as_float(A.w7[node]);
    const double sa = s[0], cnt = (double)A.count[node];
    double c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        rec[a] = (float)(sa > 0.0 ? s[1 + a] / sa : s[4 + a] / cnt);
        c[a] = (double)rec[a];
        rec[4 + a] = (float)s[7 + a];
    }
    double M[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) M[a][b] = s[10 + 3 * a + b] - s[7 + a] * c[b];
    rec[3] = 0.0f;  // (k_tb_r2_fin)
    rec[7] = 0.0f;
    rec[8] = (float)M[0][0]; rec[9] = (float)M[1][1]; rec[10] = (float)M[2][2];
    rec[11] = (float)(0.5 * (M[0][1] + M[1][0]));
    rec[12] = (float)(0.5 * (M[0][2] + M[2][0]));
    rec[13] = (float)(0.5 * (M[1][2] + M[2][1]));
    rec[14] = 0.0f; rec[15] = 0.0f;
    A.r2[node] = 0ull;
}

// One thread per position, down the position's path from the root; A.depth rounds for every lane, so
// that the wave stays together: where all its live lanes stand at one node, one atomic for the wave.
__global__ __launch_bounds__(256) void k_tb_r2(TriBuildArgs A) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    bool act = p < A.ntl;
    D3 v[3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    if (act) {
        const float *q = A.tris + (size_t)p * 12;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = D3{(double)q[4 * c], (double)q[4 * c + 1], (double)q[4 * c + 2]};
    }
    int node = 0, first = 0, count = A.ntl;
    for (int level = 0; level < A.depth; ++level) {
        double r2 = 0.0;
        if (act) {
            const float *rec = A.moments + (size_t)node * 16;
            const D3 c{(double)rec[0], (double)rec[1], (double)rec[2]};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const D3 e = dsub(v[k], c);
                r2 = fmax(r2, ddot(e, e));
            }
        }
        const unsigned long long live = __ballot(act);
        if (live == 0ull) break;
        const int lead = __builtin_ctzll(live);
        const int n0 = __shfl(node, lead);
        const bool same = __all(!act || node == n0);
        unsigned long long bits = (unsigned long long)__double_as_longlong(r2);
        if (same) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const unsigned long long o = ((unsigned long long)(uint32_t)__shfl_xor((int)(bits >> 32), off) << 32) |
                                             (unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)bits, off);
                bits = bits > o ? bits : o;
            }
            if ((int)(threadIdx.x & 63) == lead) atomicMax(&A.r2[n0], bits);
        } else if (act) {
            atomicMax(&A.r2[node], bits);
        }
        if (act) {
            const int w7 = A.w7[node];
            if (w7 <= 0) {
                act = false;
            } else {
                const int half = (count + 1) / 2;
                if (p < (long)first + half) { node = A.w3[node]; count = half; }
                else { node = w7; first += half; count -= half; }
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_tb_r2_fin(TriBuildArgs A) {
    const long node = (long)blockIdx.x * 256 + threadIdx.x;
    if (node >= A.nnodes) return;
    A.moments[(size_t)node * 16 + 3] = tb_round_up(__longlong_as_double((long long)A.r2[node]));
}

// one thread per block of 256 positions: the running sum inside the block, in place, and its total
__global__ __launch_bounds__(64) void k_tb_area_block(TriBuildArgs A, int nblk) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= nblk) return;
    const long p0 = (long)b * 256, p1 = p0 + 256 < (long)A.ntl ? p0 + 256 : (long)A.ntl;
    double run = 0.0;
    for (long p = p0; p < p1; ++p) {
        run = run + A.area[p];
        A.area[p] = run;
    }
    A.base[b] = run;
}
// one thread: the blocks' exclusive sums, the total after them
__global__ void k_tb_area_base(TriBuildArgs A, int nblk) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double run = 0.0;
    for (int b = 0; b < nblk; ++b) {
        const double tot = A.base[b];
        A.base[b] = run;
        run = run + tot;
    }
    A.base[nblk] = run;
}
__device__ __forceinline__ uint32_t tb_threshold(double C, double sum) {
    const double f = __builtin_floor(C / sum * 4294967296.0);
    return f >= 4294967295.0 ? 0xffffffffu : (uint32_t)f;
}
__global__ __launch_bounds__(256) void k_tb_area_thresholds(TriBuildArgs A, int nblk) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= A.ntl) return;
    const double sum = A.base[nblk];
    if (!(sum > 0.0) || !dfinite(sum)) { A.thresholds[p] = 0u; return; }
    const uint32_t T = tb_threshold(A.base[p >> 8] + A.area[p], sum);
    const uint32_t prev = p > 0 ? tb_threshold(A.base[(p - 1) >> 8] + A.area[p - 1], sum) : 0u;
    A.thresholds[p] = T;
    if (T > prev) atomicMax(&A.head->area_last, (int32_t)p);
}

}  // namespace

hipError_t launch_tribuild_scan(const TriBuildArgs &A, hipStream_t st) {
    hipLaunchKernelGGL(k_tb_head, dim3(1), dim3(64), 0, st, A.head);
    hipLaunchKernelGGL(k_tb_bound, dim3(stride_grid(A.nv)), dim3(256), 0, st, A.V, A.nv, A.head);
    hipLaunchKernelGGL(k_tb_faces, dim3(stride_grid(A.nt)), dim3(256), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_tribuild_table(const TriBuildArgs &A, hipStream_t st) {
    const long n3 = 3 * A.nt;
    hipError_t e = launch_sort_pairs(A.tkeys, A.tvals, A.nt, A.ttable, (int)((A.nt + SORT_TILE - 1) / SORT_TILE), nullptr, st);
    if (e != hipSuccess) return e;
    e = launch_sort_pairs(A.ckeys, A.cvals, n3, A.ctable, (int)((n3 + SORT_TILE - 1) / SORT_TILE), nullptr, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_tb_vertex, dim3(flat_grid(n3)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_tb_edge, dim3(flat_grid(n3)), dim3(256), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_tribuild_tree(const TriBuildArgs &A, hipStream_t st) {
    hipLaunchKernelGGL(k_tb_gather, dim3(flat_grid(A.ntl)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_tb_leaves, dim3(flat_grid(A.nleaves)), dim3(256), 0, st, A);
    for (int l = 0; l < A.ninner_levels; ++l) {
        const int begin = A.nleaves + A.level_off[l], end = A.nleaves + A.level_off[l + 1];
        hipLaunchKernelGGL(k_tb_level, dim3(flat_grid(end - begin)), dim3(256), 0, st, A, begin, end);
    }
    hipLaunchKernelGGL(k_tb_finish, dim3(flat_grid(A.nnodes)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_tb_r2, dim3(flat_grid(A.ntl)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_tb_r2_fin, dim3(flat_grid(A.nnodes)), dim3(256), 0, st, A);
    const int nblk = (A.ntl + 255) / 256;
    hipLaunchKernelGGL(k_tb_area_block, dim3((nblk + 63) / 64), dim3(64), 0, st, A, nblk);
    hipLaunchKernelGGL(k_tb_area_base, dim3(1), dim3(64), 0, st, A, nblk);
    hipLaunchKernelGGL(k_tb_area_thresholds, dim3(flat_grid(A.ntl)), dim3(256), 0, st, A, nblk);
    return hipGetLastError();
}

}  // namespace nr
