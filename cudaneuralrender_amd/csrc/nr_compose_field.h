// nr_compose_field.h -- the composed field as device functions, shared by the tracer and the point
// sampler (nr_compose.hip), by the lattice, brick and vertex kernels (nr_compose_mesh.hip) and by the
// lighting tracer (nr_compose_light.hip), as nr_grad.h is shared by nr_grad.hip and nr_project.hip:
// one definition, the same bits everywhere.
#pragma once
#include "nr_mlp16.h"

namespace nr {

// the largest workgroup of the kernels that stage the packs: 12 waves, three per SIMD, which is also
// what bounds the registers
constexpr int NR_COMPOSE_MAX_THREADS = 768;

// what a wave adds to the statistics while it evaluates the field
struct FieldCount {
    uint32_t pairs;  // (live lane, part) pairs in bound
    uint32_t evals;  // network evaluations issued
    uint32_t skips;  // parts with no lane in bound
};

// The composed field at p (neural_render.h: q = R^T (p - pos) / scale per part, the network where
// qq <= 1.45, the bound's distance elsewhere, folded in part order), shared by the march, the normal
// passes and k_compose_sample.  live: the lane holds a point; the others feed the networks zeros and
// their result means nothing.  lds: the staged packs.
__device__ __forceinline__ float compose_field(const ComposeArgs &C, const float *lds, float fr, F3 p, bool live,
                                               int &owner, FieldCount &cnt) {
    float d = 0.0f;
    int own = 0;
    for (int j = 0; j < C.nparts; ++j) {
        const ComposePart &P = C.parts[j];
        const F3 v = mk3(p.x - P.pos[0], p.y - P.pos[1], p.z - P.pos[2]);
        const F3 q = mk3(((v.x * P.rot[0] + v.y * P.rot[3]) + v.z * P.rot[6]) * P.inv_s,
                         ((v.x * P.rot[1] + v.y * P.rot[4]) + v.z * P.rot[7]) * P.inv_s,
                         ((v.x * P.rot[2] + v.y * P.rot[5]) + v.z * P.rot[8]) * P.inv_s);
        const float qq = dot3(q, q);
        const bool inb = live && qq <= 1.45f;
        const uint64_t m = __ballot(inb);
        float sdf = 0.0f;
        if (m) {
            const ComposeNet &N = C.nets[P.net];
            // lanes out of bound feed a finite point and discard the result
            const F3 qi = inb ? q : mk3(0.0f, 0.0f, 0.0f);
            const bool cl = N.f32_clamp && inputs_in_bound_f32(qi.x, qi.y, qi.z, fr);
            sdf = mlp16_fp32(lds + N.off, N.in0, N.nh, fr, qi.x, qi.y, qi.z, tiles_of(m), cl);
            cnt.evals += 1;
            cnt.pairs += (uint32_t)__popcll(m);
        } else {
            cnt.skips += 1;
        }
        float dj;
        if (inb) dj = P.scale * nr_tanh(sdf);
        else dj = P.scale * (sqrtf(qq) - 1.19f);  // (a NaN qq lands here)
        if (j == 0) {
            d = dj;
        } else if (P.op == NR_PART_SUBTRACT) {
            const float nd = -dj;
            if (nd > d) { d = nd; own = j; }
        } else {
            if (dj < d) { d = dj; own = j; }
        }
    }
    owner = own;
    return d;
}

// One term of the tetrahedral gradient at sp, for a pass of 16 points x 4 samples (lane 4 k + q =
// sample q of point k): tp_q * field(sp + tp_q * epsilon).  The four lanes of a quad sum their terms
// (quad_bcast3_*) and normalise: the hit normal of k_compose and the vertex normal of k_compose_vertex.
__device__ __forceinline__ F3 compose_tet_term(const ComposeArgs &C, const float *lds, float fr, F3 sp, int q4, bool live,
                                               FieldCount &cnt) {
    // tetrahedron point q (c_tet): x = +1 for q = 0, 3; y = +1 for q = 2, 3; z = +1 for q = 1, 3
    int qo = q4;
    asm volatile("" : "+v"(qo));
    const F3 tp = mk3((qo == 0 || qo == 3) ? 1.0f : -1.0f, qo >= 2 ? 1.0f : -1.0f, (qo & 1) ? 1.0f : -1.0f);
    const F3 pq = add3(sp, mul3s(tp, NORMAL_EPSILON));
    int own;
    return mul3s(tp, compose_field(C, lds, fr, pq, live, own, cnt));
}

// intersect_bounding (nr_device.h) against the sphere (c, r): the same expressions on Q = o - c and r2 = r * r
__device__ __forceinline__ bool compose_intersect(F3 o, F3 d, const ComposeArgs &C, float &tnear, float &tfar) {
    const F3 Qv = mk3(o.x - C.center[0], o.y - C.center[1], o.z - C.center[2]);
    const float a = dot3(d, d);
    const float b = 2.0f * dot3(Qv, d);
    const float cc = dot3(Qv, Qv) - C.r2;
    const float disc = b * b - 4 * a * cc;
    if (!(disc > 0)) return false;
    const float sq = sqrtf(disc);
    const float a2 = 2.0f * a;
    tnear = (-b - sq) / a2;
    tfar = (-b + sq) / a2;
    return true;
}

// the packs into dynamic LDS, block-wide 16-byte copies
__device__ __forceinline__ const float *compose_stage(const ComposeArgs &C) {
    const int4 *src = reinterpret_cast<const int4 *>(C.packs);
    int4 *dst = reinterpret_cast<int4 *>(nr_smem16);
    for (int i = threadIdx.x; i < C.pack_bytes / 16; i += blockDim.x) dst[i] = src[i];
    __syncthreads();
    return reinterpret_cast<const float *>(nr_smem16);
}

}  // namespace nr
