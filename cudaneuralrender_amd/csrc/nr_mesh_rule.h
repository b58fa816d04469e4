// nr_mesh_rule.h -- the marching-tetrahedra rule of nr_mesh_grid (include/neural_render.h) as a
// compile-time table: the Kuhn split of a lattice cell, the lattice edge under every tetrahedron
// edge and, per tetrahedron and inside mask, its triangles with the winding decided on the
// topology; and what one lattice point contributes to the mesh, as functions the kernels call per
// thread.  Plain C++: it compiles for the host alone too.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

namespace nr {

// Corner c of a cell: bit 0 = +x, bit 1 = +y, bit 2 = +z.  The 7 edge kinds run from a lattice
// point o to o + e; slot order 100, 010, 001, 110, 101, 011, 111 (x first), as corner bits:
constexpr int MESH_SLOT_BITS[7] = {1, 2, 4, 3, 5, 6, 7};
constexpr int MESH_SLOT_OF[8] = {-1, 0, 1, 3, 2, 4, 5, 6};  // slot of the edge vector with these corner bits

struct MeshRule {
    // corner[t][m]: the cell corner of path vertex m of tetrahedron t; t counts the axis
    // permutations (a, b, c) in lexicographic order, v0 = 000, v1 = v0 + e_a, v2 = v1 + e_b, v3 = 111
    uint8_t corner[6][4];
    // tri[t][mask][q]: triangle q of tetrahedron t whose path vertex m is inside iff bit m of mask:
    // three 6-bit vertex codes (base corner << 3 | slot, the lattice edge base -> base + e), code r
    // in bits 6 r .. 6 r + 5.  popcount(mask) = 1 or 3: one triangle, 2: two, 0 or 4: none.
    uint32_t tri[6][16][2];
};

constexpr MeshRule make_mesh_rule() {
    MeshRule R{};
    const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    for (int t = 0; t < 6; ++t) {
        int cor[4] = {0, 0, 0, 7};
        cor[1] = 1 << perms[t][0];
        cor[2] = cor[1] | (1 << perms[t][1]);
        for (int m = 0; m < 4; ++m) R.corner[t][m] = (uint8_t)cor[m];
        for (int mask = 1; mask < 15; ++mask) {
            int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, nin = 0, nout = 0;
            for (int m = 0; m < 4; ++m) {
                if ((mask >> m) & 1) in[nin++] = m;
                else out[nout++] = m;
            }
            // the triangles as pairs of path vertices (tetrahedron edges)
            int e[2][3][2] = {};
            int ntri = 1;
            if (nin == 1) {
                for (int r = 0; r < 3; ++r) { e[0][r][0] = in[0]; e[0][r][1] = out[r]; }
            } else if (nout == 1) {
                for (int r = 0; r < 3; ++r) { e[0][r][0] = out[0]; e[0][r][1] = in[r]; }
            } else {
                const int A = in[0], B = in[1], C = out[0], D = out[1];
                ntri = 2;
                e[0][0][0] = A; e[0][0][1] = C; e[0][1][0] = A; e[0][1][1] = D; e[0][2][0] = B; e[0][2][1] = D;
                e[1][0][0] = A; e[1][0][1] = C; e[1][1][0] = B; e[1][1][1] = D; e[1][2][0] = B; e[1][2][1] = C;
            }
            // inside -> outside direction, scaled by nin * nout: sum(out) nin - sum(in) nout
            int dir[3] = {0, 0, 0};
            for (int ax = 0; ax < 3; ++ax) {
                int si = 0, so = 0;
                for (int m = 0; m < nin; ++m) si += (cor[in[m]] >> ax) & 1;
                for (int m = 0; m < nout; ++m) so += (cor[out[m]] >> ax) & 1;
                dir[ax] = so * nin - si * nout;
            }
            for (int q = 0; q < ntri; ++q) {
                // edge midpoints, doubled: the sum of the two corners
                int P[3][3] = {};
                for (int r = 0; r < 3; ++r)
                    for (int ax = 0; ax < 3; ++ax) P[r][ax] = ((cor[e[q][r][0]] >> ax) & 1) + ((cor[e[q][r][1]] >> ax) & 1);
                const int u[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]};
                const int v[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
                const int nrm[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
                const int dot = nrm[0] * dir[0] + nrm[1] * dir[1] + nrm[2] * dir[2];
                const int order[3] = {0, dot > 0 ? 1 : 2, dot > 0 ? 2 : 1};
                uint32_t code = 0;
                for (int r = 0; r < 3; ++r) {
                    const int m0 = e[q][order[r]][0], m1 = e[q][order[r]][1];
                    const int lo = m0 < m1 ? m0 : m1, hi = m0 < m1 ? m1 : m0;
                    const int slot = MESH_SLOT_OF[cor[hi] ^ cor[lo]];
                    code |= (uint32_t)((cor[lo] << 3) | slot) << (6 * r);
                }
                R.tri[t][mask][q] = code;
            }
        }
    }
    return R;
}

#if defined(__HIPCC__)
#define NR_MESH_HD __host__ __device__ __forceinline__
#else
#define NR_MESH_HD inline
#endif

// What lattice point p = (i, j, k) contributes: the vertices on the 7 edges that start at it and
// the triangles of the cell whose corner 000 it is.
struct MeshPoint {
    float s[8];        // the values at the cell's corners (0 for a corner outside the lattice)
    uint32_t valid;    // bit c: corner c lies in the lattice (bit 7: p has a cell)
    uint32_t inside;   // bit c: corner c is valid and s < iso (NaN and s == iso are outside)
    uint32_t vmask;    // bit slot: the edge p -> p + e_slot lies in the lattice and crosses iso
    uint32_t ntri;     // triangles of the cell
};

NR_MESH_HD uint32_t mesh_corner_offset(int c, uint32_t nx, uint32_t nxy) {
    return (uint32_t)(c & 1) + ((c & 2) ? nx : 0u) + ((c & 4) ? nxy : 0u);
}

// bit m: path vertex m of tetrahedron t is inside
NR_MESH_HD uint32_t mesh_tet_mask(const MeshRule &R, uint32_t inside, int t) {
    uint32_t m = 0;
    for (int v = 0; v < 4; ++v) m |= ((inside >> R.corner[t][v]) & 1u) << v;
    return m;
}

// vmask and ntri of a point whose s, valid and inside are set
NR_MESH_HD void mesh_point_masks(const MeshRule &R, MeshPoint &P) {
    P.vmask = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int slot = 0; slot < 7; ++slot) {
        const int b = MESH_SLOT_BITS[slot];
        P.vmask |= ((P.valid >> b) & ((P.inside >> b) ^ P.inside) & 1u) << slot;
    }
    P.ntri = 0;
    if ((P.valid >> 7) & 1u)
        for (int t = 0; t < 6; ++t) {
            const int pc = __builtin_popcount(mesh_tet_mask(R, P.inside, t));
            P.ntri += pc == 2 ? 2u : (pc == 1 || pc == 3) ? 1u : 0u;
        }
}

NR_MESH_HD MeshPoint mesh_point(const MeshRule &R, const float *sdf, uint32_t p, int i, int j, int k, int nx, int ny,
                                int nz, float iso) {
    MeshPoint P;
    const bool vx = i + 1 < nx, vy = j + 1 < ny, vz = k + 1 < nz;
    const uint32_t nxy = (uint32_t)nx * (uint32_t)ny;
    P.valid = 0;
    P.inside = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int c = 0; c < 8; ++c) {
        const bool ok = (!(c & 1) || vx) && (!(c & 2) || vy) && (!(c & 4) || vz);
        const float s = ok ? sdf[p + mesh_corner_offset(c, (uint32_t)nx, nxy)] : 0.0f;
        P.s[c] = s;
        P.valid |= (uint32_t)ok << c;
        P.inside |= (uint32_t)(ok && s < iso) << c;
    }
    mesh_point_masks(R, P);
    return P;
}

// The vertex on the edge a -> b: t = (iso - s_a) / (s_b - s_a), pos = p_a + (p_b - p_a) t per
// component, one f32 rounding per operation.  A NaN coordinate is written as the positive quiet NaN.
NR_MESH_HD float mesh_lerp(float pa, float pb, float t) {
    const float v = pa + (pb - pa) * t;
    return v != v ? __builtin_nanf("") : v;
}

// The id of the vertex on slot `slot` of lattice point q: the vertices before q's block, before q in
// its block and on q's lower slots
NR_MESH_HD int32_t mesh_vertex_id(const uint32_t *word, const unsigned long long *offv, uint32_t q, int slot) {
    const uint32_t w = word[q];
    return (int32_t)((uint32_t)offv[q >> 8] + ((w >> 7) & 0x7ffu) + (uint32_t)__builtin_popcount(w & ((1u << slot) - 1u)));
}

// Writes point p's vertices (from id v0) and its cell's triangles (from index t0).
NR_MESH_HD void mesh_emit_point(const MeshRule &R, const MeshPoint &P, const float *origin, const float *step, uint32_t p,
                                int i, int j, int k, uint32_t nx, uint32_t nxy, float iso, const uint32_t *word,
                                const unsigned long long *offv, unsigned long long v0, unsigned long long t0,
                                float *vertices, int32_t *triangles) {
    if (P.vmask) {
        const int idx[3] = {i, j, k};
        const float sa = P.s[0];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int slot = 0; slot < 7; ++slot) {
            if (!((P.vmask >> slot) & 1u)) continue;
            const int b = MESH_SLOT_BITS[slot];
            const float t = (iso - sa) / (P.s[b] - sa);
            float *o = vertices + v0 * 3;
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int a = 0; a < 3; ++a) {
                const float pa = origin[a] + (float)idx[a] * step[a];
                const float pb = origin[a] + (float)(idx[a] + ((b >> a) & 1)) * step[a];
                o[a] = mesh_lerp(pa, pb, t);
            }
            ++v0;
        }
    }
    if (!P.ntri) return;
    for (int t = 0; t < 6; ++t) {
        const uint32_t m = mesh_tet_mask(R, P.inside, t);
        const int pc = __builtin_popcount(m);
        const int ntri = pc == 2 ? 2 : (pc == 1 || pc == 3) ? 1 : 0;
        for (int q = 0; q < ntri; ++q) {
            const uint32_t code = R.tri[t][m][q];
            int32_t *o = triangles + t0 * 3;
            for (int r = 0; r < 3; ++r) {
                const uint32_t cd = (code >> (6 * r)) & 63u;
                o[r] = mesh_vertex_id(word, offv, p + mesh_corner_offset((int)(cd >> 3), nx, nxy), (int)(cd & 7u));
            }
            ++t0;
        }
    }
}

}  // namespace nr
