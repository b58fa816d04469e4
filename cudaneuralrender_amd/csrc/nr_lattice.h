// nr_lattice.h -- the lattice and brick index arithmetic as device functions, shared by the
// single-network samplers and mesh passes (nr_mesh.hip, nr_sparse.hip) and by the composed-scene
// samplers (nr_compose_mesh.hip): a point's coordinate always comes from its global lattice index,
// origin[a] + (float)idx_a * step[a], so a value has the same bits whichever kernel or brick
// evaluates it.
#pragma once
#include "nr_internal.h"
#include "nr_kernels.h"
#include "nr_device.h"

namespace nr {

// (i, j, k) of linear index p
__device__ __forceinline__ void lattice_ijk(const LatticeArgs &L, uint32_t p, int &i, int &j, int &k) {
    const uint32_t nxy = (uint32_t)L.nx * (uint32_t)L.ny;
    const uint32_t kk = udiv_r(p, nxy, L.inv_nxy);
    const uint32_t r = p - kk * nxy;
    const uint32_t jj = udiv_r(r, (uint32_t)L.nx, L.inv_nx);
    i = (int)(r - jj * (uint32_t)L.nx);
    j = (int)jj;
    k = (int)kk;
}

struct Brick {
    int b[3];  // brick coordinates
    int e[3];  // cells along each axis, 1..B (the last brick of an axis may be ragged)
};

__device__ __forceinline__ Brick brick_of(const SparseLattice &L, uint32_t idx) {
    Brick K;
    const uint32_t nbxy = (uint32_t)L.nbx * (uint32_t)L.nby;
    const uint32_t bz = udiv_r(idx, nbxy, L.inv_nbxy);
    const uint32_t r = idx - bz * nbxy;
    const uint32_t by = udiv_r(r, (uint32_t)L.nbx, L.inv_nbx);
    K.b[0] = (int)(r - by * (uint32_t)L.nbx);
    K.b[1] = (int)by;
    K.b[2] = (int)bz;
    K.e[0] = min(L.B, L.nx - 1 - L.B * K.b[0]);
    K.e[1] = min(L.B, L.ny - 1 - L.B * K.b[1]);
    K.e[2] = min(L.B, L.nz - 1 - L.B * K.b[2]);
    return K;
}

__device__ __forceinline__ uint32_t brick_index(const SparseLattice &L, int bx, int by, int bz) {
    return ((uint32_t)bz * (uint32_t)L.nby + (uint32_t)by) * (uint32_t)L.nbx + (uint32_t)bx;
}

// (li, lj, lk) of local index r < S^3
__device__ __forceinline__ void local_ijk(const SparseLattice &L, uint32_t r, int &li, int &lj, int &lk) {
    const uint32_t ss = (uint32_t)(L.S * L.S);
    const uint32_t kk = udiv_r(r, ss, L.inv_ss);
    const uint32_t q = r - kk * ss;
    const uint32_t jj = udiv_r(q, (uint32_t)L.S, L.inv_s);
    li = (int)(q - jj * (uint32_t)L.S);
    lj = (int)jj;
    lk = (int)kk;
}

__device__ __forceinline__ F3 lattice_point(const SparseLattice &L, int i, int j, int k) {
    return mk3(L.origin[0] + (float)i * L.step[0], L.origin[1] + (float)j * L.step[1], L.origin[2] + (float)k * L.step[2]);
}

// the brick-corner lattice (cx = nbx + 1 by nby + 1 by nbz + 1 corners, cxy = cx (nby + 1)): corner
// idx < ncoarse is the lattice point min(B c, dim - 1) per axis
__device__ __forceinline__ F3 corner_point(const SparseLattice &L, uint32_t idx, uint32_t cx, uint32_t cxy) {
    const uint32_t ck = udiv_r(idx, cxy, L.inv_cxy);
    const uint32_t r = idx - ck * cxy;
    const uint32_t cj = udiv_r(r, cx, L.inv_cx);
    const uint32_t ci = r - cj * cx;
    return lattice_point(L, min(L.B * (int)ci, L.nx - 1), min(L.B * (int)cj, L.ny - 1), min(L.B * (int)ck, L.nz - 1));
}

}  // namespace nr
