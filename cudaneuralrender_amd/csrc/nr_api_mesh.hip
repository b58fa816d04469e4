// nr_api_mesh.hip -- the C ABI's lattice calls: volume sampling, dense and brick-sparse isosurface
// extraction (nr_mesh.hip, nr_sparse.hip) and nr_obj_save.  mesh_run and sparse_run serve a composed
// scene's extraction too (nr_api_compose.hip).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>

#include "nr_ctx.h"

using namespace nr;

// ---- volume sampling and isosurface extraction (nr_mesh.hip) ----

static int fused_check(nr_ctx *c, const char *fn) {
    if (c->dims.empty()) return set_err(c, NR_E_STATE, "%s: no network loaded", fn);
    if (!c->fused)
        return set_err(c, NR_E_FORMAT, "%s: volume sampling needs a [3|4, 32, ..., 32, 1] network (no layered fallback)", fn);
    return NR_OK;
}

// One k_grid launch over the lattice into d_sdf.  The grid by the CU count: nr_set_occupancy's
// workgroups per CU, or 12 as nr_mlp_forward's (more than fit at once, so that they start staggered)
static int grid_launch(nr_ctx *c, const LatticeArgs &L, float *d_sdf, hipStream_t s) {
    GridArgs G{};
    G.L = L;
    G.scene = c->scene;
    G.frame = c->frame;
    G.sdf = d_sdf;
    HIPCHK(c, launch_grid(G, c->mlp16, persistent_grid(c, (size_t)L.n, 256, 12), s));
    return NR_OK;
}

// ensure_buf for scratch whose size the lattice decides: a refused allocation is NR_E_NOMEM
static int ensure_scratch(nr_ctx *c, const char *fn, const char *what, unsigned long long *&p, size_t &cap, size_t words) {
    if (words <= cap) return NR_OK;
    dfree(p);
    cap = 0;
    if (hipMalloc(&p, words * 8) != hipSuccess) {
        (void)hipGetLastError();
        p = nullptr;
        return set_err(c, NR_E_NOMEM, "%s: cannot allocate %zu bytes of %s scratch", fn, words * 8, what);
    }
    cap = words;
    return NR_OK;
}

namespace nr {

// The lattice arguments: every dim >= min_dim and at most 2^30 points.
int lattice_check(nr_ctx *c, const char *fn, const float *origin, const float *step, const int *dims, int min_dim) {
    if (!origin || !step || !dims) return set_err(c, NR_E_INVALID, "%s: NULL lattice arguments", fn);
    long n = 1;
    for (int a = 0; a < 3; ++a) {
        if (dims[a] < min_dim) return set_err(c, NR_E_INVALID, "%s: dims[%d] = %d < %d", fn, a, dims[a], min_dim);
        n *= dims[a];  // (at most 2^30 * 2^31 before the test)
        if (n > (1l << 30)) return set_err(c, NR_E_INVALID, "%s: more than 2^30 lattice points", fn);
    }
    return NR_OK;
}

// Count, scan and (with output buffers of sufficient capacity) emit over the device lattice d_sdf;
// with `normals` the vertex normals too.  cp: the lattice holds the composed field of cp (whose owner
// is c): the normals are that field's and `part` (may be NULL) gets the vertices' owners.  field: the
// lattice holds that field: no normals, and `part` (may be NULL) gets its labels.  *launches counts
// the kernels issued.
int mesh_run(nr_ctx *c, const char *fn, hipStream_t s, const LatticeArgs &L, const float *d_sdf, float iso,
                    float *vertices, float *normals, long v_cap, int32_t *triangles, long t_cap, long *nv, long *nt,
                    int loc, int *launches, nr_compose *cp, int32_t *part, const FieldSource *field) {
    const size_t N = (size_t)L.n;
    const size_t nblk = (N + 255) / 256;
    // scratch, in 8-byte words: totals [2], scans [2][nblk], block counts [2][nblk] u32, point words [N] u32
    const size_t need = 2 + 2 * nblk + nblk + (N + 1) / 2;
    int rc;
    if ((rc = ensure_buf(c, c->d_mesh, c->cap_mesh, need)) != NR_OK) return rc;
    MeshArgs A{};
    A.L = L;
    A.sdf = d_sdf;
    A.iso = iso;
    A.nblk = (int)nblk;
    A.total = c->d_mesh;
    A.off = c->d_mesh + 2;
    A.cnt = reinterpret_cast<uint32_t *>(c->d_mesh + 2 + 2 * nblk);
    A.word = A.cnt + 2 * nblk;
    HIPCHK(c, launch_mesh_count(A, s));
    *launches += 2;
    unsigned long long tot[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(tot, A.total, sizeof tot, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    *nv = (long)tot[0];
    *nt = (long)tot[1];
    if (tot[0] > (unsigned long long)INT32_MAX)
        return set_err(c, NR_E_INVALID, "%s: %llu vertices do not fit 32-bit indices", fn, tot[0]);
    if (!vertices && !triangles) return NR_OK;  // count only
    if (!vertices || !triangles) return set_err(c, NR_E_INVALID, "%s: vertices and triangles are given together", fn);
    if (v_cap < *nv || t_cap < *nt)
        return set_err(c, NR_E_NOMEM, "%s: %ld vertices / %ld triangles exceed the capacities %ld / %ld", fn, *nv, *nt,
                       v_cap, t_cap);
    if (tot[0] == 0) return NR_OK;  // (no crossing edge: no triangle either)
    const size_t NV = (size_t)tot[0], V3 = 3 * NV, T3 = 3 * (size_t)tot[1];
    float *dv = vertices, *dn = normals;
    int32_t *dt = triangles, *dp = part;
    Staging io(loc);  // (in the order of the downloads)
    io.out(dv, V3); io.out(dn, V3); io.out(dp, NV); io.out(dt, T3);
    if ((rc = io.begin(c, c->d_mio, c->cap_mio, s)) != NR_OK) return rc;
    A.vertices = dv;
    A.triangles = dt;
    HIPCHK(c, launch_mesh_emit(A, s));
    *launches += 1;
    if (field) {
        if (dp && (rc = field->label(field->self, dv, dp, NV, s, launches)) != NR_OK) return rc;
    } else if (cp) {
        if (dn || dp) {
            if ((rc = compose_vertex_pass(cp, dv, dn, dp, NV, s)) != NR_OK) return rc;
            *launches += 1;
        }
    } else if (normals) {
        VNormalArgs V{};
        V.vertices = dv;
        V.normals = dn;
        V.nv = (long)tot[0];
        V.scene = c->scene;
        V.frame = c->frame;
        // 64 vertices per workgroup and pass
        HIPCHK(c, launch_vnormal(V, c->mlp16, persistent_grid(c, NV, 64, 4), s));
        *launches += 1;
    }
    if ((rc = io.end(c, s)) != NR_OK) return rc;
    if (loc != NR_DEVICE) HIPCHK(c, hipStreamSynchronize(s));
    return NR_OK;
}

// ---- brick-sparse extraction (nr_sparse.hip) ----

// nr_extract_mesh_sparse on c's stream and scratch.  cp == NULL: c's network and scene.  cp: the
// composed field of cp (whose owner is c) in the two samplers and the vertex pass, which then
// writes `part` too (may be NULL); the caller has zeroed cp's statistics.  field (cp == NULL): that
// field in the two samplers, and its labels into `part` (may be NULL; no normals).  timed: *done gets ms.
int sparse_run(nr_ctx *c, nr_compose *cp, const char *fn, const float origin[3], const float step[3], const int dims[3],
                      float iso, int brick, float band, float *vertices, float *normals, int32_t *part, int64_t *keys,
                      long v_cap, int32_t *triangles, long t_cap, long *nv, long *nt, long *active_bricks, int loc, bool timed,
                      SparseDone *done, const FieldSource *field) {
    if (!origin || !step || !dims || !nv || !nt) return set_err(c, NR_E_INVALID, "%s: NULL origin, step, dims, nv or nt", fn);
    *nv = 0;
    *nt = 0;
    if (active_bricks) *active_bricks = 0;
    for (int a = 0; a < 3; ++a)
        if (dims[a] < 2 || dims[a] > 65536) return set_err(c, NR_E_INVALID, "%s: dims[%d] = %d outside 2..65536", fn, a, dims[a]);
    if (brick != 4 && brick != 8 && brick != 16) return set_err(c, NR_E_INVALID, "%s: brick = %d is not 4, 8 or 16", fn, brick);
    if (!(band >= 0.0f)) return set_err(c, NR_E_INVALID, "%s: band is negative or NaN", fn);
    if (!std::isfinite(iso)) return set_err(c, NR_E_INVALID, "%s: iso is not finite", fn);
    if (!vertices != !triangles) return set_err(c, NR_E_INVALID, "%s: vertices and triangles are given together", fn);
    if ((keys || normals) && !vertices) return set_err(c, NR_E_INVALID, "%s: keys and normals need vertices", fn);
    if (part && !vertices) return set_err(c, NR_E_INVALID, "%s: part needs vertices", fn);
    SparseArgs A{};
    SparseLattice &L = A.L;
    for (int a = 0; a < 3; ++a) { L.origin[a] = origin[a]; L.step[a] = step[a]; }
    L.nx = dims[0]; L.ny = dims[1]; L.nz = dims[2];
    L.B = brick; L.S = brick + 1;
    L.nbx = (L.nx - 1 + brick - 1) / brick; L.nby = (L.ny - 1 + brick - 1) / brick; L.nbz = (L.nz - 1 + brick - 1) / brick;
    const unsigned long long nbricks = (unsigned long long)L.nbx * L.nby * L.nbz;
    if (nbricks > (1ull << 30)) return set_err(c, NR_E_INVALID, "%s: %llu bricks, more than 2^30", fn, nbricks);
    int rc;
    if (!cp && !field && (rc = fused_check(c, fn)) != NR_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    L.nbricks = (uint32_t)nbricks;
    L.ncoarse = (uint32_t)((unsigned long long)(L.nbx + 1) * (L.nby + 1) * (L.nbz + 1));  // < 2^32: at most 2^30 bricks of <= 2^14 an axis
    L.P = (uint32_t)(L.S * L.S * L.S);
    L.stride = (L.P + 63u) & ~63u;
    L.inv_nbx = 1.0 / (double)L.nbx;
    L.inv_nbxy = 1.0 / ((double)L.nbx * (double)L.nby);
    L.inv_cx = 1.0 / (double)(L.nbx + 1);
    L.inv_cxy = 1.0 / ((double)(L.nbx + 1) * (double)(L.nby + 1));
    L.inv_s = 1.0 / (double)L.S;
    L.inv_ss = 1.0 / (double)(L.S * L.S);
    L.inv_wpb = 1.0 / (double)(L.stride >> 6);
    A.iso = iso; A.band = band;
    A.scene = c->scene; A.frame = c->frame;
    // per-brick scratch, in 8-byte words: totals [2], scans [2][nblk], block counts [2][nblk] u32, the
    // map [nbricks] i32, the corner values [ncoarse] f32
    const size_t nblk_b = ((size_t)L.nbricks + 255) / 256;
    if ((rc = ensure_scratch(c, fn, "per-brick", c->d_spb, c->cap_spb,
                             2 + 2 * nblk_b + nblk_b + ((size_t)L.nbricks + 1) / 2 + ((size_t)L.ncoarse + 1) / 2)) != NR_OK)
        return rc;
    A.nblk_b = (int)nblk_b;
    A.btotal = c->d_spb;
    A.boff = c->d_spb + 2;
    A.bcnt = reinterpret_cast<uint32_t *>(c->d_spb + 2 + 2 * nblk_b);
    A.map = reinterpret_cast<int32_t *>(c->d_spb + 2 + 3 * nblk_b);
    A.coarse = reinterpret_cast<float *>(c->d_spb + 2 + 3 * nblk_b + ((size_t)L.nbricks + 1) / 2);
    HIPCHK(c, hipEventRecord(c->ev0, s));
    int launches = 3;  // a sampler's one launch, the classification, its scan
    if (field) {
        launches -= 1;
        if ((rc = field->sample(field->self, A, false, s, &launches)) != NR_OK) return rc;
    } else if (cp) {
        if ((rc = compose_sparse_sampler(cp, A, false, s)) != NR_OK) return rc;
    } else {
        HIPCHK(c, launch_sparse_coarse(A, c->mlp16, persistent_grid(c, L.ncoarse, 256, 12), s));  // as nr_sample_grid
    }
    HIPCHK(c, launch_sparse_classify_count(A, s));
    MeshArgs scan{};
    scan.nblk = A.nblk_b; scan.cnt = A.bcnt; scan.off = A.boff; scan.total = A.btotal;
    HIPCHK(c, launch_mesh_scan(scan, s));
    unsigned long long btot[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(btot, A.btotal, sizeof btot, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    A.nactive = (uint32_t)btot[0];
    if (active_bricks) *active_bricks = (long)btot[0];
    unsigned long long mtot[2] = {0, 0};
    const bool with_normals = normals && vertices;
    if (A.nactive) {
        // per-active-brick scratch: totals [2], scans [2][nblk], block counts [2][nblk] u32, the list
        // [nactive] u32, the words and the values [nactive stride] u32 / f32
        const size_t npts = (size_t)A.nactive * L.stride;
        if (npts >= ((size_t)1 << 37))
            return set_err(c, NR_E_NOMEM, "%s: %u active bricks need more than 1 TiB of scratch", fn, A.nactive);
        const size_t nblk_m = (npts + 255) / 256;
        if ((rc = ensure_scratch(c, fn, "per-active-brick", c->d_spa, c->cap_spa,
                                 2 + 2 * nblk_m + nblk_m + ((size_t)A.nactive + 1) / 2 + npts)) != NR_OK)
            return rc;
        A.nblk_m = (int)nblk_m;
        A.total = c->d_spa;
        A.off = c->d_spa + 2;
        A.cnt = reinterpret_cast<uint32_t *>(c->d_spa + 2 + 2 * nblk_m);
        A.list = reinterpret_cast<uint32_t *>(c->d_spa + 2 + 3 * nblk_m);
        A.word = reinterpret_cast<uint32_t *>(c->d_spa + 2 + 3 * nblk_m + ((size_t)A.nactive + 1) / 2);
        A.store = reinterpret_cast<float *>(A.word + npts);
        HIPCHK(c, launch_sparse_classify_emit(A, s));
        if (field) {
            launches -= 1;
            if ((rc = field->sample(field->self, A, true, s, &launches)) != NR_OK) return rc;
        } else if (cp) {
            if ((rc = compose_sparse_sampler(cp, A, true, s)) != NR_OK) return rc;
        } else {
            HIPCHK(c, launch_sparse_sample(A, c->mlp16, persistent_grid(c, npts, 256, 12), s));
        }
        HIPCHK(c, launch_sparse_mesh_count(A, s));
        scan.nblk = A.nblk_m; scan.cnt = A.cnt; scan.off = A.off; scan.total = A.total;
        HIPCHK(c, launch_mesh_scan(scan, s));
        launches += 4;
        HIPCHK(c, hipMemcpyAsync(mtot, A.total, sizeof mtot, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
    }
    *nv = (long)mtot[0];
    *nt = (long)mtot[1];
    if (mtot[0] > (unsigned long long)INT32_MAX)
        return set_err(c, NR_E_INVALID, "%s: %llu vertices do not fit 32-bit indices", fn, mtot[0]);
    if (vertices && (v_cap < *nv || t_cap < *nt))
        return set_err(c, NR_E_NOMEM, "%s: %ld vertices / %ld triangles exceed the capacities %ld / %ld", fn, *nv, *nt,
                       v_cap, t_cap);
    if (vertices && mtot[0]) {
        const size_t NV = (size_t)mtot[0], V3 = 3 * NV, T3 = 3 * (size_t)mtot[1];
        float *dv = vertices, *dn = with_normals ? normals : nullptr;
        int64_t *dk = keys;
        int32_t *dt = triangles, *dp = part;
        Staging io(loc);  // (in the order of the downloads; the keys get their 8-byte alignment)
        io.out(dv, V3); io.out(dn, V3); io.out(dk, 2 * NV); io.out(dp, NV); io.out(dt, T3);
        if ((rc = io.begin(c, c->d_mio, c->cap_mio, s)) != NR_OK) return rc;
        A.vertices = dv;
        A.keys = reinterpret_cast<long long *>(dk);
        A.triangles = dt;
        HIPCHK(c, launch_sparse_mesh_emit(A, s));
        launches += 1;
        if (field) {
            if (dp && (rc = field->label(field->self, dv, dp, NV, s, &launches)) != NR_OK) return rc;
        } else if (cp) {
            if (dn || dp) {
                if ((rc = compose_vertex_pass(cp, dv, dn, dp, NV, s)) != NR_OK) return rc;
                launches += 1;
            }
        } else if (with_normals) {
            VNormalArgs V{};
            V.vertices = dv;
            V.normals = dn;
            V.nv = (long)NV;
            V.scene = c->scene;
            V.frame = c->frame;
            HIPCHK(c, launch_vnormal(V, c->mlp16, persistent_grid(c, NV, 64, 4), s));  // as nr_extract_mesh
            launches += 1;
        }
        if ((rc = io.end(c, s)) != NR_OK) return rc;
        if (loc != NR_DEVICE) HIPCHK(c, hipStreamSynchronize(s));
    }
    HIPCHK(c, hipEventRecord(c->ev1, s));
    done->points = (uint64_t)L.ncoarse + btot[1];
    done->active = btot[0];
    done->launches = launches;
    if (timed) {
        HIPCHK(c, hipStreamSynchronize(s));
        HIPCHK(c, hipEventElapsedTime(&done->ms, c->ev0, c->ev1));
    }
    return NR_OK;
}

}  // namespace nr

extern "C" {

int nr_sample_grid(nr_ctx *c, const float origin[3], const float step[3], const int dims[3], float *sdf, int loc,
                   nr_stats *stats) {
    if (!c) return set_err(nullptr, NR_E_INVALID, "nr_sample_grid: ctx is NULL");
    if (!sdf) return set_err(c, NR_E_INVALID, "nr_sample_grid: sdf is NULL");
    int rc;
    if ((rc = lattice_check(c, "nr_sample_grid", origin, step, dims, 1)) != NR_OK) return rc;
    if ((rc = fused_check(c, "nr_sample_grid")) != NR_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    const LatticeArgs L = make_lattice(origin, step, dims);
    const size_t N = (size_t)L.n;
    float *d = sdf;
    if (loc != NR_DEVICE) {
        if ((rc = ensure_buf(c, c->d_grid, c->cap_grid, N)) != NR_OK) return rc;
        d = c->d_grid;
    }
    HIPCHK(c, hipEventRecord(c->ev0, s));
    if ((rc = grid_launch(c, L, d, s)) != NR_OK) return rc;
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if (loc != NR_DEVICE) HIPCHK(c, hipMemcpyAsync(sdf, d, N * 4, hipMemcpyDeviceToHost, s));
    nr_stats st{};
    st.ray_steps = N;
    st.launches = 1;
    if ((rc = end_timed(c, stats != nullptr, loc, s, &st.ms_total)) != NR_OK) return rc;
    if (stats) *stats = st;
    return NR_OK;
}

int nr_mesh_grid(nr_ctx *c, const float *sdf, const float origin[3], const float step[3], const int dims[3], float iso,
                 float *vertices, long v_cap, int32_t *triangles, long t_cap, long *nv, long *nt, int loc) {
    if (!c) return set_err(nullptr, NR_E_INVALID, "nr_mesh_grid: ctx is NULL");
    if (!sdf || !nv || !nt) return set_err(c, NR_E_INVALID, "nr_mesh_grid: NULL sdf, nv or nt");
    *nv = 0;
    *nt = 0;
    int rc;
    if ((rc = lattice_check(c, "nr_mesh_grid", origin, step, dims, 2)) != NR_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    const LatticeArgs L = make_lattice(origin, step, dims);
    const float *d = sdf;
    if (loc != NR_DEVICE) {
        if ((rc = ensure_buf(c, c->d_grid, c->cap_grid, (size_t)L.n)) != NR_OK) return rc;
        HIPCHK(c, hipMemcpyAsync(c->d_grid, sdf, (size_t)L.n * 4, hipMemcpyHostToDevice, s));
        d = c->d_grid;
    }
    int launches = 0;
    return mesh_run(c, "nr_mesh_grid", s, L, d, iso, vertices, nullptr, v_cap, triangles, t_cap, nv, nt, loc, &launches);
}

int nr_extract_mesh(nr_ctx *c, const float origin[3], const float step[3], const int dims[3], float iso, float *vertices,
                    float *normals, long v_cap, int32_t *triangles, long t_cap, long *nv, long *nt, int loc,
                    nr_stats *stats) {
    if (!c) return set_err(nullptr, NR_E_INVALID, "nr_extract_mesh: ctx is NULL");
    if (!nv || !nt) return set_err(c, NR_E_INVALID, "nr_extract_mesh: NULL nv or nt");
    *nv = 0;
    *nt = 0;
    int rc;
    if ((rc = lattice_check(c, "nr_extract_mesh", origin, step, dims, 2)) != NR_OK) return rc;
    if ((rc = fused_check(c, "nr_extract_mesh")) != NR_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    const LatticeArgs L = make_lattice(origin, step, dims);
    if ((rc = ensure_buf(c, c->d_grid, c->cap_grid, (size_t)L.n)) != NR_OK) return rc;
    HIPCHK(c, hipEventRecord(c->ev0, s));
    if ((rc = grid_launch(c, L, c->d_grid, s)) != NR_OK) return rc;
    int launches = 1;
    const bool with_normals = normals && vertices && triangles;
    rc = mesh_run(c, "nr_extract_mesh", s, L, c->d_grid, iso, vertices, with_normals ? normals : nullptr, v_cap, triangles,
                  t_cap, nv, nt, loc, &launches);
    if (rc != NR_OK) return rc;
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if (stats) {
        HIPCHK(c, hipStreamSynchronize(s));
        nr_stats st{};
        st.ray_steps = (uint64_t)L.n;
        st.rays_shaded = (uint64_t)*nv;
        st.shade_evals = with_normals ? 4ull * (uint64_t)*nv : 0ull;
        st.launches = launches;
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
        st.ms_total = ms;
        *stats = st;
    }
    return NR_OK;
}

int nr_extract_mesh_sparse(nr_ctx *c, const float origin[3], const float step[3], const int dims[3], float iso, int brick,
                           float band, float *vertices, float *normals, int64_t *keys, long v_cap, int32_t *triangles,
                           long t_cap, long *nv, long *nt, long *active_bricks, int loc, nr_stats *stats) {
    const char *fn = "nr_extract_mesh_sparse";
    if (!c) return set_err(nullptr, NR_E_INVALID, "%s: ctx is NULL", fn);
    SparseDone done;
    const int rc = sparse_run(c, nullptr, fn, origin, step, dims, iso, brick, band, vertices, normals, nullptr, keys, v_cap,
                              triangles, t_cap, nv, nt, active_bricks, loc, stats != nullptr, &done);
    if (rc != NR_OK) return rc;
    if (stats) {
        nr_stats st{};
        st.ray_steps = done.points;
        st.rays_hit = done.active;
        st.rays_shaded = (uint64_t)*nv;
        st.shade_evals = normals && vertices ? 4ull * (uint64_t)*nv : 0ull;
        st.launches = done.launches;
        st.ms_total = done.ms;
        *stats = st;
    }
    return NR_OK;
}

int nr_obj_save(const char *path, const float *vertices, long nv, const float *normals, const int32_t *triangles,
                long nt) {
    if (!path || nv < 0 || nt < 0 || (nv > 0 && !vertices) || (nt > 0 && !triangles))
        return set_err(nullptr, NR_E_INVALID, "nr_obj_save: bad arguments");
    FILE *f = fopen(path, "w");
    if (!f) return set_err(nullptr, NR_E_IO, "nr_obj_save: cannot open %s", path);
    for (long i = 0; i < nv; ++i)
        fprintf(f, "v %.9g %.9g %.9g\n", (double)vertices[3 * i], (double)vertices[3 * i + 1], (double)vertices[3 * i + 2]);
    if (normals)
        for (long i = 0; i < nv; ++i)
            fprintf(f, "vn %.9g %.9g %.9g\n", (double)normals[3 * i], (double)normals[3 * i + 1], (double)normals[3 * i + 2]);
    for (long i = 0; i < nt; ++i) {
        const long a = (long)triangles[3 * i] + 1, b = (long)triangles[3 * i + 1] + 1, d = (long)triangles[3 * i + 2] + 1;
        if (normals) fprintf(f, "f %ld//%ld %ld//%ld %ld//%ld\n", a, a, b, b, d, d);
        else fprintf(f, "f %ld %ld %ld\n", a, b, d);
    }
    const bool bad = ferror(f) != 0;
    if (fclose(f) != 0 || bad) return set_err(nullptr, NR_E_IO, "nr_obj_save: write to %s failed", path);
    return NR_OK;
}

}  // extern "C"
