// nr_api_sample.hip -- the C ABI's fitting samples: nr_mesh_sample, nr_points_order, nr_mesh_fit_samples
// (nr_sample.hip, nr_sort.hip; the area table and nr_mesh_area_table: nr_trimesh_host.cpp).
#include <cmath>

#include "nr_ctx.h"

using namespace nr;

namespace {

// what both sampling calls ask of the options; n = n_surface + n_volume
int check_opts(nr_ctx *c, const char *fn, const nr_sample_opts *o, long *n) {
    if (!o) return set_err(c, NR_E_INVALID, "%s: opts is NULL", fn);
    if (o->n_surface < 0 || o->n_volume < 0) return set_err(c, NR_E_INVALID, "%s: a negative count", fn);
    if (o->n_surface > (1l << 27) || o->n_volume > (1l << 27) || o->n_surface + o->n_volume < 1 || o->n_surface + o->n_volume > (1l << 27))
        return set_err(c, NR_E_INVALID, "%s: n = %ld outside [1, 2^27]", fn, o->n_surface + o->n_volume);
    if (!std::isfinite(o->sigma) || o->sigma < 0.0f) return set_err(c, NR_E_INVALID, "%s: sigma = %g is negative or not finite", fn, (double)o->sigma);
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(o->lo[a]) || !std::isfinite(o->hi[a]) || !(o->hi[a] > o->lo[a]))
            return set_err(c, NR_E_INVALID, "%s: the box is empty or not finite along axis %d", fn, a);
    *n = o->n_surface + o->n_volume;
    return NR_OK;
}

int sample_launch(nr_trimesh *m, const nr_sample_opts *o, float *points, int32_t *tri, float *bary, hipStream_t s) {
    nr_ctx *c = m->owner;
    SampleArgs A{};
    A.seed = o->seed;
    A.n_surface = o->n_surface; A.n = o->n_surface + o->n_volume;
    A.sigma = o->sigma;
    for (int a = 0; a < 3; ++a) { A.lo[a] = o->lo[a]; A.ext[a] = o->hi[a] - o->lo[a]; }
    A.tris = m->d_tris; A.thresholds = m->d_area;
    A.ntl = (int)m->ntl; A.last = (int)m->area_last;
    A.points = points; A.tri = tri; A.bary = bary;
    const int grid = (int)std::max<size_t>(1, std::min<size_t>(((size_t)A.n + 255) / 256, (size_t)num_cus(c->device) * 16));
    HIPCHK(c, launch_mesh_sample(A, grid, s));
    return NR_OK;
}

// perm [n] (device) = the stable order of the keys of `mode`, through the context's sort scratch
int order_launch(nr_ctx *c, const float *X, long n, int mode, const float lo[3], const float hi[3], uint64_t seed, int32_t *perm,
                 hipStream_t s) {
    const size_t N = (size_t)n;
    int rc;
    if ((rc = ensure_buf(c, c->d_sort, c->cap_sort, sort_scratch_words(N))) != NR_OK) return rc;
    SortArgs A{};
    A.X = X; A.n = n; A.mode = mode; A.seed = seed;
    if (mode == NR_ORDER_MORTON)
        for (int a = 0; a < 3; ++a) { A.lo[a] = lo[a]; A.inv[a] = 1023.0f / (hi[a] - lo[a]); }
    A.keys[0] = c->d_sort; A.vals[0] = c->d_sort + N; A.keys[1] = c->d_sort + 2 * N; A.vals[1] = c->d_sort + 3 * N;
    A.table = c->d_sort + 4 * N;
    A.nblk = (int)((N + SORT_TILE - 1) / SORT_TILE);
    A.perm = perm;
    HIPCHK(c, launch_points_order(A, s));
    return NR_OK;
}

int check_box(nr_ctx *c, const char *fn, const float lo[3], const float hi[3]) {
    if (!lo || !hi) return set_err(c, NR_E_INVALID, "%s: lo or hi is NULL", fn);
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(lo[a]) || !std::isfinite(hi[a]) || !(hi[a] > lo[a]))
            return set_err(c, NR_E_INVALID, "%s: the box is empty or not finite along axis %d", fn, a);
    return NR_OK;
}

}  // namespace

extern "C" {

int nr_mesh_sample(nr_trimesh *m, const nr_sample_opts *o, float *points, int32_t *tri, float *bary, int loc, nr_stats *stats) {
    if (!m) return set_err(nullptr, NR_E_INVALID, "nr_mesh_sample: mesh is NULL");
    nr_ctx *c = m->owner;
    long n = 0;
    int rc;
    if ((rc = check_opts(c, "nr_mesh_sample", o, &n)) != NR_OK) return rc;
    if (!points) return set_err(c, NR_E_INVALID, "nr_mesh_sample: points is NULL");
    if (o->n_surface > 0 && m->area_last < 0) return set_err(c, NR_E_STATE, "nr_mesh_sample: the mesh has no area to sample");
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    const size_t N = (size_t)n;
    Staging io(loc);
    io.out(points, 3 * N); io.out(tri, N); io.out(bary, 3 * N);
    if ((rc = io.begin(c, m->d_io, m->cap_io, s)) != NR_OK) return rc;
    nr_stats st{};
    HIPCHK(c, hipEventRecord(c->ev0, s));
    if ((rc = sample_launch(m, o, points, tri, bary, s)) != NR_OK) return rc;
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if ((rc = io.end(c, s)) != NR_OK) return rc;
    rc = end_timed(c, stats != nullptr, loc, s, &st.ms_total);
    if (rc != NR_OK || !stats) return rc;
    st.ray_steps = (uint64_t)n;
    st.launches = 1;
    *stats = st;
    return NR_OK;
}

int nr_points_order(nr_ctx *c, const float *X, long n, int mode, const float lo[3], const float hi[3], uint64_t seed, int32_t *perm,
                    float *sorted, int loc, nr_stats *stats) {
    if (!c) return set_err(nullptr, NR_E_INVALID, "nr_points_order: ctx is NULL");
    if (!perm) return set_err(c, NR_E_INVALID, "nr_points_order: perm is NULL");
    if (n < 1 || n > (1l << 27)) return set_err(c, NR_E_INVALID, "nr_points_order: n = %ld outside [1, 2^27]", n);
    if (mode != NR_ORDER_MORTON && mode != NR_ORDER_SHUFFLE) return set_err(c, NR_E_INVALID, "nr_points_order: unknown mode %d", mode);
    if (mode == NR_ORDER_MORTON && !X) return set_err(c, NR_E_INVALID, "nr_points_order: X is NULL");
    if (sorted && !X) return set_err(c, NR_E_INVALID, "nr_points_order: sorted without X");
    int rc;
    if (mode == NR_ORDER_MORTON && (rc = check_box(c, "nr_points_order", lo, hi)) != NR_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    const size_t N = (size_t)n;
    Staging io(loc);
    io.in(X, 3 * N);
    io.out(perm, N); io.out(sorted, 3 * N);
    if ((rc = io.begin(c, c->d_sortio, c->cap_sortio, s)) != NR_OK) return rc;
    nr_stats st{};
    HIPCHK(c, hipEventRecord(c->ev0, s));
    if ((rc = order_launch(c, X, n, mode, lo, hi, seed, perm, s)) != NR_OK) return rc;
    if (sorted) HIPCHK(c, launch_gather(X, nullptr, perm, n, sorted, nullptr, s));
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if ((rc = io.end(c, s)) != NR_OK) return rc;
    rc = end_timed(c, stats != nullptr, loc, s, &st.ms_total);
    if (rc != NR_OK || !stats) return rc;
    st.ray_steps = (uint64_t)n;
    st.launches = SORT_LAUNCHES + (sorted ? 1 : 0);
    *stats = st;
    return NR_OK;
}

int nr_mesh_fit_samples(nr_trimesh *m, const nr_sample_opts *o, float *X, float *Y, int loc, nr_stats *stats) {
    if (!m) return set_err(nullptr, NR_E_INVALID, "nr_mesh_fit_samples: mesh is NULL");
    nr_ctx *c = m->owner;
    long n = 0;
    int rc;
    if ((rc = check_opts(c, "nr_mesh_fit_samples", o, &n)) != NR_OK) return rc;
    if (!X || !Y) return set_err(c, NR_E_INVALID, "nr_mesh_fit_samples: X or Y is NULL");
    if (o->sign != NR_SAMPLE_SIGN_NORMAL && o->sign != NR_SAMPLE_SIGN_WINDING)
        return set_err(c, NR_E_INVALID, "nr_mesh_fit_samples: unknown sign %d", o->sign);
    if (!std::isfinite(o->beta) || o->beta < 0.0f)
        return set_err(c, NR_E_INVALID, "nr_mesh_fit_samples: beta = %g is negative or not finite", (double)o->beta);
    if (o->n_surface > 0 && m->area_last < 0) return set_err(c, NR_E_STATE, "nr_mesh_fit_samples: the mesh has no area to sample");
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    const size_t N = (size_t)n;
    if ((rc = ensure_buf(c, c->d_fitsamp, c->cap_fitsamp, 8 * N)) != NR_OK) return rc;
    float *P = c->d_fitsamp, *Ps = P + 3 * N, *Ys = P + 6 * N;  // the samples, in Morton order, their values
    int32_t *perm = reinterpret_cast<int32_t *>(P + 7 * N);
    Staging io(loc);
    io.out(X, 3 * N); io.out(Y, N);
    if ((rc = io.begin(c, m->d_io, m->cap_io, s)) != NR_OK) return rc;
    nr_stats st{};
    HIPCHK(c, hipEventRecord(c->ev0, s));
    HIPCHK(c, hipMemsetAsync(m->d_stats, 0, 8, s));
    if ((rc = sample_launch(m, o, P, nullptr, nullptr, s)) != NR_OK) return rc;
    if ((rc = order_launch(c, P, n, NR_ORDER_MORTON, o->lo, o->hi, 0, perm, s)) != NR_OK) return rc;
    HIPCHK(c, launch_gather(P, nullptr, perm, n, Ps, nullptr, s));
    // the query's own launches (nr_trimesh_distance, nr_mesh_winding with sdf) on the sorted points
    const size_t chunks = (N + 63) / 64;
    const int grid = (int)std::max<size_t>(1, std::min<size_t>((chunks + 3) / 4, (size_t)num_cus(c->device) * 8));
    TriMeshArgs D{};
    D.X = Ps; D.n = n;
    D.nodes = m->d_nodes; D.tris = m->d_tris; D.table = m->d_table;
    D.nnodes = (int)m->nnodes; D.ntl = (int)m->ntl;
    D.sdf = Ys;
    D.stats = m->d_stats;
    HIPCHK(c, launch_trimesh_distance(D, grid, s));
    if (o->sign == NR_SAMPLE_SIGN_WINDING) {
        TriWindArgs W{};
        W.X = Ps; W.n = n;
        W.nodes = m->d_nodes; W.tris = m->d_tris; W.moments = m->d_moments;
        W.nnodes = (int)m->nnodes; W.ntl = (int)m->ntl;
        W.beta = o->beta == 0.0f ? 2.0f : o->beta;
        W.sdf = Ys;
        W.stats = m->d_stats;
        HIPCHK(c, launch_trimesh_winding(W, grid, s));
    }
    if ((rc = order_launch(c, nullptr, n, NR_ORDER_SHUFFLE, nullptr, nullptr, o->seed, perm, s)) != NR_OK) return rc;
    HIPCHK(c, launch_gather(Ps, Ys, perm, n, X, Y, s));
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if ((rc = io.end(c, s)) != NR_OK) return rc;
    unsigned long long evals = 0;
    if (stats) HIPCHK(c, hipMemcpyAsync(&evals, m->d_stats, 8, hipMemcpyDeviceToHost, s));
    rc = end_timed(c, stats != nullptr, loc, s, &st.ms_total);
    if (rc != NR_OK || !stats) return rc;
    st.ray_steps = (uint64_t)n;
    st.shade_evals = evals;
    // the counter's memset, k_mesh_sample, two orders, two gathers, k_trimesh_distance, k_trimesh_winding
    st.launches = 5 + 2 * SORT_LAUNCHES + (o->sign == NR_SAMPLE_SIGN_WINDING ? 1 : 0);
    *stats = st;
    return NR_OK;
}

}  // extern "C"
