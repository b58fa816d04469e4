// nr_api_points.hip -- the C ABI's calls over caller-supplied rays and points: ray queries and
// geometry buffers (nr_query.hip), lighting (nr_light.hip), the MLP itself (nr_mlp_forward,
// nr_layer_forward, nr_dense_forward), its gradient (nr_grad.hip) and projection (nr_project.hip).
//
// Replaces, on the reference side (daviesthomas/cudaNeuralRender @ v1):
//   NeuralNetwork::load / forward                          src/neuralNetwork.cpp:54-151
//   DenseLayer ctor / forward                              src/layers/denseLayer.cu:180-278
#include <algorithm>
#include <cmath>
#include <cstring>

#include "nr_ctx.h"

using namespace nr;

namespace {

// one dense layer over n rows (k_dense<0>)
hipError_t dense_rows(const float *W, const float *b, const float *A, float *Z, long n, int in, int out, int relu,
                      int cus, hipStream_t s) {
    DenseArgs D{};
    D.W = W; D.b = b; D.A = A; D.Z = Z;
    D.n = n; D.chunk0 = 0; D.chunk_n = n;
    D.in = in; D.out = out; D.relu = relu;
    const int grid = (int)std::max<long>(1, std::min<long>((n * out + 255) / 256, (long)cus * 8));
    return launch_dense(D, 0, grid, s);
}

}  // namespace

// The QueryArgs of n rays but for the rays and the outputs: the view, scene and frame of the
// context, the cursor and the statistics in d_qs (allocated by the caller).
static QueryArgs query_args(const nr_ctx *c, long n, int W, int H, int max_steps) {
    QueryArgs Q{};
    Q.n = n; Q.W = W; Q.H = H;
    Q.inv_w = 1.0 / (double)W;
    Q.rcp_w = pow2_rcp(W); Q.rcp_h = pow2_rcp(H);
    memcpy(Q.inv_view, c->inv_view, sizeof Q.inv_view);
    Q.max_steps = max_steps; Q.scene = c->scene; Q.frame = c->frame;
    Q.cursor = c->d_qs;
    Q.stats = reinterpret_cast<unsigned long long *>(c->d_qs + 32);
    return Q;
}

// The grid of a persistent launch over n rays or pixels (k_query, k_light_trace), by the CU count
// as the frame tracer's: nr_set_occupancy's workgroups per CU, or 2 (one launch of rays is a single
// frame's worth: the tail outweighs the bulk, default_bpc)
static int query_grid(const nr_ctx *c, size_t n) { return persistent_grid(c, n, 256, 2); }

// Ray queries: n caller-supplied rays (origins / dirs), or with origins == NULL the W x H pixel
// rays of the context's view, through one k_query launch (nr_query.hip).  Always the fp32 MLP.
static int query_rays(nr_ctx *c, const char *fn, const float *origins, const float *dirs, long n, int W, int H,
                      int max_steps, int32_t *status, int32_t *steps, float *t, float *position, float *normal, int loc,
                      nr_stats *stats) {
    if (c->dims.empty()) return set_err(c, NR_E_STATE, "%s: no network loaded", fn);
    if (!c->fused)
        return set_err(c, NR_E_FORMAT, "%s: ray queries need a [3|4, 32, ..., 32, 1] network (no layered fallback)", fn);
    nr_stats st{};
    if (n == 0) { if (stats) *stats = st; return NR_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    if (!c->d_qs) HIPCHK(c, hipMalloc(&c->d_qs, CURSOR_STATS_BYTES));
    QueryArgs Q = query_args(c, n, W, H, max_steps);
    Q.origins = origins; Q.dirs = dirs;
    Q.status = status; Q.steps = steps; Q.t = t; Q.position = position; Q.normal = normal;
    const size_t N = (size_t)n;
    // staged: the rays, then every output the caller asked for
    Staging io(loc);
    io.in(Q.origins, 3 * N); io.in(Q.dirs, 3 * N);
    io.out(Q.status, N); io.out(Q.steps, N); io.out(Q.t, N); io.out(Q.position, 3 * N); io.out(Q.normal, 3 * N);
    int rc;
    if ((rc = io.begin(c, c->d_qio, c->cap_qio, s)) != NR_OK) return rc;
    HIPCHK(c, hipEventRecord(c->ev0, s));
    HIPCHK(c, hipMemsetAsync(c->d_qs, 0, CURSOR_STATS_BYTES, s));
    HIPCHK(c, launch_query(Q, c->mlp16, query_grid(c, N), s));
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if ((rc = io.end(c, s)) != NR_OK) return rc;
    unsigned long long hs[4];
    if (stats) HIPCHK(c, hipMemcpyAsync(hs, Q.stats, sizeof hs, hipMemcpyDeviceToHost, s));
    rc = end_timed(c, stats != nullptr, loc, s, &st.ms_total);
    if (rc != NR_OK || !stats) return rc;
    st.ray_steps = hs[0];
    st.rays_hit = hs[1];
    st.iterations = (int32_t)hs[2];
    st.rays_shaded = hs[3];
    st.shade_evals = normal ? 4ull * hs[3] : 0ull;
    st.launches = 2;
    *stats = st;
    return NR_OK;
}

// ---- ambient occlusion and soft shadows (nr_light.hip) ----

namespace nr {

// The checks on the fields of a light, shared by nr_render_lit and nr_compose_render_lit.
int check_light(nr_ctx *c, const char *fn, const nr_light &l) {
    const float lf[8] = {l.dir[0], l.dir[1], l.dir[2], l.shadow_bias, l.shadow_k, l.ao_step, l.ao_strength, l.ambient};
    for (float v : lf)
        if (!std::isfinite(v)) return set_err(c, NR_E_INVALID, "%s: a non-finite light field", fn);
    if (l.dir[0] == 0.0f && l.dir[1] == 0.0f && l.dir[2] == 0.0f) return set_err(c, NR_E_INVALID, "%s: dir is zero", fn);
    if (l.shadow_steps < 0) return set_err(c, NR_E_INVALID, "%s: shadow_steps < 0", fn);
    if (l.shadow_k < 0.0f || l.ao_step < 0.0f || l.ao_strength < 0.0f)
        return set_err(c, NR_E_INVALID, "%s: negative shadow_k, ao_step or ao_strength", fn);
    if (l.ambient < 0.0f || l.ambient > 1.0f) return set_err(c, NR_E_INVALID, "%s: ambient outside 0..1", fn);
    return NR_OK;
}

}  // namespace nr

extern "C" {

int nr_trace_rays(nr_ctx *c, const float *origins, const float *dirs, long n, int max_steps, int32_t *status,
                  int32_t *steps, float *t, float *position, float *normal, int loc, nr_stats *stats) {
    if (!c) return set_err(nullptr, NR_E_INVALID, "nr_trace_rays: ctx is NULL");
    if (n < 0 || n > (1l << 30)) return set_err(c, NR_E_INVALID, "nr_trace_rays: n = %ld outside [0, 2^30]", n);
    if (max_steps < 1) return set_err(c, NR_E_INVALID, "nr_trace_rays: max_steps < 1");
    if (n > 0 && (!origins || !dirs)) return set_err(c, NR_E_INVALID, "nr_trace_rays: NULL rays");
    return query_rays(c, "nr_trace_rays", origins, dirs, n, 1, 1, max_steps, status, steps, t, position, normal, loc, stats);
}

int nr_render_gbuffer(nr_ctx *c, int W, int H, int max_steps, int32_t *status, int32_t *steps, float *t, float *position,
                      float *normal, int loc, nr_stats *stats) {
    if (!c) return set_err(nullptr, NR_E_INVALID, "nr_render_gbuffer: ctx is NULL");
    if (W < 1 || H < 1 || (long)W * H > (1l << 30)) return set_err(c, NR_E_INVALID, "nr_render_gbuffer: bad size %dx%d", W, H);
    if (max_steps < 1) return set_err(c, NR_E_INVALID, "nr_render_gbuffer: max_steps < 1");
    return query_rays(c, "nr_render_gbuffer", nullptr, nullptr, (long)W * H, W, H, max_steps, status, steps, t, position,
                      normal, loc, stats);
}

// Three launches on the context's stream: the geometry buffer (k_query<true>) into context scratch,
// k_light_trace over its pixels (ao and shadow), k_light_resolve where a frame is wanted.  No
// host read in between: the tracer's cursor runs over all pixels, not over a list of the hits.
int nr_render_lit(nr_ctx *c, uint32_t *out, int W, int H, int max_steps, const nr_light *light, float *ao, float *shadow,
                  int loc, nr_stats *stats) {
    if (!c || !light) return set_err(c, NR_E_INVALID, "nr_render_lit: NULL argument");
    if (!out && !ao && !shadow) return set_err(c, NR_E_INVALID, "nr_render_lit: no output wanted");
    int rc;
    if ((rc = check_shape(c, W, H, H > 0 ? H : 1, 1, 0, max_steps)) != NR_OK) return rc;
    if ((long)W * H > (1l << 30)) return set_err(c, NR_E_INVALID, "nr_render_lit: bad size %dx%d", W, H);
    if (max_steps < 1) return set_err(c, NR_E_INVALID, "nr_render_lit: max_steps < 1");
    const nr_light &l = *light;
    if ((rc = check_light(c, "nr_render_lit", l)) != NR_OK) return rc;
    if (c->dims.empty()) return set_err(c, NR_E_STATE, "nr_render_lit: no network loaded");
    if (!c->fused)
        return set_err(c, NR_E_FORMAT, "nr_render_lit: needs a [3|4, 32, ..., 32, 1] network (no layered fallback)");
    if ((rc = check_scene(c)) != NR_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    const size_t N = (size_t)W * H;
    const bool host = loc != NR_DEVICE;
    // ---- scratch: the geometry buffer, the values without a device buffer of the caller's, the frame's staging
    if (!c->d_qs) HIPCHK(c, hipMalloc(&c->d_qs, CURSOR_STATS_BYTES));
    if (!c->d_ls) HIPCHK(c, hipMalloc(&c->d_ls, CURSOR_STATS_BYTES));
    if ((rc = ensure_buf(c, c->d_lgbuf, c->cap_lgbuf, 7 * N)) != NR_OK) return rc;
    float *d_ao = host ? nullptr : ao, *d_shadow = host ? nullptr : shadow;
    if ((rc = ensure_buf(c, c->d_lao, c->cap_lao, (d_ao ? 0 : N) + (d_shadow ? 0 : N))) != NR_OK) return rc;
    if (!d_shadow) d_shadow = c->d_lao;
    if (!d_ao) d_ao = d_shadow == c->d_lao ? c->d_lao + N : c->d_lao;
    uint32_t *dout = out;
    if (out && host) {
        if ((rc = ensure_buf(c, c->d_out, c->cap_out, N)) != NR_OK) return rc;
        dout = c->d_out;
    }
    // ---- pass A: the geometry buffer
    QueryArgs Q = query_args(c, (long)N, W, H, max_steps);
    Q.status = reinterpret_cast<int32_t *>(c->d_lgbuf);
    Q.position = c->d_lgbuf + N;
    Q.normal = c->d_lgbuf + 4 * N;
    // ---- pass B: ao and shadow of every pixel
    LightArgs X{};
    X.n = (long)N; X.scene = c->scene; X.frame = c->frame;
    X.status = Q.status; X.position = Q.position; X.normal = Q.normal;
    for (int a = 0; a < 3; ++a) X.dir[a] = l.dir[a];
    X.shadow_steps = l.shadow_steps; X.shadow_bias = l.shadow_bias; X.shadow_k = l.shadow_k;
    X.ao_step = l.ao_step; X.ao_strength = l.ao_strength; X.ambient = l.ambient;
    X.ao = d_ao; X.shadow = d_shadow;
    X.cursor = c->d_ls;
    X.stats = reinterpret_cast<unsigned long long *>(c->d_ls + 32);
    const int grid = query_grid(c, N);
    nr_stats st{};
    HIPCHK(c, hipEventRecord(c->ev0, s));
    HIPCHK(c, hipMemsetAsync(c->d_qs, 0, CURSOR_STATS_BYTES, s));
    HIPCHK(c, launch_query(Q, c->mlp16, grid, s));
    HIPCHK(c, hipMemsetAsync(c->d_ls, 0, CURSOR_STATS_BYTES, s));
    HIPCHK(c, launch_light_trace(X, c->mlp16, grid, s));
    st.launches = 4;
    if (out) {
        // ---- pass C: the base colour times the light
        RenderArgs A = render_args(c, W, H, H, H, 1, 0, max_steps);
        A.out = dout;
        A.frame = c->frame;
        memcpy(A.inv_view, c->inv_view, sizeof A.inv_view);
        memcpy(A.normal, c->normal, sizeof A.normal);
        HIPCHK(c, launch_light_resolve(A, X, s));
        st.launches += 1;
    }
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if (host) {
        if (out) HIPCHK(c, hipMemcpyAsync(out, dout, N * 4, hipMemcpyDeviceToHost, s));
        if (ao) HIPCHK(c, hipMemcpyAsync(ao, d_ao, N * 4, hipMemcpyDeviceToHost, s));
        if (shadow) HIPCHK(c, hipMemcpyAsync(shadow, d_shadow, N * 4, hipMemcpyDeviceToHost, s));
    }
    unsigned long long hq[4], hl[2];
    if (stats) {
        HIPCHK(c, hipMemcpyAsync(hq, Q.stats, sizeof hq, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(hl, X.stats, sizeof hl, hipMemcpyDeviceToHost, s));
    }
    rc = end_timed(c, stats != nullptr, loc, s, &st.ms_total);
    if (rc != NR_OK || !stats) return rc;
    st.ray_steps = hq[0] + hl[0];
    st.rays_hit = hq[1];
    st.iterations = (int32_t)std::max(hq[2], hl[1]);
    st.rays_shaded = hq[3];
    st.shade_evals = (l.ao_strength > 0.0f ? 8ull : 4ull) * hq[3];
    *stats = st;
    return NR_OK;
}

int nr_mlp_forward(nr_ctx *c, const float *X, float *Y, long n, int loc) {
    if (!c || (n > 0 && (!X || !Y)) || n < 0) return set_err(c, NR_E_INVALID, "nr_mlp_forward: bad arguments");
    if (c->dims.empty()) return set_err(c, NR_E_STATE, "nr_mlp_forward: no network loaded");
    if (n == 0) return NR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int nl = (int)c->dims.size() - 1, in0 = c->dims[0], outn = c->dims[nl];
    GET_STREAM(c, s);
    const float *dX = X;
    float *dY = Y;
    int rc;
    int maxw = *std::max_element(c->dims.begin(), c->dims.end());
    // the generic chain runs in chunks of at most 64 MiB of activations per buffer
    const long chunk = std::min<long>(n, std::max<long>(16384, (64l << 20) / (4l * maxw)));
    // one allocation: the staged points and results, then the generic chain's two buffers
    Staging io(loc);
    io.in(dX, (size_t)n * in0); io.out(dY, (size_t)n * outn);
    if ((rc = io.begin(c, c->d_io, c->cap_io, s, c->fused ? 0 : (size_t)2 * chunk * maxw)) != NR_OK) return rc;
    float *scratch = c->d_io + io.words;
    if (c->fused) {
        // workgroups per CU: 8 (queued beyond the resident ones, they keep every SIMD fed
        // to the end of the batch): 2^24 points fp32 0.796 -> 0.825 of peak, bf16 (102 VGPRs,
        // 5 waves per SIMD resident) 0.352 -> 0.410 against 4 (profiles/r2_mlp_microbench.txt)
        // 12 workgroups per CU by default: more than fit at once (3-5), so that workgroups start
        // staggered as earlier ones retire -- a grid of exactly the resident workgroups runs the
        // bf16 MLP 17 % slower (its waves stay in step: profiles/r3_mlp_bpc.txt)
        // (a per-CU LDS chunk queue balanced the SIMD's waves but left the kernel time unchanged,
        // round 4: profiles/r4_mlp_ab.txt)
        const MlpArgs M = c->mlp16;
        const int bpc = c->blocks_per_cu > 0 ? c->blocks_per_cu : 12;
        const int grid = num_cus(c->device) * bpc;
        if (c->debug & 64)  // diagnostic: n = repetitions, X >= 64 points, Y >= 65 floats
            HIPCHK(c, launch_mlp_latency(c->mlp16, c->precision, dX, dY, (int)n,
                                         ((c->wave_rays > 0 ? c->wave_rays : 64) + 15) / 16,
                                         ((c->debug >> 7) & 1) | (((c->debug >> 13) & 3) << 1), s));
            // (bf16/fp16: wave_rays 16 / 32 time the tracer's 64-point form on 1 / 2 32-point tiles,
            // otherwise the 128-point form)
        else
            HIPCHK(c, launch_mlp16(M, c->precision, dX, dY, n, grid, s));
    } else {
        float *bufs[2] = {scratch, scratch + (size_t)chunk * maxw};
        const int cus = num_cus(c->device);
        for (long p0 = 0; p0 < n; p0 += chunk) {
            const long m = std::min(chunk, n - p0);
            const float *a = dX + (size_t)p0 * in0;
            for (int l = 0; l < nl; ++l) {
                float *z = (l == nl - 1) ? dY + (size_t)p0 * outn : bufs[l & 1];
                HIPCHK(c, dense_rows(c->d_W[l], c->d_b[l], a, z, m, c->dims[l], c->dims[l + 1], l != nl - 1, cus, s));
                a = z;
            }
        }
    }
    if ((rc = io.end(c, s)) != NR_OK) return rc;
    if (loc != NR_DEVICE) HIPCHK(c, hipStreamSynchronize(s));
    return NR_OK;
}

// The analytic gradient: one k_grad launch (nr_grad.hip).  Always the fp32 MLP.
constexpr int GRAD_BPC = 12;  // workgroups per CU of its grid by default
int nr_mlp_gradient(nr_ctx *c, const float *X, long n, float *value, float *grad, float *normal, int loc,
                    nr_stats *stats) {
    if (!c) return set_err(nullptr, NR_E_INVALID, "nr_mlp_gradient: ctx is NULL");
    if (n < 0 || n > (1l << 30)) return set_err(c, NR_E_INVALID, "nr_mlp_gradient: n = %ld outside [0, 2^30]", n);
    if (n > 0 && !X) return set_err(c, NR_E_INVALID, "nr_mlp_gradient: X is NULL");
    if (!value && !grad && !normal) return set_err(c, NR_E_INVALID, "nr_mlp_gradient: every output is NULL");
    if (c->dims.empty()) return set_err(c, NR_E_STATE, "nr_mlp_gradient: no network loaded");
    if (!c->fused)
        return set_err(c, NR_E_FORMAT, "nr_mlp_gradient: needs a [3|4, 32, ..., 32, 1] network (no layered fallback)");
    if (!c->d_gpack16)
        return set_err(c, NR_E_FORMAT, "nr_mlp_gradient: more than %d hidden 32 x 32 layers", GRAD_MAX_HIDDEN);
    nr_stats st{};
    if (n == 0) { if (stats) *stats = st; return NR_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    const size_t N = (size_t)n, in0 = (size_t)c->dims[0];
    GradArgs G{};
    G.X = X; G.n = n;
    G.value = value; G.grad = grad; G.normal = normal;
    G.gb = c->d_gpack16; G.gb_bytes = c->gpack_bytes;
    // staged: the points, then every output the caller asked for
    Staging io(loc);
    io.in(G.X, N * in0);
    io.out(G.value, N); io.out(G.grad, N * in0); io.out(G.normal, 3 * N);
    int rc;
    if ((rc = io.begin(c, c->d_io, c->cap_io, s)) != NR_OK) return rc;
    const MlpArgs M = c->mlp16;
    if (grad_lds_bytes(M, G) > 64 * 1024) return set_err(c, NR_E_FORMAT, "nr_mlp_gradient: the packs exceed 64 KB of LDS");
    // two workgroups per CU are resident (their LDS: the two packs); the grid by the CU count:
    // nr_set_occupancy's workgroups per CU, or GRAD_BPC
    const int grid = persistent_grid(c, N, 256, GRAD_BPC);
    HIPCHK(c, hipEventRecord(c->ev0, s));
    HIPCHK(c, launch_grad(G, M, grid, s));
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if ((rc = io.end(c, s)) != NR_OK) return rc;
    st.ray_steps = (uint64_t)n;
    st.launches = 1;
    rc = end_timed(c, stats != nullptr, loc, s, &st.ms_total);
    if (rc == NR_OK && stats) *stats = st;
    return rc;
}

// Projection onto a level set: one persistent k_project launch (nr_project.hip).  Always the fp32 MLP.
#ifndef NR_PROJ_COMPACT
#define NR_PROJ_COMPACT 1  // pack a draining wave's live points into its lowest tiles (0: A/B builds)
#endif
int nr_project_points(nr_ctx *c, const float *X, long n, const nr_project_opts *opts, float *position, float *value,
                      float *normal, float *distance, int32_t *iters, int32_t *status, int loc, nr_stats *stats) {
    if (!c) return set_err(nullptr, NR_E_INVALID, "nr_project_points: ctx is NULL");
    if (!opts) return set_err(c, NR_E_INVALID, "nr_project_points: opts is NULL");
    if (n < 0 || n > (1l << 30)) return set_err(c, NR_E_INVALID, "nr_project_points: n = %ld outside [0, 2^30]", n);
    if (n > 0 && !X) return set_err(c, NR_E_INVALID, "nr_project_points: X is NULL");
    if (!position && !value && !normal && !distance && !iters && !status)
        return set_err(c, NR_E_INVALID, "nr_project_points: every output is NULL");
    if (!std::isfinite(opts->iso) || !std::isfinite(opts->tol) || !std::isfinite(opts->max_step))
        return set_err(c, NR_E_INVALID, "nr_project_points: iso, tol and max_step must be finite");
    if (opts->tol < 0.0f || opts->max_step < 0.0f)
        return set_err(c, NR_E_INVALID, "nr_project_points: tol = %g or max_step = %g is negative", opts->tol, opts->max_step);
    if (opts->max_iters < 0 || opts->max_iters > 4096)
        return set_err(c, NR_E_INVALID, "nr_project_points: max_iters = %d outside 0..4096", opts->max_iters);
    if (c->dims.empty()) return set_err(c, NR_E_STATE, "nr_project_points: no network loaded");
    if (!c->fused)
        return set_err(c, NR_E_FORMAT, "nr_project_points: needs a [3|4, 32, ..., 32, 1] network (no layered fallback)");
    if (!c->d_gpack16)
        return set_err(c, NR_E_FORMAT, "nr_project_points: more than %d hidden 32 x 32 layers", GRAD_MAX_HIDDEN);
    nr_stats st{};
    if (n == 0) { if (stats) *stats = st; return NR_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    if (!c->d_ps) HIPCHK(c, hipMalloc(&c->d_ps, CURSOR_STATS_BYTES));
    const size_t N = (size_t)n, in0 = (size_t)c->dims[0];
    ProjArgs A{};
    A.X = X; A.n = n;
    A.iso = opts->iso; A.tol = opts->tol; A.max_step = opts->max_step; A.max_iters = opts->max_iters;
    A.position = position; A.value = value; A.normal = normal; A.distance = distance;
    A.iters = iters; A.status = status;
    A.gb = c->d_gpack16; A.gb_bytes = c->gpack_bytes;
    A.compact = NR_PROJ_COMPACT;
    A.cursor = c->d_ps;
    A.stats = reinterpret_cast<unsigned long long *>(c->d_ps + 32);
    // staged: the points, then every output the caller asked for
    Staging io(loc);
    io.in(A.X, N * in0);
    io.out(A.position, 3 * N); io.out(A.value, N); io.out(A.normal, 3 * N); io.out(A.distance, N);
    io.out(A.iters, N); io.out(A.status, N);
    int rc;
    if ((rc = io.begin(c, c->d_io, c->cap_io, s)) != NR_OK) return rc;
    const MlpArgs M = c->mlp16;
    if (project_lds_bytes(M, A) > 64 * 1024)
        return set_err(c, NR_E_FORMAT, "nr_project_points: the packs exceed 64 KB of LDS");
    // two workgroups per CU are resident (their LDS: the two packs), and the launch is persistent:
    // nr_set_occupancy's workgroups per CU, or the resident two
    const int grid = persistent_grid(c, N, 256, 2);
    HIPCHK(c, hipEventRecord(c->ev0, s));
    HIPCHK(c, hipMemsetAsync(c->d_ps, 0, CURSOR_STATS_BYTES, s));
    HIPCHK(c, launch_project(A, M, grid, s));
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if ((rc = io.end(c, s)) != NR_OK) return rc;
    unsigned long long hs[3];
    if (stats) HIPCHK(c, hipMemcpyAsync(hs, A.stats, sizeof hs, hipMemcpyDeviceToHost, s));
    rc = end_timed(c, stats != nullptr, loc, s, &st.ms_total);
    if (rc != NR_OK || !stats) return rc;
    st.ray_steps = hs[0];
    st.rays_shaded = hs[1];
    st.iterations = (int32_t)hs[2];
    st.launches = 2;  // the counters' memset and k_project
    *stats = st;
    return NR_OK;
}

int nr_layer_forward(nr_ctx *c, int layer, const float *A, float *Z, long n, int loc) {
    if (!c || n < 0 || (n > 0 && (!A || !Z))) return set_err(c, NR_E_INVALID, "nr_layer_forward: bad arguments");
    int nl = c->dims.empty() ? 0 : (int)c->dims.size() - 1;
    if (layer < 0 || layer >= nl) return set_err(c, NR_E_INVALID, "nr_layer_forward: layer %d out of range", layer);
    if (n == 0) return NR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int in = c->dims[layer], out = c->dims[layer + 1];
    GET_STREAM(c, s);
    Staging io(loc);
    io.in(A, (size_t)n * in); io.out(Z, (size_t)n * out);
    int rc;
    if ((rc = io.begin(c, c->d_io, c->cap_io, s)) != NR_OK) return rc;
    HIPCHK(c, dense_rows(c->d_W[layer], c->d_b[layer], A, Z, n, in, out, layer != nl - 1, num_cus(c->device), s));
    if ((rc = io.end(c, s)) != NR_OK) return rc;
    if (loc != NR_DEVICE) HIPCHK(c, hipStreamSynchronize(s));
    return NR_OK;
}

int nr_dense_forward(nr_ctx *c, const float *W, const float *b, int in, int out, int relu, const float *A, float *Z,
                     long n, int loc) {
    if (!c || !W || !b || in < 1 || out < 1 || n < 0 || (n > 0 && (!A || !Z)))
        return set_err(c, NR_E_INVALID, "nr_dense_forward: bad arguments");
    if (n == 0) return NR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    // host buffers: stage everything
    Staging io(loc);
    io.in(W, (size_t)in * out); io.in(b, (size_t)out); io.in(A, (size_t)n * in); io.out(Z, (size_t)n * out);
    int rc;
    if ((rc = io.begin(c, c->d_io, c->cap_io, s)) != NR_OK) return rc;
    HIPCHK(c, dense_rows(W, b, A, Z, n, in, out, relu, num_cus(c->device), s));
    if ((rc = io.end(c, s)) != NR_OK) return rc;
    if (loc != NR_DEVICE) HIPCHK(c, hipStreamSynchronize(s));
    return NR_OK;
}

}  // extern "C"
