// nr_api_compose.hip -- the C ABI's composed scenes (nr_compose_*; nr_compose.hip, nr_compose_light.hip,
// nr_compose_mesh.hip): several networks, placed and combined, traced, lit, sampled and meshed at once.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

#include "nr_ctx.h"

using namespace nr;

// ---- composed scenes (nr_compose.hip) ----

struct nr_compose {
    nr_ctx *owner = nullptr;
    float *d_packs = nullptr;
    ComposeArgs A{};              // packs, nets, parts and the bound; the per-call fields are filled per call
    int npacks = 0;               // distinct packs in d_packs
    float center[3] = {0, 0, 0}, radius = 0;
    // the ray cursor on its own 128-byte line + 7 x u64 stats; staging of host rays, points and results;
    // the frame's geometry buffer (status, normal: 16 B per pixel) and its staging
    uint32_t *d_cs = nullptr;
    float *d_io = nullptr;
    size_t cap_io = 0;
    float *d_gbuf = nullptr;
    size_t cap_gbuf = 0;
    uint32_t *d_out = nullptr;
    size_t cap_out = 0;
    // nr_compose_render_lit: the lighting launch's cursor and stats (as d_cs), its geometry buffer
    // (status, position, normal: 28 B per pixel), ao and shadow where the caller gave no device
    // buffer, and the staging of a host part and occluder
    uint32_t *d_ls = nullptr;
    float *d_lgbuf = nullptr;
    size_t cap_lgbuf = 0;
    float *d_lao = nullptr;
    size_t cap_lao = 0;
    int32_t *d_lown = nullptr;
    size_t cap_lown = 0;
};
constexpr size_t COMPOSE_CS_BYTES = 128 + 7 * 8;

extern "C" {

int nr_compose_bound(const nr_part *parts, int nparts, int nnets, float center[3], float *radius) {
    if (!parts) return set_err(nullptr, NR_E_INVALID, "nr_compose: parts is NULL");
    if (nnets < 1 || nnets > NR_COMPOSE_MAX_NETS) return set_err(nullptr, NR_E_INVALID, "nr_compose: %d nets outside 1..%d", nnets, NR_COMPOSE_MAX_NETS);
    if (nparts < 1 || nparts > NR_COMPOSE_MAX_PARTS)
        return set_err(nullptr, NR_E_INVALID, "nr_compose: %d parts outside 1..%d", nparts, NR_COMPOSE_MAX_PARTS);
    for (int j = 0; j < nparts; ++j) {
        const nr_part &p = parts[j];
        if (p.net < 0 || p.net >= nnets) return set_err(nullptr, NR_E_INVALID, "nr_compose: part %d: net %d out of range", j, p.net);
        if (p.op != NR_PART_UNION && p.op != NR_PART_SUBTRACT) return set_err(nullptr, NR_E_INVALID, "nr_compose: part %d: unknown op %d", j, p.op);
        if (j == 0 && p.op != NR_PART_UNION) return set_err(nullptr, NR_E_INVALID, "nr_compose: part 0 must be a union");
        if (!std::isfinite(p.scale) || !(p.scale > 0.0f)) return set_err(nullptr, NR_E_INVALID, "nr_compose: part %d: scale must be finite and > 0", j);
        if (!std::isfinite(1.0f / p.scale) || !std::isfinite(1.2f * p.scale))
            return set_err(nullptr, NR_E_INVALID, "nr_compose: part %d: scale out of range", j);
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(p.pos[k])) return set_err(nullptr, NR_E_INVALID, "nr_compose: part %d: non-finite position", j);
        const float *R = p.rot;
        double dev = 0.0;
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                double s = 0.0;
                for (int k = 0; k < 3; ++k) s += (double)R[3 * a + k] * (double)R[3 * b + k];
                dev = std::max(dev, std::fabs(s - (a == b ? 1.0 : 0.0)));
            }
        const double det = (double)R[0] * ((double)R[4] * R[8] - (double)R[5] * R[7]) -
                           (double)R[1] * ((double)R[3] * R[8] - (double)R[5] * R[6]) +
                           (double)R[2] * ((double)R[3] * R[7] - (double)R[4] * R[6]);
        if (!(dev <= 1e-4) || !(det >= 0.0)) return set_err(nullptr, NR_E_INVALID, "nr_compose: part %d: rot is not a rotation", j);
    }
    // the bound: the mean position, and the farthest reach of a part's sphere of radius 1.2 scale
    float c[3];
    for (int k = 0; k < 3; ++k) {
        double s = 0.0;
        for (int j = 0; j < nparts; ++j) s += (double)parts[j].pos[k];
        c[k] = (float)(s / (double)nparts);
    }
    double rd = 0.0;
    for (int j = 0; j < nparts; ++j) {
        double q = 0.0;
        for (int k = 0; k < 3; ++k) {
            const double t = (double)parts[j].pos[k] - (double)c[k];
            q += t * t;
        }
        rd = std::max(rd, std::sqrt(q) * (1.0 + 0x1p-20) + (double)(1.2f * parts[j].scale));
    }
    float r = (float)rd;
    if ((double)r < rd) r = std::nextafterf(r, INFINITY);
    if (!std::isfinite(r) || !std::isfinite(r * r)) return set_err(nullptr, NR_E_INVALID, "nr_compose: the bound is not finite");
    if (center) for (int k = 0; k < 3; ++k) center[k] = c[k];
    if (radius) *radius = r;
    return NR_OK;
}

// the parts and their bound into the composition (validated first: nothing changes on an error)
static int compose_set(nr_compose *cp, const nr_part *parts, int nparts) {
    float c[3], r;
    const int rc = nr_compose_bound(parts, nparts, cp->A.nnets, c, &r);
    if (rc != NR_OK) { cp->owner->err = nr_last_error(nullptr); return rc; }
    ComposeArgs &A = cp->A;
    A.nparts = nparts;
    for (int j = 0; j < nparts; ++j) {
        ComposePart &P = A.parts[j];
        memcpy(P.rot, parts[j].rot, sizeof P.rot);
        memcpy(P.pos, parts[j].pos, sizeof P.pos);
        P.scale = parts[j].scale;
        P.inv_s = 1.0f / parts[j].scale;
        P.net = parts[j].net;
        P.op = parts[j].op;
    }
    for (int k = 0; k < 3; ++k) { cp->center[k] = c[k]; A.center[k] = c[k]; }
    cp->radius = r;
    A.r2 = r * r;
    return NR_OK;
}

int nr_compose_create(nr_ctx *owner, nr_ctx *const *nets, int nnets, const nr_part *parts, int nparts, nr_compose **out) {
    if (out) *out = nullptr;
    if (!owner || !nets || !parts || !out) return set_err(owner, NR_E_INVALID, "nr_compose_create: NULL argument");
    if (nnets < 1 || nnets > NR_COMPOSE_MAX_NETS)
        return set_err(owner, NR_E_INVALID, "nr_compose_create: %d nets outside 1..%d", nnets, NR_COMPOSE_MAX_NETS);
    int rc;
    if ((rc = nr_compose_bound(parts, nparts, nnets, nullptr, nullptr)) != NR_OK) { owner->err = nr_last_error(nullptr); return rc; }
    size_t total = 0;
    int npacks = 0;
    ComposeNet cn[NR_COMPOSE_MAX_NETS];
    for (int i = 0; i < nnets; ++i) {
        const nr_ctx *s = nets[i];
        if (!s) return set_err(owner, NR_E_INVALID, "nr_compose_create: net %d is NULL", i);
        if (s->dims.empty()) return set_err(owner, NR_E_STATE, "nr_compose_create: net %d has no network", i);
        if (!s->fused || !s->d_pack16)
            return set_err(owner, NR_E_FORMAT, "nr_compose_create: net %d is not a [3|4, 32, ..., 32, 1] network (no fp32 pack)", i);
        if (s->device != owner->device) return set_err(owner, NR_E_INVALID, "nr_compose_create: net %d lives on device %d, the owner on %d", i, s->device, owner->device);
        int same = -1;
        for (int k = 0; k < i && same < 0; ++k)
            if (nets[k] == nets[i]) same = k;
        cn[i].off = same >= 0 ? cn[same].off : (int)(total / 4);
        cn[i].in0 = s->mlp16.in0;
        cn[i].nh = s->mlp16.nh;
        cn[i].f32_clamp = s->mlp16.f32_clamp;
        if (same < 0) { total += (size_t)s->mlp16.pk_bytes; ++npacks; }
    }
    // every workgroup shape the launches use must fit a CU's LDS: the packs and four waves' lists
    // at the least, twelve waves' for more than one pack (compose_threads)
    ComposeArgs probe{};
    probe.pack_bytes = (int)total;
    const int threads = npacks > 1 ? 768 : 256;
    if (total > (size_t)NR_LDS_PER_CU || compose_lds_bytes(probe, threads) > NR_LDS_PER_CU)
        return set_err(owner, NR_E_INVALID, "nr_compose_create: the packs need %zu bytes of LDS (limit %d with the per-wave lists)", total, NR_LDS_PER_CU);
    nr_compose *cp = new (std::nothrow) nr_compose();
    if (!cp) return set_err(owner, NR_E_NOMEM, "out of host memory");
    cp->owner = owner;
    cp->npacks = npacks;
    cp->A.nnets = nnets;
    cp->A.pack_bytes = (int)total;
    for (int i = 0; i < nnets; ++i) cp->A.nets[i] = cn[i];
    if ((rc = compose_set(cp, parts, nparts)) != NR_OK) { delete cp; return rc; }
    hipError_t e = hipSetDevice(owner->device);
    if (e == hipSuccess) e = hipMalloc(&cp->d_packs, total);
    if (e == hipSuccess) e = hipMalloc(&cp->d_cs, COMPOSE_CS_BYTES);
    for (int i = 0; i < nnets && e == hipSuccess; ++i) {
        // (a blocking copy: the source may be destroyed as soon as this returns)
        bool first = true;
        for (int k = 0; k < i; ++k) first = first && nets[k] != nets[i];
        if (first) e = hipMemcpy(cp->d_packs + cn[i].off, nets[i]->d_pack16, (size_t)nets[i]->mlp16.pk_bytes, hipMemcpyDeviceToDevice);
    }
    if (e != hipSuccess) {
        dfree(cp->d_packs); dfree(cp->d_cs);
        delete cp;
        return set_err(owner, NR_E_HIP, "nr_compose_create: %s", hipGetErrorString(e));
    }
    cp->A.packs = cp->d_packs;
    *out = cp;
    return NR_OK;
}

int nr_compose_destroy(nr_compose *cp) {
    if (!cp) return NR_OK;
    nr_ctx *c = cp->owner;
    (void)hipSetDevice(c->device);
    if (!(c->use_own && !c->own_stream)) (void)hipStreamSynchronize(c->stream);
    dfree(cp->d_packs); dfree(cp->d_cs); dfree(cp->d_io); dfree(cp->d_gbuf); dfree(cp->d_out);
    dfree(cp->d_ls); dfree(cp->d_lgbuf); dfree(cp->d_lao); dfree(cp->d_lown);
    delete cp;
    return NR_OK;
}

int nr_compose_set_parts(nr_compose *cp, const nr_part *parts, int nparts) {
    if (!cp) return set_err(nullptr, NR_E_INVALID, "nr_compose_set_parts: composition is NULL");
    return compose_set(cp, parts, nparts);
}

int nr_compose_info(const nr_compose *cp, int *nnets, int *nparts, float center[3], float *radius) {
    if (!cp) return set_err(nullptr, NR_E_INVALID, "nr_compose_info: composition is NULL");
    if (nnets) *nnets = cp->A.nnets;
    if (nparts) *nparts = cp->A.nparts;
    if (center) for (int k = 0; k < 3; ++k) center[k] = cp->center[k];
    if (radius) *radius = cp->radius;
    return NR_OK;
}

// The workgroup of a k_compose launch and the grid: one pack keeps k_query's shape (4 waves, two
// workgroups per CU by default, as query_grid); more packs leave room for one or two workgroups
// per CU, so one of 12 waves holds three waves per SIMD.  nr_set_occupancy on the owner asks for
// that many 4-wave workgroups per CU instead, as far as the LDS allows.
static void compose_shape(const nr_compose *cp, size_t n, int &threads, int &grid) {
    const nr_ctx *c = cp->owner;
    const bool one = cp->npacks == 1;
    int bpc;
    if (c->blocks_per_cu > 0 || one) {
        threads = 256;
        const int fit = std::max(1, NR_LDS_PER_CU / compose_lds_bytes(cp->A, threads));
        bpc = std::min(c->blocks_per_cu > 0 ? c->blocks_per_cu : 2, fit);
    } else {
        threads = 768;
        bpc = 1;
    }
    grid = (int)std::max<size_t>(1, std::min<size_t>((n + threads - 1) / threads, (size_t)num_cus(c->device) * bpc));
}

static void compose_stats(const unsigned long long *hs, bool normals, int launches, float ms, nr_compose_stats *stats) {
    nr_compose_stats st{};
    st.ray_steps = hs[0];
    st.rays_hit = hs[1];
    st.iterations = (int32_t)hs[2];
    st.rays_shaded = hs[3];
    st.shade_evals = normals ? 4ull * hs[3] : 0ull;
    st.part_evals = hs[4];
    st.wave_evals = hs[5];
    st.wave_skips = hs[6];
    st.launches = launches;
    st.ms_total = ms;
    *stats = st;
}

// n caller-supplied rays, or with origins == NULL the W x H pixel rays of the owner's view, through
// one k_compose launch; with `out` the colouring launch follows (nr_compose_render: status and normal
// then live in the composition's geometry buffer).
static int compose_rays(nr_compose *cp, const char *fn, const float *origins, const float *dirs, long n, int W, int H,
                        int max_steps, int32_t *status, int32_t *steps, float *t, float *position, float *normal,
                        int32_t *part, uint32_t *out, int loc, nr_compose_stats *stats) {
    nr_ctx *c = cp->owner;
    if (n == 0) { if (stats) *stats = nr_compose_stats{}; return NR_OK; }
    if (out && c->color_type == NR_COLOR_MATCAP && !c->d_matcap) return set_err(c, NR_E_STATE, "%s: matcap colouring without a matcap", fn);
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    ComposeArgs Q = cp->A;
    Q.n = n; Q.W = W; Q.H = H;
    Q.inv_w = 1.0 / (double)W;
    Q.rcp_w = pow2_rcp(W); Q.rcp_h = pow2_rcp(H);
    memcpy(Q.inv_view, c->inv_view, sizeof Q.inv_view);
    Q.max_steps = max_steps; Q.frame = c->frame;
    Q.cursor = cp->d_cs;
    Q.stats = reinterpret_cast<unsigned long long *>(cp->d_cs + 32);
    Q.origins = origins; Q.dirs = dirs;
    Q.status = status; Q.steps = steps; Q.t = t; Q.position = position; Q.normal = normal; Q.part = part;
    const size_t N = (size_t)n;
    const bool host = loc != NR_DEVICE;
    int rc;
    // staged: the rays, then every output the caller asked for
    Staging io(loc);
    io.in(Q.origins, 3 * N); io.in(Q.dirs, 3 * N);
    io.out(Q.status, N); io.out(Q.steps, N); io.out(Q.t, N); io.out(Q.position, 3 * N); io.out(Q.normal, 3 * N);
    io.out(Q.part, N);
    if ((rc = io.begin(c, cp->d_io, cp->cap_io, s)) != NR_OK) return rc;
    uint32_t *dout = out;
    if (out) {
        if ((rc = ensure_buf(c, cp->d_gbuf, cp->cap_gbuf, 4 * N)) != NR_OK) return rc;
        Q.status = reinterpret_cast<int32_t *>(cp->d_gbuf);
        Q.normal = cp->d_gbuf + N;
        if (host) {
            if ((rc = ensure_buf(c, cp->d_out, cp->cap_out, N)) != NR_OK) return rc;
            dout = cp->d_out;
        }
    }
    int threads, grid;
    compose_shape(cp, N, threads, grid);
    HIPCHK(c, hipEventRecord(c->ev0, s));
    HIPCHK(c, hipMemsetAsync(cp->d_cs, 0, COMPOSE_CS_BYTES, s));
    HIPCHK(c, launch_compose(Q, grid, threads, s));
    int launches = 2;
    if (out) {
        RenderArgs A = render_args(c, W, H, H, H, 1, 0, max_steps);
        A.out = dout;
        A.frame = c->frame;
        memcpy(A.inv_view, c->inv_view, sizeof A.inv_view);
        memcpy(A.normal, c->normal, sizeof A.normal);
        HIPCHK(c, launch_compose_color(A, Q.status, Q.normal, s));
        launches += 1;
    }
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if ((rc = io.end(c, s)) != NR_OK) return rc;
    if (host && out) HIPCHK(c, hipMemcpyAsync(out, dout, N * 4, hipMemcpyDeviceToHost, s));
    unsigned long long hs[7];
    if (stats) HIPCHK(c, hipMemcpyAsync(hs, Q.stats, sizeof hs, hipMemcpyDeviceToHost, s));
    float ms = 0.0f;
    rc = end_timed(c, stats != nullptr, loc, s, &ms);
    if (rc != NR_OK || !stats) return rc;
    compose_stats(hs, Q.normal != nullptr, launches, ms, stats);
    return NR_OK;
}

int nr_compose_trace_rays(nr_compose *cp, const float *origins, const float *dirs, long n, int max_steps, int32_t *status,
                          int32_t *steps, float *t, float *position, float *normal, int32_t *part, int loc,
                          nr_compose_stats *stats) {
    if (!cp) return set_err(nullptr, NR_E_INVALID, "nr_compose_trace_rays: composition is NULL");
    nr_ctx *c = cp->owner;
    if (n < 0 || n > (1l << 30)) return set_err(c, NR_E_INVALID, "nr_compose_trace_rays: n = %ld outside [0, 2^30]", n);
    if (max_steps < 1) return set_err(c, NR_E_INVALID, "nr_compose_trace_rays: max_steps < 1");
    if (n > 0 && (!origins || !dirs)) return set_err(c, NR_E_INVALID, "nr_compose_trace_rays: NULL rays");
    return compose_rays(cp, "nr_compose_trace_rays", origins, dirs, n, 1, 1, max_steps, status, steps, t, position, normal,
                        part, nullptr, loc, stats);
}

int nr_compose_gbuffer(nr_compose *cp, int W, int H, int max_steps, int32_t *status, int32_t *steps, float *t, float *position,
                       float *normal, int32_t *part, int loc, nr_compose_stats *stats) {
    if (!cp) return set_err(nullptr, NR_E_INVALID, "nr_compose_gbuffer: composition is NULL");
    nr_ctx *c = cp->owner;
    if (W < 1 || H < 1 || (long)W * H > (1l << 30)) return set_err(c, NR_E_INVALID, "nr_compose_gbuffer: bad size %dx%d", W, H);
    if (max_steps < 1) return set_err(c, NR_E_INVALID, "nr_compose_gbuffer: max_steps < 1");
    return compose_rays(cp, "nr_compose_gbuffer", nullptr, nullptr, (long)W * H, W, H, max_steps, status, steps, t, position,
                        normal, part, nullptr, loc, stats);
}

int nr_compose_render(nr_compose *cp, uint32_t *out, int W, int H, int max_steps, int32_t *part, int loc,
                      nr_compose_stats *stats) {
    if (!cp) return set_err(nullptr, NR_E_INVALID, "nr_compose_render: composition is NULL");
    nr_ctx *c = cp->owner;
    if (!out) return set_err(c, NR_E_INVALID, "nr_compose_render: out is NULL");
    if (W < 1 || H < 1 || (long)W * H > (1l << 30)) return set_err(c, NR_E_INVALID, "nr_compose_render: bad size %dx%d", W, H);
    if (max_steps < 1) return set_err(c, NR_E_INVALID, "nr_compose_render: max_steps < 1");
    return compose_rays(cp, "nr_compose_render", nullptr, nullptr, (long)W * H, W, H, max_steps, nullptr, nullptr, nullptr,
                        nullptr, nullptr, part, out, loc, stats);
}

// ---- ambient occlusion and shadows of a composed scene (nr_compose_light.hip) ----

// The workgroup of a k_compose_light launch and its grid: compose_shape's choice with
// compose_light_lds_bytes in the fit test, and 768 -> 512 -> 256 threads where the two per-wave
// lists do not fit beside the packs.  false: not even four waves' lists fit.
static bool compose_light_shape(const nr_compose *cp, size_t n, int &threads, int &grid) {
    const nr_ctx *c = cp->owner;
    const bool one = cp->npacks == 1;
    int bpc = 1;
    if (c->blocks_per_cu > 0 || one) {
        threads = 256;
    } else {
        threads = 768;
        while (threads > 256 && compose_light_lds_bytes(cp->A, threads) > NR_LDS_PER_CU) threads -= 256;
    }
    const int bytes = compose_light_lds_bytes(cp->A, threads);
    if (bytes > NR_LDS_PER_CU) return false;
    if (c->blocks_per_cu > 0 || one) bpc = std::min(c->blocks_per_cu > 0 ? c->blocks_per_cu : 2, std::max(1, NR_LDS_PER_CU / bytes));
    grid = (int)std::max<size_t>(1, std::min<size_t>((n + threads - 1) / threads, (size_t)num_cus(c->device) * bpc));
    return true;
}

// Launches on the owner's stream: the geometry buffer (k_compose<true>) into the composition's
// scratch, k_compose_light over its pixels (ao, shadow, occluder), k_light_resolve where a frame is
// wanted.  No host read in between.
int nr_compose_render_lit(nr_compose *cp, uint32_t *out, int W, int H, int max_steps, const nr_light *light, float *ao,
                          float *shadow, int32_t *part, int32_t *occluder, int loc, nr_compose_stats *stats) {
    if (!cp) return set_err(nullptr, NR_E_INVALID, "nr_compose_render_lit: composition is NULL");
    nr_ctx *c = cp->owner;
    if (!light) return set_err(c, NR_E_INVALID, "nr_compose_render_lit: light is NULL");
    if (!out && !ao && !shadow) return set_err(c, NR_E_INVALID, "nr_compose_render_lit: no output wanted");
    if (W < 1 || H < 1 || (long)W * H > (1l << 30)) return set_err(c, NR_E_INVALID, "nr_compose_render_lit: bad size %dx%d", W, H);
    if (max_steps < 1) return set_err(c, NR_E_INVALID, "nr_compose_render_lit: max_steps < 1");
    const nr_light &l = *light;
    int rc;
    if ((rc = check_light(c, "nr_compose_render_lit", l)) != NR_OK) return rc;
    if (out && c->color_type == NR_COLOR_MATCAP && !c->d_matcap)
        return set_err(c, NR_E_STATE, "nr_compose_render_lit: matcap colouring without a matcap");
    const size_t N = (size_t)W * H;
    int threads, grid, lthreads, lgrid;
    compose_shape(cp, N, threads, grid);
    if (!compose_light_shape(cp, N, lthreads, lgrid))
        return set_err(c, NR_E_INVALID, "nr_compose_render_lit: the packs and the per-wave lists need %d bytes of LDS (limit %d)",
                       compose_light_lds_bytes(cp->A, 256), NR_LDS_PER_CU);
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    const bool host = loc != NR_DEVICE;
    // ---- scratch: the geometry buffer, the values without a device buffer of the caller's, the frame's staging
    if (!cp->d_ls) HIPCHK(c, hipMalloc(&cp->d_ls, COMPOSE_CS_BYTES));
    if ((rc = ensure_buf(c, cp->d_lgbuf, cp->cap_lgbuf, 7 * N)) != NR_OK) return rc;
    float *d_ao = host ? nullptr : ao, *d_shadow = host ? nullptr : shadow;
    if ((rc = ensure_buf(c, cp->d_lao, cp->cap_lao, (d_ao ? 0 : N) + (d_shadow ? 0 : N))) != NR_OK) return rc;
    if (!d_shadow) d_shadow = cp->d_lao;
    if (!d_ao) d_ao = d_shadow == cp->d_lao ? cp->d_lao + N : cp->d_lao;
    int32_t *d_part = part, *d_occ = occluder;
    if (host) {
        if ((rc = ensure_buf(c, cp->d_lown, cp->cap_lown, (part ? N : 0) + (occluder ? N : 0))) != NR_OK) return rc;
        if (part) d_part = cp->d_lown;
        if (occluder) d_occ = cp->d_lown + (part ? N : 0);
    }
    uint32_t *dout = out;
    if (out && host) {
        if ((rc = ensure_buf(c, cp->d_out, cp->cap_out, N)) != NR_OK) return rc;
        dout = cp->d_out;
    }
    // ---- pass A: the geometry buffer
    ComposeArgs Q = cp->A;
    Q.n = (long)N; Q.W = W; Q.H = H;
    Q.inv_w = 1.0 / (double)W;
    Q.rcp_w = pow2_rcp(W); Q.rcp_h = pow2_rcp(H);
    memcpy(Q.inv_view, c->inv_view, sizeof Q.inv_view);
    Q.max_steps = max_steps; Q.frame = c->frame;
    Q.cursor = cp->d_cs;
    Q.stats = reinterpret_cast<unsigned long long *>(cp->d_cs + 32);
    Q.status = reinterpret_cast<int32_t *>(cp->d_lgbuf);
    Q.position = cp->d_lgbuf + N;
    Q.normal = cp->d_lgbuf + 4 * N;
    Q.part = d_part;
    // ---- pass B: ao, shadow and occluder of every pixel
    ComposeArgs B = cp->A;
    B.n = (long)N; B.frame = c->frame;
    B.cursor = cp->d_ls;
    B.stats = reinterpret_cast<unsigned long long *>(cp->d_ls + 32);
    ComposeLightArgs X{};
    X.status = Q.status; X.position = Q.position; X.normal = Q.normal;
    for (int a = 0; a < 3; ++a) X.dir[a] = l.dir[a];
    X.shadow_steps = l.shadow_steps; X.shadow_bias = l.shadow_bias; X.shadow_k = l.shadow_k;
    X.ao_step = l.ao_step; X.ao_strength = l.ao_strength;
    X.ao = d_ao; X.shadow = d_shadow; X.occluder = d_occ;
    HIPCHK(c, hipEventRecord(c->ev0, s));
    HIPCHK(c, hipMemsetAsync(cp->d_cs, 0, COMPOSE_CS_BYTES, s));
    HIPCHK(c, launch_compose(Q, grid, threads, s));
    HIPCHK(c, hipMemsetAsync(cp->d_ls, 0, COMPOSE_CS_BYTES, s));
    HIPCHK(c, launch_compose_light(B, X, lgrid, lthreads, s));
    int launches = 4;
    if (out) {
        // ---- pass C: the base colour times the light (k_light_resolve reads these fields of LightArgs)
        LightArgs R{};
        R.n = (long)N;
        R.status = Q.status; R.normal = Q.normal;
        for (int a = 0; a < 3; ++a) R.dir[a] = l.dir[a];
        R.ambient = l.ambient;
        R.ao = d_ao; R.shadow = d_shadow;
        RenderArgs A = render_args(c, W, H, H, H, 1, 0, max_steps);
        A.out = dout;
        A.frame = c->frame;
        memcpy(A.inv_view, c->inv_view, sizeof A.inv_view);
        memcpy(A.normal, c->normal, sizeof A.normal);
        HIPCHK(c, launch_light_resolve(A, R, s));
        launches += 1;
    }
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if (host) {
        if (out) HIPCHK(c, hipMemcpyAsync(out, dout, N * 4, hipMemcpyDeviceToHost, s));
        if (ao) HIPCHK(c, hipMemcpyAsync(ao, d_ao, N * 4, hipMemcpyDeviceToHost, s));
        if (shadow) HIPCHK(c, hipMemcpyAsync(shadow, d_shadow, N * 4, hipMemcpyDeviceToHost, s));
        if (part) HIPCHK(c, hipMemcpyAsync(part, d_part, N * 4, hipMemcpyDeviceToHost, s));
        if (occluder) HIPCHK(c, hipMemcpyAsync(occluder, d_occ, N * 4, hipMemcpyDeviceToHost, s));
    }
    unsigned long long hs[7], hl[7];
    if (stats) {
        HIPCHK(c, hipMemcpyAsync(hs, Q.stats, sizeof hs, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(hl, B.stats, sizeof hl, hipMemcpyDeviceToHost, s));
    }
    float ms = 0.0f;
    rc = end_timed(c, stats != nullptr, loc, s, &ms);
    if (rc != NR_OK || !stats) return rc;
    nr_compose_stats st{};
    st.ray_steps = hs[0] + hl[0];
    st.rays_hit = hs[1];
    st.rays_shaded = hs[3];
    st.shade_evals = (l.ao_strength > 0.0f ? 8ull : 4ull) * hs[3];
    st.part_evals = hs[4] + hl[4];
    st.wave_evals = hs[5] + hl[5];
    st.wave_skips = hs[6] + hl[6];
    st.iterations = (int32_t)std::max(hs[2], hl[2]);
    st.launches = launches;
    st.ms_total = ms;
    *stats = st;
    return NR_OK;
}

int nr_compose_sample(nr_compose *cp, const float *points, long n, float *value, int32_t *owner, int loc,
                      nr_compose_stats *stats) {
    if (!cp) return set_err(nullptr, NR_E_INVALID, "nr_compose_sample: composition is NULL");
    nr_ctx *c = cp->owner;
    if (n < 0 || n > (1l << 30)) return set_err(c, NR_E_INVALID, "nr_compose_sample: n = %ld outside [0, 2^30]", n);
    if (n > 0 && !points) return set_err(c, NR_E_INVALID, "nr_compose_sample: points is NULL");
    if (n == 0) { if (stats) *stats = nr_compose_stats{}; return NR_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    ComposeArgs Q = cp->A;
    Q.n = n; Q.frame = c->frame;
    Q.points = points; Q.value = value; Q.owner = owner;
    Q.stats = reinterpret_cast<unsigned long long *>(cp->d_cs + 32);
    const size_t N = (size_t)n;
    Staging io(loc);
    io.in(Q.points, 3 * N);
    io.out(Q.value, N); io.out(Q.owner, N);
    int rc;
    if ((rc = io.begin(c, cp->d_io, cp->cap_io, s)) != NR_OK) return rc;
    // 4-wave workgroups, as many per CU as the packs allow (at most k_query's three)
    const int fit = std::max(1, std::min(3, NR_LDS_PER_CU / std::max(1, Q.pack_bytes)));
    const int bpc = c->blocks_per_cu > 0 ? std::min(c->blocks_per_cu, fit) : fit;
    const int grid = (int)std::max<size_t>(1, std::min<size_t>((N + 255) / 256, (size_t)num_cus(c->device) * bpc));
    HIPCHK(c, hipEventRecord(c->ev0, s));
    HIPCHK(c, hipMemsetAsync(cp->d_cs, 0, COMPOSE_CS_BYTES, s));
    HIPCHK(c, launch_compose_sample(Q, grid, s));
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if ((rc = io.end(c, s)) != NR_OK) return rc;
    unsigned long long hs[7];
    if (stats) HIPCHK(c, hipMemcpyAsync(hs, Q.stats, sizeof hs, hipMemcpyDeviceToHost, s));
    float ms = 0.0f;
    rc = end_timed(c, stats != nullptr, loc, s, &ms);
    if (rc != NR_OK || !stats) return rc;
    hs[0] = (unsigned long long)N;  // points evaluated
    compose_stats(hs, false, 2, ms, stats);
    return NR_OK;
}

}  // extern "C"

// ---- composed scenes on a lattice (nr_compose_mesh.hip) ----

// The ComposeArgs of the lattice kernels: the packs, nets and parts with the owner's frame and the
// statistics words.  Their workgroup and grid are compose_shape's, over the points of the launch.
static ComposeArgs compose_field_args(const nr_compose *cp) {
    ComposeArgs Q = cp->A;
    Q.frame = cp->owner->frame;
    Q.stats = reinterpret_cast<unsigned long long *>(cp->d_cs + 32);
    return Q;
}

namespace nr {

int compose_sparse_sampler(nr_compose *cp, const SparseArgs &A, bool sample, hipStream_t s) {
    nr_ctx *c = cp->owner;
    const ComposeArgs Q = compose_field_args(cp);
    int threads, grid;
    compose_shape(cp, sample ? (size_t)A.nactive * A.L.stride : (size_t)A.L.ncoarse, threads, grid);
    if (sample) HIPCHK(c, launch_compose_sp_sample(Q, A, grid, threads, s));
    else HIPCHK(c, launch_compose_sp_coarse(Q, A, grid, threads, s));
    return NR_OK;
}

int compose_vertex_pass(nr_compose *cp, const float *d_vertices, float *d_normals, int32_t *d_part, size_t nv,
                               hipStream_t s) {
    nr_ctx *c = cp->owner;
    ComposeVertexArgs V{};
    V.vertices = d_vertices;
    V.normals = d_normals;
    V.part = d_part;
    V.nv = (long)nv;
    int threads, grid;
    compose_shape(cp, nv, threads, grid);
    HIPCHK(c, launch_compose_vertex(compose_field_args(cp), V, grid, threads, s));
    return NR_OK;
}

}  // namespace nr

// one k_compose_grid launch over the lattice (the statistics zeroed before it: two launches)
static int compose_grid_launch(nr_compose *cp, const LatticeArgs &L, float *d_value, int32_t *d_owner, hipStream_t s) {
    nr_ctx *c = cp->owner;
    ComposeGridArgs G{};
    G.L = L;
    G.value = d_value;
    G.owner = d_owner;
    int threads, grid;
    compose_shape(cp, (size_t)L.n, threads, grid);
    HIPCHK(c, hipMemsetAsync(cp->d_cs, 0, COMPOSE_CS_BYTES, s));
    HIPCHK(c, launch_compose_grid(compose_field_args(cp), G, grid, threads, s));
    return NR_OK;
}

// the statistics of a lattice call: the device words [4..6] and what the host knows
static int compose_lattice_stats(nr_compose *cp, hipStream_t s, uint64_t points, uint64_t active, long nv, bool normals,
                                 bool part, int launches, float ms, nr_compose_stats *stats) {
    nr_ctx *c = cp->owner;
    unsigned long long hs[7];
    HIPCHK(c, hipMemcpyAsync(hs, reinterpret_cast<unsigned long long *>(cp->d_cs + 32), sizeof hs, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    nr_compose_stats st{};
    st.ray_steps = points;
    st.rays_hit = active;
    st.rays_shaded = (uint64_t)nv;
    st.shade_evals = (normals ? 4ull * (uint64_t)nv : 0ull) + (part ? (uint64_t)nv : 0ull);
    st.part_evals = hs[4];
    st.wave_evals = hs[5];
    st.wave_skips = hs[6];
    st.launches = launches;
    st.ms_total = ms;
    *stats = st;
    return NR_OK;
}

extern "C" {

int nr_compose_sample_grid(nr_compose *cp, const float origin[3], const float step[3], const int dims[3], float *value,
                           int32_t *owner, int loc, nr_compose_stats *stats) {
    const char *fn = "nr_compose_sample_grid";
    if (!cp) return set_err(nullptr, NR_E_INVALID, "%s: composition is NULL", fn);
    nr_ctx *c = cp->owner;
    if (!value && !owner) return set_err(c, NR_E_INVALID, "%s: value and owner are both NULL", fn);
    int rc;
    if ((rc = lattice_check(c, fn, origin, step, dims, 1)) != NR_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    const LatticeArgs L = make_lattice(origin, step, dims);
    const size_t N = (size_t)L.n;
    float *dv = value;
    int32_t *dw = owner;
    Staging io(loc);
    io.out(dv, N); io.out(dw, N);
    if ((rc = io.begin(c, cp->d_io, cp->cap_io, s)) != NR_OK) return rc;
    HIPCHK(c, hipEventRecord(c->ev0, s));
    if ((rc = compose_grid_launch(cp, L, dv, dw, s)) != NR_OK) return rc;
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if ((rc = io.end(c, s)) != NR_OK) return rc;
    float ms = 0.0f;
    if ((rc = end_timed(c, stats != nullptr, loc, s, &ms)) != NR_OK || !stats) return rc;
    return compose_lattice_stats(cp, s, N, 0, 0, false, false, 2, ms, stats);
}

int nr_compose_extract_mesh(nr_compose *cp, const float origin[3], const float step[3], const int dims[3], float iso,
                            float *vertices, float *normals, int32_t *part, long v_cap, int32_t *triangles, long t_cap,
                            long *nv, long *nt, int loc, nr_compose_stats *stats) {
    const char *fn = "nr_compose_extract_mesh";
    if (!cp) return set_err(nullptr, NR_E_INVALID, "%s: composition is NULL", fn);
    nr_ctx *c = cp->owner;
    if (!nv || !nt) return set_err(c, NR_E_INVALID, "%s: NULL nv or nt", fn);
    *nv = 0;
    *nt = 0;
    int rc;
    if ((rc = lattice_check(c, fn, origin, step, dims, 2)) != NR_OK) return rc;
    if (!std::isfinite(iso)) return set_err(c, NR_E_INVALID, "%s: iso is not finite", fn);
    if (!vertices != !triangles) return set_err(c, NR_E_INVALID, "%s: vertices and triangles are given together", fn);
    if ((normals || part) && !vertices) return set_err(c, NR_E_INVALID, "%s: normals and part need vertices", fn);
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    const LatticeArgs L = make_lattice(origin, step, dims);
    if ((rc = ensure_buf(c, c->d_grid, c->cap_grid, (size_t)L.n)) != NR_OK) return rc;
    HIPCHK(c, hipEventRecord(c->ev0, s));
    if ((rc = compose_grid_launch(cp, L, c->d_grid, nullptr, s)) != NR_OK) return rc;
    int launches = 2;
    if ((rc = mesh_run(c, fn, s, L, c->d_grid, iso, vertices, normals, v_cap, triangles, t_cap, nv, nt, loc, &launches, cp,
                       part)) != NR_OK)
        return rc;
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if (!stats) return NR_OK;
    HIPCHK(c, hipStreamSynchronize(s));
    float ms = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    return compose_lattice_stats(cp, s, (uint64_t)L.n, 0, *nv, normals != nullptr, part != nullptr, launches, ms, stats);
}

int nr_compose_extract_mesh_sparse(nr_compose *cp, const float origin[3], const float step[3], const int dims[3], float iso,
                                   int brick, float band, float *vertices, float *normals, int32_t *part, int64_t *keys,
                                   long v_cap, int32_t *triangles, long t_cap, long *nv, long *nt, long *active_bricks,
                                   int loc, nr_compose_stats *stats) {
    const char *fn = "nr_compose_extract_mesh_sparse";
    if (!cp) return set_err(nullptr, NR_E_INVALID, "%s: composition is NULL", fn);
    nr_ctx *c = cp->owner;
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    HIPCHK(c, hipMemsetAsync(cp->d_cs, 0, COMPOSE_CS_BYTES, s));
    SparseDone done;
    const int rc = sparse_run(c, cp, fn, origin, step, dims, iso, brick, band, vertices, normals, part, keys, v_cap, triangles,
                              t_cap, nv, nt, active_bricks, loc, stats != nullptr, &done);
    if (rc != NR_OK || !stats) return rc;
    return compose_lattice_stats(cp, s, done.points, done.active, *nv, normals && vertices, part && vertices,
                                 done.launches + 1, done.ms, stats);
}

}  // extern "C"
