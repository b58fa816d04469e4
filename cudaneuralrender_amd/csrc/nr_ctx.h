// nr_ctx.h -- the context behind the C ABI (struct nr_ctx) and the helpers its host files share
// (nr_api*.hip, nr_group.hip).  Private to them: no kernel file and no C++ class includes it.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <cstring>
#include <string>
#include <vector>

#include "nr_internal.h"

constexpr int NR_MAX_QUEUES = 64;
#include "nr_kernels.h"

struct nr_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    bool use_own = true;  // stream = own_stream, created lazily: a context driven on a
                          // caller's stream never takes a hardware queue of its own
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::string err;

    // network
    std::vector<int> dims;
    std::vector<std::vector<float>> kernels, biases;  // Keras (in x out), bias
    std::vector<float *> d_W, d_b;                     // out-major per layer (generic kernel)
    bool fused = false;
    int precision = NR_PRECISION_FP32;
    float *d_pack16 = nullptr;
    float *d_gpack16 = nullptr;  // the backward pack (pack_grad_16; nr_mlp_gradient), null: none
    int gpack_bytes = 0;
    uint16_t *d_lp16 = nullptr;
    uint16_t *d_x3lp = nullptr;  // bf16/fp16: the fp32x3 pack for the normals (MlpArgs::x3n)
    float *d_x3fl = nullptr;
    int x3lp_bytes = 0, x3fl_bytes = 0;  // its sizes (TraceArgs: the EG instances stage it in LDS)
    bool fp32_normals = false;   // nr_set_debug bit 15: the bf16/fp16 tracers' normals in fp32 (A/B)
    float eg_tau = NR_ENDGAME_DEFAULT;  // nr_set_endgame: bf16/fp16 persistent renders' fp32x3 endgame
    float *d_lpf16 = nullptr;
    uint16_t *d_lps16 = nullptr;  // the 16x16x32 layout of d_lp16 / d_lpf16 (k_mlp16, 7 hidden layers)
    float *d_lpfs16 = nullptr;
    bool no_s16 = true;           // nr_set_debug bit 12 clear: k_mlp16 on the 32x32x16 stream (the
                                  // default; the 16x16x32 one measured 3-5 % slower, round 6)
    nr::MlpArgs mlp16{};  // 16-point-tile packs: k_trace, k_mlp16, k_march16, k_shade16
    bool clamp_ok = false;  // the bf16 pack is scaled for the clamped ReLU (pack_lowp_32)
    bool no_stream = false;  // nr_set_debug bit 11: the 16-bit MLP's builtin form (MlpArgs::lp_stream)
    bool no_clamp = false;  // nr_set_debug bit 9: bf16 ReLU by v_pk_max_i16, fp32 by add + max,
                            // on the same packs
    bool f32_clamp_ok = false;  // the fp32 pack is scaled for the clamped ReLU (pack_fp32_16)
    float *d_pkp = nullptr;     // the pruned fp32 pack (pack_fp32_16_pruned; the batched fp32 k_trace), null: none
    nr::PruneInfo prune;            // its order and k-steps (nrelu = 0: none)
    int prune_mode = 1;         // nr_set_prune
    float *d_pku = nullptr;     // the unit pack (pack_fp32_units; the batched fp32 k_trace), null: refused
    int unit_skip = 1;          // nr_set_unit_skip
    int schedule = 0; // NR_SCHED_PERSISTENT
    uint32_t *d_tr = nullptr;  // persistent-schedule counters + stats
    int debug = 0;
    int blocks_per_cu = 0;     // persistent grid: blocks (4 waves) per CU; 0 = auto
    // temporal block ordering (nr_set_temporal_order)
    int temporal = 0;
    int spread = -1;  // nr_set_pixel_spread; -1 = auto (spread_for)
    int probe_steps = 0, probe_take = 16, probe_dilate = 1;  // nr_set_cost_probe
    int wave_rays = 0;  // nr_set_wave_rays (0: automatic, wave_rays_for)
    int nq_shift = 3;    // nr_set_queue_shards: 8
    // nr_render_batch: per-frame arguments (pinned staging + device copy), host-output scratch
    nr::FrameArgs *h_frames = nullptr, *d_frames = nullptr;
    size_t cap_frames = 0;
    hipEvent_t ev_frames = nullptr;
    uint32_t *d_bout = nullptr;
    size_t cap_bout = 0;
    uint32_t *d_bcost = nullptr, *d_order[2] = {nullptr, nullptr};
    size_t cap_blocks = 0;
    int order_valid = 0, order_cur = 0;
    long long order_key = -1;  // image configuration the stored order belongs to
    unsigned long long *d_stamps = nullptr;
    size_t n_stamps = 0;       // waves of the last traced launch
    // ray queries (nr_trace_rays, nr_render_gbuffer): the ray cursor on its own 128-byte line +
    // 4 x u64 stats; staging of host rays and results
    uint32_t *d_qs = nullptr;
    float *d_qio = nullptr;
    size_t cap_qio = 0;
    // antialiasing (nr_render_aa): the sample cursor and the edge count on their own 128-byte lines
    // + 4 x u64 stats; the edge list (4 B per pixel) and the accumulators (8 B per edge pixel)
    uint32_t *d_aas = nullptr;
    uint32_t *d_aalist = nullptr;
    size_t cap_aalist = 0;
    unsigned long long *d_aaacc = nullptr;
    size_t cap_aaacc = 0;
    // lighting (nr_render_lit): the pixel cursor on its own 128-byte line + 4 x u64 stats; the
    // geometry buffer (status, position, normal: 28 B per pixel) and the ao / shadow values the
    // caller gave no device buffer for (8 B per pixel)
    uint32_t *d_ls = nullptr;
    float *d_lgbuf = nullptr;
    size_t cap_lgbuf = 0;
    float *d_lao = nullptr;
    size_t cap_lao = 0;
    // projection (nr_project_points): the point cursor on its own 128-byte line + 4 x u64 counters
    uint32_t *d_ps = nullptr;
    // volume sampling and isosurface extraction (nr_sample_grid, nr_mesh_grid, nr_extract_mesh):
    // the lattice of nr_extract_mesh (4 B per point; the staging of host lattices too), the
    // extraction's scratch (MeshArgs: 4 B per point + 24 B per 256 points) and the staging of
    // host meshes
    float *d_grid = nullptr;
    size_t cap_grid = 0;
    unsigned long long *d_mesh = nullptr;
    size_t cap_mesh = 0;
    float *d_mio = nullptr;
    size_t cap_mio = 0;
    // brick-sparse extraction (nr_extract_mesh_sparse; SparseArgs): the per-brick scratch (corner
    // values, brick -> slot map, block counts and scans) and the per-active-brick one (active list,
    // value store, point words, block counts and scans), both in 8-byte words
    unsigned long long *d_spb = nullptr, *d_spa = nullptr;
    size_t cap_spb = 0, cap_spa = 0;
    // ordering (nr_points_order; SortArgs): the two key / value buffers and the digit table, reused
    // across calls; the staging of its host arrays; nr_mesh_fit_samples' points, sorted points,
    // values and permutation (8 words per sample)
    uint32_t *d_sort = nullptr;
    size_t cap_sort = 0;
    float *d_sortio = nullptr;
    size_t cap_sortio = 0;
    float *d_fitsamp = nullptr;
    size_t cap_fitsamp = 0;
    // nr_mesh_create_device: its two sorts take d_sort; the read-back record, the f64 face normals
    // and areas, the tree's shape and the nodes' raw sums (8-byte words), reused across calls
    unsigned long long *d_tbuild = nullptr;
    size_t cap_tbuild = 0;

    // settings
    float inv_view[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 2};
    float normal[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -2, 0, 0, 0, 1};
    int frame = 0, color_type = NR_COLOR_FACING, num_inputs = 3, scene = NR_SCENE_V1;
    uint32_t *d_matcap = nullptr;
    int mw = 0, mh = 0;

    // scratch (owned per context; the reference keeps static globals)
    size_t cap_rays = 0;
    float4 *d_P[2] = {nullptr, nullptr}, *d_D[2] = {nullptr, nullptr};
    float4 *d_SP = nullptr, *d_SD = nullptr;
    float4 *d_FP[2] = {nullptr, nullptr}, *d_FD[2] = {nullptr, nullptr};  // wavefront endgame: fine queues
    size_t cap_fine = 0;
    size_t cap_ctr = 0;
    uint32_t *d_ctr = nullptr;       // [cap_ctr]: live counts per iteration, then shade count, then shade_it
    uint32_t *h_ctr = nullptr;       // pinned mirror
    size_t cap_out = 0;
    uint32_t *d_out = nullptr;
    size_t cap_io = 0;
    float *d_io = nullptr;           // mlp_forward staging
    int check_every = 32;            // host polls the live count every N iterations
    // layered schedule (any dense network): per-frame args in device memory, the frame's
    // launch sequence captured once per image configuration and replayed as a hipGraph
    nr::RenderArgs *d_rargs = nullptr;
    float *d_lsdf = nullptr, *d_lz = nullptr;  // SDFs (4 per converged ray), layer scratch
    size_t cap_lsdf = 0, cap_lz = 0;
    hipGraphExec_t lgraph = nullptr;
    std::vector<long long> lkey;               // configuration lgraph was captured for
    long long net_ver = 0;                     // bumped by every network upload
    long layer_chunk = 0;                      // nr_set_layer_chunk (0: auto)

    // per-launch profiling (nr_set_profiling)
    bool profiling = false;
    std::vector<hipEvent_t> ev_pool;
    struct Rec { int kind; int e0, e1; };   // kind 0 init, 1 march, 2 shade
    std::vector<Rec> recs;
    uint64_t prof_renders = 0;
};

struct nr_compose;

// A triangle mesh on the device (nr_api_trimesh.hip creates and queries it, nr_api_sample.hip samples
// it): the hierarchy with its moments, the reordered triangles, the pseudonormal table and the area
// table, all built on the host at create time (nr_trimesh_create) or by kernels (nr_mesh_create_device).
struct nr_trimesh {
    nr_ctx *owner = nullptr;
    long nv = 0, nt = 0, nnodes = 0, ntl = 0;
    int depth = 0, closed = 0;
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    float scale = 0;              // largest |coordinate| + largest axis extent: the boxes' slack times 2^18
    float *d_nodes = nullptr, *d_tris = nullptr, *d_table = nullptr, *d_moments = nullptr;
    uint32_t *d_area = nullptr;   // [ntl] thresholds of the area table (nr_mesh_sample)
    long area_last = -1;          // its last pickable position; -1: the area sum is not > 0
    unsigned long long *d_stats = nullptr;
    float *d_io = nullptr;        // staging of host points and results
    size_t cap_io = 0;
};

namespace nr {

// ---- errors, device memory, the stream (nr_api.hip) ----

// Records the text as the context's (c may be NULL) and the calling thread's last error; returns code.
int set_err(nr_ctx *c, int code, const char *fmt, ...);

#define HIPCHK(ctx, expr)                                                                            \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) return set_err(ctx, NR_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

template <class T>
void dfree(T *&p) {
    if (p) { (void)hipFree(p); p = nullptr; }
}

template <class T>
int ensure_buf(nr_ctx *c, T *&p, size_t &cap, size_t n) {
    if (n <= cap) return NR_OK;
    dfree(p);
    cap = 0;
    HIPCHK(c, hipMalloc(&p, std::max<size_t>(n, 64) * sizeof(T)));
    cap = std::max<size_t>(n, 64);
    return NR_OK;
}

int num_cus(int dev);

// The context's stream: the caller's (nr_set_stream) or the private one, created here on
// first use.  Returns NULL only if that creation failed (error recorded).
#define GET_STREAM(c, s)                                           \
    hipStream_t s = cur_stream(c);                                 \
    if ((c)->use_own && !(c)->own_stream) return NR_E_HIP;

hipStream_t cur_stream(nr_ctx *c);

// The end of a timed call whose launches lie between ev0 and ev1: with statistics wanted,
// synchronise and read the time; without, synchronise only if results went to the host.
int end_timed(nr_ctx *c, bool timed, int loc, hipStream_t s, float *ms);

// a cursor on its own 128-byte line + 4 x u64 counters (nr_ctx::d_qs, d_ls, d_ps)
constexpr size_t CURSOR_STATS_BYTES = 128 + 4 * 8;

// The grid of a launch over n items, per_workgroup of them to a workgroup, by the CU count:
// nr_set_occupancy's workgroups per CU, or default_bpc
inline int persistent_grid(const nr_ctx *c, size_t n, size_t per_workgroup, int default_bpc) {
    const int bpc = c->blocks_per_cu > 0 ? c->blocks_per_cu : default_bpc;
    return (int)std::max<size_t>(1, std::min<size_t>((n + per_workgroup - 1) / per_workgroup, (size_t)num_cus(c->device) * bpc));
}

// ---- what the frame drivers check and fill (nr_api_render.hip) ----
int check_shape(nr_ctx *c, int W, int H, int band, int nshards, int shard, int max_steps);
int check_scene(nr_ctx *c);
RenderArgs render_args(const nr_ctx *c, int W, int H, int rows, int band, int nshards, int shard, int max_steps);

// ---- shared by a network's calls and a composed scene's (nr_api_points.hip, nr_api_mesh.hip, nr_api_compose.hip) ----
int check_light(nr_ctx *c, const char *fn, const nr_light &l);
int lattice_check(nr_ctx *c, const char *fn, const float *origin, const float *step, const int *dims, int min_dim);
// what a brick-sparse extraction did, for the caller's statistics
struct SparseDone {
    uint64_t points = 0;   // the brick-corner lattice plus the active bricks' point sets
    uint64_t active = 0;
    int launches = 0;
    float ms = 0;
};
// A third field for mesh_run and sparse_run, beside c's network and a composed scene: whoever owns
// it (a triangle mesh: nr_api_trimesh.hip) samples the brick lattices and labels the vertices.  Both
// enqueue on s and add the kernels they issued to *launches.
struct FieldSource {
    void *self;
    // store == false: the brick-corner values into A.coarse; true: the active bricks' point sets into A.store
    int (*sample)(void *self, const SparseArgs &A, bool store, hipStream_t s, int *launches);
    // one int32 per device vertex into d_label (the `part` argument of mesh_run / sparse_run)
    int (*label)(void *self, const float *d_vertices, int32_t *d_label, size_t nv, hipStream_t s, int *launches);
};
int mesh_run(nr_ctx *c, const char *fn, hipStream_t s, const LatticeArgs &L, const float *d_sdf, float iso,
             float *vertices, float *normals, long v_cap, int32_t *triangles, long t_cap, long *nv, long *nt,
             int loc, int *launches, nr_compose *cp = nullptr, int32_t *part = nullptr, const FieldSource *field = nullptr);
int sparse_run(nr_ctx *c, nr_compose *cp, const char *fn, const float origin[3], const float step[3], const int dims[3],
               float iso, int brick, float band, float *vertices, float *normals, int32_t *part, int64_t *keys,
               long v_cap, int32_t *triangles, long t_cap, long *nv, long *nt, long *active_bricks, int loc, bool timed,
               SparseDone *done, const FieldSource *field = nullptr);
// The brick samplers of a composed scene (k_compose_sp_coarse; sample: k_compose_sp_sample), one launch on s.
int compose_sparse_sampler(nr_compose *cp, const SparseArgs &A, bool sample, hipStream_t s);
// The vertex pass of a composed scene (k_compose_vertex):
// normals and / or owners of the nv device vertices, one launch on s.
int compose_vertex_pass(nr_compose *cp, const float *d_vertices, float *d_normals, int32_t *d_part, size_t nv,
                        hipStream_t s);

// ---- staging of a call's host arrays ----

// The caller declares, in order, the arrays to upload (in) and the results it wants back (out):
// each by the argument-struct field or local pointer that holds the caller's array, and a size in
// 4-byte words.  A null array is skipped.  The staging buffer is carved in that order, every array
// aligned for its element type.  begin() sizes the buffer (plus `extra` words of the caller's own
// scratch, at buf + words), enqueues the uploads and repoints the fields at the staging memory;
// end(), after the launches, enqueues the downloads in declaration order.  With loc == NR_DEVICE
// nothing is staged and the fields keep the caller's pointers.
struct Staging {
    struct Item { void *field, *host; size_t off, words; bool out; };
    Item items[12];
    int n = 0;
    const bool host;
    size_t words = 0;  // staged so far
    float *base = nullptr;

    explicit Staging(int loc) : host(loc != NR_DEVICE) {}
    template <class T> void in(const T *&field, size_t w) { add(&field, w, false, sizeof(T) / 4); }
    template <class T> void out(T *&field, size_t w) { add(&field, w, true, sizeof(T) / 4); }

    int begin(nr_ctx *c, float *&buf, size_t &cap, hipStream_t s, size_t extra = 0) {
        int rc;
        if ((rc = ensure_buf(c, buf, cap, words + extra)) != NR_OK) return rc;
        base = buf;
        for (int i = 0; i < n; ++i) {
            const Item &it = items[i];
            float *dev = base + it.off;
            if (!it.out && it.words) HIPCHK(c, hipMemcpyAsync(dev, it.host, it.words * 4, hipMemcpyHostToDevice, s));
            memcpy(it.field, &dev, sizeof dev);
        }
        return NR_OK;
    }
    int end(nr_ctx *c, hipStream_t s) {
        for (int i = 0; i < n; ++i)
            if (items[i].out && items[i].words)
                HIPCHK(c, hipMemcpyAsync(items[i].host, base + items[i].off, items[i].words * 4, hipMemcpyDeviceToHost, s));
        return NR_OK;
    }

private:
    void add(const void *field, size_t w, bool out, size_t align) {
        void *p;
        memcpy(&p, field, sizeof p);
        if (!host || !p) return;
        assert(n < 12 && align >= 1);
        words = (words + align - 1) / align * align;
        items[n++] = Item{const_cast<void *>(field), p, words, w, out};
        words += w;
    }
};

}  // namespace nr
