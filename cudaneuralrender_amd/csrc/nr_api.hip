// nr_api.hip -- the C ABI of libnr.so (include/neural_render.h): contexts, buffers,
// the render loop driver and the host helpers.
//
// Replaces, on the reference side (daviesthomas/cudaNeuralRender @ v1):
//   render_kernel / copyViewMatrices / copyStaticSettings  src/volumeRender_kernel.cu:608-706
//   allocateBuffers + the static scratch globals           :578-606
//   NeuralNetwork::load / forward                          src/neuralNetwork.cpp:54-151
//   DenseLayer ctor / forward                              src/layers/denseLayer.cu:180-278
//   Image::loadPNG / savePNG                               src/neuralUtils/image.cu:36-110
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "nr_internal.h"

constexpr int NR_MAX_QUEUES = 64;
#include "nr_kernels.h"

using namespace nr;

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
    MlpArgs mlp16{};  // 16-point-tile packs: k_trace, k_mlp16, k_march16, k_shade16
    bool clamp_ok = false;  // the bf16 pack is scaled for the clamped ReLU (pack_lowp_32)
    bool no_stream = false;  // nr_set_debug bit 11: the 16-bit MLP's builtin form (MlpArgs::lp_stream)
    bool no_clamp = false;  // nr_set_debug bit 9: bf16 ReLU by v_pk_max_i16, fp32 by add + max,
                            // on the same packs
    bool f32_clamp_ok = false;  // the fp32 pack is scaled for the clamped ReLU (pack_fp32_16)
    float *d_pkp = nullptr;     // the pruned fp32 pack (pack_fp32_16_pruned; the batched fp32 k_trace), null: none
    PruneInfo prune;            // its order and k-steps (nrelu = 0: none)
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
    FrameArgs *h_frames = nullptr, *d_frames = nullptr;
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
    RenderArgs *d_rargs = nullptr;
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

namespace {
thread_local std::string g_err;

int set_err(nr_ctx *c, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    g_err = buf;
    return code;
}

// Pixel spread of a launch of `nframes` frames of `npix` pixels each (nr_set_pixel_spread;
// -1 = auto).  One frame deals groups of 16 blocks pixel-major, so one slow block's rays
// spread over many waves and the frame's tail is shorter (fp32 2.649 -> 2.517 ms).  A batch
// hides the tails behind the next frame's bulk, and block-major dealing (coherent waves: one
// 8x8 block per refill) is faster there: bf16 at every batch size (1024^2 x 32: 0.568 ->
// 0.519 ms/frame, one 8-way shard: 0.087 -> 0.081), fp32 once a launch holds >= 8 M pixels
// (1024^2 x 32: 1.961 -> 1.908; one 8-way shard x 32 frames, 4 M: 0.290 vs 0.293).
// Measurements: profiles/r1_ab_experiments.txt.
int spread_for(const nr_ctx *c, int prec, int nframes, size_t npix) {
    if (c->spread >= 0) return c->spread;
    if (nframes < 4) return 16;
    if (prec != NR_PRECISION_FP32) return 0;
    return (size_t)nframes * npix >= ((size_t)8 << 20) ? 0 : 16;
}

}  // namespace

int nr::report_error(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// ---- shard and batch geometry (exported: the callers that split frames use the same rules) ----

int nr_shard_rows(int H, int band, int nshards, int shard) {
    if (H < 0 || band < 1 || nshards < 1 || shard < 0 || shard >= nshards) return 0;
    int full = H / band, rem = H % band;
    int rows = (full / nshards) * band;
    int extra = full % nshards;               // bands beyond the complete rounds
    if (shard < extra) rows += band;
    if (shard == extra && rem) rows += rem;   // the partial last band
    return rows;
}

// Queue positions are uint32 (pix_ctr atomics in k_trace): one launch hands out
// shard_total = blocks of the busiest queue shard x 64 x frames positions.  Past a shard's end
// a wave of the low-precision tracers can take two pending reservations of up to 64 positions
// (NR_QUEUE_CHUNK_DENSE: one absorbed and found past the end while the wave still had positions
// of its pool, the next requested right after) and one blocking reservation of up to 64 before
// it moves on: with the grid nr_set_occupancy allows (16 workgroups x 4 waves per CU) on up to
// 512 CUs the over-reservation stays below 512 x 16 x 4 x 192 = 6,291,456 (the old
// 2^19 assumed 8 workgroups and no pending reservation).
int nr_batch_frames_per_launch(int W, int H, int band, int nshards, int shard, int nframes, int queue_shards) {
    if (W < 1 || H < 1 || nframes < 1 || queue_shards < 1) return 0;
    const int rows = nr_shard_rows(H, band, nshards, shard);
    if (rows < 1) return std::min(nframes, NR_MAX_BATCH);
    const long long nblocks = (long long)((W + 7) / 8) * ((rows + 7) / 8);
    const long long per_frame = ((nblocks + queue_shards - 1) / queue_shards) * 64;  // busiest shard
    const long long slop = 512ll * 16 * 4 * (64 + 2 * 64);
    const long long cap = ((1ll << 32) - 1 - slop) / per_frame;
    return (int)std::min<long long>(std::min(nframes, NR_MAX_BATCH), cap);
}

namespace {

#define HIPCHK(ctx, expr)                                                                            \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) return set_err(ctx, NR_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

template <class T>
void dfree(T *&p) {
    if (p) { (void)hipFree(p); p = nullptr; }
}

int free_network(nr_ctx *c) {
    for (auto *p : c->d_W) (void)hipFree(p);
    for (auto *p : c->d_b) (void)hipFree(p);
    c->d_W.clear(); c->d_b.clear();
    dfree(c->d_pack16); dfree(c->d_pkp); dfree(c->d_pku); dfree(c->d_gpack16); dfree(c->d_lp16); dfree(c->d_lpf16); dfree(c->d_x3lp); dfree(c->d_x3fl);
    dfree(c->d_lps16); dfree(c->d_lpfs16);
    c->fused = false;
    if (c->lgraph) { (void)hipGraphExecDestroy(c->lgraph); c->lgraph = nullptr; }
    c->lkey.clear();
    ++c->net_ver;
    return NR_OK;
}

int upload_pack(nr_ctx *c, const std::vector<uint16_t> &a, const std::vector<float> &f, uint16_t *&d_a, float *&d_f,
                MlpArgs &M) {
    std::vector<uint16_t> aa(a);
    std::vector<float> ff(f);
    size_t ab = (aa.size() * 2 + 15) / 16 * 16, fb = (ff.size() * 4 + 15) / 16 * 16;
    aa.resize(ab / 2, 0); ff.resize(fb / 4, 0.0f);
    HIPCHK(c, hipMalloc(&d_a, ab));
    HIPCHK(c, hipMalloc(&d_f, fb));
    HIPCHK(c, hipMemcpy(d_a, aa.data(), ab, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d_f, ff.data(), fb, hipMemcpyHostToDevice));
    M.lp = d_a; M.lpf = d_f;
    M.lp_bytes = (int)ab; M.lpf_bytes = (int)fb;
    return NR_OK;
}

int upload_lowp(nr_ctx *c) {
    dfree(c->d_lp16); dfree(c->d_lpf16);
    c->mlp16.lp = nullptr; c->mlp16.lpf = nullptr; c->mlp16.lp_bytes = 0; c->mlp16.lpf_bytes = 0;
    c->mlp16.lp_clamp = 0;
    dfree(c->d_x3lp); dfree(c->d_x3fl);
    c->mlp16.x3lp = nullptr; c->mlp16.x3fl = nullptr; c->mlp16.x3n = 0;
    c->x3lp_bytes = 0; c->x3fl_bytes = 0;
    dfree(c->d_lps16); dfree(c->d_lpfs16);
    c->mlp16.lps = nullptr; c->mlp16.lpfs = nullptr;
    if (!c->fused || c->precision == NR_PRECISION_FP32) return NR_OK;
    std::vector<uint16_t> a;
    std::vector<float> f;
    int clamp = 0;
    if (c->precision == NR_PRECISION_FP32X3) {
        // lp_clamp = the fp32x3 pack is valid (its scales exist); without it (or with
        // nr_set_debug bit 9) every wave runs the fp32 MLP
        if (!pack_x3_32(c->dims, c->kernels, c->biases, a, f, &clamp))
            return set_err(c, NR_E_INVALID, "fp32x3 pack failed");
        c->clamp_ok = clamp != 0;
        c->mlp16.lp_clamp = c->clamp_ok && !c->no_clamp;
        return upload_pack(c, a, f, c->d_lp16, c->d_lpf16, c->mlp16);
    }
    if (!pack_lowp_32(c->dims, c->kernels, c->biases, c->precision, a, f, &clamp))
        return set_err(c, NR_E_INVALID, "low-precision pack failed");
    c->clamp_ok = clamp != 0;
    c->mlp16.lp_clamp = c->clamp_ok && !c->no_clamp;
    int rc = upload_pack(c, a, f, c->d_lp16, c->d_lpf16, c->mlp16);
    if (rc != NR_OK) return rc;
    // k_mlp16's 16x16x32 layout of the same pack (the networks its streams take: 7 hidden layers)
    if (c->mlp16.nh == 7) {
        std::vector<uint16_t> sa;
        std::vector<float> sf;
        pack_lowp_s16(a, f, c->mlp16.nh, sa, sf);
        MlpArgs S{};
        if ((rc = upload_pack(c, sa, sf, c->d_lps16, c->d_lpfs16, S)) != NR_OK) return rc;
        if (S.lp_bytes != c->mlp16.lp_bytes || S.lpf_bytes != c->mlp16.lpf_bytes)
            return set_err(c, NR_E_INVALID, "16x16x32 pack size mismatch");
        c->mlp16.lps = c->no_s16 ? nullptr : c->d_lps16;
        c->mlp16.lpfs = c->no_s16 ? nullptr : c->d_lpfs16;
    }
    // the fp32x3 pack beside it, for the normals (read from global memory); a network whose
    // pack is not valid keeps the fp32 normals
    std::vector<uint16_t> xa;
    std::vector<float> xf;
    int xok = 0;
    if (pack_x3_32(c->dims, c->kernels, c->biases, xa, xf, &xok) && xok) {
        MlpArgs X{};
        if ((rc = upload_pack(c, xa, xf, c->d_x3lp, c->d_x3fl, X)) != NR_OK) return rc;
        c->mlp16.x3lp = X.lp; c->mlp16.x3fl = X.lpf;
        c->x3lp_bytes = X.lp_bytes; c->x3fl_bytes = X.lpf_bytes;
        c->mlp16.x3n = c->fp32_normals ? 0 : 1;
    }
    return NR_OK;
}

// The pruned fp32 pack for c->prune_mode beside the full one (same size); MlpArgs::pkp only while
// the clamped form is on (nr_set_debug bit 9 turns both off).
// MlpArgs::pku: the unit form runs while unit skip is on, the prune mode is 1 and the clamped form
// is on; nr_set_prune 0 and 2 and nr_set_unit_skip(0) keep the paths they had
void select_unit_pack(nr_ctx *c) {
    c->mlp16.pku = c->unit_skip && c->prune_mode == 1 && c->mlp16.f32_clamp ? c->d_pku : nullptr;
}

int upload_pruned(nr_ctx *c) {
    dfree(c->d_pkp);
    dfree(c->d_pku);
    c->prune = PruneInfo{};
    c->mlp16.pkp = nullptr;
    c->mlp16.pku = nullptr;
    c->mlp16.ks_bits = 0;
    if (!c->fused) return NR_OK;
    std::vector<float> pp;
    if (pack_fp32_units(c->dims, c->kernels, c->biases, pp)) {
        pp.resize((size_t)c->mlp16.pk_bytes / 4, 0.0f);
        HIPCHK(c, hipMalloc(&c->d_pku, (size_t)c->mlp16.pk_bytes));
        HIPCHK(c, hipMemcpy(c->d_pku, pp.data(), (size_t)c->mlp16.pk_bytes, hipMemcpyHostToDevice));
    }
    select_unit_pack(c);
    if (!pack_fp32_16_pruned(c->dims, c->kernels, c->biases, c->prune_mode, pp, c->prune)) {
        c->prune = PruneInfo{};
        return NR_OK;
    }
    pp.resize((size_t)c->mlp16.pk_bytes / 4, 0.0f);
    HIPCHK(c, hipMalloc(&c->d_pkp, (size_t)c->mlp16.pk_bytes));
    HIPCHK(c, hipMemcpy(c->d_pkp, pp.data(), (size_t)c->mlp16.pk_bytes, hipMemcpyHostToDevice));
    c->mlp16.ks_bits = prune_ks_bits(c->prune);
    c->mlp16.pkp = c->mlp16.f32_clamp ? c->d_pkp : nullptr;
    return NR_OK;
}

int set_network(nr_ctx *c, std::vector<int> dims, std::vector<std::vector<float>> K, std::vector<std::vector<float>> B) {
    HIPCHK(c, hipSetDevice(c->device));
    free_network(c);
    c->dims = std::move(dims); c->kernels = std::move(K); c->biases = std::move(B);
    int nl = (int)c->dims.size() - 1;
    for (int l = 0; l < nl; ++l) {
        int in = c->dims[l], out = c->dims[l + 1];
        // DenseLayer::initializeWeights (denseLayer.cu:217-227): W[y*in + x] = kernel[x][y]
        std::vector<float> W((size_t)in * out);
        for (int x = 0; x < in; ++x)
            for (int y = 0; y < out; ++y) W[(size_t)y * in + x] = c->kernels[l][(size_t)x * out + y];
        float *dw = nullptr, *db = nullptr;
        HIPCHK(c, hipMalloc(&dw, W.size() * 4));
        HIPCHK(c, hipMalloc(&db, (size_t)out * 4));
        c->d_W.push_back(dw); c->d_b.push_back(db);
        HIPCHK(c, hipMemcpy(dw, W.data(), W.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(db, c->biases[l].data(), (size_t)out * 4, hipMemcpyHostToDevice));
    }
    std::vector<float> pack16;
    int f32_clamp = 0;
    c->fused = pack_fp32_16(c->dims, c->kernels, c->biases, pack16, &f32_clamp);
    c->mlp16 = MlpArgs{};
    c->mlp16.lp_stream = !c->no_stream;
    c->f32_clamp_ok = c->fused && f32_clamp != 0;
    c->mlp16.f32_clamp = c->f32_clamp_ok && !c->no_clamp;
    if (c->fused) {
        size_t pb = (pack16.size() * 4 + 15) / 16 * 16;
        pack16.resize(pb / 4, 0.0f);
        HIPCHK(c, hipMalloc(&c->d_pack16, pb));
        HIPCHK(c, hipMemcpy(c->d_pack16, pack16.data(), pb, hipMemcpyHostToDevice));
        c->mlp16.pk = c->d_pack16;
        c->mlp16.pk_bytes = (int)pb;
        c->mlp16.in0 = c->dims[0];
        c->mlp16.nh = nl - 2;
        // the backward pack beside it (networks of at most GRAD_MAX_HIDDEN hidden layers)
        std::vector<float> gpack;
        c->gpack_bytes = 0;
        if (pack_grad_16(c->dims, c->kernels, gpack)) {
            const size_t gb = (gpack.size() * 4 + 15) / 16 * 16;
            gpack.resize(gb / 4, 0.0f);
            HIPCHK(c, hipMalloc(&c->d_gpack16, gb));
            HIPCHK(c, hipMemcpy(c->d_gpack16, gpack.data(), gb, hipMemcpyHostToDevice));
            c->gpack_bytes = (int)gb;
        }
        int rc;
        if ((rc = upload_pruned(c)) != NR_OK) return rc;
    }
    return upload_lowp(c);
}

int ensure_rays(nr_ctx *c, size_t n) {
    if (n <= c->cap_rays) return NR_OK;
    for (int i = 0; i < 2; ++i) { dfree(c->d_P[i]); dfree(c->d_D[i]); }
    dfree(c->d_SP); dfree(c->d_SD);
    c->cap_rays = 0;
    size_t b = std::max<size_t>(n, 64) * sizeof(float4);
    for (int i = 0; i < 2; ++i) {
        HIPCHK(c, hipMalloc(&c->d_P[i], b));
        HIPCHK(c, hipMalloc(&c->d_D[i], b));
    }
    HIPCHK(c, hipMalloc(&c->d_SP, b));
    HIPCHK(c, hipMalloc(&c->d_SD, b));
    c->cap_rays = std::max<size_t>(n, 64);
    return NR_OK;
}

// the wavefront schedule's fine queues (the endgame: rays marching in fp32x3), ping-pong
int ensure_fine(nr_ctx *c, size_t n) {
    if (n <= c->cap_fine) return NR_OK;
    for (int i = 0; i < 2; ++i) { dfree(c->d_FP[i]); dfree(c->d_FD[i]); }
    c->cap_fine = 0;
    const size_t b = std::max<size_t>(n, 64) * sizeof(float4);
    for (int i = 0; i < 2; ++i) {
        HIPCHK(c, hipMalloc(&c->d_FP[i], b));
        HIPCHK(c, hipMalloc(&c->d_FD[i], b));
    }
    c->cap_fine = std::max<size_t>(n, 64);
    return NR_OK;
}

int ensure_ctr(nr_ctx *c, size_t n) {
    if (n <= c->cap_ctr) return NR_OK;
    dfree(c->d_ctr);
    if (c->h_ctr) { (void)hipHostFree(c->h_ctr); c->h_ctr = nullptr; }
    c->cap_ctr = 0;
    HIPCHK(c, hipMalloc(&c->d_ctr, n * 4));
    HIPCHK(c, hipHostMalloc(&c->h_ctr, n * 4, hipHostMallocDefault));
    c->cap_ctr = n;
    return NR_OK;
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

// event pair for one launch when profiling; returns indices into ev_pool
int prof_begin(nr_ctx *c, int kind, hipStream_t s) {
    if (!c->profiling) return 0;
    size_t need = c->recs.size() * 2 + 2;
    while (c->ev_pool.size() < need) {
        hipEvent_t e;
        HIPCHK(c, hipEventCreate(&e));
        c->ev_pool.push_back(e);
    }
    int e0 = (int)c->recs.size() * 2;
    c->recs.push_back({kind, e0, e0 + 1});
    HIPCHK(c, hipEventRecord(c->ev_pool[e0], s));
    return NR_OK;
}
int prof_end(nr_ctx *c, hipStream_t s) {
    if (!c->profiling) return NR_OK;
    HIPCHK(c, hipEventRecord(c->ev_pool[c->recs.back().e1], s));
    return NR_OK;
}

int num_cus(int dev) {
    int cus = 256;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    return cus;
}

// The context's stream: the caller's (nr_set_stream) or the private one, created here on
// first use.  Returns NULL only if that creation failed (error recorded).
#define GET_STREAM(c, s)                                           \
    hipStream_t s = cur_stream(c);                                 \
    if ((c)->use_own && !(c)->own_stream) return NR_E_HIP;

hipStream_t cur_stream(nr_ctx *c) {
    if (c->use_own && !c->own_stream) {
        if (hipSetDevice(c->device) != hipSuccess ||
            hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
            c->own_stream = nullptr;
            set_err(c, NR_E_HIP, "stream creation failed");
            return nullptr;
        }
        c->stream = c->own_stream;
    }
    return c->stream;
}

// The end of a timed call whose launches lie between ev0 and ev1: with statistics wanted,
// synchronise and read the time; without, synchronise only if results went to the host.
int end_timed(nr_ctx *c, bool timed, int loc, hipStream_t s, float *ms) {
    if (timed) {
        HIPCHK(c, hipStreamSynchronize(s));
        HIPCHK(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
    } else if (loc != NR_DEVICE) {
        HIPCHK(c, hipStreamSynchronize(s));
    }
    return NR_OK;
}

// ---- what every frame render checks and fills (nr_render_shard, nr_render_batch, nr_render_aa) ----

int check_shape(nr_ctx *c, int W, int H, int band, int nshards, int shard, int max_steps) {
    if (W < 1 || H < 1 || (long)W * H > (1l << 31)) return set_err(c, NR_E_INVALID, "nr_render: bad size %dx%d", W, H);
    if (band < 1 || nshards < 1 || shard < 0 || shard >= nshards) return set_err(c, NR_E_INVALID, "nr_render: bad shard");
    if (max_steps < 0) return set_err(c, NR_E_INVALID, "nr_render: max_steps < 0");
    return NR_OK;
}

// network, inputs and matcap
int check_scene(nr_ctx *c) {
    if (c->dims.empty()) return set_err(c, NR_E_STATE, "nr_render: no network loaded");
    if (c->dims.back() != 1)
        return set_err(c, NR_E_FORMAT, "nr_render: the SDF network must have one output (has %d)", c->dims.back());
    if (c->dims[0] != c->num_inputs)
        return set_err(c, NR_E_STATE, "nr_render: network takes %d inputs but numInputs = %d", c->dims[0], c->num_inputs);
    if (c->color_type == NR_COLOR_MATCAP && !c->d_matcap) return set_err(c, NR_E_STATE, "nr_render: matcap colouring without a matcap");
    return NR_OK;
}

// The RenderArgs every schedule shares: the shard image, scene, colouring and matcap.  The caller
// adds out, frame and the view where one launch has them (a batch's are in its FrameArgs).
RenderArgs render_args(const nr_ctx *c, int W, int H, int rows, int band, int nshards, int shard, int max_steps) {
    RenderArgs A{};
    A.W = W; A.H = H; A.rows = rows; A.band = band; A.nshards = nshards; A.shard = shard;
    A.max_steps = max_steps; A.scene = c->scene; A.color_type = c->color_type;
    A.matcap = c->d_matcap; A.mw = c->mw; A.mh = c->mh;
    set_recips(A);
    return A;
}

int read_queue_counters(nr_ctx *c, int max_steps, nr_stats &st, hipStream_t s);

// The endgame's threshold for a persistent render (TraceArgs::eg_tau): nr_set_endgame's, for the
// bf16/fp16 tracers with fp32x3 normals (the fine passes use their fp32x3 pack) and iteration
// counts that fit the fine queue's 24 bits; 0 otherwise (the pure 16-bit march)
static float endgame_tau(const nr_ctx *c, int prec, int max_steps) {
    const bool lowp = prec == NR_PRECISION_BF16 || prec == NR_PRECISION_FP16;
    return lowp && c->mlp16.x3n && max_steps < (1 << 24) ? c->eg_tau : 0.0f;
}

// Persistent-tracer workgroups per CU for a launch of `total` pixels over `nframes` frames
// (profiles/r2_occupancy.txt, r2_single_bpc.txt, r2_lowp_occ.txt):
//   fp32: 2 for one frame or fewer than 4 frames or under 1 M pixels (the tail outweighs the
//         bulk), 4 from 8 M pixels (the 38 KB, <= 128-VGPR batched instance), else 3;
//   bf16/fp16 (<= 128 VGPRs, 31 KB): 2 under 1 M pixels, 3 under 2 M (a 1024^2 frame: 0.885 /
//         0.843 / 0.856 ms at 2 / 3 / 4), else 4 (1024^2 x 20: 0.424 -> 0.404 ms/frame at 3 -> 4,
//         2048^2 x 8: 1.661 -> 1.569, one 2048^2 frame 2.503 -> 2.481).
int default_bpc(int prec, size_t total, int nframes) {
    const size_t M = (size_t)1 << 20;
    // fp32x3: its k_trace instance is built for 3 waves per SIMD (168 VGPRs)
    if (prec == NR_PRECISION_FP32X3) return total < M ? 2 : 3;
    if (prec == NR_PRECISION_FP32) {
        if (nframes < 4 || total < M) return 2;
        return total >= 8 * M ? 4 : 3;
    }
    if (total < M) return 2;
    return total < 2 * M ? 3 : 4;
}

// Workgroups per CU of a persistent launch: nr_set_occupancy's value or default_bpc's; for the
// endgame's instances (eg: a bf16/fp16 launch with T.eg_tau > 0; the diagnostic stamps and probe
// instances march without the endgame, launch_trace_k) NR_TRACE_BPC_EG 4-wave workgroups' worth:
// with NR_EG_WAVES > 4 exactly that -- launch_trace_k runs them as one NR_EG_WAVES-wave workgroup
// per CU, and fewer would leave CUs idle -- else at most that
int trace_bpc(const nr_ctx *c, int prec, size_t total, int nframes, bool eg) {
    const int bpc = c->blocks_per_cu > 0 ? c->blocks_per_cu : default_bpc(prec, total, nframes);
    if (eg) return NR_EG_WAVES > 4 ? NR_TRACE_BPC_EG : std::min(bpc, NR_TRACE_BPC_EG);
    return bpc;
}

// Rays per wave of a persistent launch (nr_set_wave_rays; 0 = automatic): an fp32 launch whose
// pixels fill at most 2x its waves' 64-ray slots marches 32 per wave -- at 64 nearly every ray
// is dealt in the first refills and every wave runs 4 tiles per iteration (one 1024^2 frame on
// 8 row-band shards: 1.015 -> 0.854 ms, on 4 shards 1.139 -> 1.124; on 2 shards or whole frames
// 32 is slower, and bf16, whose tiles are cheap, gains nothing; profiles/r3_ab_experiments.txt
// (24), (25)).
int wave_rays_for(const nr_ctx *c, int prec, size_t pixels, int grid) {
    if (c->wave_rays > 0) return c->wave_rays;
    if (prec == NR_PRECISION_FP32 && pixels <= 2 * (size_t)grid * 4 * 64) return 32;
    return 64;
}

// Block-cost buffers of the temporal order / cost probe for a frame-shard shape: a new shape
// (key) invalidates the recorded order; the buffers grow with the block count.
int order_buffers(nr_ctx *c, int W, int H, int band, int nshards, int shard, int nblocks) {
    const long long key = ((((long long)W * 65536 + H) * 4096 + band) * 64 + nshards) * 64 + shard;
    if (key != c->order_key) { c->order_valid = 0; c->order_key = key; }
    if ((size_t)nblocks > c->cap_blocks) {
        dfree(c->d_bcost); dfree(c->d_order[0]); dfree(c->d_order[1]);
        HIPCHK(c, hipMalloc(&c->d_bcost, (size_t)nblocks * 4));
        HIPCHK(c, hipMalloc(&c->d_order[0], (size_t)nblocks * 4));
        HIPCHK(c, hipMalloc(&c->d_order[1], (size_t)nblocks * 4));
        c->cap_blocks = nblocks;
        c->order_valid = 0;
    }
    return NR_OK;
}

// ---- the persistent tracer's launch (k_trace), shared by its single-frame and batched drivers ----

// d_tr: one set of NR_MAX_QUEUES shard counters on their own 128-byte lines, then 16 x u64 stats
// (allocated twice over: the cost probe's launch has a set of its own)
constexpr size_t TR_BYTES = NR_MAX_QUEUES * 128 + 16 * 8;

inline uint64_t lane_cap_for(int take) { return take >= 64 ? ~0ull : (1ull << take) - 1ull; }

// The TraceArgs that follow from the shard image (W x rows, bands of `band` rows) and the context,
// whatever the launch: counters and statistics in d_tr, the queue geometry -- the pixel spread is
// chosen for the whole call's `nframes` frames of `npix` pixels -- the endgame's threshold and
// the fp32x3 pack sizes.
int trace_args(nr_ctx *c, int prec, int W, int rows, int band, int nframes, size_t npix, int max_steps, TraceArgs &T) {
    if (!c->d_tr) HIPCHK(c, hipMalloc(&c->d_tr, 2 * TR_BYTES));
    T = TraceArgs{};
    T.pix_ctr = c->d_tr;
    T.stats = reinterpret_cast<unsigned long long *>(c->d_tr + NR_MAX_QUEUES * 32);
    T.nq_shift = c->nq_shift;
    T.bw = (W + 7) / 8;
    T.nblocks = T.bw * ((rows + 7) / 8);
    const int sp = spread_for(c, prec, nframes, npix);
    T.spread_shift = sp > 1 ? 31 - __builtin_clz((unsigned)sp) : 0;
    T.inv_bw = 1.0 / (double)T.bw;
    T.inv_band = 1.0 / (double)band;
    T.eg_tau = endgame_tau(c, prec, max_steps);
    T.x3lp_bytes = c->x3lp_bytes;
    T.x3fl_bytes = c->x3fl_bytes;
    return NR_OK;
}

// The grid of a launch of `total` pixels over `nframes` frames on `cus` CUs, and the rays per wave
// that go with it (T.take, T.lane_cap).  T.eg_tau must be final: the endgame's instances have
// their own workgroups per CU (trace_bpc).
int trace_grid(const nr_ctx *c, int prec, TraceArgs &T, size_t total, int nframes, int cus) {
    const int bpc = trace_bpc(c, prec, total, nframes, T.eg_tau > 0.0f && c->mlp16.x3n);
    int grid = (int)std::min<size_t>((total + 255) / 256, (size_t)cus * bpc);
    if (grid < 1) grid = 1;
    T.take = wave_rays_for(c, prec, total, grid);
    T.lane_cap = lane_cap_for(T.take);
    return grid;
}

// Temporal block order (nr_set_temporal_order) around one launch: the launch dispenses the blocks
// of its frames longest-first by the costs the previous launch of this frame-shard shape recorded
// (the block layout is the same for every frame of a batch; the costs are the max over them), and
// records its own for the next one.  order_buffers comes first.
int order_begin(nr_ctx *c, TraceArgs &T, hipStream_t s) {
    if (!c->temporal) return NR_OK;
    T.order = c->order_valid ? c->d_order[c->order_cur] : nullptr;
    T.bcost = c->d_bcost;
    HIPCHK(c, hipMemsetAsync(c->d_bcost, 0, (size_t)T.nblocks * 4, s));
    return NR_OK;
}
int order_end(nr_ctx *c, const TraceArgs &T, hipStream_t s) {
    if (!c->temporal) return NR_OK;
    HIPCHK(c, launch_order(c->d_bcost, c->d_order[c->order_cur ^ 1], T.nblocks, T.bw, c->temporal > 1, s));
    c->order_cur ^= 1;
    c->order_valid = 1;
    return NR_OK;
}

// The statistics of a call's k_trace launches (T.stats, accumulated since the call cleared them)
// and its ev0 -> ev1 time; without `stats` it only waits for results that went to the host.
int trace_stats(nr_ctx *c, const TraceArgs &T, int launches, int loc, nr_stats *stats, hipStream_t s) {
    unsigned long long hs[6];
    if (stats) HIPCHK(c, hipMemcpyAsync(hs, T.stats, sizeof hs, hipMemcpyDeviceToHost, s));
    float ms = 0;
    const int rc = end_timed(c, stats != nullptr, loc, s, &ms);
    if (rc != NR_OK || !stats) return rc;
    nr_stats st{};
    st.ray_steps = hs[0];
    st.rays_hit = hs[1];
    st.iterations = (int32_t)hs[2];
    st.rays_shaded = hs[3];
    st.shade_evals = 4ull * hs[3];
    st.endgame_evals = hs[4];
    st.endgame_switches = hs[5];
    st.launches = launches;
    st.ms_total = ms;
    *stats = st;
    return NR_OK;
}

// The MLP arguments of a launch over these frame numbers: the bf16 clamped-ReLU form
// (nr_mlp16.h) needs every network input within LP_INPUT_BOUND.  Ray positions stay inside
// the bounding sphere; the 4th input of an animation network is the frame number, checked here.
MlpArgs mlp_for_frames(const nr_ctx *c, const nr_frame *frames, int nframes, int frame) {
    MlpArgs M = c->mlp16;
    if (M.in0 == 4) {
        bool ok = std::fabs((float)frame) <= LP_INPUT_BOUND;
        for (int i = 0; i < nframes && ok; ++i) ok = std::fabs((float)frames[i].frame) <= LP_INPUT_BOUND;
        if (!ok) M.lp_clamp = 0;
    }
    return M;
}

// Per-frame arguments of a batch: pinned staging (reused only once the previous upload
// has been consumed) + device copy.  With host outputs the frames of one launch go
// through d_bout (`chunk` frames).
int upload_frames(nr_ctx *c, const nr_frame *frames, int nframes, size_t npix, int loc, int chunk, hipStream_t s) {
    if (!c->ev_frames) HIPCHK(c, hipEventCreateWithFlags(&c->ev_frames, hipEventDisableTiming));
    HIPCHK(c, hipEventSynchronize(c->ev_frames));
    if ((size_t)nframes > c->cap_frames) {
        if (c->h_frames) HIPCHK(c, hipHostFree(c->h_frames));
        dfree(c->d_frames);
        c->h_frames = nullptr;
        c->cap_frames = 0;
        HIPCHK(c, hipHostMalloc(&c->h_frames, (size_t)nframes * sizeof(FrameArgs)));
        HIPCHK(c, hipMalloc(&c->d_frames, (size_t)nframes * sizeof(FrameArgs)));
        c->cap_frames = nframes;
    }
    int rc;
    if (loc != NR_DEVICE && (rc = ensure_buf(c, c->d_bout, c->cap_bout, npix * chunk)) != NR_OK) return rc;
    for (int i = 0; i < nframes; ++i) {
        FrameArgs &f = c->h_frames[i];
        memcpy(f.inv_view, frames[i].inv_view, sizeof f.inv_view);
        memcpy(f.normal, frames[i].normal, sizeof f.normal);
        f.zoff = -0.7 + ((double)(frames[i].frame * 2) * 0.7 / 360.0);  // sphere_zoff, same f64 ops
        f.frame = frames[i].frame;
        f.frame_f = (float)frames[i].frame;
        f.out = loc == NR_DEVICE ? frames[i].out : c->d_bout + (size_t)(i % chunk) * npix;
    }
    HIPCHK(c, hipMemcpyAsync(c->d_frames, c->h_frames, (size_t)nframes * sizeof(FrameArgs), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipEventRecord(c->ev_frames, s));
    return NR_OK;
}

// Wavefront schedule over the frames of a batch (one frame for nr_render_shard): the
// rays of up to 32 frames share one queue; per iteration ONE k_march16 launch (mlp16 +
// step + compaction) over it, at the end k_shade16.  The host polls the live count every
// check_every iterations and stops early once it is 0.
// bf16 / fp16 with the endgame (round 6, the persistent tracer's rule; endgame_tau): per
// iteration the coarse pass (k_march16 mode 1) hands the rays whose 16-bit SDF is below tau to
// the iteration's fine queue, then the fine pass (mode 2) marches that queue in fp32x3 -- so the
// frames equal the persistent schedule's, bit for bit (tests/test_gpu_endgame.py).
int render_wavefront(nr_ctx *c, const nr_frame *frames, int nframes, int W, int H, int band, int nshards, int shard,
                     int max_steps, int loc, nr_stats *stats, hipStream_t s) {
    const int rows = nr_shard_rows(H, band, nshards, shard);
    const size_t npix = (size_t)W * rows;
    nr_stats tot{};
    if (npix == 0) { if (stats) *stats = tot; return NR_OK; }
    if (npix > (1u << 27))
        return set_err(c, NR_E_INVALID, "nr_render: the wavefront schedule takes at most 2^27 pixels per shard");
    const int chunk = std::min(nframes, NR_MAX_BATCH);
    // WF_SEGS queue segments of seg_cap entries (a multiple of the 256-thread block)
    const size_t seg_cap = ((npix * chunk + WF_SEGS - 1) / WF_SEGS + 255) / 256 * 256;
    // counters: (max_steps + 1) x [WF_SEGS live counts], [WF_SEGS shade counts], then
    // max_steps shade flags; each count on its own 128-byte line
    const size_t line = (size_t)WF_SEGS * 32;
    const float tau = endgame_tau(c, c->precision, max_steps);
    const bool eg = tau > 0.0f;
    // the endgame's counters after them: (max_steps + 1) x [WF_SEGS fine counts], then one switch
    // count per iteration
    const size_t f_base = ((size_t)(max_steps + 2) * line + max_steps + line - 1) / line * line;
    const size_t sw_base = f_base + (size_t)(max_steps + 1) * line;
    const size_t nctr = eg ? sw_base + max_steps : (size_t)(max_steps + 2) * line + max_steps;
    int rc;
    if ((rc = ensure_rays(c, seg_cap * WF_SEGS)) != NR_OK) return rc;
    if (eg && (rc = ensure_fine(c, seg_cap * WF_SEGS)) != NR_OK) return rc;
    if ((rc = ensure_ctr(c, nctr + 8)) != NR_OK) return rc;
    if ((rc = upload_frames(c, frames, nframes, npix, loc, chunk, s)) != NR_OK) return rc;
    const RenderArgs A = render_args(c, W, H, rows, band, nshards, shard, max_steps);
    const int cus = num_cus(c->device);
    const int bpc = c->blocks_per_cu > 0 ? c->blocks_per_cu : 16;  // measured: 4 -> 2.10, 8 -> 2.06, 16 -> 2.02 ms/frame (32-frame batch)
    uint32_t *cnt = c->d_ctr, *shade_cnt = c->d_ctr + (size_t)(max_steps + 1) * line,
             *shade_it = c->d_ctr + (size_t)(max_steps + 2) * line;
    HIPCHK(c, hipEventRecord(c->ev0, s));
    for (int f0 = 0; f0 < nframes; f0 += chunk) {
        const int n = std::min(chunk, nframes - f0);
        const FrameArgs *F = c->d_frames + f0;
        const size_t total = npix * n;
        HIPCHK(c, hipMemsetAsync(c->d_ctr, 0, nctr * 4, s));
        QueueArgs Q{};
        Q.seg_cap = (long)seg_cap;
        Q.cnt_out = cnt; Q.p_out = c->d_P[0]; Q.d_out = c->d_D[0];
        Q.shade_cnt = shade_cnt; Q.shade_p = c->d_SP; Q.shade_d = c->d_SD; Q.shade_it = shade_it;
        Q.eg_tau = tau;
        uint32_t *fcnt = c->d_ctr + f_base, *fsw = c->d_ctr + sw_base;
        if ((rc = prof_begin(c, 0, s)) != NR_OK) return rc;
        HIPCHK(c, launch_init_f(A, F, Q, (long)npix, (long)total, cus * 8, s));
        if ((rc = prof_end(c, s)) != NR_OK) return rc;
        tot.launches += 2;
        const int grid = (int)std::max<size_t>(1, std::min<size_t>((total + 255) / 256, (size_t)cus * bpc));
        for (int it = 0; it < max_steps; ++it) {
            Q.cnt_in = cnt + (size_t)it * line; Q.cnt_out = cnt + (size_t)(it + 1) * line;
            Q.p_in = c->d_P[it & 1]; Q.d_in = c->d_D[it & 1];
            Q.p_out = c->d_P[(it + 1) & 1]; Q.d_out = c->d_D[(it + 1) & 1];
            // the endgame: the coarse pass appends this iteration's switched rays to fine queue `it`
            // (where the previous fine pass left its survivors), the fine pass then marches it
            Q.fcnt = fcnt + (size_t)it * line; Q.fp = c->d_FP[it & 1]; Q.fd = c->d_FD[it & 1]; Q.fsw = fsw + it;
            if ((rc = prof_begin(c, 1, s)) != NR_OK) return rc;
            HIPCHK(c, launch_march16(A, mlp_for_frames(c, frames, nframes, 0), Q, F, c->precision, it, grid, s, eg ? 1 : 0));
            if ((rc = prof_end(c, s)) != NR_OK) return rc;
            ++tot.launches;
            if (eg) {
                QueueArgs G = Q;
                G.cnt_in = fcnt + (size_t)it * line; G.cnt_out = fcnt + (size_t)(it + 1) * line;
                G.p_in = c->d_FP[it & 1]; G.d_in = c->d_FD[it & 1];
                G.p_out = c->d_FP[(it + 1) & 1]; G.d_out = c->d_FD[(it + 1) & 1];
                if ((rc = prof_begin(c, 1, s)) != NR_OK) return rc;
                HIPCHK(c, launch_march16(A, mlp_for_frames(c, frames, nframes, 0), G, F, c->precision, it, grid, s, 2));
                if ((rc = prof_end(c, s)) != NR_OK) return rc;
                ++tot.launches;
            }
            if (c->check_every > 0 && (it + 1) % c->check_every == 0 && it + 1 < max_steps) {
                HIPCHK(c, hipMemcpyAsync(c->h_ctr, Q.cnt_out, line * 4, hipMemcpyDeviceToHost, s));
                if (eg) HIPCHK(c, hipMemcpyAsync(c->h_ctr + line, fcnt + (size_t)(it + 1) * line, line * 4,
                                                 hipMemcpyDeviceToHost, s));
                HIPCHK(c, hipStreamSynchronize(s));
                uint64_t live = 0;
                for (int q = 0; q < WF_SEGS; ++q) live += c->h_ctr[q * 32] + (eg ? c->h_ctr[line + q * 32] : 0u);
                if (live == 0) break;
            }
        }
        const int shade_grid = (int)std::max<size_t>(1, std::min<size_t>((total + 1023) / 1024, (size_t)cus * 4));
        if ((rc = prof_begin(c, 2, s)) != NR_OK) return rc;
        HIPCHK(c, launch_shade16(A, c->mlp16, Q, F, shade_grid, s));
        if ((rc = prof_end(c, s)) != NR_OK) return rc;
        if (loc != NR_DEVICE)
            for (int i = f0; i < f0 + n; ++i)
                HIPCHK(c, hipMemcpyAsync(frames[i].out, c->d_bout + (size_t)(i % chunk) * npix, npix * 4,
                                         hipMemcpyDeviceToHost, s));
        if (stats) {
            HIPCHK(c, hipMemcpyAsync(c->h_ctr, c->d_ctr, nctr * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
            const uint32_t *h = c->h_ctr;
            int iters = 0;
            for (int it = 0; it < max_steps; ++it) {
                uint64_t live = 0, fine = 0;
                for (int q = 0; q < WF_SEGS; ++q) live += h[(size_t)it * line + q * 32];
                if (it == 0) tot.rays_hit += live;
                if (eg) {
                    // the fine queue of iteration it: its switched rays (counted in `live` too: their
                    // 16-bit evaluation) and the survivors of the previous fine pass
                    for (int q = 0; q < WF_SEGS; ++q) fine += h[f_base + (size_t)it * line + q * 32];
                    tot.endgame_evals += fine;
                    tot.endgame_switches += h[sw_base + it];
                    live += fine;
                }
                tot.ray_steps += live;
                if (live) iters = std::max(iters, it + 1);
                if (h[(size_t)(max_steps + 2) * line + it]) iters = std::max(iters, std::min(it + 2, max_steps));
            }
            uint64_t shaded = 0;
            for (int q = 0; q < WF_SEGS; ++q) shaded += h[(size_t)(max_steps + 1) * line + q * 32];
            tot.rays_shaded += shaded;
            tot.shade_evals += 4 * shaded;
            tot.iterations = std::max(tot.iterations, iters);
        }
    }
    if (c->profiling) c->prof_renders += nframes;
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if ((rc = end_timed(c, stats != nullptr, loc, s, &tot.ms_total)) != NR_OK) return rc;
    if (stats) *stats = tot;
    return NR_OK;
}

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

// counts of the queue schedules (wavefront, layered) from their per-iteration counters
int read_queue_counters(nr_ctx *c, int max_steps, nr_stats &st, hipStream_t s) {
    const size_t nctr = (size_t)2 * max_steps + 2;
    HIPCHK(c, hipMemcpyAsync(c->h_ctr, c->d_ctr, nctr * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    uint64_t steps = 0;
    int iters = 0;
    for (int it = 0; it < max_steps; ++it) {
        steps += c->h_ctr[it];
        if (c->h_ctr[it]) iters = std::max(iters, it + 1);
        if (c->h_ctr[max_steps + 2 + it]) iters = std::max(iters, std::min(it + 2, max_steps));
    }
    st.ray_steps = steps;
    st.rays_hit = c->h_ctr[0];
    st.rays_shaded = c->h_ctr[max_steps + 1];
    st.shade_evals = 4ull * st.rays_shaded;
    st.iterations = iters;
    return NR_OK;
}
int queue_stats(nr_ctx *c, int max_steps, int launches, nr_stats *stats, hipStream_t s) {
    if (!stats) return NR_OK;
    nr_stats st{};
    int rc = read_queue_counters(c, max_steps, st, s);
    if (rc != NR_OK) return rc;
    st.launches = launches;
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    st.ms_total = ms;
    *stats = st;
    return NR_OK;
}

// Layered schedule: the reference's structure (render_kernel :608-692, one
// NeuralNetwork::forward over the live points per iteration, denseLayer.cu:229-278) for
// any dense [3|4, ..., 1] network.  Per iteration: the dense layers over the live-ray
// queue in chunks of lchunk points (bounded scratch, the kernel.cu:659-660 TODO), then
// k_march_l; at the end the layers over 4 points per converged ray and k_shade_l.  All
// counts stay on the device; the whole frame is captured once per configuration and
// replayed as a hipGraph (the per-frame RenderArgs are rewritten in device memory by
// k_set_args before each replay).  fp32 throughout (nr_set_precision applies to the
// fused kernels).
int render_layered(nr_ctx *c, const RenderArgs &A0, uint32_t *out, size_t npix, int max_steps, int loc, nr_stats *stats,
                   hipStream_t s) {
    const int nl = (int)c->dims.size() - 1;
    if (c->dims[0] > 4) return set_err(c, NR_E_FORMAT, "nr_render: at most 4 network inputs (has %d)", c->dims[0]);
    int maxw = 1;
    for (int l = 1; l < nl; ++l) maxw = std::max(maxw, c->dims[l]);
    // chunk: 128 MiB per scratch buffer, at least 64K points, at most what a frame needs
    const long lchunk = c->layer_chunk > 0 ? c->layer_chunk
                                           : std::min<long>(4l * (long)npix, std::max<long>(65536, (128l << 20) / (4l * maxw)));
    int rc;
    if ((rc = ensure_rays(c, npix)) != NR_OK) return rc;
    if ((rc = ensure_ctr(c, (size_t)2 * max_steps + 8)) != NR_OK) return rc;
    if ((rc = ensure_buf(c, c->d_lsdf, c->cap_lsdf, 4 * npix)) != NR_OK) return rc;
    if ((rc = ensure_buf(c, c->d_lz, c->cap_lz, (size_t)2 * lchunk * maxw)) != NR_OK) return rc;
    if (!c->d_rargs) HIPCHK(c, hipMalloc(&c->d_rargs, sizeof(RenderArgs)));
    RenderArgs A = A0;
    if (loc != NR_DEVICE) {
        if ((rc = ensure_buf(c, c->d_out, c->cap_out, npix)) != NR_OK) return rc;
        A.out = c->d_out;
    }
    const int cus = num_cus(c->device);
    const int step_grid = (int)std::max<size_t>(1, std::min<size_t>((npix + 255) / 256, (size_t)cus * 4));
    const int shade_grid = (int)std::max<size_t>(1, std::min<size_t>((npix + 1023) / 1024, (size_t)cus * 4));
    const long nch_march = ((long)npix + lchunk - 1) / lchunk, nch_shade = (4l * (long)npix + lchunk - 1) / lchunk;
    uint32_t *cnt = c->d_ctr, *shade_cnt = c->d_ctr + max_steps + 1, *shade_it = c->d_ctr + max_steps + 2;
    const size_t nctr = (size_t)2 * max_steps + 2;
    float *zb[2] = {c->d_lz, c->d_lz + (size_t)lchunk * maxw};
    QueueArgs Q{};
    Q.shade_cnt = shade_cnt; Q.shade_p = c->d_SP; Q.shade_d = c->d_SD; Q.shade_it = shade_it;
    // the dense chain over one chunk of a queue (src 1: live rays, 2: tetrahedron points)
    auto chain = [&](int src, const float4 *pts, const uint32_t *count, int mul, long chunk0) -> hipError_t {
        for (int l = 0; l < nl; ++l) {
            DenseArgs D{};
            D.W = c->d_W[l]; D.b = c->d_b[l];
            D.in = c->dims[l]; D.out = c->dims[l + 1]; D.relu = l != nl - 1;
            D.A = l == 0 ? nullptr : zb[(l - 1) & 1];
            D.Z = l == nl - 1 ? c->d_lsdf + chunk0 : zb[l & 1];
            D.pts = pts; D.count = count; D.count_mul = mul; D.args = c->d_rargs;
            D.chunk0 = chunk0; D.chunk_n = lchunk;
            const int grid = (int)std::max<long>(1, std::min<long>((lchunk * D.out + 255) / 256, (long)cus * 8));
            hipError_t e = launch_dense(D, l == 0 ? src : 0, grid, s);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    };
    // one frame's launches (captured into the graph, or issued directly for long caps)
    auto frame = [&]() -> hipError_t {
        hipError_t e = hipMemsetAsync(c->d_ctr, 0, nctr * 4, s);
        if (e != hipSuccess) return e;
        Q.cnt_out = cnt; Q.p_out = c->d_P[0]; Q.d_out = c->d_D[0];
        if ((e = launch_init_l(c->d_rargs, Q, (long)npix, s)) != hipSuccess) return e;
        for (int it = 0; it < max_steps; ++it) {
            Q.cnt_in = cnt + it; Q.cnt_out = cnt + it + 1;
            Q.p_in = c->d_P[it & 1]; Q.d_in = c->d_D[it & 1];
            Q.p_out = c->d_P[(it + 1) & 1]; Q.d_out = c->d_D[(it + 1) & 1];
            for (long ch = 0; ch < nch_march; ++ch)
                if ((e = chain(1, Q.p_in, Q.cnt_in, 1, ch * lchunk)) != hipSuccess) return e;
            if ((e = launch_march_l(c->d_rargs, Q, c->d_lsdf, it, step_grid, s)) != hipSuccess) return e;
        }
        for (long ch = 0; ch < nch_shade; ++ch)
            if ((e = chain(2, c->d_SP, shade_cnt, 4, ch * lchunk)) != hipSuccess) return e;
        return launch_shade_l(c->d_rargs, Q, c->d_lsdf, shade_grid, s);
    };
    const int launches = 2 + max_steps * (int)(1 + nch_march * nl) + (int)(nch_shade * nl) + 1;
    HIPCHK(c, hipEventRecord(c->ev0, s));
    HIPCHK(c, launch_set_args(A, c->d_rargs, s));
    if ((rc = prof_begin(c, 1, s)) != NR_OK) return rc;
    // graph unless: long caps, the legacy null stream (not capturable), or debug bit 256
    // (direct launches, for profilers that do not follow graph launches)
    if (max_steps <= 1024 && s != nullptr && !(c->debug & 256)) {
        const std::vector<long long> key = {A.W, A.rows, A.band, A.nshards, A.shard, max_steps, c->net_ver, lchunk,
                                            (long long)(uintptr_t)c->d_P[0], (long long)(uintptr_t)c->d_ctr,
                                            (long long)(uintptr_t)c->d_lsdf, (long long)(uintptr_t)c->d_lz,
                                            (long long)(uintptr_t)c->d_SP, (long long)(uintptr_t)s};
        if (!c->lgraph || key != c->lkey) {
            if (c->lgraph) { HIPCHK(c, hipGraphExecDestroy(c->lgraph)); c->lgraph = nullptr; }
            hipGraph_t g = nullptr;
            HIPCHK(c, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            hipError_t e = frame();
            hipError_t e2 = hipStreamEndCapture(s, &g);
            if (e != hipSuccess || e2 != hipSuccess) {
                if (g) (void)hipGraphDestroy(g);
                return set_err(c, NR_E_HIP, "nr_render: layered graph capture failed: %s",
                               hipGetErrorString(e != hipSuccess ? e : e2));
            }
            e = hipGraphInstantiate(&c->lgraph, g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (e != hipSuccess) { c->lgraph = nullptr; return set_err(c, NR_E_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e)); }
            c->lkey = key;
        }
        HIPCHK(c, hipGraphLaunch(c->lgraph, s));
    } else {
        HIPCHK(c, frame());
    }
    if ((rc = prof_end(c, s)) != NR_OK) return rc;
    if (c->profiling) c->prof_renders++;
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if (loc != NR_DEVICE) HIPCHK(c, hipMemcpyAsync(out, A.out, npix * 4, hipMemcpyDeviceToHost, s));
    if (!stats && loc != NR_DEVICE) HIPCHK(c, hipStreamSynchronize(s));
    return queue_stats(c, max_steps, launches, stats, s);
}

// the context's view (nr_set_view) as a frame into `out`
nr_frame context_view(const nr_ctx *c, uint32_t *out) {
    nr_frame v;
    memcpy(v.inv_view, c->inv_view, sizeof v.inv_view);
    memcpy(v.normal, c->normal, sizeof v.normal);
    v.frame = c->frame;
    v.out = out;
    return v;
}

// One frame (shard) of the view `v` into v.out, at precision `prec` on schedule `sched`:
// nr_render_shard with what it takes from the context passed in, so that nr_render_batch's
// frame-by-frame fallback and nr_render_aa's base frame render theirs without touching the context.
int render_frame(nr_ctx *c, const nr_frame &v, int prec, int sched, int W, int H, int band, int nshards, int shard,
                 int max_steps, int loc, nr_stats *stats) {
    int rc;
    if ((rc = check_shape(c, W, H, band, nshards, shard, max_steps)) != NR_OK) return rc;
    if ((rc = check_scene(c)) != NR_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const int rows = nr_shard_rows(H, band, nshards, shard);
    const size_t npix = (size_t)W * rows;
    if (npix == 0) { if (stats) *stats = nr_stats{}; return NR_OK; }
    if ((rc = ensure_rays(c, npix)) != NR_OK) return rc;
    if ((rc = ensure_ctr(c, (size_t)2 * max_steps + 8)) != NR_OK) return rc;
    uint32_t *dout = v.out;
    if (loc != NR_DEVICE) {
        if ((rc = ensure_buf(c, c->d_out, c->cap_out, npix)) != NR_OK) return rc;
        dout = c->d_out;
    }
    RenderArgs A = render_args(c, W, H, rows, band, nshards, shard, max_steps);
    A.out = dout;
    A.frame = v.frame;
    memcpy(A.inv_view, v.inv_view, sizeof A.inv_view);
    memcpy(A.normal, v.normal, sizeof A.normal);
    GET_STREAM(c, s);
    const int cus = num_cus(c->device);
    if (!c->fused || sched == NR_SCHED_LAYERED) return render_layered(c, A, v.out, npix, max_steps, loc, stats, s);
    if (sched != NR_SCHED_PERSISTENT) {
        // the wavefront schedule (render_wavefront) on this one frame
        nr_frame fr = v;
        fr.out = dout;
        if ((rc = render_wavefront(c, &fr, 1, W, H, band, nshards, shard, max_steps, NR_DEVICE, stats, s)) != NR_OK)
            return rc;
        if (loc != NR_DEVICE) {
            HIPCHK(c, hipMemcpyAsync(v.out, dout, npix * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
        }
        return NR_OK;
    }
    TraceArgs T;
    if ((rc = trace_args(c, prec, W, rows, band, 1, npix, max_steps, T)) != NR_OK) return rc;
    T.itmap = (c->debug & 8) != 0;
    if (c->debug & 1) T.eg_tau = 0.0f;  // the stamps instance (nr_set_debug bit 0) marches without the endgame
    if (c->temporal || c->probe_steps > 0)
        if ((rc = order_buffers(c, W, H, band, nshards, shard, T.nblocks)) != NR_OK) return rc;
    const bool probe = c->probe_steps > 0 && max_steps > 0 && !(c->temporal && c->order_valid);
    const int grid = trace_grid(c, prec, T, npix, 1, cus);
    if (c->debug & 1) {
        if (!c->d_stamps) HIPCHK(c, hipMalloc(&c->d_stamps, (size_t)cus * 16 * 4 * 16 * 8));
        T.stamps = c->d_stamps;
        c->n_stamps = (size_t)grid * 4;
    }
    const MlpArgs M = mlp_for_frames(c, nullptr, 0, A.frame);
    HIPCHK(c, hipEventRecord(c->ev0, s));
    HIPCHK(c, hipMemsetAsync(c->d_tr, 0, (probe ? 2 : 1) * TR_BYTES, s));
    if (probe) {
        // cost probe: march each block's centre ray for at most probe_steps iterations,
        // then hand the blocks out longest-first
        if ((rc = prof_begin(c, 0, s)) != NR_OK) return rc;
        HIPCHK(c, hipMemsetAsync(c->d_bcost, 0, (size_t)T.nblocks * 4, s));
        TraceArgs P = T;
        P.probe = 1;
        P.take = c->probe_take;
        P.lane_cap = lane_cap_for(P.take);
        P.pix_ctr = c->d_tr + TR_BYTES / 4;
        P.stats = reinterpret_cast<unsigned long long *>(c->d_tr + TR_BYTES / 4 + NR_MAX_QUEUES * 32);
        P.stamps = nullptr;
        P.bcost = c->d_bcost;
        P.spread_shift = 0;
        RenderArgs Ap = A;
        Ap.max_steps = std::min(max_steps, c->probe_steps);
        const long pwaves = ((long)T.nblocks + P.take - 1) / P.take;
        const int pgrid = (int)std::max<long>(1, std::min<long>((pwaves + 3) / 4, grid));
        HIPCHK(c, launch_trace(Ap, M, P, prec, pgrid, s));
        HIPCHK(c, launch_order(c->d_bcost, c->d_order[c->order_cur], T.nblocks, T.bw, c->probe_dilate, s));
        if ((rc = prof_end(c, s)) != NR_OK) return rc;
    }
    if ((rc = order_begin(c, T, s)) != NR_OK) return rc;
    if (probe) T.order = c->d_order[c->order_cur];  // (no recorded order: the probe's)
    if ((rc = prof_begin(c, 1, s)) != NR_OK) return rc;
    HIPCHK(c, launch_trace(A, M, T, prec, grid, s));
    if ((rc = prof_end(c, s)) != NR_OK) return rc;
    if ((rc = order_end(c, T, s)) != NR_OK) return rc;
    if (c->profiling) c->prof_renders++;
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if (loc != NR_DEVICE) HIPCHK(c, hipMemcpyAsync(v.out, dout, npix * 4, hipMemcpyDeviceToHost, s));
    return trace_stats(c, T, 2, loc, stats, s);
}

}  // namespace

extern "C" {

int nr_abi_version(void) { return NR_ABI_VERSION; }

const char *nr_last_error(const nr_ctx *ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int nr_create(int device, nr_ctx **out) {
    if (!out) return set_err(nullptr, NR_E_INVALID, "nr_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) return set_err(nullptr, NR_E_HIP, "no HIP device available (%s)", hipGetErrorString(e));
    if (device < 0 || device >= ndev) return set_err(nullptr, NR_E_INVALID, "device %d out of range (%d devices)", device, ndev);
    nr_ctx *c = new (std::nothrow) nr_ctx();
    if (!c) return set_err(nullptr, NR_E_NOMEM, "out of host memory");
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipEventCreate(&c->ev0) != hipSuccess ||
        hipEventCreate(&c->ev1) != hipSuccess) {
        delete c;
        return set_err(nullptr, NR_E_HIP, "stream/event creation failed");
    }
    c->use_own = true;  // the private stream is created on first use (cur_stream)
    *out = c;
    return NR_OK;
}

int nr_destroy(nr_ctx *c) {
    if (!c) return NR_OK;
    (void)hipSetDevice(c->device);
    if (!(c->use_own && !c->own_stream)) (void)hipStreamSynchronize(c->stream);
    free_network(c);
    for (int i = 0; i < 2; ++i) { dfree(c->d_P[i]); dfree(c->d_D[i]); dfree(c->d_FP[i]); dfree(c->d_FD[i]); }
    dfree(c->d_SP); dfree(c->d_SD); dfree(c->d_ctr); dfree(c->d_out); dfree(c->d_tr); dfree(c->d_stamps); dfree(c->d_bcost); dfree(c->d_order[0]); dfree(c->d_order[1]); dfree(c->d_io); dfree(c->d_matcap);
    dfree(c->d_rargs); dfree(c->d_lsdf); dfree(c->d_lz);
    dfree(c->d_frames); dfree(c->d_bout);
    dfree(c->d_qs); dfree(c->d_qio);
    dfree(c->d_aas); dfree(c->d_aalist); dfree(c->d_aaacc);
    dfree(c->d_ls); dfree(c->d_lgbuf); dfree(c->d_lao);
    dfree(c->d_ps);
    dfree(c->d_grid); dfree(c->d_mesh); dfree(c->d_mio); dfree(c->d_spb); dfree(c->d_spa);
    if (c->h_frames) (void)hipHostFree(c->h_frames);
    if (c->ev_frames) (void)hipEventDestroy(c->ev_frames);
    if (c->h_ctr) (void)hipHostFree(c->h_ctr);
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    return NR_OK;
}

int nr_set_stream(nr_ctx *c, void *s, int own) {
    if (!c) return set_err(nullptr, NR_E_INVALID, "ctx is NULL");
    c->use_own = own != 0;
    c->stream = own ? c->own_stream : (hipStream_t)s;
    return NR_OK;
}

int nr_synchronize(nr_ctx *c) {
    if (!c) return set_err(nullptr, NR_E_INVALID, "ctx is NULL");
    {
        GET_STREAM(c, s_);
        HIPCHK(c, hipStreamSynchronize(s_));
    }
    return NR_OK;
}

int nr_load_h5(nr_ctx *c, const char *path) {
    if (!c || !path) return set_err(c, NR_E_INVALID, "nr_load_h5: NULL argument");
    std::vector<int> dims;
    std::vector<std::vector<float>> K, B;
    std::string err;
    int rc = h5_read_keras(path, dims, K, B, err);
    if (rc != NR_OK) return set_err(c, rc, "Failed to initialize model (%s): %s", path, err.c_str());
    return set_network(c, std::move(dims), std::move(K), std::move(B));
}

int nr_load_mlp(nr_ctx *c, int nlayers, const int *dims, const float *const *kernels, const float *const *biases) {
    if (!c || nlayers < 1 || !dims || !kernels || !biases) return set_err(c, NR_E_INVALID, "nr_load_mlp: bad arguments");
    std::vector<int> d(dims, dims + nlayers + 1);
    for (int v : d)
        if (v < 1 || v > 4096) return set_err(c, NR_E_INVALID, "nr_load_mlp: layer size %d out of range", v);
    std::vector<std::vector<float>> K(nlayers), B(nlayers);
    for (int l = 0; l < nlayers; ++l) {
        if (!kernels[l] || !biases[l]) return set_err(c, NR_E_INVALID, "nr_load_mlp: NULL layer %d", l);
        K[l].assign(kernels[l], kernels[l] + (size_t)d[l] * d[l + 1]);
        B[l].assign(biases[l], biases[l] + d[l + 1]);
    }
    return set_network(c, std::move(d), std::move(K), std::move(B));
}

int nr_mlp_info(const nr_ctx *c, int *nlayers, int *dims, int *nw, int *nb) {
    if (!c) return set_err(nullptr, NR_E_INVALID, "ctx is NULL");
    int nl = c->dims.empty() ? 0 : (int)c->dims.size() - 1;
    if (nlayers) *nlayers = nl;
    int w = 0, b = 0;
    for (int l = 0; l < nl; ++l) {
        if (dims) dims[l] = c->dims[l];
        w += c->dims[l] * c->dims[l + 1];
        b += c->dims[l + 1];
    }
    if (dims && nl) dims[nl] = c->dims[nl];
    if (nw) *nw = w;
    if (nb) *nb = b;
    return NR_OK;
}

int nr_set_precision(nr_ctx *c, int precision) {
    if (!c) return set_err(nullptr, NR_E_INVALID, "ctx is NULL");
    if (precision < NR_PRECISION_FP32 || precision > NR_PRECISION_FP32X3)
        return set_err(c, NR_E_INVALID, "unknown precision %d", precision);
    c->precision = precision;
    HIPCHK(c, hipSetDevice(c->device));
    return upload_lowp(c);
}

int nr_set_view(nr_ctx *c, const float inv_view[12], const float normal[16], int frame) {
    if (!c || !inv_view || !normal) return set_err(c, NR_E_INVALID, "nr_set_view: NULL argument");
    memcpy(c->inv_view, inv_view, sizeof c->inv_view);
    memcpy(c->normal, normal, sizeof c->normal);
    c->frame = frame;
    return NR_OK;
}

int nr_set_static(nr_ctx *c, int color_type, int num_inputs) {
    if (!c) return set_err(nullptr, NR_E_INVALID, "ctx is NULL");
    if (color_type != NR_COLOR_FACING && color_type != NR_COLOR_MATCAP)
        return set_err(c, NR_E_INVALID, "unknown color type %d", color_type);
    if (num_inputs != 3 && num_inputs != 4) return set_err(c, NR_E_INVALID, "numInputs must be 3 or 4");
    c->color_type = color_type;
    c->num_inputs = num_inputs;
    return NR_OK;
}

int nr_set_scene(nr_ctx *c, int scene) {
    if (!c) return set_err(nullptr, NR_E_INVALID, "ctx is NULL");
    if (scene < NR_SCENE_V1 || scene > NR_SCENE_ROUND) return set_err(c, NR_E_INVALID, "unknown scene %d", scene);
    c->scene = scene;
    return NR_OK;
}

int nr_set_matcap(nr_ctx *c, const uint32_t *rgba, int w, int h) {
    if (!c || !rgba || w < 1 || h < 1) return set_err(c, NR_E_INVALID, "nr_set_matcap: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    dfree(c->d_matcap);
    HIPCHK(c, hipMalloc(&c->d_matcap, (size_t)w * h * 4));
    HIPCHK(c, hipMemcpy(c->d_matcap, rgba, (size_t)w * h * 4, hipMemcpyHostToDevice));
    c->mw = w; c->mh = h;
    return NR_OK;
}

int nr_render_batch(nr_ctx *c, const nr_frame *frames, int nframes, int W, int H, int band, int nshards, int shard,
                    int max_steps, int loc, nr_stats *stats) {
    if (!c || !frames || nframes < 1) return set_err(c, NR_E_INVALID, "nr_render_batch: bad arguments");
    for (int i = 0; i < nframes; ++i)
        if (!frames[i].out) return set_err(c, NR_E_INVALID, "nr_render_batch: frame %d has no output", i);
    int rc;
    if ((rc = check_shape(c, W, H, band, nshards, shard, max_steps)) != NR_OK) return rc;
    const bool wavefront = c->schedule == NR_SCHED_WAVEFRONT && c->fused;
    if (!wavefront && (c->schedule != NR_SCHED_PERSISTENT || !c->fused || (c->debug & (1 | 8)))) {
        // frame by frame (the layered schedule, a network the fused kernels do not take and the
        // diagnostics are single-frame)
        nr_stats tot{};
        for (int i = 0; i < nframes; ++i) {
            nr_stats st{};
            rc = render_frame(c, frames[i], c->precision, c->schedule, W, H, band, nshards, shard, max_steps, loc,
                              stats ? &st : nullptr);
            if (rc != NR_OK) return rc;
            tot.ray_steps += st.ray_steps; tot.shade_evals += st.shade_evals; tot.rays_hit += st.rays_hit;
            tot.rays_shaded += st.rays_shaded; tot.iterations = std::max(tot.iterations, st.iterations);
            tot.launches += st.launches; tot.ms_total += st.ms_total; tot.endgame_evals += st.endgame_evals;
            tot.endgame_switches += st.endgame_switches;
        }
        if (stats) *stats = tot;
        return NR_OK;
    }
    if ((rc = check_scene(c)) != NR_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (wavefront) {
        GET_STREAM(c, s);
        return render_wavefront(c, frames, nframes, W, H, band, nshards, shard, max_steps, loc, stats, s);
    }
    const int rows = nr_shard_rows(H, band, nshards, shard);
    const size_t npix = (size_t)W * rows;
    if (npix == 0) { if (stats) *stats = nr_stats{}; return NR_OK; }
    GET_STREAM(c, s);
    const int chunk = nr_batch_frames_per_launch(W, H, band, nshards, shard, nframes, 1 << c->nq_shift);
    if (chunk < 1)
        return set_err(c, NR_E_INVALID, "nr_render_batch: %dx%d shard overflows the 32-bit pixel queue", W, H);
    if ((rc = upload_frames(c, frames, nframes, npix, loc, chunk, s)) != NR_OK) return rc;
    // out, frame and the view stay clear: the frames' are in their FrameArgs
    const RenderArgs A = render_args(c, W, H, rows, band, nshards, shard, max_steps);
    const MlpArgs M = mlp_for_frames(c, frames, nframes, 0);
    TraceArgs T;
    if ((rc = trace_args(c, c->precision, W, rows, band, nframes, npix, max_steps, T)) != NR_OK) return rc;
    const int cus = num_cus(c->device);
    if (c->temporal && (rc = order_buffers(c, W, H, band, nshards, shard, T.nblocks)) != NR_OK) return rc;
    HIPCHK(c, hipEventRecord(c->ev0, s));
    int launches = 0;
    for (int f0 = 0; f0 < nframes; f0 += chunk) {
        const int n = std::min(chunk, nframes - f0);
        T.frames = c->d_frames + f0;
        T.nframes = n;
        T.inv_nframes = 1.0 / (double)n;
        // frames interleaved in 64-position chunks: every frame of the launch progresses
        // together, so the launch does not end on one frame's silhouette rays started last
        // (1024^2 x 32 frames 1.866 -> 1.825 ms/frame, one 8-way shard x 8 frames 0.367 ->
        // 0.334; profiles/r2_ab_experiments.txt (10)).  Debug bit 10: frame-major (A/B).
        T.interleave = !((c->debug >> 10) & 1);
        // the counters restart for every launch; the statistics accumulate
        HIPCHK(c, hipMemsetAsync(c->d_tr, 0, f0 == 0 ? TR_BYTES : (size_t)NR_MAX_QUEUES * 128, s));
        // workgroups per CU: default_bpc (with several frames in a launch their tails overlap,
        // so the extra waves per SIMD lift the bulk rate instead of lengthening the tail)
        const int grid = trace_grid(c, c->precision, T, npix * n, n, cus);
        if ((rc = order_begin(c, T, s)) != NR_OK) return rc;
        if ((rc = prof_begin(c, 1, s)) != NR_OK) return rc;
        HIPCHK(c, launch_trace(A, M, T, c->precision, grid, s));
        if ((rc = prof_end(c, s)) != NR_OK) return rc;
        if ((rc = order_end(c, T, s)) != NR_OK) return rc;
        ++launches;
        if (loc != NR_DEVICE)
            for (int i = f0; i < f0 + n; ++i)
                HIPCHK(c, hipMemcpyAsync(frames[i].out, c->d_bout + (size_t)(i % chunk) * npix, npix * 4,
                                         hipMemcpyDeviceToHost, s));
    }
    if (c->profiling) c->prof_renders += nframes;
    HIPCHK(c, hipEventRecord(c->ev1, s));
    return trace_stats(c, T, launches, loc, stats, s);
}

int nr_render_shard(nr_ctx *c, uint32_t *out, int W, int H, int band, int nshards, int shard, int max_steps, int loc,
                    nr_stats *stats) {
    if (!c || !out) return set_err(c, NR_E_INVALID, "nr_render: NULL argument");
    return render_frame(c, context_view(c, out), c->precision, c->schedule, W, H, band, nshards, shard, max_steps, loc,
                        stats);
}

int nr_render(nr_ctx *c, uint32_t *out, int W, int H, int max_steps, int loc, nr_stats *stats) {
    return nr_render_shard(c, out, W, H, H > 0 ? H : 1, 1, 0, max_steps, loc, stats);
}

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
static int query_grid(const nr_ctx *c, size_t n) {
    const int bpc = c->blocks_per_cu > 0 ? c->blocks_per_cu : 2;
    return (int)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, (size_t)num_cus(c->device) * bpc));
}

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
    if (!c->d_qs) HIPCHK(c, hipMalloc(&c->d_qs, 128 + 4 * 8));
    QueryArgs Q = query_args(c, n, W, H, max_steps);
    Q.origins = origins; Q.dirs = dirs;
    Q.status = status; Q.steps = steps; Q.t = t; Q.position = position; Q.normal = normal;
    const size_t N = (size_t)n;
    if (loc != NR_DEVICE) {
        // staging, in floats: the rays, then every output the caller asked for
        const size_t need = (origins ? 6 * N : 0) + (status ? N : 0) + (steps ? N : 0) + (t ? N : 0) +
                            (position ? 3 * N : 0) + (normal ? 3 * N : 0);
        int rc;
        if ((rc = ensure_buf(c, c->d_qio, c->cap_qio, need)) != NR_OK) return rc;
        float *q = c->d_qio;
        if (origins) {
            HIPCHK(c, hipMemcpyAsync(q, origins, 3 * N * 4, hipMemcpyHostToDevice, s));
            HIPCHK(c, hipMemcpyAsync(q + 3 * N, dirs, 3 * N * 4, hipMemcpyHostToDevice, s));
            Q.origins = q; Q.dirs = q + 3 * N;
            q += 6 * N;
        }
        if (status) { Q.status = reinterpret_cast<int32_t *>(q); q += N; }
        if (steps) { Q.steps = reinterpret_cast<int32_t *>(q); q += N; }
        if (t) { Q.t = q; q += N; }
        if (position) { Q.position = q; q += 3 * N; }
        if (normal) { Q.normal = q; q += 3 * N; }
    }
    HIPCHK(c, hipEventRecord(c->ev0, s));
    HIPCHK(c, hipMemsetAsync(c->d_qs, 0, 128 + 4 * 8, s));
    HIPCHK(c, launch_query(Q, c->mlp16, query_grid(c, N), s));
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if (loc != NR_DEVICE) {
        if (status) HIPCHK(c, hipMemcpyAsync(status, Q.status, N * 4, hipMemcpyDeviceToHost, s));
        if (steps) HIPCHK(c, hipMemcpyAsync(steps, Q.steps, N * 4, hipMemcpyDeviceToHost, s));
        if (t) HIPCHK(c, hipMemcpyAsync(t, Q.t, N * 4, hipMemcpyDeviceToHost, s));
        if (position) HIPCHK(c, hipMemcpyAsync(position, Q.position, 3 * N * 4, hipMemcpyDeviceToHost, s));
        if (normal) HIPCHK(c, hipMemcpyAsync(normal, Q.normal, 3 * N * 4, hipMemcpyDeviceToHost, s));
    }
    unsigned long long hs[4];
    if (stats) HIPCHK(c, hipMemcpyAsync(hs, Q.stats, sizeof hs, hipMemcpyDeviceToHost, s));
    const int rc = end_timed(c, stats != nullptr, loc, s, &st.ms_total);
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

// ---- adaptive antialiasing (nr_aa.hip) ----

// The base frame is nr_render's fp32 persistent render into the output buffer; the edge rule, the
// sub-sample tracer and the resolve follow on the same stream.  One host read of the edge count
// sizes the accumulators and the tracer's launch (none when there is no edge).
constexpr int AA_BPC = 2;  // workgroups per CU of the sub-sample tracer's grid by default
int nr_render_aa(nr_ctx *c, uint32_t *out, int W, int H, int samples, int mode, int contrast, int max_steps, int loc,
                 long *edge_pixels, nr_stats *stats) {
    if (!c || !out) return set_err(c, NR_E_INVALID, "nr_render_aa: NULL argument");
    if (W < 1 || H < 1) return set_err(c, NR_E_INVALID, "nr_render_aa: bad size %dx%d", W, H);
    if (samples < 1 || samples > 8) return set_err(c, NR_E_INVALID, "nr_render_aa: samples = %d outside 1..8", samples);
    if (mode != NR_AA_ADAPTIVE && mode != NR_AA_FULL) return set_err(c, NR_E_INVALID, "nr_render_aa: unknown mode %d", mode);
    if (contrast < 0 || contrast > 255) return set_err(c, NR_E_INVALID, "nr_render_aa: contrast = %d outside 0..255", contrast);
    if ((long)samples * W > (1l << 30) || (long)samples * H > (1l << 30) ||
        ((long)samples * W) * ((long)samples * H) > (1l << 30))
        return set_err(c, NR_E_INVALID, "nr_render_aa: %d x %d samples of a %dx%d frame exceed 2^30", samples, samples, W, H);
    if (max_steps < 0) return set_err(c, NR_E_INVALID, "nr_render_aa: max_steps < 0");
    if (c->dims.empty()) return set_err(c, NR_E_STATE, "nr_render_aa: no network loaded");
    if (!c->fused)
        return set_err(c, NR_E_FORMAT, "nr_render_aa: needs a [3|4, 32, ..., 32, 1] network (no layered fallback)");
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    const size_t npix = (size_t)W * H;
    int rc;
    uint32_t *dout = out;
    if (loc != NR_DEVICE) {
        if ((rc = ensure_buf(c, c->d_out, c->cap_out, npix)) != NR_OK) return rc;
        dout = c->d_out;
    }
    // ---- the base frame: always the fp32 persistent tracer, whatever the context's settings
    nr_stats st{};
    rc = render_frame(c, context_view(c, dout), NR_PRECISION_FP32, NR_SCHED_PERSISTENT, W, H, H, 1, 0, max_steps, NR_DEVICE,
                      stats ? &st : nullptr);
    if (rc != NR_OK) return rc;
    const int S = samples;
    const bool full = mode == NR_AA_FULL;
    long nedge = 0;
    float ms_aa = 0.0f;
    unsigned long long hs[4] = {0, 0, 0, 0};
    if (S == 1) {
        nedge = full ? (long)npix : 0;  // one sample per pixel: the base frame is the result
    } else if (full || contrast < 255) {
        if (!c->d_aas) HIPCHK(c, hipMalloc(&c->d_aas, 2 * 128 + 4 * 8));
        if ((rc = ensure_buf(c, c->d_aalist, c->cap_aalist, npix)) != NR_OK) return rc;
        AaArgs X{};
        X.out = dout; X.W = W; X.H = H; X.S = S; X.per = S * S - 1;
        X.contrast = contrast; X.full = full ? 1 : 0;
        X.inv_w = 1.0 / (double)W; X.inv_s = 1.0 / (double)S; X.inv_per = 1.0 / (double)X.per;
        X.list = c->d_aalist;
        X.cursor = c->d_aas;
        X.count = c->d_aas + 32;
        X.stats = reinterpret_cast<unsigned long long *>(c->d_aas + 64);
        if (stats) HIPCHK(c, hipEventRecord(c->ev0, s));
        HIPCHK(c, hipMemsetAsync(c->d_aas, 0, 2 * 128 + 4 * 8, s));
        HIPCHK(c, launch_aa_detect(X, s));
        st.launches += 2;
        uint32_t cnt = 0;
        HIPCHK(c, hipMemcpyAsync(&cnt, X.count, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        nedge = (long)cnt;
        if (cnt) {
            if ((rc = ensure_buf(c, c->d_aaacc, c->cap_aaacc, (size_t)cnt)) != NR_OK) return rc;
            X.accum = c->d_aaacc;
            X.nedge = cnt;
            X.inv_nedge = 1.0 / (double)cnt;
            X.nsub = cnt * (uint32_t)X.per;  // < S W * S H <= 2^30
            // the S W x S H frame's arguments, as nr_render builds them
            RenderArgs A = render_args(c, S * W, S * H, S * H, S * H, 1, 0, max_steps);
            A.frame = c->frame;
            memcpy(A.inv_view, c->inv_view, sizeof A.inv_view);
            memcpy(A.normal, c->normal, sizeof A.normal);
            // The grid by the CU count (nr_set_occupancy's workgroups per CU, or AA_BPC), at least 16
            // samples per wave.  Edge samples are few and long: a launch whose samples fill at most 2x
            // its waves' 64-ray slots is mostly tail, and there a wave fills only its 32 lowest lanes
            // (or 16, when that deals every sample at once) and refills -- an iteration costs less the
            // fewer tiles it holds (wave_rays_for's rule for the frame tracer; nr_set_wave_rays
            // overrides, in whole tiles).  1024^2, S = 2, 92,820 samples: 1.94 ms at 64, 1.55 at 48,
            // 1.34 at 32; S = 4, 464,100 samples: 4.03 at 64, 4.40 at 32.
            const int bpc = c->blocks_per_cu > 0 ? c->blocks_per_cu : AA_BPC;
            const size_t waves64 = ((size_t)X.nsub + 63) / 64;
            const int grid = (int)std::max<size_t>(1, std::min<size_t>(waves64, (size_t)num_cus(c->device) * bpc));
            const size_t slots = (size_t)grid * 4 * 64;
            const size_t per_wave = ((size_t)X.nsub + (size_t)grid * 4 - 1) / ((size_t)grid * 4);
            if (c->wave_rays > 0) X.take = std::min(64, (c->wave_rays + 15) / 16 * 16);
            else X.take = (size_t)X.nsub > 2 * slots ? 64 : (per_wave <= 16 ? 16 : 32);
            HIPCHK(c, hipMemsetAsync(c->d_aaacc, 0, (size_t)cnt * 8, s));
            HIPCHK(c, launch_aa_trace(A, X, c->mlp16, grid, s));
            HIPCHK(c, launch_aa_resolve(X, s));
            st.launches += 3;
            if (stats) HIPCHK(c, hipMemcpyAsync(hs, X.stats, sizeof hs, hipMemcpyDeviceToHost, s));
        }
        if (stats) {
            HIPCHK(c, hipEventRecord(c->ev1, s));
            HIPCHK(c, hipStreamSynchronize(s));
            HIPCHK(c, hipEventElapsedTime(&ms_aa, c->ev0, c->ev1));
        }
    }
    if (loc != NR_DEVICE) {
        HIPCHK(c, hipMemcpyAsync(out, dout, npix * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
    }
    if (edge_pixels) *edge_pixels = nedge;
    if (stats) {
        st.ray_steps += hs[0];
        st.rays_hit += hs[1];
        st.iterations = std::max(st.iterations, (int32_t)hs[2]);
        st.rays_shaded += hs[3];
        st.shade_evals += 4ull * hs[3];
        st.ms_total += ms_aa;
        *stats = st;
    }
    return NR_OK;
}

// ---- ambient occlusion and soft shadows (nr_light.hip) ----

// The checks on the fields of a light, shared by nr_render_lit and nr_compose_render_lit.
static int check_light(nr_ctx *c, const char *fn, const nr_light &l) {
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
    if (!c->d_qs) HIPCHK(c, hipMalloc(&c->d_qs, 128 + 4 * 8));
    if (!c->d_ls) HIPCHK(c, hipMalloc(&c->d_ls, 128 + 4 * 8));
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
    HIPCHK(c, hipMemsetAsync(c->d_qs, 0, 128 + 4 * 8, s));
    HIPCHK(c, launch_query(Q, c->mlp16, grid, s));
    HIPCHK(c, hipMemsetAsync(c->d_ls, 0, 128 + 4 * 8, s));
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

// ---- volume sampling and isosurface extraction (nr_mesh.hip) ----

// The lattice arguments: every dim >= min_dim and at most 2^30 points.
static int lattice_check(nr_ctx *c, const char *fn, const float *origin, const float *step, const int *dims, int min_dim) {
    if (!origin || !step || !dims) return set_err(c, NR_E_INVALID, "%s: NULL lattice arguments", fn);
    long n = 1;
    for (int a = 0; a < 3; ++a) {
        if (dims[a] < min_dim) return set_err(c, NR_E_INVALID, "%s: dims[%d] = %d < %d", fn, a, dims[a], min_dim);
        n *= dims[a];  // (at most 2^30 * 2^31 before the test)
        if (n > (1l << 30)) return set_err(c, NR_E_INVALID, "%s: more than 2^30 lattice points", fn);
    }
    return NR_OK;
}

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
    const int bpc = c->blocks_per_cu > 0 ? c->blocks_per_cu : 12;
    const size_t N = (size_t)L.n;
    const int grid = (int)std::max<size_t>(1, std::min<size_t>((N + 255) / 256, (size_t)num_cus(c->device) * bpc));
    HIPCHK(c, launch_grid(G, c->mlp16, grid, s));
    return NR_OK;
}

// The brick samplers of a composed scene (k_compose_sp_coarse; sample: k_compose_sp_sample), one launch on s.
static int compose_sparse_sampler(nr_compose *cp, const SparseArgs &A, bool sample, hipStream_t s);
// The vertex pass of a composed scene (k_compose_vertex; defined with the nr_compose_* calls below):
// normals and / or owners of the nv device vertices, one launch on s.
static int compose_vertex_pass(nr_compose *cp, const float *d_vertices, float *d_normals, int32_t *d_part, size_t nv,
                               hipStream_t s);

// Count, scan and (with output buffers of sufficient capacity) emit over the device lattice d_sdf;
// with `normals` the vertex normals too.  cp: the lattice holds the composed field of cp (whose owner
// is c): the normals are that field's and `part` (may be NULL) gets the vertices' owners.  *launches
// counts the kernels issued.
static int mesh_run(nr_ctx *c, const char *fn, hipStream_t s, const LatticeArgs &L, const float *d_sdf, float iso,
                    float *vertices, float *normals, long v_cap, int32_t *triangles, long t_cap, long *nv, long *nt,
                    int loc, int *launches, nr_compose *cp = nullptr, int32_t *part = nullptr) {
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
    if (loc != NR_DEVICE) {
        if ((rc = ensure_buf(c, c->d_mio, c->cap_mio, V3 * (normals ? 2 : 1) + T3 + (part ? NV : 0))) != NR_OK) return rc;
        dv = c->d_mio;
        dn = normals ? dv + V3 : nullptr;
        dt = reinterpret_cast<int32_t *>(dv + V3 * (normals ? 2 : 1));
        dp = part ? dt + T3 : nullptr;
    }
    A.vertices = dv;
    A.triangles = dt;
    HIPCHK(c, launch_mesh_emit(A, s));
    *launches += 1;
    if (cp) {
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
        const int bpc = c->blocks_per_cu > 0 ? c->blocks_per_cu : 4;
        const int grid = (int)std::max<size_t>(1, std::min<size_t>(((size_t)tot[0] + 63) / 64, (size_t)num_cus(c->device) * bpc));
        HIPCHK(c, launch_vnormal(V, c->mlp16, grid, s));
        *launches += 1;
    }
    if (loc != NR_DEVICE) {
        HIPCHK(c, hipMemcpyAsync(vertices, dv, V3 * 4, hipMemcpyDeviceToHost, s));
        if (normals) HIPCHK(c, hipMemcpyAsync(normals, dn, V3 * 4, hipMemcpyDeviceToHost, s));
        if (part) HIPCHK(c, hipMemcpyAsync(part, dp, NV * 4, hipMemcpyDeviceToHost, s));
        if (T3) HIPCHK(c, hipMemcpyAsync(triangles, dt, T3 * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
    }
    return NR_OK;
}

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

// ---- brick-sparse extraction (nr_sparse.hip) ----

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

// what a brick-sparse extraction did, for the caller's statistics
struct SparseDone {
    uint64_t points = 0;   // the brick-corner lattice plus the active bricks' point sets
    uint64_t active = 0;
    int launches = 0;
    float ms = 0;
};

// nr_extract_mesh_sparse on c's stream and scratch.  cp == NULL: c's network and scene.  cp: the
// composed field of cp (whose owner is c) in the two samplers and the vertex pass, which then
// writes `part` too (may be NULL); the caller has zeroed cp's statistics.  timed: *done gets ms.
static int sparse_run(nr_ctx *c, nr_compose *cp, const char *fn, const float origin[3], const float step[3], const int dims[3],
                      float iso, int brick, float band, float *vertices, float *normals, int32_t *part, int64_t *keys,
                      long v_cap, int32_t *triangles, long t_cap, long *nv, long *nt, long *active_bricks, int loc, bool timed,
                      SparseDone *done) {
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
    if (!cp && (rc = fused_check(c, fn)) != NR_OK) return rc;
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
    const int cus = num_cus(c->device);
    const int bpc = c->blocks_per_cu > 0 ? c->blocks_per_cu : 12;  // as nr_sample_grid
    HIPCHK(c, hipEventRecord(c->ev0, s));
    if (cp) {
        if ((rc = compose_sparse_sampler(cp, A, false, s)) != NR_OK) return rc;
    } else {
        HIPCHK(c, launch_sparse_coarse(A, c->mlp16, (int)std::max<size_t>(1, std::min<size_t>(((size_t)L.ncoarse + 255) / 256, (size_t)cus * bpc)), s));
    }
    HIPCHK(c, launch_sparse_classify_count(A, s));
    MeshArgs scan{};
    scan.nblk = A.nblk_b; scan.cnt = A.bcnt; scan.off = A.boff; scan.total = A.btotal;
    HIPCHK(c, launch_mesh_scan(scan, s));
    int launches = 3;
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
        if (cp) {
            if ((rc = compose_sparse_sampler(cp, A, true, s)) != NR_OK) return rc;
        } else {
            HIPCHK(c, launch_sparse_sample(A, c->mlp16, (int)std::max<size_t>(1, std::min<size_t>(nblk_m, (size_t)cus * bpc)), s));
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
        if (loc != NR_DEVICE) {
            // staging: keys (8-byte aligned) first, then vertices, normals, triangles, owners
            if ((rc = ensure_buf(c, c->d_mio, c->cap_mio, (keys ? 2 * NV : 0) + V3 * (with_normals ? 2 : 1) + T3 + (part ? NV : 0))) != NR_OK) return rc;
            dk = keys ? reinterpret_cast<int64_t *>(c->d_mio) : nullptr;
            dv = c->d_mio + (keys ? 2 * NV : 0);
            dn = with_normals ? dv + V3 : nullptr;
            dt = reinterpret_cast<int32_t *>(dv + V3 * (with_normals ? 2 : 1));
            dp = part ? dt + T3 : nullptr;
        }
        A.vertices = dv;
        A.keys = reinterpret_cast<long long *>(dk);
        A.triangles = dt;
        HIPCHK(c, launch_sparse_mesh_emit(A, s));
        launches += 1;
        if (cp) {
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
            const int vbpc = c->blocks_per_cu > 0 ? c->blocks_per_cu : 4;  // as nr_extract_mesh
            HIPCHK(c, launch_vnormal(V, c->mlp16, (int)std::max<size_t>(1, std::min<size_t>((NV + 63) / 64, (size_t)cus * vbpc)), s));
            launches += 1;
        }
        if (loc != NR_DEVICE) {
            HIPCHK(c, hipMemcpyAsync(vertices, dv, V3 * 4, hipMemcpyDeviceToHost, s));
            if (with_normals) HIPCHK(c, hipMemcpyAsync(normals, dn, V3 * 4, hipMemcpyDeviceToHost, s));
            if (keys) HIPCHK(c, hipMemcpyAsync(keys, dk, NV * 8, hipMemcpyDeviceToHost, s));
            if (part) HIPCHK(c, hipMemcpyAsync(part, dp, NV * 4, hipMemcpyDeviceToHost, s));
            if (T3) HIPCHK(c, hipMemcpyAsync(triangles, dt, T3 * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
        }
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

int nr_assemble_shards(nr_ctx *c, const uint32_t *src, size_t stride, uint32_t *dst, int W, int H, int band,
                       int nshards, int loc) {
    if (!src || !dst || W < 1 || H < 1 || band < 1 || nshards < 1) return set_err(c, NR_E_INVALID, "nr_assemble_shards: bad arguments");
    if (loc == NR_DEVICE) {
        if (!c) return set_err(nullptr, NR_E_INVALID, "device assembly needs a context");
        HIPCHK(c, hipSetDevice(c->device));
        GET_STREAM(c, s);
        HIPCHK(c, launch_assemble(src, stride, dst, W, H, band, nshards, s));
        return NR_OK;
    }
    for (int y = 0; y < H; ++y) {
        int b = y / band, s = b % nshards, lr = (b / nshards) * band + y % band;
        memcpy(dst + (size_t)y * W, src + (size_t)s * stride + (size_t)lr * W, (size_t)W * 4);
    }
    return NR_OK;
}

int nr_pack_x3(int nlayers, const int *dims, const float *const *kernels, const float *const *biases, uint16_t *a,
               long a_cap, float *f, long f_cap, long *a_len, long *f_len, int *ok) {
    if (nlayers < 1 || !dims || !kernels || !biases || !a_len || !f_len || !ok)
        return nr::report_error(NR_E_INVALID, "nr_pack_x3: bad arguments");
    std::vector<int> d(dims, dims + nlayers + 1);
    std::vector<std::vector<float>> K(nlayers), B(nlayers);
    for (int l = 0; l < nlayers; ++l) {
        if (!kernels[l] || !biases[l] || d[l] < 1 || d[l + 1] < 1)
            return nr::report_error(NR_E_INVALID, "nr_pack_x3: layer %d", l);
        K[l].assign(kernels[l], kernels[l] + (size_t)d[l] * d[l + 1]);
        B[l].assign(biases[l], biases[l] + d[l + 1]);
    }
    std::vector<uint16_t> av;
    std::vector<float> fv;
    int k = 0;
    if (!pack_x3_32(d, K, B, av, fv, &k)) return nr::report_error(NR_E_INVALID, "nr_pack_x3: not a fused shape");
    *a_len = (long)av.size();
    *f_len = (long)fv.size();
    *ok = k;
    if (a && a_cap >= (long)av.size()) std::memcpy(a, av.data(), av.size() * 2);
    if (f && f_cap >= (long)fv.size()) std::memcpy(f, fv.data(), fv.size() * 4);
    return NR_OK;
}

int nr_pack_fp32_pruned(int nlayers, const int *dims, const float *const *kernels, const float *const *biases, int mode,
                        float *full, float *pruned, long cap, long *len, int *clamp, int *has_pruned, int *cand,
                        int *ks, int *order, int cap_layers) {
    if (nlayers < 1 || !dims || !kernels || !biases || !len || !clamp || !has_pruned || mode < 0 || mode > 2)
        return nr::report_error(NR_E_INVALID, "nr_pack_fp32_pruned: bad arguments");
    std::vector<int> d(dims, dims + nlayers + 1);
    std::vector<std::vector<float>> K(nlayers), B(nlayers);
    for (int l = 0; l < nlayers; ++l) {
        if (!kernels[l] || !biases[l] || d[l] < 1 || d[l + 1] < 1)
            return nr::report_error(NR_E_INVALID, "nr_pack_fp32_pruned: layer %d", l);
        K[l].assign(kernels[l], kernels[l] + (size_t)d[l] * d[l + 1]);
        B[l].assign(biases[l], biases[l] + d[l + 1]);
    }
    std::vector<float> fv, pv;
    int cl = 0;
    if (!pack_fp32_16(d, K, B, fv, &cl)) return nr::report_error(NR_E_INVALID, "nr_pack_fp32_pruned: not a fused shape");
    PruneInfo P;
    const bool hp = pack_fp32_16_pruned(d, K, B, mode, pv, P);
    *len = (long)fv.size();
    *clamp = cl;
    *has_pruned = hp ? 1 : 0;
    if (full && cap >= (long)fv.size()) std::memcpy(full, fv.data(), fv.size() * 4);
    if (hp && pruned && cap >= (long)pv.size()) std::memcpy(pruned, pv.data(), pv.size() * 4);
    if (hp && cap_layers >= P.nrelu) {
        if (cand) std::copy(P.cand.begin(), P.cand.end(), cand);
        if (ks) std::copy(P.ks.begin(), P.ks.end(), ks);
        if (order) std::copy(P.order.begin(), P.order.end(), order);
    }
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
    size_t need = (loc == NR_DEVICE ? 0 : (size_t)n * (in0 + outn)) + (c->fused ? 0 : (size_t)2 * chunk * maxw);
    if ((rc = ensure_buf(c, c->d_io, c->cap_io, need)) != NR_OK) return rc;
    float *scratch = c->d_io;
    if (loc != NR_DEVICE) {
        float *hx = scratch; scratch += (size_t)n * in0;
        dY = scratch; scratch += (size_t)n * outn;
        HIPCHK(c, hipMemcpyAsync(hx, X, (size_t)n * in0 * 4, hipMemcpyHostToDevice, s));
        dX = hx;
    }
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
    if (loc != NR_DEVICE) {
        HIPCHK(c, hipMemcpyAsync(Y, dY, (size_t)n * outn * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
    }
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
    if (loc != NR_DEVICE) {
        // staging, in floats: the points, then every output the caller asked for
        const size_t need = N * in0 + (value ? N : 0) + (grad ? N * in0 : 0) + (normal ? 3 * N : 0);
        int rc;
        if ((rc = ensure_buf(c, c->d_io, c->cap_io, need)) != NR_OK) return rc;
        float *q = c->d_io;
        HIPCHK(c, hipMemcpyAsync(q, X, N * in0 * 4, hipMemcpyHostToDevice, s));
        G.X = q; q += N * in0;
        if (value) { G.value = q; q += N; }
        if (grad) { G.grad = q; q += N * in0; }
        if (normal) { G.normal = q; q += 3 * N; }
    }
    const MlpArgs M = c->mlp16;
    if (grad_lds_bytes(M, G) > 64 * 1024) return set_err(c, NR_E_FORMAT, "nr_mlp_gradient: the packs exceed 64 KB of LDS");
    // two workgroups per CU are resident (their LDS: the two packs); the grid by the CU count:
    // nr_set_occupancy's workgroups per CU, or GRAD_BPC
    const int bpc = c->blocks_per_cu > 0 ? c->blocks_per_cu : GRAD_BPC;
    const int grid = (int)std::max<size_t>(1, std::min<size_t>((N + 255) / 256, (size_t)num_cus(c->device) * bpc));
    HIPCHK(c, hipEventRecord(c->ev0, s));
    HIPCHK(c, launch_grad(G, M, grid, s));
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if (loc != NR_DEVICE) {
        if (value) HIPCHK(c, hipMemcpyAsync(value, G.value, N * 4, hipMemcpyDeviceToHost, s));
        if (grad) HIPCHK(c, hipMemcpyAsync(grad, G.grad, N * in0 * 4, hipMemcpyDeviceToHost, s));
        if (normal) HIPCHK(c, hipMemcpyAsync(normal, G.normal, 3 * N * 4, hipMemcpyDeviceToHost, s));
    }
    st.ray_steps = (uint64_t)n;
    st.launches = 1;
    const int rc = end_timed(c, stats != nullptr, loc, s, &st.ms_total);
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
    constexpr size_t PS_BYTES = 128 + 4 * 8;
    if (!c->d_ps) HIPCHK(c, hipMalloc(&c->d_ps, PS_BYTES));
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
    if (loc != NR_DEVICE) {
        // staging, in 4-byte words: the points, then every output the caller asked for
        const size_t need = N * in0 + (position ? 3 * N : 0) + (value ? N : 0) + (normal ? 3 * N : 0) +
                            (distance ? N : 0) + (iters ? N : 0) + (status ? N : 0);
        int rc;
        if ((rc = ensure_buf(c, c->d_io, c->cap_io, need)) != NR_OK) return rc;
        float *q = c->d_io;
        HIPCHK(c, hipMemcpyAsync(q, X, N * in0 * 4, hipMemcpyHostToDevice, s));
        A.X = q; q += N * in0;
        if (position) { A.position = q; q += 3 * N; }
        if (value) { A.value = q; q += N; }
        if (normal) { A.normal = q; q += 3 * N; }
        if (distance) { A.distance = q; q += N; }
        if (iters) { A.iters = reinterpret_cast<int32_t *>(q); q += N; }
        if (status) { A.status = reinterpret_cast<int32_t *>(q); q += N; }
    }
    const MlpArgs M = c->mlp16;
    if (project_lds_bytes(M, A) > 64 * 1024)
        return set_err(c, NR_E_FORMAT, "nr_project_points: the packs exceed 64 KB of LDS");
    // two workgroups per CU are resident (their LDS: the two packs), and the launch is persistent:
    // nr_set_occupancy's workgroups per CU, or the resident two
    const int bpc = c->blocks_per_cu > 0 ? c->blocks_per_cu : 2;
    const int grid = (int)std::max<size_t>(1, std::min<size_t>((N + 255) / 256, (size_t)num_cus(c->device) * bpc));
    HIPCHK(c, hipEventRecord(c->ev0, s));
    HIPCHK(c, hipMemsetAsync(c->d_ps, 0, PS_BYTES, s));
    HIPCHK(c, launch_project(A, M, grid, s));
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if (loc != NR_DEVICE) {
        if (position) HIPCHK(c, hipMemcpyAsync(position, A.position, 3 * N * 4, hipMemcpyDeviceToHost, s));
        if (value) HIPCHK(c, hipMemcpyAsync(value, A.value, N * 4, hipMemcpyDeviceToHost, s));
        if (normal) HIPCHK(c, hipMemcpyAsync(normal, A.normal, 3 * N * 4, hipMemcpyDeviceToHost, s));
        if (distance) HIPCHK(c, hipMemcpyAsync(distance, A.distance, N * 4, hipMemcpyDeviceToHost, s));
        if (iters) HIPCHK(c, hipMemcpyAsync(iters, A.iters, N * 4, hipMemcpyDeviceToHost, s));
        if (status) HIPCHK(c, hipMemcpyAsync(status, A.status, N * 4, hipMemcpyDeviceToHost, s));
    }
    unsigned long long hs[3];
    if (stats) HIPCHK(c, hipMemcpyAsync(hs, A.stats, sizeof hs, hipMemcpyDeviceToHost, s));
    const int rc = end_timed(c, stats != nullptr, loc, s, &st.ms_total);
    if (rc != NR_OK || !stats) return rc;
    st.ray_steps = hs[0];
    st.rays_shaded = hs[1];
    st.iterations = (int32_t)hs[2];
    st.launches = 2;  // the counters' memset and k_project
    *stats = st;
    return NR_OK;
}

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
    if (host) {
        // staging, in floats: the rays, then every output the caller asked for
        const size_t need = (origins ? 6 * N : 0) + (status ? N : 0) + (steps ? N : 0) + (t ? N : 0) +
                            (position ? 3 * N : 0) + (normal ? 3 * N : 0) + (part ? N : 0);
        if ((rc = ensure_buf(c, cp->d_io, cp->cap_io, need)) != NR_OK) return rc;
        float *q = cp->d_io;
        if (origins) {
            HIPCHK(c, hipMemcpyAsync(q, origins, 3 * N * 4, hipMemcpyHostToDevice, s));
            HIPCHK(c, hipMemcpyAsync(q + 3 * N, dirs, 3 * N * 4, hipMemcpyHostToDevice, s));
            Q.origins = q; Q.dirs = q + 3 * N;
            q += 6 * N;
        }
        if (status) { Q.status = reinterpret_cast<int32_t *>(q); q += N; }
        if (steps) { Q.steps = reinterpret_cast<int32_t *>(q); q += N; }
        if (t) { Q.t = q; q += N; }
        if (position) { Q.position = q; q += 3 * N; }
        if (normal) { Q.normal = q; q += 3 * N; }
        if (part) { Q.part = reinterpret_cast<int32_t *>(q); q += N; }
    }
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
    if (host) {
        if (status) HIPCHK(c, hipMemcpyAsync(status, Q.status, N * 4, hipMemcpyDeviceToHost, s));
        if (steps) HIPCHK(c, hipMemcpyAsync(steps, Q.steps, N * 4, hipMemcpyDeviceToHost, s));
        if (t) HIPCHK(c, hipMemcpyAsync(t, Q.t, N * 4, hipMemcpyDeviceToHost, s));
        if (position) HIPCHK(c, hipMemcpyAsync(position, Q.position, 3 * N * 4, hipMemcpyDeviceToHost, s));
        if (normal) HIPCHK(c, hipMemcpyAsync(normal, Q.normal, 3 * N * 4, hipMemcpyDeviceToHost, s));
        if (part) HIPCHK(c, hipMemcpyAsync(part, Q.part, N * 4, hipMemcpyDeviceToHost, s));
        if (out) HIPCHK(c, hipMemcpyAsync(out, dout, N * 4, hipMemcpyDeviceToHost, s));
    }
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
    const bool host = loc != NR_DEVICE;
    if (host) {
        int rc;
        if ((rc = ensure_buf(c, cp->d_io, cp->cap_io, 3 * N + (value ? N : 0) + (owner ? N : 0))) != NR_OK) return rc;
        float *q = cp->d_io;
        HIPCHK(c, hipMemcpyAsync(q, points, 3 * N * 4, hipMemcpyHostToDevice, s));
        Q.points = q; q += 3 * N;
        if (value) { Q.value = q; q += N; }
        if (owner) { Q.owner = reinterpret_cast<int32_t *>(q); q += N; }
    }
    // 4-wave workgroups, as many per CU as the packs allow (at most k_query's three)
    const int fit = std::max(1, std::min(3, NR_LDS_PER_CU / std::max(1, Q.pack_bytes)));
    const int bpc = c->blocks_per_cu > 0 ? std::min(c->blocks_per_cu, fit) : fit;
    const int grid = (int)std::max<size_t>(1, std::min<size_t>((N + 255) / 256, (size_t)num_cus(c->device) * bpc));
    HIPCHK(c, hipEventRecord(c->ev0, s));
    HIPCHK(c, hipMemsetAsync(cp->d_cs, 0, COMPOSE_CS_BYTES, s));
    HIPCHK(c, launch_compose_sample(Q, grid, s));
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if (host) {
        if (value) HIPCHK(c, hipMemcpyAsync(value, Q.value, N * 4, hipMemcpyDeviceToHost, s));
        if (owner) HIPCHK(c, hipMemcpyAsync(owner, Q.owner, N * 4, hipMemcpyDeviceToHost, s));
    }
    unsigned long long hs[7];
    if (stats) HIPCHK(c, hipMemcpyAsync(hs, Q.stats, sizeof hs, hipMemcpyDeviceToHost, s));
    float ms = 0.0f;
    const int rc = end_timed(c, stats != nullptr, loc, s, &ms);
    if (rc != NR_OK || !stats) return rc;
    hs[0] = (unsigned long long)N;  // points evaluated
    compose_stats(hs, false, 2, ms, stats);
    return NR_OK;
}

// ---- composed scenes on a lattice (nr_compose_mesh.hip) ----

// The ComposeArgs of the lattice kernels: the packs, nets and parts with the owner's frame and the
// statistics words.  Their workgroup and grid are compose_shape's, over the points of the launch.
static ComposeArgs compose_field_args(const nr_compose *cp) {
    ComposeArgs Q = cp->A;
    Q.frame = cp->owner->frame;
    Q.stats = reinterpret_cast<unsigned long long *>(cp->d_cs + 32);
    return Q;
}

static int compose_sparse_sampler(nr_compose *cp, const SparseArgs &A, bool sample, hipStream_t s) {
    nr_ctx *c = cp->owner;
    const ComposeArgs Q = compose_field_args(cp);
    int threads, grid;
    compose_shape(cp, sample ? (size_t)A.nactive * A.L.stride : (size_t)A.L.ncoarse, threads, grid);
    if (sample) HIPCHK(c, launch_compose_sp_sample(Q, A, grid, threads, s));
    else HIPCHK(c, launch_compose_sp_coarse(Q, A, grid, threads, s));
    return NR_OK;
}

static int compose_vertex_pass(nr_compose *cp, const float *d_vertices, float *d_normals, int32_t *d_part, size_t nv,
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
    if (loc != NR_DEVICE) {
        if ((rc = ensure_buf(c, cp->d_io, cp->cap_io, (value ? N : 0) + (owner ? N : 0))) != NR_OK) return rc;
        dv = value ? cp->d_io : nullptr;
        dw = owner ? reinterpret_cast<int32_t *>(cp->d_io + (value ? N : 0)) : nullptr;
    }
    HIPCHK(c, hipEventRecord(c->ev0, s));
    if ((rc = compose_grid_launch(cp, L, dv, dw, s)) != NR_OK) return rc;
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if (loc != NR_DEVICE) {
        if (value) HIPCHK(c, hipMemcpyAsync(value, dv, N * 4, hipMemcpyDeviceToHost, s));
        if (owner) HIPCHK(c, hipMemcpyAsync(owner, dw, N * 4, hipMemcpyDeviceToHost, s));
    }
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

int nr_layer_forward(nr_ctx *c, int layer, const float *A, float *Z, long n, int loc) {
    if (!c || n < 0 || (n > 0 && (!A || !Z))) return set_err(c, NR_E_INVALID, "nr_layer_forward: bad arguments");
    int nl = c->dims.empty() ? 0 : (int)c->dims.size() - 1;
    if (layer < 0 || layer >= nl) return set_err(c, NR_E_INVALID, "nr_layer_forward: layer %d out of range", layer);
    if (n == 0) return NR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int in = c->dims[layer], out = c->dims[layer + 1];
    GET_STREAM(c, s);
    const float *dA = A;
    float *dZ = Z;
    if (loc != NR_DEVICE) {
        int rc = ensure_buf(c, c->d_io, c->cap_io, (size_t)n * (in + out));
        if (rc != NR_OK) return rc;
        float *ha = c->d_io;
        dZ = c->d_io + (size_t)n * in;
        HIPCHK(c, hipMemcpyAsync(ha, A, (size_t)n * in * 4, hipMemcpyHostToDevice, s));
        dA = ha;
    }
    HIPCHK(c, dense_rows(c->d_W[layer], c->d_b[layer], dA, dZ, n, in, out, layer != nl - 1, num_cus(c->device), s));
    if (loc != NR_DEVICE) {
        HIPCHK(c, hipMemcpyAsync(Z, dZ, (size_t)n * out * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
    }
    return NR_OK;
}

int nr_set_profiling(nr_ctx *c, int on) {
    if (!c) return set_err(nullptr, NR_E_INVALID, "ctx is NULL");
    c->profiling = on != 0;
    return NR_OK;
}

int nr_prof_collect(nr_ctx *c, nr_kernel_prof *out) {
    if (!c || !out) return set_err(c, NR_E_INVALID, "nr_prof_collect: NULL argument");
    HIPCHK(c, hipSetDevice(c->device));
    {
        GET_STREAM(c, s_);
        HIPCHK(c, hipStreamSynchronize(s_));
    }
    nr_kernel_prof p{};
    for (auto &r : c->recs) {
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev_pool[r.e0], c->ev_pool[r.e1]));
        if (r.kind == 0) { p.init_ms += ms; p.init_launches++; }
        else if (r.kind == 1) { p.march_ms += ms; p.march_launches++; }
        else { p.shade_ms += ms; p.shade_launches++; }
    }
    p.renders = c->prof_renders;
    c->recs.clear();
    c->prof_renders = 0;
    *out = p;
    return NR_OK;
}

int nr_set_schedule(nr_ctx *c, int schedule) {
    if (!c) return set_err(nullptr, NR_E_INVALID, "ctx is NULL");
    if (schedule != NR_SCHED_PERSISTENT && schedule != NR_SCHED_WAVEFRONT && schedule != NR_SCHED_LAYERED)
        return set_err(c, NR_E_INVALID, "unknown schedule %d", schedule);
    c->schedule = schedule;
    return NR_OK;
}

int nr_set_temporal_order(nr_ctx *c, int on) {
    if (!c) return set_err(nullptr, NR_E_INVALID, "ctx is NULL");
    c->temporal = on < 0 ? 0 : (on > 2 ? 2 : on);
    c->order_valid = 0;
    return NR_OK;
}

int nr_set_pixel_spread(nr_ctx *c, int group_blocks) {
    if (!c || group_blocks < -1 || group_blocks > 65536 || (group_blocks > 0 && (group_blocks & (group_blocks - 1))))
        return set_err(c, NR_E_INVALID,
                       "nr_set_pixel_spread: group_blocks must be -1 (auto), 0 or a power of two <= 65536");
    c->spread = group_blocks;
    return NR_OK;
}

int nr_set_cost_probe(nr_ctx *c, int max_steps, int rays_per_wave) {
    if (!c || max_steps < 0 || max_steps > 1023 || rays_per_wave < 1 || rays_per_wave > 64)
        return set_err(c, NR_E_INVALID, "nr_set_cost_probe: bad arguments");
    c->probe_steps = max_steps;
    c->probe_take = rays_per_wave;
    c->probe_dilate = (c->debug & 16) ? 0 : 1;
    return NR_OK;
}

int nr_set_layer_chunk(nr_ctx *c, long points) {
    if (!c || points < 0 || (points > 0 && points < 64))
        return set_err(c, NR_E_INVALID, "nr_set_layer_chunk: points must be 0 (auto) or >= 64");
    c->layer_chunk = points;
    return NR_OK;
}

int nr_set_queue_shards(nr_ctx *c, int n) {
    if (!c || n < 1 || n > NR_MAX_QUEUES || (n & (n - 1)))
        return set_err(c, NR_E_INVALID, "nr_set_queue_shards: n must be a power of two in [1, %d]", NR_MAX_QUEUES);
    c->nq_shift = 31 - __builtin_clz((unsigned)n);
    return NR_OK;
}

int nr_set_wave_rays(nr_ctx *c, int rays) {
    if (!c || rays < 0 || rays > 64) return set_err(c, NR_E_INVALID, "nr_set_wave_rays: rays must be in [0, 64]");
    c->wave_rays = rays;
    return NR_OK;
}

int nr_set_occupancy(nr_ctx *c, int blocks_per_cu) {
    if (!c || blocks_per_cu < 0 || blocks_per_cu > 16) return set_err(c, NR_E_INVALID, "nr_set_occupancy: bad arguments");
    c->blocks_per_cu = blocks_per_cu;
    return NR_OK;
}

int nr_set_endgame(nr_ctx *c, float tau) {
    if (!c) return set_err(nullptr, NR_E_INVALID, "ctx is NULL");
    if (!(tau >= 0.0f) || tau > 1e30f) return set_err(c, NR_E_INVALID, "nr_set_endgame: tau must be finite and >= 0");
    c->eg_tau = tau;
    return NR_OK;
}

int nr_set_debug(nr_ctx *c, int flags) {
    if (!c) return set_err(nullptr, NR_E_INVALID, "ctx is NULL");
    c->debug = flags;
    c->no_clamp = (flags >> 9) & 1;
    c->no_stream = (flags >> 11) & 1;
    c->no_s16 = !((flags >> 12) & 1);
    c->mlp16.lps = c->no_s16 ? nullptr : c->d_lps16;
    c->mlp16.lpfs = c->no_s16 ? nullptr : c->d_lpfs16;
    c->fp32_normals = (flags >> 15) & 1;
    c->mlp16.x3n = !c->fp32_normals && c->mlp16.x3lp != nullptr;
    c->mlp16.lp_stream = !c->no_stream;
    c->mlp16.lp_clamp = c->clamp_ok && !c->no_clamp && c->mlp16.lp != nullptr;
    c->mlp16.f32_clamp = c->f32_clamp_ok && !c->no_clamp;
    c->mlp16.pkp = c->mlp16.f32_clamp ? c->d_pkp : nullptr;
    select_unit_pack(c);
    return NR_OK;
}

int nr_set_prune(nr_ctx *c, int mode) {
    if (!c) return set_err(nullptr, NR_E_INVALID, "ctx is NULL");
    if (mode < 0 || mode > 2) return set_err(c, NR_E_INVALID, "nr_set_prune: mode must be 0, 1 or 2");
    if (mode == c->prune_mode) return NR_OK;
    c->prune_mode = mode;
    if (c->dims.empty()) return NR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    {
        GET_STREAM(c, s_);
        HIPCHK(c, hipStreamSynchronize(s_));
    }
    return upload_pruned(c);
}

int nr_prune_info(const nr_ctx *c, int *nrelu, int *cand, int *ks, int *order, int cap_layers) {
    if (!c || !nrelu) return set_err(nullptr, NR_E_INVALID, "nr_prune_info: NULL argument");
    const PruneInfo &P = c->prune;
    *nrelu = P.nrelu;
    if (cap_layers >= P.nrelu) {
        if (cand) std::copy(P.cand.begin(), P.cand.end(), cand);
        if (ks) std::copy(P.ks.begin(), P.ks.end(), ks);
        if (order) std::copy(P.order.begin(), P.order.end(), order);
    }
    return NR_OK;
}

int nr_prune_redos(nr_ctx *c, unsigned long long *redos) {
    if (!c || !redos) return set_err(c, NR_E_INVALID, "nr_prune_redos: NULL argument");
    *redos = 0;
    if (!c->d_tr) return NR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipMemcpy(redos, reinterpret_cast<unsigned long long *>(c->d_tr + NR_MAX_QUEUES * 32) + 6, 8,
                        hipMemcpyDeviceToHost));
    return NR_OK;
}

int nr_set_unit_skip(nr_ctx *c, int on) {
    if (!c) return set_err(nullptr, NR_E_INVALID, "ctx is NULL");
    c->unit_skip = on != 0;
    select_unit_pack(c);
    return NR_OK;
}

int nr_unit_skip_counts(nr_ctx *c, unsigned long long *issued, unsigned long long *skipped) {
    if (!c || !issued || !skipped) return set_err(c, NR_E_INVALID, "nr_unit_skip_counts: NULL argument");
    *issued = *skipped = 0;
    if (!c->d_tr || c->dims.empty()) return NR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    HIPCHK(c, hipStreamSynchronize(s));
    unsigned long long h[2] = {0, 0};  // [7] skipped, [8] wave evaluations of the unit form
    HIPCHK(c, hipMemcpy(h, reinterpret_cast<unsigned long long *>(c->d_tr + NR_MAX_QUEUES * 32) + 7, sizeof h,
                        hipMemcpyDeviceToHost));
    *skipped = h[0];
    *issued = h[1] * (unsigned long long)(c->mlp16.in0 + 32 * c->mlp16.nh);
    return NR_OK;
}

int nr_pack_fp32_units(int nlayers, const int *dims, const float *const *kernels, const float *const *biases, float *pack,
                       long cap, long *len, int *has_pack) {
    if (nlayers < 1 || !dims || !kernels || !biases || !len || !has_pack)
        return nr::report_error(NR_E_INVALID, "nr_pack_fp32_units: bad arguments");
    std::vector<int> d(dims, dims + nlayers + 1);
    std::vector<std::vector<float>> K(nlayers), B(nlayers);
    for (int l = 0; l < nlayers; ++l) {
        if (!kernels[l] || !biases[l] || d[l] < 1 || d[l + 1] < 1)
            return nr::report_error(NR_E_INVALID, "nr_pack_fp32_units: layer %d", l);
        K[l].assign(kernels[l], kernels[l] + (size_t)d[l] * d[l + 1]);
        B[l].assign(biases[l], biases[l] + d[l + 1]);
    }
    std::vector<float> pv;
    const bool hp = pack_fp32_units(d, K, B, pv);
    *has_pack = hp ? 1 : 0;
    *len = hp ? (long)pv.size() : 0;
    if (hp && pack && cap >= (long)pv.size()) std::memcpy(pack, pv.data(), pv.size() * 4);
    return NR_OK;
}

int nr_debug_stamps(nr_ctx *c, unsigned long long *out, size_t cap, size_t *n) {
    if (!c || !n) return set_err(c, NR_E_INVALID, "nr_debug_stamps: NULL argument");
    *n = c->n_stamps;
    if (!out || !c->d_stamps) return NR_OK;
    {
        GET_STREAM(c, s_);
        HIPCHK(c, hipStreamSynchronize(s_));
    }
    size_t m = std::min(cap / 16, c->n_stamps);
    HIPCHK(c, hipMemcpy(out, c->d_stamps, m * 16 * 8, hipMemcpyDeviceToHost));
    return NR_OK;
}

int nr_set_poll_interval(nr_ctx *c, int every) {
    if (!c || every < 0) return set_err(c, NR_E_INVALID, "nr_set_poll_interval: bad arguments");
    c->check_every = every;
    return NR_OK;
}

int nr_dense_forward(nr_ctx *c, const float *W, const float *b, int in, int out, int relu, const float *A, float *Z,
                     long n, int loc) {
    if (!c || !W || !b || in < 1 || out < 1 || n < 0 || (n > 0 && (!A || !Z)))
        return set_err(c, NR_E_INVALID, "nr_dense_forward: bad arguments");
    if (n == 0) return NR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    if (loc == NR_DEVICE) {
        HIPCHK(c, dense_rows(W, b, A, Z, n, in, out, relu, num_cus(c->device), s));
        return NR_OK;
    }
    // host buffers: stage everything
    size_t need = (size_t)in * out + out + (size_t)n * (in + out);
    int rc = ensure_buf(c, c->d_io, c->cap_io, need);
    if (rc != NR_OK) return rc;
    float *dW = c->d_io, *db = dW + (size_t)in * out, *dA = db + out, *dZ = dA + (size_t)n * in;
    HIPCHK(c, hipMemcpyAsync(dW, W, (size_t)in * out * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(db, b, (size_t)out * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(dA, A, (size_t)n * in * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, dense_rows(dW, db, dA, dZ, n, in, out, relu, num_cus(c->device), s));
    HIPCHK(c, hipMemcpyAsync(Z, dZ, (size_t)n * out * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return NR_OK;
}

int nr_camera(float rx, float ry, float zoom, float tx, float ty, float inv_view[12], float normal[16]) {
    return nr_camera_ex(rx, ry, zoom, tx, ty, NR_CAMERA_F64, inv_view, normal);
}

int nr_camera_ex(float rx, float ry, float zoom, float tx, float ty, int mode, float inv_view[12], float normal[16]) {
    if (!inv_view || !normal) return set_err(nullptr, NR_E_INVALID, "nr_camera: NULL output");
    if (mode == NR_CAMERA_F64) camera_matrices(rx, ry, zoom, tx, ty, inv_view, normal);
    else if (mode == NR_CAMERA_EIGEN) camera_matrices_eigen(rx, ry, zoom, tx, ty, inv_view, normal);
    else return set_err(nullptr, NR_E_INVALID, "nr_camera_ex: unknown mode %d", mode);
    return NR_OK;
}

int nr_h5_read_keras(const char *path, int max_layers, int *nlayers, int *dims, float *params, size_t cap) {
    if (!path || !nlayers) return set_err(nullptr, NR_E_INVALID, "nr_h5_read_keras: NULL argument");
    std::vector<int> d;
    std::vector<std::vector<float>> K, B;
    std::string err;
    int rc = h5_read_keras(path, d, K, B, err);
    if (rc != NR_OK) return set_err(nullptr, rc, "%s", err.c_str());
    int nl = (int)d.size() - 1;
    *nlayers = nl;
    if (dims) {
        if (max_layers < nl) return set_err(nullptr, NR_E_INVALID, "nr_h5_read_keras: %d layers > max_layers", nl);
        for (int i = 0; i <= nl; ++i) dims[i] = d[i];
    }
    if (params) {
        size_t need = 0;
        for (int l = 0; l < nl; ++l) need += K[l].size() + B[l].size();
        if (cap < need) return set_err(nullptr, NR_E_INVALID, "nr_h5_read_keras: params buffer too small (%zu < %zu)", cap, need);
        float *p = params;
        for (int l = 0; l < nl; ++l) {
            memcpy(p, K[l].data(), K[l].size() * 4); p += K[l].size();
            memcpy(p, B[l].data(), B[l].size() * 4); p += B[l].size();
        }
    }
    return NR_OK;
}

int nr_png_load(const char *path, uint32_t **rgba, int *w, int *h) {
    if (!path || !rgba || !w || !h) return set_err(nullptr, NR_E_INVALID, "nr_png_load: NULL argument");
    std::vector<uint32_t> px;
    std::string err;
    int rc = png_decode(path, px, *w, *h, err);
    if (rc != NR_OK) return set_err(nullptr, rc, "Error reading png: %s", err.c_str());
    *rgba = (uint32_t *)malloc(px.size() * 4);
    if (!*rgba) return set_err(nullptr, NR_E_NOMEM, "out of memory");
    memcpy(*rgba, px.data(), px.size() * 4);
    return NR_OK;
}

int nr_png_save(const char *path, const uint32_t *rgba, int w, int h, int flip) {
    if (!path || !rgba) return set_err(nullptr, NR_E_INVALID, "nr_png_save: NULL argument");
    std::string err;
    int rc = png_encode(path, rgba, w, h, flip, err);
    if (rc != NR_OK) return set_err(nullptr, rc, "[ERROR] Unable to save png: %s", err.c_str());
    return NR_OK;
}

int nr_ppm_save(const char *path, const uint32_t *rgba, int w, int h) {
    if (!path || !rgba || w < 1 || h < 1) return set_err(nullptr, NR_E_INVALID, "nr_ppm_save: bad arguments");
    std::string err;
    int rc = ppm_encode(path, rgba, w, h, err);
    if (rc != NR_OK) return set_err(nullptr, rc, "%s", err.c_str());
    return NR_OK;
}

void nr_free(void *p) { free(p); }

}  // extern "C"

// ---- fitting (nr_fit_*; nr_fit.hip) ----
// Master weights, Adam's moments, the fit pack and the partial sums live on the device; a step is
// two launches (k_fit_grad, k_fit_update) whose arguments carry the step's constants, so a run
// enqueues and never reads back.
struct nr_fit {
    nr_ctx *owner = nullptr;
    int nh = 0, P = 0, S = 0, grid = 0;
    nr_fit_opts o{};
    long step = 0;
    float *d_theta = nullptr, *d_m = nullptr, *d_v = nullptr, *d_pack = nullptr, *d_partial = nullptr;
    float *d_out = nullptr;       // nr_fit_gradient's gradient [P] and loss [1] for host callers
    float *d_io = nullptr;        // staging of host points, targets, values and losses
    size_t cap_io = 0;
};

namespace {
FitArgs fit_grad_args(const nr_fit *f, const float *X, const float *Y, long n, float *value) {
    FitArgs F{};
    F.X = X; F.Y = Y; F.n = n;
    F.pack = f->d_pack; F.partial = f->d_partial; F.value = value;
    F.clamp = f->o.clamp; F.S = f->S; F.nh = f->nh;
    return F;
}
FitUpdArgs fit_upd_args(const nr_fit *f, int mode, long n) {
    FitUpdArgs U{};
    U.partial = f->d_partial;
    U.S = f->S; U.nh = f->nh; U.mode = mode;
    U.inv_n = n > 0 ? 1.0f / (float)n : 0.0f;
    U.theta = f->d_theta; U.m = f->d_m; U.v = f->d_v; U.pack = f->d_pack;
    return U;
}
}  // namespace

extern "C" {

int nr_fit_create(nr_ctx *owner, int nlayers, const int *dims, const float *const *kernels, const float *const *biases,
                  const nr_fit_opts *opts, nr_fit **out) {
    if (out) *out = nullptr;
    if (!owner || !dims || !kernels || !biases || !opts || !out) return set_err(owner, NR_E_INVALID, "nr_fit_create: NULL argument");
    if (nlayers < 1) return set_err(owner, NR_E_INVALID, "nr_fit_create: %d layers", nlayers);
    for (int l = 0; l < nlayers; ++l)
        if (!kernels[l] || !biases[l]) return set_err(owner, NR_E_INVALID, "nr_fit_create: NULL layer %d", l);
    const nr_fit_opts &o = *opts;
    if (!(std::isfinite(o.lr) && o.lr > 0.0f)) return set_err(owner, NR_E_INVALID, "nr_fit_create: lr must be finite and positive");
    if (!(o.beta1 >= 0.0f && o.beta1 < 1.0f) || !(o.beta2 >= 0.0f && o.beta2 < 1.0f))
        return set_err(owner, NR_E_INVALID, "nr_fit_create: beta1 and beta2 must lie in [0, 1)");
    if (!(std::isfinite(o.eps) && o.eps > 0.0f)) return set_err(owner, NR_E_INVALID, "nr_fit_create: eps must be finite and positive");
    if (!(std::isfinite(o.clamp) && o.clamp >= 0.0f)) return set_err(owner, NR_E_INVALID, "nr_fit_create: clamp must be finite and not negative");
    if (o.partials < 0 || o.partials > 4096) return set_err(owner, NR_E_INVALID, "nr_fit_create: partials = %d outside 0..4096", o.partials);
    if (o.grid < 0) return set_err(owner, NR_E_INVALID, "nr_fit_create: grid = %d is negative", o.grid);
    const int nh = nlayers - 2;
    bool shape = nlayers >= 2 && nh <= GRAD_MAX_HIDDEN && dims[0] == 3 && dims[nlayers] == 1;
    for (int l = 1; l < nlayers && shape; ++l) shape = dims[l] == 32;
    if (!shape) return set_err(owner, NR_E_FORMAT, "nr_fit_create: needs a [3, 32, ..., 32, 1] network with at most %d hidden 32 x 32 layers", GRAD_MAX_HIDDEN);
    nr_fit *f = new (std::nothrow) nr_fit();
    if (!f) return set_err(owner, NR_E_NOMEM, "out of host memory");
    f->owner = owner;
    f->nh = nh;
    f->P = fit_params(nh);
    f->S = o.partials > 0 ? o.partials : FIT_PARTIALS_DEFAULT;
    f->o = o;
    const int full = std::min(num_cus(owner->device), (f->S + FIT_WAVES - 1) / FIT_WAVES);
    f->grid = o.grid > 0 ? o.grid : std::max(1, full);
    if (fit_lds_bytes(nh) > NR_LDS_PER_CU) { delete f; return set_err(owner, NR_E_FORMAT, "nr_fit_create: the packs exceed the LDS of a CU"); }
    // flat parameter order: K_0, B_0, ..., K_last, B_last
    std::vector<float> theta((size_t)f->P);
    {
        size_t q = 0;
        for (int l = 0; l < nlayers; ++l) {
            const size_t nk = (size_t)dims[l] * dims[l + 1], nb = (size_t)dims[l + 1];
            memcpy(theta.data() + q, kernels[l], nk * 4); q += nk;
            memcpy(theta.data() + q, biases[l], nb * 4); q += nb;
        }
    }
    const size_t P = (size_t)f->P, pack_bytes = (size_t)fit_pack_floats(nh) * 4;
    hipError_t e = hipSetDevice(owner->device);
    hipStream_t s = e == hipSuccess ? cur_stream(owner) : nullptr;
    if (e == hipSuccess && owner->use_own && !owner->own_stream) { delete f; return NR_E_HIP; }
    if (e == hipSuccess) e = hipMalloc(&f->d_theta, P * 4);
    if (e == hipSuccess) e = hipMalloc(&f->d_m, P * 4);
    if (e == hipSuccess) e = hipMalloc(&f->d_v, P * 4);
    if (e == hipSuccess) e = hipMalloc(&f->d_out, (P + 1) * 4);
    if (e == hipSuccess) e = hipMalloc(&f->d_pack, pack_bytes);
    if (e == hipSuccess) e = hipMalloc(&f->d_partial, (size_t)f->S * (P + 1) * 4);
    if (e == hipSuccess) e = hipMemsetAsync(f->d_m, 0, P * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(f->d_v, 0, P * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(f->d_pack, 0, pack_bytes, s);
    if (e == hipSuccess) e = hipMemcpyAsync(f->d_theta, theta.data(), P * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = launch_fit_update(fit_upd_args(f, FIT_MODE_PACK, 0), s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // (theta is a local)
    if (e != hipSuccess) {
        const bool nomem = e == hipErrorOutOfMemory;
        dfree(f->d_theta); dfree(f->d_m); dfree(f->d_v); dfree(f->d_out); dfree(f->d_pack); dfree(f->d_partial);
        delete f;
        return set_err(owner, nomem ? NR_E_NOMEM : NR_E_HIP, "nr_fit_create: %s", hipGetErrorString(e));
    }
    *out = f;
    return NR_OK;
}

int nr_fit_destroy(nr_fit *f) {
    if (!f) return NR_OK;
    nr_ctx *c = f->owner;
    (void)hipSetDevice(c->device);
    if (!(c->use_own && !c->own_stream)) (void)hipStreamSynchronize(c->stream);
    dfree(f->d_theta); dfree(f->d_m); dfree(f->d_v); dfree(f->d_out); dfree(f->d_pack); dfree(f->d_partial); dfree(f->d_io);
    delete f;
    return NR_OK;
}

int nr_fit_num_params(const nr_fit *f, long *count) {
    if (!f || !count) return set_err(f ? f->owner : nullptr, NR_E_INVALID, "nr_fit_num_params: NULL argument");
    *count = f->P;
    return NR_OK;
}

int nr_fit_gradient(nr_fit *f, const float *X, const float *Y, long n, float *loss, float *grad, float *value, int loc) {
    if (!f) return set_err(nullptr, NR_E_INVALID, "nr_fit_gradient: fit is NULL");
    nr_ctx *c = f->owner;
    if (!X || !Y) return set_err(c, NR_E_INVALID, "nr_fit_gradient: X or Y is NULL");
    if (n < 1 || n > (1l << 30)) return set_err(c, NR_E_INVALID, "nr_fit_gradient: n = %ld outside [1, 2^30]", n);
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    const size_t N = (size_t)n, P = (size_t)f->P;
    const float *dX = X, *dY = Y;
    float *dvalue = value, *dgrad = grad, *dloss = loss;
    if (loc != NR_DEVICE) {
        int rc;
        if ((rc = ensure_buf(c, f->d_io, f->cap_io, 5 * N)) != NR_OK) return rc;
        HIPCHK(c, hipMemcpyAsync(f->d_io, X, 3 * N * 4, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(f->d_io + 3 * N, Y, N * 4, hipMemcpyHostToDevice, s));
        dX = f->d_io; dY = f->d_io + 3 * N;
        if (value) dvalue = f->d_io + 4 * N;
        if (grad) dgrad = f->d_out;
        if (loss) dloss = f->d_out + P;
    }
    HIPCHK(c, launch_fit_grad(fit_grad_args(f, dX, dY, n, dvalue), f->grid, s));
    if (loss || grad) {
        FitUpdArgs U = fit_upd_args(f, FIT_MODE_GRADIENT, n);
        U.grad = dgrad; U.loss = dloss;
        HIPCHK(c, launch_fit_update(U, s));
    }
    if (loc != NR_DEVICE) {
        if (value) HIPCHK(c, hipMemcpyAsync(value, dvalue, N * 4, hipMemcpyDeviceToHost, s));
        if (grad) HIPCHK(c, hipMemcpyAsync(grad, dgrad, P * 4, hipMemcpyDeviceToHost, s));
        if (loss) HIPCHK(c, hipMemcpyAsync(loss, dloss, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
    }
    return NR_OK;
}

int nr_fit_run(nr_fit *f, const float *X, const float *Y, long n, long batch, float *loss, int loc, nr_stats *stats) {
    if (!f) return set_err(nullptr, NR_E_INVALID, "nr_fit_run: fit is NULL");
    nr_ctx *c = f->owner;
    if (!X || !Y) return set_err(c, NR_E_INVALID, "nr_fit_run: X or Y is NULL");
    if (n < 1 || n > (1l << 30)) return set_err(c, NR_E_INVALID, "nr_fit_run: n = %ld outside [1, 2^30]", n);
    if (batch < 1 || n % batch != 0) return set_err(c, NR_E_INVALID, "nr_fit_run: n = %ld is no multiple of batch = %ld", n, batch);
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    const size_t N = (size_t)n;
    const long steps = n / batch;
    const float *dX = X, *dY = Y;
    float *dloss = loss;
    if (loc != NR_DEVICE) {
        int rc;
        if ((rc = ensure_buf(c, f->d_io, f->cap_io, 4 * N + (size_t)steps)) != NR_OK) return rc;
        HIPCHK(c, hipMemcpyAsync(f->d_io, X, 3 * N * 4, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(f->d_io + 3 * N, Y, N * 4, hipMemcpyHostToDevice, s));
        dX = f->d_io; dY = f->d_io + 3 * N;
        if (loss) dloss = f->d_io + 4 * N;
    }
    nr_stats st{};
    HIPCHK(c, hipEventRecord(c->ev0, s));
    const double b1 = (double)f->o.beta1, b2 = (double)f->o.beta2;
    for (long k = 0; k < steps; ++k) {
        HIPCHK(c, launch_fit_grad(fit_grad_args(f, dX + (size_t)k * (size_t)batch * 3, dY + (size_t)k * (size_t)batch, batch, nullptr), f->grid, s));
        const double t = (double)(f->step + 1);
        FitUpdArgs U = fit_upd_args(f, FIT_MODE_ADAM, batch);
        U.a_t = (float)((double)f->o.lr * std::sqrt(1.0 - std::pow(b2, t)) / (1.0 - std::pow(b1, t)));
        U.beta1 = f->o.beta1; U.beta2 = f->o.beta2;
        U.omb1 = (float)(1.0 - b1); U.omb2 = (float)(1.0 - b2);
        U.eps = f->o.eps;
        U.loss = dloss ? dloss + k : nullptr;
        HIPCHK(c, launch_fit_update(U, s));
        ++f->step;  // (enqueued: the step is taken in stream order)
    }
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if (loc != NR_DEVICE && loss) HIPCHK(c, hipMemcpyAsync(loss, dloss, (size_t)steps * 4, hipMemcpyDeviceToHost, s));
    st.ray_steps = (uint64_t)n;
    st.launches = (int32_t)(2 * steps);
    const int rc = end_timed(c, stats != nullptr, loc, s, &st.ms_total);
    if (rc == NR_OK && stats) *stats = st;
    return rc;
}

int nr_fit_weights(nr_fit *f, float *params, long *step) {
    if (!f) return set_err(nullptr, NR_E_INVALID, "nr_fit_weights: fit is NULL");
    nr_ctx *c = f->owner;
    if (!params && !step) return set_err(c, NR_E_INVALID, "nr_fit_weights: params and step are NULL");
    if (params) {
        HIPCHK(c, hipSetDevice(c->device));
        GET_STREAM(c, s);
        HIPCHK(c, hipMemcpyAsync(params, f->d_theta, (size_t)f->P * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
    }
    if (step) *step = f->step;
    return NR_OK;
}

}  // extern "C"

// ---- triangle meshes (nr_trimesh_*; nr_trimesh_host.cpp, nr_trimesh.hip) ----
// The hierarchy, the reordered triangles and the pseudonormal table are built on the host at create
// time and live on the device; a query is one launch.
struct nr_trimesh {
    nr_ctx *owner = nullptr;
    long nv = 0, nt = 0, nnodes = 0, ntl = 0;
    int depth = 0, closed = 0;
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    float *d_nodes = nullptr, *d_tris = nullptr, *d_table = nullptr;
    unsigned long long *d_stats = nullptr;
    float *d_io = nullptr;        // staging of host points and results
    size_t cap_io = 0;
};

extern "C" {

int nr_trimesh_create(nr_ctx *owner, const float *vertices, long nv, const int32_t *triangles, long nt, int leaf,
                      nr_trimesh **out) {
    if (out) *out = nullptr;
    if (!owner || !vertices || !triangles || !out) return set_err(owner, NR_E_INVALID, "nr_trimesh_create: NULL argument");
    if (nv < 1 || nv > (long)INT32_MAX) return set_err(owner, NR_E_INVALID, "nr_trimesh_create: nv = %ld outside [1, 2^31)", nv);
    if (nt < 1 || nt > (1l << 24)) return set_err(owner, NR_E_INVALID, "nr_trimesh_create: nt = %ld outside [1, 2^24]", nt);
    if (leaf < 0 || leaf > 32) return set_err(owner, NR_E_INVALID, "nr_trimesh_create: leaf = %d outside 0..32", leaf);
    if (!trimesh_indices_ok(triangles, nt, nv))
        return set_err(owner, NR_E_INVALID, "nr_trimesh_create: a vertex index outside 0..%ld", nv - 1);
    for (long i = 0; i < 3 * nv; ++i)
        if (!std::isfinite(vertices[i])) return set_err(owner, NR_E_INVALID, "nr_trimesh_create: vertex %ld is not finite", i / 3);
    nr_trimesh *m = new (std::nothrow) nr_trimesh();
    if (!m) return set_err(owner, NR_E_NOMEM, "out of host memory");
    m->owner = owner;
    m->nv = nv; m->nt = nt;
    std::vector<float> table((size_t)nt * 21);
    trimesh_normals(vertices, nv, triangles, nt, table.data(), &m->closed);
    TriBvh H;
    if (!trimesh_build(vertices, nv, triangles, nt, leaf > 0 ? leaf : TRIMESH_LEAF_DEFAULT, table.data(), H)) {
        delete m;
        return set_err(owner, NR_E_INVALID, "nr_trimesh_create: a hierarchy of %d levels (the walk's stack holds %d)", H.depth, TRIMESH_STACK);
    }
    m->nnodes = H.nnodes; m->ntl = H.ntl; m->depth = H.depth;
    for (int a = 0; a < 3; ++a) { m->lo[a] = H.lo[a]; m->hi[a] = H.hi[a]; }
    hipError_t e = hipSetDevice(owner->device);
    hipStream_t s = e == hipSuccess ? cur_stream(owner) : nullptr;
    if (e == hipSuccess && owner->use_own && !owner->own_stream) { delete m; return NR_E_HIP; }
    if (e == hipSuccess) e = hipMalloc(&m->d_nodes, H.nodes.size() * 4);
    if (e == hipSuccess) e = hipMalloc(&m->d_tris, H.tris.size() * 4);
    if (e == hipSuccess) e = hipMalloc(&m->d_table, table.size() * 4);
    if (e == hipSuccess) e = hipMalloc(&m->d_stats, 128);
    if (e == hipSuccess) e = hipMemcpyAsync(m->d_nodes, H.nodes.data(), H.nodes.size() * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(m->d_tris, H.tris.data(), H.tris.size() * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(m->d_table, table.data(), table.size() * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // (the sources are locals)
    if (e != hipSuccess) {
        const bool nomem = e == hipErrorOutOfMemory;
        dfree(m->d_nodes); dfree(m->d_tris); dfree(m->d_table); dfree(m->d_stats);
        delete m;
        return set_err(owner, nomem ? NR_E_NOMEM : NR_E_HIP, "nr_trimesh_create: %s", hipGetErrorString(e));
    }
    *out = m;
    return NR_OK;
}

int nr_trimesh_destroy(nr_trimesh *m) {
    if (!m) return NR_OK;
    nr_ctx *c = m->owner;
    (void)hipSetDevice(c->device);
    if (!(c->use_own && !c->own_stream)) (void)hipStreamSynchronize(c->stream);
    dfree(m->d_nodes); dfree(m->d_tris); dfree(m->d_table); dfree(m->d_stats); dfree(m->d_io);
    delete m;
    return NR_OK;
}

int nr_trimesh_info(const nr_trimesh *m, long *nv, long *nt, long *nodes, int *depth, float lo[3], float hi[3], int *closed) {
    if (!m) return set_err(nullptr, NR_E_INVALID, "nr_trimesh_info: mesh is NULL");
    if (nv) *nv = m->nv;
    if (nt) *nt = m->nt;
    if (nodes) *nodes = m->nnodes;
    if (depth) *depth = m->depth;
    for (int a = 0; a < 3; ++a) {
        if (lo) lo[a] = m->lo[a];
        if (hi) hi[a] = m->hi[a];
    }
    if (closed) *closed = m->closed;
    return NR_OK;
}

int nr_trimesh_distance(nr_trimesh *m, const float *X, long n, float *sdf, float *closest, int32_t *tri, int32_t *feature,
                        int flags, int loc, nr_stats *stats) {
    if (!m) return set_err(nullptr, NR_E_INVALID, "nr_trimesh_distance: mesh is NULL");
    nr_ctx *c = m->owner;
    if (!X) return set_err(c, NR_E_INVALID, "nr_trimesh_distance: X is NULL");
    if (n < 1 || n > (1l << 30)) return set_err(c, NR_E_INVALID, "nr_trimesh_distance: n = %ld outside [1, 2^30]", n);
    if (flags & ~NR_TRIMESH_BRUTE) return set_err(c, NR_E_INVALID, "nr_trimesh_distance: unknown flag bits %#x", flags);
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    const size_t N = (size_t)n;
    TriMeshArgs A{};
    A.X = X; A.n = n;
    A.nodes = m->d_nodes; A.tris = m->d_tris; A.table = m->d_table;
    A.nnodes = (int)m->nnodes; A.ntl = (int)m->ntl;
    A.brute = (flags & NR_TRIMESH_BRUTE) != 0;
    A.sdf = sdf; A.closest = closest; A.tri = tri; A.feature = feature;
    A.stats = m->d_stats;
    if (loc != NR_DEVICE) {
        // staging, in 4-byte words: the points, then every output the caller asked for
        const size_t need = 3 * N + (sdf ? N : 0) + (closest ? 3 * N : 0) + (tri ? N : 0) + (feature ? N : 0);
        int rc;
        if ((rc = ensure_buf(c, m->d_io, m->cap_io, need)) != NR_OK) return rc;
        float *q = m->d_io;
        HIPCHK(c, hipMemcpyAsync(q, X, 3 * N * 4, hipMemcpyHostToDevice, s));
        A.X = q; q += 3 * N;
        if (sdf) { A.sdf = q; q += N; }
        if (closest) { A.closest = q; q += 3 * N; }
        if (tri) { A.tri = reinterpret_cast<int32_t *>(q); q += N; }
        if (feature) { A.feature = reinterpret_cast<int32_t *>(q); q += N; }
    }
    // a grid-stride over chunks of 64 points: at most 8 four-wave workgroups per CU
    const size_t chunks = (N + 63) / 64;
    const int grid = (int)std::max<size_t>(1, std::min<size_t>((chunks + 3) / 4, (size_t)num_cus(c->device) * 8));
    nr_stats st{};
    HIPCHK(c, hipEventRecord(c->ev0, s));
    HIPCHK(c, hipMemsetAsync(m->d_stats, 0, 8, s));
    HIPCHK(c, launch_trimesh_distance(A, grid, s));
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if (loc != NR_DEVICE) {
        if (sdf) HIPCHK(c, hipMemcpyAsync(sdf, A.sdf, N * 4, hipMemcpyDeviceToHost, s));
        if (closest) HIPCHK(c, hipMemcpyAsync(closest, A.closest, 3 * N * 4, hipMemcpyDeviceToHost, s));
        if (tri) HIPCHK(c, hipMemcpyAsync(tri, A.tri, N * 4, hipMemcpyDeviceToHost, s));
        if (feature) HIPCHK(c, hipMemcpyAsync(feature, A.feature, N * 4, hipMemcpyDeviceToHost, s));
    }
    unsigned long long evals = 0;
    if (stats) HIPCHK(c, hipMemcpyAsync(&evals, m->d_stats, 8, hipMemcpyDeviceToHost, s));
    const int rc = end_timed(c, stats != nullptr, loc, s, &st.ms_total);
    if (rc != NR_OK || !stats) return rc;
    st.ray_steps = (uint64_t)n;
    st.shade_evals = evals;
    st.launches = 2;  // the counter's memset and k_trimesh_distance
    *stats = st;
    return NR_OK;
}

}  // extern "C"

// context internals for nr_group.hip (nr_internal.h)
namespace nr {
int ctx_device(const nr_ctx *c) { return c->device; }
void *ctx_stream(nr_ctx *c) { return (void *)cur_stream(c); }
}  // namespace nr
