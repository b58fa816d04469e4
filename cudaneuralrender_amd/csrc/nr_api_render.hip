// nr_api_render.hip -- the frame drivers of the C ABI: the persistent tracer's launch builder, the
// wavefront and layered schedules, nr_render*, nr_render_batch, nr_render_aa and nr_assemble_shards.
//
// Replaces, on the reference side (daviesthomas/cudaNeuralRender @ v1):
//   render_kernel / copyViewMatrices / copyStaticSettings  src/volumeRender_kernel.cu:608-706
//   allocateBuffers + the static scratch globals           :578-606
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "nr_ctx.h"

using namespace nr;

namespace nr {

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

}  // namespace nr

namespace {

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

}  // extern "C"
