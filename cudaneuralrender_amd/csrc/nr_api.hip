// nr_api.hip -- the C ABI of libnr.so (include/neural_render.h): contexts, streams and errors, the
// network and its packs, the settings and the file helpers.  The drivers live beside it, one file an
// area: nr_api_render.hip (frames), nr_api_points.hip (rays, points, lighting), nr_api_mesh.hip
// (lattices and meshes), nr_api_compose.hip, nr_api_fit.hip and nr_api_trimesh.hip; nr_ctx.h holds
// the context and what they share.
//
// Replaces, on the reference side (daviesthomas/cudaNeuralRender @ v1):
//   copyViewMatrices / copyStaticSettings                  src/volumeRender_kernel.cu:694-706
//   NeuralNetwork::load                                    src/neuralNetwork.cpp:54-151
//   DenseLayer ctor                                        src/layers/denseLayer.cu:180-278
//   Image::loadPNG / savePNG                               src/neuralUtils/image.cu:36-110
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "nr_ctx.h"

using namespace nr;

namespace {
thread_local std::string g_err;
}  // namespace

namespace nr {

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

int num_cus(int dev) {
    int cus = 256;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    return cus;
}

// The context's stream: the caller's (nr_set_stream) or the private one, created here on
// first use.  Returns NULL only if that creation failed (error recorded).
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

}  // namespace nr

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
    dfree(c->d_sort); dfree(c->d_sortio); dfree(c->d_fitsamp); dfree(c->d_tbuild);
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
