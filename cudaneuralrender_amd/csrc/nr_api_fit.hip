// nr_api_fit.hip -- the C ABI's network fitting (nr_fit_*).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "nr_ctx.h"

using namespace nr;

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
    Staging io(loc);
    io.in(dX, 3 * N); io.in(dY, N); io.out(dvalue, N);
    int rc;
    if ((rc = io.begin(c, f->d_io, f->cap_io, s)) != NR_OK) return rc;
    if (loc != NR_DEVICE) {
        // the gradient and the loss come through d_out
        if (grad) dgrad = f->d_out;
        if (loss) dloss = f->d_out + P;
    }
    HIPCHK(c, launch_fit_grad(fit_grad_args(f, dX, dY, n, dvalue), f->grid, s));
    if (loss || grad) {
        FitUpdArgs U = fit_upd_args(f, FIT_MODE_GRADIENT, n);
        U.grad = dgrad; U.loss = dloss;
        HIPCHK(c, launch_fit_update(U, s));
    }
    if ((rc = io.end(c, s)) != NR_OK) return rc;
    if (loc != NR_DEVICE) {
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
    Staging io(loc);
    io.in(dX, 3 * N); io.in(dY, N); io.out(dloss, (size_t)steps);
    int rc;
    if ((rc = io.begin(c, f->d_io, f->cap_io, s)) != NR_OK) return rc;
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
    if ((rc = io.end(c, s)) != NR_OK) return rc;
    st.ray_steps = (uint64_t)n;
    st.launches = (int32_t)(2 * steps);
    rc = end_timed(c, stats != nullptr, loc, s, &st.ms_total);
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
