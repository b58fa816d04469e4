/*
 * neural_render.h -- C ABI of libnr.so, the MI355X (gfx950) neural-SDF renderer.
 *
 * Drop-in boundary for the reference's hot path (daviesthomas/cudaNeuralRender @ v1):
 * the sphere-trace loop of src/volumeRender_kernel.cu and the batched dense-layer
 * forward of src/layers/denseLayer.cu + src/neuralNetwork.cpp.  Every entry point
 * takes plain pointers and sizes; state lives in an opaque per-device context
 * (the reference keeps it in non-reentrant globals, volumeRender_kernel.cu:31-35,
 * :578-585).  Functions return NR_OK (0) or a negative NR_E* code; the message is
 * available from nr_last_error().  Nothing in the library calls exit()/abort()
 * (the reference exits inside checkCudaErrors, helper_cuda.h:576-591).
 *
 * Threading: one context per GPU; calls on one context are not thread-safe, calls
 * on different contexts are.  Each context owns one HIP stream.
 */
#ifndef NEURAL_RENDER_H
#define NEURAL_RENDER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NR_ABI_VERSION 3   /* 2: nr_stats.endgame_evals, nr_set_endgame (round 5); 3: nr_stats.endgame_switches (round 6) */
/* (nr_trace_rays / nr_render_gbuffer are new symbols only -- no struct or existing signature changed --
 * so the version stays 3) */

/* status codes */
#define NR_OK 0
#define NR_E_INVALID (-1)    /* bad argument */
#define NR_E_HIP (-2)        /* HIP runtime error */
#define NR_E_IO (-3)         /* file missing / unreadable */
#define NR_E_FORMAT (-4)     /* unsupported HDF5 / PNG content */
#define NR_E_STATE (-5)      /* call out of order (e.g. render before load) */
#define NR_E_NOMEM (-6)

/* MLP arithmetic for the 32x32 hidden layers */
#define NR_PRECISION_FP32 0  /* bit-exact with the CPU oracle (f32 MFMA = fmaf chain) */
#define NR_PRECISION_BF16 1  /* bf16 MFMA, f32 accumulate; normals (the 4 tetrahedron samples) in fp32x3,
                                 nr_set_debug bit 15: fp32; rays near a surface finish in fp32x3
                                 (nr_set_endgame, on by default) */
#define NR_PRECISION_FP16 2  /* fp16 MFMA, f32 accumulate; normals and endgame as bf16 */
#define NR_PRECISION_FP32X3 3 /* fp32-class on the fp16 matrix core: three-term split a.w ~ ah.wh + al.wh + ah.wl,
                                  f32 accumulate (~2-3x the f32 chain's error against an exact
                                  evaluation); normals evaluated in fp32 (bit-exact); points with
                                  inputs outside the pack's bounds run the fp32 MLP.  A network whose
                                  pack is refused (nr_pack_x3 *ok = 0: scales outside fp16's range, or
                                  interval bounds so far above the network's activations that the
                                  split would lose bits -- dense networks of more than ~8 hidden
                                  layers) runs the fp32 MLP at every point,
                                  bit-exact with NR_PRECISION_FP32 */

/* scene composition, sceneSDF (volumeRender_kernel.cu:217-230) */
#define NR_SCENE_V1 0        /* v1: manySphere(p, nSDF, true) -- 9-sphere smooth union (:222) */
#define NR_SCENE_TANH 1      /* tanh(nSDF), the pure neural surface (:229) */
#define NR_SCENE_SUBTRACT 2  /* manySphere(p, nSDF, false) -- 9 spheres smooth-subtracted (:139-142, :190-191) */
#define NR_SCENE_CYLINDERS 3 /* manyCylinderCut(p, nSDF) -- 300 cylinders smooth-subtracted (:157-174) */
#define NR_SCENE_DISPLACE 4  /* displacementPattern(p, nSDF) = sdfOpDisplace(p, tanh(nSDF)) (:104-110, :152-154) */
#define NR_SCENE_ROUND 5     /* sdfOpRound(tanh(nSDF), 0.04) (:112-115, :221) */

/* colouring, c_coloringType (volumeRender_kernel.cu:33) */
#define NR_COLOR_FACING 0    /* facingColor (:380-384) */
#define NR_COLOR_MATCAP 1    /* matCapColor (:387-413) */

/* march schedule (nr_set_schedule) */
#define NR_SCHED_PERSISTENT 0 /* one persistent k_trace launch per frame (default) */
#define NR_SCHED_WAVEFRONT 1  /* one k_march launch per iteration over a compacted ray queue */
#define NR_SCHED_LAYERED 2    /* the reference's structure: per iteration one dense-layer launch per
                                 layer over the live-ray queue, then the step; replayed as a hipGraph.
                                 Any dense [3|4, ..., 1] network, fp32.  Networks the fused kernels
                                 do not take ([3|4, 32, ..., 32, 1]) always render this way. */

/* buffer location flags */
#define NR_HOST 0
#define NR_DEVICE 1

typedef struct nr_ctx nr_ctx;

typedef struct nr_stats {
    uint64_t ray_steps;      /* MLP evaluations of marching rays (one per live ray per iteration) */
    uint64_t shade_evals;    /* MLP evaluations for tetrahedral normals (4 per coloured ray) */
    uint64_t rays_hit;       /* rays that entered the bounding sphere */
    uint64_t rays_shaded;    /* pixels coloured */
    int32_t iterations;      /* march iterations that had live rays (reference host-loop count) */
    int32_t launches;        /* kernel launches issued */
    float ms_total;          /* device time of the render, HIP events */
    uint64_t endgame_evals;  /* bf16/fp16 with the endgame (nr_set_endgame): the march evaluations
                                in fp32x3, included in ray_steps */
    uint64_t endgame_switches; /* the rays handed to the endgame: each one's switch point is evaluated
                                in 16 bits and again in fp32x3, and both evaluations are counted in
                                ray_steps (ray_steps - endgame_switches counts every march point once) */
} nr_stats;

/* ---- context ------------------------------------------------------------ */
int nr_create(int device, nr_ctx **out);
int nr_destroy(nr_ctx *ctx);
/* Last error of this context (ctx may be NULL: last error of the calling thread). */
const char *nr_last_error(const nr_ctx *ctx);
int nr_abi_version(void);
/* Stream the context's work is issued on: own != 0 selects the context's private
 * (non-blocking) stream; otherwise hip_stream is used verbatim, NULL meaning HIP's
 * default (null) stream -- e.g. torch.cuda.current_stream().cuda_stream. */
int nr_set_stream(nr_ctx *ctx, void *hip_stream, int own);
int nr_synchronize(nr_ctx *ctx);

/* ---- network (NeuralNetwork::load / DenseLayer ctor) ---------------------- */
/* Replaces NeuralNetwork::load(fp) (neuralNetwork.cpp:85-151): root groups in HDF5
 * name order, each holding one subgroup with "bias:0" (1-D) and "kernel:0" (2-D,
 * Keras (in, out)); last layer linear, others ReLU. */
int nr_load_h5(nr_ctx *ctx, const char *path);
/* Replaces DenseLayer(name, weights, biases, act) x nlayers (denseLayer.cu:180-227).
 * dims[nlayers+1]; kernels[l] is the Keras (in=dims[l], out=dims[l+1]) row-major
 * matrix, biases[l] has dims[l+1] floats.  ReLU on all layers but the last. */
int nr_load_mlp(nr_ctx *ctx, int nlayers, const int *dims,
                const float *const *kernels, const float *const *biases);
/* The fp32x3 pack of a [3|4, 32, ..., 32, 1] network (host only, no GPU): fp16 hi / residual
 * operands a[*a_len] in the kernels' layout and the floats f[*f_len] (scaled biases, final layer,
 * scales); *ok = 0 when the scales do not fit fp16 or leave the activations below the window in
 * which the fp16 split keeps its bits (the kernels then run fp32).  Copies only when
 * the capacities suffice (call with a = f = NULL for the lengths).  For the test oracle's fp32x3
 * emulation (the bf16/fp16 tracers' normals); not part of the reference's interface. */
int nr_pack_x3(int nlayers, const int *dims, const float *const *kernels, const float *const *biases,
               uint16_t *a, long a_cap, float *f, long f_cap, long *a_len, long *f_len, int *ok);
/* The fp32 packs of a [3|4, 32, ..., 32, 1] network, host only (new symbols only: NR_ABI_VERSION
 * stays 3): the full pack, and the pruned pack the batched fp32 tracer stages in LDS -- the same
 * scaled weights with every ReLU layer's units re-ordered, live units ascending, then the cand[l]
 * units that fire at next to no point of the marched volume (nr_set_prune for the modes).  *len =
 * floats per pack (both), *clamp = the full pack is scaled for the clamped ReLU, *has_pruned = 0
 * when that pack is refused (no pruned pack then).  cand, ks [nlayers - 1] and order
 * [nlayers - 1][32] (position -> unit) are filled when cap_layers >= nlayers - 1; ks[l] = the
 * k-steps of 4 positions that the layer after ReLU layer l runs while the candidates are +0. */
int nr_pack_fp32_pruned(int nlayers, const int *dims, const float *const *kernels, const float *const *biases,
                        int mode, float *full, float *pruned, long cap, long *len, int *clamp, int *has_pruned,
                        int *cand, int *ks, int *order, int cap_layers);
int nr_mlp_info(const nr_ctx *ctx, int *nlayers, int *dims /* >= nlayers+1 or NULL */,
                int *num_weight_params, int *num_bias_params);
int nr_set_precision(nr_ctx *ctx, int precision);

/* ---- per-frame settings (copyViewMatrices / copyStaticSettings) ---------- */
/* Replaces copyViewMatrices (volumeRender_kernel.cu:694-700): inv_view = rows 0..2
 * of the model-view matrix (3x4 row-major, c_invViewMatrix), normal = its inverse
 * (4x4 row-major, c_normalMatrix), frame = c_frameNumber. */
int nr_set_view(nr_ctx *ctx, const float inv_view[12], const float normal[16], int frame);
/* Replaces copyStaticSettings (volumeRender_kernel.cu:702-706). */
int nr_set_static(nr_ctx *ctx, int color_type, int num_inputs);
int nr_set_scene(nr_ctx *ctx, int scene);
/* Replaces Image::loadPNG + the matcap argument of render_kernel (image.cu:36-65):
 * w*h texels packed a<<24 | b<<16 | g<<8 | r, row 0 = first PNG row. */
int nr_set_matcap(nr_ctx *ctx, const uint32_t *rgba, int w, int h);

/* ---- the hot path --------------------------------------------------------- */
/* Replaces render_kernel (volumeRender_kernel.cu:608-692): renders a W x H frame,
 * at most max_steps march iterations (reference MAX_STEPS = 6000), into out
 * (W*H packed RGBA, row y*W + x, unconverged / missed pixels 0).  out_loc is
 * NR_HOST or NR_DEVICE.  stats may be NULL.  Any dense network with 3 or 4 inputs and
 * one output renders (NeuralNetwork takes any layer list, neuralNetwork.cpp:85-151):
 * [3|4, 32, ..., 32, 1] on the fused kernels of the selected schedule, every other
 * shape on NR_SCHED_LAYERED. */
int nr_render(nr_ctx *ctx, uint32_t *out, int W, int H, int max_steps, int out_loc,
              nr_stats *stats);
/* Multi-GPU shard of a frame: rows are dealt in bands of band_rows, band b goes to
 * shard b % nshards.  out receives this shard's rows only, in increasing y
 * (nr_shard_rows() of them, each W wide).  Pixels are identical to the same rows
 * of nr_render. */
int nr_render_shard(nr_ctx *ctx, uint32_t *out, int W, int H, int band_rows,
                    int nshards, int shard, int max_steps, int out_loc, nr_stats *stats);

/* ---- ray queries / geometry buffers ------------------------------------------ */
/* status of a queried ray */
#define NR_RAY_MISS    0  /* never entered the bounding sphere (r = 1.2) */
#define NR_RAY_ESCAPED 1  /* marched out of it (tfar exhausted): a background pixel */
#define NR_RAY_HIT     2  /* converged (tstep < 1e-6) with an iteration left to shade: a coloured pixel */
#define NR_RAY_LIMIT   3  /* max_steps reached, or converged in the last iteration */

/* Marches n caller-supplied rays through the scene exactly as nr_render marches a pixel ray
 * (initMarcher's entry, singleMarch's step, surfaceNormal's tetrahedron) and returns the geometry
 * instead of a colour, in one persistent launch.  Ray i is p = origins[i] + t * dirs[i]; dirs is
 * used as given (not normalised).  Entry: no root of the bounding sphere -> MISS; else tnear =
 * max(tnear, 0), p = o + d * tnear, tfar = the far root (tnear is not subtracted, as in the
 * reference).  Iteration it = 0 .. max_steps - 1: tstep = sceneSDF(p, mlp(p)); tfar -= tstep, tfar
 * <= 0 -> ESCAPED; p += d * tstep, travel += tstep; tstep < 1e-6 -> HIT when it + 1 < max_steps,
 * else LIMIT; steps = it + 1 in all three.  A ray still live after max_steps iterations is LIMIT
 * with steps = max_steps.  A HIT has position = p, t = tnear + travel and normal = the normalised
 * tetrahedral gradient at p (epsilon 1e-5); every other status has t, position and normal +0.0 and
 * a MISS has steps 0.
 * Any output pointer may be NULL.  With normal == NULL the four tetrahedron evaluations per hit
 * are not run and stats->shade_evals is 0 (occlusion / shadow rays).
 * Scene and frame are the context's (nr_set_scene, nr_set_view); a 4-input network gets
 * (float)frame as its 4th input.  The MLP is always the fp32 one (bit-exact with the CPU oracle):
 * nr_set_precision is ignored, as NR_SCHED_LAYERED ignores it.  A ray's results depend only on
 * that ray: they are the same bits for any n, order or split into calls.
 * loc = NR_HOST or NR_DEVICE for all the pointers.  stats (may be NULL): ray_steps = sum of steps,
 * rays_hit = rays that entered the sphere, rays_shaded = HITs, shade_evals = 4 per HIT (0 without
 * normals), iterations = the largest steps.
 * Errors: NR_E_INVALID (ctx NULL, n < 0, n > 2^30, max_steps < 1, origins / dirs NULL with n > 0),
 * NR_E_STATE (no network), NR_E_FORMAT (a network the fused kernels do not take: there is no
 * layered fallback for queries).  n = 0 returns NR_OK without a launch. */
int nr_trace_rays(nr_ctx *ctx, const float *origins /*[n][3]*/, const float *dirs /*[n][3]*/, long n,
                  int max_steps, int32_t *status, int32_t *steps, float *t,
                  float *position /*[n][3]*/, float *normal /*[n][3]*/, int loc, nr_stats *stats);
/* The same query for the W x H pixel rays of the context's view (nr_set_view), generated in the
 * kernel: pixel (x, y) is at index y * W + x and its ray is nr_render's.  status == NR_RAY_HIT
 * exactly where nr_render's pixel is coloured.  NR_E_INVALID also for W or H < 1 or W * H > 2^30. */
int nr_render_gbuffer(nr_ctx *ctx, int W, int H, int max_steps, int32_t *status, int32_t *steps, float *t,
                      float *position, float *normal, int loc, nr_stats *stats);

/* ---- adaptive supersampled antialiasing ---------------------------------------- */
/* (a new symbol only, as the ray queries: NR_ABI_VERSION stays 3) */
#define NR_AA_ADAPTIVE 0
#define NR_AA_FULL 1
#define NR_AA_CONTRAST_DEFAULT 32
/* Renders the W x H frame of the context's view with the edge pixels resolved from S x S samples,
 * S = samples, 1 <= S <= 8.  Let `big` be the frame nr_render gives for S W x S H with the context's
 * view, frame number, scene, colouring and matcap at NR_PRECISION_FP32 and max_steps, and
 * base[y][x] = big[S y][S x] -- which is nr_render's W x H frame: sub-sample (0, 0) of pixel (x, y)
 * has that pixel's ray.  The antialiased frame is a box filter over `big`, applied where the base
 * frame shows an edge:
 *  1. Channels.  A pixel is (r, g, b, a) = bits 0-7, 8-15, 16-23, 24-31; a background, missed or
 *     unconverged pixel is 0 in all four.
 *  2. Edge.  Pixel (x, y) is an edge iff some pixel n of its 8-neighbourhood that lies inside the
 *     image has max over the four channels of |base(x, y) - base(n)| > contrast (strict; 0 <=
 *     contrast <= 255).  Neighbours outside the image do not exist: a frame border is not an edge.
 *     A coloured pixel has alpha 255 next to the background's 0, so every contrast below 255 finds
 *     the silhouette and lower values add creases and shading gradients; contrast = 255 finds no
 *     edge.  NR_AA_FULL treats every pixel as an edge.
 *  3. Resolve.  Each channel of an edge pixel is (sum + S S / 2) / (S S) in integer arithmetic, the
 *     sum over that channel of the S S pixels big[S y + sy][S x + sx]: alpha becomes coverage and
 *     the colours come out premultiplied against a transparent black background.  Any other pixel
 *     is base(x, y) unchanged.
 *  4. Arithmetic and settings.  Always the fp32 MLP: nr_set_precision and nr_set_schedule are
 *     ignored, as for the ray queries, and the call leaves the context's settings as it found
 *     them.  The output depends only on the inputs: the same bits on every call, for any grid size
 *     or order in which the samples are dealt (the sums are integer).
 *  5. Outputs.  *edge_pixels (may be NULL) = the number of edge pixels (W H in FULL mode; 0 in
 *     adaptive mode with S = 1, where no pixel is resolved).  stats (may be NULL): ray_steps,
 *     shade_evals, rays_hit and rays_shaded are the base frame's plus those of the additional
 *     sub-sample rays -- in FULL mode nr_render's for the S W x S H frame; iterations is the larger
 *     of the two passes'; launches and ms_total as elsewhere.
 *  6. Errors.  NR_E_INVALID: ctx or out NULL, W or H < 1, S outside 1..8, an unknown mode, contrast
 *     outside 0..255, S W * S H > 2^30, max_steps < 0.  NR_E_STATE: no network.  NR_E_FORMAT: a
 *     network the fused kernels do not take, as for the queries (no layered fallback).  Everything
 *     else nr_render would report for the same context is reported as nr_render reports it.
 *  7. Limitation.  Adaptive mode only refines what the base samples reveal: a feature thinner than
 *     a pixel that no base ray hits is not found.  NR_AA_FULL is the exact form.
 *  8. Scratch.  The context owns it and keeps it until nr_destroy: 4 bytes per pixel (the edge
 *     list) and 8 bytes per edge pixel (the accumulators), plus W H x 4 bytes of staging for a host
 *     output.  The S W x S H image is never materialised.
 * With S = 1, contrast = 255 (adaptive) or no edge pixel the result is the base frame and no
 * sub-sample pass is launched.  The call reads the edge count on the host once (it synchronises the
 * context's stream) before it launches the sub-sample pass. */
int nr_render_aa(nr_ctx *ctx, uint32_t *out, int W, int H, int samples, int mode, int contrast,
                 int max_steps, int out_loc, long *edge_pixels, nr_stats *stats);

/* ---- ambient occlusion and soft shadows ------------------------------------------ */
/* (new symbols and one new struct only: NR_ABI_VERSION stays 3, nr_stats is unchanged) */
typedef struct nr_light {
    float dir[3];       /* from the surface towards the light, world space; used as given (not normalised) */
    int   shadow_steps; /* at most this many march iterations per shadow ray; 0 = no shadows (shadow = 1) */
    float shadow_bias;  /* shadow-ray origin = hit position + normal * shadow_bias */
    float shadow_k;     /* penumbra sharpness; 0 = hard shadow */
    float ao_step;      /* spacing of the 4 occlusion samples along the normal */
    float ao_strength;  /* 0 = no ambient occlusion (ao = 1, no evaluations run) */
    float ambient;      /* share of the light that no shadow removes, 0..1 */
} nr_light;
/* Renders the W x H frame of the context's view lit by one directional light: every coloured pixel
 * of nr_render's frame is scaled by an ambient-occlusion factor and a soft-shadow factor taken from
 * the same signed-distance field, in one call (a geometry buffer, one persistent lighting launch,
 * one compositing launch; no host round trip).  All arithmetic is f32, one rounding per operation,
 * no contraction; dot3(a, b) = (a0 b0 + a1 b1) + a2 b2; sat(x) = x for 0 < x <= 1, 1 above, else 0
 * (NaN -> 0).  G is what nr_render_gbuffer(W, H, max_steps) returns for the context's view, scene
 * and frame (status, position, normal); base is nr_render's W x H frame at NR_PRECISION_FP32 with
 * the context's colouring and matcap; L = light->dir.
 *  1. A pixel that is not NR_RAY_HIT has out = 0, ao = 1.0f, shadow = 1.0f.
 *  2. Geometry of a HIT pixel.  p = G.position, n = G.normal, dd = dot3(n, L), ndl = dd > 0 ? dd : 0
 *     (a NaN normal gives 0).
 *  3. Ambient occlusion (ao_strength > 0).  For q = 0..3: h_q = (float)(q + 1) * ao_step, a_q = p +
 *     n * h_q per component (multiply, then add), s_q = sceneSDF(a_q, mlp(a_q)) with the fp32 MLP (a
 *     4-input network gets (float)frame), c_q = (h_q - s_q) * w_q with w = 1, 0.5, 0.25, 0.125.
 *     occ = ((c_0 + c_1) + c_2) + c_3 and ao = sat(1.0f - ao_strength * occ).  With ao_strength == 0,
 *     ao = 1.0f, nothing is evaluated and those shade_evals are not counted.
 *  4. Shadow (shadow_steps > 0).  If ndl is 0, shadow = 0.0f and no ray is marched.  Otherwise the ray
 *     o = p + n * shadow_bias (multiply, then add), d = L is marched exactly as nr_trace_rays marches
 *     a ray -- the same entry, step and end conditions, shadow_steps in the place of max_steps, no
 *     normals -- with one addition: res = 1.0f at the start, and at every iteration, once tstep =
 *     sceneSDF(p, mlp(p)) is known and before tfar is tested, dist = tnear + travel and, if dist > 0,
 *     r = shadow_k * tstep / dist (multiply, then an IEEE divide) and res = r where r < res.  (dist
 *     is 0 at the first point of a ray that starts inside the bounding sphere, as every shadow ray
 *     of a surface does: there the quotient would be +inf or NaN and says nothing; shadow_bias
 *     decides how far that point is from the surface.)  The ray's status gives the value: MISS
 *     1.0f; ESCAPED shadow_k > 0 ? sat(res) : 1.0f; HIT and LIMIT 0.0f.  With shadow_steps == 0,
 *     shadow = 1.0f for every pixel and no ray is marched.
 *  5. Composite.  f = ao * (ambient + (1.0f - ambient) * (shadow * ndl)); each of the r, g, b bytes c
 *     of base(x, y) becomes (uint32)((float)c * f) by truncation, at most 255 (f exceeds 1 only for
 *     a dir longer than 1); alpha stays base's.  With ao_strength = 0, shadow_steps = 0 and ambient
 *     = 1, f is exactly 1 and out is nr_render's fp32 frame, bit for bit.
 *  6. Settings and precision.  Always the fp32 MLP: nr_set_precision and nr_set_schedule are
 *     ignored, as for the ray queries, and the call leaves the context's settings as it found
 *     them.  The outputs depend only on the inputs: the same bits for any grid size, occupancy
 *     (nr_set_occupancy) or order in which the pixels are dealt.
 *  7. Outputs.  out (W H pixels), ao and shadow (W H floats each), index y * W + x: any may be NULL
 *     but not all three; loc = NR_HOST or NR_DEVICE for all of them.  stats (may be NULL): ray_steps
 *     = the geometry buffer's plus the sum of the shadow rays' steps; rays_hit and rays_shaded the
 *     geometry buffer's; shade_evals = 4 per HIT, plus 4 per HIT with ambient occlusion on;
 *     iterations = the larger of the primary and the shadow rays' longest; launches and ms_total
 *     as elsewhere.
 *  8. Errors.  NR_E_INVALID: ctx or light NULL, all three outputs NULL, W or H < 1, W H > 2^30,
 *     max_steps < 1, shadow_steps < 0, a non-finite field, dir all zero, shadow_k, ao_step or
 *     ao_strength negative, ambient outside 0..1.  NR_E_STATE: no network.  NR_E_FORMAT: a network
 *     the fused kernels do not take, as for the queries (no layered fallback).  Everything else
 *     nr_render would report for the same context is reported as nr_render reports it.
 *  9. Scratch.  The context owns it and keeps it until nr_destroy: 28 bytes per pixel of geometry
 *     buffer (status, position, normal), 8 bytes per pixel (ao, shadow) where the caller gave none
 *     or gave host pointers (4 for one of the two), plus W H x 4 bytes of staging for a host out. */
int nr_render_lit(nr_ctx *ctx, uint32_t *out /*W*H or NULL*/, int W, int H, int max_steps,
                  const nr_light *light, float *ao /*W*H or NULL*/, float *shadow /*W*H or NULL*/,
                  int loc, nr_stats *stats);

/* ---- volume sampling / isosurface extraction ------------------------------------ */
/* (new symbols only, as the ray queries: NR_ABI_VERSION stays 3)
 *
 * The lattice of the three calls: dims = (nx, ny, nz); point (i, j, k), 0 <= i < nx and likewise j,
 * k, has linear index (k * ny + j) * nx + i and coordinates origin[a] + (float)idx_a * step[a] --
 * one f32 multiply, then one f32 add.  At most 2^30 points.
 *
 * nr_sample_grid writes sdf[idx] = sceneSDF(p, mlp(p)) for every lattice point, generated in the
 * kernel (no point list), with the context's scene and frame (nr_set_scene, nr_set_view); a 4-input
 * network gets (float)frame as its 4th input.  Always the fp32 MLP (bit-exact with the CPU oracle):
 * nr_set_precision is ignored, as for the ray queries.  A point's value depends only on that point:
 * the same bits for any grid size, occupancy or lattice that contains the point.  sdf is
 * [nz][ny][nx], a host or device pointer per loc.  stats (may be NULL): ray_steps = points
 * evaluated, launches, ms_total.
 * Errors: NR_E_INVALID (a NULL argument, a dim < 1, nx * ny * nz > 2^30), NR_E_STATE (no network),
 * NR_E_FORMAT (a network the fused kernels do not take, as for the ray queries). */
int nr_sample_grid(nr_ctx *ctx, const float origin[3], const float step[3], const int dims[3],
                   float *sdf /*[nz][ny][nx]*/, int loc, nr_stats *stats);
/* Marching tetrahedra over a caller-supplied lattice of values (any values: it needs no network and
 * works on a context without one).  loc applies to every pointer but nv / nt.  The output is a pure
 * function of the inputs -- counts, an exclusive scan and an emit pass; no atomic decides an order:
 *  1. Inside.  A corner is inside iff s < iso: NaN is outside, and so is s == iso.
 *  2. Tetrahedra.  Each cell (i, j, k), i < nx - 1 and likewise j, k, is split into the 6 Kuhn
 *     tetrahedra: for each permutation (a, b, c) of the axes, in lexicographic order xyz, xzy, yxz,
 *     yzx, zxy, zyx, the path v0 = the cell's corner 000, v1 = v0 + e_a, v2 = v1 + e_b, v3 = v2 + e_c
 *     = its corner 111.
 *  3. Vertices.  One per lattice edge whose endpoints differ in insideness.  The edges are the 7
 *     kinds the split uses, from a lattice point o to o + e for e in this slot order: 100, 010, 001,
 *     110, 101, 011, 111 (x first); both ends must lie in the lattice.  Vertices are numbered by
 *     increasing index(o) * 7 + slot.  With a = o and b = o + e: t = (iso - s_a) / (s_b - s_a) and
 *     pos = p_a + (p_b - p_a) * t per component, all f32 with one rounding per operation (p_a, p_b
 *     the lattice coordinates above); a NaN coordinate is written as the quiet NaN 0x7fc00000.  As a
 *     is always the lower lattice end, every tetrahedron sharing the edge gets the same vertex.
 *  4. Triangles.  A tetrahedron with one inside corner P and outside corners Q1 < Q2 < Q3 (by path
 *     index) emits one triangle on the edges (P,Q1), (P,Q2), (P,Q3); likewise with inside and
 *     outside exchanged.  One with inside corners A < B and outside corners C < D emits two, {AC, AD,
 *     BD} and {AC, BD, BC} (the diagonal joins AC and BD).  The winding is decided on the topology,
 *     not on floats: with every vertex moved to the midpoint of its edge, (b - a) x (c - a) points
 *     from the centroid of the inside corners towards the centroid of the outside corners.
 *     Triangles are written in increasing cell index ((k * ny + j) * nx + i of the cell's corner
 *     000); within a cell the order is fixed -- the same on every call -- but not specified, and so
 *     is the vertex a triangle starts with.
 *  5. Capacities.  *nv and *nt are always set.  With vertices == NULL && triangles == NULL the call
 *     only counts.  If v_cap < *nv or t_cap < *nt nothing is written and the call returns
 *     NR_E_NOMEM.
 *  6. Errors.  NR_E_INVALID: a NULL ctx, sdf, origin, step, dims, nv or nt; only one of vertices /
 *     triangles NULL; a dim < 2; nx * ny * nz > 2^30; more than 2^31 - 1 vertices.
 * Scratch: the context keeps 4 B per lattice point + 24 B per 256 points of device memory for the
 * passes (and, for loc = NR_HOST, staging for the lattice and the mesh) until nr_destroy. */
int nr_mesh_grid(nr_ctx *ctx, const float *sdf /*[nz][ny][nx]*/, const float origin[3], const float step[3],
                 const int dims[3], float iso, float *vertices /*[v_cap][3]*/, long v_cap,
                 int32_t *triangles /*[t_cap][3]*/, long t_cap, long *nv, long *nt, int loc);
/* nr_sample_grid into a context-owned device buffer (4 B per lattice point, kept until nr_destroy),
 * then nr_mesh_grid on it: capacities, counting call (which samples too) and errors as both.  If
 * normals is given (with vertices and triangles), vertex i gets the world normal of
 * nr_trace_rays' hits at its position: the normalised tetrahedral gradient, epsilon 1e-5, in the
 * same arithmetic.  stats (may be NULL): ray_steps = lattice points, rays_shaded = *nv, shade_evals
 * = 4 * *nv with normals, else 0; launches, ms_total. */
int nr_extract_mesh(nr_ctx *ctx, const float origin[3], const float step[3], const int dims[3], float iso,
                    float *vertices /*[v_cap][3]*/, float *normals /*[v_cap][3] or NULL*/, long v_cap,
                    int32_t *triangles /*[t_cap][3]*/, long t_cap, long *nv, long *nt, int loc, nr_stats *stats);
/* nr_extract_mesh on a lattice too large to sample densely: the lattice is cut into bricks of
 * `brick`^3 cells, the scene is sampled at the brick corners, and only the bricks the surface can
 * reach are sampled and meshed.  The mesh is nr_mesh_grid's mesh of the full lattice restricted to
 * those bricks, bit for bit.
 *  1. Lattice.  That of nr_sample_grid (index (k * ny + j) * nx + i, coordinate origin[a] +
 *     (float)idx_a * step[a]), every dim 2..65,536; nx * ny * nz is not limited to 2^30, and linear
 *     indices and keys are 64-bit.
 *  2. Bricks.  brick = B in {4, 8, 16}.  Axis a has nb_a = ceil((dims[a] - 1) / B) bricks; brick
 *     (bx, by, bz) has linear index (bz * nby + by) * nbx + bx and covers, along axis a, the cells
 *     B b_a .. min(B b_a + B, dims[a] - 1) - 1 (the last brick of an axis may be ragged, 1..B cells).
 *     Its point set is the lattice points B b_a .. min(B b_a + B, dims[a] - 1) per axis, its 8
 *     corners the extreme points of that set.  nbx * nby * nbz <= 2^30.
 *  3. Values.  Every value used is sceneSDF(p, mlp(p)) at a lattice point, with nr_sample_grid's
 *     bits for that point: the coordinate comes from the global index as in 1, never from a brick
 *     origin plus an offset.  Always the fp32 MLP with the context's scene and frame;
 *     nr_set_precision and nr_set_schedule are ignored, and the call leaves the context's settings
 *     as it found them.
 *  4. Active bricks.  With d = fabsf(s - iso) (one f32 subtract) for a corner value s, a brick is
 *     active iff a corner value is NaN, or its corners differ in insideness (inside: s < iso, as
 *     nr_mesh_grid), or the smallest d of its corners is <= band.  band >= 0; +INFINITY makes every
 *     brick active.
 *  5. Mesh.  Triangles: exactly those nr_mesh_grid's rule gives for the cells of active bricks.
 *     Vertices: exactly the crossing lattice edges (o, slot) whose two ends both lie in the point
 *     set of some active brick (each is an edge of a Kuhn tetrahedron of a cell of that brick); one
 *     vertex per edge however many bricks share it, at nr_mesh_grid's position, bit for bit.
 *     keys[v] = index(o) * 7 + slot with the 64-bit linear index of o -- the number that orders the
 *     dense mesh's vertices, so a caller can sort into the dense order or stitch tiles.  normals as
 *     nr_extract_mesh.  vertices, normals and keys share one order; that order, the triangle order
 *     and the vertex a triangle starts with are fixed -- the same bytes on every call for the same
 *     inputs, at any grid size or occupancy, no atomic deciding an order -- but not otherwise
 *     specified.  The windings are nr_mesh_grid's.  With band = +INFINITY the mesh sorted by key is
 *     nr_extract_mesh's; with a band for which every crossing cell lies in an active brick it is
 *     that mesh too, closed wherever the dense one is.
 *     What it is not: a proof that nothing was culled.  The band is sound when the field changes by
 *     at most `band` over a brick's diagonal; a network is only approximately a distance field, and
 *     too small a band silently leaves holes at the culled bricks.
 *  6. Capacities.  As nr_mesh_grid: *nv and *nt are always set, *active_bricks when given; with
 *     vertices == NULL && triangles == NULL the call only counts; if a capacity is short nothing is
 *     written and the call returns NR_E_NOMEM.  keys and normals need vertices.  At most 2^31 - 1
 *     vertices.  loc applies to every pointer but nv, nt and active_bricks.
 *  7. Stats (may be NULL).  ray_steps = (nbx + 1)(nby + 1)(nbz + 1) plus the sum over the active
 *     bricks of their point-set sizes (a point shared by neighbouring active bricks counts once per
 *     brick: it is evaluated in each, to the same bits); rays_hit = active bricks; rays_shaded =
 *     *nv; shade_evals = 4 * *nv with normals, else 0; launches and ms_total as elsewhere.
 *  8. Errors.  NR_E_INVALID: a NULL ctx, origin, step, dims, nv or nt; a dim outside 2..65,536;
 *     brick not 4, 8 or 16; band negative or NaN; iso not finite; only one of vertices / triangles
 *     given; keys or normals without vertices; more than 2^30 bricks.  NR_E_STATE: no network.
 *     NR_E_FORMAT: a network the fused kernels do not take.  NR_E_NOMEM: short capacities, or scratch
 *     that cannot be allocated (the message through nr_last_error).
 *  9. Scratch.  The context owns it and keeps it until nr_destroy.  Per brick: 4 bytes (the brick ->
 *     slot map) + 4 bytes per point of the brick-corner lattice + 24 bytes per 256 bricks.  Per
 *     active brick: 4 bytes (the active list) + 8 bytes (value, pass word) per active point -- the
 *     brick's (B + 1)^3 points rounded up to a multiple of 64: 128, 768 or 4,928 -- + 24 bytes per
 *     256 active points.  For loc = NR_HOST also staging of the mesh's size.  The active-brick count is read on the host once, before the per-brick store is
 *     sized (as nr_render_aa reads its edge count). */
int nr_extract_mesh_sparse(nr_ctx *ctx, const float origin[3], const float step[3], const int dims[3],
                           float iso, int brick, float band,
                           float *vertices /*[v_cap][3]*/, float *normals /*[v_cap][3] or NULL*/,
                           int64_t *keys /*[v_cap] or NULL*/, long v_cap,
                           int32_t *triangles /*[t_cap][3]*/, long t_cap,
                           long *nv, long *nt, long *active_bricks /*or NULL*/, int loc, nr_stats *stats);
/* Wavefront OBJ writer (host only, host pointers): "v x y z" per vertex and, when normals is given,
 * "vn x y z", printed with %.9g (which round-trips f32); faces "f a b c", or "f a//a b//b c//c" with
 * normals, 1-based.  NR_E_IO when the file cannot be opened or written. */
int nr_obj_save(const char *path, const float *vertices /*[nv][3]*/, long nv, const float *normals /*or NULL*/,
                const int32_t *triangles /*[nt][3]*/, long nt);

/* Batched frames (persistent schedule): render nframes frames -- each with its own camera
 * (the nr_set_view matrices), frame number and output image -- of the same size/shard
 * in as few launches as possible (up to 32 frames per launch).  The pixel queue runs
 * through the frames in order, so one frame's longest rays march while the next
 * frame's pixels keep the matrix cores busy: the throughput form of a sequence of
 * nr_render_shard calls, with identical pixels.  The network, precision, scene,
 * colouring and matcap are the context's.  `out` is a device or host pointer per `loc`;
 * stats are summed over the frames.  Schedules other than persistent, and the debug
 * flags 1 and 8, render frame by frame. */
typedef struct nr_frame {
    float inv_view[12];
    float normal[16];
    int frame;
    uint32_t *out;
} nr_frame;
int nr_render_batch(nr_ctx *ctx, const nr_frame *frames, int nframes, int W, int H, int band, int nshards,
                    int shard, int max_steps, int loc, nr_stats *stats);
int nr_shard_rows(int H, int band_rows, int nshards, int shard);
/* Frames per k_trace launch nr_render_batch uses for this shard: min(nframes, 32), further
 * capped so that every pixel-queue position of a launch, plus the positions its waves can
 * over-reserve, fits the 32-bit queue counters (queue_shards = nr_set_queue_shards' n).
 * Returns 0 when not even one frame fits (nr_render_batch then fails with NR_E_INVALID). */
int nr_batch_frames_per_launch(int W, int H, int band_rows, int nshards, int shard, int nframes, int queue_shards);
/* Re-interleave gathered shards (shard s's rows at src + s*stride_pixels) into a full
 * frame.  Host or device buffers (loc applies to both). */
int nr_assemble_shards(nr_ctx *ctx, const uint32_t *src, size_t stride_pixels,
                       uint32_t *dst, int W, int H, int band_rows, int nshards, int loc);

/* ---- multi-GPU, one process (main.cpp's render loop over the GPUs of a node) --------------
 * A group joins contexts on distinct GPUs (each created by nr_create on its device, with the
 * same network, precision, scene, colouring, matcap and schedule settings) with one RCCL
 * communicator (ncclCommInitAll).  nr_group_render_batch renders nframes frames across them:
 * context r renders row-band shard r of every frame (bands of `band` rows dealt round-robin,
 * the contexts in parallel, one host thread each), every shard's status is checked before any
 * transfer (a failed shard returns its error and starts no collective), ONE RCCL gather per call
 * (ncclSend / ncclRecv in one ncclGroupStart / ncclGroupEnd) brings the shards to the first
 * context's GPU, and one re-interleave launch per frame writes frames[i].out -- device pointers
 * on the first context's GPU (loc = NR_DEVICE) or host pointers (NR_HOST).  Pixels are
 * identical to nr_render on one GPU.  stats: summed over the shards (ms_total: the slowest). */
typedef struct nr_group nr_group;
int nr_group_create(nr_ctx *const *ctxs, int n, nr_group **out);
/* flags (round 5): NR_GROUP_COPY moves the shards with hipMemcpyPeerAsync instead of RCCL (the same
 * layout and re-interleave; contexts may then share a GPU -- how a one-GPU box runs multi-rank
 * groups); NR_GROUP_ASYNC returns once the call's gather and re-interleave are enqueued on the
 * group's communication streams, so the next call's render overlaps this call's transfer (shard
 * and gather buffers are double-buffered): frames[i].out of an NR_DEVICE call is complete after
 * nr_group_synchronize -- or, without the flag, when the call returns.  A call with host outputs
 * (loc != NR_DEVICE) always returns with its frames written.  Round 6: with NR_GROUP_ASYNC and
 * stats == NULL the renders are only enqueued too (the transfer streams wait for them device-side),
 * so the host submits call k + 1 while call k renders; a launch error still ends the call before
 * any transfer, a fault during the march is returned by the next call or nr_group_synchronize.
 * Asking for stats makes the call wait for its renders (the counters are read from the devices).
 * With NR_GROUP_COPY the contexts may sit on distinct GPUs as well. */
#define NR_GROUP_COPY 1
#define NR_GROUP_ASYNC 2
int nr_group_create_ex(nr_ctx *const *ctxs, int n, int flags, nr_group **out);
int nr_group_destroy(nr_group *group);
int nr_group_size(const nr_group *group);
int nr_group_render_batch(nr_group *group, const nr_frame *frames, int nframes, int W, int H, int band,
                          int max_steps, int loc, nr_stats *stats);
int nr_group_synchronize(nr_group *group);
/* The gather layout nr_group_render_batch uses: frame i's shard on every rank at i * shard_px
 * (shard_px = nr_shard_rows(H, band, n, 0) * W, the largest shard), rank r's shards at
 * r * per_rank of the gather buffer (per_rank = shard_px * nframes). */
int nr_group_layout(int W, int H, int band, int n, int nframes, size_t *shard_px, size_t *per_rank);

/* Replaces NeuralNetwork::forward(X) (neuralNetwork.cpp:54-63) on a batch:
 * X [n][dims[0]] fp32, Y [n][dims[nlayers]] fp32.  loc = NR_HOST or NR_DEVICE. */
int nr_mlp_forward(nr_ctx *ctx, const float *X, float *Y, long n, int loc);

/* The network's analytic gradient (a new symbol only: NR_ABI_VERSION stays 3): per point of
 * X [n][dims[0]] the value, the exact gradient d value / d input by one backward pass, and the
 * normalised gradient.  One launch; networks of the fused shape [3|4, 32, ..., 32, 1] with at most
 * 7 hidden 32 x 32 layers (the ReLU masks of the 8 layers are held in registers).
 *  - Forward: nr_mlp_forward's fp32 pass.  value[i] has the bits nr_mlp_forward gives in fp32;
 *    nr_set_precision is ignored, as for the ray queries.  X has 3 or 4 columns as the network has:
 *    a 4-input network takes its 4th input from X, not from the context's frame.
 *  - Mask: hidden layer l (l = 0 .. nh, the layers with ReLU) has the pre-activation z_l, bias
 *    added, as the forward computes it; m_l[u] = z_l[u] > 0 (false at 0, false for NaN).
 *  - Backward, all fp32; every dot product is one fmaf chain from +0.0 over the summed index in
 *    ascending natural unit order.  With the Keras kernels K_l (in x out):
 *      g[u] = m_nh[u] ? K_last[u][0] : +0.0;
 *      for l = nh .. 1: acc[i] = chain over j = 0..31 of fmaf(K_l[i][j], g[j], acc),
 *                       g[i] = m_(l-1)[i] ? acc[i] : +0.0;
 *      grad[c] = chain over j of fmaf(K_0[c][j], g[j], +0.0) for c < dims[0].
 *    (A masked unit contributes an exact +0 operand: masking before the product and skipping the
 *    term give the same bits for finite weights.)
 *  - normal[i] = the device normalize3 of the first three gradient components,
 *    v * (1 / sqrt((x x + y y) + z z)) without contraction -- the arithmetic of nr_trace_rays'
 *    normals; a zero gradient gives what that arithmetic gives (NaN).  For NR_SCENE_TANH and
 *    NR_SCENE_ROUND this is the scene's exact normal direction (tanh and the offset are monotone);
 *    the other scenes compose spheres and cylinders, whose gradient is not computed here.
 *  - A point's outputs depend only on that point: the same bits for any n, order or split into calls.
 *    Non-finite inputs: unspecified outputs, no fault.
 *  - value [n], grad [n][dims[0]], normal [n][3]: any may be NULL, not all three.  loc = NR_HOST or
 *    NR_DEVICE for all the pointers.  stats (may be NULL): ray_steps = n, launches, ms_total;
 *    everything else 0.
 * Errors: NR_E_INVALID (ctx NULL, n < 0, n > 2^30, X NULL with n > 0, every output NULL),
 * NR_E_STATE (no network), NR_E_FORMAT (a network the fused kernels do not take, or more than 7
 * hidden 32 x 32 layers: there is no layered fallback).  n = 0 returns NR_OK without a launch. */
int nr_mlp_gradient(nr_ctx *ctx, const float *X /*[n][dims[0]]*/, long n, float *value /*[n] or NULL*/,
                    float *grad /*[n][dims[0]] or NULL*/, float *normal /*[n][3] or NULL*/, int loc, nr_stats *stats);

/* Projection of points onto a level set of the network (new symbols only: NR_ABI_VERSION stays 3):
 * per point of X, Newton steps along the analytic gradient until the network's value is within tol
 * of iso, all in one persistent launch.  Networks as for nr_mlp_gradient.
 *  All arithmetic is f32, one rounding per operation, no contraction;
 *  dot3(a, b) = (a0 b0 + a1 b1) + a2 b2.  Per point: p = the first three columns of X, p0 = p; a
 *  4-input network takes its 4th input w from X and holds it constant (as nr_mlp_gradient: it is not
 *  the context's frame).  For it = 0, 1, ...:
 *    1. (v, g) = the bits nr_mlp_gradient gives for value and grad at (p[, w]).
 *    2. r = v - iso; at it == 0, r0 = r.
 *    3. If |r| <= tol: NR_PROJ_CONVERGED, stop.
 *    4. Otherwise, if it == max_iters: NR_PROJ_LIMIT, stop.
 *    5. gg = dot3(g, g) over the first three components.  If !(gg > 0): NR_PROJ_FLAT, stop.
 *    6. t = r / gg (the IEEE divide).
 *    7. If max_step > 0: m = |r| / sqrtf(gg), and where m > max_step, t = t * (max_step / m).
 *    8. p_c = p_c - g_c * t for c = 0..2 (multiply, then subtract); the next iteration follows.
 *  Outputs, all at the final p: position = p; value = v (the bits of nr_mlp_forward at position);
 *  normal = the device normalize3(g) (the bits of nr_mlp_gradient's normal at position; NaN for a
 *  zero gradient); iters = it, the steps taken; status = NR_PROJ_*; distance = sqrtf(dot3(d, d)) with
 *  d_c = p_c - p0_c, negated where r0 < 0 (-0.0 where such a point took no step).
 *  - max_iters = 0 is nr_mlp_gradient plus a status.
 *  - A point's outputs depend only on that point and on opts: the same bits for any n, order, split
 *    into calls, grid size or occupancy.  Non-finite inputs: unspecified outputs, no fault, and at
 *    most max_iters + 1 evaluations.
 *  - nr_set_precision and nr_set_schedule are ignored, as for the ray queries; the call leaves the
 *    context's settings as it found them.
 *  - position [n][3], value [n], normal [n][3], distance [n], iters [n], status [n]: any may be NULL,
 *    not all six.  loc = NR_HOST or NR_DEVICE for all the pointers.
 *  - stats (may be NULL): ray_steps = the evaluations (iters + 1 per point, summed), rays_shaded =
 *    the CONVERGED points, iterations = the largest evaluation count of a point, launches, ms_total;
 *    everything else 0.
 *  What it is not: a Newton step along the gradient lands on the level set, in general not on its
 *  point nearest to p0, and the network is only approximately a distance field.  distance is the
 *  length of the chord from p0 to position, not a proven distance to the surface.
 *  iso = 0 is the surface nr_render shows for NR_SCENE_TANH (the network's zero set);
 *  NR_SCENE_ROUND's is iso = atanhf(0.04).
 * Errors: NR_E_INVALID (ctx or opts NULL, n < 0, n > 2^30, X NULL with n > 0, every output NULL, tol
 * or max_step negative, a field of opts not finite, max_iters outside 0..4096), NR_E_STATE (no
 * network), NR_E_FORMAT (what nr_mlp_gradient refuses: a network the fused kernels do not take, or
 * more than 7 hidden 32 x 32 layers).  n = 0 returns NR_OK without a launch and leaves the outputs
 * untouched. */
#define NR_PROJ_CONVERGED 0  /* |value - iso| <= tol at the returned position */
#define NR_PROJ_LIMIT     1  /* max_iters steps taken and still not within tol */
#define NR_PROJ_FLAT      2  /* gradient zero or not a number: no step can be taken */
typedef struct nr_project_opts {
    float iso;       /* project onto {network value == iso} */
    float tol;       /* >= 0 */
    float max_step;  /* longest step, in world units; 0 = unlimited */
    int   max_iters; /* 0..4096 steps per point */
} nr_project_opts;
int nr_project_points(nr_ctx *ctx, const float *X /*[n][dims[0]]*/, long n, const nr_project_opts *opts,
                      float *position /*[n][3]*/, float *value /*[n]*/, float *normal /*[n][3]*/,
                      float *distance /*[n]*/, int32_t *iters /*[n]*/, int32_t *status /*[n]*/,
                      int loc, nr_stats *stats);

/* ---- fitting: train a network on the device ------------------------------------------ */
/* (new symbols and one new struct only: NR_ABI_VERSION stays 3, nr_stats is unchanged)
 * Fits a [3, 32, ..., 32, 1] ReLU network (nh <= 7 hidden 32 x 32 layers) to (point, value) pairs:
 * the gradient of the plain or clamped L2 loss with respect to every weight, and Adam, with the
 * weights, the moments and every sum on the device.  The caller supplies the initial weights in
 * nr_load_mlp's layout (the device draws no random numbers); nr_fit_weights returns them, and
 * nr_load_mlp of those builds every pack the renderer uses.  owner supplies the device and the
 * stream and needs no network; destroy the fit object before its owner.
 * Flat parameter order (grad, params; P = nr_fit_num_params): K_0, B_0, K_1, B_1, ..., K_last,
 * B_last, each kernel Keras (in, out) row-major.
 *
 * The arithmetic, all f32, one rounding per operation, no contraction except the fmaf named; S =
 * partials.  n points form ceil(n / 16) tiles of 16 consecutive points; a ragged last tile is
 * completed with points x = (0, 0, 0) whose e and g (step 2) are +0.0: they take part in every
 * chain below, where they change no bit unless an accumulator is -0.
 *  1. Forward: nr_mlp_forward's fp32 pass on the raw weights (each layer an ascending fmaf chain
 *     from +0, then + bias; a_l = max(z_l, 0), m_l = z_l > 0).  value[p] has the bits nr_mlp_forward
 *     returns for a context loaded with the same weights.
 *  2. Residual: with c = clamp > 0, vc = fminf(fmaxf(v, -c), c) and inside = v > -c && v < c; with
 *     clamp == 0, vc = v and inside = true.  e = vc - y, g = inside ? e : +0.0.
 *  3. Backward: nr_mlp_gradient's chains seeded with g: d_nh[u] = m_nh[u] ? K_last[u][0] * g : +0.0;
 *     for l = nh .. 1: acc[i] = chain over j ascending of fmaf(K_l[i][j], d_l[j], acc) from +0,
 *     d_(l-1)[i] = m_(l-1)[i] ? acc[i] : +0.0.
 *  4. Partial sums: tile t = p >> 4 belongs to partial t mod S.  Within a partial every sum is one
 *     chain from +0.0 over the partial's points (completed tiles) in ascending p:
 *       GK_last[u]: fmaf(a_nh[u], g, .);  GB_last: . + g;  SS: fmaf(e, e, .)
 *       GK_l[i][j]: fmaf(a_(l-1)[i], d_l[j], .);  GB_l[j]: . + d_l[j]   (l = 1 .. nh)
 *       GK_0[c][j]: fmaf(x_c, d_0[j], .);  GB_0[j]: . + d_0[j]
 *  5. Totals, in two levels fixed by S alone: the partials form 16 chunks of C = ceil(S / 16)
 *     consecutive partials (chunk k: partials k C .. min((k + 1) C, S) - 1; beyond S: empty).
 *     U_k = +0.0, then U_k = U_k + partial_s over the chunk's s ascending; T = +0.0, then
 *     T = T + U_k for k = 0 .. 15.  All S partials take part; one with no tile is +0.0.
 *  6. inv_n = 1.0f / (float)n; loss = SS_T * inv_n; G = T * inv_n.
 *  7. Adam, step t 1-based and kept in the object.  The host forms in double and rounds to f32:
 *     a_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t), omb1 = 1 - beta1, omb2 = 1 - beta2.  Per
 *     parameter, m and v from +0:  m = beta1 * m + omb1 * G;  v = beta2 * v + omb2 * (G * G);
 *     theta = theta - (a_t * m) / (sqrtf(v) + eps), sqrtf and the divide correctly rounded.
 * No sum depends on grid, the CU count or which wave ran what, and there are no floating-point
 * atomics: the same arguments give the same bits.
 *
 *  - nr_fit_opts: partials = S in 1..4096, 0 = 1024; grid = workgroups of the gradient launch, 0 =
 *    one per CU (at most ceil(S / 4)), which changes no bit.
 *  - nr_fit_gradient: loss [1], grad [P], value [n], any of them NULL; loc = NR_HOST or NR_DEVICE
 *    for all the pointers.  It leaves the weights and the step count alone.
 *  - nr_fit_run: n / batch Adam steps (n % batch == 0); step k takes rows [k batch, (k + 1) batch)
 *    as its n points, and loss[k] is their loss before the update.  Two launches per step and no
 *    synchronisation or read-back between steps; with loc = NR_DEVICE the call only enqueues (the
 *    step count advances at once).  stats (may be NULL): ray_steps = n, launches, ms_total;
 *    everything else 0.
 *  - nr_fit_weights: the master weights params [P] (host) and the steps taken; either may be NULL.
 * Errors: NR_E_INVALID (a NULL argument, n < 1, n > 2^30, n % batch != 0, lr or eps not finite and
 * positive, a beta outside [0, 1), clamp negative or not finite, partials outside 0..4096, grid
 * negative), NR_E_FORMAT (any other shape, 4 inputs included), NR_E_HIP, NR_E_NOMEM.
 * Memory: 16 P + 4 S (P + 1) bytes and the packs on the device until nr_fit_destroy, and for
 * NR_HOST callers staging of the points' size. */
typedef struct nr_fit nr_fit;
typedef struct nr_fit_opts {
    float lr, beta1, beta2, eps;  /* Adam */
    float clamp;                  /* c > 0: the clamped residual; 0: plain */
    int   partials;               /* S: partial sums, 1..4096; 0 = 1024 */
    int   grid;                   /* workgroups of the gradient launch; 0 = default */
} nr_fit_opts;
int nr_fit_create(nr_ctx *owner, int nlayers, const int *dims, const float *const *kernels,
                  const float *const *biases, const nr_fit_opts *opts, nr_fit **out);
int nr_fit_destroy(nr_fit *f);
int nr_fit_num_params(const nr_fit *f, long *count);
int nr_fit_gradient(nr_fit *f, const float *X /*[n][3]*/, const float *Y /*[n]*/, long n,
                    float *loss /*1 or NULL*/, float *grad /*[P] or NULL*/, float *value /*[n] or NULL*/, int loc);
int nr_fit_run(nr_fit *f, const float *X /*[n][3]*/, const float *Y /*[n]*/, long n, long batch,
               float *loss /*[n / batch] or NULL*/, int loc, nr_stats *stats);
int nr_fit_weights(nr_fit *f, float *params /*[P], host*/, long *step);

/* ---- triangle meshes: signed distance from points to a mesh ------------------------- */
/* (new symbols only: NR_ABI_VERSION stays 3, nr_stats is unchanged)
 * nr_obj_load reads a Wavefront OBJ; nr_trimesh_normals builds the pseudonormal table of a mesh;
 * a nr_trimesh holds a mesh, its table and a bounding-box hierarchy on the device, and
 * nr_trimesh_distance gives, per point, the signed distance to the mesh, the closest point, its
 * triangle and the feature of the triangle it lies on.  owner supplies the device and the stream and
 * needs no network; destroy the mesh object before its owner.
 *
 * nr_obj_load (host only).  Records `v x y z [w]` (w ignored) and `f` with corners i, i/t, i//n or
 * i/t/n, 1-based or negative (relative to the vertices read so far); a face of more than three
 * corners becomes a fan from its first corner.  Every other record is ignored.  NR_E_IO: the file
 * cannot be read.  NR_E_FORMAT: a vertex without three numbers, a corner that is no index, an index
 * out of range, a face of fewer than 3 corners.  vertices [nv][3] and triangles [nt][3] (0-based) are
 * the caller's to nr_free.  nr_obj_save -> nr_obj_load returns the same bits (%.9g round-trips f32).
 *
 * The pseudonormal table N [nt][7][3] (nr_trimesh_normals, host only): entry 0 the face, 1..3 the
 * edges AB, BC, CA, 4..6 the vertices A, B, C of triangle (A, B, C).  Computed in double from the f32
 * coordinates and rounded to f32 once, not normalised (only the direction is used):
 *   face    (b - a) x (c - a), normalised; a triangle whose cross product is 0 (zero area) or not
 *           finite has face entry (0, 0, 0);
 *   edge    the sum of the (double) face normals of every triangle that uses the undirected edge, in
 *           ascending triangle index; every triangle of the edge gets the same bits;
 *   vertex  the sum over the triangles that use the vertex, ascending triangle index, of angle * face
 *           normal, angle = atan2(|u x v|, u . v) of the two edges u, v leaving that corner;
 *           zero-area triangles are left out.
 * Vertices are identified by index, never by position.  closed = 1 iff every undirected edge is used
 * by exactly two triangles, once in each direction, and joins two different vertices.
 *
 * The distance, all f32, one rounding per operation, no contraction except the fmaf named.  For
 * vectors dot(u, v) = fmaf(u.z, v.z, fmaf(u.y, v.y, u.x * v.x)); differences and fmaf of vectors are
 * componentwise.
 *  1. Per triangle (a, b, c) and point p (Ericson, Real-Time Collision Detection 5.1.5):
 *       ab = b - a, ac = c - a, bc = c - b, ap = p - a, bp = p - b, cp = p - c
 *       d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp),
 *       d6 = dot(ac, cp);  vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4
 *       (two products and one subtraction each);  e43 = d4 - d3, e56 = d5 - d6.
 *     The first region that holds, in this order, gives the closest point q and the feature:
 *       4 (A)   d1 <= 0 && d2 <= 0:                q = a
 *       5 (B)   d3 >= 0 && d4 <= d3:               q = b
 *       1 (AB)  vc <= 0 && d1 >= 0 && d3 <= 0:     q = fmaf(ab, d1 / (d1 - d3), a)
 *       6 (C)   d6 >= 0 && d5 <= d6:               q = c
 *       3 (CA)  vb <= 0 && d2 >= 0 && d6 <= 0:     q = fmaf(ac, d2 / (d2 - d6), a)
 *       2 (BC)  va <= 0 && e43 >= 0 && e56 >= 0:   q = fmaf(bc, e43 / (e43 + e56), b)
 *       0 (face) otherwise: den = (va + vb) + vc;  q = fmaf(ac, vc / den, fmaf(ab, vb / den, a))
 *     (every quotient one correctly rounded division; a comparison with a NaN is false).
 *     d2(t) = dot(p - q, p - q).  A zero-area triangle (face entry (0, 0, 0)) has d2 = NaN by
 *     definition, whatever its corners.
 *  2. The winner is the triangle with the lexicographic minimum of (d2, triangle index) over all
 *     triangles of the mesh; a NaN d2 never wins (every comparison is d2 < best, or d2 == best with
 *     the smaller index).  A minimum does not depend on the order it is taken in: the result is the
 *     same bits for any traversal, leaf size, grid, or with NR_TRIMESH_BRUTE.  closest = q and
 *     feature of the winner (step 1 once more), tri = its index in the caller's triangles,
 *     d = sqrtf(d2), correctly rounded.
 *  3. Sign: s = dot(p - q, N[tri][feature]); sdf = s < 0 ? -d : d.  With the library's meshes
 *     ((b - a) x (c - a) points outward: step 4 of nr_mesh_grid) inside is negative.  The sign means
 *     something only for a closed mesh (closed = 1); otherwise it is computed all the same
 *     (nr_mesh_winding, below, signs the distance to a mesh that is not closed).
 *  4. A point with a non-finite coordinate, or a mesh of zero-area triangles only, gives sdf = closest =
 *     the quiet NaN 0x7fc00000 and tri = feature = -1.
 * The hierarchy (built by nr_trimesh_create on the host): a binary tree over the triangles' boxes,
 * split at the median of the centroids along the axis of their largest extent, ordered by
 * (coordinate, triangle index), until a node holds at most `leaf` triangles (0 = 8); its depth is at
 * most ceil(log2 nt) + 1 (checked against the walk's stack of 32 levels).  Every box is grown by
 * slack = 2^-18 (largest |coordinate| + largest axis extent of the vertices) and rounded outward; a
 * point's bound to a box is lb = 0.9999847412109375f (1 - 2^-16) * dot(g, g) with g the componentwise
 * gap max(lo - p, p - hi, 0), and a node is left out only when lb > best for every point that shares
 * the walk.  The result is therefore that of step 2 whenever every computed q lies inside its
 * triangle's grown box -- always, except for slivers whose quotients are rounding noise; with
 * NR_TRIMESH_BRUTE unconditionally.
 *
 *  - nr_trimesh_distance: any of sdf [n], closest [n][3], tri [n], feature [n] may be NULL; loc =
 *    NR_HOST or NR_DEVICE for X and all of them.  One launch; with loc = NR_DEVICE and no stats the
 *    call only enqueues.  Points are taken 64 at a time in the order given and the 64 share one walk:
 *    points that are neighbours in space should be neighbours in X (the call does not sort;
 *    nr_points_order, below, gives the order).
 *    stats (may be NULL): ray_steps = n, shade_evals = point-triangle evaluations done (summed over
 *    the points), launches, ms_total; everything else 0.
 *  - nr_trimesh_info: any output may be NULL; lo, hi = the vertices' bound (not grown); nodes and
 *    depth of the hierarchy.
 * Errors: NR_E_INVALID (a NULL owner, mesh, vertices, triangles, out or X; nv < 1; nt < 1; nt > 2^24;
 * an index outside 0..nv - 1; a vertex that is not finite; leaf outside 0..32; n < 1; n > 2^30; a flag
 * bit other than NR_TRIMESH_BRUTE), NR_E_IO and NR_E_FORMAT (nr_obj_load), NR_E_HIP, NR_E_NOMEM.
 * Memory on the device until nr_trimesh_destroy: 132 bytes per triangle (48: the reordered corners
 * and index; 84: the table) and 96 bytes per node (32: the box and the links; 64: the moments of
 * nr_mesh_winding; at most 2 ceil(nt / ceil(leaf / 2)) nodes), and for NR_HOST callers staging of
 * the points' and outputs' size.
 *
 * nr_mesh_winding: the generalized winding number (Jacobson et al. 2013) w of the mesh at each
 * point -- the signed solid angles of all triangles seen from the point, summed, over 4 pi -- through
 * the hierarchy with far nodes replaced by an expansion of their moments (Barill et al. 2018).  For a
 * closed mesh whose triangles wind outward w is 1 inside and 0 outside; for an open, overlapping or
 * nested mesh it varies smoothly and w >= 0.5 is the inside test.  Unlike the distance the result
 * depends on the hierarchy and on the order of the sum, so both are part of the contract
 * (tests/winding_ref.py restates it; nr_mesh_hierarchy returns the tree).  Both calls belong to the
 * nr_trimesh object above: nr_mesh_winding queries one, nr_mesh_hierarchy returns what its
 * creation builds.
 *
 * The hierarchy's layout (nr_mesh_hierarchy, host only, no device: exactly what nr_trimesh_create
 * uploads, the caller's to nr_free).  The live triangles -- those whose face entry is not (0, 0, 0) --
 * are reordered: order [ntl] is the original index of the triangle at each position.  nodes
 * [nnodes][8] 32-bit words, the root first, in preorder (a node, its left subtree, its right one):
 * words 0..2 and 4..6 the grown box (f32), word 3 | word 7 (int32) = first | -count of a leaf's
 * triangles, positions [first, first + count), or left | right child of an inner node (word 7 > 0).
 * A node's triangles are contiguous positions.  moments [nnodes][16] f32 per node:
 *     c.xyz, R2, N.xyz, 0, Sxx, Syy, Szz, Sxy, Sxz, Syz, 0, 0
 * computed in double from the f32 corners (a, b, c) of the node's triangles t in position order,
 * every sum sequential and every entry rounded to f32 once:
 *     A_t = 0.5 ((b - a) x (c - a)),  |A_t| = sqrt((A.x A.x + A.y A.y) + A.z A.z),
 *     x_t = ((a + b) + c) / 3.0
 *     c  = (sum |A_t| x_t) / (sum |A_t|), or (sum x_t) / count if the area sum is not > 0
 *     N  = sum A_t
 *     M  = sum A_t (x_t - c)^T  about the f32-rounded c;  Sxx = M00, Syy = M11, Szz = M22,
 *          Sxy = 0.5 (M01 + M10), Sxz = 0.5 (M02 + M20), Syz = 0.5 (M12 + M21)
 *     R2 = max over the corners v of the node's triangles of ((e.x e.x + e.y e.y) + e.z e.z),
 *          e = v - c (the rounded c), rounded up to f32.
 * (c is rounded before S and R2 are formed, so that they describe the centre the query uses.)
 *
 * The sum, all f64, one rounding per operation, no contraction; f32 values are promoted exactly;
 * dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z and len(u) = (double)sqrtf((float)dot(u, u)), the f32
 * square root correctly rounded.
 *  1. A triangle (A, B, C) seen from p, a = A - p, b = B - p, c = C - p:
 *       det = (a.x (b.y c.z - b.z c.y) + a.y (b.z c.x - b.x c.z)) + a.z (b.x c.y - b.y c.x)
 *       la = len(a), lb = len(b), lc = len(c)
 *       den = (((la lb) lc + dot(a, b) lc) + dot(b, c) la) + dot(c, a) lb
 *       Omega = 2 h(det, den)
 *  2. h(num, den), an atan2 from basic operations: with an = |num|, ad = |den|,
 *       t = (an < ad ? an : ad) / (an < ad ? ad : an)
 *       h = 0 if num == 0 or t is not finite (a NaN included): a point in the triangle's plane, or at
 *       a corner, contributes 0.  Otherwise
 *       u = t > 0.41421356237309503 ? (t - 1) / (t + 1) : t,  base = 0.7853981633974483 or 0,
 *       z = u u,  P = the Horner form of sum_{k = 0..11} (-1)^k z^k / (2k + 1) from k = 11 down
 *       (p = p z + c_k, two roundings a step, c_k the double nearest (-1)^k / (2k + 1)),
 *       h = base + u P;  then, in this order: an > ad: h = 1.5707963267948966 - h;  den < 0:
 *       h = 3.141592653589793 - h;  num < 0: h = -h.  (Within 1e-11 of atan2.)
 *  3. A node's expansion, from its moments: r = c - p, d2 = dot(r, r), d = (double)sqrtf((float)d2),
 *       d3 = d2 d,  s = ((Sxx r.x + Sxy r.y) + Sxz r.z, (Sxy r.x + Syy r.y) + Syz r.z,
 *       (Sxz r.x + Syz r.y) + Szz r.z),  q = dot(r, s),  tr = (Sxx + Syy) + Szz
 *       E = dot(N, r) / d3 + (tr / d3 - (3.0 q) / (d3 d2))
 *     The node is far for p iff d2 > ((double)beta (double)beta) (double)R2.
 *  4. W = 0; visit(root), where visit(node): far: W += E; else a leaf: W += Omega of its triangles
 *     in position order; else visit(left), visit(right).  w = (float)(W 0.07957747154594767).
 *     With NR_TRIMESH_BRUTE W is the sum of Omega over all positions in order; a walk in which no
 *     node is far gives the same bits.  A point's result does not depend on the other points.
 *  5. A point with a non-finite coordinate, or a mesh with no live triangle, gives the quiet NaN.
 *
 *  - nr_mesh_winding: winding [n] and sdf [n], at least one not NULL; beta finite and >= 0, 0 = 2.0
 *    (larger: fewer nodes far, closer to the exact sum, slower); flags 0 or NR_TRIMESH_BRUTE; loc for
 *    X and both outputs.  With sdf the call first runs nr_trimesh_distance's launch for the magnitude
 *    (the same bits, flags applied to it too) and then writes sdf = w >= 0.5f ? -|sdf| : |sdf|, a NaN
 *    left as it is: two launches on the stream, nothing read back between them.  With loc = NR_DEVICE
 *    and no stats the call only enqueues.  Points are taken 64 at a time in the order given and the
 *    64 share one walk, the union of their cuts through the tree: neighbours in space should be
 *    neighbours in X (the call does not sort; nr_points_order does).  stats: ray_steps = n, shade_evals = solid angles and
 *    expansions evaluated, summed over the points (plus the distance launch's evaluations with sdf),
 *    launches, ms_total.
 * Errors of nr_mesh_winding: as nr_trimesh_distance, and NR_E_INVALID for a beta that is negative
 * or not finite, or winding and sdf both NULL; of nr_mesh_hierarchy: as nr_trimesh_create (with any
 * NULL argument NR_E_INVALID). */
typedef struct nr_trimesh nr_trimesh;
#define NR_TRIMESH_BRUTE 1   /* visit every triangle, no hierarchy: the cross-check and the baseline */
int nr_obj_load(const char *path, float **vertices /*[nv][3]*/, long *nv, int32_t **triangles /*[nt][3]*/, long *nt);
int nr_trimesh_normals(const float *vertices /*[nv][3]*/, long nv, const int32_t *triangles /*[nt][3]*/, long nt,
                       float *table /*[nt][7][3] or NULL*/, int *closed /*or NULL*/);
int nr_trimesh_create(nr_ctx *owner, const float *vertices /*[nv][3], host*/, long nv,
                      const int32_t *triangles /*[nt][3], host*/, long nt, int leaf /*0 = 8, else 1..32*/,
                      nr_trimesh **out);
int nr_trimesh_destroy(nr_trimesh *m);
int nr_trimesh_info(const nr_trimesh *m, long *nv, long *nt, long *nodes, int *depth, float lo[3], float hi[3],
                    int *closed);
int nr_trimesh_distance(nr_trimesh *m, const float *X /*[n][3]*/, long n, float *sdf /*[n]*/,
                        float *closest /*[n][3]*/, int32_t *tri /*[n]*/, int32_t *feature /*[n]*/, int flags,
                        int loc, nr_stats *stats);
int nr_mesh_hierarchy(const float *vertices /*[nv][3]*/, long nv, const int32_t *triangles /*[nt][3]*/, long nt,
                      int leaf /*0 = 8, else 1..32*/, float **nodes /*[nnodes][8]*/, long *nnodes,
                      int32_t **order /*[ntl]: original index per position*/, long *ntl,
                      float **moments /*[nnodes][16]*/, int *depth);
int nr_mesh_winding(nr_trimesh *m, const float *X /*[n][3]*/, long n, float beta /*0 = 2.0*/,
                    float *winding /*[n] or NULL*/, float *sdf /*[n] or NULL*/,
                    int flags /*0 or NR_TRIMESH_BRUTE*/, int loc, nr_stats *stats);

/* ---- triangle meshes: ray casting and geometry buffers -------------------------------- */
/* (new symbols only: NR_ABI_VERSION stays 3, nr_stats is unchanged)
 * The third query of a nr_trimesh: rays.  nr_mesh_trace_rays casts caller-supplied rays,
 * nr_mesh_gbuffer the W x H pixel rays of the owner's view (nr_render's rays), nr_mesh_render shades
 * those into a frame.  The result is the closest hit of each ray, or with NR_MESH_RAY_ANY whether
 * there is any hit (occlusion and shadow rays).
 *
 * The contract, all f32, one rounding per operation, no contraction except the fmaf named; every `/`
 * one correctly rounded division; a comparison with a NaN is false.  The ray-triangle test is the
 * shear form of Woop, Benthin and Wald (Watertight Ray/Triangle Intersection, JCGT 2013): the edge
 * function of an edge shared by two triangles is the exact negation of the neighbour's, so no ray
 * slips between two triangles of a closed mesh.
 *  1. Per ray (o, d).  The ray is dead if any of its six numbers is not finite or d = (0, 0, 0): it
 *     returns MISS.  Otherwise kz = 0; if |d.y| > |d[kz]| then kz = 1; if |d.z| > |d[kz]| then kz = 2;
 *     kx = (kz + 1) % 3, ky = (kx + 1) % 3, swapped if d[kz] < 0;
 *       Sx = d[kx] / d[kz],  Sy = d[ky] / d[kz],  Sz = 1.0f / d[kz].
 *  2. Per live triangle (a, b, c) -- one whose face entry in the pseudonormal table is not (0, 0, 0);
 *     a zero-area triangle is never hit, by definition:
 *       A = a - o, B = b - o, C = c - o (componentwise)
 *       Px = P[kx] - Sx * P[kz],  Py = P[ky] - Sy * P[kz]           for P in A, B, C
 *       U = Cx * By - Cy * Bx,  V = Ax * Cy - Ay * Cx,  W = Bx * Ay - By * Ax
 *     (two products and one subtraction each).  The triangle is missed if
 *       (U < 0 || V < 0 || W < 0) && (U > 0 || V > 0 || W > 0)
 *     -- no back-face culling, no f64 fallback.  det = (U + V) + W; missed unless det != 0.  Then
 *       Pz = Sz * P[kz] for P in A, B, C;  Tn = (U * Az + V * Bz) + W * Cz;  t = Tn / det
 *     and the triangle is hit iff tmin <= t && t <= tmax.
 *  3. Closest hit: the winner is the lexicographic minimum of (t, original triangle index) over all
 *     hit triangles.  A minimum does not depend on the order it is taken in: the result is the same
 *     bits for any traversal, leaf size, grid, or with NR_TRIMESH_BRUTE.  A ray with a winner has
 *       status   = NR_RAY_HIT (2)
 *       t, tri   = the winner's t and its index in the caller's triangles
 *       bary     = (U / det, V / det, W / det): the weights of a, b, c
 *       position = fmaf(d, t, o), componentwise
 *       normal   = the table's face entry N[tri][0] as stored, not turned towards the ray; or with
 *                  NR_MESH_RAY_SMOOTH, with normalise(v) = v * (1.0f / sqrtf((v.x v.x + v.y v.y) +
 *                  v.z v.z)) (nr_trace_rays' normal): n_k = normalise(N[tri][4 + k]) for the corners
 *                  k = A, B, C, the face entry instead where the corner's squared length is 0 or not
 *                  finite; m = fmaf(n_C, bary[2], fmaf(n_B, bary[1], n_A * bary[0])) componentwise;
 *                  normal = normalise(m), the face entry where m's squared length is 0 or not finite.
 *     Every other ray, a dead one included, has status = NR_RAY_MISS (0), tri = -1 and t, bary,
 *     position, normal all +0.0.
 *  4. NR_MESH_RAY_ANY: status = NR_RAY_HIT iff some live triangle is hit under step 2, else
 *     NR_RAY_MISS; existence does not depend on the traversal.  Only status may be asked for.
 *  5. The walk (not part of the bits, only of the cost).  A node is left out only if no ray that
 *     shares the walk wants it.  A ray wants a node unless tn > tf, or tf < tmin, or tn > min(best,
 *     tmax) (strict: a tie in t with a smaller index is still found), where best is the ray's
 *     smallest t so far and [tn, tf] its slab interval of the node's stored (grown) box widened by
 *       pad = 2^-18 * (max(|o.x|, |o.y|, |o.z|) + S),
 *     S = the scale of the boxes' slack (largest |coordinate| + largest axis extent of the vertices):
 *       t1, t2 = ((lo - pad) - o) * (1.0f / d), ((hi + pad) - o) * (1.0f / d)     per axis
 *       tn = max over the axes of min(t1, t2),  tf = min over the axes of max(t1, t2)
 *     with min and max that ignore a NaN.  The rounding of step 2 scales with |a - o|, not with the
 *     mesh, which is why the pad depends on the origin.  The result is therefore that of step 3
 *     whenever every hit's t lies inside the slab interval of its triangle's widened box -- always
 *     in tests/test_mesh_rays_cpu.py, origins up to |o| = 100 included; with NR_TRIMESH_BRUTE
 *     unconditionally.
 *
 *  - nr_mesh_trace_rays: dirs is used as given and t is in units of d; tmin <= tmax, neither a NaN,
 *    tmax may be +INFINITY.  Any of status [n], t [n], tri [n], bary [n][3], position [n][3],
 *    normal [n][3] may be NULL; loc = NR_HOST or NR_DEVICE for the rays and all of them.  One launch;
 *    with loc = NR_DEVICE and no stats the call only enqueues.  Rays are taken 64 at a time in the
 *    order given and the 64 share one walk: rays that are neighbours in space should be neighbours in
 *    the arrays (the call does not sort).  stats (may be NULL): ray_steps = n, rays_hit = the HITs,
 *    shade_evals = ray-triangle evaluations summed over the live rays, launches, ms_total;
 *    everything else 0.
 *  - nr_mesh_gbuffer: the W x H pixel rays of the owner's view (nr_set_view), generated in the kernel
 *    with nr_render's arithmetic; pixel (x, y) is at index y * W + x; tmin = 0, tmax = +INFINITY.  A
 *    wave takes one 8 x 8 pixel tile.  W * H <= 2^30.
 *  - nr_mesh_render: the same rays; a HIT pixel is nr_render's colour of (normal, ray direction) with
 *    the owner's colouring (nr_set_static's colour type, nr_set_matcap, the normal matrix of
 *    nr_set_view), every other pixel 0.  NR_E_STATE for matcap colouring without a matcap, as
 *    nr_render.  flags: NR_TRIMESH_BRUTE and NR_MESH_RAY_SMOOTH.
 * Errors: as nr_trimesh_distance (a NULL mesh, n outside [1, 2^30], an unknown flag bit, NR_E_HIP,
 * NR_E_NOMEM), and NR_E_INVALID for NULL origins or dirs, a tmin or tmax that is a NaN or tmin > tmax,
 * W or H < 1, W * H > 2^30, a NULL out, NR_MESH_RAY_ANY with NR_MESH_RAY_SMOOTH or with any output
 * other than status.  A mesh with no live triangle gives MISS everywhere. */
#define NR_MESH_RAY_ANY    2  /* status only: is any triangle hit in [tmin, tmax] */
#define NR_MESH_RAY_SMOOTH 4  /* normal interpolated from the vertex pseudonormals */
int nr_mesh_trace_rays(nr_trimesh *m, const float *origins /*[n][3]*/, const float *dirs /*[n][3]*/, long n,
                       float tmin, float tmax, int32_t *status /*[n]*/, float *t /*[n]*/, int32_t *tri /*[n]*/,
                       float *bary /*[n][3]*/, float *position /*[n][3]*/, float *normal /*[n][3]*/, int flags,
                       int loc, nr_stats *stats);
int nr_mesh_gbuffer(nr_trimesh *m, int W, int H, int32_t *status, float *t, int32_t *tri, float *bary,
                    float *position, float *normal, int flags, int loc, nr_stats *stats);
int nr_mesh_render(nr_trimesh *m, uint32_t *out /*[H][W]*/, int W, int H, int flags, int out_loc, nr_stats *stats);

/* ---- triangle meshes: fitting samples, drawn, ordered and labelled on the device ------- */
/* (new symbols only: NR_ABI_VERSION stays 3, nr_stats is unchanged)
 * The stage between a mesh and nr_fit_run: nr_mesh_sample draws seeded points on the surface of a
 * nr_trimesh (in proportion to triangle area, optionally jittered) and in a box; nr_points_order gives
 * the Morton order or a seeded shuffle of any point set, by a stable sort on the device;
 * nr_mesh_fit_samples runs draw -> Morton order -> signed distance -> shuffle in one call and leaves
 * X [n][3], Y [n] for nr_fit_run, nothing read back.  Every bit is fixed by this text -- integers,
 * and the f32 operations named, one rounding each, no transcendental function -- and
 * tests/sample_ref.py restates it in numpy.
 *
 *  1. Random numbers: Philox4x32-10 (Salmon et al. 2011, Random123) with key (k0, k1) = (seed low 32,
 *     seed high 32) and counter (c0, c1, c2, c3) = (i low 32, i high 32, stream, 0), i the sample's index
 *     in the output.  Ten rounds of
 *       p0 = 0xD2511F53 * c0,  p1 = 0xCD9E8D57 * c2                      (64-bit products)
 *       (c0, c1, c2, c3) = (hi(p1) ^ c1 ^ k0, lo(p1), hi(p0) ^ c3 ^ k1, lo(p0))
 *       k0 += 0x9E3779B9,  k1 += 0xBB67AE85                               (mod 2^32)
 *     give the words w0..w3.  Known answers: zero counter and key -> 6627e8d5 e169c58d bc57ac4c
 *     9b00dbd8; all-ones counter and key -> 408f276d 41c83b0e a20bc7c6 6d5451fd.  Streams: 0 draws the
 *     sample, 1, 2, 3 jitter x, y, z, 4 is the shuffle key.
 *  2. The area table (built by nr_trimesh_create on the host; nr_mesh_area_table returns it without a
 *     device, from the same code) over the live triangles in position order, nr_mesh_hierarchy's
 *     `order` -- neighbours in the table are neighbours in space.  In f64 from the f32 corners, as the
 *     moments above:  |A_p| = sqrt((A.x A.x + A.y A.y) + A.z A.z),  A = 0.5 ((b - a) x (c - a));
 *     C_p = the sequential running sum of |A_p|;  T_p = min(floor(C_p / C_last * 2^32), 2^32 - 1) as
 *     uint32;  L = the last position whose T exceeds its predecessor's (T_-1 = 0).  If C_last is not
 *     > 0 (no live triangle) every T is 0 and L = -1.
 *  3. Surface samples, i < n_surface.  Position p = min(#{q : T_q <= w0}, L): a triangle is picked
 *     with probability (T_p - T_p-1) / 2^32, a triangle of zero share never.  tri = order[p].  With
 *     (a, b, c) the triangle's corners:  iu = w1 >> 8, iv = w2 >> 8;  if iu + iv > 2^24 then
 *     iu = 2^24 - iu, iv = 2^24 - iv;  u = iu 2^-24, v = iv 2^-24 (exact);  e1 = b - a, e2 = c - a (f32);
 *       point_k = fmaf(v, e2_k, fmaf(u, e1_k, a_k))  per axis k,
 *       bary = ((2^24 - iu - iv) 2^-24, u, v).
 *  4. Jitter, when sigma > 0, of the surface samples only: for axis k, S = the sum of the eight 16-bit
 *     halves of the four words of stream 1 + k;  g = (float)(S - 262140) * c, c the f32 with bits
 *     0x379cc471 (sqrt(1.5) / 65536);  point_k = fmaf(sigma, g, point_k).  g is a sum of eight uniform
 *     terms, not a normal deviate: mean 0, variance 1, support about +-4.9, and exact in integers up
 *     to one product, which no inverse-CDF or Box-Muller deviate would be; eight terms are close
 *     enough to a bell to smear a surface.  tri and bary stay those of the point before the jitter.
 *  5. Volume samples, i >= n_surface: point_k = fmaf((float)(w_k >> 8) * 2^-24, hi_k - lo_k, lo_k) with
 *     the words of stream 0 and hi_k - lo_k one f32 subtraction; tri = -1, bary = 0.
 *  6. Order keys.  NR_ORDER_MORTON: inv_k = 1023.0f / (hi_k - lo_k) in f32;  t = (x_k - lo_k) * inv_k;
 *     q_k = 1023 if t >= 1023, else (int)t if t > 0, else 0 (so a NaN gives 0, a point outside the box
 *     its nearest cell);  key = the 30-bit interleave of q, x in bit 0, y in bit 1, z in bit 2, and so on.
 *     NR_ORDER_SHUFFLE: key = w0 of stream 4 at counter i; X may be NULL (and sorted then too).
 *  7. perm = the stable ascending sort of the keys, ties by index -- numpy's argsort(key,
 *     kind="stable") -- and sorted[j] = X[perm[j]].  n in [1, 2^27].  (Equal shuffle keys are rare but
 *     possible; the tie rule keeps perm a permutation and a function of the seed.)
 *  8. nr_mesh_fit_samples = bit for bit, with n = n_surface + n_volume <= 2^27:  nr_mesh_sample into
 *     scratch;  nr_points_order MORTON with the box lo / hi;  nr_trimesh_distance (sign =
 *     NR_SAMPLE_SIGN_NORMAL) or nr_mesh_winding's sdf output with beta (NR_SAMPLE_SIGN_WINDING) of the
 *     sorted points;  nr_points_order SHUFFLE with the same seed;  X and Y = the sorted points and
 *     their values gathered by that permutation.  The distance's winner is a minimum and a point's
 *     winding sum does not depend on the other points, so Y does not depend on the order it was
 *     computed in: the Morton order is there for speed only (the 64 points of a walk are neighbours).
 *
 *  - nr_mesh_area_table (host only, no device): thresholds [ntl], the caller's to nr_free; last = L.
 *  - nr_mesh_sample: points [n][3], tri [n] or NULL, bary [n][3] or NULL; loc for all three.  One
 *    launch; with loc = NR_DEVICE and no stats the call only enqueues.  stats: ray_steps = n, launches,
 *    ms_total.  NR_E_STATE: n_surface > 0 on a mesh whose area sum is not > 0 (creating one works).
 *  - nr_points_order: perm [n] int32, sorted [n][3] or NULL; loc for X, perm and sorted; lo and hi are
 *    read in MORTON mode only, seed in SHUFFLE mode only.  The sort is a least-significant-digit radix
 *    sort of four 8-bit passes (count, scan, scatter: 13 launches, 14 with sorted) in which no
 *    workgroup waits on another; scratch, 16 bytes per point and 1 KiB per 2048 points, is held by the
 *    context and reused.  stats: ray_steps = n, launches, ms_total.
 *  - nr_mesh_fit_samples: X [n][3], Y [n]; loc for both.  stats: ray_steps = n, shade_evals = the
 *    query's evaluations, launches, ms_total.  Scratch of 48 bytes per sample is held by the context.
 * Errors: as nr_trimesh_distance (a NULL mesh, ctx or output, NR_E_HIP, NR_E_NOMEM), and NR_E_INVALID
 * for a NULL opts, a negative count, n = 0 or n > 2^27, a sigma that is negative or not finite, a box
 * with hi_k <= lo_k or an edge that is not finite, an unknown mode or sign, a beta that is negative
 * or not finite, X NULL in MORTON mode, sorted without X. */
typedef struct nr_sample_opts {
    uint64_t seed;
    long n_surface;      /* points on the surface, area-weighted, first in the output */
    long n_volume;       /* points uniform in the box [lo, hi], after them */
    float sigma;         /* jitter of the surface points, >= 0; 0 = none */
    float lo[3], hi[3];  /* the box: volume points, and the Morton quantisation of nr_mesh_fit_samples */
    int sign;            /* nr_mesh_fit_samples: NR_SAMPLE_SIGN_NORMAL or NR_SAMPLE_SIGN_WINDING */
    float beta;          /* for WINDING, 0 = 2.0 */
} nr_sample_opts;
#define NR_SAMPLE_SIGN_NORMAL  0  /* nr_trimesh_distance's sign (the pseudonormal's) */
#define NR_SAMPLE_SIGN_WINDING 1  /* nr_mesh_winding's sdf output */
#define NR_ORDER_MORTON  0
#define NR_ORDER_SHUFFLE 1
int nr_mesh_area_table(const float *vertices /*[nv][3]*/, long nv, const int32_t *triangles /*[nt][3]*/, long nt,
                       int leaf /*0 = 8, else 1..32*/, uint32_t **thresholds /*[ntl]*/, long *ntl, long *last);
int nr_mesh_sample(nr_trimesh *m, const nr_sample_opts *opts, float *points /*[n][3]*/, int32_t *tri /*[n] or NULL*/,
                   float *bary /*[n][3] or NULL*/, int loc, nr_stats *stats);
int nr_points_order(nr_ctx *ctx, const float *X /*[n][3] or NULL*/, long n, int mode, const float lo[3],
                    const float hi[3], uint64_t seed, int32_t *perm /*[n]*/, float *sorted /*[n][3] or NULL*/,
                    int loc, nr_stats *stats);
int nr_mesh_fit_samples(nr_trimesh *m, const nr_sample_opts *opts, float *X /*[n][3]*/, float *Y /*[n]*/, int loc,
                        nr_stats *stats);

/* ---- a mesh's signed distance on a lattice, remeshed ------------------------------- */
/* (new symbols only: NR_ABI_VERSION stays 3; named nr_mesh_* like every query added since
 * nr_trimesh_distance -- nr_mesh_winding, nr_mesh_trace_rays, nr_mesh_fit_samples -- the nr_trimesh_*
 * names being the object's own: create, destroy, info, normals, distance)
 *
 * The lattice calls of a triangle mesh: nr_sample_grid, nr_extract_mesh and nr_extract_mesh_sparse
 * with the mesh's signed distance in place of the network.  The points are generated in the kernel;
 * there is no new arithmetic, every rule refers to an existing one.  The winding-signed distance of
 * an open or self-overlapping mesh, remeshed, is a closed and consistently oriented mesh (repair);
 * iso != 0 gives offset surfaces and shells.
 *  1. Lattice.  nr_sample_grid's: index (k * ny + j) * nx + i, coordinate origin[a] +
 *     (float)idx_a * step[a].
 *  2. Value.  The value at a lattice point is, bit for bit, what the point calls return for X = that
 *     point's three coordinates: sign = NR_SAMPLE_SIGN_NORMAL nr_trimesh_distance's sdf;
 *     NR_SAMPLE_SIGN_WINDING nr_mesh_winding's sdf output with that beta (0 = 2.0) -- the distance
 *     launch's magnitude signed by w >= 0.5f, in a second launch.  NaN results are kept: a
 *     coordinate that overflows, or a mesh without live triangles.  Both point calls make a point's
 *     result independent of the other 63 points of its wave, so any assignment of lattice points to
 *     waves gives these bits; a wave here takes a 4 x 4 x 4 block of the lattice.  NR_TRIMESH_BRUTE
 *     (nr_mesh_sample_grid's flags) as in the point calls: the same bits without the hierarchy.
 *  3. nr_mesh_sample_grid: sdf [nz][ny][nx] (loc), dims >= 1, at most 2^30 points.  For
 *     loc = NR_HOST the lattice is staged in the owner context's buffer.
 *  4. nr_mesh_remesh = nr_mesh_sample_grid into a buffer the owner context keeps (as
 *     nr_extract_mesh does), then nr_mesh_grid's passes on it: vertices and triangles are exactly
 *     nr_mesh_grid's for those values -- order, capacities, the counting call (vertices ==
 *     triangles == NULL) and errors included; dims >= 2.  source_tri[v], when given, is
 *     nr_trimesh_distance's tri for vertex v's position, from one more k_trimesh_distance launch
 *     over the vertex array on the device: the original triangle nearest each new vertex, by which
 *     a caller carries attributes across.  loc applies to vertices, source_tri and triangles.
 *  5. nr_mesh_remesh_sparse = rules 1, 2 and 4-9 of nr_extract_mesh_sparse with rule 3's value
 *     replaced by 2 above and `normals` replaced by source_tri (which needs vertices).
 *     Why the band is sound here when it is not for a network: the unsigned distance to a mesh is
 *     1-Lipschitz, and so is the signed one across a closed surface.  A brick that holds a crossing
 *     cell has, on a crossing edge of that cell, a point at the level; that point is within half
 *     the brick's diagonal plus one cell diagonal of the brick's nearest corner, so that corner's
 *     value is within that much of iso -- at most the brick's diagonal for B >= 4 (B/2 + 1 <= B
 *     cells per axis), which is the band the Python wrapper passes for band=None.
 *     What stays unproven: the f32 rounding of the distances (a few ulp against a band of whole
 *     cells); the sign from the beta-approximated winding number; and the winding sign's jumps away
 *     from the surface of an open mesh -- the cap that closes a hole is a level crossing with
 *     |sdf| large on both sides, and it can pass through a brick without flipping one of its
 *     corners.  There band = +INFINITY is the safe choice.
 *  6. Stats (may be NULL).  ray_steps = lattice points evaluated (sparse: rule 7 of
 *     nr_extract_mesh_sparse); shade_evals = point-triangle evaluations (source_tri's launch
 *     included) plus, with NR_SAMPLE_SIGN_WINDING, the solid angles and expansions; rays_hit =
 *     active bricks (sparse); rays_shaded = *nv (the two remesh calls); launches and ms_total as
 *     elsewhere.
 *  7. Errors.  The lattice and capacity errors are those of nr_sample_grid, nr_extract_mesh and
 *     nr_extract_mesh_sparse (no NR_E_STATE / NR_E_FORMAT: no network is needed).  NR_E_INVALID
 *     too for an unknown sign, a beta that is negative or not finite, unknown flag bits, and a
 *     NULL mesh (recorded without a context).
 *  8. Scratch.  The owner context's, shared with its own lattice calls: do not run them
 *     concurrently. */
int nr_mesh_sample_grid(nr_trimesh *m, const float origin[3], const float step[3], const int dims[3],
                           int sign, float beta /*WINDING only; 0 = 2.0*/, int flags /*0 or NR_TRIMESH_BRUTE*/,
                           float *sdf /*[nz][ny][nx]*/, int loc, nr_stats *stats);
int nr_mesh_remesh(nr_trimesh *m, const float origin[3], const float step[3], const int dims[3], float iso,
                      int sign, float beta, float *vertices /*[v_cap][3]*/, int32_t *source_tri /*[v_cap] or NULL*/,
                      long v_cap, int32_t *triangles /*[t_cap][3]*/, long t_cap, long *nv, long *nt, int loc,
                      nr_stats *stats);
int nr_mesh_remesh_sparse(nr_trimesh *m, const float origin[3], const float step[3], const int dims[3], float iso,
                             int sign, float beta, int brick, float band, float *vertices, int32_t *source_tri,
                             int64_t *keys /*or NULL*/, long v_cap, int32_t *triangles, long t_cap, long *nv, long *nt,
                             long *active_bricks /*or NULL*/, int loc, nr_stats *stats);

/* ---- triangle meshes: the object built on the device ------------------------------- */
/* (new symbols only: NR_ABI_VERSION stays 3, nr_stats is unchanged; named nr_mesh_* like everything
 * added since nr_trimesh_distance -- see the remesh section above)
 * nr_mesh_create_device is nr_trimesh_create for vertices and triangles that are in device
 * memory -- the meshes of nr_extract_mesh*, nr_compose_extract_mesh* and nr_mesh_remesh*: table,
 * order, tree, moments and area table are made by kernels, no geometry crosses to the host, and every
 * query above takes the object unchanged.  nr_mesh_download returns what any nr_trimesh holds.
 *
 * The contract of a device-built mesh.  libm's atan2, nth_element's order inside a leaf and one
 * sequential f64 sum over all triangles cannot be had from kernels, so a device-built mesh has its
 * own contract, to the bit (tests/trimesh_device_ref.py restates it in numpy): node layout, words,
 * slack, box growth, the moments' formulas and the area table's T and L are those above; what
 * differs is this.  f64 from the f32 coordinates, one rounding per operation, no contraction; dot and
 * len are nr_mesh_winding's: dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z, len(u) =
 * (double)sqrtf((float)dot(u, u)).
 *  1. Bound.  lo, hi and the largest |coordinate| over all nv vertices, exact, -0 below +0;
 *     slack = 2^-18 (largest |coordinate| + largest axis extent) in f64, as above.
 *  2. Table, each entry rounded to f32 once.
 *     face    n = (b - a) x (c - a); (0, 0, 0), the triangle dead, if n is (0, 0, 0) or not finite;
 *             else s = max |n_k|, m = n / s (three divisions), the entry m / len(m) (three more).
 *     edge    as above: the sum of the f64 face normals of every use of the undirected edge, in
 *             ascending triangle index.
 *     vertex  the sum over the live triangles that use the vertex, ascending triangle index, of
 *             angle * face normal (per component s = s + angle * n), angle = h(len(u x v), dot(u, v))
 *             with h of nr_mesh_winding's step 2 (the angle is h, not 2 h).
 *     closed  as above.
 *  3. Order.  Centroid x_k = ((a_k + b_k) + c_k) / 3.0f in f32; key = the NR_ORDER_MORTON key of x in
 *     the box [lo, hi] of 1 (rule 6 of the fitting samples; an axis of no extent gives cell 0); a dead
 *     triangle's key is 2^30.  order = the first ntl entries of the stable ascending sort of the
 *     keys, ties by triangle index; ntl = the live triangles.
 *  4. Tree.  The node of positions [first, first + count) is a leaf if count <= leaf, else it splits
 *     at half = (count + 1) / 2; preorder.  Words 3 and 7 are therefore those of the host tree for
 *     the same (ntl, leaf), and depth <= ceil(log2 ntl) + 1.  A box is the exact f32 bound of the
 *     node's corners, grown by slack in f64 and rounded outward as above.  ntl = 0: the one empty
 *     leaf.
 *  5. Moments.  Per position A_t and x_t as above, |A_t| = len(A_t).  A leaf's raw sums, sequential
 *     in position order: sa = sum |A|, sx = sum |A| x, mx = sum x, N = sum A, P = sum A x^T; an inner
 *     node's are left + right, one addition per entry.  c as above from sa, sx, mx and the count,
 *     rounded to f32; M = P - N c^T about the rounded c, one product and one subtraction per entry;
 *     S from M and the record as above; R2 as above (a maximum: no order).
 *  6. Area table.  |A_p| as in 5; C_p = base[p / 256] + the sequential running sum inside p's block
 *     of 256 positions, base = the sequential exclusive sum of the blocks' totals, C_last the sum
 *     after the last block; T and L as above.
 *
 *  - nr_mesh_create_device: limits and errors as nr_trimesh_create; indices and vertices are
 *    checked by a kernel (NR_E_INVALID, *out = NULL, nothing kept).  The arrays are read during the
 *    call only.  The host reads back two records of 128 bytes (the error flags, the bound, ntl;
 *    closed and L) and makes the tree's shape, a function of (ntl, leaf), between them; the call
 *    returns when the mesh is built.  Two radix sorts (nr_points_order's passes) of nt and 3 nt
 *    keys, one launch per level of the tree: 36 + depth launches.  Scratch held by the owner context
 *    and reused: 98 bytes per triangle and 204 bytes per node of the tree nt live triangles would
 *    give (leaf 8: fewer than nt / 2 nodes, so at most 200 bytes per triangle; leaf 1: 2 nt - 1
 *    nodes).  stats (may be NULL): ray_steps = nt, launches, ms_total.
 *  - nr_mesh_download: what the object holds, however built; any pointer may be NULL.  nodes
 *    [nodes of nr_trimesh_info][8], order [ntl], moments [nodes][16], table [nt][7][3], thresholds
 *    [ntl] (size them by nt and 2 nt nodes, or call once for ntl).  For a host-built mesh these are
 *    nr_mesh_hierarchy's, nr_trimesh_normals' and nr_mesh_area_table's bytes.  NR_E_INVALID: a
 *    NULL mesh. */
int nr_mesh_create_device(nr_ctx *owner, const float *d_vertices /*[nv][3], device*/, long nv,
                             const int32_t *d_triangles /*[nt][3], device*/, long nt,
                             int leaf /*0 = 8, else 1..32*/, nr_trimesh **out, nr_stats *stats /*or NULL*/);
int nr_mesh_download(nr_trimesh *m, float *nodes /*[nnodes][8]*/, int32_t *order /*[ntl]*/,
                        float *moments /*[nnodes][16]*/, float *table /*[nt][7][3]*/,
                        uint32_t *thresholds /*[ntl]*/, long *ntl, long *area_last);

/* ---- composed scenes: several networks, placed and combined by CSG ---------------- */
/* (new symbols and new structs only: NR_ABI_VERSION stays 3, nr_stats is unchanged)
 *
 * A composition holds copies of the fp32 packs of 1..NR_COMPOSE_MAX_NETS source contexts and
 * 1..NR_COMPOSE_MAX_PARTS parts, each one network rotated, moved and uniformly scaled, folded in
 * part order by union or subtraction.  It is created on an owner context, which supplies the device,
 * the stream, the view, the frame number, the colour settings and the matcap at the time of each
 * call; the owner needs no network of its own.  The source contexts may be destroyed after
 * nr_compose_create; the composition must be destroyed before its owner.
 *
 * The field.  All arithmetic is f32, one rounding per operation, no contraction; dot3(a, b) =
 * (a0 b0 + a1 b1) + a2 b2.  For a world point p and part j, with inv_s = 1.0f / scale:
 *     v   = p - pos
 *     q_k = ((v.x rot[0 + k] + v.y rot[3 + k]) + v.z rot[6 + k]) * inv_s,   k = 0, 1, 2
 *     qq  = dot3(q, q)
 *     d_j = qq <= 1.45f ? scale * tanh(net_j(q[, (float)frame]))    (NR_SCENE_TANH's value)
 *                       : scale * (sqrtf(qq) - 1.19f)               (the bound's distance; a NaN qq too)
 * and d = d_0, owner = 0; then for j = 1 .. nparts - 1: a union takes d_j where d_j < d, a subtraction
 * takes -d_j where -d_j > d, and owner = j where it took.  A NaN comparison is false.  The network is
 * only evaluated where qq <= 1.45: a part costs a ray far from it no evaluation.
 *
 * The bound.  centre c = the mean of the part positions (in double, rounded to f32); radius =
 * max_j(|pos_j - c| (1 + 2^-20) + (double)(1.2f * scale_j)), rounded up to f32 (nr_compose_info).
 *
 * Rays.  The entry is nr_trace_rays' on o - c and radius * radius; tnear = max(tnear, 0), p = o + d *
 * tnear, tfar = tfar - tnear (the remaining interval; the single-network calls keep the reference's
 * unreduced tfar).  Each iteration: tstep = field(p); tfar -= tstep; tfar <= 0 -> ESCAPED; else p += d *
 * tstep, travel += tstep, and tstep < 1e-6 -> HIT when an iteration is left, else LIMIT, as
 * nr_trace_rays; t = tnear + travel.  A HIT's normal is the normalised tetrahedral gradient of the
 * composed field at p (epsilon 1e-5); part[i] = the owner at the converging step, -1 for every other
 * status.  A ray's results depend only on that ray. */
#define NR_COMPOSE_MAX_NETS 4
#define NR_COMPOSE_MAX_PARTS 16
#define NR_PART_UNION 0
#define NR_PART_SUBTRACT 1
typedef struct nr_part {
    int net;        /* index into the nets given at creation */
    int op;         /* NR_PART_UNION, NR_PART_SUBTRACT; part 0 must be a union */
    float rot[9];   /* row-major rotation, local -> world (orthonormal, det +1) */
    float pos[3];   /* world position of the local origin */
    float scale;    /* uniform, > 0 */
} nr_part;
typedef struct nr_compose nr_compose;
typedef struct nr_compose_stats {
    uint64_t ray_steps;    /* sum of the rays' steps (field evaluations of marching rays) */
    uint64_t shade_evals;  /* 4 per HIT with normals, else 0 */
    uint64_t rays_hit;     /* rays that entered the bound */
    uint64_t rays_shaded;  /* HITs */
    uint64_t part_evals;   /* (marching ray, part) pairs inside that part's bound: network evaluations a ray needed */
    uint64_t wave_evals;   /* network evaluations issued, per wave (march, normals and samples); depends on the grouping */
    uint64_t wave_skips;   /* (wave, part) pairs with no lane in bound: evaluations not issued; depends on the grouping */
    int32_t iterations;    /* the largest steps */
    int32_t launches;
    float ms_total;
} nr_compose_stats;
/* Errors of create / set_parts, before any launch: NR_E_INVALID (a NULL argument, nnets outside
 * 1..4, nparts outside 1..16, a net index out of range, part 0 not a union, an unknown op, a scale
 * that is not finite or <= 0, max |R R^T - I| > 1e-4 or det < 0, a non-finite position, a source on
 * another device, the packs and the per-wave lists over the LDS of a CU), NR_E_STATE (a source
 * without a network), NR_E_FORMAT (a source whose network the fused kernels do not take). */
int nr_compose_create(nr_ctx *owner, nr_ctx *const *nets, int nnets, const nr_part *parts, int nparts,
                      nr_compose **out);
int nr_compose_destroy(nr_compose *c);
/* The checks create and set_parts make on the parts (for nnets networks) and the bound above, on the
 * host alone: no context, no device.  center and radius may be NULL. */
int nr_compose_bound(const nr_part *parts, int nparts, int nnets, float center[3], float *radius);
/* New transforms, ops or part count; the packs stay where they are. */
int nr_compose_set_parts(nr_compose *c, const nr_part *parts, int nparts);
/* Any pointer may be NULL. */
int nr_compose_info(const nr_compose *c, int *nnets, int *nparts, float center[3], float *radius);
/* value[i] = the field at points[i], owner[i] = its owner; on the points of a lattice the values are
 * what nr_mesh_grid takes.  n <= 2^30; n = 0 returns NR_OK without a launch. */
int nr_compose_sample(nr_compose *c, const float *points /*[n][3]*/, long n, float *value /*[n]*/,
                      int32_t *owner /*[n]*/, int loc, nr_compose_stats *stats);
/* nr_trace_rays through the composed field (above); part [n] as the other outputs, any may be NULL. */
int nr_compose_trace_rays(nr_compose *c, const float *origins /*[n][3]*/, const float *dirs /*[n][3]*/, long n,
                          int max_steps, int32_t *status, int32_t *steps, float *t, float *position /*[n][3]*/,
                          float *normal /*[n][3]*/, int32_t *part, int loc, nr_compose_stats *stats);
/* The same for the W x H pixel rays of the owner's view (nr_render_gbuffer's rays); W * H <= 2^30. */
int nr_compose_gbuffer(nr_compose *c, int W, int H, int max_steps, int32_t *status, int32_t *steps, float *t,
                       float *position, float *normal, int32_t *part, int loc, nr_compose_stats *stats);
/* The frame: a HIT pixel gets the owner's colouring (facing, or its matcap) of the composed normal,
 * every other pixel 0 -- the geometry buffer and one colouring launch.  part (may be NULL) as above.
 * NR_E_STATE for matcap colouring without a matcap. */
int nr_compose_render(nr_compose *c, uint32_t *out /*W*H*/, int W, int H, int max_steps, int32_t *part /*W*H or NULL*/,
                      int loc, nr_compose_stats *stats);

/* ---- composed scenes: ambient occlusion and shadows cast between parts ------------- */
/* (one new symbol: NR_ABI_VERSION stays 3; nr_light, nr_stats and nr_compose_stats are unchanged)
 *
 * nr_render_lit for a composition: the frame of nr_compose_render lit by one directional light, the
 * occlusion and the shadow taken from the composed field, so that a part darkens the others and a
 * cut-out lies in the shadow of what surrounds it -- the geometry buffer, one persistent lighting
 * launch over the composed field, one compositing launch; no host round trip.  Rules 1-9 of
 * nr_render_lit hold word for word with these differences:
 *  1. G is what nr_compose_gbuffer(W, H, max_steps) returns for the owner's view and frame (status,
 *     position, normal, part); base is nr_compose_render's W x H frame (the owner's colouring and
 *     matcap).
 *  2. The field.  Wherever nr_render_lit evaluates sceneSDF(x, mlp(x)) -- s_q of rule 3, tstep of
 *     rule 4 -- this call evaluates the composed field at x (above): always NR_SCENE_TANH's value
 *     per part, the owner's frame number for 4-input networks; nr_set_scene on the owner is not read.
 *  3. The shadow ray.  o = p + n * shadow_bias, d = L is marched by the composed ray rule (Rays,
 *     above) with shadow_steps in the place of max_steps: the entry on the world bound, tnear =
 *     max(tnear, 0), tfar reduced by tnear, then per iteration tstep = field(p), rule 4's running
 *     minimum (dist = tnear + travel; if dist > 0, r = shadow_k * tstep / dist, res = r where r <
 *     res), then the composed step and end tests.  MISS gives 1.0f; ESCAPED shadow_k > 0 ? sat(res)
 *     : 1.0f; HIT and LIMIT 0.0f.
 *  4. occluder[i] = the part that blocked the light: the owner at the converging step of pixel i's
 *     shadow ray where that ray ends HIT, -1 for every other pixel (not a HIT pixel, no ray marched,
 *     a ray that ends MISS, ESCAPED or LIMIT).  part[i] is nr_compose_gbuffer's.
 *  5. With ao_strength = 0, shadow_steps = 0 and ambient = 1, out is nr_compose_render's frame, bit
 *     for bit.
 *  6. Settings.  The outputs depend only on the inputs: the same bits for any workgroup size, grid,
 *     occupancy (nr_set_occupancy on the owner) or order in which the pixels are dealt.
 *  7. Outputs.  out, ao, shadow, part and occluder (W H values each, index y * W + x) may each be
 *     NULL, but not all of out, ao and shadow; loc = NR_HOST or NR_DEVICE for all of them.  stats
 *     (may be NULL): ray_steps = the geometry buffer's plus the sum of the shadow rays' steps;
 *     rays_hit and rays_shaded the geometry buffer's; shade_evals = 4 per HIT, plus 4 per HIT with
 *     ambient occlusion on; part_evals = the (marching ray, part) pairs in bound of the primary and
 *     of the shadow rays; wave_evals and wave_skips summed over both launches (the occlusion passes
 *     count there, as the normal passes do); iterations = the larger of the primary and the shadow
 *     rays' longest; launches and ms_total as elsewhere.
 *  8. Errors.  NR_E_INVALID: c or light NULL, out, ao and shadow all NULL, W or H < 1, W H > 2^30,
 *     max_steps < 1, and nr_render_lit's checks of the light fields.  NR_E_STATE: matcap colouring
 *     without a matcap when out is wanted.
 *  9. Scratch.  The composition owns it and keeps it until nr_compose_destroy: 28 bytes per pixel of
 *     geometry buffer, 8 bytes per pixel (ao, shadow) where the caller gave none or gave host
 *     pointers (4 for one of the two), and for loc = NR_HOST 4 bytes per pixel for each of out, part
 *     and occluder that is wanted. */
int nr_compose_render_lit(nr_compose *c, uint32_t *out /*W*H or NULL*/, int W, int H, int max_steps,
                          const nr_light *light, float *ao /*W*H or NULL*/, float *shadow /*W*H or NULL*/,
                          int32_t *part /*W*H or NULL*/, int32_t *occluder /*W*H or NULL*/, int loc,
                          nr_compose_stats *stats);

/* ---- composed scenes: lattice sampling and mesh extraction ------------------------- */
/* (new symbols only: NR_ABI_VERSION stays 3, nr_stats and nr_compose_stats are unchanged)
 *
 * nr_sample_grid, nr_extract_mesh and nr_extract_mesh_sparse for a composition: the same lattice, the
 * same mesh rule, the composed field (above) in the place of sceneSDF(p, mlp(p)).
 *  1. Lattice.  nr_sample_grid's: index (k * ny + j) * nx + i, coordinate origin[a] + (float)idx_a *
 *     step[a] (one f32 multiply, then one f32 add), the points generated in the kernel.  The dense
 *     calls take at most 2^30 points; the sparse call dims 2..65,536 per axis, 64-bit indices and at
 *     most 2^30 bricks.
 *  2. Values.  Every value used is the composed field at a lattice point, with nr_compose_sample's
 *     bits for that point, value and owner, the frame being the owner context's.  A point's value
 *     depends only on that point: the same bits for any workgroup size, grid, occupancy or lattice that
 *     contains the point.  The field is a distance only near the parts: outside every part's bound it
 *     is the nearest bound's distance, scale * (sqrtf(qq) - 1.19f), and at a bound's edge (qq = 1.45)
 *     it is discontinuous -- a network's tanh inside, about 0.014 * scale outside.  A level iso above
 *     0.014 * scale therefore shows the bound spheres, not the models.
 *  3. Mesh.  nr_mesh_grid's mesh of those values at iso, bit for bit: vertices, numbering, triangles,
 *     windings, the capacity and counting protocol (rule 5 there) and the NaN rules.  iso is any finite
 *     value.
 *  4. Sparse.  Rules 2 and 4-6 of nr_extract_mesh_sparse word for word, with "the composed field" in
 *     the place of sceneSDF: the bricks, activity by band, one vertex per shared edge, keys, the fixed
 *     but unspecified order, the capacities.  What the band proves is less than for one network: the
 *     field's discontinuity at the bound edges is a step of up to about scale * (1 - 0.014), so a
 *     band below that can cull a brick whose corners all lie outside a bound the surface lies within;
 *     the default of the Python binding (the brick's diagonal) is sound only while bricks are small
 *     against the parts.
 *  5. Normals and part.  normals[v] = the normalised tetrahedral gradient of the composed field at
 *     vertices[v] (epsilon 1e-5): nr_compose_trace_rays' hit normal in the same arithmetic.  part[v] =
 *     the owner of the composed field at vertices[v], the value nr_compose_sample returns there.
 *     Each needs vertices; either may be NULL.
 *  6. Stats (may be NULL).  ray_steps = lattice points evaluated -- for the sparse call
 *     nr_extract_mesh_sparse's sum, the brick-corner lattice plus the active bricks' point sets;
 *     part_evals = (lattice point, part) pairs inside that part's bound over the sampling passes
 *     (not the vertex pass), independent of the grouping; rays_hit = active bricks (sparse) or 0
 *     (dense); rays_shaded = *nv; shade_evals = 4 * *nv with normals plus *nv with part; wave_evals
 *     and wave_skips as elsewhere (they depend on the grouping), over all passes; iterations = 0;
 *     launches (the zeroing of the statistics counts as one) and ms_total as elsewhere.
 *  7. Errors.  Those of the composed calls and of the mesh calls, the message through nr_last_error
 *     of the owner.  NR_E_INVALID: a NULL composition, origin, step, dims, nv or nt; nr_compose_sample_grid
 *     with value and owner both NULL or a dim < 1; a dim < 2 (dense mesh) or outside 2..65,536
 *     (sparse); more than 2^30 points (dense) or bricks (sparse); iso not finite; only one of
 *     vertices / triangles given; normals, part or keys without vertices; brick not 4, 8 or 16; band
 *     negative or NaN; more than 2^31 - 1 vertices.  NR_E_NOMEM: short capacities (nothing written),
 *     or scratch that cannot be allocated.
 *  8. Scratch.  The owner context's, the buffers nr_mesh_grid, nr_extract_mesh and
 *     nr_extract_mesh_sparse use on it, kept until nr_destroy; the owner needs no network.  Dense: 8
 *     bytes per lattice point (value, pass word) + 24 bytes per 256 points.  Sparse: per brick 4 bytes
 *     + 4 bytes per point of the brick-corner lattice + 24 bytes per 256 bricks; per active brick 4
 *     bytes + 8 bytes per active point ((B + 1)^3 rounded up to a multiple of 64: 128, 768 or 4,928)
 *     + 24 bytes per 256 active points.  For loc = NR_HOST also staging of the results' size.  The
 *     active-brick count is read on the host once, as in nr_extract_mesh_sparse.
 * All launches run on the owner's stream; the count, scan, emit and classify passes are those of the
 * single-network calls. */
int nr_compose_sample_grid(nr_compose *c, const float origin[3], const float step[3], const int dims[3],
                           float *value /*[nz][ny][nx] or NULL*/, int32_t *owner /*[nz][ny][nx] or NULL*/,
                           int loc, nr_compose_stats *stats);
int nr_compose_extract_mesh(nr_compose *c, const float origin[3], const float step[3], const int dims[3], float iso,
                            float *vertices /*[v_cap][3]*/, float *normals /*[v_cap][3] or NULL*/,
                            int32_t *part /*[v_cap] or NULL*/, long v_cap,
                            int32_t *triangles /*[t_cap][3]*/, long t_cap, long *nv, long *nt, int loc,
                            nr_compose_stats *stats);
int nr_compose_extract_mesh_sparse(nr_compose *c, const float origin[3], const float step[3], const int dims[3],
                                   float iso, int brick, float band,
                                   float *vertices /*[v_cap][3]*/, float *normals /*[v_cap][3] or NULL*/,
                                   int32_t *part /*[v_cap] or NULL*/, int64_t *keys /*[v_cap] or NULL*/, long v_cap,
                                   int32_t *triangles /*[t_cap][3]*/, long t_cap,
                                   long *nv, long *nt, long *active_bricks /*or NULL*/, int loc, nr_compose_stats *stats);

/* One DenseLayer::forward (denseLayer.cu:229-278) on device buffers: layer l of the
 * loaded network applied to A [n][dims[l]] -> Z [n][dims[l+1]]. */
int nr_layer_forward(nr_ctx *ctx, int layer, const float *A, float *Z, long n, int loc);

/* Stateless dense layer on device (or host) buffers: Z = act(W A + b) per row of A,
 * W out-major [out][in] (DenseLayer's layout, denseLayer.cu:217-227), act = ReLU if
 * relu != 0 else linear.  Runs on ctx's stream (DenseLayer::forward objects that are
 * not part of a loaded network). */
int nr_dense_forward(nr_ctx *ctx, const float *W, const float *b, int in, int out, int relu,
                     const float *A, float *Z, long n, int loc);

/* ---- measurement ------------------------------------------------------------ */
/* Per-launch HIP events around every kernel of nr_render* on the context's stream
 * (the stream those kernels run on).  nr_prof_collect() waits for the stream, sums
 * the recorded durations since the previous collect and resets them. */
typedef struct nr_kernel_prof {
    double march_ms;         /* sum over k_march launches */
    double shade_ms;         /* sum over k_shade launches */
    double init_ms;          /* sum over k_init launches */
    uint64_t march_launches, shade_launches, init_launches;
    uint64_t renders;        /* nr_render* calls covered */
} nr_kernel_prof;
int nr_set_profiling(nr_ctx *ctx, int on);
int nr_prof_collect(nr_ctx *ctx, nr_kernel_prof *out);
/* The pixel contract per schedule (round 6): fp32 frames are identical on all three schedules, and
 * so are bf16 / fp16 frames on the persistent and wavefront schedules, endgame included (the
 * wavefront schedule runs it as a second, fp32x3 queue per iteration); the layered schedule renders
 * fp32 whatever the precision.  tests/test_gpu_endgame.py test_schedule_pixel_contract asserts this. */
int nr_set_schedule(nr_ctx *ctx, int schedule);
/* Diagnostics: flags bit 0 = per-wave s_memrealtime stamps in k_trace
 * {start, pixel queue drained, end (100 MHz), (wave iterations after the drain << 32) |
 * wave iterations, shader-clock cycles spent in refill, shading, MLP, scene, step, and within
 * refill (bf16/fp16 tracers) in the queue reservation, bulk ray generation and dealing; after
 * the queue drained: cycles in refill + shading + step, MLP, scene, iterations with at most
 * 4 rays}; the stamps instance marches bf16/fp16 without the endgame (the pure 16-bit march);
 * nr_debug_stamps copies the last
 * frame's (16 u64 per wave, *n = waves).  Bit 3 = iteration map: the persistent
 * schedule writes each hit pixel's iteration count instead of its colour.  Bit 6 =
 * MLP latency probe: nr_mlp_forward(X >= 64 points, Y >= 65 floats, n = repetitions, on
 * the device) runs one wave of ceil(wave_rays / 16) tiles n times back to back and
 * writes the shader cycles per evaluation to Y[0]; bit 7 times it without the final
 * layer; for fp32, bit 13 in the clamped-ReLU form the tracers run (scaled pack) and bit 14 with
 * the hidden layers unrolled for 7 (the network must have 7).  Bit 8 = NR_SCHED_LAYERED issues its launches one by one instead of replaying
 * the captured hipGraph (for profilers that do not follow graph launches).  Bit 9 = the plain ReLU
 * forms on the scaled packs: bf16 by v_pk_max_i16 instead of the conversion's clamp bit,
 * fp32 by add + max instead of v_add_f32 with the clamp bit (the same values: parity and
 * A/B of the two forms); fp32x3 by the fp32 MLP for every wave (its fallback, bit-exact fp32).  Bit 10 = nr_render_batch deals its pixel queue frame after
 * frame instead of interleaving the frames in 64-pixel chunks (pixels are unaffected).  Bit 11 = the
 * bf16/fp16 MLP of 7-hidden-layer networks in its builtin-compiled form instead of the
 * software-pipelined instruction streams (nr_mlp16_asm.h; the same values, for A/B and parity).
 * Bit 12 = nr_mlp_forward's bf16/fp16 MLP (k_mlp16, 7 hidden layers) with the hidden layers on
 * v_mfma_f32_16x16x32 instead of 32x32x16 (round 6; the same values; 3-5 % slower for bf16 and
 * 4-12 % for fp16, profiles/r6_mlp_s16_ab.txt, so it is an A/B form, not the default).
 * Bit 15 = the bf16/fp16 tracers' normals (the four tetrahedron
 * samples of every coloured ray) by the fp32 MLP instead of the fp32x3 split (A/B; the frames'
 * march is the same, their shading moves by the two forms' rounding). */
int nr_set_debug(nr_ctx *ctx, int flags);
/* The reduced-precision endgame (bf16 / fp16, round 5): a marching ray whose
 * 16-bit MLP output falls below tau (a surface is near) re-evaluates that point in fp32x3 and
 * takes every later step of its march in fp32x3, so the convergence test (tstep < 1e-6,
 * volumeRender_kernel.cu:474), the background test and the hit point are decided at fp32-class
 * precision while the bulk of the march stays 16-bit.  Default NR_ENDGAME_DEFAULT; 0 = the pure
 * 16-bit march.  It needs the network's fp32x3 pack (a [3|4, 32..., 1] network whose pack
 * nr_pack_x3 accepts, as for the fp32x3 normals): a network whose pack is refused marches in pure
 * 16 bits whatever tau is, takes its normals from the fp32 MLP and reports endgame_evals = 0.  It
 * is off with nr_set_debug bit 15 (fp32 normals) too; the
 * wavefront schedule applies it too (round 6: a fine queue per iteration, the same frames), the
 * layered schedule renders fp32.  nr_stats.endgame_evals counts the fp32x3
 * evaluations, nr_stats.endgame_switches the rays handed over.  The default (round 6, DESIGN.md
 * section 2): the threshold that meets the fixed quality targets of tests/test_gpu_lowp_contract.py
 * against the exact-MLP frame (C3 identical >= 0.77, C4 >= 0.88 with mean |delta| <= 5.0, coverage
 * IoU >= 0.99 / 0.98): 1e-3 (round 5's 3e-4 left C4's mean |delta| at 6.4). */
#define NR_ENDGAME_DEFAULT 0.001f
int nr_set_endgame(nr_ctx *ctx, float tau);
/* The batched fp32 tracer (nr_render_batch at NR_PRECISION_FP32) skips the matrix-core k-steps of
 * hidden units that never fire in the marched volume, checked per wave at run time: a wave that
 * sees one fire evaluates again on the full pack, so frames and statistics are the same in every
 * mode, bit for bit.  mode 0: no unit is a candidate (the A/B arm); 1 (default): candidates chosen
 * when the network is loaded, from firing counts over a fixed sample (3-input networks with
 * finite weights whose scaled pack is accepted; others have none); 2 (tests): the four
 * highest-numbered units of every hidden layer, whatever they do, so that the redo runs
 * constantly.  nr_prune_info: the loaded network's ReLU layers (*nrelu; 0: no pruned pack) and,
 * when cap_layers >= *nrelu, the candidates per layer, the k-steps and the order [nrelu][32]
 * (position -> unit).  nr_prune_redos: wave evaluations redone by the last nr_render_batch. */
int nr_set_prune(nr_ctx *ctx, int mode);
int nr_prune_info(const nr_ctx *ctx, int *nrelu, int *cand, int *ks, int *order, int cap_layers);
int nr_prune_redos(nr_ctx *ctx, unsigned long long *redos);

/* The batched fp32 tracer (nr_render_batch), one matrix instruction per hidden unit (added after
 * 3.0; NR_ABI_VERSION stays 3): a unit whose activation is +0 at every point a wave holds is not
 * issued -- the images and statistics are the same bit for bit.  on (the default): this form runs
 * while the prune mode is 1; nr_set_prune 0 and 2, and on = 0, run the paths they ran before.
 * Networks whose scaled pack is refused, or with a non-finite weight or a bias of -0, never take
 * it.  nr_unit_skip_counts, for the last nr_render_batch: *issued = the unit instructions its
 * waves came to (one per input unit of layer 0 and of every hidden layer, for one wave of 64
 * points), *skipped = those of them that were not executed, so skipped <= issued and
 * issued - skipped ran on the matrix core (unit 0 of a hidden layer always does; both 0 when the
 * form did not run).
 * nr_pack_fp32_units (host only): the pack that form reads (layout: nr_internal.h), *has_pack = 0
 * and *len = 0 when it is refused. */
int nr_set_unit_skip(nr_ctx *ctx, int on);
int nr_unit_skip_counts(nr_ctx *ctx, unsigned long long *issued, unsigned long long *skipped);
int nr_pack_fp32_units(int nlayers, const int *dims, const float *const *kernels, const float *const *biases,
                       float *pack, long cap, long *len, int *has_pack);
/* Temporal scheduling: each launch (a frame, or a batch's launch of up to 32 frames)
 * records its 8x8 pixel blocks' longest ray (the max over the batch's frames) and the next
 * launch of the same size/shard dispenses blocks longest-first (pixels are unaffected --
 * only the order work is handed out changes).  on = 2: each block's cost is the max over its
 * 3x3 neighbourhood (for a moving camera, whose silhouettes shift between frames). */
int nr_set_temporal_order(nr_ctx *ctx, int on);
/* Persistent-schedule grid: blocks of 4 waves per CU (0 = default).  A bf16/fp16 launch with the
 * endgame on runs one 12-wave workgroup per CU (3 blocks' worth, with the fp32x3 weights in its LDS;
 * networks of more than 9 hidden layers: at most 3 blocks of 4 waves), whatever is set here. */
int nr_set_occupancy(nr_ctx *ctx, int blocks_per_cu);
/* Rays per wave (persistent schedule, 1-64; 0 = automatic, the default): a wave marches at
 * most this many rays at once (in lanes 0..rays-1), so 16 or 32 make every iteration one or
 * two 16-ray tiles -- shorter per-iteration latency for small frames or shards, where the
 * longest ray rather than the matrix-core throughput sets the frame time.  Automatic: 64, or
 * 32 for an fp32 launch whose pixels fill at most 2x its waves' 64-ray slots (a frame on 4 or
 * 8 shards). */
int nr_set_wave_rays(nr_ctx *ctx, int rays);
/* Pixel-queue shards (persistent schedule; power of two <= 64, default 8): the queue's
 * atomic counters, each on its own 128-byte line, that the waves take pixels from. */
int nr_set_queue_shards(nr_ctx *ctx, int n);
/* NR_SCHED_LAYERED: points per dense-layer launch (the activations of one chunk are the
 * layer scratch: 2 x points x widest hidden layer x 4 B).  0 = auto (128 MiB per buffer).
 * The reference sizes Z for the whole batch, W*H*4 points (volumeRender_kernel.cu:659-661). */
int nr_set_layer_chunk(nr_ctx *ctx, long points);
/* Pixel spread (persistent schedule): the pixel queue deals each group of
 * `group_blocks` 8x8 blocks pixel-major -- one refill takes one pixel from each of up
 * to 64 blocks -- so the rays of one slow block are spread over many waves (0 =
 * block-major; -1 = automatic, the default: 16 for launches of fewer than 4 frames and
 * for fp32 batches of under 8 M pixels in all, 0 for the other nr_render_batch launches).
 * Pixels are unaffected. */
int nr_set_pixel_spread(nr_ctx *ctx, int group_blocks);
/* Cost probe (persistent schedule): before each frame, march the centre ray of every
 * 8x8 block for at most `max_steps` iterations (`rays_per_wave` rays per wave, so the
 * probe runs at short per-iteration latency), then hand the blocks out in decreasing
 * order of their probe's iteration count, so the frame's longest rays start first
 * (max_steps 0 = off; a valid temporal order takes precedence).  Pixels are unaffected. */
int nr_set_cost_probe(nr_ctx *ctx, int max_steps, int rays_per_wave);
int nr_debug_stamps(nr_ctx *ctx, unsigned long long *out, size_t cap, size_t *n);
/* Host polls the live-ray count every `every` iterations to stop early (0 = never). */
int nr_set_poll_interval(nr_ctx *ctx, int every);

/* ---- host helpers (the reference's main.cpp / image.cu side) -------------- */
/* updateViewMatrices (main.cpp:207-222): M = Rx(-rx deg) * Ry(-ry deg), then
 * translate(-(tx, ty, -zoom)); inv_view = rows 0..2 of M, normal = M^-1. */
int nr_camera(float rx_deg, float ry_deg, float zoom, float tx, float ty,
              float inv_view[12], float normal[16]);
/* The same with a choice of arithmetic.  NR_CAMERA_F64 (nr_camera's): the rotation and its
 * exact transpose-inverse in double, rounded once to float.  NR_CAMERA_EIGEN: main.cpp's float
 * Eigen expression restated step by step -- AngleAxisf * AngleAxisf as a quaternion product,
 * toRotationMatrix, Affine3f rotate/translate, Matrix4f::inverse by cofactors (Eigen 3.3's scalar
 * paths; Eigen is not available to pin it, and an SSE build inverts 4x4 floats differently). */
#define NR_CAMERA_F64 0
#define NR_CAMERA_EIGEN 1
int nr_camera_ex(float rx_deg, float ry_deg, float zoom, float tx, float ty, int mode,
                 float inv_view[12], float normal[16]);
/* Minimal HDF5 (superblock v0, symbol-table groups, contiguous datasets) Keras
 * reader.  Call with kernels/biases NULL to query sizes. */
int nr_h5_read_keras(const char *path, int max_layers, int *nlayers, int *dims,
                     float *params /* per layer: kernel (in x out) then bias, or NULL */,
                     size_t params_cap);
/* HDF5 object tree: the calls HighFive makes for NeuralNetwork::load (neuralNetwork.cpp:86-129)
 * and simpleInfer's loadModelFromH5 (simpleInfer.cpp:13-79) -- File(fp, ReadOnly),
 * listObjectNames, getObjectType, getGroup, getNumberObjects, getDataSet, getDimensions,
 * read -- over the same minimal reader; the headers in include/highfive/ wrap them in HighFive's
 * class names.  Objects are identified by their object-header addresses; group members
 * come in HDF5 name order (what HighFive's listObjectNames returns). */
typedef struct nr_h5_file nr_h5_file;
#define NR_H5_OTHER 0
#define NR_H5_GROUP 1
#define NR_H5_DATASET 2
int nr_h5_open(const char *path, nr_h5_file **out);
void nr_h5_close(nr_h5_file *f);
int nr_h5_root(const nr_h5_file *f, uint64_t *obj);
int nr_h5_object_type(nr_h5_file *f, uint64_t obj, int *type);
int nr_h5_num_members(nr_h5_file *f, uint64_t group, size_t *n);
/* member i of a group: name (NUL-terminated, cap bytes; NULL to query *name_len) and id */
int nr_h5_member(nr_h5_file *f, uint64_t group, size_t i, char *name, size_t cap, size_t *name_len,
                 uint64_t *obj);
/* dims may be NULL to query *ndims */
int nr_h5_dims(nr_h5_file *f, uint64_t dataset, uint64_t *dims, int cap, int *ndims);
/* all elements, row-major, converted to float; count must equal the element count */
int nr_h5_read_f32(nr_h5_file *f, uint64_t dataset, float *out, size_t count);
/* PNG decode to packed RGBA (image.cu:36-65 packing).  *rgba is malloc'ed; free
 * with nr_free(). */
int nr_png_load(const char *path, uint32_t **rgba, int *w, int *h);
/* Image::savePNG (image.cu:67-110): flip=1 reproduces the reference's 180 deg
 * rotation (quirk Q9). */
int nr_png_save(const char *path, const uint32_t *rgba, int w, int h, int flip);
/* sdkSavePPM4ub-style P6 (helper_image.h:310-328), buffer row 0 first. */
int nr_ppm_save(const char *path, const uint32_t *rgba, int w, int h);
void nr_free(void *p);

#ifdef __cplusplus
}
#endif
#endif /* NEURAL_RENDER_H */
