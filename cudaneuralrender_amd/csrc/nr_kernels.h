// nr_kernels.h -- kernel argument blocks and launchers (nr_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Workgroups per CU the persistent tracer's endgame instances (bf16/fp16 with nr_set_endgame) are
// built for: their registers (161 VGPRs) and the fine queue's LDS leave room for this many, so the
// host caps their grid at it (nr_api_render.hip trace_bpc; a larger grid would queue workgroups behind the
// resident ones)
#ifndef NR_TRACE_BPC_EG
#define NR_TRACE_BPC_EG 3
#endif
// Waves per workgroup of the endgame instances (round 6): 12 -- one workgroup per CU, the same 3
// waves per SIMD -- so that one LDS copy of the fp32x3 pack (~31 KB, read by the fine passes and
// the normals) fits beside the 16-bit pack and the 12 waves' queues; 4 = round 5's form (three
// 4-wave workgroups per CU, the fp32x3 weights read from global memory / L2)
#ifndef NR_EG_WAVES
#define NR_EG_WAVES 12
#endif
// LDS per CU on gfx950 (MI355X_MICROARCH.md): one workgroup's static + dynamic LDS must fit
constexpr int NR_LDS_PER_CU = 160 * 1024;

namespace nr {

// Network packs resident in device memory, staged into LDS by every block.
struct MlpArgs {
    const float *pk;        // fp32 pack (nr_internal.h PK_*; 32- or 16-wide layout)
    const uint16_t *lp;     // bf16/fp16 A operands (precision != fp32)
    const float *lpf;       // float side of the low-precision pack
    int pk_bytes, lp_bytes, lpf_bytes;
    int in0, nh;
    int lp_clamp;           // bf16 pack scaled for the clamped ReLU (nr_pack.cpp): valid for
                            // inputs within LP_INPUT_BOUND; the launch clears it otherwise
    int f32_clamp;          // fp32 pack scaled for the clamped ReLU (pack_fp32_16): used by the
                            // waves whose inputs are all within F32_INPUT_BOUND
    int lp_stream;          // 16-bit MLP as the pipelined streams of nr_mlp16_asm.h (7 hidden
                            // layers); 0 (nr_set_debug bit 11): the builtin form, same values
    const uint16_t *x3lp;   // bf16/fp16 tracers: the fp32x3 pack (global memory), for their normals
    const float *x3fl;
    int x3n;                // bf16/fp16: 1 = the normals (4 MLP evaluations per coloured ray) in fp32x3
                            // (mlp16_x3_normal), 0 = in fp32
    const uint16_t *lps;    // bf16/fp16, 7 hidden layers: the 16x16x32 layout of lp / lpf for k_mlp16
    const float *lpfs;      // (nr_pack.cpp pack_lowp_s16; null: not built, or nr_set_debug bit 12 clear)
    int lp_s16;             // k_mlp16 only (launch_mlp16): lp / lpf ARE the 16x16x32 layout, every
                            // chunk takes the NR_S16_* stream
    const float *pkp;       // the batched fp32 k_trace: the pruned fp32 pack (nr_internal.h PruneInfo), which
                            // it stages in LDS instead of pk; null: none (the scaled pack was refused, or
                            // f32_clamp is off) -- it then stages pk and runs the add + max form
    unsigned long long ks_bits;  // pkp: k-steps per ReLU layer, ks[l] - 4 in bits [3l, 3l + 3)
    const float *pku;       // the batched fp32 k_trace: the unit pack (nr_internal.h pack_fp32_units), which it
                            // stages in LDS instead of pkp / pk for the one-MFMA-per-unit form
                            // (nr_mlp16.h mlp64_fp32_units); null: off (nr_set_unit_skip, nr_set_prune 0 or 2),
                            // or the pack was refused
};

// Per-render constants (the reference's __constant__ state, volumeRender_kernel.cu:31-35,
// passed by value so contexts are independent).
struct RenderArgs {
    uint32_t *out;          // this shard's rows, W per row
    int W, H, rows, band, nshards, shard;
    int max_steps, scene, frame, color_type;
    const uint32_t *matcap;
    int mw, mh;
    float inv_view[12];
    float normal[16];
    double inv_w, inv_band;  // 1/W, 1/band for udiv_r (set_recips)
    // 1/W, 1/H where W (H) is a power of two, else 0: initMarcher's (float)x / (float)W is then
    // (float)x * (1/W) exactly (a power-of-two divisor only shifts the exponent), which saves
    // ray generation two correctly rounded divisions (set_recips; pixel_uv)
    float rcp_w, rcp_h;
};
inline float pow2_rcp(int n) { return n > 0 && (n & (n - 1)) == 0 ? 1.0f / (float)n : 0.0f; }
inline void set_recips(RenderArgs &A) {
    A.inv_w = 1.0 / (double)A.W;
    A.inv_band = 1.0 / (double)A.band;
    A.rcp_w = pow2_rcp(A.W);
    A.rcp_h = pow2_rcp(A.H);
}

// Ray queues: live rays {p.xyz, tfar} + {d.xyz, pixel}; converged rays {p.xyz, -} + {d.xyz, pixel}.
struct QueueArgs {
    const uint32_t *cnt_in;
    uint32_t *cnt_out;
    const float4 *p_in, *d_in;
    float4 *p_out, *d_out;
    uint32_t *shade_cnt;
    float4 *shade_p, *shade_d;
    uint32_t *shade_it;     // per-iteration count of waves that enqueued converged rays
    long seg_cap;           // segmented queues (wavefront schedule): WF_SEGS segments of
                            // seg_cap entries, one counter each (cnt_*[s], shade_cnt[s])
    // the endgame on the wavefront schedule (round 6; bf16/fp16): the coarse pass appends the rays
    // whose 16-bit SDF falls below eg_tau, unstepped, to this iteration's fine queue (fcnt, fp, fd;
    // segmented like the live queue) and counts them in *fsw
    uint32_t *fcnt;
    float4 *fp, *fd;
    uint32_t *fsw;
    float eg_tau;
};
constexpr int WF_SEGS = 8;

// One dense layer over a chunk of points (k_dense; layered schedule and the generic
// nr_mlp_forward).  Z is chunk-local [chunk][out].
struct DenseArgs {
    const float *W, *b;        // out-major [out][in], bias [out]
    const float *A;            // SRC 0: chunk-local rows [chunk][in]
    float *Z;
    const float4 *pts;         // SRC 1: live-ray queue; SRC 2: converged-ray queue
    const uint32_t *count;     // device-side point count (x count_mul), or NULL: use n
    const RenderArgs *args;    // SRC 1/2: the frame number (4th input)
    long n, chunk0, chunk_n;
    int count_mul, in, out, relu, lds;
};

// Persistent-schedule state (nr_trace.hip).
// One frame of a batched launch (nr_render_batch): its camera, sphere-grid offset,
// animation input and output image.  Staged into LDS by k_trace<.., BATCH>.
struct FrameArgs {
    float inv_view[12];
    float normal[16];
    double zoff;        // sphere_zoff(frame)
    uint32_t *out;
    float frame_f;      // the network's 4th input when it takes one
    int frame;
};
constexpr int NR_MAX_BATCH = 32;


struct TraceArgs {
    uint32_t *pix_ctr;          // 2^nq_shift pixel-queue shard counters, one per 128-byte line (stride 32)
    int nq_shift;
    unsigned long long *stats;  // [0] ray-steps, [1] rays hit, [2] max iterations, [3] rays shaded,
                                // [4] fp32x3 march evaluations (the endgame), [5] rays handed to it,
                                // [6] wave evaluations redone on the full fp32 pack (MlpArgs::pkp),
                                // [7] unit instructions skipped, [8] wave evaluations of the unit form
                                // (MlpArgs::pku)
    unsigned long long *stamps; // diagnostics (nr_set_debug): per wave {start, queue drained, end, ray-steps}
    // pixel queue over 8x8 pixel blocks of the shard image, dispensed in `order`
    // (NULL = raster order); bcost (may be NULL) receives each block's max ray iterations
    const uint32_t *order;
    uint32_t *bcost;
    int bw, nblocks;            // blocks per row, blocks in the shard image
    // pixel spread: the queue deals a group of 2^spread_shift blocks pixel-major (a refill
    // takes one pixel from each of 64 blocks), so a block of long rays is marched by 64
    // different waves instead of one (0/1 = block-major)
    int spread_shift;           // log2 of the spread group (0 = block-major)
    int itmap;                  // diagnostics: write each pixel's iteration count instead of its colour
    double inv_bw, inv_band;    // 1/bw, 1/band for udiv_r
    // cost probe (k_trace<.., true>): one ray per block
    int probe, take;
    uint64_t lane_cap;          // lanes a wave may fill: (1 << take) - 1, all 64 for take = 64
    const FrameArgs *frames;    // batched launch: nframes frames (k_trace<.., BATCH>)
    int nframes;
    int interleave;             // batched: 64-position queue chunks dealt to the frames in turn
                                // (all frames progress together) instead of frame-major
    double inv_nframes;         // 1 / nframes for udiv_r
    float eg_tau;               // bf16/fp16 with an fp32x3 pack: the endgame's switch threshold (0 = off;
                                // k_trace's EG instances, nr_set_endgame)
    int x3lp_bytes, x3fl_bytes; // sizes of the fp32x3 pack (16-byte multiples): the endgame
                                // instances stage it in LDS beside the 16-bit pack (NR_EG_WAVES)
};

// Ray queries (nr_query.hip; nr_trace_rays, nr_render_gbuffer): n rays, each writing its own slot
// of the outputs that are not NULL.
struct QueryArgs {
    const float *origins, *dirs;  // [n][3]; both NULL: the pixel rays of the W x H view below
    long n;                       // <= 2^30
    int W, H;
    double inv_w;                 // 1/W for udiv_r
    float rcp_w, rcp_h;           // pow2_rcp(W), pow2_rcp(H) (pixel_uv)
    float inv_view[12];
    int max_steps, scene, frame;
    int32_t *status, *steps;      // NR_RAY_*, iterations taken
    float *t, *position, *normal; // [n], [n][3], [n][3]; normal NULL: no tetrahedron evaluations
    uint32_t *cursor;             // next ray to deal (zeroed before the launch)
    unsigned long long *stats;    // [0] ray-steps, [1] rays that entered the sphere, [2] max steps, [3] hits
};

// Adaptive antialiasing (nr_aa.hip; nr_render_aa): the W x H base frame in out, its edge pixels'
// indices in list[0 .. *count) and one accumulator per list entry.
struct AaArgs {
    uint32_t *out;                // [H][W]: the base frame, resolved in place
    int W, H, S;                  // S x S samples per edge pixel, S W * S H <= 2^30
    int per;                      // S S - 1: the samples the tracer adds to sample (0, 0)
    int contrast, full;           // the edge rule's threshold; full: every pixel is an edge
    double inv_w, inv_s, inv_per; // 1/W, 1/S, 1/per for udiv_r
    double inv_nedge;             // 1/nedge
    uint32_t *list;               // [W H]: edge pixels y W + x, in the order the appends landed
    uint32_t *count;              // their number (zeroed before k_aa_detect)
    uint32_t nedge, nsub;         // *count and *count x per once the host has read it
    unsigned long long *accum;    // [nedge]: r, g, b, a sums in four 16-bit fields (zeroed before k_aa_trace)
    uint32_t *cursor;             // next sample to deal (zeroed before the launch)
    int take;                     // lanes a wave of k_aa_trace fills, 16..64
    unsigned long long *stats;    // [0] ray-steps, [1] rays that entered the sphere, [2] max iterations, [3] coloured
};

// Lighting (nr_light.hip; nr_render_lit): the W x H geometry buffer k_query<true> left in status /
// position / normal, the light, and one ao and one shadow value per pixel.
struct LightArgs {
    long n;                       // W H <= 2^30
    int scene, frame;
    const int32_t *status;        // [n] NR_RAY_*
    const float *position, *normal;  // [n][3], of the hits
    float dir[3];                 // nr_light, field by field
    int shadow_steps;
    float shadow_bias, shadow_k, ao_step, ao_strength, ambient;
    float *ao, *shadow;           // [n], both always written by k_light_trace
    uint32_t *cursor;             // next pixel to deal (zeroed before the launch)
    unsigned long long *stats;    // [0] shadow-ray steps, [1] the longest shadow ray's
};

// The lattice of nr_sample_grid / nr_mesh_grid / nr_extract_mesh: point (i, j, k) has linear index
// (k ny + j) nx + i and coordinates origin[a] + (float)idx_a * step[a] (one f32 multiply, one add).
struct LatticeArgs {
    float origin[3], step[3];
    int nx, ny, nz;
    long n;                       // nx ny nz <= 2^30
    double inv_nx, inv_nxy;       // 1/nx, 1/(nx ny) for udiv_r
};
inline LatticeArgs make_lattice(const float *origin, const float *step, const int *dims) {
    LatticeArgs L{};
    for (int a = 0; a < 3; ++a) { L.origin[a] = origin[a]; L.step[a] = step[a]; }
    L.nx = dims[0]; L.ny = dims[1]; L.nz = dims[2];
    L.n = (long)dims[0] * dims[1] * dims[2];
    L.inv_nx = 1.0 / (double)L.nx;
    L.inv_nxy = 1.0 / ((double)L.nx * (double)L.ny);
    return L;
}

// Volume sampling (nr_mesh.hip k_grid): sdf[idx] = sceneSDF(p, mlp(p)) over the lattice.
struct GridArgs {
    LatticeArgs L;
    int scene, frame;
    float *sdf;                   // [n]
};

// Isosurface extraction (nr_mesh.hip k_mesh_count / k_mesh_scan / k_mesh_emit) over 256-point
// blocks of the lattice's linear index.
struct MeshArgs {
    LatticeArgs L;
    const float *sdf;             // [n]
    float iso;
    int nblk;                     // ceil(n / 256)
    uint32_t *word;               // [n]: bits 0-6 the point's vertex mask (edge slots), 7-17 the vertices
                                  // and 18-29 the triangles of its block before it
    uint32_t *cnt;                // [2][nblk]: vertices, triangles of each block
    unsigned long long *off;      // [2][nblk]: their exclusive scans
    unsigned long long *total;    // [2]: vertices, triangles
    float *vertices;              // [nv][3]
    int32_t *triangles;           // [nt][3]
};

// Vertex normals (nr_mesh.hip k_vnormal): the normalised tetrahedral gradient at each vertex.
struct VNormalArgs {
    const float *vertices;        // [nv][3]
    float *normals;               // [nv][3]
    long nv;
    int scene, frame;
};

// Analytic gradient (nr_grad.hip k_grad): every point writes its slot of the outputs that are not NULL.
struct GradArgs {
    const float *X;               // [n][in0]
    long n;                       // <= 2^30
    float *value, *grad, *normal; // [n], [n][in0], [n][3]
    const float *gb;              // the backward pack (nr_internal.h pack_grad_16), staged after the fp32 pack
    int gb_bytes;
};

// Fitting (nr_fit.hip; nr_fit_*).  k_fit_grad: the weight gradients' partial sums of n points;
// k_fit_update: their totals, then the gradient written out, or Adam and the packs rewritten.
struct FitArgs {
    const float *X, *Y;           // [n][3], [n]
    long n;                       // 1 .. 2^30
    const float *pack;            // the fit pack (nr_internal.h fit_pack_floats)
    float *partial;               // [S][P + 1]: partial s's sums in flat parameter order, then SS
    float *value;                 // [n] or NULL
    float clamp;                  // > 0: the clamped residual
    int S, nh;
};
enum { FIT_MODE_GRADIENT = 0, FIT_MODE_ADAM = 1, FIT_MODE_PACK = 2 };
struct FitUpdArgs {
    const float *partial;         // as FitArgs
    int S, nh, mode;
    float inv_n;
    float *theta, *m, *v;         // [P] master weights and Adam's moments
    float *pack;                  // the fit pack (ADAM, PACK: rewritten from theta)
    float a_t, beta1, beta2, omb1, omb2, eps;
    float *grad, *loss;           // GRADIENT: [P] or NULL; GRADIENT, ADAM: [1] or NULL
};

// Projection onto a level set (nr_project.hip k_project; nr_project_points): every point writes its
// slot of the outputs that are not NULL.
struct ProjArgs {
    const float *X;               // [n][in0]
    long n;                       // <= 2^30
    float iso, tol, max_step;     // nr_project_opts, field by field
    int max_iters;
    float *position, *value, *normal, *distance;  // [n][3], [n], [n][3], [n]
    int32_t *iters, *status;      // [n]: steps taken, NR_PROJ_*
    const float *gb;              // the backward pack, staged after the fp32 pack (as GradArgs)
    int gb_bytes;
    int compact;                  // pack the live slots into the lowest tiles once the cursor is past n
    uint32_t *cursor;             // next point to deal (zeroed before the launch)
    unsigned long long *stats;    // [0] evaluations, [1] converged points, [2] the largest evaluation count
};

// Signed distance to a triangle mesh (nr_trimesh.hip k_trimesh_distance; nr_trimesh_distance): every
// point writes its slot of the outputs that are not NULL.  nodes / tris: nr_internal.h TriBvh.
struct TriMeshArgs {
    const float *X;               // [n][3]
    long n;                       // 1 .. 2^30
    const float *nodes, *tris;    // [nnodes][8], [ntl][12]
    const float *table;           // [nt][7][3] pseudonormals, original triangle order
    int nnodes, ntl;
    int brute;                    // every triangle of tris in order, no hierarchy
    float *sdf, *closest;         // [n], [n][3]
    int32_t *tri, *feature;       // [n]
    unsigned long long *stats;    // [0] point-triangle evaluations (zeroed before the launch)
};
hipError_t launch_trimesh_distance(const TriMeshArgs &A, int grid, hipStream_t st);  // 4-wave workgroups

// The generalized winding number of a triangle mesh (nr_winding.hip k_trimesh_winding;
// nr_mesh_winding): every point writes its slot of the outputs that are not NULL.
struct TriWindArgs {
    const float *X;               // [n][3]
    long n;                       // 1 .. 2^30
    const float *nodes, *tris;    // [nnodes][8], [ntl][12]
    const float *moments;         // [nnodes][16]
    int nnodes, ntl;
    int brute;                    // every triangle of tris in order, no expansion
    float beta;                   // a node is far iff |centre - p|^2 > beta^2 R2
    float *winding;               // [n]
    float *sdf;                   // [n]: k_trimesh_distance's result on entry, signed by the winding number on exit
    unsigned long long *stats;    // [0] += solid angles and expansions evaluated (not zeroed here)
};
hipError_t launch_trimesh_winding(const TriWindArgs &A, int grid, hipStream_t st);  // 4-wave workgroups

// Rays against a triangle mesh (nr_mesh_rays.hip k_mesh_rays; nr_mesh_trace_rays, nr_mesh_gbuffer,
// nr_mesh_render): every ray writes its slot of the outputs that are not NULL.  A chunk of 64 rays
// is 64 consecutive caller rays, or with origins == NULL one 8 x 8 tile of the W x H view.
struct MeshRayArgs {
    const float *origins, *dirs;  // [n][3]; both NULL: the pixel rays of the W x H view below
    long n;                       // 1 .. 2^30 (W H for pixel rays)
    int W, H, tiles_x, tiles_y;   // pixel rays: the view and its 8 x 8 tiles
    float rcp_w, rcp_h;           // pow2_rcp(W), pow2_rcp(H) (pixel_uv)
    float inv_view[12];
    const float *nodes, *tris;    // [nnodes][8], [ntl][12]
    const float *table;           // [nt][7][3] pseudonormals, original triangle order
    int nnodes, ntl;
    int brute, any, smooth;       // NR_TRIMESH_BRUTE, NR_MESH_RAY_ANY, NR_MESH_RAY_SMOOTH
    float tmin, tmax;
    float scale;                  // S of the per-ray pad: 2^18 times the slack of the boxes
    int32_t *status, *tri;        // [n]
    float *t, *bary, *position, *normal;  // [n], [n][3] x 3
    unsigned long long *stats;    // [0] ray-triangle evaluations, [1] hits (zeroed before the launch)
};
// 4-wave workgroups; with `color` the frame A.out of shade_color (A: render_args, the view and the
// normal matrix) instead of the hit record
hipError_t launch_mesh_rays(const MeshRayArgs &R, const RenderArgs *color, int grid, hipStream_t st);

// Fitting samples of a triangle mesh (nr_sample.hip k_mesh_sample; nr_mesh_sample): sample i < n_surface
// lies on the surface, the rest in the box; every sample writes its slot of the outputs that are not NULL.
struct SampleArgs {
    unsigned long long seed;
    long n_surface, n;            // n = n_surface + n_volume, 1 .. 2^27
    float sigma;
    float lo[3], ext[3];          // the box: lo, hi - lo
    const float *tris;            // [ntl][12]
    const uint32_t *thresholds;   // [ntl] (nr_internal.h trimesh_area_table)
    int ntl, last;
    float *points;                // [n][3]
    int32_t *tri;                 // [n] or NULL
    float *bary;                  // [n][3] or NULL
};
hipError_t launch_mesh_sample(const SampleArgs &A, int grid, hipStream_t st);  // 256-thread workgroups

// The stable order of n 32-bit keys (nr_sort.hip; nr_points_order): k_sort_keys writes the keys and the
// indices 0..n-1 into (keys[0], vals[0]); four passes of k_sort_hist, k_sort_scan, k_sort_scatter move
// them 0 -> 1 -> 0 -> 1 -> 0, the last pass writing its indices to perm.  Every dependency between
// workgroups is a kernel boundary.
constexpr int SORT_TILE = 2048;       // keys per workgroup of k_sort_hist / k_sort_scatter
constexpr int SORT_SCAN_STEP = 4096;  // table entries per step of k_sort_scan
struct SortArgs {
    const float *X;               // [n][3], MORTON
    long n;                       // 1 .. 2^27
    int mode;                     // NR_ORDER_MORTON | NR_ORDER_SHUFFLE
    float lo[3], inv[3];          // MORTON: the box' corner, 1023.0f / (hi - lo)
    unsigned long long seed;      // SHUFFLE
    uint32_t *keys[2], *vals[2];  // [n] each
    uint32_t *table;              // [256][nblk], digit-major: counts, then their exclusive scan
    int nblk;                     // ceil(n / SORT_TILE)
    int32_t *perm;                // [n]
};
inline size_t sort_scratch_words(size_t n) { return 4 * n + 256 * ((n + SORT_TILE - 1) / SORT_TILE); }
hipError_t launch_points_order(const SortArgs &A, hipStream_t st);  // 13 launches
constexpr int SORT_LAUNCHES = 13;
// The four passes alone, for any n 32-bit keys with a 32-bit payload already in (keys[0], vals[0]):
// the sorted keys end in keys[0], the payloads in vals_out, or in vals[0] where vals_out is NULL
// (nr_trimesh_build.hip sorts triangles and corners with it).  12 launches.
hipError_t launch_sort_pairs(uint32_t *const keys[2], uint32_t *const vals[2], long n, uint32_t *table, int nblk,
                             uint32_t *vals_out, hipStream_t st);
constexpr int SORT_PAIR_LAUNCHES = 12;
// dst[j] = src[perm[j]] of float3 rows, and col_dst[j] = col_src[perm[j]] where col_dst is not NULL
hipError_t launch_gather(const float *src, const float *col_src, const int32_t *perm, long n, float *dst, float *col_dst,
                         hipStream_t st);

// The device build of a nr_trimesh (nr_trimesh_build.hip; nr_mesh_create_device): the table, the
// order, the tree with its moments and the area table from vertices and triangles in device memory,
// by the contract of a device-built mesh in include/neural_render.h.  TriBuildHead is the only thing
// the host reads back: once after launch_tribuild_scan (err, the bound, ntl), once at the end.
struct TriBuildHead {             // 128 bytes
    uint32_t lo[3], hi[3];        // the vertices' bound, each float as an ordered integer: a negative
                                  // float's bits inverted, any other's with the top bit set (-0 < +0)
    uint32_t maxabs;              // the bits of the largest |coordinate|
    uint32_t err;                 // bit 0: an index outside 0..nv-1; bit 1: a vertex that is not finite
    uint32_t ntl;                 // the live triangles
    uint32_t open;                // != 0: some edge is not used exactly twice, once each way
    int32_t area_last;            // L of the area table
    uint32_t pad[21];
};
struct TriBuildArgs {
    const float *V;               // [nv][3]
    const int32_t *T;             // [nt][3]
    long nv, nt;
    TriBuildHead *head;
    uint32_t *tkeys[2], *tvals[2], *ttable;  // the triangle sort: [nt] each, the digit table; order = tvals[0]
    uint32_t *ckeys[2], *cvals[2], *ctable;  // the corner sort: [3 nt] each; after it [1] hold rank and group head
    double *fn;                   // [nt][3] the f64 face normals
    float *table;                 // [nt][7][3]
    // from here on: set after the first read-back
    double slack;
    int ntl, nnodes, nleaves, depth;
    const int32_t *w3, *w7, *first, *count;  // [nnodes] the tree's shape (host-made)
    const int32_t *list;          // [nnodes] the leaves, then the inner nodes level by level, deepest first
    const int *level_off;         // host: [ninner_levels + 1] offsets into list after the leaves
    int ninner_levels;
    double *sums;                 // [nnodes][19] sa, sx, mx, N, P
    float *box;                   // [nnodes][6] the exact bound of the node's corners
    unsigned long long *r2;       // [nnodes] the bits of the largest squared corner distance
    double *area;                 // [ntl] |A_p|, then the running sum inside each block of 256
    double *base;                 // [ceil(ntl / 256) + 1] block totals, then their exclusive sums and the total
    float *nodes, *tris, *moments;  // the mesh's arrays
    uint32_t *thresholds;
};
hipError_t launch_tribuild_scan(const TriBuildArgs &A, hipStream_t st);   // the head's start values, the bound, faces and keys
constexpr int TRIBUILD_SCAN_LAUNCHES = 3;
hipError_t launch_tribuild_table(const TriBuildArgs &A, hipStream_t st);  // both sorts, vertex and edge sums
constexpr int TRIBUILD_TABLE_LAUNCHES = 2 * SORT_PAIR_LAUNCHES + 2;
// the gather, the leaves, one launch per level of inner nodes, the finish, R2 (two) and the area table (three)
hipError_t launch_tribuild_tree(const TriBuildArgs &A, hipStream_t st);
inline int tribuild_tree_launches(const TriBuildArgs &A) { return 8 + A.ninner_levels; }

// Composed scenes (nr_compose.hip; nr_compose_*): the distinct fp32 packs back to back in one device
// buffer (staged into dynamic LDS in that order), the parts, and the queried rays or points.  The
// struct travels in the kernarg segment: the part loop is wave-uniform and reads it with scalar loads.
struct ComposeNet {
    int off;                      // the pack's first float in the buffer (and in LDS)
    int in0, nh, f32_clamp;       // as MlpArgs
};
struct ComposePart {
    float rot[9];                 // nr_part::rot
    float pos[3];
    float scale, inv_s;           // inv_s = 1.0f / scale, formed on the host
    int net, op;
};
constexpr int NR_COMPOSE_NETS = 4, NR_COMPOSE_PARTS = 16;
struct ComposeArgs {
    const float *packs;
    int pack_bytes;               // all packs, a multiple of 16
    int nnets, nparts;
    ComposeNet nets[NR_COMPOSE_NETS];
    ComposePart parts[NR_COMPOSE_PARTS];
    float center[3], r2;          // the world bound: centre, radius * radius
    // the rays (QueryArgs' fields; origins NULL: the pixel rays of the W x H view)
    const float *origins, *dirs;
    long n;                       // rays or sample points, <= 2^30
    int W, H;
    double inv_w;
    float rcp_w, rcp_h;
    float inv_view[12];
    int max_steps, frame;
    int32_t *status, *steps;
    float *t, *position, *normal;
    int32_t *part;                // [n] the owner of a hit, -1 otherwise
    // k_compose_sample
    const float *points;          // [n][3]
    float *value;                 // [n]
    int32_t *owner;               // [n]
    uint32_t *cursor;             // next ray to deal (zeroed before the launch)
    unsigned long long *stats;    // [0] ray-steps, [1] rays that entered the bound, [2] max steps, [3] hits,
                                  // [4] in-bound (marching ray, part) pairs, [5] wave evaluations issued, [6] skipped
};
// dynamic LDS of a k_compose workgroup of `threads` threads: the packs, then one list of converged rays per wave
int compose_lds_bytes(const ComposeArgs &C, int threads);
hipError_t launch_compose(const ComposeArgs &C, int grid, int threads, hipStream_t st);         // threads: 256, 512 or 768
hipError_t launch_compose_sample(const ComposeArgs &C, int grid, hipStream_t st);               // 4-wave workgroups
// colours the HIT pixels of a W x H geometry buffer (A: W, H, out, view, colouring), 0 elsewhere
hipError_t launch_compose_color(const RenderArgs &A, const int32_t *status, const float *normal, hipStream_t st);

// Lighting of a composed scene (nr_compose_light.hip; nr_compose_render_lit): the W x H geometry buffer
// k_compose<true> left, the light, and one ao, one shadow and one occluder value per pixel.  The
// ComposeArgs of the launch carry the packs, nets, parts, the bound, n = W H, frame, cursor and stats
// ([0] shadow-ray steps, [2] the longest shadow ray's, [4] in-bound (marching shadow ray, part) pairs,
// [5] wave evaluations issued, [6] skipped).
struct ComposeLightArgs {
    const int32_t *status;        // [n] NR_RAY_*
    const float *position, *normal;  // [n][3], of the hits
    float dir[3];                 // nr_light, field by field
    int shadow_steps;
    float shadow_bias, shadow_k, ao_step, ao_strength;
    float *ao, *shadow;           // [n], both always written
    int32_t *occluder;            // [n] or NULL: the owner at the converging step of a shadow ray that ends HIT, else -1
};
// dynamic LDS of a k_compose_light workgroup of `threads` threads: the packs, then two lists of hit pixels per wave
int compose_light_lds_bytes(const ComposeArgs &C, int threads);
hipError_t launch_compose_light(const ComposeArgs &C, const ComposeLightArgs &X, int grid, int threads, hipStream_t st);  // threads: 256, 512 or 768

// Composed-scene lattices and meshes (nr_compose_mesh.hip; nr_compose_sample_grid,
// nr_compose_extract_mesh, nr_compose_extract_mesh_sparse).  The ComposeArgs of these launches carry
// the packs, nets, parts, frame and stats ([4] in-bound (lattice point, part) pairs of the sampling
// passes, [5] wave evaluations issued, [6] skipped); the workgroup is k_compose's (threads: 256, 512
// or 768) and its dynamic LDS the packs alone.
struct ComposeGridArgs {
    LatticeArgs L;
    float *value;                 // [n] or NULL
    int32_t *owner;               // [n] or NULL
};
struct ComposeVertexArgs {
    const float *vertices;        // [nv][3]
    float *normals;               // [nv][3] or NULL: the normalised tetrahedral gradient of the composed field
    int32_t *part;                // [nv] or NULL: the owner of the field at the vertex
    long nv;
};
struct SparseArgs;
hipError_t launch_compose_grid(const ComposeArgs &C, const ComposeGridArgs &G, int grid, int threads, hipStream_t st);
hipError_t launch_compose_vertex(const ComposeArgs &C, const ComposeVertexArgs &V, int grid, int threads, hipStream_t st);
// k_sp_coarse / k_sp_sample with the composed field (A.scene and A.frame are not read: C.frame)
hipError_t launch_compose_sp_coarse(const ComposeArgs &C, const SparseArgs &A, int grid, int threads, hipStream_t st);
hipError_t launch_compose_sp_sample(const ComposeArgs &C, const SparseArgs &A, int grid, int threads, hipStream_t st);

int dense_lds_bytes(int in, int out);
int grad_lds_bytes(const MlpArgs &M, const GradArgs &G);  // one k_grad workgroup's dynamic LDS
hipError_t launch_grad(const GradArgs &G, const MlpArgs &M, int grid, hipStream_t st);  // 4-wave workgroups
int fit_lds_bytes(int nh);  // one k_fit_grad workgroup's dynamic LDS
hipError_t launch_fit_grad(const FitArgs &F, int grid, hipStream_t st);  // FIT_WAVES-wave workgroups
hipError_t launch_fit_update(const FitUpdArgs &U, hipStream_t st);
int project_lds_bytes(const MlpArgs &M, const ProjArgs &P);  // one k_project workgroup's dynamic LDS
hipError_t launch_project(const ProjArgs &P, const MlpArgs &M, int grid, hipStream_t st);  // 4-wave workgroups
hipError_t launch_grid(const GridArgs &G, const MlpArgs &M, int grid, hipStream_t st);
hipError_t launch_vnormal(const VNormalArgs &V, const MlpArgs &M, int grid, hipStream_t st);
hipError_t launch_mesh_count(const MeshArgs &A, hipStream_t st);  // k_mesh_count, then k_mesh_scan
hipError_t launch_mesh_emit(const MeshArgs &A, hipStream_t st);
hipError_t launch_mesh_scan(const MeshArgs &A, hipStream_t st);  // k_mesh_scan alone: reads nblk, cnt; writes off, total
// nr_sparse.hip (SparseArgs: nr_internal.h)
struct SparseArgs;
hipError_t launch_sparse_coarse(const SparseArgs &A, const MlpArgs &M, int grid, hipStream_t st);
hipError_t launch_sparse_classify_count(const SparseArgs &A, hipStream_t st);
hipError_t launch_sparse_classify_emit(const SparseArgs &A, hipStream_t st);
hipError_t launch_sparse_sample(const SparseArgs &A, const MlpArgs &M, int grid, hipStream_t st);
hipError_t launch_sparse_mesh_count(const SparseArgs &A, hipStream_t st);
hipError_t launch_sparse_mesh_emit(const SparseArgs &A, hipStream_t st);
// nr_trimesh_grid.hip: a mesh's signed distance into D.sdf over points generated in the kernel
// (D.X, D.n, W->X and W->n are not read) -- k_trimesh_grid_distance and, with W (W->sdf = D.sdf), the
// k_trimesh_grid_winding launch that signs the values in place.  The grid by `cus`, the CU count:
// 4-wave workgroups, at most 8 per CU.  lattice: D.sdf [L.n], 4 x 4 x 4 blocks per wave; sparse:
// store == false the brick-corner lattice into D.sdf = S.coarse, store == true the active bricks'
// point sets into D.sdf = S.store (k_sp_coarse's and k_sp_sample's points and slots).
hipError_t launch_trimesh_lattice(const TriMeshArgs &D, const TriWindArgs *W, const LatticeArgs &L, int cus, hipStream_t st);
hipError_t launch_trimesh_sparse(const TriMeshArgs &D, const TriWindArgs *W, const SparseArgs &S, bool store, int cus,
                                 hipStream_t st);
hipError_t launch_query(const QueryArgs &Q, const MlpArgs &M, int grid, hipStream_t st);
hipError_t launch_aa_detect(const AaArgs &X, hipStream_t st);
hipError_t launch_aa_trace(const RenderArgs &A, const AaArgs &X, const MlpArgs &M, int grid, hipStream_t st);  // 4-wave workgroups
hipError_t launch_aa_resolve(const AaArgs &X, hipStream_t st);
hipError_t launch_light_trace(const LightArgs &X, const MlpArgs &M, int grid, hipStream_t st);  // 4-wave workgroups
hipError_t launch_light_resolve(const RenderArgs &A, const LightArgs &X, hipStream_t st);  // A: W, H, out, view, colouring
hipError_t launch_dense(const DenseArgs &D, int src, int grid, hipStream_t st);
hipError_t launch_init_f(const RenderArgs &A, const FrameArgs *F, const QueueArgs &Q, long npix, long total,
                         int grid, hipStream_t st);
hipError_t launch_march16(const RenderArgs &A, const MlpArgs &M, const QueueArgs &Q, const FrameArgs *F, int prec,
                          int it, int grid, hipStream_t st, int mode = 0);
hipError_t launch_shade16(const RenderArgs &A, const MlpArgs &M, const QueueArgs &Q, const FrameArgs *F, int grid,
                          hipStream_t st);
hipError_t launch_set_args(const RenderArgs &A, RenderArgs *d, hipStream_t st);
hipError_t launch_init_l(const RenderArgs *Ad, const QueueArgs &Q, long npix, hipStream_t st);
hipError_t launch_march_l(const RenderArgs *Ad, const QueueArgs &Q, const float *sdf, int it, int grid, hipStream_t st);
hipError_t launch_shade_l(const RenderArgs *Ad, const QueueArgs &Q, const float *sdf4, int grid, hipStream_t st);
hipError_t launch_trace(const RenderArgs &A, const MlpArgs &M, const TraceArgs &T, int prec, int grid, hipStream_t st);
hipError_t launch_mlp16(const MlpArgs &M, int prec, const float *X, float *Y, long n, int grid, hipStream_t st);
hipError_t launch_mlp_latency(const MlpArgs &M, int prec, const float *X, float *Y, int reps, int nt, int part,
                              hipStream_t st);
hipError_t launch_order(const uint32_t *bcost, uint32_t *order, int nblocks, int bw, int dilate, hipStream_t st);
hipError_t launch_assemble(const uint32_t *src, size_t stride, uint32_t *dst, int W, int H, int band, int nshards,
                           hipStream_t st);

}  // namespace nr
