// nr_internal.h -- declarations shared by the host side of libnr.so.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/neural_render.h"

#if defined(__HIPCC__)
#define NR_HD __host__ __device__
#else
#define NR_HD
#endif

namespace nr {

// ---- host-side file formats (h5_keras.cpp, png_codec.cpp) ----
int h5_read_keras(const char *path, std::vector<int> &dims, std::vector<std::vector<float>> &kernels,
                  std::vector<std::vector<float>> &biases, std::string &err);
int png_decode(const char *path, std::vector<uint32_t> &rgba, int &w, int &h, std::string &err);
int png_encode(const char *path, const uint32_t *rgba, int w, int h, int flip, std::string &err);
int ppm_encode(const char *path, const uint32_t *rgba, int w, int h, std::string &err);
// Records the calling thread's last error (nr_last_error(NULL)) and returns code.
int report_error(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// ---- packed network layouts (nr_pack.cpp) ----
// fp32 16-point-tile layout (nr_mlp16.h), in floats.  Lane (j, g) of a wave = row /
// point j, unit group g; hidden unit u lives in register k of group g with u = 4k + g
// (u = 8g + k for the layer that feeds the final VALU layer), so every f32 MFMA chain
// runs over k ascending:
//   [0,128)    layer-0 A operand   [row tile 2][lane 64]      (k = x, y, z, frame)
//   [128,160)  layer-0 bias        [group 4][register 8]
//   per hidden layer j (0..nh-1), base 160 + j*1056:
//              A operand           [m >> 2][lane 64][m & 3]   (m = 2 * k-step + row tile)
//              bias                [group 4][register 8]
//   final:     weights [group 4][register 8], bias [1], layer-0 output scale 2^-e0 [1] (+2 pad)
constexpr int PK_L0W = 0;
constexpr int PK_L0B = 128;
constexpr int PK_HID = 160;
constexpr int PK_HID_STRIDE = 1024 + 32;
constexpr int MAX_HIDDEN = 16;
NR_HD constexpr inline int pk_final(int nh) { return PK_HID + nh * PK_HID_STRIDE; }
NR_HD constexpr inline int pk_floats(int nh) { return pk_final(nh) + 36; }

// Backward (gradient) pack beside the fp32 one (pack_grad_16; nr_grad.h), in floats, raw
// (unscaled) weights.  The backward pass of hidden layer j is the forward's MFMA loop on the
// transposed kernel: row (A operand) = the layer's input unit, k = its output unit, so every
// chain runs over the output units 0..31 ascending.  The gradient of register k of lane group g
// belongs to unit 4k + g -- the order the forward's masks of layers 0..nh-1 are in, and the
// order a C result is the next B operand in; the last ReLU layer's mask (units 8g + k in the
// forward) is transposed once per tile.
//   per hidden layer j (0..nh-1), base j*1024:
//              A operand           [m >> 2][lane 64][m & 3]   (m = 2 * k-step + row tile), lane
//                                  (i, kk): K_(j+1)[in = 16mt + 4(i & 3) + (i >> 2)][out = 4st + kk]
//   gb_l0(nh): K_0 transposed, one row tile [k-step >> 2][lane 64][k-step & 3], lane (i, kk):
//              K_0[in = i & 3][out = 4st + kk] (0 for i & 3 >= dims[0]): rows repeat every 4, so
//              every lane group's C registers 0..3 hold the point's gradient
//   gb_last(nh): the last kernel [group 4][register 8] = K_last[4k + g]
// The masks of the nh + 1 ReLU layers are 8 bits per lane, tile and layer in two 32-bit words,
// hence GRAD_MAX_HIDDEN.
constexpr int GRAD_MAX_HIDDEN = 7;
NR_HD constexpr inline int gb_l0(int nh) { return nh * 1024; }
NR_HD constexpr inline int gb_last(int nh) { return gb_l0(nh) + 512; }
NR_HD constexpr inline int gb_floats(int nh) { return gb_last(nh) + 32; }

// The fit pack (nr_fit.hip; nr_fit_*): what k_fit_grad stages in LDS and k_fit_update rewrites on the
// device after every step, in floats, raw weights.
//   forward, pk_floats(nh) floats in the PK_* layout above, except that every ReLU layer keeps unit
//   4k + g in register k of lane group g (the last one too) and the final layer is
//   [unit 32] in natural order, bias [1] (+3 pad): its chain runs in the point's lane over staged
//   activations;
//   backward, at fit_bwd(nh): hidden layer j's transposed A operand at j * 1024, as the backward
//   pack's.  (No transposed K_0 and no copy of the last kernel: the weight gradients need d_0 but
//   not d value / d input, and the last kernel is read from the forward part.)
// Flat parameter order (nr_fit_gradient's grad, nr_fit_weights' params): K_0 [3][32], B_0 [32],
// K_l [32][32], B_l [32] for l = 1..nh, K_last [32], B_last [1].
NR_HD constexpr inline int fit_bwd(int nh) { return pk_floats(nh); }
NR_HD constexpr inline int fit_pack_floats(int nh) { return pk_floats(nh) + nh * 1024; }
NR_HD constexpr inline int fit_off_k(int l) { return l == 0 ? 0 : 128 + (l - 1) * 1056; }  // l = 0 .. nh + 1
NR_HD constexpr inline int fit_off_b(int l) { return l == 0 ? 96 : fit_off_k(l) + 1024; }  // l = 0 .. nh
NR_HD constexpr inline int fit_params(int nh) { return fit_off_k(nh + 1) + 33; }
// per-wave LDS of k_fit_grad, in floats: the nh + 1 ReLU layers' activations and one layer's deltas
// as [unit 32][point 16], the inputs [4][16] (row 3: ones), the residuals e and g [2][16]
NR_HD constexpr inline int fit_wave_floats(int nh) { return (nh + 2) * 512 + 64 + 32; }
constexpr int FIT_WAVES = 4;
constexpr int FIT_CHUNKS = 16;  // the totals' two-level order (include/neural_render.h, nr_fit_*)
constexpr int FIT_PARTIALS_DEFAULT = 1024;

// Low-precision (bf16/fp16) pack for the 32-point-tile MLP (nr_mlp16.h, mlp32_lowp):
// v_mfma_f32_32x32x16_{bf16,f16}, lane l = (row / point r = l & 31, half h = l >> 5).
// 16-bit elements (a_ops):
//   [0, 512)                    layer-0 A operand [lane 64][8]: K = 16 slots holding the
//                               hi/lo split of weights and inputs (w*x ~ wh*xh + wh*xl + wl*xh)
//   LP32_HID + j*LP32_HSTRIDE   hidden layer j: A operand [k-step 2][lane 64][8]; element e of
//                               lane half h in k-step s multiplies unit 16s + 8(e>>2) + 4h + (e&3)
//                               (the accumulator-as-B-operand order of the previous layer)
//   lp32_final(nh)              final layer: row 0 of the A operand only, [k-step 2][h 2][8]
// floats (fl): biases as accumulator inits, [h 2][register 16] per layer (register i of half
// h = unit (i&3) + 8(i>>2) + 4h): layer 0 at 0, hidden j at 32 + 32j, final bias at 32 + 32nh.
constexpr int LP32_HID = 512;
constexpr int LP32_HSTRIDE = 1024;
NR_HD constexpr inline int lp32_final(int nh) { return LP32_HID + nh * LP32_HSTRIDE; }
NR_HD constexpr inline int lp32_elems(int nh) { return lp32_final(nh) + 32; }
NR_HD constexpr inline int lp32_floats(int nh) { return 32 + 32 * nh + 4; }
// bf16 clamped-ReLU pack: every network input within +-LP_INPUT_BOUND keeps every scaled
// activation at or below 1/4 (interval bounds, nr_pack.cpp pack_lowp_32)
constexpr float LP_INPUT_BOUND = 1048576.0f;
// fp32 clamped-ReLU pack (pack_fp32_16): inputs within +-F32_INPUT_BOUND keep every scaled
// activation at or below 1/2 (nr_mlp16.h inputs_in_bound_f32; beyond it the add + max form)
constexpr float F32_INPUT_BOUND = 1024.0f;

// fp32x3 pack (pack_x3_32): fp32-class hidden layers on the fp16 matrix core by a three-term
// split, a.w ~ ah.wh + al.wh + ah.wl (nr_mlp16.h mlp32_x3_nt).  16-bit elements (fp16):
//   [0, 512)                    layer-0 A operand, as LP32 (hi/lo split of scaled weights)
//   X3_HID + j*X3_HSTRIDE       hidden layer j: hi A operand [k-step 2][lane 64][8], then the
//                               residual (lo) A operand in the same order (+1024)
// floats (fl): layer-0 bias [h 2][register 16] at 0, hidden j's bias at 32 + 32j (all scaled,
// accumulator inits), the final layer's f32 weights in the accumulator's register order
// [h 2][register 16] at x3_final(nh), its bias at +32, then -1 (the residual's multiplier, read
// at run time so that the compiler emits v_fma_mix), the xyz input scale and the 4th input's
// scale.  Activations of ReLU layer l are scaled by 2^-e[l] so that their interval bound over
// inputs within X3_INPUT_BOUND (xyz) / X3_FRAME_BOUND (4th input) is at most 2^10: the split's
// residual (x - rtz(x)) is then below 1 and the clamp of v_fma_mixlo_f16 is its ReLU.
constexpr int X3_HID = 512;
constexpr int X3_HSTRIDE = 2048;
NR_HD constexpr inline int x3_elems(int nh) { return X3_HID + nh * X3_HSTRIDE; }
NR_HD constexpr inline int x3_final(int nh) { return 32 + 32 * nh; }
NR_HD constexpr inline int x3_floats(int nh) { return x3_final(nh) + 36; }
constexpr float X3_INPUT_BOUND = 4.0f;
constexpr float X3_FRAME_BOUND = 1024.0f;
constexpr int X3_XYZ_SHIFT = 6;  // xyz inputs enter layer 0 times 2^6

bool fused_shape_ok(const std::vector<int> &dims);
// Keras kernels (in x out, row-major) -> packs.  Return false if the shape is not
// [3|4, 32, ..., 32, 1] (those networks render on the layered schedule).
// pack_fp32_16: clamp (if not null) = 1 when the pack is scaled for the clamped ReLU
bool pack_fp32_16(const std::vector<int> &dims, const std::vector<std::vector<float>> &kernels,
                  const std::vector<std::vector<float>> &biases, std::vector<float> &pack, int *clamp = nullptr);
// The pruned fp32 pack (the batched fp32 k_trace; nr_mlp16.h mlp16_fp32_pruned): the scaled pack's
// values in the PK_* layout, except that
//   * the units of every ReLU layer l (0..nh) are re-ordered: position p holds unit order[l][p] --
//     the layer's live units in ascending index, then its cand[l] candidates (a multiple of 4:
//     units that fire at next to no point of the marched volume).  Rows (outputs, biases) and the
//     next layer's k positions follow the same order, so a chain over positions 0..31 is the
//     original chain with the candidates' terms moved to its end, and ks[l] = (32 - cand[l]) / 4
//     is the number of k-steps the next layer needs while every candidate's activation is +0;
//   * the last ReLU layer keeps position 4k + g in register k of lane group g like the others
//     (the full pack: 8g + k), and the final weights are stored by position: the final chain runs
//     in the point's own lane after a transpose, at every tile count.
// mode (nr_set_prune): 0 = no candidates (identity order, ks all 8); 1 = candidates chosen from
// the units' firing counts over a fixed sample (nr_pack.cpp, the rule in DESIGN.md section 5);
// 2 = the four highest-numbered units of every layer.  No candidates either for 4 inputs,
// non-finite weights or a bias of -0.  False (no pack) if the shape is not fused or the scaled
// pack is refused.
struct PruneInfo {
    int nrelu = 0;           // ReLU layers: nh + 1
    std::vector<int> cand;   // [nrelu]
    std::vector<int> ks;     // [nrelu], 4..8
    std::vector<int> order;  // [nrelu][32]
};
bool pack_fp32_16_pruned(const std::vector<int> &dims, const std::vector<std::vector<float>> &kernels,
                         const std::vector<std::vector<float>> &biases, int mode, std::vector<float> &pack,
                         PruneInfo &info);
// MlpArgs::ks_bits: ks[l] - 4 in bits [3l, 3l + 3)
inline unsigned long long prune_ks_bits(const PruneInfo &p) {
    unsigned long long b = 0;
    for (int l = 0; l < p.nrelu; ++l) b |= (unsigned long long)(p.ks[l] - 4) << (3 * l);
    return b;
}
// The unit pack (the batched fp32 k_trace; nr_mlp16.h mlp64_fp32_units): the scaled pack's values
// (clamp_scales / apply_scales as pack_fp32_16, bit for bit) in identity unit order, pk_floats(nh)
// floats like the others:
//   [0,128)    layer-0 weights     [input 4][row 32]          (0 for input >= dims[0]; unscaled)
//   [128,160)  layer-0 bias        [row 32]
//   per hidden layer j (0..nh-1), base 160 + j*1056:
//              weights             [k >> 2][row 32][k & 3]    (k = input unit: a lane reads four
//                                                              consecutive k of its row at once)
//              bias                [row 32]
//   final:     weights [unit 32], bias [1], layer-0 output scale 2^-e0 [1] (+2 pad)
// False (no pack) if the shape is not fused, the scaled pack is refused, a weight or bias is not
// finite, or a bias is -0 (the exactness argument in nr_mlp16.h).
bool pack_fp32_units(const std::vector<int> &dims, const std::vector<std::vector<float>> &kernels,
                     const std::vector<std::vector<float>> &biases, std::vector<float> &pack);
// the backward pack (above); false if the shape is not fused or has more than GRAD_MAX_HIDDEN
// hidden 32 x 32 layers
bool pack_grad_16(const std::vector<int> &dims, const std::vector<std::vector<float>> &kernels,
                  std::vector<float> &pack);
bool pack_lowp_32(const std::vector<int> &dims, const std::vector<std::vector<float>> &kernels,
                  const std::vector<std::vector<float>> &biases, int precision,
                  std::vector<uint16_t> &a_ops, std::vector<float> &bias, int *clamp = nullptr);
// The 16x16x32 form of pack_lowp_32's output for k_mlp16 (round 6; nr_mlp16_asm.h NR_S16_*,
// tools/gen_mlp_asm.py build_s16): the same elements re-ordered -- the input layer's rows permuted,
// each hidden layer's A operand as [half 2][lane 64][8] (lane (row j, group g): output unit
// U(half, j), k-slot 8g + e: input unit V(g, e)) and its bias as [group 4][half 2][4]; the final
// layer unchanged.  Same sizes as the 32x32x16 pack.
void pack_lowp_s16(const std::vector<uint16_t> &a32, const std::vector<float> &f32, int nh,
                   std::vector<uint16_t> &a16, std::vector<float> &f16);
// ok (if not null) = 1 when the scales exist (every scaled weight and bound inside fp16's range)
// and leave every ReLU layer's activations inside the window where the split keeps its bits
// (nr_pack.cpp X3_SPLIT_FLOOR); otherwise the kernels run the fp32 MLP for every point
bool pack_x3_32(const std::vector<int> &dims, const std::vector<std::vector<float>> &kernels,
                const std::vector<std::vector<float>> &biases, std::vector<uint16_t> &a_ops, std::vector<float> &fl,
                int *ok = nullptr);

// ---- brick-sparse isosurface extraction (nr_sparse.hip; nr_extract_mesh_sparse) ----
// The lattice and its bricks of B cells a side.  The values of an active brick's point set live in
// a compact store: slot a of the active list (ascending brick index) owns the floats
// [a * stride, a * stride + (B + 1)^3), local point (li, lj, lk) at (lk (B + 1) + lj)(B + 1) + li.
// stride = (B + 1)^3 rounded up to a multiple of 64, so that a wave's 64 consecutive store points
// belong to one brick.  A ragged brick (the last of an axis) uses the points up to its extent.
struct SparseLattice {
    float origin[3], step[3];
    int nx, ny, nz;
    int B, S;                     // brick edge in cells: 4, 8 or 16; S = B + 1
    int nbx, nby, nbz;            // bricks per axis, ceil((dim - 1) / B)
    uint32_t nbricks;             // nbx nby nbz <= 2^30
    uint32_t ncoarse;             // (nbx + 1)(nby + 1)(nbz + 1): the brick-corner lattice
    uint32_t P, stride;           // S^3 and its multiple of 64
    double inv_nbx, inv_nbxy;     // reciprocals for udiv_r: the brick index,
    double inv_cx, inv_cxy;       // the corner lattice (nbx + 1, (nbx + 1)(nby + 1)),
    double inv_s, inv_ss;         // the local index (S, S^2)
    double inv_wpb;               // and a wave's brick slot (stride / 64 waves per brick)
};

struct SparseArgs {
    SparseLattice L;
    float iso, band;
    int scene, frame;
    float *coarse;                // [ncoarse] the values at the brick corners
    int32_t *map;                 // [nbricks] the brick's slot in the active list, -1: culled
    int nblk_b;                   // ceil(nbricks / 256)
    uint32_t *bcnt;               // [2][nblk_b]: active bricks, their point-set sizes, per 256 bricks
    unsigned long long *boff;     // [2][nblk_b]: their exclusive scans
    unsigned long long *btotal;   // [2]
    uint32_t nactive;             // (read on the host once, after the classification)
    uint32_t *list;               // [nactive] the active bricks, ascending
    float *store;                 // [nactive][stride]
    uint32_t *word;               // [nactive][stride]: as MeshArgs::word, over 256-point blocks of the store
    int nblk_m;                   // ceil(nactive stride / 256)
    uint32_t *cnt;                // [2][nblk_m]
    unsigned long long *off;      // [2][nblk_m]
    unsigned long long *total;    // [2]
    float *vertices;              // [nv][3]
    long long *keys;              // [nv] or null
    int32_t *triangles;           // [nt][3]
};

// ---- triangle meshes (nr_trimesh_host.cpp: host only; nr_trimesh.hip k_trimesh_distance) ----
// The OBJ reader behind nr_obj_load: `v` and `f` records, triangles as fans; NR_OK, NR_E_IO or NR_E_FORMAT.
int obj_parse(const char *path, std::vector<float> &V, std::vector<int32_t> &T, std::string &err);
bool trimesh_indices_ok(const int32_t *T, long nt, long nv);
// nr_trimesh_normals on checked arguments (table [nt][7][3] or NULL, closed or NULL)
void trimesh_normals(const float *V, long nv, const int32_t *T, long nt, float *table, int *closed);
// The hierarchy over the triangles whose face entry in `table` is not zero, in device layout:
//   nodes  8 words each: lo.xyz, first | left, hi.xyz, -count | right -- the inflated box, then a leaf's
//          triangles [first, first + count) of `tris` (word 7 <= 0) or an inner node's children (word 7
//          > 0; the root is node 0, so no child is).  Preorder: a node, its left subtree, its right one.
//   tris   12 words each, leaf by leaf: a.xyz, original index, b.xyz, 0, c.xyz, 0
//   moments 16 words each, node by node (k_trimesh_winding's far field; include/neural_render.h):
//          centre.xyz, R2, N.xyz, 0, Sxx, Syy, Szz, Sxy, Sxz, Syz, 0, 0
// Boxes are inflated by slack = 2^-TRIMESH_SLACK_SHIFT (largest |coordinate| + largest axis extent)
// and rounded outward.  False when the depth exceeds ceil(log2 ntl) + 1 or TRIMESH_STACK (the wave's
// stack in k_trimesh_distance and k_trimesh_winding holds one pending child per level).
constexpr int TRIMESH_SLACK_SHIFT = 18;
constexpr int TRIMESH_STACK = 32;
constexpr int TRIMESH_LEAF_DEFAULT = 8;
struct TriBvh {
    std::vector<float> nodes, tris, moments;
    long nnodes = 0, ntl = 0;
    int depth = 0;
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};  // the vertices' bound, not inflated
    float slack = 0;
};
bool trimesh_build(const float *V, long nv, const int32_t *T, long nt, int leaf, const float *table, TriBvh &out);
// The area table of H's positions (nr_mesh_sample's triangle choice; include/neural_render.h):
// thresholds [ntl] = min(floor(C_p / C_last 2^32), 2^32 - 1) of the running f64 area sum C, and the
// last position whose threshold exceeds its predecessor's; -1 (thresholds all 0) when the area sum
// is not > 0.
long trimesh_area_table(const TriBvh &H, std::vector<uint32_t> &thresholds);

// ---- camera (nr_pack.cpp; the C ABI's nr_camera) ----
void camera_matrices(float rx, float ry, float zoom, float tx, float ty, float inv_view[12], float normal[16]);
void camera_matrices_eigen(float rx, float ry, float zoom, float tx, float ty, float inv_view[12], float normal[16]);

}  // namespace nr
