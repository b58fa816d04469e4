// nr_api_trimesh.hip -- the C ABI's triangle meshes (nr_trimesh_*).
#include <climits>
#include <cmath>
#include <map>
#include <new>
#include <vector>

#include "nr_ctx.h"

using namespace nr;

// ---- triangle meshes (nr_trimesh_*; nr_trimesh_host.cpp, nr_trimesh.hip, nr_winding.hip, nr_mesh_rays.hip) ----
// The hierarchy with its moments, the reordered triangles and the pseudonormal table are built at
// create time, on the host (nr_trimesh_create) or by kernels (nr_mesh_create_device, further
// down), and live on the device; a distance query is one launch, a winding query
// one, or two with the sdf output, a ray query (nr_mesh_rays.hip) one.  (struct nr_trimesh: nr_ctx.h)

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
    m->scale = std::ldexp(H.slack, TRIMESH_SLACK_SHIFT);
    std::vector<uint32_t> area;
    m->area_last = trimesh_area_table(H, area);
    area.resize(std::max<size_t>(area.size(), 1), 0u);
    hipError_t e = hipSetDevice(owner->device);
    hipStream_t s = e == hipSuccess ? cur_stream(owner) : nullptr;
    if (e == hipSuccess && owner->use_own && !owner->own_stream) { delete m; return NR_E_HIP; }
    if (e == hipSuccess) e = hipMalloc(&m->d_nodes, H.nodes.size() * 4);
    if (e == hipSuccess) e = hipMalloc(&m->d_tris, H.tris.size() * 4);
    if (e == hipSuccess) e = hipMalloc(&m->d_table, table.size() * 4);
    if (e == hipSuccess) e = hipMalloc(&m->d_moments, H.moments.size() * 4);
    if (e == hipSuccess) e = hipMalloc(&m->d_area, area.size() * 4);
    if (e == hipSuccess) e = hipMemcpyAsync(m->d_area, area.data(), area.size() * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMalloc(&m->d_stats, 128);
    if (e == hipSuccess) e = hipMemcpyAsync(m->d_nodes, H.nodes.data(), H.nodes.size() * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(m->d_tris, H.tris.data(), H.tris.size() * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(m->d_table, table.data(), table.size() * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(m->d_moments, H.moments.data(), H.moments.size() * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // (the sources are locals)
    if (e != hipSuccess) {
        const bool nomem = e == hipErrorOutOfMemory;
        dfree(m->d_nodes); dfree(m->d_tris); dfree(m->d_table); dfree(m->d_moments); dfree(m->d_area); dfree(m->d_stats);
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
    dfree(m->d_nodes); dfree(m->d_tris); dfree(m->d_table); dfree(m->d_moments); dfree(m->d_area); dfree(m->d_stats); dfree(m->d_io);
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
    // staged: the points, then every output the caller asked for
    Staging io(loc);
    io.in(A.X, 3 * N);
    io.out(A.sdf, N); io.out(A.closest, 3 * N); io.out(A.tri, N); io.out(A.feature, N);
    int rc;
    if ((rc = io.begin(c, m->d_io, m->cap_io, s)) != NR_OK) return rc;
    // a grid-stride over chunks of 64 points: at most 8 four-wave workgroups per CU
    const size_t chunks = (N + 63) / 64;
    const int grid = (int)std::max<size_t>(1, std::min<size_t>((chunks + 3) / 4, (size_t)num_cus(c->device) * 8));
    nr_stats st{};
    HIPCHK(c, hipEventRecord(c->ev0, s));
    HIPCHK(c, hipMemsetAsync(m->d_stats, 0, 8, s));
    HIPCHK(c, launch_trimesh_distance(A, grid, s));
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if ((rc = io.end(c, s)) != NR_OK) return rc;
    unsigned long long evals = 0;
    if (stats) HIPCHK(c, hipMemcpyAsync(&evals, m->d_stats, 8, hipMemcpyDeviceToHost, s));
    rc = end_timed(c, stats != nullptr, loc, s, &st.ms_total);
    if (rc != NR_OK || !stats) return rc;
    st.ray_steps = (uint64_t)n;
    st.shade_evals = evals;
    st.launches = 2;  // the counter's memset and k_trimesh_distance
    *stats = st;
    return NR_OK;
}

int nr_mesh_winding(nr_trimesh *m, const float *X, long n, float beta, float *winding, float *sdf, int flags, int loc,
                    nr_stats *stats) {
    if (!m) return set_err(nullptr, NR_E_INVALID, "nr_mesh_winding: mesh is NULL");
    nr_ctx *c = m->owner;
    if (!X) return set_err(c, NR_E_INVALID, "nr_mesh_winding: X is NULL");
    if (!winding && !sdf) return set_err(c, NR_E_INVALID, "nr_mesh_winding: winding and sdf are both NULL");
    if (n < 1 || n > (1l << 30)) return set_err(c, NR_E_INVALID, "nr_mesh_winding: n = %ld outside [1, 2^30]", n);
    if (!std::isfinite(beta) || beta < 0.0f) return set_err(c, NR_E_INVALID, "nr_mesh_winding: beta = %g is negative or not finite", (double)beta);
    if (flags & ~NR_TRIMESH_BRUTE) return set_err(c, NR_E_INVALID, "nr_mesh_winding: unknown flag bits %#x", flags);
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    const size_t N = (size_t)n;
    TriWindArgs A{};
    A.X = X; A.n = n;
    A.nodes = m->d_nodes; A.tris = m->d_tris; A.moments = m->d_moments;
    A.nnodes = (int)m->nnodes; A.ntl = (int)m->ntl;
    A.brute = (flags & NR_TRIMESH_BRUTE) != 0;
    A.beta = beta == 0.0f ? 2.0f : beta;
    A.winding = winding; A.sdf = sdf;
    A.stats = m->d_stats;
    Staging io(loc);
    io.in(A.X, 3 * N);
    io.out(A.winding, N); io.out(A.sdf, N);
    int rc;
    if ((rc = io.begin(c, m->d_io, m->cap_io, s)) != NR_OK) return rc;
    const size_t chunks = (N + 63) / 64;
    const int grid = (int)std::max<size_t>(1, std::min<size_t>((chunks + 3) / 4, (size_t)num_cus(c->device) * 8));
    nr_stats st{};
    HIPCHK(c, hipEventRecord(c->ev0, s));
    HIPCHK(c, hipMemsetAsync(m->d_stats, 0, 8, s));
    if (A.sdf) {
        // the magnitude first, by the distance call's own launch; k_trimesh_winding then signs it in place
        TriMeshArgs D{};
        D.X = A.X; D.n = n;
        D.nodes = m->d_nodes; D.tris = m->d_tris; D.table = m->d_table;
        D.nnodes = A.nnodes; D.ntl = A.ntl;
        D.brute = A.brute;
        D.sdf = A.sdf;
        D.stats = m->d_stats;
        HIPCHK(c, launch_trimesh_distance(D, grid, s));
    }
    HIPCHK(c, launch_trimesh_winding(A, grid, s));
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if ((rc = io.end(c, s)) != NR_OK) return rc;
    unsigned long long evals = 0;
    if (stats) HIPCHK(c, hipMemcpyAsync(&evals, m->d_stats, 8, hipMemcpyDeviceToHost, s));
    rc = end_timed(c, stats != nullptr, loc, s, &st.ms_total);
    if (rc != NR_OK || !stats) return rc;
    st.ray_steps = (uint64_t)n;
    st.shade_evals = evals;
    st.launches = A.sdf ? 3 : 2;  // the counter's memset, k_trimesh_distance for sdf, k_trimesh_winding
    *stats = st;
    return NR_OK;
}

}  // extern "C"

// ---- the device build (nr_trimesh_build.hip) and the download of what a mesh holds ----
// The kernels do everything but the tree's shape, which depends on (ntl, leaf) alone: made here
// once ntl is known (the first of the two records read back) and uploaded.

namespace {

// the float behind an ordered integer of TriBuildHead
float tb_decode(uint32_t e) {
    const uint32_t b = (e & 0x80000000u) ? e ^ 0x80000000u : ~e;
    float f;
    memcpy(&f, &b, 4);
    return f;
}

// the nodes of Builder::build's tree over n positions (nr_trimesh_host.cpp): non-decreasing in n
long tree_nodes(long n, int leaf, std::map<long, long> &memo) {
    if (n <= leaf) return 1;
    const auto it = memo.find(n);
    if (it != memo.end()) return it->second;
    const long half = (n + 1) / 2;
    return memo[n] = 1 + tree_nodes(half, leaf, memo) + tree_nodes(n - half, leaf, memo);
}

// That tree's shape in preorder: links, position ranges, and `list` = the leaves, then the inner nodes
// level by level from the deepest (level_off: where each of those levels starts).
struct TreeShape {
    std::vector<int32_t> w3, w7, first, count, list;
    std::vector<int> level_off;
    int nleaves = 0, depth = 0;
};
void tree_shape(long ntl, int leaf, TreeShape &S) {
    struct Todo { int32_t first, count, parent; int level; bool right; };
    std::vector<Todo> todo{{0, (int32_t)ntl, -1, 1, false}};
    std::vector<int> level;
    while (!todo.empty()) {
        const Todo t = todo.back();
        todo.pop_back();
        const int32_t me = (int32_t)S.w3.size();
        if (t.parent >= 0) (t.right ? S.w7 : S.w3)[(size_t)t.parent] = me;
        S.first.push_back(t.first);
        S.count.push_back(t.count);
        level.push_back(t.level);
        S.depth = std::max(S.depth, t.level);
        if (t.count <= leaf) {
            S.w3.push_back(t.first);
            S.w7.push_back(-t.count);
            continue;
        }
        S.w3.push_back(0);
        S.w7.push_back(0);
        const int32_t half = (t.count + 1) / 2;
        todo.push_back({t.first + half, t.count - half, me, t.level + 1, true});
        todo.push_back({t.first, half, me, t.level + 1, false});  // (the left child is numbered first)
    }
    const size_t nn = S.w3.size();
    S.list.reserve(nn);
    for (size_t i = 0; i < nn; ++i)
        if (S.w7[i] <= 0) S.list.push_back((int32_t)i);
    S.nleaves = (int)S.list.size();
    // the inner nodes by level, deepest first (level depth holds leaves only)
    std::vector<int> at((size_t)S.depth + 1, 0);  // at[l]: the inner nodes of levels deeper than l, then the cursor of level l
    for (size_t i = 0; i < nn; ++i)
        if (S.w7[i] > 0) ++at[(size_t)level[i] - 1];
    for (int l = S.depth - 1; l >= 0; --l) at[(size_t)l] += at[(size_t)l + 1];
    S.level_off.push_back(0);
    for (int l = S.depth - 1; l >= 1; --l) S.level_off.push_back(at[(size_t)l - 1]);
    S.list.resize(nn);
    for (size_t i = 0; i < nn; ++i)
        if (S.w7[i] > 0) S.list[(size_t)S.nleaves + (size_t)at[(size_t)level[i]]++] = (int32_t)i;
}

}  // namespace

extern "C" {

int nr_mesh_create_device(nr_ctx *owner, const float *d_vertices, long nv, const int32_t *d_triangles, long nt, int leaf,
                             nr_trimesh **out, nr_stats *stats) {
    const char *fn = "nr_mesh_create_device";
    if (out) *out = nullptr;
    if (!owner || !d_vertices || !d_triangles || !out) return set_err(owner, NR_E_INVALID, "%s: NULL argument", fn);
    if (nv < 1 || nv > (long)INT32_MAX) return set_err(owner, NR_E_INVALID, "%s: nv = %ld outside [1, 2^31)", fn, nv);
    if (nt < 1 || nt > (1l << 24)) return set_err(owner, NR_E_INVALID, "%s: nt = %ld outside [1, 2^24]", fn, nt);
    if (leaf < 0 || leaf > 32) return set_err(owner, NR_E_INVALID, "%s: leaf = %d outside 0..32", fn, leaf);
    if (leaf == 0) leaf = TRIMESH_LEAF_DEFAULT;
    nr_ctx *c = owner;
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    // scratch: the two sorts in d_sort; in d_tbuild (8-byte words) the record, fn, the areas and their
    // block sums, and per node of the largest tree nt triangles can give the shape, sums, box and r2
    const size_t NT = (size_t)nt, N3 = 3 * NT;
    const size_t tri_words = sort_scratch_words(NT), nblk_a = (NT + 255) / 256;
    std::map<long, long> memo;
    const size_t nn_max = (size_t)tree_nodes(nt, leaf, memo);
    const size_t w_head = 16, w_fn = 3 * NT, w_area = NT, w_base = nblk_a + 1, w_shape = (5 * nn_max + 1) / 2;
    const size_t w_sums = 19 * nn_max, w_box = 3 * nn_max, w_r2 = nn_max;
    int rc;
    if ((rc = ensure_buf(c, c->d_sort, c->cap_sort, tri_words + sort_scratch_words(N3))) != NR_OK) return rc;
    if ((rc = ensure_buf(c, c->d_tbuild, c->cap_tbuild, w_head + w_fn + w_area + w_base + w_shape + w_sums + w_box + w_r2)) != NR_OK)
        return rc;
    nr_trimesh *m = new (std::nothrow) nr_trimesh();
    if (!m) return set_err(c, NR_E_NOMEM, "out of host memory");
    m->owner = c;
    m->nv = nv; m->nt = nt;
    // from here on every exit but the last frees m and what it holds
    auto fail = [&](int code, hipError_t e) {
        (void)hipStreamSynchronize(s);
        dfree(m->d_nodes); dfree(m->d_tris); dfree(m->d_table); dfree(m->d_moments); dfree(m->d_area); dfree(m->d_stats);
        delete m;
        if (e != hipSuccess) return set_err(c, e == hipErrorOutOfMemory ? NR_E_NOMEM : NR_E_HIP, "%s: %s", fn, hipGetErrorString(e));
        return code;
    };
    TriBuildArgs A{};
    A.V = d_vertices; A.T = d_triangles; A.nv = nv; A.nt = nt;
    {
        uint32_t *w = c->d_sort;
        A.tkeys[0] = w; A.tvals[0] = w + NT; A.tkeys[1] = w + 2 * NT; A.tvals[1] = w + 3 * NT; A.ttable = w + 4 * NT;
        w += tri_words;
        A.ckeys[0] = w; A.cvals[0] = w + N3; A.ckeys[1] = w + 2 * N3; A.cvals[1] = w + 3 * N3; A.ctable = w + 4 * N3;
        unsigned long long *q = c->d_tbuild;
        A.head = reinterpret_cast<TriBuildHead *>(q); q += w_head;
        A.fn = reinterpret_cast<double *>(q); q += w_fn;
        A.area = reinterpret_cast<double *>(q); q += w_area;
        A.base = reinterpret_cast<double *>(q); q += w_base;
        int32_t *shape = reinterpret_cast<int32_t *>(q); q += w_shape;
        A.w3 = shape; A.w7 = shape + nn_max; A.first = shape + 2 * nn_max; A.count = shape + 3 * nn_max; A.list = shape + 4 * nn_max;
        A.sums = reinterpret_cast<double *>(q); q += w_sums;
        A.box = reinterpret_cast<float *>(q); q += w_box;
        A.r2 = q;
    }
    hipError_t e = hipMalloc(&m->d_table, NT * 21 * 4);
    if (e == hipSuccess) e = hipMalloc(&m->d_stats, 128);
    if (e != hipSuccess) return fail(0, e);
    A.table = m->d_table;
    int launches = TRIBUILD_SCAN_LAUNCHES;
    TriBuildHead head;
    e = hipEventRecord(c->ev0, s);
    if (e == hipSuccess) e = launch_tribuild_scan(A, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&head, A.head, sizeof head, hipMemcpyDeviceToHost, s);  // the first record
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(0, e);
    if (head.err & 1u) return fail(set_err(c, NR_E_INVALID, "%s: a vertex index outside 0..%ld", fn, nv - 1), hipSuccess);
    if (head.err & 2u) return fail(set_err(c, NR_E_INVALID, "%s: a vertex that is not finite", fn), hipSuccess);
    // the bound and the boxes' slack, as trimesh_build forms them
    double extent = 0.0;
    for (int a = 0; a < 3; ++a) {
        m->lo[a] = tb_decode(head.lo[a]);
        m->hi[a] = tb_decode(head.hi[a]);
        extent = std::max(extent, (double)m->hi[a] - (double)m->lo[a]);
    }
    float maxabs;
    memcpy(&maxabs, &head.maxabs, 4);
    A.slack = std::ldexp((double)maxabs + extent, -TRIMESH_SLACK_SHIFT);
    m->scale = std::ldexp((float)A.slack, TRIMESH_SLACK_SHIFT);
    const long ntl = (long)head.ntl;
    TreeShape S;
    tree_shape(ntl, leaf, S);
    const size_t nn = S.w3.size();
    m->ntl = ntl; m->nnodes = (long)nn; m->depth = S.depth;
    const size_t ntl1 = (size_t)std::max(ntl, 1l);
    e = hipMalloc(&m->d_nodes, nn * 8 * 4);
    if (e == hipSuccess) e = hipMalloc(&m->d_moments, nn * 16 * 4);
    if (e == hipSuccess) e = hipMalloc(&m->d_tris, ntl1 * 12 * 4);
    if (e == hipSuccess) e = hipMalloc(&m->d_area, ntl1 * 4);
    if (e == hipSuccess) e = launch_tribuild_table(A, s);
    launches += TRIBUILD_TABLE_LAUNCHES;
    if (e != hipSuccess) return fail(0, e);
    float empty[8];  // ntl = 0: the one empty leaf trimesh_build makes
    if (ntl > 0) {
        const int32_t *parts[5] = {S.w3.data(), S.w7.data(), S.first.data(), S.count.data(), S.list.data()};
        const int32_t *dst[5] = {A.w3, A.w7, A.first, A.count, A.list};
        for (int k = 0; k < 5 && e == hipSuccess; ++k)
            e = hipMemcpyAsync(const_cast<int32_t *>(dst[k]), parts[k], nn * 4, hipMemcpyHostToDevice, s);
        A.ntl = (int)ntl; A.nnodes = (int)nn; A.nleaves = S.nleaves; A.depth = S.depth;
        A.level_off = S.level_off.data();
        A.ninner_levels = (int)S.level_off.size() - 1;
        A.nodes = m->d_nodes; A.tris = m->d_tris; A.moments = m->d_moments; A.thresholds = m->d_area;
        if (e == hipSuccess) e = launch_tribuild_tree(A, s);
        launches += tribuild_tree_launches(A);
    } else {
        for (int a = 0; a < 3; ++a) { empty[a] = INFINITY; empty[4 + a] = -INFINITY; }
        empty[3] = 0.0f; empty[7] = 0.0f;
        e = hipMemcpyAsync(m->d_nodes, empty, sizeof empty, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemsetAsync(m->d_moments, 0, 16 * 4, s);
        if (e == hipSuccess) e = hipMemsetAsync(m->d_tris, 0, 12 * 4, s);
        if (e == hipSuccess) e = hipMemsetAsync(m->d_area, 0, 4, s);
    }
    if (e == hipSuccess) e = hipEventRecord(c->ev1, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&head, A.head, sizeof head, hipMemcpyDeviceToHost, s);  // the second record
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(0, e);
    m->closed = head.open ? 0 : 1;
    m->area_last = head.area_last;
    if (stats) {
        nr_stats st{};
        float ms = 0;
        (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
        st.ray_steps = (uint64_t)nt;
        st.launches = launches;
        st.ms_total = ms;
        *stats = st;
    }
    *out = m;
    return NR_OK;
}

int nr_mesh_download(nr_trimesh *m, float *nodes, int32_t *order, float *moments, float *table, uint32_t *thresholds, long *ntl,
                        long *area_last) {
    if (!m) return set_err(nullptr, NR_E_INVALID, "nr_mesh_download: mesh is NULL");
    nr_ctx *c = m->owner;
    if (ntl) *ntl = m->ntl;
    if (area_last) *area_last = m->area_last;
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    const size_t nn = (size_t)m->nnodes, n = (size_t)m->ntl;
    if (nodes) HIPCHK(c, hipMemcpyAsync(nodes, m->d_nodes, nn * 8 * 4, hipMemcpyDeviceToHost, s));
    if (moments) HIPCHK(c, hipMemcpyAsync(moments, m->d_moments, nn * 16 * 4, hipMemcpyDeviceToHost, s));
    if (table) HIPCHK(c, hipMemcpyAsync(table, m->d_table, (size_t)m->nt * 21 * 4, hipMemcpyDeviceToHost, s));
    if (thresholds && n) HIPCHK(c, hipMemcpyAsync(thresholds, m->d_area, n * 4, hipMemcpyDeviceToHost, s));
    std::vector<float> tris;
    if (order && n) {
        tris.resize(n * 12);
        HIPCHK(c, hipMemcpyAsync(tris.data(), m->d_tris, n * 12 * 4, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(c, hipStreamSynchronize(s));
    for (size_t p = 0; p < tris.size() / 12; ++p) memcpy(order + p, &tris[p * 12 + 3], 4);  // word 3 of every position's 12
    return NR_OK;
}

}  // extern "C"

// ---- the mesh's signed distance on a lattice, remeshed (nr_trimesh_grid.hip; mesh_run and sparse_run: nr_api_mesh.hip) ----
// The values are the point calls': k_trimesh_grid_distance and, for the winding sign, the
// k_trimesh_grid_winding launch that signs them in place.  The lattice, the extraction's scratch and
// the staging of a host mesh are the owner context's, as for nr_extract_mesh.

namespace {

struct GridField {
    nr_trimesh *m;
    int sign, brute;
    float beta;
};

int grid_check(nr_ctx *c, const char *fn, int sign, float beta, int flags) {
    if (sign != NR_SAMPLE_SIGN_NORMAL && sign != NR_SAMPLE_SIGN_WINDING) return set_err(c, NR_E_INVALID, "%s: unknown sign %d", fn, sign);
    if (!std::isfinite(beta) || beta < 0.0f) return set_err(c, NR_E_INVALID, "%s: beta = %g is negative or not finite", fn, (double)beta);
    if (flags & ~NR_TRIMESH_BRUTE) return set_err(c, NR_E_INVALID, "%s: unknown flag bits %#x", fn, flags);
    return NR_OK;
}

// the two launches' arguments for values into d_sdf
void grid_args(const GridField &F, float *d_sdf, TriMeshArgs &D, TriWindArgs &W) {
    const nr_trimesh *m = F.m;
    D = TriMeshArgs{};
    D.nodes = m->d_nodes; D.tris = m->d_tris; D.table = m->d_table;
    D.nnodes = (int)m->nnodes; D.ntl = (int)m->ntl;
    D.brute = F.brute;
    D.sdf = d_sdf;
    D.stats = m->d_stats;
    W = TriWindArgs{};
    W.nodes = m->d_nodes; W.tris = m->d_tris; W.moments = m->d_moments;
    W.nnodes = D.nnodes; W.ntl = D.ntl;
    W.brute = F.brute;
    W.beta = F.beta == 0.0f ? 2.0f : F.beta;
    W.sdf = d_sdf;
    W.stats = m->d_stats;
}

int grid_dense(const GridField &F, const LatticeArgs &L, float *d_sdf, hipStream_t s, int *launches) {
    nr_ctx *c = F.m->owner;
    TriMeshArgs D;
    TriWindArgs W;
    grid_args(F, d_sdf, D, W);
    const bool wind = F.sign == NR_SAMPLE_SIGN_WINDING;
    HIPCHK(c, launch_trimesh_lattice(D, wind ? &W : nullptr, L, num_cus(c->device), s));
    *launches += wind ? 2 : 1;
    return NR_OK;
}

// FieldSource::sample
int grid_sparse(void *self, const SparseArgs &A, bool store, hipStream_t s, int *launches) {
    const GridField &F = *static_cast<const GridField *>(self);
    nr_ctx *c = F.m->owner;
    TriMeshArgs D;
    TriWindArgs W;
    grid_args(F, store ? A.store : A.coarse, D, W);
    const bool wind = F.sign == NR_SAMPLE_SIGN_WINDING;
    HIPCHK(c, launch_trimesh_sparse(D, wind ? &W : nullptr, A, store, num_cus(c->device), s));
    *launches += wind ? 2 : 1;
    return NR_OK;
}

// FieldSource::label: source_tri, nr_trimesh_distance's tri of the device vertices by its own launch
int grid_label(void *self, const float *d_vertices, int32_t *d_label, size_t nv, hipStream_t s, int *launches) {
    const GridField &F = *static_cast<const GridField *>(self);
    const nr_trimesh *m = F.m;
    nr_ctx *c = m->owner;
    TriMeshArgs D{};
    D.X = d_vertices; D.n = (long)nv;
    D.nodes = m->d_nodes; D.tris = m->d_tris; D.table = m->d_table;
    D.nnodes = (int)m->nnodes; D.ntl = (int)m->ntl;
    D.tri = d_label;
    D.stats = m->d_stats;
    const size_t chunks = (nv + 63) / 64;
    const int grid = (int)std::max<size_t>(1, std::min<size_t>((chunks + 3) / 4, (size_t)num_cus(c->device) * 8));
    HIPCHK(c, launch_trimesh_distance(D, grid, s));
    *launches += 1;
    return NR_OK;
}

}  // namespace

extern "C" {

int nr_mesh_sample_grid(nr_trimesh *m, const float origin[3], const float step[3], const int dims[3], int sign, float beta,
                           int flags, float *sdf, int loc, nr_stats *stats) {
    const char *fn = "nr_mesh_sample_grid";
    if (!m) return set_err(nullptr, NR_E_INVALID, "%s: mesh is NULL", fn);
    nr_ctx *c = m->owner;
    if (!sdf) return set_err(c, NR_E_INVALID, "%s: sdf is NULL", fn);
    int rc;
    if ((rc = lattice_check(c, fn, origin, step, dims, 1)) != NR_OK) return rc;
    if ((rc = grid_check(c, fn, sign, beta, flags)) != NR_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    const LatticeArgs L = make_lattice(origin, step, dims);
    const size_t N = (size_t)L.n;
    float *d = sdf;
    if (loc != NR_DEVICE) {
        if ((rc = ensure_buf(c, c->d_grid, c->cap_grid, N)) != NR_OK) return rc;
        d = c->d_grid;
    }
    const GridField F{m, sign, (flags & NR_TRIMESH_BRUTE) != 0, beta};
    nr_stats st{};
    int launches = 1;  // the counter's memset
    HIPCHK(c, hipEventRecord(c->ev0, s));
    HIPCHK(c, hipMemsetAsync(m->d_stats, 0, 8, s));
    if ((rc = grid_dense(F, L, d, s, &launches)) != NR_OK) return rc;
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if (loc != NR_DEVICE) HIPCHK(c, hipMemcpyAsync(sdf, d, N * 4, hipMemcpyDeviceToHost, s));
    unsigned long long evals = 0;
    if (stats) HIPCHK(c, hipMemcpyAsync(&evals, m->d_stats, 8, hipMemcpyDeviceToHost, s));
    rc = end_timed(c, stats != nullptr, loc, s, &st.ms_total);
    if (rc != NR_OK || !stats) return rc;
    st.ray_steps = (uint64_t)N;
    st.shade_evals = evals;
    st.launches = launches;
    *stats = st;
    return NR_OK;
}

int nr_mesh_remesh(nr_trimesh *m, const float origin[3], const float step[3], const int dims[3], float iso, int sign,
                      float beta, float *vertices, int32_t *source_tri, long v_cap, int32_t *triangles, long t_cap, long *nv,
                      long *nt, int loc, nr_stats *stats) {
    const char *fn = "nr_mesh_remesh";
    if (!m) return set_err(nullptr, NR_E_INVALID, "%s: mesh is NULL", fn);
    nr_ctx *c = m->owner;
    if (!nv || !nt) return set_err(c, NR_E_INVALID, "%s: NULL nv or nt", fn);
    *nv = 0;
    *nt = 0;
    int rc;
    if ((rc = lattice_check(c, fn, origin, step, dims, 2)) != NR_OK) return rc;
    if ((rc = grid_check(c, fn, sign, beta, 0)) != NR_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    const LatticeArgs L = make_lattice(origin, step, dims);
    if ((rc = ensure_buf(c, c->d_grid, c->cap_grid, (size_t)L.n)) != NR_OK) return rc;
    GridField F{m, sign, 0, beta};
    const FieldSource field{&F, grid_sparse, grid_label};
    int launches = 1;  // the counter's memset
    HIPCHK(c, hipEventRecord(c->ev0, s));
    HIPCHK(c, hipMemsetAsync(m->d_stats, 0, 8, s));
    if ((rc = grid_dense(F, L, c->d_grid, s, &launches)) != NR_OK) return rc;
    rc = mesh_run(c, fn, s, L, c->d_grid, iso, vertices, nullptr, v_cap, triangles, t_cap, nv, nt, loc, &launches, nullptr,
                  vertices && triangles ? source_tri : nullptr, &field);
    if (rc != NR_OK) return rc;
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if (stats) {
        unsigned long long evals = 0;
        HIPCHK(c, hipMemcpyAsync(&evals, m->d_stats, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        nr_stats st{};
        st.ray_steps = (uint64_t)L.n;
        st.rays_shaded = (uint64_t)*nv;
        st.shade_evals = evals;
        st.launches = launches;
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
        st.ms_total = ms;
        *stats = st;
    }
    return NR_OK;
}

int nr_mesh_remesh_sparse(nr_trimesh *m, const float origin[3], const float step[3], const int dims[3], float iso, int sign,
                             float beta, int brick, float band, float *vertices, int32_t *source_tri, int64_t *keys,
                             long v_cap, int32_t *triangles, long t_cap, long *nv, long *nt, long *active_bricks, int loc,
                             nr_stats *stats) {
    const char *fn = "nr_mesh_remesh_sparse";
    if (!m) return set_err(nullptr, NR_E_INVALID, "%s: mesh is NULL", fn);
    nr_ctx *c = m->owner;
    int rc;
    if ((rc = grid_check(c, fn, sign, beta, 0)) != NR_OK) return rc;
    if (source_tri && !vertices) return set_err(c, NR_E_INVALID, "%s: source_tri needs vertices", fn);
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    GridField F{m, sign, 0, beta};
    const FieldSource field{&F, grid_sparse, grid_label};
    HIPCHK(c, hipMemsetAsync(m->d_stats, 0, 8, s));
    SparseDone done;
    rc = sparse_run(c, nullptr, fn, origin, step, dims, iso, brick, band, vertices, nullptr, source_tri, keys, v_cap, triangles,
                    t_cap, nv, nt, active_bricks, loc, stats != nullptr, &done, &field);
    if (rc != NR_OK) return rc;
    if (stats) {
        unsigned long long evals = 0;
        HIPCHK(c, hipMemcpyAsync(&evals, m->d_stats, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        nr_stats st{};
        st.ray_steps = done.points;
        st.rays_hit = done.active;
        st.rays_shaded = (uint64_t)*nv;
        st.shade_evals = evals;
        st.launches = done.launches + 1;  // the counter's memset
        st.ms_total = done.ms;
        *stats = st;
    }
    return NR_OK;
}

}  // extern "C"

// n caller-supplied rays, or with origins == NULL the W x H pixel rays of the owner's view, through
// one k_mesh_rays launch; with `out` the payload is the frame (nr_mesh_render).
static int mesh_rays(nr_trimesh *m, const char *fn, const float *origins, const float *dirs, long n, int W, int H, float tmin,
                     float tmax, int32_t *status, float *t, int32_t *tri, float *bary, float *position, float *normal,
                     uint32_t *out, int flags, int loc, nr_stats *stats) {
    nr_ctx *c = m->owner;
    if (flags & ~(NR_TRIMESH_BRUTE | NR_MESH_RAY_ANY | NR_MESH_RAY_SMOOTH)) return set_err(c, NR_E_INVALID, "%s: unknown flag bits %#x", fn, flags);
    if (flags & NR_MESH_RAY_ANY) {
        if (flags & NR_MESH_RAY_SMOOTH) return set_err(c, NR_E_INVALID, "%s: NR_MESH_RAY_ANY with NR_MESH_RAY_SMOOTH", fn);
        if (t || tri || bary || position || normal || out) return set_err(c, NR_E_INVALID, "%s: NR_MESH_RAY_ANY gives status only", fn);
    }
    if (out && c->color_type == NR_COLOR_MATCAP && !c->d_matcap) return set_err(c, NR_E_STATE, "%s: matcap colouring without a matcap", fn);
    HIPCHK(c, hipSetDevice(c->device));
    GET_STREAM(c, s);
    const size_t N = (size_t)n;
    MeshRayArgs R{};
    R.origins = origins; R.dirs = dirs; R.n = n;
    R.W = W; R.H = H; R.tiles_x = (W + 7) / 8; R.tiles_y = (H + 7) / 8;
    R.rcp_w = pow2_rcp(W); R.rcp_h = pow2_rcp(H);
    memcpy(R.inv_view, c->inv_view, sizeof R.inv_view);
    R.nodes = m->d_nodes; R.tris = m->d_tris; R.table = m->d_table;
    R.nnodes = (int)m->nnodes; R.ntl = (int)m->ntl;
    R.brute = (flags & NR_TRIMESH_BRUTE) != 0;
    R.any = (flags & NR_MESH_RAY_ANY) != 0;
    R.smooth = (flags & NR_MESH_RAY_SMOOTH) != 0;
    R.tmin = tmin; R.tmax = tmax;
    R.scale = m->scale;
    R.status = status; R.t = t; R.tri = tri; R.bary = bary; R.position = position; R.normal = normal;
    R.stats = m->d_stats;
    RenderArgs A{};
    if (out) {
        A = render_args(c, W, H, H, H, 1, 0, 0);
        A.out = out;
        A.frame = c->frame;
        memcpy(A.inv_view, c->inv_view, sizeof A.inv_view);
        memcpy(A.normal, c->normal, sizeof A.normal);
    }
    // staged: the rays, then every output the caller asked for
    Staging io(loc);
    io.in(R.origins, 3 * N); io.in(R.dirs, 3 * N);
    io.out(R.status, N); io.out(R.t, N); io.out(R.tri, N); io.out(R.bary, 3 * N); io.out(R.position, 3 * N);
    io.out(R.normal, 3 * N); io.out(A.out, N);
    int rc;
    if ((rc = io.begin(c, m->d_io, m->cap_io, s)) != NR_OK) return rc;
    // a grid-stride over chunks of 64 rays: at most 8 four-wave workgroups per CU
    const size_t chunks = origins ? (N + 63) / 64 : (size_t)R.tiles_x * (size_t)R.tiles_y;
    const int grid = (int)std::max<size_t>(1, std::min<size_t>((chunks + 3) / 4, (size_t)num_cus(c->device) * 8));
    nr_stats st{};
    HIPCHK(c, hipEventRecord(c->ev0, s));
    HIPCHK(c, hipMemsetAsync(m->d_stats, 0, 16, s));
    HIPCHK(c, launch_mesh_rays(R, out ? &A : nullptr, grid, s));
    HIPCHK(c, hipEventRecord(c->ev1, s));
    if ((rc = io.end(c, s)) != NR_OK) return rc;
    unsigned long long counts[2] = {0, 0};
    if (stats) HIPCHK(c, hipMemcpyAsync(counts, m->d_stats, 16, hipMemcpyDeviceToHost, s));
    rc = end_timed(c, stats != nullptr, loc, s, &st.ms_total);
    if (rc != NR_OK || !stats) return rc;
    st.ray_steps = (uint64_t)n;
    st.shade_evals = counts[0];
    st.rays_hit = counts[1];
    st.launches = 2;  // the counters' memset and k_mesh_rays
    *stats = st;
    return NR_OK;
}

extern "C" {

int nr_mesh_trace_rays(nr_trimesh *m, const float *origins, const float *dirs, long n, float tmin, float tmax, int32_t *status,
                       float *t, int32_t *tri, float *bary, float *position, float *normal, int flags, int loc,
                       nr_stats *stats) {
    if (!m) return set_err(nullptr, NR_E_INVALID, "nr_mesh_trace_rays: mesh is NULL");
    nr_ctx *c = m->owner;
    if (!origins || !dirs) return set_err(c, NR_E_INVALID, "nr_mesh_trace_rays: NULL rays");
    if (n < 1 || n > (1l << 30)) return set_err(c, NR_E_INVALID, "nr_mesh_trace_rays: n = %ld outside [1, 2^30]", n);
    if (!(tmin <= tmax)) return set_err(c, NR_E_INVALID, "nr_mesh_trace_rays: tmin = %g, tmax = %g: a NaN, or tmin > tmax", (double)tmin, (double)tmax);
    return mesh_rays(m, "nr_mesh_trace_rays", origins, dirs, n, 1, 1, tmin, tmax, status, t, tri, bary, position, normal, nullptr,
                     flags, loc, stats);
}

int nr_mesh_gbuffer(nr_trimesh *m, int W, int H, int32_t *status, float *t, int32_t *tri, float *bary, float *position,
                    float *normal, int flags, int loc, nr_stats *stats) {
    if (!m) return set_err(nullptr, NR_E_INVALID, "nr_mesh_gbuffer: mesh is NULL");
    nr_ctx *c = m->owner;
    if (W < 1 || H < 1 || (long)W * H > (1l << 30)) return set_err(c, NR_E_INVALID, "nr_mesh_gbuffer: bad size %dx%d", W, H);
    return mesh_rays(m, "nr_mesh_gbuffer", nullptr, nullptr, (long)W * H, W, H, 0.0f, INFINITY, status, t, tri, bary, position,
                     normal, nullptr, flags, loc, stats);
}

int nr_mesh_render(nr_trimesh *m, uint32_t *out, int W, int H, int flags, int out_loc, nr_stats *stats) {
    if (!m) return set_err(nullptr, NR_E_INVALID, "nr_mesh_render: mesh is NULL");
    nr_ctx *c = m->owner;
    if (!out) return set_err(c, NR_E_INVALID, "nr_mesh_render: out is NULL");
    if (W < 1 || H < 1 || (long)W * H > (1l << 30)) return set_err(c, NR_E_INVALID, "nr_mesh_render: bad size %dx%d", W, H);
    return mesh_rays(m, "nr_mesh_render", nullptr, nullptr, (long)W * H, W, H, 0.0f, INFINITY, nullptr, nullptr, nullptr, nullptr,
                     nullptr, nullptr, out, flags, out_loc, stats);
}

}  // extern "C"
