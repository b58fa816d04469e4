// nr_trimesh_host.cpp -- the host side of the triangle-mesh queries (nr_trimesh_*): the OBJ reader
// (nr_obj_load), the pseudonormal table (nr_trimesh_normals) and the hierarchy k_trimesh_distance
// and k_trimesh_winding walk, with the far-field moments of every node (trimesh_build;
// nr_mesh_hierarchy returns it), and the area table nr_mesh_sample picks triangles from
// (trimesh_area_table; nr_mesh_area_table returns it).  No GPU and no HIP here: tests/cpp/trimesh_sanitize.cpp links
// this file alone.  The contract is in include/neural_render.h; tests/trimesh_ref.py and
// tests/winding_ref.py restate it in numpy.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>

#include "nr_internal.h"

namespace nr {

// ---- OBJ ----

namespace {
const char *skip_blank(const char *p, const char *e) {
    while (p < e && (*p == ' ' || *p == '\t' || *p == '\r')) ++p;
    return p;
}
const char *line_end(const char *p, const char *e) {
    while (p < e && *p != '\n') ++p;
    return p;
}
// a decimal integer of at most 18 digits at [p, e); false if there is none
bool read_long(const char *&p, const char *e, long &v) {
    const char *q = p;
    bool neg = false;
    if (q < e && (*q == '-' || *q == '+')) { neg = *q == '-'; ++q; }
    const char *d0 = q;
    long a = 0;
    while (q < e && *q >= '0' && *q <= '9' && q - d0 < 18) { a = a * 10 + (*q - '0'); ++q; }
    if (q == d0 || (q < e && *q >= '0' && *q <= '9')) return false;
    v = neg ? -a : a;
    p = q;
    return true;
}
}  // namespace

int obj_parse(const char *path, std::vector<float> &V, std::vector<int32_t> &T, std::string &err) {
    V.clear(); T.clear();
    FILE *f = fopen(path, "rb");
    if (!f) { err = std::string("cannot open ") + path; return NR_E_IO; }
    std::vector<char> buf;
    {
        char chunk[65536];
        size_t got;
        while ((got = fread(chunk, 1, sizeof chunk, f)) > 0) buf.insert(buf.end(), chunk, chunk + got);
        const bool bad = ferror(f) != 0;
        fclose(f);
        if (bad) { err = std::string("cannot read ") + path; return NR_E_IO; }
    }
    buf.push_back('\n');
    buf.push_back('\0');  // (strtof stops here at the latest)
    const char *p = buf.data(), *const end = buf.data() + buf.size() - 1;
    std::vector<long> face;   // a face's corners as written (1-based, or negative), then resolved
    std::vector<long> raw;    // every triangle's resolved 0-based corners (checked against nv at the end)
    long line = 0;
    char msg[160];
    while (p < end) {
        ++line;
        const char *le = line_end(p, end);
        const char *q = skip_blank(p, le);
        const bool is_v = le - q >= 2 && q[0] == 'v' && (q[1] == ' ' || q[1] == '\t');
        const bool is_f = le - q >= 2 && q[0] == 'f' && (q[1] == ' ' || q[1] == '\t');
        if (is_v) {
            q += 2;
            float xyz[3];
            for (int a = 0; a < 3; ++a) {
                q = skip_blank(q, le);
                char *stop = nullptr;
                xyz[a] = q < le ? strtof(q, &stop) : 0.0f;
                if (q >= le || stop == q || stop > le) {
                    snprintf(msg, sizeof msg, "line %ld: a vertex needs three numbers", line);
                    err = msg;
                    return NR_E_FORMAT;
                }
                q = stop;
            }
            V.insert(V.end(), xyz, xyz + 3);
        } else if (is_f) {
            q += 2;
            face.clear();
            const long nv_now = (long)(V.size() / 3);
            while (true) {
                q = skip_blank(q, le);
                if (q >= le) break;
                long i = 0;
                if (!read_long(q, le, i) || i == 0) {
                    snprintf(msg, sizeof msg, "line %ld: a face corner is no vertex index", line);
                    err = msg;
                    return NR_E_FORMAT;
                }
                if (i < 0) {
                    i = nv_now + i;  // relative to the vertices read so far
                    if (i < 0) {
                        snprintf(msg, sizeof msg, "line %ld: a relative index reaches before the first vertex", line);
                        err = msg;
                        return NR_E_FORMAT;
                    }
                } else {
                    i -= 1;
                }
                face.push_back(i);
                while (q < le && *q != ' ' && *q != '\t' && *q != '\r') ++q;  // /t, //n, /t/n
            }
            if (face.size() < 3) {
                snprintf(msg, sizeof msg, "line %ld: a face of %zu corners", line, face.size());
                err = msg;
                return NR_E_FORMAT;
            }
            for (size_t k = 1; k + 1 < face.size(); ++k) {
                raw.push_back(face[0]); raw.push_back(face[k]); raw.push_back(face[k + 1]);
            }
        }
        p = le + 1;
    }
    const long nv = (long)(V.size() / 3);
    if (nv > (long)std::numeric_limits<int32_t>::max()) { err = "more than 2^31 - 1 vertices"; return NR_E_FORMAT; }
    T.resize(raw.size());
    for (size_t k = 0; k < raw.size(); ++k) {
        if (raw[k] >= nv) {
            snprintf(msg, sizeof msg, "a face names vertex %ld of %ld", raw[k] + 1, nv);
            err = msg;
            return NR_E_FORMAT;
        }
        T[k] = (int32_t)raw[k];
    }
    return NR_OK;
}

// ---- pseudonormals ----

namespace {
struct D3 { double x, y, z; };
inline D3 sub(const float *a, const float *b) { return {(double)a[0] - (double)b[0], (double)a[1] - (double)b[1], (double)a[2] - (double)b[2]}; }
inline D3 cross(D3 u, D3 v) { return {u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x}; }
inline double dot(D3 u, D3 v) { return u.x * v.x + u.y * v.y + u.z * v.z; }
inline double len(D3 u) { return std::sqrt(dot(u, u)); }

struct EdgeUse { uint64_t key; int32_t tri; int8_t slot, fwd; };  // key: (min vertex, max vertex)
struct CornerUse { int32_t vert, tri; int8_t corner; };
}  // namespace

bool trimesh_indices_ok(const int32_t *T, long nt, long nv) {
    for (long k = 0; k < 3 * nt; ++k)
        if (T[k] < 0 || (long)T[k] >= nv) return false;
    return true;
}

void trimesh_normals(const float *V, long nv, const int32_t *T, long nt, float *table, int *closed) {
    (void)nv;
    // face normals, normalised; a zero-area triangle: 0
    std::vector<D3> fn((size_t)nt);
    for (long t = 0; t < nt; ++t) {
        const float *a = V + 3 * (size_t)T[3 * t], *b = V + 3 * (size_t)T[3 * t + 1], *c = V + 3 * (size_t)T[3 * t + 2];
        const D3 n = cross(sub(b, a), sub(c, a));
        const double l = len(n);
        fn[t] = l > 0.0 && std::isfinite(l) ? D3{n.x / l, n.y / l, n.z / l} : D3{0.0, 0.0, 0.0};
    }
    // edges: the uses of every undirected edge, ascending triangle index
    std::vector<EdgeUse> eu((size_t)nt * 3);
    for (long t = 0; t < nt; ++t)
        for (int s = 0; s < 3; ++s) {
            const uint32_t i = (uint32_t)T[3 * t + s], j = (uint32_t)T[3 * t + (s + 1) % 3];
            const uint64_t key = i < j ? ((uint64_t)i << 32) | j : ((uint64_t)j << 32) | i;
            eu[(size_t)t * 3 + s] = {key, (int32_t)t, (int8_t)s, (int8_t)(i < j)};
        }
    std::sort(eu.begin(), eu.end(), [](const EdgeUse &a, const EdgeUse &b) {
        return a.key != b.key ? a.key < b.key : (a.tri != b.tri ? a.tri < b.tri : a.slot < b.slot);
    });
    bool is_closed = true;
    for (size_t g0 = 0; g0 < eu.size();) {
        size_t g1 = g0;
        D3 s{0.0, 0.0, 0.0};
        while (g1 < eu.size() && eu[g1].key == eu[g0].key) {
            const D3 n = fn[eu[g1].tri];
            s = {s.x + n.x, s.y + n.y, s.z + n.z};
            ++g1;
        }
        if (g1 - g0 != 2 || eu[g0].fwd == eu[g0 + 1].fwd || (eu[g0].key >> 32) == (eu[g0].key & 0xffffffffu)) is_closed = false;
        if (table)
            for (size_t k = g0; k < g1; ++k) {
                float *o = table + ((size_t)eu[k].tri * 7 + 1 + eu[k].slot) * 3;
                o[0] = (float)s.x; o[1] = (float)s.y; o[2] = (float)s.z;
            }
        g0 = g1;
    }
    if (closed) *closed = is_closed ? 1 : 0;
    if (!table) return;
    for (long t = 0; t < nt; ++t) {
        float *o = table + (size_t)t * 21;
        o[0] = (float)fn[t].x; o[1] = (float)fn[t].y; o[2] = (float)fn[t].z;
    }
    // vertices: angle-weighted, ascending triangle index
    std::vector<CornerUse> cu((size_t)nt * 3);
    for (long t = 0; t < nt; ++t)
        for (int s = 0; s < 3; ++s) cu[(size_t)t * 3 + s] = {T[3 * t + s], (int32_t)t, (int8_t)s};
    std::sort(cu.begin(), cu.end(), [](const CornerUse &a, const CornerUse &b) {
        return a.vert != b.vert ? a.vert < b.vert : (a.tri != b.tri ? a.tri < b.tri : a.corner < b.corner);
    });
    for (size_t g0 = 0; g0 < cu.size();) {
        size_t g1 = g0;
        D3 s{0.0, 0.0, 0.0};
        while (g1 < cu.size() && cu[g1].vert == cu[g0].vert) {
            const long t = cu[g1].tri;
            const int c = cu[g1].corner;
            const D3 n = fn[t];
            if (n.x != 0.0 || n.y != 0.0 || n.z != 0.0) {
                const float *o = V + 3 * (size_t)T[3 * t + c];
                const D3 u = sub(V + 3 * (size_t)T[3 * t + (c + 1) % 3], o), v = sub(V + 3 * (size_t)T[3 * t + (c + 2) % 3], o);
                const double ang = std::atan2(len(cross(u, v)), dot(u, v));
                s = {s.x + ang * n.x, s.y + ang * n.y, s.z + ang * n.z};
            }
            ++g1;
        }
        for (size_t k = g0; k < g1; ++k) {
            float *o = table + ((size_t)cu[k].tri * 7 + 4 + cu[k].corner) * 3;
            o[0] = (float)s.x; o[1] = (float)s.y; o[2] = (float)s.z;
        }
        g0 = g1;
    }
}

// ---- hierarchy ----

namespace {
struct Builder {
    const float *V;
    const int32_t *T;
    int leaf;
    std::vector<int32_t> order;     // the live triangles, reordered in place
    std::vector<double> cen;        // [nt][3] centroids
    std::vector<float> nodes;       // 8 words per node
    double slack;
    int depth = 0;

    static void put_int(float *w, int32_t v) { memcpy(w, &v, 4); }

    // the node of order[first, first + count): returns its index
    int32_t build(long first, long count, int level) {
        depth = std::max(depth, level);
        const int32_t me = (int32_t)(nodes.size() / 8);
        nodes.resize(nodes.size() + 8);
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        double clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (long k = first; k < first + count; ++k) {
            const long t = order[(size_t)k];
            for (int c = 0; c < 3; ++c) {
                const float *p = V + 3 * (size_t)T[3 * t + c];
                for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], p[a]); hi[a] = std::max(hi[a], p[a]); }
            }
            for (int a = 0; a < 3; ++a) {
                clo[a] = std::min(clo[a], cen[(size_t)t * 3 + a]);
                chi[a] = std::max(chi[a], cen[(size_t)t * 3 + a]);
            }
        }
        // inflated, rounded outward
        for (int a = 0; a < 3; ++a) {
            float l = (float)((double)lo[a] - slack), h = (float)((double)hi[a] + slack);
            if ((double)l > (double)lo[a] - slack) l = std::nextafterf(l, -INFINITY);
            if ((double)h < (double)hi[a] + slack) h = std::nextafterf(h, INFINITY);
            nodes[(size_t)me * 8 + a] = l;
            nodes[(size_t)me * 8 + 4 + a] = h;
        }
        if (count <= leaf) {
            put_int(&nodes[(size_t)me * 8 + 3], (int32_t)first);
            put_int(&nodes[(size_t)me * 8 + 7], (int32_t)-count);
            return me;
        }
        int axis = 0;
        for (int a = 1; a < 3; ++a)
            if (chi[a] - clo[a] > chi[axis] - clo[axis]) axis = a;
        const long half = (count + 1) / 2;
        auto less = [&](int32_t x, int32_t y) {
            const double cx = cen[(size_t)x * 3 + axis], cy = cen[(size_t)y * 3 + axis];
            return cx != cy ? cx < cy : x < y;
        };
        std::nth_element(order.begin() + first, order.begin() + first + half, order.begin() + first + count, less);
        const int32_t l = build(first, half, level + 1);
        const int32_t r = build(first + half, count - half, level + 1);
        put_int(&nodes[(size_t)me * 8 + 3], l);
        put_int(&nodes[(size_t)me * 8 + 7], r);
        return me;
    }
};

// The far-field record of every node of H (the header's "moments"): sums in double over the node's
// triangles in position order, each entry rounded to f32 once.  The centre is rounded first and S and
// R2 are taken about the rounded centre, the one k_trimesh_winding expands about.
void trimesh_moments(TriBvh &H) {
    const long nn = H.nnodes, ntl = H.ntl;
    H.moments.assign((size_t)nn * 16, 0.0f);
    std::vector<double> q((size_t)ntl * 7);  // per position: A.xyz, |A|, x.xyz
    for (long k = 0; k < ntl; ++k) {
        const float *t = H.tris.data() + (size_t)k * 12;
        const D3 A = cross(sub(t + 4, t), sub(t + 8, t));
        double *o = q.data() + (size_t)k * 7;
        o[0] = 0.5 * A.x; o[1] = 0.5 * A.y; o[2] = 0.5 * A.z;
        o[3] = std::sqrt((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]);
        for (int a = 0; a < 3; ++a) o[4 + a] = (((double)t[a] + (double)t[4 + a]) + (double)t[8 + a]) / 3.0;
    }
    // a node's triangles [first, first + count): children follow their parent in preorder
    std::vector<int32_t> first((size_t)nn), count((size_t)nn);
    for (long i = nn - 1; i >= 0; --i) {
        int32_t w3, w7;
        memcpy(&w3, &H.nodes[(size_t)i * 8 + 3], 4);
        memcpy(&w7, &H.nodes[(size_t)i * 8 + 7], 4);
        if (w7 <= 0) { first[(size_t)i] = w3; count[(size_t)i] = -w7; }
        else { first[(size_t)i] = first[(size_t)w3]; count[(size_t)i] = count[(size_t)w3] + count[(size_t)w7]; }
    }
    for (long i = 0; i < nn; ++i) {
        const long k0 = first[(size_t)i], k1 = k0 + count[(size_t)i];
        if (k1 == k0) continue;
        double sa = 0.0, sx[3] = {0.0, 0.0, 0.0}, mx[3] = {0.0, 0.0, 0.0}, N[3] = {0.0, 0.0, 0.0};
        for (long k = k0; k < k1; ++k) {
            const double *o = q.data() + (size_t)k * 7;
            sa += o[3];
            for (int a = 0; a < 3; ++a) { sx[a] += o[3] * o[4 + a]; mx[a] += o[4 + a]; N[a] += o[a]; }
        }
        float *rec = H.moments.data() + (size_t)i * 16;
        double c[3];
        for (int a = 0; a < 3; ++a) {
            rec[a] = (float)(sa > 0.0 ? sx[a] / sa : mx[a] / (double)(k1 - k0));
            c[a] = (double)rec[a];
            rec[4 + a] = (float)N[a];
        }
        double M[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, r2 = 0.0;
        for (long k = k0; k < k1; ++k) {
            const double *o = q.data() + (size_t)k * 7;
            const double d[3] = {o[4] - c[0], o[5] - c[1], o[6] - c[2]};
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) M[a][b] += o[a] * d[b];
            const float *t = H.tris.data() + (size_t)k * 12;
            for (int v = 0; v < 3; ++v) {
                const double e0 = (double)t[4 * v] - c[0], e1 = (double)t[4 * v + 1] - c[1], e2 = (double)t[4 * v + 2] - c[2];
                r2 = std::max(r2, (e0 * e0 + e1 * e1) + e2 * e2);
            }
        }
        float R2 = (float)r2;
        if ((double)R2 < r2) R2 = std::nextafterf(R2, INFINITY);
        rec[3] = R2;
        rec[8] = (float)M[0][0]; rec[9] = (float)M[1][1]; rec[10] = (float)M[2][2];
        rec[11] = (float)(0.5 * (M[0][1] + M[1][0]));
        rec[12] = (float)(0.5 * (M[0][2] + M[2][0]));
        rec[13] = (float)(0.5 * (M[1][2] + M[2][1]));
    }
}
}  // namespace

bool trimesh_build(const float *V, long nv, const int32_t *T, long nt, int leaf, const float *table, TriBvh &out) {
    out = TriBvh{};
    Builder B{};
    B.V = V; B.T = T; B.leaf = leaf;
    double maxabs = 0.0;
    for (int a = 0; a < 3; ++a) { out.lo[a] = INFINITY; out.hi[a] = -INFINITY; }
    for (long i = 0; i < nv; ++i)
        for (int a = 0; a < 3; ++a) {
            const float v = V[3 * (size_t)i + a];
            out.lo[a] = std::min(out.lo[a], v);
            out.hi[a] = std::max(out.hi[a], v);
            maxabs = std::max(maxabs, std::fabs((double)v));
        }
    double extent = 0.0;
    for (int a = 0; a < 3; ++a) extent = std::max(extent, (double)out.hi[a] - (double)out.lo[a]);
    B.slack = std::ldexp(maxabs + extent, -TRIMESH_SLACK_SHIFT);
    out.slack = (float)B.slack;
    B.cen.resize((size_t)nt * 3);
    for (long t = 0; t < nt; ++t) {
        const float *n = table + (size_t)t * 21;
        for (int a = 0; a < 3; ++a)
            B.cen[(size_t)t * 3 + a] =
                ((double)V[3 * (size_t)T[3 * t] + a] + (double)V[3 * (size_t)T[3 * t + 1] + a] + (double)V[3 * (size_t)T[3 * t + 2] + a]) / 3.0;
        // a zero-area triangle takes no part (its distance is NaN by definition)
        if (n[0] != 0.0f || n[1] != 0.0f || n[2] != 0.0f) B.order.push_back((int32_t)t);
    }
    const long ntl = (long)B.order.size();
    B.nodes.reserve((size_t)(ntl / std::max(leaf, 1) + 1) * 16);
    B.build(0, ntl, 1);
    out.depth = B.depth;
    out.ntl = ntl;
    out.nnodes = (long)(B.nodes.size() / 8);
    out.nodes.swap(B.nodes);
    out.tris.assign((size_t)std::max(ntl, 1l) * 12, 0.0f);
    for (long k = 0; k < ntl; ++k) {
        const int32_t t = B.order[(size_t)k];
        float *o = out.tris.data() + (size_t)k * 12;
        for (int c = 0; c < 3; ++c)
            for (int a = 0; a < 3; ++a) o[4 * c + a] = V[3 * (size_t)T[3 * t + c] + a];
        memcpy(o + 3, &t, 4);
    }
    trimesh_moments(out);
    // ceil(log2 ntl) + 1 levels at most
    int bound = 1;
    while ((1l << (bound - 1)) < std::max(ntl, 1l)) ++bound;
    return out.depth <= bound && out.depth <= TRIMESH_STACK;
}

long trimesh_area_table(const TriBvh &H, std::vector<uint32_t> &thresholds) {
    const long ntl = H.ntl;
    thresholds.assign((size_t)ntl, 0u);
    std::vector<double> C((size_t)ntl);
    double sum = 0.0;
    for (long k = 0; k < ntl; ++k) {
        // |A_p| as trimesh_moments forms it
        const float *t = H.tris.data() + (size_t)k * 12;
        const D3 A = cross(sub(t + 4, t), sub(t + 8, t));
        const double x = 0.5 * A.x, y = 0.5 * A.y, z = 0.5 * A.z;
        sum += std::sqrt((x * x + y * y) + z * z);
        C[(size_t)k] = sum;
    }
    if (!(sum > 0.0) || !std::isfinite(sum)) return -1;
    long last = -1;
    uint32_t prev = 0;
    for (long k = 0; k < ntl; ++k) {
        const double f = std::floor(C[(size_t)k] / sum * 4294967296.0);
        const uint32_t T = f >= 4294967295.0 ? 0xffffffffu : (uint32_t)f;
        thresholds[(size_t)k] = T;
        if (T > prev) last = k;
        prev = T;
    }
    return last;
}

}  // namespace nr

// ---- C ABI (host only) ----

extern "C" {

int nr_obj_load(const char *path, float **vertices, long *nv, int32_t **triangles, long *nt) {
    if (vertices) *vertices = nullptr;
    if (triangles) *triangles = nullptr;
    if (nv) *nv = 0;
    if (nt) *nt = 0;
    if (!path || !vertices || !nv || !triangles || !nt) return nr::report_error(NR_E_INVALID, "nr_obj_load: NULL argument");
    std::vector<float> V;
    std::vector<int32_t> T;
    std::string err;
    const int rc = nr::obj_parse(path, V, T, err);
    if (rc != NR_OK) return nr::report_error(rc, "nr_obj_load: %s", err.c_str());
    float *v = (float *)malloc(std::max<size_t>(V.size(), 1) * 4);
    int32_t *t = (int32_t *)malloc(std::max<size_t>(T.size(), 1) * 4);
    if (!v || !t) { free(v); free(t); return nr::report_error(NR_E_NOMEM, "nr_obj_load: out of host memory"); }
    if (!V.empty()) memcpy(v, V.data(), V.size() * 4);
    if (!T.empty()) memcpy(t, T.data(), T.size() * 4);
    *vertices = v; *nv = (long)(V.size() / 3);
    *triangles = t; *nt = (long)(T.size() / 3);
    return NR_OK;
}

int nr_trimesh_normals(const float *vertices, long nv, const int32_t *triangles, long nt, float *table, int *closed) {
    if (!vertices || !triangles || (!table && !closed)) return nr::report_error(NR_E_INVALID, "nr_trimesh_normals: NULL argument");
    if (nv < 1 || nt < 1 || nt > (1l << 24)) return nr::report_error(NR_E_INVALID, "nr_trimesh_normals: nv = %ld or nt = %ld out of range", nv, nt);
    if (!nr::trimesh_indices_ok(triangles, nt, nv)) return nr::report_error(NR_E_INVALID, "nr_trimesh_normals: a vertex index outside 0..%ld", nv - 1);
    nr::trimesh_normals(vertices, nv, triangles, nt, table, closed);
    return NR_OK;
}

int nr_mesh_hierarchy(const float *vertices, long nv, const int32_t *triangles, long nt, int leaf, float **nodes,
                      long *nnodes, int32_t **order, long *ntl, float **moments, int *depth) {
    if (nodes) *nodes = nullptr;
    if (order) *order = nullptr;
    if (moments) *moments = nullptr;
    if (nnodes) *nnodes = 0;
    if (ntl) *ntl = 0;
    if (depth) *depth = 0;
    if (!vertices || !triangles || !nodes || !nnodes || !order || !ntl || !moments || !depth)
        return nr::report_error(NR_E_INVALID, "nr_mesh_hierarchy: NULL argument");
    if (nv < 1 || nv > (long)std::numeric_limits<int32_t>::max() || nt < 1 || nt > (1l << 24))
        return nr::report_error(NR_E_INVALID, "nr_mesh_hierarchy: nv = %ld or nt = %ld out of range", nv, nt);
    if (leaf < 0 || leaf > 32) return nr::report_error(NR_E_INVALID, "nr_mesh_hierarchy: leaf = %d outside 0..32", leaf);
    if (!nr::trimesh_indices_ok(triangles, nt, nv)) return nr::report_error(NR_E_INVALID, "nr_mesh_hierarchy: a vertex index outside 0..%ld", nv - 1);
    for (long i = 0; i < 3 * nv; ++i)
        if (!std::isfinite(vertices[i])) return nr::report_error(NR_E_INVALID, "nr_mesh_hierarchy: vertex %ld is not finite", i / 3);
    std::vector<float> table((size_t)nt * 21);
    nr::trimesh_normals(vertices, nv, triangles, nt, table.data(), nullptr);
    nr::TriBvh H;
    if (!nr::trimesh_build(vertices, nv, triangles, nt, leaf > 0 ? leaf : nr::TRIMESH_LEAF_DEFAULT, table.data(), H))
        return nr::report_error(NR_E_INVALID, "nr_mesh_hierarchy: a hierarchy of %d levels (the walk's stack holds %d)", H.depth, nr::TRIMESH_STACK);
    float *n = (float *)malloc(H.nodes.size() * 4), *m = (float *)malloc(H.moments.size() * 4);
    int32_t *o = (int32_t *)malloc(std::max<size_t>((size_t)H.ntl, 1) * 4);
    if (!n || !m || !o) { free(n); free(m); free(o); return nr::report_error(NR_E_NOMEM, "nr_mesh_hierarchy: out of host memory"); }
    memcpy(n, H.nodes.data(), H.nodes.size() * 4);
    memcpy(m, H.moments.data(), H.moments.size() * 4);
    for (long k = 0; k < H.ntl; ++k) memcpy(o + k, &H.tris[(size_t)k * 12 + 3], 4);
    *nodes = n; *nnodes = H.nnodes;
    *order = o; *ntl = H.ntl;
    *moments = m; *depth = H.depth;
    return NR_OK;
}

int nr_mesh_area_table(const float *vertices, long nv, const int32_t *triangles, long nt, int leaf, uint32_t **thresholds,
                       long *ntl, long *last) {
    if (thresholds) *thresholds = nullptr;
    if (ntl) *ntl = 0;
    if (last) *last = -1;
    if (!vertices || !triangles || !thresholds || !ntl || !last) return nr::report_error(NR_E_INVALID, "nr_mesh_area_table: NULL argument");
    if (nv < 1 || nv > (long)std::numeric_limits<int32_t>::max() || nt < 1 || nt > (1l << 24))
        return nr::report_error(NR_E_INVALID, "nr_mesh_area_table: nv = %ld or nt = %ld out of range", nv, nt);
    if (leaf < 0 || leaf > 32) return nr::report_error(NR_E_INVALID, "nr_mesh_area_table: leaf = %d outside 0..32", leaf);
    if (!nr::trimesh_indices_ok(triangles, nt, nv)) return nr::report_error(NR_E_INVALID, "nr_mesh_area_table: a vertex index outside 0..%ld", nv - 1);
    for (long i = 0; i < 3 * nv; ++i)
        if (!std::isfinite(vertices[i])) return nr::report_error(NR_E_INVALID, "nr_mesh_area_table: vertex %ld is not finite", i / 3);
    std::vector<float> table((size_t)nt * 21);
    nr::trimesh_normals(vertices, nv, triangles, nt, table.data(), nullptr);
    nr::TriBvh H;
    if (!nr::trimesh_build(vertices, nv, triangles, nt, leaf > 0 ? leaf : nr::TRIMESH_LEAF_DEFAULT, table.data(), H))
        return nr::report_error(NR_E_INVALID, "nr_mesh_area_table: a hierarchy of %d levels (the walk's stack holds %d)", H.depth, nr::TRIMESH_STACK);
    std::vector<uint32_t> T;
    const long l = nr::trimesh_area_table(H, T);
    uint32_t *o = (uint32_t *)malloc(std::max<size_t>(T.size(), 1) * 4);
    if (!o) return nr::report_error(NR_E_NOMEM, "nr_mesh_area_table: out of host memory");
    if (!T.empty()) memcpy(o, T.data(), T.size() * 4);
    *thresholds = o; *ntl = H.ntl; *last = l;
    return NR_OK;
}

}  // extern "C"
