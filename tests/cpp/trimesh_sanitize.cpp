// trimesh_sanitize.cpp -- host-side driver for an AddressSanitizer / UndefinedBehaviorSanitizer build
// of the triangle-mesh host code (csrc/nr_trimesh_host.cpp: the OBJ reader, the pseudonormal table and
// the hierarchy builder), which indexes arrays by what a file says.  No GPU and no HIP:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off \
//       -Iinclude -Icudaneuralrender_amd/csrc tests/cpp/trimesh_sanitize.cpp \
//       cudaneuralrender_amd/csrc/nr_trimesh_host.cpp -o build/trimesh_sanitize
//   build/trimesh_sanitize FILE.obj...
//
// Every file is read by nr_obj_load; a malformed one must fail with a code, never touch memory it does
// not own.  A mesh that loads gets its table (nr_trimesh_normals) and, at leaf sizes 1, 3, 8 and 32,
// its hierarchy, whose invariants are checked: every triangle with a face normal in exactly one leaf,
// every box around its triangles and its children, the depth within ceil(log2 n) + 1.  Then the walk
// k_trimesh_distance makes (64 points sharing one stack, restated here on the host in the header's
// f32 chains) is compared with brute force on points around the mesh: the same winner, bit for bit.
// Prints "ok N failed M"; the sanitizers abort on the first finding (exit status != 0).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "nr_internal.h"

// nr_api.hip is not part of this build: its error recorder, as a plain formatter
int nr::report_error(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return code;
}

namespace {

struct V3 { float x, y, z; };
V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
float dot(V3 u, V3 v) { return fmaf(u.z, v.z, fmaf(u.y, v.y, u.x * v.x)); }
V3 fma3(V3 e, float t, V3 b) { return {fmaf(e.x, t, b.x), fmaf(e.y, t, b.y), fmaf(e.z, t, b.z)}; }

// step 1 of the header
float tri_d2(V3 p, V3 a, V3 b, V3 c) {
    const V3 ab = sub(b, a), ac = sub(c, a), bc = sub(c, b), ap = sub(p, a), bp = sub(p, b), cp = sub(p, c);
    const float d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4, e43 = d4 - d3, e56 = d5 - d6;
    V3 q;
    if (d1 <= 0 && d2 <= 0) q = a;
    else if (d3 >= 0 && d4 <= d3) q = b;
    else if (vc <= 0 && d1 >= 0 && d3 <= 0) q = fma3(ab, d1 / (d1 - d3), a);
    else if (d6 >= 0 && d5 <= d6) q = c;
    else if (vb <= 0 && d2 >= 0 && d6 <= 0) q = fma3(ac, d2 / (d2 - d6), a);
    else if (va <= 0 && e43 >= 0 && e56 >= 0) q = fma3(bc, e43 / (e43 + e56), b);
    else {
        const float den = (va + vb) + vc;
        q = fma3(ac, vc / den, fma3(ab, vb / den, a));
    }
    const V3 d = sub(p, q);
    return dot(d, d);
}

int word(const float *w) { int v; memcpy(&v, w, 4); return v; }

float box_bound(V3 p, const float *n) {
    const float dx = fmaxf(fmaxf(n[0] - p.x, p.x - n[4]), 0.0f), dy = fmaxf(fmaxf(n[1] - p.y, p.y - n[5]), 0.0f),
                dz = fmaxf(fmaxf(n[2] - p.z, p.z - n[6]), 0.0f);
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx)) * 0.9999847412109375f;
}

struct Best { float d2 = INFINITY; int idx = 0x7fffffff; };

void eval(const nr::TriBvh &H, long t, const std::vector<V3> &P, std::vector<Best> &best) {
    const float *q = H.tris.data() + (size_t)t * 12;
    const V3 a{q[0], q[1], q[2]}, b{q[4], q[5], q[6]}, c{q[8], q[9], q[10]};
    const int oi = word(q + 3);
    for (size_t l = 0; l < P.size(); ++l) {
        const float d2 = tri_d2(P[l], a, b, c);
        if (d2 < best[l].d2 || (d2 == best[l].d2 && oi < best[l].idx)) best[l] = {d2, oi};
    }
}

// the kernel's walk for the points of one wave; returns the triangle evaluations per point
long walk(const nr::TriBvh &H, const std::vector<V3> &P, std::vector<Best> &best) {
    auto wanted = [&](const float *n) {
        for (size_t l = 0; l < P.size(); ++l)
            if (!(box_bound(P[l], n) > best[l].d2)) return true;
        return false;
    };
    int stack[nr::TRIMESH_STACK], sp = 0, node = 0;
    long evals = 0;
    for (long entered = 0; entered < H.nnodes; ++entered) {
        const float *n = H.nodes.data() + (size_t)node * 8;
        const int w3 = word(n + 3), w7 = word(n + 7);
        if (w7 <= 0) {
            for (long t = w3; t < (long)w3 - w7; ++t) eval(H, t, P, best);
            evals += -w7;
            node = -1;
        } else {
            const float *nl = H.nodes.data() + (size_t)w3 * 8, *nr_ = H.nodes.data() + (size_t)w7 * 8;
            size_t nearer = 0;
            for (size_t l = 0; l < P.size(); ++l) nearer += box_bound(P[l], nl) <= box_bound(P[l], nr_);
            const bool left_near = 2 * nearer >= P.size();
            const int near = left_near ? w3 : w7, far = left_near ? w7 : w3;
            const bool want_near = wanted(left_near ? nl : nr_), want_far = wanted(left_near ? nr_ : nl);
            if (want_near) {
                node = near;
                if (want_far) {
                    if (sp >= nr::TRIMESH_STACK) { fprintf(stderr, "stack overflow\n"); exit(1); }
                    stack[sp++] = far;
                }
            } else {
                node = want_far ? far : -1;
            }
        }
        if (node < 0) {
            while (sp > 0) {
                const int cand = stack[--sp];
                if (wanted(H.nodes.data() + (size_t)cand * 8)) { node = cand; break; }
            }
            if (node < 0) break;
        }
    }
    return evals;
}

bool check_tree(const nr::TriBvh &H, const float *V, const int32_t *T, long nt, const float *table, int leaf) {
    std::vector<int> seen((size_t)nt, 0);
    long leaves_tris = 0;
    for (long k = 0; k < H.nnodes; ++k) {
        const float *n = H.nodes.data() + (size_t)k * 8;
        const int w3 = word(n + 3), w7 = word(n + 7);
        if (w7 > 0) {
            if (w3 <= k || w3 >= H.nnodes || w7 <= k || w7 >= H.nnodes) return false;
            for (int ch : {w3, w7}) {
                const float *c = H.nodes.data() + (size_t)ch * 8;
                for (int a = 0; a < 3; ++a)
                    if (c[a] < n[a] || c[4 + a] > n[4 + a]) return false;
            }
        } else {
            const long first = w3, count = -w7;
            if (first < 0 || first + count > H.ntl || count > leaf || (count == 0 && H.ntl != 0)) return false;
            leaves_tris += count;
            for (long t = first; t < first + count; ++t) {
                const float *q = H.tris.data() + (size_t)t * 12;
                const int oi = word(q + 3);
                if (oi < 0 || oi >= nt || seen[(size_t)oi]++) return false;
                for (int c = 0; c < 3; ++c)
                    for (int a = 0; a < 3; ++a) {
                        const float v = V[3 * (size_t)T[3 * oi + c] + a];
                        if (q[4 * c + a] != v || !(n[a] < v) || !(n[4 + a] > v)) return false;
                    }
            }
        }
    }
    long live = 0;
    for (long t = 0; t < nt; ++t) {
        const float *f = table + (size_t)t * 21;
        const bool has = f[0] != 0 || f[1] != 0 || f[2] != 0;
        live += has;
        if (has != (seen[(size_t)t] == 1)) return false;
    }
    int bound = 1;
    while ((1l << (bound - 1)) < (live > 1 ? live : 1)) ++bound;
    return leaves_tris == live && H.ntl == live && H.depth <= bound;
}

unsigned rnd(unsigned &s) { s = s * 1664525u + 1013904223u; return s >> 8; }

int run_mesh(const char *name, const float *V, long nv, const int32_t *T, long nt) {
    std::vector<float> table((size_t)nt * 21);
    int closed = -1;
    if (nr_trimesh_normals(V, nv, T, nt, table.data(), &closed) != NR_OK || closed < 0) return 1;
    for (int leaf : {1, 3, 8, 32}) {
        nr::TriBvh H;
        if (!nr::trimesh_build(V, nv, T, nt, leaf, table.data(), H) || !check_tree(H, V, T, nt, table.data(), leaf)) {
            fprintf(stderr, "%s: leaf %d: the hierarchy breaks an invariant\n", name, leaf);
            return 1;
        }
        // four waves of points: in the bound scaled 1.5, on vertices, and far away; ragged sizes
        unsigned seed = 12345u + (unsigned)leaf;
        long total = 0;
        for (int w = 0; w < 4; ++w) {
            std::vector<V3> P;
            const int np = w == 3 ? 39 : 64;
            for (int l = 0; l < np; ++l) {
                float c[3];
                for (int a = 0; a < 3; ++a) {
                    const float mid = 0.5f * (H.lo[a] + H.hi[a]), half = 0.75f * (H.hi[a] - H.lo[a]) + 1e-3f;
                    c[a] = mid + half * ((float)rnd(seed) / 8388608.0f - 1.0f);
                    if (w == 1 && l % 4 == 0) c[a] = V[3 * (size_t)(rnd(seed) % (unsigned)nv) + a];
                    if (w == 2 && l == 7) c[a] = 50.0f * (a + 1);
                }
                P.push_back({c[0], c[1], c[2]});
            }
            std::vector<Best> hb(P.size()), bb(P.size());
            total += walk(H, P, hb);
            for (long t = 0; t < H.ntl; ++t) eval(H, t, P, bb);
            for (size_t l = 0; l < P.size(); ++l)
                if (memcmp(&hb[l].d2, &bb[l].d2, 4) != 0 || hb[l].idx != bb[l].idx) {
                    fprintf(stderr, "%s: leaf %d: the walk finds (%g, %d), brute force (%g, %d)\n", name, leaf, hb[l].d2,
                            hb[l].idx, bb[l].d2, bb[l].idx);
                    return 1;
                }
        }
        printf("%s: nv %ld nt %ld closed %d leaf %d: %ld nodes, depth %d, %.1f of %ld triangles per wave\n", name, nv, nt,
               closed, leaf, H.nnodes, H.depth, total / 4.0, H.ntl);
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s FILE.obj...\n", argv[0]);
        return 2;
    }
    int ok = 0, failed = 0;
    for (int i = 1; i < argc; ++i) {
        float *V = nullptr;
        int32_t *T = nullptr;
        long nv = 0, nt = 0;
        const int rc = nr_obj_load(argv[i], &V, &nv, &T, &nt);
        if (rc != NR_OK) {
            if (V || T || (rc != NR_E_IO && rc != NR_E_FORMAT)) return 1;
            ++failed;
            continue;
        }
        ++ok;
        int bad = 0;
        if (nv >= 1 && nt >= 1) bad = run_mesh(argv[i], V, nv, T, nt);
        free(V);
        free(T);
        if (bad) return 1;
    }
    printf("ok %d failed %d\n", ok, failed);
    return 0;
}
