// Ray casting against a triangle mesh (include/gs2m_meshao.h): an LBVH built on the device, a stackless
// any-hit and closest-hit traversal, ambient occlusion, and the transfer of a source mesh's detail to the points of another
// (include/gs2m_meshtransfer.h).  fp64 throughout, evaluated as written (-ffp-contract=off): the triangle test, the AO frame and
// the transfer's interpolation are a contract that tests/mesh_ao_ref.py and tests/mesh_transfer_ref.py restate bit for bit.
#include <cmath>
#include "eval_common.h"
#include "../../include/gs2m_meshao.h"
#include "../../include/gs2m_meshtransfer.h"

namespace {

typedef gs2m_bvh_node Node;
static_assert(sizeof(Node) == GS2M_BVH_NODE_BYTES, "the node layout is part of the header");

constexpr long long BVH_LIMIT = 1ll << 30;  // the radix sort's bound
constexpr uint32_t DEAD_CODE = 1u << 30;
constexpr int SORT_BITS = 31;

// ---- the contract's arithmetic ----
__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const double* a, const double* b, double* r) {
    r[0] = a[1] * b[2] - a[2] * b[1];
    r[1] = a[2] * b[0] - a[0] * b[2];
    r[2] = a[0] * b[1] - a[1] * b[0];
}

struct Ray {
    double o[3], d[3], inv[3];
    double tmin, tmax;
};
__device__ __forceinline__ void ray_finish(Ray& r) {
#pragma unroll
    for (int k = 0; k < 3; k++) r.inv[k] = 1.0 / r.d[k];
}

// the Triangle paragraph up to t, whatever the range says
__device__ __forceinline__ bool triangle_tuv(const Ray& r, const double* a, const double* b, const double* c, double& det, double& t, double& u,
                                             double& v) {
    double e1[3], e2[3], T[3], P[3], Q[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        e1[k] = b[k] - a[k];
        e2[k] = c[k] - a[k];
        T[k] = r.o[k] - a[k];
    }
    cross3(r.d, e2, P);
    det = dot3(e1, P);
    if (det == 0.0 || !std::isfinite(det)) return false;
    u = dot3(T, P) / det;
    if (!(u >= 0.0 && u <= 1.0)) return false;
    cross3(T, e1, Q);
    v = dot3(r.d, Q) / det;
    if (!(v >= 0.0 && u + v <= 1.0)) return false;
    t = dot3(e2, Q) / det;
    return true;
}
__device__ __forceinline__ bool hits_triangle(const Ray& r, const double* a, const double* b, const double* c) {
    double det, t, u, v;
    return triangle_tuv(r, a, b, c, det, t, u, v) && t > r.tmin && t <= r.tmax;
}
// the Candidate and Facing paragraphs: closed at both ends
__device__ __forceinline__ bool candidate(const Ray& r, int facing, const double* a, const double* b, const double* c, double& t, double& u,
                                          double& v) {
    double det;
    if (!triangle_tuv(r, a, b, c, det, t, u, v)) return false;
    if ((facing > 0 && !(det > 0.0)) || (facing < 0 && !(det < 0.0))) return false;
    return t >= r.tmin && t <= r.tmax;
}

__device__ __forceinline__ bool finite3(const double* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

// a mesh of n triangles over nv vertices and the 2 n - 1 nodes of its hierarchy, as the entry points got them
struct Mesh {
    const Node* nodes;
    long long n, nv;
    const double* verts;
    const int* tris;
};

// the corners of triangle t, or false for a dead one (no vertex is read through an index that has not been tested)
__device__ __forceinline__ bool load_live(const Mesh& m, long long t, double* a, double* b, double* c) {
    const int ia = m.tris[3 * t], ib = m.tris[3 * t + 1], ic = m.tris[3 * t + 2];
    if (!ids_in_range(ia, ib, ic, m.nv)) return false;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        a[k] = m.verts[3 * (size_t)ia + k];
        b[k] = m.verts[3 * (size_t)ib + k];
        c[k] = m.verts[3 * (size_t)ic + k];
    }
    return finite3(a) && finite3(b) && finite3(c);
}

// the Box test paragraph: conservative
constexpr double BOX_PAD = 1.0 / 1073741824.0;         // 2^-30
constexpr double BOX_SLACK = 1.0 / 1099511627776.0;    // 2^-40
__device__ __forceinline__ bool box_maybe_hit(const Ray& r, const Node& n) {
    if (!(n.lo[0] <= n.hi[0])) return false;  // empty
    double te = r.tmin, tx = r.tmax;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double pad = BOX_PAD * ((fabs(n.lo[k]) + fabs(n.hi[k])) + fabs(r.o[k]));
        const double lo = n.lo[k] - pad, hi = n.hi[k] + pad;
        if (r.d[k] == 0.0) {
            if (r.o[k] < lo || r.o[k] > hi) return false;
        } else if (!std::isinf(r.inv[k])) {
            const double t1 = (lo - r.o[k]) * r.inv[k], t2 = (hi - r.o[k]) * r.inv[k];
            const double tn = t2 < t1 ? t2 : t1, tf = t2 > t1 ? t2 : t1;
            te = tn > te ? tn : te;  // a NaN never wins
            tx = tf < tx ? tf : tx;
        }
    }
    return !(te > tx && te - tx > BOX_SLACK * (fabs(te) + fabs(tx)));
}

// the Traversal paragraph.  Every index is tested before it is followed and the walk stops after 2 n - 1 nodes: a buffer that
// was never built gives a wrong answer, not a wild read.  at_leaf(triangle, a, b, c) gets every live triangle other than `skip`
// whose leaf box the ray may hit, and ends the walk by returning true; it may shrink r.tmax, which the box test reads anew.
// Not __forceinline__: inlined before its callers' other calls, the any-hit loop gets another register allocation and the
// AO kernel loses 0.75 % (profiles/mesh_bvh_refactor_resources.md); the inliner takes it anyway, no kernel has a call.
template <class Leaf>
__device__ void walk(const Mesh& m, const Ray& r, int skip, Leaf at_leaf) {
    const long long total = 2 * m.n - 1;
    long long node = 0;
    for (long long step = 0; step < total && node >= 0 && node < total; step++) {
        const Node nd = m.nodes[node];
        if (!box_maybe_hit(r, nd)) {
            node = nd.miss;
        } else if (node >= m.n - 1) {  // leaf
            const long long t = nd.left;
            double a[3], b[3], c[3];
            if (t >= 0 && t < m.n && t != skip && load_live(m, t, a, b, c) && at_leaf((int)t, a, b, c)) return;
            node = nd.miss;
        } else {
            node = nd.left;
        }
    }
}

__device__ bool occluded(const Mesh& m, const Ray& r, int skip) {
    bool hit = false;
    walk(m, r, skip, [&](int, const double* a, const double* b, const double* c) { return hit = hits_triangle(r, a, b, c); });
    return hit;
}

// the Answer and Closest traversal paragraphs: no leaf ends the walk, and the ray, a copy, has its tmax shrunk to the best t so
// far.  A candidate beyond the best fails `t <= r.tmax`; one at the best is kept for the index rule.
struct Closest {
    double t, u, v;
    int tri;
};
__device__ Closest closest(const Mesh& m, Ray r, int skip, int facing) {
    Closest best = {INFINITY, 0.0, 0.0, -1};
    walk(m, r, skip, [&](int tri, const double* a, const double* b, const double* c) {
        double t, u, v;
        if (candidate(r, facing, a, b, c, t, u, v) && (t < best.t || (t == best.t && (best.tri < 0 || tri < best.tri)))) {
            best = {t, u, v, tri};
            r.tmax = t;
        }
        return false;
    });
    return best;
}

// ---- build ----
struct BvhWs {
    Node* nodes;         // 2 n - 1
    double* cen;         // 3 n: centroids
    uint32_t* keys;      // n
    SortBufs sort;       // n each; (code, triangle) sorted in kB / vB
    int *rightof, *last; // n: the right child of the internal node that splits behind position g; the last position of internal node i
    uint32_t* arrived;   // n: arrival counters of the refit
    double *part, *bounds;  // 6 RED_BLOCKS, 6: lo, hi of the live centroids
    void* temp;
    size_t temp_bytes, bytes;
};
BvhWs carve(char* base, long long nt) {
    Carver c{base, 0};
    BvhWs w;
    const size_t n = (size_t)(nt > 0 ? nt : 1);
    w.nodes = c.take<Node>(2 * n - 1);
    w.cen = c.take<double>(3 * n);
    w.keys = c.take<uint32_t>(n);
    w.sort = take_sort_bufs(c, n);
    w.rightof = c.take<int>(n);
    w.last = c.take<int>(n);
    w.arrived = c.take<uint32_t>(n);
    w.part = c.take<double>(6 * RED_BLOCKS);
    w.bounds = c.take<double>(6);
    w.temp_bytes = gs2m_radix_temp_bytes(n, SORT_BITS);
    w.temp = c.take<char>(w.temp_bytes + GS2M_ALIGN);
    w.bytes = c.off;
    return w;
}

// centroid of a live triangle, NaN marks a dead one
__global__ void __launch_bounds__(256) centroid_kernel(const Mesh m, double* __restrict__ cen) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= m.n) return;
    double a[3], b[3], c[3];
    if (load_live(m, t, a, b, c)) {
#pragma unroll
        for (int k = 0; k < 3; k++) cen[3 * t + k] = ((a[k] + b[k]) + c[k]) / 3.0;
    } else {
#pragma unroll
        for (int k = 0; k < 3; k++) cen[3 * t + k] = NAN;
    }
}

struct BoundsOp {  // q < 3: min, else max
    __device__ static double identity(int q) { return q < 3 ? INFINITY : -INFINITY; }
    __device__ static double combine(int q, double a, double b) { return q < 3 ? (b < a ? b : a) : (b > a ? b : a); }
};
struct BoundsTerm {
    const double* cen;
    __device__ void operator()(long long i, double* acc, u64&) const {
        const double x = cen[3 * i], y = cen[3 * i + 1], z = cen[3 * i + 2];
        if (!(x == x && y == y && z == z)) return;  // dead, or a centroid that overflowed
        acc[0] = BoundsOp::combine(0, acc[0], x); acc[1] = BoundsOp::combine(1, acc[1], y); acc[2] = BoundsOp::combine(2, acc[2], z);
        acc[3] = BoundsOp::combine(3, acc[3], x); acc[4] = BoundsOp::combine(4, acc[4], y); acc[5] = BoundsOp::combine(5, acc[5], z);
    }
};

__device__ __forceinline__ uint32_t spread10(uint32_t x) {  // 10 bits -> every third bit
    x &= 0x3FFu;
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}
__global__ void __launch_bounds__(256) key_kernel(long long n, const double* __restrict__ cen, const double* __restrict__ bounds,
                                                  uint32_t* __restrict__ keys) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    uint32_t q[3];
    bool live = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double x = cen[3 * t + k], lo = bounds[k], hi = bounds[3 + k];
        live = live && x == x;
        const double f = hi > lo ? (x - lo) / (hi - lo) * 1023.0 : 0.0;
        q[k] = f >= 1023.0 ? 1023u : (f > 0.0 ? (uint32_t)(int)f : 0u);  // NaN -> 0
    }
    keys[t] = live ? (spread10(q[0]) << 2) | (spread10(q[1]) << 1) | spread10(q[2]) : DEAD_CODE;
}

// leaves: box, triangle; the refit's counters; the root has no parent (Karras's kernel writes every other parent)
__global__ void __launch_bounds__(256) leaf_kernel(const Mesh m, const uint32_t* __restrict__ sorted_tri, Node* __restrict__ nodes,
                                                   uint32_t* __restrict__ arrived) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= m.n) return;
    const long long t = sorted_tri[i];
    Node& nd = nodes[m.n - 1 + i];
    double a[3], b[3], c[3];
    if (t < m.n && load_live(m, t, a, b, c)) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double m0 = b[k] < a[k] ? b[k] : a[k], m1 = b[k] > a[k] ? b[k] : a[k];
            nd.lo[k] = c[k] < m0 ? c[k] : m0;
            nd.hi[k] = c[k] > m1 ? c[k] : m1;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            nd.lo[k] = INFINITY;
            nd.hi[k] = -INFINITY;
        }
    }
    nd.left = (int)t;
    nd.right = -1;
    arrived[i] = 0u;
    if (i == 0) nodes[0].parent = -1;
}

// common prefix of the keys (code, position) at the sorted positions i and j; -1 outside the array
__device__ __forceinline__ int prefix_of(const uint32_t* __restrict__ codes, long long n, long long i, long long j) {
    if (j < 0 || j >= n) return -1;
    const u64 x = ((u64)(codes[i] ^ codes[j]) << 32) | (u64)(uint32_t)(i ^ j);
    return __clzll((long long)x);
}

// Karras 2012, section 4: internal node i covers the positions between i and its other end j; it splits behind position g
__global__ void __launch_bounds__(256) hierarchy_kernel(long long n, const uint32_t* __restrict__ codes, Node* __restrict__ nodes,
                                                        int* __restrict__ rightof, int* __restrict__ last) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n - 1) return;
    const int d = prefix_of(codes, n, i, i + 1) - prefix_of(codes, n, i, i - 1) < 0 ? -1 : 1;
    const int pmin = prefix_of(codes, n, i, i - d);
    long long lmax = 2;
    while (prefix_of(codes, n, i, i + lmax * d) > pmin) lmax *= 2;
    long long l = 0;
    for (long long t = lmax / 2; t >= 1; t /= 2)
        if (prefix_of(codes, n, i, i + (l + t) * d) > pmin) l += t;
    const long long j = i + l * d;
    const int pnode = prefix_of(codes, n, i, j);
    long long s = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (prefix_of(codes, n, i, i + (s + t) * d) > pnode) s += t;
    } while (t > 1);
    const long long g = i + s * d + (d < 0 ? -1 : 0);
    const long long first = i < j ? i : j, end = i < j ? j : i;
    const long long left = first == g ? n - 1 + g : g, right = end == g + 1 ? n - 1 + g + 1 : g + 1;
    nodes[i].left = (int)left;
    nodes[i].right = (int)right;
    nodes[left].parent = (int)i;
    nodes[right].parent = (int)i;
    rightof[g] = (int)right;
    last[i] = (int)end;
}

// the next subtree in depth-first order behind a node whose last position is e: the right child of the node that splits behind e
__global__ void __launch_bounds__(256) miss_kernel(long long n, const int* __restrict__ rightof, const int* __restrict__ last,
                                                   Node* __restrict__ nodes) {
    const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
    if (x >= 2 * n - 1) return;
    const long long e = x < n - 1 ? last[x] : x - (n - 1);
    nodes[x].miss = e == n - 1 ? -1 : rightof[e];
}

__device__ __forceinline__ double load_fresh(const double* p) {  // past this CU's L1: the other child was written by another CU
    return __longlong_as_double((long long)__hip_atomic_load((const u64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// One thread per leaf climbs; at every node the second arrival (an acq_rel counter) makes the box from left then right.
__global__ void __launch_bounds__(256) refit_kernel(long long n, Node* __restrict__ nodes, uint32_t* __restrict__ arrived) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    long long p = nodes[n - 1 + i].parent;
    for (long long step = 0; step < n && p >= 0 && p < n - 1; step++) {
        if (__hip_atomic_fetch_add(arrived + p, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == 0u) return;
        const int l = nodes[p].left, r = nodes[p].right;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double a = load_fresh(&nodes[l].lo[k]), b = load_fresh(&nodes[r].lo[k]);
            const double c = load_fresh(&nodes[l].hi[k]), e = load_fresh(&nodes[r].hi[k]);
            nodes[p].lo[k] = b < a ? b : a;
            nodes[p].hi[k] = e > c ? e : c;
        }
        p = nodes[p].parent;
    }
}

// ---- queries ----
__device__ __forceinline__ void load_ray(long long i, const double* __restrict__ origins, const double* __restrict__ dirs, double tmin,
                                         double tmax, Ray& r) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        r.o[k] = origins[3 * i + k];
        r.d[k] = dirs[3 * i + k];
    }
    r.tmin = tmin;
    r.tmax = tmax;
    ray_finish(r);
}

__global__ void __launch_bounds__(256) occluded_kernel(const Mesh m, long long n_rays, const double* __restrict__ origins,
                                                       const double* __restrict__ dirs, double tmin, double tmax,
                                                       const int* __restrict__ skip, unsigned char* __restrict__ hit) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rays) return;
    Ray r;
    load_ray(i, origins, dirs, tmin, tmax, r);
    hit[i] = m.n > 0 && occluded(m, r, skip ? skip[i] : -1) ? 1 : 0;
}

// point p and its normal, or false for "no point here": a negative entry of `gate` (the skip or owner array; may be null), a
// normal whose dot(n, n) is not positive and finite, or a coordinate that is not finite.  Such a point casts no ray.  `entry` gets
// the gate's entry as read, -1 without a gate.
__device__ __forceinline__ bool load_point(long long p, const double* __restrict__ points, const double* __restrict__ normals,
                                           const int* __restrict__ gate, double* pt, double* n, int& entry) {
    entry = gate ? gate[p] : -1;
    if (gate && entry < 0) return false;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        pt[k] = points[3 * p + k];
        n[k] = normals[3 * p + k];
    }
    const double nn = dot3(n, n);
    return nn > 0.0 && std::isfinite(nn) && finite3(pt);
}

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// the AO paragraph's frame and origin of point p; false: visible = K without a ray
struct AoPoint {
    double o[3], T[3], B[3], n[3];
    const double* table;
    int skip;
};
__device__ __forceinline__ bool ao_point(long long p, const double* __restrict__ points, const double* __restrict__ normals,
                                         const int* __restrict__ skip, int R, int K, const double* __restrict__ dirs, double bias, long long index0,
                                         long long seed, AoPoint& a) {
    double pt[3];
    if (!load_point(p, points, normals, skip, pt, a.n, a.skip)) return false;
    const uint32_t r = mix32((uint32_t)((u64)index0 + (u64)p + (u64)seed)) % (uint32_t)R;
    a.table = dirs + (size_t)r * K * 3;
    const double s = copysign(1.0, a.n[2]);
    const double q = -1.0 / (s + a.n[2]);
    const double b = (a.n[0] * a.n[1]) * q;
    a.T[0] = 1.0 + ((s * a.n[0]) * a.n[0]) * q; a.T[1] = s * b; a.T[2] = -(s * a.n[0]);
    a.B[0] = b; a.B[1] = s + (a.n[1] * a.n[1]) * q; a.B[2] = -a.n[1];
#pragma unroll
    for (int k = 0; k < 3; k++) a.o[k] = pt[k] + a.n[k] * bias;
    return true;
}
__device__ __forceinline__ void ao_ray(const AoPoint& a, int k, double radius, Ray& r) {
    const double lx = a.table[3 * k], ly = a.table[3 * k + 1], lz = a.table[3 * k + 2];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        r.o[c] = a.o[c];
        r.d[c] = (a.T[c] * lx + a.B[c] * ly) + a.n[c] * lz;
    }
    r.tmin = 0.0;
    r.tmax = radius;
    ray_finish(r);
}

// one wave per point: the lanes take 64 directions per step; the rays share their origin and the top of the tree
__global__ void __launch_bounds__(256) ao_wave_kernel(const Mesh m, long long n_points, const double* __restrict__ points,
                                                      const double* __restrict__ normals, const int* __restrict__ skip, int R, int K,
                                                      const double* __restrict__ dirs, double bias, double radius, long long index0, long long seed,
                                                      int* __restrict__ visible) {
    const int lane = threadIdx.x & 63;
    const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= n_points) return;
    AoPoint a;
    int count = K;
    if (m.n > 0 && ao_point(p, points, normals, skip, R, K, dirs, bias, index0, seed, a)) {
        count = 0;
        for (int k0 = 0; k0 < K; k0 += 64) {
            const int k = k0 + lane;
            bool open = false;
            if (k < K) {
                Ray r;
                ao_ray(a, k, radius, r);
                open = !occluded(m, r, a.skip);
            }
            count += __popcll(__ballot(open));
        }
    }
    if (lane == 0) visible[p] = count;
}

__global__ void __launch_bounds__(256) texture_occlusion_kernel(long long n, const int* __restrict__ owner, const int* __restrict__ visible, int K,
                                                                unsigned char* __restrict__ orm) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n || owner[p] < 0) return;
    const double x = floor(255.0 * ((double)visible[p] / (double)K) + 0.5);
    orm[3 * p] = (unsigned char)(x < 0.0 ? 0.0 : (x > 255.0 ? 255.0 : x));
}

__global__ void __launch_bounds__(256) closest_kernel(const Mesh m, long long n_rays, const double* __restrict__ origins,
                                                      const double* __restrict__ dirs, double tmin, double tmax, const int* __restrict__ skip,
                                                      int facing, int* __restrict__ tri, double* __restrict__ t, double* __restrict__ uv) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rays) return;
    Closest best = {INFINITY, 0.0, 0.0, -1};
    if (m.n > 0) {
        Ray r;
        load_ray(i, origins, dirs, tmin, tmax, r);
        best = closest(m, r, skip ? skip[i] : -1, facing);
    }
    tri[i] = best.tri;
    t[i] = best.t;
    uv[2 * i] = best.u;
    uv[2 * i + 1] = best.v;
}

// gs2m_meshtransfer.h: one lane per point casts both rays
__global__ void __launch_bounds__(256) transfer_kernel(const Mesh m, long long n_points, const double* __restrict__ points,
                                                       const double* __restrict__ normals, const int* __restrict__ owner, double distance,
                                                       int two_sided, int channels, const float* __restrict__ att,
                                                       const double* __restrict__ src_normals, int want_normal, int stride,
                                                       float* __restrict__ values, int* __restrict__ hit_tri, double* __restrict__ offset) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_points) return;
    Closest best = {INFINITY, 0.0, 0.0, -1};
    double off = 0.0;
    Ray r;
    int own;
    if (m.n > 0 && load_point(p, points, normals, owner, r.o, r.d, own)) {
        r.tmin = 0.0;
        r.tmax = distance;
        ray_finish(r);
        best = closest(m, r, -1, two_sided ? 0 : -1);
        off = best.t;
#pragma unroll
        for (int k = 0; k < 3; k++) r.d[k] = -r.d[k];
        r.tmax = best.t < distance ? best.t : distance;  // B wins only with a smaller t: nothing beyond t_F is looked at
        ray_finish(r);
        const Closest back = closest(m, r, -1, two_sided ? 0 : 1);
        if (back.tri >= 0 && (best.tri < 0 || back.t < best.t)) {
            best = back;
            off = -back.t;
        }
        if (best.tri < 0) off = 0.0;
    }
    hit_tri[p] = best.tri;
    if (offset) offset[p] = off;
    if (best.tri < 0) return;
    double a[3], b[3], c[3];
    if (!load_live(m, best.tri, a, b, c)) return;  // never: it was hit, so it is live and its indices are in range
    const size_t i0 = (size_t)m.tris[3 * (size_t)best.tri], i1 = (size_t)m.tris[3 * (size_t)best.tri + 1], i2 = (size_t)m.tris[3 * (size_t)best.tri + 2];
    const double u = best.u, v = best.v, w = (1.0 - u) - v;
    float* row = values + (size_t)p * stride;
    for (int ch = 0; ch < channels; ch++)
        row[ch] = (float)((w * (double)att[i0 * channels + ch] + u * (double)att[i1 * channels + ch]) + v * (double)att[i2 * channels + ch]);
    if (!want_normal) return;
    if (src_normals) {
#pragma unroll
        for (int k = 0; k < 3; k++)
            row[channels + k] = (float)((w * src_normals[3 * i0 + k] + u * src_normals[3 * i1 + k]) + v * src_normals[3 * i2 + k]);
    } else {
        double e1[3], e2[3], face[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            e1[k] = b[k] - a[k];
            e2[k] = c[k] - a[k];
        }
        cross3(e1, e2, face);
#pragma unroll
        for (int k = 0; k < 3; k++) row[channels + k] = (float)face[k];
    }
}

// the checks every query shares
int query_status(const void* bvh, long long bvh_bytes, long long nv, const double* verts, long long nt, const int* tris) {
    if (nv < 0 || nt < 0) return GS2M_ERR_INVALID_ARG;
    if (nt >= BVH_LIMIT || nv > 0x7FFFFFFFll) return GS2M_ERR_UNSUPPORTED;
    if (nt > 0 && (!bvh || !tris || (nv > 0 && !verts) || bvh_bytes < (long long)carve(nullptr, nt).bytes)) return GS2M_ERR_INVALID_ARG;
    return GS2M_OK;
}
// ... and, behind them, the checks of a query's `count` rays or points: `valid` says that its other arguments are, `buffers` that
// every per-row buffer is there.  GS2M_OK with count == 0: nothing to launch.
int rows_status(long long count, bool valid, bool buffers, long long limit) {
    if (count < 0 || !valid || (count > 0 && !buffers)) return GS2M_ERR_INVALID_ARG;
    return count > limit ? GS2M_ERR_UNSUPPORTED : GS2M_OK;
}
int rays_status(long long n_rays, const double* origins, const double* dirs, double tmin, double tmax, bool outputs) {
    return rows_status(n_rays, tmin == tmin && tmax == tmax, origins && dirs && outputs, MAX_LAUNCH);
}

}  // namespace

extern "C" {

int gs2m_bvh_bytes(long long n_triangles, long long* bytes) {
    if (!bytes || n_triangles < 0) return GS2M_ERR_INVALID_ARG;
    if (n_triangles >= BVH_LIMIT) return GS2M_ERR_UNSUPPORTED;
    *bytes = (long long)carve(nullptr, n_triangles).bytes;
    return GS2M_OK;
}

int gs2m_bvh_build(long long n_verts, const double* verts, long long n_triangles, const int* triangles, void* bvh, long long bvh_bytes,
                   void* stream) {
    const int st = query_status(bvh, bvh_bytes, n_verts, verts, n_triangles, triangles);
    if (st != GS2M_OK) return st;
    const long long n = n_triangles;
    if (n == 0) return GS2M_OK;
    hipStream_t s = (hipStream_t)stream;
    const BvhWs w = carve((char*)bvh, n);
    const SortBufs& b = w.sort;
    const Mesh m = {nullptr, n, n_verts, verts, triangles};  // no nodes to read yet: the kernels below write them through w.nodes
    centroid_kernel<<<blocks_of(n), 256, 0, s>>>(m, w.cen);
    reduce_fixed_order<6, BoundsOp>(n, BoundsTerm{w.cen}, w.part, nullptr, w.bounds, nullptr, s);
    key_kernel<<<blocks_of(n), 256, 0, s>>>(n, w.cen, w.bounds, w.keys);
    if (hipGetLastError() != hipSuccess ||
        gs2m_radix_sort_pairs(w.temp, w.temp_bytes, w.keys, nullptr, b.kA, b.vA, b.kB, b.vB, (size_t)n, SORT_BITS, false, s) != hipSuccess)
        return GS2M_ERR_HIP;
    leaf_kernel<<<blocks_of(n), 256, 0, s>>>(m, b.vB, w.nodes, w.arrived);
    if (n > 1) {
        hierarchy_kernel<<<blocks_of(n - 1), 256, 0, s>>>(n, b.kB, w.nodes, w.rightof, w.last);
        refit_kernel<<<blocks_of(n), 256, 0, s>>>(n, w.nodes, w.arrived);
    }
    miss_kernel<<<blocks_of(2 * n - 1), 256, 0, s>>>(n, w.rightof, w.last, w.nodes);
    return gs2m_status(hipGetLastError());
}

int gs2m_bvh_occluded(const void* bvh, long long bvh_bytes, long long n_verts, const double* verts, long long n_triangles,
                      const int* triangles, long long n_rays, const double* origins, const double* dirs, double tmin, double tmax,
                      const int* skip, unsigned char* hit, void* stream) {
    int st = query_status(bvh, bvh_bytes, n_verts, verts, n_triangles, triangles);
    if (st == GS2M_OK) st = rays_status(n_rays, origins, dirs, tmin, tmax, hit != nullptr);
    if (st != GS2M_OK || n_rays == 0) return st;
    const Mesh m = {(const Node*)bvh, n_triangles, n_verts, verts, triangles};
    occluded_kernel<<<blocks_of(n_rays), 256, 0, (hipStream_t)stream>>>(m, n_rays, origins, dirs, tmin, tmax, skip, hit);
    return gs2m_status(hipGetLastError());
}

int gs2m_bvh_closest(const void* bvh, long long bvh_bytes, long long n_verts, const double* verts, long long n_triangles,
                     const int* triangles, long long n_rays, const double* origins, const double* dirs, double tmin, double tmax,
                     const int* skip, int facing, int* tri, double* t, double* uv, void* stream) {
    int st = query_status(bvh, bvh_bytes, n_verts, verts, n_triangles, triangles);
    if (st == GS2M_OK && (facing < -1 || facing > 1)) st = GS2M_ERR_INVALID_ARG;
    if (st == GS2M_OK) st = rays_status(n_rays, origins, dirs, tmin, tmax, tri && t && uv);
    if (st != GS2M_OK || n_rays == 0) return st;
    const Mesh m = {(const Node*)bvh, n_triangles, n_verts, verts, triangles};
    closest_kernel<<<blocks_of(n_rays), 256, 0, (hipStream_t)stream>>>(m, n_rays, origins, dirs, tmin, tmax, skip, facing, tri, t, uv);
    return gs2m_status(hipGetLastError());
}

int gs2m_bvh_ao(const void* bvh, long long bvh_bytes, long long n_verts, const double* verts, long long n_triangles, const int* triangles,
                long long n_points, const double* points, const double* normals, const int* skip, int R, int K, const double* dirs, double bias,
                double radius, long long index0, long long seed, int* visible, void* stream) {
    int st = query_status(bvh, bvh_bytes, n_verts, verts, n_triangles, triangles);
    if (st == GS2M_OK)
        st = rows_status(n_points, R >= 1 && K >= 1 && dirs && bias == bias && radius == radius, points && normals && visible, 0x7FFFFFFFll);
    if (st != GS2M_OK || n_points == 0) return st;
    const Mesh m = {(const Node*)bvh, n_triangles, n_verts, verts, triangles};
    ao_wave_kernel<<<(unsigned)((n_points + 3) / 4), 256, 0, (hipStream_t)stream>>>(m, n_points, points, normals, skip, R, K, dirs, bias, radius,
                                                                                    index0, seed, visible);
    return gs2m_status(hipGetLastError());
}

int gs2m_texture_occlusion(long long n_texels, const int* owner, const int* visible, int K, unsigned char* orm, void* stream) {
    if (n_texels < 0 || K < 1 || (n_texels > 0 && (!owner || !visible || !orm))) return GS2M_ERR_INVALID_ARG;
    if (n_texels == 0) return GS2M_OK;
    if (n_texels > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    texture_occlusion_kernel<<<blocks_of(n_texels), 256, 0, (hipStream_t)stream>>>(n_texels, owner, visible, K, orm);
    return gs2m_status(hipGetLastError());
}

int gs2m_mesh_transfer(const void* bvh, long long bvh_bytes, long long n_src_verts, const double* src_verts, long long n_src_triangles,
                       const int* src_triangles, long long n_points, const double* points, const double* normals, const int* owner,
                       double distance, int two_sided, int channels, const float* src_attributes, const double* src_normals, int want_normal,
                       int stride, float* values, int* hit_tri, double* offset, void* stream) {
    int st = query_status(bvh, bvh_bytes, n_src_verts, src_verts, n_src_triangles, src_triangles);
    const long long columns = (long long)channels + (want_normal ? 3 : 0);
    if (st == GS2M_OK)
        st = rows_status(n_points, distance >= 0.0 && channels >= 0 && (channels == 0 || src_attributes) && stride >= columns,
                         points && normals && hit_tri && (columns == 0 || values), MAX_LAUNCH);
    if (st != GS2M_OK || n_points == 0) return st;
    const Mesh m = {(const Node*)bvh, n_src_triangles, n_src_verts, src_verts, src_triangles};
    transfer_kernel<<<blocks_of(n_points), 256, 0, (hipStream_t)stream>>>(m, n_points, points, normals, owner, distance, two_sided != 0, channels,
                                                                          src_attributes, src_normals, want_normal != 0, stride, values, hit_tri,
                                                                          offset);
    return gs2m_status(hipGetLastError());
}

}  // extern "C"
