// The triangle rasterizer core shared by mesh_depth.hip (the depth image of the visibility cull) and mesh_view.hip (the
// visibility buffer of the shaded views); the contract: DESIGN.md §14.  Compile the including unit with -ffp-contract=off.
//
// A thread per triangle loads its three vertices once and walks the views of the call: camera-space vertices, the
// three edge planes cross(b, c), cross(c, a), cross(a, b) and the plane (n, dot(n, a)), all fp64, then the pixel box: the box
// of the projected corners of the triangle's part at z >= near (a shade below it), widened outwards to whole pixels and clamped
// to the frame, so a triangle that crosses the camera plane is boxed by its part in front; one that cannot reach [near, far]
// is dropped.  By the clamped box's size:
//   <= LANE_MAX_PIXELS   the triangle's own lane walks it (TnT meshes: millions of triangles of a pixel or less);
//   <= WAVE_MAX_PIXELS   the triangle goes to the front of the view's list: one wave per entry, 64 pixels a step;
//   beyond               it goes to the back of the list: every workgroup of the view's row takes 256-pixel chunks of it.
// Lists are filled with one atomic per wave and class (ballot, leader, prefix by lane).  A pixel test is: the three edge values
// at the centre's ray, the sign rule, z = dot(n, a) / dot(n, r), the range test, z rounded once to fp32 and handed with the
// triangle's index to the SINK, which keeps a per-pixel unsigned minimum: an atomicMin skipped when a plain read already shows a
// smaller value (values only fall, so a stale read merely costs an atomic).
//   DepthSink   32 bits per pixel: the fp32 z's bit pattern;
//   KeySink     64 bits per pixel: (z bits << 32) | triangle index, so equal z goes to the lowest index.
// Both images start as all ones.  Nothing depends on the order in which triangles or list entries are met: two runs, or a
// permuted triangle list, give the same bits.
// Every pixel loop runs over a box clamped to [0, W - 1] x [0, H - 1]; list slots are < n_tris because a triangle enters a
// view's list at most once; vertex indices are checked before the first load.
#pragma once
#include <math.h>
#include "eval_common.h"

namespace mesh_raster {

constexpr int LANE_MAX_PIXELS = 16;
constexpr int WAVE_MAX_PIXELS = 4096;
constexpr int COOP_BLOCKS = 512;  // workgroups per view of the cooperative kernel (4 waves each)

struct Frame {
    double fx, fy, cx, cy, near_z, far_z;
    int W, H;
};

struct Setup {
    double e0[3], e1[3], e2[3];  // cross(b, c), cross(c, a), cross(a, b)
    double n[3], na;             // cross(b - a, c - a), dot(n, a)
    int x0, y0, x1, y1;          // the clamped box, inclusive
};

// the per-pixel minimum of the fp32 z bits; `img`: the call's images, one frame after the other
struct DepthSink {
    unsigned* img;
    __device__ __forceinline__ DepthSink view(int v, size_t frame) const { return DepthSink{img + v * frame}; }
    __device__ __forceinline__ void operator()(size_t pixel, unsigned zbits, unsigned) const {
        unsigned* p = img + pixel;
        if (zbits < *p) atomicMin(p, zbits);
    }
};

// the per-pixel minimum of (z bits << 32) | triangle index
struct KeySink {
    u64* img;
    __device__ __forceinline__ KeySink view(int v, size_t frame) const { return KeySink{img + v * frame}; }
    __device__ __forceinline__ void operator()(size_t pixel, unsigned zbits, unsigned tri) const {
        u64* p = img + pixel;
        const u64 key = ((u64)zbits << 32) | (u64)tri;
        if (key < *p) atomicMin(p, key);
    }
};

__device__ __forceinline__ void to_camera(const double* __restrict__ M, const double* p, double* out) {
#pragma unroll
    for (int k = 0; k < 3; k++) out[k] = ((M[4 * k] * p[0] + M[4 * k + 1] * p[1]) + M[4 * k + 2] * p[2]) + M[4 * k + 3];
}

__device__ __forceinline__ void cross3(const double* u, const double* v, double* o) {
    o[0] = u[1] * v[2] - u[2] * v[1];
    o[1] = u[2] * v[0] - u[0] * v[2];
    o[2] = u[0] * v[1] - u[1] * v[0];
}

__device__ __forceinline__ double dot3(const double* u, const double* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

// false: the triangle gives this view nothing (rejected, out of the depth range or off the frame)
__device__ __forceinline__ bool setup_triangle(const double* __restrict__ M, const double* P, const Frame& q, Setup& s) {
    double a[3], b[3], c[3];
    to_camera(M, P, a);
    to_camera(M, P + 3, b);
    to_camera(M, P + 6, c);
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 3; k++) finite = finite && isfinite(a[k]) && isfinite(b[k]) && isfinite(c[k]);
    if (!finite) return false;
    const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    cross3(ab, ac, s.n);
    if (s.n[0] == 0.0 && s.n[1] == 0.0 && s.n[2] == 0.0) return false;
    const double zmin = fmin(a[2], fmin(b[2], c[2])), zmax = fmax(a[2], fmax(b[2], c[2]));
    // a hit lies inside the triangle, so its z lies within [zmin, zmax] up to rounding: the margin is for that rounding
    if (!(zmax >= q.near_z * (1.0 - 1e-6) && zmin <= q.far_z * (1.0 + 1e-6))) return false;
    s.na = dot3(s.n, a);
    cross3(b, c, s.e0);
    cross3(c, a, s.e1);
    cross3(a, b, s.e2);
    // The box: a hit has z >= near, so it lies in the part of the triangle at z >= zc, zc a shade below near.  That part's
    // corners -- the vertices at z >= zc and the points where an edge crosses z = zc -- all project, and the covered centres lie
    // within their box.
    const double zc = q.near_z * (1.0 - 1e-6);
    const double* V[3] = {a, b, c};
    double ulo = INFINITY, uhi = -INFINITY, vlo = INFINITY, vhi = -INFINITY;
    bool nan = false;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double *p = V[k], *n = V[(k + 1) % 3];
        double x = p[0], y = p[1], z = p[2];
#pragma unroll
        for (int pass = 0; pass < 2; pass++) {
            if (pass == 0 ? p[2] >= zc : (p[2] >= zc) != (n[2] >= zc)) {
                if (pass == 1) {
                    const double t = (zc - p[2]) / (n[2] - p[2]);
                    x = p[0] + t * (n[0] - p[0]), y = p[1] + t * (n[1] - p[1]), z = zc;
                }
                const double u = q.fx * x / z + q.cx, v = q.fy * y / z + q.cy;
                nan = nan || u != u || v != v;
                ulo = fmin(ulo, u), uhi = fmax(uhi, u), vlo = fmin(vlo, v), vhi = fmax(vhi, v);
            }
        }
    }
    s.x0 = 0, s.y0 = 0, s.x1 = q.W - 1, s.y1 = q.H - 1;
    if (!nan) {
        // centres i + 0.5 within [ulo, uhi], widened by 1e-6 pixel and outwards to whole pixels; clamped while still double
        const double xl = fmax(floor(ulo - 0.5 - 1e-6), 0.0), xh = fmin(ceil(uhi - 0.5 + 1e-6), (double)(q.W - 1));
        const double yl = fmax(floor(vlo - 0.5 - 1e-6), 0.0), yh = fmin(ceil(vhi - 0.5 + 1e-6), (double)(q.H - 1));
        if (!(xl <= xh && yl <= yh)) return false;
        s.x0 = (int)xl, s.x1 = (int)xh, s.y0 = (int)yl, s.y1 = (int)yh;
    }
    return true;
}

// the ray through the centre of pixel (i, j)
__device__ __forceinline__ void pixel_ray(const Frame& q, int i, int j, double* r) {
    r[0] = ((double)i + 0.5 - q.cx) / q.fx, r[1] = ((double)j + 0.5 - q.cy) / q.fy, r[2] = 1.0;
}

// pixel (i, j) of the frame, 0 <= i < W, 0 <= j < H; tri: the triangle's index
template <class Sink>
__device__ __forceinline__ void test_pixel(const Setup& s, const Frame& q, int i, int j, unsigned tri, const Sink& sink) {
    double r[3];
    pixel_ray(q, i, j, r);
    const double w0 = dot3(s.e0, r), w1 = dot3(s.e1, r), w2 = dot3(s.e2, r);
    const bool pos = w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0, neg = w0 <= 0.0 && w1 <= 0.0 && w2 <= 0.0;
    if (!(pos || neg) || (w0 == 0.0 && w1 == 0.0 && w2 == 0.0)) return;
    const double z = s.na / dot3(s.n, r);
    if (!(z >= q.near_z && z <= q.far_z)) return;  // NaN fails
    sink((size_t)j * q.W + i, __float_as_uint((float)z), tri);
}

// the slot of each wanting lane in a list that grows by `counter`: one atomic per wave
__device__ __forceinline__ unsigned wave_append(bool want, unsigned* counter, int lane) {
    const u64 m = __ballot(want);
    if (m == 0) return 0;
    const int leader = __ffsll((long long)m) - 1;
    unsigned base = 0;
    if (lane == leader) base = atomicAdd(counter, (unsigned)__popcll(m));
    base = __shfl(base, leader, 64);
    return base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
}

// triangle t's three vertex ids -> id; false: one of them is outside [0, nv), and no vertex may be loaded through them
__device__ __forceinline__ bool load_ids(const int* __restrict__ tris, long long t, long long nv, int* id) {
#pragma unroll
    for (int k = 0; k < 3; k++) id[k] = tris[3 * (size_t)t + k];
    return ids_in_range(id[0], id[1], id[2], nv);
}

__device__ __forceinline__ void load_triangle(const double* __restrict__ verts, const int* __restrict__ tris, long long t, double* P) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double* v = verts + 3 * (size_t)tris[3 * t + k];
        P[3 * k] = v[0], P[3 * k + 1] = v[1], P[3 * k + 2] = v[2];
    }
}

// lists: n_views x nt slots, view v's wave entries from slot 0 up, its workgroup entries from slot nt - 1 down;
// counts: n_views x 2 (wave entries, workgroup entries)
template <class Sink>
__global__ void __launch_bounds__(256) raster_triangles_kernel(long long nv, const double* __restrict__ verts, long long nt,
                                                               const int* __restrict__ tris, int n_views,
                                                               const double* __restrict__ w2c, Frame q, Sink sink,
                                                               unsigned* __restrict__ lists, unsigned* __restrict__ counts,
                                                               int* __restrict__ err) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    double P[9];
    bool ok = false;
    if (t < nt) {
        ok = tri_in_range(tris[3 * t], tris[3 * t + 1], tris[3 * t + 2], nv, err);
        if (ok) load_triangle(verts, tris, t, P);
    }
    const size_t frame = (size_t)q.W * q.H;
    for (int v = 0; v < n_views; v++) {  // the same trip count in every lane: the ballots below meet whole waves
        int kind = 0;
        Setup s;
        if (ok && setup_triangle(w2c + 16 * (size_t)v, P, q, s)) {
            const long long area = (long long)(s.x1 - s.x0 + 1) * (s.y1 - s.y0 + 1);
            if (area <= LANE_MAX_PIXELS) {
                const Sink im = sink.view(v, frame);
                for (int j = s.y0; j <= s.y1; j++)
                    for (int i = s.x0; i <= s.x1; i++) test_pixel(s, q, i, j, (unsigned)t, im);
            } else {
                kind = area <= WAVE_MAX_PIXELS ? 1 : 2;
            }
        }
        unsigned* list = lists + (size_t)v * nt;
        const unsigned k1 = wave_append(kind == 1, counts + 2 * v, lane);
        if (kind == 1) list[k1] = (unsigned)t;
        const unsigned k2 = wave_append(kind == 2, counts + 2 * v + 1, lane);
        if (kind == 2) list[nt - 1 - k2] = (unsigned)t;
    }
}

template <class Sink>
__global__ void __launch_bounds__(256) raster_cooperative_kernel(const double* __restrict__ verts, long long nt,
                                                                 const int* __restrict__ tris, const double* __restrict__ w2c, Frame q,
                                                                 Sink sink, const unsigned* __restrict__ lists,
                                                                 const unsigned* __restrict__ counts) {
    const int v = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned* list = lists + (size_t)v * nt;
    const unsigned n_wave = counts[2 * v], n_group = counts[2 * v + 1];  // n_wave + n_group <= nt
    const Sink im = sink.view(v, (size_t)q.W * q.H);
    const double* M = w2c + 16 * (size_t)v;
    double P[9];
    Setup s;
    for (unsigned k = blockIdx.x * 4 + wave; k < n_wave; k += gridDim.x * 4) {
        const unsigned t = list[k];
        load_triangle(verts, tris, t, P);
        if (!setup_triangle(M, P, q, s)) continue;  // (it passed once already: the same arithmetic)
        const unsigned bw = (unsigned)(s.x1 - s.x0 + 1), area = bw * (unsigned)(s.y1 - s.y0 + 1);
        for (unsigned idx = lane; idx < area; idx += 64) test_pixel(s, q, s.x0 + (int)(idx % bw), s.y0 + (int)(idx / bw), t, im);
    }
    for (unsigned k = 0; k < n_group; k++) {
        const unsigned t = list[nt - 1 - k];
        load_triangle(verts, tris, t, P);
        if (!setup_triangle(M, P, q, s)) continue;
        const unsigned bw = (unsigned)(s.x1 - s.x0 + 1), area = bw * (unsigned)(s.y1 - s.y0 + 1);  // <= W H <= 2^31 - 1
        const unsigned chunks = (area + 255u) / 256u;
        // chunk c of entry k belongs to workgroup (c + k) mod gridDim.x: entries of few chunks spread over the row
        for (unsigned c = (blockIdx.x + gridDim.x - k % gridDim.x) % gridDim.x; c < chunks; c += gridDim.x) {
            const unsigned idx = c * 256u + threadIdx.x;
            if (idx < area) test_pixel(s, q, s.x0 + (int)(idx % bw), s.y0 + (int)(idx / bw), t, im);
        }
    }
}

// ---- host side: the workspace both units carve, the frame check, the two launches ----

struct RasterWs {
    int* err;          // 1: a vertex index out of range
    unsigned* counts;  // n_views x 2
    unsigned* lists;   // n_views x n_tris
    size_t bytes;
};
static inline RasterWs carve_raster(char* base, long long nt, int n_views) {
    Carver c{base, 0};
    RasterWs w;
    w.err = c.take<int>(1);
    w.counts = c.take<unsigned>(2 * (size_t)n_views);
    w.lists = c.take<unsigned>((size_t)n_views * (size_t)nt);
    w.bytes = c.off;
    return w;
}

static inline bool frame_ok(int n_views, long long W, long long H, double fx, double fy, double cx, double cy) {
    // the grid's y extent, 32-bit pixel indices within a view, a launch over every pixel of the call
    return n_views >= 0 && n_views <= 65535 && W >= 1 && H >= 1 && W <= 0x7FFFFFFFll && H <= 0x7FFFFFFFll && W * H <= 0x7FFFFFFFll &&
           (long long)n_views * W * H <= MAX_LAUNCH && isfinite(fx) && isfinite(fy) && isfinite(cx) && isfinite(cy) && fx != 0.0 && fy != 0.0;
}

// Clears the workspace's flag and counters and rasterizes into `sink`, whose images the caller has set to all ones.
// n_tris, n_verts <= 2^31 - 1.  The flag is left in w.err for the caller to read back.
template <class Sink>
static inline int raster_launch(long long n_verts, const double* verts, long long n_tris, const int* tris, int n_views,
                                const double* w2c, const Frame& q, const RasterWs& w, Sink sink, hipStream_t s) {
    if (hipMemsetAsync(w.err, 0, sizeof(int), s) != hipSuccess) return GS2M_ERR_HIP;
    if (n_views > 0 && hipMemsetAsync(w.counts, 0, sizeof(unsigned) * 2 * (size_t)n_views, s) != hipSuccess) return GS2M_ERR_HIP;
    if (n_tris > 0) {  // (also with no view: the indices are checked)
        raster_triangles_kernel<Sink><<<blocks_of(n_tris), 256, 0, s>>>(n_verts, verts, n_tris, tris, n_views, w2c, q, sink, w.lists, w.counts, w.err);
        if (n_views > 0)
            raster_cooperative_kernel<Sink><<<dim3(COOP_BLOCKS, (unsigned)n_views), 256, 0, s>>>(verts, n_tris, tris, w2c, q, sink, w.lists, w.counts);
    }
    return GS2M_OK;
}

}  // namespace mesh_raster
