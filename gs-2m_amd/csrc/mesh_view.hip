// Mesh visualisation: the visibility buffer, the vertex normals and the headlight shade of include/gs2m_meshview.h
// (the contract: DESIGN.md §16).
//
// Visibility: the shared rasterizer core of mesh_raster.h on the sample frame (H ss, W ss), with the sink that keeps the 64-bit
// unsigned minimum of (z bits << 32) | triangle index.  The buffer starts as all ones and stays so where nothing reaches.
// Normals: a thread per triangle adds the unit face normal in 2^-32 units to the three vertices' int64 sums (integer atomics:
// exact, whatever the order), then a thread per vertex normalises.
// Shade: a thread per output pixel walks its ss x ss keys in row-major order; per covered sample it gathers the triangle's three
// indices and vertices (84 bytes; neighbours mostly share the triangle, so the loads hit the cache), recomputes the barycentrics
// at the sample's ray, shades, and at the end writes the four bytes.  Keys are not trusted: a triangle index or a vertex index
// out of range makes the sample empty.  All fp64, as written.
// G-buffer: a thread per sample runs the same per-sample code as the shade (sample_surface) and writes the world-space
// normal and view direction and the interpolated vertex attributes, rounded once to fp32, for a shading done elsewhere; Resolve RGB:
// a thread per output pixel applies the Resolve paragraph to such shaded samples.
// Textured G-buffer: the same thread per sample interpolates the triangle's UVs instead of vertex attributes and
// reads the 8-bit textures bilinearly, the bytes decoded through a 256-entry table in LDS (one pow per entry and block instead of
// twelve per sample); the normal map is decoded in the tangent frame of tangent_frame.h at the sample's world-space normal.
#include <math.h>
#include "eval_common.h"
#include "mesh_raster.h"
#include "srgb_encode.h"
#include "tangent_frame.h"
#include "../../include/gs2m_atlas.h"
#include "../../include/gs2m_meshview.h"

using namespace mesh_raster;

namespace {

constexpr u64 EMPTY_KEY = ~0ull;
constexpr double FIX = 4294967296.0;  // 2^32: the unit of the normal sums

__global__ void __launch_bounds__(256) normal_sums_kernel(long long nv, const double* __restrict__ verts, long long nt,
                                                          const int* __restrict__ tris, u64* __restrict__ sums, int* __restrict__ err) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const int ia = tris[3 * t], ib = tris[3 * t + 1], ic = tris[3 * t + 2];
    if (!tri_in_range(ia, ib, ic, nv, err)) return;
    double P[9], n[3];
    load_triangle(verts, tris, t, P);
    const double ab[3] = {P[3] - P[0], P[4] - P[1], P[5] - P[2]}, ac[3] = {P[6] - P[0], P[7] - P[1], P[8] - P[2]};
    cross3(ab, ac, n);
    if (n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0) return;
    const double len = sqrt(dot3(n, n));
    const double u[3] = {n[0] / len, n[1] / len, n[2] / len};
    if (!(isfinite(u[0]) && isfinite(u[1]) && isfinite(u[2]))) return;
    const int id[3] = {ia, ib, ic};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const u64 q = (u64)llrint(u[k] * FIX);  // |u| <= 1: two's complement sums of at most 2^31 terms stay within int64
        if (q == 0) continue;
#pragma unroll
        for (int j = 0; j < 3; j++) atomicAdd(sums + 3 * (size_t)id[j] + k, q);
    }
}

__global__ void __launch_bounds__(256) normalise_kernel(long long nv, const long long* __restrict__ sums, double* __restrict__ normals) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const long long q[3] = {sums[3 * i], sums[3 * i + 1], sums[3 * i + 2]};
    double o[3] = {0.0, 0.0, 0.0};
    if (q[0] != 0 || q[1] != 0 || q[2] != 0) {
        const double s[3] = {(double)q[0], (double)q[1], (double)q[2]};
        const double len = sqrt(dot3(s, s));
        o[0] = s[0] / len, o[1] = s[1] / len, o[2] = s[2] / len;
    }
    normals[3 * i] = o[0], normals[3 * i + 1] = o[1], normals[3 * i + 2] = o[2];
}

struct Shade {
    const double* normals;  // null: flat
    const float* colors;    // null: base
    double base[3], ambient, diffuse;
    int srgb, ss;
};

// The Shade paragraph up to the normal, for sample (i, j) of the sample frame q with key `key`: the triangle's vertex indices, the
// sample's ray, the barycentrics and N in camera space (smooth where `normals` is given and usable, else flat).  false: the
// sample is empty, or its key names a triangle or a vertex out of range.
__device__ __forceinline__ bool sample_surface(long long nv, const double* __restrict__ verts, long long nt, const int* __restrict__ tris,
                                               const double* __restrict__ M, const Frame& q, const double* __restrict__ normals, u64 key,
                                               int i, int j, int* id, double* r, double* l, double* N) {
    if (key == EMPTY_KEY) return false;
    const long long t = (long long)(key & 0xFFFFFFFFull);
    if (t >= nt) return false;
    if (!load_ids(tris, t, nv, id)) return false;
    double P[9], a[3], b[3], c[3], x[3];
    load_triangle(verts, tris, t, P);
    to_camera(M, P, a);
    to_camera(M, P + 3, b);
    to_camera(M, P + 6, c);
    pixel_ray(q, i, j, r);
    cross3(b, c, x);
    const double e0 = dot3(x, r);
    cross3(c, a, x);
    const double e1 = dot3(x, r);
    cross3(a, b, x);
    const double e2 = dot3(x, r);
    const double s = (e0 + e1) + e2;
    l[0] = e0 / s, l[1] = e1 / s, l[2] = e2 / s;
    const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    cross3(ab, ac, N);
    if (normals) {
        double S[3];
        bool ok = true;
        double C3[3][3];
#pragma unroll
        for (int w = 0; w < 3; w++) {
            const double* nw = normals + 3 * (size_t)id[w];
            const double n0 = nw[0], n1 = nw[1], n2 = nw[2];
            ok = ok && !(n0 == 0.0 && n1 == 0.0 && n2 == 0.0);
#pragma unroll
            for (int d = 0; d < 3; d++) C3[w][d] = (M[4 * d] * n0 + M[4 * d + 1] * n1) + M[4 * d + 2] * n2;
        }
#pragma unroll
        for (int d = 0; d < 3; d++) S[d] = (l[0] * C3[0][d] + l[1] * C3[1][d]) + l[2] * C3[2][d];
        ok = ok && isfinite(S[0]) && isfinite(S[1]) && isfinite(S[2]) && !(S[0] == 0.0 && S[1] == 0.0 && S[2] == 0.0);
        if (ok) N[0] = S[0], N[1] = S[1], N[2] = S[2];
    }
    return true;
}

// q: the SAMPLE frame; W, H: the output frame
__global__ void __launch_bounds__(256) shade_kernel(long long nv, const double* __restrict__ verts, long long nt,
                                                    const int* __restrict__ tris, const double* __restrict__ w2c, Frame q, int W, int H,
                                                    const u64* __restrict__ vis, Shade sh, unsigned char* __restrict__ rgba,
                                                    float* __restrict__ depth, int* __restrict__ tri_id) {
    const int v = blockIdx.y;
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (long long)W * H) return;
    const int px = (int)(pix % W), py = (int)(pix / W);
    const int ss = sh.ss;
    const double* M = w2c + 16 * (size_t)v;
    const u64* keys = vis + (size_t)v * q.W * q.H;
    double sum[3] = {0.0, 0.0, 0.0};
    int m = 0;
    float zc = 0.f;
    int tc = -1;
    for (int k = 0; k < ss * ss; k++) {
        const int i = px * ss + k % ss, j = py * ss + k / ss;
        const u64 key = keys[(size_t)j * q.W + i];
        int id[3];
        double r[3], l[3], N[3];
        if (!sample_surface(nv, verts, nt, tris, M, q, sh.normals, key, i, j, id, r, l, N)) continue;
        const double l0 = l[0], l1 = l[1], l2 = l[2];
        const double cosv = fabs(dot3(N, r)) / sqrt(dot3(N, N) * dot3(r, r));
        const double light = sh.ambient + sh.diffuse * cosv;
#pragma unroll
        for (int d = 0; d < 3; d++) {
            double alb = sh.base[d];
            if (sh.colors)
                alb = (l0 * (double)sh.colors[3 * (size_t)id[0] + d] + l1 * (double)sh.colors[3 * (size_t)id[1] + d]) +
                      l2 * (double)sh.colors[3 * (size_t)id[2] + d];
            sum[d] = sum[d] + fmin(fmax(alb * light, 0.0), 1.0);
        }
        m++;
        if (k == (ss / 2) * (ss + 1)) zc = __uint_as_float((unsigned)(key >> 32)), tc = (int)(key & 0xFFFFFFFFull);
    }
    const size_t o = (size_t)v * W * H + (size_t)pix;
    uchar4 out = make_uchar4(0, 0, 0, 0);
    if (m > 0) {
        unsigned char by[3];
#pragma unroll
        for (int d = 0; d < 3; d++) by[d] = (unsigned char)floor(255.0 * encode(sum[d] / (double)m, sh.srgb) + 0.5);
        out = make_uchar4(by[0], by[1], by[2], (unsigned char)floor(255.0 * (double)m / (double)(ss * ss) + 0.5));
    }
    reinterpret_cast<uchar4*>(rgba)[o] = out;
    if (depth) depth[o] = zc;
    if (tri_id) tri_id[o] = tc;
}

// ---- G-buffer and resolve of shaded samples ----

struct GBuffer {
    float *normal, *view_dir, *albedo, *roughness, *metallic;
    unsigned char* coverage;
};

// through the transposed rotation rows of the view: camera space to world space
__device__ __forceinline__ void to_world_dir(const double* __restrict__ M, const double* c, double* o) {
#pragma unroll
    for (int k = 0; k < 3; k++) o[k] = (M[k] * c[0] + M[4 + k] * c[1]) + M[8 + k] * c[2];
}

// a thread per sample of the SAMPLE frame q; every output of an empty sample is 0
__global__ void __launch_bounds__(256) gbuffer_kernel(long long nv, const double* __restrict__ verts, long long nt,
                                                      const int* __restrict__ tris, const double* __restrict__ w2c, Frame q,
                                                      const u64* __restrict__ vis, const double* __restrict__ normals,
                                                      const float* __restrict__ albedo, const float* __restrict__ roughness,
                                                      const float* __restrict__ metallic, GBuffer g) {
    const int v = blockIdx.y;
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long frame = (long long)q.W * q.H;
    if (pix >= frame) return;
    const int i = (int)(pix % q.W), j = (int)(pix / q.W);
    const double* M = w2c + 16 * (size_t)v;
    const size_t o = (size_t)v * frame + (size_t)pix;
    int id[3];
    double r[3], l[3], N[3];
    float out[11];
#pragma unroll
    for (int k = 0; k < 11; k++) out[k] = 0.f;
    const bool hit = sample_surface(nv, verts, nt, tris, M, q, normals, vis[o], i, j, id, r, l, N);
    if (hit) {
        double Nw[3], Vw[3];
        const double back[3] = {-r[0], -r[1], -r[2]};
        if (dot3(N, r) > 0.0) N[0] = -N[0], N[1] = -N[1], N[2] = -N[2];  // towards the eye
        to_world_dir(M, N, Nw);
        to_world_dir(M, back, Vw);
        const double nl = sqrt(dot3(Nw, Nw)), vl = sqrt(dot3(Vw, Vw));
#pragma unroll
        for (int k = 0; k < 3; k++) {
            out[k] = (float)(Nw[k] / nl);
            out[3 + k] = (float)(Vw[k] / vl);
            out[6 + k] = (float)((l[0] * (double)albedo[3 * (size_t)id[0] + k] + l[1] * (double)albedo[3 * (size_t)id[1] + k]) +
                                 l[2] * (double)albedo[3 * (size_t)id[2] + k]);
        }
        out[9] = (float)((l[0] * (double)roughness[id[0]] + l[1] * (double)roughness[id[1]]) + l[2] * (double)roughness[id[2]]);
        out[10] = (float)((l[0] * (double)metallic[id[0]] + l[1] * (double)metallic[id[1]]) + l[2] * (double)metallic[id[2]]);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) g.normal[3 * o + k] = out[k], g.view_dir[3 * o + k] = out[3 + k], g.albedo[3 * o + k] = out[6 + k];
    g.roughness[o] = out[9];
    g.metallic[o] = out[10];
    g.coverage[o] = hit ? 1 : 0;
}

struct Textures {
    const float* uvs;  // (n_tris, 3, 2)
    const unsigned char *base, *orm, *normal;  // (th, tw, 3); orm and normal may be null
    int tw, th, srgb;
};

// the first tap's index along an axis of n texels for the coordinate x = u n - 0.5, kept within [-1, n] (a NaN goes to -1)
// before it becomes an int, and the fraction from the tap's own floor
__device__ __forceinline__ int tap_floor(double x, int n, double* t) {
    const double f = floor(x);
    *t = x - f;
    return (int)(f >= -1.0 ? (f <= (double)n ? f : (double)n) : -1.0);
}
__device__ __forceinline__ int clamp_tap(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// a thread per sample of the SAMPLE frame q, as gbuffer_kernel; lut[b]: base-colour byte b decoded
__global__ void __launch_bounds__(256) gbuffer_textured_kernel(long long nv, const double* __restrict__ verts, long long nt,
                                                               const int* __restrict__ tris, const double* __restrict__ w2c, Frame q,
                                                               const u64* __restrict__ vis, const double* __restrict__ normals, Textures tx,
                                                               GBuffer g) {
    __shared__ double lut[256];
    lut[threadIdx.x] = decode((double)threadIdx.x / 255.0, tx.srgb);
    __syncthreads();
    const int v = blockIdx.y;
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long frame = (long long)q.W * q.H;
    if (pix >= frame) return;
    const int i = (int)(pix % q.W), j = (int)(pix / q.W);
    const double* M = w2c + 16 * (size_t)v;
    const size_t o = (size_t)v * frame + (size_t)pix;
    int id[3];
    double r[3], l[3], N[3];
    float out[11];
#pragma unroll
    for (int k = 0; k < 11; k++) out[k] = 0.f;
    const bool hit = sample_surface(nv, verts, nt, tris, M, q, normals, vis[o], i, j, id, r, l, N);
    if (hit) {
        const long long t = (long long)(vis[o] & 0xFFFFFFFFull);
        double uv[6];
#pragma unroll
        for (int k = 0; k < 6; k++) uv[k] = (double)tx.uvs[6 * (size_t)t + k];
        const double u = (l[0] * uv[0] + l[1] * uv[2]) + l[2] * uv[4], w = (l[0] * uv[1] + l[1] * uv[3]) + l[2] * uv[5];
        double fx, fy;
        const int x0 = tap_floor(u * (double)tx.tw - 0.5, tx.tw, &fx), y0 = tap_floor(w * (double)tx.th - 0.5, tx.th, &fy);
        const double wt[4] = {(1.0 - fx) * (1.0 - fy), fx * (1.0 - fy), (1.0 - fx) * fy, fx * fy};
        size_t tap[4];
#pragma unroll
        for (int k = 0; k < 4; k++) tap[k] = 3 * ((size_t)clamp_tap(y0 + k / 2, tx.th) * tx.tw + clamp_tap(x0 + k % 2, tx.tw));
        double Nw[3], Vw[3], n[3];
        const double back[3] = {-r[0], -r[1], -r[2]};
        to_world_dir(M, back, Vw);
        if (tx.normal) {
            double P[9], m[3], rw[3];
            load_triangle(verts, tris, t, P);
            to_world_dir(M, N, Nw);  // before the flip: the frame is the surface's, not the view's
#pragma unroll
            for (int k = 0; k < 3; k++) {
                double b[4];
#pragma unroll
                for (int c = 0; c < 4; c++) b[c] = (double)tx.normal[tap[c] + k] / 255.0 * 2.0 - 1.0;
                m[k] = ((b[0] * wt[0] + b[1] * wt[1]) + b[2] * wt[2]) + b[3] * wt[3];
            }
            TangentFrame F;
            tangent_frame(P, P + 3, P + 6, uv, Nw, &F);
            tangent_decode(F, m, n);
            to_world_dir(M, r, rw);
            if (dot3(n, rw) > 0.0) n[0] = -n[0], n[1] = -n[1], n[2] = -n[2];
        } else {
            if (dot3(N, r) > 0.0) N[0] = -N[0], N[1] = -N[1], N[2] = -N[2];  // towards the eye
            to_world_dir(M, N, Nw);
            const double nl = sqrt(dot3(Nw, Nw));
#pragma unroll
            for (int k = 0; k < 3; k++) n[k] = Nw[k] / nl;
        }
        const double vl = sqrt(dot3(Vw, Vw));
#pragma unroll
        for (int k = 0; k < 3; k++) {
            out[k] = (float)n[k];
            out[3 + k] = (float)(Vw[k] / vl);
            out[6 + k] = (float)(((lut[tx.base[tap[0] + k]] * wt[0] + lut[tx.base[tap[1] + k]] * wt[1]) + lut[tx.base[tap[2] + k]] * wt[2]) +
                                 lut[tx.base[tap[3] + k]] * wt[3]);
        }
        out[9] = 1.f;
        if (tx.orm) {
#pragma unroll
            for (int k = 1; k < 3; k++)
                out[8 + k] = (float)((((double)tx.orm[tap[0] + k] / 255.0 * wt[0] + (double)tx.orm[tap[1] + k] / 255.0 * wt[1]) +
                                      (double)tx.orm[tap[2] + k] / 255.0 * wt[2]) +
                                     (double)tx.orm[tap[3] + k] / 255.0 * wt[3]);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) g.normal[3 * o + k] = out[k], g.view_dir[3 * o + k] = out[3 + k], g.albedo[3 * o + k] = out[6 + k];
    g.roughness[o] = out[9];
    g.metallic[o] = out[10];
    g.coverage[o] = hit ? 1 : 0;
}

// a thread per output pixel: the Resolve paragraph on per-sample linear RGB
__global__ void __launch_bounds__(256) resolve_rgb_kernel(int W, int H, int ss, const float* __restrict__ rgb,
                                                          const unsigned char* __restrict__ coverage, int srgb,
                                                          const float* __restrict__ background, unsigned char* __restrict__ rgba) {
    const int v = blockIdx.y;
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (long long)W * H) return;
    const int px = (int)(pix % W), py = (int)(pix / W);
    const int Ws = W * ss;
    const size_t base = (size_t)v * Ws * ((size_t)H * ss);
    double sum[3] = {0.0, 0.0, 0.0};
    int m = 0;
    for (int k = 0; k < ss * ss; k++) {
        const size_t s = base + (size_t)(py * ss + k / ss) * Ws + (px * ss + k % ss);
        if (!coverage[s]) continue;
#pragma unroll
        for (int d = 0; d < 3; d++) sum[d] = sum[d] + fmin(fmax((double)rgb[3 * s + d], 0.0), 1.0);
        m++;
    }
    const size_t o = (size_t)v * W * H + (size_t)pix;
    double enc[3] = {0.0, 0.0, 0.0};
    if (m > 0) {
#pragma unroll
        for (int d = 0; d < 3; d++) enc[d] = encode(sum[d] / (double)m, srgb);
    }
    const double a = (double)m / (double)(ss * ss);
    uchar4 out = make_uchar4(0, 0, 0, 0);
    if (background) {
        unsigned char by[3];
#pragma unroll
        for (int d = 0; d < 3; d++) by[d] = (unsigned char)floor(255.0 * (a * enc[d] + (1.0 - a) * fmin(fmax((double)background[3 * o + d], 0.0), 1.0)) + 0.5);
        out = make_uchar4(by[0], by[1], by[2], 255);
    } else if (m > 0) {
        out = make_uchar4((unsigned char)floor(255.0 * enc[0] + 0.5), (unsigned char)floor(255.0 * enc[1] + 0.5),
                          (unsigned char)floor(255.0 * enc[2] + 0.5), (unsigned char)floor(255.0 * a + 0.5));
    }
    reinterpret_cast<uchar4*>(rgba)[o] = out;
}

bool view_frame_ok(int n_views, int W, int H, int ss, double fx, double fy, double cx, double cy) {
    return ss >= 1 && ss <= 4 && W >= 1 && H >= 1 && frame_ok(n_views, (long long)W * ss, (long long)H * ss, fx, fy, cx, cy);
}

}  // namespace

extern "C" {

int gs2m_meshview_workspace_bytes(long long n_tris, int n_views, long long* bytes) {
    if (n_tris < 0 || n_views < 0 || !bytes) return GS2M_ERR_INVALID_ARG;
    if (n_tris > 0x7FFFFFFFll || n_views > 65535) return GS2M_ERR_UNSUPPORTED;
    *bytes = (long long)carve_raster(nullptr, n_tris, n_views).bytes;
    return GS2M_OK;
}

int gs2m_meshview_visibility(long long n_verts, const double* verts, long long n_tris, const int* tris, int n_views,
                             const double* w2c, double fx, double fy, double cx, double cy, int W, int H, int ss, double near_z,
                             double far_z, void* ws, unsigned long long* vis, void* stream) {
    if (n_verts < 0 || n_tris < 0 || n_tris > 0xFFFFFFFEll || !view_frame_ok(n_views, W, H, ss, fx, fy, cx, cy) || !ws)
        return GS2M_ERR_INVALID_ARG;
    if (!(near_z > 0.0 && near_z <= far_z && isfinite(far_z))) return GS2M_ERR_INVALID_ARG;
    if (n_views > 0 && (!w2c || !vis)) return GS2M_ERR_INVALID_ARG;
    if (n_tris > 0 && (!tris || (n_verts > 0 && !verts))) return GS2M_ERR_INVALID_ARG;
    if (n_tris > 0x7FFFFFFFll || n_verts > 0x7FFFFFFFll) return GS2M_ERR_UNSUPPORTED;  // ids are int, list entries 32-bit
    hipStream_t s = (hipStream_t)stream;
    const RasterWs w = carve_raster((char*)ws, n_tris, n_views);
    const Frame q{ss * fx, ss * fy, ss * cx, ss * cy, near_z, far_z, W * ss, H * ss};
    const size_t samples = (size_t)n_views * q.W * q.H;
    if (n_views > 0 && hipMemsetAsync(vis, 0xFF, sizeof(u64) * samples, s) != hipSuccess) return GS2M_ERR_HIP;
    if (raster_launch(n_verts, verts, n_tris, tris, n_views, w2c, q, w, KeySink{(u64*)vis}, s) != GS2M_OK) return GS2M_ERR_HIP;
    int err;
    if (gs2m_read_back(s, {{&err, w.err, sizeof(err)}}) != GS2M_OK) return GS2M_ERR_HIP;
    return err ? GS2M_ERR_INVALID_ARG : GS2M_OK;
}

int gs2m_meshview_normals_workspace_bytes(long long* bytes) {
    if (!bytes) return GS2M_ERR_INVALID_ARG;
    *bytes = GS2M_ALIGN;  // the flag
    return GS2M_OK;
}

int gs2m_meshview_normals(long long n_verts, const double* verts, long long n_tris, const int* tris, void* ws, long long* sums,
                          double* normals, void* stream) {
    if (n_verts < 0 || n_tris < 0 || !ws || (n_verts > 0 && (!verts || !sums || !normals)) || (n_tris > 0 && !tris)) return GS2M_ERR_INVALID_ARG;
    if (n_tris > 0x7FFFFFFFll || n_verts > 0x7FFFFFFFll) return GS2M_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    int* d_err = (int*)ws;
    if (hipMemsetAsync(d_err, 0, sizeof(int), s) != hipSuccess) return GS2M_ERR_HIP;
    if (n_verts > 0 && hipMemsetAsync(sums, 0, sizeof(long long) * 3 * (size_t)n_verts, s) != hipSuccess) return GS2M_ERR_HIP;
    if (n_tris > 0) normal_sums_kernel<<<blocks_of(n_tris), 256, 0, s>>>(n_verts, verts, n_tris, tris, (u64*)sums, d_err);
    if (n_verts > 0) normalise_kernel<<<blocks_of(n_verts), 256, 0, s>>>(n_verts, sums, normals);
    int err;
    if (gs2m_read_back(s, {{&err, d_err, sizeof(err)}}) != GS2M_OK) return GS2M_ERR_HIP;
    return err ? GS2M_ERR_INVALID_ARG : GS2M_OK;
}

int gs2m_meshview_shade(long long n_verts, const double* verts, long long n_tris, const int* tris, int n_views, const double* w2c,
                        double fx, double fy, double cx, double cy, int W, int H, int ss, const unsigned long long* vis,
                        const double* normals, const float* colors, double base_r, double base_g, double base_b, double ambient,
                        double diffuse, int srgb, unsigned char* rgba, float* depth, int* tri_id, void* stream) {
    if (n_verts < 0 || n_tris < 0 || !view_frame_ok(n_views, W, H, ss, fx, fy, cx, cy)) return GS2M_ERR_INVALID_ARG;
    if (n_views > 0 && (!w2c || !vis || !rgba)) return GS2M_ERR_INVALID_ARG;
    if (n_tris > 0 && (!tris || (n_verts > 0 && !verts))) return GS2M_ERR_INVALID_ARG;
    if (n_tris > 0x7FFFFFFFll || n_verts > 0x7FFFFFFFll) return GS2M_ERR_UNSUPPORTED;
    if (n_views == 0) return GS2M_OK;
    const Frame q{ss * fx, ss * fy, ss * cx, ss * cy, 0.0, 0.0, W * ss, H * ss};
    const Shade sh{normals, colors, {base_r, base_g, base_b}, ambient, diffuse, srgb ? 1 : 0, ss};
    shade_kernel<<<dim3(blocks_of((long long)W * H), (unsigned)n_views), 256, 0, (hipStream_t)stream>>>(
        n_verts, verts, n_tris, tris, w2c, q, W, H, (const u64*)vis, sh, rgba, depth, tri_id);
    return gs2m_status(hipGetLastError());
}

int gs2m_meshview_gbuffer(long long n_verts, const double* verts, long long n_tris, const int* tris, int n_views, const double* w2c,
                          double fx, double fy, double cx, double cy, int W, int H, int ss, const unsigned long long* vis,
                          const double* normals, const float* albedo, const float* roughness, const float* metallic,
                          float* out_normal, float* out_view_dir, float* out_albedo, float* out_roughness, float* out_metallic,
                          unsigned char* coverage, void* stream) {
    if (n_verts < 0 || n_tris < 0 || !view_frame_ok(n_views, W, H, ss, fx, fy, cx, cy)) return GS2M_ERR_INVALID_ARG;
    if (n_views > 0 && (!w2c || !vis || !out_normal || !out_view_dir || !out_albedo || !out_roughness || !out_metallic || !coverage))
        return GS2M_ERR_INVALID_ARG;
    if (n_tris > 0 && (!tris || (n_verts > 0 && (!verts || !albedo || !roughness || !metallic)))) return GS2M_ERR_INVALID_ARG;
    if (n_tris > 0x7FFFFFFFll || n_verts > 0x7FFFFFFFll) return GS2M_ERR_UNSUPPORTED;
    if (n_views == 0) return GS2M_OK;
    const Frame q{ss * fx, ss * fy, ss * cx, ss * cy, 0.0, 0.0, W * ss, H * ss};
    const GBuffer g{out_normal, out_view_dir, out_albedo, out_roughness, out_metallic, coverage};
    gbuffer_kernel<<<dim3(blocks_of((long long)q.W * q.H), (unsigned)n_views), 256, 0, (hipStream_t)stream>>>(
        n_verts, verts, n_tris, tris, w2c, q, (const u64*)vis, normals, albedo, roughness, metallic, g);
    return gs2m_status(hipGetLastError());
}

int gs2m_meshview_gbuffer_textured(long long n_verts, const double* verts, long long n_tris, const int* tris, const float* uvs, int n_views,
                                   const double* w2c, double fx, double fy, double cx, double cy, int W, int H, int ss,
                                   const unsigned long long* vis, const double* normals, int tw, int th, const unsigned char* base_color,
                                   int srgb, const unsigned char* orm, const unsigned char* normal_map, float* out_normal,
                                   float* out_view_dir, float* out_albedo, float* out_roughness, float* out_metallic,
                                   unsigned char* coverage, void* stream) {
    if (n_verts < 0 || n_tris < 0 || !view_frame_ok(n_views, W, H, ss, fx, fy, cx, cy) || tw < 1 || th < 1) return GS2M_ERR_INVALID_ARG;
    if (n_views > 0 && (!w2c || !vis || !out_normal || !out_view_dir || !out_albedo || !out_roughness || !out_metallic || !coverage))
        return GS2M_ERR_INVALID_ARG;
    if (n_tris > 0 && (!tris || !uvs || !base_color || (n_verts > 0 && !verts))) return GS2M_ERR_INVALID_ARG;
    if (n_tris > 0x7FFFFFFFll || n_verts > 0x7FFFFFFFll || tw > GS2M_ATLAS_MAX_WIDTH || th > GS2M_ATLAS_MAX_WIDTH) return GS2M_ERR_UNSUPPORTED;
    if (n_views == 0) return GS2M_OK;
    const Frame q{ss * fx, ss * fy, ss * cx, ss * cy, 0.0, 0.0, W * ss, H * ss};
    const GBuffer g{out_normal, out_view_dir, out_albedo, out_roughness, out_metallic, coverage};
    const Textures tx{uvs, base_color, orm, normal_map, tw, th, srgb ? 1 : 0};
    gbuffer_textured_kernel<<<dim3(blocks_of((long long)q.W * q.H), (unsigned)n_views), 256, 0, (hipStream_t)stream>>>(
        n_verts, verts, n_tris, tris, w2c, q, (const u64*)vis, normals, tx, g);
    return gs2m_status(hipGetLastError());
}

int gs2m_meshview_resolve_rgb(int n_views, int W, int H, int ss, const float* rgb, const unsigned char* coverage, int srgb,
                              const float* background, unsigned char* rgba, void* stream) {
    if (!view_frame_ok(n_views, W, H, ss, 1.0, 1.0, 0.0, 0.0)) return GS2M_ERR_INVALID_ARG;
    if (n_views > 0 && (!rgb || !coverage || !rgba)) return GS2M_ERR_INVALID_ARG;
    if (n_views == 0) return GS2M_OK;
    resolve_rgb_kernel<<<dim3(blocks_of((long long)W * H), (unsigned)n_views), 256, 0, (hipStream_t)stream>>>(
        W, H, ss, rgb, coverage, srgb ? 1 : 0, background, rgba);
    return gs2m_status(hipGetLastError());
}

}  // extern "C"
