// Attribute bakes: the views' attribute maps averaged onto the mesh's vertices, or onto the texels of its atlas
// (include/gs2m_meshbake.h; the contracts: DESIGN.md §20 and §22).
//
// Accumulate: a thread per point -- a vertex, or a texel's point on its triangle -- keeps its position, its normal and its C + 1
// running sums in registers and walks the views of the call in order (bake_views.h: the views staged in LDS, the projection and
// the taps of vertex_project.h); a wave's lanes are 64 neighbouring vertices, or 64 texels of a row, which within a cell are
// neighbours on the surface, so their taps share lines.  The kernels are instantiated per C so that the sums are registers.
// One thread owns a point: no atomics, and the order of the additions is the order of the views.
// Resolve: a thread per point.  An unseen texel reads its triangle's per-vertex attributes at the chart's barycentrics
// (atlas_layout.h), recomputed from the triangle's cell rather than stored per texel.
// Pack: a thread per texel, two 8-bit images.
// Normals: a thread per texel builds the tangent frame of its triangle at its interpolated normal (tangent_frame.h) and encodes
// the baked world normal in it.
#include <math.h>
#include "eval_common.h"
#include "mesh_raster.h"
#include "bake_views.h"
#include "atlas_layout.h"
#include "srgb_encode.h"
#include "tangent_frame.h"
#include "../../include/gs2m_meshbake.h"

using namespace mesh_raster;

namespace {

constexpr int BAKE_CMAX = 8;

// owner: null = every point below n is owned (the vertex bake); else a point with owner[i] < 0 -- an empty texel -- has no point: it
// walks no view and its sums are 0.
template <int C>
__global__ void __launch_bounds__(256) bake_kernel(long long n, const double* __restrict__ points, const double* __restrict__ normals,
                                                   const int* __restrict__ owner, BakeViews views, int accumulate,
                                                   double* __restrict__ sums, double* __restrict__ weights) {
    __shared__ double s_m[BAKE_CHUNK][BAKE_ROW];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n;
    const bool owned = live && (!owner || owner[i] >= 0);
    double p[3] = {0.0, 0.0, 0.0}, N[3] = {0.0, 0.0, 0.0}, nn = 0.0;
    bool lit = owned;  // false: every view weighs 0
    if (owned) {
#pragma unroll
        for (int k = 0; k < 3; k++) p[k] = points[3 * i + k];
        if (normals) {
#pragma unroll
            for (int k = 0; k < 3; k++) N[k] = normals[3 * i + k];
            nn = dot3(N, N);
            lit = normal_ok(N);
        }
    }
    double acc[C], wsum = 0.0;
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = 0.0;
    if (owned && accumulate) {
#pragma unroll
        for (int c = 0; c < C; c++) acc[c] = sums[(size_t)i * C + c];
        wsum = weights[i];
    }
    bake_views<C>(views, lit, p, normals != nullptr, N, nn, s_m, acc, wsum);  // every thread: it holds barriers
    if (live) {
#pragma unroll
        for (int c = 0; c < C; c++) sums[(size_t)i * C + c] = acc[c];
        weights[i] = wsum;
    }
}

struct Fallback {
    float v[BAKE_CMAX];
};

// owner: null = every point is owned and none has a triangle (the vertex bake); else point i of the call is texel
// (i % width, row0 + i / width) of the atlas.  attrs: null = a point no view reached takes the fallback.
__global__ void __launch_bounds__(256) resolve_kernel(long long n, int C, int width, int row0, const double* __restrict__ sums,
                                                      const double* __restrict__ weights, double min_weight, Fallback fb,
                                                      const int* __restrict__ owner, long long nt, const int* __restrict__ tris,
                                                      const int* __restrict__ cells, long long nv, const float* __restrict__ attrs,
                                                      float* __restrict__ out, unsigned char* __restrict__ seen) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int t = owner ? owner[i] : 0;
    const double w = t >= 0 ? weights[i] : 0.0;
    const bool ok = w >= min_weight && w > 0.0;
    seen[i] = ok ? 1 : 0;
    if (ok) {
        for (int c = 0; c < C; c++) out[(size_t)i * C + c] = (float)(sums[(size_t)i * C + c] / w);
        return;
    }
    bool from_vertices = false;
    double l[3] = {0.0, 0.0, 0.0};
    int id[3] = {0, 0, 0};
    if (attrs && owner && t >= 0 && t < nt) {
        const int* cell = cells + 4 * (size_t)t;
        const int side = cell[2], half = cell[3];
        const int li = (int)(i % width) - cell[0], lj = row0 + (int)(i / width) - cell[1];
        from_vertices = load_ids(tris, t, nv, id) && side >= 8 && side <= 256 && (half == 0 || half == 1) && li >= 0 && lj >= 0 && li < side &&
                        lj < side;
        if (from_vertices) atlas_bary(side, half, li, lj, l);
    }
    for (int c = 0; c < C; c++) {
        float x = fb.v[c];
        if (from_vertices)
            x = (float)((l[0] * (double)attrs[(size_t)id[0] * C + c] + l[1] * (double)attrs[(size_t)id[1] * C + c]) +
                        l[2] * (double)attrs[(size_t)id[2] * C + c]);
        out[(size_t)i * C + c] = x;
    }
}

__device__ __forceinline__ double clamp01(double x) { return x > 0.0 ? (x < 1.0 ? x : 1.0) : 0.0; }  // NaN -> 0
__device__ __forceinline__ unsigned char to_byte(double x) { return (unsigned char)floor(255.0 * x + 0.5); }  // x in [0, 1]

__global__ void __launch_bounds__(256) texture_pack_kernel(long long n, int C, const float* __restrict__ values, int srgb,
                                                           unsigned char* __restrict__ base, unsigned char* __restrict__ orm) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* v = values + (size_t)i * C;
    for (int d = 0; d < 3; d++) base[3 * (size_t)i + d] = to_byte(encode(clamp01((double)v[d]), srgb));  // clamped, then encoded
    if (orm) {
        orm[3 * (size_t)i] = 255;
        orm[3 * (size_t)i + 1] = to_byte(clamp01((double)v[3]));
        orm[3 * (size_t)i + 2] = to_byte(clamp01((double)v[4]));
    }
}

// values: the resolved planes of the texel, the normal's three from `offset` on
__global__ void __launch_bounds__(256) texture_normals_kernel(long long n, const int* __restrict__ owner, const double* __restrict__ tnormals,
                                                              long long nt, const int* __restrict__ tris, const float* __restrict__ uvs,
                                                              long long nv, const double* __restrict__ verts, int C, int offset,
                                                              const float* __restrict__ values, unsigned char* __restrict__ normal_map,
                                                              double* __restrict__ tangent) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double m[3] = {0.0, 0.0, 1.0};
    const int t = owner[i];
    if (t >= 0 && t < nt) {
        int id[3];
        if (load_ids(tris, t, nv, id)) {
            double P[9], uv[6], N[3], w[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
#pragma unroll
                for (int d = 0; d < 3; d++) P[3 * k + d] = verts[3 * (size_t)id[k] + d];
                uv[2 * k] = (double)uvs[6 * (size_t)t + 2 * k], uv[2 * k + 1] = (double)uvs[6 * (size_t)t + 2 * k + 1];
                N[k] = tnormals[3 * (size_t)i + k];
                w[k] = (double)values[(size_t)i * C + offset + k];
            }
            TangentFrame F;
            tangent_frame(P, P + 3, P + 6, uv, N, &F);
            tangent_encode(F, w, m);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        normal_map[3 * (size_t)i + k] = tangent_byte(m[k]);
        if (tangent) tangent[3 * (size_t)i + k] = m[k];
    }
}

int views_status(int n_views, double fx, double fy, double cx, double cy, int W, int H, const double* w2c, const float* depth, int C,
                 const float* maps, double eps) {
    if (C < 1 || C > BAKE_CMAX || !frame_ok(n_views, W, H, fx, fy, cx, cy) || eps != eps) return GS2M_ERR_INVALID_ARG;
    if (n_views > 0 && (!w2c || !depth || !maps)) return GS2M_ERR_INVALID_ARG;
    return GS2M_OK;
}

// points: vertices (texels false: no owner) or texels with their owner
int bake_accumulate(bool texels, long long n, const double* points, const double* normals, const int* owner, int n_views, const double* w2c,
                    double fx, double fy, double cx, double cy, int W, int H, const float* depth, int C, const float* maps, const float* mask,
                    double eps, int accumulate, double* sums, double* weights, void* stream) {
    if (n < 0 || views_status(n_views, fx, fy, cx, cy, W, H, w2c, depth, C, maps, eps) != GS2M_OK) return GS2M_ERR_INVALID_ARG;
    if (n > 0 && (!points || (texels && !owner) || !sums || !weights)) return GS2M_ERR_INVALID_ARG;
    if (n == 0) return GS2M_OK;
    if (n > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    if ((long long)n_views * C * W * H > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    const BakeViews views{n_views, w2c, Frame{fx, fy, cx, cy, 0.0, 0.0, W, H}, depth, maps, mask, eps};
    hipStream_t s = (hipStream_t)stream;
#define BAKE_CASE(c) \
    case c: bake_kernel<c><<<blocks_of(n), 256, 0, s>>>(n, points, normals, owner, views, accumulate, sums, weights); break;
    switch (C) {
        BAKE_CASE(1) BAKE_CASE(2) BAKE_CASE(3) BAKE_CASE(4) BAKE_CASE(5) BAKE_CASE(6) BAKE_CASE(7) BAKE_CASE(8)
    }
#undef BAKE_CASE
    return gs2m_status(hipGetLastError());
}

// texels false: no owner, no attributes, and the atlas arguments are unused
int bake_resolve(bool texels, long long n, int C, int width, int row0, const double* sums, const double* weights, double min_weight,
                 const float* fallback, const int* owner, long long n_triangles, const int* triangles, const int* cells, long long n_verts,
                 const float* attributes, float* out, unsigned char* seen, void* stream) {
    if (n < 0 || C < 1 || C > BAKE_CMAX || min_weight != min_weight || !fallback || width < 1 || row0 < 0 || n_triangles < 0 || n_verts < 0)
        return GS2M_ERR_INVALID_ARG;
    if (n > 0 && (!sums || !weights || (texels && !owner) || !out || !seen)) return GS2M_ERR_INVALID_ARG;
    if (attributes && (!triangles || !cells)) return GS2M_ERR_INVALID_ARG;
    if (n == 0) return GS2M_OK;
    if (n > MAX_LAUNCH || (texels && (n + width - 1) / width + row0 > 0x7FFFFFFFll)) return GS2M_ERR_UNSUPPORTED;
    Fallback fb{};
    for (int c = 0; c < C; c++) fb.v[c] = fallback[c];
    resolve_kernel<<<blocks_of(n), 256, 0, (hipStream_t)stream>>>(n, C, width, row0, sums, weights, min_weight, fb, owner, n_triangles, triangles,
                                                                  cells, n_verts, attributes, out, seen);
    return gs2m_status(hipGetLastError());
}

}  // namespace

extern "C" {

int gs2m_meshbake_accumulate(long long n_verts, const double* verts, const double* normals, int n_views, const double* w2c,
                             double fx, double fy, double cx, double cy, int W, int H, const float* depth, int C, const float* maps,
                             const float* mask, double eps, int accumulate, double* sums, double* weights, void* stream) {
    return bake_accumulate(false, n_verts, verts, normals, nullptr, n_views, w2c, fx, fy, cx, cy, W, H, depth, C, maps, mask, eps, accumulate, sums,
                        weights, stream);
}

int gs2m_meshbake_resolve(long long n_verts, int C, const double* sums, const double* weights, double min_weight,
                          const float* fallback, float* out, unsigned char* seen, void* stream) {
    return bake_resolve(false, n_verts, C, 1, 0, sums, weights, min_weight, fallback, nullptr, 0, nullptr, nullptr, 0, nullptr, out, seen, stream);
}

int gs2m_texbake_accumulate(long long n_texels, const double* points, const double* normals, const int* owner, int n_views,
                            const double* w2c, double fx, double fy, double cx, double cy, int W, int H, const float* depth, int C,
                            const float* maps, const float* mask, double eps, int accumulate, double* sums, double* weights,
                            void* stream) {
    return bake_accumulate(true, n_texels, points, normals, owner, n_views, w2c, fx, fy, cx, cy, W, H, depth, C, maps, mask, eps, accumulate, sums,
                        weights, stream);
}

int gs2m_texbake_resolve(long long n_texels, int C, int width, int row0, const double* sums, const double* weights, double min_weight,
                         const float* fallback, const int* owner, long long n_triangles, const int* triangles, const int* cells,
                         long long n_verts, const float* attributes, float* out, unsigned char* seen, void* stream) {
    return bake_resolve(true, n_texels, C, width, row0, sums, weights, min_weight, fallback, owner, n_triangles, triangles, cells, n_verts,
                   attributes, out, seen, stream);
}

int gs2m_texture_pack(long long n_texels, int C, const float* values, int srgb, unsigned char* base_color, unsigned char* orm,
                      void* stream) {
    if (n_texels < 0 || (C != 3 && C != 5) || (C == 3 && orm) || (C == 5 && n_texels > 0 && !orm)) return GS2M_ERR_INVALID_ARG;
    if (n_texels > 0 && (!values || !base_color)) return GS2M_ERR_INVALID_ARG;
    if (n_texels == 0) return GS2M_OK;
    if (n_texels > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    texture_pack_kernel<<<blocks_of(n_texels), 256, 0, (hipStream_t)stream>>>(n_texels, C, values, srgb ? 1 : 0, base_color, orm);
    return gs2m_status(hipGetLastError());
}

int gs2m_texture_normals(long long n_texels, const int* owner, const double* tnormals, long long n_triangles, const int* triangles,
                         const float* uvs, long long n_verts, const double* vertices, int C, int offset, const float* values,
                         unsigned char* normal_map, double* tangent, void* stream) {
    if (n_texels < 0 || n_triangles < 0 || n_verts < 0 || C < 3 || C > BAKE_CMAX || offset < 0 || offset > C - 3) return GS2M_ERR_INVALID_ARG;
    if (n_texels > 0 && (!owner || !tnormals || !values || !normal_map)) return GS2M_ERR_INVALID_ARG;
    if (n_triangles > 0 && (!triangles || !uvs || (n_verts > 0 && !vertices))) return GS2M_ERR_INVALID_ARG;
    if (n_texels == 0) return GS2M_OK;
    if (n_texels > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    texture_normals_kernel<<<blocks_of(n_texels), 256, 0, (hipStream_t)stream>>>(n_texels, owner, tnormals, n_triangles, triangles, uvs, n_verts,
                                                                                 vertices, C, offset, values, normal_map, tangent);
    return gs2m_status(hipGetLastError());
}

}  // extern "C"
