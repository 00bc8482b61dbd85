// Per-vertex attribute bake: the views' attribute maps averaged onto the mesh's vertices (include/gs2m_meshbake.h; the
// contract: DESIGN.md §20).
//
// Accumulate: a thread per vertex keeps its position, its normal and its C + 1 running sums in registers and walks the views of
// the call in order; a wave's lanes are 64 neighbouring vertices.  The views' matrices and camera centres are staged in LDS,
// BAKE_CHUNK at a time, by the whole workgroup (every lane then reads the same words: a broadcast), so no lane re-reads a matrix
// from memory.  Projection, inside test, taps and the depth sample are vertex_project.h's, the ones the votes use.  A view costs a
// vertex the four depth taps, and only where it passes them the mask's and the C x 4 attribute taps.  The kernel is instantiated
// per C so that the sums are registers.  Every tap lies within [0, W - 1] x [0, H - 1]: x0, y0 come from a passed inside test and
// the neighbours are read only where they exist.  One thread owns a vertex: no atomics, and the order of the additions is the
// order of the views.
// Resolve: a thread per vertex.
#include <math.h>
#include "eval_common.h"
#include "mesh_raster.h"
#include "vertex_project.h"
#include "../../include/gs2m_meshbake.h"

using namespace mesh_raster;

namespace {

constexpr int BAKE_CHUNK = 64;   // views staged in LDS at a time
constexpr int BAKE_ROW = 16;     // doubles per staged view: the matrix's three rows, the camera centre, one pad
constexpr int BAKE_CMAX = 8;

template <int C>
__global__ void __launch_bounds__(256) bake_kernel(long long n, const double* __restrict__ verts, const double* __restrict__ normals,
                                                   int n_views, const double* __restrict__ w2c, Frame q, const float* __restrict__ depth,
                                                   const float* __restrict__ maps, const float* __restrict__ mask, double eps,
                                                   int accumulate, double* __restrict__ sums, double* __restrict__ weights) {
    __shared__ double s_m[BAKE_CHUNK][BAKE_ROW];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n;
    double p[3] = {0.0, 0.0, 0.0}, N[3] = {0.0, 0.0, 0.0}, nn = 0.0;
    bool lit = live;  // false: every view weighs 0
    if (live) {
#pragma unroll
        for (int k = 0; k < 3; k++) p[k] = verts[3 * i + k];
        if (normals) {
#pragma unroll
            for (int k = 0; k < 3; k++) N[k] = normals[3 * i + k];
            nn = dot3(N, N);
            lit = isfinite(N[0]) && isfinite(N[1]) && isfinite(N[2]) && !(N[0] == 0.0 && N[1] == 0.0 && N[2] == 0.0);
        }
    }
    double acc[C], wsum = 0.0;
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = 0.0;
    if (live && accumulate) {
#pragma unroll
        for (int c = 0; c < C; c++) acc[c] = sums[(size_t)i * C + c];
        wsum = weights[i];
    }
    const size_t frame = (size_t)q.W * q.H;
    for (int v0 = 0; v0 < n_views; v0 += BAKE_CHUNK) {
        const int nv = min(BAKE_CHUNK, n_views - v0);
        __syncthreads();
        for (int k = threadIdx.x; k < nv * BAKE_ROW; k += 256) {
            const int v = k / BAKE_ROW, e = k % BAKE_ROW;
            const double* M = w2c + 16 * (size_t)(v0 + v);
            double x = 0.0;
            if (e < 12) x = M[e];
            else if (e < 15) x = -((M[e - 12] * M[3] + M[4 + e - 12] * M[7]) + M[8 + e - 12] * M[11]);
            s_m[v][e] = x;
        }
        __syncthreads();
        if (!lit) continue;
        for (int v = 0; v < nv; v++) {
            const double* M = s_m[v];
            double w = 1.0;
            if (normals) {
                const double e[3] = {M[12] - p[0], M[13] - p[1], M[14] - p[2]};
                w = fmax(0.0, dot3(N, e) / sqrt(nn * dot3(e, e)));
            }
            if (!(w > 0.0)) continue;  // NaN fails
            VertexTaps t;
            if (!project_vertex(M, p, q, t)) continue;
            const size_t view = (size_t)(v0 + v);
            if (!in_front(t.z, bilinear_taps(depth + view * frame, q.W, t), eps)) continue;
            if (mask) {
                const float* K = mask + view * frame + (size_t)t.y0 * q.W + t.x0;
                const double ax = 1.0 - t.tx, ay = 1.0 - t.ty;
                bool ok = true;
                if (ax * ay != 0.0) ok = ok && K[0] >= 0.5f;
                if (t.right && t.tx * ay != 0.0) ok = ok && K[1] >= 0.5f;
                if (t.below && ax * t.ty != 0.0) ok = ok && K[q.W] >= 0.5f;
                if (t.right && t.below && t.tx * t.ty != 0.0) ok = ok && K[q.W + 1] >= 0.5f;
                if (!ok) continue;
            }
            const float* A = maps + view * C * frame;
#pragma unroll
            for (int c = 0; c < C; c++) acc[c] = acc[c] + w * bilinear_taps(A + c * frame, q.W, t);
            wsum = wsum + w;
        }
    }
    if (live) {
#pragma unroll
        for (int c = 0; c < C; c++) sums[(size_t)i * C + c] = acc[c];
        weights[i] = wsum;
    }
}

struct Fallback {
    float v[BAKE_CMAX];
};

__global__ void __launch_bounds__(256) bake_resolve_kernel(long long n, int C, const double* __restrict__ sums,
                                                           const double* __restrict__ weights, double min_weight, Fallback fb,
                                                           float* __restrict__ out, unsigned char* __restrict__ seen) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double w = weights[i];
    const bool ok = w >= min_weight && w > 0.0;
    for (int c = 0; c < C; c++) out[(size_t)i * C + c] = ok ? (float)(sums[(size_t)i * C + c] / w) : fb.v[c];
    seen[i] = ok ? 1 : 0;
}

template <int C>
void bake_launch(long long n, const double* verts, const double* normals, int n_views, const double* w2c, const Frame& q,
                 const float* depth, const float* maps, const float* mask, double eps, int accumulate, double* sums, double* weights,
                 hipStream_t s) {
    bake_kernel<C><<<blocks_of(n), 256, 0, s>>>(n, verts, normals, n_views, w2c, q, depth, maps, mask, eps, accumulate, sums, weights);
}

}  // namespace

extern "C" {

int gs2m_meshbake_accumulate(long long n_verts, const double* verts, const double* normals, int n_views, const double* w2c,
                             double fx, double fy, double cx, double cy, int W, int H, const float* depth, int C, const float* maps,
                             const float* mask, double eps, int accumulate, double* sums, double* weights, void* stream) {
    if (n_verts < 0 || C < 1 || C > BAKE_CMAX || !frame_ok(n_views, W, H, fx, fy, cx, cy) || eps != eps) return GS2M_ERR_INVALID_ARG;
    if (n_verts > 0 && (!verts || !sums || !weights)) return GS2M_ERR_INVALID_ARG;
    if (n_views > 0 && (!w2c || !depth || !maps)) return GS2M_ERR_INVALID_ARG;
    if (n_verts == 0) return GS2M_OK;
    if (n_verts > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    if ((long long)n_views * C * W * H > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    const Frame q{fx, fy, cx, cy, 0.0, 0.0, W, H};
    hipStream_t s = (hipStream_t)stream;
#define BAKE_CASE(c) \
    case c: bake_launch<c>(n_verts, verts, normals, n_views, w2c, q, depth, maps, mask, eps, accumulate, sums, weights, s); break;
    switch (C) {
        BAKE_CASE(1) BAKE_CASE(2) BAKE_CASE(3) BAKE_CASE(4) BAKE_CASE(5) BAKE_CASE(6) BAKE_CASE(7) BAKE_CASE(8)
    }
#undef BAKE_CASE
    return gs2m_status(hipGetLastError());
}

int gs2m_meshbake_resolve(long long n_verts, int C, const double* sums, const double* weights, double min_weight,
                          const float* fallback, float* out, unsigned char* seen, void* stream) {
    if (n_verts < 0 || C < 1 || C > BAKE_CMAX || min_weight != min_weight || !fallback) return GS2M_ERR_INVALID_ARG;
    if (n_verts > 0 && (!sums || !weights || !out || !seen)) return GS2M_ERR_INVALID_ARG;
    if (n_verts == 0) return GS2M_OK;
    if (n_verts > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    Fallback fb{};
    for (int c = 0; c < C; c++) fb.v[c] = fallback[c];
    bake_resolve_kernel<<<blocks_of(n_verts), 256, 0, (hipStream_t)stream>>>(n_verts, C, sums, weights, min_weight, fb, out, seen);
    return gs2m_status(hipGetLastError());
}

}  // extern "C"
