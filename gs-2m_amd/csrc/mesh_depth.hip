// Mesh visibility cull: a z-buffer depth rasterizer for triangle meshes, the per-vertex view votes and the keep flags
// (include/gs2m_visibility.h; the contract: DESIGN.md §14).
//
// Rasterizer: the shared core of mesh_raster.h (its head describes the lane, wave and workgroup paths) with the sink that keeps the
// unsigned minimum of the fp32 z's bit pattern.  The image starts as 0xFFFFFFFF and a last pass turns what is left of that into 0.
// Votes: a thread per vertex, the views in a loop, fp64 as written.
#include <math.h>
#include "eval_common.h"
#include "mesh_raster.h"
#include "vertex_project.h"
#include "../../include/gs2m_visibility.h"

using namespace mesh_raster;

namespace {

constexpr unsigned EMPTY = 0xFFFFFFFFu;

__global__ void __launch_bounds__(256) resolve_empty_kernel(long long n, unsigned* __restrict__ img) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && img[i] == EMPTY) img[i] = 0u;
}

// ---- votes ----

__global__ void __launch_bounds__(256) votes_kernel(long long n, const double* __restrict__ verts, int n_views,
                                                    const double* __restrict__ w2c, Frame q, const float* __restrict__ depth,
                                                    double eps, int accumulate, int* __restrict__ votes) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double p[3] = {verts[3 * i], verts[3 * i + 1], verts[3 * i + 2]};
    int count = 0;
    for (int v = 0; v < n_views; v++) {
        VertexTaps t;
        if (!project_vertex(w2c + 16 * (size_t)v, p, q, t)) continue;
        const double d = bilinear_taps(depth + (size_t)v * q.W * q.H, q.W, t);
        count += in_front(t.z, d, eps) ? 1 : 0;
    }
    votes[i] = (accumulate ? votes[i] : 0) + count;
}

__global__ void __launch_bounds__(256) keep_kernel(long long n, const int* __restrict__ votes, int min_views,
                                                   unsigned char* __restrict__ keep) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) keep[i] = votes[i] >= min_views ? 1 : 0;
}

// the same byte from every writer: the stores need no order
__global__ void __launch_bounds__(256) referenced_kernel(long long nv, const unsigned char* __restrict__ keep, long long nt,
                                                         const int* __restrict__ tris, unsigned char* __restrict__ flags) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const int a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
    if (a < 0 || b < 0 || c < 0 || a >= nv || b >= nv || c >= nv) return;
    if (keep[a] & keep[b] & keep[c] & 1) flags[a] = flags[b] = flags[c] = 1;
}

}  // namespace

extern "C" {

int gs2m_meshdepth_workspace_bytes(long long n_tris, int n_views, long long* bytes) {
    if (n_tris < 0 || n_views < 0 || !bytes) return GS2M_ERR_INVALID_ARG;
    if (n_tris > 0x7FFFFFFFll || n_views > 65535) return GS2M_ERR_UNSUPPORTED;
    *bytes = (long long)carve_raster(nullptr, n_tris, n_views).bytes;
    return GS2M_OK;
}

int gs2m_meshdepth_render(long long n_verts, const double* verts, long long n_tris, const int* tris, int n_views,
                          const double* w2c, double fx, double fy, double cx, double cy, int W, int H, double near_z, double far_z,
                          void* ws, float* depth, void* stream) {
    if (n_verts < 0 || n_tris < 0 || !frame_ok(n_views, W, H, fx, fy, cx, cy) || !ws) return GS2M_ERR_INVALID_ARG;
    if (!(near_z > 0.0 && near_z <= far_z && isfinite(far_z))) return GS2M_ERR_INVALID_ARG;
    if (n_views > 0 && (!w2c || !depth)) return GS2M_ERR_INVALID_ARG;
    if (n_tris > 0 && (!tris || (n_verts > 0 && !verts))) return GS2M_ERR_INVALID_ARG;
    if (n_tris > 0x7FFFFFFFll || n_verts > 0x7FFFFFFFll) return GS2M_ERR_UNSUPPORTED;  // ids are int, list entries 32-bit
    hipStream_t s = (hipStream_t)stream;
    const RasterWs w = carve_raster((char*)ws, n_tris, n_views);
    const long long pixels = (long long)n_views * W * H;
    if (n_views > 0 && hipMemsetAsync(depth, 0xFF, sizeof(float) * (size_t)pixels, s) != hipSuccess) return GS2M_ERR_HIP;
    const Frame q{fx, fy, cx, cy, near_z, far_z, W, H};
    unsigned* img = (unsigned*)depth;
    if (raster_launch(n_verts, verts, n_tris, tris, n_views, w2c, q, w, DepthSink{img}, s) != GS2M_OK) return GS2M_ERR_HIP;
    if (n_views > 0) resolve_empty_kernel<<<blocks_of(pixels), 256, 0, s>>>(pixels, img);
    int err;
    if (gs2m_read_back(s, {{&err, w.err, sizeof(err)}}) != GS2M_OK) return GS2M_ERR_HIP;
    return err ? GS2M_ERR_INVALID_ARG : GS2M_OK;
}

int gs2m_visibility_votes(long long n_verts, const double* verts, int n_views, const double* w2c, double fx, double fy,
                          double cx, double cy, int W, int H, const float* depth, double eps, int accumulate, int* votes,
                          void* stream) {
    if (n_verts < 0 || !frame_ok(n_views, W, H, fx, fy, cx, cy) || eps != eps) return GS2M_ERR_INVALID_ARG;
    if (n_verts > 0 && (!verts || !votes)) return GS2M_ERR_INVALID_ARG;
    if (n_views > 0 && (!w2c || !depth)) return GS2M_ERR_INVALID_ARG;
    if (n_verts == 0) return GS2M_OK;
    if (n_verts > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    const Frame q{fx, fy, cx, cy, 0.0, 0.0, W, H};
    votes_kernel<<<blocks_of(n_verts), 256, 0, (hipStream_t)stream>>>(n_verts, verts, n_views, w2c, q, depth, eps, accumulate, votes);
    return gs2m_status(hipGetLastError());
}

int gs2m_visibility_keep(long long n_verts, const int* votes, int min_views, unsigned char* keep, void* stream) {
    if (n_verts < 0 || (n_verts > 0 && (!votes || !keep))) return GS2M_ERR_INVALID_ARG;
    if (n_verts == 0) return GS2M_OK;
    if (n_verts > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    keep_kernel<<<blocks_of(n_verts), 256, 0, (hipStream_t)stream>>>(n_verts, votes, min_views, keep);
    return gs2m_status(hipGetLastError());
}

int gs2m_visibility_referenced(long long n_verts, const unsigned char* keep, long long n_tris, const int* tris,
                               unsigned char* flags, void* stream) {
    if (n_verts < 0 || n_tris < 0 || (n_verts > 0 && (!keep || !flags)) || (n_tris > 0 && !tris)) return GS2M_ERR_INVALID_ARG;
    if (n_tris > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    if (n_verts == 0) return GS2M_OK;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(flags, 0, (size_t)n_verts, s) != hipSuccess) return GS2M_ERR_HIP;
    if (n_tris > 0) referenced_kernel<<<blocks_of(n_tris), 256, 0, s>>>(n_verts, keep, n_tris, tris, flags);
    return gs2m_status(hipGetLastError());
}

}  // extern "C"
