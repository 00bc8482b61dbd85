// The per-vertex projection and the bilinear taps of the Votes paragraph of include/gs2m_visibility.h, shared by the units that
// look a vertex up in a view's images: mesh_depth.hip (the votes) and mesh_bake.hip (the attribute bake).  fp64, as written:
// compile the including unit with -ffp-contract=off.
#pragma once
#include "mesh_raster.h"

namespace mesh_raster {

struct VertexTaps {
    double z;            // z0 + 1e-8
    double tx, ty;       // u - x0, v - y0
    int x0, y0;          // floor(u), floor(v): within the frame
    bool right, below;   // x0 + 1 < W, y0 + 1 < H: the neighbours that exist
};

// false: the vertex is not inside the view's frame (or not in front of the camera, or a coordinate is NaN); `t` is then not set.
// M: the view's matrix, 12 doubles at least, in global memory or LDS.
__device__ __forceinline__ bool project_vertex(const double* M, const double* p, const Frame& q, VertexTaps& t) {
    double c[3];
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] = ((M[4 * k] * p[0] + M[4 * k + 1] * p[1]) + M[4 * k + 2] * p[2]) + M[4 * k + 3];
    const double w1 = (double)(q.W - 1), h1 = (double)(q.H - 1);
    const double z = c[2] + 1e-8;
    const double x = (q.fx * c[0] + q.cx * c[2]) / z, y = (q.fy * c[1] + q.cy * c[2]) / z;
    if (!(x >= 0.0 && x <= w1 && y >= 0.0 && y <= h1 && z > 0.0)) return false;  // NaN fails
    t.z = z;
    t.x0 = (int)floor(x), t.y0 = (int)floor(y);
    t.tx = x - (double)t.x0, t.ty = y - (double)t.y0;
    t.right = t.x0 + 1 < q.W, t.below = t.y0 + 1 < q.H;
    return true;
}

// The bilinear sample of one (H, W) image at the taps; a neighbour outside the frame is not read and enters as 0.
__device__ __forceinline__ double bilinear_taps(const float* __restrict__ img, int W, const VertexTaps& t) {
    const float* D = img + (size_t)t.y0 * W + t.x0;
    const double d00 = (double)D[0], d01 = t.right ? (double)D[1] : 0.0;
    const double d10 = t.below ? (double)D[W] : 0.0, d11 = t.right && t.below ? (double)D[W + 1] : 0.0;
    return ((d00 * ((1.0 - t.tx) * (1.0 - t.ty)) + d01 * (t.tx * (1.0 - t.ty))) + d10 * ((1.0 - t.tx) * t.ty)) + d11 * (t.tx * t.ty);
}

// front: the vertex is not behind the rendered surface
__device__ __forceinline__ bool in_front(double z, double d, double eps) { return d > 0.0 ? z < d + eps : true; }

}  // namespace mesh_raster
