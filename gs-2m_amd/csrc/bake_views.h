// The per-point view loop of the attribute bakes (the Weight, Project, Mask, Sample and Accumulate paragraphs of
// include/gs2m_meshbake.h), the body of mesh_bake.hip's accumulate kernel: a point is a vertex there, or a texel's point on its
// triangle.  fp64, as written: compile the including unit with -ffp-contract=off.
//
// The views' matrices and camera centres are staged in LDS, BAKE_CHUNK at a time, by the whole workgroup (every lane then reads
// the same words: a broadcast), so no lane re-reads a matrix from memory: EVERY thread of the 256-thread workgroup calls
// bake_views, a thread without a point with lit == false.  Projection, inside test, taps and the depth sample are
// vertex_project.h's.  A view costs a point the four depth taps, and only where it passes them the mask's and the C x 4 attribute
// taps.  Every tap lies within [0, W - 1] x [0, H - 1]: x0, y0 come from a passed inside test and the neighbours are read only
// where they exist.  The sums are the caller's registers, and the order of the additions is the order of the views.
// The views travel in one by-value struct, so its pointers are plain ones: the __restrict__ the vertex bake's kernel parameters had
// is gone.  Every load through them is of read-only data that no store of the kernels can alias in a correct call, and the vertex
// bake measured the same after the move.
#pragma once
#include "mesh_raster.h"
#include "vertex_project.h"

namespace mesh_raster {

constexpr int BAKE_CHUNK = 64;   // views staged in LDS at a time
constexpr int BAKE_ROW = 16;     // doubles per staged view: the matrix's three rows, the camera centre, one pad

struct BakeViews {
    int n_views;
    const double* w2c;
    Frame q;
    const float *depth, *maps, *mask;  // mask: null = every tap is foreground
    double eps;
};

// a usable normal: finite and not zero
__device__ __forceinline__ bool normal_ok(const double* N) {
    return isfinite(N[0]) && isfinite(N[1]) && isfinite(N[2]) && !(N[0] == 0.0 && N[1] == 0.0 && N[2] == 0.0);
}

// lit: false = every view weighs 0 (no point, or a normal that is zero or not finite); with_normals: weigh by the cosine between
// N and the direction to the camera, nn = dot(N, N).  s_m: the workgroup's staging block.
template <int C>
__device__ __forceinline__ void bake_views(const BakeViews& b, bool lit, const double* p, bool with_normals, const double* N, double nn,
                                           double (*s_m)[BAKE_ROW], double* acc, double& wsum) {
    const Frame& q = b.q;
    const size_t frame = (size_t)q.W * q.H;
    for (int v0 = 0; v0 < b.n_views; v0 += BAKE_CHUNK) {
        const int nv = min(BAKE_CHUNK, b.n_views - v0);
        __syncthreads();
        for (int k = threadIdx.x; k < nv * BAKE_ROW; k += 256) {
            const int v = k / BAKE_ROW, e = k % BAKE_ROW;
            const double* M = b.w2c + 16 * (size_t)(v0 + v);
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
            if (with_normals) {
                const double e[3] = {M[12] - p[0], M[13] - p[1], M[14] - p[2]};
                w = fmax(0.0, dot3(N, e) / sqrt(nn * dot3(e, e)));
            }
            if (!(w > 0.0)) continue;  // NaN fails
            VertexTaps t;
            if (!project_vertex(M, p, q, t)) continue;
            const size_t view = (size_t)(v0 + v);
            if (!in_front(t.z, bilinear_taps(b.depth + view * frame, q.W, t), b.eps)) continue;
            if (b.mask) {
                const float* K = b.mask + view * frame + (size_t)t.y0 * q.W + t.x0;
                const double ax = 1.0 - t.tx, ay = 1.0 - t.ty;
                bool ok = true;
                if (ax * ay != 0.0) ok = ok && K[0] >= 0.5f;
                if (t.right && t.tx * ay != 0.0) ok = ok && K[1] >= 0.5f;
                if (t.below && ax * t.ty != 0.0) ok = ok && K[q.W] >= 0.5f;
                if (t.right && t.below && t.tx * t.ty != 0.0) ok = ok && K[q.W + 1] >= 0.5f;
                if (!ok) continue;
            }
            const float* A = b.maps + view * C * frame;
#pragma unroll
            for (int c = 0; c < C; c++) acc[c] = acc[c] + w * bilinear_taps(A + c * frame, q.W, t);
            wsum = wsum + w;
        }
    }
}

}  // namespace mesh_raster
