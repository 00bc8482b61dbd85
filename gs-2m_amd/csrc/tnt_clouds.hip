// Tanks and Temples evaluation, the error-coloured clouds: k-nearest-neighbour normals and distance colours
// (include/gs2m_tnt.h; the contract: DESIGN.md §11).
//
//   box_kernel          the cloud's box in grid cells (integer minimum / maximum: any order gives the same box)
//   knn_normals_kernel  one thread per point: the k nearest neighbours over the hashed grid of mesh_eval.hip, kept as a sorted
//                       list of (d2, index) pairs in registers, then the normal of their covariance (tnt_normal.h)
//   colors_kernel       hot_r of the capped distance
//
// The search walks the cells around the query's own in shells of growing Chebyshev radius r, each shell clipped to the box.
// A bucket of the hashed grid holds every point whose cell hashes to it, so a candidate counts only when its own cell is the
// cell being visited: every point is then met exactly once, in the one shell that holds its cell.  After shell r every
// unvisited point is at least r cells away on some axis, so the walk stops once the list is full and its largest d2 is at
// most (r cell - eps)^2 (eps: the rounding of x / cell, as in mesh_eval.hip's nearest), or when r reaches R, the largest
// distance in cells from the query's cell to a face of the box -- both integers known before the loop.
// Compiled with -ffp-contract=off: d2 is evaluated as written, so the tie rule does not depend on the compiler.
#include <limits.h>
#include <math.h>
#include "eval_common.h"
#include "tnt_hot_r.h"
#include "tnt_normal.h"
#include "../../include/gs2m_tnt.h"

namespace {

constexpr int KNN_MAX = 32;
constexpr int BOX_CELLS_MAX = 65535;  // per axis

struct Box {
    int lo[3], hi[3];
};

__global__ void box_init_kernel(int* __restrict__ box) {
    if (threadIdx.x < 6) box[threadIdx.x] = threadIdx.x < 3 ? INT_MAX : INT_MIN;
}

__global__ void __launch_bounds__(256) box_kernel(long long n, const double* __restrict__ pts, double inv, int* __restrict__ box) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
    if (i < n) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double x = pts[3 * i + a];
            lo[a] = hi[a] = cell_coord(x, inv);
            if (!(fabs(x) < __builtin_huge_val())) lo[a] = INT_MIN, hi[a] = INT_MAX;  // NaN or infinite: the host refuses the cloud
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            lo[a] = min(lo[a], __shfl_xor(lo[a], o, 64));
            hi[a] = max(hi[a], __shfl_xor(hi[a], o, 64));
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            atomicMin(box + a, lo[a]);
            atomicMax(box + 3 + a, hi[a]);
        }
    }
}

// (d, i) before (e, j) in the neighbour order
__device__ __forceinline__ bool before(double d, uint32_t i, double e, uint32_t j) { return d < e || (d == e && i < j); }

// KCAP: the list's length, k <= KCAP.  The list is indexed by unrolled loops alone, so it stays in registers: 2 KCAP VGPRs of
// d2 and KCAP of indices.
template <int KCAP>
__global__ void __launch_bounds__(256) knn_normals_kernel(long long n, const double* __restrict__ pts, double cell, double inv, uint32_t mask,
                                                          const double* __restrict__ spts, const uint32_t* __restrict__ sidx,
                                                          const uint32_t* __restrict__ start, int k, Box box,
                                                          double* __restrict__ normals, long long* __restrict__ knn_index) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double INF = __builtin_huge_val();
    const double q[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    int c[3], R = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        c[a] = cell_coord(q[a], inv);
        R = max(R, max(c[a] - box.lo[a], box.hi[a] - c[a]));  // c lies in the box: the box was taken from these cells
    }
    const int m = (int)(n < (long long)k ? n : (long long)k);  // the neighbours there are
    const double eps = 1e-6 * cell + 1e-13 * fmax(fabs(q[0]), fmax(fabs(q[1]), fabs(q[2])));
    double d2[KCAP];
    uint32_t id[KCAP];
#pragma unroll
    for (int j = 0; j < KCAP; j++) d2[j] = INF, id[j] = 0xFFFFFFFFu;
    double worst = INF;  // entry m - 1 of the list: what a candidate has to come before
    uint32_t worst_i = 0xFFFFFFFFu;

    auto visit = [&](int X, int Y, int Z) {
        const uint32_t b = hash3(X, Y, Z, mask);
        const uint32_t e = start[b + 1];
        for (uint32_t s = start[b]; s < e; s++) {  // at most the bucket's length <= n
            const double* p = spts + 3 * (size_t)s;
            const double px = p[0], py = p[1], pz = p[2];
            if (cell_coord(px, inv) != X || cell_coord(py, inv) != Y || cell_coord(pz, inv) != Z) continue;  // a hash collision
            const double dx = q[0] - px, dy = q[1] - py, dz = q[2] - pz;
            const double d = (dx * dx + dy * dy) + dz * dz;
            const uint32_t o = sidx[s];
            if (!before(d, o, worst, worst_i)) continue;
#pragma unroll
            for (int j = KCAP - 1; j > 0; j--) {  // from the end: entry j - 1 is still the old one
                if (before(d, o, d2[j - 1], id[j - 1])) d2[j] = d2[j - 1], id[j] = id[j - 1];
                else if (before(d, o, d2[j], id[j])) d2[j] = d, id[j] = o;
            }
            if (before(d, o, d2[0], id[0])) d2[0] = d, id[0] = o;
#pragma unroll
            for (int j = 0; j < KCAP; j++)
                if (j == m - 1) worst = d2[j], worst_i = id[j];
        }
    };

    // r = 0 .. R: at most R + 1 <= BOX_CELLS_MAX + 1 shells, whatever the data; a shell's loops run over its cells inside
    // the box, so all shells together visit at most the box's cells once.
    for (int r = 0; r <= R; r++) {
        const int z0 = max(-r, box.lo[2] - c[2]), z1 = min(r, box.hi[2] - c[2]);
        const int y0 = max(-r, box.lo[1] - c[1]), y1 = min(r, box.hi[1] - c[1]);
        const int x0 = max(-r, box.lo[0] - c[0]), x1 = min(r, box.hi[0] - c[0]);
        for (int dz = z0; dz <= z1; dz++)
            for (int dy = y0; dy <= y1; dy++) {
                if (dz == -r || dz == r || dy == -r || dy == r) {
                    for (int dx = x0; dx <= x1; dx++) visit(c[0] + dx, c[1] + dy, c[2] + dz);
                } else {  // the two cells of the row that lie on the shell (r >= 1 here)
                    if (x0 == -r) visit(c[0] - r, c[1] + dy, c[2] + dz);
                    if (x1 == r) visit(c[0] + r, c[1] + dy, c[2] + dz);
                }
            }
        const double lb = (double)r * cell - eps;  // what shell r + 1 and beyond can hold is farther than this
        if (lb > 0.0 && worst <= lb * lb) break;   // worst is finite only once the list holds m entries
    }

    // Every point's cell lies in the box, so the list holds m entries here.  A grid built over another cloud or with another
    // edge breaks that: its missing entries read no memory (index -1, the fallback normal).
    bool whole = true;
#pragma unroll
    for (int j = 0; j < KCAP; j++)
        if (j < m && (long long)id[j] >= n) whole = false;
    if (knn_index) {
        long long* out = knn_index + (size_t)i * k;
#pragma unroll
        for (int j = 0; j < KCAP; j++)
            if (j < k) out[j] = j < m && (long long)id[j] < n ? (long long)id[j] : -1ll;
    }

    double nrm[3] = {0.0, 0.0, 1.0};
    if (m >= 3 && whole) {
        double mean[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < KCAP; j++)
            if (j < m) {
                const double* p = pts + 3 * (size_t)id[j];
                mean[0] += p[0], mean[1] += p[1], mean[2] += p[2];
            }
        mean[0] /= (double)m, mean[1] /= (double)m, mean[2] /= (double)m;
        double cxx = 0.0, cxy = 0.0, cxz = 0.0, cyy = 0.0, cyz = 0.0, czz = 0.0;
#pragma unroll
        for (int j = 0; j < KCAP; j++)
            if (j < m) {
                const double* p = pts + 3 * (size_t)id[j];
                const double ax = p[0] - mean[0], ay = p[1] - mean[1], az = p[2] - mean[2];
                cxx += ax * ax, cxy += ax * ay, cxz += ax * az, cyy += ay * ay, cyz += ay * az, czz += az * az;
            }
        gs2m_normal_of_covariance(cxx, cxy, cxz, cyy, cyz, czz, nrm);
    }
    normals[3 * i] = nrm[0];
    normals[3 * i + 1] = nrm[1];
    normals[3 * i + 2] = nrm[2];
}

__device__ const double hot_r_table[256][3] = GS2M_HOT_R_TABLE;

__global__ void __launch_bounds__(256) colors_kernel(long long n, const double* __restrict__ dist, double cap, unsigned char* __restrict__ rgb,
                                                     int* __restrict__ err) {
    __shared__ unsigned char s_rgb[768];
    for (int t = threadIdx.x; t < 768; t += 256) s_rgb[t] = (unsigned char)rint(hot_r_table[t / 3][t % 3] * 255.0);
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double d = dist[i];
    if (d != d) {
        err[0] = 1;
        return;
    }
    const int row = gs2m_color_row(d, cap);
#pragma unroll
    for (int ch = 0; ch < 3; ch++) rgb[3 * i + ch] = s_rgb[3 * row + ch];
}

struct KnnWs {
    int* box;  // 6: lo, hi
    size_t bytes;
};
KnnWs carve_knn(char* base) {
    Carver c{base, 0};
    KnnWs w;
    w.box = c.take<int>(6);
    w.bytes = c.off;
    return w;
}

}  // namespace

extern "C" {

int gs2m_tnt_knn_normals_workspace_bytes(long long n, long long* bytes) {
    if (n < 0 || !bytes) return GS2M_ERR_INVALID_ARG;
    if (n > MAX_POINTS) return GS2M_ERR_UNSUPPORTED;
    *bytes = (long long)carve_knn(nullptr).bytes;
    return GS2M_OK;
}

int gs2m_tnt_knn_normals(long long n, const double* pts, double cell, const void* grid, int k, void* ws, double* normals,
                         long long* knn_index, void* stream) {
    if (n < 0 || k < 1 || k > KNN_MAX || !(cell > 0.0) || !(cell < __builtin_huge_val()) || !grid || !ws ||
        (n > 0 && (!pts || !normals)))
        return GS2M_ERR_INVALID_ARG;
    if (n > MAX_POINTS) return GS2M_ERR_UNSUPPORTED;
    if (n == 0) return GS2M_OK;
    hipStream_t s = (hipStream_t)stream;
    const KnnWs w = carve_knn((char*)ws);
    const double inv = 1.0 / cell;  // gs2m_eval_grid_build's own factor: the cells here are the grid's
    box_init_kernel<<<1, 64, 0, s>>>(w.box);
    box_kernel<<<blocks_of(n), 256, 0, s>>>(n, pts, inv, w.box);
    Box box;
    if (gs2m_read_back(s, {{&box, w.box, sizeof(box)}}) != GS2M_OK) return GS2M_ERR_HIP;
    for (int a = 0; a < 3; a++) {
        if (box.lo[a] == INT_MIN) return GS2M_ERR_INVALID_ARG;  // a coordinate that is not finite
        if ((long long)box.hi[a] - box.lo[a] > BOX_CELLS_MAX) return GS2M_ERR_UNSUPPORTED;
    }
    const Grid g = carve_grid((char*)const_cast<void*>(grid), n);
    const uint32_t mask = (uint32_t)((1ll << g.bits) - 1);
    if (k <= 20)
        knn_normals_kernel<20><<<blocks_of(n), 256, 0, s>>>(n, pts, cell, inv, mask, g.spts, g.sidx, g.start, k, box, normals, knn_index);
    else
        knn_normals_kernel<KNN_MAX><<<blocks_of(n), 256, 0, s>>>(n, pts, cell, inv, mask, g.spts, g.sidx, g.start, k, box, normals, knn_index);
    return gs2m_status(hipGetLastError());
}

int gs2m_tnt_distance_colors(long long n, const double* dist, double max_distance, void* ws, unsigned char* rgb, void* stream) {
    if (n < 0 || !(max_distance > 0.0) || !(max_distance < __builtin_huge_val()) || !ws || (n > 0 && (!dist || !rgb)))
        return GS2M_ERR_INVALID_ARG;
    if (n > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    if (n == 0) return GS2M_OK;
    hipStream_t s = (hipStream_t)stream;
    int* err = (int*)ws;
    if (hipMemsetAsync(err, 0, 8, s) != hipSuccess) return GS2M_ERR_HIP;
    colors_kernel<<<blocks_of(n), 256, 0, s>>>(n, dist, max_distance, rgb, err);
    int e = 0;
    if (gs2m_read_back(s, {{&e, err, sizeof(e)}}) != GS2M_OK) return GS2M_ERR_HIP;
    return e ? GS2M_ERR_INVALID_ARG : GS2M_OK;
}

}  // extern "C"
