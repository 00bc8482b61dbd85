// Triangle atlas: a right-isosceles chart per triangle, two charts to a power-of-two cell, cells in Z-order
// (include/gs2m_atlas.h has the contract, DESIGN.md §22 the plan; the integer side is atlas_layout.h).
//
// Class: a thread per triangle tests its indices and corners, takes the longest edge and writes the 3-bit sort key 5 - k; the
// class histogram is counted per workgroup in LDS and added with six integer atomics (their order cannot change a count).  One
// read-back brings the error flags and the histogram; the layout follows on the host.
// Place: the project's stable radix sort orders the triangles by key; a thread per sorted position derives rank, cell, half,
// the cell's origin (Morton decode) and the three UVs.  Nothing is scattered from triangles into texels:
// Texels: a thread per texel Morton-encodes its unit, finds class and cell from the six bases, and reads its owner from `order`.
// Every index is tested before it is used: a triangle's vertex ids in the class kernel (and again where the texel kernel
// receives them from its caller), sorted positions against F, texel coordinates against the rows of the call.
#include <math.h>
#include "eval_common.h"
#include "atlas_layout.h"
#include "../../include/gs2m_atlas.h"

namespace {

constexpr long long ATLAS_SORT_LIMIT = 0x3FFFFFFFll;
constexpr int KEY_BITS = 3;

__device__ __forceinline__ double rdot(const double* u, const double* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

// err[0]: a vertex index out of range; err[1]: a corner that is not finite
__global__ void __launch_bounds__(256) atlas_class_kernel(long long nv, const double* __restrict__ verts, long long nt,
                                                          const int* __restrict__ tris, double density, uint32_t* __restrict__ key,
                                                          u64* __restrict__ hist, int* __restrict__ err) {
    __shared__ unsigned s_hist[ATLAS_CLASSES];
    if (threadIdx.x < ATLAS_CLASSES) s_hist[threadIdx.x] = 0;
    __syncthreads();
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < nt) {
        const int ia = tris[3 * t], ib = tris[3 * t + 1], ic = tris[3 * t + 2];
        int k = 0;
        if (tri_in_range(ia, ib, ic, nv, err)) {
            double P[9];
            const int id[3] = {ia, ib, ic};
            bool finite = true;
#pragma unroll
            for (int c = 0; c < 3; c++)
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    P[3 * c + d] = verts[3 * (size_t)id[c] + d];
                    finite = finite && isfinite(P[3 * c + d]);
                }
            if (!finite) err[1] = 1;
            double e = 0.0;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const int n = (c + 1) % 3;
                const double d[3] = {P[3 * n] - P[3 * c], P[3 * n + 1] - P[3 * c + 1], P[3 * n + 2] - P[3 * c + 2]};
                e = fmax(e, sqrt(rdot(d, d)));
            }
            const double want = e * density;
            k = ATLAS_CLASSES - 1;
#pragma unroll
            for (int c = ATLAS_CLASSES - 2; c >= 0; c--)
                if ((double)((8 << c) - 4) >= want) k = c;  // NaN fails: the largest class (and the call is refused)
        }
        key[t] = (uint32_t)(ATLAS_CLASSES - 1 - k);
        atomicAdd(&s_hist[k], 1u);
    }
    __syncthreads();
    if (threadIdx.x < ATLAS_CLASSES && s_hist[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (u64)s_hist[threadIdx.x]);
}

__global__ void __launch_bounds__(256) atlas_place_kernel(long long nt, AtlasLayout L, const uint32_t* __restrict__ skey,
                                                          const uint32_t* __restrict__ sval, int* __restrict__ cells,
                                                          float* __restrict__ uvs, int* __restrict__ order) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= nt) return;
    const uint32_t t = sval[q], kk = skey[q];
    if (t >= (uint32_t)nt || kk >= (uint32_t)ATLAS_CLASSES) return;  // (the sort hands back what it was given)
    const int k = ATLAS_CLASSES - 1 - (int)kk;
    const long long rank = q - L.start[k];
    if (rank < 0 || rank >= L.hist[k]) return;
    const int half = (int)(rank & 1), side = 8 << k;
    int ox, oy;
    atlas_cell_origin(L, k, rank >> 1, &ox, &oy);
    order[q] = (int)t;
    int* c = cells + 4 * (size_t)t;
    c[0] = ox, c[1] = oy, c[2] = side, c[3] = half;
#pragma unroll
    for (int v = 0; v < 3; v++) {
        int x, y;
        atlas_corner(side, half, v, &x, &y);
        uvs[6 * (size_t)t + 2 * v] = (float)((double)(ox + x) / (double)L.width);
        uvs[6 * (size_t)t + 2 * v + 1] = (float)((double)(oy + y) / (double)L.height);
    }
}

__global__ void __launch_bounds__(256) atlas_texels_kernel(long long nv, const double* __restrict__ verts,
                                                           const double* __restrict__ normals, long long nt,
                                                           const int* __restrict__ tris, const int* __restrict__ order, AtlasLayout L,
                                                           int row0, long long n, int* __restrict__ owner,
                                                           unsigned char* __restrict__ interior, double* __restrict__ points,
                                                           double* __restrict__ tnormals) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int X = (int)(i % L.width), Y = row0 + (int)(i / L.width);
    int own = -1;
    bool in = false;
    double p[3] = {0.0, 0.0, 0.0}, N[3] = {0.0, 0.0, 0.0};
    AtlasTexel tx;
    if (atlas_texel(L, X, Y, &tx) && tx.pos < nt) {
        const int t = order[tx.pos];
        if (t >= 0 && t < nt) {
            const int id[3] = {tris[3 * (size_t)t], tris[3 * (size_t)t + 1], tris[3 * (size_t)t + 2]};
            if (id[0] >= 0 && id[1] >= 0 && id[2] >= 0 && id[0] < nv && id[1] < nv && id[2] < nv) {
                own = t;
                double l[3];
                in = atlas_bary(tx.side, tx.half, tx.i, tx.j, l);
                const double *a = verts + 3 * (size_t)id[0], *b = verts + 3 * (size_t)id[1], *c = verts + 3 * (size_t)id[2];
#pragma unroll
                for (int d = 0; d < 3; d++) p[d] = (l[0] * a[d] + l[1] * b[d]) + l[2] * c[d];
                bool smooth = false;
                if (normals) {
                    const double *na = normals + 3 * (size_t)id[0], *nb = normals + 3 * (size_t)id[1], *nc = normals + 3 * (size_t)id[2];
#pragma unroll
                    for (int d = 0; d < 3; d++) N[d] = (l[0] * na[d] + l[1] * nb[d]) + l[2] * nc[d];
                    smooth = isfinite(N[0]) && isfinite(N[1]) && isfinite(N[2]) && !(N[0] == 0.0 && N[1] == 0.0 && N[2] == 0.0);
                }
                if (!smooth) {
                    const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, v[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
                    N[0] = u[1] * v[2] - u[2] * v[1];
                    N[1] = u[2] * v[0] - u[0] * v[2];
                    N[2] = u[0] * v[1] - u[1] * v[0];
                }
            }
        }
    }
    owner[i] = own;
    interior[i] = in ? 1 : 0;
#pragma unroll
    for (int d = 0; d < 3; d++) points[3 * (size_t)i + d] = p[d], tnormals[3 * (size_t)i + d] = N[d];
}

struct AtlasWs {
    uint32_t* key;   // F
    SortBufs sort;   // 4 F
    u64* hist;       // 6
    int* err;        // 2
    char* temp;
    size_t temp_bytes, bytes;
};

AtlasWs carve(char* base, long long nt) {
    Carver c{base, 0};
    AtlasWs w;
    const size_t F = (size_t)(nt > 0 ? nt : 1);
    w.key = c.take<uint32_t>(F);
    w.sort = take_sort_bufs(c, F);
    w.hist = c.take<u64>(ATLAS_CLASSES);
    w.err = c.take<int>(2);
    w.temp_bytes = gs2m_radix_temp_bytes(F, KEY_BITS);
    w.temp = c.take<char>(w.temp_bytes + GS2M_ALIGN);
    w.bytes = c.off;
    return w;
}

int sizes_status(long long nv, long long nt) {
    if (nv < 0 || nt < 0) return GS2M_ERR_INVALID_ARG;
    if (nv > 0x7FFFFFFFll || nt > ATLAS_SORT_LIMIT) return GS2M_ERR_UNSUPPORTED;
    return GS2M_OK;
}

void publish(const AtlasLayout& L, long long* hist, long long* bases, int* dims) {
    for (int k = 0; k < ATLAS_CLASSES; k++) {
        hist[k] = L.hist[k];
        if (bases) bases[k] = L.base[k];
    }
    dims[0] = L.width, dims[1] = L.height;
}

// classes, histogram, layout; with `cells` also the sort and the placement
int run(long long nv, long long nt, const double* verts, const int* tris, double density, void* ws, int* cells, float* uvs, int* order,
        long long* hist, long long* bases, int* dims, hipStream_t s) {
    const int st = sizes_status(nv, nt);
    if (st != GS2M_OK) return st;
    if (!(density > 0.0) || !isfinite(density) || !hist || !dims) return GS2M_ERR_INVALID_ARG;
    const bool place = cells != nullptr;
    if (nt > 0 && (!verts || !tris || !ws || nv == 0)) return GS2M_ERR_INVALID_ARG;
    AtlasLayout L;
    long long h[ATLAS_CLASSES] = {0, 0, 0, 0, 0, 0};
    if (nt == 0) {
        atlas_layout(h, &L);
        publish(L, hist, bases, dims);
        return GS2M_OK;
    }
    const AtlasWs w = carve((char*)ws, nt);
    if (hipMemsetAsync(w.hist, 0, sizeof(u64) * ATLAS_CLASSES, s) != hipSuccess || hipMemsetAsync(w.err, 0, sizeof(int) * 2, s) != hipSuccess)
        return GS2M_ERR_HIP;
    atlas_class_kernel<<<blocks_of(nt), 256, 0, s>>>(nv, verts, nt, tris, density, w.key, w.hist, w.err);
    u64 hd[ATLAS_CLASSES];
    int err[2];
    if (gs2m_read_back(s, {{hd, w.hist, sizeof(hd)}, {err, w.err, sizeof(err)}}) != GS2M_OK) return GS2M_ERR_HIP;
    if (err[0] || err[1]) return GS2M_ERR_INVALID_ARG;
    for (int k = 0; k < ATLAS_CLASSES; k++) h[k] = (long long)hd[k];
    const int ls = atlas_layout(h, &L);
    if (ls == 2) return GS2M_ERR_UNSUPPORTED;
    if (ls != 0) return GS2M_ERR_HIP;  // the histogram does not count nt triangles
    if (place) {
        const SortBufs& b = w.sort;
        if (gs2m_radix_sort_pairs(w.temp, w.temp_bytes, w.key, nullptr, b.kA, b.vA, b.kB, b.vB, (size_t)nt, KEY_BITS, false, s) != hipSuccess)
            return GS2M_ERR_HIP;
        atlas_place_kernel<<<blocks_of(nt), 256, 0, s>>>(nt, L, b.kB, b.vB, cells, uvs, order);
        if (hipGetLastError() != hipSuccess) return GS2M_ERR_HIP;
        const int rc = gs2m_status(hipStreamSynchronize(s));
        if (rc != GS2M_OK) return rc;
    }
    publish(L, hist, bases, dims);
    return GS2M_OK;
}

}  // namespace

extern "C" {

int gs2m_atlas_workspace_bytes(long long n_triangles, long long* bytes) {
    if (!bytes) return GS2M_ERR_INVALID_ARG;
    const int st = sizes_status(0, n_triangles);
    if (st != GS2M_OK) return st;
    *bytes = (long long)carve(nullptr, n_triangles).bytes;
    return GS2M_OK;
}

int gs2m_atlas_count(long long n_vertices, long long n_triangles, const double* vertices, const int* triangles, double density,
                     void* ws, long long* hist, int* dims, void* stream) {
    return run(n_vertices, n_triangles, vertices, triangles, density, ws, nullptr, nullptr, nullptr, hist, nullptr, dims, (hipStream_t)stream);
}

int gs2m_atlas_build(long long n_vertices, long long n_triangles, const double* vertices, const int* triangles, double density,
                     void* ws, int* cells, float* uvs, int* order, long long* hist, long long* bases, int* dims, void* stream) {
    if (!bases || (n_triangles > 0 && (!cells || !uvs || !order))) return GS2M_ERR_INVALID_ARG;
    return run(n_vertices, n_triangles, vertices, triangles, density, ws, cells, uvs, order, hist, bases, dims, (hipStream_t)stream);
}

int gs2m_atlas_texels(long long n_vertices, const double* vertices, const double* normals, long long n_triangles,
                      const int* triangles, const int* order, const long long* hist, int width, int height, int row0, int n_rows,
                      int* owner, unsigned char* interior, double* points, double* tnormals, void* stream) {
    const int st = sizes_status(n_vertices, n_triangles);
    if (st != GS2M_OK) return st;
    if (!hist || row0 < 0 || n_rows < 0) return GS2M_ERR_INVALID_ARG;
    AtlasLayout L;
    const int ls = atlas_layout(hist, &L);
    if (ls == 2) return GS2M_ERR_UNSUPPORTED;
    long long count = 0;
    for (int k = 0; k < ATLAS_CLASSES && ls == 0; k++) count += L.hist[k];
    if (ls != 0 || count != n_triangles || L.width != width || L.height != height || (long long)row0 + n_rows > height)
        return GS2M_ERR_INVALID_ARG;
    const long long n = (long long)n_rows * width;
    if (n == 0) return GS2M_OK;
    if (!vertices || !triangles || !order || !owner || !interior || !points || !tnormals) return GS2M_ERR_INVALID_ARG;
    atlas_texels_kernel<<<blocks_of(n), 256, 0, (hipStream_t)stream>>>(n_vertices, vertices, normals, n_triangles, triangles, order, L, row0, n,
                                                                       owner, interior, points, tnormals);
    return gs2m_status(hipGetLastError());
}

}  // extern "C"
