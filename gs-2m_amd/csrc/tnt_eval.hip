// Tanks and Temples mesh evaluation: mesh points, affine transform, polygon-volume crop, voxel downsample, ICP moment
// reductions and the distance histogram (include/gs2m_tnt.h; the contract: DESIGN.md §11).  The nearest neighbour with its
// index, the compaction and the count below a threshold are mesh_eval.hip's (gs2m_eval.h).
//
// Crop: the polygon travels in the kernel arguments, CROP_EDGES edges per launch; the crossing parity of a point is carried
// from launch to launch in its flag byte, and the last launch applies the axis range.
// Voxel downsample: the cloud's box comes back to the host (it fixes lo and the bits per axis of the key); the keys
// ix : iy : iz sort with the project's stable 32-bit radix sort, low word first and then the high word (LSD), so that the
// members of a voxel stay in input order; a thread per voxel then adds its members one after the other.
// ICP moments and the cloud's box: the fixed-order reduction of eval_common.h (the one of gs2m_eval_masked_mean), several
// quantities at once; the box folds with a NaN-keeping min / max in place of +.
// Every sum is an integer sum or a fixed-order fp64 reduction: two runs are bitwise identical.  Compiled with -ffp-contract=off.
#include <math.h>
#include "eval_common.h"
#include "../../include/gs2m_tnt.h"

namespace {

constexpr int CROP_EDGES = 96;    // polygon edges per launch
constexpr int POLY_MAX = 1024;
constexpr int HIST_MAX_BINS = 4096;
constexpr int HIST_BLOCKS = 1024;
constexpr double VOXEL_LIMIT = 2097152.0;  // 2^21 per axis

struct M34 {
    double m[12];
};

// ---- mesh points, transform, strided gather ----

__global__ void __launch_bounds__(256) centres_kernel(long long nv, const double* __restrict__ verts, long long nt,
                                                      const int* __restrict__ tris, double* __restrict__ cloud, int* __restrict__ err) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const int a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
    double* o = cloud + 3 * (size_t)(nv + t);
    if (!tri_in_range(a, b, c, nv, err)) {
        o[0] = o[1] = o[2] = __builtin_nan("");
        return;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) o[k] = ((verts[3 * (size_t)a + k] + verts[3 * (size_t)b + k]) + verts[3 * (size_t)c + k]) / 3.0;
}

__global__ void __launch_bounds__(256) affine_kernel(long long n, const double* in, M34 T, double* out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
#pragma unroll
    for (int r = 0; r < 3; r++) out[3 * i + r] = ((T.m[4 * r] * x + T.m[4 * r + 1] * y) + T.m[4 * r + 2] * z) + T.m[4 * r + 3];
}

__global__ void __launch_bounds__(256) stride_kernel(long long m, const double* __restrict__ pts, long long k, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
#pragma unroll
    for (int c = 0; c < 3; c++) out[3 * i + c] = pts[3 * (i * k) + c];
}

// ---- crop ----

struct PolyChunk {
    double u[CROP_EDGES + 1], v[CROP_EDGES + 1];  // vertices k0 .. k0 + ne (indices mod m)
    int ne;
};

__global__ void __launch_bounds__(256) crop_kernel(long long n, const double* __restrict__ pts, int au, int av, int aw, PolyChunk c,
                                                   int first, int last, double axis_min, double axis_max,
                                                   unsigned char* __restrict__ flags) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double pu = pts[3 * i + au], pv = pts[3 * i + av];
    unsigned odd = first ? 0u : flags[i];
    for (int e = 0; e < c.ne; e++) {
        const double iu = c.u[e], iv = c.v[e], ju = c.u[e + 1], jv = c.v[e + 1];
        if ((iv < pv && jv >= pv) || (jv < pv && iv >= pv)) {
            const double node = iu + ((pv - iv) / (jv - iv)) * (ju - iu);
            if (node < pu) odd ^= 1u;
        }
    }
    if (last) {
        const double pw = pts[3 * i + aw];
        odd = (odd && pw >= axis_min && pw <= axis_max) ? 1u : 0u;
    }
    flags[i] = (unsigned char)odd;
}

// ---- voxel downsample ----

// min / max that keep a NaN (fmin / fmax drop it): a cloud with a NaN coordinate gets a NaN box, which the host refuses
__device__ __forceinline__ double nmin(double a, double b) { return a != a ? a : (b != b ? b : fmin(a, b)); }
__device__ __forceinline__ double nmax(double a, double b) { return a != a ? a : (b != b ? b : fmax(a, b)); }

// the cloud's box as a fixed-order reduction of 6 quantities: min x, y, z, then max x, y, z
struct BoxOp {
    __device__ static double identity(int q) { return q < 3 ? __builtin_huge_val() : -__builtin_huge_val(); }
    __device__ static double combine(int q, double a, double b) { return q < 3 ? nmin(a, b) : nmax(a, b); }
};
struct BoxTerm {
    const double* pts;
    __device__ void operator()(long long i, double* m, u64&) const {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double x = pts[3 * i + k];
            m[k] = nmin(m[k], x);
            m[3 + k] = nmax(m[3 + k], x);
        }
    }
};

struct VoxelSpec {
    double lo[3], s;
    double imax[3];  // the largest voxel index per axis
    int by, bz;      // key = ix << (by + bz) | iy << bz | iz
};

__device__ __forceinline__ u64 voxel_key(const double* __restrict__ p, const VoxelSpec& v) {
    u64 idx[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double f = floor((p[k] - v.lo[k]) / v.s);
        idx[k] = (u64)(f >= 0.0 && f <= v.imax[k] ? f : v.imax[k]);  // in range for every point of the box (a clamp for safety only)
    }
    return (idx[0] << (v.by + v.bz)) | (idx[1] << v.bz) | idx[2];
}

__global__ void __launch_bounds__(256) voxel_key_kernel(long long n, const double* __restrict__ pts, VoxelSpec v,
                                                        uint32_t* __restrict__ klo, uint32_t* __restrict__ khi) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 key = voxel_key(pts + 3 * i, v);
    klo[i] = (uint32_t)key;
    khi[i] = (uint32_t)(key >> 32);
}

__global__ void __launch_bounds__(256) voxel_regather_kernel(long long n, const uint32_t* __restrict__ order, const uint32_t* __restrict__ khi,
                                                             uint32_t* __restrict__ k2, uint32_t* __restrict__ v2) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = order[j];
    k2[j] = khi[i];
    v2[j] = i;
}

// a[j] = 1 where the sorted slot j opens a voxel
__global__ void __launch_bounds__(256) voxel_head_kernel(long long n, const double* __restrict__ pts, const uint32_t* __restrict__ order,
                                                         VoxelSpec v, u64* __restrict__ a) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    a[j] = j == 0 || voxel_key(pts + 3 * (size_t)order[j], v) != voxel_key(pts + 3 * (size_t)order[j - 1], v) ? 1 : 0;
}

// a: the exclusive prefixes of the heads, a[n] the voxel count.  start[voxel] = its first sorted slot, start[count] = n.
__global__ void __launch_bounds__(256) voxel_start_kernel(long long n, const u64* __restrict__ a, uint32_t* __restrict__ start) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j > n) return;
    if (j == n) start[a[n]] = (uint32_t)n;
    else if (a[j + 1] != a[j]) start[a[j]] = (uint32_t)j;
}

// a thread per voxel: its members one after the other, in input order (the sort is stable)
__global__ void __launch_bounds__(256) voxel_emit_kernel(long long n, const double* __restrict__ pts, const uint32_t* __restrict__ order,
                                                         const u64* __restrict__ a, const uint32_t* __restrict__ start,
                                                         double* __restrict__ out) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n || (u64)v >= a[n]) return;
    const uint32_t b = start[v], e = start[v + 1];
    double s[3] = {0.0, 0.0, 0.0};
    for (uint32_t j = b; j < e; j++) {
        const double* p = pts + 3 * (size_t)order[j];
#pragma unroll
        for (int k = 0; k < 3; k++) s[k] += p[k];
    }
    const double c = (double)(e - b);
#pragma unroll
    for (int k = 0; k < 3; k++) out[3 * v + k] = s[k] / c;
}

struct VoxelWs {
    uint32_t *klo, *khi, *v2;  // n each, as the sort's arrays
    SortBufs sort;
    uint32_t* start;                               // n + 1
    u64* a;                                        // n + 1
    u64* bsum;                                     // scan blocks + 1
    double* part;                                  // 6 RED_BLOCKS + 6
    void* temp;
    size_t temp_bytes, bytes;
};
VoxelWs carve_voxel(char* base, long long n) {
    Carver c{base, 0};
    VoxelWs w;
    const size_t m = (size_t)(n > 0 ? n : 1);
    w.klo = c.take<uint32_t>(m);
    w.khi = c.take<uint32_t>(m);
    w.v2 = c.take<uint32_t>(m);
    w.sort = take_sort_bufs(c, m);
    w.start = c.take<uint32_t>(m + 1);
    w.a = c.take<u64>(m + 1);
    w.bsum = c.take<u64>(gs2m_scan_blocks(n) + 1);
    w.part = c.take<double>(6 * RED_BLOCKS + 6);
    const size_t t32 = gs2m_radix_temp_bytes(m, 32), t16 = gs2m_radix_temp_bytes(m, 16);
    w.temp_bytes = t32 > t16 ? t32 : t16;
    w.temp = c.take<char>(w.temp_bytes + GS2M_ALIGN);
    w.bytes = c.off;
    return w;
}

int bits_for(double imax) {  // bits that hold 0 .. imax
    int b = 1;
    while (b < 21 && (double)(1u << b) <= imax) b++;
    return b;
}

// ---- ICP moments: the terms of the fixed-order sums over the pairs ----

struct Means {
    double mx[3], my[3];
};

// STAGE 0: d^2, x, y (7 sums) and the count; STAGE 1: Sigma (9, row major: rows y, columns x) and sx2, about the means
template <int STAGE>
struct IcpTerm {
    const double *src, *tgt;
    const long long* index;
    long long nt;
    Means mu;
    unsigned* err;
    __device__ void operator()(long long i, double* acc, u64& c) const {
        const long long t = index[i];
        if (t < 0) return;
        if (t >= nt) {  // not an index into these targets: the host refuses the call
            err[0] = 1u;
            return;
        }
        const double x[3] = {src[3 * i], src[3 * i + 1], src[3 * i + 2]};
        const double y[3] = {tgt[3 * t], tgt[3 * t + 1], tgt[3 * t + 2]};
        if (STAGE == 0) {
            const double dx = x[0] - y[0], dy = x[1] - y[1], dz = x[2] - y[2];
            acc[0] += (dx * dx + dy * dy) + dz * dz;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                acc[1 + k] += x[k];
                acc[4 + k] += y[k];
            }
        } else {
            const double a[3] = {x[0] - mu.mx[0], x[1] - mu.mx[1], x[2] - mu.mx[2]};
            const double b[3] = {y[0] - mu.my[0], y[1] - mu.my[1], y[2] - mu.my[2]};
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int k = 0; k < 3; k++) acc[3 * r + k] += b[r] * a[k];
            acc[9] += (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
        }
        c++;
    }
};

struct IcpWs {
    double* psum;  // 10 RED_BLOCKS
    u64* pcnt;     // RED_BLOCKS
    double* tot;   // 10
    u64* cnt;      // 1
    unsigned* err; // 1: an index at or beyond n_targets was met
    size_t bytes;
};
IcpWs carve_icp(char* base) {
    Carver c{base, 0};
    IcpWs w;
    w.psum = c.take<double>(10 * RED_BLOCKS);
    w.pcnt = c.take<u64>(RED_BLOCKS);
    w.tot = c.take<double>(10);
    w.cnt = c.take<u64>(1);
    w.err = c.take<unsigned>(1);
    w.bytes = c.off;
    return w;
}

// ---- histogram ----

__global__ void __launch_bounds__(256) hist_kernel(long long n, const double* __restrict__ dist, int ne, const double* __restrict__ edges,
                                                   u64* __restrict__ counts) {
    __shared__ unsigned s_h[HIST_MAX_BINS];
    const int nbins = ne - 1;
    for (int k = threadIdx.x; k < nbins; k += 256) s_h[k] = 0u;
    __syncthreads();
    const double e0 = edges[0], e1 = edges[ne - 1];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double x = dist[i];
        if (!(x >= e0 && x <= e1)) continue;
        int lo = 0, hi = ne;  // edges[lo] <= x, the answer in [lo, hi)
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (edges[mid] <= x) lo = mid;
            else hi = mid;
        }
        atomicAdd(&s_h[lo < nbins ? lo : nbins - 1], 1u);  // x == the last edge: the last bin is closed
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nbins; k += 256)
        if (s_h[k]) atomicAdd(&counts[k], (u64)s_h[k]);
}

}  // namespace

extern "C" {

int gs2m_tnt_mesh_points(long long n_verts, const double* verts, long long n_tris, const int* tris, void* ws, double* cloud,
                         void* stream) {
    if (n_verts < 0 || n_tris < 0 || !ws || (n_verts + n_tris > 0 && !cloud) || (n_verts > 0 && !verts) || (n_tris > 0 && !tris))
        return GS2M_ERR_INVALID_ARG;
    if (n_tris > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    int* err = (int*)ws;
    if (hipMemsetAsync(err, 0, 8, s) != hipSuccess) return GS2M_ERR_HIP;
    if (n_verts > 0 && hipMemcpyAsync(cloud, verts, 24 * (size_t)n_verts, hipMemcpyDeviceToDevice, s) != hipSuccess) return GS2M_ERR_HIP;
    if (n_tris > 0) centres_kernel<<<blocks_of(n_tris), 256, 0, s>>>(n_verts, verts, n_tris, tris, cloud, err);
    int bad = 0;
    if (gs2m_read_back(s, {{&bad, err, 4}}) != GS2M_OK) return GS2M_ERR_HIP;
    return bad ? GS2M_ERR_INVALID_ARG : GS2M_OK;
}

int gs2m_tnt_transform(long long n, const double* in, const double* T, double* out, void* stream) {
    if (n < 0 || !T || (n > 0 && (!in || !out))) return GS2M_ERR_INVALID_ARG;
    if (!(T[12] == 0.0 && T[13] == 0.0 && T[14] == 0.0 && T[15] == 1.0)) return GS2M_ERR_INVALID_ARG;
    if (n == 0) return GS2M_OK;
    if (n > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    M34 m;
    for (int k = 0; k < 12; k++) m.m[k] = T[k];
    affine_kernel<<<blocks_of(n), 256, 0, (hipStream_t)stream>>>(n, in, m, out);
    return gs2m_status(hipGetLastError());
}

int gs2m_tnt_crop_flags(long long n, const double* pts, int axis, double axis_min, double axis_max, int m, const double* polygon,
                        unsigned char* flags, void* stream) {
    if (n < 0 || axis < 0 || axis > 2 || m < 0 || (m > 0 && !polygon) || (n > 0 && (!pts || !flags))) return GS2M_ERR_INVALID_ARG;
    if (m > POLY_MAX || n > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    if (n == 0) return GS2M_OK;
    hipStream_t s = (hipStream_t)stream;
    if (m == 0) return gs2m_status(hipMemsetAsync(flags, 0, (size_t)n, s));
    const int uvw[3][3] = {{1, 2, 0}, {0, 2, 1}, {0, 1, 2}};
    const int au = uvw[axis][0], av = uvw[axis][1], aw = uvw[axis][2];
    for (int k0 = 0; k0 < m; k0 += CROP_EDGES) {
        PolyChunk c;
        c.ne = m - k0 < CROP_EDGES ? m - k0 : CROP_EDGES;
        for (int e = 0; e <= c.ne; e++) {
            const double* P = polygon + 3 * (size_t)((k0 + e) % m);
            c.u[e] = P[au];
            c.v[e] = P[av];
        }
        for (int e = c.ne + 1; e <= CROP_EDGES; e++) c.u[e] = c.v[e] = 0.0;
        crop_kernel<<<blocks_of(n), 256, 0, s>>>(n, pts, au, av, aw, c, k0 == 0, k0 + CROP_EDGES >= m, axis_min, axis_max, flags);
    }
    return gs2m_status(hipGetLastError());
}

int gs2m_tnt_voxel_workspace_bytes(long long n, long long* bytes) {
    if (n < 0 || !bytes) return GS2M_ERR_INVALID_ARG;
    if (n > MAX_POINTS) return GS2M_ERR_UNSUPPORTED;
    *bytes = (long long)carve_voxel(nullptr, n).bytes;
    return GS2M_OK;
}

int gs2m_tnt_voxel_downsample(long long n, const double* pts, double s, void* ws, double* out, long long* host_count,
                              void* stream) {
    if (n < 0 || !(s > 0.0) || !ws || !host_count || (n > 0 && (!pts || !out))) return GS2M_ERR_INVALID_ARG;
    if (n > MAX_POINTS) return GS2M_ERR_UNSUPPORTED;
    *host_count = 0;
    if (n == 0) return GS2M_OK;
    hipStream_t st = (hipStream_t)stream;
    const VoxelWs w = carve_voxel((char*)ws, n);
    reduce_fixed_order<6, BoxOp>(n, BoxTerm{pts}, w.part, nullptr, w.part + 6 * RED_BLOCKS, nullptr, st);
    double box[6];
    if (gs2m_read_back(st, {{box, w.part + 6 * RED_BLOCKS, sizeof(box)}}) != GS2M_OK) return GS2M_ERR_HIP;
    VoxelSpec v;
    v.s = s;
    int bits[3];
    for (int k = 0; k < 3; k++) {
        v.lo[k] = box[k] - s * 0.5;
        v.imax[k] = floor((box[3 + k] - v.lo[k]) / s);  // the index is monotone in the coordinate: the box's far corner has the largest
        if (!(v.imax[k] >= 0.0 && v.imax[k] < VOXEL_LIMIT)) return GS2M_ERR_INVALID_ARG;
        bits[k] = bits_for(v.imax[k]);
    }
    v.by = bits[1];
    v.bz = bits[2];
    const int total = bits[0] + bits[1] + bits[2];
    voxel_key_kernel<<<blocks_of(n), 256, 0, st>>>(n, pts, v, w.klo, w.khi);
    if (hipGetLastError() != hipSuccess) return GS2M_ERR_HIP;
    const SortBufs& b = w.sort;
    if (gs2m_radix_sort_pairs(w.temp, w.temp_bytes, w.klo, nullptr, b.kA, b.vA, b.kB, b.vB, (size_t)n, total < 32 ? total : 32, false, st) !=
        hipSuccess)
        return GS2M_ERR_HIP;
    if (total > 32) {
        // LSD: the order by the low word, then stably by the high word (klo is free again: it takes the gathered high words)
        voxel_regather_kernel<<<blocks_of(n), 256, 0, st>>>(n, b.vB, w.khi, w.klo, w.v2);
        if (hipGetLastError() != hipSuccess ||
            gs2m_radix_sort_pairs(w.temp, w.temp_bytes, w.klo, w.v2, b.kA, b.vA, b.kB, b.vB, (size_t)n, total - 32, false, st) != hipSuccess)
            return GS2M_ERR_HIP;
    }
    voxel_head_kernel<<<blocks_of(n), 256, 0, st>>>(n, pts, b.vB, v, w.a);
    if (hipGetLastError() != hipSuccess || gs2m_scan_u64(w.a, n, w.bsum, st) != hipSuccess) return GS2M_ERR_HIP;
    voxel_start_kernel<<<blocks_of(n + 1), 256, 0, st>>>(n, w.a, w.start);
    voxel_emit_kernel<<<blocks_of(n), 256, 0, st>>>(n, pts, b.vB, w.a, w.start, out);
    u64 total_voxels;
    if (gs2m_read_back(st, {{&total_voxels, w.a + n, 8}}) != GS2M_OK) return GS2M_ERR_HIP;
    *host_count = (long long)total_voxels;
    return GS2M_OK;
}

int gs2m_tnt_stride_gather(long long n, const double* pts, long long k, double* out, void* stream) {
    if (n < 0 || k < 1 || (n > 0 && (!pts || !out))) return GS2M_ERR_INVALID_ARG;
    if (n == 0) return GS2M_OK;
    const long long m = (n + k - 1) / k;  // rows 0, k, 2k, ... < n
    if (m > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    stride_kernel<<<blocks_of(m), 256, 0, (hipStream_t)stream>>>(m, pts, k, out);
    return gs2m_status(hipGetLastError());
}

int gs2m_tnt_icp_workspace_bytes(long long* bytes) {
    if (!bytes) return GS2M_ERR_INVALID_ARG;
    *bytes = (long long)carve_icp(nullptr).bytes;
    return GS2M_OK;
}

int gs2m_tnt_icp_moments(long long n, const double* source, long long n_targets, const double* targets, const long long* index,
                         void* ws, long long* host_count, double* host_out, void* stream) {
    if (n < 0 || n_targets < 0 || !ws || !host_count || !host_out || (n > 0 && (!source || !index)) || (n_targets > 0 && !targets))
        return GS2M_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    const IcpWs w = carve_icp((char*)ws);
    for (int k = 0; k < 17; k++) host_out[k] = 0.0;
    *host_count = 0;
    Means mu = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    if (hipMemsetAsync(w.err, 0, 4, s) != hipSuccess) return GS2M_ERR_HIP;
    reduce_fixed_order<7, SumOp>(n, IcpTerm<0>{source, targets, index, n_targets, mu, w.err}, w.psum, w.pcnt, w.tot, w.cnt, s);
    double t[10];
    u64 c;
    unsigned bad = 0;
    if (gs2m_read_back(s, {{t, w.tot, 7 * 8}, {&c, w.cnt, 8}, {&bad, w.err, 4}}) != GS2M_OK) return GS2M_ERR_HIP;
    if (bad) return GS2M_ERR_INVALID_ARG;
    if (c == 0) return GS2M_OK;
    const double cd = (double)c;
    *host_count = (long long)c;
    host_out[0] = t[0];
    for (int k = 0; k < 3; k++) {
        host_out[1 + k] = mu.mx[k] = t[1 + k] / cd;
        host_out[4 + k] = mu.my[k] = t[4 + k] / cd;
    }
    reduce_fixed_order<10, SumOp>(n, IcpTerm<1>{source, targets, index, n_targets, mu, w.err}, w.psum, w.pcnt, w.tot, w.cnt, s);
    if (gs2m_read_back(s, {{t, w.tot, 10 * 8}}) != GS2M_OK) return GS2M_ERR_HIP;
    for (int k = 0; k < 10; k++) host_out[7 + k] = t[k] / cd;
    return GS2M_OK;
}

int gs2m_tnt_histogram(long long n, const double* dist, int n_edges, const double* edges, unsigned long long* counts,
                       void* stream) {
    if (n < 0 || n_edges < 2 || n_edges > HIST_MAX_BINS + 1 || !edges || !counts || (n > 0 && !dist)) return GS2M_ERR_INVALID_ARG;
    if (n == 0) return GS2M_OK;
    const long long nb = (n + 255) / 256;
    hist_kernel<<<(unsigned)(nb < HIST_BLOCKS ? nb : HIST_BLOCKS), 256, 0, (hipStream_t)stream>>>(n, dist, n_edges, edges, counts);
    return gs2m_status(hipGetLastError());
}

}  // extern "C"
