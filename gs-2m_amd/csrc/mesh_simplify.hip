// Mesh simplification: vertex clustering on a uniform lattice with quadric placement (include/gs2m_simplify.h has the
// contract, DESIGN.md §21 the plan).
//
// Keys: a reduction finds the occupied index range per axis (integer atomicMin / atomicMax of the biased fp64 floor, one per
// wave); every vertex packs its three relative indices into one key of bx + by + bz <= 63 bits, x uppermost, and the keys
// sort with the project's stable 32-bit radix sort, the low word first and then the high word (LSD; one sort when the key
// fits 32 bits).  Head flags of the sorted keys go through gs2m_scan_u64: the cells come out numbered in (ix, iy, iz) order
// with their vertices in input order.  Quadrics: every triangle writes a slot per DISTINCT cell of its corners, the slots sort
// by cell, and a cell's run is summed in the header's fixed order.  Segments: sixteen lanes per cell (seg_short_kernel); a
// cell with more than LONG_SEG elements is appended to a list (integer atomic: the list's order changes no result) and gets a
// whole workgroup (seg_long_kernel).  Placement: a thread per cell, Jacobi in registers.  Triangles: the sorted cell triple
// of every surviving triangle sorts hi, mid, lo (stable, so the first of a run is the smallest input index); run heads are
// kept and gs2m_mesh_compact renumbers; its scan (CompactWs::av) is read for the attributes and vertex_map.
// No floating-point atomics anywhere: two runs are bitwise identical.
#include <chrono>
#include <cmath>
#include "eval_common.h"
#include "../../include/gs2m_mesh.h"
#include "../../include/gs2m_simplify.h"

namespace {

constexpr int GROUP = 16;         // lanes per cell in seg_short_kernel
constexpr int LONG_SEG = 256;     // a longer segment goes to seg_long_kernel
constexpr int LONG_BLOCKS = 256;  // its grid: workgroups that walk the list
constexpr long long IDX_BIAS = 1ll << 52;
constexpr long long SORT_LIMIT = 0x3FFFFFFFll;

struct Lattice {
    double cell;
    long long mn[3];  // smallest occupied index per axis
    int bits[3];      // bits that hold the relative indices
};

__device__ __forceinline__ u64 cell_key(const Lattice& L, float x, float y, float z) {
    const u64 rx = (u64)((long long)floor((double)x / L.cell) - L.mn[0]);
    const u64 ry = (u64)((long long)floor((double)y / L.cell) - L.mn[1]);
    const u64 rz = (u64)((long long)floor((double)z / L.cell) - L.mn[2]);
    return (rx << (L.bits[1] + L.bits[2])) | (ry << L.bits[2]) | rz;
}

__device__ __forceinline__ void key_centre(const Lattice& L, u64 key, double c[3]) {
    const u64 rz = key & ((1ull << L.bits[2]) - 1), ry = (key >> L.bits[2]) & ((1ull << L.bits[1]) - 1);
    const u64 rx = key >> (L.bits[1] + L.bits[2]);
    c[0] = ((double)((long long)rx + L.mn[0]) + 0.5) * L.cell;
    c[1] = ((double)((long long)ry + L.mn[1]) + 0.5) * L.cell;
    c[2] = ((double)((long long)rz + L.mn[2]) + 0.5) * L.cell;
}

// ---- keys ----

// mm[0..2] = min, mm[3..5] = max of floor(x / cell) + IDX_BIAS per axis; err[0]: a non-finite coordinate, err[1]: an index
// beyond 2^52
__global__ void __launch_bounds__(256) bounds_kernel(long long nv, const float* __restrict__ v, double cell, u64* __restrict__ mm,
                                                     int* __restrict__ err) {
    u64 lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0, 0, 0};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float x = v[3 * i + k];
            if (!isfinite(x)) {
                err[0] = 1;
                continue;
            }
            const double f = floor((double)x / cell);
            if (!(fabs(f) < (double)IDX_BIAS)) {
                err[1] = 1;
                continue;
            }
            const u64 u = (u64)((long long)f + IDX_BIAS);
            lo[k] = u < lo[k] ? u : lo[k];
            hi[k] = u > hi[k] ? u : hi[k];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const u64 a = __shfl_down(lo[k], o, 64), b = __shfl_down(hi[k], o, 64);
            lo[k] = a < lo[k] ? a : lo[k];
            hi[k] = b > hi[k] ? b : hi[k];
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            atomicMin(mm + k, lo[k]);
            atomicMax(mm + 3 + k, hi[k]);
        }
    }
}

__global__ void __launch_bounds__(256) check_triangles_kernel(long long nv, long long nt, const int* __restrict__ tris, int* __restrict__ err) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < nt) tri_in_range(tris[3 * t], tris[3 * t + 1], tris[3 * t + 2], nv, err);
}

__global__ void __launch_bounds__(256) key_kernel(long long nv, const float* __restrict__ v, Lattice L, uint32_t* __restrict__ klo,
                                                  uint32_t* __restrict__ khi) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const u64 key = cell_key(L, v[3 * i], v[3 * i + 1], v[3 * i + 2]);
    klo[i] = (uint32_t)key;
    khi[i] = (uint32_t)(key >> 32);
}

__global__ void __launch_bounds__(256) regather_kernel(long long m, const uint32_t* __restrict__ order, const uint32_t* __restrict__ key,
                                                       uint32_t* __restrict__ k2, uint32_t* __restrict__ v2) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const uint32_t s = order[j];
    k2[j] = key[s];
    v2[j] = s;
}

// sorted position j: sidx[j] = its vertex, flag[j] = its key differs from that of j - 1
__global__ void __launch_bounds__(256) head_kernel(long long nv, const uint32_t* __restrict__ order, const uint32_t* __restrict__ klo,
                                                   const uint32_t* __restrict__ khi, uint32_t* __restrict__ sidx, u64* __restrict__ flag) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= nv) return;
    const uint32_t v = order[j];
    sidx[j] = v;
    bool head = j == 0;
    if (!head) {
        const uint32_t u = order[j - 1];
        head = klo[u] != klo[v] || khi[u] != khi[v];
    }
    flag[j] = head ? 1ull : 0ull;
}

// a: the exclusive prefixes of the head flags, a[nv] = the cell count.  vcell[v] = v's cell, cstart[c] = the cell's first
// sorted position, cstart[cells] = nv.
__global__ void __launch_bounds__(256) assign_kernel(long long nv, const u64* __restrict__ a, const uint32_t* __restrict__ sidx,
                                                     int* __restrict__ vcell, uint32_t* __restrict__ cstart) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= nv) return;
    const u64 before = a[j];
    const bool head = a[j + 1] != before;
    const u64 c = head ? before : before - 1;
    vcell[sidx[j]] = (int)c;
    if (head) cstart[c] = (uint32_t)j;
    if (j == nv - 1) cstart[a[nv]] = (uint32_t)nv;
}

// ---- triangles ----

// ctri: the corners' cells; ikey (may be null): a slot per distinct cell of the triangle, `nc` for a repeated one; the
// sorted triple (lo, mid, hi) of a triangle whose cells differ pairwise, (nc, nc, nc) otherwise
__global__ void __launch_bounds__(256) remap_kernel(long long nv, long long nt, uint32_t nc, const int* __restrict__ tris,
                                                    const int* __restrict__ vcell, int* __restrict__ ctri, uint32_t* __restrict__ ikey,
                                                    uint32_t* __restrict__ tlo, uint32_t* __restrict__ tmid, uint32_t* __restrict__ thi,
                                                    int* __restrict__ err) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const int a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
    uint32_t c0 = nc, c1 = nc, c2 = nc;
    const bool ok = tri_in_range(a, b, c, nv, err);
    if (ok) {
        c0 = (uint32_t)vcell[a];
        c1 = (uint32_t)vcell[b];
        c2 = (uint32_t)vcell[c];
    }
    ctri[3 * t] = ok ? (int)c0 : 0;
    ctri[3 * t + 1] = ok ? (int)c1 : 0;
    ctri[3 * t + 2] = ok ? (int)c2 : 0;
    if (ikey) {
        ikey[3 * t] = c0;
        ikey[3 * t + 1] = c1 != c0 ? c1 : nc;
        ikey[3 * t + 2] = c2 != c0 && c2 != c1 ? c2 : nc;
    }
    const bool distinct = ok && c0 != c1 && c1 != c2 && c0 != c2;
    const uint32_t lo = min(c0, min(c1, c2)), hi = max(c0, max(c1, c2));
    const uint32_t mid = c0 ^ c1 ^ c2 ^ lo ^ hi;
    tlo[t] = distinct ? lo : nc;
    tmid[t] = distinct ? mid : nc;
    thi[t] = distinct ? hi : nc;
}

// sorted position j (by lo, mid, hi; ties in input order): keep[t] = t heads its run and its triple is a real one
__global__ void __launch_bounds__(256) keep_heads_kernel(long long nt, uint32_t nc, const uint32_t* __restrict__ slo, const uint32_t* __restrict__ order,
                                                         const uint32_t* __restrict__ tmid, const uint32_t* __restrict__ thi,
                                                         unsigned char* __restrict__ keep) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= nt) return;
    const uint32_t t = order[j];
    bool head = j == 0;
    if (!head) {
        const uint32_t u = order[j - 1];
        head = slo[j] != slo[j - 1] || tmid[t] != tmid[u] || thi[t] != thi[u];
    }
    keep[t] = head && slo[j] != nc ? 1 : 0;
}

// count only: used[c] = 1 for the cells of the kept triangles, cnt[0] += kept triangles
__global__ void __launch_bounds__(256) mark_cells_kernel(long long nt, const unsigned char* __restrict__ keep, const int* __restrict__ ctri,
                                                         unsigned char* __restrict__ used, u64* __restrict__ cnt) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool k = t < nt && keep[t] != 0;
    if (k) used[ctri[3 * t]] = used[ctri[3 * t + 1]] = used[ctri[3 * t + 2]] = 1;
    const u64 b = __ballot(k);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(cnt, (u64)__popcll(b));
}

__global__ void __launch_bounds__(256) count_used_kernel(long long nc, const unsigned char* __restrict__ used, u64* __restrict__ cnt) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    const u64 b = __ballot(c < nc && used[c] != 0);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(cnt + 1, (u64)__popcll(b));
}

// ---- segmented fixed-order sums ----
// Fn: Ctx; range(c, s, e); begin(c, ch, ctx); add(ctx, j, acc); finish(c, ch, ctx, n, acc).  blockIdx.y = ch.

template <int Q, class Fn>
__global__ void __launch_bounds__(256) seg_short_kernel(long long nc, Fn fn, uint32_t* __restrict__ list, uint32_t* __restrict__ count) {
    const int lane = threadIdx.x & (GROUP - 1);
    const long long c = ((long long)blockIdx.x * 256 + threadIdx.x) / GROUP;
    const int ch = blockIdx.y;
    long long s = 0, e = 0;
    typename Fn::Ctx ctx;
    bool live = c < nc;
    if (live) {
        fn.range(c, s, e);
        if (e - s > LONG_SEG) {
            if (lane == 0 && list) list[atomicAdd(count, 1u)] = (uint32_t)c;
            live = false;
            e = s;
        } else {
            fn.begin(c, ch, ctx);
        }
    }
    double acc[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) acc[q] = 0.0;
    for (long long j = s + lane; j < e; j += GROUP) fn.add(ctx, j, acc);
#pragma unroll
    for (int o = GROUP / 2; o > 0; o >>= 1) {
#pragma unroll
        for (int q = 0; q < Q; q++) acc[q] += __shfl_down(acc[q], o, GROUP);
    }
    if (live && lane == 0) fn.finish(c, ch, ctx, e - s, acc);
}

template <int Q, class Fn>
__global__ void __launch_bounds__(256) seg_long_kernel(Fn fn, const uint32_t* __restrict__ list, const uint32_t* __restrict__ count) {
    __shared__ double s_a[4][Q];
    const int ch = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t n = *count;
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const long long c = list[i];
        long long s, e;
        typename Fn::Ctx ctx;
        fn.range(c, s, e);
        fn.begin(c, ch, ctx);
        double acc[Q];
#pragma unroll
        for (int q = 0; q < Q; q++) acc[q] = 0.0;
        for (long long j = s + threadIdx.x; j < e; j += 256) fn.add(ctx, j, acc);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
            for (int q = 0; q < Q; q++) acc[q] += __shfl_down(acc[q], o, 64);
        }
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < Q; q++) s_a[w][q] = acc[q];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int q = 0; q < Q; q++) acc[q] = (s_a[0][q] + s_a[1][q]) + (s_a[2][q] + s_a[3][q]);
            fn.finish(c, ch, ctx, e - s, acc);
        }
        __syncthreads();
    }
}

struct Centre {
    double c[3];
};

// what the functors share: the cell's centre from the key of its first vertex
struct CellBase {
    Lattice L;
    const uint32_t *klo, *khi, *sidx, *cstart;
    __device__ void centre(long long c, double out[3]) const {
        const uint32_t v = sidx[cstart[c]];
        key_centre(L, (u64)klo[v] | ((u64)khi[v] << 32), out);
    }
};

// the vertices of a cell: sum of (p - centre) and of the weights -> cq[12 c + 0..2] = the mean, wsum[c]
struct VertexSums : CellBase {
    typedef Centre Ctx;
    const float *v, *w;
    double *cq, *wsum;
    __device__ void range(long long c, long long& s, long long& e) const {
        s = cstart[c];
        e = cstart[c + 1];
    }
    __device__ void begin(long long c, int, Ctx& ctx) const { centre(c, ctx.c); }
    __device__ void add(const Ctx& ctx, long long j, double acc[4]) const {
        const uint32_t i = sidx[j];
#pragma unroll
        for (int k = 0; k < 3; k++) acc[k] += (double)v[3 * (size_t)i + k] - ctx.c[k];
        acc[3] += w ? (double)w[i] : 1.0;
    }
    __device__ void finish(long long c, int, const Ctx&, long long n, const double acc[4]) const {
#pragma unroll
        for (int k = 0; k < 3; k++) cq[12 * c + k] = acc[k] / (double)n;
        wsum[c] = acc[3];
    }
};

// channel ch of a cell: sum(w a) and sum(a) -> cattr[c nch + ch]
struct AttributeSums : CellBase {
    struct Ctx {
        int ch;
    };
    const float *attr, *w;
    const double* wsum;
    float* cattr;
    int nch;
    __device__ void range(long long c, long long& s, long long& e) const {
        s = cstart[c];
        e = cstart[c + 1];
    }
    __device__ void begin(long long, int ch, Ctx& ctx) const { ctx.ch = ch; }
    __device__ void add(const Ctx& ctx, long long j, double acc[2]) const {
        const uint32_t i = sidx[j];
        const double a = (double)attr[(size_t)i * nch + ctx.ch];
        acc[0] += (w ? (double)w[i] : 1.0) * a;
        acc[1] += a;
    }
    __device__ void finish(long long c, int ch, const Ctx&, long long n, const double acc[2]) const {
        const double ws = wsum[c];
        cattr[(size_t)c * nch + ch] = (float)(ws == 0.0 ? acc[1] / (double)n : acc[0] / ws);
    }
};

// the triangles of a cell: its run [lower_bound(c), lower_bound(c + 1)) of the sorted slots -> cq[12 c + 3..11] = A (xx, xy, xz,
// yy, yz, zz) and b
struct QuadricSums : CellBase {
    typedef Centre Ctx;
    const uint32_t *skey, *slot;  // the 3 F slots sorted by cell
    long long m;
    const float* v;
    const int* tris;
    double* cq;
    __device__ long long lower(uint32_t key) const {
        long long lo = 0, hi = m;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (skey[mid] < key) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    }
    __device__ void range(long long c, long long& s, long long& e) const {
        s = lower((uint32_t)c);
        e = lower((uint32_t)c + 1u);
    }
    __device__ void begin(long long c, int, Ctx& ctx) const { centre(c, ctx.c); }
    __device__ void add(const Ctx& ctx, long long j, double acc[9]) const {
        const size_t t = slot[j] / 3u;
        double p[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const size_t id = (size_t)tris[3 * t + i];  // tested by check_triangles_kernel: the call has returned otherwise
#pragma unroll
            for (int k = 0; k < 3; k++) p[i][k] = (double)v[3 * id + k] - ctx.c[k];
        }
        const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
        const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
        const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        if (!(len > 0.0)) return;
        const double d = -(n[0] * p[0][0] + n[1] * p[0][1] + n[2] * p[0][2]);
        acc[0] += n[0] * n[0] / len;
        acc[1] += n[0] * n[1] / len;
        acc[2] += n[0] * n[2] / len;
        acc[3] += n[1] * n[1] / len;
        acc[4] += n[1] * n[2] / len;
        acc[5] += n[2] * n[2] / len;
        acc[6] += n[0] * d / len;
        acc[7] += n[1] * d / len;
        acc[8] += n[2] * d / len;
    }
    __device__ void finish(long long c, int, const Ctx&, long long, const double acc[9]) const {
#pragma unroll
        for (int q = 0; q < 9; q++) cq[12 * c + 3 + q] = acc[q];
    }
};

// ---- placement ----

template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double a[3][3], double u[3][3]) {
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double x = a[k][P], y = a[k][Q];
        a[k][P] = c * x - s * y;
        a[k][Q] = s * x + c * y;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double x = a[P][k], y = a[Q][k];
        a[P][k] = c * x - s * y;
        a[Q][k] = s * x + c * y;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double x = u[k][P], y = u[k][Q];
        u[k][P] = c * x - s * y;
        u[k][Q] = s * x + c * y;
    }
}

__global__ void __launch_bounds__(256) place_kernel(long long nc, CellBase cb, const double* __restrict__ cq, const double* __restrict__ wsum,
                                                    float* __restrict__ cellpos, float* __restrict__ cw) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= nc) return;
    const double* q = cq + 12 * c;
    const double m[3] = {q[0], q[1], q[2]};
    const double A[3][3] = {{q[3], q[4], q[5]}, {q[4], q[6], q[7]}, {q[5], q[7], q[8]}};
    const double b[3] = {q[9], q[10], q[11]};
    double a[3][3], u[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            a[i][k] = A[i][k];
            u[i][k] = i == k ? 1.0 : 0.0;
        }
    }
    for (int sweep = 0; sweep < GS2M_SIMPLIFY_SWEEPS; sweep++) {
        jacobi_rotate<0, 1>(a, u);
        jacobi_rotate<0, 2>(a, u);
        jacobi_rotate<1, 2>(a, u);
    }
    const double l[3] = {a[0][0], a[1][1], a[2][2]};
    const double lmax = fmax(l[0], fmax(l[1], l[2]));
    double x[3] = {m[0], m[1], m[2]};
    if (lmax > 0.0) {
        double r[3], y[3];
#pragma unroll
        for (int i = 0; i < 3; i++) r[i] = -b[i] - (A[i][0] * m[0] + A[i][1] * m[1] + A[i][2] * m[2]);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double inv = l[k] > 1e-3 * lmax ? 1.0 / l[k] : 0.0;
            y[k] = (u[0][k] * r[0] + u[1][k] * r[1] + u[2][k] * r[2]) * inv;
        }
        double z[3];
        bool inside = true;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            z[i] = m[i] + (u[i][0] * y[0] + u[i][1] * y[1] + u[i][2] * y[2]);
            inside = inside && fabs(z[i]) <= 0.5 * cb.L.cell;
        }
        if (inside) {
#pragma unroll
            for (int i = 0; i < 3; i++) x[i] = z[i];
        }
    }
    double ctr[3];
    cb.centre(c, ctr);
#pragma unroll
    for (int k = 0; k < 3; k++) cellpos[3 * c + k] = (float)(ctr[k] + x[k]);
    cw[c] = (float)wsum[c];
}

// ---- outputs that follow gs2m_mesh_compact's numbering (av: its scan) ----

__global__ void __launch_bounds__(256) gather_cells_kernel(long long nc, int nch, const u64* __restrict__ av, const float* __restrict__ cattr,
                                                           const float* __restrict__ cw, float* __restrict__ out_attr, float* __restrict__ out_w) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= nc) return;
    const u64 d = av[c];
    if (av[c + 1] == d) return;
    if (out_attr)
        for (int k = 0; k < nch; k++) out_attr[(size_t)d * nch + k] = cattr[(size_t)c * nch + k];
    if (out_w) out_w[d] = cw[c];
}

__global__ void __launch_bounds__(256) vertex_map_kernel(long long nv, const int* __restrict__ vcell, const u64* __restrict__ av, int* __restrict__ vmap) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const int c = vcell[i];
    const u64 d = av[c];
    vmap[i] = av[c + 1] != d ? (int)d : -1;
}

// ---- host ----

struct SimplifyWs {
    uint32_t *klo, *khi, *sidx, *cstart;  // V, V, V, V + 1
    int* vcell;                           // V
    SortBufs sort;                        // M = max(V, 3 F) each
    uint32_t *k2, *v2;                    // M
    uint32_t *ikey, *tlo, *tmid, *thi;    // 3 F, F, F, F
    int* ctri;                            // 3 F
    unsigned char *keep, *used;           // F, V
    u64 *a, *bsum;                        // max(V, F) + 1
    double *cq, *wsum;                    // 12 V, V
    float *cellpos, *cattr, *cw;          // 3 V, nch V, V
    uint32_t *vlist, *tlist;              // long cells
    u64* mm;                              // 6 bounds + 2 counts
    uint32_t* lcount;                     // 2
    int* err;                             // 4
    void *temp, *compact;
    size_t temp_bytes, bytes;
};

SimplifyWs carve(char* base, long long nv, long long nt, int nch) {
    Carver c{base, 0};
    SimplifyWs w;
    const size_t V = (size_t)(nv > 0 ? nv : 1), F = (size_t)(nt > 0 ? nt : 1), M = V > 3 * F ? V : 3 * F;
    w.klo = c.take<uint32_t>(V);
    w.khi = c.take<uint32_t>(V);
    w.sidx = c.take<uint32_t>(V);
    w.cstart = c.take<uint32_t>(V + 1);
    w.vcell = c.take<int>(V);
    w.sort = take_sort_bufs(c, M);
    w.k2 = c.take<uint32_t>(M);
    w.v2 = c.take<uint32_t>(M);
    w.ikey = c.take<uint32_t>(3 * F);
    w.tlo = c.take<uint32_t>(F);
    w.tmid = c.take<uint32_t>(F);
    w.thi = c.take<uint32_t>(F);
    w.ctri = c.take<int>(3 * F);
    w.keep = c.take<unsigned char>(F);
    w.used = c.take<unsigned char>(V);
    const long long longest = nv > nt ? nv : nt;
    w.a = c.take<u64>((size_t)longest + 1);
    w.bsum = c.take<u64>(gs2m_scan_blocks(longest) + 1);
    w.cq = c.take<double>(12 * V);
    w.wsum = c.take<double>(V);
    w.cellpos = c.take<float>(3 * V);
    w.cattr = c.take<float>(V * (size_t)(nch > 0 ? nch : 1));
    w.cw = c.take<float>(V);
    w.vlist = c.take<uint32_t>(V / LONG_SEG + 1);
    w.tlist = c.take<uint32_t>(3 * F / LONG_SEG + 1);
    w.mm = c.take<u64>(8);
    w.lcount = c.take<uint32_t>(2);
    w.err = c.take<int>(4);
    w.temp_bytes = gs2m_radix_temp_bytes(M, 32);
    w.temp = c.take<char>(w.temp_bytes + GS2M_ALIGN);
    w.compact = c.take<char>(carve_compact(nullptr, nv, nt).bytes);
    w.bytes = c.off;
    return w;
}

int bits_holding(long long vmax) {  // bits that hold 0 .. vmax
    int b = 1;
    while (b < 62 && (1ll << b) <= vmax) b++;
    return b;
}

int sizes_status(long long nv, long long nt, int nch) {
    if (nv < 0 || nt < 0 || nch < 0) return GS2M_ERR_INVALID_ARG;
    if (nv > 0x7FFFFFFFll || 3 * nt > MAX_POINTS || nv > SORT_LIMIT || 3 * nt > SORT_LIMIT) return GS2M_ERR_UNSUPPORTED;
    return GS2M_OK;
}

bool g_timing = false;
float g_stage_ms[5] = {0, 0, 0, 0, 0};

// stage times: only with timing on, and then with a wait for the stream at every stage boundary
struct StageClock {
    hipStream_t s;
    std::chrono::steady_clock::time_point t0;
    explicit StageClock(hipStream_t stream) : s(stream) {
        if (g_timing) {
            for (float& m : g_stage_ms) m = 0.f;
            (void)hipStreamSynchronize(s);
            t0 = std::chrono::steady_clock::now();
        }
    }
    void lap(int stage) {
        if (!g_timing) return;
        (void)hipStreamSynchronize(s);
        const auto t1 = std::chrono::steady_clock::now();
        g_stage_ms[stage] += std::chrono::duration<float, std::milli>(t1 - t0).count();
        t0 = t1;
    }
};

#define SORT_OK(call) ((call) == hipSuccess)

// count_only: totals alone (no quadrics, placement, attributes or outputs)
int run(long long nv, long long nt, const float* vertices, const int* triangles, int nch, const float* attributes, const float* weights,
        double cell, void* ws, float* out_vertices, float* out_attributes, float* out_weight, int* out_triangles, int* vertex_map,
        long long* totals, bool count_only, hipStream_t s) {
    const SimplifyWs w = carve((char*)ws, nv, nt, nch);
    const SortBufs& b = w.sort;
    StageClock clock(s);

    // bounds, checks
    if (hipMemsetAsync(w.mm, 0xFF, 24, s) != hipSuccess || hipMemsetAsync(w.mm + 3, 0, 40, s) != hipSuccess ||
        hipMemsetAsync(w.lcount, 0, 8, s) != hipSuccess || hipMemsetAsync(w.err, 0, 16, s) != hipSuccess)
        return GS2M_ERR_HIP;
    const unsigned bgrid = blocks_of(nv) < 1024u ? blocks_of(nv) : 1024u;
    bounds_kernel<<<bgrid, 256, 0, s>>>(nv, vertices, cell, w.mm, w.err);
    check_triangles_kernel<<<blocks_of(nt), 256, 0, s>>>(nv, nt, triangles, w.err + 2);
    u64 mm[6];
    int err[4];
    if (gs2m_read_back(s, {{mm, w.mm, 48}, {err, w.err, 16}}) != GS2M_OK) return GS2M_ERR_HIP;
    if (err[0] || err[2]) return GS2M_ERR_INVALID_ARG;
    if (err[1]) return GS2M_ERR_UNSUPPORTED;
    Lattice L;
    L.cell = cell;
    int total_bits = 0;
    for (int k = 0; k < 3; k++) {
        const long long extent = (long long)(mm[3 + k] - mm[k]) + 1;
        if (extent > GS2M_SIMPLIFY_MAX_AXIS_CELLS) return GS2M_ERR_UNSUPPORTED;
        L.mn[k] = (long long)mm[k] - IDX_BIAS;
        L.bits[k] = bits_holding(extent - 1);
        total_bits += L.bits[k];
    }

    // keys + sorts -> cells
    key_kernel<<<blocks_of(nv), 256, 0, s>>>(nv, vertices, L, w.klo, w.khi);
    if (hipGetLastError() != hipSuccess ||
        !SORT_OK(gs2m_radix_sort_pairs(w.temp, w.temp_bytes, w.klo, nullptr, b.kA, b.vA, b.kB, b.vB, (size_t)nv,
                                       total_bits < 32 ? total_bits : 32, false, s)))
        return GS2M_ERR_HIP;
    if (total_bits > 32) {
        regather_kernel<<<blocks_of(nv), 256, 0, s>>>(nv, b.vB, w.khi, w.k2, w.v2);
        if (hipGetLastError() != hipSuccess ||
            !SORT_OK(gs2m_radix_sort_pairs(w.temp, w.temp_bytes, w.k2, w.v2, b.kA, b.vA, b.kB, b.vB, (size_t)nv, total_bits - 32, false, s)))
            return GS2M_ERR_HIP;
    }
    head_kernel<<<blocks_of(nv), 256, 0, s>>>(nv, b.vB, w.klo, w.khi, w.sidx, w.a);
    if (hipGetLastError() != hipSuccess || gs2m_scan_u64(w.a, nv, w.bsum, s) != hipSuccess) return GS2M_ERR_HIP;
    assign_kernel<<<blocks_of(nv), 256, 0, s>>>(nv, w.a, w.sidx, w.vcell, w.cstart);
    u64 ncells = 0;
    if (gs2m_read_back(s, {{&ncells, w.a + nv, 8}}) != GS2M_OK) return GS2M_ERR_HIP;
    const long long nc = (long long)ncells;
    const int cbits = bits_holding(nc);  // the keys 0 .. nc
    clock.lap(0);

    // triangle remap
    remap_kernel<<<blocks_of(nt), 256, 0, s>>>(nv, nt, (uint32_t)nc, triangles, w.vcell, w.ctri, count_only ? nullptr : w.ikey, w.tlo, w.tmid,
                                               w.thi, w.err + 2);
    if (hipGetLastError() != hipSuccess) return GS2M_ERR_HIP;
    clock.lap(3);

    CellBase cb;
    cb.L = L;
    cb.klo = w.klo;
    cb.khi = w.khi;
    cb.sidx = w.sidx;
    cb.cstart = w.cstart;
    const dim3 sgrid((unsigned)((nc * GROUP + 255) / 256), 1, 1);
    if (!count_only) {
        // quadrics
        const long long m = 3 * nt;
        if (!SORT_OK(gs2m_radix_sort_pairs(w.temp, w.temp_bytes, w.ikey, nullptr, b.kA, b.vA, b.kB, b.vB, (size_t)m, cbits, false, s)))
            return GS2M_ERR_HIP;
        QuadricSums qs;
        static_cast<CellBase&>(qs) = cb;
        qs.skey = b.kB;
        qs.slot = b.vB;
        qs.m = m;
        qs.v = vertices;
        qs.tris = triangles;
        qs.cq = w.cq;
        seg_short_kernel<9, QuadricSums><<<sgrid, 256, 0, s>>>(nc, qs, w.tlist, w.lcount + 1);
        seg_long_kernel<9, QuadricSums><<<LONG_BLOCKS, 256, 0, s>>>(qs, w.tlist, w.lcount + 1);
        if (hipGetLastError() != hipSuccess) return GS2M_ERR_HIP;
        clock.lap(1);

        // vertex means, attributes, placement
        VertexSums vs;
        static_cast<CellBase&>(vs) = cb;
        vs.v = vertices;
        vs.w = weights;
        vs.cq = w.cq;
        vs.wsum = w.wsum;
        seg_short_kernel<4, VertexSums><<<sgrid, 256, 0, s>>>(nc, vs, w.vlist, w.lcount);
        seg_long_kernel<4, VertexSums><<<LONG_BLOCKS, 256, 0, s>>>(vs, w.vlist, w.lcount);
        if (nch > 0) {
            AttributeSums as;
            static_cast<CellBase&>(as) = cb;
            as.attr = attributes;
            as.w = weights;
            as.wsum = w.wsum;
            as.cattr = w.cattr;
            as.nch = nch;
            seg_short_kernel<2, AttributeSums><<<dim3(sgrid.x, (unsigned)nch, 1), 256, 0, s>>>(nc, as, nullptr, nullptr);
            seg_long_kernel<2, AttributeSums><<<dim3(LONG_BLOCKS, (unsigned)nch, 1), 256, 0, s>>>(as, w.vlist, w.lcount);
        }
        place_kernel<<<blocks_of(nc), 256, 0, s>>>(nc, cb, w.cq, w.wsum, w.cellpos, w.cw);
        if (hipGetLastError() != hipSuccess) return GS2M_ERR_HIP;
        clock.lap(2);
    }

    // dedupe: sort by (lo, mid, hi), least significant first
    if (!SORT_OK(gs2m_radix_sort_pairs(w.temp, w.temp_bytes, w.thi, nullptr, b.kA, b.vA, b.kB, b.vB, (size_t)nt, cbits, false, s)))
        return GS2M_ERR_HIP;
    regather_kernel<<<blocks_of(nt), 256, 0, s>>>(nt, b.vB, w.tmid, w.k2, w.v2);
    if (hipGetLastError() != hipSuccess ||
        !SORT_OK(gs2m_radix_sort_pairs(w.temp, w.temp_bytes, w.k2, w.v2, b.kA, b.vA, b.kB, b.vB, (size_t)nt, cbits, false, s)))
        return GS2M_ERR_HIP;
    regather_kernel<<<blocks_of(nt), 256, 0, s>>>(nt, b.vB, w.tlo, w.k2, w.v2);
    if (hipGetLastError() != hipSuccess ||
        !SORT_OK(gs2m_radix_sort_pairs(w.temp, w.temp_bytes, w.k2, w.v2, b.kA, b.vA, b.kB, b.vB, (size_t)nt, cbits, false, s)))
        return GS2M_ERR_HIP;
    keep_heads_kernel<<<blocks_of(nt), 256, 0, s>>>(nt, (uint32_t)nc, b.kB, b.vB, w.tmid, w.thi, w.keep);
    if (hipGetLastError() != hipSuccess) return GS2M_ERR_HIP;
    clock.lap(3);

    if (count_only) {
        if (hipMemsetAsync(w.used, 0, (size_t)nc, s) != hipSuccess) return GS2M_ERR_HIP;
        mark_cells_kernel<<<blocks_of(nt), 256, 0, s>>>(nt, w.keep, w.ctri, w.used, w.mm + 6);
        count_used_kernel<<<blocks_of(nc), 256, 0, s>>>(nc, w.used, w.mm + 6);
        u64 cnt[2];
        if (gs2m_read_back(s, {{cnt, w.mm + 6, 16}}) != GS2M_OK) return GS2M_ERR_HIP;
        totals[0] = (long long)cnt[1];
        totals[1] = (long long)cnt[0];
        clock.lap(4);
        return GS2M_OK;
    }

    // compaction: gs2m_mesh_compact numbers the surviving cells in their order, which is the (ix, iy, iz) order
    const int rc = gs2m_mesh_compact(nc, nt, w.cellpos, nullptr, w.ctri, w.keep, w.compact, out_vertices, nullptr, out_triangles, totals, s);
    if (rc != GS2M_OK) return rc;
    const CompactWs cw = carve_compact((char*)w.compact, nc, nt);
    if (out_attributes || out_weight)
        gather_cells_kernel<<<blocks_of(nc), 256, 0, s>>>(nc, nch, cw.av, w.cattr, w.cw, nch > 0 ? out_attributes : nullptr, out_weight);
    if (vertex_map) vertex_map_kernel<<<blocks_of(nv), 256, 0, s>>>(nv, w.vcell, cw.av, vertex_map);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return GS2M_ERR_HIP;
    clock.lap(4);
    return GS2M_OK;
}

}  // namespace

extern "C" {

int gs2m_simplify_workspace_bytes(long long n_vertices, long long n_triangles, int n_channels, long long* bytes) {
    if (!bytes) return GS2M_ERR_INVALID_ARG;
    const int st = sizes_status(n_vertices, n_triangles, n_channels);
    if (st != GS2M_OK) return st;
    *bytes = (long long)carve(nullptr, n_vertices, n_triangles, n_channels).bytes;
    return GS2M_OK;
}

int gs2m_simplify_count(long long n_vertices, long long n_triangles, const float* vertices, const int* triangles, double cell, void* ws,
                        long long* totals, void* stream) {
    if (!totals || !(cell > 0.0) || !std::isfinite(cell)) return GS2M_ERR_INVALID_ARG;
    const int st = sizes_status(n_vertices, n_triangles, 0);
    if (st != GS2M_OK) return st;
    if (n_vertices > 0 && n_triangles > 0 && (!vertices || !triangles || !ws)) return GS2M_ERR_INVALID_ARG;
    totals[0] = totals[1] = 0;
    if (n_vertices == 0 || n_triangles == 0) return GS2M_OK;
    return run(n_vertices, n_triangles, vertices, triangles, 0, nullptr, nullptr, cell, ws, nullptr, nullptr, nullptr, nullptr, nullptr, totals,
               true, (hipStream_t)stream);
}

int gs2m_simplify(long long n_vertices, long long n_triangles, const float* vertices, const int* triangles, int n_channels,
                  const float* attributes, const float* weights, double cell, void* ws, float* out_vertices, float* out_attributes,
                  float* out_weight, int* out_triangles, int* vertex_map, long long* totals, void* stream) {
    if (!totals || !(cell > 0.0) || !std::isfinite(cell)) return GS2M_ERR_INVALID_ARG;
    const int st = sizes_status(n_vertices, n_triangles, n_channels);
    if (st != GS2M_OK) return st;
    const bool work = n_vertices > 0 && n_triangles > 0;
    if (work && (!vertices || !triangles || !ws || !out_vertices || !out_triangles || (n_channels > 0 && (!attributes || !out_attributes))))
        return GS2M_ERR_INVALID_ARG;
    totals[0] = totals[1] = 0;
    if (!work) return GS2M_OK;  // no triangle: no cell survives, nothing is launched or written
    return run(n_vertices, n_triangles, vertices, triangles, n_channels, attributes, weights, cell, ws, out_vertices, out_attributes, out_weight,
               out_triangles, vertex_map, totals, false, (hipStream_t)stream);
}

int gs2m_simplify_set_timing(int on) {
    g_timing = on != 0;
    return GS2M_OK;
}

int gs2m_simplify_stage_ms(float* ms) {
    if (!ms) return GS2M_ERR_INVALID_ARG;
    for (int k = 0; k < 5; k++) ms[k] = g_stage_ms[k];
    return GS2M_OK;
}

}  // extern "C"
