// DTU mesh evaluation: sampling, thinning, observation-mask filter and capped nearest-neighbour distances
// (include/gs2m_eval.h; the contract: DESIGN.md §10).
//
// Sampling (count / scan / emit, three levels so that a triangle of 10^5 samples is spread over many threads):
//   tri_rows_kernel      per triangle: n1, n2 and its rows that can hold samples (i < n1)
//   row_count_kernel     per row: the kept candidates of the row (k0 + k1 is monotone in j: a binary search)
//   emit_kernel          per sample: its row and triangle by binary searches over the two scans, then the point
// Spatial index: a hashed uniform grid.  The cell (floor(p / cell) per axis) hashes to a bucket of 2^bits; the buckets sort
// with the project's radix sort (gs2m_radix_sort_pairs) and a bucket-start table is filled from the sorted keys.  A coarse
// occupancy table (cells of 8^3 fine cells, same hash) bounds the nearest-neighbour walk.  Hash collisions only add candidates;
// every candidate passes the exact distance test.
// Thinning: rounds of the rank-priority rule over the grid-sorted points (thin_round_kernel); a point decides once every
// neighbour of lower rank has decided, so the result is the sequential greedy set whatever the rounds' timing.
// Nearest: shells of cells walked outward from the query's cell until the shell's lower bound passes the best distance or
// max_dist; the first occupied coarse shell sets where the walk starts, or proves that nothing lies within max_dist.
// Every sum is an integer sum or a fixed-order fp64 reduction: two runs are bitwise identical.  Compiled with -ffp-contract=off.
#include <math.h>
#include "eval_common.h"
#include "../../include/gs2m_eval.h"

namespace {

constexpr int TILE = 1024;           // scan: entries per workgroup (256 threads x 4)
constexpr int COARSE_SHIFT = 3;      // coarse cell = 8^3 fine cells
constexpr int COARSE_SHELLS_MAX = 24;

// ---- device-wide exclusive scan of u64 counts (in place; a[n] = total): gs2m_scan_u64 of eval_common.h ----

__global__ void __launch_bounds__(256) scan_reduce_kernel(long long n, const u64* __restrict__ a, u64* __restrict__ bsum) {
    __shared__ u64 s_w[4];
    const long long i0 = (long long)blockIdx.x * TILE + 4 * threadIdx.x;
    u64 v = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) v += i0 + k < n ? a[i0 + k] : 0ull;
    u64 tot;
    gs2m_wg_exclusive_scan(v, s_w, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(256) scan_blocks_kernel(long long nb, u64* __restrict__ bsum, u64* __restrict__ total) {
    __shared__ u64 s_w[4];
    u64 carry = 0;
    for (long long b = 0; b < nb; b += 256) {
        const long long i = b + threadIdx.x;
        const u64 v = i < nb ? bsum[i] : 0ull;
        u64 t;
        const u64 e = gs2m_wg_exclusive_scan(v, s_w, &t);
        if (i < nb) bsum[i] = carry + e;
        carry += t;
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ void __launch_bounds__(256) scan_down_kernel(long long n, u64* a, const u64* __restrict__ bsum) {
    __shared__ u64 s_w[4];
    const long long i0 = (long long)blockIdx.x * TILE + 4 * threadIdx.x;
    u64 v[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        v[k] = i0 + k < n ? a[i0 + k] : 0ull;
        s += v[k];
    }
    u64 tot;
    u64 e = gs2m_wg_exclusive_scan(s, s_w, &tot) + bsum[blockIdx.x];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (i0 + k < n) a[i0 + k] = e;
        e += v[k];
    }
}

}  // namespace

long long gs2m_scan_blocks(long long n) { return (n + TILE - 1) / TILE; }

hipError_t gs2m_scan_u64(u64* a, long long n, u64* bsum, hipStream_t s) {
    const long long nb = gs2m_scan_blocks(n);
    if (nb == 0) return hipMemsetAsync(a, 0, sizeof(u64), s);
    scan_reduce_kernel<<<(unsigned)nb, 256, 0, s>>>(n, a, bsum);
    scan_blocks_kernel<<<1, 256, 0, s>>>(nb, bsum, a + n);
    scan_down_kernel<<<(unsigned)nb, 256, 0, s>>>(n, a, bsum);
    return hipGetLastError();
}

namespace {

// the last index k in [0, m) with a[k] <= x (a non-decreasing, a[0] <= x)
__device__ __forceinline__ long long last_le(const u64* __restrict__ a, long long m, u64 x) {
    long long lo = 0, hi = m;  // a[lo] <= x, answer in [lo, hi)
    while (hi - lo > 1) {
        const long long mid = lo + (hi - lo) / 2;
        if (a[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---- sampling ----

struct TriGeom {
    double p0[3], v1[3], v2[3];
};

__device__ __forceinline__ double norm3(const double v[3]) { return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }

__device__ __forceinline__ void tri_geom(const double* __restrict__ verts, int a, int b, int c, TriGeom& g) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        g.p0[k] = verts[3 * (size_t)a + k];
        g.v1[k] = verts[3 * (size_t)b + k] - g.p0[k];
        g.v2[k] = verts[3 * (size_t)c + k] - g.p0[k];
    }
}

__global__ void __launch_bounds__(256) tri_rows_kernel(long long nv, const double* __restrict__ verts, long long nt,
                                                       const int* __restrict__ tris, double thresh, double2* __restrict__ n12,
                                                       u64* __restrict__ rows, int* __restrict__ err) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const int a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
    if (!tri_in_range(a, b, c, nv, err)) {
        n12[t] = make_double2(0.0, 0.0);
        rows[t] = 0;
        return;
    }
    TriGeom g;
    tri_geom(verts, a, b, c, g);
    const double l1 = norm3(g.v1), l2 = norm3(g.v2);
    const double cr[3] = {g.v1[1] * g.v2[2] - g.v1[2] * g.v2[1], g.v1[2] * g.v2[0] - g.v1[0] * g.v2[2],
                          g.v1[0] * g.v2[1] - g.v1[1] * g.v2[0]};
    const double area2 = norm3(cr);
    double n1 = 0.0, n2 = 0.0;
    u64 r = 0;
    if (area2 > 0.0) {
        const double thr = thresh * sqrt((l1 * l2) / area2);
        n1 = floor(l1 / thr);
        n2 = floor(l2 / thr);
        // i = n1 gives k0 > 1: the rows that can hold a sample are i < n1; n1 == 0 or n2 == 0 (or NaN) gives none
        if (n1 >= 1.0 && n2 >= 1.0) {
            if (n1 > 2147483647.0 || n2 > 2147483647.0) err[1] = 1;
            else r = (u64)n1;
        }
    }
    n12[t] = make_double2(n1, n2);
    rows[t] = r;
}

__device__ __forceinline__ double k_of(double i, double n) { return (i + 0.5) / fmax(n, 1e-7); }

__global__ void __launch_bounds__(256) row_count_kernel(long long nt, long long nr, const u64* __restrict__ row_base,
                                                        const double2* __restrict__ n12, u64* __restrict__ cnt) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= nr) return;
    const long long t = last_le(row_base, nt + 1, (u64)r);
    const double2 n = n12[t];
    const double k0 = k_of((double)(r - (long long)row_base[t]), n.x);
    // candidates j = 0..n2; k0 + k1(j) < 1 holds on a prefix of them
    long long lo = 0, hi = (long long)n.y + 1;  // answer in [lo, hi]
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (k0 + k_of((double)mid, n.y) < 1.0) lo = mid + 1;
        else hi = mid;
    }
    cnt[r] = (u64)lo;
}

__global__ void __launch_bounds__(256) emit_kernel(long long nv, const double* __restrict__ verts, long long nt,
                                                   const int* __restrict__ tris, const double2* __restrict__ n12,
                                                   const u64* __restrict__ row_base, long long nr, const u64* __restrict__ sample_base,
                                                   long long ns, double* __restrict__ cloud) {
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= ns) return;
    const long long r = last_le(sample_base, nr + 1, (u64)s);
    const long long t = last_le(row_base, nt + 1, (u64)r);
    const double2 n = n12[t];
    const double k0 = k_of((double)(r - (long long)row_base[t]), n.x);
    const double k1 = k_of((double)(s - (long long)sample_base[r]), n.y);
    TriGeom g;
    tri_geom(verts, tris[3 * t], tris[3 * t + 1], tris[3 * t + 2], g);
    double* o = cloud + 3 * (size_t)(nv + s);
#pragma unroll
    for (int k = 0; k < 3; k++) o[k] = (g.v1[k] * k0 + g.v2[k] * k1) + g.p0[k];
}

struct TriWs {
    double2* n12;  // nt
    u64* rows;     // nt + 1: rows per triangle, then their exclusive prefixes
    u64* bsum;     // scan_blocks(nt) + 1
    int* err;      // 2: [0] vertex index out of range, [1] n1 or n2 beyond 2^31
    size_t bytes;
};
TriWs carve_tri(char* base, long long nt) {
    Carver c{base, 0};
    TriWs w;
    w.n12 = c.take<double2>(nt);
    w.rows = c.take<u64>(nt + 1);
    w.bsum = c.take<u64>(gs2m_scan_blocks(nt) + 1);
    w.err = c.take<int>(2);
    w.bytes = c.off;
    return w;
}
struct RowWs {
    u64* cnt;   // nr + 1: samples per row, then their exclusive prefixes
    u64* bsum;  // scan_blocks(nr) + 1
    size_t bytes;
};
RowWs carve_row(char* base, long long nr) {
    Carver c{base, 0};
    RowWs w;
    w.cnt = c.take<u64>(nr + 1);
    w.bsum = c.take<u64>(gs2m_scan_blocks(nr) + 1);
    w.bytes = c.off;
    return w;
}

// ---- hashed uniform grid (its layout and hash: eval_common.h) ----

struct BuildWs {
    uint32_t* keys;  // max(n, 1), as the sort's arrays
    SortBufs sort;
    void* temp;
    size_t temp_bytes, bytes;
};
BuildWs carve_build(char* base, long long n, int bits) {
    Carver c{base, 0};
    BuildWs w;
    const size_t m = (size_t)(n > 0 ? n : 1);
    w.keys = c.take<uint32_t>(m);
    w.sort = take_sort_bufs(c, m);
    w.temp_bytes = gs2m_radix_temp_bytes(m, bits);
    w.temp = c.take<char>(w.temp_bytes);
    w.bytes = c.off;
    return w;
}

__global__ void __launch_bounds__(256) grid_key_kernel(long long n, const double* __restrict__ pts, double inv, uint32_t mask,
                                                       uint32_t* __restrict__ keys, uint8_t* __restrict__ occ) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = cell_coord(pts[3 * i], inv), y = cell_coord(pts[3 * i + 1], inv), z = cell_coord(pts[3 * i + 2], inv);
    keys[i] = hash3(x, y, z, mask);
    occ[hash3(x >> COARSE_SHIFT, y >> COARSE_SHIFT, z >> COARSE_SHIFT, mask)] = 1;
}

// slot j in [0, n]: the sorted point j, and the starts of the buckets (key[j - 1], key[j]]
__global__ void __launch_bounds__(256) grid_place_kernel(long long n, const double* __restrict__ pts, const uint32_t* __restrict__ kB,
                                                         const uint32_t* __restrict__ vB, long long nbuckets, double* __restrict__ spts,
                                                         uint32_t* __restrict__ sidx, uint32_t* __restrict__ start) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j > n) return;
    if (j < n) {
        const uint32_t i = vB[j];
        sidx[j] = i;
#pragma unroll
        for (int k = 0; k < 3; k++) spts[3 * j + k] = pts[3 * (size_t)i + k];
    }
    const long long prev = j == 0 ? -1 : (long long)kB[j - 1];
    const long long cur = j == n ? nbuckets : (long long)kB[j];
    for (long long b = prev + 1; b <= cur; b++) start[b] = (uint32_t)j;
}

hipError_t build_grid(long long n, const double* pts, double cell, const Grid& g, const BuildWs& w, hipStream_t s) {
    const long long nb = 1ll << g.bits;
    const uint32_t mask = (uint32_t)(nb - 1);
    hipError_t e = hipMemsetAsync(g.occ, 0, (size_t)nb, s);
    if (e != hipSuccess) return e;
    if (n > 0) {
        grid_key_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(n, pts, 1.0 / cell, mask, w.keys, g.occ);
        e = gs2m_radix_sort_pairs(w.temp, w.temp_bytes, w.keys, nullptr, w.sort.kA, w.sort.vA, w.sort.kB, w.sort.vB, (size_t)n, g.bits,
                                  false, s);
        if (e != hipSuccess) return e;
    }
    grid_place_kernel<<<(unsigned)((n + 1 + 255) / 256), 256, 0, s>>>(n, pts, w.sort.kB, w.sort.vB, nb, g.spts, g.sidx, g.start);
    return hipGetLastError();
}

__device__ __forceinline__ double dist2(const double* __restrict__ p, const double q[3]) {
    const double dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// ---- thinning ----

__global__ void __launch_bounds__(256) thin_init_kernel(long long n, const uint32_t* __restrict__ sidx, const unsigned* __restrict__ rank,
                                                        uint32_t* __restrict__ rank_s, uint8_t* __restrict__ st) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    rank_s[j] = rank ? rank[sidx[j]] : sidx[j];
    st[j] = 0;
}

// st: 0 undecided, 1 kept, 2 removed, per sorted slot.  Decisions only read decided neighbours' final states, so they do not
// depend on which of this round's writes a thread sees.
__global__ void __launch_bounds__(256) thin_round_kernel(long long n, double inv, uint32_t mask, const double* __restrict__ spts,
                                                         const uint32_t* __restrict__ start, const uint32_t* __restrict__ rank_s,
                                                         double r2, uint8_t* st, unsigned* undecided) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n || st[j] != 0) return;
    const double q[3] = {spts[3 * j], spts[3 * j + 1], spts[3 * j + 2]};
    const uint32_t rj = rank_s[j];
    const int cx = cell_coord(q[0], inv), cy = cell_coord(q[1], inv), cz = cell_coord(q[2], inv);
    bool blocked = false, removed = false;
    for (int dz = -1; dz <= 1 && !removed; dz++)
        for (int dy = -1; dy <= 1 && !removed; dy++)
            for (int dx = -1; dx <= 1 && !removed; dx++) {
                const uint32_t b = hash3(cx + dx, cy + dy, cz + dz, mask);
                const uint32_t e = start[b + 1];
                for (uint32_t k = start[b]; k < e; k++) {
                    if (k == (uint32_t)j || rank_s[k] >= rj) continue;
                    if (dist2(spts + 3 * (size_t)k, q) <= r2) {
                        const uint8_t sk = st[k];
                        if (sk == 1) {
                            removed = true;
                            break;
                        }
                        if (sk == 0) blocked = true;
                    }
                }
            }
    if (removed) st[j] = 2;
    else if (!blocked) st[j] = 1;
    else if (undecided) atomicAdd(undecided, 1u);
}

__global__ void __launch_bounds__(256) thin_keep_kernel(long long n, const uint32_t* __restrict__ sidx, const uint8_t* __restrict__ st,
                                                        unsigned char* __restrict__ keep) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    keep[sidx[j]] = st[j] == 1 ? 1 : 0;
}

// ---- nearest neighbour ----

// visits the cells at Chebyshev distance exactly s from (cx, cy, cz); f(bucket) per cell
template <class F>
__device__ __forceinline__ bool shell_any(int cx, int cy, int cz, int s, uint32_t mask, F f) {
    for (int dz = -s; dz <= s; dz++)
        for (int dy = -s; dy <= s; dy++) {
            const bool face = dz == -s || dz == s || dy == -s || dy == s;
            const int step = face || s == 0 ? 1 : 2 * s;
            for (int dx = -s; dx <= s; dx += step)
                if (f(hash3(cx + dx, cy + dy, cz + dz, mask))) return true;
        }
    return false;
}

// IDX: also the nearest point's index in the targets' given order (sidx), ties to the lowest index; -1 where dist is +inf.
// The distances are the same with and without: the minimum over the same candidates.
template <bool IDX>
__global__ void __launch_bounds__(256) nearest_kernel(long long nq, const double* __restrict__ queries, long long n, double cell,
                                                      double inv, uint32_t mask, const double* __restrict__ spts,
                                                      const uint32_t* __restrict__ sidx, const uint32_t* __restrict__ start,
                                                      const uint8_t* __restrict__ occ, double max_dist, int fine_shells,
                                                      int coarse_shells, long long* __restrict__ index, double* __restrict__ dist) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    const double q[3] = {queries[3 * i], queries[3 * i + 1], queries[3 * i + 2]};
    const double INF = __builtin_huge_val();
    if (IDX) index[i] = -1;
    if (n == 0) {
        dist[i] = INF;
        return;
    }
    const int cx = cell_coord(q[0], inv), cy = cell_coord(q[1], inv), cz = cell_coord(q[2], inv);
    const double qmax = fmax(fabs(q[0]), fmax(fabs(q[1]), fabs(q[2])));
    // cell assignment is exact up to the rounding of x / cell: a margin for the shells' lower bounds
    const double eps = 1e-6 * cell + 1e-13 * (qmax + max_dist);
    int s0 = 0;
    if (coarse_shells > 0) {
        const int ax = cx >> COARSE_SHIFT, ay = cy >> COARSE_SHIFT, az = cz >> COARSE_SHIFT;
        int first = -1;
        for (int s = 0; s <= coarse_shells && first < 0; s++)
            if (shell_any(ax, ay, az, s, mask, [&](uint32_t b) { return occ[b] != 0; })) first = s;
        // every point lies in a coarse cell >= `first` cells away: its separation on some axis is >= (first - 1) * 8 cell
        const double lb = (double)(first - 1) * (double)(1 << COARSE_SHIFT) * cell - eps;
        if (first < 0 || lb >= max_dist) {
            dist[i] = INF;
            return;
        }
        s0 = first >= 1 ? ((first - 1) << COARSE_SHIFT) - 2 : 0;
        if (s0 < 0) s0 = 0;
    }
    double best = INF;
    uint32_t best_i = 0xFFFFFFFFu;
    for (int s = s0; s <= fine_shells; s++) {
        shell_any(cx, cy, cz, s, mask, [&](uint32_t b) {
            const uint32_t e = start[b + 1];
            for (uint32_t k = start[b]; k < e; k++) {
                const double d2 = dist2(spts + 3 * (size_t)k, q);
                if (IDX) {
                    // a tie lies at the same distance, so inside the shells walked before the walk may stop
                    if (d2 < best || (d2 == best && sidx[k] < best_i)) {
                        best = d2;
                        best_i = sidx[k];
                    }
                } else {
                    best = fmin(best, d2);
                }
            }
            return false;
        });
        // points beyond shell s are >= s cells away on some axis
        const double lb = (double)s * cell - eps;
        if (lb >= max_dist || (lb > 0.0 && best <= lb * lb)) break;
    }
    const double d = sqrt(best);
    dist[i] = d < max_dist ? d : INF;
    if (IDX && d < max_dist) index[i] = (long long)best_i;
}

// ---- filters, compaction, mean ----

__global__ void __launch_bounds__(256) filter_kernel(long long n, const double* __restrict__ pts, V3 lo, V3 hi, V3 bb0, double res,
                                                     const unsigned char* __restrict__ mask, int X, int Y, int Z,
                                                     unsigned char* __restrict__ flags) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    bool inb = true;
#pragma unroll
    for (int k = 0; k < 3; k++) inb = inb && p[k] >= lo.v[k] && p[k] < hi.v[k];
    bool obs = false;
    if (inb) {
        const int dims[3] = {X, Y, Z};
        long long g[3];
        bool in = true;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double r = rint((p[k] - bb0.v[k]) / res);  // round half to even
            in = in && r >= 0.0 && r < (double)dims[k];
            g[k] = in ? (long long)r : 0;
        }
        obs = in && mask[(g[0] * Y + g[1]) * Z + g[2]] != 0;
    }
    flags[i] = (inb ? 1 : 0) | (obs ? 2 : 0);
}

__global__ void __launch_bounds__(256) plane_kernel(long long n, const double* __restrict__ pts, double P0, double P1, double P2,
                                                    double P3, unsigned char* __restrict__ flags) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    flags[i] = ((P0 * pts[3 * i] + P1 * pts[3 * i + 1]) + P2 * pts[3 * i + 2]) + P3 > 0.0 ? 1 : 0;
}

__global__ void __launch_bounds__(256) flag_count_kernel(long long n, const unsigned char* __restrict__ flags, int bit, u64* __restrict__ a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] = (flags[i] >> bit) & 1;
}

__global__ void __launch_bounds__(256) compact_kernel(long long n, const double* __restrict__ pts, const unsigned char* __restrict__ flags,
                                                      int bit, const u64* __restrict__ a, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !((flags[i] >> bit) & 1)) return;
    const u64 o = a[i];
#pragma unroll
    for (int k = 0; k < 3; k++) out[3 * o + k] = pts[3 * i + k];
}

__global__ void __launch_bounds__(256) gather_kernel(long long n, const double* __restrict__ pts, const long long* __restrict__ order,
                                                     double* __restrict__ out) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const long long o = order[q];
    const bool ok = o >= 0 && o < n;
#pragma unroll
    for (int k = 0; k < 3; k++) out[3 * q + k] = ok ? pts[3 * o + k] : __builtin_nan("");
}

__global__ void __launch_bounds__(256) transform_kernel(long long n, const double* in, double scale, V3 t, double* out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int k = 0; k < 3; k++) out[3 * i + k] = in[3 * i + k] * scale + t.v[k];
}

// the masked mean's term of the fixed-order reduction (eval_common.h): the distances below max_dist and their count
struct MeanTerm {
    const double* d;
    double max_dist;
    __device__ void operator()(long long i, double* acc, u64& c) const {
        const double x = d[i];
        if (x < max_dist) {
            acc[0] += x;
            c++;
        }
    }
};

// the mean's partials first: their place does not depend on n, so any scan workspace (n >= 0) serves the mean
struct ScanWs {
    double* psum;  // RED_BLOCKS + 1 (the last: the total)
    u64* pcnt;     // RED_BLOCKS + 1
    u64* a;        // n + 1
    u64* bsum;     // scan_blocks(n) + 1
    size_t bytes;
};
ScanWs carve_scan(char* base, long long n) {
    Carver c{base, 0};
    ScanWs w;
    w.psum = c.take<double>(RED_BLOCKS + 1);
    w.pcnt = c.take<u64>(RED_BLOCKS + 1);
    w.a = c.take<u64>(n + 1);
    w.bsum = c.take<u64>(gs2m_scan_blocks(n) + 1);
    w.bytes = c.off;
    return w;
}

struct ThinWs {
    Grid g;
    BuildWs b;
    uint32_t* rank_s;
    uint8_t* st;
    unsigned* counter;
    size_t bytes;
};
ThinWs carve_thin(char* base, long long n) {
    ThinWs w;
    w.g = carve_grid(base, n);
    w.b = carve_build(base + w.g.bytes, n, w.g.bits);
    Carver c{base, w.g.bytes + w.b.bytes};
    w.rank_s = c.take<uint32_t>(n);
    w.st = c.take<uint8_t>(n);
    w.counter = c.take<unsigned>(1);
    w.bytes = c.off;
    return w;
}

int nearest(long long n_queries, const double* queries, long long n_targets, double cell, const void* grid, double max_dist,
            long long* index, double* dist, bool with_index, void* stream) {
    if (n_queries < 0 || n_targets < 0 || !(cell > 0.0) || !(max_dist > 0.0) || !grid || (n_queries > 0 && (!queries || !dist)))
        return GS2M_ERR_INVALID_ARG;
    if (n_targets > MAX_POINTS || n_queries > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    if (n_queries == 0) return GS2M_OK;
    const Grid g = carve_grid((char*)const_cast<void*>(grid), n_targets);
    const double fs = ceil(max_dist / cell) + 1.0;
    if (!(fs < 1e6)) return GS2M_ERR_UNSUPPORTED;  // cell far too small for max_dist
    const double cs = ceil(max_dist / (cell * (1 << COARSE_SHIFT))) + 1.0;
    const int coarse = cs <= COARSE_SHELLS_MAX ? (int)cs : 0;  // 0: no coarse bound (the fine walk alone is still exact)
    const uint32_t mask = (uint32_t)((1ll << g.bits) - 1);
    hipStream_t s = (hipStream_t)stream;
    if (with_index)
        nearest_kernel<true><<<blocks_of(n_queries), 256, 0, s>>>(n_queries, queries, n_targets, cell, 1.0 / cell, mask, g.spts, g.sidx,
                                                                  g.start, g.occ, max_dist, (int)fs, coarse, index, dist);
    else
        nearest_kernel<false><<<blocks_of(n_queries), 256, 0, s>>>(n_queries, queries, n_targets, cell, 1.0 / cell, mask, g.spts, g.sidx,
                                                                   g.start, g.occ, max_dist, (int)fs, coarse, nullptr, dist);
    return gs2m_status(hipGetLastError());
}

}  // namespace

extern "C" {

int gs2m_eval_transform(long long n, const double* in, double scale, const double* t, double* out, void* stream) {
    if (n < 0 || !t || (n > 0 && (!in || !out))) return GS2M_ERR_INVALID_ARG;
    if (n == 0) return GS2M_OK;
    if (n > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    transform_kernel<<<blocks_of(n), 256, 0, (hipStream_t)stream>>>(n, in, scale, V3{{t[0], t[1], t[2]}}, out);
    return gs2m_status(hipGetLastError());
}

int gs2m_eval_sample_workspace_bytes(long long n_tris, long long n_rows, long long* tri_bytes, long long* row_bytes) {
    if (n_tris < 0 || n_rows < 0) return GS2M_ERR_INVALID_ARG;
    if (tri_bytes) *tri_bytes = (long long)carve_tri(nullptr, n_tris).bytes;
    if (row_bytes) *row_bytes = (long long)carve_row(nullptr, n_rows).bytes;
    return GS2M_OK;
}

int gs2m_eval_sample_rows(long long n_verts, const double* verts, long long n_tris, const int* tris, double thresh, void* tri_ws,
                          long long* host_rows, void* stream) {
    if (n_verts < 0 || n_tris < 0 || !host_rows || !tri_ws || !(thresh > 0.0) || (n_tris > 0 && (!verts || !tris)))
        return GS2M_ERR_INVALID_ARG;
    if (n_tris > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const TriWs w = carve_tri((char*)tri_ws, n_tris);
    if (hipMemsetAsync(w.err, 0, 8, s) != hipSuccess) return GS2M_ERR_HIP;
    if (n_tris > 0)
        tri_rows_kernel<<<blocks_of(n_tris), 256, 0, s>>>(n_verts, verts, n_tris, tris, thresh, w.n12, w.rows, w.err);
    if (hipGetLastError() != hipSuccess || gs2m_scan_u64(w.rows, n_tris, w.bsum, s) != hipSuccess) return GS2M_ERR_HIP;
    int err[2];
    u64 total;
    if (gs2m_read_back(s, {{err, w.err, sizeof(err)}, {&total, w.rows + n_tris, sizeof(total)}}) != GS2M_OK) return GS2M_ERR_HIP;
    if (err[0]) return GS2M_ERR_INVALID_ARG;
    if (err[1] || total > (u64)MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    *host_rows = (long long)total;
    return GS2M_OK;
}

int gs2m_eval_sample_count(long long n_tris, long long n_rows, const void* tri_ws, void* row_ws, long long* host_samples,
                           void* stream) {
    if (n_tris < 0 || n_rows < 0 || !tri_ws || !row_ws || !host_samples) return GS2M_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    const TriWs tw = carve_tri((char*)tri_ws, n_tris);
    const RowWs rw = carve_row((char*)row_ws, n_rows);
    if (n_rows > 0) row_count_kernel<<<blocks_of(n_rows), 256, 0, s>>>(n_tris, n_rows, tw.rows, tw.n12, rw.cnt);
    if (hipGetLastError() != hipSuccess || gs2m_scan_u64(rw.cnt, n_rows, rw.bsum, s) != hipSuccess) return GS2M_ERR_HIP;
    u64 total;
    if (gs2m_read_back(s, {{&total, rw.cnt + n_rows, sizeof(total)}}) != GS2M_OK) return GS2M_ERR_HIP;
    if (total > (u64)MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    *host_samples = (long long)total;
    return GS2M_OK;
}

int gs2m_eval_sample_emit(long long n_verts, const double* verts, long long n_tris, const int* tris, long long n_rows,
                          const void* tri_ws, const void* row_ws, long long n_samples, double* cloud, void* stream) {
    if (n_verts < 0 || n_tris < 0 || n_rows < 0 || n_samples < 0 || !tri_ws || !row_ws || (n_verts + n_samples > 0 && !cloud) ||
        (n_verts > 0 && !verts) || (n_samples > 0 && !tris))
        return GS2M_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (n_verts > 0 && hipMemcpyAsync(cloud, verts, 24 * (size_t)n_verts, hipMemcpyDeviceToDevice, s) != hipSuccess) return GS2M_ERR_HIP;
    const TriWs tw = carve_tri((char*)tri_ws, n_tris);
    const RowWs rw = carve_row((char*)row_ws, n_rows);
    if (n_samples > 0)
        emit_kernel<<<blocks_of(n_samples), 256, 0, s>>>(n_verts, verts, n_tris, tris, tw.n12, tw.rows, n_rows, rw.cnt, n_samples, cloud);
    return gs2m_status(hipGetLastError());
}

int gs2m_eval_gather(long long n, const double* pts, const long long* order, double* out, void* stream) {
    if (n < 0 || (n > 0 && (!pts || !order || !out))) return GS2M_ERR_INVALID_ARG;
    if (n == 0) return GS2M_OK;
    if (n > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    gather_kernel<<<blocks_of(n), 256, 0, (hipStream_t)stream>>>(n, pts, order, out);
    return gs2m_status(hipGetLastError());
}

int gs2m_eval_grid_bytes(long long n, long long* grid_bytes, long long* build_bytes) {
    if (n < 0) return GS2M_ERR_INVALID_ARG;
    if (n > MAX_POINTS) return GS2M_ERR_UNSUPPORTED;
    const Grid g = carve_grid(nullptr, n);
    if (grid_bytes) *grid_bytes = (long long)g.bytes;
    if (build_bytes) *build_bytes = (long long)carve_build(nullptr, n, g.bits).bytes;
    return GS2M_OK;
}

int gs2m_eval_grid_build(long long n, const double* pts, double cell, void* grid, void* build_ws, void* stream) {
    if (n < 0 || !(cell > 0.0) || !grid || !build_ws || (n > 0 && !pts)) return GS2M_ERR_INVALID_ARG;
    if (n > MAX_POINTS) return GS2M_ERR_UNSUPPORTED;
    const Grid g = carve_grid((char*)grid, n);
    return gs2m_status(build_grid(n, pts, cell, g, carve_build((char*)build_ws, n, g.bits), (hipStream_t)stream));
}

int gs2m_eval_thin_workspace_bytes(long long n, long long* bytes) {
    if (n < 0 || !bytes) return GS2M_ERR_INVALID_ARG;
    if (n > MAX_POINTS) return GS2M_ERR_UNSUPPORTED;
    *bytes = (long long)carve_thin(nullptr, n).bytes;
    return GS2M_OK;
}

int gs2m_eval_thin(long long n, const double* pts, const unsigned* rank, double radius, void* ws, unsigned char* keep,
                   int* host_rounds, void* stream) {
    if (n < 0 || !(radius > 0.0) || !ws || (n > 0 && (!pts || !keep))) return GS2M_ERR_INVALID_ARG;
    if (n > MAX_POINTS) return GS2M_ERR_UNSUPPORTED;
    if (host_rounds) *host_rounds = 0;
    if (n == 0) return GS2M_OK;
    hipStream_t s = (hipStream_t)stream;
    const ThinWs w = carve_thin((char*)ws, n);
    // a cell a little wider than the radius: neighbours within the radius lie in the 27 cells around whatever the rounding of x / cell
    const double cell = radius * (1.0 + 1.0 / (1 << 20));
    if (build_grid(n, pts, cell, w.g, w.b, s) != hipSuccess) return GS2M_ERR_HIP;
    thin_init_kernel<<<blocks_of(n), 256, 0, s>>>(n, w.g.sidx, rank, w.rank_s, w.st);
    if (hipGetLastError() != hipSuccess) return GS2M_ERR_HIP;
    const uint32_t mask = (uint32_t)((1ll << w.g.bits) - 1);
    const double inv = 1.0 / cell, r2 = radius * radius;
    // every round decides at least the undecided point of lowest rank: at most n rounds.  The host reads the undecided count
    // after every BATCH rounds only.
    const int BATCH = 8;
    long long rounds = 0;
    for (;;) {
        for (int k = 0; k < BATCH - 1; k++)
            thin_round_kernel<<<blocks_of(n), 256, 0, s>>>(n, inv, mask, w.g.spts, w.g.start, w.rank_s, r2, w.st, nullptr);
        if (hipMemsetAsync(w.counter, 0, 4, s) != hipSuccess) return GS2M_ERR_HIP;
        thin_round_kernel<<<blocks_of(n), 256, 0, s>>>(n, inv, mask, w.g.spts, w.g.start, w.rank_s, r2, w.st, w.counter);
        rounds += BATCH;
        unsigned left = 0;
        if (gs2m_read_back(s, {{&left, w.counter, 4}}) != GS2M_OK) return GS2M_ERR_HIP;
        if (left == 0) break;
        if (rounds > n + BATCH) return GS2M_ERR_HIP;  // cannot happen: see above
    }
    if (host_rounds) *host_rounds = (int)(rounds < 0x7FFFFFFF ? rounds : 0x7FFFFFFF);
    thin_keep_kernel<<<blocks_of(n), 256, 0, s>>>(n, w.g.sidx, w.st, keep);
    return gs2m_status(hipGetLastError());
}

int gs2m_eval_filter(long long n, const double* pts, const double* lo, const double* hi, const double* bb0, double res,
                     const unsigned char* mask, const int* dims, unsigned char* flags, void* stream) {
    if (n < 0 || !lo || !hi || !bb0 || !dims || !(res > 0.0) || dims[0] < 0 || dims[1] < 0 || dims[2] < 0 ||
        (n > 0 && (!pts || !flags)) || (!mask && (long long)dims[0] * dims[1] * dims[2] > 0))
        return GS2M_ERR_INVALID_ARG;
    if (n == 0) return GS2M_OK;
    if (n > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    filter_kernel<<<blocks_of(n), 256, 0, (hipStream_t)stream>>>(n, pts, V3{{lo[0], lo[1], lo[2]}}, V3{{hi[0], hi[1], hi[2]}},
                                                                 V3{{bb0[0], bb0[1], bb0[2]}}, res, mask, dims[0], dims[1], dims[2],
                                                                 flags);
    return gs2m_status(hipGetLastError());
}

int gs2m_eval_above_plane(long long n, const double* pts, const double* plane, unsigned char* flags, void* stream) {
    if (n < 0 || !plane || (n > 0 && (!pts || !flags))) return GS2M_ERR_INVALID_ARG;
    if (n == 0) return GS2M_OK;
    if (n > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    plane_kernel<<<blocks_of(n), 256, 0, (hipStream_t)stream>>>(n, pts, plane[0], plane[1], plane[2], plane[3], flags);
    return gs2m_status(hipGetLastError());
}

int gs2m_eval_scan_workspace_bytes(long long n, long long* bytes) {
    if (n < 0 || !bytes) return GS2M_ERR_INVALID_ARG;
    *bytes = (long long)carve_scan(nullptr, n).bytes;
    return GS2M_OK;
}

int gs2m_eval_compact(long long n, const double* pts, const unsigned char* flags, int bit, void* ws, double* out,
                      long long* host_count, void* stream) {
    if (n < 0 || bit < 0 || bit > 7 || !ws || !host_count || (n > 0 && (!pts || !flags || !out))) return GS2M_ERR_INVALID_ARG;
    if (n > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const ScanWs w = carve_scan((char*)ws, n);
    if (n > 0) flag_count_kernel<<<blocks_of(n), 256, 0, s>>>(n, flags, bit, w.a);
    if (hipGetLastError() != hipSuccess || gs2m_scan_u64(w.a, n, w.bsum, s) != hipSuccess) return GS2M_ERR_HIP;
    if (n > 0) compact_kernel<<<blocks_of(n), 256, 0, s>>>(n, pts, flags, bit, w.a, out);
    u64 total;
    if (gs2m_read_back(s, {{&total, w.a + n, 8}}) != GS2M_OK) return GS2M_ERR_HIP;
    *host_count = (long long)total;
    return GS2M_OK;
}

int gs2m_eval_nearest(long long n_queries, const double* queries, long long n_targets, double cell, const void* grid,
                      double max_dist, double* dist, void* stream) {
    return nearest(n_queries, queries, n_targets, cell, grid, max_dist, nullptr, dist, false, stream);
}

int gs2m_eval_nearest_index(long long n_queries, const double* queries, long long n_targets, double cell, const void* grid,
                            double max_dist, long long* index, double* dist, void* stream) {
    if (n_queries > 0 && !index) return GS2M_ERR_INVALID_ARG;
    return nearest(n_queries, queries, n_targets, cell, grid, max_dist, index, dist, true, stream);
}

int gs2m_eval_masked_mean(long long n, const double* dist, double max_dist, void* ws, double* host_sum, long long* host_count,
                          void* stream) {
    if (n < 0 || !ws || !host_sum || !host_count || (n > 0 && !dist)) return GS2M_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    const ScanWs w = carve_scan((char*)ws, 0);  // the partials only (at the same place for every n)
    reduce_fixed_order<1, SumOp>(n, MeanTerm{dist, max_dist}, w.psum, w.pcnt, w.psum + RED_BLOCKS, w.pcnt + RED_BLOCKS, s);
    u64 c;
    if (gs2m_read_back(s, {{host_sum, w.psum + RED_BLOCKS, 8}, {&c, w.pcnt + RED_BLOCKS, 8}}) != GS2M_OK) return GS2M_ERR_HIP;
    *host_count = (long long)c;
    return GS2M_OK;
}

}  // extern "C"
