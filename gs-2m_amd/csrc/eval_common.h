// Host and device primitives shared by the mesh units: tsdf.hip, mesh_eval.hip, tnt_eval.hip and mesh_post.hip.
#pragma once
#include <initializer_list>
#include "common.h"

typedef unsigned long long u64;
constexpr long long MAX_POINTS = 0xFFFFFFF0ll;  // sorted slots and indices are u32
constexpr long long MAX_LAUNCH = 256ll * 0x7FFFFFFFll;
static inline unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }

struct V3 {
    double v[3];
};

// ---- workspace carving ----
// Typed arrays one after the other out of a caller's byte buffer, each followed by padding to GS2M_ALIGN.  base may be null:
// `off` then sizes the buffer.  The layouts are part of what callers rely on (a grid is held across calls; the reductions'
// partials sit in front of the scan workspace at a place that does not depend on n): arrays are taken in a fixed order.
struct Carver {
    char* base;
    size_t off;  // bytes taken so far
    template <class T>
    T* take(size_t count) {
        T* p = (T*)(base + off);
        off = gs2m_align_up(off + sizeof(T) * count);
        return p;
    }
};

// the four ping-pong arrays of gs2m_radix_sort_pairs, m entries each; the sorted pairs end in kB / vB
struct SortBufs {
    uint32_t *kA, *vA, *kB, *vB;
};
static inline SortBufs take_sort_bufs(Carver& c, size_t m) {
    SortBufs b;
    b.kA = c.take<uint32_t>(m);
    b.vA = c.take<uint32_t>(m);
    b.kB = c.take<uint32_t>(m);
    b.vB = c.take<uint32_t>(m);
    return b;
}

// ---- blocking read-back of a few words ----
struct ReadBack {
    void* dst;        // host
    const void* src;  // device
    size_t bytes;
};
// What the launches before it left in hipGetLastError, the copies to the host, the wait for the stream.
static inline int gs2m_read_back(hipStream_t s, std::initializer_list<ReadBack> copies) {
    if (hipGetLastError() != hipSuccess) return GS2M_ERR_HIP;
    for (const ReadBack& c : copies)
        if (hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, s) != hipSuccess) return GS2M_ERR_HIP;
    return gs2m_status(hipStreamSynchronize(s));
}

// ---- device-wide exclusive scan of u64 counts, in place (mesh_eval.hip) ----
// a: n + 1 entries, counts in [0, n); bsum: gs2m_scan_blocks(n) + 1 entries.  Exclusive prefixes in place, the total in a[n].
long long gs2m_scan_blocks(long long n);
hipError_t gs2m_scan_u64(u64* a, long long n, u64* bsum, hipStream_t s);

// ---- hashed uniform grid (built by mesh_eval.hip: gs2m_eval_grid_build; read there and by tnt_clouds.hip) ----
// The cell (floor(p / cell) per axis) hashes to a bucket of 2^bits; a bucket holds every point whose cell hashes to it, so a
// reader that needs one cell's points alone compares each candidate's own cell.
constexpr int CELL_LIMIT = 1 << 30;

__device__ __forceinline__ int cell_coord(double x, double inv) {
    const double f = floor(x * inv);
    return f < -(double)CELL_LIMIT ? -CELL_LIMIT : (f > (double)CELL_LIMIT ? CELL_LIMIT : (int)f);  // NaN -> the upper bound
}

__device__ __forceinline__ uint32_t hash3(int x, int y, int z, uint32_t mask) {
    uint64_t h = (uint64_t)(uint32_t)x * 0x9E3779B97F4A7C15ull;
    h ^= (uint64_t)(uint32_t)y * 0xC2B2AE3D27D4EB4Full;
    h ^= (uint64_t)(uint32_t)z * 0x165667B19E3779F9ull;
    h ^= h >> 31;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 29;
    return (uint32_t)h & mask;
}

static inline int grid_bits(long long n) {
    int k = 10;
    while (k < 28 && (1ll << k) < n) k++;
    return k;
}

struct Grid {
    double* spts;    // n x 3: the points in bucket order
    uint32_t* sidx;  // n: their original indices
    uint32_t* start; // 2^bits + 1: first sorted slot of every bucket
    uint8_t* occ;    // 2^bits: 1 = a coarse cell hashing here holds a point
    int bits;
    size_t bytes;
};
static inline Grid carve_grid(char* base, long long n) {
    Carver c{base, 0};
    Grid g;
    g.bits = grid_bits(n);
    const size_t nb = (size_t)1 << g.bits;
    g.spts = c.take<double>(3 * (size_t)n);
    g.sidx = c.take<uint32_t>(n);
    g.start = c.take<uint32_t>(nb + 1);
    g.occ = c.take<uint8_t>(nb);
    g.bytes = c.off;
    return g;
}
// ---- the workspace of gs2m_mesh_compact (mesh_post.hip) ----
// mesh_simplify.hip reads `av` after the call: av[v] is the new id of vertex v where av[v + 1] != av[v] (v survived).
struct CompactWs {
    unsigned char* used;  // V
    u64* av;              // V + 1
    u64* at;              // F + 1
    u64* bsum;            // scan blocks of the longer of the two + 1
    int* err;
    size_t bytes;
};
static inline CompactWs carve_compact(char* base, long long nv, long long nt) {
    Carver c{base, 0};
    CompactWs w;
    w.used = c.take<unsigned char>((size_t)(nv > 0 ? nv : 1));
    w.av = c.take<u64>((size_t)nv + 1);
    w.at = c.take<u64>((size_t)nt + 1);
    w.bsum = c.take<u64>(gs2m_scan_blocks(nv > nt ? nv : nt) + 1);
    w.err = c.take<int>(2);
    w.bytes = c.off;
    return w;
}

// a triangle's vertex indices against the vertex count
__device__ __forceinline__ bool ids_in_range(int a, int b, int c, long long nv) {
    return !(a < 0 || b < 0 || c < 0 || a >= nv || b >= nv || c >= nv);
}
// the same; err[0] = 1 tells the host of one out of range
__device__ __forceinline__ bool tri_in_range(int a, int b, int c, long long nv, int* __restrict__ err) {
    if (!ids_in_range(a, b, c, nv)) {
        err[0] = 1;
        return false;
    }
    return true;
}

// ---- fixed-order reduction of Q fp64 quantities and a count over n elements ----
// The order of the operations is a contract (two runs are bitwise identical; tests/dtu_eval_ref.py
// fixed_order_sum restates it and the GPU tests hold the sums to it bit for bit):
//   RED_BLOCKS workgroups of 256 threads; a thread folds the elements b * 256 + tid + m * RED_BLOCKS * 256 in m order into
//   Op::identity, through term(i, acc, count); the lanes of a wave fold by __shfl_down 32, 16, 8, 4, 2, 1; the four waves
//   as (w0 op w1) op (w2 op w3); a second kernel folds the RED_BLOCKS partials in order into Op::identity.
// part: Q RED_BLOCKS, pcnt: RED_BLOCKS (null: no count), out: Q, out_cnt: 1.
constexpr int RED_BLOCKS = 256;

struct SumOp {
    __device__ static double identity(int) { return 0.0; }
    __device__ static double combine(int, double a, double b) { return a + b; }
};

template <int Q, class Term, class Op>
__global__ void __launch_bounds__(256) reduce_partial_kernel(long long n, Term term, double* __restrict__ part, u64* __restrict__ pcnt) {
    __shared__ double s_a[4][Q];
    __shared__ u64 s_c[4];
    double acc[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) acc[q] = Op::identity(q);
    u64 c = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) term(i, acc, c);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int q = 0; q < Q; q++) acc[q] = Op::combine(q, acc[q], __shfl_down(acc[q], o, 64));
        c += __shfl_down(c, o, 64);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < Q; q++) s_a[w][q] = acc[q];
        s_c[w] = c;
    }
    __syncthreads();
    if (threadIdx.x < Q) {
        const int q = threadIdx.x;
        part[(size_t)blockIdx.x * Q + q] = Op::combine(q, Op::combine(q, s_a[0][q], s_a[1][q]), Op::combine(q, s_a[2][q], s_a[3][q]));
    }
    if (threadIdx.x == 0 && pcnt) pcnt[blockIdx.x] = (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]);
}

template <int Q, class Op>
__global__ void __launch_bounds__(64) reduce_final_kernel(const double* __restrict__ part, const u64* __restrict__ pcnt,
                                                          double* __restrict__ out, u64* __restrict__ out_cnt) {
    const int q = threadIdx.x;
    if (q < Q) {
        double r = Op::identity(q);
        for (int b = 0; b < RED_BLOCKS; b++) r = Op::combine(q, r, part[(size_t)b * Q + q]);
        out[q] = r;
    }
    if (q == 0 && pcnt) {
        u64 c = 0;
        for (int b = 0; b < RED_BLOCKS; b++) c += pcnt[b];
        *out_cnt = c;
    }
}

template <int Q, class Op, class Term>
void reduce_fixed_order(long long n, const Term& term, double* part, u64* pcnt, double* out, u64* out_cnt, hipStream_t s) {
    reduce_partial_kernel<Q, Term, Op><<<RED_BLOCKS, 256, 0, s>>>(n, term, part, pcnt);
    reduce_final_kernel<Q, Op><<<1, 64, 0, s>>>(part, pcnt, out, out_cnt);
}
