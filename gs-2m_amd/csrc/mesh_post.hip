// Mesh post-processing: edge-connected triangle clusters and the compaction behind post_process_mesh
// (include/gs2m_mesh.h, "post-processing"; the contract and the choice of algorithm: DESIGN.md §9).
//
// Clusters: every triangle writes its three unordered vertex pairs (lo, hi) at the slots 3 t + k; the slots sort by
// (lo, hi) with the project's stable 32-bit radix sort, hi first and then lo (LSD, as tnt_eval.hip sorts its 64-bit voxel
// keys), each over just the bits that hold V - 1; a thread per sorted position whose pair equals its predecessor's unites
// the two owning triangles in a lock-free union-find that hooks the larger root under the smaller (CAS on roots only), so
// that a component's root is its smallest triangle index whatever the order of the unions; a pointer-jumping pass without
// atomics brings every triangle to its root; the root flags go through gs2m_scan_u64 and give the cluster numbers; integer
// atomicAdds, one per wave and label where the lanes agree, count the sizes.  Vertex ids are only ever sort keys here.
// Compaction: plain byte stores of 1 mark the vertices of the kept triangles, two scans number the surviving vertices and
// the emitted triangles, two gathers write them.  A kernel that indexes with a vertex id tests it first (tri_in_range).
// tri_cluster doubles as the union-find's parent array.  Integer work only: two runs are bitwise identical.
#include "eval_common.h"
#include "../../include/gs2m_mesh.h"

namespace {

constexpr int ROWS = 4;  // triangle rows per thread: 48 bytes, three 16-byte loads

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// rows t0 .. t0 + 3 (t0 a multiple of 4) as 12 ints; `vec`: the array is 16-byte aligned.  Rows at or beyond nt read as 0.
__device__ __forceinline__ void load_rows(const int* __restrict__ tris, long long t0, long long nt, bool vec, int v[3 * ROWS]) {
    if (vec && t0 + ROWS <= nt) {
        const int4* p = reinterpret_cast<const int4*>(tris + 3 * t0);
        const int4 a = p[0], b = p[1], c = p[2];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
    } else {
#pragma unroll
        for (int k = 0; k < 3 * ROWS; k++) v[k] = 3 * t0 + k < 3 * nt ? tris[3 * t0 + k] : 0;
    }
}

// ---- clusters ----

// slots 3 t + k: the pair of (v_k, v_k+1) as (lo, hi); parent[t] = t.  A triangle with an id out of range sets err and
// writes (0, 0): the call fails, and the keys stay within the bits the sort looks at.
__global__ void __launch_bounds__(256) edge_kernel(long long nv, long long nt, const int* __restrict__ tris, bool vec,
                                                   uint32_t* __restrict__ lo, uint32_t* __restrict__ hi, int* __restrict__ parent,
                                                   int* __restrict__ err) {
    const long long t0 = ROWS * ((long long)blockIdx.x * 256 + threadIdx.x);
    if (t0 >= nt) return;
    int v[3 * ROWS];
    load_rows(tris, t0, nt, vec, v);
    uint32_t l[3 * ROWS], h[3 * ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; r++) {
        const bool ok = t0 + r < nt && tri_in_range(v[3 * r], v[3 * r + 1], v[3 * r + 2], nv, err);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int a = v[3 * r + k], b = v[3 * r + (k + 1) % 3];
            l[3 * r + k] = ok ? (uint32_t)(a < b ? a : b) : 0u;
            h[3 * r + k] = ok ? (uint32_t)(a < b ? b : a) : 0u;
        }
    }
    if (t0 + ROWS <= nt) {  // lo and hi are carved at GS2M_ALIGN and 12 t0 words is a multiple of 16 bytes
        uint4* pl = reinterpret_cast<uint4*>(lo + 3 * t0);
        uint4* ph = reinterpret_cast<uint4*>(hi + 3 * t0);
#pragma unroll
        for (int q = 0; q < 3; q++) {
            pl[q] = make_uint4(l[4 * q], l[4 * q + 1], l[4 * q + 2], l[4 * q + 3]);
            ph[q] = make_uint4(h[4 * q], h[4 * q + 1], h[4 * q + 2], h[4 * q + 3]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3 * ROWS; k++)
            if (3 * t0 + k < 3 * nt) {
                lo[3 * t0 + k] = l[k];
                hi[3 * t0 + k] = h[k];
            }
    }
#pragma unroll
    for (int r = 0; r < ROWS; r++)
        if (t0 + r < nt) parent[t0 + r] = (int)(t0 + r);
}

// the order by hi -> the keys of the second sort: k2[j] = lo of the slot at j, v2[j] = that slot
__global__ void __launch_bounds__(256) edge_regather_kernel(long long m, const uint32_t* __restrict__ order, const uint32_t* __restrict__ lo,
                                                            uint32_t* __restrict__ k2, uint32_t* __restrict__ v2) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const uint32_t s = order[j];
    k2[j] = lo[s];
    v2[j] = s;
}

// The union-find's loads and stores while unions are under way: relaxed, at device scope, so that a value another
// compute die has written is seen sooner or later; no read-modify-write.  Every value ever stored in parent[x] is x or an
// ancestor of x in x's component, and parent[x] <= x, so a late or a lost plain update costs steps, never correctness.
__device__ __forceinline__ int uf_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void uf_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above x, halving the path on the way: only entries that already have a parent other than themselves are
// rewritten (never a root: the CAS of a hook is the only writer of a root's entry)
__device__ __forceinline__ int uf_find(int* parent, int x) {
    int p = uf_load(parent + x);
    while (p != x) {
        const int g = uf_load(parent + p);
        if (g != p) uf_store(parent + x, g);
        x = p;
        p = g;
    }
    return x;
}

__device__ __forceinline__ void uf_unite(int* parent, int a, int b) {
    int ra = uf_find(parent, a), rb = uf_find(parent, b);
    while (ra != rb) {
        const int big = ra > rb ? ra : rb, small = ra > rb ? rb : ra;
        const int old = atomicCAS(parent + big, big, small);
        if (old == big) return;
        ra = uf_find(parent, old);  // `big` was hooked by another thread meanwhile: go on from what it hangs under
        rb = uf_find(parent, small);
    }
}

// sorted position j whose pair equals that of j - 1: the two owning triangles are connected
__global__ void __launch_bounds__(256) unite_kernel(long long m, const uint32_t* __restrict__ klo, const uint32_t* __restrict__ slot,
                                                    const uint32_t* __restrict__ hi, int* parent) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x + 1;
    if (j >= m || klo[j] != klo[j - 1]) return;
    const uint32_t s1 = slot[j], s0 = slot[j - 1];
    if (hi[s1] != hi[s0]) return;
    const int a = (int)(s1 / 3u), b = (int)(s0 / 3u);
    if (a != b) uf_unite(parent, a, b);
}

// every triangle to its root (the roots are final: no hook runs any more), flag[t] = t is a root
__global__ void __launch_bounds__(256) flatten_kernel(long long nt, int* parent, u64* __restrict__ flag) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    int r = parent[t];
    for (int p = parent[r]; p != r; p = parent[r]) r = p;
    parent[t] = r;
    flag[t] = r == (int)t ? 1ull : 0ull;
}

// num: the exclusive prefixes of the root flags.  tri_cluster[t] (the root on entry) = num[root]; sizes counted with one
// atomicAdd per wave and label for the labels the first lanes left hold (a mesh's triangles come cluster by cluster), one
// per lane after LABEL_ROUNDS of that.
constexpr int LABEL_ROUNDS = 4;
__global__ void __launch_bounds__(256) label_kernel(long long nt, int* tri_cluster, const u64* __restrict__ num, int* __restrict__ size) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    bool active = t < nt;
    int label = 0;
    if (active) {
        label = (int)num[tri_cluster[t]];
        tri_cluster[t] = label;
    }
    const int lane = threadIdx.x & 63;
    for (int round = 0; round < LABEL_ROUNDS; round++) {
        const u64 left = __ballot(active);
        if (!left) break;
        const int leader = __ffsll((long long)left) - 1;
        const int lead = __shfl(label, leader, 64);
        const bool same = active && label == lead;
        const int cnt = __popcll(__ballot(same));
        if (lane == leader) atomicAdd(size + lead, cnt);
        active = active && !same;
    }
    if (active) atomicAdd(size + label, 1);
}

__global__ void __launch_bounds__(256) keep_kernel(long long nt, const int* __restrict__ tri_cluster, const int* __restrict__ size,
                                                   int min_size, unsigned char* __restrict__ keep) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const int c = tri_cluster[t];
    keep[t] = c >= 0 && c < nt && size[c] >= min_size ? 1 : 0;  // size has nt entries
}

struct ClusterWs {
    uint32_t *lo, *hi, *k2, *v2;  // 3 F each
    SortBufs sort;
    u64* a;     // F + 1
    u64* bsum;  // scan blocks + 1
    int* err;
    void* temp;
    size_t temp_bytes, bytes;
};
ClusterWs carve_cluster(char* base, long long nt) {
    Carver c{base, 0};
    ClusterWs w;
    const size_t m = (size_t)(nt > 0 ? 3 * nt : 1);
    w.lo = c.take<uint32_t>(m);
    w.hi = c.take<uint32_t>(m);
    w.k2 = c.take<uint32_t>(m);
    w.v2 = c.take<uint32_t>(m);
    w.sort = take_sort_bufs(c, m);
    w.a = c.take<u64>((size_t)nt + 1);
    w.bsum = c.take<u64>(gs2m_scan_blocks(nt) + 1);
    w.err = c.take<int>(2);
    const size_t t32 = gs2m_radix_temp_bytes(m, 32), t16 = gs2m_radix_temp_bytes(m, 16);
    w.temp_bytes = t32 > t16 ? t32 : t16;
    w.temp = c.take<char>(w.temp_bytes + GS2M_ALIGN);
    w.bytes = c.off;
    return w;
}

// ---- compaction ----

// used[v] = 1 for the vertices of the kept triangles (degenerate ones included); flag[t] = t is kept and its ids differ
__global__ void __launch_bounds__(256) mark_kernel(long long nv, long long nt, const int* __restrict__ tris, bool vec,
                                                   const unsigned char* __restrict__ keep, unsigned char* __restrict__ used,
                                                   u64* __restrict__ flag, int* __restrict__ err) {
    const long long t0 = ROWS * ((long long)blockIdx.x * 256 + threadIdx.x);
    if (t0 >= nt) return;
    int v[3 * ROWS];
    load_rows(tris, t0, nt, vec, v);
#pragma unroll
    for (int r = 0; r < ROWS; r++) {
        if (t0 + r >= nt) break;
        const int a = v[3 * r], b = v[3 * r + 1], c = v[3 * r + 2];
        const bool k = tri_in_range(a, b, c, nv, err) && keep[t0 + r] != 0;
        if (k) used[a] = used[b] = used[c] = 1;
        flag[t0 + r] = k && a != b && b != c && c != a ? 1ull : 0ull;
    }
}

__global__ void __launch_bounds__(256) widen_kernel(long long n, const unsigned char* __restrict__ used, u64* __restrict__ flag) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) flag[i] = used[i];
}

// a thread per float of the vertex array (coalesced reads; the survivors keep their order, so the writes are runs too)
__global__ void __launch_bounds__(256) gather_vertices_kernel(long long n3, const u64* __restrict__ av, const float* __restrict__ vin,
                                                              const float* __restrict__ cin, float* __restrict__ vout,
                                                              float* __restrict__ cout) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n3) return;
    const long long v = i / 3;
    const u64 d = av[v];
    if (av[v + 1] == d) return;
    const size_t o = 3 * (size_t)d + (size_t)(i - 3 * v);
    vout[o] = vin[i];
    if (cin) cout[o] = cin[i];
}

// at[t + 1] != at[t]: t is emitted, so it was kept with ids in range (mark_kernel), all three of them marked
__global__ void __launch_bounds__(256) gather_triangles_kernel(long long nt, const int* __restrict__ tris, bool vec, const u64* __restrict__ at,
                                                               const u64* __restrict__ av, int* __restrict__ out) {
    const long long t0 = ROWS * ((long long)blockIdx.x * 256 + threadIdx.x);
    if (t0 >= nt) return;
    int v[3 * ROWS];
    load_rows(tris, t0, nt, vec, v);
    u64 d = at[t0];
#pragma unroll
    for (int r = 0; r < ROWS; r++) {
        if (t0 + r >= nt) break;
        const u64 e = at[t0 + r + 1];
        if (e != d) {
#pragma unroll
            for (int k = 0; k < 3; k++) out[3 * (size_t)d + k] = (int)av[v[3 * r + k]];
        }
        d = e;
    }
}

int bits_holding(long long vmax) {  // bits that hold 0 .. vmax
    int b = 1;
    while (b < 32 && (1ll << b) <= vmax) b++;
    return b;
}

bool sizes_ok(long long nv, long long nt) { return nv <= 0x7FFFFFFFll && 3 * nt <= MAX_POINTS; }

}  // namespace

extern "C" {

int gs2m_mesh_post_workspace_bytes(long long n_vertices, long long n_triangles, long long* cluster_bytes, long long* compact_bytes) {
    if (n_vertices < 0 || n_triangles < 0 || (!cluster_bytes && !compact_bytes)) return GS2M_ERR_INVALID_ARG;
    if (!sizes_ok(n_vertices, n_triangles)) return GS2M_ERR_UNSUPPORTED;
    if (cluster_bytes) *cluster_bytes = (long long)carve_cluster(nullptr, n_triangles).bytes;
    if (compact_bytes) *compact_bytes = (long long)carve_compact(nullptr, n_vertices, n_triangles).bytes;
    return GS2M_OK;
}

int gs2m_mesh_cluster_triangles(long long n_vertices, long long n_triangles, const int* triangles, void* ws, int* tri_cluster,
                                int* cluster_size, long long* n_clusters, void* stream) {
    if (n_vertices < 0 || n_triangles < 0 || !n_clusters || (n_triangles > 0 && (!triangles || !ws || !tri_cluster || !cluster_size)))
        return GS2M_ERR_INVALID_ARG;
    if (!sizes_ok(n_vertices, n_triangles)) return GS2M_ERR_UNSUPPORTED;
    *n_clusters = 0;
    if (n_triangles == 0) return GS2M_OK;
    hipStream_t s = (hipStream_t)stream;
    const long long nt = n_triangles, m = 3 * nt;
    const ClusterWs w = carve_cluster((char*)ws, nt);
    const SortBufs& b = w.sort;
    const int bits = bits_holding(n_vertices - 1);
    if (hipMemsetAsync(w.err, 0, 8, s) != hipSuccess || hipMemsetAsync(cluster_size, 0, 4 * (size_t)nt, s) != hipSuccess) return GS2M_ERR_HIP;
    edge_kernel<<<blocks_of((nt + ROWS - 1) / ROWS), 256, 0, s>>>(n_vertices, nt, triangles, aligned16(triangles), w.lo, w.hi, tri_cluster, w.err);
    if (hipGetLastError() != hipSuccess ||
        gs2m_radix_sort_pairs(w.temp, w.temp_bytes, w.hi, nullptr, b.kA, b.vA, b.kB, b.vB, (size_t)m, bits, false, s) != hipSuccess)
        return GS2M_ERR_HIP;
    edge_regather_kernel<<<blocks_of(m), 256, 0, s>>>(m, b.vB, w.lo, w.k2, w.v2);
    if (hipGetLastError() != hipSuccess ||
        gs2m_radix_sort_pairs(w.temp, w.temp_bytes, w.k2, w.v2, b.kA, b.vA, b.kB, b.vB, (size_t)m, bits, false, s) != hipSuccess)
        return GS2M_ERR_HIP;
    unite_kernel<<<blocks_of(m), 256, 0, s>>>(m, b.kB, b.vB, w.hi, tri_cluster);
    flatten_kernel<<<blocks_of(nt), 256, 0, s>>>(nt, tri_cluster, w.a);
    if (hipGetLastError() != hipSuccess || gs2m_scan_u64(w.a, nt, w.bsum, s) != hipSuccess) return GS2M_ERR_HIP;
    label_kernel<<<blocks_of(nt), 256, 0, s>>>(nt, tri_cluster, w.a, cluster_size);
    u64 total = 0;
    int bad = 0;
    if (gs2m_read_back(s, {{&total, w.a + nt, 8}, {&bad, w.err, 4}}) != GS2M_OK) return GS2M_ERR_HIP;
    if (bad) return GS2M_ERR_INVALID_ARG;
    *n_clusters = (long long)total;
    return GS2M_OK;
}

int gs2m_mesh_keep_clusters(long long n_triangles, const int* tri_cluster, const int* cluster_size, int min_size, unsigned char* keep,
                            void* stream) {
    if (n_triangles < 0 || (n_triangles > 0 && (!tri_cluster || !cluster_size || !keep))) return GS2M_ERR_INVALID_ARG;
    if (n_triangles > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    if (n_triangles == 0) return GS2M_OK;
    keep_kernel<<<blocks_of(n_triangles), 256, 0, (hipStream_t)stream>>>(n_triangles, tri_cluster, cluster_size, min_size, keep);
    return gs2m_status(hipGetLastError());
}

int gs2m_mesh_compact(long long n_vertices, long long n_triangles, const float* vertices, const float* colors, const int* triangles,
                      const unsigned char* keep, void* ws, float* out_vertices, float* out_colors, int* out_triangles, long long* totals,
                      void* stream) {
    if (n_vertices < 0 || n_triangles < 0 || !totals || (n_vertices > 0 && (!vertices || !out_vertices || (colors && !out_colors))) ||
        (n_triangles > 0 && (!triangles || !keep || !ws || !out_triangles)))
        return GS2M_ERR_INVALID_ARG;
    if (!sizes_ok(n_vertices, n_triangles)) return GS2M_ERR_UNSUPPORTED;
    totals[0] = totals[1] = 0;
    if (n_triangles == 0) return GS2M_OK;  // nothing is kept: no vertex survives
    hipStream_t s = (hipStream_t)stream;
    const long long nv = n_vertices, nt = n_triangles;
    const CompactWs w = carve_compact((char*)ws, nv, nt);
    const bool vec = aligned16(triangles);
    if (hipMemsetAsync(w.err, 0, 8, s) != hipSuccess || (nv > 0 && hipMemsetAsync(w.used, 0, (size_t)nv, s) != hipSuccess)) return GS2M_ERR_HIP;
    mark_kernel<<<blocks_of((nt + ROWS - 1) / ROWS), 256, 0, s>>>(nv, nt, triangles, vec, keep, w.used, w.at, w.err);
    if (nv > 0) widen_kernel<<<blocks_of(nv), 256, 0, s>>>(nv, w.used, w.av);
    if (hipGetLastError() != hipSuccess || gs2m_scan_u64(w.av, nv, w.bsum, s) != hipSuccess || gs2m_scan_u64(w.at, nt, w.bsum, s) != hipSuccess)
        return GS2M_ERR_HIP;
    if (nv > 0) gather_vertices_kernel<<<blocks_of(3 * nv), 256, 0, s>>>(3 * nv, w.av, vertices, colors, out_vertices, out_colors);
    gather_triangles_kernel<<<blocks_of((nt + ROWS - 1) / ROWS), 256, 0, s>>>(nt, triangles, vec, w.at, w.av, out_triangles);
    u64 tv = 0, tt = 0;
    int bad = 0;
    if (gs2m_read_back(s, {{&tv, w.av + nv, 8}, {&tt, w.at + nt, 8}, {&bad, w.err, 4}}) != GS2M_OK) return GS2M_ERR_HIP;
    if (bad) return GS2M_ERR_INVALID_ARG;
    totals[0] = (long long)tv;
    totals[1] = (long long)tt;
    return GS2M_OK;
}

}  // extern "C"
