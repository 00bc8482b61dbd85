// TSDF depth fusion and marching-cubes extraction (include/gs2m_mesh.h; the contract: DESIGN.md §9).
//
// Data: a pool of 16^3-voxel blocks (fp32 tsdf / weight / colour, structure-of-arrays per block slot) and a dense int32
// block-index table over a fixed box of blocks (an indirection table, not a hash).  Per view:
//   touch_kernel           one thread per stride-4 pixel: marks the blocks its point's trunc box touches (plain stores of 1
//                          into a byte per domain block; the count of ignored points is the only atomic, an integer add)
//   chunk_count_kernel     per 1024 domain blocks: touched and new (touched, no slot yet) counts, packed in one word
//   chunk_scan_kernel      one workgroup: exclusive prefixes over the chunks, capacity check, slot count update
//   chunk_assign_kernel    per 1024 domain blocks: new slots in linear-index order, the view's touched-slot list; clears
//                          the marks.  Writes nothing but the marks when the pool is full.
//   integrate_kernel       one thread per voxel of the touched blocks, gathering from the depth / colour images
// Extraction:
//   cube_case_kernel       per voxel: the cube's validity and case (u16, 0xFFFF = invalid)
//   mesh_count_kernel      per block: the owned edges a valid cube uses (each voxel's mask kept in vinfo) and the triangles,
//                          packed per block
//   slot_scan_kernel       one workgroup: exclusive prefixes over the blocks, the totals
//   emit_vertices_kernel   per block: vertex positions / colours in (voxel, axis) order from the stored masks; each voxel's
//                          first vertex id joins its mask in vinfo
//   emit_triangles_kernel  per block: triangles in (voxel, table order), vertex ids looked up at the edges' owner voxels
// No float atomics anywhere: every value is written by one thread in an order fixed by the scans, so two runs are bitwise
// identical.  Compiled with -ffp-contract=off: every expression is evaluated as written, which tests/mesh_ref.py restates.
#include <limits.h>
#include "eval_common.h"
#include "../../include/gs2m_mesh.h"
#define GS2M_MC_CONST __constant__
#include "tsdf_tables.h"

namespace {

constexpr int BV = 4096;        // voxels per block
constexpr int CHUNK = 1024;     // domain blocks per workgroup of the touch scan (256 threads x 4)
constexpr int VINFO_BITS = 29;  // emit: first vertex id of a voxel below, its used-edge mask above

struct Dom {
    int x0, y0, z0, nx, ny, nz;
};
struct Mat34 {
    float m[12];
};

// cube corner offsets and, per edge, the owner voxel's offset from the cube origin and the edge's axis
__constant__ int c_corner[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
__constant__ int c_edge_owner[12][4] = {{0, 0, 0, 0}, {1, 0, 0, 1}, {0, 1, 0, 0}, {0, 0, 0, 1}, {0, 0, 1, 0}, {1, 0, 1, 1},
                                        {0, 1, 1, 0}, {0, 0, 1, 1}, {0, 0, 0, 2}, {1, 0, 0, 2}, {1, 1, 0, 2}, {0, 1, 0, 2}};

struct TouchWs {
    uint8_t* flags;     // N: 1 = touched by this view
    uint32_t* chunk;    // nchunks: touched | new << 16, then their exclusive prefixes (touched_pref, new_pref in two arrays)
    uint32_t* pref_t;   // nchunks
    uint32_t* pref_n;   // nchunks
    int* counters;      // 8: [0] new, [1] touched, [2] base slot, [3] fits, [4] ignored points
    size_t bytes;
};
TouchWs carve_touch(char* base, long long N) {
    const size_t nch = (size_t)((N + CHUNK - 1) / CHUNK);
    Carver c{base, 0};
    TouchWs w;
    w.flags = c.take<uint8_t>(N);
    w.chunk = c.take<uint32_t>(nch);
    w.pref_t = c.take<uint32_t>(nch);
    w.pref_n = c.take<uint32_t>(nch);
    w.counters = c.take<int>(8);
    w.bytes = c.off;
    return w;
}
struct MeshWs {
    uint16_t* cube;      // n * 4096: case, or 0xFFFF for an invalid cube
    uint32_t* vinfo;     // n * 4096: used-edge mask << 29 (mesh_count_kernel), then | first vertex id (emit_vertices_kernel)
    uint32_t* slot_cnt;  // n: vertices | triangles << 16 of the block
    uint32_t* pref_v;    // n
    uint32_t* pref_t;    // n
    u64* totals;         // 2
    size_t bytes;
};
MeshWs carve_mesh(char* base, long long n) {
    Carver c{base, 0};
    MeshWs w;
    const size_t nv = (size_t)n * BV;
    w.cube = c.take<uint16_t>(nv);
    w.vinfo = c.take<uint32_t>(nv);
    w.slot_cnt = c.take<uint32_t>(n);
    w.pref_v = c.take<uint32_t>(n);
    w.pref_t = c.take<uint32_t>(n);
    w.totals = c.take<u64>(2);
    w.bytes = c.off;
    return w;
}

__device__ __forceinline__ int float_key(float f) {
    const int b = __float_as_int(f);
    return b >= 0 ? b : b ^ 0x7FFFFFFF;
}

// the camera-space point of pixel (u, v) at depth d, in world space
__device__ __forceinline__ void back_project(int u, int v, float d, float fx, float fy, float cx, float cy, const Mat34& c,
                                             float p[3]) {
    const float xc = (((float)u - cx) * d) / fx;
    const float yc = (((float)v - cy) * d) / fy;
    const float zc = d;
#pragma unroll
    for (int r = 0; r < 3; r++) p[r] = ((c.m[4 * r] * xc + c.m[4 * r + 1] * yc) + c.m[4 * r + 2] * zc) + c.m[4 * r + 3];
}

__device__ __forceinline__ bool depth_ok(float d, float depth_trunc) { return d > 0.f && d <= depth_trunc; }

__global__ void __launch_bounds__(256) points_aabb_kernel(int W, int H, const float* __restrict__ depth, float depth_trunc,
                                                          float fx, float fy, float cx, float cy, Mat34 c2w, int* __restrict__ aabb) {
    __shared__ int s[6][4];
    const int ws = (W + 3) / 4, n = ws * ((H + 3) / 4);
    const int i = blockIdx.x * 256 + threadIdx.x;
    int key[6] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN};
    if (i < n) {
        const int u = 4 * (i % ws), v = 4 * (i / ws);
        const float d = depth[(size_t)v * W + u];
        if (depth_ok(d, depth_trunc)) {
            float p[3];
            back_project(u, v, d, fx, fy, cx, cy, c2w, p);
#pragma unroll
            for (int r = 0; r < 3; r++) key[r] = key[r + 3] = float_key(p[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < 6; r++) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const int o = __shfl_xor(key[r], d, 64);
            key[r] = r < 3 ? min(key[r], o) : max(key[r], o);
        }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0)
        for (int r = 0; r < 6; r++) s[r][w] = key[r];
    __syncthreads();
    if (threadIdx.x < 6) {
        const int r = threadIdx.x;
        int k = s[r][0];
        for (int q = 1; q < 4; q++) k = r < 3 ? min(k, s[r][q]) : max(k, s[r][q]);
        if (r < 3) atomicMin(aabb + r, k);
        else atomicMax(aabb + r, k);
    }
}

__global__ void __launch_bounds__(256) touch_kernel(Dom dom, float L, float trunc, int W, int H, const float* __restrict__ depth,
                                                    float depth_trunc, float fx, float fy, float cx, float cy, Mat34 c2w,
                                                    uint8_t* __restrict__ flags, int* __restrict__ ignored) {
    const int ws = (W + 3) / 4, n = ws * ((H + 3) / 4);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int u = 4 * (i % ws), v = 4 * (i / ws);
    const float d = depth[(size_t)v * W + u];
    if (!depth_ok(d, depth_trunc)) return;
    float p[3];
    back_project(u, v, d, fx, fy, cx, cy, c2w, p);
    int lo[3], hi[3];
    const int dmin[3] = {dom.x0, dom.y0, dom.z0}, dn[3] = {dom.nx, dom.ny, dom.nz};
    bool inside = true;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const float a = floorf((p[r] - trunc) / L), b = floorf((p[r] + trunc) / L);
        // compare as floats first: a point far outside must not overflow the int conversion
        inside = inside && a >= (float)dmin[r] && b < (float)dmin[r] + (float)dn[r];
        lo[r] = inside ? (int)a - dmin[r] : 0;
        hi[r] = inside ? (int)b - dmin[r] : -1;
        inside = inside && lo[r] >= 0 && hi[r] < dn[r];
    }
    if (!inside) {
        atomicAdd(ignored, 1);
        return;
    }
    for (int z = lo[2]; z <= hi[2]; z++)
        for (int y = lo[1]; y <= hi[1]; y++)
            for (int x = lo[0]; x <= hi[0]; x++) flags[((size_t)z * dom.ny + y) * dom.nx + x] = 1;
}

__global__ void __launch_bounds__(256) chunk_count_kernel(long long N, const uint8_t* __restrict__ flags, const int* __restrict__ index,
                                                          uint32_t* __restrict__ chunk) {
    __shared__ uint32_t s_w[4];
    const long long b0 = (long long)blockIdx.x * CHUNK + 4 * threadIdx.x;
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const long long b = b0 + k;
        if (b < N && flags[b]) c += 1u | (index[b] < 0 ? 1u << 16 : 0u);
    }
    uint32_t tot;
    gs2m_wg_exclusive_scan(c, s_w, &tot);
    if (threadIdx.x == 0) chunk[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(256) chunk_scan_kernel(int nchunks, const uint32_t* __restrict__ chunk, uint32_t* __restrict__ pref_t,
                                                         uint32_t* __restrict__ pref_n, int capacity, int* __restrict__ state,
                                                         int* __restrict__ counters) {
    __shared__ uint32_t s_w[4];
    unsigned long long carry_t = 0, carry_n = 0;
    for (int b = 0; b < nchunks; b += 256) {
        const int i = b + (int)threadIdx.x;
        const uint32_t c = i < nchunks ? chunk[i] : 0u;
        uint32_t tt, tn;
        const uint32_t et = gs2m_wg_exclusive_scan(c & 0xFFFFu, s_w, &tt);
        const uint32_t en = gs2m_wg_exclusive_scan(c >> 16, s_w, &tn);
        if (i < nchunks) {
            pref_t[i] = (uint32_t)(carry_t + et);
            pref_n[i] = (uint32_t)(carry_n + en);
        }
        carry_t += tt;
        carry_n += tn;
    }
    if (threadIdx.x == 0) {
        const long long base = state[0];
        const long long need = base + (long long)carry_n;
        const int fits = need <= (long long)capacity;
        counters[0] = (int)carry_n;
        counters[1] = (int)carry_t;
        counters[2] = (int)base;
        counters[3] = fits;
        if (fits) state[0] = (int)need;
        else counters[5] = need > INT_MAX ? INT_MAX : (int)need;
    }
}

__global__ void __launch_bounds__(256) chunk_assign_kernel(Dom dom, long long N, uint8_t* __restrict__ flags, int* __restrict__ index,
                                                           const uint32_t* __restrict__ pref_t, const uint32_t* __restrict__ pref_n,
                                                           const int* __restrict__ counters, int* __restrict__ block_coords,
                                                           int* __restrict__ touched_slots) {
    __shared__ uint32_t s_w[4];
    const long long b0 = (long long)blockIdx.x * CHUNK + 4 * threadIdx.x;
    uint8_t f[4];
    int idx[4];
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const long long b = b0 + k;
        f[k] = b < N ? flags[b] : 0;
        idx[k] = f[k] ? index[b] : 0;
        if (f[k]) c += 1u | (idx[k] < 0 ? 1u << 16 : 0u);
    }
    uint32_t tot;
    const uint32_t e = gs2m_wg_exclusive_scan(c, s_w, &tot);
    const bool fits = counters[3] != 0;
    uint32_t et = pref_t[blockIdx.x] + (e & 0xFFFFu), en = pref_n[blockIdx.x] + (e >> 16);
    const int base = counters[2];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const long long b = b0 + k;
        if (!f[k]) continue;
        flags[b] = 0;
        if (!fits) continue;
        int slot = idx[k];
        if (slot < 0) {
            slot = base + (int)en++;
            index[b] = slot;
            const long long x = b % dom.nx, yz = b / dom.nx, y = yz % dom.ny, z = yz / dom.ny;
            block_coords[3 * (size_t)slot] = dom.x0 + (int)x;
            block_coords[3 * (size_t)slot + 1] = dom.y0 + (int)y;
            block_coords[3 * (size_t)slot + 2] = dom.z0 + (int)z;
        }
        touched_slots[et++] = slot;
    }
}

// voxel centre coordinate along one axis
__device__ __forceinline__ float voxel_centre(int block, int i, float L, float voxel) {
    return (float)block * L + ((float)i + 0.5f) * voxel;
}

__global__ void __launch_bounds__(256) integrate_kernel(float voxel, float L, float trunc, int W, int H, const float* __restrict__ depth,
                                                        const float* __restrict__ color, float depth_trunc, float fx, float fy,
                                                        float cx, float cy, Mat34 w2c, const int* __restrict__ touched_slots,
                                                        const int* __restrict__ block_coords, float* __restrict__ tsdf,
                                                        float* __restrict__ weight, float* __restrict__ color_acc) {
    const int t = blockIdx.x >> 4;
    const int v = ((blockIdx.x & 15) << 8) + threadIdx.x;
    const int slot = touched_slots[t];
    const int bx = block_coords[3 * (size_t)slot], by = block_coords[3 * (size_t)slot + 1], bz = block_coords[3 * (size_t)slot + 2];
    const float x = voxel_centre(bx, v & 15, L, voxel), y = voxel_centre(by, (v >> 4) & 15, L, voxel), z = voxel_centre(bz, v >> 8, L, voxel);
    const float* m = w2c.m;
    const float xc = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
    const float yc = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
    const float zc = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
    if (!(zc > 0.f)) return;
    const float uf = ((xc * fx) / zc + cx) + 0.5f;
    const float vf = ((yc * fy) / zc + cy) + 0.5f;
    if (!(uf >= 0.0001f && uf < (float)W && vf >= 0.0001f && vf < (float)H)) return;
    const int u = (int)uf, vv = (int)vf;
    const size_t pix = (size_t)vv * W + u;
    const float d = depth[pix];
    if (!depth_ok(d, depth_trunc)) return;
    const float a = ((float)u - cx) / fx, b = ((float)vv - cy) / fy;
    const float sdf = (d - zc) * sqrtf((1.0f + a * a) + b * b);
    if (!(sdf > -trunc)) return;
    const float tv = fminf(1.0f, sdf / trunc);
    const size_t g = (size_t)slot * BV + v;
    const float w = weight[g], w1 = w + 1.0f;
    tsdf[g] = (tsdf[g] * w + tv) / w1;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const size_t gc = ((size_t)slot * 3 + c) * BV + v;
        color_acc[gc] = (color_acc[gc] * w + color[3 * pix + c]) / w1;
    }
    weight[g] = w1;
}

// The global voxel id of voxel (i, j, k) of the block at block coordinates (bx, by, bz) + the carry of i, j, k out of
// [0, 16) -- i, j, k in [-1, 17] --, or -1 when that block does not exist.
__device__ __forceinline__ long long voxel_ref(const Dom& dom, const int* __restrict__ index, int slot, int bx, int by, int bz, int i,
                                               int j, int k) {
    const int ox = i < 0 ? -1 : (i >= 16 ? 1 : 0), oy = j < 0 ? -1 : (j >= 16 ? 1 : 0), oz = k < 0 ? -1 : (k >= 16 ? 1 : 0);
    if (ox | oy | oz) {
        const int x = bx + ox - dom.x0, y = by + oy - dom.y0, z = bz + oz - dom.z0;
        if (x < 0 || y < 0 || z < 0 || x >= dom.nx || y >= dom.ny || z >= dom.nz) return -1;
        slot = index[((size_t)z * dom.ny + y) * dom.nx + x];
        if (slot < 0) return -1;
    }
    return (long long)slot * BV + ((i - 16 * ox) + 16 * (j - 16 * oy) + 256 * (k - 16 * oz));
}

__device__ __forceinline__ int ntri_of(int c) {
    int n = 0;
    while (n < 5 && GS2M_MC_TRI[c][3 * n] >= 0) n++;
    return n;
}

__global__ void __launch_bounds__(256) cube_case_kernel(Dom dom, const int* __restrict__ index, const int* __restrict__ block_coords,
                                                        const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                        uint16_t* __restrict__ cube) {
    const int slot = blockIdx.x >> 4;
    const int v = ((blockIdx.x & 15) << 8) + threadIdx.x;
    const int bx = block_coords[3 * (size_t)slot], by = block_coords[3 * (size_t)slot + 1], bz = block_coords[3 * (size_t)slot + 2];
    const int i = v & 15, j = (v >> 4) & 15, k = v >> 8;
    uint32_t c = 0;
    bool valid = true;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const long long g = voxel_ref(dom, index, slot, bx, by, bz, i + c_corner[q][0], j + c_corner[q][1], k + c_corner[q][2]);
        if (g < 0 || !(weight[g] > 0.f)) {
            valid = false;
            break;
        }
        c |= tsdf[g] < 0.f ? 1u << q : 0u;
    }
    cube[(size_t)slot * BV + v] = valid ? (uint16_t)c : (uint16_t)0xFFFF;
}

// the used-edge mask of voxel (i, j, k): bit a = the edge to the +a neighbour is crossed and a valid cube contains it
__device__ __forceinline__ uint32_t edge_mask(const Dom& dom, const int* __restrict__ index, int slot, int bx, int by, int bz, int i,
                                              int j, int k, const float* __restrict__ tsdf, const uint16_t* __restrict__ cube) {
    uint32_t mask = 0;
    const long long g0 = (long long)slot * BV + i + 16 * j + 256 * k;
    const float f0 = tsdf[g0];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        // the four cubes around the edge: origins at the voxel minus 0 / 1 along each of the two other axes
        const int b1 = a == 0 ? 1 : 0, b2 = a == 2 ? 1 : 2;
        bool any = false;
#pragma unroll
        for (int s = 0; s < 4; s++) {
            int o[3] = {0, 0, 0};
            o[b1] = -(s & 1);
            o[b2] = -(s >> 1);
            const long long g = voxel_ref(dom, index, slot, bx, by, bz, i + o[0], j + o[1], k + o[2]);
            any = any || (g >= 0 && cube[g] != 0xFFFF);
        }
        if (any) {  // a valid cube holds the edge: both ends exist with weight > 0
            const long long g1 = voxel_ref(dom, index, slot, bx, by, bz, i + (a == 0), j + (a == 1), k + (a == 2));
            if ((f0 < 0.f) != (tsdf[g1] < 0.f)) mask |= 1u << a;
        }
    }
    return mask;
}

__device__ __forceinline__ uint32_t popc(uint32_t x) { return (uint32_t)__popc(x); }

__global__ void __launch_bounds__(256) mesh_count_kernel(Dom dom, const int* __restrict__ index, const int* __restrict__ block_coords,
                                                         const float* __restrict__ tsdf, const uint16_t* __restrict__ cube,
                                                         uint32_t* __restrict__ vinfo, uint32_t* __restrict__ slot_cnt) {
    __shared__ uint32_t s_w[4];
    const int slot = blockIdx.x;
    const int bx = block_coords[3 * (size_t)slot], by = block_coords[3 * (size_t)slot + 1], bz = block_coords[3 * (size_t)slot + 2];
    const int j = threadIdx.x & 15, k = threadIdx.x >> 4;  // a thread owns the row of voxels (0..15, j, k)
    uint32_t nv = 0, nt = 0;
    const size_t row = (size_t)slot * BV + 16 * threadIdx.x;
    for (int i = 0; i < 16; i++) {
        const uint32_t m = edge_mask(dom, index, slot, bx, by, bz, i, j, k, tsdf, cube);
        vinfo[row + i] = m << VINFO_BITS;  // the mask, kept for the emit pass; the vertex id is added there
        nv += popc(m);
        const uint32_t c = cube[row + i];
        nt += c != 0xFFFF ? (uint32_t)ntri_of((int)c) : 0u;
    }
    uint32_t tot;
    gs2m_wg_exclusive_scan(nv | nt << 16, s_w, &tot);
    if (threadIdx.x == 0) slot_cnt[slot] = tot;
}

__global__ void __launch_bounds__(256) slot_scan_kernel(int n, const uint32_t* __restrict__ slot_cnt, uint32_t* __restrict__ pref_v,
                                                        uint32_t* __restrict__ pref_t, unsigned long long* __restrict__ totals) {
    __shared__ uint32_t s_w[4];
    unsigned long long cv = 0, ct = 0;
    for (int b = 0; b < n; b += 256) {
        const int i = b + (int)threadIdx.x;
        const uint32_t c = i < n ? slot_cnt[i] : 0u;
        uint32_t tv, tt;
        const uint32_t ev = gs2m_wg_exclusive_scan(c & 0xFFFFu, s_w, &tv);
        const uint32_t et = gs2m_wg_exclusive_scan(c >> 16, s_w, &tt);
        if (i < n) {
            pref_v[i] = (uint32_t)(cv + ev);  // meaningful while the totals stay below 2^32 (checked on the host)
            pref_t[i] = (uint32_t)(ct + et);
        }
        cv += tv;
        ct += tt;
    }
    if (threadIdx.x == 0) {
        totals[0] = cv;
        totals[1] = ct;
    }
}

__global__ void __launch_bounds__(256) emit_vertices_kernel(Dom dom, float voxel, float L, const int* __restrict__ index,
                                                            const int* __restrict__ block_coords, const float* __restrict__ tsdf,
                                                            const float* __restrict__ color_acc, const uint32_t* __restrict__ pref_v,
                                                            uint32_t* __restrict__ vinfo, float* __restrict__ vertices,
                                                            float* __restrict__ vcolors) {
    __shared__ uint32_t s_w[4];
    const int slot = blockIdx.x;
    const int bx = block_coords[3 * (size_t)slot], by = block_coords[3 * (size_t)slot + 1], bz = block_coords[3 * (size_t)slot + 2];
    const int j = threadIdx.x & 15, k = threadIdx.x >> 4;
    const size_t row = (size_t)slot * BV + 16 * threadIdx.x;
    uint32_t nv = 0;
    for (int i = 0; i < 16; i++) nv += popc(vinfo[row + i] >> VINFO_BITS);  // the masks mesh_count_kernel stored
    uint32_t tot;
    uint32_t id = pref_v[slot] + gs2m_wg_exclusive_scan(nv, s_w, &tot);
    const float cyz[2] = {voxel_centre(by, j, L, voxel), voxel_centre(bz, k, L, voxel)};
    for (int i = 0; i < 16; i++) {
        const long long g0 = (long long)(row + i);
        const uint32_t m = vinfo[g0] >> VINFO_BITS;
        vinfo[g0] = id | m << VINFO_BITS;
        if (!m) continue;
        const float p0[3] = {voxel_centre(bx, i, L, voxel), cyz[0], cyz[1]};
        const float f0 = tsdf[g0];
        for (int a = 0; a < 3; a++) {
            if (!(m >> a & 1u)) continue;
            // a used edge: its far end exists (a valid cube holds the edge)
            const long long g1 = voxel_ref(dom, index, slot, bx, by, bz, i + (a == 0), j + (a == 1), k + (a == 2));
            const float f1 = tsdf[g1];
            const float af0 = fabsf(f0);
            const float t = af0 / (af0 + fabsf(f1));
#pragma unroll
            for (int r = 0; r < 3; r++) vertices[3 * (size_t)id + r] = r == a ? p0[r] + t * voxel : p0[r];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float c0 = color_acc[((g0 / BV) * 3 + c) * BV + g0 % BV];
                const float c1 = color_acc[((g1 / BV) * 3 + c) * BV + g1 % BV];
                vcolors[3 * (size_t)id + c] = (c0 + t * (c1 - c0)) / 255.0f;
            }
            id++;
        }
    }
}

__global__ void __launch_bounds__(256) emit_triangles_kernel(Dom dom, const int* __restrict__ index, const int* __restrict__ block_coords,
                                                             const uint16_t* __restrict__ cube, const uint32_t* __restrict__ pref_t,
                                                             const uint32_t* __restrict__ vinfo, int* __restrict__ triangles) {
    __shared__ uint32_t s_w[4];
    const int slot = blockIdx.x;
    const int bx = block_coords[3 * (size_t)slot], by = block_coords[3 * (size_t)slot + 1], bz = block_coords[3 * (size_t)slot + 2];
    const int j = threadIdx.x & 15, k = threadIdx.x >> 4;
    const size_t row = (size_t)slot * BV + 16 * threadIdx.x;
    uint32_t nt = 0;
    for (int i = 0; i < 16; i++) {
        const uint32_t c = cube[row + i];
        nt += c != 0xFFFF ? (uint32_t)ntri_of((int)c) : 0u;
    }
    uint32_t tot;
    uint32_t t = pref_t[slot] + gs2m_wg_exclusive_scan(nt, s_w, &tot);
    for (int i = 0; i < 16; i++) {
        const uint32_t c = cube[row + i];
        if (c == 0xFFFF) continue;
        const signed char* tr = GS2M_MC_TRI[c];
        for (int e = 0; e < 15 && tr[e] >= 0; e++) {
            const int* ow = c_edge_owner[tr[e]];
            const long long g = voxel_ref(dom, index, slot, bx, by, bz, i + ow[0], j + ow[1], k + ow[2]);
            const uint32_t vi = vinfo[g];
            const uint32_t m = vi >> VINFO_BITS;
            triangles[3 * (size_t)t + e % 3] = (int)((vi & ((1u << VINFO_BITS) - 1u)) + popc(m & ((1u << ow[3]) - 1u)));
            if (e % 3 == 2) t++;
        }
    }
}

bool read_dom(const int* d, Dom* o) {
    if (!d) return false;
    *o = Dom{d[0], d[1], d[2], d[3], d[4], d[5]};
    return o->nx > 0 && o->ny > 0 && o->nz > 0;
}
Mat34 mat34(const float* m) {
    Mat34 r;
    for (int i = 0; i < 12; i++) r.m[i] = m[i];
    return r;
}
long long dom_blocks(const Dom& d) { return (long long)d.nx * d.ny * d.nz; }

}  // namespace

extern "C" {

int gs2m_tsdf_workspace_bytes(const int* dom, int n_blocks, long long* touch_bytes, long long* mesh_bytes) {
    Dom d;
    if (!read_dom(dom, &d) || n_blocks < 0) return GS2M_ERR_INVALID_ARG;
    if (touch_bytes) *touch_bytes = (long long)carve_touch(nullptr, dom_blocks(d)).bytes;
    if (mesh_bytes) *mesh_bytes = (long long)carve_mesh(nullptr, n_blocks).bytes;
    return GS2M_OK;
}

int gs2m_tsdf_points_aabb(int W, int H, const float* depth, float depth_trunc, float fx, float fy, float cx, float cy,
                          const float* c2w, int* aabb, void* stream) {
    if (W <= 0 || H <= 0 || !depth || !c2w || !aabb) return GS2M_ERR_INVALID_ARG;
    const int n = ((W + 3) / 4) * ((H + 3) / 4);
    points_aabb_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(W, H, depth, depth_trunc, fx, fy, cx, cy, mat34(c2w), aabb);
    return gs2m_status(hipGetLastError());
}

int gs2m_tsdf_touch(const int* dom, float voxel, float trunc, int W, int H, const float* depth, float depth_trunc, float fx,
                    float fy, float cx, float cy, const float* c2w, int capacity, int* state, int* index, int* block_coords,
                    int* touched_slots, void* touch_ws, int* info, void* stream) {
    Dom d;
    if (!read_dom(dom, &d) || W <= 0 || H <= 0 || !depth || !c2w || capacity < 0 || !state || !index || !block_coords ||
        !touched_slots || !touch_ws || !info || !(voxel > 0.f) || !(trunc > 0.f))
        return GS2M_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    const long long N = dom_blocks(d);
    const long long nch = (N + CHUNK - 1) / CHUNK;
    if (nch > INT_MAX) return GS2M_ERR_UNSUPPORTED;
    TouchWs w = carve_touch((char*)touch_ws, N);
    if (hipMemsetAsync(w.counters, 0, 8 * sizeof(int), s) != hipSuccess) return GS2M_ERR_HIP;
    const int n = ((W + 3) / 4) * ((H + 3) / 4);
    touch_kernel<<<(n + 255) / 256, 256, 0, s>>>(d, 16.0f * voxel, trunc, W, H, depth, depth_trunc, fx, fy, cx, cy, mat34(c2w),
                                                 w.flags, w.counters + 4);
    chunk_count_kernel<<<(unsigned)nch, 256, 0, s>>>(N, w.flags, index, w.chunk);
    chunk_scan_kernel<<<1, 256, 0, s>>>((int)nch, w.chunk, w.pref_t, w.pref_n, capacity, state, w.counters);
    chunk_assign_kernel<<<(unsigned)nch, 256, 0, s>>>(d, N, w.flags, index, w.pref_t, w.pref_n, w.counters, block_coords,
                                                      touched_slots);
    int cnt[8], st = 0;
    if (gs2m_read_back(s, {{cnt, w.counters, sizeof(cnt)}, {&st, state, sizeof(int)}}) != GS2M_OK) return GS2M_ERR_HIP;
    info[0] = cnt[3] ? st : cnt[5];
    info[1] = cnt[1];
    info[2] = cnt[0];
    info[3] = cnt[4];
    return cnt[3] ? GS2M_OK : GS2M_TSDF_POOL_FULL;
}

int gs2m_tsdf_integrate(float voxel, float trunc, int W, int H, const float* depth, const float* color, float depth_trunc,
                        float fx, float fy, float cx, float cy, const float* w2c, int n_touched, const int* touched_slots,
                        const int* block_coords, float* tsdf, float* weight, float* color_acc, void* stream) {
    if (W <= 0 || H <= 0 || !depth || !color || !w2c || n_touched < 0 || !touched_slots || !block_coords || !tsdf || !weight ||
        !color_acc || !(voxel > 0.f) || !(trunc > 0.f))
        return GS2M_ERR_INVALID_ARG;
    if (n_touched == 0) return GS2M_OK;
    if ((long long)n_touched * 16 > INT_MAX) return GS2M_ERR_UNSUPPORTED;
    integrate_kernel<<<n_touched * 16, 256, 0, (hipStream_t)stream>>>(voxel, 16.0f * voxel, trunc, W, H, depth, color, depth_trunc, fx,
                                                                      fy, cx, cy, mat34(w2c), touched_slots, block_coords, tsdf,
                                                                      weight, color_acc);
    return gs2m_status(hipGetLastError());
}

int gs2m_tsdf_mesh_count(const int* dom, int n_blocks, const int* index, const int* block_coords, const float* tsdf,
                         const float* weight, void* mesh_ws, long long* totals, void* stream) {
    Dom d;
    if (!read_dom(dom, &d) || n_blocks < 0 || !index || !block_coords || !tsdf || !weight || !mesh_ws || !totals)
        return GS2M_ERR_INVALID_ARG;
    totals[0] = totals[1] = 0;
    if (n_blocks == 0) return GS2M_OK;
    if ((long long)n_blocks * 16 > INT_MAX) return GS2M_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    MeshWs w = carve_mesh((char*)mesh_ws, n_blocks);
    cube_case_kernel<<<n_blocks * 16, 256, 0, s>>>(d, index, block_coords, tsdf, weight, w.cube);
    mesh_count_kernel<<<n_blocks, 256, 0, s>>>(d, index, block_coords, tsdf, w.cube, w.vinfo, w.slot_cnt);
    slot_scan_kernel<<<1, 256, 0, s>>>(n_blocks, w.slot_cnt, w.pref_v, w.pref_t, w.totals);
    u64 t[2];
    if (gs2m_read_back(s, {{t, w.totals, sizeof(t)}}) != GS2M_OK) return GS2M_ERR_HIP;
    totals[0] = (long long)t[0];
    totals[1] = (long long)t[1];
    if (t[0] >= (1ull << VINFO_BITS) || t[1] >= (1ull << 31)) return GS2M_ERR_UNSUPPORTED;
    return GS2M_OK;
}

int gs2m_tsdf_mesh_emit(const int* dom, float voxel, int n_blocks, const int* index, const int* block_coords,
                        const float* tsdf, const float* color_acc, void* mesh_ws, long long n_vertices, long long n_triangles,
                        float* vertices, float* vertex_colors, int* triangles, void* stream) {
    Dom d;
    if (!read_dom(dom, &d) || n_blocks < 0 || !index || !block_coords || !tsdf || !color_acc || !mesh_ws || n_vertices < 0 ||
        n_triangles < 0 || !(voxel > 0.f))
        return GS2M_ERR_INVALID_ARG;
    if (n_blocks == 0 || (n_vertices == 0 && n_triangles == 0)) return GS2M_OK;
    if (!vertices || !vertex_colors || !triangles) return GS2M_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    MeshWs w = carve_mesh((char*)mesh_ws, n_blocks);
    emit_vertices_kernel<<<n_blocks, 256, 0, s>>>(d, voxel, 16.0f * voxel, index, block_coords, tsdf, color_acc, w.pref_v, w.vinfo,
                                                  vertices, vertex_colors);
    emit_triangles_kernel<<<n_blocks, 256, 0, s>>>(d, index, block_coords, w.cube, w.pref_t, w.vinfo, triangles);
    return gs2m_status(hipGetLastError());
}

int gs2m_tsdf_block_coords(int n_blocks, const int* block_coords, int* host_coords, void* stream) {
    if (n_blocks < 0 || (n_blocks > 0 && (!block_coords || !host_coords))) return GS2M_ERR_INVALID_ARG;
    if (n_blocks == 0) return GS2M_OK;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(host_coords, block_coords, 3 * sizeof(int) * (size_t)n_blocks, hipMemcpyDeviceToHost, s) != hipSuccess)
        return GS2M_ERR_HIP;
    return gs2m_status(hipStreamSynchronize(s));
}

}  // extern "C"
