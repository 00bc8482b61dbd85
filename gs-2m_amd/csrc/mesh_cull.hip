// DTU mask culling: disk dilation of the object masks, the per-vertex view test and the triangle renumbering
// (include/gs2m_eval.h; the contract: DESIGN.md §10 "Mask culling").
//
// Dilation, exact and separable: dil[y, x] = any (dx, dy) with dx^2 + dy^2 <= r^2 and a foreground pixel at (y + dy, x + dx).
//   pass 1  g[y, x] = distance to the nearest foreground pixel of column x, capped at r + 1 (two running scans, down and up)
//   pass 2  dil[y, x] = any dx in [-r, r] with g[y, x + dx] <= lim[dx], lim[dx] = floor(sqrt(r^2 - dx^2))
// Both passes run in one kernel: a workgroup owns 64 x DIL_TH output pixels; a thread per column of the tile and its r-wide
// apron makes pass 1 (the column's bits are kept per row as a 64-lane ballot for the scan back up), g lies in LDS as bytes and
// pass 2 takes 2r + 1 byte taps out of it.  A wave is 64 consecutive pixels of a row: its ballot is the packed word.
// Vertex test: one thread per vertex, the views' matrices staged in LDS, the loop left at the first failing view.
// Triangles: exclusive scans of the vertex flags and of the kept faces (gs2m_scan_u64), then the kept faces with their new ids.
// Integer work and fp32 evaluated as written (-ffp-contract=off): two runs are bitwise identical.
#include <math.h>
#include "eval_common.h"
#include "../../include/gs2m_eval.h"

namespace {

constexpr int DIL_RMAX = 64;
constexpr int DIL_TH = 64;                    // rows of a tile (16 per wave)
constexpr int DIL_CW = 64 + 2 * DIL_RMAX;     // columns of a tile with its apron, at most
constexpr int DIL_ROWS = DIL_TH + 2 * DIL_RMAX;
constexpr int VIEW_CHUNK = 256;               // views staged in LDS at a time (12 floats each)

__global__ void __launch_bounds__(256) dilate_kernel(int H, int W, const unsigned char* __restrict__ masks, int r, int stride,
                                                     u64* __restrict__ packed) {
    __shared__ unsigned char s_g[DIL_TH][DIL_CW];
    __shared__ u64 s_bits[DIL_ROWS][DIL_CW / 64];
    __shared__ unsigned char s_lim[2 * DIL_RMAX + 1];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int x0 = blockIdx.x * 64, y0 = blockIdx.y * DIL_TH;
    const int rows = min(DIL_TH, H - y0);  // >= 1
    const int cw = 64 + 2 * r;
    const unsigned char* m = masks + (size_t)blockIdx.z * H * W;
    if (tid <= 2 * r) {
        const int dx = tid - r, room = r * r - dx * dx;
        int t = 0;
        while ((t + 1) * (t + 1) <= room) t++;
        s_lim[tid] = (unsigned char)t;
    }
    // pass 1: the waves that hold a column of the tile; lanes past the last column take part in the ballots with no pixel
    const int x = x0 - r + tid;
    const bool col = tid < cw && x >= 0 && x < W;
    const int ys = y0 - r, ye = y0 + rows + r;  // rows [ys, ye) can reach the tile
    if (w * 64 < cw) {
        int last = ys - r - 2;  // no foreground seen: further than the cap
        for (int y = ys; y < y0 + rows; y++) {
            const bool fg = col && y >= 0 && y < H && m[(size_t)y * W + x] != 0;
            const u64 b = __ballot(fg);
            if (lane == 0) s_bits[y - ys][w] = b;
            if (fg) last = y;
            if (y >= y0 && tid < cw) s_g[y - y0][tid] = (unsigned char)min(y - last, r + 1);
        }
    }
    __syncthreads();
    if (w * 64 < cw) {
        int next = ye + r + 1;
        for (int y = ye - 1; y >= y0; y--) {
            bool fg;
            if (y >= y0 + rows) fg = col && y < H && m[(size_t)y * W + x] != 0;  // below the tile: not read yet (y >= 0 here)
            else fg = (s_bits[y - ys][w] >> lane) & 1;                          // this wave's own ballot of the way down
            if (fg) next = y;
            if (y < y0 + rows && tid < cw) s_g[y - y0][tid] = (unsigned char)min((int)s_g[y - y0][tid], min(next - y, r + 1));
        }
    }
    __syncthreads();
    // pass 2: wave w takes the rows w, w + 4, ...; lane = pixel of the word
    u64* out = packed + ((size_t)blockIdx.z * H + y0) * stride + blockIdx.x;
    for (int row = w; row < rows; row += 4) {
        const unsigned char* g = &s_g[row][lane];  // g[k]: the column at dx = k - r
        bool hit = false;
        for (int k = 0; k <= 2 * r; k++) hit |= g[k] <= s_lim[k];
        const u64 word = __ballot(hit && x0 + lane < W);
        if (lane == 0) out[(size_t)row * stride] = word;
    }
}

// ---- vertex test ----

__global__ void __launch_bounds__(256) cull_flags_kernel(long long n, const double* __restrict__ verts, int n_views,
                                                         const float* __restrict__ M, int H, int W, int stride,
                                                         const u64* __restrict__ packed, float wn1, float hn1,
                                                         unsigned char* __restrict__ keep) {
    __shared__ float s_m[VIEW_CHUNK][12];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    float x = 0.f, y = 0.f, z = 0.f;
    if (i < n) {
        x = (float)verts[3 * i];
        y = (float)verts[3 * i + 1];
        z = (float)verts[3 * i + 2];
    }
    bool ok = true;
    const float w1 = (float)(W - 1), h1 = (float)(H - 1);
    for (int v0 = 0; v0 < n_views; v0 += VIEW_CHUNK) {
        const int nv = min(VIEW_CHUNK, n_views - v0);
        __syncthreads();
        for (int k = threadIdx.x; k < nv * 12; k += 256) s_m[k / 12][k % 12] = M[(size_t)(v0 + k / 12) * 16 + k % 12];
        __syncthreads();
        if (i >= n) continue;
        for (int v = 0; v < nv && ok; v++) {
            const float* a = s_m[v];
            const float c0 = ((a[0] * x + a[1] * y) + a[2] * z) + a[3];
            const float c1 = ((a[4] * x + a[5] * y) + a[6] * z) + a[7];
            const float c2 = ((a[8] * x + a[9] * y) + a[10] * z) + a[11];
            const float d = c2 + 1e-6f;
            const float px = c0 / d, py = c1 / d;
            const float nx = (px / wn1 - 0.5f) * 2.f, ny = (py / hn1 - 0.5f) * 2.f;
            const bool valid = nx > -1.f && nx < 1.f && ny > -1.f && ny < 1.f;  // false for NaN
            if (!valid) continue;
            const float fx = rintf(((nx + 1.f) / 2.f) * w1), fy = rintf(((ny + 1.f) / 2.f) * h1);  // half to even
            bool sample = false;
            if (fx >= 0.f && fx < (float)W && fy >= 0.f && fy < (float)H) {
                const int ix = (int)fx, iy = (int)fy;
                sample = (packed[((size_t)(v0 + v) * H + iy) * stride + (ix >> 6)] >> (ix & 63)) & 1;
            }
            ok = sample;
        }
    }
    if (i < n) keep[i] = ok ? 1 : 0;
}

// ---- triangles ----

__global__ void __launch_bounds__(256) keep_count_kernel(long long n, const unsigned char* __restrict__ keep, u64* __restrict__ a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] = keep[i] & 1;
}

__global__ void __launch_bounds__(256) face_count_kernel(long long nv, const unsigned char* __restrict__ keep, long long nt,
                                                         const int* __restrict__ tris, u64* __restrict__ a, int* __restrict__ err) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const int p = tris[3 * t], q = tris[3 * t + 1], s = tris[3 * t + 2];
    a[t] = tri_in_range(p, q, s, nv, err) && (keep[p] & keep[q] & keep[s] & 1) ? 1 : 0;
}

// va, fa: the exclusive scans (n + 1 entries each); a kept face is one whose count was 1, so all three ids are in range
__global__ void __launch_bounds__(256) face_emit_kernel(long long nt, const int* __restrict__ tris, const u64* __restrict__ va,
                                                        const u64* __restrict__ fa, int* __restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const u64 o = fa[t];
    if (fa[t + 1] == o) return;
#pragma unroll
    for (int k = 0; k < 3; k++) out[3 * o + k] = (int)va[tris[3 * t + k]];
}

struct CullWs {
    u64* va;     // n_verts + 1
    u64* vbsum;  // scan_blocks(n_verts) + 1
    u64* fa;     // n_tris + 1
    u64* fbsum;  // scan_blocks(n_tris) + 1
    int* err;    // 1: a vertex index out of range
    size_t bytes;
};
CullWs carve_cull(char* base, long long nv, long long nt) {
    Carver c{base, 0};
    CullWs w;
    w.va = c.take<u64>(nv + 1);
    w.vbsum = c.take<u64>(gs2m_scan_blocks(nv) + 1);
    w.fa = c.take<u64>(nt + 1);
    w.fbsum = c.take<u64>(gs2m_scan_blocks(nt) + 1);
    w.err = c.take<int>(1);
    w.bytes = c.off;
    return w;
}

bool mask_dims_ok(int n_views, int H, int W) {
    // the grid's y and z extents, and 32-bit pixel indices within a view
    return n_views >= 0 && H >= 1 && W >= 1 && n_views <= 65535 && (H + DIL_TH - 1) / DIL_TH <= 65535 && (long long)H * W <= 0x7FFFFFFFll;
}

}  // namespace

extern "C" {

int gs2m_eval_dilate_bytes(int n_views, int H, int W, long long* bytes) {
    if (!mask_dims_ok(n_views, H, W) || !bytes) return GS2M_ERR_INVALID_ARG;
    *bytes = (long long)n_views * H * ((W + 63) / 64) * 8;
    return GS2M_OK;
}

int gs2m_eval_dilate_disk(int n_views, int H, int W, const unsigned char* masks, int r, void* packed, void* stream) {
    if (!mask_dims_ok(n_views, H, W) || r < 0 || r > DIL_RMAX || (n_views > 0 && (!masks || !packed))) return GS2M_ERR_INVALID_ARG;
    if (n_views == 0) return GS2M_OK;
    const int stride = (W + 63) / 64;
    const dim3 grid((unsigned)stride, (unsigned)((H + DIL_TH - 1) / DIL_TH), (unsigned)n_views);
    dilate_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(H, W, masks, r, stride, (u64*)packed);
    return gs2m_status(hipGetLastError());
}

int gs2m_eval_cull_flags(long long n, const double* verts, int n_views, const float* view_mats, int H, int W, const void* packed,
                         int Wn, int Hn, unsigned char* keep, void* stream) {
    if (n < 0 || n_views < 0 || Wn < 1 || Hn < 1 || (n > 0 && (!verts || !keep))) return GS2M_ERR_INVALID_ARG;
    if (n_views > 0 && (!mask_dims_ok(n_views, H, W) || !view_mats || !packed)) return GS2M_ERR_INVALID_ARG;
    if (n == 0) return GS2M_OK;
    if (n > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;
    cull_flags_kernel<<<blocks_of(n), 256, 0, (hipStream_t)stream>>>(n, verts, n_views, view_mats, H, W, (W + 63) / 64,
                                                                     (const u64*)packed, (float)(Wn - 1), (float)(Hn - 1), keep);
    return gs2m_status(hipGetLastError());
}

int gs2m_eval_cull_workspace_bytes(long long n_verts, long long n_tris, long long* bytes) {
    if (n_verts < 0 || n_tris < 0 || !bytes) return GS2M_ERR_INVALID_ARG;
    *bytes = (long long)carve_cull(nullptr, n_verts, n_tris).bytes;
    return GS2M_OK;
}

int gs2m_eval_cull_triangles(long long n_verts, const unsigned char* keep, long long n_tris, const int* tris, void* ws,
                             int* out_tris, long long* host_totals, void* stream) {
    if (n_verts < 0 || n_tris < 0 || !ws || !host_totals || (n_verts > 0 && !keep) || (n_tris > 0 && (!tris || !out_tris)))
        return GS2M_ERR_INVALID_ARG;
    if (n_verts > 0x7FFFFFFFll || n_tris > MAX_LAUNCH) return GS2M_ERR_UNSUPPORTED;  // ids are int
    hipStream_t s = (hipStream_t)stream;
    const CullWs w = carve_cull((char*)ws, n_verts, n_tris);
    if (hipMemsetAsync(w.err, 0, sizeof(int), s) != hipSuccess) return GS2M_ERR_HIP;
    if (n_verts > 0) keep_count_kernel<<<blocks_of(n_verts), 256, 0, s>>>(n_verts, keep, w.va);
    if (hipGetLastError() != hipSuccess || gs2m_scan_u64(w.va, n_verts, w.vbsum, s) != hipSuccess) return GS2M_ERR_HIP;
    if (n_tris > 0) face_count_kernel<<<blocks_of(n_tris), 256, 0, s>>>(n_verts, keep, n_tris, tris, w.fa, w.err);
    if (hipGetLastError() != hipSuccess || gs2m_scan_u64(w.fa, n_tris, w.fbsum, s) != hipSuccess) return GS2M_ERR_HIP;
    if (n_tris > 0) face_emit_kernel<<<blocks_of(n_tris), 256, 0, s>>>(n_tris, tris, w.va, w.fa, out_tris);
    int err;
    u64 tv, tf;
    if (gs2m_read_back(s, {{&err, w.err, sizeof(err)}, {&tv, w.va + n_verts, 8}, {&tf, w.fa + n_tris, 8}}) != GS2M_OK) return GS2M_ERR_HIP;
    if (err) return GS2M_ERR_INVALID_ARG;
    host_totals[0] = (long long)tv;
    host_totals[1] = (long long)tf;
    return GS2M_OK;
}

}  // extern "C"
