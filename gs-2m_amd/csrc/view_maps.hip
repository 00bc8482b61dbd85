// Per-view map images for gfx950: render.py's depth, normal and BRDF images formed on the device as the 8-bit arrays that are
// stored (include/gs2m_maps.h).  Three entry points:
//   gs2m_order_stats     exact order statistics of an fp32 array by radix select (np.percentile's np.partition)
//   gs2m_depth_colorize  save_depth_map: percentile clip, normalisation and matplotlib's magma table, all fp32
//   gs2m_pack_image      save_image's rounding / map_to_rgba's truncation of every other map, with the normal transform,
//                        the sRGB transfer and the mask composition render.py applies in front of them
//
// The select: four passes over the array, most significant byte of the order-preserving key first.  In a pass every rank
// has a prefix (the key bytes found so far) and a remaining rank among the elements with that prefix; ranks with the same
// prefix form a group with one histogram, kept by the group's first rank (its "leader").  os_hist_kernel counts, per group,
// the next byte of every element that carries the group's prefix: in LDS per workgroup, then one integer atomic per non-empty
// bin into the workspace.  Depth maps are full of ties (a masked map is half zeros), and 64 lanes adding to one LDS word take
// 64 turns, so a wave whose matching lanes all hold the same byte adds their count once.  os_narrow_kernel (one workgroup)
// scans each rank's histogram, finds the bin that holds the rank, appends it to the prefix and recomputes the groups; after the
// last pass the prefix IS the key.  Integer counts only: the result does not depend on the order of the atomics.
#include "common.h"
#include "../../include/gs2m_maps.h"
#include "view_maps_magma.h"

namespace {

constexpr int OS_K = GS2M_MAPS_MAX_RANKS;
constexpr int OS_THREADS = 256;
constexpr int OS_HIST_WORDS = 4 * OS_K * 256;  // [pass][rank][bin]
// workspace, in 32-bit words: the histograms, then prefix[8], rem[8], leader[8], nonfinite, 7 words of padding
constexpr int OS_PREFIX = OS_HIST_WORDS, OS_REM = OS_PREFIX + OS_K, OS_LEADER = OS_REM + OS_K, OS_NONFINITE = OS_LEADER + OS_K;
constexpr int OS_WORDS = OS_NONFINITE + 8;

struct OsRanks {
    uint32_t r[OS_K];
};

// the float's place in a sort as an unsigned integer; every NaN last
__device__ __forceinline__ uint32_t os_key(uint32_t bits) {
    if ((bits & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
__device__ __forceinline__ uint32_t os_unkey(uint32_t key) { return (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key; }

__global__ void __launch_bounds__(OS_THREADS) os_init_kernel(int k, OsRanks ranks, uint32_t* __restrict__ ws) {
    const int i = blockIdx.x * OS_THREADS + threadIdx.x;
    if (i >= OS_WORDS) return;
    uint32_t v = 0u;  // histograms, prefixes, leaders (every rank starts in rank 0's group: the empty prefix), the count
    if (i >= OS_REM && i < OS_REM + k) v = ranks.r[i - OS_REM];
    ws[i] = v;
}

__global__ void __launch_bounds__(OS_THREADS) os_hist_kernel(const float* __restrict__ x, uint32_t n, int k, int pass,
                                                             uint32_t* __restrict__ ws) {
    __shared__ uint32_t s_h[OS_K * 256];
    __shared__ uint32_t s_nf;
    const int tid = threadIdx.x, lane = tid & 63;
    const int shift = 24 - 8 * pass;
    const uint32_t himask = pass == 0 ? 0u : 0xFFFFFFFFu << (shift + 8);
    // the groups: their leaders' rank indices and prefixes
    __shared__ int s_nl, s_lead[OS_K];
    __shared__ uint32_t s_pre[OS_K];
    if (tid == 0) {
        int c = 0;
        for (int r = 0; r < k; r++)
            if (ws[OS_LEADER + r] == (uint32_t)r) {
                s_lead[c] = r;
                s_pre[c] = ws[OS_PREFIX + r];
                c++;
            }
        s_nl = c;
        s_nf = 0u;
    }
    for (int i = tid; i < OS_K * 256; i += OS_THREADS) s_h[i] = 0u;
    gs2m_sync();
    const int nl = s_nl;

    const size_t step = (size_t)gridDim.x * OS_THREADS;
    for (size_t base = (size_t)blockIdx.x * OS_THREADS; base < n; base += step) {  // workgroup-uniform trip count
        const size_t i = base + tid;
        const bool valid = i < n;
        const uint32_t bits = valid ? f2u(x[i]) : 0u;
        const uint32_t key = os_key(bits);
        const uint32_t d = (key >> shift) & 255u;
        if (pass == 0) {
            const unsigned long long nf = __ballot(valid && (bits & 0x7F800000u) == 0x7F800000u);
            if (nf != 0ull && lane == 0) atomicAdd(&s_nf, (uint32_t)__popcll(nf));
        }
        for (int j = 0; j < nl; j++) {
            const bool m = valid && (key & himask) == s_pre[j];
            const unsigned long long b = __ballot(m);
            if (b == 0ull) continue;  // wave-uniform
            const int first = __ffsll((long long)b) - 1;
            const uint32_t d0 = (uint32_t)__shfl((int)d, first, 64);
            if (__ballot(m && d == d0) == b) {  // one byte in the whole wave: one add
                if (lane == first) atomicAdd(&s_h[j * 256 + d0], (uint32_t)__popcll(b));
            } else if (m) {
                atomicAdd(&s_h[j * 256 + d], 1u);
            }
        }
    }
    gs2m_sync();
    uint32_t* __restrict__ g = ws + (size_t)pass * OS_K * 256;
    for (int i = tid; i < nl * 256; i += OS_THREADS) {
        const uint32_t c = s_h[i];
        if (c != 0u) atomicAdd(&g[s_lead[i >> 8] * 256 + (i & 255)], c);
    }
    if (pass == 0 && tid == 0 && s_nf != 0u) atomicAdd(&ws[OS_NONFINITE], s_nf);
}

// one workgroup of 256: thread t holds bin t
__global__ void __launch_bounds__(OS_THREADS) os_narrow_kernel(int k, int pass, uint32_t* __restrict__ ws, float* __restrict__ out,
                                                               long long* __restrict__ nonfinite) {
    __shared__ uint32_t s_w[4];
    __shared__ uint32_t s_pre[OS_K], s_rem[OS_K], s_lead[OS_K], s_npre[OS_K], s_nrem[OS_K];
    const int tid = threadIdx.x;
    const int shift = 24 - 8 * pass;
    if (tid < k) {
        s_pre[tid] = ws[OS_PREFIX + tid];
        s_rem[tid] = ws[OS_REM + tid];
        s_lead[tid] = ws[OS_LEADER + tid];
        s_npre[tid] = s_pre[tid];
        s_nrem[tid] = s_rem[tid];
    }
    gs2m_sync();
    const uint32_t* __restrict__ g = ws + (size_t)pass * OS_K * 256;
    for (int r = 0; r < k; r++) {
        const uint32_t c = g[s_lead[r] * 256 + tid];
        uint32_t total;
        const uint32_t excl = gs2m_wg_exclusive_scan(c, s_w, &total);
        const uint32_t rem = s_rem[r];
        if (c != 0u && rem >= excl && rem - excl < c) {  // exactly one bin: rem < total = the elements under this prefix
            s_npre[r] = s_pre[r] | ((uint32_t)tid << shift);
            s_nrem[r] = rem - excl;
        }
    }
    gs2m_sync();
    if (tid < k) {
        const uint32_t p = s_npre[tid];
        int leader = tid;
        for (int q = tid - 1; q >= 0; q--)
            if (s_npre[q] == p) leader = q;
        ws[OS_PREFIX + tid] = p;
        ws[OS_REM + tid] = s_nrem[tid];
        ws[OS_LEADER + tid] = (uint32_t)leader;
        if (pass == 3) out[tid] = u2f(os_unkey(p));
    }
    if (pass == 3 && tid == 0) *nonfinite = (long long)ws[OS_NONFINITE];
}

// ---- depth image ---------------------------------------------------------------------------------------------------------
__device__ __constant__ const uint32_t MAGMA[256] = GS2M_MAGMA_WORDS;

// numpy's _lerp in fp32, as written (the library is built with -ffp-contract=off)
__device__ __forceinline__ float np_lerp(float a, float b, float t) {
    const float d = b - a;
    return t >= 0.5f ? b - d * (1.0f - t) : a + d * t;
}

__global__ void __launch_bounds__(256) depth_colorize_kernel(uint32_t n, const float* __restrict__ depth, const float* __restrict__ stats,
                                                             float t_lo, float t_hi, uint32_t* __restrict__ rgba) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float lo = np_lerp(stats[0], stats[1], t_lo), hi = np_lerp(stats[2], stats[3], t_hi);
    const float c = fminf(fmaxf(depth[i], lo), hi);
    const float x = (c - lo) / (hi - lo + 1e-8f);
    const float s = x * 256.0f;
    const int idx = s >= 255.0f ? 255 : (s > 0.0f ? (int)s : 0);
    rgba[i] = MAGMA[idx];
}

// ---- image packing -------------------------------------------------------------------------------------------------------
struct PackArgs {
    uint32_t n;  // pixels
    int C, layout, flags, out_channels;
    const float *src, *alpha, *mask, *bg, *rot;
    uint8_t* out;
};

__device__ __forceinline__ uint32_t pack_trunc(float v) { return (uint32_t)fminf(fmaxf(v * 255.0f, 0.0f), 255.0f); }
__device__ __forceinline__ uint32_t pack_round(float v) {
    return (uint32_t)fminf(fmaxf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f + 0.5f, 0.0f), 255.0f);
}

// pixel p as r | g << 8 | b << 16 | a << 24
__device__ __forceinline__ uint32_t pack_pixel(const PackArgs& a, size_t p) {
    float v[3];
    if (a.C == 1) {
        v[0] = v[1] = v[2] = a.src[p];
    } else if (a.layout == GS2M_PACK_CHW) {
        v[0] = a.src[p]; v[1] = a.src[(size_t)a.n + p]; v[2] = a.src[2 * (size_t)a.n + p];
    } else {
        v[0] = a.src[3 * p]; v[1] = a.src[3 * p + 1]; v[2] = a.src[3 * p + 2];
    }
    if (a.flags & GS2M_PACK_NORMAL) {
        const float len = fmaxf(sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), 1e-12f);
        float x = v[0] / len, y = v[1] / len, z = v[2] / len;
        if (a.rot) {
            const float* R = a.rot;
            const float rx = x * R[0] + y * R[3] + z * R[6], ry = x * R[1] + y * R[4] + z * R[7], rz = x * R[2] + y * R[5] + z * R[8];
            x = rx; y = -ry; z = -rz;
        }
        v[0] = x * 0.5f + 0.5f; v[1] = y * 0.5f + 0.5f; v[2] = z * 0.5f + 0.5f;
    }
    if (a.flags & GS2M_PACK_SRGB) {
#pragma unroll
        for (int c = 0; c < 3; c++)
            v[c] = v[c] <= 0.0031308f ? 12.92f * v[c] : (211.0f * powf(fmaxf(v[c], 1.1920928955078125e-07f), (float)(5.0 / 12.0)) - 11.0f) / 200.0f;
    }
    if (a.mask) {
        const bool in = a.mask[p] > 0.5f;
#pragma unroll
        for (int c = 0; c < 3; c++) v[c] = in ? fminf(fmaxf(v[c], 0.0f), 1.0f) : a.bg[c];
    }
    uint32_t w = 0xFF000000u;
    if (a.alpha) w = pack_trunc(a.alpha[p]) << 24;
#pragma unroll
    for (int c = 0; c < 3; c++) w |= ((a.flags & GS2M_PACK_TRUNC) ? pack_trunc(v[c]) : pack_round(v[c])) << (8 * c);
    return w;
}

// WORDS: the output is 4-byte aligned.  RGBA: a thread per pixel.  RGB: a thread per four pixels = three words; the last
// group of an image whose pixel count is no multiple of four, and every group of an unaligned output, goes out as bytes.
template <bool WORDS>
__global__ void __launch_bounds__(256) pack_image_kernel(PackArgs a) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (a.out_channels == 4) {
        if (t >= a.n) return;
        const uint32_t w = pack_pixel(a, t);
        if (WORDS) {
            reinterpret_cast<uint32_t*>(a.out)[t] = w;
        } else {
#pragma unroll
            for (int c = 0; c < 4; c++) a.out[4 * t + c] = (uint8_t)(w >> (8 * c));
        }
        return;
    }
    const size_t p0 = 4 * t;
    if (p0 >= a.n) return;
    if (WORDS && p0 + 4 <= a.n) {
        const uint32_t w0 = pack_pixel(a, p0) & 0xFFFFFFu, w1 = pack_pixel(a, p0 + 1) & 0xFFFFFFu;
        const uint32_t w2 = pack_pixel(a, p0 + 2) & 0xFFFFFFu, w3 = pack_pixel(a, p0 + 3) & 0xFFFFFFu;
        uint32_t* o = reinterpret_cast<uint32_t*>(a.out) + 3 * t;  // byte 12 t
        o[0] = w0 | (w1 << 24);
        o[1] = (w1 >> 8) | (w2 << 16);
        o[2] = (w2 >> 16) | (w3 << 8);
        return;
    }
    for (size_t p = p0; p < a.n && p < p0 + 4; p++) {
        const uint32_t w = pack_pixel(a, p);
        a.out[3 * p] = (uint8_t)w; a.out[3 * p + 1] = (uint8_t)(w >> 8); a.out[3 * p + 2] = (uint8_t)(w >> 16);
    }
}

bool maps_pixels(int H, int W, uint32_t* n) {
    if (H < 1 || W < 1 || (long long)H * W > 0x7FFFFFFFll) return false;
    *n = (uint32_t)((long long)H * W);
    return true;
}

}  // namespace

extern "C" int gs2m_order_stats_workspace_bytes(long long n, int k, long long* bytes) {
    if (!bytes || n < 1 || n > 0x7FFFFFFFll || k < 1 || k > OS_K) return GS2M_ERR_INVALID_ARG;
    *bytes = 4ll * OS_WORDS;
    return GS2M_OK;
}

extern "C" int gs2m_order_stats(long long n, const float* x, int k, const long long* ranks, void* ws, long long ws_bytes, float* out,
                                long long* nonfinite, void* stream) {
    if (!x || !ranks || !ws || !out || !nonfinite || n < 1 || n > 0x7FFFFFFFll || k < 1 || k > OS_K) return GS2M_ERR_INVALID_ARG;
    if (ws_bytes < 4ll * OS_WORDS || ((uintptr_t)ws & 7u) != 0) return GS2M_ERR_INVALID_ARG;
    OsRanks r = {};
    for (int j = 0; j < k; j++) {
        if (ranks[j] < 0 || ranks[j] >= n) return GS2M_ERR_INVALID_ARG;
        r.r[j] = (uint32_t)ranks[j];
    }
    hipStream_t s = (hipStream_t)stream;
    uint32_t* w = reinterpret_cast<uint32_t*>(ws);
    // 1024 elements per workgroup and pass at least, 1024 workgroups at most (4 per CU): 1200 x 1600 is 8 rounds of each
    const unsigned blocks = (unsigned)((n + 1023) / 1024 < 1024 ? (n + 1023) / 1024 : 1024);
    os_init_kernel<<<(OS_WORDS + OS_THREADS - 1) / OS_THREADS, OS_THREADS, 0, s>>>(k, r, w);
    for (int pass = 0; pass < 4; pass++) {
        os_hist_kernel<<<blocks, OS_THREADS, 0, s>>>(x, (uint32_t)n, k, pass, w);
        os_narrow_kernel<<<1, OS_THREADS, 0, s>>>(k, pass, w, out, nonfinite);
    }
    return hipGetLastError() == hipSuccess ? GS2M_OK : GS2M_ERR_HIP;
}

extern "C" int gs2m_depth_colorize(int H, int W, const float* depth, const float* stats, float t_lo, float t_hi, unsigned char* rgba,
                                   void* stream) {
    uint32_t n;
    if (!depth || !stats || !rgba || !maps_pixels(H, W, &n) || ((uintptr_t)rgba & 3u) != 0) return GS2M_ERR_INVALID_ARG;
    if (!(t_lo >= 0.0f && t_lo <= 1.0f && t_hi >= 0.0f && t_hi <= 1.0f)) return GS2M_ERR_INVALID_ARG;
    depth_colorize_kernel<<<(n + 255u) / 256u, 256, 0, (hipStream_t)stream>>>(n, depth, stats, t_lo, t_hi, reinterpret_cast<uint32_t*>(rgba));
    return hipGetLastError() == hipSuccess ? GS2M_OK : GS2M_ERR_HIP;
}

extern "C" int gs2m_pack_image(int H, int W, int C, int layout, const float* src, const float* alpha, const float* mask, const float* bg,
                               const float* rot, int flags, int out_channels, unsigned char* out, void* stream) {
    PackArgs a;
    if (!src || !out || !maps_pixels(H, W, &a.n)) return GS2M_ERR_INVALID_ARG;
    if ((C != 1 && C != 3) || (layout != GS2M_PACK_CHW && layout != GS2M_PACK_HWC) || (out_channels != 3 && out_channels != 4))
        return GS2M_ERR_INVALID_ARG;
    if ((flags & ~(GS2M_PACK_TRUNC | GS2M_PACK_SRGB | GS2M_PACK_NORMAL)) != 0) return GS2M_ERR_INVALID_ARG;
    if (((flags & GS2M_PACK_NORMAL) && C != 3) || (rot && !(flags & GS2M_PACK_NORMAL)) || (mask && !bg) || (alpha && out_channels != 4))
        return GS2M_ERR_INVALID_ARG;
    a.C = C; a.layout = layout; a.flags = flags; a.out_channels = out_channels;
    a.src = src; a.alpha = alpha; a.mask = mask; a.bg = bg; a.rot = rot; a.out = out;
    const uint32_t threads = out_channels == 4 ? a.n : (a.n + 3u) / 4u;
    const unsigned blocks = (threads + 255u) / 256u;
    if (((uintptr_t)out & 3u) == 0)
        pack_image_kernel<true><<<blocks, 256, 0, (hipStream_t)stream>>>(a);
    else
        pack_image_kernel<false><<<blocks, 256, 0, (hipStream_t)stream>>>(a);
    return hipGetLastError() == hipSuccess ? GS2M_OK : GS2M_ERR_HIP;
}
