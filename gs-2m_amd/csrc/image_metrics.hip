// Image metrics of 8-bit image pairs for gfx950: the exact sum of squared differences (PSNR) and the sum of the SSIM map, in
// ONE pass over the input (metrics.py's two scores; include/gs2m_metrics.h).
//
// The images stay interleaved (H, W, CH) as they are decoded.  A row is a flat run of E = CH W bytes in which the horizontal
// taps of an element lie CH bytes apart, and "tap outside [0, W)" is "byte outside [0, E)", so one kernel serves CH = 1 and 3.
// A workgroup of 64 CH threads (CH waves) owns a tile of 64 pixels x 32 rows and walks down its rows with the shared walk of
// window11.h: per input row it stages the 64 CH + 10 CH bytes of both images in LDS, every thread forms the five horizontal sums
// (a, a^2, b, b^2, ab) of its element and the walk's register ring does the vertical pass; the row that completes is evaluated
// to its SSIM value, which is added to the thread's sum.  ALL of this is fp64 (the fp32 weights widened exactly), on the byte
// values themselves (every product of two of them is exact), scaled by 1 / 255 and 1 / 255^2 once per output element: in fp32 the
// variances E[x^2] - mu^2 of a flat region are rounding error of the size of 1e-7, which stands against C2 = 9e-4 with one
// sign over the whole region -- the reference's fp32 scores of flat images are 2e-5 .. 1e-4 off.
// The squared differences are taken from the staged bytes of the tile's own rows and elements, as integers.  Neither the map
// nor a moment reaches global memory: HBM sees each byte once, plus the halo (10 rows of 42, 10 pixels of 74, out of L2).
//
// Reduction, in a fixed order: lanes by xor butterfly, the workgroup's waves in order -> one (int64, fp64) partial per tile in
// the workspace; image_metrics_sum_kernel adds an image's partials in index order.  A tile's partial depends on its image only.
#include "common.h"
#include "window11.h"
#include "../../include/gs2m_metrics.h"

namespace {

constexpr int TILE_H = GS2M_METRICS_TILE_H;
constexpr int METRICS_PF = 3;  // input rows in flight ahead of the row being consumed

template <int CH>
__global__ void __launch_bounds__(64 * CH) image_metrics_kernel(int H, int W, int tiles_x, int tiles_y, const uint8_t* __restrict__ a,
                                                                const uint8_t* __restrict__ b, long long* __restrict__ part_sse,
                                                                double* __restrict__ part_ssim) {
    constexpr int T = 64 * CH;       // threads = elements (bytes) of a tile row
    constexpr int HALO = 5 * CH;     // elements of 5 pixels
    constexpr int LDSW = T + 2 * HALO;
    __shared__ double s_a[2][LDSW], s_b[2][LDSW];  // byte values 0 .. 255
    __shared__ double s_ssim[CH];
    __shared__ unsigned long long s_sse[CH];
    const int tid = threadIdx.x;
    const unsigned blk = blockIdx.x;
    const int tx = (int)(blk % (unsigned)tiles_x);
    const unsigned rest = blk / (unsigned)tiles_x;
    const int ty = (int)(rest % (unsigned)tiles_y), n = (int)(rest / (unsigned)tiles_y);
    const int E = W * CH;
    const int e0 = tx * T, y0 = ty * TILE_H;
    const size_t image = (size_t)n * (size_t)H * (size_t)E;
    const uint8_t* __restrict__ A = a + image;
    const uint8_t* __restrict__ Bm = b + image;
    const int ea = e0 - HALO + tid, eb = e0 - HALO + T + tid;  // main element and (threads 0 .. 2 HALO - 1) the tail of the right halo
    const bool ina = ea >= 0 && ea < E, inb = tid < 2 * HALO && eb < E;
    const int rows = min(TILE_H, H - y0);
    const bool mine = e0 + tid < E;  // this thread's element exists
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    const double inv = 1.0 / 255.0, inv2 = 1.0 / 65025.0;  // moments of the byte values -> moments of value / 255
    double ssim = 0.0;
    uint32_t sse = 0u;  // at most 32 rows x 255^2 per thread
    // the multi-wave buffer and barrier rule at CH = 1 too: one template, and the one-wave rule would be another kernel
    window11_walk<double, int, 5, 4, METRICS_PF, T, false>(
        y0, rows,
        [&](int y, int (&v)[4]) {  // bytes outside the image read as 0: the zero padding
            const bool row = y >= 0 && y < H;
            const size_t o = (size_t)(row ? y : 0) * (size_t)E;
            v[0] = (row && ina) ? A[o + ea] : 0;
            v[1] = (row && ina) ? Bm[o + ea] : 0;
            v[2] = (row && inb) ? A[o + eb] : 0;
            v[3] = (row && inb) ? Bm[o + eb] : 0;
        },
        [&](int buf, int t, const int (&v)[4]) {
            s_a[buf][tid] = (double)v[0]; s_b[buf][tid] = (double)v[1];
            if (tid < 2 * HALO) { s_a[buf][T + tid] = (double)v[2]; s_b[buf][T + tid] = (double)v[3]; }
            if (t >= 5 && t < rows + 5) {  // a row of the tile itself: elements e0 .. e0 + T - 1, each held by exactly one thread
                const int dd = tid >= HALO ? v[0] - v[1] : v[2] - v[3];
                sse += (uint32_t)(dd * dd);
            }
        },
        [&](int buf, const double (&w)[11], double (&h)[5]) { window11_moments<CH>(s_a[buf], s_b[buf], tid, w, h); },
        [&](int, const double (&m)[5]) {
            const auto [Cc, Dd, Aa, Bb] = window11_ssim(m[0] * inv, m[1] * inv2, m[2] * inv, m[3] * inv2, m[4] * inv2, C1, C2);
            if (mine) ssim += (Cc * Dd) / (Aa * Bb);
        });

    unsigned long long e = sse;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        ssim += __shfl_xor(ssim, d, 64);
        e += __shfl_xor(e, d, 64);
    }
    if ((tid & 63) == 0) { s_ssim[tid >> 6] = ssim; s_sse[tid >> 6] = e; }
    gs2m_sync();
    if (tid == 0) {
        double s = s_ssim[0];
        unsigned long long q = s_sse[0];
#pragma unroll
        for (int k = 1; k < CH; k++) { s += s_ssim[k]; q += s_sse[k]; }
        part_sse[blk] = (long long)q;
        part_ssim[blk] = s;
    }
}

// one thread per image: its partials in index order
__global__ void __launch_bounds__(64) image_metrics_sum_kernel(int N, int parts, const long long* __restrict__ part_sse,
                                                               const double* __restrict__ part_ssim, long long* __restrict__ sse,
                                                               double* __restrict__ ssim_sum) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    const size_t o = (size_t)n * (size_t)parts;
    long long e = 0;
    double s = 0.0;
    for (int p = 0; p < parts; p++) {
        e += part_sse[o + p];
        s += part_ssim[o + p];
    }
    sse[n] = e;
    ssim_sum[n] = s;
}

// tiles of one image along x and y, or false when the sizes are refused
bool metrics_plan(int N, int H, int W, int CH, int* tiles_x, int* tiles_y) {
    if (N < 1 || H < 1 || W < 1 || (CH != 1 && CH != 3)) return false;
    if ((long long)CH * W > (1ll << 30) || H > (1 << 30) || (long long)CH * W * H > (1ll << 40)) return false;
    const long long nx = ((long long)W + GS2M_METRICS_TILE_W - 1) / GS2M_METRICS_TILE_W;
    const long long ny = ((long long)H + TILE_H - 1) / TILE_H;
    if (nx * ny > 0x7FFFFFFFll || nx * ny * N > 0x7FFFFFFFll) return false;
    *tiles_x = (int)nx;
    *tiles_y = (int)ny;
    return true;
}

}  // namespace

extern "C" int gs2m_image_metrics_workspace_bytes(int N, int H, int W, int CH, long long* bytes) {
    int nx, ny;
    if (!bytes || !metrics_plan(N, H, W, CH, &nx, &ny)) return GS2M_ERR_INVALID_ARG;
    *bytes = 16ll * N * nx * ny;  // int64[N tiles], then fp64[N tiles]
    return GS2M_OK;
}

extern "C" int gs2m_image_metrics(int N, int H, int W, int CH, const unsigned char* a, const unsigned char* b, void* ws,
                                  long long ws_bytes, long long* sse, double* ssim_sum, void* stream) {
    int nx, ny;
    if (!a || !b || !ws || !sse || !ssim_sum || !metrics_plan(N, H, W, CH, &nx, &ny)) return GS2M_ERR_INVALID_ARG;
    const long long parts = (long long)nx * ny, tiles = parts * N;
    if (ws_bytes < 16 * tiles || ((uintptr_t)ws & 7u) != 0) return GS2M_ERR_INVALID_ARG;
    long long* part_sse = reinterpret_cast<long long*>(ws);
    double* part_ssim = reinterpret_cast<double*>(part_sse + tiles);
    hipStream_t s = (hipStream_t)stream;
    if (CH == 1)
        image_metrics_kernel<1><<<(unsigned)tiles, 64, 0, s>>>(H, W, nx, ny, a, b, part_sse, part_ssim);
    else
        image_metrics_kernel<3><<<(unsigned)tiles, 192, 0, s>>>(H, W, nx, ny, a, b, part_sse, part_ssim);
    image_metrics_sum_kernel<<<(N + 63) / 64, 64, 0, s>>>(N, (int)parts, part_sse, part_ssim, sse, ssim_sum);
    return hipGetLastError() == hipSuccess ? GS2M_OK : GS2M_ERR_HIP;
}
