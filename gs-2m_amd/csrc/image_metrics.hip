// Image metrics of 8-bit image pairs for gfx950: the exact sum of squared differences (PSNR) and the sum of the SSIM map, in
// ONE pass over the input (metrics.py's two scores; include/gs2m_metrics.h).
//
// The images stay interleaved (H, W, CH) as they are decoded.  A row is a flat run of E = CH W bytes in which the horizontal
// taps of an element lie CH bytes apart, and "tap outside [0, W)" is "byte outside [0, E)", so one kernel serves CH = 1 and 3.
// A workgroup of 64 CH threads (CH waves) owns a tile of 64 pixels x 32 rows and walks down its rows the way ssim.hip's wave walks
// its strip: per input row it stages the 64 CH + 10 CH bytes of both images in LDS, every thread forms the five horizontal sums
// (a, a^2, b, b^2, ab) of its element and feeds them into a ring of 11 vertical accumulators per quantity held in registers; the
// row that completes is evaluated to its SSIM value, which is added to the thread's sum.  ALL of this is fp64, on the byte
// values themselves (every product of two of them is exact), scaled by 1 / 255 and 1 / 255^2 once per output element: in fp32 the
// variances E[x^2] - mu^2 of a flat region are rounding error of the size of 1e-7, which stands against C2 = 9e-4 with one
// sign over the whole region -- the reference's fp32 scores of flat images are 2e-5 .. 1e-4 off.
// The squared differences are taken from the staged bytes of the tile's own rows and elements, as integers.  Neither the map
// nor a moment reaches global memory: HBM sees each byte once, plus the halo (10 rows of 42, 10 pixels of 74, out of L2).
//
// Reduction, in a fixed order: lanes by xor butterfly, the workgroup's waves in order -> one (int64, fp64) partial per tile in
// the workspace; image_metrics_sum_kernel adds an image's partials in index order.  A tile's partial depends on its image only.
#include "common.h"
#include "../../include/gs2m_metrics.h"

namespace {

// torch.Tensor([exp(-(x - 5)^2 / (2 * 1.5^2)) for x in range(11)]) / sum, in fp32 (utils/loss_utils.py:41-43); the same eleven
// numbers as ssim.hip's
__device__ __constant__ const float METRICS_W[11] = {0.001028380123898387f, 0.0075987582094967365f, 0.036000773310661316f,
                                                     0.10936068743467331f,  0.21300552785396576f,   0.26601171493530273f,
                                                     0.21300552785396576f,  0.10936068743467331f,   0.036000773310661316f,
                                                     0.0075987582094967365f, 0.001028380123898387f};

constexpr int TILE_H = GS2M_METRICS_TILE_H;
constexpr int METRICS_PF = 3;  // input rows in flight ahead of the row being consumed (as ssim.hip's forward)

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
    double w[11];  // the fp32 weights, exactly
#pragma unroll
    for (int k = 0; k < 11; k++) w[k] = (double)METRICS_W[k];

    const int ea = e0 - HALO + tid, eb = e0 - HALO + T + tid;  // main element and (threads 0 .. 2 HALO - 1) the tail of the right halo
    const bool ina = ea >= 0 && ea < E, inb = tid < 2 * HALO && eb < E;
    auto fetch = [&](int y, int& a0, int& b0, int& a1, int& b1) {  // bytes outside the image read as 0: the zero padding
        const bool row = y >= 0 && y < H;
        const size_t o = (size_t)(row ? y : 0) * (size_t)E;
        a0 = (row && ina) ? A[o + ea] : 0;
        b0 = (row && ina) ? Bm[o + ea] : 0;
        a1 = (row && inb) ? A[o + eb] : 0;
        b1 = (row && inb) ? Bm[o + eb] : 0;
    };

    double R[5][11];  // 5 quantities x 11 vertical accumulators
#pragma unroll
    for (int q = 0; q < 5; q++)
#pragma unroll
        for (int j = 0; j < 11; j++) R[q][j] = 0.0;

    const int rows = min(TILE_H, H - y0);
    const int nrows = rows + 10;  // input rows y0 - 5 .. y0 + rows + 4
    int pf[METRICS_PF][4];        // queue of fetched rows: pf[0] is the next one to consume
#pragma unroll
    for (int d = 0; d < METRICS_PF; d++) fetch(d < nrows ? y0 - 5 + d : -1, pf[d][0], pf[d][1], pf[d][2], pf[d][3]);
    const bool mine = e0 + tid < E;  // this thread's element exists
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    const double inv = 1.0 / 255.0, inv2 = 1.0 / 65025.0;  // moments of the byte values -> moments of value / 255
    double ssim = 0.0;
    uint32_t sse = 0u;  // at most 32 rows x 255^2 per thread
    for (int t0 = 0; t0 < nrows; t0 += 11) {
#pragma unroll
        for (int u = 0; u < 11; u++) {
            const int t = t0 + u;
            if (t < nrows) {  // workgroup-uniform
                // row t goes to buffer t & 1: a wave writes it again at row t + 2, behind the barrier of row t + 1, which every
                // wave reaches only after its reads of row t
                const int buf = t & 1;
                s_a[buf][tid] = (double)pf[0][0]; s_b[buf][tid] = (double)pf[0][1];
                if (tid < 2 * HALO) { s_a[buf][T + tid] = (double)pf[0][2]; s_b[buf][T + tid] = (double)pf[0][3]; }
                if (t >= 5 && t < nrows - 5) {  // a row of the tile itself: elements e0 .. e0 + T - 1, each held by exactly one thread
                    const int dd = tid >= HALO ? pf[0][0] - pf[0][1] : pf[0][2] - pf[0][3];
                    sse += (uint32_t)(dd * dd);
                }
#pragma unroll
                for (int d = 0; d + 1 < METRICS_PF; d++)
#pragma unroll
                    for (int c = 0; c < 4; c++) pf[d][c] = pf[d + 1][c];
                {
                    constexpr int D = METRICS_PF - 1;
                    fetch(t + METRICS_PF < nrows ? y0 - 5 + t + METRICS_PF : -1, pf[D][0], pf[D][1], pf[D][2], pf[D][3]);
                }
                gs2m_sync();
                double h[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int k = 0; k < 11; k++) {
                    const double va = s_a[buf][tid + k * CH], vb = s_b[buf][tid + k * CH];
                    const double wa = w[k] * va, wb = w[k] * vb;
                    h[0] += wa; h[1] = __builtin_fma(wa, va, h[1]);
                    h[2] += wb; h[3] = __builtin_fma(wb, vb, h[3]);
                    h[4] = __builtin_fma(wa, vb, h[4]);
                }
                // input row t is tap k of the output row t - k: ring slot (u - k) mod 11
#pragma unroll
                for (int k = 0; k < 11; k++) {
                    const int j = (u - k + 11) % 11;
#pragma unroll
                    for (int q = 0; q < 5; q++) R[q][j] = __builtin_fma(w[k], h[q], R[q][j]);
                }
                const int jo = (u + 1) % 11;  // output row t - 10 is complete
                if (t >= 10) {
                    const double mu1 = R[0][jo] * inv, mu2 = R[2][jo] * inv;
                    const double sigma1_sq = R[1][jo] * inv2 - mu1 * mu1;
                    const double sigma2_sq = R[3][jo] * inv2 - mu2 * mu2;
                    const double sigma12 = R[4][jo] * inv2 - mu1 * mu2;
                    const double Cc = 2.0 * (mu1 * mu2) + C1;
                    const double Dd = 2.0 * sigma12 + C2;
                    const double Aa = mu1 * mu1 + mu2 * mu2 + C1;
                    const double Bb = sigma1_sq + sigma2_sq + C2;
                    if (mine) ssim += (Cc * Dd) / (Aa * Bb);
                }
#pragma unroll
                for (int q = 0; q < 5; q++) R[q][jo] = 0.0;
            }
        }
    }

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
