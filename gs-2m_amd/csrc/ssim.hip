// Fused SSIM map (11x11 separable Gaussian window, sigma 1.5, zero "same" padding), forward and backward, for gfx950
// (the ROCm replacement of submodules/fused-ssim, the D-SSIM term of train.py:103 and :136).
//
// Same operator as utils/loss_utils.py:30-70 `ssim` (five depthwise 11x11 conv2d + ~15 elementwise ops), same op
// boundary as the reference's extension (fused_ssim/__init__.py:8-41): forward returns the map plus the three
// partial derivatives the backward needs, backward turns dL/dmap into dL/dimg1.
//
// Layout for wave64: ONE WAVE walks down a 64-column strip with the shared walk of window11.h.  Per image row it stages
// the 74 halo columns in LDS (both images forward, the three products dL dm/d. backward) and every lane forms the
// horizontal sums for its column; the walk's register ring does the vertical pass, so each input row is read from HBM
// once per strip (+10 halo rows per SSIM_ROWS).  The epilogue (SSIM value and derivatives, or dL/dimg1) runs on the
// row that completes.  HBM: 8 B read + 16 B written per element forward, 24 + 4 B backward; the kernels are VALU
// bound (~200 lane-ops per element), not HBM bound.
#include "common.h"
#include "window11.h"
#include "../../include/gs2m_ssim.h"

namespace {

constexpr int SSIM_ROWS = 45;   // output rows per strip at most (1080 = 24 * 45); +10 halo rows of input.  ssim_rows() below picks fewer on small frames
constexpr int SSIM_LDSW = 80;   // 64 + 10 halo columns, padded
constexpr int SSIM_PF_FWD = 3;  // input rows in flight ahead of the row being consumed: the strip walk is a chain of
constexpr int SSIM_PF_BWD = 5;  // dependent HBM round trips (~1 us each) with only ~2 waves per SIMD to hide them

// ---------------------------------------------------------------- forward
__global__ void __launch_bounds__(64) ssim_fwd_kernel(int H, int W, int rows, float C1, float C2, const float* __restrict__ img1,
                                                      const float* __restrict__ img2, float* __restrict__ ssim_map,
                                                      float* __restrict__ dm_dmu1, float* __restrict__ dm_dsigma1_sq,
                                                      float* __restrict__ dm_dsigma12) {
    __shared__ float s_a[2][SSIM_LDSW], s_b[2][SSIM_LDSW];
    const int lane = threadIdx.x;
    const int x0 = blockIdx.x * 64, y0 = blockIdx.y * rows;
    const size_t plane = (size_t)blockIdx.z * H * W;
    const float* __restrict__ A = img1 + plane;
    const float* __restrict__ Bm = img2 + plane;
    const int xa = x0 - 5 + lane, xb = x0 + 59 + lane;  // main column and (lanes 0..9) the right halo column
    const bool ina = xa >= 0 && xa < W, inb = lane < 10 && xb < W;
    const int x = x0 + lane;
    window11_walk<float, float, 5, 4, SSIM_PF_FWD, 64>(
        y0, min(rows, H - y0),
        [&](int y, float (&v)[4]) {
            const bool row = y >= 0 && y < H;
            const size_t o = (size_t)(row ? y : 0) * W;
            v[0] = (row && ina) ? A[o + xa] : 0.f;
            v[1] = (row && ina) ? Bm[o + xa] : 0.f;
            v[2] = (row && inb) ? A[o + xb] : 0.f;
            v[3] = (row && inb) ? Bm[o + xb] : 0.f;
        },
        [&](int buf, int, const float (&v)[4]) {
            s_a[buf][lane] = v[0]; s_b[buf][lane] = v[1];
            if (lane < 10) { s_a[buf][64 + lane] = v[2]; s_b[buf][64 + lane] = v[3]; }
        },
        [&](int buf, const float (&w)[11], float (&h)[5]) { window11_moments<1>(s_a[buf], s_b[buf], lane, w, h); },
        [&](int yo, const float (&m)[5]) {
            const float mu1 = m[0], mu2 = m[2];
            const auto [Cc, Dd, Aa, Bb] = window11_ssim(mu1, m[1], mu2, m[3], m[4], C1, C2);
            const float rAB = 1.f / (Aa * Bb);
            if (x < W) {
                const size_t o = plane + (size_t)yo * W + x;
                ssim_map[o] = (Cc * Dd) * rAB;
                if (dm_dmu1 != nullptr) {
                    // d/dmu1 of (C D)/(A B) with sigma1_sq, sigma12 depending on mu1 through -mu1^2, -mu1 mu2
                    dm_dmu1[o] = (mu2 * 2.f * Dd) * rAB - (mu2 * 2.f * Cc) * rAB - (mu1 * 2.f * Cc * Dd) * rAB / Aa +
                                 (mu1 * 2.f * Cc * Dd) * rAB / Bb;
                    dm_dsigma1_sq[o] = (-Cc * Dd) * rAB / Bb;
                    dm_dsigma12[o] = (2.f * Cc) * rAB;
                }
            }
        });
}

// ---------------------------------------------------------------- backward
// dL/dimg1 = conv(dL dm/dmu1) + 2 img1 conv(dL dm/dsigma1_sq) + img2 conv(dL dm/dsigma12)   (the window is symmetric)
__global__ void __launch_bounds__(64) ssim_bwd_kernel(int H, int W, int rows, const float* __restrict__ img1,
                                                      const float* __restrict__ img2, const float* __restrict__ dL_dmap,
                                                      const float* __restrict__ dm_dmu1, const float* __restrict__ dm_dsigma1_sq,
                                                      const float* __restrict__ dm_dsigma12, float* __restrict__ dL_dimg1,
                                                      const float* __restrict__ dL_dvalue, float mul, float div) {
    __shared__ float s_x[2][3][SSIM_LDSW];
    // dL_dmap == nullptr: the map's gradient is the same at every element, dL_dvalue[0] * mul / div (the mean's backward)
    const float gu = dL_dmap == nullptr ? (dL_dvalue[0] * mul) / div : 0.f;
    const int lane = threadIdx.x;
    const int x0 = blockIdx.x * 64, y0 = blockIdx.y * rows;
    const size_t plane = (size_t)blockIdx.z * H * W;
    const int xa = x0 - 5 + lane, xb = x0 + 59 + lane;
    const bool ina = xa >= 0 && xa < W, inb = lane < 10 && xb < W;
    const int x = x0 + lane;
    window11_walk<float, float, 3, 8, SSIM_PF_BWD, 64>(
        y0, min(rows, H - y0),
        [&](int y, float (&v)[8]) {  // dL and the three derivative maps, main and halo column
            const bool row = y >= 0 && y < H;
            const size_t o = plane + (size_t)(row ? y : 0) * W;
            const bool m0 = row && ina, m1 = row && inb;
            v[0] = m0 ? (dL_dmap ? dL_dmap[o + xa] : gu) : 0.f;
            v[1] = m0 ? dm_dmu1[o + xa] : 0.f;
            v[2] = m0 ? dm_dsigma1_sq[o + xa] : 0.f;
            v[3] = m0 ? dm_dsigma12[o + xa] : 0.f;
            v[4] = m1 ? (dL_dmap ? dL_dmap[o + xb] : gu) : 0.f;
            v[5] = m1 ? dm_dmu1[o + xb] : 0.f;
            v[6] = m1 ? dm_dsigma1_sq[o + xb] : 0.f;
            v[7] = m1 ? dm_dsigma12[o + xb] : 0.f;
        },
        [&](int buf, int, const float (&v)[8]) {
#pragma unroll
            for (int q = 0; q < 3; q++) {
                s_x[buf][q][lane] = v[0] * v[1 + q];
                if (lane < 10) s_x[buf][q][64 + lane] = v[4] * v[5 + q];
            }
        },
        [&](int buf, const float (&w)[11], float (&h)[3]) {
#pragma unroll
            for (int q = 0; q < 3; q++) h[q] = 0.f;
#pragma unroll
            for (int k = 0; k < 11; k++)
#pragma unroll
                for (int q = 0; q < 3; q++) h[q] = __builtin_fmaf(w[k], s_x[buf][q][lane + k], h[q]);
        },
        [&](int yo, const float (&m)[3]) {
            if (x < W) {
                const size_t o = plane + (size_t)yo * W + x;
                const float a = img1[o], b = img2[o];
                dL_dimg1[o] = m[0] + 2.f * a * m[1] + b * m[2];
            }
        });
}

// Rows per strip: a strip is ONE wave walking its rows as a chain of dependent memory round trips, so a frame has to be cut into
// enough strips to fill the chip (~2000 waves): 45 rows at 1080p (2160 strips), 12 at 777 x 581 (1900 strips instead of 507, whose
// 55-row chains made the kernels 55 us each on a frame a fifth of 1080p's size).  The halo (10 input rows per strip) is re-read from L2.
inline int ssim_rows(int B, int CH, int H, int W) {
    const long long cols = (W + 63) / 64;
    const long long r = (cols * H * (long long)B * CH) / 2048;
    return (int)(r < 12 ? 12 : (r > SSIM_ROWS ? SSIM_ROWS : r));
}
inline bool ssim_dims_ok(int B, int CH, int H, int W) {
    return B > 0 && CH > 0 && H > 0 && W > 0 && (long long)B * CH <= 65535 && (H + 11) / 12 <= 65535;
}

// What the three entry points share.  `ptrs_ok`: the caller's own pointer validation, which counts on a frame that is not empty
// only; launch(grid, rows) starts the kernel.
template <class Launch>
int ssim_run(int B, int CH, int H, int W, bool ptrs_ok, Launch launch) {
    if (B == 0 || CH == 0 || H == 0 || W == 0) return GS2M_OK;
    if (B < 0 || CH < 0 || H < 0 || W < 0 || !ptrs_ok) return GS2M_ERR_INVALID_ARG;
    if (!ssim_dims_ok(B, CH, H, W)) return GS2M_ERR_UNSUPPORTED;
    const int rows = ssim_rows(B, CH, H, W);
    launch(dim3((W + 63) / 64, (H + rows - 1) / rows, B * CH), rows);
    return hipGetLastError() == hipSuccess ? GS2M_OK : GS2M_ERR_HIP;
}

// the two backward entry points: dL_dmap, or nullptr and the uniform gradient dL_dvalue[0] * mul / div
int ssim_backward(int B, int CH, int H, int W, bool ptrs_ok, const float* img1, const float* img2, const float* dL_dmap,
                  const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12, float* dL_dimg1,
                  const float* dL_dvalue, float mul, float div, void* stream) {
    return ssim_run(B, CH, H, W, ptrs_ok, [&](dim3 grid, int rows) {
        ssim_bwd_kernel<<<grid, 64, 0, (hipStream_t)stream>>>(H, W, rows, img1, img2, dL_dmap, dm_dmu1, dm_dsigma1_sq, dm_dsigma12,
                                                             dL_dimg1, dL_dvalue, mul, div);
    });
}

}  // namespace

extern "C" int gs2m_ssim_strip_rows(int B, int CH, int H, int W) {
    if (B < 0 || CH < 0 || H < 0 || W < 0) return GS2M_ERR_INVALID_ARG;
    if (!ssim_dims_ok(B, CH, H, W)) return GS2M_ERR_UNSUPPORTED;  // an empty frame too: it launches nothing, so it has no strips
    return ssim_rows(B, CH, H, W);
}

extern "C" int gs2m_ssim_forward(int B, int CH, int H, int W, float C1, float C2, const float* img1, const float* img2,
                                 float* ssim_map, float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, void* stream) {
    const bool train = dm_dmu1 || dm_dsigma1_sq || dm_dsigma12;  // all three maps or none
    const bool ok = img1 && img2 && ssim_map && (!train || (dm_dmu1 && dm_dsigma1_sq && dm_dsigma12));
    return ssim_run(B, CH, H, W, ok, [&](dim3 grid, int rows) {
        ssim_fwd_kernel<<<grid, 64, 0, (hipStream_t)stream>>>(H, W, rows, C1, C2, img1, img2, ssim_map, dm_dmu1, dm_dsigma1_sq,
                                                             dm_dsigma12);
    });
}

extern "C" int gs2m_ssim_backward(int B, int CH, int H, int W, const float* img1, const float* img2, const float* dL_dmap,
                                  const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12,
                                  float* dL_dimg1, void* stream) {
    const bool ok = img1 && img2 && dL_dmap && dm_dmu1 && dm_dsigma1_sq && dm_dsigma12 && dL_dimg1;
    return ssim_backward(B, CH, H, W, ok, img1, img2, dL_dmap, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, dL_dimg1, nullptr, 0.f, 1.f, stream);
}

extern "C" int gs2m_ssim_backward_uniform(int B, int CH, int H, int W, const float* img1, const float* img2, const float* dL_dvalue,
                                          float mul, float div, const float* dm_dmu1, const float* dm_dsigma1_sq,
                                          const float* dm_dsigma12, float* dL_dimg1, void* stream) {
    const bool ok = img1 && img2 && dL_dvalue && dm_dmu1 && dm_dsigma1_sq && dm_dsigma12 && dL_dimg1 && div != 0.f;
    return ssim_backward(B, CH, H, W, ok, img1, img2, nullptr, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, dL_dimg1, dL_dvalue, mul, div, stream);
}
