// Dataset preparation for gfx950: COLMAP's image_undistorter on the decoded bytes and on the 2-D observations
// (include/gs2m_undistort.h, undistort_model.h).  fp64 with + - * / only, evaluated as written
// (-ffp-contract=off): every output equals the numpy restatement's, byte for byte and bit for bit.
//
//   images   one thread per OUTPUT pixel; a workgroup is a 64 x 4 tile (a wave = 64 consecutive pixels of a row, so the stores
//            of a wave are one run of 64 channels bytes per image and its gathers walk one or two source rows).  The source
//            position is computed once, in fp64, and the thread then loops over the n_images that share the camera: four taps
//            per channel, the blend, one byte.  The position arithmetic (~45 fp64 operations) is paid once per batch and no
//            map is ever written to memory; the model travels in the kernel's argument block (scalar registers).
//   points   one thread per observation runs the Newton iteration; a failed one adds 1 to the count with an integer atomic.
#include "common.h"
#include "undistort_model.h"
#include "../../include/gs2m_undistort.h"

namespace {

constexpr int TILE_X = 64, TILE_Y = 4;

struct Pinhole {
    double q[4];
};

template <int CH>
__global__ void __launch_bounds__(TILE_X* TILE_Y) undistort_images_kernel(UndistortModel m, Pinhole out, int w, int h, int n_images,
                                                                          const uint8_t* __restrict__ src, int ow, int oh,
                                                                          uint8_t* __restrict__ dst, uint8_t* __restrict__ valid) {
    const int x = blockIdx.x * TILE_X + (threadIdx.x & (TILE_X - 1));
    const int y = blockIdx.y * TILE_Y + (threadIdx.x / TILE_X);
    if (x >= ow || y >= oh) return;
    double sx, sy;
    undistort_source_position(m, out.q, x, y, &sx, &sy);
    // (a NaN fails every comparison)
    const bool inside = sx >= 0.0 && sx <= (double)(w - 1) && sy >= 0.0 && sy <= (double)(h - 1);
    const size_t opix = (size_t)y * (size_t)ow + (size_t)x;
    if (valid) valid[opix] = inside ? (uint8_t)255 : (uint8_t)0;
    const size_t src_image = (size_t)w * (size_t)h * CH, dst_image = (size_t)ow * (size_t)oh * CH;
    uint8_t* __restrict__ o = dst + opix * CH;
    if (!inside) {
        for (int n = 0; n < n_images; n++, o += dst_image) {
#pragma unroll
            for (int c = 0; c < CH; c++) o[c] = 0;
        }
        return;
    }
    const int x0 = (int)sx, y0 = (int)sy;  // 0 <= sx: the truncation is the floor
    const int x1 = x0 + 1 < w ? x0 + 1 : w - 1, y1 = y0 + 1 < h ? y0 + 1 : h - 1;  // on the last sample tx = 0: the tap's weight is 0
    const double tx = sx - (double)x0, ty = sy - (double)y0;
    const double wx0 = 1.0 - tx, wy0 = 1.0 - ty;
    const size_t o00 = ((size_t)y0 * w + x0) * CH, o01 = ((size_t)y0 * w + x1) * CH;
    const size_t o10 = ((size_t)y1 * w + x0) * CH, o11 = ((size_t)y1 * w + x1) * CH;
    const uint8_t* __restrict__ s = src;
    for (int n = 0; n < n_images; n++, s += src_image, o += dst_image) {
#pragma unroll
        for (int c = 0; c < CH; c++) {
            const double p00 = (double)s[o00 + c], p01 = (double)s[o01 + c], p10 = (double)s[o10 + c], p11 = (double)s[o11 + c];
            const double v = wy0 * (wx0 * p00 + tx * p01) + ty * (wx0 * p10 + tx * p11);
            const int b = (int)(v + 0.5);
            o[c] = (uint8_t)(b > 255 ? 255 : b);
        }
    }
}

__global__ void __launch_bounds__(256) undistort_points_kernel(UndistortModel m, Pinhole out, long long n, const double* __restrict__ xy,
                                                               double* __restrict__ xy_out, int* __restrict__ failed) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double x = xy[2 * i], y = xy[2 * i + 1];
        double ox, oy;
        const bool ok = undistort_point(m, out.q, x, y, &ox, &oy);
        xy_out[2 * i] = ox;
        xy_out[2 * i + 1] = oy;
        if (!ok) atomicAdd(failed, 1);
    }
}

bool pinhole_of(const double* pinhole4, Pinhole* q) {
    if (!pinhole4) return false;
    for (int k = 0; k < 4; k++) q->q[k] = pinhole4[k];
    return true;
}

}  // namespace

extern "C" int gs2m_undistort_camera(int model, int w, int h, const double* params, double blank_pixels, double min_scale, double max_scale,
                                     int* out_w, int* out_h, double* pinhole4) {
    return undistort_camera_rule(model, w, h, params, blank_pixels, min_scale, max_scale, out_w, out_h, pinhole4) == 0 ? GS2M_OK
                                                                                                                        : GS2M_ERR_INVALID_ARG;
}

extern "C" int gs2m_undistort_images_u8(int model, const double* params, int w, int h, int channels, int n_images, const unsigned char* src,
                                        const double* pinhole4, int ow, int oh, unsigned char* dst, unsigned char* valid, void* stream) {
    UndistortModel m;
    Pinhole q;
    if (!params || !src || !dst || !pinhole_of(pinhole4, &q) || !undistort_unpack(model, params, &m)) return GS2M_ERR_INVALID_ARG;
    if (w < 1 || h < 1 || ow < 1 || oh < 1 || n_images < 1 || (channels != 1 && channels != 3)) return GS2M_ERR_INVALID_ARG;
    if ((long long)w * channels > 0x7FFFFFFFll || (long long)ow * channels > 0x7FFFFFFFll) return GS2M_ERR_INVALID_ARG;
    const long long by = ((long long)oh + TILE_Y - 1) / TILE_Y;
    if (by > 65535) return GS2M_ERR_UNSUPPORTED;  // the grid's y limit: an output of more than 262140 rows
    const dim3 grid((unsigned)((ow + TILE_X - 1) / TILE_X), (unsigned)by);
    hipStream_t s = (hipStream_t)stream;
    if (channels == 1)
        undistort_images_kernel<1><<<grid, TILE_X * TILE_Y, 0, s>>>(m, q, w, h, n_images, src, ow, oh, dst, valid);
    else
        undistort_images_kernel<3><<<grid, TILE_X * TILE_Y, 0, s>>>(m, q, w, h, n_images, src, ow, oh, dst, valid);
    return gs2m_status(hipGetLastError());
}

extern "C" int gs2m_undistort_points(long long n, const double* xy, int model, const double* params, const double* pinhole4, double* xy_out,
                                     int* failed, void* stream) {
    UndistortModel m;
    Pinhole q;
    if (n < 0 || !params || !failed || !pinhole_of(pinhole4, &q) || !undistort_unpack(model, params, &m)) return GS2M_ERR_INVALID_ARG;
    if (n > 0 && (!xy || !xy_out)) return GS2M_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(failed, 0, sizeof(int), s) != hipSuccess) return GS2M_ERR_HIP;
    if (n == 0) return GS2M_OK;
    const long long blocks = (n + 255) / 256;
    undistort_points_kernel<<<(unsigned)(blocks > 65536 ? 65536 : blocks), 256, 0, s>>>(m, q, n, xy, xy_out, failed);
    return gs2m_status(hipGetLastError());
}
