/* gs2m_lpips.h -- C ABI of LPIPS (VGG16, v0.1) on 8-bit image pairs (lpips.hip), part of libgs2m_raster.so.
 *
 * The reference scores its rendered views with metrics.py:57 `lpips(render, gt, net_type='vgg')`; lpipsPyTorch/modules/lpips.py,
 * networks.py:36-63,88-96 and utils.py:6-8 are the computation, DESIGN.md §18 writes the contract down.
 *
 *   Input       N pairs of contiguous 8-bit images (H, W, 3), as gs2m_image_metrics takes them; value / 255 in fp32, NOT mapped to
 *               [-1, 1] (metrics.py:33).  z-score (x - mean) / std, a divide, with the constants of networks.py:41-44.
 *   Network     vgg16().features modules 0 .. 29: thirteen 3x3 convolutions (stride 1, zero padding 1, bias) each followed by ReLU,
 *               2x2 / stride 2 max-pools (floor sizing) after convolutions 2, 4, 7 and 10; the taps are the ReLU outputs of
 *               convolutions 2, 4, 7, 10 and 13 with GS2M_LPIPS_TAP_CHANNELS channels.
 *   Distance    per tap and pixel f / (sqrt(sum_c f^2) + 1e-10) of both images, sum_c lin[c] (fx - fy)^2, then the spatial mean;
 *               LPIPS is the sum of the five means.
 *
 * Numerics: activations and weights are fp32.  A convolution output is ONE fp32 fmaf chain over K = 9 Cin products that starts
 * from the bias, in (Cin chunk of 16, tap, channel) order, on the fp32-input matrix instruction (v_mfma_f32_32x32x2_f32, whose
 * result is that chain bit for bit) -- Cin = 3 on the vector unit in (tap, channel) order.  A pixel's tap value is fp32; pixels
 * are added in fp64 per workgroup and the workgroups' partials in index order.  No float atomics: two calls give the same bits,
 * and a pair's value does not depend on the batch it is in.
 *
 * Activations are channels-innermost (N, H, W, C).  Weights are PACKED once per weight set: per convolution 9 Cin Cout floats
 * [tap = 3 ky + kx][cin][cout] followed by Cout bias floats (gs2m_lpips_pack_conv's output, which gs2m_lpips_conv3x3 reads), the
 * thirteen layers back to back, then the five lin vectors: GS2M_LPIPS_PACKED_FLOATS floats in all.
 *
 * gs2m_lpips LOOPS over the N pairs with ONE pair's workspace: render and ground truth go through the network as a batch of two
 * in two ping-pong buffers of 2 H W 64 floats each (about 1 GB each at 1600x1200).
 *
 * Every buffer is the caller's (the library allocates nothing).  Calls are asynchronous on `stream`.  Return GS2M_OK (0) or a
 * negative GS2M_ERR_* code (gs2m_raster.h); on an error nothing is launched or written. */
#ifndef GS2M_LPIPS_H
#define GS2M_LPIPS_H

#ifdef __cplusplus
extern "C" {
#endif

#define GS2M_LPIPS_CONVS 13
#define GS2M_LPIPS_TAPS 5
#define GS2M_LPIPS_MIN_SIZE 16      /* four floor-sized pools leave one pixel of a 16 .. 31 pixel side */
#define GS2M_LPIPS_TILE 16          /* a workgroup of the convolution takes GS2M_LPIPS_TILE x GS2M_LPIPS_TILE pixels x 64 Cout */
#define GS2M_LPIPS_PACKED_FLOATS 14716160ll /* sum of 9 Cin Cout + Cout over the 13 layers, + 64 + 128 + 256 + 512 + 512 */

/* One convolution's weights (DEVICE, OIHW: float[cout][cin][3][3]) and bias (DEVICE float[cout]) -> packed (DEVICE,
 * 16-byte aligned, float[9 cin cout + cout]).  cin is 3 or a multiple of 16, cout a multiple of 64, both <= 512:
 * GS2M_ERR_UNSUPPORTED otherwise. */
int gs2m_lpips_pack_conv(int cin, int cout, const float* w_oihw, const float* bias, float* packed, void* stream);

/* conv_w, conv_b: HOST arrays of GS2M_LPIPS_CONVS DEVICE pointers (OIHW weights and biases of vgg16 features 0, 2, 5, 7, 10, 12,
 * 14, 17, 19, 21, 24, 26, 28); lin: HOST array of GS2M_LPIPS_TAPS DEVICE pointers to the lin vectors (64, 128, 256, 512, 512
 * floats).  packed: DEVICE, 16-byte aligned, GS2M_LPIPS_PACKED_FLOATS floats. */
int gs2m_lpips_pack_weights(const void* const* conv_w, const void* const* conv_b, const void* const* lin, float* packed,
                            void* stream);

/* Bytes of gs2m_lpips' workspace for pairs of (H, W, 3) images (HOST output); it does not grow with N.  GS2M_ERR_INVALID_ARG
 * for N < 1, H or W < GS2M_LPIPS_MIN_SIZE (the last tap would be empty), H or W > 32768, H W > 2^26. */
int gs2m_lpips_workspace_bytes(int N, int H, int W, long long* bytes);

/* a, b: DEVICE (N, H, W, 3) uint8; packed: gs2m_lpips_pack_weights' output; ws: DEVICE, 16-byte aligned, ws_bytes >= what the
 * query returns; out_total: DEVICE double[N]; out_layers: DEVICE double[N * 5], the per-tap means whose sum (taps in order)
 * out_total is.  GS2M_ERR_INVALID_ARG as above and for a NULL pointer, a misaligned or too-small workspace. */
int gs2m_lpips(int N, int H, int W, const unsigned char* a, const unsigned char* b, const float* packed, void* ws,
               long long ws_bytes, double* out_total, double* out_layers, void* stream);

/* ONE convolution + bias + ReLU, the kernel gs2m_lpips launches: in DEVICE float (N, H, W, cin), packed as gs2m_lpips_pack_conv
 * writes it, out DEVICE float (N, H, W, cout); in, packed and out 16-byte aligned (in of cin = 3: 4-byte).  N, H, W >= 1 (any
 * size: borders and tile remainders are predicated), N H W <= 2^26; cin, cout as gs2m_lpips_pack_conv. */
int gs2m_lpips_conv3x3(int N, int H, int W, int cin, int cout, const float* in, const float* packed, float* out, void* stream);

/* 2x2 / stride 2 max-pool with floor sizing, the kernel gs2m_lpips launches: in DEVICE float (N, H, W, C) -> out DEVICE float
 * (N, H / 2, W / 2, C); C a multiple of 4, H and W >= 2, both pointers 16-byte aligned. */
int gs2m_lpips_maxpool2x2(int N, int H, int W, int C, const float* in, float* out, void* stream);

/* Bytes of gs2m_lpips_tap_distance's workspace (HOST output). */
int gs2m_lpips_tap_workspace_bytes(int N, int H, int W, long long* bytes);

/* One tap's distance, the kernel gs2m_lpips launches: fx, fy DEVICE float (N, H, W, C) feature maps (NOT yet normalised),
 * lin DEVICE float[C]; out DEVICE double[N]: the mean over the H W pixels of sum_c lin[c] (fx / (|fx| + 1e-10) - fy / (|fy| +
 * 1e-10))^2.  C is 64, 128, 256 or 512 (GS2M_ERR_UNSUPPORTED otherwise); ws 8-byte aligned. */
int gs2m_lpips_tap_distance(int N, int H, int W, int C, const float* fx, const float* fy, const float* lin, void* ws,
                            long long ws_bytes, double* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
