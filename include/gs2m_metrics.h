/* gs2m_metrics.h -- C ABI of the image metrics (image_metrics.hip), part of libgs2m_raster.so.
 *
 * The reference scores its rendered views with metrics.py: utils/image_utils.py:22-24 `psnr` and utils/loss_utils.py:30-70
 * `ssim` of every render/<name> against gt/<name>, both decoded from 8-bit files; DESIGN.md §12 writes the contract down.
 *
 *   Input       N pairs of contiguous 8-bit images (H, W, CH), CH in {1, 3}: image n of `a` starts at a + n H W CH, likewise b.
 *               The pointers need no alignment.
 *   SSE         sse[n] = the sum over all CH H W elements of (a - b)^2, an exact 64-bit integer.  The host forms
 *               mse = sse / (255^2 CH H W) and psnr = 20 log10(1 / sqrt(mse)) in double; sse = 0 gives +inf.
 *   SSIM        ssim_sum[n] = the sum of the SSIM map over all CH H W elements in fp64; the host divides by the count.  The map
 *               is gs2m_ssim.h's operator on value / 255: 11x11 separable Gaussian window, sigma 1.5, the eleven weights
 *               normalised in fp32, zero "same" padding per channel, C1 = 0.01^2, C2 = 0.03^2.  Unlike gs2m_ssim.h the moments
 *               and the map are evaluated in fp64 (as written, -ffp-contract=off): a score, not a training signal, and
 *               fp32 variances of flat regions are rounding error that C2 does not cover.
 *
 * Each workgroup takes a tile of GS2M_METRICS_TILE_W x GS2M_METRICS_TILE_H pixels (all channels), reads it and its 5-pixel
 * halo once, and writes one partial (int64, fp64) to the workspace; a second kernel adds every image's partials in index
 * order.  No float atomics, no map in global memory: two calls, and a batch of N against N single calls, give the same bits.
 *
 * Every buffer is the caller's (the library allocates nothing).  Calls are asynchronous on `stream`.  Return GS2M_OK (0) or a
 * negative GS2M_ERR_* code (gs2m_raster.h). */
#ifndef GS2M_METRICS_H
#define GS2M_METRICS_H

#ifdef __cplusplus
extern "C" {
#endif

#define GS2M_METRICS_TILE_W 64
#define GS2M_METRICS_TILE_H 32

/* Bytes of gs2m_image_metrics' workspace for N pairs of (H, W, CH) (HOST output).  GS2M_ERR_INVALID_ARG for N, H or W < 1,
 * CH outside {1, 3}, and sizes beyond the index arithmetic (CH W > 2^30, CH H W > 2^40, more than 2^31 - 1 tiles). */
int gs2m_image_metrics_workspace_bytes(int N, int H, int W, int CH, long long* bytes);

/* sse: DEVICE long long[N]; ssim_sum: DEVICE double[N]; ws: DEVICE, 8-byte aligned, ws_bytes >= what the query returns.
 * GS2M_ERR_INVALID_ARG as above and for a NULL pointer, a misaligned or too-small workspace: nothing is launched or written. */
int gs2m_image_metrics(int N, int H, int W, int CH, const unsigned char* a, const unsigned char* b, void* ws,
                       long long ws_bytes, long long* sse, double* ssim_sum, void* stream);

#ifdef __cplusplus
}
#endif

#endif
