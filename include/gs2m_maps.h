/* gs2m_maps.h -- C ABI of the per-view map images (view_maps.hip), part of libgs2m_raster.so.
 *
 * The reference's render.py stores, per view, the colour, the ground truth, a normal image, a colour-mapped depth image and
 * (material models) the BRDF maps, formed on the host by utils/image_utils.py (`save_depth_map`, `convert_normal_for_save`,
 * `map_to_rgba`) and torchvision's `save_image`.  Here every image is formed on the device as the 8-bit array that is stored;
 * DESIGN.md §13 writes the contract down.
 *
 * Every buffer is the caller's (the library allocates nothing).  Calls are asynchronous on `stream`.  Return GS2M_OK (0) or a
 * negative GS2M_ERR_* code (gs2m_raster.h); GS2M_ERR_INVALID_ARG means that nothing was launched or written.  No float
 * atomics: two calls give the same bytes. */
#ifndef GS2M_MAPS_H
#define GS2M_MAPS_H

#ifdef __cplusplus
extern "C" {
#endif

#define GS2M_MAPS_MAX_RANKS 8

/* ---- exact order statistics ------------------------------------------------------------------------------------------
 * out[j] = the value a sort of x[0 .. n) puts at ranks[j], bit for bit, found by a radix select (four 8-bit digits, most
 * significant first) on the order-preserving key of the float: sign bit flipped for x >= +0, all bits flipped below.  The
 * key orders -0.0 directly below +0.0 -- numpy's sort calls the two equal and leaves their order inside a run of zeros to
 * its algorithm; every other finite value and both infinities have one place.  Every NaN takes the key 0xFFFFFFFF: NaNs are
 * last, as in numpy, and a rank that falls among them returns the NaN 0x7FFFFFFF.
 * Per pass one kernel builds a 256-bin histogram for each distinct prefix among the ranks (LDS per workgroup, merged with
 * integer atomics) and a one-workgroup kernel narrows every rank's prefix and remaining rank on the device: nine launches,
 * no host synchronisation, the array is not sorted or copied.
 *   nonfinite  DEVICE long long[1]: the number of NaN and +-Inf among x. */

/* Bytes of gs2m_order_stats' workspace (HOST output).  GS2M_ERR_INVALID_ARG for n < 1, n > 2^31 - 1, k outside [1, 8]. */
int gs2m_order_stats_workspace_bytes(long long n, int k, long long* bytes);

/* x: DEVICE float[n]; ranks: HOST long long[k], each in [0, n), repeats allowed (read before the call returns);
 * ws: DEVICE, 8-byte aligned, ws_bytes >= the query's; out: DEVICE float[k]; nonfinite: DEVICE long long[1]. */
int gs2m_order_stats(long long n, const float* x, int k, const long long* ranks, void* ws, long long ws_bytes, float* out,
                     long long* nonfinite, void* stream);

/* ---- depth image: utils/image_utils.py:79-87 -----------------------------------------------------------------------------
 * stats: DEVICE float[4] = the order statistics at {prev, next} of the lower and {prev, next} of the upper percentile;
 * t_lo, t_hi: numpy's interpolation weights (host, fp32).  Per bound, in fp32 and as written (numpy's `_lerp`):
 *     d = next - prev;  bound = t >= 0.5 ? next - d * (1 - t) : prev + d * t
 * then per pixel  x = (min(max(depth, lo), hi) - lo) / (hi - lo + 1e-8f),  i = min(trunc(x * 256), 255),
 * rgba = {T[i][0], T[i][1], T[i][2], 255} with T matplotlib's 8-bit magma table (csrc/view_maps_magma.h).
 * depth: DEVICE float[H W]; rgba: DEVICE unsigned char[H W 4], 4-byte aligned.  H, W >= 1, H W <= 2^31 - 1. */
int gs2m_depth_colorize(int H, int W, const float* depth, const float* stats, float t_lo, float t_hi, unsigned char* rgba,
                        void* stream);

/* ---- image packing: every other map of render.py --------------------------------------------------------------------------
 * src: DEVICE float, (C, H, W) [GS2M_PACK_CHW] or (H, W, C) [GS2M_PACK_HWC], C in {1, 3}; a C = 1 source fills all three
 * colour channels.  out: DEVICE unsigned char (H, W, out_channels), out_channels in {3, 4}, no alignment needed.
 * Per pixel and channel, in this order (fp32, as written):
 *   1. GS2M_PACK_NORMAL (C = 3): v = v / max(|v|_2, 1e-12); with `rot` (DEVICE float[9], row major: the view's
 *      world_view_transform[:3, :3]) v = (v rot) * (1, -1, -1); then v = 0.5 v + 0.5   (convert_normal_for_save).
 *   2. GS2M_PACK_SRGB: v = v <= 0.0031308 ? 12.92 v : (211 max(v, eps)^(5/12) - 11) / 200   (pbr linear_to_srgb).
 *   3. mask (DEVICE float[H W], optional; needs bg, DEVICE float[3]): v = mask > 0.5 ? min(max(v, 0), 1) : bg[c].
 *   4. quantisation.  Default ROUND, torchvision's save_image: trunc(min(max(min(max(v, 0), 1) * 255 + 0.5, 0), 255)).
 *      GS2M_PACK_TRUNC, map_to_rgba's `(v * 255).byte()`: trunc(min(max(v * 255, 0), 255)).  For v in [0, 1] these are the
 *      reference's bytes; outside [0, 1] TRUNC saturates (the reference's cast wraps) and a NaN gives 0 in both.
 *   alpha (DEVICE float[H W], optional; out_channels must be 4): fourth byte trunc(min(max(alpha * 255, 0), 255)); without
 *   it the fourth byte of a 4-channel output is 255.
 * One thread writes whole 32-bit words (one RGBA pixel, or four RGB pixels as three words); the last one to three pixels
 * of an RGB image and every pixel of an output that is not 4-byte aligned are stored as bytes.
 * GS2M_ERR_INVALID_ARG: sizes (H, W < 1, H W > 2^31 - 1), C, layout, out_channels, unknown flag bits, NORMAL with C = 1, rot
 * without NORMAL, mask without bg, alpha with out_channels 3, src or out NULL. */
#define GS2M_PACK_CHW 0
#define GS2M_PACK_HWC 1
#define GS2M_PACK_TRUNC 1
#define GS2M_PACK_SRGB 2
#define GS2M_PACK_NORMAL 4
int gs2m_pack_image(int H, int W, int C, int layout, const float* src, const float* alpha, const float* mask, const float* bg,
                    const float* rot, int flags, int out_channels, unsigned char* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
