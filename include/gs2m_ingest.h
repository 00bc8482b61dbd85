/* gs2m_ingest.h -- C ABI of the dataset ingestion (ingest.hip), part of libgs2m_raster.so.
 *
 * The reference turns a dataset's image files into training tensors with utils/image_utils.py:48-77 `process_input_image`:
 * mask the 8-bit image by its mask (`--mask_gt`), resize image and mask with Pillow's default filter (BICUBIC), divide by 255
 * and by the mask's maximum; scene/__init__.py:193-204 takes the NCC gray image from a second resize of the same file.
 * DESIGN.md section 15 writes the arithmetic down.  Everything here is integer arithmetic or fp32 evaluated as written, so the
 * outputs equal the reference's byte for byte and bit for bit.
 *
 *   Images      8-bit, interleaved (H, W, channels), rows dense; the pointers need no alignment.
 *   Resize      Pillow's ImagingResample for 8-bit pixels: a horizontal pass, then a vertical pass, each writing uint8.  For an
 *               axis of `in` -> `out` samples a PLAN holds, per output sample, the first input sample and the number of taps
 *               (bounds) and the taps as 22-bit fixed point (coeffs, `ksize` ints per output sample, zero behind the last tap):
 *               out = clamp(((1 << 21) + sum px[xmin + x] k[x]) >> 22, 0, 255) in a 32-bit int.  A pass whose sizes are equal is
 *               skipped.
 *   Plan        int[4 + 2 out + out ksize]: {in, out, ksize, 0}, bounds, coeffs.  Built on the host in double precision
 *               (gs2m_resize_plan touches no GPU), handed to the resize as a DEVICE copy.  The resize trusts only the taps: it
 *               derives ksize from the sizes itself and clamps every bound to the image, so a wrong plan gives wrong pixels, never
 *               an access outside the buffers.
 *
 * Every buffer is the caller's (the library allocates nothing).  Calls with a `stream` are asynchronous on it.  Return GS2M_OK
 * (0) or a negative GS2M_ERR_* code (gs2m_raster.h). */
#ifndef GS2M_INGEST_H
#define GS2M_INGEST_H

#ifdef __cplusplus
extern "C" {
#endif

#define GS2M_RESIZE_PLAN_HEADER 4

/* Bytes of the plan of an axis of `in` -> `out` samples and its taps per output sample (HOST outputs; `ksize` may be NULL).
 * GS2M_ERR_INVALID_ARG for in < 1, out < 1 and a NULL `bytes`. */
int gs2m_resize_plan_bytes(int in, int out, long long* bytes, int* ksize);

/* Fills `plan` (HOST, gs2m_resize_plan_bytes(in, out) bytes).  No GPU is touched.  GS2M_ERR_INVALID_ARG as above. */
int gs2m_resize_plan(int in, int out, int* plan);

/* out[0] (DEVICE int) = the maximum of the n bytes at src (DEVICE), 0 for n = 0.  GS2M_ERR_INVALID_ARG for n < 0 or a NULL
 * pointer. */
int gs2m_image_max_u8(long long n, const unsigned char* src, int* out, void* stream);

/* `--mask_gt`: dst = u8(clip((rgb / 255.f) * (alpha / max), 0, 1) * 255.f), the conversion truncating, per pixel of a (h, w, 3)
 * image and a (h, w) mask; max_ptr: DEVICE int, the mask's maximum (gs2m_image_max_u8).  A maximum of 0 -- the reference
 * divides by zero -- writes zeros.  dst must not overlap the inputs. */
int gs2m_image_mask_u8(int w, int h, const unsigned char* rgb_u8_hwc, const unsigned char* alpha_u8, const int* max_ptr,
                       unsigned char* dst_u8_hwc, void* stream);

/* Bytes of gs2m_image_resize_u8's `tmp` (HOST output): ow h channels when both passes run, 0 otherwise.
 * GS2M_ERR_INVALID_ARG for a size < 1, channels outside {1, 3}, and a row of more than 2^31 - 1 bytes. */
int gs2m_image_resize_workspace_bytes(int w, int h, int channels, int ow, int oh, long long* bytes);

/* src (h, w, channels) -> dst (oh, ow, channels); plan_x: the DEVICE plan of w -> ow, plan_y: of h -> oh (either may be NULL
 * when its sizes are equal); tmp: DEVICE, what the query returns (may be NULL for 0 bytes).  dst and tmp must not overlap src.
 * GS2M_ERR_INVALID_ARG as the query and for a missing pointer: nothing is launched. */
int gs2m_image_resize_u8(int w, int h, int channels, const unsigned char* src, int ow, int oh, const int* plan_x,
                         const int* plan_y, unsigned char* tmp, unsigned char* dst, void* stream);

/* One pass over a (h, w, channels) image, channels in {1, 3}; every output is optional (NULL):
 *   rgb_chw   float (channels, h, w) = u8 / 255.f, a true division
 *   alpha_1hw float (1, h, w) = alpha_u8 / max, max = alpha_max_ptr[0] (DEVICE int); zeros when max is 0.  Needs alpha_u8 and
 *             alpha_max_ptr.
 *   gray_1hw  float (1, h, w) = (r * 0.299f + g * 0.587f) + b * 0.114f of the rgb values above; channels = 3 only. */
int gs2m_image_unpack(int w, int h, int channels, const unsigned char* src_u8_hwc, const unsigned char* alpha_u8,
                      const int* alpha_max_ptr, float* rgb_chw, float* alpha_1hw, float* gray_1hw, void* stream);

#ifdef __cplusplus
}
#endif

#endif
