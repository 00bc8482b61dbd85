/* gs2m_png.h -- C ABI of the PNG encoder (png.hip), part of libgs2m_raster.so.
 *
 * The offline stages form their 8-bit images on the device; this turns them into the zlib stream of a PNG file there: the row
 * filters, deflate and the Adler-32.  The container (signature, IHDR, one IDAT, IEND and the chunk CRCs) is the caller's, on the
 * host, over bytes that have to reach the host anyway.  DESIGN.md section 17 is the contract; in short:
 *
 *   Images      N >= 1 images of one shape, each contiguous uint8 (H, W, CH) on the device, CH in {1, 3, 4} (PNG colour types 0,
 *               2, 6; bit depth 8; no interlace).  `images` is a HOST array of N device pointers; they need no alignment.
 *   Filter      stride = 1 + W CH.  Per row the five PNG filters (None, Sub, Up, Average, Paeth; bytes left of the row and above
 *               row 0 are 0), each priced at the sum over its bytes of (v < 128 ? v : 256 - v); the cheapest wins, ties go to the
 *               lowest filter number.  The filtered stream is H records [filter byte][W CH bytes].
 *   Segments    rows_per_segment = max(1, 32768 / stride); segment s holds rows [s rps, min(H, (s + 1) rps)).  A function of
 *               (H, W, CH) only.  stride > 65536 and H stride > 2^31 - 1 are refused (GS2M_ERR_UNSUPPORTED).
 *   Deflate     per segment, independent of every other segment: literals and matches of distance 1 (length 3 .. 258), one
 *               dynamic-Huffman block, or stored blocks when those are not larger.  Every segment but the last is followed by an
 *               empty stored block, so every segment starts on a byte boundary; the last block of the last segment is final.
 *   Stream      78 01, the segments, the big-endian Adler-32 of the filtered stream.
 *
 * Integer arithmetic only; the bytes are a function of the image alone (not of N, of the launch or of the run).  Every buffer
 * is the caller's (the library allocates nothing).  Calls with a `stream` are asynchronous on it.  Return GS2M_OK (0) or a
 * negative GS2M_ERR_* code (gs2m_raster.h). */
#ifndef GS2M_PNG_H
#define GS2M_PNG_H

#ifdef __cplusplus
extern "C" {
#endif

#define GS2M_PNG_SEGMENT_BYTES 32768 /* target bytes of a segment */
#define GS2M_PNG_MAX_STRIDE 65536    /* longest record: 1 + W CH */

/* The plan of N images (H, W, CH); every output is a HOST long long and may be NULL.  No GPU is touched.
 *   rows_per_segment, n_segments   as above
 *   max_stream_bytes   capacity to reserve per image: every segment stored, 2 + sum over segments of
 *                      (bytes + 5 ceil(bytes / 65535)) + 5 (n_segments - 1) + 4
 *   workspace_bytes    gs2m_png_encode's `ws` for N images
 * GS2M_ERR_INVALID_ARG for H, W, N < 1 and CH outside {1, 3, 4}; GS2M_ERR_UNSUPPORTED for the sizes named above. */
int gs2m_png_plan(int H, int W, int CH, int N, long long* rows_per_segment, long long* n_segments, long long* max_stream_bytes,
                  long long* workspace_bytes);

/* filtered (DEVICE, N H stride bytes): the filtered streams of the N images, one after the other.  `filtered` must not overlap
 * an image.  GS2M_ERR_INVALID_ARG as the plan and for a NULL pointer (also inside `images`): nothing is launched. */
int gs2m_png_filter(int N, int H, int W, int CH, const unsigned char* const* images, unsigned char* filtered, void* stream);

/* out + n out_stride (DEVICE) receives image n's complete zlib stream, sizes[n] (DEVICE long long[N]) its length.
 * ws: DEVICE, aligned to 256 bytes, ws_bytes >= the plan's workspace_bytes; out_stride >= the plan's max_stream_bytes.
 * GS2M_ERR_INVALID_ARG as the plan, for a NULL pointer, a short or misaligned workspace and a short out_stride;
 * GS2M_ERR_UNSUPPORTED as the plan: nothing is launched or written. */
int gs2m_png_encode(int N, int H, int W, int CH, const unsigned char* const* images, void* ws, long long ws_bytes,
                    unsigned char* out, long long out_stride, long long* sizes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
