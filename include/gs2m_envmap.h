/* gs2m_envmap.h -- C ABI of the environment-map stage (envmap.hip), part of libgs2m_raster.so.
 *
 * Radiance .hdr pixels <-> float32 images on the device, and a lat-long image -> the (6, R, R, 3) cube map that
 * pbr.CubemapLight holds as its base.  DESIGN.md section 19 is the contract; in short:
 *
 *   Pixels      the bytes of a Radiance file behind its header and resolution line ("-Y H +X W"): H scanlines, top row first.
 *   Rows        a row is NEW-STYLE RLE only when 8 <= W <= 32767 and it begins 02 02 hi lo with (hi << 8 | lo) == W; then four
 *               channel planes (R, G, B, E) follow, each coded as: a code byte c > 128 is a run of c - 128 copies of the next
 *               byte, 1 <= c <= 128 is c literal bytes.  Any other row is 4 W flat bytes, pixel by pixel.
 *   Table       5 long long per row: {kind, o0, o1, o2, o3}.  kind GS2M_HDR_ROW_FLAT: channel c of pixel x is byte o_c + 4 x
 *               (o_c = row start + c); kind GS2M_HDR_ROW_RLE: o_c is the offset of plane c's first code byte.
 *   RGBE        e == 0 -> (0, 0, 0), else m 2^(e - 136) per component (the stb / OpenCV convention, no + 0.5): exact in fp32.
 *   Encode      per pixel: negatives and NaN -> 0, +inf -> the largest finite fp32, then every component limited to 255 2^119,
 *               the largest value the format holds; v = max(r, g, b); v < 1e-32 -> 0 0 0 0; else (f, e) = frexpf(v), each
 *               mantissa byte trunc(component 2^(8 - e)) (an exact product), the exponent byte e + 128.
 *   Cube map    gs2m_latlong_to_cubemap below.
 *
 * THE SCAN'S CONTRACT: for every table that gs2m_hdr_scan accepted (returned GS2M_OK for the same bytes, nbytes, W and H),
 * gs2m_hdr_decode reads no byte outside [bytes, bytes + nbytes) and writes no float outside the row it is expanding.  (The
 * decoder also clips against nbytes and W on its own, so a table that was never scanned cannot take it out of bounds either;
 * what it then writes is unspecified.)
 *
 * Every buffer is the caller's (the library allocates nothing).  Calls with a `stream` are asynchronous on it.  Return GS2M_OK
 * (0), a negative GS2M_ERR_* code of gs2m_raster.h (GS2M_ERR_INVALID_ARG -1 for refused arguments, GS2M_ERR_HIP -2,
 * GS2M_ERR_UNSUPPORTED -4) or, from gs2m_hdr_scan, one of the GS2M_HDR_ERR_* codes below. */
#ifndef GS2M_ENVMAP_H
#define GS2M_ENVMAP_H

#ifdef __cplusplus
extern "C" {
#endif

#define GS2M_HDR_ROW_FLAT 0
#define GS2M_HDR_ROW_RLE 1
#define GS2M_HDR_TABLE_COLS 5 /* long long per row of the scan table */

#define GS2M_HDR_ERR_TRUNCATED (-10) /* the bytes end inside a row (or before one) */
#define GS2M_HDR_ERR_ZERO_CODE (-11) /* a code byte 0 in an RLE plane */
#define GS2M_HDR_ERR_OVERRUN (-12)   /* a run or a literal passes W */
#define GS2M_HDR_ERR_TRAILING (-13)  /* bytes left behind the last row */
#define GS2M_HDR_ERR_OLD_RLE (-14)   /* a flat pixel 1 1 1 n: an old-style RLE repeat marker (not supported) */

#define GS2M_ENVMAP_MIN_RES 16     /* CubemapLight.LIGHT_MIN_RES */
#define GS2M_ENVMAP_MAX_RES 16384  /* larger powers of two: GS2M_ERR_UNSUPPORTED */
#define GS2M_ENVMAP_MAX_SAMPLES 16 /* S in 1 .. 16 */

/* HOST function, no GPU call.  bytes: HOST, the nbytes pixel bytes of a W x H file; table: HOST long long[5 H], written row by
 * row (rows in front of the one that is refused are complete).  The rows are walked once, in order; the first defect decides
 * the code.  In an RLE plane a code is checked for 0, then for passing W, then for its payload lying inside the bytes.  A flat row
 * is checked for its 4 W bytes, then for repeat markers.  GS2M_ERR_INVALID_ARG for W, H < 1, nbytes < 0 and NULL pointers. */
int gs2m_hdr_scan(const unsigned char* bytes, long long nbytes, int W, int H, long long* table);

/* bytes (DEVICE, nbytes), table (DEVICE long long[5 H], as gs2m_hdr_scan wrote it) -> out (DEVICE float[H W 3], row-major
 * (H, W, 3)).  One workgroup per row.  GS2M_ERR_INVALID_ARG for W, H < 1, nbytes < 1 and NULL pointers: nothing is launched. */
int gs2m_hdr_decode(const unsigned char* bytes, long long nbytes, int W, int H, const long long* table, float* out, void* stream);

/* image (DEVICE float[H W 3]) -> out (DEVICE, 4 H W bytes): flat scanlines R G B E.  GS2M_ERR_INVALID_ARG for W, H < 1 and NULL
 * pointers: nothing is launched. */
int gs2m_hdr_encode(int W, int H, const float* image, unsigned char* out, void* stream);

/* src (DEVICE float[Hs Ws 3], lat-long, row 0 = +y, column centre u + 0.5 at phi = (2 (u + 0.5) / Ws - 1) pi) ->
 * out (DEVICE float[6 R R 3]).  Texel (f, r, c) = scale sum(w L) / sum(w) over the S x S sub-samples (a, b):
 *   x = -1 + (2 (c S + b) + 1) / (R S),  y = -1 + (2 (r S + a) + 1) / (R S)
 *   d = normalize(cube_to_dir(f, x, y))      (pbr/light.py; f = 0 .. 5: +x -x +y -y +z -z)
 *   w = (1 + x^2 + y^2)^(-3/2)               (the sub-sample's solid angle up to a constant)
 *   d' = R_y(-angle) d:  d'_x = cos(angle) d_x - sin(angle) d_z,  d'_z = sin(angle) d_x + cos(angle) d_z
 *   theta = acos(clamp(d'_y, -1, 1)),  phi = atan2(d'_x, -d'_z)
 *   u = (phi / pi + 1) / 2 Ws - 0.5,  v = theta / pi Hs - 0.5
 *   L = bilinear tap of src at (u, v), columns wrapping and rows clamping, in the form a + t (b - a)
 * fp32 throughout, sub-samples added in (a, b) order.  GS2M_ERR_INVALID_ARG for R not a power of two >= 16, S outside 1 .. 16,
 * Hs or Ws < 2, a non-finite angle or scale and NULL pointers; GS2M_ERR_UNSUPPORTED for R > 16384 and for a source of more than
 * 2^31 - 1 floats: nothing is launched. */
int gs2m_latlong_to_cubemap(int Hs, int Ws, const float* src, int R, int S, float angle, float scale, float* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
