/* gs2m_undistort.h -- C ABI of the dataset preparation (undistort.hip), part of libgs2m_raster.so.
 *
 * What COLMAP's `image_undistorter` does between the mapper and every loader here: a reconstruction with a distorted camera
 * model becomes PINHOLE cameras, resampled images and transformed 2-D observations.  The contract is THIS PROJECT'S OWN,
 * modelled on image_undistorter (UndistortCamera, bilinear resampling); no file of COLMAP's pins it.  It is written down in
 * full in csrc/undistort_model.h and DESIGN.md section 24, and restated in numpy by tests/undistort_ref.py.  Everything is
 * fp64 with + - * / and comparisons only, evaluated as written, so the host, the device and numpy agree bit for bit.
 *
 *   Models      `model` is COLMAP's id, `params` its parameters in COLMAP's order (HOST doubles; they travel as kernel arguments):
 *               0 SIMPLE_PINHOLE, 1 PINHOLE (identity), 2 SIMPLE_RADIAL, 3 RADIAL, 4 OPENCV, 6 FULL_OPENCV.  The fisheye family
 *               (5, 8, 9), FOV (7) and THIN_PRISM_FISHEYE (10) are refused with GS2M_ERR_INVALID_ARG: they need atan / tan.
 *   pinhole4    {fx, fy, cx, cy} of the undistorted PINHOLE camera (HOST doubles).
 *   Images      8-bit, interleaved (n, h, w, channels), dense; the pointers need no alignment.
 *
 * Every buffer is the caller's (the library allocates nothing).  Calls with a `stream` are asynchronous on it.  Return GS2M_OK
 * (0) or a negative GS2M_ERR_* code (gs2m_raster.h); a call that returns an error has launched nothing and written nothing. */
#ifndef GS2M_UNDISTORT_H
#define GS2M_UNDISTORT_H

#ifdef __cplusplus
extern "C" {
#endif

/* The undistorted camera (undistort_model.h, "the undistorted camera"): a crop about the principal point whose size follows
 * from the undistorted image borders; blank_pixels in [0, 1] (0: no black pixels, 1: every source pixel kept), the scale
 * clamped to [min_scale, max_scale].  Host only, no GPU is touched.  out_w, out_h, pinhole4: HOST outputs.
 * GS2M_ERR_INVALID_ARG for a refused model, w or h < 1, a NULL pointer, non-finite parameters, a focal length <= 0,
 * blank_pixels outside [0, 1], min_scale <= 0, max_scale < min_scale, max_scale * max(w, h) > 2^31 - 1, and when no sample of an
 * image border can be undistorted. */
int gs2m_undistort_camera(int model, int w, int h, const double* params, double blank_pixels, double min_scale, double max_scale,
                          int* out_w, int* out_h, double* pinhole4);

/* src (n_images, h, w, channels) -> dst (n_images, oh, ow, channels), channels in {1, 3}, all images under one camera.  Output
 * pixel (x, y) reads the source at distort((x + 0.5 - cx') / fx', (y + 0.5 - cy') / fy') in pixels minus 0.5, bilinear in fp64:
 * (1 - ty) ((1 - tx) p00 + tx p01) + ty ((1 - tx) p10 + tx p11), the byte floor(v + 0.5).  A position outside
 * [0, w - 1] x [0, h - 1] or a non-finite one gives 0 in every channel.  valid (oh, ow) or NULL: 255 where the position was
 * inside, 0 elsewhere.  dst and valid must not overlap src.
 * GS2M_ERR_INVALID_ARG for a refused model, a size or n_images < 1, channels outside {1, 3}, a row of more than 2^31 - 1 bytes,
 * and a NULL params, src, pinhole4 or dst; GS2M_ERR_UNSUPPORTED for oh > 262140. */
int gs2m_undistort_images_u8(int model, const double* params, int w, int h, int channels, int n_images, const unsigned char* src,
                             const double* pinhole4, int ow, int oh, unsigned char* dst, unsigned char* valid, void* stream);

/* n observations xy (n, 2) DEVICE doubles, pixels of the distorted camera -> xy_out (n, 2): ((x - cx) / fx, (y - cy) / fy)
 * through the Newton iteration of undistort_model.h, then fx' u + cx', fy' v + cy'.  failed: DEVICE int, the number of
 * observations whose iteration failed (they keep their last finite iterate); it is zeroed on the stream first.  xy_out may be
 * xy.  n = 0 is valid (failed = 0).  GS2M_ERR_INVALID_ARG for a refused model, n < 0, and a NULL params, pinhole4, failed, or
 * (n > 0) xy or xy_out. */
int gs2m_undistort_points(long long n, const double* xy, int model, const double* params, const double* pinhole4, double* xy_out,
                          int* failed, void* stream);

#ifdef __cplusplus
}
#endif

#endif
