/* gs2m_meshview.h -- C ABI of the mesh visualisation (mesh_view.hip), part of libgs2m_raster.so.
 *
 * The reference looks at a reconstructed mesh with scripts/vis_dtu.py and scripts/vis_shiny.py: Blender and Cycles render a grey
 * diffuse mesh lit from the camera.  Here a deterministic contract takes their place: a visibility buffer from the
 * rasterizer of gs2m_visibility.h, Open3D-style vertex normals, and a headlight Lambert shade resolved over a regular grid of
 * samples.  Everything is fp64 and evaluated as written (-ffp-contract=off).  Vertices are (n, 3) fp64, triangles (n, 3) int, a
 * view is a DEVICE double 4 x 4 world-to-camera matrix, row major, OpenCV convention; fx, fy, cx, cy are the pinhole intrinsics of
 * every view at the OUTPUT size W x H; ss in {1, 2, 3, 4} is the supersampling factor.
 *
 *   Sample frame   (H ss, W ss) with the intrinsics (ss fx, ss fy, ss cx, ss cy).  Camera space, pixel centre and ray, inclusive
 *                  coverage without clipping, the depth formula, the range test and the rejected triangles are those of
 *                  gs2m_visibility.h, applied to the sample frame.
 *   Visibility     per sample the minimum over the covering triangles of the key (bits of the fp32 z << 32) | triangle index;
 *                  all ones where no triangle reaches.  Equal z goes to the lowest index: the buffer does not depend on the
 *                  order of the launch.  At ss == 1 the high words are gs2m_meshdepth_render's image.
 *   Normals        per triangle with n = cross(b - a, c - a) != 0 in world space: u = n / sqrt(dot(n, n)), and llrint(u_k 2^32)
 *                  is added to an int64 (n_verts, 3) sum at each of its three vertices (a triangle whose u is not finite adds
 *                  nothing).  The normal is sum / sqrt(dot(sum, sum)) with the sums widened to double, (0, 0, 0) for a zero sum.
 *   Shade          a sample with key (z, t): a, b, c = triangle t's vertices in camera space, r = the sample's ray,
 *                  e0 = dot(cross(b, c), r), e1 = dot(cross(c, a), r), e2 = dot(cross(a, b), r), s = (e0 + e1) + e2, l_k = e_k / s.
 *                  N = cross(b - a, c - a) (flat) or (l0 Na + l1 Nb) + l2 Nc of the vertex normals taken through the rotation
 *                  rows of the view (smooth; flat instead when one of the three is zero or N is zero or not finite).
 *                  cos = |dot(N, r)| / sqrt(dot(N, N) dot(r, r)).  Albedo: base[k], or (l0 Ca + l1 Cb) + l2 Cc of float vertex
 *                  colours widened to double.  lin_k = min(max(albedo_k (ambient + diffuse cos), 0), 1).
 *   Resolve        a pixel's ss x ss samples in row-major order, m of them covered: m == 0 gives bytes (0, 0, 0, 0); else
 *                  mean_k = (the sum of lin_k in that order) / m, enc = mean, or with srgb: 12.92 x for x <= 0.0031308, else
 *                  1.055 pow(x, 1 / 2.4) - 0.055; colour byte floor(255 enc + 0.5), alpha byte floor(255 m / ss^2 + 0.5).
 *                  Colour is straight, not premultiplied.  depth and tri_id come from sample (ss / 2) (ss + 1) of the block:
 *                  the fp32 z and the triangle index, 0 and -1 where it is empty.
 *   G-buffer       per sample, with r, l_k and N (flat or smooth) of the Shade paragraph: N is negated when dot(N, r) > 0, so
 *                  that it faces the eye; Nw_k = (M[0][k] N0 + M[1][k] N1) + M[2][k] N2 takes it to world space and
 *                  normal = Nw / sqrt(dot(Nw, Nw)); the view direction, surface to eye, is the same of -r.  albedo_k, roughness
 *                  and metallic are (l0 Xa + l1 Xb) + l2 Xc of the float vertex arrays widened to double.  Every value is
 *                  rounded once to fp32; coverage is 1.  An empty sample has coverage 0 and every value 0.
 *   Resolve RGB    the Resolve paragraph on samples shaded elsewhere: lin_k = min(max(rgb_k, 0), 1) of the sample's float RGB
 *                  widened to double, covered = its coverage byte is not 0.  With a background, (0, 0, 0) for enc where m == 0,
 *                  a = m / ss^2, the colour byte is floor(255 (a enc_k + (1 - a) min(max(bg_k, 0), 1)) + 0.5) and alpha is 255.
 *   Textured       the G-buffer paragraph with the materials read from textures: uv = (l0 uv_a + l1 uv_b) + l2 uv_c
 *                  per coordinate of the triangle's fp32 UVs widened to double, v from the top row.  An image is th rows of tw
 *                  texels of three bytes; x = u tw - 0.5, y = v th - 0.5, and the taps and weights are those of the Taps paragraph
 *                  of gs2m_meshbake.h with (x, y) for (u, v), except that a tap outside the image is clamped to the edge; the
 *                  bytes are decoded before they are mixed, in the order of the Sample paragraph there.  base_color: byte / 255,
 *                  then with srgb the inverse of the Resolve paragraph's encode (x / 12.92 up to 12.92 * 0.0031308, else
 *                  pow((x + 0.055) / 1.055, 2.4)); orm: roughness = G / 255, metallic = B / 255, without it 1 and 0;
 *                  normal_map: m_k = byte_k / 255 * 2 - 1.  With a normal map the Tangent frame paragraph of gs2m_meshbake.h
 *                  (csrc/tangent_frame.h: one definition for the bake and for this decode) is built from the triangle's world-space
 *                  corners, its UVs and N = Nw, the sample's flat or smooth normal taken to world space BEFORE the eye-facing
 *                  flip; normal = Decode of the mixed m, negated when its dot with the ray taken to world space
 *                  (rw_k = (M[0][k] r0 + M[1][k] r1) + M[2][k] r2) is > 0.  Without one the normal is the G-buffer paragraph's.
 *
 * Every buffer is the caller's; workspace sizes come from the *_workspace_bytes functions.  Return GS2M_OK (0) or a negative
 * GS2M_ERR_* code (gs2m_raster.h).  No float atomics: results are bitwise reproducible. */
#ifndef GS2M_MESHVIEW_H
#define GS2M_MESHVIEW_H

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of gs2m_meshview_visibility's workspace for n_tris triangles and n_views views in one call (HOST output). */
int gs2m_meshview_workspace_bytes(long long n_tris, int n_views, long long* bytes);

/* vis: unsigned long long (n_views, H ss, W ss), the keys (see above).  W, H >= 1, fx, fy != 0, 0 < near <= far, all finite.
 * GS2M_ERR_INVALID_ARG when ss is not 1 .. 4, W ss * H ss > 2^31 - 1, n_tris > 2^32 - 2, or a triangle names a vertex outside
 * [0, n_verts): such a triangle is never dereferenced.  The call waits for the stream (it reads that flag back). */
int gs2m_meshview_visibility(long long n_verts, const double* verts, long long n_tris, const int* tris, int n_views,
                             const double* w2c, double fx, double fy, double cx, double cy, int W, int H, int ss, double near_z,
                             double far_z, void* ws, unsigned long long* vis, void* stream);

/* Bytes of gs2m_meshview_normals's workspace (HOST output). */
int gs2m_meshview_normals_workspace_bytes(long long* bytes);

/* sums: long long (n_verts, 3); normals: double (n_verts, 3) (see above).  GS2M_ERR_INVALID_ARG when a triangle names a vertex
 * outside [0, n_verts): it adds nothing.  The call waits for the stream. */
int gs2m_meshview_normals(long long n_verts, const double* verts, long long n_tris, const int* tris, void* ws, long long* sums,
                          double* normals, void* stream);

/* rgba: unsigned char (n_views, H, W, 4) from `vis`, the keys gs2m_meshview_visibility wrote for the same mesh, views, frame
 * and ss.  normals: double (n_verts, 3) for smooth shading, NULL for flat.  colors: float (n_verts, 3) vertex colours, NULL for
 * the constant albedo (base_r, base_g, base_b).  depth: float (n_views, H, W) and tri_id: int (n_views, H, W), each NULL when
 * not wanted.  A key whose triangle index is not below n_tris, or whose triangle names a vertex outside [0, n_verts), counts as
 * an empty sample. */
int gs2m_meshview_shade(long long n_verts, const double* verts, long long n_tris, const int* tris, int n_views, const double* w2c,
                        double fx, double fy, double cx, double cy, int W, int H, int ss, const unsigned long long* vis,
                        const double* normals, const float* colors, double base_r, double base_g, double base_b, double ambient,
                        double diffuse, int srgb, unsigned char* rgba, float* depth, int* tri_id, void* stream);

/* The G-buffer of the samples (see above) from `vis`, as gs2m_meshview_shade reads it: out_normal, out_view_dir, out_albedo:
 * float (n_views, H ss, W ss, 3); out_roughness, out_metallic: float (n_views, H ss, W ss); coverage: unsigned char
 * (n_views, H ss, W ss).  normals: double (n_verts, 3) for smooth normals, NULL for flat.  albedo: float (n_verts, 3), roughness
 * and metallic: float (n_verts).  Keys are not trusted: one whose triangle index is not below n_tris, or whose triangle names a
 * vertex outside [0, n_verts), is an empty sample. */
int gs2m_meshview_gbuffer(long long n_verts, const double* verts, long long n_tris, const int* tris, int n_views, const double* w2c,
                          double fx, double fy, double cx, double cy, int W, int H, int ss, const unsigned long long* vis,
                          const double* normals, const float* albedo, const float* roughness, const float* metallic,
                          float* out_normal, float* out_view_dir, float* out_albedo, float* out_roughness, float* out_metallic,
                          unsigned char* coverage, void* stream);

/* As gs2m_meshview_gbuffer, the Textured paragraph in the place of the vertex arrays: uvs: float (n_tris, 3, 2); base_color,
 * orm, normal_map: unsigned char (th, tw, 3), orm and normal_map may each be NULL; 1 <= tw, th, and beyond GS2M_ATLAS_MAX_WIDTH
 * (gs2m_atlas.h) GS2M_ERR_UNSUPPORTED.  Keys are not trusted, as there. */
int gs2m_meshview_gbuffer_textured(long long n_verts, const double* verts, long long n_tris, const int* tris, const float* uvs, int n_views,
                                   const double* w2c, double fx, double fy, double cx, double cy, int W, int H, int ss,
                                   const unsigned long long* vis, const double* normals, int tw, int th, const unsigned char* base_color,
                                   int srgb, const unsigned char* orm, const unsigned char* normal_map, float* out_normal,
                                   float* out_view_dir, float* out_albedo, float* out_roughness, float* out_metallic,
                                   unsigned char* coverage, void* stream);

/* rgba: unsigned char (n_views, H, W, 4) from rgb: float (n_views, H ss, W ss, 3), the samples' linear colour, and coverage:
 * unsigned char (n_views, H ss, W ss) (see above).  background: float (n_views, H, W, 3) composited under the alpha, in the
 * encoding of the output, or NULL. */
int gs2m_meshview_resolve_rgb(int n_views, int W, int H, int ss, const float* rgb, const unsigned char* coverage, int srgb,
                              const float* background, unsigned char* rgba, void* stream);

#ifdef __cplusplus
}
#endif

#endif
