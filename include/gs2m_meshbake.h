/* gs2m_meshbake.h -- C ABI of the per-vertex attribute bake (mesh_bake.hip), part of libgs2m_raster.so.
 *
 * The per-view material maps of a trained model (albedo, roughness, metallic: any C <= 8 planes) are carried onto the vertices of
 * the reconstructed mesh: every vertex is projected into every view, the views that see it are sampled bilinearly and averaged
 * with a weight that favours head-on views; DESIGN.md §20 writes the contract down.  Everything is fp64 and evaluated as written
 * (-ffp-contract=off).  Vertices and normals are (n, 3) fp64, a view is a DEVICE double 4 x 4 world-to-camera matrix, row major,
 * OpenCV convention; fx, fy, cx, cy are the pinhole intrinsics of every view of the call; images are float32, row major.
 *
 *   Project, test  per vertex p and view: the camera-space point, z, u, v, `inside`, the depth sample d and `front` are those of
 *                  the Votes paragraph of gs2m_visibility.h (its z = z0 + 1e-8 included), d read from `depth`: the mesh's own
 *                  z-buffer, gs2m_meshdepth_render's image for the same views and frame.
 *   Taps           x0 = floor(u), y0 = floor(v), tx = u - x0, ty = v - y0; the four taps (y0, x0), (y0, x0 + 1), (y0 + 1, x0),
 *                  (y0 + 1, x0 + 1) have the weights (1 - tx) (1 - ty), tx (1 - ty), (1 - tx) ty, tx ty.  A neighbour outside
 *                  the frame has weight 0 and is not read.
 *   Mask           with `mask`, the view is skipped unless every tap of non-zero weight has mask >= 0.5.
 *   Weight         without `normals`, w = 1.  With them, N = the vertex's normal, o = the camera centre,
 *                  o_k = -((M[0][k] M[0][3] + M[1][k] M[1][3]) + M[2][k] M[2][3]), e = o - p,
 *                  w = max(0, dot(N, e) / sqrt(dot(N, N) dot(e, e))), dot(a, b) = (a0 b0 + a1 b1) + a2 b2;
 *                  N zero or not finite gives w = 0.
 *   Sample         a_c = ((A[y0][x0] ((1 - tx) (1 - ty)) + A[y0][x0 + 1] (tx (1 - ty))) + A[y0 + 1][x0] ((1 - tx) ty))
 *                  + A[y0 + 1][x0 + 1] (tx ty), A = maps[view][c], the fp32 taps widened to double.
 *   Accumulate     when the view is inside, front, unmasked and w > 0: sums[p][c] = sums[p][c] + w a_c for every c, then
 *                  weights[p] = weights[p] + w.  With accumulate == 0 both start from 0, else from the stored values.  The
 *                  additions happen one view at a time in view order: one call over the views 0 .. n and two calls over
 *                  0 .. k and k .. n (the second with accumulate != 0) give the same bits.
 *   Resolve        seen[p] = weights[p] >= min_weight && weights[p] > 0; out[p][c] = (float)(sums[p][c] / weights[p]) when
 *                  seen, else fallback[c].
 *
 * Every buffer is the caller's.  Return GS2M_OK (0) or a negative GS2M_ERR_* code (gs2m_raster.h).  No float atomics: a vertex
 * belongs to one thread, results are bitwise reproducible. */
#ifndef GS2M_MESHBAKE_H
#define GS2M_MESHBAKE_H

#ifdef __cplusplus
extern "C" {
#endif

/* verts: double (n_verts, 3); normals: double (n_verts, 3), gs2m_meshview_normals's output, or NULL; w2c: DEVICE double
 * (n_views, 4, 4); depth: float (n_views, H, W); maps: float (n_views, C, H, W), 1 <= C <= 8; mask: float (n_views, H, W) or NULL;
 * sums: double (n_verts, C); weights: double (n_verts) (see above).  n_verts == 0 or n_views == 0 is valid: nothing is sampled,
 * and with accumulate == 0 the two buffers are still set to 0.  GS2M_ERR_INVALID_ARG, without a launch, for C outside 1 .. 8,
 * W or H < 1, fx or fy == 0, a NaN eps or a missing buffer. */
int gs2m_meshbake_accumulate(long long n_verts, const double* verts, const double* normals, int n_views, const double* w2c,
                             double fx, double fy, double cx, double cy, int W, int H, const float* depth, int C, const float* maps,
                             const float* mask, double eps, int accumulate, double* sums, double* weights, void* stream);

/* out: float (n_verts, C); seen: unsigned char (n_verts), 1 or 0; fallback: C HOST floats (see above). */
int gs2m_meshbake_resolve(long long n_verts, int C, const double* sums, const double* weights, double min_weight,
                          const float* fallback, float* out, unsigned char* seen, void* stream);

/* ---- the texel bake: the same views averaged onto the texels of a triangle atlas (gs2m_atlas.h) ----
 *
 *   Accumulate     a texel is a point: points, normals (n_texels, 3) and owner (n_texels) are gs2m_atlas_texels's output (any
 *                  run of whole rows of it).  A texel with owner < 0 walks no view; its sums and weight are set to 0.  For
 *                  every other texel the Project .. Accumulate paragraphs above apply word for word with p = its point and
 *                  N = its normal (both kernels run the same code: csrc/bake_views.h), `accumulate` included.
 *   Resolve        seen[p] = owner[p] >= 0 && weights[p] >= min_weight && weights[p] > 0; out[p][c] =
 *                  (float)(sums[p][c] / weights[p]) when seen.  An owned texel that is not seen takes, with `attributes`
 *                  (float (n_verts, C): the vertex bake's output, or the vertex colours), (float)((l0 Xa + l1 Xb) + l2 Xc),
 *                  X the attribute rows of its triangle's corners widened to double and l the texel's barycentrics of the
 *                  Texel paragraph of gs2m_atlas.h, recomputed from cells[owner]; without `attributes`, or where its owner,
 *                  cell or corners are out of range, fallback[c].  An empty texel takes fallback[c].
 *   Pack           x = the fp32 value widened, clamped to [0, 1] (NaN -> 0).  base_color[p][d] = floor(255 enc(x_d) + 0.5),
 *                  d < 3, enc the sRGB encode of gs2m_meshview.h when srgb != 0, else the identity.  With C == 5 also
 *                  orm[p] = (255, floor(255 x_3 + 0.5), floor(255 x_4 + 0.5)): occlusion 1 (gs2m_texture_occlusion of
 *                  gs2m_meshao.h overwrites R where it is traced), roughness in G, metallic in B, glTF's ORM layout.
 *                  C == 3 (a plain colour bake) takes orm == NULL.
 *
 * ---- the tangent-space normal map (csrc/tangent_frame.h, shared with gs2m_meshview.h) ----
 *
 *   Tangent frame  of a point of a textured triangle: corners a, b, c in world space, their fp32 UVs widened to double (v from the
 *                  top row, gs2m_atlas.h), a shading normal N at the point.  e1 = b - a, e2 = c - a, (du1, dv1) = uv_b - uv_a,
 *                  (du2, dv2) = uv_c - uv_a, det = du1 dv2 - du2 dv1, d_u = (e1 dv2 - e2 dv1) / det per coordinate,
 *                  Nf = cross(e1, e2).  unit(x) = x / sqrt(dot(x, x)), dot as above.  N = unit(N); where N is zero or not finite
 *                  (or dot(N, N) is not > 0), or dot(N, Nf) <= 0, N = unit(Nf).  T = unit(d_u - N dot(N, d_u)),
 *                  B = w cross(N, T) with w = -1: glTF's bitangent points towards decreasing v, and the two halves of an atlas
 *                  cell are rotations of one another, so w is -1 for every chart of the atlas (tangent_frame.h derives it).
 *                  valid = 0 when det == 0 or is not finite, when Nf or the argument of a unit() is zero or not finite: then
 *                  T = B = 0, and N is the N above, or without a usable Nf the unit of the given normal, (0, 0, 1) without either.
 *   Encode         a world normal n: n' = unit(n), m = (dot(n', T), dot(n', B), dot(n', N)), m_z = max(m_z, 0), m = unit(m);
 *                  m = (0, 0, 1) for an invalid frame, for n zero or not finite, and where m becomes zero.
 *                  byte_k = floor(255 (0.5 m_k + 0.5) + 0.5).
 *   Decode         m_k = byte_k / 255 * 2 - 1 (a bilinear lookup mixes such values first); n = unit((T m_x + B m_y) + N m_z)
 *                  per coordinate, N for an invalid frame or where that sum is zero or not finite.
 *   Normals        per texel p with owner t: the frame of triangle t's corners and `uvs` at N = tnormals[p], the texel's
 *                  interpolated normal (gs2m_atlas_texels); n = values[p][offset .. offset + 2], the resolved planes of the baked
 *                  world normal, widened (the views' unit normals averaged: an unseen or empty texel carries 0 there and encodes
 *                  flat).  tangent[p] = Encode's m, normal_map[p] = its bytes.  An empty texel, an owner not below n_triangles
 *                  and a corner outside [0, n_verts) give m = (0, 0, 1), bytes (128, 128, 255).  The frame needs no cell: the
 *                  chart enters through the UVs alone, so any run of texels may be converted in one call. */

/* As gs2m_meshbake_accumulate; points, normals: double (n_texels, 3), normals may be NULL; owner: int (n_texels). */
int gs2m_texbake_accumulate(long long n_texels, const double* points, const double* normals, const int* owner, int n_views,
                            const double* w2c, double fx, double fy, double cx, double cy, int W, int H, const float* depth, int C,
                            const float* maps, const float* mask, double eps, int accumulate, double* sums, double* weights,
                            void* stream);

/* The n_texels texels from row `row0` on of an atlas `width` wide (whole rows, but for the last).  triangles (n_triangles, 3),
 * cells (n_triangles, 4) as gs2m_atlas_build wrote them and attributes (n_verts, C) are read only for unseen owned texels;
 * attributes may be NULL.  out: float (n_texels, C); seen: unsigned char (n_texels); fallback: C HOST floats. */
int gs2m_texbake_resolve(long long n_texels, int C, int width, int row0, const double* sums, const double* weights, double min_weight,
                         const float* fallback, const int* owner, long long n_triangles, const int* triangles, const int* cells,
                         long long n_verts, const float* attributes, float* out, unsigned char* seen, void* stream);

/* values: float (n_texels, C), C = 3 or 5; base_color, orm: unsigned char (n_texels, 3) (see Pack). */
int gs2m_texture_pack(long long n_texels, int C, const float* values, int srgb, unsigned char* base_color, unsigned char* orm,
                      void* stream);

/* The Normals paragraph for n_texels texels: owner: int (n_texels) and tnormals: double (n_texels, 3) as gs2m_atlas_texels wrote
 * them; triangles: int (n_triangles, 3); uvs: float (n_triangles, 3, 2), gs2m_atlas_build's; vertices: double (n_verts, 3);
 * values: float (n_texels, C), gs2m_texbake_resolve's output, 3 <= C <= 8, the normal in the planes offset .. offset + 2
 * (0 <= offset <= C - 3).  normal_map: unsigned char (n_texels, 3); tangent: double (n_texels, 3), the m before packing, or NULL. */
int gs2m_texture_normals(long long n_texels, const int* owner, const double* tnormals, long long n_triangles, const int* triangles,
                         const float* uvs, long long n_verts, const double* vertices, int C, int offset, const float* values,
                         unsigned char* normal_map, double* tangent, void* stream);

#ifdef __cplusplus
}
#endif

#endif
