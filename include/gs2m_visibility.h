/* gs2m_visibility.h -- C ABI of the mesh visibility cull (mesh_depth.hip), part of libgs2m_raster.so.
 *
 * The reference culls a reconstructed mesh against the camera trajectory with scripts/eval_tnt/cull_mesh.py: it renders the
 * mesh's depth from every camera, projects every vertex into every view and keeps the vertices that at least min_views views
 * see; DESIGN.md §14 writes the contract down.  Transform, coverage and depth are fp64 and evaluated as written
 * (-ffp-contract=off).  Vertices are (n, 3) fp64, triangles (n, 3) int, a view is a DEVICE double 4 x 4 world-to-camera matrix,
 * row major, OpenCV convention (x right, y down, z forward); fx, fy, cx, cy are the pinhole intrinsics of every view.
 *
 *   Camera space   c_k = ((M[k][0] x + M[k][1] y) + M[k][2] z) + M[k][3], k = 0, 1, 2.
 *   Pixel centre   pixel (i, j) (column i, row j) has its centre at (i + 0.5, j + 0.5); its ray is
 *                  r = ((i + 0.5 - cx) / fx, (j + 0.5 - cy) / fy, 1).
 *   Coverage       on the camera-space vertices a, b, c: the triangle covers the pixel when dot(cross(b, c), r),
 *                  dot(cross(c, a), r) and dot(cross(a, b), r) are all >= 0 or all <= 0 and not all zero.  Both faces count; a
 *                  centre exactly on an edge is covered.  Geometry is not clipped: a triangle that crosses the camera plane gives
 *                  the pixels of its part in front.
 *   Depth          z = dot(n, a) / dot(n, r), n = cross(b - a, c - a); the sample counts only when near <= z <= far.  z is
 *                  rounded once to fp32.
 *   Resolve        the per-pixel minimum of the fp32 values (taken on their bit patterns: positive floats order as unsigned
 *                  integers); a pixel no sample reaches is 0.  The image does not depend on the order of the triangles.
 *   Rejected       a triangle with n == 0, or with a non-finite camera-space coordinate, is skipped.
 *   Votes          per vertex p and view: (x, y, z0) = the camera-space point, z = z0 + 1e-8, u = (fx x + cx z0) / z,
 *                  v = (fy y + cy z0) / z; inside: 0 <= u <= W - 1, 0 <= v <= H - 1 and z > 0; d: the bilinear sample of the
 *                  view's depth at texel coordinates (u, v), texel centres at integers (grid_sample, padding_mode='border',
 *                  align_corners=True), pixels of value 0 entering the average as 0:
 *                  x0 = floor(u), y0 = floor(v), tx = u - x0, ty = v - y0,
 *                  d = ((D[y0][x0] ((1 - tx) (1 - ty)) + D[y0][x0 + 1] (tx (1 - ty))) + D[y0 + 1][x0] ((1 - tx) ty)) + D[y0 + 1][x0 + 1] (tx ty),
 *                  a neighbour outside the frame (its weight is 0) taken as 0; front: d > 0 ? z < d + eps : true; the view
 *                  votes when inside and front.
 *
 * Every buffer is the caller's; the workspace size comes from gs2m_meshdepth_workspace_bytes.  Return GS2M_OK (0) or a negative
 * GS2M_ERR_* code (gs2m_raster.h).  No float atomics: results are bitwise reproducible. */
#ifndef GS2M_VISIBILITY_H
#define GS2M_VISIBILITY_H

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of gs2m_meshdepth_render's workspace for n_tris triangles rendered into n_views views in one call (HOST output). */
int gs2m_meshdepth_workspace_bytes(long long n_tris, int n_views, long long* bytes);

/* depth: float (n_views, H, W), the camera-space z of the nearest surface through each pixel centre, 0 where there is none
 * (see above).  W, H >= 1, fx, fy != 0, 0 < near <= far, all finite.  The n_views views of a call share the triangle loads.
 * GS2M_ERR_INVALID_ARG when a triangle names a vertex outside [0, n_verts): such a triangle is never dereferenced.  The call
 * waits for the stream (it reads that flag back). */
int gs2m_meshdepth_render(long long n_verts, const double* verts, long long n_tris, const int* tris, int n_views,
                          const double* w2c, double fx, double fy, double cx, double cy, int W, int H, double near_z, double far_z,
                          void* ws, float* depth, void* stream);

/* votes[i] (int) = the views of the n_views given that vote for vertex i (see above), added to the value already there when
 * `accumulate` is not 0.  depth: float (n_views, H, W). */
int gs2m_visibility_votes(long long n_verts, const double* verts, int n_views, const double* w2c, double fx, double fy,
                          double cx, double cy, int W, int H, const float* depth, double eps, int accumulate, int* votes,
                          void* stream);

/* keep[i] = votes[i] >= min_views ? 1 : 0: the byte flags gs2m_eval_cull_triangles and gs2m_eval_compact take (gs2m_eval.h). */
int gs2m_visibility_keep(long long n_verts, const int* votes, int min_views, unsigned char* keep, void* stream);

/* flags[i] = 1 when keep[i] is set and vertex i is named by a triangle whose three vertices have keep set, else 0: the kept
 * vertices that a kept face still refers to (the reference drops the others: remove_unreferenced_vertices).  Culling with
 * `flags` keeps the same faces as culling with `keep`.  A triangle that names a vertex outside [0, n_verts) is passed over
 * here, never dereferenced; gs2m_eval_cull_triangles reports it. */
int gs2m_visibility_referenced(long long n_verts, const unsigned char* keep, long long n_tris, const int* tris,
                               unsigned char* flags, void* stream);

#ifdef __cplusplus
}
#endif

#endif
