/* gs2m_eval.h -- C ABI of the DTU mesh evaluation (mesh_eval.hip), part of libgs2m_raster.so.
 *
 * The reference scores a mesh with scripts/eval_dtu/eval.py (mesh mode) after evaluate_single_scene.py has moved it to
 * world coordinates; DESIGN.md §10 writes the contract down.  Everything is fp64 and evaluated as written
 * (-ffp-contract=off).  Points are (n, 3) fp64, row major.
 *
 *   Transform   world = v * scale + t, per component.
 *   Sampling    per triangle (p0, p1, p2): v1 = p1 - p0, v2 = p2 - p0, l = sqrt((x x + y y) + z z), c = v1 x v2, area2 = |c|;
 *               triangles with !(area2 > 0) are dropped; thr = thresh sqrt((l1 l2) / area2), n1 = floor(l1 / thr), n2 alike;
 *               candidates (i, j), i = 0..n1, j = 0..n2 row major, k0 = (i + 0.5) / max(n1, 1e-7), k1 alike, kept when
 *               k0 + k1 < 1, point (v1 k0 + v2 k1) + p0.  The cloud is the vertices, then the samples in triangle order.
 *   Thinning    in rank order a point not yet removed is kept and removes every point q with (dx dx + dy dy) + dz dz <= r r:
 *               the lexicographically-first maximal independent set of the radius graph by rank.
 *   Filter      flag bit 0 (inbound): lo <= p < hi on every axis; bit 1 (observed): inbound, g = rint((p - bb0) / res) with
 *               0 <= g < dims on every axis and mask[(g0 dims1 + g1) dims2 + g2] != 0.  Plane flag: ((P0 x + P1 y) + P2 z) + P3 > 0.
 *   Nearest     the distance sqrt((dx dx + dy dy) + dz dz) to the nearest target point when it is < max_dist, +inf otherwise.
 *   Mask cull   (csrc/mesh_cull.hip, fp32 as written) dil = the mask (any non-zero byte is foreground) dilated by the disk
 *               dx dx + dy dy <= r r, outside the image background.  Per vertex (cast to fp32) and view matrix M (4 x 4 fp32):
 *               c_k = ((M[k][0] x + M[k][1] y) + M[k][2] z) + M[k][3], px = c_0 / (c_2 + 1e-6f), py alike,
 *               nx = (px / (Wn - 1) - 0.5f) * 2, valid = -1 < nx < 1 and -1 < ny < 1, ix = rint(((nx + 1) / 2) (W - 1)), iy alike,
 *               sample = dil[iy, ix] inside the mask, 0 outside; the view passes when sample or not valid; a vertex is kept when
 *               every view passes.  A face is kept when its three vertices are; kept vertices keep their order, referenced or not.
 *
 * Every buffer is the caller's (the library allocates nothing); workspace sizes come from the *_bytes calls.  Calls are
 * asynchronous on `stream` except those that write a HOST result (they wait for the stream).  Return GS2M_OK (0) or a negative
 * GS2M_ERR_* code (gs2m_raster.h).  No float atomics: results are bitwise reproducible. */
#ifndef GS2M_EVAL_H
#define GS2M_EVAL_H

#ifdef __cplusplus
extern "C" {
#endif

/* out[i] = in[i] * scale + t (HOST double[3]); in and out may be the same buffer. */
int gs2m_eval_transform(long long n, const double* in, double scale, const double* t, double* out, void* stream);

/* Workspaces of the sampling: tri_bytes per `n_tris` triangles, row_bytes per `n_rows` rows (HOST outputs; either may be NULL). */
int gs2m_eval_sample_workspace_bytes(long long n_tris, long long n_rows, long long* tri_bytes, long long* row_bytes);

/* Sampling, pass 1: n1, n2 and the candidate rows holding samples (i < n1) of every triangle, scanned.  host_rows: HOST long long,
 * the total.  GS2M_ERR_INVALID_ARG when a triangle names a vertex outside [0, n_verts). */
int gs2m_eval_sample_rows(long long n_verts, const double* verts, long long n_tris, const int* tris, double thresh, void* tri_ws,
                          long long* host_rows, void* stream);

/* Pass 2: the kept samples of every row, scanned.  host_samples: HOST long long, the total. */
int gs2m_eval_sample_count(long long n_tris, long long n_rows, const void* tri_ws, void* row_ws, long long* host_samples,
                           void* stream);

/* Pass 3: cloud (n_verts + n_samples, 3): the vertices, then the samples. */
int gs2m_eval_sample_emit(long long n_verts, const double* verts, long long n_tris, const int* tris, long long n_rows,
                          const void* tri_ws, const void* row_ws, long long n_samples, double* cloud, void* stream);

/* out[q] = pts[order[q]]; an order entry outside [0, n) gives a NaN point. */
int gs2m_eval_gather(long long n, const double* pts, const long long* order, double* out, void* stream);

/* A hashed uniform grid over n points: grid_bytes for the grid itself, build_bytes for the build's scratch (HOST outputs). */
int gs2m_eval_grid_bytes(long long n, long long* grid_bytes, long long* build_bytes);

/* Builds the grid of edge `cell` (> 0) over pts into `grid`. */
int gs2m_eval_grid_build(long long n, const double* pts, double cell, void* grid, void* build_ws, void* stream);

/* Bytes of the thinning workspace for n points (grid, build scratch and state; HOST output). */
int gs2m_eval_thin_workspace_bytes(long long n, long long* bytes);

/* Thinning of pts with radius r > 0 by rank (rank: unsigned[n], distinct, or NULL for rank = index).  keep: uint8[n], 1 = kept.
 * host_rounds: HOST int, the rounds run (may be NULL). */
int gs2m_eval_thin(long long n, const double* pts, const unsigned* rank, double radius, void* ws, unsigned char* keep,
                   int* host_rounds, void* stream);

/* Filter flags (see above): lo, hi, bb0 HOST double[3], dims HOST int[3], mask uint8 C-contiguous (dims0, dims1, dims2). */
int gs2m_eval_filter(long long n, const double* pts, const double* lo, const double* hi, const double* bb0, double res,
                     const unsigned char* mask, const int* dims, unsigned char* flags, void* stream);

/* flags[i] = ((P0 x + P1 y) + P2 z) + P3 > 0, plane HOST double[4]. */
int gs2m_eval_above_plane(long long n, const double* pts, const double* plane, unsigned char* flags, void* stream);

/* Bytes of the compaction workspace for n entries (HOST output); the masked mean needs the one for n = 0. */
int gs2m_eval_scan_workspace_bytes(long long n, long long* bytes);

/* out: the points whose flags have `bit` set, in index order (room for n); host_count: HOST long long. */
int gs2m_eval_compact(long long n, const double* pts, const unsigned char* flags, int bit, void* ws, double* out,
                      long long* host_count, void* stream);

/* dist[i]: the distance of queries[i] to its nearest point of the grid built over the n_targets points with edge `cell`
 * when it is < max_dist, else +inf. */
int gs2m_eval_nearest(long long n_queries, const double* queries, long long n_targets, double cell, const void* grid,
                      double max_dist, double* dist, void* stream);

/* gs2m_eval_nearest plus index[i]: the nearest point's index in the targets' given order (the lowest index among points at
 * the same (dx dx + dy dy) + dz dz), -1 where dist[i] is +inf.  dist equals gs2m_eval_nearest's bit for bit. */
int gs2m_eval_nearest_index(long long n_queries, const double* queries, long long n_targets, double cell, const void* grid,
                            double max_dist, long long* index, double* dist, void* stream);

/* The sum and count of the entries < max_dist, summed in a fixed order (HOST outputs). */
int gs2m_eval_masked_mean(long long n, const double* dist, double max_dist, void* ws, double* host_sum, long long* host_count,
                          void* stream);

/* Bytes of n_views dilated masks, bit-packed: one bit per pixel (bit x & 63 of word x >> 6), rows of ceil(W / 64) 64-bit words,
 * padding bits 0 (HOST output). */
int gs2m_eval_dilate_bytes(int n_views, int H, int W, long long* bytes);

/* packed = masks (n_views, H, W) uint8, != 0 is foreground, dilated by the disk of radius r (0 <= r <= 64), in the layout of
 * gs2m_eval_dilate_bytes.  H, W >= 1. */
int gs2m_eval_dilate_disk(int n_views, int H, int W, const unsigned char* masks, int r, void* packed, void* stream);

/* keep[i] = 1 when vertex i passes every view (see above), else 0.  view_mats: DEVICE float (n_views, 4, 4), row major;
 * packed: the dilated masks (n_views, H, W); Wn, Hn: the image size the pixel coordinates are normalised by.  n_views = 0 keeps
 * every vertex. */
int gs2m_eval_cull_flags(long long n, const double* verts, int n_views, const float* view_mats, int H, int W, const void* packed,
                         int Wn, int Hn, unsigned char* keep, void* stream);

/* Bytes of gs2m_eval_cull_triangles' workspace (HOST output). */
int gs2m_eval_cull_workspace_bytes(long long n_verts, long long n_tris, long long* bytes);

/* out_tris (room for n_tris): the triangles whose three vertices have bit 0 of keep set, in input order, renumbered to the kept
 * vertices' positions (the vertices themselves: gs2m_eval_compact with the same flags, bit 0).  host_totals: HOST long long[2],
 * the kept vertices and the kept triangles.  GS2M_ERR_INVALID_ARG when a triangle names a vertex outside [0, n_verts). */
int gs2m_eval_cull_triangles(long long n_verts, const unsigned char* keep, long long n_tris, const int* tris, void* ws,
                             int* out_tris, long long* host_totals, void* stream);

#ifdef __cplusplus
}
#endif

#endif
