/* gs2m_tnt.h -- C ABI of the Tanks and Temples mesh evaluation (tnt_eval.hip), part of libgs2m_raster.so.
 *
 * The reference scores a mesh with scripts/eval_tnt/run.py: Open3D's crop, voxel downsample, ICP with scaling and cloud to
 * cloud distances.  DESIGN.md §11 writes the contract down; it is Open3D's behaviour as read, unpinned (Open3D is not part
 * of this stack).  Everything is fp64 and evaluated as written (-ffp-contract=off).  Points are (n, 3) fp64, row major.
 * The nearest neighbour with its index is gs2m_eval_nearest_index (gs2m_eval.h); compaction and the count below a
 * threshold are gs2m_eval_compact and gs2m_eval_masked_mean.
 *
 *   Mesh points  the vertices in order, then ((p0 + p1) + p2) / 3.0 per component for every triangle in order.
 *   Transform    x' = ((T00 x + T01 y) + T02 z) + T03, rows 1 and 2 alike.
 *   Crop         axes (u, v, w) = (1, 2, 0) for X, (0, 2, 1) for Y, (0, 1, 2) for Z.  Edge (i, j = (i + 1) mod m) crosses when
 *                (Pi[v] < p[v] && Pj[v] >= p[v]) || (Pj[v] < p[v] && Pi[v] >= p[v]); its node is
 *                Pi[u] + ((p[v] - Pi[v]) / (Pj[v] - Pi[v])) * (Pj[u] - Pi[u]).  Kept: axis_min <= p[w] <= axis_max and an odd
 *                number of crossings with node < p[u].
 *   Voxels       lo = min over the cloud - s * 0.5 per axis, voxel = floor((p - lo) / s); one point per occupied voxel: the sum
 *                of its members in input order, divided by their count; voxels in ascending (ix, iy, iz) order.
 *   ICP moments  over the pairs (x = source[i], y = target[index[i]]) with index[i] >= 0: c, sum of (dx dx + dy dy) + dz dz
 *                with d = x - y, the two means, then Sigma = (1 / c) sum (y - my)(x - mx)^T and
 *                sx2 = (1 / c) sum ((ax ax + ay ay) + az az), a = x - mx.  Every sum is taken in the fixed order of
 *                gs2m_eval_masked_mean: 256 x 256 partial sums by stride, a fixed tree, the partials in order.
 *   Histogram    numpy's rule for given edges: bin k holds edges[k] <= d < edges[k + 1], the last bin also d == edges[last].
 *
 * Every buffer is the caller's (the library allocates nothing); workspace sizes come from the *_bytes calls.  Calls are
 * asynchronous on `stream` except those that write a HOST result (they wait for the stream).  Return GS2M_OK (0) or a negative
 * GS2M_ERR_* code (gs2m_raster.h).  No float atomics: results are bitwise reproducible. */
#ifndef GS2M_TNT_H
#define GS2M_TNT_H

#ifdef __cplusplus
extern "C" {
#endif

/* cloud (n_verts + n_tris, 3): the vertices, then the triangle centres.  ws: 8 bytes of device scratch.  Waits for the
 * stream: GS2M_ERR_INVALID_ARG when a triangle names a vertex outside [0, n_verts) (the cloud is then undefined). */
int gs2m_tnt_mesh_points(long long n_verts, const double* verts, long long n_tris, const int* tris, void* ws, double* cloud,
                         void* stream);

/* out = T applied to in; T: HOST double[16], row major, last row (0, 0, 0, 1) or GS2M_ERR_INVALID_ARG.  in and out may be
 * the same buffer. */
int gs2m_tnt_transform(long long n, const double* in, const double* T, double* out, void* stream);

/* flags[i] = 1 when point i lies in the polygon volume, else 0.  axis: 0, 1, 2 for the orthogonal axis X, Y, Z; polygon: HOST
 * double[m][3], m <= 1024 (more: GS2M_ERR_UNSUPPORTED; m == 0 keeps nothing). */
int gs2m_tnt_crop_flags(long long n, const double* pts, int axis, double axis_min, double axis_max, int m, const double* polygon,
                        unsigned char* flags, void* stream);

/* Bytes of the voxel downsample's workspace for n points (HOST output). */
int gs2m_tnt_voxel_workspace_bytes(long long n, long long* bytes);

/* Voxel downsample with edge s > 0.  out: room for n points; host_count: HOST long long, the occupied voxels.
 * GS2M_ERR_INVALID_ARG when a voxel index reaches 2^21 on an axis, or when any coordinate is infinite or NaN (the box of the
 * cloud is taken with a minimum / maximum that keeps NaN). */
int gs2m_tnt_voxel_downsample(long long n, const double* pts, double s, void* ws, double* out, long long* host_count,
                              void* stream);

/* out[i] = pts[i * k], i < ceil(n / k); k >= 1. */
int gs2m_tnt_stride_gather(long long n, const double* pts, long long k, double* out, void* stream);

/* Bytes of the ICP moments' workspace (HOST output). */
int gs2m_tnt_icp_workspace_bytes(long long* bytes);

/* The ICP moments (see above) of n source points, the targets in their given order and index[n] from
 * gs2m_eval_nearest_index: a negative entry is "no pair", an entry at or beyond n_targets gives GS2M_ERR_INVALID_ARG (an
 * index array taken against another target cloud).  host_count: the pairs c; host_out: HOST double[17]: sum d^2, mx[3],
 * my[3], Sigma[9] row major, sx2 (all 0 when c == 0). */
int gs2m_tnt_icp_moments(long long n, const double* source, long long n_targets, const double* targets, const long long* index,
                         void* ws, long long* host_count, double* host_out, void* stream);

/* counts[k] += the entries of dist in bin k of the n_edges ascending device edges (2 <= n_edges <= 4097); counts: device
 * unsigned long long[n_edges - 1], zeroed by the caller.  +inf and NaN fall in no bin. */
int gs2m_tnt_histogram(long long n, const double* dist, int n_edges, const double* edges, unsigned long long* counts,
                       void* stream);

/* ---- the error-coloured clouds (tnt_clouds.hip): EvaluateHisto's <scene>.precision.ply and <scene>.recall.ply ----
 *
 *   Neighbours   of point i: the min(k, n) points of the cloud with the smallest (d2, index), d2 = (dx dx + dy dy) + dz dz
 *                evaluated as written; point i itself is among them at d2 = 0 (Open3D's KNN search includes the query point),
 *                and equal d2 goes to the lower index.
 *   Normal       the unit eigenvector of the smallest eigenvalue of the neighbours' covariance about their own mean (two passes
 *                in neighbour order; Open3D accumulates raw moments in one), by 8 cyclic Jacobi sweeps.  Open3D leaves the sign
 *                to its solver; here it is fixed: n . (0, 0, 1) >= 0, and where that product is exactly 0 the first non-zero
 *                component is positive.  Fewer than 3 neighbours, a zero covariance or a non-finite vector: (0, 0, 1), Open3D's
 *                fallback.
 *   Colour       x = min(d, max_distance) / max_distance; entry min(trunc(x * 256), 255) of matplotlib's hot_r table
 *                (csrc/tnt_hot_r.h), each channel stored as round-half-even(c * 255). */

/* Bytes of gs2m_tnt_knn_normals' workspace for n points (HOST output). */
int gs2m_tnt_knn_normals_workspace_bytes(long long n, long long* bytes);

/* normals (n, 3) of the cloud pts (n, 3) from each point's k nearest neighbours; knn_index (n, k) long long or NULL: the
 * neighbours in (d2, index) order, -1 beyond min(k, n).  grid: gs2m_eval_grid_build's (gs2m_eval.h) over pts itself with the
 * edge `cell`.  1 <= k <= 32 or GS2M_ERR_INVALID_ARG (nothing is launched).  Waits for the stream once (the cloud's box in
 * cells is read back): GS2M_ERR_INVALID_ARG for a NaN or infinite coordinate, GS2M_ERR_UNSUPPORTED when the box is wider than
 * 65535 cells on an axis (the walk's shells are bounded by the box). */
int gs2m_tnt_knn_normals(long long n, const double* pts, double cell, const void* grid, int k, void* ws, double* normals,
                         long long* knn_index, void* stream);

/* rgb (n, 3) unsigned char: the colour (see above) of every distance; +inf takes the cap's colour.  max_distance > 0 and
 * finite.  ws: 8 bytes of device scratch.  Waits for the stream: GS2M_ERR_INVALID_ARG when a distance is NaN (rgb is then
 * undefined). */
int gs2m_tnt_distance_colors(long long n, const double* dist, double max_distance, void* ws, unsigned char* rgb, void* stream);

#ifdef __cplusplus
}
#endif

#endif
