/* gs2m_mesh.h -- C ABI of the TSDF depth fusion and marching-cubes mesh extraction (tsdf.hip) and of the mesh
 * post-processing (mesh_post.hip; its contract: the block further down), part of libgs2m_raster.so.
 *
 * The reference extracts its mesh with Open3D's CPU ScalableTSDFVolume (utils/mesh_utils.py: fuse_depths,
 * render.py --extract_mesh).  This is that pipeline as DESIGN.md §9 writes it down; the contract, restated:
 *
 *   Blocks      16^3 voxels of edge `voxel`; block b has its origin at b * L (L = 16 * voxel, fp32), the centre of its voxel
 *               (i, j, k) at origin + (i + 0.5) * voxel.  Voxel v = i + 16 j + 256 k of a block; tsdf, weight and colour are
 *               fp32, structure-of-arrays per block slot: tsdf[slot * 4096 + v], weight[slot * 4096 + v],
 *               color[(slot * 3 + c) * 4096 + v] on a 0..255 scale.
 *   Domain      a dense int32 block-index table over the box [dom[0], dom[0] + dom[3]) x .. x .. in block units (dom: HOST
 *               int[6] = min x, y, z, extent x, y, z), linear index ((z - z0) ny + (y - y0)) nx + (x - x0); -1: no block.
 *   Touch       every pixel (u, v) with u, v multiples of 4 and 0 < d <= depth_trunc back-projects to
 *               c2w ((u - cx) d / fx, (v - cy) d / fy, d) and touches the blocks floor((p -/+ trunc) / L) per axis; a point whose
 *               block range does not lie wholly inside the domain is ignored and counted.  Touched blocks without a slot get
 *               the next slots in increasing linear index; the view's touched slots are listed in increasing linear index.
 *   Integrate   every voxel of the touched blocks: camera space z <= 0 skipped; uf = x fx / z + cx + 0.5, vf alike, needs
 *               0.0001 <= uf < W, 0.0001 <= vf < H; u = (int)uf, v = (int)vf; d = depth[v][u], skipped unless 0 < d <= depth_trunc;
 *               sdf = (d - z) sqrt(1 + ((u - cx) / fx)^2 + ((v - cy) / fy)^2); if sdf > -trunc: t = min(1, sdf / trunc),
 *               tsdf = (tsdf w + t) / (w + 1), color = (color w + rgb) / (w + 1), w = w + 1.
 *   Extract     the cube of voxel i is i and its +x / +y / +z neighbours (possibly in neighbouring blocks); a cube with a missing
 *               corner or a corner of weight 0 is skipped; corner k is inside when tsdf < 0; triangles from tsdf_tables.h.
 *               One vertex per crossed edge that a valid cube uses, owned by the edge's lower voxel, at
 *               p0 + |f0| / (|f0| + |f1|) * voxel along the edge, colour c0 + t (c1 - c0) divided by 255.  Vertices are numbered
 *               by (slot, voxel, axis x y z), triangles by (slot, voxel, table order); triangles face the tsdf >= 0 side.
 *
 * Every buffer is the caller's (the library allocates nothing): the block pool (block_coords int[capacity * 3], tsdf,
 * weight, color as above, ZERO-filled before first use), the index table (int[nx ny nz], -1-filled), `state` (int[4]
 * device: [0] = blocks in use, 0 at creation) and the workspaces sized by gs2m_tsdf_workspace_bytes.  Device pointers,
 * camera matrices are HOST float[16] row major.  Calls are asynchronous on `stream` except where a HOST result is written
 * (touch, mesh_count, block_coords: they wait for the stream).  Return GS2M_OK (0), GS2M_TSDF_POOL_FULL, or a negative
 * GS2M_ERR_* code (gs2m_raster.h).  No float atomics: results are bitwise reproducible. */
#ifndef GS2M_MESH_H
#define GS2M_MESH_H

#ifdef __cplusplus
extern "C" {
#endif

/* touch: the view's new blocks do not fit in `capacity`; nothing but the outside-point count was written. */
#define GS2M_TSDF_POOL_FULL 1

/* Bytes of the touch workspace (per domain) and of the mesh workspace (per `n_blocks` blocks in use), HOST outputs. */
int gs2m_tsdf_workspace_bytes(const int* dom, int n_blocks, long long* touch_bytes, long long* mesh_bytes);

/* The AABB of the view's back-projected points (the touch rule's points, before the trunc padding) merged into aabb (device
 * int[6]: min x y z, max x y z as order-preserving integer keys of the floats; the caller fills it with INT_MAX x 3,
 * INT_MIN x 3 before the first view).  key(f) = bits(f) >= 0 ? bits(f) : bits(f) ^ 0x7FFFFFFF. */
int gs2m_tsdf_points_aabb(int W, int H, const float* depth, float depth_trunc, float fx, float fy, float cx, float cy,
                          const float* c2w, int* aabb, void* stream);

/* Touch / allocate for one view.  touch_ws: the touch workspace, ZERO when first used (the call leaves it so).
 * touched_slots: int[capacity].  info (HOST int[4]): [0] blocks in use after the call (POOL_FULL: the count required),
 * [1] blocks the view touched, [2] of them new, [3] points ignored outside the domain. */
int gs2m_tsdf_touch(const int* dom, float voxel, float trunc, int W, int H, const float* depth, float depth_trunc, float fx,
                    float fy, float cx, float cy, const float* c2w, int capacity, int* state, int* index, int* block_coords,
                    int* touched_slots, void* touch_ws, int* info, void* stream);

/* Integrate one view into the `n_touched` blocks listed by the last touch.  color: (H, W, 3) fp32 on 0..255. */
int gs2m_tsdf_integrate(float voxel, float trunc, int W, int H, const float* depth, const float* color, float depth_trunc,
                        float fx, float fy, float cx, float cy, const float* w2c, int n_touched, const int* touched_slots,
                        const int* block_coords, float* tsdf, float* weight, float* color_acc, void* stream);

/* Marching cubes, pass 1: classify every cube of the `n_blocks` blocks in use, count the vertices and triangles, scan.
 * totals (HOST long long[2]): vertices, triangles.  GS2M_ERR_UNSUPPORTED beyond 2^29 vertices. */
int gs2m_tsdf_mesh_count(const int* dom, int n_blocks, const int* index, const int* block_coords, const float* tsdf,
                         const float* weight, void* mesh_ws, long long* totals, void* stream);

/* Pass 2 (after mesh_count on the same workspace, volume unchanged): vertices (V, 3), vertex_colors (V, 3) in 0..1,
 * triangles (F, 3) int32. */
int gs2m_tsdf_mesh_emit(const int* dom, float voxel, int n_blocks, const int* index, const int* block_coords,
                        const float* tsdf, const float* color_acc, void* mesh_ws, long long n_vertices, long long n_triangles,
                        float* vertices, float* vertex_colors, int* triangles, void* stream);

/* Tests: the block coordinates of the `n_blocks` slots in use, copied to HOST int[n_blocks * 3]. */
int gs2m_tsdf_block_coords(int n_blocks, const int* block_coords, int* host_coords, void* stream);

/* ---- post-processing (mesh_post.hip) -------------------------------------------------------------------------------
 *
 * Open3D's cluster_connected_triangles + remove_triangles_by_mask + remove_unreferenced_vertices +
 * remove_degenerate_triangles as the reference's post_process_mesh strings them together; the contract:
 *
 *   Edges       triangle t has the three unordered vertex pairs (min, max) of (v0, v1), (v1, v2), (v2, v0); a degenerate
 *               triangle contributes its pairs as they come, (a, a) included.
 *   Connection  two triangles are connected when they have an equal pair (orientation does not matter; an edge with three
 *               or more triangles connects them all; sharing only a vertex is no connection).  Clusters are the connected
 *               components.
 *   Numbering   clusters are numbered 0 .. C - 1 by increasing smallest triangle index; tri_cluster[t] is the number,
 *               cluster_size[c] the triangle count: both a pure function of `triangles`.
 *   Keep        keep[t] = cluster_size[tri_cluster[t]] >= min_size (the caller chooses min_size: max(n-th largest, 50)).
 *   Compaction  a vertex survives when a kept triangle references it (a degenerate kept triangle counts); survivors keep
 *               their order and are renumbered densely, their colours move with them; a triangle is emitted when it is
 *               kept and its three ids are pairwise different, in input order, with the new ids.
 *   Limits      3 F <= 0xFFFFFFF0 and V < 2^31 (else GS2M_ERR_UNSUPPORTED); vertex ids are int32.  A triangle (kept or
 *               not) with an id outside [0, V) makes cluster_triangles and compact return GS2M_ERR_INVALID_ARG; no kernel
 *               indexes with an id it has not tested.  F = 0 and V = 0 are valid and launch nothing.
 *
 * Integer atomics only where their order cannot change the result (the union-find hooks the larger root under the smaller,
 * so a cluster's root is its smallest triangle; integer counts): two runs are bitwise identical.
 * Workspaces (the caller's, as everything here): the cluster workspace is 104 bytes per triangle -- eight u32 arrays over
 * the 3 F edge slots (the pairs, the second sort's input, the sort's ping-pong buffers) and a u64 per triangle for the scan
 * -- plus the radix sort's look-back rows, 3.1 bytes per triangle: 107.1 in all, 3.53 GB at F = 33 M; the compaction
 * workspace is 9 bytes per vertex and 8 per triangle (0.42 GB at V = 17 M, F = 33 M).  tri_cluster serves as the union-find's parent array during the call. */

/* HOST outputs; either pointer may be NULL (not asked for). */
int gs2m_mesh_post_workspace_bytes(long long n_vertices, long long n_triangles, long long* cluster_bytes,
                                   long long* compact_bytes);

/* triangles (F, 3) int32; ws: the cluster workspace.  tri_cluster int[F], cluster_size int[F] (the first C valid, the rest
 * 0), n_clusters HOST = C; waits for the stream. */
int gs2m_mesh_cluster_triangles(long long n_vertices, long long n_triangles, const int* triangles, void* ws, int* tri_cluster,
                                int* cluster_size, long long* n_clusters, void* stream);

/* keep[t] = cluster_size[tri_cluster[t]] >= min_size (0 for a number outside [0, F)); cluster_size int[F]. */
int gs2m_mesh_keep_clusters(long long n_triangles, const int* tri_cluster, const int* cluster_size, int min_size,
                            unsigned char* keep, void* stream);

/* ws: the compaction workspace.  colors / out_colors may be NULL.  out_vertices, out_colors (V, 3) and out_triangles (F, 3)
 * are sized by the caller for the input's counts; totals (HOST long long[2]) = surviving vertices, emitted triangles: the
 * rows written.  Waits for the stream. */
int gs2m_mesh_compact(long long n_vertices, long long n_triangles, const float* vertices, const float* colors,
                      const int* triangles, const unsigned char* keep, void* ws, float* out_vertices, float* out_colors,
                      int* out_triangles, long long* totals, void* stream);

#ifdef __cplusplus
}
#endif

#endif
