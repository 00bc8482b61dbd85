/* gs2m_simplify.h -- C ABI of the mesh simplification (mesh_simplify.hip), part of libgs2m_raster.so: vertex clustering on a
 * uniform lattice with quadric placement (Lindstrom, "Out-of-core simplification of large polygonal models", 2000).
 * DESIGN.md §21 has the kernel plan; tests/mesh_simplify_ref.py restates this contract in fp64 numpy.  The contract:
 *
 *   Cells       vertex v lies in the cell (floor(x / cell), floor(y / cell), floor(z / cell)): division and floor in fp64, of
 *               the fp32 coordinate widened.  The lattice is anchored at the world origin (adding far-away geometry moves no
 *               cell); indices are taken relative to the smallest occupied index per axis; the centre of a cell is
 *               (index + 0.5) * cell in fp64, index the absolute one.
 *   Limits      `cell` finite and > 0, every coordinate finite, every triangle id in [0, V): else GS2M_ERR_INVALID_ARG, and
 *               no kernel indexes with an id it has not tested.  More than 2^21 cells along an axis (or an index beyond
 *               2^52, where fp64 no longer tells cells apart): GS2M_ERR_UNSUPPORTED, before any sort is launched.
 *               V < 2^31 and 3 F <= 0xFFFFFFF0 as in gs2m_mesh.h, and max(V, 3 F) < 2^30, the radix sort's bound (else
 *               GS2M_ERR_UNSUPPORTED).  V = 0 or F = 0 is valid, launches nothing, writes no array and gives totals = {0, 0}.
 *               An error leaves every output array untouched.
 *   Quadric     of a cell: A (3 x 3 symmetric) and b (3), fp64, relative to the cell's centre, summed over every input
 *               triangle with at least one corner in the cell -- once per distinct cell, however many of its corners lie
 *               there.  With p_i the corners minus the centre (fp64) and n = (p1 - p0) x (p2 - p0), len = sqrt(n . n):
 *               A_ij += (n_i n_j) / len, b_i += (n_i (-(n . p0))) / len; a triangle with len == 0 adds nothing.
 *   Placement   m = the mean of the cell's vertices minus the centre.  A = U diag(l) U^T by cyclic Jacobi, GS2M_SIMPLIFY_SWEEPS
 *               sweeps over (0,1), (0,2), (1,2), no data-dependent iteration.  lmax = the largest l_i; lmax <= 0: the cell
 *               takes the mean.  Else inv_i = 1 / l_i where l_i > 1e-3 lmax (Lindstrom's constant), else 0;
 *               x = m + U diag(inv) U^T (-b - A m); x is accepted when |x_k| <= cell / 2 on all three axes, otherwise the cell
 *               takes m (which always lies in the cell).  Position = centre + x in fp64, rounded once to fp32.
 *   Attributes  n_channels fp32 channels per vertex, attributes (V, n_channels); weights (V) fp32 >= 0 or NULL (all ones).
 *               A cell's value is sum(w a) / sum(w) (products and sums in fp64), out_weight = sum(w); a cell with
 *               sum(w) == 0 takes sum(a) / n and out_weight = 0.  Both rounded once to fp32.
 *   Summation   every per-cell sum is fp64 in this order.  The cell's elements e_0 .. e_n-1 are its vertices in increasing
 *               input index, or its triangles in increasing input index.  n <= 256: sixteen partials, partial l = 0.0 + e_l +
 *               e_(l+16) + ... left to right; then r_l += r_(l+o) for l < o, o = 8, 4, 2, 1; the sum is r_0.  n > 256: 256
 *               partials, partial t = 0.0 + e_t + e_(t+256) + ...; each run of 64 folds by r_l += r_(l+o), o = 32 .. 1,
 *               and the four results as (w0 + w1) + (w2 + w3).  No floating-point atomics; integer atomics only where
 *               their order cannot change a result.  Two runs are bitwise identical and the result does not depend on
 *               what the workspace held before.
 *   Triangles   every corner is remapped to its cell; a triangle whose three cells are not pairwise different is dropped;
 *               among triangles with the same unordered cell triple the one with the smallest input index stays
 *               (orientation does not distinguish them); survivors are emitted in input order with the input's corner order.
 *   Vertices    a cell survives when an emitted triangle references it; survivors are numbered densely in increasing
 *               (ix, iy, iz) order (gs2m_mesh_compact does the renumbering); vertex_map[v] = the new id of v's cell or -1.
 *
 * Every buffer is the caller's; device pointers except `bytes` and `totals` (HOST).  Both calls wait for the stream.
 * Workspace: 158 + 4 n_channels bytes per vertex (96 of them the cell's mean, A and b), 45 per triangle, 8 per
 * max(V, F) for the scan, and 24 per max(V, 3 F) for the sort's ping-pong and regather arrays, plus the sort's look-back
 * rows: 0.41 KB per vertex on a closed mesh (F = 2 V), 1.6 GB at V = 3.9 M, F = 7.7 M. */
#ifndef GS2M_SIMPLIFY_H
#define GS2M_SIMPLIFY_H

#ifdef __cplusplus
extern "C" {
#endif

#define GS2M_SIMPLIFY_SWEEPS 8
#define GS2M_SIMPLIFY_MAX_AXIS_CELLS (1 << 21)

/* HOST output. */
int gs2m_simplify_workspace_bytes(long long n_vertices, long long n_triangles, int n_channels, long long* bytes);

/* totals (HOST long long[2]) = surviving vertices, emitted triangles of the contract, without placement or attributes. */
int gs2m_simplify_count(long long n_vertices, long long n_triangles, const float* vertices, const int* triangles, double cell,
                        void* ws, long long* totals, void* stream);

/* vertices (V, 3) fp32, triangles (F, 3) int32.  attributes / out_attributes may be NULL with n_channels = 0; weights,
 * out_weight and vertex_map (int[V]) may be NULL.  out_vertices (V, 3), out_attributes (V, n_channels), out_weight (V) and
 * out_triangles (F, 3) are sized for the input's counts; totals = the rows written. */
int gs2m_simplify(long long n_vertices, long long n_triangles, const float* vertices, const int* triangles, int n_channels,
                  const float* attributes, const float* weights, double cell, void* ws, float* out_vertices,
                  float* out_attributes, float* out_weight, int* out_triangles, int* vertex_map, long long* totals,
                  void* stream);

/* Tests and tools: the stage times of the last gs2m_simplify in ms, HOST float[5]: keys + sorts, quadrics, placement,
 * triangle remap + dedupe, compaction.  Measured only after gs2m_simplify_set_timing(1), which brackets every stage with
 * stream synchronisations. */
int gs2m_simplify_set_timing(int on);
int gs2m_simplify_stage_ms(float* ms);

#ifdef __cplusplus
}
#endif

#endif
