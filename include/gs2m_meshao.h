/* gs2m_meshao.h -- C ABI of the mesh ray casting (mesh_bvh.hip), part of libgs2m_raster.so: a bounding-volume hierarchy over a
 * triangle mesh, built on the device, a stackless any-hit traversal with ambient occlusion as its first user, and a closest-hit
 * query on the same walk (its first user: gs2m_meshtransfer.h).  DESIGN.md §26 and §27 have the kernel plan; tests/mesh_ao_ref.py
 * and tests/mesh_transfer_ref.py restate this contract in fp64 numpy.  The reference has no such step: the
 * contract is this project's own.  Every expression is fp64 and evaluated as written (-ffp-contract=off) with + - * / and
 * comparisons alone, so the host, the device and numpy give the same bits.  Vertices are double (n_verts, 3), triangles int
 * (n_triangles, 3), the layout gs2m_meshbake_accumulate takes.
 *
 *   Products     dot(a, b) = (a0 b0 + a1 b1) + a2 b2; cross(a, b) = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0).
 *   Triangle     a ray (o, d, tmin, tmax) against the corners a, b, c: e1 = b - a, e2 = c - a, P = cross(d, e2), det = dot(e1, P);
 *                miss when det == 0 or det is not finite.  T = o - a, u = dot(T, P) / det; miss unless u >= 0 && u <= 1.
 *                Q = cross(T, e1), v = dot(d, Q) / det; miss unless v >= 0 && u + v <= 1.  t = dot(e2, Q) / det; hit iff
 *                t > tmin && t <= tmax.  Two-sided.  NOT watertight: a ray that passes exactly through an edge two triangles
 *                share may miss both of them.
 *   Dead         a triangle with an index outside [0, n_verts) or a corner that is not finite is dead: it is never hit, it has
 *                an empty box (below) and leaves every other box alone.  A zero-area triangle has det == 0 for the rays that
 *                matter and dies in the test itself.
 *   Occluded     a ray is occluded iff it hits any live triangle other than its `skip` triangle (skip < 0 or NULL: none is
 *                skipped).  Any-hit over a set does not depend on the order: the answer of the traversal is DEFINED as the
 *                answer of the loop over all triangles, bit for bit, and the tests hold it to that.
 *
 *   Hierarchy    an LBVH over all n = n_triangles triangles, dead ones included (no count comes back to the host; both calls
 *                are asynchronous).  Centroid ((a + b) + c) / 3 per coordinate; the bounds lo, hi of the live centroids by a
 *                fixed-order min / max; q_k = (int)((centroid_k - lo_k) / (hi_k - lo_k) * 1023), clamped to 0 .. 1023, 0 where
 *                hi_k == lo_k; the code is the 30-bit Morton interleave of (q_x, q_y, q_z), x highest; a dead triangle takes
 *                the code 2^30 and sorts behind every live one.  gs2m_radix_sort_pairs (31 bits, stable) orders (code,
 *                triangle), so equal codes stay in triangle order; the split search (Karras, "Maximizing parallelism in the
 *                construction of BVHs, octrees, and k-d trees", 2012) compares the 64-bit keys code << 32 | sorted position,
 *                so n identical triangles still give a tree of depth ceil(log2 n).  Boxes are refitted bottom up with
 *                integer arrival counters; a parent is min / max (by comparison) of its left and its right child in that
 *                order, whichever arrived first.  No floating-point atomics: two builds give the same bytes.
 *   Layout       the first (2 n - 1) * 64 bytes of the buffer are the nodes, gs2m_bvh_node below: the n - 1 internal nodes
 *                first (node 0 is the root), then the n leaves, leaf n - 1 + i holding the i-th triangle of the sorted
 *                order.  n = 1: the one leaf is node 0.  A box is the exact fp64 min / max of its triangles' corners; an
 *                empty box (a dead triangle, a subtree of dead triangles) is lo = +inf, hi = -inf.  Internal: left, right =
 *                the child nodes; leaf: left = the triangle, right = -1.  parent = -1 at the root.  miss = the node
 *                traversal continues with when the box is missed or the leaf is done: the next subtree in depth-first
 *                order, -1 at the end.  What follows the nodes is the builder's scratch, of no defined content.
 *   Traversal    node = 0; while node >= 0: box missed -> node = miss; leaf -> test its triangle, leave at a hit, node = miss;
 *                else node = left.  No stack and no per-thread scratch, whatever the depth.
 *   Box test     conservative: it may accept a box the ray misses, never the other way round.  An empty box is rejected.
 *                Per axis, the slab [lo, hi] is first widened by pad = 2^-30 ((|lo| + |hi|) + |o_k|) on both sides.
 *                d_k == 0: rejected iff o_k lies outside the widened slab (no division, no 0 * inf).  1 / d_k infinite (a
 *                subnormal d_k): the axis constrains nothing.  Else the entry and exit parameters (lo - o_k) (1 / d_k),
 *                (hi - o_k) (1 / d_k) narrow [tmin, tmax] to [te, tx] by comparisons that a NaN never wins, and the box is
 *                rejected only when te > tx && te - tx > 2^-40 (|te| + |tx|).  The widening exceeds the rounding of the slab
 *                arithmetic (2^-52 relative, cancellation in lo - o_k included) by 2^22 and the slack that of the products by
 *                2^12, so a point of the ray that lies in the box in exact arithmetic is never rejected; the same margin
 *                covers the rounding of the triangle test's own t, u, v as long as |det| is above 2^-20 of the products
 *                it is made of (nearer to a triangle's plane than that a ray stays inside the widened slab of the box for a
 *                long stretch of t, which makes the test more lenient, not less: the tests' grazing family, |det| down to
 *                1e-13 of its products, is held to equality).  A ray in the plane of a box face, a ray grazing a box edge and a hit at exactly tmax are
 *                inside the widened box.  A ray with a NaN anywhere accepts every box and misses every triangle.
 *
 *   Candidate    (gs2m_bvh_closest) e1, e2, P, det, u, Q, v, t exactly as in the Triangle paragraph: the same products in the same
 *                order, the same misses on det, u and v, the same Dead and skip rules.  The range is CLOSED AT BOTH ENDS: a
 *                triangle is a candidate iff t >= tmin && t <= tmax, so a ray that starts exactly on the surface (t == 0 with
 *                tmin = 0) finds it.  This predicate belongs to the closest-hit query alone; Occluded keeps t > tmin.
 *   Facing       det = -dot(d, cross(e1, e2)).  facing == 0 accepts both signs of det; facing == +1 only det > 0 (the ray meets
 *                the side cross(e1, e2) points out of); facing == -1 only det < 0.  Any other value: GS2M_ERR_INVALID_ARG.
 *   Answer       of all candidates the one with the smallest t, among equal t the one with the smallest triangle index:
 *                tri, t, uv = (u, v) of that candidate; without a candidate tri = -1, t = +inf, u = v = 0.  This does not depend
 *                on the order of visits: the answer of the traversal is DEFINED as the answer of the loop over all triangles,
 *                bit for bit, in all four outputs.
 *   Closest      the Traversal above with tmax replaced, for the box test and the range alike, by the best t so far; a leaf is
 *   traversal    never left early.  A candidate replaces the best when t < best, or t == best and its index is smaller.  The order
 *                stays fixed (left first, miss links; not front to back).  The box test is closed at tmax and padded -- "a hit
 *                at exactly tmax is inside the widened box" -- and the best t is the t of a triangle test, whose rounding the
 *                margin argument of the Box test paragraph covers: the box of a triangle whose t equals the best so far is not
 *                rejected, so an equal-t neighbour with a smaller index is never culled, and neither is any nearer candidate.
 *                The same guards: every index is tested before it is followed, the walk stops after 2 n - 1 nodes, a ray with
 *                a NaN finds nothing.
 *
 *   mix32        x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 on 32-bit unsigned x.
 *   AO           per point p of the call, with its unit normal n (the CALLER normalises: the kernel takes no square root):
 *                r = mix32(the low 32 bits of (index0 + p + seed)) % R picks one of the R tables of K local directions
 *                (z up).  Frame (Duff et al., "Building an orthonormal basis, revisited", 2017): s = copysign(1, n_z),
 *                a = -1 / (s + n_z), b = (n_x n_y) a, T = (1 + ((s n_x) n_x) a, s b, -(s n_x)),
 *                B = (b, s + (n_y n_y) a, -n_y).  For each direction l of the table: d_k = (T_k l_x + B_k l_y) + n_k l_z,
 *                o_k = p_k + n_k bias, tmin = 0, tmax = radius (+inf allowed), skip = skip[p].  visible[p] = the number of
 *                the K rays that are not occluded.  visible[p] = K, and nothing is walked, for a point with skip[p] < 0
 *                ("no point here": the atlas's owner < 0), with dot(n, n) not > 0 or not finite, or with a coordinate that
 *                is not finite (no ray from there hits anything under the test above).  A point's result depends on
 *                index0 + p alone: splitting the points over two calls with the matching index0 gives the same bits.
 *   Occlusion    orm[p][0] = floor(255 (visible[p] / K) + 0.5) for texels with owner[p] >= 0, the division in fp64; every
 *                other byte of orm is left alone (gs2m_texture_pack wrote 255 there: glTF's occlusionTexture reads R).
 *
 * Every buffer is the caller's and on the device, except `bytes` (HOST).  No call waits for the stream.  Return GS2M_OK (0) or
 * a negative GS2M_ERR_* code (gs2m_raster.h): GS2M_ERR_INVALID_ARG, without a launch, for a negative count, a missing buffer,
 * a bvh buffer smaller than gs2m_bvh_bytes says, K or R < 1, a NaN tmin, tmax, bias or radius, a facing outside -1 .. 1;
 * GS2M_ERR_UNSUPPORTED for
 * n_triangles >= 2^30 (the radix sort's bound) or n_verts >= 2^31.  The traversal tests every node and triangle index it
 * reads against the counts it was given before it follows it, and stops after 2 n - 1 nodes. */
#ifndef GS2M_MESHAO_H
#define GS2M_MESHAO_H

#ifdef __cplusplus
extern "C" {
#endif

#define GS2M_BVH_NODE_BYTES 64

typedef struct gs2m_bvh_node {
    double lo[3], hi[3];
    int left, right, miss, parent;
} gs2m_bvh_node;

/* HOST output: the size of the buffer of a mesh of n_triangles (nodes + build scratch, about 0.19 KB per triangle). */
int gs2m_bvh_bytes(long long n_triangles, long long* bytes);

/* Builds the hierarchy into bvh.  n_triangles == 0 is valid and launches nothing. */
int gs2m_bvh_build(long long n_verts, const double* verts, long long n_triangles, const int* triangles, void* bvh,
                   long long bvh_bytes, void* stream);

/* origins, dirs: double (n_rays, 3); skip: int (n_rays) or NULL; hit: unsigned char (n_rays), 1 = occluded.  One lane per ray.
 * bvh: gs2m_bvh_build's, of the same mesh. */
int gs2m_bvh_occluded(const void* bvh, long long bvh_bytes, long long n_verts, const double* verts, long long n_triangles,
                      const int* triangles, long long n_rays, const double* origins, const double* dirs, double tmin, double tmax,
                      const int* skip, unsigned char* hit, void* stream);

/* The closest hit per ray (Candidate, Facing, Answer): origins, dirs, skip as above; tri: int (n_rays); t: double (n_rays);
 * uv: double (n_rays, 2).  One lane per ray.  n_triangles == 0: every ray misses. */
int gs2m_bvh_closest(const void* bvh, long long bvh_bytes, long long n_verts, const double* verts, long long n_triangles,
                     const int* triangles, long long n_rays, const double* origins, const double* dirs, double tmin, double tmax,
                     const int* skip, int facing, int* tri, double* t, double* uv, void* stream);

/* points, normals: double (n_points, 3); skip: int (n_points) or NULL; dirs: double (R, K, 3); visible: int (n_points). */
int gs2m_bvh_ao(const void* bvh, long long bvh_bytes, long long n_verts, const double* verts, long long n_triangles,
                const int* triangles, long long n_points, const double* points, const double* normals, const int* skip, int R, int K,
                const double* dirs, double bias, double radius, long long index0, long long seed, int* visible, void* stream);

/* owner, visible: int (n_texels); orm: unsigned char (n_texels, 3) (see Occlusion). */
int gs2m_texture_occlusion(long long n_texels, const int* owner, const int* visible, int K, unsigned char* orm, void* stream);

#ifdef __cplusplus
}
#endif

#endif
