/* gs2m_meshtransfer.h -- C ABI of the detail transfer between two meshes of one surface (mesh_bvh.hip), part of
 * libgs2m_raster.so: for every point of a target (the texels of a simplified mesh's atlas) a short ray along the normal, forth
 * and back, finds the SOURCE mesh (the full one) and copies what it carries there -- a high-to-low bake.  It is the first user of
 * gs2m_bvh_closest; every term below that gs2m_meshao.h defines (Products, Triangle, Dead, Candidate, Facing, Answer) is that
 * header's.  DESIGN.md §27 has the plan; tests/mesh_transfer_ref.py restates this contract in numpy.  The reference has no such
 * step: the contract is this project's own.  fp64, evaluated as written (-ffp-contract=off); the one rounding to float is named.
 *
 *   Skipped      a point p is skipped when owner[p] < 0 (owner == NULL: none is), when dot(n, n) is not > 0 or not finite, or
 *                when a coordinate of p is not finite: hit_tri[p] = -1, offset[p] = 0, its row of `values` is left alone.
 *   Rays         n is the point's unit normal (the CALLER normalises).  F = closest(p, +n, tmin = 0, tmax = distance, no skip,
 *                facing = two_sided ? 0 : -1); B = closest(p, -n, 0, distance, no skip, facing = two_sided ? 0 : +1).  One-sided
 *                thus counts only source triangles whose cross(e1, e2) points to the side of n, from either ray.
 *   Choice       B wins iff it has a hit and (F has none or t_B < t_F); on a tie F wins.  offset[p] = +t_F or -t_B, hit_tri[p] =
 *                the winner's triangle.  Without any hit hit_tri[p] = -1, offset[p] = 0 and the row is left alone.  (The kernel
 *                runs B with tmax = min(distance, t_F), which cannot change the choice; the rule here is the definition.)
 *   Values       on a hit with the corners i0, i1, i2 of the triangle and (u, v) of the Answer, w = (1 - u) - v: channel
 *                c < channels of the row gets (float)((w a0 + u a1) + v a2), a_k = (double)src_attributes[i_k][c].  With
 *                want_normal the channels channels .. channels + 2 get the same expression of src_normals' rows, or with
 *                src_normals == NULL cross(e1, e2) of the Triangle paragraph's e1, e2, rounded to float.  Neither is normalised
 *                (gs2m_texture_normals takes a normal of any length).  The other columns of the row, up to stride, are left alone.
 *   Independence a point's result depends on that point alone: any split of the points over calls gives the same bits.
 *
 * Every buffer is the caller's and on the device.  No call waits for the stream.  Return GS2M_OK (0) or a negative GS2M_ERR_*
 * code (gs2m_raster.h): what gs2m_bvh_occluded returns for the mesh and the tree, and GS2M_ERR_INVALID_ARG, without a launch,
 * for a negative n_points, a missing points, normals or hit_tri, a missing values when channels + 3 want_normal > 0, a distance
 * that is NaN or negative (+inf is allowed), channels < 0, channels > 0 without src_attributes, stride < channels + 3 want_normal.
 * n_src_triangles == 0: every point misses. */
#ifndef GS2M_MESHTRANSFER_H
#define GS2M_MESHTRANSFER_H

#ifdef __cplusplus
extern "C" {
#endif

/* bvh: gs2m_bvh_build's, of the SOURCE mesh src_verts double (n_src_verts, 3), src_triangles int (n_src_triangles, 3).  points,
 * normals: double (n_points, 3); owner: int (n_points) or NULL; src_attributes: float (n_src_verts, channels) or NULL;
 * src_normals: double (n_src_verts, 3) or NULL (the face normal); values: float (n_points, stride); hit_tri: int (n_points);
 * offset: double (n_points) or NULL.  One lane per point casts both rays. */
int gs2m_mesh_transfer(const void* bvh, long long bvh_bytes, long long n_src_verts, const double* src_verts, long long n_src_triangles,
                       const int* src_triangles, long long n_points, const double* points, const double* normals, const int* owner,
                       double distance, int two_sided, int channels, const float* src_attributes, const double* src_normals, int want_normal,
                       int stride, float* values, int* hit_tri, double* offset, void* stream);

#ifdef __cplusplus
}
#endif

#endif
