/* gs2m_atlas.h -- C ABI of the triangle atlas (mesh_atlas.hip), part of libgs2m_raster.so: a texture layout in which every
 * triangle has a right-isosceles chart of its own.  The layout is a pure function of the mesh and of one number, `density`
 * (texels per world unit); every decision is taken in integers, there is no search.  DESIGN.md §22 has the plan;
 * tests/mesh_texture_ref.py restates this contract in fp64 numpy.  Vertices and normals are (V, 3) fp64 as in gs2m_meshbake.h,
 * triangles (F, 3) int32.  The contract:
 *
 *   Class       e = the longest edge of the triangle, max over the three edges d of sqrt((d0 d0 + d1 d1) + d2 d2), fp64.  The
 *               side s is the smallest of 8, 16, 32, 64, 128, 256 with (double)(s - 4) >= e * density, else 256 (a longer edge
 *               is sampled more coarsely).  s = 8 << k names the class k = 0 .. 5.  A zero-area triangle is legal (side 8 when
 *               its corners coincide).  A corner that is not finite or a vertex index outside [0, V): GS2M_ERR_INVALID_ARG,
 *               found by the class kernel and one read-back; `density` must be finite and > 0.
 *   Order       triangles are stably sorted by class, largest first (the project's stable radix sort on the 3-bit key 5 - k).
 *               order[q] = the triangle at sorted position q; start_k = the number of triangles of a larger class.  The
 *               triangle at position q has rank r = q - start_k in its class and goes to cell r / 2, half r % 2.
 *   Placement   in units of 8 x 8 texels a class-k cell covers 4^k units; class k has ceil(hist_k / 2) cells.  base_k = the
 *               units of all larger classes (a multiple of 4^k).  Cell m of class k sits at the unit offset base_k + m 4^k,
 *               and its unit coordinates are the Morton decode of that offset: x from the even bits (0, 2, ...), y from the
 *               odd ones.  total = the units of all classes.  width = 8 * 2^j with j the smallest value such that
 *               4^j >= total; height = width / 2 when j >= 1 and 2 total <= 4^j (the first half of the Z-curve is the upper
 *               half of the square), else width.  width > GS2M_ATLAS_MAX_WIDTH: GS2M_ERR_UNSUPPORTED.  F = 0 is valid:
 *               width = height = 0, nothing is launched or written besides hist, bases and dims.
 *   Chart       in cell-local texel coordinates, texel (i, j) having its centre at (i + 0.5, j + 0.5), and L = s - 4: half 0
 *               maps the corners a, b, c to (1, 1), (1 + L, 1), (1, 1 + L); half 1 to (s - 1, s - 1), (s - 1 - L, s - 1),
 *               (s - 1, s - 1 - L).  Texel (i, j) belongs to half 0 when i + j <= s - 1, else to half 1.
 *               uv = (cell origin + local) / (width, height): the integer sum, divided in fp64, rounded once to fp32; v is
 *               measured from the top row, as glTF measures it.
 *   Texel       (X, Y) of the atlas lies in unit (X / 8, Y / 8), whose Morton code is compared with the classes' bases: that
 *               gives class, cell, local (i, j), half, rank and through `order` the owner.  A rank >= hist_k (the half after
 *               an odd count) and a unit >= total are empty: owner -1, interior 0, point and normal 0.  For an owned texel,
 *               with (i', j') = (i, j) for half 0 and (s - 1 - i, s - 1 - j) for half 1:
 *               l1 = ((2 i' - 1) 0.5) / L, l2 = ((2 j' - 1) 0.5) / L, l0 = (1 - l1) - l2 -- the centre's barycentrics;
 *               interior = 2 i' - 1 >= 0 && 2 j' - 1 >= 0 && (2 i' - 1) + (2 j' - 1) <= 2 L (a centre on an edge is inside);
 *               then l_k = max(l_k, 0) and l_k = l_k / ((l0 + l1) + l2): a skirt texel takes a point of the triangle.
 *               point = (l0 a + l1 b) + l2 c per coordinate.  normal = (l0 Na + l1 Nb) + l2 Nc of the vertex normals; with
 *               normals == NULL, or where that sum is zero or not finite, the face normal cross(b - a, c - a) (not
 *               normalised; zero for a zero-area triangle, which the bake then never sees).
 *               An `order` entry outside [0, F) or a triangle naming a vertex outside [0, V) makes the texel empty.
 *
 * The four bilinear taps of any point of a chart, corners and hypotenuse included, are texels of the chart's half (the skirt is one
 * texel wide on the legs and at least one wide along the hypotenuse); mip levels above 0 are not covered.
 * Every buffer is the caller's; device pointers except `bytes`, `hist`, `bases`, `dims` (HOST).  count and build wait for the
 * stream.  Integer atomics only (the class histogram).  An error leaves every output untouched.  Return GS2M_OK (0) or a
 * negative GS2M_ERR_* code (gs2m_raster.h).  F <= 2^30 - 1 (the radix sort's bound), V <= 2^31 - 1: else GS2M_ERR_UNSUPPORTED.
 * Workspace: 20 bytes per triangle and the sort's look-back rows. */
#ifndef GS2M_ATLAS_H
#define GS2M_ATLAS_H

#ifdef __cplusplus
extern "C" {
#endif

#define GS2M_ATLAS_CLASSES 6
#define GS2M_ATLAS_MAX_WIDTH 16384 /* the PNG encoder's row limit at three channels */

/* HOST output. */
int gs2m_atlas_workspace_bytes(long long n_triangles, long long* bytes);

/* The probe for a target size.  hist (HOST long long[6]): triangles per class k; dims (HOST int[2]): width, height. */
int gs2m_atlas_count(long long n_vertices, long long n_triangles, const double* vertices, const int* triangles, double density,
                     void* ws, long long* hist, int* dims, void* stream);

/* cells: int (F, 4) = cell origin x, y in texels, side, half; uvs: float (F, 3, 2); order: int (F); bases (HOST long long[6]):
 * base_k in units. */
int gs2m_atlas_build(long long n_vertices, long long n_triangles, const double* vertices, const int* triangles, double density,
                     void* ws, int* cells, float* uvs, int* order, long long* hist, long long* bases, int* dims, void* stream);

/* Texels row0 .. row0 + n_rows - 1 of the atlas of `hist` (HOST), whose size must be width x height (else
 * GS2M_ERR_INVALID_ARG, as when hist does not sum to n_triangles).  owner: int (n_rows, width); interior: unsigned char
 * (n_rows, width); points, tnormals: double (n_rows, width, 3).  normals may be NULL. */
int gs2m_atlas_texels(long long n_vertices, const double* vertices, const double* normals, long long n_triangles,
                      const int* triangles, const int* order, const long long* hist, int width, int height, int row0, int n_rows,
                      int* owner, unsigned char* interior, double* points, double* tnormals, void* stream);

#ifdef __cplusplus
}
#endif

#endif
