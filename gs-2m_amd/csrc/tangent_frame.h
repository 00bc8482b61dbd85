// The tangent frame of a point of a textured triangle, and the normal-map encode and decode in it (the Tangent frame paragraph of
// include/gs2m_meshbake.h).  Plain C++ for host and device: mesh_bake.hip encodes with it, mesh_view.hip decodes
// with it, and it compiles without HIP (tools/tangent_frame_check.cpp runs it under the host sanitizers).  fp64, as written
// (-ffp-contract=off), dot(a, b) = (a0 b0 + a1 b1) + a2 b2.
//
// Handedness.  The chart maps (u, v) to the surface, p(u, v) = a + d_u (u - u_a) + d_v (v - v_a), so e1 = d_u du1 + d_v dv1 and
// e2 = d_u du2 + d_v dv2, whose solution is d_u = (e1 dv2 - e2 dv1) / det, d_v = (e2 du1 - e1 du2) / det, and
// cross(d_u, d_v) = cross(e1, e2) / det.  With det > 0 and N on the side of Nf = cross(e1, e2), (T, cross(N, T), N) is a right-handed
// frame whose second axis has a positive component along d_v: the direction of growing v.  v is measured from the top row, and a
// glTF normal map's green axis points up the image, towards decreasing v: B = -cross(N, T), w = -1.  Half 0 of an atlas cell has
// (du1, dv1) = (L / W, 0), (du2, dv2) = (0, L / H), half 1 the negatives of both: det = L^2 / (W H) > 0 for both (a rotation by
// 180 degrees, not a reflection), so w is -1 for every triangle of the atlas.  A mirrored chart (det < 0) would need w = +1; the
// atlas makes none and this frame does not support one.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define TF_HD __host__ __device__ __forceinline__
#else
#define TF_HD inline
#endif

struct TangentFrame {
    double T[3], B[3], N[3];
    int valid;
};

TF_HD double tf_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
TF_HD void tf_cross(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1], o[1] = a[2] * b[0] - a[0] * b[2], o[2] = a[0] * b[1] - a[1] * b[0];
}
TF_HD bool tf_finite3(const double* a) { return isfinite(a[0]) && isfinite(a[1]) && isfinite(a[2]); }
// o = a / |a|; false (o untouched) when a is zero or not finite, or its unit is not
TF_HD bool tf_unit(const double* a, double* o) {
    const double s = tf_dot(a, a);
    if (!(s > 0.0) || !tf_finite3(a)) return false;
    const double len = sqrt(s);
    const double u[3] = {a[0] / len, a[1] / len, a[2] / len};
    if (!tf_finite3(u)) return false;
    o[0] = u[0], o[1] = u[1], o[2] = u[2];
    return true;
}

// a, b, c: the corners in world space; uv: the triangle's three UVs (u_a, v_a, u_b, v_b, u_c, v_c), the fp32 values widened;
// Nin: the shading normal at the point.  An invalid frame has T = B = 0 and N = the unit of Nin, or (0, 0, 1) where there is none.
TF_HD void tangent_frame(const double* a, const double* b, const double* c, const double* uv, const double* Nin, TangentFrame* F) {
    const double e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double du1 = uv[2] - uv[0], dv1 = uv[3] - uv[1], du2 = uv[4] - uv[0], dv2 = uv[5] - uv[1];
    const double det = du1 * dv2 - du2 * dv1;
    double Nf[3], Uf[3], Un[3];
    tf_cross(e1, e2, Nf);
    const bool face = tf_unit(Nf, Uf), own = tf_unit(Nin, Un);
    for (int k = 0; k < 3; k++) F->T[k] = 0.0, F->B[k] = 0.0, F->N[k] = own ? Un[k] : (k == 2 ? 1.0 : 0.0);
    F->valid = 0;
    if (!face) return;
    if (!(own && tf_dot(Un, Nf) > 0.0))
        for (int k = 0; k < 3; k++) F->N[k] = Uf[k];
    if (det == 0.0 || !isfinite(det)) return;
    const double du[3] = {(e1[0] * dv2 - e2[0] * dv1) / det, (e1[1] * dv2 - e2[1] * dv1) / det, (e1[2] * dv2 - e2[2] * dv1) / det};
    const double along = tf_dot(F->N, du);
    const double t[3] = {du[0] - F->N[0] * along, du[1] - F->N[1] * along, du[2] - F->N[2] * along};
    double T[3], x[3];
    if (!tf_unit(t, T)) return;
    tf_cross(F->N, T, x);
    for (int k = 0; k < 3; k++) F->T[k] = T[k], F->B[k] = -x[k];
    F->valid = 1;
}

// the world normal n in the frame: m, unit, m_z >= 0; (0, 0, 1) for an invalid frame, a zero or non-finite n, or a zero m
TF_HD void tangent_encode(const TangentFrame& F, const double* n, double* m) {
    double u[3];
    m[0] = 0.0, m[1] = 0.0, m[2] = 1.0;
    if (!F.valid || !tf_unit(n, u)) return;
    double q[3] = {tf_dot(u, F.T), tf_dot(u, F.B), tf_dot(u, F.N)};
    q[2] = q[2] > 0.0 ? q[2] : 0.0;
    tf_unit(q, m);
}

TF_HD unsigned char tangent_byte(double m) { return (unsigned char)floor(255.0 * (0.5 * m + 0.5) + 0.5); }

// a normal-map value m (byte / 255 * 2 - 1 per component, or a bilinear mix of such) to the world normal n, unit; N for an invalid
// frame or where the sum is zero or not finite
TF_HD void tangent_decode(const TangentFrame& F, const double* m, double* n) {
    n[0] = F.N[0], n[1] = F.N[1], n[2] = F.N[2];
    if (!F.valid) return;
    const double s[3] = {(F.T[0] * m[0] + F.B[0] * m[1]) + F.N[0] * m[2], (F.T[1] * m[0] + F.B[1] * m[1]) + F.N[1] * m[2],
                         (F.T[2] * m[0] + F.B[2] * m[1]) + F.N[2] * m[2]};
    tf_unit(s, n);
}
