// The per-point arithmetic of tnt_clouds.hip that needs no device: the eigenvector of a symmetric 3 x 3 matrix's smallest
// eigenvalue, the normal's sign rule and the colour-table index (include/gs2m_tnt.h states them).  Host and device alike, so
// that a host program can check them without a GPU.  Compiled with -ffp-contract=off like every fp64 unit of the evaluators.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GS2M_HD __host__ __device__ __forceinline__
#else
#define GS2M_HD static inline
#endif

constexpr int GS2M_JACOBI_SWEEPS = 8;  // a 3 x 3 converges to fp64 in 4 or 5; the count is fixed, not tested

// One Jacobi rotation in the (p, q) plane of a symmetric matrix: app, aqq, apq its entries there, arp / arq the third index's
// couplings; vp, vq the eigenvector matrix's columns p and q.  The smaller root t of t^2 + 2 theta t - 1 = 0 keeps |angle| <= pi / 4.
GS2M_HD void gs2m_jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double vp[3], double vq[3]) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));  // theta^2 = inf: t = 0
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp;
    arq = rq;
    for (int k = 0; k < 3; k++) {
        const double a = c * vp[k] - s * vq[k], b = s * vp[k] + c * vq[k];
        vp[k] = a;
        vq[k] = b;
    }
}

// n: the normal of the covariance (c00 c01 c02; . c11 c12; . . c22) under the header's rules.  Any common positive factor of
// the six entries is immaterial: they are divided by their largest magnitude first.
GS2M_HD void gs2m_normal_of_covariance(double c00, double c01, double c02, double c11, double c12, double c22, double n[3]) {
    n[0] = 0.0;
    n[1] = 0.0;
    n[2] = 1.0;
    const double big = fmax(fmax(fabs(c00), fabs(c11)), fmax(fabs(c22), fmax(fabs(c01), fmax(fabs(c02), fabs(c12)))));
    if (!(big > 0.0) || !(big < __builtin_huge_val())) return;  // zero, NaN or infinite
    c00 /= big, c01 /= big, c02 /= big, c11 /= big, c12 /= big, c22 /= big;
    double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};
    for (int sweep = 0; sweep < GS2M_JACOBI_SWEEPS; sweep++) {
        gs2m_jacobi_rotate(c00, c11, c01, c02, c12, v0, v1);
        gs2m_jacobi_rotate(c00, c22, c02, c01, c12, v0, v2);
        gs2m_jacobi_rotate(c11, c22, c12, c01, c02, v1, v2);
    }
    double x = v0[0], y = v0[1], z = v0[2], lam = c00;  // the smallest eigenvalue's column; the lower index among equals
    if (c11 < lam) x = v1[0], y = v1[1], z = v1[2], lam = c11;
    if (c22 < lam) x = v2[0], y = v2[1], z = v2[2], lam = c22;
    const double len = sqrt((x * x + y * y) + z * z);
    if (!(len > 0.0) || !(len < __builtin_huge_val())) return;
    x /= len, y /= len, z /= len;
    const bool flip = z != 0.0 ? z < 0.0 : (x != 0.0 ? x < 0.0 : y < 0.0);
    n[0] = flip ? -x : x;
    n[1] = flip ? -y : y;
    n[2] = flip ? -z : z;
}

// the hot_r table's row of a distance that is not NaN: min(trunc(x * 256), 255), x = min(d, cap) / cap; below 0: row 0
GS2M_HD int gs2m_color_row(double d, double cap) {
    const double x = (d < cap ? d : cap) / cap;
    const double r = x * 256.0;
    return r >= 255.0 ? 255 : (r > 0.0 ? (int)r : 0);
}
