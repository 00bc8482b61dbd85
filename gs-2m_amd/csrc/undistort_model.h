// COLMAP's distortion models and their inverse (include/gs2m_undistort.h).  Plain C++ for host and device:
// undistort.hip includes it, and it compiles without HIP (tools/undistort_model_check.cpp runs it under the host sanitizers).
//
// Everything is fp64 and uses only + - * / and comparisons -- no sqrt, no pow, no transcendental -- so that under
// -ffp-contract=off the host, the device and numpy evaluate the same bits.  tests/undistort_ref.py restates every function below
// line by line; the ORDER OF OPERATIONS written here is the contract.
//
//   Models      COLMAP's ids and parameter orders: 0 SIMPLE_PINHOLE f cx cy; 1 PINHOLE fx fy cx cy; 2 SIMPLE_RADIAL f cx cy k1;
//               3 RADIAL f cx cy k1 k2; 4 OPENCV fx fy cx cy k1 k2 p1 p2; 6 FULL_OPENCV fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6.
//               Every other id (the fisheye family, FOV, THIN_PRISM_FISHEYE: they need atan / tan) is refused.
//               All of them are unpacked into one form {fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6} with the missing
//               coefficients 0 and `rational` set for FULL_OPENCV only; `identity` is set for the two pinhole models and for a
//               model whose distortion coefficients are all zero (it is a pinhole camera: no iteration, no rounding).
//
//   distort     (u, v) -> (u', v') on normalised coordinates, and its Jacobian:
//                   u2 = u*u; v2 = v*v; uv = u*v; r2 = u2 + v2; r4 = r2*r2
//                   polynomial:  rad = k1*r2 + k2*r4
//                                g   = k1 + (2*k2)*r2                                          (d rad / d r2)
//                   rational:    r6  = r4*r2
//                                num = ((1 + k1*r2) + k2*r4) + k3*r6;  den = ((1 + k4*r2) + k5*r4) + k6*r6
//                                rad = num/den - 1
//                                dn  = (k1 + (2*k2)*r2) + (3*k3)*r4;   dd  = (k4 + (2*k5)*r2) + (3*k6)*r4
//                                g   = (dn*den - num*dd) / (den*den)
//                   du = (u*rad + (2*p1)*uv) + p2*(r2 + 2*u2);   u' = u + du
//                   dv = (v*rad + (2*p2)*uv) + p1*(r2 + 2*v2);   v' = v + dv
//                   j00 = (((1 + rad) + (2*u2)*g) + (2*p1)*v) + (6*p2)*u        d u' / d u
//                   j01 = ((2*uv)*g + (2*p1)*u) + (2*p2)*v                      d u' / d v  =  d v' / d u  = j10
//                   j11 = (((1 + rad) + (2*v2)*g) + (2*p2)*u) + (6*p1)*v        d v' / d v
//               The radial models are the case p1 = p2 = 0 (the tangential products are then exact zeros).
//
//   undistort   Newton on distort(u, v) = (tu, tv), started at (u, v) = (tu, tv), at most UNDISTORT_MAX_ITER iterations:
//                   (pu, pv, j00, j01, j11) = distort(u, v);  fu = pu - tu;  fv = pv - tv
//                   det = j00*j11 - j01*j01          not finite or == 0: FAIL
//                   su = (j11*fu - j01*fv) / det;    sv = (j00*fv - j01*fu) / det
//                   nu = u - su;  nv = v - sv        not finite: FAIL (u, v keep the last finite iterate)
//                   u = nu;  v = nv
//                   max(|su|, |sv|) <= UNDISTORT_EPS: DONE
//               100 iterations without DONE: FAIL.  `x is finite` is written (x - x) == 0.  The identity models return the input.
//
//   pixels      x = fx*u' + cx, y = fy*v' + cy; normalised u = (x - cx) / fx.
#pragma once

#if defined(__HIPCC__)
#define UNDISTORT_HD __host__ __device__ __forceinline__
#else
#define UNDISTORT_HD inline
#endif

constexpr int UNDISTORT_MAX_ITER = 100;
constexpr double UNDISTORT_EPS = 1e-12;
constexpr int UNDISTORT_MAX_PARAMS = 12;

struct UndistortModel {
    double fx, fy, cx, cy;
    double k1, k2, p1, p2, k3, k4, k5, k6;
    int rational, identity;
};

// Number of parameters of a supported model, 0 for a refused one.
UNDISTORT_HD int undistort_model_params(int model) {
    switch (model) {
        case 0: return 3;
        case 1: return 4;
        case 2: return 4;
        case 3: return 5;
        case 4: return 8;
        case 6: return 12;
        default: return 0;
    }
}

UNDISTORT_HD bool undistort_finite(double x) { return (x - x) == 0.0; }

// params (COLMAP's order) -> the common form.  false for a refused model.
UNDISTORT_HD bool undistort_unpack(int model, const double* p, UndistortModel* m) {
    if (undistort_model_params(model) == 0) return false;
    const bool single = model == 0 || model == 2 || model == 3;  // one focal length in front of the principal point
    m->fx = p[0];
    m->fy = single ? p[0] : p[1];
    m->cx = single ? p[1] : p[2];
    m->cy = single ? p[2] : p[3];
    m->k1 = m->k2 = m->p1 = m->p2 = m->k3 = m->k4 = m->k5 = m->k6 = 0.0;
    m->rational = model == 6;
    if (model == 2) m->k1 = p[3];
    if (model == 3) { m->k1 = p[3]; m->k2 = p[4]; }
    if (model == 4 || model == 6) { m->k1 = p[4]; m->k2 = p[5]; m->p1 = p[6]; m->p2 = p[7]; }
    if (model == 6) { m->k3 = p[8]; m->k4 = p[9]; m->k5 = p[10]; m->k6 = p[11]; }
    m->identity = m->k1 == 0.0 && m->k2 == 0.0 && m->p1 == 0.0 && m->p2 == 0.0 && m->k3 == 0.0 && m->k4 == 0.0 && m->k5 == 0.0 && m->k6 == 0.0;
    return true;
}

// (u, v) -> (u', v') and the Jacobian (j10 = j01), in the order of operations of the comment above
UNDISTORT_HD void undistort_distort_jac(const UndistortModel& m, double u, double v, double* pu, double* pv, double* j00, double* j01,
                                        double* j11) {
    if (m.identity) {
        *pu = u; *pv = v; *j00 = 1.0; *j01 = 0.0; *j11 = 1.0;
        return;
    }
    const double u2 = u * u, v2 = v * v, uv = u * v;
    const double r2 = u2 + v2;
    const double r4 = r2 * r2;
    double rad, g;
    if (m.rational) {
        const double r6 = r4 * r2;
        const double num = ((1.0 + m.k1 * r2) + m.k2 * r4) + m.k3 * r6;
        const double den = ((1.0 + m.k4 * r2) + m.k5 * r4) + m.k6 * r6;
        rad = num / den - 1.0;
        const double dn = (m.k1 + (2.0 * m.k2) * r2) + (3.0 * m.k3) * r4;
        const double dd = (m.k4 + (2.0 * m.k5) * r2) + (3.0 * m.k6) * r4;
        g = (dn * den - num * dd) / (den * den);
    } else {
        rad = m.k1 * r2 + m.k2 * r4;
        g = m.k1 + (2.0 * m.k2) * r2;
    }
    const double du = (u * rad + (2.0 * m.p1) * uv) + m.p2 * (r2 + 2.0 * u2);
    const double dv = (v * rad + (2.0 * m.p2) * uv) + m.p1 * (r2 + 2.0 * v2);
    *pu = u + du;
    *pv = v + dv;
    *j00 = (((1.0 + rad) + (2.0 * u2) * g) + (2.0 * m.p1) * v) + (6.0 * m.p2) * u;
    *j01 = ((2.0 * uv) * g + (2.0 * m.p1) * u) + (2.0 * m.p2) * v;
    *j11 = (((1.0 + rad) + (2.0 * v2) * g) + (2.0 * m.p2) * u) + (6.0 * m.p1) * v;
}

UNDISTORT_HD void undistort_distort(const UndistortModel& m, double u, double v, double* pu, double* pv) {
    double j00, j01, j11;
    undistort_distort_jac(m, u, v, pu, pv, &j00, &j01, &j11);
}

// (u', v') = (tu, tv) -> (u, v).  true: converged; false: failed, (*u, *v) the last finite iterate.
UNDISTORT_HD bool undistort_undistort(const UndistortModel& m, double tu, double tv, double* ou, double* ov) {
    double u = tu, v = tv;
    *ou = u; *ov = v;
    if (m.identity) return true;
    for (int it = 0; it < UNDISTORT_MAX_ITER; it++) {
        double pu, pv, j00, j01, j11;
        undistort_distort_jac(m, u, v, &pu, &pv, &j00, &j01, &j11);
        const double fu = pu - tu, fv = pv - tv;
        const double det = j00 * j11 - j01 * j01;
        if (!undistort_finite(det) || det == 0.0) return false;
        const double su = (j11 * fu - j01 * fv) / det;
        const double sv = (j00 * fv - j01 * fu) / det;
        const double nu = u - su, nv = v - sv;
        if (!undistort_finite(nu) || !undistort_finite(nv)) return false;
        u = nu; v = nv;
        *ou = u; *ov = v;
        const double au = su < 0.0 ? -su : su, av = sv < 0.0 ? -sv : sv;
        if ((au > av ? au : av) <= UNDISTORT_EPS) return true;
    }
    return false;
}

// The source position of output pixel (x, y) of the undistorted PINHOLE camera {fx, fy, cx, cy} = q, in the distorted image's
// sample coordinates (pixel centres at integers): ((x + 0.5 - cx') / fx', ...) -> distort -> pixels -> - 0.5.  An identity
// model seen through its own intrinsics is a copy: the position is (x, y) exactly, whatever the division would round to.
UNDISTORT_HD void undistort_source_position(const UndistortModel& m, const double* q, int x, int y, double* sx, double* sy) {
    if (m.identity && q[0] == m.fx && q[1] == m.fy && q[2] == m.cx && q[3] == m.cy) {
        *sx = (double)x; *sy = (double)y;
        return;
    }
    const double u = (((double)x + 0.5) - q[2]) / q[0];
    const double v = (((double)y + 0.5) - q[3]) / q[1];
    double pu, pv;
    undistort_distort(m, u, v, &pu, &pv);
    *sx = (m.fx * pu + m.cx) - 0.5;
    *sy = (m.fy * pv + m.cy) - 0.5;
}

// A distorted observation (pixels) -> the undistorted PINHOLE camera q.  false: the iteration failed.
UNDISTORT_HD bool undistort_point(const UndistortModel& m, const double* q, double x, double y, double* ox, double* oy) {
    double u, v;
    const bool ok = undistort_undistort(m, (x - m.cx) / m.fx, (y - m.cy) / m.fy, &u, &v);
    *ox = q[0] * u + q[2];
    *oy = q[1] * v + q[3];
    return ok;
}

// ---- the undistorted camera (host; after COLMAP's UndistortCamera) ------------------------------------------------------------
//   1. fx, fy, cx, cy, w, h of the input.  A pinhole model: the output is the input.
//   2. Undistort the pixel centres of the four borders, (0.5, y + 0.5) and (w - 0.5, y + 0.5) for every row, (x + 0.5, 0.5) and
//      (x + 0.5, h - 0.5) for every column, and express them in the starting pinhole camera: px = fx*u + cx, py = fy*v + cy.
//      left_min_x .. bottom_max_y are their extrema; a sample whose iteration fails is left out, a side without any: error.
//   3. min_sx = min(cx / (cx - left_min_x), ((w - 0.5) - cx) / (right_max_x - cx))
//      max_sx = max(cx / (cx - left_max_x), ((w - 0.5) - cx) / (right_min_x - cx))
//      sx = 1 / (min_sx*blank + max_sx*(1 - blank)), clamped to [min_scale, max_scale] (a NaN goes to min_scale); sy likewise.
//   4. out_w = max(1, (int)(sx*w)), out_h likewise; cx' = (cx*out_w) / w, cy' = (cy*out_h) / h; the focal lengths stay.
// 0: ok; 1: bad argument, refused model or a side without a sample.  Nothing is written unless 0 is returned.
struct UndistortExtrema {
    double mn, mx;
    int any;
};
inline void undistort_extend(UndistortExtrema* e, double v) {
    if (!e->any) { e->mn = e->mx = v; e->any = 1; return; }
    if (v < e->mn) e->mn = v;
    if (v > e->mx) e->mx = v;
}
inline double undistort_scale(double c, double size, double lo_min, double lo_max, double hi_min, double hi_max, double blank, double min_scale,
                              double max_scale) {
    const double a0 = c / (c - lo_min), a1 = ((size - 0.5) - c) / (hi_max - c);
    const double b0 = c / (c - lo_max), b1 = ((size - 0.5) - c) / (hi_min - c);
    const double min_s = a0 < a1 ? a0 : a1;
    const double max_s = b0 > b1 ? b0 : b1;
    const double s = 1.0 / (min_s * blank + max_s * (1.0 - blank));
    return !(s >= min_scale) ? min_scale : (s > max_scale ? max_scale : s);
}
inline int undistort_camera_rule(int model, int w, int h, const double* params, double blank, double min_scale, double max_scale, int* out_w,
                                 int* out_h, double* pinhole4) {
    UndistortModel m;
    if (!params || !out_w || !out_h || !pinhole4 || w < 1 || h < 1 || !undistort_unpack(model, params, &m)) return 1;
    for (int k = 0; k < undistort_model_params(model); k++)
        if (!undistort_finite(params[k])) return 1;
    if (!(m.fx > 0.0) || !(m.fy > 0.0)) return 1;
    if (!(blank >= 0.0 && blank <= 1.0) || !(min_scale > 0.0) || !(max_scale >= min_scale) || !undistort_finite(max_scale)) return 1;
    if (!(max_scale * (double)(w > h ? w : h) <= 2147483647.0)) return 1;
    if (m.identity) {
        *out_w = w; *out_h = h;
        pinhole4[0] = m.fx; pinhole4[1] = m.fy; pinhole4[2] = m.cx; pinhole4[3] = m.cy;
        return 0;
    }
    UndistortExtrema left = {0, 0, 0}, right = {0, 0, 0}, top = {0, 0, 0}, bottom = {0, 0, 0};
    const double q[4] = {m.fx, m.fy, m.cx, m.cy};
    double px, py;
    for (int y = 0; y < h; y++) {
        if (undistort_point(m, q, 0.5, (double)y + 0.5, &px, &py)) undistort_extend(&left, px);
        if (undistort_point(m, q, (double)w - 0.5, (double)y + 0.5, &px, &py)) undistort_extend(&right, px);
    }
    for (int x = 0; x < w; x++) {
        if (undistort_point(m, q, (double)x + 0.5, 0.5, &px, &py)) undistort_extend(&top, py);
        if (undistort_point(m, q, (double)x + 0.5, (double)h - 0.5, &px, &py)) undistort_extend(&bottom, py);
    }
    if (!left.any || !right.any || !top.any || !bottom.any) return 1;
    const double sx = undistort_scale(m.cx, (double)w, left.mn, left.mx, right.mn, right.mx, blank, min_scale, max_scale);
    const double sy = undistort_scale(m.cy, (double)h, top.mn, top.mx, bottom.mn, bottom.mx, blank, min_scale, max_scale);
    const int ow = (int)(sx * (double)w), oh = (int)(sy * (double)h);
    *out_w = ow < 1 ? 1 : ow;
    *out_h = oh < 1 ? 1 : oh;
    pinhole4[0] = m.fx; pinhole4[1] = m.fy;
    pinhole4[2] = (m.cx * (double)*out_w) / (double)w;
    pinhole4[3] = (m.cy * (double)*out_h) / (double)h;
    return 0;
}
