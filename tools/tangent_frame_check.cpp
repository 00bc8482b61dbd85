// Host-only check of the tangent frame (gs-2m_amd/csrc/tangent_frame.h): for both halves of every class of atlas chart and for
// random triangles with degenerate and non-finite inputs mixed in, a valid frame is orthonormal with B = -cross(N, T), T along d_u
// and B against d_v; an invalid one has T = B = 0 and a finite unit N, encodes (0, 0, 1) and decodes to N; encode then decode of a
// normal of the upper hemisphere stays within the quantisation bound.  Plain C++, no GPU: build it with the host sanitizers and run it,
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/tangent_frame_check.cpp -o tangent_frame_check
// exit status 0 and "ok" when every case passes.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include "../gs-2m_amd/csrc/tangent_frame.h"

static int failures = 0;
static void expect(bool ok, const char* what, int k) {
    if (!ok && failures++ < 10) std::fprintf(stderr, "FAILED: %s in case %d\n", what, k);
}

static void check(const double* a, const double* b, const double* c, const double* uv, const double* N, const double* n, int k, bool must_be_valid) {
    TangentFrame F;
    tangent_frame(a, b, c, uv, N, &F);
    double m[3], back[3];
    tangent_encode(F, n, m);
    expect(tf_finite3(F.N) && fabs(tf_dot(F.N, F.N) - 1.0) <= 1e-14, "N is unit", k);
    expect(tf_finite3(m) && fabs(tf_dot(m, m) - 1.0) <= 1e-14 && m[2] >= 0.0, "m is unit with m_z >= 0", k);
    if (must_be_valid) expect(F.valid == 1, "valid", k);
    if (!F.valid) {
        expect(tf_dot(F.T, F.T) == 0.0 && tf_dot(F.B, F.B) == 0.0, "an invalid frame has no T, B", k);
        expect(m[0] == 0.0 && m[1] == 0.0 && m[2] == 1.0, "an invalid frame encodes flat", k);
        tangent_decode(F, n, back);
        expect(back[0] == F.N[0] && back[1] == F.N[1] && back[2] == F.N[2], "an invalid frame decodes to N", k);
        return;
    }
    double x[3];
    tf_cross(F.N, F.T, x);
    expect(fabs(tf_dot(F.T, F.N)) <= 1e-13 && fabs(tf_dot(F.B, F.N)) <= 1e-13 && fabs(tf_dot(F.T, F.B)) <= 1e-13, "orthogonal", k);
    expect(fabs(tf_dot(F.T, F.T) - 1.0) <= 1e-13 && fabs(tf_dot(F.B, F.B) - 1.0) <= 1e-13, "unit", k);
    expect(F.B[0] == -x[0] && F.B[1] == -x[1] && F.B[2] == -x[2], "B = -cross(N, T)", k);
    const double du1 = uv[2] - uv[0], dv1 = uv[3] - uv[1], du2 = uv[4] - uv[0], dv2 = uv[5] - uv[1], det = du1 * dv2 - du2 * dv1;
    double d_u[3], d_v[3];
    for (int d = 0; d < 3; d++) {
        d_u[d] = ((b[d] - a[d]) * dv2 - (c[d] - a[d]) * dv1) / det;
        d_v[d] = ((c[d] - a[d]) * du1 - (b[d] - a[d]) * du2) / det;
    }
    expect(tf_dot(F.T, d_u) > 0.0, "T along d_u", k);
    if (det > 0.0) expect(tf_dot(F.B, d_v) < 0.0, "B against d_v", k);
    // the round trip through the bytes, for a normal above the horizon of the frame
    double u[3];
    if (tf_unit(n, u) && tf_dot(u, F.N) > 0.02) {
        const double q[3] = {tangent_byte(m[0]) / 255.0 * 2.0 - 1.0, tangent_byte(m[1]) / 255.0 * 2.0 - 1.0, tangent_byte(m[2]) / 255.0 * 2.0 - 1.0};
        tangent_decode(F, q, back);
        const double bound = asin(sqrt(3.0) / 255.0 / (1.0 - sqrt(3.0) / 255.0));
        double cr[3];
        tf_cross(back, u, cr);
        expect(asin(fmin(sqrt(tf_dot(cr, cr)), 1.0)) <= bound && tf_dot(back, u) > 0.0, "round trip within the quantisation bound", k);
    }
}

int main() {
    std::mt19937_64 rng(5);
    std::normal_distribution<double> g(0.0, 1.0);
    std::uniform_real_distribution<double> r01(0.0, 1.0);
    int k = 0;
    for (int cls = 0; cls < 6; cls++)
        for (int half = 0; half < 2; half++, k++) {
            const int side = 8 << cls, L = side - 4;
            const int cx[3] = {half ? side - 1 : 1, half ? side - 1 - L : 1 + L, half ? side - 1 : 1};
            const int cy[3] = {half ? side - 1 : 1, half ? side - 1 : 1, half ? side - 1 - L : 1 + L};
            double P[9], uv[6], N[3], e1[3], e2[3];
            for (double& p : P) p = g(rng);
            for (int c = 0; c < 3; c++) uv[2 * c] = (double)(float)((24 + cx[c]) / 512.0), uv[2 * c + 1] = (double)(float)((8 + cy[c]) / 256.0);
            for (int d = 0; d < 3; d++) e1[d] = P[3 + d] - P[d], e2[d] = P[6 + d] - P[d];
            tf_cross(e1, e2, N);
            double n[3] = {N[0] + 0.3 * g(rng), N[1] + 0.3 * g(rng), N[2] + 0.3 * g(rng)};
            check(P, P + 3, P + 6, uv, N, n, k, true);
        }
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (int t = 0; t < 20000; t++, k++) {
        double P[9], uv[6], N[3], n[3];
        for (double& p : P) p = g(rng);
        for (double& x : uv) x = (double)(float)r01(rng);
        for (int d = 0; d < 3; d++) N[d] = g(rng), n[d] = g(rng);
        switch (t % 10) {  // one in two is damaged somewhere
            case 0: uv[4] = uv[2], uv[5] = uv[3]; break;                          // det == 0
            case 1: for (int d = 0; d < 3; d++) P[6 + d] = P[3 + d]; break;       // zero area
            case 2: P[t % 9] = nan; break;
            case 3: uv[t % 6] = inf; break;
            case 4: N[0] = N[1] = N[2] = 0.0; n[t % 3] = nan; break;
            default: break;
        }
        check(P, P + 3, P + 6, uv, N, n, k, false);
    }
    if (failures) return std::fprintf(stderr, "%d failures\n", failures), 1;
    std::puts("ok");
    return 0;
}
