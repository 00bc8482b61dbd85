// Host-only check of the undistortion arithmetic (gs-2m_amd/csrc/undistort_model.h): for every supported model with barrel and
// pincushion coefficients, distort(undistort(p)) returns p to 1e-12 on a grid, the camera rule accepts blank_pixels 0, 0.5 and 1
// and gives a size within the scale clamp, the border walk and the 1 x 1 and min_scale-clamped cases stay inside their buffers,
// refused models and bad arguments return 1 and write nothing, and a target far beyond the fold of a barrel model fails
// without a non-finite iterate.  Plain C++, no GPU: build it with the host sanitizers and run it,
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/undistort_model_check.cpp -o undistort_model_check
// exit status 0 and "ok" when every case passes.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>
#include "../gs-2m_amd/csrc/undistort_model.h"

struct Case {
    const char* name;
    int model;
    std::vector<double> params;
};

static int fail(const char* what, const Case& c) {
    std::fprintf(stderr, "FAILED: %s for %s\n", what, c.name);
    return 1;
}

static double absd(double x) { return x < 0 ? -x : x; }

static int check(const Case& c, int w, int h) {
    UndistortModel m;
    if (!undistort_unpack(c.model, c.params.data(), &m)) return fail("unpack", c);
    // the round trip on the normalised footprint of the image
    for (int j = 0; j <= 8; j++)
        for (int i = 0; i <= 8; i++) {
            const double tu = ((double)i / 8.0 * w - m.cx) / m.fx, tv = ((double)j / 8.0 * h - m.cy) / m.fy;
            double u, v, pu, pv;
            if (!undistort_undistort(m, tu, tv, &u, &v)) return fail("newton did not converge", c);
            undistort_distort(m, u, v, &pu, &pv);
            if (!(absd(pu - tu) <= 1e-12 && absd(pv - tv) <= 1e-12)) return fail("round trip", c);
        }
    const double blanks[3] = {0.0, 0.5, 1.0};
    for (double blank : blanks) {
        int ow = -7, oh = -7;
        double q[4] = {-7, -7, -7, -7};
        if (undistort_camera_rule(c.model, w, h, c.params.data(), blank, 0.2, 2.0, &ow, &oh, q) != 0) return fail("camera rule", c);
        if (ow < 1 || oh < 1 || ow > 2 * w || oh > 2 * h || (double)ow < 0.2 * w - 1 || (double)oh < 0.2 * h - 1) return fail("camera size", c);
        if (q[0] != m.fx || q[1] != m.fy || !undistort_finite(q[2]) || !undistort_finite(q[3])) return fail("camera parameters", c);
        // every output pixel has a finite source position or is reported outside by the comparisons
        for (int y = 0; y < oh; y++)
            for (int x = 0; x < ow; x++) {
                double sx, sy;
                undistort_source_position(m, q, x, y, &sx, &sy);
                const bool inside = sx >= 0.0 && sx <= (double)(w - 1) && sy >= 0.0 && sy <= (double)(h - 1);
                if (inside && ((int)sx < 0 || (int)sx > w - 1 || (int)sy < 0 || (int)sy > h - 1)) return fail("tap index", c);
            }
    }
    return 0;
}

int main() {
    const std::vector<Case> cases = {
        {"SIMPLE_PINHOLE", 0, {40.0, 18.2, 11.9}},
        {"PINHOLE", 1, {40.0, 42.0, 18.2, 11.9}},
        {"SIMPLE_RADIAL barrel", 2, {40.0, 18.2, 11.9, -0.08}},
        {"SIMPLE_RADIAL pincushion", 2, {40.0, 18.2, 11.9, 0.1}},
        {"RADIAL barrel", 3, {40.0, 18.2, 11.9, -0.1, 0.02}},
        {"RADIAL pincushion", 3, {40.0, 18.2, 11.9, 0.1, 0.02}},
        {"OPENCV barrel", 4, {40.0, 42.0, 18.2, 11.9, -0.1, 0.02, 0.003, -0.002}},
        {"OPENCV pincushion", 4, {40.0, 42.0, 18.2, 11.9, 0.12, 0.01, -0.002, 0.003}},
        {"FULL_OPENCV barrel", 6, {40.0, 42.0, 18.2, 11.9, -0.1, 0.02, 0.003, -0.002, 0.01, 0.05, 0.01, 0.002}},
        {"FULL_OPENCV pincushion", 6, {40.0, 42.0, 18.2, 11.9, 0.15, 0.02, -0.002, 0.003, 0.01, 0.02, 0.01, 0.002}},
        {"OPENCV zero", 4, {40.0, 42.0, 18.2, 11.9, 0.0, 0.0, 0.0, 0.0}},
    };
    int bad = 0;
    const int sizes[4][2] = {{1, 1}, {2, 2}, {3, 5}, {37, 23}};
    for (const Case& c : cases)
        for (const auto& s : sizes) {
            Case k = c;  // the principal point at the image centre for the small sizes
            const bool single = k.model == 0 || k.model == 2 || k.model == 3;
            if (s[0] != 37) {
                k.params[single ? 1 : 2] = 0.5 * s[0];
                k.params[single ? 2 : 3] = 0.5 * s[1];
            }
            bad += check(k, s[0], s[1]);
        }

    // refused models and bad arguments: 1, and nothing written
    const Case& o = cases[6];
    const int refused[5] = {5, 7, 8, 9, 10};
    int ow = -7, oh = -7;
    double q[4] = {-7, -7, -7, -7};
    std::vector<double> twelve(12, 0.1);
    for (int model : refused) bad += undistort_camera_rule(model, 37, 23, twelve.data(), 0.0, 0.2, 2.0, &ow, &oh, q) != 1;
    bad += undistort_camera_rule(-1, 37, 23, twelve.data(), 0.0, 0.2, 2.0, &ow, &oh, q) != 1;
    bad += undistort_camera_rule(11, 37, 23, twelve.data(), 0.0, 0.2, 2.0, &ow, &oh, q) != 1;
    bad += undistort_camera_rule(4, 0, 23, o.params.data(), 0.0, 0.2, 2.0, &ow, &oh, q) != 1;
    bad += undistort_camera_rule(4, 37, 0, o.params.data(), 0.0, 0.2, 2.0, &ow, &oh, q) != 1;
    bad += undistort_camera_rule(4, 37, 23, nullptr, 0.0, 0.2, 2.0, &ow, &oh, q) != 1;
    bad += undistort_camera_rule(4, 37, 23, o.params.data(), -0.1, 0.2, 2.0, &ow, &oh, q) != 1;
    bad += undistort_camera_rule(4, 37, 23, o.params.data(), 1.1, 0.2, 2.0, &ow, &oh, q) != 1;
    bad += undistort_camera_rule(4, 37, 23, o.params.data(), 0.0, 0.0, 2.0, &ow, &oh, q) != 1;
    bad += undistort_camera_rule(4, 37, 23, o.params.data(), 0.0, 0.5, 0.4, &ow, &oh, q) != 1;
    bad += undistort_camera_rule(4, 37, 23, o.params.data(), 0.0, 0.2, 1e300, &ow, &oh, q) != 1;
    bad += undistort_camera_rule(4, 37, 23, o.params.data(), 0.0, 0.2, 2.0, nullptr, &oh, q) != 1;
    {
        std::vector<double> p = o.params;
        p[0] = 0.0;
        bad += undistort_camera_rule(4, 37, 23, p.data(), 0.0, 0.2, 2.0, &ow, &oh, q) != 1;
        p = o.params;
        p[4] = std::numeric_limits<double>::quiet_NaN();
        bad += undistort_camera_rule(4, 37, 23, p.data(), 0.0, 0.2, 2.0, &ow, &oh, q) != 1;
    }
    if (ow != -7 || oh != -7 || q[0] != -7 || q[3] != -7) bad += fail("outputs touched by a refused call", o);

    // the min_scale clamp down to 1 x 1
    bad += undistort_camera_rule(4, 3, 5, cases[7].params.data(), 0.0, 0.2, 0.2, &ow, &oh, q) != 0 || ow != 1 || oh != 1;

    // far beyond the fold of a barrel model r (1 + k1 r^2) the iteration runs out of steps: it fails, its iterate stays finite
    {
        UndistortModel m;
        const double p[4] = {40.0, 18.2, 11.9, -0.08};
        undistort_unpack(2, p, &m);
        double u, v;
        if (undistort_undistort(m, (-400.0 - p[1]) / p[0], (-60.0 - p[2]) / p[0], &u, &v) || !undistort_finite(u) || !undistort_finite(v)) bad += fail("fold", cases[2]);
        const double nan = std::numeric_limits<double>::quiet_NaN();
        if (undistort_undistort(m, nan, 0.0, &u, &v)) bad += fail("NaN target", cases[2]);
    }
    if (bad) return 1;
    std::puts("ok");
    return 0;
}
