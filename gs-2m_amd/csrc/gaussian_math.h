// The per-Gaussian projection chain, written once for the forward (preprocess.hip) and its backward (gaussian_bwd.hip): view-space
// point and near plane, 3D covariance (computeCov3D, forward.cu:109-142), 2D covariance (computeCov2D, forward.cu:70-104), the SH
// constants.  The backward's gradients are those of THESE expressions in THIS order (-ffp-contract=off: written order is evaluation
// order), which is why neither file carries a copy.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

struct M3 {  // column-major 3x3, m[col][row]
    float m[3][3];
};
__device__ __forceinline__ M3 m3_cols(float a, float b, float c, float d, float e, float f, float g, float h, float i) {
    M3 r;
    r.m[0][0] = a; r.m[0][1] = b; r.m[0][2] = c;
    r.m[1][0] = d; r.m[1][1] = e; r.m[1][2] = f;
    r.m[2][0] = g; r.m[2][1] = h; r.m[2][2] = i;
    return r;
}
__device__ __forceinline__ M3 m3_mul(const M3& A, const M3& B) {
    M3 R;
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int r = 0; r < 3; r++)
            R.m[c][r] = A.m[0][r] * B.m[c][0] + A.m[1][r] * B.m[c][1] + A.m[2][r] * B.m[c][2];
    return R;
}
__device__ __forceinline__ M3 m3_t(const M3& A) {
    M3 R;
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int r = 0; r < 3; r++) R.m[c][r] = A.m[r][c];
    return R;
}

// real SH basis constants: degree 0, degree 1, and the tables of degrees 2 and 3 (forward.cu / backward.cu: SH_C2, SH_C3)
#define SH_C0 0.28209479177387814f
#define SH_C1 0.4886025119029199f
static __constant__ float kSH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                                       -1.0925484305920792f, 0.5462742152960396f};
static __constant__ float kSH_C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f,
                                       -0.4570457994644658f, 1.445305721320277f, -0.5900435899266435f};

// view-space point (transformPoint4x3) and the near plane: a Gaussian is processed when its view depth is ABOVE kNearZ (in_frustum)
constexpr float kNearZ = 0.2f;
__device__ __forceinline__ float gs2m_view_z(const float* __restrict__ vm, float px, float py, float pz) {
    return vm[2] * px + vm[6] * py + vm[10] * pz + vm[14];
}
__device__ __forceinline__ float3 gs2m_view_point(const float* __restrict__ vm, float px, float py, float pz) {
    return make_float3(vm[0] * px + vm[4] * py + vm[8] * pz + vm[12], vm[1] * px + vm[5] * py + vm[9] * pz + vm[13],
                       gs2m_view_z(vm, px, py, pz));
}

// 3D covariance Sigma = M^t M, M = S R, of the (already scale-modified) scales and the quaternion q = (r, x, y, z), not normalised
// (nor does the reference): c3 = its upper triangle, row by row.  R and M: for the backward's scale / rotation step.
__device__ __forceinline__ void gs2m_cov3d(float sx, float sy, float sz, float4 q, float c3[6], M3& R, M3& Mm) {
    const float r = q.x, x = q.y, y = q.z, z = q.w;
    M3 S = m3_cols(sx, 0.f, 0.f, 0.f, sy, 0.f, 0.f, 0.f, sz);
    R = m3_cols(1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y),
                2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x),
                2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y));
    Mm = m3_mul(S, R);
    M3 Sig = m3_mul(m3_t(Mm), Mm);
    c3[0] = Sig.m[0][0]; c3[1] = Sig.m[0][1]; c3[2] = Sig.m[0][2]; c3[3] = Sig.m[1][1]; c3[4] = Sig.m[1][2]; c3[5] = Sig.m[2][2];
}

// EWA projection of the 3D covariance c3 at the view-space point v: cov = T^t Vrk^t T with T = W J, of which m[0][0], m[0][1]
// and m[1][1] are the 2D covariance (no low-pass here: the forward has none, the backward adds its own).  The point's ratios
// x/z, y/z are clamped to 1.3 tan(fov / 2) inside J; the backward masks its gradients with the unclamped ones and asks for the
// clamped point as well (want_xy: handed out only on request -- the compiler emits other code for the forward when the values
// leave this function, even unread).
struct Cov2D {
    M3 cov, T, Vrk, W;
    float limx, limy, txtz, tytz;  // the clamp, 1.3 * tan_fov, and x/z, y/z as they are
    float tx, ty;      // x, y of the clamped point, with want_xy only
};
__device__ __forceinline__ void gs2m_cov2d(float3 v, const float c3[6], const float* __restrict__ vm, float focal_x, float focal_y,
                                           float tan_fovx, float tan_fovy, Cov2D& o, bool want_xy = false) {
    const float vx = v.x, vy = v.y, vz = v.z;
    const float limx = 1.3f * tan_fovx, limy = 1.3f * tan_fovy;
    const float txtz = vx / vz, tytz = vy / vz;
    const float tx = fminf(limx, fmaxf(-limx, txtz)) * vz;
    const float ty = fminf(limy, fmaxf(-limy, tytz)) * vz;
    M3 J = m3_cols(focal_x / vz, 0.0f, -(focal_x * tx) / (vz * vz), 0.0f, focal_y / vz, -(focal_y * ty) / (vz * vz), 0.f, 0.f, 0.f);
    o.W = m3_cols(vm[0], vm[4], vm[8], vm[1], vm[5], vm[9], vm[2], vm[6], vm[10]);
    o.T = m3_mul(o.W, J);
    o.Vrk = m3_cols(c3[0], c3[1], c3[2], c3[1], c3[3], c3[4], c3[2], c3[4], c3[5]);
    o.cov = m3_mul(m3_mul(m3_t(o.T), m3_t(o.Vrk)), o.T);
    o.limx = limx; o.limy = limy; o.txtz = txtz; o.tytz = tytz;
    if (want_xy) { o.tx = tx; o.ty = ty; }
}
