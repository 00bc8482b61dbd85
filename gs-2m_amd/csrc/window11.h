// The 11-tap separable Gaussian window (sigma 1.5, zero "same" padding) of the SSIM operator and the walk that applies it,
// shared by ssim.hip (forward and backward, fp32) and image_metrics.hip (fp64): one copy of the weights, of the row walk, of
// the five-moment horizontal step and of the SSIM terms.
//
// The walk: a workgroup walks down a strip of rows.  Per input row it takes the oldest of PF prefetched rows, has the kernel
// stage it into one of two LDS row buffers, issues the fetch of the row PF ahead, has the kernel form its NQ horizontal sums
// out of LDS, and feeds them into a ring of 11 vertical accumulators per quantity that lives in registers (scatter form: input
// row t is tap k of output row t - k), so the vertical pass costs no LDS traffic and each input row is read once per strip
// (+10 halo rows).  The kernel's epilogue runs on the output row that completes; its ring slot is then reset.
#pragma once
#include "common.h"

// torch.Tensor([exp(-(x - 5)^2 / (2 * 1.5^2)) for x in range(11)]) / sum, in fp32 (utils/loss_utils.py:41-43)
__device__ __constant__ const float WINDOW11_W[11] = {0.001028380123898387f, 0.0075987582094967365f, 0.036000773310661316f,
                                                      0.10936068743467331f,  0.21300552785396576f,   0.26601171493530273f,
                                                      0.21300552785396576f,  0.10936068743467331f,   0.036000773310661316f,
                                                      0.0075987582094967365f, 0.001028380123898387f};

__device__ __forceinline__ float window11_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double window11_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// T: the type of the sums (the weights are widened to it exactly).  V, NV: a fetched row is NV values of type V per thread.
// NQ: ring quantities.  PF: rows in flight ahead of the row being consumed.  WIDTH: threads of the workgroup.
//   fetch(y, V (&v)[NV])            loads input row y of the thread's columns, zeros for y < 0 (outside the frame or the strip)
//   stage(buf, t, const V (&v)[NV]) writes the consumed row t into LDS row buffer `buf` (and may use its values otherwise)
//   hsum(buf, const T (&w)[11], T (&h)[NQ])  the thread's horizontal sums out of buffer `buf`
//   done(yo, const T (&m)[NQ])      the window sums of output row yo = y0 + t - 10 are complete
// rows: output rows of the strip, y0 .. y0 + rows - 1, from the input rows t = 0 .. rows + 9 (y0 - 5 .. y0 + rows + 4).  Every
// callable is called by the whole workgroup.
//
// THE BUFFER AND BARRIER RULE.  Row t is staged while other threads may still read row t - 1, hence two buffers, and read after
// a barrier.  STATIC_BUF picks the buffer as u & 1, u = t mod 11 the unrolled position, a compile-time constant that makes every
// LDS address an immediate -- but 11 is odd, so rows t = 10 and t = 11 (u = 10, u = 0) share buffer 0 and row 11 is staged with no
// barrier since the reads of row 10.  That is correct ONLY in a workgroup of one wave, whose LDS operations execute in order;
// there the barrier orders nothing across waves and a plain __syncthreads() will do.  A workgroup of more than one wave must use
// t & 1 (a wave writes a buffer again at row t + 2, behind the barrier of row t + 1, which every wave reaches only after its
// reads of row t) and gs2m_sync(), whose LDS wait hipcc cannot drop at the loop head (common.h).  A one-wave workgroup may ask
// for the multi-wave rule (image_metrics_kernel<1> does, being one template with <3>); the reverse does not compile.
template <typename T, typename V, int NQ, int NV, int PF, int WIDTH, bool STATIC_BUF = (WIDTH <= 64), class Fetch, class Stage,
          class Hsum, class Done>
__device__ __forceinline__ void window11_walk(int y0, int rows, Fetch fetch, Stage stage, Hsum hsum, Done done) {
    static_assert(!STATIC_BUF || WIDTH <= 64, "the u & 1 buffer index is safe in a one-wave workgroup only: see the rule above");
    const int nrows = rows + 10;
    T w[11];
#pragma unroll
    for (int k = 0; k < 11; k++) w[k] = (T)WINDOW11_W[k];
    T R[NQ][11];  // NQ quantities x 11 vertical accumulators
#pragma unroll
    for (int q = 0; q < NQ; q++)
#pragma unroll
        for (int j = 0; j < 11; j++) R[q][j] = (T)0;
    V pf[PF][NV];  // queue of fetched rows: pf[0] is the next one to consume
#pragma unroll
    for (int d = 0; d < PF; d++) fetch(d < nrows ? y0 - 5 + d : -1, pf[d]);
    for (int t0 = 0; t0 < nrows; t0 += 11) {
#pragma unroll
        for (int u = 0; u < 11; u++) {  // unrolled, so that every ring slot below is a register of its own
            const int t = t0 + u;
            if (t < nrows) {  // workgroup-uniform
                const int buf = STATIC_BUF ? (u & 1) : (t & 1);
                stage(buf, t, pf[0]);
#pragma unroll
                for (int d = 0; d + 1 < PF; d++)
#pragma unroll
                    for (int c = 0; c < NV; c++) pf[d][c] = pf[d + 1][c];
                fetch(t + PF < nrows ? y0 - 5 + t + PF : -1, pf[PF - 1]);
                if constexpr (STATIC_BUF) __syncthreads(); else gs2m_sync();
                T h[NQ];
                hsum(buf, w, h);
                // input row t is tap k of the output row t - k: ring slot (u - k) mod 11
#pragma unroll
                for (int k = 0; k < 11; k++) {
                    const int j = (u - k + 11) % 11;
#pragma unroll
                    for (int q = 0; q < NQ; q++) R[q][j] = window11_fma(w[k], h[q], R[q][j]);
                }
                const int jo = (u + 1) % 11;  // output row t - 10 is complete
                if (t >= 10) {
                    T m[NQ];
#pragma unroll
                    for (int q = 0; q < NQ; q++) m[q] = R[q][jo];
                    done(y0 + t - 10, m);
                }
#pragma unroll
                for (int q = 0; q < NQ; q++) R[q][jo] = (T)0;
            }
        }
    }
}

// The five horizontal moments (a, a^2, b, b^2, ab) of one element: its 11 taps lie STRIDE elements apart from sa[i] and sb[i] on.
// As written (-ffp-contract=off): plain adds for h[0] and h[2], FMAs for the rest.
template <int STRIDE, typename T, int N>
__device__ __forceinline__ void window11_moments(const T (&sa)[N], const T (&sb)[N], int i, const T (&w)[11], T (&h)[5]) {
#pragma unroll
    for (int q = 0; q < 5; q++) h[q] = (T)0;
#pragma unroll
    for (int k = 0; k < 11; k++) {
        const T a = sa[i + k * STRIDE], b = sb[i + k * STRIDE];
        const T wa = w[k] * a, wb = w[k] * b;
        h[0] += wa; h[1] = window11_fma(wa, a, h[1]);
        h[2] += wb; h[3] = window11_fma(wb, b, h[3]);
        h[4] = window11_fma(wa, b, h[4]);
    }
}

// SSIM = (Cc Dd) / (Aa Bb) from the five window moments E[a], E[a^2], E[b], E[b^2], E[ab]
template <typename T>
struct Window11Ssim {
    T Cc, Dd, Aa, Bb;
};
template <typename T>
__device__ __forceinline__ Window11Ssim<T> window11_ssim(T mu1, T e11, T mu2, T e22, T e12, T C1, T C2) {
    const T sigma1_sq = e11 - mu1 * mu1;
    const T sigma2_sq = e22 - mu2 * mu2;
    const T sigma12 = e12 - mu1 * mu2;
    Window11Ssim<T> s;
    s.Cc = (T)2 * (mu1 * mu2) + C1;
    s.Dd = (T)2 * sigma12 + C2;
    s.Aa = mu1 * mu1 + mu2 * mu2 + C1;
    s.Bb = sigma1_sq + sigma2_sq + C2;
    return s;
}
