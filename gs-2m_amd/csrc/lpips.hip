// LPIPS (VGG16, v0.1) of 8-bit image pairs for gfx950 (metrics.py:57's third score; include/gs2m_lpips.h).
//
// The work is thirteen 3x3 convolutions at image resolution, done as an IMPLICIT GEMM on the fp32-input matrix instruction
// v_mfma_f32_32x32x2_f32: M = the pixels of a 16x16 spatial tile, N = 64 output channels, K = (Cin chunk of 16, tap, channel).
// Activations are channels-innermost (N, H, W, C), so a chunk of 16 input channels of the 18x18 tile-with-halo is staged in LDS
// ONCE and the nine taps are nine shifted reads of it; the chunk's 9 x 16 x 64 weights are staged beside it.  A workgroup of four
// waves: wave w owns rows 4w .. 4w + 3 of the tile (two 32-pixel M fragments: two rows of 16 each) x 64 channels (two N
// fragments), i.e. four 32x32 accumulators, 64 registers.  Per k-step of 2 channels it reads two A and two B values from LDS
// and issues four MFMAs.  The instruction's result is a k-ordered fp32 fmaf chain, so an output element is one chain of 9 Cin
// products that starts from the bias -- the precision class of the reference's fp32 run.
//
// LDS images (59.4 KB, two workgroups per CU):
//   s_in[channel][pixel of the 18x18 tile], plane stride 352: the 32 lanes of a fragment half read two runs of 16 consecutive
//     words 18 apart, the other half the next plane, 32 banks on: conflict-free but for two words.
//   s_w[tap][channel][64 cout], the odd channel rows rotated by 32 columns: the two halves of a B read hit disjoint banks.
// Borders are zero-filled by predicated loads: an address is formed only for a pixel inside the image.
//
// Cin = 3 (K = 27, 0.6 % of the work) runs on the vector unit, a thread per pixel, the 27 x 64 weights broadcast from LDS.
// The prologue (u8 -> value / 255 -> z-score), the 2x2 max-pool and the tap distance are kernels of their own; the tap
// distance adds pixels in fp64 per workgroup in a fixed order, a last kernel adds the workgroups' partials in index order.
#include "common.h"
#include "../../include/gs2m_lpips.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TILE = GS2M_LPIPS_TILE;  // 16 x 16 output pixels per workgroup
constexpr int HT = TILE + 2;           // with the 1-pixel halo
constexpr int PLANE = 352;             // words per channel plane of s_in: 18 * 18 = 324, padded to 32 mod 64
constexpr int KC = 16;                 // input channels per LDS stage
constexpr int NB = 64;                 // output channels per workgroup

const int CONV_CIN[GS2M_LPIPS_CONVS] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
const int CONV_COUT[GS2M_LPIPS_CONVS] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
const int TAP_AFTER[GS2M_LPIPS_TAPS] = {1, 3, 6, 9, 12};  // the convolution whose ReLU output is tap t; a pool follows all but the last
const int TAP_C[GS2M_LPIPS_TAPS] = {64, 128, 256, 512, 512};

// ---- packing ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) pack_conv_kernel(int cin, int cout, const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ packed) {
    const int nw = 9 * cin * cout;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < nw) {
        const int co = i % cout, r = i / cout, ci = r % cin, tap = r / cin;
        packed[i] = w[((size_t)co * cin + ci) * 9 + tap];
    } else if (i < nw + cout) {
        packed[i] = bias[i - nw];
    }
}

__global__ void __launch_bounds__(256) copy_kernel(int n, const float* __restrict__ src, float* __restrict__ dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// ---- prologue: (N = 2, H, W, 3) u8 of the pair -> fp32 z-scores (networks.py:50-51 on metrics.py:33's value / 255) ------------
__global__ void __launch_bounds__(256) prologue_kernel(size_t per_image, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                       float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * per_image) return;
    const bool second = i >= per_image;
    const size_t e = second ? i - per_image : i;
    const int c = (int)(e % 3);
    const float mean = c == 0 ? -.030f : c == 1 ? -.088f : -.188f;
    const float sd = c == 0 ? .458f : c == 1 ? .448f : .450f;
    const float v = __fdiv_rn((float)(second ? b[e] : a[e]), 255.0f);
    out[i] = __fdiv_rn(v - mean, sd);
}

// ---- conv3x3 + bias + ReLU, Cin a multiple of 16, Cout a multiple of 64: implicit GEMM on the fp32 MFMA ----------------------
__global__ void __launch_bounds__(256) conv3x3_mfma_kernel(int H, int W, int Cin, int Cout, int tiles_x, int tiles_y,
                                                           const float* __restrict__ in, const float* __restrict__ wpk,
                                                           float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float s_in[KC * PLANE];
    __shared__ __attribute__((aligned(16))) float s_w[9 * KC * NB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned blk = blockIdx.x;
    const int tx = (int)(blk % (unsigned)tiles_x);
    const unsigned rest = blk / (unsigned)tiles_x;
    const int ty = (int)(rest % (unsigned)tiles_y), img = (int)(rest / (unsigned)tiles_y);
    const int x0 = tx * TILE, y0 = ty * TILE, n0 = (int)blockIdx.y * NB;
    const size_t img_base = (size_t)img * (size_t)H * (size_t)W;
    const float* __restrict__ bias = wpk + (size_t)9 * Cin * Cout;
    const int h = lane >> 5, j = lane & 31;  // k within the MFMA's pair; row of A / column of B within the fragment

    f32x16 acc[2][2];
#pragma unroll
    for (int nt = 0; nt < 2; nt++) {
        const float bv = bias[n0 + nt * 32 + j];  // the chain starts from the bias
#pragma unroll
        for (int mt = 0; mt < 2; mt++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[mt][nt][r] = bv;
    }

    const int a_off = h * PLANE + (wave * 4 + (j >> 4)) * HT + (j & 15);
    const int b_off0 = h * NB + ((j + 32 * h) & 63), b_off1 = h * NB + ((j + 32 + 32 * h) & 63);

    for (int c0 = 0; c0 < Cin; c0 += KC) {
        // the 18 x 18 pixels x 16 channels of the tile and its halo: a float4 (4 channels of one pixel) per item
        for (int item = tid; item < HT * HT * 4; item += 256) {
            const int pix = item >> 2, q = item & 3;
            const int py = pix / HT, px = pix - py * HT;
            const int y = y0 - 1 + py, x = x0 - 1 + px;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (y >= 0 && y < H && x >= 0 && x < W)
                v = *reinterpret_cast<const float4*>(in + (img_base + (size_t)y * W + x) * (size_t)Cin + c0 + q * 4);
            float* d = s_in + (q * 4) * PLANE + pix;
            d[0] = v.x; d[PLANE] = v.y; d[2 * PLANE] = v.z; d[3 * PLANE] = v.w;
        }
        // the chunk's weights: 9 taps x 16 channels x 64 cout, a float4 per thread and tap
        {
            const int k = tid >> 4, j4 = tid & 15;
#pragma unroll
            for (int tap = 0; tap < 9; tap++) {
                const float4 v = *reinterpret_cast<const float4*>(wpk + ((size_t)tap * Cin + c0 + k) * (size_t)Cout + n0 + j4 * 4);
                *reinterpret_cast<float4*>(s_w + (tap * KC + k) * NB + ((j4 * 4 + 32 * (k & 1)) & 63)) = v;
            }
        }
        gs2m_sync();
#pragma unroll
        for (int tap = 0; tap < 9; tap++) {
            const int dy = tap / 3, dx = tap % 3;
#pragma unroll
            for (int kk = 0; kk < KC / 2; kk++) {
                const float a0 = s_in[a_off + 2 * kk * PLANE + dy * HT + dx];
                const float a1 = s_in[a_off + 2 * kk * PLANE + (dy + 2) * HT + dx];
                const float b0 = s_w[(tap * KC + 2 * kk) * NB + b_off0];
                const float b1 = s_w[(tap * KC + 2 * kk) * NB + b_off1];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
        gs2m_sync();  // every wave has read this stage before the next one is written
    }

    // C/D map of the 32x32 forms: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int mt = 0; mt < 2; mt++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int i = (r & 3) + 8 * (r >> 2) + 4 * h;  // pixel of the fragment: row i >> 4, column i & 15
            const int y = y0 + wave * 4 + mt * 2 + (i >> 4), x = x0 + (i & 15);
            if (y < H && x < W) {
                float* o = out + (img_base + (size_t)y * W + x) * (size_t)Cout + n0 + j;
                o[0] = fmaxf(acc[mt][0][r], 0.f);
                o[32] = fmaxf(acc[mt][1][r], 0.f);
            }
        }
}

// ---- conv3x3 + bias + ReLU, Cin = 3: a thread per pixel on the vector unit, the chain in (tap, channel) order ----------------
__global__ void __launch_bounds__(256) conv3x3_c3_kernel(int H, int W, int Cout, size_t pixels, const float* __restrict__ in,
                                                         const float* __restrict__ wpk, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float s_w[28 * NB];  // 27 rows of weights, then the bias
    const int tid = threadIdx.x, n0 = (int)blockIdx.y * NB;
    for (int i = tid; i < 28 * NB; i += 256) s_w[i] = wpk[(size_t)(i >> 6) * Cout + n0 + (i & 63)];  // row 27 of [28][Cout] is the bias
    gs2m_sync();
    const size_t p = (size_t)blockIdx.x * 256 + tid;
    if (p >= pixels) return;
    const size_t hw = (size_t)H * W;
    const size_t img = p / hw;
    const int r = (int)(p - img * hw), y = r / W, x = r - y * W;
    float v[27];
#pragma unroll
    for (int tap = 0; tap < 9; tap++) {
        const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
        const bool inside = yy >= 0 && yy < H && xx >= 0 && xx < W;
#pragma unroll
        for (int c = 0; c < 3; c++) v[tap * 3 + c] = inside ? in[(img * hw + (size_t)yy * W + xx) * 3 + c] : 0.f;
    }
    float* o = out + p * (size_t)Cout + n0;
#pragma unroll 4
    for (int j4 = 0; j4 < NB / 4; j4++) {
        float4 a = *reinterpret_cast<const float4*>(s_w + 27 * NB + j4 * 4);
#pragma unroll
        for (int k = 0; k < 27; k++) {
            const float4 w = *reinterpret_cast<const float4*>(s_w + k * NB + j4 * 4);
            a.x = __builtin_fmaf(v[k], w.x, a.x); a.y = __builtin_fmaf(v[k], w.y, a.y);
            a.z = __builtin_fmaf(v[k], w.z, a.z); a.w = __builtin_fmaf(v[k], w.w, a.w);
        }
        *reinterpret_cast<float4*>(o + j4 * 4) = make_float4(fmaxf(a.x, 0.f), fmaxf(a.y, 0.f), fmaxf(a.z, 0.f), fmaxf(a.w, 0.f));
    }
}

// ---- 2x2 / stride 2 max-pool, floor sizing: a thread per output pixel and channel quad -----------------------------------------
__global__ void __launch_bounds__(256) maxpool2x2_kernel(int H, int W, int C4, int Ho, int Wo, size_t total,
                                                         const float4* __restrict__ in, float4* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % (size_t)C4);
    size_t r = i / (size_t)C4;
    const int xo = (int)(r % (size_t)Wo);
    r /= (size_t)Wo;
    const int yo = (int)(r % (size_t)Ho);
    const size_t img = r / (size_t)Ho;
    const size_t row0 = ((img * H + 2 * (size_t)yo) * W + 2 * (size_t)xo) * C4 + c, row1 = row0 + (size_t)W * C4;
    const float4 a = in[row0], b = in[row0 + C4], d = in[row1], e = in[row1 + C4];
    out[i] = make_float4(fmaxf(fmaxf(a.x, b.x), fmaxf(d.x, e.x)), fmaxf(fmaxf(a.y, b.y), fmaxf(d.y, e.y)),
                         fmaxf(fmaxf(a.z, b.z), fmaxf(d.z, e.z)), fmaxf(fmaxf(a.w, b.w), fmaxf(d.w, e.w)));
}

// ---- tap distance: a wave per pixel, lane l holds channels l, l + 64, ...; 256 pixels per workgroup -----------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

template <int CJ>
__global__ void __launch_bounds__(256) tap_distance_kernel(int HW, int parts, const float* __restrict__ fx, const float* __restrict__ fy,
                                                           const float* __restrict__ lin, double* __restrict__ part) {
    constexpr int C = 64 * CJ;
    __shared__ double s_part[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned blk = blockIdx.x;
    const size_t img = blk / (unsigned)parts;
    const int first = (int)(blk % (unsigned)parts) * 256 + wave * 64;
    float l[CJ];
#pragma unroll
    for (int k = 0; k < CJ; k++) l[k] = lin[lane + 64 * k];
    double acc = 0.0;
    const int last = min(first + 64, HW);
    for (int p = first; p < last; p++) {  // wave-uniform
        const size_t o = (img * (size_t)HW + (size_t)p) * C + lane;
        float a[CJ], b[CJ];
#pragma unroll
        for (int k = 0; k < CJ; k++) { a[k] = fx[o + 64 * k]; b[k] = fy[o + 64 * k]; }
        float sa = 0.f, sb = 0.f;
#pragma unroll
        for (int k = 0; k < CJ; k++) { sa = __builtin_fmaf(a[k], a[k], sa); sb = __builtin_fmaf(b[k], b[k], sb); }
        const float na = __fsqrt_rn(wave_sum(sa)) + 1e-10f, nb = __fsqrt_rn(wave_sum(sb)) + 1e-10f;  // utils.py:6-8
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < CJ; k++) {
            const float d = __fdiv_rn(a[k], na) - __fdiv_rn(b[k], nb);
            v = __builtin_fmaf(l[k], d * d, v);
        }
        acc += (double)wave_sum(v);  // every lane holds the same sum
    }
    if (lane == 0) s_part[wave] = acc;
    gs2m_sync();
    if (tid == 0) part[blk] = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
}

// one thread per image: its partials in index order, then the spatial mean
__global__ void __launch_bounds__(64) tap_mean_kernel(int N, int parts, int HW, const double* __restrict__ part, double* __restrict__ out,
                                                      int out_stride) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    double s = 0.0;
    for (int p = 0; p < parts; p++) s += part[(size_t)n * parts + p];
    out[(size_t)n * out_stride] = s / (double)HW;
}

__global__ void lpips_total_kernel(const double* __restrict__ layers, double* __restrict__ total) {
    if (threadIdx.x == 0) *total = (((layers[0] + layers[1]) + layers[2]) + layers[3]) + layers[4];
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

bool channels_ok(int cin, int cout) { return (cin == 3 || (cin >= KC && cin % KC == 0)) && cin <= 512 && cout >= NB && cout % NB == 0 && cout <= 512; }

// N images of (H, W): N H W <= 2^26 keeps every grid below 2^31 blocks and every element index far below 2^63
bool plane_ok(int N, int H, int W) {
    return N >= 1 && H >= 1 && W >= 1 && (long long)N * H * W <= (1ll << 26);
}

void launch_conv(int N, int H, int W, int cin, int cout, const float* in, const float* packed, float* out, hipStream_t s) {
    if (cin == 3) {
        const size_t pixels = (size_t)N * H * W;
        conv3x3_c3_kernel<<<dim3((unsigned)((pixels + 255) / 256), cout / NB), 256, 0, s>>>(H, W, cout, pixels, in, packed, out);
    } else {
        const int tiles_x = (W + TILE - 1) / TILE, tiles_y = (H + TILE - 1) / TILE;
        conv3x3_mfma_kernel<<<dim3((unsigned)tiles_x * tiles_y * N, cout / NB), 256, 0, s>>>(H, W, cin, cout, tiles_x, tiles_y, in, packed, out);
    }
}

void launch_pool(int N, int H, int W, int C, const float* in, float* out, hipStream_t s) {
    const int Ho = H / 2, Wo = W / 2, C4 = C / 4;
    const size_t total = (size_t)N * Ho * Wo * C4;
    maxpool2x2_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(H, W, C4, Ho, Wo, total, reinterpret_cast<const float4*>(in),
                                                                      reinterpret_cast<float4*>(out));
}

int tap_parts(int H, int W) { return (H * W + 255) / 256; }

void launch_tap(int N, int H, int W, int C, const float* fx, const float* fy, const float* lin, double* part, double* out, int out_stride,
                hipStream_t s) {
    const int HW = H * W, parts = tap_parts(H, W);
    const unsigned grid = (unsigned)parts * N;
    switch (C) {
    case 64: tap_distance_kernel<1><<<grid, 256, 0, s>>>(HW, parts, fx, fy, lin, part); break;
    case 128: tap_distance_kernel<2><<<grid, 256, 0, s>>>(HW, parts, fx, fy, lin, part); break;
    case 256: tap_distance_kernel<4><<<grid, 256, 0, s>>>(HW, parts, fx, fy, lin, part); break;
    default: tap_distance_kernel<8><<<grid, 256, 0, s>>>(HW, parts, fx, fy, lin, part); break;
    }
    tap_mean_kernel<<<(N + 63) / 64, 64, 0, s>>>(N, parts, HW, part, out, out_stride);
}

size_t conv_packed_floats(int l) { return (size_t)9 * CONV_CIN[l] * CONV_COUT[l] + CONV_COUT[l]; }

bool lpips_plan(int N, int H, int W, size_t* buf_floats, size_t* part_doubles) {
    if (N < 1 || H < GS2M_LPIPS_MIN_SIZE || W < GS2M_LPIPS_MIN_SIZE || H > 32768 || W > 32768 || (long long)H * W > (1ll << 26) / 2)
        return false;  // (the pair is a batch of two: 2 H W <= 2^26)
    *buf_floats = (size_t)2 * H * W * 64;  // the largest layer: 64 channels at full size, both images
    *part_doubles = (size_t)tap_parts(H, W);
    return true;
}

}  // namespace

extern "C" int gs2m_lpips_pack_conv(int cin, int cout, const float* w_oihw, const float* bias, float* packed, void* stream) {
    if (!w_oihw || !bias || !packed || !aligned16(packed)) return GS2M_ERR_INVALID_ARG;
    if (!channels_ok(cin, cout)) return GS2M_ERR_UNSUPPORTED;
    const int n = 9 * cin * cout + cout;
    pack_conv_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(cin, cout, w_oihw, bias, packed);
    return gs2m_status(hipGetLastError());
}

extern "C" int gs2m_lpips_pack_weights(const void* const* conv_w, const void* const* conv_b, const void* const* lin, float* packed,
                                       void* stream) {
    if (!conv_w || !conv_b || !lin || !packed || !aligned16(packed)) return GS2M_ERR_INVALID_ARG;
    for (int l = 0; l < GS2M_LPIPS_CONVS; l++)
        if (!conv_w[l] || !conv_b[l]) return GS2M_ERR_INVALID_ARG;
    for (int t = 0; t < GS2M_LPIPS_TAPS; t++)
        if (!lin[t]) return GS2M_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    size_t off = 0;
    for (int l = 0; l < GS2M_LPIPS_CONVS; l++) {
        const int n = (int)conv_packed_floats(l);
        pack_conv_kernel<<<(n + 255) / 256, 256, 0, s>>>(CONV_CIN[l], CONV_COUT[l], (const float*)conv_w[l], (const float*)conv_b[l],
                                                         packed + off);
        off += (size_t)n;
    }
    for (int t = 0; t < GS2M_LPIPS_TAPS; t++) {
        copy_kernel<<<(TAP_C[t] + 255) / 256, 256, 0, s>>>(TAP_C[t], (const float*)lin[t], packed + off);
        off += (size_t)TAP_C[t];
    }
    return off == (size_t)GS2M_LPIPS_PACKED_FLOATS ? gs2m_status(hipGetLastError()) : GS2M_ERR_INVALID_ARG;
}

extern "C" int gs2m_lpips_workspace_bytes(int N, int H, int W, long long* bytes) {
    size_t buf, parts;
    if (!bytes || !lpips_plan(N, H, W, &buf, &parts)) return GS2M_ERR_INVALID_ARG;
    *bytes = (long long)(2 * buf * sizeof(float) + gs2m_align_up(parts * sizeof(double)));
    return GS2M_OK;
}

extern "C" int gs2m_lpips(int N, int H, int W, const unsigned char* a, const unsigned char* b, const float* packed, void* ws,
                          long long ws_bytes, double* out_total, double* out_layers, void* stream) {
    size_t buf, parts;
    if (!a || !b || !packed || !ws || !out_total || !out_layers || !lpips_plan(N, H, W, &buf, &parts)) return GS2M_ERR_INVALID_ARG;
    if (!aligned16(ws) || !aligned16(packed) || ws_bytes < (long long)(2 * buf * sizeof(float) + gs2m_align_up(parts * sizeof(double))))
        return GS2M_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    float* bufs[2] = {reinterpret_cast<float*>(ws), reinterpret_cast<float*>(ws) + buf};
    double* part = reinterpret_cast<double*>(bufs[1] + buf);
    size_t conv_off[GS2M_LPIPS_CONVS], off = 0;
    for (int l = 0; l < GS2M_LPIPS_CONVS; l++) { conv_off[l] = off; off += conv_packed_floats(l); }
    const float* lin = packed + off;
    const size_t per_image = (size_t)H * W * 3;
    for (int n = 0; n < N; n++) {
        int cur = 1;  // the z-scores go to buffer 1; every kernel reads bufs[cur] and writes bufs[cur ^ 1]
        prologue_kernel<<<(unsigned)((2 * per_image + 255) / 256), 256, 0, s>>>(per_image, a + n * per_image, b + n * per_image, bufs[cur]);
        int h = H, w = W, tap = 0;
        size_t lin_off = 0;
        for (int l = 0; l < GS2M_LPIPS_CONVS; l++) {
            launch_conv(2, h, w, CONV_CIN[l], CONV_COUT[l], bufs[cur], packed + conv_off[l], bufs[cur ^ 1], s);
            cur ^= 1;
            if (l == TAP_AFTER[tap]) {
                const int C = TAP_C[tap];
                launch_tap(1, h, w, C, bufs[cur], bufs[cur] + (size_t)h * w * C, lin + lin_off, part, out_layers + (size_t)n * 5 + tap, 1, s);
                lin_off += (size_t)C;
                if (++tap == GS2M_LPIPS_TAPS) break;  // the fifth pool is never run
                launch_pool(2, h, w, C, bufs[cur], bufs[cur ^ 1], s);
                cur ^= 1;
                h /= 2; w /= 2;
            }
        }
        lpips_total_kernel<<<1, 64, 0, s>>>(out_layers + (size_t)n * 5, out_total + n);
    }
    return gs2m_status(hipGetLastError());
}

extern "C" int gs2m_lpips_conv3x3(int N, int H, int W, int cin, int cout, const float* in, const float* packed, float* out, void* stream) {
    if (!in || !packed || !out || !plane_ok(N, H, W) || !aligned16(packed) || !aligned16(out) || ((uintptr_t)in & (cin == 3 ? 3u : 15u)) != 0)
        return GS2M_ERR_INVALID_ARG;
    if (!channels_ok(cin, cout)) return GS2M_ERR_UNSUPPORTED;
    launch_conv(N, H, W, cin, cout, in, packed, out, (hipStream_t)stream);
    return gs2m_status(hipGetLastError());
}

extern "C" int gs2m_lpips_maxpool2x2(int N, int H, int W, int C, const float* in, float* out, void* stream) {
    if (!in || !out || !plane_ok(N, H, W) || H < 2 || W < 2 || C < 4 || C % 4 != 0 || C > 512 || !aligned16(in) || !aligned16(out))
        return GS2M_ERR_INVALID_ARG;
    launch_pool(N, H, W, C, in, out, (hipStream_t)stream);
    return gs2m_status(hipGetLastError());
}

extern "C" int gs2m_lpips_tap_workspace_bytes(int N, int H, int W, long long* bytes) {
    if (!bytes || !plane_ok(N, H, W)) return GS2M_ERR_INVALID_ARG;
    *bytes = (long long)sizeof(double) * N * tap_parts(H, W);
    return GS2M_OK;
}

extern "C" int gs2m_lpips_tap_distance(int N, int H, int W, int C, const float* fx, const float* fy, const float* lin, void* ws,
                                       long long ws_bytes, double* out, void* stream) {
    if (!fx || !fy || !lin || !ws || !out || !plane_ok(N, H, W) || ((uintptr_t)ws & 7u) != 0) return GS2M_ERR_INVALID_ARG;
    if (C != 64 && C != 128 && C != 256 && C != 512) return GS2M_ERR_UNSUPPORTED;
    if (ws_bytes < (long long)sizeof(double) * N * tap_parts(H, W)) return GS2M_ERR_INVALID_ARG;
    launch_tap(N, H, W, C, fx, fy, lin, reinterpret_cast<double*>(ws), out, 1, (hipStream_t)stream);
    return gs2m_status(hipGetLastError());
}
