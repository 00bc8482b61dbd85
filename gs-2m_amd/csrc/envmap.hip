// Environment maps for gfx950: Radiance RGBE pixels <-> float32 images, and a lat-long image -> the cube map a CubemapLight holds
// (include/gs2m_envmap.h).  Four entry points:
//   gs2m_hdr_scan            HOST: one walk over the scanlines -> per row its kind and the offsets of its four channel planes
//   gs2m_hdr_decode          a workgroup per row: the planes expanded through LDS, RGBE -> fp32 by integer arithmetic (exact)
//   gs2m_hdr_encode          a thread per pixel: fp32 -> RGBE, flat scanlines
//   gs2m_latlong_to_cubemap  a thread per texel: S x S solid-angle-weighted bilinear taps
//
// Why the scan is host work: where a row starts is known only when the row before it has been parsed, code byte by code byte; a
// 4096 x 2048 file is 2048 such chains of ~16 K bytes each, a few milliseconds of one core over bytes that are in the host's memory
// anyway.  What then crosses to the device is the file's 4 bytes per pixel (less, when it is run-length coded), not the 12 of the
// float image, and within a row the four planes and, across rows, the H rows are independent: that is the device's part.
//
// The decoder: wave c of a row's workgroup walks plane c.  A code is one wave step: the code byte is the same address in every lane,
// its run or literal (at most 128 bytes) is two strides of the 64 lanes into LDS.  The row goes through LDS in chunks of 4096 pixels
// (16 KiB for the four planes); a code that straddles a chunk's end is stored in part and read again for the next chunk.  After the
// barrier all 256 threads convert the chunk and store the floats in memory order.
//
// The conversion kernel is arithmetic bound: per sub-sample one rsqrt, one acosf, one atan2f and twelve loads that neighbouring
// lanes share cache lines for; a 4096 x 2048 source (100 MB) stays in the Infinity Cache between the faces.
#include "common.h"
#include "../../include/gs2m_envmap.h"
#include <math.h>

namespace {

constexpr int ENV_THREADS = 256;
constexpr int DEC_CHUNK = 4096;  // pixels of a row in LDS at a time

// m 2^(e - 136) as fp32 bits, m in 0 .. 255, e in 1 .. 255: exact, normal or subnormal, whatever the float mode
__device__ __forceinline__ uint32_t rgbe_bits(uint32_t m, uint32_t e) {
    if (m == 0u) return 0u;
    const int p = 31 - __clz((int)m);  // 0 .. 7
    const int E = p + (int)e - 136;    // the value is 1.xxx 2^E
    if (E >= -126) return ((uint32_t)(E + 127) << 23) | ((m << (23 - p)) & 0x007FFFFFu);
    return m << (e + 13u);  // subnormal: m 2^(e - 136) = (m << (e + 13)) 2^-149, and p + e < 10 keeps it below 2^23
}

__global__ void __launch_bounds__(ENV_THREADS) hdr_decode_kernel(const uint8_t* __restrict__ bytes, long long nbytes, int W,
                                                                 const long long* __restrict__ table, float* __restrict__ out) {
    __shared__ uint8_t s_p[4][DEC_CHUNK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row = blockIdx.x;
    const long long* t = table + row * GS2M_HDR_TABLE_COLS;
    uint32_t* o = reinterpret_cast<uint32_t*>(out) + (size_t)row * (size_t)W * 3u;
    if (t[0] != GS2M_HDR_ROW_RLE) {  // (the same in every thread of the workgroup)
        const long long o0 = t[1];
        for (int j = tid; j < 3 * W; j += ENV_THREADS) {
            const int px = j / 3, ch = j - 3 * px;
            const long long b = o0 + 4LL * px;
            uint32_t v = 0u;
            if (b >= 0 && b + 3 < nbytes) {
                const uint32_t e = bytes[b + 3];
                if (e != 0u) v = rgbe_bits(bytes[b + ch], e);
            }
            o[j] = v;
        }
        return;
    }
    long long pos = t[1 + wave];  // this wave's plane: the next code byte
    int x = 0;                    // pixels of the plane expanded so far
    for (int lo = 0; lo < W; lo += DEC_CHUNK) {
        const int hi = min(lo + DEC_CHUNK, W);
        while (x < hi) {
            if (pos < 0 || pos >= nbytes) { x = W; break; }  // (not for a scanned table)
            const int c = bytes[pos];
            if (c == 0) { x = W; break; }                    // (not for a scanned table)
            const bool run = c > 128;
            const int n = min(run ? c - 128 : c, W - x);
            const uint8_t rv = (run && pos + 1 < nbytes) ? bytes[pos + 1] : (uint8_t)0;
            for (int k = lane; k < n; k += 64) {
                const int idx = x + k;
                if (idx >= lo && idx < hi) {
                    const long long q = pos + 1 + k;
                    s_p[wave][idx - lo] = run ? rv : (q < nbytes ? bytes[q] : (uint8_t)0);
                }
            }
            if (x + n > hi) break;  // the rest of this code belongs to the next chunk: it is read again there
            x += n;
            pos += run ? 2 : 1 + n;
        }
        gs2m_sync();
        const int cnt = 3 * (hi - lo);
        for (int j = tid; j < cnt; j += ENV_THREADS) {
            const int px = j / 3, ch = j - 3 * px;
            const uint32_t e = s_p[3][px];
            o[(size_t)lo * 3u + j] = e != 0u ? rgbe_bits(s_p[ch][px], e) : 0u;
        }
        gs2m_sync();
    }
}

__global__ void __launch_bounds__(ENV_THREADS) hdr_encode_kernel(long long n, const float* __restrict__ image, uint32_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * ENV_THREADS + threadIdx.x;
    if (i >= n) return;
    const float top = 255.0f * 0x1p119f;  // the largest value of the format: mantissa 255, exponent byte 255
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float a = image[i * 3 + k];
        c[k] = fminf(a > 0.f ? a : 0.f, top);  // NaN and negatives -> 0; +inf -> FLT_MAX -> top
    }
    const float v = fmaxf(c[0], fmaxf(c[1], c[2]));
    uint32_t word = 0u;
    if (!(v < 1e-32f)) {
        const int e = (int)((f2u(v) >> 23) & 0xFFu) - 126;            // frexpf's exponent of a normal number: v = f 2^e, 0.5 <= f < 1
        const float sc = u2f((uint32_t)(127 + 8 - e) << 23);          // 2^(8 - e), e in -106 .. 127
        word = (uint32_t)(int)(c[0] * sc) | ((uint32_t)(int)(c[1] * sc) << 8) | ((uint32_t)(int)(c[2] * sc) << 16) | ((uint32_t)(e + 128) << 24);
    }
    out[i] = word;
}

__device__ __forceinline__ int wrap_col(int i, int n) {
    i %= n;
    return i < 0 ? i + n : i;
}

__global__ void __launch_bounds__(ENV_THREADS) latlong_cube_kernel(const float* __restrict__ src, int Hs, int Ws, int R, int log2R, int S, float ca,
                                                                   float sa, float scale, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * ENV_THREADS + threadIdx.x;
    if (i >= (6LL << (2 * log2R))) return;
    const int c = (int)(i & (R - 1)), r = (int)((i >> log2R) & (R - 1)), f = (int)(i >> (2 * log2R));
    const float PI = 3.14159265358979323846f;
    const float denom = (float)(R * S), fw = (float)Ws, fh = (float)Hs;
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, wsum = 0.f;
    for (int a = 0; a < S; a++) {
        const float y = -1.0f + (float)(2 * (r * S + a) + 1) / denom;
        for (int b = 0; b < S; b++) {
            const float x = -1.0f + (float)(2 * (c * S + b) + 1) / denom;
            const float inv = 1.0f / sqrtf((1.0f + x * x) + y * y);
            const float w = (inv * inv) * inv;
            float dx, dy, dz;  // pbr/light.py cube_to_dir
            switch (f) {
                case 0: dx = 1.f; dy = -y; dz = -x; break;
                case 1: dx = -1.f; dy = -y; dz = x; break;
                case 2: dx = x; dy = 1.f; dz = y; break;
                case 3: dx = x; dy = -1.f; dz = -y; break;
                case 4: dx = x; dy = -y; dz = 1.f; break;
                default: dx = -x; dy = -y; dz = -1.f; break;
            }
            dx *= inv; dy *= inv; dz *= inv;
            const float rx = ca * dx - sa * dz, rz = sa * dx + ca * dz;
            const float theta = acosf(fminf(fmaxf(dy, -1.0f), 1.0f));
            const float phi = atan2f(rx, -rz);
            const float u = (phi / PI + 1.0f) * 0.5f * fw - 0.5f;
            const float v = theta / PI * fh - 0.5f;
            const float uf = floorf(u), vf = floorf(v);
            const float tu = u - uf, tv = v - vf;
            const int iu = (int)uf, iv = (int)vf;
            const int x0 = wrap_col(iu, Ws), x1 = wrap_col(iu + 1, Ws);
            const int y0 = min(max(iv, 0), Hs - 1), y1 = min(max(iv + 1, 0), Hs - 1);
            const float* p00 = src + ((size_t)y0 * Ws + x0) * 3;
            const float* p01 = src + ((size_t)y0 * Ws + x1) * 3;
            const float* p10 = src + ((size_t)y1 * Ws + x0) * 3;
            const float* p11 = src + ((size_t)y1 * Ws + x1) * 3;
            float L[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const float top = p00[k] + tu * (p01[k] - p00[k]);
                const float bot = p10[k] + tu * (p11[k] - p10[k]);
                L[k] = top + tv * (bot - top);
            }
            acc0 += w * L[0]; acc1 += w * L[1]; acc2 += w * L[2];
            wsum += w;
        }
    }
    float* o = out + i * 3;
    o[0] = scale * (acc0 / wsum);
    o[1] = scale * (acc1 / wsum);
    o[2] = scale * (acc2 / wsum);
}

}  // namespace

extern "C" {

int gs2m_hdr_scan(const unsigned char* bytes, long long nbytes, int W, int H, long long* table) {
    if (bytes == nullptr || table == nullptr || W < 1 || H < 1 || nbytes < 0) return GS2M_ERR_INVALID_ARG;
    const bool rle_width = W >= 8 && W <= 32767;
    long long pos = 0;
    for (int row = 0; row < H; row++) {
        long long* t = table + (long long)row * GS2M_HDR_TABLE_COLS;
        const bool rle = rle_width && nbytes - pos >= 4 && bytes[pos] == 2 && bytes[pos + 1] == 2 && (((int)bytes[pos + 2] << 8) | bytes[pos + 3]) == W;
        if (!rle) {
            if (nbytes - pos < 4LL * W) return GS2M_HDR_ERR_TRUNCATED;
            for (int x = 0; x < W; x++) {
                const unsigned char* q = bytes + pos + 4LL * x;
                if (q[0] == 1 && q[1] == 1 && q[2] == 1) return GS2M_HDR_ERR_OLD_RLE;
            }
            t[0] = GS2M_HDR_ROW_FLAT;
            for (int c = 0; c < 4; c++) t[1 + c] = pos + c;
            pos += 4LL * W;
            continue;
        }
        t[0] = GS2M_HDR_ROW_RLE;
        pos += 4;
        for (int c = 0; c < 4; c++) {
            t[1 + c] = pos;
            int x = 0;
            while (x < W) {
                if (pos >= nbytes) return GS2M_HDR_ERR_TRUNCATED;
                const int code = bytes[pos];
                if (code == 0) return GS2M_HDR_ERR_ZERO_CODE;
                const bool run = code > 128;
                const int n = run ? code - 128 : code;
                if (x + n > W) return GS2M_HDR_ERR_OVERRUN;
                const long long next = pos + (run ? 2 : 1 + n);
                if (next > nbytes) return GS2M_HDR_ERR_TRUNCATED;
                x += n;
                pos = next;
            }
        }
    }
    return pos == nbytes ? GS2M_OK : GS2M_HDR_ERR_TRAILING;
}

int gs2m_hdr_decode(const unsigned char* bytes, long long nbytes, int W, int H, const long long* table, float* out, void* stream) {
    if (bytes == nullptr || table == nullptr || out == nullptr || W < 1 || H < 1 || nbytes < 1) return GS2M_ERR_INVALID_ARG;
    if ((long long)W * 3 > 2147483647LL) return GS2M_ERR_UNSUPPORTED;
    hdr_decode_kernel<<<(unsigned)H, ENV_THREADS, 0, (hipStream_t)stream>>>(bytes, nbytes, W, table, out);
    return gs2m_status(hipGetLastError());
}

int gs2m_hdr_encode(int W, int H, const float* image, unsigned char* out, void* stream) {
    if (image == nullptr || out == nullptr || W < 1 || H < 1 || (uintptr_t)out % 4 != 0) return GS2M_ERR_INVALID_ARG;
    const long long n = (long long)W * H;
    const long long blocks = (n + ENV_THREADS - 1) / ENV_THREADS;
    if (blocks > 2147483647LL) return GS2M_ERR_UNSUPPORTED;
    hdr_encode_kernel<<<(unsigned)blocks, ENV_THREADS, 0, (hipStream_t)stream>>>(n, image, reinterpret_cast<uint32_t*>(out));
    return gs2m_status(hipGetLastError());
}

int gs2m_latlong_to_cubemap(int Hs, int Ws, const float* src, int R, int S, float angle, float scale, float* out, void* stream) {
    if (src == nullptr || out == nullptr || Hs < 2 || Ws < 2 || R < GS2M_ENVMAP_MIN_RES || (R & (R - 1)) != 0 || S < 1 || S > GS2M_ENVMAP_MAX_SAMPLES ||
        !isfinite(angle) || !isfinite(scale))
        return GS2M_ERR_INVALID_ARG;
    if (R > GS2M_ENVMAP_MAX_RES || (long long)Hs * Ws * 3 > 2147483647LL) return GS2M_ERR_UNSUPPORTED;
    int log2R = 0;
    while ((1 << log2R) < R) log2R++;
    const long long blocks = ((6LL << (2 * log2R)) + ENV_THREADS - 1) / ENV_THREADS;
    latlong_cube_kernel<<<(unsigned)blocks, ENV_THREADS, 0, (hipStream_t)stream>>>(src, Hs, Ws, R, log2R, S, (float)cos((double)angle),
                                                                                  (float)sin((double)angle), scale, out);
    return gs2m_status(hipGetLastError());
}

}  // extern "C"
