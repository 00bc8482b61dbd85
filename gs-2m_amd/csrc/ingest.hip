// Dataset ingestion for gfx950: the reference's process_input_image (utils/image_utils.py:48-77) on the decoded bytes -- the
// mask_gt product, Pillow's default 8-bit resize (BICUBIC, two fixed-point passes), and the conversion to the planar floats the
// loop trains on (include/gs2m_ingest.h).  Integer arithmetic and fp32 evaluated as written (-ffp-contract=off):
// every output equals the reference's, byte for byte.
//
// The images stay interleaved (H, W, CH) as they are decoded; a row is a flat run of E = CH W bytes.
//   horizontal pass   a workgroup of 64 CH threads owns 64 output columns (all channels: thread = output byte of the row) and
//                     walks RESIZE_ROWS rows.  The columns' taps are the same for every row: they are staged in LDS once per
//                     tile (64 ksize ints; ksize is odd, so the lanes' rows start on different banks) and every row re-reads
//                     them from there.  Taps too long for LDS (ksize > 128: a reduction by more than 63) are read from global.
//   vertical pass     a workgroup of 256 threads owns one output row x 1024 bytes.  The row's bounds and taps depend on the
//                     work item only, which is derived from blockIdx: they are wave-uniform, live in scalar registers and are
//                     fetched by scalar loads; the lanes stream the bytes of the input rows, coalesced.
// Both passes walk their tiles grid-stride, accumulate in a 32-bit int and store bytes with plain vector stores; the uint8
// rounding between the passes is part of the result.  No atomics except the single atomicMax per workgroup of the maximum.
#include "common.h"
#include "../../include/gs2m_ingest.h"

#include <math.h>

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;  // Pillow's: 8 bits of pixel, 2 bits of headroom for the negative lobes
constexpr int RESIZE_COLS = 64;             // output columns of a horizontal tile
constexpr int RESIZE_ROWS = 8;              // rows of a horizontal tile
constexpr int RESIZE_LDS_KSIZE = 128;       // taps per column that still go to LDS (64 x 128 ints = 32 KiB)
constexpr int RESIZE_V_THREADS = 256, RESIZE_V_PER = 4;  // a vertical tile: 1024 bytes of one output row
constexpr unsigned MAX_GRID = 1024;         // workgroups of a grid-stride launch: 4 per CU

// ---- the plan (host, double precision: Pillow's precompute_coeffs + normalize_coeffs_8bpc) ------------------------------
struct Axis {
    double scale, filterscale, support;
    int ksize;
};

bool axis_of(int in, int out, Axis* a) {
    if (in < 1 || out < 1) return false;
    a->scale = (double)in / (double)out;
    a->filterscale = a->scale < 1.0 ? 1.0 : a->scale;
    a->support = 2.0 * a->filterscale;  // BICUBIC's support is 2
    const double k = ceil(a->support) * 2.0 + 1.0;
    if (k > 2147483647.0) return false;
    a->ksize = (int)k;
    return true;
}

inline double bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint8_t clip8(int acc) {
    const int v = acc >> PRECISION_BITS;  // arithmetic shift
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// bounds of output sample i, clamped so that [first, first + count) lies inside [0, in) and count <= ksize whatever the plan holds
__device__ __forceinline__ void plan_bounds(const int* __restrict__ bounds, size_t i, int in, int ksize, int& first, int& count) {
    const int b0 = bounds[2 * i], b1 = bounds[2 * i + 1];
    first = b0 < 0 ? 0 : (b0 > in - 1 ? in - 1 : b0);
    const int room = min(ksize, in - first);
    count = b1 < 0 ? 0 : (b1 > room ? room : b1);
}

template <int CH, bool LDSK>
__global__ void __launch_bounds__(RESIZE_COLS * CH) resize_h_kernel(int in_w, int rows, int out_w, int ksize, const int* __restrict__ bounds,
                                                                    const int* __restrict__ coeffs, const uint8_t* __restrict__ src,
                                                                    uint8_t* __restrict__ dst, long long tiles_x, long long tiles) {
    constexpr int T = RESIZE_COLS * CH;
    extern __shared__ int s_k[];  // LDSK: the taps of the tile's columns, ksize per column
    const int tid = threadIdx.x;
    const int col = tid / CH, c = tid - col * CH;
    const size_t in_e = (size_t)in_w * CH, out_e = (size_t)out_w * CH;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {  // the trip count depends on blockIdx only: the barriers are uniform
        const long long ty = t / tiles_x;
        const int x0 = (int)(t - ty * tiles_x) * RESIZE_COLS;
        const int ncol = min(RESIZE_COLS, out_w - x0);
        const size_t k0 = (size_t)x0 * (size_t)ksize;
        if (LDSK) {
            gs2m_sync();  // the previous tile's reads are done
            for (int i = tid; i < ncol * ksize; i += T) s_k[i] = coeffs[k0 + i];
            gs2m_sync();
        }
        if (col < ncol) {
            int first, count;
            plan_bounds(bounds, (size_t)(x0 + col), in_w, ksize, first, count);
            const int* __restrict__ kg = coeffs + k0 + (size_t)col * ksize;
            const int* ks = s_k + col * ksize;
            const long long y0 = ty * RESIZE_ROWS;
            const int ny = (int)min((long long)RESIZE_ROWS, rows - y0);
            const uint8_t* __restrict__ line = src + (size_t)y0 * in_e + (size_t)first * CH + c;
            uint8_t* __restrict__ o = dst + (size_t)y0 * out_e + (size_t)(x0 + col) * CH + c;
            for (int y = 0; y < ny; y++) {
                int acc = 1 << (PRECISION_BITS - 1);
                for (int x = 0; x < count; x++) acc += (int)line[(size_t)x * CH] * (LDSK ? ks[x] : kg[x]);
                *o = clip8(acc);
                line += in_e;
                o += out_e;
            }
        }
    }
}

__global__ void __launch_bounds__(RESIZE_V_THREADS) resize_v_kernel(long long E, int in_h, int ksize, const int* __restrict__ bounds,
                                                                    const int* __restrict__ coeffs, const uint8_t* __restrict__ src,
                                                                    uint8_t* __restrict__ dst, long long segs, long long items) {
    const int tid = threadIdx.x;
    for (long long t = blockIdx.x; t < items; t += gridDim.x) {
        const long long yy = t / segs;  // wave-uniform, as everything derived from it
        const long long e0 = (t - yy * segs) * (RESIZE_V_THREADS * RESIZE_V_PER) + tid;
        int first, count;
        plan_bounds(bounds, (size_t)yy, in_h, ksize, first, count);
        const int* __restrict__ k = coeffs + (size_t)yy * (size_t)ksize;
        int acc[RESIZE_V_PER];
#pragma unroll
        for (int j = 0; j < RESIZE_V_PER; j++) acc[j] = 1 << (PRECISION_BITS - 1);
        const uint8_t* __restrict__ row = src + (size_t)first * (size_t)E;
        for (int y = 0; y < count; y++) {
            const int kv = k[y];
#pragma unroll
            for (int j = 0; j < RESIZE_V_PER; j++) {
                const long long e = e0 + j * RESIZE_V_THREADS;
                if (e < E) acc[j] += (int)row[e] * kv;
            }
            row += E;
        }
        uint8_t* __restrict__ o = dst + (size_t)yy * (size_t)E;
#pragma unroll
        for (int j = 0; j < RESIZE_V_PER; j++) {
            const long long e = e0 + j * RESIZE_V_THREADS;
            if (e < E) o[e] = clip8(acc[j]);
        }
    }
}

__device__ __forceinline__ uint32_t max_bytes(uint32_t m, uint32_t v) {
    return max(max(m, v & 0xFFu), max(max((v >> 8) & 0xFFu, (v >> 16) & 0xFFu), v >> 24));
}

// *out was zeroed on the stream in front of this kernel.  The bytes in front of the first and behind the last 16-byte
// boundary go one by one (workgroup 0), the body as uint4.
__global__ void __launch_bounds__(256) max_u8_kernel(long long n, const uint8_t* __restrict__ src, int* __restrict__ out) {
    __shared__ uint32_t s_m[4];
    const int tid = threadIdx.x;
    const long long head = min(n, (long long)((16u - (uint32_t)((uintptr_t)src & 15u)) & 15u));
    const long long chunks = (n - head) / 16, tail = head + chunks * 16;
    const uint4* __restrict__ body = reinterpret_cast<const uint4*>(src + head);
    uint32_t m = 0u;
    for (long long i = (long long)blockIdx.x * 256 + tid; i < chunks; i += (long long)gridDim.x * 256) {
        const uint4 v = body[i];
        m = max_bytes(max_bytes(max_bytes(max_bytes(m, v.x), v.y), v.z), v.w);
    }
    if (blockIdx.x == 0) {
        for (long long i = tid; i < head; i += 256) m = max(m, (uint32_t)src[i]);
        for (long long i = tail + tid; i < n; i += 256) m = max(m, (uint32_t)src[i]);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d, 64));
    if ((tid & 63) == 0) s_m[tid >> 6] = m;
    gs2m_sync();
    if (tid == 0) {
        m = max(max(s_m[0], s_m[1]), max(s_m[2], s_m[3]));
        if (m != 0u) atomicMax(out, (int)m);
    }
}

__global__ void __launch_bounds__(256) mask_u8_kernel(long long elems, const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ alpha,
                                                      const int* __restrict__ max_ptr, uint8_t* __restrict__ dst) {
    const int mx = max_ptr[0];
    const float fm = (float)mx;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < elems; e += (long long)gridDim.x * 256) {
        const float a = (float)alpha[e / 3] / fm;
        float v = ((float)rgb[e] / 255.f) * a;
        v = fminf(fmaxf(v, 0.f), 1.f) * 255.f;
        dst[e] = mx > 0 ? (uint8_t)(int)v : (uint8_t)0;
    }
}

template <int CH>
__global__ void __launch_bounds__(256) unpack_kernel(long long pixels, const uint8_t* __restrict__ src, const uint8_t* __restrict__ alpha,
                                                     const int* __restrict__ max_ptr, float* __restrict__ rgb, float* __restrict__ alpha_out,
                                                     float* __restrict__ gray) {
    const int mx = alpha_out ? max_ptr[0] : 1;
    const float fm = (float)mx;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < pixels; p += (long long)gridDim.x * 256) {
        float v[CH];
#pragma unroll
        for (int c = 0; c < CH; c++) v[c] = (float)src[p * CH + c] / 255.f;
        if (rgb) {
#pragma unroll
            for (int c = 0; c < CH; c++) rgb[(long long)c * pixels + p] = v[c];
        }
        if (alpha_out) alpha_out[p] = mx > 0 ? (float)alpha[p] / fm : 0.f;
        if (CH == 3 && gray) gray[p] = (v[0] * 0.299f + v[1] * 0.587f) + v[CH - 1] * 0.114f;
    }
}

unsigned grid_for(long long items) { return (unsigned)(items < 1 ? 1 : (items > (long long)MAX_GRID ? (long long)MAX_GRID : items)); }

bool resize_sizes(int w, int h, int channels, int ow, int oh) {
    if (w < 1 || h < 1 || ow < 1 || oh < 1 || (channels != 1 && channels != 3)) return false;
    return (long long)w * channels <= 0x7FFFFFFFll && (long long)ow * channels <= 0x7FFFFFFFll;
}

template <int CH>
void launch_h(int in_w, int rows, int out_w, int ksize, const int* plan, const uint8_t* src, uint8_t* dst, hipStream_t s) {
    const int* bounds = plan + GS2M_RESIZE_PLAN_HEADER;
    const int* coeffs = bounds + 2 * (size_t)out_w;
    const long long tiles_x = ((long long)out_w + RESIZE_COLS - 1) / RESIZE_COLS;
    const long long tiles = tiles_x * (((long long)rows + RESIZE_ROWS - 1) / RESIZE_ROWS);
    if (ksize <= RESIZE_LDS_KSIZE)
        resize_h_kernel<CH, true><<<grid_for(tiles), RESIZE_COLS * CH, (size_t)RESIZE_COLS * ksize * sizeof(int), s>>>(
            in_w, rows, out_w, ksize, bounds, coeffs, src, dst, tiles_x, tiles);
    else
        resize_h_kernel<CH, false><<<grid_for(tiles), RESIZE_COLS * CH, 0, s>>>(in_w, rows, out_w, ksize, bounds, coeffs, src, dst, tiles_x, tiles);
}

void launch_v(long long E, int in_h, int out_h, int ksize, const int* plan, const uint8_t* src, uint8_t* dst, hipStream_t s) {
    const int* bounds = plan + GS2M_RESIZE_PLAN_HEADER;
    const int* coeffs = bounds + 2 * (size_t)out_h;
    const long long segs = (E + RESIZE_V_THREADS * RESIZE_V_PER - 1) / (RESIZE_V_THREADS * RESIZE_V_PER);
    const long long items = segs * out_h;
    resize_v_kernel<<<grid_for(items), RESIZE_V_THREADS, 0, s>>>(E, in_h, ksize, bounds, coeffs, src, dst, segs, items);
}

}  // namespace

extern "C" int gs2m_resize_plan_bytes(int in, int out, long long* bytes, int* ksize) {
    Axis a;
    if (!bytes || !axis_of(in, out, &a)) return GS2M_ERR_INVALID_ARG;
    *bytes = 4ll * (GS2M_RESIZE_PLAN_HEADER + 2ll * out + (long long)out * a.ksize);
    if (ksize) *ksize = a.ksize;
    return GS2M_OK;
}

extern "C" int gs2m_resize_plan(int in, int out, int* plan) {
    Axis a;
    if (!plan || !axis_of(in, out, &a)) return GS2M_ERR_INVALID_ARG;
    plan[0] = in; plan[1] = out; plan[2] = a.ksize; plan[3] = 0;
    int* bounds = plan + GS2M_RESIZE_PLAN_HEADER;
    int* coeffs = bounds + 2 * (size_t)out;
    double stack_w[64];
    double* w = a.ksize <= 64 ? stack_w : new double[a.ksize];
    for (int xx = 0; xx < out; xx++) {
        const double center = (xx + 0.5) * a.scale;
        long long xmin = (long long)(center - a.support + 0.5);
        if (xmin < 0) xmin = 0;
        long long xmax = (long long)(center + a.support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        double ww = 0.0;
        for (long long x = 0; x < xmax; x++) {
            w[x] = bicubic(((double)(x + xmin) - center + 0.5) / a.filterscale);
            ww += w[x];
        }
        int* k = coeffs + (size_t)xx * a.ksize;
        for (long long x = 0; x < a.ksize; x++) {
            double v = 0.0;
            if (x < xmax) v = ww != 0.0 ? w[x] / ww : w[x];
            k[x] = v < 0 ? (int)(-0.5 + v * (1 << PRECISION_BITS)) : (int)(0.5 + v * (1 << PRECISION_BITS));
        }
        bounds[2 * (size_t)xx] = (int)xmin;
        bounds[2 * (size_t)xx + 1] = (int)xmax;
    }
    if (w != stack_w) delete[] w;
    return GS2M_OK;
}

extern "C" int gs2m_image_max_u8(long long n, const unsigned char* src, int* out, void* stream) {
    if (n < 0 || !out || (n > 0 && !src)) return GS2M_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(out, 0, sizeof(int), s) != hipSuccess) return GS2M_ERR_HIP;
    if (n == 0) return GS2M_OK;
    max_u8_kernel<<<grid_for((n + 4095) / 4096), 256, 0, s>>>(n, src, out);
    return gs2m_status(hipGetLastError());
}

extern "C" int gs2m_image_mask_u8(int w, int h, const unsigned char* rgb_u8_hwc, const unsigned char* alpha_u8, const int* max_ptr,
                                  unsigned char* dst_u8_hwc, void* stream) {
    if (w < 1 || h < 1 || !rgb_u8_hwc || !alpha_u8 || !max_ptr || !dst_u8_hwc) return GS2M_ERR_INVALID_ARG;
    const long long elems = 3ll * w * h;
    mask_u8_kernel<<<grid_for((elems + 255) / 256), 256, 0, (hipStream_t)stream>>>(elems, rgb_u8_hwc, alpha_u8, max_ptr, dst_u8_hwc);
    return gs2m_status(hipGetLastError());
}

extern "C" int gs2m_image_resize_workspace_bytes(int w, int h, int channels, int ow, int oh, long long* bytes) {
    if (!bytes || !resize_sizes(w, h, channels, ow, oh)) return GS2M_ERR_INVALID_ARG;
    *bytes = (w != ow && h != oh) ? (long long)ow * channels * h : 0;
    return GS2M_OK;
}

extern "C" int gs2m_image_resize_u8(int w, int h, int channels, const unsigned char* src, int ow, int oh, const int* plan_x,
                                    const int* plan_y, unsigned char* tmp, unsigned char* dst, void* stream) {
    if (!src || !dst || !resize_sizes(w, h, channels, ow, oh)) return GS2M_ERR_INVALID_ARG;
    const bool hp = w != ow, vp = h != oh;
    Axis ax = {}, ay = {};
    if ((hp && (!plan_x || !axis_of(w, ow, &ax))) || (vp && (!plan_y || !axis_of(h, oh, &ay))) || (hp && vp && !tmp)) return GS2M_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (!hp && !vp) return gs2m_status(hipMemcpyAsync(dst, src, (size_t)w * channels * h, hipMemcpyDeviceToDevice, s));
    const unsigned char* mid = src;  // the vertical pass's input
    if (hp) {
        unsigned char* o = vp ? tmp : dst;
        if (channels == 1)
            launch_h<1>(w, h, ow, ax.ksize, plan_x, src, o, s);
        else
            launch_h<3>(w, h, ow, ax.ksize, plan_x, src, o, s);
        mid = o;
    }
    if (vp) launch_v((long long)ow * channels, h, oh, ay.ksize, plan_y, mid, dst, s);
    return gs2m_status(hipGetLastError());
}

extern "C" int gs2m_image_unpack(int w, int h, int channels, const unsigned char* src_u8_hwc, const unsigned char* alpha_u8,
                                 const int* alpha_max_ptr, float* rgb_chw, float* alpha_1hw, float* gray_1hw, void* stream) {
    if (w < 1 || h < 1 || (channels != 1 && channels != 3) || !src_u8_hwc) return GS2M_ERR_INVALID_ARG;
    if ((alpha_1hw && (!alpha_u8 || !alpha_max_ptr)) || (gray_1hw && channels != 3)) return GS2M_ERR_INVALID_ARG;
    const long long pixels = (long long)w * h;
    const unsigned grid = grid_for((pixels + 255) / 256);
    hipStream_t s = (hipStream_t)stream;
    if (channels == 1)
        unpack_kernel<1><<<grid, 256, 0, s>>>(pixels, src_u8_hwc, alpha_u8, alpha_max_ptr, rgb_chw, alpha_1hw, gray_1hw);
    else
        unpack_kernel<3><<<grid, 256, 0, s>>>(pixels, src_u8_hwc, alpha_u8, alpha_max_ptr, rgb_chw, alpha_1hw, gray_1hw);
    return gs2m_status(hipGetLastError());
}
