// Per-quadrant front-to-back alpha compositing (forward) for gfx950.
//
// Semantics: renderCUDA, diff-gaussian-rasterization/cuda_rasterizer/forward.cu:246-372 -- the same per-pixel
// sequence of tests and updates, on the per-quadrant lists tile_sort.hip builds.
//
// One wave per 8x8 quadrant, pixel per lane, no workgroup barriers: every list entry survives the quadrant test by
// construction, so the wave walks its list straight down, 16 entries per chunk.  The chunk's blend records are
// gathered by the wave itself (lane = entry x record quad, full 16-B loads) a whole chunk ahead of their use and
// parked in LDS; the evaluation reads them back with wave-uniform (broadcast) addresses at constant offsets, so the
// inner loop is fully unrolled and spends no vector instruction on addressing, ballot walks or quadrant tests.
// Lane predicates live in SGPR pairs as wave masks.  A first version fetched the records with SCALAR loads
// (s_load_dwordx8 one entry ahead, SGPR operands): it ran at half the speed -- scalar loads return out of order, so
// the only wait is "all of them", the prefetch distance is one evaluation, and the ~0.45 us load latency was exposed
// on every entry.
// Two other forms were built and measured: the alpha of two consecutive entries as packed fp32
// pairs out of a component-wise LDS layout (5 fewer vector instructions per entry, but 76 VGPRs = 6 waves per SIMD
// and the LDS reads right in front of their use: 0.30 instead of 0.27 ms), and the scalar-load form with the record
// lines touched ahead by a vector load (no better: the scalar path itself is the latency).
// What goes through which path (profiles/blend_fwd_scalar_ab.md):
//   geometry (6 dwords) and the channel quads (12 at fc 9): global -> VGPR -> LDS a chunk ahead, read back per entry as
//     broadcast ds_read_b128 / one ds_read_b64: 19 LDS-array cycles per entry and wave;
//   the entry's id: stays in a VGPR of the wave (lane = entry of the chunk), read by v_readlane on the observe path only;
//   the entry's position in the tile list: not carried.  A pixel's last contributor is kept as (slot in the chunk, an
//     inline constant of the select; list index, folded once per chunk) and becomes a position by ONE gather from the
//     list behind the loop.  Before, {id, position + 1} was a fourth LDS read per entry which the compiler fused with
//     the geometry's second read into a ds_read2_b64 (8 LDS cycles for 16 bytes): 25 cycles per entry, the LDS array
//     78 % busy and 12 % of the wave time spent waiting to issue an LDS instruction (now 2 %).  0.268 -> 0.255 ms.
//   Channel quads as the packed FMAs' scalar operands (scalar loads two entries ahead, geometry alone in LDS) were built
//     and lost, 0.373 ms: profiles/blend_fwd_scalar_ab.md, NOTEBOOK.md.
// `observe` (forward.cu:348-350: one atomicAdd per pixel) is one integer atomic per (list entry, quadrant) that sees
// a pixel with T > 0.5, straight into the output tensor (zeroed by the preprocess kernel): only the first few
// entries of a list do, and the wave stops looking once no live pixel has T > 0.5.
#include "common.h"

#include <type_traits>

namespace {

typedef float v2f __attribute__((ext_vector_type(2)));

// f(integral_constant<J>), J = 0 .. N - 1, fully unrolled with J a compile-time constant; stops when f returns true
template <int J, int N, class F>
__device__ __forceinline__ bool unrolled_until(F&& f) {
    if constexpr (J < N) {
        if (f(std::integral_constant<int, J>{})) return true;
        return unrolled_until<J + 1, N>(f);
    } else {
        return false;
    }
}

template <int FC>  // feature channels blended (compile time); runtime fc <= FC
__global__ void __launch_bounds__(64) blend_fwd_q_kernel(
    const uint2* __restrict__ ranges, const uint2* __restrict__ qlist, const uint32_t* __restrict__ qcount,
    const float4* __restrict__ rec, int W, int H, int tiles_x, int tiles, const float* __restrict__ bg, int fc,
    float* __restrict__ out_color, float* __restrict__ out_buffer, float* __restrict__ final_T,
    uint32_t* __restrict__ n_contrib, int* __restrict__ observe, uint32_t* __restrict__ qlast) {
    constexpr int NC = 3 + FC;        // blended channels: r, g, b, features
    constexpr int KQ = (NC + 3) / 4;  // channel quads of the record
    constexpr int NP = (NC + 1) / 2;  // channel pairs accumulated

    const int b = blockIdx.x;
    const int tile = (b >> 5) * 8 + (b & 7);  // the four quadrants of a tile run on one XCD (block ids go round the 8 XCDs)
    const int quad = (b >> 3) & 3;
    if (tile >= tiles) return;
    const int lane = threadIdx.x;
    const int tile_x = tile % tiles_x, tile_y = tile / tiles_x;
    const int qx0 = tile_x * GS2M_TILE + (quad & 1) * 8, qy0 = tile_y * GS2M_TILE + (quad >> 1) * 8;
    if (qx0 >= W || qy0 >= H) return;
    const int px = qx0 + (lane & 7), py = qy0 + (lane >> 3);
    const bool inside = px < W && py < H;
    const float pxf = (float)px, pyf = (float)py;

    const uint2 range = ranges[tile];
    const uint32_t len = range.y - range.x;
    const int n = __builtin_amdgcn_readfirstlane((int)qcount[tile * 4 + quad]);
    const uint2* list = qlist + (size_t)4 * range.x + (size_t)quad * len;

    // record quads parked per entry: geo0, geo1, channel quads (the bin quad is only needed on the rare observe path)
    constexpr int CH = 16;       // entries per chunk
    constexpr int NS = 2 + KQ;   // quads staged
    // one LDS block, [buffer][NS quads][CH], addressed from ONE per-buffer base kept in a VGPR the compiler cannot
    // rematerialise: with separate arrays at known addresses it re-creates two address registers from SGPRs for every
    // entry (2 of 32 vector instructions).  The chunk's Gaussian ids stay in a VGPR (lane = entry), read by v_readlane on the
    // rare observe path; list positions are not carried at all (see last_slot)
    constexpr int BUFQ = NS * CH;  // float4 per buffer
    __shared__ float4 s_buf[2 * BUFQ];
    uint32_t lds_zero;
    asm volatile("v_mov_b32 %0, 0" : "=v"(lds_zero));  // opaque 0
    float4* const s_base = s_buf + lds_zero;
    auto q_at = [&](int buf, int slot, int jj) -> float4& { return s_base[buf * BUFQ + slot * CH + jj]; };
    const int ej = lane & 15, eq = lane >> 4;  // staging role: entry ej of the chunk, quad slot eq (and eq + 4)
    auto quad_of = [](int slot) { return slot < 2 ? slot : slot + 1; };  // staged slot -> record quad (skips REC_BIN)

    float T = 1.0f;
    // the last contributor in two levels, so that the per-entry select takes an inline constant and nothing is read for it:
    uint32_t last_slot = 0;   // slot + 1 in the CURRENT chunk of the last entry this pixel accepted, 0: none in this chunk
    uint32_t last_index = 0;  // list index + 1 of the last entry of an EARLIER chunk this pixel accepted, 0: none
    v2f acc[NP];  // acc[k] = channels 2k, 2k + 1
#pragma unroll
    for (int k = 0; k < NP; k++) acc[k] = v2f{0.f, 0.f};
    // Lane predicates are kept as wave masks in SGPR pairs and combined on the scalar unit; the selects take the
    // mask as v_cndmask's scalar operand.  (As `bool`s carried round the loop the compiler keeps them in VGPRs and
    // spends ~8 vector instructions per entry converting back and forth.)
    typedef unsigned long long mask_t;
    mask_t live = __builtin_amdgcn_ballot_w64(inside);  // pixels that have not finished (forward.cu:288, 340-343)
    bool watch = true;  // some live pixel may still have T > 0.5 (wave-uniform)
    int ilast = 0;      // list entries up to and including the last one some pixel accepted (wave-uniform)

    // one list entry (index i of the list, slot jj of LDS buffer `buf`, the chunk's ids in `ids`): returns true when every
    // pixel has finished
    auto eval = [&](const int i, const int buf, auto jc, const uint32_t ids) {
        constexpr int jj = decltype(jc)::value;
        const float4 a = q_at(buf, 0, jj);
        const float2 b = *reinterpret_cast<const float2*>(&q_at(buf, 1, jj));
        float4 c[KQ];
#pragma unroll
        for (int q = 0; q < KQ; q++) c[q] = q_at(buf, 2 + q, jj);
        const float dx = a.x - pxf, dy = a.y - pyf;
        const float p2 = gs2m_power(dx, dy, a.z, a.w, b.x);
        const float alpha = fminf(0.99f, b.y * gs2m_exp(p2));
        const float test_T = T * (1.0f - alpha);
        const mask_t cand = live & __builtin_amdgcn_ballot_w64(p2 <= 0.0f) & __builtin_amdgcn_ballot_w64(alpha >= 1.0f / 255.0f);
        const mask_t fin = cand & __builtin_amdgcn_ballot_w64(test_T < 0.0001f);  // these pixels stop here, without this entry
        const mask_t contrib = cand & ~fin;
        live &= ~fin;
        if (contrib != 0ull) ilast = i + 1;
        float tw;  // contrib ? T : 0 -- branch-free: non-contributing lanes add 0
        asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(tw) : "v"(T), "s"(contrib));
        // w and test_T share one register PAIR whose halves are both written here: a packed FMA names the pair (it reads w for
        // both halves, op_sel), and with the upper half left undefined the allocator may put it on the destination of a load
        // still in flight -- the compiler then waits for that load (the next chunk's records) in front of the first entry
        v2f wt = {alpha * tw, test_T};
        asm("" : "+v"(wt));
        const v2f ww = __builtin_shufflevector(wt, wt, 0, 0);
#pragma unroll
        for (int q = 0; q < KQ; q++) {
            if (4 * q < NC) acc[2 * q] = __builtin_elementwise_fma(v2f{c[q].x, c[q].y}, ww, acc[2 * q]);
            if (4 * q + 2 < NC) acc[2 * q + 1] = __builtin_elementwise_fma(v2f{c[q].z, c[q].w}, ww, acc[2 * q + 1]);
        }
        asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(last_slot) : "n"(jj + 1), "s"(contrib));
        if (watch) {
            const mask_t half = contrib & __builtin_amdgcn_ballot_w64(T > 0.5f);
            if (half != 0ull) {  // rare: only the front of a list
                const uint32_t gid = (uint32_t)__builtin_amdgcn_readlane((int)ids, jj) & GS2M_GID_MASK;
                if (lane == 0) atomicAdd(&observe[gid], (int)__popcll(half));  // integer: the order does not matter
            }
            // T only falls: once no live pixel is above 0.5 nothing later can be
            watch = (live & __builtin_amdgcn_ballot_w64(T > 0.5f)) != 0ull;
        }
        asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(T) : "v"(wt.y), "s"(contrib));
        return live == 0ull;
    };

    // Software pipeline by chunks of 16 entries: while chunk c is evaluated out of LDS buffer c & 1, the record quads
    // of chunk c + 1 are in flight towards registers (written to the other buffer after the evaluation) and the ids
    // of chunk c + 2 are being fetched.  One wave, in-order LDS: no barriers.
    const int nchunks = (n + CH - 1) / CH;
    auto load_entry = [&](int c) {  // id of entry ej of chunk c (clamped inside the list: the surplus lanes are never evaluated)
        return list[min(c * CH + ej, n - 1)].x;
    };
    struct Stage { float4 a, b; };
    auto load_quads = [&](const uint32_t e) {  // this lane's two quads of its entry's record
        Stage st;
        const float4* p = rec + (size_t)(e & GS2M_GID_MASK) * REC_Q;  // the entry carries the quadrant-hit mask above the id
        st.a = p[quad_of(eq)];
        st.b = eq + 4 < NS ? p[quad_of(eq + 4)] : make_float4(0.f, 0.f, 0.f, 0.f);
        return st;
    };
    auto park = [&](int buf, const Stage& st) {
        q_at(buf, eq, ej) = st.a;
        if (eq + 4 < NS) q_at(buf, eq + 4, ej) = st.b;
    };
    if (nchunks > 0) {
        uint32_t ids = load_entry(0);  // chunk c
        park(0, load_quads(ids));
        uint32_t e1 = nchunks > 1 ? load_entry(1) : ids;
        bool stop = false;
        for (int c = 0; c < nchunks && !stop; c++) {
            Stage st;
            const uint32_t ecur = e1;  // chunk c + 1
            if (c + 1 < nchunks) st = load_quads(ecur);
            if (c + 2 < nchunks) e1 = load_entry(c + 2);
            const int base = c * CH, buf = c & 1;
            bool every = false;  // every pixel has finished
            unrolled_until<0, CH>([&](auto jc) {
                if (base + decltype(jc)::value >= n) return true;
                every = eval(base + decltype(jc)::value, buf, jc, ids);
                return every;
            });
            stop = every;
            last_index = last_slot != 0u ? (uint32_t)base + last_slot : last_index;
            last_slot = 0u;
            if (c + 1 < nchunks && !stop) park(buf ^ 1, st);
            ids = ecur;
        }
    }

    if (lane == 0) qlast[tile * 4 + quad] = (uint32_t)ilast;
    if (inside) {
        const size_t HW = (size_t)H * W;
        const size_t pix = (size_t)py * W + px;
        final_T[pix] = T;
        // position in the tile list + 1 of the last contributor, as the reference counts contributors: one gather
        n_contrib[pix] = last_index != 0u ? list[last_index - 1u].y + 1u : 0u;
        out_color[pix] = acc[0][0] + T * bg[0];
        out_color[HW + pix] = acc[0][1] + T * bg[1];
        out_color[2 * HW + pix] = acc[1][0] + T * bg[2];
#pragma unroll
        for (int ch = 0; ch < GS2M_NUM_FEATURES; ch++) {
            const int cch = 3 + ch;
            out_buffer[ch * HW + pix] = (ch < FC && ch < fc) ? acc[(cch >> 1) < NP ? (cch >> 1) : 0][cch & 1] : 0.0f;
        }
    }
}

}  // namespace

void gs2m_launch_blend_fwd_q(int W, int H, int tiles_x, int tiles_y, int fc, const float* bg, const GeomState& g,
                             const BinningState& b, const ImageState& im, float* out_color, float* out_buffer,
                             int* out_observe, hipStream_t s) {
    const int tiles = tiles_x * tiles_y;
    const int grid = ((tiles + 7) / 8) * 32;
    const int fct = fc <= 1 ? 1 : (fc <= 5 ? 5 : (fc <= 9 ? 9 : 10));
#define GS2M_FWDQ(FC)                                                                                                   \
    blend_fwd_q_kernel<FC><<<grid, 64, 0, s>>>(im.ranges, b.qlist, im.qcount, g.rec, W, H, tiles_x, tiles, bg, fc, out_color, \
                                               out_buffer, im.final_T, im.n_contrib, out_observe, im.qlast)
    switch (fct) {
        case 1: GS2M_FWDQ(1); break;
        case 5: GS2M_FWDQ(5); break;
        case 9: GS2M_FWDQ(9); break;
        default: GS2M_FWDQ(10); break;
    }
#undef GS2M_FWDQ
}
