// PNG encoding for gfx950: row filters, deflate and Adler-32 of 8-bit images that already sit in device memory
// (include/gs2m_png.h).  Integer arithmetic only; the bytes written are a function of the image alone.
//
//   filter_kernel    a workgroup of 256 per row: the five PNG filters are priced in one pass over the row (the row above
//                    comes from L2), the 5 sums are reduced through the waves, and a second pass writes the cheapest one.
//   encode_kernel    a workgroup of 1024 per (image, segment); the segment (<= 64 KiB of filtered bytes) is staged in LDS
//                    and every thread owns one contiguous chunk of it (<= 64 bytes).
//                      parse     literals and matches of distance 1.  Inside a run of equal bytes the repeats are cut every 258
//                                bytes and a piece of 3 or more is a match -- what a greedy parse gives -- so a byte knows its
//                                token from its index in the run (a max-scan of the chunks' last run starts) and a look ahead of
//                                at most 258 bytes: no walk over the segment.
//                      codes     a histogram in LDS (integer atomics), then length-limited Huffman lengths: a rank sort by
//                                (count, symbol), the two-queue merge on one lane (285 steps), leaf depths in parallel, the
//                                over-long codes folded back by moving Kraft weight one code at a time (bounded by the number of
//                                symbols), lengths handed out in rank order.  Always complete, a function of the histogram.
//                      bits      a prefix sum of the chunks' bit counts, then every thread ORs its tokens into LDS words (OR
//                                commutes: the words do not depend on the order).  The smaller of the coded block and stored
//                                blocks goes to the segment's slot in the workspace, with its byte length.
//                      Adler     the segment's partial (A, B) from per-chunk sums.
//   scan_kernel      a workgroup of 256 per image: prefix sum of the segments' byte lengths (their offsets in the stream), the
//                    partial Adler sums combined, the stream's header, trailer and length.  Its own launch: no workgroup ever
//                    waits for another.
//   compact_kernel   a workgroup per segment copies the slot to its place in the stream.
// Every loop has a bound that can be read off the code; there is no spin-wait and no cross-workgroup communication inside a launch.
#include "common.h"
#include "../../include/gs2m_png.h"

#include <atomic>

namespace {

constexpr int FILTER_THREADS = 256;
constexpr int ENC_THREADS = 1024, ENC_WAVES = ENC_THREADS / 64;
constexpr int PTR_BATCH = 16;               // image pointers that travel in one filter launch's arguments
constexpr unsigned MAX_GRID = 1u << 20;     // workgroups of a grid-stride launch
constexpr int NLIT = 286, NCL = 19, MAXSEQ = NLIT + 1;  // literal/length symbols, code-length symbols, lengths a header describes
constexpr int LIT_BITS = 15, CL_BITS = 7;
constexpr uint32_t ADLER = 65521u;
constexpr int STORED_MAX = 65535;
constexpr int ENC_LDS_BUDGET = 150 * 1024;  // dynamic LDS of an encode workgroup: segment + bit buffer (<= 2 x 64 KiB + 26 bytes)

// ---- the plan (host) ---------------------------------------------------------------------------------------------------------
struct Plan {
    long long stride, rps, nseg, seg_full, image_bytes, max_stream;
    size_t cap_seg;  // bytes of a segment's slot in the workspace (and of the bit buffer in LDS): a multiple of 4
    size_t off_filtered, off_segbuf, off_segsize, off_adler, off_segoff, ws_bytes;
};

inline long long stored_bytes(long long b) { return b + 5 * ((b + STORED_MAX - 1) / STORED_MAX); }

int plan_of(int H, int W, int CH, int N, Plan* P) {
    if (H < 1 || W < 1 || N < 1 || (CH != 1 && CH != 3 && CH != 4)) return GS2M_ERR_INVALID_ARG;
    P->stride = 1 + (long long)W * CH;
    if (P->stride > GS2M_PNG_MAX_STRIDE || (long long)H * P->stride > 2147483647LL) return GS2M_ERR_UNSUPPORTED;
    P->rps = GS2M_PNG_SEGMENT_BYTES / P->stride < 1 ? 1 : GS2M_PNG_SEGMENT_BYTES / P->stride;
    P->nseg = (H + P->rps - 1) / P->rps;
    P->seg_full = (P->rps < H ? P->rps : H) * P->stride;  // <= 65536
    P->image_bytes = (long long)H * P->stride;
    const long long last = P->image_bytes - (P->nseg - 1) * P->rps * P->stride;
    P->max_stream = 2 + (P->nseg - 1) * stored_bytes(P->rps * P->stride) + stored_bytes(last) + 5 * (P->nseg - 1) + 4;
    P->cap_seg = (size_t)((stored_bytes(P->seg_full) + 5 + 3) / 4 * 4 + 8);
    const size_t segs = (size_t)N * (size_t)P->nseg;
    size_t o = 0;
    P->off_filtered = o; o = gs2m_align_up(o + (size_t)N * (size_t)P->image_bytes);
    P->off_segbuf = o;   o = gs2m_align_up(o + segs * P->cap_seg);
    P->off_segsize = o;  o = gs2m_align_up(o + segs * sizeof(uint32_t));
    P->off_adler = o;    o = gs2m_align_up(o + segs * sizeof(uint2));
    P->off_segoff = o;   o = gs2m_align_up(o + segs * sizeof(long long));
    P->ws_bytes = o;
    return GS2M_OK;
}

// ---- row filter ----------------------------------------------------------------------------------------------------------------
struct PngPtrs {
    const uint8_t* p[PTR_BATCH];
};

__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// the five filtered values of byte i of a row (cur; up: the row above or nullptr)
__device__ __forceinline__ void filter5(const uint8_t* __restrict__ cur, const uint8_t* __restrict__ up, int i, int bpp, int v[5]) {
    const int x = cur[i];
    const int a = i >= bpp ? cur[i - bpp] : 0;
    const int b = up != nullptr ? up[i] : 0;
    const int c = (up != nullptr && i >= bpp) ? up[i - bpp] : 0;
    v[0] = x;
    v[1] = (x - a) & 255;
    v[2] = (x - b) & 255;
    v[3] = (x - ((a + b) >> 1)) & 255;
    v[4] = (x - paeth(a, b, c)) & 255;
}

__global__ void __launch_bounds__(FILTER_THREADS) filter_kernel(PngPtrs imgs, int H, int row_bytes, int bpp, uint8_t* __restrict__ filtered,
                                                                long long rows) {
    __shared__ int s_cost[FILTER_THREADS / 64][5];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (long long r = blockIdx.x; r < rows; r += gridDim.x) {  // the trip count depends on blockIdx only: the barriers are uniform
        const int n = (int)(r / H), y = (int)(r - (long long)n * H);
        const uint8_t* __restrict__ cur = imgs.p[n] + (size_t)y * row_bytes;
        const uint8_t* __restrict__ up = y > 0 ? cur - row_bytes : nullptr;
        uint8_t* __restrict__ o = filtered + (size_t)r * (size_t)(row_bytes + 1);
        int cost[5] = {0, 0, 0, 0, 0};
        for (int i = tid; i < row_bytes; i += FILTER_THREADS) {
            int v[5];
            filter5(cur, up, i, bpp, v);
#pragma unroll
            for (int k = 0; k < 5; k++) cost[k] += v[k] < 128 ? v[k] : 256 - v[k];
        }
#pragma unroll
        for (int k = 0; k < 5; k++) {
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) cost[k] += __shfl_xor(cost[k], d, 64);
            if (lane == 0) s_cost[w][k] = cost[k];
        }
        gs2m_sync();
        int best = 0, best_cost = 0x7fffffff;
#pragma unroll
        for (int k = 0; k < 5; k++) {
            int c = 0;
#pragma unroll
            for (int j = 0; j < FILTER_THREADS / 64; j++) c += s_cost[j][k];
            if (c < best_cost) { best_cost = c; best = k; }  // ties: the lowest filter number
        }
        if (tid == 0) o[0] = (uint8_t)best;
        for (int i = tid; i < row_bytes; i += FILTER_THREADS) {
            int v[5];
            filter5(cur, up, i, bpp, v);
            o[1 + i] = (uint8_t)(best == 0 ? v[0] : best == 1 ? v[1] : best == 2 ? v[2] : best == 3 ? v[3] : v[4]);
        }
        gs2m_sync();  // s_cost is written again by the next row
    }
}

// ---- workgroup scans of the encode kernel (1024 threads) -----------------------------------------------------------------------
struct OpAdd {
    template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct OpMax {
    template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a > b ? a : b; }
};

// exclusive scan of one value per thread; *total: the whole workgroup's.  s_part: ENC_WAVES values of LDS.
template <typename T, typename Op>
__device__ __forceinline__ T enc_scan_exclusive(T v, T identity, Op op, T* s_part, T* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T t = __shfl_up(v, d, 64);
        if (lane >= d) v = op(t, v);
    }
    if (lane == 63) s_part[w] = v;
    T prev = __shfl_up(v, 1, 64);
    if (lane == 0) prev = identity;
    gs2m_sync();
    T off = identity, tot = identity;
#pragma unroll
    for (int k = 0; k < ENC_WAVES; k++) {
        const T x = s_part[k];
        if (k < w) off = op(off, x);
        tot = op(tot, x);
    }
    gs2m_sync();  // s_part may be written again by the next scan
    *total = tot;
    return op(off, prev);
}

// ---- Huffman construction --------------------------------------------------------------------------------------------------------
struct HuffScratch {
    uint32_t w[2 * NLIT];      // node weights: the used symbols in rank order, then the merged nodes
    uint16_t parent[2 * NLIT];
    uint16_t sorted[NLIT];     // symbol at each rank
    uint16_t depth[NLIT];      // leaf depth at each rank
    uint32_t cnt[16];          // codes per length
    int nused;
};

// lens[0 .. n) <- code lengths of at most `maxbits` for the counts freq[0 .. n), n <= NLIT: a complete prefix code over the symbols
// with a count (when fewer than two have one, symbols 0 and 1 count as used, so that the code is complete), 0 for the others.
// A function of the counts: ties go by symbol index.  Called by the whole workgroup.
__device__ void build_lengths(const uint32_t* freq, int n, int maxbits, uint32_t* lens, HuffScratch& h) {
    const int tid = threadIdx.x;
    if (tid < n) {
        int nused0 = 0;
        for (int j = 0; j < n; j++) nused0 += freq[j] > 0;
        const bool force = nused0 < 2;
        const uint32_t f = (force && tid < 2 && freq[tid] == 0) ? 1u : freq[tid];
        int rank = 0, nused = 0;
        for (int j = 0; j < n; j++) {
            const uint32_t fj = (force && j < 2 && freq[j] == 0) ? 1u : freq[j];
            nused += fj > 0;
            rank += fj > 0 && (fj < f || (fj == f && j < tid));
        }
        lens[tid] = 0;
        if (f > 0) {
            h.sorted[rank] = (uint16_t)tid;
            h.w[rank] = f;
        }
        if (tid == 0) h.nused = nused;
    }
    gs2m_sync();
    const int nused = h.nused;  // 2 .. n
    if (tid == 0) {  // the two-queue merge: leaves in rank order, merged nodes in the order they are made (their weights ascend)
        int li = 0, ni = nused, nn = nused;
        for (int k = 0; k < nused - 1; k++) {
            int pick[2];
#pragma unroll
            for (int t = 0; t < 2; t++) {
                if (li < nused && (ni >= nn || h.w[li] <= h.w[ni])) pick[t] = li++;
                else pick[t] = ni++;
            }
            h.w[nn] = h.w[pick[0]] + h.w[pick[1]];
            h.parent[pick[0]] = h.parent[pick[1]] = (uint16_t)nn;
            nn++;
        }
    }
    gs2m_sync();
    if (tid < nused) {
        const int root = 2 * nused - 2;
        int node = tid, d = 0;
        for (int it = 0; it < NLIT && node != root; it++) {  // a leaf is at most nused - 1 below the root
            node = h.parent[node];
            d++;
        }
        h.depth[tid] = (uint16_t)d;
    }
    if (tid < 16) h.cnt[tid] = 0;
    gs2m_sync();
    if (tid == 0) {
        uint32_t total = 0;  // Kraft sum in units of 2^-maxbits, after cutting the lengths at maxbits
        for (int r = 0; r < nused; r++) {
            const int d = h.depth[r] < maxbits ? h.depth[r] : maxbits;
            h.cnt[d]++;
            total += 1u << (maxbits - d);
        }
        // each step takes a code off the longest length, lengthens one shorter code by a bit and puts the first beside it: the
        // sum drops by one unit; it starts less than `nused` units above 1
        for (int it = 0; it < NLIT && total > (1u << maxbits); it++) {
            h.cnt[maxbits]--;
            for (int i = maxbits - 1; i > 0; i--)
                if (h.cnt[i]) {
                    h.cnt[i]--;
                    h.cnt[i + 1] += 2;
                    break;
                }
            total--;
        }
        int r = 0;  // rank order is ascending count: the rarest symbols take the longest codes
        for (int l = maxbits; l >= 1; l--)
            for (uint32_t c = 0; c < h.cnt[l] && r < nused; c++) lens[h.sorted[r++]] = (uint32_t)l;
    }
    gs2m_sync();
}

// canonical codes of lens[0 .. n), bit-reversed for the LSB-first stream.  s_bl: 16 words.  Called by the whole workgroup.
__device__ void make_codes(const uint32_t* lens, int n, uint32_t* codes, uint32_t* s_bl) {
    const int tid = threadIdx.x;
    if (tid < 16) {
        uint32_t c = 0;
        for (int j = 0; j < n; j++) c += lens[j] == (uint32_t)tid;
        s_bl[tid] = tid == 0 ? 0u : c;
    }
    gs2m_sync();
    if (tid < n) {
        const uint32_t l = lens[tid];
        uint32_t code = 0;
        if (l > 0) {
            for (uint32_t b = 1; b <= l; b++) code = (code + s_bl[b - 1]) << 1;  // l <= 15
            for (int j = 0; j < tid; j++) code += lens[j] == l;
            code = __brev(code) >> (32 - l);
        }
        codes[tid] = code;
    }
    gs2m_sync();
}

// ---- tokens --------------------------------------------------------------------------------------------------------------------
// length 3 .. 258 -> literal/length symbol, extra bits and their value (RFC 1951, 3.2.5)
__device__ __forceinline__ void length_symbol(int len, int& sym, int& ebits, int& evalue) {
    if (len == 258) { sym = 285; ebits = 0; evalue = 0; return; }
    const int x = len - 3;
    if (x < 8) { sym = 257 + x; ebits = 0; evalue = 0; return; }
    const int msb = 31 - __clz(x);  // 3 .. 7
    ebits = msb - 2;
    sym = 261 + 4 * ebits + ((x >> ebits) & 3);
    evalue = x & ((1 << ebits) - 1);
}

// The tokens whose first byte lies in [p0, p1) of the segment d[0 .. seglen): lit(byte) / match(length), in order.  k0: the number
// of bytes directly in front of p0 that repeat their predecessor.  A run's repeats are cut every 258 bytes; a piece of 3 or more
// is a match of distance 1, a shorter one literals.
template <typename FL, typename FM>
__device__ __forceinline__ void walk_tokens(const uint8_t* d, int p0, int p1, int seglen, int k0, FL&& lit, FM&& match) {
    int k = k0;
    for (int p = p0; p < p1; p++) {
        const int x = d[p];
        if (p == 0 || x != d[p - 1]) {
            k = 0;
            lit(x);
            continue;
        }
        const int m = k % 258;
        k++;
        if (m >= 2) continue;  // the piece began 2 or more bytes ago and reaches here: inside a match
        if (m == 1) {          // second byte of a piece: a match when the piece has a third
            if (!(p + 1 < seglen && d[p + 1] == x)) lit(x);
            continue;
        }
        int cnt = 1;
        for (int q = p + 1; q < seglen && cnt < 258 && d[q] == x; q++) cnt++;  // at most 257 steps
        if (cnt >= 3) match(cnt);
        else lit(x);
    }
}

__device__ __forceinline__ void put_bits(uint32_t* out, uint32_t bitpos, uint32_t value) {
    const uint64_t v = (uint64_t)value << (bitpos & 31);
    const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    if (lo) atomicOr(&out[bitpos >> 5], lo);
    if (hi) atomicOr(&out[(bitpos >> 5) + 1], hi);
}

__constant__ uint8_t CL_ORDER[NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__global__ void __launch_bounds__(ENC_THREADS) encode_kernel(int H, int stride, int rps, int nseg, int data_words, int cap_words,
                                                              const uint8_t* __restrict__ filtered, uint8_t* __restrict__ segbuf,
                                                              uint32_t* __restrict__ seg_size, uint2* __restrict__ seg_adler) {
    extern __shared__ uint32_t s_dyn[];
    uint32_t* s_dataw = s_dyn;                 // data_words: the segment's filtered bytes
    uint32_t* s_out = s_dyn + data_words;      // cap_words: the coded block
    uint8_t* s_data = reinterpret_cast<uint8_t*>(s_dataw);
    __shared__ uint32_t s_freq[NLIT], s_len[NLIT], s_code[NLIT];
    __shared__ uint32_t s_clfreq[NCL], s_cllen[NCL], s_clcode[NCL];
    __shared__ uint16_t s_cltok[MAXSEQ];       // the header's code-length tokens: symbol | extra value << 8
    __shared__ HuffScratch s_h;
    __shared__ uint32_t s_bl[16];
    __shared__ unsigned long long s_part64[ENC_WAVES];
    __shared__ int s_parti[ENC_WAVES];
    __shared__ uint32_t s_partu[ENC_WAVES];
    __shared__ uint32_t s_nmatch, s_hdrbits;
    __shared__ int s_ntok, s_hlit, s_hclen;

    const int tid = threadIdx.x;
    const size_t seg_id = blockIdx.x;          // n * nseg + s
    const int n = (int)(seg_id / (size_t)nseg), s = (int)(seg_id - (size_t)n * nseg);
    const int row0 = s * rps, row1 = min(H, row0 + rps);
    const int seglen = (row1 - row0) * stride;  // 1 .. 65536
    const bool last = s == nseg - 1;
    const uint8_t* __restrict__ src = filtered + ((size_t)n * H + row0) * (size_t)stride;

    for (int i = tid; i < seglen; i += ENC_THREADS) s_data[i] = src[i];
    for (int i = tid; i < NLIT; i += ENC_THREADS) s_freq[i] = 0;
    if (tid < NCL) s_clfreq[tid] = 0;
    if (tid == 0) s_nmatch = 0;
    gs2m_sync();

    // ---- the thread's chunk: its last run start and its Adler sums
    const int chunk = (seglen + ENC_THREADS - 1) / ENC_THREADS;  // 1 .. 64
    const int p0 = min(seglen, tid * chunk), p1 = min(seglen, p0 + chunk);
    int lb = -1;
    uint32_t sum1 = 0, sum2 = 0;  // sum of the bytes; sum of (p1 - p) byte[p]: <= 255 * 64 * 65 / 2
    for (int p = p0; p < p1; p++) {
        const uint32_t x = s_data[p];
        if (p == 0 || x != s_data[p - 1]) lb = p;
        sum1 += x;
        sum2 += (uint32_t)(p1 - p) * x;
    }
    int lb_all;
    const int lb_prev = enc_scan_exclusive(lb, -1, OpMax(), s_parti, &lb_all);
    const int k0 = p0 - 1 - lb_prev;  // (meaningless for p0 = 0, whose byte starts a run)
    {
        unsigned long long t_all, s_all;
        enc_scan_exclusive((unsigned long long)sum2 + (unsigned long long)sum1 * (unsigned long long)(seglen - p1), 0ull, OpAdd(), s_part64, &t_all);
        enc_scan_exclusive((unsigned long long)sum1, 0ull, OpAdd(), s_part64, &s_all);
        if (tid == 0) seg_adler[seg_id] = make_uint2((uint32_t)((1ull + s_all) % ADLER), (uint32_t)(((unsigned long long)seglen + t_all) % ADLER));
    }

    // ---- histogram
    walk_tokens(s_data, p0, p1, seglen, k0,
                [&](int x) { atomicAdd(&s_freq[x], 1u); },
                [&](int len) {
                    int sym, eb, ev;
                    length_symbol(len, sym, eb, ev);
                    atomicAdd(&s_freq[sym], 1u);
                    atomicAdd(&s_nmatch, 1u);
                });
    if (tid == 0) atomicAdd(&s_freq[256], 1u);  // end of block
    gs2m_sync();

    // ---- the literal/length code; the distance code is one symbol (distance 1) of one bit, or none
    build_lengths(s_freq, NLIT, LIT_BITS, s_len, s_h);
    make_codes(s_len, NLIT, s_code, s_bl);
    const uint32_t dist_len = s_nmatch > 0 ? 1u : 0u;

    // ---- the header's code-length sequence, run-length coded (symbols 16, 17, 18)
    if (tid == 0) {
        int hlit = NLIT;
        for (int i = NLIT - 1; i >= 257 && s_len[i] == 0; i--) hlit = i;  // the end of block (256) always has a code
        const int total = hlit + 1;  // + one distance length
        int ntok = 0, i = 0;
        for (int guard = 0; guard < MAXSEQ && i < total; guard++) {  // one run of equal lengths per step
            const uint32_t v = i < hlit ? s_len[i] : dist_len;
            int run = 1;
            for (int j = i + 1; j < total && (j < hlit ? s_len[j] : dist_len) == v; j++) run++;
            i += run;
            if (v == 0) {
                for (int g = 0; g < MAXSEQ && run >= 11; g++) {
                    const int r = run < 138 ? run : 138;
                    s_cltok[ntok++] = (uint16_t)(18 | ((r - 11) << 8));
                    run -= r;
                }
                if (run >= 3) {
                    s_cltok[ntok++] = (uint16_t)(17 | ((run - 3) << 8));
                    run = 0;
                }
            } else {
                s_cltok[ntok++] = (uint16_t)v;
                run--;
                for (int g = 0; g < MAXSEQ && run >= 3; g++) {
                    const int r = run < 6 ? run : 6;
                    s_cltok[ntok++] = (uint16_t)(16 | ((r - 3) << 8));
                    run -= r;
                }
            }
            for (int g = 0; g < 10 && run > 0; g++, run--) s_cltok[ntok++] = (uint16_t)v;  // what is left: fewer than 11
        }
        for (int t = 0; t < ntok; t++) s_clfreq[s_cltok[t] & 255]++;
        s_ntok = ntok;
        s_hlit = hlit;
    }
    gs2m_sync();
    build_lengths(s_clfreq, NCL, CL_BITS, s_cllen, s_h);
    make_codes(s_cllen, NCL, s_clcode, s_bl);
    if (tid == 0) {
        int hclen = 4;
        for (int i = 4; i < NCL; i++)
            if (s_cllen[CL_ORDER[i]] > 0) hclen = i + 1;
        uint32_t bits = 3 + 5 + 5 + 4 + 3 * hclen;
        for (int t = 0; t < s_ntok; t++) {
            const int sym = s_cltok[t] & 255;
            bits += s_cllen[sym] + (sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0);
        }
        s_hclen = hclen;
        s_hdrbits = bits;
    }

    // ---- bits of the chunk's tokens, their prefix sum
    uint32_t mybits = 0;
    walk_tokens(s_data, p0, p1, seglen, k0,
                [&](int x) { mybits += s_len[x]; },
                [&](int len) {
                    int sym, eb, ev;
                    length_symbol(len, sym, eb, ev);
                    mybits += s_len[sym] + eb + 1;
                });
    uint32_t tokbits;
    const uint32_t mybit0 = enc_scan_exclusive(mybits, 0u, OpAdd(), s_partu, &tokbits);  // (its barriers publish s_hdrbits)
    const uint32_t hdrbits = s_hdrbits;
    const uint32_t coded_bits = hdrbits + tokbits + s_len[256];  // <= 65536 * 15 + the header
    const uint32_t coded_bytes = last ? (coded_bits + 7) / 8 : (coded_bits + 3 + 7) / 8 + 4;
    const int nblk = (seglen + STORED_MAX - 1) / STORED_MAX;  // 1 or 2
    const uint32_t plain_bytes = (uint32_t)seglen + 5 * nblk + (last ? 0 : 5);
    uint8_t* __restrict__ dst = segbuf + seg_id * (size_t)cap_words * 4;

    if (coded_bytes < plain_bytes) {  // (workgroup-uniform)
        const int words = (int)(coded_bytes + 3) / 4;  // < cap_words
        for (int i = tid; i < words; i += ENC_THREADS) s_out[i] = 0;
        gs2m_sync();
        if (tid == 0) {
            uint32_t pos = 0;
            put_bits(s_out, pos, (last ? 1u : 0u) | (2u << 1)); pos += 3;
            put_bits(s_out, pos, (uint32_t)(s_hlit - 257)); pos += 5;
            put_bits(s_out, pos, 0u); pos += 5;  // one distance length
            put_bits(s_out, pos, (uint32_t)(s_hclen - 4)); pos += 4;
            for (int i = 0; i < s_hclen; i++) { put_bits(s_out, pos, s_cllen[CL_ORDER[i]]); pos += 3; }
            for (int t = 0; t < s_ntok; t++) {
                const int sym = s_cltok[t] & 255, ev = s_cltok[t] >> 8;
                put_bits(s_out, pos, s_clcode[sym]); pos += s_cllen[sym];
                const int eb = sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0;
                if (eb) { put_bits(s_out, pos, (uint32_t)ev); pos += eb; }
            }
            put_bits(s_out, hdrbits + tokbits, s_code[256]);
            if (!last) put_bits(s_out, 8 * (coded_bytes - 4), 0xFFFF0000u);  // the empty stored block: 000, padding, 00 00 FF FF
        }
        uint32_t pos = hdrbits + mybit0;
        walk_tokens(s_data, p0, p1, seglen, k0,
                    [&](int x) { put_bits(s_out, pos, s_code[x]); pos += s_len[x]; },
                    [&](int len) {
                        int sym, eb, ev;
                        length_symbol(len, sym, eb, ev);
                        const uint32_t l = s_len[sym];
                        put_bits(s_out, pos, s_code[sym] | ((uint32_t)ev << l));  // the distance code is one 0 bit
                        pos += l + eb + 1;
                    });
        gs2m_sync();
        uint32_t* __restrict__ dw = reinterpret_cast<uint32_t*>(dst);
        for (int i = tid; i < words; i += ENC_THREADS) dw[i] = s_out[i];
        if (tid == 0) seg_size[seg_id] = coded_bytes;
    } else {
        const int len1 = seglen < STORED_MAX ? seglen : STORED_MAX, len2 = seglen - len1;  // len2: 0 or 1
        if (tid == 0) {
            dst[0] = (uint8_t)((last && len2 == 0) ? 1 : 0);
            dst[1] = (uint8_t)(len1 & 255); dst[2] = (uint8_t)(len1 >> 8);
            dst[3] = (uint8_t)(~len1 & 255); dst[4] = (uint8_t)((~len1 >> 8) & 255);
            uint8_t* e = dst + 5 + len1;
            if (len2 > 0) {
                e[0] = (uint8_t)(last ? 1 : 0);
                e[1] = 1; e[2] = 0; e[3] = 0xFE; e[4] = 0xFF;
                e[5] = s_data[len1];
                e += 6;
            }
            if (!last) { e[0] = 0; e[1] = 0; e[2] = 0; e[3] = 0xFF; e[4] = 0xFF; }
            seg_size[seg_id] = plain_bytes;
        }
        for (int i = tid; i < len1; i += ENC_THREADS) dst[5 + i] = s_data[i];
    }
}

// ---- stream assembly -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) scan_kernel(int H, int stride, int rps, int nseg, const uint32_t* __restrict__ seg_size,
                                                   const uint2* __restrict__ seg_adler, long long* __restrict__ seg_off,
                                                   uint8_t* __restrict__ out, long long out_stride, long long* __restrict__ sizes) {
    __shared__ unsigned long long s_w[4];
    const int tid = threadIdx.x, n = blockIdx.x;
    const size_t base = (size_t)n * nseg;
    const long long image_bytes = (long long)H * stride;
    unsigned long long carry = 2, sa = 0, sb = 0;  // bytes in front of the tile; the thread's share of the Adler sums, mod 65521
    for (int t0 = 0; t0 < nseg; t0 += 256) {  // (workgroup-uniform trip count)
        const int sg = t0 + tid;
        unsigned long long sz = 0;
        if (sg < nseg) {
            sz = seg_size[base + sg];
            // (A, B, len) of segment sg joins what is in front of it by A = A1 + A2 - 1, B = B1 + B2 + len2 (A1 - 1); taken over all
            // segments in order that is A = 1 + sum (A_k - 1), B = sum (B_k + (A_k - 1) x bytes behind segment k), mod 65521
            const uint2 ab = seg_adler[base + sg];
            const long long end = (long long)min(H, (sg + 1) * rps) * stride;
            const unsigned long long behind = (unsigned long long)((image_bytes - end) % ADLER);
            sa = (sa + ab.x + ADLER - 1) % ADLER;
            sb = (sb + ab.y + (unsigned long long)((ab.x + ADLER - 1) % ADLER) * behind) % ADLER;
        }
        unsigned long long total;
        const unsigned long long off = gs2m_wg_exclusive_scan(sz, s_w, &total);
        if (sg < nseg) seg_off[base + sg] = (long long)(carry + off);
        carry += total;
    }
    unsigned long long ta, tb;
    gs2m_wg_exclusive_scan(sa, s_w, &ta);
    gs2m_wg_exclusive_scan(sb, s_w, &tb);
    if (tid == 0) {
        const uint32_t A = (uint32_t)((1 + ta) % ADLER), B = (uint32_t)(tb % ADLER);
        uint8_t* o = out + (size_t)n * (size_t)out_stride;
        o[0] = 0x78; o[1] = 0x01;
        o[carry] = (uint8_t)(B >> 8); o[carry + 1] = (uint8_t)B; o[carry + 2] = (uint8_t)(A >> 8); o[carry + 3] = (uint8_t)A;
        sizes[n] = (long long)(carry + 4);
    }
}

__global__ void __launch_bounds__(256) compact_kernel(int nseg, size_t cap_seg, const uint8_t* __restrict__ segbuf,
                                                      const uint32_t* __restrict__ seg_size, const long long* __restrict__ seg_off,
                                                      uint8_t* __restrict__ out, long long out_stride) {
    const size_t seg_id = blockIdx.x;
    const size_t n = seg_id / (size_t)nseg;
    const uint8_t* __restrict__ src = segbuf + seg_id * cap_seg;
    uint8_t* __restrict__ dst = out + n * (size_t)out_stride + (size_t)seg_off[seg_id];
    const uint32_t bytes = min(seg_size[seg_id], (uint32_t)cap_seg);
    for (uint32_t i = threadIdx.x; i < bytes; i += 256) dst[i] = src[i];
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
bool pointers_ok(int N, const unsigned char* const* images) {
    if (images == nullptr) return false;
    for (int n = 0; n < N; n++)
        if (images[n] == nullptr) return false;
    return true;
}

int launch_filter(const Plan& P, int N, int H, int W, int CH, const unsigned char* const* images, uint8_t* filtered, hipStream_t s) {
    for (int n0 = 0; n0 < N; n0 += PTR_BATCH) {
        PngPtrs ptrs = {};
        const int nb = N - n0 < PTR_BATCH ? N - n0 : PTR_BATCH;
        for (int k = 0; k < nb; k++) ptrs.p[k] = images[n0 + k];
        const long long rows = (long long)nb * H;
        const unsigned grid = (unsigned)(rows < (long long)MAX_GRID ? rows : (long long)MAX_GRID);
        filter_kernel<<<grid, FILTER_THREADS, 0, s>>>(ptrs, H, W * CH, CH, filtered + (size_t)n0 * (size_t)P.image_bytes, rows);
        if (hipGetLastError() != hipSuccess) return GS2M_ERR_HIP;
    }
    return GS2M_OK;
}

// More than 64 KB of dynamic LDS has to be allowed per kernel and per device (one bit per device; see texture.hip)
int allow_encode_lds() {
    static std::atomic<unsigned long long> allowed{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return GS2M_ERR_HIP;
    const unsigned long long bit = (dev >= 0 && dev < 64) ? 1ULL << dev : 0;
    if (allowed.load(std::memory_order_acquire) & bit) return GS2M_OK;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(encode_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, ENC_LDS_BUDGET) != hipSuccess)
        return GS2M_ERR_HIP;
    allowed.fetch_or(bit, std::memory_order_release);
    return GS2M_OK;
}

}  // namespace

extern "C" {

int gs2m_png_plan(int H, int W, int CH, int N, long long* rows_per_segment, long long* n_segments, long long* max_stream_bytes,
                  long long* workspace_bytes) {
    Plan P;
    const int rc = plan_of(H, W, CH, N, &P);
    if (rc != GS2M_OK) return rc;
    if (rows_per_segment) *rows_per_segment = P.rps;
    if (n_segments) *n_segments = P.nseg;
    if (max_stream_bytes) *max_stream_bytes = P.max_stream;
    if (workspace_bytes) *workspace_bytes = (long long)P.ws_bytes;
    return GS2M_OK;
}

int gs2m_png_filter(int N, int H, int W, int CH, const unsigned char* const* images, unsigned char* filtered, void* stream) {
    Plan P;
    const int rc = plan_of(H, W, CH, N, &P);
    if (rc != GS2M_OK) return rc;
    if (!pointers_ok(N, images) || filtered == nullptr) return GS2M_ERR_INVALID_ARG;
    return launch_filter(P, N, H, W, CH, images, filtered, (hipStream_t)stream);
}

int gs2m_png_encode(int N, int H, int W, int CH, const unsigned char* const* images, void* ws, long long ws_bytes,
                    unsigned char* out, long long out_stride, long long* sizes, void* stream) {
    Plan P;
    int rc = plan_of(H, W, CH, N, &P);
    if (rc != GS2M_OK) return rc;
    if (!pointers_ok(N, images) || ws == nullptr || out == nullptr || sizes == nullptr) return GS2M_ERR_INVALID_ARG;
    if ((uintptr_t)ws % GS2M_ALIGN != 0 || ws_bytes < (long long)P.ws_bytes || out_stride < P.max_stream) return GS2M_ERR_INVALID_ARG;
    const size_t segs = (size_t)N * (size_t)P.nseg;
    if (segs > 2147483647u) return GS2M_ERR_UNSUPPORTED;  // one workgroup per segment
    const int data_words = (int)((P.seg_full + 3) / 4), cap_words = (int)(P.cap_seg / 4);
    const size_t lds = (size_t)(data_words + cap_words) * 4;
    if (lds > (size_t)ENC_LDS_BUDGET) return GS2M_ERR_UNSUPPORTED;  // (cannot happen: both are bounded by the longest record)
    if ((rc = allow_encode_lds()) != GS2M_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* base = static_cast<char*>(ws);
    uint8_t* filtered = reinterpret_cast<uint8_t*>(base + P.off_filtered);
    uint8_t* segbuf = reinterpret_cast<uint8_t*>(base + P.off_segbuf);
    uint32_t* seg_size = reinterpret_cast<uint32_t*>(base + P.off_segsize);
    uint2* seg_adler = reinterpret_cast<uint2*>(base + P.off_adler);
    long long* seg_off = reinterpret_cast<long long*>(base + P.off_segoff);
    if ((rc = launch_filter(P, N, H, W, CH, images, filtered, s)) != GS2M_OK) return rc;
    encode_kernel<<<(unsigned)segs, ENC_THREADS, lds, s>>>(H, (int)P.stride, (int)P.rps, (int)P.nseg, data_words, cap_words, filtered, segbuf,
                                                           seg_size, seg_adler);
    if (hipGetLastError() != hipSuccess) return GS2M_ERR_HIP;
    scan_kernel<<<(unsigned)N, 256, 0, s>>>(H, (int)P.stride, (int)P.rps, (int)P.nseg, seg_size, seg_adler, seg_off, out, out_stride, sizes);
    if (hipGetLastError() != hipSuccess) return GS2M_ERR_HIP;
    compact_kernel<<<(unsigned)segs, 256, 0, s>>>((int)P.nseg, P.cap_seg, segbuf, seg_size, seg_off, out, out_stride);
    return hipGetLastError() == hipSuccess ? GS2M_OK : GS2M_ERR_HIP;
}

}  // extern "C"
