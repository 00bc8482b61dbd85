// The integer side of the triangle atlas (include/gs2m_atlas.h): class bases, Morton placement, atlas size, the owner of a
// texel and the chart's barycentrics.  Plain C++ for host and device: mesh_atlas.hip and mesh_bake.hip include it, and it
// compiles without HIP (tools/atlas_layout_check.cpp runs it under the host sanitizers).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ATLAS_HD __host__ __device__ __forceinline__
#else
#define ATLAS_HD inline
#endif

constexpr int ATLAS_CLASSES = 6;        // sides 8 << k, k = 0 .. 5
constexpr int ATLAS_MAX_WIDTH = 16384;  // GS2M_ATLAS_MAX_WIDTH

struct AtlasLayout {
    long long hist[ATLAS_CLASSES];   // triangles of class k
    long long start[ATLAS_CLASSES];  // sorted position of the class's first triangle (larger classes first)
    long long base[ATLAS_CLASSES];   // unit offset of the class's first cell
    long long total;                 // units of all classes
    int width, height;               // texels
};

// x from the even bits, y from the odd bits of a unit offset below 4^16
ATLAS_HD uint32_t atlas_compact_bits(uint64_t v) {
    v &= 0x5555555555555555ull;
    v = (v | (v >> 1)) & 0x3333333333333333ull;
    v = (v | (v >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    v = (v | (v >> 4)) & 0x00FF00FF00FF00FFull;
    v = (v | (v >> 8)) & 0x0000FFFF0000FFFFull;
    v = (v | (v >> 16)) & 0x00000000FFFFFFFFull;
    return (uint32_t)v;
}
ATLAS_HD uint64_t atlas_spread_bits(uint32_t x) {
    uint64_t v = x;
    v = (v | (v << 16)) & 0x0000FFFF0000FFFFull;
    v = (v | (v << 8)) & 0x00FF00FF00FF00FFull;
    v = (v | (v << 4)) & 0x0F0F0F0F0F0F0F0Full;
    v = (v | (v << 2)) & 0x3333333333333333ull;
    v = (v | (v << 1)) & 0x5555555555555555ull;
    return v;
}
ATLAS_HD void atlas_morton_decode(uint64_t m, int* x, int* y) {
    *x = (int)atlas_compact_bits(m);
    *y = (int)atlas_compact_bits(m >> 1);
}
ATLAS_HD uint64_t atlas_morton_encode(int x, int y) { return atlas_spread_bits((uint32_t)x) | (atlas_spread_bits((uint32_t)y) << 1); }

ATLAS_HD long long atlas_cells(long long count) { return (count + 1) / 2; }

// 0: fine; 1: a negative count or counts beyond 2^31 together; 2: wider than ATLAS_MAX_WIDTH (L then holds all but the size)
inline int atlas_layout(const long long* hist, AtlasLayout* L) {
    long long n = 0, units = 0;
    for (int k = ATLAS_CLASSES - 1; k >= 0; k--) {
        if (hist[k] < 0 || hist[k] > 0x7FFFFFFFll) return 1;
        L->hist[k] = hist[k];
        L->start[k] = n;
        L->base[k] = units;
        n += hist[k];
        units += atlas_cells(hist[k]) << (2 * k);
    }
    if (n > 0x7FFFFFFFll) return 1;
    L->total = units;
    L->width = L->height = 0;
    if (units == 0) return 0;
    int j = 0;
    while (j < 16 && (1ll << (2 * j)) < units) j++;
    if (8ll << j > ATLAS_MAX_WIDTH) return 2;
    L->width = 8 << j;
    L->height = j >= 1 && 2 * units <= (1ll << (2 * j)) ? L->width / 2 : L->width;
    return 0;
}

// the origin, in texels, of cell `cell` of class k
ATLAS_HD void atlas_cell_origin(const AtlasLayout& L, int k, long long cell, int* ox, int* oy) {
    int ux, uy;
    atlas_morton_decode((uint64_t)(L.base[k] + (cell << (2 * k))), &ux, &uy);
    *ox = 8 * ux, *oy = 8 * uy;
}

struct AtlasTexel {
    long long pos;  // the owner's sorted position
    int side, half, i, j;  // cell-local coordinates
};

// false: texel (X, Y), 0 <= X < width, 0 <= Y < height, is empty
ATLAS_HD bool atlas_texel(const AtlasLayout& L, int X, int Y, AtlasTexel* t) {
    const long long m = (long long)atlas_morton_encode(X >> 3, Y >> 3);
    if (m >= L.total) return false;
    int k = ATLAS_CLASSES - 1;  // the last class, in placement order, whose base is <= m and that has a cell
    for (int c = ATLAS_CLASSES - 2; c >= 0; c--)
        if (L.hist[c] > 0 && m >= L.base[c]) k = c;
    const long long cell = (m - L.base[k]) >> (2 * k);
    int ox, oy;
    atlas_cell_origin(L, k, cell, &ox, &oy);
    t->side = 8 << k;
    t->i = X - ox, t->j = Y - oy;
    t->half = t->i + t->j <= t->side - 1 ? 0 : 1;
    const long long rank = 2 * cell + t->half;
    if (rank >= L.hist[k]) return false;
    t->pos = L.start[k] + rank;
    return true;
}

// the chart's local corner coordinates, corner c = 0, 1, 2
ATLAS_HD void atlas_corner(int side, int half, int c, int* x, int* y) {
    const int Lc = side - 4, dx = c == 1 ? Lc : 0, dy = c == 2 ? Lc : 0;
    *x = half ? side - 1 - dx : 1 + dx;
    *y = half ? side - 1 - dy : 1 + dy;
}

// the clamped, renormalised barycentrics of texel (i, j) of half `half` of a cell of side `side`; returns `interior`
ATLAS_HD bool atlas_bary(int side, int half, int i, int j, double* l) {
    const int Lc = side - 4;
    const int a = 2 * (half ? side - 1 - i : i) - 1, b = 2 * (half ? side - 1 - j : j) - 1;
    const bool interior = a >= 0 && b >= 0 && a + b <= 2 * Lc;
    const double l1 = ((double)a * 0.5) / (double)Lc, l2 = ((double)b * 0.5) / (double)Lc;
    l[0] = (1.0 - l1) - l2, l[1] = l1, l[2] = l2;
    for (int k = 0; k < 3; k++) l[k] = l[k] > 0.0 ? l[k] : 0.0;
    const double sum = (l[0] + l[1]) + l[2];
    for (int k = 0; k < 3; k++) l[k] = l[k] / sum;
    return interior;
}
