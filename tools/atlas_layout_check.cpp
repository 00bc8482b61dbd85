// Host-only check of the atlas's index arithmetic (gs-2m_amd/csrc/atlas_layout.h): for a set of class histograms, every cell's
// origin is inside the atlas and aligned to its side, no two cells overlap, every texel of the atlas resolves to at most one
// (sorted position, half), and every triangle's half owns exactly its texels.  Plain C++, no GPU: build it with the host
// sanitizers and run it,
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/atlas_layout_check.cpp -o atlas_layout_check
// exit status 0 and "ok" when every histogram passes.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../gs-2m_amd/csrc/atlas_layout.h"

static int fail(const char* what, const long long* h) {
    std::fprintf(stderr, "FAILED: %s for hist %lld %lld %lld %lld %lld %lld\n", what, h[0], h[1], h[2], h[3], h[4], h[5]);
    return 1;
}

static int check(const long long* h) {
    AtlasLayout L;
    const int st = atlas_layout(h, &L);
    if (st == 2) return 0;  // wider than the limit: nothing to index
    if (st != 0) return fail("layout", h);
    const size_t W = (size_t)L.width, H = (size_t)L.height;
    std::vector<unsigned char> cover(W * H, 0);
    long long n = 0;
    for (int k = 0; k < ATLAS_CLASSES; k++) {
        n += h[k];
        const int side = 8 << k;
        if (L.base[k] % (1ll << (2 * k))) return fail("base alignment", h);
        for (long long m = 0; m < atlas_cells(h[k]); m++) {
            int ox, oy;
            atlas_cell_origin(L, k, m, &ox, &oy);
            if (ox < 0 || oy < 0 || ox % side || oy % side || (size_t)(ox + side) > W || (size_t)(oy + side) > H) return fail("cell origin", h);
            for (int j = 0; j < side; j++)
                for (int i = 0; i < side; i++)
                    if (cover[(size_t)(oy + j) * W + (size_t)(ox + i)]++) return fail("overlap", h);
        }
    }
    std::vector<long long> owned((size_t)n, 0);
    for (size_t Y = 0; Y < H; Y++)
        for (size_t X = 0; X < W; X++) {
            AtlasTexel t;
            if (!atlas_texel(L, (int)X, (int)Y, &t)) continue;
            if (!cover[Y * W + X] || t.pos < 0 || t.pos >= n || t.i < 0 || t.j < 0 || t.i >= t.side || t.j >= t.side) return fail("texel", h);
            double l[3];
            atlas_bary(t.side, t.half, t.i, t.j, l);
            if (!(l[0] >= 0.0 && l[1] >= 0.0 && l[2] >= 0.0 && l[0] + l[1] + l[2] > 0.999 && l[0] + l[1] + l[2] < 1.001)) return fail("barycentrics", h);
            owned[(size_t)t.pos]++;
        }
    for (int k = 0; k < ATLAS_CLASSES; k++)
        for (long long r = 0; r < h[k]; r++) {
            const long long s = 8 << k, want = r % 2 == 0 ? s * (s + 1) / 2 : s * (s - 1) / 2;
            if (owned[(size_t)(L.start[k] + r)] != want) return fail("texels per half", h);
        }
    for (uint64_t m = 0; m < 4096; m++) {
        int x, y;
        atlas_morton_decode(m * 1023u, &x, &y);
        if (atlas_morton_encode(x, y) != m * 1023u) return fail("morton", h);
    }
    return 0;
}

int main() {
    const long long fixed[][ATLAS_CLASSES] = {{0, 0, 0, 0, 0, 0}, {1, 0, 0, 0, 0, 0}, {2, 0, 0, 0, 0, 0}, {3, 0, 0, 0, 0, 0}, {4, 0, 0, 0, 0, 0},
                                              {1, 1, 1, 1, 1, 1}, {1, 0, 0, 0, 0, 1}, {2, 0, 1, 0, 0, 0}, {70, 0, 0, 0, 0, 0}, {64, 0, 0, 0, 0, 0},
                                              {0, 120, 200, 0, 0, 0}, {0, 0, 72, 0, 0, 0}, {5000, 300, 70, 9, 3, 1}, {0, 0, 0, 0, 0, 8192},
                                              {0, 0, 0, 0, 0, 8193}, {0x7FFFFFFFll, 0, 0, 0, 0, 0}, {-1, 0, 0, 0, 0, 0}};
    int bad = 0;
    for (const auto& h : fixed) {
        if (h[0] < 0 || h[5] == 8192) {  // refused, or too large to walk here: the layout alone
            AtlasLayout L;
            const int st = atlas_layout(h, &L);
            if (h[0] < 0 ? st != 1 : (st != 0 || L.width != ATLAS_MAX_WIDTH)) bad += fail("limits", h);
            continue;
        }
        bad += check(h);
    }
    unsigned long long seed = 12345;
    for (int it = 0; it < 200; it++) {
        long long h[ATLAS_CLASSES];
        for (int k = 0; k < ATLAS_CLASSES; k++) {
            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
            h[k] = (seed >> 60) < 6 ? 0 : (long long)((seed >> 33) % (k < 3 ? 40 : 5));
        }
        bad += check(h);
    }
    if (bad) return 1;
    std::puts("ok");
    return 0;
}
