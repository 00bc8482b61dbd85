"""Writes gs-2m_amd/csrc/view_maps_magma.h: matplotlib's magma colour map as the 256 x 3 8-bit table
T = (magma(arange(256))[:, :3] * 255).astype(uint8) that save_depth_map's `plt.cm.magma(x)`, `(c * 255).astype(uint8)` indexes
with min(trunc(x * 256), 255).  Needs matplotlib; the header is committed, so the build does not.

    python tools/make_magma_table.py
"""
import os

import matplotlib
import matplotlib.pyplot as plt
import numpy as np

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gs-2m_amd", "csrc", "view_maps_magma.h")


def table():
    return (plt.cm.magma(np.arange(256))[:, :3] * 255).astype(np.uint8)


def main():
    t = table()
    x = np.linspace(0.0, 1.0, 100001, dtype=np.float32)  # the equivalence the header rests on
    assert np.array_equal((plt.cm.magma(x)[:, :3] * 255).astype(np.uint8), t[np.minimum((x * 256).astype(np.int64), 255)])
    rows = [", ".join(f"0x{(int(r) | int(g) << 8 | int(b) << 16 | 0xFF << 24):08X}u" for r, g, b in t[i:i + 8]) for i in range(0, 256, 8)]
    with open(OUT, "w") as f:
        f.write(f"// matplotlib {matplotlib.__version__}'s magma colour map, (magma(arange(256))[:, :3] * 255).astype(uint8), one little-endian RGBA\n"
                "// word per entry (alpha 255).  Written by tools/make_magma_table.py; tests/test_view_maps.py compares it with the table\n"
                "// recorded in tests/golden/ref_view_maps.npz.\n#pragma once\n"
                "#define GS2M_MAGMA_WORDS { \\\n    " + ", \\\n    ".join(rows) + " }\n")
    print(OUT)


if __name__ == "__main__":
    main()
