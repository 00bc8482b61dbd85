"""Writes gs-2m_amd/csrc/tnt_hot_r.h: matplotlib's hot_r colour map as its 256 x 3 table of doubles, hot_r(arange(256))[:, :3],
which a float x in [0, 1] indexes with min(trunc(x * 256), 255) (Colormap.__call__).  Every entry is written
with repr(), which reads back to the same double.  Needs matplotlib; the header is committed, so the build does not.

    python tools/make_hot_r_table.py
"""
import os

import matplotlib
import numpy as np

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gs-2m_amd", "csrc", "tnt_hot_r.h")


def table():
    return np.asarray(matplotlib.colormaps["hot_r"](np.arange(256))[:, :3], np.float64)


def main():
    t = table()
    x = np.linspace(0.0, 1.0, 100001)  # the equivalence the header rests on
    assert np.array_equal(matplotlib.colormaps["hot_r"](x)[:, :3], t[np.minimum((x * 256).astype(np.int64), 255)])
    rows = ["{" + ", ".join(repr(float(c)) for c in row) + "}" for row in t]
    with open(OUT, "w") as f:
        f.write(f"// matplotlib {matplotlib.__version__}'s hot_r colour map, hot_r(arange(256))[:, :3], as doubles (red, green, blue per entry).\n"
                "// Written by tools/make_hot_r_table.py; tests/test_tnt_clouds.py compares it with matplotlib's table.\n#pragma once\n"
                "#define GS2M_HOT_R_TABLE { \\\n    " + ", \\\n    ".join(rows) + " }\n")
    print(OUT)


if __name__ == "__main__":
    main()
