"""The texture backward (csrc/texture.hip: texture_bwd_kernel, shade_bwd_kernel) alone, texel by texel against the
float64 transpose of oracle/texture_oracle.py.  Both kernels accumulate through one sink (TexelSink, laid out by plan_sink),
and both are held to the same bound on each of its paths: the 16-lane run merge, the workgroup-private LDS copies, the LDS
combining table and its overflow to global atomics, the LDS budget fallback, both pixel orders; for the fused shading
backward also its clamp gate and an irradiance map that is too wide for LDS and goes straight to memory.

The bound, per gradient texel and channel, is

    |got - want| <= 8 * 2^-24 * (w_level + cnt) * S + 1e-12

S = sum over the texel's contributions of |scale dy| (scale = the level blend factor), cnt = their number, both from the
oracle.  Where it comes from: the texel-space coordinate u w - 0.5 carries an absolute error of ~w ulp(1) (the forward tests
note the same loss), which enters each of the two bilinear fractions; each of the cnt atomic adds rounds once against a
running sum bounded by S; the factor 8 covers the product of the two fractions, the level blend and the corner third.  For a
2-D texture w_level is the larger of width and height.  The constant is fixed by that derivation, not fitted; no case has an
exception budget, and a texel the oracle gives no contribution must be exactly 0.  Every test prints its worst err / bound.
"""
import ctypes as C
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from test_texture_gpu import _dirs  # noqa: E402  (the forward tests' generator: a third near edges, a third near corners)

EPS = 2.0 ** -24
COMB_HT = 2048             # csrc/texture.hip: slots of the combining table
LDS_MAX_WIDTH = 32         # levels up to this width get a private LDS copy
LDS_BUDGET = 159 * 1024    # bytes: private copies + table


# ------------------------------------------------------------------------------------------------ inputs and references
def _smooth(H, W, slow=1.0):
    """A direction field that changes slowly along a row, from row to row faster: neighbouring pixels land on the same
    texel, in runs that are long in the first rows and short in the last."""
    yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    span = np.linspace(0.3, 1.6, H)[:, None] * slow
    return torch.from_numpy(np.stack([0.1 + span * xx, -0.2 + 0.3 * slow * yy, np.ones_like(xx)], axis=-1).astype(np.float32))


_ODD = torch.tensor([[float("nan"), 0.0, 1.0], [0.0, 0.0, 0.0], [float("inf"), float("inf"), 1.0], [0.0, 0.0, 0.0],
                     [float("nan")] * 3, [float("-inf"), 1.0, 0.0]])


def _inputs(H, W, C, seed, band, spread_rows=0, slow=1.0):
    """dirs (H, W, 3), dy (H, W, C): `_dirs` everywhere but rows band[0]:band[1], which hold a smooth field; six non-finite
    / all-zero directions, half of them inside the band; ~10 % of the pixels with dy == 0 at random places, so inside the
    band they sit in the middle of runs.  `spread_rows`: that many leading rows are `_dirs` without its near-edge and
    near-corner shares (those crowd onto few texels), the shares follow in the rows after them; `slow` scales the band's
    extent on the cube."""
    g = torch.Generator().manual_seed(1000 + seed)
    d = _dirs(H * W, seed).view(H, W, 3).clone()
    if spread_rows:
        d = torch.cat([_dirs(spread_rows * W, seed, near_edges=False).view(spread_rows, W, 3), d[:H - spread_rows]])
    r0, r1 = band
    d[r0:r1] = _smooth(r1 - r0, W, slow)
    flat = d.view(-1, 3)
    spots = torch.cat([torch.randint(0, H * W, (3,), generator=g), r0 * W + torch.randint(0, (r1 - r0) * W, (3,), generator=g)])
    flat[spots] = _ODD
    dy = torch.randn(H * W, C, generator=g)
    dy[torch.rand(H * W, generator=g) < 0.1] = 0.0
    return d, dy.view(H, W, C), g


def _bias(n, nlevels, g):
    """[-0.7, nlevels - 0.2]: below 0 and above the last level included, and every exact level."""
    b = torch.rand(n, generator=g) * (nlevels + 0.5) - 0.7
    top = float(nlevels - 1)
    b[:50] = torch.tensor([0.0, 1.0, 2.0, top, top - 0.001]).repeat(10)
    return b


# name -> (level widths, C, H, W, mip by bias, rows of the smooth band[, leading rows of spread-out directions[, slow]])
CASES = {
    "lds_c1": ((8,), 1, 37, 45, False, (12, 24)), "lds_c2": ((8,), 2, 37, 45, False, (12, 24)),
    "lds_c3": ((8,), 3, 37, 45, False, (12, 24)), "lds_c4": ((8,), 4, 37, 45, False, (12, 24)),
    "two_images": ((8,), 3, 38, 45, False, (15, 23)),           # fed as (2, 19, 45, 3): the band crosses the seam
    "runs": ((4,), 3, 48, 64, False, (0, 48)),
    "table_random": ((128, 64, 32, 16), 3, 40, 70, True, (38, 40), 32),
    # a quarter of the extent: a tile of the band keeps to a few hundred texels of the 128 and 64 levels
    "table_smooth": ((128, 64, 32, 16), 3, 40, 70, True, (0, 40), 0, 0.25),
    "budget_c4": ((32, 16, 8), 4, 37, 45, True, (12, 24)), "budget_c3": ((32, 16, 8), 3, 37, 45, True, (12, 24)),
    "thin": ((64, 16), 2, 700, 3, True, (200, 400)),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs and the float64 reference of one case, computed once and shared by the tests that use it."""
    from oracle import texture_oracle as O
    widths, Cc, H, W, mip, band = CASES[name][:6]
    d, dy, g = _inputs(H, W, Cc, sorted(CASES).index(name), band, *CASES[name][6:])
    bias = _bias(H * W, len(widths), g) if mip else None
    dn, dyn, bn = d.view(-1, 3).numpy(), dy.view(-1, Cc).numpy(), None if bias is None else bias.numpy()
    level, texel, weight, scale = O.cube_contributions(widths, dn, bn)
    want, S, cnt = O._scatter([(6, w, w, Cc) for w in widths], level, texel, (weight, scale), dyn)
    live = (texel >= 0) & (dyn != 0).any(axis=1)[:, None, None]
    keys = np.where(live, (level << 24) | texel, -1).reshape(H * W, 8)
    return types.SimpleNamespace(name=name, widths=widths, C=Cc, H=H, W=W, dirs=d, dy=dy, bias=bias, want=want, S=S, cnt=cnt, keys=keys)


def _check(name, got, want, S, cnt, w_level):
    """-> worst err / bound over the tensor; texels without a contribution must be exactly 0."""
    got = np.asarray(got, dtype=np.float64).reshape(want.shape)
    assert (got[cnt == 0] == 0).all(), f"{name}: a texel the oracle gives nothing is not 0"
    bound = 8 * EPS * (w_level + cnt[..., None]) * S + 1e-12
    worst = float((np.abs(got - want) / bound).max())
    print(f"ERR/BOUND {name} w={w_level}: {worst:.4f}")
    return worst


def _check_levels(name, got, ref, times=1, factor=1):
    worst = max(_check(f"{name}[L{l}]", got[l].cpu().numpy(), times * ref.want[l], times * ref.S[l], times * ref.cnt[l], factor * w)
                for l, w in enumerate(ref.widths))
    assert worst <= 1.0, f"{name}: err / bound = {worst}"
    return worst


def _through_dr_texture(ref, batch=1):
    import nvdiffrast.torch as dr
    g = torch.Generator().manual_seed(7)
    texs = [torch.rand(1, 6, w, w, ref.C, generator=g).cuda().requires_grad_(True) for w in ref.widths]
    uv = ref.dirs.view(batch, ref.H // batch, ref.W, 3).cuda()
    if ref.bias is None:
        out = dr.texture(texs[0], uv, filter_mode="linear", boundary_mode="cube")
    else:
        out = dr.texture(texs[0], uv, mip=texs[1:], mip_level_bias=ref.bias.view(batch, ref.H // batch, ref.W).cuda(),
                         filter_mode="linear-mipmap-linear", boundary_mode="cube")
    grads = torch.autograd.grad(out, texs, ref.dy.view(out.shape).cuda())
    return [x[0] for x in grads]


def _native_cube_backward(ref, image_width, grads=None):
    import gs2m_native as N
    dev = torch.device("cuda")
    if grads is None:
        grads = [torch.zeros(6, w, w, ref.C, device=dev) for w in ref.widths]
    d, dy = ref.dirs.view(-1, 3).to(dev), ref.dy.reshape(-1, ref.C).to(dev)
    bias = None if ref.bias is None else ref.bias.to(dev)
    N.launch("gs2m_texture_cube_backward", dev, d.shape[0], ref.C, len(grads), (C.c_void_p * len(grads))(*[x.data_ptr() for x in grads]),
             (C.c_int * len(grads))(*ref.widths), d.data_ptr(), N.ptr(bias), dy.data_ptr(), image_width)
    torch.cuda.synchronize()
    return grads


# ------------------------------------------------------------------------------------ the kernel's lane order, from the oracle
def _lane_keys(keys, n, img_w):
    """keys (n, 8) -> (tiles, 1024, 8) in the order `tile_pixel` gives the 1024 threads of a workgroup their pixels: 32 x 32
    image tiles for img_w > 0, else runs of 1024; -1 where a thread has no pixel."""
    t = np.arange(1024)
    if img_w > 0:
        img_h, tiles_x = n // img_w, (img_w + 31) // 32
        tile = np.arange(tiles_x * ((img_h + 31) // 32))[:, None]
        x, y = (tile % tiles_x) * 32 + (t & 31), (tile // tiles_x) * 32 + (t >> 5)
        pix = np.where((x < img_w) & (y < img_h), y * img_w + x, -1)
    else:
        pix = np.arange((n + 1023) // 1024)[:, None] * 1024 + t
        pix = np.where(pix < n, pix, -1)
    return np.where(pix[..., None] >= 0, keys[np.maximum(pix, 0)], -1)


def _run_statistics(lanes):
    """-> (histogram {run length: count} of equal non-negative keys inside the 16-lane rows, number of equal-key pairs
    that straddle a row boundary, number of 'A, -1, A' gaps inside a row), over the eight texel slots of a pixel."""
    hist, straddle, gaps = {}, 0, 0
    for s in range(lanes.shape[-1]):
        k = lanes[..., s].reshape(-1, 1024)
        straddle += int(((k[:, 15:1023:16] == k[:, 16:1024:16]) & (k[:, 15:1023:16] >= 0)).sum())
        rows = k.reshape(-1, 16)
        gaps += int(((rows[:, :-2] == rows[:, 2:]) & (rows[:, :-2] >= 0) & (rows[:, 1:-1] < 0)).sum())
        for row in rows:
            start = 0
            for j in range(1, 17):
                if j == 16 or row[j] != row[start]:
                    if row[start] >= 0:
                        hist[j - start] = hist.get(j - start, 0) + 1
                    start = j
    return hist, straddle, gaps


def _table_load(ref, img_w):
    """per pixel tile: (number of distinct (level, texel) keys on the levels that go through the combining table, longest
    run of occupied slots those keys leave in the table).  The set of occupied slots of linear probing does not depend on
    the order of insertion, and a probe sequence ends at the first free slot of its cluster: with no cluster longer than
    the 8 probes nothing overflows, whatever the order of the threads."""
    lanes = _lane_keys(ref.keys, ref.H * ref.W, img_w)
    table_levels = [l for l, w in enumerate(ref.widths) if w > LDS_MAX_WIDTH]
    out = []
    for t in lanes:
        keys = np.unique(t[(t >= 0) & np.isin(t >> 24, table_levels)])
        used = np.zeros(COMB_HT, dtype=bool)
        for k in keys[:COMB_HT]:
            h = ((int(k) * 2654435761) & 0xFFFFFFFF) >> 21
            while used[h]:
                h = (h + 1) & (COMB_HT - 1)
            used[h] = True
        run = longest = 0
        for u in np.concatenate([used, used]):                  # the table wraps around
            run = run + 1 if u else 0
            longest = max(longest, run)
        out.append((int(keys.size), min(longest, COMB_HT)))
    return out


# ------------------------------------------------------------------------------------------------ the texture backward
@pytest.mark.parametrize("name", ["lds_c1", "lds_c2", "lds_c3", "lds_c4"])
def test_private_lds_path_every_channel_count(name):
    """w = 8 at every C, a 37 x 45 image: ragged against the 32 x 32 tile and the 16-lane row; the level is LDS-private."""
    ref = _case(name)
    _check_levels(name, _through_dr_texture(ref), ref)


def test_private_lds_path_tile_across_two_images():
    """uv (2, 19, 45, 3): the backward sees one 38-row image, so the tile of rows 0 .. 31 holds pixels of both."""
    ref = _case("two_images")
    _check_levels("two_images", _through_dr_texture(ref, batch=2), ref)


def test_run_merge_on_a_smooth_field():
    ref = _case("runs")
    hist, straddle, gaps = _run_statistics(_lane_keys(ref.keys, ref.H * ref.W, ref.W))
    print("run lengths:", dict(sorted(hist.items())), "row-straddling pairs:", straddle, "mid-run gaps:", gaps)
    assert sum(c for r, c in hist.items() if r >= 8) > 0 and all(hist.get(r, 0) > 0 for r in range(2, 17))
    assert straddle > 0 and gaps > 0
    _check_levels("runs", _through_dr_texture(ref), ref)


def test_table_path_overflows_on_random_directions():
    """levels (128, 64) cannot be privatised; random directions put more distinct keys into a tile than the table has slots,
    so the eight probes fail and the adds go straight to memory."""
    ref = _case("table_random")
    load = _table_load(ref, ref.W)
    print("table keys, longest cluster per tile:", load)
    assert max(n for n, _ in load) > COMB_HT
    _check_levels("table_random", _through_dr_texture(ref), ref)


def test_table_path_without_overflow_on_a_smooth_field():
    ref = _case("table_smooth")
    load = _table_load(ref, ref.W)
    print("table keys, longest cluster per tile:", load)
    assert all(n > 0 for n, _ in load) and max(c for _, c in load) <= 8
    _check_levels("table_smooth", _through_dr_texture(ref), ref)


def _lds_bytes(widths, Cc):
    private = sum(6 * w * w * Cc * 4 for w in widths if w <= LDS_MAX_WIDTH)
    return private, COMB_HT * (1 + Cc) * 4


def test_budget_fallback_demotes_the_widest_private_level():
    """(32, 16, 8) at C = 4: private copies 6 (1024 + 256 + 64) 4 floats = 129024 B, table 2048 (1 + 4) 4 = 40960 B, together
    169984 B > 159 KiB = 162816 B: the width-32 level is demoted to the table and the other two are re-packed.  At C = 3:
    96768 B + 32768 B = 129536 B, no demotion."""
    assert _lds_bytes((32, 16, 8), 4) == (129024, 40960) and 129024 + 40960 > LDS_BUDGET
    assert 129024 - 6 * 32 * 32 * 4 * 4 + 40960 <= LDS_BUDGET                     # one demotion suffices
    assert _lds_bytes((32, 16, 8), 3) == (96768, 32768) and 96768 + 32768 <= LDS_BUDGET
    for name in ("budget_c4", "budget_c3"):
        ref = _case(name)
        _check_levels(name, _through_dr_texture(ref), ref)


@functools.lru_cache(maxsize=None)
def _case_2d(H, W, Cc):
    from oracle import texture_oracle as O
    g = torch.Generator().manual_seed(H + W + Cc)
    n = 2800
    uv = torch.rand(n, 2, generator=g) * 1.2 - 0.1
    uv[:8] = torch.tensor([[0.0, 0.0], [1.0, 1.0], [0.5 / W, 0.5 / H], [1 - 0.5 / W, 0.3], [0.3, 1 - 0.5 / H], [0.5, 0.5], [-1.0, 2.0],
                           [1.5 / W, 1.5 / H]])
    xx = torch.linspace(0.2, 0.2 + 3.0 / W, 600)                # a slow sweep: runs of equal texels
    uv[100:700] = torch.stack([xx, 0.4 + 0.0 * xx], dim=-1)
    dy = torch.randn(n, Cc, generator=g)
    dy[torch.rand(n, generator=g) < 0.1] = 0.0
    texel, weight = O.tex2d_contributions(H, W, uv.numpy())
    return uv, dy, texel, weight


@pytest.mark.parametrize("H,W,Cc", [(40, 24, 2), (24, 40, 2), (200, 8, 1), (256, 256, 2)])
def test_tex2d_clamp_backward(H, W, Cc):
    """(40, 24) is LDS-private (width <= 32, height <= 192); width 40, height 200 and the (256, 256, 2) BRDF table go through
    the combining table.  The entry point has no image width: pixels are taken in runs of 1024, so n = 1, 700, 1024, 2800
    are part of a run, most of one, exactly one, and 2.7."""
    import nvdiffrast.torch as dr
    from oracle import texture_oracle as O
    assert (W <= LDS_MAX_WIDTH and H <= 6 * LDS_MAX_WIDTH) == ((H, W) == (40, 24))          # the kernel's rule for a private copy
    uv, dy, texel, weight = _case_2d(H, W, Cc)
    tex = torch.rand(1, H, W, Cc, generator=torch.Generator().manual_seed(1)).cuda().requires_grad_(True)
    worst = 0.0
    for n in (1, 700, 1024, 2800):
        out = dr.texture(tex, uv[:n].view(1, 1, n, 2).cuda(), filter_mode="linear", boundary_mode="clamp")
        (got,) = torch.autograd.grad(out, [tex], dy[:n].view(1, 1, n, Cc).cuda())
        want, S, cnt = O._scatter([(H, W, Cc)], np.zeros_like(texel[:n]), texel[:n], (weight[:n], np.ones_like(weight[:n])), dy[:n].numpy())
        worst = max(worst, _check(f"2d {H}x{W}x{Cc} n={n}", got[0].cpu().numpy(), want[0], S[0], cnt[0], max(H, W)))
    assert worst <= 1.0


def test_both_pixel_orders_and_the_accumulation_contract():
    """gs2m_texture_cube_backward directly: image tiles (image_width = W) and runs of 1024 (image_width = 0) on the same
    inputs; then a second call into the same tensors, which must hold twice the gradient (the header: accumulated)."""
    ref = _case("table_random")
    tiled = _native_cube_backward(ref, ref.W)
    _check_levels("order tiles", tiled, ref)
    _check_levels("order runs-of-1024", _native_cube_backward(ref, 0), ref)
    again = _native_cube_backward(ref, ref.W, grads=tiled)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(again, tiled))
    _check_levels("accumulated twice", again, ref, times=2)


def test_thin_image_pixel_tiles():
    """a 3 x 700 image with image_width = 3: 22 tiles of 32 rows, three valid lanes in each 32-lane tile row."""
    ref = _case("thin")
    assert (ref.H, ref.W) == (700, 3)
    _check_levels("thin", _native_cube_backward(ref, 3), ref)


def test_texel_index_must_fit_the_key():
    """The merge / table key holds the texel index in 24 bits.  C = 1, real zero-filled gradient tensors of the true size and
    dy == 0, so that no add is issued whether the size is refused or not."""
    import gs2m_native as N
    dev = torch.device("cuda")
    n = 64
    d, uv, dy = _dirs(n, 3).to(dev), torch.rand(n, 2, device=dev), torch.zeros(n, 1, device=dev)

    def cube(w):
        g = torch.zeros(6, w, w, 1, device=dev)
        N.launch("gs2m_texture_cube_backward", dev, n, 1, 1, (C.c_void_p * 1)(g.data_ptr()), (C.c_int * 1)(w), d.data_ptr(), None, dy.data_ptr(), 0)
        torch.cuda.synchronize()
        return g

    def flat(w, h):
        g = torch.zeros(h, w, 1, device=dev)
        N.launch("gs2m_texture_2d_clamp_backward", dev, n, 1, w, h, g.data_ptr(), uv.data_ptr(), dy.data_ptr())
        torch.cuda.synchronize()
        return g

    assert 6 * 1672 ** 2 <= 2 ** 24 < 6 * 1673 ** 2
    with pytest.raises(RuntimeError, match="unsupported size"):
        cube(1673)
    assert torch.count_nonzero(cube(1672)).item() == 0
    with pytest.raises(RuntimeError, match="unsupported size"):
        flat(4096, 4097)
    with pytest.raises(RuntimeError, match="unsupported size"):
        flat(4097, 4096)
    assert torch.count_nonzero(flat(4096, 4096)).item() == 0


# ------------------------------------------------------------------------------------------ the fused shading backward
SHADE_H, SHADE_W = 45, 70
NEAR = 1e-5                 # pixel-channels whose float64 raw value is this close to 0 or 1 get d_rgb = 0: the gate jumps there


def _halve(x):
    w = x.shape[1] // 2
    return x.view(6, w, 2, w, 2, 3).mean(dim=(2, 4))


# name -> (specular widths, irradiance width): which path of the sink each gradient tensor takes
LIGHTS = {
    "table": ((128, 64, 32), 16),                # two levels through the table, one private; irradiance private
    "demoted": ((32, 16, 8), 32),                # all four are small, together over the budget: level 0 goes to the table
    "irradiance_direct": ((128, 64, 32), 64),    # the irradiance map is too wide for LDS: straight to memory
}


@functools.lru_cache(maxsize=None)
def _shade_inputs(light="table"):
    """G-buffer and light, all on the CPU.  The light is a base map of the first specular width, in [-0.9, 2.7] so that the
    clamp cuts at both ends, with box-filtered levels: the specular stack, and the irradiance map (the mean of 4^k texels,
    spread out again by 2^k)."""
    from pbr import get_brdf_lut
    widths, irr_w = LIGHTS[light]
    H, W = SHADE_H, SHADE_W
    g = torch.Generator().manual_seed(31)
    n = torch.nn.functional.normalize(torch.randn(H, W, 3, generator=g), dim=-1)
    n[:3] = 0.0                                                # background rows
    n[20:30] = torch.nn.functional.normalize(_smooth(10, W), dim=-1)
    v = torch.nn.functional.normalize(n + 0.8 * torch.randn(H, W, 3, generator=g), dim=-1)
    albedo, metal = torch.rand(H, W, 3, generator=g), torch.rand(H, W, 1, generator=g)
    rough = 0.02 + 0.98 * torch.rand(H, W, 1, generator=g)      # from below MIN_ROUGHNESS, across MAX_ROUGHNESS
    rough.view(-1)[300:310] = torch.tensor([0.0, 0.01, 0.04, 0.04, 0.4999, 0.5, 0.5001, 0.5, 1.0, 1.0])
    base = torch.rand(6, widths[0], widths[0], 3, generator=g) * 3.6 - 0.9
    spec = [base, _halve(base), _halve(_halve(base))]
    assert tuple(s.shape[1] for s in spec) == widths
    diffuse, spread = base, 1.0
    while diffuse.shape[1] > irr_w:
        diffuse, spread = _halve(diffuse), 2.0 * spread
    diffuse = ((diffuse - 0.9) * spread + 0.8).contiguous()                      # part of it below 0
    d_rgb = torch.randn(H, W, 3, generator=g)
    return types.SimpleNamespace(n=n, v=v, albedo=albedo, metal=metal, rough=rough, spec=[s.contiguous() for s in spec], diffuse=diffuse,
                                 d_rgb=d_rgb, lut=get_brdf_lut())


@functools.lru_cache(maxsize=None)
def _shade_reference(light, with_metallic):
    """float64 evaluation through the oracle's samplers -> raw, the gated d_rgb, and every expected gradient."""
    from oracle import texture_oracle as O
    I = _shade_inputs(light)
    f64 = lambda t, c: t.double().numpy().reshape(-1, c)
    nn_, vv, al, ro, me = f64(I.n, 3), f64(I.v, 3), f64(I.albedo, 3), f64(I.rough, 1), f64(I.metal, 1)
    ndv = (nn_ * vv).sum(-1, keepdims=True)
    refl_dir = 2.0 * np.clip(ndv, 0.0, None) * nn_ - vv
    lo_r, hi_r, nl = float(np.float32(0.04)), float(np.float32(0.5)), len(I.spec)
    r = ro[:, 0]
    mip = np.where(r < hi_r, (np.clip(r, lo_r, hi_r) - lo_r) / (hi_r - lo_r) * (nl - 2), (np.clip(r, hi_r, 1.0) - hi_r) / (1.0 - hi_r) + (nl - 2))
    widths = [int(s.shape[1]) for s in I.spec]
    E = O.cube_sample([I.diffuse.numpy()], nn_)
    fg = O.tex2d_clamp_sample(I.lut[0].numpy(), np.concatenate([np.clip(ndv, 1e-4, 1.0), ro], axis=1))
    L = O.cube_sample([s.numpy() for s in I.spec], refl_dir, mip)
    fgA, fgB = fg[:, 0:1], fg[:, 1:2]
    F0 = (1.0 - me) * 0.04 + al * me if with_metallic else np.full_like(al, 0.04)
    refl = F0 * fgA + fgB
    raw = E * al + L * refl
    near = (np.abs(raw) < NEAR) | (np.abs(raw - 1.0) < NEAR)
    d_rgb = np.where(near, 0.0, f64(I.d_rgb, 3))
    g = np.where((raw >= 0.0) & (raw <= 1.0), d_rgb, 0.0)
    dF0 = g * L * fgA
    d_albedo = g * E + (dF0 * me if with_metallic else 0.0)
    d_metallic = (dF0 * (al - 0.04)).sum(-1, keepdims=True)
    dd, dS, dcnt = O.cube_scatter([int(I.diffuse.shape[1])], 3, nn_, g * al)
    ds, sS, scnt = O.cube_scatter(widths, 3, refl_dir, g * refl, mip)
    shares = {"excluded": float(near.mean()), "high": float((raw > 1.0).mean()), "low": float((raw < 0.0).mean()),
              "passing": float(((raw >= 0.0) & (raw <= 1.0) & ~near).mean())}
    return types.SimpleNamespace(widths=widths, d_rgb=torch.from_numpy(d_rgb.astype(np.float32)).view(SHADE_H, SHADE_W, 3), d_albedo=d_albedo,
                                 d_metallic=d_metallic, diffuse=(dd[0], dS[0], dcnt[0]), spec=(ds, sS, scnt), shares=shares, mip=mip)


def _shade_backward_against_float64(name, with_metallic):
    from pbr import pbr_shading_fused
    I, R = _shade_inputs(name), _shade_reference(name, with_metallic)
    print("clamp shares:", R.shares)
    assert R.shares["excluded"] <= 0.01 and R.shares["high"] >= 0.10 and R.shares["passing"] >= 0.10 and R.shares["low"] >= 0.01
    irr_w = LIGHTS[name][1]
    assert tuple(R.widths) == LIGHTS[name][0] and tuple(I.diffuse.shape) == (6, irr_w, irr_w, 3)
    assert (R.mip == 0).sum() >= 3 and (R.mip == 1).sum() >= 2 and (R.mip == 2).sum() >= 2 and (I.rough < 0.04).any()
    H, W = SHADE_H, SHADE_W
    for shape in ((H, W), (H * W,)):                            # (H, W, 3): image_width = W; (n, 3): image_width = 0
        light = types.SimpleNamespace(MIN_ROUGHNESS=0.04, MAX_ROUGHNESS=0.5, diffuse=I.diffuse.cuda().requires_grad_(True),
                                      specular=[s.cuda().requires_grad_(True) for s in I.spec])
        albedo = I.albedo.view(shape + (3,)).cuda().requires_grad_(True)
        metal = I.metal.view(shape + (1,)).cuda().requires_grad_(True) if with_metallic else None
        pkg = pbr_shading_fused(light, I.n.view(shape + (3,)).cuda(), I.v.view(shape + (3,)).cuda(), albedo, I.rough.view(shape + (1,)).cuda(),
                                metallic=metal, brdf_lut=I.lut.cuda())
        wrt = [albedo, light.diffuse] + light.specular + ([metal] if with_metallic else [])
        grads = torch.autograd.grad(pkg["render_rgb"], wrt, R.d_rgb.view(shape + (3,)).cuda())
        tag = f"shade {name} metallic={with_metallic} image_width={W if len(shape) == 2 else 0}"
        err = np.abs(grads[0].cpu().double().numpy().reshape(-1, 3) - R.d_albedo).max()
        print(f"{tag}: d_albedo max err {err:.3e} of {np.abs(R.d_albedo).max():.3e}")
        assert err < 1e-4 * max(1.0, np.abs(R.d_albedo).max())
        if with_metallic:
            err = np.abs(grads[-1].cpu().double().numpy().reshape(-1, 1) - R.d_metallic).max()
            print(f"{tag}: d_metallic max err {err:.3e} of {np.abs(R.d_metallic).max():.3e}")
            assert err < 1e-4 * max(1.0, np.abs(R.d_metallic).max())
        # the reflection vector is itself formed in fp32: 4 w_level in place of w_level
        worst = _check(f"{tag} d_diffuse", grads[1].cpu().numpy(), *R.diffuse, 4 * irr_w)
        for l, w in enumerate(R.widths):
            worst = max(worst, _check(f"{tag} d_specular[L{l}]", grads[2 + l].cpu().numpy(), R.spec[0][l], R.spec[1][l], R.spec[2][l], 4 * w))
        assert worst <= 1.0, f"{tag}: err / bound = {worst}"


@pytest.mark.parametrize("with_metallic", [True, False])
def test_fused_shading_backward_against_float64(with_metallic):
    """specular (128, 64, 32) with a 16^2 irradiance map: two levels through the table, the rest private."""
    _shade_backward_against_float64("table", with_metallic)


@pytest.mark.parametrize("with_metallic", [True, False])
def test_fused_shading_backward_demotes_the_widest_level(with_metallic):
    """specular (32, 16, 8) with a 32^2 irradiance map, C = 3: all four are small enough for a private copy, 6 (1024 + 256 +
    64 + 1024) 3 floats = 170496 B, table 32768 B, together 203264 B > 159 KiB = 162816 B.  The widest private slot goes to
    the table: level 0 and the irradiance map tie at 32 and the level comes first, which leaves 129536 B.  The call must
    succeed, with level 0 through the table and the other three private."""
    assert _lds_bytes((32, 16, 8, 32), 3) == (170496, 32768) and 170496 + 32768 == 203264 > LDS_BUDGET == 162816
    assert 203264 - 6 * 32 * 32 * 3 * 4 == 129536 <= LDS_BUDGET                   # one demotion suffices
    _shade_backward_against_float64("demoted", with_metallic)


@pytest.mark.parametrize("with_metallic", [True, False])
def test_fused_shading_backward_irradiance_straight_to_memory(with_metallic):
    """a 64^2 irradiance map gets no private copy and is not a level of the stack: its adds skip the table."""
    assert LIGHTS["irradiance_direct"][1] > LDS_MAX_WIDTH
    _shade_backward_against_float64("irradiance_direct", with_metallic)
