"""A reference of the per-Gaussian forward preprocess kernel (csrc/preprocess.hip) for tests/test_preprocess_gpu.py and
tests/test_preprocess_ref.py, with no GPU code in it.

What exists is used: the per-Gaussian state (depths, means2D, conic_opacity, rgb, clamped, cov3D, radii, tiles_touched) is the C
oracle's (oracle.forward, pinned bit for bit to the reference build by tests/test_reference_gpu.py); ex, ey, tau2f are
emit_ref.cull_params; block_tt and block_hu are emit_ref.block_counts.  Added here:

  shrunk_rect   the tile rectangle the kernel emits, in float32 and in the written order of its description: the reference's radius
                rectangle intersected with the tiles the box [x - ex, x + ex] x [y - ey, y + ey] reaches;
  sh_dir        d(SH colour) / d(unit view direction) in float64, derived from the basis polynomials (a table of monomials,
                differentiated term by term), with the sum of the absolute values of its terms for the error bound;
  the families  of inputs, each a function that returns a case dict, so that the CPU test (which asserts that a family holds its
                edge cases) and the GPU test see the same arrays.

All inputs are finite and |pix| < 1e6: the float -> int conversions of the rectangle are defined here and in the kernel alike."""
import functools

import numpy as np

import emit_ref as E
import gs2m_synth as S

NUM_FEATURES = 10
F32 = np.float32

# ---- (a) the emitted rectangle ------------------------------------------------------------------------------------------------------


def _trunc_clip(v, n):
    """(int) of a finite float32 (truncation), clamped to 0 .. n"""
    return np.clip(np.trunc(v).astype(np.int64), 0, n)


def reference_rect(pix, piy, radius, tiles_x, tiles_y):
    """-> (x0, x1, y0, y1) int64: the reference's rectangle (int)((p - r) / 16) .. (int)((p + r + 16 - 1) / 16) in float32, each
    operation rounded on its own and in that order, clamped to the grid"""
    pix, piy, r = np.asarray(pix, F32), np.asarray(piy, F32), np.asarray(radius).astype(F32)
    t, one = F32(E.TILE), F32(1.0)
    x0, x1 = _trunc_clip((pix - r) / t, tiles_x), _trunc_clip((((pix + r) + t) - one) / t, tiles_x)
    y0, y1 = _trunc_clip((piy - r) / t, tiles_y), _trunc_clip((((piy + r) + t) - one) / t, tiles_y)
    return x0, x1, y0, y1


def shrunk_rect(pix, piy, ex, ey, radius, tiles_x, tiles_y, shrink):
    """-> (tiles_touched uint32[P], rect uint32[P, 2], bin uint32[P, 2]).  rect = {x0 | y0 << 16, w | h << 16} of the emitted
    rectangle, (0, 0) when it is empty; bin = the same two words as the record carries them (not zeroed when empty: a width or a
    height of 0).  radius 0 or an empty reference rectangle: nothing is emitted and nothing recorded (all zeros).
    shrink: the box ceil((p - e - 15) * 0.0625) .. floor((p + e) * 0.0625) + 1 in float32, clamped to [-1, 70000] before the
    conversion, intersected with the reference's rectangle; ex < 0 (opacity below 1/255): empty at the reference's corner."""
    pix, piy, ex, ey = (np.asarray(v, F32) for v in (pix, piy, ex, ey))
    radius = np.asarray(radius, np.int64)
    x0, x1, y0, y1 = reference_rect(pix, piy, radius, tiles_x, tiles_y)
    seen = (radius > 0) & ((x1 - x0) * (y1 - y0) != 0)
    if shrink:
        c15, s16, one = F32(15.0), F32(0.0625), F32(1.0)
        box = lambda v: np.clip(v, F32(-1.0), F32(70000.0)).astype(np.int64)
        with np.errstate(invalid="ignore", over="ignore"):
            lx, hx = np.ceil(((pix - ex) - c15) * s16), np.floor((pix + ex) * s16) + one
            ly, hy = np.ceil(((piy - ey) - c15) * s16), np.floor((piy + ey) * s16) + one
        low = ex < 0
        lx, hx, ly, hy = (np.where(low, F32(0.0), v) for v in (lx, hx, ly, hy))   # (not used below; NaN-free for the conversion)
        sx0, sx1 = np.maximum(x0, box(lx)), np.minimum(x1, box(hx))
        sy0, sy1 = np.maximum(y0, box(ly)), np.minimum(y1, box(hy))
        sx1, sy1 = np.maximum(sx1, sx0), np.maximum(sy1, sy0)
        x1, y1 = np.where(low, x0, sx1), np.where(low, y0, sy1)
        x0, y0 = np.where(low, x0, sx0), np.where(low, y0, sy0)
    w, h = x1 - x0, y1 - y0
    tt = np.where(seen, w * h, 0)
    bin_ = np.stack([x0 | (y0 << 16), w | (h << 16)], axis=1)
    bin_[~seen] = 0
    rect = bin_.copy()
    rect[tt == 0] = 0
    return tt.astype(np.uint32), rect.astype(np.uint32), bin_.astype(np.uint32)


# ---- (b) the derivative of the SH colour with respect to the direction ----------------------------------------------------------------
# The real spherical harmonics of degree 0 .. 3 in the sign convention of the colour evaluation, as polynomials in the components
# of the direction: basis function k = sum of coefficient * x^a y^b z^c.
_C0 = 0.28209479177387814
_C1 = 0.4886025119029199
_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
       -0.5900435899266435)
SH_BASIS = [
    [(_C0, (0, 0, 0))],
    [(-_C1, (0, 1, 0))], [(_C1, (0, 0, 1))], [(-_C1, (1, 0, 0))],
    [(_C2[0], (1, 1, 0))], [(_C2[1], (0, 1, 1))], [(2 * _C2[2], (0, 0, 2)), (-_C2[2], (2, 0, 0)), (-_C2[2], (0, 2, 0))],
    [(_C2[3], (1, 0, 1))], [(_C2[4], (2, 0, 0)), (-_C2[4], (0, 2, 0))],
    [(3 * _C3[0], (2, 1, 0)), (-_C3[0], (0, 3, 0))], [(_C3[1], (1, 1, 1))],
    [(4 * _C3[2], (0, 1, 2)), (-_C3[2], (2, 1, 0)), (-_C3[2], (0, 3, 0))],
    [(2 * _C3[3], (0, 0, 3)), (-3 * _C3[3], (2, 0, 1)), (-3 * _C3[3], (0, 2, 1))],
    [(4 * _C3[4], (1, 0, 2)), (-_C3[4], (3, 0, 0)), (-_C3[4], (1, 2, 0))],
    [(_C3[5], (2, 0, 1)), (-_C3[5], (0, 2, 1))],
    [(_C3[6], (3, 0, 0)), (-3 * _C3[6], (1, 2, 0))],
]


def sh_dir(D, sh, dirs):
    """sh (P, M, 3) with M >= (D + 1)^2, dirs (P, 3) unit directions -> (val[P, 9], abs[P, 9], n_terms[9]) in float64: the nine
    derivatives of the SH colour (before + 0.5 and the clamp) with respect to the direction, the polynomials extended off the
    sphere as they stand, in the layout element 3 a + c = d colour[c] / d direction[a]; with each value the sum of the absolute
    values of its terms (one term per monomial of a differentiated basis function) and the number of those terms"""
    sh, dirs = np.asarray(sh, np.float64), np.asarray(dirs, np.float64)
    P = len(dirs)
    val, ab, n = np.zeros((P, 9)), np.zeros((P, 9)), np.zeros(9, np.int64)
    for k in range((D + 1) ** 2):
        for coef, powers in SH_BASIS[k]:
            for a in range(3):
                if powers[a] == 0:
                    continue
                q = list(powers)
                q[a] -= 1
                mono = coef * powers[a] * dirs[:, 0] ** q[0] * dirs[:, 1] ** q[1] * dirs[:, 2] ** q[2]
                term = mono[:, None] * sh[:, k, :]
                val[:, 3 * a:3 * a + 3] += term
                ab[:, 3 * a:3 * a + 3] += np.abs(term)
                n[3 * a:3 * a + 3] += 1
    return val, ab, n


def unit_dirs(means3D, campos):
    """the unit view directions in float64 from the float32 inputs"""
    d = np.asarray(means3D, F32).astype(np.float64) - np.asarray(campos, F32).astype(np.float64)[None, :]
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def clamp_bits(clamped):
    """the oracle's (P, 3) clamped flags packed as the kernel packs them: bit c = channel c"""
    c = np.asarray(clamped).astype(np.uint8)
    return (c[:, 0] | (c[:, 1] << 1) | (c[:, 2] << 2)).astype(np.uint8)


# ---- (c) the case families -------------------------------------------------------------------------------------------------------------
INV255 = F32(1.0) / F32(255.0)
# the six opacities around 1/255 of tests/test_cull_cover_gpu.py
AROUND_255 = np.array([np.nextafter(INV255, F32(0)), INV255, np.nextafter(INV255, F32(1)), 0.0039, 0.004, 0.0045], F32)
SIZES = (1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 258, 259, 511, 513, 1027)
LAYOUT_SIZES = (257, 1027)
ZERO_WORDS = (0, 1, 255, 256, 257, 5000)


@functools.lru_cache(maxsize=None)
def camera(W, H):
    """the identity-pose camera (view matrix = identity: the view depth of a point is its z, exactly)"""
    cam = S.make_camera(W, H)
    return dict(W=W, H=H, tanfovx=float(cam["tanfovx"]), tanfovy=float(cam["tanfovy"]), focal=float(cam["fx"]),
                viewmatrix=cam["viewmatrix"].numpy().astype(F32).reshape(-1).copy(), projmatrix=cam["projmatrix"].numpy().astype(F32).reshape(-1).copy(),
                campos=cam["campos"].numpy().astype(F32).copy(), synth=cam)


def make_case(name, W, H, g, D=3, M=16, layout="aligned", **opt):
    """g: means3D (P, 3), scales (P, 3), rotations (P, 4), opacities (P,) or (P, 1), shs (P, >= M, 3), features (P, 10) or None.
    layout: 'aligned' | 'offset' (the SH tensor one float off a 16-byte boundary) | 'split' (DC and rest apart; M = 16).
    opt: cov3D_precomp, colors_precomp, scale_modifier, observe (False: no observe_zero array), groups (name -> index array)"""
    a = lambda v, shape: np.ascontiguousarray(np.asarray(v, F32).reshape(shape))
    P = len(g["means3D"])
    cam = camera(W, H)
    c = dict(name=name, P=P, D=D, M=M, W=W, H=H, layout=layout, cam=cam, means3D=a(g["means3D"], (P, 3)), scales=a(g["scales"], (P, 3)),
             rotations=a(g["rotations"], (P, 4)), opacities=a(g["opacities"], (P,)), shs=a(np.asarray(g["shs"])[:, :M], (P, M, 3)),
             features=None if g.get("features") is None else a(g["features"], (P, NUM_FEATURES)), cov3D_precomp=None, colors_precomp=None,
             scale_modifier=1.0, observe=True, groups={})
    c.update(opt)
    assert np.all(np.isfinite(c["means3D"])) and np.all(np.isfinite(c["scales"])) and np.all(np.isfinite(c["shs"]))
    return c


def oracle_forward(oracle, c):
    """the C oracle on a case's inputs"""
    cam = c["cam"]
    kw = dict(bg=np.zeros(3, F32), viewmatrix=cam["viewmatrix"], projmatrix=cam["projmatrix"], campos=cam["campos"], W=c["W"], H=c["H"],
              tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], sh_degree=c["D"], scale_modifier=c["scale_modifier"],
              feature_count=0 if c["features"] is None else NUM_FEATURES, features=c["features"])
    if c["colors_precomp"] is None:
        kw["shs"] = c["shs"]
    else:
        kw["colors_precomp"] = c["colors_precomp"]
    if c["cov3D_precomp"] is None:
        kw["scales"], kw["rotations"] = c["scales"], c["rotations"]
    else:
        kw["cov3D_precomp"] = c["cov3D_precomp"]
    return oracle.forward(c["means3D"], c["opacities"], **kw)


def _scene(P, W, H, seed, scale_lo=0.005, scale_hi=0.3, behind_frac=0.01):
    g = S.make_gaussians(P, camera(W, H)["synth"], seed=seed, sh_degree=3, behind_frac=behind_frac, scale_lo=scale_lo, scale_hi=scale_hi)
    return {k: v.numpy().copy() for k, v in g.items()}


def sizes_case(P, which):
    """a make_scene-like scene (1 % behind the camera, centres up to 10 % outside the image, splats of a few pixels to a few tiles)
    at every P % 4, one block, a full block and a partial one, a last wave of one lane; which: 8 | 9 (emit_ref.IMAGES)"""
    W, H = E.IMAGES[which]
    return make_case(f"sizes-{P}-w{which}", W, H, _scene(P, W, H, seed=1000 + P))


def _uniform_shs(P, seed):
    return np.random.default_rng([seed, P]).uniform(-1.0, 1.0, (P, 16, 3)).astype(F32)


def layout_cases(P):
    """-> {name: case}: the same coefficients, uniform in [-1, 1] (so that colours clamp), as one aligned tensor, one float off
    alignment (the path without LDS staging), split DC / rest, cut to M = 1, 4, 9 at their degree, and M = 16 at degrees 0 .. 2"""
    W, H = E.IMAGES[8 if P % 2 else 9]
    g = _scene(P, W, H, seed=2000 + P, behind_frac=0.0)
    g["shs"] = _uniform_shs(P, 7)
    out = {}
    for lay in ("aligned", "offset", "split"):
        out[lay] = make_case(f"sh-{lay}-{P}", W, H, g, layout=lay)
    for deg in (0, 1, 2):
        out[f"M{(deg + 1) ** 2}"] = make_case(f"sh-M{(deg + 1) ** 2}-{P}", W, H, g, D=deg, M=(deg + 1) ** 2)
        out[f"M16-D{deg}"] = make_case(f"sh-M16-D{deg}-{P}", W, H, g, D=deg)
    return out


OTHER_KINDS = ("cov3D_precomp", "colors_precomp", "both_precomp", "modifier0.5", "modifier1", "modifier2.5", "no_features", "no_observe")


def other_case(kind, oracle=None):
    """the optional inputs on one scene of 700 Gaussians.  cov3D_precomp is the oracle's own cov3D of the scene (zeros for the
    Gaussians behind the near plane, which the kernel culls before it reads them): `oracle` is needed for those kinds"""
    W, H = E.IMAGES[9]
    g = _scene(700, W, H, seed=31)
    opt = {}
    if kind in ("cov3D_precomp", "both_precomp"):
        opt["cov3D_precomp"] = np.ascontiguousarray(oracle_forward(oracle, make_case("base", W, H, g)).cov3D, dtype=F32)
    if kind in ("colors_precomp", "both_precomp"):
        opt["colors_precomp"] = np.random.default_rng(32).uniform(0.0, 1.0, (700, 3)).astype(F32)
    if kind.startswith("modifier"):
        opt["scale_modifier"] = float(kind[8:])
    if kind == "no_features":
        g["features"] = None
    if kind == "no_observe":
        opt["observe"] = False
    return make_case(f"other-{kind}", W, H, g, **opt)


def _place(cam, pix, piy, z):
    """means3D whose centre projects to pixel (pix, piy) at depth z"""
    W, H = cam["W"], cam["H"]
    return np.stack([z * cam["tanfovx"] * ((2.0 * pix + 1.0) / W - 1.0), z * cam["tanfovy"] * ((2.0 * piy + 1.0) / H - 1.0), z], axis=1)


def _round_scale(cam, mean, radius):
    """the isotropic scale whose splat at `mean` has the reference radius `radius` (an integer >= 3): the 2-D covariance of an
    isotropic Gaussian is s^2 f^2 / z^2 (I + t t^T) with t = (x / z, y / z), largest eigenvalue s^2 f^2 / z^2 (1 + |t|^2); the
    radius is ceil(3 sqrt(that)), aimed at radius - 0.5"""
    t2 = (mean[:, 0] / mean[:, 2]) ** 2 + (mean[:, 1] / mean[:, 2]) ** 2
    return (radius - 0.5) / 3.0 * mean[:, 2] / (cam["focal"] * np.sqrt(1.0 + t2))


def _plain(P, rng, mean, scale, opacity=0.8):
    """identity rotations, random SH and features around given centres and (P,) or (P, 3) scales"""
    rot = np.zeros((P, 4)); rot[:, 0] = 1.0
    sc = np.broadcast_to(np.asarray(scale, np.float64).reshape(P, -1), (P, 3))
    return dict(means3D=mean, scales=sc, rotations=rot, opacities=np.full(P, opacity), shs=np.concatenate([rng.normal(0, 1, (P, 1, 3)), 0.1 * rng.normal(0, 1, (P, 15, 3))], 1),
                features=rng.uniform(0, 1, (P, NUM_FEATURES)))


def near_plane_case():
    """view depth = z exactly (identity view matrix): 0.2f, the float below, the float above, 0.2f + 1e-4 and -1, 40 of each,
    spread over the image.  Visible: depth > 0.2f."""
    W, H = E.IMAGES[8]
    cam, rng = camera(W, H), np.random.default_rng(41)
    n2 = F32(0.2)
    depths = np.array([n2, np.nextafter(n2, F32(0)), np.nextafter(n2, F32(1)), n2 + F32(1e-4), F32(-1.0)], F32)
    z = np.repeat(depths, 40)[rng.permutation(200)].astype(np.float64)
    mean = _place(cam, rng.uniform(4, W - 4, 200), rng.uniform(4, H - 4, 200), z)
    g = _plain(200, rng, mean, np.abs(z) * rng.uniform(0.01, 0.05, 200))
    c = make_case("near-plane", W, H, g)
    assert np.array_equal(c["means3D"][:, 2], z.astype(F32))
    c["groups"] = {"front": np.nonzero(c["means3D"][:, 2] > n2)[0], "behind": np.nonzero(c["means3D"][:, 2] <= n2)[0]}
    return c


def degenerate_case():
    """the scene of tests/test_cull_cover_gpu.py (0 .. 499 thin discs seen edge-on, every third thickened: indefinite, ill-conditioned
    and merely elongated conics, the culling off for 5 .. 50 % of them; 500 .. 699
    large splats centred up to three half-widths off-screen: empty and non-empty rectangles, centres beyond 1.3 tan(fov); 700 .. 799
    just beyond the near plane; opacities around 1/255 on every fifth) followed by
      zero       40 with all scales zero, centres inside the image: the 2-D covariance is exactly zero, det == 0, no radius;
      subpixel  100 splats of a few thousandths of a pixel: mid^2 - det < 0.1, the 0.1 floor gives radius ceil(3 sqrt(mid + sqrt(0.1))) = 2;
      clamp     100 large splats with centres at 1.35 .. 2.5 tan(fov) on one axis or both: the 1.3 tan(fov) clamp of the Jacobian;
      whole      30 splats of 3 .. 10 image widths centred inside: every tile of the grid."""
    import test_cull_cover_gpu as CC
    sc = CC._scene()
    W, H = sc["W"], sc["H"]
    cam, rng = camera(W, H), np.random.default_rng(51)
    g = {k: v.numpy().astype(np.float64) for k, v in sc["g"].items()}
    g["opacities"] = g["opacities"].reshape(-1)
    g["scales"][2:500:3, 2] *= 40.0     # every third disc 50 times thinner than wide, not 2000: as they stand 62 % of the discs have the culling off
    base = len(g["means3D"])
    parts, groups, at = [], {"discs": np.arange(0, 500), "offscreen": np.arange(500, 700)}, base

    def add(name, part):
        nonlocal at
        n = len(part["means3D"])
        parts.append(part); groups[name] = np.arange(at, at + n); at += n
    z = rng.uniform(1.0, 6.0, 40)
    add("zero", _plain(40, rng, _place(cam, rng.uniform(4, W - 4, 40), rng.uniform(4, H - 4, 40), z), np.zeros(40)))
    z = rng.uniform(2.0, 8.0, 100)
    add("subpixel", _plain(100, rng, _place(cam, rng.uniform(4, W - 4, 100), rng.uniform(4, H - 4, 100), z), z[:, None] * np.exp(rng.uniform(np.log(2e-5), np.log(2e-4), (100, 3)))))
    z = rng.uniform(2.0, 8.0, 100)
    k = np.arange(100) % 3
    fx, fy = rng.uniform(1.35, 2.5, 100) * rng.choice([-1.0, 1.0], 100), rng.uniform(1.35, 2.5, 100) * rng.choice([-1.0, 1.0], 100)
    x = np.where(k != 1, fx, rng.uniform(-1, 1, 100)) * z * cam["tanfovx"]
    y = np.where(k != 0, fy, rng.uniform(-1, 1, 100)) * z * cam["tanfovy"]
    add("clamp", _plain(100, rng, np.stack([x, y, z], 1), (z * np.exp(rng.uniform(np.log(0.03), np.log(1.2), 100)))[:, None] * rng.uniform(0.7, 1.0, (100, 3))))
    z = rng.uniform(2.0, 8.0, 30)
    mean = _place(cam, rng.uniform(4, W - 4, 30), rng.uniform(4, H - 4, 30), z)
    add("whole", _plain(30, rng, mean, z / cam["focal"] * W * rng.uniform(3.0, 10.0, 30)))
    for k2 in ("means3D", "scales", "rotations", "opacities", "shs", "features"):
        g[k2] = np.concatenate([g[k2]] + [p[k2] for p in parts], 0)
    return make_case("degenerate", W, H, g, groups=groups)


def opacity_case():
    """600 splats of 3 .. 40 pixels radius centred inside the image (a non-empty reference rectangle) with the six opacities
    around 1/255 in turn: below it (two of the six) radii > 0, nothing emitted, the record still stored"""
    W, H = E.IMAGES[9]
    cam, rng = camera(W, H), np.random.default_rng(61)
    z = rng.uniform(1.0, 8.0, 600)
    mean = _place(cam, rng.uniform(2, W - 2, 600), rng.uniform(2, H - 2, 600), z)
    g = _plain(600, rng, mean, _round_scale(cam, mean, rng.integers(3, 41, 600).astype(np.float64)))
    g["opacities"] = AROUND_255[np.arange(600) % 6]
    return make_case("opacity", W, H, g, groups={"below": np.nonzero(AROUND_255[np.arange(600) % 6] < INV255)[0]})


def heavy_case():
    """Counts chosen for the heavy rule (with shrink = 0 they follow from radius and centre alone), 12 x 8 tiles:
      waves 0, 1   60 Gaussians of 3 x 2 = 6 tiles and 4 of 3 x 3 = 9 (radius 10, centres at a tile column's middle and on a row
                   boundary or at a row's middle): light sum 396 > 320, a crowded wave, the bar at 8: the four are heavy;
      waves 2, 3   1-tile Gaussians (radius 3 at a tile's middle) with three of 40 or more tiles among them (radius 50: 7 x 7; the
                   whole grid): not crowded, the bar at 40;
      wave 4       crowded as waves 0, 1 but all of 6 tiles: nobody is heavy;
      wave 5       a last partial wave of 20: 1-tile Gaussians and one that covers the grid."""
    W, H = E.IMAGES[9]
    cam, rng = camera(W, H), np.random.default_rng(71)
    P = 5 * 64 + 20
    pix, piy, rad = np.zeros(P), np.zeros(P), np.zeros(P)
    tx, ty = rng.integers(1, 10, P), rng.integers(1, 7, P)
    pix[:], piy[:], rad[:] = 16 * tx + 8, 16 * ty + 8, 3
    six = np.r_[0:128, 256:320]
    piy[six], rad[six] = 16 * ty[six], 10
    nine = np.array([5, 20, 41, 63, 64, 70, 100, 127])
    piy[nine] = 16 * ty[nine] + 8
    big = np.array([130, 150, 191, 192, 200, 255])
    pix[big], piy[big], rad[big] = 88, 56, 50
    whole = np.array([140, 210, 330])
    rad[whole] = 900
    z = rng.uniform(2.0, 6.0, P)
    mean = _place(cam, pix, piy, z)
    g = _plain(P, rng, mean, _round_scale(cam, mean, rad))
    return make_case("heavy", W, H, g, groups={"six": six, "nine": nine, "big": big, "whole": whole})


def zero_case(P):
    W, H = E.IMAGES[8]
    return make_case(f"zero-{P}", W, H, _scene(P, W, H, seed=81))


def rejected_calls():
    """-> [(name, what to change in the arguments of a good call)]: every case the hook has to refuse"""
    return ["P=0", "P=-1", "P=2^28", "null:means3D", "null:opacities", "null:viewmatrix", "null:projmatrix", "null:radii", "null:rec", "null:tiles_touched",
            "null:rect", "null:block_tt", "null:block_hu", "null:depth_key", "null:clamped", "null:sh_dir", "null:cam_pos", "null:shs", "null:scales", "null:rotations",
            "misaligned:rec", "misaligned:sh_dir", "misaligned:rect", "misaligned:rotations", "rest:M=9", "rest:misaligned"]
