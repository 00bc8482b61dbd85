"""The promise of the culling through the real forward: the shrunk tile rectangle (preprocess.hip), the quadrant masks
(gs2m_reaches_quads) and the image-edge masks (expand_instance) together never drop a pixel the blend kernel would accept.

A scene of thin discs seen edge-on at every angle about the view axis, large splats centred off-screen, opacities at and around
1/255 and depths just beyond the near plane is rendered with the default binning and with the reference's rectangles:

  cover      every image pixel that accepts a visible Gaussian (tests/emit_ref.py: the blend kernels' float32 `power`, alpha in
             float64, from the record's own conic, centre and opacity) and lies in a tile of the reference's rectangle finds that
             Gaussian in its tile's list with the bit of the pixel's quadrant set.  No exception budget; pixels within 1e-5 of
             1/255 are neither required nor forbidden and number at most 0.1 % of the required ones.  (The reference's rectangle
             is cut at a radius of three standard deviations while alpha reaches 1/255 at up to 3.33: the pixels beyond belong
             to no list of the reference either -- 81 quadrant entries of this scene -- and the rectangle of the default
             binning is by construction inside the reference's.  The rectangle is computed here from `radii` and the centre and
             compared with the lists of the reference-binning run.);
  cost-free  colour, feature buffer and final transmittance are BITWISE those of the run with the reference's rectangles: both walk
             the same (depth, id) order and an entry a lane does not accept adds w = 0 through an fma;
  subset     the default run's instances per tile are a subset of the reference run's."""
import math

import numpy as np
import pytest
import torch

import emit_ref as E
import gs2m_synth as S

pytestmark = pytest.mark.gpu

W, H, FC = 184, 120, 9
TX, TY = (W + 15) // 16, (H + 15) // 16


def _quat_with_z_axis(n):
    """unit quaternions (w, x, y, z) of rotations whose third column is the unit vector n"""
    h = np.where(np.abs(n[:, :1]) < 0.9, np.array([[1.0, 0.0, 0.0]]), np.array([[0.0, 1.0, 0.0]]))
    u = np.cross(h, n); u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(n, u)
    R = np.stack([u, v, n], axis=2)
    q = np.zeros((len(n), 4))
    for k, M in enumerate(R):      # (the branch on the largest diagonal term: no division by a small number)
        t = np.trace(M)
        if t > 0:
            r = math.sqrt(1 + t); q[k] = (0.5 * r, (M[2, 1] - M[1, 2]) / (2 * r), (M[0, 2] - M[2, 0]) / (2 * r), (M[1, 0] - M[0, 1]) / (2 * r))
        else:
            a = int(np.argmax(np.diag(M))); b, c = (a + 1) % 3, (a + 2) % 3
            r = math.sqrt(1 + M[a, a] - M[b, b] - M[c, c])
            q[k, 0], q[k, 1 + a], q[k, 1 + b], q[k, 1 + c] = (M[c, b] - M[b, c]) / (2 * r), 0.5 * r, (M[b, a] + M[a, b]) / (2 * r), (M[c, a] + M[a, c]) / (2 * r)
    return q


def _scene():
    cam = S.make_camera(W, H)
    g = S.make_gaussians(1500, cam, seed=11, sh_degree=3, behind_frac=0.01)
    g = {k: v.numpy().copy() for k, v in g.items()}
    rng = np.random.default_rng(11)
    tx, ty = cam["tanfovx"], cam["tanfovy"]
    # 0 .. 499: thin discs (scales a, a, a / 2000) seen edge-on -- the normal at right angles to the ray through the centre, at any
    # angle about the view axis, half of them tipped by a fraction of a degree: lines up to several hundred pixels long and (with
    # the 0.3-pixel low-pass) half a pixel wide
    n = 500
    z = rng.uniform(1.0, 6.0, n)
    mean = np.stack([z * tx * rng.uniform(-1.0, 1.0, n), z * ty * rng.uniform(-1.0, 1.0, n), z], axis=1)
    g["means3D"][:n] = mean
    a = np.exp(rng.uniform(np.log(0.02), np.log(1.5), n)) * z
    g["scales"][:n] = np.stack([a, a, a / 2000.0], axis=1)
    th = np.where(np.arange(n) % 3 == 0, np.deg2rad(45.0 * rng.integers(0, 4, n)), rng.uniform(0, np.pi, n))
    ray = mean / np.linalg.norm(mean, axis=1, keepdims=True)
    u = np.stack([np.cos(th), np.sin(th), 0 * th], axis=1)
    nrm = u - (u * ray).sum(1, keepdims=True) * ray
    nrm += np.where(np.arange(n) % 2 == 0, 0.0, rng.normal(0, 0.005, n))[:, None] * ray
    g["rotations"][:n] = _quat_with_z_axis(nrm / np.linalg.norm(nrm, axis=1, keepdims=True))
    # 500 .. 699: large round splats centred outside the image, up to three half-widths away
    m = 200
    z = rng.uniform(2.0, 8.0, m)
    side = rng.choice([-1.0, 1.0], (2, m))
    fx, fy = rng.uniform(1.05, 3.0, m), rng.uniform(1.05, 3.0, m)
    both = rng.random(m) < 0.3
    horiz = rng.random(m) < 0.5
    x = np.where(both | horiz, side[0] * fx, rng.uniform(-1, 1, m)) * z * tx
    y = np.where(both | ~horiz, side[1] * fy, rng.uniform(-1, 1, m)) * z * ty
    g["means3D"][n:n + m] = np.stack([x, y, z], axis=1)
    g["scales"][n:n + m] = (np.exp(rng.uniform(np.log(0.3), np.log(4.0), m)) * z / 4.0)[:, None] * rng.uniform(0.7, 1.0, (m, 3))
    # 700 .. 799: just beyond the near plane (z > 0.2)
    k = 100
    z = 0.2 + np.exp(rng.uniform(np.log(1e-4), np.log(0.05), k))
    g["means3D"][700:800] = np.stack([z * tx * rng.uniform(-1, 1, k), z * ty * rng.uniform(-1, 1, k), z], axis=1)
    g["scales"][700:800] = np.exp(rng.uniform(np.log(0.0005), np.log(0.02), (k, 3)))
    # opacities at and around 1/255 on every fifth Gaussian
    inv = np.float32(1.0) / np.float32(255.0)
    around = np.array([np.nextafter(inv, np.float32(0)), inv, np.nextafter(inv, np.float32(1)), 0.0039, 0.004, 0.0045], np.float32)
    idx = np.arange(0, 1500, 5)
    g["opacities"][idx, 0] = around[rng.integers(0, len(around), len(idx))]
    g["features"][:, 0] = 1.0
    g = {k2: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for k2, v in g.items()}
    Gc, Gb = S.make_upstream_grads(H, W, seed=0)
    return dict(cam=cam, g=g, Gc=Gc, Gb=Gb, W=W, H=H, fc=FC, sh_degree=3, bg=torch.tensor((0.1, 0.2, 0.3), dtype=torch.float32))


def _render(sc, reference_binning):
    import diff_gaussian_rasterization as dgr
    import gs2m_native
    import helpers as Hh
    gs2m_native.set_reference_binning(reference_binning)
    g = {k: v.cuda() for k, v in sc["g"].items()}
    st = Hh.settings_for(sc, "cuda")
    e = torch.Tensor([])
    P = g["means3D"].shape[0]
    R, color, radii, observe, buffer, geomB, binB, imgB = dgr._C.rasterize_gaussians(
        st.bg, g["means3D"], e, g["opacities"], g["scales"], g["rotations"], 1.0, e, g["features"], st.viewmatrix,
        st.projmatrix, st.tanfovx, st.tanfovy, H, W, g["shs"], 3, st.campos, False, FC)
    torch.cuda.synchronize()
    gs2m_native.set_reference_binning(False)
    lay = gs2m_native.debug_layout(P, R, W, H)
    al = lambda t: (-t.data_ptr()) % 256
    view = lambda t, off, n, dt: t[al(t) + off: al(t) + off + n * np.dtype(dt).itemsize].cpu().numpy().view(dt)
    tiles = TX * TY
    rec = view(geomB, lay.rec, P * 32, np.float32).reshape(P, 32).copy()
    pl = view(binB, lay.point_list, R, np.uint32).copy()
    rg = view(imgB, lay.ranges, 2 * tiles, np.uint32).reshape(tiles, 2).astype(np.int64)
    present, mask = np.zeros((P, tiles), bool), np.zeros((P, tiles), np.int64)
    for t in range(tiles):
        v = pl[rg[t, 0]:rg[t, 1]]
        present[v & np.uint32(0x0FFFFFFF), t] = True
        mask[v & np.uint32(0x0FFFFFFF), t] = v >> np.uint32(28)
    return dict(R=R, color=color.cpu().numpy(), buffer=buffer.cpu().numpy(), radii=radii.cpu().numpy(), rec=rec, present=present, mask=mask,
                final_T=view(imgB, lay.final_T, W * H, np.float32).copy())


@pytest.fixture(scope="module")
def runs():
    sc = _scene()
    return _render(sc, False), _render(sc, True)


def _required(rec, vis):
    """-> (need[P, tiles, 4] bool, required pixels, ambiguous pixels): the quadrants that hold a pixel accepting the Gaussian"""
    P = len(rec)
    py, px = np.mgrid[0:H, 0:W]
    cell = ((py // 16) * TX + px // 16) * 4 + ((py % 16) // 8) * 2 + (px % 16) // 8
    need = np.zeros((P, TX * TY * 4), bool)
    n_req = n_amb = 0
    ids = np.nonzero(vis)[0]
    for lo in range(0, len(ids), 64):
        i = ids[lo:lo + 64]
        r = rec[i][:, :, None, None]
        power, alpha = E.pixel_alpha(r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4], r[:, 5], px[None].astype(np.float32), py[None].astype(np.float32))
        req, amb = E.accepts(power, alpha)
        n_req += int(req.sum()); n_amb += int(amb.sum())
        k, yy, xx = np.nonzero(req)
        need[i[k], cell[yy, xx]] = True
    return need.reshape(P, TX * TY, 4), n_req, n_amb


def _reference_rect(rec, radii):
    """-> in_rect[P, tiles] bool: the tiles of the reference's rectangle, (int)((p - r) / 16) .. (int)((p + r + 15) / 16) clamped to
    the grid, in float32 as the reference computes it"""
    r = radii.astype(np.float32)
    f = lambda v, n: np.clip(np.trunc(v).astype(np.int64), 0, n)
    x0, x1 = f((rec[:, 0] - r) / np.float32(16), TX), f((rec[:, 0] + r + np.float32(15)) / np.float32(16), TX)
    y0, y1 = f((rec[:, 1] - r) / np.float32(16), TY), f((rec[:, 1] + r + np.float32(15)) / np.float32(16), TY)
    t = np.arange(TX * TY)[None, :]
    return (t % TX >= x0[:, None]) & (t % TX < x1[:, None]) & (t // TX >= y0[:, None]) & (t // TX < y1[:, None]) & (radii > 0)[:, None]


def test_scene_holds_the_edge_cases(runs):
    d, r = runs
    vis = d["radii"] > 0
    rec = d["rec"].astype(np.float64)
    A, B, C = rec[:, 2], rec[:, 3], rec[:, 4]
    cond = np.where(vis, A * C / np.maximum(A * C - B * B, 1e-300), 0)
    assert vis.sum() > 1200
    assert ((cond > 100) & (cond < 1e4)).sum() > 50 and (cond > 1e4).sum() > 20, "thin tilted splats, culled and with the culling off"
    off_screen = vis & ((rec[:, 0] < -8) | (rec[:, 0] > W + 8) | (rec[:, 1] < -8) | (rec[:, 1] > H + 8))
    assert (off_screen & d["present"].any(1)).sum() > 50, "splats centred off-screen that reach the image"
    assert (vis[700:800]).sum() > 50, "Gaussians just beyond the near plane"
    assert (vis & (np.abs(d["rec"][:, 5] * 255.0 - 1.0) < 0.2)).sum() > 100, "opacities around 1/255"
    assert d["R"] < r["R"], "the default binning emits fewer instances"


def test_cover(runs):
    d, r = runs
    vis = d["radii"] > 0
    need, n_req, n_amb = _required(d["rec"], vis)
    in_rect = _reference_rect(d["rec"], d["radii"])
    assert np.array_equal(in_rect, r["present"]), "the reference's rectangle, from radii and the centre, is what the reference-binning run lists"
    print(f"\n[cover] {int((need & ~in_rect[:, :, None]).sum())} required quadrant entries lie beyond the reference's three-sigma rectangle")
    need &= in_rect[:, :, None]
    print(f"\n[cover] {int(vis.sum())} visible Gaussians, {n_req} accepted (Gaussian, pixel) pairs, {n_amb} ambiguous, {int(need.sum())} required quadrant entries, "
          f"{int(E.popcount4(d['mask']).sum())} set")
    assert n_req > 100000 and n_amb <= 1e-3 * n_req
    have = ((d["mask"][:, :, None] >> np.arange(4)[None, None, :]) & 1).astype(bool) & d["present"][:, :, None]
    lost = np.argwhere(need & ~have)
    assert len(lost) == 0, (f"{len(lost)} (Gaussian, tile, quadrant) entries hold an accepted pixel and are not in the lists; the first: Gaussian {lost[0][0]} "
                            f"record {d['rec'][lost[0][0], :12]} tile {lost[0][1]} quadrant {lost[0][2]}, in the tile's list: {d['present'][lost[0][0], lost[0][1]]}, "
                            f"mask {d['mask'][lost[0][0], lost[0][1]]:#x}")


def test_culling_is_free(runs):
    d, r = runs
    for k in ("color", "buffer", "final_T"):
        a, b = d[k], r[k]
        assert a.shape == b.shape
        diff = a.view(np.uint32) != b.view(np.uint32)
        assert not diff.any(), f"{k}: {int(diff.sum())} values differ bitwise from the run with the reference's rectangles, max |d| {float(np.abs(a - b).max()):.3e}"
    assert np.array_equal(d["radii"], r["radii"])


def test_instances_are_a_subset_of_the_reference_rectangles(runs):
    d, r = runs
    assert not np.any(d["present"] & ~r["present"])
    both = d["present"] & r["present"]
    assert np.array_equal(d["mask"][both], r["mask"][both]), "the quadrant test does not depend on the rectangle"
    assert r["present"].sum() == r["R"] and d["present"].sum() == d["R"], "a Gaussian appears once per tile"
