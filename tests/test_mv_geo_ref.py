"""The float64 arbiter of the multi-view geometric term (tests/mv_geo_ref.py) against OUTPUTS OF THE REFERENCE's own chain
(tests/golden/ref_mv_geo.npz, written by tests/golden/make_mv_geo_golden.py), and the conditions the GPU test's scenes must meet,
asserted from the float64 margins alone: every edge class is populated, and the pixels a float32 evaluation may decide
differently are at most 1 % of each scene.  CPU only."""
import os

import numpy as np
import pytest
import torch

import mv_geo_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_mv_geo.npz")
ULP_NOISE, ULP_ANGLE = 2.0 ** -18, 2.0 ** -22   # float32 spacing at the largest reprojection error of the golden (41 px) and at pi


def _golden():
    z = np.load(GOLD)
    maps = [torch.tensor(z[k]) for k in ("depth", "normal", "depth_n", "normal_n")]
    return z, maps, R.RefCam.from_numbers(z["ref_cam"]), R.RefCam.from_numbers(z["near_cam"]), float(z["occlusion"])


def test_restatement_and_op_by_op_reproduce_the_reference_chain():
    """Both restatements against the reference's own float32 run of utils/loss_utils.py:256-276 (unequal views, a background
    block of depth 0): `valid` identical; noise and angle within float32 rounding.  Measured here: float64 restatement to golden
    6.1e-6 px (noise, values up to 41 px) and 1.12e-6 rad (angle); gs2m_mvs.mv_geo_torch on the CPU to golden 3.7e-6 px and
    3.9e-7 rad.  Asserted: the measured value plus three float32 ulps of the output's scale."""
    import gs2m_mvs as MV
    z, maps, rc, nc, occ = _golden()
    assert (rc.W, rc.H, nc.W, nc.H) == (23, 17, 19, 13) and rc.Fx != nc.Fx and nc.Fx != nc.Fy and nc.Cx != 0.5 * nc.W
    noise, angle = torch.tensor(z["noise"]).double(), torch.tensor(z["angle"]).double()
    assert 0.2 < z["valid"].mean() < 0.8 and torch.isfinite(noise).all() and torch.isfinite(angle).all()
    r = R.restate(*[m.double() for m in maps], rc, nc, occ)
    assert np.array_equal(r.valid.numpy(), z["valid"])
    en, ea = float((r.noise - noise).abs().max()), float((r.angle - angle).abs().max())
    print("float64 restatement to golden:", en, ea)
    assert en <= 6.2e-6 + 3 * ULP_NOISE and ea <= 1.13e-6 + 3 * ULP_ANGLE
    n, a, v = MV.mv_geo_torch(*maps, rc.project_camera(), nc.project_camera(), occ, R.pixel_grid(rc.W, rc.H, torch.float32))
    assert np.array_equal(v.numpy(), z["valid"])
    en, ea = float((n.double() - noise).abs().max()), float((a.double() - angle).abs().max())
    print("mv_geo_torch to golden:", en, ea)
    assert en <= 6.2e-6 + 3 * ULP_NOISE and ea <= 1.13e-6 + 3 * ULP_ANGLE


def test_restatement_makes_no_float32_cast_and_differentiates_to_all_four_maps():
    r = R.reference("one_wave").f64
    assert all(t.dtype == torch.float64 for t in (r.noise, r.angle, r.q, r.zs, r.nraw, r.c))
    assert all(g is not None and g.dtype == torch.float64 and torch.isfinite(g).all() and bool((g != 0).any()) for g in r.grads)
    assert set(r.margins) >= {"qx", "qy", "Wn-qx", "Hn-qy", "Y.z-0.1", "occlusion", "clip x", "clip y", "clamp", "noise"}


@pytest.mark.parametrize("name", R.SCENES)
def test_dense_scatter_is_the_lookup_backward(name):
    """The float64 dense scatter of the per-sample contributions dL/dzs, dL/dnraw equals autograd's gradient of the border-clamped
    bilinear lookups to the neighbour's maps (to float64 rounding): footprint, clip and weights restate grid_sample's."""
    r = R.reference(name)
    auto = torch.cat([r.f64.grads[2], r.f64.grads[3]], dim=0)
    assert (r.scatter - auto).abs().max().item() <= 1e-13 * auto.abs().max().item()


def test_general_scene_populates_every_edge_class():
    """From the float64 margins only (flip-band pixels never count): at least 8 members per class, ordinary pixels >= 30 %."""
    r = R.reference("general")
    s = r.scene
    assert (s.ref.W, s.ref.H, s.near.W, s.near.H) == (67, 45, 53, 41) and (s.ref.W * s.ref.H) % 64 == 7 and (s.ref.W * s.ref.H) % 256 == 199
    assert s.near.Fx != s.ref.Fx and s.near.Fy != s.near.Fx and s.near.Cx != 0.5 * s.near.W and s.near.Cy != 0.5 * s.near.H
    counts = {k: int(v.sum()) for k, v in r.k.items() if k not in ("flip", "flip_bwd", "stiff")}
    print(counts)
    for k in ("off left", "off right", "off top", "off bottom", "last column", "last row", "behind", "occluded", "just not occluded",
              "clamp binds", "zero reference normal", "zero sampled normal"):
        assert counts[k] >= 8, (k, counts)
    depth0 = (s.depth.reshape(-1) == 0) & ~r.k["flip"]
    assert int(depth0.sum()) >= 8
    assert int((r.k["behind"] & ~depth0).sum()) >= 8, "points at or behind the near limit that are not background"
    assert counts["ordinary"] >= 0.3 * r.k["flip"].numel()
    # in the last-column / last-row band `valid` holds, the clip binds and the second column / row does not exist
    x0, y0, fx, fy, bx, by = R.footprint(r.f64.q.detach(), s.near.W, s.near.H)
    assert not bool(bx[r.k["last column"]].any()) and not bool(by[r.k["last row"]].any())
    # where the clamp binds float64 autograd gives exactly zero to both normals; at a zero-length reference normal it does NOT give
    # zero to that normal (x / (|x| + 1e-8) has the derivative 1 / 1e-8 at 0) but exactly zero to the sampled one, and vice versa
    up = (r.upstream[1] != 0)
    clamp, zr, zsn = r.k["clamp binds"], r.k["zero reference normal"], r.k["zero sampled normal"]
    # (the reference normal is itself looked up bilinearly AT the pixel centre: float64 rounding of the position leaks ~1e-16 of
    # the neighbouring pixels' gradients into the map's, hence `tiny` and not 0 for the map; the per-sample values are exact)
    gn = r.f64.grads[1].reshape(3, -1)
    tiny = 1e-12 * gn[:, ~(zr | zsn)].abs().max().item()
    assert gn[:, clamp].abs().max().item() <= tiny and bool((r.f64.dnraw[clamp] == 0).all())
    assert bool((r.f64.dnraw[zr] == 0).all()) and gn[:, zsn & ~zr].abs().max().item() <= tiny
    assert r.f64.grads[1].reshape(3, -1)[:, zr & up & ~zsn].abs().max().item() > 1e6


@pytest.mark.parametrize("name", R.SCENES)
def test_flip_band_share_is_at_most_one_percent(name):
    r = R.reference(name)
    n = r.k["flip"].numel()
    assert int(r.k["flip_bwd"].sum()) <= 0.01 * n, (name, int(r.k["flip"].sum()), int(r.k["flip_bwd"].sum()), n)
    assert bool((r.f64.valid == r.op.valid)[~r.k["flip"]].all()), "outside the band the float32 op-by-op chain decides as float64 does"
    s = r.scene
    if name == "one_wave":
        assert s.ref.W * s.ref.H < 64
    if name == "contention":
        assert (s.near.W, s.near.H) == (2, 2) and int(r.f64.valid.sum()) > 0.5 * n
    if name == "identity":
        assert torch.equal(s.ref.V, s.near.V) and r.f64.noise[r.f64.valid].max().item() < 1e-4 and int(r.f64.valid.sum()) > 0.8 * n
