"""The inputs of the TSDF kernel tests, built once and shared by tests/test_tsdf_ref.py (which asserts on the CPU that they
contain what they are meant to: the censuses) and by the two GPU files.  Volumes are tests/mesh_ref.py `Volume` objects used
as plain containers (dom, coords, index, tsdf, weight, color)."""
import functools

import numpy as np

import mesh_ref as R

f32 = np.float32
VOX, TRUNC = 0.01, 0.04
L = 16 * VOX


def look_at(eye, target, roll):
    """W2C (4, 4) float32 of a camera at `eye` looking at `target`, rolled about its axis: a general rotation."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    up = np.array([0.0, -1.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    c, s = np.cos(roll), np.sin(roll)
    x, y = c * x + s * y, -s * x + c * y
    Rm = np.stack([x, y, z])
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = Rm, -Rm @ eye
    return w2c.astype(f32)


def c2w_of(w2c):
    return np.linalg.inv(np.asarray(w2c, np.float64)).astype(f32)


# ---- injected volumes (marching cubes) -------------------------------------------------------------------------------

def _to_block(dense, r):
    """the 16^3 block at block offset r of a dense [x, y, z] array, as the pool stores it (v = i + 16 j + 256 k)"""
    sl = tuple(slice(16 * int(q), 16 * int(q) + 16) for q in r)
    return dense[sl].transpose(2, 1, 0).reshape(-1)


def make_volume(dom, blocks, tsdf, weight, color, voxel=VOX):
    """dom (6,), blocks (n, 3) in slot order, dense [x, y, z] fields over the domain's voxels (color: (3, X, Y, Z))."""
    vol = R.Volume(dom, voxel, 4 * voxel, 100.0)
    blocks = np.asarray(blocks, np.int64).reshape(-1, 3)
    vol.coords = blocks
    vol.index[vol.linear(blocks)] = np.arange(len(blocks))
    rel = blocks - np.array(dom[:3])
    vol.tsdf = np.stack([_to_block(tsdf, r) for r in rel]).astype(f32)
    vol.weight = np.stack([_to_block(weight, r) for r in rel]).astype(f32)
    vol.color = np.stack([np.stack([_to_block(color[c], r) for c in range(3)]) for r in rel]).astype(f32)
    return vol


def _all_blocks(dom):
    x0, y0, z0, nx, ny, nz = dom
    return np.array([(x0 + x, y0 + y, z0 + z) for z in range(nz) for y in range(ny) for x in range(nx)], np.int64)  # linear order


def _random_field(rng, shape):
    neg = rng.random(shape) < 0.5
    mag = 1.0 - rng.random(shape)                                  # (0, 1]
    return np.where(neg, -mag, mag).astype(f32), (rng.random((3,) + tuple(shape)) * 255.0).astype(f32)


@functools.lru_cache(None)
def every_case_volume():
    """3 x 3 x 3 blocks, all present, weight 1: random signs, checkerboards forced around the 8 inner block corners (where a
    cube's edges are owned by face, edge and corner neighbours), each bent to give its corner voxel a chosen used-edge mask."""
    rng = np.random.default_rng(11)
    dom = [-1, -1, -1, 3, 3, 3]
    tsdf, color = _random_field(rng, (48, 48, 48))
    g = np.arange(48)
    par = ((g[:, None, None] + g[None, :, None] + g[None, None, :]) & 1).astype(bool)
    mag = np.abs(tsdf)
    for n, (cx, cy, cz) in enumerate([(a, b, c) for a in (16, 32) for b in (16, 32) for c in (16, 32)]):
        sl = (slice(cx - 3, cx + 3), slice(cy - 3, cy + 3), slice(cz - 3, cz + 3))
        tsdf[sl] = np.where(par[sl], -mag[sl], mag[sl])
        # the block's last voxel on all three axes owns edges ending in three different neighbour blocks: give the eight of
        # them the used-edge masks 1..7 (and 1 again), which also turns the checkerboard around them into near-checkerboards
        p = np.array([cx - 1, cy - 1, cz - 1])
        for a in range(3):
            q = tuple(p + np.eye(3, dtype=int)[a])
            differs = bool(((n % 7) + 1) >> a & 1)
            tsdf[q] = abs(tsdf[q]) * (1 if (tsdf[tuple(p)] < 0) == differs else -1)
    return make_volume(dom, _all_blocks(dom), tsdf, np.ones((48, 48, 48), f32), color)


NEIGHBOUR_DIRS = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]


@functools.lru_cache(None)
def sparse_volume():
    """4 x 4 x 4 blocks from (-2, -1, -3), about a third absent, slots in a random permutation, weight 0 on scattered voxels
    and on one whole face layer of a block."""
    rng = np.random.default_rng(23)
    dom = [-2, -1, -3, 4, 4, 4]
    blocks = _all_blocks(dom)
    present = rng.random(len(blocks)) > 1.0 / 3.0
    blocks = blocks[present]
    blocks = blocks[rng.permutation(len(blocks))]
    tsdf, color = _random_field(rng, (64, 64, 64))
    weight = np.where(rng.random((64, 64, 64)) < 0.01, 0.0, rng.integers(1, 5, (64, 64, 64))).astype(f32)
    r = blocks[5] - np.array(dom[:3])
    weight[16 * r[0], 16 * r[1]:16 * r[1] + 16, 16 * r[2]:16 * r[2] + 16] = 0.0  # the face layer i = 0 of slot 5
    return make_volume(dom, blocks, tsdf, weight, color)


SPECIALS = [0.0, -0.0, 1.0, -1.0, float(np.finfo(f32).tiny), -float(np.finfo(f32).tiny), float(np.nextafter(f32(0), f32(1))),
            -float(np.nextafter(f32(0), f32(1)))]


@functools.lru_cache(None)
def value_edges_volume():
    """5 x 1 x 1 blocks, 1 and 3 absent: block 0 a random field sprinkled with +-0, +-1, the smallest normal and denormal
    (every special next to every special along one row, scattered copies next to random values of both signs), block 2
    all positive, block 4 all negative (isolated: no valid cube reaches a neighbour, so no output from them)."""
    rng = np.random.default_rng(37)
    dom = [3, -2, 0, 5, 1, 1]
    tsdf, color = _random_field(rng, (80, 16, 16))
    where = rng.random((16, 16, 16)) < 0.08
    tsdf[:16][where] = rng.choice(np.array(SPECIALS, f32), size=int(where.sum()))
    pairs = [(a, b) for a in SPECIALS for b in SPECIALS]            # 64 ordered pairs, 8 rows of 16 voxels
    for n, (a, b) in enumerate(pairs):
        tsdf[2 * (n % 8):2 * (n % 8) + 2, 2 + n // 8, 7] = (a, b)
    tsdf[32:48] = np.abs(tsdf[32:48]) + f32(1e-3)
    tsdf[64:80] = -np.abs(tsdf[64:80]) - f32(1e-3)
    blocks = np.array([(3, -2, 0), (5, -2, 0), (7, -2, 0)], np.int64)
    return make_volume(dom, blocks, tsdf, np.ones((80, 16, 16), f32), color)


@functools.lru_cache(None)
def no_crossing_volume():
    """Two adjacent blocks, everything positive (+0.0 and a denormal among it): no vertex, no triangle."""
    rng = np.random.default_rng(41)
    dom = [0, 0, 0, 2, 1, 1]
    tsdf, color = _random_field(rng, (32, 16, 16))
    tsdf = np.abs(tsdf)
    tsdf[3, 3, 3], tsdf[15, 8, 8], tsdf[16, 8, 8] = 0.0, SPECIALS[6], -0.0
    return make_volume(dom, _all_blocks(dom), tsdf, np.ones((32, 16, 16), f32), color)


CHECKER_CENTRE_SLOT = 13


@functools.lru_cache(None)
def checkerboard_volume():
    """3 x 3 x 3 blocks, sign = parity of x + y + z everywhere: the centre block (slot 13, all 26 neighbours present) owns
    3 * 4096 = 12288 vertices and 4 * 4096 = 16384 triangles, the most a block can."""
    rng = np.random.default_rng(43)
    dom = [-1, 0, 2, 3, 3, 3]
    tsdf, color = _random_field(rng, (48, 48, 48))
    g = np.arange(48)
    par = ((g[:, None, None] + g[None, :, None] + g[None, None, :]) & 1).astype(bool)
    tsdf = np.where(par, -np.abs(tsdf), np.abs(tsdf)).astype(f32)
    return make_volume(dom, _all_blocks(dom), tsdf, np.ones((48, 48, 48), f32), color)


BIG_POOL_BLOCKS = 515
BIG_POOL_LIVE = (0, 255, 256, 511, BIG_POOL_BLOCKS - 1)


@functools.lru_cache(None)
def big_pool_volume():
    """515 blocks in a 103 x 5 x 1 domain, weight 0 everywhere but in slots 0, 255, 256, 511 and 514: the block scan runs
    three loop trips and has to carry counts over empty stretches."""
    rng = np.random.default_rng(47)
    dom = [-50, 2, -1, 103, 5, 1]
    blocks = _all_blocks(dom)
    assert len(blocks) == BIG_POOL_BLOCKS
    shape = (103 * 16, 80, 16)
    tsdf, color = _random_field(rng, shape)
    weight = np.zeros(shape, f32)
    for s in BIG_POOL_LIVE:
        r = blocks[s] - np.array(dom[:3])
        weight[16 * r[0]:16 * r[0] + 16, 16 * r[1]:16 * r[1] + 16, 16 * r[2]:16 * r[2] + 16] = 1.0
    return make_volume(dom, blocks, tsdf, weight, color)


MC_VOLUMES = {"every_case": every_case_volume, "sparse": sparse_volume, "value_edges": value_edges_volume,
              "no_crossing": no_crossing_volume, "checkerboard": checkerboard_volume, "big_pool": big_pool_volume}


def big_pool_live_volume():
    """big_pool_volume without its weight-0 blocks, the live ones in the same order.  A block of weight 0 owns no vertex and
    no triangle and invalidates every cube that reaches into it, exactly as an absent block does, so both volumes have the
    same mesh, array for array; the restatement takes 6 s on the 515 blocks and none on these 5.  tests/test_tsdf_ref.py
    checks the mesh of this volume with the invariants of the full one."""
    full = big_pool_volume()
    vol = R.Volume(full.dom, VOX, 4 * VOX, 100.0)
    live = np.array(BIG_POOL_LIVE)
    vol.coords = full.coords[live]
    vol.index[vol.linear(vol.coords)] = np.arange(len(live))
    vol.tsdf, vol.weight, vol.color = full.tsdf[live], full.weight[live], full.color[live]
    return vol


@functools.lru_cache(None)
def mc_reference(name):
    """tests/mesh_ref.py marching cubes of the named volume, computed once: (vertices, colours, triangles)."""
    return R.marching_cubes(big_pool_live_volume() if name == "big_pool" else MC_VOLUMES[name]())


# ---- points_aabb -----------------------------------------------------------------------------------------------------

def _general_depth(rng, W, H, lo=0.5, hi=3.0, holes=0.15):
    d = rng.uniform(lo, hi, (H, W)).astype(f32)
    d[rng.random((H, W)) < holes] = 0.0
    return d


def aabb_cases():
    """name -> (depth_trunc, [(depth, fx, fy, cx, cy, c2w), ...]): the views accumulate into one key array."""
    rng = np.random.default_rng(5)
    pose = c2w_of(look_at((0.3, -0.2, -0.4), (0.0, 0.1, 1.0), 0.4))
    far = c2w_of(look_at((-7.0, 3.0, 2.0), (0.0, 0.0, 0.0), -0.9))
    cases = {}
    cases["1x1"] = (5.0, [(np.array([[1.25]], f32), 3.0, 2.0, 0.3, -0.2, pose)])
    cases["61x47"] = (2.5, [(_general_depth(rng, 61, 47), 70.0, 64.0, 28.3, 25.1, pose)])  # some depths beyond depth_trunc
    cases["257x130"] = (5.0, [(_general_depth(rng, 257, 130), 240.0, 250.0, 120.5, 70.25, far)])
    bad = np.zeros((47, 61), f32)
    bad[::8] = np.nan
    bad[4::8] = 9.0
    bad[0, ::8] = -1.0
    bad[0, 4::8] = np.inf
    cases["all_invalid"] = (5.0, [(bad, 70.0, 64.0, 28.3, 25.1, pose)])
    # x is -0.0 where (u - cx) d >= 0 and +0.0 where it is < 0: the extremes are the two zeros, ordered by their keys;
    # y and z take negative values
    zeros = np.array([[-0.0, -0.0, -0.0, -0.0], [0.6, -0.8, 0.0, -3.0], [0.0, 0.0, 1.0, -5.0], [0, 0, 0, 1]], f32)
    cases["signed_zeros"] = (5.0, [(np.full((9, 13), 1.5, f32), 10.0, 10.0, 4.0, 4.0, zeros)])
    last = np.zeros((130, 257), f32)
    last[128, 256] = 2.0                                            # stride-4 pixel 2144 of 2145: thread 96 of the ninth workgroup
    cases["last_pixel"] = (5.0, [(last, 240.0, 250.0, 120.5, 70.25, far)])
    cases["two_views"] = (5.0, [cases["61x47"][1][0], (np.array([[4.0]], f32), 3.0, 2.0, 0.3, -0.2, far),
                                (_general_depth(rng, 30, 21), 33.0, 31.0, 14.2, 11.7, far)])
    return cases


def aabb_expected(depth_trunc, views):
    """fp32 min / max of mesh_ref's points over the views, (min (3,), max (3,)) or (None, None); among equal zeros the
    minimum is -0.0 and the maximum +0.0, the order of the integer keys."""
    vol = R.Volume([0, 0, 0, 1, 1, 1], VOX, TRUNC, depth_trunc)
    with np.errstate(invalid="ignore"):
        pts = [vol.points(d, fx, fy, cx, cy, c) for d, fx, fy, cx, cy, c in views]
    pts = np.concatenate([p.reshape(-1, 3) for p in pts])
    if len(pts) == 0:
        return None, None
    lo, hi = pts.min(0), pts.max(0)
    for r in range(3):
        col = pts[:, r]
        if lo[r] == 0 and np.any(np.signbit(col[col == 0])):
            lo[r] = f32(-0.0)
        if hi[r] == 0 and np.any(~np.signbit(col[col == 0])):
            hi[r] = f32(0.0)
    return lo, hi


# ---- touch -----------------------------------------------------------------------------------------------------------

MC_DOM = [-35, -35, -30, 70, 70, 61]                                # 298900 blocks: 292 chunks of 1024, the last of 916
MC_N = 70 * 70 * 61
MC_DEPTH_TRUNC = 12.0
# block offsets (from the domain's first block) the views are aimed at; a pair: the point sits 1 cm inside the second block,
# so its truncation box touches both
MC_TARGETS = [((0, 0, 0),), ((69, 69, 60),), ((63, 34, 53), (64, 34, 53)), ((3, 10, 10), (4, 10, 10))]


def mc_linear(b):
    return (b[2] * 70 + b[1]) * 70 + b[0]


@functools.lru_cache(None)
def touch_multichunk_views():
    """Five views on one pool.  Pixel (0, 0) of view k (cx = cy = 0: its ray is the camera axis) hits target k at depth 1; the
    other stride-4 pixels scatter over the whole domain (and beyond it: ignored points).  View 4 is view 0 with half its
    depths changed: part of its blocks exist already, part are new."""
    rng = np.random.default_rng(3)
    W, H = 61, 47
    views = []
    centre = (np.array(MC_DOM[:3]) + np.array(MC_DOM[3:]) / 2.0) * L
    for k, tgt in enumerate(MC_TARGETS):
        b = np.array(tgt[-1], np.float64) + np.array(MC_DOM[:3])
        T = (b + 0.5) * L
        if len(tgt) == 2:
            T[0] = b[0] * L + 0.01
        aim = centre + rng.uniform(-1.0, 1.0, 3)
        zdir = (aim - T) / np.linalg.norm(aim - T)
        w2c = look_at(T - zdir, T, rng.uniform(-1.0, 1.0))
        depth = rng.uniform(0.5, 9.0, (H, W)).astype(f32)
        depth[rng.random((H, W)) < 0.1] = 0.0
        depth[0, 0] = 1.0
        views.append((depth, 40.0 + k, 37.0 - k, 0.0, 0.0, c2w_of(w2c)))
    d = views[0][0].copy()
    d[:, 32:] = rng.uniform(0.5, 9.0, d[:, 32:].shape).astype(f32)
    views.append((d,) + views[0][1:])
    return views


@functools.lru_cache(None)
def touch_multichunk_reference():
    """mesh_ref over the five views -> per view dict(slots, n, coords, index, ignored) after that view, and the touched
    linear indices."""
    vol = R.Volume(MC_DOM, VOX, TRUNC, MC_DEPTH_TRUNC)
    out = []
    for v in touch_multichunk_views():
        before = vol.n
        slots = vol.touch(*v)
        lin = vol.linear(vol.coords[slots]) if len(slots) else np.zeros(0, np.int64)
        out.append(dict(slots=np.asarray(slots, np.int64), n=vol.n, new=vol.n - before, coords=vol.coords.copy(),
                        index=vol.index.copy(), ignored=vol.ignored, linear=np.asarray(lin, np.int64)))
    return out


def _axis_c2w(axis, t=(0.0, 0.0, 0.0)):
    """camera axis z -> world axis `axis`, x and y to the other two: with fx = fy = 1e12 every pixel's point is
    t + d e_axis up to 1e-11."""
    c = np.zeros((4, 4), f32)
    c[axis, 2], c[(axis + 1) % 3, 0], c[(axis + 2) % 3, 1] = 1.0, 1.0, 1.0
    c[:3, 3] = t
    c[3, 3] = 1.0
    return c


REJ_DOM = [0, 0, 0, 3, 3, 3]                                        # world [0, 0.48)^3


def _line_depth(values):
    d = np.zeros((1, 4 * len(values) - 3), f32)
    d[0, ::4] = np.asarray(values, f32)
    return d


def touch_rejection_cases():
    """name -> (depth_trunc, (depth, fx, fy, cx, cy, c2w), valid: the number of stride-4 pixels with a valid depth, or None)."""
    tr = f32(TRUNC)
    up, dn = (lambda x: np.nextafter(f32(x), f32(np.inf))), (lambda x: np.nextafter(f32(x), f32(-np.inf)))
    cases = {}
    for axis in range(3):
        t = [0.24, 0.24, 0.24]
        t[axis] = 0.0
        # p - trunc = 0 exactly (kept), just below (ignored: block -1); p + trunc just below 0.48 = 3 L (kept), at and above it
        vals = [tr, dn(tr), up(tr), f32(0.0399), f32(0.2), dn(dn(f32(0.48) - tr)), f32(0.48) - tr, up(f32(0.48) - tr), f32(0.45),
                f32(0.6)]
        cases[f"box_axis{axis}"] = (10.0, (_line_depth(vals), 1e12, 1e12, 0.0, 0.0, _axis_c2w(axis, t)), None)
    dt = f32(0.3)
    vals = [np.nan, np.inf, -0.2, 0.0, -0.0, dt, up(dt), dn(dt), 0.1, -np.inf]
    cases["depth_values"] = (float(dt), (_line_depth(vals), 1e12, 1e12, 0.0, 0.0, _axis_c2w(0, [0.0, 0.24, 0.24])), None)
    rng = np.random.default_rng(9)
    d = _general_depth(rng, 21, 14, 0.1, 0.4, 0.2)
    n_valid = int((d[::4, ::4] > 0).sum())
    good = c2w_of(look_at((0.2, 0.2, -0.1), (0.24, 0.24, 0.3), 0.3))
    for name, bad in (("pose_1e30", 1e30), ("pose_inf", np.inf), ("pose_nan", np.nan)):
        c = good.copy()
        c[1, 3] = bad
        cases[name] = (10.0, (d, 30.0, 28.0, 9.5, 6.5, c), n_valid)
    c = good.copy()
    c[0, 0] = np.nan
    c[2, 1] = -np.inf
    cases["pose_nan_rotation"] = (10.0, (d, 30.0, 28.0, 9.5, 6.5, c), n_valid)
    cases["pose_good"] = (10.0, (d, 30.0, 28.0, 9.5, 6.5, good), None)   # the same view with a sane pose: something is touched
    return cases


def touch_reference(dom, depth_trunc, view):
    vol = R.Volume(dom, VOX, TRUNC, depth_trunc)
    with np.errstate(invalid="ignore", over="ignore"):
        slots = vol.touch(*view)
    return vol, np.asarray(slots, np.int64)


# ---- fusion ----------------------------------------------------------------------------------------------------------

FUSION_DEPTH_TRUNC = 2.0


def _height(x, y):
    return 0.6 + 0.04 * np.sin(7.0 * x) * np.cos(5.0 * y)


def _render_depth(w2c, W, H, fx, fy, cx, cy):
    """camera-z depth of the height field z = _height(x, y) along every pixel's ray (fixed-point iteration)"""
    c2w = np.linalg.inv(np.asarray(w2c, np.float64))
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], axis=-1) @ c2w[:3, :3].T
    E = c2w[:3, 3]
    d = np.full((H, W), 0.5)
    for _ in range(40):
        p = E + d[..., None] * ray
        d = (_height(p[..., 0], p[..., 1]) - E[2]) / ray[..., 2]
    return d.astype(f32)


@functools.lru_cache(None)
def fusion_scene():
    """-> (dom, views): four views of a wavy surface near z = 0.6 under general rotations, fx != fy, cx / cy off centre, W and H
    no multiples of 4, depth with holes; view 2 has colours 0 and 255 only; view 3 is 0.1 from the surface (below 16 voxels:
    its touched blocks reach behind the camera) and sees a patch all others see; view 1 has lost its left third."""
    rng = np.random.default_rng(17)
    spec = [((-0.15, -0.10, 0.00), (0.00, 0.00, 0.6), 0.20, 61, 47, 70.0, 64.0, 28.3, 25.1),
            ((0.20, 0.05, -0.05), (0.05, 0.00, 0.6), -0.35, 61, 47, 66.0, 75.0, 33.7, 20.4),
            ((0.00, 0.25, 0.05), (-0.05, 0.05, 0.6), 0.60, 53, 59, 72.0, 69.0, 24.6, 31.2),
            ((0.10, -0.05, 0.50), (0.12, -0.03, 0.6), 1.00, 37, 29, 61.0, 67.0, 17.4, 15.8)]
    views = []
    for k, (eye, tgt, roll, W, H, fx, fy, cx, cy) in enumerate(spec):
        w2c = look_at(eye, tgt, roll)
        d = _render_depth(w2c, W, H, fx, fy, cx, cy)
        d[rng.random((H, W)) < 0.08] = 0.0
        d[H // 3:H // 3 + 5, W // 2:W // 2 + 9] = 0.0
        if k == 1:
            d[:, :W // 3] = 0.0
        if k == 0:
            d[3, 5], d[9, 2], d[20, 20] = np.nan, 5.0, -1.0          # invalid depths the gather meets
        col = rng.integers(0, 256, (H, W, 3)).astype(f32)
        if k == 2:
            col = np.where(rng.random((H, W, 3)) < 0.5, 0.0, 255.0).astype(f32)
        views.append((d, col, fx, fy, cx, cy, w2c))
    dom = [-4, -4, 1, 8, 8, 5]
    return dom, views


@functools.lru_cache(None)
def fusion_reference():
    """mesh_ref over the scene -> (vol, touched slots per view)."""
    dom, views = fusion_scene()
    vol = R.Volume(dom, VOX, TRUNC, FUSION_DEPTH_TRUNC)
    touched = []
    with np.errstate(invalid="ignore"):
        for d, col, fx, fy, cx, cy, w2c in views:
            touched.append(np.asarray(vol.integrate(d, col, fx, fy, cx, cy, w2c), np.int64))
    return vol, touched
