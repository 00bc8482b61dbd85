"""What the four raster entry points refuse, and with which code, called directly through the C ABI with bad arguments.

Every case returns before the first HIP call, so no device is needed: the pointers are dummies that are never dereferenced and
the allocator callbacks only record that they ran (none may).  One case per argument rule of the library (csrc/raster_args.h),
per entry point that applies the rule; the hooks' rejections are pinned by tests/test_preprocess_gpu.py and
tests/test_gaussian_bwd_gpu.py."""
import os

import pytest

import gs2m_native

INVALID, ALLOC, UNSUPPORTED = -1, -3, -4


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(gs2m_native.LIB_PATH):
        gs2m_native.build()
    return gs2m_native.lib()


def _dummy(k):
    return 0x100000 + 0x1000 * k  # distinct, non-null, 16-byte aligned; never dereferenced


FWD_ORDER = ("geometry_alloc geometry_user binning_alloc binning_user image_alloc image_user P D M background width height means3D "
             "shs sh_rest colors_precomp opacities scales scale_modifier rotations cov3D_precomp features viewmatrix projmatrix cam_pos "
             "tan_fovx tan_fovy prefiltered feature_count out_color out_radii out_observe out_buffer").split()
BWD_ORDER = ("P D M R background width height means3D shs sh_rest colors_precomp scales scale_modifier rotations cov3D_precomp features "
             "viewmatrix projmatrix cam_pos tan_fovx tan_fovy radii buffer geom_buffer binning_buffer image_buffer feature_count "
             "grad_colors grad_buffer dL_dmeans2D dL_dconics dL_dopacities dL_dcolors dL_dmeans3D dL_dcov3D dL_dshs dL_dsh_rest dL_dscales "
             "dL_drots dL_dfeatures scratch_alloc scratch_user").split()
SCALARS = dict(P=100, D=3, M=16, R=0, width=64, height=48, scale_modifier=1.0, tan_fovx=0.5, tan_fovy=0.4, prefiltered=0, feature_count=9)
ABSENT = ("colors_precomp", "cov3D_precomp", "dL_dcolors", "dL_dcov3D", "geometry_user", "binning_user", "image_user", "scratch_user")


class Call:
    """A good call of one entry point (SH colours, scales + rotations, 9 features) whose arguments the cases spoil by name."""

    def __init__(self, lib, direction, split):
        self.fn = getattr(lib, f"gs2m_raster_{direction}" + ("_split_sh" if split else ""))
        self.order = [n for n in (FWD_ORDER if direction == "forward" else BWD_ORDER) if split or n not in ("sh_rest", "dL_dsh_rest")]
        self.ran = []
        self.a = {}
        for k, n in enumerate(self.order):
            if n.endswith("_alloc"):
                self.a[n] = gs2m_native.ALLOC_FN(lambda bytes_, user, n=n: self.ran.append(n))  # (returns NULL: the call ends there)
            else:
                self.a[n] = SCALARS[n] if n in SCALARS else None if n in ABSENT else _dummy(k)

    def __call__(self, **spoiled):
        assert set(spoiled) <= set(self.a), spoiled
        a = dict(self.a, **spoiled)
        null_fn = gs2m_native.ALLOC_FN()  # (ctypes passes a null callback as an instance, not as None)
        rc = self.fn(*[null_fn if a[n] is None and n.endswith("_alloc") else a[n] for n in self.order], None)
        return rc, list(self.ran)


ENTRIES = [("forward", False), ("forward", True), ("backward", False), ("backward", True)]
SPARE = _dummy(99)
WIDE = 16 * 65535 + 1

# (entry points, spoiled arguments, code).  "fwd" / "bwd": both layouts; the rules of the inputs (which colour and covariance
# source, the SH degree, the image's size) are the forward's: the backward takes the frame its forward accepted.
CASES = {
    "P=-1": ("fwd bwd", dict(P=-1), INVALID),
    "width=0": ("fwd bwd", dict(width=0), INVALID),
    "height=-3": ("fwd bwd", dict(height=-3), INVALID),
    "feature_count=11": ("fwd bwd", dict(feature_count=11), INVALID),
    "feature_count=-1": ("fwd bwd", dict(feature_count=-1), INVALID),
    "R=-1": ("bwd", dict(R=-1), INVALID),
    "SH and colours": ("fwd", dict(colors_precomp=SPARE), INVALID),
    "neither SH nor colours": ("forward", dict(shs=None), INVALID),
    "scales, rotations and covariance": ("fwd", dict(cov3D_precomp=SPARE), INVALID),
    "neither scales + rotations nor covariance": ("fwd", dict(scales=None, rotations=None), INVALID),
    "scales without rotations": ("fwd", dict(rotations=None), INVALID),
    "D=4": ("fwd", dict(D=4), INVALID),
    "D=-1": ("fwd", dict(D=-1), INVALID),
    "M=9 at D=3": ("fwd", dict(M=9), INVALID),
    "SH without cam_pos": ("fwd", dict(cam_pos=None), INVALID),
    "split SH: M=9": ("forward_split_sh backward_split_sh", dict(M=9, D=2), UNSUPPORTED),
    "split SH: rest at offset 4": ("forward_split_sh backward_split_sh", dict(sh_rest=SPARE + 4), UNSUPPORTED),
    "split SH: no rest": ("forward_split_sh backward_split_sh", dict(sh_rest=None), INVALID),
    "split SH: no DC": ("forward_split_sh backward_split_sh", dict(shs=None), INVALID),
    "split SH: dL/drest at offset 4": ("backward_split_sh", dict(dL_dsh_rest=SPARE + 4), UNSUPPORTED),
    "split SH: dL/dDC alone": ("backward_split_sh", dict(dL_dsh_rest=None), UNSUPPORTED),
    "split SH: dL/drest alone": ("backward_split_sh", dict(dL_dshs=None), UNSUPPORTED),
    "features missing": ("fwd", dict(features=None), INVALID),
    "width=16*65535+1": ("fwd", dict(width=WIDE), UNSUPPORTED),
    "height=16*65535+1": ("fwd", dict(height=WIDE), UNSUPPORTED),
    "more than 2^28 tiles": ("fwd", dict(width=WIDE - 1, height=WIDE - 1), UNSUPPORTED),
    "P=2^28": ("fwd bwd", dict(P=1 << 28), UNSUPPORTED),
    "P=2^28 and width=0": ("fwd", dict(P=1 << 28, width=0), INVALID),
    "P=2^28 and width=0 (backward)": ("bwd", dict(P=1 << 28, width=0), UNSUPPORTED),
    "colours without dL_dcolors": ("bwd", dict(colors_precomp=SPARE), INVALID),
    "covariance without dL_dcov3D": ("bwd", dict(cov3D_precomp=SPARE), INVALID),
    "no grad_buffer with features": ("bwd", dict(grad_buffer=None), INVALID),
}
for _n in ("geometry_alloc", "binning_alloc", "image_alloc", "background", "means3D", "opacities", "viewmatrix", "projmatrix", "out_color", "out_radii",
           "out_observe", "out_buffer"):
    CASES[f"null {_n}"] = ("fwd", {_n: None}, INVALID)
for _n in ("geom_buffer", "binning_buffer", "image_buffer", "scratch_alloc", "grad_colors", "radii", "dL_dmeans2D", "dL_dopacities", "dL_dmeans3D",
           "dL_dscales", "dL_drots", "dL_dfeatures"):
    CASES[f"null {_n} (backward)"] = ("bwd", {_n: None}, INVALID)


def _applies(who, direction, split):
    name = direction + ("_split_sh" if split else "")
    return any(w == name or w == {"forward": "fwd", "backward": "bwd"}[direction] for w in who.split())


@pytest.mark.parametrize("what,direction,split", [(w, d, s) for w in sorted(CASES) for d, s in ENTRIES if _applies(CASES[w][0], d, s)])
def test_rejected(lib, what, direction, split):
    _, spoiled, code = CASES[what]
    rc, ran = Call(lib, direction, split)(**spoiled)
    assert rc == code, what
    assert ran == [], f"{what}: an allocator callback ran"


@pytest.mark.parametrize("direction,split", ENTRIES)
def test_the_good_call_gets_as_far_as_its_first_allocation(lib, direction, split):
    """the unspoiled call passes every argument check: it ends at the first allocator callback, which hands out nothing"""
    rc, ran = Call(lib, direction, split)()
    assert rc == ALLOC
    assert ran == ["geometry_alloc" if direction == "forward" else "scratch_alloc"]


@pytest.mark.parametrize("split", [False, True])
def test_backward_of_no_gaussians_is_a_no_op(lib, split):
    assert Call(lib, "backward", split)(P=0, width=0, scratch_alloc=None) == (0, [])


@pytest.mark.parametrize("split", [False, True])
def test_forward_of_no_gaussians_needs_no_scene(lib, split):
    """P = 0: the per-Gaussian pointers may be null (the split layout's own two excepted); the call gets to its allocations"""
    none = dict.fromkeys(("means3D", "opacities", "scales", "rotations", "features", "viewmatrix", "projmatrix", "cam_pos", "out_radii", "out_observe"))
    if not split:
        none["shs"] = None
    rc, ran = Call(lib, "forward", split)(P=0, **none)
    assert (rc, ran) == (ALLOC, ["geometry_alloc"])
