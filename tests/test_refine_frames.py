"""The refine path's exports that need no GPU: lsnRefineComposePoses against the restatement in tests/refine_ref.py, lsnRefineRelease in a
process that never refined, and lsnRefineFromDepthMaps on a machine without a device."""
import ctypes as C

import numpy as np
import pytest

from livescan3d_amd import native, synth
from tests import refine_ref, support


def _poses(n, seed):
    """n ICP poses (rotations by a few degrees, centimetre translations), world transforms whose R is NOT orthogonal (with an orthogonal
    R the C#'s in-place update of the rows cannot show), camera poses."""
    rng = np.random.default_rng(seed)
    Rs = np.stack([synth.rot_y(rng.uniform(-0.1, 0.1)) @ synth.rot_x(rng.uniform(-0.1, 0.1)) for _ in range(n)]).astype(np.float32)
    Ts = rng.uniform(-0.05, 0.05, size=(n, 3)).astype(np.float32)
    wR = rng.uniform(-1.5, 1.5, size=(n, 3, 3)).astype(np.float32)
    wt = rng.uniform(-2, 2, size=(n, 3)).astype(np.float32)
    cR = rng.uniform(-1.5, 1.5, size=(n, 3, 3)).astype(np.float32)
    ct = rng.uniform(-2, 2, size=(n, 3)).astype(np.float32)
    return Rs, Ts, wR, wt, cR, ct


def _same(got, want):
    return (got is None and want is None) or (got is not None and want is not None and got.tobytes() == want.tobytes())


@pytest.mark.parametrize("n", [1, 8])
@pytest.mark.parametrize("pairs", ["world+camera", "world", "camera", "none"])
def test_compose_poses_is_the_csharp_composition_bit_for_bit(n, pairs):
    Rs, Ts, wR, wt, cR, ct = _poses(n, seed=10 * n + len(pairs))
    if "world" not in pairs:
        wR = wt = None
    if "camera" not in pairs:
        cR = ct = None
    before = [None if a is None else a.copy() for a in (Rs, Ts, wR, wt, cR, ct)]
    got = native.compose_poses(Rs, Ts, wR, wt, cR, ct)
    want = refine_ref.compose_poses(Rs, Ts, wR, wt, cR, ct)
    for g, w, name in zip(got, want, ("world_R", "world_t", "camera_R", "camera_t")):
        assert _same(g, w), name
    for a, b in zip((Rs, Ts, wR, wt, cR, ct), before):      # the wrapper works on copies
        assert _same(a, b)
    if wR is not None:
        # the in-place update is what is being held: the textbook product Rs^T * R is something else on these matrices
        textbook = np.einsum("nlj,nlk->njk", Rs, wR).astype(np.float32)
        assert np.abs(got[0] - textbook).max() > 1e-3
        if cR is not None:
            assert got[2].tobytes() == got[0].tobytes()     # :407 copies :406
    elif cR is not None:
        assert got[2].tobytes() == cR.tobytes()              # no world rotation to compose: the camera rotations stay


def test_compose_poses_works_in_place_on_the_callers_arrays_and_refuses_nonsense():
    L = native.lib()
    Rs, Ts, wR, wt, cR, ct = _poses(3, seed=5)
    want = refine_ref.compose_poses(Rs, Ts, wR, wt, cR, ct)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.lsnRefineComposePoses(3, p(Rs), p(Ts), p(wR), p(wt), p(cR), p(ct)) == 0
    for g, w in zip((wR, wt, cR, ct), want):
        assert g.tobytes() == w.tobytes()
    assert L.lsnRefineComposePoses(0, p(Rs), p(Ts), p(wR), p(wt), None, None) == -1 and native.last_error()
    assert L.lsnRefineComposePoses(3, None, p(Ts), p(wR), p(wt), None, None) == -1 and native.last_error()


_RELEASE = """
from livescan3d_amd import native
L = native.lib()
print(L.lsnRefineRelease(0), L.lsnRefineRelease(-1), L.lsnRefineRelease(7), native.refine_release())
"""


def test_release_returns_zero_in_a_process_that_never_refined():
    out, _ = support.child(_RELEASE, {})
    assert out.split() == ["0", "0", "0", "0"]


@pytest.mark.skipif(native.device_count() > 0, reason="only meaningful on a machine without a GPU")
def test_refine_from_depth_maps_fails_loudly_without_gpu_and_touches_nothing():
    rig = synth.make_rig("scene", 2, 32, 24, seed=4, perturb=True)
    n = rig.n
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    outs = {"wt": np.full(12 * n, 7.5, np.float32), "cR": np.full(9 * n, 7.5, np.float32), "ct": np.full(3 * n, 7.5, np.float32),
            "Rs": np.full(9 * n, 7.5, np.float32), "Ts": np.full(3 * n, 7.5, np.float32),
            "clouds": np.full(3 * 32 * 24 * n, 7.5, np.float32), "counts": np.full(n, 75, np.int32)}
    frames = rig.depth_maps.copy(), rig.depth_colors.copy()
    for radial in (0, 1):
        rc = native.lib().lsnRefineFromDepthMaps(n, p(rig.depth_maps), p(rig.depth_colors), p(rig.widths), p(rig.heights), p(rig.intr), p(rig.wt),
                                                 *[float(x) for x in rig.bounds], radial, 2, 5, p(outs["wt"]), p(outs["cR"]), p(outs["ct"]),
                                                 p(outs["Rs"]), p(outs["Ts"]), p(outs["clouds"]), p(outs["counts"]))
        assert rc == -1 and "no HIP device" in native.last_error()
        assert all((a == (75 if a.dtype == np.int32 else 7.5)).all() for a in outs.values())
        assert np.array_equal(rig.depth_maps, frames[0]) and np.array_equal(rig.depth_colors, frames[1])
    with pytest.raises(native.NativeUtilsError, match="no HIP device"):
        native.refine_frames(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
