"""The colour blend's switch (lsnSetColorBlend, $LSN_COLOR_BLEND) through the host exports: generateMeshFromDepthMaps with and without
bcolor_transfer and the overlay-merge opt-in, lsnCorrectAndGenerateMesh, and the calls sharded over the one GPU listed three times.
Switched on, each equals the device-resident chain (run_mesh, color_transfer, color_blend, overlay_merge) byte for byte, and that chain
the definition (tests/color_blend_ref.py).  Switched off, the bytes are the parent's: the reference's own, from
tests/golden/export_ref.npz through tests/test_export_pin_gpu.py's helpers -- never a second run of the code under test."""
import hashlib

import numpy as np
import pytest

from livescan3d_amd import native
from tests import color_blend_ref as ref, color_cases, color_ref, support
from tests import test_export_pin_gpu as pin

pytestmark = pytest.mark.gpu

SETTING = (20, 5)
RIG_ARGS = dict(n=3, sizes=[(256, 212)] * 3, of=8)      # large enough for the colour transfer to choose pairs


def _rig():
    return color_cases.ring(**RIG_ARGS)


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).view(np.uint8).tobytes())
    return h.hexdigest()


def _chain(rig, ct, merge, setting=SETTING, radial=False):
    """The device-resident chain on one tick: (vertices, triangles)."""
    from livescan3d_amd.fusion import DeviceFusion
    with DeviceFusion.from_rigs([rig]) as fus:
        if radial:
            fus.radial_correct()
        fus.run_mesh()
        if ct:
            fus.color_transfer()
        fus.color_blend(*setting)
        if merge:
            fus.overlay_merge()
        return fus.tick_cloud(0)[0], fus.tick_triangles(0)


@pytest.mark.parametrize("ct", (False, True))
@pytest.mark.parametrize("merge", (False, True))
def test_merge_export_equals_the_device_chain(gpu, orc, ct, merge):
    rig = _rig()
    v, t, err = support.export(rig, color_transfer=ct, generate_triangles=True, overlay_merge=merge, color_blend=SETTING)
    cv, ctri = _chain(rig, ct, merge)
    assert v.tobytes() == cv.tobytes() and t.tobytes() == ctri.tobytes(), (ct, merge)
    moved, transfer = color_ref.color_transfer(rig, orc)
    assert transfer["pairs"]
    want, diag = ref.blend(rig, orc, *SETTING, verts=moved if ct else None)
    assert v.tobytes() == want.tobytes() and diag["blended"].sum() > 100      # the chain is the definition's, and the blend did something
    plain, pt, plain_err = support.export(rig, color_transfer=ct, generate_triangles=True, overlay_merge=merge)
    # the error channel is the unblended call's: empty with the merge on, else the notice that goes with the unmerged mesh and nothing more
    assert err == plain_err and (err == "" if merge else "returned the cropped vertices of all sensors" in err), (err, plain_err)
    assert plain.tobytes() != v.tobytes() and pt.tobytes() == t.tobytes()      # the switch went back: the next call is unblended
    assert native.set_color_blend(0, 0) == (0, 0)


def test_33_sensors_fail_the_host_call_with_a_message(gpu):
    """With the switch on a call of more than 32 sensors fails as a whole -- an empty mesh and the message that names the limit -- for both
    exports; the same call with the switch off returns all 33 sensors, and so does the next one."""
    from tests import color_blend_cases
    rig = color_blend_cases.rig33()
    plain, _, e0 = support.export(rig)
    assert e0 == "" and len(plain) == 33 * 16
    with pytest.raises(native.NativeUtilsError, match=r"lsnFusionColorBlend: at most 32 sensors \(the plan has 33\)"):
        support.export(rig, color_blend=SETTING)
    with pytest.raises(native.NativeUtilsError, match=r"at most 32 sensors \(the plan has 33\)"):
        native.correct_and_generate_mesh(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds, color_blend=SETTING)
    again, _, e1 = support.export(rig)
    assert e1 == "" and again.tobytes() == plain.tobytes() and native.set_color_blend(0, 0) == (0, 0)


def test_single_sensor_export_never_blends(gpu):
    rig = _rig()
    prev = native.set_color_blend(*SETTING)
    try:
        for i in range(rig.n):
            one = native.generate_vertices_from_depth_map(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds, i)
            native.set_color_blend(0, 0)
            off = native.generate_vertices_from_depth_map(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds, i)
            native.set_color_blend(*SETTING)
            assert one.tobytes() == off.tobytes() and len(one) > 0, i
    finally:
        native.set_color_blend(*prev)


def test_correct_and_generate_equals_the_device_chain(gpu):
    rig = _rig()
    v, t, d, c = native.correct_and_generate_mesh(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds,
                                                  color_blend=SETTING)
    cv, ctri = _chain(rig, False, False, radial=True)
    assert v.tobytes() == cv.tobytes() and t.tobytes() == ctri.tobytes()
    v0, t0, d0, c0 = native.correct_and_generate_mesh(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
    assert v0.tobytes() != v.tobytes() and t0.tobytes() == t.tobytes() and d0.tobytes() == d.tobytes() and c0.tobytes() == c.tobytes()


OFF_MESH = [n for n in pin.CASES if pin.KIND[n] == "mesh" and n != "d_n0"]
OFF_RADIAL = [n for n in pin.CASES if pin.KIND[n] == "radial_mesh"]


@pytest.mark.parametrize("setting", ((0, 5), (-3, 0), (20, 21)))
def test_switched_off_the_bytes_are_the_references(gpu, setting):
    """Every small fixture of tests/golden/export_ref.npz with more than one sensor, every flag pair, with the switch set to a pair that
    means off."""
    assert OFF_MESH and OFF_RADIAL
    prev, prev_merge = native.set_color_blend(*setting), native.set_overlay_merge(True)
    try:
        seen = 0
        for name in OFF_MESH + OFF_RADIAL:
            rig, kind, flags, want, counts = pin.case(name)
            if rig.n < 2:
                continue
            seen += 1
            if kind == "radial_mesh":
                v, t, d, c = native.correct_and_generate_mesh(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
                pin.same(name, "v0", v, want)
                pin.same(name, "t0", t, want)
                continue
            for ct, tri in flags:
                v, t = native.generate_mesh_from_depth_maps(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds,
                                                            color_transfer=bool(ct), generate_triangles=bool(tri))
                pin.same(name, f"v{ct}", v, want)
                pin.same(name, f"t{tri}", t, want)
        assert seen >= 5, seen
    finally:
        native.set_overlay_merge(prev_merge)
        native.set_color_blend(*prev)


CHILD = """
import sys, hashlib, numpy as np
from livescan3d_amd import native
from tests import color_cases
from tests.test_color_blend_flows_gpu import RIG_ARGS, _sha
rig = color_cases.ring(**RIG_ARGS)
out = []
for ct in (False, True):
    v, t = native.generate_mesh_from_depth_maps(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds,
                                                color_transfer=ct, generate_triangles=True)
    out.append(_sha(v, t))
v, t, _, _ = native.correct_and_generate_mesh(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
out.append(_sha(v, t))
prev = native.set_color_blend(0, 0)
print(prev[0], prev[1], *out)
"""


def _chains(rig, setting):
    return [_sha(*_chain(rig, False, False, setting)), _sha(*_chain(rig, True, False, setting)), _sha(*_chain(rig, False, False, setting, radial=True))]


def test_environment_variable_and_sharded_calls(gpu):
    """A child process with LSN_COLOR_BLEND=20,5 and LSN_HOST_DEVICES=0,0,0: the switch starts at the variable's pair, and the calls --
    which the context would cut over three devices -- run whole on the first one and equal the device chain."""
    line, _ = support.child(CHILD, {"LSN_COLOR_BLEND": " 20 , 5", "LSN_HOST_DEVICES": "0,0,0"})
    got = line.split()
    assert got[:2] == ["20", "5"], line
    assert got[2:] == _chains(_rig(), SETTING)


def test_malformed_environment_variable_means_off(gpu):
    line, err = support.child(CHILD, {"LSN_COLOR_BLEND": "20;5"}, drop=("LSN_HOST_DEVICES",))
    got = line.split()
    assert got[:2] == ["0", "0"] and "LSN_COLOR_BLEND" in err and "stays off" in err, (line, err[-300:])
    assert got[2:] == _chains(_rig(), (0, 0))
