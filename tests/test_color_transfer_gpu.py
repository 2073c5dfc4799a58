"""generateMeshFromDepthMaps(bcolor_transfer = true) and lsnFusionColorTransfer on the GPU against the CPU reference (tests/color_ref.py).

Bar: bit-exact -- the merged vertex bytes equal the reference's; XYZ, nVertices and the triangles are byte-identical to the call with the
flag false; the confidence maps, the coverage table and the chosen pairs of the diagnostics equal the reference's."""
import numpy as np
import pytest

from livescan3d_amd import native, synth
from tests import color_cases, color_ref
from tests.support import CUT_BOUNDS, export

pytestmark = pytest.mark.gpu


def _xyz(v):
    return np.stack([v["X"], v["Y"], v["Z"]]).tobytes()


def _check_export(rig, orc, expect_change):
    plain, t0, e0 = export(rig)
    got, t1, e1 = export(rig, color_transfer=True)
    want, diag = color_ref.color_transfer(rig, orc)
    assert e0 == "" and e1 == "", (e0, e1)
    assert len(got) == len(plain) == len(want)
    assert _xyz(got) == _xyz(plain) and np.array_equal(got["A"], plain["A"])
    assert t1.tobytes() == t0.tobytes()
    assert got.tobytes() == want.tobytes(), f"colours differ at {np.flatnonzero(got.view('u1').reshape(-1, 16)[:, :3].any(1) != 0)[:5]}"
    changed = got.tobytes() != plain.tobytes()
    assert expect_change is None or changed == expect_change, (changed, diag["pairs"])
    return got, t1, diag


def test_ring_scene_is_corrected(gpu, orc):
    """Fails without the feature: the flag used to be ignored (uncorrected colours, an error message)."""
    rig = color_cases.ring(8)
    got, tris, diag = _check_export(rig, orc, True)
    assert len(diag["pairs"]) == 7
    assert native.last_mesh_ply() == orc.ply_binary(got, tris)   # lsnLastMesh* serves the corrected mesh


def test_ragged_sizes(gpu, orc):
    rig = color_cases.ring(4, sizes=[(512, 424), (320, 240), (640, 480), (256, 212)], of=8)
    _check_export(rig, orc, True)


def test_one_sensor_unchanged(gpu, orc):
    _check_export(color_cases.ring(1, of=8), orc, False)


def test_no_overlap_unchanged(gpu, orc):
    _, _, diag = _check_export(color_cases.no_overlap(), orc, False)
    assert diag["coverage"].max() <= color_ref.COVERAGE_THRESHOLD


def test_disjoint_pairs_second_branch(gpu, orc):
    _, _, diag = _check_export(color_cases.disjoint_pairs(), orc, True)
    assert diag["pairs"] == [(0, 1), (2, 3)] or diag["pairs"] == [(2, 3), (0, 1)]
    assert diag["coverage"][0, 2] == diag["coverage"][1, 3] == diag["coverage"][0, 3] == diag["coverage"][1, 2] == 0


def test_crop_through_the_overlap(gpu, orc):
    """The crop box removes vertices whose pixels still have depth: samples there are skipped."""
    rig = color_cases.ring(8, bounds=CUT_BOUNDS)
    _check_export(rig, orc, True)
    # the case is real: some sample pixel of a chosen pair has depth but no vertex
    s = [color_ref.Sensor(*_frame(rig, k), rig.intr[7 * k:7 * k + 7], rig.wt[12 * k:12 * k + 12], rig.bounds, orc) for k in range(rig.n)]
    _, diag = color_ref.color_transfer(rig, orc)
    skipped = 0
    for i, j in diag["pairs"]:
        ok, q = color_ref._tests(s[i], s[j], False)
        skipped += int((ok & (s[i].p2v[q] < 0)).sum())
    assert skipped > 0


def _frame(rig, k):
    sizes = (rig.widths.astype(np.int64) * rig.heights).tolist()
    a = int(sum(sizes[:k]))
    w, h = int(rig.widths[k]), int(rig.heights[k])
    return rig.depth_maps.view("<u2")[a:a + w * h].reshape(h, w), rig.depth_colors[3 * a:3 * (a + w * h)].reshape(h, w, 3)


def test_constant_colour_sensor_goes_to_zero(gpu, orc):
    """Scale ~ 1e15 on the constant sensor: its other colours leave the int range; x64 gives INT_MIN -> 0 (saturation would give 255)."""
    rig = color_cases.constant_colour(color_ref)
    got, _, diag = _check_export(rig, orc, True)
    assert np.abs(diag["transforms"][:, 6:]).max() > 1e12
    off = np.concatenate([[0], np.cumsum([len(orc.create_vertices(*_frame(rig, k), rig.intr[7 * k:7 * k + 7], rig.wt[12 * k:12 * k + 12],
                                                                         rig.bounds)) for k in range(rig.n)])])
    seg = got[off[2]:off[3]]
    assert (seg["R"] == 0).sum() > 100


def test_tiny_and_odd_frames(gpu, orc):
    for sizes in ([(1, 1), (37, 29), (511, 423), (333, 211)], [(511, 423), (509, 421), (1, 1)], [(1, 1)] * 3):
        _check_export(color_cases.ring(len(sizes), sizes=sizes, of=8), orc, None)


def _device_run(rigs):
    """run_mesh over a batch of ticks, then the colour transfer; synchronised."""
    import torch
    from livescan3d_amd.fusion import DeviceFusion
    fus = DeviceFusion.from_rigs(rigs)
    fus.run_mesh()
    fus.color_transfer()
    torch.cuda.synchronize()
    return fus


def test_diagnostics_match_reference(gpu, orc):
    rig = color_cases.ring(8)
    d = _device_run([rig]).plan.color_diagnostics(0)
    _, want = color_ref.color_transfer(rig, orc)
    assert np.array_equal(d["confidence"], want["confidence"])
    assert np.array_equal(d["coverage"], want["coverage"])
    assert d["pairs"] == want["pairs"]
    assert d["transforms"].tobytes() == want["transforms"].tobytes()


def test_confidence_shift_x_frames(gpu):
    """The reference's wall test probes (x + shift_x, y + shift_x): frame B's diagonal step seeds nothing, as in the reference."""
    a, b = color_cases.shift_x_frames()
    intr = np.concatenate([synth.kinect_intrinsics(64, 48)] * 2)
    wt = np.concatenate([synth.pack_pose(*synth.ring_pose(0, 8))] * 2)
    rig = synth.Rig([a, b], [np.zeros((48, 64, 3), np.uint8)] * 2, intr, wt, synth.DEFAULT_BOUNDS)
    conf = _device_run([rig]).plan.color_diagnostics(0)["confidence"]
    assert np.array_equal(conf[:64 * 48].reshape(48, 64), color_ref.confidence_map(a))
    assert np.array_equal(conf[64 * 48:].reshape(48, 64), color_ref.confidence_map(b))


def test_device_batch_equals_export_calls(gpu):
    """lsnFusionColorTransfer over a 16-tick batch: every tick equals its own export call."""
    T = 16
    rigs = [color_cases.ring(8, tick=k, seed=1 + k % 3, sizes=[(256, 212)] * 8) for k in range(T)]
    for r in rigs[1:]:   # the export calls below: with the plan's calibration (rigs[0]'s)
        r.intr, r.wt, r.bounds = rigs[0].intr, rigs[0].wt, rigs[0].bounds
    with _device_run(rigs) as fus:
        off = fus.host_offsets()
        for k in range(T):
            want, _, err = export(rigs[k], color_transfer=True)
            nv = int(off[k, -1])
            assert err == "" and nv == len(want)
            assert fus.tick_bytes(k).tobytes() == want.tobytes(), k


def test_overlay_merge_flag_still_reports(gpu, orc):
    """bgenerate_triangles = true: the message stays as it was; the colour transfer is applied when its own flag is set."""
    rig = color_cases.ring(4, sizes=[(256, 212)] * 4, of=8)
    v0, t0, e0 = export(rig, generate_triangles=True)
    assert "overlay merge are outside this library's scope" in e0
    v1, t1, e1 = export(rig, color_transfer=True, generate_triangles=True)
    assert e1 == e0
    want, diag = color_ref.color_transfer(rig, orc)
    assert diag["pairs"] and v1.tobytes() == want.tobytes() and t1.tobytes() == t0.tobytes()
