"""The GPU against the reference's OWN exports: every case of tests/golden/export_ref.npz and tests/golden/export_ref_digests.json
(tests/golden/make_export_golden.py; tests/test_export_pin.py holds the oracle to the same files) matched bit for bit by

  * the host exports: generateMeshFromDepthMaps with every flag pair of the case (the overlay merge switched on, the switch restored),
    generateVerticesFromDepthMap for every index, depthMapAndColorSetRadialCorrection, lsnCorrectAndGenerateMesh;
  * the device-resident FusionPlan: a one-tick plan (run: the single pass) and a plan of two ticks (run, run_mesh: the count -> scan ->
    write kernels), then color_transfer / overlay_merge in the reference's order; radial_correct and radial_correct_to;
    the 16 rigs of the tick sequence stacked as the ticks of ONE plan;
  * TickPipeline.run (lsnTickRun) for the radial -> mesh cases;
  * the host exports again in a child run with LSN_HOST_DEVICES=0,0,0 (the call sharded over three "devices").
No reference checkout is read here."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from livescan3d_amd import native
from tests import export_cases

pytestmark = pytest.mark.gpu

_Z = np.load(os.path.join(export_cases.GOLDEN, "export_ref.npz"))
CASES = [str(c) for c in _Z["cases"]]
KIND = {c: str(_Z[c + "/kind"]) for c in CASES}
DIG = json.load(open(os.path.join(export_cases.GOLDEN, "export_ref_digests.json")))
SEQ = sorted(n for n in DIG if n.startswith("L_seq_"))
sha = export_cases.sha


@functools.lru_cache(maxsize=None)
def _large():
    return {name: rig for name, _, rig, _ in export_cases.large_cases()}


def case(name):
    """(rig, kind, flags, want) with want[key] = bytes (fixtures) or sha256 hex (digests) of the reference's outputs."""
    if name in DIG:
        e = DIG[name]
        rig = _large()[name]
        assert sha(export_cases.rig_inputs(rig)) == e["inputs"], name
        want = {k: e[k] for k in ("radial_depth", "radial_colors", "v0", "v1", "t0", "t1") if k in e}
        return rig, e["kind"], [tuple(f) for f in e["flags"]], want, e.get("counts")
    p = name + "/"
    want = {k: _Z[p + k].tobytes() for k in ("radial_depth", "radial_colors", "v0", "v1", "t0", "t1") if p + k in _Z.files}
    counts = _Z[p + "counts"].tolist() if p + "counts" in _Z.files else None
    return export_cases.fixture_rig(_Z, name), KIND[name], [tuple(f) for f in _Z[p + "flags"].tolist()], want, counts


def same(name, key, got, want):
    b = np.ascontiguousarray(got).view(np.uint8).tobytes()
    ok = (sha(np.frombuffer(b, np.uint8)) == want[key]) if isinstance(want[key], str) else b == want[key]
    assert ok, f"{name}: {key} differs from the reference's"


ALL = CASES + sorted(DIG)
MESH = [n for n in ALL if (KIND.get(n) or DIG[n]["kind"]) == "mesh"]
RADIAL = [n for n in ALL if (KIND.get(n) or DIG[n]["kind"]) in ("radial", "radial_mesh")]
RADIAL_MESH = [n for n in ALL if (KIND.get(n) or DIG[n]["kind"]) == "radial_mesh"]


@pytest.mark.parametrize("name", MESH + RADIAL_MESH)
def test_host_exports_match_the_reference(gpu, name):
    rig, kind, flags, want, counts = case(name)
    if kind == "radial_mesh":
        d, c = native.radial_correction(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr)
        same(name, "radial_depth", d, want)
        same(name, "radial_colors", c, want)
        v, t, d1, c1 = native.correct_and_generate_mesh(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
        same(name, "v0", v, want)
        same(name, "t0", t, want)
        same(name, "radial_depth", d1, want)
        same(name, "radial_colors", c1, want)
        rig = export_cases.corrected_rig(rig, d, c)
    prev = native.set_overlay_merge(True)
    try:
        for ct, tri in flags:
            v, t = native.generate_mesh_from_depth_maps(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds,
                                                        color_transfer=bool(ct), generate_triangles=bool(tri))
            same(name, f"v{ct}", v, want)
            same(name, f"t{tri}", t, want)
    finally:
        native.set_overlay_merge(prev)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    for i in range(rig.n):
        one = native.generate_vertices_from_depth_map(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds, i)
        assert len(one) == counts[i], (name, i)
        if "v0" in want and not isinstance(want["v0"], str):
            assert one.tobytes() == want["v0"][16 * off[i]:16 * off[i + 1]], (name, i)


@pytest.mark.parametrize("name", [n for n in RADIAL if KIND.get(n, DIG.get(n, {}).get("kind")) == "radial"])
def test_host_radial_export_matches_the_reference(gpu, name):
    rig, _, _, want, _ = case(name)
    d, c = native.radial_correction(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr)
    same(name, "radial_depth", d, want)
    same(name, "radial_colors", c, want)


def _plan_mesh(rigs, ct, tri):
    """run_mesh over the stacked ticks, then colour transfer and the overlay merge in the reference's order.
    Returns per tick (vertex bytes, offsets, triangles)."""
    from livescan3d_amd.fusion import DeviceFusion
    with DeviceFusion.from_rigs(rigs) as fus:
        fus.run_mesh()
        if ct:
            fus.color_transfer()
        if tri:
            fus.overlay_merge()
        o = fus.host_offsets()
        return [(fus.tick_bytes(k), o[k], fus.tick_triangles(k)) for k in range(len(rigs))]


def _plan_run(rigs):
    """run (no triangles): the single pass for one tick, count -> scan -> write for more.  Returns per tick (vertex bytes, offsets)."""
    from livescan3d_amd.fusion import DeviceFusion
    with DeviceFusion.from_rigs(rigs) as fus:
        fus.run()
        o = fus.host_offsets()
        return [(fus.tick_bytes(k), o[k]) for k in range(len(rigs))]


def _check_counts(name, o, counts):
    assert o[0] == 0 and np.diff(o).tolist() == list(counts), (name, o.tolist(), counts)


PLAN_MESH = [n for n in MESH if n not in SEQ and n != "d_n0"]   # no plan of zero sensors


@pytest.mark.parametrize("name", PLAN_MESH)
def test_fusion_plan_matches_the_reference(gpu, name):
    rig, _, flags, want, counts = case(name)
    for T in (1, 2):
        for v, o in _plan_run([rig] * T):
            _check_counts(name, o, counts)
            same(name, "v0", v, want)
    for ct, tri in flags:
        for v, o, t in _plan_mesh([rig] * (1 if (ct or tri) else 2), ct, tri):
            _check_counts(name, o, counts)
            same(name, f"v{ct}", v, want)
            same(name, f"t{tri}", t, want)


def test_fusion_plan_tick_sequence_matches_the_reference(gpu):
    """The 16 distinct rigs of the sequence (one calibration) as the 16 ticks of one plan: each tick on its own, as 16 calls would be."""
    got = [case(n) for n in SEQ]
    assert len(got) == 16 and all(f == [(1, 1)] for _, _, f, _, _ in got)
    for n, (v, o, t), (_, _, _, want, counts) in zip(SEQ, _plan_mesh([g[0] for g in got], 1, 1), got):
        _check_counts(n, o, counts)
        same(n, "v1", v, want)
        same(n, "t1", t, want)
    for n, (v, o), (_, _, _, want, counts) in zip(SEQ, _plan_run([g[0] for g in got]), got):
        _check_counts(n, o, counts)
        assert len(v) == sum(counts)


@pytest.mark.parametrize("name", RADIAL)
def test_fusion_plan_radial_matches_the_reference(gpu, name):
    import torch
    from livescan3d_amd.fusion import DeviceFusion
    rig, _, _, want, _ = case(name)
    with DeviceFusion.from_rigs([rig]) as fus:
        d2, c2 = torch.zeros_like(fus.depth), torch.zeros_like(fus.rgb)
        fus.radial_correct_to(d2, c2)
        fus.radial_correct()
        torch.cuda.synchronize()
        for tag, d, c in (("out of place", d2, c2), ("in place", fus.depth, fus.rgb)):
            same(f"{name} {tag}", "radial_depth", d.cpu().numpy(), want)
            same(f"{name} {tag}", "radial_colors", c.cpu().numpy(), want)


@pytest.mark.parametrize("name", RADIAL_MESH)
def test_tick_pipeline_matches_the_reference(gpu, name):
    """lsnTickRun: radial correction out of place -> vertices -> triangulation, one tick and two."""
    import torch
    from livescan3d_amd.fusion import upload_rig
    rig, _, _, want, counts = case(name)
    for T in (1, 2):
        N = rig.n
        tp = native.TickPipeline(0, T, rig.widths, rig.heights)
        tp.set_params(rig.intr, rig.wt, rig.bounds)
        depth, rgb = upload_rig(rig, T)
        cd, cc = torch.zeros_like(depth), torch.zeros_like(rgb)
        v = torch.zeros((T, tp.capacity, 16), dtype=torch.uint8, device="cuda")
        o = torch.full((T, N + 1), -7, dtype=torch.int32, device="cuda")
        tr = torch.zeros((T, tp.tri_capacity, 3), dtype=torch.int32, device="cuda")
        to = torch.full((T, N + 1), -7, dtype=torch.int32, device="cuda")
        st = int(torch.cuda.current_stream().cuda_stream)
        tp.run(depth.data_ptr(), rgb.data_ptr(), cd.data_ptr(), cc.data_ptr(), v.data_ptr(), o.data_ptr(), tr.data_ptr(), to.data_ptr(), st)
        torch.cuda.synchronize()
        for k in range(T):
            ok = o[k].cpu().numpy()
            _check_counts(name, ok, counts)
            same(name, "radial_depth", cd[k].cpu().numpy(), want)
            same(name, "radial_colors", cc[k].cpu().numpy(), want)
            same(name, "v0", v[k, :ok[-1]].cpu().numpy(), want)
            same(name, "t0", tr[k, :int(to[k, -1])].cpu().numpy(), want)
        tp.close()


def test_host_exports_sharded_over_three_devices(gpu):
    """The host-export tests again in ONE child run with the calls cut over three "devices" (the one GPU listed three times): the flow
    is chosen once per process."""
    if os.environ.get("LSN_EXPORT_PIN_CHILD"):
        pytest.skip("the child run")
    env = dict(os.environ, LSN_EXPORT_PIN_CHILD="1", LSN_HOST_DEVICES="0,0,0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k", "host_", "-p",
                        "no:cacheprovider"], capture_output=True, text=True, env=env, timeout=900,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-1500:])
    n = len(MESH + RADIAL_MESH) + len([x for x in RADIAL if x not in RADIAL_MESH])
    assert f"{n} passed" in r.stdout, r.stdout[-500:]
