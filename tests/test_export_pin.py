"""The CPU oracle and the numpy restatements against the reference's OWN exports (no GPU).

tests/golden/export_ref.npz and tests/golden/export_ref_digests.json hold what generateMeshFromDepthMaps (every flag pair),
generateVerticesFromDepthMap (every index) and depthMapAndColorSetRadialCorrection of src/NativeUtils/depthprocessing.cpp computed,
compiled as they lie (tests/golden/make_export_golden.py), on the inputs of tests/export_cases.py.  Here:
  * the C oracle (orc.generate_mesh, generate_vertices_from_depth_map, radial_correction) equals every fixture and digest;
  * tests/color_ref.py (bcolor_transfer) and tests/merge_ref.py (bgenerate_triangles) equal the colour and merge fixtures;
  * the numpy restatements of tests/test_oracle_depth.py and tests/test_oracle_radial.py equal the small fixtures;
  * one test reruns the generator against a reference checkout when there is one (the only test that reads it).
A disagreement means the oracle is wrong -- and so is every GPU path the GPU tests hold to it."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from livescan3d_amd import synth
from tests import color_ref, export_cases, merge_ref
from tests.depth_ref import numpy_create_vertices, py_radial

GOLDEN = export_cases.GOLDEN
NPZ = os.path.join(GOLDEN, "export_ref.npz")
DIGESTS = os.path.join(GOLDEN, "export_ref_digests.json")
REFERENCE = os.environ.get("LIVESCAN3D_REFERENCE", "/root/reference")   # the checkout oracle/Makefile's REF names

_Z = np.load(NPZ)
CASES = [str(c) for c in _Z["cases"]]
KIND = {c: str(_Z[c + "/kind"]) for c in CASES}
DIG = json.load(open(DIGESTS))


def fixture_rig(name):
    return export_cases.fixture_rig(_Z, name)


def flags(name):
    return [tuple(f) for f in _Z[name + "/flags"].tolist()]


sha, rig_inputs, corrected_rig = export_cases.sha, export_cases.rig_inputs, export_cases.corrected_rig


@functools.lru_cache(maxsize=None)
def large_rigs():
    return {name: (kind, rig, fl) for name, kind, rig, fl in export_cases.large_cases()}


def oracle_outputs(rig, kind, fl, orc):
    """What the oracle and the restatements compute for a case, keyed as the fixtures are."""
    out = {}
    if kind in ("radial", "radial_mesh"):
        d, c = orc.radial_correction(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr)
        out["radial_depth"], out["radial_colors"] = d.view("<u2"), c
        rig = corrected_rig(rig, d, c)
    if kind in ("mesh", "radial_mesh"):
        v, counts, t = orc.generate_mesh(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
        out["counts"] = counts
        for ct, tri in fl:
            out[f"v{ct}"] = color_ref.color_transfer(rig, orc)[0] if ct else v
            out[f"t{tri}"] = merge_ref.overlay_merge(rig, orc)[0] if tri else t
        out["by_index"] = [orc.generate_vertices_from_depth_map(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr,
                                                                rig.wt, rig.bounds, i) for i in range(rig.n)]
    return out


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def test_fixtures_are_present_and_cover_the_edges():
    assert {KIND[c] for c in CASES} == {"mesh", "radial", "radial_mesh"}
    assert any(c.startswith("d_faces_") for c in CASES) and "d_n0" in CASES
    assert any(c + "/v1" in _Z.files for c in CASES)
    assert any(c + "/t1" in _Z.files for c in CASES)
    assert {e["kind"] for e in DIG.values()} == {"mesh", "radial", "radial_mesh"}


@pytest.mark.parametrize("name", CASES)
def test_oracle_equals_reference_fixture(orc, name):
    rig = fixture_rig(name)
    got = oracle_outputs(rig, KIND[name], flags(name), orc)
    keys = [k for k in ("radial_depth", "radial_colors", "counts", "v0", "v1", "t0", "t1") if name + "/" + k in _Z.files]
    assert keys
    for k in keys:
        want = _Z[name + "/" + k]
        assert _bytes(got[k]) == _bytes(want), (name, k)
    if "counts" in got:
        e = np.concatenate([[0], np.cumsum(_Z[name + "/counts"])]).astype(np.int64)
        v0 = _Z[name + "/v0"] if name + "/v0" in _Z.files else None
        for i, one in enumerate(got["by_index"]):
            assert len(one) == _Z[name + "/counts"][i], (name, i)
            if v0 is not None:
                assert _bytes(one) == v0[16 * e[i]:16 * e[i + 1]].tobytes(), (name, i)


def _split_frames(rig):
    dm, po = rig.depth_maps.view("<u2"), 0
    for s in range(rig.n):
        w, h = int(rig.widths[s]), int(rig.heights[s])
        yield (dm[po:po + w * h].reshape(h, w), rig.depth_colors[3 * po:3 * (po + w * h)].reshape(h, w, 3),
               rig.intr[7 * s:7 * s + 7], rig.wt[12 * s:12 * s + 12])
        po += w * h


@pytest.mark.parametrize("name", [c for c in CASES if KIND[c] == "mesh" and c + "/v0" in _Z.files and _Z[c + "/widths"].size])
def test_numpy_depth_restatement_equals_reference_fixture(name):
    rig = fixture_rig(name)
    want = _Z[name + "/v0"]
    got = np.concatenate([numpy_create_vertices(d, c, i, t, rig.bounds) for d, c, i, t in _split_frames(rig)])
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", [c for c in CASES if KIND[c] in ("radial", "radial_mesh")])
def test_python_radial_restatement_equals_reference_fixture(name):
    rig = fixture_rig(name)
    dd, cc = [], []
    for d, c, i, _ in _split_frames(rig):
        a, b = py_radial(d, c, i)
        dd.append(a.ravel())
        cc.append(b.ravel())
    assert np.concatenate(dd).tobytes() == _Z[name + "/radial_depth"].tobytes()
    assert np.concatenate(cc).tobytes() == _Z[name + "/radial_colors"].tobytes()


@pytest.mark.parametrize("name", sorted(DIG))
def test_oracle_equals_reference_digest(orc, name):
    kind, rig, fl = large_rigs()[name]
    e = DIG[name]
    assert (kind, [list(f) for f in fl]) == (e["kind"], e["flags"])
    assert sha(rig_inputs(rig)) == e["inputs"], "the case builder no longer rebuilds the inputs the digests were taken on"
    got = oracle_outputs(rig, kind, fl, orc)
    for k in ("radial_depth", "radial_colors", "v0", "v1", "t0", "t1"):
        if k in e:
            assert sha(got[k]) == e[k], (name, k)
            if "n_" + k in e:
                assert len(got[k]) == e["n_" + k], (name, k)
    if "counts" in e:
        assert [int(c) for c in got["counts"]] == e["counts"]
        assert [len(v) for v in got["by_index"]] == e["counts"]


def test_generator_reproduces_the_fixtures(tmp_path):
    """Rebuilds the reference's exports from a checkout and reruns every case: the arrays must equal the committed ones."""
    if not os.path.exists(os.path.join(REFERENCE, "src", "NativeUtils", "depthprocessing.cpp")):
        pytest.skip("no LiveScan3D checkout at $LIVESCAN3D_REFERENCE; the committed fixtures stand for it")
    gen = os.path.join(GOLDEN, "make_export_golden.py")
    subprocess.check_call([sys.executable, gen, REFERENCE, str(tmp_path)], stdout=subprocess.DEVNULL, timeout=900)
    fresh = np.load(tmp_path / "export_ref.npz")
    assert sorted(fresh.files) == sorted(_Z.files)
    for k in _Z.files:
        assert fresh[k].dtype == _Z[k].dtype and fresh[k].tobytes() == _Z[k].tobytes(), k
    assert json.load(open(tmp_path / "export_ref_digests.json")) == DIG
