"""The CPU restatement of the vertex-normals stage (tests/normals_ref.py): hand-made meshes for every rule of the definition, the known
answers and the orientation on the oracle's ring meshes, and the names the feature adds.  No GPU."""
import numpy as np
import pytest

from livescan3d_amd import native
from tests import color_cases, normals_ref
from tests.normals_cases import BELOW_4096, cases, rounding_mesh, wrap_mesh
from tests.simplify_ref import cloud

NAMES = ("lsnFusionNormals", "lsnFusionNormalsDiagnostics", "lsnPlyNormalsBytes", "lsnPlyPackNormals", "lsnLastMeshPlyNormals")
# rig -> (triangles, zero normals, vertices whose normal is not zero) of the oracle's mesh
RINGS = {"3x96x80": (16924, 1458, 9629), "4x64x48": (6174, 2115, 3969)}


def run(name):
    xyz, off, tri, toff = cases()[name]
    return normals_ref.normals(cloud(xyz), off, tri, toff)


def test_one_triangle_in_the_plane_z_0():
    o = run("one_triangle")      # (p2 - p0) x (p1 - p0) = (0, 1, 0) x (1, 0, 0) = (0, 0, -1)
    assert o["normals"].tolist() == [[0, 0, -1]] * 3 and o["sums"].tolist() == [[0, 0, -2 ** 40]] * 3
    assert (o["used"], o["skipped"], o["zero_normals"]) == (1, 0, 0)
    o = run("reversed")
    assert o["normals"].tolist() == [[0, 0, 1]] * 3 and o["sums"].tolist() == [[0, 0, 2 ** 40]] * 3


def test_skipped_and_degenerate_triangles():
    o = run("skipped_and_degenerate")
    assert (o["used"], o["skipped"]) == (5, 7)
    # the good triangle and the one just below 4096 carry sums; nothing else does
    assert np.flatnonzero(o["sums"].any(axis=1)).tolist() == [0, 1, 2, 12, 13, 14]
    assert o["sums"][12].tolist() == [0, 0, 2 ** 52 - 2 ** 28] and float(np.float32(BELOW_4096)) == 4096 - 2.0 ** -12
    assert o["zero_normals"] == 15 and o["normals"][12].tolist() == [0, 0, 1]
    assert not np.signbit(o["normals"][3:12]).any()          # (+0, +0, +0)


def test_opposite_triangles_cancel():
    o = run("cancelling_pair")
    assert o["used"] == 2 and o["zero_normals"] == 3 and not o["sums"].any() and o["normals"].tobytes() == bytes(36)


def test_sums_beyond_2_24_round_to_nearest_even():
    xyz, tri, want = rounding_mesh()
    o = normals_ref.normals(cloud(xyz), [0, len(xyz)], tri, [0, len(tri)])
    assert o["used"] == len(tri) and {h: tuple(o["sums"][h].tolist()) for h in want} == want
    sz = o["sums"][sorted(want), 2]
    assert sz.astype(np.float32).astype(np.int64).tolist() == [2 ** 25, 2 ** 25, 2 ** 25 + 8, 2 ** 25 + 4, 2 ** 54 - 2 ** 30]     # down, tie, tie, up, > 2^53: down
    assert sz[4] == 4 * (2 ** 52 - 2 ** 28) + 1 > 2 ** 53 and (sz % 2).tolist() == [1, 0, 0, 1, 1]
    # the cases tell a wrong conversion apart: with the sums rounded towards zero, or away from it, the normals are different bytes
    for which in (0, 1):
        differ = 0
        for h in sorted(want):
            f = np.array([float_neighbours(int(c))[which] for c in o["sums"][h]], np.float32)
            n = f / np.sqrt((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2])
            differ += n.tobytes() != o["normals"][h].tobytes()
        assert differ >= 2, (which, differ)


def float_neighbours(c):
    """(the float32 next to the integer c towards zero, the one away from zero); both c itself where it is a float32."""
    f = np.float32(c)
    if int(f) == c:
        return f, f
    g = np.nextafter(f, np.float32(np.inf if int(f) < c else -np.inf))
    lo, hi = (f, g) if abs(int(f)) < abs(int(g)) else (g, f)
    return lo, hi


def test_wrap_around():
    xyz, tri = wrap_mesh()
    o = normals_ref.normals(cloud(xyz), [0, len(xyz)], tri, [0, len(tri)])
    q = 2 ** 52 - 2 ** 28
    assert 2100 * q > 2 ** 63 and o["used"] == 2101
    wrapped = 2100 * q - 2 ** 64
    assert o["sums"][0].tolist() == [2 ** 40, 0, wrapped] and wrapped < 0
    n = o["normals"][0]
    assert n[2] == -1 and 0 < n[0] < 1e-6                      # the normal follows the wrapped sum: -z, although every face vector is +z


def test_counts_are_clipped_and_negative_counts_are_zero():
    xyz, off, tri, toff = cases()["fan"]
    v = cloud(xyz)
    o = normals_ref.normals(v, [0, 99], tri, [0, 999], vertex_capacity=40, triangle_capacity=50)
    same = normals_ref.normals(v[:40], [0, 40], tri[:50], [0, 50])
    assert len(o["normals"]) == 40 and o["normals"].tobytes() == same["normals"].tobytes() and o["used"] + o["skipped"] == 50
    assert o["skipped"] == int((tri[:50] >= 40).any(axis=1).sum()) > 0
    o = normals_ref.normals(v, [0, -3], tri, [0, -1])
    assert len(o["normals"]) == 0 and (o["used"], o["skipped"], o["zero_normals"]) == (0, 0, 0)
    o = normals_ref.normals(v, [0, 64], tri, [0, -1])
    assert o["zero_normals"] == 64 and o["used"] == 0


@pytest.mark.parametrize("name", sorted(RINGS))
def test_ring_orientation_on_the_oracle(orc, name):
    """Every triangle the reference's triangulation emits faces the sensor that saw it, and so does every non-zero vertex normal."""
    rig = color_cases.ring(3, sizes=[(96, 80)] * 3) if name == "3x96x80" else color_cases.ring(4, sizes=[(64, 48)] * 4)
    n_tri, n_zero, n_facing = RINGS[name]
    n = len(rig.widths)
    v, counts, t = orc.generate_mesh(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
    off = np.concatenate([[0], np.cumsum(counts[:n])]).astype(np.int32)
    o = normals_ref.normals(v, off, t, [0, len(t)])
    assert (o["used"], o["skipped"], o["zero_normals"]) == (n_tri, 0, n_zero) and len(t) == n_tri
    if name == "3x96x80":
        assert len(v) == 11087
    wt = rig.wt.reshape(n, 12).astype(np.float64)
    centres = np.stack([wt[s, 3:].reshape(3, 3) @ wt[s, :3] for s in range(n)])       # a sensor's place in the world: R t
    xyz = np.stack([v["X"], v["Y"], v["Z"]], axis=1)
    f = normals_ref.face_vectors(xyz, t)
    sensor = np.searchsorted(off, t[:, 0], side="right") - 1
    for dtype in (np.float64, np.float32):
        to_sensor = centres[sensor].astype(dtype) - xyz[t[:, 0]].astype(dtype)
        assert ((f.astype(dtype) * to_sensor).sum(axis=1) > 0).all()                    # all of them, no share left out
    nz = ~(o["sums"] == 0).all(axis=1)
    vs = np.searchsorted(off, np.arange(len(v)), side="right") - 1
    facing = (o["normals"][nz].astype(np.float64) * (centres[vs[nz]] - xyz[nz])).sum(axis=1) > 0
    assert facing.all() and int(nz.sum()) == n_facing == len(v) - n_zero
    length = np.sqrt((o["normals"][nz].astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(length - 1).max() <= 2e-7
    assert not o["normals"][~nz].any()
    if name == "3x96x80":      # sums beyond 2^24 are the rule, not the exception: the conversion rounds all over the ring
        assert int((np.abs(o["sums"]) > 2 ** 24).sum()) > 20000


def test_the_feature_is_declared():
    """Fails on a tree without the feature."""
    from livescan3d_amd.fusion import DeviceFusion
    for name in NAMES:
        assert name in native.EXPORTS, name
    assert callable(getattr(native.FusionPlan, "normals", None)) and callable(getattr(native.FusionPlan, "normals_diagnostics", None))
    assert callable(getattr(DeviceFusion, "normals", None)) and callable(getattr(native, "last_mesh_ply_normals", None))
    assert callable(getattr(native, "ply_pack_normals", None))
    header = ("ply\nformat binary_little_endian 1.0\r\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
              "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
              "element face 1\nproperty list uchar int vertex_index\nend_header\n")
    assert native.ply_normals_bytes(3, 1) == len(header) + 3 * 27 + 13
    assert native.ply_normals_bytes(3, 1) - native.ply_binary_bytes(3, 1) == 3 * 12 + len("property float nx\n") * 3
    assert native.ply_normals_bytes(-1, 0) == -1
