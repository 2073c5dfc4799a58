"""The CPU restatement of the mesh-smoothing stage (tests/smooth_ref.py): every hand-made mesh reaches what it is named for, the hashed
rule for open vertices is the exact multiset rule, one pass is what a plain-Python loop computes, the mutants of the restatement are told
apart by the cases, and the names the feature adds are there.  No GPU."""
import numpy as np
import pytest

from livescan3d_amd import native
from tests import smooth_ref
from tests.smooth_cases import cases, exact_open
from tests.simplify_ref import cloud

NAMES = ("lsnFusionSmooth", "lsnFusionSmoothDiagnostics", "lsnLastMeshPlySmooth", "lsnLastMeshTransferFrameSmooth")
CASES = cases()
# which hand-made cases must tell each mutant of the restatement from the definition
KILLS = {
    "floor": ("tiny_and_negative",),
    "dedup": ("closed_fan_free", "sixty_four_iterations"),
    "count_one": ("closed_fan", "fan_300", "bow_tie"),
    "no_mu": ("closed_fan", "one_iteration"),
    "gauss_seidel": ("closed_fan_free", "single_triangle_free"),
    "no_pin": ("single_triangle", "open_fan", "two_fans_apart"),
    "mix_identity": ("index_sums_cancel",),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_made_case_reaches_its_point(name):
    c = CASES[name]
    o = c.run()
    c.witness(o, c)
    assert o["used"] + o["skipped"] == len(c.tri) and o["vertices"].view(np.uint8).reshape(-1, 16)[:, :4].tobytes() == \
        cloud(c.xyz).view(np.uint8).reshape(-1, 16)[:, :4].tobytes()                       # the colour words are carried over
    assert np.array_equal(o["open"], exact_open(c.tri, len(c.xyz))), name


def grid_mesh(rng, w, h, drop):
    """The two triangles of every pixel quad of a w x h grid, a share `drop` of them left out."""
    i = (np.arange(h - 1)[:, None] * w + np.arange(w - 1)[None, :]).reshape(-1)
    t = np.concatenate([np.stack([i, i + 1, i + w], axis=1), np.stack([i + 1, i + w + 1, i + w], axis=1)])
    return t[rng.random(len(t)) >= drop]


def test_open_vertices_are_the_exact_multiset_rule():
    """Seeded grid meshes with dropped triangles and random triangle soup: the hash agrees with the Counter comparison on every vertex,
    and the cheaper rule on raw indices does not (which is why mix is there)."""
    rng = np.random.default_rng(2024)
    checked = open_seen = closed_seen = cheap_wrong = 0
    for _ in range(60):
        w, h = rng.integers(3, 40, 2)
        t = grid_mesh(rng, int(w), int(h), rng.uniform(0, 0.8))
        nv = int(w * h)
        want = exact_open(t, nv)
        got = smooth_ref.open_hash(t.astype(np.int64), nv) != 0
        assert np.array_equal(got, want), (w, h)
        cheap_wrong += int(((smooth_ref.open_hash(t.astype(np.int64), nv, "mix_identity") != 0) != want).sum())
        checked, open_seen, closed_seen = checked + nv, open_seen + int(want.sum()), closed_seen + int((~want).sum())
    for _ in range(200):
        nv = int(rng.integers(4, 12))
        t = rng.integers(0, nv, (int(rng.integers(1, 30)), 3))
        t = t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])]
        assert np.array_equal(smooth_ref.open_hash(t.astype(np.int64), nv) != 0, exact_open(t, nv))
        checked += nv
    assert checked > 20000 and open_seen > 1000 and closed_seen > 1000 and cheap_wrong > 0, (checked, open_seen, closed_seen, cheap_wrong)


def loop_pass(xyz, tri, f, pinned):
    """One pass in plain Python: integers of any size reduced to 64 bits two's complement, float() and / for the double steps."""
    nv = len(xyz)
    S, N = [[0, 0, 0] for _ in range(nv)], [0] * nv
    lim = np.float32(4096.0)

    def q(c):
        return int(np.trunc(np.float32(c) * np.float32(2.0 ** 32)))

    for t in np.asarray(tri).tolist():
        if not (all(0 <= i < nv for i in t) and len(set(t)) == 3):
            continue
        if not all(abs(xyz[i][k]) < lim for i in t for k in range(3)):
            continue
        for a in range(3):
            for other in (t[(a + 1) % 3], t[(a + 2) % 3]):
                for k in range(3):
                    S[t[a]][k] += q(xyz[other][k])
            N[t[a]] += 2
    out = np.array(xyz, np.float32)
    for a in range(nv):
        if N[a] == 0 or pinned[a]:
            continue
        for k in range(3):
            s = (S[a][k] + 2 ** 63) % 2 ** 64 - 2 ** 63
            m = np.float32((float(s) / float(N[a])) * 2.0 ** -32)
            d = np.float32(m - np.float32(xyz[a][k]))
            out[a][k] = np.float32(np.float32(xyz[a][k]) + np.float32(np.float32(f) * d))
    return out


@pytest.mark.parametrize("name", sorted(set(CASES) - {"fan_300"}))
def test_one_pass_is_the_plain_loop(name):
    c = CASES[name]
    for pin in (False, True):
        o = c.run(iterations=1, lam=c.lam, mu=0.0, pin_boundary=pin)
        pinned = exact_open(c.tri, len(c.xyz)) if pin else np.zeros(len(c.xyz), bool)
        with np.errstate(all="ignore"):
            want = loop_pass(c.xyz, c.tri, c.lam, pinned)
        assert o["xyz"].tobytes() == want.tobytes(), (name, pin)


@pytest.mark.parametrize("mutant", smooth_ref.MUTANTS)
def test_the_cases_kill_the_mutant(mutant):
    assert set(KILLS) == set(smooth_ref.MUTANTS)
    for name in KILLS[mutant]:
        c = CASES[name]
        assert c.run(mutant=mutant)["xyz"].tobytes() != c.run()["xyz"].tobytes(), (mutant, name)


def test_counts_are_clipped_and_parameters_are_checked():
    c = CASES["closed_fan"]
    v, off, tri, toff = c.tick()
    o = smooth_ref.smooth(v, [0, 99], tri, [0, 999], 2, 0.5, -0.53, True, vertex_capacity=6, triangle_capacity=5)
    same = smooth_ref.smooth(v[:6], [0, 6], tri[:5], [0, 5], 2, 0.5, -0.53, True)
    assert len(o["vertices"]) == 6 and o["vertices"].tobytes() == same["vertices"].tobytes() and o["used"] + o["skipped"] == 5 and o["skipped"] > 0
    o = smooth_ref.smooth(v, [0, -3], tri, [0, -1], 1, 0.5, 0.0)
    assert len(o["vertices"]) == 0 and (o["used"], o["skipped"], o["pinned"], o["isolated"]) == (0, 0, 0, 0)
    for bad in ((0, 0.5, -0.5), (65, 0.5, -0.5), (1, 0.0, -0.5), (1, 1.5, -0.5), (1, np.nan, -0.5), (1, 0.5, 0.1), (1, 0.5, -1.5), (1, 0.5, np.nan)):
        with pytest.raises(smooth_ref.Refused):
            smooth_ref.smooth(v, off, tri, toff, *bad)
    assert len(smooth_ref.factors(64, 1.0, -1.0)) == 128 and len(smooth_ref.factors(3, 0.5, 0.0)) == 3


def test_taubin_keeps_the_volume_laplacian_does_not():
    """What the mu pass is for, on an icosphere-like closed mesh (an octahedron subdivided three times, noise added): ten lambda|mu iterations keep
    the mean radius within 2 % and take out more than 40 % of the radial noise; ten Laplacian ones shrink the sphere by more than 2 %."""
    xyz, tri = noisy_sphere(np.random.default_rng(3), 3, 0.02)
    v = cloud(xyz)
    r0 = np.linalg.norm(xyz.astype(np.float64), axis=1)
    out = {}
    for name, mu in (("taubin", -0.53), ("laplacian", 0.0)):
        o = smooth_ref.smooth(v, [0, len(v)], tri, [0, len(tri)], 10, 0.5, mu, True)
        assert o["pinned"] == 0 and o["isolated"] == 0 and o["skipped"] == 0
        r = np.linalg.norm(o["xyz"].astype(np.float64), axis=1)
        out[name] = (r.mean() / r0.mean(), r.std() / r0.std())
    assert abs(out["taubin"][0] - 1) < 0.02 < 1 - out["laplacian"][0] and out["taubin"][1] < 0.6, out


def noisy_sphere(rng, levels, sigma):
    """An octahedron subdivided `levels` times onto the unit sphere, every radius scaled by 1 + N(0, sigma).  -> (xyz float32, triangles)."""
    xyz = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    tri = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(levels):
        mid, new = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = np.add(xyz[a], xyz[b]) / 2
                xyz.append(tuple(p / np.linalg.norm(p)))
                mid[key] = len(xyz) - 1
            return mid[key]

        for a, b, c in tri:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            new += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        tri = new
    xyz = np.asarray(xyz, np.float64) * (1 + rng.normal(0, sigma, (len(xyz), 1)))
    return xyz.astype(np.float32), np.asarray(tri, np.int32)


def test_the_feature_is_declared():
    """Fails on a tree without the feature."""
    from livescan3d_amd.fusion import DeviceFusion
    for name in NAMES:
        assert name in native.EXPORTS, name
    assert callable(getattr(native.FusionPlan, "smooth", None)) and callable(getattr(native.FusionPlan, "smooth_diagnostics", None))
    assert callable(getattr(DeviceFusion, "smooth", None))
    assert callable(getattr(native, "last_mesh_ply_smooth", None)) and callable(getattr(native, "last_mesh_transfer_frame_smooth", None))
