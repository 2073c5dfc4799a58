"""The CPU restatement of the fragment filter (tests/fragments_ref.py): every hand-made case with its witness, a second opinion from
scipy's connected components, mutants of the restatement each caught by a named case, idempotence, the known answers on the oracle's
rings, and the names the feature adds.  No GPU."""
import numpy as np
import pytest

from livescan3d_amd import native
from tests import color_cases, fragments_ref
from tests.fragments_cases import CAP, cases

NAMES = ("lsnFusionFragments", "lsnFusionFragmentsDiagnostics", "lsnLastMeshTransferFrameFragments", "lsnLastMeshPlyFragments")
CASES = cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_reaches_what_it_is_named_for(name):
    CASES[name].check_witness()


def _counted(case, tick):
    v, off, tri, toff = case.ticks[tick]
    nv, nt = min(max(int(off[-1]), 0), CAP), min(max(int(toff[-1]), 0), 2 * CAP)
    return nv, tri[:nt]


@pytest.mark.parametrize("name", sorted(CASES))
def test_labels_and_sizes_agree_with_scipy(name):
    """scipy.sparse.csgraph.connected_components on the edges i0-i1, i1-i2 of the valid triangles, its components relabelled by their
    lowest index: an independent second opinion on labels and sizes."""
    from scipy import sparse
    from scipy.sparse.csgraph import connected_components
    case = CASES[name]
    for tick in range(len(case.ticks)):
        nv, t = _counted(case, tick)
        r = case.ref(tick, 2)
        if nv == 0:
            assert len(r["labels"]) == 0
            continue
        t = t[((t >= 0) & (t < nv)).all(axis=1)].astype(np.int64)
        rows, cols = np.concatenate([t[:, 0], t[:, 1]]), np.concatenate([t[:, 1], t[:, 2]])
        graph = sparse.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(nv, nv))
        n_comp, comp = connected_components(graph, directed=False)
        lowest = np.full(n_comp, nv)
        np.minimum.at(lowest, comp, np.arange(nv))
        assert np.array_equal(r["labels"], lowest[comp]), (name, tick)
        assert r["components"] == n_comp
        sizes = np.bincount(comp)
        assert r["removed_vertices"] == int((sizes[comp] < 2).sum())
        for m in case.mins:
            if m > 1:
                assert np.array_equal(case.ref(tick, m)["remap"] >= 0, sizes[comp] >= m), (name, tick, m)


def _mutant(kind, nv, tri, min_vertices):
    """-> (labels, kept) of a restatement with one rule changed."""
    parent = list(range(nv))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            if kind == "label_is_highest":
                parent[min(a, b)] = max(a, b)
            else:
                parent[max(a, b)] = min(a, b)

    for i0, i1, i2 in np.asarray(tri, np.int64).reshape(-1, 3).tolist():
        ok = [0 <= i < nv for i in (i0, i1, i2)]
        if kind == "invalid_join_their_valid_indices":
            if ok[0] and ok[1]:
                union(i0, i1)
            if ok[1] and ok[2]:
                union(i1, i2)
            continue
        if not all(ok):
            continue
        if kind == "degenerate_ignored" and (i0 == i1 or i1 == i2 or i0 == i2):
            continue
        union(i0, i1)
        if kind == "third_edge_for_second":
            union(i0, i2)
        elif kind != "second_edge_left_out":
            union(i1, i2)
    label = np.array([find(v) for v in range(nv)], np.int64).reshape(nv)
    size = np.bincount(label, minlength=nv)
    return label, (size[label] > min_vertices if kind == "greater_for_greater_equal" else size[label] >= min_vertices)


# mutant -> (the case that catches it, tick, min_vertices)
CAUGHT_BY = {"second_edge_left_out": ("two_triangles_and_a_loner", 0, 3), "label_is_highest": ("snake_permuted", 0, 2),
             "greater_for_greater_equal": ("threshold", 0, 5), "invalid_join_their_valid_indices": ("bad_indices", 0, 4),
             "degenerate_ignored": ("bad_indices", 1, 4)}


def _same(case, tick, m, kind):
    nv, t = _counted(case, tick)
    label, kept = _mutant(kind, nv, t, m)
    r = case.ref(tick, m)
    return np.array_equal(label, r["labels"]) and np.array_equal(kept, r["remap"] >= 0)


@pytest.mark.parametrize("kind", sorted(CAUGHT_BY))
def test_mutants_of_the_restatement_are_caught(kind):
    name, tick, m = CAUGHT_BY[kind]
    assert _same(CASES[name], tick, m, "none")          # the mutant's own code, no rule changed: the restatement
    assert not _same(CASES[name], tick, m, kind)


def test_the_third_edge_in_place_of_the_second_is_the_same_function():
    """Any two edges of a triangle span its three vertices: joining i0-i2 where the definition joins i1-i2 changes no label, so no case can
    catch it (only leaving the second edge out WITHOUT a replacement is a mutant, above).  Held here on every case."""
    for name, case in CASES.items():
        for tick in range(len(case.ticks)):
            assert _same(case, tick, 2, "third_edge_for_second"), (name, tick)


@pytest.mark.parametrize("name", sorted(CASES))
def test_idempotent(name):
    case = CASES[name]
    for tick in range(len(case.ticks)):
        for m in case.mins:
            o = case.ref(tick, m)
            again = fragments_ref.fragments(o["vertices"], o["offsets"], o["triangles"], o["tri_offsets"], m)
            if m > 1:      # (off copies rows and triangles as they are: the counts of a clipped row are not the rows' last entries)
                assert again["vertices"].tobytes() == o["vertices"].tobytes(), (name, tick, m)
                for k in ("offsets", "triangles", "tri_offsets"):
                    assert np.array_equal(again[k], o[k]), (name, tick, m, k)
                assert again["remap"].tolist() == list(range(len(o["vertices"]))) and again["removed_vertices"] == 0


# rig -> {min_vertices: (removed vertices, removed components)}; vertices, triangles, components
RINGS = {(3, 96, 80): (11087, 16924, 1471, {256: (1995, 1467), 2: (1458, 1458)}),
         (4, 64, 48): (6084, 6174, 2145, {64: (2193, 2129)})}


@pytest.mark.parametrize("ring", sorted(RINGS))
def test_known_answers_on_the_oracles_rings(orc, ring):
    n, w, h = ring
    rig = color_cases.ring(n, sizes=[(w, h)] * n)
    v, counts, t = orc.generate_mesh(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
    off = np.concatenate([[0], np.cumsum(counts[:n])]).astype(np.int32)
    nv, nt, comps, answers = RINGS[ring]
    assert (len(v), len(t)) == (nv, nt)
    for m, (removed, removed_comps) in answers.items():
        o = fragments_ref.fragments(v, off, t, [0] * n + [len(t)], m)
        assert (o["components"], o["removed_vertices"], o["removed_components"]) == (comps, removed, removed_comps), m
        assert o["offsets"][-1] == len(o["vertices"]) == nv - removed and o["tri_offsets"][-1] == len(o["triangles"]) == nt - o["dropped_triangles"]
        again = fragments_ref.fragments(o["vertices"], o["offsets"], o["triangles"], o["tri_offsets"], m)
        assert again["vertices"].tobytes() == o["vertices"].tobytes() and np.array_equal(again["triangles"], o["triangles"])


def test_the_feature_is_declared():
    """Fails on a tree without the feature."""
    from livescan3d_amd import fusion
    for name in NAMES:
        assert name in native.EXPORTS, name
    assert callable(getattr(native.FusionPlan, "fragments", None)) and callable(getattr(native.FusionPlan, "fragments_diagnostics", None))
    assert callable(getattr(fusion.DeviceFusion, "fragments", None))
    assert callable(getattr(native, "last_mesh_transfer_frame_fragments", None)) and callable(getattr(native, "last_mesh_ply_fragments", None))
