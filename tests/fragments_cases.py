"""What the tests of the fragment filter share (test infrastructure): the hand-made meshes, one for every rule of the definition and
every path of the kernels, each with a CPU witness that it reaches what it is named for, and the device check -- lsnFusionFragments into
guarded, prefilled buffers against tests/fragments_ref.py, bit for bit.  torch is handed in by the GPU tests; nothing here imports it.

The meshes are the smallest at which the kernels can still go wrong: plans of 3072 vertices per tick (one 64 x 48 sensor, or four of
32 x 24 where the offset rows matter), that is 12 workgroups of vertices and up to 24 of triangles, several ticks in one batch."""
import numpy as np

from livescan3d_amd import native
from tests import fragments_ref
from tests.simplify_cases import PREFILL, Clouds
from tests.simplify_ref import cloud
from tests.support import Guarded

ONE = ((64, 48),)            # one sensor: capacity 3072
FOUR = ((32, 24),) * 4       # four sensors, the same capacity: offset rows of five entries
CAP = 3072


class Case:
    """sizes: the plan's sensors; ticks: [(vertices VERTEX_DTYPE, offsets row, triangles int32 [m, 3], tri_offsets row)]; mins: the
    min_vertices the case is run with; witness(ref): asserts on the CPU that the case reaches what it is named for, ref(tick, min) being
    the restatement's dict."""

    def __init__(self, sizes, ticks, mins, witness):
        self.sizes, self.mins, self.witness = sizes, list(mins), witness
        n = len(sizes)
        self.ticks = []
        for nv, off, tri, toff in ticks:
            tri = np.asarray(tri, np.int32).reshape(-1, 3)
            off = np.asarray([0, nv] if off is None else off, np.int32)
            toff = np.asarray([0, len(tri)] if toff is None else toff, np.int32)
            assert len(off) == n + 1 == len(toff)
            self.ticks.append((_verts(nv), off, tri, toff))

    def ref(self, tick, min_vertices):
        v, off, tri, toff = self.ticks[tick]
        return fragments_ref.fragments(v, off, tri, toff, min_vertices, CAP, 2 * CAP)

    def check_witness(self):
        self.witness(self.ref)


def _verts(nv):
    rng = np.random.default_rng(nv)
    return cloud(rng.uniform(-1.0, 1.0, (nv, 3)))      # positions play no part: any will do


def strip(idx):
    """The triangles (idx[i], idx[i + 1], idx[i + 2]): one component of len(idx) >= 3 vertices."""
    idx = np.asarray(idx, np.int64)
    return np.stack([idx[:-2], idx[1:-1], idx[2:]], axis=1)


def fan(idx):
    idx = np.asarray(idx, np.int64)
    return np.stack([np.full(len(idx) - 2, idx[0]), idx[1:-1], idx[2:]], axis=1)


def grid(base, w, h):
    """Two triangles per cell of a w x h vertex grid whose first vertex is `base`."""
    i = (np.arange(h - 1)[:, None] * w + np.arange(w - 1)[None, :]).ravel() + base
    return np.concatenate([np.stack([i, i + 1, i + w], axis=1), np.stack([i + 1, i + w + 1, i + w], axis=1)])


def chain_depth(nv, tri):
    """The depth of vertex nv - 1 after the unions of `tri` one after the other, the higher root hooked under the lower, no compression."""
    parent = list(range(nv))

    def root(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for i0, i1, i2 in np.asarray(tri).tolist():
        for a, b in ((i0, i1), (i1, i2)):
            a, b = root(a), root(b)
            if a != b:
                parent[max(a, b)] = min(a, b)
    depth, x = 0, nv - 1
    while parent[x] != x:
        x, depth = parent[x], depth + 1
    return depth


BAD = [[0, 1, 2], [3, 4, 5], [2, 3, 6], [-1, 0, 3], [2, 3, 2 ** 30], [4, 4, 4]]


def cases():
    """name -> Case."""
    c = {}

    def w(ref):
        assert ref(0, 3)["remap"].tolist() == [0, 1, 2, 3, 4, 5, -1] and ref(0, 3)["removed_components"] == 1
        assert len(ref(0, 4)["vertices"]) == 0 and ref(0, 4)["components"] == 3
        for off_value in (1, 0, -5):
            assert ref(0, off_value)["labels"] is None and len(ref(0, off_value)["vertices"]) == 7
    c["two_triangles_and_a_loner"] = Case(ONE, [(7, None, [[0, 1, 2], [3, 4, 5]], None)], (3, 4, 1, 0, -5), w)

    # fans of m - 1, m and m + 1 vertices, m = 5, their indices interleaved
    who = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 1, 2, 2])
    tri = np.concatenate([fan(np.flatnonzero(who == k)) for k in range(3)])

    def w(ref):
        assert sorted(np.bincount(ref(0, 5)["labels"]).tolist())[-3:] == [4, 5, 6]
        assert [ref(0, m)["removed_vertices"] for m in (4, 5, 6, 7)] == [0, 4, 9, 15]
    c["threshold"] = Case(ONE, [(15, None, tri, None)], (4, 5, 6, 7), w)

    # strips of 255, 256 and 257 vertices back to back; their triangle lists padded to 255, 256 and 257 entries with triangles that join
    # nothing; both offset rows with entries on 255, 256 and 257; then the same cut at 255, 256 and 257 vertices and triangles
    parts, at = [], 0
    for k in (255, 256, 257):
        parts += [strip(np.arange(at, at + k)), [[at, at, at]] * 2]
        at += k
    tri = np.concatenate(parts)
    row = [0, 255, 256, 257, 768]
    cut = [(768, [0, 100, 200, 255, k], tri, [0, 100, 200, 255, k]) for k in (255, 256, 257)]

    def w(ref, n_tri=len(tri)):
        r = ref(0, 256)
        assert n_tri == 768 and r["removed_vertices"] == 255 and r["offsets"].tolist() == [0, 0, 1, 2, 513]
        assert r["tri_offsets"].tolist() == [0, 0, 1, 2, 513] and r["dropped_triangles"] == 255
        assert [ref(k, 255)["removed_vertices"] for k in (1, 2, 3)] == [0, 1, 2]      # cut at 255 ... 257: the first strip and loners
        assert [len(ref(k, 255)["triangles"]) for k in (1, 2, 3)] == [255] * 3 and [ref(k, 255)["dropped_triangles"] for k in (1, 2, 3)] == [0, 1, 2]
    c["tile_edges"] = Case(FOUR, [(768, row, tri, row)] + cut, (255, 256, 257), w)

    # two 600-vertex grids joined by the LAST triangle of the list; the twin has no bridge
    two = np.concatenate([grid(0, 30, 20), grid(600, 30, 20)])

    def w(ref):
        assert len(ref(0, 1000)["vertices"]) == 1200 and ref(0, 1000)["components"] == 1
        assert len(ref(1, 1000)["vertices"]) == 0 and ref(1, 1000)["components"] == 2 and ref(1, 1000)["labels"][600] == 600
    c["bridge_last"] = Case(ONE, [(1200, None, np.concatenate([two, [[599, 600, 601]]]), None), (1200, None, two, None)], (1000,), w)

    # one strip of 3000 vertices, the indices through a seeded permutation (index 0 mid-strip), the triangle order shuffled; the twin cut
    # in the middle
    rng = np.random.default_rng(5)
    perm = rng.permutation(3000)
    j = int(np.flatnonzero(perm == 0)[0])
    perm[[j, 1400]] = perm[[1400, j]]
    whole = strip(perm)
    halves = np.delete(whole, [1498, 1499], axis=0)                     # the two triangles across positions 1499 | 1500
    order = rng.permutation(len(whole))

    def w(ref):
        assert perm[1400] == 0 and ref(0, 3000)["components"] == 1 and len(ref(0, 3000)["vertices"]) == 3000
        lab = ref(1, 2)["labels"]
        lows = sorted(set(lab.tolist()))
        assert len(lows) == 2 and lows[0] == 0 and ref(1, 1501)["removed_vertices"] == 3000 and ref(1, 1500)["removed_vertices"] == 0
        pos = [int(np.flatnonzero(perm == low)[0]) for low in lows]
        assert all(p not in (0, 1499, 1500, 2999) for p in pos), pos            # neither label at the end of a half
    c["snake_permuted"] = Case(ONE, [(3000, None, whole[order], None), (3000, None, halves[order[order < len(halves)]], None)],
                               (2, 1500, 1501, 3000), w)

    # every union installs a new, lower root: the deepest forest the flatten pass can meet
    k = np.arange(2999, 0, -1)
    down = np.stack([k, k, k - 1], axis=1)

    def w(ref):
        assert chain_depth(3000, down) >= 1000
        assert (ref(0, 3000)["labels"] == 0).all() and len(ref(0, 3001)["vertices"]) == 0
    c["descending_chain"] = Case(ONE, [(3000, None, down, None)], (3000, 3001), w)

    # vertex i lies in strip i % 3 while i is below that strip's end: every run of equal labels in a wave is one lane long
    ends = (1000, 700, 400)
    tri = np.concatenate([strip(np.arange(s, ends[s], 3)) for s in range(3)])

    def w(ref):
        r = ref(0, 200)
        lab = r["labels"]
        assert (lab[1:] != lab[:-1]).all()
        sizes = [int((lab == s).sum()) for s in range(3)]
        assert sizes == [334, 233, 133] and [bool(r["remap"][s] >= 0) for s in range(3)] == [True, True, False]
    c["interleaved"] = Case(ONE, [(1000, None, tri, None)], (200,), w)

    def w(ref):
        assert (ref(0, 3072)["labels"] == 0).all() and len(ref(0, 3072)["vertices"]) == 3072 and len(ref(0, 3073)["vertices"]) == 0
    c["one_label_many_waves"] = Case(ONE, [(3072, None, strip(np.arange(3072)), None)], (3072, 3073), w)

    def w(ref):
        assert ref(0, 4)["labels"].tolist() == [0, 0, 0, 3, 3, 3] and len(ref(0, 4)["vertices"]) == 0 and ref(0, 4)["dropped_triangles"] == 6
        assert ref(1, 4)["labels"].tolist() == [0] * 6 and ref(1, 4)["triangles"].tolist() == [[0, 1, 2], [3, 4, 5], [4, 4, 4], [2, 2, 3]]
    c["bad_indices"] = Case(ONE, [(6, None, BAD, None), (6, None, BAD + [[2, 2, 3]], None)], (4, 3), w)

    # blocks {0..3}, {}, {4}, {5..11}: component {0, 1, 2, 7, 8} spans two blocks, {4, 5, 6} takes a block with it, 3 is alone, {9, 10, 11}
    tri = [[0, 1, 2], [2, 7, 8], [4, 5, 6], [4, 6, 5], [9, 10, 11], [1, 2, 7]]

    def w(ref):
        r = ref(0, 4)
        assert r["offsets"].tolist() == [0, 3, 3, 3, 5] and r["tri_offsets"].tolist() == [0, 2, 2, 2, 3]
        assert r["triangles"].tolist() == [[0, 1, 2], [2, 3, 4], [1, 2, 3]] and r["removed_components"] == 3
    c["two_sensors"] = Case(FOUR, [(12, [0, 4, 4, 5, 12], tri, [0, 2, 3, 4, 6])], (4,), w)

    # the last entries of both rows above the capacities, and below zero
    full = np.concatenate([strip(np.arange(3000)), np.full((2 * CAP - 2998, 3), -3)])

    def w(ref):
        assert len(ref(0, 2)["vertices"]) == 3000 and ref(0, 2)["removed_vertices"] == 72 and ref(0, 2)["dropped_triangles"] == 2 * CAP - 2998
        assert len(ref(0, 1)["vertices"]) == CAP and len(ref(0, 1)["triangles"]) == 2 * CAP and ref(0, 1)["offsets"].tolist() == [0, 5000]
        assert len(ref(1, 2)["remap"]) == 0 and ref(1, 2)["dropped_triangles"] == 5 and ref(1, 2)["offsets"].tolist() == [0, 0]
        assert ref(2, 2)["removed_vertices"] == 10 and ref(2, 2)["tri_offsets"].tolist() == [0, 0] and ref(2, 1)["tri_offsets"].tolist() == [0, -1]
    c["clipped_counts"] = Case(ONE, [(CAP, [0, 5000], full, [0, 7000]), (10, [0, -4], strip(np.arange(7)), [0, 5]),
                                     (10, [0, 10], strip(np.arange(7)), [0, -1])], (2, 1), w)

    def w(ref):
        assert len(ref(0, 2)["vertices"]) == 600 and len(ref(1, 2)["remap"]) == 0
        assert ref(2, 2)["removed_vertices"] == 500 and ref(2, 2)["components"] == 500 and len(ref(2, 1)["vertices"]) == 500
    c["ticks"] = Case(ONE, [(600, None, grid(0, 30, 20), None), (0, None, np.zeros((0, 3)), None), (500, None, np.zeros((0, 3)), None)], (2, 1), w)

    def w(ref):
        r = ref(0, 2 ** 31 - 1)
        assert len(r["vertices"]) == 0 and len(r["triangles"]) == 0 and r["removed_vertices"] == 600 and r["offsets"].tolist() == [0, 0]
    c["everything_removed"] = Case(ONE, [(600, None, grid(0, 30, 20), None)], (2 ** 31 - 1,), w)

    def w(ref):
        for m in (1, 0):
            assert ref(0, m)["triangles"].tolist() == BAD and ref(0, m)["dropped_triangles"] == 0 and ref(0, m)["remap"].tolist() == list(range(6))
    c["off_copies_bad_triangles"] = Case(ONE, [(6, None, BAD, None)], (1, 0), w)
    return c


class Outputs:
    """The six outputs of one call between guard bands, prefilled, in lsnFusionRunMesh's layout for T ticks of n sensors."""

    def __init__(self, torch, T, n, cap):
        self.T, self.n, self.cap = T, n, cap
        sizes = {"v": T * cap * 16, "off": T * (n + 1) * 4, "t": T * 2 * cap * 12, "toff": T * (n + 1) * 4, "remap": T * cap * 4, "labels": T * cap * 4}
        self.g = {k: Guarded(torch, b, "cuda") for k, b in sizes.items()}
        for g in self.g.values():
            g.body().fill_(PREFILL)

    def ptr(self, k):
        return self.g[k].ptr

    def intact(self):
        return all(g.intact() for g in self.g.values())

    def untouched(self):
        return self.intact() and all(bool((g.body() == PREFILL).all().item()) for g in self.g.values())

    def tensors(self, torch):
        """The four mesh outputs as tensors of a batch's shapes: the input of another call."""
        T, n, cap = self.T, self.n, self.cap
        body = lambda k, dt, shape: self.g[k].body().view(dt).reshape(shape)
        return (body("v", torch.uint8, (T, cap, 16)), body("off", torch.int32, (T, n + 1)), body("t", torch.int32, (T, 2 * cap, 3)),
                body("toff", torch.int32, (T, n + 1)))

    def host(self):
        T, n, cap = self.T, self.n, self.cap
        b = {k: g.body().cpu().numpy() for k, g in self.g.items()}
        return {"v": b["v"].reshape(T, cap, 16), "off": b["off"].view(np.int32).reshape(T, n + 1), "t": b["t"].view(np.int32).reshape(T, 2 * cap, 3),
                "toff": b["toff"].view(np.int32).reshape(T, n + 1), "remap": b["remap"].view(np.int32).reshape(T, cap),
                "labels": b["labels"].view(np.int32).reshape(T, cap)}


DIAGNOSTICS = ("components", "removed_components", "removed_vertices", "dropped_triangles")


def check_device(torch, plan, v, off, tri, toff, min_vertices, with_remap=True, with_labels=True):
    """plan.fragments(min_vertices) on the device tensors v [T, cap, 16] u8, off [T, n + 1] i32, tri [T, 2 cap, 3] i32, toff [T, n + 1] i32
    into fresh Outputs; every tick against the restatement: vertices, both offset rows, triangles, remap, labels and the diagnostics'
    four counts equal, the guard bands intact, nothing behind the new counts written, a nullable output that was not handed in untouched.
    Returns (Outputs, [the restatement's dict per tick])."""
    T, cap, n = int(v.shape[0]), int(v.shape[1]), int(off.shape[1]) - 1
    assert cap == plan.capacity and T == plan.n_ticks
    out = Outputs(torch, T, n, cap)
    plan.fragments(min_vertices, v.data_ptr(), off.data_ptr(), tri.data_ptr(), toff.data_ptr(), out.ptr("v"), out.ptr("off"), out.ptr("t"),
                   out.ptr("toff"), out.ptr("remap") if with_remap else 0, out.ptr("labels") if with_labels else 0)
    torch.cuda.synchronize()
    assert out.intact()
    got = out.host()
    hv, hoff, ht, htoff = v.cpu().numpy().reshape(T, cap, 16), off.cpu().numpy(), tri.cpu().numpy(), toff.cpu().numpy()
    refs = []
    for k in range(T):
        verts = np.ascontiguousarray(hv[k]).view(native.VERTEX_DTYPE).reshape(-1)
        r = fragments_ref.fragments(verts, hoff[k], ht[k], htoff[k], min_vertices, cap, 2 * cap)
        nv_in, nv, nt = len(r["remap"]), len(r["vertices"]), len(r["triangles"])
        want_v = r["vertices"].view(np.uint8).reshape(-1, 16)
        assert np.array_equal(got["v"][k, :nv], want_v), (k, "vertices", int((got["v"][k, :nv] != want_v).any(axis=1).sum()))
        assert (got["v"][k, nv:] == PREFILL).all(), (k, "written behind the new nVertices")
        assert np.array_equal(got["off"][k], r["offsets"]), (k, got["off"][k], r["offsets"])
        assert np.array_equal(got["t"][k, :nt], r["triangles"]), (k, "triangles", int((got["t"][k, :nt] != r["triangles"]).any(axis=1).sum()))
        assert (got["t"][k, nt:].view(np.uint8) == PREFILL).all(), (k, "written behind the new nTriangles")
        assert np.array_equal(got["toff"][k], r["tri_offsets"]), (k, got["toff"][k], r["tri_offsets"])
        if with_remap:
            assert np.array_equal(got["remap"][k, :nv_in], r["remap"]), (k, "remap")
            assert (got["remap"][k, nv_in:].view(np.uint8) == PREFILL).all(), (k, "remap written behind nVertices")
        else:
            assert (got["remap"][k].view(np.uint8) == PREFILL).all()
        if with_labels and r["labels"] is not None:
            assert np.array_equal(got["labels"][k, :nv_in], r["labels"]), (k, "labels", int((got["labels"][k, :nv_in] != r["labels"]).sum()))
            assert (got["labels"][k, nv_in:].view(np.uint8) == PREFILL).all(), (k, "labels written behind nVertices")
        else:
            assert (got["labels"][k].view(np.uint8) == PREFILL).all()
        d = plan.fragments_diagnostics(k)
        assert d == {key: r[key] for key in DIAGNOSTICS}, (k, d, {key: r[key] for key in DIAGNOSTICS})
        refs.append(r)
    return out, refs


def clouds(torch, case):
    """The case's ticks as one batch on the device (tests/simplify_cases.py Clouds)."""
    return Clouds(torch, case.ticks, sizes=case.sizes)
