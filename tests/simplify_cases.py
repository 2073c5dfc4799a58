"""What the tests of the mesh level-of-detail stage share (test infrastructure): the hand-made clouds, one for every rule of the
definition, and the device check -- lsnFusionSimplify into guarded, prefilled buffers against tests/simplify_ref.py, bit for bit.
torch is handed in by the GPU tests; nothing here imports it."""
import numpy as np

from livescan3d_amd import native
from tests import simplify_ref
from tests.support import Guarded

PREFILL = 249   # -7 as a byte: what DeviceFusion prefills its tables with


def cases():
    """name -> (xyz [n, 3], offsets row, triangles or None, tri_offsets or None, cell): the hand-made clouds, shared with the GPU test."""
    inf, nan = np.inf, np.nan
    c = {}
    c["two_in_one_cell"] = ([[0.01, 0.01, 0.01], [0.04, 0.02, 0.03], [0.11, 0.01, 0.01]], [0, 3], None, None, 0.1)
    # floor, not truncation: -0.01 and +0.01 lie in cells -1 and 0; -0.19 in cell -2, -0.11 with it
    c["negative_coordinates"] = ([[-0.01, 0, 0], [0.01, 0, 0], [-0.19, 0, 0], [-0.11, 0, 0], [-0.05, 0, 0]], [0, 5], None, None, 0.1)
    # exactly on k * cell (0.25 = 2^-2: the products are exact): the boundary belongs to the upper cell
    c["on_the_boundary"] = ([[0.25, 0.5, -0.25], [0.26, 0.5, -0.25], [0.2499, 0.5, -0.25], [0.5, 0.74, -0.01], [-0.25, 0, 0], [-0.2501, 0, 0]],
                            [0, 6], None, None, 0.25)
    c["unclustered"] = ([[nan, 0, 0], [nan, 0, 0], [0, inf, 0], [0, inf, 0], [0, 0, -inf], [0.01, 0.01, 0.01], [0.02, 0.02, 0.02],
                         [2 ** 20 * 0.5, 0, 0], [2 ** 20 * 0.5, 0, 0], [2 ** 20 * 0.5 - 0.5, 0, 0], [2 ** 20 * 0.5 - 0.4, 0, 0],
                         [-2 ** 20 * 0.5, 0, 0], [-2 ** 20 * 0.5 + 0.1, 0, 0], [-2 ** 20 * 0.5 - 0.5, 0, 0], [-2 ** 20 * 0.5 - 0.4, 0, 0]],
                        [0, 15], None, None, 0.5)
    # vertices 0, 1 share a cell, 2, 3, 4 have their own: an edge collapse, a point collapse, survivors, bad indices, a duplicate pair
    xyz = [[0.01, 0, 0], [0.02, 0, 0], [0.15, 0, 0], [0.25, 0, 0], [0.35, 0, 0]]
    tris = [[0, 1, 2], [0, 1, 0], [2, 3, 4], [0, 2, 3], [1, 2, 3], [0, 1, 5], [-1, 2, 3], [2, 3, 2 ** 30], [4, 3, 2], [1, 1, 1], [3, 4, 0]]
    c["triangles"] = (xyz, [0, 5], tris, [0, len(tris)], 0.1)
    # a cell that spans two sensor blocks (vertices 1 and 3), an empty block, a block that vanishes whole
    c["two_sensors"] = ([[0.01, 0, 0], [0.11, 0, 0], [0.21, 0, 0], [0.12, 0, 0], [0.31, 0, 0], [0.02, 0.01, 0], [0.32, 0, 0]], [0, 3, 3, 5, 7],
                        [[0, 1, 2], [1, 2, 4], [3, 4, 2], [2, 3, 1], [5, 6, 2], [4, 6, 0]], [0, 1, 1, 4, 6], 0.1)
    return {k: (np.asarray(x, np.float32), np.asarray(o, np.int32), None if t is None else np.asarray(t, np.int32),
                None if to is None else np.asarray(to, np.int32), cell) for k, (x, o, t, to, cell) in c.items()}


class Outputs:
    """The five outputs of one call between guard bands, prefilled, in lsnFusionRunMesh's layout for T ticks of n sensors."""

    def __init__(self, torch, T, n, cap):
        self.T, self.n, self.cap = T, n, cap
        sizes = {"v": T * cap * 16, "off": T * (n + 1) * 4, "t": T * 2 * cap * 12, "toff": T * (n + 1) * 4, "remap": T * cap * 4}
        self.g = {k: Guarded(torch, b, "cuda") for k, b in sizes.items()}
        for g in self.g.values():
            g.body().fill_(PREFILL)

    def ptr(self, k):
        return self.g[k].ptr

    def intact(self):
        return all(g.intact() for g in self.g.values())

    def untouched(self):
        return self.intact() and all(bool((g.body() == PREFILL).all().item()) for g in self.g.values())

    def host(self):
        T, n, cap = self.T, self.n, self.cap
        b = {k: g.body().cpu().numpy() for k, g in self.g.items()}
        return {"v": b["v"].reshape(T, cap, 16), "off": b["off"].view(np.int32).reshape(T, n + 1), "t": b["t"].view(np.int32).reshape(T, 2 * cap, 3),
                "toff": b["toff"].view(np.int32).reshape(T, n + 1), "remap": b["remap"].view(np.int32).reshape(T, cap)}


def check_device(torch, plan, v, off, tri, toff, cell, points=False, with_remap=True):
    """plan.simplify(cell) on the device tensors v [T, cap, 16] u8, off [T, n + 1] i32, tri [T, 2 cap, 3] i32, toff [T, n + 1] i32 into
    fresh Outputs; every tick against the restatement: vertices, both offset rows, triangles, remap and the diagnostics' three counts
    equal, the guard bands intact, nothing behind the new counts written.  Returns (Outputs, [the restatement's dict per tick])."""
    T, cap, n = int(v.shape[0]), int(v.shape[1]), int(off.shape[1]) - 1
    assert cap == plan.capacity and T == plan.n_ticks
    out = Outputs(torch, T, n, cap)
    plan.simplify(cell, v.data_ptr(), off.data_ptr(), 0 if points else tri.data_ptr(), 0 if points else toff.data_ptr(), out.ptr("v"), out.ptr("off"),
                  0 if points else out.ptr("t"), 0 if points else out.ptr("toff"), out.ptr("remap") if with_remap else 0)
    torch.cuda.synchronize()
    assert out.intact()
    got = out.host()
    hv, hoff = v.cpu().numpy().reshape(T, cap, 16), off.cpu().numpy()
    ht, htoff = (None, None) if points else (tri.cpu().numpy(), toff.cpu().numpy())
    refs = []
    for k in range(T):
        verts = np.ascontiguousarray(hv[k]).view(native.VERTEX_DTYPE).reshape(-1)
        r = simplify_ref.simplify(verts, hoff[k], None if points else ht[k], None if points else htoff[k], cell, cap, 2 * cap)
        nv_in, nv = len(r["remap"]), len(r["vertices"])
        want_v = r["vertices"].view(np.uint8).reshape(-1, 16)
        assert np.array_equal(got["v"][k, :nv], want_v), (k, "vertices", int((got["v"][k, :nv] != want_v).any(axis=1).sum()))
        assert (got["v"][k, nv:] == PREFILL).all(), (k, "written behind the new nVertices")
        assert np.array_equal(got["off"][k], r["offsets"]), (k, got["off"][k], r["offsets"])
        if with_remap:
            assert np.array_equal(got["remap"][k, :nv_in], r["remap"]), (k, "remap")
            assert (got["remap"][k, nv_in:].view(np.uint8) == PREFILL).all(), (k, "remap written behind nVertices")
        else:
            assert (got["remap"][k].view(np.uint8) == PREFILL).all()
        if points:
            assert (got["t"][k].view(np.uint8) == PREFILL).all() and (got["toff"][k].view(np.uint8) == PREFILL).all()
        else:
            nt = len(r["triangles"])
            assert np.array_equal(got["t"][k, :nt], r["triangles"]), (k, "triangles", int((got["t"][k, :nt] != r["triangles"]).any(axis=1).sum()))
            assert (got["t"][k, nt:].view(np.uint8) == PREFILL).all(), (k, "written behind the new nTriangles")
            assert np.array_equal(got["toff"][k], r["tri_offsets"]), (k, got["toff"][k], r["tri_offsets"])
        d = plan.simplify_diagnostics(k)
        assert d == {"cells": r["cells"], "unclustered": r["unclustered"], "dropped_triangles": r["dropped_triangles"]}, (k, d)
        refs.append(r)
    return out, refs


class Clouds:
    """A plan of `sizes` sensors per tick with hand-made clouds uploaded as its ticks: ticks[k] = (vertices VERTEX_DTYPE, offsets row,
    triangles or None, tri_offsets row or None)."""

    def __init__(self, torch, ticks, sizes=((8, 8),)):
        self.torch, self.T = torch, len(ticks)
        self.plan = native.FusionPlan(0, self.T, [s[0] for s in sizes], [s[1] for s in sizes])
        cap, n = self.plan.capacity, len(sizes)
        v = np.full((self.T, cap, 16), 0x5A, np.uint8)       # what lies behind a tick's counts is never read
        t = np.full((self.T, 2 * cap, 3), -3, np.int32)
        off, toff = np.zeros((self.T, n + 1), np.int32), np.zeros((self.T, n + 1), np.int32)
        for k, (cv, co, ct, cto) in enumerate(ticks):
            assert len(cv) <= cap and len(co) == n + 1
            v[k, :len(cv)] = np.frombuffer(cv.tobytes(), np.uint8).reshape(-1, 16)
            off[k] = co
            if ct is not None:
                assert len(ct) <= 2 * cap
                t[k, :len(ct)] = ct
                toff[k] = cto
        self.v, self.t, self.off, self.toff = (torch.from_numpy(a).cuda() for a in (v, t, off, toff))

    def check(self, cell, points=False, with_remap=True):
        return check_device(self.torch, self.plan, self.v, self.off, self.t, self.toff, cell, points, with_remap)

    def close(self):
        self.plan.close()
