"""lsnFusionOutlierFilter (csrc/outlier.hip) on the boundary cases of tests/outlier_boundary_cases.py: every case as the multi-sensor,
multi-tick batch it describes, through FusionPlan.outlier_filter on a plan of the case's frames (zero depth maps, the case's offsets).
Bit for bit: the removed flags of every tick equal what the reference's own filter() returned for every block
(tests/golden/outlier_boundary_ref.npz), and removed_per_sensor, exact_per_sensor and total equal the restatement's counts.  The vertex,
offset and depth-out buffers lie between guard bands, which stay intact, and the vertices and offsets are not written.  Every case runs
twice on one plan, the second time after a case with other settings: nothing of a call's buckets, boxes, points or totals is left for
the next.  tests/test_outlier_boundary_ref.py holds the cases to what they claim to reach and to decide."""
import os

import numpy as np
import pytest

from livescan3d_amd import native, synth
from tests import color_cases, outlier_boundary_cases as cases
from tests.support import PATTERN, Guarded

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "outlier_boundary_ref.npz")


def _shape(c):
    return tuple(c.frames), len(c.ticks)


def _other(c):
    """The case run between the two runs of c: the next case of the same plan shape, or (none there) c's own points mirrored, with
    other settings."""
    same = [x for x in cases.CASES if _shape(x) == _shape(c)]
    if len(same) > 1:
        return same[(same.index(c) + 1) % len(same)]
    return cases.Case(c.name + "_mirrored", c.frames, [[-b for b in tick] for tick in c.ticks], c.k + 1, 3 * float(min(c.max_dist, 1e10)), None)


@pytest.fixture(scope="module")
def fixture_flags():
    """name -> per tick the removed flag of every vertex, as the reference's changedVerticesMap has it."""
    g = np.load(GOLDEN)
    pos = np.concatenate([[0], np.cumsum(g["block_n"])])
    out = {name: [[] for _ in cases.BY_NAME[name].ticks] for name in (str(n) for n in g["case_names"])}
    names = [str(n) for n in g["case_names"]]
    for b in range(len(g["block_n"])):
        c = cases.BY_NAME[names[int(g["block_case"][b])]]
        t, s = int(g["block_tick"][b]), int(g["block_sensor"][b])
        assert g["points"][pos[b]:pos[b + 1]].tobytes() == c.ticks[t][s].tobytes(), (c.name, t, s)
        assert len(out[c.name][t]) == s
        out[c.name][t].append(g["changed"][pos[b]:pos[b + 1]] < 0)
    return {name: [np.concatenate(tick) if tick else np.zeros(0, bool) for tick in ticks] for name, ticks in out.items()}


class Plan:
    """A plan of one shape with its buffers: vertices, offsets and depth out between guard bands, the depth maps zero."""

    def __init__(self, torch, frames, T):
        self.torch, self.T, self.n = torch, T, len(frames)
        self.plan = native.FusionPlan(0, T, [w for w, _ in frames], [h for _, h in frames])
        self.plan.set_params(np.concatenate([synth.kinect_intrinsics(w, h) for w, h in frames]),
                             np.tile(synth.pack_pose(np.eye(3), np.zeros(3)), self.n), color_cases.WIDE_BOUNDS)
        self.cap = self.plan.capacity
        assert self.cap == sum(w * h for w, h in frames)
        self.verts = Guarded(torch, T * self.cap * 16, "cuda")
        self.offs = Guarded(torch, T * (self.n + 1) * 4, "cuda")
        self.out = Guarded(torch, T * self.cap * 2, "cuda")
        self.depth = torch.zeros(T * self.cap + 64, dtype=torch.int16, device="cuda")

    def run(self, c):
        """One call on case c; returns the diagnostics of every tick."""
        torch = self.torch
        rec = np.full((self.T, self.cap, 16), PATTERN, np.uint8)
        off = np.zeros((self.T, self.n + 1), np.int32)
        for t, tick in enumerate(c.ticks):
            pts = np.concatenate(tick) if tick else np.zeros((0, 3), np.float32)
            v = np.zeros(len(pts), native.VERTEX_DTYPE)
            v["X"], v["Y"], v["Z"] = pts[:, 0], pts[:, 1], pts[:, 2]
            v["R"], v["A"] = 7, 255
            rec[t, :len(pts)] = v.view(np.uint8).reshape(-1, 16)
            off[t] = np.cumsum([0] + [len(b) for b in tick])
            assert off[t, -1] <= self.cap
        self.verts.body().copy_(torch.from_numpy(rec.reshape(-1)).cuda())
        self.offs.body().copy_(torch.from_numpy(off.view(np.uint8).reshape(-1)).cuda())
        self.out.body().fill_(PATTERN)
        self.plan.outlier_filter(c.k, float(c.max_dist), self.depth.data_ptr(), self.verts.ptr, self.offs.ptr, self.out.ptr)
        torch.cuda.synchronize()
        assert self.verts.intact() and self.offs.intact() and self.out.intact(), (c.name, "a guard band was written")
        assert self.verts.body().cpu().numpy().tobytes() == rec.tobytes(), (c.name, "the vertices were written")
        assert self.offs.body().cpu().numpy().tobytes() == off.tobytes(), (c.name, "the offsets were written")
        assert not bool(self.out.body().any().item()), (c.name, "the masked maps are not the zero maps")
        return [self.plan.outlier_diagnostics(t, int(off[t, -1])) for t in range(self.T)]

    def check(self, c, want_flags=None):
        diags = self.run(c)
        keep, counts = c.keep(), c.counts()
        for t, d in enumerate(diags):
            removed = ~np.concatenate(keep[t]) if keep[t] else np.zeros(0, bool)
            if want_flags is not None:          # the reference's own result, with nothing in between
                assert np.array_equal(d["removed"].astype(bool), want_flags[t]), (c.name, t, np.flatnonzero(d["removed"].astype(bool) != want_flags[t])[:8])
            assert np.array_equal(d["removed"].astype(bool), removed), (c.name, t)
            assert d["removed_per_sensor"].tolist() == counts[t][0], (c.name, t, d["removed_per_sensor"].tolist(), counts[t][0])
            assert d["exact_per_sensor"].tolist() == counts[t][1], (c.name, t, d["exact_per_sensor"].tolist(), counts[t][1])
            assert d["total"] == sum(counts[t][0]), (c.name, t)


_plans = {}


@pytest.fixture(scope="module")
def plans(gpu):
    import torch

    def get(c):
        if _shape(c) not in _plans:
            _plans[_shape(c)] = Plan(torch, *_shape(c))
        return _plans[_shape(c)]
    yield get
    for p in _plans.values():
        p.plan.close()
    _plans.clear()


def test_every_case_is_in_the_fixture(fixture_flags):
    assert list(fixture_flags) == cases.NAMES


@pytest.mark.parametrize("name", cases.NAMES)
def test_case_equals_the_reference(plans, fixture_flags, name):
    c = cases.BY_NAME[name]
    other = _other(c)
    assert (other.k, float(other.max_dist)) != (c.k, float(c.max_dist)) or any(a.tobytes() != b.tobytes() for (_, _, a), (_, _, b) in zip(other.blocks(), c.blocks()))
    p = plans(c)
    p.check(c, fixture_flags[name])
    p.check(other, fixture_flags.get(other.name))
    p.check(c, fixture_flags[name])
