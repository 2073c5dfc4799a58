"""tri_kernel (csrc/mesh.hip) on the boundary frames of tests/tri_cases.py, in its three forms -- the device-resident VEC form (widths % 8
== 0, compact pixel -> vertex map), the general per-pixel form and the HOST form of generateMeshFromDepthMaps -- against the CPU oracle
and, with nothing in between, against what the reference's own generateTrianglesGradients returned (tests/golden/tri_boundary_ref.npz).
Bit for bit: vertices, offsets, triangle offsets, triangles in order.  Nothing here has a tolerance.  tests/test_tri_boundary_ref.py holds
the frames to what they claim to contain."""
import functools
import os

import numpy as np
import pytest

from livescan3d_amd import native
from tests import tri_cases
from tests.support import PATTERN, Guarded

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tri_boundary_ref.npz")


@functools.lru_cache(maxsize=None)
def _frames():
    vec, gen = tri_cases.vec_frame(), tri_cases.general_frame()
    out = {f.name: f for g in (vec, gen) for f in (g.with_background("holes"), g.with_background("dense"))}
    out.update({f.name: f for f in (tri_cases.hand_frame(64), tri_cases.hand_frame(61))})
    out.update({f.name: f for f in tri_cases.write_pass_frames()})
    # a write-pass frame as a tick of the VEC frame's plan: the same first tile, nothing below
    d = np.zeros_like(vec.depth)
    d[:40] = out["write64x40_1537"].depth
    out["write_in_vec64"] = tri_cases.frame_of("write_in_vec64", d)
    # sensor 0 of the two-sensor plan: 61 x 9, every pixel with a vertex
    rng = np.random.default_rng(61)
    out["head61x9"] = tri_cases.frame_of("head61x9", (1500 + rng.integers(-6, 7, size=(9, 61))).astype(np.uint16))
    return out


_oracle_cache = {}


def _oracle(orc, names, box):
    """orc.generate_mesh of the frames `names` as the sensors of one call under `box`: computed once per rig, never changed."""
    key = (tuple(names), box.tobytes())
    if key not in _oracle_cache:
        rig = tri_cases.rig_of([_frames()[n] for n in names], box)
        v, counts, tri = orc.generate_mesh(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
        for a in (v, counts, tri):
            a.setflags(write=False)
        _oracle_cache[key] = (v, counts, tri)
    return _oracle_cache[key]


def _assert_triangles(orc, names, box, got, want, what):
    """got == want, or: the first differing triangle, its pixel and the stencil (target tuple) that pixel belongs to."""
    if got.shape == want.shape and np.array_equal(got, want):
        return
    n = min(len(got), len(want))
    diff = np.nonzero((got[:n] != want[:n]).any(axis=1))[0]
    k = int(diff[0]) if len(diff) else n
    here = want[k] if k < len(want) else got[k]
    where, base = "?", 0
    for name in names:
        f = _frames()[name]
        v, v2p, _ = orc.create_vertices(f.depth, f.rgb(), tri_cases.intrinsics(f.w, f.h), tri_cases.POSE, box, want_maps=True)
        if base <= int(here[0]) < base + len(v):
            pix = int(v2p[int(here[0]) - base])
            where = f.describe(pix % f.w, pix // f.w)
            break
        base += len(v)
    pytest.fail(f"{what}: {len(got)} triangles, the reference has {len(want)}; first difference at triangle {k}: got "
                f"{got[k].tolist() if k < len(got) else None}, want {want[k].tolist() if k < len(want) else None}; its first vertex is {where}")


class _Run:
    """One plan of len(ticks) ticks (each a list of frame names, the sensors) run through lsnFusionRunMesh, every output in a guarded
    buffer prefilled with the guard pattern."""

    def __init__(self, gpu, ticks, box):
        import torch
        from livescan3d_amd.fusion import upload_rigs
        self.torch, self.ticks, self.box = torch, ticks, box
        rigs = [tri_cases.rig_of([_frames()[n] for n in names], box) for names in ticks]
        self.T, self.N = len(ticks), rigs[0].n
        self.plan = native.FusionPlan(gpu.index, self.T, rigs[0].widths, rigs[0].heights)
        self.stream = int(torch.cuda.current_stream().cuda_stream)
        self.plan.set_params(rigs[0].intr, rigs[0].wt, box, self.stream)
        self.depth, self.rgb = upload_rigs(rigs, self.T, gpu.index)
        self.cap = self.plan.capacity
        self.vec = bool((rigs[0].widths % 8 == 0).all()) and self.plan.pixels_per_tick % 8 == 0 and self.depth.data_ptr() % 16 == 0
        self.vertices = Guarded(torch, self.T * self.cap * 16, gpu)
        self.offsets = Guarded(torch, self.T * (self.N + 1) * 4, gpu)
        self.triangles = Guarded(torch, self.T * 2 * self.cap * 12, gpu)
        self.tri_offsets = Guarded(torch, self.T * (self.N + 1) * 4, gpu)
        self.buffers = (self.vertices, self.offsets, self.triangles, self.tri_offsets)

    def run(self):
        self.plan.run_mesh(self.depth.data_ptr(), self.rgb.data_ptr(), self.vertices.ptr, self.offsets.ptr, self.triangles.ptr,
                           self.tri_offsets.ptr, self.stream)
        self.torch.cuda.synchronize()
        return [b.buf.cpu().numpy().copy() for b in self.buffers]

    def host(self):
        """(vertices uint8 [T, cap, 16], offsets [T, N + 1], triangles int32 [T, 2 cap, 3], tri_offsets [T, N + 1]) and the guards' verdict."""
        assert all(b.intact() for b in self.buffers), "a guard band was written"
        v = self.vertices.body().cpu().numpy().reshape(self.T, self.cap, 16)
        o = self.offsets.body().cpu().numpy().view(np.int32).reshape(self.T, self.N + 1)
        t = self.triangles.body().cpu().numpy().view(np.int32).reshape(self.T, 2 * self.cap, 3)
        to = self.tri_offsets.body().cpu().numpy().view(np.int32).reshape(self.T, self.N + 1)
        return v, o, t, to

    def check(self, orc):
        """Every tick against the oracle; nothing behind a tick's last triangle or vertex.  Returns the ticks' triangle lists."""
        v, o, t, to = self.host()
        out = []
        for k, names in enumerate(self.ticks):
            want_v, counts, want_t = _oracle(orc, names, self.box)
            what = f"tick {k} ({' + '.join(names)}, {'VEC' if self.vec else 'general'} form)"
            assert list(o[k]) == [0] + list(np.cumsum(counts)), what
            assert v[k, :len(want_v)].tobytes() == want_v.tobytes(), f"{what}: vertex bytes differ"
            assert to[k, 0] == 0 and (np.diff(to[k]) >= 0).all() and 0 <= to[k, -1] <= 2 * self.cap, (what, to[k])
            nt = int(to[k, -1])
            _assert_triangles(orc, names, self.box, t[k, :nt], want_t, what)
            assert (t[k, nt:].view(np.uint8) == PATTERN).all(), f"{what}: written behind tri_offsets[-1]"
            out.append(t[k, :nt].copy())
        return out

    def close(self):
        self.plan.close()


def _run_checked(gpu, orc, ticks, box, twice=False, want_vec=None):
    r = _Run(gpu, ticks, box)
    try:
        if want_vec is not None:
            assert r.vec == want_vec
        first = r.run()
        tris = r.check(orc)
        if twice:     # once more into the same buffers: the same bytes (the passes' scratch -- codes, tile counts -- is reused)
            again = r.run()
            assert all(np.array_equal(a, b) for a, b in zip(first, again)), "the second run of the plan wrote other bytes"
        return tris
    finally:
        r.close()


VEC_TICKS = [["vec64_holes"], ["vec64_dense"], ["write_in_vec64"]]


@functools.lru_cache(maxsize=None)
def _vec_triangles(gpu, orc):
    """The VEC frames' triangles from the device-resident VEC form, checked against the oracle: computed once."""
    tris = _run_checked(gpu, orc, VEC_TICKS, tri_cases.BOX, twice=True, want_vec=True)
    for t in tris:
        t.setflags(write=False)
    return tris


def test_device_vec_form_three_tick_plan(gpu, orc):
    """The VEC frame with holes, the VEC frame dense and a write-pass frame as the three ticks of one plan, twice into the same buffers."""
    tris = _vec_triangles(gpu, orc)
    assert len(tris[0]) > 500 and len(tris[1]) > 500 and len(tris[2]) == 1537


@pytest.mark.parametrize("name", ["vec64_holes", "vec64_dense"])
def test_device_vec_form_one_tick_plan(gpu, orc, name):
    """A one-tick plan: the vertex pass is the single pass that writes the compact map."""
    (got,) = _run_checked(gpu, orc, [[name]], tri_cases.BOX, want_vec=True)
    assert np.array_equal(got, _vec_triangles(gpu, orc)[["vec64_holes", "vec64_dense"].index(name)])


def test_device_general_form(gpu, orc):
    """The general frame (width 61: tiles begin mid-row, a lane's pixels span rows), both backgrounds, and the special stencils under the
    wide box at both widths."""
    _run_checked(gpu, orc, [["gen61_holes"], ["gen61_dense"]], tri_cases.BOX, twice=True, want_vec=False)
    _run_checked(gpu, orc, [["hand61"]], tri_cases.WIDE_BOX, want_vec=False)
    _run_checked(gpu, orc, [["hand64"]], tri_cases.WIDE_BOX, want_vec=True)


def test_vec_frame_through_the_general_form_as_second_sensor(gpu, orc):
    """The VEC frame as sensor 1 behind a 61 x 9 sensor: the plan is not a VEC plan, the same stencils go through the per-pixel path, and
    index_base and the frame's depth_off / tile_start are non-zero.  Sensor 1's triangles are the VEC run's, shifted by sensor 0's vertices."""
    ticks = [["head61x9", "vec64_holes"], ["head61x9", "vec64_dense"]]
    tris = _run_checked(gpu, orc, ticks, tri_cases.BOX, want_vec=False)
    for k, names in enumerate(ticks):
        _, counts, _ = _oracle(orc, names, tri_cases.BOX)
        _, _, head = _oracle(orc, names[:1], tri_cases.BOX)
        assert counts[0] == 61 * 9 and len(head) > 0
        assert np.array_equal(tris[k][:len(head)], head)
        _assert_triangles(orc, names, tri_cases.BOX, tris[k][len(head):], _vec_triangles(gpu, orc)[k] + counts[0], f"sensor 1 of tick {k}")


def _host(orc, name, box):
    f = _frames()[name]
    rig = tri_cases.rig_of([f], box)
    v, t = native.generate_mesh_from_depth_maps(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds,
                                                generate_triangles=True, overlay_merge=False)
    want_v, _, want_t = _oracle(orc, [name], box)
    assert v.tobytes() == want_v.tobytes(), f"{name}: vertex bytes differ"
    _assert_triangles(orc, [name], box, t, want_t, f"{name} (HOST form)")
    return v, t


def test_host_form_every_frame(gpu, orc):
    """generateMeshFromDepthMaps (triangles on): the VEC and the general frame, both backgrounds, the special stencils, every write-pass
    frame -- against the oracle, and the frames of the fixture against the reference's own output with no oracle in between."""
    z = np.load(GOLDEN)
    pinned = set(z["names"])
    assert len(pinned) == 4 + 2 * (len(tri_cases.WRITE_COUNTS) + 1)
    for name, f in _frames().items():
        if name in ("write_in_vec64", "head61x9"):
            continue
        v, t = _host(orc, name, f.box)
        if name in pinned:
            assert np.array_equal(z[f"{name}_depth"], f.depth), name
            assert len(v) == int((z[f"{name}_p2v"] != -1).sum()), name
            _assert_triangles(orc, [name], f.box, t, z[f"{name}_tri"], f"{name} (HOST form against the reference's own output)")
            pinned.discard(name)
    assert not pinned


@pytest.mark.parametrize("w,h", tri_cases.WRITE_SIZES)
def test_write_pass_counts(gpu, orc, w, h):
    """Flat frames whose first tile emits exactly 0, 1, 15 .. 17, 1535 .. 1537 (the staged window), 3071 .. 3073 triangles, the full tile,
    and an empty first tile in front of a second one that is not: one plan with a tick each (64 x 40: the VEC form; 61 x 42: the general
    form) and the HOST form.  tri_offsets holds the exact counts, the guards and everything behind a tick's last triangle stay untouched."""
    keys = list(tri_cases.WRITE_COUNTS) + ["tile1"]
    names = [f"write{w}x{h}_{k}" for k in keys]
    r = _Run(gpu, [[n] for n in names], tri_cases.WIDE_BOX)
    try:
        assert r.vec == (w % 8 == 0)
        r.run()
        r.check(orc)
        to = r.host()[3]
    finally:
        r.close()
    for tick, (k, name) in enumerate(zip(keys, names)):
        counts = tri_cases.tile_counts(_frames()[name].depth)
        assert list(to[tick]) == [0, sum(counts)], (name, to[tick])
        if k == "tile1":
            assert counts[0] == 0 and counts[1] > 0
        elif k != "full":
            assert counts == [k, 0] and to[tick, -1] == k
        _, t = _host(orc, name, tri_cases.WIDE_BOX)
        assert len(t) == sum(counts)
