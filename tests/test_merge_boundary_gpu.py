"""lsnFusionOverlayMerge (csrc/merge.hip) and the host export with the merge on the boundary rigs of tests/merge_boundary_cases.py, against
the CPU reference (tests/merge_ref.py) and, with nothing in between, against what the reference's own generateMeshFromDepthMaps
returned (tests/golden/merge_boundary_ref.npz).  Bit for bit: triangles in order, reprojected and merged maps, point_assigned.  Nothing
here has a tolerance.  tests/test_merge_boundary_ref.py holds the rigs to what they claim to reach: zero writers with and without a later
writer (mg_raster_kernel<0>'s val == 0 branch, the t > zmax filter, mg_resolve_kernel's zero-only branch and its reset of zmax / key),
both sides of depth_threshold and of the confidence threshold, every drop test of the projection, colliding reprojections, den == 0."""
import functools
import os

import numpy as np
import pytest

from livescan3d_amd import native
from tests import color_ref, merge_boundary_cases as cases, merge_ref, render_ref
from tests.support import PATTERN, Clouds, Guarded, export

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merge_boundary_ref.npz")
MERGED = dict(generate_triangles=True, overlay_merge=True)

_refs = {}


def _ref(orc, rig_or_name):
    """merge_ref.overlay_merge of a rig: computed once, never changed."""
    rig = cases.rig(rig_or_name) if isinstance(rig_or_name, str) else rig_or_name
    if id(rig) not in _refs:
        tris, diag = merge_ref.overlay_merge(rig, orc)
        for a in (tris, *diag.values()):
            a.setflags(write=False)
        _refs[id(rig)] = (rig, tris, diag)
    return _refs[id(rig)][1:]


@functools.lru_cache(maxsize=None)
def _fixture():
    return np.load(GOLDEN)


class Merge:
    """A plan of the rigs' sizes with the triangles and their offsets in guarded caller buffers: run_mesh, then the overlay merge."""

    def __init__(self, rigs):
        import torch
        from livescan3d_amd.fusion import SENTINEL, DeviceFusion
        self.torch = torch
        self.fus = DeviceFusion.from_rigs(rigs)
        T, n, cap = self.fus.n_ticks, self.fus.n_maps, self.fus.capacity
        self.tri = Guarded(torch, T * 2 * cap * 12, self.fus.device)
        self.toff = Guarded(torch, T * (n + 1) * 4, self.fus.device)
        self.toff.body().view(torch.int32).fill_(SENTINEL)
        self.T, self.n, self.cap = T, n, cap

    def load(self, rigs, params=False):
        """Other frames (and, with params, their calibration) into the same plan."""
        from livescan3d_amd.fusion import upload_rigs
        if params:
            self.fus.set_params(rigs[0].intr, rigs[0].wt, rigs[0].bounds)
        self.fus.depth, self.fus.rgb = upload_rigs(rigs, self.T, self.fus.device.index)

    def run(self, order=("merge",)):
        f, s = self.fus, int(self.torch.cuda.current_stream().cuda_stream)
        f.plan.run_mesh(f.depth.data_ptr(), f.rgb.data_ptr(), f.vertices.data_ptr(), f.offsets.data_ptr(), self.tri.ptr, self.toff.ptr, s)
        for stage in order:
            if stage == "merge":
                f.plan.overlay_merge(f.depth.data_ptr(), f.vertices.data_ptr(), f.offsets.data_ptr(), self.tri.ptr, self.toff.ptr, s)
            else:
                f.color_transfer()
        self.torch.cuda.synchronize()
        assert self.tri.intact() and self.toff.intact(), "the merge wrote outside the caller's triangle buffers"
        return self

    def triangles(self, k):
        toff = self.toff.body().view(self.torch.int32).view(self.T, self.n + 1).cpu().numpy()
        tri = self.tri.body().view(self.torch.int32).view(self.T, 2 * self.cap, 3)
        assert toff[k, 0] == 0 and (np.diff(toff[k]) >= 0).all() and toff[k, -1] <= 2 * self.cap, toff[k]
        return tri[k, :int(toff[k, -1])].cpu().numpy()

    def check_tick(self, k, tris, diag, what):
        got = self.triangles(k)
        assert got.shape == tris.shape and np.array_equal(got, tris), (what, got.shape, tris.shape)
        off = self.fus.host_offsets()[k]
        assert np.array_equal(off, diag["offsets"]), what
        d = self.fus.plan.overlay_diagnostics(k, int(off[-1]))
        assert np.array_equal(d["reprojected"], diag["reprojected"]), what
        assert np.array_equal(d["merged"], diag["merged"]), what
        assert np.array_equal(d["assigned"], diag["assigned"]) and d["n_assigned"] == int(diag["assigned"].sum()), what

    def close(self):
        self.fus.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


@pytest.mark.parametrize("name", cases.NAMES)
def test_device_path_equals_the_reference(gpu, orc, name):
    tris, diag = _ref(orc, name)
    with Merge([cases.rig(name)]) as m:
        m.run().check_tick(0, tris, diag, name)
        assert cases.equals_fixture(_fixture(), name, m.triangles(0)), name     # the reference's own triangles, with nothing in between
        assert int(m.fus.host_offsets()[0, -1]) == int(_fixture()[name + "/n_vertices"])


@pytest.mark.parametrize("name", cases.NAMES)
def test_host_export_equals_the_reference(gpu, orc, name):
    rig = cases.rig(name)
    plain, _, e0 = export(rig, overlay_merge=False)
    got, tris, e1 = export(rig, **MERGED)
    assert e0 == "" and e1 == "", (e0, e1)
    assert got.tobytes() == plain.tobytes()                   # the merge touches no vertex
    assert cases.equals_fixture(_fixture(), name, tris)
    assert np.array_equal(tris, _ref(orc, name)[0])


@pytest.mark.parametrize("name", ("zero_m3_d1", "zero_m2.5_d1", "zero_roll_d3", "discard_215"))
def test_zero_writers_leave_nothing_behind_on_the_plan(gpu, orc, name):
    """The zero_val rig twice on one plan, then a rig without zero writers on that plan: mg_resolve_kernel puts zmax and key back."""
    with Merge([cases.rig(name)]) as m:
        for again in range(2):
            m.run().check_tick(0, *_ref(orc, name), (name, again))
        for plain in ("shared_m3", "thresholds"):
            m.load([cases.rig(plain)], params=True)
            m.run().check_tick(0, *_ref(orc, plain), (name, "then", plain))
        m.load([cases.rig(name)], params=True)
        m.run().check_tick(0, *_ref(orc, name), (name, "at last"))


@functools.lru_cache(maxsize=None)
def _ticks():
    """Ticks of one calibration (sensor 1 magnifies sensor 0 by 3, both at the origin): the zero_m3 rigs between rigs without a zero writer."""
    plain = [cases.shared_edges(3.0, (cases.W // 2, cases.H // 2), seed) for seed in (31, 32, 33)]
    z = [cases.rig(n) for n in ("zero_m3_d1", "zero_m3_d2", "zero_m3_d3")]
    ticks = [z[0], plain[0], z[1], z[2], plain[1], z[0], plain[2], z[1], plain[0]]
    for r in ticks:
        assert np.array_equal(r.intr, ticks[0].intr) and np.array_equal(r.wt, ticks[0].wt) and np.array_equal(r.bounds, ticks[0].bounds)
    return ticks, plain


def test_ticks_of_one_plan_with_zero_writers_between_plain_ones(gpu, orc):
    """blockIdx.y strides, the per-tick toff and the per-tick scratch slots, crossed with live zmax: every tick equals the reference and
    its single-tick run."""
    ticks, plain = _ticks()
    for r in plain:
        t = {}
        merge_ref.overlay_merge(r, orc, trace=t)
        assert sum(np.bincount(d["classes"].ravel(), minlength=6) for d in t["draw"])[merge_ref.ZERO_THEN_LATER:].sum() == 0
    with Merge(ticks) as m:
        m.run()
        for k, r in enumerate(ticks):
            m.check_tick(k, *_ref(orc, r), k)
        batch = [m.triangles(k) for k in range(len(ticks))]
    for k in (0, 1, 3):
        with Merge([ticks[k]]) as one:
            assert np.array_equal(one.run().triangles(0), batch[k]), k


def test_ticks_whose_zero_writers_discard_an_earlier_smaller_val(gpu, orc):
    """The discard_* rigs (one calibration) as the ticks of one plan: at their named pixels mg_raster_kernel<1>'s t > zmax filter keeps
    out a NON-zero writer that would otherwise win, and the merged map depends on it (test_census_discarded_smaller_val)."""
    ticks = [cases.rig(n) for n in ("discard_215", "discard_24", "discard_215")]
    assert all(np.array_equal(r.intr, ticks[0].intr) and np.array_equal(r.wt, ticks[0].wt) for r in ticks)
    with Merge(ticks) as m:
        m.run()
        for k, r in enumerate(ticks):
            m.check_tick(k, *_ref(orc, r), k)


def test_merge_and_colour_in_both_orders_with_zero_writers(gpu, orc):
    name = "zero_m3_d2"
    rig = cases.rig(name)
    tris, diag = _ref(orc, name)
    cwant, _ = color_ref.color_transfer(rig, orc)
    with Merge([rig]) as a, Merge([rig]) as b:
        a.run(("merge", "color"))
        b.run(("color", "merge"))
        va, vb = a.fus.vertices.cpu().numpy(), b.fus.vertices.cpu().numpy()
        a.check_tick(0, tris, diag, "merge, colour")
        b.check_tick(0, tris, diag, "colour, merge")
    assert va.tobytes() == vb.tobytes() and va[0, :len(cwant)].tobytes() == cwant.tobytes()
    got, t, err = export(rig, color_transfer=True, **MERGED)
    assert err == "" and got.tobytes() == cwant.tobytes() and np.array_equal(t, tris)


def test_render_and_merge_draw_the_same_triangles_alike(gpu, orc):
    """raster.hip's set-up, fill rule and value arithmetic (the render stage) and merge.hip's written-out copy: the projected triangles
    the trace recorded for the magnified draws of the shared_* rigs -- shared edges and vertices through pixel centres, no zero writer --
    rendered as a mesh of their own.  Coverage and depth equal merge_ref.draw's, which the merge is held to above through its outputs."""
    import torch
    intr = render_ref.intrinsics(cases.W, cases.H)
    draws = []
    for name in ("shared_m3", "shared_m2"):
        t = {}
        merge_ref.overlay_merge(cases.rig(name), orc, trace=t)
        (d,) = [d for d in t["draw"] if d["b"] == 1]
        assert len(d["tris"]) > 500 and (d["classes"] >= merge_ref.ZERO_THEN_LATER).sum() == 0
        draws.append(d)
    c = Clouds(torch, [render_ref.soup(d["tris"], intr) for d in draws], (128, 106))     # (room for three vertices per triangle)
    depth, _, _ = c.check(intr, render_ref.IDENTITY, cases.W, cases.H)
    for k, d in enumerate(draws):
        want, _ = merge_ref.draw(d["tris"], d["tags"], cases.W, cases.H)
        assert np.array_equal(depth[k, 0] != 0, d["classes"] != merge_ref.NEVER) and np.array_equal(depth[k, 0], want), k
    c.close()


def test_more_than_32_sensors_are_refused(gpu):
    """33 sensors of 8 x 8: an error that names the limit, and no byte of any output touched."""
    import torch
    n, w, h = 33, 8, 8
    rng = np.random.default_rng(33)
    plan = native.FusionPlan(0, 1, [w] * n, [h] * n)
    intr = np.tile(np.float32([w / 2, h / 2, 50, 50, 0, 0, 0]), n)
    wt = np.tile(np.float32([0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1]), n)
    plan.set_params(intr, wt, cases.HUGE_BOUNDS)
    cap = plan.capacity
    depth = torch.from_numpy(rng.integers(1400, 1600, n * w * h).astype(np.int16)).cuda()
    bufs = [Guarded(torch, nbytes, "cuda") for nbytes in (16 * cap, 4 * (n + 1), 24 * cap, 4 * (n + 1))]   # vertices, offsets, triangles, their offsets
    with pytest.raises(native.NativeUtilsError, match=r"at most 32 sensors \(the plan has 33\)"):
        plan.overlay_merge(depth.data_ptr(), *[b.ptr for b in bufs], 0)
    torch.cuda.synchronize()
    for b in bufs:
        assert b.intact() and bool((b.body() == PATTERN).all().item())
    plan.close()
