"""lsnFusionColorBlend (csrc/color_blend.hip) through DeviceFusion.color_blend on the hand-made rigs of tests/color_blend_cases.py,
against the definition (tests/color_blend_ref.py).  Bit for bit: the vertex bytes and the three counters per sensor; nothing here has a
tolerance.  The vertex buffer lies between guard bands; what lies behind a tick's vertices, the offsets and the triangles must stay as
they were.  tests/test_color_blend_ref.py holds the rigs to what they claim to reach and to the mutants they kill, without a GPU."""
import numpy as np
import pytest

from livescan3d_amd import native
from tests import color_blend_cases as cases, color_blend_ref as ref
from tests.support import PATTERN, Guarded

pytestmark = pytest.mark.gpu

_refs = {}


def _ref(orc, name, again=False):
    """Per tick of a case the definition's (vertices, diagnostics) -- again: of a second blend on the first one's output.  Computed once,
    never changed."""
    if (name, again) not in _refs:
        c, out = cases.case(name), []
        for k, rig in enumerate(c.ticks):
            v, d = ref.blend(rig, orc, c.tol, c.minc, verts=_ref(orc, name)[k][0] if again else cases.start(c, k, orc))
            for a in (v, *d.values()):
                a.setflags(write=False)
            out.append((v, d))
        _refs[(name, again)] = out
    return _refs[(name, again)]


class Blend:
    """A plan of a case's ticks whose vertex buffer lies between guard bands: run_mesh, what the case runs in front, then the blend."""

    def __init__(self, c):
        import torch
        from livescan3d_amd.fusion import DeviceFusion
        self.torch, self.c = torch, c
        self.fus = DeviceFusion.from_rigs(c.ticks)
        self.T, self.cap = self.fus.n_ticks, self.fus.capacity
        self.guard = Guarded(torch, self.T * self.cap * 16, self.fus.device)
        self.fus.vertices = self.guard.body().view(self.T, self.cap, 16)

    def fuse(self):
        self.guard.body().fill_(PATTERN)
        self.fus.run_mesh()
        if self.c.pre == "transfer":
            self.fus.color_transfer()
        elif self.c.pre == "alpha":
            n = int(self.fus.host_offsets()[0, -1])
            self.fus.vertices[0, :n, 3] = self.torch.from_numpy(cases.alpha_pattern(n)).to(self.fus.device)
        return self

    def blend(self, stream=None):
        self.torch.cuda.synchronize()
        self.before = (self.fus.vertices.clone(), self.fus.offsets.clone(), self.fus.triangles.clone(), self.fus.tri_offsets.clone())
        self.fus.color_blend(self.c.tol, self.c.minc, stream=stream)
        self.torch.cuda.synchronize()
        assert self.guard.intact(), "the blend wrote outside the vertex buffer"
        return self

    def check(self, want, what):
        for now, was in zip((self.fus.offsets, self.fus.triangles, self.fus.tri_offsets), self.before[1:]):
            assert bool((now == was).all().item()), (what, "offsets or triangles were written")
        for k, (v, d) in enumerate(want):
            n = int(self.fus.host_offsets()[k, -1])
            slot, before = self.fus.vertices[k].cpu().numpy(), self.before[0][k].cpu().numpy()
            assert slot[:n].tobytes() == v.tobytes(), (what, k, n, len(v))
            assert slot[:n, 3:].tobytes() == before[:n, 3:].tobytes() and slot[n:].tobytes() == before[n:].tobytes(), (what, k, "A, XYZ or bytes behind the vertices")
            got = self.fus.color_blend_diagnostics(k)
            for key in ("blended", "partners", "abs_change"):
                assert got[key].dtype == d[key].dtype and np.array_equal(got[key], d[key]), (what, k, key, got[key].tolist(), d[key].tolist())
            assert got["n_blended"] == int(d["blended"].sum())

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.fus.close()


@pytest.mark.parametrize("name", cases.NAMES)
def test_case_equals_the_definition(gpu, orc, name):
    with Blend(cases.case(name)) as b:
        b.fuse().blend().check(_ref(orc, name), name)


@pytest.mark.parametrize("name", ("jacobi", "two_ticks"))
def test_on_a_stream_of_its_own(gpu, orc, name):
    import torch
    s = torch.cuda.Stream()
    with Blend(cases.case(name)) as b:
        b.fuse()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            b.blend(stream=s)
        b.check(_ref(orc, name), name)


@pytest.mark.parametrize("name", ("conf_edge", "proj_shift", "mixed"))
def test_twice(gpu, orc, name):
    """The second call blends the first call's output: its snapshot is taken when IT starts, and its counters replace the first's."""
    first, second = _ref(orc, name), _ref(orc, name, again=True)
    assert first[0][0].tobytes() != second[0][0].tobytes()
    with Blend(cases.case(name)) as b:
        b.fuse().blend().check(first, name)
        b.blend().check(second, (name, "again"))


def test_a_call_that_is_off_leaves_zero_counters(gpu, orc):
    c = cases.case("jacobi")
    with Blend(c) as b:
        b.fuse().blend().check(_ref(orc, "jacobi"), "jacobi")
        after = b.fus.vertices.clone()
        b.fus.color_blend(0, c.minc)
        d = b.fus.color_blend_diagnostics(0)
        assert d["n_blended"] == 0 and not d["partners"].any() and not d["abs_change"].any()
        assert bool((b.fus.vertices == after).all().item()) and b.guard.intact()


def test_diagnostics_before_the_first_blend_are_refused(gpu):
    with Blend(cases.case("three")) as b:
        b.fuse()
        with pytest.raises(native.NativeUtilsError, match="lsnFusionColorBlendDiagnostics: no colour blend has run on this plan"):
            b.fus.color_blend_diagnostics(0)
        b.blend()
        with pytest.raises(native.NativeUtilsError, match=r"the plan has 1 ticks \(asked for tick 1\)"):
            b.fus.color_blend_diagnostics(1)


def test_33_sensors_are_refused(gpu):
    """-1 with a message that names the limit, and no byte of the vertices touched."""
    with Blend(cases.Case([cases.rig33()])) as b:
        b.fuse()
        b.torch.cuda.synchronize()
        before = b.guard.buf.clone()
        with pytest.raises(native.NativeUtilsError, match=r"lsnFusionColorBlend: at most 32 sensors \(the plan has 33\)"):
            b.fus.color_blend(15, 1)
        b.torch.cuda.synchronize()
        assert bool((b.guard.buf == before).all().item()) and b.guard.intact()
