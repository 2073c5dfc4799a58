"""What the tests of the vertex-normals stage share (test infrastructure): the hand-made meshes, one for every rule of the definition, and
the device check -- lsnFusionNormals into a guarded, prefilled buffer against tests/normals_ref.py, bit for bit.  torch is handed in by
the GPU tests; nothing here imports it."""
import numpy as np

from livescan3d_amd import native
from tests import normals_ref
from tests.simplify_cases import PREFILL, Clouds   # the upload of hand-made ticks (garbage behind the counts) is the simplifier's
from tests.simplify_ref import cloud
from tests.support import Guarded

BELOW_4096 = float(np.nextafter(np.float32(4096.0), np.float32(0.0)))     # the largest float32 below 4096: 4096 - 2^-12


class Builder:
    """A mesh around hubs at the origin: inject(hub, axis, a, b) adds one triangle (hub, s1, s2) whose face vector is a * b along `axis`
    and 0 elsewhere (a, b exact in float32; the satellites are shared between triangles by position, and get the same sums)."""

    def __init__(self):
        self.xyz, self.tri, self.at = [], [], {}

    def vertex(self, *p):
        self.xyz.append([float(c) for c in p])
        return len(self.xyz) - 1

    def shared(self, *p):
        if p not in self.at:
            self.at[p] = self.vertex(*p)
        return self.at[p]

    def inject(self, hub, axis, a, b):
        # f = (p2 - p0) x (p1 - p0) with p0 = 0: z: p2 = (a, 0, 0), p1 = (0, b, 0); x: p2 = (0, a, 0), p1 = (0, 0, b); y: p2 = (0, 0, a), p1 = (b, 0, 0)
        e = np.eye(3)
        p2, p1 = a * e[(axis + 1) % 3], b * e[(axis + 2) % 3]
        self.tri.append([hub, self.shared(*p1), self.shared(*p2)])

    def mesh(self):
        return np.asarray(self.xyz, np.float32), np.asarray(self.tri, np.int32)


def rounding_mesh():
    """Hubs whose z sums need rounding on the way to float32, each with a second component so that the rounding shows in the normal:
    -> (xyz, triangles, {hub: expected (Sx, Sy, Sz)}).  2^25 + 1 (down), + 2 (a tie, to even: down), + 6 (a tie, to even: up), + 3 (up),
    and 4 x (2^52 - 2^28) + 1 > 2^53."""
    b = Builder()
    X, Y, Z = 0, 1, 2
    big = int(np.float32(BELOW_4096) * np.float32(2.0 ** 40))
    want = {}
    for low, (axis, k) in ((1, (X, 3)), (2, (X, 5)), (6, (X, 7)), (3, (Y, -3))):
        h = b.vertex(0, 0, 0)
        b.inject(h, Z, 2.0 ** -7, 2.0 ** -8)                    # q = 2^25
        for bit in range(3):
            if low >> bit & 1:
                b.inject(h, Z, 2.0 ** -20, 2.0 ** (bit - 20))   # q = 2^bit
        b.inject(h, axis, 2.0 ** -10, k * 2.0 ** -10)           # q = k 2^20
        s = [0, 0, 2 ** 25 + low]
        s[axis] = k * 2 ** 20
        want[h] = tuple(s)
    h = b.vertex(0, 0, 0)
    for _ in range(4):
        b.inject(h, Z, 1.0, BELOW_4096)
    b.inject(h, Z, 2.0 ** -20, 2.0 ** -20)
    b.inject(h, X, 64.0, 32.0)                                  # q = 2^51
    want[h] = (2 ** 51, 0, 4 * big + 1)
    xyz, tri = b.mesh()
    return xyz, tri, want


def cases():
    """name -> (xyz float32 [n, 3], offsets row, triangles int32 [m, 3], tri_offsets row): the hand-made meshes of one 8 x 8 sensor
    (at most 64 vertices, 128 triangles), shared with the GPU test."""
    nan, inf = np.nan, np.inf
    c = {}
    c["one_triangle"] = ([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]])
    c["reversed"] = ([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 2, 1]])
    # 0-2: a good triangle, alone in carrying sums; bad indices (-1, nVertices = 21, 2^30); 3-5 with a NaN, 6-8 with an infinite coordinate;
    # 9-11: fz = 64 x 64 = 4096 exactly (skipped); 12-14: fz = 1 x (4096 - 2^-12) (used); 15-17 collinear, and a repeated index (used, zeros);
    # 18-20: fz = -4096 (skipped)
    xyz = [[0, 0, 0], [0, 0.5, 0.25], [0.5, 0, 0.125], [0, 0, 0], [nan, 1, 0], [1, 0, 0], [0, 0, 0], [0, 1, 0], [1, inf, 0],
           [0, 0, 0], [0, 64, 0], [64, 0, 0], [0, 0, 0], [0, BELOW_4096, 0], [1, 0, 0], [1, 1, 1], [2, 2, 2], [4, 4, 4],
           [0, 0, 0], [64, 0, 0], [0, 64, 0]]
    tris = [[0, 1, 2], [-1, 1, 2], [0, 21, 2], [0, 1, 2 ** 30], [3, 4, 5], [6, 7, 8], [9, 10, 11], [12, 13, 14], [15, 16, 17], [15, 15, 16],
            [1, 1, 1], [18, 19, 20]]
    c["skipped_and_degenerate"] = (xyz, tris)
    c["cancelling_pair"] = ([[0, 0, 0], [0.3, 0.1, 0.7], [0.2, 0.9, 0.4]], [[0, 1, 2], [0, 2, 1]])
    xyz, tris, _ = rounding_mesh()
    c["rounding"] = (xyz, tris)
    # every add of 126 triangles on vertex 0: a hub and 63 rim vertices on a tilted circle
    k = np.arange(63)
    rim = np.stack([np.cos(k * 0.1) * (1 + 0.01 * k), np.sin(k * 0.1) * (1 + 0.01 * k), 0.3 * np.cos(k * 0.37)], axis=1) + [0.1, -0.2, 0.05]
    fan = [[0, 1 + i, 1 + (i + 1) % 63] for i in range(63)] + [[0, 1 + i, 1 + (i + 2) % 63] for i in range(63)]
    c["fan"] = (np.concatenate([[[0.1, -0.2, 0.9]], rim]), fan)
    out = {}
    for name, (x, t) in c.items():
        x, t = np.asarray(x, np.float32).reshape(-1, 3), np.asarray(t, np.int32).reshape(-1, 3)
        assert len(x) <= 64 and len(t) <= 128, name
        out[name] = (x, np.array([0, len(x)], np.int32), t, np.array([0, len(t)], np.int32))
    return out


def wrap_mesh(n=2100):
    """More than 2048 triangles of the largest face vector below 4096 on one hub (and on their two shared satellites), one more along x:
    the z sums pass 2^63 and wrap.  -> (xyz, triangles)."""
    b = Builder()
    h = b.vertex(0, 0, 0)
    for _ in range(n):
        b.inject(h, 2, 1.0, BELOW_4096)
    b.inject(h, 0, 1.0, 1.0)
    return b.mesh()


def tick(name):
    """A case as simplify_cases.Clouds takes a tick: (vertices VERTEX_DTYPE, offsets row, triangles, tri_offsets row)."""
    xyz, off, tri, toff = cases()[name]
    return cloud(xyz), off, tri, toff


def restate(v, off, tri, toff, T, cap):
    """The restatement on every tick of host copies of a device batch (v uint8 [T, cap, 16])."""
    return [normals_ref.normals(np.ascontiguousarray(v[k]).view(native.VERTEX_DTYPE).reshape(-1), off[k], tri[k], toff[k], cap, 2 * cap)
            for k in range(T)]


def check_device(torch, plan, v, off, tri, toff, out=None, refs=None):
    """plan.normals on the device tensors v [T, cap, 16] u8, off [T, n + 1] i32, tri [T, 2 cap, 3] i32, toff [T, n + 1] i32 into a
    guarded buffer prefilled with PREFILL (a fresh one unless `out` is handed in); every tick against the restatement (computed here
    unless `refs` is handed in): the normals byte for byte, the diagnostics' three counts equal, the guard bands intact, nothing behind
    nVertices written.  Returns (the Guarded output, the restatement's dict per tick)."""
    T, cap = int(v.shape[0]), int(v.shape[1])
    assert cap == plan.capacity and T == plan.n_ticks
    if out is None:
        out = Guarded(torch, T * cap * 12, "cuda")
        out.body().fill_(PREFILL)
    plan.normals(v.data_ptr(), off.data_ptr(), tri.data_ptr(), toff.data_ptr(), out.ptr)
    torch.cuda.synchronize()
    assert out.intact()
    got = out.body().cpu().numpy().reshape(T, cap, 12)
    if refs is None:
        refs = restate(v.cpu().numpy().reshape(T, cap, 16), off.cpu().numpy(), tri.cpu().numpy(), toff.cpu().numpy(), T, cap)
    for k, r in enumerate(refs):
        nv = len(r["normals"])
        want = np.ascontiguousarray(r["normals"]).view(np.uint8).reshape(nv, 12)
        bad = (got[k, :nv] != want).any(axis=1)
        assert not bad.any(), (k, "normals", int(bad.sum()), got[k, :nv][bad][:3].view(np.float32), r["normals"][bad][:3], r["sums"][bad][:3])
        assert (got[k, nv:] == PREFILL).all(), (k, "written behind nVertices")
        d = plan.normals_diagnostics(k)
        assert d == {"used": r["used"], "skipped": r["skipped"], "zero_normals": r["zero_normals"]}, (k, d, r["used"], r["skipped"], r["zero_normals"])
    return out, refs
