"""What the tests of the mesh-smoothing stage share (test infrastructure): the hand-made meshes, each with a witness that it reaches what
it is named for, and the device check -- lsnFusionSmooth into a guarded, prefilled buffer against tests/smooth_ref.py, bit for bit.
torch is handed in by the GPU tests; nothing here imports it."""
from collections import Counter

import numpy as np

from livescan3d_amd import native
from tests import smooth_ref
from tests.simplify_cases import PREFILL, Clouds   # noqa: F401  (the upload of hand-made ticks is the simplifier's)
from tests.simplify_ref import cloud
from tests.support import Guarded

TAUBIN = (10, 0.5, -0.53)                          # the documented defaults
BELOW_4096 = float(np.nextafter(np.float32(4096.0), np.float32(0.0)))


def closed_fan(k, hub=0, first=1):
    return [[hub, first + i, first + (i + 1) % k] for i in range(k)]


def open_fan(k, hub=0, first=1):
    """k triangles over k + 1 rim vertices."""
    return [[hub, first + i, first + i + 1] for i in range(k)]


def ring_xyz(k, r=1.0, z=0.0, centre=(0.0, 0.0, 0.3), wobble=0.07):
    """A hub above a wobbling circle of k rim vertices, off centre (so that no mean is 0 by symmetry)."""
    a = 2 * np.pi * np.arange(k) / k
    rim = np.stack([r * np.cos(a) * (1 + wobble * np.sin(3 * a)), r * np.sin(a) * (1 - wobble * np.cos(2 * a)), z + wobble * np.sin(5 * a)], axis=1) + [0.2, -0.1, 0.05]
    return np.concatenate([[centre], rim])


def exact_open(tri, nv):
    """The exact rule the hash stands for: per vertex the multiset of next neighbours against the multiset of previous ones, over the
    triangles that are in range and pairwise distinct.  -> bool [nv]."""
    nxt, prv = [Counter() for _ in range(nv)], [Counter() for _ in range(nv)]
    for t in np.asarray(tri, np.int64).reshape(-1, 3).tolist():
        if all(0 <= i < nv for i in t) and len(set(t)) == 3:
            for k in range(3):
                nxt[t[k]][t[(k + 1) % 3]] += 1
                prv[t[k]][t[(k + 2) % 3]] += 1
    return np.array([nxt[a] != prv[a] for a in range(nv)], bool)


class Case:
    """One hand-made mesh with its parameters; witness(o, case): asserts on the restatement's result o that the case reaches its point."""

    def __init__(self, xyz, tri, params=TAUBIN, pin=True, witness=None):
        self.xyz, self.tri = np.asarray(xyz, np.float32).reshape(-1, 3), np.asarray(tri, np.int32).reshape(-1, 3)
        self.iterations, self.lam, self.mu = params
        self.pin, self.witness = pin, witness

    def tick(self):
        """As simplify_cases.Clouds takes a tick."""
        return cloud(self.xyz), np.array([0, len(self.xyz)], np.int32), self.tri, np.array([0, len(self.tri)], np.int32)

    def run(self, mutant=None, **kw):
        a = dict(iterations=self.iterations, lam=self.lam, mu=self.mu, pin_boundary=self.pin)
        a.update(kw)
        v, off, tri, toff = self.tick()
        return smooth_ref.smooth(v, off, tri, toff, mutant=mutant, **a)

    def moved(self, o):
        return (o["xyz"].view(np.uint32) != self.xyz.view(np.uint32)).any(axis=1)


def _w_single(o, c):
    assert o["open"].all() and o["pinned"] == 3 and not c.moved(o).any() and (o["used"], o["skipped"], o["isolated"]) == (1, 0, 0)


def _w_single_free(o, c):
    assert o["pinned"] == 0 and c.moved(o).all()


def _w_closed_fan(o, c):
    assert not o["open"][0] and o["open"][1:].all() and c.moved(o).tolist() == [True] + [False] * 8 and o["pinned"] == 8


def _w_open_fan(o, c):
    assert o["open"].all() and not c.moved(o).any()


def _w_fans_meeting(o, c):
    assert not o["open"][0] and c.moved(o)[0] and o["open"][1:].all()


def _w_fans_apart(o, c):
    assert o["open"][0] and not c.moved(o)[0] and (o["used"], o["skipped"]) == (4, 0)


def _w_bow_tie(o, c):
    assert not o["open"][0] and c.moved(o)[0] and o["open"][1:].all() and o["used"] == 9


def _w_isolated(o, c):
    assert o["isolated"] == 2 and not c.moved(o)[[9, 10]].any() and c.moved(o)[0]


def _w_bad_indices(o, c):
    # the closed fan of 5 is used; (-1, ..), (.., nVertices), (.., 2^30) and the three repeated forms are skipped, and change nothing
    assert (o["used"], o["skipped"]) == (5, 6)
    good = Case(c.xyz, c.tri[:5], (c.iterations, c.lam, c.mu), c.pin).run()
    assert good["xyz"].tobytes() == o["xyz"].tobytes() and np.array_equal(good["open"], o["open"]) and c.moved(o)[0]


def _w_non_finite(o, c):
    # three closed fans (hubs 0, 9, 18), each with one bad rim vertex: NaN, inf, 4096.0.  The two triangles at the bad vertex are skipped in
    # every pass; the hub still moves on its other six, and the bad vertex keeps its bytes
    assert (o["used"], o["skipped"]) == (18, 6) and c.moved(o)[[0, 9, 18]].all() and not c.moved(o)[[3, 12, 21]].any()
    assert not o["open"][[0, 9, 18]].any() and o["isolated"] == 3


def _w_inflates(o, c):
    # the hub ends the first iteration beyond 4096; the second skips every triangle and everything stays where the first left it
    one = c.run(iterations=1)
    assert np.abs(one["xyz"][0, 0]) > 4096 and one["used"] == 6 and (o["used"], o["skipped"], o["isolated"]) == (0, 6, 7)
    assert o["xyz"].tobytes() == one["xyz"].tobytes()


def _w_tiny(o, c):
    q = smooth_ref.quantise(c.xyz)
    assert (np.abs(c.xyz) < 2.0 ** -9).all() and (c.xyz < 0).any() and (q == 0).any() and (np.floor(c.xyz * np.float32(2.0 ** 32)) != q).any()
    assert c.moved(o).any()


def _w_big_fan(o, c):
    q = smooth_ref.quantise(c.xyz)
    S = 2 * q[2:301].sum(axis=0) + q[1] + q[301]    # the hub's sums in the first pass: the fan's two ends once, the rest twice
    assert (np.abs(S) > 2 ** 53).all() and (S % 2 == 1).all() and (S.astype(np.float64).astype(np.int64) != S).all()     # odd beyond 2^53: a tie
    assert c.moved(o)[0] and c.run(iterations=1, mu=0.0)["used"] == 300 and o["open"][0] and o["pinned"] == 0
    assert 0 < o["skipped"] < 10                    # (and by the last pass a free rim vertex has been pushed past 4096)


def _w_index_sum(o, c):
    # next {1, 4}, previous {2, 3}: the raw indices cancel (5 = 5, 17 = 13 + 4 fails only in squares; here even the squares: see cases())
    assert o["open"][0] and not c.moved(o)[0]


def cases():
    """name -> Case.  All but `fan_300` fit one 8 x 8 sensor (at most 64 vertices, 128 triangles); fan_300 needs 302 vertices."""
    nan, inf = np.nan, np.inf
    rng = np.random.default_rng(21)
    c = {}
    tri_xyz = [[0, 0, 0], [1, 0, 0.25], [0.25, 1, 0]]
    c["single_triangle"] = Case(tri_xyz, [[0, 1, 2]], witness=_w_single)
    c["single_triangle_free"] = Case(tri_xyz, [[0, 1, 2]], pin=False, witness=_w_single_free)
    c["closed_fan"] = Case(ring_xyz(8), closed_fan(8), witness=_w_closed_fan)
    c["closed_fan_free"] = Case(ring_xyz(8), closed_fan(8), pin=False, witness=lambda o, c: _all_moved(o, c))
    c["open_fan"] = Case(ring_xyz(8), open_fan(7), witness=_w_open_fan)
    # 0's fan runs 1 -> 2 -> 3 and then, in a second piece listed apart and backwards, 3 -> 4 -> 1: ends 1 and 3 coincide
    c["two_fans_meeting"] = Case(ring_xyz(4), [[0, 1, 2], [0, 2, 3], [0, 4, 1], [0, 3, 4]], witness=_w_fans_meeting)
    c["two_fans_apart"] = Case(ring_xyz(6), [[0, 1, 2], [0, 2, 3], [0, 4, 5], [0, 5, 6]], witness=_w_fans_apart)
    bow = np.concatenate([ring_xyz(4), ring_xyz(5, 0.5, 0.6)[1:]])
    c["bow_tie"] = Case(bow, closed_fan(4) + closed_fan(5, 0, 5), witness=_w_bow_tie)
    c["isolated_vertices"] = Case(np.concatenate([ring_xyz(8), [[5, 5, 5], [nan, 0, 0]]]), closed_fan(8), witness=_w_isolated)
    c["bad_indices"] = Case(ring_xyz(5), closed_fan(5) + [[-1, 1, 2], [0, 6, 2], [0, 1, 2 ** 30], [0, 0, 1], [1, 2, 1], [3, 2, 2]], witness=_w_bad_indices)
    x = np.concatenate([ring_xyz(8), ring_xyz(8) + [3, 0, 0], ring_xyz(8) + [0, 3, 0]])
    x[3, 1], x[12, 2], x[21, 0] = nan, -inf, 4096.0
    c["non_finite"] = Case(x, closed_fan(8) + closed_fan(8, 9, 10) + closed_fan(8, 18, 19), witness=_w_non_finite)
    x = ring_xyz(6) * 40 + [4000, 0, 0]
    x[0] = [4090, 0, 0]
    c["inflates_past_4096"] = Case(x, closed_fan(6), (2, 2.0 ** -10, -1.0), witness=_w_inflates)
    x = (rng.integers(-2 ** 12, 2 ** 12, (20, 3)) * 2.0 ** -35).astype(np.float32) * np.float32(1.25)      # |c| < 2^-22, many below 2^-32
    x[1] = [-1.5 * 2.0 ** -32, -2.0 ** -33, 2.0 ** -33]
    c["tiny_and_negative"] = Case(x, closed_fan(19), (3, 0.5, -0.53), pin=False, witness=_w_tiny)
    # an open fan, free: one sign per component, so that the hub's sums pass 2^53; the first rim vertex has odd q, so that they are odd
    x = rng.uniform(4094.0, BELOW_4096, (302, 3)) * [1, -1, 1]
    x[0] = [4000.25, -4000.75, 4001.5]
    x[1] = [2.0 ** -32, -3 * 2.0 ** -32, 5 * 2.0 ** -32]
    c["fan_300"] = Case(x, open_fan(300), (2, 0.5, -0.53), pin=False, witness=_w_big_fan)
    c["laplacian_mu_0"] = Case(ring_xyz(8), closed_fan(8), (4, 0.5, 0.0), pin=False, witness=lambda o, c: _all_moved(o, c))
    c["one_iteration"] = Case(ring_xyz(8), closed_fan(8), (1, 1.0, -1.0), pin=False, witness=lambda o, c: _all_moved(o, c))
    c["sixty_four_iterations"] = Case(ring_xyz(8), closed_fan(8), (64, 0.5, -0.53), pin=False, witness=lambda o, c: _all_moved(o, c))
    # vertex 0: next {1, 4}, previous {2, 3} -- 1 + 4 = 2 + 3, so the sum of raw indices cancels and only the mixed ones tell it open
    c["index_sums_cancel"] = Case(ring_xyz(4), [[0, 1, 2], [0, 4, 3]], witness=_w_index_sum)
    for name, case in c.items():
        assert name == "fan_300" or (len(case.xyz) <= 64 and len(case.tri) <= 128), name
    return c


def _all_moved(o, c):
    assert o["pinned"] == 0 and c.moved(o).all() and o["isolated"] == 0


def restate(v, off, tri, toff, T, cap, iterations, lam, mu, pin):
    """The restatement on every tick of host copies of a device batch (v uint8 [T, cap, 16])."""
    return [smooth_ref.smooth(np.ascontiguousarray(v[k]).view(native.VERTEX_DTYPE).reshape(-1), off[k], tri[k], toff[k], iterations, lam, mu, pin,
                              cap, 2 * cap) for k in range(T)]


def check_device(torch, plan, v, off, tri, toff, iterations, lam, mu, pin=True, out=None, refs=None):
    """plan.smooth on the device tensors v [T, cap, 16] u8, off [T, n + 1] i32, tri [T, 2 cap, 3] i32, toff [T, n + 1] i32 into a guarded
    buffer prefilled with PREFILL (a fresh one unless `out` is handed in); every tick against the restatement (computed here unless `refs`
    is handed in): the vertices byte for byte, the diagnostics' four counts equal, the guard bands intact, nothing behind nVertices
    written, the inputs unchanged.  Returns (the Guarded output, the restatement's dict per tick)."""
    T, cap = int(v.shape[0]), int(v.shape[1])
    assert cap == plan.capacity and T == plan.n_ticks
    if out is None:
        out = Guarded(torch, T * cap * 16, "cuda")
        out.body().fill_(PREFILL)
    v_before, tri_before = v.clone(), tri.clone()
    plan.smooth(iterations, lam, mu, pin, v.data_ptr(), off.data_ptr(), tri.data_ptr(), toff.data_ptr(), out.ptr)
    torch.cuda.synchronize()
    assert out.intact() and torch.equal(v, v_before) and torch.equal(tri, tri_before)
    got = out.body().cpu().numpy().reshape(T, cap, 16)
    if refs is None:
        refs = restate(v.cpu().numpy().reshape(T, cap, 16), off.cpu().numpy(), tri.cpu().numpy(), toff.cpu().numpy(), T, cap, iterations, lam, mu, pin)
    for k, r in enumerate(refs):
        nv = len(r["vertices"])
        want = np.frombuffer(r["vertices"].tobytes(), np.uint8).reshape(nv, 16)
        bad = (got[k, :nv] != want).any(axis=1)
        assert not bad.any(), (k, "vertices", int(bad.sum()), np.flatnonzero(bad)[:3], got[k, :nv][bad][:3, 4:].copy().view(np.float32), r["xyz"][bad][:3])
        assert (got[k, nv:] == PREFILL).all(), (k, "written behind nVertices")
        d = plan.smooth_diagnostics(k)
        assert d == {key: r[key] for key in ("used", "skipped", "pinned", "isolated")}, (k, d, {key: r[key] for key in ("used", "skipped", "pinned", "isolated")})
    return out, refs
