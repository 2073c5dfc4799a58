"""What only the tests need and several of them share: the seeded ring-rig fuzzer, the guard-band allocation, the merge export with its
error message, the child-process runner, hand-made clouds as the ticks of a plan for the render stage.  (The device batch itself is livescan3d_amd.fusion.DeviceFusion; torch is imported by the GPU
tests alone, so nothing here imports it.)"""
import os
import subprocess
import sys

import numpy as np

from livescan3d_amd import native, synth
from tests import color_cases, merge_cases, render_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUT_BOUNDS = np.array([-0.3, -1.0, -1.5, 1.5, 1.5, 1.5], dtype=np.float32)   # through the sphere, inside the views' overlap

GUARD = 4096
PATTERN = 0xA5


class Guarded:
    """`nbytes` of device memory with GUARD pattern bytes either side."""

    def __init__(self, torch, nbytes, dev):
        self.torch, self.n = torch, int(nbytes)
        self.buf = torch.full((GUARD + self.n + GUARD,), PATTERN, dtype=torch.uint8, device=dev)

    @property
    def ptr(self):
        return self.buf.data_ptr() + GUARD

    def body(self):
        return self.buf[GUARD:GUARD + self.n]

    def intact(self):
        return bool((self.buf[:GUARD] == PATTERN).all().item()) and bool((self.buf[GUARD + self.n:] == PATTERN).all().item())


def export(rig, **flags):
    """generateMeshFromDepthMaps with native.generate_mesh_from_depth_maps' flags.  Returns (vertices, triangles, last error message)."""
    v, t = native.generate_mesh_from_depth_maps(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds, **flags)
    return v, t, native.last_error()


def child(code, env_extra, *args, drop=(), timeout=300):
    """`code` (with sys.argv[1:] = args) in a fresh Python process started in the repository root, its environment this one's without the
    variables of `drop` and with env_extra.  It must exit with 0.  Returns (last line of its stdout, its stderr)."""
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", code, *map(str, args)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.strip().splitlines()[-1], r.stderr


def ragged_or_equal(max_w, max_h, widths, heights):
    """sizes(rng, n) for ring_rig: in half of the cases every sensor its own size below (max_w, max_h), else one size out of widths x heights."""
    def sizes(rng, n):
        if rng.random() < 0.5:
            return [(int(rng.integers(1, max_w)), int(rng.integers(1, max_h))) for _ in range(n)]
        w, h = int(rng.choice(widths)), int(rng.choice(heights))
        return [(w, h)] * n
    return sizes


def one_of(pairs):
    """sizes(rng, n) for ring_rig: one of `pairs` for all sensors."""
    return lambda rng, n: [pairs[int(rng.integers(0, len(pairs)))]] * n


def ring_rig(rng, max_n, densities, sizes, wall=None):
    """One random rig of the colour / outlier / merge fuzzers: 1..max_n sensors on a ring of n or one of `densities` positions, sizes(rng, n)
    their frame sizes, a random crop box in 70 % of the cases, every sensor moved out of the others' view with probability 0.15.
    wall = None: the density is drawn before the sizes.  wall = p: the sizes come first and with probability p the rig is a
    merge_cases.wall of the first size instead.  (The order of the draws is part of the fuzzers' cases: a seed names the same rig as ever.)"""
    n = int(rng.integers(1, max_n + 1))
    if wall is None:
        of = max(n, int(rng.choice([n] + densities)))
        sz = sizes(rng, n)
    else:
        sz = sizes(rng, n)
        if rng.random() < wall:
            return merge_cases.wall(n, *sz[0], seed=int(rng.integers(1, 1000)), step_deg=float(rng.uniform(0.0, 10.0)), tick=int(rng.integers(0, 5)))
        of = max(n, int(rng.choice([n] + densities)))
    lo, hi = rng.uniform(-1.6, -0.2, 3), rng.uniform(0.2, 1.6, 3)
    bounds = np.concatenate([lo, hi]).astype(np.float32) if rng.random() < 0.7 else color_cases.WIDE_BOUNDS
    poses = []
    for s in range(n):
        R, t = synth.ring_pose(s, of)
        if rng.random() < 0.15:   # this sensor's world is elsewhere
            t = t + R.T @ np.array([float(rng.uniform(5, 50)), 0.0, 0.0])
        poses.append((R, t))
    return color_cases.ring(n, sizes=sz, bounds=bounds, seed=int(rng.integers(1, 1000)), tick=int(rng.integers(0, 5)), poses=poses, of=of)


CLOUDS_PREFILL = 249   # -7 as a byte: what DeviceFusion prefills its tables with


class Clouds:
    """A plan of one `size` sensor per tick with hand-made clouds uploaded as its ticks: clouds[k] = (vertices, triangles or None).
    vertex_fill: the byte that lies behind every tick's vertices (never read)."""

    def __init__(self, torch, clouds, size=(64, 48), vertex_fill=0):
        self.torch, self.clouds, self.T = torch, clouds, len(clouds)
        self.plan = native.FusionPlan(0, self.T, [size[0]], [size[1]])
        cap = self.cap = self.plan.capacity
        v = np.full((self.T, cap, 16), vertex_fill, np.uint8)
        t = np.full((self.T, 2 * cap, 3), -3, np.int32)     # what lies behind a tick's triangles is never read
        off, toff = np.zeros((self.T, 2), np.int32), np.zeros((self.T, 2), np.int32)
        for k, (cv, ct) in enumerate(clouds):
            assert len(cv) <= cap and (ct is None or len(ct) <= 2 * cap)
            v[k, :len(cv)] = np.frombuffer(cv.tobytes(), np.uint8).reshape(-1, 16)
            off[k, 1] = len(cv)
            if ct is not None:
                t[k, :len(ct)] = ct
                toff[k, 1] = len(ct)
        self.v, self.t, self.off, self.toff = (torch.from_numpy(a).cuda() for a in (v, t, off, toff))

    def render(self, intr, wt, w, h, points=False):
        """-> (depth u16 [T, V, h, w], rgb u8 [T, V, h, w, 3]) between guard bands, prefilled."""
        V = np.asarray(intr).size // 7
        gd, gc = Guarded(self.torch, self.T * V * w * h * 2, "cuda"), Guarded(self.torch, self.T * V * w * h * 3, "cuda")
        gd.body().fill_(CLOUDS_PREFILL)
        gc.body().fill_(CLOUDS_PREFILL)
        self.plan.render_views(intr, wt, w, h, self.v.data_ptr(), self.off.data_ptr(), 0 if points else self.t.data_ptr(),
                               0 if points else self.toff.data_ptr(), gd.ptr, gc.ptr)
        self.torch.cuda.synchronize()
        assert gd.intact() and gc.intact()
        return (gd.body().cpu().numpy().view(np.uint16).reshape(self.T, V, h, w), gc.body().cpu().numpy().reshape(self.T, V, h, w, 3))

    def check(self, intr, wt, w, h, points=False, refs=None):
        """Renders and compares with render_ref.render, tick by tick and view by view (every view its own 7 + 12 floats).  refs: a list of
        the restatement's (depth, rgb, info) in that order, computed elsewhere."""
        depth, rgb = self.render(intr, wt, w, h, points)
        intr, wt = np.asarray(intr, np.float32).reshape(-1, 7), np.asarray(wt, np.float32).reshape(-1, 12)
        diags = []
        for k, (cv, ct) in enumerate(self.clouds):
            for q in range(len(intr)):
                if refs is not None:
                    wd, wc, info = refs[len(diags)]
                else:
                    wd, wc, info = render_ref.render(cv, None if points else (np.zeros((0, 3), np.int32) if ct is None else ct), intr[q], wt[q], w, h)
                assert np.array_equal(depth[k, q], wd), (k, q, int((depth[k, q] != wd).sum()))
                assert np.array_equal(rgb[k, q], wc), (k, q, int((rgb[k, q] != wc).any(axis=-1).sum()))
                d = self.plan.render_diagnostics(k, q)
                assert d["drawn"] == info["drawn"] and d["pixels"] == info["pixels"], (k, q, d, info)
                diags.append(d)
        return depth, rgb, diags

    def close(self):
        self.plan.close()
