"""lsnIcpPointToPlane: ICP's flow on host arrays with the point-to-plane residual equals lsnIcpRunPlane on the same data bit for bit; bad
arguments fail, a run of no iterations succeeds, and either leaves the caller's arrays as they were."""
import ctypes as C

import numpy as np
import pytest

from livescan3d_amd import native
from tests import icp_plane_cases as cases

pytestmark = pytest.mark.gpu

F32 = np.float32
START = (cases.START_R, cases.START_T)
_bits, _run = cases.bits, cases.run_device


@pytest.mark.parametrize("name", ["chain", "zero_normals", "single_wall"])
def test_host_export_returns_the_device_runs_bits(gpu, orc, name):
    c = cases.get(name, orc)
    v, R, t, _ = _run(c, c.iters, native.NN_GRID, START)
    before = [np.array(a) for a in (c.tgt, c.nrm, c.src)]
    hv, hR, ht = native.icp_point_to_plane(c.tgt, c.nrm, c.src, R=cases.START_R, t=cases.START_T, max_iter=c.iters)
    assert np.array_equal(_bits(hv), _bits(v)) and np.array_equal(_bits(hR), _bits(R)) and np.array_equal(_bits(ht), _bits(t))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(before, (c.tgt, c.nrm, c.src)))      # read only
    assert not np.array_equal(_bits(hv), _bits(c.src))


def test_brute_force_nn_through_the_environment(gpu, orc, monkeypatch):
    c = cases.get("corner", orc)
    grid = native.icp_point_to_plane(c.tgt, c.nrm, c.src, max_iter=2)
    monkeypatch.setenv("LSN_NN", "brute")
    brute = native.icp_point_to_plane(c.tgt, c.nrm, c.src, max_iter=2)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(grid, brute))


def test_bad_arguments_touch_nothing(gpu, orc):
    c = cases.get("block_edges_65", orc)
    L = native.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    tgt, nrm = np.array(c.tgt), np.array(c.nrm)

    def call(v1, n1, v2, c1, c2, R, t, iters):
        native.lib().lsnIcpPointToPlane(None, None, None, 0, 0, None, None, 0)      # leaves a message behind: the next call must clear or replace it
        return L.lsnIcpPointToPlane(v1, n1, v2, c1, c2, R, t, iters), native.last_error()

    def fresh():
        return np.array(c.src), np.array(cases.START_R).reshape(-1), np.array(cases.START_T)

    def untouched(src, R, t):
        return np.array_equal(_bits(src), _bits(c.src)) and np.array_equal(_bits(R), _bits(cases.START_R).reshape(-1)) and np.array_equal(_bits(t), _bits(cases.START_T))

    n1, n2 = len(tgt), len(c.src)
    for bad in ("verts1", "normals1", "verts2", "R", "t", "nVerts1", "nVerts2", "negative"):
        src, R, t = fresh()
        args = dict(v1=p(tgt), n1=p(nrm), v2=p(src), c1=n1, c2=n2, R=p(R), t=p(t), iters=3)
        args.update({"verts1": dict(v1=None), "normals1": dict(n1=None), "verts2": dict(v2=None), "R": dict(R=None), "t": dict(t=None),
                     "nVerts1": dict(c1=0), "nVerts2": dict(c2=0), "negative": dict(c1=-5)}[bad])
        rc, err = call(**args)
        assert rc == -1 and "lsnIcpPointToPlane" in err, (bad, rc, err)
        assert untouched(src, R, t), bad
    for iters in (0, -3):                                   # nothing to do: success, no message, nothing written
        src, R, t = fresh()
        rc, err = call(p(tgt), p(nrm), p(src), n1, n2, p(R), p(t), iters)
        assert rc == 0 and not err, (iters, rc, err)
        assert untouched(src, R, t), iters
    src, R, t = fresh()                                     # and the call works on these very arrays
    rc, err = call(p(tgt), p(nrm), p(src), n1, n2, p(R), p(t), 1)
    assert rc == 0 and not err and not untouched(src, R, t)
