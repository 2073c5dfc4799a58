"""ctypes binding of libNativeUtils.so (include/NativeUtils.h).

Part 1 mirrors LiveScanServer's P/Invoke declarations (LiveScanServer/KinectServer.cs:35-60,
MainWindowForm.cs:42-43): same entry points, same array conventions.  Part 2 binds the device-resident
API; device pointers are plain integers (e.g. torch.Tensor.data_ptr()).

The library is loaded from livescan3d_amd/lib/ (built in-tree by __graft_entry__.build()).  If it is missing
or a call fails, NativeUtilsError is raised -- nothing here computes on the CPU.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# $LSN_NATIVE_LIB: another build of the same library (development A/Bs); the default is the in-tree build
LIB_PATH = os.environ.get("LSN_NATIVE_LIB") or os.path.join(_HERE, "lib", "libNativeUtils.so")

VERTEX_DTYPE = np.dtype([("R", "u1"), ("G", "u1"), ("B", "u1"), ("A", "u1"),
                         ("X", "<f4"), ("Y", "<f4"), ("Z", "<f4")])  # VertexC4ubV3f, 16 bytes

class NativeUtilsError(RuntimeError):
    pass


class Mesh(C.Structure):
    """struct Mesh (include/NativeUtils/depthprocessing.h:42-48; C# mirror Utils.cs:335-342)."""
    _fields_ = [("nVertices", C.c_int), ("vertices", C.c_void_p), ("nTriangles", C.c_int), ("triangles", C.c_void_p)]


assert C.sizeof(Mesh) == 32


class FrameInfo(C.Structure):
    """LsnFrameInfo: the 16-byte header of a frame message (KinectSocket.cs:229-239)."""
    _fields_ = [("payload_bytes", C.c_int), ("compressed", C.c_int), ("width", C.c_int), ("height", C.c_int)]


_vp, _i, _ll, _f, _b, _s = C.c_void_p, C.c_int, C.c_longlong, C.c_float, C.c_bool, C.c_char_p
_mesh = C.POINTER(Mesh)

# Every function include/NativeUtils.h declares: name -> (restype, argtypes).  This is the one place the header's types are restated
# (tests/test_abi.py holds every entry against the header); lib() declares them all in one loop.
_PROTOTYPES = {
    # part 1: the reference's exports and what belongs to them
    "generateVerticesFromDepthMap": (None, [_vp, _vp, _vp, _vp, _vp, _vp, _mesh, _f, _f, _f, _f, _f, _f, _i]),
    "generateMeshFromDepthMaps": (None, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _mesh, _b, _f, _f, _f, _f, _f, _f, _b]),
    "depthMapAndColorSetRadialCorrection": (None, [_i, _vp, _vp, _vp, _vp, _vp]),
    "createMesh": (_mesh, []),
    "deleteMesh": (None, [_mesh]),
    "ICP": (_f, [_vp, _vp, _i, _i, _vp, _vp, _i]),
    "lsnIcpPointToPlane": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i]),
    "lsnGetLastError": (_i, [_s, _i]),
    "lsnDeviceCount": (_i, []),
    "lsnCorrectAndGenerateMesh": (None, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _mesh, _f, _f, _f, _f, _f, _f, _i]),
    "lsnRefineFromDepthMaps": (_i, [_i] + [_vp] * 6 + [_f] * 6 + [_i] * 3 + [_vp] * 7),
    "lsnHostScheduleDescribe": (_i, [_i, _vp, _vp, _i, _i, _i, _i, _s, _i]),
    "lsnHostShardDescribe": (_i, [_i, _i, _vp, _s, _i]),
    "lsnHostShardPartMicros": (_i, [_vp, _i]),
    "lsnTestFaultPoints": (_ll, [_i]),
    "lsnHostPoolStats": (_i, [_vp, _vp, _vp]),
    "lsnSetOverlayMerge": (_i, [_i]),
    "lsnSetOutlierFilter": (_i, [_i, _f, _vp, _vp]),
    "lsnSetColorBlend": (_i, [_i, _i, _vp, _vp]),
    "lsnSetFlyingPixelFilter": (_i, [_i, _i, _vp, _vp]),
    "lsnSetDepthSmooth": (_i, [_i, _f, _f, _vp, _vp, _vp]),
    "lsnDepthSmoothGaussian": (_i, [_i, _f, _f, _vp, _vp, _i]),
    "lsnSetTemporalFilter": (_i, [_i, _i, _i, _vp, _vp, _vp]),
    "lsnResetTemporalFilter": (_i, []),
    "lsnSetBackground": (_i, [_i, _i, _i, _vp, _vp, _vp]),
    "lsnLearnBackground": (_i, [_i]),
    # part 2: the device-resident API
    "lsnFusionCreate": (_vp, [_i, _i, _i, _vp, _vp]),
    "lsnFusionDestroy": (None, [_vp]),
    "lsnFusionTickCapacity": (_ll, [_vp]),
    "lsnFusionSetParams": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "lsnPackSensorParams": (_i, [_vp, _vp, _vp]),
    "lsnFusionSetMode": (_i, [_vp, _i]),
    "lsnFusionRun": (_i, [_vp] * 6),
    "lsnFusionRunStreamed": (_i, [_vp] * 7),
    "lsnFusionSetPipelined": (_i, [_vp, _i]),
    "lsnFusionRadialCorrect": (_i, [_vp] * 5),
    "lsnFusionRadialCorrectTo": (_i, [_vp] * 7),
    "lsnFusionRadialCountersLeft": (_i, [_vp, _vp]),
    "lsnFusionRunMesh": (_i, [_vp] * 8),
    "lsnFusionTickTriangleCapacity": (_ll, [_vp]),
    "lsnFusionProfile": (_i, [_vp, _i]),
    "lsnFusionKernelStats": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(_ll), _s, _i, _i]),
    "lsnFusionLookbackFailed": (_i, [_vp, _vp]),
    "lsnFusionCheck": (_i, [_vp, _vp]),
    "lsnFusionThresholds": (_i, [_vp, _vp, C.POINTER(_f), _vp]),
    "lsnMergeShards": (_i, [_i, _i, _i, _i, _vp, _ll, _vp, _vp, _ll, _vp, _vp]),
    "lsnFusionColorTransfer": (_i, [_vp] * 5),
    "lsnFusionColorDiagnostics": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "lsnFusionColorBlend": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp]),
    "lsnFusionColorBlendDiagnostics": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "lsnFusionOverlayMerge": (_i, [_vp] * 7),
    "lsnFusionOverlayDiagnostics": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "lsnFusionOutlierFilter": (_i, [_vp, _i, _f, _vp, _vp, _vp, _vp, _vp]),
    "lsnFusionOutlierDiagnostics": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "lsnFusionFlyingPixels": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    "lsnFusionFlyingDiagnostics": (_i, [_vp, _i, _vp, _vp]),
    "lsnFusionSetDepthSmooth": (_i, [_vp, _i, _vp, _vp, _i]),
    "lsnFusionDepthSmooth": (_i, [_vp] * 4),
    "lsnFusionDepthSmoothDiagnostics": (_i, [_vp, _i, _vp, _vp, _vp]),
    "lsnFusionSetTemporal": (_i, [_vp, _i, _i, _i]),
    "lsnFusionTemporal": (_i, [_vp] * 4),
    "lsnFusionTemporalReset": (_i, [_vp, _vp]),
    "lsnFusionTemporalStateRead": (_i, [_vp] * 3),
    "lsnFusionTemporalStateWrite": (_i, [_vp] * 3),
    "lsnFusionTemporalDiagnostics": (_i, [_vp, _i] + [_vp] * 5),
    "lsnFusionSetBackground": (_i, [_vp, _i, _i, _i]),
    "lsnFusionBackgroundLearn": (_i, [_vp] * 3),
    "lsnFusionBackground": (_i, [_vp] * 4),
    "lsnFusionBackgroundReset": (_i, [_vp, _vp]),
    "lsnFusionBackgroundModelRead": (_i, [_vp] * 3),
    "lsnFusionBackgroundModelWrite": (_i, [_vp] * 3),
    "lsnFusionBackgroundDiagnostics": (_i, [_vp, _i] + [_vp] * 7),
    "lsnFusionRenderViews": (_i, [_vp, _i, _vp, _vp, _i, _i] + [_vp] * 7),
    "lsnFusionRenderDiagnostics": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp]),
    "lsnFusionSimplify": (_i, [_vp, _f] + [_vp] * 10),
    "lsnFusionSimplifyDiagnostics": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "lsnFusionFragments": (_i, [_vp, _i] + [_vp] * 11),
    "lsnFusionFragmentsDiagnostics": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "lsnFusionNormals": (_i, [_vp] * 7),
    "lsnFusionNormalsDiagnostics": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "lsnFusionSmooth": (_i, [_vp, _i, _f, _f, _i] + [_vp] * 6),
    "lsnFusionSmoothDiagnostics": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "lsnFusionTilesPerTick": (_i, [_vp]),
    "lsnFusionPackSurvivors": (_i, [_vp] * 9),
    "lsnFusionReconstruct": (_i, [_vp, _i, _i, _vp, _vp, _vp, _ll, _vp, _vp, _vp, _vp, _vp]),
    "lsnFusionPackSurvivorsRun": (_i, [_vp] * 10),
    "lsnFusionReconstructRun": (_i, [_vp, _i, _i, _vp, _vp, _vp, _ll, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lsnDeviceMalloc": (_vp, [_i, _ll]),
    "lsnDeviceFree": (_i, [_i, _vp]),
    "lsnDeviceUpload": (_i, [_i, _vp, _vp, _ll, _vp]),
    "lsnDeviceDownload": (_i, [_i, _vp, _vp, _ll, _vp]),
    "lsnStreamCreate": (_vp, [_i]),
    "lsnStreamDestroy": (_i, [_i, _vp]),
    "lsnStreamSynchronize": (_i, [_i, _vp]),
    "lsnShardUniqueId": (_i, [_vp]),
    "lsnShardCreate": (_vp, [_i, _i, _i, _vp, _i, _i, _vp, _vp]),
    "lsnShardPrepare": (_vp, [_i, _i, _i, _i, _i, _vp, _vp]),
    "lsnShardConnect": (_i, [_vp, _vp]),
    "lsnShardRcclPath": (_i, [_s, _i]),
    "lsnShardPlan": (_vp, [_vp, _i]),
    "lsnShardDestroy": (None, [_vp]),
    "lsnShardMergedCapacity": (_ll, [_vp]),
    "lsnShardSetParams": (_i, [_vp] * 5),
    "lsnShardStep": (_i, [_vp] * 6),
    "lsnShardLastBytesSent": (_ll, [_vp]),
    "lsnShardRanksSeen": (_i, [_vp]),
    "lsnIcpCreate": (_vp, [_i, _i, _i]),
    "lsnIcpDestroy": (None, [_vp]),
    "lsnIcpRun": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _vp]),
    "lsnIcpRunPlane": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _vp]),
    "lsnIcpNearest": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp]),
    "lsnIcpTrace": (_i, [_vp, _vp, _i, _vp]),
    "lsnIcpSetProfiling": (_i, [_vp, _i]),
    "lsnIcpProfile": (_i, [_vp, _vp, _vp]),
    "lsnIcpNearResolved": (_i, [_vp, _vp]),
    "lsnRefine": (_i, [_i, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "lsnRefineVertices": (_i, [_i, _i, _vp, _vp, _i, _i] + [_vp] * 8),
    "lsnRefineVerticesPlane": (_i, [_i, _i, _vp, _vp, _vp, _i, _i] + [_vp] * 8),
    "lsnRefineComposePoses": (_i, [_i] + [_vp] * 6),
    "lsnRefineRelease": (_ll, [_i]),
    "lsnTickCreate": (_vp, [_i, _i, _i, _vp, _vp]),
    "lsnTickDestroy": (None, [_vp]),
    "lsnTickSetParams": (_i, [_vp] * 5),
    "lsnTickSetFlyingPixels": (_i, [_vp, _i, _i]),
    "lsnTickSetDepthSmooth": (_i, [_vp, _i, _f, _f]),
    "lsnTickSetTemporal": (_i, [_vp, _i, _i, _i]),
    "lsnTickTemporalReset": (_i, [_vp, _vp]),
    "lsnTickSetBackground": (_i, [_vp, _i, _i, _i]),
    "lsnTickBackgroundLearn": (_i, [_vp] * 3),
    "lsnTickBackgroundReset": (_i, [_vp, _vp]),
    "lsnTickCapacity": (_ll, [_vp]),
    "lsnTickTriangleCapacity": (_ll, [_vp]),
    "lsnTickParts": (_i, [_vp]),
    "lsnTickRun": (_i, [_vp] * 10),
    # part 3: wire / disk formats
    "lsnTransferCreate": (_vp, [_i, _i, _i]),
    "lsnTransferDestroy": (None, [_vp]),
    "lsnTransferFrameBound": (_ll, [_i, _i]),
    "lsnTransferPack": (_ll, [_vp, _vp, _i, _vp, _i, _vp, _ll, _vp]),
    "lsnTransferLastPath": (_i, [_vp]),
    "lsnPlyBinaryBytes": (_ll, [_i, _i]),
    "lsnPlyPack": (_ll, [_i, _vp, _i, _vp, _i, _vp, _ll, _vp]),
    "lsnPlyNormalsBytes": (_ll, [_i, _i]),
    "lsnPlyPackNormals": (_ll, [_i, _vp, _vp, _i, _vp, _i, _vp, _ll, _vp]),
    "lsnLastMeshTransferFrame": (_ll, [_vp, _ll]),
    "lsnLastMeshPly": (_ll, [_vp, _ll]),
    "lsnLastMeshRenderView": (_ll, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "lsnLastMeshTransferFrameLod": (_ll, [_f, _vp, _ll]),
    "lsnLastMeshPlyLod": (_ll, [_f, _vp, _ll]),
    "lsnLastMeshPlyNormals": (_ll, [_f, _vp, _ll]),
    "lsnLastMeshTransferFrameFragments": (_ll, [_i, _f, _vp, _ll]),
    "lsnLastMeshPlyFragments": (_ll, [_i, _f, _i, _vp, _ll]),
    "lsnLastMeshPlySmooth": (_ll, [_i, _f, _i, _f, _f, _i, _i, _vp, _ll]),
    "lsnLastMeshTransferFrameSmooth": (_ll, [_i, _f, _i, _f, _f, _i, _vp, _ll]),
    "lsnZstdAvailable": (_i, []),
    "lsnFrameParseHeader": (_i, [_vp, C.POINTER(FrameInfo)]),
    "lsnFrameDecode": (_ll, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, C.POINTER(_i)]),
    "lsnFrameEncode": (_ll, [_vp, _vp, _i, _i, _vp, _i, _i, _vp, _ll]),
    "lsnRecordingNext": (_ll, [_vp, _ll, _ll, C.POINTER(_ll), C.POINTER(_i), C.POINTER(_i)]),
    "lsnRecordingAppend": (_ll, [_vp, _ll, _vp, _i, _i]),
}
EXPORTS = list(_PROTOTYPES)

_lib = None


def lib():
    """Loads libNativeUtils.so and declares the prototypes.  Raises NativeUtilsError when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeUtilsError(f"{LIB_PATH} is missing -- run __graft_entry__.build() (there is no CPU fallback)")
    # PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64 under the same SONAME as /opt/rocm's.  A
    # process must run ONE HIP runtime (device pointers handed over by torch have to belong to the runtime that launches
    # our kernels), and the dynamic loader keeps whichever copy is loaded first -- so when torch is installed it is
    # imported before the library.  Hosts without torch (LiveScanServer, C/C++ callers) simply get /opt/rocm's runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    try:
        L = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise NativeUtilsError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (restype, argtypes) in _PROTOTYPES.items():
        fn = getattr(L, name, None)   # a foreign build ($LSN_NATIVE_LIB) may lack an export: it stays undeclared, and calling it raises
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def last_error():
    buf = C.create_string_buffer(1024)
    lib().lsnGetLastError(buf, len(buf))
    return buf.value.decode("utf-8", "replace")


def _check(rc, what):
    if rc != 0:
        raise NativeUtilsError(f"{what} failed: {last_error()}")


def _nonneg(n, what):
    """A count / size / code an export returns: negative means it failed."""
    if n < 0:
        raise NativeUtilsError(f"{what} failed: {last_error()}")
    return n


def _handle(h, what):
    """The handle an lsn*Create export returns: null means it failed."""
    if not h:
        raise NativeUtilsError(f"{what} failed: {last_error()}")
    return h


def device_count():
    return int(lib().lsnDeviceCount())


def require_gpu():
    if device_count() <= 0:
        raise NativeUtilsError("no HIP device visible: libNativeUtils has no CPU path")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _as(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


# ----------------------------------------------------------------------------------------------------------
# Part 1: the reference's exports (host buffers in, host buffers out)
# ----------------------------------------------------------------------------------------------------------

def _copy_mesh(mesh):
    """KinectServer.CopyMeshToVerticesWithColoursArray (KinectServer.cs:376-389) + deleteMesh."""
    n = mesh.nVertices
    if n > 0:
        if not mesh.vertices:
            raise NativeUtilsError("mesh has nVertices > 0 but a null vertices pointer")
        raw = C.string_at(mesh.vertices, n * 16)
        verts = np.frombuffer(raw, dtype=VERTEX_DTYPE).copy()
    else:
        verts = np.zeros(0, dtype=VERTEX_DTYPE)
    ntri = mesh.nTriangles
    tris = np.zeros((0, 3), dtype=np.int32)
    if ntri > 0:
        tris = np.frombuffer(C.string_at(mesh.triangles, ntri * 12), dtype=np.int32).reshape(-1, 3).copy()
    lib().deleteMesh(C.byref(mesh))
    return verts, tris


def set_overlay_merge(enable):
    """lsnSetOverlayMerge: the process-wide switch of generateMeshFromDepthMaps' overlay merge.  Returns the previous value (bool)."""
    return bool(lib().lsnSetOverlayMerge(1 if enable else 0))


def set_outlier_filter(k, max_dist):
    """lsnSetOutlierFilter: the process-wide (k, max_dist) of the exports' outlier filter (k <= 0 or max_dist <= 0: off).
    Returns the previous pair."""
    pk, pd = C.c_int(0), C.c_float(0)
    _check(lib().lsnSetOutlierFilter(int(k), float(max_dist), C.byref(pk), C.byref(pd)), "lsnSetOutlierFilter")
    return pk.value, pd.value


def set_color_blend(depth_tol, min_confidence):
    """lsnSetColorBlend: the process-wide (depth_tol, min_confidence) of the colour blend in generate_mesh_from_depth_maps and
    correct_and_generate_mesh (depth_tol <= 0 or min_confidence > 20: off).  Returns the previous pair."""
    pt, pc = C.c_int(0), C.c_int(0)
    _check(lib().lsnSetColorBlend(int(depth_tol), int(min_confidence), C.byref(pt), C.byref(pc)), "lsnSetColorBlend")
    return pt.value, pc.value


def set_flying_pixel_filter(neighbourhood, threshold):
    """lsnSetFlyingPixelFilter: the process-wide (neighbourhood, threshold) of the flying-pixel filter in the exports that start with the
    radial correction (radial_correction, correct_and_generate_mesh); neighbourhood <= 0: off.  Returns the previous pair."""
    pn, pt = C.c_int(0), C.c_int(0)
    _check(lib().lsnSetFlyingPixelFilter(int(neighbourhood), int(threshold), C.byref(pn), C.byref(pt)), "lsnSetFlyingPixelFilter")
    return pn.value, pt.value


def depth_smooth_gaussian(radius, sigma_s, sigma_r, range_cap=1024):
    """lsnDepthSmoothGaussian (needs no GPU): the Gaussian tables of depth smoothing for (radius, sigma_s, sigma_r).  Returns (spatial
    uint16 [2r+1, 2r+1], range uint16 [n_range]); n_range is at most min(range_cap, 1024)."""
    side = 2 * int(radius) + 1 if 1 <= int(radius) <= 3 else 1
    ws = np.zeros(side * side, dtype=np.uint16)
    wr = np.zeros(max(min(int(range_cap), 1024), 1), dtype=np.uint16)
    n = _nonneg(lib().lsnDepthSmoothGaussian(int(radius), float(sigma_s), float(sigma_r), _ptr(ws), _ptr(wr), int(range_cap)), "lsnDepthSmoothGaussian")
    return ws.reshape(side, side), wr[:n].copy()


def set_depth_smooth(radius, sigma_s=0.0, sigma_r=0.0):
    """lsnSetDepthSmooth: the process-wide (radius, sigma_s, sigma_r) of depth smoothing in the exports that start with the radial correction
    (radial_correction, correct_and_generate_mesh), between the flying-pixel filter and the correction; radius <= 0: off.  Returns the
    previous triple."""
    pr, ps, pq = C.c_int(0), C.c_float(0), C.c_float(0)
    _check(lib().lsnSetDepthSmooth(int(radius), float(sigma_s), float(sigma_r), C.byref(pr), C.byref(ps), C.byref(pq)), "lsnSetDepthSmooth")
    return pr.value, ps.value, pq.value


def set_temporal_filter(alpha_q, delta=0, persist=0):
    """lsnSetTemporalFilter: the process-wide (alpha_q, delta, persist) of the temporal depth filter in the exports that start at raw frames
    (radial_correction, correct_and_generate_mesh), in front of the flying-pixel filter; each such call is one tick; alpha_q <= 0: off.
    Returns the previous triple."""
    pa, pd, pp = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(lib().lsnSetTemporalFilter(int(alpha_q), int(delta), int(persist), C.byref(pa), C.byref(pd), C.byref(pp)), "lsnSetTemporalFilter")
    return pa.value, pd.value, pp.value


def reset_temporal_filter():
    """lsnResetTemporalFilter: the exports' next filtering call starts from no history."""
    _check(lib().lsnResetTemporalFilter(), "lsnResetTemporalFilter")


def set_background(margin, rel_q=0, min_pixels=0):
    """lsnSetBackground: the process-wide (margin, rel_q, min_pixels) of background subtraction in the exports that start at raw frames
    (radial_correction, correct_and_generate_mesh), behind the temporal filter; each such call is one tick; margin <= 0: off.  Returns the
    previous triple."""
    pm, pq, pp = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(lib().lsnSetBackground(int(margin), int(rel_q), int(min_pixels), C.byref(pm), C.byref(pq), C.byref(pp)), "lsnSetBackground")
    return pm.value, pq.value, pp.value


def learn_background(n_calls):
    """lsnLearnBackground: every lane zeroes its model at its next call with the stage on and learns for n_calls calls before it subtracts."""
    _check(lib().lsnLearnBackground(int(n_calls)), "lsnLearnBackground")


class _Scoped:
    """Sets a process-wide setting for the body of a with-statement: setter(*setting) returns the previous one, which goes back in on the
    way out (None: leaves the setting as it is)."""

    def __init__(self, setter, setting):
        self.setter, self.setting, self.prev = setter, setting, None

    def __enter__(self):
        if self.setting is not None:
            self.prev = self.setter(*self.setting)

    def __exit__(self, *exc):
        if self.prev is not None:
            self.setter(*self.prev)


def _host_args(depth_maps, depth_colors, widths, heights, intr, wt=None, bounds=None, copy=False):
    """The host arrays of a part 1 export as it reads them, their sizes checked: (n, depth bytes, colour bytes, widths, heights, intr, wt,
    bounds as six floats); wt / bounds stay None for the export without them.  copy: the depth and colour bytes are private copies (for
    an export that works in place)."""
    widths, heights = _as(widths, np.int32), _as(heights, np.int32)
    n = len(widths)
    dm = np.ascontiguousarray(depth_maps).view(np.uint8).ravel()
    dc = _as(depth_colors, np.uint8).ravel()
    if copy:
        dm, dc = dm.copy(), dc.copy()
    intr = _as(intr, np.float32).ravel()
    assert intr.size == 7 * n
    if wt is not None:
        wt, bounds = _as(wt, np.float32).ravel(), _as(bounds, np.float32).ravel()
        assert wt.size == 12 * n and bounds.size == 6
        bounds = [float(x) for x in bounds]
    return n, dm, dc, widths, heights, intr, wt, bounds


def _raise_if_empty(mesh):
    """A mesh export left a message and an empty mesh: the mesh goes back to the library and the message is raised."""
    err = last_error()
    if err and mesh.nVertices == 0:
        lib().deleteMesh(C.byref(mesh))
        raise NativeUtilsError(err)


def generate_mesh_from_depth_maps(depth_maps, depth_colors, widths, heights, intr, wt, bounds,
                                  color_transfer=False, generate_triangles=False, overlay_merge=None, outlier_filter=None, color_blend=None):
    """KinectServer.GenerateMesh (KinectServer.cs:354-374).  Returns (vertices[VERTEX_DTYPE], triangles int32).
    overlay_merge: None leaves the process-wide switch (lsnSetOverlayMerge) as it is; True / False sets it for this call alone.
    outlier_filter: None leaves the process-wide outlier filter (lsnSetOutlierFilter) as it is; (k, max_dist) sets it for this call alone.
    color_blend: None leaves the process-wide colour blend (lsnSetColorBlend) as it is; (depth_tol, min_confidence) sets it for this call alone."""
    with _Scoped(set_outlier_filter, outlier_filter), _Scoped(set_color_blend, color_blend), \
            _Scoped(lambda on: (set_overlay_merge(on),), None if overlay_merge is None else (overlay_merge,)):
        require_gpu()
        n, dm, dc, widths, heights, intr, wt, b = _host_args(depth_maps, depth_colors, widths, heights, intr, wt, bounds)
        mesh = Mesh()
        lib().generateMeshFromDepthMaps(n, _ptr(dm), _ptr(dc), _ptr(widths), _ptr(heights), _ptr(intr), _ptr(wt),
                                        C.byref(mesh), bool(color_transfer), *b, bool(generate_triangles))
        if not generate_triangles:   # (with triangles the message may be the notice that goes with the unmerged mesh)
            _raise_if_empty(mesh)
        return _copy_mesh(mesh)


def host_shards(n_maps, n_devices=0):
    """How a merge call over n_maps sensors is cut over n_devices devices of $LSN_HOST_DEVICES (lsnHostShardDescribe; needs no GPU).
    Returns (block bounds [first_0, ..., first_D], text such as "0:[0-3] 1:[4-7]")."""
    buf = C.create_string_buffer(1024)
    first = (C.c_int * 18)()
    d = lib().lsnHostShardDescribe(int(n_maps), int(n_devices), first, buf, len(buf))
    if d < 0:
        raise NativeUtilsError(last_error())
    return [int(first[i]) for i in range(d + 1)], buf.value.decode()


def host_shard_part_micros():
    """Wall time (us) of every part of the last sharded call when the parts ran one after the other ($LSN_HOST_SHARD_SOLO=1); [] if none."""
    out = (C.c_longlong * 16)()
    d = lib().lsnHostShardPartMicros(out, 16)
    return [int(out[i]) for i in range(max(0, d))]


def host_pool_stats():
    """(blocks out with callers, blocks waiting for reuse, bytes out) of the pool of pinned mesh blocks (lsnHostPoolStats)."""
    live, pooled, nbytes = C.c_int(0), C.c_int(0), C.c_longlong(0)
    _check(lib().lsnHostPoolStats(C.byref(live), C.byref(pooled), C.byref(nbytes)), "lsnHostPoolStats")
    return live.value, pooled.value, nbytes.value


def host_schedule(widths, heights, first=0, count=None, radial=False, sensors_per_group=0):
    """The upload schedule the host exports follow for these frames (lsnHostScheduleDescribe; needs no GPU).
    Returns (number of groups, text such as "D[0-2] C[0-2] | D[3-7] C[3-5] | C[6-7]")."""
    widths, heights = _as(widths, np.int32), _as(heights, np.int32)
    n = len(widths)
    buf = C.create_string_buffer(4096)
    g = lib().lsnHostScheduleDescribe(n, _ptr(widths), _ptr(heights), int(first), int(n - first if count is None else count), int(radial),
                                      int(sensors_per_group), buf, len(buf))
    if g < 0:
        raise NativeUtilsError(last_error())
    return g, buf.value.decode()


def radial_correction(depth_maps, depth_colors, widths, heights, intr, flying_pixels=None, depth_smooth=None, temporal_filter=None, background=None):
    """KinectServer.CorrectRadialDistortionsForDepthMaps (KinectServer.cs:518-525): returns corrected copies
    (depth as a uint8 view of the u16 maps, colours); the export itself works in place on the arrays it is given.
    flying_pixels: None leaves the process-wide flying-pixel filter (lsnSetFlyingPixelFilter) as it is; (neighbourhood, threshold) sets
    it for this call alone (the maps are filtered, then corrected).
    depth_smooth: None leaves the process-wide depth smoothing (lsnSetDepthSmooth) as it is; (radius, sigma_s, sigma_r) sets it for this
    call alone (the maps are filtered if that is on, smoothed, then corrected).
    temporal_filter: None leaves the process-wide temporal depth filter (lsnSetTemporalFilter) as it is; (alpha_q, delta, persist) sets it
    for this call alone (one tick of the history the library keeps for the rig; it runs in front of the other two).
    background: None leaves the process-wide background subtraction (lsnSetBackground) as it is; (margin, rel_q, min_pixels) sets it for this
    call alone (one tick against -- or, while the lane learns, into -- the model the library keeps for the rig; it runs behind the temporal filter)."""
    with _Scoped(set_temporal_filter, temporal_filter), _Scoped(set_background, background), _Scoped(set_flying_pixel_filter, flying_pixels), _Scoped(set_depth_smooth, depth_smooth):
        require_gpu()
        n, dm, dc, widths, heights, intr, _, _ = _host_args(depth_maps, depth_colors, widths, heights, intr, copy=True)
        lib().depthMapAndColorSetRadialCorrection(n, _ptr(dm), _ptr(dc), _ptr(widths), _ptr(heights), _ptr(intr))
        err = last_error()
        if err:
            raise NativeUtilsError(err)
        return dm, dc


def correct_and_generate_mesh(depth_maps, depth_colors, widths, heights, intr, wt, bounds, write_back=True, outlier_filter=None,
                              flying_pixels=None, depth_smooth=None, temporal_filter=None, background=None, color_blend=None):
    """One call per tick (extension): radial correction + merge call with a single upload.  Returns (vertices, triangles,
    corrected depth as uint8, corrected colours); with write_back=False the last two are the untouched inputs.
    outlier_filter / color_blend: as for generate_mesh_from_depth_maps (the corrected maps written back are the unmasked ones).
    flying_pixels / depth_smooth / temporal_filter / background: as for radial_correction (the corrected maps written back are the filtered,
    subtracted, smoothed, corrected ones)."""
    with _Scoped(set_temporal_filter, temporal_filter), _Scoped(set_background, background), _Scoped(set_flying_pixel_filter, flying_pixels), _Scoped(set_depth_smooth, depth_smooth), _Scoped(set_outlier_filter, outlier_filter), _Scoped(set_color_blend, color_blend):
        require_gpu()
        n, dm, dc, widths, heights, intr, wt, b = _host_args(depth_maps, depth_colors, widths, heights, intr, wt, bounds, copy=True)
        mesh = Mesh()
        lib().lsnCorrectAndGenerateMesh(n, _ptr(dm), _ptr(dc), _ptr(widths), _ptr(heights), _ptr(intr), _ptr(wt), C.byref(mesh),
                                        *b, 1 if write_back else 0)
        _raise_if_empty(mesh)
        v, t = _copy_mesh(mesh)
        return v, t, dm, dc


def generate_vertices_from_depth_map(depth_maps, depth_colors, widths, heights, intr, wt, bounds, index, outlier_filter=None):
    """One sensor's cropped cloud, as KinectServer.GetLatestFrameVerticesOnly calls it (KinectServer.cs:527-554).
    outlier_filter: as for generate_mesh_from_depth_maps."""
    with _Scoped(set_outlier_filter, outlier_filter):
        require_gpu()
        _, dm, dc, widths, heights, intr, wt, b = _host_args(depth_maps, depth_colors, widths, heights, intr, wt, bounds)
        mesh = Mesh()
        lib().generateVerticesFromDepthMap(_ptr(dm), _ptr(dc), _ptr(widths), _ptr(heights), _ptr(intr), _ptr(wt),
                                           C.byref(mesh), *b, int(index))
        _raise_if_empty(mesh)
        return _copy_mesh(mesh)[0]


def icp(verts1, verts2, R=None, t=None, max_iter=10):
    """ICP export (MainWindowForm.cs:42-43,370).  Returns (verts2_out, R_out[3,3], t_out[3]); inputs are not modified."""
    require_gpu()
    v1 = _as(verts1, np.float32).reshape(-1, 3)
    v2 = _as(verts2, np.float32).reshape(-1, 3).copy()
    R = np.eye(3, dtype=np.float32).ravel() if R is None else _as(R, np.float32).ravel().copy()
    t = np.zeros(3, dtype=np.float32) if t is None else _as(t, np.float32).ravel().copy()
    lib().ICP(_ptr(v1), _ptr(v2), len(v1), len(v2), _ptr(R), _ptr(t), int(max_iter))
    err = last_error()
    if err:
        raise NativeUtilsError(err)
    return v2, R.reshape(3, 3), t


def icp_point_to_plane(verts1, normals1, verts2, R=None, t=None, max_iter=10):
    """lsnIcpPointToPlane: ICP's flow on host arrays with the point-to-plane residual (normals1: the target's normals, [n1, 3]).
    Returns (verts2_out, R_out[3,3], t_out[3]); inputs are not modified."""
    require_gpu()
    v1 = _as(verts1, np.float32).reshape(-1, 3)
    n1 = _as(normals1, np.float32).reshape(-1, 3)
    assert n1.shape == v1.shape, (n1.shape, v1.shape)
    v2 = _as(verts2, np.float32).reshape(-1, 3).copy()
    R = np.eye(3, dtype=np.float32).ravel() if R is None else _as(R, np.float32).ravel().copy()
    t = np.zeros(3, dtype=np.float32) if t is None else _as(t, np.float32).ravel().copy()
    _check(lib().lsnIcpPointToPlane(_ptr(v1), _ptr(n1), _ptr(v2), len(v1), len(v2), _ptr(R), _ptr(t), int(max_iter)), "lsnIcpPointToPlane")
    return v2, R.reshape(3, 3), t


def refine(clouds, world_R, world_t, n_refine_iters=2, n_icp_iters=10, device=0):
    """refineWorker_DoWork (MainWindowForm.cs:330-410) through lsnRefine.  clouds: list of [n_i, 3] float arrays.
    Returns (clouds_out, world_R [n,3,3], world_t [n,3], Rs [n,3,3], Ts [n,3]); inputs are not modified."""
    require_gpu()
    cl = [_as(c, np.float32).reshape(-1, 3).copy() for c in clouds]
    n = np.array([len(c) for c in cl], dtype=np.int32)
    ptrs = (C.c_void_p * len(cl))(*[c.ctypes.data for c in cl])
    wR = _as(world_R, np.float32).reshape(-1).copy()
    wt = _as(world_t, np.float32).reshape(-1).copy()
    assert wR.size == 9 * len(cl) and wt.size == 3 * len(cl)
    Rs = np.zeros(9 * len(cl), dtype=np.float32)
    Ts = np.zeros(3 * len(cl), dtype=np.float32)
    _check(lib().lsnRefine(int(device), len(cl), C.cast(ptrs, C.c_void_p), _ptr(n), int(n_refine_iters), int(n_icp_iters),
                           _ptr(wR), _ptr(wt), _ptr(Rs), _ptr(Ts)), "lsnRefine")
    return cl, wR.reshape(-1, 3, 3), wt.reshape(-1, 3), Rs.reshape(-1, 3, 3), Ts.reshape(-1, 3)


def _pose_pair(R, t, n):
    """An in/out pose pair of a refine export as private flat f32 copies, or (None, None)."""
    if R is None or t is None:
        return None, None
    R, t = _as(R, np.float32).reshape(-1).copy(), _as(t, np.float32).reshape(-1).copy()
    assert R.size == 9 * n and t.size == 3 * n
    return R, t


def _opt(a):
    return None if a is None else _ptr(a)


def _shaped(a, *shape):
    return None if a is None else a.reshape(*shape)


def compose_poses(Rs, Ts, world_R=None, world_t=None, camera_R=None, camera_t=None):
    """lsnRefineComposePoses (needs no GPU): the pose composition at the end of refineWorker_DoWork (MainWindowForm.cs:382-410), the C#
    loops as written.  Returns (world_R [n,3,3], world_t [n,3], camera_R, camera_t), None for a pair that was not given; inputs are
    not modified."""
    Rs, Ts = _as(Rs, np.float32).reshape(-1), _as(Ts, np.float32).reshape(-1)
    n = Ts.size // 3
    assert Rs.size == 9 * n and Ts.size == 3 * n
    wR, wt = _pose_pair(world_R, world_t, n)
    cR, ct = _pose_pair(camera_R, camera_t, n)
    _check(lib().lsnRefineComposePoses(n, _ptr(Rs), _ptr(Ts), _opt(wR), _opt(wt), _opt(cR), _opt(ct)), "lsnRefineComposePoses")
    return _shaped(wR, -1, 3, 3), _shaped(wt, -1, 3), _shaped(cR, -1, 3, 3), _shaped(ct, -1, 3)


def refine_frames(depth_maps, depth_colors, widths, heights, intr, wt, bounds, n_refine_iters=2, n_icp_iters=10, correct_radial=False,
                  camera_R=None, camera_t=None, outlier_filter=None, flying_pixels=None):
    """lsnRefineFromDepthMaps: LiveScanServer's "Refine calibration" in one call -- frames up once, vertices, XYZ and the Gauss-Seidel loop
    on the device.  Returns a dict: clouds (list of [n_i, 3] f32, refined), counts, Rs [n,3,3], Ts [n,3], wt (the refined world
    transforms, packed like the input), camera_R / camera_t (None unless given); inputs are not modified.
    outlier_filter / flying_pixels: as for correct_and_generate_mesh (the latter only matters with correct_radial)."""
    with _Scoped(set_flying_pixel_filter, flying_pixels), _Scoped(set_outlier_filter, outlier_filter):
        n, dm, dc, widths, heights, intr, wt, b = _host_args(depth_maps, depth_colors, widths, heights, intr, wt, bounds)
        cR, ct = _pose_pair(camera_R, camera_t, n)
        Rs, Ts = np.zeros(9 * n, dtype=np.float32), np.zeros(3 * n, dtype=np.float32)
        wt_out = np.zeros(12 * n, dtype=np.float32)
        clouds = np.zeros(max(1, int(np.sum(widths.astype(np.int64) * heights))) * 3, dtype=np.float32)
        counts = np.zeros(n, dtype=np.int32)
        _check(lib().lsnRefineFromDepthMaps(n, _ptr(dm), _ptr(dc), _ptr(widths), _ptr(heights), _ptr(intr), _ptr(wt), *b,
                                            1 if correct_radial else 0, int(n_refine_iters), int(n_icp_iters), _ptr(wt_out), _opt(cR), _opt(ct),
                                            _ptr(Rs), _ptr(Ts), _ptr(clouds), _ptr(counts)), "lsnRefineFromDepthMaps")
        off = np.concatenate([[0], np.cumsum(counts)])
        return {"clouds": [clouds[3 * off[i]:3 * off[i + 1]].reshape(-1, 3).copy() for i in range(n)], "counts": counts,
                "Rs": Rs.reshape(-1, 3, 3), "Ts": Ts.reshape(-1, 3), "wt": wt_out,
                "camera_R": _shaped(cR, -1, 3, 3), "camera_t": _shaped(ct, -1, 3)}


def refine_vertices(device, n_sensors, d_vertices, d_offsets, n_refine_iters=2, n_icp_iters=10, world_R=None, world_t=None, camera_R=None,
                    camera_t=None, d_clouds_out=None, stream=0):
    """lsnRefineVertices: the refine pass on ONE tick's merged cloud that is resident on `device` (d_vertices / d_offsets / d_clouds_out:
    device pointers as integers).  Synchronises `stream`; complete on return.  Returns (world_R, world_t, camera_R, camera_t, Rs, Ts),
    None for a pair that was not given; inputs are not modified."""
    n = int(n_sensors)
    wR, wt = _pose_pair(world_R, world_t, n)
    cR, ct = _pose_pair(camera_R, camera_t, n)
    Rs, Ts = np.zeros(9 * n, dtype=np.float32), np.zeros(3 * n, dtype=np.float32)
    _check(lib().lsnRefineVertices(int(device), n, d_vertices, d_offsets, int(n_refine_iters), int(n_icp_iters), _opt(wR), _opt(wt), _opt(cR),
                                   _opt(ct), _ptr(Rs), _ptr(Ts), d_clouds_out, stream), "lsnRefineVertices")
    return _shaped(wR, -1, 3, 3), _shaped(wt, -1, 3), _shaped(cR, -1, 3, 3), _shaped(ct, -1, 3), Rs.reshape(-1, 3, 3), Ts.reshape(-1, 3)


def refine_vertices_plane(device, n_sensors, d_vertices, d_normals, d_offsets, n_refine_iters=2, n_icp_iters=10, world_R=None, world_t=None,
                          camera_R=None, camera_t=None, d_clouds_out=None, stream=0):
    """lsnRefineVerticesPlane: refine_vertices with the point-to-plane residual; d_normals: the tick's vertex normals (one tick of
    lsnFusionNormals' output, a device pointer as an integer).  Returns what refine_vertices returns."""
    n = int(n_sensors)
    wR, wt = _pose_pair(world_R, world_t, n)
    cR, ct = _pose_pair(camera_R, camera_t, n)
    Rs, Ts = np.zeros(9 * n, dtype=np.float32), np.zeros(3 * n, dtype=np.float32)
    _check(lib().lsnRefineVerticesPlane(int(device), n, d_vertices, d_normals, d_offsets, int(n_refine_iters), int(n_icp_iters), _opt(wR), _opt(wt),
                                        _opt(cR), _opt(ct), _ptr(Rs), _ptr(Ts), d_clouds_out, stream), "lsnRefineVerticesPlane")
    return _shaped(wR, -1, 3, 3), _shaped(wt, -1, 3), _shaped(cR, -1, 3, 3), _shaped(ct, -1, 3), Rs.reshape(-1, 3, 3), Ts.reshape(-1, 3)


def refine_release(device=-1):
    """lsnRefineRelease: frees what the refine passes keep on `device` (default: every device).  Returns the bytes released."""
    return int(_nonneg(lib().lsnRefineRelease(int(device)), "lsnRefineRelease"))


# ----------------------------------------------------------------------------------------------------------
# Part 2: device-resident API
# ----------------------------------------------------------------------------------------------------------

class _Handle:
    """What the classes around an lsn*Create'd handle share: close() destroys the handle once, through the export the class names; a
    collected object closes itself and never raises."""
    _destroy = None   # the export that destroys the handle
    _h = None

    def close(self):
        if self._h:
            getattr(lib(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _set_params(what, h, n_maps, intr, wt, bounds, stream):
    """lsnFusionSetParams / lsnShardSetParams / lsnTickSetParams: the calibration of n_maps sensors and the bounding box."""
    intr, wt, b = _as(intr, np.float32).ravel(), _as(wt, np.float32).ravel(), _as(bounds, np.float32).ravel()
    assert intr.size == 7 * n_maps and wt.size == 12 * n_maps and b.size == 6
    _check(getattr(lib(), what)(h, _ptr(intr), _ptr(wt), _ptr(b), stream), what)


class FusionPlan(_Handle):
    """lsnFusion*: T ticks x N sensors fused per call on HBM-resident inputs."""
    _destroy = "lsnFusionDestroy"

    def __init__(self, device, n_ticks, widths, heights):
        require_gpu()
        self.widths, self.heights = _as(widths, np.int32), _as(heights, np.int32)
        self.n_maps, self.n_ticks, self.device = len(self.widths), int(n_ticks), int(device)
        self._h = _handle(lib().lsnFusionCreate(self.device, self.n_ticks, self.n_maps, _ptr(self.widths), _ptr(self.heights)), "lsnFusionCreate")
        self.capacity = int(lib().lsnFusionTickCapacity(self._h))
        self.pixels_per_tick = int(np.sum(self.widths.astype(np.int64) * self.heights))

    def set_params(self, intr, wt, bounds, stream=0):
        _set_params("lsnFusionSetParams", self._h, self.n_maps, intr, wt, bounds, stream)

    def set_pipelined(self, enable=True):
        """Overlap the count pass of the next call with the write kernel of the current one (inputs must be resident)."""
        _check(lib().lsnFusionSetPipelined(self._h, 1 if enable else 0), "lsnFusionSetPipelined")

    def set_mode(self, mode):
        _check(lib().lsnFusionSetMode(self._h, int(mode)), "lsnFusionSetMode")

    def run(self, d_depth, d_colors, d_vertices, d_offsets, stream=0):
        """All four are device pointers (ints); asynchronous on `stream` (a hipStream_t as int, 0 = null stream)."""
        _check(lib().lsnFusionRun(self._h, d_depth, d_colors, d_vertices, d_offsets, stream), "lsnFusionRun")

    def radial_correct(self, intr, d_depth, d_colors, stream=0):
        """In-place radial correction of the plan's n_ticks x n_maps frames resident in HBM."""
        intr = _as(intr, np.float32).ravel()
        assert intr.size == 7 * self.n_maps
        _check(lib().lsnFusionRadialCorrect(self._h, _ptr(intr), d_depth, d_colors, stream), "lsnFusionRadialCorrect")

    def radial_correct_to(self, intr, d_depth, d_colors, d_depth_out, d_colors_out, stream=0):
        """Out-of-place radial correction (the cheaper form: the un-closed maps never leave the GPU's LDS)."""
        intr = _as(intr, np.float32).ravel()
        assert intr.size == 7 * self.n_maps
        _check(lib().lsnFusionRadialCorrectTo(self._h, _ptr(intr), d_depth, d_colors, d_depth_out, d_colors_out, stream),
               "lsnFusionRadialCorrectTo")

    def radial_counters_left(self, stream=0):
        """Work counters of the hole-closing chain that are not zero once `stream` has drained (test hook; 0 after a complete chain)."""
        n = _nonneg(lib().lsnFusionRadialCountersLeft(self._h, stream), "lsnFusionRadialCountersLeft")
        return n

    def run_mesh(self, d_depth, d_colors, d_vertices, d_offsets, d_triangles, d_tri_offsets, stream=0):
        """Vertices + triangles (the reference's complete merge call); d_triangles: n_ticks x 2*capacity x 3 int32."""
        _check(lib().lsnFusionRunMesh(self._h, d_depth, d_colors, d_vertices, d_offsets, d_triangles, d_tri_offsets, stream),
               "lsnFusionRunMesh")

    def color_transfer(self, d_depth, d_vertices, d_offsets, stream=0):
        """Colour transfer (bcolor_transfer) in place on the clouds run() / run_mesh() wrote from d_depth; every tick on its own."""
        _check(lib().lsnFusionColorTransfer(self._h, d_depth, d_vertices, d_offsets, stream or None), "lsnFusionColorTransfer")

    def color_diagnostics(self, tick=0, stream=0):
        """What the last color_transfer() computed for one tick: {"confidence": uint8[pixels_per_tick], "coverage": int32[n, n]
        (symmetric), "pairs": [(i, j), ...] in the order they were chosen, "transforms": float64[n_pairs, 9] (mean_i[3], mean_j[3],
        scale[3])}."""
        n = self.n_maps
        conf = np.zeros(max(self.pixels_per_tick, 1), dtype=np.uint8)
        cov = np.zeros((n, n), dtype=np.int32)
        pairs = np.zeros(2 * max(n - 1, 1), dtype=np.int32)
        xf = np.zeros((max(n - 1, 1), 9), dtype=np.float64)
        k = _nonneg(lib().lsnFusionColorDiagnostics(self._h, int(tick), _ptr(conf), _ptr(cov), _ptr(pairs), _ptr(xf), stream or None), "lsnFusionColorDiagnostics")
        return {"confidence": conf[:self.pixels_per_tick], "coverage": cov,
                "pairs": [(int(pairs[2 * q]), int(pairs[2 * q + 1])) for q in range(k)], "transforms": xf[:k].copy()}

    def color_blend(self, depth_tol, min_confidence, d_depth, d_vertices, d_offsets, stream=0):
        """Colour blending across views in place on the clouds run() / run_mesh() wrote from d_depth (behind color_transfer() when both
        run); every tick on its own.  depth_tol <= 0 or min_confidence > 20: off."""
        _check(lib().lsnFusionColorBlend(self._h, int(depth_tol), int(min_confidence), d_depth, d_vertices, d_offsets, stream or None),
               "lsnFusionColorBlend")

    def color_blend_diagnostics(self, tick=0, stream=0):
        """What the last color_blend() did to one tick, per sensor: {"blended": int32[n] (vertices with at least one partner), "partners":
        int64[n] (partner terms), "abs_change": int64[n] (sum over R, G, B of |new - old|), "n_blended": int}."""
        n = self.n_maps
        blended, partners, change = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        k = _nonneg(lib().lsnFusionColorBlendDiagnostics(self._h, int(tick), _ptr(blended), _ptr(partners), _ptr(change), stream or None),
                    "lsnFusionColorBlendDiagnostics")
        return {"blended": blended, "partners": partners, "abs_change": change, "n_blended": k}

    def overlay_merge(self, d_depth, d_vertices, d_offsets, d_triangles, d_tri_offsets, stream=0):
        """Overlay merge (bgenerate_triangles) on the clouds run() / run_mesh() wrote from d_depth: rewrites the triangles and their
        offsets (run_mesh's layout); every tick on its own."""
        _check(lib().lsnFusionOverlayMerge(self._h, d_depth, d_vertices, d_offsets, d_triangles, d_tri_offsets, stream or None),
               "lsnFusionOverlayMerge")

    def overlay_diagnostics(self, tick=0, n_vertices=None, stream=0):
        """What the last overlay_merge() left for one tick: {"reprojected": uint16[pixels_per_tick] (step 1), "merged": uint16
        [pixels_per_tick] (the final maps), "assigned": uint8[n_vertices] (point_assigned), "n_assigned": int}."""
        rep = np.zeros(max(self.pixels_per_tick, 1), dtype=np.uint16)
        mer = np.zeros(max(self.pixels_per_tick, 1), dtype=np.uint16)
        asg = np.zeros(max(int(self.capacity), 1), dtype=np.uint8)
        k = _nonneg(lib().lsnFusionOverlayDiagnostics(self._h, int(tick), _ptr(rep), _ptr(mer), _ptr(asg), stream or None), "lsnFusionOverlayDiagnostics")
        nv = int(self.capacity) if n_vertices is None else int(n_vertices)
        return {"reprojected": rep[:self.pixels_per_tick], "merged": mer[:self.pixels_per_tick], "assigned": asg[:nv].copy(), "n_assigned": k}

    def outlier_filter(self, k, max_dist, d_depth, d_vertices, d_offsets, d_depth_out, stream=0):
        """Outlier filter on the clouds run() / run_mesh() wrote from d_depth: d_depth_out (may be d_depth) receives the maps with depth 0
        at the pixels of removed vertices; every sensor of every tick on its own.  Run run() / run_mesh() on d_depth_out next."""
        _check(lib().lsnFusionOutlierFilter(self._h, int(k), float(max_dist), d_depth, d_vertices, d_offsets, d_depth_out, stream or None),
               "lsnFusionOutlierFilter")

    def outlier_diagnostics(self, tick=0, n_vertices=None, stream=0):
        """What the last outlier_filter() decided for one tick: {"removed_per_sensor": int32[n], "removed": uint8[n_vertices] (flag per
        vertex of the filtered cloud), "exact_per_sensor": int32[n] (vertices the grid pass decided), "total": int}."""
        rps = np.zeros(max(self.n_maps, 1), dtype=np.int32)
        eps = np.zeros(max(self.n_maps, 1), dtype=np.int32)
        rem = np.zeros(max(int(self.capacity), 1), dtype=np.uint8)
        k = _nonneg(lib().lsnFusionOutlierDiagnostics(self._h, int(tick), _ptr(rps), _ptr(rem), _ptr(eps), stream or None), "lsnFusionOutlierDiagnostics")
        nv = int(self.capacity) if n_vertices is None else int(n_vertices)
        return {"removed_per_sensor": rps[:self.n_maps].copy(), "removed": rem[:nv].copy(), "exact_per_sensor": eps[:self.n_maps].copy(),
                "total": k}

    def flying_pixels(self, neighbourhood, threshold, d_depth_in, d_depth_out, stream=0):
        """Flying-pixel filter on every map of the plan, d_depth_in into d_depth_out (out of place: overlapping buffers are refused;
        neighbourhood <= 0 copies).  Run radial_correct_to() / run() on d_depth_out next."""
        _check(lib().lsnFusionFlyingPixels(self._h, int(neighbourhood), int(threshold), d_depth_in, d_depth_out, stream or None),
               "lsnFusionFlyingPixels")

    def flying_diagnostics(self, tick=0, stream=0):
        """What the last flying_pixels() removed in one tick: (pixels of depth != 0 set to 0 per sensor int32[n], their sum)."""
        rps = np.zeros(max(self.n_maps, 1), dtype=np.int32)
        k = _nonneg(lib().lsnFusionFlyingDiagnostics(self._h, int(tick), _ptr(rps), stream or None), "lsnFusionFlyingDiagnostics")
        return rps[:self.n_maps].copy(), k

    def set_depth_smooth(self, radius, spatial=None, range_table=None):
        """The plan's depth smoothing (lsnFusionSetDepthSmooth): radius 1..3 with a spatial table of (2 radius + 1)^2 and a range table of
        1..1024 uint16 entries <= 4095 (e.g. depth_smooth_gaussian's); radius <= 0: off.  A refused setting leaves the previous one."""
        ws = _as(np.zeros(1) if spatial is None else spatial, np.uint16).ravel()
        wr = _as(np.zeros(1) if range_table is None else range_table, np.uint16).ravel()
        if int(radius) >= 1 and ws.size != (2 * int(radius) + 1) ** 2:
            raise NativeUtilsError(f"set_depth_smooth: the spatial table of radius {radius} has {(2 * int(radius) + 1) ** 2} entries, not {ws.size}")
        _check(lib().lsnFusionSetDepthSmooth(self._h, int(radius), _ptr(ws), _ptr(wr), int(wr.size)), "lsnFusionSetDepthSmooth")

    def depth_smooth(self, d_depth_in, d_depth_out, stream=0):
        """Depth smoothing on every map of the plan with the tables of set_depth_smooth(), d_depth_in into d_depth_out (out of place:
        overlapping buffers are refused; off copies).  Run radial_correct_to() / run() on d_depth_out next."""
        _check(lib().lsnFusionDepthSmooth(self._h, d_depth_in, d_depth_out, stream or None), "lsnFusionDepthSmooth")

    def depth_smooth_diagnostics(self, tick=0, stream=0):
        """What the last depth_smooth() did in one tick: (pixels with out != in per sensor int32[n], sum of |out - in| per sensor int64[n],
        the total of changed pixels)."""
        ch = np.zeros(max(self.n_maps, 1), dtype=np.int32)
        mv = np.zeros(max(self.n_maps, 1), dtype=np.int64)
        k = _nonneg(lib().lsnFusionDepthSmoothDiagnostics(self._h, int(tick), _ptr(ch), _ptr(mv), stream or None), "lsnFusionDepthSmoothDiagnostics")
        return ch[:self.n_maps].copy(), mv[:self.n_maps].copy(), k

    def set_temporal(self, alpha_q, delta=0, persist=0):
        """The plan's temporal depth filter (lsnFusionSetTemporal): alpha_q 1..256, delta 1..4095 mm, persist 0..255; alpha_q <= 0: off.  A
        refused setting leaves the previous one; changing the setting keeps the history."""
        _check(lib().lsnFusionSetTemporal(self._h, int(alpha_q), int(delta), int(persist)), "lsnFusionSetTemporal")

    def temporal(self, d_depth_in, d_depth_out, stream=0):
        """The temporal filter on every tick of the plan in order, d_depth_in into d_depth_out (the same pointer: in place; any other overlap
        is refused; off copies); the plan's history advances by n_ticks.  Run flying_pixels() / radial_correct_to() on d_depth_out next."""
        _check(lib().lsnFusionTemporal(self._h, d_depth_in, d_depth_out, stream or None), "lsnFusionTemporal")

    def temporal_reset(self, stream=0):
        _check(lib().lsnFusionTemporalReset(self._h, stream or None), "lsnFusionTemporalReset")

    def temporal_state(self, stream=0):
        """The history: uint32 [pixels per tick] (F | miss << 24) in the layout of one tick's depth maps."""
        st = np.zeros(max(self.capacity, 1), dtype=np.uint32)
        _check(lib().lsnFusionTemporalStateRead(self._h, _ptr(st), stream or None), "lsnFusionTemporalStateRead")
        return st[:self.capacity]

    def set_temporal_state(self, state, stream=0):
        st = _as(state, np.uint32).ravel()
        if st.size != self.capacity:
            raise NativeUtilsError(f"set_temporal_state: the history has {self.capacity} words, not {st.size}")
        _check(lib().lsnFusionTemporalStateWrite(self._h, _ptr(st), stream or None), "lsnFusionTemporalStateWrite")

    def temporal_diagnostics(self, tick=0, stream=0):
        """What the last temporal() did in one tick: int32 [n, 4] per sensor -- blended, restarted with history, filled, expired."""
        c = [np.zeros(max(self.n_maps, 1), dtype=np.int32) for _ in range(4)]
        _check(lib().lsnFusionTemporalDiagnostics(self._h, int(tick), *[_ptr(x) for x in c], stream or None), "lsnFusionTemporalDiagnostics")
        return np.stack(c, axis=1)[:self.n_maps]

    def set_background(self, margin, rel_q=0, min_pixels=0):
        """The plan's background subtraction (lsnFusionSetBackground): margin 1..4095 mm, rel_q 0..255 (1/1024), min_pixels 0..2^24 (<= 1: no
        blob pass); margin <= 0: off.  A refused setting leaves the previous one; changing the setting keeps the model."""
        _check(lib().lsnFusionSetBackground(self._h, int(margin), int(rel_q), int(min_pixels)), "lsnFusionSetBackground")

    def background_learn(self, d_depth, stream=0):
        """Folds every tick of d_depth into the plan's model (the smallest non-zero sample per pixel); writes no maps."""
        _check(lib().lsnFusionBackgroundLearn(self._h, d_depth, stream or None), "lsnFusionBackgroundLearn")

    def background(self, d_depth_in, d_depth_out, stream=0):
        """Background subtraction on every tick of the plan, d_depth_in into d_depth_out (the same pointer: in place; any other overlap is
        refused; off copies); the model is only read.  Run flying_pixels() / radial_correct_to() on d_depth_out next."""
        _check(lib().lsnFusionBackground(self._h, d_depth_in, d_depth_out, stream or None), "lsnFusionBackground")

    def background_reset(self, stream=0):
        _check(lib().lsnFusionBackgroundReset(self._h, stream or None), "lsnFusionBackgroundReset")

    def background_model(self, stream=0):
        """The model: uint16 [pixels per tick] in the layout of one tick's depth maps (0: nothing learned)."""
        m = np.zeros(max(self.capacity, 1), dtype=np.uint16)
        _check(lib().lsnFusionBackgroundModelRead(self._h, _ptr(m), stream or None), "lsnFusionBackgroundModelRead")
        return m[:self.capacity]

    def set_background_model(self, model, stream=0):
        m = _as(model, np.uint16).ravel()
        if m.size != self.capacity:
            raise NativeUtilsError(f"set_background_model: the model has {self.capacity} values, not {m.size}")
        _check(lib().lsnFusionBackgroundModelWrite(self._h, _ptr(m), stream or None), "lsnFusionBackgroundModelWrite")

    def background_diagnostics(self, tick=0, stream=0):
        """What the last background() did in one tick: int32 [n, 6] per sensor -- foreground kept, unknown kept, background removed,
        components, components removed, pixels removed by the blob pass."""
        c = [np.zeros(max(self.n_maps, 1), dtype=np.int32) for _ in range(6)]
        _check(lib().lsnFusionBackgroundDiagnostics(self._h, int(tick), *[_ptr(x) for x in c], stream or None), "lsnFusionBackgroundDiagnostics")
        return np.stack(c, axis=1)[:self.n_maps]

    def render_views(self, intr, wt, width, height, d_vertices, d_offsets, d_triangles, d_tri_offsets, d_depth_out, d_colors_out, stream=0):
        """Render view: every tick's merged mesh (d_triangles None / 0: its vertices as points) drawn from the virtual cameras of intr
        (7 floats per view) / wt (12 per view), each width x height, into d_depth_out [n_ticks][n_views][h][w] u16 and d_colors_out
        [...][3] u8 (device pointers).  Returns the number of views."""
        intr, wt = _as(intr, np.float32).ravel(), _as(wt, np.float32).ravel()
        n_views = intr.size // 7
        assert intr.size == 7 * n_views and wt.size == 12 * n_views
        _check(lib().lsnFusionRenderViews(self._h, n_views, _ptr(intr), _ptr(wt), int(width), int(height), d_vertices, d_offsets,
                                          d_triangles or None, d_tri_offsets or None, d_depth_out, d_colors_out, stream or None),
               "lsnFusionRenderViews")
        return n_views

    def render_diagnostics(self, tick=0, view=0, stream=0):
        """The last render_views() of (tick, view): {"drawn": primitives drawn, "large": triangles that took the work-list path, "pixels":
        pixels with depth != 0}."""
        d, l, p = C.c_int(0), C.c_int(0), C.c_int(0)
        _check(lib().lsnFusionRenderDiagnostics(self._h, int(tick), int(view), C.byref(d), C.byref(l), C.byref(p), stream or None),
               "lsnFusionRenderDiagnostics")
        return {"drawn": d.value, "large": l.value, "pixels": p.value}

    def simplify(self, cell, d_vertices, d_offsets, d_triangles, d_tri_offsets, d_vertices_out, d_offsets_out, d_triangles_out,
                 d_tri_offsets_out, d_remap_out=0, stream=0):
        """Mesh level of detail: every tick's merged mesh (d_triangles None / 0: its vertices alone) clustered on a grid of edge `cell`
        into the out buffers (run_mesh's layouts; d_remap_out: capacity ints per tick, optional).  Out of place; cell <= 0 copies."""
        _check(lib().lsnFusionSimplify(self._h, float(cell), d_vertices, d_offsets, d_triangles or None, d_tri_offsets or None, d_vertices_out,
                                       d_offsets_out, d_triangles_out or None, d_tri_offsets_out or None, d_remap_out or None, stream or None),
               "lsnFusionSimplify")

    def simplify_diagnostics(self, tick=0, stream=0):
        """The last simplify() of one tick: {"cells": occupied cells = vertices out, "unclustered": vertices that are a cell of their own,
        "dropped_triangles": triangles that collapsed or named a vertex out of range}."""
        c, u, d = C.c_int(0), C.c_int(0), C.c_int(0)
        _check(lib().lsnFusionSimplifyDiagnostics(self._h, int(tick), C.byref(c), C.byref(u), C.byref(d), stream or None),
               "lsnFusionSimplifyDiagnostics")
        return {"cells": c.value, "unclustered": u.value, "dropped_triangles": d.value}

    def fragments(self, min_vertices, d_vertices, d_offsets, d_triangles, d_tri_offsets, d_vertices_out, d_offsets_out, d_triangles_out,
                  d_tri_offsets_out, d_remap_out=0, d_labels_out=0, stream=0):
        """Fragment filter: the connected components of fewer than `min_vertices` vertices of every tick's merged mesh dropped, into the
        out buffers (run_mesh's layouts; d_remap_out, d_labels_out: capacity ints per tick, optional).  Out of place; min_vertices <= 1
        copies; a mesh without triangles (d_triangles 0) is refused."""
        _check(lib().lsnFusionFragments(self._h, int(min_vertices), d_vertices, d_offsets, d_triangles or None, d_tri_offsets or None,
                                        d_vertices_out or None, d_offsets_out or None, d_triangles_out or None, d_tri_offsets_out or None,
                                        d_remap_out or None, d_labels_out or None, stream or None), "lsnFusionFragments")

    def fragments_diagnostics(self, tick=0, stream=0):
        """The last fragments() of one tick: {"components", "removed_components", "removed_vertices", "dropped_triangles": triangles in
        minus triangles out}; all 0 after min_vertices <= 1."""
        c, r, v, d = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        _check(lib().lsnFusionFragmentsDiagnostics(self._h, int(tick), C.byref(c), C.byref(r), C.byref(v), C.byref(d), stream or None),
               "lsnFusionFragmentsDiagnostics")
        return {"components": c.value, "removed_components": r.value, "removed_vertices": v.value, "dropped_triangles": d.value}

    def normals(self, d_vertices, d_offsets, d_triangles, d_tri_offsets, d_normals_out, stream=0):
        """Vertex normals of every tick's merged mesh (run_mesh's layouts) into d_normals_out, float32 [n_ticks, capacity, 3]: area
        weighted, summed as 64-bit integers, so bit-exact in any order.  Out of place; a mesh without triangles (d_triangles 0) is refused."""
        _check(lib().lsnFusionNormals(self._h, d_vertices, d_offsets, d_triangles or None, d_tri_offsets or None, d_normals_out, stream or None),
               "lsnFusionNormals")

    def normals_diagnostics(self, tick=0, stream=0):
        """The last normals() of one tick: {"used": triangles that were summed, "skipped": triangles with an index out of range or a face
        component that is not finite and below 4096, "zero_normals": vertices whose normal is (0, 0, 0)}."""
        u, k, z = C.c_int(0), C.c_int(0), C.c_int(0)
        _check(lib().lsnFusionNormalsDiagnostics(self._h, int(tick), C.byref(u), C.byref(k), C.byref(z), stream or None),
               "lsnFusionNormalsDiagnostics")
        return {"used": u.value, "skipped": k.value, "zero_normals": z.value}

    def smooth(self, iterations, lam, mu, pin_boundary, d_vertices, d_offsets, d_triangles, d_tri_offsets, d_vertices_out, stream=0):
        """Taubin lambda|mu smoothing of every tick's merged mesh (run_mesh's layouts) into d_vertices_out, uint8 [n_ticks, capacity, 16]:
        `iterations` times a pass with `lam` and one with `mu` (0: plain Laplacian), open vertices pinned if asked; offsets and triangles
        stay the input's.  Out of place, asynchronous; DESIGN.md section 21."""
        _check(lib().lsnFusionSmooth(self._h, int(iterations), float(lam), float(mu), 1 if pin_boundary else 0, d_vertices, d_offsets,
                                     d_triangles or None, d_tri_offsets or None, d_vertices_out, stream or None), "lsnFusionSmooth")

    def smooth_diagnostics(self, tick=0, stream=0):
        """The last smooth() of one tick: {"used", "skipped": triangles of the last pass that entered the sums / did not, "pinned": open
        vertices held in place, "isolated": vertices without a used triangle in the last pass}."""
        u, k, p, z = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        _check(lib().lsnFusionSmoothDiagnostics(self._h, int(tick), C.byref(u), C.byref(k), C.byref(p), C.byref(z), stream or None),
               "lsnFusionSmoothDiagnostics")
        return {"used": u.value, "skipped": k.value, "pinned": p.value, "isolated": z.value}

    def thresholds(self, capacity=None, stream=0, copy=True):
        """Builds the per-pixel depth thresholds now.  Returns (table uint32[capacity] or None, build_ms); table is None when
        the plan does not use thresholds ($LSN_NO_THRESHOLDS=1)."""
        out = np.zeros(int(capacity or self.capacity), dtype=np.uint32) if copy else None
        ms = C.c_float(0)
        rc = _nonneg(lib().lsnFusionThresholds(self._h, _ptr(out) if copy else None, C.byref(ms), stream or None), "lsnFusionThresholds")
        return (None if rc == 1 else out), ms.value

    @property
    def tiles_per_tick(self):
        return int(lib().lsnFusionTilesPerTick(self._h))

    def pack_survivors(self, d_depth, d_colors, d_mask, d_depth_c, d_rgb_c, d_tile_prefix, d_offsets, stream=0):
        _check(lib().lsnFusionPackSurvivors(self._h, d_depth, d_colors, d_mask, d_depth_c, d_rgb_c, d_tile_prefix, d_offsets, stream or None),
               "lsnFusionPackSurvivors")

    def reconstruct(self, n_shards, maps_per_shard, d_masks, d_depth_c, d_rgb_c, slab, d_tile_prefix, d_shard_offsets, d_merged, d_merged_offsets,
                    stream=0):
        """Called on the whole-rig plan: rebuilds all shards' vertices from the gathered survivor streams."""
        _check(lib().lsnFusionReconstruct(self._h, int(n_shards), int(maps_per_shard), d_masks, d_depth_c, d_rgb_c, int(slab), d_tile_prefix,
                                          d_shard_offsets, d_merged, d_merged_offsets, stream or None), "lsnFusionReconstruct")

    def pack_survivors_run(self, d_depth, d_colors, d_mask, d_depth_c, d_rgb_c, d_tile_prefix, d_offsets, d_tick_base, stream=0):
        """pack_survivors with all ticks back to back (one contiguous run per shard); fills d_tick_base [n_ticks]."""
        _check(lib().lsnFusionPackSurvivorsRun(self._h, d_depth, d_colors, d_mask, d_depth_c, d_rgb_c, d_tile_prefix, d_offsets, d_tick_base,
                                               stream or None), "lsnFusionPackSurvivorsRun")

    def reconstruct_run(self, n_shards, maps_per_shard, d_masks, d_depth_c, d_rgb_c, run_len, d_tile_prefix, d_shard_offsets, d_merged,
                        d_merged_offsets, d_tick_base_scratch, stream=0):
        _check(lib().lsnFusionReconstructRun(self._h, int(n_shards), int(maps_per_shard), d_masks, d_depth_c, d_rgb_c, int(run_len), d_tile_prefix,
                                             d_shard_offsets, d_merged, d_merged_offsets, d_tick_base_scratch, stream or None),
               "lsnFusionReconstructRun")

    def lookback_failed(self, stream=0):
        return int(lib().lsnFusionLookbackFailed(self._h, stream))

    def check(self, stream=0):
        """The plan's sticky device-side error flag (0 fine, 1 look-back gave up, 2 inputs changed between count and write); clears it."""
        return int(lib().lsnFusionCheck(self._h, stream))

    def run_streamed(self, d_depth, d_colors, d_vertices, d_offsets, d_next_depth=None, stream=0):
        """This batch is written while the next batch's depth (already resident) is counted in the same kernel."""
        _check(lib().lsnFusionRunStreamed(self._h, d_depth, d_colors, d_vertices, d_offsets, d_next_depth, stream), "lsnFusionRunStreamed")

    def profile(self, enable=True, every=1):
        """HIP events around the dominant kernel of every launch sequence (every = 1) or of every n-th one."""
        _check(lib().lsnFusionProfile(self._h, max(1, int(every)) if enable else 0), "lsnFusionProfile")

    def kernel_stats(self, reset=True):
        avg, n = C.c_double(0), C.c_longlong(0)
        name = C.create_string_buffer(128)
        _check(lib().lsnFusionKernelStats(self._h, C.byref(avg), C.byref(n), name, len(name), 1 if reset else 0),
               "lsnFusionKernelStats")
        return {"kernel": name.value.decode(), "avg_ms": avg.value, "launches": n.value}


def merge_shards(device, n_shards, n_ticks, maps_per_shard, d_shards, shard_cap, d_shard_offsets, d_merged, merged_cap,
                 d_merged_offsets, stream=0):
    _check(lib().lsnMergeShards(int(device), int(n_shards), int(n_ticks), int(maps_per_shard), d_shards, int(shard_cap),
                                d_shard_offsets, d_merged, int(merged_cap), d_merged_offsets, stream), "lsnMergeShards")


def shard_rccl_path():
    """The file the library's nccl* entry points came from (an RCCL already mapped in the process is preferred)."""
    buf = C.create_string_buffer(1024)
    n = lib().lsnShardRcclPath(buf, len(buf))
    return buf.value.decode() if n >= 0 else None


def shard_unique_id():
    """128 bytes from rank 0's RCCL (lsnShardUniqueId); every rank passes the same ones to Shard()."""
    require_gpu()
    buf = (C.c_ubyte * 128)()
    _check(lib().lsnShardUniqueId(buf), "lsnShardUniqueId")
    return bytes(buf)


class Shard(_Handle):
    """lsnShard*: this rank's block of sensors in, the merged cloud of all sensors out (RCCL all-gathers inside the library)."""
    _destroy = "lsnShardDestroy"

    def __init__(self, device, rank, world, unique_id, n_ticks, widths, heights):
        """unique_id: rank 0's 128 bytes -> prepare + connect at once (lsnShardCreate); None -> lsnShardPrepare only, the caller
        connects (connect()) once every rank has reported that its own preparation worked."""
        require_gpu()
        w, h = _as(widths, np.int32), _as(heights, np.int32)
        self.n_ticks, self.n_maps, self.world, self.rank = int(n_ticks), len(w), int(world), int(rank)
        if unique_id is None:
            self._h = _handle(lib().lsnShardPrepare(int(device), self.rank, self.world, self.n_ticks, self.n_maps, _ptr(w), _ptr(h)), "lsnShardPrepare")
        else:
            idb = (C.c_ubyte * 128).from_buffer_copy(bytes(unique_id))
            self._h = _handle(lib().lsnShardCreate(int(device), self.rank, self.world, idb, self.n_ticks, self.n_maps, _ptr(w), _ptr(h)),
                              "lsnShardCreate")
        self.capacity = int(lib().lsnShardMergedCapacity(self._h))

    def connect(self, unique_id):
        idb = (C.c_ubyte * 128).from_buffer_copy(bytes(unique_id))
        _check(lib().lsnShardConnect(self._h, idb), "lsnShardConnect")

    def set_params(self, intr_all, wt_all, bounds, stream=0):
        _set_params("lsnShardSetParams", self._h, self.n_maps, intr_all, wt_all, bounds, stream)

    def step(self, d_depth_local, d_colors_local, stream=0):
        """Returns (device pointer of the merged cloud [n_ticks][capacity] vertices, device pointer of its offsets [n_ticks][n_maps + 1])."""
        mv, mo = C.c_void_p(), C.c_void_p()
        _check(lib().lsnShardStep(self._h, d_depth_local, d_colors_local, C.byref(mv), C.byref(mo), stream), "lsnShardStep")
        return mv.value, mo.value

    def last_bytes_sent(self):
        return int(lib().lsnShardLastBytesSent(self._h))

    def ranks_seen(self):
        """The rank count the connected communicator itself reports (ncclCommCount); -1 if it cannot say."""
        return int(lib().lsnShardRanksSeen(self._h))

    def plan(self, whole=True):
        """A non-owning FusionPlan view of one of the handle's plans (profile / kernel_stats / check only)."""
        v = object.__new__(FusionPlan)
        v._h = lib().lsnShardPlan(self._h, 1 if whole else 0)
        v.close = lambda: None   # (also what the view's __del__ calls: the handle stays the Shard's)
        return v


NN_BRUTE, NN_GRID = 0, 1


class TickPipeline(_Handle):
    """lsnTick*: the chained tick (radial correction out of place -> vertices -> triangulation) of n_ticks x n_maps frames in HBM as one call."""
    _destroy = "lsnTickDestroy"

    def __init__(self, device, n_ticks, widths, heights):
        require_gpu()
        self.widths, self.heights = _as(widths, np.int32), _as(heights, np.int32)
        self.n_ticks, self.n_maps = int(n_ticks), len(self.widths)
        self._h = _handle(lib().lsnTickCreate(int(device), self.n_ticks, self.n_maps, _ptr(self.widths), _ptr(self.heights)), "lsnTickCreate")
        self.capacity = int(lib().lsnTickCapacity(self._h))
        self.tri_capacity = int(lib().lsnTickTriangleCapacity(self._h))
        self.parts = int(lib().lsnTickParts(self._h))

    def set_params(self, intr, wt, bounds, stream=0):
        _set_params("lsnTickSetParams", self._h, self.n_maps, intr, wt, bounds, stream)

    def set_flying_pixels(self, neighbourhood, threshold):
        """The flying-pixel filter as the first stage of run() (neighbourhood <= 0: off): filter -> radial correction -> vertices ->
        triangles; d_depth_corr then receives the filtered and corrected maps."""
        _check(lib().lsnTickSetFlyingPixels(self._h, int(neighbourhood), int(threshold)), "lsnTickSetFlyingPixels")

    def set_depth_smooth(self, radius, sigma_s=0.0, sigma_r=0.0):
        """Depth smoothing with the Gaussian tables of (radius, sigma_s, sigma_r) as a stage of run() (radius <= 0: off): flying pixels
        (if set) -> depth smoothing -> radial correction -> vertices -> triangles."""
        _check(lib().lsnTickSetDepthSmooth(self._h, int(radius), float(sigma_s), float(sigma_r)), "lsnTickSetDepthSmooth")

    def set_temporal(self, alpha_q, delta=0, persist=0):
        """The temporal depth filter as the first stage of run() (alpha_q <= 0: off): temporal -> flying pixels (if set) -> depth smoothing (if
        set) -> radial correction -> vertices -> triangles.  The tick object's one history continues from run to run."""
        _check(lib().lsnTickSetTemporal(self._h, int(alpha_q), int(delta), int(persist)), "lsnTickSetTemporal")

    def temporal_reset(self, stream=0):
        _check(lib().lsnTickTemporalReset(self._h, stream or None), "lsnTickTemporalReset")

    def set_background(self, margin, rel_q=0, min_pixels=0):
        """Background subtraction as the stage of run() behind the temporal filter (margin <= 0: off).  The tick object owns one model."""
        _check(lib().lsnTickSetBackground(self._h, int(margin), int(rel_q), int(min_pixels)), "lsnTickSetBackground")

    def background_learn(self, d_depth_in, stream=0):
        """Folds the batch at d_depth_in (through the temporal filter, if that is set) into the tick object's model; runs nothing else."""
        _check(lib().lsnTickBackgroundLearn(self._h, d_depth_in, stream or None), "lsnTickBackgroundLearn")

    def background_reset(self, stream=0):
        _check(lib().lsnTickBackgroundReset(self._h, stream or None), "lsnTickBackgroundReset")

    def run(self, d_depth_in, d_colors_in, d_depth_corr, d_colors_corr, d_vertices, d_offsets, d_triangles, d_tri_offsets, stream=0):
        _check(lib().lsnTickRun(self._h, d_depth_in, d_colors_in, d_depth_corr, d_colors_corr, d_vertices, d_offsets, d_triangles, d_tri_offsets, stream),
               "lsnTickRun")


class IcpWorkspace(_Handle):
    """lsnIcp*: device-resident ICP for clouds up to (max_n1, max_n2)."""
    _destroy = "lsnIcpDestroy"

    def __init__(self, device, max_n1, max_n2):
        require_gpu()
        self.device = int(device)
        self._h = _handle(lib().lsnIcpCreate(self.device, int(max_n1), int(max_n2)), "lsnIcpCreate")

    def run(self, d_verts1, n1, d_verts2, n2, d_R, d_t, max_iter=10, nn_mode=NN_GRID, stream=0):
        _check(lib().lsnIcpRun(self._h, d_verts1, int(n1), d_verts2, int(n2), d_R, d_t, int(max_iter), int(nn_mode), stream),
               "lsnIcpRun")

    def run_plane(self, d_verts1, d_normals1, n1, d_verts2, n2, d_R, d_t, max_iter=10, nn_mode=NN_GRID, stream=0):
        """lsnIcpRunPlane: run() with the point-to-plane residual; d_normals1: the target's normals, n1 x 3 floats on the device."""
        _check(lib().lsnIcpRunPlane(self._h, d_verts1, d_normals1, int(n1), d_verts2, int(n2), d_R, d_t, int(max_iter), int(nn_mode), stream),
               "lsnIcpRunPlane")

    def nearest(self, d_verts1, n1, d_verts2, n2, d_idx, d_dist2, nn_mode=NN_GRID, stream=0):
        _check(lib().lsnIcpNearest(self._h, d_verts1, int(n1), d_verts2, int(n2), d_idx, d_dist2, int(nn_mode), stream),
               "lsnIcpNearest")

    def set_profiling(self, on=True):
        _check(lib().lsnIcpSetProfiling(self._h, 1 if on else 0), "lsnIcpSetProfiling")

    def profile(self, stream=0):
        """Milliseconds of the last profiled run(): {build, nn, match_reduce_solve, final_apply} (synchronises the stream)."""
        ms = np.zeros(4, dtype=np.float32)
        _nonneg(lib().lsnIcpProfile(self._h, _ptr(ms), stream), "lsnIcpProfile")
        return {"build": float(ms[0]), "nn": float(ms[1]), "match_reduce_solve": float(ms[2]), "final_apply": float(ms[3])}

    def near_resolved(self, stream=0):
        """Queries of the last voxel-grid NN step that the near path settled (diagnostic; synchronises the stream)."""
        n = _nonneg(lib().lsnIcpNearResolved(self._h, stream), "lsnIcpNearResolved")
        return int(n)

    def trace(self, max_iters, stream=0):
        out = np.zeros((max(max_iters, 1), 16), dtype=np.float32)
        n = _nonneg(lib().lsnIcpTrace(self._h, _ptr(out), int(max_iters), stream), "lsnIcpTrace")
        return out[:n]


# ----------------------------------------------------------------------------------------------------------
# Part 3: wire / disk formats either side of the path
# ----------------------------------------------------------------------------------------------------------

class TransferPacker(_Handle):
    """LsnTransfer: builds the TransferSocket.SendFrame byte stream (TransferSocket.cs:50-104; chunks as
    TransferServer.cs:177-270) on the device."""
    _destroy = "lsnTransferDestroy"
    h = property(lambda self: self._h, doc="the LsnTransfer handle (None once closed)")

    def __init__(self, device, max_vertices, max_triangles):
        require_gpu()
        self._h = _handle(lib().lsnTransferCreate(int(device), int(max_vertices), int(max_triangles)), "lsnTransferCreate")

    def pack(self, d_vertices, n_vertices, d_triangles, n_triangles, d_out, out_cap, stream=0):
        n = _nonneg(lib().lsnTransferPack(self._h, d_vertices, int(n_vertices), d_triangles or None, int(n_triangles), d_out, int(out_cap), stream or None), "lsnTransferPack")
        return int(n)

    def last_path(self):
        """0 vertices only, 1 all chunks from one prefix sum, 2 chunk after chunk (lsnTransferLastPath)."""
        return int(lib().lsnTransferLastPath(self._h))


def transfer_frame_bound(n_vertices, n_triangles):
    return int(lib().lsnTransferFrameBound(int(n_vertices), int(n_triangles)))


def ply_binary_bytes(n_vertices, n_triangles):
    return int(lib().lsnPlyBinaryBytes(int(n_vertices), int(n_triangles)))


def ply_pack(device, d_vertices, n_vertices, d_triangles, n_triangles, d_out, out_cap, stream=0):
    require_gpu()
    n = _nonneg(lib().lsnPlyPack(int(device), d_vertices, int(n_vertices), d_triangles or None, int(n_triangles), d_out, int(out_cap), stream or None), "lsnPlyPack")
    return int(n)


def ply_normals_bytes(n_vertices, n_triangles):
    """The exact length of lsnPlyPackNormals' file: lsnPlyPack's with nx, ny, nz in the header and 27-byte vertex records."""
    return int(lib().lsnPlyNormalsBytes(int(n_vertices), int(n_triangles)))


def ply_pack_normals(device, d_vertices, d_normals, n_vertices, d_triangles, n_triangles, d_out, out_cap, stream=0):
    require_gpu()
    n = _nonneg(lib().lsnPlyPackNormals(int(device), d_vertices, d_normals, int(n_vertices), d_triangles or None, int(n_triangles), d_out,
                                        int(out_cap), stream or None), "lsnPlyPackNormals")
    return int(n)


def _last_mesh(fn, what):
    require_gpu()
    cap = _nonneg(fn(None, 0), what)
    out = np.zeros(cap, dtype=np.uint8)
    return out[:_nonneg(fn(_ptr(out), cap), what)].tobytes()


def last_mesh_transfer_frame():
    """SendFrame stream (TransferSocket.cs:50-104) of the mesh the last merge call returned, built in HBM."""
    return _last_mesh(lib().lsnLastMeshTransferFrame, "lsnLastMeshTransferFrame")


def last_mesh_ply():
    """Binary PLY file image (Utils.cs:222-262) of the mesh the last merge call returned, built in HBM."""
    return _last_mesh(lib().lsnLastMeshPly, "lsnLastMeshPly")


def last_mesh_transfer_frame_lod(cell):
    """lsnLastMeshTransferFrameLod: the SendFrame stream of that mesh after vertex clustering with cell size `cell` (<= 0: as it is)."""
    fn = lib().lsnLastMeshTransferFrameLod
    return _last_mesh(lambda out, cap: fn(float(cell), out, cap), "lsnLastMeshTransferFrameLod")


def last_mesh_ply_lod(cell):
    """lsnLastMeshPlyLod: the binary PLY file image of that mesh after vertex clustering with cell size `cell` (<= 0: as it is)."""
    fn = lib().lsnLastMeshPlyLod
    return _last_mesh(lambda out, cap: fn(float(cell), out, cap), "lsnLastMeshPlyLod")


def last_mesh_ply_normals(cell=0.0):
    """lsnLastMeshPlyNormals: the binary PLY file image of that mesh with vertex normals, after vertex clustering with cell size `cell`
    (<= 0: as it is).  A mesh without triangles is an error."""
    fn = lib().lsnLastMeshPlyNormals
    return _last_mesh(lambda out, cap: fn(float(cell), out, cap), "lsnLastMeshPlyNormals")


def last_mesh_transfer_frame_fragments(min_vertices, cell=0.0):
    """lsnLastMeshTransferFrameFragments: the SendFrame stream of that mesh after the fragment filter with `min_vertices` (<= 1: off), then
    vertex clustering with cell size `cell` (<= 0: off)."""
    fn = lib().lsnLastMeshTransferFrameFragments
    return _last_mesh(lambda out, cap: fn(int(min_vertices), float(cell), out, cap), "lsnLastMeshTransferFrameFragments")


def last_mesh_ply_fragments(min_vertices, cell=0.0, with_normals=False):
    """lsnLastMeshPlyFragments: the binary PLY file image of that mesh after the fragment filter with `min_vertices` (<= 1: off), then
    vertex clustering with cell size `cell` (<= 0: off), with vertex normals if asked."""
    fn = lib().lsnLastMeshPlyFragments
    return _last_mesh(lambda out, cap: fn(int(min_vertices), float(cell), 1 if with_normals else 0, out, cap), "lsnLastMeshPlyFragments")


def last_mesh_ply_smooth(min_vertices=0, cell=0.0, iterations=10, lam=0.5, mu=-0.53, pin_boundary=True, with_normals=False):
    """lsnLastMeshPlySmooth: last_mesh_ply_fragments with Taubin smoothing (iterations <= 0: off) between the level of detail and the
    normals."""
    fn = lib().lsnLastMeshPlySmooth
    return _last_mesh(lambda out, cap: fn(int(min_vertices), float(cell), int(iterations), float(lam), float(mu), 1 if pin_boundary else 0,
                                          1 if with_normals else 0, out, cap), "lsnLastMeshPlySmooth")


def last_mesh_transfer_frame_smooth(min_vertices=0, cell=0.0, iterations=10, lam=0.5, mu=-0.53, pin_boundary=True):
    """lsnLastMeshTransferFrameSmooth: last_mesh_transfer_frame_fragments with Taubin smoothing (iterations <= 0: off) behind the level
    of detail."""
    fn = lib().lsnLastMeshTransferFrameSmooth
    return _last_mesh(lambda out, cap: fn(int(min_vertices), float(cell), int(iterations), float(lam), float(mu), 1 if pin_boundary else 0,
                                          out, cap), "lsnLastMeshTransferFrameSmooth")


def last_mesh_render_view(intr7, wt12, width, height, points_only=False):
    """lsnLastMeshRenderView: one view of the mesh the calling thread's last mesh call returned, rendered in HBM.  Returns (depth uint16
    [h, w], rgb uint8 [h, w, 3], pixels with depth != 0)."""
    require_gpu()
    intr, wt = _as(intr7, np.float32).ravel(), _as(wt12, np.float32).ravel()
    assert intr.size == 7 and wt.size == 12
    w, h = int(width), int(height)
    depth = np.zeros((max(h, 0), max(w, 0)), dtype=np.uint16)
    rgb = np.zeros((max(h, 0), max(w, 0), 3), dtype=np.uint8)
    n = _nonneg(lib().lsnLastMeshRenderView(_ptr(intr), _ptr(wt), w, h, 1 if points_only else 0, _ptr(depth), _ptr(rgb)), "lsnLastMeshRenderView")
    return depth, rgb, int(n)


def zstd_available():
    return bool(lib().lsnZstdAvailable())


def frame_parse_header(header16):
    """Returns FrameInfo, or None for the "no more frames" header (payload_bytes <= 0)."""
    buf = np.frombuffer(bytes(header16[:16]), dtype=np.uint8)
    if buf.size != 16:
        raise NativeUtilsError("a frame header is 16 bytes")
    info = FrameInfo()
    rc = _nonneg(lib().lsnFrameParseHeader(_ptr(buf), C.byref(info)), "lsnFrameParseHeader")
    return None if rc == 1 else info


def frame_decode(message):
    """One whole frame message (header + payload) -> (depth u16 [h,w], rgb u8 [h,w,3], bodies bytes, n_bodies)."""
    msg = np.frombuffer(bytes(message), dtype=np.uint8)
    info = frame_parse_header(msg[:16])
    if info is None:
        return None
    if 16 + info.payload_bytes > msg.size:
        raise NativeUtilsError("frame message shorter than its header says")
    w, h = info.width, info.height
    depth = np.zeros((h, w), dtype=np.uint16)
    rgb = np.zeros((h, w, 3), dtype=np.uint8)
    bodies = np.zeros(1 << 16, dtype=np.uint8)
    nb = C.c_int(0)
    payload = np.ascontiguousarray(msg[16:16 + info.payload_bytes])
    bl = _nonneg(lib().lsnFrameDecode(_ptr(payload), info.payload_bytes, info.compressed, w, h, _ptr(depth), _ptr(rgb), _ptr(bodies), bodies.size, C.byref(nb)), "lsnFrameDecode")
    return depth, rgb, bodies[:bl].tobytes(), nb.value


def frame_encode(depth, rgb, bodies=None, compression_level=0):
    depth = _as(depth, np.uint16)
    h, w = depth.shape
    rgb = _as(rgb, np.uint8).reshape(h, w, 3)
    b = np.frombuffer(bodies, dtype=np.uint8) if bodies else None
    out = np.zeros(16 + 5 * w * h + (b.size if b is not None else 4) + 1024 + (w * h * 5) // 64, dtype=np.uint8)
    n = _nonneg(lib().lsnFrameEncode(_ptr(depth), _ptr(rgb), w, h, _ptr(b) if b is not None else None, b.size if b is not None else 0,
                                     int(compression_level), _ptr(out), out.size), "lsnFrameEncode")
    return out[:n].tobytes()


def recording_frames(file_bytes):
    """Iterates (timestamp_ms, frame message bytes) over the memory image of a client recording file."""
    buf = np.frombuffer(file_bytes, dtype=np.uint8)
    pos = 0
    off, ln, ts = C.c_longlong(0), C.c_int(0), C.c_int(0)
    while True:
        nxt = lib().lsnRecordingNext(_ptr(buf), buf.size, pos, C.byref(off), C.byref(ln), C.byref(ts))
        if nxt < 0:
            err = last_error()
            if err:
                raise NativeUtilsError(err)
            return
        yield ts.value, buf[off.value:off.value + ln.value].tobytes()
        pos = nxt


def recording_append(frame, timestamp_ms):
    f = np.frombuffer(bytes(frame), dtype=np.uint8)
    out = np.zeros(f.size + 96, dtype=np.uint8)
    n = _nonneg(lib().lsnRecordingAppend(_ptr(out), out.size, _ptr(f) if f.size else None, f.size, int(timestamp_ms)), "lsnRecordingAppend")
    return out[:n].tobytes()
