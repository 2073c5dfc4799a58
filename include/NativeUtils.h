/*
 * NativeUtils.h -- C-ABI of libNativeUtils.so, the MI355X-native drop-in for LiveScan3D's NativeUtils.dll
 * on the per-tick fusion path (depth -> XYZ unprojection, R(p+t), AABB crop, raster-order merged cloud, ICP).
 *
 * Part 1 are the reference's own exports, same names, argument order and meaning, so LiveScanServer's
 * P/Invoke declarations bind unchanged (LiveScanServer/KinectServer.cs:35-60, MainWindowForm.cs:42-43).
 * Part 2 is the device-resident API the same code runs on (plain pointers and sizes; no torch / HIP types):
 * what a host that already keeps frames in HBM (bench.py, the multi-GPU harness) calls.
 *
 * Nothing here throws; on failure the exports leave an empty mesh / untouched R,t and lsnGetLastError()
 * tells why.  There is NO CPU fallback: without a usable HIP device every compute entry point fails loudly.
 *
 * Paths in comments are relative to the reference repository root.
 */
#ifndef LSN_NATIVEUTILS_H
#define LSN_NATIVEUTILS_H

#include <stdbool.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------------
 * Part 1 -- the reference's exports
 * ------------------------------------------------------------------------------------------------------- */

/* include/NativeUtils/depthprocessing.h:29-33 -- 16 bytes, what KinectServer.CopyMeshToVerticesWithColoursArray
 * copies out (KinectServer.cs:376-389). */
typedef struct VertexC4ubV3f {
    unsigned char R, G, B, A;
    float X, Y, Z;
} VertexC4ubV3f;

/* include/NativeUtils/depthprocessing.h:42-48 (C# mirror LiveScanServer/Utils.cs:335-342) -- 32 bytes on LP64. */
typedef struct Mesh {
    int nVertices;
    VertexC4ubV3f *vertices;
    int nTriangles;
    int *triangles;
} Mesh;

/* include/NativeUtils/icp.h:15-18 */
typedef struct Point3f {
    float X, Y, Z;
} Point3f;

/* Replaces generateVerticesFromDepthMap, include/NativeUtils/depthprocessing.h:103-105
 * (src/NativeUtils/depthprocessing.cpp:1631-1657).  depth_maps / depth_colors are the concatenated per-sensor
 * buffers (u16 LE [h][w] / RGB8 [h][w][3]); intr_params 7 floats per sensor {cx,cy,fx,fy,r2,r4,r6};
 * wtransform_params 12 floats per sensor {t[3], R[3][3] row-major}, p' = R (p + t).
 * out_mesh->vertices is host memory owned by the library until deleteMesh; nTriangles = 0. */
void generateVerticesFromDepthMap(unsigned char *depth_maps, unsigned char *depth_colors, int *widths, int *heights,
                                  float *intr_params, float *wtransform_params, Mesh *out_mesh,
                                  float minX, float minY, float minZ, float maxX, float maxY, float maxZ,
                                  int depth_map_index);

/* Replaces generateMeshFromDepthMaps, include/NativeUtils/depthprocessing.h:108-110
 * (src/NativeUtils/depthprocessing.cpp:1715-1792).  In scope: the vertices of all sensors, cropped, in sensor
 * order then raster order, and the triangles of the reference's always-on triangulation (meshGenerator.cpp; indices
 * into `vertices`, reference order) -- i.e. the reference with both flags false.
 * bcolor_transfer = true runs the reference's colour transfer (confidence maps, pairwise coverage, greedy pairing,
 * per-channel mean / mean-absolute-deviation transfer in RGB; depthprocessing.cpp:263-385,1387-1575, colorcorrection.cpp)
 * on the device before the mesh leaves it: only the R,G,B bytes of the corrected sensors' vertices change (as
 * lsnFusionColorTransfer below; the call runs on one device even with $LSN_HOST_DEVICES).  bgenerate_triangles = true (the
 * cross-view overlay merge) is an opt-in, see lsnSetOverlayMerge: while the switch is off (the default) the call returns the
 * unmerged mesh and reports the flag through lsnGetLastError(); while it is on it returns the merged mesh (as lsnFusionOverlayMerge
 * below: same vertices, other triangles; one device; every sensor of the same size, else the unmerged mesh and a message). */
void generateMeshFromDepthMaps(int n_maps, unsigned char *depth_maps, unsigned char *depth_colors, int *widths,
                               int *heights, float *intr_params, float *wtransform_params, Mesh *out_mesh,
                               bool bcolor_transfer, float minX, float minY, float minZ, float maxX, float maxY,
                               float maxZ, bool bgenerate_triangles);

/* Replaces depthMapAndColorSetRadialCorrection, include/NativeUtils/depthprocessing.h:111
 * (src/NativeUtils/depthprocessing.cpp:191-261,1794-1815): radial-distortion correction of every sensor's depth map and
 * colours, in place in the caller's host arrays (forward warp, last writer wins; raster-order in-place hole closing). */
void depthMapAndColorSetRadialCorrection(int n_maps, unsigned char *depth_maps, unsigned char *depth_colors, int *widths,
                                         int *heights, float *intr_params);

/* Extension for hosts that want one call per tick: LiveScanServer's tick is depthMapAndColorSetRadialCorrection followed by
 * generateMeshFromDepthMaps on the same arrays (LiveScanServer/KinectServer.cs:518-525, then :354-374), which sends the same
 * 8.7 MB of frames over PCIe twice.  This export does both with ONE upload: radial correction on the device, then the merge
 * call (flags false, false; vertices + triangles) on the corrected frames.  write_back_corrected != 0 also writes the corrected
 * maps back into depth_maps / depth_colors, as the separate export does (KinectServer keeps them, e.g. for recording);
 * 0 leaves the caller's arrays untouched.  Result = the two reference exports called one after the other, bit for bit. */
void lsnCorrectAndGenerateMesh(int n_maps, unsigned char *depth_maps, unsigned char *depth_colors, int *widths, int *heights,
                               float *intr_params, float *wtransform_params, Mesh *out_mesh, float minX, float minY, float minZ,
                               float maxX, float maxY, float maxZ, int write_back_corrected);

/* Extension: LiveScanServer's "Refine calibration" (refineWorker_DoWork, LiveScanServer/MainWindowForm.cs:304-416, fed by
 * KinectServer.GetLatestFrameVerticesOnly, KinectServer.cs:527-554) as ONE call.  Through the reference's exports that path is the radial
 * export, n x generateVerticesFromDepthMap, a host loop that strips X, Y, Z out of the vertices (:318-327) and the ICP loop: every point
 * crosses PCIe three times.  Here the frames (the arrays of generateMeshFromDepthMaps) go up once and the clouds never leave the device:
 * all sensors are fused with the crop box, vertices only, into one merged cloud in HBM -- sensor i's block is byte for byte what
 * generateVerticesFromDepthMap(..., i) returns at that moment, the outlier filter (lsnSetOutlierFilter) included -- the blocks are stripped
 * to packed XYZ on the device and refined by lsnRefine's Gauss-Seidel loop.  Runs on the lane of the single-sensor calls and on ONE device,
 * also under $LSN_HOST_DEVICES.
 *   correct_radial  0: the frames are already corrected (the reference's order: CorrectRadialDistortionsForDepthMaps, then the vertices);
 *                   != 0: the flying-pixel filter (lsnSetFlyingPixelFilter) and the radial correction run on the device first, as in
 *                   lsnCorrectAndGenerateMesh.  The caller's frames are never written.
 *   wtransform_refined (12 floats per sensor, packed as wtransform_params; may be wtransform_params itself; nullable) receives the world
 *                   transforms after the pose composition of MainWindowForm.cs:382-410; camera_R (n x 9) / camera_t (n x 3), in/out,
 *                   nullable, are updated like cameraPoses[i] (:394, :407); Rs_out / Ts_out as in lsnRefine.
 *   clouds_out (room for sum(w * h) x 3 floats, nullable) / counts_out (n_maps ints, nullable) receive the refined clouds, sensor blocks in
 *                   sensor order, and their point counts: they exist so that the call can be checked; LiveScanServer needs neither.
 * Returns 0, also when there is nothing to refine (lsnRefine's rule: fewer than two sensors, a sensor with no vertex inside the crop box,
 * n_refine_iters <= 0 or n_icp_iters <= 0): then Rs = I, Ts = 0, the poses are composed with those and the clouds come back unrefined.
 * Returns -1 with the message set and NO output array touched on failure; without a HIP device that is what happens (no CPU path).
 * It is NOT a mesh call: it returns no Mesh and leaves its lane without a "last mesh" -- lsnLastMesh* on a thread whose last call was this
 * one report that no mesh is resident. */
int lsnRefineFromDepthMaps(int n_maps, unsigned char *depth_maps, unsigned char *depth_colors, int *widths, int *heights,
                           float *intr_params, float *wtransform_params, float minX, float minY, float minZ, float maxX, float maxY,
                           float maxZ, int correct_radial, int n_refine_iters, int n_icp_iters, float *wtransform_refined,
                           float *camera_R, float *camera_t, float *Rs_out, float *Ts_out, float *clouds_out, int *counts_out);

/* Host-only (no device needed), for tests and for operators who want to see it: the upload schedule a merge call (radial = 0), a
 * call that starts with the radial correction and goes on to the fusion (radial = 1: lsnCorrectAndGenerateMesh) or the radial export alone
 * (radial = 2: depthMapAndColorSetRadialCorrection) follows for sensors [first, first + count) of these frames, written to buf
 * as text -- e.g. "D[0-2] C[0-2] | D[3-7] C[3-5] | C[6-7]": runs of the depth / colour arrays in upload order (a pageable copy of
 * >= 1 MiB is pinned in place by the runtime, a smaller one staged at a quarter of the rate), `|` where a group of sensors is complete on
 * the device and launched.  sensors_per_group = 0: by size (the default); > 0: forced, like $LSN_HOST_GROUP.  Returns the number of
 * groups, -1 on bad arguments. */
int lsnHostScheduleDescribe(int n_maps, const int *widths, const int *heights, int first, int count, int radial, int sensors_per_group,
                            char *buf, int len);

/* Merge calls sharded over several devices.  $LSN_HOST_DEVICES=a,b,... (>= 2 entries, read at the first call; an entry may repeat):
 * generateMeshFromDepthMaps and lsnCorrectAndGenerateMesh give every listed device one contiguous block of the call's sensors -- uploaded
 * over that device's link, fused there, and stored by its kernels over its link into the SAME pinned Mesh blocks, behind the blocks
 * before it (formMesh's sensor order and triangle rebase, src/NativeUtils/depthprocessing.cpp:1594-1626; the reference's std::thread per
 * sensor, :708-733, with a device where it has a thread).  The mesh returned is byte for byte the one-device mesh.
 * lsnHostShardDescribe (host-only): how n_maps sensors are cut over n_devices (0 = as configured by the environment) -- text such as
 * "0:[0-3] 1:[4-7]" into buf, the block bounds into first_out (n_devices + 1 ints; may be NULL).  Returns the number of shards, -1 on
 * bad arguments. */
int lsnHostShardDescribe(int n_maps, int n_devices, int *first_out, char *buf, int len);
/* Measurement aid.  With $LSN_HOST_SHARD_SOLO=1 (read at the first sharded call) the parts of a sharded call run one after the other on
 * the calling thread, each alone on the link, and lsnHostShardPartMicros returns the wall time of every part of the last such call
 * (microseconds; `n` = room in `out`; returns the number of parts, 0 if there was no such call).  What a one-GPU box can say about a call
 * on several devices: each part's own cost on a link of its own; the call would take about as long as its slowest part. */
int lsnHostShardPartMicros(long long *out, int n);

/* Test hooks (no device needed).  lsnTestFaultPoints: how many fault points of a kind the process has passed (0 = guarded entries,
 * 1 = device / pinned allocations; $LSN_TEST_THROW / $LSN_TEST_FAIL_ALLOC = n make the n-th one throw std::bad_alloc inside the export).
 * lsnHostPoolStats: the pool of pinned mesh blocks -- blocks out with callers (a block a failed call did not return would stay here),
 * blocks waiting for reuse, bytes out; any pointer may be NULL. */
long long lsnTestFaultPoints(int kind);
int lsnHostPoolStats(int *live_blocks, int *pooled_blocks, long long *live_bytes);

/* Replaces createMesh / deleteMesh, src/NativeUtils/depthprocessing.cpp:1818-1835.  deleteMesh releases the two
 * arrays only (not the struct) and, unlike the reference, also nulls them so a second call is harmless. */
Mesh *createMesh(void);
void deleteMesh(Mesh *mesh);

/* Replaces ICP, include/NativeUtils/icp.h:65 (src/NativeUtils/icp.cpp:75-177): point-to-point ICP with exact
 * nearest neighbours, one-to-one matching, 2.5-sigma rejection on squared distances and an uncentred Kabsch step.
 * verts1 = target (read only), verts2 = source (moved in place), R (9, row-major) and t (3) in/out.
 * Returns 1.0f like the reference. */
float ICP(Point3f *verts1, Point3f *verts2, int nVerts1, int nVerts2, float *R, float *t, int maxIter);

/* ICP's flow on host arrays with the point-to-plane residual (an extension the reference has no counterpart of; the step is
 * lsnIcpRunPlane's, part 2): normals1 = the target's normals, nVerts1 x 3 floats at the target's own index, read only and used as given.
 * The same context, lock, stream and $LSN_NN as ICP; the result equals lsnIcpRunPlane's on the same data bit for bit.  Returns 0 -- also
 * for maxIter <= 0, which does nothing --, or -1 with lsnGetLastError set: a null argument, an empty cloud, no device, a failed copy.  On -1
 * verts2, R and t are untouched. */
int lsnIcpPointToPlane(Point3f *verts1, Point3f *normals1, Point3f *verts2, int nVerts1, int nVerts2, float *R, float *t, int maxIter);

/* ---------------------------------------------------------------------------------------------------------
 * Part 2 -- device-resident API (extension; every pointer named d_* is HIP device memory)
 * ------------------------------------------------------------------------------------------------------- */

/* Copies the calling thread's last error message (empty string = none) into buf; returns its length. */
int lsnGetLastError(char *buf, int len);

/* Number of visible HIP devices (0 when there is none or the runtime cannot initialise). */
int lsnDeviceCount(void);

/* Device memory and streams for hosts that speak nothing but this C-ABI (a C# or plain C host of the device-resident API has
 * no HIP of its own): thin wrappers over hipMalloc / hipFree / hipMemcpyAsync / hipStreamCreate / hipStreamSynchronize.
 * Copies are asynchronous on `stream` (0 = the null stream); host buffers must stay valid until the stream has been
 * synchronised.  All return 0 / a non-null pointer on success. */
void *lsnDeviceMalloc(int device, long long bytes);
int lsnDeviceFree(int device, void *d_ptr);
int lsnDeviceUpload(int device, void *d_dst, const void *h_src, long long bytes, void *stream);
int lsnDeviceDownload(int device, void *h_dst, const void *d_src, long long bytes, void *stream);
void *lsnStreamCreate(int device);
int lsnStreamDestroy(int device, void *stream);
int lsnStreamSynchronize(int device, void *stream);

/* A fusion plan: fixed rig geometry (n_maps sensors with widths/heights, as in the reference call) replicated
 * over n_ticks ticks that are fused by ONE launch sequence.  Holds the geometry tables and scan scratch in HBM. */
typedef struct LsnFusion LsnFusion;

LsnFusion *lsnFusionCreate(int device, int n_ticks, int n_maps, const int *widths, const int *heights);
void lsnFusionDestroy(LsnFusion *plan);

/* Vertices one tick can produce at most (= sum of w*h): the per-tick stride of d_vertices. */
long long lsnFusionTickCapacity(const LsnFusion *plan);

/* Host arrays exactly like the reference call: intr 7*n_maps, wt 12*n_maps, bounds {minX,minY,minZ,maxX,maxY,maxZ}.
 * stream is a hipStream_t passed as void* (NULL = the null stream). */
int lsnFusionSetParams(LsnFusion *plan, const float *intr_params, const float *wtransform_params,
                       const float *bounds6, void *stream);

/* Host-only (no device needed): the 16 floats the kernels read for one sensor -- {cx, cy, fx, fy, t[3], R[3][3] row-major} -- from the
 * caller's 7 intrinsics and 12 world-transform floats, exactly as lsnFusionSetParams packs them.  Exists so that the unpack order can be
 * held against the reference's IntrinsicCameraParameters(float*) / WorldTranformation(float*) constructors
 * (include/NativeUtils/depthprocessing.h:56-63,96-97) without a GPU. */
int lsnPackSensorParams(const float *intr7, const float *wt12, float *out16);

/* Selects how the raster-order compaction gets its global offsets: 0 = two-pass (count kernel + write kernel) -- except that a
 * ONE-tick plan of up to 2048 tiles takes the single pass of mode 2 by itself (one launch instead of three: 7.5-13.6 us per call
 * against 13.4-15.8; $LSN_ONE_TICK_SINGLE_PASS=0 / 1, read by lsnFusionCreate, forces either), 1 = single launch, runs of tiles
 * counted then re-evaluated, decoupled look-back per run, 2 = single pass, every tile evaluated once, decoupled look-back per
 * tile.  Results are identical; 0 is the fastest on MI355X.  The look-back forms (modes 1, 2 and the
 * one-tick case of mode 0) poll with a bound so that the grid always drains: a launch that gives up raises flag 1 of
 * lsnFusionCheck, writes nothing for the tiles concerned and -- single pass -- stores -1 as the tick's vertex count
 * (offsets[n_maps]) instead of leaving the previous call's value there. */
int lsnFusionSetMode(LsnFusion *plan, int mode);

/* Pipelined calls (mode 0 only): the caller promises that the INPUTS of a call are already resident and stay untouched
 * when the call is issued, whatever is still queued on its stream (true for double-buffered ingest).  The count + scan
 * of call k+1 then run on an internal side stream while the write kernel of call k is still running on the caller's
 * stream; outputs and their ordering on the caller's stream are unchanged. */
int lsnFusionSetPipelined(LsnFusion *plan, int enable);

/* Streamed calls: like lsnFusionRun (mode 0), but while this batch is written the NEXT batch's depth maps
 * (d_next_depth_maps, already resident; NULL = none) are counted by the same kernel -- the count pass is VALU-bound, the
 * write pass HBM-bound, so in one kernel they share every CU.  The following call with d_depth_maps == this call's
 * d_next_depth_maps skips its count pass.  Results are identical to lsnFusionRun. */
int lsnFusionRunStreamed(LsnFusion *plan, const void *d_depth_maps, const void *d_depth_colors, void *d_vertices, int *d_offsets,
                         const void *d_next_depth_maps, void *stream);

/* Fuses n_ticks ticks.  d_depth_maps: n_ticks x (concatenated u16 maps of one tick); d_depth_colors likewise RGB8;
 * d_vertices: n_ticks x lsnFusionTickCapacity() VertexC4ubV3f, tick k's merged cloud starts at k*capacity;
 * d_offsets: n_ticks x (n_maps+1) ints, [k][i] = index of sensor i's first vertex inside tick k's cloud,
 * [k][n_maps] = nVertices of tick k.  Asynchronous on `stream`; returns 0 on success. */
int lsnFusionRun(LsnFusion *plan, const void *d_depth_maps, const void *d_depth_colors, void *d_vertices,
                 int *d_offsets, void *stream);

/* The count pass needs no arithmetic once the calibration is fixed: from the second run with the same parameters on, the
 * plan keeps, per pixel, the interval of depth values that survive the transform + crop (found by bisection with the
 * pipeline's own roundings, exact by construction) and counts with two integer operations per pixel.  This call builds
 * the table now, reports the build time and optionally copies the table out (lsnFusionTickCapacity() words,
 * lo | count << 16; lo == 0: "evaluate arithmetically").  Returns 0, 1 when disabled ($LSN_NO_THRESHOLDS=1), -1 on error. */
int lsnFusionThresholds(LsnFusion *plan, unsigned int *out_host, float *build_ms, void *stream);

/* The complete merge call: vertices as lsnFusionRun plus the reference's always-on triangulation
 * (MeshGenerator::generateTrianglesGradients, src/NativeUtils/meshGenerator.cpp:14-181; index rebasing of formMesh,
 * src/NativeUtils/depthprocessing.cpp:1611-1627).  d_triangles: n_ticks x lsnFusionTickTriangleCapacity() x 3 ints
 * (vertex indices into the tick's merged cloud, reference order); d_tri_offsets: n_ticks x (n_maps+1) ints like d_offsets
 * ([k][n_maps] = nTriangles of tick k). */
long long lsnFusionTickTriangleCapacity(const LsnFusion *plan);
int lsnFusionRunMesh(LsnFusion *plan, const void *d_depth_maps, const void *d_depth_colors, void *d_vertices, int *d_offsets,
                     void *d_triangles, int *d_tri_offsets, void *stream);

/* Colour transfer (generateMeshFromDepthMaps' bcolor_transfer stage) in place on the output of lsnFusionRun / lsnFusionRunMesh:
 * d_depth_maps the depth maps that call read, d_vertices / d_offsets what it wrote; every tick on its own, asynchronous on `stream`.
 * Only the R,G,B bytes of the vertices of corrected sensors change.  Reference: generateVerticesConfidence,
 * updateColorCorrectionCoefficients and applyColorCorrection (src/NativeUtils/depthprocessing.cpp:285-384,1387-1575,
 * colorcorrection.cpp:6-170, CS_RGB), with two defined deviations: a transform sample whose pixel in the base
 * sensor has depth but no vertex is skipped (the reference reads out of bounds), and a double -> int conversion of a NaN or of a
 * value out of range gives INT_MIN (the reference's x64 result), so such a channel becomes 0.  At most 32 sensors.
 * lsnFusionColorDiagnostics (synchronises `stream`): what the last colour transfer computed for tick `tick` -- the confidence maps
 * (lsnFusionTickCapacity() bytes, the sensors' maps back to back), the symmetric coverage table (n_maps^2 ints), the chosen pairs
 * {base, corrected} in order (2 * (n_maps - 1) ints) and their transforms {mean_base[3], mean_corrected[3], scale[3]}
 * (9 * max(n_maps - 1, 1) doubles); any pointer may be NULL.  Returns the number of pairs, -1 on error.  The confidence maps live in
 * the index the plan's three stages share (colour transfer, overlay merge, outlier filter): they are valid until another of the three
 * stages runs on the plan; everything else is the last colour transfer's until the next one. */
int lsnFusionColorTransfer(LsnFusion *plan, const void *d_depth_maps, void *d_vertices, const int *d_offsets, void *stream);
int lsnFusionColorDiagnostics(LsnFusion *plan, int tick, unsigned char *confidence, int *coverage, int *pairs, double *transforms,
                              void *stream);

/* Colour blending across views, in place on the output of lsnFusionRun / lsnFusionRunMesh (behind lsnFusionColorTransfer when both run):
 * d_depth_maps the depth maps that call read, d_vertices / d_offsets what it wrote; every tick on its own, asynchronous on `stream`.
 * Not in the reference: defined.  The colour of a vertex of sensor j becomes, per channel, floor((sum w c +
 * floor(W / 2)) / W) over its own term -- w the confidence level of its pixel (1 .. 20: lsnFusionColorDiagnostics' maps), c its colour --
 * and one term per other sensor i in which it projects (the colour transfer's projection) onto a pixel (x, y) of i's frame with
 * projected depth d1 != 0, depth_i[y, x] = d2 > 0, |d1 - d2| < depth_tol (mm), a vertex of i at that pixel and confidence
 * w = conf_i[y, x] >= min_confidence: that confidence, that vertex's colour.  Every term reads the colours as they were when the call
 * started (the call snapshots them), so the result depends on no order.  A vertex without a partner keeps its bytes; A, X, Y, Z, the
 * offsets and the triangles never change.  depth_tol <= 0 or min_confidence > 20: off, nothing is touched; min_confidence < 1 is read
 * as 1; a plan of one sensor: nothing to do.  At most 32 sensors; mixed frame sizes are allowed.  Returns 0, -1 on error.
 * The blend rebuilds the index the plan's stages share (colour transfer, overlay merge, outlier filter): what their diagnostics keep in
 * that index -- the confidence maps, nVertices -- is valid only until it runs, as it is between any two of them.
 * lsnFusionColorBlendDiagnostics (synchronises `stream`): for tick `tick` of the last blend, per sensor (n_maps entries each) the
 * vertices that had at least one partner, the partner terms they summed and the sum over R, G, B of |new - old|; any pointer may be
 * NULL.  Returns the tick's number of blended vertices, -1 on error.  (The counters are the blend's own: they stay until the next one; a
 * call that is off leaves zeros.)
 * lsnSetColorBlend: the process-wide switch of the blend in generateMeshFromDepthMaps and lsnCorrectAndGenerateMesh (every host flow;
 * with $LSN_HOST_DEVICES the call runs on the first device alone, like a call with colour transfer): behind the colour transfer when
 * bcolor_transfer is set, in front of the overlay merge.  generateVerticesFromDepthMap never blends (one sensor).  Initially
 * $LSN_COLOR_BLEND="depth_tol,min_confidence" (e.g. "20,5"; unset or malformed: off); every call reads the current value.  The previous
 * pair goes to prev_depth_tol / prev_min_confidence (either may be NULL); returns 0. */
int lsnFusionColorBlend(LsnFusion *plan, int depth_tol, int min_confidence, const void *d_depth_maps, void *d_vertices, const int *d_offsets,
                        void *stream);
int lsnFusionColorBlendDiagnostics(LsnFusion *plan, int tick, int *blended_per_sensor, long long *partners_per_sensor,
                                   long long *abs_change_per_sensor, void *stream);
int lsnSetColorBlend(int depth_tol, int min_confidence, int *prev_depth_tol, int *prev_min_confidence);

/* Cross-view overlay merge (generateMeshFromDepthMaps' bgenerate_triangles stage) on the output of lsnFusionRun / lsnFusionRunMesh:
 * d_depth_maps the raw depth maps that call read (for the confidence maps), d_vertices / d_offsets what it wrote (read only); every tick
 * on its own, asynchronous on `stream`.  Rewrites d_triangles / d_tri_offsets in lsnFusionRunMesh's layout and capacity: the triangles
 * of every sensor's reprojected depth map after the base / overlay schedule of mergeVerticesForViews (src/NativeUtils/depthprocessing.cpp
 * :598-1099,1227-1313,1659-1691).  Independent of lsnFusionColorTransfer (neither reads what the other writes).  Every sensor must have
 * the same size; at most 32 sensors.  Returns 0, -1 on error.
 * lsnFusionOverlayDiagnostics (synchronises `stream`): for the last merge of tick `tick`, the reprojected maps as first built and as
 * the merge left them (lsnFusionTickCapacity() u16 each, the sensors' maps back to back) and the point_assigned flag of every vertex
 * (nVertices bytes); any pointer may be NULL.  Returns the number of assigned vertices, -1 on error.  nVertices comes from the index the
 * plan's three stages share: the flags and the return value are valid until another of the three stages runs on the plan (the maps are
 * the last merge's until the next one).
 * lsnSetOverlayMerge: the process-wide switch of generateMeshFromDepthMaps' merge (initially $LSN_OVERLAY_MERGE == "1"); returns the
 * previous value. */
int lsnFusionOverlayMerge(LsnFusion *plan, const void *d_depth_maps, const void *d_vertices, const int *d_offsets, void *d_triangles,
                          int *d_tri_offsets, void *stream);
int lsnFusionOverlayDiagnostics(LsnFusion *plan, int tick, unsigned short *reprojected, unsigned short *merged, unsigned char *assigned,
                                void *stream);
int lsnSetOverlayMerge(int enable);

/* Outlier filter (LiveScanClient's filter(), src/LiveScanClient/filter.cpp:36-81, with the server's bFilter / nFilterNeighbors /
 * fFilterThreshold, LiveScanServer/KinectSettings.cs:30-32) on the output of lsnFusionRun / lsnFusionRunMesh: d_depth_maps the depth maps
 * that call read, d_vertices / d_offsets what it wrote (read only).  Every sensor's block of every tick is filtered on its own: a vertex is
 * removed iff fewer than k vertices of its block (itself included) lie at a squared distance <= max_dist * max_dist in float, evaluated as
 * PointCloud::kdtree_distance does (= the reference's k-th nearest distance > pow(maxDist, 2); a block of fewer than k vertices is kept iff
 * that threshold is >= FLT_MAX).  Writes the maps with depth 0 at the pixels of removed vertices to d_depth_out (may equal d_depth_maps);
 * the caller then runs lsnFusionRun / lsnFusionRunMesh on d_depth_out, and colour transfer / the overlay merge after that if wanted.
 * k <= 0, max_dist <= 0 or NaN: the maps are copied unchanged.  Asynchronous on `stream`; returns 0, -1 on error.
 * lsnFusionOutlierDiagnostics (synchronises `stream`): for tick `tick` of the last filter, the removed vertices per sensor (n_maps ints),
 * the removed flag of every vertex (nVertices bytes) and the vertices the grid pass decided per sensor (n_maps ints; 0 for a block of fewer
 * than k vertices, decided by its size); any pointer may be NULL.  Returns the number of removed vertices, -1 on error.  (All of it is
 * the filter's own: it stays until the next filter, whatever other stage runs on the plan.)
 * lsnSetOutlierFilter: the process-wide switch of the filter in generateMeshFromDepthMaps, generateVerticesFromDepthMap and
 * lsnCorrectAndGenerateMesh (which writes back the unmasked corrected maps): they return the mesh of the masked maps.  Initially
 * $LSN_OUTLIER_FILTER="k,max_dist" (e.g. "10,0.1"; unset or malformed: off); every call reads the current value.  The previous pair goes to
 * prev_k / prev_max_dist (either may be NULL); returns 0. */
int lsnFusionOutlierFilter(LsnFusion *plan, int k, float max_dist, const void *d_depth_maps, const void *d_vertices, const int *d_offsets,
                           void *d_depth_out, void *stream);
int lsnFusionOutlierDiagnostics(LsnFusion *plan, int tick, int *removed_per_sensor, unsigned char *removed_per_vertex, int *exact_per_sensor,
                                void *stream);
int lsnSetOutlierFilter(int k, float max_dist, int *prev_k, float *prev_max_dist);

/* Render view: the merged mesh of every tick (what lsnFusionRun / lsnFusionRunMesh and the stages above left in d_vertices / d_offsets /
 * d_triangles / d_tri_offsets, read only) drawn from n_views <= 16 virtual pinhole cameras into frames with a sensor's layout: d_depth_out
 * [n_ticks][n_views][height][width] u16 millimetres, 0 = nothing drawn; d_colors_out [n_ticks][n_views][height][width][3] RGB8, 0,0,0 where
 * the depth is 0.  They can go into lsnFrameEncode, a PPM, or back into a fusion plan as a synthetic sensor.  A view is described like a
 * sensor: intr_params 7 floats per view (cx, cy, fx, fy; the three distortion terms are ignored), wtransform_params 12 floats per view
 * (p_world = R (p_cam + t)), both on the host; every view is width x height, 1 <= width, height <= 1024.  The reference shows the mesh in
 * an OpenGL window (LiveScanServer's OpenGLWindow) and has no renderer of its own to copy: the stage is defined here
 * from the reference's pointProjection and drawTriangle (src/NativeUtils/depthprocessing.cpp:735-747, :598-706), both pinned bit for bit.
 * A vertex is projected with the view's inverted pose to integer (x, y) and depth d in mm, clamped to [0, 65535]; it is drawable iff it
 * lands inside the image and d != 0 (which drops what is behind the camera, closer than 1 mm or not finite).  d_triangles given: a
 * triangle is drawn iff its three indices are below the tick's nVertices and all three vertices are drawable -- there is NO CLIPPING, a
 * triangle that leaves the image or crosses the camera plane is dropped whole -- over the pixels drawTriangle covers, with its depth
 * value; a plain z-buffer: per pixel the candidate of smallest (depth value, triangle index) wins, candidates of value 0 are skipped; the
 * colour is the winner's vertex colours under drawTriangle's weights, per channel trunc(c1 w1 + c2 w2 + c3 w3 + 0.5f) in float, clamped
 * to [0, 255].  d_triangles == NULL (then d_tri_offsets is not read): points, every drawable vertex a candidate (d, vertex index) at its
 * pixel, with its own colour.  The image does not depend on the order in which the device takes the primitives.  Triangle counts are
 * clipped to lsnFusionTickTriangleCapacity().  Asynchronous on `stream`; returns 0, -1 with a message on a null argument, more than 16
 * views or a bad size -- then no output is touched.
 * Scratch, the plan's own, reserved by the first call, grown when a later call needs more, freed with the plan (a plan that never renders
 * has none): 8 bytes x n_ticks x n_views x width x height of pixel keys and, with triangles, 8 bytes x n_ticks x lsnFusionTickCapacity() of
 * projected vertices + 4 bytes x n_ticks x lsnFusionTickTriangleCapacity() of work list (the views of a call take turns on these two):
 * 8 x 512x424 sensors, one tick, four 512x424 views = 6.9 + 13.9 + 13.9 MB.
 * lsnFusionRenderDiagnostics (synchronises `stream`): for (tick, view) of the plan's last render, the primitives drawn (triangles with
 * three drawable vertices / drawable vertices), the triangles whose bounding box was large enough to be drawn by a whole wave instead of
 * one lane (a measurement aid: the image does not depend on it; 0 for points), and the pixels with depth != 0; any pointer may be NULL.
 * Returns 0, -1 on error or before any render. */
int lsnFusionRenderViews(LsnFusion *plan, int n_views, const float *intr_params, const float *wtransform_params, int width, int height,
                         const void *d_vertices, const int *d_offsets, const void *d_triangles, const int *d_tri_offsets, void *d_depth_out,
                         void *d_colors_out, void *stream);
int lsnFusionRenderDiagnostics(LsnFusion *plan, int tick, int view, int *n_drawn, int *n_large, int *n_pixels, void *stream);

/* Mesh level of detail: vertex clustering of the merged mesh of every tick (what lsnFusionRun / lsnFusionRunMesh and the stages above left
 * in d_vertices / d_offsets / d_triangles / d_tri_offsets, read only) on a uniform grid of edge `cell` metres, after the stages and in
 * front of lsnTransferPack / lsnPlyPack / lsnFusionRenderViews / lsnRefineVertices, which take the outputs as they are.  The reference
 * has no decimation to copy: the stage is defined here (tests/simplify_ref.py restates it).  Per tick, on its own:
 * nVertices = d_offsets[n_maps] clipped to [0, lsnFusionTickCapacity()], nTriangles = d_tri_offsets[n_maps] clipped to [0,
 * lsnFusionTickTriangleCapacity()].  inv = 1.0f / cell, once, in float.  Per axis of a vertex q = floorf(c * inv) (one float multiply,
 * not fused with anything); the axis is in range iff q is finite and -2^20 <= q < 2^20, compared in float.  A vertex with three axes in
 * range has the 63-bit key (qx + 2^20) | (qy + 2^20) << 21 | (qz + 2^20) << 42 and shares its cell with every vertex of that key; any
 * other vertex (a NaN or infinite coordinate, q out of range) is unclustered: a cell of its own, always kept.  The vertex of LOWEST INDEX
 * of a cell represents it and keeps its own 16 bytes: nothing is averaged, the result does not depend on the order in which the device
 * takes the vertices.  d_vertices_out: the representatives in ascending input index (sensor order and raster order survive);
 * d_offsets_out[i] = the kept vertices whose input index is below d_offsets[i], i = 0..n_maps, so d_offsets_out[n_maps] is the new
 * nVertices; d_remap_out (nullable; lsnFusionTickCapacity() ints per tick): the output index of every input vertex's representative.
 * d_triangles given: a triangle whose three indices are in [0, nVertices) is remapped; it is dropped if two of its new indices are equal
 * or an index was out of range; the survivors keep their input order, d_tri_offsets_out[i] = the survivors whose input position is below
 * d_tri_offsets[i].  DUPLICATE TRIANGLES ARE NOT REMOVED: two input triangles that become the same triple are both kept.  d_triangles ==
 * NULL: points only, d_tri_offsets, d_triangles_out and d_tri_offsets_out are neither read nor written.  cell <= 0 or NaN: off -- the
 * counted vertices, the counted triangles (out-of-range and degenerate ones too) and both offset rows are copied as they are, the remap
 * is the identity.  cell = +inf (inv = 0: everything finite in one cell) and a denormal cell (inv = inf: everything unclustered) follow
 * the arithmetic.  Simplifying the output again with the same cell returns the same bytes.  Outputs have lsnFusionRunMesh's layouts and
 * per-tick strides; nothing behind a tick's new counts is written.  Out of place: an output that overlaps an input is refused.
 * Asynchronous on `stream`; returns 0, -1 with a message (null argument, overlap) -- then no output is touched.
 * Scratch, the plan's own, reserved by the first call, grown when a later call needs more, freed with the plan (a plan that never
 * simplifies has none): per tick a hash table of 12 bytes x the power of two at or above 2 x lsnFusionTickCapacity() (cleared by every
 * call, on `stream`; not reserved while cell <= 0), 8 bytes x lsnFusionTickCapacity() of representative / remap and output index, and
 * 4 bytes per 256 vertices and per 256 triangles: 8 x 512x424 sensors, one tick = 50.3 + 13.9 + 0.1 MB.
 * lsnFusionSimplifyDiagnostics (synchronises `stream`): for one tick of the plan's last call the occupied cells (= the new nVertices),
 * the unclustered vertices (0 after cell <= 0) and the dropped triangles; any pointer may be NULL.  Returns 0, -1 on error or before any
 * call. */
int lsnFusionSimplify(LsnFusion *plan, float cell, const void *d_vertices, const int *d_offsets, const void *d_triangles,
                      const int *d_tri_offsets, void *d_vertices_out, int *d_offsets_out, void *d_triangles_out, int *d_tri_offsets_out,
                      int *d_remap_out, void *stream);
int lsnFusionSimplifyDiagnostics(LsnFusion *plan, int tick, int *n_cells, int *n_unclustered, int *n_dropped_triangles, void *stream);

/* Fragment filter: the small connected components of the merged mesh of every tick (what lsnFusionRunMesh or any stage above left in
 * d_vertices / d_offsets / d_triangles / d_tri_offsets, read only) are dropped, in front of the packers, the renderer, the level of detail
 * and the normals.  The reference has no such step: the stage is defined here (tests/fragments_ref.py restates it).
 * Only minima and integer counts: the bytes do not depend on the order in which the device takes the triangles.  Per tick, on its own:
 * Counts: nVertices = d_offsets[n_maps] clipped to [0, lsnFusionTickCapacity()], nTriangles = d_tri_offsets[n_maps] clipped to [0,
 * lsnFusionTickTriangleCapacity()].
 * Graph: a triangle is VALID iff its three indices are in [0, nVertices), compared unsigned.  A valid triangle (i0, i1, i2) joins i0-i1
 * and i1-i2 (i0-i2 follows).  A repeated index is fine: (2, 2, 3) joins 2 and 3, (4, 4, 4) joins nothing.  An invalid triangle joins
 * nothing.  Positions play no part.
 * Label: label[v] = the LOWEST vertex index of v's connected component; a vertex of no valid triangle is a component of one, label[v] = v.
 * Size: the size of a component is the number of vertices that carry its label.
 * Kept: a vertex is kept iff size[label[v]] >= min_vertices.
 * Vertices out: the kept vertices in ascending input index with their own 16 bytes; d_offsets_out[i] = the kept vertices of input index
 * below d_offsets[i], i = 0..n_maps; d_remap_out[j] (nullable) = the output index of a kept vertex, -1 for a removed one; d_labels_out[j]
 * (nullable) = the label, an input index, for every j < nVertices (both lsnFusionTickCapacity() ints per tick).
 * Triangles out: a valid triangle whose component is kept is remapped (its three vertices share one fate) and stays in its input order,
 * degenerate ones too; invalid triangles and triangles of removed components are dropped; d_tri_offsets_out[i] = the survivors of input
 * position below d_tri_offsets[i].
 * Off: min_vertices <= 1 copies the counted vertices, the counted triangles (invalid ones too) and both offset rows as they are; the
 * remap is the identity, the labels are NOT written, all four diagnostics are 0.
 * Refused, with a message and no output touched: a null argument; d_triangles == NULL (the components of a bare point cloud are not
 * defined here); an output that overlaps an input.
 * Idempotent: the output filtered again with the same min_vertices is the same bytes.
 * Outputs have lsnFusionRunMesh's layouts and per-tick strides; nothing behind a tick's new counts is written.  Asynchronous on `stream`;
 * returns 0, -1 with a message.
 * Scratch, the plan's own, reserved by the first call, grown when a later call needs more, freed with the plan (a plan that never
 * filters has none): 12 bytes x lsnFusionTickCapacity() per tick (parent / label, size, output index; 4 of them while min_vertices <= 1),
 * 4 bytes per 256 vertices and per 256 triangles, 16 bytes of counters per tick: 8 x 512x424 sensors, one tick = 20.8 + 0.1 MB.
 * lsnFusionFragmentsDiagnostics (synchronises `stream`): for one tick of the plan's last call the components, the removed components,
 * the removed vertices and the dropped triangles (in minus out); any pointer may be NULL.  Returns 0, -1 on error or before any call. */
int lsnFusionFragments(LsnFusion *plan, int min_vertices, const void *d_vertices, const int *d_offsets, const void *d_triangles,
                       const int *d_tri_offsets, void *d_vertices_out, int *d_offsets_out, void *d_triangles_out, int *d_tri_offsets_out,
                       int *d_remap_out, int *d_labels_out, void *stream);
int lsnFusionFragmentsDiagnostics(LsnFusion *plan, int tick, int *n_components, int *n_removed_components, int *n_removed_vertices,
                                  int *n_dropped_triangles, void *stream);

/* Vertex normals of the merged mesh of every tick (what lsnFusionRunMesh and the stages above -- overlay merge, outlier filter, level of
 * detail -- left in d_vertices / d_offsets / d_triangles / d_tri_offsets, read only): area weighted, bit-exact whatever order the device
 * takes the triangles in.  The reference computes no normals: the stage is defined here (tests/normals_ref.py
 * restates it).  Per tick, on its own: nVertices = d_offsets[n_maps] clipped to [0, lsnFusionTickCapacity()], nTriangles =
 * d_tri_offsets[n_maps] clipped to [0, lsnFusionTickTriangleCapacity()].  Face vector of the triangle (i0, i1, i2) with positions p0, p1,
 * p2, all in float, every operation rounded on its own, nothing fused: u = p2 - p0, v = p1 - p0; fx = u.y * v.z - u.z * v.y, fy = u.z * v.x
 * - u.x * v.z, fz = u.x * v.y - u.y * v.x, that is (p2 - p0) x (p1 - p0): twice the area long, and for the triples lsnFusionRunMesh emits
 * it points towards the sensor that saw the triangle.  A triangle is USED iff its three indices are in [0, nVertices) and fx, fy, fz are
 * all finite with |c| < 4096.0f (compared in float, before any conversion); any other triangle contributes nothing and is counted as
 * skipped.  A degenerate triangle (a repeated index, collinear points) is used and contributes zeros.  Fixed point: q_c = (int64)
 * trunc(c * 2^40); the float multiply is exact for |c| < 4096, the product is below 2^52, so the conversion is exact; a component below
 * 2^-40 becomes 0, so the result does not depend on whether the device flushes float denormals.  Sum: S[i] += q for i = i0, i1, i2 --
 * three signed 64-bit sums per vertex, two's complement with wrap-around (more than 2048 triangles of 4096 m^2 on one vertex).  Integer
 * addition is associative: the sums do not depend on the order of the triangles.  Normal: S[i] == (0, 0, 0) (a vertex of no used
 * triangle, or one whose contributions cancel) gives (+0, +0, +0); otherwise s_c = (float) S_c, one round-to-nearest-even conversion from
 * int64 each, len = sqrtf((s.x * s.x + s.y * s.y) + s.z * s.z), n_c = s_c / len: float throughout, in that order, sqrtf and the divisions
 * correctly rounded.  Nothing overflows (3 x 2^126 < FLT_MAX) and len >= 1.
 * d_normals_out: [n_ticks][lsnFusionTickCapacity()][3] floats, 12 bytes per vertex at the vertex's own index; nothing behind a tick's
 * nVertices is written.  Out of place: an output that overlaps an input is refused.  d_triangles == NULL is refused: the normals of a
 * bare point cloud are not defined here.  Asynchronous on `stream`; returns 0, -1 with a message (null argument, overlap) -- then no
 * output is touched.
 * Scratch, the plan's own, reserved by the first call, grown when a later call needs more, freed with the plan (a plan that never asks
 * for normals has none): the sums as three planes [n_ticks][3][lsnFusionTickCapacity()] of int64 (24 bytes per vertex; 8 x 512x424
 * sensors, one tick = 41.7 MB; the counted vertices are cleared by every call, on `stream`) and 16 bytes of counters per tick.
 * lsnFusionNormalsDiagnostics (synchronises `stream`): for one tick of the plan's last call the used triangles, the skipped triangles and
 * the vertices whose normal is (0, 0, 0); any pointer may be NULL.  Returns 0, -1 on error or before any call. */
int lsnFusionNormals(LsnFusion *plan, const void *d_vertices, const int *d_offsets, const void *d_triangles, const int *d_tri_offsets,
                     void *d_normals_out, void *stream);
int lsnFusionNormalsDiagnostics(LsnFusion *plan, int tick, int *n_used, int *n_skipped, int *n_zero_normals, void *stream);

/* Mesh smoothing: Taubin's lambda|mu filter on the merged mesh of every tick (what lsnFusionRunMesh or any stage above left in d_vertices
 * / d_offsets / d_triangles / d_tri_offsets, read only), bit-exact whatever order the device takes the triangles in.  The reference moves
 * no vertex: the stage is defined here (tests/smooth_ref.py restates it).  Per tick, on its own: nVertices =
 * d_offsets[n_maps] clipped to [0, lsnFusionTickCapacity()], nTriangles = d_tri_offsets[n_maps] clipped to [0,
 * lsnFusionTickTriangleCapacity()].  Vertices are the 16-byte records {colour, x, y, z}.
 * ONE PASS with factor f goes from positions P to positions P', both float, and reads only P (Jacobi, never half-updated positions).
 * Used triangle: a triangle is USED iff it has three indices in [0, nVertices), the indices are pairwise distinct, and all nine
 * coordinates of its corners in P satisfy fabsf(c) < 4096.0f, which NaN and +-inf fail.  Anything else contributes nothing and is counted
 * as skipped.
 * Fixed point: q(c) = (int64) trunc(c * 2^32).  The float multiply by a power of two is exact, the product is below 2^44, and truncation
 * is toward zero.  Anything below 2^-32 m becomes 0, so denormal flushing cannot matter.
 * Sums: a used triangle (i0, i1, i2) adds the positions of a corner's two other corners to that corner.  For corner a with other corners
 * b, c and each component: S[a] += q(P[b]) + q(P[c]), and N[a] += 2.  S is three signed 64-bit sums per vertex, two's complement with
 * wrap-around; N is a 32-bit count.  An edge shared by two triangles therefore weighs twice and a border edge once: that is part of the
 * definition, there is no de-duplication.  Only integer adds enter, so the bytes cannot depend on the order of the atomics.
 * New position: if N[a] == 0, or the vertex is pinned (below), then P'[a] = P[a] bit for bit.  Otherwise, per component: m = (float)
 * (((double) S / (double) N) * 2^-32) -- one round-to-nearest-even conversion of S to double, one correctly rounded double division, an
 * exact scaling, one rounding to float -- then d = m - p and p' = p + f * d in float, every operation rounded on its own, nothing fused.
 * The colour word is carried over.
 * OPEN VERTICES are found once per call from the indices alone; coordinates play no part.  For every triangle that is in range and
 * pairwise distinct, and every corner a with next corner n and previous corner p in the triangle's own order: H[a] += mix(n) - mix(p),
 * as unsigned 64-bit with wrap.  mix is the splitmix64 finaliser of the index: add 0x9E3779B97F4A7C15; x ^= x >> 30, then multiply by
 * 0xBF58476D1CE4E5B9; x ^= x >> 27, then multiply by 0x94D049BB133111EB; x ^= x >> 31.  A vertex with at least one such triangle is OPEN
 * iff H[a] != 0: the multiset of its "next" neighbours differs from that of its "previous" neighbours, some incident edge is not matched
 * by its opposite.  With pin_boundary != 0, open vertices are pinned in every pass.
 * THE FILTER: iterations in [1, 64], lambda in (0, 1], mu in [-1, 0].  Each iteration is one pass with lambda, then one with mu; with
 * mu == 0 the second pass is left out, which gives plain Laplacian smoothing.  Usual values: 10, 0.5, -0.53.
 * Refused, with a message and no output touched: a null argument; NaN or a value out of range; d_triangles == NULL; an output that
 * overlaps an input.
 * d_vertices_out: [n_ticks][lsnFusionTickCapacity()] 16-byte records; only the first nVertices of each tick are written.  Offsets and
 * triangles are unchanged, so the caller hands the input's own rows to whatever follows.  Asynchronous on `stream`; returns 0, -1 with
 * a message.
 * Scratch, the plan's own, reserved by the first call, grown when a later call needs more, freed with the plan (a plan that never
 * smooths has none), per vertex and tick: 24 bytes of sums (three planes [n_ticks][3][lsnFusionTickCapacity()] of int64), 4 of count, 8
 * of H, 1 of flag and 16 of the vertex buffer the passes take turns on with d_vertices_out (none for a call of one pass): 8 x 512x424
 * sensors, one tick = 92.0 MB; and 16 bytes of counters per tick.
 * lsnFusionSmoothDiagnostics (synchronises `stream`): for one tick of the plan's last call the used and the skipped triangles of the
 * last pass, the pinned vertices (0 with pin_boundary == 0) and the vertices with N == 0 in the last pass; any pointer may be NULL.
 * Returns 0, -1 on error or before any call. */
int lsnFusionSmooth(LsnFusion *plan, int iterations, float lambda, float mu, int pin_boundary, const void *d_vertices, const int *d_offsets,
                    const void *d_triangles, const int *d_tri_offsets, void *d_vertices_out, void *stream);
int lsnFusionSmoothDiagnostics(LsnFusion *plan, int tick, int *n_used, int *n_skipped, int *n_pinned, int *n_isolated, void *stream);

/* Flying-pixel filter (LiveScanClient's KinectCapture::filterFlyingPixels, src/LiveScanClient/kinectCapture.cpp:132-174, with the server's
 * bFilterFlyingPixels / nFPNeighbourhoodSize / nFPThreshold, LiveScanServer/KinectSettings.cs:34-37) on all n_ticks x n_maps depth maps of
 * the plan, in front of the radial correction: a pixel with `neighbourhood` <= x < w - neighbourhood and the same for y (value 0 included)
 * becomes 0 iff MORE than N / 2 of the N = (2 neighbourhood + 1)^2 - 1 pixels of its window differ from it by MORE than `threshold`
 * (integer comparison; a neighbour of depth 0 counts like any other value); every decision reads the unmodified map, the border band
 * is copied through, a frame smaller than the window is copied.  The reference's nFPMaxNonFittingNeighbours is overwritten with N / 2
 * before it is read, so it is no parameter.  neighbourhood <= 0: the maps are copied unchanged.  Any neighbourhood >= 1 is right; up to 3
 * the window comes from on-chip memory, above that from cached global loads (slow).  Out of place: a d_depth_out that overlaps
 * d_depth_in (equal pointers included) is refused.  Asynchronous on `stream`; returns 0, -1 on error.
 * lsnFusionFlyingDiagnostics (synchronises `stream`): for tick `tick` of the plan's last filter, the pixels of depth != 0 it set to 0, per
 * sensor (n_maps ints; may be NULL; all 0 after a call with neighbourhood <= 0).  Returns their sum, -1 on error or before any filter call.
 * lsnSetFlyingPixelFilter: the process-wide switch of the filter in the exports that START AT RAW FRAMES, i.e. with the radial correction:
 * depthMapAndColorSetRadialCorrection and lsnCorrectAndGenerateMesh filter every sensor's map before correcting it, on every device of
 * $LSN_HOST_DEVICES, and what they write back is the filtered, corrected maps.  generateMeshFromDepthMaps and
 * generateVerticesFromDepthMap never filter: LiveScanServer calls them on the maps the radial export has just returned
 * (KinectServer.cs:518-525, :354-374), and the filter is not idempotent -- there it would run twice per tick.  It runs for
 * neighbourhood >= 1.  Initially $LSN_FLYING_PIXELS="neighbourhood,threshold" (e.g. "1,20", the client's defaults; unset or malformed:
 * off); every call reads the current value.  The previous pair goes to prev_neighbourhood / prev_threshold (either may be NULL); returns 0. */
int lsnFusionFlyingPixels(LsnFusion *plan, int neighbourhood, int threshold, const void *d_depth_in, void *d_depth_out, void *stream);
int lsnFusionFlyingDiagnostics(LsnFusion *plan, int tick, int *removed_per_sensor, void *stream);
int lsnSetFlyingPixelFilter(int neighbourhood, int threshold, int *prev_neighbourhood, int *prev_threshold);

/* Depth smoothing: an integer bilateral filter on all n_ticks x n_maps raw depth maps of the plan, between the flying-pixel filter and the
 * radial correction.  The reference has no such step; the stage is DEFINED here, tests/depth_smooth_ref.py restates this text in numpy and
 * the kernels are held to the restatement bit for bit.
 * One u16 map D of w x h (millimetres, 0 = no sample).  Inputs: a radius r in {1, 2, 3}; a spatial table ws[(2r+1)^2], row-major over
 * (dy, dx); a range table wr[n_range], indexed by |delta| in millimetres; both tables unsigned short with every entry <= 4095;
 * 1 <= n_range <= 1024, ws[centre] >= 1 and wr[0] >= 1.
 * Per pixel, with c = D[y][x]:  c == 0 gives out = 0 (holes are not filled: that is the closing's job).  Otherwise every window position
 * (dy, dx), |dy|, |dx| <= r, centre included, contributes iff its pixel lies inside the frame, its value v != 0, and a = |v - c| < n_range.
 * A contributing position has the weight wt = ws[dy+r][dx+r] * wr[a] (below 2^24).  W = sum of wt (at least 1: the centre contributes
 * ws[centre] * wr[0]; below 2^30).  S = sum of wt * (v - c), signed, |S| < 2^40: 64 bits.  out = c + floor((2 S + W) / (2 W)), the
 * division being mathematical floor division: an exact half rounds towards +infinity.  The result is a rounded weighted mean of non-zero
 * samples: it lies in [1, 65535], and |out - c| < n_range.
 * Across the map: every pixel, borders included, is treated this way (out-of-frame positions simply do not contribute); every decision
 * reads the unmodified map, so the pass runs out of place; everything is an integer, so the order of the sums cannot matter.  The filter
 * is not idempotent: a tick applies it exactly once.
 * lsnDepthSmoothGaussian (host only, needs no device): Gaussian tables, all arithmetic in double:
 * ws[dy][dx] = rint(4095 exp(-(dx^2 + dy^2) / (2 ss ss))) with ss = (double) sigma_s into spatial_out ((2 radius + 1)^2 entries),
 * wr[k] = rint(4095 exp(-k^2 / (2 sr sr))) into range_out; n_range, the return value, is the number of leading non-zero entries, at most
 * min(range_cap, 1024) -- nothing behind them is written.  Refused with a message (-1): a radius outside 1..3, a sigma that is not finite
 * and positive, a null pointer, range_cap < 1.  (Two exp implementations may differ in the last bit, so an entry may differ by one unit
 * from another library's: that is why the kernels take tables, not sigmas.)
 * lsnFusionSetDepthSmooth: the plan's setting.  radius <= 0: off (the default; the table pointers are ignored).  Otherwise the tables are
 * validated as above -- refused with a message (-1), they leave the plan's previous setting in place -- and kept by the plan: both
 * tables are uploaded into a buffer of the plan's once per new setting (setting the same tables again costs nothing; replacing them waits
 * for the device).
 * lsnFusionDepthSmooth: d_depth_in into d_depth_out ([n_ticks][pixels per tick] u16, as lsnFusionRun's input) on every tick and sensor of
 * the plan; off: a device-to-device copy.  Out of place: a d_depth_out that overlaps d_depth_in (equal pointers included) is refused with
 * nothing written; a null argument is refused.  Asynchronous on `stream`; returns 0, -1 on error.  The plan's list of 128 x 16 tiles
 * (shared with the flying-pixel filter) and two words per tile of every tick are reserved by the first filtering call and freed with
 * the plan.
 * lsnFusionDepthSmoothDiagnostics (synchronises `stream`): for tick `tick` of the plan's last call, per sensor the pixels with out != in
 * (n_maps ints) and the sum of |out - in| (n_maps long longs); either may be NULL; all 0 after a call with the filter off.  Returns the
 * total of changed pixels, -1 on error or before any call.
 * lsnSetDepthSmooth: the process-wide switch of the stage in the exports that START AT RAW FRAMES, depthMapAndColorSetRadialCorrection and
 * lsnCorrectAndGenerateMesh: they smooth every sensor's map between the flying-pixel filter (if that is on) and the correction, on every
 * device of $LSN_HOST_DEVICES, with the Gaussian tables of (radius, sigma_s, sigma_r), and what they write back is the smoothed, corrected
 * maps.  generateMeshFromDepthMaps and generateVerticesFromDepthMap never smooth (they run on maps the radial export has already
 * returned), nor does lsnRefineFromDepthMaps.  radius <= 0: off.  A triple lsnDepthSmoothGaussian refuses is refused here (-1, the
 * setting stays).  Initially $LSN_DEPTH_SMOOTH="radius,sigma_s,sigma_r" (e.g. "2,1.5,12"; unset, malformed or refused: off); every call
 * reads the current value.  The previous triple goes to prev_* (each may be NULL); returns 0. */
int lsnDepthSmoothGaussian(int radius, float sigma_s, float sigma_r, unsigned short *spatial_out, unsigned short *range_out, int range_cap);
int lsnFusionSetDepthSmooth(LsnFusion *plan, int radius, const unsigned short *spatial, const unsigned short *range, int n_range);
int lsnFusionDepthSmooth(LsnFusion *plan, const void *d_depth_in, void *d_depth_out, void *stream);
int lsnFusionDepthSmoothDiagnostics(LsnFusion *plan, int tick, int *changed_per_sensor, long long *abs_change_per_sensor, void *stream);
int lsnSetDepthSmooth(int radius, float sigma_s, float sigma_r, int *prev_radius, float *prev_sigma_s, float *prev_sigma_r);

/* The temporal depth filter: a range-gated recursive mean ACROSS TICKS on the raw depth maps, in front of the flying-pixel filter (order:
 * temporal -> flying pixels -> depth smoothing -> radial correction).  It removes what no single-frame stage can: per-pixel noise that is
 * independent from tick to tick (shimmer) and pixels that drop out for a tick or two (flicker holes).  The reference has no such step; the
 * stage is DEFINED here, tests/temporal_ref.py restates this text in numpy int64 and the kernel is held to the restatement bit for bit, in
 * maps and in state.  Integers only.
 * Inputs: per tick one u16 map D (millimetres, 0 = no sample) per sensor.
 * Parameters: alpha_q in 1..256, the weight of the new sample in 1/256; delta in 1..4095 mm, the gate; persist in 0..255, how many
 * consecutive ticks a missing sample is served from history.
 * State: one u32 word per pixel, F | miss << 24.  F is the filtered depth in 1/256 mm; it lies in 256 .. 65535 * 256 (below 2^24), and
 * F == 0 means no history.  miss counts the consecutive ticks served from history.  The word 0 is "no history": a zeroed buffer is a reset.
 * Per pixel and tick, with sample c:
 *   1. Blend: c != 0, F != 0 and |256 c - F| <= 256 delta.  F' = F + floor((alpha_q (256 c - F) + 128) / 256), mathematical floor (the
 *      product stays below 2^29: 32 bits are enough); miss' = 0; out = floor((F' + 128) / 256).
 *   2. Restart: c != 0 otherwise (no history, or the gate failed because of motion or an edge).  F' = 256 c, miss' = 0, out = c.
 *   3. Fill: c == 0, F != 0 and miss < persist.  F' = F, miss' = miss + 1, out = floor((F + 128) / 256).
 *   4. Expire or empty: c == 0 otherwise.  The state word becomes 0 and out = 0.
 * Consequences: F' of a blend lies between F and 256 c; out lies in [1, 65535] wherever something is served; alpha_q = 256 with
 * persist = 0 is the identity on the maps; the pass is pointwise, so it may run in place; ticks are sequential per pixel, so a call of n
 * ticks equals n calls of one tick, byte for byte, in maps and in state.  Lag is by design: a surface that moves by less than delta per
 * tick keeps being blended and lags behind itself (by up to (256 - alpha_q) / alpha_q steps); one that moves further restarts.
 * Because the stage runs on the raw samples in front of the flying-pixel filter, a pixel that filter removes is never filled back in, and a
 * pixel served from history still passes that filter.
 * lsnFusionSetTemporal: the plan's setting.  alpha_q <= 0: off (the default).  Out-of-range values are refused with a message (-1) and the
 * previous setting stays in force.  Changing the setting keeps the history.
 * lsnFusionTemporal: d_depth_in into d_depth_out ([n_ticks][pixels per tick] u16) on all ticks and sensors of the plan, in tick order; the
 * plan's history advances by n_ticks.  Off: a device-to-device copy (nothing when in place), the history untouched.  d_depth_out ==
 * d_depth_in is allowed; any other overlap is refused with nothing written.  Asynchronous on `stream`; a call on another stream than the
 * previous call's first waits for that one.  The first filtering call reserves the history (4 bytes per pixel of ONE tick, zeroed) and four
 * count words per 128 x 16 tile of every tick; a plan that never filters allocates nothing.
 * lsnFusionTemporalReset: zeroes the history (asynchronous on `stream`).
 * lsnFusionTemporalStateRead / lsnFusionTemporalStateWrite (both synchronise `stream`): the history as [pixels per tick] u32 in the layout
 * of one tick's depth maps, to / from host memory -- a checkpoint of the history (before any filtering call: all 0).  Write refuses (-1,
 * the history stays) a word whose F is outside {0} and 256 .. 65535 * 256, or whose F is 0 and miss is not.
 * lsnFusionTemporalDiagnostics (synchronises `stream`): for tick `tick` of the plan's last call, per sensor (n_maps ints each, any pointer
 * may be NULL) the pixels blended, restarted although they had history, filled from history, and expired; all 0 after a call with the
 * stage off.  Returns 0, -1 on error or before any call.
 * lsnSetTemporalFilter: the process-wide switch of the stage in the exports that START AT RAW FRAMES, depthMapAndColorSetRadialCorrection
 * and lsnCorrectAndGenerateMesh: each such call is ONE tick, and what it writes back is the temporally filtered (then flying-filtered,
 * smoothed) and corrected maps.  The history lives with the calling lane (on every device of $LSN_HOST_DEVICES: of that device's block),
 * one word per pixel at the sensor's offset in the caller's arrays, whatever the grouping or host path; it is keyed by the rig (sensor
 * count, widths, heights): a call with another rig, or lsnResetTemporalFilter, starts from no history.  generateMeshFromDepthMaps,
 * generateVerticesFromDepthMap and lsnRefineFromDepthMaps never run the stage.  alpha_q <= 0: off.  Out-of-range values are refused (-1,
 * the setting stays).  Initially $LSN_TEMPORAL_FILTER="alpha_q,delta,persist" (e.g. "64,20,2"; unset, malformed or refused: off, a
 * refused value with a message on stderr); every call reads the current value.  The previous triple goes to prev_* (each may be NULL);
 * returns 0. */
int lsnFusionSetTemporal(LsnFusion *plan, int alpha_q, int delta, int persist);
int lsnFusionTemporal(LsnFusion *plan, const void *d_depth_in, void *d_depth_out, void *stream);
int lsnFusionTemporalReset(LsnFusion *plan, void *stream);
int lsnFusionTemporalStateRead(LsnFusion *plan, unsigned int *h_state, void *stream);
int lsnFusionTemporalStateWrite(LsnFusion *plan, const unsigned int *h_state, void *stream);
int lsnFusionTemporalDiagnostics(LsnFusion *plan, int tick, int *blended, int *restarted, int *filled, int *expired, void *stream);
int lsnSetTemporalFilter(int alpha_q, int delta, int persist, int *prev_alpha_q, int *prev_delta, int *prev_persist);
int lsnResetTemporalFilter(void);

/* Background subtraction: a learned per-pixel depth model of the EMPTY scene, what matches it dropped, the small blobs that survive dropped
 * too -- "keep the subject, drop the room", which the axis-aligned crop box cannot do (the floor under the feet, a wall behind a shoulder,
 * furniture inside the box).  It sits behind the temporal depth filter and in front of the flying-pixel filter (order: temporal ->
 * background -> flying pixels -> depth smoothing -> radial correction): it sees the temporal stage's output (the raw maps when that stage is
 * off) both when it learns and when it classifies, and the flying-pixel filter then cleans the silhouette the subtraction creates.  The
 * reference has no such step; the stage is DEFINED here, tests/background_ref.py restates this text in numpy and the kernels are held to the
 * restatement bit for bit, in maps, model and diagnostics.  Integers only.
 * Inputs: per tick one u16 map (millimetres, 0 = no sample) per sensor.
 * Parameters: margin in 1..4095 mm (<= 0: off); rel_q in 0..255, the part of the threshold that grows with depth, in 1/1024; min_pixels in
 * 0..2^24 (<= 1: no blob pass).
 * Model: one u16 per pixel of ONE tick, lo: the smallest non-zero sample seen while learning; 0 means none seen.  The model is itself a
 * depth map: every u16 map is a valid model, and a zeroed buffer is "nothing learned".
 *   1. Learn, per pixel and tick with sample c.  c != 0: lo' = (lo == 0) ? c : min(lo, c).  c == 0: unchanged.  Learning is therefore
 *      order-independent, and a call of n ticks equals n calls of one tick.  A learning pass writes no maps.
 *   2. Classify, per pixel and tick.  thr = margin + floor(lo * rel_q / 1024) (the product stays below 2^24).  c != 0 and lo == 0: UNKNOWN,
 *      kept.  c != 0, lo != 0 and c + thr < lo (strict <, int arithmetic): FOREGROUND, kept.  Otherwise out = 0.  m is the kept mask.  The
 *      model is never changed by classification.
 *   3. Blobs, only when min_pixels >= 2.  Two kept pixels of the same frame and tick are joined when they are 4-neighbours (connectivity
 *      is the mask alone: no depth gate -- out of scope).  label[p] is the lowest raster index y * w + x in p's component, size its pixel
 *      count.  A kept pixel survives iff size[label] >= min_pixels, else out = 0.  Only minima and integer counts enter, so the bytes do not
 *      depend on the order of the device's atomics.
 *   4. Diagnostics, per (tick, frame), six ints: foreground kept by classification, unknown kept by classification, samples removed as
 *      background, components, components removed, pixels removed by the blob pass (the last three are 0 when no blob pass ran).
 * The stage is pointwise plus per-frame, so out == in is allowed; any other overlap is refused with nothing written.
 * lsnFusionSetBackground: the plan's setting.  margin <= 0: off (the default).  Out-of-range values are refused with a message (-1) and the
 * previous setting stays in force.  Changing the setting keeps the model.
 * lsnFusionBackgroundLearn: folds all ticks of d_depth ([n_ticks][pixels per tick] u16) into the plan's model, which is reserved (2 bytes per
 * pixel of ONE tick, zeroed) on first use; it needs no setting.  Asynchronous on `stream`.
 * lsnFusionBackground: d_depth_in into d_depth_out on all ticks and sensors of the plan against the plan's model (never learned: every
 * sample is unknown and kept).  Off: a device-to-device copy (nothing when in place), the model untouched.  Asynchronous on `stream`; a call
 * on another stream than the previous call's that touched the model first waits for that one.  The first call with the stage on reserves six
 * count words per 128 x 16 tile of every tick; the first with min_pixels >= 2 reserves the blob pass's scratch, 8 bytes per pixel of
 * min(n_ticks, 16) ticks (the pass labels 16 ticks at a time).  A plan that never runs the stage allocates nothing.
 * lsnFusionBackgroundReset: zeroes the model (asynchronous on `stream`).
 * lsnFusionBackgroundModelRead / lsnFusionBackgroundModelWrite (both synchronise `stream`): the model as [pixels per tick] u16 in the layout
 * of one tick's depth maps, to / from host memory (before any learning: all 0).  Write accepts any map.
 * lsnFusionBackgroundDiagnostics (synchronises `stream`): for tick `tick` of the plan's last lsnFusionBackground, per sensor (n_maps ints
 * each, any pointer may be NULL) the six counts of 4.; all 0 after a call with the stage off.  Returns 0, -1 on error or before any call.
 * lsnSetBackground: the process-wide switch of the stage in the exports that START AT RAW FRAMES, depthMapAndColorSetRadialCorrection and
 * lsnCorrectAndGenerateMesh: each such call is ONE tick.  The model lives with the calling lane (on every device of $LSN_HOST_DEVICES: of
 * that device's block), one value per pixel at the sensor's offset in the caller's arrays, whatever the grouping or host path; it is keyed
 * by the rig (sensor count, widths, heights) and a generation.  lsnLearnBackground(n_calls) advances the generation.  When the rig or the
 * generation changes, the lane zeroes its model and its next n_calls calls (the last value requested; 0 if none was) are LEARNING calls: a
 * learning call folds its maps into the model, passes them through unchanged and runs no blob pass; the calls behind them subtract.
 * generateMeshFromDepthMaps, generateVerticesFromDepthMap and lsnRefineFromDepthMaps never run the stage.  margin <= 0: off.  Out-of-range
 * values are refused (-1, the setting stays).  Initially $LSN_BACKGROUND="margin,rel_q,min_pixels[,learn_calls]" (e.g. "40,8,64,30"; unset,
 * malformed or refused: off, a refused value with a message on stderr); every call reads the current value.  The previous triple goes to
 * prev_* (each may be NULL); returns 0.  lsnLearnBackground returns 0, -1 for a negative n_calls. */
int lsnFusionSetBackground(LsnFusion *plan, int margin, int rel_q, int min_pixels);
int lsnFusionBackgroundLearn(LsnFusion *plan, const void *d_depth, void *stream);
int lsnFusionBackground(LsnFusion *plan, const void *d_depth_in, void *d_depth_out, void *stream);
int lsnFusionBackgroundReset(LsnFusion *plan, void *stream);
int lsnFusionBackgroundModelRead(LsnFusion *plan, unsigned short *h_model, void *stream);
int lsnFusionBackgroundModelWrite(LsnFusion *plan, const unsigned short *h_model, void *stream);
int lsnFusionBackgroundDiagnostics(LsnFusion *plan, int tick, int *foreground, int *unknown, int *background, int *components,
                                   int *components_removed, int *pixels_removed, void *stream);
int lsnSetBackground(int margin, int rel_q, int min_pixels, int *prev_margin, int *prev_rel_q, int *prev_min_pixels);
int lsnLearnBackground(int n_calls);

/* Radial correction of n_ticks x n_maps frames in place in HBM (same layouts as lsnFusionRun's inputs);
 * intr_params: host, 7 floats per sensor {cx,cy,fx,fy,r2,r4,r6}. */
int lsnFusionRadialCorrect(LsnFusion *plan, const float *intr_params, void *d_depth_maps, void *d_depth_colors, void *stream);
/* The same out of place: the corrected frames go to d_depth_out / d_colors_out, the inputs stay as they are (the reference works
 * on copies and writes them back at the end, depthprocessing.cpp:193-194,259-260).  This is the cheaper form: the warped, not yet
 * closed maps then never leave the GPU's local memory (in place they pass through a scratch copy in HBM, because a pixel's source
 * may lie in rows another workgroup is already overwriting).  Both pointers equal to the inputs = lsnFusionRadialCorrect. */
int lsnFusionRadialCorrectTo(LsnFusion *plan, const float *intr_params, const void *d_depth_maps, const void *d_depth_colors,
                             void *d_depth_out, void *d_colors_out, void *stream);
/* Test hook: the number of work counters of the hole-closing chain that are NOT zero once `stream` has drained (0 after every complete
 * chain: the chain clears them itself, which is why the next call on the same stream needs no memset); -1 on error. */
int lsnFusionRadialCountersLeft(LsnFusion *plan, void *stream);

/* Name and average duration (ms, HIP events on the plan's stream) of the dominant kernel over the launches
 * since the last call with reset != 0; used by bench.py's roofline block.  Enable with lsnFusionProfile(plan, 1); lsnFusionProfile(plan, n)
 * with n > 1 times every n-th launch only (the two event records around a launch cost a few microseconds of stream time each). */
int lsnFusionProfile(LsnFusion *plan, int enable);
int lsnFusionKernelStats(LsnFusion *plan, double *avg_ms, long long *launches, char *name, int name_len, int reset);

/* Merged-cloud assembly after an all-gather of per-GPU shards (one block of sensors per GPU, rank order = sensor order):
 * d_shards [n_shards][n_ticks][shard_cap] vertices and d_shard_offsets [n_shards][n_ticks][maps_per_shard+1] are the
 * gathered outputs of lsnFusionRun; writes d_merged [n_ticks][merged_cap] (each tick contiguous, formMesh order,
 * src/NativeUtils/depthprocessing.cpp:1594-1608) and d_merged_offsets [n_ticks][n_shards*maps_per_shard+1]. */
int lsnMergeShards(int device, int n_shards, int n_ticks, int maps_per_shard, const void *d_shards, long long shard_cap,
                   const int *d_shard_offsets, void *d_merged, long long merged_cap, int *d_merged_offsets, void *stream);

/* Survivor exchange for the multi-GPU path: a vertex is 16 bytes, what it is computed from is 5 (u16 depth + RGB8) plus
 * one bit per pixel.  lsnFusionPackSurvivors fuses like lsnFusionRun but writes, per tick, the survivors' depth and colour
 * as compact streams in vertex order (d_depth_c [n_ticks][capacity] u16, d_rgb_c [n_ticks][capacity][3]), the survivor
 * mask (d_mask [n_ticks][capacity/8], bit p&7 of byte p>>3 = pixel p of the tick), the tiles' exclusive prefixes
 * (d_tile_prefix [n_ticks][lsnFusionTilesPerTick()]) and the usual offsets table.  After an all-gather of these arrays
 * lsnFusionReconstruct, called on a plan that covers the WHOLE rig (all sensors' parameters set, same n_ticks), rebuilds
 * every shard's vertices with the same arithmetic -- bit-identical to fusing all sensors in one plan -- directly into the
 * merged cloud d_merged [n_ticks][lsnFusionTickCapacity(all)] and fills d_merged_offsets [n_ticks][n_maps+1].  The
 * gathered arrays are [n_shards][n_ticks][...] with the per-tick vertex capacity of the streams cut to `slab`.
 * Needs identically sized sensors whose width is a multiple of 8; otherwise exchange vertices (lsnMergeShards). */
int lsnFusionTilesPerTick(const LsnFusion *plan);
int lsnFusionPackSurvivors(LsnFusion *plan, const void *d_depth_maps, const void *d_depth_colors, void *d_mask, void *d_depth_c,
                           void *d_rgb_c, int *d_tile_prefix, int *d_offsets, void *stream);
int lsnFusionReconstruct(LsnFusion *all, int n_shards, int maps_per_shard, const void *d_masks, const void *d_depth_c,
                         const void *d_rgb_c, long long slab, const int *d_tile_prefix, const int *d_shard_offsets, void *d_merged,
                         int *d_merged_offsets, void *stream);

/* The same two ends with the streams laid out the way lsnShardStep sends them: all ticks of a shard back to back, ONE
 * contiguous run per shard (d_depth_c / d_rgb_c as above but tick k's survivors start at d_tick_base[k], which the call
 * fills, [n_ticks] ints), so that a collective can send the run as it is.  The gathered streams are [n_shards][run_len]
 * (run_len >= the largest shard total); d_tick_base_scratch: [n_shards][n_ticks] ints. */
int lsnFusionPackSurvivorsRun(LsnFusion *plan, const void *d_depth_maps, const void *d_depth_colors, void *d_mask, void *d_depth_c,
                              void *d_rgb_c, int *d_tile_prefix, int *d_offsets, int *d_tick_base, void *stream);
int lsnFusionReconstructRun(LsnFusion *all, int n_shards, int maps_per_shard, const void *d_masks, const void *d_depth_c,
                            const void *d_rgb_c, long long run_len, const int *d_tile_prefix, const int *d_shard_offsets, void *d_merged,
                            int *d_merged_offsets, int *d_tick_base_scratch, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Part 2b -- the multi-GPU step (one process per GPU): this rank's block of sensors in, the merged cloud of ALL sensors out.
 * Replaces the per-sensor thread fan-out and the concatenation of formMesh (src/NativeUtils/depthprocessing.cpp:708-733,
 * :1594-1608) across GPUs: rank r owns sensors [r * n_maps / world, (r + 1) * n_maps / world) of every tick (rank order =
 * sensor order); one exchange step over RCCL / xGMI (all-gathers of the survivors' inputs: 5 bytes per vertex + 1 bit per
 * pixel instead of 16 bytes per vertex) and every rank rebuilds the whole merged cloud, bit-identical to a single-GPU
 * lsnFusionRun over all sensors.  That exchange needs identically sized sensors whose width is a multiple of 8; any other rig
 * whose rank blocks hold the same number of pixels (or any rig with $LSN_SHARD_VERTICES=1) exchanges the 16-byte vertices
 * instead (lsnFusionRun on the block, one all-gather per tick cut to the step's largest shard, lsnMergeShards' packing pass):
 * the same merged cloud for about three times the bytes on the links.
 *
 * Rendezvous, in two steps so that no rank is left waiting inside a communicator that will never form: (1) every rank calls
 * lsnShardPrepare -- everything that can fail on one rank alone: argument checks, loading RCCL, device buffers -- and rank 0
 * calls lsnShardUniqueId; (2) the ranks agree, over whatever channel the host has (a file, a socket, torch.distributed), that ALL
 * of them are ready, and rank 0's 128 bytes go to everybody; (3) only then every rank calls lsnShardConnect with the same id
 * (collective: ncclCommInitRank blocks until all ranks have arrived).  lsnShardCreate = Prepare + Connect for hosts that have no
 * such channel.  widths / heights / intr / wt describe ALL n_maps sensors on every rank.
 * RCCL is loaded on first use: an instance already mapped in the process (PyTorch-ROCm's bundled one) is preferred, so a process
 * never holds two; lsnShardRcclPath reports the file.
 * lsnShardStep is collective and asynchronous on `stream` except for one event wait on a small pinned read-back (the element
 * count of a collective is a host-side argument; $LSN_SHARD_PADDED=1 trades it for full-capacity transfers).  All collectives
 * run on the caller's stream in one ncclGroup; $LSN_SHARD_CHUNKS=n (opt-in, not yet verified on a multi-GPU node) sends the
 * streams in n groups of ticks on a second stream beside the reconstruction.  After a failed step the handle refuses further
 * steps (the ranks' communicators are no longer in step): destroy it.
 * *d_merged: n_ticks x lsnShardMergedCapacity() VertexC4ubV3f, *d_merged_offsets: n_ticks x (n_maps + 1) ints, both owned
 * by the handle and valid until its next step. */
typedef struct LsnShard LsnShard;
int lsnShardUniqueId(unsigned char *id128);
LsnShard *lsnShardPrepare(int device, int rank, int world, int n_ticks, int n_maps, const int *widths, const int *heights);
int lsnShardConnect(LsnShard *shard, const unsigned char *id128);
LsnShard *lsnShardCreate(int device, int rank, int world, const unsigned char *id128, int n_ticks, int n_maps, const int *widths,
                         const int *heights);
int lsnShardRcclPath(char *buf, int len);
void lsnShardDestroy(LsnShard *shard);
long long lsnShardMergedCapacity(const LsnShard *shard);
int lsnShardSetParams(LsnShard *shard, const float *intr_all, const float *wt_all, const float *bounds6, void *stream);
int lsnShardStep(LsnShard *shard, const void *d_depth_local, const void *d_colors_local, void **d_merged, int **d_merged_offsets,
                 void *stream);
/* The handle's two plans, for lsnFusionProfile / lsnFusionKernelStats / lsnFusionCheck only (owned by the handle):
 * whole = 0: this rank's block of sensors (count / pack kernels), whole != 0: the whole rig (recon_kernel). */
LsnFusion *lsnShardPlan(LsnShard *shard, int whole);
/* bytes this rank contributed to the collectives of the last step (what every other rank received from it) */
long long lsnShardLastBytesSent(const LsnShard *shard);
/* the rank count the connected communicator itself reports (ncclCommCount; its ncclCommUserRank must equal the handle's rank);
 * -1 when the handle is not connected or the RCCL in use lacks the call */
int lsnShardRanksSeen(LsnShard *shard);

/* The plan's sticky device-side error flag since the last check (synchronises `stream`, clears the flag):
 *   0 = fine; 1 = a look-back launch (mode 1, mode 2, a one-tick plan of mode 0: lsnFusionSetMode) gave up on a bounded spin --
 *   the call's outputs are invalid (single pass: offsets[n_maps] = -1); 2 = a write pass found a tile whose survivors
 *   differ from what the count pass had counted (the inputs changed between the two passes: a buffer counted ahead by
 *   lsnFusionRunStreamed was refilled, or the inputs of a call in flight were overwritten) -- the affected tiles wrote
 *   nothing, the outputs of that call are invalid.  lsnFusionLookbackFailed is the same call under its round-1 name. */
int lsnFusionCheck(LsnFusion *plan, void *stream);
int lsnFusionLookbackFailed(LsnFusion *plan, void *stream);

/* An ICP workspace for clouds of at most max_n1 target / max_n2 source points. */
typedef struct LsnIcp LsnIcp;

LsnIcp *lsnIcpCreate(int device, int max_n1, int max_n2);
void lsnIcpDestroy(LsnIcp *icp);

/* nn_mode: 0 = brute force (one query per lane, the targets streamed through scalar loads; the ablation leg),
 *          1 = voxel grid (exact at any distance: near path per query + box hierarchy per group of 64 queries; when a work
 *              list overflows, the complete hierarchy walk per group).  Both give the same bits.
 * d_verts1: n1*3 floats (target), d_verts2: n2*3 floats (source, moved in place), d_R 9 floats, d_t 3 floats
 * (in/out, device).  Asynchronous on `stream`; no host synchronisation inside the iteration loop. */
int lsnIcpRun(LsnIcp *icp, const float *d_verts1, int n1, float *d_verts2, int n2, float *d_R, float *d_t,
              int maxIter, int nn_mode, void *stream);

/* lsnIcpRun with the point-to-plane residual: DEFINED by this project, not copied -- the reference has point-to-point ICP only; the
 * definition is tests/icp_plane_ref.py.  d_normals1: n1*3 floats, the target's normals at the target's own index, used
 * as given (never renormalised).  Per iteration the exact NN, the one-to-one matching, the statistics and the 2.5 sigma rejection are
 * lsnIcpRun's, bit for bit; a kept match takes part when its target normal is finite and (nx nx + ny ny) + nz nz > 0 in f32 (lsnFusionNormals
 * writes (0, 0, 0) for a vertex of no used triangle: those matches drop out).  The usable matches' residuals r = (b - a) . n with
 * J = [b x n, n] are summed in double into the 6x6 normal equations, solved by pseudo-inverse over the eigen-decomposition -- a mode whose
 * eigenvalue is <= 2^-20 of the largest is unconstrained and gets zero step (a single wall leaves three) --, and the step becomes a motion
 * (T, Rn) in f32 that moves the cloud and updates d_R / d_t exactly as lsnIcpRun's does.  No usable match: no motion.  Everything else as
 * lsnIcpRun: both nn_modes, asynchronous on `stream`, $LSN_ICP_NEAR; lsnIcpTrace's record carries the usable count where the kept count
 * goes.  A run's bits repeat.  Returns 0, -1 on error. */
int lsnIcpRunPlane(LsnIcp *icp, const float *d_verts1, const float *d_normals1, int n1, float *d_verts2, int n2, float *d_R,
                   float *d_t, int maxIter, int nn_mode, void *stream);

/* The NN step alone (parity tests, ablation): d_idx n2 ints, d_dist2 n2 floats. */
int lsnIcpNearest(LsnIcp *icp, const float *d_verts1, int n1, const float *d_verts2, int n2, int *d_idx,
                  float *d_dist2, int nn_mode, void *stream);

/* The whole pose-refinement pass of LiveScanServer (refineWorker_DoWork, LiveScanServer/MainWindowForm.cs:330-410) in one
 * call: Gauss-Seidel over the sensors x n_refine_iters, each step ICP(all other sensors' current clouds, this sensor's
 * cloud, Rs[i], Ts[i], n_icp_iters), with every cloud resident in HBM for the whole pass.  clouds[i] = counts[i] x 3 floats
 * on the HOST, moved in place; world_R (n x 9) / world_t (n x 3), nullable, are updated like worldTransforms[i]
 * (:382-410, the C# loops as written); Rs_out (n x 9) / Ts_out (n x 3), nullable, receive the accumulated ICP poses.
 * The pass's device state (ICP workspace, cloud buffers, stream) is kept for the next call on the same device, one state per device
 * (grown when a rig needs more; lsnRefineRelease frees it); a pass that runs while another is in flight on the device allocates its own
 * and frees it again.
 * What stays on the device between passes, per device: the clouds (12 bytes per point), "all other sensors" (12 bytes per point less the
 * smallest cloud), the seeds (4 bytes per point), the poses, and an ICP workspace for (all points but the smallest cloud, the largest
 * cloud) -- 134.7 MB for 8 x 512x424 scene frames (858 708 points) and 86.0 MB for 3 x 96x80 (11 074 points), as lsnRefineRelease
 * reported them: the workspace's grids' cell tables do not depend on the rig.
 * There is no switch on this path: $LSN_REFINE_SEEDS, the A/B switch of the seeding between passes that the round 6 records mention, was
 * retired with the other settled switches -- the seeds are always on; $LSN_ICP_NEAR / $LSN_ICP_NEAR_PTS (below) still apply. */
int lsnRefine(int device, int n_sensors, float *const *clouds, const int *counts, int n_refine_iters, int n_icp_iters,
              float *world_R, float *world_t, float *Rs_out, float *Ts_out);

/* The same pass for a cloud that is ALREADY resident: d_vertices / d_offsets are ONE tick's merged cloud (VertexC4ubV3f, 16-byte aligned) and
 * its row of n_sensors + 1 offsets as lsnFusionRun wrote them -- for tick k of a plan pass d_vertices + k * capacity * 16 bytes and
 * d_offsets + k * (n_sensors + 1).  Both are read only.  The call is ordered behind the work queued on `stream`, reads the offsets row
 * back (one small copy that SYNCHRONISES `stream`) and is complete on return: its results are host arrays.  world_R / world_t in/out as in
 * lsnRefine, camera_R / camera_t as in lsnRefineFromDepthMaps, all nullable; d_clouds_out (device, offsets[n_sensors] x 3 floats, nullable)
 * receives the refined points, sensor blocks in sensor order.  Nothing to refine: as lsnRefineFromDepthMaps.  Returns 0, -1 on error. */
int lsnRefineVertices(int device, int n_sensors, const void *d_vertices, const int *d_offsets, int n_refine_iters, int n_icp_iters,
                      float *world_R, float *world_t, float *camera_R, float *camera_t, float *Rs_out, float *Ts_out, float *d_clouds_out,
                      void *stream);

/* lsnRefineVertices with the point-to-plane residual (lsnIcpRunPlane's step in every ICP call of the Gauss-Seidel loop).  d_normals: ONE
 * tick of lsnFusionNormals' output -- 12 bytes per vertex at the vertex's own index, so for tick k of a plan d_normals_out + k * capacity * 12
 * bytes --, read only and final like d_vertices.  "All other sensors" is concatenated for the normals as for the points (two more
 * device-to-device copies per step); after sensor i's call its current normals are recomputed as n0_i R_i in f32 from the tick's ORIGINAL
 * normals and the sensor's accumulated pose -- never chained from the step before.  The seeds between passes, the kept device state
 * (lsnRefineRelease frees and reports the three normals buffers with the rest: 36 bytes per point more, less 12 per point of the smallest
 * cloud), the "nothing to refine" rules and every other argument: as lsnRefineVertices.  Returns 0, -1 on error. */
int lsnRefineVerticesPlane(int device, int n_sensors, const void *d_vertices, const float *d_normals, const int *d_offsets,
                           int n_refine_iters, int n_icp_iters, float *world_R, float *world_t, float *camera_R, float *camera_t,
                           float *Rs_out, float *Ts_out, float *d_clouds_out, void *stream);

/* Host-only (no device needed): the pose composition at the end of refineWorker_DoWork (MainWindowForm.cs:382-410) in f32, the C# loops
 * as written -- including their in-place update of worldTransforms[i].R while later rows still read it.  Rs (n x 9) / Ts (n x 3) are the
 * accumulated ICP poses; world_R (n x 9) / world_t (n x 3) and camera_R / camera_t are updated in place; either pair may be NULL (without
 * the world pair the camera rotations stay as they are: :407 copies what :403 computed from the world rotation).  The one place the
 * composition lives: lsnRefine, lsnRefineVertices and lsnRefineFromDepthMaps end with it.  Returns 0, -1 on bad arguments. */
int lsnRefineComposePoses(int n, const float *Rs, const float *Ts, float *world_R, float *world_t, float *camera_R, float *camera_t);

/* Frees what the refine passes keep on `device` (every device: device < 0); a pass in flight on that state ends first.  Returns the bytes
 * of device memory released, 0 if nothing was held (no device is touched then), -1 on error.  The next pass allocates afresh.  Like
 * every export that takes a device it makes that device the calling thread's current one (hipSetDevice) and does not switch back: after
 * lsnRefineRelease(-1) the thread is on the last device whose state it freed. */
long long lsnRefineRelease(int device);

/* How many queries of the workspace's last voxel-grid NN step were settled by the near path (the walk over the cells around
 * a query whose bound is small; diagnostic, synchronises `stream`; -1 on error).  $LSN_ICP_NEAR (read by lsnIcpCreate):
 * 0 = the path off, every query goes through the group search; 1 (default) = the unseeded step always probes, a seeded step takes
 * the path when at least half of the previous step's queries lay within one target cell of their neighbour; 2 = always.
 * $LSN_ICP_NEAR_PTS: the candidate cap per query (<= 128).  Speed only: all settings give the same bits. */
int lsnIcpNearResolved(LsnIcp *icp, void *stream);

/* Optional phase timing of lsnIcpRun (measurement aid): with profiling on, every lsnIcpRun records HIP events on its stream;
 * lsnIcpProfile synchronises `stream` and returns the milliseconds of the last run in ms4 = {grid build + source sort,
 * NN steps (incl. the fused apply of the previous iteration), match statistics + Kabsch sums + solve, final apply}. */
int lsnIcpSetProfiling(LsnIcp *icp, int on);
int lsnIcpProfile(LsnIcp *icp, float *ms4, void *stream);

/* Per-iteration diagnostics of the last lsnIcpRun (copied to host; synchronises `stream`):
 * out[iter] = {n_matched, n_kept, mean, stddev, T[3], Rn[9]} as 16 floats (counts stored as floats). */
int lsnIcpTrace(LsnIcp *icp, float *out16_per_iter, int max_iters, void *stream);

/* The reference's tick, device resident, as ONE call: the radial correction (out of place) then the merge call with its
 * triangulation -- CorrectRadialDistortionsForDepthMaps then GenerateMesh on every tick (LiveScanServer/KinectServer.cs:518-525,
 * :354-374) = lsnFusionRadialCorrectTo + lsnFusionRunMesh on a batch of n_ticks ticks.  From 8 ticks up the batch is cut in two
 * halves that run side by side -- the caller's stream and an internal one, joined before the call's work ends on the caller's
 * stream, the second half started behind the first half's band kernel -- so that one half's latency chains (the closing rounds)
 * are filled by the other half's throughput-bound passes: +2 % ticks/s on scene frames with the join per call (+5 % for two
 * free-running streams, which a caller that can consume the halves separately may build from two plans itself);
 * $LSN_TICK_PARTS=1: one plan, one stream.  Same bytes as the two calls on one plan.  Arrays as for those calls: inputs and corrected maps [n_ticks][pixels per tick] u16 / [..][3] u8,
 * d_vertices [n_ticks][lsnTickCapacity()] VertexC4ubV3f, d_triangles [n_ticks][lsnTickTriangleCapacity()][3] int,
 * offset tables [n_ticks][n_maps + 1]. */
typedef struct LsnTick LsnTick;
LsnTick *lsnTickCreate(int device, int n_ticks, int n_maps, const int *widths, const int *heights);
void lsnTickDestroy(LsnTick *tick);
int lsnTickSetParams(LsnTick *tick, const float *intr_params, const float *wtransform_params, const float *bounds6, void *stream);
long long lsnTickCapacity(const LsnTick *tick);
long long lsnTickTriangleCapacity(const LsnTick *tick);
int lsnTickParts(const LsnTick *tick);   /* 1 or 2 */
/* The flying-pixel filter as the tick's first stage: lsnTickRun then runs filter -> radial correction -> vertices -> triangles, on both
 * halves of a two-part tick.  d_depth_in stays untouched; d_depth_corrected receives the filtered AND corrected maps.  The filtered maps
 * pass through scratch of the tick object (2 bytes per pixel per tick), reserved by the first lsnTickRun that filters: a tick object
 * that never filters allocates nothing for it.  neighbourhood <= 0: off (the default).  Returns 0, -1 on error. */
int lsnTickSetFlyingPixels(LsnTick *tick, int neighbourhood, int threshold);
/* Depth smoothing (lsnFusionDepthSmooth, with the Gaussian tables of lsnDepthSmoothGaussian) as a stage of the tick: lsnTickRun then runs
 * flying pixels (if set) -> depth smoothing -> radial correction -> vertices -> triangles on each half, on that half's plan and stream.
 * d_depth_in stays untouched; the smoothed maps pass through scratch of the tick object (2 bytes per pixel per tick) that only a
 * smoothing run reserves.  radius <= 0: off (the default).  Returns 0; -1 with a message where lsnDepthSmoothGaussian refuses the triple,
 * which leaves the previous setting in place. */
int lsnTickSetDepthSmooth(LsnTick *tick, int radius, float sigma_s, float sigma_r);
/* The temporal depth filter (lsnFusionTemporal) as the tick's first stage: lsnTickRun then runs temporal -> flying pixels (if set) -> depth
 * smoothing (if set) -> radial correction -> vertices -> triangles.  The tick object owns ONE history, which continues from run to run,
 * and the pass runs once over the whole batch in tick order on the caller's stream, in front of the fork of a two-part tick, into scratch
 * of the tick object (2 bytes per pixel per tick; history and scratch are reserved by the first run that filters); d_depth_in stays
 * untouched.  alpha_q <= 0: off (the default); out-of-range values are refused (-1) and leave the previous setting; changing the setting
 * keeps the history.  lsnTickTemporalReset zeroes the history (asynchronous on `stream`). */
int lsnTickSetTemporal(LsnTick *tick, int alpha_q, int delta, int persist);
int lsnTickTemporalReset(LsnTick *tick, void *stream);
/* Background subtraction (lsnFusionBackground) as the tick's second stage: lsnTickRun then runs temporal (if set) -> background -> flying
 * pixels (if set) -> depth smoothing (if set) -> radial correction -> vertices -> triangles.  The tick object owns ONE model and a scratch
 * of the batch's size; the pass runs once over the whole batch on the caller's stream in front of the fork of a two-part tick, right behind
 * the temporal pass, whose output it reads; d_depth_in stays untouched.  margin <= 0: off (the default); out-of-range values are refused
 * (-1) and leave the previous setting; changing the setting keeps the model.  lsnTickBackgroundLearn folds every tick of d_depth_in -- as
 * the temporal stage serves it, when that is set, whose history advances -- into the model (reserved on first use) and runs nothing else;
 * lsnTickBackgroundReset zeroes the model.  Both are asynchronous on `stream`. */
int lsnTickSetBackground(LsnTick *tick, int margin, int rel_q, int min_pixels);
int lsnTickBackgroundLearn(LsnTick *tick, const void *d_depth_in, void *stream);
int lsnTickBackgroundReset(LsnTick *tick, void *stream);
int lsnTickRun(LsnTick *tick, const void *d_depth_in, const void *d_colors_in, void *d_depth_corrected, void *d_colors_corrected,
               void *d_vertices, int *d_offsets, void *d_triangles, int *d_tri_offsets, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Part 3 -- the data formats either side of the path.
 *
 * Outbound, built on the device from a cloud / mesh that is already in HBM (e.g. the outputs of lsnFusionRunMesh):
 * the byte stream TransferSocket.SendFrame writes (LiveScanServer/TransferSocket.cs:50-104) for the chunks
 * TransferServer forms (formMeshChunks, LiveScanServer/TransferServer.cs:203-270, when there are triangles, else
 * formVerticesChunks, :177-201), and the file Utils.saveToPly(binary) writes (LiveScanServer/Utils.cs:222-262).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct LsnTransfer LsnTransfer;

/* Workspace for clouds of at most max_vertices vertices / max_triangles triangles.  Like LsnFusion and LsnIcp a handle
 * serialises its own calls (internal mutex); independent handles run concurrently. */
LsnTransfer *lsnTransferCreate(int device, int max_vertices, int max_triangles);
void lsnTransferDestroy(LsnTransfer *t);

/* Upper bound on the length of the SendFrame stream. */
long long lsnTransferFrameBound(int n_vertices, int n_triangles);

/* d_vertices: n_vertices VertexC4ubV3f, d_triangles: n_triangles x 3 ints (may be null when n_triangles == 0), both on
 * the device.  Writes to d_out (device, 4-byte aligned, out_cap bytes):
 *   int nVertices, int nTriangles, int nChunks, int vChunkSizes[nChunks], int tChunkSizes[nChunks],
 *   float xyz[3*nVertices], u8 rgb[3*nVertices], int tri[3*nTriangles]
 * where, as in formMeshChunks, vertices are re-emitted per chunk in order of first use, triangle indices are
 * chunk-local, a chunk closes at the first triangle end with >= 64997 vertices (and the first chunk's triangle count
 * is one short when there are several chunks, TransferServer.cs:244).  Returns the stream length in bytes, -1 on
 * error (an index outside [0, n_vertices) is an error; the reference would throw).  Synchronises `stream`. */
long long lsnTransferPack(LsnTransfer *t, const void *d_vertices, int n_vertices, const int *d_triangles, int n_triangles,
                          void *d_out, long long out_cap, void *stream);

/* How the last lsnTransferPack of this handle formed its chunks (a measurement / test aid; the bytes do not depend on it):
 * 0 = vertices only (formVerticesChunks), 1 = all chunks at once from one prefix sum over the index positions (meshes whose
 * vertices are each used at most 16 times, consecutive uses < 64997 index positions apart: every grid mesh), 2 = chunk after
 * chunk (any mesh; what 1 falls back to).  -1 on a null handle. */
int lsnTransferLastPath(LsnTransfer *t);

/* Binary PLY: header + 15-byte vertex records {f32 x,y,z; u8 r,g,b} + 13-byte face records {u8 3; i32 a,b,c}.
 * lsnPlyBinaryBytes gives the exact file length; lsnPlyPack writes the file image to d_out (device, any alignment),
 * asynchronously on `stream`, and returns its length (-1 on error). */
long long lsnPlyBinaryBytes(int n_vertices, int n_triangles);
long long lsnPlyPack(int device, const void *d_vertices, int n_vertices, const int *d_triangles, int n_triangles, void *d_out,
                     long long out_cap, void *stream);
/* The same file with vertex normals: the header has "property float nx\nproperty float ny\nproperty float nz\n" between z and red (the
 * "\r\n" behind the format line is kept), the vertex records are the 27 bytes {f32 x,y,z; f32 nx,ny,nz; u8 r,g,b}, the face records the
 * same 13.  d_normals: 3 floats per vertex (one tick of lsnFusionNormals' output).  lsnPlyNormalsBytes is the exact length. */
long long lsnPlyNormalsBytes(int n_vertices, int n_triangles);
long long lsnPlyPackNormals(int device, const void *d_vertices, const void *d_normals, int n_vertices, const int *d_triangles, int n_triangles,
                            void *d_out, long long out_cap, void *stream);

/* Host callers (LiveScanServer): the mesh the last generateMeshFromDepthMaps / generateVerticesFromDepthMap /
 * lsnCorrectAndGenerateMesh call OF THE CALLING THREAD returned is still in HBM -- or its frames are, and it is rebuilt there on demand
 * (a call sharded over $LSN_HOST_DEVICES: its frames are gathered from the devices first); these build its SendFrame stream / binary
 * PLY image on the device and copy the bytes to `out` (host).  With out == NULL they return an upper bound on (stream) / the exact (PLY)
 * length.  Return the length, -1 on error.
 * Which mesh: the one of the calling thread's own last mesh call (merge calls and single-sensor calls run on different workers in
 * LiveScanServer, MainWindowForm.cs:238,304: the refine thread's single-sensor call does not change what the update thread gets);
 * a thread that has made no mesh call gets the process's last one.  A LATER call of the same family from another thread still
 * replaces the mesh -- one thread per family, as in LiveScanServer. */
long long lsnLastMeshTransferFrame(unsigned char *out, long long out_cap);
long long lsnLastMeshPly(unsigned char *out, long long out_cap);
/* The same mesh (found and, where needed, rebuilt in HBM the same way) drawn from ONE virtual camera as lsnFusionRenderViews draws it, into
 * host arrays: depth_out width x height u16 (as bytes), colors_out width x height x 3; points_only != 0, or a mesh without triangles: its
 * vertices as points.  The preview of a server that has no OpenGLWindow.  Returns the number of pixels with depth != 0, -1 on error (no
 * mesh, a bad size); complete on return. */
long long lsnLastMeshRenderView(const float *intr7, const float *wt12, int width, int height, int points_only, unsigned char *depth_out,
                                unsigned char *colors_out);
/* lsnLastMeshTransferFrame / lsnLastMeshPly at a level of detail: the same mesh goes through lsnFusionSimplify's stage with `cell` (as one
 * tick of one sensor, in HBM) and is packed from there.  out == NULL: an UPPER BOUND of the length, the one of the unsimplified mesh.
 * cell <= 0 or NaN: byte for byte what the plain calls return.  The resident mesh is not changed: the plain calls still return all of it.
 * A simplified mesh uses some vertices many times, so lsnTransferPack forms its chunks one after the other; only the bytes matter. */
long long lsnLastMeshTransferFrameLod(float cell, unsigned char *out, long long out_cap);
long long lsnLastMeshPlyLod(float cell, unsigned char *out, long long out_cap);
/* lsnLastMeshPly with vertex normals (lsnPlyPackNormals' file): the same mesh goes through the level-of-detail stage with `cell` (<= 0 or
 * NaN: the mesh as it is), then through lsnFusionNormals' stage on what that left, both as one tick of one sensor, in HBM, and is packed
 * from there.  out == NULL: the length for the unsimplified mesh, an upper bound.  A mesh without triangles: -1 with a message.  The
 * resident mesh is not changed. */
long long lsnLastMeshPlyNormals(float cell, unsigned char *out, long long out_cap);
/* The outbound formats through the fragment filter: the same mesh goes through lsnFusionFragments' stage with `min_vertices`, then through
 * the level-of-detail stage if cell > 0, then (with_normals != 0) through lsnFusionNormals' stage, each on what the step before left, as
 * one tick of one sensor, in HBM, and is packed from there.  out == NULL: the length for the unfiltered mesh, an upper bound.
 * min_vertices <= 1 together with cell <= 0 (or NaN): byte for byte what the plain calls return.  A mesh that loses everything leaves as
 * the packers' bytes for (0, 0).  A resident mesh without triangles: -1 with a message when min_vertices > 1 or with_normals != 0.  The
 * resident mesh is not changed. */
long long lsnLastMeshTransferFrameFragments(int min_vertices, float cell, unsigned char *out, long long out_cap);
long long lsnLastMeshPlyFragments(int min_vertices, float cell, int with_normals, unsigned char *out, long long out_cap);
/* The same two with mesh smoothing: open, fragments if min_vertices > 1, level of detail if cell > 0, lsnFusionSmooth's stage with
 * (iterations, lambda, mu, pin_boundary), normals if asked, pack -- each on what the one before left, as one tick of one sensor, in
 * HBM.  iterations <= 0: byte for byte what the Fragments calls return.  out == NULL: the same upper bound as theirs (the stage moves
 * vertices and drops none).  With iterations > 0: -1 with a message for a resident mesh without triangles and for what lsnFusionSmooth
 * refuses.  The resident mesh is not changed. */
long long lsnLastMeshPlySmooth(int min_vertices, float cell, int iterations, float lambda, float mu, int pin_boundary, int with_normals,
                               unsigned char *out, long long out_cap);
long long lsnLastMeshTransferFrameSmooth(int min_vertices, float cell, int iterations, float lambda, float mu, int pin_boundary,
                                         unsigned char *out, long long out_cap);

/* Inbound (host-side parsing, no device work): the client's frame message -- LiveScanClient::SerializeFrame
 * (src/LiveScanClient/liveScanClient.cpp:185-290) as KinectSocket.ReceiveFrame reads it
 * (LiveScanServer/KinectSocket.cs:211-304): 16-byte header {i32 payload bytes, i32 compressed, i32 w, i32 h}, then
 * the payload (one zstd frame when compressed == 1) = u16 depth[w*h], u8 rgb[3*w*h], body block.  zstd is the system
 * libzstd.so.1, loaded on first use (the reference P/Invokes libzstd.dll, LiveScanServer/ZSTDDecompressor.cs:13-31). */
typedef struct LsnFrameInfo { int payload_bytes, compressed, width, height; } LsnFrameInfo;

int lsnZstdAvailable(void);
/* 0 = a frame follows, 1 = "no more frames" (payload_bytes <= 0, KinectSocket.cs:231-235), -1 = malformed. */
int lsnFrameParseHeader(const unsigned char *header16, LsnFrameInfo *info);
/* Copies depth (w*h*2 bytes), rgb (w*h*3) and the body block (at most bodies_cap bytes) out of a payload; any of the
 * three outputs may be null.  Returns the length of the body block (>= 4), -1 on error. */
long long lsnFrameDecode(const unsigned char *payload, int payload_bytes, int compressed, int width, int height,
                         unsigned char *depth_out, unsigned char *rgb_out, unsigned char *bodies_out, int bodies_cap,
                         int *n_bodies);
/* The inverse (SerializeFrame after its colour mapping): header + payload into out; compression_level 0 = raw,
 * > 0 = zstd at that level.  bodies may be null (= no bodies).  Returns the message length, -1 on error. */
long long lsnFrameEncode(const unsigned char *depth, const unsigned char *rgb, int width, int height, const unsigned char *bodies,
                         int bodies_bytes, int compression_level, unsigned char *out, long long out_cap);

/* The client's recording file (src/LiveScanClient/frameFileWriterReader.cpp:59-82 reader, :115-130 writer): records
 * "bufferSize= %d\nframe_timestamp= %d\n" + frame message + "\n", parsed from / appended to a memory image of the
 * file.  lsnRecordingNext returns the position after the record at `pos` (-1 at the end of the file or on a malformed
 * record -- then lsnGetLastError is non-empty); lsnRecordingAppend returns the bytes written (-1 when out is too small). */
long long lsnRecordingNext(const unsigned char *file, long long len, long long pos, long long *frame_off, int *frame_len,
                           int *timestamp_ms);
long long lsnRecordingAppend(unsigned char *out, long long cap, const unsigned char *frame, int len, int timestamp_ms);

#ifdef __cplusplus
}
#endif
#endif
