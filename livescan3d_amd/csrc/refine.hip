// refine.hip -- the refine pass: LiveScanServer's "Refine calibration" over several sensors' clouds, resident on the device.  Compiled as
// part of icp.hip's translation unit (icp.hip includes it at its end); it relies on icp.hip's LsnIcp, lsnIcpCreate / lsnIcpDestroy, icp_run
// and rotate_normals_kernel, on icp_grid.hip's blocks_for, bytes_of and kThreads, and on refine_xyz.hip, which it includes.  Holds the kept
// state, the Gauss-Seidel loop, the pose composition, lsn::refine_cloud / lsn::refine_compose (abi.hip calls them) and the lsnRefine* exports.
#include "refine_xyz.hip"   // xyz_of_vertices: a merged cloud's vertices as the packed points the pass below works on

// refineWorker_DoWork (LiveScanServer/MainWindowForm.cs:330-410) with every cloud resident in HBM for the whole
// Gauss-Seidel loop: the reference re-uploads "all other sensors" and the sensor's own cloud for each of the
// n_sensors x n_refine_iters ICP calls; here each cloud goes up once and comes back once -- or never leaves the device at all
// (lsnRefineVertices, lsnRefineFromDepthMaps).  The pose composition at the end repeats the C# loops literally, including
// their in-place update of worldTransforms[i].R while later rows still read it (:398-406).
struct RefineState {   // what a refine pass keeps on the device between calls
    std::mutex mu;
    int device = -1;
    LsnIcp *ws = nullptr;
    hipStream_t s = nullptr;
    lsn::DevBuf d_all, d_others, d_Rt, d_seeds;
    // the point-to-plane pass only (lsnRefineVerticesPlane): the normals twin of d_all / d_others, and the tick's original normals every
    // sensor's current ones are recomputed from
    lsn::DevBuf d_nrm, d_nrm_others, d_nrm0;
    std::array<lsn::DevBuf *, 7> bufs() { return {&d_all, &d_others, &d_Rt, &d_seeds, &d_nrm, &d_nrm_others, &d_nrm0}; }
    long long bytes() { return (long long)(bytes_of(bufs()) + (ws ? ws->bytes() : 0)); }
    void drop()
    {
        if (device >= 0) (void)hipSetDevice(device);
        if (ws) lsnIcpDestroy(ws);
        ws = nullptr;
        if (s) (void)hipStreamDestroy(s);
        s = nullptr;
        for (lsn::DevBuf *b : bufs()) b->release();
    }
    ~RefineState() { drop(); }
};

// The kept states, one per device (lsnRefineRelease frees them).  Never destroyed: no HIP calls from static destructors at process exit.
struct RefineStates {
    std::mutex mu;
    std::map<int, RefineState *> of_device;
};

static RefineStates &refine_states()
{
    static RefineStates *all = new RefineStates();
    return *all;
}

static RefineState &refine_state(int device)
{
    RefineStates &all = refine_states();
    std::lock_guard<std::mutex> g(all.mu);
    RefineState *&st = all.of_device[device];
    if (!st) st = new RefineState();
    return *st;
}

// The Gauss-Seidel loop (:347-376) on clouds that are resident: rs.d_all holds every sensor's current cloud, sensor i's counts[i] points at
// 3 * off[i] floats, and rs.d_Rt its accumulated pose {R[9], t[3]} at 12 * i.  Everything is queued on rs.s; nothing is waited for.
// plane: the point-to-plane pass -- rs.d_nrm holds every sensor's current normals like rs.d_all its points, "all other sensors" is
// concatenated for both, and after sensor i's call its normals are recomputed as n0_i R_i from the original ones (rs.d_nrm0) and the
// accumulated pose.
// 0, or non-zero with the message set or a HIP error pending.
static int refine_gauss_seidel(const char *who, RefineState &rs, int n_sensors, const int *counts, const long long *off, int n_refine_iters,
                               int n_icp_iters, bool plane)
{
    hipStream_t s = rs.s;
    LsnIcp *ws = rs.ws;
    lsn::DevBuf &d_all = rs.d_all, &d_others = rs.d_others, &d_Rt = rs.d_Rt, &d_seeds = rs.d_seeds;
    const long long total = off[n_sensors];
    int rc = 0;
    for (int it = 0; it < n_refine_iters && !rc; it++) {                  // :347
        for (int i = 0; i < n_sensors && !rc; i++) {                      // :349
            // :352-357 all other sensors' current clouds, in sensor order = everything before sensor i's block and everything behind it: two copies
            const long long pos = total - counts[i];
            auto gather_others = [&](lsn::DevBuf &dst, const lsn::DevBuf &src) {
                if (!rc && off[i] > 0)
                    rc = hipMemcpyAsync(dst.as<float>(), src.as<float>(), sizeof(float) * 3 * (size_t)off[i], hipMemcpyDeviceToDevice, s) != hipSuccess;
                if (!rc && off[i + 1] < total)
                    rc = hipMemcpyAsync(dst.as<float>() + 3 * off[i], src.as<float>() + 3 * off[i + 1], sizeof(float) * 3 * (size_t)(total - off[i + 1]),
                                        hipMemcpyDeviceToDevice, s) != hipSuccess;
            };
            gather_others(d_others, d_all);
            if (plane) gather_others(rs.d_nrm_others, rs.d_nrm);
            // From the second pass on the first NN step of a call is seeded with the neighbours the sensor's call of the previous pass ended
            // with ("all other sensors" is the same concatenation in every pass, so the indices still name real points; the others have moved a
            // little, which only makes the seeds a little less tight): ~65 us instead of ~150 for that step, same result (14.23-14.38 ->
            // 13.98-14.07 ms per call, same digest).
            if (!rc)
                rc = lsn::guarded(who, -1, [&]() {
                    return icp_run(plane ? "lsnIcpRunPlane" : "lsnIcpRun", ws, d_others.as<float>(), plane ? rs.d_nrm_others.as<float>() : (const float *)nullptr,
                                   (int)pos, d_all.as<float>() + 3 * off[i], counts[i], d_Rt.as<float>() + 12 * i, d_Rt.as<float>() + 12 * i + 9,
                                   n_icp_iters, 1, s, it > 0 ? d_seeds.as<int>() + off[i] : (const int *)nullptr);     // :370
                });
            if (!rc && plane) {
                hipLaunchKernelGGL(rotate_normals_kernel, dim3(blocks_for(counts[i])), dim3(kThreads), 0, s, (const float *)rs.d_nrm0.as<float>() + 3 * off[i],
                                   (const float *)d_Rt.as<float>() + 12 * i, rs.d_nrm.as<float>() + 3 * off[i], counts[i]);
                rc = hipGetLastError() != hipSuccess;
            }
            if (!rc && it + 1 < n_refine_iters)
                rc = hipMemcpyAsync(d_seeds.as<int>() + off[i], ws->idx.p, sizeof(int) * (size_t)counts[i], hipMemcpyDeviceToDevice, s) != hipSuccess;
        }
    }
    return rc;
}

// What a pass is, by its clouds' sizes: off[i] = first point of sensor i, off[n_sensors] = all points.  `runnable` is the rule of every refine
// export: at least two sensors, none of them empty, at least one pass of at least one ICP iteration (MainWindowForm.cs:469-473 guards the
// same way; ICP on an empty cloud would throw out of nanoflann in the reference).
struct RefineShape {
    std::vector<long long> off;
    long long total = 0;
    int max_n = 0, min_n = INT_MAX;
    bool runnable = false;
    RefineShape(int n_sensors, const int *counts, int n_refine_iters, int n_icp_iters) : off((size_t)n_sensors + 1, 0)
    {
        for (int i = 0; i < n_sensors; i++) {
            off[i + 1] = off[i] + counts[i];
            max_n = counts[i] > max_n ? counts[i] : max_n;
            min_n = counts[i] < min_n ? counts[i] : min_n;
        }
        total = off[n_sensors];
        runnable = n_sensors >= 2 && min_n > 0 && total - min_n <= (long long)INT_MAX && n_refine_iters > 0 && n_icp_iters > 0;
    }
};

// One pass on `device`, on the device's kept state: fill(rs, off) queues on rs.s whatever brings the clouds into rs.d_all; the Gauss-Seidel
// loop runs if the shape is runnable; drain(rs) queues the copies that take the clouds wherever the caller wants them; Rt (n_sensors x 12,
// handed in as {I, 0}) receives the accumulated poses.  Complete on return.  -1: the message is set and nothing of the pass is kept.
// d_normals (device, nullable): shape.total x 3 floats, the clouds' normals in d_all's order, final -- the pass is the point-to-plane one.
template <class Fill, class Drain>
static int refine_pass(const char *who, int device, int n_sensors, const int *counts, const RefineShape &shape, int n_refine_iters, int n_icp_iters,
                       float *Rt, const float *d_normals, Fill &&fill, Drain &&drain)
{
    const long long total = shape.total;
    const size_t rt_bytes = sizeof(float) * 12 * (size_t)n_sensors;
    LSN_HIP(hipSetDevice(device));
    // the pass's device state (workspace, cloud buffers, stream) is kept between calls: allocating it was 2-3 ms of a 20 ms pass.
    // A second pass running at the same time on the device gets a state of its own.
    RefineState *rs = &refine_state(device);
    std::unique_lock<std::mutex> hold(rs->mu, std::try_to_lock);
    RefineState own;
    if (!hold.owns_lock()) rs = &own;
    int rc = 0;
    if (shape.runnable) {
        const int need1 = (int)(total - shape.min_n), need2 = shape.max_n;
        if (rs->ws && (rs->ws->max_n1 < need1 || rs->ws->max_n2 < need2)) rs->drop();
        if (!rs->ws) rs->ws = lsnIcpCreate(device, need1, need2);
        rc = rs->ws ? 0 : -1;
    }
    rs->device = device;
    if (!rc && !rs->s) rc = hipStreamCreateWithFlags(&rs->s, hipStreamNonBlocking) != hipSuccess;
    hipStream_t s = rs->s;
    if (!rc) rc = rs->d_all.reserve(sizeof(float) * 3 * (size_t)total);
    if (!rc && shape.runnable)
        rc = rs->d_others.reserve(sizeof(float) * 3 * (size_t)(total - shape.min_n)) || rs->d_Rt.reserve(rt_bytes) ||
             rs->d_seeds.reserve(sizeof(int) * (size_t)total);
    if (!rc && shape.runnable && d_normals)
        rc = rs->d_nrm.reserve(sizeof(float) * 3 * (size_t)total) || rs->d_nrm0.reserve(sizeof(float) * 3 * (size_t)total) ||
             rs->d_nrm_others.reserve(sizeof(float) * 3 * (size_t)(total - shape.min_n));
    // (allocated before anything is queued: once a copy into host memory is in flight nothing below may throw before the synchronise)
    std::vector<float> Rt_back(shape.runnable ? 12 * (size_t)n_sensors : 0);
    if (!rc) rc = fill(*rs, shape.off.data());
    if (!rc && shape.runnable) {
        rc = hipMemcpyAsync(rs->d_Rt.p, Rt, rt_bytes, hipMemcpyHostToDevice, s) != hipSuccess;
        if (!rc && d_normals)
            rc = hipMemcpyAsync(rs->d_nrm0.p, d_normals, sizeof(float) * 3 * (size_t)total, hipMemcpyDeviceToDevice, s) != hipSuccess ||
                 hipMemcpyAsync(rs->d_nrm.p, d_normals, sizeof(float) * 3 * (size_t)total, hipMemcpyDeviceToDevice, s) != hipSuccess;
        if (!rc) rc = refine_gauss_seidel(who, *rs, n_sensors, counts, shape.off.data(), n_refine_iters, n_icp_iters, d_normals != nullptr);
    }
    // results land in scratch first: the caller's arrays are only touched when everything worked
    if (!rc) rc = drain(*rs);
    if (!rc && shape.runnable) rc = hipMemcpyAsync(Rt_back.data(), rs->d_Rt.p, rt_bytes, hipMemcpyDeviceToHost, s) != hipSuccess;
    if (!rc && s) rc = hipStreamSynchronize(s) != hipSuccess;
    if (rc) {
        if (!lsn::has_error()) lsn::set_error("%s: %s", who, hipGetErrorString(hipGetLastError()));
        if (s) (void)hipStreamSynchronize(s);
        rs->drop();   // nothing of a failed pass is kept
        return -1;
    }
    if (shape.runnable) memcpy(Rt, Rt_back.data(), rt_bytes);
    return 0;
}

static void identity_poses(std::vector<float> &Rt, int n_sensors)
{
    Rt.assign((size_t)n_sensors * 12, 0.0f);
    for (int i = 0; i < n_sensors; i++)
        for (int j = 0; j < 3; j++) Rt[(size_t)i * 12 + j + j * 3] = 1.0f;   // Rs[i] = I, Ts[i] = 0 (:330-344)
}

// :382-410 pose composition, the C# loops as written (f32, every product rounded before it is added: the build keeps contraction off).
// The rows of worldTransforms[i].R are overwritten while later rows still read it (:398-406), so the result is not Rs^T * R unless R is
// orthogonal to the last bit -- the reference's behaviour, kept.  Rs / Ts: pose i at Rs + stride_R * i / Ts + stride_T * i.
// A null world pair leaves the camera rotations alone (:407 copies what :403 computed from the world rotation); the camera translations
// (:394) need the ICP translations only.
static void compose_poses(int n, const float *Rs, int stride_R, const float *Ts, int stride_T, float *world_R, float *world_t, float *camera_R,
                          float *camera_t)
{
    const bool world = world_R && world_t, camera = camera_R && camera_t;
    for (int i = 0; i < n; i++) {
        const float *Ri = Rs + (size_t)stride_R * i, *Ti = Ts + (size_t)stride_T * i;
        if (world) {
            float *WR = world_R + 9 * i, *Wt = world_t + 3 * i;
            float tempT[3] = {0, 0, 0};
            for (int j = 0; j < 3; j++) {
                for (int k = 0; k < 3; k++) tempT[j] += Ti[k] * WR[3 * k + j];
                Wt[j] += tempT[j];
            }
        }
        if (camera)
            for (int j = 0; j < 3; j++) camera_t[3 * i + j] += Ti[j];   // :394
        if (world) {
            float *WR = world_R + 9 * i;
            float tempR[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int j = 0; j < 3; j++)
                for (int k = 0; k < 3; k++) {
                    for (int l = 0; l < 3; l++) tempR[3 * j + k] += Ri[l * 3 + j] * WR[3 * l + k];
                    WR[3 * j + k] = tempR[3 * j + k];
                    if (camera) camera_R[9 * i + 3 * j + k] = tempR[3 * j + k];   // :407
                }
        }
    }
}

void lsn::refine_compose(int n, const float *Rt, float *world_R, float *world_t, float *camera_R, float *camera_t, float *Rs_out, float *Ts_out)
{
    compose_poses(n, Rt, 12, Rt + 9, 12, world_R, world_t, camera_R, camera_t);
    for (int i = 0; i < n; i++) {
        if (Rs_out) memcpy(Rs_out + 9 * i, Rt + 12 * (size_t)i, 9 * sizeof(float));
        if (Ts_out) memcpy(Ts_out + 3 * i, Rt + 12 * (size_t)i + 9, 3 * sizeof(float));
    }
}

extern "C" int lsnRefineComposePoses(int n, const float *Rs, const float *Ts, float *world_R, float *world_t, float *camera_R, float *camera_t)
{
    return lsn::guarded("lsnRefineComposePoses", -1, [&]() {
        lsn::clear_error();
        if (n <= 0 || !Rs || !Ts) {
            lsn::set_error("lsnRefineComposePoses: bad arguments");
            return -1;
        }
        compose_poses(n, Rs, 9, Ts, 3, world_R, world_t, camera_R, camera_t);
        return 0;
    });
}

extern "C" int lsnRefine(int device, int n_sensors, float *const *clouds, const int *counts, int n_refine_iters, int n_icp_iters,
                         float *world_R, float *world_t, float *Rs_out, float *Ts_out)
{
    return lsn::guarded("lsnRefine", -1, [&]() {
        lsn::clear_error();
        if (n_sensors <= 0 || !clouds || !counts) {
            lsn::set_error("lsnRefine: bad arguments");
            return -1;
        }
        for (int i = 0; i < n_sensors; i++) {
            if (counts[i] < 0 || (counts[i] > 0 && !clouds[i])) {
                lsn::set_error("lsnRefine: bad cloud %d", i);
                return -1;
            }
        }
        const RefineShape shape(n_sensors, counts, n_refine_iters, n_icp_iters);
        std::vector<float> Rt;
        identity_poses(Rt, n_sensors);
        if (shape.runnable) {
            std::vector<float> back((size_t)shape.total * 3);   // before the pass: nothing may throw between the queued download and its synchronise
            const int rc = refine_pass(
                "lsnRefine", device, n_sensors, counts, shape, n_refine_iters, n_icp_iters, Rt.data(), nullptr,
                [&](RefineState &rs, const long long *off) -> int {
                    int bad = 0;
                    for (int i = 0; i < n_sensors && !bad; i++)
                        bad = hipMemcpyAsync(rs.d_all.as<float>() + 3 * off[i], clouds[i], sizeof(float) * 3 * (size_t)counts[i], hipMemcpyHostToDevice, rs.s) != hipSuccess;
                    return bad;
                },
                [&](RefineState &rs) -> int {
                    return hipMemcpyAsync(back.data(), rs.d_all.p, sizeof(float) * 3 * (size_t)shape.total, hipMemcpyDeviceToHost, rs.s) != hipSuccess;
                });
            if (rc) return -1;
            for (int i = 0; i < n_sensors; i++) memcpy(clouds[i], back.data() + 3 * shape.off[i], sizeof(float) * 3 * (size_t)counts[i]);
        }
        lsn::refine_compose(n_sensors, Rt.data(), world_R, world_t, nullptr, nullptr, Rs_out, Ts_out);
        return 0;
    });
}

// The pass on ONE tick's merged cloud that is resident on `device` and final (nothing that writes it is still in flight): the vertices are
// stripped to points (refine_xyz.hip), refined where they lie, and leave as the caller asks -- h_clouds (host, nullable) and d_clouds
// (device, nullable) each receive offsets[n_sensors] - offsets[0] points, sensor blocks in sensor order.  offsets: the tick's row on the
// HOST.  Rt: n_sensors x 12, receives {Rs[i], Ts[i]} ({I, 0} when the shape is not runnable: then the clouds leave as they came).
int lsn::refine_cloud(const char *who, int device, int n_sensors, const void *d_vertices, const int *offsets, int n_refine_iters, int n_icp_iters,
                      float *Rt, float *h_clouds, float *d_clouds, const float *d_normals)
{
    std::vector<int> counts((size_t)n_sensors);
    bool bad = offsets[0] < 0;
    for (int i = 0; i < n_sensors; i++) {
        bad |= offsets[i + 1] < offsets[i];
        counts[i] = offsets[i + 1] - offsets[i];
    }
    if (bad) {
        lsn::set_error("%s: the offsets row is not one a fusion wrote (it must start at >= 0 and never decrease)", who);
        return -1;
    }
    const RefineShape shape(n_sensors, counts.data(), n_refine_iters, n_icp_iters);
    std::vector<float> poses;
    identity_poses(poses, n_sensors);
    const size_t cloud_bytes = sizeof(float) * 3 * (size_t)shape.total;
    const int rc = refine_pass(
        who, device, n_sensors, counts.data(), shape, n_refine_iters, n_icp_iters, poses.data(), d_normals ? d_normals + 3 * (size_t)offsets[0] : nullptr,
        [&](RefineState &rs, const long long *) -> int {
            return xyz_of_vertices(static_cast<const char *>(d_vertices) + (size_t)offsets[0] * sizeof(VertexC4ubV3f), rs.d_all.as<float>(), (int)shape.total, rs.s);
        },
        [&](RefineState &rs) -> int {
            if (cloud_bytes == 0) return 0;
            if (h_clouds && hipMemcpyAsync(h_clouds, rs.d_all.p, cloud_bytes, hipMemcpyDeviceToHost, rs.s) != hipSuccess) return 1;
            if (d_clouds && hipMemcpyAsync(d_clouds, rs.d_all.p, cloud_bytes, hipMemcpyDeviceToDevice, rs.s) != hipSuccess) return 1;
            return 0;
        });
    if (rc) return -1;
    memcpy(Rt, poses.data(), sizeof(float) * poses.size());
    return 0;
}

// The body of lsnRefineVertices and lsnRefineVerticesPlane under the export's name `who`; plane: d_normals is required (else it is null).
static int refine_vertices(const char *who, bool plane, int device, int n_sensors, const void *d_vertices, const float *d_normals, const int *d_offsets,
                           int n_refine_iters, int n_icp_iters, float *world_R, float *world_t, float *camera_R, float *camera_t, float *Rs_out,
                           float *Ts_out, float *d_clouds_out, void *stream)
{
    return lsn::guarded(who, -1, [&]() {
        lsn::clear_error();
        // (the strip kernel loads a vertex as one 16-byte word)
        if (n_sensors <= 0 || !d_vertices || (plane && !d_normals) || !d_offsets || (reinterpret_cast<uintptr_t>(d_vertices) & 15) != 0) {
            lsn::set_error("%s: bad arguments", who);
            return -1;
        }
        LSN_HIP(hipSetDevice(device));
        // behind everything queued on the caller's stream: once the row is here, the cloud (and the normals) it describes are final
        std::vector<int> offsets((size_t)n_sensors + 1);
        LSN_HIP(hipMemcpyAsync(offsets.data(), d_offsets, sizeof(int) * offsets.size(), hipMemcpyDeviceToHost, lsn::as_stream(stream)));
        LSN_HIP(hipStreamSynchronize(lsn::as_stream(stream)));
        std::vector<float> Rt((size_t)n_sensors * 12);
        if (lsn::refine_cloud(who, device, n_sensors, d_vertices, offsets.data(), n_refine_iters, n_icp_iters, Rt.data(), nullptr, d_clouds_out, d_normals))
            return -1;
        lsn::refine_compose(n_sensors, Rt.data(), world_R, world_t, camera_R, camera_t, Rs_out, Ts_out);
        return 0;
    });
}

extern "C" int lsnRefineVertices(int device, int n_sensors, const void *d_vertices, const int *d_offsets, int n_refine_iters, int n_icp_iters,
                                 float *world_R, float *world_t, float *camera_R, float *camera_t, float *Rs_out, float *Ts_out,
                                 float *d_clouds_out, void *stream)
{
    return refine_vertices("lsnRefineVertices", false, device, n_sensors, d_vertices, nullptr, d_offsets, n_refine_iters, n_icp_iters, world_R, world_t,
                           camera_R, camera_t, Rs_out, Ts_out, d_clouds_out, stream);
}

extern "C" int lsnRefineVerticesPlane(int device, int n_sensors, const void *d_vertices, const float *d_normals, const int *d_offsets, int n_refine_iters,
                                      int n_icp_iters, float *world_R, float *world_t, float *camera_R, float *camera_t, float *Rs_out, float *Ts_out,
                                      float *d_clouds_out, void *stream)
{
    return refine_vertices("lsnRefineVerticesPlane", true, device, n_sensors, d_vertices, d_normals, d_offsets, n_refine_iters, n_icp_iters, world_R,
                           world_t, camera_R, camera_t, Rs_out, Ts_out, d_clouds_out, stream);
}

extern "C" long long lsnRefineRelease(int device)
{
    return lsn::guarded("lsnRefineRelease", -1LL, [&]() -> long long {
        lsn::clear_error();
        std::vector<RefineState *> states;
        {
            RefineStates &all = refine_states();
            std::lock_guard<std::mutex> g(all.mu);
            for (const auto &kv : all.of_device)
                if (device < 0 || kv.first == device) states.push_back(kv.second);
        }
        long long released = 0;
        for (RefineState *st : states) {
            std::lock_guard<std::mutex> g(st->mu);   // a pass in flight on this state ends first
            const long long held = st->bytes();
            if (held == 0 && !st->s) continue;       // never used, or released already: no device is touched
            st->drop();
            released += held;
        }
        return released;
    });
}
