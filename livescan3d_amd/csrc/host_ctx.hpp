// host_ctx.hpp -- the process-wide context behind the reference's exports on HOST arrays: lanes (streams, device buffers, plan tables), the
// pool of pinned mesh blocks, the devices of $LSN_HOST_DEVICES with their worker threads -- the record of the opt-in stages in front of
// the radial correction that a call carries (DepthStages) with the lane's side of them (DepthChain), the record of a mesh call (MeshCall)
// -- and the entry points of the three call flows that run on it (host_flows.hip; the design notes are at the top of that file).
// abi.hip holds the exports themselves.
#pragma once

#include "lsn_common.hpp"

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <unordered_map>
#include <vector>

namespace lsn {
namespace host {

// One group of consecutive sensors of a call: fused by one launch as soon as its frames are on the device (file comment).
struct Group {
    int first = 0, count = 0;        // sensors [first, first + count) of the caller's arrays
    size_t d_off = 0, c_off = 0;     // where the group's frames start in the lane's device buffers (bytes)
    size_t d_src = 0, c_src = 0;     // ... and in the caller's arrays
    size_t dbytes = 0, cbytes = 0;
    int ready_after = 0;             // how many copies of the call's upload schedule must have landed before its launch
    LsnFusion *radial_plan = nullptr;   // calls that start with the radial correction: the group's own plan for it (its warp tables)
};

// One blocking upload of the schedule: a run of whole frames of the caller's depth or colour array.
struct Copy {
    size_t dev_off = 0, src_off = 0, bytes = 0;
    bool colours = false;
};

constexpr int kMaxGroups = 16;

struct Ctx;

// The opt-in stages on a call's raw u16 depth maps, in front of its radial correction, in the order they run: the temporal depth filter
// (temporal.hip, lsnSetTemporalFilter) with the generation of lsnResetTemporalFilter, background subtraction (background.hip,
// lsnSetBackground) with the generation of lsnLearnBackground and the learning calls it asked for, the flying-pixel filter (flying.hip,
// lsnSetFlyingPixelFilter), depth smoothing (depth_smooth.hip, lsnSetDepthSmooth; the Gaussian tables, null: off).  The export fills it from
// the process-wide switches (abi.hip); this is the one place that says when a stage runs.
struct DepthStages {
    lsn::TemporalSetting temporal;
    unsigned long long temporal_gen = 0;
    lsn::BackgroundSetting background;
    unsigned long long background_gen = 0;
    int background_learn = 0;        // the learning calls a lane runs when it starts a generation
    bool background_on() const { return background.on(); }
    int fp_neighbourhood = 0, fp_threshold = 0;
    std::shared_ptr<const lsn::DepthSmoothTables> smooth;
    bool temporal_on() const { return temporal.on(); }
    bool flying_on() const { return lsn::flying_on(fp_neighbourhood); }
    bool smooth_on() const { return smooth != nullptr && lsn::smooth_on(smooth->radius); }
};

// A lane's side of those stages: each stage's output, laid out like the lane's d_depth, which the next stage or the correction reads; and
// for the two stages with state their record (lsn::StageState) for the rig the lane sees call after call -- the temporal filter's history,
// one word per pixel at the sensor's offset in the call's arrays (so neither grouping nor the host path changes which word a pixel owns),
// and background subtraction's model, one u16 per pixel -- keyed by the rig (sensor count, widths, heights) and the generation of
// lsnResetTemporalFilter / lsnLearnBackground; for the model also the learning calls the lane still owes, and the blob pass's scratch.  All
// allocated by the first call that runs the stage.
struct DepthChain {
    lsn::DevBuf d_temporal, d_background, d_flying, d_smooth, bg_blob;
    struct Keyed {
        lsn::StageState st;
        std::vector<int> rig;
        unsigned long long gen = 0;
        Keyed(size_t px_bytes, size_t pad) : st(px_bytes, pad) {}
    };
    Keyed tp{4, 0}, bg{2, 16};
    int bg_learn_left = 0;           // learning calls still to come
    bool bg_learning = false;        // ... and whether the call in progress is one (decided once per call, in reserve())
    // the state up to date for a call of this rig and generation: zeroed when either changed (`fresh`)
    static int keyed(Keyed &k, const std::vector<int> &rig, size_t pixels, unsigned long long gen, hipStream_t s, bool &fresh)
    {
        fresh = !(k.st.state.p && rig == k.rig && gen == k.gen);
        if (!fresh) return 0;
        const bool grown = !k.st.state.p || k.st.state.bytes < k.st.px_bytes * pixels + k.st.pad;
        if (k.st.reserve(pixels, s)) return -1;   // (a new buffer comes zeroed)
        if (!grown && k.st.reset(pixels, s)) return -1;
        k.rig = rig;
        k.gen = gen;
        return 0;
    }
    // What the stages that are on need for a call whose depth block has `dbytes` bytes and whose sensors are widths / heights [0, count).
    int reserve(const DepthStages &st, size_t dbytes, const int *widths, const int *heights, int count, hipStream_t s)
    {
        std::vector<int> rig;
        size_t pixels = 0;
        if (st.temporal_on() || st.background_on()) {
            rig.assign(1, count);
            rig.insert(rig.end(), widths, widths + count);
            rig.insert(rig.end(), heights, heights + count);
            for (int i = 0; i < count; i++) pixels += (size_t)widths[i] * heights[i];
        }
        bool fresh = false;
        if (st.temporal_on() && (d_temporal.reserve(dbytes + 16) || keyed(tp, rig, pixels, st.temporal_gen, s, fresh))) return -1;
        if (st.background_on()) {   // a call is one tick and counts once, whichever groups the host path cuts it into
            if (d_background.reserve(dbytes + 16) || keyed(bg, rig, pixels, st.background_gen, s, fresh)) return -1;
            if (fresh) bg_learn_left = st.background_learn;   // a new model has that many learning calls ahead
            bg_learning = bg_learn_left > 0;
            if (bg_learning) bg_learn_left--;
        }
        if (st.flying_on() && d_flying.reserve(dbytes + 16)) return -1;
        if (st.smooth_on() && d_smooth.reserve(dbytes + 16)) return -1;
        return 0;
    }
    // Queues the stages that are on for one plan's maps, which start `off` bytes into the lane's depth block `d_depth` (and so into every
    // buffer here; the history word and the model value of a pixel are at off / 2), the temporal filter and the subtraction as ONE tick.
    // Returns the maps the correction must read -- d_depth + off itself when nothing is on -- or null with the message set.
    const void *run(LsnFusion *plan, const DepthStages &st, const lsn::DevBuf &d_depth, size_t off, hipStream_t s)
    {
        const char *in = d_depth.as<char>() + off;
        if (st.temporal_on()) {
            char *out = d_temporal.as<char>() + off;
            if (lsn::temporal(plan, st.temporal, in, out, tp.st.state.as<unsigned int>() + off / 2, tp.st.counts, 1, s)) return nullptr;
            in = out;
        }
        if (st.background_on()) {   // a learning call folds its maps into the model and passes them on as they are
            unsigned short *model = bg.st.state.as<unsigned short>() + off / 2;
            char *out = d_background.as<char>() + off;
            if (bg_learning) {
                if (lsn::background_learn(plan, in, model, 1, s)) return nullptr;
            } else {
                if (lsn::background(plan, st.background, in, out, model, bg.st.counts, bg_blob, 1, s)) return nullptr;
                in = out;
            }
        }
        if (st.flying_on()) {
            char *out = d_flying.as<char>() + off;
            if (lsn::flying_pixels(plan, st.fp_neighbourhood, st.fp_threshold, in, out, s)) return nullptr;
            in = out;
        }
        if (st.smooth_on()) {   // the plan takes the call's tables first (nothing to do when it has them)
            const lsn::DepthSmoothTables &t = *st.smooth;
            char *out = d_smooth.as<char>() + off;
            if (lsn::set_depth_smooth(plan, "lsnSetDepthSmooth", t.radius, t.spatial, t.range, t.n_range) || lsn::depth_smooth(plan, in, out, s)) return nullptr;
            in = out;
        }
        return in;
    }
};

// What one call in flight needs: streams, events, device buffers, plans.  LiveScanServer runs its merge calls (updateWorker: radial
// correction, generateMeshFromDepthMaps) and its refine calls (refineWorker: generateVerticesFromDepthMap per sensor, then ICP) on two
// threads (MainWindowForm.cs:238,304); each of the three families has its own lane, so they only meet at the pool of pinned blocks.
struct Lane {
    std::mutex mu;
    int device = 0;           // the device the lane's streams, buffers and plans live on
    hipStream_t stream = nullptr, up = nullptr, down = nullptr, back = nullptr;   // kernels; uploads; mesh downloads; write-backs of corrected maps
    hipEvent_t ev_group[kMaxGroups] = {};    // "group g's vertices are in HBM (and its corrected maps final)"
    hipEvent_t ev_tri = nullptr;             // "the triangle counts are known"
    int *h_off = nullptr, *h_toff = nullptr;   // pinned: the offset tables of the call in progress
    int h_off_cap = 0;
    lsn::DevBuf d_depth, d_colors, d_depth2, d_colors2, d_out, d_off, d_tri, d_tri_off;
    lsn::DevBuf d_masked;     // a call with the outlier filter on: its depth maps with the removed vertices' pixels at 0 (allocated by the first such call)
    DepthChain pre;           // a call that starts at raw frames with stages in front of the correction: their scratch and history
    // the lane's plans: key = n sensors, first sensor, widths..., heights...  Owned by the lane and only touched under its lock, so a
    // plan never runs on two lanes' streams at once and an eviction cannot pull a plan from under the other lane's call
    std::map<std::vector<int>, LsnFusion *> plans;
    // The mesh of the lane's last call (lsnLastMesh* read it): its vertex / triangle counts, and whether it is in d_out / d_tri.
    // The direct path stores the mesh to host memory only; the inputs stay in d_depth / d_colors (d_depth2 / d_colors2 after the
    // radial correction), so the mesh can be rebuilt in HBM by last_plan when somebody asks for it.
    int last_nv = -1, last_nt = 0;
    bool last_in_hbm = false, last_radial = false, last_tri = false;
    LsnFusion *last_plan = nullptr;
    // ... or it was a call sharded over the devices of $LSN_HOST_DEVICES: the mesh only exists in host memory and its inputs are spread
    // over the shards' lanes; what materialize() needs to rebuild it here
    bool last_sharded = false;
    std::vector<int> last_w, last_h;
    std::vector<float> last_intr, last_wt, last_bounds;
    std::vector<Group> groups;
    std::vector<Copy> copies;
    // the lane's buffers are about to be reused: until a call publishes its mesh, lsnLastMesh* have nothing to read
    void forget_last()
    {
        last_nv = -1;
        last_plan = nullptr;
        last_sharded = false;
    }
    // the mesh of the call that just ended is the lane's last, and the lane the last of its thread and of the process (host_flows.hip)
    void publish_last(Ctx &c, int nv, int nt, bool in_hbm, bool sharded, bool radial, bool with_triangles);
};

// A thread that runs one job at a time for the thread that hands it over.  A pageable upload keeps the thread that issues it until the
// bytes are on the device (file comment), so D links are only busy at once when D threads issue the copies: one worker per device of
// $LSN_HOST_DEVICES beyond the first (the calling thread serves the first).  Started on first use, never joined (the context is never
// destroyed): an idle worker sits in its condition variable and touches nothing.
struct Worker {
    std::mutex mu;
    std::condition_variable cv;
    void (*fn)(void *, int) = nullptr;
    void *arg = nullptr;
    int index = 0;
    bool busy = false, started = false;
    void loop()
    {
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv.wait(lk, [&] { return fn != nullptr; });
            void (*f)(void *, int) = fn;
            void *a = arg;
            const int i = index;
            fn = nullptr;
            lk.unlock();
            f(a, i);   // never throws: the job catches everything itself
            lk.lock();
            busy = false;
            cv.notify_all();
        }
    }
    void submit(void (*f)(void *, int), void *a, int i)
    {
        std::unique_lock<std::mutex> lk(mu);
        if (!started) {
            std::thread(&Worker::loop, this).detach();
            started = true;
        }
        fn = f;
        arg = a;
        index = i;
        busy = true;
        cv.notify_all();
    }
    void wait()
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !busy; });
    }
};

// One device of $LSN_HOST_DEVICES: its lane (streams, buffers, plans -- only used under the merge lane's lock) and its worker.
struct HostShard {
    Lane lane;
    Worker worker;
};

constexpr int kMaxShards = 16;

struct Ctx {
    Lane merge, single;       // lane of the merge / radial / last-mesh calls; lane of the single-sensor calls
    std::mutex icp_mu;        // ICP: own buffers, own stream
    std::mutex init_mu;
    std::mutex tab_mu;        // the pool of pinned blocks
    std::atomic<Lane *> last_lane{nullptr};   // the lane whose call finished last: lsnLastMesh* read the mesh it left in HBM
    bool ready = false;
    int device = 0;
    std::vector<HostShard *> shards;   // $LSN_HOST_DEVICES=a,b,...: merge calls are sharded over these devices (>= 2 entries; an entry may repeat)
    int host_path = 0;        // $LSN_HOST_PATH: 0 = by call (default), 1 = "direct" (kernel stores) always, 2 = "grouped" (copy engine) always
    int group_override = 0;   // $LSN_HOST_GROUP: sensors per group (0 = by size)
    hipStream_t icp_stream = nullptr;
    lsn::DevBuf d_v1, d_v2, d_Rt, d_n1;   // d_n1: the target's normals (lsnIcpPointToPlane)
    LsnIcp *icp = nullptr;
    int icp_n1 = 0, icp_n2 = 0;
    // pinned host blocks handed out as Mesh::vertices, recycled by deleteMesh
    std::unordered_map<void *, size_t> live;          // ptr -> capacity (bytes)
    std::multimap<size_t, void *> pool;               // capacity -> ptr
    std::mutex wire_mu;       // the packer and its output buffer (lsnLastMesh*)
    LsnTransfer *xfer = nullptr;
    int xfer_v = 0, xfer_t = 0;
    lsn::DevBuf d_wire;
    // the steps of lsnLastMesh* (abi.hip LastMesh; under wire_mu too): the mesh's two counts as offset rows {0, nVertices}, {0, nTriangles}
    // and behind them the rows the level of detail writes, then the rows the fragment filter writes; the stages' scratch; the simplified
    // mesh, the filtered mesh, the normals, the rendered image
    lsn::DevBuf d_mesh_rows;
    int mesh_rows[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    lsn::RenderScratch rv;
    lsn::SimplifyScratch sp;
    lsn::FragmentsScratch fr;
    lsn::NormalsScratch nm;
    lsn::SmoothScratch sm;
    lsn::DevBuf d_lod_v, d_lod_t, d_frag_v, d_frag_t, d_sm_v, d_nm, d_rv_img;
    bool warned_flags = false;
};

// the lane of the calling thread's own last mesh call (lsnLastMesh* read that lane's mesh; include/NativeUtils.h)
extern thread_local Lane *t_last_lane;

Ctx &ctx();
int ensure_ready(Ctx &c);                  // takes c.init_mu itself; callers may hold a lane's lock or c.icp_mu
void drain(Lane &l);                       // waits for everything the lane has in flight
void *pinned_get(Ctx &c, size_t bytes);    // a pinned block of the pool (handed out as Mesh::vertices / Mesh::triangles; ICP's scratch)
void pinned_put(Ctx &c, void *p);          // ... back (a pointer that is not ours is left alone)
extern int g_no_triangles[1];              // what Mesh::triangles points at when a mesh has no triangles
void empty_mesh(Mesh *m) noexcept;

// The upload schedule of a call (pure host logic: lsnHostScheduleDescribe) and the split of a call over devices (lsnHostShardDescribe).
void plan_schedule(std::vector<Group> &groups, std::vector<Copy> &copies, const int *widths, const int *heights, int first, int count, bool radial,
                   int group_override, bool small_first);
void plan_shards(int count, int n_devices, int *first, int &D);
int parse_device_list(const char *text, int n_visible, std::vector<int> &out);

// What one mesh call is, as its export received it.  A record that the export fills by name and the flows read: nothing is decided in it.
struct MeshCall {
    const unsigned char *depth_maps = nullptr, *depth_colors = nullptr;   // the caller's packed frames of ALL its sensors ...
    const int *widths = nullptr, *heights = nullptr;
    const float *intr = nullptr, *wt = nullptr;                           // ... their intrinsics [7] and world transforms [12] ...
    const float *bounds6 = nullptr;                                       // ... and the crop box
    int first = 0, count = 0;                // the sensors of the call: [first, first + count) (generateVerticesFromDepthMap uses one)
    bool with_triangles = false;
    bool radial = false;                     // the call starts with the radial correction of the frames, on the device
    unsigned char *back_d = nullptr, *back_c = nullptr;   // optional: the corrected maps are also copied to these host arrays, like the separate export does
    bool color_transfer = false, overlay_merge = false;   // the stages on the fused cloud (color.hip, merge.hip) ...
    int outlier_k = 0;                       // ... and the outlier filter (outlier.hip, lsnSetOutlierFilter): it runs when outlier_k > 0
    float outlier_max_dist = 0.0f;           //     and outlier_max_dist > 0
    int blend_tol = 0, blend_min_conf = 0;   // ... and the colour blend (color_blend.hip, lsnSetColorBlend) behind the colour transfer
    DepthStages stages;                      // the stages in front of the radial correction of a call that starts with it (`radial`)
    // the blend runs for depth_tol > 0 and min_confidence <= 20, on more than one sensor (color_blend.hip: everything else changes nothing)
    bool blends() const { return blend_tol > 0 && blend_min_conf <= 20 && count > 1; }
};

// The calls.  The lane's lock is held by the caller; `out` is left untouched on failure (the export then returns an empty mesh).
int fuse_host(Ctx &c, Lane &l, const MeshCall &call, Mesh *out);
void radial_host(Ctx &c, Lane &l, int n_maps, unsigned char *depth_maps, unsigned char *depth_colors, const int *widths, const int *heights,
                 const float *intr_params, const DepthStages &stages);
// The fusion of a call whose cloud stays on the device: vertices only (with the outlier filter if the call has it on) into l.d_out, final on
// return, the tick's offset row (call.count + 1 ints) into `offsets`.  No mesh: the lane is left without a last one.
int fuse_resident(Ctx &c, Lane &l, const MeshCall &call, int *offsets);
int materialize(Lane &l);                // lsnLastMesh*: the mesh of the lane's last call in d_out / d_tri

}  // namespace host
}  // namespace lsn
