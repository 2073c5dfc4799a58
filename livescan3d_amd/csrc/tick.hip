// tick.hip -- the reference's tick, device resident, as ONE call: CorrectRadialDistortionsForDepthMaps then GenerateMesh on every tick
// (LiveScanServer/KinectServer.cs:518-525, :354-374) = lsnFusionRadialCorrectTo + lsnFusionRunMesh on a batch of ticks in HBM.
//
// Why it is a call of its own: the stages of the chain are bound by different things -- the radial correction's closing rounds are a
// latency chain that occupies a quarter of the wave slots for 0.23 ms, the count passes are VALU-bound, the write passes store-bound --
// and a batch cut in two halves that run side by side (the caller's stream and an internal one, two plans) lets one half's waits be
// the other half's work.  Round 4 measured that at +1.7 % and did not build it; with the band kernel regrouped into 27 KB workgroups
// (round 6: room beside the closing's two 64 KB workgroups per CU) two FREE-RUNNING streams gain +4.5 to +6.5 % on scene frames (44.1-44.7 ->
// 46.6-47.4 k ticks/s for 64 ticks x 8 x 512x424; four parts: 42.0 k; hash-noise frames, which have nothing to close: -2 %;
// tools/tick_pipelined.py).  This call forks from and joins to the caller's stream every time -- its outputs are complete on the caller's
// stream when its work there is -- which keeps +2 % of that (45.0-45.1 k against 44.1-44.3; profiles/r06_tick_pipelined.txt): the rest is
// overlap across calls.  Results are those of the two calls on one plan, byte for byte: the halves share nothing but the calibration.
#include "fusion_shared.hpp"

#include <mutex>
#include <vector>

struct LsnTick {
    int device = 0, n_ticks = 0, n_maps = 0, parts = 1;
    LsnFusion *plan[2] = {nullptr, nullptr};
    int first[3] = {0, 0, 0};            // part k covers ticks [first[k], first[k + 1])
    long long cap = 0, tri_cap = 0;      // vertices / triangles per tick
    std::vector<float> intr;             // the radial correction's intrinsics (lsnTickSetParams)
    int fp_neighbourhood = 0, fp_threshold = 0;   // the flying-pixel filter in front of the correction (lsnTickSetFlyingPixels; <= 0: off)
    lsn::DevBuf d_filtered;              // ... and its output, [n_ticks][pixels per tick] u16: reserved by the first run that filters
    int ds_radius = 0;                   // depth smoothing between the filter and the correction (lsnTickSetDepthSmooth; <= 0: off; the plans hold the tables)
    lsn::DevBuf d_smoothed;              // ... and its output, laid out like d_filtered: reserved by the first run that smooths
    // the two stages with state in front of all of them, each with its setting (lsnTickSetTemporal, lsnTickSetBackground; off by default),
    // its record (lsn::StageState: the history, one word per pixel of one tick, and the model, one u16; handed from run to run) and its
    // output, laid out like d_filtered -- all reserved by the first run that needs them: the temporal depth filter, then background subtraction
    lsn::TemporalSetting tp_setting;
    lsn::StageState tp{4, 0};
    lsn::DevBuf d_temporal;
    lsn::BackgroundSetting bg_setting;
    lsn::StageState bg{2, 16};
    lsn::DevBuf bg_blob, d_background;
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_band = nullptr;
    std::mutex mu;
};

// The body of lsnTickDestroy under a name of its own: lsnTickCreate calls it too, on a tick object it could not finish.
static void tick_destroy(LsnTick *t)
{
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->side) {
        (void)hipStreamSynchronize(t->side);
        (void)hipStreamDestroy(t->side);
    }
    if (t->ev_fork) (void)hipEventDestroy(t->ev_fork);
    if (t->ev_join) (void)hipEventDestroy(t->ev_join);
    if (t->ev_band) (void)hipEventDestroy(t->ev_band);
    for (LsnFusion *p : t->plan)
        if (p) lsnFusionDestroy(p);
    delete t;
}

extern "C" void lsnTickDestroy(LsnTick *t)
{
    lsn::guarded_void("lsnTickDestroy", [&]() { tick_destroy(t); });
}

extern "C" LsnTick *lsnTickCreate(int device, int n_ticks, int n_maps, const int *widths, const int *heights)
{
    return lsn::guarded("lsnTickCreate", static_cast<LsnTick *>(nullptr), [&]() -> LsnTick * {
        lsn::clear_error();
        if (n_ticks <= 0 || n_maps <= 0 || !widths || !heights) {
            lsn::set_error("lsnTickCreate: bad arguments");
            return nullptr;
        }
        LsnTick *t = new (std::nothrow) LsnTick();
        if (!t) return nullptr;
        t->device = device;
        t->n_ticks = n_ticks;
        t->n_maps = n_maps;
        // two halves from 8 ticks up ($LSN_TICK_PARTS=1: one plan, one stream -- the two calls as they are)
        int parts = n_ticks >= 8 ? 2 : 1;
        if (const char *e = getenv("LSN_TICK_PARTS")) parts = atoi(e) >= 2 && n_ticks >= 2 ? 2 : 1;
        t->parts = parts;
        t->first[0] = 0;
        t->first[1] = parts == 2 ? (n_ticks + 1) / 2 : n_ticks;
        t->first[2] = n_ticks;
        bool bad = false;
        for (int k = 0; k < parts && !bad; k++) {
            t->plan[k] = lsnFusionCreate(device, t->first[k + 1] - t->first[k], n_maps, widths, heights);
            bad = !t->plan[k];
        }
        if (!bad) {
            t->cap = lsnFusionTickCapacity(t->plan[0]);
            t->tri_cap = lsnFusionTickTriangleCapacity(t->plan[0]);
            bad = hipSetDevice(device) != hipSuccess;
            if (!bad && parts == 2)
                bad = hipStreamCreateWithFlags(&t->side, hipStreamNonBlocking) != hipSuccess ||
                      hipEventCreateWithFlags(&t->ev_fork, hipEventDisableTiming) != hipSuccess ||
                      hipEventCreateWithFlags(&t->ev_join, hipEventDisableTiming) != hipSuccess ||
                      hipEventCreateWithFlags(&t->ev_band, hipEventDisableTiming) != hipSuccess;
            if (bad && !lsn::has_error()) lsn::set_error("lsnTickCreate: %s", hipGetErrorString(hipGetLastError()));
        }
        if (bad) {
            tick_destroy(t);
            return nullptr;
        }
        return t;
    });
}

extern "C" long long lsnTickCapacity(const LsnTick *t) { return t ? t->cap : 0; }
extern "C" long long lsnTickTriangleCapacity(const LsnTick *t) { return t ? t->tri_cap : 0; }
extern "C" int lsnTickParts(const LsnTick *t) { return t ? t->parts : 0; }

extern "C" int lsnTickSetParams(LsnTick *t, const float *intr, const float *wt, const float *bounds6, void *stream)
{
    return lsn::guarded("lsnTickSetParams", -1, [&]() {
        lsn::clear_error();
        if (!t || !intr || !wt || !bounds6) {
            lsn::set_error("lsnTickSetParams: null argument");
            return -1;
        }
        std::lock_guard<std::mutex> g(t->mu);
        t->intr.assign(intr, intr + 7 * (size_t)t->n_maps);
        for (int k = 0; k < t->parts; k++)
            if (lsnFusionSetParams(t->plan[k], intr, wt, bounds6, stream)) return -1;
        return 0;
    });
}

extern "C" int lsnTickSetFlyingPixels(LsnTick *t, int neighbourhood, int threshold)
{
    return lsn::guarded("lsnTickSetFlyingPixels", -1, [&]() {
        lsn::clear_error();
        if (!t) {
            lsn::set_error("lsnTickSetFlyingPixels: null argument");
            return -1;
        }
        std::lock_guard<std::mutex> g(t->mu);
        t->fp_neighbourhood = neighbourhood;
        t->fp_threshold = threshold;
        return 0;
    });
}

extern "C" int lsnTickSetDepthSmooth(LsnTick *t, int radius, float sigma_s, float sigma_r)
{
    return lsn::guarded("lsnTickSetDepthSmooth", -1, [&]() {
        lsn::clear_error();
        if (!t) {
            lsn::set_error("lsnTickSetDepthSmooth: null argument");
            return -1;
        }
        lsn::DepthSmoothTables tab;
        if (radius >= 1 && lsn::depth_smooth_gaussian(radius, sigma_s, sigma_r, tab)) return -1;   // refused: the previous setting stays
        std::lock_guard<std::mutex> g(t->mu);
        for (int k = 0; k < t->parts; k++)
            if (lsn::set_depth_smooth(t->plan[k], "lsnTickSetDepthSmooth", radius, tab.spatial, tab.range, tab.n_range)) return -1;
        t->ds_radius = radius >= 1 ? radius : 0;
        return 0;
    });
}

extern "C" int lsnTickSetTemporal(LsnTick *t, int alpha_q, int delta, int persist)
{
    return lsn::guarded("lsnTickSetTemporal", -1, [&]() {
        lsn::clear_error();
        if (!t) {
            lsn::set_error("lsnTickSetTemporal: null argument");
            return -1;
        }
        if (lsn::temporal_setting_ok("lsnTickSetTemporal", alpha_q, delta, persist)) return -1;   // refused: the previous setting stays
        std::lock_guard<std::mutex> g(t->mu);
        t->tp_setting = alpha_q >= 1 ? lsn::TemporalSetting{alpha_q, delta, persist} : lsn::TemporalSetting{};
        return 0;
    });
}

extern "C" int lsnTickTemporalReset(LsnTick *t, void *stream)
{
    return lsn::guarded("lsnTickTemporalReset", -1, [&]() {
        lsn::clear_error();
        if (!t) {
            lsn::set_error("lsnTickTemporalReset: null argument");
            return -1;
        }
        std::lock_guard<std::mutex> g(t->mu);
        LSN_HIP(hipSetDevice(t->device));
        return t->tp.reset((size_t)t->cap, lsn::as_stream(stream));
    });
}

extern "C" int lsnTickSetBackground(LsnTick *t, int margin, int rel_q, int min_pixels)
{
    return lsn::guarded("lsnTickSetBackground", -1, [&]() {
        lsn::clear_error();
        if (!t) {
            lsn::set_error("lsnTickSetBackground: null argument");
            return -1;
        }
        if (lsn::background_setting_ok("lsnTickSetBackground", margin, rel_q, min_pixels)) return -1;   // refused: the previous setting stays
        std::lock_guard<std::mutex> g(t->mu);
        t->bg_setting = margin >= 1 ? lsn::BackgroundSetting{margin, rel_q, min_pixels} : lsn::BackgroundSetting{};
        return 0;
    });
}

// The temporal pass of a run or a learning call (t->mu held): the whole batch once, in tick order, on the caller's stream, plan 0's frame and
// tile tables serving all ticks and one history seeing them in order; d_depth_in becomes its output.  Off: nothing.
static int tick_temporal(LsnTick *t, const void *&d_depth_in, hipStream_t s)
{
    if (!t->tp_setting.on()) return 0;
    if (t->d_temporal.reserve(2 * (size_t)t->cap * t->n_ticks + 16) || t->tp.reserve((size_t)t->cap, s) || t->tp.hand_over(s)) return -1;
    for (int k = 0; k < t->parts; k++)
        if (t->plan[k]->rd.wait_for_chain(s)) return -1;
    if (lsn::temporal(t->plan[0], t->tp_setting, d_depth_in, t->d_temporal.p, t->tp.state.as<unsigned int>(), t->tp.counts, t->n_ticks, s)) return -1;
    d_depth_in = t->d_temporal.p;
    return 0;
}

extern "C" int lsnTickBackgroundLearn(LsnTick *t, const void *d_depth_in, void *stream)
{
    return lsn::guarded("lsnTickBackgroundLearn", -1, [&]() {
        lsn::clear_error();
        if (!t || !d_depth_in) {
            lsn::set_error("lsnTickBackgroundLearn: null argument");
            return -1;
        }
        std::lock_guard<std::mutex> g(t->mu);
        LSN_HIP(hipSetDevice(t->device));
        hipStream_t s = lsn::as_stream(stream);
        // the stage learns what it will classify: the temporal stage's output when that is set
        if (tick_temporal(t, d_depth_in, s) || t->bg.reserve((size_t)t->cap, s) || t->bg.hand_over(s)) return -1;
        return lsn::background_learn(t->plan[0], d_depth_in, t->bg.state.as<unsigned short>(), t->n_ticks, s);
    });
}

extern "C" int lsnTickBackgroundReset(LsnTick *t, void *stream)
{
    return lsn::guarded("lsnTickBackgroundReset", -1, [&]() {
        lsn::clear_error();
        if (!t) {
            lsn::set_error("lsnTickBackgroundReset: null argument");
            return -1;
        }
        std::lock_guard<std::mutex> g(t->mu);
        LSN_HIP(hipSetDevice(t->device));
        return t->bg.reset((size_t)t->cap, lsn::as_stream(stream));
    });
}

extern "C" int lsnTickRun(LsnTick *t, const void *d_depth_in, const void *d_colors_in, void *d_depth_corr, void *d_colors_corr, void *d_vertices,
                          int *d_offsets, void *d_triangles, int *d_tri_offsets, void *stream)
{
    return lsn::guarded("lsnTickRun", -1, [&]() {
        lsn::clear_error();
        if (!t || !d_depth_in || !d_colors_in || !d_depth_corr || !d_colors_corr || !d_vertices || !d_offsets || !d_triangles || !d_tri_offsets) {
            lsn::set_error("lsnTickRun: null argument");
            return -1;
        }
        std::lock_guard<std::mutex> g(t->mu);
        if (t->intr.empty()) {   // (under the lock: lsnTickSetParams assigns the vector under it)
            lsn::set_error("lsnTickRun: lsnTickSetParams has not been called");
            return -1;
        }
        LSN_HIP(hipSetDevice(t->device));
        hipStream_t s = lsn::as_stream(stream);
        const bool filter = lsn::flying_on(t->fp_neighbourhood);
        if (filter && t->d_filtered.reserve(2 * (size_t)t->cap * t->n_ticks + 16)) return -1;
        const bool smooth = lsn::smooth_on(t->ds_radius);
        if (smooth && t->d_smoothed.reserve(2 * (size_t)t->cap * t->n_ticks + 16)) return -1;
        // the temporal filter runs once over the whole batch, in tick order, on the caller's stream in front of the fork: the halves share the
        // rig, so plan 0's frame and tile tables serve all ticks, and one history sees them in order.  The halves then start from d_temporal
        // at their own offsets.  (The scratch follows d_filtered's rule below: a run on another stream waits for the previous run's chains.)
        if (tick_temporal(t, d_depth_in, s)) return -1;
        // background subtraction follows right behind it under the same rules, from the temporal pass's output into scratch of its own
        if (t->bg_setting.on()) {
            if (t->d_background.reserve(2 * (size_t)t->cap * t->n_ticks + 16) || t->bg.reserve((size_t)t->cap, s) || t->bg.hand_over(s)) return -1;
            for (int k = 0; k < t->parts; k++)
                if (t->plan[k]->rd.wait_for_chain(s)) return -1;
            if (lsn::background(t->plan[0], t->bg_setting, d_depth_in, t->d_background.p, t->bg.state.as<unsigned short>(), t->bg.counts, t->bg_blob, t->n_ticks, s)) return -1;
            d_depth_in = t->d_background.p;
        }
        // part k's slices of the caller's arrays: [tick][pixels], [tick][pixels][3], [tick][capacity] vertices, [tick][n_maps + 1], ...
        auto part = [&](int k, hipStream_t st) -> int {
            const size_t t0 = (size_t)t->first[k];
            const size_t px = (size_t)t->cap, nm = (size_t)t->n_maps + 1;
            const unsigned char *din = static_cast<const unsigned char *>(d_depth_in) + 2 * px * t0, *cin = static_cast<const unsigned char *>(d_colors_in) + 3 * px * t0;
            unsigned char *dco = static_cast<unsigned char *>(d_depth_corr) + 2 * px * t0, *cco = static_cast<unsigned char *>(d_colors_corr) + 3 * px * t0;
            if (filter) {   // filter -> correction: the filtered maps go through the tick's scratch, the caller's input stays as it is
                unsigned char *dfl = t->d_filtered.as<unsigned char>() + 2 * px * t0;
                // the scratch is shared by all runs of the tick object: a run on another stream than the previous one's waits until that
                // run's correction has read it (the event radial.hip records behind every chain)
                if (t->plan[k]->rd.wait_for_chain(st)) return -1;
                if (lsn::flying_pixels(t->plan[k], t->fp_neighbourhood, t->fp_threshold, din, dfl, st)) return -1;
                din = dfl;
            }
            if (smooth) {   // (filter ->) smoothing -> correction, through scratch of its own under the same rule
                unsigned char *dsm = t->d_smoothed.as<unsigned char>() + 2 * px * t0;
                if (t->plan[k]->rd.wait_for_chain(st)) return -1;
                if (lsn::depth_smooth(t->plan[k], din, dsm, st)) return -1;
                din = dsm;
            }
            if (lsnFusionRadialCorrectTo(t->plan[k], t->intr.data(), din, cin, dco, cco, st)) return -1;
            return lsnFusionRunMesh(t->plan[k], dco, cco, static_cast<unsigned char *>(d_vertices) + 16 * px * t0, d_offsets + nm * t0,
                                    static_cast<unsigned char *>(d_triangles) + 12 * (size_t)t->tri_cap * t0, d_tri_offsets + nm * t0, st);
        };
        if (t->parts == 1) return part(0, s);
        // fork: the side stream starts where the caller's stream stands -- and only when the first half's band kernel is through (staggered): two
        // halves that start together march in step (band beside band, closing beside closing) and gain nothing; half a stage apart, one half's
        // closing rounds run beside the other half's band kernel, then beside its count / write / triangle passes.  join: the caller's stream
        // continues behind both halves.
        LSN_HIP(hipEventRecord(t->ev_fork, s));
        LSN_HIP(hipStreamWaitEvent(t->side, t->ev_fork, 0));
        t->plan[0]->rd.after_band = t->ev_band;
        const int rc_a = part(0, s);
        t->plan[0]->rd.after_band = nullptr;
        char err_a[lsn::kErrorLen];
        snprintf(err_a, sizeof(err_a), "%s", lsn::error_buffer());   // (every export clears the channel on entry: the second half's calls would wipe the first half's text)
        if (hipStreamWaitEvent(t->side, t->ev_band, 0) != hipSuccess) (void)hipGetLastError();   // (a closing route without a band kernel records nothing new: no wait, the halves start together)
        const int rc_b = part(1, t->side);
        if (rc_a) lsn::set_error("%s", err_a);
        // (the join is enqueued whatever happened: nothing of a failed half may still be running unobserved when the caller's stream goes on)
        if (hipEventRecord(t->ev_join, t->side) == hipSuccess) (void)hipStreamWaitEvent(s, t->ev_join, 0);
        else (void)hipGetLastError();
        return rc_a || rc_b ? -1 : 0;
    });
}
