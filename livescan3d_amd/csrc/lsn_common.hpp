// lsn_common.hpp -- shared host-side plumbing of libNativeUtils.so (error channel, HIP checks, small RAII).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <exception>
#include <new>
#include <string>
#include <vector>

#include "../../include/NativeUtils.h"

namespace lsn {

// Thread-local error text behind lsnGetLastError().  The reference's exports have no error channel at all
// (void / constant returns, src/NativeUtils/depthprocessing.cpp:1631,1715; icp.cpp:176); nothing may throw
// across the C-ABI, so failures end up here.
constexpr int kErrorLen = 1024;
char *error_buffer() noexcept;                         // fixed thread-local storage: setting an error never allocates
void set_error(const char *fmt, ...) noexcept;
inline void clear_error() noexcept { error_buffer()[0] = 0; }
inline bool has_error() noexcept { return error_buffer()[0] != 0; }
long test_fault_points(int kind);                      // how many fault points of that kind the process has passed
void test_fault_point(int kind);                       // 0 = guarded entry, 1 = allocation; throws std::bad_alloc when a test asks for it

// Every extern "C" entry point runs its body through this: no exception may cross the C-ABI into a P/Invoke frame
// (SURVEY 8b "exceptions must not escape"; the reference itself lets nanoflann throw, include/nanoflann.h:904).
// R is the type of `fail`, what the export returns when its body threw; a body whose returns are not all of that type names it (-> R).
template <class R, class F>
inline R guarded(const char *name, R fail, F &&body) noexcept
{
    try {
        test_fault_point(0);
        return body();
    } catch (const std::exception &e) {
        set_error("%s: %s", name, e.what());
    } catch (...) {
        set_error("%s: unknown exception", name);
    }
    return fail;
}
// The same for an export that returns nothing.
template <class F>
inline void guarded_void(const char *name, F &&body) noexcept
{
    (void)guarded(name, false, [&]() {
        body();
        return true;
    });
}

#define LSN_HIP(expr)                                                                                    \
    do {                                                                                                 \
        hipError_t _e = (expr);                                                                          \
        if (_e != hipSuccess) {                                                                          \
            lsn::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__);   \
            return -1;                                                                                   \
        }                                                                                                \
    } while (0)

#define LSN_HIP_NULL(expr)                                                                               \
    do {                                                                                                 \
        hipError_t _e = (expr);                                                                          \
        if (_e != hipSuccess) {                                                                          \
            lsn::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__);   \
            return nullptr;                                                                              \
        }                                                                                                \
    } while (0)

// Device buffer that frees itself; not copyable.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    // grow-only
    int reserve(size_t n) {
        if (n <= bytes) return 0;
        test_fault_point(1);
        release();
        LSN_HIP(hipMalloc(&p, n));
        bytes = n;
        return 0;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

inline hipStream_t as_stream(void *s) { return static_cast<hipStream_t>(s); }

// What a stage keeps that carries per-pixel state from call to call (the temporal filter's history, temporal.hip: 4 bytes a pixel, no pad;
// background subtraction's model, background.hip: 2 bytes a pixel and 16 behind them): the state of ONE tick's pixels, the count words of
// the last call, and the stream that touched the state last.  One rule for every owner (a plan, a tick object, a lane of the host
// exports): whatever touches the state first calls hand_over(s), which waits for the previous stream's work when that is another one and
// records `s`.  The owner holds the lock that guards the record and has made its device current.
struct StageState {
    const size_t px_bytes, pad;
    DevBuf state, counts;
    hipStream_t stream = nullptr;    // the stream that touched the state last ...
    bool busy = false;               // ... once something has
    StageState(size_t bytes_per_pixel, size_t tail_pad) : px_bytes(bytes_per_pixel), pad(tail_pad) {}
    // room for `pixels`, all zero ("no history" / "nothing learned") on first use and when it grows (grow-only: a larger one starts empty too)
    int reserve(size_t pixels, hipStream_t s)
    {
        if (px_bytes * pixels + pad <= state.bytes && state.p) return 0;
        if (state.reserve(px_bytes * pixels + pad)) return -1;
        LSN_HIP(hipMemsetAsync(state.p, 0, state.bytes, s));
        LSN_HIP(hipStreamSynchronize(s));   // (once per buffer: whichever stream comes next finds the zeros)
        return 0;
    }
    int hand_over(hipStream_t s)
    {
        if (busy && stream != s) LSN_HIP(hipStreamSynchronize(stream));
        stream = s;
        busy = true;
        return 0;
    }
    // back to all zero, queued on `s`; nothing reserved yet: nothing to do
    int reset(size_t pixels, hipStream_t s)
    {
        if (!state.p) return 0;
        if (hand_over(s)) return -1;
        LSN_HIP(hipMemsetAsync(state.p, 0, px_bytes * pixels, s));
        return 0;
    }
    // the state of `pixels` pixels into / from a host array, complete on return; nothing reserved yet reads as zeros, a write reserves
    int read(void *host, size_t pixels, hipStream_t s)
    {
        if (!state.p) {
            memset(host, 0, px_bytes * pixels);
            return 0;
        }
        if (hand_over(s)) return -1;
        LSN_HIP(hipMemcpyAsync(host, state.p, px_bytes * pixels, hipMemcpyDeviceToHost, s));
        LSN_HIP(hipStreamSynchronize(s));
        return 0;
    }
    int write(const void *host, size_t pixels, hipStream_t s)
    {
        if (reserve(pixels, s) || hand_over(s)) return -1;
        LSN_HIP(hipMemcpyAsync(state.p, host, px_bytes * pixels, hipMemcpyHostToDevice, s));
        LSN_HIP(hipStreamSynchronize(s));   // (the caller's array is free again on return)
        return 0;
    }
};

// lsnFusionRun on a stream, for the library's own flows (takes the plan's mutex; leaves the error text as it is unless it fails).
int run_vertices(LsnFusion *p, const void *d_depth, const void *d_colors, void *d_vertices, int *d_offsets, hipStream_t s);
// The same with the mutex already held; with_pixmap also fills the pixel -> vertex map the triangulation reads, which the caller has
// reserved (reserve_pixmap, fusion_shared.hpp).  Picks the launch form from the plan's mode (fusion.hip run_form).
int run_locked(LsnFusion *p, const void *d_depth, const void *d_colors, void *d_vertices, int *d_offsets, hipStream_t s, bool with_pixmap);
// lsnFusionRunMesh on a stream (takes the mutex once for the vertex and the triangle passes).
int run_mesh(LsnFusion *p, const void *d_depth, const void *d_colors, void *d_vertices, int *d_offsets, void *d_triangles, int *d_tri_offsets,
             hipStream_t s);

// One launch, single pass, over frames [f0, f1) of a one-tick plan (fusion.hip); and the triangle passes alone over the whole tick, for
// a pixel -> vertex map that run_frames(with_pixmap) launches have filled (mesh.hip).  tri_mirror: optional pinned, device-visible copy of
// the table, stored by the scan kernel itself; tri_counted: optional event recorded behind the scan (the counts are in the mirror), before
// the triangle write pass; host_out: d_triangles is pinned host memory (the write pass's HOST form).
int run_frames(LsnFusion *p, const void *d_depth, const void *d_colors, void *d_vertices, int *d_offsets, int f0, int f1, bool first_of_tick,
               bool with_pixmap, int *offsets_mirror, int *group_end_mirror, bool host_out, hipStream_t s);
int run_triangles(LsnFusion *p, const void *d_depth, void *d_triangles, int *d_tri_offsets, int *tri_mirror, bool host_out, hipStream_t s,
                  hipEvent_t tri_counted = nullptr);

// The two halves of the two-pass form of a one-tick plan (fusion.hip) and of its triangle passes (mesh.hip), for a caller that places
// the tick's vertices / triangles behind somebody else's: host_flows.hip's calls sharded over devices.  index_base: added to every vertex index a
// triangle names (formMesh's rebase, depthprocessing.cpp:1614-1626, across devices).
int run_count(LsnFusion *p, const void *d_depth, const void *d_colors, int *d_offsets, int *offsets_mirror, hipEvent_t counted, hipStream_t s);
int run_write(LsnFusion *p, const void *d_depth, const void *d_colors, void *vertices, int *d_offsets, bool with_pixmap, bool host_out, hipStream_t s);
int run_triangles_count(LsnFusion *p, const void *d_depth, int *d_tri_offsets, int *tri_mirror, hipEvent_t tri_counted, hipStream_t s);
int run_triangles_write(LsnFusion *p, const void *d_depth, void *d_triangles, int index_base, bool host_out, hipStream_t s);

// lsnFusionColorTransfer on a stream (color.hip): colour transfer in place on the cloud lsnFusionRun* wrote from d_depth.
int color_transfer(LsnFusion *p, const void *d_depth, void *d_vertices, const int *d_offsets, hipStream_t s);
// lsnFusionColorBlend on a stream (color_blend.hip): the confidence-weighted blend across views in place on the same cloud, behind the
// colour transfer when both run.  Takes the plan's mutex.
int color_blend(LsnFusion *p, int depth_tol, int min_confidence, const void *d_depth, void *d_vertices, const int *d_offsets, hipStream_t s);
// lsnFusionOverlayMerge on a stream (merge.hip): rewrites the triangles of the cloud lsnFusionRun* wrote from d_depth.
int overlay_merge(LsnFusion *p, const void *d_depth, const void *d_vertices, const int *d_offsets, void *d_triangles, int *d_tri_offsets,
                  hipStream_t s);
// lsnFusionOutlierFilter on a stream (outlier.hip): d_depth with depth 0 at the pixels of removed vertices into d_depth_out.
int outlier_filter(LsnFusion *p, int k, float max_dist, const void *d_depth, const void *d_vertices, const int *d_offsets, void *d_depth_out,
                   hipStream_t s);

// lsnFusionFlyingPixels on a stream (flying.hip): the flying-pixel filter on every map of the plan, d_depth_in into d_depth_out (out of
// place; neighbourhood <= 0 copies).  Takes the plan's mutex.
int flying_pixels(LsnFusion *p, int neighbourhood, int threshold, const void *d_depth_in, void *d_depth_out, hipStream_t s);

// Depth smoothing (depth_smooth.hip).  One setting as the process-wide switch and the tick hold it: the Gaussian tables of
// lsnDepthSmoothGaussian for (radius, sigma_s, sigma_r).  set_depth_smooth is lsnFusionSetDepthSmooth under the name `who` (a setting the
// plan already has costs nothing), depth_smooth is lsnFusionDepthSmooth on a stream; both take the plan's mutex.
struct DepthSmoothTables {
    int radius = 0, n_range = 0;
    unsigned short spatial[49] = {};
    unsigned short range[1024] = {};
};
int set_depth_smooth(LsnFusion *p, const char *who, int radius, const unsigned short *spatial, const unsigned short *range, int n_range);
int depth_smooth(LsnFusion *p, const void *d_depth_in, void *d_depth_out, hipStream_t s);
// The tables of (radius, sigma_s, sigma_r) into `t`; -1 with lsnDepthSmoothGaussian's message where it refuses them.
int depth_smooth_gaussian(int radius, float sigma_s, float sigma_r, DepthSmoothTables &t);

// The temporal depth filter (temporal.hip), the stage in front of the flying-pixel filter.  One setting as the plans, the tick and the
// process-wide switch hold it (alpha_q <= 0: off).  temporal is lsnFusionTemporal with an explicit history and tick count, on a stream: the
// history belongs to whoever sees the same rig tick after tick (a plan, a tick object, a lane of the host exports), not to the plan whose
// frame and tile tables the pass reads.  It takes the plan's mutex.
struct TemporalSetting {
    int alpha_q = 0, delta = 0, persist = 0;
    bool on() const { return alpha_q >= 1; }
};
int temporal_setting_ok(const char *who, int alpha_q, int delta, int persist);
int temporal_state_ok(const char *who, const unsigned int *h_state, size_t pixels);
int temporal(LsnFusion *p, const TemporalSetting &ts, const void *d_depth_in, void *d_depth_out, unsigned int *d_state, DevBuf &counts, int n_ticks,
             hipStream_t s);

// Background subtraction (background.hip), the stage between the temporal filter and the flying-pixel filter.  One setting as the plans, the
// tick and the process-wide switch hold it (margin <= 0: off; min_pixels <= 1: no blob pass).  background_learn and background are
// lsnFusionBackgroundLearn and lsnFusionBackground with an explicit model and tick count, on a stream: the model belongs to whoever sees the
// same rig tick after tick (a plan, a tick object, a lane of the host exports), not to the plan whose frame and tile tables the passes read.
// Both take the plan's mutex.
struct BackgroundSetting {
    int margin = 0, rel_q = 0, min_pixels = 0;
    bool on() const { return margin >= 1; }
    bool blobs() const { return min_pixels >= 2; }
};
int background_setting_ok(const char *who, int margin, int rel_q, int min_pixels);
int background_learn(LsnFusion *p, const void *d_depth, unsigned short *d_model, int n_ticks, hipStream_t s);
int background(LsnFusion *p, const BackgroundSetting &bs, const void *d_depth_in, void *d_depth_out, const unsigned short *d_model, DevBuf &counts,
               DevBuf &blob, int n_ticks, hipStream_t s);

// What the two stages' calls open with (the caller holds the plan's mutex): the plan's device, the rule "in place or on disjoint buffers"
// with the stage's export `who` in the message, and a stage that is off, which copies.  1: the stage runs; 0: off, the call is done; -1: refused.
int stage_preamble(LsnFusion *p, const char *who, bool on, const void *d_depth_in, void *d_depth_out, int n_ticks, hipStream_t s);
// The count words of tick `tick`, `n_fields` plain words per 128 x 16 tile as a stage's kernels left them in `counts`, summed per frame of
// the plan into per_frame[n_maps][n_fields] (p->mu held or the plan otherwise quiet).
int stage_counts(LsnFusion *p, const DevBuf &counts, int tick, int n_fields, int *per_frame);

// What "on" means for the two stages behind it, for everybody who chains them in front of the correction (the host exports' DepthStages,
// host_ctx.hpp; the tick object, tick.hip): a neighbourhood / a radius of at least one pixel; 0 and below mean off.  The temporal filter's is
// TemporalSetting::on().
inline bool flying_on(int neighbourhood) { return neighbourhood >= 1; }
inline bool smooth_on(int radius) { return radius >= 1; }

// A batch of meshes in lsnFusionRunMesh's layout, as the three stages on the merged mesh read it (render.hip, simplify.hip, normals.hip;
// what they share is mesh_batch.hip's).  The stages' device structs embed it; it is built from a plan (plan_batch, mesh_batch.hip) or
// from a lane's last mesh (LastMesh::batch, abi.hip).
struct MeshBatch {
    const uint4 *verts;              // [n_ticks][tick_vert]
    const int *voff;                 // [n_ticks][n + 1]
    const int *tri;                  // [n_ticks][tick_tri][3], null: points only
    const int *toff;                 // [n_ticks][n + 1]
    long long tick_vert, tick_tri;   // vertices / triangles per tick: the strides, and what a tick's counts are clipped to
    int n_ticks, n;                  // ticks; sensors per offset row
};

// The counters behind a stage's diagnostics: four ints per slot (a tick; a (tick, view) of the render stage) and the shape of the last
// call, which a call forgets when it begins and remembers when everything is queued -- a failed call leaves "nothing yet".
struct StageCounters {
    DevBuf buf;
    int ticks = 0, per_tick = 0;     // the shape of the last call (0: none yet)
    int begin(size_t reserve_slots, size_t slots, hipStream_t s);   // reserve, clear `slots` on `s`, forget the last shape
    void finish(int n_ticks, int n_per_tick = 1) { ticks = n_ticks; per_tick = n_per_tick; }
    // slot (tick, sub) of the last call into c; synchronises `s`.  No call yet: "who: nothing_yet"; no such slot: what out_of_range() says.
    template <class F>
    int read(const char *who, const char *nothing_yet, int tick, int sub, int c[4], hipStream_t s, F &&out_of_range) const;
};

// The render stage (render.hip): what one renderer keeps between calls -- the per-pixel keys [n_ticks][n_views][w * h] u64, one view's
// projected vertices [n_ticks][vertices per tick] and work list [n_ticks][triangles per tick] (the views of a call take turns on them;
// mesh mode only), the counters behind lsnFusionRenderDiagnostics.  Reserved by the first call, grown by a call that needs more.
struct RenderScratch {
    DevBuf key, proj, list;
    StageCounters cnt;                // per (tick, view)
    bool keys_clean = false;          // every key is "none": the resolve passes of the last call were all queued
};
// Each stage on a batch, and the counters of one slot of the last call with its scratch (synchronises `s`).  The caller holds the lock
// that guards the scratch and has made its device current; `who` names the export in messages.
int render_views(RenderScratch &rs, const char *who, const MeshBatch &m, int n_views, const float *intr_params, const float *wtransform_params,
                 int width, int height, void *d_depth_out, void *d_colors_out, hipStream_t s);
int render_counts(RenderScratch &rs, const char *who, int tick, int view, int *n_drawn, int *n_large, int *n_pixels, hipStream_t s);

// Mesh level of detail (simplify.hip): what one simplifier keeps between calls -- the hash table [n_ticks][slots] of u64 keys and, behind
// them, u32 values (slots: the power of two at or above 2 x the vertices per tick), representative / remap and output index per vertex,
// the per-256 counts of kept vertices and triangles, the counters behind lsnFusionSimplifyDiagnostics.  Reserved by the first call, grown
// by a call that needs more; cell <= 0 never reserves the table.
struct SimplifyScratch {
    DevBuf table, rep, newidx, tiles;
    StageCounters cnt;                // per tick
};
int simplify(SimplifyScratch &ss, const char *who, const MeshBatch &m, float cell, void *d_vertices_out, int *d_offsets_out, void *d_triangles_out,
             int *d_tri_offsets_out, int *d_remap_out, hipStream_t s);
int simplify_counts(SimplifyScratch &ss, const char *who, int tick, int *n_cells, int *n_unclustered, int *n_dropped_triangles, hipStream_t s);

// The fragment filter (fragments.hip): what one filter keeps between calls -- the parent / label array, the sizes (at the label's index)
// and the output index, each [n_ticks][vertices per tick] ints, the per-256 counts of kept vertices and triangles, the counters behind
// lsnFusionFragmentsDiagnostics.  Reserved by the first call, grown by a call that needs more; min_vertices <= 1 reserves neither the
// parents nor the sizes.
struct FragmentsScratch {
    DevBuf parent, size, newidx, tiles;
    StageCounters cnt;                // per tick
};
// d_remap_out, d_labels_out: nullable; a batch without triangles is refused.
int fragments(FragmentsScratch &fs, const char *who, const MeshBatch &m, int min_vertices, void *d_vertices_out, int *d_offsets_out,
              void *d_triangles_out, int *d_tri_offsets_out, int *d_remap_out, int *d_labels_out, hipStream_t s);
int fragments_counts(FragmentsScratch &fs, const char *who, int tick, int *n_components, int *n_removed_components, int *n_removed_vertices,
                     int *n_dropped_triangles, hipStream_t s);

// Vertex normals (normals.hip): what one stage keeps between calls -- the sums, three planes [n_ticks][3][vertices per tick] of i64 (24 B
// per vertex; the counted vertices are cleared by every call), and the counters behind lsnFusionNormalsDiagnostics.  Reserved by the
// first call, grown by a call that needs more.
struct NormalsScratch {
    DevBuf acc;
    StageCounters cnt;                // per tick
};
// d_normals_out: tick_vert x 3 floats per tick; prof (nullable): the plan whose lsnFusionProfile brackets the face pass.
int normals(NormalsScratch &ns, const char *who, const MeshBatch &m, void *d_normals_out, LsnFusion *prof, hipStream_t s);
int normals_counts(NormalsScratch &ns, const char *who, int tick, int *n_used, int *n_skipped, int *n_zero_normals, hipStream_t s);

// Mesh smoothing (smooth.hip): what one stage keeps between calls -- the sums, three planes [n_ticks][3][vertices per tick] of i64, the
// counts N (u32), the open-vertex hashes H (u64) and the pinned flags (a byte), each [n_ticks][vertices per tick], the vertex buffer the
// passes take turns on with the output (16 B per vertex; a call of one pass needs none), and the counters behind
// lsnFusionSmoothDiagnostics: 53 B per vertex.  Reserved by the first call, grown by a call that needs more; the counted vertices are
// cleared by every call.
struct SmoothScratch {
    DevBuf acc, num, hash, flag, verts;
    StageCounters cnt;                // per tick
};
// d_vertices_out: tick_vert 16-byte records per tick; refuses iterations outside [1, 64], lambda outside (0, 1], mu outside [-1, 0].
int smooth(SmoothScratch &ss, const char *who, const MeshBatch &m, int iterations, float lambda, float mu, int pin_boundary, void *d_vertices_out,
           hipStream_t s);
int smooth_counts(SmoothScratch &ss, const char *who, int tick, int *n_used, int *n_skipped, int *n_pinned, int *n_isolated, hipStream_t s);

// The radial correction (radial.hip): what one plan keeps between calls -- the sensors' parameters, the warp tables of the current
// calibration ([pixels per tick][4] candidates and their compact form, one dword per destination) with the intrinsics they were built for,
// the scratch maps and the winner array of the routes that warp through memory, and the hole closing's band list, hole bitmap, two
// work lists (used in turn) and their counters.  All of it is shared by every call on the plan: calls on one stream are ordered by
// the stream, and an event recorded behind every chain orders a call on another stream behind the chain before it.  Reserved by the
// first call that needs each piece, grown by a call that needs more.
struct RadialScratch {
    DevBuf params, cand, ctab;
    std::vector<float> intr;          // the intrinsics `cand` / `ctab` were built for
    bool tables_valid = false, overflow = false;   // overflow: a destination has more than four sources, the calls take the atomicMax warp
    DevBuf winner, map_copy, colors_copy;
    DevBuf bands, holes, work, work2, work_cnt;
    int band_rows = 0, bands_per_tick = 0;         // what `bands` was built for
    bool work_cnt_clean = false;      // the closing chain of the last call was enqueued to its end (it leaves work_cnt zeroed)
    bool band_attr_set = false;
    hipEvent_t after_band = nullptr;  // not owned: recorded behind the band kernel of a call (set by lsnTickRun around its calls)
    hipStream_t stream = nullptr;     // the stream of the last call ...
    hipEvent_t done = nullptr;        // ... and the end of its chain
    bool chain_open = false;          // `done` has been recorded at least once
    // Work on `s` that clears, refills or reads the scratch first waits for the previous chain's end if that was enqueued on another stream.
    int wait_for_chain(hipStream_t s)
    {
        if (chain_open && stream != s) LSN_HIP(hipStreamWaitEvent(s, done, 0));
        return 0;
    }
    // `s` now holds the last chain (also one that failed half-way: whatever it did enqueue is what the next stream has to wait for).
    void chain_ends_on(hipStream_t s)
    {
        if (hipEventRecord(done, s) == hipSuccess) chain_open = true;
        else (void)hipGetLastError();
        stream = s;
    }
    void destroy_event() { if (done) (void)hipEventDestroy(done); }   // lsnFusionDestroy, with the plan's device current
};

// The refine pass (refine.hip) on ONE tick's merged cloud, resident on `device` and final: vertices -> packed points -> Gauss-Seidel loop.
// offsets: the tick's n_sensors + 1 row on the HOST; Rt: n_sensors x 12 floats, receives {Rs[i][9], Ts[i][3]}; h_clouds (host) / d_clouds
// (device), both nullable, receive the refined points.  d_normals (device, nullable): the tick's vertex normals, 3 floats per vertex at the
// vertex's own index and final -- the pass then minimises the point-to-plane residual (lsnRefineVerticesPlane).  Complete on return.
// refine_compose: the pose composition of the reference's refine worker for those poses (world and camera pairs nullable), and the poses
// themselves into Rs_out / Ts_out (nullable).
int refine_cloud(const char *who, int device, int n_sensors, const void *d_vertices, const int *offsets, int n_refine_iters, int n_icp_iters,
                 float *Rt, float *h_clouds, float *d_clouds, const float *d_normals = nullptr);
void refine_compose(int n, const float *Rt, float *world_R, float *world_t, float *camera_R, float *camera_t, float *Rs_out, float *Ts_out);

// The survivor exchange's two ends with the back-to-back stream layout (exchange.hip; see their definitions).
int pack_survivors(LsnFusion *p, const void *d_depth, const void *d_colors, void *d_mask, void *d_depth_c, void *d_rgb_c, int *d_tile_prefix,
                   int *d_offsets, int *d_tick_base, void *stream);
// The ticks one reconstruct call covers (lsnShardStep's pipelined form cuts a step into chunks; everybody else takes the default, all of
// them): [tick0, tick0 + n_ticks), n_ticks <= 0 = up to the plan's last; only a step's first chunk fills the tick bases.
struct ReconChunk {
    int tick0 = 0, n_ticks = 0;
    bool fill_tick_base = true;
};
int reconstruct(LsnFusion *all, int n_shards, int maps_per_shard, const void *d_masks, const void *d_depth_c, const void *d_rgb_c, long long slab,
                const int *d_tile_prefix, const int *d_shard_offsets, void *d_merged, int *d_merged_offsets, int *d_tick_base, void *stream,
                ReconChunk chunk = ReconChunk());

// lsnMergeShards, optionally for shards laid out [n_ticks][n_shards][shard_cap] (per-tick all-gathers).
int merge_shards(int device, int n_shards, int n_ticks, int maps_per_shard, const void *d_shards, long long shard_cap, const int *d_shard_offsets,
                 void *d_merged, long long merged_cap, int *d_merged_offsets, bool tick_major, void *stream);

}  // namespace lsn
