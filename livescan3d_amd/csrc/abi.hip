// abi.hip -- the reference's C-ABI exports (include/NativeUtils.h part 1) on top of the device-resident API.
//
// LiveScanServer hands over host arrays (pinned managed arrays / AllocHGlobal blocks, KinectServer.cs:354-374,
// MainWindowForm.cs:364-370) and reads host memory back (Marshal.Copy, KinectServer.cs:383), so these entry points
// add the H2D / D2H hops around the same kernels bench.py drives directly on HBM-resident data.  How a call runs -- the
// upload schedule, kernels storing into the pinned mesh blocks, the copy-engine flow, the call sharded over devices -- is
// host_flows.hip; the context it runs on (lanes, pinned pool, devices) and the records a call carries host_ctx.hpp.  This file: argument
// checks, locks, the exception trampoline, the process-wide switches of the exports' opt-in stages (the outlier filter, the overlay merge, the colour blend;
// the temporal filter, background subtraction, the flying-pixel filter and depth smoothing in front of the radial correction, which current_stages() hands to a
// call) with their setters, and the exports that need no flow (error channel, device helpers, createMesh / deleteMesh, ICP, the outbound
// formats of the last mesh).
#include "host_ctx.hpp"

using namespace lsn::host;

namespace lsn {

// The error text lives in a fixed thread-local buffer: reporting a failure (an allocation failure, for one) must not allocate.
char *error_buffer() noexcept
{
    static thread_local char buf[kErrorLen] = {0};
    return buf;
}

void set_error(const char *fmt, ...) noexcept
{
    char *buf = error_buffer();
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, kErrorLen, fmt, ap);
    va_end(ap);
    if (getenv("LSN_VERBOSE")) fprintf(stderr, "[NativeUtils] %s\n", buf);
}

// Test hook of the exception trampoline (lsn::guarded): $LSN_TEST_THROW=n makes the n-th guarded entry of the process throw
// std::bad_alloc from inside the guarded region; $LSN_TEST_FAIL_ALLOC=n makes the n-th device / pinned allocation throw it
// (what a std::vector or std::map growing under memory pressure would do).  Read once.
static std::atomic<long> fault_points_seen[2];
long test_fault_points(int kind) { return kind >= 0 && kind < 2 ? fault_points_seen[kind].load() : -1; }

void test_fault_point(int kind)
{
    static const long want[2] = {getenv("LSN_TEST_THROW") ? atol(getenv("LSN_TEST_THROW")) : 0,
                                 getenv("LSN_TEST_FAIL_ALLOC") ? atol(getenv("LSN_TEST_FAIL_ALLOC")) : 0};
    const long n = ++fault_points_seen[kind];
    if (want[kind] > 0 && n == want[kind]) throw std::bad_alloc();
}

}  // namespace lsn

// (not routed through lsn::guarded: nothing in here can throw, and reading the message must not disturb it)
extern "C" int lsnGetLastError(char *buf, int len)
{
    const char *s = lsn::error_buffer();
    if (buf && len > 0) snprintf(buf, (size_t)len, "%s", s);
    return (int)strlen(s);
}

extern "C" int lsnDeviceCount(void)
{
    return lsn::guarded("lsnDeviceCount", -1, [&]() {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) {
            (void)hipGetLastError();
            return 0;
        }
        return n;
    });
}

// ---- device memory / streams for hosts without a HIP of their own ------------------------------------------------------------

extern "C" void * lsnDeviceMalloc(int device, long long bytes)
{
    return lsn::guarded("lsnDeviceMalloc", static_cast<void *>(nullptr), [&]() -> void * {
        lsn::clear_error();
        if (bytes <= 0) {
            lsn::set_error("lsnDeviceMalloc: bad size %lld", bytes);
            return nullptr;
        }
        LSN_HIP_NULL(hipSetDevice(device));
        void *p = nullptr;
        LSN_HIP_NULL(hipMalloc(&p, (size_t)bytes));
        return p;
    });
}

extern "C" int lsnDeviceFree(int device, void *d_ptr)
{
    return lsn::guarded("lsnDeviceFree", -1, [&]() {
        lsn::clear_error();
        if (!d_ptr) return 0;
        LSN_HIP(hipSetDevice(device));
        LSN_HIP(hipFree(d_ptr));
        return 0;
    });
}

extern "C" int lsnDeviceUpload(int device, void *d_dst, const void *h_src, long long bytes, void *stream)
{
    return lsn::guarded("lsnDeviceUpload", -1, [&]() {
        lsn::clear_error();
        if (!d_dst || !h_src || bytes < 0) {
            lsn::set_error("lsnDeviceUpload: bad arguments");
            return -1;
        }
        LSN_HIP(hipSetDevice(device));
        if (bytes > 0) LSN_HIP(hipMemcpyAsync(d_dst, h_src, (size_t)bytes, hipMemcpyHostToDevice, lsn::as_stream(stream)));
        return 0;
    });
}

extern "C" int lsnDeviceDownload(int device, void *h_dst, const void *d_src, long long bytes, void *stream)
{
    return lsn::guarded("lsnDeviceDownload", -1, [&]() {
        lsn::clear_error();
        if (!h_dst || !d_src || bytes < 0) {
            lsn::set_error("lsnDeviceDownload: bad arguments");
            return -1;
        }
        LSN_HIP(hipSetDevice(device));
        if (bytes > 0) LSN_HIP(hipMemcpyAsync(h_dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost, lsn::as_stream(stream)));
        return 0;
    });
}

extern "C" void * lsnStreamCreate(int device)
{
    return lsn::guarded("lsnStreamCreate", static_cast<void *>(nullptr), [&]() -> void * {
        lsn::clear_error();
        LSN_HIP_NULL(hipSetDevice(device));
        hipStream_t s = nullptr;
        LSN_HIP_NULL(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        return s;
    });
}

extern "C" int lsnStreamDestroy(int device, void *stream)
{
    return lsn::guarded("lsnStreamDestroy", -1, [&]() {
        lsn::clear_error();
        if (!stream) return 0;
        LSN_HIP(hipSetDevice(device));
        LSN_HIP(hipStreamDestroy(lsn::as_stream(stream)));
        return 0;
    });
}

extern "C" int lsnStreamSynchronize(int device, void *stream)
{
    return lsn::guarded("lsnStreamSynchronize", -1, [&]() {
        lsn::clear_error();
        LSN_HIP(hipSetDevice(device));
        LSN_HIP(hipStreamSynchronize(lsn::as_stream(stream)));
        return 0;
    });
}

// A process-wide pair of numbers that switches a filter of the exports: its first value comes from $env, written as `format` reads it
// (unset: off; malformed: off, with the message `malformed`); from then on it is what the last lsnSet* call set, and every export reads
// it when called.
namespace {
template <class A, class B>
struct PairSetting {
    std::mutex mu;
    A a{};
    B b{};
    PairSetting(const char *env, const char *format, const char *malformed)
    {
        const char *e = getenv(env);
        if (!e || !*e) return;
        A x{};
        B y{};
        int used = 0;
        if (sscanf(e, format, &x, &y, &used) == 2 && e[used] == '\0') {
            a = x;
            b = y;
        } else {
            fprintf(stderr, malformed, e);
        }
    }
    void current(A &x, B &y)
    {
        std::lock_guard<std::mutex> g(mu);
        x = a;
        y = b;
    }
    // lsnSet*: the previous pair goes to prev_* (either may be null)
    void exchange(A x, B y, A *prev_a, B *prev_b)
    {
        std::lock_guard<std::mutex> g(mu);
        if (prev_a) *prev_a = a;
        if (prev_b) *prev_b = b;
        a = x;
        b = y;
    }
};
}  // namespace

// (k, max_dist) of the exports' outlier filter (lsnSetOutlierFilter); never destroyed: an export may run while the process exits
static PairSetting<int, float> &outlier_setting()
{
    static auto *s = new PairSetting<int, float>(
        "LSN_OUTLIER_FILTER", " %d , %f %n",
        "[NativeUtils] $LSN_OUTLIER_FILTER=\"%s\" is not \"k,max_dist\" (e.g. \"10,0.1\"): the outlier filter stays off\n");
    return *s;
}

// (depth_tol, min_confidence) of the exports' colour blend (lsnSetColorBlend): generateMeshFromDepthMaps and lsnCorrectAndGenerateMesh read
// it, generateVerticesFromDepthMap never does (one sensor has no partner)
static PairSetting<int, int> &blend_setting()
{
    static auto *s = new PairSetting<int, int>(
        "LSN_COLOR_BLEND", " %d , %d %n",
        "[NativeUtils] $LSN_COLOR_BLEND=\"%s\" is not \"depth_tol,min_confidence\" (e.g. \"20,5\"): the colour blend stays off\n");
    return *s;
}

// (neighbourhood, threshold) of the flying-pixel filter of the exports that start at raw frames, i.e. with the radial correction:
// depthMapAndColorSetRadialCorrection and lsnCorrectAndGenerateMesh (lsnSetFlyingPixelFilter).  generateMeshFromDepthMaps and
// generateVerticesFromDepthMap never read it: LiveScanServer calls them on the maps the radial export has just returned
// (KinectServer.cs:518-525, :354-374), and the filter is not idempotent -- there it would run twice per tick.
static PairSetting<int, int> &flying_setting()
{
    static auto *s = new PairSetting<int, int>(
        "LSN_FLYING_PIXELS", " %d , %d %n",
        "[NativeUtils] $LSN_FLYING_PIXELS=\"%s\" is not \"neighbourhood,threshold\" (e.g. \"1,20\"): the flying-pixel filter stays off\n");
    return *s;
}

// The depth smoothing of the same two exports, between that filter and the correction (lsnSetDepthSmooth): (radius, sigma_s, sigma_r) and the
// Gaussian tables built from them, which a call takes with it (null: off).  generateMeshFromDepthMaps, generateVerticesFromDepthMap and
// lsnRefineFromDepthMaps never read it -- the first two for the flying pixels' reason: the filter is not idempotent either.
namespace {
struct SmoothSetting {
    std::mutex mu;
    std::shared_ptr<const lsn::DepthSmoothTables> tables;   // null: off
    float sigma_s = 0.0f, sigma_r = 0.0f;                   // what an "off" setting was given, so that the previous triple goes back as it came
    int radius = 0;
    SmoothSetting()
    {
        const char *e = getenv("LSN_DEPTH_SMOOTH");
        if (!e || !*e) return;
        int r = 0, used = 0;
        float ss = 0.0f, sr = 0.0f;
        if (sscanf(e, " %d , %f , %f %n", &r, &ss, &sr, &used) == 3 && e[used] == '\0' && exchange(r, ss, sr, nullptr, nullptr, nullptr) == 0) return;
        fprintf(stderr, "[NativeUtils] $LSN_DEPTH_SMOOTH=\"%s\" is not \"radius,sigma_s,sigma_r\" with a radius of at most 3 and positive sigmas "
                        "(e.g. \"2,1.5,12\"): depth smoothing stays off\n", e);
    }
    // lsnSetDepthSmooth: the new triple in, the previous one to prev_* (any may be null), under one acquisition of the lock; refused (-1,
    // lsnDepthSmoothGaussian's message) it leaves the setting and prev_* as they were
    int exchange(int r, float ss, float sr, int *prev_r, float *prev_ss, float *prev_sr)
    {
        std::shared_ptr<const lsn::DepthSmoothTables> fresh;
        if (r >= 1) {   // (the tables depend on the arguments alone: built, and refused, in front of the lock)
            auto t = std::make_shared<lsn::DepthSmoothTables>();
            if (lsn::depth_smooth_gaussian(r, ss, sr, *t)) return -1;
            fresh = t;
        }
        std::lock_guard<std::mutex> g(mu);
        if (prev_r) *prev_r = radius;
        if (prev_ss) *prev_ss = sigma_s;
        if (prev_sr) *prev_sr = sigma_r;
        tables = fresh;
        radius = r;
        sigma_s = ss;
        sigma_r = sr;
        return 0;
    }
    std::shared_ptr<const lsn::DepthSmoothTables> current()
    {
        std::lock_guard<std::mutex> g(mu);
        return tables;
    }
};
}  // namespace

static SmoothSetting &smooth_setting()
{
    static auto *s = new SmoothSetting();   // never destroyed, like the pairs above
    return *s;
}

// The process-wide switch of a stage with state, for the same two exports: the triple as the stage holds it and as it was given, the
// generation its reset export advances, the rig of the last call with the stage on.  A lane whose state is of an older generation starts
// from none; a call of another rig than the last one's starts a generation of its own, so that every lane -- the shards' too, which only
// ever see their blocks -- does.  The other exports never read the switches, for the flying pixels' reason: there the stage would run
// twice per tick.
//   the temporal depth filter, in front of the flying-pixel filter: lsnSetTemporalFilter (alpha_q, delta, persist), lsnResetTemporalFilter;
//   background subtraction, behind the temporal filter: lsnSetBackground (margin, rel_q, min_pixels), lsnLearnBackground, which also sets
//   the learning calls a lane runs on a zeroed model before it subtracts ($LSN_BACKGROUND's optional fourth field).
namespace {
template <class Setting>
struct StageSwitch {
    std::mutex mu;
    Setting setting;
    int given[3] = {0, 0, 0};        // what an "off" setting was given, so that the previous triple goes back as it came
    int learn_calls = 0;             // the last value lsnLearnBackground (or the environment) requested
    unsigned long long gen = 1;
    std::vector<int> rig;            // sensor count, widths, heights
    int (*const ok)(const char *, int, int, int);
    const char *const who;           // the set export, for the validator's message
    // env: the variable; usage: its form with an example; what: the stage, for "... stays off"; fourth: a learn_calls field is admitted
    StageSwitch(int (*validator)(const char *, int, int, int), const char *set_export, const char *env, const char *usage, const char *what, bool fourth)
        : ok(validator), who(set_export)
    {
        const char *e = getenv(env);
        if (!e || !*e) return;
        int a = 0, b = 0, c = 0, n = 0, used = 0;
        const int got = sscanf(e, " %d , %d , %d %n, %d %n", &a, &b, &c, &used, &n, &used);
        if ((got == 3 || (fourth && got == 4)) && e[used] == '\0' && n >= 0) {
            if (exchange(a, b, c, nullptr, nullptr, nullptr) == 0) {
                learn_calls = n;
                return;
            }
            fprintf(stderr, "[NativeUtils] $%s=\"%s\": %s: %s stays off\n", env, e, lsn::error_buffer(), what);
            lsn::clear_error();
            return;
        }
        fprintf(stderr, "[NativeUtils] $%s=\"%s\" is not %s: %s stays off\n", env, e, usage, what);
    }
    // the set export: the new triple in, the previous one to prev_* (any may be null), under one acquisition of the lock; refused (-1, with
    // the message) it leaves the setting and prev_* as they were
    int exchange(int a, int b, int c, int *prev_a, int *prev_b, int *prev_c)
    {
        if (ok(who, a, b, c)) return -1;
        std::lock_guard<std::mutex> g(mu);
        if (prev_a) *prev_a = given[0];
        if (prev_b) *prev_b = given[1];
        if (prev_c) *prev_c = given[2];
        setting = a >= 1 ? Setting{a, b, c} : Setting{};
        given[0] = a;
        given[1] = b;
        given[2] = c;
        return 0;
    }
    // the reset export: every lane finds its state stale at its next call with the stage on
    void advance(int learn)
    {
        std::lock_guard<std::mutex> g(mu);
        learn_calls = learn;
        gen++;
    }
    // what a call of this rig takes with it
    void current(Setting &st, unsigned long long &generation, int &learn, int n_maps, const int *widths, const int *heights)
    {
        std::lock_guard<std::mutex> g(mu);
        st = setting;
        if (st.on() && n_maps > 0 && widths && heights) {
            std::vector<int> now(1, n_maps);
            now.insert(now.end(), widths, widths + n_maps);
            now.insert(now.end(), heights, heights + n_maps);
            if (now != rig) {
                rig.swap(now);
                gen++;
            }
        }
        generation = gen;
        learn = learn_calls;
    }
};
}  // namespace

static StageSwitch<lsn::TemporalSetting> &temporal_switch()
{
    static auto *s = new StageSwitch<lsn::TemporalSetting>(   // never destroyed, like the pairs above
        lsn::temporal_setting_ok, "lsnSetTemporalFilter", "LSN_TEMPORAL_FILTER", "\"alpha_q,delta,persist\" (e.g. \"64,20,2\")", "the temporal filter", false);
    return *s;
}

static StageSwitch<lsn::BackgroundSetting> &background_switch()
{
    static auto *s = new StageSwitch<lsn::BackgroundSetting>(   // never destroyed, like the pairs above
        lsn::background_setting_ok, "lsnSetBackground", "LSN_BACKGROUND", "\"margin,rel_q,min_pixels[,learn_calls]\" (e.g. \"40,8,64,30\")",
        "background subtraction", true);
    return *s;
}

// The stages in front of the radial correction that a call of this rig takes with it: the four switches as they stand when it is called.
static DepthStages current_stages(int n_maps, const int *widths, const int *heights)
{
    DepthStages st;
    flying_setting().current(st.fp_neighbourhood, st.fp_threshold);
    st.smooth = smooth_setting().current();
    int no_learning = 0;
    temporal_switch().current(st.temporal, st.temporal_gen, no_learning, n_maps, widths, heights);
    background_switch().current(st.background, st.background_gen, st.background_learn, n_maps, widths, heights);
    return st;
}

// What the three mesh exports share: `call` as `name` filled it (everything but the outlier filter's and the colour blend's settings, which are read here) runs on
// lane `l` of the context.  0: *out_mesh is the call's mesh; -1: the call was refused or failed, *out_mesh (if there is one) is empty and,
// unless the caller merely passed no sensors, the message is set.
static int mesh_export(const char *name, Lane &l, MeshCall &call, Mesh *out_mesh)
{
    lsn::clear_error();
    if (!out_mesh) return -1;
    std::lock_guard<std::mutex> g(l.mu);
    if (call.count <= 0 || call.first < 0 || !call.depth_maps || !call.depth_colors || !call.widths || !call.heights || !call.intr || !call.wt) {
        if (call.count != 0) lsn::set_error("%s: bad arguments", name);
        empty_mesh(out_mesh);
        return -1;
    }
    outlier_setting().current(call.outlier_k, call.outlier_max_dist);
    blend_setting().current(call.blend_tol, call.blend_min_conf);   // (MeshCall::blends(): never on one sensor)
    Ctx &c = ctx();
    if (ensure_ready(c) || fuse_host(c, l, call, out_mesh)) {
        empty_mesh(out_mesh);
        return -1;
    }
    return 0;
}

extern "C" void generateVerticesFromDepthMap(unsigned char *depth_maps, unsigned char *depth_colors, int *widths, int *heights,
                                             float *intr_params, float *wtransform_params, Mesh *out_mesh, float minX, float minY,
                                             float minZ, float maxX, float maxY, float maxZ, int depth_map_index)
{
    const bool done = lsn::guarded("generateVerticesFromDepthMap", false, [&]() {
        const float b[6] = {minX, minY, minZ, maxX, maxY, maxZ};
        MeshCall call;
        call.depth_maps = depth_maps;
        call.depth_colors = depth_colors;
        call.widths = widths;
        call.heights = heights;
        call.intr = intr_params;
        call.wt = wtransform_params;
        call.bounds6 = b;
        call.first = depth_map_index;
        call.count = 1;
        (void)mesh_export("generateVerticesFromDepthMap", ctx().single, call, out_mesh);
        return true;
    });
    if (!done && out_mesh) empty_mesh(out_mesh);   // nothing reaches the caller but an empty mesh and the message
}

// lsnSetOverlayMerge: whether generateMeshFromDepthMaps(..., bgenerate_triangles = true) runs the overlay merge; read once from $LSN_OVERLAY_MERGE
static std::atomic<int> &overlay_merge_switch()
{
    static std::atomic<int> on{[] {
        const char *e = getenv("LSN_OVERLAY_MERGE");
        return e && strcmp(e, "1") == 0 ? 1 : 0;
    }()};
    return on;
}

extern "C" int lsnSetOverlayMerge(int enable) { return overlay_merge_switch().exchange(enable ? 1 : 0); }

extern "C" int lsnSetOutlierFilter(int k, float max_dist, int *prev_k, float *prev_max_dist)
{
    return lsn::guarded("lsnSetOutlierFilter", -1, [&]() {
        outlier_setting().exchange(k, max_dist, prev_k, prev_max_dist);
        return 0;
    });
}

extern "C" int lsnSetColorBlend(int depth_tol, int min_confidence, int *prev_depth_tol, int *prev_min_confidence)
{
    return lsn::guarded("lsnSetColorBlend", -1, [&]() {
        blend_setting().exchange(depth_tol, min_confidence, prev_depth_tol, prev_min_confidence);
        return 0;
    });
}

extern "C" int lsnSetFlyingPixelFilter(int neighbourhood, int threshold, int *prev_neighbourhood, int *prev_threshold)
{
    return lsn::guarded("lsnSetFlyingPixelFilter", -1, [&]() {
        flying_setting().exchange(neighbourhood, threshold, prev_neighbourhood, prev_threshold);
        return 0;
    });
}

extern "C" int lsnSetDepthSmooth(int radius, float sigma_s, float sigma_r, int *prev_radius, float *prev_sigma_s, float *prev_sigma_r)
{
    return lsn::guarded("lsnSetDepthSmooth", -1, [&]() {
        lsn::clear_error();
        return smooth_setting().exchange(radius, sigma_s, sigma_r, prev_radius, prev_sigma_s, prev_sigma_r);
    });
}

extern "C" int lsnSetTemporalFilter(int alpha_q, int delta, int persist, int *prev_alpha_q, int *prev_delta, int *prev_persist)
{
    return lsn::guarded("lsnSetTemporalFilter", -1, [&]() {
        lsn::clear_error();
        return temporal_switch().exchange(alpha_q, delta, persist, prev_alpha_q, prev_delta, prev_persist);
    });
}

extern "C" int lsnResetTemporalFilter(void)
{
    return lsn::guarded("lsnResetTemporalFilter", -1, [&]() {
        lsn::clear_error();
        temporal_switch().advance(0);   // every lane finds its history stale at its next filtering call
        return 0;
    });
}

extern "C" int lsnSetBackground(int margin, int rel_q, int min_pixels, int *prev_margin, int *prev_rel_q, int *prev_min_pixels)
{
    return lsn::guarded("lsnSetBackground", -1, [&]() {
        lsn::clear_error();
        return background_switch().exchange(margin, rel_q, min_pixels, prev_margin, prev_rel_q, prev_min_pixels);
    });
}

extern "C" int lsnLearnBackground(int n_calls)
{
    return lsn::guarded("lsnLearnBackground", -1, [&]() {
        lsn::clear_error();
        if (n_calls < 0) {
            lsn::set_error("lsnLearnBackground: n_calls %d is negative", n_calls);
            return -1;
        }
        background_switch().advance(n_calls);   // every lane finds its model stale at its next call with the stage on
        return 0;
    });
}

extern "C" void generateMeshFromDepthMaps(int n_maps, unsigned char *depth_maps, unsigned char *depth_colors, int *widths, int *heights,
                                          float *intr_params, float *wtransform_params, Mesh *out_mesh, bool bcolor_transfer, float minX,
                                          float minY, float minZ, float maxX, float maxY, float maxZ, bool bgenerate_triangles)
{
    const bool done = lsn::guarded("generateMeshFromDepthMaps", false, [&]() {
        const float b[6] = {minX, minY, minZ, maxX, maxY, maxZ};
        // the overlay merge runs when the caller asks for it and the process opted in (lsnSetOverlayMerge / $LSN_OVERLAY_MERGE); it needs
        // every sensor of the same size (merge.hip): otherwise the unmerged mesh goes back, with a message
        bool merge = bgenerate_triangles && overlay_merge_switch().load();
        bool mixed = false;
        for (int i = 1; merge && widths && heights && i < n_maps; i++) mixed |= widths[i] != widths[0] || heights[i] != heights[0];
        merge &= !mixed;
        MeshCall call;
        call.depth_maps = depth_maps;
        call.depth_colors = depth_colors;
        call.widths = widths;
        call.heights = heights;
        call.intr = intr_params;
        call.wt = wtransform_params;
        call.bounds6 = b;
        call.count = n_maps;
        call.with_triangles = true;
        call.color_transfer = bcolor_transfer;
        call.overlay_merge = merge;
        Ctx &c = ctx();
        if (mesh_export("generateMeshFromDepthMaps", c.merge, call, out_mesh)) return true;
        if (merge) return true;
        if (mixed) {
            lsn::set_error("generateMeshFromDepthMaps: the overlay merge needs every sensor of the same size; returned the unmerged mesh");
            return true;
        }
        // bcolor_transfer is implemented (color.hip, through fuse_host's colour flow); the overlay merge is not
        if (bgenerate_triangles) {
            lsn::set_error("generateMeshFromDepthMaps: colour transfer / overlay merge are outside this library's scope; "
                           "returned the cropped vertices of all sensors (flags false,false behaviour)");
            if (!c.warned_flags) {
                // nobody on the C# side reads lsnGetLastError, and bGenerateTriangles = true is LiveScanServer's default
                // (KinectSettings.cs:50): say it once per process where an operator can see it
                c.warned_flags = true;
                fprintf(stderr, "[NativeUtils] generateMeshFromDepthMaps was called with bcolor_transfer=%d bgenerate_triangles=%d: this library "
                                "implements the (false, false) behaviour only (no cross-view overlay merge, no colour transfer); the mesh "
                                "returned is the unmerged one. Set bGenerateTriangles / bColorTransfer to false in LiveScanServer's settings.\n",
                        (int)bcolor_transfer, (int)bgenerate_triangles);
            }
        }
        return true;
    });
    if (!done && out_mesh) empty_mesh(out_mesh);   // nothing reaches the caller but an empty mesh and the message
}

extern "C" void lsnCorrectAndGenerateMesh(int n_maps, unsigned char *depth_maps, unsigned char *depth_colors, int *widths, int *heights,
                                          float *intr_params, float *wtransform_params, Mesh *out_mesh, float minX, float minY, float minZ,
                                          float maxX, float maxY, float maxZ, int write_back_corrected)
{
    const bool done = lsn::guarded("lsnCorrectAndGenerateMesh", false, [&]() {
        const float b[6] = {minX, minY, minZ, maxX, maxY, maxZ};
        MeshCall call;
        call.depth_maps = depth_maps;
        call.depth_colors = depth_colors;
        call.widths = widths;
        call.heights = heights;
        call.intr = intr_params;
        call.wt = wtransform_params;
        call.bounds6 = b;
        call.count = n_maps;
        call.with_triangles = true;
        call.radial = true;
        call.back_d = write_back_corrected ? depth_maps : nullptr;
        call.back_c = write_back_corrected ? depth_colors : nullptr;
        call.stages = current_stages(n_maps, widths, heights);
        (void)mesh_export("lsnCorrectAndGenerateMesh", ctx().merge, call, out_mesh);
        return true;
    });
    if (!done && out_mesh) empty_mesh(out_mesh);   // nothing reaches the caller but an empty mesh and the message
}

extern "C" void depthMapAndColorSetRadialCorrection(int n_maps, unsigned char *depth_maps, unsigned char *depth_colors, int *widths,
                                                    int *heights, float *intr_params)
{
    lsn::guarded_void("depthMapAndColorSetRadialCorrection", [&]() {
        lsn::clear_error();
        if (n_maps <= 0 || !depth_maps || !depth_colors || !widths || !heights || !intr_params) {
            if (n_maps != 0) lsn::set_error("depthMapAndColorSetRadialCorrection: bad arguments");
            return;
        }
        Ctx &c = ctx();
        Lane &l = c.merge;
        std::lock_guard<std::mutex> g(l.mu);
        if (ensure_ready(c)) return;
        radial_host(c, l, n_maps, depth_maps, depth_colors, widths, heights, intr_params, current_stages(n_maps, widths, heights));
    });
}

// LiveScanServer's "Refine calibration" as one call: the frames go up once, the clouds never leave the device.  The fusion runs on the
// single-sensor lane -- the refine worker's lane, so the update worker's merge calls go on beside it -- and on that lane's device alone,
// whatever $LSN_HOST_DEVICES says; the pass itself is refine.hip's (lsn::refine_cloud).  Every result is computed into scratch first: a call
// that fails has touched none of the caller's arrays.
extern "C" int lsnRefineFromDepthMaps(int n_maps, unsigned char *depth_maps, unsigned char *depth_colors, int *widths, int *heights,
                                      float *intr_params, float *wtransform_params, float minX, float minY, float minZ, float maxX, float maxY,
                                      float maxZ, int correct_radial, int n_refine_iters, int n_icp_iters, float *wtransform_refined,
                                      float *camera_R, float *camera_t, float *Rs_out, float *Ts_out, float *clouds_out, int *counts_out)
{
    return lsn::guarded("lsnRefineFromDepthMaps", -1, [&]() {
        lsn::clear_error();
        if (n_maps <= 0 || !depth_maps || !depth_colors || !widths || !heights || !intr_params || !wtransform_params) {
            lsn::set_error("lsnRefineFromDepthMaps: bad arguments");
            return -1;
        }
        const float b[6] = {minX, minY, minZ, maxX, maxY, maxZ};
        MeshCall call;
        call.depth_maps = depth_maps;
        call.depth_colors = depth_colors;
        call.widths = widths;
        call.heights = heights;
        call.intr = intr_params;
        call.wt = wtransform_params;
        call.bounds6 = b;
        call.count = n_maps;
        call.radial = correct_radial != 0;
        if (call.radial) flying_setting().current(call.stages.fp_neighbourhood, call.stages.fp_threshold);
        outlier_setting().current(call.outlier_k, call.outlier_max_dist);
        Ctx &c = ctx();
        Lane &l = c.single;
        std::lock_guard<std::mutex> g(l.mu);
        if (ensure_ready(c)) return -1;
        std::vector<int> offsets((size_t)n_maps + 1);
        if (fuse_resident(c, l, call, offsets.data())) return -1;
        const size_t cloud_bytes = sizeof(float) * 3 * (size_t)offsets[n_maps];
        // the refined points come home through a pinned block of the pool (recycled call after call; the download runs as DMA into it)
        struct Block {
            Ctx &c;
            void *p = nullptr;
            explicit Block(Ctx &c_) : c(c_) {}
            ~Block() { if (p) pinned_put(c, p); }
        } home(c);
        if (clouds_out && cloud_bytes > 0 && !(home.p = pinned_get(c, cloud_bytes))) return -1;
        std::vector<float> Rt((size_t)n_maps * 12);
        if (lsn::refine_cloud("lsnRefineFromDepthMaps", l.device, n_maps, l.d_out.p, offsets.data(), n_refine_iters, n_icp_iters, Rt.data(),
                              static_cast<float *>(home.p), nullptr))
            return -1;
        // worldTransforms[i] = {t[3], R[3][3]} of wtransform_params: unpacked, composed, packed again
        std::vector<float> world_R((size_t)n_maps * 9), world_t((size_t)n_maps * 3);
        for (int i = 0; i < n_maps; i++) {
            memcpy(world_t.data() + 3 * (size_t)i, wtransform_params + 12 * (size_t)i, 3 * sizeof(float));
            memcpy(world_R.data() + 9 * (size_t)i, wtransform_params + 12 * (size_t)i + 3, 9 * sizeof(float));
        }
        lsn::refine_compose(n_maps, Rt.data(), world_R.data(), world_t.data(), camera_R, camera_t, Rs_out, Ts_out);
        for (int i = 0; wtransform_refined && i < n_maps; i++) {
            memcpy(wtransform_refined + 12 * (size_t)i, world_t.data() + 3 * (size_t)i, 3 * sizeof(float));
            memcpy(wtransform_refined + 12 * (size_t)i + 3, world_R.data() + 9 * (size_t)i, 9 * sizeof(float));
        }
        if (home.p) memcpy(clouds_out, home.p, cloud_bytes);
        for (int i = 0; counts_out && i < n_maps; i++) counts_out[i] = offsets[i + 1] - offsets[i];
        return 0;
    });
}

extern "C" Mesh * createMesh(void)
{
    return lsn::guarded("createMesh", static_cast<Mesh *>(nullptr), [&]() -> Mesh * {
        Mesh *m = (Mesh *)calloc(1, sizeof(Mesh));  // zeroed like depthprocessing.cpp:1820-1825
        return m;
    });
}

extern "C" void deleteMesh(Mesh *mesh)
{
    lsn::guarded_void("deleteMesh", [&]() {
        if (!mesh) return;
        Ctx &c = ctx();
        if (mesh->triangles) pinned_put(c, mesh->triangles);   // a pinned block of ours; the static empty array or a foreign pointer is left alone
        if (mesh->vertices) pinned_put(c, mesh->vertices);
        mesh->triangles = nullptr;
        mesh->vertices = nullptr;
    });
}

// ICP's flow on host arrays, for either residual: the context's workspace, lock, stream and device buffers, pinned scratch for the way
// home, the caller's buffers untouched unless everything worked.  normals1 (nullable): the target's normals -- the point-to-plane step.
// 0, or -1 (the message is set wherever the failure has one).
static int icp_on_host_arrays(const char *who, Point3f *verts1, Point3f *normals1, Point3f *verts2, int nVerts1, int nVerts2, float *R, float *t, int maxIter)
{
    Ctx &c = ctx();
    std::lock_guard<std::mutex> g(c.icp_mu);   // not c.mu: merge calls go on while a refine call runs
    if (ensure_ready(c)) return -1;
    if (!c.icp || nVerts1 > c.icp_n1 || nVerts2 > c.icp_n2) {
        if (c.icp) lsnIcpDestroy(c.icp);
        c.icp_n1 = nVerts1 > c.icp_n1 ? nVerts1 : c.icp_n1;
        c.icp_n2 = nVerts2 > c.icp_n2 ? nVerts2 : c.icp_n2;
        c.icp = lsnIcpCreate(c.device, c.icp_n1, c.icp_n2);
        if (!c.icp) {
            c.icp_n1 = c.icp_n2 = 0;
            return -1;
        }
    }
    const size_t v1_bytes = sizeof(float) * 3 * (size_t)nVerts1;
    if (c.d_v1.reserve(v1_bytes) || c.d_v2.reserve(sizeof(float) * 3 * (size_t)nVerts2) || c.d_Rt.reserve(64) || (normals1 && c.d_n1.reserve(v1_bytes)))
        return -1;
    const char *env = getenv("LSN_NN");
    const int nn_mode = (env && strcmp(env, "brute") == 0) ? 0 : 1;
    if (hipMemcpyAsync(c.d_v1.p, verts1, v1_bytes, hipMemcpyHostToDevice, c.icp_stream) != hipSuccess ||
        (normals1 && hipMemcpyAsync(c.d_n1.p, normals1, v1_bytes, hipMemcpyHostToDevice, c.icp_stream) != hipSuccess) ||
        hipMemcpyAsync(c.d_v2.p, verts2, sizeof(float) * 3 * (size_t)nVerts2, hipMemcpyHostToDevice, c.icp_stream) != hipSuccess ||
        hipMemcpyAsync(c.d_Rt.p, R, sizeof(float) * 9, hipMemcpyHostToDevice, c.icp_stream) != hipSuccess ||
        hipMemcpyAsync(c.d_Rt.as<float>() + 9, t, sizeof(float) * 3, hipMemcpyHostToDevice, c.icp_stream) != hipSuccess) {
        lsn::set_error("%s: upload failed: %s", who, hipGetErrorString(hipGetLastError()));
        return -1;
    }
    const int rc = normals1 ? lsnIcpRunPlane(c.icp, c.d_v1.as<float>(), c.d_n1.as<float>(), nVerts1, c.d_v2.as<float>(), nVerts2, c.d_Rt.as<float>(),
                                             c.d_Rt.as<float>() + 9, maxIter, nn_mode, c.icp_stream)
                            : lsnIcpRun(c.icp, c.d_v1.as<float>(), nVerts1, c.d_v2.as<float>(), nVerts2, c.d_Rt.as<float>(), c.d_Rt.as<float>() + 9, maxIter,
                                        nn_mode, c.icp_stream);
    if (rc) return -1;
    // results go to a scratch first so that the caller's buffers stay untouched when anything fails: a pinned block of the pool
    // (recycled call after call; the download runs as DMA into it)
    const size_t v2_bytes = sizeof(float) * 3 * (size_t)nVerts2;
    float *v2 = static_cast<float *>(pinned_get(c, v2_bytes + sizeof(float) * 12));
    if (!v2) return -1;
    float *Rt = v2 + (size_t)nVerts2 * 3;
    if (hipMemcpyAsync(v2, c.d_v2.p, v2_bytes, hipMemcpyDeviceToHost, c.icp_stream) != hipSuccess ||
        hipMemcpyAsync(Rt, c.d_Rt.p, sizeof(float) * 12, hipMemcpyDeviceToHost, c.icp_stream) != hipSuccess ||
        hipStreamSynchronize(c.icp_stream) != hipSuccess) {
        lsn::set_error("%s: download failed: %s", who, hipGetErrorString(hipGetLastError()));
        (void)hipStreamSynchronize(c.icp_stream);
        pinned_put(c, v2);
        return -1;
    }
    memcpy(verts2, v2, v2_bytes);
    memcpy(R, Rt, sizeof(float) * 9);
    memcpy(t, Rt + 9, sizeof(float) * 3);
    pinned_put(c, v2);
    return 0;
}

extern "C" float ICP(Point3f *verts1, Point3f *verts2, int nVerts1, int nVerts2, float *R, float *t, int maxIter)
{
    return lsn::guarded("ICP", 1.0f, [&]() {
        lsn::clear_error();
        const float error = 1.0f;  // icp.cpp:85,176
        if (!verts1 || !verts2 || !R || !t || nVerts1 <= 0 || nVerts2 <= 0 || maxIter <= 0) {
            // the reference would throw out of nanoflann on an empty cloud (include/nanoflann.h:904); callers guard
            if (nVerts1 <= 0 || nVerts2 <= 0) lsn::set_error("ICP: empty cloud (nVerts1=%d nVerts2=%d)", nVerts1, nVerts2);
            return error;
        }
        (void)icp_on_host_arrays("ICP", verts1, nullptr, verts2, nVerts1, nVerts2, R, t, maxIter);
        return error;
    });
}

extern "C" int lsnIcpPointToPlane(Point3f *verts1, Point3f *normals1, Point3f *verts2, int nVerts1, int nVerts2, float *R, float *t, int maxIter)
{
    return lsn::guarded("lsnIcpPointToPlane", -1, [&]() {
        lsn::clear_error();
        if (!verts1 || !normals1 || !verts2 || !R || !t || nVerts1 <= 0 || nVerts2 <= 0) {
            lsn::set_error("lsnIcpPointToPlane: null argument or empty cloud (nVerts1=%d nVerts2=%d)", nVerts1, nVerts2);
            return -1;
        }
        if (maxIter <= 0) return 0;   // nothing to do: the caller's arrays stay as they are
        return icp_on_host_arrays("lsnIcpPointToPlane", verts1, normals1, verts2, nVerts1, nVerts2, R, t, maxIter);
    });
}

// ---- the outbound formats of the mesh the last merge call left in HBM (include/NativeUtils.h part 3) ----------------------------

namespace {
// The exports below as steps on the mesh the calling thread's last mesh call left: the lane is picked and locked here; `resident` says
// whether there is a mesh (from then on nv / nt are its counts, and a call that only asks for a length is answered); `open` puts it into
// HBM and makes it a batch of one tick of one "sensor" whose offset rows are its two counts; `fragments`, `lod`, `smooth` and `normals`
// run their stage on what the step before left, `render`, `frame` and `ply` bring the result home.  Locks: the lane's, then c.wire_mu
// from `open` on.
struct LastMesh {
    Ctx &c;
    Lane &l;
    std::lock_guard<std::mutex> lane_lock;
    std::unique_lock<std::mutex> wire_lock;
    int nv = 0, nt = 0;              // the mesh the next step sees ...
    int nv0 = 0, nt0 = 0;            // ... and its strides: the resident mesh's counts (the simplified mesh keeps them)
    const void *d_v = nullptr;
    const int *d_t = nullptr, *d_rows = nullptr;   // d_rows: {0, nv}, {0, nt} on the device

    static Lane &pick(Ctx &c)
    {
        Lane *l = t_last_lane ? t_last_lane : c.last_lane.load();   // this thread's own last mesh call, else the process's
        return l ? *l : c.merge;
    }
    LastMesh() : c(ctx()), l(pick(c)), lane_lock(l.mu) {}

    int resident()
    {
        if (ensure_ready(c)) return -1;
        if (l.last_nv < 0) {
            lsn::set_error("lsnLastMesh*: no mesh is resident (call generateMeshFromDepthMaps / generateVerticesFromDepthMap first)");
            return -1;
        }
        nv = nv0 = l.last_nv;
        nt = nt0 = l.last_nt;
        return 0;
    }
    int open(long long wire_bytes = 0)   // wire_bytes: what a packer may write
    {
        if (materialize(l)) return -1;
        wire_lock = std::unique_lock<std::mutex>(c.wire_mu);
        if (wire_bytes > 0 && c.d_wire.reserve((size_t)wire_bytes + 16)) return -1;
        LSN_HIP(hipSetDevice(l.device));
        if (c.d_mesh_rows.reserve(sizeof(c.mesh_rows))) return -1;
        c.mesh_rows[0] = 0; c.mesh_rows[1] = nv; c.mesh_rows[2] = 0; c.mesh_rows[3] = nt;
        LSN_HIP(hipMemcpyAsync(c.d_mesh_rows.p, c.mesh_rows, 4 * sizeof(int), hipMemcpyHostToDevice, l.stream));
        d_v = l.d_out.p;
        d_t = l.d_tri.as<int>();
        d_rows = c.d_mesh_rows.as<int>();
        return 0;
    }
    lsn::MeshBatch batch(bool points_only = false) const
    {
        return {static_cast<const uint4 *>(d_v), d_rows, nt0 > 0 && !points_only ? d_t : nullptr, d_rows + 2, nv0, nt0 > 0 ? nt0 : 0, 1, 1};
    }
    // the level of detail (simplify.hip), in HBM: the later steps see the simplified mesh and the rows the stage wrote
    int lod(const char *who, float cell)
    {
        if (nv <= 0) return 0;
        // (the batch's strides, which the stage's overlap test measures with: the fragment filter may have left fewer than nv0 / nt0)
        if (c.d_lod_v.reserve(16 * (size_t)nv0) || c.d_lod_t.reserve(12 * (size_t)(nt0 > 0 ? nt0 : 1))) return -1;
        int *out_rows = c.d_mesh_rows.as<int>() + 4;
        if (lsn::simplify(c.sp, who, batch(), cell, c.d_lod_v.p, out_rows, c.d_lod_t.p, out_rows + 2, nullptr, l.stream)) return -1;
        LSN_HIP(hipMemcpyAsync(c.mesh_rows + 4, out_rows, 4 * sizeof(int), hipMemcpyDeviceToHost, l.stream));
        LSN_HIP(hipStreamSynchronize(l.stream));
        nv = c.mesh_rows[5];
        if (nt > 0) nt = c.mesh_rows[7];
        d_v = c.d_lod_v.p;
        d_t = c.d_lod_t.as<int>();
        d_rows = out_rows;
        return 0;
    }
    // the fragment filter (fragments.hip), in HBM, in front of `lod`: the later steps see the filtered mesh and the rows the stage wrote.
    // min_vertices <= 1 is the stage's "off", a copy: the mesh stays where it is.
    int fragments(const char *who, int min_vertices)
    {
        if (min_vertices <= 1 || nv <= 0) return 0;
        if (c.d_frag_v.reserve(16 * (size_t)nv) || c.d_frag_t.reserve(12 * (size_t)(nt > 0 ? nt : 1))) return -1;
        int *out_rows = c.d_mesh_rows.as<int>() + 8;
        if (lsn::fragments(c.fr, who, batch(), min_vertices, c.d_frag_v.p, out_rows, c.d_frag_t.p, out_rows + 2, nullptr, nullptr, l.stream)) return -1;
        LSN_HIP(hipMemcpyAsync(c.mesh_rows + 8, out_rows, 4 * sizeof(int), hipMemcpyDeviceToHost, l.stream));
        LSN_HIP(hipStreamSynchronize(l.stream));
        nv = c.mesh_rows[9];
        nt = c.mesh_rows[11];
        d_v = c.d_frag_v.p;
        d_t = c.d_frag_t.as<int>();
        d_rows = out_rows;
        return 0;
    }
    // Taubin smoothing (smooth.hip), in HBM, behind `lod`: the later steps see the moved vertices; the rows and the triangles stay
    int smooth(const char *who, int iterations, float lambda, float mu, int pin_boundary)
    {
        if (c.d_sm_v.reserve(16 * (size_t)(nv0 > 0 ? nv0 : 1))) return -1;
        if (lsn::smooth(c.sm, who, batch(), iterations, lambda, mu, pin_boundary, c.d_sm_v.p, l.stream)) return -1;
        d_v = c.d_sm_v.p;
        return 0;
    }
    // the vertex normals (normals.hip) of that mesh into c.d_nm
    int normals(const char *who)
    {
        if (c.d_nm.reserve(12 * (size_t)(nv0 > 0 ? nv0 : 1))) return -1;
        return lsn::normals(c.nm, who, batch(), c.d_nm.p, nullptr, l.stream);
    }
    // one view of it (render.hip) into the host arrays; the pixels with depth != 0
    long long render(const char *who, const float *intr7, const float *wt12, int width, int height, bool points_only, unsigned char *depth_out,
                     unsigned char *colors_out)
    {
        const size_t npix = (size_t)(width > 0 ? width : 0) * (size_t)(height > 0 ? height : 0);
        if (c.d_rv_img.reserve(5 * npix + 16)) return -1;
        unsigned char *d_depth = c.d_rv_img.as<unsigned char>(), *d_col = d_depth + 2 * npix;
        if (lsn::render_views(c.rv, who, batch(points_only), 1, intr7, wt12, width, height, d_depth, d_col, l.stream)) return -1;
        LSN_HIP(hipMemcpyAsync(depth_out, d_depth, 2 * npix, hipMemcpyDeviceToHost, l.stream));
        LSN_HIP(hipMemcpyAsync(colors_out, d_col, 3 * npix, hipMemcpyDeviceToHost, l.stream));
        int n_pixels = 0;
        if (lsn::render_counts(c.rv, who, 0, 0, nullptr, nullptr, &n_pixels, l.stream)) return -1;   // synchronises
        return n_pixels;
    }
    // the TransferSocket.SendFrame stream of it, at most `bound` bytes, into out
    long long frame(long long bound, unsigned char *out, long long out_cap)
    {
        if (!c.xfer || nv > c.xfer_v || nt > c.xfer_t) {
            if (c.xfer) lsnTransferDestroy(c.xfer);
            c.xfer_v = nv > c.xfer_v ? nv : c.xfer_v;
            c.xfer_t = nt > c.xfer_t ? nt : c.xfer_t;
            c.xfer = lsnTransferCreate(c.device, c.xfer_v, c.xfer_t);
            if (!c.xfer) {
                c.xfer_v = c.xfer_t = 0;
                return -1;
            }
        }
        return home(lsnTransferPack(c.xfer, d_v, nv, nt > 0 ? d_t : nullptr, nt, c.d_wire.p, bound, l.stream), out, out_cap);
    }
    // the binary PLY file image of it, with the normals of c.d_nm if asked
    long long ply(long long bound, bool with_normals, unsigned char *out, long long out_cap)
    {
        const int *tri = nt > 0 ? d_t : nullptr;
        return home(with_normals ? lsnPlyPackNormals(c.device, d_v, c.d_nm.p, nv, tri, nt, c.d_wire.p, bound, l.stream)
                                 : lsnPlyPack(c.device, d_v, nv, tri, nt, c.d_wire.p, bound, l.stream),
                    out, out_cap);
    }
    long long home(long long n, unsigned char *out, long long out_cap)
    {
        if (n < 0) return -1;
        if (n > out_cap) {
            (void)hipStreamSynchronize(l.stream);
            lsn::set_error("lsnLastMesh*: the result is %lld bytes, the buffer holds %lld", n, out_cap);
            return -1;
        }
        LSN_HIP(hipMemcpyAsync(out, c.d_wire.p, (size_t)n, hipMemcpyDeviceToHost, l.stream));
        LSN_HIP(hipStreamSynchronize(l.stream));
        return n;
    }
};
}  // namespace

// out == NULL: the length (an upper bound where the level of detail runs), before anything touches the device.
extern "C" long long lsnLastMeshTransferFrame(unsigned char *out, long long out_cap)
{
    return lsn::guarded("lsnLastMeshTransferFrame", -1LL, [&]() -> long long {
        lsn::clear_error();
        LastMesh m;
        if (m.resident()) return -1;
        const long long bound = lsnTransferFrameBound(m.nv, m.nt);
        if (!out) return bound;
        if (m.open(bound)) return -1;
        return m.frame(bound, out, out_cap);
    });
}

extern "C" long long lsnLastMeshPly(unsigned char *out, long long out_cap)
{
    return lsn::guarded("lsnLastMeshPly", -1LL, [&]() -> long long {
        lsn::clear_error();
        LastMesh m;
        if (m.resident()) return -1;
        const long long bound = lsnPlyBinaryBytes(m.nv, m.nt);
        if (!out) return bound;
        if (m.open(bound)) return -1;
        return m.ply(bound, false, out, out_cap);
    });
}

// The same two through the level of detail (simplify.hip) with cell size `cell`; out == NULL: the length of the unsimplified mesh, an
// upper bound (fewer vertices and triangles are never longer, except that a mesh that loses every triangle leaves as points).
extern "C" long long lsnLastMeshTransferFrameLod(float cell, unsigned char *out, long long out_cap)
{
    return lsn::guarded("lsnLastMeshTransferFrameLod", -1LL, [&]() -> long long {
        lsn::clear_error();
        LastMesh m;
        if (m.resident()) return -1;
        const long long bound = std::max(lsnTransferFrameBound(m.nv, m.nt), lsnTransferFrameBound(m.nv, 0));
        if (!out) return bound;
        if (m.open(bound) || m.lod("lsnLastMeshTransferFrameLod", cell)) return -1;
        return m.frame(bound, out, out_cap);
    });
}

extern "C" long long lsnLastMeshPlyLod(float cell, unsigned char *out, long long out_cap)
{
    return lsn::guarded("lsnLastMeshPlyLod", -1LL, [&]() -> long long {
        lsn::clear_error();
        LastMesh m;
        if (m.resident()) return -1;
        const long long bound = lsnPlyBinaryBytes(m.nv, m.nt);
        if (!out) return bound;
        if (m.open(bound) || m.lod("lsnLastMeshPlyLod", cell)) return -1;
        return m.ply(bound, false, out, out_cap);
    });
}

// The PLY file of that mesh with vertex normals (normals.hip), after the level-of-detail stage with `cell` (<= 0 or NaN: the mesh as it is).
extern "C" long long lsnLastMeshPlyNormals(float cell, unsigned char *out, long long out_cap)
{
    return lsn::guarded("lsnLastMeshPlyNormals", -1LL, [&]() -> long long {
        lsn::clear_error();
        LastMesh m;
        if (m.resident()) return -1;
        if (m.nt <= 0) {
            lsn::set_error("lsnLastMeshPlyNormals: the resident mesh has no triangles (the normals of a bare point cloud are not defined)");
            return -1;
        }
        const long long bound = lsnPlyNormalsBytes(m.nv, m.nt);
        if (!out) return bound;
        if (m.open(bound) || (cell > 0.0f && m.lod("lsnLastMeshPlyNormals", cell)) || m.normals("lsnLastMeshPlyNormals")) return -1;
        return m.ply(bound, true, out, out_cap);
    });
}

// The outbound formats through the fragment filter (fragments.hip) with `min_vertices`, then the level of detail if cell > 0, then the
// normals if asked: open, fragments, lod, normals, pack.  out == NULL: the length of the unfiltered mesh, an upper bound.  min_vertices
// <= 1 with cell <= 0: the plain exports' bytes.  A resident mesh without triangles is refused when min_vertices > 1 (fragments.hip
// defines no components for a bare point cloud), and always with normals.
extern "C" long long lsnLastMeshTransferFrameFragments(int min_vertices, float cell, unsigned char *out, long long out_cap)
{
    return lsn::guarded("lsnLastMeshTransferFrameFragments", -1LL, [&]() -> long long {
        lsn::clear_error();
        LastMesh m;
        if (m.resident()) return -1;
        const long long bound = std::max(lsnTransferFrameBound(m.nv, m.nt), lsnTransferFrameBound(m.nv, 0));
        if (!out) return bound;
        if (m.open(bound) || m.fragments("lsnLastMeshTransferFrameFragments", min_vertices) ||
            (cell > 0.0f && m.lod("lsnLastMeshTransferFrameFragments", cell)))
            return -1;
        return m.frame(bound, out, out_cap);
    });
}

extern "C" long long lsnLastMeshPlyFragments(int min_vertices, float cell, int with_normals, unsigned char *out, long long out_cap)
{
    return lsn::guarded("lsnLastMeshPlyFragments", -1LL, [&]() -> long long {
        lsn::clear_error();
        LastMesh m;
        if (m.resident()) return -1;
        if (with_normals && m.nt <= 0) {
            lsn::set_error("lsnLastMeshPlyFragments: the resident mesh has no triangles (the normals of a bare point cloud are not defined)");
            return -1;
        }
        const long long bound = with_normals ? lsnPlyNormalsBytes(m.nv, m.nt) : lsnPlyBinaryBytes(m.nv, m.nt);
        if (!out) return bound;
        if (m.open(bound) || m.fragments("lsnLastMeshPlyFragments", min_vertices) || (cell > 0.0f && m.lod("lsnLastMeshPlyFragments", cell)) ||
            (with_normals && m.normals("lsnLastMeshPlyFragments")))
            return -1;
        return m.ply(bound, with_normals != 0, out, out_cap);
    });
}

// The same two with Taubin smoothing (smooth.hip) between the level of detail and the normals: open, fragments, lod, smooth, normals,
// pack.  iterations <= 0: the Fragments exports' bytes; out == NULL: their bound (the stage moves vertices and drops none).  With
// iterations > 0 a resident mesh without triangles is refused, and so is what lsnFusionSmooth refuses.
extern "C" long long lsnLastMeshTransferFrameSmooth(int min_vertices, float cell, int iterations, float lambda, float mu, int pin_boundary,
                                                    unsigned char *out, long long out_cap)
{
    return lsn::guarded("lsnLastMeshTransferFrameSmooth", -1LL, [&]() -> long long {
        lsn::clear_error();
        LastMesh m;
        if (m.resident()) return -1;
        if (iterations > 0 && m.nt <= 0) {
            lsn::set_error("lsnLastMeshTransferFrameSmooth: the resident mesh has no triangles (a bare point cloud has no neighbours to smooth with)");
            return -1;
        }
        const long long bound = std::max(lsnTransferFrameBound(m.nv, m.nt), lsnTransferFrameBound(m.nv, 0));
        if (!out) return bound;
        if (m.open(bound) || m.fragments("lsnLastMeshTransferFrameSmooth", min_vertices) ||
            (cell > 0.0f && m.lod("lsnLastMeshTransferFrameSmooth", cell)) ||
            (iterations > 0 && m.smooth("lsnLastMeshTransferFrameSmooth", iterations, lambda, mu, pin_boundary)))
            return -1;
        return m.frame(bound, out, out_cap);
    });
}

extern "C" long long lsnLastMeshPlySmooth(int min_vertices, float cell, int iterations, float lambda, float mu, int pin_boundary, int with_normals,
                                          unsigned char *out, long long out_cap)
{
    return lsn::guarded("lsnLastMeshPlySmooth", -1LL, [&]() -> long long {
        lsn::clear_error();
        LastMesh m;
        if (m.resident()) return -1;
        if ((with_normals || iterations > 0) && m.nt <= 0) {
            lsn::set_error("lsnLastMeshPlySmooth: the resident mesh has no triangles (%s)", with_normals ? "the normals of a bare point cloud are not defined"
                                                                                                      : "a bare point cloud has no neighbours to smooth with");
            return -1;
        }
        const long long bound = with_normals ? lsnPlyNormalsBytes(m.nv, m.nt) : lsnPlyBinaryBytes(m.nv, m.nt);
        if (!out) return bound;
        if (m.open(bound) || m.fragments("lsnLastMeshPlySmooth", min_vertices) || (cell > 0.0f && m.lod("lsnLastMeshPlySmooth", cell)) ||
            (iterations > 0 && m.smooth("lsnLastMeshPlySmooth", iterations, lambda, mu, pin_boundary)) ||
            (with_normals && m.normals("lsnLastMeshPlySmooth")))
            return -1;
        return m.ply(bound, with_normals != 0, out, out_cap);
    });
}

// One view of that mesh (render.hip) into host arrays.
extern "C" long long lsnLastMeshRenderView(const float *intr7, const float *wt12, int width, int height, int points_only, unsigned char *depth_out,
                                           unsigned char *colors_out)
{
    return lsn::guarded("lsnLastMeshRenderView", -1LL, [&]() -> long long {
        lsn::clear_error();
        if (!intr7 || !wt12 || !depth_out || !colors_out) {
            lsn::set_error("lsnLastMeshRenderView: null argument");
            return -1;
        }
        LastMesh m;
        if (m.resident() || m.open()) return -1;
        return m.render("lsnLastMeshRenderView", intr7, wt12, width, height, points_only != 0, depth_out, colors_out);
    });
}
