// soak_main.cpp -- drives the exports of libNativeUtils' HOST side, built against tests/fake_hip (no GPU) under a sanitizer.
//   1. every export with NULL pointers and zero sizes; random rigs of sensors of different sizes through every host export, the caller's
//      arrays exactly as long as needed; the inbound formats (frame messages, recordings) valid, truncated, with flipped bits and lying headers;
//   2. the call mix of LiveScanServer from four threads at once (MainWindowForm.cs:238,304: updateWorker's merge calls, refineWorker's
//      single-sensor calls + ICP, plus the radial export and all six last-mesh formats), every result checked against what the runtime
//      double's kernels "compute" (every non-zero depth pixel survives, one triangle per vertex);
//   3. the setters of two process-wide switches from four threads at once: every "previous" value handed back is one that was stored;
//   4. the device-resident forms of the two depth stages with state (temporal filter, background subtraction) on a plan and on a tick
//      object: set, learn, run, reset, state / model read and write, diagnostics, on two streams, the tick object from two threads;
//   5. the pool of pinned mesh blocks must be empty at the end.
// $LSN_HOST_DEVICES (read by the library) switches the merge calls to the sharded flow; $LSN_TEST_FAIL_ALLOC / $LSN_TEST_THROW make
// single calls fail, which must leave empty meshes and still an empty pool.  Exit code 0 = all checks held (the sanitizer adds its own).
#include "../../include/NativeUtils.h"

#include <cstddef>
extern "C" int hipMalloc(void **, size_t);   // the runtime double's (fake_hip.cpp); hipSuccess = 0
extern "C" int hipFree(void *);
static int fakeDevMalloc(void **p, size_t n) { return hipMalloc(p, n); }
static int fakeDevFree(void *p) { return hipFree(p); }

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

namespace {

std::atomic<int> g_bad{0};
const bool g_faults = getenv("LSN_TEST_FAIL_ALLOC") || getenv("LSN_TEST_THROW");

#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            fprintf(stderr, "CHECK failed: %s: ", #cond); \
            fprintf(stderr, __VA_ARGS__);         \
            fprintf(stderr, "\n");                \
            g_bad++;                              \
        }                                         \
    } while (0)

struct Rig {
    int n, w, h;
    std::vector<int> widths, heights;
    std::vector<unsigned char> depth, colours;   // the caller's packed arrays (KinectServer.cs:453-498)
    std::vector<float> intr, wt;
    std::vector<int> valid;                       // non-zero depth pixels per sensor
    float b[6] = {-1.5f, -1.0f, -1.5f, 1.5f, 1.5f, 1.5f};
    Rig(int n_, int w_, int h_, unsigned seed) : n(n_), w(w_), h(h_), widths(n_, w_), heights(n_, h_), depth((size_t)n_ * w_ * h_ * 2), colours((size_t)n_ * w_ * h_ * 3),
                                                 intr(7 * n_), wt(12 * n_), valid(n_, 0)
    {
        uint32_t x = seed * 2654435761u + 1;
        unsigned short *d = reinterpret_cast<unsigned short *>(depth.data());
        for (int s = 0; s < n; s++)
            for (int i = 0; i < w * h; i++) {
                x = x * 1664525u + 1013904223u;
                const unsigned short v = (x >> 28) == 0 ? 0 : (unsigned short)(500 + ((x >> 8) % 4000));
                d[(size_t)s * w * h + i] = v;
                valid[s] += v != 0;
            }
        for (size_t i = 0; i < colours.size(); i++) colours[i] = (unsigned char)(i * 7);
        for (int s = 0; s < n; s++) {
            const float in[7] = {(w - 1) * 0.5f, (h - 1) * 0.5f, 365.0f, 365.0f, 0.09f, -0.27f, 0.09f};
            const float tr[12] = {0, 0, -2, 1, 0, 0, 0, 1, 0, 0, 0, 1};
            memcpy(&intr[7 * s], in, sizeof(in));
            memcpy(&wt[12 * s], tr, sizeof(tr));
        }
    }
    // sensors of different sizes; the packed arrays are EXACTLY as long as the sensors need, so a read or a write-back that runs over
    // the end of the caller's arrays (a copy run of the upload schedule cut wrongly, say) is a sanitizer report
    Rig(const std::vector<int> &ws, const std::vector<int> &hs, unsigned seed) : n((int)ws.size()), w(0), h(0), widths(ws), heights(hs), intr(7 * ws.size()),
                                                                                   wt(12 * ws.size()), valid(ws.size(), 0)
    {
        size_t px = 0;
        for (int s = 0; s < n; s++) px += (size_t)widths[s] * heights[s];
        depth.resize(px * 2);
        colours.resize(px * 3);
        uint32_t x = seed * 2654435761u + 1;
        unsigned short *d = reinterpret_cast<unsigned short *>(depth.data());
        size_t at = 0;
        for (int s = 0; s < n; s++) {
            for (int i = 0; i < widths[s] * heights[s]; i++) {
                x = x * 1664525u + 1013904223u;
                const unsigned short v = (x >> 28) == 0 ? 0 : (unsigned short)(500 + ((x >> 8) % 4000));
                d[at++] = v;
                valid[s] += v != 0;
            }
            const float in[7] = {(widths[s] - 1) * 0.5f, (heights[s] - 1) * 0.5f, 365.0f, 365.0f, 0.09f, -0.27f, 0.09f};
            const float tr[12] = {0, 0, -2, 1, 0, 0, 0, 1, 0, 0, 0, 1};
            memcpy(&intr[7 * s], in, sizeof(in));
            memcpy(&wt[12 * s], tr, sizeof(tr));
        }
        for (size_t i = 0; i < colours.size(); i++) colours[i] = (unsigned char)(i * 7);
    }
    int total() const
    {
        int t = 0;
        for (int v : valid) t += v;
        return t;
    }
};

// deleteMesh as a caller that checks would use it: the call nulls the pointers it has released, so pointers that are still there mean the call
// itself did not run -- which only the fault hooks can make happen ($LSN_TEST_THROW hitting deleteMesh's own entry) -- and it is made again.
void release(Mesh &m)
{
    deleteMesh(&m);
    if (m.vertices) deleteMesh(&m);
}

bool failed_call(const Mesh &m)   // a call that a fault hook hit: empty mesh + a message
{
    char msg[256];
    return g_faults && m.nVertices == 0 && lsnGetLastError(msg, sizeof(msg)) > 0;
}

bool mesh_gone()   // a last-mesh call that found nothing: the radial thread's calls reuse the merge lane's buffers, which forgets its mesh
{
    char msg[256];
    return lsnGetLastError(msg, sizeof(msg)) > 0 && strstr(msg, "no mesh is resident");
}

void check_mesh(const Mesh &m, int want_v, bool triangles, const char *what)
{
    if (failed_call(m)) return;
    CHECK(m.nVertices == want_v, "%s: %d vertices, expected %d", what, m.nVertices, want_v);
    CHECK(m.nTriangles == (triangles ? want_v : 0), "%s: %d triangles, expected %d", what, m.nTriangles, triangles ? want_v : 0);
    CHECK(m.triangles != nullptr, "%s: null triangle pointer", what);
    // every byte the call promises is readable (ASan) and carries what the double's kernels wrote: A = 255, indices inside the cloud
    long long bad = 0;
    for (int i = 0; i < m.nVertices; i++) bad += m.vertices[i].A != 255;
    for (int i = 0; i < 3 * m.nTriangles; i++) bad += m.triangles[i] < 0 || m.triangles[i] >= m.nVertices;
    CHECK(bad == 0, "%s: %lld bad vertices / indices", what, bad);
}

void merge_thread(int iters)
{
    Rig rig(8, 512, 424, 1), small(3, 250, 121, 2);
    for (int it = 0; it < iters; it++) {
        Mesh m;
        memset(&m, 0, sizeof(m));
        generateMeshFromDepthMaps(rig.n, rig.depth.data(), rig.colours.data(), rig.widths.data(), rig.heights.data(), rig.intr.data(), rig.wt.data(), &m, false,
                                  rig.b[0], rig.b[1], rig.b[2], rig.b[3], rig.b[4], rig.b[5], false);
        check_mesh(m, rig.total(), true, "merge 8x512x424");
        release(m);
        generateMeshFromDepthMaps(small.n, small.depth.data(), small.colours.data(), small.widths.data(), small.heights.data(), small.intr.data(),
                                  small.wt.data(), &m, false, small.b[0], small.b[1], small.b[2], small.b[3], small.b[4], small.b[5], false);
        check_mesh(m, small.total(), true, "merge 3x250x121");
        const long long bound = lsnLastMeshTransferFrame(nullptr, 0);   // whichever lane finished last: the TransferServer stream of its mesh
        if (bound > 0) {
            std::vector<unsigned char> frame((size_t)bound);
            (void)lsnLastMeshTransferFrame(frame.data(), bound);
        }
        // the other outbound formats of that mesh, one after the other on the steps they share (the offset rows, the stages' scratch, the
        // packers' buffer).  The level of detail, the normals and the renderer are not emulated: their counts read back as 0 and the packers
        // see an empty mesh, so what runs here is the steps' host side -- reserves, the rows' copies, the order of the locks
        auto packed = [](const char *what, long long need, auto &&call) {
            if (need <= 0) return;
            std::vector<unsigned char> out((size_t)need);
            const long long n = call(out.data(), need);
            CHECK(g_faults || (n >= 0 && n <= need) || mesh_gone(), "%s: %lld bytes of at most %lld", what, n, need);
        };
        packed("lsnLastMeshPly", lsnLastMeshPly(nullptr, 0), [](unsigned char *o, long long n) { return lsnLastMeshPly(o, n); });
        packed("lsnLastMeshPlyNormals", lsnLastMeshPlyNormals(0.05f, nullptr, 0), [](unsigned char *o, long long n) { return lsnLastMeshPlyNormals(0.05f, o, n); });
        {
            std::vector<unsigned char> view_d(2 * 64 * 48), view_c(3 * 64 * 48);
            const long long px = lsnLastMeshRenderView(small.intr.data(), small.wt.data(), 64, 48, it & 1, view_d.data(), view_c.data());
            CHECK(g_faults || px == 0 || mesh_gone(), "lsnLastMeshRenderView: %lld pixels", px);
        }
        packed("lsnLastMeshTransferFrameLod", lsnLastMeshTransferFrameLod(0.2f, nullptr, 0), [](unsigned char *o, long long n) { return lsnLastMeshTransferFrameLod(0.2f, o, n); });
        packed("lsnLastMeshPlyNormals, no level of detail", lsnLastMeshPlyNormals(0.0f, nullptr, 0), [](unsigned char *o, long long n) { return lsnLastMeshPlyNormals(0.0f, o, n); });
        packed("lsnLastMeshPlyLod", lsnLastMeshPlyLod(0.05f, nullptr, 0), [](unsigned char *o, long long n) { return lsnLastMeshPlyLod(0.05f, o, n); });
        release(m);
        // the same rig with bcolor_transfer: the flow that keeps the whole cloud in HBM, and the colour transfer's scratch on the plan (its
        // kernels are no-ops on the double and it only changes colour bytes on a device, so the same mesh is expected)
        generateMeshFromDepthMaps(small.n, small.depth.data(), small.colours.data(), small.widths.data(), small.heights.data(), small.intr.data(),
                                  small.wt.data(), &m, true, small.b[0], small.b[1], small.b[2], small.b[3], small.b[4], small.b[5], false);
        check_mesh(m, small.total(), true, "merge 3x250x121, colour transfer");
        release(m);
        // the tick as one call: the radial kernels are not emulated, the corrected maps read as zeros -> an empty cloud, through every copy
        // and event of the flow; the caller's arrays are overwritten with the (zero) corrected maps, so they are copies
        std::vector<unsigned char> d2 = rig.depth, c2 = rig.colours;
        lsnCorrectAndGenerateMesh(rig.n, d2.data(), c2.data(), rig.widths.data(), rig.heights.data(), rig.intr.data(), rig.wt.data(), &m, rig.b[0], rig.b[1],
                                  rig.b[2], rig.b[3], rig.b[4], rig.b[5], it & 1);
        check_mesh(m, 0, false, "tick as one call");
        release(m);
    }
}

void single_thread(int iters)
{
    Rig rig(8, 512, 424, 3);
    for (int it = 0; it < iters; it++)
        for (int s = 0; s < rig.n; s++) {
            Mesh m;
            memset(&m, 0, sizeof(m));
            generateVerticesFromDepthMap(rig.depth.data(), rig.colours.data(), rig.widths.data(), rig.heights.data(), rig.intr.data(), rig.wt.data(), &m, rig.b[0],
                                         rig.b[1], rig.b[2], rig.b[3], rig.b[4], rig.b[5], s);
            check_mesh(m, rig.valid[s], false, "single sensor");
            release(m);
        }
}

void radial_thread(int iters)
{
    Rig rig(8, 512, 424, 4);
    for (int it = 0; it < iters; it++) {
        std::vector<unsigned char> d2 = rig.depth, c2 = rig.colours;
        depthMapAndColorSetRadialCorrection(rig.n, d2.data(), c2.data(), rig.widths.data(), rig.heights.data(), rig.intr.data());
    }
}

void icp_thread(int iters)
{
    const int n1 = 5000, n2 = 3000;
    std::vector<Point3f> a(n1), b(n2);
    for (int i = 0; i < n1; i++) a[i] = {0.001f * i, 0.002f * (i % 97), 0.5f};
    for (int i = 0; i < n2; i++) b[i] = {0.0015f * i, 0.002f * (i % 89), 0.51f};
    for (int it = 0; it < iters; it++) {
        float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
        const float r = ICP(a.data(), b.data(), n1, n2, R, t, 3);
        CHECK(r == 1.0f, "ICP returned %f", r);
    }
}

// lsnSetTemporalFilter and lsnSetDepthSmooth, two threads each, every thread alternating between two triples and putting back what it was
// handed.  A setter exchanges under one acquisition of its switch's lock, so whatever it hands back -- the raw numbers of an "off"
// request included -- is a triple some call stored: one of `known` (the initial value first, which main reads before the threads start).
// (A guard, not a reproduction: two setters that were handed the same previous value still hand back known ones.)
template <class B>
struct Triple {
    int a;
    B b, c;
    bool operator==(const Triple &o) const { return a == o.a && b == o.b && c == o.c; }
};

template <class B>
void setter_thread(int (*set)(int, B, B, int *, B *, B *), const char *what, const Triple<B> *known, int first, int rounds)
{
    for (int r = 0; r < rounds; r++) {
        const Triple<B> &mine = known[1 + ((first + r) & 1)];
        Triple<B> prev = {-12345, (B)-1, (B)-1};
        if (set(mine.a, mine.b, mine.c, &prev.a, &prev.b, &prev.c)) {   // refused: only a fault hook can do that, and prev stays untouched
            CHECK(g_faults && prev.a == -12345, "%s refused a valid triple", what);
            continue;
        }
        CHECK(prev == known[0] || prev == known[1] || prev == known[2], "%s handed back (%d, %g, %g), which nobody stored", what, prev.a, (double)prev.b, (double)prev.c);
        CHECK(set(prev.a, prev.b, prev.c, nullptr, nullptr, nullptr) == 0 || g_faults, "%s refused the triple it had handed back", what);
    }
}

// Behind the call mix, not beside it: the switches are process-wide, and calls that found them on or off by chance would pass a number of
// allocation fault points that depends on the scheduling.  The initial values are put back at the end.
void setter_race(int rounds)
{
    Triple<int> tp[3] = {{0, 0, 0}, {64, 20, 2}, {128, 30, 1}};
    Triple<float> ds[3] = {{0, 0.0f, 0.0f}, {1, 1.0f, 10.0f}, {2, 1.5f, 12.0f}};
    const bool read = lsnSetTemporalFilter(tp[1].a, tp[1].b, tp[1].c, &tp[0].a, &tp[0].b, &tp[0].c) == 0 &&
                      lsnSetTemporalFilter(tp[0].a, tp[0].b, tp[0].c, nullptr, nullptr, nullptr) == 0 &&
                      lsnSetDepthSmooth(ds[1].a, ds[1].b, ds[1].c, &ds[0].a, &ds[0].b, &ds[0].c) == 0 &&
                      lsnSetDepthSmooth(ds[0].a, ds[0].b, ds[0].c, nullptr, nullptr, nullptr) == 0;
    CHECK(read || g_faults, "the switches' initial values");
    if (!read) return;
    std::vector<std::thread> th;
    for (int k = 0; k < 2; k++) {
        th.emplace_back(setter_thread<int>, lsnSetTemporalFilter, "lsnSetTemporalFilter", tp, k, rounds);
        th.emplace_back(setter_thread<float>, lsnSetDepthSmooth, "lsnSetDepthSmooth", ds, k, rounds);
    }
    for (auto &t : th) t.join();
    // each switch holds one of the values that were set; then the initial ones again
    Triple<int> t_end = {-1, -1, -1};
    Triple<float> d_end = {-1, -1.0f, -1.0f};
    const bool put = lsnSetTemporalFilter(tp[0].a, tp[0].b, tp[0].c, &t_end.a, &t_end.b, &t_end.c) == 0 &&
                     lsnSetDepthSmooth(ds[0].a, ds[0].b, ds[0].c, &d_end.a, &d_end.b, &d_end.c) == 0;
    CHECK(g_faults || (put && (t_end == tp[0] || t_end == tp[1] || t_end == tp[2]) && (d_end == ds[0] || d_end == ds[1] || d_end == ds[2])),
          "the switches ended at (%d, %d, %d) and (%d, %g, %g)", t_end.a, t_end.b, t_end.c, d_end.a, (double)d_end.b, (double)d_end.c);
}

void null_sweep()
{
    Mesh m;
    memset(&m, 0, sizeof(m));
    generateMeshFromDepthMaps(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &m, false, 0, 0, 0, 0, 0, 0, false);
    generateMeshFromDepthMaps(4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &m, false, 0, 0, 0, 0, 0, 0, false);
    generateMeshFromDepthMaps(4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, false, 0, 0, 0, 0, 0, 0, false);
    generateVerticesFromDepthMap(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &m, 0, 0, 0, 0, 0, 0, 0);
    generateVerticesFromDepthMap(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, 0, -1);
    depthMapAndColorSetRadialCorrection(0, nullptr, nullptr, nullptr, nullptr, nullptr);
    depthMapAndColorSetRadialCorrection(2, nullptr, nullptr, nullptr, nullptr, nullptr);
    lsnCorrectAndGenerateMesh(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &m, 0, 0, 0, 0, 0, 0, 1);
    lsnCorrectAndGenerateMesh(3, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, 0, 1);
    CHECK(m.nVertices == 0 && m.nTriangles == 0, "a refused call left a mesh behind");
    deleteMesh(nullptr);
    deleteMesh(&m);
    deleteMesh(&m);
    float R[9] = {0}, t[3] = {0};
    CHECK(ICP(nullptr, nullptr, 0, 0, R, t, 10) == 1.0f, "ICP(null)");
    CHECK(ICP(nullptr, nullptr, 5, 5, nullptr, nullptr, 0) == 1.0f, "ICP(null, 5)");
    (void)lsnLastMeshTransferFrame(nullptr, 0);
    (void)lsnLastMeshPly(nullptr, 0);
    (void)lsnLastMeshTransferFrameLod(0.05f, nullptr, 0);
    (void)lsnLastMeshPlyLod(0.05f, nullptr, 0);
    (void)lsnLastMeshPlyNormals(0.05f, nullptr, 0);
    CHECK(lsnLastMeshRenderView(nullptr, nullptr, 0, 0, 0, nullptr, nullptr) == -1, "lsnLastMeshRenderView(null)");
    char buf[64];
    CHECK(lsnHostScheduleDescribe(0, nullptr, nullptr, 0, 0, 0, 0, buf, sizeof(buf)) == -1, "schedule(null)");
    CHECK(lsnHostShardDescribe(0, 0, nullptr, buf, sizeof(buf)) == -1, "shards(0)");
    CHECK(lsnFusionCreate(0, 0, 0, nullptr, nullptr) == nullptr, "lsnFusionCreate(0)");
    lsnFusionDestroy(nullptr);
    CHECK(lsnFusionRun(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == -1, "lsnFusionRun(null)");
    CHECK(lsnFusionRunMesh(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == -1, "lsnFusionRunMesh(null)");
    // (device memory for the device-resident call below comes straight from the runtime double: this file includes no HIP header)
    // the chained tick as one call: NULL handles and arguments, then a real two-half pipeline on the double (two plans, side stream, fork / join):
    // what it allocates and enqueues is checked by the sanitizers and by the double's device discipline
    CHECK(lsnTickCreate(0, 0, 0, nullptr, nullptr) == nullptr, "lsnTickCreate(0)");
    lsnTickDestroy(nullptr);
    CHECK(lsnTickRun(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == -1, "lsnTickRun(null)");
    CHECK(lsnTickSetParams(nullptr, nullptr, nullptr, nullptr, nullptr) == -1, "lsnTickSetParams(null)");
    CHECK(lsnTickCapacity(nullptr) == 0 && lsnTickTriangleCapacity(nullptr) == 0 && lsnTickParts(nullptr) == 0, "lsnTick getters(null)");
    {
        const int T = 9, n = 2, w[2] = {64, 24}, h[2] = {48, 16};
        LsnTick *tk = lsnTickCreate(0, T, n, w, h);
        CHECK(g_faults || (tk != nullptr && lsnTickParts(tk) == 2), "lsnTickCreate");   // (a fault hook may hit any of its allocations: then it returns NULL)
        if (tk) {
            const long long cap = lsnTickCapacity(tk), tcap = lsnTickTriangleCapacity(tk);
            CHECK(cap == 64 * 48 + 24 * 16 && tcap == 2 * cap, "lsnTick capacities");
            float intr[14], wt[24], bounds[6] = {-2, -2, -2, 2, 2, 2};
            for (int i = 0; i < n; i++) {
                const float k[7] = {w[i] / 2.0f, h[i] / 2.0f, 365.0f * w[i] / 512.0f, 365.0f * w[i] / 512.0f, 0.09f, -0.05f, 0.01f};
                memcpy(intr + 7 * i, k, sizeof(k));
                const float p[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
                memcpy(wt + 12 * i, p, sizeof(p));
            }
            void *d_in = nullptr, *c_in = nullptr, *d_co = nullptr, *c_co = nullptr, *v = nullptr, *tr = nullptr;
            int *o = nullptr, *to = nullptr;
            CHECK(lsnTickRun(tk, &d_in, &c_in, &d_co, &c_co, &v, o, &tr, to, nullptr) == -1, "lsnTickRun before lsnTickSetParams / with null tables");
            const bool set = lsnTickSetParams(tk, intr, wt, bounds, nullptr) == 0;
            CHECK(g_faults || set, "lsnTickSetParams");
            bool ok = fakeDevMalloc(&d_in, 2 * cap * T)== 0 && fakeDevMalloc(&c_in, 3 * cap * T)== 0 && fakeDevMalloc(&d_co, 2 * cap * T)== 0 &&
                      fakeDevMalloc(&c_co, 3 * cap * T)== 0 && fakeDevMalloc(&v, 16 * cap * T)== 0 && fakeDevMalloc(&tr, 12 * tcap * T)== 0 &&
                      fakeDevMalloc((void **)&o, sizeof(int) * (n + 1) * T)== 0 && fakeDevMalloc((void **)&to, sizeof(int) * (n + 1) * T)== 0;
            CHECK(g_faults || ok, "device buffers for lsnTickRun");
            if (ok && set)
                for (int rep = 0; rep < 2; rep++) {
                    char why[256] = "";
                    const int rc = lsnTickRun(tk, d_in, c_in, d_co, c_co, v, o, tr, to, nullptr);
                    if (rc) (void)lsnGetLastError(why, sizeof(why));
                    CHECK(g_faults || rc == 0, "lsnTickRun: %s", why);
                }
            for (void *q : {d_in, c_in, d_co, c_co, v, tr, (void *)o, (void *)to}) (void)fakeDevFree(q);
            lsnTickDestroy(tk);
        }
    }
    Mesh *heap = createMesh();
    CHECK(heap && heap->nVertices == 0 && heap->vertices == nullptr, "createMesh");
    deleteMesh(heap);
    free(heap);
}

// The exports of the multi-GPU exchange step (exchange.hip, shard.hip) with NULL handles and arguments: each must refuse with its failure
// value -- and a message, where it sets one -- before it touches RCCL.  (lsnShardRcclPath and lsnShardRanksSeen load RCCL before they look
// at their arguments: they are not called, no real RCCL is mapped into a sanitizer process.)
void exchange_null_sweep()
{
    auto refused = [](bool failed, const char *what) {
        char msg[256] = "";
        CHECK(failed && lsnGetLastError(msg, sizeof(msg)) > 0, "%s: %s", what, failed ? "no message" : "did not fail");
    };
    refused(lsnFusionPackSurvivors(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == -1, "lsnFusionPackSurvivors(null)");
    refused(lsnFusionPackSurvivorsRun(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == -1,
            "lsnFusionPackSurvivorsRun(null)");
    refused(lsnFusionReconstruct(nullptr, 0, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == -1, "lsnFusionReconstruct(null)");
    refused(lsnFusionReconstructRun(nullptr, 0, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == -1,
            "lsnFusionReconstructRun(null)");
    refused(lsnMergeShards(0, 0, 0, 0, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr) == -1, "lsnMergeShards(0)");
    CHECK(lsnShardUniqueId(nullptr) == -1, "lsnShardUniqueId(null)");
    refused(lsnShardPrepare(0, 0, 0, 0, 0, nullptr, nullptr) == nullptr, "lsnShardPrepare(world 0)");
    refused(lsnShardConnect(nullptr, nullptr) == -1, "lsnShardConnect(null)");
    refused(lsnShardCreate(0, 0, 1, nullptr, 1, 1, nullptr, nullptr) == nullptr, "lsnShardCreate(null id)");
    refused(lsnShardSetParams(nullptr, nullptr, nullptr, nullptr, nullptr) == -1, "lsnShardSetParams(null)");
    refused(lsnShardStep(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == -1, "lsnShardStep(null)");
    lsnShardDestroy(nullptr);
    CHECK(lsnShardPlan(nullptr, 0) == nullptr && lsnShardPlan(nullptr, 1) == nullptr, "lsnShardPlan(null)");
    CHECK(lsnShardMergedCapacity(nullptr) == 0 && lsnShardLastBytesSent(nullptr) == 0 && lsnFusionTilesPerTick(nullptr) == 0, "lsnShard getters(null)");
}

}  // namespace

// Random rigs of 1-8 sensors of different sizes (1 x 1 up to ~0.9 MB of colours each: below and above the size at which the upload
// schedule cuts a call into groups and merges short copy runs) through every host export, one after the other on this thread.
void ragged_rigs(int n_rigs)
{
    uint32_t x = 12345;
    auto rnd = [&](int lo, int hi) {
        x = x * 1664525u + 1013904223u;
        return lo + (int)((x >> 8) % (uint32_t)(hi - lo + 1));
    };
    for (int r = 0; r < n_rigs; r++) {
        const int n = rnd(1, 8);
        std::vector<int> ws, hs;
        for (int s = 0; s < n; s++) {
            const int kind = rnd(0, 3);
            ws.push_back(kind == 0 ? rnd(1, 12) : kind == 1 ? 8 * rnd(1, 80) + rnd(-1, 1) : rnd(200, 640));
            hs.push_back(kind == 0 ? rnd(1, 9) : kind == 1 ? rnd(1, 60) : rnd(100, 480));
        }
        Rig rig(ws, hs, 100 + r);
        char what[96];
        snprintf(what, sizeof(what), "ragged rig %d (%d sensors)", r, n);
        Mesh m;
        generateMeshFromDepthMaps(rig.n, rig.depth.data(), rig.colours.data(), rig.widths.data(), rig.heights.data(), rig.intr.data(), rig.wt.data(), &m, false,
                                  rig.b[0], rig.b[1], rig.b[2], rig.b[3], rig.b[4], rig.b[5], false);
        check_mesh(m, rig.total(), true, what);
        release(m);
        const int one = rnd(0, n - 1);
        generateVerticesFromDepthMap(rig.depth.data(), rig.colours.data(), rig.widths.data(), rig.heights.data(), rig.intr.data(), rig.wt.data(), &m, rig.b[0],
                                     rig.b[1], rig.b[2], rig.b[3], rig.b[4], rig.b[5], one);
        check_mesh(m, rig.valid[one], false, what);
        release(m);
        {
            std::vector<unsigned char> d2 = rig.depth, c2 = rig.colours;   // exact-size copies: the export writes the corrected maps back into them
            depthMapAndColorSetRadialCorrection(rig.n, d2.data(), c2.data(), rig.widths.data(), rig.heights.data(), rig.intr.data());
        }
        for (int back = 0; back < 2; back++) {
            std::vector<unsigned char> d2 = rig.depth, c2 = rig.colours;
            lsnCorrectAndGenerateMesh(rig.n, d2.data(), c2.data(), rig.widths.data(), rig.heights.data(), rig.intr.data(), rig.wt.data(), &m, rig.b[0], rig.b[1],
                                      rig.b[2], rig.b[3], rig.b[4], rig.b[5], back);
            if (!failed_call(m)) CHECK(m.nVertices >= 0 && m.triangles != nullptr, "%s: tick as one call", what);
            release(m);
        }
    }
}

// The inbound formats are what arrives from the network and from disk: valid messages, then the same messages truncated, with bytes
// flipped and with headers that lie about sizes, from buffers exactly as long as what is handed over.  Nothing may read or write outside
// them (the sanitizers watch), and every answer is either a sensible length or -1.
void parser_fuzz(int rounds)
{
    uint32_t x = 777;
    auto rnd = [&](uint32_t n) {
        x = x * 1664525u + 1013904223u;
        return (x >> 8) % n;
    };
    for (int r = 0; r < rounds; r++) {
        const int w = 1 + (int)rnd(40), h = 1 + (int)rnd(30), nb = (int)rnd(3);
        // body block (liveScanClient.cpp:233-268): i32 count, then per body one flag byte, i32 joints, 28 bytes per joint
        const int nj = 2;
        std::vector<unsigned char> depth((size_t)w * h * 2), rgb((size_t)w * h * 3), bodies(4 + (size_t)nb * (5 + 28 * nj), 0);
        for (auto &b : depth) b = (unsigned char)rnd(256);
        for (auto &b : rgb) b = (unsigned char)rnd(256);
        memcpy(bodies.data(), &nb, 4);
        for (int k = 0; k < nb; k++) memcpy(bodies.data() + 4 + (size_t)k * (5 + 28 * nj) + 1, &nj, 4);
        const int level = (lsnZstdAvailable() && (r & 1)) ? 3 : 0;
        std::vector<unsigned char> msg(16 + depth.size() + rgb.size() + bodies.size() + 1024);
        const long long len = lsnFrameEncode(depth.data(), rgb.data(), w, h, bodies.data(), (int)bodies.size(), level, msg.data(), (long long)msg.size());
        CHECK(len > 16, "lsnFrameEncode %dx%d level %d: %lld", w, h, level, len);
        if (len <= 16) continue;
        msg.resize((size_t)len);
        for (int variant = 0; variant < 12; variant++) {
            std::vector<unsigned char> m = msg;                       // exact size: the sanitizer sees any byte read past it
            if (variant >= 1 && variant <= 4) m.resize(16 + rnd((uint32_t)(m.size() - 16)));            // truncated payload
            if (variant >= 5 && variant <= 8)
                for (int k = 0; k < 1 + (int)rnd(8); k++) m[rnd((uint32_t)m.size())] ^= (unsigned char)(1u << rnd(8));   // flipped bits, header included
            if (variant >= 9) {                                                                           // a header that lies
                int lie = variant == 9 ? 0x7FFFFFFF : variant == 10 ? -5 : (int)rnd(1u << 20);
                memcpy(m.data() + 4 * rnd(4), &lie, 4);
            }
            LsnFrameInfo info;
            const int rc = lsnFrameParseHeader(m.data(), &info);
            if (rc != 0) continue;
            if (info.width <= 0 || info.height <= 0 || (long long)info.width * info.height > (1 << 22)) continue;   // a caller sizes its buffers from these
            const size_t px = (size_t)info.width * info.height;
            std::vector<unsigned char> d_out(px * 2), c_out(px * 3), b_out(256);
            int n_bodies = -1;
            const int have = (int)m.size() - 16;
            const long long got = lsnFrameDecode(m.data() + 16, std::min(have, info.payload_bytes), info.compressed, info.width, info.height, d_out.data(), c_out.data(),
                                                 b_out.data(), (int)b_out.size(), &n_bodies);
            CHECK(got == -1 || got >= 4, "lsnFrameDecode returned %lld", got);
            if (variant == 0)
                CHECK(got == (long long)bodies.size() && d_out == depth && c_out == rgb, "round trip of a %dx%d frame (level %d): body block %lld of %zu, depth %d, colours %d", w,
                      h, level, got, bodies.size(), (int)(d_out == depth), (int)(c_out == rgb));
        }
        // a recording of three such frames, then cut and damaged
        std::vector<unsigned char> file(3 * (msg.size() + 96));
        long long at = 0;
        for (int k = 0; k < 3; k++) {
            const long long wrote = lsnRecordingAppend(file.data() + at, (long long)file.size() - at, msg.data(), (int)msg.size(), 1000 * k);
            CHECK(wrote > (long long)msg.size(), "lsnRecordingAppend");
            if (wrote > 0) at += wrote;
        }
        file.resize((size_t)at);
        for (int variant = 0; variant < 6; variant++) {
            std::vector<unsigned char> f = file;
            if (variant == 1 || variant == 2) f.resize(rnd((uint32_t)f.size()));
            if (variant >= 3)
                for (int k = 0; k < 1 + (int)rnd(6); k++) f[rnd((uint32_t)f.size())] = (unsigned char)rnd(256);
            long long pos = 0;
            int frames = 0;
            while (pos >= 0 && pos < (long long)f.size() && frames < 16) {
                long long off = 0;
                int flen = 0, ts = 0;
                const long long next = lsnRecordingNext(f.data(), (long long)f.size(), pos, &off, &flen, &ts);
                if (next < 0) break;
                CHECK(next > pos && off >= 0 && flen >= 0 && off + flen <= (long long)f.size(), "lsnRecordingNext: record [%lld, +%d) in a file of %zu", off, flen, f.size());
                pos = next;
                frames++;
            }
            if (variant == 0) CHECK(frames == 3, "a recording of three frames read back %d", frames);
        }
    }
}

// The device-resident exports of the fused pass on the double, one call after the other on this thread: every launch form a plan can take
// (lsnFusionSetMode 0 / 1 / 2, with and without the triangulation, pipelined, streamed) on a multi-tick plan of 8-pixel-aligned sensors
// and on a one-tick plan with a ragged one (the general-width kernels and map).  The double emulates the count, scan, write and
// single-pass kernels, so where only those run the vertex totals are checked; the look-back-per-run kernel and the streamed write +
// count are no-ops there and only have to be enqueued without an error.
void fusion_forms(int T, const int *w, const int *h)
{
    const int n = 2;
    char what[64];
    snprintf(what, sizeof(what), "fusion forms (%d tick(s), %dx%d + %dx%d)", T, w[0], h[0], w[1], h[1]);
    LsnFusion *p = lsnFusionCreate(0, T, n, w, h);
    CHECK(g_faults || p != nullptr, "%s: lsnFusionCreate", what);
    if (!p) return;
    const long long cap = lsnFusionTickCapacity(p), tcap = lsnFusionTickTriangleCapacity(p);
    CHECK(cap == (long long)w[0] * h[0] + (long long)w[1] * h[1] && tcap == 2 * cap, "%s: capacities", what);
    float intr[14], wt[24], bounds[6] = {-2, -2, -2, 2, 2, 2};
    for (int i = 0; i < n; i++) {
        const float k[7] = {w[i] / 2.0f, h[i] / 2.0f, 365.0f * w[i] / 512.0f, 365.0f * w[i] / 512.0f, 0.09f, -0.05f, 0.01f};
        memcpy(intr + 7 * i, k, sizeof(k));
        const float q[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
        memcpy(wt + 12 * i, q, sizeof(q));
    }
    void *d[3] = {nullptr, nullptr, nullptr}, *c = nullptr, *v = nullptr, *tr = nullptr;
    int *o = nullptr, *to = nullptr;
    bool ok = fakeDevMalloc(&d[0], 2 * cap * T) == 0 && fakeDevMalloc(&d[1], 2 * cap * T) == 0 && fakeDevMalloc(&d[2], 2 * cap * T) == 0 &&
              fakeDevMalloc(&c, 3 * cap * T) == 0 && fakeDevMalloc(&v, 16 * cap * T) == 0 && fakeDevMalloc(&tr, 12 * tcap * T) == 0 &&
              fakeDevMalloc((void **)&o, sizeof(int) * (n + 1) * T) == 0 && fakeDevMalloc((void **)&to, sizeof(int) * (n + 1) * T) == 0;
    CHECK(g_faults || ok, "%s: device buffers", what);
    CHECK(!ok || lsnFusionRun(p, d[0], c, v, o, nullptr) == -1, "%s: lsnFusionRun before lsnFusionSetParams", what);
    const bool set = lsnFusionSetParams(p, intr, wt, bounds, nullptr) == 0;
    CHECK(g_faults || set, "%s: lsnFusionSetParams", what);
    if (ok && set) {
        // the double's "device" memory is the host's: three batches of depth, every seventh pixel without a measurement
        std::vector<int> want(T, 0);
        for (int b = 0; b < 3; b++) {
            unsigned short *dep = static_cast<unsigned short *>(d[b]);
            for (long long i = 0; i < cap * T; i++) dep[i] = (i + b) % 7 == 0 ? 0 : (unsigned short)(600 + i % 900);
        }
        for (int t = 0; t < T; t++)
            for (long long i = cap * t; i < cap * (t + 1); i++) want[t] += i % 7 != 0;
        auto call = [&](int rc, bool counted, const char *which) {
            char why[256] = "";
            if (rc) (void)lsnGetLastError(why, sizeof(why));
            CHECK(g_faults || rc == 0, "%s: %s: %s", what, which, why);
            if (rc || !counted) return;
            for (int t = 0; t < T; t++) CHECK(o[t * (n + 1) + n] == want[t], "%s: %s: tick %d has %d vertices, expected %d", what, which, t, o[t * (n + 1) + n], want[t]);
        };
        for (int mode = 0; mode < 3; mode++) {
            CHECK(lsnFusionSetMode(p, mode) == 0 || g_faults, "%s: lsnFusionSetMode(%d)", what, mode);
            for (int rep = 0; rep < 2; rep++) {   // (the second run with unchanged parameters builds the depth thresholds)
                call(lsnFusionRun(p, d[0], c, v, o, nullptr), mode != 1, "lsnFusionRun");
                call(lsnFusionRunMesh(p, d[0], c, v, o, tr, to, nullptr), true, "lsnFusionRunMesh");
                for (int t = 0; t < T && !g_faults; t++)
                    CHECK(to[t * (n + 1) + n] == want[t], "%s: lsnFusionRunMesh: tick %d has %d triangles, expected %d", what, t, to[t * (n + 1) + n], want[t]);
            }
        }
        CHECK(lsnFusionSetMode(p, 3) == -1, "%s: lsnFusionSetMode(3)", what);
        CHECK(lsnFusionSetMode(p, 0) == 0 || g_faults, "%s: lsnFusionSetMode(0)", what);
        const bool piped = lsnFusionSetPipelined(p, 1) == 0;
        CHECK(g_faults || piped, "%s: lsnFusionSetPipelined(1)", what);
        if (piped)
            for (int rep = 0; rep < 3; rep++) call(lsnFusionRun(p, d[0], c, v, o, nullptr), true, "lsnFusionRun, pipelined");
        CHECK(lsnFusionSetPipelined(p, 0) == 0 || g_faults, "%s: lsnFusionSetPipelined(0)", what);
        call(lsnFusionRun(p, d[0], c, v, o, nullptr), true, "lsnFusionRun after the pipelined calls");
        // streamed: batch 0 counted now and batch 1 ahead, batch 1 from the counts made ahead (the double makes none: nothing to check),
        // then batch 2, which nobody counted ahead
        call(lsnFusionRunStreamed(p, d[0], c, v, o, d[1], nullptr), true, "lsnFusionRunStreamed with a next batch");
        call(lsnFusionRunStreamed(p, d[1], c, v, o, nullptr, nullptr), false, "lsnFusionRunStreamed without one");
        call(lsnFusionRunStreamed(p, d[2], c, v, o, nullptr, nullptr), false, "lsnFusionRunStreamed, not counted ahead");
        CHECK(lsnFusionRunStreamed(p, nullptr, c, v, o, nullptr, nullptr) == -1, "%s: lsnFusionRunStreamed(null)", what);
    }
    for (void *q : {d[0], d[1], d[2], c, v, tr, (void *)o, (void *)to}) (void)fakeDevFree(q);
    lsnFusionDestroy(p);
}

// The device-resident forms of the two stages with state (temporal.hip, background.hip) on the double: each export once with NULL
// arguments; then on a plan and on a tick object set, learn, run, reset, state / model read and write and diagnostics, on two streams, the
// tick object from two threads at once.  The stages' kernels are launch stubs there, so a state that was written reads back as it was and
// every count is 0: what is checked is what the host side reserves, copies and hands over from stream to stream, and that a call a fault
// hook hits fails with -1 and leaves everything usable.
void stateful_stages()
{
    auto refused = [](int rc, const char *what) { CHECK(rc == -1, "%s: returned %d", what, rc); };
    auto works = [](int rc, const char *what) {
        char why[256] = "";
        if (rc) (void)lsnGetLastError(why, sizeof(why));
        CHECK(g_faults || rc == 0, "%s: %s", what, why);
        return rc == 0;
    };
    unsigned int word = 0;
    unsigned short value = 0;
    int cnt = 0;
    refused(lsnFusionSetTemporal(nullptr, 64, 20, 2), "lsnFusionSetTemporal(null)");
    refused(lsnFusionTemporal(nullptr, nullptr, nullptr, nullptr), "lsnFusionTemporal(null)");
    refused(lsnFusionTemporalReset(nullptr, nullptr), "lsnFusionTemporalReset(null)");
    refused(lsnFusionTemporalStateRead(nullptr, &word, nullptr), "lsnFusionTemporalStateRead(null)");
    refused(lsnFusionTemporalStateWrite(nullptr, &word, nullptr), "lsnFusionTemporalStateWrite(null)");
    refused(lsnFusionTemporalDiagnostics(nullptr, 0, &cnt, &cnt, &cnt, &cnt, nullptr), "lsnFusionTemporalDiagnostics(null)");
    refused(lsnFusionSetBackground(nullptr, 40, 8, 64), "lsnFusionSetBackground(null)");
    refused(lsnFusionBackgroundLearn(nullptr, nullptr, nullptr), "lsnFusionBackgroundLearn(null)");
    refused(lsnFusionBackground(nullptr, nullptr, nullptr, nullptr), "lsnFusionBackground(null)");
    refused(lsnFusionBackgroundReset(nullptr, nullptr), "lsnFusionBackgroundReset(null)");
    refused(lsnFusionBackgroundModelRead(nullptr, &value, nullptr), "lsnFusionBackgroundModelRead(null)");
    refused(lsnFusionBackgroundModelWrite(nullptr, &value, nullptr), "lsnFusionBackgroundModelWrite(null)");
    refused(lsnFusionBackgroundDiagnostics(nullptr, 0, &cnt, &cnt, &cnt, &cnt, &cnt, &cnt, nullptr), "lsnFusionBackgroundDiagnostics(null)");
    refused(lsnTickSetTemporal(nullptr, 64, 20, 2), "lsnTickSetTemporal(null)");
    refused(lsnTickTemporalReset(nullptr, nullptr), "lsnTickTemporalReset(null)");
    refused(lsnTickSetBackground(nullptr, 40, 8, 64), "lsnTickSetBackground(null)");
    refused(lsnTickBackgroundLearn(nullptr, nullptr, nullptr), "lsnTickBackgroundLearn(null)");
    refused(lsnTickBackgroundReset(nullptr, nullptr), "lsnTickBackgroundReset(null)");

    const int n = 2, w[2] = {136, 128}, h[2] = {40, 16};   // a tile edge in x and in y, one width that is no multiple of 128
    void *s1 = lsnStreamCreate(0), *s2 = lsnStreamCreate(0);
    CHECK(g_faults || (s1 && s2), "lsnStreamCreate");
    // ---- a plan ----
    const int T = 3;
    LsnFusion *p = s1 && s2 ? lsnFusionCreate(0, T, n, w, h) : nullptr;
    CHECK(g_faults || p != nullptr, "stateful stages: lsnFusionCreate");
    if (p) {
        const long long cap = lsnFusionTickCapacity(p);
        void *d_in = nullptr, *d_out = nullptr;
        const bool bufs = fakeDevMalloc(&d_in, 2 * cap * T + 16) == 0 && fakeDevMalloc(&d_out, 2 * cap * T) == 0;
        CHECK(g_faults || bufs, "stateful stages: device buffers");
        std::vector<unsigned int> st((size_t)cap), st2((size_t)cap, 7u);
        std::vector<unsigned short> md((size_t)cap), md2((size_t)cap, 7);
        std::vector<int> c(6 * n, -1);
        auto counts_zero = [&](int fields, const char *what) {
            for (int i = 0; i < fields * n; i++) CHECK(c[i] == 0, "%s: count %d is %d", what, i, c[i]);
        };
        for (size_t i = 0; i < st.size(); i++) st[i] = i % 5 == 0 ? 0u : (unsigned int)(256 * (500 + i % 3000)) | (unsigned int)(i % 3) << 24;
        for (size_t i = 0; i < md.size(); i++) md[i] = (unsigned short)(i % 7 == 0 ? 0 : 400 + i % 5000);
        // the temporal filter
        if (!g_faults) refused(lsnFusionTemporalDiagnostics(p, 0, c.data(), c.data() + n, c.data() + 2 * n, c.data() + 3 * n, s1), "lsnFusionTemporalDiagnostics before a call");
        if (works(lsnFusionTemporalStateRead(p, st2.data(), s1), "lsnFusionTemporalStateRead before a history"))
            for (unsigned int v : st2) CHECK(v == 0, "no history read as %u", v);
        works(lsnFusionTemporalReset(p, s2), "lsnFusionTemporalReset before a history");
        refused(lsnFusionSetTemporal(p, 300, 20, 2), "lsnFusionSetTemporal(300)");
        works(lsnFusionSetTemporal(p, 64, 20, 2), "lsnFusionSetTemporal");
        if (bufs) {
            works(lsnFusionTemporal(p, d_in, d_out, s1), "lsnFusionTemporal");
            works(lsnFusionTemporal(p, d_in, d_in, s2), "lsnFusionTemporal in place, on the other stream");
            refused(lsnFusionTemporal(p, d_in, static_cast<char *>(d_in) + 16, s1), "lsnFusionTemporal on overlapping maps");
            if (works(lsnFusionTemporalDiagnostics(p, T - 1, c.data(), c.data() + n, c.data() + 2 * n, c.data() + 3 * n, s1), "lsnFusionTemporalDiagnostics"))
                counts_zero(4, "lsnFusionTemporalDiagnostics");
        }
        st2[3] = 5u << 24;   // a miss count without history
        refused(lsnFusionTemporalStateWrite(p, st2.data(), s2), "lsnFusionTemporalStateWrite of a word that is no state");
        if (works(lsnFusionTemporalStateWrite(p, st.data(), s2), "lsnFusionTemporalStateWrite") &&
            works(lsnFusionTemporalStateRead(p, st2.data(), s1), "lsnFusionTemporalStateRead"))
            CHECK(st2 == st, "the history read back differs from what was written");
        if (works(lsnFusionTemporalReset(p, s2), "lsnFusionTemporalReset") && bufs && works(lsnFusionTemporal(p, d_in, d_out, s1), "lsnFusionTemporal behind a reset") &&
            works(lsnFusionTemporalStateRead(p, st2.data(), nullptr), "lsnFusionTemporalStateRead behind a reset"))
            for (unsigned int v : st2) CHECK(v == 0, "a reset history read as %u", v);
        works(lsnFusionSetTemporal(p, 0, 0, 0), "lsnFusionSetTemporal(off)");
        if (bufs && works(lsnFusionTemporal(p, d_in, d_out, s1), "lsnFusionTemporal, off") &&
            works(lsnFusionTemporalDiagnostics(p, 0, c.data(), nullptr, nullptr, c.data() + 3 * n, s2), "lsnFusionTemporalDiagnostics behind a copy"))
            CHECK(c[0] == 0 && c[3 * n] == 0, "lsnFusionTemporalDiagnostics behind a copy");
        // background subtraction
        if (!g_faults) refused(lsnFusionBackgroundDiagnostics(p, 0, c.data(), nullptr, nullptr, nullptr, nullptr, nullptr, s1), "lsnFusionBackgroundDiagnostics before a call");
        if (works(lsnFusionBackgroundModelRead(p, md2.data(), s1), "lsnFusionBackgroundModelRead before a model"))
            for (unsigned short v : md2) CHECK(v == 0, "no model read as %u", v);
        works(lsnFusionBackgroundReset(p, s2), "lsnFusionBackgroundReset before a model");
        refused(lsnFusionSetBackground(p, 5000, 0, 0), "lsnFusionSetBackground(5000)");
        works(lsnFusionSetBackground(p, 40, 8, 64), "lsnFusionSetBackground");
        if (bufs) {
            works(lsnFusionBackgroundLearn(p, d_in, s1), "lsnFusionBackgroundLearn");
            works(lsnFusionBackground(p, d_in, d_out, s2), "lsnFusionBackground, on the other stream");
            works(lsnFusionBackground(p, d_in, d_in, s1), "lsnFusionBackground in place");
            refused(lsnFusionBackground(p, d_in, static_cast<char *>(d_in) + 16, s1), "lsnFusionBackground on overlapping maps");
            if (works(lsnFusionBackgroundDiagnostics(p, T - 1, c.data(), c.data() + n, c.data() + 2 * n, c.data() + 3 * n, c.data() + 4 * n, c.data() + 5 * n, s2),
                      "lsnFusionBackgroundDiagnostics"))
                counts_zero(6, "lsnFusionBackgroundDiagnostics");
        }
        if (works(lsnFusionBackgroundModelWrite(p, md.data(), s2), "lsnFusionBackgroundModelWrite") &&
            works(lsnFusionBackgroundModelRead(p, md2.data(), s1), "lsnFusionBackgroundModelRead"))
            CHECK(md2 == md, "the model read back differs from what was written");
        if (works(lsnFusionBackgroundReset(p, s2), "lsnFusionBackgroundReset") && bufs && works(lsnFusionBackground(p, d_in, d_out, s1), "lsnFusionBackground behind a reset") &&
            works(lsnFusionBackgroundModelRead(p, md2.data(), nullptr), "lsnFusionBackgroundModelRead behind a reset"))
            for (unsigned short v : md2) CHECK(v == 0, "a reset model read as %u", v);
        works(lsnFusionSetBackground(p, 0, 0, 0), "lsnFusionSetBackground(off)");
        if (bufs) works(lsnFusionBackground(p, d_in, d_out, s1), "lsnFusionBackground, off");
        (void)fakeDevFree(d_in);
        (void)fakeDevFree(d_out);
        lsnFusionDestroy(p);
    }
    // ---- a tick object, two threads, each on its own stream ----
    const int TT = 9;
    LsnTick *tk = s1 && s2 ? lsnTickCreate(0, TT, n, w, h) : nullptr;
    CHECK(g_faults || tk != nullptr, "stateful stages: lsnTickCreate");
    if (tk) {
        const long long cap = lsnTickCapacity(tk), tcap = lsnTickTriangleCapacity(tk);
        float intr[14], wt[24], bounds[6] = {-2, -2, -2, 2, 2, 2};
        for (int i = 0; i < n; i++) {
            const float k[7] = {w[i] / 2.0f, h[i] / 2.0f, 365.0f * w[i] / 512.0f, 365.0f * w[i] / 512.0f, 0.09f, -0.05f, 0.01f};
            memcpy(intr + 7 * i, k, sizeof(k));
            const float q[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
            memcpy(wt + 12 * i, q, sizeof(q));
        }
        void *d_in = nullptr, *c_in = nullptr, *d_co = nullptr, *c_co = nullptr, *v = nullptr, *tr = nullptr;
        int *o = nullptr, *to = nullptr;
        const bool bufs = fakeDevMalloc(&d_in, 2 * cap * TT) == 0 && fakeDevMalloc(&c_in, 3 * cap * TT) == 0 && fakeDevMalloc(&d_co, 2 * cap * TT) == 0 &&
                          fakeDevMalloc(&c_co, 3 * cap * TT) == 0 && fakeDevMalloc(&v, 16 * cap * TT) == 0 && fakeDevMalloc(&tr, 12 * tcap * TT) == 0 &&
                          fakeDevMalloc((void **)&o, sizeof(int) * (n + 1) * TT) == 0 && fakeDevMalloc((void **)&to, sizeof(int) * (n + 1) * TT) == 0;
        CHECK(g_faults || bufs, "stateful stages: device buffers for the tick object");
        const bool set = works(lsnTickSetParams(tk, intr, wt, bounds, nullptr), "lsnTickSetParams");
        refused(lsnTickSetTemporal(tk, 64, 5000, 2), "lsnTickSetTemporal(delta 5000)");
        refused(lsnTickSetBackground(tk, 40, 300, 64), "lsnTickSetBackground(rel_q 300)");
        works(lsnTickTemporalReset(tk, s1), "lsnTickTemporalReset before a history");
        works(lsnTickBackgroundReset(tk, s2), "lsnTickBackgroundReset before a model");
        works(lsnTickSetTemporal(tk, 64, 20, 2), "lsnTickSetTemporal");
        works(lsnTickSetBackground(tk, 40, 8, 64), "lsnTickSetBackground");
        if (bufs && set) {
            auto worker = [&](void *s) {   // (the tick object's lock orders the calls; the runs write the shared outputs under it)
                for (int rep = 0; rep < 3; rep++) {
                    works(lsnTickBackgroundLearn(tk, d_in, s), "lsnTickBackgroundLearn");
                    works(lsnTickRun(tk, d_in, c_in, d_co, c_co, v, o, tr, to, s), "lsnTickRun with both stages");
                    works(lsnTickTemporalReset(tk, s), "lsnTickTemporalReset");
                    works(lsnTickBackgroundReset(tk, s), "lsnTickBackgroundReset");
                    works(lsnTickRun(tk, d_in, c_in, d_co, c_co, v, o, tr, to, s), "lsnTickRun behind the resets");
                }
            };
            std::thread a(worker, s1), b(worker, s2);
            a.join();
            b.join();
        }
        works(lsnTickSetTemporal(tk, 0, 0, 0), "lsnTickSetTemporal(off)");
        works(lsnTickSetBackground(tk, 0, 0, 0), "lsnTickSetBackground(off)");
        for (void *q : {d_in, c_in, d_co, c_co, v, tr, (void *)o, (void *)to}) (void)fakeDevFree(q);
        lsnTickDestroy(tk);
    }
    if (s1) (void)lsnStreamDestroy(0, s1);
    if (s2) (void)lsnStreamDestroy(0, s2);
}

int main(int argc, char **argv)
{
    const int iters = argc > 1 ? atoi(argv[1]) : 4;
    null_sweep();
    exchange_null_sweep();
    stateful_stages();
    ragged_rigs(3 * iters);
    parser_fuzz(20 * iters);
    {
        // (behind everything else this thread does alone: the fault hooks count allocations and guarded entries from the start)
        const int w_even[2] = {64, 24}, h_even[2] = {48, 16}, w_ragged[2] = {64, 20}, h_ragged[2] = {48, 16};
        fusion_forms(3, w_even, h_even);
        fusion_forms(1, w_ragged, h_ragged);
    }
    {
        std::vector<std::thread> th;
        th.emplace_back(merge_thread, iters);
        th.emplace_back(single_thread, iters);
        th.emplace_back(radial_thread, iters);
        th.emplace_back(icp_thread, iters);
        for (auto &t : th) t.join();
    }
    setter_race(200 * iters);
    int live = -1, pooled = -1;
    long long bytes = -1;
    CHECK(lsnHostPoolStats(&live, &pooled, &bytes) == 0, "lsnHostPoolStats");
    CHECK(live == 0 && bytes == 0, "%d pinned block(s) (%lld bytes) never came back to the pool", live, bytes);
    char shards[256] = {0};
    const int D = lsnHostShardDescribe(8, 0, nullptr, shards, sizeof(shards));
    printf("soak: %d iteration(s) per thread, merge calls over %d device part(s) [%s], pool %d live / %d pooled, fault points %lld, %d check(s) failed\n", iters, D,
           shards, live, pooled, lsnTestFaultPoints(1), g_bad.load());
    return g_bad.load() ? 1 : 0;
}
