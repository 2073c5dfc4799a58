// color_blend.hip -- colour blending across views: lsnFusionColorBlend, lsnFusionColorBlendDiagnostics and what the exports run while
// lsnSetColorBlend is on.
//
// No reference: the stage is DEFINED (tests/color_blend_ref.py is the definition in numpy).  The colour transfer
// (color.hip) maps a whole sensor's colours with one affine transform; what it leaves is the local difference along the line where one
// sensor's surface ends and the next begins.  The blend feathers it: the colour of vertex g of sensor j becomes the weighted mean of its
// own colour and of the colours every other sensor saw at the same surface point, each weighted with its pixel's confidence level
// (cloud_index.hip: 1 + the distance to the sensor's depth edge, capped at 20) -- in integers, so that nothing depends on an order:
//
//   own term       weight conf_j[pixel of g], colour C_in[g]; always takes part
//   partner i != j (x, y, d1) = project(sensor i, X, Y, Z); takes part iff (x, y) lies in i's frame, d1 != 0, d2 = depth_i[y, x] > 0,
//                  |d1 - d2| < depth_tol, v = pix2v_i[y, x] >= 0 and w = conf_i[y, x] >= min_confidence: weight w, colour C_in[v]
//   result         per channel floor((sum w c + floor(W / 2)) / W), W = sum w (at most 32 * 20 * 255 in the numerator: 32-bit integers);
//                  a vertex without a partner keeps its bytes; A, X, Y, Z never change
//
// C_in is every vertex's colour as it is when the call starts: cb_snapshot_kernel packs the colour dwords into plan scratch (4 bytes a
// vertex), cb_blend_kernel gathers partners' colours from there and writes the colour dword of its own vertex in place.  Without the
// snapshot a lane could read a colour another lane has already blended (a Gauss-Seidel sweep whose result depends on the schedule);
// with it the in-place write cannot be observed, and a gather moves a 4-byte record instead of a 16-byte one.
// Bounds: a lane reads its own vertex g < min(offsets[n], capacity), its pixel only when it lies in its sensor's frame, a partner's
// pixel only after the frame test, and a partner's colour only for 0 <= v < the tick's vertex count.
// Compiled as part of mesh.hip's translation unit (the include at its end, behind color.hip and mesh_batch.hip: it uses cloud_index.hip's
// index, projection and sensor_of, and mesh_batch.hip's plan_export), not on its own.
#include "fusion_shared.hpp"

#include <algorithm>

namespace {

constexpr int kCbMaxMaps = 32;     // the largest sum, 32 * 20 * 255, and the LDS counter table are sized by it
constexpr int kCbThreads = 256;
constexpr int kCbCounters = 3;     // per (tick, sensor): vertices with a partner, partner terms, sum over R, G, B of |new - old|

struct CbArgs {
    const FrameDesc *frames;
    const SensorParams *params;
    const unsigned short *depth;
    const int *offsets;            // [n_ticks][n+1]: the caller's table
    const int *pix2v, *v2pix;      // [n_ticks][pixels per tick], [n_ticks][vertices per tick]
    const unsigned char *conf;     // [n_ticks][pixels per tick]
    uint4 *verts;                  // [n_ticks][vertices per tick]
    unsigned int *snap;            // [n_ticks][vertices per tick]: the colour dwords as the call found them
    unsigned long long *diag;      // [n_ticks][n][kCbCounters]
    int n, depth_tol, min_conf;
    long long tick_pix, tick_vert;
};

// The vertices of a tick the stage touches: the caller's total, clipped to the tick's capacity.
__device__ __forceinline__ int cb_count(const CbArgs &a, const int *off)
{
    return (int)min((long long)max(off[a.n], 0), a.tick_vert);
}

__global__ __launch_bounds__(kCbThreads) void cb_snapshot_kernel(CbArgs a)
{
    const int tick = blockIdx.y;
    const int g = blockIdx.x * kCbThreads + threadIdx.x;
    if (g >= cb_count(a, a.offsets + tick * (a.n + 1))) return;
    a.snap[tick * a.tick_vert + g] = a.verts[tick * a.tick_vert + g].x;
}

__global__ __launch_bounds__(kCbThreads) void cb_blend_kernel(CbArgs a)
{
    __shared__ unsigned int s_diag[kCbMaxMaps * kCbCounters];
    const int tick = blockIdx.y, n = a.n;
    for (int i = threadIdx.x; i < n * kCbCounters; i += kCbThreads) s_diag[i] = 0;
    __syncthreads();
    const int *off = a.offsets + tick * (n + 1);
    const int nv = cb_count(a, off);
    const int g = blockIdx.x * kCbThreads + threadIdx.x;
    const bool active = g < nv;
    int j = 0, partners = 0, change = 0;
    if (active) {
        j = sensor_of(off, n, g);
        const int pj = a.v2pix[tick * a.tick_vert + g];
        const FrameDesc fj = a.frames[j];
        // (pj is in the frame whenever the offsets belong to these depth maps; the test keeps a mismatched call in bounds)
        if ((unsigned int)pj < (unsigned int)fj.npix) {
            const long long pix0 = tick * a.tick_pix;
            const unsigned int *snap = a.snap + tick * a.tick_vert;
            uint4 *vp = a.verts + tick * a.tick_vert + g;
            const uint4 v = *vp;
            const float X = __uint_as_float(v.y), Y = __uint_as_float(v.z), Z = __uint_as_float(v.w);
            int W = a.conf[pix0 + fj.depth_off + pj];
            int s0 = W * (int)(v.x & 255u), s1 = W * (int)((v.x >> 8) & 255u), s2 = W * (int)((v.x >> 16) & 255u);
            // sensor i's record is indexed by the loop counter: wave-uniform, scalar loads
            for (int i = 0; i < n; i++) {
                const FrameDesc fi = a.frames[i];
                int x, y, d1;
                project(a.params[i], X, Y, Z, x, y, d1);
                if (i == j || x < 0 || x >= fi.w || y < 0 || y >= fi.h || d1 == 0) continue;
                const long long q = pix0 + fi.depth_off + (long long)y * fi.w + x;
                // the three gathers of this partner are issued before any of them is tested: the four conditions are combined
                // without a short circuit, so that no load can sink behind a branch on another one's value
                const int d2 = a.depth[q];
                const int w = a.conf[q];
                const int u = a.pix2v[q];
                // u < 0: depth but no vertex (the crop removed it); u >= nv only when the offsets do not belong to these maps
                const int ok = (int)(d2 > 0) & (int)(abs(d1 - d2) < a.depth_tol) & (int)(w >= a.min_conf) & (int)((unsigned int)u < (unsigned int)nv);
                if (ok) {
                    const unsigned int c = snap[u];
                    W += w;
                    s0 += w * (int)(c & 255u);
                    s1 += w * (int)((c >> 8) & 255u);
                    s2 += w * (int)((c >> 16) & 255u);
                    partners++;
                }
            }
            if (partners) {   // W >= min_conf >= 1
                const unsigned int uw = (unsigned int)W, half = uw >> 1;
                const unsigned int r0 = ((unsigned int)s0 + half) / uw, r1 = ((unsigned int)s1 + half) / uw, r2 = ((unsigned int)s2 + half) / uw;
                change = abs((int)r0 - (int)(v.x & 255u)) + abs((int)r1 - (int)((v.x >> 8) & 255u)) + abs((int)r2 - (int)((v.x >> 16) & 255u));
                vp->x = (v.x & 0xFF000000u) | r0 | (r1 << 8) | (r2 << 16);
            }
        }
    }
    // the counters: per wave one sum per sensor met in it (one sensor, but for the waves a sensor boundary runs through), LDS adds per
    // workgroup, then one global atomic per non-zero entry
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(partners > 0);
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const int sj = __shfl(j, lead, 64);
        const bool mine = partners > 0 && j == sj;
        const int b = wave_sum(mine ? 1 : 0), t = wave_sum(mine ? partners : 0), c = wave_sum(mine ? change : 0);
        if (lane == lead) {
            atomicAdd(&s_diag[sj * kCbCounters], (unsigned int)b);
            atomicAdd(&s_diag[sj * kCbCounters + 1], (unsigned int)t);
            if (c) atomicAdd(&s_diag[sj * kCbCounters + 2], (unsigned int)c);
        }
        todo &= ~__ballot(mine);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n * kCbCounters; i += kCbThreads)
        if (s_diag[i]) atomicAdd(&a.diag[(long long)tick * n * kCbCounters + i], (unsigned long long)s_diag[i]);
}

}  // namespace

namespace lsn {

// The blend on `s` over all ticks of the plan; d_vertices / d_offsets as lsnFusionRun left them.  Plan mutex held, the plan's device current.
static int color_blend_locked(LsnFusion *p, int depth_tol, int min_confidence, const void *d_depth, void *d_vertices, const int *d_offsets,
                              hipStream_t s)
{
    if (!d_depth || !d_vertices || !d_offsets) {
        lsn::set_error("lsnFusionColorBlend: null argument");
        return -1;
    }
    if (!p->params_set) {
        lsn::set_error("lsnFusionColorBlend: lsnFusionSetParams has not been called");
        return -1;
    }
    const int n = p->n_maps, T = p->n_ticks;
    if (n > kCbMaxMaps) {
        lsn::set_error("lsnFusionColorBlend: at most %d sensors (the plan has %d)", kCbMaxMaps, n);
        return -1;
    }
    // the counters are this call's, also when it changes nothing
    const size_t diag_bytes = sizeof(unsigned long long) * kCbCounters * (size_t)n * T;
    if (p->cb_diag.reserve(diag_bytes)) return -1;
    LSN_HIP(hipMemsetAsync(p->cb_diag.p, 0, diag_bytes, s));
    p->cb_ready = true;
    if (depth_tol <= 0 || min_confidence > 20 || n == 1) return 0;   // off; one sensor has no partner
    if (p->cb_snap.reserve(sizeof(unsigned int) * (size_t)p->cap * T)) return -1;
    // pixel <-> vertex maps and confidence
    if (cloud_index_locked(p, d_depth, d_vertices, true, s)) return -1;
    CbArgs a;
    a.frames = p->frames.as<FrameDesc>();
    a.params = p->params.as<SensorParams>();
    a.depth = static_cast<const unsigned short *>(d_depth);
    a.offsets = d_offsets;
    a.pix2v = p->ix_pix2v.as<int>();
    a.v2pix = p->ix_v2pix.as<int>();
    a.conf = p->ix_conf.as<unsigned char>();
    a.verts = static_cast<uint4 *>(d_vertices);
    a.snap = p->cb_snap.as<unsigned int>();
    a.diag = p->cb_diag.as<unsigned long long>();
    a.n = n;
    a.depth_tol = depth_tol;
    a.min_conf = std::max(min_confidence, 1);
    a.tick_pix = p->tick_depth_elems;
    a.tick_vert = p->cap;
    const dim3 grid((unsigned int)((p->cap + kCbThreads - 1) / kCbThreads), T);
    hipLaunchKernelGGL(cb_snapshot_kernel, grid, dim3(kCbThreads), 0, s, a);
    hipLaunchKernelGGL(cb_blend_kernel, grid, dim3(kCbThreads), 0, s, a);
    LSN_HIP(hipGetLastError());
    return 0;
}

int color_blend(LsnFusion *p, int depth_tol, int min_confidence, const void *d_depth, void *d_vertices, const int *d_offsets, hipStream_t s)
{
    if (!p) {
        lsn::set_error("lsnFusionColorBlend: null argument");
        return -1;
    }
    std::lock_guard<std::mutex> g(p->mu);
    LSN_HIP(hipSetDevice(p->device));
    return color_blend_locked(p, depth_tol, min_confidence, d_depth, d_vertices, d_offsets, s);
}

}  // namespace lsn

extern "C" int lsnFusionColorBlend(LsnFusion *p, int depth_tol, int min_confidence, const void *d_depth_maps, void *d_vertices,
                                   const int *d_offsets, void *stream)
{
    return plan_export("lsnFusionColorBlend", p, [&] {
        return lsn::color_blend_locked(p, depth_tol, min_confidence, d_depth_maps, d_vertices, d_offsets, lsn::as_stream(stream));
    });
}

extern "C" int lsnFusionColorBlendDiagnostics(LsnFusion *p, int tick, int *blended_per_sensor, long long *partners_per_sensor,
                                              long long *abs_change_per_sensor, void *stream)
{
    return plan_export("lsnFusionColorBlendDiagnostics", p, [&] {
        if (tick < 0 || tick >= p->n_ticks) {
            lsn::set_error("lsnFusionColorBlendDiagnostics: the plan has %d ticks (asked for tick %d)", p->n_ticks, tick);
            return -1;
        }
        if (!p->cb_ready) {
            lsn::set_error("lsnFusionColorBlendDiagnostics: no colour blend has run on this plan");
            return -1;
        }
        hipStream_t s = lsn::as_stream(stream);
        const int n = p->n_maps;
        std::vector<unsigned long long> c((size_t)n * kCbCounters);
        LSN_HIP(hipMemcpyAsync(c.data(), p->cb_diag.as<unsigned long long>() + (size_t)tick * n * kCbCounters, sizeof(unsigned long long) * c.size(),
                               hipMemcpyDeviceToHost, s));
        LSN_HIP(hipStreamSynchronize(s));
        long long total = 0;
        for (int i = 0; i < n; i++) {
            if (blended_per_sensor) blended_per_sensor[i] = (int)c[(size_t)i * kCbCounters];
            if (partners_per_sensor) partners_per_sensor[i] = (long long)c[(size_t)i * kCbCounters + 1];
            if (abs_change_per_sensor) abs_change_per_sensor[i] = (long long)c[(size_t)i * kCbCounters + 2];
            total += (long long)c[(size_t)i * kCbCounters];
        }
        return (int)total;
    });
}
