// cloud_index.hip -- what the three post-fusion stages (color.hip, merge.hip, outlier.hip) share: the cloud index of a plan and the device
// helpers that go with it.
//
// The cloud index of a set of depth maps is what the reference keeps beside every sensor's vertices while it generates them: the pixel of
// every vertex (vertices_to_depth_map), the vertex of every pixel (depth_to_vertices_map, -1 = none) and, for the stages that weigh
// pixels, the confidence maps (generateVerticesConfidence, src/NativeUtils/depthprocessing.cpp:285-398).  The fusion keeps none of them,
// so every stage starts by deriving them from the depth maps it was handed (cloud_index_locked, at the end of this file):
//
//   * index pass (ct_index_kernel<0>, scan_kernel, ct_index_kernel<1>): the fusion's own keep predicate, re-evaluated per tile, gives
//     every pixel its vertex (index inside the tick's cloud) and every vertex its pixel.  Same arithmetic as the write pass, so the same
//     vertex order.
//   * confidence (ct_conf_kernel), for the stages that ask: generateMapConfidence on every sensor's full depth map, 32x32 pixels per
//     workgroup with a 20-pixel halo in LDS; the level-synchronous BFS runs inside the workgroup (18 sweeps at most).  A pixel's level is
//     1 + its BFS distance from the seeds, capped at 20: only paths of <= 19 steps matter and they stay inside the halo, so the tile
//     result is exact.
//
// The plan holds ONE set of index buffers (LsnFusion::ix_*).  Every stage rebuilds them from its own input -- in a call with the outlier
// filter on, the filter indexes the unmasked maps and the stages behind it the masked ones -- so what the buffers hold is the index of
// the last stage that ran on the plan.
// Also here: the conversions and the projection that more than one stage evaluates (cvt_i32_x64, project, sensor_of) and the block scan
// of per-workgroup counts (ct_block_scan_kernel).
// Compiled as part of mesh.hip's translation unit (the include at its end, ahead of the three stages), not on its own.
#include "fusion_shared.hpp"

#include <vector>

namespace {

constexpr int kConfTile = 32;        // output pixels per side of a confidence tile
constexpr int kConfHalo = 20;        // et_limit: a level depends on pixels up to 20 away (19 steps + the seed test's neighbour)
constexpr int kConfSide = kConfTile + 2 * kConfHalo;
constexpr int kConfLimit = 20;       // et_limit (:392)
constexpr int kDepthThreshold = 20;  // depth_threshold (:393); calculateMapsCoverage / getColorCorrectionTransform (:1401, :1442)

// (int)v of a double as x64 code computes it (cvttsd2si): truncation toward zero, INT_MIN for NaN and for anything out of range.
__device__ __forceinline__ int cvt_i32_x64(double v)
{
    return (v > -2147483649.0 && v < 2147483648.0) ? (int)v : (int)0x80000000u;
}

// pointProjection (:735-747) with the inverted world transform of sensor i (WorldTranformation::inv, depthprocessing.h:65-75:
// R -> R^T, t -> -t; rotate first, then add t).  Float arithmetic in the reference's order; the "+ 0.5" is a double add.
__device__ __forceinline__ void project(const SensorParams &P, float X, float Y, float Z, int &x, int &y, int &d)
{
    float tx = X * P.r00 + Y * P.r10 + Z * P.r20;
    float ty = X * P.r01 + Y * P.r11 + Z * P.r21;
    float tz = X * P.r02 + Y * P.r12 + Z * P.r22;
    tx += -P.t0;
    ty += -P.t1;
    tz += -P.t2;
    x = cvt_i32_x64((double)((tx * P.fx) / tz + P.cx) + 0.5);
    y = cvt_i32_x64((double)(P.cy - (ty * P.fy) / tz) + 0.5);
    d = min(max(0, cvt_i32_x64((double)(tz * 1000.0f))), 65535);
}

// Sensor of vertex g of a tick: the last sensor whose first vertex is <= g (offsets [n+1], g < offsets[n]).
__device__ __forceinline__ int sensor_of(const int *off, int n, int g)
{
    int s = 0;
    for (int k = 1; k < n; k++) s = off[k] <= g ? k : s;
    return s;
}

// ---- index pass ------------------------------------------------------------------------------------------------------------------
// MAP = 0: survivors per tile into counts; MAP = 1 (after scan_kernel turned them into exclusive prefixes inside the tick): the two maps.
template <int MAP>
__global__ __launch_bounds__(kThreads) void ct_index_kernel(FuseArgs a, int *counts, int *pix2v, int *v2pix)
{
    __shared__ int s_wave[kThreads / 64];
    const int tile = blockIdx.x, tick = blockIdx.y;
    const Tile t = locate(a, tick, tile);
    Inputs in;
    load_inputs<false, false>(t, in);
    bool keep[kPxPerLane];
    uint4 vert[kPxPerLane];
    compute_tile<false, false>(a, t, in, keep, vert);
    int below, wave_total;
    rank_from_masks(keep, below, wave_total);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_wave[wave] = wave_total;
    __syncthreads();
    int pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; w++) {
        pre += w < wave ? s_wave[w] : 0;
        tot += s_wave[w];
    }
    const long long lin = (long long)tick * a.tiles_per_tick + tile;
    if (!MAP) {
        if (threadIdx.x == 0) counts[lin] = tot;
        return;
    }
    int r = counts[lin] + pre + below;   // the lane's first vertex inside the tick
    const int p0 = t.px0 + threadIdx.x * kPxPerLane;
    int *pm = pix2v + tick * a.tick_depth_stride + t.pix_base;
    int *vm = v2pix + tick * a.tick_vert_stride;
#pragma unroll
    for (int k = 0; k < kPxPerLane; k++) {
        if (p0 + k < t.npix) {
            pm[p0 + k] = keep[k] ? r : -1;
            if (keep[k]) vm[r] = p0 + k;   // the pixel inside the sensor's frame
        }
        r += keep[k] ? 1 : 0;
    }
}

// ---- confidence ------------------------------------------------------------------------------------------------------------------
// LDS codes besides the levels 0..19: kFree = not reached yet (may be reached), kFixed = keeps 20 (x == 0 or y == 0, or a zero depth on
// the border), kOut = outside the frame.
constexpr unsigned char kFree = 255, kFixed = 254, kOut = 253;

__global__ __launch_bounds__(256) void ct_conf_kernel(const FrameDesc *frames, const int *ctile, int n_maps, const unsigned short *depth,
                                                     long long tick_pix, unsigned char *conf)
{
    __shared__ unsigned short s_d[kConfSide * kConfSide];
    __shared__ unsigned char s_c[kConfSide * kConfSide];
    const int tick = blockIdx.y;
    int f = 0;
    for (int k = 1; k < n_maps; k++) f = ctile[k] <= (int)blockIdx.x ? k : f;
    const FrameDesc fd = frames[f];
    const int w = fd.w, h = fd.h;
    const int tiles_x = (w + kConfTile - 1) / kConfTile;
    const int ti = (int)blockIdx.x - ctile[f];
    const int ox = (ti % tiles_x) * kConfTile - kConfHalo, oy = (ti / tiles_x) * kConfTile - kConfHalo;
    const unsigned short *dm = depth + tick * tick_pix + fd.depth_off;
    for (int i = threadIdx.x; i < kConfSide * kConfSide; i += blockDim.x) {
        const int x = ox + i % kConfSide, y = oy + i / kConfSide;
        const bool in = x >= 0 && y >= 0 && x < w && y < h;
        s_d[i] = in ? dm[(long long)y * w + x] : 0;
    }
    __syncthreads();
    // seeds (:309-337): interior pixels only; the "wall" test reads the neighbour at (x + shift_x, y + shift_x) -- the reference's row
    // offset uses shift_x too (:320), so its 8 probes are (-1,-1), (0,0) and (1,1), repeated
    for (int i = threadIdx.x; i < kConfSide * kConfSide; i += blockDim.x) {
        const int lx = i % kConfSide, ly = i / kConfSide;
        const int x = ox + lx, y = oy + ly;
        unsigned char c;
        if (x < 0 || y < 0 || x >= w || y >= h) {
            c = kOut;
        } else {
            const int d = s_d[i];
            const bool interior = x >= 1 && y >= 1 && x < w - 1 && y < h - 1;
            if (interior && d == 0) {
                c = 0;
            } else if (interior && lx >= 1 && ly >= 1 && lx < kConfSide - 1 && ly < kConfSide - 1) {
                const int a = s_d[i - kConfSide - 1], b = s_d[i + kConfSide + 1];
                c = (abs(d - a) > kDepthThreshold || a == 0 || abs(d - b) > kDepthThreshold || b == 0) ? 1 : kFree;
            } else if (interior) {
                c = kFree;   // on the halo's rim: its seed test needs pixels outside, and nothing it could change reaches the tile
            } else {
                // the border: never a seed; x == 0 / y == 0 are never visited (:356), x == w-1 / y == h-1 may be reached (d != 0)
                c = (x >= 1 && y >= 1 && d != 0) ? kFree : kFixed;
            }
        }
        s_c[i] = c;
    }
    __syncthreads();
    // level k -> k + 1 (:341-377): a free pixel next to a level-k pixel whose depth differs from its own by less than 20
    for (int k = 1; k < kConfLimit - 1; k++) {
        int changed = 0;
        for (int i = threadIdx.x; i < kConfSide * kConfSide; i += blockDim.x) {
            if (s_c[i] != kFree) continue;
            const int lx = i % kConfSide, ly = i / kConfSide;
            const int d = s_d[i];
            bool hit = false;
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    const int nx = lx + dx, ny = ly + dy;
                    if ((dx | dy) == 0 || nx < 0 || ny < 0 || nx >= kConfSide || ny >= kConfSide) continue;
                    const int j = ny * kConfSide + nx;
                    hit |= s_c[j] == k && abs((int)s_d[j] - d) < kDepthThreshold;
                }
            if (hit) {
                s_c[i] = (unsigned char)(k + 1);   // read as "not k" by the other threads of this sweep either way
                changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) break;   // an empty frontier (:339)
    }
    unsigned char *cm = conf + tick * tick_pix + fd.depth_off;
    for (int i = threadIdx.x; i < kConfTile * kConfTile; i += blockDim.x) {
        const int lx = kConfHalo + i % kConfTile, ly = kConfHalo + i / kConfTile;
        const int x = ox + lx, y = oy + ly;
        if (x >= w || y >= h) continue;
        const unsigned char c = s_c[ly * kConfSide + lx];
        cm[(long long)y * w + x] = c >= kOut ? (unsigned char)kConfLimit : c;
    }
}

// The per-block sample counts of one (tick, pair) into exclusive prefixes, in place: one workgroup per (tick, pair).
__global__ __launch_bounds__(1024) void ct_block_scan_kernel(int *blk, int nblk)
{
    __shared__ int s_wave[16];
    int *b = blk + (long long)blockIdx.x * nblk;
    block_scan_array_excl<int, 1024>(b, 1, b, nblk, s_wave);
}

}  // namespace

namespace lsn {

// The cloud index of d_depth, over all ticks of the plan, on `s`: the pixel <-> vertex maps into ix_pix2v / ix_v2pix (ix_off: the vertex
// offsets the pass itself finds) and, with_conf, the confidence maps into ix_conf.  The buffers are reserved on first use -- the
// confidence ones by the first caller that asks for them.  Plan mutex held, the plan's device current.
static int cloud_index_locked(LsnFusion *p, const void *d_depth, void *d_vertices, bool with_conf, hipStream_t s)
{
    const int n = p->n_maps, T = p->n_ticks;
    const size_t px = (size_t)p->cap * T;
    if (p->ix_counts.reserve(sizeof(int) * (size_t)p->tiles_per_tick * T) || p->ix_off.reserve(sizeof(int) * (size_t)(n + 1) * T) ||
        p->ix_pix2v.reserve(sizeof(int) * px) || p->ix_v2pix.reserve(sizeof(int) * px))
        return -1;
    std::vector<int> ctile(with_conf ? n + 1 : 0, 0);   // first confidence tile of every sensor
    for (int i = 0; with_conf && i < n; i++) ctile[i + 1] = ctile[i] + ((p->w[i] + kConfTile - 1) / kConfTile) * ((p->h[i] + kConfTile - 1) / kConfTile);
    if (with_conf && !p->ix_conf_ready) {
        if (p->ix_conf.reserve(px) || p->ix_ctile.reserve(sizeof(int) * (size_t)(n + 1))) return -1;
        LSN_HIP(hipMemcpy(p->ix_ctile.p, ctile.data(), sizeof(int) * (size_t)(n + 1), hipMemcpyHostToDevice));
        p->ix_conf_ready = true;
    }
    // the fusion's keep predicate, arithmetic form
    FuseArgs fa;
    fill_args(p, fa, d_depth, d_depth, d_vertices, p->ix_off.as<int>(), false);
    fa.thr = nullptr;
    hipLaunchKernelGGL(ct_index_kernel<0>, dim3(p->tiles_per_tick, T), dim3(kThreads), 0, s, fa, p->ix_counts.as<int>(), p->ix_pix2v.as<int>(),
                       p->ix_v2pix.as<int>());
    hipLaunchKernelGGL(scan_kernel, dim3(T), dim3(kScanThreads), 0, s, p->ix_counts.as<int>(), p->tiles_per_tick, fa.frames, n,
                       p->ix_off.as<int>(), (int *)nullptr);
    hipLaunchKernelGGL(ct_index_kernel<1>, dim3(p->tiles_per_tick, T), dim3(kThreads), 0, s, fa, p->ix_counts.as<int>(), p->ix_pix2v.as<int>(),
                       p->ix_v2pix.as<int>());
    if (with_conf)
        hipLaunchKernelGGL(ct_conf_kernel, dim3(ctile[n], T), dim3(256), 0, s, fa.frames, p->ix_ctile.as<int>(), n,
                           static_cast<const unsigned short *>(d_depth), p->tick_depth_elems, p->ix_conf.as<unsigned char>());
    return 0;
}

}  // namespace lsn
