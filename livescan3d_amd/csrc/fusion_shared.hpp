// fusion_shared.hpp -- what the translation units of the fusion plan share: the device-side building blocks of the fused
// unproject + transform + crop + compaction kernels (fusion.hip holds the design notes), the scan kernel, and the host-side
// plan object behind the opaque LsnFusion handle.  Device code lives in an anonymous namespace: every .hip file gets its own copy.
#pragma once

#include "lsn_common.hpp"
#include "wave_ops.hpp"

#include <cstdint>
#include <mutex>
#include <vector>

namespace lsn {

// Two numberings are called "mode" in this library.  The PLAN's mode is what lsnFusionSetMode takes (LsnFusion::mode) and says how a
// call resolves the tiles' offsets; the kernel PASS is fuse_kernel's MODE template parameter and says what one launch does.  Plain ints,
// not an enum type: the value is part of the kernels' mangled names, which the profiles and lsnFusionKernelStats report.
constexpr int kPlanThreeLaunches = 0;   // count -> scan -> write
constexpr int kPlanLookbackRuns = 1;    // one launch of run_kernel: runs of tiles, one look-back per run
constexpr int kPlanSinglePass = 2;      // one launch of fuse_kernel<kPassSingle>: one look-back per tile
constexpr int kPassCount = 0;           // counts into tile_counts
constexpr int kPassWrite = 1;           // writes at the scanned tile_counts
constexpr int kPassWriteCountNext = 3;  // kPassWrite + the count of the NEXT batch (lsnFusionRunStreamed)
constexpr int kPassSingle = 4;          // computes once, resolves its offset by look-back over the tiles before it

struct FrameDesc {
    int w, h, npix, tile_start;  // tile_start: first tile of this frame inside its tick
    long long depth_off;         // u16 elements from the tick's depth base
    long long rgb_off;           // bytes from the tick's colour base
    int xtab_off, ytab_off;      // this sensor's rows of the unprojection tables (floats)
    float inv_w;                 // 1 / w, for the (corrected, exact) float division of small pixel offsets
    int pad1;
};

struct TileDesc {  // one per tile of a tick
    int frame;     // sensor-frame the tile belongs to
    int x0, y0;    // column / row of the tile's first pixel (host-computed: no integer division on the device)
    int pad;
};

struct SensorParams {  // 16 floats, wave-uniform -> scalar loads
    float cx, cy, fx, fy;
    float t0, t1, t2;
    float r00, r01, r02, r10, r11, r12, r20, r21, r22;
};

// IntrinsicCameraParameters(float*) / WorldTranformation(float*), include/NativeUtils/depthprocessing.h:56-63,96-97: the caller's 7 and 12
// floats of one sensor as the kernels read them.  The one place the unpack order is written down (tests/test_abi.py holds it against
// the reference's own constructors through lsnPackSensorParams).
inline void pack_sensor_params(const float *ip, const float *tp, SensorParams &s)
{
    s.cx = ip[0]; s.cy = ip[1]; s.fx = ip[2]; s.fy = ip[3];
    s.t0 = tp[0]; s.t1 = tp[1]; s.t2 = tp[2];
    s.r00 = tp[3]; s.r01 = tp[4]; s.r02 = tp[5];
    s.r10 = tp[6]; s.r11 = tp[7]; s.r12 = tp[8];
    s.r20 = tp[9]; s.r21 = tp[10]; s.r22 = tp[11];
}

struct FuseArgs {
    const FrameDesc *frames;
    const TileDesc *tiles;             // tile (within tick) -> frame and first-pixel coordinates
    const SensorParams *params;
    const float *xtab;  // [(x - cx) / fx] per sensor column
    const float *ytab;  // [(cy - y) / fy] per sensor row
    const unsigned short *depth;
    const unsigned char *rgb;
    uint4 *out;
    int *tile_counts;                // count and write passes: [n_ticks * tiles_per_tick] counts, then exclusive prefixes (scan_kernel)
    unsigned long long *run_state;   // [n_ticks * tiles_per_tick] look-back words: run_kernel {flag:2 | value}, indexed by run; kPassSingle {epoch | flag:2 | value}, by tile
    unsigned int *ticket;            // run_kernel: per-tick run tickets, 32 words apart
    int *offsets;                    // [n_ticks][n_frames + 1]
    int *pixmap;                     // optional [n_ticks][pixels per tick]: vertex index inside the tick's cloud, -1 = none (rigs the 8-pixel lanes do not fit)
    int *pm_first;                   // ... or its compact form, per lane of 8 pixels: index of the lane's first vertex ...
    unsigned char *pm_mask;          // ... and which of the 8 pixels have one (0.625 instead of 4 bytes per pixel)
    const unsigned short *depth_next;  // kPassWriteCountNext: the NEXT batch's depth, counted in the shadow of this write
    int *tile_counts_next;             // ... and where its per-tile counts go
    int *error_flag;                 // run_kernel, kPassSingle: set when a bounded look-back spin gives up; write passes: a tile's count differs from the scanned one (sticky until read)
    const unsigned int *thr;         // optional [pixels per tick]: the depth interval each pixel survives in (thresh_kernel), null = none
    int n_frames;
    int tiles_per_tick;
    int n_ticks;
    int tiles_per_run;               // run_kernel
    unsigned int epoch;              // kPassSingle: tag of this launch's look-back words (run_state is cleared only when it wraps)
    int chunk;                       // write pass block order: 0 = tick-major; C > 0 = chunks of C consecutive tiles, all ticks of a chunk before the next chunk
    int reverse_ticks;               // the write pass takes the ticks last to first (what the count pass read last is nearest in cache); always 1
    int tile0;                       // one-tick plans only: the launch covers tiles [tile0, tile0 + gridDim.x) of the tick (a group of sensors, run_frames)
    int host_out;                    // kPassSingle: `out` is pinned host memory (plain, destination-aligned stores; see stage_and_store)
    int *group_end_mirror;           // kPassSingle, optional (pinned host memory): where this launch's vertices end inside the tick, stored by its last tile
    int *offsets_mirror;             // kPassSingle, optional: the offset table entries are also stored here (pinned host memory), [n_frames + 1] = give-up flag
    int runs_per_tick;               // run_kernel
    long long tick_depth_stride;  // u16 elements
    long long tick_rgb_stride;    // bytes
    long long tick_vert_stride;   // vertices
    float minX, minY, minZ, maxX, maxY, maxZ;
};

// Kernel arguments of the triangulation passes (mesh.hip: tri_kernel<0 / 1>).
struct TriArgs {
    const FrameDesc *frames;
    const TileDesc *tiles;
    const unsigned short *depth;
    const int *pixmap;   // [n_ticks][pixels per tick] (rigs whose widths are not multiples of 8) ...
    const int *pm_first; // ... or [n_ticks][pixels per tick / 8]: the first vertex index of every lane of 8 pixels ...
    const unsigned char *pm_mask;   // ... and the mask of its pixels that have a vertex
    int *tri;            // [n_ticks][tri_cap][3]
    int *tile_counts;    // [n_ticks * tiles_per_tick] counts, then exclusive prefixes (scan_kernel)
    unsigned int *codes; // [n_ticks * tiles_per_tick * 256] per-lane 4-bit-per-pixel triangle codes: count pass -> write pass
    int tiles_per_tick;
    int win;                    // triangles staged per LDS round of the write pass
    int host_out;               // `tri` is pinned host memory: the launch picks the HOST form of the write pass
    int index_base;             // added to every vertex index a triangle names: the tick's vertices start there in the caller's cloud (a call
                                // sharded over devices, host_flows.hip: formMesh's rebase across devices); 0 everywhere else
    long long tick_pix_stride;  // pixels per tick
    long long tick_tri_stride;  // triangles per tick (capacity)
};

}  // namespace lsn
using lsn::FrameDesc;
using lsn::FuseArgs;
using lsn::TriArgs;
using lsn::SensorParams;
using lsn::pack_sensor_params;
using lsn::TileDesc;

namespace {

constexpr int kThreads = 256;
constexpr int kPxPerLane = 8;
constexpr int kTile = kThreads * kPxPerLane;  // 2048 pixels per workgroup step
constexpr int kWin = 1152;                    // survivors staged per LDS round (9/16 of a tile)
// The merged cloud is written once and not read again by the launch sequence: streaming (nt) stores keep the 15 MB per tick
// out of L2 / Infinity Cache, where the depth frames and the threshold table live between the count and the write pass
// (measured: 0.335 -> 0.310 ms per 64-tick step; nt loads of the inputs in the write pass changed nothing).
constexpr bool kNontemporalStores = true;

// (FrameDesc, TileDesc, SensorParams and FuseArgs are declared above, in namespace lsn: they appear in the signatures of
// the host helpers shared between the translation units and therefore need external linkage)


typedef float f2 __attribute__((ext_vector_type(2)));

// Z = float(d) / 1000.0f (depthprocessing.cpp:149-150) for two pixels without the ~13-instruction IEEE division:
// with r = fl32(1/1000) = 0x3a83126f, q0 = d*r, e = fma(-q0, 1000, d), q = fma(e, r, q0) is the correctly rounded
// quotient for EVERY u16 d -- proven exhaustively with exact rational arithmetic in tests/test_fast_division.py.
__device__ __forceinline__ f2 depth_to_metres2(f2 d)
{
    const f2 r = {0x1.0624dep-10f, 0x1.0624dep-10f};
    const f2 k = {1000.0f, 1000.0f};
    const f2 q0 = d * r;
    const f2 e = __builtin_elementwise_fma(-q0, k, d);
    return __builtin_elementwise_fma(e, r, q0);
}

// createVertices' per-pixel arithmetic (depthprocessing.cpp:149-163) on TWO pixels at once, one rounding per
// operation (contraction is off, so a*b+c stays a packed multiply and a packed add: v_pk_mul_f32 / v_pk_add_f32 do two
// f32 lanes' worth per issue slot, which halves the VALU time of this VALU-heavy kernel).
// xfac = (float(x) - cx) / fx and yfac = (cy - float(y)) / fy (:151-152) depend on the column / row only; they come
// from per-sensor tables filled on the device with the same IEEE operations (table_kernel), so the per-pixel work
// has no division left.
__device__ __forceinline__ void unproject2(f2 d, f2 xfac, f2 yfac, const SensorParams &P, f2 &ox, f2 &oy, f2 &oz)
{
    f2 Z = depth_to_metres2(d);
    f2 X = xfac * Z;
    f2 Y = yfac * Z;
    X = X + P.t0;
    Y = Y + P.t1;
    Z = Z + P.t2;
    ox = X * P.r00 + Y * P.r01 + Z * P.r02;
    oy = X * P.r10 + Y * P.r11 + Z * P.r12;
    oz = X * P.r20 + Y * P.r21 + Z * P.r22;
}

// The inclusive AABB test with the reference's own comparisons (:162), so that a NaN coordinate is kept exactly like
// the reference keeps it (non-short-circuit '|': six compares and lane-mask ORs, no divergent branches).
__device__ __forceinline__ bool inside_box(float ox, float oy, float oz, const FuseArgs &a)
{
    const bool rejected = (ox < a.minX) | (ox > a.maxX) | (oy < a.minY) | (oy > a.maxY) | (oz < a.minZ) | (oz > a.maxZ);
    return !rejected;
}

// Number of survivors among the lower lanes of the wave, and in the whole wave, straight from the keep predicates'
// lane masks: v_mbcnt per mask for the lanes below, s_bcnt1 (SALU) for the total -- no shuffles, no per-lane counters.
__device__ __forceinline__ void rank_from_masks(const bool (&keep)[kPxPerLane], int &below, int &wave_total)
{
    below = 0;
    wave_total = 0;
#pragma unroll
    for (int k = 0; k < kPxPerLane; k++) {
        const unsigned long long m = __ballot(keep[k]);
        below = __builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, below));
        wave_total += __popcll(m);
    }
}

// ---- one tile: where it is, its inputs, its arithmetic --------------------------------------------------------

struct Tile {  // wave-uniform (SGPRs)
    long long pix_base;      // index of the frame's first pixel inside its tick (= depth_off)
    int f, w, h, npix, px0;  // frame, its size, first pixel of the tile inside the frame
    int x0, y0;              // that pixel's column / row
    float inv_w;
    bool frame_start;
    const unsigned short *dptr;
    const unsigned char *cptr;
    const float *xt, *yt;
};

__device__ __forceinline__ Tile locate(const FuseArgs &a, int tick, int tile)
{
    Tile t;
    const TileDesc td = a.tiles[tile];
    t.f = td.frame;
    t.x0 = td.x0;
    t.y0 = td.y0;
    const FrameDesc fd = a.frames[t.f];
    t.inv_w = fd.inv_w;
    t.pix_base = fd.depth_off;
    t.w = fd.w;
    t.h = fd.h;
    t.npix = fd.npix;
    t.px0 = (tile - fd.tile_start) * kTile;
    t.frame_start = tile == fd.tile_start;
    t.dptr = a.depth + tick * a.tick_depth_stride + fd.depth_off;
    t.cptr = a.rgb + tick * a.tick_rgb_stride + fd.rgb_off;
    t.xt = a.xtab + fd.xtab_off;
    t.yt = a.ytab + fd.ytab_off;
    return t;
}

struct Inputs {  // one lane's 8 pixels
    unsigned int dw[4];  // 8 x u16 depth
    unsigned int cw[6];  // 8 x RGB8
};

// VEC: every frame has w % 8 == 0 and the buffers are 16-B aligned -> one 16-B depth load, 24 B of colour per lane.
template <bool VEC, bool RGB>
__device__ __forceinline__ void load_inputs(const Tile &t, Inputs &in)
{
    const int p0 = t.px0 + threadIdx.x * kPxPerLane;
#pragma unroll
    for (int i = 0; i < 4; i++) in.dw[i] = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) in.cw[i] = 0;
    if (VEC) {
        if (p0 < t.npix) {
            const uint4 dv = *reinterpret_cast<const uint4 *>(t.dptr + p0);
            in.dw[0] = dv.x; in.dw[1] = dv.y; in.dw[2] = dv.z; in.dw[3] = dv.w;
            if (RGB) {
                const uint2 *cp = reinterpret_cast<const uint2 *>(t.cptr + 3ll * p0);
                const uint2 c0 = cp[0], c1 = cp[1], c2 = cp[2];
                in.cw[0] = c0.x; in.cw[1] = c0.y; in.cw[2] = c1.x; in.cw[3] = c1.y; in.cw[4] = c2.x; in.cw[5] = c2.y;
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < kPxPerLane; k++) {
            if (p0 + k < t.npix) {
                const unsigned int d = t.dptr[p0 + k];
                in.dw[k >> 1] |= d << ((k & 1) * 16);
                if (RGB) {
                    const unsigned char *c = t.cptr + 3ll * (p0 + k);
                    const unsigned int rgb = c[0] | (c[1] << 8) | (c[2] << 16);
                    const int b = 3 * k;  // the pixel's 3 bytes start at byte 3k of the lane's 24-byte group
                    in.cw[b >> 2] |= rgb << ((b & 3) * 8);
                    if ((b & 3) > 1) in.cw[(b >> 2) + 1] |= rgb >> ((4 - (b & 3)) * 8);
                }
            }
        }
    }
}

// The colours alone (the lazy-colour write pass loads them after the keep predicates are known, for the lanes that kept anything).
template <bool VEC>
__device__ __forceinline__ void load_rgb(const Tile &t, Inputs &in)
{
    const int p0 = t.px0 + threadIdx.x * kPxPerLane;
    if (VEC) {
        if (p0 < t.npix) {
            const uint2 *cp = reinterpret_cast<const uint2 *>(t.cptr + 3ll * p0);
            const uint2 c0 = cp[0], c1 = cp[1], c2 = cp[2];
            in.cw[0] = c0.x; in.cw[1] = c0.y; in.cw[2] = c1.x; in.cw[3] = c1.y; in.cw[4] = c2.x; in.cw[5] = c2.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < kPxPerLane; k++) {
            if (p0 + k < t.npix) {
                const unsigned char *c = t.cptr + 3ll * (p0 + k);
                const unsigned int rgb = c[0] | (c[1] << 8) | (c[2] << 16);
                const int b = 3 * k;
                in.cw[b >> 2] |= rgb << ((b & 3) * 8);
                if ((b & 3) > 1) in.cw[(b >> 2) + 1] |= rgb >> ((4 - (b & 3)) * 8);
            }
        }
    }
}

// {R, G, B, A = 255} of pixel k of the lane (depthprocessing.cpp:1598-1601)
__device__ __forceinline__ unsigned int rgba_of(const Inputs &in, int k)
{
    const int b = 3 * k;
    const unsigned int lo = in.cw[b >> 2];
    const unsigned int hi = in.cw[(b >> 2) + 1 < 6 ? (b >> 2) + 1 : 5];
    return (__funnelshift_r(lo, hi, (b & 3) * 8) & 0x00FFFFFFu) | 0xFF000000u;
}

// Keep predicates (wave-wide lane masks in SGPR pairs) and, when WRITE, the assembled vertices of a lane's 8 pixels.
// Branch-free: a zero depth (invalid pixel, :144, or a lane past the frame end) is computed and then dropped.
// (column, row) of the lane's first pixel: the tile starts at (x0, y0) and the lane is v = x0 + 8*tid < w + 2048 columns
// further; v / w by a float multiply and an exact +-1 correction (v < 2^23, so the estimate is off by at most one).
__device__ __forceinline__ void lane_origin(const Tile &t, int &x, int &y)
{
    const int p0 = t.px0 + threadIdx.x * kPxPerLane;
    const int v = t.x0 + (int)threadIdx.x * kPxPerLane;
    int q = (int)((float)v * t.inv_w);
    x = v - q * t.w;
    if (x < 0) { q--; x += t.w; }
    if (x >= t.w) { q++; x -= t.w; }
    y = t.y0 + q;
    if (p0 >= t.npix) { x = 0; y = 0; }
}

// streaming 16-byte store of one vertex (the merged cloud is written once and not read again by the launch sequence)
__device__ __forceinline__ void store_vertex(uint4 *dst, const uint4 v)
{
    if (kNontemporalStores) {
        __builtin_nontemporal_store(v.x, &dst->x);
        __builtin_nontemporal_store(v.y, &dst->y);
        __builtin_nontemporal_store(v.z, &dst->z);
        __builtin_nontemporal_store(v.w, &dst->w);
    } else {
        *dst = v;
    }
}

// The column / row factors of a lane's 8 pixels (they depend on the tile geometry only, not on the tick or the batch).
template <bool VEC>
__device__ __forceinline__ void tile_factors(const Tile &t, float (&xf)[kPxPerLane], float (&yf)[kPxPerLane])
{
    int x, y;
    lane_origin(t, x, y);
    float yfac = t.yt[y];
    if (VEC) {
        // w % 8 == 0: the lane's 8 pixels share a row and their columns are 8 consecutive, 32-B aligned table entries
        const float4 x0 = *reinterpret_cast<const float4 *>(t.xt + x);
        const float4 x1 = *reinterpret_cast<const float4 *>(t.xt + x + 4);
        xf[0] = x0.x; xf[1] = x0.y; xf[2] = x0.z; xf[3] = x0.w;
        xf[4] = x1.x; xf[5] = x1.y; xf[6] = x1.z; xf[7] = x1.w;
#pragma unroll
        for (int k = 0; k < kPxPerLane; k++) yf[k] = yfac;
    } else {
#pragma unroll
        for (int k = 0; k < kPxPerLane; k++) {
            xf[k] = t.xt[x];
            yf[k] = yfac;
            // rows may end inside a lane's 8 pixels when w % 8 != 0
            x++;
            if (x == t.w) {
                x = 0;
                y = y + 1 < t.h ? y + 1 : y;
                yfac = t.yt[y];
            }
        }
    }
}

template <bool WRITE>
__device__ __forceinline__ void compute_pixels(const FuseArgs &a, const SensorParams &P, const Inputs &in, const float (&xf)[kPxPerLane],
                                               const float (&yf)[kPxPerLane], bool (&keep)[kPxPerLane], uint4 (&vert)[kPxPerLane])
{
#pragma unroll
    for (int k = 0; k < kPxPerLane; k += 2) {
        const unsigned int d0 = in.dw[k >> 1] & 0xFFFFu, d1 = in.dw[k >> 1] >> 16;
        f2 ox, oy, oz;
        unproject2(f2{(float)d0, (float)d1}, f2{xf[k], xf[k + 1]}, f2{yf[k], yf[k + 1]}, P, ox, oy, oz);
        keep[k] = inside_box(ox.x, oy.x, oz.x, a) && d0 != 0;
        keep[k + 1] = inside_box(ox.y, oy.y, oz.y, a) && d1 != 0;
        if (WRITE) {
#pragma unroll
            for (int j = 0; j < 2; j++) {
                vert[k + j].x = rgba_of(in, k + j);  // A = 255 (:1601)
                vert[k + j].y = __float_as_uint(j ? ox.y : ox.x);
                vert[k + j].z = __float_as_uint(j ? oy.y : oy.x);
                vert[k + j].w = __float_as_uint(j ? oz.y : oz.x);
            }
        }
    }
}

template <bool VEC, bool WRITE>
__device__ __forceinline__ void compute_tile(const FuseArgs &a, const Tile &t, const Inputs &in, bool (&keep)[kPxPerLane],
                                             uint4 (&vert)[kPxPerLane])
{
    const SensorParams P = a.params[t.f];
    float xf[kPxPerLane], yf[kPxPerLane];
    tile_factors<VEC>(t, xf, yf);
    compute_pixels<WRITE>(a, P, in, xf, yf, keep, vert);
}

// Where rank q of a staged window lives: q + q / 8 (one 16-byte pad per 8 ranks; one per 16 ranks or none measured 0.2958 / 0.2951 /
// 0.3005 ms per step: profiles/r04_ab_pad.txt).
constexpr int kStagePadShift = 3;
__device__ __forceinline__ int stage_slot16(int q) { return q + (q >> kStagePadShift); }
constexpr int kStageSlots = kWin + (kWin >> kStagePadShift) + 1;

// Stages a tile's survivors in LDS in rank order, window by window, and copies them out with consecutive lanes writing
// consecutive 16-B vertices.  Rank q of a window lives at slot q + q/8: a lane's 8 consecutive ranks then start 9 slots
// (144 B) apart, which keeps the 16-B LDS writes of neighbouring lanes on different bank groups (stride 128 B is an
// 8-way conflict).  A typical tile (crop + invalid pixels) fits in one window of kWin; the 20.7 KB footprint (instead of
// 36.9 KB for a whole tile) lets 7 workgroups share a CU.  Every thread must call this (barriers inside); rank0 is the
// lane's first rank inside the tile, tile_tot is uniform.  On return the LDS window is free again.
// host_dst: the destination is pinned host memory (the exports' output block, host_flows.hip) -- the stores cross PCIe, where plain stores
// move ~5 % more than streaming ones and a wave whose 1 KB starts on a 1 KB boundary ~3 % more than one that straddles lines
// (tools/link_probe.hip), so the copy-out is shifted to the destination's alignment.
__device__ __forceinline__ void stage_and_store(uint4 *stage, const bool (&keep)[kPxPerLane], const uint4 (&vert)[kPxPerLane], int rank0,
                                                int tile_tot, uint4 *dst, bool host_dst = false)
{
    for (int w0 = 0; w0 < tile_tot; w0 += kWin) {
        int r = rank0 - w0;
#pragma unroll
        for (int k = 0; k < kPxPerLane; k++) {
            if (keep[k]) {
                if ((unsigned int)r < (unsigned int)kWin) stage[stage_slot16(r)] = vert[k];
                r++;
            }
        }
        __syncthreads();
        const int n = min(kWin, tile_tot - w0);
        if (host_dst) {
            const int mis = (int)((reinterpret_cast<uintptr_t>(dst + w0) >> 4) & 63);
            for (int i = (int)threadIdx.x - mis; i < n; i += kThreads)
                if (i >= 0) dst[w0 + i] = stage[stage_slot16(i)];
        } else
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const uint4 v = stage[stage_slot16(i)];
            if (kNontemporalStores) {   // written once, never read again by this launch sequence
                __builtin_nontemporal_store(v.x, &dst[w0 + i].x);
                __builtin_nontemporal_store(v.y, &dst[w0 + i].y);
                __builtin_nontemporal_store(v.z, &dst[w0 + i].z);
                __builtin_nontemporal_store(v.w, &dst[w0 + i].w);
            } else {
                dst[w0 + i] = v;
            }
        }
        __syncthreads();
    }
}

// Aligned copy of n bytes that sit in LDS at lds[lead ..), lead = (address of dst) mod 16, to dst: the 16-byte chunks that lie
// wholly inside the range go out as one store each, the (< 16-byte) pieces at either end element by element (ELEM bytes each) --
// the neighbouring tiles own the rest of those chunks.  Every thread of a kThreads workgroup calls it.  (exchange.hip: pack_kernel's survivor
// streams; radial.hip: radial_gather_pack_kernel's tile.)
template <int ELEM, typename T>
__device__ __forceinline__ void store_run(T *dst, const T *lds, int lead, int n)
{
    static_assert(sizeof(T) == ELEM, "element size");
    const int end = lead + n;                        // in bytes, relative to the aligned start of the first chunk
    const int c0 = lead ? 1 : 0, c1 = end >> 4;       // chunks [c0, c1) are whole
    uint4 *g16 = reinterpret_cast<uint4 *>(reinterpret_cast<unsigned char *>(dst) - lead);
    const uint4 *l16 = reinterpret_cast<const uint4 *>(lds);
    for (int j = c0 + (int)threadIdx.x; j < c1; j += kThreads) g16[j] = l16[j];
    const int head = lead ? min(n, 16 - lead) : 0;   // bytes before the first whole chunk
    const int tail0 = max(head, 16 * c1 - lead);     // first byte after the last whole chunk
    const int t = (int)threadIdx.x * ELEM;
    if (t < head) dst[threadIdx.x] = lds[lead / ELEM + threadIdx.x];
    if (tail0 + t < n) dst[tail0 / ELEM + threadIdx.x] = lds[(lead + tail0) / ELEM + threadIdx.x];
}

// Mode 0, between the count and the write launch: one workgroup per tick turns that tick's tile counts into exclusive
// prefixes in place and fills the per-sensor offset table (offsets[tick][f] = first vertex of sensor f, [n_frames] = total).
// 1024 threads x 8 consecutive counts each: a tick of up to 8192 tiles (16 x 1024x1024) is ONE round -- two 16-byte loads, a serial
// prefix in registers, a wave scan of the lane totals, 16 wave totals through LDS -- where 256 threads x 1 count walked it in 32
// rounds of three barriers each (the config-5 shape has 8 such ticks per step: 8 workgroups on 256 CUs, all of them that slow).
// mirror (optional): the offset table is also stored there -- pinned host memory, so the host has the counts when the stream
// is idle without a copy of its own.
constexpr int kScanThreads = 1024;
constexpr int kScanItems = 8;
constexpr int kScanWaves = kScanThreads / 64;

__device__ __forceinline__ void scan_tick(int *tc, int tiles_per_tick, const FrameDesc *frames, int n_frames, int *off, int *mirror_row,
                                          int (&s_wave)[kScanWaves])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;   // uniform: every thread adds the same round totals
    for (int c0 = 0; c0 < tiles_per_tick; c0 += kScanThreads * kScanItems) {
        const int i0 = c0 + (int)threadIdx.x * kScanItems;
        int v[kScanItems];
        const bool whole = i0 + kScanItems <= tiles_per_tick && (reinterpret_cast<uintptr_t>(tc + i0) & 15) == 0;
        if (whole) {
            const int4 a = reinterpret_cast<const int4 *>(tc + i0)[0], b = reinterpret_cast<const int4 *>(tc + i0)[1];
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        } else {
#pragma unroll
            for (int k = 0; k < kScanItems; k++) v[k] = i0 + k < tiles_per_tick ? tc[i0 + k] : 0;
        }
        int t = 0;
#pragma unroll
        for (int k = 0; k < kScanItems; k++) {   // v[k] becomes the exclusive prefix inside the lane
            const int x = v[k];
            v[k] = t;
            t += x;
        }
        const int incl = wave_scan_incl(t, lane);
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int pre = carry, round_tot = 0;
#pragma unroll
        for (int w = 0; w < kScanWaves; w++) {
            const int x = s_wave[w];
            if (w < wave) pre += x;
            round_tot += x;
        }
        pre += incl - t;
        if (whole) {
            reinterpret_cast<int4 *>(tc + i0)[0] = make_int4(pre + v[0], pre + v[1], pre + v[2], pre + v[3]);
            reinterpret_cast<int4 *>(tc + i0)[1] = make_int4(pre + v[4], pre + v[5], pre + v[6], pre + v[7]);
        } else {
#pragma unroll
            for (int k = 0; k < kScanItems; k++)
                if (i0 + k < tiles_per_tick) tc[i0 + k] = pre + v[k];
        }
        carry += round_tot;
        __syncthreads();   // s_wave is rewritten by the next round; the prefixes above are visible to the workgroup below
    }
    // frames are few: thread f looks up the prefix at its first tile (written above by this workgroup)
    for (int f = threadIdx.x; f <= n_frames; f += kScanThreads) {
        const int v = f < n_frames ? tc[frames[f].tile_start] : carry;
        off[f] = v;
        if (mirror_row) mirror_row[f] = v;
    }
}

// Launch with dim3(n_ticks) x dim3(kScanThreads).
__attribute__((unused)) __global__ __launch_bounds__(kScanThreads) void scan_kernel(int *tile_counts, int tiles_per_tick, const FrameDesc *frames, int n_frames,
                                                        int *offsets, int *mirror)
{
    __shared__ int s_wave[kScanWaves];
    const int tick = blockIdx.x;
    scan_tick(tile_counts + (long long)tick * tiles_per_tick, tiles_per_tick, frames, n_frames, offsets + (long long)tick * (n_frames + 1),
                     mirror ? mirror + (long long)tick * (n_frames + 1) : nullptr, s_wave);
}


}  // namespace

// -------------------------------------------------------------------------------------------------------------
// host side: the plan
// -------------------------------------------------------------------------------------------------------------

struct LsnFusion {
    int device = 0;
    int n_ticks = 0, n_maps = 0;
    std::vector<int> w, h;
    std::vector<int> tile_start;  // first tile of every frame inside a tick, [n_maps] = tiles_per_tick
    long long cap = 0;  // vertices per tick
    long long tick_depth_elems = 0, tick_rgb_bytes = 0;
    int tiles_per_tick = 0;
    bool vec_ok = false;
    bool params_set = false;
    int mode = lsn::kPlanThreeLaunches;   // lsnFusionSetMode
    unsigned int epoch = 0;          // single-pass launches so far (tags the look-back words)
    float bounds[6] = {0, 0, 0, 0, 0, 0};
    lsn::DevBuf frames, tile_frame, params, tile_counts, tile_state, misc;  // misc: error flag (word 0) + tickets
    lsn::DevBuf xtab, ytab;
    lsn::DevBuf pixmap, pm_first, pm_mask, tri_counts, tri_codes;  // triangulation scratch, allocated on first use
    bool pixmap_compact = false;     // which form of the pixel -> vertex map the last run wrote
    lsn::RadialScratch rd;           // the radial correction (radial.hip), allocated on first use
    // pipelined mode: the count + scan of call k+1 run on a side stream while the write kernel of call k is still busy
    bool pipelined = false;
    hipStream_t side = nullptr;
    hipEvent_t ev_counted = nullptr, ev_written[2] = {nullptr, nullptr};
    lsn::DevBuf tile_counts_b, offs_int;  // second count buffer, internal offsets [2][n_ticks][n_maps+1]
    unsigned long long calls = 0;
    // streamed mode: which batch the "other" half of the count scratch was counted for
    const void *counted_for = nullptr;
    unsigned long long counted_gen = 0, params_gen = 1;
    int stream_half = 0;
    // per-pixel depth thresholds (thresh_kernel): built once the same parameters are used for a second run
    lsn::DevBuf thr;
    // the cloud index the three stages below start from (cloud_index.hip), allocated on first use and rebuilt by every stage from its own
    // input: tile counts / offsets of the index pass, pixel <-> vertex maps; confidence maps and confidence-tile starts (allocated by the
    // first stage that asks for them)
    lsn::DevBuf ix_counts, ix_off, ix_pix2v, ix_v2pix, ix_conf, ix_ctile;
    bool ix_conf_ready = false;
    // colour transfer (color.hip), allocated on first use: coverage tables, chosen pairs, per-block sample counts, colour sums, compacted
    // samples, transforms
    lsn::DevBuf ct_cov, ct_pairs, ct_blk, ct_stats, ct_samples, ct_xform;
    bool ct_ready = false;
    int ct_nblk = 0;                     // sample blocks per pair (the largest sensor's pixels / 256)
    // colour blend (color_blend.hip), allocated on first use: the colour dword of every vertex as the call found it, and the counters of
    // the last call, three 64-bit words per (tick, sensor)
    lsn::DevBuf cb_snap, cb_diag;
    bool cb_ready = false;
    // overlay merge (merge.hip), allocated on its first call: intermediate triangle offsets, the reprojected maps (as first built / as
    // modified) and their pixel -> vertex maps, point_assigned, per-vertex confidence and projection, raster scratch, mapped depth / tag
    // maps, eroded mask
    lsn::DevBuf mg_toff, mg_depth0, mg_depth, mg_d2v, mg_assigned, mg_vconf, mg_proj, mg_zmax, mg_key, mg_mdepth, mg_mtag, mg_ero;
    bool mg_ready = false;
    // outlier filter (outlier.hip), allocated on its first call: each vertex's bucket, the bucket tables and their chunk sums, the points in
    // bucket order, removed flags, per-sensor counts, the caller's offsets, the sensors' bucket bases and masks, the blocks' bounding boxes
    // and grid frames
    lsn::DevBuf ol_key, ol_bucket, ol_chunk, ol_pts, ol_removed, ol_stats, ol_offs, ol_tab, ol_box, ol_frame;
    bool ol_ready = false;
    int ol_nb = 0, ol_nchunk = 0;        // buckets per tick, scan chunks per tick
    // flying-pixel filter (flying.hip), allocated on its first call: the 128 x 16 tiles of one tick, the removed pixels of depth != 0 per
    // tile of every tick (lsnFusionFlyingDiagnostics adds them up per sensor through fl_tile_frame)
    lsn::DevBuf fl_tiles, fl_counts;
    std::vector<int> fl_tile_frame;
    bool fl_ready = false;
    int fl_tiles_per_tick = 0;
    int fl_last = 0;                     // what the last call was: 0 = none yet, 1 = a copy (neighbourhood <= 0), 2 = the filter
    hipStream_t fl_stream = nullptr;     // ... and its stream
    // depth smoothing (depth_smooth.hip): the setting of lsnFusionSetDepthSmooth (radius 0: off) -- one device table, the range table
    // zero-padded to the 1032 entries the kernel stages and the spatial table behind it (ds_table_host: what it holds) -- and, allocated
    // by the first filtering call, two words per 128 x 16 tile of every tick (the tile list is fl_tiles)
    int ds_radius = 0, ds_n_range = 0;
    std::vector<unsigned short> ds_table_host;
    lsn::DevBuf ds_table, ds_counts;
    int ds_last = 0;                     // what the last call was: 0 = none yet, 1 = a copy (off), 2 = the filter
    hipStream_t ds_stream = nullptr;     // ... and its stream
    // the two stages with state (lsn::StageState, lsn_common.hpp), each with its setting (off by default), its record -- allocated by the
    // first call that needs it -- and what its last call was: 0 = none yet, 1 = a copy (off), 2 = the stage.  The temporal depth filter
    // (temporal.hip): the history, one word per pixel of one tick, four count words per 128 x 16 tile of every tick.  Background
    // subtraction (background.hip): the model, one u16 per pixel of one tick, six count words, and the blob pass's scratch.
    lsn::TemporalSetting tp_setting;
    lsn::StageState tp{4, 0};
    int tp_last = 0;
    lsn::BackgroundSetting bg_setting;
    lsn::StageState bg{2, 16};
    lsn::DevBuf bg_blob;
    int bg_last = 0;
    // the three stages on the merged mesh (render.hip, simplify.hip, normals.hip): each one's scratch, allocated on its first call
    lsn::RenderScratch rv;
    lsn::SimplifyScratch sp;
    lsn::FragmentsScratch fr;            // (fragments.hip: the fourth stage on the merged mesh)
    lsn::NormalsScratch nm;
    lsn::SmoothScratch sm;               // (smooth.hip: the stage that moves vertices)
    bool thr_valid = false;
    bool thr_enabled = true;             // $LSN_NO_THRESHOLDS=1 keeps the arithmetic count pass (ablation / tests)
    bool one_tick_single_pass = false;   // a one-tick plan of <= 2048 tiles takes the single pass (fuse_kernel<4>) instead of count -> scan -> write; $LSN_ONE_TICK_SINGLE_PASS=0 / 1 forces
    bool lazy_rgb = true;                // the write pass loads colours only where a lane kept a pixel; $LSN_LAZY_RGB=0 loads them with the depth (ablation)
    int runs_with_params = 0;
    std::vector<float> last_intr, last_wt;
    float thr_build_ms = 0;
    // dominant-kernel timing
    bool profile = false;
    int profile_every = 1;               // ... of every launch, or of every n-th (lsnFusionProfile(plan, n)): two event records cost ~2 us each on the stream
    unsigned long long profile_seq = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    size_t ev_used = 0;
    double acc_ms = 0;
    long long launches = 0;
    const char *timed_kernel = nullptr;  // which kernel the event pairs bracket (set by the entry point that records them)
    std::mutex mu;
};

namespace lsn {
// Whether a call on these buffers takes the wide-load kernels (16-B depth / 8-B colour loads): the rig allows it (vec_ok), the buffers
// are aligned and so is every tick's start inside them.  Every pass of a call, and the triangulation that reads the map its vertex
// pass wrote, must agree on it: this is the one place it is decided.
inline bool wide_loads(const LsnFusion *p, const void *d_depth, const void *d_colors)
{
    return p->vec_ok && ((uintptr_t)d_depth & 15) == 0 && ((uintptr_t)d_colors & 7) == 0 && (p->tick_depth_elems % 8) == 0;
}
// The pixel -> vertex map the next vertex pass fills (p->mu held): 5 bytes per 8 pixels when it runs its wide-load form, else one int per pixel.
inline int reserve_pixmap(LsnFusion *p, bool vec)
{
    const size_t px = (size_t)p->cap * p->n_ticks;
    if (vec ? (p->pm_first.reserve(sizeof(int) * (px / 8 + 2)) || p->pm_mask.reserve(px / 8 + 2)) : p->pixmap.reserve(sizeof(int) * px)) return -1;
    p->pixmap_compact = vec;   // the triangulation reads the form that pass writes
    return 0;
}
// Kernel arguments of one call (everything but the scratch selection of the launch form); with_pixmap: the write pass also fills the
// pixel -> vertex map (reserve_pixmap).
void fill_args(LsnFusion *p, FuseArgs &a, const void *d_depth, const void *d_colors, void *d_vertices, int *d_offsets, bool with_pixmap);
// Called at the top of every run (p->mu held): builds the per-pixel depth thresholds on the second run with unchanged parameters.
int ensure_thresholds(LsnFusion *p, hipStream_t s);
// The count pass of one batch into a.tile_counts (from the thresholds when they exist, else arithmetically), then the scan: exclusive
// prefixes in place, the offset table to a.offsets and, when given, to `mirror` (pinned host memory).
void count_and_scan(LsnFusion *p, bool vec, hipStream_t s, const FuseArgs &a, int *mirror = nullptr);
// Next HIP-event pair of the dominant-kernel timer (profiling on).
int next_event_pair(LsnFusion *p, hipEvent_t &e0, hipEvent_t &e1);
// whether the dominant kernel of the launch sequence being queued is timed (profiling on, and this launch's turn)
inline bool timed_launch(LsnFusion *p) { return p->profile && (p->profile_every <= 1 || p->profile_seq++ % (unsigned long long)p->profile_every == 0); }
}  // namespace lsn
using lsn::ensure_thresholds;
using lsn::fill_args;
using lsn::count_and_scan;
using lsn::reserve_pixmap;
using lsn::wide_loads;
using lsn::next_event_pair;
using lsn::timed_launch;
