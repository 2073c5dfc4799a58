// depth_smooth.hip -- depth smoothing: an integer bilateral filter on the raw depth maps, between the flying-pixel filter and the radial
// correction.  The reference has no such step: the stage is defined here (include/NativeUtils.h holds the exact wording,
// tests/depth_smooth_ref.py restates it in numpy, the kernels are held to the restatement bit for bit).  Compiled as part of radial.hip's
// translation unit, behind flying.hip, whose tile list it shares (see the end of radial.hip).  DESIGN.md section 20.
//
// One u16 map w x h (millimetres, 0 = no sample), radius r in {1, 2, 3}, a spatial table ws[(2r+1)^2] and a range table wr[n_range], both
// u16 <= 4095.  A pixel c == 0 stays 0.  Otherwise every window position (|dy|, |dx| <= r, centre included) inside the frame with a value
// v != 0 and a = |v - c| < n_range contributes wt = ws[dy+r][dx+r] * wr[a]:  W = sum wt,  S = sum wt * (v - c) (64 bits),
// out = c + floor((2 S + W) / (2 W)).  Everything is an integer: the order of the sum cannot matter.
//
// Shape: flying_kernel's.  One workgroup of 256 lanes takes a tile of 128 x 16 pixels, one lane 8 consecutive pixels of one row; the tile's
// rows with r halo rows and one 8-pixel chunk either side are staged in LDS with 16-byte loads, out-of-frame chunks as 0 -- which this
// definition reads as "no sample", so the frame's border needs no case of its own.  The range table is staged in LDS once per workgroup
// (1032 u16: entries from n_range on are 0, and so is entry 1024, where every |v - c| >= 1024 and every v == 0 is sent) and gathered by
// |v - c|; a weight of 0 adds nothing to W or S, which is the same as not contributing.  The spatial weights are uniform per window
// position: they lie behind the range table in the plan's device table and are read from LDS at one address per wave.  Per tile two
// plain words are stored (no atomics): the pixels with out != in and the sum of |out - in|; lsnFusionDepthSmoothDiagnostics adds them
// up per sensor on the host.
#include <algorithm>
#include <cmath>

namespace {

constexpr int kSmoothMaxR = 3;
constexpr int kSmoothMaxRange = 1024;                 // the longest range table
constexpr int kSmoothRangeLds = kSmoothMaxRange + 8;  // staged entries: the table, zeros behind it, entry 1024 = 0 (16-byte chunks)
constexpr int kSmoothTableLen = kSmoothRangeLds + 56; // the plan's device table: the staged range entries, then the spatial table (49 used)
constexpr int kSmoothNoSample = 0x20000;              // what a staged 0 is read as: further than 1024 from every u16

struct SmoothArgs {
    const FrameDesc *frames;
    const TileDesc *tiles;        // the 128 x 16 tiles of one tick (flying.hip's list)
    const unsigned short *in;
    unsigned short *out;
    const unsigned short *table;  // [kSmoothTableLen]: the range table, zero from n_range on; behind it the spatial table, row-major over (dy, dx)
    int *counts;                  // [n_ticks * tiles_per_tick][2]: pixels with out != in, sum of |out - in|
    int tiles_per_tick;
    long long tick_stride;        // u16 elements
};

// floor((2 S + W) / (2 W)) for W >= 1, |quotient| < 1024: a float estimate (relative error of a few 2^-23, so at most one off after the
// floor) and one exact integer correction.  (The plain 64-bit division gives the same bits and takes 0.16-0.19 ms more per batch:
// EXPERIMENTS.md "Depth smoothing".)
__device__ __forceinline__ int smooth_quotient(long long S, unsigned int W)
{
    const long long num = 2 * S + (long long)W;
    const long long den = 2 * (long long)W;
    int q = (int)floorf((float)num * __builtin_amdgcn_rcpf((float)den));
    const long long rem = num - (long long)q * den;
    q += rem >= den ? 1 : 0;
    q -= rem < 0 ? 1 : 0;
    return q;
}

template <int R, bool VEC>
__global__ __launch_bounds__(kFlyThreads) void depth_smooth_kernel(const SmoothArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned short s_px[(kFlyH + 2 * R) * kFlyChunks * 8];
    __shared__ __attribute__((aligned(16))) unsigned short s_wr[kSmoothRangeLds];
    __shared__ unsigned int s_ws[(2 * R + 1) * (2 * R + 1)];
    __shared__ int s_cnt[2][kFlyThreads / 64];
    const int tid = threadIdx.x;
    const int tick = blockIdx.x / a.tiles_per_tick;
    const int tile = blockIdx.x - tick * a.tiles_per_tick;
    const TileDesc td = a.tiles[tile];
    const FrameDesc fd = a.frames[td.frame];
    const int w = fd.w, h = fd.h;
    const unsigned short *src = a.in + (long long)tick * a.tick_stride + fd.depth_off;
    unsigned short *dst = a.out + (long long)tick * a.tick_stride + fd.depth_off;

    if (tid < kSmoothRangeLds / 8) reinterpret_cast<uint4 *>(s_wr)[tid] = reinterpret_cast<const uint4 *>(a.table)[tid];
    else if (tid - kSmoothRangeLds / 8 < (2 * R + 1) * (2 * R + 1)) s_ws[tid - kSmoothRangeLds / 8] = a.table[kSmoothRangeLds + tid - kSmoothRangeLds / 8];
    for (int i = tid; i < (kFlyH + 2 * R) * kFlyChunks; i += kFlyThreads) {
        const int srow = i / kFlyChunks, sc = i - srow * kFlyChunks;
        const int gy = td.y0 - R + srow, gx = td.x0 - 8 + sc * 8;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (gy >= 0 && gy < h) {
            if (VEC) {
                if (gx >= 0 && gx < w) v = *reinterpret_cast<const uint4 *>(src + (long long)gy * w + gx);   // w % 8 == 0: a whole chunk
            } else {
                unsigned int e[8];
#pragma unroll
                for (int j = 0; j < 8; j++) e[j] = (gx + j >= 0 && gx + j < w) ? src[(long long)gy * w + gx + j] : 0u;
                v = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
            }
        }
        reinterpret_cast<uint4 *>(s_px)[i] = v;
    }
    __syncthreads();

    const int ry = tid >> 4, cx = tid & 15;
    const int y = td.y0 + ry, x = td.x0 + cx * 8;
    int changed = 0, moved = 0;
    if (y < h && x < w) {
        int c[8];
        unsigned int W[8];
        long long S[8];
        {
            const uint4 cq = reinterpret_cast<const uint4 *>(s_px)[(ry + R) * kFlyChunks + cx + 1];
            const unsigned int cd[4] = {cq.x, cq.y, cq.z, cq.w};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                c[2 * k] = (int)(cd[k] & 0xFFFFu);
                c[2 * k + 1] = (int)(cd[k] >> 16);
            }
        }
#pragma unroll
        for (int j = 0; j < 8; j++) {
            W[j] = 0;
            S[j] = 0;
        }
        // a loop over the window's rows (rolled: unrolled, the scheduler hoists every gather of the window to the top and the kernel needs all
        // 512 registers and scratch), the row's 2R+1 columns unrolled
#pragma unroll 1
        for (int dy = 0; dy <= 2 * R; dy++) {
            // the lane's chunk and its two neighbours of staged row ry + dy: pixels x - 8 .. x + 15
            const uint4 *row = reinterpret_cast<const uint4 *>(s_px) + (ry + dy) * kFlyChunks + cx;
            const uint4 q[3] = {row[0], row[1], row[2]};
            const unsigned int d[12] = {q[0].x, q[0].y, q[0].z, q[0].w, q[1].x, q[1].y, q[1].z, q[1].w, q[2].x, q[2].y, q[2].z, q[2].w};
            int v[8 + 2 * R];   // pixels x - R .. x + 7 + R; a 0 (no sample, out of frame) becomes a value no centre is near
#pragma unroll
            for (int k = 0; k < 8 + 2 * R; k++) {
                const int px = 8 - R + k;
                const int val = (px & 1) ? (int)(d[px >> 1] >> 16) : (int)(d[px >> 1] & 0xFFFFu);
                v[k] = val == 0 ? kSmoothNoSample : val;
            }
#pragma unroll
            for (int dx = 0; dx <= 2 * R; dx++) {
                const unsigned int ws = s_ws[dy * (2 * R + 1) + dx];   // one address for the wave: a broadcast
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const int delta = v[j + dx] - c[j];
                    const int idx = min(abs(delta), kSmoothMaxRange);
                    const unsigned int wt = __umul24(ws, (unsigned int)s_wr[idx]);   // both <= 4095; 0 where the position does not contribute
                    W[j] += wt;
                    S[j] += (long long)(int)wt * delta;
                }
            }
        }
        unsigned int o[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            // a centre of 0 stays 0 (its sums mean nothing: W may be 0 there)
            const int out = c[j] == 0 ? 0 : c[j] + smooth_quotient(S[j], W[j] > 0 ? W[j] : 1u);
            o[j] = (unsigned int)out;
            const int diff = x + j < w ? abs(out - c[j]) : 0;
            changed += diff != 0 ? 1 : 0;
            moved += diff;
        }
        unsigned short *dp = dst + (long long)y * w + x;
        if (VEC) {
            *reinterpret_cast<uint4 *>(dp) = make_uint4(o[0] | (o[1] << 16), o[2] | (o[3] << 16), o[4] | (o[5] << 16), o[6] | (o[7] << 16));
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (x + j < w) dp[j] = (unsigned short)o[j];
        }
    }
    // the tile's two words: wave sums, then two plain stores
    changed = wave_sum(changed);
    moved = wave_sum(moved);
    if ((tid & 63) == 0) {
        s_cnt[0][tid >> 6] = changed;
        s_cnt[1][tid >> 6] = moved;
    }
    __syncthreads();
    if (tid < 2) {
        int total = 0;
#pragma unroll
        for (int k = 0; k < kFlyThreads / 64; k++) total += s_cnt[tid][k];
        a.counts[2 * (long long)blockIdx.x + tid] = total;
    }
}

template <int R>
void launch_depth_smooth(bool vec, unsigned grid, hipStream_t s, const SmoothArgs &a)
{
    if (vec) hipLaunchKernelGGL((depth_smooth_kernel<R, true>), dim3(grid), dim3(kFlyThreads), 0, s, a);
    else hipLaunchKernelGGL((depth_smooth_kernel<R, false>), dim3(grid), dim3(kFlyThreads), 0, s, a);
}

// The tables as the definition admits them; `who` names the export in the message.
int smooth_tables_ok(const char *who, int radius, const unsigned short *spatial, const unsigned short *range, int n_range)
{
    if (radius > kSmoothMaxR) {
        lsn::set_error("%s: radius %d is outside 1..%d", who, radius, kSmoothMaxR);
        return -1;
    }
    if (!spatial || !range) {
        lsn::set_error("%s: null table", who);
        return -1;
    }
    if (n_range < 1 || n_range > kSmoothMaxRange) {
        lsn::set_error("%s: n_range %d is outside 1..%d", who, n_range, kSmoothMaxRange);
        return -1;
    }
    const int side = 2 * radius + 1;
    for (int i = 0; i < side * side; i++)
        if (spatial[i] > 4095) {
            lsn::set_error("%s: spatial[%d] = %d exceeds 4095", who, i, (int)spatial[i]);
            return -1;
        }
    for (int i = 0; i < n_range; i++)
        if (range[i] > 4095) {
            lsn::set_error("%s: range[%d] = %d exceeds 4095", who, i, (int)range[i]);
            return -1;
        }
    if (spatial[radius * side + radius] < 1 || range[0] < 1) {
        lsn::set_error("%s: the centre's spatial weight and range[0] must be at least 1", who);
        return -1;
    }
    return 0;
}

}  // namespace

extern "C" int lsnDepthSmoothGaussian(int radius, float sigma_s, float sigma_r, unsigned short *spatial_out, unsigned short *range_out, int range_cap)
{
    return lsn::guarded("lsnDepthSmoothGaussian", -1, [&]() {
        lsn::clear_error();
        if (radius < 1 || radius > kSmoothMaxR) {
            lsn::set_error("lsnDepthSmoothGaussian: radius %d is outside 1..%d", radius, kSmoothMaxR);
            return -1;
        }
        if (!std::isfinite(sigma_s) || !(sigma_s > 0.0f) || !std::isfinite(sigma_r) || !(sigma_r > 0.0f)) {
            lsn::set_error("lsnDepthSmoothGaussian: sigma_s and sigma_r must be finite and positive");
            return -1;
        }
        if (!spatial_out || !range_out || range_cap < 1) {
            lsn::set_error("lsnDepthSmoothGaussian: null table or range_cap < 1");
            return -1;
        }
        const double ss = (double)sigma_s, sr = (double)sigma_r;
        const int side = 2 * radius + 1;
        for (int dy = -radius; dy <= radius; dy++)
            for (int dx = -radius; dx <= radius; dx++)
                spatial_out[(dy + radius) * side + dx + radius] = (unsigned short)rint(4095.0 * exp(-(double)(dx * dx + dy * dy) / (2.0 * ss * ss)));
        const int cap = range_cap < kSmoothMaxRange ? range_cap : kSmoothMaxRange;
        int n = 0;
        for (; n < cap; n++) {
            const unsigned short v = (unsigned short)rint(4095.0 * exp(-((double)n * (double)n) / (2.0 * sr * sr)));
            if (v == 0) break;
            range_out[n] = v;
        }
        return n;
    });
}

int lsn::depth_smooth_gaussian(int radius, float sigma_s, float sigma_r, DepthSmoothTables &t)
{
    const int n = lsnDepthSmoothGaussian(radius, sigma_s, sigma_r, t.spatial, t.range, kSmoothMaxRange);
    if (n < 0) return -1;
    t.radius = radius;
    t.n_range = n;
    return 0;
}

// lsnFusionSetDepthSmooth for the library's own flows (takes the plan's mutex).  A setting the plan already has costs nothing; a new one
// goes into a fresh device table, and freeing the old one waits for whatever still reads it.
int lsn::set_depth_smooth(LsnFusion *p, const char *who, int radius, const unsigned short *spatial, const unsigned short *range, int n_range)
{
    std::lock_guard<std::mutex> g(p->mu);
    if (radius <= 0) {
        p->ds_radius = 0;
        return 0;
    }
    if (smooth_tables_ok(who, radius, spatial, range, n_range)) return -1;
    const int taps = (2 * radius + 1) * (2 * radius + 1);
    std::vector<unsigned short> padded((size_t)kSmoothTableLen, (unsigned short)0);
    std::copy(range, range + n_range, padded.begin());
    std::copy(spatial, spatial + taps, padded.begin() + kSmoothRangeLds);
    if (padded != p->ds_table_host) {
        LSN_HIP(hipSetDevice(p->device));
        lsn::DevBuf fresh;
        if (fresh.reserve(sizeof(unsigned short) * padded.size())) return -1;
        LSN_HIP(hipMemcpy(fresh.p, padded.data(), sizeof(unsigned short) * padded.size(), hipMemcpyHostToDevice));
        std::swap(fresh.p, p->ds_table.p);
        std::swap(fresh.bytes, p->ds_table.bytes);
        p->ds_table_host.swap(padded);
    }
    p->ds_radius = radius;
    p->ds_n_range = n_range;
    return 0;
}

// lsnFusionDepthSmooth on a stream, for the library's own flows (takes the plan's mutex).
int lsn::depth_smooth(LsnFusion *p, const void *d_depth_in, void *d_depth_out, hipStream_t s)
{
    std::lock_guard<std::mutex> g(p->mu);
    LSN_HIP(hipSetDevice(p->device));
    const size_t bytes = 2 * (size_t)p->cap * p->n_ticks;
    const uintptr_t x = (uintptr_t)d_depth_in, y = (uintptr_t)d_depth_out;
    if (x < y + bytes && y < x + bytes) {
        lsn::set_error("lsnFusionDepthSmooth: the output maps overlap the input maps (the filter reads the unmodified maps: it runs out of place)");
        return -1;
    }
    p->ds_stream = s;
    if (p->ds_radius <= 0) {   // off: the maps as they are
        LSN_HIP(hipMemcpyAsync(d_depth_out, d_depth_in, bytes, hipMemcpyDeviceToDevice, s));
        p->ds_last = 1;
        return 0;
    }
    // the tile list is the flying-pixel filter's (128 x 16 tiles of one tick); the two words per tile of every tick are this pass's own
    if (flying_prepare(p) || p->ds_counts.reserve(2 * sizeof(int) * (size_t)p->fl_tiles_per_tick * (size_t)p->n_ticks)) return -1;
    const bool vec = p->vec_ok && (x & 15) == 0 && (y & 15) == 0 && (p->tick_depth_elems % 8) == 0;
    SmoothArgs a;
    a.frames = p->frames.as<FrameDesc>();
    a.tiles = p->fl_tiles.as<TileDesc>();
    a.in = static_cast<const unsigned short *>(d_depth_in);
    a.out = static_cast<unsigned short *>(d_depth_out);
    a.table = p->ds_table.as<unsigned short>();
    a.counts = p->ds_counts.as<int>();
    a.tiles_per_tick = p->fl_tiles_per_tick;
    a.tick_stride = p->tick_depth_elems;
    const unsigned grid = (unsigned)((long long)p->fl_tiles_per_tick * p->n_ticks);
    switch (p->ds_radius) {
    case 1: launch_depth_smooth<1>(vec, grid, s, a); break;
    case 2: launch_depth_smooth<2>(vec, grid, s, a); break;
    default: launch_depth_smooth<3>(vec, grid, s, a); break;
    }
    LSN_HIP(hipGetLastError());
    p->ds_last = 2;
    return 0;
}

extern "C" int lsnFusionSetDepthSmooth(LsnFusion *p, int radius, const unsigned short *spatial, const unsigned short *range, int n_range)
{
    return lsn::guarded("lsnFusionSetDepthSmooth", -1, [&]() {
        lsn::clear_error();
        if (!p) {
            lsn::set_error("lsnFusionSetDepthSmooth: null argument");
            return -1;
        }
        return lsn::set_depth_smooth(p, "lsnFusionSetDepthSmooth", radius, spatial, range, n_range);
    });
}

extern "C" int lsnFusionDepthSmooth(LsnFusion *p, const void *d_depth_in, void *d_depth_out, void *stream)
{
    return lsn::guarded("lsnFusionDepthSmooth", -1, [&]() {
        lsn::clear_error();
        if (!p || !d_depth_in || !d_depth_out) {
            lsn::set_error("lsnFusionDepthSmooth: null argument");
            return -1;
        }
        return lsn::depth_smooth(p, d_depth_in, d_depth_out, lsn::as_stream(stream));
    });
}

extern "C" int lsnFusionDepthSmoothDiagnostics(LsnFusion *p, int tick, int *changed_per_sensor, long long *abs_change_per_sensor, void *stream)
{
    return lsn::guarded("lsnFusionDepthSmoothDiagnostics", -1, [&]() {
        lsn::clear_error();
        if (!p || tick < 0 || tick >= p->n_ticks) {
            lsn::set_error("lsnFusionDepthSmoothDiagnostics: bad arguments");
            return -1;
        }
        std::lock_guard<std::mutex> g(p->mu);
        if (p->ds_last == 0) {
            lsn::set_error("lsnFusionDepthSmoothDiagnostics: the plan has not run the filter");
            return -1;
        }
        LSN_HIP(hipSetDevice(p->device));
        std::vector<int> changed(p->n_maps, 0);
        std::vector<long long> moved(p->n_maps, 0);
        if (p->ds_last == 2) {
            std::vector<int> counts(2 * (size_t)p->fl_tiles_per_tick);
            LSN_HIP(hipStreamSynchronize(lsn::as_stream(stream)));
            if (p->ds_stream != lsn::as_stream(stream)) LSN_HIP(hipStreamSynchronize(p->ds_stream));
            LSN_HIP(hipMemcpy(counts.data(), p->ds_counts.as<int>() + 2 * (size_t)tick * p->fl_tiles_per_tick, sizeof(int) * counts.size(), hipMemcpyDeviceToHost));
            for (size_t t = 0; t < (size_t)p->fl_tiles_per_tick; t++) {
                changed[p->fl_tile_frame[t]] += counts[2 * t];
                moved[p->fl_tile_frame[t]] += counts[2 * t + 1];
            }
        }
        long long total = 0;
        for (int f = 0; f < p->n_maps; f++) {
            if (changed_per_sensor) changed_per_sensor[f] = changed[f];
            if (abs_change_per_sensor) abs_change_per_sensor[f] = moved[f];
            total += changed[f];
        }
        return (int)total;
    });
}
