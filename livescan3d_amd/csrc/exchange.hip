// exchange.hip -- the multi-GPU exchange step: survivor exchange (pack_kernel / recon_kernel) and the vertex exchange's
// packing pass (merge_shards_kernel).  Shares the plan and the per-pixel arithmetic of fusion.hip (fusion_shared.hpp).  One translation
// unit of two files: this one holds the kernels, their launchers (lsn::pack_survivors, lsn::reconstruct, lsn::merge_shards) and the
// exports built on them, and includes, at its end, shard.hip (host code only: the dlopen()ed RCCL binding, LsnShard and lsnShardStep,
// which calls the three launchers).
#include "fusion_shared.hpp"

namespace {

// The gathered offset tables [n_shards][n_ticks][maps_per_shard + 1]: shard q's row of one tick, and the row's last entry -- the shard's
// vertices (or survivors) in that tick.  The kernels read them on the device, lsnShardStep (shard.hip) in the pinned copy of the tables.
__host__ __device__ inline const int *offset_row(const int *off, int n_ticks, int mps, long long q, int tick) { return off + (q * n_ticks + tick) * (mps + 1); }
__host__ __device__ inline int tick_total(const int *off, int n_ticks, int mps, long long q, int tick) { return offset_row(off, n_ticks, mps, q, tick)[mps]; }

// (the launchers fill the three argument structs of this file by aggregate initialisation: the members' order is part of them)
struct MergeArgs {
    const uint4 *shards;     // [n_shards][n_ticks][shard_cap]
    const int *shard_off;    // [n_shards][n_ticks][maps_per_shard + 1]  (the gathered lsnFusionRun offsets)
    uint4 *merged;           // [n_ticks][merged_cap]
    int *merged_off;         // [n_ticks][n_shards * maps_per_shard + 1]
    long long shard_cap, merged_cap;
    int n_shards, n_ticks, maps_per_shard;
    int tick_major;          // shards laid out [n_ticks][n_shards][shard_cap] instead (what per-tick all-gathers produce)
};

__global__ __launch_bounds__(kThreads) void merge_shards_kernel(const MergeArgs a)
{
    const int tick = blockIdx.y / a.n_shards;
    const int shard = blockIdx.y - tick * a.n_shards;
    int base = 0;
    for (int r = 0; r < shard; r++) base += tick_total(a.shard_off, a.n_ticks, a.maps_per_shard, r, tick);
    const int *my_off = offset_row(a.shard_off, a.n_ticks, a.maps_per_shard, shard, tick);
    const int count = my_off[a.maps_per_shard];
    const uint4 *src = a.shards + (a.tick_major ? (long long)tick * a.n_shards + shard : (long long)shard * a.n_ticks + tick) * a.shard_cap;
    uint4 *dst = a.merged + (long long)tick * a.merged_cap + base;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < count; i += gridDim.x * kThreads)
        store_vertex(dst + i, src[i]);                        // streaming stores, like the write kernel (kNontemporalStores)
    if (blockIdx.x == 0 && threadIdx.x <= a.maps_per_shard) {
        int *mo = a.merged_off + (long long)tick * (a.n_shards * a.maps_per_shard + 1);
        if (threadIdx.x < a.maps_per_shard) mo[shard * a.maps_per_shard + threadIdx.x] = base + my_off[threadIdx.x];
        else if (shard == a.n_shards - 1) mo[a.n_shards * a.maps_per_shard] = base + count;
    }
}

// ---- survivor exchange (multi-GPU): ship what the vertices are made of ---------------------------------------------------------
// A vertex is 16 bytes, the inputs it is computed from are 5 (u16 depth + RGB8) plus one bit of "this pixel survived".
// pack_kernel writes a shard's survivors as compact depth / colour streams in vertex order and the survivor mask;
// after the all-gather recon_kernel rebuilds every sensor's vertices on every GPU with the same arithmetic as
// fuse_kernel<1> (same helpers, same rounding) straight into the merged cloud.  Only for plans on the wide-load path
// (all widths multiples of 8) with identically sized sensors; other rigs exchange vertices (merge_shards_kernel).
struct PackArgs {
    unsigned char *mask;      // [n_ticks][cap / 8]      bit (p & 7) of byte p >> 3 = pixel p of the tick survived
    unsigned short *depth_c;  // [n_ticks][cap]          survivors' depth, vertex order
    unsigned char *rgb_c;     // [n_ticks][cap][3]       survivors' colour, vertex order
    const int *tick_base;     // null: tick k's survivors start at k * cap (layout above).  Else [n_ticks]: they start at tick_base[k] --
                              // all ticks back to back, ONE contiguous run per shard: what the RCCL all-gather sends as it is
};

// The survivors of a tile are staged in LDS in rank order and leave as 16-byte stores (the first version had every lane store
// its own short run: 32 one- and two-byte stores per lane, 0.32 ms per 64 ticks x 8 sensors against 0.14 at the copy rate).
__global__ __launch_bounds__(kThreads) void pack_kernel(const FuseArgs a, const PackArgs pk)
{
    __shared__ alignas(16) unsigned short s_d[kTile + 8];
    __shared__ alignas(16) unsigned char s_c[3 * kTile + 16];
    __shared__ int s_wave_tot[4];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int tick = blockIdx.x / a.tiles_per_tick;
    const int tile = blockIdx.x - tick * a.tiles_per_tick;
    const Tile t = locate(a, tick, tile);
    Inputs in;
    load_inputs<true, true>(t, in);
    const SensorParams P = a.params[t.f];
    float xf[kPxPerLane], yf[kPxPerLane];
    tile_factors<true>(t, xf, yf);
    bool keep[kPxPerLane];
    uint4 unused[kPxPerLane];
    compute_pixels<false>(a, P, in, xf, yf, keep, unused);
    int below, wave_total;
    rank_from_masks(keep, below, wave_total);
    if (lane == 0) s_wave_tot[wave] = wave_total;
    const int base = a.tile_counts[blockIdx.x];               // exclusive prefix inside the tick (scan_kernel)
    const long long r0 = (pk.tick_base ? (long long)pk.tick_base[tick] : tick * a.tick_vert_stride) + base;   // the tile's first stream entry
    __syncthreads();
    int wave_off = 0, tile_tot = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int v = s_wave_tot[i];
        if (i < wave) wave_off += v;
        tile_tot += v;
    }
    const int p0 = t.px0 + threadIdx.x * kPxPerLane;
    unsigned short *gd = pk.depth_c + r0;
    unsigned char *gc = pk.rgb_c + 3 * r0;
    const int lead_d = (int)(reinterpret_cast<uintptr_t>(gd) & 15), lead_c = (int)(reinterpret_cast<uintptr_t>(gc) & 15);   // bytes
    if (p0 < t.npix) {
        unsigned int m8 = 0;
#pragma unroll
        for (int k = 0; k < kPxPerLane; k++) m8 |= (keep[k] ? 1u : 0u) << k;
        pk.mask[(tick * a.tick_depth_stride + t.pix_base + p0) >> 3] = (unsigned char)m8;
        int e = wave_off + below;
#pragma unroll
        for (int k = 0; k < kPxPerLane; k++) {
            if (keep[k]) {
                const int b = 3 * k;
                const unsigned int lo = in.cw[b >> 2], hi = in.cw[(b >> 2) + 1 < 6 ? (b >> 2) + 1 : 5];
                const unsigned int rgb = __funnelshift_r(lo, hi, (b & 3) * 8);
                s_d[lead_d / 2 + e] = (unsigned short)((k & 1) ? in.dw[k >> 1] >> 16 : in.dw[k >> 1] & 0xFFFFu);
                unsigned char *c = s_c + lead_c + 3 * e;
                c[0] = (unsigned char)rgb;
                c[1] = (unsigned char)(rgb >> 8);
                c[2] = (unsigned char)(rgb >> 16);
                e++;
            }
        }
    }
    __syncthreads();
    store_run<2>(gd, s_d, lead_d, 2 * tile_tot);
    store_run<1>(gc, s_c, lead_c, 3 * tile_tot);
}

struct ReconArgs {
    const unsigned char *mask;       // [n_shards][n_ticks][cap_loc / 8]
    const unsigned short *depth_c;   // [n_shards][n_ticks][slab]
    const unsigned char *rgb_c;      // [n_shards][n_ticks][slab][3]
    const int *tile_prefix;          // [n_shards][n_ticks][tiles_loc]
    const int *shard_off;            // [n_shards][n_ticks][maps_per_shard + 1]
    int *merged_off;                 // [n_ticks][n_maps + 1]
    long long slab, cap_loc;
    int tiles_loc, n_shards, maps_per_shard;
    const int *tick_base;            // null: streams laid out [n_shards][n_ticks][slab].  Else [n_shards][n_ticks]: shard q's streams are ONE
                                     // run of `slab` entries, tick k's survivors start at tick_base[q][k] inside it
    int tick0;                       // first tick of this launch (a launch may cover a chunk of the ticks: the streams passed then
                                     // start at tick0's survivors, `slab` entries per shard for the chunk)
};

// Exclusive prefix over the ticks of every shard's per-tick survivor count (the last entry of its offset rows): where each
// tick starts in a shard's back-to-back streams.  One workgroup per shard.
__global__ __launch_bounds__(kThreads) void tick_base_kernel(const int *shard_off /* [n_shards][n_ticks][mps + 1] */, int n_ticks, int mps,
                                                             int *tick_base /* [n_shards][n_ticks] */)
{
    __shared__ int s_wave[kThreads / 64];
    const int *totals = offset_row(shard_off, n_ticks, mps, blockIdx.x, 0) + mps;   // tick_total(.., blockIdx.x, k) = totals[k * (mps + 1)]
    block_scan_array_excl<int, kThreads>(totals, mps + 1, tick_base + (long long)blockIdx.x * n_ticks, n_ticks, s_wave);
}

// `a` describes the WHOLE rig (all sensors, their parameters, a.out = the merged cloud).
// Two phases per tile.  Pixel-major: the survivor mask gives every lane the ranks of its 8 pixels, and the kept pixels leave their
// (column, row) in LDS at their rank.  Survivor-major: thread i takes survivors i, i + 256, ... -- consecutive threads read
// consecutive entries of the shard's compact depth / colour streams and write consecutive 16-byte vertices, so neither the
// gathers nor the stores need staging (the first version kept the pixel-major layout of the write kernel throughout: every lane
// fetched its own short run of the streams, 32 scattered 1- and 2-byte loads per lane, and staged the vertices through LDS:
// 0.37 ms per 64 ticks x 8 sensors against the 0.2 ms its 1.28 GB take at the copy rate).
struct ReconGeom {   // wave-uniform
    Tile t;
    int tick, shard, local_tile;
    long long st, mask_pix0;
};

__device__ __forceinline__ ReconGeom recon_geom(const FuseArgs &a, const ReconArgs &r, int b)
{
    ReconGeom g;
    g.tick = b / a.tiles_per_tick + r.tick0;
    const int tile = b - (g.tick - r.tick0) * a.tiles_per_tick;
    g.t = locate(a, g.tick, tile);
    g.shard = g.t.f / r.maps_per_shard;
    const FrameDesc f0 = a.frames[g.shard * r.maps_per_shard];   // first sensor of the owning shard
    g.st = (long long)g.shard * a.n_ticks + g.tick;              // (shard, tick) slot in the gathered arrays
    g.local_tile = tile - f0.tile_start;
    g.mask_pix0 = g.st * r.cap_loc + (g.t.pix_base - f0.depth_off) + g.t.px0;
    return g;
}

// Measured and dropped: a persistent form (a workgroup walks tiles b, b + grid, ... and fetches the next tile's mask byte and
// prefixes ahead) -- 0.50-0.66 ms: loads and stores share one in-order counter on this GPU, so the next tile's gathers wait
// for the previous tile's 16-byte stores to be acknowledged.
__global__ __launch_bounds__(kThreads, 8) void recon_kernel(const FuseArgs a, const ReconArgs r)
{
    __shared__ unsigned int s_xy[kTile];   // (column | row << 16) of the tile's survivors, by rank
    __shared__ int s_wave_tot[4];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const ReconGeom g = recon_geom(a, r, blockIdx.x);
    const Tile &t = g.t;
    const int p0 = t.px0 + threadIdx.x * kPxPerLane;
    const unsigned int m8 = p0 < t.npix ? r.mask[(g.mask_pix0 + threadIdx.x * kPxPerLane) >> 3] : 0u;
    const int tile_base = r.tile_prefix[g.st * r.tiles_loc + g.local_tile];
    int shard_base = 0;
    for (int q = 0; q < g.shard; q++) shard_base += tick_total(r.shard_off, a.n_ticks, r.maps_per_shard, q, g.tick);
    const SensorParams P = a.params[t.f];
    bool keep[kPxPerLane];
#pragma unroll
    for (int k = 0; k < kPxPerLane; k++) keep[k] = (m8 >> k) & 1u;
    int below, wave_total;
    rank_from_masks(keep, below, wave_total);
    if (lane == 0) s_wave_tot[wave] = wave_total;
    int x, y;
    lane_origin(t, x, y);
    __syncthreads();
    int wave_off = 0, tile_tot = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int v = s_wave_tot[i];
        if (i < wave) wave_off += v;
        tile_tot += v;
    }
    {
        int e = wave_off + below;   // w % 8 == 0: the lane's 8 pixels share row y, columns x .. x + 7
#pragma unroll
        for (int k = 0; k < kPxPerLane; k++)
            if (keep[k]) s_xy[e++] = (unsigned int)(x + k) | ((unsigned int)y << 16);
    }
    if (t.frame_start && threadIdx.x == 0) {
        int *mo = r.merged_off + (long long)g.tick * (a.n_frames + 1);
        mo[t.f] = shard_base + tile_base;             // the frame's first tile: its prefix is the sensor's offset in the shard
        if (t.f == a.n_frames - 1) {
            int total = 0;
            for (int q = 0; q < r.n_shards; q++) total += tick_total(r.shard_off, a.n_ticks, r.maps_per_shard, q, g.tick);
            mo[a.n_frames] = total;
        }
    }
    __syncthreads();
    // the tile's survivors are consecutive entries of the shard's compact streams
    const long long run = r.tick_base ? (long long)g.shard * r.slab + (r.tick_base[g.st] - r.tick_base[(long long)g.shard * a.n_ticks + r.tick0])
                                      : g.st * r.slab;
    const unsigned short *dc = r.depth_c + run + tile_base;
    const unsigned char *cc = r.rgb_c + 3 * (run + tile_base);
    uint4 *dst = a.out + g.tick * a.tick_vert_stride + shard_base + tile_base;
    // all of a thread's (<= 8) survivors are fetched before the first one is evaluated: one memory round trip
    unsigned int d[kPxPerLane], c[kPxPerLane];
    float xf[kPxPerLane], yf[kPxPerLane];
#pragma unroll
    for (int i = 0; i < kPxPerLane; i++) {
        const int e = threadIdx.x + i * kThreads;
        d[i] = 0;
        c[i] = 0;
        unsigned int xy = 0;
        if (e < tile_tot) {
            xy = s_xy[e];
            d[i] = dc[e];
            c[i] = cc[3 * e] | (cc[3 * e + 1] << 8) | (cc[3 * e + 2] << 16);
        }
        xf[i] = t.xt[xy & 0xFFFFu];
        yf[i] = t.yt[xy >> 16];
    }
#pragma unroll
    for (int i = 0; i < kPxPerLane; i += 2) {
        f2 ox, oy, oz;
        unproject2(f2{(float)d[i], (float)d[i + 1]}, f2{xf[i], xf[i + 1]}, f2{yf[i], yf[i + 1]}, P, ox, oy, oz);
        const int e0 = threadIdx.x + i * kThreads, e1 = e0 + kThreads;
        if (e0 < tile_tot) store_vertex(dst + e0, make_uint4(c[i] | 0xFF000000u, __float_as_uint(ox.x), __float_as_uint(oy.x), __float_as_uint(oz.x)));
        if (e1 < tile_tot) store_vertex(dst + e1, make_uint4(c[i + 1] | 0xFF000000u, __float_as_uint(ox.y), __float_as_uint(oy.y), __float_as_uint(oz.y)));
    }
}

}  // namespace

extern "C" int lsnFusionTilesPerTick(const LsnFusion *p) { return p ? p->tiles_per_tick : 0; }

// Survivor exchange, sender side: count + scan as in lsnFusionRun, then the compact streams instead of vertices.
// d_tick_base (nullable, [n_ticks]): filled with every tick's start in the back-to-back layout, which the streams then use.
int lsn::pack_survivors(LsnFusion *p, const void *d_depth, const void *d_colors, void *d_mask, void *d_depth_c, void *d_rgb_c,
                        int *d_tile_prefix, int *d_offsets, int *d_tick_base, void *stream)
{
    if (!p || !d_depth || !d_colors || !d_mask || !d_depth_c || !d_rgb_c || !d_offsets || (!d_tile_prefix && !d_tick_base)) {
        lsn::set_error("lsnFusionPackSurvivors: null argument");
        return -1;
    }
    if (!p->params_set) {
        lsn::set_error("lsnFusionPackSurvivors: lsnFusionSetParams has not been called");
        return -1;
    }
    std::lock_guard<std::mutex> g(p->mu);
    LSN_HIP(hipSetDevice(p->device));
    hipStream_t s = lsn::as_stream(stream);
    if (!wide_loads(p, d_depth, d_colors)) {
        lsn::set_error("lsnFusionPackSurvivors: needs frame widths that are multiples of 8 and 16-byte aligned buffers (exchange vertices instead)");
        return -1;
    }
    if (ensure_thresholds(p, s)) return -1;
    FuseArgs a;
    fill_args(p, a, d_depth, d_colors, nullptr, d_offsets, false);
    count_and_scan(p, true, s, a);
    const PackArgs pk{static_cast<unsigned char *>(d_mask), static_cast<unsigned short *>(d_depth_c), static_cast<unsigned char *>(d_rgb_c), d_tick_base};
    if (d_tick_base) hipLaunchKernelGGL(tick_base_kernel, dim3(1), dim3(kThreads), 0, s, (const int *)d_offsets, p->n_ticks, p->n_maps, d_tick_base);
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)(p->tiles_per_tick * p->n_ticks)), dim3(kThreads), 0, s, a, pk);
    LSN_HIP(hipGetLastError());
    // (LsnShard sends the prefixes straight from the plan's scratch and passes no copy target)
    if (d_tile_prefix)
        LSN_HIP(hipMemcpyAsync(d_tile_prefix, p->tile_counts.p, sizeof(int) * (size_t)p->tiles_per_tick * p->n_ticks, hipMemcpyDeviceToDevice, s));
    return 0;
}

// The four exports of the two ends share one guarded body; the Run forms (the back-to-back layout) add their own null check.
template <class F>
static int exchange_export(const char *name, bool run_argument_missing, F &&call)
{
    return lsn::guarded(name, -1, [&]() {
        lsn::clear_error();
        if (run_argument_missing) {
            lsn::set_error("%s: null argument", name);
            return -1;
        }
        return call();
    });
}

extern "C" int lsnFusionPackSurvivors(LsnFusion *p, const void *d_depth, const void *d_colors, void *d_mask, void *d_depth_c, void *d_rgb_c,
                                      int *d_tile_prefix, int *d_offsets, void *stream)
{
    return exchange_export("lsnFusionPackSurvivors", false, [&]() {
        return lsn::pack_survivors(p, d_depth, d_colors, d_mask, d_depth_c, d_rgb_c, d_tile_prefix, d_offsets, nullptr, stream);
    });
}

extern "C" int lsnFusionPackSurvivorsRun(LsnFusion *p, const void *d_depth, const void *d_colors, void *d_mask, void *d_depth_c, void *d_rgb_c,
                                         int *d_tile_prefix, int *d_offsets, int *d_tick_base, void *stream)
{
    return exchange_export("lsnFusionPackSurvivorsRun", !d_tick_base || !d_tile_prefix, [&]() {
        return lsn::pack_survivors(p, d_depth, d_colors, d_mask, d_depth_c, d_rgb_c, d_tile_prefix, d_offsets, d_tick_base, stream);
    });
}

// Survivor exchange, receiver side: `all` is a plan over the WHOLE rig (every sensor, lsnFusionSetParams called with all
// parameters, same n_ticks); the gathered arrays hold n_shards equally shaped shards of maps_per_shard sensors each.
extern "C" int lsnFusionReconstruct(LsnFusion *all, int n_shards, int maps_per_shard, const void *d_masks, const void *d_depth_c,
                                    const void *d_rgb_c, long long slab, const int *d_tile_prefix, const int *d_shard_offsets,
                                    void *d_merged, int *d_merged_offsets, void *stream)
{
    return exchange_export("lsnFusionReconstruct", false, [&]() {
        return lsn::reconstruct(all, n_shards, maps_per_shard, d_masks, d_depth_c, d_rgb_c, slab, d_tile_prefix, d_shard_offsets, d_merged,
                                d_merged_offsets, nullptr, stream);
    });
}

extern "C" int lsnFusionReconstructRun(LsnFusion *all, int n_shards, int maps_per_shard, const void *d_masks, const void *d_depth_c,
                                       const void *d_rgb_c, long long run_len, const int *d_tile_prefix, const int *d_shard_offsets,
                                       void *d_merged, int *d_merged_offsets, int *d_tick_base_scratch, void *stream)
{
    return exchange_export("lsnFusionReconstructRun", !d_tick_base_scratch, [&]() {
        return lsn::reconstruct(all, n_shards, maps_per_shard, d_masks, d_depth_c, d_rgb_c, run_len, d_tile_prefix, d_shard_offsets, d_merged,
                                d_merged_offsets, d_tick_base_scratch, stream);
    });
}

// d_tick_base (nullable, scratch [n_shards][n_ticks]): the gathered streams are one back-to-back run of `slab` entries per shard
// (lsn::pack_survivors with a tick base); the per-shard tick starts are recomputed here from the gathered offset tables.
int lsn::reconstruct(LsnFusion *all, int n_shards, int maps_per_shard, const void *d_masks, const void *d_depth_c, const void *d_rgb_c,
                     long long slab, const int *d_tile_prefix, const int *d_shard_offsets, void *d_merged, int *d_merged_offsets,
                     int *d_tick_base, void *stream, lsn::ReconChunk chunk)
{
    if (!all || !d_masks || !d_depth_c || !d_rgb_c || !d_tile_prefix || !d_shard_offsets || !d_merged || !d_merged_offsets) {
        lsn::set_error("lsnFusionReconstruct: null argument");
        return -1;
    }
    if (!all->params_set) {
        lsn::set_error("lsnFusionReconstruct: lsnFusionSetParams has not been called on the whole-rig plan");
        return -1;
    }
    std::lock_guard<std::mutex> g(all->mu);
    if (n_shards <= 0 || maps_per_shard <= 0 || n_shards * maps_per_shard != all->n_maps || slab <= 0) {
        lsn::set_error("lsnFusionReconstruct: %d shards x %d sensors do not make the plan's %d sensors", n_shards, maps_per_shard, all->n_maps);
        return -1;
    }
    for (int i = 1; i < all->n_maps; i++)
        if (all->w[i] != all->w[0] || all->h[i] != all->h[0]) {
            lsn::set_error("lsnFusionReconstruct: the survivor exchange needs identically sized sensors");
            return -1;
        }
    if (!all->vec_ok || (all->tick_depth_elems % 8) != 0 || ((uintptr_t)d_merged & 15) != 0) {
        lsn::set_error("lsnFusionReconstruct: needs frame widths that are multiples of 8 and a 16-byte aligned output");
        return -1;
    }
    LSN_HIP(hipSetDevice(all->device));
    FuseArgs a;
    fill_args(all, a, nullptr, nullptr, d_merged, d_merged_offsets, false);
    a.thr = nullptr;
    const ReconArgs r{static_cast<const unsigned char *>(d_masks), static_cast<const unsigned short *>(d_depth_c), static_cast<const unsigned char *>(d_rgb_c),
                      d_tile_prefix, d_shard_offsets, d_merged_offsets, slab, /* cap_loc */ all->cap / n_shards,
                      /* tiles_loc */ all->tiles_per_tick / n_shards, n_shards, maps_per_shard, d_tick_base, chunk.tick0};
    const int n_chunk_ticks = chunk.n_ticks > 0 ? chunk.n_ticks : all->n_ticks - chunk.tick0;
    if (chunk.tick0 < 0 || chunk.tick0 + n_chunk_ticks > all->n_ticks || (chunk.tick0 != 0 && !d_tick_base)) {
        lsn::set_error("lsnFusionReconstruct: bad tick range");
        return -1;
    }
    if (d_tick_base && chunk.fill_tick_base)
        hipLaunchKernelGGL(tick_base_kernel, dim3((unsigned)n_shards), dim3(kThreads), 0, lsn::as_stream(stream), d_shard_offsets, all->n_ticks,
                           maps_per_shard, d_tick_base);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (timed_launch(all)) {
        if (next_event_pair(all, e0, e1)) return -1;
        all->timed_kernel = "recon_kernel";
        LSN_HIP(hipEventRecord(e0, lsn::as_stream(stream)));
    }
    hipLaunchKernelGGL(recon_kernel, dim3((unsigned)(all->tiles_per_tick * n_chunk_ticks)), dim3(kThreads), 0, lsn::as_stream(stream), a, r);
    if (e1) LSN_HIP(hipEventRecord(e1, lsn::as_stream(stream)));
    LSN_HIP(hipGetLastError());
    return 0;
}

extern "C" int lsnMergeShards(int device, int n_shards, int n_ticks, int maps_per_shard, const void *d_shards, long long shard_cap,
                              const int *d_shard_offsets, void *d_merged, long long merged_cap, int *d_merged_offsets, void *stream)
{
    return lsn::guarded("lsnMergeShards", -1, [&]() {
        lsn::clear_error();
        return lsn::merge_shards(device, n_shards, n_ticks, maps_per_shard, d_shards, shard_cap, d_shard_offsets, d_merged, merged_cap, d_merged_offsets,
                                 false, stream);
    });
}

int lsn::merge_shards(int device, int n_shards, int n_ticks, int maps_per_shard, const void *d_shards, long long shard_cap,
                      const int *d_shard_offsets, void *d_merged, long long merged_cap, int *d_merged_offsets, bool tick_major, void *stream)
{
    if (n_shards <= 0 || n_ticks <= 0 || maps_per_shard <= 0 || maps_per_shard >= kThreads || !d_shards || !d_shard_offsets || !d_merged ||
        !d_merged_offsets || shard_cap <= 0 || merged_cap < shard_cap) {
        lsn::set_error("lsnMergeShards: bad arguments");
        return -1;
    }
    if ((long long)n_shards * n_ticks > 65535) {
        lsn::set_error("lsnMergeShards: n_shards * n_ticks must not exceed 65535");
        return -1;
    }
    LSN_HIP(hipSetDevice(device));
    const MergeArgs a{static_cast<const uint4 *>(d_shards), d_shard_offsets, static_cast<uint4 *>(d_merged), d_merged_offsets, shard_cap, merged_cap,
                      n_shards, n_ticks, maps_per_shard, tick_major ? 1 : 0};
    long long chunks = (shard_cap + kThreads * 8 - 1) / (kThreads * 8);
    if (chunks > 256) chunks = 256;
    hipLaunchKernelGGL(merge_shards_kernel, dim3((unsigned)chunks, (unsigned)(n_shards * n_ticks)), dim3(kThreads), 0, lsn::as_stream(stream), a);
    LSN_HIP(hipGetLastError());
    return 0;
}

#include "shard.hip"   // LsnShard: the RCCL binding and lsnShardStep (host code only)
