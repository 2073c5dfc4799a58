// background.hip -- background subtraction on the raw depth maps: a learned per-pixel model of the empty scene, what matches it dropped, the
// small blobs that survive dropped too.  The stage sits behind the temporal depth filter and in front of the flying-pixel filter.  The
// reference has no such step: the stage is defined here (include/NativeUtils.h holds the exact wording, tests/background_ref.py restates it
// in numpy, the kernels are held to the restatement bit for bit, in maps, model and counts).  Compiled as part of radial.hip's translation
// unit, behind temporal.hip, with flying.hip's tile list (see the end of radial.hip).  DESIGN.md section 23.
//
// Per tick one u16 map (millimetres, 0 = no sample) per sensor; margin in 1..4095 mm, rel_q in 0..255 (1/1024), min_pixels in 0..2^24.
// Model: one u16 per pixel of ONE tick, lo = the smallest non-zero sample seen while learning, 0 = none seen.
//   learn     c != 0:  lo' = lo == 0 ? c : min(lo, c);  c == 0: unchanged.  No maps are written.
//   classify  thr = margin + floor(lo rel_q / 1024);  c != 0, lo == 0: unknown, kept;  c != 0, c + thr < lo: foreground, kept;  else out = 0.
//   blobs     (min_pixels >= 2) kept pixels of one frame and tick that are 4-neighbours are joined; label = the component's lowest raster
//             index, size = its pixel count; a kept pixel survives iff size[label] >= min_pixels.
// Only minima and integer counts: the bytes do not depend on the order in which the device takes the pixels.
//
// Shape.  Every kernel takes 128 x 16 tiles of flying.hip's list with tile_lane.hpp's lane: 8 consecutive pixels of a row.
//   learn (bg_learn_kernel): temporal_kernel's shape.  One launch per call whatever its ticks, tiles_per_tick workgroups; a lane keeps its 8
//     model values in registers as lo - 1 mod 2^16 (0 becomes 65535, "none seen" is the largest value: the rule is one unsigned minimum),
//     keeps the loads of kBgAhead ticks in flight ahead of the minimum and stores the model once.
//   classify (bg_classify_kernel): one launch over tiles x ticks.  The three counts (foreground, unknown, background) are packed per lane
//     and stored as plain words per (tick, tile) (tile_lane.hpp's tile count) with three zeros behind them.  min_pixels <= 1: that is
//     the whole stage -- no scratch, no further launch.
//   blobs, on the classified maps (non-zero = kept), kBgBlobTicks ticks at a time to bound the scratch (a `parent` and a `size` int per
//     pixel of that many ticks); an index is the pixel's position in its tick, frame offset + y w + x, so a frame's order is its raster order:
//     1. bg_local_kernel: a tile is labelled inside LDS.  The pixels start as row runs (each kept pixel points at the first pixel of its
//        run in the tile's row, found from the lanes' masks with a ballot), then one union per run of vertically adjacent kept pairs, by
//        union_find.hpp's lock-free union on the LDS words; parent[p] = the index of the tile-local root (p itself where p is not kept),
//        size[p] = 0 -- for the lanes that hold a kept pixel; the others' words are neither written nor ever read.
//     2. bg_border_kernel: one lane per pixel of a tile's top row and left column joins it with its kept neighbour across the tile's edge
//        (one union per run of kept pairs along the edge), by the same union on the global words: parent[v] <= v always holds and a
//        tree's root is its lowest index.
//     3. bg_size_kernel: the flatten and the sizes in ONE launch.  Every kept pixel walks to its root -- the forest no longer changes, a
//        walk only falls in index, and a pixel's parent is its tile's root, so the walk is the chain of hooked roots alone -- and stores
//        it over its own word (a concurrent walk through that word reads the old parent or the root: an ancestor either way).  A launch
//        count that depended on the depth of the chains (pointer jumping) is not needed: the number of launches is fixed.  Sizes: a lane
//        adds its earlier runs of equal labels directly and hands its last run to the wave, where one integer atomicAdd serves each run of
//        lanes with equal labels, as fr_size_kernel does.
//     4. bg_apply_kernel: out = 0 where size[label] < min_pixels; the tile's components (its roots), removed components and removed
//        pixels go out as the (tick, tile)'s last three plain count words.
// No kernel waits for another workgroup; every loop is bounded by a size the host passes or by an index that only falls.  Plain vector
// stores and HIP atomics only.
#include "union_find.hpp"

namespace {

constexpr int kBgAhead = 8;        // ticks whose loads a learning lane keeps in flight
constexpr int kBgBlobTicks = 16;   // ticks the blob pass labels at a time: its scratch is 8 bytes per pixel of that many ticks
constexpr int kBgTilePixels = kFlyW * kFlyH;

typedef unsigned short bg_u16x8 __attribute__((ext_vector_type(8)));

struct BgArgs {
    const FrameDesc *frames;
    const TileDesc *tiles;          // the 128 x 16 tiles of one tick (flying.hip's list)
    const unsigned short *in;
    unsigned short *out;            // may be `in`
    unsigned short *model;          // [pixels per tick], in the layout of one tick's maps
    int *counts;                    // [n_ticks][tiles_per_tick][6]
    int *parent, *size;             // [ticks of a chunk][tick_stride]
    int tiles_per_tick, n_ticks;
    int tick0;                      // the blob pass: the chunk's first tick
    int margin, rel_q, min_pixels;
    long long tick_stride;          // u16 elements
};

// ---- learn ----------------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(kFlyThreads) void bg_learn_kernel(const BgArgs a)
{
    const TileLane l = tile_lane(a.frames, a.tiles[blockIdx.x]);
    if (!l.live) return;                                           // (no wave operation below)
    const int n = a.n_ticks;
    auto load = [&](int t) -> bg_u16x8 {
        return __builtin_bit_cast(bg_u16x8, load8<VEC>(a.in + (long long)t * a.tick_stride + l.pix, l.x, l.w));
    };
    bg_u16x8 ahead[kBgAhead];
#pragma unroll
    for (int k = 0; k < kBgAhead; k++) ahead[k] = k < n ? load(k) : (bg_u16x8)(0);
    // lo - 1 mod 2^16: "none seen" (0) is the largest value and a missing sample (0) never lowers the minimum
    const bg_u16x8 one = (bg_u16x8)(1);
    bg_u16x8 acc = __builtin_bit_cast(bg_u16x8, load8<VEC>(a.model + l.pix, l.x, l.w)) - one;
    for (int base = 0; base < n; base += kBgAhead) {
#pragma unroll
        for (int k = 0; k < kBgAhead; k++) {
            const int t = base + k;
            if (t >= n) break;                                     // uniform
            const bg_u16x8 cur = ahead[k];
            if (t + kBgAhead < n) ahead[k] = load(t + kBgAhead);
            acc = __builtin_elementwise_min(acc, (bg_u16x8)(cur - one));
        }
    }
    unsigned int o[8];
    unpack8(__builtin_bit_cast(uint4, (bg_u16x8)(acc + one)), o);
    store8<VEC>(a.model + l.pix, l.x, l.w, o);
}

// ---- classify -------------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(kFlyThreads) void bg_classify_kernel(const BgArgs a)
{
    __shared__ TileCount s_cnt;
    const int tid = threadIdx.x;
    const int tick = blockIdx.x / a.tiles_per_tick;
    const int tile = blockIdx.x - tick * a.tiles_per_tick;
    const TileLane l = tile_lane(a.frames, a.tiles[tile]);
    unsigned int lo_w = 0, hi_w = 0;                               // foreground | unknown << 16, background
    if (l.live) {
        unsigned int c[8], lo[8], o[8];
        unpack8(load8<VEC>(a.in + (long long)tick * a.tick_stride + l.pix, l.x, l.w), c);
        unpack8(load8<VEC>(a.model + l.pix, l.x, l.w), lo);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int thr = a.margin + (int)((lo[j] * (unsigned int)a.rel_q) >> 10);   // the product stays below 2^24
            const bool sample = c[j] != 0;
            const bool unknown = sample && lo[j] == 0;
            const bool fore = sample && lo[j] != 0 && (int)c[j] + thr < (int)lo[j];
            o[j] = (unknown || fore) ? c[j] : 0u;
            lo_w += fore ? 1u : unknown ? 0x10000u : 0u;
            hi_w += (sample && !unknown && !fore) ? 1u : 0u;
        }
        store8<VEC>(a.out + (long long)tick * a.tick_stride + l.pix, l.x, l.w, o);
    }
    tile_count_put(s_cnt, lo_w, hi_w);
    __syncthreads();
    if (tid < 6) {
        const int total = tid < 3 ? tile_count_get(s_cnt, tid) : 0;
        a.counts[(long long)blockIdx.x * 6 + tid] = total;         // (the blob pass's three words start at 0)
    }
}

// ---- blobs 1: a tile inside LDS ---------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(kFlyThreads) void bg_local_kernel(const BgArgs a)
{
    __shared__ int s_par[kBgTilePixels];
    __shared__ unsigned int s_mask[kFlyThreads];
    const int tid = threadIdx.x;
    const int slot = blockIdx.x / a.tiles_per_tick;
    const int tile = blockIdx.x - slot * a.tiles_per_tick;
    const TileDesc td = a.tiles[tile];
    const TileLane l = tile_lane(a.frames, td);
    unsigned int mask = 0;
    if (l.live) {
        unsigned int c[8];
        unpack8(load8<VEC>(a.out + (long long)(a.tick0 + slot) * a.tick_stride + l.pix, l.x, l.w), c);
#pragma unroll
        for (int j = 0; j < 8; j++) mask |= c[j] != 0 ? 1u << j : 0u;
    }
    s_mask[tid] = mask;
    {
        // Row runs, across the 16 lanes of a row (a quarter of a wave): a kept pixel points at its run's first pixel.  A lane is linked
        // when its first pixel and the last pixel of the lane before are kept; a run that enters a linked lane began in the nearest lane
        // below it that is not passed through (all 8 kept and linked itself), at the start of that lane's last run.  A row's first lane is
        // never linked, so the search never leaves the row.
        const int lane = tid & 63;
        const unsigned int before = __shfl_up(mask, 1);
        const bool linked = (tid & 15) != 0 && (mask & 1u) && (before & 0x80u);
        const unsigned long long through = __ballot(linked && mask == 0xFFu);
        const unsigned long long stops = ~through & ((1ull << lane) - 1ull);              // (non-zero where linked: the row's first lane)
        const int from = linked ? 63 - __clzll((long long)stops) : lane;
        const int last_run = tid * 8 + (mask == 0xFFu ? 0 : 32 - __clz((int)(~mask & 0xFFu)));   // behind the lane's highest pixel that is not kept
        int start = __shfl(last_run, from);
        if (!linked) start = tid * 8;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const bool kept = mask >> j & 1u;
            if (j > 0 && kept && !(mask >> (j - 1) & 1u)) start = tid * 8 + j;
            s_par[tid * 8 + j] = kept ? start : tid * 8 + j;
        }
    }
    __syncthreads();
    // one union per run of pixels that are kept here and in the row below (the pairs of a run are joined along both rows already; a run
    // that continues from the lane before is that lane's)
    if (tid < kFlyThreads - 16) {
        const unsigned int both = mask & s_mask[tid + 16];
        unsigned int heads = both & ~(both << 1);
        if ((tid & 15) != 0 && (s_mask[tid - 1] & s_mask[tid + 15] & 0x80u)) heads &= ~1u;
        while (heads) {                                            // at most 4 rounds
            const int j = __ffs((int)heads) - 1;
            heads &= heads - 1;
            (void)uf_unite(s_par, tid * 8 + j, tid * 8 + j + kFlyW);
        }
    }
    __syncthreads();
    if (mask == 0) return;                                         // (a lane without a kept pixel leaves its words unwritten: nobody reads them)
    int par[8], zero[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int r = uf_find(s_par, tid * 8 + j);                 // (a pixel that is not kept is its own root)
        // the root's position in the tick: the tile's first pixel + its row and column inside the tile
        par[j] = (int)(l.frame_off + (long long)(td.y0 + (r >> 7)) * l.w + td.x0 + (r & (kFlyW - 1)));
        zero[j] = 0;
    }
    const long long at = (long long)slot * a.tick_stride + l.pix;
    store8<VEC>(a.parent + at, l.x, l.w, par);
    store8<VEC>(a.size + at, l.x, l.w, zero);
}

// ---- blobs 2: across the tiles' edges -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFlyThreads) void bg_border_kernel(const BgArgs a)
{
    const int tid = threadIdx.x;
    if (tid >= kFlyW + kFlyH) return;
    const int slot = blockIdx.x / a.tiles_per_tick;
    const int tile = blockIdx.x - slot * a.tiles_per_tick;
    const TileDesc td = a.tiles[tile];
    const FrameDesc fd = a.frames[td.frame];
    const bool top = tid < kFlyW;
    const int x = top ? td.x0 + tid : td.x0, y = top ? td.y0 : td.y0 + (tid - kFlyW);
    if (x >= fd.w || y >= fd.h || (top ? td.y0 == 0 : td.x0 == 0)) return;
    const long long p = fd.depth_off + (long long)y * fd.w + x, q = top ? p - fd.w : p - 1;
    const unsigned short *map = a.out + (long long)(a.tick0 + slot) * a.tick_stride;
    if (map[p] == 0 || map[q] == 0) return;
    // one union per run of kept pairs along this tile's edge: the pair before this one lies in the same two tiles, where bg_local_kernel
    // has joined it with this pair on either side of the edge
    const long long back = top ? 1 : fd.w;
    if ((top ? x > td.x0 : y > td.y0) && map[p - back] != 0 && map[q - back] != 0) return;
    (void)uf_unite(a.parent + (long long)slot * a.tick_stride, (int)q, (int)p);
}

// ---- blobs 3: the labels and the sizes --------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(kFlyThreads) void bg_size_kernel(const BgArgs a)
{
    const int lane = threadIdx.x & 63;
    const int slot = blockIdx.x / a.tiles_per_tick;
    const int tile = blockIdx.x - slot * a.tiles_per_tick;
    const TileLane l = tile_lane(a.frames, a.tiles[tile]);
    int *parent = a.parent + (long long)slot * a.tick_stride, *size = a.size + (long long)slot * a.tick_stride;
    int label = -1, n = 0;                                         // the lane's last run of equal labels (-1: no kept pixel)
    if (l.live) {
        unsigned int c[8];
        int par[8];
        unpack8(load8<VEC>(a.out + (long long)(a.tick0 + slot) * a.tick_stride + l.pix, l.x, l.w), c);
        bool any = false;
#pragma unroll
        for (int j = 0; j < 8; j++) any |= c[j] != 0;
        if (any) load8<VEC>(parent + l.pix, l.x, l.w, par);   // (bg_local_kernel wrote the words of the lanes with a kept pixel)
        int from = -1;                                             // the parent the label was found from
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (c[j] == 0) continue;                               // (its word stays: the pixel itself)
            int lab = label;
            if (par[j] != from || label < 0) {
                from = par[j];
                lab = uf_find(parent, from);
            }
            par[j] = lab;
            if (lab != label) {
                if (n > 0) atomicAdd(&size[label], n);             // an earlier run of the lane
                label = lab;
                n = 0;
            }
            n++;
        }
        if (any) store8<VEC>(parent + l.pix, l.x, l.w, par);
    }
    // the lanes' last runs: one atomicAdd per run of lanes with equal labels
    const int incl = wave_scan_incl(n, lane);
    const int before = __shfl_up(label, 1);
    const bool head = lane == 0 || before != label;
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
    const int next = above ? __ffsll((long long)above) - 1 : 64;   // the next run's head
    const int upto = __shfl(incl, next - 1);
    if (head && label >= 0) atomicAdd(&size[label], upto - (incl - n));
}

// ---- blobs 4: the small components leave ----------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(kFlyThreads) void bg_apply_kernel(const BgArgs a)
{
    __shared__ TileCount s_cnt;
    const int tid = threadIdx.x;
    const int slot = blockIdx.x / a.tiles_per_tick;
    const int tile = blockIdx.x - slot * a.tiles_per_tick;
    const int tick = a.tick0 + slot;
    const TileLane l = tile_lane(a.frames, a.tiles[tile]);
    const int *parent = a.parent + (long long)slot * a.tick_stride, *size = a.size + (long long)slot * a.tick_stride;
    unsigned int lo_w = 0, hi_w = 0;                               // components | removed components << 16, removed pixels
    if (l.live) {
        unsigned int c[8];
        int par[8];
        unsigned short *map = a.out + (long long)tick * a.tick_stride + l.pix;
        unpack8(load8<VEC>(map, l.x, l.w), c);
        bool any = false;
#pragma unroll
        for (int j = 0; j < 8; j++) any |= c[j] != 0;
        if (any) load8<VEC>(parent + l.pix, l.x, l.w, par);
        int label = -1;
        bool stays = false, changed = false;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (c[j] == 0) continue;
            if (par[j] != label) {
                label = par[j];
                stays = size[label] >= a.min_pixels;
            }
            const bool root = label == (int)l.pix + j;
            lo_w += root ? (stays ? 1u : 0x10001u) : 0u;
            hi_w += stays ? 0u : 1u;
            if (!stays) {
                c[j] = 0;
                changed = true;
            }
        }
        if (changed) store8<VEC>(map, l.x, l.w, c);             // (the classified map is in place already)
    }
    tile_count_put(s_cnt, lo_w, hi_w);
    __syncthreads();
    if (tid < 3) a.counts[((long long)tick * a.tiles_per_tick + tile) * 6 + 3 + tid] = tile_count_get(s_cnt, tid);
}

// what the learning pass and the stage share: the plan's tables, the maps, the model
int bg_args(LsnFusion *p, BgArgs &a, const void *d_in, void *d_out, const unsigned short *d_model, int n_ticks)
{
    if (flying_prepare(p)) return -1;
    if ((long long)p->fl_tiles_per_tick * n_ticks > 0x7FFFFFFFll) {
        lsn::set_error("lsnFusionBackground: too many tiles");
        return -1;
    }
    a.frames = p->frames.as<FrameDesc>();
    a.tiles = p->fl_tiles.as<TileDesc>();
    a.in = static_cast<const unsigned short *>(d_in);
    a.out = static_cast<unsigned short *>(d_out);
    a.model = const_cast<unsigned short *>(d_model);
    a.counts = nullptr;
    a.parent = a.size = nullptr;
    a.tiles_per_tick = p->fl_tiles_per_tick;
    a.n_ticks = n_ticks;
    a.tick0 = 0;
    a.margin = a.rel_q = a.min_pixels = 0;
    a.tick_stride = p->tick_depth_elems;
    return 0;
}

bool bg_vec(const LsnFusion *p, const void *x, const void *y, const void *z)
{
    return p->vec_ok && (((uintptr_t)x | (uintptr_t)y | (uintptr_t)z) & 15) == 0 && (p->tick_depth_elems % 8) == 0;
}

}  // namespace

// The setting as the definition admits it; `who` names the export in the message.  margin <= 0 (off) is always admitted.
int lsn::background_setting_ok(const char *who, int margin, int rel_q, int min_pixels)
{
    if (margin <= 0) return 0;
    if (margin > 4095 || rel_q < 0 || rel_q > 255 || min_pixels < 0 || min_pixels > (1 << 24)) {
        lsn::set_error("%s: (margin %d, rel_q %d, min_pixels %d) is outside margin 1..4095 (<= 0: off), rel_q 0..255, min_pixels 0..2^24", who, margin,
                       rel_q, min_pixels);
        return -1;
    }
    return 0;
}

// The learning pass for the library's own flows (takes the plan's mutex): `n_ticks` ticks in the plan's frame layout folded into d_model.
int lsn::background_learn(LsnFusion *p, const void *d_depth, unsigned short *d_model, int n_ticks, hipStream_t s)
{
    std::lock_guard<std::mutex> g(p->mu);
    LSN_HIP(hipSetDevice(p->device));
    if (n_ticks < 1 || !d_depth || !d_model) {
        lsn::set_error("lsnFusionBackgroundLearn: bad arguments");
        return -1;
    }
    BgArgs a;
    if (bg_args(p, a, d_depth, nullptr, d_model, n_ticks)) return -1;
    if (bg_vec(p, d_depth, d_model, nullptr)) hipLaunchKernelGGL((bg_learn_kernel<true>), dim3((unsigned)a.tiles_per_tick), dim3(kFlyThreads), 0, s, a);
    else hipLaunchKernelGGL((bg_learn_kernel<false>), dim3((unsigned)a.tiles_per_tick), dim3(kFlyThreads), 0, s, a);
    LSN_HIP(hipGetLastError());
    return 0;
}

// The stage for the library's own flows (takes the plan's mutex): `n_ticks` ticks in the plan's frame layout from d_depth_in into d_depth_out
// (the same pointer: in place; any other overlap is refused) against d_model, which is only read; the counts of the call in `counts` (six
// words per tile and tick), the blob pass's scratch in `blob` (both reserved here, `blob` only when min_pixels >= 2).  A setting that is off
// copies and leaves the counts alone.
int lsn::background(LsnFusion *p, const BackgroundSetting &bs, const void *d_depth_in, void *d_depth_out, const unsigned short *d_model,
                    lsn::DevBuf &counts, lsn::DevBuf &blob, int n_ticks, hipStream_t s)
{
    std::lock_guard<std::mutex> g(p->mu);
    const int run = stage_preamble(p, "lsnFusionBackground", bs.on(), d_depth_in, d_depth_out, n_ticks, s);
    if (run <= 0) return run;
    if (background_setting_ok("lsnFusionBackground", bs.margin, bs.rel_q, bs.min_pixels) || n_ticks < 1 || !d_model) {
        if (!lsn::has_error()) lsn::set_error("lsnFusionBackground: bad arguments");
        return -1;
    }
    BgArgs a;
    if (bg_args(p, a, d_depth_in, d_depth_out, d_model, n_ticks) || counts.reserve(6 * sizeof(int) * (size_t)a.tiles_per_tick * (size_t)n_ticks)) return -1;
    const int chunk = n_ticks < kBgBlobTicks ? n_ticks : kBgBlobTicks;
    if (bs.blobs() && blob.reserve(2 * sizeof(int) * (size_t)p->tick_depth_elems * (size_t)chunk + 32)) return -1;
    a.counts = counts.as<int>();
    a.margin = bs.margin;
    a.rel_q = bs.rel_q;
    a.min_pixels = bs.min_pixels;
    const bool vec = bg_vec(p, d_depth_in, d_depth_out, d_model);
    const unsigned grid = (unsigned)(a.tiles_per_tick * n_ticks);
    if (vec) hipLaunchKernelGGL((bg_classify_kernel<true>), dim3(grid), dim3(kFlyThreads), 0, s, a);
    else hipLaunchKernelGGL((bg_classify_kernel<false>), dim3(grid), dim3(kFlyThreads), 0, s, a);
    if (bs.blobs()) {
        a.parent = blob.as<int>();
        a.size = a.parent + (((size_t)p->tick_depth_elems * (size_t)chunk + 3) & ~(size_t)3);   // (16-byte aligned like the first)
        for (int t0 = 0; t0 < n_ticks; t0 += chunk) {
            a.tick0 = t0;
            const unsigned g2 = (unsigned)(a.tiles_per_tick * (n_ticks - t0 < chunk ? n_ticks - t0 : chunk));
            if (vec) hipLaunchKernelGGL((bg_local_kernel<true>), dim3(g2), dim3(kFlyThreads), 0, s, a);
            else hipLaunchKernelGGL((bg_local_kernel<false>), dim3(g2), dim3(kFlyThreads), 0, s, a);
            hipLaunchKernelGGL(bg_border_kernel, dim3(g2), dim3(kFlyThreads), 0, s, a);
            if (vec) hipLaunchKernelGGL((bg_size_kernel<true>), dim3(g2), dim3(kFlyThreads), 0, s, a);
            else hipLaunchKernelGGL((bg_size_kernel<false>), dim3(g2), dim3(kFlyThreads), 0, s, a);
            if (vec) hipLaunchKernelGGL((bg_apply_kernel<true>), dim3(g2), dim3(kFlyThreads), 0, s, a);
            else hipLaunchKernelGGL((bg_apply_kernel<false>), dim3(g2), dim3(kFlyThreads), 0, s, a);
        }
    }
    LSN_HIP(hipGetLastError());
    return 0;
}

extern "C" int lsnFusionSetBackground(LsnFusion *p, int margin, int rel_q, int min_pixels)
{
    return lsn::guarded("lsnFusionSetBackground", -1, [&]() {
        lsn::clear_error();
        if (!p) {
            lsn::set_error("lsnFusionSetBackground: null argument");
            return -1;
        }
        if (lsn::background_setting_ok("lsnFusionSetBackground", margin, rel_q, min_pixels)) return -1;   // refused: the previous setting stays
        std::lock_guard<std::mutex> g(p->mu);
        p->bg_setting = margin >= 1 ? lsn::BackgroundSetting{margin, rel_q, min_pixels} : lsn::BackgroundSetting{};
        return 0;   // (the model stays as it is)
    });
}

extern "C" int lsnFusionBackgroundLearn(LsnFusion *p, const void *d_depth, void *stream)
{
    return lsn::guarded("lsnFusionBackgroundLearn", -1, [&]() {
        lsn::clear_error();
        if (!p || !d_depth) {
            lsn::set_error("lsnFusionBackgroundLearn: null argument");
            return -1;
        }
        hipStream_t s = lsn::as_stream(stream);
        {
            std::lock_guard<std::mutex> g(p->mu);
            LSN_HIP(hipSetDevice(p->device));
            if (p->bg.reserve((size_t)p->cap, s) || p->bg.hand_over(s)) return -1;
        }
        return lsn::background_learn(p, d_depth, p->bg.state.as<unsigned short>(), p->n_ticks, s);
    });
}

extern "C" int lsnFusionBackground(LsnFusion *p, const void *d_depth_in, void *d_depth_out, void *stream)
{
    return lsn::guarded("lsnFusionBackground", -1, [&]() {
        lsn::clear_error();
        if (!p || !d_depth_in || !d_depth_out) {
            lsn::set_error("lsnFusionBackground: null argument");
            return -1;
        }
        hipStream_t s = lsn::as_stream(stream);
        lsn::BackgroundSetting bs;
        {
            std::lock_guard<std::mutex> g(p->mu);
            bs = p->bg_setting;
            // the first call with the stage on reserves the model (nothing learned: every sample is unknown and kept); a copy leaves the
            // model and its stream as they are
            if (bs.on()) {
                LSN_HIP(hipSetDevice(p->device));
                if (p->bg.reserve((size_t)p->cap, s) || p->bg.hand_over(s)) return -1;
            }
        }
        if (lsn::background(p, bs, d_depth_in, d_depth_out, p->bg.state.as<unsigned short>(), p->bg.counts, p->bg_blob, p->n_ticks, s)) return -1;
        std::lock_guard<std::mutex> g(p->mu);
        p->bg_last = bs.on() ? 2 : 1;
        return 0;
    });
}

extern "C" int lsnFusionBackgroundReset(LsnFusion *p, void *stream)
{
    return lsn::guarded("lsnFusionBackgroundReset", -1, [&]() {
        lsn::clear_error();
        if (!p) {
            lsn::set_error("lsnFusionBackgroundReset: null argument");
            return -1;
        }
        std::lock_guard<std::mutex> g(p->mu);
        LSN_HIP(hipSetDevice(p->device));
        return p->bg.reset((size_t)p->cap, lsn::as_stream(stream));
    });
}

extern "C" int lsnFusionBackgroundModelRead(LsnFusion *p, unsigned short *h_model, void *stream)
{
    return lsn::guarded("lsnFusionBackgroundModelRead", -1, [&]() {
        lsn::clear_error();
        if (!p || !h_model) {
            lsn::set_error("lsnFusionBackgroundModelRead: null argument");
            return -1;
        }
        std::lock_guard<std::mutex> g(p->mu);
        LSN_HIP(hipSetDevice(p->device));
        return p->bg.read(h_model, (size_t)p->cap, lsn::as_stream(stream));
    });
}

extern "C" int lsnFusionBackgroundModelWrite(LsnFusion *p, const unsigned short *h_model, void *stream)
{
    return lsn::guarded("lsnFusionBackgroundModelWrite", -1, [&]() {
        lsn::clear_error();
        if (!p || !h_model) {
            lsn::set_error("lsnFusionBackgroundModelWrite: null argument");
            return -1;
        }
        std::lock_guard<std::mutex> g(p->mu);
        LSN_HIP(hipSetDevice(p->device));
        return p->bg.write(h_model, (size_t)p->cap, lsn::as_stream(stream));
    });
}

extern "C" int lsnFusionBackgroundDiagnostics(LsnFusion *p, int tick, int *foreground, int *unknown, int *background, int *components,
                                              int *components_removed, int *pixels_removed, void *stream)
{
    return lsn::guarded("lsnFusionBackgroundDiagnostics", -1, [&]() {
        lsn::clear_error();
        if (!p || tick < 0 || tick >= p->n_ticks) {
            lsn::set_error("lsnFusionBackgroundDiagnostics: bad arguments");
            return -1;
        }
        std::lock_guard<std::mutex> g(p->mu);
        if (p->bg_last == 0) {
            lsn::set_error("lsnFusionBackgroundDiagnostics: the plan has not run the stage");
            return -1;
        }
        int *const dst[6] = {foreground, unknown, background, components, components_removed, pixels_removed};
        return stage_diagnostics(p, p->bg_last == 2, p->bg, tick, 6, dst, lsn::as_stream(stream));
    });
}
