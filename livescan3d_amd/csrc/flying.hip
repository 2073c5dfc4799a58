// flying.hip -- the flying-pixel filter (LiveScanClient's KinectCapture::filterFlyingPixels, src/LiveScanClient/kinectCapture.cpp:132-174,
// with the server's bFilterFlyingPixels / nFPThreshold / nFPNeighbourhoodSize, LiveScanServer/KinectSettings.cs:34-37): the per-pixel
// stage every frame passes on the client before it is sent, here on the device in front of the radial correction.  Compiled as part of
// radial.hip's translation unit (see the end of that file).  DESIGN.md section 12.
//
// One u16 map w x h, neighbourhood r, threshold thr: an examined pixel (r <= x < w - r, r <= y < h - r; value 0 included) is removed
// (set to 0) iff MORE than N / 2 of its N = (2r+1)^2 - 1 window neighbours differ from it by MORE than thr; a neighbour of depth 0 counts
// like any other value; the border band of width r is copied through.  Every decision reads the unmodified map, so the pass is out of
// place.  The reference's third argument (maxNonFittingNeighbours) is overwritten with N / 2 before it is read: no parameter here.
// The reference compares int differences against (float)thr; |difference| <= 65535 is exact in float, so the comparison is done in ints.
//
// Shape: a stencil that reads 2 B and writes 2 B per pixel.  One workgroup of 256 lanes takes a tile of 128 x 16 pixels, one lane 8
// consecutive pixels of one row (one 16-byte load, one 16-byte store).  The tile's rows, r halo rows above and below and one 8-pixel chunk
// left and right, are staged in LDS once (16-byte loads; out-of-frame chunks are 0 -- only pixels of the border band, which are never
// examined, can see them); a lane then reads the 2r+1 rows of its window as three 16-byte LDS reads each and counts in registers.  r = 1, 2,
// 3 take this form (6.3 KB of LDS at r = 3); a larger r takes the plain form of the same kernel (R = 0), which reads every window from
// global memory -- right for any r, and (2r+1)^2 cached loads per pixel slow.  Rigs with a width that is no multiple of 8 (or unaligned
// buffers) take the element-wise loads and stores of the VEC = false forms, like the other map kernels.
// The pixels of depth != 0 a tile removes are left in a per-tile word (plain store, no atomics): lsnFusionFlyingDiagnostics adds them up.
namespace {

constexpr int kFlyW = 128, kFlyH = 16, kFlyThreads = 256;
constexpr int kFlyChunks = kFlyW / 8 + 2;   // chunks of 8 pixels per staged row: the tile's 16 and one halo chunk either side
constexpr int kFlyMaxR = 3;                 // the largest neighbourhood of the LDS form
static_assert(kFlyThreads == (kFlyW / 8) * kFlyH, "one lane per chunk of the tile");
static_assert(kFlyMaxR <= 8, "the halo is one chunk wide");

struct FlyArgs {
    const FrameDesc *frames;
    const TileDesc *tiles;        // the 128 x 16 tiles of one tick
    const unsigned short *in;
    unsigned short *out;
    int *counts;                  // [n_ticks * tiles_per_tick]: removed pixels of depth != 0
    int tiles_per_tick;
    int r, thr;
    long long tick_stride;        // u16 elements
};

template <int R, bool VEC>
__global__ __launch_bounds__(kFlyThreads) void flying_kernel(const FlyArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned short s_px[R > 0 ? (kFlyH + 2 * R) * kFlyChunks * 8 : 8];
    __shared__ int s_cnt[kFlyThreads / 64];
    const int tid = threadIdx.x;
    const int tick = blockIdx.x / a.tiles_per_tick;
    const int tile = blockIdx.x - tick * a.tiles_per_tick;
    const TileDesc td = a.tiles[tile];
    const FrameDesc fd = a.frames[td.frame];
    const int w = fd.w, h = fd.h;
    const unsigned short *src = a.in + (long long)tick * a.tick_stride + fd.depth_off;
    unsigned short *dst = a.out + (long long)tick * a.tick_stride + fd.depth_off;
    const int r = R > 0 ? R : a.r;
    const int half = ((2 * r + 1) * (2 * r + 1) - 1) / 2;
    const int thr = a.thr;

    if (R > 0) {
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
    }

    const int ry = tid >> 4, cx = tid & 15;
    const int y = td.y0 + ry, x = td.x0 + cx * 8;
    int removed = 0;
    if (y < h && x < w) {
        int c[8], nd[8];
#pragma unroll
        for (int j = 0; j < 8; j++) nd[j] = 0;
        const bool y_in = y >= r && y < h - r;
        if (R > 0) {
#pragma unroll
            for (int dy = 0; dy <= 2 * R; dy++) {
                // the lane's chunk and its two neighbours of staged row ry + dy: pixels x - 8 .. x + 15
                const uint4 *row = reinterpret_cast<const uint4 *>(s_px) + (ry + dy) * kFlyChunks + cx;
                const uint4 q[3] = {row[0], row[1], row[2]};
                const unsigned int d[12] = {q[0].x, q[0].y, q[0].z, q[0].w, q[1].x, q[1].y, q[1].z, q[1].w, q[2].x, q[2].y, q[2].z, q[2].w};
                int v[24];
#pragma unroll
                for (int k = 0; k < 12; k++) {
                    v[2 * k] = (int)(d[k] & 0xFFFFu);
                    v[2 * k + 1] = (int)(d[k] >> 16);
                }
                if (dy == 0) {   // the centre row sits R rows further down: fetch the centres first
                    const uint4 cq = reinterpret_cast<const uint4 *>(s_px)[(ry + R) * kFlyChunks + cx + 1];
                    const unsigned int cd[4] = {cq.x, cq.y, cq.z, cq.w};
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        c[2 * k] = (int)(cd[k] & 0xFFFFu);
                        c[2 * k + 1] = (int)(cd[k] >> 16);
                    }
                }
#pragma unroll
                for (int j = 0; j < 8; j++)
#pragma unroll
                    for (int dx = -R; dx <= R; dx++)
                        if (dy != R || dx != 0) nd[j] += abs(v[8 + j + dx] - c[j]) > thr ? 1 : 0;
            }
        } else {
            // the plain form: every window from global memory.  Only examined pixels read it, and theirs lies inside the frame.
#pragma unroll 1
            for (int j = 0; j < 8; j++) {
                const int xx = x + j;
                c[j] = xx < w ? src[(long long)y * w + xx] : 0;
                if (!y_in || xx < r || xx >= w - r) continue;
                int n = 0;
                for (int dy = -r; dy <= r; dy++) {
                    const unsigned short *line = src + (long long)(y + dy) * w + xx;
                    for (int dx = -r; dx <= r; dx++) n += abs((int)line[dx] - c[j]) > thr ? 1 : 0;   // (the centre itself differs by 0 ...
                }
                nd[j] = n - (0 > thr ? 1 : 0);   // ... which only counts for a negative thr: taken out again)
            }
        }
        unsigned int o[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int xx = x + j;
            const bool gone = y_in && xx >= r && xx < w - r && nd[j] > half;
            o[j] = gone ? 0u : (unsigned int)c[j];
            removed += (gone && c[j] != 0 && xx < w) ? 1 : 0;
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
    // the tile's count: wave sums, then one plain store
    // (wave_sum of wave_ops.hpp, kept written out: the call changed nothing but this kernel's instruction schedule, and r = 3 on 1024 x 1024
    // frames measured 0.7 % slower with it)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) removed += __shfl_xor(removed, m, 64);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = removed;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
#pragma unroll
        for (int k = 0; k < kFlyThreads / 64; k++) total += s_cnt[k];
        a.counts[blockIdx.x] = total;
    }
}

template <int R>
void launch_flying(bool vec, unsigned grid, hipStream_t s, const FlyArgs &a)
{
    if (vec) hipLaunchKernelGGL((flying_kernel<R, true>), dim3(grid), dim3(kFlyThreads), 0, s, a);
    else hipLaunchKernelGGL((flying_kernel<R, false>), dim3(grid), dim3(kFlyThreads), 0, s, a);
}

}  // namespace

// The plan's tile list for this pass (built by its first call; p->mu held): every frame cut into 128 x 16 tiles.
static int flying_prepare(LsnFusion *p)
{
    if (p->fl_ready) return 0;
    std::vector<TileDesc> tiles;
    p->fl_tile_frame.clear();
    for (int f = 0; f < p->n_maps; f++)
        for (int y0 = 0; y0 < p->h[f]; y0 += kFlyH)
            for (int x0 = 0; x0 < p->w[f]; x0 += kFlyW) {
                tiles.push_back(TileDesc{f, x0, y0, 0});
                p->fl_tile_frame.push_back(f);
            }
    if ((long long)tiles.size() * p->n_ticks > 0x7FFFFFFFll) {
        lsn::set_error("lsnFusionFlyingPixels: too many tiles");
        return -1;
    }
    if (p->fl_tiles.reserve(sizeof(TileDesc) * tiles.size()) || p->fl_counts.reserve(sizeof(int) * tiles.size() * (size_t)p->n_ticks)) return -1;
    LSN_HIP(hipMemcpy(p->fl_tiles.p, tiles.data(), sizeof(TileDesc) * tiles.size(), hipMemcpyHostToDevice));
    p->fl_tiles_per_tick = (int)tiles.size();
    p->fl_ready = true;
    return 0;
}

// lsnFusionFlyingPixels on a stream, for the library's own flows (takes the plan's mutex).
int lsn::flying_pixels(LsnFusion *p, int neighbourhood, int threshold, const void *d_depth_in, void *d_depth_out, hipStream_t s)
{
    std::lock_guard<std::mutex> g(p->mu);
    LSN_HIP(hipSetDevice(p->device));
    const size_t bytes = 2 * (size_t)p->cap * p->n_ticks;
    const uintptr_t x = (uintptr_t)d_depth_in, y = (uintptr_t)d_depth_out;
    if (x < y + bytes && y < x + bytes) {
        lsn::set_error("lsnFusionFlyingPixels: the output maps overlap the input maps (the filter decides on the unmodified maps: it runs out of place)");
        return -1;
    }
    p->fl_stream = s;
    if (neighbourhood <= 0) {   // off: the maps as they are
        LSN_HIP(hipMemcpyAsync(d_depth_out, d_depth_in, bytes, hipMemcpyDeviceToDevice, s));
        p->fl_last = 1;
        return 0;
    }
    if (flying_prepare(p)) return -1;
    const bool vec = p->vec_ok && (x & 15) == 0 && (y & 15) == 0 && (p->tick_depth_elems % 8) == 0;
    FlyArgs a;
    a.frames = p->frames.as<FrameDesc>();
    a.tiles = p->fl_tiles.as<TileDesc>();
    a.in = static_cast<const unsigned short *>(d_depth_in);
    a.out = static_cast<unsigned short *>(d_depth_out);
    a.counts = p->fl_counts.as<int>();
    a.tiles_per_tick = p->fl_tiles_per_tick;
    a.r = neighbourhood;
    a.thr = threshold;
    a.tick_stride = p->tick_depth_elems;
    const unsigned grid = (unsigned)((long long)p->fl_tiles_per_tick * p->n_ticks);
    switch (neighbourhood <= kFlyMaxR ? neighbourhood : 0) {
    case 1: launch_flying<1>(vec, grid, s, a); break;
    case 2: launch_flying<2>(vec, grid, s, a); break;
    case 3: launch_flying<3>(vec, grid, s, a); break;
    default: launch_flying<0>(vec, grid, s, a); break;
    }
    LSN_HIP(hipGetLastError());
    p->fl_last = 2;
    return 0;
}

extern "C" int lsnFusionFlyingPixels(LsnFusion *p, int neighbourhood, int threshold, const void *d_depth_in, void *d_depth_out, void *stream)
{
    return lsn::guarded("lsnFusionFlyingPixels", -1, [&]() {
        lsn::clear_error();
        if (!p || !d_depth_in || !d_depth_out) {
            lsn::set_error("lsnFusionFlyingPixels: null argument");
            return -1;
        }
        return lsn::flying_pixels(p, neighbourhood, threshold, d_depth_in, d_depth_out, lsn::as_stream(stream));
    });
}

extern "C" int lsnFusionFlyingDiagnostics(LsnFusion *p, int tick, int *removed_per_sensor, void *stream)
{
    return lsn::guarded("lsnFusionFlyingDiagnostics", -1, [&]() {
        lsn::clear_error();
        if (!p || tick < 0 || tick >= p->n_ticks) {
            lsn::set_error("lsnFusionFlyingDiagnostics: bad arguments");
            return -1;
        }
        std::lock_guard<std::mutex> g(p->mu);
        if (p->fl_last == 0) {
            lsn::set_error("lsnFusionFlyingDiagnostics: the plan has not run the filter");
            return -1;
        }
        LSN_HIP(hipSetDevice(p->device));
        std::vector<int> per(p->n_maps, 0);
        if (p->fl_last == 2) {
            LSN_HIP(hipStreamSynchronize(lsn::as_stream(stream)));
            if (p->fl_stream != lsn::as_stream(stream)) LSN_HIP(hipStreamSynchronize(p->fl_stream));
            if (lsn::stage_counts(p, p->fl_counts, tick, 1, per.data())) return -1;
        }
        long long total = 0;
        for (int f = 0; f < p->n_maps; f++) {
            if (removed_per_sensor) removed_per_sensor[f] = per[f];
            total += per[f];
        }
        return (int)total;
    });
}
