// tile_lane.hpp -- what the kernels of the two stateful depth stages (temporal.hip, background.hip) share, and the opening and the count
// summation of their host calls.  Included by radial.hip behind flying.hip, whose 128 x 16 tile list and constants it builds on.
//
// The lane: one workgroup of kFlyThreads = 256 lanes takes one tile, one lane 8 consecutive pixels of a row -- two pixels a word where VEC
// holds (widths that are multiples of 8, 16-byte aligned buffers: one 16-byte load or store for u16 pixels, two for 32-bit state), else
// element by element with the pixels beyond the row's end read as 0 and never stored.
// The packed tile count: a lane counts into two words of two 16-bit fields each (a lane adds at most 8 to a field, a wave 512, the tile
// 2048: 16 bits hold it); the words are summed per wave into LDS, and behind a barrier field f of the tile is the sum of the waves'
// halves.  The fields go out as plain words per (tick, tile): no atomics.  lsn::stage_counts adds them up per frame on the host.
#pragma once

namespace {

static_assert(kFlyW == 128 && kFlyThreads * 8 == kFlyW * kFlyH, "a tile-local index is lane * 8 + j = row * 128 + column");

// What a kernel knows of its lane: the frame, the lane's first pixel and whether it lies in the frame.
struct TileLane {
    int w, h, x, y;
    bool live;
    long long frame_off, pix;       // the frame's first pixel and the lane's, inside a tick (pix is 0 for a lane outside the frame)
};

__device__ __forceinline__ TileLane tile_lane(const FrameDesc *frames, const TileDesc &td)
{
    const FrameDesc fd = frames[td.frame];
    TileLane l;
    l.w = fd.w;
    l.h = fd.h;
    l.y = td.y0 + ((int)threadIdx.x >> 4);
    l.x = td.x0 + ((int)threadIdx.x & 15) * 8;
    l.live = l.y < l.h && l.x < l.w;
    l.frame_off = fd.depth_off;
    l.pix = l.live ? fd.depth_off + (long long)l.y * l.w + l.x : 0;
    return l;
}

// A lane's 8 u16 pixels at p, two a word: into v, or as a value.  (temporal_kernel, which keeps eight of them in flight, takes the first
// form: with the value returned through the call its VEC form was compiled to 81 VGPRs, one step of occupancy below the 77 it has.)
template <bool VEC>
__device__ __forceinline__ void load8(uint4 &v, const unsigned short *p, int x, int w)
{
    if (VEC) {
        v = *reinterpret_cast<const uint4 *>(p);                   // w % 8 == 0: a whole chunk
    } else {
        unsigned int e[8];
#pragma unroll
        for (int j = 0; j < 8; j++) e[j] = x + j < w ? p[j] : 0u;
        v = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
    }
}

template <bool VEC>
__device__ __forceinline__ uint4 load8(const unsigned short *p, int x, int w)
{
    uint4 v;
    load8<VEC>(v, p, x, w);
    return v;
}

template <bool VEC>
__device__ __forceinline__ void store8(unsigned short *p, int x, int w, const unsigned int (&o)[8])
{
    if (VEC) {
        *reinterpret_cast<uint4 *>(p) = make_uint4(o[0] | (o[1] << 16), o[2] | (o[3] << 16), o[4] | (o[5] << 16), o[6] | (o[7] << 16));
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (x + j < w) p[j] = (unsigned short)o[j];
    }
}

__device__ __forceinline__ void unpack8(const uint4 v, unsigned int (&c)[8])
{
    const unsigned int d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 8; j++) c[j] = (j & 1) ? d[j >> 1] >> 16 : d[j >> 1] & 0xFFFFu;
}

// A lane's 8 words of 32-bit state (T: int or unsigned int).
template <bool VEC, class T>
__device__ __forceinline__ void load8(const T *p, int x, int w, T (&v)[8])
{
    static_assert(sizeof(T) == 4, "two 16-byte halves");
    if (VEC) {
        const uint4 a = reinterpret_cast<const uint4 *>(p)[0], b = reinterpret_cast<const uint4 *>(p)[1];
        v[0] = (T)a.x; v[1] = (T)a.y; v[2] = (T)a.z; v[3] = (T)a.w;
        v[4] = (T)b.x; v[5] = (T)b.y; v[6] = (T)b.z; v[7] = (T)b.w;
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = x + j < w ? p[j] : (T)0;
    }
}

template <bool VEC, class T>
__device__ __forceinline__ void store8(T *p, int x, int w, const T (&v)[8])
{
    static_assert(sizeof(T) == 4, "two 16-byte halves");
    if (VEC) {
        reinterpret_cast<uint4 *>(p)[0] = make_uint4((unsigned int)v[0], (unsigned int)v[1], (unsigned int)v[2], (unsigned int)v[3]);
        reinterpret_cast<uint4 *>(p)[1] = make_uint4((unsigned int)v[4], (unsigned int)v[5], (unsigned int)v[6], (unsigned int)v[7]);
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (x + j < w) p[j] = v[j];
    }
}

// The packed tile count.  Every lane of the workgroup calls tile_count_put with its two words; behind a barrier tile_count_get(s, f) is
// field f of the tile: 0 and 1 the low and high half of the first word, 2 and 3 of the second.
typedef unsigned int TileCount[kFlyThreads / 64][2];

__device__ __forceinline__ void tile_count_put(TileCount &s, unsigned int lo, unsigned int hi)
{
    lo = wave_sum(lo);
    hi = wave_sum(hi);
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) {
        s[tid >> 6][0] = lo;
        s[tid >> 6][1] = hi;
    }
}

__device__ __forceinline__ int tile_count_get(const TileCount &s, int f)
{
    int total = 0;
#pragma unroll
    for (int wv = 0; wv < kFlyThreads / 64; wv++) {
        const unsigned int word = s[wv][f >> 1];
        total += (int)((f & 1) ? word >> 16 : word & 0xFFFFu);
    }
    return total;
}

}  // namespace

int lsn::stage_preamble(LsnFusion *p, const char *who, bool on, const void *d_depth_in, void *d_depth_out, int n_ticks, hipStream_t s)
{
    LSN_HIP(hipSetDevice(p->device));
    const size_t bytes = 2 * (size_t)p->cap * (size_t)n_ticks;
    const uintptr_t x = (uintptr_t)d_depth_in, y = (uintptr_t)d_depth_out;
    if (x != y && x < y + bytes && y < x + bytes) {
        lsn::set_error("%s: the output maps overlap the input maps (the pass runs in place or on disjoint buffers)", who);
        return -1;
    }
    if (on) return 1;
    if (x != y) LSN_HIP(hipMemcpyAsync(d_depth_out, d_depth_in, bytes, hipMemcpyDeviceToDevice, s));
    return 0;
}

int lsn::stage_counts(LsnFusion *p, const lsn::DevBuf &counts, int tick, int n_fields, int *per_frame)
{
    std::vector<int> words((size_t)n_fields * (size_t)p->fl_tiles_per_tick);
    LSN_HIP(hipMemcpy(words.data(), counts.as<int>() + words.size() * (size_t)tick, sizeof(int) * words.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < n_fields * p->n_maps; i++) per_frame[i] = 0;
    for (size_t t = 0; t < (size_t)p->fl_tiles_per_tick; t++)
        for (int f = 0; f < n_fields; f++) per_frame[n_fields * p->fl_tile_frame[t] + f] += words[(size_t)n_fields * t + f];
    return 0;
}

// What the two stages' diagnostics exports end with (p->mu held): the per-frame sums of tick `tick`'s n_fields count words into
// dst[k][frame] (a null dst[k] is skipped), behind everything queued on `s` and on the stage's last stream; a last call that copied
// (`ran` false) reads as zeros.
static int stage_diagnostics(LsnFusion *p, bool ran, const lsn::StageState &st, int tick, int n_fields, int *const *dst, hipStream_t s)
{
    LSN_HIP(hipSetDevice(p->device));
    std::vector<int> per((size_t)n_fields * (size_t)p->n_maps, 0);
    if (ran) {
        LSN_HIP(hipStreamSynchronize(s));
        if (st.stream != s) LSN_HIP(hipStreamSynchronize(st.stream));
        if (lsn::stage_counts(p, st.counts, tick, n_fields, per.data())) return -1;
    }
    for (int f = 0; f < p->n_maps; f++)
        for (int k = 0; k < n_fields; k++)
            if (dst[k]) dst[k][f] = per[n_fields * f + k];
    return 0;
}
