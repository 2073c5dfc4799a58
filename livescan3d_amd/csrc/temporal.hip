// temporal.hip -- the temporal depth filter: a range-gated recursive mean across ticks on the raw depth maps, in front of the flying-pixel
// filter.  The reference has no such step: the stage is defined here (include/NativeUtils.h holds the exact wording,
// tests/temporal_ref.py restates it in numpy, the kernel is held to the restatement bit for bit, in maps and in state).  Compiled as part
// of radial.hip's translation unit, behind flying.hip, whose tile list it shares (see the end of radial.hip).  DESIGN.md section 22.
//
// Per tick one u16 map (millimetres, 0 = no sample) per sensor; alpha_q in 1..256, delta in 1..4095 mm, persist in 0..255.  State: one u32
// word per pixel, F | miss << 24 (F: the filtered depth in 1/256 mm, 0 = no history; miss: consecutive ticks served from history).  Per
// pixel and tick, with sample c:
//   blend    c != 0, F != 0, |256 c - F| <= 256 delta:  F' = F + floor((alpha_q (256 c - F) + 128) / 256), miss' = 0, out = floor((F' + 128) / 256)
//   restart  c != 0 otherwise:                          F' = 256 c, miss' = 0, out = c
//   fill     c == 0, F != 0, miss < persist:            F' = F, miss' = miss + 1, out = floor((F + 128) / 256)
//   expire / empty  c == 0 otherwise:                   the word becomes 0, out = 0
// Everything is an integer in 32 bits (the blend's product stays below 2^29); the pass is pointwise, so it may run in place.
//
// Shape: one launch per call, whatever its ticks.  One workgroup takes one 128 x 16 tile of flying.hip's list with tile_lane.hpp's lane (8
// consecutive pixels of a row); the lane loads its 8 state words, walks the call's ticks in order with the state in registers and stores
// the state once at the end: 4 B per pixel and tick, 8 B per pixel and call.  The grid is only tiles_per_tick workgroups, so the tick loop
// hides the latency itself: the samples do not depend on the state, and each lane keeps the loads of kTempAhead ticks in flight ahead of
// the arithmetic (8 x 16 B x 256 lanes = 32 KiB per workgroup).  No LDS staging of pixels, no atomics: the branch counts of a tick
// (blended, restarted with history, filled, expired) are tile_lane.hpp's packed tile count, four plain words per (tick, tile) once per
// kTempAhead ticks.  The history, its count words and the stream hand-over are a lsn::StageState (lsn_common.hpp) in whoever owns them.
namespace {

constexpr int kTempAhead = 8;   // ticks whose loads a lane keeps in flight

struct TemporalArgs {
    const FrameDesc *frames;
    const TileDesc *tiles;        // the 128 x 16 tiles of one tick (flying.hip's list)
    const unsigned short *in;
    unsigned short *out;          // may be `in`
    unsigned int *state;          // [pixels per tick], in the layout of one tick's maps
    int *counts;                  // [n_ticks][tiles_per_tick][4]: blended, restarted with history, filled, expired
    int tiles_per_tick, n_ticks;
    int alpha_q, gate, persist;   // gate = 256 delta
    long long tick_stride;        // u16 elements
};

// One pixel, one tick: the served value; `word` becomes the new state.  lo counts blended | restarted << 16, hi filled | expired << 16.
__device__ __forceinline__ unsigned int temporal_pixel(unsigned int c, unsigned int &word, int alpha_q, int gate, int persist, unsigned int &lo,
                                                       unsigned int &hi)
{
    const int F = (int)(word & 0xFFFFFFu), miss = (int)(word >> 24);
    const bool hist = F != 0, sample = c != 0;
    const int d = (int)(c << 8) - F;
    const bool blend = sample && hist && abs(d) <= gate;
    const bool fill = !sample && hist && miss < persist;
    const int Fb = F + (((blend ? d : 0) * alpha_q + 128) >> 8);   // (>> on a negative int is arithmetic: the mathematical floor)
    const int F2 = blend ? Fb : sample ? (int)(c << 8) : fill ? F : 0;
    const unsigned int served = (unsigned int)(F2 + 128) >> 8;      // restart: (256 c + 128) >> 8 = c; expire / empty: 0
    word = (unsigned int)F2 | (fill ? (unsigned int)(miss + 1) << 24 : 0u);
    lo += blend ? 1u : (sample && hist) ? 0x10000u : 0u;
    hi += fill ? 1u : (!sample && hist) ? 0x10000u : 0u;
    return served;
}

template <bool VEC>
__global__ __launch_bounds__(kFlyThreads) void temporal_kernel(const TemporalArgs a)
{
    __shared__ TileCount s_cnt[2][kTempAhead];
    const int tid = threadIdx.x;
    const TileLane l = tile_lane(a.frames, a.tiles[blockIdx.x]);   // (a lane outside the frame walks the loop for the wave sums and touches no memory)
    const int n = a.n_ticks;

    // the lane's chunk of tick t
    auto load = [&](int t) -> uint4 {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (l.live) load8<VEC>(v, a.in + (long long)t * a.tick_stride + l.pix, l.x, l.w);
        return v;
    };

    uint4 ahead[kTempAhead];
#pragma unroll
    for (int k = 0; k < kTempAhead; k++) ahead[k] = k < n ? load(k) : make_uint4(0, 0, 0, 0);

    unsigned int st[8];
#pragma unroll
    for (int j = 0; j < 8; j++) st[j] = 0;
    if (l.live) load8<VEC>(a.state + l.pix, l.x, l.w, st);

    int par = 0;
    for (int base = 0; base < n; base += kTempAhead, par ^= 1) {
#pragma unroll
        for (int k = 0; k < kTempAhead; k++) {
            const int t = base + k;
            if (t >= n) break;                                 // uniform
            const uint4 cur = ahead[k];
            if (t + kTempAhead < n) ahead[k] = load(t + kTempAhead);
            unsigned int c[8], o[8], lo = 0, hi = 0;
            unpack8(cur, c);
#pragma unroll
            for (int j = 0; j < 8; j++) o[j] = temporal_pixel(c[j], st[j], a.alpha_q, a.gate, a.persist, lo, hi);
            if (l.live) store8<VEC>(a.out + (long long)t * a.tick_stride + l.pix, l.x, l.w, o);
            tile_count_put(s_cnt[par][k], lo, hi);
        }
        // these ticks' four words per tile: one barrier per kTempAhead ticks (the other half of s_cnt is the next round's)
        __syncthreads();
        if (tid < kTempAhead * 4) {
            const int k = tid >> 2, f = tid & 3, t = base + k;
            if (t < n) a.counts[((long long)t * a.tiles_per_tick + blockIdx.x) * 4 + f] = tile_count_get(s_cnt[par][k], f);
        }
    }

    if (l.live) store8<VEC>(a.state + l.pix, l.x, l.w, st);
}

}  // namespace

// The setting as the definition admits it; `who` names the export in the message.  alpha_q <= 0 (off) is always admitted.
int lsn::temporal_setting_ok(const char *who, int alpha_q, int delta, int persist)
{
    if (alpha_q <= 0) return 0;
    if (alpha_q > 256 || delta < 1 || delta > 4095 || persist < 0 || persist > 255) {
        lsn::set_error("%s: (alpha_q %d, delta %d, persist %d) is outside alpha_q 1..256 (<= 0: off), delta 1..4095, persist 0..255", who, alpha_q,
                       delta, persist);
        return -1;
    }
    return 0;
}

// A state of `pixels` words as lsnFusionTemporalStateWrite admits it: F in {0} u [256, 65535 * 256], no miss without history.
int lsn::temporal_state_ok(const char *who, const unsigned int *h_state, size_t pixels)
{
    for (size_t i = 0; i < pixels; i++) {
        const unsigned int F = h_state[i] & 0xFFFFFFu, miss = h_state[i] >> 24;
        if (F == 0 ? miss != 0 : (F < 256u || F > 65535u * 256u)) {
            lsn::set_error("%s: word %zu = 0x%08x is no state (F outside {0} and 256 .. 65535 * 256, or a miss count without history)", who, i, h_state[i]);
            return -1;
        }
    }
    return 0;
}

// The filter for the library's own flows (takes the plan's mutex): `n_ticks` ticks in the plan's frame layout from d_depth_in into
// d_depth_out (the same pointer: in place; any other overlap is refused), the history in d_state advanced by them, the branch counts of the
// call in `counts` (reserved here: four words per tile and tick).  A setting that is off copies and leaves state and counts alone.
int lsn::temporal(LsnFusion *p, const TemporalSetting &ts, const void *d_depth_in, void *d_depth_out, unsigned int *d_state, lsn::DevBuf &counts,
                  int n_ticks, hipStream_t s)
{
    std::lock_guard<std::mutex> g(p->mu);
    const int run = stage_preamble(p, "lsnFusionTemporal", ts.on(), d_depth_in, d_depth_out, n_ticks, s);
    if (run <= 0) return run;
    if (temporal_setting_ok("lsnFusionTemporal", ts.alpha_q, ts.delta, ts.persist) || n_ticks < 1 || !d_state) {
        if (!lsn::has_error()) lsn::set_error("lsnFusionTemporal: bad arguments");
        return -1;
    }
    if (flying_prepare(p) || counts.reserve(4 * sizeof(int) * (size_t)p->fl_tiles_per_tick * (size_t)n_ticks)) return -1;
    TemporalArgs a;
    a.frames = p->frames.as<FrameDesc>();
    a.tiles = p->fl_tiles.as<TileDesc>();
    a.in = static_cast<const unsigned short *>(d_depth_in);
    a.out = static_cast<unsigned short *>(d_depth_out);
    a.state = d_state;
    a.counts = counts.as<int>();
    a.tiles_per_tick = p->fl_tiles_per_tick;
    a.n_ticks = n_ticks;
    a.alpha_q = ts.alpha_q;
    a.gate = 256 * ts.delta;
    a.persist = ts.persist;
    a.tick_stride = p->tick_depth_elems;
    const uintptr_t x = (uintptr_t)d_depth_in, y = (uintptr_t)d_depth_out;
    const bool vec = p->vec_ok && (x & 15) == 0 && (y & 15) == 0 && ((uintptr_t)d_state & 15) == 0 && (p->tick_depth_elems % 8) == 0;
    if (vec) hipLaunchKernelGGL((temporal_kernel<true>), dim3((unsigned)p->fl_tiles_per_tick), dim3(kFlyThreads), 0, s, a);
    else hipLaunchKernelGGL((temporal_kernel<false>), dim3((unsigned)p->fl_tiles_per_tick), dim3(kFlyThreads), 0, s, a);
    LSN_HIP(hipGetLastError());
    return 0;
}

extern "C" int lsnFusionSetTemporal(LsnFusion *p, int alpha_q, int delta, int persist)
{
    return lsn::guarded("lsnFusionSetTemporal", -1, [&]() {
        lsn::clear_error();
        if (!p) {
            lsn::set_error("lsnFusionSetTemporal: null argument");
            return -1;
        }
        if (lsn::temporal_setting_ok("lsnFusionSetTemporal", alpha_q, delta, persist)) return -1;   // refused: the previous setting stays
        std::lock_guard<std::mutex> g(p->mu);
        p->tp_setting = alpha_q >= 1 ? lsn::TemporalSetting{alpha_q, delta, persist} : lsn::TemporalSetting{};
        return 0;   // (the history stays as it is)
    });
}

extern "C" int lsnFusionTemporal(LsnFusion *p, const void *d_depth_in, void *d_depth_out, void *stream)
{
    return lsn::guarded("lsnFusionTemporal", -1, [&]() {
        lsn::clear_error();
        if (!p || !d_depth_in || !d_depth_out) {
            lsn::set_error("lsnFusionTemporal: null argument");
            return -1;
        }
        hipStream_t s = lsn::as_stream(stream);
        lsn::TemporalSetting ts;
        {
            std::lock_guard<std::mutex> g(p->mu);
            LSN_HIP(hipSetDevice(p->device));
            ts = p->tp_setting;
            // the first filtering call reserves the history (a plan that never filters allocates nothing); a call on another stream than the
            // last one's starts behind it
            if (ts.on() && (p->tp.reserve((size_t)p->cap, s) || p->tp.hand_over(s))) return -1;
        }
        if (lsn::temporal(p, ts, d_depth_in, d_depth_out, p->tp.state.as<unsigned int>(), p->tp.counts, p->n_ticks, s)) return -1;
        std::lock_guard<std::mutex> g(p->mu);
        p->tp_last = ts.on() ? 2 : 1;
        return 0;
    });
}

extern "C" int lsnFusionTemporalReset(LsnFusion *p, void *stream)
{
    return lsn::guarded("lsnFusionTemporalReset", -1, [&]() {
        lsn::clear_error();
        if (!p) {
            lsn::set_error("lsnFusionTemporalReset: null argument");
            return -1;
        }
        std::lock_guard<std::mutex> g(p->mu);
        LSN_HIP(hipSetDevice(p->device));
        return p->tp.reset((size_t)p->cap, lsn::as_stream(stream));
    });
}

extern "C" int lsnFusionTemporalStateRead(LsnFusion *p, unsigned int *h_state, void *stream)
{
    return lsn::guarded("lsnFusionTemporalStateRead", -1, [&]() {
        lsn::clear_error();
        if (!p || !h_state) {
            lsn::set_error("lsnFusionTemporalStateRead: null argument");
            return -1;
        }
        std::lock_guard<std::mutex> g(p->mu);
        LSN_HIP(hipSetDevice(p->device));
        return p->tp.read(h_state, (size_t)p->cap, lsn::as_stream(stream));
    });
}

extern "C" int lsnFusionTemporalStateWrite(LsnFusion *p, const unsigned int *h_state, void *stream)
{
    return lsn::guarded("lsnFusionTemporalStateWrite", -1, [&]() {
        lsn::clear_error();
        if (!p || !h_state) {
            lsn::set_error("lsnFusionTemporalStateWrite: null argument");
            return -1;
        }
        if (lsn::temporal_state_ok("lsnFusionTemporalStateWrite", h_state, (size_t)p->cap)) return -1;   // refused: the history stays
        std::lock_guard<std::mutex> g(p->mu);
        LSN_HIP(hipSetDevice(p->device));
        return p->tp.write(h_state, (size_t)p->cap, lsn::as_stream(stream));
    });
}

extern "C" int lsnFusionTemporalDiagnostics(LsnFusion *p, int tick, int *blended, int *restarted, int *filled, int *expired, void *stream)
{
    return lsn::guarded("lsnFusionTemporalDiagnostics", -1, [&]() {
        lsn::clear_error();
        if (!p || tick < 0 || tick >= p->n_ticks) {
            lsn::set_error("lsnFusionTemporalDiagnostics: bad arguments");
            return -1;
        }
        std::lock_guard<std::mutex> g(p->mu);
        if (p->tp_last == 0) {
            lsn::set_error("lsnFusionTemporalDiagnostics: the plan has not run the filter");
            return -1;
        }
        int *const dst[4] = {blended, restarted, filled, expired};
        return stage_diagnostics(p, p->tp_last == 2, p->tp, tick, 4, dst, lsn::as_stream(stream));
    });
}
