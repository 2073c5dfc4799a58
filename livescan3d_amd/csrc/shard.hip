// shard.hip -- part of exchange.hip's translation unit (included at its end); host code only, no kernel.
// LsnShard: the whole multi-GPU step behind the C-ABI -- one process per GPU, this rank's block of sensors in, the merged
// cloud of ALL sensors out, RCCL over xGMI in between (include/NativeUtils.h part 2b).
//
// The reference fans createVertices out over one std::thread per sensor and concatenates the per-sensor clouds in sensor
// order (src/NativeUtils/depthprocessing.cpp:708-733, formMesh :1594-1608).  Across GPUs: rank r owns the contiguous block
// [r * S / G, (r + 1) * S / G) of every tick's sensors (rank order = formMesh's sensor order) and ONE exchange step forms the
// merged cloud on every rank.  What crosses the links is what the vertices are made of (5 bytes per survivor + 1 bit per
// pixel instead of 16 bytes per vertex); every rank rebuilds all vertices with the arithmetic of the write kernel.
//
// The collectives of one step are the contract between the ranks: a rank that issues another sequence does not fail, its peers hang.
// Every line is one ncclAllGather: send -> receive, elements per rank and type, stream (s = the caller's, comm = the handle's second
// stream).  T ticks, W ranks, mpr sensors per rank, cap pixels per tick of a rank's block, tiles = the local plan's tiles per tick.
//   every mode, after pack (count, scan, tick bases, compact streams -- all ticks of the rank back to back, so the send buffer is one
//   contiguous run and nothing is staged) or, in vertex mode, after the fused pass over the rank's block:
//     1. offsets -> g_off, T * (mpr + 1) int32, s, outside any group.  Unless padded the host then reads g_off through pinned memory
//        (one event wait: the element count of a collective is a host argument, and all ranks must pass the same one, so the largest
//        count has to be known on the host).
//   survivors, one shot (chunks = 1, or padded) -- ONE group on s, then reconstruct on s:
//     2. local tile prefixes -> g_tp, T * tiles int32
//     3. mask -> g_mask, T * cap / 8 uint8
//     4. depth_c -> g_dc, 2 * slab uint8        slab = the largest rank total of the step rounded up to 8 entries; T * cap when padded
//     5. rgb_c -> g_cc, 3 * slab uint8
//   survivors, C chunks of ceil(T / C) ticks -- a group on s with 2. and 3. as above; ev_pre recorded on s, comm waits for it; then for
//   every chunk c a group on comm, ev_chunk[c] recorded on comm, s waits for it and reconstructs the chunk's ticks:
//     4c. depth_c + mine -> g_dc + recv, 2 * slab_c uint8      slab_c = the largest rank total over the chunk's ticks rounded up to 8;
//     5c. rgb_c + 3 * mine -> g_cc + 3 * recv, 3 * slab_c uint8   mine = this rank's survivors before the chunk, recv = W * the earlier slab_c
//   vertex mode -- ONE group on s, then the packing pass (lsn::merge_shards, tick-major) on s:
//     2k. for every tick k: v_local + k * cap -> v_gathered + k * W * slab (vertices), 16 * slab uint8      slab = the largest
//         (rank, tick) count of the step; cap when padded
// $LSN_SHARD_PADDED=1 skips the host read and always gathers full-capacity streams (no synchronisation at all, about twice the bytes on
// the links).  RCCL is loaded with dlopen on first use: a single-GPU host of this library never maps it.
#include <dlfcn.h>

// RCCL is only ever dlopen()ed, so the library builds without the rccl development headers: the handful of types and constants the
// seven entry points need are declared here (the nccl.h ABI: opaque communicator, 128-byte id, ncclSuccess = 0, ncclUint8 = 1,
// ncclInt32 = 2).
extern "C" {
typedef struct ncclComm *ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclInt8 = 0, ncclUint8 = 1, ncclInt32 = 2 } ncclDataType_t;
}

namespace {

struct Rccl {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;      // optional: what the communicator itself reports (lsnShardRanksSeen)
    ncclResult_t (*CommUserRank)(const ncclComm_t, int *) = nullptr;
    std::string path;   // the file the entry points came from
};

// ncclGroupStart ... ncclGroupEnd with the end guaranteed: a collective that fails inside a group must not leave the thread's group
// open (every later collective would be queued and never launched -- the next step would hang instead of reporting an error).
struct NcclGroup {
    Rccl *r;
    bool open = false;
    explicit NcclGroup(Rccl *r_) : r(r_) {}
    ncclResult_t start() { const ncclResult_t rc = r->GroupStart(); open = rc == ncclSuccess; return rc; }
    ncclResult_t end() { open = false; return r->GroupEnd(); }
    ~NcclGroup() { if (open) (void)r->GroupEnd(); }
};

Rccl *rccl()
{
    static std::mutex mu;
    static Rccl *r = nullptr;
    std::lock_guard<std::mutex> g(mu);
    if (r) return r;
    void *lib = nullptr;
    // $LSN_RCCL_LIBRARY: an RCCL build outside the loader path -- or the shared-memory test double of tests/fake_rccl, which
    // lets several ranks share one GPU (RCCL itself refuses that)
    const char *custom = getenv("LSN_RCCL_LIBRARY");
    if (custom && *custom) {
        lib = dlopen(custom, RTLD_NOW | RTLD_LOCAL);
    } else {
        // An RCCL that is already mapped in this process comes first (PyTorch-ROCm maps its own bundled librccl.so when
        // torch.distributed initialises the "nccl" backend): one process never holds two RCCL instances.  Only a host without one
        // (LiveScanServer, C/C++ callers) loads the system's.
        for (const char *name : {"librccl.so", "librccl.so.1"}) {
            lib = dlopen(name, RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
            if (lib) break;
        }
        if (!lib) {
            for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
                lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
                if (lib) break;
            }
        }
    }
    if (!lib) {
        lsn::set_error("lsnShard: cannot load %s (%s)", custom && *custom ? custom : "librccl.so.1", dlerror());
        return nullptr;
    }
    Rccl *t = new Rccl();
    t->lib = lib;
    auto load = [lib](const char *name, auto &fn) {
        fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(lib, name));
        return fn != nullptr;
    };
    const bool all = load("ncclGetUniqueId", t->GetUniqueId) && load("ncclCommInitRank", t->CommInitRank) && load("ncclCommDestroy", t->CommDestroy) &&
                     load("ncclAllGather", t->AllGather) && load("ncclGroupStart", t->GroupStart) && load("ncclGroupEnd", t->GroupEnd) &&
                     load("ncclGetErrorString", t->GetErrorString);
    (void)load("ncclCommCount", t->CommCount);         // the two optional ones
    (void)load("ncclCommUserRank", t->CommUserRank);
    if (!all) {
        lsn::set_error("lsnShard: librccl.so.1 lacks an expected entry point");
        delete t;
        return nullptr;
    }
    Dl_info info;
    if (dladdr((void *)t->AllGather, &info) && info.dli_fname) t->path = info.dli_fname;
    r = t;
    return r;
}

#define LSN_NCCL(expr)                                                                                     \
    do {                                                                                                   \
        ncclResult_t _r = (expr);                                                                          \
        if (_r != ncclSuccess) {                                                                           \
            lsn::set_error("%s failed: %s (%s:%d)", #expr, rccl()->GetErrorString(_r), __FILE__, __LINE__); \
            return -1;                                                                                     \
        }                                                                                                  \
    } while (0)

// $LSN_SHARD_*: an integer, `unset` when the variable is not there
int env_int(const char *name, int unset)
{
    const char *e = getenv(name);
    return e ? atoi(e) : unset;
}

}  // namespace

struct LsnShard {
    int device = 0, rank = 0, world = 1;
    int n_ticks = 0, n_maps = 0, mpr = 0;     // all sensors / sensors per rank
    LsnFusion *local = nullptr, *whole = nullptr;
    ncclComm_t comm = nullptr;
    bool padded = false;                       // $LSN_SHARD_PADDED=1
    // Rigs the survivor exchange cannot serve (sensors of different sizes, widths that are not multiples of 8) exchange the
    // 16-byte vertices instead: lsnFusionRun on the rank's block, one all-gather per tick (all ticks in one ncclGroup) of slabs
    // cut to the largest shard of the step, then the packing pass of lsnMergeShards.  Same merged cloud, ~3x the bytes.
    bool vertex_mode = false;
    lsn::DevBuf v_local, v_gathered;           // [n_ticks][cap_loc] vertices of this rank / [n_ticks][world][slab]
    long long cap_loc = 0;                     // vertices per tick of one rank's block
    int tiles_loc = 0;
    lsn::DevBuf mask, depth_c, rgb_c, offsets, tick_base;        // this rank's packed survivors
    lsn::DevBuf g_off, g_tp, g_mask, g_dc, g_cc, g_tick_base;    // gathered, [world][...]
    lsn::DevBuf merged, merged_off;
    int *h_goff = nullptr;                     // pinned copy of the gathered offset tables
    hipEvent_t ev_off = nullptr;
    // the streams travel in `chunks` groups of ticks on a second stream while the reconstruction of the previous group runs
    int chunks = 1;                            // $LSN_SHARD_CHUNKS (1 = one shot on the caller's stream, the default)
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_pre = nullptr;
    std::vector<hipEvent_t> ev_chunk;
    long long last_slab = 0, last_bytes_per_rank = 0;
    bool failed = false;                       // a step returned an error: every later step refuses
    std::string failure;
    std::mutex mu;
};

extern "C" int lsnShardUniqueId(unsigned char *id128)
{
    return lsn::guarded("lsnShardUniqueId", -1, [&]() {
        lsn::clear_error();
        if (!id128) return -1;
        Rccl *r = rccl();
        if (!r) return -1;
        static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
        ncclUniqueId id;
        LSN_NCCL(r->GetUniqueId(&id));
        memcpy(id128, &id, 128);
        return 0;
    });
}

extern "C" void lsnShardDestroy(LsnShard *sh)
{
    lsn::guarded_void("lsnShardDestroy", [&]() {
        if (!sh) return;
        (void)hipSetDevice(sh->device);
        if (sh->comm && rccl()) (void)rccl()->CommDestroy(sh->comm);
        if (sh->local) lsnFusionDestroy(sh->local);
        if (sh->whole) lsnFusionDestroy(sh->whole);
        if (sh->h_goff) (void)hipHostFree(sh->h_goff);
        if (sh->ev_off) (void)hipEventDestroy(sh->ev_off);
        if (sh->ev_pre) (void)hipEventDestroy(sh->ev_pre);
        for (hipEvent_t e : sh->ev_chunk) (void)hipEventDestroy(e);
        if (sh->comm_stream) (void)hipStreamDestroy(sh->comm_stream);
        delete sh;
    });
}

extern "C" LsnShard * lsnShardPrepare(int device, int rank, int world, int n_ticks, int n_maps, const int *widths, const int *heights)
{
    return lsn::guarded("lsnShardPrepare", static_cast<LsnShard *>(nullptr), [&]() -> LsnShard * {
        lsn::clear_error();
        if (world <= 0 || rank < 0 || rank >= world || n_ticks <= 0 || n_maps <= 0 || !widths || !heights || n_maps % world != 0) {
            lsn::set_error("lsnShardPrepare: bad arguments (rank %d of %d, %d sensors must split evenly)", rank, world, n_maps);
            return nullptr;
        }
        bool uniform = true;
        for (int i = 0; i < n_maps; i++) uniform = uniform && widths[i] == widths[0] && heights[i] == heights[0] && widths[i] % 8 == 0;
        const int per_rank = n_maps / world;
        // the vertex exchange needs equally shaped shards as well (an all-gather moves equal blocks): every rank's block must have
        // the same pixel capacity
        long long cap0 = 0;
        for (int q = 0; q < world; q++) {
            long long capq = 0;
            for (int i = 0; i < per_rank; i++) capq += (long long)widths[q * per_rank + i] * heights[q * per_rank + i];
            if (q == 0) cap0 = capq;
            if (capq != cap0) {
                lsn::set_error("lsnShardPrepare: the ranks' sensor blocks must hold the same number of pixels (%lld vs %lld)", cap0, capq);
                return nullptr;
            }
        }
        Rccl *r = rccl();
        if (!r) return nullptr;
        LSN_HIP_NULL(hipSetDevice(device));
        LsnShard *sh = new (std::nothrow) LsnShard();
        if (!sh) return nullptr;
        sh->device = device;
        sh->rank = rank;
        sh->world = world;
        sh->n_ticks = n_ticks;
        sh->n_maps = n_maps;
        sh->mpr = n_maps / world;
        sh->vertex_mode = !uniform || env_int("LSN_SHARD_VERTICES", 0) != 0;
        sh->padded = env_int("LSN_SHARD_PADDED", 0) != 0;
        // One shot on the caller's stream unless $LSN_SHARD_CHUNKS asks for the pipelined form (collectives on a second stream beside the
        // reconstruction): that form has only ever run with the shared-memory test double and with one real rank -- it stays opt-in until
        // a run on a multi-GPU node has verified it.
        sh->chunks = std::max(1, std::min({env_int("LSN_SHARD_CHUNKS", 1), 16, n_ticks}));
        sh->local = lsnFusionCreate(device, n_ticks, sh->mpr, widths + rank * sh->mpr, heights + rank * sh->mpr);
        sh->whole = lsnFusionCreate(device, n_ticks, n_maps, widths, heights);
        bool bad = !sh->local || !sh->whole;
        if (!bad) {
            sh->cap_loc = sh->local->cap;
            sh->tiles_loc = sh->local->tiles_per_tick;
            const size_t T = (size_t)n_ticks, W = (size_t)world, cap = (size_t)sh->cap_loc;
            if (sh->vertex_mode) {
                bad |= sh->v_local.reserve(T * cap * 16) != 0;
                bad |= sh->v_gathered.reserve(W * T * cap * 16) != 0;
            }
            bad |= sh->mask.reserve(T * cap / 8) != 0;
            // a chunk's send starts at the rank's own tick start and is as long as the LONGEST rank's chunk: room to read past the end
            const size_t chunk_cap = ((T + sh->chunks - 1) / sh->chunks) * cap + 64;
            bad |= sh->depth_c.reserve((T * cap + chunk_cap) * 2 + 64) != 0;
            bad |= sh->rgb_c.reserve((T * cap + chunk_cap) * 3 + 64) != 0;
            bad |= sh->offsets.reserve(sizeof(int) * T * (sh->mpr + 1)) != 0;
            bad |= sh->tick_base.reserve(sizeof(int) * T) != 0;
            bad |= sh->g_off.reserve(sizeof(int) * W * T * (sh->mpr + 1)) != 0;
            bad |= sh->g_tp.reserve(sizeof(int) * W * T * sh->tiles_loc) != 0;
            bad |= sh->g_mask.reserve(W * T * cap / 8) != 0;
            bad |= sh->g_dc.reserve(W * (T * cap + 8 * 16 + 64) * 2) != 0;
            bad |= sh->g_cc.reserve(W * (T * cap + 8 * 16 + 64) * 3) != 0;
            bad |= sh->g_tick_base.reserve(sizeof(int) * W * T) != 0;
            bad |= sh->merged.reserve((size_t)sh->whole->cap * 16 * T) != 0;
            bad |= sh->merged_off.reserve(sizeof(int) * T * (n_maps + 1)) != 0;
            bad |= hipHostMalloc((void **)&sh->h_goff, sizeof(int) * W * T * (sh->mpr + 1), hipHostMallocDefault) != hipSuccess;
            bad |= hipEventCreateWithFlags(&sh->ev_off, hipEventDisableTiming) != hipSuccess;
            bad |= hipEventCreateWithFlags(&sh->ev_pre, hipEventDisableTiming) != hipSuccess;
            bad |= hipStreamCreateWithFlags(&sh->comm_stream, hipStreamNonBlocking) != hipSuccess;
            for (int c = 0; c < sh->chunks && !bad; c++) {
                hipEvent_t e = nullptr;
                bad |= hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess;
                if (e) sh->ev_chunk.push_back(e);
            }
        }
        if (bad) {
            if (!lsn::has_error()) lsn::set_error("lsnShardPrepare: allocation failed: %s", hipGetErrorString(hipGetLastError()));
            lsnShardDestroy(sh);
            return nullptr;
        }
        return sh;
    });
}

extern "C" int lsnShardConnect(LsnShard *sh, const unsigned char *id128)
{
    return lsn::guarded("lsnShardConnect", -1, [&]() {
        lsn::clear_error();
        if (!sh || !id128) {
            lsn::set_error("lsnShardConnect: null argument");
            return -1;
        }
        Rccl *r = rccl();
        if (!r) return -1;
        std::lock_guard<std::mutex> g(sh->mu);
        if (sh->comm) {
            lsn::set_error("lsnShardConnect: already connected");
            return -1;
        }
        LSN_HIP(hipSetDevice(sh->device));
        ncclUniqueId id;
        memcpy(&id, id128, 128);
        const ncclResult_t rc = r->CommInitRank(&sh->comm, sh->world, id, sh->rank);   // blocks until every rank of the world has called it
        if (rc != ncclSuccess) {
            lsn::set_error("lsnShardConnect: ncclCommInitRank failed: %s", r->GetErrorString(rc));
            sh->comm = nullptr;
            return -1;
        }
        return 0;
    });
}

extern "C" LsnShard * lsnShardCreate(int device, int rank, int world, const unsigned char *id128, int n_ticks, int n_maps, const int *widths,
                                    const int *heights)
{
    return lsn::guarded("lsnShardCreate", static_cast<LsnShard *>(nullptr), [&]() -> LsnShard * {
        if (!id128) {
            lsn::clear_error();
            lsn::set_error("lsnShardCreate: null id");
            return nullptr;
        }
        LsnShard *sh = lsnShardPrepare(device, rank, world, n_ticks, n_maps, widths, heights);
        if (!sh) return nullptr;
        if (lsnShardConnect(sh, id128)) {
            const std::string why = lsn::error_buffer();
            lsnShardDestroy(sh);
            lsn::set_error("%s", why.c_str());
            return nullptr;
        }
        return sh;
    });
}

extern "C" int lsnShardRcclPath(char *buf, int len)
{
    return lsn::guarded("lsnShardRcclPath", -1, [&]() {
        Rccl *r = rccl();
        if (!r) return -1;
        if (buf && len > 0) snprintf(buf, (size_t)len, "%s", r->path.c_str());
        return (int)r->path.size();
    });
}

// What the connected communicator itself reports: its rank count, or -1 (not connected / the RCCL in use lacks ncclCommCount / the
// communicator's own rank differs from the handle's).  bench.py puts it into the N > 1 line as n_ranks_seen.
extern "C" int lsnShardRanksSeen(LsnShard *sh)
{
    return lsn::guarded("lsnShardRanksSeen", -1, [&]() {
        lsn::clear_error();
        Rccl *r = rccl();
        if (!sh || !r) return -1;
        std::lock_guard<std::mutex> g(sh->mu);
        if (!sh->comm || !r->CommCount) {
            lsn::set_error("lsnShardRanksSeen: %s", !sh->comm ? "the handle is not connected" : "this RCCL has no ncclCommCount");
            return -1;
        }
        int n = -1, me = sh->rank;
        LSN_NCCL(r->CommCount(sh->comm, &n));
        if (r->CommUserRank) LSN_NCCL(r->CommUserRank(sh->comm, &me));
        if (me != sh->rank) {
            lsn::set_error("lsnShardRanksSeen: the communicator says rank %d, the handle %d", me, sh->rank);
            return -1;
        }
        return n;
    });
}

extern "C" LsnFusion *lsnShardPlan(LsnShard *sh, int whole) { return sh ? (whole ? sh->whole : sh->local) : nullptr; }
extern "C" long long lsnShardMergedCapacity(const LsnShard *sh) { return sh && sh->whole ? sh->whole->cap : 0; }
extern "C" long long lsnShardLastBytesSent(const LsnShard *sh) { return sh ? sh->last_bytes_per_rank : 0; }

extern "C" int lsnShardSetParams(LsnShard *sh, const float *intr_all, const float *wt_all, const float *bounds6, void *stream)
{
    return lsn::guarded("lsnShardSetParams", -1, [&]() {
        lsn::clear_error();
        if (!sh || !intr_all || !wt_all || !bounds6) {
            lsn::set_error("lsnShardSetParams: null argument");
            return -1;
        }
        if (lsnFusionSetParams(sh->whole, intr_all, wt_all, bounds6, stream)) return -1;
        return lsnFusionSetParams(sh->local, intr_all + 7 * (size_t)sh->rank * sh->mpr, wt_all + 12 * (size_t)sh->rank * sh->mpr, bounds6, stream);
    });
}

static int shard_step(LsnShard *sh, const void *d_depth_local, const void *d_colors_local, void **d_merged, int **d_merged_offsets, void *stream);

extern "C" int lsnShardStep(LsnShard *sh, const void *d_depth_local, const void *d_colors_local, void **d_merged, int **d_merged_offsets,
                            void *stream)
{
    return lsn::guarded("lsnShardStep", -1, [&]() {
        lsn::clear_error();
        if (!sh || !d_depth_local || !d_colors_local) {
            lsn::set_error("lsnShardStep: null argument");
            return -1;
        }
        std::lock_guard<std::mutex> g(sh->mu);
        if (!sh->comm) {
            lsn::set_error("lsnShardStep: the handle is not connected (lsnShardConnect)");
            return -1;
        }
        if (sh->failed) {
            // a collective of an earlier step failed: the ranks' communicators are no longer in step, nothing further may be queued on them
            lsn::set_error("lsnShardStep: an earlier step failed (%s); destroy the handle", sh->failure.c_str());
            return -1;
        }
        const int rc = shard_step(sh, d_depth_local, d_colors_local, d_merged, d_merged_offsets, stream);
        if (rc) {
            sh->failed = true;
            sh->failure = lsn::error_buffer();
        }
        return rc;
    });
}

namespace {

// The largest count a rank reports over ticks [t0, t1) of the pinned offset tables (at least 1: no collective of no elements); *mine is
// this rank's own.
long long largest_rank_total(const LsnShard *sh, int t0, int t1, long long *mine = nullptr)
{
    long long most = 1;
    for (int q = 0; q < sh->world; q++) {
        long long tot = 0;
        for (int k = t0; k < t1; k++) tot += tick_total(sh->h_goff, sh->n_ticks, sh->mpr, q, k);
        most = std::max(most, tot);
        if (mine && q == sh->rank) *mine = tot;
    }
    return most;
}

// Collective 1 of every mode, and what the host learns from it.  *slab comes in as a rank's capacity and leaves as the largest count
// the ranks report: per rank over all ticks (survivors: one run per rank travels) or per (rank, tick) (vertices: one slab per tick).
// Padded: the all-gather only, *slab stays the capacity.
int gather_offsets(LsnShard *sh, Rccl *r, hipStream_t s, bool per_rank_total, long long *slab)
{
    const size_t off_ints = (size_t)sh->n_ticks * (sh->mpr + 1);
    LSN_NCCL(r->AllGather(sh->offsets.p, sh->g_off.p, off_ints, ncclInt32, sh->comm, s));
    if (sh->padded) return 0;
    LSN_HIP(hipMemcpyAsync(sh->h_goff, sh->g_off.p, sizeof(int) * (size_t)sh->world * off_ints, hipMemcpyDeviceToHost, s));
    LSN_HIP(hipEventRecord(sh->ev_off, s));
    LSN_HIP(hipEventSynchronize(sh->ev_off));
    long long most = per_rank_total ? largest_rank_total(sh, 0, sh->n_ticks) : 1;
    for (int k = 0; k < sh->n_ticks && !per_rank_total; k++) most = std::max(most, largest_rank_total(sh, k, k + 1));
    if (most > *slab) {
        lsn::set_error(per_rank_total ? "lsnShardStep: a rank reports %lld survivors, more than its %lld pixels"
                                      : "lsnShardStep: a shard reports %lld vertices, more than its %lld pixels", most, *slab);
        return -1;
    }
    *slab = most;
    return 0;
}

// What this rank put into the step's all-gathers (lsnShardLastBytesSent): the offset tables, in the survivor exchange the tile prefixes
// and the masks, and `slab_entries` entries of `bytes_per_entry` bytes.
void account(LsnShard *sh, long long slab_entries, size_t bytes_per_entry)
{
    const size_t T = (size_t)sh->n_ticks;
    size_t bytes = sizeof(int) * T * (sh->mpr + 1);
    if (!sh->vertex_mode) bytes += sizeof(int) * T * sh->tiles_loc + T * (size_t)sh->cap_loc / 8;
    sh->last_slab = slab_entries;
    sh->last_bytes_per_rank = (long long)(bytes + (size_t)slab_entries * bytes_per_entry);
}

int vertex_step(LsnShard *sh, Rccl *r, const void *d_depth_local, const void *d_colors_local, void *stream)
{
    hipStream_t s = lsn::as_stream(stream);
    const size_t T = (size_t)sh->n_ticks, W = (size_t)sh->world, cap = (size_t)sh->cap_loc;
    if (lsn::run_vertices(sh->local, d_depth_local, d_colors_local, sh->v_local.p, sh->offsets.as<int>(), s)) return -1;
    long long slab = (long long)cap;
    if (gather_offsets(sh, r, s, false, &slab)) return -1;
    NcclGroup grp(r);
    LSN_NCCL(grp.start());
    for (size_t k = 0; k < T; k++)
        LSN_NCCL(r->AllGather(sh->v_local.as<uint4>() + k * cap, sh->v_gathered.as<uint4>() + k * W * (size_t)slab, (size_t)slab * 16, ncclUint8,
                              sh->comm, s));
    LSN_NCCL(grp.end());
    account(sh, slab, T * 16);   // (a slab entry is one vertex in each of the T ticks)
    return lsn::merge_shards(sh->device, sh->world, sh->n_ticks, sh->mpr, sh->v_gathered.p, slab, sh->g_off.as<int>(), sh->merged.p, sh->whole->cap,
                             sh->merged_off.as<int>(), true, stream);
}

// One shot (C = 1): collectives 2 to 5 in ONE group on the caller's stream, no event.  Pipelined (C > 1): the tile prefixes and the
// masks travel first (every chunk needs them); then the streams of tick group c cross the links on the communication stream while the
// caller's stream reconstructs group c - 1.  Every rank cuts the ticks the same way and derives the same chunk lengths from the same
// gathered offset tables.
int survivor_step(LsnShard *sh, Rccl *r, const void *d_depth_local, const void *d_colors_local, void *stream)
{
    hipStream_t s = lsn::as_stream(stream);
    const size_t T = (size_t)sh->n_ticks, W = (size_t)sh->world, cap = (size_t)sh->cap_loc;
    if (lsn::pack_survivors(sh->local, d_depth_local, d_colors_local, sh->mask.p, sh->depth_c.p, sh->rgb_c.p, nullptr, sh->offsets.as<int>(),
                            sh->tick_base.as<int>(), stream))
        return -1;
    long long slab = (long long)(T * cap);   // entries of one rank's streams that travel
    if (gather_offsets(sh, r, s, true, &slab)) return -1;
    const int C = sh->padded ? 1 : sh->chunks, per = (int)((T + C - 1) / C);
    const bool piped = C > 1;
    NcclGroup grp(r);
    LSN_NCCL(grp.start());
    LSN_NCCL(r->AllGather(sh->local->tile_counts.p, sh->g_tp.p, T * sh->tiles_loc, ncclInt32, sh->comm, s));
    LSN_NCCL(r->AllGather(sh->mask.p, sh->g_mask.p, T * cap / 8, ncclUint8, sh->comm, s));
    if (piped) {
        LSN_NCCL(grp.end());
        LSN_HIP(hipEventRecord(sh->ev_pre, s));                    // pack and the small gathers are done: the streams may be read
        LSN_HIP(hipStreamWaitEvent(sh->comm_stream, sh->ev_pre, 0));
    }
    long long my_start = 0, recv_off = 0, sent = 0;
    for (int c = 0; c < C; c++) {
        const int t0 = c * per, t1 = (int)std::min<size_t>(T, (size_t)(c + 1) * per);
        if (t0 >= t1) break;
        long long mine = 0;   // (the colour stream of every rank starts 8-byte aligned behind a count rounded up to 8)
        const long long slab_c = sh->padded ? slab : (largest_rank_total(sh, t0, t1, &mine) + 7) & ~7ll;
        unsigned short *dc = sh->g_dc.as<unsigned short>() + recv_off;
        unsigned char *cc = sh->g_cc.as<unsigned char>() + 3 * recv_off;
        if (piped) LSN_NCCL(grp.start());
        LSN_NCCL(r->AllGather(sh->depth_c.as<unsigned short>() + my_start, dc, (size_t)slab_c * 2, ncclUint8, sh->comm, piped ? sh->comm_stream : s));
        LSN_NCCL(r->AllGather(sh->rgb_c.as<unsigned char>() + 3 * my_start, cc, (size_t)slab_c * 3, ncclUint8, sh->comm, piped ? sh->comm_stream : s));
        LSN_NCCL(grp.end());
        if (piped) {
            LSN_HIP(hipEventRecord(sh->ev_chunk[c], sh->comm_stream));
            LSN_HIP(hipStreamWaitEvent(s, sh->ev_chunk[c], 0));
        }
        if (lsn::reconstruct(sh->whole, sh->world, sh->mpr, sh->g_mask.p, dc, cc, slab_c, sh->g_tp.as<int>(), sh->g_off.as<int>(), sh->merged.p,
                             sh->merged_off.as<int>(), sh->g_tick_base.as<int>(), stream, lsn::ReconChunk{t0, t1 - t0, c == 0}))
            return -1;
        my_start += mine;
        recv_off += (long long)W * slab_c;
        sent += slab_c;
    }
    account(sh, sent, 5);
    return 0;
}

}  // namespace

// offsets, then the vertex path or the survivor path (the head of this file lists their collectives), then the result
static int shard_step(LsnShard *sh, const void *d_depth_local, const void *d_colors_local, void **d_merged, int **d_merged_offsets, void *stream)
{
    Rccl *r = rccl();
    if (!r) return -1;
    LSN_HIP(hipSetDevice(sh->device));
    if ((sh->vertex_mode ? vertex_step : survivor_step)(sh, r, d_depth_local, d_colors_local, stream)) return -1;
    if (d_merged) *d_merged = sh->merged.p;
    if (d_merged_offsets) *d_merged_offsets = sh->merged_off.as<int>();
    return 0;
}
