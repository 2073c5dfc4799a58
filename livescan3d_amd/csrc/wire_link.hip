// wire_link.hip -- part of wire.hip's translation unit: formMeshChunks (LiveScanServer/TransferServer.cs:203-270) without a chunk-by-chunk
// walk, the default path.  The uses of every vertex linked into chains, two device-wide prefix sums (one tile frame for both), the chunk
// ends by one wave (:239-260 with its counters in closed form), the emit pass, and the host driver.
//
// The window walk (wire_walk.hip) finds the chunks one after the other: three dependent launches per chunk, ~50 for the mesh of a tick.  For meshes
// whose vertex re-use is LOCAL -- every vertex used at most 16 times, two consecutive uses less than a chunk's worth of index positions
// apart: every grid mesh -- the chunks follow from one prefix sum:
//   * prev[pos] = the previous index position that uses the same vertex (-1: none), last[pos] = no later position does.  A position opens
//     a new vertex in the chunk that starts at triangle s iff prev[pos] < 3 s;
//   * PF[t] = vertices used for the first time up to and including triangle t, PH[t] = vertices used for the last time up to and
//     including t.  The chunk that starts at triangle s holds, through triangle e, PF[e] - PH[s - 1] vertices: those that have begun minus
//     those that had already ended -- exact unless a vertex is used before s and after e but not in between, which a link shorter than
//     64997 positions rules out from e = s + 21665 on, and a chunk cannot close earlier (a triangle opens at most three vertices).  The end
//     of a chunk is therefore a search in PF; the chunks of a mesh are ~13 such searches by one wave;
//   * the new index of a position = its rank among the chunk's opening positions (one more prefix sum), or the rank of the opening
//     position its prev-chain leads to.
// A vertex with more than 16 uses or a longer link sends the call down the window walk instead (same bytes).

namespace {
constexpr int kMaxUses = 16;
constexpr int kScanPerBlock = 2048;   // elements per workgroup of the prefix sums (8 per thread)
constexpr unsigned kLastUse = 0x80000000u;   // prev[] holds (previous position + 1) | kLastUse

struct LinkState { int n_chunks, n_send, bad, fallback; };

// the path was abandoned (a bad index: prev[] is incomplete; a fallback: the closed form does not hold): nothing may follow prev[] or the chunks
__device__ __forceinline__ bool link_abandoned(const LinkState *st) { return (st->bad | st->fallback) != 0; }

__device__ __forceinline__ int link_prev_of(unsigned code) { return (int)(code & ~kLastUse) - 1; }

// uses[v][k] = the index positions that use vertex v, in no particular order.  A workgroup takes 12288 consecutive positions (4096
// triangles, a few rows of a grid mesh), counts the vertices within 8192 ids of its smallest one in LDS and reserves each vertex's slots in
// the global row with ONE atomic per vertex it touches; ids outside the window take one atomic per position.  (Device-scope atomics execute
// at the memory side: one returning atomic per position costs 56 us for a tick's mesh, this 23 us, of which the scattered stores are most.)
constexpr int kUsesThreads = 1024, kUsesPer = 12, kUsesWindow = 8192;

__global__ __launch_bounds__(kUsesThreads) void link_uses_kernel(const int *__restrict__ tri, int n_pos, int nV, int *cnt, int *uses, LinkState *st)
{
    __shared__ int s_cnt[kUsesWindow];
    __shared__ int s_base[kUsesWindow];
    __shared__ int s_min[kUsesThreads / 64];
    const int tid = threadIdx.x;
    const long long block0 = (long long)blockIdx.x * (kUsesThreads * kUsesPer);
    int val[kUsesPer], kl[kUsesPer];
    int vmin = 0x7fffffff;
    bool bad = false;
#pragma unroll
    for (int i = 0; i < kUsesPer; i++) {
        const long long pos = block0 + i * kUsesThreads + tid;
        val[i] = pos < n_pos ? tri[pos] : -1;
        if (pos < n_pos && (unsigned)val[i] >= (unsigned)nV) { bad = true; val[i] = -1; }
        if (val[i] >= 0) vmin = min(vmin, val[i]);
    }
    if (bad) atomicOr(&st->bad, 1);
    for (int i = tid; i < kUsesWindow; i += kUsesThreads) s_cnt[i] = 0;
    vmin = wave_min(vmin);
    if ((tid & 63) == 0) s_min[tid >> 6] = vmin;
    __syncthreads();
    vmin = s_min[0];
#pragma unroll
    for (int w2 = 1; w2 < kUsesThreads / 64; w2++) vmin = min(vmin, s_min[w2]);
#pragma unroll
    for (int i = 0; i < kUsesPer; i++) {
        const unsigned d = (unsigned)val[i] - (unsigned)vmin;
        kl[i] = val[i] >= 0 && d < (unsigned)kUsesWindow ? atomicAdd(&s_cnt[d], 1) : -1;
    }
    __syncthreads();
    for (int d = tid; d < kUsesWindow; d += kUsesThreads) {
        const int n = s_cnt[d];
        if (n) s_base[d] = atomicAdd(&cnt[vmin + d], n);
    }
    __syncthreads();
    bool over = false;
#pragma unroll
    for (int i = 0; i < kUsesPer; i++) {
        if (val[i] < 0) continue;
        const long long pos = block0 + i * kUsesThreads + tid;
        const int k = kl[i] >= 0 ? s_base[val[i] - vmin] + kl[i] : atomicAdd(&cnt[val[i]], 1);
        if (k < kMaxUses) uses[(size_t)val[i] * kMaxUses + k] = (int)pos;
        else over = true;
    }
    if (over) atomicOr(&st->fallback, 1);
}

// the uses of one vertex, each against all: the previous use = the largest smaller one (no sort), the last use = none larger
template <int N>
__device__ __forceinline__ void link_row(const int (&u)[16], int n, unsigned *prev, LinkState *st)
{
#pragma unroll
    for (int i = 0; i < N; i++) {
        if (i < n) {
            const int p = u[i];
            int best = -1;
            bool later = false;
#pragma unroll
            for (int j = 0; j < N; j++) {
                const int q = u[j];                               // -2 where the row has no entry
                best = (q < p && q > best) ? q : best;
                later |= q > p;
            }
            prev[p] = (unsigned)(best + 1) | (later ? 0u : kLastUse);
            if (best >= 0 && p - best >= kChunkLimit) atomicOr(&st->fallback, 1);   // a link as long as a chunk: the closed form does not hold
        }
    }
}

__global__ __launch_bounds__(256) void link_prev_kernel(const int *__restrict__ cnt, const int *__restrict__ uses, int nV, unsigned *prev, LinkState *st)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    const int n = v < nV ? min(cnt[v], kMaxUses) : 0;
    const int4 *row = reinterpret_cast<const int4 *>(uses + (size_t)min(v, nV - 1) * kMaxUses);
    int u[16];
    const bool wide = __any(n > 8);
    {
        const int4 a = row[0], b = row[1];
        u[0] = a.x; u[1] = a.y; u[2] = a.z; u[3] = a.w; u[4] = b.x; u[5] = b.y; u[6] = b.z; u[7] = b.w;
    }
    if (wide) {
        const int4 a = row[2], b = row[3];
        u[8] = a.x; u[9] = a.y; u[10] = a.z; u[11] = a.w; u[12] = b.x; u[13] = b.y; u[14] = b.z; u[15] = b.w;
    }
#pragma unroll
    for (int i = 0; i < 16; i++)
        if (i >= n) u[i] = -2;
    if (wide) link_row<16>(u, n, prev, st);
    else link_row<8>(u, n, prev, st);
}

// one thread per triangle: how many of its positions are first uses (low half) and last uses (high half)
__global__ __launch_bounds__(256) void link_pack_kernel(const unsigned *__restrict__ prev, int nT, unsigned long long *pack, const LinkState *st)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nT || link_abandoned(st)) return;
    unsigned f = 0, h = 0;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const unsigned c = prev[3 * t + j];
        f += (c & ~kLastUse) == 0;
        h += c >> 31;
    }
    pack[t] = (unsigned long long)f | ((unsigned long long)h << 32);
}

// ---- prefix sums over a few million elements: block totals, one workgroup over the totals, blocks again ----
// eight consecutive elements of a thread (the arrays are 32-byte aligned and padded to a multiple of eight)
template <typename T>
__device__ __forceinline__ void load8(const T *in, long long base, long long n, T (&v)[8])
{
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "");
    constexpr int kVec = 16 / sizeof(T);
    const uint4 *src = reinterpret_cast<const uint4 *>(in + base);
    uint4 raw[8 / kVec];
    if (base < n) {
#pragma unroll
        for (int i = 0; i < 8 / kVec; i++) raw[i] = src[i];
    }
    const T *r = reinterpret_cast<const T *>(raw);
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = base + k < n ? r[k] : T(0);
}

template <typename T>
__device__ __forceinline__ void store8(T *out, long long base, long long n, const T (&v)[8])
{
    constexpr int kVec = 16 / sizeof(T);
    if (base + 8 <= n) {
        const uint4 *r = reinterpret_cast<const uint4 *>(v);
        uint4 *dst = reinterpret_cast<uint4 *>(out + base);
#pragma unroll
        for (int i = 0; i < 8 / kVec; i++) dst[i] = r[i];
    } else {
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (base + k < n) out[base + k] = v[k];
    }
}

// The tile frame of both prefix sums: a workgroup of 256 threads takes kScanPerBlock consecutive elements, a thread eight of them from
// tile_base() on.  tile_total: the tile's sum into totals[]; tile_prefixes: v[k] -> the sum of every element of the array before it
// (INCLUSIVE: and itself), once scan_top_kernel has made totals[] exclusive prefixes.  s_wave: four entries of LDS.
__device__ __forceinline__ long long tile_base() { return (long long)blockIdx.x * kScanPerBlock + threadIdx.x * 8; }

template <typename T> __device__ __forceinline__ T sum8(const T (&v)[8]) { return v[0] + v[1] + v[2] + v[3] + v[4] + v[5] + v[6] + v[7]; }

template <typename T> __device__ __forceinline__ void tile_total(const T (&v)[8], T *s_wave, T *totals)
{
    const T incl = block_scan_incl<T, 4>(sum8(v), s_wave);
    if (threadIdx.x == 255) totals[blockIdx.x] = incl;
}

template <bool INCLUSIVE, typename T> __device__ __forceinline__ void tile_prefixes(T (&v)[8], T *s_wave, const T *totals)
{
    const T sum = sum8(v);
    T run = block_scan_incl<T, 4>(sum, s_wave) - sum + totals[blockIdx.x];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const T x = v[k];
        v[k] = INCLUSIVE ? run + x : run;
        run += x;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void scan_totals_kernel(const T *__restrict__ in, long long n, T *totals)
{
    __shared__ T s_wave[4];
    T v[8];
    load8(in, tile_base(), n, v);
    tile_total(v, s_wave, totals);
}

template <typename T>
__global__ __launch_bounds__(1024) void scan_top_kernel(T *totals, int nb)   // totals -> exclusive prefixes, in place
{
    __shared__ T s_wave[16];
    block_scan_array_excl<T, 1024>(totals, 1, totals, nb, s_wave);
}

template <typename T>
__global__ __launch_bounds__(256) void scan_apply_kernel(T *data /* in place, inclusive */, long long n, const T *__restrict__ totals)
{
    __shared__ T s_wave[4];
    T v[8];
    load8(data, tile_base(), n, v);
    tile_prefixes<true>(v, s_wave, totals);
    store8(data, tile_base(), n, v);
}

// the first index in [lo, hi] whose key reaches `need` (keys non-decreasing, key(get(hi)) >= need), by the whole wave; *found = get(index)
template <class V, class Get, class Key>
__device__ __forceinline__ int wave_first(int lo, int hi, int need, Get get, Key key, V *found)
{
    const int lane = threadIdx.x & 63;
    while (hi - lo >= 64) {
        const int step = (hi - lo + 64) / 65;                          // probes lo + step, lo + 2 step, ... clipped to hi
        const int probe = min(lo + (lane + 1) * step, hi);             // (no overflow: callers search ranges far below 2^31 / 64)
        const unsigned long long m = __ballot(key(get(probe)) >= need);
        if (m == 0) {
            lo = lo + 64 * step + 1;
        } else {
            const int first = __ffsll((long long)m) - 1;
            hi = min(lo + (first + 1) * step, hi);
            lo = first == 0 ? lo : lo + first * step + 1;
        }
    }
    const V v = get(min(lo + lane, hi));
    const unsigned long long m = __ballot(key(v) >= need);
    const int first = __ffsll((long long)m) - 1;
    *found = __shfl(v, first, 64);
    return lo + first;
}

constexpr int kLinkChunksLds = 1024;      // chunk starts a workgroup keeps in LDS
constexpr int kLinkTotalsLds = 12288;     // block totals the chunk search keeps in LDS (>= 1024 chunks' worth of triangles / 2048)

// one wave: the chunk ends, one search per chunk; every lane keeps the cursor, lane 0 stores what it says
__global__ __launch_bounds__(64) void link_chunks_kernel(const unsigned long long *__restrict__ P /* inclusive prefix of pack[], nT entries */,
                                                         const unsigned long long *__restrict__ totals /* exclusive, per 2048 triangles */, int nT,
                                                         int max_chunks, int *chunk_start /* [max_chunks + 1] */, int *chunk_vbase, int *v_chunks,
                                                         int *t_chunks, LinkState *st)
{
    __shared__ int s_tot[kLinkTotalsLds];
    const int lane = threadIdx.x;
    if (link_abandoned(st)) return;
    const int nb = div_up(nT, kScanPerBlock);
    for (int b = lane; b < nb; b += 64) s_tot[b] = (int)(unsigned)totals[b];                 // PF before block b
    __syncthreads();
    auto low = [](unsigned long long v) { return (int)(unsigned)v; };
    ChunkCursor cur{v_chunks, t_chunks};
    int s = 0;
    int ended = 0;                                                     // vertices whose last use lies before the chunk: PH[s - 1]
    const int pf_last = low(P[nT - 1]);
    while (s < nT && cur.c < max_chunks) {
        const int need = kChunkLimit + ended;                          // the chunk closes at the first e with PF[e] >= need ...
        const int lo = s + div_up(kChunkLimit, 3) - 1;                 // ... which is never before this triangle
        if (lane == 0) { chunk_start[cur.c] = s; chunk_vbase[cur.c] = cur.vbase; }
        if (lo > nT - 1 || pf_last < need) {                           // the mesh ends first (:256-260)
            cur.end_of_mesh(nT, pf_last - ended, lane == 0);
            s = nT;
            break;
        }
        // the block of 2048 triangles in which PF reaches `need`: the last one whose prefix is still short of it
        int b = nb - 1, unused;
        if (s_tot[nb - 1] >= need)                                     // s_tot[0] = 0 < need: the first block that is not short is >= 1
            b = wave_first(0, nb - 1, need, [&](int i) { return s_tot[i]; }, [](int v) { return v; }, &unused) - 1;
        unsigned long long at_e;
        int e = wave_first(b * kScanPerBlock, min(b * kScanPerBlock + kScanPerBlock - 1, nT - 1), need, [&](int t) { return P[t]; }, low, &at_e);
        if (e < lo) {                                                  // the closed form over-counts before `lo` (vertices used on both sides of a short window only); it is monotone, so then the chunk closes at `lo`
            e = lo;
            at_e = P[e];
        }
        cur.close(e, low(at_e) - ended, lane == 0);
        ended = (int)(at_e >> 32);                                     // PH[e]: what has ended before the next chunk
        s = e + 1;
    }
    if (lane == 0) {
        chunk_start[cur.c] = nT;
        if (s < nT) st->fallback = 1;                                  // more chunks than the tables hold
        st->n_chunks = cur.c;
        st->n_send = cur.vbase;
    }
}

__device__ __forceinline__ int chunk_of(const int *s_start, int n_chunks, int t)
{
    int lo = 0, hi = n_chunks - 1;                                     // last chunk with start <= t
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s_start[mid] <= t) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// which of a thread's eight positions open a vertex in their chunk (s_start[n_chunks] = nT)
__device__ __forceinline__ void opening_flags(const unsigned *prev, long long base, int n_pos, const int *s_start, int nc, int (&flag)[8])
{
    unsigned code[8];
    load8(prev, base, (long long)n_pos, code);
    int c = base < n_pos ? chunk_of(s_start, nc, (int)(base / 3)) : 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int pos = (int)base + k;
        if (pos < n_pos && pos / 3 >= s_start[c + 1]) c++;
        flag[k] = pos < n_pos && link_prev_of(code[k]) < 3 * s_start[c];
    }
}

__device__ __forceinline__ bool load_chunk_starts(int *s_start, const int *chunk_start, const LinkState *st, int &nc)
{
    if (link_abandoned(st)) return false;
    nc = st->n_chunks;
    for (int i = threadIdx.x; i <= nc && i <= kLinkChunksLds; i += 256) s_start[i] = chunk_start[i];
    __syncthreads();
    return true;
}

__global__ __launch_bounds__(256) void rank_totals_kernel(const unsigned *__restrict__ prev, int n_pos, const int *__restrict__ chunk_start,
                                                          const LinkState *st, int *totals)
{
    __shared__ int s_start[kLinkChunksLds + 1];
    __shared__ int s_wave[4];
    int nc, flag[8];
    if (!load_chunk_starts(s_start, chunk_start, st, nc)) return;
    opening_flags(prev, tile_base(), n_pos, s_start, nc, flag);
    tile_total(flag, s_wave, totals);
}

// rank[pos] = opening positions before pos (exclusive prefix over the whole mesh)
__global__ __launch_bounds__(256) void rank_apply_kernel(const unsigned *__restrict__ prev, int n_pos, const int *__restrict__ chunk_start,
                                                         const LinkState *st, const int *__restrict__ totals, int *__restrict__ rank)
{
    __shared__ int s_start[kLinkChunksLds + 1];
    __shared__ int s_wave[4];
    int nc, flag[8];
    if (!load_chunk_starts(s_start, chunk_start, st, nc)) return;
    opening_flags(prev, tile_base(), n_pos, s_start, nc, flag);
    tile_prefixes<false>(flag, s_wave, totals);
    store8(rank, tile_base(), (long long)n_pos, flag);
}

__global__ __launch_bounds__(256) void link_emit_kernel(const int *__restrict__ tri, const unsigned *__restrict__ prev, int n_pos,
                                                        const uint4 *__restrict__ verts, const int *__restrict__ chunk_start,
                                                        const int *__restrict__ chunk_vbase, const LinkState *st,
                                                        const int *__restrict__ rank, uint4 *__restrict__ new_v, int *__restrict__ new_tri)
{
    __shared__ int s_start[kLinkChunksLds + 1];
    int nc;
    if (!load_chunk_starts(s_start, chunk_start, st, nc)) return;
    const int pos = blockIdx.x * 256 + threadIdx.x;
    if (pos >= n_pos) return;
    const int c = chunk_of(s_start, nc, pos / 3);
    const int p0 = 3 * s_start[c];
    const int r0 = rank[p0];
    int q = pos;
    for (int hop = 0; hop < kMaxUses; hop++) {                              // the position that opened this vertex in the chunk
        const int before = link_prev_of(prev[q]);
        if (before < p0) break;
        q = before;
    }
    const int li = rank[q] - r0;
    new_tri[pos] = li;                                                       // verticesMap[val] / verticesInCurrentChunk (:231-241)
    if (q == pos) new_v[chunk_vbase[c] + li] = verts[tri[pos]];              // newVertices[currentVertex] = lVertices[val] (:234)
}

}  // namespace

// the link path has room for this mesh on this handle: its chunk starts and block totals fit the kernels' LDS tables
static bool link_fits(const LsnTransfer &t, int n_triangles)
{
    return chunk_bound(0, n_triangles) <= kLinkChunksLds && div_up(n_triangles, kScanPerBlock) <= kLinkTotalsLds && t.max_chunks <= kLinkChunksLds;
}

// 0: the chunks are formed; 1: the mesh is not one for this path (nothing of `out` is set: the walk forms them); -1: error
static int link_path(LsnTransfer &t, const Chunked &in, int n_triangles, hipStream_t s, Chunked &out)
{
    const int nv = in.n_send, n_pos = 3 * n_triangles;
    LinkState *st = t.l_state.as<LinkState>();
    int *cnt = t.l_cnt.as<int>(), *uses = t.l_uses.as<int>(), *rank = t.l_rank.as<int>(), *start = t.l_start.as<int>(), *vbase = t.l_vbase.as<int>();
    unsigned *prev = t.l_prev.as<unsigned>();
    auto *pack = t.l_pack.as<unsigned long long>();
    auto *totals64 = t.l_totals.as<unsigned long long>();
    int *totals32 = t.l_totals.as<int>();
    LSN_HIP(hipMemsetAsync(st, 0, sizeof(LinkState), s));
    LSN_HIP(hipMemsetAsync(cnt, 0, (size_t)nv * 4, s));
    link_uses_kernel<<<div_up(n_pos, kUsesThreads * kUsesPer), kUsesThreads, 0, s>>>(in.tri, n_pos, nv, cnt, uses, st);
    link_prev_kernel<<<div_up(nv, 256), 256, 0, s>>>(cnt, uses, nv, prev, st);
    link_pack_kernel<<<div_up(n_triangles, 256), 256, 0, s>>>(prev, n_triangles, pack, st);
    const int pb = div_up(n_triangles, kScanPerBlock);
    scan_totals_kernel<unsigned long long><<<pb, 256, 0, s>>>(pack, n_triangles, totals64);
    scan_top_kernel<unsigned long long><<<1, 1024, 0, s>>>(totals64, pb);
    scan_apply_kernel<unsigned long long><<<pb, 256, 0, s>>>(pack, n_triangles, totals64);
    link_chunks_kernel<<<1, 64, 0, s>>>(pack, totals64, n_triangles, t.max_chunks, start, vbase, t.v_chunks.as<int>(), t.t_chunks.as<int>(), st);
    const int rb = div_up(n_pos, kScanPerBlock);
    rank_totals_kernel<<<rb, 256, 0, s>>>(prev, n_pos, start, st, totals32);
    scan_top_kernel<int><<<1, 1024, 0, s>>>(totals32, rb);
    rank_apply_kernel<<<rb, 256, 0, s>>>(prev, n_pos, start, st, totals32, rank);
    link_emit_kernel<<<div_up(n_pos, 256), 256, 0, s>>>(in.tri, prev, n_pos, in.verts, start, vbase, st, rank, t.new_v.as<uint4>(), t.new_tri.as<int>());
    LSN_HIP(hipGetLastError());
    LSN_HIP(hipMemcpyAsync(t.h_link, st, sizeof(LinkState), hipMemcpyDeviceToHost, s));
    LSN_HIP(hipStreamSynchronize(s));
    if (t.h_link->bad) return bad_index(nv);
    if (t.h_link->fallback) return 1;
    out = t.out(t.h_link->n_send, t.h_link->n_chunks);
    return 0;
}
