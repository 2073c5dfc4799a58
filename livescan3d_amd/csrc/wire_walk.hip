// wire_walk.hip -- part of wire.hip's translation unit: formMeshChunks (LiveScanServer/TransferServer.cs:203-270) found chunk after chunk,
// the path for meshes the link path (wire_link.hip) gives up on or has no room for.  Three kernels per window, and the host loop over them.
//
// formMeshChunks is a sequential re-indexing loop in the reference (a vertex is re-emitted the first time a chunk uses it,
// a chunk closes at the first triangle end with >= 64997 vertices).  Here every index position of a window is processed in
// parallel: positions claim their vertex with a 64-bit atomicMin of (chunk, position) -- the winner is the first use inside
// the chunk --, a block-sum + last-block scan finds the triangle that closes the chunk, and the new indices are the ranks of
// the winners.  Only the chunk boundaries are found one after the other (the boundary of chunk c+1 depends on chunk c).

namespace {
constexpr int kTriPerBlock = 256;                            // one triangle (3 index positions) per thread
constexpr int kWindowBlocks = 768;
constexpr int kWindowTri = kWindowBlocks * kTriPerBlock;     // triangles examined per iteration (a chunk of a grid mesh spans ~130 k)

struct ChunkState {
    int s_tri;       // first triangle of the current chunk
    int win_tri;     // first triangle of the current window (>= s_tri)
    int c;           // current chunk id
    int vbase;       // vertices emitted by closed chunks
    int carry;       // vertices of the current chunk found by earlier windows
    int tri_start;   // the reference's trianglesChunkStart (index-position units, :213,:244)
    int done;
    int bad;         // an index outside [0, nV) was seen
    int e_tri;       // count pass: last triangle of this window that belongs to the current chunk
    int closes;      //             the chunk ends at e_tri
    int vcount;      //             vertices of the chunk through e_tri (carry included)
    int p_first;     // triangles [p_first, p_last] wait for their new indices (written by the next tag pass), -1 none
    int p_last;
    unsigned arrive_count;
    unsigned arrive_emit;
    int pad;
};

__device__ __forceinline__ unsigned long long chunk_key(int c, int pos) { return ((unsigned long long)(0xFFFFFFu - (unsigned)c) << 32) | (unsigned)pos; }

// ---- pass 1: (a) new indices of the previous window, (b) claim the vertices of this window -----------------------------
__global__ __launch_bounds__(kTriPerBlock) void chunk_tag_kernel(ChunkState *st, const int *__restrict__ tri, int nT, int nV,
                                                                   unsigned long long *tag, const int *__restrict__ lidx,
                                                                   int *__restrict__ new_tri)
{
    const int tid = blockIdx.x * kTriPerBlock + threadIdx.x;
    const int pf = st->p_first, pl = st->p_last;
    if (pf >= 0 && pf + tid <= pl) {
        const int k = pf + tid;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int val = tri[3 * k + j];
            new_tri[3 * k + j] = (unsigned)val < (unsigned)nV ? lidx[val] : -1;
        }
    }
    if (st->done) return;
    const int k = st->win_tri + tid;
    if (k >= nT) return;
    const int c = st->c;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int val = tri[3 * k + j];
        if ((unsigned)val < (unsigned)nV)
            atomicMin(&tag[val], chunk_key(c, 3 * k + j));
        else
            bad = true;
    }
    if (bad) atomicOr(&st->bad, 1);
}

__device__ __forceinline__ int triangle_new_mask(const int *__restrict__ tri, int k, int nV, int c, const unsigned long long *tag)
{
    int m = 0;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int val = tri[3 * k + j];
        if ((unsigned)val < (unsigned)nV && tag[val] == chunk_key(c, 3 * k + j)) m |= 1 << j;
    }
    return m;
}

// What the workgroups of ONE launch tell each other here goes through agent-scope (write-through) atomic stores and loads, and a
// workgroup counts itself in once those stores have been acknowledged: vmcnt(0).  Not __threadfence(): an agent-scope fence writes back
// and invalidates the XCD's whole L2 (buffer_wbl2 / buffer_inv), per wave that executes it -- measured on ICP's match step, where two
// such fences per workgroup made one fused launch cost 44 us against 24 us for the three launches it replaced
// (profiles/r05_ab_icp_fused_match.txt).  Everything else these kernels write is read by LATER launches.
// This rests on two gfx9 (gfx942 / gfx950) facts, not on the HSA memory model: agent-scope atomics are sc1 write-through accesses that
// reach the memory side, and s_waitcnt's vmcnt counts STORES as well as loads -- on gfx10+ stores have their own counter (vscnt) and
// s_waitcnt(0) would not wait for them.  The library is built for gfx950 only (csrc/Makefile); any other target stops here.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__)
#error "stores_acknowledged() relies on gfx9 semantics (vmcnt covers stores, sc1 write-through atomics): build for gfx950"
#endif
__device__ __forceinline__ void stores_acknowledged()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_waitcnt(0);
}

// One thread of every workgroup of a launch takes a ticket; the last to come holds the highest, and acts for the launch.  A workgroup
// that has published something the last one reads calls stores_acknowledged() first; the last one sets the counter back to zero.
__device__ __forceinline__ bool last_to_arrive(unsigned *counter) { return atomicAdd(counter, 1u) == gridDim.x - 1; }

// ---- pass 2: vertices first used per block; the last block to arrive finds where the chunk closes --------------------------
__global__ __launch_bounds__(kTriPerBlock) void chunk_count_kernel(ChunkState *st, const int *__restrict__ tri, int nT, int nV,
                                                                     const unsigned long long *tag, int *bsum, int *boff)
{
    __shared__ int s_wave[4];
    __shared__ int s_flag;
    __shared__ int s_found_block, s_found_off;
    if (st->done) return;
    const int win = st->win_tri, c = st->c;
    const int k = win + blockIdx.x * kTriPerBlock + threadIdx.x;
    const int cnt = k < nT ? __popc(triangle_new_mask(tri, k, nV, c, tag)) : 0;
    const int incl = block_scan_incl<int, 4>(cnt, s_wave);
    if (threadIdx.x == kTriPerBlock - 1) {
        __hip_atomic_store(&bsum[blockIdx.x], incl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        stores_acknowledged();                                // bsum[] is read by the last block of this launch
        s_flag = last_to_arrive(&st->arrive_count);
    }
    __syncthreads();
    if (!s_flag) return;
    // ---- last block: exclusive offsets of the blocks, and the block in which the running count reaches the limit
    const int carry = st->carry;
    const int nb = gridDim.x;
    if (threadIdx.x == 0) { s_found_block = -1; s_found_off = 0; }
    __syncthreads();
    int running = carry;
    for (int b0 = 0; b0 < nb; b0 += kTriPerBlock) {
        const int b = b0 + threadIdx.x;
        const int v = b < nb ? __hip_atomic_load(&bsum[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        const int inc = block_scan_incl<int, 4>(v, s_wave) + running;
        if (b < nb) {
            boff[b] = inc - v;
            if (inc >= kChunkLimit && inc - v < kChunkLimit) { s_found_block = b; s_found_off = inc - v; }   // unique: inc is monotone
        }
        if (threadIdx.x == kTriPerBlock - 1) s_flag = inc;
        __syncthreads();
        running = s_flag;
        __syncthreads();
    }
    const int fb = s_found_block;
    if (fb >= 0) {
        // the triangle inside block fb at which the count reaches the limit: the chunk closes at its last index (:239)
        const int kk = win + fb * kTriPerBlock + threadIdx.x;
        const int c2 = kk < nT ? __popc(triangle_new_mask(tri, kk, nV, c, tag)) : 0;
        const int inc2 = block_scan_incl<int, 4>(c2, s_wave) + s_found_off;
        if (inc2 >= kChunkLimit && inc2 - c2 < kChunkLimit) {
            st->e_tri = kk;
            st->closes = 1;
            st->vcount = inc2;
        }
    } else if (threadIdx.x == 0) {
        const int nwin = min(kWindowTri, nT - win);
        st->e_tri = win + nwin - 1;
        st->closes = 0;
        st->vcount = running;
    }
    if (threadIdx.x == 0) st->arrive_count = 0;
}

// ---- pass 3: emit the chunk's vertices of this window; the last block to arrive advances the state ------------------------
__global__ __launch_bounds__(kTriPerBlock) void chunk_emit_kernel(ChunkState *st, const int *__restrict__ tri, int nT, int nV,
                                                                    const uint4 *__restrict__ verts, const unsigned long long *tag,
                                                                    const int *__restrict__ boff, int *lidx, uint4 *__restrict__ new_v,
                                                                    int *v_chunks, int *t_chunks)
{
    __shared__ int s_wave[4];
    __shared__ int s_flag;
    if (st->done) return;
    const int win = st->win_tri, c = st->c, e = st->e_tri, vbase = st->vbase;
    const int k = win + blockIdx.x * kTriPerBlock + threadIdx.x;
    const int m = (k <= e && k < nT) ? triangle_new_mask(tri, k, nV, c, tag) : 0;
    const int cnt = __popc(m);
    int li = block_scan_incl<int, 4>(cnt, s_wave) - cnt + boff[blockIdx.x];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        if (m & (1 << j)) {
            const int val = tri[3 * k + j];
            new_v[vbase + li] = verts[val];                   // newVertices[currentVertex] = lVertices[val]  (:234)
            lidx[val] = li;                                   // verticesMap[val] = verticesInCurrentChunk     (:235)
            li++;
        }
    }
    if (threadIdx.x == 0) s_flag = last_to_arrive(&st->arrive_emit);   // nothing published: what this launch wrote, later launches read
    __syncthreads();
    if (!s_flag || threadIdx.x != 0) return;
    st->arrive_emit = 0;
    st->p_first = win;
    st->p_last = e;
    const int vcount = st->vcount;
    ChunkCursor cur{v_chunks, t_chunks, c, vbase, st->tri_start};
    if (st->closes) {
        cur.close(e, vcount, true);
        st->carry = 0;
        st->s_tri = e + 1;
    } else {
        st->carry = vcount;
        if (e + 1 >= nT) cur.end_of_mesh(nT, vcount, true);
    }
    st->c = cur.c; st->vbase = cur.vbase; st->tri_start = cur.tri_start;
    st->win_tri = e + 1;
    if (e + 1 >= nT) st->done = 1;
}

}  // namespace

// The walk: windows of kWindowTri triangles until the mesh ends, four at a time between two looks at the state.  It keeps its own check of
// the indices: a handle too large for the link path comes straight here.
static int walk_path(LsnTransfer &t, const Chunked &in, int n_triangles, hipStream_t s, Chunked &out)
{
    *t.h_state = ChunkState{};
    t.h_state->p_first = t.h_state->p_last = -1;
    LSN_HIP(hipMemcpyAsync(t.state.p, t.h_state, sizeof(ChunkState), hipMemcpyHostToDevice, s));
    LSN_HIP(hipMemsetAsync(t.tag.p, 0xff, (size_t)in.n_send * 8, s));
    ChunkState *st = t.state.as<ChunkState>();
    auto *tag = t.tag.as<unsigned long long>();
    const int nv = in.n_send;
    auto tag_pass = [&] { chunk_tag_kernel<<<kWindowBlocks, kTriPerBlock, 0, s>>>(st, in.tri, n_triangles, nv, tag, t.lidx.as<int>(), t.new_tri.as<int>()); };
    const long long max_iter = n_triangles / kWindowTri + chunk_bound(0, n_triangles) + 2;
    long long it = 0;
    bool done = false;
    while (!done) {
        for (int r = 0; r < 4; r++, it++) {
            tag_pass();
            chunk_count_kernel<<<kWindowBlocks, kTriPerBlock, 0, s>>>(st, in.tri, n_triangles, nv, tag, t.bsum.as<int>(), t.boff.as<int>());
            chunk_emit_kernel<<<kWindowBlocks, kTriPerBlock, 0, s>>>(st, in.tri, n_triangles, nv, in.verts, tag, t.boff.as<int>(), t.lidx.as<int>(),
                                                                     t.new_v.as<uint4>(), t.v_chunks.as<int>(), t.t_chunks.as<int>());
        }
        LSN_HIP(hipMemcpyAsync(t.h_state, t.state.p, sizeof(ChunkState), hipMemcpyDeviceToHost, s));
        LSN_HIP(hipStreamSynchronize(s));
        done = t.h_state->done != 0;
        if (!done && it > max_iter) { lsn::set_error("lsnTransferPack: chunk search did not terminate"); return -1; }
    }
    tag_pass();   // the new indices of the last window (idempotent when a pass after the last emit already wrote them)
    if (t.h_state->bad) {
        (void)hipStreamSynchronize(s);
        return bad_index(nv);
    }
    out = t.out(t.h_state->vbase, t.h_state->c);
    return 0;
}
