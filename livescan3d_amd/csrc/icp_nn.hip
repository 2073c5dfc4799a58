// icp_nn.hip -- the ICP's exact nearest-neighbour step and the one-to-one claim.  Compiled as part of icp.hip's translation unit; it relies
// on icp_grid.hip (the grid's constants, GridParams, Box, QueryBox, the box distances, cell_coord / cell_index, GridBufs, blocks_for) and on
// what icp.hip defines in front of its include: IcpState (the seeded cull applies the previous iteration's motion and reads near_next) and
// LsnIcp (run_nn works on a workspace).
//
// Two searches, the same bits: a brute force (nn_mode 0, the ablation leg: one query per lane, the targets streamed through scalar loads /
// SGPRs, no LDS) and the voxel-grid search by QUERY GROUPS of 64 sorted queries with the NEAR PATH in front of it (see those sections).
// Distances are evaluated exactly like PointCloud::kdtree_distance (include/NativeUtils/icp.h:40-47): (d0*d0 + d1*d1) + d2*d2, no FMA.
// Equal distances resolve to the lowest target index (nanoflann's tie order is traversal dependent).  One-to-one matching: claim_key.
namespace {

constexpr int kChunk = 256;            // points per scan item (4 LDS batches of 64)
constexpr int kSeedBlocks = 4;        // blocks nearest to a query patch that are scanned first when it has no candidates yet

// A query's search key: (distance bits << 32 | target index); distances are >= +0, so atomicMin on it is the lexicographic minimum.
constexpr int kNoIndex = 0x7FFFFFFF;  // no target yet; above every real index, so any real point at the same distance beats it
constexpr unsigned long long kNoKey = (0x7F800000ull << 32) | (unsigned int)kNoIndex;  // (+inf, no index)

__device__ __forceinline__ unsigned long long pack_key(float d, int k)
{
    return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned int)k;
}
__device__ __forceinline__ float key_dist(unsigned long long key) { return __uint_as_float((unsigned int)(key >> 32)); }
__device__ __forceinline__ int key_index(unsigned long long key) { return (int)(unsigned int)key; }

// A target's claim key: (distance bits << 32 | ~source index) -- under a 64-bit atomicMin per target the smallest distance wins and, among
// equal distances, the LATER source: what the sequential scan at icp.cpp:95-126 ends with.  claim_source: whose claim a target's key holds.
__device__ __forceinline__ unsigned long long claim_key(float d, int i) { return pack_key(d, (int)(0xFFFFFFFFu - (unsigned int)i)); }
__device__ __forceinline__ int claim_source(unsigned long long key) { return (int)(0xFFFFFFFFu - (unsigned int)key); }

__device__ __forceinline__ bool finite3(float x, float y, float z) { return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY; }

__device__ __forceinline__ float dist2(float qx, float qy, float qz, float px, float py, float pz)
{
    const float d0 = qx - px;
    const float d1 = qy - py;
    const float d2 = qz - pz;
    return d0 * d0 + d1 * d1 + d2 * d2;  // (d0*d0 + d1*d1) + d2*d2, contraction is off
}

// The claims of a whole workgroup.  In a scene most queries of a patch share a handful of targets (the rim of the other
// sensor's surface): one global atomicMin per query then piles thousands of atomics onto single addresses, which the L2
// serialises (measured: 100 us for 108 k claims).  The workgroup therefore first combines its claims in LDS -- a
// direct-mapped table of kClaimSlots (target, smallest key) pairs filled with LDS atomics; a query whose slot is taken by
// another target claims in global memory directly -- and then issues one global atomicMin per occupied slot, skipped
// when the target's key is already smaller.  Same result: a minimum of minima.  Must be reached by every thread.
constexpr int kClaimSlots = 1024;
__device__ __forceinline__ void claim_targets(unsigned long long *keys, bool active, int k, float d, int i, int *slot_k, unsigned long long *slot_v)
{
    for (int t = threadIdx.x; t < kClaimSlots; t += kThreads) {
        slot_k[t] = -1;
        slot_v[t] = ~0ull;
    }
    __syncthreads();
    if (active) {
        const unsigned long long key = claim_key(d, i);
        const int slot = k & (kClaimSlots - 1);
        const int owner = atomicCAS(&slot_k[slot], -1, k);
        if (owner == -1 || owner == k)
            atomicMin(&slot_v[slot], key);
        else if (keys[k] > key)
            atomicMin(&keys[k], key);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < kClaimSlots; t += kThreads) {
        const int tk = slot_k[t];
        if (tk >= 0) {
            const unsigned long long v = slot_v[t];
            if (keys[tk] > v) atomicMin(&keys[tk], v);
        }
    }
}

// In-wave LDS hand-over: LDS instructions of one wave execute in order, so a ds_write of all lanes followed by ds_reads of
// the same wave needs no hardware wait -- only the compiler must not move the accesses across this point.
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct alignas(16) WaveStage {  // 64 candidate points of one wave, structure of arrays: 4 consecutive points = one 16-B LDS read
    float x[64], y[64], z[64];
    int i[64];
};

typedef float f2v __attribute__((ext_vector_type(2)));
typedef float f4v __attribute__((ext_vector_type(4)));
typedef int i4v __attribute__((ext_vector_type(4)));

// dist2 of one query against four points, as packed f32 pairs (v_pk_add_f32 with negated operand, v_pk_mul_f32): one
// rounding per operation and the order (d0*d0 + d1*d1) + d2*d2 of PointCloud::kdtree_distance (icp.h:40-47); contraction is off.
__device__ __forceinline__ f4v dist2x4(f2v qx, f2v qy, f2v qz, f4v X, f4v Y, f4v Z)
{
    const f2v ax = qx - X.xy, bx = qx - X.zw;
    const f2v ay = qy - Y.xy, by = qy - Y.zw;
    const f2v az = qz - Z.xy, bz = qz - Z.zw;
    const f2v a = ax * ax + ay * ay + az * az;
    const f2v b = bx * bx + by * by + bz * bz;
    f4v d;
    d.xy = a;
    d.zw = b;
    return d;
}

__device__ __forceinline__ void scan_batch(const float4 &p, int cnt, WaveStage &st, int lane, f2v qx2, f2v qy2, f2v qz2, float &best, int &best_i)
{
    st.x[lane] = p.x;
    st.y[lane] = p.y;
    st.z[lane] = p.z;
    st.i[lane] = __float_as_int(p.w);
    wave_lds_fence();
    for (int t = 0; t < cnt; t += 8) {  // two independent groups of four per step (fills the issue slots between dependent packed ops)
        const f4v d = dist2x4(qx2, qy2, qz2, *reinterpret_cast<const f4v *>(&st.x[t]), *reinterpret_cast<const f4v *>(&st.y[t]),
                              *reinterpret_cast<const f4v *>(&st.z[t]));
        const f4v e = dist2x4(qx2, qy2, qz2, *reinterpret_cast<const f4v *>(&st.x[t + 4]), *reinterpret_cast<const f4v *>(&st.y[t + 4]),
                              *reinterpret_cast<const f4v *>(&st.z[t + 4]));
        const float m = fminf(fminf(fminf(d.x, d.y), fminf(d.z, d.w)), fminf(fminf(e.x, e.y), fminf(e.z, e.w)));  // fminf skips NaN
        if (__ballot(m <= best)) {                                                                                 // wave-uniform branch
            // some lane is improved or tied: the step's candidate of a lane is (m, lowest index among its points at distance m),
            // branch-free (16 compares / selects and a min tree instead of eight conditional updates)
            const i4v K = *reinterpret_cast<const i4v *>(&st.i[t]);
            const i4v L = *reinterpret_cast<const i4v *>(&st.i[t + 4]);
            const int none = kNoIndex;
            const int k0 = d.x == m ? K.x : none, k1 = d.y == m ? K.y : none, k2 = d.z == m ? K.z : none, k3 = d.w == m ? K.w : none;
            const int k4 = e.x == m ? L.x : none, k5 = e.y == m ? L.y : none, k6 = e.z == m ? L.z : none, k7 = e.w == m ? L.w : none;
            const int km = min(min(min(k0, k1), min(k2, k3)), min(min(k4, k5), min(k6, k7)));
            const bool take = (m < best) | ((m == best) & (km < best_i));
            best = take ? m : best;
            best_i = take ? km : best_i;
        }
    }
    wave_lds_fence();
}

__device__ __forceinline__ float4 load_point_or_pad(const float4 *__restrict__ sorted, int j, int je)
{
    float4 p = make_float4(NAN, NAN, NAN, __int_as_float(kNoIndex));  // padding: its distance is NaN, never taken
    if (j < je) p = sorted[j];
    return p;
}

// Every lane (one query each) against the points sorted[js, je): the wave loads 64 points at a time with one coalesced
// 16-byte load per lane -- up to four such batches in flight at once, one memory round trip per kChunk points -- parks a
// batch in its LDS stage and then walks it eight points at a time: all lanes read the same LDS address (broadcast), the
// differences / products / sums run as packed f32 pairs (one rounding per operation, the order of
// PointCloud::kdtree_distance, icp.h:40-47).  Only the minimum of the eight distances is compared with the lane's best;
// the (distance, index) bookkeeping runs in the rare case that some lane of the wave is improved or tied.
__device__ __forceinline__ void scan_points(const float4 *__restrict__ sorted, int js, int je, WaveStage &st, int lane, float qx, float qy,
                                            float qz, float &best, int &best_i)
{
    const f2v qx2 = {qx, qx}, qy2 = {qy, qy}, qz2 = {qz, qz};
    for (int base = js; base < je; base += kChunk) {
        const float4 p0 = load_point_or_pad(sorted, base + lane, je);
        const float4 p1 = load_point_or_pad(sorted, base + 64 + lane, je);
        const float4 p2 = load_point_or_pad(sorted, base + 128 + lane, je);
        const float4 p3 = load_point_or_pad(sorted, base + 192 + lane, je);
        const int left = je - base;  // wave-uniform
        scan_batch(p0, min(64, left), st, lane, qx2, qy2, qz2, best, best_i);
        if (left > 64) scan_batch(p1, min(64, left - 64), st, lane, qx2, qy2, qz2, best, best_i);
        if (left > 128) scan_batch(p2, min(64, left - 128), st, lane, qx2, qy2, qz2, best, best_i);
        if (left > 192) scan_batch(p3, min(64, left - 192), st, lane, qx2, qy2, qz2, best, best_i);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// QUERY GROUPS: exact nearest neighbour for 64 SPATIALLY SORTED QUERIES AT A TIME ("query group" = one wave's worth).  The source cloud
// is sorted once per call along its own voxel order, so a group is a compact patch (about one 4^3-cell block) and -- the
// motion being rigid -- stays one for every iteration.  A patch shares its candidates: instead of 64 private tree walks
// (one wave per far query, each a chain of dependent loads) the two-level box hierarchy is culled once per
// group against the box W of its queries, 64 boxes per step, one per lane, and every surviving block is streamed through
// LDS for all 64 queries at once.
//
// The search is cut into INDEPENDENT work items so that no wave ever runs a chain of dependent memory round trips and
// no slow wave holds the launch up (measured: the one-kernel form below, kept as the overflow fallback, was bound by its
// slowest wave -- ~200 us for ~50 dependent loads -- while the average wave needed 370 candidate points):
//   nn_cull_kernel    one wave per group: seed every query with its previous neighbour (a REAL target point, so the
//                     result does not depend on it), W, the largest bound; emits (group, super-block) items
//   nn_blocks_kernel  one wave per item: the super-block's 64 block boxes, one per lane, against W, then against every
//                     query's own bound; emits (group, point range) items, at most 128 points each
//   nn_scan_kernel    one wave per item: 64 queries x the range's points through LDS, packed f32; the lexicographic
//                     (distance, index) minimum is merged into the query's 64-bit key with atomicMin
//   nn_finish_kernel  one thread per query: index / distance out (original order) + the one-to-one claim
// Without seeds (first ICP iteration, lsnIcpNearest) nn_probe_kernel first lets every query look around its own cell and emits
// the blocks nearest to the queries that found nothing as scan items; their minima are the seeds.
//
// Exactness: a query's key only ever takes (distance, index) pairs of real target points, and a box is passed over only
// when no query of the group can need it: the group test opens a box when boxbox_min_dist2(W, box) <= max_l bound_l,
// which holds whenever some lane's own box_min_dist2(q_l, box) <= bound_l (see boxbox_min_dist2); the per-lane test
// skips a box only when its exact f32 lower bound EXCEEDS every lane's bound, so equal-distance candidates are still
// evaluated and the lowest index wins, like everywhere else.  The bounds are fixed for the whole step (the seeds); they
// are distances of real points, so every point that could beat or tie them is inside an opened box.
// The item lists have a fixed capacity; if one overflows (pathological inputs: no usable seeds, far outliers everywhere)
// the finish kernel runs the complete walk (wave_search) for every group instead -- slower, same result.
//
// Queries with a non-finite coordinate do not take part in the culling (they would open every box); they end with
// index 0 / distance +inf, which is what the search gives them when target 0 is finite.

struct GroupInfo {  // per query group, written by nn_cull_kernel
    QueryBox w;                          // W: the box of the group's queries that still search
    float rmax;                          // largest bound among them (-1: nobody searches)
    int pad;
    unsigned long long resolved;         // lanes whose key is already final (the near path below): they open no box
};
static_assert(sizeof(GroupInfo) == 40 && offsetof(GroupInfo, resolved) == 32, "lsnIcpNearResolved reads the groups back on the host");

// W of one wave's queries (lane = query): the box of those with `take` set.
__device__ __forceinline__ QueryBox wave_query_box(bool take, float qx, float qy, float qz)
{
    return {wave_min(take ? qx : INFINITY),  wave_min(take ? qy : INFINITY),  wave_min(take ? qz : INFINITY),
            wave_max(take ? qx : -INFINITY), wave_max(take ? qy : -INFINITY), wave_max(take ? qz : -INFINITY)};
}

// Block b's box out of bb = a super-block's 64 block boxes, one per lane: broadcast from lane b (b is wave-uniform).
__device__ __forceinline__ Box lane_box(const Box &bb, int b)
{
    auto from_b = [b](float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), b)); };
    return {from_b(bb.lx), from_b(bb.ly), from_b(bb.lz), from_b(bb.hx), from_b(bb.hy), from_b(bb.hz), 0, 0};
}

constexpr int kSegs = 64;        // the work lists are cut into 64 segments with a counter each: an append is one atomicAdd per
                                 // wave on the counter of segment (group mod 64) -- a single counter serialised ~10^4 atomics
                                 // per step on one address (measured: 30-50 us per launch)
constexpr int kSegStride = 32;  // ints between two segments' counters: one 128-byte line each -- atomics on one line serialise in its L2 channel
                                // whatever the address (measured: 8 k appends on 64 adjacent counters took as long as on one)
constexpr int kCntA = 0, kCntB = 1, kCntSeed = 2;          // a segment's counters inside its line: list A, list B, seed-round part of B
constexpr int kOverflow = kSegs * kSegStride;              // the bank's overflow flag
constexpr int kBankInts = kSegs * kSegStride + kSegStride; // ints per bank

struct NnWork {  // device work lists of one ICP workspace
    uint2 *list_a;      // (group, super-block), segment s = entries [s * seg_a, (s + 1) * seg_a)
    int4 *list_b;       // (group, first point, end point, -)
    int seg_a, seg_b;   // segment capacities
    int item_points;    // points per scan item (a multiple of 64, <= kChunk)
    int *counters;      // two banks of kBankInts
};

// Consumers: wave w of a launch serves segment (w mod 64), entries w / 64, w / 64 + waves / 64, ...: the segment's length
// and the wave's first entry are independent loads (one memory round trip before the work starts, no prefix sums).
// One wave per workgroup: a slot on the CU is free again as soon as its wave is done.  count: kCntA, kCntB or kCntSeed; body(item) serves one
// entry.  Both consumers' listings were compared with their own loops' (EXPERIMENTS.md, "Fold icp.hip"): nn_blocks_kernel is the same instruction
// for instruction; nn_scan_kernel has the same loads in the same order, other SGPR numbers and one s_nop between two scalar loads.
template <class Item, class Body>
__device__ __forceinline__ void for_each_item(const Item *lists, int seg_cap, const int *bank, int count, Body &&body)
{
    const int wave_id = blockIdx.x, stride = gridDim.x >> 6, seg = wave_id & (kSegs - 1);
    const Item *list = lists + (size_t)seg * seg_cap;
    int slot = wave_id >> 6;
    Item item = list[min(slot, seg_cap - 1)];  // speculative: issued together with the length
    const int n_items = min(bank[seg * kSegStride + count], seg_cap);
    for (; slot < n_items; slot += stride, item = list[min(slot, seg_cap - 1)]) body(item);
}

// Appends the point range [js, je) of every lane with `take` set to list B as (group, range) items of <= item_points points.
// `spread` picks the segment: a heavy group's ranges are spread over the segments by its super-blocks.
__device__ __forceinline__ void emit_ranges(const NnWork &wk, int *bank, int which, int g, int spread, bool take, int js, int je, int lane)
{
    const int n_items = take ? (je - js + wk.item_points - 1) / wk.item_points : 0;
    const int before = wave_scan_incl(n_items, lane) - n_items;
    const int total = __shfl(before + n_items, 63, 64);
    if (total == 0) return;  // wave-uniform
    const int seg = spread & (kSegs - 1);
    int base = 0;
    if (lane == 0) base = atomicAdd(bank + seg * kSegStride + which, total);
    base = __shfl(base, 0, 64);
    if (base + total > wk.seg_b) {  // (the seed round's items are consumed before the search's are written: both start at 0)
        if (lane == 0) atomicExch(bank + kOverflow, 1);
        return;
    }
    for (int c = 0; c < n_items; c++) {
        const int a = js + c * wk.item_points;
        wk.list_b[(size_t)seg * wk.seg_b + base + before + c] = make_int4(g, a, min(a + wk.item_points, je), 0);
    }
}

// Where a group without candidates starts (one wave; w: the box of the queries that need a seed): the super-block nearest to w (returned; -1:
// no target point with comparable coordinates at all), its 64 block boxes with their point ranges (bb, one per lane) and the mask of its
// kSeedBlocks blocks nearest to w (fewer when fewer hold points).  Ties go to the lowest index at both levels.
__device__ __forceinline__ int nearest_seed_blocks(const GridParams *__restrict__ gp, const Box *__restrict__ boxes, const Box *__restrict__ supers,
                                                   const QueryBox &w, int lane, Box &bb, unsigned long long &chosen)
{
    chosen = 0;
    const int n_supers = gp->ncells / 4096;
    float m_best = INFINITY;
    int s_best = 0;
    for (int c0 = 0; c0 < n_supers; c0 += 64) {
        const int sl = c0 + lane;
        if (sl < n_supers) {
            const float m = boxbox_min_dist2(w, supers[sl]);
            if (m < m_best) {
                m_best = m;
                s_best = sl;
            }
        }
    }
    const float wm = wave_min(m_best);
    if (!(wm < INFINITY)) return -1;
    const int seed_super = __shfl(s_best, __ffsll((long long)__ballot(m_best == wm)) - 1, 64);
    bb = boxes[seed_super * 64 + lane];
    float mb = boxbox_min_dist2(w, bb);
    for (int t = 0; t < kSeedBlocks; t++) {
        const float wmb = wave_min(mb);
        if (!(wmb < INFINITY)) break;
        const int b = __ffsll((long long)__ballot(mb == wmb)) - 1;
        chosen |= 1ull << b;
        if (lane == b) mb = INFINITY;
    }
    return seed_super;
}

// The complete walk for one group in one wave: seeds the search from the nearest blocks when some query has no candidate,
// then opens every super-block / block that a query may need, tightening the bounds as it goes.  Exact for any input;
// used when the item lists overflow.
__device__ void wave_search(const GridParams *__restrict__ gp, const float4 *__restrict__ sorted, const Box *__restrict__ boxes,
                            const Box *__restrict__ supers, WaveStage &st, int lane, float qx, float qy, float qz, bool part, float &best,
                            int &best_i)
{
    if (!__ballot(part)) return;
    const QueryBox w = wave_query_box(part, qx, qy, qz);
    const int n_supers = gp->ncells / 4096;
    int seed_super = -1;
    unsigned long long seed_done = 0;
    if (__ballot(part && !(best < INFINITY))) {
        // some query has no candidate yet: scan the blocks nearest to the patch first (any real point bounds the search) -- in ascending
        // block index, not nearest first: the merge is a lexicographic (distance, index) minimum, so the order does not change a bit
        Box bb;
        seed_super = nearest_seed_blocks(gp, boxes, supers, w, lane, bb, seed_done);
        for (unsigned long long todo = seed_done; todo; todo &= todo - 1) {
            const int b = __ffsll((long long)todo) - 1;
            const int js = __builtin_amdgcn_readlane(__float_as_int(bb.pad0), b), je = __builtin_amdgcn_readlane(__float_as_int(bb.pad1), b);
            scan_points(sorted, js, je, st, lane, qx, qy, qz, best, best_i);
        }
    }
    float bound = part ? best : -1.0f;  // a lane outside the search never opens a box
    float rmax = wave_max(bound);
    for (int c0 = 0; c0 < n_supers; c0 += 64) {
        const int sl = c0 + lane;
        float m = INFINITY;
        if (sl < n_supers) m = boxbox_min_dist2(w, supers[sl]);
        unsigned long long open = __ballot(m <= rmax && m < INFINITY);
        while (open) {
            const int s = c0 + __ffsll((long long)open) - 1;
            open &= open - 1;
            // the super-block's 64 blocks, one per lane, with their point ranges
            const Box bb = boxes[s * 64 + lane];
            const float mb = boxbox_min_dist2(w, bb);
            unsigned long long cand = __ballot(mb <= rmax && mb < INFINITY);
            if (s == seed_super) cand &= ~seed_done;
            while (cand) {
                const int b = __ffsll((long long)cand) - 1;
                cand &= cand - 1;
                const Box xb = lane_box(bb, b);
                if (!__ballot(box_min_dist2(qx, qy, qz, xb) <= bound)) continue;  // no lane can find anything nearer or tied in it
                const int js = __builtin_amdgcn_readlane(__float_as_int(bb.pad0), b), je = __builtin_amdgcn_readlane(__float_as_int(bb.pad1), b);
                scan_points(sorted, js, je, st, lane, qx, qy, qz, best, best_i);
                bound = part ? best : -1.0f;
            }
            rmax = wave_max(bound);
            open &= __ballot(m <= rmax);  // super-blocks of this chunk that the tighter bounds rule out need not be opened
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The NEAR PATH: a query that knows a REAL target point near it walks the target grid's cells around it by itself -- a
// handful of candidates instead of its group's ~800 -- and its key is final.  What the kd-tree does for such a query
// (include/nanoflann.h:1200-1247: the leaf the query falls in and the few leaves its ball touches), with the grid's cells
// as the leaves.  Two forms:
//   seeded (nn_cull_kernel<true>)  the bound B is the f32 squared distance of the query's previous neighbour; the cells the ball
//                                  of B touches are walked, and the result is final;
//   probe (nn_probe_kernel)        no bound yet: the 27 cells around the query's own cell are walked; the result is final when
//                                  the ball of the best distance found stays inside those cells, a seed for the group search otherwise.
//
// Exactness.  dist2 = fl(fl(fl(d0*d0) + fl(d1*d1)) + fl(d2*d2)), d_a = fl(q_a - p_a).  Every term is >= 0 and rounding is
// monotone, so fl(d_a*d_a) <= dist2 for each axis.  With r such that fl(r*r) > B (checked, not assumed), any p with
// dist2(q, p) <= B has |d_a| < r on every axis; fl(q_a - p_a) is off from q_a - p_a by <= 2^-24 relative, so
// |q_a - p_a| < r (1 + 2^-23), and with r2 = r * 1.0001 + |q_a| * 2.4e-7 the f32 values lo = fl(q_a - r2), hi = fl(q_a + r2)
// satisfy lo <= p_a <= hi (the two margins cover the roundings of r2 and of the subtraction / addition).  cell_coord is
// monotone in its first argument (an f32 subtraction of o, a multiplication by inv_h > 0, floor, clamp), and it is the
// very function -- same GridParams -- that binned the targets: every such p lies in a cell of
// [cell(lo), cell(hi)]^3.  A walk over a box of cells that contains those takes (d < best) or (d == best and a lower index)
// starting from (B, that real point's index): the result is the lexicographic (distance, index) minimum over ALL targets,
// like the hierarchy's.  A target with a NaN coordinate never wins anywhere (its distance is NaN).  The path is taken only
// when the box spans <= kNearSpan cells per axis and holds <= max_pts points; everything else goes through the query
// groups below.
//
// Work split (measured, EXPERIMENTS.md R6-1: a lane -- or a team of 4 / 8 lanes -- walking its query's cells alone leaves the launch
// waiting for the few workgroups whose queries sit in crowded cells: 9-15 us of walk at the 95th percentile against 0.2 us at the
// median): the workgroup is one query group and shares ALL its candidates out evenly.  Wave 0 prepares the 64 queries (lane =
// query); a team of 4 consecutive lanes per query fetches the cell ranges of the box's runs (a row of cells along x is one run
// of consecutive cell indices inside a 4-cell block row, two when it crosses into the next block) and appends them to the
// workgroup's list in LDS as chunks of <= 8 consecutive points; then every thread takes chunks from that list -- eight
// loads in flight per chunk -- and merges the chunk's (distance, index) minimum into its query's key with
// a 64-bit LDS atomicMin (the lexicographic minimum: distances are >= +0, so their bit patterns order like their values).
constexpr int kNearSpan = 3;
constexpr int kNearRows = kNearSpan * kNearSpan;
constexpr int kNearRuns = 2 * kNearRows;     // runs per query at most
constexpr int kTeam = 4;                     // lanes per query in the team phase; the workgroup is 64 x kTeam threads
constexpr int kCullThreads = 64 * kTeam;
constexpr int kChunkPts = 8;                 // points per chunk = loads in flight per thread and chunk
constexpr int kNearCapMax = 128;             // largest candidate cap per query
constexpr int kMaxChunks = 64 * (kNearCapMax / kChunkPts + kNearRuns);   // a run of n points is ceil(n / 8) chunks

struct NearBox {   // a query's box of cells (inclusive), filled by lane = query, read by its team
    int xl, xh, yl, yh, zl, zh;
    int want;      // the query takes the near path (after near_enqueue: and its box held <= the cap)
    int pad;
};

struct NearShared {   // LDS of one query group
    float4 q[64];              // x, y, z, bound
    unsigned long long key[64];
    NearBox box[64];
    int flag[64];              // seeded: resolved; probe: bit 0 resolved, bit 1 has a key
    int n_chunks;
    int2 chunks[kMaxChunks];   // (first point, query | points << 8)
};

__device__ __forceinline__ bool near_radius(float B, const GridParams &g, float &r)
{
    r = fmaxf(sqrtf(B) * 1.00001f, 1e-18f);
    return r * r > B && r < 1e18f && g.inv_h > 0.0f && g.inv_h < INFINITY;
}

__device__ __forceinline__ void near_axis(float q, float r, float o, float inv_h, int n, int &lo, int &hi)
{
    const float r2 = r * 1.0001f + fabsf(q) * 2.4e-7f;
    lo = cell_coord(q - r2, o, inv_h, n);
    hi = cell_coord(q + r2, o, inv_h, n);
}

// lane = query: the cells the ball of B around q touches; want = it is small enough for the near path
__device__ __forceinline__ NearBox near_ball_box(const GridParams &g, bool want, float qx, float qy, float qz, float B)
{
    NearBox b = {0, 0, 0, 0, 0, 0, 0, 0};
    float r;
    if (want && near_radius(B, g, r)) {
        near_axis(qx, r, g.ox, g.inv_h, g.nx, b.xl, b.xh);
        near_axis(qy, r, g.oy, g.inv_h, g.ny, b.yl, b.yh);
        near_axis(qz, r, g.oz, g.inv_h, g.nz, b.zl, b.zh);
        b.want = b.xh - b.xl < kNearSpan && b.yh - b.yl < kNearSpan && b.zh - b.zl < kNearSpan;
    }
    return b;
}

// Team phase (all kCullThreads threads; thread = (query ql, lane sub of its team); sh.n_chunks is zero and the boxes are in LDS):
// the runs of the query's box become chunks of the workgroup's list when the box holds <= max_pts (<= kNearCapMax) points;
// sh.box[ql].want says so afterwards.
template <bool PROBE>
__device__ __forceinline__ void near_enqueue(NearShared &sh, const GridParams &g, const int *__restrict__ cell_start, int max_pts, int ql, int sub)
{
    constexpr int kMine = (kNearRuns + kTeam - 1) / kTeam;
    const NearBox bx = sh.box[ql];
    bool want = bx.want != 0;
    if (!__ballot(want)) return;   // wave-uniform
    const int xb = min(bx.xh, bx.xl | 3);
    const bool two = bx.xh > xb;
    const int nyr = bx.yh - bx.yl + 1, n_rows = nyr * (bx.zh - bx.zl + 1);
    const int n_runs = want ? (two ? 2 * n_rows : n_rows) : 0;
    int s[kMine], e[kMine];
    int total = 0;
#pragma unroll
    for (int m = 0; m < kMine; m++) {
        const int k = sub + m * kTeam;
        s[m] = e[m] = 0;
        if (k < n_runs) {
            const int row = two ? k >> 1 : k;
            const bool second = two && (k & 1);
            const int dz = (row >= nyr) + (row >= 2 * nyr), dy = row - dz * nyr;
            const int c = cell_index(second ? xb + 1 : bx.xl, bx.yl + dy, bx.zl + dz, g);
            s[m] = cell_start[c];
            e[m] = cell_start[c + (second ? bx.xh - xb : xb - bx.xl + 1)];
        }
        total += e[m] - s[m];
    }
#pragma unroll
    for (int off = 1; off < kTeam; off <<= 1) total += __shfl_xor(total, off, 64);
    const bool fits = total <= min(max_pts, kNearCapMax);
    // a crowded box: left to the group search; the probe still takes a few of its points -- any real point is a seed (want = 2)
    if (want && !fits && sub == 0) sh.box[ql].want = PROBE ? 2 : 0;
    if (PROBE && want && !fits && e[0] > s[0]) {
        const int base = atomicAdd(&sh.n_chunks, 1);
        sh.chunks[base] = make_int2(s[0], ql | (min(kChunkPts, e[0] - s[0]) << 8));
    }
    want = want && fits;
#pragma unroll
    for (int m = 0; m < kMine; m++) {
        const int n = want ? (e[m] - s[m] + kChunkPts - 1) / kChunkPts : 0;
        if (n > 0) {
            const int base = atomicAdd(&sh.n_chunks, n);   // <= kMaxChunks in total: every query's runs hold <= kNearCapMax points
            for (int c = 0; c < n; c++) {
                const int j = s[m] + kChunkPts * c;
                sh.chunks[base + c] = make_int2(j, ql | (min(kChunkPts, e[m] - j) << 8));
            }
        }
    }
}

// All threads, behind a barrier: the workgroup's chunks; sh.key[q] ends as the lexicographic minimum of
// its start value and every point of the query's box.
__device__ __forceinline__ void near_consume(NearShared &sh, const float4 *__restrict__ sorted)
{
    const int n = sh.n_chunks;
    auto fetch = [&](int2 ck, float4 (&p)[kChunkPts]) {
#pragma unroll
        for (int u = 0; u < kChunkPts; u++)
            if (u < (ck.y >> 8)) p[u] = sorted[ck.x + u];
    };
    auto merge = [&](int2 ck, const float4 (&p)[kChunkPts]) {
        const int q = ck.y & 63, cnt = ck.y >> 8;
        const float4 qq = sh.q[q];
        float b = INFINITY;
        int bi = kNoIndex;
#pragma unroll
        for (int u = 0; u < kChunkPts; u++) {
            const float d = dist2(qq.x, qq.y, qq.z, p[u].x, p[u].y, p[u].z);
            const int i = __float_as_int(p[u].w);
            const bool take = (u < cnt) & ((d < b) | ((d == b) & (i < bi)));   // NaN: never
            b = take ? d : b;
            bi = take ? i : bi;
        }
        const unsigned long long key = pack_key(b, bi);
        if (cnt > 0 && b < INFINITY && key < sh.key[q]) atomicMin(&sh.key[q], key);
    };
    for (int c = threadIdx.x; c < n; c += kCullThreads) {
        const int2 ck = sh.chunks[c];
        float4 p[kChunkPts];
        fetch(ck, p);
        merge(ck, p);
    }
}

// The kSeedBlocks blocks nearest to the box W of a group's queries (inside the nearest super-block) become scan items of the seed
// round; what they yield seeds the real search (any real point bounds it).  One wave, lane = query; `need`: the lane takes part.
__device__ __forceinline__ void emit_seed_blocks(const GridParams *__restrict__ gp, const Box *__restrict__ boxes, const Box *__restrict__ supers,
                                                 const NnWork &wk, int bank, int g, int lane, bool need, float qx, float qy, float qz)
{
    if (!__ballot(need)) return;
    Box bb;
    unsigned long long chosen;
    if (nearest_seed_blocks(gp, boxes, supers, wave_query_box(need, qx, qy, qz), lane, bb, chosen) < 0) return;
    emit_ranges(wk, wk.counters + kBankInts * bank, kCntSeed, g, g, (chosen >> lane) & 1, __float_as_int(bb.pad0), __float_as_int(bb.pad1), lane);
}

// No seeds yet (first ICP iteration, lsnIcpNearest).  One workgroup per query group.  Every query's key starts empty; the probe
// (near_pts > 0) walks the 27 cells around the query's own cell: a query whose best find's ball stays inside them is settled
// (groups[g].resolved, read by nn_cull_kernel<false>), any other find is the query's seed.  When some query of the group still has
// no key, the blocks nearest to those queries become scan items of the seed round.
__global__ __launch_bounds__(kCullThreads) __attribute__((amdgpu_waves_per_eu(7, 8))) void nn_probe_kernel(const float4 *__restrict__ src, int n2, const GridParams *__restrict__ gp,
                                                                const Box *__restrict__ boxes, const Box *__restrict__ supers,
                                                                unsigned long long *best_key, GroupInfo *groups, NnWork wk, int bank,
                                                                const int *__restrict__ cell_start, const float4 *__restrict__ sorted, int near_pts)
{
    __shared__ NearShared sh;
    const int g = blockIdx.x;
    if (g * 64 >= n2) return;  // workgroup-uniform
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const GridParams grid = *gp;
    if (wave == 0) {
        const int j = g * 64 + lane;
        float4 q4 = make_float4(NAN, NAN, NAN, 0.0f);
        if (j < n2) q4 = src[j];
        const bool part = j < n2 && finite3(q4.x, q4.y, q4.z);
        NearBox b = {0, 0, 0, 0, 0, 0, 0, 0};
        if (near_pts > 0 && part && grid.inv_h > 0.0f && grid.inv_h < INFINITY) {
            const int cx = cell_coord(q4.x, grid.ox, grid.inv_h, grid.nx), cy = cell_coord(q4.y, grid.oy, grid.inv_h, grid.ny),
                      cz = cell_coord(q4.z, grid.oz, grid.inv_h, grid.nz);
            b.xl = max(cx - 1, 0); b.xh = min(cx + 1, grid.nx - 1);
            b.yl = max(cy - 1, 0); b.yh = min(cy + 1, grid.ny - 1);
            b.zl = max(cz - 1, 0); b.zh = min(cz + 1, grid.nz - 1);
            b.want = 1;
        }
        sh.q[lane] = make_float4(q4.x, q4.y, q4.z, part ? 0.0f : -1.0f);
        sh.box[lane] = b;
        sh.flag[lane] = 0;
        sh.key[lane] = kNoKey;
        if (lane == 0) sh.n_chunks = 0;
    }
    __syncthreads();
    if (near_pts > 0) {
        near_enqueue<true>(sh, grid, cell_start, near_pts, threadIdx.x / kTeam, threadIdx.x % kTeam);
        __syncthreads();
        near_consume(sh, sorted);
        __syncthreads();
        if (wave == 0 && sh.box[lane].want && sh.key[lane] != kNoKey) {
            // final when every target within the distance found lies in a cell that was walked
            const float4 q = sh.q[lane];
            const NearBox w = sh.box[lane];
            const NearBox n = near_ball_box(grid, true, q.x, q.y, q.z, key_dist(sh.key[lane]));
            const bool done = n.want && n.xl >= w.xl && n.xh <= w.xh && n.yl >= w.yl && n.yh <= w.yh && n.zl >= w.zl && n.zh <= w.zh;
            sh.flag[lane] = done && w.want == 1 ? 3 : 2;
        }
    }
    if (wave != 0) return;
    const int j = g * 64 + lane;
    const float4 me = sh.q[lane];
    const int flag = sh.flag[lane];
    if (j < n2) best_key[j] = sh.key[lane];
    const unsigned long long resolved = __ballot((flag & 1) != 0);
    if (lane == 0) {
        GroupInfo gi = {{0, 0, 0, 0, 0, 0}, -1.0f, 0, resolved};   // the rest is nn_cull_kernel<false>'s to fill
        groups[g] = gi;
    }
    emit_seed_blocks(gp, boxes, supers, wk, bank, g, lane, me.w >= 0.0f && !(flag & 2), me.x, me.y, me.z);
}

// One workgroup of 64 x kTeam threads per query group.
// Phase A, wave 0 with lane = query: (APPLY) move the query by the previous iteration's (T, Rn) -- icp.cpp:143-146 + :165:
// v = (v + T) * Rn, row vectors, f32, one rounding per operation -- in the sorted working copy and in the caller's array (same
// three floats at the query's original position); the query's seed (its previous neighbour's distance from where the query is
// now; without seed_targets the key the probe / the seed round left) and the cells its ball touches.  All threads (APPLY): clear
// the match keys for this iteration's claims.  The team phases: the near path (seeded form; after a probe its verdicts are
// taken from groups[g].resolved instead).  Phase B, every wave with lane = query: the box and the largest bound of the queries
// that still search, and one (group, super-block) item per super-block they may need -- the waves share out the chunks of
// super-blocks.
template <bool APPLY>
__global__ __launch_bounds__(kCullThreads) __attribute__((amdgpu_waves_per_eu(7, 8))) void nn_cull_kernel(float4 *src, float *verts2, int n2, const IcpState *st, unsigned long long *keys,
                                                               int n_keys, const GridParams *__restrict__ gp, const Box *__restrict__ supers,
                                                               const float *__restrict__ seed_targets, int n1, const int *idx,
                                                               unsigned long long *best_key, GroupInfo *groups, NnWork wk, int bank,
                                                               const int *__restrict__ cell_start, const float4 *__restrict__ sorted, int near_arg)
{
    __shared__ NearShared sh;
    // near_arg: 0 = no near path; n > 0 = candidate cap n, seeded steps when the previous step said so (st->near_next); n < 0 = cap -n, always
    const int near_pts = near_arg < 0 ? -near_arg : (!APPLY || st->near_next ? near_arg : 0);
    if (APPLY)
        for (int k = blockIdx.x * kCullThreads + threadIdx.x; k < n_keys; k += gridDim.x * kCullThreads) keys[k] = ~0ull;
    const int g = blockIdx.x;
    if (g * 64 >= n2) return;  // workgroup-uniform
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const GridParams grid = *gp;
    if (wave == 0) {
        const int j = g * 64 + lane;
        const bool active = j < n2;
        float4 q4 = make_float4(NAN, NAN, NAN, 0.0f);
        if (active) q4 = src[j];
        const int orig = __float_as_int(q4.w);
        if (APPLY && active && st->mk > 0) {
            const float x = q4.x + st->T[0], y = q4.y + st->T[1], z = q4.z + st->T[2];
            rows_times(x, y, z, st->Rn, q4.x, q4.y, q4.z);
            src[j] = q4;
            const size_t o = 3 * (size_t)orig;
            verts2[o] = q4.x;
            verts2[o + 1] = q4.y;
            verts2[o + 2] = q4.z;
        }
        const float qx = q4.x, qy = q4.y, qz = q4.z;
        const bool part = active && finite3(qx, qy, qz);
        unsigned long long key = kNoKey;
        bool settled = false;   // by the probe
        if (seed_targets) {
            if (part) {
                const int k = idx[j];   // the sorted-order copy of the previous neighbours (nn_finish_kernel): loaded together with src[j]
                if ((unsigned int)k < (unsigned int)n1) {
                    const float d = dist2(qx, qy, qz, seed_targets[3 * (size_t)k], seed_targets[3 * (size_t)k + 1], seed_targets[3 * (size_t)k + 2]);
                    if (d == d) key = pack_key(d, k);  // not NaN
                }
            }
        } else {
            if (active) key = best_key[j];
            settled = near_pts > 0 && ((groups[g].resolved >> lane) & 1);
        }
        const float B = key_dist(key);
        sh.q[lane] = make_float4(qx, qy, qz, part && !settled ? B : -1.0f);
        sh.key[lane] = key;
        sh.box[lane] = near_ball_box(grid, seed_targets && near_pts > 0 && part && B < INFINITY, qx, qy, qz, B);
        sh.flag[lane] = settled;
        if (lane == 0) sh.n_chunks = 0;
    }
    __syncthreads();
    if (seed_targets && near_pts > 0) {
        near_enqueue<false>(sh, grid, cell_start, near_pts, threadIdx.x / kTeam, threadIdx.x % kTeam);
        __syncthreads();
        near_consume(sh, sorted);
        __syncthreads();
        if (wave == 0 && sh.box[lane].want) {   // the walk covered the ball of the bound: the key is final
            sh.q[lane].w = -1.0f;
            sh.flag[lane] = 1;
        }
        __syncthreads();
    }
    const float4 me = sh.q[lane];
    if (wave == 0 && seed_targets && g * 64 + lane < n2) best_key[g * 64 + lane] = sh.key[lane];
    const bool search = me.w >= 0.0f;   // (a bound is a squared distance or +inf)
    const GroupInfo gi = {wave_query_box(search, me.x, me.y, me.z), wave_max(me.w), 0, __ballot(sh.flag[lane] != 0)};
    if (threadIdx.x == 0) groups[g] = gi;
    if (!(gi.rmax >= 0.0f)) return;
    const int n_supers = grid.ncells / 4096;
    int *cnt = wk.counters + kBankInts * bank;
    // two passes over the wave's super-block boxes (count, then write) so that the append costs the wave ONE atomicAdd; the boxes of
    // four chunks (256 super-blocks) are loaded at once: one memory round trip per four chunks instead of one per chunk
    auto chunk_dist = [&](int c0, float (&m)[4]) {
        float4 lo[4];   // lx, ly, lz, hx
        float2 hi[4];   // hy, hz (the two spare words of a super-block's box stay where they are)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int sl = c0 + 64 * k + lane;
            if (sl < n_supers) {
                lo[k] = *reinterpret_cast<const float4 *>(&supers[sl].lx);
                hi[k] = *reinterpret_cast<const float2 *>(&supers[sl].hy);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int sl = c0 + 64 * k + lane;
            const Box b = {lo[k].x, lo[k].y, lo[k].z, lo[k].w, hi[k].x, hi[k].y, 0.0f, 0.0f};
            m[k] = sl < n_supers ? boxbox_min_dist2(gi.w, b) : INFINITY;
        }
    };
    int total = 0;
    for (int c0 = 256 * wave; c0 < n_supers; c0 += 256 * kTeam) {
        float m[4];
        chunk_dist(c0, m);
#pragma unroll
        for (int k = 0; k < 4; k++) total += __popcll(__ballot(m[k] <= gi.rmax && m[k] < INFINITY));
    }
    if (total == 0) return;
    const int seg = (g + wave) & (kSegs - 1);
    int base = 0;
    if (lane == 0) base = atomicAdd(cnt + seg * kSegStride + kCntA, total);
    base = __shfl(base, 0, 64);
    if (base + total > wk.seg_a) {
        if (lane == 0) atomicExch(cnt + kOverflow, 1);
        return;
    }
    uint2 *out = wk.list_a + (size_t)seg * wk.seg_a + base;
    for (int c0 = 256 * wave; c0 < n_supers; c0 += 256 * kTeam) {
        float m[4];
        chunk_dist(c0, m);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool open = m[k] <= gi.rmax && m[k] < INFINITY;
            const unsigned long long mask = __ballot(open);
            if (open) out[__popcll(mask & ((1ull << lane) - 1))] = make_uint2((unsigned int)g, (unsigned int)(c0 + 64 * k + lane));
            out += __popcll(mask);
        }
    }
}

// One wave per (group, super-block) item: the super-block's 64 blocks, one per lane, against the group's box, then each
// surviving block against every query's own bound; what is left becomes scan items.
__global__ __launch_bounds__(64) void nn_blocks_kernel(const float4 *__restrict__ src, int n2, const Box *__restrict__ boxes,
                                                             const unsigned long long *__restrict__ best_key,
                                                             const GroupInfo *__restrict__ groups, NnWork wk, int bank)
{
    const int lane = threadIdx.x & 63;
    int *cnt = wk.counters + kBankInts * bank;
    if (cnt[kOverflow]) return;  // a list overflowed: the finish kernel searches from scratch
    for_each_item(wk.list_a, wk.seg_a, cnt, kCntA, [&](uint2 item) {
        const int g = (int)item.x, s = (int)item.y;
        const int j = g * 64 + lane;
        const Box bb = boxes[s * 64 + lane];
        const GroupInfo gi = groups[g];
        float4 q4 = make_float4(NAN, NAN, NAN, 0.0f);
        float bound = -1.0f;
        if (j < n2) {
            q4 = src[j];
            if (finite3(q4.x, q4.y, q4.z) && !((gi.resolved >> lane) & 1)) bound = key_dist(best_key[j]);
        }
        const float mb = boxbox_min_dist2(gi.w, bb);
        unsigned long long cand = __ballot(mb <= gi.rmax && mb < INFINITY);
        unsigned long long take = 0;
        while (cand) {
            const int b = __ffsll((long long)cand) - 1;
            cand &= cand - 1;
            if (__ballot(box_min_dist2(q4.x, q4.y, q4.z, lane_box(bb, b)) <= bound)) take |= 1ull << b;  // some query may find something nearer or tied in it
        }
        emit_ranges(wk, cnt, kCntB, g, g + s, (take >> lane) & 1, __float_as_int(bb.pad0), __float_as_int(bb.pad1), lane);
    });
}

// One wave per (group, point range) item: the group's 64 queries against the range's points; a query whose (distance,
// index) pair improved merges it into its key -- atomicMin on (distance bits << 32 | index) is the lexicographic minimum.
__global__ __launch_bounds__(64) void nn_scan_kernel(const float4 *__restrict__ src, int n2, const float4 *__restrict__ sorted,
                                                           unsigned long long *best_key, NnWork wk, int bank, int which)
{
    __shared__ WaveStage st;
    const int lane = threadIdx.x;
    const int *cnt = wk.counters + kBankInts * bank;
    if (cnt[kOverflow]) return;
    for_each_item(wk.list_b, wk.seg_b, cnt, which, [&](int4 item) {
        const int j = item.x * 64 + lane;
        float4 q4 = make_float4(NAN, NAN, NAN, 0.0f);
        unsigned long long key = kNoKey;
        if (j < n2) {
            q4 = src[j];
            key = best_key[j];
        }
        float best = key_dist(key);
        int best_i = key_index(key);
        scan_points(sorted, item.y, item.z, st, lane, q4.x, q4.y, q4.z, best, best_i);
        const unsigned long long now = pack_key(best, best_i);
        if (j < n2 && now < key) atomicMin(&best_key[j], now);
    });
}

// How both searches end, one thread per query (every thread of the workgroup must get here): the neighbour index and squared distance at the
// query's ORIGINAL position `orig`, the index once more at its sorted position j when idx_sorted is given, and the claim when keys is.
__device__ __forceinline__ void finish_query(bool active, int j, int orig, float best, int best_i, int *idx, float *dist, int *idx_sorted,
                                             unsigned long long *keys, int *slot_k, unsigned long long *slot_v)
{
    if (active) {
        if (best_i == kNoIndex) best_i = 0;  // nothing comparable (NaN everywhere): keep the index in range
        idx[orig] = best_i;
        dist[orig] = best;
        if (idx_sorted) idx_sorted[j] = best_i;   // the next iteration's seeds, where nn_cull_kernel reads them with the queries
    }
    if (keys) claim_targets(keys, active, best_i, best, orig, slot_k, slot_v);
}

// One thread per query: finish_query.  When an item list overflowed, every group first runs the complete walk (seeded with whatever its keys hold).
__global__ __launch_bounds__(kThreads) void nn_finish_kernel(const float4 *__restrict__ src, int n2, const GridParams *__restrict__ gp,
                                                             const float4 *__restrict__ sorted, const Box *__restrict__ boxes,
                                                             const Box *__restrict__ supers, const unsigned long long *best_key, int *idx,
                                                             float *dist, int *idx_sorted, unsigned long long *keys, NnWork wk, int bank)
{
    __shared__ WaveStage s_stage[kThreads / 64];
    __shared__ int s_claim_k[kClaimSlots];
    __shared__ unsigned long long s_claim_v[kClaimSlots];
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * kThreads + threadIdx.x;
    int *cnt = wk.counters + kBankInts * bank;
    const bool overflow = cnt[kOverflow] != 0;
    // the other bank served the previous step and is read by nobody any more: clear it for the next step
    if (blockIdx.x == 0)
        for (int t = threadIdx.x; t < kBankInts; t += kThreads) wk.counters[kBankInts * (1 - bank) + t] = 0;
    const bool active = j < n2;
    float4 q4 = make_float4(NAN, NAN, NAN, 0.0f);
    unsigned long long key = kNoKey;
    if (active) {
        q4 = src[j];
        key = best_key[j];
    }
    float best = key_dist(key);
    int best_i = key_index(key);
    if (overflow) wave_search(gp, sorted, boxes, supers, s_stage[threadIdx.x >> 6], lane, q4.x, q4.y, q4.z, active && finite3(q4.x, q4.y, q4.z), best, best_i);
    finish_query(active, j, __float_as_int(q4.w), best, best_i, idx, dist, idx_sorted, keys, s_claim_k, s_claim_v);
}

// Brute force (nn_mode 0, the ablation leg).  A lane owns one query; the targets of a step are wave-uniform, so they are fetched
// with scalar loads (s_load_dwordx16 + x8 = 8 points of the AoS cloud as it stands) and enter the VALU ops as SGPR operands:
// no tile loads, no barriers, no LDS traffic in the loop.  Targets are visited in index order and a lane is only updated on
// a strictly smaller distance, so the lowest index wins ties inside a slice; the launch cuts the target cloud into slices
// (grid.y) whose (distance, index) keys are combined with a 64-bit atomicMin (lexicographic: smaller distance, then lower
// index) and nn_brute_finish_kernel writes the results.
// Measured on the way (configs[1], 1.2e10 pairs): LDS-tiled with broadcast ds_read_b128 and packed f32, one workgroup per 256
// queries over all targets 2.79 ms (435 workgroups = 1.7 waves per SIMD, the kernel lasting as long as its busiest CU);
// the same in 5 slices with the next step's LDS reads prefetched 2.40; scalar loads 2.13; ~75 slices (32 k workgroups of
// ~1500 points) 1.77 ms = 54 TFLOP/s.  Ceiling (tools/pk_rate.hip): packed or not, dependent f32 add / mul chains retire at
// 60-61 TFLOP/s chip-wide -- without FMA (contraction is off by contract) half of the nominal 157 is out of reach.
__global__ __launch_bounds__(kThreads) void nn_brute_kernel(const float *__restrict__ targets, int n1, const float4 *__restrict__ src, int n2,
                                                            int slice_points /* a multiple of 8 */, unsigned long long *best_key)
{
    const int j = blockIdx.x * kThreads + threadIdx.x;
    const float4 q4 = j < n2 ? src[j] : make_float4(NAN, NAN, NAN, 0.0f);
    const float qx = q4.x, qy = q4.y, qz = q4.z;
    float best = INFINITY;
    int best_i = kNoIndex;
    const int first = (int)min((long long)n1, (long long)blockIdx.y * slice_points);
    const int last = (int)min((long long)n1, (long long)first + slice_points);
    const int full = first + ((last - first) & ~7);   // whole steps of 8 points
    const float *__restrict__ tp = targets + 3 * (size_t)first;
    // two register (SGPR) buffers used alternately, so the prefetched step needs no copy
    float bufA[24], bufB[24];
    const int last_step = max(full - 8, first);
    auto fetch = [&](float (&buf)[24], int t) {   // unconditional (a prefetch past the end re-reads the last step): no wait lands behind the loads
        const float *__restrict__ p = tp + 3 * (min(t, last_step) - first);
#pragma unroll
        for (int c = 0; c < 24; c++) buf[c] = p[c];
    };
    auto step = [&](const float (&buf)[24], int t) {
        float d[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {   // the order (dx*dx + dy*dy) + dz*dz of PointCloud::kdtree_distance (icp.h:40-47); contraction is off
            const float dx = qx - buf[3 * k], dy = qy - buf[3 * k + 1], dz = qz - buf[3 * k + 2];
            d[k] = dx * dx + dy * dy + dz * dz;
        }
        const float m = fminf(fminf(fminf(d[0], d[1]), fminf(d[2], d[3])), fminf(fminf(d[4], d[5]), fminf(d[6], d[7])));   // fminf skips NaN
        if (__ballot(m < best)) {   // wave-uniform; rare once the running minima have settled
#pragma unroll
            for (int k = 0; k < 8; k++)
                if (d[k] < best) { best = d[k]; best_i = t + k; }
        }
    };
    if (first < full) fetch(bufA, first);
    for (int t = first; t < full; t += 16) {
        // scalar loads return out of order, so the only wait is "all of them": a buffer's first use must come BEFORE the next
        // fetch is issued, or that wait would cover the fresh loads too (the empty asm pins that order)
        fetch(bufB, t + 8);
        step(bufA, t);
        asm volatile("" ::"s"(bufB[0]));
        fetch(bufA, t + 16);
        if (t + 8 < full) step(bufB, t + 8);
        asm volatile("" ::"s"(bufA[0]));
    }
    for (int t = full; t < last; t++) {   // the cloud's last < 8 points
        const float dx = qx - targets[3 * (size_t)t], dy = qy - targets[3 * (size_t)t + 1], dz = qz - targets[3 * (size_t)t + 2];
        const float d = dx * dx + dy * dy + dz * dz;
        if (d < best) { best = d; best_i = t; }
    }
    if (j < n2 && best_i != kNoIndex) atomicMin(&best_key[j], pack_key(best, best_i));
}

__global__ __launch_bounds__(kThreads) void nn_brute_init_kernel(unsigned long long *best_key, int n2)
{
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j < n2) best_key[j] = kNoKey;
}

// after a sliced brute-force search: results to the queries' original positions + the one-to-one claims
__global__ __launch_bounds__(kThreads) void nn_brute_finish_kernel(const float4 *__restrict__ src, int n2, const unsigned long long *best_key, int *idx,
                                                                   float *dist, unsigned long long *keys)
{
    __shared__ int s_claim_k[kClaimSlots];
    __shared__ unsigned long long s_claim_v[kClaimSlots];
    const int j = blockIdx.x * kThreads + threadIdx.x;
    const bool active = j < n2;
    const unsigned long long key = active ? best_key[j] : kNoKey;
    finish_query(active, j, active ? __float_as_int(src[j].w) : 0, key_dist(key), key_index(key), idx, dist, nullptr, keys, s_claim_k, s_claim_v);
}

}  // namespace

constexpr int kItemPoints = 128;   // points per scan item (NnWork::item_points).  128 instead of 256: 0.094 -> 0.089 ms/iteration (configs[1])

// $LSN_ICP_DEBUG, a development aid behind run_nn's grid step: synchronises and prints the work-list sizes and the grid.
static void debug_report(LsnIcp *w, int n1, int n2, int n_groups, bool seeded, int bank, hipStream_t s)
{
    int c[2 * kBankInts];
    GridParams g;
    (void)hipStreamSynchronize(s);
    (void)hipMemcpy(c, w->counters.p, sizeof(c), hipMemcpyDeviceToHost);   // (the other bank has been cleared by now)
    (void)hipMemcpy(&g, w->tgt.gp.p, sizeof(g), hipMemcpyDeviceToHost);
    const int *b = c + kBankInts * bank;
    long long na = 0, nb = 0, ns = 0;
    int ma = 0, mb = 0;
    for (int k = 0; k < kSegs; k++) {
        const int *c3 = b + k * kSegStride;
        na += c3[kCntA]; nb += c3[kCntB]; ns += c3[kCntSeed];
        ma = c3[kCntA] > ma ? c3[kCntA] : ma;
        mb = c3[kCntB] > mb ? c3[kCntB] : mb;
        mb = c3[kCntSeed] > mb ? c3[kCntSeed] : mb;
    }
    fprintf(stderr, "[lsn icp] n1=%d n2=%d groups=%d seeded=%d h=%g grid=%dx%dx%d supers=%d; items: super-blocks %lld (fullest segment %d of %d), ranges %lld + seed ranges %lld (fullest segment %d of %d), overflow %d\n",
            n1, n2, n_groups, (int)seeded, (double)g.h, g.nx, g.ny, g.nz, g.ncells / 4096, na, ma, w->seg_a, nb, ns, mb, w->seg_b, b[kOverflow]);
}

// One NN step over the sorted working copy of the source (w->src.sorted, n2 queries); results land at the queries'
// ORIGINAL positions in d_idx / d_dist.  seeded: d_idx holds every query's previous neighbour (ICP iterations > 0); the
// first launch then also applies the previous iteration's motion (st) to the source and clears `keys`.
// `bank` alternates between consecutive steps on a stream (the counters of the other bank are cleared meanwhile).
static int run_nn(LsnIcp *w, const float *d_verts1, int n1, float *d_verts2, int n2, int *d_idx, float *d_dist, unsigned long long *keys,
                  int nn_mode, hipStream_t s, bool seeded, const IcpState *st, int bank)
{
    float4 *src = w->src.sorted.as<float4>();
    if (nn_mode == 0) {
        // slices of the target cloud: ~32 k workgroups of a few hundred to a few thousand points each (measured best at configs[1]
        // and [2]: 2 k workgroups 2.13 ms, 8 k 1.80, 16-32 k 1.77, 64 k 1.83)
        constexpr int kBruteWorkgroups = 32768;
        const int qblocks = blocks_for(n2);
        int slices = std::max(1, std::min(65535, (kBruteWorkgroups + qblocks - 1) / qblocks));
        const int slice_points = std::max(64, (((n1 + slices - 1) / slices) + 7) & ~7);
        slices = std::max(1, (n1 + slice_points - 1) / slice_points);
        unsigned long long *best_key = w->best_key.as<unsigned long long>();
        hipLaunchKernelGGL(nn_brute_init_kernel, dim3(qblocks), dim3(kThreads), 0, s, best_key, n2);
        hipLaunchKernelGGL(nn_brute_kernel, dim3(qblocks, slices), dim3(kThreads), 0, s, d_verts1, n1, (const float4 *)src, n2, slice_points, best_key);
        hipLaunchKernelGGL(nn_brute_finish_kernel, dim3(qblocks), dim3(kThreads), 0, s, (const float4 *)src, n2,
                           (const unsigned long long *)best_key, d_idx, d_dist, keys);
        LSN_HIP(hipGetLastError());
        return 0;
    }
    const GridParams *gp = w->tgt.gp.as<GridParams>();
    const float4 *sorted = w->tgt.sorted.as<float4>();
    const Box *boxes = w->tgt.boxes.as<Box>(), *supers = w->tgt.supers.as<Box>();
    const int *cell_start = w->tgt.cell_start.as<int>();
    unsigned long long *best_key = w->best_key.as<unsigned long long>();
    GroupInfo *groups = w->groups.as<GroupInfo>();
    const NnWork wk = {w->list_a.as<uint2>(), w->list_b.as<int4>(), w->seg_a, w->seg_b, kItemPoints, w->counters.as<int>()};
    const int n_groups = (n2 + 63) / 64;
    w->last_groups = n_groups;
    // the near path's argument: the candidate cap, negated for the seeded cull when the path is forced (nn_cull_kernel's near_arg)
    const int near_pts = w->near_mode == 0 ? 0 : w->near_pts;
    // consumer launches (one wave per workgroup, a multiple of 64 of them): a seeded group needs ~3-5 super-blocks and ~5-8
    // point ranges; longer lists are served by looping.  Waves without an item leave after one load.
    // waves per query group of the two list consumers.  The scan list of a seeded step holds ~6 (configs[1]) to ~11 (configs[2]) items
    // per group, unevenly over the 64 segments: with fewer waves than the fullest segment has items, some waves serve a second item
    // behind their first -- a second chain of dependent round trips that sets the launch time (A/B in EXPERIMENTS.md, profiles/r04_ab_icp.txt)
    constexpr int scan_waves = 12, block_waves = 8;
    const dim3 blocks_grid(64 * ((block_waves * n_groups + 63) / 64)), scan_grid(64 * ((scan_waves * n_groups + 63) / 64));
    if (seeded) {
        hipLaunchKernelGGL(nn_cull_kernel<true>, dim3(n_groups), dim3(kCullThreads), 0, s, src, d_verts2, n2, st, keys, n1, gp, supers, d_verts1, n1,
                           (const int *)w->idx_sorted.as<int>(), best_key, groups, wk, bank, cell_start, sorted,
                           w->near_mode == 2 ? -near_pts : near_pts);
    } else {
        hipLaunchKernelGGL(nn_probe_kernel, dim3(n_groups), dim3(kCullThreads), 0, s, (const float4 *)src, n2, gp, boxes, supers, best_key, groups, wk, bank,
                           cell_start, sorted, near_pts);
        hipLaunchKernelGGL(nn_scan_kernel, scan_grid, dim3(64), 0, s, (const float4 *)src, n2, sorted, best_key, wk, bank, kCntSeed);
        hipLaunchKernelGGL(nn_cull_kernel<false>, dim3(n_groups), dim3(kCullThreads), 0, s, src, (float *)nullptr, n2, (const IcpState *)nullptr,
                           (unsigned long long *)nullptr, 0, gp, supers, (const float *)nullptr, n1, (const int *)nullptr, best_key, groups, wk, bank,
                           cell_start, sorted, near_pts);
    }
    hipLaunchKernelGGL(nn_blocks_kernel, blocks_grid, dim3(64), 0, s, (const float4 *)src, n2, boxes,
                       (const unsigned long long *)best_key, (const GroupInfo *)groups, wk, bank);
    hipLaunchKernelGGL(nn_scan_kernel, scan_grid, dim3(64), 0, s, (const float4 *)src, n2, sorted, best_key, wk, bank, kCntB);
    hipLaunchKernelGGL(nn_finish_kernel, dim3(blocks_for(n2)), dim3(kThreads), 0, s, (const float4 *)src, n2, gp, sorted, boxes, supers,
                       (const unsigned long long *)best_key, d_idx, d_dist, keys ? w->idx_sorted.as<int>() : (int *)nullptr, keys, wk, bank);
    LSN_HIP(hipGetLastError());
    static const bool debug = getenv("LSN_ICP_DEBUG") != nullptr;
    if (debug) debug_report(w, n1, n2, n_groups, seeded, bank, s);
    return 0;
}
