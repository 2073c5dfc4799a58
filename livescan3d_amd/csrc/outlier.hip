// outlier.hip -- the k-nearest-neighbour outlier filter (the "Filtering" group of LiveScanServer's settings: bFilter, nFilterNeighbors,
// fFilterThreshold): lsnFusionOutlierFilter, lsnFusionOutlierDiagnostics and what the exports run while lsnSetOutlierFilter is on.
//
// Reference: filter() (src/LiveScanClient/filter.cpp:36-81) removes every point whose k-th smallest squared distance to the cloud
// (KNNeighbors, :19-34: nanoflann's kd-tree over the same cloud, the point itself included at distance 0, duplicates counted) exceeds
// distThreshold = pow(maxDist, 2) stored in a float.  "The k-th smallest distance is > thr" is "fewer than k points lie at d^2 <= thr",
// so the device counts neighbours -- no top-k, nothing stored per k -- and stops as soon as it has k:
//     keep i  <=>  #{ j in the block : d^2(i, j) <= thr } >= k
// with d^2 exactly as PointCloud::kdtree_distance evaluates it (include/LiveScanClient/filter.h:38-45: d = query - point,
// d0*d0 + d1*d1 + d2*d2 left to right; the Makefile's -ffp-contract=off keeps it free of FMAs, like the reference's /fp:precise build).
// A block of fewer than k points never overwrites KNNResultSet::init's FLT_MAX: it is kept iff thr >= FLT_MAX.  k <= 0 and maxDist <= 0
// change nothing (:40-41), and neither does a NaN maxDist (it passes that test, and kDistance > NaN is false for every point).
//
// Scope (DESIGN.md sections 2 and 11): every sensor's block of every tick on its own -- the cloud generateVerticesFromDepthMap returns
// for that sensor; a removed vertex becomes depth 0 at its pixel, and the caller fuses the masked maps again.  Stages, each ONE launch over
// all ticks and sensors of the plan:
//   1. index pass (the plan's cloud index without the confidence maps, cloud_index.hip): the pixel of every vertex.
//   2. grid (ol_box_kernel, ol_frame_kernel, ol_key_kernel, ol_chunk_kernel<0>, ct_block_scan_kernel, ol_chunk_kernel<1>,
//      ol_scatter_kernel): the bounding box of every (tick, sensor) block; every vertex's cell of a uniform grid anchored at the box's
//      corner whose edge is at least maxDist and at least 2^-20 of the box's extent (ol_cell below), hashed into its sensor's table of
//      2^m >= pixels buckets; counts per bucket, an exclusive scan over the tick's buckets, the points scattered into their buckets (the
//      scan's starts become the ends).  The table is per sensor, so no point ever meets another sensor's; its size depends on the frame,
//      not on the radius or the crop box, so a 1 mm radius in a 10 m box allocates what a 10 cm one does; the edge's floor keeps every
//      axis below 2^20 + 1 cells, so no radius, however small, piles a block into a few cells.  A bucket that holds points of several
//      cells only costs time: every candidate is tested with the exact distance.  Consecutive vertices of a wave that share a bucket
//      (neighbouring pixels of one surface) share one atomic.  A vertex that is not finite (outside the contract)
//      takes a bucket by its index and is removed without a walk.
//   3. count (ol_count_kernel): every vertex walks the buckets of the 27 cells around its own (its own cell first, each bucket once) and
//      stops at k.  Duplicates or a radius larger than the cloud do not make this quadratic: every candidate then counts, and the walk
//      stops after k of them.
//   4. mask (ol_mask_kernel): depth 0 at the pixels of removed vertices, in d_depth_out (a copy of the input maps unless in place).
// Compiled as part of mesh.hip's translation unit (after cloud_index.hip, whose cloud index, sensor_of and block scan it uses).
#include "fusion_shared.hpp"

#include <cfloat>
#include <cmath>

namespace {

constexpr int kOlThreads = 256;
constexpr int kOlChunk = kOlThreads * 8;   // buckets per workgroup of the bucket scan
constexpr int kOlMinBuckets = 64;

struct OlArgs {
    const FrameDesc *frames;
    const int *offsets;        // [n_ticks][n+1]: the caller's table
    const uint4 *verts;        // [n_ticks][tick_vert]: the caller's clouds
    const int *v2pix;          // [n_ticks][tick_vert]: the index pass's vertex -> pixel (inside the sensor's frame)
    const int *bbase;          // [n]: first bucket of each sensor inside a tick's table ...
    const int *bmask;          // [n]: ... and its bucket count - 1 (a power of two - 1)
    int *key;                  // [n_ticks][tick_vert]: each vertex's bucket
    int *bucket;               // [n_ticks][nb]: counts, then exclusive starts, then (after the scatter) ends
    int *chunk;                // [n_ticks][nchunk]: bucket sums per kOlChunk, then their exclusive prefixes
    float4 *pts;               // [n_ticks][tick_vert]: the tick's points bucket after bucket
    unsigned char *removed;    // [n_ticks][tick_vert]
    int *stats;                // [n_ticks][2][n]: removed vertices, vertices the grid pass decided
    unsigned short *depth_out; // [n_ticks][tick_pix]
    long long tick_pix, tick_vert;
    int n, nb, nchunk, k;
    float thr;                 // distThreshold
    int keep_small;            // a block of fewer than k points is kept (thr >= FLT_MAX)
    double edge;               // maxDist (1 + 2^-20) + 2^-70: the smallest cell edge (ol_cell)
    int *box;                  // [n_ticks][n][6]: min x, y, z, max x, y, z of the finite vertices, as order-preserving ints
    double4 *frame;            // [n_ticks][n]: the grid's corner x, y, z and 1 / its edge
};

// a finite float as an int whose signed order is the float order (atomicMin / atomicMax on the bounding box), and back
__device__ __forceinline__ int ol_ord(float f)
{
    const int i = __float_as_int(f);
    return i >= 0 ? i : i ^ 0x7FFFFFFF;
}
__device__ __forceinline__ float ol_unord(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7FFFFFFF); }

__device__ __forceinline__ bool ol_finite(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// The cell of a coordinate along one axis: floor((x - corner) / e) with the block's bounding-box corner and an edge e >= e0 =
// maxDist (1 + 2^-20) + 2^-70 (ol_frame_kernel: e = max(e0, 2^-20 x the box's largest side)); every pair the count can accept lies in
// cells at most one apart on every axis.  Proof for e = e0 (a larger edge only brings cells closer): let u = 2^-24 and eta = 2^-150
// (half the smallest subnormal float).  A pair
// passes when fl(fl(fl(d0^2) + fl(d1^2)) + fl(d2^2)) <= thr with every fl(di^2) >= 0; rounding is monotone, so fl(d0^2) <= the sum <= thr
// (likewise d1, d2).  fl(x) >= x (1 - u) - eta gives d0^2 <= (thr + eta) / (1 - u), and thr = fl(maxDist^2) <= maxDist^2 (1 + u) + eta.
// d0 = fl(q0 - p0) with |q0 - p0| <= |d0| / (1 - u) (a float difference that is subnormal is exact).  Together |q0 - p0| <=
// sqrt((maxDist^2 (1 + u) + 2 eta) / (1 - u)^3) <= maxDist (1 + 2.1 u) + 2^-74.4 < e (1 - 2^-21).  The coordinate in cells,
// (x - corner) / e, is formed in double: the difference of two floats carries a relative error of at most 2^-53, and a finite vertex lies
// in its block's box, so the product lies in [0, 2^20 + 1] with an error of at most 2^-31; two coordinates whose exact images are
// < 1 - 2^-21 apart stay < 1 apart, and floor() puts them at most one cell apart.  The clamp to +-2^30 (a 1-Lipschitz map: pairs only get
// closer) only keeps the int conversion defined.  maxDist = +inf gives e = inf, 1 / e = 0: one cell holds the block.
__device__ __forceinline__ int ol_cell(float x, double corner, double inv_edge)
{
    return (int)floor(fmin(fmax(((double)x - corner) * inv_edge, -1073741824.0), 1073741824.0));
}

__device__ __forceinline__ unsigned int ol_hash(int cx, int cy, int cz)
{
    unsigned int h = ((unsigned int)cx * 73856093u) ^ ((unsigned int)cy * 19349663u) ^ ((unsigned int)cz * 83492791u);
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    return h;
}

__device__ __forceinline__ int ol_bucket(const OlArgs &a, int s, int cx, int cy, int cz)
{
    return a.bbase[s] + (int)(ol_hash(cx, cy, cz) & (unsigned int)a.bmask[s]);
}

// ---- 2. grid -----------------------------------------------------------------------------------------------------------------------
// Runs of equal keys among consecutive live lanes of a wave: whether this lane continues the run of the lane below it (cont), the lanes
// that do (m), the run's length when this lane leads it, and the leader of this lane's run.
__device__ __forceinline__ void ol_runs(bool live, int key, bool &cont, unsigned long long &m, int &len, int &leader)
{
    const int lane = threadIdx.x & 63;
    const int below = __shfl_up(key, 1, 64);
    cont = live && lane > 0 && below == key;   // a lane that is not live carries key -1, which no live key equals
    m = __ballot(cont);
    const unsigned long long above = lane == 63 ? 0ull : (~m) >> (lane + 1);
    len = 1 + (above == 0 ? 63 - lane : __builtin_ctzll(above));
    const unsigned long long heads = ~m & (lane == 63 ? ~0ull : ((2ull << lane) - 1));
    leader = 63 - __clzll(heads);
}

__global__ __launch_bounds__(kOlThreads) void ol_box_init_kernel(int *box, int n6)
{
    const int i = blockIdx.x * kOlThreads + threadIdx.x;
    if (i < n6) box[i] = i % 6 < 3 ? 0x7FFFFFFF : (int)0x80000000u;
}

// The bounding box of every (tick, sensor) block's finite vertices: a wave reduces the lanes of its first sensor, the others (sensor
// boundaries) add themselves.
__global__ __launch_bounds__(kOlThreads) void ol_box_kernel(OlArgs a)
{
    const int tick = blockIdx.y, n = a.n;
    const int *off = a.offsets + (long long)tick * (n + 1);
    const int g = blockIdx.x * kOlThreads + threadIdx.x;
    const bool live = g < off[n] && g < a.tick_vert;
    int s = 0;
    float c[3] = {0.0f, 0.0f, 0.0f};
    bool fin = false;
    if (live) {
        s = sensor_of(off, n, g);
        const uint4 v = a.verts[tick * a.tick_vert + g];
        c[0] = __uint_as_float(v.y), c[1] = __uint_as_float(v.z), c[2] = __uint_as_float(v.w);
        fin = ol_finite(c[0], c[1], c[2]);
    }
    const unsigned long long lm = __ballot(live);
    if (lm == 0) return;   // wave-uniform
    const int s0 = __shfl(s, __ffsll((long long)lm) - 1, 64);
    const bool same = fin && s == s0;
    int *bx = a.box + ((long long)tick * n) * 6;
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const int lo = wave_min(same ? ol_ord(c[q]) : 0x7FFFFFFF), hi = wave_max(same ? ol_ord(c[q]) : (int)0x80000000u);
        if ((threadIdx.x & 63) == 0 && lo <= hi) {
            atomicMin(&bx[s0 * 6 + q], lo);
            atomicMax(&bx[s0 * 6 + 3 + q], hi);
        }
        if (fin && !same) {
            atomicMin(&bx[s * 6 + q], ol_ord(c[q]));
            atomicMax(&bx[s * 6 + 3 + q], ol_ord(c[q]));
        }
    }
}

// Every (tick, sensor): the grid's corner and 1 / edge, e = max(e0, 2^-20 x the box's largest side) (ol_cell).
__global__ __launch_bounds__(kOlThreads) void ol_frame_kernel(OlArgs a, int n_blocks)
{
    const int i = blockIdx.x * kOlThreads + threadIdx.x;
    if (i >= n_blocks) return;
    const int *bx = a.box + (long long)i * 6;
    double4 f = make_double4(0.0, 0.0, 0.0, 1.0 / a.edge);
    if (bx[0] <= bx[3]) {   // the block has a finite vertex
        double side = 0.0;
        double lo[3];
#pragma unroll
        for (int q = 0; q < 3; q++) {
            lo[q] = (double)ol_unord(bx[q]);
            side = fmax(side, (double)ol_unord(bx[3 + q]) - lo[q]);
        }
        f = make_double4(lo[0], lo[1], lo[2], 1.0 / fmax(a.edge, side * 0x1p-20));
    }
    a.frame[i] = f;
}

__device__ __forceinline__ int ol_key(const OlArgs &a, int tick, int s, int g, float X, float Y, float Z)
{
    if (!ol_finite(X, Y, Z)) return a.bbase[s] + (int)(ol_hash(g, 0x5bd1e995, tick) & (unsigned int)a.bmask[s]);
    const double4 f = a.frame[(long long)tick * a.n + s];
    return ol_bucket(a, s, ol_cell(X, f.x, f.w), ol_cell(Y, f.y, f.w), ol_cell(Z, f.z, f.w));
}

__global__ __launch_bounds__(kOlThreads) void ol_key_kernel(OlArgs a)
{
    const int tick = blockIdx.y, n = a.n;
    const int *off = a.offsets + (long long)tick * (n + 1);
    const int g = blockIdx.x * kOlThreads + threadIdx.x;
    const bool live = g < off[n] && g < a.tick_vert;
    int b = -1;
    if (live) {
        const uint4 v = a.verts[tick * a.tick_vert + g];
        b = ol_key(a, tick, sensor_of(off, n, g), g, __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
        a.key[tick * a.tick_vert + g] = b;
    }
    bool cont;
    unsigned long long m;
    int len, leader;
    ol_runs(live, b, cont, m, len, leader);
    if (live && !cont) atomicAdd(&a.bucket[(long long)tick * a.nb + b], len);
}

// PASS 0: the sum of every chunk of kOlChunk buckets; PASS 1 (chunk holds exclusive prefixes inside the tick): the buckets' exclusive
// starts inside the tick, in place.
template <int PASS>
__global__ __launch_bounds__(kOlThreads) void ol_chunk_kernel(int *bucket, int *chunk, int nb, int nchunk)
{
    __shared__ int s_wave[kOlThreads / 64];
    const int tick = blockIdx.y, c = blockIdx.x;
    int *b = bucket + (long long)tick * nb;
    const int i0 = c * kOlChunk + (int)threadIdx.x * 8;
    int v[8], t = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const int x = i0 + q < nb ? b[i0 + q] : 0;
        v[q] = t;
        t += x;
    }
    int tot;
    const int incl = block_scan_incl<int, kOlThreads / 64>(t, s_wave, &tot);
    if (PASS == 0) {
        if (threadIdx.x == 0) chunk[(long long)tick * nchunk + c] = tot;
        return;
    }
    const int pre = chunk[(long long)tick * nchunk + c] + incl - t;
#pragma unroll
    for (int q = 0; q < 8; q++)
        if (i0 + q < nb) b[i0 + q] = pre + v[q];
}

__global__ __launch_bounds__(kOlThreads) void ol_scatter_kernel(OlArgs a)
{
    const int tick = blockIdx.y, n = a.n;
    const int *off = a.offsets + (long long)tick * (n + 1);
    const int g = blockIdx.x * kOlThreads + threadIdx.x;
    const bool live = g < off[n] && g < a.tick_vert;
    const int b = live ? a.key[tick * a.tick_vert + g] : -1;
    bool cont;
    unsigned long long m;
    int len, leader;
    ol_runs(live, b, cont, m, len, leader);
    int base = 0;
    if (live && !cont) base = atomicAdd(&a.bucket[(long long)tick * a.nb + b], len);   // the run's slots, in lane order
    base = __shfl(base, leader, 64);
    const int pos = base + ((int)(threadIdx.x & 63) - leader);
    if (live && pos >= 0 && pos < a.tick_vert) {
        const uint4 v = a.verts[tick * a.tick_vert + g];
        a.pts[tick * a.tick_vert + pos] = make_float4(__uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w), 0.0f);
    }
}

// ---- 3. count ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kOlThreads) void ol_count_kernel(OlArgs a)
{
    const int tick = blockIdx.y, n = a.n;
    const int *off = a.offsets + (long long)tick * (n + 1);
    const int g = blockIdx.x * kOlThreads + threadIdx.x;
    const bool live = g < off[n] && g < a.tick_vert;
    int s = 0;
    bool rem = false, grid = false;
    if (live) {
        s = sensor_of(off, n, g);
        if (off[s + 1] - off[s] < a.k) {
            rem = !a.keep_small;   // KNNResultSet::init's FLT_MAX survives
        } else {
            grid = true;
            const uint4 v = a.verts[tick * a.tick_vert + g];
            const float X = __uint_as_float(v.y), Y = __uint_as_float(v.z), Z = __uint_as_float(v.w);
            const double4 f = a.frame[(long long)tick * n + s];
            const int cx = ol_cell(X, f.x, f.w), cy = ol_cell(Y, f.y, f.w), cz = ol_cell(Z, f.z, f.w);
            const int *ends = a.bucket + (long long)tick * a.nb;
            const float4 *pts = a.pts + tick * a.tick_vert;
            const int lim = (int)min((long long)off[n], a.tick_vert);
            int bk[27];
#pragma unroll
            for (int c = 0; c < 27; c++) {
                const int q = c == 0 ? 13 : (c <= 13 ? c - 1 : c);   // the vertex's own cell first: its nearest points are most likely there
                bk[c] = ol_bucket(a, s, cx + q % 3 - 1, cy + (q / 3) % 3 - 1, cz + q / 9 - 1);
            }
            int cnt = ol_finite(X, Y, Z) ? 0 : -0x40000000;   // not finite: removed without a walk (outside the contract)
#pragma unroll
            for (int c = 0; c < 27; c++) {
                bool dup = false;   // two cells whose hashes share a bucket: the bucket is walked once
#pragma unroll
                for (int e = 0; e < c; e++) dup |= bk[e] == bk[c];
                if (dup || cnt >= a.k || cnt < 0) continue;
                const int j0 = max(bk[c] > 0 ? ends[bk[c] - 1] : 0, 0), j1 = min(ends[bk[c]], lim);
                for (int j = j0; j < j1 && cnt < a.k; j++) {
                    const float4 p = pts[j];
                    const float d0 = X - p.x, d1 = Y - p.y, d2 = Z - p.z;
                    const float d = d0 * d0 + d1 * d1 + d2 * d2;   // kdtree_distance, left to right
                    cnt += d <= a.thr ? 1 : 0;
                }
            }
            rem = cnt < a.k;
        }
        a.removed[tick * a.tick_vert + g] = rem ? 1 : 0;
    }
    // per-sensor totals: one atomic per wave for the lanes of the wave's first sensor, one per lane for the others (sensor boundaries)
    const unsigned long long lm = __ballot(live);
    if (lm == 0) return;   // wave-uniform
    const int s0 = __shfl(s, __ffsll((long long)lm) - 1, 64);
    const bool same = live && s == s0;
    const unsigned long long mr = __ballot(same && rem), mg = __ballot(same && grid);
    int *st = a.stats + (long long)tick * 2 * n;
    if ((threadIdx.x & 63) == 0) {
        if (mr) atomicAdd(&st[s0], (int)__popcll(mr));
        if (mg) atomicAdd(&st[n + s0], (int)__popcll(mg));
    }
    if (live && !same) {
        if (rem) atomicAdd(&st[s], 1);
        if (grid) atomicAdd(&st[n + s], 1);
    }
}

// ---- 4. mask -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kOlThreads) void ol_mask_kernel(OlArgs a)
{
    const int tick = blockIdx.y, n = a.n;
    const int *off = a.offsets + (long long)tick * (n + 1);
    const int g = blockIdx.x * kOlThreads + threadIdx.x;
    if (g >= off[n] || g >= a.tick_vert || !a.removed[tick * a.tick_vert + g]) return;
    const FrameDesc f = a.frames[sensor_of(off, n, g)];
    const int pix = a.v2pix[tick * a.tick_vert + g];
    // (pix is in the frame whenever the offsets belong to these depth maps; the test keeps a mismatched call in bounds)
    if ((unsigned int)pix < (unsigned int)f.npix) a.depth_out[tick * a.tick_pix + f.depth_off + pix] = 0;
}

}  // namespace

namespace lsn {

// The four stages on `s` over all ticks of the plan; d_vertices / d_offsets as lsnFusionRun left them from d_depth.  Plan mutex held.
static int outlier_filter_locked(LsnFusion *p, int k, float max_dist, const void *d_depth, const void *d_vertices, const int *d_offsets,
                                 void *d_depth_out, hipStream_t s)
{
    const int n = p->n_maps, T = p->n_ticks;
    LSN_HIP(hipSetDevice(p->device));
    if (!p->ol_ready) {
        // every sensor's bucket table: the power of two >= its pixels (a load factor <= 1)
        std::vector<int> tab(2 * (size_t)n);
        long long nb = 0;
        for (int i = 0; i < n; i++) {
            long long hb = kOlMinBuckets;
            while (hb < (long long)p->w[i] * p->h[i]) hb <<= 1;
            tab[i] = (int)nb;
            tab[n + i] = (int)(hb - 1);
            nb += hb;
            if (nb > 0x7FFFFFFFll) {
                lsn::set_error("lsnFusionOutlierFilter: the bucket tables of one tick exceed 2^31-1 entries");
                return -1;
            }
        }
        const int nchunk = (int)((nb + kOlChunk - 1) / kOlChunk);
        const size_t px = (size_t)p->cap * T;
        if (p->ol_key.reserve(sizeof(int) * px) ||
            p->ol_bucket.reserve(sizeof(int) * (size_t)nb * T) || p->ol_chunk.reserve(sizeof(int) * (size_t)nchunk * T) ||
            p->ol_pts.reserve(sizeof(float4) * px) || p->ol_removed.reserve(px + 1) || p->ol_stats.reserve(sizeof(int) * 2 * (size_t)n * T) ||
            p->ol_offs.reserve(sizeof(int) * (size_t)(n + 1) * T) || p->ol_tab.reserve(sizeof(int) * 2 * (size_t)n) ||
            p->ol_box.reserve(sizeof(int) * 6 * (size_t)n * T) || p->ol_frame.reserve(sizeof(double4) * (size_t)n * T))
            return -1;
        LSN_HIP(hipMemcpy(p->ol_tab.p, tab.data(), sizeof(int) * 2 * (size_t)n, hipMemcpyHostToDevice));
        p->ol_nb = (int)nb;
        p->ol_nchunk = nchunk;
        p->ol_ready = true;
    }
    const size_t depth_bytes = sizeof(unsigned short) * (size_t)p->tick_depth_elems * T;
    if (d_depth_out != d_depth) LSN_HIP(hipMemcpyAsync(d_depth_out, d_depth, depth_bytes, hipMemcpyDeviceToDevice, s));
    // the caller's offsets, for the diagnostics
    LSN_HIP(hipMemcpyAsync(p->ol_offs.p, d_offsets, sizeof(int) * (size_t)(n + 1) * T, hipMemcpyDeviceToDevice, s));
    LSN_HIP(hipMemsetAsync(p->ol_stats.p, 0, sizeof(int) * 2 * (size_t)n * T, s));
    if (!(k > 0 && max_dist > 0.0f)) {   // k <= 0, maxDist <= 0 (filter.cpp:40-41) or NaN (every kDistance > NaN is false): nothing changes
        LSN_HIP(hipMemsetAsync(p->ol_removed.p, 0, (size_t)p->cap * T, s));
        return 0;
    }
    // 1. vertex -> pixel
    if (cloud_index_locked(p, d_depth, const_cast<void *>(d_vertices), false, s)) return -1;
    OlArgs a;
    a.frames = p->frames.as<FrameDesc>();
    a.offsets = d_offsets;
    a.verts = static_cast<const uint4 *>(d_vertices);
    a.v2pix = p->ix_v2pix.as<int>();
    a.bbase = p->ol_tab.as<int>();
    a.bmask = p->ol_tab.as<int>() + n;
    a.key = p->ol_key.as<int>();
    a.bucket = p->ol_bucket.as<int>();
    a.chunk = p->ol_chunk.as<int>();
    a.pts = p->ol_pts.as<float4>();
    a.removed = p->ol_removed.as<unsigned char>();
    a.stats = p->ol_stats.as<int>();
    a.depth_out = static_cast<unsigned short *>(d_depth_out);
    a.tick_pix = p->tick_depth_elems;
    a.tick_vert = p->cap;
    a.n = n;
    a.nb = p->ol_nb;
    a.nchunk = p->ol_nchunk;
    a.k = k;
    a.thr = max_dist * max_dist;   // pow(maxDist, 2) into a float (filter.cpp:53): the double square of a float is exact, so its rounding is this product's
    a.keep_small = a.thr >= FLT_MAX ? 1 : 0;
    a.edge = (double)max_dist * (1.0 + 0x1p-20) + 0x1p-70;   // ol_cell's smallest edge
    a.box = p->ol_box.as<int>();
    a.frame = p->ol_frame.as<double4>();
    const unsigned int vblocks = (unsigned int)((p->cap + kOlThreads - 1) / kOlThreads);
    // 2. grid
    const int n_blocks = n * T;
    hipLaunchKernelGGL(ol_box_init_kernel, dim3((6 * n_blocks + kOlThreads - 1) / kOlThreads), dim3(kOlThreads), 0, s, a.box, 6 * n_blocks);
    hipLaunchKernelGGL(ol_box_kernel, dim3(vblocks, T), dim3(kOlThreads), 0, s, a);
    hipLaunchKernelGGL(ol_frame_kernel, dim3((n_blocks + kOlThreads - 1) / kOlThreads), dim3(kOlThreads), 0, s, a, n_blocks);
    LSN_HIP(hipMemsetAsync(a.bucket, 0, sizeof(int) * (size_t)a.nb * T, s));
    hipLaunchKernelGGL(ol_key_kernel, dim3(vblocks, T), dim3(kOlThreads), 0, s, a);
    hipLaunchKernelGGL(ol_chunk_kernel<0>, dim3(a.nchunk, T), dim3(kOlThreads), 0, s, a.bucket, a.chunk, a.nb, a.nchunk);
    hipLaunchKernelGGL(ct_block_scan_kernel, dim3(T), dim3(1024), 0, s, a.chunk, a.nchunk);
    hipLaunchKernelGGL(ol_chunk_kernel<1>, dim3(a.nchunk, T), dim3(kOlThreads), 0, s, a.bucket, a.chunk, a.nb, a.nchunk);
    hipLaunchKernelGGL(ol_scatter_kernel, dim3(vblocks, T), dim3(kOlThreads), 0, s, a);
    // 3. count, 4. mask
    hipLaunchKernelGGL(ol_count_kernel, dim3(vblocks, T), dim3(kOlThreads), 0, s, a);
    hipLaunchKernelGGL(ol_mask_kernel, dim3(vblocks, T), dim3(kOlThreads), 0, s, a);
    LSN_HIP(hipGetLastError());
    return 0;
}

int outlier_filter(LsnFusion *p, int k, float max_dist, const void *d_depth, const void *d_vertices, const int *d_offsets, void *d_depth_out,
                   hipStream_t s)
{
    if (!p || !d_depth || !d_vertices || !d_offsets || !d_depth_out) {
        lsn::set_error("lsnFusionOutlierFilter: null argument");
        return -1;
    }
    if (!p->params_set) {
        lsn::set_error("lsnFusionOutlierFilter: lsnFusionSetParams has not been called");
        return -1;
    }
    std::lock_guard<std::mutex> g(p->mu);
    return outlier_filter_locked(p, k, max_dist, d_depth, d_vertices, d_offsets, d_depth_out, s);
}

}  // namespace lsn

extern "C" int lsnFusionOutlierFilter(LsnFusion *p, int k, float max_dist, const void *d_depth_maps, const void *d_vertices, const int *d_offsets,
                                      void *d_depth_out, void *stream)
{
    return lsn::guarded("lsnFusionOutlierFilter", -1, [&]() {
        lsn::clear_error();
        return lsn::outlier_filter(p, k, max_dist, d_depth_maps, d_vertices, d_offsets, d_depth_out, lsn::as_stream(stream));
    });
}

extern "C" int lsnFusionOutlierDiagnostics(LsnFusion *p, int tick, int *removed_per_sensor, unsigned char *removed_per_vertex, int *exact_per_sensor,
                                           void *stream)
{
    return lsn::guarded("lsnFusionOutlierDiagnostics", -1, [&]() {
        lsn::clear_error();
        if (!p || tick < 0 || tick >= p->n_ticks) {
            lsn::set_error("lsnFusionOutlierDiagnostics: bad arguments");
            return -1;
        }
        std::lock_guard<std::mutex> g(p->mu);
        if (!p->ol_ready) {
            lsn::set_error("lsnFusionOutlierDiagnostics: no outlier filter has run on this plan");
            return -1;
        }
        LSN_HIP(hipSetDevice(p->device));
        hipStream_t s = lsn::as_stream(stream);
        const int n = p->n_maps;
        std::vector<int> off((size_t)n + 1), st(2 * (size_t)n);
        LSN_HIP(hipMemcpyAsync(off.data(), p->ol_offs.as<int>() + (size_t)tick * (n + 1), sizeof(int) * (n + 1), hipMemcpyDeviceToHost, s));
        LSN_HIP(hipMemcpyAsync(st.data(), p->ol_stats.as<int>() + (size_t)tick * 2 * n, sizeof(int) * 2 * n, hipMemcpyDeviceToHost, s));
        LSN_HIP(hipStreamSynchronize(s));
        const int nv = (int)std::min<long long>(std::max(off[n], 0), p->cap);
        if (removed_per_vertex && nv > 0)
            LSN_HIP(hipMemcpy(removed_per_vertex, p->ol_removed.as<unsigned char>() + (size_t)tick * p->cap, (size_t)nv, hipMemcpyDeviceToHost));
        int total = 0;
        for (int i = 0; i < n; i++) {
            total += st[i];
            if (removed_per_sensor) removed_per_sensor[i] = st[i];
            if (exact_per_sensor) exact_per_sensor[i] = st[n + i];
        }
        return total;
    });
}
