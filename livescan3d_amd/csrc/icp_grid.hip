// icp_grid.hip -- the voxel grid the ICP's exact nearest-neighbour search runs on.  Compiled as part of icp.hip's translation unit (icp.hip
// includes it first); it relies on lsn_common.hpp and wave_ops.hpp only.
//
// A grid is built ONCE per call over the target (which never moves): a counting sort by cell, the cells ordered super-block (16^3 cells) ->
// block (4^3 cells) -> cell so that every block and super-block is one contiguous range of the sorted points, and a tight AABB per block and
// super-block.  The source cloud is sorted the same way once per call (no boxes), so 64 consecutive queries form a compact patch -- what
// icp_nn.hip's query groups are made of.  The build takes one atomic per RUN of equal cells among a wave's lanes (consecutive points are
// raster neighbours), whose return value ranks the run's points: the scatter needs no atomics.  Holds the constants, GridParams, Box and
// QueryBox with their distance functions, the build's kernels, and on the host GridBufs and build_grid.
#include "lsn_common.hpp"
#include "wave_ops.hpp"

#include <algorithm>
#include <array>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;      // partial-sum slots
constexpr int kMaxCells = 1 << 22;    // dense grid capacity (16 MiB of cell starts)
constexpr int kScanItems = 16;        // cells per thread in the scan kernels
constexpr int kScanBlock = kThreads * kScanItems;  // 4096
constexpr int kSuper = 16;            // cells per super-block edge
constexpr int kMaxSupers = kMaxCells / (kSuper * kSuper * kSuper);  // 1024
static_assert(kMaxCells % kScanBlock == 0, "the int4 scans take whole scan blocks");
static_assert(kSuper * kSuper * kSuper == kScanBlock, "a scan block is one super-block's cells: it lies inside the grid or outside it");
constexpr int kMaxBlocks3 = kMaxCells / 64;                          // 4^3-cell blocks

struct GridParams {
    float ox, oy, oz;   // origin (bbox min)
    float h, inv_h;
    int nx, ny, nz;     // cells per axis (multiples of 16)
    int nsx, nsy, nsz;  // super-blocks per axis
    int ncells;         // nx * ny * nz
    int n_points;
};

struct Box {  // tight AABB of a block / super-block; empty: lo = +inf, hi = -inf
    float lx, ly, lz, hx, hy, hz, pad0, pad1;
};

struct QueryBox { float wlx, wly, wlz, whx, why, whz; };  // W: the box of a group's queries that take part in a search; nobody: lo = +inf, hi = -inf

__device__ __forceinline__ int cell_coord(float v, float o, float inv_h, int n)
{
    float f = floorf((v - o) * inv_h);
    int c = (f >= 0.0f) ? ((f < (float)n) ? (int)f : n - 1) : 0;  // NaN -> 0
    return c;
}

// Cell order: super-block (16^3 cells) major, then block (4^3 cells), then cell -- every block / super-block is a
// contiguous range of cell indices, hence of the cell-sorted point array.
__device__ __forceinline__ int cell_index(int cx, int cy, int cz, const GridParams &g)
{
    const int s = ((cz >> 4) * g.nsy + (cy >> 4)) * g.nsx + (cx >> 4);
    const int b = ((((cz >> 2) & 3) * 4) + ((cy >> 2) & 3)) * 4 + ((cx >> 2) & 3);
    const int l = (((cz & 3) * 4) + (cy & 3)) * 4 + (cx & 3);
    return (s << 12) | (b << 6) | l;
}

// Exact f32 lower bound of dist2(q, p) over every p inside the box: component-wise |q - p| >= the clamped gap, and
// rounding is monotone, so the same operation order as dist2 keeps the inequality in floating point.
__device__ __forceinline__ float box_min_dist2(float qx, float qy, float qz, const Box &b)
{
    const float dx = fmaxf(0.0f, fmaxf(b.lx - qx, qx - b.hx));
    const float dy = fmaxf(0.0f, fmaxf(b.ly - qy, qy - b.hy));
    const float dz = fmaxf(0.0f, fmaxf(b.lz - qz, qz - b.hz));
    return dx * dx + dy * dy + dz * dz;
}

// Lower bound of dist2(q, p) for EVERY q inside the query box W = [wl, wh] and every p inside b, evaluated with the same
// operations as box_min_dist2: q <= wh gives b.l - wh <= b.l - q exactly, rounding is monotone, so the per-axis gap never
// exceeds the one box_min_dist2 computes for any q of W, and the squares and sums keep the order.  Empty boxes
// (lo = +inf, hi = -inf) come out as +inf.
__device__ __forceinline__ float boxbox_min_dist2(const QueryBox &w, const Box &b)
{
    const float dx = fmaxf(0.0f, fmaxf(b.lx - w.whx, w.wlx - b.hx));
    const float dy = fmaxf(0.0f, fmaxf(b.ly - w.why, w.wly - b.hy));
    const float dz = fmaxf(0.0f, fmaxf(b.lz - w.whz, w.wlz - b.hz));
    return dx * dx + dy * dy + dz * dz;
}

// ---- grid build -----------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void bbox_partial_kernel(const float *pts, int n, float *part /* [blocks][6] */)
{
    __shared__ float lds[4 * 6];
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float v = pts[3 * (size_t)i + c];
            mn[c] = fminf(mn[c], v);  // fminf/fmaxf ignore NaN operands
            mx[c] = fmaxf(mx[c], v);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float a = wave_min(mn[c]), b = wave_max(mx[c]);
        if (lane == 0) {
            lds[wave * 6 + c] = a;
            lds[wave * 6 + 3 + c] = b;
        }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        float v = lds[threadIdx.x];
        for (int w = 1; w < 4; w++) v = threadIdx.x < 3 ? fminf(v, lds[w * 6 + threadIdx.x]) : fmaxf(v, lds[w * 6 + threadIdx.x]);
        part[blockIdx.x * 6 + threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(64) void grid_setup_kernel(const float *part, int n_parts, int n_points, GridParams *gp)
{
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int b = threadIdx.x; b < n_parts; b += 64)
        for (int c = 0; c < 3; c++) {
            mn[c] = fminf(mn[c], part[b * 6 + c]);
            mx[c] = fmaxf(mx[c], part[b * 6 + 3 + c]);
        }
    for (int c = 0; c < 3; c++) {
        mn[c] = wave_min(mn[c]);
        mx[c] = wave_max(mx[c]);
    }
    if (threadIdx.x != 0) return;
    float ext[3];
    for (int c = 0; c < 3; c++) {
        if (!(mn[c] <= mx[c])) { mn[c] = 0; mx[c] = 0; }  // all-NaN axis
        ext[c] = fminf(mx[c] - mn[c], 1e30f);
    }
    float L = fmaxf(ext[0], fmaxf(ext[1], ext[2]));
    if (!(L > 0.0f) || !(L < INFINITY)) L = 1.0f;
    // cell edge ~ twice the point spacing of a surface-like cloud spread over the bbox faces
    float area = ext[0] * ext[1] + ext[1] * ext[2] + ext[0] * ext[2];
    float h = 2.0f * sqrtf(fmaxf(area, 1e-12f) / (float)(n_points > 0 ? n_points : 1));
    h = fminf(fmaxf(h, L / 512.0f), L / 4.0f);
    int nsx = 1, nsy = 1, nsz = 1;
    for (int guard = 0; guard < 2000; guard++) {
        // cells needed per axis, rounded up to whole super-blocks
        nsx = (int)fminf(floorf(ext[0] / h / kSuper) + 1.0f, 4096.0f);
        nsy = (int)fminf(floorf(ext[1] / h / kSuper) + 1.0f, 4096.0f);
        nsz = (int)fminf(floorf(ext[2] / h / kSuper) + 1.0f, 4096.0f);
        if ((long long)nsx * nsy * nsz <= kMaxSupers && (float)(nsx * kSuper) * h > ext[0] * 1.001f &&
            (float)(nsy * kSuper) * h > ext[1] * 1.001f && (float)(nsz * kSuper) * h > ext[2] * 1.001f)
            break;
        h *= 1.26f;
        nsx = nsy = nsz = 1;
    }
    if ((long long)nsx * nsy * nsz > kMaxSupers) nsx = nsy = nsz = 1;
    const int nx = nsx * kSuper, ny = nsy * kSuper, nz = nsz * kSuper;
    gp->ox = mn[0]; gp->oy = mn[1]; gp->oz = mn[2];
    gp->h = h;
    gp->inv_h = 1.0f / h;
    gp->nx = nx; gp->ny = ny; gp->nz = nz;
    gp->nsx = nsx; gp->nsy = nsy; gp->nsz = nsz;
    gp->ncells = nx * ny * nz;
    gp->n_points = n_points;
}

// One point per thread: its cell and its rank inside the cell (the value the cell's counter had: cell_scatter_kernel then needs no
// atomics).  Consecutive points of a cloud are raster neighbours and mostly share a cell, so a run of equal cells among the wave's
// lanes costs ONE atomicAdd (measured on configs[2]'s 738 k targets: an atomic per point 47 us, per run see EXPERIMENTS.md R6-1).
__global__ __launch_bounds__(kThreads) void cell_count_kernel(const float *pts, int n, const GridParams *gp, int *cell_of, int *rank_of,
                                                              int *cell_cnt)
{
    const GridParams g = *gp;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int c = -1 - lane;   // past the end: a run of its own, no atomic
    if (i < n) {
        const int cx = cell_coord(pts[3 * (size_t)i], g.ox, g.inv_h, g.nx);
        const int cy = cell_coord(pts[3 * (size_t)i + 1], g.oy, g.inv_h, g.ny);
        const int cz = cell_coord(pts[3 * (size_t)i + 2], g.oz, g.inv_h, g.nz);
        c = cell_index(cx, cy, cz, g);
    }
    const int prev = __shfl_up(c, 1, 64);
    const unsigned long long starts = __ballot(lane == 0 || c != prev);
    const int first = 63 - __clzll((long long)(starts & (~0ull >> (63 - lane))));                 // the run's first lane (<= lane)
    const unsigned long long later = lane == 63 ? 0ull : starts & (~0ull << (lane + 1));
    const int end = later ? __ffsll((long long)later) - 1 : 64;                                    // one past the run's last lane
    int base = 0;
    if (lane == first && c >= 0) base = atomicAdd(&cell_cnt[c], end - first);
    base = __shfl(base, first, 64);
    if (i < n) {
        cell_of[i] = c;
        rank_of[i] = base + (lane - first);
    }
}

// exclusive scan of cell_cnt[0..ncells) into cell_start[0..ncells], three small kernels over the fixed capacity
// (ncells is a multiple of 16^3 = kScanBlock: a scan block lies inside the grid or outside it)
__global__ __launch_bounds__(kThreads) void scan_block_sums_kernel(const int *cnt, const GridParams *gp, int *block_sums)
{
    __shared__ int lds[4];
    const int ncells = gp->ncells;
    const int base = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    int s = 0;
    if (blockIdx.x * kScanBlock < ncells) {
        const int4 *v = reinterpret_cast<const int4 *>(cnt + base);
#pragma unroll
        for (int k = 0; k < kScanItems / 4; k++) {
            const int4 a = v[k];
            s += (a.x + a.y) + (a.z + a.w);
        }
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) block_sums[blockIdx.x] = lds[0] + lds[1] + lds[2] + lds[3];
}

__global__ __launch_bounds__(1024) void scan_top_kernel(int *block_sums, int n_blocks)
{
    __shared__ int s_wave[16];
    block_scan_array_excl<int, 1024>(block_sums, 1, block_sums, n_blocks, s_wave, block_sums + n_blocks);   // [n_blocks]: the grand total, for the tail block
}

__global__ __launch_bounds__(kThreads) void scan_finish_kernel(const int *cnt, const GridParams *gp, const int *block_sums,
                                                               int *cell_start)
{
    __shared__ int lds[4];
    const int ncells = gp->ncells;
    const int base = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    if (blockIdx.x * kScanBlock >= ncells) {
        if (blockIdx.x * kScanBlock == ncells && threadIdx.x == 0) cell_start[ncells] = block_sums[blockIdx.x];   // = n_points
        return;
    }
    int v[kScanItems];
    int s = 0;
    {
        const int4 *v4 = reinterpret_cast<const int4 *>(cnt + base);
#pragma unroll
        for (int k = 0; k < kScanItems / 4; k++) {
            const int4 a = v4[k];
            v[4 * k] = a.x; v[4 * k + 1] = a.y; v[4 * k + 2] = a.z; v[4 * k + 3] = a.w;
            s += (a.x + a.y) + (a.z + a.w);
        }
    }
    int run = block_sums[blockIdx.x] + block_scan_incl<int, kThreads / 64>(s, lds) - s;
    int4 *o4 = reinterpret_cast<int4 *>(cell_start + base);
#pragma unroll
    for (int k = 0; k < kScanItems / 4; k++) {
        int4 o;
        o.x = run; run += v[4 * k];
        o.y = run; run += v[4 * k + 1];
        o.z = run; run += v[4 * k + 2];
        o.w = run; run += v[4 * k + 3];
        o4[k] = o;
    }
}

__global__ __launch_bounds__(kThreads) void cell_scatter_kernel(const float *pts, int n, const int *cell_of, const int *rank_of, const int *cell_start,
                                                                int *cell_cnt, float4 *sorted)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int c = cell_of[i];
    sorted[cell_start[c] + rank_of[i]] = make_float4(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], __int_as_float(i));
    cell_cnt[c] = 0;   // every touched counter back to zero (plain stores of the same value): one memset per workspace, not per build
}

// Tight AABB of every 4^3-cell block (one wave per block; its points are one contiguous range).
__global__ __launch_bounds__(kThreads) void block_box_kernel(const GridParams *gp, const int *cell_start, const float4 *sorted, Box *boxes)
{
    const int lane = threadIdx.x & 63;
    const int n_blocks = gp->ncells / 64;
    for (int b = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); b < n_blocks; b += gridDim.x * (kThreads / 64)) {
        Box bx = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0, 0};
        const int s = cell_start[b * 64], e = cell_start[b * 64 + 64];
        if (s < e) {  // wave-uniform
            for (int j = s + lane; j < e; j += 64) {
                const float4 p = sorted[j];
                bx.lx = fminf(bx.lx, p.x); bx.ly = fminf(bx.ly, p.y); bx.lz = fminf(bx.lz, p.z);
                bx.hx = fmaxf(bx.hx, p.x); bx.hy = fmaxf(bx.hy, p.y); bx.hz = fmaxf(bx.hz, p.z);
            }
            bx.lx = wave_min(bx.lx); bx.ly = wave_min(bx.ly); bx.lz = wave_min(bx.lz);
            bx.hx = wave_max(bx.hx); bx.hy = wave_max(bx.hy); bx.hz = wave_max(bx.hz);
        }
        // the point range rides in the two spare words: one 32-byte load per block in the query kernel
        bx.pad0 = __int_as_float(s);
        bx.pad1 = __int_as_float(e);
        if (lane == 0) boxes[b] = bx;
    }
}

// AABB of every super-block = union of its 64 block boxes (one wave per super-block).
__global__ __launch_bounds__(64) void super_box_kernel(const GridParams *gp, const Box *boxes, Box *supers)
{
    const int s = blockIdx.x;
    if (s >= gp->ncells / 4096) return;
    const Box b = boxes[s * 64 + threadIdx.x];
    Box r;
    r.lx = wave_min(b.lx); r.ly = wave_min(b.ly); r.lz = wave_min(b.lz);
    r.hx = wave_max(b.hx); r.hy = wave_max(b.hy); r.hz = wave_max(b.hz);
    r.pad0 = r.pad1 = 0;
    if (threadIdx.x == 0) supers[s] = r;
}

}  // namespace

// Device memory behind a list of buffers: every owner of DevBufs here names them ONCE, in its bufs(); what it reports and frees iterates that.
template <class List>
static size_t bytes_of(const List &bufs) { size_t n = 0; for (const lsn::DevBuf *b : bufs) n += b->bytes; return n; }

// One voxel grid over a cloud: the cell-sorted copy (x, y, z, original index) and, for a target, the box hierarchy.
struct GridBufs {
    lsn::DevBuf gp, cell_of, rank_of, cell_cnt, cell_start, sorted, boxes, supers;
    bool counts_clear = false;   // cell_cnt is all zero (cell_scatter_kernel writes every touched count back to zero: one memset per workspace, not per build)
    int reserve(int max_n, bool with_boxes)
    {
        int bad = 0;
        bad |= gp.reserve(sizeof(GridParams));
        bad |= cell_of.reserve(sizeof(int) * (size_t)max_n);
        bad |= rank_of.reserve(sizeof(int) * (size_t)max_n);
        bad |= cell_cnt.reserve(sizeof(int) * (size_t)kMaxCells);
        bad |= cell_start.reserve(sizeof(int) * ((size_t)kMaxCells + kScanBlock));
        bad |= sorted.reserve(sizeof(float4) * (size_t)max_n);
        if (with_boxes) {
            bad |= boxes.reserve(sizeof(Box) * (size_t)kMaxBlocks3);
            bad |= supers.reserve(sizeof(Box) * (size_t)kMaxSupers);
        }
        return bad;
    }
    std::array<lsn::DevBuf *, 8> bufs() { return {&gp, &cell_of, &rank_of, &cell_cnt, &cell_start, &sorted, &boxes, &supers}; }
};

static inline int blocks_for(int n) { return (n + kThreads - 1) / kThreads; }
static inline int capped_blocks(int n) { int b = blocks_for(n); return b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b); }

// Builds the voxel grid over a cloud (stream ordered, no host synchronisation): g.sorted = the points in cell order with
// their original index; with_boxes adds the block / super-block AABBs the query kernel culls with.  bbox_part (6 * kMaxBlocks floats) and
// block_sums (2048 ints): scratch of the workspace that owns g, shared by its grids.
static int build_grid(GridBufs &g, float *bbox_part, int *block_sums, const float *d_pts, int n, bool with_boxes, hipStream_t s)
{
    const int nb = capped_blocks(n);
    GridParams *gp = g.gp.as<GridParams>();
    hipLaunchKernelGGL(bbox_partial_kernel, dim3(nb), dim3(kThreads), 0, s, d_pts, n, bbox_part);
    hipLaunchKernelGGL(grid_setup_kernel, dim3(1), dim3(64), 0, s, bbox_part, nb, n, gp);
    if (!g.counts_clear) LSN_HIP(hipMemsetAsync(g.cell_cnt.p, 0, sizeof(int) * (size_t)kMaxCells, s));
    g.counts_clear = false;   // dirty until the scatter below has been enqueued
    const int nall = std::max(1, blocks_for(n));   // one point per thread: a capped grid makes every thread a chain of dependent rounds
    hipLaunchKernelGGL(cell_count_kernel, dim3(nall), dim3(kThreads), 0, s, d_pts, n, gp, g.cell_of.as<int>(), g.rank_of.as<int>(), g.cell_cnt.as<int>());
    const int sb = kMaxCells / kScanBlock;  // 1024
    hipLaunchKernelGGL(scan_block_sums_kernel, dim3(sb), dim3(kThreads), 0, s, g.cell_cnt.as<int>(), gp, block_sums);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(1024), 0, s, block_sums, sb);
    hipLaunchKernelGGL(scan_finish_kernel, dim3(sb + 1), dim3(kThreads), 0, s, g.cell_cnt.as<int>(), gp, block_sums,
                       g.cell_start.as<int>());
    hipLaunchKernelGGL(cell_scatter_kernel, dim3(nall), dim3(kThreads), 0, s, d_pts, n, g.cell_of.as<int>(), g.rank_of.as<int>(), g.cell_start.as<int>(),
                       g.cell_cnt.as<int>(), g.sorted.as<float4>());
    LSN_HIP(hipGetLastError());   // (a failed launch leaves counts_clear false: the next build clears them again)
    g.counts_clear = true;
    if (with_boxes) {
        hipLaunchKernelGGL(block_box_kernel, dim3(2048), dim3(kThreads), 0, s, (const GridParams *)gp, (const int *)g.cell_start.as<int>(),
                           (const float4 *)g.sorted.as<float4>(), g.boxes.as<Box>());
        hipLaunchKernelGGL(super_box_kernel, dim3(kMaxSupers), dim3(64), 0, s, (const GridParams *)gp, (const Box *)g.boxes.as<Box>(),
                           g.supers.as<Box>());
    }
    LSN_HIP(hipGetLastError());
    return 0;
}
