// simplify.hip -- mesh level of detail: vertex clustering of a tick's merged mesh on a uniform grid of edge `cell`: lsnFusionSimplify,
// lsnFusionSimplifyDiagnostics and what lsnLastMeshTransferFrameLod / lsnLastMeshPlyLod run.
//
// The reference has no decimation: the stage is DEFINED here (include/NativeUtils.h has the exact wording, tests/simplify_ref.py restates
// it).  inv = 1.0f / cell on the host; per axis q = floorf(c * inv), one uncontracted f32 multiply; a vertex whose three q are finite and
// in [-2^20, 2^20) has the 63-bit key (qx + 2^20) | (qy + 2^20) << 21 | (qz + 2^20) << 42, any other vertex is a cell of its own.  The
// vertex of LOWEST INDEX of a cell represents it and keeps its 16 bytes; the representatives leave in ascending input index; a triangle
// is remapped and dropped when two of its new indices are equal or an input index was out of range; survivors keep their order.  Nothing
// is averaged and duplicate triangles are not removed.  Per call, over every tick of the batch (grid y = tick):
//
//   1. insert (sp_insert_kernel): one lane per vertex.  An open-addressing table per tick, u64 key + u32 value, slots = the power of two
//      at or above 2 x the tick's capacity (load <= 0.5).  One returning 64-bit atomicCAS per probed slot claims it (or finds it already
//      the key's); on a foreign key the lane moves to the next slot -- it never looks at a slot twice and never waits for another lane;
//      then a no-return atomicMin of the vertex index on the slot's value.  The probe loop is bounded by the table size.  The lane leaves
//      its slot in `rep`.
//   2. look up (sp_rep_kernel), a launch later: rep = the slot's value, kept = (rep == self); the kept lanes of every 256 are counted.
//   3. ordered compaction in the project's multi-launch form: the per-tile counts of 2, their exclusive scan (ct_block_scan_kernel, one
//      workgroup per tick), then
//   4. write (sp_write_kernel): the kept vertices, 16 bytes per lane, to tile prefix + rank inside the tile, which also goes into `newidx`;
//      compact_offsets_kernel<.., false> counts the kept vertices below every entry of the offset row; sp_remap_kernel (a launch behind
//      the write) turns rep into remap = newidx[rep].
//   5. triangles: compact_tri_kernel<.., 0> (remap, flag, count per tile), the scan, compact_tri_kernel<.., 1> (write),
//      compact_offsets_kernel<.., true> -- the two kernels are mesh_batch.hip's, shared with fragments.hip.
//
// cell <= 0 or NaN: the same launches with every vertex and every triangle kept and the offset rows copied as they are.
// No kernel waits for another workgroup; every loop is bounded by a size the host passes.  Plain vector stores and HIP atomics only.
// Compiled as part of mesh.hip's translation unit (after cloud_index.hip and mesh_batch.hip: ct_block_scan_kernel, the batch).
#include "fusion_shared.hpp"

namespace {

constexpr int kSpThreads = 256;
constexpr unsigned long long kSpEmpty = ~0ull;   // no key: keys have 63 bits
constexpr float kSpLim = 1048576.0f;             // 2^20

// (restates the fields of lsn::MeshBatch: embedding it moves the kernel arguments and sp_write_kernel from 16 to 14 VGPRs)
struct SpArgs {
    const uint4 *verts;            // [n_ticks][tick_vert]
    const int *voff;               // [n_ticks][n + 1]
    const int *tri;                // [n_ticks][tick_tri][3], null in points mode
    const int *toff;               // [n_ticks][n + 1]
    uint4 *verts_out;
    int *voff_out, *tri_out, *toff_out, *remap_out;   // remap_out nullable
    unsigned long long *keys;      // [n_ticks][slots]
    unsigned int *vals;            // [n_ticks][slots]
    int *rep;                      // [n_ticks][tick_vert]: slot (-1: unclustered) -> representative -> remap
    int *newidx;                   // [n_ticks][tick_vert]: output index of a kept vertex
    int *vtile, *ttile;            // [n_ticks][nvb + 1], [n_ticks][ntb + 1]: kept per 256 -> exclusive prefixes, the last one the total
    int *cnt;                      // [n_ticks][4]: unclustered, vertices out, triangles out, triangles in
    float inv;
    int n, identity, nvb, ntb;
    unsigned int mask;             // slots - 1
    long long tick_vert, tick_tri;
};

// One axis: false when it is out of range; else its 21 bits.
__device__ __forceinline__ bool sp_axis(float c, float inv, unsigned long long &bits)
{
    const float q = floorf(__fmul_rn(c, inv));
    if (!(q >= -kSpLim && q < kSpLim)) return false;   // NaN and +-inf fail both
    bits = (unsigned long long)((int)q + (1 << 20));
    return true;
}

__device__ __forceinline__ unsigned int sp_hash(unsigned long long key)
{
    key *= 0x9E3779B97F4A7C15ull;
    return (unsigned int)(key >> 32) ^ (unsigned int)key;
}

// ---- 1. insert ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSpThreads) void sp_insert_kernel(SpArgs a)
{
    const int tick = blockIdx.y;
    const int nv = mesh_count(a.voff, tick, a.n, a.tick_vert);
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    bool loose = false;
    if (g < nv) {
        const uint4 v = a.verts[tick * a.tick_vert + g];
        unsigned long long bx, by, bz;
        int slot = -1;
        if (sp_axis(__uint_as_float(v.y), a.inv, bx) && sp_axis(__uint_as_float(v.z), a.inv, by) && sp_axis(__uint_as_float(v.w), a.inv, bz)) {
            const unsigned long long key = bx | (by << 21) | (bz << 42);
            unsigned long long *keys = a.keys + (size_t)tick * ((size_t)a.mask + 1);
            unsigned int h = sp_hash(key) & a.mask;
            for (unsigned int i = 0; i <= a.mask; i++) {   // at most nv <= slots / 2 keys: an empty slot comes first
                const unsigned long long was = atomicCAS(&keys[h], kSpEmpty, key);
                if (was == kSpEmpty || was == key) {
                    slot = (int)h;
                    break;
                }
                h = (h + 1) & a.mask;
            }
            if (slot >= 0) atomicMin(&a.vals[(size_t)tick * ((size_t)a.mask + 1) + slot], (unsigned int)g);
        }
        loose = slot < 0;
        a.rep[tick * a.tick_vert + g] = slot;
    }
    const int n_loose = __popcll(__ballot(loose));
    if ((threadIdx.x & 63) == 0 && n_loose) atomicAdd(&a.cnt[tick * 4], n_loose);
}

// ---- 2. look up ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSpThreads) void sp_rep_kernel(SpArgs a)
{
    __shared__ int s_wave[kSpThreads / 64];
    const int tick = blockIdx.y;
    const int nv = mesh_count(a.voff, tick, a.n, a.tick_vert);
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    bool kept = false;
    if (g < nv) {
        int *rep = a.rep + tick * a.tick_vert;
        int r = g;
        if (!a.identity) {
            const int slot = rep[g];
            if (slot >= 0) r = (int)a.vals[(size_t)tick * ((size_t)a.mask + 1) + slot];
        }
        rep[g] = r;
        kept = r == g;
    }
    int total;
    (void)block_rank<kSpThreads / 64>(kept, s_wave, total);
    if (threadIdx.x == 0) a.vtile[tick * (a.nvb + 1) + blockIdx.x] = total;
}

// ---- 4. write -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSpThreads) void sp_write_kernel(SpArgs a)
{
    __shared__ int s_wave[kSpThreads / 64];
    const int tick = blockIdx.y;
    const int nv = mesh_count(a.voff, tick, a.n, a.tick_vert);
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    const bool kept = g < nv && a.rep[tick * a.tick_vert + g] == g;
    int total;
    const int rank = a.vtile[tick * (a.nvb + 1) + blockIdx.x] + block_rank<kSpThreads / 64>(kept, s_wave, total);
    if (kept) {   // rank < kept vertices of the tick <= nv
        a.verts_out[tick * a.tick_vert + rank] = a.verts[tick * a.tick_vert + g];
        a.newidx[tick * a.tick_vert + g] = rank;
    }
}

__global__ __launch_bounds__(kSpThreads) void sp_remap_kernel(SpArgs a)
{
    const int tick = blockIdx.y;
    const int nv = mesh_count(a.voff, tick, a.n, a.tick_vert);
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nv) return;
    int *rep = a.rep + tick * a.tick_vert;
    const int m = a.newidx[tick * a.tick_vert + rep[g]];   // (this lane alone reads and writes rep[g])
    rep[g] = m;
    if (a.remap_out) a.remap_out[tick * a.tick_vert + g] = m;
}

// ---- 5. triangles -------------------------------------------------------------------------------------------------------------------
// The triangle at position t < nt through the remap: false when it is dropped.
__device__ __forceinline__ bool sp_triangle(const SpArgs &a, int tick, int t, int nv, int &i1, int &i2, int &i3)
{
    const int *tr = a.tri + 3 * (tick * a.tick_tri + t);
    i1 = tr[0]; i2 = tr[1]; i3 = tr[2];
    if (a.identity) return true;
    if (!((unsigned int)i1 < (unsigned int)nv && (unsigned int)i2 < (unsigned int)nv && (unsigned int)i3 < (unsigned int)nv)) return false;
    const int *remap = a.rep + tick * a.tick_vert;
    i1 = remap[i1]; i2 = remap[i2]; i3 = remap[i3];
    return i1 != i2 && i2 != i3 && i1 != i3;
}

// What compact_tri_kernel / compact_offsets_kernel (mesh_batch.hip) ask of the stage.
__device__ __forceinline__ bool compact_triangle(const SpArgs &a, int tick, int t, int nv, int &i1, int &i2, int &i3) { return sp_triangle(a, tick, t, nv, i1, i2, i3); }
// (queued in front of sp_remap_kernel: rep still names representatives)
__device__ __forceinline__ bool compact_vertex_kept(const SpArgs &a, int tick, int e) { return a.rep[tick * a.tick_vert + e] == e; }
__device__ __forceinline__ void compact_totals(const SpArgs &a, int tick, bool tri, int count, int kept)
{
    a.cnt[tick * 4 + (tri ? 2 : 1)] = kept;
    if (tri) a.cnt[tick * 4 + 3] = count;
}

}  // namespace

namespace lsn {

// The stage on a batch (d_remap_out: tick_vert ints per tick), with `ss` as its scratch: lsn_common.hpp says what the caller holds.
int simplify(SimplifyScratch &ss, const char *who, const MeshBatch &m, float cell, void *d_vertices_out, int *d_offsets_out, void *d_triangles_out,
             int *d_tri_offsets_out, int *d_remap_out, hipStream_t s)
{
    const bool points = m.tri == nullptr;
    if (!m.verts || !m.voff || !d_vertices_out || !d_offsets_out || (!points && (!m.toff || !d_triangles_out || !d_tri_offsets_out))) {
        lsn::set_error("%s: null argument", who);
        return -1;
    }
    if (check_batch(who, m)) return -1;
    const int n_ticks = m.n_ticks, n = m.n;
    const long long tick_vert = m.tick_vert, tick_tri = m.tick_tri;
    const size_t T = (size_t)n_ticks, row = sizeof(int) * (size_t)(n + 1) * T;
    if (check_out_of_place(who, m,
                           {{d_vertices_out, 16 * (size_t)tick_vert * T, "d_vertices_out"}, {d_offsets_out, row, "d_offsets_out"},
                            {points ? nullptr : d_triangles_out, 12 * (size_t)tick_tri * T, "d_triangles_out"},
                            {points ? nullptr : d_tri_offsets_out, row, "d_tri_offsets_out"}, {d_remap_out, 4 * (size_t)tick_vert * T, "d_remap_out"}},
                           "the stage reads the whole input while it writes: it runs out of place"))
        return -1;
    const bool identity = !(cell > 0.0f);   // <= 0 or NaN: off
    size_t slots = 1;
    while (slots < 2 * (size_t)tick_vert) slots <<= 1;
    const int nvb = (int)std::max<long long>(1, (tick_vert + kSpThreads - 1) / kSpThreads), ntb = (int)std::max<long long>(1, (tick_tri + kSpThreads - 1) / kSpThreads);
    const size_t tile_ints = T * ((size_t)nvb + 1 + (points ? 0 : (size_t)ntb + 1));
    if (ss.cnt.begin(T, T, s) || ss.rep.reserve(sizeof(int) * T * (size_t)std::max(tick_vert, 1LL)) ||
        ss.newidx.reserve(sizeof(int) * T * (size_t)std::max(tick_vert, 1LL)) || ss.tiles.reserve(sizeof(int) * tile_ints) || (!identity && ss.table.reserve(12 * slots * T)))
        return -1;
    // the table: every key "none", every value above any index
    if (!identity) LSN_HIP(hipMemsetAsync(ss.table.p, 0xFF, 12 * slots * T, s));
    LSN_HIP(hipMemsetAsync(ss.tiles.p, 0, sizeof(int) * tile_ints, s));
    SpArgs a;
    a.verts = m.verts;
    a.voff = m.voff;
    a.tri = m.tri;
    a.toff = m.toff;
    a.verts_out = static_cast<uint4 *>(d_vertices_out);
    a.voff_out = d_offsets_out;
    a.tri_out = static_cast<int *>(d_triangles_out);
    a.toff_out = d_tri_offsets_out;
    a.remap_out = d_remap_out;
    a.keys = ss.table.as<unsigned long long>();
    a.vals = identity ? nullptr : reinterpret_cast<unsigned int *>(ss.table.as<unsigned long long>() + slots * T);
    a.rep = ss.rep.as<int>();
    a.newidx = ss.newidx.as<int>();
    a.vtile = ss.tiles.as<int>();
    a.ttile = a.vtile + T * ((size_t)nvb + 1);
    a.cnt = ss.cnt.buf.as<int>();
    a.inv = identity ? 0.0f : 1.0f / cell;
    a.n = n;
    a.identity = identity ? 1 : 0;
    a.nvb = nvb;
    a.ntb = ntb;
    a.mask = (unsigned int)(slots - 1);
    a.tick_vert = tick_vert;
    a.tick_tri = tick_tri;
    const dim3 vgrid(nvb, n_ticks), tgrid(ntb, n_ticks), ogrid(n + 1, n_ticks), block(kSpThreads);
    if (!identity) hipLaunchKernelGGL(sp_insert_kernel, vgrid, block, 0, s, a);
    hipLaunchKernelGGL(sp_rep_kernel, vgrid, block, 0, s, a);
    hipLaunchKernelGGL(ct_block_scan_kernel, dim3(n_ticks), dim3(1024), 0, s, a.vtile, nvb + 1);
    hipLaunchKernelGGL(sp_write_kernel, vgrid, block, 0, s, a);
    hipLaunchKernelGGL((compact_offsets_kernel<SpArgs, false>), ogrid, block, 0, s, a);
    hipLaunchKernelGGL(sp_remap_kernel, vgrid, block, 0, s, a);
    if (!points) {
        hipLaunchKernelGGL((compact_tri_kernel<SpArgs, 0>), tgrid, block, 0, s, a);
        hipLaunchKernelGGL(ct_block_scan_kernel, dim3(n_ticks), dim3(1024), 0, s, a.ttile, ntb + 1);
        hipLaunchKernelGGL((compact_tri_kernel<SpArgs, 1>), tgrid, block, 0, s, a);
        hipLaunchKernelGGL((compact_offsets_kernel<SpArgs, true>), ogrid, block, 0, s, a);
    }
    LSN_HIP(hipGetLastError());
    ss.cnt.finish(n_ticks);
    return 0;
}

// {occupied cells = vertices out, unclustered vertices, dropped triangles} of one tick of the last call with `ss`; synchronises `s`.
int simplify_counts(SimplifyScratch &ss, const char *who, int tick, int *n_cells, int *n_unclustered, int *n_dropped_triangles, hipStream_t s)
{
    int c[4] = {0, 0, 0, 0};
    if (ss.cnt.read(who, "nothing has been simplified yet", tick, 0, c, s,
                    [&] { lsn::set_error("%s: the last call had %d ticks (asked for tick %d)", who, ss.cnt.ticks, tick); }))
        return -1;
    if (n_unclustered) *n_unclustered = c[0];
    if (n_cells) *n_cells = c[1];
    if (n_dropped_triangles) *n_dropped_triangles = c[3] - c[2];
    return 0;
}

}  // namespace lsn

extern "C" int lsnFusionSimplify(LsnFusion *p, float cell, const void *d_vertices, const int *d_offsets, const void *d_triangles,
                                 const int *d_tri_offsets, void *d_vertices_out, int *d_offsets_out, void *d_triangles_out, int *d_tri_offsets_out,
                                 int *d_remap_out, void *stream)
{
    return plan_export("lsnFusionSimplify", p, [&] {
        return lsn::simplify(p->sp, "lsnFusionSimplify", plan_batch(p, d_vertices, d_offsets, d_triangles, d_tri_offsets), cell, d_vertices_out,
                             d_offsets_out, d_triangles_out, d_tri_offsets_out, d_remap_out, lsn::as_stream(stream));
    });
}

extern "C" int lsnFusionSimplifyDiagnostics(LsnFusion *p, int tick, int *n_cells, int *n_unclustered, int *n_dropped_triangles, void *stream)
{
    return plan_export("lsnFusionSimplifyDiagnostics", p, [&] {
        return lsn::simplify_counts(p->sp, "lsnFusionSimplifyDiagnostics", tick, n_cells, n_unclustered, n_dropped_triangles, lsn::as_stream(stream));
    });
}
