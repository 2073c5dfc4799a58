// fragments.hip -- the fragment filter: the small connected components of a tick's merged mesh are dropped: lsnFusionFragments,
// lsnFusionFragmentsDiagnostics and what lsnLastMeshTransferFrameFragments / lsnLastMeshPlyFragments run.
//
// The reference has no such step: the stage is DEFINED here (include/NativeUtils.h has the exact wording, tests/fragments_ref.py restates
// it).  A triangle whose three indices lie in [0, nVertices) joins i0-i1 and i1-i2; label[v] is the LOWEST vertex index of v's connected
// component, a component's size the number of vertices that carry its label; a vertex is kept iff size[label[v]] >= min_vertices.  The
// kept vertices leave in ascending input index with their own 16 bytes, the valid triangles of kept components are remapped and keep
// their order.  Only minima and integer counts: the bytes do not depend on the order in which the device takes the triangles.
// Per call, over every tick of the batch (grid y = tick):
//
//   1. init (fr_init_kernel): parent[v] = v, size[v] = 0 for the tick's counted vertices.
//   2. union (fr_union_kernel): one lane per triangle, two unions by union_find.hpp's lock-free union (its header says how parent[] is
//      touched and why plain loads suffice): the HIGHER root is hooked under the LOWER, so parent[v] <= v holds at every moment and a
//      tree's root is its lowest index.  Paths are shortened inside the launch only by a no-return atomicMin(&parent[v], r) on the
//      triangle's own three vertices, r the root the lane's last union ended on: r lies in v's tree and below v, so parent[v] <= v and
//      "parent[v] is in v's tree" both survive, in any interleaving with the hooks (a hook writes only roots, and a vertex with a lower
//      vertex in its tree is none).  Halving the path on every step of a walk, by atomicMin or by a store, was measured and is slower
//      (1.2 - 2.0 ms for the call against 1.0 ms): the walks are a chain of dependent loads, and the extra traffic costs more than the
//      shorter paths save.
//   3. flatten (fr_jump_kernel), ceil(log2(vertices per tick)) launches: parent[v] = parent[parent[v]], one step per lane per launch, plain
//      loads and one plain store of the lane's own word.  A launch sees at least what the launch before wrote; what it sees of its own
//      launch is an ancestor further up.  Every hop of the new forest covers two hops of the old one (or ends on the root), so a launch
//      halves the depth, rounded up; the depth after the unions is below the tick's vertex capacity, so after that many launches it is
//      at most 1 -- parent[v] is the root, the label.  The bound is the capacity's logarithm, stated by the host; the mesh's depth (a chain
//      hooked in descending order is nVertices deep) bounds nothing here.
//   4. sizes (fr_size_kernel): one integer atomicAdd on size[label] per RUN of equal labels inside a wave (the run's head finds its
//      length in the ballot of the heads), as icp_grid.hip counts its cells -- on a surface nearly every lane of a wave has the same label.
//      The lanes that are their own label are the tick's components.
//   5. ordered compaction in the project's multi-launch form, as simplify.hip does it: fr_keep_kernel (kept = size[label] >=
//      min_vertices, kept per 256), ct_block_scan_kernel, fr_write_kernel (vertices, remap, labels), compact_offsets_kernel<.., false>,
//      then compact_tri_kernel<.., 0>, the scan, compact_tri_kernel<.., 1>, compact_offsets_kernel<.., true> -- those two kernels are
//      mesh_batch.hip's, written once for this stage and simplify.hip.  No look-back, no single-pass scan.
//
// min_vertices <= 1: launches 5 alone with every vertex and every triangle kept and the offset rows copied as they are; parent[] is not
// touched, the labels are not written, the counters stay 0.
// No kernel waits for another workgroup; every loop is bounded by a size the host passes or by a vertex index.  Plain vector stores and
// HIP atomics only.  Compiled as part of mesh.hip's translation unit (after cloud_index.hip and mesh_batch.hip: ct_block_scan_kernel, the
// batch), behind simplify.hip.
#include "fusion_shared.hpp"
#include "union_find.hpp"

namespace {

constexpr int kFrThreads = 256;

struct FrArgs {
    const uint4 *verts;            // [n_ticks][tick_vert]
    const int *voff;               // [n_ticks][n + 1]
    const int *tri;                // [n_ticks][tick_tri][3]
    const int *toff;               // [n_ticks][n + 1]
    uint4 *verts_out;
    int *voff_out, *tri_out, *toff_out, *remap_out, *labels_out;   // remap_out, labels_out nullable
    int *parent;                   // [n_ticks][tick_vert]: the forest -> the label
    int *size;                     // [n_ticks][tick_vert]: vertices per label, at the label's index
    int *newidx;                   // [n_ticks][tick_vert]: 0 kept / -1 removed -> the output index / -1: the remap
    int *vtile, *ttile;            // [n_ticks][nvb + 1], [n_ticks][ntb + 1]: kept per 256 -> exclusive prefixes, the last one the total
    int *cnt;                      // [n_ticks][4]: components, removed components, removed vertices, dropped triangles
    int n, identity, nvb, ntb, min_vertices;
    long long tick_vert, tick_tri;
};

// ---- 1. init ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFrThreads) void fr_init_kernel(FrArgs a)
{
    const int tick = blockIdx.y;
    const int nv = mesh_count(a.voff, tick, a.n, a.tick_vert);
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nv) return;
    a.parent[tick * a.tick_vert + g] = g;
    a.size[tick * a.tick_vert + g] = 0;
}

// ---- 2. union -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFrThreads) void fr_union_kernel(FrArgs a)
{
    const int tick = blockIdx.y;
    const int nv = mesh_count(a.voff, tick, a.n, a.tick_vert), nt = mesh_count(a.toff, tick, a.n, a.tick_tri);
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const int *tr = a.tri + 3 * (tick * a.tick_tri + t);
    const int i0 = tr[0], i1 = tr[1], i2 = tr[2];
    if (!((unsigned int)i0 < (unsigned int)nv && (unsigned int)i1 < (unsigned int)nv && (unsigned int)i2 < (unsigned int)nv)) return;
    int *parent = a.parent + tick * a.tick_vert;
    const int r = uf_unite(parent, uf_unite(parent, i0, i1), i2);   // (the first union's root stands for i1: one walk less)
    if (r < i0) atomicMin(&parent[i0], r);                          // no return; r lies in the three vertices' tree, below them
    if (r < i1) atomicMin(&parent[i1], r);
    if (r < i2) atomicMin(&parent[i2], r);
}

// ---- 3. flatten: one pointer-doubling step ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFrThreads) void fr_jump_kernel(FrArgs a)
{
    const int tick = blockIdx.y;
    const int nv = mesh_count(a.voff, tick, a.n, a.tick_vert);
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nv) return;
    int *parent = a.parent + tick * a.tick_vert;
    const int p = parent[g];
    if (p == g) return;
    const int gp = parent[p];                            // as the launch found it, or already further up: an ancestor either way
    if (gp != p) parent[g] = gp;                         // (this lane alone writes parent[g])
}

// ---- 4. sizes -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFrThreads) void fr_size_kernel(FrArgs a)
{
    const int tick = blockIdx.y;
    const int nv = mesh_count(a.voff, tick, a.n, a.tick_vert);
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool there = g < nv;
    const int label = there ? a.parent[tick * a.tick_vert + g] : -1;   // -1 ends the run in front of the lanes behind the tick
    const int before = __shfl_up(label, 1);
    const bool head = lane == 0 || before != label;
    const unsigned long long heads = __ballot(head);
    if (head && there) {
        const unsigned long long above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
        const int next = above ? __ffsll((long long)above) - 1 : 64;   // the next run's head (the lanes behind the tick are one)
        atomicAdd(&a.size[tick * a.tick_vert + label], next - lane);
    }
    const int roots = __popcll(__ballot(there && label == g));
    if (lane == 0 && roots) atomicAdd(&a.cnt[tick * 4], roots);
}

// ---- 5. compaction ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFrThreads) void fr_keep_kernel(FrArgs a)
{
    __shared__ int s_wave[kFrThreads / 64];
    const int tick = blockIdx.y;
    const int nv = mesh_count(a.voff, tick, a.n, a.tick_vert);
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    bool kept = false, lost_root = false;
    if (g < nv) {
        kept = true;
        if (!a.identity) {
            const int label = a.parent[tick * a.tick_vert + g];
            kept = a.size[tick * a.tick_vert + label] >= a.min_vertices;
            lost_root = !kept && label == g;
        }
        a.newidx[tick * a.tick_vert + g] = kept ? 0 : -1;
    }
    const int lost = __popcll(__ballot(lost_root));
    if ((threadIdx.x & 63) == 0 && lost) atomicAdd(&a.cnt[tick * 4 + 1], lost);
    int total;
    (void)block_rank<kFrThreads / 64>(kept, s_wave, total);
    if (threadIdx.x == 0) a.vtile[tick * (a.nvb + 1) + blockIdx.x] = total;
}

__global__ __launch_bounds__(kFrThreads) void fr_write_kernel(FrArgs a)
{
    __shared__ int s_wave[kFrThreads / 64];
    const int tick = blockIdx.y;
    const int nv = mesh_count(a.voff, tick, a.n, a.tick_vert);
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    const bool kept = g < nv && a.newidx[tick * a.tick_vert + g] >= 0;
    int total;
    const int rank = a.vtile[tick * (a.nvb + 1) + blockIdx.x] + block_rank<kFrThreads / 64>(kept, s_wave, total);
    if (g >= nv) return;
    if (kept) a.verts_out[tick * a.tick_vert + rank] = a.verts[tick * a.tick_vert + g];   // rank < kept vertices of the tick <= nv
    const int m = kept ? rank : -1;
    a.newidx[tick * a.tick_vert + g] = m;                // (this lane alone reads and writes newidx[g])
    if (a.remap_out) a.remap_out[tick * a.tick_vert + g] = m;
    if (a.labels_out && !a.identity) a.labels_out[tick * a.tick_vert + g] = a.parent[tick * a.tick_vert + g];
}

// The triangle at position t < nt through the remap: false when it is dropped.  Its three vertices share one component, so one fate.
__device__ __forceinline__ bool fr_triangle(const FrArgs &a, int tick, int t, int nv, int &i0, int &i1, int &i2)
{
    const int *tr = a.tri + 3 * (tick * a.tick_tri + t);
    i0 = tr[0]; i1 = tr[1]; i2 = tr[2];
    if (a.identity) return true;
    if (!((unsigned int)i0 < (unsigned int)nv && (unsigned int)i1 < (unsigned int)nv && (unsigned int)i2 < (unsigned int)nv)) return false;
    const int *remap = a.newidx + tick * a.tick_vert;
    i0 = remap[i0];
    if (i0 < 0) return false;
    i1 = remap[i1]; i2 = remap[i2];
    return true;
}

// What compact_tri_kernel / compact_offsets_kernel (mesh_batch.hip) ask of the stage.
__device__ __forceinline__ bool compact_triangle(const FrArgs &a, int tick, int t, int nv, int &i0, int &i1, int &i2) { return fr_triangle(a, tick, t, nv, i0, i1, i2); }
__device__ __forceinline__ bool compact_vertex_kept(const FrArgs &a, int tick, int e) { return a.newidx[tick * a.tick_vert + e] >= 0; }
// Entry n of a row: the tick's "in minus out" counter (off: the counters stay 0).
__device__ __forceinline__ void compact_totals(const FrArgs &a, int tick, bool tri, int count, int kept)
{
    if (!a.identity) a.cnt[tick * 4 + (tri ? 3 : 2)] = count - kept;
}

// Pointer-doubling launches that flatten any forest over `tick_vert` vertices: the least k with 2^k >= tick_vert.
int fr_jump_launches(long long tick_vert)
{
    int k = 0;
    while ((1LL << k) < tick_vert) k++;
    return k;
}

}  // namespace

namespace lsn {

// The stage on a batch (d_remap_out, d_labels_out: tick_vert ints per tick, nullable), with `fs` as its scratch: lsn_common.hpp says what
// the caller holds.
int fragments(FragmentsScratch &fs, const char *who, const MeshBatch &m, int min_vertices, void *d_vertices_out, int *d_offsets_out,
              void *d_triangles_out, int *d_tri_offsets_out, int *d_remap_out, int *d_labels_out, hipStream_t s)
{
    if (!m.tri) {
        lsn::set_error("%s: d_triangles is null (the components of a bare point cloud are not defined)", who);
        return -1;
    }
    if (!m.verts || !m.voff || !m.toff || !d_vertices_out || !d_offsets_out || !d_triangles_out || !d_tri_offsets_out) {
        lsn::set_error("%s: null argument", who);
        return -1;
    }
    if (check_batch(who, m)) return -1;
    const int n_ticks = m.n_ticks, n = m.n;
    const long long tick_vert = m.tick_vert, tick_tri = m.tick_tri;
    const size_t T = (size_t)n_ticks, row = sizeof(int) * (size_t)(n + 1) * T;
    if (check_out_of_place(who, m,
                           {{d_vertices_out, 16 * (size_t)tick_vert * T, "d_vertices_out"}, {d_offsets_out, row, "d_offsets_out"},
                            {d_triangles_out, 12 * (size_t)tick_tri * T, "d_triangles_out"}, {d_tri_offsets_out, row, "d_tri_offsets_out"},
                            {d_remap_out, 4 * (size_t)tick_vert * T, "d_remap_out"}, {d_labels_out, 4 * (size_t)tick_vert * T, "d_labels_out"}},
                           "the stage reads the whole input while it writes: it runs out of place"))
        return -1;
    const bool identity = min_vertices <= 1;
    const int nvb = (int)std::max<long long>(1, (tick_vert + kFrThreads - 1) / kFrThreads), ntb = (int)std::max<long long>(1, (tick_tri + kFrThreads - 1) / kFrThreads);
    const size_t tile_ints = T * ((size_t)nvb + 1 + (size_t)ntb + 1), per_vertex = sizeof(int) * T * (size_t)std::max(tick_vert, 1LL);
    if (fs.cnt.begin(T, T, s) || fs.newidx.reserve(per_vertex) || fs.tiles.reserve(sizeof(int) * tile_ints) ||
        (!identity && (fs.parent.reserve(per_vertex) || fs.size.reserve(per_vertex))))
        return -1;
    LSN_HIP(hipMemsetAsync(fs.tiles.p, 0, sizeof(int) * tile_ints, s));
    FrArgs a;
    a.verts = m.verts;
    a.voff = m.voff;
    a.tri = m.tri;
    a.toff = m.toff;
    a.verts_out = static_cast<uint4 *>(d_vertices_out);
    a.voff_out = d_offsets_out;
    a.tri_out = static_cast<int *>(d_triangles_out);
    a.toff_out = d_tri_offsets_out;
    a.remap_out = d_remap_out;
    a.labels_out = d_labels_out;
    a.parent = fs.parent.as<int>();
    a.size = fs.size.as<int>();
    a.newidx = fs.newidx.as<int>();
    a.vtile = fs.tiles.as<int>();
    a.ttile = a.vtile + T * ((size_t)nvb + 1);
    a.cnt = fs.cnt.buf.as<int>();
    a.n = n;
    a.identity = identity ? 1 : 0;
    a.nvb = nvb;
    a.ntb = ntb;
    a.min_vertices = min_vertices;
    a.tick_vert = tick_vert;
    a.tick_tri = tick_tri;
    const dim3 vgrid(nvb, n_ticks), tgrid(ntb, n_ticks), ogrid(n + 1, n_ticks), block(kFrThreads);
    if (!identity) {
        hipLaunchKernelGGL(fr_init_kernel, vgrid, block, 0, s, a);
        hipLaunchKernelGGL(fr_union_kernel, tgrid, block, 0, s, a);
        for (int k = fr_jump_launches(tick_vert); k > 0; k--) hipLaunchKernelGGL(fr_jump_kernel, vgrid, block, 0, s, a);
        hipLaunchKernelGGL(fr_size_kernel, vgrid, block, 0, s, a);
    }
    hipLaunchKernelGGL(fr_keep_kernel, vgrid, block, 0, s, a);
    hipLaunchKernelGGL(ct_block_scan_kernel, dim3(n_ticks), dim3(1024), 0, s, a.vtile, nvb + 1);
    hipLaunchKernelGGL(fr_write_kernel, vgrid, block, 0, s, a);
    hipLaunchKernelGGL((compact_offsets_kernel<FrArgs, false>), ogrid, block, 0, s, a);
    hipLaunchKernelGGL((compact_tri_kernel<FrArgs, 0>), tgrid, block, 0, s, a);
    hipLaunchKernelGGL(ct_block_scan_kernel, dim3(n_ticks), dim3(1024), 0, s, a.ttile, ntb + 1);
    hipLaunchKernelGGL((compact_tri_kernel<FrArgs, 1>), tgrid, block, 0, s, a);
    hipLaunchKernelGGL((compact_offsets_kernel<FrArgs, true>), ogrid, block, 0, s, a);
    LSN_HIP(hipGetLastError());
    fs.cnt.finish(n_ticks);
    return 0;
}

// {components, removed components, removed vertices, dropped triangles} of one tick of the last call with `fs`; synchronises `s`.
int fragments_counts(FragmentsScratch &fs, const char *who, int tick, int *n_components, int *n_removed_components, int *n_removed_vertices,
                     int *n_dropped_triangles, hipStream_t s)
{
    int c[4] = {0, 0, 0, 0};
    if (fs.cnt.read(who, "nothing has been filtered yet", tick, 0, c, s,
                    [&] { lsn::set_error("%s: the last call had %d ticks (asked for tick %d)", who, fs.cnt.ticks, tick); }))
        return -1;
    if (n_components) *n_components = c[0];
    if (n_removed_components) *n_removed_components = c[1];
    if (n_removed_vertices) *n_removed_vertices = c[2];
    if (n_dropped_triangles) *n_dropped_triangles = c[3];
    return 0;
}

}  // namespace lsn

extern "C" int lsnFusionFragments(LsnFusion *p, int min_vertices, const void *d_vertices, const int *d_offsets, const void *d_triangles,
                                  const int *d_tri_offsets, void *d_vertices_out, int *d_offsets_out, void *d_triangles_out, int *d_tri_offsets_out,
                                  int *d_remap_out, int *d_labels_out, void *stream)
{
    return plan_export("lsnFusionFragments", p, [&] {
        return lsn::fragments(p->fr, "lsnFusionFragments", plan_batch(p, d_vertices, d_offsets, d_triangles, d_tri_offsets), min_vertices,
                              d_vertices_out, d_offsets_out, d_triangles_out, d_tri_offsets_out, d_remap_out, d_labels_out, lsn::as_stream(stream));
    });
}

extern "C" int lsnFusionFragmentsDiagnostics(LsnFusion *p, int tick, int *n_components, int *n_removed_components, int *n_removed_vertices,
                                             int *n_dropped_triangles, void *stream)
{
    return plan_export("lsnFusionFragmentsDiagnostics", p, [&] {
        return lsn::fragments_counts(p->fr, "lsnFusionFragmentsDiagnostics", tick, n_components, n_removed_components, n_removed_vertices,
                                     n_dropped_triangles, lsn::as_stream(stream));
    });
}
