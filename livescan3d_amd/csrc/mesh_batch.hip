// mesh_batch.hip -- what the three stages on the merged mesh (render.hip, simplify.hip, normals.hip) share: the batch they read
// (lsn::MeshBatch) with its clipped counts, its check and the out-of-place test, the counters behind their diagnostics
// (lsn::StageCounters), the form of their plan exports, and the ordered compaction of triangles and offset rows that simplify.hip and
// fragments.hip share (compact_tri_kernel, compact_offsets_kernel).  A stage checks null arguments, its own limits, the batch, the overlap.
// Compiled as part of mesh.hip's translation unit (the include at its end, ahead of the three stages), not on its own.
#include "fusion_shared.hpp"

namespace {

// The vertices (off = voff, cap = tick_vert) or the triangles (toff, tick_tri) of a tick: the last entry of its offset row, clipped to
// [0, the tick's capacity].
__device__ __forceinline__ int mesh_count(const int *off, int tick, int n, long long cap)
{
    return max(0, (int)min((long long)off[tick * (n + 1) + n], cap));
}

// The plan's own batch: what lsnFusionRunMesh wrote, or anything a caller laid out like it.
lsn::MeshBatch plan_batch(const LsnFusion *p, const void *d_vertices, const int *d_offsets, const void *d_triangles, const int *d_tri_offsets)
{
    return {static_cast<const uint4 *>(d_vertices), d_offsets, static_cast<const int *>(d_triangles), d_tri_offsets, p->cap, 2 * p->cap, p->n_ticks, p->n_maps};
}

// The bounds keep every index of a tick (and three times a triangle's) inside an int.
int check_batch(const char *who, const lsn::MeshBatch &m)
{
    if (m.n_ticks >= 1 && m.n >= 0 && m.tick_vert >= 0 && m.tick_tri >= 0 && m.tick_vert <= 0x3FFFFFFFll && m.tick_tri <= 0x7FFFFFFFll / 3) return 0;
    lsn::set_error("%s: bad batch", who);
    return -1;
}

struct Range { const void *p; size_t bytes; const char *name; };

// Out of place: no range of `out` may overlap what a stage reads of the batch, the inputs under the names its export gives them (null
// ranges are not there; a batch without triangles has no triangle offsets either); `why` ends the message.
int check_out_of_place(const char *who, const lsn::MeshBatch &m, std::initializer_list<Range> out, const char *why)
{
    const size_t T = (size_t)m.n_ticks, row = sizeof(int) * (size_t)(m.n + 1) * T;
    const Range in[4] = {{m.verts, 16 * (size_t)m.tick_vert * T, "d_vertices"}, {m.voff, row, "d_offsets"},
                         {m.tri, 12 * (size_t)m.tick_tri * T, "d_triangles"}, {m.tri ? m.toff : nullptr, row, "d_tri_offsets"}};
    for (const Range &o : out)
        for (const Range &i : in) {
            const uintptr_t x = (uintptr_t)i.p, y = (uintptr_t)o.p;
            if (i.p && o.p && x < y + o.bytes && y < x + i.bytes) {
                lsn::set_error("%s: %s overlaps %s (%s)", who, o.name, i.name, why);
                return -1;
            }
        }
    return 0;
}

// A plan export of the three stages: one guarded entry under the export's name, the error cleared, the plan there, locked, its device current.
template <class F>
int plan_export(const char *name, LsnFusion *p, F &&body)
{
    return lsn::guarded(name, -1, [&]() {
        lsn::clear_error();
        if (!p) {
            lsn::set_error("%s: null argument", name);
            return -1;
        }
        std::lock_guard<std::mutex> g(p->mu);
        LSN_HIP(hipSetDevice(p->device));
        return body();
    });
}

// ---- the ordered compaction of a tick's triangles and of its two offset rows, shared by the stages that drop vertices (simplify.hip,
// fragments.hip).  A stage's argument block A has voff / tri / toff / tri_out / voff_out / toff_out, vtile / ttile ([n_ticks][nvb + 1],
// [n_ticks][ntb + 1]: kept per 256, then their exclusive prefixes with the total last), n, identity, nvb, ntb, tick_vert, tick_tri, and
// the stage says what is kept through three functions found by their argument:
//   bool compact_triangle(const A &, tick, t, nv, i1, i2, i3)   the triangle at position t < nt through the remap; false: dropped
//   bool compact_vertex_kept(const A &, tick, e)                vertex e < nv leaves
//   void compact_totals(const A &, tick, tri, count, kept)      entry n of a row (tri: the triangles') is written: the stage's counters
constexpr int kCompactThreads = 256;

template <class A, int WRITE>
__global__ __launch_bounds__(kCompactThreads) void compact_tri_kernel(A a)
{
    __shared__ int s_wave[kCompactThreads / 64];
    const int tick = blockIdx.y;
    const int nv = mesh_count(a.voff, tick, a.n, a.tick_vert), nt = mesh_count(a.toff, tick, a.n, a.tick_tri);
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    int i1 = 0, i2 = 0, i3 = 0;
    const bool kept = t < nt && compact_triangle(a, tick, t, nv, i1, i2, i3);
    int total;
    const int rank = block_rank<kCompactThreads / 64>(kept, s_wave, total);
    if (!WRITE) {
        if (threadIdx.x == 0) a.ttile[tick * (a.ntb + 1) + blockIdx.x] = total;
    } else if (kept) {   // prefix + rank < surviving triangles of the tick <= nt
        int *o = a.tri_out + 3 * (tick * a.tick_tri + a.ttile[tick * (a.ntb + 1) + blockIdx.x] + rank);
        o[0] = i1; o[1] = i2; o[2] = i3;
    }
}

// The offset rows, one workgroup per (entry, tick): out[i] = the kept elements below in[i] -- the prefix of in[i]'s tile plus the kept
// ones of that tile in front of it.
template <class A, bool TRI>
__global__ __launch_bounds__(kCompactThreads) void compact_offsets_kernel(A a)
{
    __shared__ int s_wave[kCompactThreads / 64];
    const int tick = blockIdx.y, i = blockIdx.x;
    const int nv = mesh_count(a.voff, tick, a.n, a.tick_vert);
    const int count = TRI ? mesh_count(a.toff, tick, a.n, a.tick_tri) : nv;
    const int *tile = TRI ? a.ttile + tick * (a.ntb + 1) : a.vtile + tick * (a.nvb + 1);
    const int nb = TRI ? a.ntb : a.nvb;
    const int in = (TRI ? a.toff : a.voff)[tick * (a.n + 1) + i];
    const int j = min(max(in, 0), count);
    const int b = min(j / kCompactThreads, nb);      // tile[nb] is the total; j == count may lie there
    const int e = b * kCompactThreads + threadIdx.x;
    bool kept = false;
    if (e < j) {
        if (TRI) {
            int i1, i2, i3;
            kept = compact_triangle(a, tick, e, nv, i1, i2, i3);
        } else {
            kept = compact_vertex_kept(a, tick, e);
        }
    }
    int total;
    (void)block_rank<kCompactThreads / 64>(kept, s_wave, total);
    if (threadIdx.x == 0) {
        const int below = tile[b] + total;
        (TRI ? a.toff_out : a.voff_out)[tick * (a.n + 1) + i] = a.identity ? in : below;
        if (i == a.n) compact_totals(a, tick, TRI, count, tile[nb]);
    }
}

}  // namespace

int lsn::StageCounters::begin(size_t reserve_slots, size_t slots, hipStream_t s)
{
    ticks = per_tick = 0;
    if (buf.reserve(sizeof(int) * 4 * reserve_slots)) return -1;
    LSN_HIP(hipMemsetAsync(buf.p, 0, sizeof(int) * 4 * slots, s));
    return 0;
}

template <class F>
int lsn::StageCounters::read(const char *who, const char *nothing_yet, int tick, int sub, int c[4], hipStream_t s, F &&out_of_range) const
{
    if (ticks <= 0) {
        lsn::set_error("%s: %s", who, nothing_yet);
        return -1;
    }
    if (tick < 0 || tick >= ticks || sub < 0 || sub >= per_tick) {
        out_of_range();
        return -1;
    }
    LSN_HIP(hipMemcpyAsync(c, buf.as<int>() + 4 * ((size_t)tick * per_tick + sub), 4 * sizeof(int), hipMemcpyDeviceToHost, s));
    LSN_HIP(hipStreamSynchronize(s));
    return 0;
}
