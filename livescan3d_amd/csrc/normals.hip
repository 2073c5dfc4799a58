// normals.hip -- vertex normals of a tick's merged mesh: lsnFusionNormals, lsnFusionNormalsDiagnostics and what lsnLastMeshPlyNormals runs
// (DESIGN.md section 16).
//
// The reference computes no normals: the stage is DEFINED here (include/NativeUtils.h has the exact wording, tests/normals_ref.py restates
// it).  A triangle (i0, i1, i2) whose indices are in [0, nVertices) has the face vector f = (p2 - p0) x (p1 - p0), every f32 operation
// rounded on its own; it is USED iff |fx|, |fy|, |fz| < 4096 (compared in float; NaN and inf fail), else skipped.  q = (int64) trunc(f *
// 2^40) (both steps exact) is added to the three 64-bit integer sums of each of its vertices, two's complement with wrap-around: integer
// addition is associative, so the sums -- and with them every byte of the output -- do not depend on the order in which the device takes
// the triangles.  A vertex whose sums are (0, 0, 0) has the normal (+0, +0, +0); any other s = (float) S (one round-to-nearest-even
// conversion per component), len = sqrtf((s.x * s.x + s.y * s.y) + s.z * s.z), n = s / len.  Per call, over every tick (grid y = tick):
//
//   0. clear (nm_clear_kernel): one lane per counted vertex zeroes its three sums.
//   1. faces (nm_face_kernel): one lane per triangle, grid-stride, wave-uniform trip count.  12 B of indices, the range check, three
//      16-byte gathers, the face vector, the range test, the conversion, then up to nine no-return 64-bit integer atomicAdds into the
//      three PLANES [3][capacity] of the tick (a wave that adds to consecutive vertices touches 512 contiguous bytes); adds of 0 are
//      skipped.  Used and skipped triangles: one add per wave at the end.
//   2. finish (nm_finish_kernel), a launch later: one lane per vertex, three i64 loads, the conversion, the normalisation, 12 B out;
//      the zero normals are counted, one add per wave.
//
// No kernel waits for another workgroup; every loop is bounded by a clipped count.  Plain vector stores and HIP atomics only.
// Compiled as part of mesh.hip's translation unit (after mesh_batch.hip, whose batch, counters and export form the three stages share).
#include "fusion_shared.hpp"

namespace {

constexpr int kNmThreads = 256;
constexpr int kNmMaxBlocks = 8192;               // of the face pass per tick: 32 workgroups per CU, the rest is the grid-stride loop
constexpr float kNmLim = 4096.0f;                // a face component at or above it (2^12 m^2) takes the triangle out
constexpr float kNmScale = 1099511627776.0f;     // 2^40: the sums count 2^-40 m^2

struct NmArgs {
    lsn::MeshBatch m;              // the input
    float *out;                    // [n_ticks][tick_vert][3]
    unsigned long long *acc;       // [n_ticks][3][tick_vert]: the sums' bits (two's complement)
    int *cnt;                      // [n_ticks][4]: used, skipped, zero normals, unused
};

// ---- 0. clear -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kNmThreads) void nm_clear_kernel(NmArgs a)
{
    const int tick = blockIdx.y;
    const int nv = mesh_count(a.m.voff, tick, a.m.n, a.m.tick_vert);
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nv) return;
    unsigned long long *acc = a.acc + 3 * tick * a.m.tick_vert;
    acc[g] = 0;
    acc[a.m.tick_vert + g] = 0;
    acc[2 * a.m.tick_vert + g] = 0;
}

// ---- 1. faces -----------------------------------------------------------------------------------------------------------------------
// One component of a used triangle into the plane `acc` at its three vertices (all below nVertices <= tick_vert).
__device__ __forceinline__ void nm_add(unsigned long long *acc, int i0, int i1, int i2, float c)
{
    const long long q = (long long)__fmul_rn(c, kNmScale);   // |c| < 2^12: the product is exact and below 2^52, the conversion truncates nothing but a fraction
    if (q == 0) return;
    atomicAdd(&acc[i0], (unsigned long long)q);               // result unused: no return value is asked of the memory system
    atomicAdd(&acc[i1], (unsigned long long)q);
    atomicAdd(&acc[i2], (unsigned long long)q);
}

__global__ __launch_bounds__(kNmThreads) void nm_face_kernel(NmArgs a)
{
    const int tick = blockIdx.y;
    const int nv = mesh_count(a.m.voff, tick, a.m.n, a.m.tick_vert), nt = mesh_count(a.m.toff, tick, a.m.n, a.m.tick_tri);
    const uint4 *verts = a.m.verts + tick * a.m.tick_vert;
    const int *tri = a.m.tri + 3 * (tick * a.m.tick_tri);
    unsigned long long *acc = a.acc + 3 * tick * a.m.tick_vert;
    const int lane = threadIdx.x & 63;
    const int stride = gridDim.x * kNmThreads;                // <= kNmMaxBlocks x 256; nt <= 2^31 / 3: base + stride stays an int
    int used = 0, skipped = 0;
    for (int base = blockIdx.x * kNmThreads + (threadIdx.x - lane); base < nt; base += stride) {   // the same trips for a wave's 64 lanes
        const int t = base + lane;
        bool ok = false;
        if (t < nt) {
            const int i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];
            if ((unsigned int)i0 < (unsigned int)nv && (unsigned int)i1 < (unsigned int)nv && (unsigned int)i2 < (unsigned int)nv) {
                const uint4 p0 = verts[i0], p1 = verts[i1], p2 = verts[i2];   // {colour, x, y, z}
                const float ux = __fsub_rn(__uint_as_float(p2.y), __uint_as_float(p0.y)), uy = __fsub_rn(__uint_as_float(p2.z), __uint_as_float(p0.z)),
                            uz = __fsub_rn(__uint_as_float(p2.w), __uint_as_float(p0.w));
                const float vx = __fsub_rn(__uint_as_float(p1.y), __uint_as_float(p0.y)), vy = __fsub_rn(__uint_as_float(p1.z), __uint_as_float(p0.z)),
                            vz = __fsub_rn(__uint_as_float(p1.w), __uint_as_float(p0.w));
                const float fx = __fsub_rn(__fmul_rn(uy, vz), __fmul_rn(uz, vy));
                const float fy = __fsub_rn(__fmul_rn(uz, vx), __fmul_rn(ux, vz));
                const float fz = __fsub_rn(__fmul_rn(ux, vy), __fmul_rn(uy, vx));
                if (fabsf(fx) < kNmLim && fabsf(fy) < kNmLim && fabsf(fz) < kNmLim) {   // NaN and +-inf fail
                    ok = true;
                    nm_add(acc, i0, i1, i2, fx);
                    nm_add(acc + a.m.tick_vert, i0, i1, i2, fy);
                    nm_add(acc + 2 * a.m.tick_vert, i0, i1, i2, fz);
                }
            }
        }
        used += __popcll(__ballot(ok));
        skipped += __popcll(__ballot(t < nt && !ok));
    }
    if (lane == 0) {
        if (used) atomicAdd(&a.cnt[tick * 4], used);
        if (skipped) atomicAdd(&a.cnt[tick * 4 + 1], skipped);
    }
}

// ---- 2. finish ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kNmThreads) void nm_finish_kernel(NmArgs a)
{
    const int tick = blockIdx.y;
    const int nv = mesh_count(a.m.voff, tick, a.m.n, a.m.tick_vert);
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    bool zero = false;
    if (g < nv) {
        const unsigned long long *acc = a.acc + 3 * tick * a.m.tick_vert;
        const long long sx = (long long)acc[g], sy = (long long)acc[a.m.tick_vert + g], sz = (long long)acc[2 * a.m.tick_vert + g];
        zero = (sx | sy | sz) == 0;
        float nx = 0.0f, ny = 0.0f, nz = 0.0f;
        if (!zero) {
            const float x = (float)sx, y = (float)sy, z = (float)sz;       // round to nearest even, |.| <= 2^63: the squares stay finite
            const float len = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z)));   // >= 1; correctly rounded, as the divisions are
            nx = x / len;
            ny = y / len;
            nz = z / len;
        }
        float *o = a.out + 3 * (tick * a.m.tick_vert + g);
        o[0] = nx;
        o[1] = ny;
        o[2] = nz;
    }
    const int n_zero = __popcll(__ballot(zero));
    if ((threadIdx.x & 63) == 0 && n_zero) atomicAdd(&a.cnt[tick * 4 + 2], n_zero);
}

}  // namespace

namespace lsn {

// The stage on a batch, with `ns` as its scratch.  prof (nullable): a plan whose profiling (lsnFusionProfile) then brackets the face pass.
int normals(NormalsScratch &ns, const char *who, const MeshBatch &m, void *d_normals_out, LsnFusion *prof, hipStream_t s)
{
    if (!m.verts || !m.voff || !m.toff || !d_normals_out) {
        lsn::set_error("%s: null argument", who);
        return -1;
    }
    if (!m.tri) {
        lsn::set_error("%s: null argument (d_triangles: the normals of a bare point cloud are not defined)", who);
        return -1;
    }
    if (check_batch(who, m)) return -1;
    const long long tick_vert = m.tick_vert, tick_tri = m.tick_tri;
    const size_t T = (size_t)m.n_ticks;
    if (check_out_of_place(who, m, {{d_normals_out, 12 * (size_t)tick_vert * T, "d_normals_out"}}, "the stage runs out of place")) return -1;
    if (ns.cnt.begin(T, T, s) || ns.acc.reserve(24 * T * (size_t)std::max(tick_vert, 1LL))) return -1;
    NmArgs a;
    a.m = m;
    a.out = static_cast<float *>(d_normals_out);
    a.acc = ns.acc.as<unsigned long long>();
    a.cnt = ns.cnt.buf.as<int>();
    const int nvb = (int)std::max<long long>(1, (tick_vert + kNmThreads - 1) / kNmThreads);
    const int ntb = (int)std::min<long long>(kNmMaxBlocks, std::max<long long>(1, (tick_tri + kNmThreads - 1) / kNmThreads));
    const dim3 vgrid(nvb, m.n_ticks), tgrid(ntb, m.n_ticks), block(kNmThreads);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (prof && timed_launch(prof)) {
        if (next_event_pair(prof, e0, e1)) return -1;
        prof->timed_kernel = "nm_face_kernel";
    }
    hipLaunchKernelGGL(nm_clear_kernel, vgrid, block, 0, s, a);
    if (e0) LSN_HIP(hipEventRecord(e0, s));
    hipLaunchKernelGGL(nm_face_kernel, tgrid, block, 0, s, a);
    if (e1) LSN_HIP(hipEventRecord(e1, s));
    hipLaunchKernelGGL(nm_finish_kernel, vgrid, block, 0, s, a);
    LSN_HIP(hipGetLastError());
    ns.cnt.finish(m.n_ticks);
    return 0;
}

// {used triangles, skipped triangles, zero normals} of one tick of the last call with `ns`; synchronises `s`.
int normals_counts(NormalsScratch &ns, const char *who, int tick, int *n_used, int *n_skipped, int *n_zero_normals, hipStream_t s)
{
    int c[4] = {0, 0, 0, 0};
    if (ns.cnt.read(who, "no normals have been computed yet", tick, 0, c, s,
                    [&] { lsn::set_error("%s: the last call had %d ticks (asked for tick %d)", who, ns.cnt.ticks, tick); }))
        return -1;
    if (n_used) *n_used = c[0];
    if (n_skipped) *n_skipped = c[1];
    if (n_zero_normals) *n_zero_normals = c[2];
    return 0;
}

}  // namespace lsn

extern "C" int lsnFusionNormals(LsnFusion *p, const void *d_vertices, const int *d_offsets, const void *d_triangles, const int *d_tri_offsets,
                                void *d_normals_out, void *stream)
{
    return plan_export("lsnFusionNormals", p, [&] {
        return lsn::normals(p->nm, "lsnFusionNormals", plan_batch(p, d_vertices, d_offsets, d_triangles, d_tri_offsets), d_normals_out, p,
                            lsn::as_stream(stream));
    });
}

extern "C" int lsnFusionNormalsDiagnostics(LsnFusion *p, int tick, int *n_used, int *n_skipped, int *n_zero_normals, void *stream)
{
    return plan_export("lsnFusionNormalsDiagnostics", p, [&] {
        return lsn::normals_counts(p->nm, "lsnFusionNormalsDiagnostics", tick, n_used, n_skipped, n_zero_normals, lsn::as_stream(stream));
    });
}
