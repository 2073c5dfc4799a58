// smooth.hip -- Taubin lambda|mu smoothing of a tick's merged mesh: lsnFusionSmooth, lsnFusionSmoothDiagnostics and what
// lsnLastMeshPlySmooth / lsnLastMeshTransferFrameSmooth run.
//
// The reference smooths nothing: the stage is DEFINED here (include/NativeUtils.h has the exact wording, tests/smooth_ref.py restates
// it).  One pass with factor f goes from positions P to P' and reads only P.  A triangle is USED iff its indices are in [0, nVertices),
// pairwise distinct, and the nine coordinates of its corners in P satisfy fabsf(c) < 4096 (NaN and inf fail).  q(c) = (int64) trunc(c *
// 2^32) (both steps exact); a used triangle adds the q of a corner's two other corners to that corner's three 64-bit integer sums S, two's
// complement with wrap-around, and 2 to its count N: integer addition is associative, so the sums -- and with them every byte of the
// output -- do not depend on the order in which the device takes the triangles.  N == 0 or a pinned vertex: P' = P bit for bit; else
// m = (float)(((double)S / (double)N) * 2^-32), d = m - p, p' = p + f * d, every f32 operation rounded on its own.  Open vertices come
// from the indices alone: H[a] += mix(next) - mix(previous) over the triangles that are in range and pairwise distinct, mix the
// splitmix64 finaliser; open iff H != 0; pinned in every pass when the caller asks.  Per call, over every tick (grid y = tick):
//
//   0. clear (sm_clear_kernel): one lane per counted vertex zeroes its sums, count, H and flag.
//   1. topology, only with pin_boundary (sm_topo_kernel): one lane per triangle, three no-return 64-bit atomicAdds into H; then
//      sm_flag_kernel, one lane per vertex: H -> the flag byte, the pinned vertices counted, one add per wave.
//   2. per pass, the scatter (sm_scatter_kernel): one lane per triangle, grid-stride, wave-uniform trip count.  12 B of indices, the
//      index test, three 16-byte gathers, the range test, then up to nine no-return 64-bit integer atomicAdds into the three PLANES
//      [3][capacity] of the tick (a wave that adds to consecutive vertices touches 512 contiguous bytes) and three 32-bit ones into N;
//      adds of 0 are skipped.  The last pass counts used and skipped triangles: one add per wave at the end.
//   3. per pass, the finish (sm_finish_kernel), a launch later: one lane per vertex, three i64 loads and the count, the arithmetic
//      above, one 16-byte store; it zeroes what it has read, so the next pass needs no clear launch.  The last pass counts the
//      vertices with N == 0.
//
// The positions go from the input to the scratch's own vertex buffer and d_vertices_out in turn, so that the last pass lands in
// d_vertices_out.  No kernel waits for another workgroup; every loop is bounded by a clipped count.  Plain vector stores and HIP atomics
// only.  Compiled as part of mesh.hip's translation unit (after mesh_batch.hip and normals.hip).
#include "fusion_shared.hpp"

namespace {

constexpr int kSmThreads = 256;
constexpr int kSmMaxBlocks = 8192;               // of the triangle passes per tick: 32 workgroups per CU, the rest is the grid-stride loop
constexpr float kSmLim = 4096.0f;                // a coordinate at or above it takes its triangles out
constexpr float kSmScale = 4294967296.0f;        // 2^32: the sums count 2^-32 m

struct SmArgs {
    lsn::MeshBatch m;              // the input (its vertices are read by the first pass only)
    const uint4 *src;              // [n_ticks][tick_vert]: P of this pass
    uint4 *dst;                    // [n_ticks][tick_vert]: P'
    unsigned long long *acc;       // [n_ticks][3][tick_vert]: the sums' bits (two's complement)
    unsigned int *num;             // [n_ticks][tick_vert]: N
    unsigned long long *hash;      // [n_ticks][tick_vert]: H
    unsigned char *flag;           // [n_ticks][tick_vert]: 1 = pinned
    int *cnt;                      // [n_ticks][4]: used, skipped (last pass), pinned, N == 0 (last pass)
    float f;                       // the pass's factor
    int last;                      // the pass that counts
};

__device__ __forceinline__ bool sm_valid(int i0, int i1, int i2, int nv)
{
    return (unsigned int)i0 < (unsigned int)nv && (unsigned int)i1 < (unsigned int)nv && (unsigned int)i2 < (unsigned int)nv && i0 != i1 &&
           i1 != i2 && i0 != i2;
}

// ---- 0. clear -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSmThreads) void sm_clear_kernel(SmArgs a)
{
    const int tick = blockIdx.y;
    const int nv = mesh_count(a.m.voff, tick, a.m.n, a.m.tick_vert);
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nv) return;
    unsigned long long *acc = a.acc + 3 * tick * a.m.tick_vert;
    acc[g] = 0;
    acc[a.m.tick_vert + g] = 0;
    acc[2 * a.m.tick_vert + g] = 0;
    a.num[tick * a.m.tick_vert + g] = 0;
    a.hash[tick * a.m.tick_vert + g] = 0;
    a.flag[tick * a.m.tick_vert + g] = 0;
}

// ---- 1. topology --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long sm_mix(int i)   // the splitmix64 finaliser of an index >= 0
{
    unsigned long long x = (unsigned long long)i + 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__global__ __launch_bounds__(kSmThreads) void sm_topo_kernel(SmArgs a)
{
    const int tick = blockIdx.y;
    const int nv = mesh_count(a.m.voff, tick, a.m.n, a.m.tick_vert), nt = mesh_count(a.m.toff, tick, a.m.n, a.m.tick_tri);
    const int *tri = a.m.tri + 3 * (tick * a.m.tick_tri);
    unsigned long long *hash = a.hash + tick * a.m.tick_vert;
    const int stride = gridDim.x * kSmThreads;                // <= kSmMaxBlocks x 256; nt <= 2^31 / 3: t + stride stays an int
    for (int t = blockIdx.x * kSmThreads + threadIdx.x; t < nt; t += stride) {
        const int i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];
        if (!sm_valid(i0, i1, i2, nv)) continue;
        const unsigned long long m0 = sm_mix(i0), m1 = sm_mix(i1), m2 = sm_mix(i2);   // distinct: mix is a bijection
        atomicAdd(&hash[i0], m1 - m2);                        // next - previous, in the triangle's own order; results unused
        atomicAdd(&hash[i1], m2 - m0);
        atomicAdd(&hash[i2], m0 - m1);
    }
}

__global__ __launch_bounds__(kSmThreads) void sm_flag_kernel(SmArgs a)
{
    const int tick = blockIdx.y;
    const int nv = mesh_count(a.m.voff, tick, a.m.n, a.m.tick_vert);
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    bool open = false;
    if (g < nv) {
        open = a.hash[tick * a.m.tick_vert + g] != 0;
        a.flag[tick * a.m.tick_vert + g] = open ? 1 : 0;
    }
    const int n_open = __popcll(__ballot(open));
    if ((threadIdx.x & 63) == 0 && n_open) atomicAdd(&a.cnt[tick * 4 + 2], n_open);
}

// ---- 2. scatter ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long sm_q(unsigned int bits)
{
    return (long long)__fmul_rn(__uint_as_float(bits), kSmScale);   // |c| < 2^12: the product is exact and below 2^44, the conversion truncates toward zero
}

__device__ __forceinline__ bool sm_fine(const uint4 &p)   // NaN and +-inf fail
{
    return fabsf(__uint_as_float(p.y)) < kSmLim && fabsf(__uint_as_float(p.z)) < kSmLim && fabsf(__uint_as_float(p.w)) < kSmLim;
}

// One component of a used triangle into the plane `acc`: each corner gets its two other corners (all indices below nVertices <= tick_vert).
__device__ __forceinline__ void sm_add(unsigned long long *acc, int i0, int i1, int i2, long long q0, long long q1, long long q2)
{
    const long long s0 = q1 + q2, s1 = q0 + q2, s2 = q0 + q1;
    if (s0) atomicAdd(&acc[i0], (unsigned long long)s0);      // result unused: no return value is asked of the memory system
    if (s1) atomicAdd(&acc[i1], (unsigned long long)s1);
    if (s2) atomicAdd(&acc[i2], (unsigned long long)s2);
}

__global__ __launch_bounds__(kSmThreads) void sm_scatter_kernel(SmArgs a)
{
    const int tick = blockIdx.y;
    const int nv = mesh_count(a.m.voff, tick, a.m.n, a.m.tick_vert), nt = mesh_count(a.m.toff, tick, a.m.n, a.m.tick_tri);
    const uint4 *verts = a.src + tick * a.m.tick_vert;
    const int *tri = a.m.tri + 3 * (tick * a.m.tick_tri);
    unsigned long long *acc = a.acc + 3 * tick * a.m.tick_vert;
    unsigned int *num = a.num + tick * a.m.tick_vert;
    const int lane = threadIdx.x & 63;
    const int stride = gridDim.x * kSmThreads;                // <= kSmMaxBlocks x 256; nt <= 2^31 / 3: base + stride stays an int
    int used = 0, skipped = 0;
    for (int base = blockIdx.x * kSmThreads + (threadIdx.x - lane); base < nt; base += stride) {   // the same trips for a wave's 64 lanes
        const int t = base + lane;
        bool ok = false;
        if (t < nt) {
            const int i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];
            if (sm_valid(i0, i1, i2, nv)) {
                const uint4 p0 = verts[i0], p1 = verts[i1], p2 = verts[i2];   // {colour, x, y, z}
                if (sm_fine(p0) && sm_fine(p1) && sm_fine(p2)) {
                    ok = true;
                    sm_add(acc, i0, i1, i2, sm_q(p0.y), sm_q(p1.y), sm_q(p2.y));
                    sm_add(acc + a.m.tick_vert, i0, i1, i2, sm_q(p0.z), sm_q(p1.z), sm_q(p2.z));
                    sm_add(acc + 2 * a.m.tick_vert, i0, i1, i2, sm_q(p0.w), sm_q(p1.w), sm_q(p2.w));
                    atomicAdd(&num[i0], 2u);
                    atomicAdd(&num[i1], 2u);
                    atomicAdd(&num[i2], 2u);
                }
            }
        }
        if (a.last) {
            used += __popcll(__ballot(ok));
            skipped += __popcll(__ballot(t < nt && !ok));
        }
    }
    if (lane == 0) {
        if (used) atomicAdd(&a.cnt[tick * 4], used);
        if (skipped) atomicAdd(&a.cnt[tick * 4 + 1], skipped);
    }
}

// ---- 3. finish ----------------------------------------------------------------------------------------------------------------------
// One component: the mean of the neighbours, then the step towards it.
__device__ __forceinline__ unsigned int sm_step(long long s, double n, unsigned int pbits, float f)
{
    const float p = __uint_as_float(pbits);
    const float m = (float)(((double)s / n) * 2.3283064365386962890625e-10);   // 2^-32: exact; one rounding each: s -> f64, the division, -> f32
    const float d = __fsub_rn(m, p);
    return __float_as_uint(__fadd_rn(p, __fmul_rn(f, d)));
}

__global__ __launch_bounds__(kSmThreads) void sm_finish_kernel(SmArgs a)
{
    const int tick = blockIdx.y;
    const int nv = mesh_count(a.m.voff, tick, a.m.n, a.m.tick_vert);
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    bool isolated = false;
    if (g < nv) {
        unsigned long long *acc = a.acc + 3 * tick * a.m.tick_vert;
        unsigned int *num = a.num + tick * a.m.tick_vert;
        const long long sx = (long long)acc[g], sy = (long long)acc[a.m.tick_vert + g], sz = (long long)acc[2 * a.m.tick_vert + g];
        const unsigned int n = num[g];
        uint4 p = a.src[tick * a.m.tick_vert + g];
        isolated = n == 0;
        if (n != 0) {
            acc[g] = 0;                                       // what the next pass adds into: no clear launch between the passes
            acc[a.m.tick_vert + g] = 0;                       // (against one per pass: EXPERIMENTS.md "Mesh smoothing")
            acc[2 * a.m.tick_vert + g] = 0;
            num[g] = 0;
            if (!a.flag[tick * a.m.tick_vert + g]) {
                const double dn = (double)n;
                p.y = sm_step(sx, dn, p.y, a.f);
                p.z = sm_step(sy, dn, p.z, a.f);
                p.w = sm_step(sz, dn, p.w, a.f);
            }
        }
        a.dst[tick * a.m.tick_vert + g] = p;                  // the colour word, and a vertex that stays, bit for bit
    }
    if (a.last) {
        const int n_iso = __popcll(__ballot(isolated));
        if ((threadIdx.x & 63) == 0 && n_iso) atomicAdd(&a.cnt[tick * 4 + 3], n_iso);
    }
}

}  // namespace

namespace lsn {

// The stage on a batch, with `ss` as its scratch.
int smooth(SmoothScratch &ss, const char *who, const MeshBatch &m, int iterations, float lambda, float mu, int pin_boundary, void *d_vertices_out,
           hipStream_t s)
{
    if (!m.verts || !m.voff || !m.toff || !d_vertices_out) {
        lsn::set_error("%s: null argument", who);
        return -1;
    }
    if (!m.tri) {
        lsn::set_error("%s: null argument (d_triangles: a bare point cloud has no neighbours to smooth with)", who);
        return -1;
    }
    if (!(iterations >= 1 && iterations <= 64)) {
        lsn::set_error("%s: iterations = %d is not in [1, 64]", who, iterations);
        return -1;
    }
    if (!(lambda > 0.0f && lambda <= 1.0f)) {   // NaN fails
        lsn::set_error("%s: lambda = %g is not in (0, 1]", who, (double)lambda);
        return -1;
    }
    if (!(mu >= -1.0f && mu <= 0.0f)) {
        lsn::set_error("%s: mu = %g is not in [-1, 0]", who, (double)mu);
        return -1;
    }
    if (check_batch(who, m)) return -1;
    const long long tick_vert = m.tick_vert, tick_tri = m.tick_tri;
    const size_t T = (size_t)m.n_ticks, V = T * (size_t)std::max(tick_vert, 1LL);
    if (check_out_of_place(who, m, {{d_vertices_out, 16 * (size_t)tick_vert * T, "d_vertices_out"}}, "the stage runs out of place")) return -1;
    const int passes = iterations * (mu == 0.0f ? 1 : 2);
    if (ss.cnt.begin(T, T, s) || ss.acc.reserve(24 * V) || ss.num.reserve(4 * V) || ss.hash.reserve(8 * V) || ss.flag.reserve(V) ||
        (passes > 1 && ss.verts.reserve(16 * V)))
        return -1;
    SmArgs a;
    a.m = m;
    a.src = m.verts;
    a.dst = nullptr;
    a.acc = ss.acc.as<unsigned long long>();
    a.num = ss.num.as<unsigned int>();
    a.hash = ss.hash.as<unsigned long long>();
    a.flag = ss.flag.as<unsigned char>();
    a.cnt = ss.cnt.buf.as<int>();
    a.f = 0.0f;
    a.last = 0;
    const int nvb = (int)std::max<long long>(1, (tick_vert + kSmThreads - 1) / kSmThreads);
    const int ntb = (int)std::min<long long>(kSmMaxBlocks, std::max<long long>(1, (tick_tri + kSmThreads - 1) / kSmThreads));
    const dim3 vgrid(nvb, m.n_ticks), tgrid(ntb, m.n_ticks), block(kSmThreads);
    hipLaunchKernelGGL(sm_clear_kernel, vgrid, block, 0, s, a);
    if (pin_boundary) {
        hipLaunchKernelGGL(sm_topo_kernel, tgrid, block, 0, s, a);
        hipLaunchKernelGGL(sm_flag_kernel, vgrid, block, 0, s, a);
    }
    uint4 *const out = static_cast<uint4 *>(d_vertices_out), *const own = ss.verts.as<uint4>();
    for (int k = 0; k < passes; ++k) {
        a.dst = (passes - 1 - k) % 2 == 0 ? out : own;        // the last pass lands in d_vertices_out
        a.f = mu == 0.0f || k % 2 == 0 ? lambda : mu;
        a.last = k == passes - 1;
        hipLaunchKernelGGL(sm_scatter_kernel, tgrid, block, 0, s, a);
        hipLaunchKernelGGL(sm_finish_kernel, vgrid, block, 0, s, a);
        a.src = a.dst;
    }
    LSN_HIP(hipGetLastError());
    ss.cnt.finish(m.n_ticks);
    return 0;
}

// {used triangles, skipped triangles (both of the last pass), pinned vertices, vertices with N == 0 in the last pass} of one tick of
// the last call with `ss`; synchronises `s`.
int smooth_counts(SmoothScratch &ss, const char *who, int tick, int *n_used, int *n_skipped, int *n_pinned, int *n_isolated, hipStream_t s)
{
    int c[4] = {0, 0, 0, 0};
    if (ss.cnt.read(who, "nothing has been smoothed yet", tick, 0, c, s,
                    [&] { lsn::set_error("%s: the last call had %d ticks (asked for tick %d)", who, ss.cnt.ticks, tick); }))
        return -1;
    if (n_used) *n_used = c[0];
    if (n_skipped) *n_skipped = c[1];
    if (n_pinned) *n_pinned = c[2];
    if (n_isolated) *n_isolated = c[3];
    return 0;
}

}  // namespace lsn

extern "C" int lsnFusionSmooth(LsnFusion *p, int iterations, float lambda, float mu, int pin_boundary, const void *d_vertices, const int *d_offsets,
                               const void *d_triangles, const int *d_tri_offsets, void *d_vertices_out, void *stream)
{
    return plan_export("lsnFusionSmooth", p, [&] {
        return lsn::smooth(p->sm, "lsnFusionSmooth", plan_batch(p, d_vertices, d_offsets, d_triangles, d_tri_offsets), iterations, lambda, mu,
                           pin_boundary, d_vertices_out, lsn::as_stream(stream));
    });
}

extern "C" int lsnFusionSmoothDiagnostics(LsnFusion *p, int tick, int *n_used, int *n_skipped, int *n_pinned, int *n_isolated, void *stream)
{
    return plan_export("lsnFusionSmoothDiagnostics", p, [&] {
        return lsn::smooth_counts(p->sm, "lsnFusionSmoothDiagnostics", tick, n_used, n_skipped, n_pinned, n_isolated, lsn::as_stream(stream));
    });
}
