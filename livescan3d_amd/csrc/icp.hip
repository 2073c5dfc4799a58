// icp.hip -- device-resident ICP for gfx950, replacing src/NativeUtils/icp.cpp:18-177: the ICP step and the workspace.  One translation
// unit of four files: this one includes icp_grid.hip (the voxel grid), icp_nn.hip (the exact nearest-neighbour step and the one-to-one claim;
// behind IcpState and LsnIcp, which it uses) and, at its end, refine.hip (the refine pass, which calls icp_run and rotate_normals_kernel).
//
// The reference (per iteration): nanoflann kd-tree over the target rebuilt every iteration + OpenMP queries
// (icp.cpp:18-32), a sequential one-to-one matching scan (:95-126), 2.5-sigma rejection on squared distances
// (:34-73,:128), and an uncentred Kabsch step through OpenCV (mean difference, 3x3 SVD, apply; :138-168).
//
// Here (everything stays in HBM, no host synchronisation inside the iteration loop):
//   * exact nearest neighbour and one-to-one matching -- icp_nn.hip, over a grid built ONCE per call (icp_grid.hip).
//   * statistics / Kabsch sums -- wavefront shuffle reductions -> LDS -> one partial per workgroup, combined in a
//     fixed order in double over the queries' ORIGINAL order (deterministic, run-to-run bit-identical, independent of
//     the sort).  The accumulators are count, sum(d), sum(d^2), sum(m1), sum(m2), sum(m2 m1^T): the reference's
//     solver is closed-form Kabsch, not a 6x6 normal matrix.
//   * 3x3 SVD -- one-sided Jacobi in double in a single-thread kernel (U*Vt is the polar factor of M: independent
//     of the SVD algorithm up to rounding), then the same f32 products, det test and updates as icp.cpp:155-168.
//   * apply -- the translate+rotate of the source cloud in the reference's f32 operation order rides in the first
//     kernel of the next iteration's NN step (one separate pass after the last iteration).
//   * point-to-plane step (lsnIcpRunPlane; no counterpart in the reference, defined in tests/icp_plane_ref.py) -- the same NN, matching,
//     statistics and rejection; then the 6x6 normal equations of r = (b - a) . n over the kept matches with a usable target normal, summed
//     in double like the Kabsch sums, an eigen-solve by cyclic Jacobi in the single-thread kernel with the weakly determined modes left
//     alone, and the same apply and pose update (accum_plane_kernel, solve_plane_kernel).  Compiled with -ffp-contract=off.
#include "icp_grid.hip"   // (with lsn_common.hpp, wave_ops.hpp, <algorithm> and <array>)

#include <climits>
#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>
#include <vector>

namespace {

// v M for a row vector v = (x, y, z) and a row-major 3x3 M in f32, one rounding per operation, in the association (x m0 + y m3) + z m6 of
// icp.cpp:165.  Written once: the fused apply (nn_cull_kernel<true>), apply_kernel and rotate_normals_kernel must agree to the bit.
__device__ __forceinline__ void rows_times(float x, float y, float z, const float *M, float &ox, float &oy, float &oz)
{
    ox = x * M[0] + y * M[3] + z * M[6];
    oy = x * M[1] + y * M[4] + z * M[7];
    oz = x * M[2] + y * M[5] + z * M[8];
}

// per-iteration device state
struct IcpState {
    float T[3];
    float Rn[9];
    float mean, stddev, thresh;
    int m, mk;
    // warm start of the next iteration's Jacobi SVD: the right singular vectors of this iteration's cross-covariance (the
    // clouds barely move between iterations, so the next matrix is almost diagonalised by them); v_valid is cleared at the
    // start of every lsnIcpRun, which keeps a call's result independent of what the workspace ran before
    int v_valid;
    // the next seeded NN step takes the near path: set by accum_kernel when at least half of this step's queries lie within one
    // target cell edge of their neighbour (below that the walk costs the step more than the shorter group search gives back:
    // configs[1], 18 % settled, +6 us per iteration; configs[2], 98 %, -26 us).  A matter of speed only: the results are the same bits.
    int near_next;
    double Vprev[9];
};

}  // namespace

struct LsnIcp {
    int device = 0;
    int max_n1 = 0, max_n2 = 0;
    GridBufs tgt, src;    // tgt: cell-sorted target + boxes; src.sorted: the spatially sorted working copy of the source
    lsn::DevBuf bbox_part, block_sums;
    lsn::DevBuf idx, dist, keys, counters, part1, part3, state, trace;
    lsn::DevBuf best_key, groups, list_a, list_b, idx_sorted;   // the NN step's per-query keys, per-group boxes and work lists
    int seg_a = 0, seg_b = 0;   // capacity of one list segment
    // optional phase timing of lsnIcpRun (lsnIcpSetProfiling): HIP events on the caller's stream around
    // [0] grid build + source sort, [1] the NN steps (incl. the fused apply), [2] statistics + Kabsch sums + solve, [3] final apply
    bool profiling = false;
    std::vector<hipEvent_t> events;
    std::vector<int> event_phase;   // phase that ENDS at event k (event 0 opens the run)
    size_t n_events = 0;
    int trace_iters = 0;
    int near_mode = 1;     // $LSN_ICP_NEAR: 0 = no near path, 1 = the probe always, seeded steps when the previous step's distances say it pays, 2 = always
    int near_pts = 128;    // the near path's candidate cap per query (<= kNearCapMax); $LSN_ICP_NEAR=0 turns the path off (A/B, tests), $LSN_ICP_NEAR_PTS sets the cap
    int last_groups = 0;   // query groups of the last grid NN step (lsnIcpNearResolved)
    std::mutex mu;
    std::array<lsn::DevBuf *, 15> bufs() { return {&bbox_part, &block_sums, &idx, &dist, &keys, &counters, &part1, &part3, &state, &trace, &best_key, &groups, &list_a, &list_b, &idx_sorted}; }
    size_t bytes() { return bytes_of(tgt.bufs()) + bytes_of(src.bufs()) + bytes_of(bufs()); }   // device memory the workspace holds (lsnRefineRelease reports it)
};

static constexpr int kTraceCap = 1024;

#include "icp_nn.hip"

namespace {

// Sums NV doubles per thread over the workgroup (4 waves) into out[] (valid in every thread).
template <int NV>
__device__ __forceinline__ void block_sum_d(double (&v)[NV], double *lds /* [4*NV] */)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; i++) {
        double s = wave_sum(v[i]);
        if (lane == 0) lds[wave * NV + i] = s;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; i++) v[i] = (lds[i] + lds[NV + i]) + (lds[2 * NV + i] + lds[3 * NV + i]);
    __syncthreads();
}

// Deterministic sum of n_parts partial vectors (stride NVP, a power of two >= NV) by one workgroup; result valid in every
// thread.  Thread t sums component t % NVP of the partials t / NVP, t / NVP + G, ... (G = kThreads / NVP groups; NVP
// consecutive threads read one partial: coalesced, all loads independent), the G group sums meet in LDS and thread c adds
// those of component c in a fixed order.  (One partial vector per thread and a shuffle tree over 16 doubles took 5.8 us in
// solve_kernel and in EVERY workgroup of accum_kernel: strided loads, 192 dependent cross-lane moves.)
template <int NV, int NVP>
__device__ __forceinline__ void reduce_partials(const double *parts, int n_parts, double (&out)[NV], double *lds /* [kThreads + NVP] */)
{
    constexpr int G = kThreads / NVP;
    const int c = threadIdx.x & (NVP - 1), g = threadIdx.x / NVP;
    // eight loads in flight per thread (a plain loop would wait for each load before issuing the next: n_parts / G round trips)
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0, a6 = 0, a7 = 0;
    int p = g;
    for (; p + 7 * G < n_parts; p += 8 * G) {
        const double v0 = parts[(size_t)p * NVP + c], v1 = parts[(size_t)(p + G) * NVP + c], v2 = parts[(size_t)(p + 2 * G) * NVP + c],
                     v3 = parts[(size_t)(p + 3 * G) * NVP + c], v4 = parts[(size_t)(p + 4 * G) * NVP + c], v5 = parts[(size_t)(p + 5 * G) * NVP + c],
                     v6 = parts[(size_t)(p + 6 * G) * NVP + c], v7 = parts[(size_t)(p + 7 * G) * NVP + c];
        a0 += v0; a1 += v1; a2 += v2; a3 += v3; a4 += v4; a5 += v5; a6 += v6; a7 += v7;
    }
    {   // the tail, predicated: still eight independent loads
        const double v0 = p < n_parts ? parts[(size_t)p * NVP + c] : 0.0, v1 = p + G < n_parts ? parts[(size_t)(p + G) * NVP + c] : 0.0;
        const double v2 = p + 2 * G < n_parts ? parts[(size_t)(p + 2 * G) * NVP + c] : 0.0, v3 = p + 3 * G < n_parts ? parts[(size_t)(p + 3 * G) * NVP + c] : 0.0;
        const double v4 = p + 4 * G < n_parts ? parts[(size_t)(p + 4 * G) * NVP + c] : 0.0, v5 = p + 5 * G < n_parts ? parts[(size_t)(p + 5 * G) * NVP + c] : 0.0;
        const double v6 = p + 6 * G < n_parts ? parts[(size_t)(p + 6 * G) * NVP + c] : 0.0;
        a0 += v0; a1 += v1; a2 += v2; a3 += v3; a4 += v4; a5 += v5; a6 += v6;
    }
    const double acc = ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7));
    lds[threadIdx.x] = acc;  // [g][c]
    __syncthreads();
    if (threadIdx.x < NVP) {
        double t = 0;
        for (int k = 0; k < G; k++) t += lds[k * NVP + threadIdx.x];
        lds[kThreads + threadIdx.x] = t;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; i++) out[i] = lds[kThreads + i];
    __syncthreads();
}

// ---- matching statistics and Kabsch sums ----------------------------------------------------------------------

__device__ __forceinline__ bool is_winner(const unsigned long long *keys, const int *idx, int i) { return claim_source(keys[idx[i]]) == i; }

// Thread k stores component k of v[] (valid in every thread, block_sum_d) into the workgroup's slot of STRIDE partials (zero from NV up).
template <int NV, int STRIDE>
__device__ __forceinline__ void store_partials(const double (&v)[NV], double *part)
{
    if (threadIdx.x < STRIDE) {
        double out = 0;
#pragma unroll
        for (int k = 0; k < NV; k++)
            if (threadIdx.x == k) out = v[k];
        part[blockIdx.x * STRIDE + threadIdx.x] = out;
    }
}

// The head of both accumulate loops: query i is a kept match when it won its target's claim and its squared distance is not above the
// rejection threshold; then body(k, a, b) gets the target k and the target's and the query's points as doubles.
template <class Body>
__device__ __forceinline__ void kept_match(const float *verts1, const float *verts2, const int *idx, const float *dist, const unsigned long long *keys,
                                           int i, float thresh, Body &&body)
{
    if (!is_winner(keys, idx, i)) return;
    if (dist[i] > thresh) return;  // NaN distances are kept, like the reference's comparison
    const int k = idx[i];
    const double a[3] = {verts1[3 * (size_t)k], verts1[3 * (size_t)k + 1], verts1[3 * (size_t)k + 2]};
    const double b[3] = {verts2[3 * (size_t)i], verts2[3 * (size_t)i + 1], verts2[3 * (size_t)i + 2]};
    body(k, a, b);
}

// pass 1: m = number of one-to-one matches, the sum of their squared distances and the sum of the squares of those
// (fourth sum, for the next step's choice of path: the queries within one target cell edge of their neighbour; gp null: brute force)
__global__ __launch_bounds__(kThreads) void stats_kernel(const int *idx, const float *dist, const unsigned long long *keys, int n2,
                                                         const GridParams *gp, double *part /* [blocks][4]: count, sum d, sum d^2, near */)
{
    __shared__ double lds[4 * 4];
    const float h2 = gp ? gp->h * gp->h : -1.0f;
    double v[4] = {0, 0, 0, 0};
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n2; i += gridDim.x * kThreads) {
        const float df = dist[i];
        if (df <= h2) v[3] += 1.0;
        if (is_winner(keys, idx, i)) {
            const double d = (double)df;
            v[0] += 1.0;
            v[1] += d;
            v[2] += d * d;
        }
    }
    block_sum_d<4>(v, lds);
    store_partials<4, 4>(v, part);
}

// The front half of pass 2, shared by both residuals: mean and standard deviation of the matches' squared distances from pass 1's partials
// (GetStandardDeviation, icp.cpp:34-54: the mean is rounded to f32, the deviations are taken from that f32 mean, the sum is kept in a
// float and divided by the count) and the rejection threshold 2.5*std (icp.cpp:56-73), in every thread; the first thread of the launch
// leaves them in st.  sum (d - mean)^2 = sum d^2 - 2 mean sum d + m mean^2 is evaluated in double from pass 1's three sums (mean = the
// f32 value): one pass over the matches instead of two; the cancellation costs ~1e-15 relative, far below the f32 result.
__device__ __forceinline__ float rejection_threshold(const double *part1, int n_part1, int n2, IcpState *st, double *red /* [kThreads + 4] */)
{
    double s1[4];
    reduce_partials<4, 4>(part1, n_part1, s1, red);
    const float mean = (float)(s1[1] / s1[0]);
    const float m_f = (float)(int)s1[0];
    const double dev = s1[2] - 2.0 * (double)mean * s1[1] + s1[0] * (double)mean * (double)mean;
    float sd = (float)(dev > 0.0 ? dev : 0.0);  // the reference keeps the running sum in a float
    sd = sd / m_f;
    sd = sqrtf(sd);
    const float thresh = 2.5f * sd;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->m = (int)s1[0];
        st->mean = mean;
        st->stddev = sd;
        st->thresh = thresh;
        st->near_next = 2.0 * s1[3] >= (double)n2;
    }
    return thresh;
}

// pass 2 of the point-to-point step: reject d > 2.5*std, accumulate count, sum m1, sum m2, sum m2 m1^T over the kept matches.
__global__ __launch_bounds__(kThreads) void accum_kernel(const float *verts1, const float *verts2, const int *idx, const float *dist,
                                                         const unsigned long long *keys, int n2, const double *part1, int n_part1,
                                                         double *part /* [blocks][16] */, IcpState *st)
{
    __shared__ double lds[4 * 16];
    __shared__ double red[kThreads + 4];
    const float thresh = rejection_threshold(part1, n_part1, n2, st, red);
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; k++) v[k] = 0;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n2; i += gridDim.x * kThreads) {
        kept_match(verts1, verts2, idx, dist, keys, i, thresh, [&](int, const double (&a)[3], const double (&b)[3]) {
            v[0] += 1.0;
            v[1] += a[0]; v[2] += a[1]; v[3] += a[2];
            v[4] += b[0]; v[5] += b[1]; v[6] += b[2];
            v[7] += b[0] * a[0]; v[8] += b[0] * a[1]; v[9] += b[0] * a[2];
            v[10] += b[1] * a[0]; v[11] += b[1] * a[1]; v[12] += b[1] * a[2];
            v[13] += b[2] * a[0]; v[14] += b[2] * a[1]; v[15] += b[2] * a[2];
        });
    }
    block_sum_d<16>(v, lds);
    store_partials<16, 16>(v, part);
}

// pass 2 of the point-to-plane step (lsnIcpRunPlane; defined in tests/icp_plane_ref.py): accum_kernel's front half
// (rejection_threshold: the same mean, sigma and threshold from pass 1's partials, the same bits in st), then, over the kept matches whose
// target normal is usable (finite, (nx nx + ny ny) + nz nz > 0 in f32), the 28 sums of the 6x6 normal equations: the count, the 21
// distinct sums of A = sum J J^T (row-major upper triangle) and the 6 of g = sum J r, with r = (b - a) . n and J = [b x n, n] in
// double.  A product of two f32 values is exact in double, so every term has one value in any IEEE double arithmetic; the sums are
// reduced without atomics in a fixed order: a run's bits repeat.  The partials' stride is kPlaneStride (reduce_partials takes a
// power of two); the four spare components are written as zero.
constexpr int kPlaneSums = 28, kPlaneStride = 32;
__global__ __launch_bounds__(kThreads) void accum_plane_kernel(const float *verts1, const float *normals1, const float *verts2, const int *idx,
                                                               const float *dist, const unsigned long long *keys, int n2, const double *part1,
                                                               int n_part1, double *part /* [blocks][kPlaneStride] */, IcpState *st)
{
    __shared__ double lds[4 * kPlaneSums];
    __shared__ double red[kThreads + 4];
    const float thresh = rejection_threshold(part1, n_part1, n2, st, red);
    double v[kPlaneSums];
#pragma unroll
    for (int k = 0; k < kPlaneSums; k++) v[k] = 0;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n2; i += gridDim.x * kThreads) {
        kept_match(verts1, verts2, idx, dist, keys, i, thresh, [&](int k, const double (&a)[3], const double (&b)[3]) {
            const float nx = normals1[3 * (size_t)k], ny = normals1[3 * (size_t)k + 1], nz = normals1[3 * (size_t)k + 2];
            if (!finite3(nx, ny, nz) || !(nx * nx + ny * ny + nz * nz > 0.0f)) return;   // (nx nx + ny ny) + nz nz, contraction is off
            const double b0 = b[0], b1 = b[1], b2 = b[2], n0 = nx, n1 = ny, n2d = nz;
            const double d0 = b0 - a[0], d1 = b1 - a[1], d2 = b2 - a[2];
            const double r = (d0 * n0 + d1 * n1) + d2 * n2d;
            const double J[6] = {b1 * n2d - b2 * n1, b2 * n0 - b0 * n2d, b0 * n1 - b1 * n0, n0, n1, n2d};
            v[0] += 1.0;
            int c = 1;
#pragma unroll
            for (int p = 0; p < 6; p++)
#pragma unroll
                for (int q = p; q < 6; q++) v[c++] += J[p] * J[q];
#pragma unroll
            for (int p = 0; p < 6; p++) v[22 + p] += J[p] * r;
        });
    }
    block_sum_d<kPlaneSums>(v, lds);
    store_partials<kPlaneSums, kPlaneStride>(v, part);
}

// 3x3 SVD by one-sided Jacobi (double).  A = U diag(w) V^T, singular values sorted descending.
// V0 (nullable): an orthonormal matrix to start from (B = A V0): any orthonormal start gives the same decomposition up to
// rounding; a good one saves sweeps.
__device__ void svd3(const double A[9], double U[9], double w[3], double V[9], const double *V0)
{
    double B[9];
    for (int i = 0; i < 9; i++) { B[i] = A[i]; V[i] = (i % 4 == 0) ? 1.0 : 0.0; }
    if (V0) {
        for (int i = 0; i < 9; i++) V[i] = V0[i];
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) B[3 * r + c] = A[3 * r] * V0[c] + A[3 * r + 1] * V0[3 + c] + A[3 * r + 2] * V0[6 + c];
    }
    for (int sweep = 0; sweep < 60; sweep++) {
        int rotations = 0;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                double a = 0, b = 0, c = 0;
                for (int k = 0; k < 3; k++) {
                    a += B[3 * k + p] * B[3 * k + p];
                    b += B[3 * k + q] * B[3 * k + q];
                    c += B[3 * k + p] * B[3 * k + q];
                }
                if (fabs(c) <= 1e-300 || c * c <= 1e-32 * (a * b)) continue;  // columns already orthogonal to ~1e-16
                rotations++;
                // tan of the rotation: sign(zeta) / (|zeta| + sqrt(1 + zeta^2)) with zeta = (b - a) / (2c), multiplied through
                // by 2|c| -- one division and one square root per rotation instead of three and two (this thread is the
                // critical path of an ICP iteration)
                const double ba = b - a;
                const double tt = ((ba >= 0) == (c >= 0) ? 2.0 : -2.0) * fabs(c) / (fabs(ba) + sqrt(ba * ba + 4.0 * c * c));
                const double cs = rsqrt(1.0 + tt * tt), sn = cs * tt;
                for (int k = 0; k < 3; k++) {
                    const double bp = B[3 * k + p], bq = B[3 * k + q];
                    B[3 * k + p] = cs * bp - sn * bq;
                    B[3 * k + q] = sn * bp + cs * bq;
                    const double vp = V[3 * k + p], vq = V[3 * k + q];
                    V[3 * k + p] = cs * vp - sn * vq;
                    V[3 * k + q] = sn * vp + cs * vq;
                }
            }
        if (rotations == 0) break;
    }
    for (int j = 0; j < 3; j++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += B[3 * k + j] * B[3 * k + j];
        w[j] = sqrt(s);
    }
    int ord[3] = {0, 1, 2};
    for (int i = 0; i < 2; i++)
        for (int j = i + 1; j < 3; j++)
            if (w[ord[j]] > w[ord[i]]) { int t = ord[i]; ord[i] = ord[j]; ord[j] = t; }
    double Bs[9], Vs[9], ws[3];
    for (int j = 0; j < 3; j++) {
        ws[j] = w[ord[j]];
        for (int k = 0; k < 3; k++) { Bs[3 * k + j] = B[3 * k + ord[j]]; Vs[3 * k + j] = V[3 * k + ord[j]]; }
    }
    for (int i = 0; i < 9; i++) V[i] = Vs[i];
    for (int j = 0; j < 3; j++) w[j] = ws[j];
    for (int j = 0; j < 3; j++) {
        const double inv = (w[j] > 1e-300) ? 1.0 / w[j] : 0.0;
        for (int k = 0; k < 3; k++) U[3 * k + j] = Bs[3 * k + j] * inv;
    }
    if (!(w[0] > 1e-300)) {
        for (int i = 0; i < 9; i++) U[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    if (!(w[1] > 1e-12 * w[0])) {
        const double u0[3] = {U[0], U[3], U[6]};
        int m = 0;
        if (fabs(u0[1]) < fabs(u0[m])) m = 1;
        if (fabs(u0[2]) < fabs(u0[m])) m = 2;
        double e[3] = {0, 0, 0};
        e[m] = 1;
        const double d = u0[m];
        const double v[3] = {e[0] - d * u0[0], e[1] - d * u0[1], e[2] - d * u0[2]};
        const double nv = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        U[1] = v[0] / nv; U[4] = v[1] / nv; U[7] = v[2] / nv;
    }
    if (!(w[2] > 1e-12 * w[0])) {
        const double a0 = U[0], a1 = U[3], a2 = U[6], b0 = U[1], b1 = U[4], b2 = U[7];
        const double c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;
        const double detV = V[0] * (V[4] * V[8] - V[5] * V[7]) - V[1] * (V[3] * V[8] - V[5] * V[6]) + V[2] * (V[3] * V[7] - V[4] * V[6]);
        const double s = detV < 0 ? -1.0 : 1.0;
        U[2] = s * c0; U[5] = s * c1; U[8] = s * c2;
    }
}

// What a step's solve ends with, whichever residual it minimised (icp.cpp:167-168): with mk > 0 the pose update matT += tempT * matR.t()
// (R before the update), matR = matR * tempR in f32; then the motion for the next launch's apply and the trace record.
__device__ __forceinline__ void commit_step(const float (&T)[3], const float (&Rn)[9], int mk, float *R, float *t, IcpState *st, float *trace, int iter)
{
    st->mk = mk;
    if (mk > 0) {
        float add[3];
        for (int c = 0; c < 3; c++) add[c] = T[0] * R[3 * c] + T[1] * R[3 * c + 1] + T[2] * R[3 * c + 2];
        for (int c = 0; c < 3; c++) t[c] += add[c];
        float Rnew[9];
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) Rnew[3 * r + c] = R[3 * r] * Rn[c] + R[3 * r + 1] * Rn[3 + c] + R[3 * r + 2] * Rn[6 + c];
        for (int k = 0; k < 9; k++) R[k] = Rnew[k];
    }
    for (int c = 0; c < 3; c++) st->T[c] = T[c];
    for (int k = 0; k < 9; k++) st->Rn[k] = Rn[k];
    if (trace) {
        float *tr = trace + 16 * iter;
        tr[0] = (float)st->m;
        tr[1] = (float)mk;
        tr[2] = st->mean;
        tr[3] = st->stddev;
        for (int c = 0; c < 3; c++) tr[4 + c] = T[c];
        for (int k = 0; k < 9; k++) tr[7 + k] = Rn[k];
    }
}

// icp.cpp:141 (T), :152-163 (M, SVD, tempR), :167-168 (t, R update).  One workgroup; thread 0 does the 3x3 work.
__global__ __launch_bounds__(kThreads) void solve_kernel(const double *part3, int n_part3, float *R, float *t, IcpState *st, float *trace,
                                                         int iter)
{
    __shared__ double red[kThreads + 16];
    double s[16];
    reduce_partials<16, 16>(part3, n_part3, s, red);
    if (threadIdx.x != 0) return;
    const int mk = (int)s[0];
    float T[3] = {0, 0, 0};
    float Rn[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (mk > 0) {
        // T = mean(m1 - m2); M = sum (m2 + T) m1^T = sum m2 m1^T + T (sum m1)^T
        for (int c = 0; c < 3; c++) T[c] = (float)((s[1 + c] - s[4 + c]) / (double)mk);
        double M[9];
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) M[3 * a + b] = (double)(float)(s[7 + 3 * a + b] + (double)T[a] * s[1 + b]);
        double U[9], w[3], V[9];
        svd3(M, U, w, V, st->v_valid == 1 ? st->Vprev : nullptr);
        for (int i = 0; i < 9; i++) st->Vprev[i] = V[i];
        st->v_valid = 1;
        float Uf[9], Vtf[9];
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) {
                Uf[3 * r + c] = (float)U[3 * r + c];
                Vtf[3 * r + c] = (float)V[3 * c + r];
            }
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) Rn[3 * r + c] = Uf[3 * r] * Vtf[c] + Uf[3 * r + 1] * Vtf[3 + c] + Uf[3 * r + 2] * Vtf[6 + c];
        const double det = (double)Rn[0] * ((double)Rn[4] * Rn[8] - (double)Rn[5] * Rn[7]) -
                           (double)Rn[1] * ((double)Rn[3] * Rn[8] - (double)Rn[5] * Rn[6]) +
                           (double)Rn[2] * ((double)Rn[3] * Rn[7] - (double)Rn[4] * Rn[6]);
        if (det < 0) {
            for (int r = 0; r < 3; r++) Uf[3 * r + 2] = -Uf[3 * r + 2];
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) Rn[3 * r + c] = Uf[3 * r] * Vtf[c] + Uf[3 * r + 1] * Vtf[3 + c] + Uf[3 * r + 2] * Vtf[6 + c];
        }
    }
    commit_step(T, Rn, mk, R, t, st, trace, iter);
}

// A (6x6 symmetric, both halves filled) = V diag(a_ii) V^T on return, by cyclic Jacobi rotations in double; the eigenvectors are V's columns.
// Every index is a compile-time constant once the pair loops are unrolled, so a and V live in registers (no scratch).  A pair is passed
// over when its off-diagonal element is below 1e-16 of the geometric mean of its diagonal elements, or below 2^-70 of A's trace: the
// second floor ends the sweeps on the exact zero modes of a singular A (a wall, two walls), whose diagonal elements are rounding noise,
// and sits far below the 2^-20 lambda_max cutoff the eigenvalues are compared with.
__device__ __forceinline__ void eig6(double (&a)[6][6], double (&V)[6][6])
{
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) V[i][j] = i == j ? 1.0 : 0.0;
    const double floor_abs = 0x1p-70 * (((a[0][0] + a[1][1]) + (a[2][2] + a[3][3])) + (a[4][4] + a[5][5]));
    for (int sweep = 0; sweep < 30; sweep++) {
        int rotations = 0;
#pragma unroll
        for (int p = 0; p < 5; p++)
#pragma unroll
            for (int q = p + 1; q < 6; q++) {
                const double apq = a[p][q];
                if (fabs(apq) <= floor_abs || apq * apq <= 1e-32 * fabs(a[p][p] * a[q][q])) continue;
                rotations++;
                // tan of the rotation as in svd3: one division and one square root
                const double ba = a[q][q] - a[p][p];
                const double tt = ((ba >= 0) == (apq >= 0) ? 2.0 : -2.0) * fabs(apq) / (fabs(ba) + sqrt(ba * ba + 4.0 * apq * apq));
                const double cs = rsqrt(1.0 + tt * tt), sn = cs * tt;
                a[p][p] -= tt * apq;
                a[q][q] += tt * apq;
                a[p][q] = a[q][p] = 0.0;
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    if (k != p && k != q) {
                        const double akp = a[k][p], akq = a[k][q];
                        a[k][p] = a[p][k] = cs * akp - sn * akq;
                        a[k][q] = a[q][k] = sn * akp + cs * akq;
                    }
                    const double vp = V[k][p], vq = V[k][q];
                    V[k][p] = cs * vp - sn * vq;
                    V[k][q] = sn * vp + cs * vq;
                }
            }
        if (rotations == 0) break;
    }
}

// The point-to-plane solve (tests/icp_plane_ref.py steps 4-6): A x = -g by pseudo-inverse over A's eigen-decomposition -- a mode whose
// eigenvalue is <= 2^-20 lambda_max is unconstrained and gets zero step --, x = (omega, tau), Rinc = exp([omega]x) by Rodrigues in double
// (series for sin th / th and (1 - cos th) / th^2 below th = 2^-10), Rn = Rinc^T and T = Rinc^T tau rounded once to f32, and solve_kernel's
// pose update.  One workgroup; thread 0 does the 6x6 work.
__global__ __launch_bounds__(kThreads) void solve_plane_kernel(const double *part3, int n_part3, float *R, float *t, IcpState *st, float *trace,
                                                               int iter)
{
    __shared__ double red[kThreads + kPlaneStride];
    double s[kPlaneSums];
    reduce_partials<kPlaneSums, kPlaneStride>(part3, n_part3, s, red);
    if (threadIdx.x != 0) return;
    const int mk = (int)s[0];
    float T[3] = {0, 0, 0};
    float Rn[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (mk > 0) {
        double a[6][6], V[6][6];
        {
            int c = 1;
#pragma unroll
            for (int p = 0; p < 6; p++)
#pragma unroll
                for (int q = p; q < 6; q++) a[p][q] = a[q][p] = s[c++];
        }
        eig6(a, V);
        double lmax = a[0][0];
#pragma unroll
        for (int i = 1; i < 6; i++) lmax = a[i][i] > lmax ? a[i][i] : lmax;
        if (lmax > 0.0) {
            double x[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < 6; i++) {
                if (!(a[i][i] > 0x1p-20 * lmax)) continue;
                double c = 0;
#pragma unroll
                for (int k = 0; k < 6; k++) c += V[k][i] * s[22 + k];
                c = -c / a[i][i];
#pragma unroll
                for (int k = 0; k < 6; k++) x[k] += V[k][i] * c;
            }
            const double t2 = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
            const double th = sqrt(t2);
            double sc, cc;
            if (th < 0x1p-10) {
                sc = 1.0 - t2 / 6.0 * (1.0 - t2 / 20.0 * (1.0 - t2 / 42.0));
                cc = 0.5 - t2 / 24.0 * (1.0 - t2 / 30.0 * (1.0 - t2 / 56.0));
            } else {
                sc = sin(th) / th;
                cc = (1.0 - cos(th)) / t2;
            }
            // Rinc = I + sc K + cc K^2, K = [omega]x, K^2 = omega omega^T - |omega|^2 I
            double Ri[9];
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) Ri[3 * r + c] = cc * (x[r] * x[c] - (r == c ? t2 : 0.0)) + (r == c ? 1.0 : 0.0);
            Ri[1] -= sc * x[2]; Ri[2] += sc * x[1];
            Ri[3] += sc * x[2]; Ri[5] -= sc * x[0];
            Ri[6] -= sc * x[1]; Ri[7] += sc * x[0];
            for (int r = 0; r < 3; r++) {
                T[r] = (float)((Ri[r] * x[3] + Ri[3 + r] * x[4]) + Ri[6 + r] * x[5]);   // T = Rinc^T tau
                for (int c = 0; c < 3; c++) Rn[3 * r + c] = (float)Ri[3 * c + r];        // Rn = Rinc^T
            }
        }
    }
    commit_step(T, Rn, mk, R, t, st, trace, iter);
}

// icp.cpp:143-146 + :165: v = (v + T) * Rn, row vectors, f32, one rounding per operation.  Thread j moves query j of the
// sorted working copy and stores the same three floats into the caller's array at the query's original position; the
// same launch clears the match keys for the next iteration's atomicMin.
__global__ __launch_bounds__(kThreads) void apply_kernel(float4 *src, float *verts2, int n2, const IcpState *st, unsigned long long *keys,
                                                         int n_keys)
{
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j < n_keys) keys[j] = ~0ull;
    if (st->mk <= 0) return;
    const float T0 = st->T[0], T1 = st->T[1], T2 = st->T[2];
    const float Rn[9] = {st->Rn[0], st->Rn[1], st->Rn[2], st->Rn[3], st->Rn[4], st->Rn[5], st->Rn[6], st->Rn[7], st->Rn[8]};
    if (j >= n2) return;
    float4 q = src[j];
    const float x = q.x + T0, y = q.y + T1, z = q.z + T2;
    rows_times(x, y, z, Rn, q.x, q.y, q.z);
    src[j] = q;
    const size_t o = 3 * (size_t)__float_as_int(q.w);
    verts2[o] = q.x;
    verts2[o + 1] = q.y;
    verts2[o + 2] = q.z;
}

// out = n0 R for row vectors in f32, apply_kernel's product (rows_times): a sensor's current normals from its ORIGINAL ones
// and its accumulated pose (the point-to-plane refine pass: never chained from the previous step's normals).
__global__ __launch_bounds__(kThreads) void rotate_normals_kernel(const float *__restrict__ n0, const float *__restrict__ R, float *__restrict__ out, int n)
{
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= n) return;
    const float Rm[9] = {R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8]};
    const float x = n0[3 * (size_t)j], y = n0[3 * (size_t)j + 1], z = n0[3 * (size_t)j + 2];
    rows_times(x, y, z, Rm, out[3 * (size_t)j], out[3 * (size_t)j + 1], out[3 * (size_t)j + 2]);
}

// What lsnIcpRun clears before its first iteration.
// seeds (nullable): neighbours handed in from outside, by the queries' ORIGINAL index (lsnRefine: the previous Gauss-Seidel pass's) -- they go
// to the sorted order the first NN step reads; that step then is a seeded one with no motion to apply (mk = 0).
__global__ __launch_bounds__(kThreads) void run_init_kernel(unsigned long long *keys, int n_keys, int *counters, int n_counters, IcpState *st,
                                                            const int *__restrict__ seeds, const float4 *__restrict__ src, int n2, int *idx_sorted)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n_keys) keys[i] = ~0ull;
    if (i < n_counters) counters[i] = 0;
    if (i == 0) {
        st->v_valid = 0;
        st->mk = 0;
        if (seeds) st->near_next = 1;   // (the first step has no statistics of a previous one: seeds from a converged pass are near)
    }
    if (seeds && i < n2) idx_sorted[i] = seeds[__float_as_int(src[i].w)];
}

}  // namespace

// ---- host side ---------------------------------------------------------------------------------------------------

// The grids of one call: the target's with its boxes (not for the brute force) and the source's sort.
static int build_grids(LsnIcp *w, const float *d_verts1, int n1, const float *d_verts2, int n2, int nn_mode, hipStream_t s)
{
    if (nn_mode != 0 && build_grid(w->tgt, w->bbox_part.as<float>(), w->block_sums.as<int>(), d_verts1, n1, true, s)) return -1;
    return build_grid(w->src, w->bbox_part.as<float>(), w->block_sums.as<int>(), d_verts2, n2, false, s);
}

extern "C" LsnIcp * lsnIcpCreate(int device, int max_n1, int max_n2)
{
    return lsn::guarded("lsnIcpCreate", static_cast<LsnIcp *>(nullptr), [&]() -> LsnIcp * {
        lsn::clear_error();
        if (max_n1 <= 0 || max_n2 <= 0) {
            lsn::set_error("lsnIcpCreate: bad capacities (%d, %d)", max_n1, max_n2);
            return nullptr;
        }
        LSN_HIP_NULL(hipSetDevice(device));
        LsnIcp *w = new (std::nothrow) LsnIcp();
        if (!w) return nullptr;
        w->device = device;
        w->max_n1 = max_n1;
        w->max_n2 = max_n2;
        if (const char *e3 = getenv("LSN_ICP_NEAR_PTS")) w->near_pts = std::max(1, std::min(kNearCapMax, atoi(e3)));
        if (const char *e4 = getenv("LSN_ICP_NEAR")) w->near_mode = std::max(0, std::min(2, atoi(e4)));
        bool bad = false;
        bad |= w->tgt.reserve(max_n1, true) != 0;
        bad |= w->src.reserve(max_n2, false) != 0;
        bad |= w->bbox_part.reserve(sizeof(float) * 6 * kMaxBlocks) != 0;
        bad |= w->block_sums.reserve(sizeof(int) * 2048) != 0;
        bad |= w->idx.reserve(sizeof(int) * (size_t)max_n2) != 0;
        bad |= w->dist.reserve(sizeof(float) * (size_t)max_n2) != 0;
        bad |= w->keys.reserve(sizeof(unsigned long long) * (size_t)max_n1) != 0;
        bad |= w->counters.reserve(sizeof(int) * 2 * kBankInts) != 0;
        {
            const int n_groups = (max_n2 + 63) / 64;
            // generous: a seeded group needs ~5 super-blocks and ~10 point ranges; $LSN_ICP_TINY_LISTS=1 forces the overflow path (tests)
            const bool tiny = getenv("LSN_ICP_TINY_LISTS") && atoi(getenv("LSN_ICP_TINY_LISTS")) != 0;
            w->seg_a = tiny ? 2 : 1024 + n_groups / 4;   // x 64 segments: 64 k + 16 per group
            w->seg_b = tiny ? 2 : 8192 + 2 * n_groups;   // x 64 segments: 512 k + 128 per group
            bad |= w->best_key.reserve(sizeof(unsigned long long) * (size_t)max_n2) != 0;
            bad |= w->idx_sorted.reserve(sizeof(int) * (size_t)max_n2) != 0;
            bad |= w->groups.reserve(sizeof(GroupInfo) * (size_t)n_groups) != 0;
            bad |= w->list_a.reserve(sizeof(uint2) * (size_t)w->seg_a * kSegs) != 0;
            bad |= w->list_b.reserve(sizeof(int4) * (size_t)w->seg_b * kSegs) != 0;
        }
        bad |= w->part1.reserve(sizeof(double) * 4 * kMaxBlocks) != 0;
        bad |= w->part3.reserve(sizeof(double) * kPlaneStride * kMaxBlocks) != 0;   // 16 per slot (point-to-point) or kPlaneStride (point-to-plane)
        bad |= w->state.reserve(sizeof(IcpState)) != 0;
        bad |= w->trace.reserve(sizeof(float) * 16 * kTraceCap) != 0;
        if (bad) {
            delete w;
            return nullptr;
        }
        return w;
    });
}

extern "C" void lsnIcpDestroy(LsnIcp *w)
{
    lsn::guarded_void("lsnIcpDestroy", [&]() {
        if (!w) return;
        (void)hipSetDevice(w->device);
        for (hipEvent_t e : w->events) (void)hipEventDestroy(e);
        delete w;
    });
}

extern "C" int lsnIcpSetProfiling(LsnIcp *w, int on)
{
    return lsn::guarded("lsnIcpSetProfiling", -1, [&]() {
        lsn::clear_error();
        if (!w) return -1;
        std::lock_guard<std::mutex> g(w->mu);
        w->profiling = on != 0;
        w->n_events = 0;
        return 0;
    });
}

// records the end of `phase` on the stream (profiling only)
static void mark(LsnIcp *w, int phase, hipStream_t s)
{
    if (!w->profiling) return;
    if (w->n_events == w->events.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        w->events.push_back(e);
        w->event_phase.push_back(0);
    }
    w->event_phase[w->n_events] = phase;
    (void)hipEventRecord(w->events[w->n_events++], s);
}

extern "C" int lsnIcpProfile(LsnIcp *w, float *ms4, void *stream)
{
    return lsn::guarded("lsnIcpProfile", -1, [&]() {
        lsn::clear_error();
        if (!w || !ms4) return -1;
        std::lock_guard<std::mutex> g(w->mu);
        LSN_HIP(hipSetDevice(w->device));
        LSN_HIP(hipStreamSynchronize(lsn::as_stream(stream)));
        for (int k = 0; k < 4; k++) ms4[k] = 0.0f;
        for (size_t k = 1; k < w->n_events; k++) {
            float ms = 0.0f;
            LSN_HIP(hipEventElapsedTime(&ms, w->events[k - 1], w->events[k]));
            ms4[w->event_phase[k] & 3] += ms;
        }
        return (int)w->n_events;
    });
}

static int check_sizes(LsnIcp *w, int n1, int n2, const char *who)
{
    if (!w) {
        lsn::set_error("%s: null workspace", who);
        return -1;
    }
    if (n1 <= 0 || n2 <= 0 || n1 > w->max_n1 || n2 > w->max_n2) {
        lsn::set_error("%s: sizes (%d, %d) outside the workspace capacity (%d, %d)", who, n1, n2, w->max_n1, w->max_n2);
        return -1;
    }
    return 0;
}

extern "C" int lsnIcpNearest(LsnIcp *w, const float *d_verts1, int n1, const float *d_verts2, int n2, int *d_idx, float *d_dist2,
                             int nn_mode, void *stream)
{
    return lsn::guarded("lsnIcpNearest", -1, [&]() {
        lsn::clear_error();
        if (check_sizes(w, n1, n2, "lsnIcpNearest")) return -1;
        if (!d_verts1 || !d_verts2 || !d_idx || !d_dist2) {
            lsn::set_error("lsnIcpNearest: null argument");
            return -1;
        }
        std::lock_guard<std::mutex> g(w->mu);
        LSN_HIP(hipSetDevice(w->device));
        hipStream_t s = lsn::as_stream(stream);
        if (build_grids(w, d_verts1, n1, d_verts2, n2, nn_mode, s)) return -1;
        LSN_HIP(hipMemsetAsync(w->counters.p, 0, sizeof(int) * 2 * kBankInts, s));
        return run_nn(w, d_verts1, n1, nullptr, n2, d_idx, d_dist2, nullptr, nn_mode, s, false, nullptr, 0);
    });
}

// d_seeds (nullable, lsnRefine): n2 target indices by the queries' original index -- any index < n1 is a valid seed (a real point bounds the
// search; the result never depends on it), good ones make the first step as cheap as the later ones.
// The body of lsnIcpRun under a name of its own: lsnRefine (below) calls it too, with seeds, inside a guarded entry it makes itself.
// d_normals1 (nullable): n1 x 3 floats, the target's normals at the target's index -- non-null selects the point-to-plane step
// (accum_plane_kernel / solve_plane_kernel in place of accum_kernel / solve_kernel); null is the point-to-point path, launch for launch.
static int icp_run(const char *who, LsnIcp *w, const float *d_verts1, const float *d_normals1, int n1, float *d_verts2, int n2, float *d_R, float *d_t,
                   int maxIter, int nn_mode, void *stream, const int *d_seeds = nullptr)
{
    lsn::clear_error();
    if (check_sizes(w, n1, n2, who)) return -1;
    if (!d_verts1 || !d_verts2 || !d_R || !d_t) {
        lsn::set_error("%s: null argument", who);
        return -1;
    }
    std::lock_guard<std::mutex> g(w->mu);
    LSN_HIP(hipSetDevice(w->device));
    hipStream_t s = lsn::as_stream(stream);
    w->trace_iters = maxIter < kTraceCap ? (maxIter > 0 ? maxIter : 0) : kTraceCap;
    if (maxIter <= 0) return 0;

    w->n_events = 0;
    mark(w, 0, s);
    // the target is fixed: one grid for all iterations; the source is sorted once (rigid motion keeps neighbours together)
    if (build_grids(w, d_verts1, n1, d_verts2, n2, nn_mode, s)) return -1;

    const int nb = capped_blocks(n2);
    unsigned long long *keys = w->keys.as<unsigned long long>();
    IcpState *st = w->state.as<IcpState>();
    // one launch instead of three fills (each a kernel of its own, ~4.5 us): the match keys, the NN step's list counters, and
    // v_valid -- the first iteration's SVD starts cold
    const bool seeded0 = d_seeds && nn_mode != 0;
    hipLaunchKernelGGL(run_init_kernel, dim3(blocks_for(std::max(std::max(n1, n2), 2 * kBankInts))), dim3(kThreads), 0, s, keys, n1, w->counters.as<int>(),
                       2 * kBankInts, st, seeded0 ? d_seeds : (const int *)nullptr, (const float4 *)w->src.sorted.as<float4>(), n2, w->idx_sorted.as<int>());
    for (int iter = 0; iter < maxIter; iter++) {
        // from the second iteration on idx[] still holds every query's previous neighbour: the search is seeded with it, and
        // its first launch also carries out the previous iteration's motion and clears the match keys
        const bool fused = (iter > 0 || seeded0) && nn_mode != 0;
        if (iter > 0 && !fused)
            hipLaunchKernelGGL(apply_kernel, dim3(blocks_for(n2 > n1 ? n2 : n1)), dim3(kThreads), 0, s, w->src.sorted.as<float4>(), d_verts2, n2,
                               (const IcpState *)st, keys, n1);
        if (iter == 0) mark(w, 0, s);
        if (run_nn(w, d_verts1, n1, d_verts2, n2, w->idx.as<int>(), w->dist.as<float>(), keys, nn_mode, s, fused, st, iter & 1)) return -1;
        mark(w, 1, s);
        hipLaunchKernelGGL(stats_kernel, dim3(nb), dim3(kThreads), 0, s, w->idx.as<int>(), w->dist.as<float>(), keys, n2,
                           nn_mode != 0 ? (const GridParams *)w->tgt.gp.as<GridParams>() : (const GridParams *)nullptr, w->part1.as<double>());
        float *trace = iter < kTraceCap ? w->trace.as<float>() : (float *)nullptr;
        if (d_normals1) {
            hipLaunchKernelGGL(accum_plane_kernel, dim3(nb), dim3(kThreads), 0, s, d_verts1, d_normals1, (const float *)d_verts2, w->idx.as<int>(),
                               w->dist.as<float>(), keys, n2, w->part1.as<double>(), nb, w->part3.as<double>(), st);
            hipLaunchKernelGGL(solve_plane_kernel, dim3(1), dim3(kThreads), 0, s, w->part3.as<double>(), nb, d_R, d_t, st, trace, iter);
        } else {
            hipLaunchKernelGGL(accum_kernel, dim3(nb), dim3(kThreads), 0, s, d_verts1, (const float *)d_verts2, w->idx.as<int>(),
                               w->dist.as<float>(), keys, n2, w->part1.as<double>(), nb, w->part3.as<double>(), st);
            hipLaunchKernelGGL(solve_kernel, dim3(1), dim3(kThreads), 0, s, w->part3.as<double>(), nb, d_R, d_t, st, trace, iter);
        }
        mark(w, 2, s);
    }
    hipLaunchKernelGGL(apply_kernel, dim3(blocks_for(n2)), dim3(kThreads), 0, s, w->src.sorted.as<float4>(), d_verts2, n2, (const IcpState *)st,
                       keys, 0);
    mark(w, 3, s);
    LSN_HIP(hipGetLastError());
    return 0;
}

extern "C" int lsnIcpRun(LsnIcp *w, const float *d_verts1, int n1, float *d_verts2, int n2, float *d_R, float *d_t, int maxIter,
                         int nn_mode, void *stream)
{
    return lsn::guarded("lsnIcpRun", -1, [&]() { return icp_run("lsnIcpRun", w, d_verts1, nullptr, n1, d_verts2, n2, d_R, d_t, maxIter, nn_mode, stream); });
}

extern "C" int lsnIcpRunPlane(LsnIcp *w, const float *d_verts1, const float *d_normals1, int n1, float *d_verts2, int n2, float *d_R, float *d_t,
                              int maxIter, int nn_mode, void *stream)
{
    return lsn::guarded("lsnIcpRunPlane", -1, [&]() {
        if (!d_normals1) {
            lsn::clear_error();
            lsn::set_error("lsnIcpRunPlane: null argument");
            return -1;
        }
        return icp_run("lsnIcpRunPlane", w, d_verts1, d_normals1, n1, d_verts2, n2, d_R, d_t, maxIter, nn_mode, stream);
    });
}

// How many queries of the last voxel-grid NN step the near path settled (diagnostic: synchronises `stream`, reads the groups' masks back).
extern "C" int lsnIcpNearResolved(LsnIcp *w, void *stream)
{
    return lsn::guarded("lsnIcpNearResolved", -1, [&]() {
        lsn::clear_error();
        if (!w) return -1;
        std::lock_guard<std::mutex> g(w->mu);
        LSN_HIP(hipSetDevice(w->device));
        LSN_HIP(hipStreamSynchronize(lsn::as_stream(stream)));
        std::vector<GroupInfo> gi((size_t)w->last_groups);
        if (w->last_groups > 0) LSN_HIP(hipMemcpy(gi.data(), w->groups.p, sizeof(GroupInfo) * gi.size(), hipMemcpyDeviceToHost));
        long long n = 0;
        for (const GroupInfo &x : gi) n += __builtin_popcountll(x.resolved);
        return (int)n;
    });
}

extern "C" int lsnIcpTrace(LsnIcp *w, float *out, int max_iters, void *stream)
{
    return lsn::guarded("lsnIcpTrace", -1, [&]() {
        lsn::clear_error();
        if (!w || !out) return -1;
        LSN_HIP(hipSetDevice(w->device));
        LSN_HIP(hipStreamSynchronize(lsn::as_stream(stream)));
        int n = w->trace_iters < max_iters ? w->trace_iters : max_iters;
        if (n > 0) LSN_HIP(hipMemcpy(out, w->trace.p, sizeof(float) * 16 * (size_t)n, hipMemcpyDeviceToHost));
        return n;
    });
}

#include "refine.hip"
