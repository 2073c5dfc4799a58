// color.hip -- the merge call's colour transfer (bcolor_transfer = true): lsnFusionColorTransfer and what the export runs.
//
// Reference: generateMeshFromDepthMaps with bcolor_transfer (src/NativeUtils/depthprocessing.cpp:1745-1763) runs, between the vertex
// generation and the triangulation, generateVerticesConfidence (:285-384, :386-398), updateColorCorrectionCoefficients (:1387-1561)
// and applyColorCorrection (:1563-1575, colorcorrection.cpp:139-170).  Everything is deterministic integer / IEEE arithmetic; the
// stages map onto the data the fusion already keeps in HBM (raw depth maps, the merged cloud of 16-byte records) like this:
//
//   1. index pass and 2. confidence: the cloud index of the depth maps (cloud_index.hip): every pixel's vertex (depth_to_vertices_map),
//      every vertex's pixel (vertices_to_depth_map) and generateMapConfidence on every sensor's full depth map.
//   3. coverage (ct_cov_kernel): calculateMapsCoverage for every pair i < j in ONE pass over the tick's vertices (each vertex of j
//      projected into every lower sensor), counted in an LDS table per workgroup, then one global atomic per non-zero entry.
//   4. pairing (ct_pair_kernel): the greedy choice of :1491-1561, one wave per tick (n <= 32 sensors; each round an argmax over the
//      table).  On the device rather than the host so that a batch of ticks runs without a read-back or a host round trip.
//   5. samples (ct_sample_kernel<0>, ct_block_scan_kernel, ct_sample_kernel<1>): getColorCorrectionTransform's sample set
//      (:1426-1489) of each chosen pair, compacted in j's vertex order; the colour sums (integers: exact in any order) on the way.
//   6. statistics (ct_fold_kernel): the mean absolute deviations -- order-dependent double sums -- folded sequentially in sample order,
//      one lane per (pair, side, channel) (colorcorrection.cpp:66-80), then the transform (:82-93).
//   7. apply (ct_apply_kernel): colorcorrection.cpp:139-170 (CS_RGB) on the colour bytes of every corrected sensor's vertices, in place.
//
// Two places where the reference is defined rather than copied: a sample whose pixel in i has depth but no vertex
// (the crop removed it; the reference reads colors1[-3..-1]) is skipped by the transform (the coverage counts it, as the reference does);
// and a double -> int conversion of a NaN or of a value out of range gives INT_MIN, as in the reference's x64 build (cvttsd2si) --
// gfx950's v_cvt_i32_f64 saturates instead.
// Compiled as part of mesh.hip's translation unit (the include at its end, behind cloud_index.hip, whose index, projection and block
// scan it uses), not on its own.
#include "fusion_shared.hpp"

#include <algorithm>

namespace {

constexpr int kCtMaxMaps = 32;       // LDS coverage table: kCtMaxMaps^2 ints
constexpr int kMinConfidence = 5;    // :1412, :1461
constexpr int kCoverageThreshold = 100;  // :1498
constexpr int kSampleThreads = 256;

// ---- 3. coverage -----------------------------------------------------------------------------------------------------------------
struct CtArgs {
    const FrameDesc *frames;
    const SensorParams *params;
    const unsigned short *depth;
    const int *offsets;        // [n_ticks][n+1]: the caller's table
    const int *pix2v, *v2pix;  // [n_ticks][pixels per tick], [n_ticks][vertices per tick]
    const unsigned char *conf; // [n_ticks][pixels per tick]
    uint4 *verts;              // [n_ticks][vertices per tick]
    int *cov;                  // [n_ticks][n][n]
    int *pairs;                // [n_ticks][pair_words]: n_pairs, (i, j) x np, target[n] (pair that corrects sensor s, -1 = none)
    int *blk;                  // [n_ticks][np][nblk]: samples per block, then exclusive prefixes
    unsigned long long *stats; // [n_ticks][np][8]: sums of i's R,G,B and of j's R,G,B, number of samples
    uint2 *samples;            // [n_ticks][np][nblk * 256]: {i's RGB, j's RGB}
    double *xform;             // [n_ticks][np][9]: mean_i[3], mean_j[3], scale[3]
    int n, np, nblk, pair_words;
    long long tick_pix, tick_vert;
};

__global__ __launch_bounds__(256) void ct_cov_kernel(CtArgs a)
{
    __shared__ int s_cov[kCtMaxMaps * kCtMaxMaps];
    const int tick = blockIdx.y, n = a.n;
    for (int i = threadIdx.x; i < n * n; i += blockDim.x) s_cov[i] = 0;
    __syncthreads();
    const int *off = a.offsets + tick * (n + 1);
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < off[n] && g < a.tick_vert) {
        const int j = sensor_of(off, n, g);
        const int pj = a.v2pix[tick * a.tick_vert + g];
        const unsigned char *conf = a.conf + tick * a.tick_pix;
        // (pj is in the frame whenever the offsets belong to these depth maps; the test keeps a mismatched call in bounds)
        if ((unsigned int)pj < (unsigned int)a.frames[j].npix && conf[a.frames[j].depth_off + pj] >= kMinConfidence) {
            const uint4 v = a.verts[tick * a.tick_vert + g];
            const float X = __uint_as_float(v.y), Y = __uint_as_float(v.z), Z = __uint_as_float(v.w);
            for (int i = 0; i < j; i++) {
                const FrameDesc fi = a.frames[i];
                int x, y, d1;
                project(a.params[i], X, Y, Z, x, y, d1);
                if (x < 0 || x >= fi.w || y < 0 || y >= fi.h || d1 == 0) continue;
                const long long q = fi.depth_off + (long long)y * fi.w + x;
                if (conf[q] < kMinConfidence) continue;
                const int d2 = a.depth[tick * a.tick_pix + q];
                if (d2 > 0 && abs(d1 - d2) < kDepthThreshold) atomicAdd(&s_cov[i * n + j], 1);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n * n; i += blockDim.x)
        if (s_cov[i]) atomicAdd(&a.cov[(long long)tick * n * n + i], s_cov[i]);
}

// ---- 4. pairing (:1491-1561) -----------------------------------------------------------------------------------------------------
// One wave per tick.  Every round of the greedy loop is an argmax over the table: the reference's strict '>' from 0 in (i, j) loop order
// picks the largest value and, among equal ones, the first in row-major order -- a max over (value, -(i * n + j)), which the lanes
// reduce in parallel (the serial loop on one thread was ~100 us of dependent LDS loads).  The assigned set is a bit mask (n <= 32).
__device__ __forceinline__ void better(int &v, int &e, int v2, int e2)
{
    if (v2 > v || (v2 == v && e2 < e)) { v = v2; e = e2; }
}

__global__ __launch_bounds__(64) void ct_pair_kernel(CtArgs a)
{
    __shared__ int s_cov[kCtMaxMaps * kCtMaxMaps];
    const int tick = blockIdx.x, n = a.n, lane = threadIdx.x;
    int *g_cov = a.cov + (long long)tick * n * n;
    // the table is symmetric (:1505); the coverage pass filled i < j (the diagonal and i > j are 0)
    for (int e = lane; e < n * n; e += 64) {
        const int r = e / n, c = e % n;
        s_cov[e] = r < c ? g_cov[e] : g_cov[c * n + r];
    }
    __syncthreads();
    for (int e = lane; e < n * n; e += 64) g_cov[e] = s_cov[e];   // the full table, for the diagnostics
    int *out = a.pairs + (long long)tick * a.pair_words;
    int *target = out + 1 + 2 * a.np;
    for (int i = lane; i < n; i += 64) target[i] = -1;
    unsigned int assigned = 0;
    int np = 0;
    for (;;) {
        // a map already assigned (i) and one that is not (j) first (:1516-1528) ...
        int bv = 0, be = 0x7fffffff;
        for (int e = lane; e < n * n; e += 64) {
            const int i = e / n, j = e % n;
            if (i != j && ((assigned >> i) & 1u) && !((assigned >> j) & 1u)) better(bv, be, s_cov[e], e);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) better(bv, be, __shfl_xor(bv, off, 64), __shfl_xor(be, off, 64));
        if (bv == 0) {   // ... then any pair of two unassigned maps (:1531-1540)
            be = 0x7fffffff;
            for (int e = lane; e < n * n; e += 64) {
                const int i = e / n, j = e % n;
                if (i < j && !((assigned >> i) & 1u) && !((assigned >> j) & 1u)) better(bv, be, s_cov[e], e);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) better(bv, be, __shfl_xor(bv, off, 64), __shfl_xor(be, off, 64));
        }
        if (bv <= kCoverageThreshold || np >= a.np) break;   // coverage_threshold (:1498); every pair assigns a map: np <= n-1
        const int b1 = be / n, b2 = be % n;
        assigned |= (1u << b1) | (1u << b2);
        if (lane == 0) {
            out[1 + 2 * np] = b1;
            out[2 + 2 * np] = b2;
            target[b2] = np;
        }
        np++;
    }
    if (lane == 0) out[0] = np;
}

// ---- 5. samples (:1446-1477) -----------------------------------------------------------------------------------------------------
// PASS 0: samples per block + colour sums; PASS 1 (blk holds exclusive prefixes): the samples, compacted in j's vertex order.
template <int PASS>
__global__ __launch_bounds__(kSampleThreads) void ct_sample_kernel(CtArgs a)
{
    __shared__ int s_wave[kSampleThreads / 64][7];
    const int k = blockIdx.y, tick = blockIdx.z, n = a.n;
    const int *pr = a.pairs + (long long)tick * a.pair_words;
    if (k >= pr[0]) return;   // uniform
    const int i = pr[1 + 2 * k], j = pr[2 + 2 * k];
    const int *off = a.offsets + tick * (n + 1);
    const int v = blockIdx.x * kSampleThreads + threadIdx.x;
    bool take = false;
    unsigned int ci = 0, cj = 0;
    if (v < off[j + 1] - off[j] && off[j] + v < a.tick_vert) {
        const int g = off[j] + v;
        const uint4 vr = a.verts[tick * a.tick_vert + g];
        const FrameDesc fi = a.frames[i];
        int x, y, d1;
        project(a.params[i], __uint_as_float(vr.y), __uint_as_float(vr.z), __uint_as_float(vr.w), x, y, d1);
        if (x >= 0 && x < fi.w && y >= 0 && y < fi.h) {   // no d1 != 0 test here (:1452)
            const long long q = fi.depth_off + (long long)y * fi.w + x;
            const int pjf = a.v2pix[tick * a.tick_vert + g];
            const long long pj = a.frames[j].depth_off + pjf;
            const unsigned char *conf = a.conf + tick * a.tick_pix;
            if ((unsigned int)pjf < (unsigned int)a.frames[j].npix && conf[q] >= kMinConfidence && conf[pj] >= kMinConfidence) {
                const int d2 = a.depth[tick * a.tick_pix + q];
                const int gi = a.pix2v[tick * a.tick_pix + q];
                // gi < 0: depth but no vertex (cropped) -- the reference reads out of bounds here; skipped (file comment)
                if (d2 > 0 && abs(d1 - d2) < kDepthThreshold && gi >= 0) {
                    take = true;
                    ci = a.verts[tick * a.tick_vert + gi].x & 0xFFFFFFu;
                    cj = vr.x & 0xFFFFFFu;
                }
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(take);
    const long long slot = (long long)tick * a.np + k;
    if (PASS == 0) {
        int c[6] = {(int)(ci & 255), (int)((ci >> 8) & 255), (int)(ci >> 16), (int)(cj & 255), (int)((cj >> 8) & 255), (int)(cj >> 16)};
#pragma unroll
        for (int q = 0; q < 6; q++) c[q] = wave_sum(c[q]);
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < 6; q++) s_wave[wave][q] = c[q];
            s_wave[wave][6] = __popcll(m);
        }
        __syncthreads();
        if (threadIdx.x < 7) {
            int s = 0;
            for (int w = 0; w < kSampleThreads / 64; w++) s += s_wave[w][threadIdx.x];
            if (threadIdx.x == 6) a.blk[slot * a.nblk + blockIdx.x] = s;
            if (s) atomicAdd(&a.stats[slot * 8 + threadIdx.x], (unsigned long long)s);
        }
        return;
    }
    int total;
    const int r = a.blk[slot * a.nblk + blockIdx.x] + block_rank<kSampleThreads / 64>(take, s_wave[0], total);
    if (take) a.samples[slot * a.nblk * kSampleThreads + r] = make_uint2(ci, cj);
}

// ---- 6. statistics (colorcorrection.cpp:6-96, CS_RGB) ----------------------------------------------------------------------------
// One workgroup per (pair, tick); lane l < 6: side l / 3 (0 = i, the source; 1 = j), channel l % 3.  Each deviation sum is folded in
// sample order, as the reference's loop adds it (the channels' sums are independent of one another).
__global__ __launch_bounds__(64) void ct_fold_kernel(CtArgs a)
{
    __shared__ double s_dev[6];
    const int k = blockIdx.x, tick = blockIdx.y;
    const int *pr = a.pairs + (long long)tick * a.pair_words;
    if (k >= pr[0]) return;
    const long long slot = (long long)tick * a.np + k;
    const unsigned long long *st = a.stats + slot * 8;
    const long long ns = (long long)st[6];
    double *xf = a.xform + slot * 9;
    const int l = threadIdx.x;
    if (ns == 0) {   // empty sample set: the early return (:10-11) -- means 0, scales 1, colour space defined as RGB
        if (l < 9) xf[l] = l < 6 ? 0.0 : 1.0;
        return;
    }
    if (l < 6) {
        const double mean = (double)st[l] / (double)ns;   // :57-61 (sums of integers below 2^53: exact in any order)
        const uint2 *smp = a.samples + slot * a.nblk * kSampleThreads;
        const int shift = (l % 3) * 8;
        const bool src = l < 3;
        double dev = 0.0;
        long long s = 0;
        for (; s + 8 <= ns; s += 8) {   // the loads ahead of the dependent adds
            unsigned int c[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const uint2 e = smp[s + u];
                c[u] = ((src ? e.x : e.y) >> shift) & 255u;
            }
#pragma unroll
            for (int u = 0; u < 8; u++) dev += fabs((double)c[u] - mean);
        }
        for (; s < ns; s++) {
            const uint2 e = smp[s];
            dev += fabs((double)(((src ? e.x : e.y) >> shift) & 255u) - mean);
        }
        dev /= (double)ns;
        dev += 1e-15;
        s_dev[l] = dev;
        xf[l] = mean;
    }
    __syncthreads();
    if (l < 3) xf[6 + l] = s_dev[l] / s_dev[3 + l];
}

// ---- 7. apply (colorcorrection.cpp:139-170, CS_RGB) ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ct_apply_kernel(CtArgs a)
{
    const int tick = blockIdx.y, n = a.n;
    const int *off = a.offsets + tick * (n + 1);
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= off[n] || g >= a.tick_vert) return;
    const int *pr = a.pairs + (long long)tick * a.pair_words;
    const int k = pr[1 + 2 * a.np + sensor_of(off, n, g)];
    if (k < 0) return;
    const double *xf = a.xform + ((long long)tick * a.np + k) * 9;
    unsigned int *rgba = &a.verts[tick * a.tick_vert + g].x;
    const unsigned int c = *rgba;
    unsigned int o = c & 0xFF000000u;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const double val = ((double)((c >> (8 * ch)) & 255u) - xf[3 + ch]) * xf[6 + ch] + xf[ch];
        o |= (unsigned int)min(255, max(0, cvt_i32_x64(val))) << (8 * ch);
    }
    *rgba = o;
}

}  // namespace

namespace lsn {

// The seven stages on `s` over all ticks of the plan; d_vertices / d_offsets as lsnFusionRun left them.  Plan mutex held.
static int color_transfer_locked(LsnFusion *p, const void *d_depth, void *d_vertices, const int *d_offsets, hipStream_t s)
{
    const int n = p->n_maps, T = p->n_ticks;
    if (n > kCtMaxMaps) {
        lsn::set_error("lsnFusionColorTransfer: at most %d sensors (the plan has %d)", kCtMaxMaps, n);
        return -1;
    }
    LSN_HIP(hipSetDevice(p->device));
    const int np = n > 1 ? n - 1 : 1;   // pair slots (at most n - 1 pairs are chosen)
    const int pair_words = 1 + 2 * np + n;
    long long max_pix = 1;
    for (int i = 0; i < n; i++) max_pix = std::max(max_pix, (long long)p->w[i] * p->h[i]);
    const int nblk = (int)((max_pix + kSampleThreads - 1) / kSampleThreads);
    if (!p->ct_ready) {
        if (p->ct_cov.reserve(sizeof(int) * (size_t)n * n * T) || p->ct_pairs.reserve(sizeof(int) * (size_t)pair_words * T) ||
            p->ct_blk.reserve(sizeof(int) * (size_t)np * nblk * T) || p->ct_stats.reserve(sizeof(unsigned long long) * 8 * (size_t)np * T) ||
            p->ct_samples.reserve(sizeof(uint2) * (size_t)np * nblk * kSampleThreads * T) ||
            p->ct_xform.reserve(sizeof(double) * 9 * (size_t)np * T))
            return -1;
        p->ct_nblk = nblk;
        p->ct_ready = true;
    }
    // 1. pixel <-> vertex maps, 2. confidence
    if (cloud_index_locked(p, d_depth, d_vertices, true, s)) return -1;
    CtArgs a;
    a.frames = p->frames.as<FrameDesc>();
    a.params = p->params.as<SensorParams>();
    a.depth = static_cast<const unsigned short *>(d_depth);
    a.offsets = d_offsets;
    a.pix2v = p->ix_pix2v.as<int>();
    a.v2pix = p->ix_v2pix.as<int>();
    a.conf = p->ix_conf.as<unsigned char>();
    a.verts = static_cast<uint4 *>(d_vertices);
    a.cov = p->ct_cov.as<int>();
    a.pairs = p->ct_pairs.as<int>();
    a.blk = p->ct_blk.as<int>();
    a.stats = p->ct_stats.as<unsigned long long>();
    a.samples = p->ct_samples.as<uint2>();
    a.xform = p->ct_xform.as<double>();
    a.n = n;
    a.np = np;
    a.nblk = nblk;
    a.pair_words = pair_words;
    a.tick_pix = p->tick_depth_elems;
    a.tick_vert = p->cap;
    const unsigned int vblocks = (unsigned int)((p->cap + 255) / 256);
    // 3. coverage, 4. pairing
    LSN_HIP(hipMemsetAsync(a.cov, 0, sizeof(int) * (size_t)n * n * T, s));
    hipLaunchKernelGGL(ct_cov_kernel, dim3(vblocks, T), dim3(256), 0, s, a);
    hipLaunchKernelGGL(ct_pair_kernel, dim3(T), dim3(64), 0, s, a);
    if (n > 1) {
        // 5. samples, 6. statistics, 7. apply
        LSN_HIP(hipMemsetAsync(a.stats, 0, sizeof(unsigned long long) * 8 * (size_t)np * T, s));
        hipLaunchKernelGGL(ct_sample_kernel<0>, dim3(nblk, np, T), dim3(kSampleThreads), 0, s, a);
        hipLaunchKernelGGL(ct_block_scan_kernel, dim3(T * np), dim3(1024), 0, s, a.blk, nblk);
        hipLaunchKernelGGL(ct_sample_kernel<1>, dim3(nblk, np, T), dim3(kSampleThreads), 0, s, a);
        hipLaunchKernelGGL(ct_fold_kernel, dim3(np, T), dim3(64), 0, s, a);
        hipLaunchKernelGGL(ct_apply_kernel, dim3(vblocks, T), dim3(256), 0, s, a);
    }
    LSN_HIP(hipGetLastError());
    return 0;
}

int color_transfer(LsnFusion *p, const void *d_depth, void *d_vertices, const int *d_offsets, hipStream_t s)
{
    if (!p || !d_depth || !d_vertices || !d_offsets) {
        lsn::set_error("lsnFusionColorTransfer: null argument");
        return -1;
    }
    if (!p->params_set) {
        lsn::set_error("lsnFusionColorTransfer: lsnFusionSetParams has not been called");
        return -1;
    }
    std::lock_guard<std::mutex> g(p->mu);
    return color_transfer_locked(p, d_depth, d_vertices, d_offsets, s);
}

}  // namespace lsn

extern "C" int lsnFusionColorTransfer(LsnFusion *p, const void *d_depth_maps, void *d_vertices, const int *d_offsets, void *stream)
{
    return lsn::guarded("lsnFusionColorTransfer", -1, [&]() {
        lsn::clear_error();
        return lsn::color_transfer(p, d_depth_maps, d_vertices, d_offsets, lsn::as_stream(stream));
    });
}

extern "C" int lsnFusionColorDiagnostics(LsnFusion *p, int tick, unsigned char *conf, int *coverage, int *pairs, double *xform, void *stream)
{
    return lsn::guarded("lsnFusionColorDiagnostics", -1, [&]() {
        lsn::clear_error();
        if (!p || tick < 0 || tick >= p->n_ticks) {
            lsn::set_error("lsnFusionColorDiagnostics: bad arguments");
            return -1;
        }
        std::lock_guard<std::mutex> g(p->mu);
        if (!p->ct_ready) {
            lsn::set_error("lsnFusionColorDiagnostics: no colour transfer has run on this plan");
            return -1;
        }
        LSN_HIP(hipSetDevice(p->device));
        hipStream_t s = lsn::as_stream(stream);
        const int n = p->n_maps, np = n > 1 ? n - 1 : 1, words = 1 + 2 * np + n;
        std::vector<int> pr((size_t)words);
        LSN_HIP(hipMemcpyAsync(pr.data(), p->ct_pairs.as<int>() + (size_t)tick * words, sizeof(int) * words, hipMemcpyDeviceToHost, s));
        if (conf) LSN_HIP(hipMemcpyAsync(conf, p->ix_conf.as<unsigned char>() + (size_t)tick * p->cap, (size_t)p->cap, hipMemcpyDeviceToHost, s));
        if (coverage)
            LSN_HIP(hipMemcpyAsync(coverage, p->ct_cov.as<int>() + (size_t)tick * n * n, sizeof(int) * n * n, hipMemcpyDeviceToHost, s));
        if (xform) LSN_HIP(hipMemcpyAsync(xform, p->ct_xform.as<double>() + (size_t)tick * np * 9, sizeof(double) * 9 * np, hipMemcpyDeviceToHost, s));
        LSN_HIP(hipStreamSynchronize(s));
        const int n_pairs = pr[0] >= 0 && pr[0] <= np ? pr[0] : 0;
        if (pairs)
            for (int k = 0; k < 2 * n_pairs; k++) pairs[k] = pr[1 + k];
        return n_pairs;
    });
}
