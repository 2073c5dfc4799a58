// merge.hip -- the merge call's cross-view overlay merge (bgenerate_triangles = true): lsnFusionOverlayMerge and what the export runs.
//
// Reference: generateMeshFromDepthMaps with bgenerate_triangles (src/NativeUtils/depthprocessing.cpp:1715-1792) runs, after the vertex
// generation, generateVerticesConfidence (:386-427) and the optional colour transfer, mergeVerticesForViews (:1227-1313), then
// generateTriangles (:1659-1691) on every sensor's MODIFIED depth_map / depth_to_vertices_map and formMesh (:1578-1629).  The merge
// removes, adds or reorders no vertex and touches no colour: only the triangle list changes.  On the device, over every tick of the plan:
//
//   0. pixel <-> vertex maps and confidence maps of the raw depth maps: the plan's cloud index (cloud_index.hip; vertices_to_depth_map
//      and confidence_map of the reference).
//   1. reprojection (mg_reproject_kernel, :1241-1248, projectVerticesIntoDepthMap :749-782 with includeAssigned = false): every vertex
//      projected with the inverse of its own pose; the last vertex that lands on a pixel wins (an atomicMax of the vertex index, then
//      the winner writes its depth).  No d == 0 test here.
//   2. for every base b in turn (:1250-1300), every overlay o != b in increasing order (assignDepthMapOverlay, :932-1099):
//      a. the overlay's CURRENT maps triangulated by mesh.hip's passes (mapDepthMap :844-845; all sensors at once, b's list unused);
//      b. the overlay's unassigned vertices projected into b's camera (mg_project_kernel, :858-873);
//      c. every triangle whose three depths are non-zero rasterised into the mapped map of (o, b) (mg_raster_kernel, drawTriangle
//         :598-706).  drawTriangle's "d == 0 || val < depth_map[x]" makes the result depend on the order: per pixel it equals
//         the covering triangle of smallest (val, index) among those behind the last one whose val is 0 (Z), or depth 0 with Z's
//         tag when there is none -- two atomic passes (atomicMax of Z, then a 64-bit atomicMin of val << 32 | index) and a resolve
//         (mg_resolve_kernel).  All n - 1 mapped maps of one base are built together: each depends on its overlay's state alone.
//      d. mask (:989-1020), morphologyErode twice (:903-930), zero the base pixels and assign their vertices (:1026-1032): the only
//         sequential fold over the overlays, two per-pixel launches per overlay (mg_erode_kernel<0/1>).
//   3. mesh.hip's triangle passes on the final maps, into the caller's triangle buffers (generateTriangles + formMesh's rebase).
//
// Defined here where the reference is not: float -> unsigned short as x64 code converts (cvttss2si, then the low 16
// bits: cvt_u16_x64, raster.hip); every sensor must have the same size (the reference strides an overlay with the base's width); no debug images or timings.
// Compiled as part of mesh.hip's translation unit (after cloud_index.hip, whose project / cvt_i32_x64 and cloud index it uses, and
// raster.hip, whose cvt_u16_x64).
#include "fusion_shared.hpp"

namespace {

constexpr int kMgMaxMaps = 32;        // as for the colour transfer
constexpr int kMgDepthThreshold = 20; // depth_threshold (:934)
constexpr int kMgConfThreshold = 5;   // overlay_confidence[el] > 5 (:1007)
constexpr int kMgRasterBlocks = 1024; // raster workgroups per tick (grid-stride over the tick's triangles)

struct MgArgs {
    const FrameDesc *frames;
    const SensorParams *params;
    const uint4 *verts;            // [n_ticks][vertices per tick]: the caller's cloud (read only)
    const int *voff;               // [n_ticks][n+1]: the caller's vertex offsets
    const int *v2pix;              // [n_ticks][vertices per tick]: vertex -> pixel of its own raw map (vertices_to_depth_map)
    const unsigned char *conf;     // [n_ticks][pixels per tick]: confidence maps of the raw maps
    unsigned short *depth;         // [n_ticks][pixels per tick]: the reprojected maps, modified by the merge (depth_map)
    int *d2v;                      // [n_ticks][pixels per tick]: their pixel -> vertex maps (depth_to_vertices_map)
    unsigned char *assigned;       // [n_ticks][vertices per tick]: point_assigned
    unsigned char *vconf;          // [n_ticks][vertices per tick]: confidence_map[vertices_to_depth_map[v]] (:870)
    int2 *proj;                    // [n_ticks][vertices per tick]: {x | y << 16, d} in the current base's camera, d = 0: dropped
    const int *tri;                // [n_ticks][triangles per tick][3]: the current maps' triangles (step 2a)
    const int *toff;               // [n_ticks][n+1]: their offsets
    int *zmax;                     // [n_ticks][pixels per tick]: per mapped pixel, the last covering triangle of val 0 (-1 = none)
    unsigned long long *key;       // [n_ticks][pixels per tick]: min (val << 32 | triangle) behind it (~0 = none)
    unsigned short *mdepth, *mtag; // [n_ticks][pixels per tick]: mapped depth / confidence tag; overlay o's map lies in o's slot
    unsigned char *ero;            // [n_ticks][pixels per tick]: the mask after the first erosion, in the base's slot
    int n;
    long long tick_pix, tick_vert, tick_tri;
};

// ---- 1. reprojection (:749-782) ------------------------------------------------------------------------------------------------
// PASS 0: per-vertex confidence, clear point_assigned, claim the pixel (the largest vertex index = the last in the loop of :768);
// PASS 1: the winner writes its depth.  d2v / depth were cleared to -1 / 0 before (:758-762).
template <int PASS>
__global__ __launch_bounds__(256) void mg_reproject_kernel(MgArgs a)
{
    const int tick = blockIdx.y, n = a.n;
    const int *off = a.voff + tick * (n + 1);
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= off[n] || g >= a.tick_vert) return;
    const int s = sensor_of(off, n, g);
    const FrameDesc f = a.frames[s];
    const long long vg = tick * a.tick_vert + g;
    if (PASS == 0) {
        const int pj = a.v2pix[vg];
        a.vconf[vg] = (unsigned int)pj < (unsigned int)f.npix ? a.conf[tick * a.tick_pix + f.depth_off + pj] : 0;
        a.assigned[vg] = 0;
    }
    const uint4 v = a.verts[vg];
    int x, y, d;
    project(a.params[s], __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w), x, y, d);
    if (x < 0 || x >= f.w || y < 0 || y >= f.h) return;   // :773-774
    const long long q = tick * a.tick_pix + f.depth_off + (long long)y * f.w + x;
    if (PASS == 0) atomicMax(&a.d2v[q], g);
    else if (a.d2v[q] == g) a.depth[q] = (unsigned short)d;   // :776-777
}

// ---- 2b. the overlays' unassigned vertices in base b's camera (mapDepthMap :858-873) ---------------------------------------------
__global__ __launch_bounds__(256) void mg_project_kernel(MgArgs a, int b)
{
    const int tick = blockIdx.y, n = a.n;
    const int *off = a.voff + tick * (n + 1);
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= off[n] || g >= a.tick_vert) return;
    const long long vg = tick * a.tick_vert + g;
    int2 r = make_int2(0, 0);
    if (sensor_of(off, n, g) != b && !a.assigned[vg]) {   // :860-861 (b's own vertices are never drawn into b)
        const FrameDesc fb = a.frames[b];
        const uint4 v = a.verts[vg];
        int x, y, d;
        project(a.params[b], __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w), x, y, d);
        if (!(x < 1 || x >= fb.w || y < 1 || y >= fb.h || d == 0)) r = make_int2(x | (y << 16), d);   // :866-867
    }
    a.proj[vg] = r;
}

// ---- 2c. drawTriangle (:598-706) -----------------------------------------------------------------------------------------------
// One lane per triangle, its bounding box walked as the reference walks it.  The set-up and the per-pixel value are raster.hip's
// tri_setup / tri_value written out in place, with the row's two terms hoisted: calling them cost this kernel 0.4 % of the merge's time
// (17 more VGPRs, the row terms recomputed per covered pixel), so it keeps its own copy -- a change to either is made in both.  PASS 0: atomicMax of the index over the covered pixels of
// val 0; PASS 1 (after PASS 0 everywhere): 64-bit atomicMin of (val << 32 | index) over the covered pixels whose Z is below the index.
template <int PASS>
__global__ __launch_bounds__(256) void mg_raster_kernel(MgArgs a, int b)
{
    const int tick = blockIdx.y, n = a.n;
    const int *toff = a.toff + tick * (n + 1);
    const int nt = min(toff[n], (int)a.tick_tri);
    const int w = a.frames[b].w;   // every sensor has b's size (checked by the host)
    const int *tri = a.tri + 3 * tick * a.tick_tri;
    const int2 *proj = a.proj + tick * a.tick_vert;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < nt; t += gridDim.x * blockDim.x) {
        const int o = sensor_of(toff, n, t);
        if (o == b) continue;
        const int i1 = tri[3 * t], i2 = tri[3 * t + 1], i3 = tri[3 * t + 2];
        if ((unsigned int)i1 >= (unsigned int)a.tick_vert || (unsigned int)i2 >= (unsigned int)a.tick_vert ||
            (unsigned int)i3 >= (unsigned int)a.tick_vert)
            continue;
        const int2 p1 = proj[i1], p2 = proj[i2], p3 = proj[i3];
        if (p1.y == 0 || p2.y == 0 || p3.y == 0) continue;   // :885-886
        const int x1 = p1.x & 0xFFFF, y1 = p1.x >> 16, x2 = p2.x & 0xFFFF, y2 = p2.x >> 16, x3 = p3.x & 0xFFFF, y3 = p3.x >> 16;
        // 28.4 fixed point of integer positions (:602-609: iround(16.0f * v) is exact)
        const int X1 = 16 * x1, X2 = 16 * x2, X3 = 16 * x3, Y1 = 16 * y1, Y2 = 16 * y2, Y3 = 16 * y3;
        const int DX12 = X1 - X2, DX23 = X2 - X3, DX31 = X3 - X1;
        const int DY12 = Y1 - Y2, DY23 = Y2 - Y3, DY31 = Y3 - Y1;
        const int minx = (min(min(X1, X2), X3) + 0xF) >> 4, maxx = (max(max(X1, X2), X3) + 0xF) >> 4;   // :629-632, half-open
        const int miny = (min(min(Y1, Y2), Y3) + 0xF) >> 4, maxy = (max(max(Y1, Y2), Y3) + 0xF) >> 4;
        int C1 = DY12 * X1 - DX12 * Y1, C2 = DY23 * X2 - DX23 * Y2, C3 = DY31 * X3 - DX31 * Y3;   // :639-641
        if (DY12 < 0 || (DY12 == 0 && DX12 > 0)) C1++;   // fill convention (:644-646)
        if (DY23 < 0 || (DY23 == 0 && DX23 > 0)) C2++;
        if (DY31 < 0 || (DY31 == 0 && DX31 > 0)) C3++;
        const int den = (y2 - y3) * (x1 - x3) + (x3 - x2) * (y1 - y3);   // :656, :660 (int, then float; den1 == den2)
        if (den == 0) continue;                                          // :662-663
        const float fden = (float)den, y23 = (float)(y2 - y3), x32 = (float)(x3 - x2), y31 = (float)(y3 - y1), x13 = (float)(x1 - x3);
        const float fd1 = (float)p1.y, fd2 = (float)p2.y, fd3 = (float)p3.y;
        const long long slot = tick * a.tick_pix + a.frames[o].depth_off;
        int CY1 = C1 + DX12 * (miny << 4) - DY12 * (minx << 4);   // :648-650
        int CY2 = C2 + DX23 * (miny << 4) - DY23 * (minx << 4);
        int CY3 = C3 + DX31 * (miny << 4) - DY31 * (minx << 4);
        for (int y = miny; y < maxy; y++) {
            int CX1 = CY1, CX2 = CY2, CX3 = CY3;
            const float term21 = __fmul_rn(x32, (float)(y - y3)), term22 = __fmul_rn(x13, (float)(y - y3));   // :671-672
            for (int x = minx; x < maxx; x++) {
                if (CX1 >= 0 && CX2 >= 0 && CX3 >= 0) {
                    const float w1 = __fdiv_rn(__fadd_rn(__fmul_rn(y23, (float)(x - x3)), term21), fden);   // :677-679
                    const float w2 = __fdiv_rn(__fadd_rn(__fmul_rn(y31, (float)(x - x3)), term22), fden);
                    const float w3 = __fsub_rn(__fsub_rn(1.0f, w1), w2);
                    const float fv = __fadd_rn(__fadd_rn(__fmul_rn(fd1, w1), __fmul_rn(fd2, w2)), __fmul_rn(fd3, w3));   // :682
                    const unsigned int val = cvt_u16_x64(fv);
                    const long long q = slot + (long long)y * w + x;
                    if (PASS == 0) {
                        if (val == 0) atomicMax(&a.zmax[q], t);
                    } else if (t > a.zmax[q]) {
                        atomicMin(&a.key[q], ((unsigned long long)val << 32) | (unsigned int)t);
                    }
                }
                CX1 -= DY12 << 4;
                CX2 -= DY23 << 4;
                CX3 -= DY31 << 4;
            }
            CY1 += DX12 << 4;
            CY2 += DX23 << 4;
            CY3 += DX31 << 4;
        }
    }
}

// The winner of every mapped pixel of the overlays of base b: depth and confidence tag ((c1 + c2 + c3) / 3.0f, :879), then the two
// scratch words back to "none" for the next base.
__global__ __launch_bounds__(256) void mg_resolve_kernel(MgArgs a, int b)
{
    const int o = blockIdx.y, tick = blockIdx.z;
    if (o == b) return;
    const FrameDesc f = a.frames[o];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= f.npix) return;
    const long long q = tick * a.tick_pix + f.depth_off + i;
    const unsigned long long k = a.key[q];
    const int z = a.zmax[q];
    const int t = k != ~0ull ? (int)(unsigned int)k : z;
    unsigned int d = 0, tag = 0;
    if (t >= 0 && t < a.tick_tri) {
        const int *tr = a.tri + 3 * (tick * a.tick_tri + t);
        const unsigned char *vc = a.vconf + tick * a.tick_vert;
        const int c = (int)vc[tr[0]] + (int)vc[tr[1]] + (int)vc[tr[2]];
        tag = cvt_u16_x64(__fdiv_rn((float)c, 3.0f));
        d = k != ~0ull ? (unsigned int)(k >> 32) : 0u;
    }
    a.mdepth[q] = (unsigned short)d;
    a.mtag[q] = (unsigned short)tag;
    a.key[q] = ~0ull;
    a.zmax[q] = -1;
}

// ---- 2d. mask, erosion x 2, assignment (:989-1032) -------------------------------------------------------------------------------
// STEP 0: ero = the mask of overlay o eroded once (the mask evaluated on the fly at the 3 x 3 neighbourhood); STEP 1: eroded again,
// and every pixel still set zeroes b's depth and assigns b's vertex there.  morphologyErode (:903-930) leaves border pixels as they are.
template <int STEP>
__global__ __launch_bounds__(256) void mg_erode_kernel(MgArgs a, int b, int o)
{
    const int tick = blockIdx.y;
    const FrameDesc fb = a.frames[b];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= fb.npix) return;
    const int w = fb.w, h = fb.h, x = i % w, y = i / w;
    const long long base = tick * a.tick_pix + fb.depth_off;
    const long long ov = tick * a.tick_pix + a.frames[o].depth_off;
    auto in = [&](int j) -> bool {
        if (STEP == 1) return a.ero[base + j] != 0;
        const int d = a.depth[base + j];
        return d != 0 && abs(d - (int)a.mdepth[ov + j]) < kMgDepthThreshold && a.mtag[ov + j] > kMgConfThreshold;   // :996-1011
    };
    bool m = in(i);
    if (m && x >= 1 && y >= 1 && x < w - 1 && y < h - 1) {
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++)
                if ((dx | dy) != 0) m = m && in(i + dx + dy * w);
    }
    if (STEP == 0) {
        a.ero[base + i] = m ? 255 : 0;
    } else if (m) {
        a.depth[base + i] = 0;   // :1029-1031
        const int v = a.d2v[base + i];
        if ((unsigned int)v < (unsigned int)a.tick_vert) a.assigned[tick * a.tick_vert + v] = 1;
    }
}

}  // namespace

namespace lsn {

// The whole merge on `s` over all ticks of the plan; d_vertices / d_offsets as lsnFusionRun left them.  Plan mutex held.
static int overlay_merge_locked(LsnFusion *p, const void *d_depth, const void *d_vertices, const int *d_offsets, void *d_triangles,
                                int *d_tri_offsets, hipStream_t s)
{
    const int n = p->n_maps, T = p->n_ticks;
    if (n > kMgMaxMaps) {
        lsn::set_error("lsnFusionOverlayMerge: at most %d sensors (the plan has %d)", kMgMaxMaps, n);
        return -1;
    }
    for (int i = 1; i < n; i++)
        if (p->w[i] != p->w[0] || p->h[i] != p->h[0]) {
            lsn::set_error("lsnFusionOverlayMerge: every sensor must have the same size (sensor 0 is %dx%d, sensor %d is %dx%d)", p->w[0], p->h[0],
                           i, p->w[i], p->h[i]);
            return -1;
        }
    LSN_HIP(hipSetDevice(p->device));
    const size_t px = (size_t)p->cap * T;
    if (!p->mg_ready) {
        if (p->mg_toff.reserve(sizeof(int) * (size_t)(n + 1) * T) ||
            p->mg_depth0.reserve(sizeof(unsigned short) * px) || p->mg_depth.reserve(sizeof(unsigned short) * px) ||
            p->mg_d2v.reserve(sizeof(int) * px) || p->mg_assigned.reserve(px) || p->mg_vconf.reserve(px) ||
            p->mg_proj.reserve(sizeof(int2) * px) || p->mg_zmax.reserve(sizeof(int) * px) ||
            p->mg_key.reserve(sizeof(unsigned long long) * px) || p->mg_mdepth.reserve(sizeof(unsigned short) * px) ||
            p->mg_mtag.reserve(sizeof(unsigned short) * px) || p->mg_ero.reserve(px) ||
            p->tri_counts.reserve(sizeof(int) * (size_t)p->tiles_per_tick * T) ||
            p->tri_codes.reserve(sizeof(unsigned int) * (size_t)p->tiles_per_tick * T * kThreads))
            return -1;
        p->mg_ready = true;
    }
    // 0. pixel <-> vertex maps and confidence maps of the raw depth maps
    if (cloud_index_locked(p, d_depth, const_cast<void *>(d_vertices), true, s)) return -1;
    MgArgs a;
    a.frames = p->frames.as<FrameDesc>();
    a.params = p->params.as<SensorParams>();
    a.verts = static_cast<const uint4 *>(d_vertices);
    a.voff = d_offsets;
    a.v2pix = p->ix_v2pix.as<int>();
    a.conf = p->ix_conf.as<unsigned char>();
    a.depth = p->mg_depth.as<unsigned short>();
    a.d2v = p->mg_d2v.as<int>();
    a.assigned = p->mg_assigned.as<unsigned char>();
    a.vconf = p->mg_vconf.as<unsigned char>();
    a.proj = p->mg_proj.as<int2>();
    a.tri = static_cast<const int *>(d_triangles);
    a.toff = p->mg_toff.as<int>();
    a.zmax = p->mg_zmax.as<int>();
    a.key = p->mg_key.as<unsigned long long>();
    a.mdepth = p->mg_mdepth.as<unsigned short>();
    a.mtag = p->mg_mtag.as<unsigned short>();
    a.ero = p->mg_ero.as<unsigned char>();
    a.n = n;
    a.tick_pix = p->tick_depth_elems;
    a.tick_vert = p->cap;
    a.tick_tri = 2 * p->cap;
    const unsigned int vblocks = (unsigned int)((p->cap + 255) / 256);
    const unsigned int pblocks = (unsigned int)((p->w[0] * p->h[0] + 255) / 256);
    // 1. reprojection; the raster scratch starts at "none" (mg_resolve_kernel puts it back after every base)
    LSN_HIP(hipMemsetAsync(a.d2v, 0xFF, sizeof(int) * px, s));
    LSN_HIP(hipMemsetAsync(a.depth, 0, sizeof(unsigned short) * px, s));
    LSN_HIP(hipMemsetAsync(a.zmax, 0xFF, sizeof(int) * px, s));
    LSN_HIP(hipMemsetAsync(a.key, 0xFF, sizeof(unsigned long long) * px, s));
    hipLaunchKernelGGL(mg_reproject_kernel<0>, dim3(vblocks, T), dim3(256), 0, s, a);
    hipLaunchKernelGGL(mg_reproject_kernel<1>, dim3(vblocks, T), dim3(256), 0, s, a);
    LSN_HIP(hipMemcpyAsync(p->mg_depth0.p, a.depth, sizeof(unsigned short) * px, hipMemcpyDeviceToDevice, s));
    // 2. bases in turn
    for (int b = 0; b < n && n > 1; b++) {
        if (triangle_count_passes(p, a.depth, p->mg_toff.as<int>(), nullptr, nullptr, s, a.d2v) ||
            triangle_write_pass(p, a.depth, d_triangles, 0, false, s, a.d2v))
            return -1;
        hipLaunchKernelGGL(mg_project_kernel, dim3(vblocks, T), dim3(256), 0, s, a, b);
        hipLaunchKernelGGL(mg_raster_kernel<0>, dim3(kMgRasterBlocks, T), dim3(256), 0, s, a, b);
        hipLaunchKernelGGL(mg_raster_kernel<1>, dim3(kMgRasterBlocks, T), dim3(256), 0, s, a, b);
        hipLaunchKernelGGL(mg_resolve_kernel, dim3(pblocks, n, T), dim3(256), 0, s, a, b);
        for (int o = 0; o < n; o++) {
            if (o == b) continue;
            hipLaunchKernelGGL(mg_erode_kernel<0>, dim3(pblocks, T), dim3(256), 0, s, a, b, o);
            hipLaunchKernelGGL(mg_erode_kernel<1>, dim3(pblocks, T), dim3(256), 0, s, a, b, o);
        }
    }
    // 3. the final maps triangulated into the caller's buffers
    if (triangle_count_passes(p, a.depth, d_tri_offsets, nullptr, nullptr, s, a.d2v) || triangle_write_pass(p, a.depth, d_triangles, 0, false, s, a.d2v))
        return -1;
    LSN_HIP(hipGetLastError());
    return 0;
}

int overlay_merge(LsnFusion *p, const void *d_depth, const void *d_vertices, const int *d_offsets, void *d_triangles, int *d_tri_offsets,
                  hipStream_t s)
{
    if (!p || !d_depth || !d_vertices || !d_offsets || !d_triangles || !d_tri_offsets) {
        lsn::set_error("lsnFusionOverlayMerge: null argument");
        return -1;
    }
    if (!p->params_set) {
        lsn::set_error("lsnFusionOverlayMerge: lsnFusionSetParams has not been called");
        return -1;
    }
    std::lock_guard<std::mutex> g(p->mu);
    return overlay_merge_locked(p, d_depth, d_vertices, d_offsets, d_triangles, d_tri_offsets, s);
}

}  // namespace lsn

extern "C" int lsnFusionOverlayMerge(LsnFusion *p, const void *d_depth_maps, const void *d_vertices, const int *d_offsets, void *d_triangles,
                                     int *d_tri_offsets, void *stream)
{
    return lsn::guarded("lsnFusionOverlayMerge", -1, [&]() {
        lsn::clear_error();
        return lsn::overlay_merge(p, d_depth_maps, d_vertices, d_offsets, d_triangles, d_tri_offsets, lsn::as_stream(stream));
    });
}

extern "C" int lsnFusionOverlayDiagnostics(LsnFusion *p, int tick, unsigned short *reprojected, unsigned short *merged, unsigned char *assigned,
                                           void *stream)
{
    return lsn::guarded("lsnFusionOverlayDiagnostics", -1, [&]() {
        lsn::clear_error();
        if (!p || tick < 0 || tick >= p->n_ticks) {
            lsn::set_error("lsnFusionOverlayDiagnostics: bad arguments");
            return -1;
        }
        std::lock_guard<std::mutex> g(p->mu);
        if (!p->mg_ready) {
            lsn::set_error("lsnFusionOverlayDiagnostics: no overlay merge has run on this plan");
            return -1;
        }
        LSN_HIP(hipSetDevice(p->device));
        hipStream_t s = lsn::as_stream(stream);
        const int n = p->n_maps;
        std::vector<int> off((size_t)n + 1);
        LSN_HIP(hipMemcpyAsync(off.data(), p->ix_off.as<int>() + (size_t)tick * (n + 1), sizeof(int) * (n + 1), hipMemcpyDeviceToHost, s));
        const size_t pix = (size_t)p->tick_depth_elems;
        if (reprojected)
            LSN_HIP(hipMemcpyAsync(reprojected, p->mg_depth0.as<unsigned short>() + (size_t)tick * pix, sizeof(unsigned short) * pix, hipMemcpyDeviceToHost, s));
        if (merged) LSN_HIP(hipMemcpyAsync(merged, p->mg_depth.as<unsigned short>() + (size_t)tick * pix, sizeof(unsigned short) * pix, hipMemcpyDeviceToHost, s));
        std::vector<unsigned char> asg((size_t)p->cap);
        LSN_HIP(hipMemcpyAsync(asg.data(), p->mg_assigned.as<unsigned char>() + (size_t)tick * p->cap, (size_t)p->cap, hipMemcpyDeviceToHost, s));
        LSN_HIP(hipStreamSynchronize(s));
        const int nv = std::min<long long>(std::max(off[n], 0), p->cap);
        int count = 0;
        for (int v = 0; v < nv; v++) count += asg[v] != 0;
        if (assigned) memcpy(assigned, asg.data(), (size_t)nv);
        return count;
    });
}
