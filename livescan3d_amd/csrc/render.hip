// render.hip -- "render view": a tick's merged mesh (or its vertices alone) drawn from virtual pinhole cameras into sensor-like frames
// (u16 depth in mm + RGB8): lsnFusionRenderViews, lsnFusionRenderDiagnostics and what lsnLastMeshRenderView runs.
//
// The reference shows the merged mesh in an OpenGL window (LiveScanServer's OpenGLWindow); this device has no rasteriser and no display,
// so the stage is DEFINED here, from pieces that are pinned to the reference: pointProjection with the view's inverted pose (project,
// cloud_index.hip) and drawTriangle's fill rule, barycentric weights and depth value (src/NativeUtils/depthprocessing.cpp:598-706:
// raster.hip, the arithmetic mg_raster_kernel of merge.hip has in its loop).  What is new: a plain z-buffer -- per pixel the candidate of smallest
// (val, primitive index) wins, candidates of val 0 are skipped -- and the winner's colour, interpolated with the same weights.  No clipping: a triangle
// with a vertex outside the image, behind the camera or closer than 1 mm is dropped.  Per view, over every tick of the batch:
//
//   1. projection (rv_project_kernel): every vertex into the view; mesh mode keeps {x | y << 16, d} (d = 0: not drawable), points mode
//      puts (d << 32 | vertex) straight into the pixel's key.
//   2. raster (rv_raster_kernel, mesh mode): one lane per triangle.  A bounding box of at most kRvSmallBox pixels is walked by the lane;
//      a larger one goes to the tick's work list (one returning atomic per wave, plain stores), which rv_large_kernel then draws with one
//      wave per triangle, lanes striding the box.  Both do a 64-bit atomicMin of (val << 32 | triangle) on the pixel's key: the image
//      does not depend on the order of the launches' lanes or of the list.
//   3. resolve (rv_resolve_kernel): per pixel the winner's weights again (tri_value, the function the raster passes called), depth and
//      colour out, the key back to "none".
//
// Every loop is bounded by the view size or by a count that an earlier kernel of the stream left; no kernel waits for another workgroup.
// Compiled as part of mesh.hip's translation unit (after cloud_index.hip, raster.hip and mesh_batch.hip: project, drawTriangle, the batch).
#include "fusion_shared.hpp"

namespace {

constexpr int kRvMaxViews = 16;
constexpr int kRvMaxSide = 1024;      // the largest sensor side the project handles: 16 * 1024 * 16 * 1024 = 2^28, every 28.4 product stays in int32
constexpr int kRvBlocks = 1024;       // workgroups per tick of the two raster kernels (grid-stride / wave-stride)
#ifndef LSN_RV_SMALL_BOX
#define LSN_RV_SMALL_BOX 16
#endif
// Bounding boxes up to this many pixels are walked by the triangle's own lane, larger ones by a whole wave (a build with
// -DLSN_RV_SMALL_BOX=2147483647 lists nothing: the A/B of EXPERIMENTS.md "Render view", which also says why 16 is not the last word).
constexpr int kRvSmallBox = LSN_RV_SMALL_BOX;
constexpr unsigned long long kRvNone = ~0ull;

struct RvArgs {
    SensorParams view;             // the view's camera, packed like a sensor's
    lsn::MeshBatch m;              // what is drawn; m.tri null in points mode
    int2 *proj;                    // [n_ticks][tick_vert]: {x | y << 16, d} in this view, d = 0: not drawable
    unsigned long long *key;       // [n_ticks][n_views][w * h]: min (val << 32 | primitive), kRvNone = nothing drawn
    int *list;                     // [n_ticks][tick_tri]: the triangles of large boxes
    int *cnt;                      // [n_ticks][n_views][4]: listed triangles, primitives drawn, pixels with depth != 0
    unsigned short *depth_out;     // [n_ticks][n_views][h][w]
    unsigned char *color_out;      // [n_ticks][n_views][h][w][3]
    int n_views, view_index, w, h;
};

__device__ __forceinline__ long long rv_slot(const RvArgs &a, int tick) { return (long long)tick * a.n_views + a.view_index; }

// The candidate of pixel (x, y), if the triangle covers it with a val other than 0.
__device__ __forceinline__ void rv_draw(const TriSetup &s, int x, int y, int t, unsigned long long *key, int w)
{
    if (!tri_covers(s, x, y)) return;
    float w1, w2, w3;
    const unsigned int val = tri_value(s, x, y, w1, w2, w3);
    if (val != 0) atomicMin(&key[(long long)y * w + x], ((unsigned long long)val << 32) | (unsigned int)t);
}

// ---- 1. projection ----------------------------------------------------------------------------------------------------------------
template <bool POINTS>
__global__ __launch_bounds__(256) void rv_project_kernel(RvArgs a)
{
    const int tick = blockIdx.y;
    const int nv = mesh_count(a.m.voff, tick, a.m.n, a.m.tick_vert);
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = false;
    if (g < nv) {
        const uint4 v = a.m.verts[tick * a.m.tick_vert + g];
        int x, y, d;
        project(a.view, __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w), x, y, d);
        ok = x >= 0 && x < a.w && y >= 0 && y < a.h && d != 0;
        if (POINTS) {
            if (ok) atomicMin(&a.key[rv_slot(a, tick) * a.w * a.h + (long long)y * a.w + x], ((unsigned long long)(unsigned int)d << 32) | (unsigned int)g);
        } else {
            a.proj[tick * a.m.tick_vert + g] = ok ? make_int2(x | (y << 16), d) : make_int2(0, 0);
        }
    }
    if (POINTS) {   // primitives drawn: one add per wave
        const int drawn = __popcll(__ballot(ok));
        if ((threadIdx.x & 63) == 0 && drawn) atomicAdd(&a.cnt[rv_slot(a, tick) * 4 + 1], drawn);
    }
}

// ---- 2. raster ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rv_raster_kernel(RvArgs a)
{
    const int tick = blockIdx.y;
    const int nv = mesh_count(a.m.voff, tick, a.m.n, a.m.tick_vert), nt = mesh_count(a.m.toff, tick, a.m.n, a.m.tick_tri);
    const int *tri = a.m.tri + 3 * tick * a.m.tick_tri;
    const int2 *proj = a.proj + tick * a.m.tick_vert;
    unsigned long long *key = a.key + rv_slot(a, tick) * a.w * a.h;
    int *list = a.list + tick * a.m.tick_tri;
    int *cnt = a.cnt + rv_slot(a, tick) * 4;
    const int lane = threadIdx.x & 63;
    int drawn = 0;
    // whole waves take the loop together (the work list's ballot below): the bound is rounded up to the wave
    const int stride = gridDim.x * blockDim.x;
    for (int t0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63); t0 < nt; t0 += stride) {
        const int t = t0 + lane;
        bool large = false;
        TriSetup s;
        if (t < nt) {
            const int i1 = tri[3 * t], i2 = tri[3 * t + 1], i3 = tri[3 * t + 2];
            if ((unsigned int)i1 < (unsigned int)nv && (unsigned int)i2 < (unsigned int)nv && (unsigned int)i3 < (unsigned int)nv) {
                const int2 p1 = proj[i1], p2 = proj[i2], p3 = proj[i3];
                drawn += p1.y != 0 && p2.y != 0 && p3.y != 0;
                if (tri_setup(p1, p2, p3, s)) {
                    if ((s.maxx - s.minx) * (s.maxy - s.miny) > kRvSmallBox) {
                        large = true;
                    } else {
                        for (int y = s.miny; y < s.maxy; y++)
                            for (int x = s.minx; x < s.maxx; x++) rv_draw(s, x, y, t, key, a.w);
                    }
                }
            }
        }
        const unsigned long long m = __ballot(large);
        if (m) {   // wave-uniform
            int base = 0;
            if (lane == 0) base = atomicAdd(&cnt[0], __popcll(m));
            base = __shfl(base, 0, 64);
            if (large) list[base + __popcll(m & ((1ull << lane) - 1ull))] = t;   // < nt <= tick_tri entries in all: every triangle is listed at most once
        }
    }
    drawn = wave_sum(drawn);
    if (lane == 0 && drawn) atomicAdd(&cnt[1], drawn);
}

// The listed triangles: one wave each, lanes striding the box.
__global__ __launch_bounds__(256) void rv_large_kernel(RvArgs a)
{
    const int tick = blockIdx.y;
    const int *cnt = a.cnt + rv_slot(a, tick) * 4;
    const int n_list = min(cnt[0], (int)a.m.tick_tri);   // left by rv_raster_kernel, a launch earlier
    const int *tri = a.m.tri + 3 * tick * a.m.tick_tri;
    const int2 *proj = a.proj + tick * a.m.tick_vert;
    unsigned long long *key = a.key + rv_slot(a, tick) * a.w * a.h;
    const int *list = a.list + tick * a.m.tick_tri;
    const int lane = threadIdx.x & 63, waves = (int)(gridDim.x * blockDim.x) >> 6;
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n_list; i += waves) {
        const int t = list[i];
        TriSetup s;
        if (!tri_setup(proj[tri[3 * t]], proj[tri[3 * t + 1]], proj[tri[3 * t + 2]], s)) continue;   // (listed: it was drawable)
        const int bw = s.maxx - s.minx, npx = bw * (s.maxy - s.miny);   // <= 1024 * 1024
        for (int j = lane; j < npx; j += 64) {
            const int r = j / bw;
            rv_draw(s, s.minx + (j - r * bw), s.miny + r, t, key, a.w);
        }
    }
}

// ---- 3. resolve ---------------------------------------------------------------------------------------------------------------------
template <bool POINTS>
__global__ __launch_bounds__(256) void rv_resolve_kernel(RvArgs a)
{
    const int tick = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int npix = a.w * a.h;
    bool hit = false;
    if (i < npix) {
        const long long q = rv_slot(a, tick) * npix + i;
        const unsigned long long k = a.key[q];
        unsigned int d = 0, r = 0, g = 0, b = 0;
        if (k != kRvNone) {
            const int t = (int)(unsigned int)k;
            const uint4 *verts = a.m.verts + tick * a.m.tick_vert;
            d = (unsigned int)(k >> 32);
            if (POINTS) {
                const unsigned int c = verts[t].x;
                r = c & 0xFFu; g = (c >> 8) & 0xFFu; b = (c >> 16) & 0xFFu;
            } else {
                const int *tr = a.m.tri + 3 * (tick * a.m.tick_tri + t);
                const int i1 = tr[0], i2 = tr[1], i3 = tr[2];
                const int2 *proj = a.proj + tick * a.m.tick_vert;
                TriSetup s;
                float w1 = 0.0f, w2 = 0.0f, w3 = 0.0f;
                if (tri_setup(proj[i1], proj[i2], proj[i3], s) && tri_covers(s, i % a.w, i / a.w)) (void)tri_value(s, i % a.w, i / a.w, w1, w2, w3);
                const unsigned int c1 = verts[i1].x, c2 = verts[i2].x, c3 = verts[i3].x;
                auto mix = [&](int sh) -> unsigned int {
                    const float f1 = (float)((c1 >> sh) & 0xFFu), f2 = (float)((c2 >> sh) & 0xFFu), f3 = (float)((c3 >> sh) & 0xFFu);
                    const float v = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(f1, w1), __fmul_rn(f2, w2)), __fmul_rn(f3, w3)), 0.5f);
                    return (unsigned int)min(max((int)v, 0), 255);
                };
                r = mix(0); g = mix(8); b = mix(16);
            }
            a.key[q] = kRvNone;
        }
        hit = d != 0;
        a.depth_out[q] = (unsigned short)d;
        unsigned char *c = a.color_out + 3 * q;
        c[0] = (unsigned char)r; c[1] = (unsigned char)g; c[2] = (unsigned char)b;
    }
    const int n_hit = __popcll(__ballot(hit));
    if ((threadIdx.x & 63) == 0 && n_hit) atomicAdd(&a.cnt[rv_slot(a, tick) * 4 + 2], n_hit);
}

}  // namespace

namespace lsn {

// The stage on a batch, with `rs` as its scratch; the caller holds whatever lock guards `rs` and has made its device current.
int render_views(RenderScratch &rs, const char *who, const MeshBatch &m, int n_views, const float *intr_params, const float *wtransform_params,
                 int width, int height, void *d_depth_out, void *d_colors_out, hipStream_t s)
{
    if (!intr_params || !wtransform_params || !m.verts || !m.voff || !d_depth_out || !d_colors_out || (m.tri && !m.toff)) {
        lsn::set_error("%s: null argument", who);
        return -1;
    }
    if (n_views < 1 || n_views > kRvMaxViews) {
        lsn::set_error("%s: 1 to %d views per call (got %d)", who, kRvMaxViews, n_views);
        return -1;
    }
    if (width < 1 || width > kRvMaxSide || height < 1 || height > kRvMaxSide) {
        lsn::set_error("%s: a view is 1x1 to %dx%d pixels (got %dx%d)", who, kRvMaxSide, kRvMaxSide, width, height);
        return -1;
    }
    if (check_batch(who, m)) return -1;
    const bool points = m.tri == nullptr;
    const int n_ticks = m.n_ticks;
    const size_t npix = (size_t)width * height, slots = (size_t)n_ticks * n_views;
    if (rs.cnt.begin((size_t)n_ticks * kRvMaxViews, slots, s) ||
        (!points && (rs.proj.reserve(sizeof(int2) * (size_t)n_ticks * (size_t)std::max(m.tick_vert, 1LL)) ||
                     rs.list.reserve(sizeof(int) * (size_t)n_ticks * (size_t)std::max(m.tick_tri, 1LL)))))
        return -1;
    // the keys last, and their flag right behind them: a call that fails further down must not leave a fresh block marked clean
    const size_t key_bytes_before = rs.key.bytes;
    const int key_rc = rs.key.reserve(sizeof(unsigned long long) * slots * npix);
    if (rs.key.bytes != key_bytes_before) rs.keys_clean = false;
    if (key_rc) return -1;
    if (!rs.keys_clean) LSN_HIP(hipMemsetAsync(rs.key.p, 0xFF, rs.key.bytes, s));
    rs.keys_clean = false;   // until every resolve pass of this call is queued: they leave the keys at "none"
    RvArgs a;
    a.m = m;
    a.proj = rs.proj.as<int2>();
    a.key = rs.key.as<unsigned long long>();
    a.list = rs.list.as<int>();
    a.cnt = rs.cnt.buf.as<int>();
    a.depth_out = static_cast<unsigned short *>(d_depth_out);
    a.color_out = static_cast<unsigned char *>(d_colors_out);
    a.n_views = n_views;
    a.w = width;
    a.h = height;
    const unsigned int vblocks = (unsigned int)((m.tick_vert + 255) / 256), pblocks = (unsigned int)((npix + 255) / 256);
    const unsigned int tblocks = (unsigned int)std::min<long long>(kRvBlocks, (m.tick_tri + 255) / 256);
    for (int v = 0; v < n_views; v++) {
        pack_sensor_params(intr_params + 7 * v, wtransform_params + 12 * v, a.view);
        a.view_index = v;
        // the views take turns on `proj` and `list`: a view's passes are queued behind the passes of the one before it
        if (points) {
            if (vblocks) hipLaunchKernelGGL(rv_project_kernel<true>, dim3(vblocks, n_ticks), dim3(256), 0, s, a);
            hipLaunchKernelGGL(rv_resolve_kernel<true>, dim3(pblocks, n_ticks), dim3(256), 0, s, a);
        } else {
            if (vblocks) hipLaunchKernelGGL(rv_project_kernel<false>, dim3(vblocks, n_ticks), dim3(256), 0, s, a);
            if (vblocks && tblocks) {
                hipLaunchKernelGGL(rv_raster_kernel, dim3(tblocks, n_ticks), dim3(256), 0, s, a);
                hipLaunchKernelGGL(rv_large_kernel, dim3(tblocks, n_ticks), dim3(256), 0, s, a);
            }
            hipLaunchKernelGGL(rv_resolve_kernel<false>, dim3(pblocks, n_ticks), dim3(256), 0, s, a);
        }
    }
    LSN_HIP(hipGetLastError());
    rs.keys_clean = true;
    rs.cnt.finish(n_ticks, n_views);
    return 0;
}

// {primitives drawn, listed triangles, pixels with depth != 0} of (tick, view) of the last render with `rs`; synchronises `s`.
int render_counts(RenderScratch &rs, const char *who, int tick, int view, int *n_drawn, int *n_large, int *n_pixels, hipStream_t s)
{
    int c[4] = {0, 0, 0, 0};
    if (rs.cnt.read(who, "nothing has been rendered yet", tick, view, c, s, [&] {
            lsn::set_error("%s: the last render had %d ticks and %d views (asked for tick %d, view %d)", who, rs.cnt.ticks, rs.cnt.per_tick, tick, view);
        }))
        return -1;
    if (n_large) *n_large = c[0];
    if (n_drawn) *n_drawn = c[1];
    if (n_pixels) *n_pixels = c[2];
    return 0;
}

}  // namespace lsn

extern "C" int lsnFusionRenderViews(LsnFusion *p, int n_views, const float *intr_params, const float *wtransform_params, int width, int height,
                                    const void *d_vertices, const int *d_offsets, const void *d_triangles, const int *d_tri_offsets,
                                    void *d_depth_out, void *d_colors_out, void *stream)
{
    return plan_export("lsnFusionRenderViews", p, [&] {
        return lsn::render_views(p->rv, "lsnFusionRenderViews", plan_batch(p, d_vertices, d_offsets, d_triangles, d_tri_offsets), n_views, intr_params,
                                 wtransform_params, width, height, d_depth_out, d_colors_out, lsn::as_stream(stream));
    });
}

extern "C" int lsnFusionRenderDiagnostics(LsnFusion *p, int tick, int view, int *n_drawn, int *n_large, int *n_pixels, void *stream)
{
    return plan_export("lsnFusionRenderDiagnostics", p, [&] {
        return lsn::render_counts(p->rv, "lsnFusionRenderDiagnostics", tick, view, n_drawn, n_large, n_pixels, lsn::as_stream(stream));
    });
}
