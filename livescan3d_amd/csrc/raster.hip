// raster.hip -- drawTriangle (src/NativeUtils/depthprocessing.cpp:598-706) for one triangle of projected vertices: its 28.4 set-up, fill
// rule, barycentric weights and depth value, for render view (render.hip), and the float -> u16 conversion it shares with the overlay merge.  mg_raster_kernel
// (merge.hip) keeps the same arithmetic written out in its loop, for its speed: a change to it is made here AND there.
// Compiled as part of mesh.hip's translation unit (after cloud_index.hip, ahead of merge.hip and render.hip).
#include "fusion_shared.hpp"

namespace {

// (unsigned short)v of a float as x64 code computes it: cvttss2si (truncation; INT_MIN for NaN and anything out of int32), then the
// low 16 bits.  gfx950's v_cvt_u32_f32 / v_cvt_i32_f32 saturate instead.
__device__ __forceinline__ unsigned int cvt_u16_x64(float v)
{
    const int i = (v >= -2147483648.0f && v < 2147483648.0f) ? (int)v : (int)0x80000000u;
    return (unsigned int)i & 0xFFFFu;
}

// What drawTriangle derives before its loops (:602-666).  A projected vertex is {x | y << 16, d}; d = 0: not drawable.
struct TriSetup {
    int C1, C2, C3, DX12, DX23, DX31, DY12, DY23, DY31;   // the half-space values at (0, 0) and their steps
    int minx, maxx, miny, maxy, x3, y3;                   // the box, half-open
    float fden, y23, x32, y31, x13, fd1, fd2, fd3;
};

// false: nothing is drawn (a vertex that is not drawable, :885-886, or den == 0)
__device__ __forceinline__ bool tri_setup(const int2 p1, const int2 p2, const int2 p3, TriSetup &s)
{
    if (p1.y == 0 || p2.y == 0 || p3.y == 0) return false;
    const int x1 = p1.x & 0xFFFF, y1 = p1.x >> 16, x2 = p2.x & 0xFFFF, y2 = p2.x >> 16, x3 = p3.x & 0xFFFF, y3 = p3.x >> 16;
    // 28.4 fixed point of integer positions (:602-609: iround(16.0f * v) is exact)
    const int X1 = 16 * x1, X2 = 16 * x2, X3 = 16 * x3, Y1 = 16 * y1, Y2 = 16 * y2, Y3 = 16 * y3;
    s.DX12 = X1 - X2; s.DX23 = X2 - X3; s.DX31 = X3 - X1;
    s.DY12 = Y1 - Y2; s.DY23 = Y2 - Y3; s.DY31 = Y3 - Y1;
    s.minx = (min(min(X1, X2), X3) + 0xF) >> 4; s.maxx = (max(max(X1, X2), X3) + 0xF) >> 4;   // :629-632, half-open
    s.miny = (min(min(Y1, Y2), Y3) + 0xF) >> 4; s.maxy = (max(max(Y1, Y2), Y3) + 0xF) >> 4;
    s.C1 = s.DY12 * X1 - s.DX12 * Y1; s.C2 = s.DY23 * X2 - s.DX23 * Y2; s.C3 = s.DY31 * X3 - s.DX31 * Y3;   // :639-641
    if (s.DY12 < 0 || (s.DY12 == 0 && s.DX12 > 0)) s.C1++;   // fill convention (:644-646)
    if (s.DY23 < 0 || (s.DY23 == 0 && s.DX23 > 0)) s.C2++;
    if (s.DY31 < 0 || (s.DY31 == 0 && s.DX31 > 0)) s.C3++;
    const int den = (y2 - y3) * (x1 - x3) + (x3 - x2) * (y1 - y3);   // :656, :660 (int, then float; den1 == den2)
    if (den == 0) return false;                                      // :662-663
    s.fden = (float)den; s.y23 = (float)(y2 - y3); s.x32 = (float)(x3 - x2); s.y31 = (float)(y3 - y1); s.x13 = (float)(x1 - x3);
    s.fd1 = (float)p1.y; s.fd2 = (float)p2.y; s.fd3 = (float)p3.y;
    s.x3 = x3; s.y3 = y3;
    return true;
}

// The three half-space values at pixel (x, y) (:648-650, :697-703 in closed form -- the same int32 numbers the reference reaches by
// stepping CX by DY << 4 along x and CY by DX << 4 along y).
__device__ __forceinline__ void tri_edges(const TriSetup &s, int x, int y, int &e1, int &e2, int &e3)
{
    e1 = s.C1 + s.DX12 * (y << 4) - s.DY12 * (x << 4);
    e2 = s.C2 + s.DX23 * (y << 4) - s.DY23 * (x << 4);
    e3 = s.C3 + s.DX31 * (y << 4) - s.DY31 * (x << 4);
}

__device__ __forceinline__ bool tri_covers(const TriSetup &s, int x, int y)
{
    int e1, e2, e3;
    tri_edges(s, x, y, e1, e2, e3);
    return e1 >= 0 && e2 >= 0 && e3 >= 0;
}

// Pixel (x, y)'s weights and its depth value (:671-682, the reference's operation order).
__device__ __forceinline__ unsigned int tri_value(const TriSetup &s, int x, int y, float &w1, float &w2, float &w3)
{
    const float term21 = __fmul_rn(s.x32, (float)(y - s.y3)), term22 = __fmul_rn(s.x13, (float)(y - s.y3));   // :671-672
    w1 = __fdiv_rn(__fadd_rn(__fmul_rn(s.y23, (float)(x - s.x3)), term21), s.fden);                           // :677-679
    w2 = __fdiv_rn(__fadd_rn(__fmul_rn(s.y31, (float)(x - s.x3)), term22), s.fden);
    w3 = __fsub_rn(__fsub_rn(1.0f, w1), w2);
    return cvt_u16_x64(__fadd_rn(__fadd_rn(__fmul_rn(s.fd1, w1), __fmul_rn(s.fd2, w2)), __fmul_rn(s.fd3, w3)));   // :682
}

}  // namespace
