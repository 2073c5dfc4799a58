// refine_xyz.hip -- a merged cloud's vertices as the packed XYZ points the refine pass works on.  Compiled as part of icp.hip's translation
// unit (refine.hip includes it, in front of the refine pass).
//
// refineWorker_DoWork strips X, Y, Z out of every sensor's VertexC4ubV3f list on the host (LiveScanServer/MainWindowForm.cs:318-327) before
// the Gauss-Seidel loop.  A tick's merged cloud lies in HBM in sensor order then raster order, so ONE launch over [0, nVertices) leaves every
// sensor's points at 3 * offsets[i] floats: the concatenation the loop's cloud buffer holds anyway.
// Bandwidth bound and tiny (8 x 512x424 scene frames: about 15 MB in, 11 MB out -- microseconds in a pass of milliseconds): a lane reads
// its vertex as one 16-byte word (the compiler drops the colour dword: one three-dword load at a 16-byte stride) and stores the last three
// dwords as one 12-byte word; consecutive lanes store consecutive 12-byte words, a wave 768 contiguous bytes.  The coordinates travel as
// integers: the same bits come out, whatever they encode.

namespace {

struct Xyz {   // 12 bytes, dword aligned: one three-dword store
    unsigned x, y, z;
};

constexpr int kXyzThreads = 256;
constexpr int kXyzMaxBlocks = 2048;   // 256 CUs x 8 workgroups; the grid-stride loop takes the rest

// vertices: n x 16 bytes, 16-byte aligned; xyz: n x 12 bytes.  Every lane checks its own index: nothing is read or written beyond n.
__global__ void __launch_bounds__(kXyzThreads) xyz_of_vertices_kernel(const uint4 *__restrict__ vertices, Xyz *__restrict__ xyz, int n)
{
    for (long long v = (long long)blockIdx.x * kXyzThreads + threadIdx.x; v < n; v += (long long)gridDim.x * kXyzThreads) {
        const uint4 q = vertices[v];   // {R G B A, X, Y, Z}
        xyz[v] = Xyz{q.y, q.z, q.w};
    }
}

// Queues the launch on `s`.  0, or -1 with the message set.
int xyz_of_vertices(const void *d_vertices, float *d_xyz, int n, hipStream_t s)
{
    if (n <= 0) return 0;
    int blocks = (n + kXyzThreads - 1) / kXyzThreads;
    if (blocks > kXyzMaxBlocks) blocks = kXyzMaxBlocks;
    hipLaunchKernelGGL(xyz_of_vertices_kernel, dim3(blocks), dim3(kXyzThreads), 0, s, static_cast<const uint4 *>(d_vertices),
                       reinterpret_cast<Xyz *>(d_xyz), n);
    LSN_HIP(hipGetLastError());
    return 0;
}

}  // namespace
