// wire.hip -- the data formats either side of the fusion path, part 3 of include/NativeUtils.h.
//
//   inbound  : the client's frame message (LiveScanClient::SerializeFrame, src/LiveScanClient/liveScanClient.cpp:185-290,
//              read by KinectSocket.ReceiveFrame, LiveScanServer/KinectSocket.cs:211-304) and the client's recording file
//              (src/LiveScanClient/frameFileWriterReader.cpp:59-82,115-130).  Host-side parsing only; zstd is the system
//              libzstd.so.1 loaded at run time (the reference P/Invokes libzstd.dll the same way, ZSTDDecompressor.cs:13-31).
//   outbound : the TransferServer stream (formVerticesChunks / formMeshChunks, LiveScanServer/TransferServer.cs:177-270, and
//              TransferSocket.SendFrame, LiveScanServer/TransferSocket.cs:50-104) and the binary PLY writer
//              (LiveScanServer/Utils.cs:222-262), built ON THE DEVICE from a cloud / mesh that is already in HBM, so that one
//              D2H copy yields the bytes to put on the socket / in the file.
//
// One translation unit of five files.  This one holds what the parts share (the chunk limit, the stream's layout, the reference's chunk
// counters) and the LsnTransfer handle with its exports; it includes wire_stream.hip (the byte-stream stores, the two assemble kernels, the
// PLY exports), wire_walk.hip and wire_link.hip (formMeshChunks chunk after chunk and from prefix sums: device code and host driver each,
// behind the handle, which they use) and, at its end, wire_inbound.hip (zstd and the parsers: host code only).
#include "lsn_common.hpp"
#include "wave_ops.hpp"

#include <dlfcn.h>

#include <array>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

namespace {

constexpr int kChunkLimit = 65000 - 3;                       // TransferServer.cs:179,205
constexpr int kItemsPerBlock = 1024;                         // assemble kernels: vertices / faces per block (4 per thread)

template <class A, class B> __host__ __device__ constexpr auto div_up(A n, B k) { return (n + k - 1) / k; }

// SendFrame's stream: [3 ints][v chunk sizes][t chunk sizes][xyz f32 x 3 x n][rgb u8 x 3 x n][tri i32 x 3 x nT] -- where its sections begin
// and where it ends (TransferSocket.cs:92-99)
struct StreamLayout {
    long long xyz, rgb, tri, end;
    __host__ __device__ StreamLayout(long long n_chunks, long long n_send, long long n_tri) : xyz(12 + 8 * n_chunks), rgb(xyz + 12 * n_send), tri(rgb + 3 * n_send), end(tri + 12 * n_tri) {}
};

// no mesh of nv vertices and nt triangles has more chunks than this: a chunk closes with at least 64997 vertices, or is the last
long long chunk_bound(long long nv, long long nt) { return 3 * nt / kChunkLimit + nv / kChunkLimit + 2; }

int bad_index(int n_vertices) { lsn::set_error("lsnTransferPack: a triangle index lies outside [0, %d)", n_vertices); return -1; }

// The reference's chunk counters and what it does with them where a chunk closes (TransferServer.cs:239-246) and where the mesh ends
// (:256-260).  The two paths find the triangle that ends a chunk each in their own way; both close the chunk here.  write: this thread
// stores the sizes (every thread that calls keeps the counters).
struct ChunkCursor {
    int *v_chunks, *t_chunks;
    int c = 0, vbase = 0, tri_start = 0;   // chunks closed, the vertices in them, trianglesChunkStart in index positions (:213)
    __device__ void add(int vcount, int tcount, bool write) { if (write) { v_chunks[c] = vcount; t_chunks[c] = tcount; } c++; vbase += vcount; }
    __device__ void close(int e, int vcount, bool write)   // triangle e is the chunk's last
    {
        const int t = 3 * e + 2;                              // the t of :239-246: e's last index position
        add(vcount, (t - tri_start) / 3, write);
        tri_start = t;                                        // sic (:244): not t + 1, so the first chunk's count comes out one short
    }
    __device__ void end_of_mesh(int nT, int vcount, bool write) { if (vcount != 0) add(vcount, (3 * nT - tri_start) / 3, write); }
};

struct ChunkState;   // wire_walk.hip
struct LinkState;    // wire_link.hip

// what a path leaves for the assemble kernel
struct Chunked { const uint4 *verts; const int *tri; int n_send, n_chunks; };

}  // namespace

struct LsnTransfer {
    int device = 0;
    int max_v = 0, max_t = 0, max_chunks = 0;
    lsn::DevBuf tag, lidx, new_v, new_tri, bsum, boff, v_chunks, t_chunks, state;
    lsn::DevBuf l_cnt, l_uses, l_prev, l_pack, l_totals, l_rank, l_start, l_vbase, l_state;   // the link path
    ChunkState *h_state = nullptr;      // pinned
    LinkState *h_link = nullptr;        // pinned
    int last_path = 0;                  // 0: vertices only, 1: link path, 2: window walk
    std::mutex mu;
    // every buffer, named once, with the bytes the handle's capacity asks of it (behind the parts: it needs their constants)
    std::array<std::pair<lsn::DevBuf *, size_t>, 18> bufs();
    Chunked out(int n_send, int n_chunks) const { return {new_v.as<uint4>(), new_tri.as<int>(), n_send, n_chunks}; }
    ~LsnTransfer() {
        if (h_state) (void)hipHostFree(h_state);
        if (h_link) (void)hipHostFree(h_link);
    }
};

// makes `device` current; -1 with the message where there is none
static int use_device(const char *who, int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { lsn::set_error("%s: no HIP device %d (this library has no CPU path)", who, device); return -1; }
    LSN_HIP(hipSetDevice(device));
    return 0;
}

#include "wire_stream.hip"
#include "wire_walk.hip"
#include "wire_link.hip"

std::array<std::pair<lsn::DevBuf *, size_t>, 18> LsnTransfer::bufs()
{
    const size_t nv = (size_t)(max_v > 0 ? max_v : 1), nt3 = (size_t)(max_t > 0 ? 3ll * max_t : 1), nc = (size_t)max_chunks;
    return {{{&tag, nv * 8}, {&lidx, nv * 4}, {&new_v, nt3 * 16}, {&new_tri, nt3 * 4}, {&bsum, kWindowBlocks * 4}, {&boff, kWindowBlocks * 4},
             {&v_chunks, nc * 4}, {&t_chunks, nc * 4}, {&state, sizeof(ChunkState)},
             {&l_cnt, nv * 4}, {&l_uses, nv * 4 * kMaxUses}, {&l_prev, nt3 * 4 + 32}, {&l_pack, (nt3 / 3 + 8) * 8},
             {&l_totals, (nt3 / kScanPerBlock + 2) * 8}, {&l_rank, nt3 * 4 + 32}, {&l_start, (nc + 1) * 4}, {&l_vbase, (nc + 1) * 4},
             {&l_state, sizeof(LinkState)}}};
}

template <class T> static int pinned_word(T **p)
{
    if (hipHostMalloc(reinterpret_cast<void **>(p), sizeof(T), hipHostMallocDefault) == hipSuccess) return 0;
    lsn::set_error("lsnTransferCreate: hipHostMalloc failed");
    return -1;
}

extern "C" {

LsnTransfer *lsnTransferCreate(int device, int max_vertices, int max_triangles)
{
    return lsn::guarded("lsnTransferCreate", static_cast<LsnTransfer *>(nullptr), [&]() -> LsnTransfer * {
        lsn::clear_error();
        if (max_vertices < 0 || max_triangles < 0) { lsn::set_error("lsnTransferCreate: negative capacity"); return nullptr; }
        if (use_device("lsnTransferCreate", device)) return nullptr;
        auto t = std::make_unique<LsnTransfer>();
        t->device = device;
        t->max_v = max_vertices;
        t->max_t = max_triangles;
        t->max_chunks = (int)chunk_bound(max_vertices, max_triangles);
        for (auto [buf, bytes] : t->bufs())
            if (buf->reserve(bytes)) return nullptr;
        if (pinned_word(&t->h_link) || pinned_word(&t->h_state)) return nullptr;
        return t.release();
    });
}

void lsnTransferDestroy(LsnTransfer *t)
{
    lsn::guarded_void("lsnTransferDestroy", [&]() {
        if (!t) return;
        (void)hipSetDevice(t->device);
        delete t;
    });
}

int lsnTransferLastPath(LsnTransfer *t)
{
    return lsn::guarded("lsnTransferLastPath", -1, [&]() {
        if (!t) return -1;
        std::lock_guard<std::mutex> guard(t->mu);
        return t->last_path;
    });
}

long long lsnTransferFrameBound(int n_vertices, int n_triangles)
{
    return lsn::guarded("lsnTransferFrameBound", -1LL, [&]() -> long long {
        const long long nt = n_triangles > 0 ? n_triangles : 0, nv = n_vertices > 0 ? n_vertices : 0;
        return StreamLayout(chunk_bound(nv, nt), nt > 0 ? 3 * nt : nv, nt).end;
    });
}

long long lsnTransferPack(LsnTransfer *t, const void *d_vertices, int n_vertices, const int *d_triangles, int n_triangles,
                          void *d_out, long long out_cap, void *stream)
{
    return lsn::guarded("lsnTransferPack", -1LL, [&]() -> long long {
        lsn::clear_error();
        if (!t) { lsn::set_error("lsnTransferPack: null handle"); return -1; }
        if (n_vertices < 0 || n_triangles < 0 || n_vertices > t->max_v || n_triangles > t->max_t) {
            lsn::set_error("lsnTransferPack: %d vertices / %d triangles exceed the handle's capacity (%d / %d)", n_vertices, n_triangles, t->max_v, t->max_t);
            return -1;
        }
        if ((n_vertices && !d_vertices) || (n_triangles && !d_triangles) || !d_out) { lsn::set_error("lsnTransferPack: null buffer"); return -1; }
        if (n_triangles > 0 && n_vertices == 0) { lsn::set_error("lsnTransferPack: triangles without vertices"); return -1; }
        std::lock_guard<std::mutex> guard(t->mu);
        LSN_HIP(hipSetDevice(t->device));
        hipStream_t s = lsn::as_stream(stream);
        const Chunked in{static_cast<const uint4 *>(d_vertices), d_triangles, n_vertices, div_up(n_vertices, kChunkLimit)};   // formVerticesChunks (:177-201)
        Chunked m = in;
        if (n_triangles == 0) t->last_path = 0;
        if (n_triangles > 0) {
            int rc = link_fits(*t, n_triangles) ? link_path(*t, in, n_triangles, s, m) : 1;   // 1: the walk forms the chunks
            if (rc == 0) t->last_path = 1;
            if (rc == 1) {
                t->last_path = 2;
                rc = walk_path(*t, in, n_triangles, s, m);
            }
            if (rc) return -1;
        }
        const long long need = StreamLayout(m.n_chunks, m.n_send, n_triangles).end;
        if (need > out_cap) { lsn::set_error("lsnTransferPack: the stream needs %lld bytes, the buffer holds %lld", need, out_cap); return -1; }
        if (((size_t)d_out & 3) != 0) { lsn::set_error("lsnTransferPack: d_out must be 4-byte aligned"); return -1; }
        const int xb = div_up(m.n_send, kItemsPerBlock), cb = xb, tb = (int)div_up(3ll * n_triangles, kItemsPerBlock * 3);
        transfer_assemble_kernel<<<xb + cb + tb + 1, 256, 0, s>>>(m.verts, m.n_send, m.tri, n_triangles, m.n_chunks, t->v_chunks.as<int>(), t->t_chunks.as<int>(),
                                                                   n_triangles == 0, static_cast<unsigned char *>(d_out), xb, cb, tb);
        LSN_HIP(hipGetLastError());
        LSN_HIP(hipStreamSynchronize(s));
        return need;
    });
}

}  // extern "C"

#include "wire_inbound.hip"
