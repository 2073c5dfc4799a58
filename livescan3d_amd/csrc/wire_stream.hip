// wire_stream.hip -- part of wire.hip's translation unit: the outbound bytes.  How a workgroup stores a run of bytes composed in LDS at any
// alignment, the kernel that writes the binary PLY file (LiveScanServer/Utils.cs:222-262) with its four exports, and the kernel that writes
// TransferSocket.SendFrame's stream (LiveScanServer/TransferSocket.cs:50-104) from what lsnTransferPack's paths left (wire.hip launches it).

namespace {
// ---- byte-stream stores -------------------------------------------------------------------------------------------------------
// Writes nbytes composed in LDS (dword 0 = stream byte 0; one readable dword past the end) to an arbitrarily aligned
// destination: single bytes up to the first aligned dword, then aligned dwords rebuilt from two LDS words with
// v_alignbyte_b32, then the tail bytes.  Coalesced regardless of the section's byte offset inside the message.
__device__ __forceinline__ unsigned lds_byte(const unsigned *lds, int i) { return (lds[i >> 2] >> (8 * (i & 3))) & 0xffu; }

__device__ __forceinline__ void block_stream_store(unsigned char *dst, const unsigned *lds, int nbytes)
{
    int head = (int)((4 - ((size_t)dst & 3)) & 3);
    if (head > nbytes) head = nbytes;
    if ((int)threadIdx.x < head) dst[threadIdx.x] = (unsigned char)lds_byte(lds, threadIdx.x);
    const int nw = (nbytes - head) >> 2;
    unsigned *d32 = reinterpret_cast<unsigned *>(dst + head);
    for (int j = threadIdx.x; j < nw; j += blockDim.x) {
        const unsigned lo = lds[j], hi = lds[j + 1];
        d32[j] = head ? __builtin_amdgcn_alignbyte(hi, lo, (unsigned)head) : lo;
    }
    for (int i = head + 4 * nw + threadIdx.x; i < nbytes; i += blockDim.x) dst[i] = (unsigned char)lds_byte(lds, i);
}

// ORs a 32-bit value into a word array at a compile-time byte offset
template <int OFF> __device__ __forceinline__ void put32(unsigned *w, unsigned v)
{
    w[OFF >> 2] |= v << (8 * (OFF & 3));
    if constexpr ((OFF & 3) != 0) w[(OFF >> 2) + 1] |= v >> (32 - 8 * (OFF & 3));
}
template <int OFF> __device__ __forceinline__ void put8(unsigned *w, unsigned v) { w[OFF >> 2] |= (v & 0xffu) << (8 * (OFF & 3)); }

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a lane's records one after the other, each with its index as a
// compile-time constant, which put32<OFF> / put8<OFF> need
template <class F, int... I>
__device__ __forceinline__ void for_each_record(F &&f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }

// record I of a lane: {R,G,B,A | X | Y | Z} -> {X, Y, Z, R, G, B} = 15 bytes (Utils.cs:248-254); NORMALS: {X, Y, Z, nx, ny, nz, R, G, B} =
// 27 bytes (lsnPlyPackNormals; n: the vertex's three floats, null behind the last vertex)
template <int I, bool NORMALS> __device__ __forceinline__ void ply_vertex(unsigned *w, const uint4 v, const float *n)
{
    constexpr int XYZ = (NORMALS ? 27 : 15) * I, RGB = XYZ + (NORMALS ? 24 : 12);
    put32<XYZ + 0>(w, v.y);
    put32<XYZ + 4>(w, v.z);
    put32<XYZ + 8>(w, v.w);
    if constexpr (NORMALS) {
        put32<XYZ + 12>(w, n ? __float_as_uint(n[0]) : 0u);
        put32<XYZ + 16>(w, n ? __float_as_uint(n[1]) : 0u);
        put32<XYZ + 20>(w, n ? __float_as_uint(n[2]) : 0u);
    }
    put8<RGB + 0>(w, v.x);
    put8<RGB + 1>(w, v.x >> 8);
    put8<RGB + 2>(w, v.x >> 16);
}

template <int I> __device__ __forceinline__ void ply_face(unsigned *w, int a, int b, int c)
{
    put8<13 * I + 0>(w, 3u);                                  // (byte)3, then the three indices (Utils.cs:259-262)
    put32<13 * I + 1>(w, (unsigned)a);
    put32<13 * I + 5>(w, (unsigned)b);
    put32<13 * I + 9>(w, (unsigned)c);
}

struct PlyHeader { int len; char text[316]; };

// blocks [0, vb) : vertex records, [vb, vb+fb) : face records, last block: the header text.  NORMALS: the vertex records carry the three
// floats of `normals` between position and colour (27 bytes instead of 15); the face records and everything else are the same.
template <bool NORMALS>
__global__ __launch_bounds__(256) void ply_pack_kernel(const uint4 *__restrict__ verts, const float *__restrict__ normals, int nV,
                                                        const int *__restrict__ tri, int nT, unsigned char *__restrict__ out, PlyHeader hdr,
                                                        int vb, int fb)
{
    constexpr int VB = NORMALS ? 27 : 15;                      // bytes per vertex record; a lane's four are VB words
    __shared__ unsigned lds[kItemsPerBlock * VB / 4 + 1];
    constexpr std::make_integer_sequence<int, 4> four{};
    const int b = blockIdx.x;
    if (b < vb) {
        const int first = b * kItemsPerBlock, n = min(kItemsPerBlock, nV - first);
        const int i0 = first + 4 * threadIdx.x;
        unsigned w[VB + 1] = {};
        for_each_record([&](auto q) {
            const int i = i0 + decltype(q)::value;
            const bool in = i < nV;                            // behind the last vertex: a record of zeros, composed and never stored
            ply_vertex<decltype(q)::value, NORMALS>(w, in ? verts[i] : make_uint4(0, 0, 0, 0), NORMALS && in ? normals + 3 * (size_t)i : nullptr);
        }, four);
#pragma unroll
        for (int q = 0; q < VB; q++) lds[VB * threadIdx.x + q] = w[q];
        __syncthreads();
        block_stream_store(out + hdr.len + (long long)VB * first, lds, VB * n);
    } else if (b < vb + fb) {
        const int first = (b - vb) * kItemsPerBlock, n = min(kItemsPerBlock, nT - first);
        const int i0 = first + 4 * threadIdx.x;
        unsigned w[14] = {};
        for_each_record([&](auto q) {
            const int i = i0 + decltype(q)::value;
            const bool in = i < nT;
            ply_face<decltype(q)::value>(w, in ? tri[3 * i] : 0, in ? tri[3 * i + 1] : 0, in ? tri[3 * i + 2] : 0);
        }, four);
#pragma unroll
        for (int q = 0; q < 13; q++) lds[13 * threadIdx.x + q] = w[q];
        __syncthreads();
        block_stream_store(out + hdr.len + (long long)VB * nV + 13ll * first, lds, 13 * n);
    } else {
        for (int i = threadIdx.x; i < hdr.len; i += blockDim.x) out[i] = (unsigned char)hdr.text[i];
    }
}

// SendFrame's stream (StreamLayout, wire.hip): blocks [0, xb): xyz, [xb, xb+cb): rgb, [.., +tb): triangles (1024 ints per block... 3072
// bytes), last block: the head
__global__ __launch_bounds__(256) void transfer_assemble_kernel(const uint4 *__restrict__ verts, int n_send, const int *__restrict__ tri,
                                                                 int n_tri, int n_chunks, const int *__restrict__ v_chunks,
                                                                 const int *__restrict__ t_chunks, int host_chunks,
                                                                 unsigned char *__restrict__ out, int xb, int cb, int tb)
{
    __shared__ unsigned lds[kItemsPerBlock * 3 + 1];
    const StreamLayout at(n_chunks, n_send, n_tri);
    const int b = blockIdx.x;
    if (b < xb) {                                             // verticesArray (:66-75, :97)
        const int first = b * kItemsPerBlock, n = min(kItemsPerBlock, n_send - first);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int l = threadIdx.x + 256 * q;
            if (l < n) {
                const uint4 v = verts[first + l];
                lds[3 * l] = v.y; lds[3 * l + 1] = v.z; lds[3 * l + 2] = v.w;
            }
        }
        __syncthreads();
        block_stream_store(out + at.xyz + 12ll * first, lds, 12 * n);
    } else if (b < xb + cb) {                                 // colorsArray (:69-71, :98)
        const int first = (b - xb) * kItemsPerBlock, n = min(kItemsPerBlock, n_send - first);
        const int i0 = first + 4 * threadIdx.x;
        unsigned c[4];
#pragma unroll
        for (int q = 0; q < 4; q++) c[q] = i0 + q < n_send ? (verts[i0 + q].x & 0xffffffu) : 0u;
        lds[3 * threadIdx.x + 0] = c[0] | (c[1] << 24);
        lds[3 * threadIdx.x + 1] = (c[1] >> 8) | (c[2] << 16);
        lds[3 * threadIdx.x + 2] = (c[2] >> 16) | (c[3] << 8);
        __syncthreads();
        block_stream_store(out + at.rgb + 3ll * first, lds, 3 * n);
    } else if (b < xb + cb + tb) {                            // trianglesBuffer (:80-81, :99)
        const long long first = (long long)(b - xb - cb) * (kItemsPerBlock * 3);
        const int n = (int)min((long long)kItemsPerBlock * 3, 3ll * n_tri - first);
        for (int l = threadIdx.x; l < n; l += 256) lds[l] = (unsigned)tri[first + l];
        __syncthreads();
        block_stream_store(out + at.tri + 4 * first, lds, 4 * n);
    } else {                                                  // WriteInt x 3 + the two chunk-size arrays (:92-96)
        int *o = reinterpret_cast<int *>(out);
        if (threadIdx.x == 0) { o[0] = n_send; o[1] = n_tri; o[2] = n_chunks; }
        for (int i = threadIdx.x; i < n_chunks; i += 256) {
            // host_chunks: formVerticesChunks (:177-201), sizes follow from n alone
            o[3 + i] = host_chunks ? min(kChunkLimit, n_send - i * kChunkLimit) : v_chunks[i];
            o[3 + n_chunks + i] = host_chunks ? 0 : t_chunks[i];
        }
    }
}

}  // namespace

static int ply_header(PlyHeader *h, int nV, int nT, bool normals)
{
    h->len = snprintf(h->text, sizeof h->text,
                      "ply\nformat binary_little_endian 1.0\r\n"          // StreamWriter.WriteLine on Windows (Utils.cs:234)
                      "element vertex %d\n"
                      "property float x\nproperty float y\nproperty float z\n%sproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
                      "element face %d\n"
                      "property list uchar int vertex_index\n"
                      "end_header\n", nV, normals ? "property float nx\nproperty float ny\nproperty float nz\n" : "", nT);
    return h->len > 0 && h->len < (int)sizeof h->text ? 0 : -1;
}

// lsnPlyBinaryBytes / lsnPlyNormalsBytes and lsnPlyPack / lsnPlyPackNormals: the same file with 15- or 27-byte vertex records.
// The file's size, and its header into *h; -1: bad counts.
static long long ply_bytes(int n_vertices, int n_triangles, bool normals, PlyHeader *h)
{
    if (n_vertices < 0 || n_triangles < 0 || ply_header(h, n_vertices, n_triangles, normals)) return -1;
    return h->len + (normals ? 27ll : 15ll) * n_vertices + 13ll * n_triangles;
}

static long long ply_pack(const char *who, int device, const void *d_vertices, const void *d_normals, bool normals, int n_vertices,
                          const int *d_triangles, int n_triangles, void *d_out, long long out_cap, void *stream)
{
    lsn::clear_error();
    PlyHeader h;
    const long long need = ply_bytes(n_vertices, n_triangles, normals, &h);
    if (need < 0) { lsn::set_error("%s: bad counts", who); return -1; }
    if ((n_vertices && (!d_vertices || (normals && !d_normals))) || (n_triangles && !d_triangles) || !d_out) { lsn::set_error("%s: null buffer", who); return -1; }
    if (need > out_cap) { lsn::set_error("%s: the file needs %lld bytes, the buffer holds %lld", who, need, out_cap); return -1; }
    if (use_device(who, device)) return -1;
    const int vb = div_up(n_vertices, kItemsPerBlock), fb = div_up(n_triangles, kItemsPerBlock);
    (normals ? ply_pack_kernel<true> : ply_pack_kernel<false>)<<<vb + fb + 1, 256, 0, lsn::as_stream(stream)>>>(
        static_cast<const uint4 *>(d_vertices), static_cast<const float *>(d_normals), n_vertices, d_triangles, n_triangles,
        static_cast<unsigned char *>(d_out), h, vb, fb);
    LSN_HIP(hipGetLastError());
    return need;
}

extern "C" {

long long lsnPlyBinaryBytes(int n_vertices, int n_triangles)
{
    return lsn::guarded("lsnPlyBinaryBytes", -1LL, [&]() -> long long { PlyHeader h; return ply_bytes(n_vertices, n_triangles, false, &h); });
}

long long lsnPlyPack(int device, const void *d_vertices, int n_vertices, const int *d_triangles, int n_triangles, void *d_out,
                     long long out_cap, void *stream)
{
    return lsn::guarded("lsnPlyPack", -1LL, [&]() -> long long {
        return ply_pack("lsnPlyPack", device, d_vertices, nullptr, false, n_vertices, d_triangles, n_triangles, d_out, out_cap, stream);
    });
}

long long lsnPlyNormalsBytes(int n_vertices, int n_triangles)
{
    return lsn::guarded("lsnPlyNormalsBytes", -1LL, [&]() -> long long { PlyHeader h; return ply_bytes(n_vertices, n_triangles, true, &h); });
}

long long lsnPlyPackNormals(int device, const void *d_vertices, const void *d_normals, int n_vertices, const int *d_triangles, int n_triangles,
                            void *d_out, long long out_cap, void *stream)
{
    return lsn::guarded("lsnPlyPackNormals", -1LL, [&]() -> long long {
        return ply_pack("lsnPlyPackNormals", device, d_vertices, d_normals, true, n_vertices, d_triangles, n_triangles, d_out, out_cap, stream);
    });
}

}  // extern "C"
