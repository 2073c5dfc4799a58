// wire_inbound.hip -- part of wire.hip's translation unit: the inbound formats, host code only, no kernels.  The client's frame message
// (liveScanClient.cpp:185-290 as KinectSocket.cs:211-304 reads it), zstd through dlopen (ZSTDDecompressor.cs:13-31), and the client's
// recording file (frameFileWriterReader.cpp:59-82,115-130).

namespace {
struct Zstd {
    void *handle = nullptr;
    size_t (*decompress)(void *, size_t, const void *, size_t) = nullptr;
    unsigned long long (*decompressed_size)(const void *, size_t) = nullptr;
    unsigned (*is_error)(size_t) = nullptr;
    size_t (*compress)(void *, size_t, const void *, size_t, int) = nullptr;
    size_t (*bound)(size_t) = nullptr;
    bool ok = false;
};

Zstd &zstd()
{
    static Zstd z;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char *name : {"libzstd.so.1", "libzstd.so"}) {
            z.handle = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (z.handle) break;
        }
        if (!z.handle) return;
        z.decompress = reinterpret_cast<decltype(z.decompress)>(dlsym(z.handle, "ZSTD_decompress"));
        z.decompressed_size = reinterpret_cast<decltype(z.decompressed_size)>(dlsym(z.handle, "ZSTD_getDecompressedSize"));
        z.is_error = reinterpret_cast<decltype(z.is_error)>(dlsym(z.handle, "ZSTD_isError"));
        z.compress = reinterpret_cast<decltype(z.compress)>(dlsym(z.handle, "ZSTD_compress"));
        z.bound = reinterpret_cast<decltype(z.bound)>(dlsym(z.handle, "ZSTD_compressBound"));
        z.ok = z.decompress && z.decompressed_size && z.is_error && z.compress && z.bound;
    });
    return z;
}

int rd_i32(const unsigned char *p) { int v; memcpy(&v, p, 4); return v; }

// walks the body block (liveScanClient.cpp:233-268 / KinectSocket.cs:262-303); returns its length or -1
long long body_block_length(const unsigned char *b, long long avail, int *n_bodies)
{
    if (avail < 4) return -1;
    const int nb = rd_i32(b);
    if (nb < 0) return -1;
    long long pos = 4;
    for (int i = 0; i < nb; i++) {
        if (pos + 5 > avail) return -1;
        const int nj = rd_i32(b + pos + 1);
        if (nj < 0) return -1;
        pos += 5 + 28ll * nj;
        if (pos > avail) return -1;
    }
    *n_bodies = nb;
    return pos;
}

// the uncompressed payload: depth, colour, body block (liveScanClient.cpp:207-268)
void raw_body(unsigned char *dst, const unsigned char *depth, const unsigned char *rgb, long long P, const unsigned char *bodies, int bodies_bytes)
{
    memcpy(dst, depth, (size_t)(2 * P));
    memcpy(dst + 2 * P, rgb, (size_t)(3 * P));
    memcpy(dst + 5 * P, bodies, (size_t)bodies_bytes);
}

bool is_space(unsigned char c) { return c == ' ' || c == '\n' || c == '\r' || c == '\t' || c == '\v' || c == '\f'; }

// one "%s" of the reader's fscanf (frameFileWriterReader.cpp:66)
bool next_token(const unsigned char *f, long long len, long long *pos, long long *b, long long *e)
{
    long long p = *pos;
    while (p < len && is_space(f[p])) p++;
    if (p >= len) return false;
    *b = p;
    while (p < len && !is_space(f[p])) p++;
    *e = p;
    *pos = p;
    return true;
}

bool next_int(const unsigned char *f, long long len, long long *pos, int *out)
{
    long long b, e;
    if (!next_token(f, len, pos, &b, &e) || e - b > 11) return false;
    char tmp[16];
    memcpy(tmp, f + b, (size_t)(e - b));
    tmp[e - b] = 0;
    char *endp;
    const long v = strtol(tmp, &endp, 10);
    if (endp == tmp || *endp != 0) return false;
    *out = (int)v;
    return true;
}
}  // namespace

extern "C" {

int lsnZstdAvailable(void) { return zstd().ok ? 1 : 0; }

int lsnFrameParseHeader(const unsigned char *header16, LsnFrameInfo *info)
{
    return lsn::guarded("lsnFrameParseHeader", -1, [&]() {
        lsn::clear_error();
        if (!header16 || !info) { lsn::set_error("lsnFrameParseHeader: null argument"); return -1; }
        info->payload_bytes = rd_i32(header16);                     // KinectSocket.cs:229
        info->compressed = rd_i32(header16 + 4);                    // :237
        info->width = rd_i32(header16 + 8);                         // :238
        info->height = rd_i32(header16 + 12);                       // :239
        if (info->payload_bytes <= 0) return 1;                     // :231-235: "no more stored frames"
        if (info->width < 0 || info->height < 0 || (long long)info->width * info->height > (1ll << 26)) {
            lsn::set_error("lsnFrameParseHeader: implausible frame size %d x %d", info->width, info->height);
            return -1;
        }
        return 0;
    });
}

long long lsnFrameDecode(const unsigned char *payload, int payload_bytes, int compressed, int width, int height,
                         unsigned char *depth_out, unsigned char *rgb_out, unsigned char *bodies_out, int bodies_cap,
                         int *n_bodies)
{
    return lsn::guarded("lsnFrameDecode", -1LL, [&]() -> long long {
        lsn::clear_error();
        if (!payload || payload_bytes <= 0 || width < 0 || height < 0) { lsn::set_error("lsnFrameDecode: bad arguments"); return -1; }
        const long long P = (long long)width * height;
        const unsigned char *raw = payload;
        long long raw_len = payload_bytes;
        std::vector<unsigned char> tmp;
        if (compressed == 1) {                                      // KinectSocket.cs:247-248
            Zstd &z = zstd();
            if (!z.ok) { lsn::set_error("lsnFrameDecode: compressed frame but libzstd.so.1 could not be loaded"); return -1; }
            const unsigned long long out = z.decompressed_size(payload, (size_t)payload_bytes);     // ZSTDDecompressor.cs:28
            // a frame is w*h*5 bytes plus a few KB of body joints: anything else is a corrupted length field, not worth allocating
            if (out < (unsigned long long)(5 * P + 4) || out > (unsigned long long)(5 * P) + (1ull << 20)) {
                lsn::set_error("lsnFrameDecode: the zstd frame announces %llu bytes, a %d x %d frame has %lld + bodies", out, width, height, 5 * P);
                return -1;
            }
            tmp.resize((size_t)out);
            const size_t got = z.decompress(tmp.data(), tmp.size(), payload, (size_t)payload_bytes);
            if (z.is_error(got) || got != out) { lsn::set_error("lsnFrameDecode: zstd decompression failed"); return -1; }
            raw = tmp.data();
            raw_len = (long long)out;
        }
        if (raw_len < 5 * P + 4) { lsn::set_error("lsnFrameDecode: payload of %lld bytes is shorter than %d x %d x 5 + 4", raw_len, width, height); return -1; }
        int nb = 0;
        const long long bl = body_block_length(raw + 5 * P, raw_len - 5 * P, &nb);
        if (bl < 0) { lsn::set_error("lsnFrameDecode: inconsistent body block"); return -1; }
        if (depth_out) memcpy(depth_out, raw, (size_t)(2 * P));                              // KinectSocket.cs:256
        if (rgb_out) memcpy(rgb_out, raw + 2 * P, (size_t)(3 * P));                          // :257
        if (bodies_out) {
            if (bl > bodies_cap) { lsn::set_error("lsnFrameDecode: body block of %lld bytes exceeds the buffer (%d)", bl, bodies_cap); return -1; }
            memcpy(bodies_out, raw + 5 * P, (size_t)bl);
        }
        if (n_bodies) *n_bodies = nb;
        return bl;
    });
}

long long lsnFrameEncode(const unsigned char *depth, const unsigned char *rgb, int width, int height, const unsigned char *bodies,
                         int bodies_bytes, int compression_level, unsigned char *out, long long out_cap)
{
    return lsn::guarded("lsnFrameEncode", -1LL, [&]() -> long long {
        lsn::clear_error();
        if (!depth || !rgb || !out || width < 0 || height < 0) { lsn::set_error("lsnFrameEncode: bad arguments"); return -1; }
        static const unsigned char no_bodies[4] = {0, 0, 0, 0};
        if (!bodies || bodies_bytes < 4) { bodies = no_bodies; bodies_bytes = 4; }
        const long long P = (long long)width * height, size = 5 * P + bodies_bytes;
        if (size > 0x7fffffffll) { lsn::set_error("lsnFrameEncode: frame too large"); return -1; }
        int isize = (int)size, comp = compression_level > 0 ? 1 : 0;
        if (!comp) {
            if (16 + size > out_cap) { lsn::set_error("lsnFrameEncode: needs %lld bytes", 16 + size); return -1; }
            raw_body(out + 16, depth, rgb, P, bodies, bodies_bytes);
        } else {                                                    // liveScanClient.cpp:270-281
            Zstd &z = zstd();
            if (!z.ok) { lsn::set_error("lsnFrameEncode: compression requested but libzstd.so.1 could not be loaded"); return -1; }
            std::vector<unsigned char> raw((size_t)size);
            raw_body(raw.data(), depth, rgb, P, bodies, bodies_bytes);
            std::vector<unsigned char> packed(z.bound((size_t)size));
            const size_t c = z.compress(packed.data(), packed.size(), raw.data(), raw.size(), compression_level);
            if (z.is_error(c)) { lsn::set_error("lsnFrameEncode: zstd compression failed"); return -1; }
            if (16 + (long long)c > out_cap) { lsn::set_error("lsnFrameEncode: needs %lld bytes", 16 + (long long)c); return -1; }
            memcpy(out + 16, packed.data(), c);
            isize = (int)c;
        }
        const int head[4] = {isize, comp, width, height};           // liveScanClient.cpp:284-288
        memcpy(out, head, 16);
        return 16 + (long long)isize;
    });
}

long long lsnRecordingAppend(unsigned char *out, long long cap, const unsigned char *frame, int len, int timestamp_ms)
{
    return lsn::guarded("lsnRecordingAppend", -1LL, [&]() -> long long {
        lsn::clear_error();
        char hdr[96];
        const int hl = snprintf(hdr, sizeof hdr, "bufferSize= %d\nframe_timestamp= %d\n", len, timestamp_ms);   // frameFileWriterReader.cpp:123
        const long long need = hl + (long long)len + 1;
        if (!out || len < 0 || need > cap) { lsn::set_error("lsnRecordingAppend: needs %lld bytes", need); return -1; }
        memcpy(out, hdr, (size_t)hl);
        if (len > 0) memcpy(out + hl, frame, (size_t)len);
        out[hl + len] = '\n';                                       // :127
        return need;
    });
}

long long lsnRecordingNext(const unsigned char *file, long long len, long long pos, long long *frame_off, int *frame_len,
                           int *timestamp_ms)
{
    return lsn::guarded("lsnRecordingNext", -1LL, [&]() -> long long {
        lsn::clear_error();
        if (!file || pos < 0 || !frame_off || !frame_len || !timestamp_ms) { lsn::set_error("lsnRecordingNext: bad arguments"); return -1; }
        long long b, e;
        int size = 0, ts = 0;
        if (!next_token(file, len, &pos, &b, &e)) return -1;        // end of file: not an error
        if (!next_int(file, len, &pos, &size) || !next_token(file, len, &pos, &b, &e) || !next_int(file, len, &pos, &ts) || size < 0) {
            lsn::set_error("lsnRecordingNext: malformed record header at byte %lld", b);
            return -1;
        }
        *frame_len = size;
        *timestamp_ms = ts;
        if (size == 0) { *frame_off = pos; return pos; }            // :72-73
        pos += 1;                                                   // fgetc '\n' (:75)
        if (pos + size > len) { lsn::set_error("lsnRecordingNext: record of %d bytes runs past the end of the file", size); return -1; }
        *frame_off = pos;
        pos += size;
        if (pos < len) pos += 1;                                    // fgetc '\n' (:78)
        return pos;
    });
}

}  // extern "C"
