// The checkpoint file of hanamaru-hip (--checkpoint / --resume): the format, one writer and one reader.  Standard library only.
// Little-endian, no padding, in this order:
//   header        {magic "HRA2" | "HRR2", width, height, samplings done, FNV-1a of the scene name}, 5 x u32; a region render's file
//                 ("HRR2") goes on with the window {x0, y0, w, h}, 4 x u32, and w x h below is the window's (else the frame's)
//   accumulator   w*h*3 f32
// then, each of them optional:
//   {"HRMS", u64 n, w*h*6 f64}          the sample moments of a render with moments on and the samplings behind them
//   {"HRSC", w*h u32}                   the per-pixel sampling counts of a render with sample counts on
//   {"HRBK", u32 K, u64 n, w*h*3K f64}  the K sample buckets of a render with --robust K and the samplings behind them
// What a render demands of a file (which trailers, which K, which window) and what it says when the file falls short is the caller's.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

namespace ckpt {

constexpr uint32_t FRAME = 0x32415248u, REGION = 0x32525248u, MOMENTS = 0x534d5248u, COUNTS = 0x43535248u, BUCKETS = 0x4b425248u;
enum Section { S_NONE, S_HEADER, S_ACCUMULATOR, S_MOMENTS, S_COUNTS, S_BUCKETS };

struct File {
    uint32_t magic = 0, width = 0, height = 0, samplings = 0, scene_hash = 0;
    uint32_t region[4] = {0, 0, 0, 0};   // "HRR2": the window; "HRA2": {0, 0, width, height}, not in the file
    std::vector<float> acc;
    bool has_moments = false, has_counts = false, has_buckets = false;
    uint64_t moments_n = 0;
    std::vector<double> moments;
    std::vector<uint32_t> counts;
    uint32_t buckets_k = 0;
    uint64_t buckets_n = 0;
    std::vector<double> buckets;
    // what read() found:
    Section complete = S_NONE;   // the last section that is whole
    Section cut = S_NONE;        // the section behind it that begins but is cut short (S_HEADER: also no file, or another magic); S_NONE: none
    bool buckets_head = false;   // "HRBK"'s K and n were read (the doubles behind them may still be cut short)
};

inline bool write(const char *path, const File &c) {
    FILE *f = fopen(path, "wb");
    if (!f) return false;
    auto put = [f](const void *p, size_t bytes) { return fwrite(p, 1, bytes, f) == bytes; };
    const uint32_t hdr[9] = {c.magic, c.width, c.height, c.samplings, c.scene_hash, c.region[0], c.region[1], c.region[2], c.region[3]};
    bool ok = put(hdr, c.magic == REGION ? 36 : 20) && put(c.acc.data(), c.acc.size() * sizeof(float));
    if (ok && c.has_moments) ok = put(&MOMENTS, 4) && put(&c.moments_n, 8) && put(c.moments.data(), c.moments.size() * sizeof(double));
    if (ok && c.has_counts) ok = put(&COUNTS, 4) && put(c.counts.data(), c.counts.size() * sizeof(uint32_t));
    if (ok && c.has_buckets) ok = put(&BUCKETS, 4) && put(&c.buckets_k, 4) && put(&c.buckets_n, 8) && put(c.buckets.data(), c.buckets.size() * sizeof(double));
    fclose(f);
    return ok;
}

// The bytes of a file that are left to read: nothing is read, and nothing allocated, beyond the file's own length.
struct Input {
    FILE *f;
    uint64_t left;
    bool get(void *p, uint64_t bytes) {
        if (bytes > left || fread(p, 1, bytes, f) != bytes) return false;
        left -= bytes;
        return true;
    }
    template <class T> bool get(std::vector<T> &v, uint64_t pixels, uint64_t per_pixel) {   // (no product is formed before it is known to fit)
        if (pixels && per_pixel > left / sizeof(T) / pixels) return false;
        v.resize(pixels * per_pixel);
        return get(v.data(), v.size() * sizeof(T));
    }
};

// Reads the sections of the file in order, each sized by the file's own header, and stops at the first that is absent or cut short.
inline void read_sections(Input &in, File &c) {
    uint32_t hdr[5];
    c.cut = S_HEADER;
    if (!in.get(hdr, 20)) return;
    c.magic = hdr[0], c.width = hdr[1], c.height = hdr[2], c.samplings = hdr[3], c.scene_hash = hdr[4];
    c.region[2] = c.width, c.region[3] = c.height;
    if ((c.magic != FRAME && c.magic != REGION) || (c.magic == REGION && !in.get(c.region, 16))) return;
    c.complete = S_HEADER, c.cut = S_ACCUMULATOR;
    const uint64_t pixels = (uint64_t)c.region[2] * c.region[3];
    if (!in.get(c.acc, pixels, 3)) return;
    c.complete = S_ACCUMULATOR, c.cut = S_NONE;
    uint32_t magic = 0;
    auto next = [&]() { if (!in.get(&magic, 4)) magic = 0; };   // the magic of the trailer that follows, 0 at the end of the file
    next();
    if (magic == MOMENTS) {
        c.cut = S_MOMENTS;
        if (!in.get(&c.moments_n, 8) || !in.get(c.moments, pixels, 6)) return;
        c.has_moments = true, c.complete = S_MOMENTS, c.cut = S_NONE;
        next();
    }
    if (magic == COUNTS) {
        c.cut = S_COUNTS;
        if (!in.get(c.counts, pixels, 1)) return;
        c.has_counts = true, c.complete = S_COUNTS, c.cut = S_NONE;
        next();
    }
    if (magic == BUCKETS) {
        c.cut = S_BUCKETS;
        c.buckets_head = in.get(&c.buckets_k, 4) && in.get(&c.buckets_n, 8);
        if (!c.buckets_head || !in.get(c.buckets, pixels, 3 * (uint64_t)c.buckets_k)) return;
        c.has_buckets = true, c.complete = S_BUCKETS, c.cut = S_NONE;
    }
}

inline File read(const char *path) {
    File c;
    c.cut = S_HEADER;
    FILE *f = fopen(path, "rb");
    if (!f) return c;
    if (fseek(f, 0, SEEK_END) == 0) {
        const long size = ftell(f);
        Input in = {f, size > 0 ? (uint64_t)size : 0};
        if (fseek(f, 0, SEEK_SET) == 0) read_sections(in, c);
    }
    fclose(f);
    return c;
}

}  // namespace ckpt
