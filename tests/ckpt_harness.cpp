// host/checkpoint.h on its own, for tests/test_checkpoint_cpu.py (built with g++ and the sanitizers; no device, no hanamaru library).
//   ckpt_harness read FILE...     one line of JSON per file: what ckpt::read found, each payload as its length and the FNV-1a (64 bit) of its bytes,
//                                 and the process's peak resident memory so far
//   ckpt_harness write FILE width height samplings hash x0 y0 w h moments_n counts K buckets_n
//                                 w x h: the accumulator's shape; x0 y0 w h other than 0 0 width height: a region file; moments_n < 0, counts == 0,
//                                 K == 0: without that trailer.  Element i of a payload is (i + 1) x {0.5, 0.25, 3, 0.125} (acc, moments, counts, buckets).
#include <cinttypes>
#include <cstdlib>
#include <cstring>

#include "checkpoint.h"

template <class T> static void payload(const char *name, const std::vector<T> &v) {
    uint64_t h = 14695981039346656037ull;
    const unsigned char *p = (const unsigned char *)v.data();
    for (size_t i = 0; i < v.size() * sizeof(T); i++) h = (h ^ p[i]) * 1099511628211ull;
    printf(", \"%s\": [%zu, \"%016" PRIx64 "\"]", name, v.size(), h);
}

// VmHWM of /proc/self/status: this program's own peak (getrusage's figure starts from the process that started it); -1 where there is none
static long peak_kb() {
    long kb = -1;
    char line[256];
    FILE *f = fopen("/proc/self/status", "r");
    while (f && fgets(line, sizeof line, f))
        if (sscanf(line, "VmHWM: %ld", &kb) == 1) break;
    if (f) fclose(f);
    return kb;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "read")) {
        for (int i = 2; i < argc; i++) {
            const ckpt::File c = ckpt::read(argv[i]);
            printf("{\"magic\": %u, \"width\": %u, \"height\": %u, \"samplings\": %u, \"scene_hash\": %u, \"region\": [%u, %u, %u, %u]", c.magic, c.width, c.height, c.samplings,
                   c.scene_hash, c.region[0], c.region[1], c.region[2], c.region[3]);
            printf(", \"has_moments\": %d, \"moments_n\": %" PRIu64 ", \"has_counts\": %d, \"has_buckets\": %d, \"buckets_head\": %d, \"buckets_k\": %u, \"buckets_n\": %" PRIu64,
                   c.has_moments, c.moments_n, c.has_counts, c.has_buckets, c.buckets_head, c.buckets_k, c.buckets_n);
            printf(", \"complete\": %d, \"cut\": %d", (int)c.complete, (int)c.cut);
            payload("acc", c.acc), payload("moments", c.moments), payload("counts", c.counts), payload("buckets", c.buckets);
            printf(", \"peak_kb\": %ld}\n", peak_kb());
        }
        return 0;
    }
    if (argc == 15 && !strcmp(argv[1], "write")) {
        uint64_t a[12];
        for (int i = 0; i < 12; i++) a[i] = (uint64_t)strtoll(argv[3 + i], nullptr, 10);
        ckpt::File c;
        c.width = (uint32_t)a[0], c.height = (uint32_t)a[1], c.samplings = (uint32_t)a[2], c.scene_hash = (uint32_t)a[3];
        for (int k = 0; k < 4; k++) c.region[k] = (uint32_t)a[4 + k];
        c.magic = c.region[2] != c.width || c.region[3] != c.height ? ckpt::REGION : ckpt::FRAME;
        const size_t pixels = (size_t)c.region[2] * c.region[3];
        c.has_moments = (int64_t)a[8] >= 0, c.has_counts = a[9] != 0, c.has_buckets = a[10] != 0;
        c.acc.resize(pixels * 3);
        for (size_t i = 0; i < c.acc.size(); i++) c.acc[i] = (float)(i + 1) * 0.5f;
        if (c.has_moments) {
            c.moments_n = a[8];
            c.moments.resize(pixels * 6);
            for (size_t i = 0; i < c.moments.size(); i++) c.moments[i] = (double)(i + 1) * 0.25;
        }
        if (c.has_counts) {
            c.counts.resize(pixels);
            for (size_t i = 0; i < c.counts.size(); i++) c.counts[i] = (uint32_t)(i + 1) * 3u;
        }
        if (c.has_buckets) {
            c.buckets_k = (uint32_t)a[10], c.buckets_n = a[11];
            c.buckets.resize(pixels * 3 * c.buckets_k);
            for (size_t i = 0; i < c.buckets.size(); i++) c.buckets[i] = (double)(i + 1) * 0.125;
        }
        return ckpt::write(argv[2], c) ? 0 : 1;
    }
    fprintf(stderr, "usage: ckpt_harness read FILE... | write FILE width height samplings hash x0 y0 w h moments_n counts K buckets_n\n");
    return 2;
}
