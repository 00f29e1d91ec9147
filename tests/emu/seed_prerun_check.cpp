// Stand-alone host check of the seed kernel's pre-run window (csrc/seed_kernels.h, device_scene.h SEGP_*) — TEST INFRASTRUCTURE ONLY.
//
// For random seeds and every column of a half (both generator classes) it replays what the kernel's lanes do — the ahead pass hands
// out entry states per class, a producer slot pre-runs SEGP_PRE blocks into kept words, writes them out and continues for SEGP_NBLK
// blocks, a consumer slot runs SEGP_NBLK blocks — and compares the 256 words with isaac_init_final.  It also checks that the slot map
// is a bijection between the 128 lanes of a half's two waves and the runs, and that the runs tile the 32 blocks of every column.
// Built by tests/test_seed_prerun.py with the host compiler and -fsanitize=address,undefined; exit status 0 = all good.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "isaac_core.h"

using namespace hr;

static const int COLS = 40;   // generators per half (seed_kernels.h SEED_LANES)

struct FinalMem {
    u64 m[256];
    void st8(int i, u64 A, u64 B, u64 C, u64 D, u64 E, u64 F, u64 G, u64 H) { m[i] = A; m[i + 1] = B; m[i + 2] = C; m[i + 3] = D; m[i + 4] = E; m[i + 5] = F; m[i + 6] = G; m[i + 7] = H; }
};
// the ring of one half and group: 128 slots of 16 words, written only where the column's class has a run
struct SlotSink {
    u64 (*slots)[16];
    bool *written;
    uint32_t col;
    bool wants(int block) const { return segp_wants(col, block); }
    void state(int block, u64 a, u64 b, u64 c, u64 d, u64 e, u64 f, u64 g, u64 h, u64 A, u64 B, u64 C, u64 D, u64 E, u64 F, u64 G, u64 H) {
        if (!segp_wants(col, block)) { std::printf("state handed out at block %d of column %u, which has no run there\n", block, col); std::exit(1); }
        const uint32_t s = segp_slot(col, block);
        if (s >= 128u || written[s]) { std::printf("slot %u of column %u block %d out of range or written twice\n", s, col, block); std::exit(1); }
        const u64 v[16] = {a, b, c, d, e, f, g, h, A, B, C, D, E, F, G, H};
        std::memcpy(slots[s], v, sizeof v);
        written[s] = true;
    }
};
// a run's destination: exactly `words` words from word `first` of the column; anything else is an error
struct RunMem {
    u64 *m;
    int *hits;
    int first, words;
    void st(int i, u64 v) {
        if (i < 0 || i >= words) { std::printf("run store at word %d outside its %d words\n", i, words); std::exit(1); }
        m[first + i] = v;
        hits[first + i]++;
    }
};

static u64 rng_state = 0x243F6A8885A308D3ULL;
static u64 next_word() {   // splitmix64
    u64 z = (rng_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 100;   // x 40 columns = seeds checked
    // ---- the slot map
    int cover[COLS][32];
    std::memset(cover, 0, sizeof cover);
    int producer_runs = 0, consumer_runs = 0;
    for (uint32_t s = 0; s < 128u; s++) {
        uint32_t col, first, nblk;
        segp_run(s, col, first, nblk);
        if (col >= (uint32_t)COLS || first + nblk > 32u) { std::printf("slot %u: column %u, blocks %u + %u\n", s, col, first, nblk); return 1; }
        if (!segp_wants(col, (int)first) || segp_slot(col, (int)first) != s) { std::printf("slot %u is not the slot of its own run (column %u block %u)\n", s, col, first); return 1; }
        if (nblk != (uint32_t)(s < 64u ? SEGP_PNBLK : SEGP_NBLK)) { std::printf("slot %u: %u blocks\n", s, nblk); return 1; }
        (s < 64u ? producer_runs : consumer_runs)++;
        for (uint32_t b = first; b < first + nblk; b++) cover[col][b]++;
    }
    for (int c = 0; c < COLS; c++)
        for (int b = 0; b < 32; b++)
            if (cover[c][b] != 1) { std::printf("block %d of column %d is covered %d times\n", b, c, cover[c][b]); return 1; }
    if (producer_runs != 64 || consumer_runs != 64) return 1;
    for (int c = 0; c < COLS; c++) {
        int wanted = 0;
        for (int b = 0; b < 32; b++) wanted += segp_wants((uint32_t)c, b) ? 1 : 0;
        if (wanted != (c < SEGP_XCOLS ? 3 : 4)) { std::printf("column %d wants %d states\n", c, wanted); return 1; }
    }
    // ---- the decomposition
    const IsaacWarm warm = isaac_warm();
    static u64 slots[128][16];
    bool written[128];
    long checked = 0;
    for (int round = 0; round < rounds; round++) {
        std::memset(written, 0, sizeof written);
        u64 want[COLS][256], got[COLS][256];
        int hits[COLS][256];
        std::memset(hits, 0, sizeof hits);
        for (int c = 0; c < COLS; c++) {
            // seeds as the kernel feeds them (small words) and, every other round, arbitrary 64-bit words
            const bool wide = (round & 1) != 0;
            const u64 s1 = wide ? next_word() : next_word() % 4096u, s2 = wide ? next_word() : next_word() % 1000000u, s3 = wide ? next_word() : next_word() % 1000000u;
            FinalMem fm;
            isaac_init_final(fm, warm, 8700304ULL, s1, s2, s3);
            std::memcpy(want[c], fm.m, sizeof fm.m);
            SlotSink sink{slots, written, (uint32_t)c};
            isaac_init_ahead_pre(sink, warm, 8700304ULL, s1, s2, s3);
            for (int i = 0; i < 256; i++) got[c][i] = 0xdeadbeefdeadbeefULL;
        }
        for (uint32_t s = 0; s < 128u; s++) {
            if (!written[s]) { std::printf("slot %u got no entry state\n", s); return 1; }
            uint32_t col, first, nblk;
            segp_run(s, col, first, nblk);
            u64 st16[16];
            std::memcpy(st16, slots[s], sizeof st16);
            if (s < 64u) {   // a producer lane: pre-run, then the window
                u64 kept[SEGP_PRE][8];
                isaac_init_prerun<SEGP_PRE>(st16, kept);
                RunMem dump{got[col], hits[col], (int)first * 8, SEGP_PRE * 8};
                for (int p = 0; p < SEGP_PRE; p++)
                    for (int j = 0; j < 8; j++) dump.st(p * 8 + j, kept[p][j]);
                RunMem m{got[col], hits[col], (int)(first + SEGP_PRE) * 8, SEGP_NBLK * 8};
                isaac_init_run<SEGP_NBLK>(m, st16);
            } else {
                RunMem m{got[col], hits[col], (int)first * 8, SEGP_NBLK * 8};
                isaac_init_run<SEGP_NBLK>(m, st16);
            }
        }
        for (int c = 0; c < COLS; c++) {
            for (int i = 0; i < 256; i++) {
                if (hits[c][i] != 1) { std::printf("round %d column %d word %d written %d times\n", round, c, i, hits[c][i]); return 1; }
                if (got[c][i] != want[c][i]) { std::printf("round %d column %d word %d: %016llx, isaac_init_final has %016llx\n", round, c, i, got[c][i], want[c][i]); return 1; }
            }
            checked++;
        }
    }
    std::printf("seed_prerun_check ok: %ld seeds, both classes, 256 words each\n", checked);
    return 0;
}
