// csrc/jpeg_sync_core.h as a program of its own: what tests/jpeg_sync_cases.host_program compiles with -fsanitize=address,undefined
// and tests/test_jpeg_sync_host_cpu.py runs as a separate process.  It does for every call what sf_jpeg_decode_split's entropy
// stage does on the device, phase by phase and segment by segment, with the core's own functions: the descriptor check and the
// route of jpeg_plan_kernel, the unstuffing (count per chunk, prefix, copy), the speculative walk of every segment, the rounds of
// jpeg_sync_kernel window by window (Jacobi: a round reads the exits of the round before), the block ordinals, the strict walk of
// every segment, the DC prefix sums and checks, the smallest error key; intervals below split_min_bytes take decode_interval with
// the serial policy of jpeg_decode_host_main.cpp.  Every buffer is a heap block of exactly its size -- the unstuffed stream of
// exactly u_len bytes -- so a read or write outside one is a sanitizer report and a loop that does not end is a hung test.
//
//   jpeg_sync_host <cases> <results>
//   cases:   int32 n_calls; per call int32 h, w, components, hs, vs, n_images, n_intervals, n_sets; int64 data_bytes; int32
//            segment_bytes; int64 split_min_bytes; the data; the descriptors (n_intervals x 6 int64); the tables (n_sets x 1824 bytes)
//   results: per call int32 status[n_images], int32 interval_status[n_intervals], int32 rounds[n_intervals] (the rounds of all
//            windows in which an entry changed; -1: the wave route), int32 redecodes[n_intervals], int32 segments[n_intervals], int16
//            coefficients[n_images x blocks x 64] in the device's layout, prefilled with zeros
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../jpeg_sync_core.h"

namespace {

using namespace sf_jpegdec;

struct SerialPolicy {
    const uint8_t* in;
    int16_t* coef_out;
    const Geom* g;
    int64_t image;
    int block[64];

    uint32_t bytes(int64_t pos, int k) {
        uint32_t v = 0;
        for (int i = 0; i < k; ++i) v = v << 8 | in[pos + i];
        return v;
    }
    uint32_t uni(uint32_t v) { return v; }
    int lane() { return 0; }
    int lanes() { return 1; }
    void sync() {}
    void coef(int k, int v) { block[k] = v; }
    void store(int c, int64_t mi, int j) {
        int16_t* dst = coef_out + block_index(*g, image, c, mi, j) * 64;
        for (int k = 0; k < 64; ++k) dst[k] = (int16_t)block[k], block[k] = 0;
    }
};

struct HostSink {
    int16_t* coef;
    const Geom* g;
    int64_t image, first_mcu;
    uint64_t* key;
    int16_t* cur;
    void begin(int64_t mcu, int slot) { cur = coef + block_index(*g, image, slot_comp(*g, slot), first_mcu + mcu, slot_block(*g, slot)) * 64; }
    void put(int nat, int v) { cur[nat] = (int16_t)v; }
    void error(int64_t ordinal, int phase, int status) {
        const uint64_t k = error_key(ordinal, phase, status);
        if (k < *key) *key = k;
    }
};

struct State {
    int64_t bit;
    int slot, k;
    bool operator!=(const State& o) const { return bit != o.bit || slot != o.slot || k != o.k; }
};

bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

// One interval on the split route -> its status; rounds / redecodes / segments for the report.
int split_interval(SerialPolicy& p, const Tables& t, const Geom& g, const uint8_t* in, const int64_t* d, int16_t* coef, const uint8_t* set,
                   int S, int32_t& rounds, int32_t& redecodes, int32_t& segments) {
    const int64_t in_len = d[1];
    // 1. unstuff: count per chunk up to the first marker, prefix, copy
    const int64_t nchunk = (in_len + S - 1) / S;
    std::vector<int64_t> start((size_t)nchunk + 1, 0);
    int end_err = 0;
    int64_t used = nchunk;
    for (int64_t c = 0; c < nchunk; ++c) {
        bool marker;
        const int64_t hi = (c + 1) * S < in_len ? (c + 1) * S : in_len;
        start[(size_t)c + 1] = start[(size_t)c] + unstuff_count(in, in_len, c * S, hi, marker);
        if (marker) {
            end_err = kBadMarker, used = c + 1;
            break;
        }
    }
    const int64_t ulen = start[(size_t)used];
    uint8_t* u = (uint8_t*)malloc(ulen ? (size_t)ulen : 1);
    if (!u) exit(2);
    for (int64_t c = 0; c < used; ++c) {
        const int64_t hi = (c + 1) * S < in_len ? (c + 1) * S : in_len;
        if (start[(size_t)c + 1] > start[(size_t)c]) unstuff_copy(in, in_len, c * S, hi, u + start[(size_t)c]);
    }
    // 2. the speculative walks
    const int64_t nseg = ulen ? (ulen + S - 1) / S : 1;
    segments = (int32_t)nseg;
    std::vector<State> entry((size_t)nseg), exits((size_t)nseg);
    std::vector<int> nblk((size_t)nseg);
    std::vector<int64_t> first_blk((size_t)nseg);
    auto end_bit = [&](int64_t s) { return 8 * ((s + 1) * S < ulen ? (s + 1) * S : ulen); };
    for (int64_t s = 0; s < nseg; ++s) {
        entry[(size_t)s] = State{8 * s * S, 0, 0};
        const SegExit e = lenient_segment(p, t, g, u, ulen, end_err, 8 * s * S, 0, 0, end_bit(s));
        exits[(size_t)s] = State{e.bit, e.slot, e.k}, nblk[(size_t)s] = e.blocks;
    }
    // 3. the rounds, window by window
    State carry{0, 0, 0};
    int64_t ord = 0;
    rounds = 0, redecodes = 0;
    for (int64_t w0 = 0; w0 < nseg; w0 += kSyncWindow) {
        const int64_t w1 = w0 + kSyncWindow < nseg ? w0 + kSyncWindow : nseg;
        for (int round = 0; round <= kSyncWindow; ++round) {
            std::vector<State> before(exits.begin() + w0, exits.begin() + w1);
            bool any = false;
            for (int64_t s = w0; s < w1; ++s) {
                const State n = s == w0 ? carry : before[(size_t)(s - w0 - 1)];
                if (!(n != entry[(size_t)s])) continue;
                any = true, ++redecodes;
                entry[(size_t)s] = n;
                const SegExit e = lenient_segment(p, t, g, u, ulen, end_err, n.bit, n.slot, n.k, end_bit(s));
                exits[(size_t)s] = State{e.bit, e.slot, e.k}, nblk[(size_t)s] = e.blocks;
            }
            if (!any) break;
            ++rounds;
        }
        for (int64_t s = w0; s < w1; ++s) first_blk[(size_t)s] = ord, ord += nblk[(size_t)s];
        carry = exits[(size_t)w1 - 1];
    }
    // 4. the strict walks
    uint64_t key = kNoError;
    const int bpm = blocks_per_mcu(g);
    HostSink sink{coef, &g, d[2], d[3], &key, nullptr};
    for (int64_t s = 0; s < nseg; ++s) {
        const State e = s == 0 ? State{0, 0, 0} : exits[(size_t)s - 1];
        strict_segment(p, sink, t, g, u, ulen, end_err, e.bit, e.slot, e.k, end_bit(s), first_blk[(size_t)s], d[4] * bpm, s == nseg - 1);
    }
    free(u);
    // 5. the DC predictions and the block sums, per component in scan order
    for (int c = 0; c < g.nc; ++c) {
        const int cb = comp_blocks(g, c), slot0 = c == 0 ? 0 : g.hs * g.vs + c - 1;
        const int q0 = set[c * kCompBytes];
        int64_t pred = 0;
        for (int64_t n = 0; n < d[4] * cb; ++n) {
            const int64_t mcu = n / cb;
            const int j = (int)(n - mcu * cb);
            int16_t* blk = coef + block_index(g, d[2], c, d[3] + mcu, j) * 64;
            pred += blk[0];
            int v;
            const int st = dc_value(pred, q0, v);
            if (st != kOk) sink.error(mcu * bpm + slot0 + j, 0, st);
            blk[0] = (int16_t)v;
            int sum = 0;
            for (int k = 0; k < 64; ++k) sum += blk[k] < 0 ? -blk[k] : blk[k];
            if (sum > kBlockSumMax) sink.error(mcu * bpm + slot0 + j, 2, kCoefRange);
        }
    }
    return key == kNoError ? kOk : key_status(key);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s <cases> <results>\n", argv[0]);
        return 2;
    }
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) {
        fprintf(stderr, "cannot open %s / %s\n", argv[1], argv[2]);
        return 2;
    }
    int32_t n_calls = 0;
    if (!get(fi, &n_calls, 4) || n_calls < 0) return 2;
    for (int32_t call = 0; call < n_calls; ++call) {
        int32_t hd[8], S = 0;
        int64_t data_bytes = 0, split_min = 0;
        if (!get(fi, hd, sizeof hd) || !get(fi, &data_bytes, 8) || data_bytes < 0 || !get(fi, &S, 4) || !get(fi, &split_min, 8)) return 2;
        const int h = hd[0], w = hd[1], nc = hd[2], hs = hd[3], vs = hd[4], n_images = hd[5], n_intervals = hd[6], n_sets = hd[7];
        if (h < 1 || w < 1 || h > 8192 || w > 8192 || (nc != 1 && nc != 3) || hs < 1 || hs > 2 || vs < 1 || vs > 2 || n_images < 1 ||
            n_intervals < 1 || n_sets < 1 || S < kSegmentBytesMin || S > kSegmentBytesMax || (S & (S - 1)) || split_min < 0)
            return 2;
        const Geom g = make_geom(h, w, nc, hs, vs);
        const int64_t mcus = mcu_count(g), ncoef = (int64_t)n_images * g.image_blocks * 64;
        // exact sizes, from malloc: the sanitizer's red zones start at the first byte outside
        uint8_t* data = (uint8_t*)malloc((size_t)data_bytes ? (size_t)data_bytes : 1);
        int64_t* desc = (int64_t*)malloc((size_t)n_intervals * kDescWords * 8);
        uint8_t* tabs = (uint8_t*)malloc((size_t)n_sets * kSetBytes);
        int16_t* coef = (int16_t*)malloc((size_t)ncoef * 2);
        if (!data || !desc || !tabs || !coef) return 2;
        if (!get(fi, data, (size_t)data_bytes) || !get(fi, desc, (size_t)n_intervals * kDescWords * 8) ||
            !get(fi, tabs, (size_t)n_sets * kSetBytes))
            return 2;
        memset(coef, 0, (size_t)ncoef * 2);                                 // the split route's memset
        std::vector<int32_t> ist(n_intervals), status(n_images), rounds(n_intervals, -1), redecodes(n_intervals, 0), segments(n_intervals, 0);
        std::vector<int64_t> first_error(n_images, -1);
        std::vector<uint32_t> covered(n_images, 0);                         // 32 bits, as on the device
        for (int i = 0; i < n_intervals; ++i) {
            const int64_t* d = desc + (int64_t)i * kDescWords;
            int st;
            if (!desc_ok(d, data_bytes, n_images, mcus, n_sets)) {
                st = kBadDesc;
            } else {
                SerialPolicy p{data + d[0], coef, &g, d[2], {0}};
                Tables t;
                memset(&t, 0xEE, sizeof t);                                 // LDS starts with garbage too: nothing may depend on it
                st = build_tables(p, t, tabs + d[5] * kSetBytes, nc);
                if (st == kOk && d[1] >= split_min)
                    st = split_interval(p, t, g, data + d[0], d, coef, tabs + d[5] * kSetBytes, S, rounds[i], redecodes[i], segments[i]);
                else if (st == kOk)
                    st = decode_interval(p, t, g, d[1], d[3], d[4]);
            }
            ist[i] = st;
            const int64_t image = desc_image(d, n_images);
            if (st != kOk) {
                if (first_error[image] < 0) first_error[image] = (int64_t)i << 5 | st;
            } else {
                covered[image] += (uint32_t)d[4];
            }
        }
        for (int i = 0; i < n_images; ++i) status[i] = image_status(first_error[i], covered[i], mcus);
        fwrite(status.data(), 4, (size_t)n_images, fo);
        fwrite(ist.data(), 4, (size_t)n_intervals, fo);
        fwrite(rounds.data(), 4, (size_t)n_intervals, fo);
        fwrite(redecodes.data(), 4, (size_t)n_intervals, fo);
        fwrite(segments.data(), 4, (size_t)n_intervals, fo);
        fwrite(coef, 2, (size_t)ncoef, fo);
        free(data), free(desc), free(tabs), free(coef);
    }
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 2;
}
