// The per-point rules of sft_track_advance (csrc/track_core.h) as a stand-alone host program, for runs under the sanitizers:
//     track_host CASES ROWS
// CASES: int32 count, then per case eight int32 (K, h, w, frame0, P, has_bwd, has_start, sticky), two float32 (alpha, beta), fwd
// [K][2][h][w], bwd when has_bwd, state xy [2][P], state status [P], start int32 [P] when has_start.  ROWS: per case xy [K][2][P]
// float32, then status [K][P].  Every array lives in a heap buffer of exactly its size, so a tap outside a field is the sanitizer's to
// see.  No HIP; compile with -ffp-contract=off (tests/test_track_cases_cpu.py).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../track_core.h"

namespace {

bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int die(const char* what) {
    fprintf(stderr, "track_host: %s\n", what);
    return 2;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return die("usage: track_host CASES ROWS");
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return die("cannot open a file");
    int32_t count = 0;
    if (!read_all(in, &count, 4) || count < 0) return die("bad count");
    for (int32_t c = 0; c < count; ++c) {
        int32_t hd[8];
        float ab[2];
        if (!read_all(in, hd, sizeof hd) || !read_all(in, ab, sizeof ab)) return die("short header");
        const int K = hd[0], h = hd[1], w = hd[2], frame0 = hd[3], P = hd[4];
        const bool has_bwd = hd[5] != 0, has_start = hd[6] != 0, sticky = hd[7] != 0;
        if (K < 1 || h < 1 || w < 1 || P < 1 || (int64_t)h * w > (1 << 24) || (int64_t)K * P > (1 << 26)) return die("bad case");
        const size_t plane = (size_t)h * w;
        std::vector<float> fwd((size_t)K * 2 * plane), bwd(has_bwd ? (size_t)K * 2 * plane : 0), sxy((size_t)2 * P);
        std::vector<uint8_t> sst((size_t)P);
        std::vector<int32_t> start(has_start ? (size_t)P : 0);
        if (!read_all(in, fwd.data(), fwd.size() * 4) || !read_all(in, bwd.data(), bwd.size() * 4) || !read_all(in, sxy.data(), sxy.size() * 4) ||
            !read_all(in, sst.data(), sst.size()) || !read_all(in, start.data(), start.size() * 4))
            return die("short case");
        std::vector<float> xy((size_t)K * 2 * P);
        std::vector<uint8_t> status((size_t)K * P);
        for (int i = 0; i < P; ++i) {
            sft_core::Point p;
            p.x = sxy[i], p.y = sxy[(size_t)P + i], p.status = sft_core::read_status(sst[i]);
            const int s0 = has_start ? start[i] : -2147483647 - 1;
            if (p.status == sft_core::kPending && s0 <= frame0) sft_core::activate(p, h, w);
            for (int k = 0; k < K; ++k) {
                sft_core::Field f, b;
                f.u = fwd.data() + (size_t)k * 2 * plane, f.v = f.u + plane, f.row = w;
                b.u = has_bwd ? bwd.data() + (size_t)k * 2 * plane : nullptr, b.v = has_bwd ? b.u + plane : nullptr, b.row = w;
                sft_core::advance_row(p, s0, frame0 + k + 1, f, b, h, w, ab[0], ab[1], sticky);
                xy[((size_t)k * 2) * P + i] = p.x, xy[((size_t)k * 2 + 1) * P + i] = p.y, status[(size_t)k * P + i] = p.status;
            }
        }
        if (fwrite(xy.data(), 4, xy.size(), out) != xy.size() || fwrite(status.data(), 1, status.size(), out) != status.size())
            return die("short write");
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : die("close failed");
}
