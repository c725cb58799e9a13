// csrc/inflate_core.h with a serial emit policy, as a program of its own: what tests/test_inflate_core_host_cpu.py compiles with
// -fsanitize=address,undefined and runs as a separate process.  Every stream gets heap buffers of exactly in_len and out_len bytes,
// so a read or write outside either -- invariant (a) of the core -- is a sanitizer report, and a loop that does not end is a hung
// test.  No HIP, no device: the decoder core is the code the kernel shares, the policy below is not.
//
//   inflate_host <cases> <results>
//   cases:   int32 n; per stream int64 in_len, int64 out_len, int32 stored, in_len bytes
//   results: per stream int32 status, out_len bytes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../inflate_core.h"

namespace {

struct SerialPolicy {
    const uint8_t* in;
    uint8_t* out;

    uint64_t bytes(int64_t pos, int k) {
        uint64_t v = 0;
        for (int i = 0; i < k; ++i) v |= (uint64_t)in[pos + i] << (8 * i);
        return v;
    }
    uint32_t uni(uint32_t v) { return v; }
    int lane() { return 0; }
    int lanes() { return 1; }
    void sync() {}
    void lit(int64_t at, uint32_t b) { out[at] = (uint8_t)b; }
    void match(int64_t at, uint32_t dist, uint32_t len) {
        for (uint32_t j = 0; j < len; ++j) out[at + j] = out[at + j - dist];
    }
    void raw(int64_t at, int64_t pos, int64_t n) {
        for (int64_t j = 0; j < n; ++j) out[at + j] = in[pos + j];
    }
    void flush() {}
    uint32_t adler(int64_t n) {
        uint32_t a = 1, b = 0;
        for (int64_t i = 0; i < n; ++i) {
            a = (a + out[i]) % 65521;
            b = (b + a) % 65521;
        }
        return b << 16 | a;
    }
};

bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

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
    int32_t n = 0;
    if (!get(fi, &n, 4) || n < 0) return 2;
    for (int32_t s = 0; s < n; ++s) {
        int64_t in_len = 0, out_len = 0;
        int32_t stored = 0;
        if (!get(fi, &in_len, 8) || !get(fi, &out_len, 8) || !get(fi, &stored, 4) || in_len < 0 || out_len < 0) return 2;
        // exact sizes, from malloc: the sanitizer's red zones start at the first byte outside
        uint8_t* in = (uint8_t*)malloc((size_t)in_len ? (size_t)in_len : 1);
        uint8_t* out = (uint8_t*)malloc((size_t)out_len ? (size_t)out_len : 1);
        if (!in || !out || !get(fi, in, (size_t)in_len)) return 2;
        memset(out, 0xA5, (size_t)out_len);
        int32_t status;
        if (stored) {
            status = in_len > out_len ? sf_zinflate::kOutputLong : in_len < out_len ? sf_zinflate::kOutputShort : sf_zinflate::kOk;
            if (status == sf_zinflate::kOk) memcpy(out, in, (size_t)in_len);
        } else {
            SerialPolicy p{in, out};
            sf_zinflate::Tables t;
            memset(&t, 0xEE, sizeof t);                                     // LDS starts with garbage too: nothing may depend on it
            status = sf_zinflate::inflate_stream(p, t, in_len, out_len);
        }
        fwrite(&status, 4, 1, fo);
        fwrite(out, 1, (size_t)out_len, fo);
        free(in);
        free(out);
    }
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 2;
}
