// csrc/jpeg_decode_core.h with a serial policy, as a program of its own: what tests/test_jpeg_decode_core_host_cpu.py compiles with
// -fsanitize=address,undefined and runs as a separate process.  It does for every call what jpeg_entropy_kernel and
// jpeg_status_kernel do on the device -- descriptor check, table build, the interval's decode, the image's status -- with the
// core's own functions.  The data, the descriptors, the tables and the coefficient area are heap buffers of exactly their sizes,
// so a read or write outside any of them -- invariant (a) of the core -- is a sanitizer report, and a loop that does not end is a
// hung test.  No HIP, no device: the decoder core is the code the kernel shares, the policy below is not.
//
//   jpeg_decode_host <cases> <results>
//   cases:   int32 n_calls; per call int32 h, w, components, hs, vs, n_images, n_intervals, n_sets; int64 data_bytes; the data; the
//            descriptors (n_intervals x 6 int64); the tables (n_sets x 1824 bytes)
//   results: per call int32 status[n_images], int32 interval_status[n_intervals], int16 coefficients[n_images x blocks x 64] in the
//            device's layout, prefilled with 0x5A5A
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../jpeg_decode_core.h"

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
    int32_t n_calls = 0;
    if (!get(fi, &n_calls, 4) || n_calls < 0) return 2;
    for (int32_t call = 0; call < n_calls; ++call) {
        int32_t hd[8];
        int64_t data_bytes = 0;
        if (!get(fi, hd, sizeof hd) || !get(fi, &data_bytes, 8) || data_bytes < 0) return 2;
        const int h = hd[0], w = hd[1], nc = hd[2], hs = hd[3], vs = hd[4], n_images = hd[5], n_intervals = hd[6], n_sets = hd[7];
        if (h < 1 || w < 1 || h > 8192 || w > 8192 || (nc != 1 && nc != 3) || hs < 1 || hs > 2 || vs < 1 || vs > 2 || n_images < 1 ||
            n_intervals < 1 || n_sets < 1)
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
        memset(coef, 0x5A, (size_t)ncoef * 2);
        std::vector<int32_t> ist(n_intervals), status(n_images);
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
                if (st == kOk) st = decode_interval(p, t, g, d[1], d[3], d[4]);
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
        fwrite(coef, 2, (size_t)ncoef, fo);
        free(data), free(desc), free(tabs), free(coef);
    }
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 2;
}
