// The entropy decoder of one restart interval of a baseline JPEG scan (ITU-T T.81: sequential DCT, 8 bit, Huffman), compilable for the
// host and for the device: the bit reader with its FF 00 unstuffing, the Huffman table construction (Annex C, F.2.2.3), the block
// walk with DC prediction, dequantisation and the coefficient bounds, and the geometry both sides share (where a block of an MCU
// lives, which descriptors are acceptable, how the intervals' statuses become an image's).  It owns no memory: input bytes come
// through the policy's bytes(), coefficients leave through the policy's coef() / store(), and the tables live where the policy's
// caller put them (LDS for csrc/jpeg_decode.hip's wave, the stack for csrc/host/jpeg_decode_host_main.cpp's serial program, which
// is what runs under the host sanitizers).
//
// The two invariants, for ANY input bytes, descriptor words and table bytes:
//   (a) bounds.  Input: Bits::refill asks the policy for bytes [pos, pos + k) only with k <= in_len - pos, on the line above the
//       call; pos never decreases and never passes in_len.  Tables: a Huffman specification is read at offsets 0 .. kSpecBytes - 1 of
//       a component's fixed-stride record and nowhere else; every index into Huff::vals is masked to 0 .. 255 (and is in range
//       anyway: build_huff refuses a specification with more than 256 codes or more codes of a length than that length has
//       patterns, and a canonical prefix that is <= maxcode[len] after being > maxcode of every shorter length is >= that length's
//       first code -- induction over the length); Huff::fast is indexed by kFastBits bits, maxcode / valoff by a length 1 .. 16,
//       Tables::zz by k <= 63, Tables::quant by a zigzag entry <= 63.  Output: decode_interval hands the policy (component c, MCU
//       mi, block j) only with c < nc, first_mcu <= mi < first_mcu + n_mcus, j < blocks of that component in an MCU; desc_ok has
//       checked first_mcu + n_mcus <= the image's MCU count and image < n_images, so block_index() lies inside the image's own
//       coefficient area, and inside the part of it that belongs to this interval's MCUs.
//   (b) progress.  With in_len input bytes and n_mcus MCUs of at most 6 blocks:
//         Bits::refill     each iteration of its loop moves pos forward by 1 .. 4 bytes: at most in_len iterations in all;
//         decode_symbol    takes at least 1 bit or returns an error; its slow loop has at most 7 iterations (lengths 10 .. 16);
//         decode_block     its coefficient loop decodes one symbol per iteration and ends at k = 64, EOB or an error;
//         decode_interval  one decode_block per block, at most 6 n_mcus, each of which takes at least one bit or ends the interval.
//       The unstuffed input has at most 8 in_len bits and no bit is handed out twice, so an interval ends within
//       8 in_len symbol decodes + in_len refill steps + min(6 n_mcus, 8 in_len + 1) block stores; table construction is a
//       constant 16 + 256 + 2^kFastBits kFastBits steps per table.  Nothing waits for anything.
//
// The coefficient bounds (what csrc/jpeg_decode.hip's inverse DCT needs; tests/jpeg_decode_cases.idct_bounds() recomputes them):
//   every dequantised coefficient has |c| <= kCoefMax = 2048, and the 64 of a block have sum |c| <= kBlockSumMax = 18432; a block
//   beyond either ends its interval with kCoefRange.  No file made from 8-bit samples gets there.  The exact DCT F of a block of
//   samples - 128 in -128 .. 127 has |F| <= 1024 (DC: the sum / 8; AC: the absolute values of a basis function sum to at most 8, the
//   encoder's comment in include/streamflow_hip.h) and, being orthonormal, sum |F| <= 8 ||F||_2 = 8 ||s||_2 <= 8 x 8 x 128 =
//   8192.  A quantiser that rounds to the nearest level or towards zero gives a dequantised value q round(F / q) that is 0 or at
//   most |F| + q / 2 <= 2 |F|, and q <= 255 in an 8-bit table: |c| <= 1024 + 127.5 and sum |c| <= 16384 (an integer forward
//   transform adds a fraction per coefficient; the slack of 2048 takes it).  Why two bounds: the per-coefficient bound alone does
//   not keep the second pass of the integer inverse DCT inside 32 bits -- 64 coefficients of 2048 with the signs of one output
//   sample's basis reach 1.74 x 2^31 -- while with both every intermediate of either pass stays below 0.88 x 2^31 (pass 1: at
//   most 2048 x 61 214 + 1024; pass 2: the weights |a_u| |b_v| / 2^11 of an intermediate on the 64 coefficients, the largest nine
//   of them at 2048 each).
//
// Policy P (one object per interval; on the device every member is called by all 64 lanes with the same arguments):
//   uint32_t bytes(int64_t pos, int k)      input bytes pos .. pos + k - 1 (1 <= k <= 4), big-endian: byte pos is the most significant
//   uint32_t uni(uint32_t v)                v, known to be the same in every lane (host: v)
//   int lane(), lanes()                     this caller's share of a table fill
//   void sync()                             table entries written by any lane are visible to all
//   void coef(int k, int v)                 coefficient k (natural order) of the current block = v; the others stay 0
//   void store(int c, int64_t mi, int j)    the current block is block j of component c in MCU mi of the interval's image: write its
//                                           64 coefficients and start the next block from zeros
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SF_JPEGDEC_FN __host__ __device__ __forceinline__
#else
#define SF_JPEGDEC_FN inline
#endif

namespace sf_jpegdec {

// status words (include/streamflow_hip.h SF_JPEG_*)
enum : int {
    kOk = 0,
    kBadCode = 1,       // bits that are no code of the table
    kBadRun = 2,        // a run past coefficient 63, a ZRL with no coefficient left to follow it, or a run / size symbol baseline lacks
    kBadCategory = 3,   // DC category above 11 or AC category above 10
    kTruncated = 4,     // the interval's input ends inside an MCU
    kNotConsumed = 5,   // behind the last MCU more than 7 bits remain, or the remaining bits are not all 1
    kBadDesc = 6,       // a descriptor outside the buffers, the images, the MCUs or the table sets; or an image whose intervals do not
                        // cover its MCUs exactly once
    kCoefRange = 7,     // a dequantised coefficient beyond kCoefMax, or a block whose absolute values sum beyond kBlockSumMax
    kBadTable = 8,      // a Huffman specification with more than 256 codes or more codes of a length than the length has patterns
    kBadMarker = 9,     // an FF byte inside the interval that is not followed by 00
};

constexpr int kCoefMax = 2048, kBlockSumMax = 18432;
constexpr int kFastBits = 9;
constexpr int kDescWords = 6;                                               // in_off, in_len, image, first_mcu, n_mcus, table_set
constexpr int kSpecBytes = 16 + 256;                                        // BITS, HUFFVAL (unused entries: any value)
constexpr int kCompBytes = 64 + 2 * kSpecBytes;                             // quantisation steps (natural order), DC spec, AC spec
constexpr int kSetBytes = 3 * kCompBytes;
constexpr int kMaxIntervals = 1 << 26;

struct Huff {
    int32_t maxcode[17];                                                    // [length]: the largest code of that length, -1: none
    int32_t valoff[17];                                                     // [length]: index of its first symbol - its first code
    uint16_t fast[1 << kFastBits];                                          // length << 8 | symbol of the code the bits start with; 0: longer
    uint8_t vals[256];
};

struct Tables {
    Huff dc[3], ac[3];
    uint8_t quant[3][64];                                                   // natural order
    uint8_t zz[64];                                                         // scan position -> natural index
};

// Where the blocks of a batch live: coefficients as [image][component][block row][block column][64].
struct Geom {
    int nc, hs, vs;                                                         // components; the luma sampling (chroma is 1 x 1)
    int mcux, mcuy;
    int bw[3], bh[3];                                                       // blocks per component
    int64_t comp_off[3], image_blocks;                                      // in blocks
};

SF_JPEGDEC_FN Geom make_geom(int h, int w, int nc, int hs, int vs) {
    Geom g;
    g.nc = nc, g.hs = hs, g.vs = vs;
    g.mcux = (w + 8 * hs - 1) / (8 * hs), g.mcuy = (h + 8 * vs - 1) / (8 * vs);
    int64_t off = 0;
    for (int c = 0; c < 3; ++c) {
        g.bw[c] = c < nc ? g.mcux * (c == 0 ? hs : 1) : 0;
        g.bh[c] = c < nc ? g.mcuy * (c == 0 ? vs : 1) : 0;
        g.comp_off[c] = off;
        off += (int64_t)g.bw[c] * g.bh[c];
    }
    g.image_blocks = off;
    return g;
}

// g.bw[c] and its like by selection: a register array indexed by a variable would live in scratch memory on the device
template <class T>
SF_JPEGDEC_FN T pick3(const T* v, int c) { return c == 0 ? v[0] : c == 1 ? v[1] : v[2]; }

SF_JPEGDEC_FN int64_t mcu_count(const Geom& g) { return (int64_t)g.mcux * g.mcuy; }
SF_JPEGDEC_FN int comp_blocks(const Geom& g, int c) { return c == 0 ? g.hs * g.vs : 1; }

// Block j of component c in MCU mi of image `image`, counted in blocks from the start of the coefficient area.
SF_JPEGDEC_FN int64_t block_index(const Geom& g, int64_t image, int c, int64_t mi, int j) {
    const int ch = c == 0 ? g.hs : 1, cv = c == 0 ? g.vs : 1;
    const int64_t my = mi / g.mcux, mx = mi - my * g.mcux;
    return image * g.image_blocks + pick3(g.comp_off, c) + (my * cv + j / ch) * pick3(g.bw, c) + mx * ch + j % ch;
}

// One descriptor row against the buffers (written so that no sum overflows).
SF_JPEGDEC_FN bool desc_ok(const int64_t* d, int64_t data_bytes, int n_images, int64_t mcus, int n_sets) {
    const int64_t in_off = d[0], in_len = d[1], image = d[2], first = d[3], n = d[4], set = d[5];
    return in_off >= 0 && in_len >= 0 && in_off <= data_bytes && in_len <= data_bytes - in_off && image >= 0 && image < n_images &&
           first >= 0 && n >= 1 && first <= mcus && n <= mcus - first && set >= 0 && set < n_sets;
}

// The image a descriptor's status is reported at: its own, or the nearest one where `image` is out of range.
SF_JPEGDEC_FN int64_t desc_image(const int64_t* d, int n_images) { return d[2] < 0 ? 0 : d[2] >= n_images ? n_images - 1 : d[2]; }

// An image's status from its intervals': `first_error` is (interval << 5 | status) of the failed interval with the lowest number,
// or < 0 for none; `covered` the MCUs of its clean intervals.
SF_JPEGDEC_FN int image_status(int64_t first_error, int64_t covered, int64_t mcus) {
    if (first_error >= 0) return (int)(first_error & 31);
    return covered == mcus ? kOk : kBadDesc;
}

// T.81 figure A.6, eight entries of six bits per word.
SF_JPEGDEC_FN int zigzag(int k) {
    constexpr uint64_t w0 = 0ull | 1ull << 6 | 8ull << 12 | 16ull << 18 | 9ull << 24 | 2ull << 30 | 3ull << 36 | 10ull << 42;
    constexpr uint64_t w1 = 17ull | 24ull << 6 | 32ull << 12 | 25ull << 18 | 18ull << 24 | 11ull << 30 | 4ull << 36 | 5ull << 42;
    constexpr uint64_t w2 = 12ull | 19ull << 6 | 26ull << 12 | 33ull << 18 | 40ull << 24 | 48ull << 30 | 41ull << 36 | 34ull << 42;
    constexpr uint64_t w3 = 27ull | 20ull << 6 | 13ull << 12 | 6ull << 18 | 7ull << 24 | 14ull << 30 | 21ull << 36 | 28ull << 42;
    constexpr uint64_t w4 = 35ull | 42ull << 6 | 49ull << 12 | 56ull << 18 | 57ull << 24 | 50ull << 30 | 43ull << 36 | 36ull << 42;
    constexpr uint64_t w5 = 29ull | 22ull << 6 | 15ull << 12 | 23ull << 18 | 30ull << 24 | 37ull << 30 | 44ull << 36 | 51ull << 42;
    constexpr uint64_t w6 = 58ull | 59ull << 6 | 52ull << 12 | 45ull << 18 | 38ull << 24 | 31ull << 30 | 39ull << 36 | 46ull << 42;
    constexpr uint64_t w7 = 53ull | 60ull << 6 | 61ull << 12 | 54ull << 18 | 47ull << 24 | 55ull << 30 | 62ull << 36 | 63ull << 42;
    const int r = (k >> 3) & 7;
    const uint64_t w = r == 0 ? w0 : r == 1 ? w1 : r == 2 ? w2 : r == 3 ? w3 : r == 4 ? w4 : r == 5 ? w5 : r == 6 ? w6 : w7;
    return (int)(w >> (6 * (k & 7))) & 63;
}

// MSB-first bits of the interval with the stuffing removed: buf holds cnt valid bits at its top, zeros below them.
template <class P>
struct Bits {
    P& p;
    int64_t in_len, pos;                                                    // pos: the next input byte to enter buf
    uint64_t buf;
    int cnt;
    int err;                                                                // kBadMarker once an FF without its 00 was met

    // top up to more than 32 bits, or to the end of the input
    SF_JPEGDEC_FN void refill() {
        while (cnt <= 32 && pos < in_len) {                                 // (b) pos grows in every iteration
            const int64_t left = in_len - pos;
            const int k = left < 4 ? (int)left : 4;
            const uint32_t w = p.bytes(pos, k);                             // (a) k <= in_len - pos
            const uint32_t inv = ~w;
            if (k == 4 && ((inv - 0x01010101u) & ~inv & 0x80808080u) == 0) {   // no FF among the four
                buf |= (uint64_t)w << (32 - cnt);
                cnt += 32, pos += 4;
                continue;
            }
            const uint32_t b = (w >> (8 * (k - 1))) & 255;
            if (b != 255) {
                pos += 1;
            } else if (k >= 2 && ((w >> (8 * (k - 2))) & 255) == 0) {
                pos += 2;
            } else {                                                        // a marker, or the input ends behind the FF
                err = kBadMarker;
                pos = in_len;
                return;
            }
            buf |= (uint64_t)b << (56 - cnt);
            cnt += 8;
        }
    }
    SF_JPEGDEC_FN int failure() const { return err ? err : kTruncated; }
    SF_JPEGDEC_FN bool take(int n, uint32_t& v) {                           // 1 <= n <= 16
        if (cnt < n) {
            refill();
            if (cnt < n) return false;
        }
        v = (uint32_t)(buf >> (64 - n));
        buf <<= n, cnt -= n;
        return true;
    }
};

// BITS and HUFFVAL (spec[0 .. 16), spec[16 .. 272)) -> the decoder's arrays.  Every lane computes the same codes; lane 0 writes them.
template <class P>
SF_JPEGDEC_FN int build_huff(P& p, Huff& t, const uint8_t* spec) {
    int code = 0, k = 0, st = kOk;
    for (int len = 1; len <= 16; ++len) {
        const int n = (int)p.uni(spec[len - 1]);
        int mc = -1, vo = 0;
        if (n > 0) {
            vo = k - code;
            code += n, k += n;
            mc = code - 1;
            if (code > (1 << len)) st = kBadTable;
        }
        if (p.lane() == 0) t.maxcode[len] = mc, t.valoff[len] = vo;
        code <<= 1;
    }
    if (k > 256) st = kBadTable;
    if (p.lane() == 0) t.maxcode[0] = -1, t.valoff[0] = 0;
    for (int i = p.lane(); i < 256; i += p.lanes()) t.vals[i] = spec[16 + i];
    p.sync();
    if (st != kOk) return st;
    for (int i = p.lane(); i < (1 << kFastBits); i += p.lanes()) {
        uint32_t e = 0;
        for (int len = 1; len <= kFastBits; ++len) {
            const int c = i >> (kFastBits - len);
            if (c <= t.maxcode[len]) {
                e = (uint32_t)len << 8 | t.vals[(t.valoff[len] + c) & 255];
                break;
            }
        }
        t.fast[i] = (uint16_t)e;
    }
    p.sync();
    return kOk;
}

// One table set -> the tables of the nc components.
template <class P>
SF_JPEGDEC_FN int build_tables(P& p, Tables& t, const uint8_t* set, int nc) {
    for (int i = p.lane(); i < 64; i += p.lanes()) t.zz[i] = (uint8_t)zigzag(i);
    int st = kOk;
    for (int c = 0; c < nc; ++c) {
        const uint8_t* rec = set + c * kCompBytes;
        for (int i = p.lane(); i < 64; i += p.lanes()) t.quant[c][i] = rec[i];
        const int s1 = build_huff(p, t.dc[c], rec + 64);
        const int s2 = build_huff(p, t.ac[c], rec + 64 + kSpecBytes);
        if (st == kOk) st = s1 != kOk ? s1 : s2;
    }
    p.sync();
    return st;
}

// One symbol.  >= 0: the symbol; < 0: -status.  B is a bit reader with Bits' members buf, cnt, refill() and failure(): Bits itself, or
// the flat reader of csrc/jpeg_sync_core.h.
template <class P, class B>
SF_JPEGDEC_FN int decode_symbol(P& p, B& b, const Huff& t) {
    if (b.cnt < 16) b.refill();
    const uint32_t look = (uint32_t)(b.buf >> 48);                          // bits past cnt are zero
    const uint32_t e = p.uni(t.fast[look >> (16 - kFastBits)]);
    int len = (int)(e >> 8), sym = (int)(e & 255);
    if (len == 0) {
        for (len = kFastBits + 1; len <= 16; ++len) {                       // (b) at most 7 iterations
            const int c = (int)(look >> (16 - len));
            if (c <= (int)p.uni((uint32_t)t.maxcode[len])) {
                sym = (int)p.uni(t.vals[((int)p.uni((uint32_t)t.valoff[len]) + c) & 255]);
                break;
            }
        }
        if (len > 16) return b.cnt < 16 ? -b.failure() : -kBadCode;
    }
    if (len > b.cnt) return -b.failure();                                   // no code as short as what is left starts here
    b.buf <<= len, b.cnt -= len;
    return sym;
}

// `s` more bits as a signed value of category s (T.81 F.2.2.1 EXTEND), 1 <= s <= 11.
template <class B>
SF_JPEGDEC_FN bool receive(B& b, int s, int& v) {
    uint32_t raw;
    if (!b.take(s, raw)) return false;
    v = (int)raw < (1 << (s - 1)) ? (int)raw - (1 << s) + 1 : (int)raw;
    return true;
}

// One block of component c: the DC difference on top of pred, the AC coefficients, dequantised, through p.coef().
template <class P>
SF_JPEGDEC_FN int decode_block(P& p, Bits<P>& b, const Tables& t, int c, int& pred) {
    int s = decode_symbol(p, b, t.dc[c]);
    if (s < 0) return -s;
    if (s > 11) return kBadCategory;
    int v = 0;
    if (s > 0 && !receive(b, s, v)) return b.failure();
    pred += v;
    if (pred > kCoefMax || pred < -kCoefMax) return kCoefRange;             // also keeps pred itself from overflowing
    v = pred * (int)p.uni(t.quant[c][0]);
    if (v > kCoefMax || v < -kCoefMax) return kCoefRange;
    p.coef(0, v);
    int sum = v < 0 ? -v : v;
    for (int k = 1; k < 64;) {                                              // (b) one symbol per iteration
        const int rs = decode_symbol(p, b, t.ac[c]);
        if (rs < 0) return -rs;
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r == 0) break;                                              // EOB
            if (r != 15 || k + 16 > 63) return kBadRun;                     // a ZRL must leave room for the coefficient it precedes
            k += 16;
            continue;
        }
        if (s > 10) return kBadCategory;
        k += r;
        if (k > 63) return kBadRun;
        if (!receive(b, s, v)) return b.failure();
        const int nat = (int)p.uni(t.zz[k]) & 63;
        v *= (int)p.uni(t.quant[c][nat]);                                   // |v| < 2^10, a step < 2^8
        if (v > kCoefMax || v < -kCoefMax) return kCoefRange;
        sum += v < 0 ? -v : v;
        p.coef(nat, v);
        ++k;
    }
    return sum > kBlockSumMax ? kCoefRange : kOk;
}

// The n_mcus MCUs of one restart interval, starting at MCU first_mcu of its image; DC prediction starts at 0.
template <class P>
SF_JPEGDEC_FN int decode_interval(P& p, const Tables& t, const Geom& g, int64_t in_len, int64_t first_mcu, int64_t n_mcus) {
    Bits<P> b{p, in_len, 0, 0, 0, 0};
    int pred0 = 0, pred1 = 0, pred2 = 0;
    for (int64_t m = 0; m < n_mcus; ++m) {
        for (int c = 0; c < g.nc; ++c) {
            const int nb = comp_blocks(g, c);
            for (int j = 0; j < nb; ++j) {
                int pred = c == 0 ? pred0 : c == 1 ? pred1 : pred2;
                const int st = decode_block(p, b, t, c, pred);
                if (st != kOk) return st;
                if (c == 0) pred0 = pred;
                else if (c == 1) pred1 = pred;
                else pred2 = pred;
                p.store(c, first_mcu + m, j);                               // (a) c < nc, first_mcu <= mi < first_mcu + n_mcus, j < nb
            }
        }
    }
    b.refill();
    if (b.err) return b.err;
    if (b.pos < in_len || b.cnt > 7) return kNotConsumed;
    if (b.cnt > 0 && (b.buf >> (64 - b.cnt)) != (1ull << b.cnt) - 1) return kNotConsumed;
    return kOk;
}

}  // namespace sf_jpegdec
