// The self-synchronising decode of one LONG restart interval (a file without DRI is one interval with all its MCUs), on top of
// csrc/jpeg_decode_core.h: the method of Klein and Wiseman (parallel Huffman decoding), applied to JPEG by Weissenberger and
// Schmidt.  The interval's bytes are unstuffed once into a flat stream; the stream is cut into segments of segment_bytes; every
// segment is decoded speculatively from its first bit; the chains of exit states are extended until every segment's entry state is
// its predecessor's exit state; then every segment is decoded again, for real, from its now-known entry.  Like the core it owns
// no memory and compiles for the host: csrc/jpeg_decode.hip runs these functions a thread per segment, and
// csrc/host/jpeg_sync_host_main.cpp runs them phase by phase, segment by segment, under the host sanitizers.
//
// A STATE is (bit, slot, k): the offset of the next symbol's first bit in the unstuffed stream, the block slot inside the MCU
// (0 .. hs vs - 1: the luma blocks, then Cb, then Cr; a grey file has slot 0 only) and the zigzag index of the next coefficient,
// k = 0 meaning that the next symbol is a DC symbol.  decode_step() moves a state over one symbol with decode_block's checks in
// decode_block's order; two walks share it:
//   lenient_segment  stores nothing.  ANY error (no code, a run past 63, a category baseline lacks) ends the current block ONE BIT
//                    behind the failed symbol's first bit, and decoding goes on with the next slot's DC symbol.  A speculative
//                    chain therefore never dies -- a dead chain would let the truth advance one segment per round only -- and on a
//                    valid stream, from a true state, it takes exactly the steps of the strict walk.  It counts the blocks it ends.
//   strict_segment   from a true entry state: the coefficients leave through the sink, the AC ones dequantised, the DC one as the
//                    raw difference (a segment does not know its predecessor's prediction: dc_value() adds the predictions up
//                    afterwards, from 64-bit prefix sums).  The first error ends the walk and goes to the sink with its KEY.
// Both stop at the first symbol boundary at or behind the segment's end, or where the stream has no bits left for a symbol.
//
// An error's KEY is (block ordinal in the interval) << 6 | phase << 4 | status: phase 0 the DC range checks, 1 an entropy error
// (the coefficient range check of an AC coefficient included), 2 the block's sum.  The interval's status is the status of its
// SMALLEST key: the first error in stream order, the only one that means anything -- the segments behind it hold garbage by
// construction.  The end-of-interval check (at most 7 bits left, all 1, no marker) has ordinal = the interval's block count.
//
// The two invariants, for ANY input (the core's header has the ones of decode_symbol and the tables):
//   (a) bounds.  unstuff_chunk() reads in[j] for lo - 1 <= j <= hi only with 0 <= j < in_len, and writes dst[0 .. count).  FlatBits reads
//       u[q] only for q < ulen.  strict_segment hands the sink a coefficient only while ordinal < total = n_mcus x blocks per MCU,
//       with mcu = ordinal / blocks per MCU < n_mcus and slot < blocks per MCU: inside the interval's own MCUs.
//   (b) progress.  Every iteration of either walk consumes at least one bit (a symbol, or the lenient rule's single bit) or returns,
//       and the walk stops at end_bit <= 8 ulen: at most 8 segment_bytes + one symbol's bits (16 + 11) from an entry inside the
//       segment.  FlatBits::seek and refill are loops over at most 8 bytes.
#pragma once
#include "jpeg_decode_core.h"

namespace sf_jpegdec {

constexpr int kSegmentBytesMin = 8, kSegmentBytesMax = 4096;
constexpr int kSyncWindow = 256;                                            // segments whose chains are extended together, in stream order

SF_JPEGDEC_FN int blocks_per_mcu(const Geom& g) { return g.nc == 1 ? 1 : g.hs * g.vs + 2; }
SF_JPEGDEC_FN int slot_comp(const Geom& g, int slot) { return slot < g.hs * g.vs ? 0 : slot - g.hs * g.vs + 1; }
SF_JPEGDEC_FN int slot_block(const Geom& g, int slot) { return slot < g.hs * g.vs ? slot : 0; }
SF_JPEGDEC_FN int next_slot(int slot, int bpm) { return slot + 1 >= bpm ? 0 : slot + 1; }

SF_JPEGDEC_FN uint64_t error_key(int64_t ordinal, int phase, int status) { return (uint64_t)ordinal << 6 | (uint64_t)phase << 4 | (uint64_t)status; }
SF_JPEGDEC_FN int key_status(uint64_t key) { return (int)(key & 15); }
constexpr uint64_t kNoError = ~0ull;

// ---- unstuffing: the interval's bytes without the 00 of every FF 00, up to the first FF that no 00 follows -----------------------------
// Byte j is dropped exactly when it is 00 behind an FF (an FF is never dropped, so the rule is local); the stream ends in front of the
// first FF that is the interval's last byte or has another byte than 00 behind it.  Bytes [lo, hi) of the interval: how many of them
// the stream keeps, and whether it ends among them.
// One walk serves both passes (dst = null: count only); it has no early exit and no pointer that moves, only an index.
SF_JPEGDEC_FN int unstuff_chunk(const uint8_t* in, int64_t in_len, int64_t lo, int64_t hi, uint8_t* dst, bool& marker) {
    int n = 0;
    int prev = lo > 0 ? in[lo - 1] : 0;                                     // (a) 0 <= lo - 1
    bool ended = false;
    for (int64_t j = lo; j < hi; ++j) {                                     // (a) lo >= 0, hi <= in_len
        const int b = in[j];
        const int next = j + 1 < in_len ? in[j + 1] : 1;                    // behind the interval: anything but 00
        const bool stuffing = b == 0 && prev == 255;
        ended = ended || (b == 255 && next != 0);
        const bool keep = !stuffing && !ended;
        if (dst && keep) dst[n] = (uint8_t)b;                               // (a) n < the count of the pass before
        n += keep ? 1 : 0;
        prev = b;
    }
    marker = ended;
    return n;
}

SF_JPEGDEC_FN int unstuff_count(const uint8_t* in, int64_t in_len, int64_t lo, int64_t hi, bool& marker) {
    return unstuff_chunk(in, in_len, lo, hi, nullptr, marker);
}

SF_JPEGDEC_FN void unstuff_copy(const uint8_t* in, int64_t in_len, int64_t lo, int64_t hi, uint8_t* dst) {
    bool marker;
    unstuff_chunk(in, in_len, lo, hi, dst, marker);
}

// ---- the flat bit reader: a position is ONE number, a bit offset into the unstuffed bytes -----------------------------------------------
struct FlatBits {
    const uint8_t* u;
    int64_t ulen, pos;                                                      // pos: the next byte to enter buf
    uint64_t buf;                                                           // cnt valid bits at its top, zeros below them
    int cnt;
    int end_err;                                                            // kBadMarker where the stream ends at a marker, else 0

    SF_JPEGDEC_FN void refill() {
        while (cnt <= 56 && pos < ulen) {                                   // (a) pos < ulen; (b) at most 8 iterations
            buf |= (uint64_t)u[pos] << (56 - cnt);
            cnt += 8, ++pos;
        }
    }
    SF_JPEGDEC_FN void seek(int64_t bit) {                                  // 0 <= bit <= 8 ulen
        pos = bit >> 3, buf = 0, cnt = 0;
        if (pos > ulen) pos = ulen;
        refill();
        const int r = (int)(bit & 7);
        if (cnt >= r) buf <<= r, cnt -= r;
    }
    SF_JPEGDEC_FN int64_t at() const { return 8 * pos - cnt; }
    SF_JPEGDEC_FN int failure() const { return end_err ? end_err : kTruncated; }
    SF_JPEGDEC_FN bool take(int n, uint32_t& v) {                           // 1 <= n <= 16
        if (cnt < n) {
            refill();
            if (cnt < n) return false;
        }
        v = (uint32_t)(buf >> (64 - n));
        buf <<= n, cnt -= n;
        return true;
    }
    // behind the interval's last block: decode_interval's closing check
    SF_JPEGDEC_FN int end_status() {
        if (end_err) return end_err;
        refill();
        if (pos < ulen || cnt > 7) return kNotConsumed;
        if (cnt > 0 && (buf >> (64 - cnt)) != (1ull << cnt) - 1) return kNotConsumed;
        return kOk;
    }
};

// One symbol of a block of component c whose next zigzag index is k (0: the DC symbol), with decode_block's checks in its order.
// kOk: k is the next index, 64 where the block is complete; zi >= 0 where the symbol carried a value v for zigzag index zi (zi = 0:
// the raw DC difference).  Any other status: k is unchanged and the reader is wherever the failure left it.
template <class P>
SF_JPEGDEC_FN int decode_step(P& p, FlatBits& b, const Tables& t, int c, int& k, int& zi, int& v) {
    zi = -1;
    if (k == 0) {
        const int s = decode_symbol(p, b, t.dc[c]);
        if (s < 0) return -s;
        if (s > 11) return kBadCategory;
        v = 0;
        if (s > 0 && !receive(b, s, v)) return b.failure();
        zi = 0, k = 1;
        return kOk;
    }
    const int rs = decode_symbol(p, b, t.ac[c]);
    if (rs < 0) return -rs;
    const int r = rs >> 4, s = rs & 15;
    if (s == 0) {
        if (r == 0) {
            k = 64;                                                         // EOB
            return kOk;
        }
        if (r != 15 || k + 16 > 63) return kBadRun;
        k += 16;
        return kOk;
    }
    if (s > 10) return kBadCategory;
    if (k + r > 63) return kBadRun;
    if (!receive(b, s, v)) return b.failure();
    zi = k + r, k = zi + 1;
    return kOk;
}

struct SegExit {
    int64_t bit;
    int slot, k;
    int blocks;                                                             // blocks ended on the way
};

// The lenient walk from (bit, slot, k) to the first symbol boundary at or behind end_bit (<= 8 ulen), or to the last boundary in
// front of a symbol the stream has no bits left for.
template <class P>
SF_JPEGDEC_FN SegExit lenient_segment(P& p, const Tables& t, const Geom& g, const uint8_t* u, int64_t ulen, int end_err, int64_t bit,
                                      int slot, int k, int64_t end_bit) {
    FlatBits b{u, ulen, 0, 0, 0, end_err};
    b.seek(bit);
    const int bpm = blocks_per_mcu(g);
    int blocks = 0;
    while (b.at() < end_bit) {                                              // (b) every iteration moves at() forward or returns
        const int64_t at0 = b.at();
        int zi, v;
        const int st = decode_step(p, b, t, slot_comp(g, slot), k, zi, v);
        if (st == kTruncated || st == kBadMarker) return SegExit{at0, slot, k, blocks};
        if (st != kOk) {                                                    // the lenient rule
            b.seek(at0 + 1);                                                // at0 < end_bit <= 8 ulen
            k = 64;
        }
        if (k == 64) k = 0, slot = next_slot(slot, bpm), ++blocks;
    }
    return SegExit{b.at(), slot, k, blocks};
}

// The strict walk of one segment from its TRUE entry state; `ordinal` is the number of blocks the interval's stream has ended in
// front of the entry, `total` the interval's block count, `last` whether the stream ends with this segment.  Sink S:
//   void begin(int64_t mcu, int slot)                  the coefficients that follow belong to this block of the interval (mcu counted
//                                                      from the interval's first; mcu < n_mcus)
//   void put(int nat, int v)                           coefficient `nat` (natural order) of that block: dequantised, or for nat = 0
//                                                      the raw DC difference (|v| <= 2047)
//   void error(int64_t ordinal, int phase, int status)
template <class P, class S>
SF_JPEGDEC_FN void strict_segment(P& p, S& sink, const Tables& t, const Geom& g, const uint8_t* u, int64_t ulen, int end_err, int64_t bit,
                                  int slot, int k, int64_t end_bit, int64_t ordinal, int64_t total, bool last) {
    if (ordinal >= total) return;
    FlatBits b{u, ulen, 0, 0, 0, end_err};
    b.seek(bit);
    const int bpm = blocks_per_mcu(g);
    int64_t mcu = ordinal / bpm;
    sink.begin(mcu, slot);                                                  // (a) ordinal < total = n_mcus bpm
    while (b.at() < end_bit) {                                              // (b) a symbol per iteration
        const int c = slot_comp(g, slot);
        int zi, v;
        int st = decode_step(p, b, t, c, k, zi, v);
        if (st == kOk && zi > 0) {
            const int nat = (int)p.uni(t.zz[zi]) & 63;
            v *= (int)p.uni(t.quant[c][nat]);                               // |v| < 2^10, a step < 2^8
            if (v > kCoefMax || v < -kCoefMax) st = kCoefRange;
            else sink.put(nat, v);
        } else if (st == kOk && zi == 0) {
            sink.put(0, v);
        }
        if (st != kOk) {
            sink.error(ordinal, 1, st);
            return;
        }
        if (k == 64) {
            k = 0, slot = next_slot(slot, bpm), ++ordinal;
            if (slot == 0) ++mcu;
            if (ordinal == total) {                                         // this walk ended the interval's last block
                st = b.end_status();
                if (st != kOk) sink.error(total, 0, st);
                return;
            }
            sink.begin(mcu, slot);                                          // (a) ordinal < total
        }
    }
    if (last) sink.error(ordinal, 1, b.failure());                          // the stream ends in front of the interval's last block
}

// The DC coefficient of a block from the component's prediction (the 64-bit sum of the differences up to and including this block's):
// decode_block's two checks.
SF_JPEGDEC_FN int dc_value(int64_t pred, int q0, int& v) {
    v = 0;
    if (pred > kCoefMax || pred < -kCoefMax) return kCoefRange;
    const int d = (int)pred * q0;
    if (d > kCoefMax || d < -kCoefMax) return kCoefRange;
    v = d;
    return kOk;
}

}  // namespace sf_jpegdec
