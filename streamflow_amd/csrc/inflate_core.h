// A zlib (RFC 1950) / deflate (RFC 1951) decoder for one stream, compilable for the host and for the device: the bit reader, the
// canonical-code construction, the symbol decode and the block walk.  It owns no memory and touches none directly: every input
// byte comes through the policy's bytes(), every output byte leaves through the policy's lit() / match() / raw(), and the tables
// live where the policy's caller put them (a Tables in LDS for csrc/flo5_decode.hip's wave, on the stack for
// csrc/host/inflate_host_main.cpp's serial program, which is what runs under the host sanitizers).
//
// The two invariants, for ANY input bytes:
//   (a) bounds: the core asks the policy for input bytes [pos, pos + k) only after checking pos + k <= in_len, and for output
//       positions [at, at + n) only after checking at + n <= out_len and, for a match, dist <= at.  Every check stands on the
//       line(s) right above the call.
//   (b) progress: every iteration of a decode loop -- the block loop, the symbol loop of a Huffman block, the code-length loop of
//       a dynamic header, the bit loop of decode_slow -- takes at least one bit out of the bit reader before it can repeat, and
//       the reader never hands out a bit twice (unread() only returns whole bytes it has not handed out).  With in_len bytes
//       there are 8 in_len bits, so the decode loops together make at most 8 in_len iterations; the copies inside match() / raw()
//       write one output byte per step, at most out_len in all.  The remaining loops (clearing and filling tables) have constant
//       trip counts and run once per block header, which itself costs at least 3 bits.  Nothing waits for anything.
//
// Policy P (one object per stream; on the device every member is called by all 64 lanes with the same arguments):
//   uint64_t bytes(int64_t pos, int k)      input bytes pos .. pos + k - 1 (1 <= k <= 7), little-endian
//   uint32_t uni(uint32_t v)                v, known to be the same in every lane (host: v)
//   int lane(), lanes()                     this caller's share of a table fill
//   void sync()                             table entries written by any lane are visible to all
//   void lit(int64_t at, uint32_t b)        output byte `at` = b
//   void match(int64_t at, uint32_t dist, uint32_t len)     output [at, at + len) = the bytes `dist` back, overlapping allowed
//   void raw(int64_t at, int64_t pos, int64_t n)             output [at, at + n) = input [pos, pos + n)
//   void flush()                            everything handed over so far is in memory
//   uint32_t adler(int64_t n)               Adler-32 of output [0, n)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SF_INFLATE_FN __host__ __device__ __forceinline__
#else
#define SF_INFLATE_FN inline
#endif

namespace sf_zinflate {

// status words (include/streamflow_hip.h SF_INFLATE_*)
enum : int {
    kOk = 0,
    kBadHeader = 1,        // CM != 8, CINFO > 7 or the FCHECK bits
    kTruncated = 2,        // the input ends inside the stream
    kBadBlockType = 3,     // BTYPE 3
    kBadCodeLengths = 4,   // over-subscribed or incomplete set, HLIT / HDIST out of range, a bad repeat, no end-of-block code
    kBadSymbol = 5,        // a bit pattern that is no code, or literal/length 286 / 287, distance 30 / 31
    kBadDistance = 6,      // a distance before the start of the output
    kOutputLong = 7,       // more output than expected
    kOutputShort = 8,      // less output than expected
    kBadAdler = 9,         // the trailer does not match
    kBadStoredLen = 10,    // a stored block's NLEN is not ~LEN
    kPresetDict = 11,      // FDICT
    kBadSlot = 12,         // (kernel only) a stream's input or output range lies outside the buffers
};

constexpr int kLitFastBits = 10, kDistFastBits = 8;

struct Tables {
    uint16_t lit_count[16], dist_count[16], offs[16];
    uint16_t lit_symbol[288], dist_symbol[32];
    uint16_t lit_fast[1 << kLitFastBits], dist_fast[1 << kDistFastBits];   // (symbol << 4) | code length; 0: take decode_slow
    uint8_t lengths[320];
};

template <class P>
struct Bits {
    P& p;
    int64_t in_len, pos;       // pos: the next input byte to enter buf
    uint64_t buf;
    int cnt;                   // valid low bits of buf

    // top up to more than 55 bits, or to the end of the input
    SF_INFLATE_FN void refill() {
        int k = (63 - cnt) >> 3;
        const int64_t left = in_len - pos;
        if (k > left) k = (int)left;
        if (k > 0) {                                                        // (a) pos + k <= in_len
            buf |= p.bytes(pos, k) << cnt;
            pos += k, cnt += 8 * k;
        }
    }
    SF_INFLATE_FN bool take(int n, uint32_t& v) {                           // n <= 16
        if (cnt < n) {
            refill();
            if (cnt < n) return false;
        }
        v = (uint32_t)buf & ((1u << n) - 1);
        buf >>= n, cnt -= n;
        return true;
    }
    // drop the rest of the current byte and give the whole bytes still in buf back to the input
    SF_INFLATE_FN void unread() {
        cnt -= cnt & 7;
        pos -= cnt >> 3;
        buf = 0, cnt = 0;
    }
};

// RFC 1951 3.2.7: the order of the code-length code's lengths, 5 bits each
SF_INFLATE_FN int cl_order(int i) {
    constexpr uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 |
                            5ull << 45 | 11ull << 50 | 4ull << 55;
    constexpr uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (int)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31);
}

// count[len] = number of symbols of that length, symbol[] = the symbols in canonical order (length, then value).
// Returns 0 for a complete set (or no codes at all), > 0 for an incomplete one, < 0 for an over-subscribed one.
template <class P>
SF_INFLATE_FN int construct(P& p, uint16_t* count, uint16_t* symbol, uint16_t* offs, const uint8_t* length, int n) {
    for (int len = 0; len < 16; ++len) count[len] = 0;
    for (int s = 0; s < n; ++s) {
        const int l = (int)p.uni(length[s]) & 15;
        count[l] = (uint16_t)(count[l] + 1);
    }
    if ((int)p.uni(count[0]) == n) return 0;
    int left = 1;
    for (int len = 1; len < 16; ++len) {
        left = 2 * left - (int)p.uni(count[len]);
        if (left < 0) return left;
    }
    offs[1] = 0;
    for (int len = 1; len < 15; ++len) offs[len + 1] = (uint16_t)(p.uni(offs[len]) + p.uni(count[len]));
    for (int s = 0; s < n; ++s) {
        const int l = (int)p.uni(length[s]) & 15;
        if (l != 0) {
            const int o = (int)p.uni(offs[l]);
            if (o < n) symbol[o] = (uint16_t)s;                             // always: the counts sum to at most n
            offs[l] = (uint16_t)(o + 1);
        }
    }
    return left;
}

// fast[i] for every FB-bit pattern i (bit 0 first): the symbol and length of the code that i starts with, or 0 where that code is
// longer than FB bits or no code at all.  Each lane fills its share; constant trip counts.
template <int FB, class P>
SF_INFLATE_FN void fill_fast(P& p, uint16_t* fast, const uint16_t* count, const uint16_t* symbol, int nsym) {
    for (int i = p.lane(); i < (1 << FB); i += p.lanes()) {
        int code = 0, first = 0, index = 0;
        uint32_t e = 0;
        for (int len = 1; len <= FB; ++len) {
            code |= (i >> (len - 1)) & 1;
            const int c = count[len];
            if (code - c < first) {
                const int at = index + (code - first);
                if (at < nsym) e = (uint32_t)symbol[at] << 4 | (uint32_t)len;
                break;
            }
            index += c, first += c;
            first <<= 1, code <<= 1;
        }
        fast[i] = (uint16_t)e;
    }
    p.sync();
}

// One symbol, a bit at a time (canonical decode: the codes of a length are consecutive).  >= 0: the symbol; < 0: -status.
template <class P>
SF_INFLATE_FN int decode_slow(P& p, Bits<P>& b, const uint16_t* count, const uint16_t* symbol, int nsym) {
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= 15; ++len) {                                   // (b) one bit per iteration
        uint32_t bit;
        if (!b.take(1, bit)) return -kTruncated;
        code |= (int)bit;
        const int c = (int)p.uni(count[len]);
        if (code - c < first) {
            const int at = index + (code - first);
            return at < nsym ? (int)p.uni(symbol[at]) : -kBadSymbol;
        }
        index += c, first += c;
        first <<= 1, code <<= 1;
    }
    return -kBadSymbol;
}

template <int FB, class P>
SF_INFLATE_FN int decode(P& p, Bits<P>& b, const uint16_t* fast, const uint16_t* count, const uint16_t* symbol, int nsym) {
    b.refill();
    const uint32_t e = p.uni(fast[(uint32_t)b.buf & ((1u << FB) - 1)]);     // bits past cnt are zero
    const int len = (int)(e & 15);
    if (len == 0) return decode_slow(p, b, count, symbol, nsym);
    if (len > b.cnt) return -kTruncated;                                    // no code as short as what is left starts here
    b.buf >>= len, b.cnt -= len;
    return (int)(e >> 4);
}

// lengths[0 .. nlen) and lengths[nlen .. nlen + ndist) -> both decoders.  zlib's rule (inftrees.c): an over-subscribed set is an
// error; an incomplete one too, unless it is a single code of one bit.
template <class P>
SF_INFLATE_FN int build_tables(P& p, Tables& t, int nlen, int ndist) {
    int left = construct(p, t.lit_count, t.lit_symbol, t.offs, t.lengths, nlen);
    if (left < 0 || (left > 0 && (int)p.uni(t.lit_count[0]) + (int)p.uni(t.lit_count[1]) != nlen)) return kBadCodeLengths;
    left = construct(p, t.dist_count, t.dist_symbol, t.offs, t.lengths + nlen, ndist);
    if (left < 0 || (left > 0 && (int)p.uni(t.dist_count[0]) + (int)p.uni(t.dist_count[1]) != ndist)) return kBadCodeLengths;
    fill_fast<kLitFastBits>(p, t.lit_fast, t.lit_count, t.lit_symbol, nlen);
    fill_fast<kDistFastBits>(p, t.dist_fast, t.dist_count, t.dist_symbol, ndist);
    return kOk;
}

template <class P>
SF_INFLATE_FN int fixed_tables(P& p, Tables& t) {
    for (int s = 0; s < 288; ++s) t.lengths[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
    for (int s = 0; s < 30; ++s) t.lengths[288 + s] = 5;                    // distance codes 30 / 31 stay without a symbol
    construct(p, t.lit_count, t.lit_symbol, t.offs, t.lengths, 288);
    construct(p, t.dist_count, t.dist_symbol, t.offs, t.lengths + 288, 30);
    fill_fast<kLitFastBits>(p, t.lit_fast, t.lit_count, t.lit_symbol, 288);
    fill_fast<kDistFastBits>(p, t.dist_fast, t.dist_count, t.dist_symbol, 30);
    return kOk;
}

template <class P>
SF_INFLATE_FN int dynamic_tables(P& p, Bits<P>& b, Tables& t, int& nlen, int& ndist) {
    uint32_t v;
    if (!b.take(5, v)) return kTruncated;
    nlen = (int)v + 257;
    if (!b.take(5, v)) return kTruncated;
    ndist = (int)v + 1;
    if (!b.take(4, v)) return kTruncated;
    const int ncode = (int)v + 4;
    if (nlen > 286 || ndist > 30) return kBadCodeLengths;
    for (int i = 0; i < 19; ++i) t.lengths[i] = 0;
    for (int i = 0; i < ncode; ++i) {
        if (!b.take(3, v)) return kTruncated;
        t.lengths[cl_order(i)] = (uint8_t)v;
    }
    // the code-length code sits in the distance decoder's arrays until the real one is built
    if (construct(p, t.dist_count, t.dist_symbol, t.offs, t.lengths, 19) != 0 || (int)p.uni(t.dist_count[0]) == 19) return kBadCodeLengths;
    const int total = nlen + ndist;
    int index = 0;
    while (index < total) {                                                 // (b) decode_slow takes at least one bit
        const int sym = decode_slow(p, b, t.dist_count, t.dist_symbol, 19);
        if (sym < 0) return -sym;
        if (sym < 16) {
            t.lengths[index++] = (uint8_t)sym;
            continue;
        }
        uint32_t prev = 0, rep;
        if (sym == 16) {
            if (index == 0) return kBadCodeLengths;
            prev = p.uni(t.lengths[index - 1]);
            if (!b.take(2, rep)) return kTruncated;
            rep += 3;
        } else if (sym == 17) {
            if (!b.take(3, rep)) return kTruncated;
            rep += 3;
        } else {
            if (!b.take(7, rep)) return kTruncated;
            rep += 11;
        }
        if (index + (int)rep > total) return kBadCodeLengths;
        for (uint32_t r = 0; r < rep; ++r) t.lengths[index++] = (uint8_t)prev;
    }
    if (p.uni(t.lengths[256]) == 0) return kBadCodeLengths;
    return build_tables(p, t, nlen, ndist);
}

// The symbols of one Huffman block up to its end-of-block code.
template <class P>
SF_INFLATE_FN int huffman_block(P& p, Bits<P>& b, Tables& t, int nlen, int ndist, int64_t out_len, int64_t& produced) {
    for (;;) {                                                              // (b) decode takes at least one bit
        const int sym = decode<kLitFastBits>(p, b, t.lit_fast, t.lit_count, t.lit_symbol, nlen);
        if (sym < 0) return -sym;
        if (sym < 256) {
            if (produced >= out_len) return kOutputLong;                    // (a)
            p.lit(produced, (uint32_t)sym);
            ++produced;
            continue;
        }
        if (sym == 256) return kOk;
        const int ls = sym - 257;
        if (ls >= 29) return kBadSymbol;
        uint32_t len = 3 + (uint32_t)ls, ext = 0;
        if (ls == 28) len = 258;
        else if (ls >= 8) {
            const int eb = (ls - 4) >> 2;
            if (!b.take(eb, ext)) return kTruncated;
            len = 3 + ((4 + ((uint32_t)ls & 3)) << eb) + ext;
        }
        const int ds = decode<kDistFastBits>(p, b, t.dist_fast, t.dist_count, t.dist_symbol, ndist);
        if (ds < 0) return -ds;
        if (ds >= 30) return kBadSymbol;
        uint32_t dist = 1 + (uint32_t)ds;
        if (ds >= 4) {
            const int eb = (ds - 2) >> 1;
            if (!b.take(eb, ext)) return kTruncated;
            dist = 1 + ((2 + ((uint32_t)ds & 1)) << eb) + ext;
        }
        if ((int64_t)dist > produced) return kBadDistance;                  // (a) the source starts at produced - dist >= 0
        if ((int64_t)len > out_len - produced) return kOutputLong;          // (a) the copy ends at produced + len <= out_len
        p.match(produced, dist, len);
        produced += len;
    }
}

// One zlib stream of in_len bytes that must inflate to exactly out_len bytes -> status.
template <class P>
SF_INFLATE_FN int inflate_stream(P& p, Tables& t, int64_t in_len, int64_t out_len) {
    if (in_len < 2) return kTruncated;
    const uint32_t hdr = (uint32_t)p.bytes(0, 2), cmf = hdr & 255, flg = hdr >> 8;   // (a) 2 <= in_len
    if ((cmf & 15) != 8 || (cmf >> 4) > 7 || (cmf * 256 + flg) % 31 != 0) return kBadHeader;
    if (flg & 0x20) return kPresetDict;
    Bits<P> b{p, in_len, 2, 0, 0};
    int64_t produced = 0;
    uint32_t last = 0;
    while (!last) {                                                         // (b) a block header is 3 bits
        uint32_t type;
        if (!b.take(1, last) || !b.take(2, type)) return kTruncated;
        if (type == 3) return kBadBlockType;
        if (type == 0) {
            b.unread();
            if (in_len - b.pos < 4) return kTruncated;                      // (a)
            const uint32_t w = (uint32_t)p.bytes(b.pos, 4), len = w & 0xFFFF;
            if ((len ^ 0xFFFF) != w >> 16) return kBadStoredLen;
            b.pos += 4;
            if ((int64_t)len > in_len - b.pos) return kTruncated;           // (a) the source ends at pos + len <= in_len
            if ((int64_t)len > out_len - produced) return kOutputLong;      // (a) the copy ends at produced + len <= out_len
            p.raw(produced, b.pos, (int64_t)len);
            b.pos += len, produced += len;
            continue;
        }
        int nlen = 288, ndist = 30;
        const int st = type == 1 ? fixed_tables(p, t) : dynamic_tables(p, b, t, nlen, ndist);
        if (st != kOk) return st;
        const int sb = huffman_block(p, b, t, nlen, ndist, out_len, produced);
        if (sb != kOk) return sb;
    }
    p.flush();
    if (produced != out_len) return kOutputShort;
    b.unread();
    if (in_len - b.pos < 4) return kTruncated;                              // (a)
    const uint32_t w = (uint32_t)p.bytes(b.pos, 4);
    const uint32_t stored = (w & 255) << 24 | (w >> 8 & 255) << 16 | (w >> 16 & 255) << 8 | w >> 24;
    return p.adler(out_len) == stored ? kOk : kBadAdler;
}

}  // namespace sf_zinflate
