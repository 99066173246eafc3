// word_funnel.h -- one lane's streaming digest over bytes that arrive in pieces at any message
// position (BRB_MD5Init / BRB_MD5UpdateBig per piece / BRB_MD5Final, md5.c:38-168; BrbSha1_Update per
// piece on a context that already holds bytes, sha1.c:143-169).
//
// A carry holds the 0..3 message bytes left over from the previous piece; whole 32-bit message words
// go to the lane's private ring in LDS, word k of lane l at (k * 64 + l) * 4 -- every access of lane
// l hits bank l, no barrier, no cross-lane traffic.  The callers read each piece from `nacc` bytes
// before it, so its words already fall on message word boundaries (head / put16w / put_block /
// put_tail); pump() compresses the oldest 16 once they are there and must run at least once per 16
// words written.  Keeping the compression out of the puts leaves one compress site per caller loop:
// with it inside, a loop of 16 unrolled puts inlined 16 copies of the compression (52 KB of code for
// metadata_unpack_kernel).  A whole block that arrives with nothing pending may be compressed from
// its registers and skip the ring (put_block).
//
// The funnel is generic over the algorithm: A gives State and compress(State &, uint32_t (&)[16]) on
// 16 little-endian message words (Md5Words in md5_device.h; Md5Stream, Sha1Stream in
// digest_stream_kernels.hip), and iv() where a message is started here (init).  It starts from the IV
// or from a context's state and buffered bytes (seed) and ends by handing back the block buffer
// (buffer): the message's byte count and the padding are the caller's (md5_funnel_finish below for
// the MD5 kernels).
#pragma once

#include "byte_stream.h"
#include "md5_device.h"

namespace brb_funnel {

constexpr uint32_t kRingWords = 32;     // per lane: 8 KiB per wave, 32 KiB per 256-lane workgroup

// RW ring words per lane (a multiple of 16, a power of two): the wave's ring is RW x 64 dwords at an
// RW * 256-byte aligned LDS address.  The wave-pair kernels (line_stream.h) put up to 33 words per
// 128-byte line ahead of their partner and take RW = 64; everything else takes 32.
template <class A, uint32_t RW = kRingWords>
struct Funnel {
    static constexpr uint32_t kMask = RW * 256 - 1;
    uint32_t *bb;       // ring word k of this lane at bb[64 k] (LDS)
    uint32_t ring;      // LDS address of this wave's ring (RW * 256-byte aligned), OR'd into word addresses
    uint32_t lane4;     // 4 x lane: the lane's byte within a ring row
    typename A::State st;
    uint32_t acc;       // the carried bytes (low nacc bytes, zeros above)
    uint32_t nacc;      // bytes held in acc (0..3)
    uint32_t wpos;      // words written
    uint32_t cpos;      // words compressed (a multiple of 16)

    // lane_words = &ring[0][lane] of a [RW][64] uint32 array at an RW * 256-byte aligned LDS
    // address, so a word's address is one and-or of its ring offset
    BRB_DEV void place(uint32_t *lane_words)
    {
        bb = lane_words;
        const uint32_t a = uint32_t(reinterpret_cast<uintptr_t>(lane_words));
        ring = a & ~kMask;
        lane4 = a & 0xFFu;
    }

    // A new message: A's IV, nothing buffered, nothing stored to the ring.
    BRB_DEV void init(uint32_t *lane_words)
    {
        place(lane_words);
        st = A::iv();
        acc = nacc = wpos = cpos = 0;
    }

    // A message continued from a context.  Its `have` buffered bytes (in: its block buffer) are the
    // message so far: have >> 2 whole words in the ring, have & 3 bytes carried.  All 16 words are
    // stored -- those from have >> 2 on are overwritten before they are read.
    BRB_DEV void seed(uint32_t *lane_words, const typename A::State &s, const uint32_t (&in)[16], uint32_t have)
    {
        place(lane_words);
        st = s;
#pragma unroll
        for (uint32_t k = 0; k < 16; k++)
            bb[64 * k] = in[k];
        const uint32_t q = have >> 2;
        uint32_t t = 0;
#pragma unroll
        for (uint32_t k = 0; k < 16; k++)
            t = k == q ? in[k] : t;
        nacc = have & 3;
        acc = t & ((1u << (8 * nacc)) - 1u);
        wpos = q;
        cpos = 0;
    }

    static BRB_DEV void lds_st(uint32_t a, uint32_t v) { *reinterpret_cast<__attribute__((address_space(3))) uint32_t *>(a) = v; }

    // word at ring position wpos + i (mod RW): (lane4 + 256 (wpos + i)) mod (RW * 256), in the wave's ring
    BRB_DEV void word_at(uint32_t i, uint32_t w) const
    {
        lds_st(((lane4 + ((wpos + i) << 8)) & kMask) | ring, w);
    }

    // a piece's first word: its low nacc bytes are the carried ones
    BRB_DEV uint32_t head(uint32_t w0) const
    {
        return nacc ? (w0 & ~((1u << (8 * nacc)) - 1u)) | acc : w0;
    }
    BRB_DEV void put16w(const uint32_t (&w)[16])
    {
#pragma unroll
        for (uint32_t i = 0; i < 16; i++)
            word_at(i, w[i]);
        wpos += 16;
    }
    // the first `left` (< 64) bytes of w: whole words to the ring, the rest (zeros past it) carried
    BRB_DEV void put_tail(const uint32_t (&w)[16], uint32_t left)
    {
#pragma unroll
        for (uint32_t i = 0; i < 16; i++)
            if (4 * i + 4 <= left) {
                word_at(0, w[i]);
                ++wpos;
            }
        const uint32_t k = left >> 2;
        uint32_t t = 0;
#pragma unroll
        for (uint32_t i = 0; i < 16; i++)
            t = i == k ? w[i] : t;
        nacc = left & 3;
        acc = nacc ? t : 0u;
    }
    // A piece ended after n bytes, the early ones included.  On a block boundary nothing is carried
    // (its last block went through put16w / put_block, which leave the carry alone).
    BRB_DEV void end_piece(uint64_t n)
    {
        if ((n & 63) == 0) {
            acc = 0;
            nacc = 0;
        }
    }

    // cpos is a multiple of 16, so the 16 words never wrap: one base, immediate offsets
    BRB_DEV void load16(uint32_t (&w)[16]) const
    {
        const uint32_t *b = bb + 64 * (cpos & (RW - 16));
#pragma unroll
        for (uint32_t i = 0; i < 16; i++)
            w[i] = b[64 * i];
    }

    // A whole block of message words still in registers.  With nothing pending it IS the oldest block:
    // it skips the ring (`direct`, to be passed on to pump(w, direct)), which a message that sits on a
    // block boundary -- a fresh context, 64-byte multiples -- then never touches.
    BRB_DEV bool put_block(const uint32_t (&w)[16])
    {
        const bool direct = wpos == cpos;
        if (direct)
            wpos += 16;
        else
            put16w(w);
        return direct;
    }
    // The compression site: the oldest block, once it is whole.  direct: it is w (put_block); else w
    // is scratch.  w is consumed.
    BRB_DEV void pump(uint32_t (&w)[16], bool direct)
    {
        if (wpos - cpos >= 16) {
            if (!direct)
                load16(w);
            A::compress(st, w);
            cpos += 16;
        }
    }
    BRB_DEV void pump()
    {
        uint32_t w[16];
        pump(w, false);
    }

    // The piece of `len` bytes behind src (a range that starts nacc bytes early) in 64-byte blocks,
    // the next one in flight; a beat per block.  DIRECT: whole blocks take put_block.  LOWER: a piece
    // with `lower` set is taken as BRB_MD5UpdateLowerText takes it -- its blocks are lower-cased as
    // fetched, before head() puts the carried bytes in: those are the previous piece's and already
    // carry that piece's treatment.
    template <bool DIRECT, bool LOWER = false, class Beat>
    BRB_DEV void feed(brb_io::BlockSrc &src, uint64_t len, Beat &beat, bool lower = false)
    {
        const uint64_t n = len + nacc;
        for (uint64_t c = 0; c < n; c += 64) {
            uint32_t w[16];
            src.fetch(w);
            if (LOWER && lower)
                brb_io::lower16(w);
            if (c == 0)
                w[0] = head(w[0]);
            const uint64_t left = n - c;
            bool direct = false;
            if (left < 64)
                put_tail(w, uint32_t(left));
            else if (DIRECT)
                direct = put_block(w);
            else
                put16w(w);
            pump(w, direct);
            beat();
        }
        end_piece(n);
    }

    // The block buffer as it stands, fewer than 16 words pending: the pending words, the carried bytes,
    // zeros behind them.  Returns the bytes buffered (4 x pending + nacc).
    BRB_DEV uint32_t buffer(uint32_t (&w)[16]) const
    {
        const uint32_t r = wpos - cpos;
        load16(w);
#pragma unroll
        for (uint32_t i = 0; i < 16; i++)
            w[i] = i < r ? w[i] : i == r ? acc : 0u;
        return 4 * r + nacc;
    }
};

template <uint32_t RW = kRingWords>
using Md5Funnel = Funnel<Md5Words, RW>;

// BRB_MD5Final (md5.c:134-168) of a message of `total` bytes, as Md5Stream::final ends: the block
// buffer with the 0x80 marker, then md5_finish.  The marker's byte is the one after the carried
// bytes, so it joins the carry before buffer() places that word (brb_io::add_marker on the buffer
// is 48 more VALU per record, at the end of the line kernels' lone wave: about 0.6 us of 43 on
// bench --op metadata, seg_line 1; profiles/r14/funnel_ab.json).
template <uint32_t RW>
BRB_DEV Md5State md5_funnel_finish(Md5Funnel<RW> &f, uint64_t total)
{
    f.pump();                                           // fewer than 16 words pending
    f.acc |= 0x80u << (8 * f.nacc);
    uint32_t w[16];
    const uint32_t t = f.buffer(w);
    md5_finish(f.st, w, t, total);
    return f.st;
}

}  // namespace brb_funnel
