// stream_funnel.h -- one lane's streaming digest over bytes that arrive in pieces at any message
// position, continued from a context and ended without padding (BRB_MD5UpdateBig / BrbSha1_Update
// per piece on a context that already holds bytes).
//
// md5_funnel.h's idea with three changes: the funnel is seeded from a context's state and buffered
// bytes instead of the IV, it is generic over the algorithm structs of digest_stream_kernels.hip
// (A::State, A::compress on 16 little-endian message words), and it ends by handing back the block
// buffer -- the pending words and the carried bytes -- instead of padding.
//
// As there: a carry holds the 0..3 message bytes left over from the previous piece; whole 32-bit
// message words go to the lane's private 32-word ring in LDS, word k of lane l at (k * 64 + l) * 4 --
// every access of lane l hits bank l.  The caller reads each piece from `nacc` bytes before it, so its
// words already fall on message word boundaries (head / put_block / put_tail); pump() compresses the
// oldest 16 once they are there and must run at least once per 16 words written, which keeps one
// compression site per caller loop.  A whole block that arrives with nothing pending is compressed
// from its registers and skips the ring (put_block).  The ring is private to its lane: no barrier,
// no cross-lane traffic, no wait on another wave.
#pragma once

#include "brb_gpu_common.h"

namespace brb_stream {

constexpr uint32_t kRingWords = 32;     // per lane: 8 KiB per wave, 32 KiB per 256-lane workgroup

template <class A>
struct Funnel {
    static constexpr uint32_t RW = kRingWords, kMask = RW * 256 - 1;
    uint32_t *bb;       // ring word k of this lane at bb[64 k] (LDS)
    uint32_t ring;      // LDS address of this wave's ring (RW * 256-byte aligned), OR'd into word addresses
    uint32_t lane4;     // 4 x lane: the lane's byte within a ring row
    typename A::State st;
    uint32_t acc;       // the carried bytes (low nacc bytes, zeros above)
    uint32_t nacc;      // bytes held in acc (0..3)
    uint32_t wpos;      // words written
    uint32_t cpos;      // words compressed (a multiple of 16)

    // lane_words = &ring[0][lane] of a [RW][64] uint32 array at an RW * 256-byte aligned LDS address.
    // The context's `have` buffered bytes (in: its block buffer) are the message so far: have >> 2
    // whole words in the ring, have & 3 bytes carried.  All 16 words are stored -- those from
    // have >> 2 on are overwritten before they are read.
    BRB_DEV void seed(uint32_t *lane_words, const typename A::State &s, const uint32_t (&in)[16], uint32_t have)
    {
        bb = lane_words;
        const uint32_t a = uint32_t(reinterpret_cast<uintptr_t>(lane_words));
        ring = a & ~kMask;
        lane4 = a & 0xFFu;
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

    // cpos is a multiple of 16, so the 16 words never wrap: one base, immediate offsets
    BRB_DEV void load16(uint32_t (&w)[16]) const
    {
        const uint32_t *b = bb + 64 * (cpos & (RW - 16));
#pragma unroll
        for (uint32_t i = 0; i < 16; i++)
            w[i] = b[64 * i];
    }

    BRB_DEV void pump()
    {
        if (wpos - cpos >= 16) {
            uint32_t w[16];
            load16(w);
            A::compress(st, w);
            cpos += 16;
        }
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
    // pump() for the caller's loop, still its one compression site; w is consumed
    BRB_DEV void pump(uint32_t (&w)[16], bool direct)
    {
        if (wpos - cpos >= 16) {
            if (!direct)
                load16(w);
            A::compress(st, w);
            cpos += 16;
        }
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

}  // namespace brb_stream
