// seg_walk.h -- one lane's walk over a list of byte segments into its word funnel (word_funnel.h):
// the segments of a record (BRB_MD5BatchSegments, md5_seg_kernels.hip) or of a streaming context's
// item (BRB_MD5UpdateSegmentsBatch, digest_stream_kernels.hip).
//
// Segment k is read in 64-byte blocks (brb_io::BlockSrc, the next block in flight) as a range that
// starts e_k = (message bytes before it) mod 4 bytes early, so its words fall on the message's word
// boundaries (Funnel::head); those e bytes are the carried ones, never loaded from below the segment.
// The next non-empty segment's first block is in flight while the current one is hashed.  An empty
// segment is skipped without forming an address (its offset is loaded with its length, never used),
// with a beat per skipped one: a million-long run of empty ones outlasts a wave-pair partner's idle
// budget (pair_sync.h).
#pragma once

#include "pair_sync.h"
#include "word_funnel.h"

namespace brb_funnel {

struct SegWalk {
    const uint8_t *data;
    const uint64_t *soff;
    const uint32_t *slen;
    uint64_t k1;            // the list's end
    uint64_t k = 0;         // the segment in sa (k >= k1: none left)
    uint32_t la = 0;        // its length
    uint32_t before = 0;    // message bytes before it, mod 2^32 (only mod 4 matters)
    brb_io::BlockSrc sa;

    // the next segment with bytes at or after kk, its length and offset
    template <class Beat>
    BRB_DEV uint64_t find(uint64_t kk, uint32_t &len, uint64_t &off, Beat &beat) const
    {
        while (kk < k1) {
            len = slen[kk];
            off = soff[kk];
            if (len)
                break;
            kk++;
            beat();
        }
        return kk;
    }
    BRB_DEV void start(brb_io::BlockSrc &src, uint64_t off, uint32_t len, uint32_t pre) const
    {
        const uint8_t *a = data + off;
        const uint32_t e = pre & 3;
        src.init(a - e, uint64_t(len) + e, a);
    }

    // Finds the first segment with bytes at or after k0 and starts its first block; `pre`: the message
    // bytes before it (mod 4 is enough), known before the funnel is seeded.  False: the list has no byte.
    template <class Beat>
    BRB_DEV bool first(uint64_t k0, uint32_t pre, Beat &beat)
    {
        uint64_t oa = 0;
        before = pre;
        k = find(k0, la, oa, beat);
        if (k < k1)
            start(sa, oa, la, before);
        return k < k1;
    }

    // The rest of the walk, after first().  done(len) once per segment, after its bytes are in.
    // LOWER (BRB_MD5UpdateSegmentsLowerBatch): segment kk is taken as BRB_MD5UpdateLowerText
    // (Funnel::feed's `lower`) when slow[kk] != 0, every segment when slow is nullptr; the byte is read
    // once the segment is found, a segment ahead of its bytes like its first block.
    template <bool DIRECT, bool LOWER = false, class F, class Beat, class Done>
    BRB_DEV void run(F &f, Beat &beat, Done done, const uint8_t *slow = nullptr)
    {
        auto low = [&](uint64_t kk) { return LOWER && kk < k1 && (!slow || slow[kk] != 0); };
        brb_io::BlockSrc sb;
        uint32_t lb = 0;
        uint64_t oa = 0, ob = 0;
        bool wa = low(k);
        while (k < k1) {
            const uint64_t kb = find(k + 1, lb, ob, beat);
            const bool wb = low(kb);
            if (kb < k1)
                start(sb, ob, lb, before + la);
            f.template feed<DIRECT, LOWER>(sa, la, beat, wa);
            done(la);
            before += la;
            if (kb >= k1)
                break;
            k = find(kb + 1, la, oa, beat);             // sb's length is lb: la is free
            wa = low(k);
            if (k < k1)
                start(sa, oa, la, before + lb);
            f.template feed<DIRECT, LOWER>(sb, lb, beat, wb);
            done(lb);
            before += lb;
        }
    }
};

}  // namespace brb_funnel
