// metadata_pack_kernels.hip -- MetaDataPack of whole packs in one pass.
//
// MetaDataPack (libbrb_core/data/utils/meta_data.c:104-140) writes a 64-byte header, then per item
// {item_id, item_sub_id, sz; sz data bytes; 0x1F}; the header's digest (MetaDataHeaderLoadData,
// :397-433) is BRB_MD5Init, one BRB_MD5UpdateBig per item, BRB_MD5Final.  Batched: one pack per lane.
// A lane walks its items as the segment walk (seg_walk.h) does -- 64-byte blocks through
// brb_io::BlockSrc, the next block in flight, the next non-empty item's first block in flight while
// the current one is hashed -- and every block it fetches has two consumers: the lane's MD5 funnel
// (word_funnel.h) and the pack's byte stream (PackSnk below).  So every item byte is loaded from HBM
// once.  The header goes out last, once the digest is known, through a brb_io::Snk (its start has any
// alignment, and the pack before it may end in the same dword).
//
// The two streams sit at different byte phases: item data begins at digest position `before` and at
// body position 25 k + before + 24.  The blocks arrive on the digest's word boundaries (the item is
// read from e = before mod 4 bytes early, Funnel::head), so the sink re-phases each block by a shift
// that is constant over an item: one v_perm_b32 per dword, the selector idiom of Snk::put16.
//
// The lane's loop handles one PIECE of at most 64 bytes per iteration: an item's 24 header bytes or
// one of its data blocks.  Both kinds go through the same PackSnk::append, and only data blocks go on
// to the funnel, so the loop has one sink site and one compress site whatever the lanes of a wave are
// doing (their item counts and lengths differ: nothing here assumes uniform control flow).
#include "brb_kernels.h"
#include "byte_stream.h"
#include "word_funnel.h"

namespace {

constexpr int kBlock = 64;      // one wave per workgroup: 17 KiB of LDS, 9 workgroups per CU

// The pack body as a byte stream written in whole, aligned 64-byte memory sectors, after
// brb_io::SectorSnk: memory-aligned dwords go to the lane's 144-byte LDS row -- two sectors, circular
// by absolute dword index -- and a sector is read back (four ds_read_b128) and stored (four aligned
// 16-byte stores) when its last dword arrives.  SectorSnk itself does not fit: its row addresses are
// fixed for blocks of 16 chunks counted from the stream's start, and a pack body mixes 24-byte item
// headers, data blocks cut at any byte and 1-byte canaries.  Here every piece is appended at byte
// granularity, and all of them -- headers and canaries too -- leave in whole sectors.  The stream's
// first dword, if the body starts inside it, is stored byte by byte; its first sector, if the body
// starts inside it, dword by dword; so are the dwords and bytes left at the end (finish).  Nothing
// outside the stream is written, and no dword holding a foreign byte is written whole.
struct PackSnk {
    static constexpr uint32_t kRowBytes = brb_io::SectorSnk::kRowBytes;
    uint32_t *p;       // the dword holding the stream's next byte
    uint32_t o;        // bytes of that dword before the next byte (0..3)
    uint32_t carry;    // the stream's bytes among them (positions fb..o-1), other bytes 0
    uint32_t fb;       // first byte of the dword at p that is the stream's: non-zero only in its first dword
    uint32_t lowd;     // index, in the sector of p, of the first dword that is in the row (0..16)
    uint32_t rowb;     // LDS address of the lane's row (16-byte aligned)

    BRB_DEV void init(uint8_t *a, uint32_t row)
    {
        const uintptr_t ad = reinterpret_cast<uintptr_t>(a);
        p = reinterpret_cast<uint32_t *>(ad & ~uintptr_t(3));
        o = fb = uint32_t(ad & 3);
        carry = 0;
        lowd = uint32_t(ad >> 2) & 15;
        rowb = row;
    }

    static BRB_DEV uint32_t lds_ld(uint32_t a) { return brb_io::SectorSnk::lds_ld(a); }
    static BRB_DEV void lds_st(uint32_t a, uint32_t v) { brb_io::SectorSnk::lds_st(a, v); }
    BRB_DEV uint32_t udw() const { return uint32_t(reinterpret_cast<uintptr_t>(p) >> 2); }   // absolute dword index

    // the sector at `sec`, complete in the row half at `half` from dword lowd on
    BRB_DEV void flush_sector(uint32_t *sec, uint32_t half)
    {
        if (lowd == 0) {
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) {
                typedef uint32_t v4u __attribute__((ext_vector_type(4)));
                const v4u x = *reinterpret_cast<const __attribute__((address_space(3))) v4u *>(half + 16 * q);
                st16_a4(reinterpret_cast<uint8_t *>(sec + 4 * q), x.x, x.y, x.z, x.w);
            }
        } else {
#pragma unroll
            for (uint32_t i = 1; i < 16; i++)
                if (i >= lowd)
                    stg(sec + i, lds_ld(half + 4 * i));
        }
        lowd = 0;
    }

    // Appends bytes lo .. hi-1 of the 64-byte block w (lo <= 3, lo < hi <= 64; bytes from hi on are 0
    // or anything).  With s = (o - lo) mod 4, y_j = {w_j : w_{j-1}} shifted left by s bytes holds block
    // bytes 4 j - s .. 4 j - s + 3: for o >= lo the stream's dword j from p on is y_j, for o < lo it is
    // y_{j+1}.  All of them go to the row (those past the piece's end are overwritten by the next
    // piece), the position moves by hi - lo bytes, and the sector that completes, if one does, is stored.
    BRB_DEV void append(const uint32_t (&w)[16], uint32_t lo, uint32_t hi)
    {
        const uint32_t nb = hi - lo;
        const uint32_t neg = o < lo ? 1u : 0u;
        const uint32_t s = (o - lo) & 3;
        const uint32_t sel = 0x07060504u - 0x01010101u * s;    // as Snk::put16
        uint32_t y[17];
        uint32_t prev = 0;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            y[j] = __builtin_amdgcn_perm(w[j], prev, sel);
            prev = w[j];
        }
        y[16] = __builtin_amdgcn_perm(0u, prev, sel);
        const uint32_t m = (1u << (8 * o)) - 1u;               // the bytes before the next one: the carried ones
        if (neg)
            y[1] = (y[1] & ~m) | carry;
        else
            y[0] = (y[0] & ~m) | carry;
        const uint32_t u = udw();
        const uint32_t b = (u - neg) & 31;                     // y_j goes to row position (b + j) mod 32
        const uint32_t a0 = rowb + 4 * b, a1 = a0 - 128, jw = 32 - b;
        if (!neg)
            lds_st(a0, y[0]);
#pragma unroll
        for (uint32_t j = 1; j < 17; j++)
            lds_st((j < jw ? a0 : a1) + 4 * j, y[j]);
        const uint32_t nd = (o + nb) >> 2, on = (o + nb) & 3;  // dwords completed, bytes of the next one
        if (fb && nd) {                                        // the stream's first dword: its bytes only
            const uint32_t first = neg ? y[1] : y[0];
            uint8_t *q = reinterpret_cast<uint8_t *>(p);
            for (uint32_t k = fb; k < 4; k++)
                stg8(q + k, first >> (8 * k));
            lowd = (u & 15) + 1;
            fb = 0;
        }
        const uint32_t d = u & 15;
        if (d + nd >= 16)
            flush_sector(p - d, rowb + 64 * ((u >> 4) & 1));
        if (nb == 64)                                          // lo = 0, s = o: the block's last o bytes
            carry = o ? w[15] >> (32 - 8 * o) : 0u;
        else
            carry = on ? lds_ld(rowb + 4 * ((u + nd) & 31)) & ((1u << (8 * on)) - 1u) : 0u;
        p += nd;
        o = on;
    }

    // one byte, past the stream's first dword (the canary: at least an item header precedes it)
    BRB_DEV void put_byte(uint32_t v)
    {
        carry |= v << (8 * o);
        if (++o == 4) {
            const uint32_t u = udw();
            lds_st(rowb + 4 * (u & 31), carry);
            if ((u & 15) == 15)
                flush_sector(p - 15, rowb + 64 * ((u >> 4) & 1));
            ++p;
            o = 0;
            carry = 0;
        }
    }

    // the dwords still only in the row, then the bytes of the last, partial dword
    BRB_DEV void finish()
    {
        const uint32_t u = udw(), d = u & 15;
        const uint32_t half = rowb + 64 * ((u >> 4) & 1);
        uint32_t *sec = p - d;
#pragma unroll
        for (uint32_t i = 0; i < 15; i++)
            if (i >= lowd && i < d)
                stg(sec + i, lds_ld(half + 4 * i));
        uint8_t *q = reinterpret_cast<uint8_t *>(p);
        for (uint32_t k = fb; k < o; k++)
            stg8(q + k, carry >> (8 * k));
    }
};

__global__ __launch_bounds__(kBlock) void metadata_pack_kernel(const uint8_t *__restrict__ data,
                                                               const uint64_t *__restrict__ ioff,
                                                               const uint32_t *__restrict__ ilen,
                                                               const uint64_t *__restrict__ iid,
                                                               const uint64_t *__restrict__ isub,
                                                               const uint64_t *__restrict__ first, uint64_t n_packs,
                                                               uint8_t *out, const uint64_t *__restrict__ ooff)
{
    __shared__ __attribute__((aligned(8192))) uint32_t blk[kBlock / 64][brb_funnel::kRingWords][64];   // 8 KiB per wave
    __shared__ __attribute__((aligned(16))) uint8_t rows[kBlock * PackSnk::kRowBytes];              // 9 KiB per wave
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t r = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (r >= n_packs)
        return;
    const uint64_t k0 = first[r], k1 = first[r + 1];
    uint64_t size = 0;                                  // MetaDataHeader.size: the body's bytes so far
    uint64_t total = 0;                                 // bytes digested
    uint8_t *pack = out + ooff[r];
    brb_funnel::Md5Funnel<> f;
    f.init(&blk[wave][0][lane]);
    PackSnk snk;
    snk.init(pack + BRB_METADATA_HEADER_SIZE,
             uint32_t(reinterpret_cast<uintptr_t>(rows)) + threadIdx.x * PackSnk::kRowBytes);

    auto next_full = [&](uint64_t kk) {                 // the next item with bytes (an empty one's
        while (kk < k1 && ilen[kk] == 0)                // address need not be memory)
            kk++;
        return kk;
    };
    auto start = [&](brb_io::BlockSrc &src, uint64_t kk, uint64_t pre) {   // as SegWalk's
        const uint64_t len = ilen[kk];
        const uint8_t *a = data + ioff[kk];
        const uint32_t e = uint32_t(pre & 3);
        src.init(a - e, len + e, a);
        return len;
    };
    brb_io::BlockSrc sa, sb;
    uint64_t k = k0;                                    // the item whose piece comes next
    uint64_t kn = next_full(k0), len_n = 0;             // the next non-empty item, its blocks in flight
    bool next_b = false;                                //   ... in sb (else sa)
    if (kn < k1)
        len_n = start(sa, kn, 0);
    uint64_t before = 0;                                // digest bytes before item k
    uint64_t len = 0, n = 0, c = 0;                     // item k: its bytes, with the e early ones, and those done
    bool cur_b = false;
    for (;;) {
        uint32_t w[16];
        uint32_t lo = 0, hi = BRB_METADATA_ITEM_RAW_SIZE;
        const bool body = c < n;
        if (body) {                                     // a data block of item k
            if (cur_b)
                sb.fetch(w);
            else
                sa.fetch(w);
            lo = c ? 0u : f.nacc;
            hi = n - c < 64 ? uint32_t(n - c) : 64u;
        } else {                                        // item k's header
            if (k >= k1)
                break;
            const uint64_t id = iid[k], sub = isub[k];
            len = k == kn ? len_n : 0;
#pragma unroll
            for (int i = 0; i < 16; i++)
                w[i] = 0;
            w[0] = uint32_t(id);
            w[1] = uint32_t(id >> 32);
            w[2] = uint32_t(sub);
            w[3] = uint32_t(sub >> 32);
            w[4] = uint32_t(len);
            if (k == kn) {                              // its blocks follow; the next item's first goes in flight
                cur_b = next_b;
                n = len + f.nacc;
                kn = next_full(k + 1);
                next_b = !next_b;
                if (kn < k1)
                    len_n = next_b ? start(sb, kn, before + len) : start(sa, kn, before + len);
            }
        }
        snk.append(w, lo, hi);
        if (body) {
            if (c == 0)
                w[0] = f.head(w[0]);
            if (hi == 64)
                f.put16w(w);
            else
                f.put_tail(w, hi);
            f.pump();
            c += 64;
        }
        if (c >= n) {                                   // item k's last piece: its canary
            if (n) {
                f.end_piece(n);
                total += len;
                before += len;
            }
            snk.put_byte(0x1F);
            size += len + BRB_METADATA_ITEM_RAW_SIZE + 1;
            k++;
            n = c = 0;
        }
    }
    snk.finish();
    const Md5State st = brb_funnel::md5_funnel_finish(f, total);
    const uint32_t hw[16] = {0u, uint32_t(k1 - k0), uint32_t(size), uint32_t(size >> 32),
                             0x5F425242u, 0x4154454Du,   // "BRB_META"
                             st.a, st.b, st.c, st.d, 0u, 0u, 0u, 0u, 0u, 0u};
    brb_io::Snk h;
    h.init(pack, BRB_METADATA_HEADER_SIZE);
#pragma unroll
    for (int i = 0; i < 16; i++)
        h.put(hw[i]);
    h.flush();
}

}  // namespace

namespace brb {

hipError_t launch_metadata_pack(const uint8_t *data, const uint64_t *ioff, const uint32_t *ilen, const uint64_t *iid,
                                const uint64_t *isub, const uint64_t *first, uint64_t n_packs, uint8_t *out,
                                const uint64_t *ooff, hipStream_t s)
{
    if (n_packs == 0)
        return hipSuccess;
    metadata_pack_kernel<<<unsigned((n_packs + kBlock - 1) / kBlock), kBlock, 0, s>>>(data, ioff, ilen, iid, isub, first,
                                                                                      n_packs, out, ooff);
    return hipGetLastError();
}

}  // namespace brb
