// digest_stream_kernels.hip -- streaming MD5 / SHA-1 contexts as a batch: Init, Update, Final.
//
// The compat digests are streaming contexts (BRB_MD5Init / Update / Final, md5.c:38-168;
// BrbSha1_Init / Update / Final, sha1.c:132-195).  Here a table of such contexts lives in HBM and a
// call advances many of them by one piece each, bit-compatible with the compat structs: one context
// per lane, like every digest kernel of this library (a digest is a serial chain).
//
// Update, the hot path (message-grid split): with `have` bytes buffered the message
// continues as in[0 .. have) ++ piece.  The head block is assembled once per piece: the piece's first
// 64 - have bytes are read as a range that starts (have & 3) bytes early (BlockSrc::init's `lo`), so
// its bytes fall on the block's word boundaries, and its words are shifted up by have >> 2 words in
// registers (four select stages).  The body is a plain BlockSrc over piece + room, its first block in
// flight while the head is assembled and compressed: the loop of md5_any_kernel, started from the
// context's state and ended without padding.  The last partial block goes to the context's buffer.
//
// Segments: item i advances its context by a LIST of segments and is then, optionally,
// finalised -- Update, Final, the fused last piece and the whole-record segment digest in one kernel.
// The bytes go through the lane's word funnel (word_funnel.h), seeded from the context, along the shared
// segment walk (seg_walk.h).
#include "brb_kernels.h"
#include "byte_stream.h"
#include "md5_device.h"
#include "seg_walk.h"
#include "sha1_device.h"

namespace {

constexpr int kBlock = 256;

// W dwords from / to a 4-byte-aligned address: 16-byte vector accesses, then single dwords.
template <uint32_t W>
BRB_DEV void load_words(const uint8_t *p, uint32_t (&w)[W])
{
#pragma unroll
    for (uint32_t k = 0; k + 4 <= W; k += 4) {
        const uint4 v = ld16_a4(p + 4 * k);
        w[k] = v.x;
        w[k + 1] = v.y;
        w[k + 2] = v.z;
        w[k + 3] = v.w;
    }
#pragma unroll
    for (uint32_t k = W & ~3u; k < W; k++)
        w[k] = ld4_a4(p + 4 * k);
}

template <uint32_t W>
BRB_DEV void store_words(uint8_t *p, const uint32_t (&w)[W])
{
#pragma unroll
    for (uint32_t k = 0; k + 4 <= W; k += 4)
        st16_a4(p + 4 * k, w[k], w[k + 1], w[k + 2], w[k + 3]);
#pragma unroll
    for (uint32_t k = W & ~3u; k < W; k++)
        stg(reinterpret_cast<uint32_t *>(p + 4 * k), w[k]);
}

// A context is kHdr header words -- the state, then the two counters -- followed by the 64-byte block
// buffer; `h` below is the header as loaded.
struct Md5Stream : Md5Words {                       // BRB_MD5_CTX: buf[4], bytes[2], in[16], digest[16], string[64]
    static constexpr uint32_t kHdr = 6, kCtxBytes = 168;

    static BRB_DEV State state(const uint32_t (&h)[kHdr]) { return State{h[0], h[1], h[2], h[3]}; }
    static BRB_DEV void put_state(uint32_t (&h)[kHdr], const State &st)
    {
        h[0] = st.a;
        h[1] = st.b;
        h[2] = st.c;
        h[3] = st.d;
    }
    static BRB_DEV void init(uint32_t (&h)[kHdr])
    {
        put_state(h, md5_iv());
        h[4] = h[5] = 0;
    }
    static BRB_DEV uint32_t have(const uint32_t (&h)[kHdr]) { return h[4] & 63u; }
    // md5.c:78-81: a 32-bit byte count with a carry into bytes[1]
    static BRB_DEV void advance(uint32_t (&h)[kHdr], uint32_t len)
    {
        const uint32_t old = h[4];
        h[4] = old + len;
        h[5] += h[4] < old ? 1u : 0u;
    }
    // final() leaves bytes as they are in memory: a call that advanced them before it stores them
    static BRB_DEV void store_counts(uint8_t *cx, const uint32_t (&h)[kHdr])
    {
        stg(reinterpret_cast<uint32_t *>(cx + 16), h[4]);
        stg(reinterpret_cast<uint32_t *>(cx + 20), h[5]);
    }

    // w: the buffered bytes with the 0x80 marker, zeros behind it.  BRB_MD5Final (md5.c:134-168): buf,
    // digest and string[0 .. 33) are written, and in is left holding the last block it transformed (the
    // padded block, or 14 zero words and the bit count when the padding took a block of its own);
    // bytes and string[33 .. 64) are not written.
    static BRB_DEV void final(uint8_t *cx, uint32_t (&h)[kHdr], uint32_t (&w)[16], uint32_t t, uint8_t *digests, uint64_t i)
    {
        State st = state(h);
        md5_finish(st, w, t, uint64_t(h[4]) | (uint64_t(h[5]) << 32));
        st16_a4(cx, st.a, st.b, st.c, st.d);
        store_words(cx + 24, w);
        st16_a4(cx + 88, st.a, st.b, st.c, st.d);
        const uint32_t d[4] = {st.a, st.b, st.c, st.d};
        uint32_t hx[8];
#pragma unroll
        for (uint32_t j = 0; j < 8; j++)
            hx[j] = hex4(d[j >> 1] >> (16 * (j & 1)));
        store_words(cx + 104, hx);
        stg8(cx + 104 + 32, 0);
        if (digests) {
            const uint4 v = make_uint4(st.a, st.b, st.c, st.d);
            __builtin_memcpy(digests + 16 * i, &v, 16);
        }
    }
};

struct Sha1Stream {                                 // BrbSha1Ctx: state[5], count[2], buffer[64]
    using State = Sha1State;
    static constexpr uint32_t kHdr = 7, kCtxBytes = 92;

    static BRB_DEV State state(const uint32_t (&h)[kHdr]) { return State{h[0], h[1], h[2], h[3], h[4]}; }
    static BRB_DEV void put_state(uint32_t (&h)[kHdr], const State &st)
    {
        h[0] = st.a;
        h[1] = st.b;
        h[2] = st.c;
        h[3] = st.d;
        h[4] = st.e;
    }
    static BRB_DEV void init(uint32_t (&h)[kHdr])
    {
        put_state(h, sha1_iv());
        h[5] = h[6] = 0;
    }
    static BRB_DEV uint32_t have(const uint32_t (&h)[kHdr]) { return (h[5] >> 3) & 63u; }
    // sha1.c:151-153: count[0] += len << 3, compared against the UNTRUNCATED len << 3 (a spurious carry
    // for len >= 2^29), then count[1] += len >> 29
    static BRB_DEV void advance(uint32_t (&h)[kHdr], uint32_t len)
    {
        const uint64_t l3 = uint64_t(len) << 3;
        h[5] += uint32_t(l3);
        h[6] += uint64_t(h[5]) < l3 ? 1u : 0u;
        h[6] += len >> 29;
    }
    static BRB_DEV void compress(State &st, uint32_t (&w)[16])   // w: little-endian words; consumed
    {
#pragma unroll
        for (int k = 0; k < 16; k++)
            w[k] = __builtin_bswap32(w[k]);
        sha1_compress(st, w);
    }
    static BRB_DEV void store_counts(uint8_t *, const uint32_t (&)[kHdr]) {}   // final() zeroes the context

    // BrbSha1_Final (sha1.c:171-195): the bit count is the counter pair as it stands, big-endian; the
    // digest is the state's words big-endian; the whole context is wiped.
    static BRB_DEV void final(uint8_t *cx, uint32_t (&h)[kHdr], uint32_t (&w)[16], uint32_t t, uint8_t *digests, uint64_t i)
    {
        State st = state(h);
#pragma unroll
        for (int k = 0; k < 16; k++)
            w[k] = __builtin_bswap32(w[k]);
        if (t >= 56) {
            sha1_compress(st, w);
#pragma unroll
            for (int k = 0; k < 14; k++)
                w[k] = 0;
        }
        w[14] = h[6];
        w[15] = h[5];
        sha1_compress(st, w);
        const uint32_t v[5] = {__builtin_bswap32(st.a), __builtin_bswap32(st.b), __builtin_bswap32(st.c),
                               __builtin_bswap32(st.d), __builtin_bswap32(st.e)};
        __builtin_memcpy(digests + 20 * i, v, 20);
        const uint32_t zero[kCtxBytes / 4] = {};
        store_words(cx, zero);
    }
};

template <class A>
BRB_DEV uint8_t *ctx_of(uint8_t *ctxs, const uint32_t *__restrict__ ctx_index, uint64_t i)
{
    return ctxs + uint64_t(ctx_index ? ctx_index[i] : i) * A::kCtxBytes;
}

// The state words and the two counters, nothing else (BRB_MD5Init md5.c:38-47, BrbSha1_Init sha1.c:132-141).
template <class A>
__global__ __launch_bounds__(kBlock) void stream_init_kernel(uint8_t *ctxs, const uint32_t *__restrict__ ctx_index, uint64_t n)
{
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n)
        return;
    uint32_t h[A::kHdr];
    A::init(h);
    store_words(ctx_of<A>(ctxs, ctx_index, i), h);
}

template <class A>
__global__ __launch_bounds__(kBlock) void stream_update_kernel(uint8_t *ctxs, const uint32_t *__restrict__ ctx_index,
                                                               const uint8_t *__restrict__ data,
                                                               const uint64_t *__restrict__ offs,
                                                               const uint32_t *__restrict__ lens, uint64_t n)
{
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n)
        return;
    const uint32_t len = lens[i];
    if (len == 0)                                   // changes nothing; its offset need not be memory
        return;
    uint8_t *cx = ctx_of<A>(ctxs, ctx_index, i);
    const uint8_t *a = data + offs[i];
    // the context and the piece's first two blocks, all in flight together
    uint32_t h[A::kHdr], in[16];
    load_words(cx, h);
    load_words(cx + 4 * A::kHdr, in);
    const uint32_t have = A::have(h), room = 64 - have, e = have & 3, q = have >> 2;
    const uint32_t hl = len < room ? len : room;    // piece bytes of the head block
    brb_io::BlockSrc head, body;
    head.init(a - e, uint64_t(hl) + e, a);          // at most 64 bytes: one block
    const uint64_t blen = len - hl;
    body.init(a + hl, blen);                        // blen == 0: no load
    A::advance(h, len);

    // head block: words below q from the buffer, word q the buffer's e carried bytes under the piece's
    // first 4 - e, words above q the range's words shifted up by q
    uint32_t w[16];
    head.fetch(w);
    // A branch per stage.  Written as a select of w[k - s] and w[k], hipcc indexes the array by
    // (on ? s : 0) and lowers every word to a 15-deep select chain: 735 v_cndmask, 33 -> 28 us (§4.8).
#pragma unroll
    for (uint32_t s = 8; s >= 1; s >>= 1) {
        if (q & s) {
#pragma unroll
            for (uint32_t k = 15; k >= s; k--)
                w[k] = w[k - s];
        }
    }
    const uint32_t m = (1u << (8 * e)) - 1u;        // e = 0: no carried byte
#pragma unroll
    for (uint32_t k = 0; k < 16; k++)
        w[k] = k < q ? in[k] : k == q ? (in[k] & m) | (w[k] & ~m) : w[k];

    if (len >= room) {                              // the head block is whole
        typename A::State st = A::state(h);
        A::compress(st, w);
        const uint64_t nfull = blen >> 6;
        for (uint64_t b = 0; b < nfull; ++b) {
            body.fetch(w);
            A::compress(st, w);
        }
        body.fetch(w);                              // the tail, zeros behind it: the new buffer
        A::put_state(h, st);
    }
    uint32_t o[A::kHdr + 16];
#pragma unroll
    for (uint32_t k = 0; k < A::kHdr; k++)
        o[k] = h[k];
#pragma unroll
    for (uint32_t k = 0; k < 16; k++)
        o[A::kHdr + k] = w[k];
    store_words(cx, o);                             // the context, once
}

template <class A>
__global__ __launch_bounds__(kBlock) void stream_final_kernel(uint8_t *ctxs, const uint32_t *__restrict__ ctx_index, uint64_t n,
                                                              uint8_t *digests)
{
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n)
        return;
    uint8_t *cx = ctx_of<A>(ctxs, ctx_index, i);
    uint32_t h[A::kHdr], in[16], w[16];
    load_words(cx, h);
    load_words(cx + 4 * A::kHdr, in);
    const uint32_t t = A::have(h);
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {             // the t buffered bytes, zeros behind them
        const int32_t keep = int32_t(t) - int32_t(4 * k);
        w[k] = keep >= 4 ? in[k] : keep <= 0 ? 0u : in[k] & ((1u << (8 * uint32_t(keep))) - 1u);
    }
    brb_io::add_marker(w, t);
    A::final(cx, h, w, t, digests, i);
}

// Item i: the segments first[i] .. first[i + 1] - 1 into its context, in order, then Final when fin[i].
// The shared walk (seg_walk.h) on a funnel seeded from the context.  The counters advance once per segment.
// LOWER (BRB_MD5UpdateSegmentsLowerBatch): segment k is lower-cased on the way in when slow[k] != 0, every
// segment when slow is nullptr; without LOWER slow is not read.
template <class A, bool LOWER>
__global__ __launch_bounds__(kBlock) void stream_segments_kernel(uint8_t *ctxs, const uint32_t *__restrict__ ctx_index,
                                                                 const uint8_t *__restrict__ data,
                                                                 const uint64_t *__restrict__ soff,
                                                                 const uint32_t *__restrict__ slen,
                                                                 const uint64_t *__restrict__ first, uint64_t n,
                                                                 const uint8_t *__restrict__ fin, uint8_t *digests,
                                                                 const uint8_t *__restrict__ slow)
{
    __shared__ __attribute__((aligned(8192))) uint32_t ring[kBlock / 64][brb_funnel::kRingWords][64];   // 8 KiB per wave
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n)
        return;
    // The context is in flight while the lists are read, a segment's offset is loaded with its length, and
    // the first segment's first block is started from the header alone, before the buffer is seeded.
    const uint64_t k0 = first[i], k1 = first[i + 1];
    const bool last = fin && fin[i];
    uint8_t *cx = ctx_of<A>(ctxs, ctx_index, i);
    uint32_t h[A::kHdr], in[16];
    load_words(cx, h);
    load_words(cx + 4 * A::kHdr, in);
    brb_line::NoBeat beat;
    brb_funnel::SegWalk walk{data, soff, slen, k1};
    const uint32_t have = A::have(h);
    if (!walk.first(k0, have, beat) && !last)       // no bytes, no final: the context is not written
        return;
    brb_funnel::Funnel<A> f;
    f.seed(&ring[wave][0][lane], A::state(h), in, have);
    walk.template run<true, LOWER>(f, beat, [&](uint32_t len) { A::advance(h, len); }, slow);

    f.pump();                                       // fewer than 16 words pending
    uint32_t w[16];
    const uint32_t t = f.buffer(w);
    A::put_state(h, f.st);
    if (!last) {
        uint32_t o[A::kHdr + 16];
#pragma unroll
        for (uint32_t j = 0; j < A::kHdr; j++)
            o[j] = h[j];
#pragma unroll
        for (uint32_t j = 0; j < 16; j++)
            o[A::kHdr + j] = w[j];
        store_words(cx, o);                         // the context, once
        return;
    }
    A::store_counts(cx, h);
    brb_io::add_marker(w, t);
    A::final(cx, h, w, t, digests, i);              // as stream_final_kernel
}

inline unsigned grid_for(uint64_t n)
{
    return unsigned((n + kBlock - 1) / kBlock);
}

template <class A>
hipError_t launch_init(uint8_t *ctxs, const uint32_t *ctx_index, uint64_t n, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    stream_init_kernel<A><<<grid_for(n), kBlock, 0, s>>>(ctxs, ctx_index, n);
    return hipGetLastError();
}

template <class A>
hipError_t launch_update(uint8_t *ctxs, const uint32_t *ctx_index, const uint8_t *data, const uint64_t *offs,
                         const uint32_t *lens, uint64_t n, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    stream_update_kernel<A><<<grid_for(n), kBlock, 0, s>>>(ctxs, ctx_index, data, offs, lens, n);
    return hipGetLastError();
}

template <class A>
hipError_t launch_final(uint8_t *ctxs, const uint32_t *ctx_index, uint64_t n, uint8_t *digests, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    stream_final_kernel<A><<<grid_for(n), kBlock, 0, s>>>(ctxs, ctx_index, n, digests);
    return hipGetLastError();
}

template <class A>
hipError_t launch_segments(uint8_t *ctxs, const uint32_t *ctx_index, const uint8_t *data, const uint64_t *soff,
                           const uint32_t *slen, const uint64_t *first, uint64_t n, const uint8_t *fin, uint8_t *digests,
                           hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    stream_segments_kernel<A, false><<<grid_for(n), kBlock, 0, s>>>(ctxs, ctx_index, data, soff, slen, first, n, fin, digests,
                                                                    nullptr);
    return hipGetLastError();
}

}  // namespace

namespace brb {

hipError_t launch_digest_stream_init(bool sha1, uint8_t *ctxs, const uint32_t *ctx_index, uint64_t n, hipStream_t s)
{
    return sha1 ? launch_init<Sha1Stream>(ctxs, ctx_index, n, s) : launch_init<Md5Stream>(ctxs, ctx_index, n, s);
}

hipError_t launch_digest_stream_update(bool sha1, uint8_t *ctxs, const uint32_t *ctx_index, const uint8_t *data,
                                       const uint64_t *offs, const uint32_t *lens, uint64_t n, hipStream_t s)
{
    return sha1 ? launch_update<Sha1Stream>(ctxs, ctx_index, data, offs, lens, n, s)
                : launch_update<Md5Stream>(ctxs, ctx_index, data, offs, lens, n, s);
}

hipError_t launch_digest_stream_final(bool sha1, uint8_t *ctxs, const uint32_t *ctx_index, uint64_t n, uint8_t *digests,
                                      hipStream_t s)
{
    return sha1 ? launch_final<Sha1Stream>(ctxs, ctx_index, n, digests, s)
                : launch_final<Md5Stream>(ctxs, ctx_index, n, digests, s);
}

hipError_t launch_digest_stream_segments(bool sha1, uint8_t *ctxs, const uint32_t *ctx_index, const uint8_t *data,
                                         const uint64_t *soff, const uint32_t *slen, const uint64_t *first, uint64_t n,
                                         const uint8_t *fin, uint8_t *digests, hipStream_t s)
{
    return sha1 ? launch_segments<Sha1Stream>(ctxs, ctx_index, data, soff, slen, first, n, fin, digests, s)
                : launch_segments<Md5Stream>(ctxs, ctx_index, data, soff, slen, first, n, fin, digests, s);
}

hipError_t launch_md5_stream_segments_lower(uint8_t *ctxs, const uint32_t *ctx_index, const uint8_t *data,
                                            const uint64_t *soff, const uint32_t *slen, const uint8_t *slow,
                                            const uint64_t *first, uint64_t n, const uint8_t *fin, uint8_t *digests,
                                            hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    stream_segments_kernel<Md5Stream, true><<<grid_for(n), kBlock, 0, s>>>(ctxs, ctx_index, data, soff, slen, first, n, fin,
                                                                           digests, slow);
    return hipGetLastError();
}

}  // namespace brb
