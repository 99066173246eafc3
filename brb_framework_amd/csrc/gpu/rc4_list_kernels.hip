// rc4_list_kernels.hip -- RC4 and RC4+MD5 framing over a buffer list per stream.
//
// rc4_kernels.hip takes one buffer per stream and launch, so a connection that queued k buffers in a
// round costs k launches, each loading and storing its 264-byte state.  Here lane s loads
// states[sidx ? sidx[s] : s] once, walks buffers first[s] .. first[s + 1] - 1 in order and stores the
// state once.  The keystream generator (rc4_device.h Gen) is a pure step pipeline that advances by
// exactly the bytes returned and knows nothing of buffer ends, so a buffer boundary is only a fresh
// source, sink and (frame / open) MD5 state; every buffer is processed exactly as the single-buffer
// kernel processes its one buffer:
//
//   rc4_crypt_list_kernel    rc4_crypt_kernel<true> per buffer (whole-sector sink)
//   rc4md5_frame_list_kernel rc4md5_frame_kernel per buffer
//   rc4md5_open_list_kernel  rc4md5_open_kernel per buffer, valid[k] per buffer
//
// One lane per stream, kWaves waves per workgroup, the 64 KiB LDS permutation image of
// rc4_device.h.  These are lone-wave kernels: no partner wave, no wait on another wave, no atomics,
// so no protocol fault can occur.  A stream without buffers stores the state it loaded (the same
// 264 bytes: Gen::store drops the byte started ahead).  An empty buffer forms no address that is
// read or written (BlockSrc / BlockSrcW / Snk with n = 0).
#include "brb_kernels.h"
#include "rc4_block.h"
#include "rc4_device.h"
#include "test_options.h"

namespace {

using namespace brb_rc4;

constexpr int kWave = 64 * int(kWaves);   // threads per workgroup

// One buffer of the RC4 pass: the block loop of rc4_crypt_kernel.  `nloop` blocks are fetched (per
// lane: the buffer's own count; cooperative loads: the wave's maximum, so every lane calls fetch the
// same number of times); blocks past `len` produce nothing.
template <class SrcT>
BRB_DEV void crypt_blocks(SrcT &src, brb_io::SectorSnk &snk, Gen &g, uint64_t len, uint32_t nloop)
{
    uint32_t c[16];
    if (nloop)
        src.fetch(c);
    for (uint32_t b = 0; b < nloop; b++) {
        const uint64_t pos = 64ull * b;
        const bool full = pos + 64 <= len;
        uint32_t ks[16];
        if (full) {
            g.words(ks);
#pragma unroll
            for (int i = 0; i < 16; i++)
                ks[i] ^= c[i];
        } else if (pos < len) {
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const uint64_t q = pos + 4 * i;
                if (q < len)
                    snk.put(c[i] ^ g.next_n(clamp4(len - q)));
            }
        }
        // the next block is taken before this block's stores go out (rc4_crypt_kernel)
        if (b + 1 < nloop)
            src.fetch(c);
        if (full)
            snk.put16(ks);
    }
}

// COOP: the blocks are loaded cooperatively (brb_io::BlockSrcW).  The wave then walks buffer RANKS
// in uniform control flow: rank r of every lane at once, an empty range for a lane with fewer
// buffers, wave_max for the rank and block loops -- BlockSrcW's contract (all 64 lanes call init and
// fetch the same number of times; a lane with an empty range receives zero blocks).  !COOP: every
// lane walks its own list with its own BlockSrc, as the frame and open kernels do.
template <bool COOP>
__global__ __launch_bounds__(kWave) void rc4_crypt_list_kernel(uint8_t *__restrict__ states, const uint8_t *in, uint8_t *out,
                                                               const uint64_t *__restrict__ offs,
                                                               const uint32_t *__restrict__ lens,
                                                               const uint64_t *__restrict__ first, uint64_t n,
                                                               const uint32_t *__restrict__ sidx,
                                                               const uint64_t *__restrict__ ooffs)
{
    __shared__ __attribute__((aligned(16))) uint8_t slot[kSlotLds];
    __shared__ __attribute__((aligned(16))) uint8_t xch[COOP ? kWaves * kXchBytes : 16];
    __shared__ __attribute__((aligned(16))) uint8_t rows[kWave * brb_io::SectorSnk::kRowBytes];
    const uint64_t s = uint64_t(blockIdx.x) * kWave + threadIdx.x;
    const bool live = s < n;                     // COOP: lanes past n only help with the block loads
    if (!COOP && !live)
        return;
    Gen g;
    g.P.lds = slot;
    g.P.lw = (threadIdx.x & 63) * 4 + (threadIdx.x >> 6);
    uint8_t *state = nullptr;
    uint64_t k0 = 0, k1 = 0;
    if (live) {
        state = states + uint64_t(sidx ? sidx[s] : s) * kStateBytes;   // sidx: connection table
        g.load(state);
        k0 = first[s];
        k1 = first[s + 1];
    }
    const uint32_t row = uint32_t(reinterpret_cast<uintptr_t>(rows)) + threadIdx.x * brb_io::SectorSnk::kRowBytes;
    brb_io::SectorSnk snk;
    if constexpr (COOP) {
        const uint64_t cnt = k1 - k0;
        const uint32_t nrank = wave_max(cnt > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(cnt));
        for (uint32_t r = 0; r < nrank; r++) {
            const uint64_t k = k0 + r;
            uint64_t off = 0, len = 0, ooff = 0;
            if (k < k1) {
                off = offs[k];
                len = lens[k];
                ooff = ooffs ? ooffs[k] : off;
            }
            brb_io::BlockSrcW src;
            src.init(in + off, len, xch + (threadIdx.x >> 6) * kXchBytes);
            snk.init(out + ooff, len, row);
            crypt_blocks(src, snk, g, len, wave_max(uint32_t((len + 63) >> 6)));
            snk.flush();                         // nothing pending for an empty range
        }
    } else {
        for (uint64_t k = k0; k < k1; k++) {
            const uint64_t off = offs[k], len = lens[k];
            brb_io::BlockSrc src;
            src.init(in + off, len);
            snk.init(out + (ooffs ? ooffs[k] : off), len, row);
            crypt_blocks(src, snk, g, len, uint32_t((len + 63) >> 6));
            snk.flush();
        }
    }
    if (live)
        g.store(state);
}

// One frame: the body of rc4md5_frame_kernel between its g.load and g.store.
BRB_DEV void frame_buffer(Gen &g, const uint8_t *pl, uint64_t len, uint64_t salt, uint8_t *frame)
{
    const uint64_t F = kHeader + len;            // frame bytes

    // keystream of frame chunks 0..7 (bytes 0..31; chunk 7 = digest[15], NUL, payload[0..1])
    uint32_t kh[8];
#pragma unroll
    for (int k = 0; k < 7; k++)
        kh[k] = g.next4();
    kh[7] = g.next_n(clamp4(F - 28));

    brb_io::BlockSrc src;
    src.init(pl, len);
    Snk snk;                                      // frame bytes 32..F-1
    snk.init(frame + 32, F > 32 ? F - 32 : 0);
    Md5State st = md5_iv();
    const uint64_t nblk = md5_blocks(len), nw = 16 * nblk;
    uint32_t prev = 0, first = 0;
    for (uint64_t b = 0; b < nblk; b++) {
        uint32_t m[16], rw[16];
        src.fetch(rw);
        // frame chunks 16b + 7 .. 16b + 22 (payload words 16b .. 16b + 15; word 0 lives in the
        // header chunk 7): when all of them lie inside the frame, their keystream is one run
        if (4 * (16 * b + 23) <= F) {
            uint32_t ks[16];
            if (b == 0) {
                uint32_t k15[15];
                g.words(k15);
#pragma unroll
                for (int i = 0; i < 15; i++)
                    ks[i + 1] = k15[i];
                ks[0] = 0;
            } else {
                g.words(ks);
            }
            uint32_t ct[16];
#pragma unroll
            for (uint32_t i = 0; i < 16; i++) {
                const uint64_t w = 16 * b + i;
                const uint32_t raw = rw[i];
                if (w == 0)
                    first = raw;
                ct[i] = __builtin_amdgcn_alignbit(raw, prev, 16) ^ ks[i];
                prev = raw;
                m[i] = raw;
            }
            md5_pad_block(m, b, len, nw);
            if (b == 0) {
#pragma unroll
                for (int i = 1; i < 16; i++)
                    snk.put(ct[i]);
            } else {
                snk.put16(ct);
            }
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 16; i++) {
                const uint64_t w = 16 * b + i;
                const uint32_t raw = rw[i];
                if (w == 0) {
                    first = raw;
                } else {
                    // frame chunk w + 7 = payload bytes 4w - 2 .. 4w + 1
                    const uint64_t fb = 4 * (w + 7);
                    if (fb < F)
                        snk.put(__builtin_amdgcn_alignbit(raw, prev, 16) ^ g.next_n(clamp4(F - fb)));
                }
                prev = raw;
                m[i] = md5_pad_word(raw, w, len, nw);
            }
        }
        md5_compress(st, m);
    }
    snk.flush();

    // header: salt (LE unsigned long), "HASH:", digest, NUL, then payload[0..1] in chunk 7
    uint32_t h[8];
    h[0] = uint32_t(salt);
    h[1] = uint32_t(salt >> 32);
    h[2] = 0x48534148u;                           // "HASH"
    h[3] = 0x3Au | (st.a << 8);                   // ':' + digest[0..2]
    h[4] = __builtin_amdgcn_alignbit(st.b, st.a, 24);
    h[5] = __builtin_amdgcn_alignbit(st.c, st.b, 24);
    h[6] = __builtin_amdgcn_alignbit(st.d, st.c, 24);
    h[7] = (st.d >> 24) | (first << 16);          // digest[15], NUL, payload[0], payload[1]
    Snk hs;
    hs.init(frame, F < 32 ? F : 32);
#pragma unroll
    for (int k = 0; k < 8; k++)
        hs.put(h[k] ^ kh[k]);
    hs.flush();
}

__global__ __launch_bounds__(kWave) void rc4md5_frame_list_kernel(uint8_t *__restrict__ states,
                                                                  const uint8_t *__restrict__ payload,
                                                                  const uint64_t *__restrict__ offs,
                                                                  const uint32_t *__restrict__ lens,
                                                                  const uint64_t *__restrict__ salts, uint8_t *frames,
                                                                  const uint64_t *__restrict__ foffs,
                                                                  const uint64_t *__restrict__ first, uint64_t n,
                                                                  const uint32_t *__restrict__ sidx)
{
    __shared__ __attribute__((aligned(16))) uint8_t slot[kSlotLds];
    const uint64_t s = uint64_t(blockIdx.x) * kWave + threadIdx.x;
    if (s >= n)
        return;
    Gen g;
    g.P.lds = slot;
    g.P.lw = (threadIdx.x & 63) * 4 + (threadIdx.x >> 6);
    uint8_t *state = states + uint64_t(sidx ? sidx[s] : s) * kStateBytes;   // sidx: connection table
    g.load(state);
    const uint64_t k1 = first[s + 1];
    for (uint64_t k = first[s]; k < k1; k++)
        frame_buffer(g, payload + offs[k], lens[k], salts[k], frames + foffs[k]);
    g.store(state);
}

// One frame of F bytes: the body of rc4md5_open_kernel between its g.load and g.store; returns valid.
BRB_DEV uint32_t open_buffer(Gen &g, const uint8_t *in, uint8_t *out, uint64_t F)
{
    brb_io::BlockSrc src;
    Snk snk;
    src.init(in, F);
    snk.init(out, F);

    // frame block 0 = chunks 0..15; the header is chunks 0..7 (frame bytes 0..31)
    uint32_t cur[16];
    decrypt_block(src, snk, g, F, 0, cur);
    uint32_t ok = 0;
    if (F >= kHeader) {
        // payload word w = frame bytes 30 + 4w .. 33 + 4w: the high half of chunk w + 7 and the low
        // half of chunk w + 8; MD5 block b needs chunks 16b + 7 .. 16b + 23 = frame blocks b, b + 1
        const uint64_t len = F - kHeader;
        const uint64_t nblk = md5_blocks(len), nw = 16 * nblk;
        const uint32_t h2 = cur[2], h3 = cur[3], h4 = cur[4], h5 = cur[5], h6 = cur[6], h7 = cur[7];
        Md5State st = md5_iv();
        for (uint64_t b = 0; b < nblk; b++) {
            uint32_t nxt[16], m[16];
            decrypt_block(src, snk, g, F, b + 1, nxt);
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const uint32_t lo = i + 7 < 16 ? cur[i + 7] : nxt[i - 9];
                const uint32_t hi = i + 8 < 16 ? cur[i + 8] : nxt[i - 8];
                m[i] = __builtin_amdgcn_alignbit(hi, lo, 16);
            }
            md5_pad_block(m, b, len, nw);
            md5_compress(st, m);
#pragma unroll
            for (int i = 0; i < 16; i++)
                cur[i] = nxt[i];
        }
        const bool tag = h2 == 0x48534148u && (h3 & 0xFFu) == 0x3Au;   // "HASH:" at 8..12
        const bool dig = __builtin_amdgcn_alignbit(h4, h3, 8) == st.a && __builtin_amdgcn_alignbit(h5, h4, 8) == st.b &&
                         __builtin_amdgcn_alignbit(h6, h5, 8) == st.c && __builtin_amdgcn_alignbit(h7, h6, 8) == st.d;
        ok = tag && dig;
    }
    snk.flush();
    return ok;
}

__global__ __launch_bounds__(kWave) void rc4md5_open_list_kernel(uint8_t *__restrict__ states, const uint8_t *in, uint8_t *out,
                                                                 const uint64_t *__restrict__ offs,
                                                                 const uint32_t *__restrict__ lens,
                                                                 const uint64_t *__restrict__ first, uint64_t n,
                                                                 uint8_t *__restrict__ valid,
                                                                 const uint32_t *__restrict__ sidx,
                                                                 const uint64_t *__restrict__ ooffs)
{
    __shared__ __attribute__((aligned(16))) uint8_t slot[kSlotLds];
    const uint64_t s = uint64_t(blockIdx.x) * kWave + threadIdx.x;
    if (s >= n)
        return;
    Gen g;
    g.P.lds = slot;
    g.P.lw = (threadIdx.x & 63) * 4 + (threadIdx.x >> 6);
    uint8_t *state = states + uint64_t(sidx ? sidx[s] : s) * kStateBytes;   // sidx: connection table
    g.load(state);
    const uint64_t k1 = first[s + 1];
    for (uint64_t k = first[s]; k < k1; k++) {
        const uint64_t off = offs[k];
        valid[k] = uint8_t(open_buffer(g, in + off, out + (ooffs ? ooffs[k] : off), lens[k]));
    }
    g.store(state);
}

inline unsigned grid_for(uint64_t n) { return unsigned((n + kWave - 1) / kWave); }

}  // namespace

namespace brb {

hipError_t launch_rc4_crypt_list(uint8_t *states, const uint8_t *in, uint8_t *out, const uint64_t *offs,
                                 const uint32_t *lens, const uint64_t *first, uint64_t n, hipStream_t s,
                                 const uint32_t *sidx, const uint64_t *ooffs)
{
    if (n == 0)
        return hipSuccess;
    // cooperative block loads unless test option "rc4_list_coop" = 0 (16 384 x k x 1500 B, tools/conn_list_ab.py:
    // k = 2 216.3 -> 213.3 us, k = 4 528.8 -> 522.1 us, k = 8 804.4 -> 784.0 us; k = 1 within the spread)
    if (brb_opt::get(brb_opt::kRc4ListCoop) != 0)
        rc4_crypt_list_kernel<true><<<grid_for(n), kWave, 0, s>>>(states, in, out, offs, lens, first, n, sidx, ooffs);
    else
        rc4_crypt_list_kernel<false><<<grid_for(n), kWave, 0, s>>>(states, in, out, offs, lens, first, n, sidx, ooffs);
    return hipGetLastError();
}

hipError_t launch_rc4md5_frame_list(uint8_t *states, const uint8_t *payload, const uint64_t *offs, const uint32_t *lens,
                                    const uint64_t *salts, uint8_t *frames, const uint64_t *foffs,
                                    const uint64_t *first, uint64_t n, hipStream_t s, const uint32_t *sidx)
{
    if (n == 0)
        return hipSuccess;
    rc4md5_frame_list_kernel<<<grid_for(n), kWave, 0, s>>>(states, payload, offs, lens, salts, frames, foffs, first, n, sidx);
    return hipGetLastError();
}

hipError_t launch_rc4md5_open_list(uint8_t *states, const uint8_t *in, uint8_t *out, const uint64_t *offs,
                                   const uint32_t *lens, const uint64_t *first, uint64_t n, uint8_t *valid,
                                   hipStream_t s, const uint32_t *sidx, const uint64_t *ooffs)
{
    if (n == 0)
        return hipSuccess;
    rc4md5_open_list_kernel<<<grid_for(n), kWave, 0, s>>>(states, in, out, offs, lens, first, n, valid, sidx, ooffs);
    return hipGetLastError();
}

}  // namespace brb
