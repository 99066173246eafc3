// rc4_block.h -- the per-buffer bodies and the start-up of the RC4 kernels, shared by
// rc4_kernels.hip (one buffer per stream) and rc4_list_kernels.hip (a buffer list per stream).
// Everything here is force-inlined, takes values or references and holds no state.
#pragma once

#include "rc4_device.h"

namespace brb_rc4 {

BRB_DEV uint32_t clamp4(uint64_t left) { return left >= 4 ? 4u : uint32_t(left); }

// Wave-uniform maximum (loop bounds of the cooperative block loads).
BRB_DEV uint32_t wave_max(uint32_t x)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const uint32_t y = uint32_t(__shfl_xor(int(x), o));
        x = y > x ? y : x;
    }
    return __builtin_amdgcn_readfirstlane(x);
}

// BlockSrcW exchange per wave.  Only the plain RC4 pass loads cooperatively: 65 536 x 1500 B,
// 135 -> 124 us.  The frame and open kernels, whose MD5 work per block hides the per-lane loads,
// measured slower with it (frame 141 -> 150 us, open 139 -> 143 us, rocprofv3, tools/gpu_ab_prof.sh).
constexpr uint32_t kXchBytes = 4096;

// A lane's column of the LDS image in a kernel of kWaves waves (the pair kernels: lane * 4 + w4).
BRB_DEV uint32_t lane_word() { return (threadIdx.x & 63) * 4 + (threadIdx.x >> 6); }

// Start-up of a lane's generator, in two steps because kernels whose lanes past n help with the
// cooperative loads run only the second under `live`: its column `lw` of the LDS image `slot`; then
// the state of stream s, loaded (returns its address for the store).
BRB_DEV void gen_place(Gen &g, uint8_t *slot, uint32_t lw)
{
    g.P.lds = slot;
    g.P.lw = lw;
}

BRB_DEV uint8_t *gen_load(Gen &g, uint8_t *states, const uint32_t *sidx, uint64_t s)
{
    uint8_t *state = states + uint64_t(sidx ? sidx[s] : s) * kStateBytes;   // sidx: connection table
    g.load(state);
    return state;
}

// ---- per-buffer bodies: what a lone wave's lane does with one buffer between its generator's load
// and store.  The single-buffer kernels call one once, the list kernels once per buffer. -------------
// One buffer of the RC4 pass.  `nloop` blocks are fetched (per lane: the buffer's own count;
// cooperative loads: the wave's maximum, so every lane calls fetch the same number of times); blocks
// past `len` produce nothing.  The caller flushes the sink.
template <class SrcT, class SnkT>
BRB_DEV void crypt_blocks(SrcT &src, SnkT &snk, Gen &g, uint64_t len, uint32_t nloop)
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
        // the next block is taken (and the one after it requested) before this block's stores go
        // out, so the wait for it never includes them
        if (b + 1 < nloop)
            src.fetch(c);
        if (full)
            snk.put16(ks);
    }
}

// One frame (WRITE side): payload pl[0 .. len) -> the 30 + len bytes at `frame`.
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

// Frame block b (chunks 16b .. 16b + 15 of a frame of F bytes): fetched, decrypted into pt and the sink.
BRB_DEV void decrypt_block(brb_io::BlockSrc &src, Snk &snk, Gen &g, uint64_t F, uint64_t b, uint32_t (&pt)[16])
{
    uint32_t c[16];
    src.fetch(c);
    const uint64_t pos = 64 * b;
    if (pos + 64 <= F) {
        uint32_t ks[16];
        g.words(ks);
#pragma unroll
        for (int i = 0; i < 16; i++)
            pt[i] = c[i] ^ ks[i];
        snk.put16(pt);
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint64_t q = pos + 4 * i;
            pt[i] = 0;
            if (q < F) {
                pt[i] = c[i] ^ g.next_n(clamp4(F - q));
                snk.put(pt[i]);
            }
        }
    }
}

// One frame of F bytes (READ side + DataValidate): in -> out, returns valid.
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

}  // namespace brb_rc4
