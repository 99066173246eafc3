// b64_piece.h -- the per-lane pieces of the base64 group kernels (base64_kernels.hip): the 12 / 16-byte
// piece loads and stores at any address, one piece's encode and decode, and the serial decode that
// finishes a record from its first skipped byte on.  They stand in a header of their own so that
// tests/c/lane_io_check.cpp can run them on the host, one lane at a time, under ASan + UBSan.
#pragma once

#include "byte_stream.h"

namespace brb_b64 {

BRB_DEV uint32_t alpha(uint32_t i)   // base64.c:42
{
    return i < 26 ? 'A' + i : i < 52 ? 'a' + (i - 26) : i < 62 ? '0' + (i - 52) : i == 62 ? '+' : '/';
}

// big-endian 24-bit quantum q (0..3) of the 12 bytes d0|d1|d2 (v_perm selectors: 0-3 = src1 bytes,
// 4-7 = src0 bytes, 0x0C = 0)
BRB_DEV uint32_t quantum(uint32_t d0, uint32_t d1, uint32_t d2, int q)
{
    switch (q) {
    case 0: return __builtin_amdgcn_perm(d0, d0, 0x0C000102u);
    case 1: return __builtin_amdgcn_perm(d1, d0, 0x0C030405u);
    case 2: return __builtin_amdgcn_perm(d2, d1, 0x0C020304u);
    default: return __builtin_amdgcn_perm(d2, d2, 0x0C010203u);
    }
}

// the 4 characters of quantum v: two lookups of 12 bits each
BRB_DEV uint32_t chars4(const uint16_t *pair, uint32_t v)
{
    return uint32_t(pair[v >> 12]) | (uint32_t(pair[v & 4095u]) << 16);
}

// base64.c:363-376: alphabet value, 0 for '=', -1 for anything else (NUL included)
BRB_DEV int b64_value(uint32_t c)
{
    if (c - 'A' < 26u)
        return int(c - 'A');
    if (c - 'a' < 26u)
        return int(c - 'a' + 26);
    if (c - '0' < 10u)
        return int(c - '0' + 52);
    if (c == '+')
        return 62;
    if (c == '/')
        return 63;
    return c == '=' ? 0 : -1;
}

// 4 characters (one dword) -> their 3 bytes in output order (b0 | b1 << 8 | b2 << 16), bit 31 set
// if any character is outside the alphabet / '=' (256-byte table: one dword per LDS bank)
BRB_DEV uint32_t group3(const int8_t *val, uint32_t ch)
{
    const int v0 = val[ch & 255u], v1 = val[(ch >> 8) & 255u], v2 = val[(ch >> 16) & 255u], v3 = val[ch >> 24];
    const uint32_t w = (uint32_t(v0) << 18) | (uint32_t(v1) << 12) | (uint32_t(v2) << 6) | uint32_t(v3 & 63);
    const uint32_t s = __builtin_amdgcn_perm(w, w, 0x0C000102u);   // bytes w2 w1 w0 -> output order
    return s | (uint32_t(v0 | v1 | v2 | v3) & 0x80000000u);
}

// bytes [a, a + m) (m <= 16) as 4 little-endian dwords, zeros past m.  Reads only dwords that hold
// a byte of the range (so never past the end of a buffer); one 16-byte load when aligned and whole.
BRB_DEV void load_piece(const uint8_t *a, uint32_t m, uint32_t (&d)[4])
{
    const uintptr_t ad = reinterpret_cast<uintptr_t>(a);
    const uint32_t s = uint32_t(ad & 3);
    if (s == 0 && m == 16) {
        const uint4 v = ld16_a4(a);
        d[0] = v.x;
        d[1] = v.y;
        d[2] = v.z;
        d[3] = v.w;
        return;
    }
    const uint8_t *a0 = a - s;
    uint32_t w[5];
#pragma unroll
    for (int k = 0; k < 5; k++)
        w[k] = m && 4u * k < s + m ? ld4_a4(a0 + 4 * k) : 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t v = funnel(w[k + 1], w[k], 8 * s);
        const uint32_t lo = 4u * k;
        d[k] = m >= lo + 4 ? v : m > lo ? v & (0xFFFFFFFFu >> (32 - 8 * (m - lo))) : 0u;
    }
}

// 12 bytes [a, a + 12), 4-byte aligned: three dword loads the compiler merges into one dwordx3
BRB_DEV void load12_a4(const uint8_t *a, uint32_t (&d)[4])
{
    d[0] = ld4_a4(a);
    d[1] = ld4_a4(a + 4);
    d[2] = ld4_a4(a + 8);
    d[3] = 0;
}

// the q (<= 16) bytes of v -> [o, o + q), writing no byte outside it: aligned dwords that the range
// covers whole go out as dword (or one 16-byte) stores, the partial dwords at its ends byte by byte
BRB_DEV void store_piece(uint8_t *o, uint32_t q, const uint32_t (&v)[4])
{
    const uintptr_t ad = reinterpret_cast<uintptr_t>(o);
    const uint32_t s = uint32_t(ad & 3);
    if (s == 0 && q == 16) {
        st16_a4(o, v[0], v[1], v[2], v[3]);
        return;
    }
    if (s == 0 && q == 12) {
        stg(reinterpret_cast<uint32_t *>(o), v[0]);
        stg(reinterpret_cast<uint32_t *>(o + 4), v[1]);
        stg(reinterpret_cast<uint32_t *>(o + 8), v[2]);
        return;
    }
    uint8_t *a0 = o - s;
    // aligned dword k holds range bytes 4k - s .. 4k - s + 3: byte b = byte 4 + b - s of {v_k : v_k-1}
    const uint32_t sel = 0x07060504u - 0x01010101u * s;
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const uint32_t first = 4u * k;                       // position of the dword in [a0, ...)
        if (first >= s + q)
            break;
        const uint32_t w = __builtin_amdgcn_perm(k < 4 ? v[k] : 0u, k > 0 ? v[k - 1] : 0u, sel);
        const uint32_t lo = first < s ? s - first : 0u;      // 0, or s in dword 0
        const uint32_t end = s + q - first;                  // bytes of this dword before the end
        const uint32_t hi = end >= 4 ? 3u : end - 1;
        if (lo == 0 && hi == 3) {
            stg(reinterpret_cast<uint32_t *>(a0 + first), w);
        } else {
#pragma unroll
            for (uint32_t b = 0; b < 4; b++)
                if (b >= lo && b <= hi)
                    stg8(a0 + first + b, w >> (8 * b));
        }
    }
}

// one encode piece: m (1..12) input bytes in d[0..2] (zeros past m) -> 4 * ceil(m / 3) characters
BRB_DEV uint32_t encode_piece(const uint16_t *pair, const uint32_t (&d)[4], uint32_t m, uint32_t (&c)[4])
{
#pragma unroll
    for (int q = 0; q < 4; q++)
        c[q] = chars4(pair, quantum(d[0], d[1], d[2], q));
    if (m < 12) {                                             // the record's last piece
        const uint32_t nq = (m + 2) / 3, rest = m % 3;        // base64.c:335-352 padding
        if (rest) {
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (uint32_t(q) == nq - 1)
                    c[q] = rest == 1 ? (c[q] & 0x0000FFFFu) | 0x3D3D0000u : (c[q] & 0x00FFFFFFu) | 0x3D000000u;
        }
        return 4 * nq;
    }
    return 16;
}

// one decode piece: the 16 characters in d; returns the flags of its first `groups` groups (bit 31
// set: a character outside the alphabet / '=' among them) and the 12 bytes in b[0..2]
BRB_DEV uint32_t decode_piece(const int8_t *val, const uint32_t (&d)[4], uint32_t groups, uint32_t (&b)[4])
{
    const uint32_t s0 = group3(val, d[0]), s1 = group3(val, d[1]), s2 = group3(val, d[2]), s3 = group3(val, d[3]);
    b[0] = (s0 & 0xFFFFFFu) | (s1 << 24);
    b[1] = ((s1 & 0xFFFFFFu) >> 8) | (s2 << 16);
    b[2] = ((s2 & 0xFFFFFFu) >> 16) | (s3 << 8);
    b[3] = 0;
    const uint32_t f = (s0 & (groups > 0 ? 0x80000000u : 0u)) | (s1 & (groups > 1 ? 0x80000000u : 0u)) |
                       (s2 & (groups > 2 ? 0x80000000u : 0u)) | (s3 & (groups > 3 ? 0x80000000u : 0u));
    return f;
}

// base64.c:131-179 character by character from character `pos` of a record (a group boundary,
// val = cnt = 0 there) with `produced` bytes already written; returns the record's output length
BRB_DEV uint32_t decode_serial(const int8_t *val, const uint8_t *a, uint64_t len, uint64_t pos, uint8_t *o,
                               uint32_t produced)
{
    brb_io::Snk ss;
    ss.init(o + produced, 3 * (len / 4) - produced);
    brb_io::Src src;
    src.init(a + pos, len - pos);
    uint32_t val4 = 0, cnt = 0, outn = 0;
    uint64_t outacc = 0;
    bool on = true;
    for (uint64_t c4 = pos; c4 < len && on; c4 += 4) {
        const uint32_t chunk = src.next();
        const uint32_t nb = len - c4 >= 4 ? 4u : uint32_t(len - c4);
        for (uint32_t b = 0; b < nb; b++) {
            const uint32_t ch = (chunk >> (8 * b)) & 0xFFu;
            if (ch == 0) {              // C-string end (base64.c:146)
                on = false;
                break;
            }
            const int v = val[ch];
            if (v < 0)
                continue;
            val4 = (val4 << 6) | uint32_t(v);
            if (++cnt < 4)
                continue;
            const uint32_t t = ((val4 >> 16) & 0xFFu) | (val4 & 0xFF00u) | ((val4 & 0xFFu) << 16);
            outacc |= uint64_t(t) << (8 * outn);
            outn += 3;
            produced += 3;
            val4 = cnt = 0;
            if (outn >= 4) {
                ss.put(uint32_t(outacc));
                outacc >>= 32;
                outn -= 4;
            }
        }
    }
    if (outn) {
        ss.rem = outn;
        ss.put(uint32_t(outacc));
    }
    ss.flush();
    return produced;
}

}  // namespace brb_b64
