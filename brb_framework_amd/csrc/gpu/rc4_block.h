// rc4_block.h -- block helpers shared by the RC4 kernels (rc4_kernels.hip: one buffer per stream;
// rc4_list_kernels.hip: a buffer list per stream).
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

// Decrypt frame block b (chunks 16b .. 16b + 15 of a frame of F bytes, fetched into c) into pt and
// the sink.
BRB_DEV void decrypt_block(const uint32_t (&c)[16], Snk &snk, Gen &g, uint64_t F, uint64_t b, uint32_t (&pt)[16])
{
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

BRB_DEV void decrypt_block(brb_io::BlockSrc &src, Snk &snk, Gen &g, uint64_t F, uint64_t b, uint32_t (&pt)[16])
{
    uint32_t c[16];
    src.fetch(c);
    decrypt_block(c, snk, g, F, b, pt);
}

}  // namespace brb_rc4
