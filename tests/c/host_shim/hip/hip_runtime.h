// Host stand-in for <hip/hip_runtime.h>: just enough for tests/c/lane_io_check.cpp to compile the
// per-lane device headers (brb_gpu_common.h, byte_stream.h, b64_piece.h, seg_walk.h) with clang++
// for the CPU, one lane at a time.  It comes first on the include path of that program only.
// The instruction stand-ins follow the CDNA ISA's definitions of the instructions, not any use the
// project makes of them.
#pragma once

#include <stdint.h>
#include <stdlib.h>

#define __device__
#define __host__
#define __forceinline__ inline

struct uint4 {
    uint32_t x, y, z, w;
};
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }

struct brb_shim_dim3 {
    uint32_t x, y, z;
};
inline brb_shim_dim3 threadIdx{0, 0, 0};

inline int __shfl(int v, int) { return v; }   // a wave of one lane

#define __HIP_MEMORY_SCOPE_SINGLETHREAD 1
#define __HIP_MEMORY_SCOPE_WAVEFRONT 2
#define __HIP_MEMORY_SCOPE_WORKGROUP 3
#define __HIP_MEMORY_SCOPE_AGENT 4
#define __HIP_MEMORY_SCOPE_SYSTEM 5

namespace brb_shim {

// v_alignbit_b32: D = ({S0, S1} >> S2[4:0]) & 0xFFFFFFFF
inline uint32_t alignbit(uint32_t s0, uint32_t s1, uint32_t s2)
{
    return uint32_t(((uint64_t(s0) << 32) | s1) >> (s2 & 31u));
}

// v_perm_b32: byte i of D is picked from the 8 bytes {S0, S1} by byte i of the selector S2:
// 0..3 = that byte of S1, 4..7 = byte 0..3 of S0, 0x0C = 0x00.  The ISA's other selectors (sign
// replication, 0xFF) are not used by the headers under test: they trap here.
inline uint32_t perm(uint32_t s0, uint32_t s1, uint32_t s2)
{
    uint32_t d = 0;
    for (uint32_t i = 0; i < 4; i++) {
        const uint32_t sel = (s2 >> (8 * i)) & 0xFFu;
        uint32_t b;
        if (sel < 4)
            b = (s1 >> (8 * sel)) & 0xFFu;
        else if (sel < 8)
            b = (s0 >> (8 * (sel - 4))) & 0xFFu;
        else if (sel == 0x0C)
            b = 0;
        else
            abort();
        d |= b << (8 * i);
    }
    return d;
}

// v_bitop3_b32: bit k of D = bit ((a_k << 2) | (b_k << 1) | c_k) of the 8-bit truth table
inline uint32_t bitop3(uint32_t a, uint32_t b, uint32_t c, uint32_t tt)
{
    uint32_t d = 0;
    for (uint32_t k = 0; k < 32; k++) {
        const uint32_t idx = (((a >> k) & 1u) << 2) | (((b >> k) & 1u) << 1) | ((c >> k) & 1u);
        d |= ((tt >> idx) & 1u) << k;
    }
    return d;
}

inline void nothing(int) {}

}  // namespace brb_shim

#define __builtin_amdgcn_alignbit brb_shim::alignbit
#define __builtin_amdgcn_perm brb_shim::perm
#define __builtin_amdgcn_bitop3_b32 brb_shim::bitop3
#define __builtin_amdgcn_readfirstlane(v) (v)
#define __builtin_amdgcn_s_waitcnt brb_shim::nothing
#define __builtin_amdgcn_s_sleep brb_shim::nothing
