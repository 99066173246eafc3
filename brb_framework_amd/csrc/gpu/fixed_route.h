// fixed_route.h -- which kernel a fixed-stride digest call (BRB_MD5BatchFixed, BrbSha1_BatchFixed)
// runs: one host function of the record base, the record length and two test options.  The
// launchers (launch_md5_fixed, launch_sha1_fixed, launch_fixed_dma) switch on it, and
// BRB_CryptoGPU_TestFixedRoute exports it, so a test can ask instead of believing a comment.
// Host code only; no device is needed.
#pragma once

#include <stdint.h>

#include "brb_crypto.h"
#include "test_options.h"

namespace brb_digest {

// The values are BRB_FIXED_ROUTE_* of include/brb_crypto.h, in launch order.
enum FixedRoute : int {
    kRouteLaneA4 = BRB_FIXED_ROUTE_LANE_A4,        // md5_/sha1_fixed_a4_kernel (per lane)
    kRouteLaneAny = BRB_FIXED_ROUTE_LANE_ANY,      // md5_/sha1_any_kernel<FIXED = true> (per lane)
    kRouteLine = BRB_FIXED_ROUTE_LINE,             // digest_line_kernel
    kRouteVarLine = BRB_FIXED_ROUTE_VAR_LINE,      // digest_var_line_kernel<..., FIXED>
    kRouteDmaTicket = BRB_FIXED_ROUTE_DMA_TICKET,  // digest_fixed_dma_kernel<Alg, 8, 2, 2, OUT_AL, false, true>
    kRouteB64R8 = BRB_FIXED_ROUTE_B64R_8,          // digest_b64r_kernel, grid cap 2048
    kRouteB64R4 = BRB_FIXED_ROUTE_B64R_4,          // digest_b64r_kernel, grid cap 1024
    kRouteB64 = BRB_FIXED_ROUTE_B64,               // digest_b64_kernel
    kRouteDmaShort = BRB_FIXED_ROUTE_DMA_SHORT     // digest_fixed_dma_kernel<Alg, 4, 2, 1, OUT_AL>
};

// The LDS-DMA kernels address a group's 64 records with 32-bit offsets from one descriptor base:
// lane 63's largest offset, 63 rec_len + 3072 + 112, has to stay below the clamped extent 2^31 - 1.
inline bool dma_supported(uint32_t rec_len)
{
    return rec_len > 0 && uint64_t(rec_len) * 64 + 64 < (uint64_t(1) << 31);
}

// Line-aligned staging needs 4-byte record bases (the window shift is whole dwords).
inline bool line_supported(uintptr_t data, uint32_t rec_len)
{
    return rec_len > 64 && rec_len <= (1u << 20) && (rec_len & 3) == 0 && (data & 3) == 0;
}

// Test option "fixed_var_line" = 0 keeps byte-aligned fixed-stride records on the record-relative
// kernel (A/B measurements).
inline bool fixed_var_line_enabled()
{
    return brb_opt::get(brb_opt::kFixedVarLine) != 0;
}

inline FixedRoute fixed_route(uintptr_t data, uint32_t rec_len)
{
    if (!dma_supported(rec_len))                   // empty records, and records of 32 MiB - 1 and more
        return (data & 3) == 0 && (rec_len & 3) == 0 ? kRouteLaneA4 : kRouteLaneAny;
    if (line_supported(data, rec_len))
        return kRouteLine;
    if (rec_len > 64 && rec_len <= (1u << 20) && fixed_var_line_enabled())
        return kRouteVarLine;                      // any byte alignment
    if (rec_len > 64)
        return kRouteDmaTicket;
    if (rec_len == 64) {
        const int k = brb_opt::get(brb_opt::kB64Kernel);
        if (k == 2)
            return kRouteB64R8;
        if (k > 2)
            return kRouteB64R4;
        if (k != 0)
            return kRouteB64;
    }
    return kRouteDmaShort;
}

}  // namespace brb_digest
