// base64_kernels.hip -- batched base64 codec, a group of lanes per record.
//
//   encode = brb_base64_encode_to_mb (libbrb_core/crypto/base64.c:304-361): every 3 input bytes
//            -> 4 characters of the standard alphabet, a 1- or 2-byte tail padded with '='.
//   decode = brb_base64_decode_to_mb (:131-179): the record is a C string (a NUL ends it), bytes
//            outside the alphabet are skipped, '=' counts as 0 (:363-376), every 4 counted
//            characters give 3 bytes, a trailing partial group is dropped.
//
// History (65 536 x 1500 B round trip): one lane per record with a per-lane dword reader, ~1.2 ms;
// per-lane 64-byte blocks, 235 us (round 2); wave-cooperative 192/256-byte steps through a per-wave
// LDS exchange, 154 us (round 3, 1 wave per SIMD at 246-497 VGPRs); the group kernels below, 91 us.
#include "brb_kernels.h"
#include "b64_piece.h"
#include "test_options.h"

namespace {

using namespace brb_b64;   // the per-lane pieces (b64_piece.h, run on the host by tests/c/lane_io_check.cpp)

constexpr int kBlock = 256;

// ---- group kernels: G lanes per record, 12 / 16-byte pieces -------------------------------------
//
// Neither direction of the codec carries state along a record (every 3 bytes <-> 4 characters on
// their own, while the characters are clean), so a record is cut into pieces: encode 12 input bytes
// -> 16 characters, decode 16 characters -> 12 bytes.  G lanes (a power of two, 1..64) work on one
// record, lane j of the group on pieces j, j + G, ...; a piece is one 16/12-byte access at a lane
// stride of 12/16 bytes, so a group's loads and stores are contiguous runs of 12 G / 16 G bytes,
// and the kernels hold 46 (encode) / 64 (decode) VGPRs -- 8 waves per SIMD instead of the
// lane-per-record kernels' 1 to 2, which waited on memory 36 % of the time.  The grid is persistent
// (kPersist workgroups): group k walks records k, k + groups, ...

constexpr unsigned kPersist = 2048;              // 8 workgroups of 4 waves on each of 256 CUs

__global__ __launch_bounds__(kBlock) void b64_encode_group_kernel(const uint8_t *__restrict__ in,
                                                                  const uint64_t *__restrict__ offs,
                                                                  const uint32_t *__restrict__ lens, uint64_t n,
                                                                  uint8_t *__restrict__ out,
                                                                  const uint64_t *__restrict__ ooffs, uint32_t lg)
{
    __shared__ uint16_t pair[4096];
    for (uint32_t e = threadIdx.x; e < 4096; e += kBlock)
        pair[e] = uint16_t(alpha(e >> 6) | (alpha(e & 63) << 8));
    __syncthreads();
    const uint32_t G = 1u << lg, sub = threadIdx.x & (G - 1);
    const uint64_t groups = uint64_t(gridDim.x) * (kBlock >> lg);
    for (uint64_t r = (uint64_t(blockIdx.x) * kBlock + threadIdx.x) >> lg; r < n; r += groups) {
        const uint64_t len = lens[r];
        const uint8_t *a = in + offs[r];
        uint8_t *o = out + ooffs[r];
        const uint64_t np = (len + 11) / 12;
        const bool al = (reinterpret_cast<uintptr_t>(a) & 3) == 0;
        // two pieces per lane per pass (p, p + G): both loads in flight before either is encoded (four
        // measured slower: 88 VGPRs, 5 waves per SIMD)
        for (uint64_t p = sub; p < np; p += 2 * G) {
            uint32_t d[2][4], m[2];
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const uint64_t pu = p + u * G;
                m[u] = pu < np ? (len - 12 * pu >= 12 ? 12u : uint32_t(len - 12 * pu)) : 0u;
                if (al && m[u] == 12)
                    load12_a4(a + 12 * pu, d[u]);
                else
                    load_piece(a + 12 * pu, m[u], d[u]);      // m == 0: nothing is read
            }
#pragma unroll
            for (int u = 0; u < 2; u++) {
                if (m[u]) {
                    uint32_t c[4];
                    const uint32_t q = encode_piece(pair, d[u], m[u], c);
                    store_piece(o + 16 * (p + u * G), q, c);
                }
            }
        }
    }
}

// Pieces before a record's first piece with a character outside the alphabet / '=' in its whole
// groups decode at fixed positions; from that piece's start the group's first lane finishes the
// record with the reference's serial rules (a skipped byte shifts every later group; a NUL ends
// the string).  The group finds that piece with one ballot per half pass, so no lane stores a
// piece at or after it.  Characters of a trailing partial group never produce output.
__global__ __launch_bounds__(kBlock) void b64_decode_group_kernel(const uint8_t *__restrict__ in,
                                                                  const uint64_t *__restrict__ offs,
                                                                  const uint32_t *__restrict__ lens, uint64_t n,
                                                                  uint8_t *__restrict__ out,
                                                                  const uint64_t *__restrict__ ooffs,
                                                                  uint32_t *__restrict__ olens, uint32_t lg)
{
    __shared__ int8_t val[256];
    for (uint32_t e = threadIdx.x; e < 256; e += kBlock)
        val[e] = int8_t(b64_value(e));
    __syncthreads();
    const uint32_t G = 1u << lg, lane = threadIdx.x & 63, sub = lane & (G - 1), gbase = lane - sub;
    const uint64_t gmask = G == 64 ? ~0ull : ((1ull << G) - 1) << gbase;
    const uint64_t groups = uint64_t(gridDim.x) * (kBlock >> lg);
    for (uint64_t r = (uint64_t(blockIdx.x) * kBlock + threadIdx.x) >> lg; r < n; r += groups) {
        const uint64_t len = lens[r];
        const uint8_t *a = in + offs[r];
        uint8_t *o = out + ooffs[r];
        const uint64_t ng = len / 4;                          // whole groups
        const uint64_t np = (ng + 3) / 4;                     // pieces holding a whole group
        uint64_t dirty = ~0ull;                               // first piece with a skipped byte / NUL
        for (uint64_t p = sub; p < np; p += 2 * G) {         // pieces p and p + G: both loads in flight
            const uint64_t p1 = p + G;
            const uint32_t g0 = ng - 4 * p >= 4 ? 4u : uint32_t(ng - 4 * p);
            const uint32_t g1 = p1 < np ? (ng - 4 * p1 >= 4 ? 4u : uint32_t(ng - 4 * p1)) : 0u;
            uint32_t d0[4], d1[4], b0[4], b1[4];
            load_piece(a + 16 * p, 4 * g0, d0);
            load_piece(a + 16 * p1, 4 * g1, d1);              // g1 == 0: nothing is read
            const uint32_t f0 = decode_piece(val, d0, g0, b0), f1 = decode_piece(val, d1, g1, b1);
            const uint64_t m0 = (__builtin_amdgcn_ballot_w64(f0 != 0) & gmask) >> gbase;
            const uint64_t m1 = (__builtin_amdgcn_ballot_w64(f1 != 0) & gmask) >> gbase;
            const uint64_t base = p - sub;
            if (m0 | m1)
                dirty = m0 ? base + __builtin_ctzll(m0) : base + G + __builtin_ctzll(m1);
            if (p < dirty)
                store_piece(o + 12 * p, 3 * g0, b0);
            if (g1 && p1 < dirty)
                store_piece(o + 12 * p1, 3 * g1, b1);
            if (dirty != ~0ull)
                break;                                        // group-uniform
        }
        if (sub == 0)
            olens[r] = dirty == ~0ull ? uint32_t(3 * ng) : decode_serial(val, a, len, 16 * dirty, o, uint32_t(12 * dirty));
    }
}

// log2 of the lanes per record: an average record takes two passes of two pieces per lane, at most
// 32 lanes (measured on 65 536 x 1500 B: 16 / 32 / 64 lanes 96.0 / 90.7 / 92.2 us per round trip);
// mean_len 0 = unknown (device mode): 32 lanes.  The test option forces it.
uint32_t group_lg(uint64_t mean_len, uint32_t piece)
{
    const int forced = brb_opt::get(brb_opt::kB64Group);
    if (forced >= 0 && forced <= 6)
        return uint32_t(forced);
    if (mean_len == 0)
        return 5;
    const uint64_t quarter = (mean_len + 4 * piece - 1) / (4 * piece);
    uint32_t lg = 0;
    while (lg < 5 && (1ull << lg) < quarter)
        lg++;
    return lg;
}

unsigned group_grid(uint64_t n, uint32_t lg)
{
    const uint64_t blocks = ((n << lg) + kBlock - 1) / kBlock;
    return unsigned(blocks < kPersist ? blocks : kPersist);
}

}  // namespace

namespace brb {

hipError_t launch_b64_encode(const uint8_t *in, const uint64_t *offs, const uint32_t *lens, uint64_t n, uint8_t *out,
                             const uint64_t *ooffs, uint64_t mean_len, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    const uint32_t lg = group_lg(mean_len, 12);
    b64_encode_group_kernel<<<group_grid(n, lg), kBlock, 0, s>>>(in, offs, lens, n, out, ooffs, lg);
    return hipGetLastError();
}

hipError_t launch_b64_decode(const uint8_t *in, const uint64_t *offs, const uint32_t *lens, uint64_t n, uint8_t *out,
                             const uint64_t *ooffs, uint32_t *olens, uint64_t mean_len, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    const uint32_t lg = group_lg(mean_len, 16);
    b64_decode_group_kernel<<<group_grid(n, lg), kBlock, 0, s>>>(in, offs, lens, n, out, ooffs, olens, lg);
    return hipGetLastError();
}

}  // namespace brb
