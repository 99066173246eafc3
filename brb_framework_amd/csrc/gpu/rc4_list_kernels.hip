// rc4_list_kernels.hip -- RC4 and RC4+MD5 framing over a buffer list per stream.
//
// rc4_kernels.hip takes one buffer per stream and launch, so a connection that queued k buffers in a
// round costs k launches, each loading and storing its 264-byte state.  Here lane s loads
// states[sidx ? sidx[s] : s] once, walks buffers first[s] .. first[s + 1] - 1 in order and stores the
// state once.  The keystream generator (rc4_device.h Gen) is a pure step pipeline that advances by
// exactly the bytes returned and knows nothing of buffer ends, so a buffer boundary is only a fresh
// source, sink and (frame / open) MD5 state.  Each buffer goes through the per-buffer body of
// rc4_block.h, the one the lone single-buffer kernel of rc4_kernels.hip calls once:
//
//   rc4_crypt_list_kernel    crypt_blocks per buffer, as rc4_crypt_kernel<true> (whole-sector sink)
//   rc4md5_frame_list_kernel frame_buffer per buffer, as rc4md5_frame_kernel
//   rc4md5_open_list_kernel  open_buffer per buffer, as rc4md5_open_kernel; valid[k] per buffer
//
// One lane per stream, kWaves waves per workgroup, the 64 KiB LDS permutation image of
// rc4_device.h.  These are lone-wave kernels: no partner wave, no wait on another wave, no atomics,
// so no protocol fault can occur.  A stream without buffers stores the state it loaded (the same
// 264 bytes: Gen::store drops the byte started ahead).  An empty buffer forms no address that is
// read or written (BlockSrc / BlockSrcW / Snk with n = 0).
//
// Launched through brb::Rc4Launch (brb_kernels.h): a descriptor with `first` set and no `kinds`.
#include "brb_kernels.h"
#include "rc4_block.h"
#include "rc4_device.h"
#include "test_options.h"

namespace {

using namespace brb_rc4;

constexpr int kWave = 64 * int(kWaves);   // threads per workgroup

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
    gen_place(g, slot, lane_word());
    uint8_t *state = nullptr;
    uint64_t k0 = 0, k1 = 0;
    if (live) {
        state = gen_load(g, states, sidx, s);
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
    gen_place(g, slot, lane_word());
    uint8_t *state = gen_load(g, states, sidx, s);
    const uint64_t k1 = first[s + 1];
    for (uint64_t k = first[s]; k < k1; k++)
        frame_buffer(g, payload + offs[k], lens[k], salts[k], frames + foffs[k]);
    g.store(state);
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
    gen_place(g, slot, lane_word());
    uint8_t *state = gen_load(g, states, sidx, s);
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

hipError_t launch_rc4_list(const Rc4Launch &l, hipStream_t s)
{
    const uint64_t n = l.n;
    if (n == 0)
        return hipSuccess;
    if (l.kind == BRB_RC4_KIND_FRAME)
        rc4md5_frame_list_kernel<<<grid_for(n), kWave, 0, s>>>(l.states, l.in, l.offs, l.lens, l.salts, l.out, l.ooffs, l.first, n,
                                                               l.sidx);
    else if (l.kind == BRB_RC4_KIND_OPEN)
        rc4md5_open_list_kernel<<<grid_for(n), kWave, 0, s>>>(l.states, l.in, l.out, l.offs, l.lens, l.first, n, l.valid, l.sidx,
                                                              l.ooffs);
    // cooperative block loads unless test option "rc4_list_coop" = 0 (16 384 x k x 1500 B, tools/conn_list_ab.py:
    // k = 2 216.3 -> 213.3 us, k = 4 528.8 -> 522.1 us, k = 8 804.4 -> 784.0 us; k = 1 within the spread)
    else if (brb_opt::get(brb_opt::kRc4ListCoop) != 0)
        rc4_crypt_list_kernel<true><<<grid_for(n), kWave, 0, s>>>(l.states, l.in, l.out, l.offs, l.lens, l.first, n, l.sidx, l.ooffs);
    else
        rc4_crypt_list_kernel<false><<<grid_for(n), kWave, 0, s>>>(l.states, l.in, l.out, l.offs, l.lens, l.first, n, l.sidx, l.ooffs);
    return hipGetLastError();
}

}  // namespace brb
