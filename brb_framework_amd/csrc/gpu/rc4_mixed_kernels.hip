// rc4_mixed_kernels.hip -- RC4, RC4+MD5 frame and RC4+MD5 open streams in one launch.
//
// The list kernels of rc4_list_kernels.hip fix one kind per launch, as the reference fixes one
// algo_code per connection (ev_kq_aio_transform.c:75-108) -- but a daemon holds RC4 and RC4_MD5
// connections side by side, and a connection's read and write directions are different states.  Here
// every stream carries its kind: lane s loads states[sidx ? sidx[s] : s] once, reads kind[s], walks
// buffers first[s] .. first[s + 1] - 1 through the per-buffer body of its kind (rc4_block.h, the bodies
// the lone and the list kernels call) and stores the state once.
//
// The branch on the kind stands outside the buffer loop: a wave whose lanes agree runs one body and
// skips the others on an empty exec mask; a wave with two or three kinds runs them one after another
// (right, only slower), so callers put streams of a kind next to each other.  All three kinds load
// their blocks per lane (BlockSrc); the cooperative form needs 64 lanes in step and stays with
// rc4_crypt_list_kernel<true>.  CRYPT writes through Snk, not SectorSnk: the sector sink's LDS rows
// (36 864 bytes) would put the kernel at 102 400 bytes of LDS and one workgroup per CU, and the frame
// and open lanes, which are most of a mixed round, would lose the second workgroup they have in
// their own list kernels.  Lone waves only: no partner wave, no wait, no atomics, so no protocol
// fault can occur.
//
// Launched through brb::Rc4Launch (brb_kernels.h): a descriptor with `kinds` set.
#include "brb_kernels.h"
#include "rc4_block.h"
#include "rc4_device.h"

namespace {

using namespace brb_rc4;

constexpr int kWave = 64 * int(kWaves);   // threads per workgroup

__global__ __launch_bounds__(kWave) void rc4_mixed_list_kernel(uint8_t *__restrict__ states,
                                                               const uint8_t *__restrict__ kind, const uint8_t *in,
                                                               uint8_t *out, const uint64_t *__restrict__ offs,
                                                               const uint32_t *__restrict__ lens,
                                                               const uint64_t *__restrict__ ooffs,
                                                               const uint64_t *__restrict__ salts,
                                                               const uint64_t *__restrict__ first, uint64_t n,
                                                               uint8_t *__restrict__ valid,
                                                               const uint32_t *__restrict__ sidx)
{
    __shared__ __attribute__((aligned(16))) uint8_t slot[kSlotLds];
    const uint64_t s = uint64_t(blockIdx.x) * kWave + threadIdx.x;
    if (s >= n)
        return;
    Gen g;
    gen_place(g, slot, lane_word());
    uint8_t *state = gen_load(g, states, sidx, s);
    const uint32_t kd = kind[s];
    const uint64_t k0 = first[s], k1 = first[s + 1];
    if (kd == BRB_RC4_KIND_CRYPT) {
        for (uint64_t k = k0; k < k1; k++) {
            const uint64_t len = lens[k];
            brb_io::BlockSrc src;
            Snk snk;
            src.init(in + offs[k], len);
            snk.init(out + ooffs[k], len);
            crypt_blocks(src, snk, g, len, uint32_t((len + 63) >> 6));
            snk.flush();
        }
    } else if (kd == BRB_RC4_KIND_FRAME) {
        for (uint64_t k = k0; k < k1; k++)
            frame_buffer(g, in + offs[k], lens[k], salts[k], out + ooffs[k]);
    } else {
        for (uint64_t k = k0; k < k1; k++)
            valid[k] = uint8_t(open_buffer(g, in + offs[k], out + ooffs[k], lens[k]));
    }
    g.store(state);
}

}  // namespace

namespace brb {

hipError_t launch_rc4_mixed(const Rc4Launch &l, hipStream_t s)
{
    if (l.n == 0)
        return hipSuccess;
    rc4_mixed_list_kernel<<<unsigned((l.n + kWave - 1) / kWave), kWave, 0, s>>>(l.states, l.kinds, l.in, l.out, l.offs, l.lens,
                                                                                l.ooffs, l.salts, l.first, l.n, l.valid, l.sidx);
    return hipGetLastError();
}

}  // namespace brb
