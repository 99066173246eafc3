// md5_lower_kernels.hip -- BRB_MD5LowerTextBatch: the MD5 of lower-cased keys, a key per lane.
//
// Digest of key r = BRB_MD5Init + BRB_MD5UpdateLowerText(key) + BRB_MD5Final (md5.c:38-47, 112-132,
// 134-168): a case-insensitive key -- a host name, a header name -- hashed without a context in memory.
// The loop is md5_any_kernel's (md5_kernels.hip): brb_io::BlockSrc on the key, the next 64-byte block
// in flight, each fetched block lower-cased in registers (brb_io::lower16) before it is compressed.  A
// fresh one-piece message starts on a block boundary, so no word funnel is needed.  The zeros that
// BlockSrc hands out past the key's end are not letters: the transform leaves the padding alone.
//
// The digest and / or ctx.string's 33 bytes (32 lower-case hex characters and a NUL, BRB_MD5ToStr's
// buffer) go out with __builtin_memcpy: neither row is aligned.
//
// Not kept: staging a wave's key span through LDS with coalesced loads.  Short keys packed
// back to back already share their cache lines between neighbouring lanes, and the per-lane loads were
// the faster form at 1 048 576 keys of 8 .. 64 bytes.
#include "brb_kernels.h"
#include "byte_stream.h"
#include "md5_device.h"

namespace {

constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock) void md5_lower_kernel(const uint8_t *__restrict__ data, const uint64_t *__restrict__ offs,
                                                           const uint32_t *__restrict__ lens, uint64_t n,
                                                           uint8_t *__restrict__ digests, uint8_t *__restrict__ strings)
{
    const uint64_t r = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (r >= n)
        return;
    const uint64_t len = lens[r];
    const uint8_t *a = data + (len ? offs[r] : 0);  // an empty key's offset need not be memory: not used
    const uint64_t nfull = len >> 6;
    Md5State st = md5_iv();
    uint32_t w[16];
    brb_io::BlockSrc src;                           // the next 64-byte block is always in flight
    src.init(a, len);
    for (uint64_t b = 0; b < nfull; ++b) {
        src.fetch(w);
        brb_io::lower16(w);
        md5_compress(st, w);
    }
    src.fetch(w);                                   // tail (bytes past the key read as 0)
    brb_io::lower16(w);
    brb_io::add_marker(w, len);
    md5_finish(st, w, uint32_t(len & 63), len);
    if (digests) {
        const uint4 v = make_uint4(st.a, st.b, st.c, st.d);
        __builtin_memcpy(digests + 16 * r, &v, 16);
    }
    if (strings) {
        const uint32_t d[4] = {st.a, st.b, st.c, st.d};
        uint32_t hx[8];
#pragma unroll
        for (uint32_t j = 0; j < 8; j++)
            hx[j] = hex4(d[j >> 1] >> (16 * (j & 1)));
        uint8_t *o = strings + 33 * r;
        __builtin_memcpy(o, hx, 32);
        stg8(o + 32, 0);
    }
}

}  // namespace

namespace brb {

hipError_t launch_md5_lower(const uint8_t *data, const uint64_t *offs, const uint32_t *lens, uint64_t n, uint8_t *digests,
                            uint8_t *strings, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    md5_lower_kernel<<<unsigned((n + kBlock - 1) / kBlock), kBlock, 0, s>>>(data, offs, lens, n, digests, strings);
    return hipGetLastError();
}

}  // namespace brb
