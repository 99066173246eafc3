// keysetup_kernels.hip -- batched key setup (EvAIOReqTransform_CryptoEnable, ev_kq_aio_transform.c:75-108):
// the RC4 key-scheduling sweep (rc4.c:40-62) and the Blowfish key schedule (blowfish.c:382-443) for
// many independent keys per launch.  Both schedules are serial per key; the parallelism is across keys.
//
// Key record i = keys[koffs[i] .. + klens[i]) at any byte offset; records may overlap or be one shared
// key.  Key bytes are read through aligned dwords (brb_io::Src), only the bytes the reference would
// read (the first min(len, 256) for RC4, min(len, 72) for Blowfish) and nothing past the dword
// holding the last of them.  A zero length (a broken promise in device mode) reads nothing and
// schedules a single zero key byte, so the lane still touches its own output only.
#include <hip/hip_runtime.h>

#include "../common/blowfish_pi.h"
#include "brb_kernels.h"
#include "byte_stream.h"
#include "rc4_device.h"

namespace {

// ------------------------------------------------------------------------------------------------
// RC4: one lane per key, 256-lane workgroups
// ------------------------------------------------------------------------------------------------
// The permutation lives in brb_rc4::Perm's 64 KiB image (byte x of (wave w, lane l) at
// x * 256 + l * 4 + w: every access of a lane lands in its own bank whatever the index).  A second
// image of the same layout holds the lane's key bytes 0 .. min(len, 256) - 1, staged once with
// independent dword loads, so the sweep never waits on HBM: the key byte of step i + 1 is read from
// LDS by a cursor that wraps at the key length.
//
// The sweep (brb_rc4.c:24-34) is 256 serial steps  j += S[i] + key[i % len]; swap(S[i], S[j]).  On
// the chain of step i are only j and the S[j] read: S[i + 1] and the next key byte are read together
// with S[j], before swap i is written, and the raw S[i + 1] is patched when the swap moved it
// (j == i + 1 -> the old S[i]), as brb_rc4::Gen does for its read-ahead.  One LDS round trip per step.
constexpr uint32_t kRc4Threads = 256;
constexpr uint32_t kStateDwords = brb_rc4::kStateBytes / 4;   // 66: perm, then indices + flags, all zero

__global__ __launch_bounds__(kRc4Threads) void rc4_keysetup_kernel(uint8_t *__restrict__ states,
                                                                   const uint8_t *__restrict__ keys,
                                                                   const uint64_t *__restrict__ koffs,
                                                                   const uint32_t *__restrict__ klens, uint64_t n,
                                                                   const uint32_t *__restrict__ slots, uint64_t second)
{
    __shared__ __attribute__((aligned(16))) uint8_t perm[brb_rc4::kSlotLds];
    __shared__ __attribute__((aligned(16))) uint8_t kimg[brb_rc4::kSlotLds];
    const uint64_t s = uint64_t(blockIdx.x) * kRc4Threads + threadIdx.x;
    if (s >= n)            // no barrier below: a lane without a key does nothing and writes nothing
        return;
    const uint32_t lw = (threadIdx.x & 63) * 4 + (threadIdx.x >> 6);
    const brb_rc4::Perm P{perm, lw}, K{kimg, lw};

    // key[k % len] for k < 256 only ever reads the first min(len, 256) bytes
    uint32_t len = min(klens[s], 256u);
    brb_io::Src src;
    src.init(keys + koffs[s], len);
    const uint32_t kwords = (len + 3) >> 2;
#pragma unroll 4
    for (uint32_t w = 0; w < kwords; w++) {
        const uint32_t v = src.next();
#pragma unroll
        for (uint32_t b = 0; b < 4; b++)
            K.wr(4 * w + b, v >> (8 * b));
    }
    if (len == 0) {
        K.wr(0, 0);
        len = 1;
    }
#pragma unroll 8
    for (uint32_t x = 0; x < 256; x++)
        P.wr(x, x);

    uint32_t j = 0;
    uint32_t a = 0;                 // S[0]
    uint32_t kb = K.rd(0);
    uint32_t kp = 0;                // cursor of kb
#pragma unroll 4
    for (uint32_t i = 0; i < 256; i++) {
        j = (j + a + kb) & 255u;
        kp = kp + 1 == len ? 0 : kp + 1;
        const uint32_t i1 = (i + 1) & 255u;
        const uint32_t u = P.rd(j);          // the only read on the chain
        const uint32_t raw = P.rd(i1);       // S[i + 1] before swap i is written
        kb = K.rd(kp);
        P.wr(i, u);
        P.wr(j, a);
        a = j == i1 ? a : raw;               // swap i moved S[i + 1]
    }

    const uint64_t d = slots ? slots[s] : s;
    uint32_t *w0 = reinterpret_cast<uint32_t *>(states + d * brb_rc4::kStateBytes);
    uint32_t *w1 = reinterpret_cast<uint32_t *>(states + d * brb_rc4::kStateBytes + second);
#pragma unroll 8
    for (uint32_t k = 0; k < kStateDwords; k++) {
        uint32_t v = 0;                      // dwords 64, 65: index1 = index2 = 0, six zero bytes
        if (k < 64)
            v = P.rd(4 * k) | (P.rd(4 * k + 1) << 8) | (P.rd(4 * k + 2) << 16) | (P.rd(4 * k + 3) << 24);
        stg(w0 + k, v);
        if (second)
            stg(w1 + k, v);
    }
}

// ------------------------------------------------------------------------------------------------
// Blowfish: 16 keys per workgroup, one lane per key
// ------------------------------------------------------------------------------------------------
// A key schedule is 521 chained encryptions (8 336 F) that replace P and S while later encryptions
// read them, so every key needs its own mutable tables: 8 KiB of S-boxes per key, 16 keys in a
// 128 KiB LDS image,
//
//   entry (table t, index x) of key slot k  ->  LDS byte  (t * 256 + x) * 128 + k * 8
//
// A ds_read_b64 banks by (address / 4) mod 64 = 32 * (x & 1) + 2 k: the bank pair depends on the
// slot only within either half row, so the 16 lanes' gathers never conflict.  An address is a
// v_bfe_u32 and a v_lshl_or_b32 onto the lane's base t * 32 KiB + k * 8.  P (18 words) stays in
// registers: the P phase is unrolled, the S phase loops with P fixed.  The four gathers of an F are
// issued together; the chain is one LDS round trip per F.  Lanes 0..15 of wave 0 run the schedules;
// all 256 lanes fill the image from the pi tables and write the finished contexts out transposed
// (consecutive lanes store consecutive qwords of one context).
constexpr uint32_t kBfKeys = 16;
constexpr uint32_t kBfThreads = 256;
constexpr uint32_t kBfEntries = 1024;                 // 4 x 256 S-box entries
constexpr uint32_t kBfCtxQwords = 18 + kBfEntries;    // BRB_BLOWFISH_CTX: P[18] then S[4][256]
constexpr uint32_t kBfKeyBytes = 72;                  // 18 P words x 4 key bytes

struct BfLane {
    uint8_t *lds;             // the image
    uint32_t b0, b1, b2, b3;  // t * 32 KiB + k * 8

    BRB_DEV uint64_t q(uint32_t a) const { return *reinterpret_cast<const uint64_t *>(lds + a); }

    // blowfish.c:445-462 on 64-bit words: indices from the low 32 bits, carries kept
    BRB_DEV uint64_t f(uint64_t x64) const
    {
        const uint32_t x = uint32_t(x64);
        const uint64_t A = q(((x >> 24) << 7) | b0);
        const uint64_t B = q((((x >> 16) & 255u) << 7) | b1);
        const uint64_t C = q((((x >> 8) & 255u) << 7) | b2);
        const uint64_t D = q(((x & 255u) << 7) | b3);
        return ((A + B) ^ C) + D;
    }

    BRB_DEV void encrypt(const uint64_t (&P)[18], uint64_t &xl, uint64_t &xr) const
    {
        uint64_t L = xl, R = xr;
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
            L ^= P[i];
            R ^= f(L);
            R ^= P[i + 1];
            L ^= f(R);
        }
        xl = R ^ P[17];
        xr = L ^ P[16];
    }
};

__global__ __launch_bounds__(kBfThreads) void blowfish_keysetup_kernel(uint64_t *__restrict__ ctxs,
                                                                       const uint8_t *__restrict__ keys,
                                                                       const uint64_t *__restrict__ koffs,
                                                                       const uint32_t *__restrict__ klens, uint64_t n)
{
    __shared__ __attribute__((aligned(16))) uint64_t tab[kBfEntries * kBfKeys];   // 128 KiB
    __shared__ uint64_t pl[kBfKeys][18];                                          // finished P arrays
    __shared__ uint32_t kw[kBfKeys][kBfKeyBytes / 4];                             // staged key bytes
    const uint32_t tid = threadIdx.x;
    const uint64_t key0 = uint64_t(blockIdx.x) * kBfKeys;
    const uint32_t nk = uint32_t(min(uint64_t(kBfKeys), n - key0));               // grid = ceil(n / 16): key0 < n

    for (uint32_t q = tid; q < kBfEntries * kBfKeys; q += kBfThreads)
        tab[q] = BRB_BF_PI_S[q >> 12][(q >> 4) & 255u];
    __syncthreads();

    if (tid < nk) {
        const uint32_t k = tid;
        // the 72 key bytes are taken cyclically: only the first min(len, 72) are read
        uint32_t len = min(klens[key0 + k], kBfKeyBytes);
        brb_io::Src src;
        src.init(keys + koffs[key0 + k], len);
        const uint32_t kwords = (len + 3) >> 2;
        for (uint32_t w = 0; w < kwords; w++)
            kw[k][w] = src.next();
        if (len == 0) {
            kw[k][0] = 0;
            len = 1;
        }
        const uint8_t *kb = reinterpret_cast<const uint8_t *>(kw[k]);

        uint64_t P[18];
        uint32_t j = 0;
#pragma unroll
        for (int i = 0; i < 18; i++) {                // blowfish.c:395-414: big-endian, j wraps at keyLen
            uint32_t data = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                data = (data << 8) | kb[j];
                j = j + 1 >= len ? 0 : j + 1;
            }
            P[i] = uint64_t(BRB_BF_PI_P[i] ^ data);
        }

        BfLane ln;
        ln.lds = reinterpret_cast<uint8_t *>(tab);
        ln.b0 = k * 8;
        ln.b1 = ln.b0 + 1 * 32768u;
        ln.b2 = ln.b0 + 2 * 32768u;
        ln.b3 = ln.b0 + 3 * 32768u;
        uint64_t L = 0, R = 0;
#pragma unroll
        for (int i = 0; i < 18; i += 2) {             // :419-427
            ln.encrypt(P, L, R);
            P[i] = L;
            P[i + 1] = R;
        }
#pragma unroll 1
        for (uint32_t e = 0; e < kBfEntries; e += 2) {   // :429-440, S[t][i] with e = t * 256 + i
            ln.encrypt(P, L, R);
            tab[e * kBfKeys + k] = L;
            tab[(e + 1) * kBfKeys + k] = R;
        }
#pragma unroll
        for (int i = 0; i < 18; i++)
            pl[k][i] = P[i];
    }
    __syncthreads();

    for (uint32_t k = 0; k < nk; k++) {
        uint64_t *out = ctxs + (key0 + k) * kBfCtxQwords;
        for (uint32_t q = tid; q < kBfCtxQwords; q += kBfThreads)
            out[q] = q < 18 ? pl[k][q] : tab[(q - 18) * kBfKeys + k];
    }
}

}  // namespace

namespace brb {

hipError_t launch_rc4_keysetup(uint8_t *states, const uint8_t *keys, const uint64_t *koffs, const uint32_t *klens,
                               uint64_t n, hipStream_t s, const uint32_t *slots, uint64_t second)
{
    if (n == 0)
        return hipSuccess;
    rc4_keysetup_kernel<<<unsigned((n + kRc4Threads - 1) / kRc4Threads), kRc4Threads, 0, s>>>(states, keys, koffs, klens,
                                                                                              n, slots, second);
    return hipGetLastError();
}

hipError_t launch_blowfish_keysetup(uint64_t *ctxs, const uint8_t *keys, const uint64_t *koffs, const uint32_t *klens,
                                    uint64_t n, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    blowfish_keysetup_kernel<<<unsigned((n + kBfKeys - 1) / kBfKeys), kBfThreads, 0, s>>>(ctxs, keys, koffs, klens, n);
    return hipGetLastError();
}

}  // namespace brb
