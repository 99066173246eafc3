// blowfish_keyed_kernels.hip -- Blowfish ECB with a context per record (BRB_Blowfish_EncryptBatchKeyed /
// DecryptBatchKeyed) and the plan / finish steps of BRB_MemBufferEncryptBatch / DecryptBatch, for gfx950.
//
// Record i = counts[i] blocks of two 64-bit words at words + woffs[i] (an offset in 8-byte words, so a
// record may start at 8 mod 16), keyed by ctxs[ctx_index ? ctx_index[i] : i].  Every output word equals
// BRB_Blowfish_Encrypt/Decrypt (blowfish.c:312-380), bit for bit in all 64 bits: the rounds are
// brb_bf::blocks_rep of blowfish_device.h, unchanged.
//
// Image.  bf_rep_kernel's 128 KiB LDS image holds 16 copies of one context's S-boxes; here the 16
// copies are 16 context *slots*:
//
//   byte address = region * 64 KiB + x * 256 + half * 128 + slot * 8      table t = 2 * region + half
//
// A lane's slot is lane & 15, exactly RepLane's copy, so brb_bf::gather serves as it stands: one
// v_perm_b32 per address, the bank pair of a ds_read_b64 is slot + 16 * half whatever the index, the
// S0 / S1 gathers of the two lanes of a 32-lane group that share a slot go to opposite halves
// (conflict-free), the S2 / S3 gathers are 2-way: 1 + 1 + 2 + 2 LDS cycles per F and lane group, as
// bf_rep_kernel.  (The key-setup kernel's image, (t * 256 + x) * 128 + slot * 8, banks by
// 32 (x & 1) + 2 slot: at worst 2-way on all four gathers, 6 cycles per F on average as well, but an
// address there is a bit-field extract and a shift-or.)  When every record names one context the
// image is bf_rep_kernel's 16x replicated table.
//
// Work.  Persistent grid, one 1024-thread workgroup per CU, over groups of 16 consecutive records:
// slot k takes record 16 g + k, and the slot's 64 lanes (4 per wave x 16 waves; lane m of the slot is
// wave * 4 + (lane >> 4)) take its blocks m, m + 64, ...  The next blocks of a lane are loaded before
// the rounds of its current ones; a lane loads only blocks of its own record and stores are guarded,
// so a record of 0 blocks touches nothing, neither its words nor its context.  P is per lane (its slot's 18 words, in application
// order) in VGPRs.  One record far longer than the others of its group runs on its slot's 64 lanes
// while the other 960 wait at the group's end: long single-key buffers belong to
// BRB_Blowfish_EncryptBatch (DESIGN.md §4.2a has the measurement).
//
// Fill.  A slot is loaded only when its record names another context than the one the slot holds
// (a record of 0 blocks names none), so equal indices at a stride of 16 records -- above all one
// context for every record -- load once per workgroup.  A ds_write_b64 is serviced in four groups of
// 16 consecutive lanes and banks by (address / 4) mod 32 = 2 * slot:
//   spread (default): lane = (slot, sub) with slot = lane & 15: the 16 lanes of a group write 16
//       slots, conflict-free; a lane loads two consecutive entries (16 bytes) of its slot's context,
//       a wave's load instruction 16 pieces of 64 bytes;
//   plain (A/B, test option "bf_keyed" = 1): slot after slot, thread t copies entry t: contiguous
//       8 KiB loads, but the 16 lanes of a group write one slot, 16-way conflicted.
//
// MemBuffer decrypt stop (mem_buf.c:1595-1596): the STOP variant first scans the record's ciphertext
// for its first block with a zero word (a min over the slot's lanes in LDS), and after a workgroup
// barrier -- so the scan of a record is complete before any of its words is written -- decrypts the
// blocks before it and writes the count to blocks_done.
#include "blowfish_device.h"
#include "brb_kernels.h"
#include "test_options.h"

namespace {

using brb_bf::kRepQwords;
using brb_bf::kRepThreads;

constexpr uint32_t kSlots = 16;                      // context slots of the image = records per group
constexpr uint32_t kSlotLanes = kRepThreads / kSlots;   // 64 lanes per record
constexpr uint32_t kCtxQwords = 18 + 1024;           // BRB_BLOWFISH_CTX: P[18] then S[4][256]

// image qword of S-box entry e = t * 256 + x of slot k
BRB_DEV uint32_t img_q(uint32_t e, uint32_t k)
{
    const uint32_t t = e >> 8, x = e & 255u;
    return (t >> 1) * 8192u + x * 32u + (t & 1u) * 16u + k;
}

template <int ILP, bool DECRYPT, bool STOP, bool SPREAD>
__global__ __launch_bounds__(kRepThreads) void bf_keyed_kernel(const uint64_t *__restrict__ ctxs,
                                                               const uint32_t *__restrict__ ctx_index,
                                                               uint64_t *__restrict__ words,
                                                               const uint64_t *__restrict__ woffs,
                                                               const uint32_t *__restrict__ counts, uint64_t n_rec,
                                                               uint32_t *__restrict__ blocks_done)
{
    __shared__ __attribute__((aligned(16))) uint64_t tab[kRepQwords];
    __shared__ uint32_t stop[kSlots];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t k = lane & 15u, sub = lane >> 4;
    const uint32_t m = wave * 4 + sub;               // this lane among its slot's 64
    brb_bf::RepLane ln;
    ln.init(lane);
    const uint8_t *lds = reinterpret_cast<const uint8_t *>(tab);

    uint64_t held = ~uint64_t(0);                    // the context index slot k holds
    uint64_t P[18];
#pragma unroll
    for (int i = 0; i < 18; i++)
        P[i] = 0;

    const uint64_t n_groups = (n_rec + kSlots - 1) / kSlots;
    for (uint64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const uint64_t rec = g * kSlots + k;
        uint64_t cnt = rec < n_rec ? counts[rec] : 0;
        uint64_t ci = held;
        uint64_t *w = words;
        if (cnt) {
            ci = ctx_index ? uint64_t(ctx_index[rec]) : rec;
            w = words + woffs[rec];
        }
        const bool need = ci != held;
        held = ci;
        __syncthreads();                             // the previous group's gathers are done
        if (need) {
            const uint64_t *ctx = ctxs + ci * kCtxQwords;
#pragma unroll
            for (int i = 0; i < 18; i++)
                P[i] = ctx[DECRYPT ? 17 - i : i];
        }
        if (SPREAD) {
            if (need) {
                const uint64_t *S = ctxs + ci * kCtxQwords + 18;
#pragma unroll 4
                for (uint32_t pass = 0; pass < 8; pass++) {
                    const uint32_t e = pass * 128u + wave * 8u + sub * 2u;   // e and e + 1 share a table
                    const uint64_t v0 = S[e], v1 = S[e + 1];
                    tab[img_q(e, k)] = v0;
                    tab[img_q(e + 1, k)] = v1;
                }
            }
        } else {
            for (uint32_t kk = 0; kk < kSlots; kk++) {   // lane kk of every wave belongs to slot kk
                const bool nk = __shfl(int(need), int(kk)) != 0;
                const uint64_t ck = __shfl(ci, int(kk));
                if (nk)
                    tab[img_q(tid, kk)] = ctxs[ck * kCtxQwords + 18 + tid];
            }
        }
        if (STOP && m == 0)
            stop[k] = uint32_t(cnt);
        __syncthreads();

        if (STOP) {
            uint64_t first = cnt;
            for (uint64_t j = m; j < cnt; j += kSlotLanes)
                if (w[2 * j] == 0 || w[2 * j + 1] == 0) {
                    first = j;
                    break;                           // later blocks of this lane are larger
                }
            if (first < cnt)
                atomicMin(&stop[k], uint32_t(first));
            __syncthreads();                         // every record of the group is scanned: writes may begin
            cnt = stop[k];
            if (m == 0 && rec < n_rec)
                blocks_done[rec] = uint32_t(cnt);
        }

        // chain c of a lane holds block j + 64 c; the next ILP blocks are loaded before the rounds.  Inside
        // the loop a lane owns block j, so a chain past the record's end re-reads block j instead of
        // branching: the loads are unconditional and hipcc issues them ahead of the rounds (a guarded
        // load is waited for inside its branch, as bf_rep_kernel found); stores are guarded.
        uint64_t j = m;
        uint64_t cl[ILP], cr[ILP];
#pragma unroll
        for (int c = 0; c < ILP; c++)
            cl[c] = cr[c] = 0;
        if (j < cnt) {
#pragma unroll
            for (int c = 0; c < ILP; c++) {
                const uint64_t b = j + uint64_t(c) * kSlotLanes;
                const uint64_t bb = b < cnt ? b : j;
                cl[c] = w[2 * bb];
                cr[c] = w[2 * bb + 1];
            }
        }
        while (j < cnt) {
            const uint64_t nj = j + uint64_t(ILP) * kSlotLanes;
            uint64_t nl[ILP], nr[ILP];
#pragma unroll
            for (int c = 0; c < ILP; c++) {
                const uint64_t b = nj + uint64_t(c) * kSlotLanes;
                const uint64_t bb = b < cnt ? b : j;
                nl[c] = w[2 * bb];
                nr[c] = w[2 * bb + 1];
            }
            brb_bf::blocks_rep<ILP>(lds, ln, P, cl, cr);
            // all chains complete here (bf_rep_kernel: hipcc otherwise sinks chain c > 0 below the
            // guarded store of chain 0 and runs the chains one after the other)
#pragma unroll
            for (int c = 0; c < ILP; c++)
                asm volatile("" ::"v"(cl[c]), "v"(cr[c]));
#pragma unroll
            for (int c = 0; c < ILP; c++) {
                const uint64_t b = j + uint64_t(c) * kSlotLanes;
                if (b < cnt) {
                    w[2 * b] = cl[c];
                    w[2 * b + 1] = cr[c];
                }
                cl[c] = nl[c];
                cr[c] = nr[c];
            }
            j = nj;
        }
    }
}

// ---- MemBuffer batch: plan and finish (device mode; host mode plans on the host) -----------------
// Buffer i = data + buf_offsets[i] with MemBuffer size sizes[i] and offset argument offsets[i]
// (mem_buf.c:1499-1617): (size +/- offset) / 8 + 2 words rounded up to pairs, from data + buf_offsets[i]
// + offsets[i].  A buffer that breaks the device-mode promises (start not 8-byte aligned, decrypt
// size < offset, seed index out of range, 2^32 pairs or more) gets 0 blocks: nothing of it is touched.
__global__ __launch_bounds__(256) void membuf_plan_kernel(const uint64_t *__restrict__ buf_offsets,
                                                          const uint64_t *__restrict__ sizes,
                                                          const uint64_t *__restrict__ offsets,
                                                          const uint32_t *__restrict__ seed_index, uint64_t n_seeds,
                                                          uint64_t n, bool decrypt,
                                                          uint64_t *__restrict__ woffs, uint32_t *__restrict__ counts,
                                                          uint32_t *__restrict__ idx, uint64_t *__restrict__ new_sizes)
{
    const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n)
        return;
    const uint64_t off = offsets ? offsets[i] : 0, size = sizes[i];
    const uint64_t start = buf_offsets[i] + off;
    const uint64_t si = seed_index ? uint64_t(seed_index[i]) : (n_seeds == 1 ? 0 : i);
    uint64_t pairs = 0;
    if (!decrypt || size >= off)
        pairs = (((decrypt ? size - off : size + off) >> 3) + 3) >> 1;
    if ((start & 7u) || si >= n_seeds || pairs > 0xFFFFFFFFull)
        pairs = 0;
    woffs[i] = start >> 3;
    counts[i] = uint32_t(pairs);
    idx[i] = uint32_t(si);
    if (!decrypt)
        new_sizes[i] = 16 * pairs + off;
}

__global__ __launch_bounds__(256) void membuf_finish_kernel(const uint32_t *__restrict__ done,
                                                            const uint64_t *__restrict__ offsets, uint64_t n,
                                                            uint64_t *__restrict__ new_sizes)
{
    const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i < n)
        new_sizes[i] = 16 * uint64_t(done[i]) + (offsets ? offsets[i] : 0);
}

int cu_count()
{
    static int n = 0;
    if (n == 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
            n = v;
        else
            n = 256;
    }
    return n;
}

constexpr int kIlp = 2;      // tools/bf_keyed_bench.py, test option "bf_keyed" = 2 runs ILP 1

}  // namespace

namespace brb {

hipError_t launch_blowfish_keyed(const uint64_t *ctxs, const uint32_t *ctx_index, uint64_t *words, const uint64_t *woffs,
                                 const uint32_t *counts, uint64_t n_rec, bool decrypt, uint32_t *blocks_done,
                                 hipStream_t s)
{
    if (n_rec == 0)
        return hipSuccess;
    const uint64_t groups = (n_rec + kSlots - 1) / kSlots;
    const uint64_t cap = uint64_t(cu_count());   // persistent: one workgroup per CU (128 KiB LDS each)
    const unsigned g = unsigned(groups < cap ? groups : cap);
    const int variant = brb_opt::get(brb_opt::kBfKeyed);
#define BRB_KEYED(ILP, DEC, STOP, SPREAD) \
    bf_keyed_kernel<ILP, DEC, STOP, SPREAD><<<g, kRepThreads, 0, s>>>(ctxs, ctx_index, words, woffs, counts, n_rec, blocks_done)
    if (blocks_done)             // the MemBuffer decrypt stop
        BRB_KEYED(kIlp, true, true, true);
    else if (variant == 1) {
        if (decrypt)
            BRB_KEYED(kIlp, true, false, false);
        else
            BRB_KEYED(kIlp, false, false, false);
    } else if (variant == 2) {
        if (decrypt)
            BRB_KEYED(1, true, false, true);
        else
            BRB_KEYED(1, false, false, true);
    } else {
        if (decrypt)
            BRB_KEYED(kIlp, true, false, true);
        else
            BRB_KEYED(kIlp, false, false, true);
    }
#undef BRB_KEYED
    return hipGetLastError();
}

hipError_t launch_membuf_plan(const uint64_t *buf_offsets, const uint64_t *sizes, const uint64_t *offsets,
                              const uint32_t *seed_index, uint64_t n_seeds, uint64_t n, bool decrypt,
                              uint64_t *woffs, uint32_t *counts, uint32_t *idx, uint64_t *new_sizes, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    membuf_plan_kernel<<<unsigned((n + 255) / 256), 256, 0, s>>>(buf_offsets, sizes, offsets, seed_index, n_seeds, n,
                                                                 decrypt, woffs, counts, idx, new_sizes);
    return hipGetLastError();
}

hipError_t launch_membuf_finish(const uint32_t *done, const uint64_t *offsets, uint64_t n, uint64_t *new_sizes,
                                hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    membuf_finish_kernel<<<unsigned((n + 255) / 256), 256, 0, s>>>(done, offsets, n, new_sizes);
    return hipGetLastError();
}

}  // namespace brb
