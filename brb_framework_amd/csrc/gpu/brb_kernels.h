// brb_kernels.h -- internal launchers of the gfx950 crypto kernels (C++ linkage, not exported).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "brb_crypto.h"
#include "brb_gpu_common.h"
#include "pair_fault.h"

namespace brb {

// All pointers are device pointers; launches are asynchronous on `s`.
hipError_t launch_md5_fixed(const uint8_t *data, uint32_t rec_len, uint64_t n_rec, uint8_t *out, hipStream_t s);
hipError_t launch_md5_var(const uint8_t *data, const uint64_t *offs, const uint32_t *lens, uint64_t n_rec,
                          uint8_t *out, hipStream_t s);
hipError_t launch_sha1_fixed(const uint8_t *data, uint32_t rec_len, uint64_t n_rec, uint8_t *out, hipStream_t s);
hipError_t launch_sha1_var(const uint8_t *data, const uint64_t *offs, const uint32_t *lens, uint64_t n_rec,
                           uint8_t *out, hipStream_t s);
// ctx_dev: device copy of BRB_BLOWFISH_CTX (P[18] then S[4][256], 64-bit words)
hipError_t launch_blowfish(const uint64_t *ctx_dev, uint64_t *words, uint64_t n_blocks, bool decrypt, hipStream_t s);
// *first = min(*first, index of the first block (xl, xr) with a zero word); *first preset by the caller
hipError_t launch_first_zero_pair(const uint64_t *words, uint64_t n_blocks, unsigned long long *first, hipStream_t s);

// Blowfish ECB with a context per record (blowfish_keyed_kernels.hip): record i = counts[i] blocks at
// words + woffs[i] (8-byte words), keyed by ctxs[ctx_index ? ctx_index[i] : i] (1042 qwords each).
// blocks_done != nullptr (decrypt only): the MemBuffer stop -- record i is decrypted up to its first
// block with a zero word and blocks_done[i] = the blocks decrypted.
hipError_t launch_blowfish_keyed(const uint64_t *ctxs, const uint32_t *ctx_index, uint64_t *words, const uint64_t *woffs,
                                 const uint32_t *counts, uint64_t n_rec, bool decrypt, uint32_t *blocks_done,
                                 hipStream_t s);
// MemBuffer batch, device mode: buffer i -> woffs[i] (words from data), counts[i] (pairs), idx[i] (its
// seed's context); encrypt also new_sizes[i].  finish (decrypt): new_sizes[i] = 16 done[i] + offsets[i].
hipError_t launch_membuf_plan(const uint64_t *buf_offsets, const uint64_t *sizes, const uint64_t *offsets,
                              const uint32_t *seed_index, uint64_t n_seeds, uint64_t n, bool decrypt, uint64_t *woffs,
                              uint32_t *counts, uint32_t *idx, uint64_t *new_sizes, hipStream_t s);
hipError_t launch_membuf_finish(const uint32_t *done, const uint64_t *offsets, uint64_t n, uint64_t *new_sizes,
                                hipStream_t s);

// MD5 of segment lists (md5_seg_kernels.hip): record r = segments first[r] .. first[r + 1] - 1
hipError_t launch_md5_segments(const uint8_t *data, const uint64_t *soff, const uint32_t *slen, const uint64_t *first,
                               uint64_t n_rec, uint8_t *out, hipStream_t s);

// Streaming digest contexts (digest_stream_kernels.hip): item i acts on context ctx_index ? ctx_index[i] : i
// of ctxs (BRB_MD5_CTX, 168 bytes; sha1: BrbSha1Ctx, 92 bytes; 4-byte aligned).  update: piece i =
// data[offs[i] .. + lens[i]).  final: digests[i] (16 / 20 bytes, any alignment; MD5 only: may be nullptr).
hipError_t launch_digest_stream_init(bool sha1, uint8_t *ctxs, const uint32_t *ctx_index, uint64_t n, hipStream_t s);
hipError_t launch_digest_stream_update(bool sha1, uint8_t *ctxs, const uint32_t *ctx_index, const uint8_t *data,
                                       const uint64_t *offs, const uint32_t *lens, uint64_t n, hipStream_t s);
hipError_t launch_digest_stream_final(bool sha1, uint8_t *ctxs, const uint32_t *ctx_index, uint64_t n, uint8_t *digests,
                                      hipStream_t s);
// segments: item i takes segments first[i] .. first[i + 1] - 1 (segment k = data[soff[k] .. + slen[k])) in order,
// then Final when fin && fin[i] (digests[i] written for those items only; fin nullptr: no item is finalised).
// Grid of ceil(n / 256); always this kernel, whatever the list lengths.
hipError_t launch_digest_stream_segments(bool sha1, uint8_t *ctxs, const uint32_t *ctx_index, const uint8_t *data,
                                         const uint64_t *soff, const uint32_t *slen, const uint64_t *first, uint64_t n,
                                         const uint8_t *fin, uint8_t *digests, hipStream_t s);
// the same for MD5 with segment k taken as BRB_MD5UpdateLowerText when slow[k] != 0 (slow nullptr: every segment)
hipError_t launch_md5_stream_segments_lower(uint8_t *ctxs, const uint32_t *ctx_index, const uint8_t *data,
                                            const uint64_t *soff, const uint32_t *slen, const uint8_t *slow,
                                            const uint64_t *first, uint64_t n, const uint8_t *fin, uint8_t *digests,
                                            hipStream_t s);

// MD5 of lower-cased keys (md5_lower_kernels.hip): key r = data[offs[r] .. + lens[r]) at any alignment; digests[r]
// (16 bytes) and / or strings[r] (33 bytes: 32 hex characters and a NUL), rows at any alignment, either may be nullptr
hipError_t launch_md5_lower(const uint8_t *data, const uint64_t *offs, const uint32_t *lens, uint64_t n, uint8_t *digests,
                            uint8_t *strings, hipStream_t s);

// MetaDataUnpack of whole packs (metadata_kernels.hip): pack r = data[offs[r] .. + lens[r])
hipError_t launch_metadata_unpack(const uint8_t *data, const uint64_t *offs, const uint32_t *lens, uint64_t n,
                                  BRB_MetaDataUnpackInfo *info, hipStream_t s);
// ... and the item table (BRB_MetaDataUnpackItemsBatch): pack r's MetaDataItemAdd calls in slots first[r] ..
// first[r + 1] - 1 of ioff / ilen / iid / isub, their number in added[r]; item offsets are data_base + the
// offset from `data` (host mode stages a span of the caller's buffer).  The same kernels and test options.
hipError_t launch_metadata_unpack_items(const uint8_t *data, uint64_t data_base, const uint64_t *offs, const uint32_t *lens,
                                        uint64_t n, BRB_MetaDataUnpackInfo *info, uint64_t *ioff, uint32_t *ilen,
                                        uint64_t *iid, uint64_t *isub, const uint64_t *first, uint32_t *added, hipStream_t s);

// MetaDataPack of whole packs (metadata_pack_kernels.hip): pack p = items first[p] .. first[p + 1] - 1, item k =
// data[ioff[k] .. + ilen[k]) with iid[k], isub[k]; written at out + ooff[p]
hipError_t launch_metadata_pack(const uint8_t *data, const uint64_t *ioff, const uint32_t *ilen, const uint64_t *iid,
                                const uint64_t *isub, const uint64_t *first, uint64_t n_packs, uint8_t *out,
                                const uint64_t *ooff, hipStream_t s);

// base64 (base64_kernels.hip)
hipError_t launch_b64_encode(const uint8_t *in, const uint64_t *offs, const uint32_t *lens, uint64_t n, uint8_t *out,
                             const uint64_t *ooffs, uint64_t mean_len, hipStream_t s);
hipError_t launch_b64_decode(const uint8_t *in, const uint64_t *offs, const uint32_t *lens, uint64_t n, uint8_t *out,
                             const uint64_t *ooffs, uint32_t *olens, uint64_t mean_len, hipStream_t s);

// RC4, RC4+MD5 frame and RC4+MD5 open (rc4_kernels.hip, rc4_list_kernels.hip, rc4_mixed_kernels.hip): one
// descriptor for every launch of the family.  Which kernel runs follows from the fields that are set:
//   kinds           the mixed kernel: stream i is walked as the list kernel of kinds[i] walks it
//   first, no kinds the list kernel of `kind`: a buffer list per stream
//   neither         the single-buffer kernels of `kind` (wave pair or lone wave, by the test options)
// The list and mixed kernels and the lone single-buffer kernels are lone waves: no pair fault word is
// involved.  The wave-pair kernels report into the word armed on the launching thread (pair_fault.h).
struct Rc4Launch {
    int kind = BRB_RC4_KIND_CRYPT;     // one BRB_RC4_KIND_* for the whole launch (not read when kinds is set)
    const uint8_t *kinds = nullptr;    // a BRB_RC4_KIND_* per stream; non-NULL selects the mixed kernel
    uint8_t *states = nullptr;         // 264-byte BRB_RC4_State records, updated in place
    const uint32_t *sidx = nullptr;    // stream i uses states[sidx ? sidx[i] : i] (a connection table, the
                                       // transform batcher's indirection)
    const uint8_t *in = nullptr;       // inputs: buffer k = in[offs[k] .. + lens[k])
    uint8_t *out = nullptr;            // outputs (frames for FRAME: lens[k] + BRB_RC4MD5_HEADER bytes each)
    const uint64_t *offs = nullptr;    // offs, lens, ooffs, salts and valid are indexed by buffer
    const uint32_t *lens = nullptr;
    const uint64_t *ooffs = nullptr;   // output offsets in `out`; NULL = out mirrors in (offs), allowed for
                                       // CRYPT and OPEN without kinds; FRAME: the frame offsets
    const uint64_t *salts = nullptr;   // read for FRAME buffers only
    const uint64_t *first = nullptr;   // stream i owns buffers first[i] .. first[i + 1] - 1 (n + 1 non-decreasing
                                       // entries): its state is loaded once, the buffers walked in order, each
                                       // as a single-buffer launch treats its one buffer, the state stored once.
                                       // NULL = one buffer per stream, buffer i = stream i
    uint64_t n = 0;                    // streams
    uint8_t *valid = nullptr;          // written for OPEN buffers only
    bool sector_out = true;            // single-buffer lone CRYPT: write whole aligned 64-byte sectors
                                       // (brb_io::SectorSnk), the default for HBM and host outputs alike since
                                       // the session-4 generator (rc4_kernels.hip); false = per-stream 16-byte
                                       // pieces (Snk)
};
hipError_t launch_rc4_single(const Rc4Launch &l, hipStream_t s);   // rc4_kernels.hip
hipError_t launch_rc4_list(const Rc4Launch &l, hipStream_t s);     // rc4_list_kernels.hip
hipError_t launch_rc4_mixed(const Rc4Launch &l, hipStream_t s);    // rc4_mixed_kernels.hip
// the one entry point of the callers
inline hipError_t launch_rc4(const Rc4Launch &l, hipStream_t s)
{
    return l.kinds ? launch_rc4_mixed(l, s) : l.first ? launch_rc4_list(l, s) : launch_rc4_single(l, s);
}

// Key setup (keysetup_kernels.hip): key i = keys[koffs[i] .. + klens[i]).
// RC4: the zeroed-then-BRB_RC4_Init state of key i is written (all 264 bytes) to states[slots ? slots[i] : i],
// and, when second != 0, also `second` bytes after it (the transform batcher's write-state table).
hipError_t launch_rc4_keysetup(uint8_t *states, const uint8_t *keys, const uint64_t *koffs, const uint32_t *klens,
                               uint64_t n, hipStream_t s, const uint32_t *slots = nullptr, uint64_t second = 0);
// Blowfish: ctxs[i] (1042 qwords, 8-byte aligned) = BRB_Blowfish_Init of key i
hipError_t launch_blowfish_keysetup(uint64_t *ctxs, const uint8_t *keys, const uint64_t *koffs, const uint32_t *klens,
                                    uint64_t n, hipStream_t s);

}  // namespace brb
