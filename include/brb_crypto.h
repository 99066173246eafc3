/*
 * brb_crypto.h -- C ABI of libbrb_crypto_gpu.so, the MI355X-native replacement for
 * libbrb_core/crypto (BrByte brb_framework @ 2024_10_08).
 *
 * Two surfaces:
 *
 *  1. COMPAT (drop-in): the reference's crypto prototypes with the same names, argument types,
 *     struct layouts and side effects, so the callers in libbrb_core/comm and libbrb_core/data link
 *     unchanged (list in INTEGRATION.md).  They run on the calling CPU thread: a single streaming
 *     context is a serial chain and does not belong on a GPU.
 *
 *  2. BATCH (new): many independent records per call, executed by hand-written gfx950 HIP
 *     kernels.  This is the hot path.  It never falls back to a CPU implementation: if no HIP
 *     device is usable the call returns 0 and BRB_CryptoGPU_LastError() says why.
 *
 * LP64 is assumed, exactly as the reference assumes it (`unsigned long` = 8 bytes inside
 * BRB_BLOWFISH_CTX).
 */
#ifndef BRB_CRYPTO_H
#define BRB_CRYPTO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ============================================================================================ */
/* 1. COMPAT SURFACE                                                                              */
/* ============================================================================================ */
/* A translation unit that already includes the reference's libbrb_data.h (guard LIBBRB_DATA_H_)
 * gets these types and prototypes from there; the definitions below are the same ABI. */
#ifndef LIBBRB_DATA_H_

/* ---- MD5 -- replaces libbrb_core/crypto/md5.c; prototypes libbrb_data.h:862-869 ------------ */
#define MD5_DIGEST_LENGTH 16                      /* libbrb_data.h:852 */

typedef struct _BRB_MD5_CTX {                     /* libbrb_data.h:854-860, sizeof == 168 */
    uint32_t buf[4];
    uint32_t bytes[2];
    uint32_t in[16];
    unsigned char digest[16];
    unsigned char string[64];                     /* lowercase hex + NUL after Final */
} BRB_MD5_CTX;

void BRB_MD5Init(BRB_MD5_CTX *ctx);                                             /* md5.c:38  */
void BRB_MD5UpdateBig(BRB_MD5_CTX *ctx, const void *_buf, unsigned long len);   /* md5.c:49  */
void BRB_MD5Update(BRB_MD5_CTX *ctx, const void *_buf, unsigned long len);      /* md5.c:72  */
/* md5.c:112.  The reference lowercases into a 128-byte stack buffer and overflows it when
 * key_sz > 128; this version lowercases in 128-byte pieces (same digest, no overflow). */
void BRB_MD5UpdateLowerText(BRB_MD5_CTX *md5_context, char *key_ptr, int key_sz);
void BRB_MD5Final(BRB_MD5_CTX *ctx);                                            /* md5.c:134 */
void BRB_MD5Transform(BRB_MD5_CTX *ctx);                                        /* md5.c:170 */
void BRB_MD5LateInitDigestString(BRB_MD5_CTX *ret);                             /* md5.c:255 */
void BRB_MD5ToStr(unsigned char *bin_digest, unsigned char *ret_buf_str);       /* md5.c:264 */

/* ---- SHA-1 -- replaces libbrb_core/crypto/sha1.c; prototypes libbrb_data.h:1947-1951 ------- */
typedef struct {                                  /* libbrb_data.h:1937-1943, sizeof == 92 */
    uint32_t state[5];
    uint32_t count[2];
    uint8_t buffer[64];
} BrbSha1Ctx;

#define BRB_SHA1_DIGEST_SIZE 20                   /* libbrb_data.h:1945 */

void BrbSha1_Init(BrbSha1Ctx *context);                                          /* sha1.c:132 */
/* sha1.c:143.  Like the reference (SHA1HANDSOFF undefined, sha1.c:84-90) every full 64-byte block
 * transformed directly from `data` is overwritten with message-schedule words W[64..79]. */
void BrbSha1_Update(BrbSha1Ctx *context, const uint8_t *data, const size_t len);
void BrbSha1_Final(BrbSha1Ctx *context, uint8_t digest[BRB_SHA1_DIGEST_SIZE]);   /* sha1.c:171 */
void BrbSha1_Transform(uint32_t state[5], const uint8_t buffer[64]);             /* sha1.c:75  */
int BrbSha1_Do(const uint8_t *in_ptr, int in_len, char *dig_str);                /* sha1.c:203 */

/* ---- Blowfish -- replaces libbrb_core/crypto/blowfish.c; prototypes libbrb_data.h:881-883 -- */
typedef struct _BRB_BLOWFISH_CTX {                /* libbrb_data.h:876-879, sizeof == 8336 */
    unsigned long P[16 + 2];
    unsigned long S[4][256];
} BRB_BLOWFISH_CTX;

void BRB_Blowfish_Init(BRB_BLOWFISH_CTX *ctx, unsigned char *key, int keyLen);         /* :382 */
void BRB_Blowfish_Encrypt(BRB_BLOWFISH_CTX *ctx, unsigned long *xl, unsigned long *xr); /* :312 */
void BRB_Blowfish_Decrypt(BRB_BLOWFISH_CTX *ctx, unsigned long *xl, unsigned long *xr); /* :347 */

/* ---- RC4 -- replaces libbrb_core/crypto/rc4.c; prototypes libbrb_data.h:899-900 ------------ */
typedef struct _BRB_RC4_State {                   /* libbrb_data.h:887-897, sizeof == 264 */
    unsigned char perm[256];
    unsigned char index1;
    unsigned char index2;
    struct {
        unsigned int initialized : 1;
    } flags;
} BRB_RC4_State;

void BRB_RC4_Init(BRB_RC4_State *state, const unsigned char *key, int keylen);            /* rc4.c:40 */
void BRB_RC4_Crypt(BRB_RC4_State *state, const unsigned char *inbuf, unsigned char *outbuf,
                   int buflen);                                                          /* rc4.c:64 */
#endif /* LIBBRB_DATA_H_ */

/* ============================================================================================ */
/* 2. BATCH SURFACE (GPU)                                                                         */
/* ============================================================================================ */

/* Return codes follow the reference's transform-hook convention (ev_kq_aio_transform.c:52-57):
 *   1  done
 *   0  not done: no usable HIP device, device error, or unsupported request
 *      (BRB_CryptoGPU_LastError() has the reason; nothing was computed on the CPU)
 *  -1  bad arguments (NULL pointer where one is required, length out of range)         */
#define BRB_BATCH_OK        1
#define BRB_BATCH_NOT_DONE  0
#define BRB_BATCH_BADARG   (-1)
#define BRB_BATCH_DROPPED  (-2)   /* transform batcher: a round was dropped (see Flush)         */
#define BRB_BATCH_PARTIAL  (-3)   /* all-devices transform batcher: some parts delivered their
                                     buffers, others could not select their device and keep their
                                     rounds pending (see Flush)                                  */
#define BRB_BATCH_FAULT    (-4)   /* segment digests, MetaData unpack, RC4 pass, RC4+MD5 frame /
                                     open: a wave-pair kernel's bounded wait on its partner wave
                                     gave up (a protocol fault; never a hang).  The call's outputs,
                                     and for RC4 the states, are wrong.  Returned by synchronous
                                     calls; a device-mode BRB_BATCH_ASYNC call cannot know yet and
                                     returns 1: BRB_CryptoGPU_AsyncFaultCheck() reports it after the
                                     caller has synchronised its stream.  A transform batcher round
                                     with a fault is dropped (Flush returns BRB_BATCH_DROPPED).
                                     Test option pair_stall injects one.                         */

/* flags */
#define BRB_BATCH_HOST      0x0u   /* pointers are host memory: copied in and out by the call      */
#define BRB_BATCH_DEVICE    0x1u   /* every pointer (data, offsets, lengths, digests, ctx, words)
                                      is device memory (HBM-resident); nothing crosses PCIe       */
#define BRB_BATCH_ASYNC     0x2u   /* with BRB_BATCH_DEVICE: enqueue on `hip_stream` and return
                                      without waiting; the caller synchronises the stream and then
                                      calls BRB_CryptoGPU_AsyncFaultCheck() (same thread) before it
                                      trusts the outputs of wave-pair calls (BRB_BATCH_FAULT)     */
#define BRB_BATCH_ALL_DEVICES 0x4u /* host mode only (every batch call except MemBuffer):
                                      split the records (blocks, streams, packs) into contiguous
                                      ranges [g*n/G, (g+1)*n/G), one per visible device g < G, run
                                      them concurrently and return when all are done (SURVEY §8(e):
                                      no collective); the RC4 states go with their streams.  Calls
                                      that write a byte span back (RC4, frames, base64 outputs, MetaData packs)
                                      split only when the ranges' spans do not interleave across
                                      parts (ranges in submission order); otherwise they run on the
                                      calling thread's device.  With BRB_BATCH_DEVICE: -1.           */

/* Device mode: `hip_stream` is a hipStream_t (NULL = the legacy default stream of the current
 * device) and the work runs on the caller's current HIP device (BRB_CryptoGPU_SetDevice,
 * hipSetDevice or torch.cuda.set_device).
 * DEVICE-MODE CONTRACT: the library cannot see how large a device allocation is, so in device mode
 * every offset, length and count is the caller's promise that the range lies inside its allocation
 * (data, offsets/lengths arrays, digests, outputs, states).  A range past the end is not detected
 * and not answered with -1: the kernel's access faults and the HIP context is lost ("illegal memory
 * access", every later call on that device fails).  Host mode copies exactly the ranges given, so
 * there a bad range is an ordinary out-of-bounds read of the caller's host memory.  Host mode: the call runs on the caller's current device
 * (or on every device with BRB_BATCH_ALL_DEVICES), copies straight from and to the caller's memory
 * (pageable or page-locked) in chunks so that copies in both directions overlap the kernels, and
 * returns when the results are in host memory; `hip_stream` is not used. */

/* GRAPH CAPTURE (hipStreamBeginCapture, torch.cuda.graph; tests/test_graph_capture.py): where a call
 * below says "graph-capturable", this is what it means.
 *   - Only BRB_BATCH_DEVICE | BRB_BATCH_ASYNC calls may be made on a capturing stream: they enqueue
 *     their kernels on `hip_stream` and nothing else.  Device mode without ASYNC synchronises the
 *     stream, host mode copies and synchronises, the MemBuffer calls ignore ASYNC, and a transform
 *     batcher owns streams and events: each of these on a capturing stream is a caller error and
 *     invalidates the capture.
 *   - Each kernel has run once eagerly before its first capture (the runtime loads a code object on a
 *     kernel's first launch): make one uncaptured call of the same kind first.
 *   - Fixed when the call is captured: the counts (n, rec_len, n_ctx), every pointer, the kernel the
 *     launcher chose from them, and the test options.  Read from device memory afresh by every
 *     replay: the data, offsets, lengths, segment / buffer / item lists, salts, `final` and
 *     `seg_lower` masks, and the RC4 states and streaming contexts, which advance with every replay
 *     as they would with every call.  A replay's ranges must lie inside the allocations like a call's.
 *   - A captured call of a wave-pair kernel (the calls that can return BRB_BATCH_FAULT) reports into
 *     the async fault word of the thread that CAPTURED it, whichever thread replays the graph: that
 *     thread calls BRB_CryptoGPU_AsyncFaultCheck() after a replay has been synchronised; a replaying
 *     thread's own check says nothing about the replay.  The word is allocated on a thread's first
 *     such call, inside a capture too (the one allocation is made with the thread's capture mode
 *     exchanged for the relaxed one; if it fails, the call returns 0 with the reason and launches
 *     nothing).  It is freed when that thread exits or calls BRB_CryptoGPU_ThreadCleanup(): the
 *     capturing thread does neither while the graph can still be replayed. */

/* MD5 of n_rec records of rec_len bytes each, stored back to back: record i is
 * data[i*rec_len .. (i+1)*rec_len).  digests[i] = BRB_MD5Init/Update/Final of record i. */
int BRB_MD5BatchFixed(const void *data, uint32_t rec_len, uint64_t n_rec,
                      unsigned char (*digests)[16], unsigned flags, void *hip_stream);

/* MD5 of n_rec records of arbitrary byte offset and length (record i = data[offsets[i] ..
 * offsets[i] + lengths[i])).  Records may overlap and need no alignment. */
int BRB_MD5Batch(const void *data, const uint64_t *offsets, const uint32_t *lengths,
                 uint64_t n_rec, unsigned char (*digests)[16], unsigned flags, void *hip_stream);

/* MD5 of segment lists: record i is the concatenation of segments
 * rec_first_seg[i] .. rec_first_seg[i + 1] - 1 (rec_first_seg has n_rec + 1 entries), segment k =
 * data[seg_offsets[k] .. + seg_lengths[k]).  digests[i] = BRB_MD5Init, BRB_MD5UpdateBig per segment,
 * BRB_MD5Final -- the MetaData pack digest of meta_data.c:397-433 with one record per MetaData. */
int BRB_MD5BatchSegments(const void *data, const uint64_t *seg_offsets, const uint32_t *seg_lengths,
                         const uint64_t *rec_first_seg, uint64_t n_rec, unsigned char (*digests)[16],
                         unsigned flags, void *hip_stream);

/* MetaData packs (the format of meta_data.c:104-140, libbrb_data.h:291-330, LP64):
 * a 64-byte header {int version; int item_count; unsigned long size; "BRB_META"; 16-byte MD5 of
 * the items' data; 24 reserved bytes}, then per item {unsigned long item_id, item_sub_id, sz;
 * sz data bytes; 0x1F}.  BRB_MetaDataUnpackBatch checks pack i = data[offsets[i] .. + lengths[i])
 * exactly as MetaDataUnpack (meta_data.c:145-328) checks a MemBuffer holding it at offset 0, and
 * writes the MetaDataUnpackerInfo fields (libbrb_data.h:332-344) plus the number of items unpacked:
 * error_code is a BRB_METADATA_UNPACK_* value (the reference's MetaDataUnpackReturnCode), SUCCESS
 * only if every canary holds and the MD5 of the items read equals the header's digest.  Quirks kept:
 * an item is only read with sizeof(MetaDataItem) = 32 bytes left (24 are its header), so a pack whose
 * last item holds 0..6 data bytes reports NEED_MORE_DATA_METAITEM; the walk stops after item_count
 * items or at the pack's end, whichever comes first.  Where the reference reads past its buffer
 * (packs shorter than the header, a size field beyond the pack), bytes past the pack read as 0 and
 * an item larger than the whole pack reports NEED_MORE_DATA_OBJECT without being read. */
#define BRB_METADATA_UNPACK_FAILED_INVALID_HEADER_MAGIC 0
#define BRB_METADATA_UNPACK_FAILED_CORRUPTED_CANARY 3
#define BRB_METADATA_UNPACK_FAILED_DIGEST_INVALID 4
#define BRB_METADATA_UNPACK_FAILED_NEED_MORE_DATA_METAITEM 5
#define BRB_METADATA_UNPACK_FAILED_NEED_MORE_DATA_OBJECT 6
#define BRB_METADATA_UNPACK_SUCCESS 7
#define BRB_METADATA_HEADER_SIZE 64
#define BRB_METADATA_ITEM_RAW_SIZE 24
typedef struct BRB_MetaDataUnpackInfo {
    int32_t error_code;       /* MetaDataUnpackReturnCode */
    uint32_t item_count;      /* items whose canary was checked before error_code was decided */
    uint64_t cur_offset;      /* MetaDataUnpackerInfo.cur_offset / cur_remaining / cur_needed */
    uint64_t cur_remaining;
    uint64_t cur_needed;
} BRB_MetaDataUnpackInfo;
int BRB_MetaDataUnpackBatch(const void *data, const uint64_t *offsets, const uint32_t *lengths, uint64_t n_packs,
                            BRB_MetaDataUnpackInfo *info, unsigned flags, void *hip_stream);

/* BRB_MetaDataUnpackBatch plus the item table MetaDataUnpack builds while it checks: one entry per
 * MetaDataItemAdd call (meta_data.c:246-248), in the reference's order -- every item that passed both
 * bounds checks (32 bytes left for its header; sz + 1 bytes left for its data, and sz <= the pack's
 * length), whatever happens next: an item whose canary then proves corrupted is in the table, and so
 * are all items of a pack whose digest then fails; the item at which a NEED_MORE_DATA_* code was
 * decided is not.  info[p] is what BRB_MetaDataUnpackBatch writes for the pack, field for field.
 * items_added[p] is the number of such calls, = info[p].item_count + (error_code == CORRUPTED_CANARY),
 * 0 for a bad magic.  Pack p owns table slots pack_first_slot[p] .. pack_first_slot[p+1]-1 (n_packs + 1
 * entries, non-decreasing) of the four arrays; its j-th item, for j below its slot count, is written
 * to slot s = pack_first_slot[p] + j:
 *   item_offsets[s]  the offset in `data` of the item's first data byte (the reference's ptr; valid
 *                    for sz == 0 too), item_lengths[s] = sz,
 *   item_ids[s], item_sub_ids[s]  its two unsigned long fields (bytes past the pack read as 0).
 * Items past the slot count are counted, not stored: items_added[p] > the slot count says so, and
 * (lengths[p] - 64) / 25 slots are always enough for a pack of at least 64 bytes (a shorter one adds
 * at most one item: the zero bytes past its end, read as an empty item whose canary is missing).
 * Slots j >= items_added[p] keep their values, in both modes, and no slot of another pack is
 * touched.  The arrays have the element
 * types of BRB_MetaDataPackBatch and BRB_MD5BatchSegments: item_offsets / item_lengths / item_ids /
 * item_sub_ids with pack_first_slot as pack_first_item (exact slot counts) repack, and item_offsets /
 * item_lengths are segment lists, with nothing leaving HBM in device mode.
 * Flags, return codes, hip_stream and the device-mode contract are BRB_MetaDataUnpackBatch's (device
 * mode checks NULL pointers, the count and the flags, and allocates nothing).  Host mode: -1 for a
 * pack_first_slot that decreases; the four arrays are staged over slots [pack_first_slot[0],
 * pack_first_slot[n_packs]) in both directions.  BRB_BATCH_ALL_DEVICES always splits (contiguous pack
 * ranges own contiguous slot ranges).  After BRB_BATCH_FAULT the table is unspecified. */
int BRB_MetaDataUnpackItemsBatch(const void *data, const uint64_t *offsets, const uint32_t *lengths, uint64_t n_packs,
                                 BRB_MetaDataUnpackInfo *info, uint64_t *item_offsets, uint32_t *item_lengths,
                                 uint64_t *item_ids, uint64_t *item_sub_ids, const uint64_t *pack_first_slot,
                                 uint32_t *items_added, unsigned flags, void *hip_stream);

/* MetaDataPack (meta_data.c:104-140, digest :397-433) for n_packs MetaDatas.  Pack p holds items
 * pack_first_item[p] .. pack_first_item[p+1]-1 (n_packs + 1 entries, non-decreasing); item k =
 * data[item_offsets[k] .. + item_lengths[k]) with item_ids[k], item_sub_ids[k].  Pack p is written
 * at out + out_offsets[p] and is BRB_METADATA_HEADER_SIZE + sum(item_lengths[k] + 25) bytes long:
 * the header above (version 0, (int) item count, size = sum(item_lengths[k] + 25), "BRB_META", the
 * MD5 of the items' data in order -- BRB_MD5Init, one BRB_MD5UpdateBig per item, BRB_MD5Final -- and
 * 24 zero bytes), then per item its three unsigned longs, its data and the 0x1F canary.  A pack with
 * no items is the header alone, with the MD5 of the empty message; the address of a zero-length item
 * is never read.  Exactly the pack's bytes are written: packs may lie back to back at any byte
 * offset of out, and bytes between packs keep their values.  Packs must not overlap each other or
 * the items they (or other packs of the call) are built from.  A pack holds at most INT32_MAX
 * items, and in host mode at most 4 GiB - 1 bytes, the unpack call's length (host mode: -1
 * otherwise; pack_first_item that decreases: -1; device mode validates nothing).  Host mode stages the span
 * of out that the packs cover in both directions.  BRB_BATCH_ALL_DEVICES splits the packs into
 * contiguous ranges only when those ranges' output spans do not interleave (as the RC4 and base64
 * calls); otherwise the call runs on the calling thread's device.  One pass on the GPU: every item
 * byte is read from HBM once and feeds both the digest and the pack. */
int BRB_MetaDataPackBatch(const void *data, const uint64_t *item_offsets, const uint32_t *item_lengths,
                          const uint64_t *item_ids, const uint64_t *item_sub_ids,
                          const uint64_t *pack_first_item, uint64_t n_packs,
                          void *out, const uint64_t *out_offsets, unsigned flags, void *hip_stream);

/* SHA-1 batches: digests[i] = BrbSha1_Do(record i) (20 raw big-endian bytes).  Unlike
 * BrbSha1_Update the batch surface never writes into the input records. */
int BrbSha1_BatchFixed(const void *data, uint32_t rec_len, uint64_t n_rec,
                       uint8_t (*digests)[20], unsigned flags, void *hip_stream);
int BrbSha1_Batch(const void *data, const uint64_t *offsets, const uint32_t *lengths,
                  uint64_t n_rec, uint8_t (*digests)[20], unsigned flags, void *hip_stream);

/* ---- Streaming MD5 / SHA-1 contexts as a batch ------------------------------------------------
 * The compat digests are streaming contexts (BRB_MD5Init / Update / UpdateBig / Final, BrbSha1_Init /
 * Update / Final): a message arrives over several event-loop rounds, a file is digested in pieces.
 * These calls keep a table of such contexts (n_ctx contiguous BRB_MD5_CTX of 168 bytes, or BrbSha1Ctx
 * of 92 bytes) and act on n of them per call, one GPU lane per context, bit-compatible with the compat
 * structs: a context may move freely between BRB_MD5Update / BrbSha1_Update on the host and these
 * calls, and with BRB_BATCH_DEVICE the table lives in HBM across calls (as the RC4 states do).
 *   Item i acts on ctxs[ctx_index ? ctx_index[i] : i].  A context may be named AT MOST ONCE per call:
 *   two pieces of one chain in one launch is a race (a chain's pieces go in consecutive calls, or as
 *   one item's segment list in BRB_MD5UpdateSegmentsBatch / BrbSha1_UpdateSegmentsBatch below).
 *   Piece i (Update) = data[offsets[i] .. + lengths[i]), at any byte alignment; pieces may overlap
 *   each other; data is never written (unlike BrbSha1_Update, which rewrites its input blocks).
 * Init writes exactly what BRB_MD5Init / BrbSha1_Init write -- the state words and the two counters --
 *   and leaves every other byte of the struct as it was.
 * Update leaves the DEFINED part of the context as BRB_MD5Update(&ctx, piece, len) (the same context as
 *   BRB_MD5UpdateBig: one call for both) / BrbSha1_Update do.  The defined part is, for MD5, buf[4],
 *   bytes[2] and the first bytes[0] & 63 bytes of in; for SHA-1, state[5], count[2] and the first
 *   (count[0] >> 3) & 63 bytes of buffer.  The counters follow the reference's own arithmetic: MD5
 *   carries from bytes[0] into bytes[1]; SHA-1 adds len << 3 to count[0], carries when the 32-bit sum is
 *   below the untruncated len << 3 (the spurious carry of sha1.c:151 for len >= 2^29 included), then
 *   adds len >> 29 to count[1].  Bytes of in / buffer PAST the buffered count are UNSPECIFIED after
 *   Update: they may differ from what the compat call leaves there.  No later
 *   call, host or batch, reads them before overwriting them.  MD5's digest and string are not touched.
 *   A piece of length 0 changes nothing, and its offset need not be memory.
 * MD5 Final = BRB_MD5Final: buf is the final state, digest its 16 bytes, string[0 .. 33) the lowercase
 *   hex and its NUL, in the last block the call transformed (the padded block; 14 zero words and the bit
 *   count when the padding took a block of its own), so the whole struct is the reference's byte for
 *   byte; string[33 .. 64) and bytes are untouched; digests[i], when digests is not NULL, gets the same
 *   16 bytes, in item order.
 * SHA-1 Final = BrbSha1_Final: 20 big-endian bytes to digests[i] (required), the whole context zeroed.
 * Flags, return codes, hip_stream and the device-mode contract are BRB_MD5Batch's.  n == 0 returns 1.
 * BRB_BATCH_DEVICE (optionally BRB_BATCH_ASYNC): ctxs, ctx_index, data, offsets, lengths and digests
 * are device memory, ctxs 4-byte aligned; nothing is allocated (with ASYNC graph-capturable: GRAPH
 * CAPTURE above) and nothing is
 * validated beyond NULL pointers and the item count.  BRB_BATCH_HOST returns -1 with a reason, and
 * writes nothing, for: a NULL required pointer (ctx_index may be NULL; data may be NULL only when every
 * length is 0; MD5's digests may be NULL); ctx_index[i] >= n_ctx; a NULL ctx_index with n > n_ctx; a
 * context named twice; more items than a launch takes; BRB_BATCH_ALL_DEVICES with BRB_BATCH_DEVICE.
 * Host mode stages only the contexts the items name (gathered in, scattered back: the rest of the
 * table is neither read nor written) and the span of the pieces.  BRB_BATCH_ALL_DEVICES (host mode)
 * splits the items into contiguous ranges, always: the contexts go with their items, and nothing is
 * written back but contexts and digests.  No wave-pair kernel: BRB_BATCH_FAULT never occurs.  No CPU
 * fallback: without a usable device the calls return 0 with a LastError and write nothing. */
int BRB_MD5InitBatch(BRB_MD5_CTX *ctxs, uint64_t n_ctx, const uint32_t *ctx_index, uint64_t n,
                     unsigned flags, void *hip_stream);
int BRB_MD5UpdateBatch(BRB_MD5_CTX *ctxs, uint64_t n_ctx, const uint32_t *ctx_index,
                       const void *data, const uint64_t *offsets, const uint32_t *lengths, uint64_t n,
                       unsigned flags, void *hip_stream);
int BRB_MD5FinalBatch(BRB_MD5_CTX *ctxs, uint64_t n_ctx, const uint32_t *ctx_index, uint64_t n,
                      unsigned char (*digests)[16], unsigned flags, void *hip_stream);
int BrbSha1_InitBatch(BrbSha1Ctx *ctxs, uint64_t n_ctx, const uint32_t *ctx_index, uint64_t n,
                      unsigned flags, void *hip_stream);
int BrbSha1_UpdateBatch(BrbSha1Ctx *ctxs, uint64_t n_ctx, const uint32_t *ctx_index,
                        const void *data, const uint64_t *offsets, const uint32_t *lengths, uint64_t n,
                        unsigned flags, void *hip_stream);
int BrbSha1_FinalBatch(BrbSha1Ctx *ctxs, uint64_t n_ctx, const uint32_t *ctx_index, uint64_t n,
                       uint8_t (*digests)[20], unsigned flags, void *hip_stream);

/* Segment lists per context and a fused Final: one call in which item i advances its context by a
 * LIST of segments and is then, optionally, finalised.  One event-loop round delivers several buffers
 * of one connection, a MetaData's items are scattered in memory (Init, one UpdateBig per item, Final),
 * and in the same round some messages end while others go on: this call takes such a round in one
 * launch, each context read and written once.  One segment and no final is UpdateBatch; no segments
 * and final is FinalBatch; an Init'd context, segments and final is BRB_MD5BatchSegments.
 *   Item i acts on ctxs[ctx_index ? ctx_index[i] : i]; a context is still named AT MOST ONCE per call.
 *   Item i's segments are item_first_seg[i] .. item_first_seg[i + 1] - 1 (n + 1 entries, non-decreasing,
 *   as rec_first_seg of BRB_MD5BatchSegments).  Segment k = data[seg_offsets[k] .. + seg_lengths[k]) at
 *   any byte alignment; segments may overlap; data is never written; the offset of an empty segment
 *   need not be memory.
 * The result for item i is exactly what the compat functions leave after BRB_MD5UpdateBig (SHA-1:
 *   BrbSha1_Update) once per segment, in order, and then, if final && final[i], BRB_MD5Final /
 *   BrbSha1_Final -- "exactly" in the defined part that Update above documents: state, counters and the
 *   buffered bytes; bytes of the block buffer past them stay unspecified.  The counters advance once
 *   PER SEGMENT with the reference's own arithmetic, so SHA-1's spurious carry is per segment, as it is
 *   per BrbSha1_Update call.
 * An item with final[i] != 0.  MD5: buf, in, digest and string[0 .. 33) are as BRB_MD5Final leaves them,
 *   bytes as the segments advanced it, string[33 .. 64) untouched; digests[i] is written when digests is
 *   not NULL.  SHA-1: digests[i] is written (digests is required whenever final is not NULL) and the
 *   whole context is zeroed.
 * An item with final[i] == 0 leaves digests[i] untouched, in host mode too.  An item with no bytes (no
 *   segments, or only empty ones) and no final leaves its context untouched.  final == NULL: no item is
 *   finalised and digests is not used.  n == 0 returns 1.
 * Flags, return codes, hip_stream and the device-mode contract are BRB_MD5UpdateBatch's.
 * BRB_BATCH_DEVICE validates nothing beyond NULL pointers, the item count and the flags; ctxs is 4-byte
 * aligned; nothing is allocated (with ASYNC graph-capturable: GRAPH CAPTURE above).  BRB_BATCH_HOST
 * returns -1 with a reason, and writes
 * nothing, for: a NULL required pointer (data may be NULL only when every named segment is empty;
 * ctx_index, final and MD5's digests may be NULL); ctx_index[i] >= n_ctx; a NULL ctx_index with
 * n > n_ctx; a context named twice; item_first_seg that decreases; a segment range that wraps; more
 * items than a launch takes; BRB_BATCH_ALL_DEVICES with BRB_BATCH_DEVICE.  Host mode stages the named
 * contexts (gathered in, scattered back on success), the span of the named segments, and the digests in
 * both directions.  BRB_BATCH_ALL_DEVICES splits the items into contiguous ranges, always; the contexts
 * and the segment ranges go with their items.  No wave-pair kernel: BRB_BATCH_FAULT never occurs.  No
 * CPU fallback: without a usable device the calls return 0 with a LastError and write nothing. */
int BRB_MD5UpdateSegmentsBatch(BRB_MD5_CTX *ctxs, uint64_t n_ctx, const uint32_t *ctx_index,
                               const void *data, const uint64_t *seg_offsets, const uint32_t *seg_lengths,
                               const uint64_t *item_first_seg, uint64_t n, const uint8_t *final,
                               unsigned char (*digests)[16], unsigned flags, void *hip_stream);
int BrbSha1_UpdateSegmentsBatch(BrbSha1Ctx *ctxs, uint64_t n_ctx, const uint32_t *ctx_index,
                                const void *data, const uint64_t *seg_offsets, const uint32_t *seg_lengths,
                                const uint64_t *item_first_seg, uint64_t n, const uint8_t *final,
                                uint8_t (*digests)[20], unsigned flags, void *hip_stream);

/* ---- BRB_MD5UpdateLowerText as a batch: case-insensitive keys -----------------------------------
 * BRB_MD5UpdateLowerText (md5.c:112-132) feeds a context the lower-cased copy of a key: host names,
 * header names, the case-insensitive half of a composite key.  It is mixed freely with BRB_MD5Update on
 * one context, and the result is read as ctx.digest or as ctx.string, the 32 hex characters.  MD5 only:
 * the reference has no SHA-1 counterpart.
 *   Lower-casing is the reference's: a byte 0x41 .. 0x5A gets + 0x20, every other byte is unchanged --
 *   bytes >= 0x80 too (the reference compares signed char: 0xC1 .. 0xDA do not move).  A piece of any
 *   length is accepted, with the meaning of this library's BRB_MD5UpdateLowerText (128-byte steps; the
 *   reference overruns its stack buffer beyond that).  The counters advance once per key / segment by
 *   its length, which MD5's additive count makes equal to those 128-byte steps.  Length 0 changes
 *   nothing (key_sz <= 0 in the reference) and its offset need not be memory.  data is never written.
 *
 * BRB_MD5LowerTextBatch, the context-free call for short keys (no 168-byte context is read or written
 *   per key): key i = data[offsets[i] .. + lengths[i]) at any byte alignment; keys may overlap and may
 *   be shared.  digests[i] / strings[i] = ctx.digest / ctx.string[0 .. 33) after BRB_MD5Init,
 *   BRB_MD5UpdateLowerText(key i), BRB_MD5Final: 16 bytes, and 32 lower-case hex characters with their
 *   NUL (BRB_MD5ToStr's buffer).  digests or strings may be NULL, not both.
 *   Flags, return codes, hip_stream and the device-mode contract are BRB_MD5Batch's; device mode
 *   validates nothing beyond NULL pointers, the key count and the flags, and allocates nothing
 *   (with ASYNC graph-capturable: GRAPH CAPTURE above).  BRB_BATCH_HOST returns -1 with a reason, and
 *   writes nothing, for: NULL offsets
 *   or lengths; both outputs NULL; NULL data with a key that has bytes; a key range that wraps; more
 *   keys than a launch takes; BRB_BATCH_ALL_DEVICES with BRB_BATCH_DEVICE.  Host mode stages the span of
 *   the non-empty keys in and the given outputs out.  BRB_BATCH_ALL_DEVICES splits the keys into
 *   contiguous ranges, always: the outputs are fixed-stride rows.  n == 0 returns 1.  No wave-pair
 *   kernel: BRB_BATCH_FAULT never occurs.  No CPU fallback: without a usable device the call returns 0
 *   with a LastError and writes nothing.
 *
 * BRB_MD5UpdateSegmentsLowerBatch is BRB_MD5UpdateSegmentsBatch with a byte per segment: seg_lower[k] != 0
 *   takes segment k as BRB_MD5UpdateLowerText, 0 as BRB_MD5UpdateBig; seg_lower == NULL: every segment is
 *   lower-cased.  seg_lower is indexed like seg_lengths.  Everything BRB_MD5UpdateSegmentsBatch documents
 *   holds word for word -- the defined part of a context, the untouched digest rows of items not
 *   finalised, each context named at most once, the host-mode refusals, the staging that travels with the
 *   item ranges under BRB_BATCH_ALL_DEVICES -- and host mode additionally stages seg_lower over the named
 *   segment range.  With seg_lower all zero the result is bit for bit BRB_MD5UpdateSegmentsBatch's.  A
 *   batch BRB_MD5UpdateLowerText on contexts is the one-segment-per-item list with seg_lower == NULL. */
int BRB_MD5LowerTextBatch(const void *data, const uint64_t *offsets, const uint32_t *lengths, uint64_t n,
                          unsigned char (*digests)[16], char (*strings)[33], unsigned flags, void *hip_stream);
int BRB_MD5UpdateSegmentsLowerBatch(BRB_MD5_CTX *ctxs, uint64_t n_ctx, const uint32_t *ctx_index,
                                    const void *data, const uint64_t *seg_offsets, const uint32_t *seg_lengths,
                                    const uint8_t *seg_lower, const uint64_t *item_first_seg, uint64_t n,
                                    const uint8_t *final, unsigned char (*digests)[16], unsigned flags,
                                    void *hip_stream);

/* Blowfish ECB over n_blocks blocks in place.  A block is the reference's (xl, xr) pair of
 * 64-bit `unsigned long` words (blowfish.c:312, mem_buf.c:1538-1539): words[2i] = xl,
 * words[2i+1] = xr.  The result equals BRB_Blowfish_Encrypt/Decrypt(ctx, &w[2i], &w[2i+1])
 * for every i, bit for bit in all 64 bits.  With BRB_BATCH_DEVICE, ctx is a device copy of the
 * 8336-byte BRB_BLOWFISH_CTX. */
int BRB_Blowfish_EncryptBatch(const BRB_BLOWFISH_CTX *ctx, unsigned long *words, uint64_t n_blocks,
                              unsigned flags, void *hip_stream);
int BRB_Blowfish_DecryptBatch(const BRB_BLOWFISH_CTX *ctx, unsigned long *words, uint64_t n_blocks,
                              unsigned flags, void *hip_stream);

/* Blowfish ECB in place with a context per record: the reference keeps a Blowfish context per
 * connection and direction (CommEvCryptoInfo, libbrb_ev_comm.h:206-236), BRB_Blowfish_InitBatch builds
 * them, and these calls use them, n_rec records in one launch.  Record i is block_counts[i] blocks
 * (pairs of 64-bit words) starting at words + word_offsets[i] -- an offset in 8-byte words, so a record
 * may start at 8 mod 16 -- keyed by ctxs[ctx_index ? ctx_index[i] : i] (n_ctx contexts of 8336 bytes,
 * contiguous).  Every word equals BRB_Blowfish_Encrypt/Decrypt with that context, bit for bit in all 64
 * bits.  Records must not overlap each other; words between records keep their values; a record of 0
 * blocks touches nothing (neither its words nor its context).  Flags and return codes as the other
 * batch calls.  BRB_BATCH_HOST: ctx_index[i] >= n_ctx, or a NULL ctx_index with n_ctx != n_rec, returns
 * -1 with nothing written; the span of the records is staged in both directions (words at any byte
 * alignment) and the contexts the records name are uploaded.  BRB_BATCH_DEVICE (optionally
 * BRB_BATCH_ASYNC) validates nothing but the alignment: words and ctxs must be 8-byte aligned (-1
 * otherwise); it runs on hip_stream and needs no workspace.  BRB_BATCH_ALL_DEVICES (host mode) splits
 * the records into contiguous ranges only when those ranges' spans do not interleave (as the RC4
 * calls), each part uploading the contexts its records name; otherwise the call runs on the calling
 * thread's device.  n_rec == 0 returns 1; a NULL pointer with n_rec > 0 returns -1 (ctx_index may be
 * NULL).  No wave-pair kernel: BRB_BATCH_FAULT never occurs.  The 64 lanes of a record work on it alone:
 * one record far longer than the others of its group of 16 holds the group up, so long single-key
 * buffers belong to BRB_Blowfish_EncryptBatch. */
int BRB_Blowfish_EncryptBatchKeyed(const BRB_BLOWFISH_CTX *ctxs, uint64_t n_ctx, const uint32_t *ctx_index,
                                   unsigned long *words, const uint64_t *word_offsets,
                                   const uint32_t *block_counts, uint64_t n_rec, unsigned flags, void *hip_stream);
int BRB_Blowfish_DecryptBatchKeyed(const BRB_BLOWFISH_CTX *ctxs, uint64_t n_ctx, const uint32_t *ctx_index,
                                   unsigned long *words, const uint64_t *word_offsets,
                                   const uint32_t *block_counts, uint64_t n_rec, unsigned flags, void *hip_stream);

/* ---- Key setup as a batch (EvAIOReqTransform_CryptoEnable, ev_kq_aio_transform.c:75-108) ------
 * Key i = keys[key_offsets[i] .. + key_lengths[i]).  Keys may sit at any byte offset and may overlap
 * or be shared: one key used by every record (all offsets equal) is the daemon's normal case.  Only
 * the key bytes the reference would read are read -- RC4 indexes key[k % len] for k < 256, the first
 * min(len, 256) bytes; Blowfish takes 72 key bytes cyclically, the first min(len, 72) -- through
 * aligned dwords, and nothing beyond the dword holding a key's last used byte is touched.
 * Flags and return codes as the other batch calls: BRB_BATCH_HOST copies the span of the key bytes,
 * the offsets and the lengths in and the states / contexts out; BRB_BATCH_DEVICE (optionally
 * BRB_BATCH_ASYNC) runs on hip_stream and copies nothing; BRB_BATCH_ALL_DEVICES (host mode) splits
 * the keys into contiguous ranges, always, since the outputs are fixed-stride.  Neither call uses a
 * wave-pair kernel: BRB_BATCH_FAULT never occurs.  n_keys == 0 returns 1 and touches nothing.  A
 * NULL pointer with n_keys > 0 returns -1; so does, in host mode, any key_lengths[i] == 0; nothing is
 * written.  Device mode validates no length: a zero length is the caller's broken promise (the
 * device-mode contract above); its record reads no key byte, gets the schedule of one zero byte, and
 * no memory outside that record's own state or context is touched.  Device mode: states must be
 * 4-byte aligned (as the RC4 calls assume), ctxs 8-byte aligned.  No CPU fallback: without a usable
 * device the calls return 0 with a LastError. */

/* states[i] (264 bytes each, contiguous) = the state EvAIOReqTransform_CryptoEnable leaves: all 264
 * bytes zeroed, then BRB_RC4_Init(&states[i], key i).  All 264 bytes are written (perm,
 * index1 = index2 = 0, six zero bytes). */
int BRB_RC4_InitBatch(BRB_RC4_State *states, const void *keys, const uint64_t *key_offsets,
                      const uint32_t *key_lengths, uint64_t n_keys, unsigned flags, void *hip_stream);

/* ctxs[i] (8336 bytes each, contiguous) = BRB_Blowfish_Init(&ctxs[i], key i), every 64-bit entry of P
 * and S bit for bit (blowfish.c:382-443 with the 64-bit carries of _F). */
int BRB_Blowfish_InitBatch(BRB_BLOWFISH_CTX *ctxs, const void *keys, const uint64_t *key_offsets,
                           const uint32_t *key_lengths, uint64_t n_keys, unsigned flags, void *hip_stream);

/* ---- RC4 and the RC4+MD5 frame of the comm transform -------------------------
 * One stream per connection; states[i] is that connection's BRB_RC4_State (an array of n
 * contiguous 264-byte states) and advances exactly as the scalar calls would.  Streams of one
 * call must belong to different connections (a connection's buffers are sequential). */

/* out[offsets[i] .. + lengths[i]) = BRB_RC4_Crypt(&states[i], in + offsets[i], ..., lengths[i]).
 * out may equal in (in place); otherwise the ranges of in and out must not overlap. */
int BRB_RC4_CryptBatch(BRB_RC4_State *states, const void *in, void *out, const uint64_t *offsets,
                       const uint32_t *lengths, uint64_t n_streams, unsigned flags, void *hip_stream);

/* Bytes before the payload in a frame: salt (8) "HASH:" (5) MD5 (16) NUL (1). */
#define BRB_RC4MD5_HEADER 30

/* WRITE side of EvAIOReqTransform_CryptoRaw(COMM_CRYPTO_FUNC_RC4_MD5) (ev_kq_aio_transform.c:
 * 212-230, 281-283) for n connections: with payload i = payload[offsets[i] .. + lengths[i]),
 *   frames[frame_offsets[i] .. + 30 + lengths[i]) =
 *       RC4(states[i], salts[i] as 8 LE bytes | "HASH:" | MD5(payload i) | NUL | payload i).
 * salts[i] is the caller's arc4random() value (the reference's `unsigned long random_salt`).
 * The frames must not overlap each other or the payloads. */
int BRB_RC4MD5_FrameBatch(BRB_RC4_State *states, const void *payload, const uint64_t *offsets,
                          const uint32_t *lengths, const uint64_t *salts, void *frames,
                          const uint64_t *frame_offsets, uint64_t n, unsigned flags, void *hip_stream);

/* READ side (ev_kq_aio_transform.c:270-279) followed by EvAIOReqTransform_RC4_MD5_DataValidate
 * (:158-184): frame i = frames[offsets[i] .. + lengths[i]) is RC4-decrypted with states[i] into
 * out at the same offset (out may equal frames), and valid[i] = 1 if bytes 8..12 are "HASH:" and
 * bytes 13..28 are the MD5 of bytes 30.., else 0.  A frame shorter than 30 bytes is decrypted and
 * reported invalid (the reference would digest past the end of the buffer). */
int BRB_RC4MD5_OpenBatch(BRB_RC4_State *states, const void *frames, void *out, const uint64_t *offsets,
                         const uint32_t *lengths, uint64_t n, uint8_t *valid, unsigned flags,
                         void *hip_stream);

/* ---- The three calls above with a buffer list per stream --------------------------------------
 * A connection that queued several buffers in one event-loop round (one aio_req per
 * EvAIOReqTransform_WriteData) needs one call per buffer above, each loading and storing its state.
 * Here stream i owns buffers stream_first_buf[i] .. stream_first_buf[i + 1] - 1 (n_streams + 1
 * entries, non-decreasing, as rec_first_seg of BRB_MD5BatchSegments); buf_offsets, buf_lengths,
 * salts, frame_offsets and valid are indexed by buffer.  One launch: states[i] is read once, the
 * stream's buffers are processed in list order, states[i] is written once.  The result -- outputs,
 * valid flags and all 264 bytes of every state -- is exactly what the scalar calls leave when applied
 * to the stream's buffers in list order with states[i]: BRB_RC4_Crypt per buffer (CryptList); the
 * WRITE side of EvAIOReqTransform_CryptoRaw(RC4_MD5) per buffer (FrameList); the READ side plus
 * EvAIOReqTransform_RC4_MD5_DataValidate per buffer (OpenList: a frame shorter than 30 bytes is
 * decrypted and reported invalid, a failed check changes nothing else, and the stream goes on with
 * its next buffer).  With one buffer per stream the outputs and states are those of the calls above.
 * A stream without buffers keeps its state bit for bit; an empty buffer reads and writes nothing and
 * its offset need not be memory.  out may equal in / frames.  Buffers of one call must not overlap
 * each other; frames must not overlap each other or any payload of the call; bytes between buffers
 * keep their values.
 * Flags, return codes and hip_stream as BRB_RC4_CryptBatch.  BRB_BATCH_DEVICE (optionally
 * BRB_BATCH_ASYNC): every pointer is device memory, states are 4-byte aligned, nothing is allocated
 * (with ASYNC graph-capturable: GRAPH CAPTURE above) and nothing is validated beyond NULL pointers, the
 * stream count and the flags.
 * BRB_BATCH_HOST returns -1 with a reason, and writes nothing, for: a NULL required pointer; a
 * stream_first_buf that decreases; an offset + length (+ 30 for frames) that wraps; more streams or
 * buffers than a launch takes; BRB_BATCH_ALL_DEVICES with BRB_BATCH_DEVICE.  Host mode stages the
 * n_streams states in both directions, the span of the named buffers (outputs in both directions, so
 * bytes between buffers survive), the index arrays, and valid out.  BRB_BATCH_ALL_DEVICES (host mode)
 * splits the streams into contiguous ranges, their buffer ranges with them, only when the parts'
 * written byte spans do not interleave (as BRB_RC4_CryptBatch); otherwise the call runs on the
 * calling thread's device.  n_streams == 0 returns 1 and touches nothing.  One wave per 64 streams, no
 * wave pairs: BRB_BATCH_FAULT never occurs.  No CPU fallback: without a usable device the call
 * returns 0 with the reason in BRB_CryptoGPU_LastError(). */
int BRB_RC4_CryptListBatch(BRB_RC4_State *states, const void *in, void *out, const uint64_t *buf_offsets,
                           const uint32_t *buf_lengths, const uint64_t *stream_first_buf, uint64_t n_streams,
                           unsigned flags, void *hip_stream);
/* Buffer k: frames[frame_offsets[k] .. + 30 + buf_lengths[k]) = the frame of payload[buf_offsets[k] ..
 * + buf_lengths[k]) with salts[k], encrypted with its stream's state (BRB_RC4MD5_FrameBatch). */
int BRB_RC4MD5_FrameListBatch(BRB_RC4_State *states, const void *payload, const uint64_t *buf_offsets,
                              const uint32_t *buf_lengths, const uint64_t *salts, void *frames,
                              const uint64_t *frame_offsets, const uint64_t *stream_first_buf, uint64_t n_streams,
                              unsigned flags, void *hip_stream);
/* Buffer k: frame k = frames[buf_offsets[k] .. + buf_lengths[k]) is decrypted into out at the same
 * offset and valid[k] is set (BRB_RC4MD5_OpenBatch). */
int BRB_RC4MD5_OpenListBatch(BRB_RC4_State *states, const void *frames, void *out, const uint64_t *buf_offsets,
                             const uint32_t *buf_lengths, const uint64_t *stream_first_buf, uint64_t n_streams,
                             uint8_t *valid, unsigned flags, void *hip_stream);

/* ---- Streams of mixed kind in one call ---------------------------------------------------------
 * The reference fixes a connection's transform when it is enabled (EvAIOReqTransform_CryptoEnable
 * stores crypto->algo_code per connection, ev_kq_aio_transform.c:75-108), so a daemon holds RC4 and
 * RC4_MD5 connections side by side, and an RC4_MD5 connection opens in one direction and frames in
 * the other.  The three list calls above take one kind per launch.  Here stream i carries its kind
 * in stream_kind[i] and uses states[state_index ? state_index[i] : i] (n_states states; every stream
 * of a call names a state of its own).  Stream i owns buffers stream_first_buf[i] ..
 * stream_first_buf[i + 1] - 1; buffer k is in[buf_offsets[k] .. + buf_lengths[k]) and its result is
 * written at out + out_offsets[k]: buf_lengths[k] bytes for CRYPT and OPEN, 30 + buf_lengths[k] for
 * FRAME.  salts[k] is read for FRAME buffers only and valid[k] written for OPEN buffers only; salts may
 * be NULL when no stream is FRAME, valid when none is OPEN.
 * The result -- outputs, valid of OPEN buffers, all 264 bytes of every named state -- is exactly
 * what the scalar calls leave when applied to the stream's buffers in list order, as the list call of
 * the stream's kind defines it.  States not named keep every byte, and so do valid entries of
 * buffers that are not OPEN.  A stream without buffers keeps its state bit for bit; an empty buffer
 * reads and writes nothing and its offsets need not be memory (a FRAME buffer of length 0 still
 * writes its 30-byte frame).  A CRYPT or OPEN buffer may be written in place (out == in and
 * out_offsets[k] == buf_offsets[k]); otherwise no output range overlaps any input or output range of
 * the call.
 * One launch, one lane per stream.  A wave (64 consecutive streams) whose streams are of one kind runs
 * that kind's code alone; a wave with two or three kinds runs them one after another, which is
 * correct and slower: group the streams by kind.
 * Flags, return codes and hip_stream as BRB_RC4_CryptListBatch.  BRB_BATCH_DEVICE (optionally
 * BRB_BATCH_ASYNC): every pointer is device memory, nothing is allocated (with ASYNC
 * graph-capturable: GRAPH CAPTURE above) and nothing is validated beyond NULL pointers, the counts and
 * the flags.  BRB_BATCH_HOST returns -1 with a reason, and writes nothing, for: a NULL required
 * pointer (salts with a FRAME stream, valid with an OPEN stream); a kind above 2; a
 * stream_first_buf that decreases; an offset + length (+ 30 for a FRAME output) that wraps; a
 * state_index entry >= n_states, or one named twice (without state_index: n_streams > n_states); more
 * streams or buffers than a launch takes; BRB_BATCH_ALL_DEVICES, which this call does not split.
 * Host mode stages the named states densely in both directions (states not named are neither read
 * nor written), the span of the inputs, the span of the outputs in both directions (so bytes between
 * buffers survive), the arrays, and valid over the named buffers in both directions.
 * n_streams == 0 returns 1 and touches nothing.  Lone waves: BRB_BATCH_FAULT never occurs.  No CPU
 * fallback: without a usable device the call returns 0 with the reason in BRB_CryptoGPU_LastError(). */
#define BRB_RC4_KIND_CRYPT 0   /* BRB_RC4_Crypt per buffer                       */
#define BRB_RC4_KIND_FRAME 1   /* WRITE side of RC4_MD5 per buffer (+30 bytes)    */
#define BRB_RC4_KIND_OPEN  2   /* READ side of RC4_MD5 + DataValidate per buffer  */
int BRB_RC4_MixedListBatch(BRB_RC4_State *states, uint64_t n_states, const uint32_t *state_index,
                           const uint8_t *stream_kind, const void *in, void *out,
                           const uint64_t *buf_offsets, const uint32_t *buf_lengths,
                           const uint64_t *out_offsets, const uint64_t *salts,
                           const uint64_t *stream_first_buf, uint64_t n_streams,
                           uint8_t *valid, unsigned flags, void *hip_stream);

/* ---- Receive-loop batching ------------------------------------------------------
 * The comm layer calls the transform hook once per buffer on the thread that owns the connection
 * (EvAIOReqTransform_ReadData / _WriteData, ev_kq_aio_transform.c:42-70, from comm_tcp_server.c:1749,
 * 1773, comm_tcp_client_read.c:176, 203, comm_tcp_server_conn.c:932).  A transform batcher takes the
 * buffers of one event-loop round from many connections and runs them as one GPU call per
 * direction.  It owns the read and write RC4 states of up to max_conns connections in HBM
 * (CommEvCryptoInfo, libbrb_ev_comm.h:206-236).  Usage per round: Read/Write for every buffer,
 * then Flush, which delivers every result through the callback in submission order.
 * A connection's buffers stay in order: two buffers of one connection and direction in one round
 * run as consecutive sub-rounds.
 *   READ  (RC4_MD5): out = the decrypted frame, valid = EvAIOReqTransform_RC4_MD5_DataValidate;
 *         the payload starts at out + BRB_RC4MD5_HEADER (the reference's MemBufferOffsetSet(30)).
 *   WRITE (RC4_MD5): out = the 30 + len byte frame, salt = the caller's arc4random() value.
 *   RC4: out = the RC4 stream of the buffer in either direction, valid = 1. */
#define BRB_CRYPTO_FUNC_RC4       1       /* COMM_CRYPTO_FUNC_RC4, libbrb_ev_comm.h:166 */
#define BRB_CRYPTO_FUNC_RC4_MD5   2       /* COMM_CRYPTO_FUNC_RC4_MD5, :167 */
#define BRB_CRYPTO_OP_READ        0       /* CRYPTO_OPERATION_READ, libbrb_ev_aio.h:101 */
#define BRB_CRYPTO_OP_WRITE       1       /* CRYPTO_OPERATION_WRITE, :102 */
/* OR into `algo` at Create: zero-copy rounds.  Read/Write keep a reference to `data` instead of
 * copying it: the bytes must lie in page-locked memory (BRB_CryptoGPU_HostRegister, or allocated
 * page-locked by HIP) and stay unchanged until Flush returns.  The kernels read the buffers over
 * PCIe and write the results into the batcher's page-locked output arena: no staging memcpy on the
 * CPU, no bulk H2D/D2H copies.  Read/Write return -1 for a buffer outside page-locked memory. */
#define BRB_BATCHER_ZERO_COPY     0x100
/* OR into `algo` at Create: pipelined rounds.  The batcher owns two rounds' arenas, so the loop fills
 * round k+1 while the GPU runs round k (BRB_TransformBatcherFlushAsync).  Twice the arena memory. */
#define BRB_BATCHER_PIPELINED     0x200
/* OR into `algo` at Create: all devices (the daemon's multi-threaded engine spreading connections,
 * ev_kq_base.c:95).  Connection c lives on device c % G (G = visible devices) with its read and
 * write states; Read/Write/Enable/GetState route by connection, and one Flush / FlushAsync enqueues
 * every device's round before it waits for any, so the devices run concurrently.  Callbacks come on
 * the calling thread, device by device: each connection's buffers keep their order, buffers of
 * connections on different devices are not interleaved in submission order.  With one device (or
 * max_conns < G) this is a plain batcher. */
#define BRB_BATCHER_ALL_DEVICES   0x400
/* OR into `algo` at Create: connection lists.  A round runs as one launch per direction (the READ
 * group, then the WRITE group) whatever the number of buffers per connection: each (direction,
 * connection) is one stream of the list calls above, its buffers in submission order, so a
 * connection's state is loaded and stored once per round and direction instead of once per buffer.
 * Results, callback order, GetState, key epochs and the dropped-round and poisoning rules are those of
 * a batcher without the flag; it combines with the three flags above (an all-devices batcher passes it
 * to its parts).  The list kernels run one wave per 64 connections, not wave pairs. */
#define BRB_BATCHER_CONN_LISTS    0x800
/* OR into `algo` at Create: an algo per connection, one launch per round.  The reference fixes a
 * connection's transform when it is enabled (crypto->algo_code, ev_kq_aio_transform.c:75-108) and a
 * daemon holds RC4 and RC4_MD5 connections side by side.  With this flag the numeric algo is only the
 * default that Enable and EnableBatch give a connection; EnableAlgo / EnableBatchAlgo give it its own.
 * A round is one launch of the mixed kernel (BRB_RC4_MixedListBatch above): every (direction,
 * connection) is a stream with its buffers in submission order, CRYPT for an RC4 connection in either
 * direction, OPEN for an RC4_MD5 read, FRAME for an RC4_MD5 write; the streams are sorted by kind, so
 * all but two waves of a round run one kind.  Read and Write take the connection's algo at submission:
 * an RC4_MD5 write delivers len + 30 bytes, an RC4 buffer ignores salt and delivers valid = 1, an
 * RC4_MD5 read delivers the check's verdict.  The flag implies BRB_BATCHER_CONN_LISTS (passing both
 * changes nothing) and combines with ZERO_COPY, PIPELINED and ALL_DEVICES (passed to the parts).
 * Enable / EnableBatch on a connection that has another algo than the default return 0, with nothing
 * changed, while the round being filled holds a buffer of it (as EnableAlgo does for any connection).
 * Callback order, GetState, key epochs and the dropped-round and poisoning rules are those of every
 * batcher.  The kernel runs lone waves, not wave pairs. */
#define BRB_BATCHER_MIXED         0x1000
typedef struct BRB_TransformBatcher BRB_TransformBatcher;
typedef void (*BRB_TransformDone)(void *user, uint32_t conn, int op, const void *out, uint32_t out_len, int valid);
/* `valid` of a buffer whose round was dropped (out = NULL, out_len = 0): see Flush. */
#define BRB_TRANSFORM_DROPPED (-1)
/* NULL on failure (reason in BRB_CryptoGPU_LastError).  A round holds at most max_round_bytes of
 * input and 4 * max_conns buffers; Read/Write return 0 when it is full (Flush, then submit again). */
BRB_TransformBatcher *BRB_TransformBatcherCreate(uint32_t max_conns, uint64_t max_round_bytes, int algo);
void BRB_TransformBatcherDestroy(BRB_TransformBatcher *b);
/* EvAIOReqTransform_CryptoEnable (ev_kq_aio_transform.c:71-105): both states of `conn` = BRB_RC4_Init(key). */
int BRB_TransformBatcherEnable(BRB_TransformBatcher *b, uint32_t conn, const void *key, int key_sz);
/* EvAIOReqTransform_CryptoEnable(transform_info, algo_code, key, key_sz): as Enable, and the
 * connection's algo becomes `algo` (Enable: the batcher's own).  Returns -1, with nothing changed, for
 * an algo other than RC4 (1) or RC4_MD5 (2), and for an algo other than the batcher's on a batcher
 * created without BRB_BATCHER_MIXED.  Returns 0 (BRB_BATCH_NOT_DONE) with a reason, and nothing
 * changed, when the round being filled holds a buffer of the connection -- it was submitted under
 * the old key and algo and would run under the new: Flush first. */
int BRB_TransformBatcherEnableAlgo(BRB_TransformBatcher *b, uint32_t conn, int algo, const void *key, int key_sz);
/* EvAIOReqTransform_CryptoDisable (ev_kq_aio_transform.c:110-123), on any batcher: both states of
 * `conn` are zeroed -- on the batcher's stream, so behind a round FlushAsync left running -- and the
 * connection is not enabled any more: Read / Write refuse it as one never enabled, GetState returns
 * 264 zero bytes, and Enable / EnableAlgo bring it back, poisoned or not.  Returns 0 with a reason,
 * and nothing changed, when the round being filled holds a buffer of the connection; -1 for a bad
 * batcher or connection id. */
int BRB_TransformBatcherDisable(BRB_TransformBatcher *b, uint32_t conn);
/* Enable for n connections in one call (host pointers; keys as in BRB_RC4_InitBatch, connection
 * conns[i] gets key i).  One H2D copy of the key bytes and index arrays, one kernel that writes both
 * the read and the write state of every listed connection straight into the batcher's state arrays,
 * one stream synchronisation -- on the batcher's own stream, so on a pipelined batcher it orders
 * behind a round FlushAsync left running, as Enable's copies do.  Returns -1, with nothing changed,
 * for a NULL argument, a connection id >= max_conns, a zero key length or a connection listed twice
 * (two lanes would write one state); n == 0 returns 1.  After success every listed connection is as
 * after Enable: enabled, its key epoch incremented (a poisoned connection is re-keyed).  All-devices
 * batcher: the list is split by conn % G into the parts, and every part is enqueued before any is
 * waited for.  On a device error the call returns 0, LastError names the parts that failed, and the
 * listed connections of those parts are left disabled (Read/Write refuse them until they are enabled
 * again); the other parts' connections are enabled. */
int BRB_TransformBatcherEnableBatch(BRB_TransformBatcher *b, const uint32_t *conns, uint64_t n,
                                    const void *keys, const uint64_t *key_offsets, const uint32_t *key_lengths);
/* EnableBatch with an algo per listed connection (algos[i] = 1 or 2; algos == NULL: the batcher's
 * own for all): one key-setup kernel, as EnableBatch.  Besides EnableBatch's refusals it returns -1,
 * with nothing changed, for an algo other than 1 or 2 and for an algo other than the batcher's on a
 * batcher without BRB_BATCHER_MIXED, and 0 with a reason, and nothing changed, when the round being
 * filled holds a buffer of a listed connection. */
int BRB_TransformBatcherEnableBatchAlgo(BRB_TransformBatcher *b, const uint32_t *conns, uint64_t n,
                                        const uint8_t *algos, const void *keys, const uint64_t *key_offsets,
                                        const uint32_t *key_lengths);
/* Read/Write may run concurrently on several threads (the reference's mt_engine, ev_kq_base.c:95)
 * as long as each connection is submitted from one thread; results come back in each connection's
 * order.  Flush/FlushAsync/Enable/EnableAlgo/EnableBatch/EnableBatchAlgo/Disable must not overlap them.  A thread reserves slots and arena bytes in
 * chunks, so a round shared by T threads may report full up to T chunks (64 buffers, 128 KiB) early. */
int BRB_TransformBatcherRead(BRB_TransformBatcher *b, uint32_t conn, const void *data, uint32_t len);
int BRB_TransformBatcherWrite(BRB_TransformBatcher *b, uint32_t conn, const void *data, uint32_t len, uint64_t salt);
/* Runs the round; returns the number of buffers delivered, or -1 for bad arguments.  All-devices
 * batcher: a part that cannot select its device (hipSetDevice fails) keeps its round pending and
 * delivers nothing, while the other parts deliver as usual; the call then returns
 * BRB_BATCH_PARTIAL (-3) if some buffers were delivered, 0 if none, with the parts and the
 * delivered count in LastError -- Flush again once the device is back.  A round that
 * fails on the device is dropped and never re-run (kernels launched before the failure may have
 * advanced their connections' states; running them again would advance them twice): each of its
 * buffers still gets its callback, in order, with valid = BRB_TRANSFORM_DROPPED, out = NULL and
 * out_len = 0, and the call returns BRB_BATCH_DROPPED (-2) with the reason in LastError -- also when
 * another round was delivered in the same call, whose buffers came back through their callbacks as
 * usual (and BRB_BATCH_PARTIAL when, besides, a part's round stays pending).  A round in which a
 * wave-pair kernel reports a protocol fault (BRB_BATCH_FAULT above) is dropped the same way, so no
 * output, frame or valid flag computed over wrong bytes is ever delivered.  The connections of a round
 * dropped on the device (a completion error or a wave-pair fault) are out of step with their peers, as
 * after a lost buffer in the reference, and stay poisoned until Enable re-keys them: their buffers
 * already launched behind the dropped round (pipelined FlushAsync) and those still waiting in the
 * filling round come back BRB_TRANSFORM_DROPPED (the call returns BRB_BATCH_DROPPED), and Read/Write
 * refuse them (BRB_BATCH_BADARG) until then.  A round whose kernel launch failed on the host is
 * dropped without poisoning (only the groups launched before the failure ran, once each).  On a
 * pipelined batcher Flush first delivers the round
 * FlushAsync left running, so Flush drains everything.  A batcher's calls run on the device it was
 * created on and leave the calling thread's current device unchanged. */
int64_t BRB_TransformBatcherFlush(BRB_TransformBatcher *b, BRB_TransformDone done, void *user);
/* Pipelined rounds: enqueues the current round and returns without waiting for it, after delivering
 * the previous round (if one is running) in submission order; Read/Write then fill the other arena.
 * Returns the number of buffers delivered (those of the previous round), or -1 / 0 as Flush.  A
 * connection's streams stay in order across rounds (one HIP stream).  In zero-copy mode a buffer
 * must stay unchanged until its round is delivered.  Without BRB_BATCHER_PIPELINED this is Flush. */
int64_t BRB_TransformBatcherFlushAsync(BRB_TransformBatcher *b, BRB_TransformDone done, void *user);
/* Copies a connection's current state (op = READ or WRITE) back to the host (tests, migration). */
int BRB_TransformBatcherGetState(BRB_TransformBatcher *b, uint32_t conn, int op, BRB_RC4_State *out);
/* Test support, not for production use: from now on the `launch`-th kernel launch (0-based) of every
 * round reports a failure without running, so a test can watch a round being dropped; -1 turns it
 * off.  A round launches one kernel per direction and sub-round (READ before WRITE in each sub-round);
 * with BRB_BATCHER_CONN_LISTS one per direction, so at most two; with BRB_BATCHER_MIXED one, so launch = 0
 * drops the round with nothing run (no state changes, nothing is poisoned) and launch = 1 never fires.  Returns 1, or -1 for a NULL batcher.  (Replaces round 2's BRB_TEST_BATCHER_FAULT variable:
 * the library reads no environment variable.) */
int BRB_TransformBatcherInjectFault(BRB_TransformBatcher *b, int launch);

/* ---- base64 -----------------------------------------------------------------------
 * Encode = brb_base64_encode_to_mb (base64.c:304-361) for n records: record i = data[offsets[i] ..
 * + lengths[i]) -> out[out_offsets[i] .. + 4 * ceil(lengths[i] / 3)), standard alphabet, '='
 * padding, no NUL written.  (brb_base64_encode_bin's static 131 070-byte result buffer cap is a
 * property of that buffer, not of the encoding, and is not reproduced.) */
int BRB_Base64EncodeBatch(const void *data, const uint64_t *offsets, const uint32_t *lengths, uint64_t n,
                          void *out, const uint64_t *out_offsets, unsigned flags, void *hip_stream);
/* Decode = brb_base64_decode_to_mb (base64.c:131-179) for n records: record i = text[offsets[i] ..
 * + lengths[i]) read as a C string (a NUL ends it); bytes outside the alphabet are skipped, '='
 * counts as the value 0 (base64.c:374), every 4 counted characters give 3 bytes, a trailing
 * partial group is dropped.  out_lengths[i] = bytes written at out + out_offsets[i]; the caller
 * reserves 3 * (lengths[i] / 4) bytes there. */
int BRB_Base64DecodeBatch(const void *text, const uint64_t *offsets, const uint32_t *lengths, uint64_t n,
                          void *out, const uint64_t *out_offsets, uint32_t *out_lengths, unsigned flags,
                          void *hip_stream);

/* ---- MemBuffer Blowfish -------------------------------------------------------
 * MemBufferEncryptData / MemBufferDecryptData (mem_buf.c:1499-1617) on the bytes of a MemBuffer:
 * buf = MemBufferDeref(mb) with mb->offset == 0, size = MemBufferGetSize(mb).  Reproduced exactly:
 *   key[i] = (i + seed) * seed + 13 i, seed = key[i] * seed            (mem_buf.c:1511-1515)
 *   encrypt: Blowfish keyLen 4 (sizeof(enc_key[16])), pairs of 64-bit words from buf + offset,
 *            (size + offset) / 8 + 2 words rounded up to pairs; new size = 8 * words + offset
 *   decrypt: keyLen 64 (sizeof(enc_key)), (size - offset) / 8 + 2 words, stops at the first pair
 *            holding a zero word; new size = 8 * words decrypted + offset
 * (so decrypt(encrypt(x)) does not restore x, as in the reference).  The caller grows the buffer
 * first, as MemBufferCheckForGrow does (mem_buf.c:1525, 1585): buf must hold
 * offset + BRB_MEMBUF_SPAN(size + offset) bytes to encrypt, offset + BRB_MEMBUF_SPAN(size - offset)
 * bytes to decrypt.  The Blowfish context is built on the host; the
 * ECB pass (and the zero-pair scan) run on the GPU.  Device mode needs buf + offset 8-byte
 * aligned.  Both calls return when *new_size is known (ASYNC is ignored). */
#define BRB_MEMBUF_SPAN(data_size) ((((data_size) / 8 + 3) / 2) * 16)
void BRB_MemBufferKey(unsigned int seed, unsigned int key[16]);
int BRB_MemBufferEncrypt(void *buf, unsigned long size, unsigned int seed, unsigned long offset,
                         unsigned long *new_size, unsigned flags, void *hip_stream);
int BRB_MemBufferDecrypt(void *buf, unsigned long size, unsigned int seed, unsigned long offset,
                         unsigned long *new_size, unsigned flags, void *hip_stream);

/* The same for n_buf MemBuffers in one call (one key-setup launch for the seeds, one keyed ECB launch,
 * one synchronisation).  Buffer i is data + buf_offsets[i]; its MemBuffer size is sizes[i], its offset
 * argument offsets[i] (offsets == NULL: 0 for all), its seed seeds[seed_index ? seed_index[i] :
 * (n_seeds == 1 ? 0 : i)].  Semantics per buffer exactly as the single calls (key derivation, keyLen 4
 * / 64, the +2 words rounded up to pairs, the zero-word stop -- bytes from the stop onward are not
 * written), new_sizes[i] as *new_size; the caller grows and zero-fills every buffer to BRB_MEMBUF_SPAN
 * first, and the buffers' spans must not overlap.  seeds is always host memory (a parameter, not
 * data); data and the other arrays follow flags.  n_seeds must be >= 1, and 1 or n_buf when seed_index
 * is NULL (-1 otherwise).  Host mode: any byte alignment per buffer; a decrypt sizes[i] < offsets[i], a
 * seed_index[i] >= n_seeds or a buffer of 2^32 pairs or more returns -1; on a refusal nothing is
 * written; BRB_BATCH_ALL_DEVICES is accepted and runs on the calling thread's device.  Device mode:
 * data must be 8-byte aligned (-1 otherwise) and so must every buf_offsets[i] + offsets[i], the
 * caller's promise; a buffer that breaks that promise or one of the host-mode rules above is left
 * untouched (its new_sizes[i] is then meaningless).  The contexts live in the calling thread's
 * workspace, so both modes return when new_sizes is known (ASYNC is ignored).  n_buf == 0 returns 1. */
int BRB_MemBufferEncryptBatch(void *data, const uint64_t *buf_offsets, const uint64_t *sizes,
                              const uint64_t *offsets, const unsigned int *seeds, uint64_t n_seeds,
                              const uint32_t *seed_index, uint64_t n_buf, uint64_t *new_sizes, unsigned flags,
                              void *hip_stream);
int BRB_MemBufferDecryptBatch(void *data, const uint64_t *buf_offsets, const uint64_t *sizes,
                              const uint64_t *offsets, const unsigned int *seeds, uint64_t n_seeds,
                              const uint32_t *seed_index, uint64_t n_buf, uint64_t *new_sizes, unsigned flags,
                              void *hip_stream);

/* ---- runtime ---------------------------------------------------------------------------- */
/* 1 if a HIP device is usable from this process, else 0 (reason in LastError). */
int BRB_CryptoGPU_Available(void);
/* Number of visible HIP devices (probed once per process); 0 if none (reason in LastError). */
int BRB_CryptoGPU_DeviceCount(void);
/* Makes `dev` the calling thread's current device for the batch calls, so a C caller that does not
 * link HIP itself can drive several GPUs (e.g. one event thread per GPU): 1 = done, 0 = no device /
 * HIP error, -1 = dev out of range. */
int BRB_CryptoGPU_SetDevice(int dev);
/* The calling thread's current device, or -1 (reason in LastError). */
int BRB_CryptoGPU_GetDevice(void);
/* Frees the calling thread's host-mode scratch (device workspaces, streams, events) now instead of
 * at thread exit.  Call it with no batch call of this thread running.  If the thread made
 * device-mode BRB_BATCH_ASYNC calls of wave-pair kernels, their devices are synchronised first
 * (hipDeviceSynchronize), since those kernels may still write the thread's fault word.  Not while a
 * graph in which this thread captured such a call can still be replayed (GRAPH CAPTURE above). */
void BRB_CryptoGPU_ThreadCleanup(void);
/* Last error of the calling thread ("" if none). */
const char *BRB_CryptoGPU_LastError(void);
/* Wave-pair faults of the calling thread's device-mode BRB_BATCH_ASYNC calls: 1 if none of the
 * wave-pair kernels they enqueued since the last check reported a protocol fault, BRB_BATCH_FAULT
 * (-4) if one did (reason in LastError; the report is cleared).  Call it after synchronising the
 * streams those calls used: a kernel still running has not reported yet.  Replays of a graph count as
 * calls of the thread that captured them (GRAPH CAPTURE above). */
int BRB_CryptoGPU_AsyncFaultCheck(void);
/* Page-lock [p, p + len) for the GPU (hipHostRegister, mapped) so that zero-copy batchers can read
 * it: 1 = done, 0 = no device / HIP error (LastError), -1 = bad arguments.  Unregister takes the
 * same `p`. */
int BRB_CryptoGPU_HostRegister(void *p, uint64_t len);
int BRB_CryptoGPU_HostUnregister(void *p);
/* Test support, not for production use: process-wide A/B switches of the kernel selection, the only
 * way to change them (the library reads no environment variable).  "rc4_sector" -1/0/1 (launcher's
 * choice / force the per-stream sink / force the whole-sector sink of the RC4 pass), "var_line" 1/0
 * (variable-length digests on the line kernel / on the per-lane kernel), "fixed_var_line" 1/0
 * (unaligned fixed-stride records on the line kernel / record-relative kernel), "var_sort" 1/0
 * (variable-length batches bucketed by length / in caller order; 2 keeps the first round of groups in
 * caller order), "devices" 0/k (all-devices calls and batchers on every visible device / forced into k <= 16
 * parts, part g on device g % count; an all-devices batcher takes at most 16 parts either way), "b64_group" -1/0..6 (base64 lanes per record: launcher's choice /
 * forced to 2^value), "host_chunk_mib" / "host_digest_chunk_mib" 0/k (host-mode chunks of the default
 * 16 / 32 MiB, or k MiB; chunk-size sweeps), "seg_line" 2/1/0 (segment digests and MetaData unpack on the
 * line-staged producer / consumer wave pairs, the line-staged single waves, the per-lane kernels), "b64_kernel" 2/3/1/0 (64-byte fixed-stride records on
 * the register-buffered kernel at 8 / 4 waves per SIMD, the two-slot kernel, the generic one),
 * "line_slots" 0/2/3 (LDS-DMA ring slots of the line-staged segment and MetaData kernels: each
 * kernel's default, or forced), "rc4md5_pair" 1/0 (BRB_RC4MD5_FrameBatch / OpenBatch on keystream +
 * partner wave pairs / one wave per connection), "rc4_pair" 1/0 (BRB_RC4_CryptBatch likewise; a forced
 * "rc4_sector" value selects the one-wave kernel), "pair_stall" 0/1 (1: the segment, MetaData, RC4
 * pass and RC4+MD5 frame / open wave pairs get a protocol fault injected, so the call returns
 * BRB_BATCH_FAULT, an async call's check reports it and a batcher round is dropped), "bf_keyed" 0/1/2
 * (the keyed Blowfish ECB calls: spread image fill and two blocks per lane / the plain fill / one
 * block per lane), "rc4_list_coop" 1/0 (BRB_RC4_CryptListBatch: cooperative / per-lane block
 * loads).  Returns 1 and the previous
 * value in *old (if not NULL), or -1 for an unknown name or a value out of range. */
int BRB_CryptoGPU_TestOption(const char *name, int value, int *old);
/* Test support, not for production use: the kernel that BRB_MD5BatchFixed / BrbSha1_BatchFixed run
 * in device mode for records of rec_len bytes whose first byte is at address data_addr, under the
 * current values of the test options "fixed_var_line" and "b64_kernel".  It is the launchers' own
 * routing function, so it is the source of truth for which shape reaches which kernel; it needs no
 * device and touches no memory.  Returns one of BRB_FIXED_ROUTE_* (in launch order):
 *   LANE_A4    rec_len == 0 or rec_len >= 33 554 431 (64 rec_len + 64 >= 2^31), base and length
 *              4-byte multiples: md5_ / sha1_fixed_a4_kernel, one record per lane
 *   LANE_ANY   the same lengths otherwise: md5_ / sha1_any_kernel, one record per lane
 *   LINE       64 < rec_len <= 1 MiB, base and length 4-byte multiples: digest_line_kernel
 *   VAR_LINE   64 < rec_len <= 1 MiB otherwise, "fixed_var_line" 1: digest_var_line_kernel
 *   DMA_TICKET every other rec_len > 64: digest_fixed_dma_kernel, groups handed out by tickets
 *   B64R_8, B64R_4, B64   rec_len == 64 under "b64_kernel" 2, 3, 1: digest_b64r_kernel at a grid
 *              cap of 2048 / 1024 workgroups, digest_b64_kernel
 *   DMA_SHORT  1 <= rec_len <= 64 otherwise: digest_fixed_dma_kernel with 64-byte stages */
#define BRB_FIXED_ROUTE_LANE_A4    0
#define BRB_FIXED_ROUTE_LANE_ANY   1
#define BRB_FIXED_ROUTE_LINE       2
#define BRB_FIXED_ROUTE_VAR_LINE   3
#define BRB_FIXED_ROUTE_DMA_TICKET 4
#define BRB_FIXED_ROUTE_B64R_8     5
#define BRB_FIXED_ROUTE_B64R_4     6
#define BRB_FIXED_ROUTE_B64        7
#define BRB_FIXED_ROUTE_DMA_SHORT  8
int BRB_CryptoGPU_TestFixedRoute(uint64_t data_addr, uint32_t rec_len);
/* Library version string. */
const char *BRB_CryptoGPU_Version(void);

#ifdef __cplusplus
}
#endif
#endif /* BRB_CRYPTO_H */
