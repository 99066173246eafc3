/*
 * ref_harness.c -- a flat C interface over a build of the reference's own units, for ctypes.
 * TEST INFRASTRUCTURE ONLY (tests/golden/make_ref_run.py and the live tests of
 * tests/test_ref_run_cpu.py).  Everything here is this project's code: it includes the reference's
 * headers (found by -I at build time, never copied) and calls the reference's functions.  It states no
 * algorithm of its own; the few checks it makes only keep a call inside defined behaviour.
 *
 * The crypto entry points that take plain buffers (BRB_MD5*, BrbSha1_*, BRB_Blowfish_*, BRB_RC4_*)
 * are exported by the shared library as they are and are called from Python directly.  The wrappers
 * below exist where a call needs one of the reference's structs (MemBuffer, MetaData) or returns a
 * pointer into a static buffer.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <libbrb_core.h>

#define REF_GROW 4096          /* MemBuffer grow rate: room behind the data, as a long-lived buffer has */

/* sizeof of the structs whose whole image is recorded */
uint64_t ref_sizeof(int which)
{
    switch (which) {
    case 0: return sizeof(BRB_MD5_CTX);
    case 1: return sizeof(BrbSha1Ctx);
    case 2: return sizeof(BRB_BLOWFISH_CTX);
    case 3: return sizeof(BRB_RC4_State);
    case 4: return sizeof(MetaDataHeader);
    case 5: return sizeof(MetaDataItem);
    default: return 0;
    }
}

/* ---- MemBuffer Blowfish ----------------------------------------------------------------------------
 * A MemBuffer holding buf[0 .. size) is encrypted / decrypted; up to `cap` bytes of what it then
 * holds are copied back over buf and its new size is returned. */
uint64_t ref_membuf_crypt(uint8_t *buf, uint64_t cap, uint64_t size, unsigned int seed, uint64_t offset, int decrypt)
{
    MemBuffer *mb = MemBufferNew(BRBDATA_THREAD_UNSAFE, REF_GROW);
    MemBufferAdd(mb, buf, size);
    if (decrypt)
        MemBufferDecryptData(mb, seed, offset);
    else
        MemBufferEncryptData(mb, seed, offset);
    uint64_t new_size = mb->size;
    uint64_t n = mb->capacity < cap ? mb->capacity : cap;
    memcpy(buf, mb->data, n);
    MemBufferDestroy(mb);
    return new_size;
}

/* ---- base64 ------------------------------------------------------------------------------------- */
static uint64_t mb_take(MemBuffer *mb, uint8_t *out, uint64_t cap)
{
    uint64_t n = MemBufferGetSize(mb);
    if (n > cap)
        n = cap;
    if (n)
        memcpy(out, MemBufferDeref(mb), n);
    uint64_t full = MemBufferGetSize(mb);
    MemBufferDestroy(mb);
    return full;
}

uint64_t ref_b64_encode_to_mb(const uint8_t *in, int len, uint8_t *out, uint64_t cap)
{
    MemBuffer *mb = MemBufferNew(BRBDATA_THREAD_UNSAFE, REF_GROW);
    brb_base64_encode_to_mb((const char *)in, len, mb);
    return mb_take(mb, out, cap);
}

/* `in` need not be terminated: the decoder is given a copy of in[0 .. len) followed by a NUL */
uint64_t ref_b64_decode_to_mb(const uint8_t *in, uint64_t len, uint8_t *out, uint64_t cap)
{
    char *text = calloc(len + 1, 1);
    memcpy(text, in, len);
    MemBuffer *mb = MemBufferNew(BRBDATA_THREAD_UNSAFE, REF_GROW);
    brb_base64_decode_to_mb(text, mb);
    free(text);
    return mb_take(mb, out, cap);
}

/* the calls that answer with a pointer to a static buffer: the text is copied out */
uint64_t ref_b64_encode_bin(const uint8_t *in, int len, uint8_t *out, uint64_t cap)
{
    const char *r = brb_base64_encode_bin((const char *)in, len);
    uint64_t n = strlen(r);
    memcpy(out, r, n < cap ? n : cap);
    return n;
}

uint64_t ref_b64_decode_bin(const uint8_t *in, uint64_t len, uint8_t *out, int cap)
{
    char *text = calloc(len + 1, 1);
    memcpy(text, in, len);
    int n = brb_base64_decode_bin(text, (char *)out, cap);
    free(text);
    return (uint64_t)n;
}

/* ---- MetaData --------------------------------------------------------------------------------------- */
uint64_t ref_metadata_pack(const uint8_t *data, const uint64_t *off, const uint64_t *len, const uint64_t *id,
                           const uint64_t *sub, uint64_t n_items, uint8_t *out, uint64_t cap)
{
    MetaData *md = MetaDataNew();
    MemBuffer *mb = MemBufferNew(BRBDATA_THREAD_UNSAFE, REF_GROW);
    for (uint64_t i = 0; i < n_items; i++)
        MetaDataItemAdd(md, id[i], sub[i], (void *)(data + off[i]), len[i]);
    MetaDataPack(md, mb);
    MetaDataDestroy(md);
    return mb_take(mb, out, cap);
}

/* An item whose stored size is the largest unsigned long makes MetaDataUnpack's `sz + 1` wrap to 0 and
 * the call digest memory it does not own.  Such a pack is not given to the reference: 0 = do not call. */
static int unpack_is_defined(const uint8_t *b, uint64_t size)
{
    if (size < sizeof(MetaDataHeader))
        return 1;                       /* the header read stays inside the MemBuffer's zeroed room */
    MetaDataHeader h;
    memcpy(&h, b, sizeof(h));
    if (memcmp(h.str, METADATA_MAGIC_HEADER, METADATA_MAGIC_HEADER_SZ))
        return 1;
    uint64_t pos = sizeof(h);
    for (int i = 0; i < h.item_count; i++) {
        uint64_t remaining = size - pos;
        if (remaining < sizeof(MetaDataItem))
            return 1;
        unsigned long sz;
        memcpy(&sz, b + pos + 2 * sizeof(long), sizeof(sz));
        if (sz == ~0UL)
            return 0;
        remaining -= METADATA_ITEM_RAW_SZ;
        if (remaining < sz + METADATA_UNIT_SEPARATOR_SZ)
            return 1;
        pos += METADATA_ITEM_RAW_SZ + sz;
        if (memcmp(b + pos, METADATA_UNIT_SEPARATOR, METADATA_UNIT_SEPARATOR_SZ))
            return 1;
        pos += METADATA_UNIT_SEPARATOR_SZ;
        if (pos == size)
            return 1;
    }
    return 1;
}

/* MetaDataUnpack of a MemBuffer holding the pack.  info[0..4] = return code, unpacker_info's error_code,
 * cur_offset, cur_remaining, cur_needed; info[5] = items the MetaData holds afterwards.  items[4 * k ..]
 * = item_id, item_sub_id, sz and the data's offset in the pack of item k < max_items.  Returns 1, or 0
 * when the pack was not given to the reference (see unpack_is_defined). */
int ref_metadata_unpack(const uint8_t *pack, uint64_t size, uint64_t *info, uint64_t *items, uint64_t max_items)
{
    if (!unpack_is_defined(pack, size))
        return 0;
    MetaData *md = MetaDataNew();
    MemBuffer *mb = MemBufferNew(BRBDATA_THREAD_UNSAFE, REF_GROW);
    MetaDataUnpackerInfo ui;
    memset(&ui, 0, sizeof(ui));
    MemBufferAdd(mb, pack, size);
    int rc = MetaDataUnpack(md, mb, &ui);
    info[0] = (uint64_t)(int64_t)rc;
    info[1] = (uint64_t)(int64_t)ui.error_code;
    info[2] = ui.cur_offset;
    info[3] = ui.cur_remaining;
    info[4] = ui.cur_needed;
    info[5] = (uint64_t)(int64_t)md->items.count;
    for (int k = 0; k < md->items.count && (uint64_t)k < max_items; k++) {
        MetaDataItem *it = MemArenaGrabByID(md->items.arena, k);
        items[4 * k + 0] = it->item_id;
        items[4 * k + 1] = it->item_sub_id;
        items[4 * k + 2] = it->sz;
        items[4 * k + 3] = (uint64_t)((char *)it->ptr - (char *)mb->data);
    }
    MetaDataDestroy(md);
    MemBufferDestroy(mb);
    return 1;
}
