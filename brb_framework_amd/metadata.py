"""MetaData packs on the GPU entry points: the format of MetaDataPack / MetaDataUnpack
(libbrb_core/data/utils/meta_data.c:104-328, libbrb_data.h:291-330, LP64), built and checked many at
a time.  The mmap'd file cache (ev_kq_file_mapped.c:2493, :2869) and the encrypted K/V files keep
their objects in this format, so a cache warm-up validates thousands of packs at once.

A pack is a 64-byte header {int version = 0; int item_count; unsigned long size; "BRB_META"; the MD5
of the items' data (MetaDataHeaderLoadData, :397-433); 24 zero bytes}, then per item
{unsigned long item_id, item_sub_id, sz; sz data bytes; 0x1F}; size = sum of (sz + 24 + 1).

pack_items_batch builds the packs on the GPU: it gathers the items' bytes and the item lists into
numpy arrays and makes one BRB_MetaDataPackBatch call (one GPU lane per pack, every item byte read
once for both the digest and the pack; crypto.metadata_pack_batch is the call itself, for callers
whose items already lie in one buffer, on the host or in HBM).  pack_sizes gives the packs' lengths
from the item lists.  pack_batch is the earlier host-side builder: it lays packs out back to back on
the host and computes every header digest with one BRB_MD5BatchSegments call whose segments are the
item data inside the packed buffer itself.
unpack_batch is BRB_MetaDataUnpackBatch (one GPU lane per pack; reference return codes and
MetaDataUnpackerInfo fields, quirks included -- include/brb_crypto.h).  unpack_items_batch is
BRB_MetaDataUnpackItemsBatch: the same check, and the item table the reference's unpack builds (offset,
length, id and sub-id of every MetaDataItemAdd call) written by the walking lane, in the arrays the pack
and segment-digest calls take.  items() lists one pack's items on the host, for packs unpack_batch
accepted."""
import struct

import numpy as np

from . import crypto

HEADER = 64
ITEM_RAW = 24
MAGIC = b"BRB_META"
CANARY = 0x1F
UNPACK_SUCCESS = 7
UNPACK_CODES = {0: "FAILED_INVALID_HEADER_MAGIC", 1: "FAILED_UNINITIALIZED", 2: "FAILED_NO_RAWDATA",
                3: "FAILED_CORRUPTED_CANARY", 4: "FAILED_DIGEST_INVALID", 5: "FAILED_NEED_MORE_DATA_METAITEM",
                6: "FAILED_NEED_MORE_DATA_OBJECT", 7: "SUCCESS"}   # MetaDataUnpackReturnCode, libbrb_data.h:299-310


def pack_size(items) -> int:
    return HEADER + sum(ITEM_RAW + len(d) + 1 for _, _, d in items)


def pack_batch(packs):
    """MetaDataPack of every MetaData in `packs` (each a list of (item_id, item_sub_id, data bytes)).
    Returns (buf, offsets, lengths): pack i is buf[offsets[i] : offsets[i] + lengths[i]].
    Built on the host, digests by BRB_MD5BatchSegments; pack_items_batch returns the same triple from
    one BRB_MetaDataPackBatch call."""
    sizes = np.array([pack_size(items) for items in packs], np.uint64)
    offsets = np.zeros(len(packs), np.uint64)
    if len(packs) > 1:
        offsets[1:] = np.cumsum(sizes)[:-1]
    buf = np.zeros(int(sizes.sum()) if len(packs) else 1, np.uint8)
    seg_off, seg_len, first = [], [], [0]
    for p, items in enumerate(packs):
        o = int(offsets[p])
        body = sum(ITEM_RAW + len(d) + 1 for _, _, d in items)
        buf[o:o + 24] = np.frombuffer(struct.pack("<iiQ8s", 0, len(items), body, MAGIC), np.uint8)
        o += HEADER
        for item_id, sub_id, data in items:
            buf[o:o + ITEM_RAW] = np.frombuffer(struct.pack("<QQQ", item_id, sub_id, len(data)), np.uint8)
            o += ITEM_RAW
            seg_off.append(o)
            seg_len.append(len(data))
            buf[o:o + len(data)] = np.frombuffer(data, np.uint8)
            o += len(data)
            buf[o] = CANARY
            o += 1
        first.append(len(seg_off))
    if len(packs):
        digests = crypto.md5_batch_segments(buf, np.array(seg_off, np.uint64), np.array(seg_len, np.uint32),
                                            np.array(first, np.uint64))
        for p in range(len(packs)):
            o = int(offsets[p]) + 24
            buf[o:o + 16] = digests[p]
    return buf, offsets, sizes.astype(np.uint32)


def pack_sizes(item_lengths, pack_first_item):
    """Bytes of every pack BRB_MetaDataPackBatch writes: HEADER + sum(item length + 25) over items
    pack_first_item[p] .. pack_first_item[p + 1] - 1 (uint64[n])."""
    first = np.asarray(pack_first_item, np.uint64).astype(np.int64)
    cum = np.zeros(len(item_lengths) + 1, np.uint64)
    np.cumsum(np.asarray(item_lengths, np.uint64) + np.uint64(ITEM_RAW + 1), out=cum[1:])
    return cum[first[1:]] - cum[first[:-1]] + np.uint64(HEADER)


def pack_items_batch(packs, stream=None, all_devices=False):
    """MetaDataPack of every MetaData in `packs` (each a list of (item_id, item_sub_id, data bytes)) by
    one BRB_MetaDataPackBatch call.  Returns (buf, offsets, lengths) as pack_batch does: pack i is
    buf[offsets[i] : offsets[i] + lengths[i]], the packs back to back."""
    items = [it for p in packs for it in p]
    lens = np.fromiter((len(d) for _, _, d in items), np.uint32, len(items))
    ids = np.array([i for i, _, _ in items], np.uint64)
    subs = np.array([s for _, s, _ in items], np.uint64)
    first = np.zeros(len(packs) + 1, np.uint64)
    np.cumsum(np.fromiter((len(p) for p in packs), np.uint64, len(packs)), out=first[1:])
    item_off = np.zeros(len(items), np.uint64)
    if len(items) > 1:
        item_off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    data = np.frombuffer(b"".join(d for _, _, d in items) + b"\0", np.uint8)
    sizes = pack_sizes(lens, first)
    offsets = np.zeros(len(packs), np.uint64)
    if len(packs) > 1:
        offsets[1:] = np.cumsum(sizes)[:-1]
    buf = np.zeros(int(sizes.sum()) if len(packs) else 1, np.uint8)
    crypto.metadata_pack_batch(data, item_off, lens, ids, subs, first, buf, offsets, stream=stream,
                               all_devices=all_devices)
    return buf, offsets, sizes.astype(np.uint32)


def unpack_batch(buf, offsets, lengths, stream=None, all_devices=False):
    """BRB_MetaDataUnpackBatch: one BRB_MetaDataUnpackInfo (error_code, item_count, cur_offset,
    cur_remaining, cur_needed) per pack, error_code a MetaDataUnpackReturnCode (7 = SUCCESS)."""
    return crypto.metadata_unpack_batch(buf, np.asarray(offsets, np.uint64), np.asarray(lengths, np.uint32),
                                        stream=stream, all_devices=all_devices)


def max_items_bound(lengths):
    """Slots that always hold a pack's item table: an added item takes at least 25 bytes after the header,
    (len - 64) // 25; a pack shorter than its header adds at most one (the zeros past its end)."""
    n = np.asarray(lengths, np.int64)
    return np.where(n >= HEADER, (n - HEADER) // (ITEM_RAW + 1), 1).astype(np.uint64)


def unpack_items_batch(buf, offsets, lengths, max_items=None, stream=None, all_devices=False):
    """BRB_MetaDataUnpackItemsBatch: unpack_batch plus the item table MetaDataUnpack builds (one entry per
    MetaDataItemAdd call, reference order).  Every pack gets max_items table slots, or with max_items None
    the max_items_bound of its length, which always suffices.  Returns (info, items_added, pack_first_slot,
    item_offsets, item_lengths, item_ids, item_sub_ids): pack p's items are slots pack_first_slot[p] ..
    + min(items_added[p], its slot count) - 1 of the four arrays (item_offsets: offsets in `buf` of each
    item's data); items_added[p] above the slot count means the table of pack p is cut short; slots past
    items_added[p] hold 0.  With a CUDA tensor `buf` (offsets int64, lengths int32 tensors) everything
    returned is a tensor on its device; the slot layout is made on the host (max_items None: from the
    lengths, read back once) and uploaded, the packs and the table stay in HBM."""
    n = len(offsets)
    dev = crypto._is_torch(buf)
    if max_items is None:
        per = max_items_bound(lengths.cpu().numpy() if dev else lengths)
    else:
        per = np.full(n, int(max_items), np.uint64)
    first = np.zeros(n + 1, np.uint64)
    np.cumsum(per, out=first[1:])
    slots = int(first[n])
    if dev:
        import torch
        z = lambda dt: torch.zeros(slots, dtype=dt, device=buf.device)
        table = [z(torch.int64), z(torch.int32), z(torch.int64), z(torch.int64)]
        first = torch.from_numpy(first.view(np.int64)).to(buf.device)
    else:
        offsets, lengths = np.asarray(offsets, np.uint64), np.asarray(lengths, np.uint32)
        table = [np.zeros(slots, np.uint64), np.zeros(slots, np.uint32), np.zeros(slots, np.uint64),
                 np.zeros(slots, np.uint64)]
    info, added = crypto.metadata_unpack_items_batch(buf, offsets, lengths, *table, first, stream=stream,
                                                     all_devices=all_devices)
    return (info, added, first, *table)


def items(pack: bytes):
    """The (item_id, item_sub_id, data) items of a pack unpack_batch accepted (MetaDataItemAdd order)."""
    count = struct.unpack_from("<i", pack, 4)[0]
    out, o = [], HEADER
    for _ in range(max(count, 0)):
        if o == len(pack):
            break
        item_id, sub_id, sz = struct.unpack_from("<QQQ", pack, o)
        o += ITEM_RAW
        out.append((item_id, sub_id, bytes(pack[o:o + sz])))
        o += sz + 1
    return out
