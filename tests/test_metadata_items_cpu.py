"""BRB_MetaDataUnpackItemsBatch without a GPU: the expected item table, and the call's refusals.

The oracle's metadata_unpack returns the five MetaDataUnpackerInfo fields only, so the table the GPU
tests (tests/test_metadata_items.py) compare against comes from py_unpack_items below: py_unpack of
tests/test_metadata.py, extended to record (offset in the pack, sz, item_id, item_sub_id) where the
reference calls MetaDataItemAdd (meta_data.c:246-248).  Here its five-tuple is pinned to the oracle's
on the 3 000-pack corpus of that file's generator and mutations, and the corpus is shown to hold the
cases the table's rules are about.  The argument checks run before any device work, so they answer
-1 on a machine with no GPU.
"""
import functools
import hashlib
import importlib.util
import os
import struct

import numpy as np

_spec = importlib.util.spec_from_file_location("metadata_cases", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                             "test_metadata.py"))
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)

M64 = 1 << 64


def py_unpack_items(pack: bytes):
    """test_metadata.py's py_unpack with the item table: -> ((code, items, cur_offset, cur_remaining,
    cur_needed), [(offset, sz, item_id, item_sub_id), ...]), one entry per MetaDataItemAdd call."""
    size = len(pack)
    byte = lambda p: pack[p] if p < size else 0
    field = lambda p, n: bytes(byte(p + k) for k in range(n))
    if field(16, 8) != b"BRB_META":                                   # :183-195
        return (0, 0, 0, 0, 0), []
    count = struct.unpack("<i", field(4, 4))[0]
    off, rem, need, n, h, table = 64, 0, 0, 0, hashlib.md5(), []      # :198-199
    for _ in range(max(count, 0)):                                    # :202
        rem = (size - off) % M64                                      # :213
        if rem < 32:                                                  # :216-224 sizeof(MetaDataItem)
            return (5, n, off, rem, (32 - rem) % M64), table
        item_id, sub_id, sz = struct.unpack("<QQQ", field(off, 24))
        off, rem = off + 24, (rem - 24) % M64                          # :227-232
        if rem < (sz + 1) % M64 or sz > size:                         # :237-246
            return (6, n, off, rem, (sz + 1 - rem) % M64), table
        table.append((off, sz, item_id, sub_id))                      # :246-248 MetaDataItemAdd
        h.update(field(off, sz))                                      # :249-254
        off, rem = off + sz, (rem - sz) % M64
        if byte(off) != 0x1F:                                         # :258-268
            return (3, n, off, rem, need), table
        off, rem, n = off + 1, (rem - 1) % M64, n + 1                   # :271-277
        if off == size:                                               # :280-281
            break
    return (7 if h.digest() == field(24, 16) else 4, n, off, rem, need), table   # :285-298


@functools.lru_cache(maxsize=None)
def walked_corpus(seed, n):
    """(packs, [py_unpack_items(pack)]) of test_metadata.corpus(seed, n), computed once per run."""
    packs = cases.corpus(seed, n)
    return packs, [py_unpack_items(p) for p in packs]


def test_walker_agrees_with_oracle_and_corpus_holds_the_cases(orc):
    packs, walked = walked_corpus(2, 3000)
    canary_nonempty = digest_full = object_after_item = 0
    for p, (five, table) in zip(packs, walked):
        assert five == orc.metadata_unpack(p) == cases.py_unpack(p), p.hex()
        code, items = five[0], five[1]
        assert len(table) == items + (code == 3), p.hex()            # items_added by construction
        for k, (off, sz, _, _) in enumerate(table):                    # MetaDataItemAdd order: ascending, disjoint
            assert off >= (table[k - 1][0] + table[k - 1][1] + 25 if k else 88) and sz <= len(p)
        if code == 0:
            assert table == []
        canary_nonempty += code == 3 and len(table) >= 1
        count = struct.unpack_from("<i", p, 4)[0] if len(p) >= 8 else 0
        digest_full += code == 4 and len(table) >= 1 and len(table) == count
        object_after_item += code == 6 and len(table) >= 1
    assert canary_nonempty >= 10 and digest_full >= 10 and object_after_item >= 10, \
        (canary_nonempty, digest_full, object_after_item)


def test_walker_on_valid_packs_is_the_construction():
    rng = np.random.default_rng(61)
    for _ in range(300):
        items = cases.random_items(rng)
        if items and len(items[-1][2]) < 7:
            items[-1] = (items[-1][0], items[-1][1], bytes(7))
        five, table = py_unpack_items(cases.build(items))
        assert five[0] == 7
        pos, want = 64, []
        for i, s, d in items:
            want.append((pos + 24, len(d), i, s))
            pos += 25 + len(d)
        assert table == want


def test_walker_quirks():
    # a pack shorter than its header whose magic holds: the zeros past its end are one empty item with no canary
    p = cases.build([(1, 2, b"0123456789")])[:40]
    assert py_unpack_items(p) == ((3, 0, 88, (40 - 88) % M64, 0), [(88, 0, 0, 0)])
    # a last item of 0..6 bytes is not added (code 5); an sz beyond the pack is not added (code 6)
    for n in range(7):
        five, table = py_unpack_items(cases.build([(9, 9, bytes(30)), (1, 2, bytes(n))]))
        assert five[0] == 5 and table == [(88, 30, 9, 9)]
    two = [(9, 9, bytes(30)), (1, 2, bytes(20))]
    b, pos = bytearray(cases.build(two)), cases.item_field_pos(two, 1)
    b[pos:pos + 8] = struct.pack("<Q", len(b) + 1)
    five, table = py_unpack_items(bytes(b))
    assert five[0] == 6 and table == [(88, 30, 9, 9)]


def test_max_items_bound_holds_on_the_corpus():
    from brb_framework_amd import metadata
    packs, walked = walked_corpus(2, 3000)
    bound = metadata.max_items_bound(np.array([len(p) for p in packs], np.uint32))
    assert bound.dtype == np.uint64
    assert all(len(t) <= int(b) for (_, t), b in zip(walked, bound))
    assert metadata.max_items_bound([63, 64, 88, 89, 64 + 50]).tolist() == [1, 0, 0, 1, 2]


# ---- the entry point without a device ------------------------------------------------------------------
def small_call():
    rng = np.random.default_rng(62)
    packs = [cases.build(cases.random_items(rng)) for _ in range(6)]
    buf, offs, lens = cases.scatter(rng, packs)
    first = np.arange(7, dtype=np.uint64) * np.uint64(8)
    table = [np.full(48, 0xA5, np.uint64), np.full(48, 0xA5, np.uint32), np.full(48, 0xA5, np.uint64),
             np.full(48, 0xA5, np.uint64)]
    info = np.zeros(6, [("error_code", "<i4"), ("item_count", "<u4"), ("cur_offset", "<u8"), ("cur_remaining", "<u8"),
                        ("cur_needed", "<u8")])
    added = np.full(6, 0xA5, np.uint32)
    return [buf, offs, lens, info, *table, first, added]


def raw_args(arrays, n=6, flags=0):
    a = [x.ctypes.data for x in arrays]
    return a[:3] + [n] + a[3:] + [flags, None]


def test_symbol_is_exported_and_declared(brb):
    from brb_framework_amd import crypto
    assert "BRB_MetaDataUnpackItemsBatch" in brb.exported_symbols()
    sig = {name: args for name, _, args in crypto._SIGNATURES}
    assert len(sig["BRB_MetaDataUnpackItemsBatch"]) == 13
    assert brb.lib().BRB_MetaDataUnpackItemsBatch.argtypes == sig["BRB_MetaDataUnpackItemsBatch"]
    with open(crypto.HEADER_PATH) as f:
        assert "int BRB_MetaDataUnpackItemsBatch(" in f.read()


def test_bad_arguments_are_refused_before_any_device_work(brb):
    """-1 (never 0, the answer of a machine without a GPU) and a reason for a NULL pack_first_slot, a NULL
    items_added, a NULL item array (and every other pointer) and a decreasing pack_first_slot; nothing is
    written; an empty batch is done."""
    L = brb.lib()
    arrays = small_call()
    before = [x.copy() for x in arrays]
    for i in (0, 1, 2, 4, 5, 6, 7, 8, 9, 10):            # every pointer: raw_args puts n at index 3
        a = raw_args(arrays)
        a[i] = None
        assert L.BRB_MetaDataUnpackItemsBatch(*a) == -1, i
        assert b"NULL" in L.BRB_CryptoGPU_LastError()
    bad = arrays[8].copy()
    bad[3] = bad[2] - np.uint64(1)                        # decreases at pack 2
    a = raw_args(arrays)
    a[9] = bad.ctypes.data
    assert L.BRB_MetaDataUnpackItemsBatch(*a) == -1
    assert b"pack_first_slot is not non-decreasing at 2" in L.BRB_CryptoGPU_LastError()
    wrap = arrays[1].copy()
    wrap[4] = np.uint64(M64 - 5)                          # a span error, as in BRB_MetaDataUnpackBatch
    a = raw_args(arrays)
    a[1] = wrap.ctypes.data
    assert L.BRB_MetaDataUnpackItemsBatch(*a) == -1
    assert b"wraps" in L.BRB_CryptoGPU_LastError()
    assert L.BRB_MetaDataUnpackItemsBatch(*raw_args(arrays, flags=brb.BATCH_DEVICE | brb.BATCH_ALL_DEVICES)) == -1
    assert b"ALL_DEVICES" in L.BRB_CryptoGPU_LastError()
    assert L.BRB_MetaDataUnpackItemsBatch(*raw_args(arrays, n=1 << 33)) == -1
    assert b"split the batch" in L.BRB_CryptoGPU_LastError()
    assert L.BRB_MetaDataUnpackItemsBatch(*raw_args(arrays, n=0)) == 1
    assert L.BRB_MetaDataUnpackItemsBatch(None, None, None, 0, None, None, None, None, None, None, None, 0, None) == 1
    for x, y in zip(arrays, before):
        assert np.array_equal(x, y)                       # none of these wrote anything


def test_valid_call_without_gpu_is_refused_not_computed(brb):
    """A valid host-mode call returns 0 with a reason when no device is usable and leaves its outputs alone;
    with a device it returns 1 and the table is the walker's."""
    L = brb.lib()
    arrays = small_call()
    before = [x.copy() for x in arrays]
    rc = L.BRB_MetaDataUnpackItemsBatch(*raw_args(arrays))
    if brb.gpu_available():
        assert rc == 1
        buf, offs, lens, info, ioff, ilen, iid, isub, first, added = arrays
        for p in range(6):
            o = int(offs[p])
            five, table = py_unpack_items(buf[o:o + int(lens[p])].tobytes())
            assert tuple(int(x) for x in info[p].tolist()) == five and int(added[p]) == len(table)
            s = int(first[p])
            got = list(zip(ioff[s:s + len(table)].tolist(), ilen[s:s + len(table)].tolist(),
                           iid[s:s + len(table)].tolist(), isub[s:s + len(table)].tolist()))
            assert got == [(o + a, b, c, d) for a, b, c, d in table]
    else:
        assert rc == 0 and L.BRB_CryptoGPU_LastError().strip()
        for x, y in zip(arrays, before):
            assert np.array_equal(x, y)
