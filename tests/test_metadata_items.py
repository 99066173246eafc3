"""BRB_MetaDataUnpackItemsBatch on the GPU: BRB_MetaDataUnpackBatch plus the item table the reference's
MetaDataUnpack builds (one entry per MetaDataItemAdd call, meta_data.c:246-248).

Expected values: `info` is the plain call's result and the walker's five fields (pinned to the oracle in
tests/test_metadata_items_cpu.py, and asserted against it again here on every pack used); the table is
the walker's (py_unpack_items of that file), and for valid packs the items they were built from.  Every
call is laid out by lay_out(): the four item arrays and items_added are filled with sentinels, the
call's slots start GUARD entries into the arrays and end GUARD entries before their end, and the whole
arrays are compared with an expected image -- so an unused slot, a slot of another pack or a guard entry
that changed fails the test.  Host, device and all-devices modes; seg_line 0 (per-lane kernel), 1 (line
kernel, three and two ring slots) and 2 (wave pairs).  No call passes a range outside its buffers.
"""
import importlib.util
import os

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("metadata_items_walk", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                                  "test_metadata_items_cpu.py"))
walk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(walk)
cases = walk.cases

M64 = 1 << 64
GUARD = 37
S64, S32 = 0xA5C3A5C3A5C3A5C3, 0xA5C3A5C3
VARIANTS = [(1, 3), (1, 2), (2, 0), (0, 0)]          # (seg_line, line_slots), as tests/test_metadata.py


@pytest.fixture()
def gpu(brb):
    assert brb.gpu_available(), brb.lib().BRB_CryptoGPU_LastError()
    return brb


def to_dev(a):
    import torch
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def infos_as_tuples(info):
    return [tuple(int(x) for x in r) for r in info.tolist()]


class Call:
    """One call's slot layout, its sentinel-filled outputs' expected images and its expected info."""


def lay_out(packs, walked, offs, caps):
    """walked[p] = py_unpack_items(packs[p]); offs[p]: the pack's offset in the call's buffer; caps[p]: its
    slot count."""
    c = Call()
    c.first = np.full(len(packs) + 1, GUARD, np.uint64)
    c.first[1:] += np.cumsum(np.asarray(caps, np.uint64))
    total = int(c.first[-1]) + GUARD
    c.want = [np.full(total, S64, np.uint64), np.full(total, S32, np.uint32), np.full(total, S64, np.uint64),
              np.full(total, S64, np.uint64)]
    c.added = np.array([len(t) for _, t in walked], np.uint32)
    for p, (_, table) in enumerate(walked):
        s = int(c.first[p])
        for j, (o, sz, i, sub) in enumerate(table[:int(caps[p])]):
            c.want[0][s + j], c.want[1][s + j], c.want[2][s + j], c.want[3][s + j] = int(offs[p]) + o, sz, i, sub
    c.info = [five for five, _ in walked]
    return c


def sentinels(c):
    return [np.full(w.size, S32 if w.dtype == np.uint32 else S64, w.dtype) for w in c.want]


def run(brb, c, buf, offs, lens, mode):
    """The call on fresh sentinel-filled arrays; -> (info tuples, items_added, the four arrays), on the host."""
    table = sentinels(c)
    added = np.full(len(offs), S32, np.uint32)
    if mode == "device":
        import torch
        t = [to_dev(a) for a in (buf, offs, lens, *table, c.first, added)]
        torch.cuda.synchronize()
        info, _ = brb.metadata_unpack_items_batch(*t[:3], *t[3:7], t[7], items_added=t[8])
        plain = brb.metadata_unpack_batch(*t[:3])
        as_info = lambda x: x.cpu().numpy().reshape(-1).view(brb.METADATA_INFO_DTYPE)
        info, plain = as_info(info), as_info(plain)
        table, added = [x.cpu().numpy().view(w.dtype) for x, w in zip(t[3:7], c.want)], t[8].cpu().numpy().view(np.uint32)
    else:
        kw = {"all_devices": True} if mode == "all" else {}
        info, _ = brb.metadata_unpack_items_batch(buf, offs, lens, *table, c.first, items_added=added, **kw)
        plain = brb.metadata_unpack_batch(buf, offs, lens, **kw)
    assert infos_as_tuples(info) == infos_as_tuples(plain)
    return infos_as_tuples(info), added, table


def check(brb, c, buf, offs, lens, modes=("host", "device", "all")):
    for mode in modes:
        if mode == "all":
            with brb.TestOption("devices", 3):           # three concurrent parts, also on a one-GPU box
                info, added, table = run(brb, c, buf, offs, lens, mode)
        else:
            info, added, table = run(brb, c, buf, offs, lens, mode)
        assert info == c.info, mode
        assert np.array_equal(added, c.added), (mode, np.flatnonzero(added != c.added)[:5])
        for name, got, want in zip(("item_offsets", "item_lengths", "item_ids", "item_sub_ids"), table, c.want):
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, f"{mode}: {name} differs in {bad.size} slots, the first {int(bad[0])} " \
                                  f"(pack {int(np.searchsorted(c.first, bad[0], side='right')) - 1}): " \
                                  f"{int(got[bad[0]]):#x} for {int(want[bad[0]]):#x}"


def walked(orc, packs):
    out = [walk.py_unpack_items(p) for p in packs]
    for p, (five, _) in zip(packs, out):
        assert five == orc.metadata_unpack(p), p.hex()
    return out


def place(packs, offsets):
    """The packs at the given (ascending, non-overlapping) offsets of one buffer of 0xEE bytes."""
    buf = np.full(int(offsets[-1]) + len(packs[-1]) + 1, 0xEE, np.uint8)
    for o, p in zip(offsets, packs):
        buf[int(o):int(o) + len(p)] = np.frombuffer(p, np.uint8)
    return buf, np.array(offsets, np.uint64), np.array([len(p) for p in packs], np.uint32)


def variant(brb, seg_line, slots):
    import contextlib
    st = contextlib.ExitStack()
    st.enter_context(brb.TestOption("seg_line", seg_line))
    st.enter_context(brb.TestOption("line_slots", slots))
    return st


def rand_bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def rand_id(rng):
    return int(rng.integers(0, M64, dtype=np.uint64))


# ---- the corpus ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seg_line,slots", VARIANTS)
def test_items_corpus_all_modes(gpu, orc, seg_line, slots):
    """1 000 valid and mutated packs (every return code) 0..7 bytes apart, the first at offset 1 234 so that
    host mode's rebasing shows in item_offsets; (len - 64) / 25 slots per pack, which always suffice."""
    from brb_framework_amd import metadata
    packs, wk = walk.walked_corpus(2, 3000)
    packs, wk = packs[:1000], wk[:1000]
    for p, (five, _) in zip(packs, wk):
        assert five == orc.metadata_unpack(p)
    buf, offs, lens = cases.scatter(np.random.default_rng(63), packs)
    buf = np.concatenate([np.full(1234, 0xEE, np.uint8), buf])
    offs = offs + np.uint64(1234)
    caps = metadata.max_items_bound(lens)
    c = lay_out(packs, wk, offs, caps)
    assert {five[0] for five in c.info} == {0, 3, 4, 5, 6, 7} and int(c.added.max()) >= 5
    assert all(int(a) <= int(k) for a, k in zip(c.added, caps))
    with variant(gpu, seg_line, slots):
        check(gpu, c, buf, offs, lens)


@pytest.mark.gpu
@pytest.mark.parametrize("seg_line,slots", VARIANTS)
def test_items_group_edges(gpu, orc, seg_line, slots):
    """1, 63, 64, 65 and 130 packs: a partial group, exactly one, and more than one group per wave."""
    packs, wk = walk.walked_corpus(2, 3000)
    with variant(gpu, seg_line, slots):
        for n in (1, 63, 64, 65, 130):
            ps, ws = packs[1000:1000 + n], wk[1000:1000 + n]
            buf, offs, lens = cases.scatter(np.random.default_rng(64 + n), ps)
            c = lay_out(ps, ws, offs, [len(t) for _, t in ws])           # exact slot counts
            check(gpu, c, buf, offs, lens, modes=("host", "device"))


# ---- where the fields lie ----------------------------------------------------------------------------------
def straddling_packs(rng):
    """For t = 104 .. 127: a pack (at a 128-byte line's start) whose items 1 and 2 have their 24-byte field block
    at byte t of a line -- item 0 holds t - 89 bytes, item 1 103 -- so item_id (t >= 121), item_sub_id (t >= 113)
    or sz (t >= 105) straddle the line's end."""
    out = []
    for t in range(104, 128):
        items = [(rand_id(rng), rand_id(rng), rand_bytes(rng, n)) for n in (t - 89, 103, 9)]
        assert (cases.item_field_pos(items, 1) - 16) % 128 == t == (cases.item_field_pos(items, 2) - 16) % 128
        out.append(items)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("seg_line,slots", VARIANTS)
def test_items_fields_across_lines(gpu, orc, seg_line, slots):
    """Field blocks at every byte position 104 .. 127 of a 128-byte line (the ids straddle the boundary), with
    the packs at buffer offsets 0 mod 128 and 127 mod 128; the table equals the items the packs were built from."""
    rng = np.random.default_rng(65)
    lists = straddling_packs(rng)
    packs = [cases.build(it) for it in lists]
    wk = walked(orc, packs)
    for items, (five, table) in zip(lists, wk):
        assert five[0] == 7 and [(sz, i, s) for _, sz, i, s in table] == [(len(d), i, s) for i, s, d in items]
    with variant(gpu, seg_line, slots):
        for shift in (0, 127):
            offsets = [256 + 512 * k + shift for k in range(len(packs))]
            buf, offs, lens = place(packs, offsets)
            c = lay_out(packs, wk, offs, [3] * len(packs))
            check(gpu, c, buf, offs, lens, modes=("host", "device"))


# ---- special items -----------------------------------------------------------------------------------------
def special_packs(rng):
    item = lambda n: (rand_id(rng), rand_id(rng), rand_bytes(rng, n))
    packs = [cases.build([item(0), item(20)]),                              # zero-length items ...
             cases.build([item(11), item(0), item(0), item(0), item(30)]),  # ... three in a row
             cases.build([item(0)] * 4 + [item(8)]),
             cases.build([]),                                                # no items
             cases.build([item(2) for _ in range(40)])]                      # 40 items of 2 bytes (the last: code 5)
    packs += [cases.build([item(50), item(17), item(n)]) for n in range(7)]  # a last item of 0..6 bytes: code 5
    for j in (0, 2):                                                         # a flipped canary on item 0 / the last
        items = [item(33), item(0), item(21)]
        b = bytearray(cases.build(items))
        b[cases.item_field_pos(items, j) + 8 + len(items[j][2])] ^= 0x40
        packs.append(bytes(b))
    items = [item(40), item(25), item(19)]                                   # an sz larger than the pack
    b = bytearray(cases.build(items))
    pos = cases.item_field_pos(items, 1)
    b[pos:pos + 8] = (len(b) + 1).to_bytes(8, "little")
    packs.append(bytes(b))
    b[pos:pos + 8] = (M64 - 1).to_bytes(8, "little")                          # sz + 1 wraps to 0
    packs.append(bytes(b))
    b = bytearray(cases.build(items))                                        # a data byte flipped: the digest fails,
    b[cases.item_field_pos(items, 2) + 8] ^= 1                               # the table is full
    packs.append(bytes(b))
    packs.append(cases.build(items)[:40])                                    # shorter than its header, magic intact
    return packs


@pytest.mark.gpu
@pytest.mark.parametrize("seg_line,slots", VARIANTS)
def test_items_special_items(gpu, orc, seg_line, slots):
    rng = np.random.default_rng(66)
    packs = special_packs(rng)
    wk = walked(orc, packs)
    codes = [five[0] for five, _ in wk]
    added = [len(t) for _, t in wk]
    assert codes[:5] == [7, 7, 7, 7, 5] and added[:5] == [2, 5, 5, 0, 39]
    assert codes[5:12] == [5] * 7 and added[5:12] == [2] * 7              # the short last item is not in the table
    assert codes[12:14] == [3, 3] and added[12:14] == [1, 3]               # item_count + 1
    assert [five[1] for five, _ in wk[12:14]] == [0, 2]
    assert codes[14:16] == [6, 6] and added[14:16] == [1, 1]
    assert codes[16] == 4 and added[16] == 3
    assert wk[17] == ((3, 0, 88, (40 - 88) % M64, 0), [(88, 0, 0, 0)])
    buf, offs, lens = cases.scatter(rng, packs)
    c = lay_out(packs, wk, offs, [max(a, 1) for a in added])
    with variant(gpu, seg_line, slots):
        check(gpu, c, buf, offs, lens)


# ---- fewer slots than items ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seg_line,slots", VARIANTS)
def test_items_overflow(gpu, orc, seg_line, slots):
    """A 5-item pack between two others with 0, 1 and 4 slots: the first `count` entries are written,
    items_added is 5, the neighbours' slots and the sentinels are intact."""
    rng = np.random.default_rng(67)
    item = lambda n: (rand_id(rng), rand_id(rng), rand_bytes(rng, n))
    packs = [cases.build([item(30), item(12)]), cases.build([item(n) for n in (9, 0, 140, 3, 25)]),
             cases.build([item(7), item(8), item(70)])]
    wk = walked(orc, packs)
    assert [five[0] for five, _ in wk] == [7, 7, 7] and [len(t) for _, t in wk] == [2, 5, 3]
    buf, offs, lens = cases.scatter(rng, packs)
    with variant(gpu, seg_line, slots):
        for count in (0, 1, 4):
            c = lay_out(packs, wk, offs, [2, count, 3])
            assert int(c.added[1]) == 5
            check(gpu, c, buf, offs, lens)


# ---- groups wider than 2 GiB ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seg_line", [1, 2])
def test_items_wide_group(gpu, orc, seg_line):
    """Two copies of a small corpus in one device buffer, more than 2 GiB apart, the packs read from them in
    turn: every group's lines span more than 2 GiB, so it takes the per-lane walk inside the line kernel."""
    import torch
    packs, wk = walk.walked_corpus(2, 3000)
    packs, wk = packs[2000:2200], wk[2000:2200]
    for p, (five, _) in zip(packs, wk):
        assert five == orc.metadata_unpack(p)
    buf, offs, lens = cases.scatter(np.random.default_rng(68), packs)
    far = (1 << 31) + 4099
    d = torch.zeros(far + buf.size, dtype=torch.uint8, device="cuda")
    src = torch.from_numpy(buf).cuda()
    d[: buf.size] = src
    d[far:] = src
    offs[1::2] += np.uint64(far)
    c = lay_out(packs, wk, offs, [len(t) + 1 for _, t in wk])
    table = [to_dev(a) for a in sentinels(c)]
    added = to_dev(np.full(len(packs), S32, np.uint32))
    with gpu.TestOption("seg_line", seg_line):
        info, _ = gpu.metadata_unpack_items_batch(d, to_dev(offs), to_dev(lens), *table, to_dev(c.first), items_added=added)
    info = info.cpu().numpy().reshape(-1).view(gpu.METADATA_INFO_DTYPE)
    assert infos_as_tuples(info) == c.info
    assert np.array_equal(added.cpu().numpy().view(np.uint32), c.added)
    for got, want in zip(table, c.want):
        assert np.array_equal(got.cpu().numpy().view(want.dtype), want)
    del d, src
    torch.cuda.empty_cache()


# ---- unpack -> repack -> digest, in HBM ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seg_line,slots", VARIANTS)
def test_items_round_trip_in_hbm(gpu, orc, seg_line, slots):
    """metadata.pack_items_batch of random item lists (every last item at least 7 bytes), then in device mode:
    the unpacked table equals the inputs; BRB_MetaDataPackBatch fed the returned device arrays (pack_first_slot
    as pack_first_item, exact slot counts) reproduces the packs byte for byte; BRB_MD5BatchSegments over the
    same arrays equals each header's digest."""
    import torch
    from brb_framework_amd import metadata
    rng = np.random.default_rng(69)
    lists = []
    for _ in range(700):
        items = [(rand_id(rng), rand_id(rng), d) for _, _, d in cases.random_items(rng, max_items=9, max_len=500)]
        if items and len(items[-1][2]) < 7:
            items[-1] = (items[-1][0], items[-1][1], rand_bytes(rng, int(rng.integers(7, 60))))
        lists.append(items)
    buf, offs, lens = metadata.pack_items_batch(lists)
    first = np.zeros(len(lists) + 1, np.uint64)
    first[1:] = np.cumsum([len(it) for it in lists])
    n_items = int(first[-1])
    d, o, ln, f = to_dev(buf), to_dev(offs), to_dev(lens), to_dev(first)
    z = lambda dt: torch.zeros(n_items, dtype=dt, device="cuda")
    ioff, ilen, iid, isub = z(torch.int64), z(torch.int32), z(torch.int64), z(torch.int64)
    with variant(gpu, seg_line, slots):
        info, added = gpu.metadata_unpack_items_batch(d, o, ln, ioff, ilen, iid, isub, f)
    info = info.cpu().numpy().reshape(-1).view(gpu.METADATA_INFO_DTYPE)
    assert set(info["error_code"].tolist()) == {7}
    assert added.cpu().numpy().tolist() == [len(it) for it in lists] == info["item_count"].tolist()
    flat = [it for items in lists for it in items]
    want_off = [int(offs[p]) + 64 + sum(25 + len(x[2]) for x in items[:j]) + 24
                for p, items in enumerate(lists) for j in range(len(items))]
    assert ioff.cpu().numpy().tolist() == want_off
    assert ilen.cpu().numpy().tolist() == [len(x[2]) for x in flat]
    assert iid.cpu().numpy().view(np.uint64).tolist() == [x[0] for x in flat]
    assert isub.cpu().numpy().view(np.uint64).tolist() == [x[1] for x in flat]
    out = torch.full((buf.size,), 0xEE, dtype=torch.uint8, device="cuda")
    gpu.metadata_pack_batch(d, ioff, ilen, iid, isub, f, out, o)
    total = int(offs[-1]) + int(lens[-1])
    assert np.array_equal(out.cpu().numpy()[:total], buf[:total])
    dig = gpu.md5_batch_segments(d, ioff, ilen, f).cpu().numpy()
    head = np.stack([buf[int(a) + 24:int(a) + 40] for a in offs])
    assert np.array_equal(dig, head)


@pytest.mark.gpu
def test_unpack_items_batch_helper(gpu, orc):
    """metadata.unpack_items_batch: slots from the (len - 64) // 25 bound or from max_items, host and device."""
    from brb_framework_amd import metadata
    packs, wk = walk.walked_corpus(2, 3000)
    packs, wk = packs[2200:2500], wk[2200:2500]
    buf, offs, lens = cases.scatter(np.random.default_rng(70), packs)
    for max_items in (None, 2):
        host = metadata.unpack_items_batch(buf, offs, lens, max_items=max_items)
        dev = metadata.unpack_items_batch(to_dev(buf), to_dev(offs), to_dev(lens), max_items=max_items)
        dev = [x.cpu().numpy() for x in dev]
        dev[0] = dev[0].reshape(-1).view(gpu.METADATA_INFO_DTYPE)
        for res in (host, dev):
            info, added, first, ioff, ilen, iid, isub = res
            first = first.view(np.uint64)
            assert infos_as_tuples(info) == [five for five, _ in wk]
            assert added.view(np.uint32).tolist() == [len(t) for _, t in wk]
            for p, (_, table) in enumerate(wk):
                s, k = int(first[p]), min(len(table), int(first[p + 1] - first[p]))
                if max_items is None:
                    assert k == len(table)
                got = list(zip(ioff[s:s + k].view(np.uint64).tolist(), ilen[s:s + k].view(np.uint32).tolist(),
                               iid[s:s + k].view(np.uint64).tolist(), isub[s:s + k].view(np.uint64).tolist()))
                assert got == [(int(offs[p]) + a, b, c_, d_) for a, b, c_, d_ in table[:k]]
