"""BRB_MetaDataPackBatch: MetaDataPack (meta_data.c:104-140, digest :397-433) of many
MetaDatas in one GPU pass -- one lane per pack, every item byte read once for the digest and the pack.

Every comparison is byte for byte against the oracle's cited restatement, orc.metadata_pack(items)
(pinned by struct + hashlib in tests/test_metadata.py::test_oracle_pack_layout_and_digest).  A call is
laid out by build_call(): the items scattered over a source buffer at arbitrary byte offsets (an empty
item's offset points far outside it: it is never read), the packs scattered over an output buffer
pre-filled with a pattern; the whole output image is compared, so every byte outside the packs must
still hold the pattern.  No call passes a range outside its buffers.

CPU: argument checks (reached before any device work) and metadata.pack_sizes.  GPU: host, device and
all-devices modes on a random corpus; the digest's block edges and the two streams' byte phases (item
lengths 0..130 and block-straddling pairs at every source alignment mod 16 and output alignment mod
64); packs back to back, so their borders fall inside dwords and 64-byte sectors; lanes of one wave
with 0, 1 and 40 items; offsets past 4 GiB on both sides; pack -> BRB_MetaDataUnpackBatch round trips;
metadata.pack_items_batch against metadata.pack_batch; an asynchronous call on a side stream.
"""
import ctypes
import functools

import numpy as np
import pytest

M64 = 1 << 64
FAR = 1 << 62                       # an empty item's offset: nothing may read there


# ---- corpus and layout ------------------------------------------------------------------------------
def random_items(rng, max_items=12, max_len=3000):
    """As tests/test_metadata.py's generator, with full 64-bit ids and sub-ids."""
    k = int(rng.integers(0, max_items + 1))
    out = []
    for j in range(k):
        n = int(rng.integers(0, 7)) if (j == k - 1 and rng.random() < 0.3) else int(rng.integers(0, max_len + 1))
        out.append((int(rng.integers(0, M64, dtype=np.uint64)), int(rng.integers(0, M64, dtype=np.uint64)),
                    rng.integers(0, 256, n, dtype=np.uint8).tobytes()))
    return out


class Call:
    """The nine arrays of one BRB_MetaDataPackBatch call, the pre-filled output and the expected one."""


def build_call(rng, packs, want, gaps=(0, 40), out_start=0, out_align=None, src_align=None):
    """packs: lists of (item_id, item_sub_id, data); want: orc.metadata_pack of each.  out_align[p] /
    src_align[p]: pack p's output offset mod 64 / its first non-empty item's source offset mod 16."""
    c = Call()
    items = [it for p in packs for it in p]
    first = np.zeros(len(packs) + 1, np.uint64)
    first[1:] = np.cumsum([len(p) for p in packs])
    align_of = {}
    if src_align is not None:
        for p, items_p in enumerate(packs):
            for j, it in enumerate(items_p):
                if it[2]:
                    align_of[int(first[p]) + j] = src_align[p]
                    break
    ioff = np.zeros(len(items), np.uint64)
    parts, pos = [], 0
    for j in rng.permutation(len(items)):                # the items in any order in the source
        d = items[j][2]
        if not d:
            ioff[j] = FAR + int(j)
            continue
        g = (align_of[j] - pos) % 16 if j in align_of else int(rng.integers(0, 8))
        parts += [rng.integers(0, 256, g, dtype=np.uint8).tobytes(), d]
        ioff[j] = pos + g
        pos += g + len(d)
    c.data = np.frombuffer(b"".join(parts) + bytes(8), np.uint8).copy()
    c.ioff = ioff
    c.ilen = np.array([len(d) for _, _, d in items], np.uint32)
    c.iid = np.array([i for i, _, _ in items], np.uint64)
    c.isub = np.array([s for _, s, _ in items], np.uint64)
    c.first = first
    ooff, pos = [], out_start
    for p, w in enumerate(want):
        g = (out_align[p] - pos) % 64 if out_align is not None else int(rng.integers(gaps[0], gaps[1] + 1))
        ooff.append(pos + g)
        pos += g + len(w)
    c.ooff = np.array(ooff, np.uint64)
    c.pattern = (np.arange(pos + 67) % 251).astype(np.uint8)
    c.expect = c.pattern.copy()
    for o, w in zip(ooff, want):
        c.expect[o:o + len(w)] = np.frombuffer(w, np.uint8)
    c.want = want
    return c


def to_dev(a):
    import torch
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def run(brb, c, mode, stream=None, async_=False):
    """The call in host / device / all-devices mode on a fresh copy of the pattern; -> the output image."""
    out = c.pattern.copy()
    if mode == "host":
        brb.metadata_pack_batch(c.data, c.ioff, c.ilen, c.iid, c.isub, c.first, out, c.ooff)
    elif mode == "all":
        with brb.TestOption("devices", 3):               # three concurrent parts, also on a one-GPU box
            brb.metadata_pack_batch(c.data, c.ioff, c.ilen, c.iid, c.isub, c.first, out, c.ooff, all_devices=True)
    else:
        import torch
        t = [to_dev(a) for a in (c.data, c.ioff, c.ilen, c.iid, c.isub, c.first, out, c.ooff)]
        torch.cuda.synchronize()
        brb.metadata_pack_batch(*t, stream=stream, async_=async_)
        if stream is not None:
            stream.synchronize()
        out = t[6].cpu().numpy()
    return out


def check(out, c):
    if np.array_equal(out, c.expect):
        return
    for p, (o, w) in enumerate(zip(c.ooff.tolist(), c.want)):
        got = out[o:o + len(w)].tobytes()
        assert got == w, f"pack {p} ({int(c.first[p + 1] - c.first[p])} items, {len(w)} bytes at {o}) differs " \
                         f"at byte {next(i for i in range(len(w)) if got[i] != w[i])}"
    bad = np.flatnonzero(out != c.expect)
    raise AssertionError(f"{bad.size} bytes outside the packs changed, the first at {int(bad[0])}")


@functools.lru_cache(maxsize=None)
def random_corpus():
    import oracle
    rng = np.random.default_rng(41)
    packs = [random_items(rng) for _ in range(4000)]
    return packs, [oracle.metadata_pack(p) for p in packs]


# ---- CPU ----------------------------------------------------------------------------------------------
def small_call(orc):
    rng = np.random.default_rng(40)
    packs = [random_items(rng, 4, 90) for _ in range(9)] + [[]]
    return build_call(rng, packs, [orc.metadata_pack(p) for p in packs])


def raw_args(c, out, n=None, flags=0):
    p = lambda a: a.ctypes.data
    return [p(c.data), p(c.ioff), p(c.ilen), p(c.iid), p(c.isub), p(c.first), len(c.ooff) if n is None else n, p(out),
            p(c.ooff), flags, None]


def test_pack_bad_arguments(brb, orc):
    """Refusals that need no device: a NULL pointer, a decreasing pack_first_item, a pack of more than
    INT32_MAX items, device pointers with BRB_BATCH_ALL_DEVICES; an empty batch is done."""
    L = brb.lib()
    c = small_call(orc)
    out = c.pattern.copy()
    for i in (0, 1, 2, 3, 4, 5, 7, 8):
        a = raw_args(c, out)
        a[i] = None
        assert L.BRB_MetaDataPackBatch(*a) == -1, i
        assert b"NULL" in L.BRB_CryptoGPU_LastError()
    bad = c.first.copy()
    bad[0] = bad[1] + 1                                  # decreases at pack 0
    a = raw_args(c, out)
    a[5] = bad.ctypes.data
    assert L.BRB_MetaDataPackBatch(*a) == -1
    assert b"non-decreasing" in L.BRB_CryptoGPU_LastError()
    many = np.array([0, 1 << 31], np.uint64)
    a = raw_args(c, out, n=1)
    a[5] = many.ctypes.data
    assert L.BRB_MetaDataPackBatch(*a) == -1
    assert b"items" in L.BRB_CryptoGPU_LastError()
    assert L.BRB_MetaDataPackBatch(*raw_args(c, out, flags=brb.BATCH_DEVICE | brb.BATCH_ALL_DEVICES)) == -1
    assert b"ALL_DEVICES" in L.BRB_CryptoGPU_LastError()
    assert L.BRB_MetaDataPackBatch(*raw_args(c, out, n=1 << 33)) == -1
    assert b"split the batch" in L.BRB_CryptoGPU_LastError()
    assert L.BRB_MetaDataPackBatch(*raw_args(c, out, n=0)) == 1
    assert L.BRB_MetaDataPackBatch(None, None, None, None, None, None, 0, None, None, 0, None) == 1
    assert np.array_equal(out, c.pattern)                # none of these wrote anything


def test_pack_valid_call_without_gpu_is_refused(brb, orc):
    """A valid host-mode call returns 0 with a reason when no device is usable -- never packs on the
    CPU -- and leaves `out` alone; with a device it returns 1 and the packs are the oracle's."""
    L = brb.lib()
    c = small_call(orc)
    out = c.pattern.copy()
    rc = L.BRB_MetaDataPackBatch(*raw_args(c, out))
    if brb.gpu_available():
        assert rc == 1
        check(out, c)
    else:
        assert rc == 0 and L.BRB_CryptoGPU_LastError().strip()
        assert np.array_equal(out, c.pattern)
        with pytest.raises(RuntimeError, match="returned 0"):
            brb.metadata_pack_batch(c.data, c.ioff, c.ilen, c.iid, c.isub, c.first, out, c.ooff)


def test_pack_sizes_vs_oracle(orc):
    from brb_framework_amd import metadata
    rng = np.random.default_rng(42)
    packs = [random_items(rng, 8, 400) for _ in range(199)] + [[]]
    lens = np.array([len(d) for p in packs for _, _, d in p], np.uint32)
    first = np.concatenate([[0], np.cumsum([len(p) for p in packs])]).astype(np.uint64)
    sizes = metadata.pack_sizes(lens, first)
    assert sizes.dtype == np.uint64
    assert sizes.tolist() == [len(orc.metadata_pack(p)) for p in packs]
    assert sizes.tolist() == [metadata.pack_size(p) for p in packs]


# ---- GPU ----------------------------------------------------------------------------------------------
@pytest.fixture()
def gpu(brb):
    assert brb.gpu_available(), brb.lib().BRB_CryptoGPU_LastError()
    return brb


@pytest.mark.gpu
def test_pack_random_corpus_all_modes(gpu, orc):
    """4 000 packs of 0..12 items of 0..3 000 bytes, full 64-bit ids, the items anywhere in the
    source, the packs 0..40 bytes apart in a patterned output: host, device and all-devices modes."""
    packs, want = random_corpus()
    c = build_call(np.random.default_rng(43), packs, want)
    for mode in ("host", "device", "all"):
        check(run(gpu, c, mode), c)


EDGE_CASES = [[n] for n in range(131)] + [[3, 61], [60, 5], [63, 1], [64, 0], [0, 64], [1, 1, 1, 1]]


@pytest.mark.gpu
@pytest.mark.parametrize("half", [0, 1])
def test_pack_digest_and_phase_edges(gpu, orc, half):
    """Single items of 0..130 bytes (the MD5 padding edges 55/56/63/64/65 and 119/120/128) and item
    lists straddling a block, each at the 32 output alignments mod 64 of this half; the source
    alignment mod 16 steps with them, so both streams meet every byte phase of the other."""
    rng = np.random.default_rng(44)
    packs, want, oa, sa = [], [], [], []
    for ci, lens in enumerate(EDGE_CASES):
        items = [(int(rng.integers(0, M64, dtype=np.uint64)), ci, rng.integers(0, 256, n, dtype=np.uint8).tobytes())
                 for n in lens]
        w = orc.metadata_pack(items)
        for a in range(32 * half, 32 * half + 32):
            packs.append(items)
            want.append(w)
            oa.append(a)
            sa.append((a + ci + a // 16) % 16)
    c = build_call(rng, packs, want, out_align=oa, src_align=sa)
    assert sorted(set(int(o) % 64 for o in c.ooff)) == list(range(32 * half, 32 * half + 32))
    check(run(gpu, c, "device"), c)


@pytest.mark.gpu
@pytest.mark.parametrize("n_packs", [1, 63, 64, 65, 129])
def test_pack_back_to_back(gpu, orc, n_packs):
    """No gap between packs, the first at output offset 1..3: pack borders inside a dword and inside a
    64-byte sector, and a last wave of 1, 63 or 64 lanes."""
    rng = np.random.default_rng(45 + n_packs)
    packs = [random_items(rng, 4, 100) for _ in range(n_packs)]
    want = [orc.metadata_pack(p) for p in packs]
    for start in (1, 2, 3):
        c = build_call(rng, packs, want, gaps=(0, 0), out_start=start)
        assert int(c.ooff[0]) == start
        check(run(gpu, c, "device"), c)
        check(run(gpu, c, "host"), c)


@pytest.mark.gpu
def test_pack_divergent_wave(gpu, orc):
    """One wave whose lanes hold 0, 1 and 40 items of 0, 2 and 1 000 bytes; then one 1 MiB item
    between empty packs."""
    rng = np.random.default_rng(46)
    packs = []
    for i in range(64):
        k = (0, 1, 40)[i % 3]
        packs.append([(i, j, rng.integers(0, 256, (0, 2, 1000)[(i // 3 + j) % 3], dtype=np.uint8).tobytes())
                      for j in range(k)])
    c = build_call(rng, packs, [orc.metadata_pack(p) for p in packs])
    check(run(gpu, c, "device"), c)
    packs = [[] for _ in range(64)]
    packs[17] = [(M64 - 1, M64 - 2, rng.integers(0, 256, 1 << 20, dtype=np.uint8).tobytes())]
    c = build_call(rng, packs, [orc.metadata_pack(p) for p in packs], gaps=(0, 3))
    check(run(gpu, c, "device"), c)


@pytest.mark.gpu
def test_pack_beyond_4gib(gpu, orc):
    """A few packs in one 4.5 GiB device buffer that holds items and packs alike: one item's source
    offset and one pack's output offset lie above 2^32 (64-bit addressing on both sides)."""
    import torch
    rng = np.random.default_rng(47)
    packs = [random_items(rng, 5, 700) for _ in range(5)]
    packs[1] = packs[1] + [(9, 9, rng.integers(0, 256, 333, dtype=np.uint8).tobytes())]
    packs[3] = packs[3] + [(8, 8, rng.integers(0, 256, 4100, dtype=np.uint8).tobytes())]
    want = [orc.metadata_pack(p) for p in packs]
    c = build_call(rng, packs, want)
    total = 9 << 29
    src_lo, src_hi = 1 << 20, (1 << 32) + (1 << 20) + 5      # the source copied twice
    out_lo, out_hi = 1 << 28, (1 << 32) + (1 << 28) + 3      # the patterned output twice; pack 2 goes high
    assert out_hi + c.pattern.size <= total and src_hi + c.data.size < out_hi
    ioff = c.ioff.copy()
    k_far = int(c.first[3 + 1]) - 1                          # pack 3's 4 100-byte item is read from the high copy
    ioff[k_far] += np.uint64(src_hi - src_lo)
    ooff = c.ooff + np.uint64(out_lo)
    ooff[2] = c.ooff[2] + np.uint64(out_hi)
    d = torch.empty(total, dtype=torch.uint8, device="cuda")
    src = to_dev(c.data)
    d[src_lo:src_lo + src.numel()] = src
    d[src_hi:src_hi + src.numel()] = src
    pat = to_dev(c.pattern)
    d[out_lo:out_lo + pat.numel()] = pat
    d[out_hi:out_hi + pat.numel()] = pat
    nonempty = c.ilen != 0
    ioff[nonempty] += np.uint64(src_lo)
    assert int(ioff[k_far]) > 1 << 32 and int(ooff[2]) > 1 << 32
    torch.cuda.synchronize()
    gpu.metadata_pack_batch(d, to_dev(ioff), to_dev(c.ilen), to_dev(c.iid), to_dev(c.isub), to_dev(c.first), d,
                            to_dev(ooff))
    low = d[out_lo:out_lo + pat.numel()].cpu().numpy()
    high = d[out_hi:out_hi + pat.numel()].cpu().numpy()
    exp_low, exp_high = c.expect.copy(), c.pattern.copy()
    o2, n2 = int(c.ooff[2]), len(want[2])
    exp_low[o2:o2 + n2] = c.pattern[o2:o2 + n2]              # pack 2 is not in the low image ...
    exp_high[o2:o2 + n2] = c.expect[o2:o2 + n2]              # ... but in the high one, alone
    assert np.array_equal(high, exp_high)
    assert np.array_equal(low, exp_low)
    del d, src, pat
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_pack_unpack_round_trip(gpu, orc):
    """BRB_MetaDataPackBatch -> BRB_MetaDataUnpackBatch: every pack whose last item has at least 7
    bytes (and the empty pack) unpacks with SUCCESS and lists its items; packs whose last item has
    0..6 bytes report what the oracle's unpack reports for them (the reference's quirk)."""
    from brb_framework_amd import metadata
    rng = np.random.default_rng(48)
    packs = [[]]
    for _ in range(1500):
        items = random_items(rng, 8, 600)
        if items and len(items[-1][2]) < 7:
            items[-1] = (items[-1][0], items[-1][1], rng.integers(0, 256, int(rng.integers(7, 50)), dtype=np.uint8).tobytes())
        packs.append(items)
    n_good = len(packs)
    packs += [[(1, 2, bytes(range(40)))] * j + [(5, 6, bytes(range(n)))] for n in range(7) for j in (0, 2)]
    want = [orc.metadata_pack(p) for p in packs]
    want_info = [orc.metadata_unpack(w) for w in want]
    assert all(i[0] == 7 for i in want_info[:n_good])        # the corpus meets its condition by construction
    assert all(i[0] != 7 for i in want_info[n_good:])
    c = build_call(rng, packs, want, gaps=(0, 9))
    out = run(gpu, c, "device")
    check(out, c)
    lens = np.array([len(w) for w in want], np.uint32)
    info = gpu.metadata_unpack_batch(out, c.ooff, lens)
    assert [tuple(int(x) for x in r) for r in info.tolist()] == want_info
    for p in range(n_good):
        o = int(c.ooff[p])
        assert metadata.items(out[o:o + int(lens[p])].tobytes()) == packs[p]


@pytest.mark.gpu
def test_pack_items_batch_equals_pack_batch(gpu, orc):
    from brb_framework_amd import metadata
    rng = np.random.default_rng(49)
    packs = [random_items(rng) for _ in range(598)] + [[], [(7, 8, b"")]]
    buf, offs, lens = metadata.pack_items_batch(packs)
    buf0, offs0, lens0 = metadata.pack_batch(packs)
    assert np.array_equal(offs, offs0) and np.array_equal(lens, lens0) and lens.dtype == lens0.dtype
    assert np.array_equal(buf, buf0)
    assert buf[int(offs[7]):int(offs[7]) + int(lens[7])].tobytes() == orc.metadata_pack(packs[7])
    buf2, _, _ = metadata.pack_items_batch(packs, all_devices=True)
    assert np.array_equal(buf2, buf0)


@pytest.mark.gpu
def test_pack_async_on_side_stream(gpu, orc):
    """Device mode with BRB_BATCH_ASYNC on a non-default stream: compared after stream.synchronize()."""
    import torch
    packs, want = random_corpus()
    c = build_call(np.random.default_rng(50), packs[:700], want[:700])
    check(run(gpu, c, "device", stream=torch.cuda.Stream(), async_=True), c)
