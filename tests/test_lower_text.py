"""BRB_MD5LowerTextBatch and BRB_MD5UpdateSegmentsLowerBatch on the GPU, byte for byte against hashlib of the
lower-cased bytes and against the product's own compat functions (md5_ctx_update / md5_ctx_update_lower /
md5_ctx_final, pinned by test_compat.py).  Every case is tiny: a few hundred keys or contexts of at most a
few hundred bytes."""
import hashlib
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODES = ("host", "device", "device_async", "all_devices")
LENS = (0, 1, 3, 4, 5, 55, 56, 57, 63, 64, 65, 119, 120, 127, 128, 129, 200, 257, 300)
STARTS = (0, 1, 2, 3, 60, 61, 62, 63, 64, 65, 66, 67)            # key start address: mod 4, and mod 64 (as 64 + k)
SPECIAL = (0x40, 0x41, 0x5A, 0x5B, 0x60, 0x61, 0x7A, 0x7B, 0xC1, 0xDA)
HAVES = (0, 1, 3, 4, 55, 56, 60, 63)
FAR = (1 << 62) + 4099                              # host mode: the offset of an empty key or segment need not be memory
HDR = 24                                            # state words and counters; the block buffer follows


@pytest.fixture(scope="module")
def torch_dev(brb):
    import torch
    assert torch.cuda.is_available(), "no HIP device visible to torch"
    assert brb.gpu_available(), brb.lib().BRB_CryptoGPU_LastError()
    return torch


def lowered(key):
    return bytes(b + 32 if 65 <= b <= 90 else b for b in key)


def md5_low(key):
    return hashlib.md5(lowered(key)).digest()


def _dev(torch, a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


# ---- one-shot keys --------------------------------------------------------------------------------
def key_of(data, offs, lens, i):
    return data[int(offs[i]):int(offs[i]) + int(lens[i])].tobytes() if lens[i] else b""


def run_keys(brb, torch, mode, data, offs, lens, outputs="ds"):
    """One BRB_MD5LowerTextBatch call in `mode` writing the outputs named ("d" digests, "s" strings) into
    0xA5-filled buffers one row longer than needed.  Returns (digests or None, strings or None, data after)."""
    n = len(offs)
    dig = np.full((n + 1, 16), 0xA5, np.uint8) if "d" in outputs else None
    strs = np.full((n + 1, 33), 0xA5, np.uint8) if "s" in outputs else None
    device = mode.startswith("device")
    if device:
        bufs = [_dev(torch, x) for x in (data, offs, lens, dig, strs)]
        flags, side = brb.BATCH_DEVICE, None
        if mode == "device_async":
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            flags |= brb.BATCH_ASYNC
    else:
        bufs = [data, offs, lens, dig, strs]
        flags, side = (brb.BATCH_HOST | brb.BATCH_ALL_DEVICES if mode == "all_devices" else brb.BATCH_HOST), None
    if "d" in outputs:                              # the Python call; strings alone go through the C call
        kw = dict(out=bufs[3], strings=bufs[4])
        if device:
            kw.update(stream=side, async_=side is not None)
        if mode == "all_devices":
            with brb.TestOption("devices", 2):
                res = brb.md5_lower_text_batch(bufs[0], bufs[1], bufs[2], all_devices=True, **kw)
        else:
            res = brb.md5_lower_text_batch(bufs[0], bufs[1], bufs[2], **kw)
        assert (res[0] is bufs[3] and res[1] is bufs[4]) if "s" in outputs else res is bufs[3]
    else:
        ptr = lambda x: None if x is None else (x.data_ptr() if device else x.ctypes.data)
        call = lambda: brb.lib().BRB_MD5LowerTextBatch(ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), n, None, ptr(bufs[4]), flags,
                                                       side.cuda_stream if side is not None else None)
        if mode == "all_devices":
            with brb.TestOption("devices", 2):
                rc = call()
        else:
            rc = call()
        assert rc == 1, brb.lib().BRB_CryptoGPU_LastError()
    if side is not None:
        side.synchronize()
    if device:
        dig, strs = (None if b is None else b.cpu().numpy() for b in bufs[3:])
        return dig, strs, bufs[0].cpu().numpy()
    return dig, strs, data


def check_keys(data, offs, lens, dig, strs, after=None, data0=None):
    n = len(offs)
    want = [md5_low(key_of(data, offs, lens, i)) for i in range(n)]
    if dig is not None:
        assert [dig[i].tobytes() for i in range(n)] == want
        assert (dig[n] == 0xA5).all()               # the spare row
    if strs is not None:
        assert [strs[i].tobytes() for i in range(n)] == [w.hex().encode() + b"\0" for w in want]
        assert (strs[n] == 0xA5).all()
    if after is not None:
        assert np.array_equal(after, data0)         # data is never written


def place(keys, starts, rng, far_empty=False):
    """(data, offsets, lengths): key i at an offset with offset % 64 == starts[i] % 64, in order, a few unused
    bytes in between.  The first key is at offset 0 (a multiple of 64), so host-mode staging, which rebases
    the span to its first byte, keeps every key's address mod 64."""
    assert starts[0] % 64 == 0 and len(keys[0])
    buf, offs = bytearray(), []
    for i, key in enumerate(keys):
        pad = (starts[i] - len(buf)) % 64
        buf += rng.integers(0, 256, pad, dtype=np.uint8).tobytes()
        offs.append(FAR + 7 * i if far_empty and not key else len(buf))
        buf += key
    buf += bytes(8)
    return (np.frombuffer(bytes(buf), np.uint8).copy(), np.array(offs, np.uint64),
            np.array([len(k) for k in keys], np.uint32))


@pytest.mark.parametrize("mode", MODES)
def test_lengths_and_start_addresses(brb, torch_dev, mode):
    """Every length class at every start address mod 4 and around a 64-byte line boundary."""
    rng = np.random.default_rng(31)
    cases = [(0, 7)] + list(itertools.product(STARTS, LENS))
    keys = [rng.integers(0x30, 0x80, n, dtype=np.uint8).tobytes() for _, n in cases]
    data, offs, lens = place(keys, [s for s, _ in cases], rng, far_empty=mode == "host")
    assert {int(o) % 64 for o, n in zip(offs, lens) if n} >= {s % 64 for s in STARTS}
    data0 = data.copy()
    dig, strs, after = run_keys(brb, torch_dev, mode, data, offs, lens)
    check_keys(data0, offs, lens, dig, strs, after, data0)


@pytest.mark.parametrize("mode", ["host", "device"])
def test_every_byte_value_on_every_byte_lane(brb, torch_dev, mode):
    """bytes(range(256)) rotated: each of 0x40 'A' 'Z' 0x5B 0x60 'a' 'z' 0x7B 0xC1 0xDA -- and every other byte
    value -- on each of the four byte lanes of a dword, and each as the last byte of a key."""
    rng = np.random.default_rng(32)
    ring = np.arange(256, dtype=np.uint8)
    keys = [np.roll(ring, r).tobytes() for r in range(4)]                   # 4-byte aligned starts
    for r, key in enumerate(keys):
        assert all(key[(v + r) % 256] == v for v in SPECIAL)
    assert {(v, (v + r) & 3) for v in SPECIAL for r in range(4)} == set(itertools.product(SPECIAL, range(4)))
    tails = [np.roll(ring, 36 - v)[:37].tobytes() for v in SPECIAL]          # 37 bytes ending in v
    assert [t[-1] for t in tails] == list(SPECIAL)
    tails += [t[-1:] for t in tails]                                       # and the one-byte key
    keys += tails
    data, offs, lens = place(keys, [0, 64, 128, 192] + list(range(len(tails))), rng)
    dig, strs, after = run_keys(brb, torch_dev, mode, data, offs, lens)
    check_keys(data, offs, lens, dig, strs, after, data.copy())
    # signed char: 0xC1 .. 0xDA do not move, 'A' .. 'Z' do
    one = {t[0]: dig[4 + len(SPECIAL) + i].tobytes() for i, t in enumerate(tails[len(SPECIAL):])}
    assert one[0xC1] == hashlib.md5(b"\xc1").digest() and one[0xDA] == hashlib.md5(b"\xda").digest()
    assert one[0x41] == hashlib.md5(b"a").digest() and one[0x5A] == hashlib.md5(b"z").digest()
    assert one[0x40] == hashlib.md5(b"@").digest() and one[0x5B] == hashlib.md5(b"[").digest()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("outputs", ["d", "s", "ds"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_counts_and_outputs(brb, torch_dev, n, outputs, mode):
    """n keys below, at and past a wave and a workgroup; digests only, strings only, both.  The spare row of
    each output keeps its fill, strings end in a NUL, data is not written, and in host mode an empty key's
    offset lies far outside the buffer."""
    rng = np.random.default_rng(3300 + n)
    lens = rng.choice(LENS, n)
    lens[0] = 9
    if n > 2:
        lens[n // 2] = 0
    keys = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in lens]
    data, offs, lens = place(keys, [0] + [int(s) for s in rng.integers(0, 64, n - 1)], rng, far_empty=mode == "host")
    data0 = data.copy()
    dig, strs, after = run_keys(brb, torch_dev, mode, data, offs, lens, outputs)
    assert (dig is None) == ("d" not in outputs) and (strs is None) == ("s" not in outputs)
    check_keys(data0, offs, lens, dig, strs, after, data0)
    if strs is not None:
        assert not strs[:n, 32].any()


def _layouts():
    """name -> (data, offsets, lengths), each with a group (64 consecutive keys) of the named shape."""
    rng = np.random.default_rng(34)
    out = {}

    def packed(lens):
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        return rng.integers(0, 256, int(np.sum(lens)) + 8, dtype=np.uint8), offs, np.asarray(lens, np.uint32)

    lens = rng.integers(8, 65, 200)
    out["packed"] = packed(lens)
    d, o, l = packed(lens)
    out["reverse"] = (d, o[::-1].copy(), l[::-1].copy())
    d = rng.integers(0x41, 0x5B, 300, dtype=np.uint8)
    out["shared"] = (d, np.full(130, 5, np.uint64), np.full(130, 77, np.uint32))
    out["overlapping"] = (d, np.arange(130, dtype=np.uint64), rng.integers(1, 170, 130).astype(np.uint32))
    d, o, l = packed(rng.integers(8, 65, 128))
    d = np.concatenate([d, rng.integers(0, 256, 1 << 20, dtype=np.uint8)])
    o[17] = len(d) - 100                            # one key 1 MiB away from the rest of its group
    o[64 + 63] = len(d) - 200
    out["one_far_key"] = (d, o, l)
    l = rng.integers(8, 65, 192).astype(np.uint32)
    l[64:128] = 0                                   # a group of empty keys only
    out["empty_group"] = packed(l)
    return out


LAYOUTS = _layouts()


@pytest.fixture(scope="module")
def layout_wants():
    return {name: [md5_low(key_of(d, o, l, i)) for i in range(len(o))] for name, (d, o, l) in LAYOUTS.items()}


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_layouts(brb, torch_dev, layout_wants, name, mode):
    """Keys packed back to back, in reverse order, shared by all lanes of a wave, overlapping, one of a group
    1 MiB away from the rest, and a group of empty keys only."""
    data, offs, lens = LAYOUTS[name]
    dig, strs, after = run_keys(brb, torch_dev, mode, data, offs, lens)
    assert np.array_equal(after, data)
    n = len(offs)
    assert [dig[i].tobytes() for i in range(n)] == layout_wants[name]
    assert [strs[i].tobytes() for i in range(n)] == [w.hex().encode() + b"\0" for w in layout_wants[name]]
    assert (dig[n] == 0xA5).all() and (strs[n] == 0xA5).all()


@pytest.mark.parametrize("mode", MODES)
def test_random_keys(brb, torch_dev, mode):
    rng = np.random.default_rng(35)
    n = 300
    keys = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(0, 301, n)]
    keys[0] = keys[0] + b"Q"
    data, offs, lens = place(keys, [0] + [int(s) for s in rng.integers(0, 64, n - 1)], rng, far_empty=mode == "host")
    perm = rng.permutation(n)
    offs, lens = offs[perm].copy(), lens[perm].copy()
    data0 = data.copy()
    dig, strs, after = run_keys(brb, torch_dev, mode, data, offs, lens)
    check_keys(data0, offs, lens, dig, strs, after, data0)


# ---- contexts -------------------------------------------------------------------------------------
def have_of(row):
    return int(row.view(np.uint32)[4]) & 63


def defined(row):
    """The part of a context that an Update defines: state, counters, the buffered bytes."""
    return row[:HDR + have_of(row)].tobytes()


def contexts_with(brb, haves, rng, fill=0xA5):
    """Rows holding compat contexts with 64 + have bytes taken (so the state is not the IV), `fill` elsewhere."""
    rows = np.full((len(haves), 168), fill, np.uint8)
    for r, have in enumerate(haves):
        msg = rng.integers(0, 256, 64 + int(have), dtype=np.uint8).tobytes()
        brb.md5_ctx_init(rows[r])
        brb.md5_ctx_update(rows[r], msg[:64])
        brb.md5_ctx_update(rows[r], msg[64:])
    return rows


def lay_out(lists, rng, far_empty, aligns=None, edge=None):
    """(data, seg_offsets, seg_lengths, item_first_seg) for per-item lists of segment lengths: segment k at an
    address with (address & 3) == aligns[k] (default k & 3).  edge: that byte value in the first and last four
    bytes of every segment.  One unnamed entry behind the lists keeps the arrays non-empty."""
    flat = [int(n) for li in lists for n in li]
    offs, pos = [], 4
    for k, n in enumerate(flat):
        pos += ((k if aligns is None else int(aligns[k])) - pos) & 3
        offs.append(FAR + 7 * k if far_empty and n == 0 else pos)
        pos += n + int(rng.integers(0, 3))
    data = rng.integers(0, 256, pos + 8, dtype=np.uint8)
    if edge is not None:
        for o, n in zip(offs, flat):
            if n:
                data[o:o + min(n, 4)] = edge
                data[o + max(n - 4, 0):o + n] = edge
    first = np.concatenate([[0], np.cumsum([len(li) for li in lists])]).astype(np.uint64)
    return data, np.array(offs + [pos], np.uint64), np.array(flat + [0], np.uint32), first


def run_segments(brb, torch, mode, ctxs, seg, low, fin, idx=None, lower=True):
    """BRB_MD5UpdateSegmentsLowerBatch (lower=False: BRB_MD5UpdateSegmentsBatch) in `mode` on a host table that is
    updated in place.  Returns (digests over a 0xA5 fill or None, data after)."""
    n = len(seg[3]) - 1
    out = None if fin is None else np.full((n, 16), 0xA5, np.uint8)
    fn = brb.md5_update_segments_lower_batch if lower else brb.md5_update_segments_batch
    kw = {"seg_lower": low} if lower else {}
    if not mode.startswith("device"):
        if mode == "all_devices":
            with brb.TestOption("devices", 2):
                res = fn(ctxs, *seg, final=fin, ctx_index=idx, out=out, all_devices=True, **kw)
        else:
            res = fn(ctxs, *seg, final=fin, ctx_index=idx, out=out, **kw)
        return res, seg[0]
    d = lambda a: _dev(torch, a)
    dc, dseg = d(ctxs), [d(a) for a in seg]
    if lower:
        kw = {"seg_lower": d(low)}
    if mode == "device_async":
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        res = fn(dc, *dseg, final=d(fin), ctx_index=d(idx), out=d(out), stream=side, async_=True, **kw)
        side.synchronize()
    else:
        res = fn(dc, *dseg, final=d(fin), ctx_index=d(idx), out=d(out), **kw)
    ctxs[...] = dc.cpu().numpy()
    return None if res is None else res.cpu().numpy(), dseg[0].cpu().numpy()


def reference(brb, ctxs, named, seg, low, fin):
    """The table and the digests (None: not finalised) the compat functions leave, segment by segment."""
    data, offs, lens, first = seg
    want, digs = ctxs.copy(), []
    for i, r in enumerate(named):
        for k in range(int(first[i]), int(first[i + 1])):
            piece = data[int(offs[k]):int(offs[k]) + int(lens[k])].tobytes() if lens[k] else b""
            (brb.md5_ctx_update_lower if low is None or low[k] else brb.md5_ctx_update)(want[r], piece)
        digs.append(brb.md5_ctx_final(want[r]) if fin is not None and fin[i] else None)
    return want, digs


def check(ctxs, before, want, named, seg, digs, got):
    """The contract of BRB_MD5UpdateSegmentsBatch, row by row."""
    first = seg[3]
    for i, r in enumerate(named):
        if digs[i] is None:
            assert defined(ctxs[r]) == defined(want[r]), (i, r)
            assert np.array_equal(ctxs[r, 88:], before[r, 88:]), (i, r)       # digest and string are not touched
            if not seg[2][int(first[i]):int(first[i + 1])].any():
                assert np.array_equal(ctxs[r], before[r]), (i, r)             # no bytes, no final: untouched
            assert got is None or (got[i] == 0xA5).all(), (i, r)
            continue
        assert got[i].tobytes() == digs[i], (i, r)
        assert np.array_equal(ctxs[r, :24], want[r, :24]), (i, r)             # buf: the final state; bytes: advanced
        assert np.array_equal(ctxs[r, 88:137], want[r, 88:137]), (i, r)       # digest, string[0 .. 33)
        assert np.array_equal(ctxs[r, 137:], before[r, 137:]), (i, r)         # string[33 .. 64) untouched
    rest = np.setdiff1d(np.arange(len(ctxs)), np.asarray(named, np.int64))
    assert np.array_equal(ctxs[rest], before[rest])


PATTERNS = ((1, 0), (0, 1), (1, 0, 1), (0, 1, 0))


def _boundary_grid():
    """(have, seg_lower pattern, segment lengths, final): the boundary between two segments falls 1, 2 and 3
    bytes into a message word, with short segments and with ones that cross a block."""
    grid = []
    for have, pat, b, long_, fin in itertools.product(HAVES, PATTERNS, (1, 2, 3), (0, 64), (0, 1)):
        l1 = ((b - have) & 3) + 8 + long_
        b2 = b % 3 + 1
        l2 = ((b2 - b) & 3) + 4 + long_
        lens = [l1, l2, 9][:len(pat)]
        assert (have + l1) & 3 == b and (len(pat) == 2 or (have + l1 + l2) & 3 == b2)
        grid.append((have, pat, lens, fin))
    return grid


@pytest.mark.parametrize("mode", MODES)
def test_segment_boundaries_inside_a_word(brb, torch_dev, mode):
    """Plain and lowered segments that meet 1, 2 and 3 bytes into a message word, 'A' on both sides of the
    boundary: the carried bytes keep the treatment of the segment they came from."""
    rng = np.random.default_rng(36)
    grid = _boundary_grid()
    ctxs = contexts_with(brb, [g[0] for g in grid], rng)
    seg = lay_out([g[2] for g in grid], rng, far_empty=False, edge=0x41)
    low = np.array([p for g in grid for p in g[1]] + [0], np.uint8)
    fin = np.array([g[3] for g in grid], np.uint8)
    named = range(len(grid))
    want, digs = reference(brb, ctxs, named, seg, low, fin)
    plain, _ = reference(brb, ctxs, named, seg, np.zeros_like(low), fin)
    assert not np.array_equal(want, plain)          # the patterns matter
    before, data0 = ctxs.copy(), seg[0].copy()
    got, after = run_segments(brb, torch_dev, mode, ctxs, seg, low, fin)
    check(ctxs, before, want, named, seg, digs, got)
    assert np.array_equal(after, data0)


@pytest.mark.parametrize("mode", MODES)
def test_segments_without_final(brb, torch_dev, mode):
    rng = np.random.default_rng(37)
    grid = _boundary_grid()
    ctxs = contexts_with(brb, [g[0] for g in grid], rng)
    seg = lay_out([g[2] for g in grid], rng, far_empty=False, edge=0x41)
    low = np.array([p for g in grid for p in g[1]] + [0], np.uint8)
    named = range(len(grid))
    want, digs = reference(brb, ctxs, named, seg, low, None)
    before = ctxs.copy()
    got, _ = run_segments(brb, torch_dev, mode, ctxs, seg, low, None)
    assert got is None
    check(ctxs, before, want, named, seg, digs, got)


def _random_case(brb, rng, n, far_empty):
    lists = [rng.integers(0, 301, int(k)) for k in rng.integers(0, 5, n)]
    nseg = sum(len(li) for li in lists)
    seg = lay_out(lists, rng, far_empty=far_empty, aligns=rng.integers(0, 4, nseg))
    seg[0][:] = rng.choice(np.frombuffer(b"@AZ[`az{MmQq\xc1\xda\x00\xff", np.uint8), len(seg[0]))
    low = rng.integers(0, 2, nseg + 1).astype(np.uint8) * rng.integers(1, 256, nseg + 1).astype(np.uint8)
    return seg, low


@pytest.mark.parametrize("mode", ["host", "device"])
def test_all_zero_seg_lower_is_update_segments_batch(brb, torch_dev, mode):
    rng = np.random.default_rng(38)
    n = 300
    ctxs = contexts_with(brb, rng.integers(0, 64, n), rng)
    seg, low = _random_case(brb, rng, n, far_empty=mode == "host")
    fin = rng.integers(0, 2, n).astype(np.uint8)
    other = ctxs.copy()
    got, _ = run_segments(brb, torch_dev, mode, ctxs, seg, np.zeros_like(low), fin)
    want, _ = run_segments(brb, torch_dev, mode, other, seg, None, fin, lower=False)
    assert np.array_equal(got, want)
    for r in range(n):
        if fin[r]:
            assert np.array_equal(ctxs[r, :24], other[r, :24]) and np.array_equal(ctxs[r, 88:], other[r, 88:]), r
        else:
            assert defined(ctxs[r]) == defined(other[r]) and np.array_equal(ctxs[r, 88:], other[r, 88:]), r


@pytest.mark.parametrize("mode", ["host", "device"])
def test_no_seg_lower_is_all_ones(brb, torch_dev, mode):
    rng = np.random.default_rng(39)
    n = 300
    ctxs = contexts_with(brb, rng.integers(0, 64, n), rng)
    seg, low = _random_case(brb, rng, n, far_empty=mode == "host")
    fin = rng.integers(0, 2, n).astype(np.uint8)
    other, before = ctxs.copy(), ctxs.copy()
    got, _ = run_segments(brb, torch_dev, mode, ctxs, seg, None, fin)
    ones, _ = run_segments(brb, torch_dev, mode, other, seg, np.ones_like(low), fin)
    assert np.array_equal(got, ones)
    assert np.array_equal(ctxs[:, :24], other[:, :24]) and np.array_equal(ctxs[:, 88:], other[:, 88:])
    want, digs = reference(brb, before, range(n), seg, None, fin)
    check(ctxs, before, want, range(n), seg, digs, got)


@pytest.mark.parametrize("mode", MODES)
def test_random_segments(brb, torch_dev, mode):
    """300 items through a sparse index: 0 to 4 segments of 0 to 300 bytes, random flags, alignment and final."""
    rng = np.random.default_rng(40)
    n, n_ctx = 300, 640
    idx = rng.permutation(n_ctx)[:n].astype(np.uint32)
    named = idx.astype(np.int64)
    ctxs = contexts_with(brb, rng.integers(0, 64, n_ctx), rng, fill=0x5C)
    seg, low = _random_case(brb, rng, n, far_empty=mode == "host")
    fin = rng.integers(0, 2, n).astype(np.uint8)
    want, digs = reference(brb, ctxs, named, seg, low, fin)
    before, data0 = ctxs.copy(), seg[0].copy()
    got, after = run_segments(brb, torch_dev, mode, ctxs, seg, low, fin, idx)
    check(ctxs, before, want, named, seg, digs, got)
    assert np.array_equal(after, data0)


def test_contexts_move_between_host_and_batch(brb, torch_dev):
    """200 chains over 5 rounds.  Each round every chain takes a piece, plain or lower-cased: half of the chains
    through the batch call, the other half on the host (md5_ctx_update / md5_ctx_update_lower), the halves drawn
    anew each round.  Every digest equals hashlib of the bytes fed, lower-cased where they were."""
    rng = np.random.default_rng(41)
    n = 200
    ctxs = np.full((n, 168), 0xA5, np.uint8)
    for r in range(n):
        brb.md5_ctx_init(ctxs[r])
    msgs = [b""] * n
    for _ in range(5):
        on_gpu = rng.permutation(n)[:n // 2]
        for r in np.setdiff1d(np.arange(n), on_gpu):
            piece = rng.integers(0x30, 0x80, int(rng.integers(0, 200)), dtype=np.uint8).tobytes()
            if rng.integers(0, 2):
                brb.md5_ctx_update_lower(ctxs[r], piece)
                msgs[r] += lowered(piece)
            else:
                brb.md5_ctx_update(ctxs[r], piece)
                msgs[r] += piece
        seg = lay_out([[k] for k in rng.integers(0, 200, len(on_gpu))], rng, far_empty=False)
        seg[0][:] = rng.integers(0x30, 0x80, len(seg[0]), dtype=np.uint8)
        low = rng.integers(0, 2, len(on_gpu) + 1).astype(np.uint8)
        run_segments(brb, torch_dev, "device", ctxs, seg, low, None, on_gpu.astype(np.uint32))
        for i, r in enumerate(on_gpu):
            piece = seg[0][int(seg[1][i]):int(seg[1][i]) + int(seg[2][i])].tobytes()
            msgs[r] += lowered(piece) if low[i] else piece
    seg = (np.zeros(8, np.uint8), np.zeros(1, np.uint64), np.zeros(1, np.uint32), np.zeros(n + 1, np.uint64))
    got, _ = run_segments(brb, torch_dev, "device", ctxs, seg, np.zeros(1, np.uint8), np.ones(n, np.uint8))
    assert [got[r].tobytes() for r in range(n)] == [hashlib.md5(m).digest() for m in msgs]
    assert [ctxs[r, 104:137].tobytes() for r in range(n)] == [hashlib.md5(m).hexdigest().encode() + b"\0" for m in msgs]
