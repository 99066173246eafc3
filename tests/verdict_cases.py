"""Deterministic inputs for the verdict sweeps (test_verdicts_cpu.py, test_verdicts.py).

A helper, not a test module: nothing here is collected by pytest and nothing touches a GPU.  Three
places of the library answer with a decision instead of data, and a wrong decision is silent:

* ``frame_table``  -- BRB_RC4MD5_OpenBatch's ``valid`` (and the batcher's READ callback): frames the
                      oracle wrote for 16 payload lengths, each untampered, with every single bit of
                      every byte flipped, and with its length off by one or cut to 30 and 29 bytes.
                      ``frame_rule`` is what ev_kq_aio_transform.c:158-184 does: it compares "HASH:"
                      and the 16 digest bytes and nothing else, so a flip in the salt (bytes 0..7) or
                      the NUL (byte 29) leaves a frame valid and any other flip makes it invalid.
* ``md_table``     -- BRB_MetaDataUnpack(Items)Batch's ``error_code``: five valid packs, every bit of
                      the four small ones and every bit of the 4 x 375 pack's header, item headers,
                      canaries and the data bytes at the items' ends and the 64-byte block edges.
                      ``md_rule_breaks`` is the rule by region of meta_data.c:145-328: version, size,
                      the reserved bytes and the ids are not looked at; the magic, the digest, the data
                      and the canaries each have their code.
* ``mb_cases``     -- MemBufferDecrypt's stop at the first pair holding a zero 64-bit word
                      (mem_buf.c:1595-1596): words that are zero in one half only (they must not stop
                      it), true zeros as xl, xr and both, and buffers with two zero pairs (the lower wins).

Every seed is written here; the tables are the same on every run and in both modules.
"""
import hashlib
import struct

import numpy as np

SEED_FRAMES = 0x56524446               # "VRDF": payload bytes
SEED_PACKS = 0x56524450                # "VRDP": item ids and data, gap bytes
SEED_WORDS = 0x56524457                # "VRDW": MemBuffer words

# ---- A. frames ---------------------------------------------------------------------------------------------
# Frame block 0 holds payload bytes 0..33; MD5 padding turns over at 55/56 and 119/120; the second MD5
# block starts at payload byte 64.
FRAME_LENS = (0, 1, 2, 33, 34, 35, 55, 56, 63, 64, 65, 98, 99, 119, 120, 128)
FRAME_KEY = bytes((37 * k + 11) & 0xFF for k in range(19))
FRAME_SALT = 0x0123456789ABCDEF
HEADER = 30                            # salt(8) "HASH:"(5) md5(16) NUL(1)
SENTINEL, OUT_FILL = 0xA5, 0x5A        # between frames in the input; an out-of-place output's fill
EXTRA = 0xC3                           # the byte that follows a frame given with one byte more
PLAIN, FLIP, MINUS1, PLUS1, CUT30, CUT29 = range(6)
UNCHECKED_BYTES = tuple(range(8)) + (29,)
N_FLIPS = 8 * sum(HEADER + L for L in FRAME_LENS)      # 11 616


class FrameTable:
    """L, kind, pos, bit: one entry per frame (pos = bit = -1 unless kind == FLIP); frames: their bytes;
    data: all frames with one SENTINEL byte before, between and eight after; offs, lens, mask: where
    they lie; states: one copy of the key's initial state per frame; rule: frame_rule's verdicts."""


def frame_rule(kind, pos, L):
    """The verdict by structure: untampered frames, flips in bytes 0..7 and 29, and the cut to 30 bytes of
    the empty payload's frame (which is that frame) are valid; everything else is not."""
    kind, pos, L = np.asarray(kind), np.asarray(pos), np.asarray(L)
    ok = (kind == PLAIN) | ((kind == FLIP) & ((pos < 8) | (pos == 29))) | ((kind == CUT30) & (L == 0))
    return ok.astype(np.uint8)


def frame_table(orc):
    t = FrameTable()
    rng = np.random.default_rng(SEED_FRAMES)
    state0 = orc.rc4_init(FRAME_KEY)
    rows, frames = [], []
    for L in FRAME_LENS:
        payload = rng.integers(0, 256, L, dtype=np.uint8).tobytes()
        f = orc.rc4md5_frame(state0, payload, FRAME_SALT)[1]
        assert len(f) == HEADER + L
        rows.append((L, PLAIN, -1, -1))
        frames.append(f)
        for pos in range(len(f)):
            for bit in range(8):
                g = bytearray(f)
                g[pos] ^= 1 << bit
                rows.append((L, FLIP, pos, bit))
                frames.append(bytes(g))
        for kind, g in ((MINUS1, f[:-1]), (PLUS1, f + bytes([EXTRA])), (CUT30, f[:30]), (CUT29, f[:29])):
            rows.append((L, kind, -1, -1))
            frames.append(g)
    t.L, t.kind, t.pos, t.bit = (np.array(c, np.int64) for c in zip(*rows))
    t.frames = frames
    t.lens = np.array([len(f) for f in frames], np.uint32)
    t.offs = (np.cumsum(t.lens.astype(np.uint64) + np.uint64(1)) - t.lens).astype(np.uint64)   # one sentinel first
    sent = bytes([SENTINEL])
    t.data = np.frombuffer(sent + b"".join(f + sent for f in frames) + 7 * sent, np.uint8).copy()
    t.mask = np.ones(t.data.size, bool)
    t.mask[0] = False
    t.mask[(t.offs + t.lens).astype(np.int64)] = False
    t.mask[-7:] = False
    assert (t.data[~t.mask] == SENTINEL).all() and int(t.mask.sum()) == int(t.lens.sum())
    t.states = np.tile(np.frombuffer(state0, np.uint8), (len(frames), 1))
    t.rule = frame_rule(t.kind, t.pos, t.L)
    for a in vars(t).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return t


def frame_expect(orc, t):
    """The oracle's open of the whole table: (buffer after an in-place open, states after, valid)."""
    buf, st, ok = t.data.copy(), t.states.copy(), np.full(len(t.frames), 0xEE, np.uint8)
    orc.rc4md5_open_batch(st, buf, t.offs, t.lens, ok)
    for a in (buf, st, ok):
        a.setflags(write=False)
    return buf, st, ok


# ---- B. MetaData packs -------------------------------------------------------------------------------------
MD_BASES = ((4, 375), (1, 7), (3, 9), (2, 64), (0, 0))       # (items, bytes per item); the first is the bench layout
MD_HEADER = 64
(R_VERSION, R_COUNT, R_SIZE, R_MAGIC, R_DIGEST, R_RESERVED, R_ID, R_SUB, R_SZ, R_DATA, R_CANARY) = range(11)
R_NAMES = ("version", "item_count", "size", "magic", "digest", "reserved", "id", "sub_id", "sz", "data", "canary")
R_UNCHECKED = (R_VERSION, R_SIZE, R_RESERVED, R_ID, R_SUB)
INFO_DTYPE = np.dtype([("error_code", "<i4"), ("item_count", "<u4"), ("cur_offset", "<u8"), ("cur_remaining", "<u8"),
                       ("cur_needed", "<u8")])                # BRB_MetaDataUnpackInfo
MAGIC_INVALID, CANARY, DIGEST_INVALID, SUCCESS = 0, 3, 4, 7


def md_pack(items) -> bytes:
    """MetaDataPack by struct (LP64 layout of libbrb_data.h:313-330), digest by hashlib."""
    body = b"".join(struct.pack("<QQQ", i, s, len(d)) + d + b"\x1f" for i, s, d in items)
    dig = hashlib.md5(b"".join(d for _, _, d in items)).digest()
    return struct.pack("<iiQ8s16s24s", 0, len(items), len(body), b"BRB_META", dig, bytes(24)) + body


def md_regions(n_items, item_len):
    """The region of every byte of a pack of n_items items of item_len bytes."""
    r = [R_VERSION] * 4 + [R_COUNT] * 4 + [R_SIZE] * 8 + [R_MAGIC] * 8 + [R_DIGEST] * 16 + [R_RESERVED] * 24
    for _ in range(n_items):
        r += [R_ID] * 8 + [R_SUB] * 8 + [R_SZ] * 8 + [R_DATA] * item_len + [R_CANARY]
    return np.array(r, np.uint8)


def md_flip_bytes(n_items, item_len):
    """The bytes whose every bit is flipped: the whole of a small pack; of the 4 x 375 pack the header, every
    item header and canary, the first and last 8 data bytes of each item and the data bytes on either side
    of a 64-byte block edge of the pack."""
    reg = md_regions(n_items, item_len)
    if reg.size <= 256:
        return np.arange(reg.size)
    keep = reg != R_DATA
    stride = 24 + item_len + 1
    for j in range(n_items):
        d0 = MD_HEADER + j * stride + 24
        keep[d0:d0 + 8] = True
        keep[d0 + item_len - 8:d0 + item_len] = True
    edge = np.arange(reg.size)
    keep |= (reg == R_DATA) & ((edge % 64 == 0) | (edge % 64 == 63))
    return np.flatnonzero(keep)


class MdTable:
    """items[b], base_pack[b]: the five valid packs; packs: every case's bytes; base, pos, bit, region: one
    entry per case (pos = bit = region = -1 for the five untampered packs, which come first)."""


def md_table():
    t = MdTable()
    rng = np.random.default_rng(SEED_PACKS)
    t.items, t.base_pack = [], []
    for n_items, item_len in MD_BASES:
        t.items.append([(int(rng.integers(0, 1 << 64, dtype=np.uint64)), int(rng.integers(0, 1 << 64, dtype=np.uint64)),
                         rng.integers(1, 256, item_len, dtype=np.uint8).tobytes()) for _ in range(n_items)])
        t.base_pack.append(md_pack(t.items[-1]))
    rows = [(b, -1, -1, -1) for b in range(len(MD_BASES))]
    packs = list(t.base_pack)
    for b, (n_items, item_len) in enumerate(MD_BASES):
        reg = md_regions(n_items, item_len)
        assert reg.size == len(t.base_pack[b])
        for pos in md_flip_bytes(n_items, item_len).tolist():
            for bit in range(8):
                g = bytearray(t.base_pack[b])
                g[pos] ^= 1 << bit
                rows.append((b, pos, bit, int(reg[pos])))
                packs.append(bytes(g))
    t.base, t.pos, t.bit, t.region = (np.array(c, np.int64) for c in zip(*rows))
    t.packs = packs
    for a in (t.base, t.pos, t.bit, t.region):
        a.setflags(write=False)
    return t


def md_oracle_info(orc, packs):
    """orc.metadata_unpack_batch of the packs laid back to back -> INFO_DTYPE[n]."""
    lens = np.array([len(p) for p in packs], np.uint32)
    offs = (np.cumsum(lens.astype(np.uint64)) - lens).astype(np.uint64)
    buf = np.frombuffer(b"".join(packs) + b"\0", np.uint8).copy()
    return orc.metadata_unpack_batch(buf, offs, lens).reshape(-1).view(INFO_DTYPE).copy()


def md_rule_breaks(t, info):
    """The cases of t whose info (INFO_DTYPE[n], in t's order) breaks the rule by region; [] when it holds.
    item_count and sz flips have no rule of their own (the oracle decides)."""
    info = np.asarray(info).reshape(-1).view(INFO_DTYPE)
    n_bases = len(MD_BASES)
    full = np.array([m for m, _ in MD_BASES], np.uint32)[t.base]
    same_as_base = info == info[:n_bases][t.base]
    code, reg = info["error_code"], t.region
    ok = np.ones(len(t.packs), bool)
    for r in (-1,) + R_UNCHECKED:
        ok &= (reg != r) | (same_as_base & (code == SUCCESS))
    ok &= (reg != R_MAGIC) | (info == np.zeros(1, INFO_DTYPE)[0])
    ok &= ~((reg == R_DIGEST) | (reg == R_DATA)) | ((code == DIGEST_INVALID) & (info["item_count"] == full))
    ok &= (reg != R_CANARY) | (code == CANARY)
    return np.flatnonzero(~ok).tolist()


def md_layout(packs, align, seed):
    """The packs in one buffer, every offset congruent to align mod 4, 1..4 random bytes between them (and
    before the first, so align 0 starts at 4) and after the last, the buffer a multiple of 4 bytes so that
    several can be joined: -> (buf, offs uint64, lens uint32)."""
    rng = np.random.default_rng(seed)
    lens = np.array([len(p) for p in packs], np.uint32)
    offs, pos = np.zeros(len(packs), np.uint64), 0
    for k, n in enumerate(lens.tolist()):
        pos += (align - pos - 1) % 4 + 1
        offs[k] = pos
        pos += n
    buf = rng.integers(0, 256, (pos + 4) // 4 * 4, dtype=np.uint8)
    for o, p in zip(offs.tolist(), packs):
        buf[o:o + len(p)] = np.frombuffer(p, np.uint8)
    return buf, offs, lens


# ---- C. MemBuffer decrypt stop -----------------------------------------------------------------------------
MB_SEED = 0x4FD9                       # the Blowfish seed of every buffer
MB_PAIRS = 768                         # (xl, xr) pairs per small buffer
MB_BIG_PAIRS = 2048 * 256 + 1024       # just over 8 MiB: past first_zero_pair_kernel's grid of 2048 x 256 threads
MB_GUARD = 0xEE                        # 16 guard bytes before, between and after the buffers
MB_CLASS_PAIRS = (0, 1, 63, 64, 65, 255, 256, MB_PAIRS - 1)   # where a word class is placed
MB_TWO_ZEROS = ((3, 700), (255, 256), (64, 128), (65, 128))
MB_BIG_TWO_ZEROS = ((2048 * 256 + 5, 2048 * 256 + 4), (300, 2048 * 256 + 300))


def mb_size(pairs):
    """The MemBuffer size with which a decrypt call walks exactly `pairs` pairs (mem_buf.c:1557-1558, :1571)."""
    return 16 * (pairs - 1)


def _nonzero_words(rng, n):
    """n 64-bit words with both 32-bit halves non-zero."""
    hi, lo = rng.integers(1, 1 << 32, n, dtype=np.uint64), rng.integers(1, 1 << 32, n, dtype=np.uint64)
    return (hi << np.uint64(32)) | lo


def mb_word_classes(rng):
    """Words that are not zero but are zero in one half, or in all bits but one."""
    r = lambda: int(rng.integers(1, 1 << 32))
    return (("low_half_zero", r() << 32), ("high_half_zero", r()), ("one", 1), ("bit32", 1 << 32), ("bit63", 1 << 63))


class MbCase:
    def __init__(self, name, words, stop):
        self.name, self.words, self.stop = name, words, stop      # stop: the pair the decrypt stops at, or None
        words.setflags(write=False)

    @property
    def new_size(self):
        return 16 * (self.words.size // 2 if self.stop is None else self.stop)


def mb_cases():
    """37 buffers of MB_PAIRS pairs, stopping and non-stopping ones interleaved (so both share a group of 16
    slots of the keyed kernel): a word class at MB_CLASS_PAIRS as xl or as xr, alone (10) and before a true
    zero at pair 500 (10); one true zero as xl, as xr and as both at pairs 0, 77 and the last (9); two zero
    pairs in the order lower-higher, on either side (8)."""
    rng = np.random.default_rng(SEED_WORDS)
    out = []

    def add(name, puts, stop):
        w = _nonzero_words(rng, 2 * MB_PAIRS)
        for pair, side, v in puts:
            w[2 * pair + side] = np.uint64(v)
        out.append(MbCase(name, w, stop))

    for cname, v in mb_word_classes(rng):
        for side in (0, 1):
            puts = [(p, side, v) for p in MB_CLASS_PAIRS]
            add(f"{cname}_as_{'xl xr'.split()[side]}", puts, None)
            add(f"{cname}_as_{'xl xr'.split()[side]}_then_zero", puts + [(500, 1 - side, 0)], 500)
    for pair in (0, 77, MB_PAIRS - 1):
        add(f"zero_xl_at_{pair}", [(pair, 0, 0)], pair)
        add(f"zero_xr_at_{pair}", [(pair, 1, 0)], pair)
        add(f"zero_both_at_{pair}", [(pair, 0, 0), (pair, 1, 0)], pair)
    for a, b in MB_TWO_ZEROS:
        add(f"zeros_at_{a}_{b}_xl_xr", [(a, 0, 0), (b, 1, 0)], a)
        add(f"zeros_at_{a}_{b}_xr_xl", [(a, 1, 0), (b, 0, 0)], a)
    n = len(out)
    return [out[(7 * k) % n] for k in range(n)]                    # 7 and 37 are coprime: a permutation


def mb_big_cases():
    """Two buffers of MB_BIG_PAIRS pairs for the single call: zero pairs in two threads of the scan's second
    sweep (the higher thread holds the lower pair), and in two iterations of one thread."""
    rng = np.random.default_rng(SEED_WORDS + 1)
    out = []
    for k, (a, b) in enumerate(MB_BIG_TWO_ZEROS):
        w = _nonzero_words(rng, 2 * MB_BIG_PAIRS)
        w[2 * a + (k & 1)] = w[2 * b + 1 - (k & 1)] = np.uint64(0)
        out.append(MbCase(f"big_zeros_at_{a}_{b}", w, min(a, b)))
    return out


def mb_layout(cases):
    """The cases' words in one buffer with 16 guard bytes around each: -> (data uint8, offs, sizes uint64)."""
    room = [16 * (c.words.size // 2) for c in cases]
    offs = (16 + np.cumsum([0] + [r + 16 for r in room[:-1]])).astype(np.uint64)
    data = np.full(int(offs[-1]) + room[-1] + 16, MB_GUARD, np.uint8)
    for o, c in zip(offs.tolist(), cases):
        data[o:o + 8 * c.words.size] = c.words.view(np.uint8)
    sizes = np.array([mb_size(c.words.size // 2) for c in cases], np.uint64)
    return data, offs, sizes


def mb_expect(orc, cases, data, offs, sizes):
    """orc.membuf_decrypt of every buffer on its own bytes: -> (the whole data expected, new sizes uint64)."""
    want, new = data.copy(), []
    for o, size, c in zip(offs.tolist(), sizes.tolist(), cases):
        b = bytearray(want[o:o + 8 * c.words.size].tobytes())
        new.append(orc.membuf_decrypt(b, size, MB_SEED, 0))
        want[o:o + len(b)] = np.frombuffer(bytes(b), np.uint8)
    return want, np.array(new, np.uint64)
