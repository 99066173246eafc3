"""The verdict sweeps without a GPU: the oracle obeys the structural rules, and the case tables hold
every bit they claim to (tests/verdict_cases.py; the GPU half is tests/test_verdicts.py).

The GPU tests compare the library with the oracle on these tables, so two things are pinned here: that the
oracle's own verdicts are the ones the reference's code gives by construction (a flip in a byte it
does not look at changes nothing, a flip in one it checks has that check's answer), and that the tables
cannot be thinned quietly: the floors below fail when a region of bits leaves a table.  (Tried once:
with the digest bytes 13..28 left out of frame_table's flips, test_frame_table_floors fails; with
R_DIGEST bytes left out of md_flip_bytes, test_md_table_floors fails.)
"""
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _sibling(name):
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
        sys.modules[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[name])
    return sys.modules[name]


V = _sibling("verdict_cases")
walk = _sibling("test_metadata_items_cpu")
cases = walk.cases                                   # tests/test_metadata.py: py_unpack, build


# ---- A. frames ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames(orc):
    t = V.frame_table(orc)
    return t, V.frame_expect(orc, t)


def test_frame_table_floors(frames):
    t, _ = frames
    flips = t.kind == V.FLIP
    assert int(flips.sum()) == V.N_FLIPS == 11616 and len(t.frames) == V.N_FLIPS + 5 * len(V.FRAME_LENS)
    assert sorted(set(t.L.tolist())) == sorted(V.FRAME_LENS) and len(V.FRAME_LENS) == 16
    for L in V.FRAME_LENS:
        here = flips & (t.L == L)
        seen = set(zip(t.pos[here].tolist(), t.bit[here].tolist()))
        assert len(seen) == int(here.sum())                                    # no flip twice
        for lo, hi, what in ((8, 29, "tag and digest"), (0, 8, "salt"), (29, 30, "NUL"), (30, 30 + L, "payload")):
            missing = {(p, b) for p in range(lo, hi) for b in range(8)} - seen
            assert not missing, (L, what, sorted(missing)[:4])
        for kind in (V.PLAIN, V.MINUS1, V.PLUS1, V.CUT30, V.CUT29):
            assert int(((t.kind == kind) & (t.L == L)).sum()) == 1
    # the flips are single bits of the untampered frame, the length tampers its prefixes (or it and one byte)
    plain = {int(L): t.frames[i] for i, L in zip(np.flatnonzero(t.kind == V.PLAIN), t.L[t.kind == V.PLAIN])}
    for i in np.flatnonzero(flips).tolist():
        f, g = plain[int(t.L[i])], t.frames[i]
        diff = [(k, a ^ b) for k, (a, b) in enumerate(zip(f, g)) if a != b]
        assert len(f) == len(g) and diff == [(int(t.pos[i]), 1 << int(t.bit[i]))]
    for i in np.flatnonzero(~flips).tolist():
        f, want = plain[int(t.L[i])], {V.PLAIN: 0, V.MINUS1: -1, V.PLUS1: 1}.get(int(t.kind[i]))
        n = len(f) + want if want is not None else (30 if t.kind[i] == V.CUT30 else 29)
        assert t.frames[i] == (f + bytes([V.EXTRA]))[:n]
    assert {int(o) & 3 for o in t.offs} == {0, 1, 2, 3}


def test_oracle_open_obeys_the_rule(orc, frames):
    """valid == 1 exactly for untampered frames and flips in bytes 0..7 and 29 (ev_kq_aio_transform.c:158-184
    compares "HASH:" and the digest, nothing else); the batch oracle equals the single call; an invalid frame
    is decrypted to its end all the same."""
    t, (buf, st, ok) = frames
    assert np.array_equal(ok, t.rule), np.flatnonzero(ok != t.rule)[:8]
    flips = t.kind == V.FLIP
    assert int(ok[flips].sum()) == 9 * 8 * len(V.FRAME_LENS) and int(ok.sum()) == 9 * 8 * 16 + 16 + 1
    assert np.array_equal(buf[~t.mask], t.data[~t.mask])
    s0 = t.states[0].tobytes()
    for i, f in enumerate(t.frames):
        s2, dec, v = orc.rc4md5_open(s0, f)
        o = int(t.offs[i])
        assert v == ok[i] and s2 == st[i].tobytes() and dec == buf[o:o + len(f)].tobytes(), i
    assert np.array_equal(st[:, 256], (t.lens & 0xFF).astype(np.uint8))      # index1: every byte was decrypted
    # a flipped ciphertext bit is the same flipped plaintext bit (a stream cipher), valid or not
    plain = {int(t.L[i]): i for i in np.flatnonzero(t.kind == V.PLAIN)}
    for i in np.flatnonzero(flips)[::97].tolist():
        o, p = int(t.offs[i]), int(t.offs[plain[int(t.L[i])]])
        x = buf[o:o + int(t.lens[i])] ^ buf[p:p + int(t.lens[i])]
        assert np.flatnonzero(x).tolist() == [int(t.pos[i])] and int(x[t.pos[i]]) == 1 << int(t.bit[i])


# ---- B. MetaData packs -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def packs(orc):
    t = V.md_table()
    return t, V.md_oracle_info(orc, t.packs), [walk.py_unpack_items(p) for p in t.packs]


def test_md_table_floors(orc, packs):
    t, _, _ = packs
    assert [len(p) for p in t.base_pack] == [1664, 96, 166, 242, 64]
    small = sum(8 * len(p) for p in t.base_pack[1:])
    assert small == 4544 and int((t.base > 0).sum()) - 4 == small            # every bit of the small packs
    assert len(t.packs) == len(set(t.packs))                                  # no case twice
    for b, (n_items, item_len) in enumerate(V.MD_BASES):
        assert t.base_pack[b] == orc.metadata_pack(t.items[b]) == cases.build(t.items[b])
        assert all(0 not in d for _, _, d in t.items[b])
        reg = V.md_regions(n_items, item_len)
        here = (t.base == b) & (t.pos >= 0)
        seen = set(zip(t.pos[here].tolist(), t.bit[here].tolist()))
        need = {V.R_VERSION: 32, V.R_COUNT: 32, V.R_SIZE: 64, V.R_MAGIC: 64, V.R_DIGEST: 128, V.R_RESERVED: 192,
                V.R_ID: 64 * n_items, V.R_SUB: 64 * n_items, V.R_SZ: 64 * n_items, V.R_CANARY: 8 * n_items,
                V.R_DATA: 8 * min(item_len, 16) * n_items}
        for r, bits in need.items():
            got = {(p, k) for p, k in seen if reg[p] == r}
            assert len(got) >= bits, (b, V.R_NAMES[r], len(got), bits)
            if r != V.R_DATA:
                assert got == {(int(p), k) for p in np.flatnonzero(reg == r) for k in range(8)}
        for i in np.flatnonzero(here).tolist():
            assert t.region[i] == reg[t.pos[i]]
            g = bytearray(t.base_pack[b])
            g[t.pos[i]] ^= 1 << int(t.bit[i])
            assert t.packs[i] == bytes(g)
    # the 4 x 375 pack: both sides of every 64-byte edge that lies in data, both ends of every item
    big = (t.base == 0) & (t.region == V.R_DATA)
    pos = set(t.pos[big].tolist())
    reg = np.concatenate([V.md_regions(4, 375), np.full(8, V.R_CANARY, np.uint8)])
    for p in range(64, 1664):
        if reg[p] == V.R_DATA and (p % 64 in (0, 63) or reg[p - 8] != V.R_DATA or reg[p + 8] != V.R_DATA):
            assert p in pos, p
    assert 2000 <= int((t.base == 0).sum()) <= 13312


def test_oracle_unpack_obeys_the_rule(orc, packs):
    """Every field against py_unpack and py_unpack_items, then the rule by region; the item_count and sz flips,
    which have no rule of their own, reach codes 3, 4, 5, 6 and 7."""
    t, info, walked = packs
    five = [tuple(int(x) for x in r) for r in info.tolist()]
    for i in range(0, len(t.packs), 41):                                     # the batch oracle is the single call
        assert five[i] == orc.metadata_unpack(t.packs[i])
    for i, p in enumerate(t.packs):
        assert five[i] == walked[i][0], (i, V.R_NAMES[t.region[i]])
        assert five[i] == cases.py_unpack(p), (i, V.R_NAMES[t.region[i]])
    assert V.md_rule_breaks(t, info) == []
    for b, (n_items, item_len) in enumerate(V.MD_BASES):
        n = len(t.base_pack[b])
        assert five[b] == (7, n_items, n, 0, 0) and len(walked[b][1]) == n_items
    free = (t.region == V.R_COUNT) | (t.region == V.R_SZ)
    assert set(info["error_code"][free].tolist()) == {3, 4, 5, 6, 7}
    assert set(info["error_code"].tolist()) == {0, 3, 4, 5, 6, 7}
    # the rule would notice a wrong verdict: one changed code breaks it in that case alone
    for r, code in ((V.R_DIGEST, 7), (V.R_RESERVED, 4), (V.R_CANARY, 4), (V.R_MAGIC, 4)):
        i = int(np.flatnonzero(t.region == r)[5])
        bad = info.copy()
        bad["error_code"][i] = code
        assert V.md_rule_breaks(t, bad) == [i]


def test_id_flips_show_in_the_item_table(packs):
    """A flipped id or sub-id bit leaves the verdict SUCCESS and changes that one table entry by that bit."""
    t, info, walked = packs
    n = 0
    for i in np.flatnonzero((t.region == V.R_ID) | (t.region == V.R_SUB)).tolist():
        b = int(t.base[i])
        n_items, item_len = V.MD_BASES[b]
        j, within = divmod(int(t.pos[i]) - 64, 25 + item_len)
        col, byte = 2 + within // 8, within % 8
        base = walked[b][1]
        want = [list(e) for e in base]
        want[j][col] ^= 1 << (8 * byte + int(t.bit[i]))
        assert info["error_code"][i] == V.SUCCESS and [list(e) for e in walked[i][1]] == want
        n += 1
    assert n == 128 * sum(m for m, _ in V.MD_BASES)


# ---- C. MemBuffer decrypt stop -----------------------------------------------------------------------------
def test_membuf_cases_and_oracle_stop(orc):
    """oracle.membuf_decrypt gives 16 x the lower zero pair for every zero case and the full length for every
    word that is zero in one half only; bytes from the stop on are unchanged, bytes before it are not."""
    cs = V.mb_cases()
    assert len(cs) >= 33 and len({c.name for c in cs}) == len(cs)
    for g in range(0, len(cs), 16):                                          # stopping and not, in every group of 16
        assert {c.stop is None for c in cs[g:g + 16]} == {True, False}, g
    names = " ".join(c.name for c in cs)
    for cname in ("low_half_zero", "high_half_zero", "one", "bit32", "bit63"):
        for side in ("xl", "xr"):
            assert f"{cname}_as_{side} " in names + " " and f"{cname}_as_{side}_then_zero" in names
    for a, b in V.MB_TWO_ZEROS:
        assert f"zeros_at_{a}_{b}_xl_xr" in names and f"zeros_at_{a}_{b}_xr_xl" in names
    for c in cs + V.mb_big_cases():
        w, pairs = c.words, c.words.size // 2
        zero = np.flatnonzero((w[0::2] == 0) | (w[1::2] == 0))
        assert (zero.size == 0) == (c.stop is None) and (c.stop is None or c.stop == int(zero.min()))
        half = np.flatnonzero(((w & np.uint64(0xFFFFFFFF)) == 0) | ((w >> np.uint64(32)) == 0))
        if "zero" not in c.name.replace("half_zero", ""):
            assert c.stop is None and half.size == len(V.MB_CLASS_PAIRS)
        elif "then_zero" in c.name:
            assert int(half.min()) // 2 == 0 < c.stop == 500                 # a 32-bit scan would stop at pair 0
        if c.name.startswith(("zeros_at", "big_zeros_at")):
            assert zero.size == 2 and {int(w[2 * z] == 0) for z in zero} == {0, 1}
        buf = bytearray(w.tobytes())
        got = orc.membuf_decrypt(buf, V.mb_size(pairs), V.MB_SEED, 0)
        assert got == c.new_size == 16 * (pairs if c.stop is None else int(zero.min())), c.name
        after = np.frombuffer(bytes(buf), np.uint64)
        assert np.array_equal(after[got // 8:], w[got // 8:]) and (after[:got // 8] != w[:got // 8]).all(), c.name
    a, b = V.mb_big_cases()
    assert a.words.nbytes > 8 << 20 and a.stop == 2048 * 256 + 4 and b.stop == 300
