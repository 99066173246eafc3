"""Every bit behind a verdict, on the card: frame open (`valid`), MetaData unpack (`error_code`) and the
MemBuffer decrypt stop, swept with the tables of tests/verdict_cases.py.

The three answers are decisions a caller acts on, and the other modules reach them with a handful of
random single-byte hits.  Here every bit is flipped: all 11 616 bits of 16 frames (plus their lengths off
by one and cut to 30 and 29 bytes), every bit of four small MetaData packs and of the header, item headers,
canaries, item ends and 64-byte block edges of the bench's 4 x 375 pack (6 733 packs, each at byte
alignments 0..3), and the 64-bit words that are zero in one half only, next to true zeros and two zero
pairs per buffer.  Every comparison is bit for bit against the C oracle, and the verdicts also against the
structural rules (test_verdicts_cpu.py shows that the oracle obeys them and that the tables hold what
they claim): a frame stays valid exactly under flips of bytes 0..7 and 29; version, size, the reserved
bytes and the ids of a pack are not looked at, while the magic, the digest, the data and the canaries each
have their code.  A verdict never shortens the work: the decrypted bytes, all 264 bytes of every RC4
state, the item table and the sentinels around every output are compared for every case, valid or not.

DESIGN.md section 4.3 ("What guards the verdicts") has the time each test takes on an MI355X and the five
one-line wrong libraries the module was run against, each of which fails here.
"""
import importlib.util
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _sibling(name):
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
        sys.modules[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[name])
    return sys.modules[name]


V = _sibling("verdict_cases")
walk = _sibling("test_metadata_items_cpu")


@pytest.fixture(scope="module")
def torch_dev(brb):
    import torch
    assert torch.cuda.is_available(), "no HIP device visible to torch"
    assert brb.gpu_available(), brb.lib().BRB_CryptoGPU_LastError()
    return torch


def _to(torch, a):
    """A device copy (the shared arrays are read-only); unsigned 64 / 32-bit arrays as int64 / int32 tensors."""
    a = np.array(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _bad_rows(got, want):
    return np.nonzero((got != want).any(axis=1))[0][:8].tolist()


# ---- A. frame open -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames(orc):
    t = V.frame_table(orc)
    return t, V.frame_expect(orc, t)


def _frame_names(t, idx):
    return [(int(t.L[i]), int(t.kind[i]), int(t.pos[i]), int(t.bit[i])) for i in idx[:8]]


@pytest.mark.parametrize("pair", [1, 0], ids=["pair", "single"])
def test_open_batch_every_bit(brb, torch_dev, frames, pair):
    """BRB_RC4MD5_OpenBatch on the whole table in one batch, device mode in place and host mode out of place:
    valid against the oracle and against the rule, the decrypted bytes, all 264 bytes of every state and the
    sentinel bytes between the frames."""
    torch, (t, (want_buf, want_st, want_ok)) = torch_dev, frames
    with brb.TestOption("rc4md5_pair", pair):
        ts, tb = _to(torch, t.states), _to(torch, t.data)
        _, valid = brb.rc4md5_open_batch(ts, tb, _to(torch, t.offs), _to(torch, t.lens), async_=bool(pair))
        torch.cuda.synchronize()
        if pair:
            brb.async_fault_check()
        hs, out = t.states.copy(), np.full_like(t.data, V.OUT_FILL)
        _, hv = brb.rc4md5_open_batch(hs, t.data.copy(), t.offs.copy(), t.lens.copy(), out=out)
        if pair:
            brb.async_fault_check()
    for mode, got_ok, got_st, got_buf, want in (
            ("device", valid.cpu().numpy(), ts.cpu().numpy(), tb.cpu().numpy(), want_buf),
            ("host", hv, hs, out, np.where(t.mask, want_buf, np.uint8(V.OUT_FILL)))):
        bad = np.flatnonzero(got_ok != want_ok)
        assert bad.size == 0, (mode, "valid differs from the oracle", bad.size, _frame_names(t, bad))
        bad = np.flatnonzero(got_ok != t.rule)
        assert bad.size == 0, (mode, "valid breaks the rule", bad.size, _frame_names(t, bad))
        assert np.array_equal(got_st, want_st), (mode, _bad_rows(got_st, want_st))
        assert np.array_equal(got_buf[t.mask], want[t.mask]), mode
        assert np.array_equal(got_buf, want), (mode, "a byte between two frames changed")


@pytest.mark.parametrize("zero_copy", [False, True], ids=["copy", "zero_copy"])
def test_batcher_read_every_bit(brb, torch_dev, frames, zero_copy):
    """TransformBatcher, RC4+MD5: the L = 35 and L = 65 tables, one connection per frame, one round: every
    READ callback's valid and out, and every read state afterwards, equal the oracle's."""
    t, (want_buf, want_st, want_ok) = frames
    idx = np.flatnonzero(np.isin(t.L, (35, 65)) & (t.kind <= V.FLIP)).tolist()
    assert len(idx) == 8 * (65 + 95) + 2
    b = brb.TransformBatcher(len(idx), 1 << 20, brb.CRYPTO_FUNC_RC4_MD5, zero_copy=zero_copy)
    try:
        b.enable_batch(np.arange(len(idx)), [V.FRAME_KEY] * len(idx))
        for c, i in enumerate(idx):
            assert b.read(c, t.frames[i]) == 1
        got = b.flush()
        assert len(got) == len(idx)
        bad = []
        for c, (i, g) in enumerate(zip(idx, got)):
            o = int(t.offs[i])
            if g != (c, brb.OP_READ, want_buf[o:o + int(t.lens[i])].tobytes(), int(want_ok[i])) or g[3] != t.rule[i]:
                bad.append(i)
        assert not bad, (len(bad), _frame_names(t, bad))
        bad = [i for c, i in enumerate(idx) if b.state(c, brb.OP_READ) != want_st[i].tobytes()]
        assert not bad, (len(bad), _frame_names(t, bad))
    finally:
        b.close()


# ---- B. MetaData unpack ------------------------------------------------------------------------------------
GUARD = 37
S64, S32 = 0xA5C3A5C3A5C3A5C3, 0xA5C3A5C3


class Packs:
    """The table at pack byte alignments 0, 1, 2 and 3 in one buffer (4 n packs), the oracle's info for every
    pack and the item table of tests/test_metadata_items_cpu.py's walker, laid out with exact slot counts
    between GUARD sentinel slots."""

    def __init__(self, orc):
        t = self.t = V.md_table()
        n = len(t.packs)
        info = V.md_oracle_info(orc, t.packs)
        walked = [walk.py_unpack_items(p) for p in t.packs]
        five = [tuple(int(x) for x in r) for r in info.tolist()]
        assert five == [w[0] for w in walked]
        assert V.md_rule_breaks(t, info) == []
        parts, offs, lens, base = [], [], [], 0
        for align in range(4):
            buf, o, ln = V.md_layout(t.packs, align, V.SEED_PACKS + 1 + align)
            assert ((o + np.uint64(base)) % np.uint64(4) == align).all() and buf.size % 4 == 0
            parts.append(buf)
            offs.append(o + np.uint64(base))
            lens.append(ln)
            base += buf.size
        self.buf, self.offs, self.lens = np.concatenate(parts), np.concatenate(offs), np.concatenate(lens)
        self.info = np.concatenate([info] * 4)
        self.case = np.tile(np.arange(n), 4)
        self.added = np.tile(np.array([len(w[1]) for w in walked], np.uint32), 4)
        self.first = np.full(4 * n + 1, GUARD, np.uint64)
        self.first[1:] += np.cumsum(self.added.astype(np.uint64))
        total = int(self.first[-1]) + GUARD
        self.table = [np.full(total, S64, np.uint64), np.full(total, S32, np.uint32), np.full(total, S64, np.uint64),
                      np.full(total, S64, np.uint64)]
        rows = np.array([e for w in walked for e in w[1]], np.uint64).reshape(-1, 4)      # (offset, sz, id, sub)
        per = int(self.added[:n].sum())
        assert rows.shape[0] == per
        for a in range(4):
            s = int(self.first[a * n])
            shift = np.repeat(self.offs[a * n:(a + 1) * n], self.added[:n].astype(np.int64))
            self.table[0][s:s + per] = rows[:, 0] + shift
            self.table[1][s:s + per] = rows[:, 1].astype(np.uint32)
            self.table[2][s:s + per] = rows[:, 2]
            self.table[3][s:s + per] = rows[:, 3]
        for a in [self.buf, self.offs, self.lens, self.info, self.added, self.first] + self.table:
            a.setflags(write=False)

    def name(self, k):
        i = int(self.case[k])
        return (f"align {k // len(self.t.packs)}", V.MD_BASES[int(self.t.base[i])], V.R_NAMES[int(self.t.region[i])],
                int(self.t.pos[i]), int(self.t.bit[i]))

    def check_info(self, got, what):
        got = np.ascontiguousarray(got).reshape(-1).view(V.INFO_DTYPE)
        bad = np.flatnonzero(got != self.info)
        assert bad.size == 0, (what, bad.size, [(self.name(k), got[k].tolist(), self.info[k].tolist()) for k in bad[:4]])
        n = len(self.t.packs)
        for a in range(4):
            bad = V.md_rule_breaks(self.t, got[a * n:(a + 1) * n])
            assert not bad, (what, "the rule by region", len(bad), [self.name(a * n + i) for i in bad[:4]])


@pytest.fixture(scope="module")
def packs(orc):
    return Packs(orc)


def test_md_sweep_shape(packs):
    n = len(packs.t.packs)
    assert packs.offs.size == 4 * n and {int(o) & 3 for o in packs.offs[:n]} == {0}
    assert [int(packs.offs[a * n]) & 3 for a in range(4)] == [0, 1, 2, 3]
    assert set(packs.info["error_code"].tolist()) == {0, 3, 4, 5, 6, 7}


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("seg_line", [2, 1, 0])
def test_unpack_batch_every_bit(brb, torch_dev, packs, seg_line, device):
    """BRB_MetaDataUnpackBatch on every flip at every alignment: every BRB_MetaDataUnpackInfo field against
    the oracle, then the rule by region.  seg_line 2: wave pairs, 1: the line kernel, 0: the per-lane kernel."""
    torch, p = torch_dev, packs
    with brb.TestOption("seg_line", seg_line):
        if device:
            got = brb.metadata_unpack_batch(_to(torch, p.buf), _to(torch, p.offs), _to(torch, p.lens)).cpu().numpy()
        else:
            got = brb.metadata_unpack_batch(p.buf.copy(), p.offs.copy(), p.lens.copy())
    p.check_info(got, "BRB_MetaDataUnpackBatch")


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("seg_line", [2, 0])
def test_unpack_items_batch_every_bit(brb, torch_dev, packs, seg_line, device):
    """BRB_MetaDataUnpackItemsBatch with exact slot counts: info as above, items_added, and the four table
    arrays whole -- a flipped id or sub-id bit shows in the table under a SUCCESS verdict, and the guard slots
    around the call's slots keep their sentinels."""
    torch, p = torch_dev, packs
    table = [np.full(w.size, S32 if w.dtype == np.uint32 else S64, w.dtype) for w in p.table]
    added = np.full(p.offs.size, S32, np.uint32)
    with brb.TestOption("seg_line", seg_line):
        if device:
            tt, ta = [_to(torch, a) for a in table], _to(torch, added)
            info, _ = brb.metadata_unpack_items_batch(_to(torch, p.buf), _to(torch, p.offs), _to(torch, p.lens), *tt,
                                                      _to(torch, p.first), items_added=ta)
            info, added = info.cpu().numpy(), ta.cpu().numpy().view(np.uint32)
            table = [x.cpu().numpy().view(w.dtype) for x, w in zip(tt, p.table)]
        else:
            info, _ = brb.metadata_unpack_items_batch(p.buf.copy(), p.offs.copy(), p.lens.copy(), *table, p.first.copy(),
                                                      items_added=added)
    p.check_info(info, "BRB_MetaDataUnpackItemsBatch")
    bad = np.flatnonzero(added != p.added)
    assert bad.size == 0, ("items_added", bad.size, [p.name(k) for k in bad[:4]])
    for name, got, want in zip(("item_offsets", "item_lengths", "item_ids", "item_sub_ids"), table, p.table):
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (name, bad.size, int(bad[0]), p.name(int(np.searchsorted(p.first, bad[0], side="right")) - 1)
                               if GUARD <= bad[0] < int(p.first[-1]) else "a guard slot",
                               hex(int(got[bad[0]])), hex(int(want[bad[0]])))


# ---- C. MemBuffer decrypt stop -----------------------------------------------------------------------------
class Buffers:
    def __init__(self, orc, cases):
        self.cases = cases
        self.data, self.offs, self.sizes = V.mb_layout(cases)
        self.want, self.new = V.mb_expect(orc, cases, self.data, self.offs, self.sizes)
        assert self.new.tolist() == [c.new_size for c in cases]
        for a in (self.data, self.offs, self.sizes, self.want, self.new):
            a.setflags(write=False)

    def check(self, got, new, what):
        bad = np.flatnonzero(np.asarray(new, np.uint64) != self.new)
        assert bad.size == 0, (what, "new_size", [(self.cases[k].name, int(new[k]), int(self.new[k])) for k in bad[:6]])
        for c, o, ns in zip(self.cases, self.offs.tolist(), self.new.tolist()):
            end = o + 8 * c.words.size
            assert np.array_equal(got[o:o + ns], self.want[o:o + ns]), (what, c.name, "decrypted bytes")
            assert np.array_equal(got[o + ns:end], self.data[o + ns:end]), (what, c.name, "bytes from the stop onward")
        assert np.array_equal(got, self.want), (what, "a guard byte changed")


@pytest.fixture(scope="module")
def buffers(orc):
    return Buffers(orc, V.mb_cases())


@pytest.fixture(scope="module")
def big_buffers(orc):
    return Buffers(orc, V.mb_big_cases())


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_membuf_decrypt_batch_stop(brb, torch_dev, buffers, device):
    """BRB_MemBufferDecryptBatch on the 37 interleaved buffers (three groups of 16 slots): new_sizes, every
    decrypted byte, every byte from the stop onward and the guard bytes between the buffers."""
    torch, b = torch_dev, buffers
    if device:
        d = _to(torch, b.data)
        new = brb.membuf_decrypt_batch(d, _to(torch, b.offs), _to(torch, b.sizes), [V.MB_SEED])
        got, new = d.cpu().numpy(), new.cpu().numpy().view(np.uint64)
    else:
        got = b.data.copy()
        new = brb.membuf_decrypt_batch(got, b.offs.copy(), b.sizes.copy(), [V.MB_SEED])
    b.check(got, new, "BRB_MemBufferDecryptBatch")


def _single_calls(brb, torch, b, device):
    whole = _to(torch, b.data) if device else b.data.copy()
    new = []
    for c, o, size in zip(b.cases, b.offs.tolist(), b.sizes.tolist()):
        new.append(brb.membuf_decrypt(whole[o:o + 8 * c.words.size], size, V.MB_SEED, 0))
    return (whole.cpu().numpy() if device else whole), new


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_membuf_decrypt_stop(brb, torch_dev, buffers, device):
    """BRB_MemBufferDecrypt, one call per buffer of the same 37."""
    got, new = _single_calls(brb, torch_dev, buffers, device)
    buffers.check(got, new, "BRB_MemBufferDecrypt")


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_membuf_decrypt_stop_past_the_grid(brb, torch_dev, big_buffers, device):
    """BRB_MemBufferDecrypt on buffers of more than 2048 x 256 pairs: zero pairs that two threads find in their
    second sweep (the lower pair in the higher thread), and that one thread meets in two sweeps."""
    got, new = _single_calls(brb, torch_dev, big_buffers, device)
    big_buffers.check(got, new, "BRB_MemBufferDecrypt")
