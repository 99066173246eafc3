"""Segment lists per streaming context with a fused Final on the GPU (BRB_MD5UpdateSegmentsBatch and
BrbSha1_UpdateSegmentsBatch), byte for byte against the product's own compat functions (one *_ctx_update per
segment, then *_ctx_final; pinned by test_compat.py) and against hashlib.  Every case is tiny: a few hundred
contexts, segments of at most a few hundred bytes."""
import hashlib
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALGS = ("md5", "sha1")
WIDTH = {"md5": 168, "sha1": 92}
DIG = {"md5": 16, "sha1": 20}
HDR = {"md5": 24, "sha1": 28}                       # state words and counters; the block buffer follows
MODES = ("host", "device", "device_async", "all_devices")
HAVES = (0, 1, 3, 4, 55, 56, 60, 63)
LENS = (0, 1, 2, 3, 4, 5, 59, 60, 61, 63, 64, 65, 127, 128, 129, 200)
FAR = (1 << 62) + 4099                              # host mode: the offset of an empty segment need not be memory


@pytest.fixture(scope="module")
def torch_dev(brb):
    import torch
    assert torch.cuda.is_available(), "no HIP device visible to torch"
    assert brb.gpu_available(), brb.lib().BRB_CryptoGPU_LastError()
    return torch


def have_of(alg, row):
    w = row.view(np.uint32)
    return int(w[4]) & 63 if alg == "md5" else (int(w[5]) >> 3) & 63


def defined(alg, row):
    """The part of a context that an Update defines: state, counters, the buffered bytes."""
    return row[:HDR[alg] + have_of(alg, row)].tobytes()


def compat(brb, alg):
    return getattr(brb, alg + "_ctx_init"), getattr(brb, alg + "_ctx_update"), getattr(brb, alg + "_ctx_final")


def hashed(alg, msg):
    return getattr(hashlib, alg)(msg).digest()


class Run:
    """The batch calls of one algorithm in one mode, on host tables that are updated in place."""

    def __init__(self, brb, torch, alg, mode):
        self.brb, self.torch, self.alg, self.mode = brb, torch, alg, mode
        self.device = mode.startswith("device")

    def _dev(self, a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint64:
            a = a.view(np.int64)
        if a.dtype == np.uint32:
            a = a.view(np.int32)
        return self.torch.from_numpy(a).cuda()

    def _go(self, op, ctxs, *args, idx=None, **kw):
        """kw values that are arrays travel with the positional ones; returns (result, device copies or None)."""
        fn = getattr(self.brb, f"{self.alg}_{op}_batch")
        if not self.device:
            if self.mode == "all_devices":
                with self.brb.TestOption("devices", 2):
                    return fn(ctxs, *args, ctx_index=idx, all_devices=True, **kw), None
            return fn(ctxs, *args, ctx_index=idx, **kw), None
        dc = self._dev(ctxs)
        dargs = [self._dev(a) for a in args]
        dkw = {k: self._dev(v) if isinstance(v, np.ndarray) else v for k, v in kw.items()}
        if self.mode == "device_async":
            self.torch.cuda.synchronize()
            side = self.torch.cuda.Stream()
            res = fn(dc, *dargs, ctx_index=self._dev(idx), stream=side, async_=True, **dkw)
            side.synchronize()
        else:
            res = fn(dc, *dargs, ctx_index=self._dev(idx), **dkw)
        ctxs[...] = dc.cpu().numpy()
        return res, dargs

    def init(self, ctxs, idx=None, n=None):
        self._go("init", ctxs, idx=idx, n=n)

    def update(self, ctxs, seg, idx=None):
        """UpdateBatch with item i taking segment i of a one-segment-per-item layout."""
        n = len(seg[3]) - 1
        assert np.array_equal(seg[3], np.arange(n + 1))
        self._go("update", ctxs, seg[0], seg[1][:n], seg[2][:n], idx=idx)

    def final(self, ctxs, idx=None, n=None):
        res, _ = self._go("final", ctxs, idx=idx, n=n)
        return res.cpu().numpy() if self.device else res

    def segments(self, ctxs, seg, fin=None, idx=None):
        """seg = (data, seg_offsets, seg_lengths, item_first_seg).  Returns (digests over a 0xA5 fill, or None
        without fin; the data buffer as the call left it)."""
        n = len(seg[3]) - 1
        kw = {} if fin is None else {"final": fin, "out": np.full((n, DIG[self.alg]), 0xA5, np.uint8)}
        res, dargs = self._go("update_segments", ctxs, *seg, idx=idx, **kw)
        if fin is None:
            assert res is None
        elif self.device:
            res = res.cpu().numpy()
        return res, seg[0] if dargs is None else dargs[0].cpu().numpy()


def contexts_with(brb, alg, haves, rng, fill=0xA5):
    """Rows holding compat contexts with 64 + have bytes taken (so the state is not the IV), `fill` elsewhere;
    and the bytes each has taken."""
    c_init, c_update, _ = compat(brb, alg)
    rows = np.full((len(haves), WIDTH[alg]), fill, np.uint8)
    msgs = []
    for r, have in enumerate(haves):
        msgs.append(rng.integers(0, 256, 64 + have, dtype=np.uint8).tobytes())
        c_init(rows[r])
        c_update(rows[r], msgs[r][:64])
        c_update(rows[r], msgs[r][64:])
    return rows, msgs


def lay_out(lists, rng, far_empty, aligns=None):
    """(data, seg_offsets, seg_lengths, item_first_seg) for per-item lists of segment lengths: segment k at an
    address with (address & 3) == aligns[k] (default: k & 3; the buffer itself is at least 4-byte aligned on the
    host and on the device).  far_empty: empty segments get offsets far outside the buffer (host mode only);
    otherwise every offset lies inside the allocation."""
    flat = [int(n) for li in lists for n in li]
    offs, pos = [], 4
    for k, n in enumerate(flat):
        pos += ((k if aligns is None else int(aligns[k])) - pos) & 3
        offs.append(FAR + 7 * k if far_empty and n == 0 else pos)
        pos += n + int(rng.integers(0, 3))
    data = rng.integers(0, 256, pos + 8, dtype=np.uint8)
    first = np.concatenate([[0], np.cumsum([len(li) for li in lists])]).astype(np.uint64)
    # one unnamed entry behind the lists, so that the arrays are never empty (an empty tensor has no address)
    return data, np.array(offs + [pos], np.uint64), np.array(flat + [0], np.uint32), first


def fed(seg, i):
    """The bytes item i's segments hold, in order."""
    data, offs, lens, first = seg
    return b"".join(data[int(offs[k]):int(offs[k]) + int(lens[k])].tobytes() if lens[k] else b""
                    for k in range(int(first[i]), int(first[i + 1])))


def reference(brb, alg, ctxs, named, seg, fin):
    """The table and the digests (None: not finalised) the compat functions leave."""
    _, c_update, c_final = compat(brb, alg)
    data, offs, lens, first = seg
    want, digs = ctxs.copy(), []
    for i, r in enumerate(named):
        for k in range(int(first[i]), int(first[i + 1])):
            c_update(want[r], data[int(offs[k]):int(offs[k]) + int(lens[k])].tobytes() if lens[k] else b"")
        digs.append(c_final(want[r]) if fin is not None and fin[i] else None)
    return want, digs


def check(alg, ctxs, before, want, named, seg, digs, got):
    """The contract, row by row."""
    for i, r in enumerate(named):
        if digs[i] is None:
            assert defined(alg, ctxs[r]) == defined(alg, want[r]), (i, r)
            if alg == "md5":
                assert np.array_equal(ctxs[r, 88:], before[r, 88:]), (i, r)   # digest and string are not touched
            if not fed(seg, i):
                assert np.array_equal(ctxs[r], before[r]), (i, r)             # no bytes, no final: untouched
            assert got is None or (got[i] == 0xA5).all(), (i, r)
            continue
        assert got[i].tobytes() == digs[i], (i, r)
        if alg == "sha1":
            assert not ctxs[r].any(), (i, r)
            continue
        assert np.array_equal(ctxs[r, :24], want[r, :24]), (i, r)             # buf: the final state; bytes: advanced
        assert np.array_equal(ctxs[r, 88:137], want[r, 88:137]), (i, r)       # digest, string[0 .. 33)
        assert np.array_equal(ctxs[r, 137:], before[r, 137:]), (i, r)         # string[33 .. 64) untouched
    rest = np.setdiff1d(np.arange(len(ctxs)), np.asarray(named, np.int64))
    assert np.array_equal(ctxs[rest], before[rest])


def _grid_lists():
    """Segment lists of 0 to 5 segments drawn from LENS: none, every single length, empty segments at the
    head, in the middle and at the tail, and a fixed-seed draw of longer lists."""
    rng = np.random.default_rng(20)
    lists = [[]] + [[n] for n in LENS]
    lists += [[0, 5, 64], [5, 0, 64], [5, 64, 0], [0, 0, 0], [0, 61, 0, 3, 0], [0], [63, 1], [1, 63], [3, 61, 64, 1]]
    lists += [[int(x) for x in rng.choice(LENS, int(k))] for k in rng.integers(2, 6, 10)]
    return lists


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("alg", ALGS)
def test_grid(brb, torch_dev, alg, mode):
    """One call, one context per (have, segment list, final): every phase of the seed against every segment
    length class, with every start alignment, finalised and not."""
    rng = np.random.default_rng(21)
    grid = list(itertools.product(HAVES, _grid_lists(), (0, 1)))
    ctxs, prior = contexts_with(brb, alg, [g[0] for g in grid], rng)
    seg = lay_out([g[1] for g in grid], rng, far_empty=mode == "host")
    assert {int(o) & 3 for o, n in zip(seg[1], seg[2]) if n} == {0, 1, 2, 3} and seg[0].ctypes.data % 4 == 0
    assert mode == "host" or int(seg[1].max()) < len(seg[0])
    fin = np.array([g[2] for g in grid], np.uint8)
    named = range(len(grid))
    want, digs = reference(brb, alg, ctxs, named, seg, fin)
    before, data0 = ctxs.copy(), seg[0].copy()
    got, after = Run(brb, torch_dev, alg, mode).segments(ctxs, seg, fin)
    check(alg, ctxs, before, want, named, seg, digs, got)
    for i, g in enumerate(grid):
        if g[2]:
            assert got[i].tobytes() == hashed(alg, prior[i] + fed(seg, i)), g
        else:
            assert have_of(alg, ctxs[i]) == (g[0] + sum(g[1])) & 63, g
    assert np.array_equal(after, data0)             # the call never writes into data


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("index", ["none", "permutation", "sparse"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("alg", ALGS)
def test_shapes(brb, torch_dev, alg, n, index, mode):
    """n items below, at and past a wave and a workgroup; without an index, through a permutation, and naming
    a sparse subset of a larger table whose other contexts keep a sentinel fill; in every mode.  The lists
    hold 0 to 5 segments and final is mixed, both varying lane by lane.  A second call gives every item further
    segments and finalises all (those finalised by the first call are re-initialised in between)."""
    rng = np.random.default_rng(1000 + n)
    n_ctx = n if index != "sparse" else 2 * n + 3
    idx = None if index == "none" else rng.permutation(n_ctx)[:n].astype(np.uint32)
    named = np.arange(n) if idx is None else idx.astype(np.int64)
    ctxs = np.full((n_ctx, WIDTH[alg]), 0x5C, np.uint8)
    run = Run(brb, torch_dev, alg, mode)
    run.init(ctxs, idx, None if idx is not None else n)
    msgs = [b""] * n
    for call in range(2):
        lists = [rng.choice(LENS, int(k)) if rng.integers(0, 4) else rng.integers(0, 200, int(k)) for k in rng.integers(0, 6, n)]
        seg = lay_out(lists, rng, far_empty=not run.device, aligns=rng.integers(0, 4, sum(len(li) for li in lists)))
        fin = rng.integers(0, 2, n).astype(np.uint8) if call == 0 else np.ones(n, np.uint8)
        want, digs = reference(brb, alg, ctxs, named, seg, fin)
        before = ctxs.copy()
        got, _ = run.segments(ctxs, seg, fin, idx)
        check(alg, ctxs, before, want, named, seg, digs, got)
        msgs = [m + fed(seg, i) for i, m in enumerate(msgs)]
        done = np.flatnonzero(fin)
        assert [got[i].tobytes() for i in done] == [hashed(alg, msgs[i]) for i in done]
        if call == 0 and len(done):
            run.init(ctxs, named[done].astype(np.uint32))
            for i in done:
                msgs[i] = b""
    assert (ctxs[np.setdiff1d(np.arange(n_ctx), named)] == 0x5C).all()


@pytest.mark.parametrize("alg", ALGS)
def test_one_segment_without_final_is_update_batch(brb, torch_dev, alg):
    rng = np.random.default_rng(22)
    n = 200
    ctxs, _ = contexts_with(brb, alg, rng.integers(0, 64, n), rng)
    seg = lay_out([[k] for k in rng.integers(0, 200, n)], rng, far_empty=False)
    other = ctxs.copy()
    run = Run(brb, torch_dev, alg, "device")
    run.update(other, seg)
    got, _ = run.segments(ctxs, seg)
    assert got is None
    for r in range(n):
        assert defined(alg, ctxs[r]) == defined(alg, other[r]), r
    assert np.array_equal(ctxs[:, HDR[alg] + 64:], other[:, HDR[alg] + 64:])


@pytest.mark.parametrize("alg", ALGS)
def test_no_segments_and_final_is_final_batch(brb, torch_dev, alg):
    rng = np.random.default_rng(23)
    n = 200
    ctxs, msgs = contexts_with(brb, alg, rng.integers(0, 64, n), rng)
    other = ctxs.copy()
    run = Run(brb, torch_dev, alg, "device")
    want = run.final(other)
    seg = (np.zeros(8, np.uint8), np.zeros(1, np.uint64), np.zeros(1, np.uint32), np.zeros(n + 1, np.uint64))
    got, _ = run.segments(ctxs, seg, np.ones(n, np.uint8))
    assert np.array_equal(got, want)
    assert [got[r].tobytes() for r in range(n)] == [hashed(alg, m) for m in msgs]
    if alg == "sha1":
        assert not ctxs.any() and not other.any()
    else:
        assert np.array_equal(ctxs[:, :24], other[:, :24]) and np.array_equal(ctxs[:, 88:], other[:, 88:])


@pytest.mark.parametrize("alg", ALGS)
def test_init_segments_final_is_the_whole_record_digest(brb, torch_dev, alg):
    rng = np.random.default_rng(24)
    n = 200
    lists = [rng.choice(LENS, int(k)) for k in rng.integers(0, 6, n)]
    seg = lay_out(lists, rng, far_empty=False, aligns=rng.integers(0, 4, sum(len(li) for li in lists)))
    ctxs = np.full((n, WIDTH[alg]), 0xA5, np.uint8)
    run = Run(brb, torch_dev, alg, "device")
    run.init(ctxs)
    got, _ = run.segments(ctxs, seg, np.ones(n, np.uint8))
    assert [got[i].tobytes() for i in range(n)] == [hashed(alg, fed(seg, i)) for i in range(n)]
    if alg == "md5":
        assert np.array_equal(got, brb.md5_batch_segments(*seg))


@pytest.mark.parametrize("alg", ALGS)
def test_counters_cross_2_32(brb, torch_dev, alg):
    """Hand-set counters 256 - have bytes below 2^32 (MD5 bytes = {0xFFFFFF00 + have, 7}; SHA-1 count =
    {0xFFFFF800 | have << 3, 7}) take three small segments that stay below 2^32 or cross it in the first, the
    second or the third: the carry lands where the compat calls put it, and the padding of the finalised half
    carries the same count."""
    rng = np.random.default_rng(25)
    triples = ((60, 60, 60), (256, 1, 1), (100, 200, 10), (10, 10, 250), (0, 192, 1))
    cases = list(itertools.product(HAVES, triples, (0, 1)))
    ctxs, _ = contexts_with(brb, alg, [c[0] for c in cases], rng)
    words = ctxs.view(np.uint32)
    for r, (have, _, _) in enumerate(cases):
        if alg == "md5":
            words[r, 4], words[r, 5] = 0xFFFFFF00 + have, 7
        else:
            words[r, 5], words[r, 6] = 0xFFFFF800 | (have << 3), 7
    seg = lay_out([c[1] for c in cases], rng, far_empty=False)
    fin = np.array([c[2] for c in cases], np.uint8)
    named = range(len(cases))
    want, digs = reference(brb, alg, ctxs, named, seg, fin)
    before = ctxs.copy()
    got, _ = Run(brb, torch_dev, alg, "device").segments(ctxs, seg, fin)
    check(alg, ctxs, before, want, named, seg, digs, got)
    hi = want.view(np.uint32)[fin == 0, 5 if alg == "md5" else 6]
    assert set(hi.tolist()) == {7, 8}               # both sides of the carry occur
    if alg == "md5":                                # a finalised MD5 context keeps the advanced count
        assert set(ctxs.view(np.uint32)[fin == 1, 5].tolist()) == {7, 8}


@pytest.mark.parametrize("alg", ALGS)
def test_chains(brb, torch_dev, alg):
    """300 contexts over 6 rounds.  Each round a random subset advances: a third by the host compat Update, a
    third by UpdateBatch, a third by the new call with 1 to 4 segments, of which a random third is finalised in
    its round and re-initialised with InitBatch.  Every finished digest equals hashlib of the bytes fed."""
    rng = np.random.default_rng(26)
    n = 300
    ctxs = np.full((n, WIDTH[alg]), 0xA5, np.uint8)
    run = Run(brb, torch_dev, alg, "device")
    run.init(ctxs)
    msgs = [b""] * n
    finished = 0
    c_update = compat(brb, alg)[1]
    for _ in range(6):
        picked = np.flatnonzero(rng.integers(0, 4, n))          # about three quarters
        how = rng.integers(0, 3, len(picked))
        for r in picked[how == 0]:
            piece = rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8).tobytes()
            c_update(ctxs[r], piece)
            msgs[r] += piece
        ub = picked[how == 1]
        if len(ub):
            seg = lay_out([[k] for k in rng.integers(0, 300, len(ub))], rng, far_empty=False)
            run.update(ctxs, seg, ub.astype(np.uint32))
            for i, r in enumerate(ub):
                msgs[r] += fed(seg, i)
        us = picked[how == 2]
        if len(us):
            lists = [rng.integers(0, 300, int(k)) for k in rng.integers(1, 5, len(us))]
            seg = lay_out(lists, rng, far_empty=False, aligns=rng.integers(0, 4, sum(len(li) for li in lists)))
            fin = (rng.integers(0, 3, len(us)) == 0).astype(np.uint8)
            got, _ = run.segments(ctxs, seg, fin, us.astype(np.uint32))
            for i, r in enumerate(us):
                msgs[r] += fed(seg, i)
                if fin[i]:
                    assert got[i].tobytes() == hashed(alg, msgs[r]), r
                    msgs[r] = b""
                    finished += 1
                else:
                    assert (got[i] == 0xA5).all()
            if fin.any():
                run.init(ctxs, us[fin == 1].astype(np.uint32))
    assert finished > 50
    seg = (np.zeros(8, np.uint8), np.zeros(1, np.uint64), np.zeros(1, np.uint32), np.zeros(n + 1, np.uint64))
    got, _ = run.segments(ctxs, seg, np.ones(n, np.uint8))
    assert [got[r].tobytes() for r in range(n)] == [hashed(alg, m) for m in msgs]
