"""Streaming MD5 / SHA-1 contexts as a batch on the GPU (BRB_MD5InitBatch / UpdateBatch / FinalBatch and the
BrbSha1_ three), byte for byte against the product's own compat functions (pinned by test_compat.py) and
against hashlib.  Every case is tiny: a few hundred contexts, pieces of at most a few hundred bytes; one
call per algorithm and mode (test_update_long_pieces) takes pieces of 64 KiB and 1 MiB."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALGS = ("md5", "sha1")
WIDTH = {"md5": 168, "sha1": 92}
DIG = {"md5": 16, "sha1": 20}
HDR = {"md5": 24, "sha1": 28}                       # state words and counters; the block buffer follows
MODES = ("host", "device", "device_async", "all_devices")
HAVES = (0, 1, 3, 4, 55, 56, 60, 63)


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
    """The part of a context that Update defines: state, counters, the buffered bytes."""
    return row[:HDR[alg] + have_of(alg, row)].tobytes()


class Run:
    """The three batch calls of one algorithm in one mode, on host tables that are updated in place."""

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
        fn = getattr(self.brb, f"{self.alg}_{op}_batch")
        if not self.device:
            if self.mode == "all_devices":
                with self.brb.TestOption("devices", 2):
                    return fn(ctxs, *args, ctx_index=idx, all_devices=True, **kw), None
            return fn(ctxs, *args, ctx_index=idx, **kw), None
        dc = self._dev(ctxs)
        dargs = [self._dev(a) for a in args]
        if self.mode == "device_async":
            self.torch.cuda.synchronize()
            side = self.torch.cuda.Stream()
            res = fn(dc, *dargs, ctx_index=self._dev(idx), stream=side, async_=True, **kw)
            side.synchronize()
        else:
            res = fn(dc, *dargs, ctx_index=self._dev(idx), **kw)
        ctxs[...] = dc.cpu().numpy()
        return res, dargs

    def init(self, ctxs, idx=None, n=None):
        self._go("init", ctxs, idx=idx, n=n)

    def update(self, ctxs, data, offs, lens, idx=None):
        """Returns the piece buffer as the call left it."""
        _, dargs = self._go("update", ctxs, data, offs, lens, idx=idx)
        return data if dargs is None else dargs[0].cpu().numpy()

    def final(self, ctxs, idx=None, n=None):
        res, _ = self._go("final", ctxs, idx=idx, n=n)
        return res.cpu().numpy() if self.device else res


def compat(brb, alg):
    return getattr(brb, alg + "_ctx_init"), getattr(brb, alg + "_ctx_update"), getattr(brb, alg + "_ctx_final")


def hashed(alg, msg):
    return getattr(hashlib, alg)(msg).digest()


def contexts_with(brb, alg, haves, rng, fill=0xA5):
    """Rows holding compat contexts with 64 + have bytes taken (so the state is not the IV), `fill` elsewhere."""
    c_init, c_update, _ = compat(brb, alg)
    rows = np.full((len(haves), WIDTH[alg]), fill, np.uint8)
    for r, have in enumerate(haves):
        c_init(rows[r])
        c_update(rows[r], rng.integers(0, 256, 64, dtype=np.uint8).tobytes())
        c_update(rows[r], rng.integers(0, 256, have, dtype=np.uint8).tobytes())
    return rows


def lay_out(lens, aligns, rng):
    """One buffer holding a piece per entry, piece i at an address with (address & 3) == aligns[i] (the
    buffer itself is at least 4-byte aligned on the host and on the device)."""
    offs, pos = [], 4
    for n, al in zip(lens, aligns):
        pos += (al - pos) & 3
        offs.append(pos)
        pos += int(n) + int(rng.integers(0, 3))
    data = rng.integers(0, 256, pos + 8, dtype=np.uint8)
    return data, np.array(offs, np.uint64), np.array(lens, np.uint32)


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("alg", ALGS)
def test_update_grid(brb, torch_dev, alg, mode):
    """One call, one context per (have, len, piece address & 3): every phase of the head block, pieces that
    stay inside the buffer, fill it exactly, and run one byte, a block and a block and a byte past it."""
    rng = np.random.default_rng(11)
    grid = []
    for have in HAVES:
        room = 64 - have
        for n in (0, 1, room - 1, room, room + 1, room + 63, room + 64, room + 65, 200):
            for al in range(4):
                grid.append((have, n, al))
    ctxs = contexts_with(brb, alg, [g[0] for g in grid], rng)
    data, offs, lens = lay_out([g[1] for g in grid], [g[2] for g in grid], rng)
    assert {int(o) & 3 for o in offs} == {0, 1, 2, 3} and data.ctypes.data % 4 == 0
    want = ctxs.copy()
    c_update = compat(brb, alg)[1]
    for r in range(len(grid)):
        c_update(want[r], data[int(offs[r]):int(offs[r]) + int(lens[r])].tobytes())
    before = data.copy()
    after = Run(brb, torch_dev, alg, mode).update(ctxs, data, offs, lens)
    for r, g in enumerate(grid):
        assert have_of(alg, ctxs[r]) == (g[0] + g[1]) & 63, g
        assert defined(alg, ctxs[r]) == defined(alg, want[r]), g
    if alg == "md5":
        assert (ctxs[:, 88:] == 0xA5).all()         # digest and string are not touched
    assert np.array_equal(after, before)            # the batch call never writes into data


LONG_HAVES = (0, 1, 3, 60, 63)
LONG_PIECES = (65535, 65536, 65537, (1 << 20) + 3)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("alg", ALGS)
def test_update_long_pieces(brb, torch_dev, alg, mode):
    """One Update call whose pieces are far longer than a block: 64 KiB - 1, 64 KiB, 64 KiB + 1 and
    1 MiB + 3 bytes, each onto contexts with 0, 1, 3, 60 and 63 bytes buffered, the piece addresses at
    every residue mod 4.  The contexts equal the compat Update's byte for byte, and after Final the
    digests equal hashlib's of the whole message."""
    rng = np.random.default_rng(17)
    cases = [(have, n) for n in LONG_PIECES for have in LONG_HAVES]
    c_init, c_update, _ = compat(brb, alg)
    heads = [rng.integers(0, 256, 64 + have, dtype=np.uint8).tobytes() for have, _ in cases]
    ctxs = np.full((len(cases), WIDTH[alg]), 0xA5, np.uint8)
    for r, head in enumerate(heads):
        c_init(ctxs[r])
        c_update(ctxs[r], head)
    data, offs, lens = lay_out([n for _, n in cases], [r & 3 for r in range(len(cases))], rng)
    assert {int(o) & 3 for o in offs} == {0, 1, 2, 3}
    pieces = [data[int(o):int(o) + int(k)].tobytes() for o, k in zip(offs, lens)]
    want = ctxs.copy()
    for r, piece in enumerate(pieces):
        c_update(want[r], piece)
    before = data.copy()
    run = Run(brb, torch_dev, alg, mode)
    after = run.update(ctxs, data, offs, lens)
    assert np.array_equal(after, before)            # the batch call never writes into data
    for r, c in enumerate(cases):
        assert have_of(alg, ctxs[r]) == (c[0] + c[1]) & 63, c
        assert defined(alg, ctxs[r]) == defined(alg, want[r]), c
    got = run.final(ctxs)
    assert [got[r].tobytes() for r in range(len(cases))] == [hashed(alg, h + p) for h, p in zip(heads, pieces)]


@pytest.mark.parametrize("alg", ALGS)
def test_counters_cross_2_32(brb, torch_dev, alg):
    """Hand-set counters just below 2^32 (MD5 bytes = {0xFFFFFFC0 + have, 7}; SHA-1 count = {0xFFFFFE00 |
    have << 3, 7}), advanced by pieces that stay below, land on and cross 2^32: the carries equal compat's.
    The spurious SHA-1 carry for a single piece of 2^29 bytes or more is not run on the GPU -- a lone lane
    would need about 10 s for such a piece.  It is covered by reading the kernel's expression (Sha1Stream::
    advance in digest_stream_kernels.hip: the 32-bit sum compared against the untruncated uint64 len << 3,
    then len >> 29 added) against sha1.c:151-153."""
    rng = np.random.default_rng(12)
    cases = [(have, n) for have in HAVES for n in (64 - have - 1, 64 - have, 64 - have + 1, 200)]
    ctxs = contexts_with(brb, alg, [c[0] for c in cases], rng)
    words = ctxs.view(np.uint32)
    for r, (have, _) in enumerate(cases):
        if alg == "md5":
            words[r, 4], words[r, 5] = 0xFFFFFFC0 + have, 7
        else:
            words[r, 5], words[r, 6] = 0xFFFFFE00 | (have << 3), 7
    data, offs, lens = lay_out([c[1] for c in cases], [r & 3 for r in range(len(cases))], rng)
    want = ctxs.copy()
    for r in range(len(cases)):
        compat(brb, alg)[1](want[r], data[int(offs[r]):int(offs[r]) + int(lens[r])].tobytes())
    Run(brb, torch_dev, alg, "device").update(ctxs, data, offs, lens)
    hi = ctxs.view(np.uint32)[:, 5 if alg == "md5" else 6]
    assert set(hi.tolist()) == {7, 8}               # both sides of the carry occur
    for r, c in enumerate(cases):
        assert defined(alg, ctxs[r]) == defined(alg, want[r]), c


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("index", ["none", "permutation", "sparse"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("alg", ALGS)
def test_shapes(brb, torch_dev, alg, n, index, mode):
    """Init, two Updates and Final of n items: below, at and past a wave and a workgroup; without an
    index, through a permutation, and naming a sparse subset of a larger table whose other contexts keep a
    sentinel fill; in host mode, device mode, device-async on a side stream and split over two parts."""
    rng = np.random.default_rng(n)
    n_ctx = n if index != "sparse" else 2 * n + 3
    idx = None if index == "none" else rng.permutation(n_ctx)[:n].astype(np.uint32)
    named = np.arange(n) if idx is None else idx.astype(np.int64)
    ctxs = np.full((n_ctx, WIDTH[alg]), 0x5C, np.uint8)
    run = Run(brb, torch_dev, alg, mode)
    run.init(ctxs, idx, None if idx is not None else n)
    msgs = [b""] * n
    for _ in range(2):
        lens = rng.integers(0, 200, n)
        data, offs, lens = lay_out(lens, rng.integers(0, 4, n), rng)
        run.update(ctxs, data, offs, lens, idx)
        msgs = [m + data[int(o):int(o) + int(k)].tobytes() for m, o, k in zip(msgs, offs, lens)]
    got = run.final(ctxs, idx, None if idx is not None else n)
    assert [got[i].tobytes() for i in range(n)] == [hashed(alg, m) for m in msgs]
    rest = np.setdiff1d(np.arange(n_ctx), named)
    assert (ctxs[rest] == 0x5C).all()
    if alg == "md5":
        assert [ctxs[r, 104:136].tobytes().decode() for r in named] == [hashlib.md5(m).hexdigest() for m in msgs]
    else:
        assert not ctxs[named].any()


def _chains(rng, n=300, rounds=6):
    """n messages of U[0, 700] bytes, each cut at random points into `rounds` pieces (empty ones allowed)."""
    msgs = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(0, 701, n)]
    cuts = [np.sort(rng.integers(0, len(m) + 1, rounds - 1)) for m in msgs]
    pieces = [[m[a:b] for a, b in zip([0, *c], [*c, len(m)])] for m, c in zip(msgs, cuts)]
    return msgs, pieces


@pytest.mark.parametrize("alg", ALGS)
def test_chains_on_the_device(brb, torch_dev, alg):
    """300 chains over 6 calls, the table resident in HBM throughout: InitBatch, six UpdateBatch rounds,
    FinalBatch.  The digests equal hashlib's and the whole-record batch call's."""
    torch = torch_dev
    rng = np.random.default_rng(13)
    msgs, pieces = _chains(rng)
    n = len(msgs)
    ctxs = torch.full((n, WIDTH[alg]), 0xA5, dtype=torch.uint8, device="cuda")
    getattr(brb, alg + "_init_batch")(ctxs)
    for k in range(6):
        lens = [len(p[k]) for p in pieces]
        data, offs, lens = lay_out(lens, rng.integers(0, 4, n), rng)
        for i, o in enumerate(offs):
            data[int(o):int(o) + int(lens[i])] = np.frombuffer(pieces[i][k], np.uint8)
        getattr(brb, alg + "_update_batch")(ctxs, torch.from_numpy(data).cuda(), torch.from_numpy(offs.view(np.int64)).cuda(),
                                            torch.from_numpy(lens.view(np.int32)).cuda())
    got = getattr(brb, alg + "_final_batch")(ctxs).cpu().numpy()
    want = [hashed(alg, m) for m in msgs]
    assert [got[i].tobytes() for i in range(n)] == want
    blob = np.frombuffer(b"".join(msgs) + b"\0", np.uint8).copy()
    wl = np.array([len(m) for m in msgs], np.uint32)
    wo = np.concatenate([[0], np.cumsum(wl[:-1], dtype=np.uint64)]).astype(np.uint64)
    whole = getattr(brb, alg + "_batch")(blob, wo, wl)
    assert [whole[i].tobytes() for i in range(n)] == want


@pytest.mark.parametrize("alg", ALGS)
def test_chains_alternate_with_host_updates(brb, torch_dev, alg):
    """The same chains with the rounds alternating between the batch call and a host compat Update on the
    downloaded contexts: a context moves freely between the two."""
    rng = np.random.default_rng(14)
    msgs, pieces = _chains(rng)
    n = len(msgs)
    ctxs = np.full((n, WIDTH[alg]), 0xA5, np.uint8)
    run = Run(brb, torch_dev, alg, "device")
    run.init(ctxs)
    c_update = compat(brb, alg)[1]
    for k in range(6):
        if k & 1:
            for i in range(n):
                c_update(ctxs[i], pieces[i][k])
            continue
        lens = [len(p[k]) for p in pieces]
        data, offs, lens = lay_out(lens, rng.integers(0, 4, n), rng)
        for i, o in enumerate(offs):
            data[int(o):int(o) + int(lens[i])] = np.frombuffer(pieces[i][k], np.uint8)
        run.update(ctxs, data, offs, lens)
    got = run.final(ctxs)
    assert [got[i].tobytes() for i in range(n)] == [hashed(alg, m) for m in msgs]


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("alg", ALGS)
def test_final(brb, torch_dev, alg, mode):
    """Final with 0, 1, 55, 56 and 63 bytes buffered (one and two padding blocks) against the compat Final."""
    rng = np.random.default_rng(15)
    haves = (0, 1, 55, 56, 63)
    ctxs = contexts_with(brb, alg, haves, rng)
    want = ctxs.copy()
    digs = [compat(brb, alg)[2](want[r]) for r in range(len(haves))]
    before = ctxs.copy()
    got = Run(brb, torch_dev, alg, mode).final(ctxs)
    assert [got[r].tobytes() for r in range(len(haves))] == digs
    if alg == "sha1":
        assert not ctxs.any()                       # the whole context is zeroed
        return
    assert np.array_equal(ctxs[:, :16], want[:, :16])           # buf: the final state
    assert np.array_equal(ctxs[:, 16:24], before[:, 16:24])     # bytes: untouched
    assert np.array_equal(ctxs[:, 88:137], want[:, 88:137])     # digest, string[0 .. 33)
    assert (ctxs[:, 137:] == 0xA5).all()                        # string[33 .. 64) keeps its fill


def test_md5_final_without_digests(brb, torch_dev):
    """MD5's digests may be NULL: the contexts still get buf, digest and string."""
    rng = np.random.default_rng(16)
    ctxs = contexts_with(brb, "md5", (0, 9, 60), rng)
    want = ctxs.copy()
    for r in range(3):
        brb.md5_ctx_final(want[r])
    assert brb.lib().BRB_MD5FinalBatch(ctxs.ctypes.data, 3, None, 3, None, brb.BATCH_HOST, None) == 1
    assert np.array_equal(ctxs[:, :16], want[:, :16]) and np.array_equal(ctxs[:, 88:137], want[:, 88:137])
    d = torch_dev.from_numpy(contexts_with(brb, "md5", (5,), rng)).cuda()
    assert brb.lib().BRB_MD5FinalBatch(d.data_ptr(), 1, None, 1, None, brb.BATCH_DEVICE, None) == 1


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("alg", ALGS)
def test_init_writes_state_and_counters_only(brb, torch_dev, alg, mode):
    ctxs = np.full((70, WIDTH[alg]), 0xA5, np.uint8)
    want = ctxs.copy()
    for r in range(70):
        compat(brb, alg)[0](want[r])
    Run(brb, torch_dev, alg, mode).init(ctxs)
    assert np.array_equal(ctxs, want) and (ctxs[:, HDR[alg]:] == 0xA5).all()
