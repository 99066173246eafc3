"""Segment lists per streaming context with a fused Final (BRB_MD5UpdateSegmentsBatch and
BrbSha1_UpdateSegmentsBatch): the exports and every host-mode refusal, which all come before any device
work.  No test here needs a GPU; where one is present the valid call is checked against the compat
functions instead of against the refusal."""
import numpy as np
import pytest

ALGS = {"md5": ("BRB_MD5UpdateSegmentsBatch", 168, 16, 24), "sha1": ("BrbSha1_UpdateSegmentsBatch", 92, 20, 28)}
SYMBOLS = {name for name, *_ in ALGS.values()}
N, N_CTX = 4, 6
FAR = (1 << 63) + 12345                             # the offset of an empty segment need not be memory


class Call:
    """One raw call: the arrays a call takes, any of them replaceable by None."""

    def __init__(self, brb, alg):
        name, self.width, self.dig, self.hdr = ALGS[alg]
        self.brb, self.alg = brb, alg
        self.fn = getattr(brb.lib(), name)
        self.ctxs = np.full((N_CTX, self.width), 0xA5, np.uint8)
        self.idx = np.array([5, 0, 3, 2], np.uint32)
        self.data = np.arange(256, dtype=np.uint8)
        # item 0: two segments; item 1: none; item 2: one; item 3: an empty one between two with bytes
        self.soff = np.array([1, 70, 2, 130, FAR, 7], np.uint64)
        self.slen = np.array([65, 3, 9, 100, 0, 64], np.uint32)
        self.first = np.array([0, 2, 2, 3, 6], np.uint64)
        self.fin = np.array([1, 0, 0, 1], np.uint8)
        self.digests = np.full((N, self.dig), 0xA5, np.uint8)
        self.n, self.n_ctx = N, N_CTX

    def __call__(self, flags=0):
        p = lambda a: None if a is None else a.ctypes.data
        return self.fn(p(self.ctxs), self.n_ctx, p(self.idx), p(self.data), p(self.soff), p(self.slen), p(self.first),
                       self.n, p(self.fin), p(self.digests), flags, None)

    def refused(self, reason, flags=0):
        keep = self.ctxs
        rc = self(flags)
        err = self.brb.lib().BRB_CryptoGPU_LastError()
        assert rc == -1 and reason in err, (self.alg, rc, err)
        if keep is not None:
            assert (keep == 0xA5).all()
        assert (self.digests is None) or (self.digests == 0xA5).all()


def _calls(brb):
    return [Call(brb, alg) for alg in ALGS]


def test_symbols_exported(brb):
    assert SYMBOLS <= brb.exported_symbols()


def test_null_required_pointer_is_refused(brb):
    for alg in ALGS:
        c = Call(brb, alg)
        keep = c.ctxs
        c.ctxs = None
        c.refused(b"NULL")
        assert (keep == 0xA5).all()
        for field in ("soff", "slen", "first"):
            c = Call(brb, alg)
            setattr(c, field, None)
            c.refused(b"NULL")
        c = Call(brb, alg)                          # data may be NULL only when every named segment is empty
        c.data = None
        c.refused(b"NULL data")
    c = Call(brb, "sha1")                           # SHA-1's digests are required whenever final is not NULL
    c.digests = None
    c.refused(b"NULL")


def test_index_out_of_range_is_refused(brb):
    for c in _calls(brb):
        c.idx[2] = N_CTX
        c.refused(b"out of range")
        c.refused(b"out of range", brb.BATCH_ALL_DEVICES)


def test_no_index_and_more_items_than_contexts_is_refused(brb):
    for c in _calls(brb):
        c.idx = None
        c.n_ctx = N - 1
        c.refused(b"n_ctx")


def test_duplicate_index_is_refused(brb):
    for c in _calls(brb):
        c.idx[3] = c.idx[0]
        c.refused(b"named twice")
        c.refused(b"named twice", brb.BATCH_ALL_DEVICES)


def test_decreasing_first_seg_is_refused(brb):
    for c in _calls(brb):
        c.first[2] = 1
        c.refused(b"non-decreasing")


def test_wrapping_segment_is_refused(brb):
    for c in _calls(brb):
        c.soff[3] = (1 << 64) - 10
        c.refused(b"wraps")


def test_oversized_item_count_is_refused(brb):
    for c in _calls(brb):
        c.n = 1 << 33
        c.refused(b"split the batch")
        c.refused(b"split the batch", brb.BATCH_DEVICE)


def test_all_devices_needs_host_pointers(brb):
    for c in _calls(brb):
        c.refused(b"ALL_DEVICES", brb.BATCH_DEVICE | brb.BATCH_ALL_DEVICES)


def test_empty_batch_is_done(brb):
    for c in _calls(brb):
        c.ctxs = c.idx = c.data = c.soff = c.slen = c.first = c.fin = c.digests = None
        c.n = 0
        assert c(brb.BATCH_HOST) == 1
        assert c(brb.BATCH_DEVICE | brb.BATCH_ASYNC) == 1


def _compat_rows(brb, alg, width, rng):
    """A table whose rows are compat contexts with 64 + 11 r bytes taken (0xA5 elsewhere)."""
    init, update = getattr(brb, alg + "_ctx_init"), getattr(brb, alg + "_ctx_update")
    rows = np.full((N_CTX, width), 0xA5, np.uint8)
    for r in range(N_CTX):
        init(rows[r])
        update(rows[r], rng.integers(0, 256, 64 + 11 * r, dtype=np.uint8).tobytes())
    return rows


def _have(alg, row):
    w = row.view(np.uint32)
    return int(w[4]) & 63 if alg == "md5" else (int(w[5]) >> 3) & 63


@pytest.mark.parametrize("alg", list(ALGS))
def test_without_device_refuses_with_a_reason(brb, alg):
    """No CPU fallback: without a usable device the call returns 0 and says why, and writes nothing.  With
    a device the same call must leave what the compat functions leave."""
    L = brb.lib()
    have_gpu = brb.gpu_available()
    _, width, dig, hdr = ALGS[alg]
    update, final = getattr(brb, alg + "_ctx_update"), getattr(brb, alg + "_ctx_final")
    c = Call(brb, alg)
    c.ctxs = _compat_rows(brb, alg, width, np.random.default_rng(5))
    before = c.ctxs.copy()
    data0 = c.data.copy()
    for flags in (brb.BATCH_HOST, brb.BATCH_ALL_DEVICES):
        c.ctxs[:] = before
        c.digests[:] = 0xA5
        rc = c(flags)
        if not have_gpu:
            assert rc == 0 and L.BRB_CryptoGPU_LastError()
            assert np.array_equal(c.ctxs, before) and (c.digests == 0xA5).all()
            continue
        assert rc == 1, L.BRB_CryptoGPU_LastError()
        want = before.copy()
        named = [int(i) for i in c.idx]
        for k, r in enumerate(named):
            for s in range(int(c.first[k]), int(c.first[k + 1])):
                o, n = int(c.soff[s]), int(c.slen[s])
                update(want[r], c.data[o:o + n].tobytes() if n else b"")
            if not c.fin[k]:
                have = _have(alg, want[r])
                assert np.array_equal(c.ctxs[r, :hdr + have], want[r, :hdr + have])
                assert (c.digests[k] == 0xA5).all()
                continue
            d = final(want[r])
            assert c.digests[k].tobytes() == d
            if alg == "md5":
                assert np.array_equal(c.ctxs[r, :24], want[r, :24]) and np.array_equal(c.ctxs[r, 88:], want[r, 88:])
            else:
                assert not c.ctxs[r].any()
        assert np.array_equal(c.ctxs[named[1]], before[named[1]])    # no segments, no final: untouched
        rest = [r for r in range(N_CTX) if r not in named]
        assert np.array_equal(c.ctxs[rest], before[rest])
        assert np.array_equal(c.data, data0)
