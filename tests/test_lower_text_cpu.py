"""BRB_MD5LowerTextBatch and BRB_MD5UpdateSegmentsLowerBatch: the exports and every host-mode refusal, which
all come before any device work.  No test here needs a GPU; where one is present the valid call is checked
against the compat functions (md5_ctx_update / md5_ctx_update_lower / md5_ctx_final, pinned against hashlib by
test_compat.py) instead of against the refusal."""
import hashlib

import numpy as np

SYMBOLS = {"BRB_MD5LowerTextBatch", "BRB_MD5UpdateSegmentsLowerBatch"}
N, N_CTX = 4, 6
FAR = (1 << 63) + 12345                             # the offset of an empty key or segment need not be memory


def lowered(key):
    return bytes(b + 32 if 65 <= b <= 90 else b for b in key)


def test_symbols_exported(brb):
    assert SYMBOLS <= brb.exported_symbols()


# ---- BRB_MD5LowerTextBatch ------------------------------------------------------------------------
class Keys:
    """One raw BRB_MD5LowerTextBatch call: the arrays it takes, any of them replaceable by None."""

    def __init__(self, brb):
        self.brb = brb
        self.fn = brb.lib().BRB_MD5LowerTextBatch
        self.data = np.arange(256, dtype=np.uint8)
        self.offs = np.array([0x3F, FAR, 2, 130], np.uint64)      # 'A'..'Z' and its neighbours; an empty key
        self.lens = np.array([40, 0, 9, 100], np.uint32)
        self.digests = np.full((N, 16), 0xA5, np.uint8)
        self.strings = np.full((N, 33), 0xA5, np.uint8)
        self.n = N

    def __call__(self, flags=0):
        p = lambda a: None if a is None else a.ctypes.data
        return self.fn(p(self.data), p(self.offs), p(self.lens), self.n, p(self.digests), p(self.strings), flags, None)

    def refused(self, reason, flags=0):
        keep = (self.digests, self.strings)
        rc = self(flags)
        err = self.brb.lib().BRB_CryptoGPU_LastError()
        assert rc == -1 and reason in err, (rc, err)
        for out in keep:
            assert out is None or (out == 0xA5).all()


def test_keys_null_lists_are_refused(brb):
    for field in ("offs", "lens"):
        c = Keys(brb)
        setattr(c, field, None)
        c.refused(b"NULL")


def test_keys_both_outputs_null_is_refused(brb):
    c = Keys(brb)
    c.digests = c.strings = None
    c.refused(b"NULL digests and strings")


def test_keys_null_data_with_a_key_that_has_bytes_is_refused(brb):
    c = Keys(brb)
    c.data = None
    c.refused(b"NULL data")


def test_keys_wrapping_range_is_refused(brb):
    c = Keys(brb)
    c.offs[2] = (1 << 64) - 5
    c.refused(b"wraps")
    c.refused(b"wraps", brb.BATCH_ALL_DEVICES)


def test_keys_oversized_count_is_refused(brb):
    c = Keys(brb)
    c.n = 1 << 32
    c.refused(b"split the batch")
    c.refused(b"split the batch", brb.BATCH_DEVICE)


def test_keys_all_devices_needs_host_pointers(brb):
    Keys(brb).refused(b"ALL_DEVICES", brb.BATCH_DEVICE | brb.BATCH_ALL_DEVICES)


def test_keys_empty_batch_is_done(brb):
    c = Keys(brb)
    c.data = c.offs = c.lens = c.digests = c.strings = None
    c.n = 0
    assert c(brb.BATCH_HOST) == 1
    assert c(brb.BATCH_DEVICE | brb.BATCH_ASYNC) == 1


def test_keys_without_device_refuses_with_a_reason(brb):
    """No CPU fallback: without a usable device the call returns 0 and says why, and writes nothing.  With a
    device the same call gives what the compat functions give."""
    L = brb.lib()
    c = Keys(brb)
    data0 = c.data.copy()
    for flags in (brb.BATCH_HOST, brb.BATCH_ALL_DEVICES):
        c.digests[:] = 0xA5
        c.strings[:] = 0xA5
        rc = c(flags)
        if not brb.gpu_available():
            assert rc == 0 and L.BRB_CryptoGPU_LastError()
            assert (c.digests == 0xA5).all() and (c.strings == 0xA5).all()
            continue
        assert rc == 1, L.BRB_CryptoGPU_LastError()
        for i in range(N):
            key = c.data[int(c.offs[i]):int(c.offs[i]) + int(c.lens[i])].tobytes() if c.lens[i] else b""
            row = np.zeros(168, np.uint8)
            brb.md5_ctx_init(row)
            brb.md5_ctx_update_lower(row, key)
            d = brb.md5_ctx_final(row)
            assert d == hashlib.md5(lowered(key)).digest()
            assert c.digests[i].tobytes() == d
            assert c.strings[i].tobytes() == row[104:137].tobytes() == d.hex().encode() + b"\0"
        assert np.array_equal(c.data, data0)


# ---- BRB_MD5UpdateSegmentsLowerBatch: every refusal of BRB_MD5UpdateSegmentsBatch ---------------------
class Call:
    """One raw call: the arrays a call takes, any of them replaceable by None."""

    width, dig, hdr = 168, 16, 24

    def __init__(self, brb, with_lower=True):
        self.brb = brb
        self.fn = brb.lib().BRB_MD5UpdateSegmentsLowerBatch
        self.ctxs = np.full((N_CTX, self.width), 0xA5, np.uint8)
        self.idx = np.array([5, 0, 3, 2], np.uint32)
        self.data = np.arange(256, dtype=np.uint8)
        # item 0: two segments; item 1: none; item 2: one; item 3: an empty one between two with bytes
        self.soff = np.array([1, 70, 2, 130, FAR, 7], np.uint64)
        self.slen = np.array([65, 3, 9, 100, 0, 64], np.uint32)
        self.low = np.array([0, 1, 1, 0, 1, 1], np.uint8) if with_lower else None
        self.first = np.array([0, 2, 2, 3, 6], np.uint64)
        self.fin = np.array([1, 0, 0, 1], np.uint8)
        self.digests = np.full((N, self.dig), 0xA5, np.uint8)
        self.n, self.n_ctx = N, N_CTX

    def __call__(self, flags=0):
        p = lambda a: None if a is None else a.ctypes.data
        return self.fn(p(self.ctxs), self.n_ctx, p(self.idx), p(self.data), p(self.soff), p(self.slen), p(self.low),
                       p(self.first), self.n, p(self.fin), p(self.digests), flags, None)

    def refused(self, reason, flags=0):
        keep = self.ctxs
        rc = self(flags)
        err = self.brb.lib().BRB_CryptoGPU_LastError()
        assert rc == -1 and reason in err, (rc, err)
        if keep is not None:
            assert (keep == 0xA5).all()
        assert (self.digests is None) or (self.digests == 0xA5).all()


def _calls(brb):
    return [Call(brb, True), Call(brb, False)]


def test_null_required_pointer_is_refused(brb):
    for with_lower in (True, False):
        c = Call(brb, with_lower)
        keep = c.ctxs
        c.ctxs = None
        c.refused(b"NULL")
        assert (keep == 0xA5).all()
        for field in ("soff", "slen", "first"):
            c = Call(brb, with_lower)
            setattr(c, field, None)
            c.refused(b"NULL")
        c = Call(brb, with_lower)                   # data may be NULL only when every named segment is empty
        c.data = None
        c.refused(b"NULL data")


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
        c.ctxs = c.idx = c.data = c.soff = c.slen = c.low = c.first = c.fin = c.digests = None
        c.n = 0
        assert c(brb.BATCH_HOST) == 1
        assert c(brb.BATCH_DEVICE | brb.BATCH_ASYNC) == 1


def _compat_rows(brb, rng):
    """A table whose rows are compat contexts with 64 + 11 r bytes taken (0xA5 elsewhere)."""
    rows = np.full((N_CTX, 168), 0xA5, np.uint8)
    for r in range(N_CTX):
        brb.md5_ctx_init(rows[r])
        brb.md5_ctx_update(rows[r], rng.integers(0, 256, 64 + 11 * r, dtype=np.uint8).tobytes())
    return rows


def test_without_device_refuses_with_a_reason(brb):
    """No CPU fallback: without a usable device the call returns 0 and says why, and writes nothing.  With
    a device the same call must leave what the compat functions leave, segment by segment."""
    L = brb.lib()
    have_gpu = brb.gpu_available()
    for with_lower in (True, False):
        c = Call(brb, with_lower)
        c.ctxs = _compat_rows(brb, np.random.default_rng(5))
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
                    update = brb.md5_ctx_update_lower if c.low is None or c.low[s] else brb.md5_ctx_update
                    update(want[r], c.data[o:o + n].tobytes() if n else b"")
                if not c.fin[k]:
                    have = int(want[r].view(np.uint32)[4]) & 63
                    assert np.array_equal(c.ctxs[r, :24 + have], want[r, :24 + have])
                    assert (c.digests[k] == 0xA5).all()
                    continue
                d = brb.md5_ctx_final(want[r])
                assert c.digests[k].tobytes() == d
                assert np.array_equal(c.ctxs[r, :24], want[r, :24]) and np.array_equal(c.ctxs[r, 88:], want[r, 88:])
            assert np.array_equal(c.ctxs[named[1]], before[named[1]])    # no segments, no final: untouched
            rest = [r for r in range(N_CTX) if r not in named]
            assert np.array_equal(c.ctxs[rest], before[rest])
            assert np.array_equal(c.data, data0)
