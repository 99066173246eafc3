"""Streaming MD5 / SHA-1 contexts as a batch (BRB_MD5InitBatch / UpdateBatch / FinalBatch and the BrbSha1_
three): the exports and every host-mode refusal, which all come before any device work.  No test here
needs a GPU; where one is present the valid call is checked against the compat functions instead of
against the refusal."""
import ctypes

import numpy as np
import pytest

ALGS = {"md5": ("BRB_MD5", 168, 16, 24), "sha1": ("BrbSha1_", 92, 20, 28)}   # prefix, context, digest, header bytes
OPS = ("Init", "Update", "Final")
SYMBOLS = {p + op + "Batch" for p, *_ in ALGS.values() for op in OPS}
N, N_CTX = 4, 6


class Call:
    """One raw call: the six arrays a call may take, any of them replaceable by None."""

    def __init__(self, brb, alg, op):
        prefix, self.width, self.dig, self.hdr = ALGS[alg]
        self.brb, self.alg, self.op = brb, alg, op
        self.fn = getattr(brb.lib(), prefix + op + "Batch")
        self.ctxs = np.full((N_CTX, self.width), 0xA5, np.uint8)
        self.idx = np.array([5, 0, 3, 2], np.uint32)
        self.data = np.arange(256, dtype=np.uint8)
        self.offs = np.array([1, 70, 2, 130], np.uint64)
        self.lens = np.array([65, 3, 0, 100], np.uint32)
        self.digests = np.full((N, self.dig), 0xA5, np.uint8)
        self.n, self.n_ctx = N, N_CTX

    def __call__(self, flags=0):
        p = lambda a: None if a is None else a.ctypes.data
        if self.op == "Init":
            return self.fn(p(self.ctxs), self.n_ctx, p(self.idx), self.n, flags, None)
        if self.op == "Update":
            return self.fn(p(self.ctxs), self.n_ctx, p(self.idx), p(self.data), p(self.offs), p(self.lens), self.n, flags, None)
        return self.fn(p(self.ctxs), self.n_ctx, p(self.idx), self.n, p(self.digests), flags, None)

    def refused(self, reason, flags=0):
        keep = self.ctxs
        rc = self(flags)
        err = self.brb.lib().BRB_CryptoGPU_LastError()
        assert rc == -1 and reason in err, (self.alg, self.op, rc, err)
        if keep is not None:
            assert (keep == 0xA5).all()
        assert (self.digests is None) or (self.digests == 0xA5).all()


def _all_calls(brb):
    return [Call(brb, alg, op) for alg in ALGS for op in OPS]


def test_symbols_exported(brb):
    assert SYMBOLS <= brb.exported_symbols()


def test_null_required_pointer_is_refused(brb):
    for c in _all_calls(brb):
        keep = c.ctxs
        c.ctxs = None
        c.refused(b"NULL")
        assert (keep == 0xA5).all()
    for alg in ALGS:
        for field in ("offs", "lens"):
            c = Call(brb, alg, "Update")
            setattr(c, field, None)
            c.refused(b"NULL")
        c = Call(brb, alg, "Update")               # data may be NULL only when every length is 0
        c.data = None
        c.refused(b"NULL data")
    c = Call(brb, "sha1", "Final")                  # SHA-1's digests are required, MD5's are not
    c.digests = None
    c.refused(b"NULL")


def test_index_out_of_range_is_refused(brb):
    for c in _all_calls(brb):
        c.idx[2] = N_CTX
        c.refused(b"out of range")
        c.refused(b"out of range", brb.BATCH_ALL_DEVICES)


def test_no_index_and_more_items_than_contexts_is_refused(brb):
    for c in _all_calls(brb):
        c.idx = None
        c.n_ctx = N - 1
        c.refused(b"n_ctx")


def test_duplicate_index_is_refused(brb):
    for c in _all_calls(brb):
        c.idx[3] = c.idx[0]
        c.refused(b"named twice")
        c.refused(b"named twice", brb.BATCH_ALL_DEVICES)


def test_oversized_item_count_is_refused(brb):
    for c in _all_calls(brb):
        c.n = 1 << 33
        c.refused(b"split the batch")
        c.refused(b"split the batch", brb.BATCH_DEVICE)


def test_all_devices_needs_host_pointers(brb):
    for c in _all_calls(brb):
        c.refused(b"ALL_DEVICES", brb.BATCH_DEVICE | brb.BATCH_ALL_DEVICES)


def test_empty_batch_is_done(brb):
    for c in _all_calls(brb):
        c.ctxs = c.idx = c.data = c.offs = c.lens = c.digests = None
        c.n = 0
        assert c(brb.BATCH_HOST) == 1
        assert c(brb.BATCH_DEVICE | brb.BATCH_ASYNC) == 1


def _compat_rows(brb, alg, width, rng):
    """A table whose rows are compat contexts with 64 + 0 .. 63 bytes taken (0xA5 elsewhere), and the bytes."""
    init, update = getattr(brb, alg + "_ctx_init"), getattr(brb, alg + "_ctx_update")
    rows = np.full((N_CTX, width), 0xA5, np.uint8)
    msgs = []
    for r in range(N_CTX):
        init(rows[r])
        msgs.append(rng.integers(0, 256, 64 + 11 * r, dtype=np.uint8).tobytes())
        update(rows[r], msgs[r])
    return rows, msgs


@pytest.mark.parametrize("alg", list(ALGS))
def test_without_device_refuses_with_a_reason(brb, alg):
    """No CPU fallback: without a usable device every call returns 0 and says why, and writes nothing.
    With a device the same calls must leave what the compat functions leave."""
    L = brb.lib()
    have_gpu = brb.gpu_available()
    _, width, dig, hdr = ALGS[alg]
    rng = np.random.default_rng(5)
    update, final = getattr(brb, alg + "_ctx_update"), getattr(brb, alg + "_ctx_final")
    for op in OPS:
        c = Call(brb, alg, op)
        if op != "Init":
            c.ctxs, msgs = _compat_rows(brb, alg, width, rng)
        before = c.ctxs.copy()
        for flags in (brb.BATCH_HOST, brb.BATCH_ALL_DEVICES):
            c.ctxs[:] = before
            rc = c(flags)
            if not have_gpu:
                assert rc == 0 and L.BRB_CryptoGPU_LastError()
                assert np.array_equal(c.ctxs, before) and (c.digests == 0xA5).all()
                continue
            assert rc == 1, L.BRB_CryptoGPU_LastError()
            want = before.copy()
            named = [int(i) for i in c.idx]
            for k, r in enumerate(named):
                if op == "Init":
                    getattr(brb, alg + "_ctx_init")(want[r])
                    assert np.array_equal(c.ctxs[r], want[r])
                elif op == "Update":
                    o, n = int(c.offs[k]), int(c.lens[k])
                    update(want[r], c.data[o:o + n].tobytes())
                    have = len(msgs[r]) + n & 63
                    assert np.array_equal(c.ctxs[r, :hdr + have], want[r, :hdr + have])
                else:
                    d = final(want[r])
                    assert c.digests[k].tobytes() == d
                    if alg == "md5":
                        assert np.array_equal(c.ctxs[r, :24], want[r, :24]) and np.array_equal(c.ctxs[r, 88:], want[r, 88:])
                    else:
                        assert not c.ctxs[r].any()
            rest = [r for r in range(N_CTX) if r not in named]
            assert np.array_equal(c.ctxs[rest], before[rest])
