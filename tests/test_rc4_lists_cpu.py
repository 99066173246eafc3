"""RC4 batch calls with a buffer list per stream (BRB_RC4_CryptListBatch, BRB_RC4MD5_FrameListBatch,
BRB_RC4MD5_OpenListBatch): the exports, every host-mode refusal -- all of which come before any device
work -- and the expected-value builder of tests/test_rc4_lists.py.  No test here needs a GPU; where
one is present the valid call is checked against the oracle instead of against the refusal."""
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


E = _sibling("rc4_lists_expect")
expect_crypt, expect_frame, expect_open = E.expect_crypt, E.expect_frame, E.expect_open

SYMBOLS = {"BRB_RC4_CryptListBatch", "BRB_RC4MD5_FrameListBatch", "BRB_RC4MD5_OpenListBatch"}
CALLS = ("crypt", "frame", "open")
N = 4
FAR = (1 << 63) + 12345                             # the offset of an empty buffer need not be memory


class Call:
    """One raw call: the arrays it takes, any of them replaceable by None."""

    def __init__(self, brb, kind):
        self.brb, self.kind = brb, kind
        L = brb.lib()
        self.fn = {"crypt": L.BRB_RC4_CryptListBatch, "frame": L.BRB_RC4MD5_FrameListBatch,
                   "open": L.BRB_RC4MD5_OpenListBatch}[kind]
        self.states = brb.rc4_states([b"key-%d" % i for i in range(N)])
        self.data = np.arange(256, dtype=np.uint8)
        self.out = np.full(512, 0xA5, np.uint8)
        # stream 0: two buffers; stream 1: none; stream 2: one; stream 3: an empty one between two with bytes
        # (buffers of one call must not overlap: 1..65, 70..72, 74..82, 130..229, 84..123)
        self.off = np.array([1, 70, 74, 130, FAR, 84], np.uint64)
        self.len = np.array([65, 3, 9, 100, 0, 40], np.uint32)
        self.first = np.array([0, 2, 2, 3, 6], np.uint64)
        self.salts = np.arange(6, dtype=np.uint64) * 0x0101010101010101
        self.foff = np.array([0, 100, 140, 180, 315, 350], np.uint64)
        self.valid = np.full(6, 0xA5, np.uint8)
        self.n = N

    def __call__(self, flags=0):
        p = lambda a: None if a is None else a.ctypes.data
        if self.kind == "crypt":
            return self.fn(p(self.states), p(self.data), p(self.out), p(self.off), p(self.len), p(self.first), self.n,
                           flags, None)
        if self.kind == "frame":
            return self.fn(p(self.states), p(self.data), p(self.off), p(self.len), p(self.salts), p(self.out),
                           p(self.foff), p(self.first), self.n, flags, None)
        return self.fn(p(self.states), p(self.data), p(self.out), p(self.off), p(self.len), p(self.first), self.n,
                       p(self.valid), flags, None)

    def fields(self):
        return {"crypt": ("states", "data", "out", "off", "len", "first"),
                "frame": ("states", "data", "off", "len", "salts", "out", "foff", "first"),
                "open": ("states", "data", "out", "off", "len", "first", "valid")}[self.kind]

    def refused(self, reason, flags=0):
        keep = [a.copy() if a is not None else None for a in (self.states, self.out, self.valid)]
        rc = self(flags)
        err = self.brb.lib().BRB_CryptoGPU_LastError()
        assert rc == -1 and reason in err, (self.kind, rc, err)
        for a, k in zip((self.states, self.out, self.valid), keep):
            assert a is None or np.array_equal(a, k)


def test_symbols_exported(brb):
    assert SYMBOLS <= brb.exported_symbols()
    assert brb.BATCHER_CONN_LISTS == 0x800


@pytest.mark.parametrize("kind", CALLS)
def test_null_required_pointer_is_refused(brb, kind):
    for field in Call(brb, kind).fields():
        c = Call(brb, kind)
        setattr(c, field, None)
        c.refused(b"NULL")
        c = Call(brb, kind)
        setattr(c, field, None)
        c.refused(b"NULL", brb.BATCH_DEVICE)


@pytest.mark.parametrize("kind", CALLS)
def test_decreasing_first_buf_is_refused(brb, kind):
    c = Call(brb, kind)
    c.first[2] = 1
    c.refused(b"non-decreasing")
    c.refused(b"non-decreasing", brb.BATCH_ALL_DEVICES)


@pytest.mark.parametrize("kind", CALLS)
def test_wrapping_buffer_is_refused(brb, kind):
    c = Call(brb, kind)
    c.off[3] = (1 << 64) - 10
    c.refused(b"wraps")
    if kind == "frame":
        c = Call(brb, kind)
        c.foff[4] = (1 << 64) - 20                  # the empty payload's frame is 30 bytes
        c.refused(b"wraps")


@pytest.mark.parametrize("kind", CALLS)
def test_oversized_counts_are_refused(brb, kind):
    c = Call(brb, kind)
    c.n = 1 << 33
    c.refused(b"split the batch")
    c.refused(b"split the batch", brb.BATCH_DEVICE)
    c = Call(brb, kind)                             # more buffers than a launch takes
    c.first[1:] = 1 << 33
    c.refused(b"split the batch")


@pytest.mark.parametrize("kind", CALLS)
def test_all_devices_needs_host_pointers(brb, kind):
    Call(brb, kind).refused(b"ALL_DEVICES", brb.BATCH_DEVICE | brb.BATCH_ALL_DEVICES)


@pytest.mark.parametrize("kind", CALLS)
def test_empty_batch_is_done(brb, kind):
    c = Call(brb, kind)
    for f in c.fields():
        setattr(c, f, None)
    c.n = 0
    assert c(brb.BATCH_HOST) == 1
    assert c(brb.BATCH_DEVICE | brb.BATCH_ASYNC) == 1


@pytest.mark.parametrize("kind", CALLS)
def test_without_device_refuses_with_a_reason(brb, orc, kind):
    """No CPU fallback: without a usable device the call returns 0 and says why, and writes nothing.  With a
    device the same call must leave what the oracle, chained over each stream's list, leaves."""
    L = brb.lib()
    have_gpu = brb.gpu_available()
    for flags in (brb.BATCH_HOST, brb.BATCH_ALL_DEVICES):
        c = Call(brb, kind)
        before, out0 = c.states.copy(), c.out.copy()
        rc = c(flags)
        if not have_gpu:
            assert rc == 0 and L.BRB_CryptoGPU_LastError()
            assert np.array_equal(c.states, before) and np.array_equal(c.out, out0) and (c.valid == 0xA5).all()
            continue
        assert rc == 1, L.BRB_CryptoGPU_LastError()
        if kind == "crypt":
            st, out = expect_crypt(orc, before, c.data, c.off, c.len, c.first, out=out0)
        elif kind == "frame":
            st, out = expect_frame(orc, before, c.data, c.off, c.len, c.salts, out0, c.foff, c.first)
        else:
            st, out, valid = expect_open(orc, before, c.data, c.off, c.len, c.first, out=out0)
            assert np.array_equal(c.valid, valid)
        assert np.array_equal(c.states, st) and np.array_equal(c.out, out)
        assert np.array_equal(c.states[1], before[1])            # no buffers: untouched


def test_expected_value_builder_split_invariance(orc):
    """Chaining orc.rc4_crypt over any split of a message equals one call over the whole: the property
    that makes the chained oracle the reference of a buffer list."""
    rng = np.random.default_rng(0x11575)
    for trial in range(20):
        key = rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
        msg = rng.integers(0, 256, int(rng.integers(0, 700)), dtype=np.uint8)
        st0 = np.frombuffer(orc.rc4_init(key), np.uint8)
        whole_st, whole = orc.rc4_crypt(st0.tobytes(), msg.tobytes())
        cuts = np.sort(rng.integers(0, msg.size + 1, int(rng.integers(0, 7))))
        edges = np.concatenate([[0], cuts, [msg.size]]).astype(np.uint64)
        off, ln = edges[:-1], np.diff(edges.astype(np.int64)).astype(np.uint32)
        st, out = expect_crypt(orc, st0[None, :], msg, off, ln, np.array([0, len(off)], np.uint64))
        assert out.tobytes() == whole and st[0].tobytes() == whole_st, trial
    # a stream without buffers keeps its state; buffers of other streams do not touch it
    st0 = np.stack([np.frombuffer(orc.rc4_init(b"a"), np.uint8), np.frombuffer(orc.rc4_init(b"b"), np.uint8)])
    msg = np.arange(10, dtype=np.uint8)
    st, out = expect_crypt(orc, st0, msg, np.array([0], np.uint64), np.array([10], np.uint32), np.array([0, 0, 1], np.uint64))
    assert np.array_equal(st[0], st0[0]) and out.tobytes() == orc.rc4_crypt(st0[1].tobytes(), msg.tobytes())[1]
