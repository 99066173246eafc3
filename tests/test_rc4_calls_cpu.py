"""RC4 batch calls with one buffer per stream (BRB_RC4_CryptBatch, BRB_RC4MD5_FrameBatch, BRB_RC4MD5_OpenBatch):
every refusal that comes before device work, and the order in which this family takes them.  The twin of
tests/test_rc4_lists_cpu.py for the list calls.  No test here needs a GPU; where one is present the valid
call is checked against the oracle instead of against the refusal.

The order differs from the list family's in one place: these calls probe the device before they look at
the ranges (NULL pointers, counts and flags, the device, then the ranges), so a wrapping range is a bad
argument only where a device is present -- see test_wrapping_range_is_refused."""
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

CALLS = ("crypt", "frame", "open")
N = 4
FAR = (1 << 63) + 12345                             # the offset of an empty stream need not be memory
ONE_EACH = np.arange(N + 1, dtype=np.uint64)        # the oracle's list form of one buffer per stream


class Call:
    """One raw call: the arrays it takes, any of them replaceable by None."""

    def __init__(self, brb, kind):
        self.brb, self.kind = brb, kind
        L = brb.lib()
        self.fn = {"crypt": L.BRB_RC4_CryptBatch, "frame": L.BRB_RC4MD5_FrameBatch, "open": L.BRB_RC4MD5_OpenBatch}[kind]
        self.states = brb.rc4_states([b"key-%d" % i for i in range(N)])
        self.data = np.arange(256, dtype=np.uint8)
        self.out = np.full(512, 0xA5, np.uint8)
        # streams of 65, 0, 9 and 100 bytes (1..65, none, 74..82, 130..229); frames of 95, 30, 39 and 130
        self.off = np.array([1, FAR, 74, 130], np.uint64)
        self.len = np.array([65, 0, 9, 100], np.uint32)
        self.salts = np.arange(N, dtype=np.uint64) * 0x0101010101010101
        self.foff = np.array([0, 100, 140, 180], np.uint64)
        self.valid = np.full(N, 0xA5, np.uint8)
        self.n = N

    def __call__(self, flags=0):
        p = lambda a: None if a is None else a.ctypes.data
        if self.kind == "crypt":
            return self.fn(p(self.states), p(self.data), p(self.out), p(self.off), p(self.len), self.n, flags, None)
        if self.kind == "frame":
            return self.fn(p(self.states), p(self.data), p(self.off), p(self.len), p(self.salts), p(self.out),
                           p(self.foff), self.n, flags, None)
        return self.fn(p(self.states), p(self.data), p(self.out), p(self.off), p(self.len), self.n, p(self.valid),
                       flags, None)

    def fields(self):
        return {"crypt": ("states", "data", "out", "off", "len"),
                "frame": ("states", "data", "off", "len", "salts", "out", "foff"),
                "open": ("states", "data", "out", "off", "len", "valid")}[self.kind]

    def refused(self, reason, flags=0, rc_want=-1):
        keep = [a.copy() if a is not None else None for a in (self.states, self.out, self.valid)]
        rc = self(flags)
        err = self.brb.lib().BRB_CryptoGPU_LastError()
        assert rc == rc_want and reason in err and err, (self.kind, rc, err)
        for a, k in zip((self.states, self.out, self.valid), keep):
            assert a is None or np.array_equal(a, k)


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
def test_oversized_count_is_refused(brb, kind):
    c = Call(brb, kind)
    c.n = 1 << 33
    c.refused(b"split the batch")
    c.refused(b"split the batch", brb.BATCH_DEVICE)


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
    device the same call must leave what the oracle leaves, stream by stream."""
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
            st, out = expect_crypt(orc, before, c.data, c.off, c.len, ONE_EACH, out=out0)
        elif kind == "frame":
            st, out = expect_frame(orc, before, c.data, c.off, c.len, c.salts, out0, c.foff, ONE_EACH)
        else:
            st, out, valid = expect_open(orc, before, c.data, c.off, c.len, ONE_EACH, out=out0)
            assert np.array_equal(c.valid, valid)
        assert np.array_equal(c.states, st) and np.array_equal(c.out, out)


@pytest.mark.parametrize("kind", CALLS)
def test_wrapping_range_is_refused(brb, kind):
    """A range that wraps the address space is a bad argument (-1, "wraps") and nothing is written -- where a
    device is present.  This family probes the device before it looks at the ranges (the list family looks
    first), so without a device the same call is not done (0) for the device's reason; nothing is written
    either way."""
    have_gpu = brb.gpu_available()
    rc_want, reason = (-1, b"wraps") if have_gpu else (0, b"")
    c = Call(brb, kind)
    c.off[3] = (1 << 64) - 10
    c.refused(reason, rc_want=rc_want)
    if kind == "frame":
        c = Call(brb, kind)
        c.foff[1] = (1 << 64) - 20                  # the empty payload's frame is 30 bytes
        c.refused(reason, rc_want=rc_want)
