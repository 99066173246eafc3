"""BRB_RC4_MixedListBatch and the transform batcher's per-connection algo, as far as no GPU is needed: the
exports, every host-mode refusal of the mixed call -- all of which come before any device work -- the
expected-value builder of tests/test_rc4_mixed.py on a hand-made call, the argument refusals of Create /
EnableAlgo / EnableBatchAlgo / Disable that need no device, and the planner's mixed layout
(tests/c/mixed_plan_check.cpp, a stand-alone program built with ASan + UBSan, runtimes linked statically,
nothing preloaded, run once).  Where a GPU is present the valid call is checked against the oracle instead
of against the "no device" refusal."""
import ctypes
import importlib.util
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _sibling(name):
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
        sys.modules[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[name])
    return sys.modules[name]


X = _sibling("rc4_mixed_expect")

SYMBOLS = {"BRB_RC4_MixedListBatch", "BRB_TransformBatcherEnableAlgo", "BRB_TransformBatcherEnableBatchAlgo",
           "BRB_TransformBatcherDisable"}
FAR = (1 << 63) + 12345                             # the offsets of an empty buffer need not be memory
GAP, FILL = 0xA5, 0x5A
N, N_STATES = 4, 6


class Call:
    """One raw call: the arrays it takes, any of them replaceable by None.  Stream 0 crypts two buffers with
    state 5, stream 1 (open, state 0) has none, stream 2 frames one with state 2, stream 3 opens three with
    state 3, the middle one empty and far away.  States 1 and 4 are not named."""

    def __init__(self, brb, orc=None):
        self.brb = brb
        self.fn = brb.lib().BRB_RC4_MixedListBatch
        self.states = brb.rc4_states([b"key-%d" % i for i in range(N_STATES)])
        self.n_states = N_STATES
        self.index = np.array([5, 0, 2, 3], np.uint32)
        self.kind = np.array([X.CRYPT, X.OPEN, X.FRAME, X.OPEN], np.uint8)
        self.data = np.full(320, GAP, np.uint8)
        self.data[1:240] = (np.arange(239) * 7 + 3).astype(np.uint8)
        self.out = np.full(512, FILL, np.uint8)
        # inputs 1..65, 70..72, 74..82, 130..229, (empty), 84..123; outputs anywhere else, unaligned
        self.off = np.array([1, 70, 74, 130, FAR, 84], np.uint64)
        self.len = np.array([65, 3, 9, 100, 0, 40], np.uint32)
        self.ooff = np.array([3, 101, 140, 181, FAR + 7, 301], np.uint64)      # the frame: 140 .. 178
        self.first = np.array([0, 2, 2, 3, 6], np.uint64)
        self.salts = np.arange(6, dtype=np.uint64) * 0x0101010101010101
        self.valid = np.full(6, 0xA5, np.uint8)
        self.n = N
        if orc is not None:                          # what a peer with key-3 wrote to stream 3: a frame, nothing, a stub
            s = orc.rc4_init(b"key-3")
            s, w = orc.rc4md5_frame(s, bytes(range(70)), 99)
            self.data[130:230] = np.frombuffer(w, np.uint8)
            s, w = orc.rc4_crypt(s, bytes(40))
            self.data[84:124] = np.frombuffer(w, np.uint8)

    def __call__(self, flags=0):
        p = lambda a: None if a is None else a.ctypes.data
        return self.fn(p(self.states), self.n_states, p(self.index), p(self.kind), p(self.data), p(self.out), p(self.off),
                       p(self.len), p(self.ooff), p(self.salts), p(self.first), self.n, p(self.valid), flags, None)

    def refused(self, reason, flags=0):
        keep = [a.copy() if a is not None else None for a in (self.states, self.out, self.valid)]
        rc = self(flags)
        err = self.brb.lib().BRB_CryptoGPU_LastError()
        assert rc == -1 and reason in err, (rc, err)
        for a, k in zip((self.states, self.out, self.valid), keep):
            assert a is None or np.array_equal(a, k)


REQUIRED = ("states", "kind", "data", "out", "off", "len", "ooff", "first")


def test_symbols_and_constants(brb):
    assert SYMBOLS <= brb.exported_symbols()
    assert (brb.RC4_KIND_CRYPT, brb.RC4_KIND_FRAME, brb.RC4_KIND_OPEN) == (0, 1, 2)
    assert brb.BATCHER_MIXED == 0x1000
    with open(os.path.join(ROOT, "include", "brb_crypto.h")) as f:
        header = f.read()
    for line in ("#define BRB_RC4_KIND_CRYPT 0", "#define BRB_RC4_KIND_FRAME 1", "#define BRB_RC4_KIND_OPEN  2",
                 "#define BRB_BATCHER_MIXED         0x1000"):
        assert line in header, line


def test_null_required_pointer_is_refused(brb):
    for field in REQUIRED:
        for flags in (brb.BATCH_HOST, brb.BATCH_DEVICE):
            c = Call(brb)
            setattr(c, field, None)
            c.refused(b"NULL", flags)
    c = Call(brb)
    c.salts = None                                  # needed: stream 2 frames
    c.refused(b"NULL salts")
    c = Call(brb)
    c.valid = None                                  # needed: streams 1 and 3 open
    c.refused(b"NULL valid")


def test_kind_above_two_is_refused(brb):
    for bad in (3, 255):
        c = Call(brb)
        c.kind[1] = bad
        c.refused(b"kind")


def test_decreasing_first_buf_is_refused(brb):
    c = Call(brb)
    c.first[2] = 1
    c.refused(b"non-decreasing")


def test_wrapping_ranges_are_refused(brb):
    c = Call(brb)
    c.off[3] = (1 << 64) - 10                       # an input
    c.refused(b"wraps")
    c = Call(brb)
    c.ooff[0] = (1 << 64) - 10                      # an output of the same length
    c.refused(b"wraps")
    c = Call(brb)
    c.len[2] = 0
    c.ooff[2] = (1 << 64) - 20                      # the empty payload's frame is 30 bytes
    c.refused(b"wraps")
    c = Call(brb)
    c.ooff[4] = (1 << 64) - 1                       # an empty open buffer writes nothing: no wrap
    c.off[4] = (1 << 64) - 1
    assert c() in (0, 1)


def test_state_index_is_checked(brb):
    c = Call(brb)
    c.index[2] = N_STATES
    c.refused(b"out of range")
    c = Call(brb)
    c.index[1] = 5                                  # also stream 0's
    c.refused(b"named twice")
    c = Call(brb)
    c.index = None
    c.n_states = N - 1
    c.refused(b"> n_ctx")


def test_oversized_counts_are_refused(brb):
    c = Call(brb)
    c.n = 1 << 33
    c.refused(b"split the batch")
    c.refused(b"split the batch", brb.BATCH_DEVICE)
    c = Call(brb)                                   # more buffers than a launch takes
    c.first[1:] = 1 << 33
    c.refused(b"split the batch")


def test_all_devices_is_refused(brb):
    Call(brb).refused(b"does not split", brb.BATCH_ALL_DEVICES)
    Call(brb).refused(b"does not split", brb.BATCH_DEVICE | brb.BATCH_ALL_DEVICES)


def test_empty_batch_is_done(brb):
    c = Call(brb)
    for f in REQUIRED + ("index", "salts", "valid"):
        setattr(c, f, None)
    c.n = c.n_states = 0
    assert c(brb.BATCH_HOST) == 1
    assert c(brb.BATCH_DEVICE | brb.BATCH_ASYNC) == 1


def _by_hand(orc, c):
    """The hand-made call through the oracle's scalar calls, written out stream by stream."""
    st, out, valid = c.states.copy(), c.out.copy(), c.valid.copy()
    s = st[5].tobytes()                             # stream 0: crypt, two buffers
    s, o = orc.rc4_crypt(s, c.data[1:66].tobytes())
    out[3:68] = np.frombuffer(o, np.uint8)
    s, o = orc.rc4_crypt(s, c.data[70:73].tobytes())
    out[101:104] = np.frombuffer(o, np.uint8)
    st[5] = np.frombuffer(s, np.uint8)
    s, fr = orc.rc4md5_frame(st[2].tobytes(), c.data[74:83].tobytes(), int(c.salts[2]))   # stream 2: one frame
    out[140:179] = np.frombuffer(fr, np.uint8)
    st[2] = np.frombuffer(s, np.uint8)
    s = st[3].tobytes()                             # stream 3: a frame, an empty buffer, a stub
    s, dec, ok0 = orc.rc4md5_open(s, c.data[130:230].tobytes())
    out[181:281] = np.frombuffer(dec, np.uint8)
    s, _, ok1 = orc.rc4md5_open(s, b"")
    s, dec, ok2 = orc.rc4md5_open(s, c.data[84:124].tobytes())
    out[301:341] = np.frombuffer(dec, np.uint8)
    st[3] = np.frombuffer(s, np.uint8)
    valid[3:6] = [ok0, ok1, ok2]
    return st, out, valid


def test_expected_value_builder_on_a_hand_made_call(orc, brb):
    """A stream of each kind, a stream without buffers, an empty buffer at a far offset: the builder equals
    the scalar calls written out by hand; the frame a peer wrote is valid, the empty buffer and the stub are
    not; states that are not named, the idle stream's state and the valid entries of buffers that are not
    OPEN keep every byte."""
    c = Call(brb, orc)
    st, out, valid = X.expect_mixed(orc, c.states, c.kind, c.data, c.off, c.len, c.ooff, c.first, c.out, c.salts, c.valid,
                                    c.index)
    want = _by_hand(orc, c)
    assert np.array_equal(st, want[0]) and np.array_equal(out, want[1]) and np.array_equal(valid, want[2])
    assert valid.tolist() == [0xA5, 0xA5, 0xA5, 1, 0, 0]
    for row in (0, 1, 4):
        assert np.array_equal(st[row], c.states[row])
    for row in (5, 2, 3):
        assert not np.array_equal(st[row], c.states[row])
    written = np.zeros(out.size, bool)
    for a, b in ((3, 68), (101, 104), (140, 179), (181, 281), (301, 341)):
        written[a:b] = True
    assert (out[~written] == FILL).all() and (out[written] != FILL).any()
    # without an index stream i uses state i
    st2, _, _ = X.expect_mixed(orc, c.states, c.kind, c.data, c.off, c.len, c.ooff, c.first, c.out, c.salts, c.valid)
    assert np.array_equal(st2[1], c.states[1]) and np.array_equal(st2[4:], c.states[4:])
    assert not np.array_equal(st2[0], c.states[0])


def test_without_device_refuses_with_a_reason(brb, orc):
    """No CPU fallback: without a usable device the call returns 0 and says why, and writes nothing.  With a
    device the same call must leave what the oracle leaves."""
    L = brb.lib()
    c = Call(brb, orc)
    before = (c.states.copy(), c.out.copy(), c.valid.copy())
    want = _by_hand(orc, c)
    rc = c()
    if not brb.gpu_available():
        assert rc == 0 and L.BRB_CryptoGPU_LastError()
        want = before
    else:
        assert rc == 1, L.BRB_CryptoGPU_LastError()
    for got, w in zip((c.states, c.out, c.valid), want):
        assert np.array_equal(got, w)


def test_batcher_argument_refusals(brb):
    """What Create, EnableAlgo, EnableBatchAlgo and Disable refuse before they need a device."""
    L = brb.lib()
    key = b"0123456789"
    assert L.BRB_TransformBatcherEnableAlgo(None, 0, 1, key, len(key)) == -1
    assert L.BRB_TransformBatcherDisable(None, 0) == -1
    ids = np.zeros(1, np.uint32)
    assert L.BRB_TransformBatcherEnableBatchAlgo(None, ids.ctypes.data, 1, None, None, None, None) == -1
    # Create knows the flag: a bad numeric algo under it is refused as a bad algo, a good one is not
    assert not L.BRB_TransformBatcherCreate(4, 1 << 12, 3 | brb.BATCHER_MIXED)
    assert b"algo" in L.BRB_CryptoGPU_LastError()
    h = L.BRB_TransformBatcherCreate(4, 1 << 12, 1 | brb.BATCHER_MIXED | brb.BATCHER_CONN_LISTS)
    if h:
        try:
            assert L.BRB_TransformBatcherEnableAlgo(h, 0, 3, key, len(key)) == -1
            assert L.BRB_TransformBatcherEnableAlgo(h, 4, 1, key, len(key)) == -1      # no such connection
            assert L.BRB_TransformBatcherDisable(h, 4) == -1
        finally:
            L.BRB_TransformBatcherDestroy(ctypes.c_void_p(h))
    else:
        assert not brb.gpu_available() and b"algo RC4 (1)" not in L.BRB_CryptoGPU_LastError()


def test_mixed_plan_against_model(tmp_path):
    exe = tmp_path / "mixed_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "brb_framework_amd", "csrc", "gpu"),
                    os.path.join(ROOT, "tests", "c", "mixed_plan_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
