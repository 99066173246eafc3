"""The transform batcher with an algo per connection (BRB_BATCHER_MIXED, EnableAlgo, EnableBatchAlgo, Disable).

Every result is compared bit for bit with the oracle's scalar calls chained on the host, callbacks in
submission order, GetState after every round; a mixed batcher is also held against ordinary batchers fed
the same traffic.  The launch count is read through the existing InjectFault hook: nothing on the device
fails in any of these tests.
"""
import importlib.util
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _sibling(name, file=None):
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, (file or name) + ".py"))
        sys.modules[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[name])
    return sys.modules[name]


L = _sibling("rc4_lists_shapes", "test_rc4_lists")     # its traffic generator and driver, under a name of its own

RC4, RC4_MD5 = 1, 2
ZERO = bytes(264)


@pytest.fixture(scope="module")
def torch_dev(brb):
    import torch
    assert torch.cuda.is_available(), "no HIP device visible to torch"
    assert brb.gpu_available(), brb.lib().BRB_CryptoGPU_LastError()
    return torch


class Peer:
    """The oracle's side of a set of connections: our read and write states and the peer's write state."""

    def __init__(self, orc, keys, algos):
        self.orc, self.algos = orc, list(algos)
        self.rd = [orc.rc4_init(k) for k in keys]
        self.wr = [orc.rc4_init(k) for k in keys]
        self.peer = [orc.rc4_init(k) for k in keys]

    def rekey(self, c, key, algo):
        self.rd[c], self.wr[c], self.peer[c] = (self.orc.rc4_init(key) for _ in range(3))
        self.algos[c] = algo

    def read(self, c, payload, salt=7, spoil=None):
        """What the peer sends for `payload` -> (the wire bytes to submit, the expected callback)."""
        orc = self.orc
        if self.algos[c] == RC4:
            self.peer[c], wire = orc.rc4_crypt(self.peer[c], payload)
            self.rd[c], dec = orc.rc4_crypt(self.rd[c], wire)
            return wire, (c, 0, dec, 1)
        if spoil == "stub":
            self.peer[c], wire = orc.rc4_crypt(self.peer[c], payload[:29])   # no frame at all
        else:
            self.peer[c], wire = orc.rc4md5_frame(self.peer[c], payload, salt)
            if spoil == "bit":
                wire = bytearray(wire)
                wire[8 + salt % (len(wire) - 8)] ^= 2
                wire = bytes(wire)
        self.rd[c], dec, ok = orc.rc4md5_open(self.rd[c], wire)
        return wire, (c, 0, dec, ok)

    def write(self, c, payload, salt):
        if self.algos[c] == RC4:
            self.wr[c], out = self.orc.rc4_crypt(self.wr[c], payload)
        else:
            self.wr[c], out = self.orc.rc4md5_frame(self.wr[c], payload, salt)
        return (c, 1, out, 1)

    def states(self):
        return [list(self.rd), list(self.wr)]


def _traffic(orc, algos, seed, rounds=3, most=3):
    """`rounds` rounds of an event loop over len(algos) connections: per round every connection gets 0..most
    buffers in each direction, reads and writes interleaved.  -> keys, and per round the submissions
    [(conn, op, bytes, salt)], the oracle's callbacks and the oracle's states after the round."""
    rng = np.random.default_rng([seed, 0x717])
    C = len(algos)
    keys = [rng.integers(0, 256, int(rng.integers(4, 32)), dtype=np.uint8).tobytes() for _ in range(C)]
    peer = Peer(orc, keys, algos)
    out = []
    for _ in range(rounds):
        subs, expect = [], []
        todo = [(c, op) for c in range(C) for op in (0, 1) for _ in range(int(rng.integers(0, most + 1)))]
        for t in rng.permutation(len(todo)):
            c, op = todo[t]
            n = int(rng.choice([0, 1, 3, 29, 31, 64, 65, 200, 1500]))
            payload = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            salt = int(rng.integers(0, 2**32))
            if op == 0:
                spoil = rng.choice(["stub", "bit", None, None, None, None, None, None])
                wire, want = peer.read(c, payload, salt, spoil)
                subs.append((c, 0, wire, 0))
            else:
                want = peer.write(c, payload, salt)
                subs.append((c, 1, payload, salt))
            expect.append(want)
        out.append((subs, expect, peer.states()))
    return keys, out


def _drive(brb, keys, algos, rounds, pipelined, only=None, **kw):
    """Feeds the traffic (of the connections in `only`, default all) to a batcher -> per round (results,
    [read states, write states] of every connection)."""
    C = len(keys)
    b = brb.TransformBatcher(16, 1 << 20, pipelined=pipelined, **kw)
    conns = [c for c in range(C) if only is None or c in only]
    if kw.get("mixed"):
        b.enable_batch(conns, [keys[c] for c in conns], [algos[c] for c in conns])
    else:
        b.enable_batch(conns, [keys[c] for c in conns])
    res, pending = [], None
    snap = lambda: [[b.state(c, op) for c in range(C)] for op in (0, 1)]
    for subs, _, _ in rounds:
        for c, op, data, salt in subs:
            if c in conns:
                assert (b.read(c, data) if op == 0 else b.write(c, data, salt)) == 1
        if pipelined:
            got = b.flush_async()
            if pending is not None:
                res.append([got, pending])
            pending = snap()
        else:
            res.append([b.flush(), snap()])
    if pipelined:
        res.append([b.flush(), pending])
    b.close()
    return res


# all-devices in two parts puts connection c in part c % 2: with alternating algos each part's rounds are of
# one algo, so that mode also runs with the algos in pairs, which mixes both algos in both parts
@pytest.mark.parametrize("mode,algos", [(m, [RC4, RC4_MD5] * 4) for m in ("copy", "zero_copy", "pipelined",
                                                                          "zero_copy_pipelined", "all_devices")] +
                         [("all_devices", [RC4, RC4, RC4_MD5, RC4_MD5] * 2)],
                         ids=["copy", "zero_copy", "pipelined", "zero_copy_pipelined", "all_devices", "all_devices-pairs"])
def test_mixed_traffic(brb, orc, torch_dev, mode, algos):
    """8 connections, RC4 and RC4_MD5 alternating, three rounds of ragged reads and writes (0..3 per
    connection and direction) through one mixed batcher: results in submission order and GetState after
    every round equal the oracle, and GetState equals two ordinary batchers, one per algo, fed the same
    traffic."""
    keys, rounds = _traffic(orc, algos, 0xA160)
    kw = dict(zero_copy="zero_copy" in mode, all_devices=mode == "all_devices")
    pipelined = "pipelined" in mode
    with brb.TestOption("devices", 2 if mode == "all_devices" else 0):
        got = _drive(brb, keys, algos, rounds, pipelined, algo=RC4, mixed=True, **kw)
        plain = {a: _drive(brb, keys, algos, rounds, pipelined, only=[c for c in range(8) if algos[c] == a], algo=a, **kw)
                 for a in (RC4, RC4_MD5)}
    assert len(got) == len(rounds)
    kinds_seen = set()
    for r, ((subs, expect, states), (res, st)) in enumerate(zip(rounds, got)):
        if mode == "all_devices":
            assert L._by_conn(res) == L._by_conn(expect), r
        else:
            assert res == expect, r
        assert st == states, r
        for c in range(8):
            for op in (0, 1):
                assert plain[algos[c]][r][1][op][c] == states[op][c], (r, c, op)
        for a in (RC4, RC4_MD5):
            want = [e for e in expect if algos[e[0]] == a]
            assert (L._by_conn(plain[a][r][0]) == L._by_conn(want)) if mode == "all_devices" else plain[a][r][0] == want
        kinds_seen |= {(algos[c], op) for c, op, _, _ in subs}
    assert len(kinds_seen) == 4                                             # crypt both ways, open and frame


@pytest.mark.parametrize("algo", [RC4, RC4_MD5])
def test_default_algo_equals_conn_lists(brb, orc, torch_dev, algo):
    """Every connection on the batcher's own algo (Enable / EnableBatch, no algo given): a mixed batcher gives
    what a conn_lists batcher gives, and both what the oracle gives."""
    keys, rounds = L._traffic(orc, algo, 0xBA7)
    mixed = L._drive(brb, keys, rounds, False, algo=algo, mixed=True)
    lists = L._drive(brb, keys, rounds, False, algo=algo, conn_lists=True)
    both = L._drive(brb, keys, rounds, False, algo=algo, mixed=True, conn_lists=True)     # the flag implies lists
    for r, ((_, expect, states), (got, st), (ref, ref_st), (b_got, b_st)) in enumerate(zip(rounds, mixed, lists, both)):
        assert got == expect and ref == expect and b_got == expect, r
        assert st == states and ref_st == states and b_st == states, r


def _launch_count_round(brb, orc, fault, **kw):
    """The round of test_rc4_lists.py's launch counts, rebuilt: RC4_MD5; connection 0: three reads and two
    writes, connection 1: one read.  Without lists five launches (sub-rounds 0, 1, 2: READ+WRITE, READ+WRITE,
    READ), with conn_lists two (READ, WRITE), mixed one."""
    keys = [b"launch-count-0", b"launch-count-1"]
    b = brb.TransformBatcher(4, 1 << 16, RC4_MD5, **kw)
    b.inject_fault(fault)
    peer = Peer(orc, keys, [RC4_MD5, RC4_MD5])
    expect = []
    for c, k in enumerate(keys):
        b.enable(c, k)
    for c, op, n in [(0, 0, 100), (0, 1, 64), (1, 0, 7), (0, 0, 0), (0, 1, 1500), (0, 0, 65)]:
        payload = bytes((n + i) & 255 for i in range(n))
        if op == 0:
            wire, want = peer.read(c, payload, 11 * n)
            assert want[3] == 1 and b.read(c, wire) == 1
        else:
            want = peer.write(c, payload, 5 * n)
            assert b.write(c, payload, 5 * n) == 1
        expect.append(want)
    return b, expect, peer, keys


def test_mixed_round_is_one_launch(brb, orc, torch_dev):
    """InjectFault(1) on a mixed batcher never fires: launch 0 is all there is, the round is delivered whole."""
    b, expect, peer, _ = _launch_count_round(brb, orc, 1, mixed=True)
    assert b.flush() == expect
    assert [b.state(0, 0), b.state(1, 0), b.state(0, 1)] == [peer.rd[0], peer.rd[1], peer.wr[0]]
    b.close()


def test_injected_fault_at_launch_0_drops_the_round(brb, orc, torch_dev):
    """InjectFault(0): the round's one launch is reported failed on the host and nothing runs -- every
    callback DROPPED, every state as it was, no connection poisoned; with the hook off the next round is right."""
    b, expect, _, keys = _launch_count_round(brb, orc, 0, mixed=True)
    with pytest.raises(RuntimeError, match="dropped") as ei:
        b.flush()
    assert ei.value.code == brb.BATCH_DROPPED
    assert ei.value.results == [(c, op, b"", brb.TRANSFORM_DROPPED) for c, op, _, _ in expect]
    fresh = [orc.rc4_init(k) for k in keys]
    assert [b.state(c, op) for c in (0, 1) for op in (0, 1)] == [fresh[0], fresh[0], fresh[1], fresh[1]]
    b.inject_fault(-1)
    assert b.flush() == []
    peer = Peer(orc, keys, [RC4_MD5, RC4_MD5])
    wire, want_r = peer.read(1, b"after the drop", 3)
    want_w = peer.write(0, b"next", 3)
    assert b.read(1, wire) == 1 and b.write(0, b"next", 3) == 1              # not poisoned
    assert b.flush() == [want_r, want_w]
    assert b.state(1, 0) == peer.rd[1] and b.state(0, 1) == peer.wr[0]
    b.close()


def test_without_the_flag_the_same_round_is_five_launches(brb, orc, torch_dev):
    """A batcher without the flag behaves as before, down to its launch count: the same round under
    InjectFault(2) is dropped (launch 2 of 5 is sub-round 1's READ group), under InjectFault(5) delivered; with
    conn_lists it is two launches."""
    b, expect, _, _ = _launch_count_round(brb, orc, 2)
    with pytest.raises(RuntimeError, match="dropped") as ei:
        b.flush()
    assert ei.value.results == [(c, op, b"", brb.TRANSFORM_DROPPED) for c, op, _, _ in expect]
    b.close()
    b, expect, peer, _ = _launch_count_round(brb, orc, 5)                    # launches 0..4 are all there is
    assert b.flush() == expect
    assert [b.state(0, 0), b.state(1, 0), b.state(0, 1)] == [peer.rd[0], peer.rd[1], peer.wr[0]]
    b.close()
    b, expect, _, _ = _launch_count_round(brb, orc, 2, conn_lists=True)      # launches 0 and 1
    assert b.flush() == expect
    b.close()


def test_algo_change_between_rounds(brb, orc, torch_dev):
    """enable(conn, key, algo) from RC4 to RC4_MD5 between rounds: the next round frames and opens; the
    connection beside it keeps its algo."""
    keys = [b"first key", b"the other one"]
    b = brb.TransformBatcher(4, 1 << 16, RC4, mixed=True)
    peer = Peer(orc, keys, [RC4, RC4_MD5])
    b.enable(0, keys[0])                                                     # the default
    b.enable(1, keys[1], RC4_MD5)
    payload = bytes(range(100))
    for rnd in range(2):
        expect = []
        for c in (0, 1):
            wire, want = peer.read(c, payload, 5)
            assert b.read(c, wire) == 1 and b.write(c, payload, 9) == 1
            expect += [want, peer.write(c, payload, 9)]
        got = b.flush()
        assert got == expect
        assert [len(g[2]) for g in got] == ([100, 100, 130, 130] if rnd == 0 else [130] * 4)
        assert [b.state(c, op) for c in (0, 1) for op in (0, 1)] == [peer.rd[0], peer.wr[0], peer.rd[1], peer.wr[1]]
        if rnd == 0:
            b.enable(0, b"second key", RC4_MD5)
            peer.rekey(0, b"second key", RC4_MD5)
    b.close()


@pytest.mark.parametrize("mixed", [True, False], ids=["mixed", "plain"])
def test_disable(brb, orc, torch_dev, mixed):
    """Disable on any batcher: read and write are refused as for a connection never enabled, both states
    read back as 264 zero bytes, the connection beside it is untouched, and enable brings it back."""
    L_ = brb.lib()
    b = brb.TransformBatcher(4, 1 << 16, RC4_MD5, mixed=mixed)
    peer = Peer(orc, [b"k0", b"k1"], [RC4_MD5, RC4_MD5])
    b.enable(0, b"k0")
    b.enable(1, b"k1")
    wire, want = peer.read(0, b"before", 1)
    assert b.read(0, wire) == 1 and b.flush() == [want]
    b.disable(0)
    assert b.read(0, b"x" * 40) == -1 and b"not enabled" in L_.BRB_CryptoGPU_LastError()
    assert b.write(0, b"x", 1) == -1
    assert b.state(0, 0) == ZERO and b.state(0, 1) == ZERO
    assert b.state(1, 0) == peer.rd[1] and b.state(1, 1) == peer.wr[1]
    assert b.flush() == []
    b.disable(0)                                                             # twice is as once
    b.enable(0, b"k0 again")
    peer.rekey(0, b"k0 again", RC4_MD5)
    wire, want_r = peer.read(0, b"after", 2)
    want_w = peer.write(0, b"after", 3)
    assert b.read(0, wire) == 1 and b.write(0, b"after", 3) == 1
    assert b.flush() == [want_r, want_w]
    assert b.state(0, 0) == peer.rd[0] and b.state(0, 1) == peer.wr[0]
    b.close()


def test_pending_buffers_hold_back_rekeying(brb, orc, torch_dev):
    """Disable, EnableAlgo and EnableBatchAlgo return 0, with nothing changed, while the filling round holds a
    buffer of the connection (or of a listed one); the buffer is then delivered right under the old key."""
    L_ = brb.lib()
    keys = [b"old key 0", b"old key 1"]
    b = brb.TransformBatcher(4, 1 << 16, RC4, mixed=True)
    peer = Peer(orc, keys, [RC4_MD5, RC4])
    b.enable_batch([0, 1], keys, [RC4_MD5, RC4])
    want = peer.write(0, b"pending payload", 77)
    assert b.write(0, b"pending payload", 77) == 1
    new = b"new key"
    ids, al = np.array([1, 0], np.uint32), np.array([RC4_MD5, RC4], np.uint8)
    blob, offs, lens = brb.pack_keys([new, new])
    for call in (lambda: L_.BRB_TransformBatcherDisable(b.h, 0),
                 lambda: L_.BRB_TransformBatcherEnableAlgo(b.h, 0, RC4, new, len(new)),
                 lambda: L_.BRB_TransformBatcherEnableBatchAlgo(b.h, ids.ctypes.data, 2, al.ctypes.data, blob.ctypes.data,
                                                                offs.ctypes.data, lens.ctypes.data)):
        assert call() == 0 and b"round being filled" in L_.BRB_CryptoGPU_LastError()
        assert [b.state(c, op) for c in (0, 1) for op in (0, 1)] == [orc.rc4_init(k) for k in keys for _ in (0, 1)]
    assert L_.BRB_TransformBatcherDisable(b.h, 1) == 1                       # connection 1 holds no buffer
    b.enable(1, keys[1], RC4)
    assert b.flush() == [want] and len(want[2]) == 15 + 30                   # framed: still RC4_MD5, the old key
    assert b.state(0, 1) == peer.wr[0]
    assert L_.BRB_TransformBatcherEnableAlgo(b.h, 0, RC4, new, len(new)) == 1   # the round is out: now it goes
    peer.rekey(0, new, RC4)
    want = peer.write(0, b"under the new key", 1)
    assert b.write(0, b"under the new key", 1) == 1 and b.flush() == [want]
    b.close()


def test_bad_arguments(brb, orc, torch_dev):
    L_ = brb.lib()
    key = b"some key"
    b = brb.TransformBatcher(4, 1 << 16, RC4, mixed=True)
    b.enable(0, key, RC4_MD5)
    before = [b.state(0, 0), b.state(0, 1)]
    assert L_.BRB_TransformBatcherEnableAlgo(b.h, 0, 3, b"other", 5) == -1
    assert L_.BRB_TransformBatcherEnableAlgo(b.h, 0, 0, b"other", 5) == -1
    ids, al = np.array([0, 1], np.uint32), np.array([RC4, 3], np.uint8)
    blob, offs, lens = brb.pack_keys([b"other", b"other"])
    assert L_.BRB_TransformBatcherEnableBatchAlgo(b.h, ids.ctypes.data, 2, al.ctypes.data, blob.ctypes.data, offs.ctypes.data,
                                                  lens.ctypes.data) == -1
    assert [b.state(0, 0), b.state(0, 1)] == before and b.state(1, 0) == ZERO
    assert b.write(0, b"abc", 1) == 1 and len(b.flush()[0][2]) == 33        # still RC4_MD5
    b.close()
    for flags in (dict(), dict(conn_lists=True)):                            # without the flag: only the batcher's algo
        b = brb.TransformBatcher(4, 1 << 16, RC4, **flags)
        assert L_.BRB_TransformBatcherEnableAlgo(b.h, 0, RC4_MD5, key, len(key)) == -1
        assert b"BRB_BATCHER_MIXED" in L_.BRB_CryptoGPU_LastError()
        al = np.array([RC4, RC4_MD5], np.uint8)
        assert L_.BRB_TransformBatcherEnableBatchAlgo(b.h, ids.ctypes.data, 2, al.ctypes.data, blob.ctypes.data,
                                                      offs.ctypes.data, lens.ctypes.data) == -1
        assert b.read(0, b"x") == -1                                         # nothing was enabled
        b.enable(0, key, RC4)                                                # its own algo is fine
        b.enable_batch([1], [key], [RC4])
        assert b.state(0, 0) == orc.rc4_init(key) and b.state(1, 1) == orc.rc4_init(key)
        b.close()
