"""BRB_RC4_MixedListBatch: streams of mixed kind (crypt, frame, open) in one launch.

Through the C ABI against the oracle's scalar calls chained on the host over each stream's list
(rc4_mixed_expect.py, which hands every stream to the list helper of its kind), bit for bit: the whole
output buffer with the sentinel bytes around and between the outputs, every valid flag (the fill of those
that belong to buffers that are not OPEN included), and all 264 bytes of every state of the table, named
or not.  The shapes are the smallest at which the kernel can go wrong: wave and workgroup edges, mixed
list lengths, every buffer length class, unaligned offsets, waves of one kind, waves with a boundary
between kinds and waves in which every lane differs from its neighbours.  Device mode unless said.
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


X = _sibling("rc4_mixed_expect")
M = _sibling("rc4_model")
L = _sibling("rc4_lists_shapes", "test_rc4_lists")     # its shapes and placement helpers, under a name of its own
G = _sibling("graph_cases")

GAP, FILL, LENS, PAYLOAD_LENS = L.GAP, L.FILL, L.LENS, L.PAYLOAD_LENS
VFILL = 0xA5                                         # valid flags before the call
STREAMS = [1, 3, 64, 65, 256, 257]
CRYPT, FRAME, OPEN = X.CRYPT, X.FRAME, X.OPEN
LAYOUTS = ["crypt", "frame", "open", "sorted", "mod3"]


@pytest.fixture(scope="module")
def torch_dev(brb):
    import torch
    assert torch.cuda.is_available(), "no HIP device visible to torch"
    assert brb.gpu_available(), brb.lib().BRB_CryptoGPU_LastError()
    return torch


def _to(torch, a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _kinds(layout, n):
    """all one kind | sorted by kind, both boundaries inside a wave (65 streams: 20 / 25 / 20) | s % 3."""
    if layout in ("crypt", "frame", "open"):
        return np.full(n, {"crypt": CRYPT, "frame": FRAME, "open": OPEN}[layout], np.uint8)
    if layout == "sorted":
        a, b = n * 20 // 65, n * 45 // 65
        return np.array([CRYPT] * a + [FRAME] * (b - a) + [OPEN] * (n - b), np.uint8)
    return (np.arange(n) % 3).astype(np.uint8)


def _wire(orc, state, lens, rng):
    """What a peer holding `state` wrote in buffers of lens[k] bytes: the frame of a random payload, below a
    header's length plain RC4 of random bytes (the reader must call it invalid and go on)."""
    out, s = [], bytes(state)
    for n in lens:
        n = int(n)
        if n < 30:
            s, w = orc.rc4_crypt(s, rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        else:
            s, w = orc.rc4md5_frame(s, rng.integers(0, 256, n - 30, dtype=np.uint8).tobytes(), int(rng.integers(0, 2**63)))
        out.append(np.frombuffer(w, np.uint8))
    return out


class Case:
    """One call's inputs with the chained oracle's results (computed once, never modified).

    mode "separate": every output in a buffer of its own, placed in another order than the inputs;
    "mirror": crypt and open outputs at their input offsets in a separate buffer (what the list calls do),
    frames behind them; "in_place": the same offsets in the input buffer itself (out = in)."""

    def __init__(self, brb, orc, n, kinds, seed, cnt=None, lens=None, states=None, index=None, mode="separate",
                 residues=True, tamper=0.15):
        self.n, self.mode = n, mode
        self.kinds = np.asarray(kinds, np.uint8)
        self.cnt = L._counts(n, seed) if cnt is None else np.asarray(cnt)
        self.first = L._first(self.cnt)
        nb = int(self.cnt.sum())
        of = np.repeat(self.kinds, self.cnt)                                 # kind per buffer
        if lens is None:
            lens = []
            for k in range(nb):
                pool = PAYLOAD_LENS if of[k] == FRAME else LENS
                ln = pool[(k * 7 + seed) % len(pool)]
                lens.append(ln + 30 if of[k] == OPEN and k % 5 != 2 else ln)  # a 7- and a 29-byte frame now and then
        self.lens = np.asarray(lens, np.uint32)
        self.index = None if index is None else np.asarray(index, np.uint32)
        self.states = brb.rc4_states(L._keys(n, seed)) if states is None else np.array(states, np.uint8)
        row = np.arange(n) if index is None else self.index
        self.offs, total = L._place(self.lens, seed, residues=residues)
        data = L._fill(self.offs, self.lens, total, seed)
        rng = np.random.default_rng([seed, 0x3E])
        for i in np.nonzero(self.kinds == OPEN)[0]:
            ks = range(int(self.first[i]), int(self.first[i + 1]))
            for k, w in zip(ks, _wire(orc, self.states[row[i]].tobytes(), self.lens[ks.start:ks.stop], rng)):
                data[int(self.offs[k]):int(self.offs[k]) + w.size] = w
                if rng.random() < tamper and w.size > 30:                    # tampered on the wire
                    data[int(self.offs[k]) + 8 + k % (w.size - 8)] ^= 1 << (k % 8)
        self.salts = np.random.default_rng([seed, 0x5A]).integers(0, 2**63, nb).astype(np.uint64)
        self.olens = (self.lens + 30 * (of == FRAME)).astype(np.uint32)
        if mode == "separate":
            order = np.random.default_rng([seed, 0x0D]).permutation(nb)
            self.ooffs, ototal = L._place(self.olens, seed + 1, order=order)
            self.out0 = np.full(ototal, FILL, np.uint8)
        else:
            fr = np.nonzero(of == FRAME)[0]
            foffs, ototal = L._place(self.olens[fr], seed + 1, base=total)
            self.ooffs = self.offs.copy()
            self.ooffs[fr] = foffs
            if mode == "in_place":
                data = np.concatenate([data, np.full(ototal - total, GAP, np.uint8)])
                self.out0 = data
            else:
                self.out0 = np.full(ototal, FILL, np.uint8)
        self.data = data
        self.valid0 = np.full(nb + 1, VFILL, np.uint8)                       # one entry past the last buffer
        self.want_st, self.want_out, self.want_valid = X.expect_mixed(orc, self.states, self.kinds, self.data, self.offs,
                                                                      self.lens, self.ooffs, self.first, self.out0,
                                                                      self.salts, self.valid0, self.index)
        for a in vars(self).values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)

    def run(self, brb, conv, **kw):
        """The call on copies made by conv (np.array: host mode; _to: device mode) -> (states, data, out, valid)."""
        st, data, valid = conv(self.states), conv(self.data), conv(self.valid0)
        out = None if self.mode == "in_place" else conv(self.out0)
        index = None if self.index is None else conv(self.index)
        res, _ = brb.rc4_mixed_list_batch(st, conv(self.kinds), data, conv(self.offs), conv(self.lens), conv(self.ooffs),
                                          conv(self.first), out=out, salts=conv(self.salts), valid=valid, state_index=index,
                                          **kw)
        return st, data, res, valid

    def check(self, got, what=""):
        st, data, out, valid = (np.asarray(x.cpu()) if hasattr(x, "cpu") else x for x in got)
        bad = np.nonzero(out != self.want_out)[0]
        assert bad.size == 0, (what, "first wrong output byte", int(bad[0]), "of", bad.size)
        assert np.array_equal(valid, self.want_valid), (what, "valid", np.nonzero(valid != self.want_valid)[0][:8])
        rows = np.nonzero((st != self.want_st).any(axis=1))[0]
        assert rows.size == 0, (what, "states differ", rows[:8])
        if self.mode != "in_place":
            assert np.array_equal(data, self.data), (what, "the inputs were written")
        of = np.repeat(self.kinds, self.cnt)
        assert (valid[:-1][of != OPEN] == VFILL).all() and valid[-1] == VFILL
        named = np.zeros(len(self.states), bool)
        named[np.arange(self.n) if self.index is None else self.index] = True
        assert np.array_equal(st[~named], self.states[~named])              # not named: every byte as it was
        idle = (np.arange(self.n) if self.index is None else self.index)[self.cnt == 0]
        assert np.array_equal(st[idle], self.states[idle])                   # no buffers: all 264 bytes as they were


_CASES = {}


def _case(brb, orc, layout, n, mode="separate"):
    key = (layout, n, mode)
    if key not in _CASES:
        _CASES[key] = Case(brb, orc, n, _kinds(layout, n), 60 + n + LAYOUTS.index(layout), mode=mode)
    return _CASES[key]


# ---- shapes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", STREAMS)
def test_mixed_shapes(brb, orc, torch_dev, n, layout):
    """Stream counts at the wave and workgroup edges, list lengths 0 / 1 / 2 / 5 mixed in one wave, streams
    without buffers at lanes 0, 63 and 64, every buffer length class, unaligned offsets, outputs placed in
    another order than the inputs; waves of one kind, waves with a kind boundary, waves of all three."""
    c = _case(brb, orc, layout, n)
    c.check(c.run(brb, lambda a: _to(torch_dev, a)), what=(layout, n))


@pytest.mark.parametrize("layout", ["crypt", "frame", "open"])
def test_all_one_kind_equals_the_list_call(brb, orc, torch_dev, layout):
    """All streams of one kind: outputs, valid flags and states equal those of the list call of that kind on
    the same inputs (GPU against GPU), and both equal the oracle."""
    torch = torch_dev
    c = _case(brb, orc, layout, 257, mode="mirror")
    to = lambda a: _to(torch, a)
    got = c.run(brb, to)
    c.check(got, layout)
    st, data, out = to(c.states), to(c.data), to(c.out0)
    offs, lens, first = to(c.offs), to(c.lens), to(c.first)
    if layout == "crypt":
        brb.rc4_crypt_list_batch(st, data, offs, lens, first, out=out)
    elif layout == "frame":
        brb.rc4md5_frame_list_batch(st, data, offs, lens, to(c.salts), out, to(c.ooffs), first)
    else:
        _, valid = brb.rc4md5_open_list_batch(st, data, offs, lens, first, out=out)
        assert torch.equal(valid, got[3][:-1])
    assert torch.equal(st, got[0]) and torch.equal(out, got[2])


# ---- state index ---------------------------------------------------------------------------------
def test_state_index_permutation(brb, orc, torch_dev):
    n = 130
    perm = np.random.default_rng(0x1D).permutation(n)
    c = Case(brb, orc, n, _kinds("mod3", n), 71, index=perm)
    c.check(c.run(brb, lambda a: _to(torch_dev, a)))


def test_state_index_batcher_layout(brb, orc, torch_dev):
    """The transform batcher's table: read states, then write states.  One call opens what every connection
    read (state c) and frames what it writes (state C + c); keyed alike, the two states of a connection
    end different."""
    C = 70
    half = brb.rc4_states(L._keys(C, 72))
    states = np.concatenate([half, half])
    kinds = np.array([OPEN] * C + [FRAME] * C, np.uint8)
    index = np.concatenate([np.arange(C), C + np.arange(C)])
    c = Case(brb, orc, 2 * C, kinds, 72, states=states, index=index)
    c.check(c.run(brb, lambda a: _to(torch_dev, a)))
    both = c.cnt[:C].astype(bool) & c.cnt[C:].astype(bool)
    assert both.any() and (c.want_st[:C][both] != c.want_st[C:][both]).any(axis=1).all()


def test_state_index_sparse(brb, orc, torch_dev):
    """66 streams name every seventh state of a table of 470: the states not named, and so every byte
    between the named ones, keep their values (check() compares the whole table)."""
    n, table = 66, 470
    states = brb.rc4_states(L._keys(table, 73))
    index = (np.arange(n) * 7 + 3)[::-1].copy()
    c = Case(brb, orc, n, _kinds("sorted", n), 73, states=states, index=index)
    c.check(c.run(brb, lambda a: _to(torch_dev, a)))


# ---- tails followed by whole blocks, on near-index states ------------------------------------------
@pytest.mark.parametrize("cls", ["class_b", "class_d"])
def test_near_index_states_in_waves_of_three_kinds(brb, orc, torch_dev, cls):
    """States of rc4_model.class_b / class_d (index2 = index1 + d, low-entropy S) under kind = s % 3: a buffer
    whose length is no multiple of 4 is followed by whole blocks on one generator, in all three bodies of
    one wave.  The first buffers are 0..3 bytes long, so the near-index state itself sits at a boundary."""
    states, _ = getattr(M, cls)()
    k = np.arange(len(states))
    states = states[(k >> 3) % 8 == 0]                # every d = 0..7 for every eighth index1: 256 states
    n = len(states)
    kinds = _kinds("mod3", n)
    lens = []
    for i in range(n):
        grow = 30 if kinds[i] == OPEN else 0
        lens += [i % 4 + grow, 64 + (i >> 2) % 4 + grow, 1 + i % 3, 67 + grow, 130 + grow]
    c = Case(brb, orc, n, kinds, 0xB0 + len(cls), cnt=[5] * n, lens=lens, states=states, residues=False)
    c.check(c.run(brb, lambda a: _to(torch_dev, a)), cls)


# ---- in place ------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["sorted", "mod3"])
def test_crypt_and_open_in_place_beside_frame(brb, orc, torch_dev, layout):
    """out == in: crypt and open buffers are overwritten where they lie, the frames go behind them in the
    same buffer; the bytes between buffers keep their values."""
    c = _case(brb, orc, layout, 65, mode="in_place")
    got = c.run(brb, lambda a: _to(torch_dev, a))
    assert got[2] is got[1]
    c.check(got, layout)
    c.check(c.run(brb, np.array), layout + ", host mode")


# ---- open: verdicts per buffer -----------------------------------------------------------------------
def test_open_verdicts_are_per_buffer(brb, orc, torch_dev):
    """In a call of all three kinds: a corrupted tag byte, a corrupted digest bit and a frame under 30 bytes
    in the middle of a list invalidate that buffer only -- the stream goes on, its later buffers are valid
    -- and the valid entries of crypt and frame buffers keep their fill."""
    n = 66
    kinds = _kinds("mod3", n)
    cnt = np.full(n, 4)
    lens = np.array([30 + 40, 30 + 1, 30 + 100, 30 + 64] * n, np.uint32)
    opens = np.nonzero(kinds == OPEN)[0]
    for j, i in enumerate(opens):
        if j % 3 == 2:
            lens[4 * i + 1] = 7 if j % 2 else 29
    c0 = Case(brb, orc, n, kinds, 9, cnt=cnt, lens=lens, tamper=0.0)
    data = c0.data.copy()
    want_valid = c0.want_valid.copy()
    is_open = np.repeat(kinds, cnt) == OPEN
    assert np.array_equal(want_valid[:-1][is_open], c0.lens[is_open] >= 30)  # untampered: valid iff a whole frame
    for j, i in enumerate(opens):
        if j % 3 == 0:                               # a digest bit of buffer 1
            data[int(c0.offs[4 * i + 1]) + 13 + j % 16] ^= 1 << (j % 8)
            want_valid[4 * i + 1] = 0
        elif j % 3 == 1:                             # a tag byte of buffer 2
            data[int(c0.offs[4 * i + 2]) + 8 + j % 5] ^= 0x20
            want_valid[4 * i + 2] = 0
    st, out, valid = X.expect_mixed(orc, c0.states, kinds, data, c0.offs, c0.lens, c0.ooffs, c0.first, c0.out0, c0.salts,
                                    c0.valid0)
    assert np.array_equal(valid, want_valid)         # the oracle agrees with the construction
    for i in opens:
        assert valid[4 * i] == 1 and valid[4 * i + 3] == 1                   # the stream goes on
    to = lambda a: _to(torch_dev, a)
    g_st, g_valid = to(c0.states), to(c0.valid0)
    g_out, _ = brb.rc4_mixed_list_batch(g_st, to(kinds), to(data), to(c0.offs), to(c0.lens), to(c0.ooffs), to(c0.first),
                                        out=to(c0.out0), salts=to(c0.salts), valid=g_valid)
    assert np.array_equal(g_valid.cpu().numpy(), want_valid)
    assert np.array_equal(g_out.cpu().numpy(), out) and np.array_equal(g_st.cpu().numpy(), st)


def test_frame_then_open_round_trip(brb, orc, torch_dev):
    """FRAME streams in one call; the frames as OPEN streams of a second call on peer states keyed alike:
    every valid is 1, the payloads are restored, and the peers' read states equal the write states."""
    n = 65
    c = _case(brb, orc, "frame", n)
    to = lambda a: _to(torch_dev, a)
    wst, _, frames, _ = c.run(brb, to)
    rst = to(c.states)
    flen = (c.lens + 30).astype(np.uint32)
    doffs, dtotal = L._place(flen, 5)
    valid = to(np.full(len(flen), VFILL, np.uint8))
    dec, _ = brb.rc4_mixed_list_batch(rst, to(np.full(n, OPEN, np.uint8)), frames, to(c.ooffs), to(flen), to(doffs),
                                      to(c.first), out=to(np.full(dtotal, FILL, np.uint8)), valid=valid)
    assert (valid.cpu().numpy() == 1).all() and torch_dev.equal(rst, wst)
    dec = dec.cpu().numpy()
    for o, ln, d in zip(c.offs.tolist(), c.lens.tolist(), doffs.tolist()):
        assert np.array_equal(dec[d + 30:d + 30 + ln], c.data[o:o + ln])
    assert (dec[~L._covered(doffs, flen, dec.size)] == FILL).all()


# ---- modes ------------------------------------------------------------------------------------
def test_host_mode_equals_device_mode(brb, orc, torch_dev):
    """The 65-stream case sorted 20 / 25 / 20 through host mode: states, out and valid equal the device
    mode's (and the oracle's)."""
    c = _case(brb, orc, "sorted", 65)
    dev = c.run(brb, lambda a: _to(torch_dev, a))
    host = c.run(brb, np.array)
    c.check(host, "host mode")
    for h, d in zip(host, dev):
        assert np.array_equal(h, d.cpu().numpy())


def test_host_mode_with_a_sparse_index(brb, orc, torch_dev):
    """Host mode stages the named states densely: those not named are neither read nor written."""
    n, table = 66, 200
    states = brb.rc4_states(L._keys(table, 74))
    c = Case(brb, orc, n, _kinds("mod3", n), 74, states=states, index=np.arange(n) * 3 + 1)
    c.check(c.run(brb, np.array), "host mode, sparse index")


def test_device_mode_on_a_stream_and_async(brb, orc, torch_dev):
    torch = torch_dev
    c = _case(brb, orc, "mod3", 65)
    s = torch.cuda.Stream()
    to = lambda a: _to(torch, a)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        got = c.run(brb, to, stream=s.cuda_stream, async_=True)
    s.synchronize()
    brb.async_fault_check()
    c.check(got, what="async on a non-default stream")


# ---- graph capture -----------------------------------------------------------------------------------
class MixedGraph(G.Case):
    """One captured mixed call: 66 streams of 0..4 buffers, kind = (s + replay) % 3, so every wave holds all
    three kinds and every stream changes kind from replay to replay; lists, lengths and placement are
    redrawn for every replay, the states carried -- replay k leaves what the oracle leaves applied k times."""
    carried = ("states",)
    N, MOST = 66, 4

    def __init__(self, brb, orc):
        self.brb, self.orc = brb, orc
        self.cap = self.N * self.MOST
        self.size = 4 + self.cap * (max(G.RC4_LENS) + 33) + 8
        self.seed = 0x6D78

    def inputs(self, r, host):
        g = G.rng_of(self.seed, r)
        cnt = g.integers(0, self.MOST + 1, self.N)
        cnt[[(7 * (r + 2)) % self.N, 64]] = 0                               # streams with no buffer
        cnt[[0, 63, 65]] = (self.MOST, 1, 2)
        nb = int(cnt.sum())
        kinds = ((np.arange(self.N) + r + 1) % 3).astype(np.uint8)
        of = np.repeat(kinds, cnt)
        lens = g.choice(G.RC4_LENS, nb).astype(np.uint32)
        first = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
        offs, end = G.place(lens, g, base=(r + 1) & 3)
        ooffs, oend = G.place(lens + 30 * (of == FRAME), g, base=(r + 2) & 3)
        assert end <= self.size and oend <= self.size
        states = host["states"] if host else G.guarded_states(self.brb, self.N, self.seed + r)
        data = G.rand_bytes(g, self.size)
        for i in np.flatnonzero(kinds == OPEN):
            s = states[1 + i].tobytes()
            for k in range(int(first[i]), int(first[i + 1])):
                s, w = G.wire_buffer(self.orc, g, s, int(lens[k]))
                data[int(offs[k]):int(offs[k]) + len(w)] = np.frombuffer(w, np.uint8)
        opens = np.flatnonzero(of == OPEN)
        G.tamper(g, data, offs[opens], lens[opens])
        d = {"kinds": kinds, "offs": G.padded(offs, self.cap + 1, np.uint64), "lens": G.padded(lens, self.cap + 1, np.uint32),
             "ooffs": G.padded(ooffs, self.cap + 1, np.uint64), "first": first, "data": data,
             "salts": G.padded(g.integers(0, 1 << 63, nb, dtype=np.uint64), self.cap + 1, np.uint64),
             "out": np.full(self.size, G.FILL, np.uint8), "valid": G.guarded(self.cap + 1)}
        if not host:
            d["states"] = states
        return d

    def call(self, t, s):
        self.brb.rc4_mixed_list_batch(t["states"][1:self.N + 1], t["kinds"], t["data"], t["offs"], t["lens"], t["ooffs"],
                                      t["first"], out=t["out"], salts=t["salts"], valid=t["valid"][1:-1], stream=s,
                                      async_=True)

    def expect(self, h):
        st, valid = h["states"].copy(), h["valid"].copy()
        inner, out, ok = X.expect_mixed(self.orc, st[1:self.N + 1], h["kinds"], h["data"], h["offs"], h["lens"], h["ooffs"],
                                        h["first"], h["out"], h["salts"], valid[1:-1])
        st[1:self.N + 1], valid[1:-1] = inner, ok
        return {"states": st, "out": out, "valid": valid}


def test_graph_capture_and_replay(brb, orc, torch_dev):
    """One capture, three replays (graph_cases.run_case, as it stands)."""
    G.run_case(brb, torch_dev, MixedGraph(brb, orc))


# ---- fuzz ----------------------------------------------------------------------------------------
def test_fuzz(brb, orc, torch_dev):
    """300 streams, random kinds, random lists, random lengths up to 1500."""
    rng = np.random.default_rng(0xF0221)
    n = 300
    kinds = rng.integers(0, 3, n).astype(np.uint8)
    cnt = rng.integers(0, 7, n)
    lens = rng.integers(0, 201, int(cnt.sum()))
    lens[rng.random(lens.size) < 0.03] = 1500
    lens[rng.random(lens.size) < 0.02] = rng.integers(1400, 1501)
    of = np.repeat(kinds, cnt)
    lens = np.where((of == OPEN) & (rng.random(lens.size) < 0.8), np.minimum(lens + 30, 1500), lens)
    c = Case(brb, orc, n, kinds, 0xF1, cnt=cnt, lens=lens, residues=False)
    c.check(c.run(brb, lambda a: _to(torch_dev, a)), what="device")
    c.check(c.run(brb, np.array), what="host")
