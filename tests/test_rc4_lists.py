"""RC4 batch calls with a buffer list per stream, and the transform batcher's connection-list rounds.

BRB_RC4_CryptListBatch / BRB_RC4MD5_FrameListBatch / BRB_RC4MD5_OpenListBatch through the C ABI against
the oracle chained on the host over each stream's list (rc4_lists_expect.py), bit for bit: outputs,
valid flags, every sentinel byte around the buffers and all 264 bytes of every state.  The shapes are
the smallest at which the kernels can go wrong (wave and workgroup edges, mixed list lengths, tails
followed by whole blocks, starts at every dword and line residue), not the workload's shapes.
"""
import importlib.util
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _sibling(name):
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
        sys.modules[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[name])
    return sys.modules[name]


E = _sibling("rc4_lists_expect")
M = _sibling("rc4_model")

GAP, FILL = 0xA5, 0x5A                   # sentinels: between the input buffers / in a separate output
LENS = [0, 1, 3, 4, 29, 30, 31, 32, 33, 63, 64, 65, 127, 128, 1500]
PAYLOAD_LENS = LENS + [2, 55, 56]        # payload bytes 0..1 live in header chunk 7; MD5 padding spills at 56
STREAMS = [1, 64, 65, 256, 257]          # wave and workgroup edges
KINDS = ["crypt", "frame", "open"]


@pytest.fixture(scope="module")
def torch_dev(brb):
    import torch
    assert torch.cuda.is_available(), "no HIP device visible to torch"
    assert brb.gpu_available(), brb.lib().BRB_CryptoGPU_LastError()
    return torch


@pytest.fixture(params=[0, 1], ids=["lane", "coop"])
def coop(request, brb):
    """Test option rc4_list_coop: the crypt list kernel's per-lane / cooperative (default) block loads."""
    with brb.TestOption("rc4_list_coop", request.param):
        yield request.param


VARIANTS = [("crypt", 0), ("crypt", 1), ("frame", 0), ("open", 0)]


@pytest.fixture(params=VARIANTS, ids=["crypt-lane", "crypt-coop", "frame", "open"])
def kind(request, brb):
    """The three calls, the crypt call on both load forms of its kernel."""
    with brb.TestOption("rc4_list_coop", request.param[1]):
        yield request.param[0]


def _to(torch, a):
    return torch.from_numpy(np.array(a)).cuda()


def _keys(n, seed):
    rng = np.random.default_rng([seed, 0x4B])
    return [rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes() for _ in range(n)]


def _counts(n, seed):
    """List lengths 0, 1, 2, 5 mixed; streams without buffers at lanes 0, 63 and 64."""
    cnt = np.random.default_rng([seed, 0xC]).choice([0, 1, 2, 5], n)
    if n == 1:
        cnt[0] = 5
    else:
        for z in (0, 63, 64):
            if z < n:
                cnt[z] = 0
        cnt[1 % n] = 5
    return cnt


def _first(cnt):
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)


def _place(lens, seed, extra=0, base=0, residues=True, order=None):
    """Offsets of ranges of lens[k] + extra bytes, placed in `order` (default: index order) with seeded gaps of
    0..3 bytes (mostly 0: neighbours share dwords and sectors); with `residues`, every third range starts at
    60 + j mod 64 for j cycling through 0..7, which also covers every offset mod 4.  -> (offs, total) with 8
    bytes past the last range."""
    rng = np.random.default_rng([seed, 0x9A])
    offs = np.zeros(len(lens), np.uint64)
    pos = base
    for t, k in enumerate(range(len(lens)) if order is None else order):
        pos += int(rng.choice([0, 0, 0, 1, 2, 3]))
        if residues and t % 3 == 0:
            pos += (60 + (t // 3) % 8 - pos) % 64
        offs[k] = pos
        pos += int(lens[k]) + extra
    return offs, pos + 8


def _covered(offs, lens, total, extra=0):
    m = np.zeros(total, bool)
    for o, n in zip(offs.tolist(), lens.tolist()):
        m[o:o + n + extra] = True
    return m


def _fill(offs, lens, total, seed):
    """`total` bytes: seeded random bytes in the buffers, GAP everywhere else."""
    buf = np.full(total, GAP, np.uint8)
    m = _covered(offs, lens, total)
    buf[m] = np.random.default_rng([seed, 0xF1]).integers(0, 256, int(m.sum()), dtype=np.uint8)
    return buf


def _wire(orc, keys, cnt, lens, offs, total, seed, short=()):
    """What a peer wrote: buffer k of stream i is the RC4+MD5 frame of a random payload of lens[k] - 30 bytes
    under the stream's running write state; a buffer shorter than 30 bytes, or listed in `short`, is plain
    RC4 of random bytes (no frame: the reader must report it invalid and go on)."""
    rng = np.random.default_rng([seed, 0x3E])
    buf = np.full(total, GAP, np.uint8)
    k = 0
    for i, c in enumerate(cnt.tolist()):
        s = orc.rc4_init(keys[i])
        for _ in range(c):
            n, o = int(lens[k]), int(offs[k])
            if n < 30 or k in short:
                s, w = orc.rc4_crypt(s, rng.integers(0, 256, n, dtype=np.uint8).tobytes())
            else:
                s, w = orc.rc4md5_frame(s, rng.integers(0, 256, n - 30, dtype=np.uint8).tobytes(), int(rng.integers(0, 2**63)))
            buf[o:o + n] = np.frombuffer(w, np.uint8)
            k += 1
    return buf


class Case:
    """One call's inputs with the chained oracle's results (computed once, never modified)."""

    def __init__(self, brb, orc, kind, n, seed, cnt=None, lens=None, states=None, **place):
        self.kind, self.n = kind, n
        frame_order = place.pop("frame_order", "shuffled")
        self.cnt = _counts(n, seed) if cnt is None else np.asarray(cnt)
        nb = int(self.cnt.sum())
        pool = PAYLOAD_LENS if kind == "frame" else LENS
        if lens is None:
            lens = [pool[(k * 7 + seed) % len(pool)] for k in range(nb)]
            if kind == "open":           # frames: header + payload, with a 7- and a 29-byte frame now and then
                lens = [n_ if k % 5 == 2 else n_ + 30 for k, n_ in enumerate(lens)]
        self.lens = np.asarray(lens, np.uint32)
        self.first = _first(self.cnt)
        keys = _keys(n, seed)
        self.states = brb.rc4_states(keys) if states is None else np.array(states, np.uint8)
        self.offs, total = _place(self.lens, seed, **place)
        if kind == "open":
            self.data = _wire(orc, keys, self.cnt, self.lens, self.offs, total, seed)
            flip = np.random.default_rng([seed, 0x7A]).random(nb) < 0.15      # tampered on the wire
            for k in np.nonzero(flip & (self.lens > 30))[0]:
                self.data[int(self.offs[k]) + 8 + int(k) % (int(self.lens[k]) - 8)] ^= 1 << (int(k) % 8)
        else:
            self.data = _fill(self.offs, self.lens, total, seed)
        self.out0 = np.full(total, FILL, np.uint8)
        if kind == "crypt":
            self.want_st, self.want = E.expect_crypt(orc, self.states, self.data, self.offs, self.lens, self.first)
            _, self.want_out = E.expect_crypt(orc, self.states, self.data, self.offs, self.lens, self.first, out=self.out0)
        elif kind == "open":
            self.want_st, self.want, self.want_valid = E.expect_open(orc, self.states, self.data, self.offs, self.lens,
                                                                     self.first)
            self.want_out = E.expect_open(orc, self.states, self.data, self.offs, self.lens, self.first, out=self.out0)[1]
        else:
            self.salts = np.random.default_rng([seed, 0x5A]).integers(0, 2**63, nb).astype(np.uint64)
            # frames in their own buffer, placed in another order than the payloads
            order = np.random.default_rng([seed, 0x0D]).permutation(nb) if frame_order == "shuffled" else None
            self.foffs, ftotal = _place(self.lens, seed + 1, extra=30, order=order)
            self.out0 = np.full(ftotal, FILL, np.uint8)
            self.want_st, self.want_out = E.expect_frame(orc, self.states, self.data, self.offs, self.lens, self.salts,
                                                         self.out0, self.foffs, self.first)
        for a in vars(self).values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)

    def run(self, brb, conv, in_place=False, **kw):
        """The list call on copies made by conv (np.array: host mode; _to: device mode) -> (states, out, valid)."""
        st, data = conv(self.states), conv(self.data)
        offs, lens, first = conv(self.offs), conv(self.lens), conv(self.first)
        if self.kind == "crypt":
            out = brb.rc4_crypt_list_batch(st, data, offs, lens, first, out=None if in_place else conv(self.out0), **kw)
            return st, out, None
        if self.kind == "open":
            out, valid = brb.rc4md5_open_list_batch(st, data, offs, lens, first, out=None if in_place else conv(self.out0),
                                                    **kw)
            return st, out, valid
        out = brb.rc4md5_frame_list_batch(st, data, offs, lens, conv(self.salts), conv(self.out0), conv(self.foffs), first,
                                          **kw)
        return st, out, None

    def check(self, got, in_place=False, what=""):
        st, out, valid = (np.asarray(x.cpu()) if hasattr(x, "cpu") else x for x in got)
        want = self.want if in_place and self.kind != "frame" else self.want_out
        bad = np.nonzero(out != want)[0]
        assert bad.size == 0, (what, self.kind, "first wrong byte", int(bad[0]), "of", bad.size)
        if self.kind == "open":
            assert np.array_equal(valid, self.want_valid), (what, np.nonzero(valid != self.want_valid)[0][:8])
        rows = np.nonzero((st != self.want_st).any(axis=1))[0]
        assert rows.size == 0, (what, self.kind, "states differ", rows[:8])
        idle = self.cnt == 0
        assert np.array_equal(st[idle], self.states[idle])          # no buffers: all 264 bytes as they were


_CASES = {}


def _case(brb, orc, kind, n, seed, **kw):
    key = (kind, n, seed, tuple(sorted(kw)))
    if key not in _CASES:
        _CASES[key] = Case(brb, orc, kind, n, seed, **kw)
    return _CASES[key]


# ---- shapes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", STREAMS)
def test_list_shapes(brb, orc, torch_dev, kind, n):
    """Stream counts at the wave and workgroup edges, list lengths 0 / 1 / 2 / 5 mixed in one wave, every
    buffer length class, starts at every offset mod 4 and at 60..67 mod 64, neighbours packed back to back;
    device and host mode, in place and with a separate output whose other bytes must survive."""
    c = _case(brb, orc, kind, n, 40 + n)
    to = lambda a: _to(torch_dev, a)
    c.check(c.run(brb, to), what="device, separate out")
    c.check(c.run(brb, np.array), what="host, separate out")
    if kind != "frame":
        c.check(c.run(brb, to, in_place=True), True, "device, in place")
        c.check(c.run(brb, np.array, in_place=True), True, "host, in place")


def test_lists_of_empty_buffers(brb, orc, torch_dev, kind):
    """Every buffer empty (crypt: nothing written, the state unchanged; frame: a 30-byte frame; open: a
    0-byte frame, invalid), offsets that are no memory at all for the empty inputs."""
    n = 70
    c = Case(brb, orc, kind, n, 7, cnt=[3] * n, lens=[0] * (3 * n), residues=False)
    far = np.full(3 * n, (1 << 63) + 4097, np.uint64)
    st = _to(torch_dev, c.states)
    first, lens = _to(torch_dev, c.first), _to(torch_dev, c.lens)
    data = _to(torch_dev, c.data)
    if kind == "crypt":
        brb.rc4_crypt_list_batch(st, data, _to(torch_dev, far), lens, first)
        assert np.array_equal(data.cpu().numpy(), c.data) and np.array_equal(st.cpu().numpy(), c.states)
    elif kind == "open":
        _, valid = brb.rc4md5_open_list_batch(st, data, _to(torch_dev, far), lens, first)
        assert not valid.cpu().numpy().any()
        assert np.array_equal(data.cpu().numpy(), c.data) and np.array_equal(st.cpu().numpy(), c.states)
    else:
        out = brb.rc4md5_frame_list_batch(st, data, _to(torch_dev, far), lens, _to(torch_dev, c.salts), _to(torch_dev, c.out0),
                                          _to(torch_dev, c.foffs), first)
        c.check((st, out, None))


# ---- tails followed by whole blocks, on near-index states ------------------------------------------
def _hazard_states(cls):
    st, _ = cls()
    k = np.arange(len(st))
    return st[(k >> 3) % 4 == 0]                    # every d = 0..7 for every fourth index1: 512 states


@pytest.mark.parametrize("cls", ["class_b", "class_d"])
def test_tail_then_blocks_on_near_index_states(brb, orc, torch_dev, cls, coop):
    """A buffer whose length is no multiple of 4 followed by another buffer: next_n(< 4) and then words() on
    one generator, which no single-buffer kernel does.  States of rc4_model.class_b / class_d (index2 =
    index1 + d, low-entropy S, so j stays near i for many bytes): the first buffers are 0..3 bytes long, so
    the near-index state itself sits at a buffer boundary, and 1..3-byte tails sit in front of 64-byte runs."""
    states = _hazard_states(getattr(M, cls))
    n = len(states)
    cnt = [6] * n
    lens = []
    for i in range(n):
        lens += [i % 4, 64 + (i >> 2) % 4, 1 + i % 3, 67, (i >> 4) % 4, 130]
    c = Case(brb, orc, "crypt", n, 0xB0 + len(cls), cnt=cnt, lens=lens, states=states, residues=False)
    c.check(c.run(brb, lambda a: _to(torch_dev, a), in_place=True), True, cls)


def test_frame_and_open_on_near_index_states(brb, orc, torch_dev):
    """The same states through the frame and open walks: a frame's tail (next_n) is followed by the next
    frame's header (next4) and first run (words)."""
    states = _hazard_states(M.class_d)[::2]
    n = len(states)
    lens = []
    for i in range(n):
        lens += [i % 4, 33 + i % 5, 2, 56 + i % 3]
    to = lambda a: _to(torch_dev, a)
    f = Case(brb, orc, "frame", n, 0xD1, cnt=[4] * n, lens=lens, states=states, residues=False)
    st, frames, _ = f.run(brb, to)
    f.check((st, frames, None))
    # open what was framed, with the same start states: every frame valid, the states end equal
    rst = to(states)
    flen = to((f.lens + 30).astype(np.uint32))
    out, valid = brb.rc4md5_open_list_batch(rst, frames, to(f.foffs), flen, to(f.first))
    assert valid.cpu().numpy().all()
    assert np.array_equal(rst.cpu().numpy(), f.want_st)
    want_st, dec, ok = E.expect_open(orc, states, f.want_out, f.foffs, f.lens + 30, f.first)
    assert np.array_equal(out.cpu().numpy(), dec) and ok.all() and np.array_equal(want_st, f.want_st)


# ---- split invariance and equivalence with the single-buffer calls -----------------------------------
def test_crypt_split_invariance(brb, torch_dev, coop):
    """One stream's contiguous bytes cut into a list at arbitrary points: the same bytes and state as
    BRB_RC4_CryptBatch on the whole (GPU against GPU)."""
    rng = np.random.default_rng(0x5911)
    n = 130
    whole = rng.choice([0, 1, 5, 63, 64, 65, 200, 777, 1500], n).astype(np.uint32)
    offs, total = _place(whole, 3, residues=False)
    data = _fill(offs, whole, total, 3)
    states = brb.rc4_states(_keys(n, 3))
    boffs, blens, cnt = [], [], []
    for o, ln in zip(offs.tolist(), whole.tolist()):
        cuts = np.sort(rng.integers(0, ln + 1, int(rng.integers(0, 6))))
        edges = [0] + cuts.tolist() + [ln]
        cnt.append(len(edges) - 1)
        boffs += [o + e for e in edges[:-1]]
        blens += np.diff(edges).tolist()
    to = lambda a: _to(torch_dev, a)
    a_st, a = to(states), to(data)
    brb.rc4_crypt_batch(a_st, a, to(offs), to(whole))
    b_st, b = to(states), to(data)
    brb.rc4_crypt_list_batch(b_st, b, to(np.array(boffs, np.uint64)), to(np.array(blens, np.uint32)), to(_first(cnt)))
    assert torch_dev.equal(a, b) and torch_dev.equal(a_st, b_st)


@pytest.mark.parametrize("pair", [1, 0], ids=["pair", "single"])
@pytest.mark.parametrize("kind", KINDS)
def test_list_call_equals_consecutive_single_buffer_calls(brb, orc, torch_dev, kind, pair):
    """One list call == k calls of the existing single-buffer entry point over the buffers of rank 0, 1, ...
    (GPU against GPU), and both equal the oracle.  The single-buffer calls on both of their routes (test
    options rc4_pair / rc4md5_pair): the wave pairs, and the lone kernels, which call the list kernels'
    per-buffer body once (rc4_block.h).  With rc4_pair = 0 and rc4_sector unset the crypt case runs the lone
    kernel the launcher picks (the sector sink, as the list kernel); rc4_crypt_kernel<false> on the same body
    is held by test_rc4.py::test_rc4_sector_sink_ragged."""
    torch = torch_dev
    c = _case(brb, orc, kind, 257, 40 + 257)
    to = lambda a: _to(torch, a)
    st, data, out = to(c.states), to(c.data), to(c.out0)
    valid = torch.zeros(len(c.offs), dtype=torch.uint8, device="cuda")
    for r in range(int(c.cnt.max())):
        who = np.nonzero(c.cnt > r)[0]
        kn = (c.first[who].astype(np.int64) + r)
        ks = torch.from_numpy(kn).cuda()
        sub = st[torch.from_numpy(who).cuda()].contiguous()
        o_r, l_r = to(c.offs[kn]), to(c.lens[kn])
        with brb.TestOption("rc4_pair" if kind == "crypt" else "rc4md5_pair", pair):
            if kind == "crypt":
                brb.rc4_crypt_batch(sub, data, o_r, l_r, out=out)
            elif kind == "open":
                _, v = brb.rc4md5_open_batch(sub, data, o_r, l_r, out=out)
                valid[ks] = v
            else:
                brb.rc4md5_frame_batch(sub, data, o_r, l_r, to(c.salts[kn]), out, to(c.foffs[kn]))
        st[torch.from_numpy(who).cuda()] = sub
    got = c.run(brb, to)
    assert torch.equal(got[0], st) and torch.equal(got[1], out)
    if kind == "open":
        assert torch.equal(got[2], valid)
    c.check(got)


def test_one_buffer_per_stream_equals_existing_calls(brb, orc, torch_dev, coop):
    torch = torch_dev
    n = 130
    c = Case(brb, orc, "crypt", n, 77, cnt=[1] * n)
    to = lambda a: _to(torch, a)
    a_st, a = to(c.states), to(c.data)
    brb.rc4_crypt_batch(a_st, a, to(c.offs), to(c.lens))
    got = c.run(brb, to, in_place=True)
    assert torch.equal(got[0], a_st) and torch.equal(got[1], a)
    c.check(got, True)


# ---- open: verdicts per buffer -----------------------------------------------------------------------
def test_open_verdicts_are_per_buffer(brb, orc, torch_dev):
    """A corrupted digest bit or tag byte in a middle buffer invalidates that buffer only; a 7-byte and a
    29-byte frame mid-list are decrypted and invalid; the stream's later buffers are still valid."""
    n = 66
    cnt = np.full(n, 4)
    lens = np.array([30 + 40, 30 + 1, 30 + 100, 30 + 64] * n, np.uint32)
    short = {}
    for i in range(n):
        if i % 4 == 2:
            lens[4 * i + 1] = 7
        if i % 4 == 3:
            lens[4 * i + 2] = 29
    keys = _keys(n, 9)
    offs, total = _place(lens, 9)
    data = _wire(orc, keys, cnt, lens, offs, total, 9, short)
    want_valid = np.ones(4 * n, np.uint8)
    for i in range(n):
        if i % 4 == 0:                               # a digest bit of buffer 1
            data[int(offs[4 * i + 1]) + 13 + i % 16] ^= 1 << (i % 8)
            want_valid[4 * i + 1] = 0
        elif i % 4 == 1:                             # a tag byte of buffer 2
            data[int(offs[4 * i + 2]) + 8 + i % 5] ^= 0x20
            want_valid[4 * i + 2] = 0
        elif i % 4 == 2:
            want_valid[4 * i + 1] = 0
        else:
            want_valid[4 * i + 2] = 0
    states = brb.rc4_states(keys)
    first = _first(cnt)
    want_st, want, ok = E.expect_open(orc, states, data, offs, lens, first)
    assert np.array_equal(ok, want_valid)            # the oracle agrees with the construction
    to = lambda a: _to(torch_dev, a)
    st = to(states)
    out, valid = brb.rc4md5_open_list_batch(st, to(data), to(offs), to(lens), to(first))
    assert np.array_equal(valid.cpu().numpy(), want_valid)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(st.cpu().numpy(), want_st)


def test_frame_then_open_round_trip(brb, orc, torch_dev):
    """Frames written by the list call, opened by the list call with equal keys: every valid is 1, the
    payloads are restored, and the write state after framing equals the read state after opening."""
    c = _case(brb, orc, "frame", 65, 40 + 65)
    to = lambda a: _to(torch_dev, a)
    wst, frames, _ = c.run(brb, to)
    rst = to(c.states)
    out, valid = brb.rc4md5_open_list_batch(rst, frames, to(c.foffs), to((c.lens + 30).astype(np.uint32)), to(c.first))
    assert valid.cpu().numpy().all() and torch_dev.equal(rst, wst)
    dec = out.cpu().numpy()
    for o, n, f in zip(c.offs.tolist(), c.lens.tolist(), c.foffs.tolist()):
        assert np.array_equal(dec[f + 30:f + 30 + n], c.data[o:o + n])
    assert (dec[~_covered(c.foffs, c.lens, dec.size, 30)] == FILL).all()


# ---- modes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_device_mode_on_a_stream_and_async(brb, orc, torch_dev, kind):
    torch = torch_dev
    c = _case(brb, orc, kind, 65, 40 + 65)
    s = torch.cuda.Stream()
    to = lambda a: _to(torch, a)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        got = c.run(brb, to, stream=s.cuda_stream)
    c.check(got, what="non-default stream")
    with torch.cuda.stream(s):
        got = c.run(brb, to, stream=s.cuda_stream, async_=True)
    s.synchronize()
    brb.async_fault_check()
    c.check(got, what="async")


@pytest.mark.parametrize("interleaved", [False, True], ids=["disjoint", "interleaved"])
@pytest.mark.parametrize("kind", KINDS)
def test_all_devices(brb, orc, torch_dev, kind, interleaved):
    """BRB_BATCH_ALL_DEVICES in three parts: buffers placed stream by stream give the parts disjoint spans
    (split); placed in a random order the spans interleave (no split).  The same results either way."""
    n = 65
    cnt = _counts(n, 5)
    nb = int(cnt.sum())
    order = np.random.default_rng(5).permutation(nb) if interleaved else None
    c = Case(brb, orc, kind, n, 50 + interleaved, cnt=cnt, order=order, frame_order="shuffled" if interleaved else None)
    with brb.TestOption("devices", 3):
        c.check(c.run(brb, np.array, all_devices=True), what="all devices")
        if kind != "frame":
            c.check(c.run(brb, np.array, in_place=True, all_devices=True), True, "all devices, in place")


# ---- fuzz ----------------------------------------------------------------------------------------
def test_fuzz(brb, orc, torch_dev, kind):
    rng = np.random.default_rng(0xF022)
    n = 300
    cnt = rng.integers(0, 7, n)
    lens = rng.integers(0, 201, int(cnt.sum()))
    lens[rng.random(lens.size) < 0.03] = 1500
    if kind == "open":
        lens = np.where(rng.random(lens.size) < 0.8, lens + 30, lens)
    c = Case(brb, orc, kind, n, 0xF0, cnt=cnt, lens=lens, residues=False)
    to = lambda a: _to(torch_dev, a)
    c.check(c.run(brb, to), what="device")
    c.check(c.run(brb, np.array, in_place=True), True, "host")


# ---- the transform batcher with BRB_BATCHER_CONN_LISTS -----------------------------------------------
def _traffic(orc, algo, seed, C=40, rounds=3):
    """Three rounds of an event loop: per round every connection gets 0..5 buffers in each direction, reads
    and writes interleaved.  -> per round a list of (conn, op, bytes, salt) and the oracle's results
    [(conn, op, out, valid)], and after each round the oracle's states."""
    rng = np.random.default_rng([seed, algo])
    keys = [rng.integers(0, 256, int(rng.integers(4, 32)), dtype=np.uint8).tobytes() for _ in range(C)]
    ours = [[orc.rc4_init(k) for k in keys] for _ in range(2)]
    peer_w = [orc.rc4_init(k) for k in keys]
    out = []
    for _ in range(rounds):
        subs, expect = [], []
        todo = [(c, op) for c in range(C) for op in (0, 1) for _ in range(int(rng.integers(0, 6)))]
        for t in rng.permutation(len(todo)):
            c, op = todo[t]
            n = int(rng.choice([0, 1, 3, 29, 31, 64, 65, 200, 1500]))
            payload = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            salt = int(rng.integers(0, 2**32))
            if op == 0 and algo == 2:
                if rng.random() < 0.1:
                    peer_w[c], wire = orc.rc4_crypt(peer_w[c], payload[:29])        # no frame at all
                else:
                    peer_w[c], wire = orc.rc4md5_frame(peer_w[c], payload, salt)
                    if rng.random() < 0.1:
                        wire = bytearray(wire)
                        wire[8 + int(rng.integers(0, len(wire) - 8))] ^= 2
                        wire = bytes(wire)
                ours[0][c], dec, ok = orc.rc4md5_open(ours[0][c], wire)
                subs.append((c, 0, wire, 0))
                expect.append((c, 0, dec, ok))
            elif op == 0:
                peer_w[c], wire = orc.rc4_crypt(peer_w[c], payload)
                ours[0][c], dec = orc.rc4_crypt(ours[0][c], wire)
                subs.append((c, 0, wire, 0))
                expect.append((c, 0, dec, 1))
            elif algo == 2:
                ours[1][c], frame = orc.rc4md5_frame(ours[1][c], payload, salt)
                subs.append((c, 1, payload, salt))
                expect.append((c, 1, frame, 1))
            else:
                ours[1][c], wire = orc.rc4_crypt(ours[1][c], payload)
                subs.append((c, 1, payload, salt))
                expect.append((c, 1, wire, 1))
        out.append((subs, expect, [list(ours[0]), list(ours[1])]))
    return keys, out


def _drive(brb, keys, rounds, pipelined, by_conn=False, **kw):
    """Feeds the traffic to a batcher -> per round (results, states of every connection)."""
    b = brb.TransformBatcher(128, 4 << 20, pipelined=pipelined, **kw)
    b.enable_batch(list(range(len(keys))), keys)
    res, pending = [], None
    for subs, _, _ in rounds:
        for c, op, data, salt in subs:
            assert (b.read(c, data) if op == 0 else b.write(c, data, salt)) == 1
        if pipelined:
            got = b.flush_async()
            if pending is not None:
                res.append([got, pending])
            pending = [[b.state(c, op) for c in range(len(keys))] for op in (0, 1)]
        else:
            got = b.flush()
            res.append([got, [[b.state(c, op) for c in range(len(keys))] for op in (0, 1)]])
    if pipelined:
        res.append([b.flush(), pending])
    b.close()
    return res


def _by_conn(results):
    """All-devices batchers deliver device by device: compare per connection and direction, in order."""
    d = {}
    for c, op, out, valid in results:
        d.setdefault((c, op), []).append((out, valid))
    return d


@pytest.mark.parametrize("mode", ["copy", "zero_copy", "pipelined", "zero_copy_pipelined", "all_devices"])
@pytest.mark.parametrize("algo", [1, 2])
def test_batcher_conn_lists(brb, orc, torch_dev, algo, mode):
    """A batcher with conn_lists=True: results in submission order and GetState after each round equal the
    oracle and a batcher without the flag fed the same traffic."""
    keys, rounds = _traffic(orc, algo, 0xBA7)
    kw = dict(algo=algo, zero_copy="zero_copy" in mode, all_devices=mode == "all_devices")
    pipelined = "pipelined" in mode
    with brb.TestOption("devices", 2 if mode == "all_devices" else 0):
        with_lists = _drive(brb, keys, rounds, pipelined, conn_lists=True, **kw)
        without = _drive(brb, keys, rounds, pipelined, conn_lists=False, **kw)
    assert len(with_lists) == len(rounds)
    for r, ((_, expect, states), (got, st), (ref, ref_st)) in enumerate(zip(rounds, with_lists, without)):
        if mode == "all_devices":
            assert _by_conn(got) == _by_conn(expect), r
            assert _by_conn(ref) == _by_conn(expect), r
        else:
            assert got == expect, r
            assert ref == expect, r
        assert st == states and ref_st == states, r


def _launch_count_round(brb, orc, conn_lists, fault):
    """RC4_MD5; connection 0: three reads and two writes, connection 1: one read.  Without lists that is five
    launches (sub-rounds 0, 1, 2: READ+WRITE, READ+WRITE, READ); with lists two (READ, WRITE)."""
    keys = [b"launch-count-0", b"launch-count-1"]
    b = brb.TransformBatcher(4, 1 << 16, 2, conn_lists=conn_lists)
    b.inject_fault(fault)
    peer = [orc.rc4_init(k) for k in keys]
    rd = [orc.rc4_init(k) for k in keys]
    wr = orc.rc4_init(keys[0])
    expect = []
    for c, k in enumerate(keys):
        b.enable(c, k)
    for c, op, n in [(0, 0, 100), (0, 1, 64), (1, 0, 7), (0, 0, 0), (0, 1, 1500), (0, 0, 65)]:
        payload = bytes((n + i) & 255 for i in range(n))
        if op == 0:
            peer[c], frame = orc.rc4md5_frame(peer[c], payload, 11 * n)
            rd[c], dec, ok = orc.rc4md5_open(rd[c], frame)
            assert ok == 1 and b.read(c, frame) == 1
            expect.append((c, 0, dec, 1))
        else:
            wr, frame = orc.rc4md5_frame(wr, payload, 5 * n)
            assert b.write(c, payload, 5 * n) == 1
            expect.append((c, 1, frame, 1))
    return b, expect, rd, wr


def test_conn_lists_round_is_two_launches(brb, orc, torch_dev):
    """The launch count through the existing hook: with the flag and InjectFault(2) the round is delivered
    whole -- launches 0 and 1 are all there is."""
    b, expect, rd, wr = _launch_count_round(brb, orc, True, 2)
    assert b.flush() == expect
    assert [b.state(0, 0), b.state(1, 0), b.state(0, 1)] == [rd[0], rd[1], wr]
    b.close()


def test_conn_lists_failed_second_launch_drops_the_round(brb, orc, torch_dev):
    """InjectFault(1): the WRITE launch fails on the host, so the round is dropped by the rule for a host-side
    launch failure: every callback DROPPED, never re-run, no poisoning; the READ group ran exactly once."""
    b, expect, rd, wr = _launch_count_round(brb, orc, True, 1)
    with pytest.raises(RuntimeError, match="dropped") as ei:
        b.flush()
    assert ei.value.code == brb.BATCH_DROPPED
    assert ei.value.results == [(c, op, b"", brb.TRANSFORM_DROPPED) for c, op, _, _ in expect]
    b.inject_fault(-1)
    assert b.flush() == []
    assert [b.state(0, 0), b.state(1, 0)] == [rd[0], rd[1]]                  # all of the READ lists ran, once
    assert b.state(0, 1) == orc.rc4_init(b"launch-count-0")                  # the WRITE group never ran
    st, frame = orc.rc4md5_frame(orc.rc4_init(b"launch-count-0"), b"next", 3)
    assert b.write(0, b"next", 3) == 1                                       # not poisoned
    assert b.flush() == [(0, 1, frame, 1)] and b.state(0, 1) == st
    b.close()


def test_without_the_flag_the_same_round_is_five_launches(brb, orc, torch_dev):
    """Without the flag the batcher behaves as before, down to its launch count: the same round under
    InjectFault(2) is dropped (launch 2 of 5 is sub-round 1's READ group)."""
    b, expect, rd, wr = _launch_count_round(brb, orc, False, 2)
    with pytest.raises(RuntimeError, match="dropped") as ei:
        b.flush()
    assert ei.value.results == [(c, op, b"", brb.TRANSFORM_DROPPED) for c, op, _, _ in expect]
    b.close()
    b, expect, rd, wr = _launch_count_round(brb, orc, False, 5)             # launches 0..4 are all there is
    assert b.flush() == expect
    b.close()
