"""The RC4 read-ahead patches and the generator's start-up on the card, with states built to hit them.

brb_rc4::Gen (csrc/gpu/rc4_device.h) reads S[i] two to three bytes ahead and repairs it with three
ordered patches; load() stands "identity swaps" in for the swaps before a call's first byte.  Random
keys from indices (0, 0) almost never make two patches fire for one byte, so these tests feed every
RC4 kernel the directed classes of tests/rc4_model.py (their hazard counts, and the broken generators
they catch, are asserted in test_rc4_hazards_cpu.py):

  A  every (index1, index2) with a fresh permutation, 1..8 bytes      -- start-up
  B  low-entropy non-permutation states, index2 = index1 + 0..7         -- double and triple patches
  C  512 states of A and B through 40 chained calls of 0..3 bytes       -- store() / load() around every byte
  D  B with random non-zero padding and flags bytes                     -- bytes 258..263 pass through

Every check is bit for bit against the C oracle: the output bytes, all 264 bytes of every state, and
the sentinel bytes between streams (gaps of 0..3 bytes, so streams start at every alignment).  The
key-setup sweep (rc4_keysetup_kernel, one patch: j == i + 1) gets keys that force j == i + 1, i, i + 2
at every step.  These tests must stay green across any re-pipelining of the generator.

Measured on an MI355X: the module's 20 tests take 2.8 s in all, 1.7 s of it the shared fixtures
(classes, oracle results, torch start-up); class A on the wave pair 0.17 s, each chained-call test
0.16 s, class A on the other routes 0.02 .. 0.05 s, every other test under 5 ms.  A library built
with the patches in reverse order and the key-setup patch dropped fails all 20.
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


M = _sibling("rc4_model")
RAGGED = _sibling("test_rc4").RAGGED

IN_GAP, OUT_FILL = 0xA5, 0x5A
# the four routes of a single-buffer CRYPT launch (brb::launch_rc4_single, brb_kernels.h): wave pair, one wave with the launcher's sink, one wave with
# the per-stream sink, one wave with the sector sink
ROUTES = [("rc4_pair", 1), ("rc4_pair", 0), ("rc4_sector", 0), ("rc4_sector", 1)]
ROUTE_IDS = [f"{k}={v}" for k, v in ROUTES]


@pytest.fixture(scope="module")
def torch_dev(brb):
    import torch
    assert torch.cuda.is_available(), "no HIP device visible to torch"
    assert brb.gpu_available(), brb.lib().BRB_CryptoGPU_LastError()
    return torch


def _to(torch, a):
    return torch.from_numpy(np.array(a)).cuda()           # a copy: the shared arrays are read-only


class Case:
    """One class laid out in a buffer, with the oracle's in-place result and states (computed once)."""

    def __init__(self, orc, name):
        self.states, lens = getattr(M, "class_" + name)()
        self.offs, self.lens, self.total = M.layout(lens, 31 + ord(name), base=ord(name) & 3)
        assert {int(o) & 3 for o in self.offs} == {0, 1, 2, 3}
        self.data = M.fill(self.offs, self.lens, self.total, 37 + ord(name), IN_GAP)
        self.mask = M.covered(self.offs, self.lens, self.total)
        self.want, self.want_st = self.data.copy(), self.states.copy()
        orc.rc4_crypt_batch(self.want_st, self.want, self.offs, self.lens)
        self.want_out = np.where(self.mask, self.want, np.uint8(OUT_FILL))
        for a in (self.states, self.offs, self.lens, self.data, self.mask, self.want, self.want_st, self.want_out):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def cases(orc):
    return {name: Case(orc, name) for name in "abd"}


def _bad_rows(got, want):
    return np.nonzero((got != want).any(axis=1))[0][:8].tolist()


@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_crypt_batch(brb, torch_dev, cases, name, route):
    """BRB_RC4_CryptBatch, device mode in place and host mode out of place, on every route."""
    torch, c = torch_dev, cases[name]
    pair = route == ("rc4_pair", 1)
    with brb.TestOption(*route):
        t, ts = _to(torch, c.data), _to(torch, c.states)
        brb.rc4_crypt_batch(ts, t, _to(torch, c.offs), _to(torch, c.lens), async_=pair)
        torch.cuda.synchronize()
        if pair:
            brb.async_fault_check()
        got_st = ts.cpu().numpy()
        assert np.array_equal(got_st, c.want_st), _bad_rows(got_st, c.want_st)
        assert np.array_equal(t.cpu().numpy(), c.want)
        hs, out = c.states.copy(), np.full_like(c.data, OUT_FILL)
        brb.rc4_crypt_batch(hs, c.data.copy(), c.offs.copy(), c.lens.copy(), out=out)
        assert np.array_equal(hs, c.want_st), _bad_rows(hs, c.want_st)
        assert np.array_equal(out, c.want_out)
        if pair:
            brb.async_fault_check()
    if name == "d":
        assert np.array_equal(got_st[:, 258:], c.states[:, 258:]) and (got_st[:, 258:] != 0).all()


@pytest.mark.parametrize("pair", [1, 0], ids=["pair", "single"])
def test_chained_tiny_calls(brb, orc, torch_dev, pair):
    """Class C: the state table stays in device memory through 40 calls of 0..3 bytes per stream; the
    concatenated output equals one oracle run over the concatenated input, the table after the last
    call equals the oracle's, and no byte between streams is ever written."""
    torch = torch_dev
    states, call_lens = M.class_c()
    n, tot = len(states), call_lens.sum(axis=0)
    zero = np.zeros(n, np.int64)
    cat_offs = (np.cumsum(tot) - tot).astype(np.uint64)
    cat = M.fill(cat_offs, tot, int(tot.sum()) + 8, 41, IN_GAP)
    want, want_st = cat.copy(), states.copy()
    orc.rc4_crypt_batch(want_st, want, cat_offs, tot.astype(np.uint32))
    got, cur = np.full_like(cat, IN_GAP), zero.copy()
    ts = _to(torch, states)
    with brb.TestOption("rc4_pair", pair):
        for call, lens in enumerate(call_lens):
            offs, lens, total = M.layout(lens, 100 + call, base=call & 3)
            k, t, pos = M.flat_index(offs, lens)
            src = cat_offs.astype(np.int64)[k] + cur[k] + t
            buf = np.full(total, IN_GAP, np.uint8)
            buf[pos] = cat[src]
            tb = _to(torch, buf)
            brb.rc4_crypt_batch(ts, tb, _to(torch, offs), _to(torch, lens), async_=bool(pair))
            res = tb.cpu().numpy()
            got[src] = res[pos]
            res[pos] = IN_GAP
            assert (res == IN_GAP).all(), call
            cur += lens
        torch.cuda.synchronize()
        if pair:
            brb.async_fault_check()
    assert np.array_equal(got, want)
    got_st = ts.cpu().numpy()
    assert np.array_equal(got_st, want_st), _bad_rows(got_st, want_st)


class Frames:
    """Class B's states as connection states: payloads of RAGGED lengths, the oracle's frames and write
    states, and the oracle's open of those frames from the same states."""

    def __init__(self, orc):
        self.states, _ = M.class_b()
        n = len(self.states)
        rag = RAGGED[:32]
        plens = [rag[k % len(rag)] for k in range(n)]
        self.offs, self.lens, total = M.layout(plens, 51, base=1)
        self.payload = M.fill(self.offs, self.lens, total, 53, IN_GAP)
        self.foffs, self.flens, ftotal = M.layout([30 + x for x in plens], 57, base=3)
        assert {int(o) & 3 for o in self.foffs} == {0, 1, 2, 3}
        self.salts = (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
        self.frames0 = np.full(ftotal, OUT_FILL, np.uint8)
        self.want_fr, self.want_ws = self.frames0.copy(), self.states.copy()
        orc.rc4md5_frame_batch(self.want_ws, self.payload, self.offs, self.lens, self.salts, self.want_fr, self.foffs)
        s1, f1 = orc.rc4md5_frame(self.states[9].tobytes(), self._payload(9), int(self.salts[9]))
        assert s1 == self.want_ws[9].tobytes() and f1 == self._frame(self.want_fr, 9)
        self.want_pt, self.want_rs = self.want_fr.copy(), self.states.copy()
        self.want_ok = np.zeros(n, np.uint8)
        orc.rc4md5_open_batch(self.want_rs, self.want_pt, self.foffs, self.flens, self.want_ok)
        s2, p2, ok = orc.rc4md5_open(self.states[9].tobytes(), f1)
        assert ok == 1 and s2 == self.want_rs[9].tobytes() and p2 == self._frame(self.want_pt, 9)
        assert self.want_ok.all() and np.array_equal(self.want_rs, self.want_ws)
        assert self._frame(self.want_pt, 9)[30:] == self._payload(9)
        self.fmask = M.covered(self.foffs, self.flens, ftotal)
        for a in vars(self).values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)

    def _payload(self, k):
        return self.payload[int(self.offs[k]):int(self.offs[k]) + int(self.lens[k])].tobytes()

    def _frame(self, buf, k):
        return buf[int(self.foffs[k]):int(self.foffs[k]) + int(self.flens[k])].tobytes()


@pytest.fixture(scope="module")
def frames(orc):
    return Frames(orc)


@pytest.fixture(params=[1, 0], ids=["pair", "single"])
def rc4md5_pair(request, brb):
    with brb.TestOption("rc4md5_pair", request.param):
        yield request.param


def test_frame_batch(brb, torch_dev, frames, rc4md5_pair):
    """BRB_RC4MD5_FrameBatch from class B's states, device and host mode: frames, write states and the
    bytes between frames against orc.rc4md5_frame."""
    torch, f = torch_dev, frames
    ts, tf = _to(torch, f.states), _to(torch, f.frames0)
    brb.rc4md5_frame_batch(ts, _to(torch, f.payload), _to(torch, f.offs), _to(torch, f.lens), _to(torch, f.salts), tf,
                           _to(torch, f.foffs), async_=bool(rc4md5_pair))
    torch.cuda.synchronize()
    if rc4md5_pair:
        brb.async_fault_check()
    got_st = ts.cpu().numpy()
    assert np.array_equal(got_st, f.want_ws), _bad_rows(got_st, f.want_ws)
    assert np.array_equal(tf.cpu().numpy(), f.want_fr)
    hs, hf = f.states.copy(), f.frames0.copy()
    brb.rc4md5_frame_batch(hs, f.payload.copy(), f.offs.copy(), f.lens.copy(), f.salts.copy(), hf, f.foffs.copy())
    assert np.array_equal(hs, f.want_ws), _bad_rows(hs, f.want_ws)
    assert np.array_equal(hf, f.want_fr)


def test_open_batch(brb, torch_dev, frames, rc4md5_pair):
    """BRB_RC4MD5_OpenBatch on the frames the oracle wrote from class B's states, the read states
    starting as those states: every frame valid, plaintext and read states equal orc.rc4md5_open;
    device mode in place, host mode out of place."""
    torch, f = torch_dev, frames
    ts, tb = _to(torch, f.states), _to(torch, f.want_fr)
    _, valid = brb.rc4md5_open_batch(ts, tb, _to(torch, f.foffs), _to(torch, f.flens), async_=bool(rc4md5_pair))
    torch.cuda.synchronize()
    if rc4md5_pair:
        brb.async_fault_check()
    got_st = ts.cpu().numpy()
    assert np.array_equal(got_st, f.want_rs), _bad_rows(got_st, f.want_rs)
    assert np.array_equal(tb.cpu().numpy(), f.want_pt)
    assert valid.cpu().numpy().tolist() == [1] * len(f.states)
    hs, out = f.states.copy(), np.full_like(f.want_fr, IN_GAP)
    _, hv = brb.rc4md5_open_batch(hs, f.want_fr.copy(), f.foffs.copy(), f.flens.copy(), out=out)
    assert np.array_equal(hs, f.want_rs), _bad_rows(hs, f.want_rs)
    assert np.array_equal(out, np.where(f.fmask, f.want_pt, np.uint8(IN_GAP)))
    assert hv.tolist() == [1] * len(f.states)


# ---- key setup -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_init_batch_forced_keys(brb, orc, torch_dev, device):
    """BRB_RC4_InitBatch on keys that put j at i + 1 (the carried S[i] rides through every step), at i,
    at i + 2 (the nearest miss) and alternating, as 256-byte keys and as 300-byte keys whose tail must
    be ignored, at odd offsets of one blob: all 264 bytes of every state against the oracle, then 200
    bytes of BRB_RC4_CryptBatch from those states."""
    torch = torch_dev
    keys = [k for _, k in M.forced_keys()]
    blob, koffs, klens = M.odd_blob(keys)
    want_st = np.frombuffer(b"".join(orc.rc4_init(k) for k in keys), np.uint8).reshape(len(keys), 264).copy()
    offs, lens, total = M.layout([200] * len(keys), 61, base=1)
    data = M.fill(offs, lens, total, 67, IN_GAP)
    want, want_st2 = data.copy(), want_st.copy()
    orc.rc4_crypt_batch(want_st2, want, offs, lens)
    if device:
        st = brb.rc4_init_batch(_to(torch, blob), _to(torch, koffs.view(np.int64)), _to(torch, klens.view(np.int32)))
        got = st.cpu().numpy()
    else:
        st = brb.rc4_init_batch(blob, koffs, klens)
        got = st.copy()
    assert np.array_equal(got, want_st), _bad_rows(got, want_st)
    buf = _to(torch, data) if device else data.copy()
    args = (_to(torch, offs), _to(torch, lens)) if device else (offs, lens)
    brb.rc4_crypt_batch(st, buf, *args)
    assert np.array_equal(buf.cpu().numpy() if device else buf, want)
    got2 = st.cpu().numpy() if device else st
    assert np.array_equal(got2, want_st2), _bad_rows(got2, want_st2)
