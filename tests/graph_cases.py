"""The scenarios and the capture / replay runner of tests/test_graph_capture.py.

A helper, not a test module: nothing here is collected by pytest.

A scenario (Case) names the device buffers of one device-mode BRB_BATCH_ASYNC call, draws their contents
for the warm-up and for every replay from fixed seeds, makes the call, and says what the oracle leaves in
every buffer the call may write.  run_case() is the one place that captures and replays:

  1. every device tensor is allocated, with replay 0's contents;
  2. one eager call on a separate set of buffers, under the same test options, loads the kernel;
  3. the call is captured with torch.cuda.graph (capture_error_mode "global", one stream, no fork or join)
     on a thread that has never called the library, so its thread-local state is cold inside the capture;
     that thread stays alive until the last replay is checked;
  4. before replay r the same tensors are overwritten in place (copy_) with replay r's contents: data
     bytes, offsets, lengths, lists, salts and masks change, counts and extents do not; state (RC4 states,
     streaming contexts) is written once and then carried;
  5. after each replay every written buffer is compared bit for bit with the oracle -- guard rows and fill
     bytes included -- and every other buffer with what was put there.

Replay r's expected image must differ from replay r - 1's (asserted on the CPU), so a graph that replayed
stale results cannot pass.
"""
import contextlib
import hashlib
import importlib.util
import os
import sys
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
K = 3                        # replays per graph
WARM = -1                    # the replay number of the warm-up's contents
PAD = 0xA5                   # guard rows and unwritten output rows
FILL = 0x5A                  # a separate output buffer's bytes outside the written ranges
GAP = 0xEE                   # input bytes between records


def sibling(name):
    """A module of this directory by file name (tests/ is not a package)."""
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
        sys.modules[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[name])
    return sys.modules[name]


def rng_of(seed, r):
    return np.random.default_rng([seed, r + 1])


def as_torch(torch, a):
    """A CPU tensor over a copy of `a` (uint64 / uint32 as int64 / int32)."""
    a = np.array(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a)


def place(lens, rng, base=0, extra=0, gap=3):
    """Byte offsets of ranges of lens[k] + extra bytes in order, 0..gap seeded bytes apart, from `base`."""
    offs, pos = np.zeros(len(lens), np.uint64), base
    for k, n in enumerate(lens):
        pos += int(rng.integers(0, gap + 1))
        offs[k] = pos
        pos += int(n) + extra
    return offs, pos


def padded(a, size, dtype):
    """`a` as `dtype` in an array of `size` entries, zeros behind it (the unnamed tail of a list array)."""
    out = np.zeros(size, dtype)
    out[:len(a)] = a
    return out


def rand_bytes(rng, n):
    return rng.integers(0, 256, int(n), dtype=np.uint8)


def span(buf, o, n):
    return buf[int(o):int(o) + int(n)].tobytes() if n else b""


def guarded(n, width=None, fill=PAD, dtype=np.uint8):
    """n + 2 rows of `fill`; the call gets rows 1 .. n."""
    return np.full((n + 2,) if width is None else (n + 2, width), fill, dtype)


# ---- the runner ------------------------------------------------------------------------------------
class CaptureThread:
    """A fresh thread that runs what it is handed, one job at a time, and lives until close(): the library
    keeps the async fault word of a captured wave-pair call in the capturing thread's state."""

    def __init__(self):
        self._job, self._have, self._done = None, threading.Event(), threading.Event()
        self._thread = threading.Thread(target=self._loop)
        self._thread.start()

    def _loop(self):
        while True:
            self._have.wait()
            self._have.clear()
            if self._job is None:
                return
            try:
                self._result = (True, self._job())
            except BaseException as e:              # handed to the caller of run()
                self._result = (False, e)
            self._done.set()

    def run(self, fn):
        self._job = fn
        self._done.clear()
        self._have.set()
        self._done.wait()
        ok, value = self._result
        if not ok:
            raise value
        return value

    def close(self):
        if self._thread.is_alive():
            self._job = None
            self._have.set()
            self._thread.join()


def capture(torch, brb, stream, fn):
    """Captures fn() on `stream` on the calling thread.  -> (graph, None), or (None, what went wrong): a call
    that fails does so inside the context manager, which then ends the capture; nothing is tried again."""
    g = torch.cuda.CUDAGraph()
    errs = []
    try:
        with torch.cuda.graph(g, stream=stream):
            try:
                fn()
            except Exception as e:
                errs.append(f"the call: {e}")
    except Exception as e:
        errs.append(f"the capture: {type(e).__name__}: {e}")
    if errs:
        last = brb.lib().BRB_CryptoGPU_LastError().decode(errors="replace")
        return None, "; ".join(errs) + f" [BRB_CryptoGPU_LastError: {last!r}]"
    return g, None


def options(brb, opts):
    st = contextlib.ExitStack()
    for name, value in opts.items():
        st.enter_context(brb.TestOption(name, value))
    return st


def differs(name, got, want, r):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    bad = np.flatnonzero(got != want)
    if bad.size:
        raise AssertionError(f"replay {r}: {name} differs in {bad.size} of {want.size} entries, the first at "
                             f"{int(bad[0])}: {int(got[bad[0]]):#x} for {int(want[bad[0]]):#x}")


class Case:
    """One call under a graph.  inputs(r, host) -> {name: array}: the contents of every device buffer for
    replay r (host: what the buffers held before, {} for replay 0 and the warm-up); the names in `carried`
    are written for replay 0 only.  call(t, stream) makes the library call on the tensors t.  expect(h) ->
    {name: array}: the whole image of every buffer the call may write, from the host copies h.  compare()
    is bit-exact equality unless a scenario narrows it to what the contract defines."""
    options = {}
    carried = ()
    constant = ()            # written buffers whose expected image is the same for every replay by nature

    def precheck(self, t):
        pass

    def compare(self, name, got, want, before, r):
        differs(name, got, want, r)

    def finish(self, t, host):
        pass


def run_case(brb, torch, case, replays=K):
    def device(arrays):
        return {name: as_torch(torch, a).cuda() for name, a in arrays.items()}

    def fetch(t, like):
        return t.cpu().numpy().view(like.dtype).reshape(like.shape)

    worker = CaptureThread()
    try:
        with options(brb, case.options):
            stream = torch.cuda.Stream()
            host = {name: np.array(a) for name, a in case.inputs(0, {}).items()}
            dev = device(host)
            warm = device(case.inputs(WARM, {}))
            case.precheck(dev)
            case.precheck(warm)
            torch.cuda.synchronize()
            case.call(warm, stream)                              # eager: loads the kernel outside the capture
            stream.synchronize()
            brb.async_fault_check()
            graph, err = worker.run(lambda: capture(torch, brb, stream, lambda: case.call(dev, stream)))
            assert graph is not None, f"the capture failed: {err}"
            prev = None
            for r in range(replays):
                if r:
                    for name, a in case.inputs(r, host).items():
                        if name in case.carried:
                            continue
                        assert a.shape == host[name].shape and a.dtype == host[name].dtype, name
                        host[name] = np.array(a)
                        dev[name].copy_(as_torch(torch, a))      # the same tensor, in place
                torch.cuda.synchronize()
                before = {name: fetch(dev[name], host[name]) for name in case.carried}
                want = case.expect(host)
                if prev is not None:
                    for name in set(want) - set(case.constant):
                        assert not np.array_equal(want[name], prev[name]), f"replay {r} expects replay {r - 1}'s {name}"
                graph.replay()
                torch.cuda.synchronize()
                for name, a in host.items():
                    got = fetch(dev[name], a)
                    if name in want:
                        case.compare(name, got, want[name], before.get(name), r)
                    else:
                        differs(name + " (an input)", got, a, r)
                for name in case.carried:
                    host[name] = want[name]
                prev = want
            brb.async_fault_check()                              # the replaying thread has nothing to report
            worker.run(brb.async_fault_check)                    # nor has the capturing one
            case.finish(dev, host)
    finally:
        torch.cuda.synchronize()
        worker.close()


# ---- stateless scenarios ---------------------------------------------------------------------------
DIGEST = {"md5": 16, "sha1": 20}


class FixedDigest(Case):
    """md5_batch_fixed / sha1_batch_fixed: n records of rec_len bytes from byte `base` of the buffer."""

    def __init__(self, brb, orc, alg, rec_len, n, base, route=None):
        self.brb, self.alg, self.L, self.n, self.base, self.route = brb, alg, rec_len, n, base, route
        self.fn = getattr(brb, alg + "_batch_fixed")
        self.orc_fn = getattr(orc, alg + "_batch_fixed")
        self.seed = 0x6701 + rec_len

    def inputs(self, r, host):
        return {"data": rand_bytes(rng_of(self.seed, r), self.base + self.n * self.L + 8),
                "out": guarded(self.n, DIGEST[self.alg])}

    def precheck(self, t):
        if self.route is not None:
            assert self.brb.fixed_route(t["data"].data_ptr() + self.base, self.L) == self.route

    def call(self, t, s):
        self.fn(t["data"][self.base:], self.L, n=self.n, out=t["out"][1:self.n + 1], stream=s, async_=True)

    def expect(self, h):
        want = h["out"].copy()
        recs = np.ascontiguousarray(h["data"][self.base:self.base + self.n * self.L])
        want[1:self.n + 1] = self.orc_fn(recs, self.L, self.n)
        return {"out": want}


class VarDigest(Case):
    """md5_batch / sha1_batch: lengths redrawn for every replay, records at byte offsets."""
    LENS = (0, 1, 55, 56, 63, 64, 65, 119, 120, 1500, 3000)
    N = 130

    def __init__(self, brb, orc, alg, var_line):
        self.fn, self.orc_fn, self.alg = getattr(brb, alg + "_batch"), getattr(orc, alg + "_batch"), alg
        self.options = {"var_line": var_line}
        self.size = 4 + self.N * (max(self.LENS) + 3) + 8
        self.seed = 0x6702

    def inputs(self, r, host):
        g = rng_of(self.seed, r)
        lens = g.choice(self.LENS, self.N).astype(np.uint32)
        lens[:len(self.LENS)] = g.permutation(self.LENS)        # every length in every replay
        offs, end = place(lens, g, base=(r + 1) & 3)
        assert end <= self.size
        return {"data": rand_bytes(g, self.size), "offs": offs, "lens": lens, "out": guarded(self.N, DIGEST[self.alg])}

    def call(self, t, s):
        self.fn(t["data"], t["offs"], t["lens"], out=t["out"][1:self.N + 1], stream=s, async_=True)

    def expect(self, h):
        want = h["out"].copy()
        want[1:self.N + 1] = self.orc_fn(h["data"], h["offs"], h["lens"])
        return {"out": want}


def lowered(key):
    return bytes(b + 32 if 65 <= b <= 90 else b for b in key)


class LowerText(Case):
    """md5_lower_text_batch: digests and hex strings of keys of 0..170 bytes."""
    N = 130

    def __init__(self, brb, orc):
        self.brb = brb
        self.size = 4 + self.N * 173 + 8
        self.seed = 0x6703

    def inputs(self, r, host):
        g = rng_of(self.seed, r)
        lens = g.integers(0, 171, self.N).astype(np.uint32)
        lens[[3, 64, 129]] = (0, 170, 0)
        offs, end = place(lens, g, base=(r + 1) & 3)
        assert end <= self.size
        data = g.integers(0x30, 0x80, self.size, dtype=np.uint8)        # letters of both cases, digits, signs
        wild = g.random(self.size) < 0.1
        data[wild] = rand_bytes(g, int(wild.sum()))                      # and any byte now and then
        return {"data": data, "offs": offs, "lens": lens, "out": guarded(self.N, 16), "strs": guarded(self.N, 33)}

    def call(self, t, s):
        self.brb.md5_lower_text_batch(t["data"], t["offs"], t["lens"], out=t["out"][1:self.N + 1],
                                      strings=t["strs"][1:self.N + 1], stream=s, async_=True)

    def expect(self, h):
        out, strs = h["out"].copy(), h["strs"].copy()
        for i in range(self.N):
            d = hashlib.md5(lowered(span(h["data"], h["offs"][i], h["lens"][i]))).digest()
            out[1 + i] = np.frombuffer(d, np.uint8)
            strs[1 + i] = np.frombuffer(d.hex().encode() + b"\0", np.uint8)
        return {"out": out, "strs": strs}


SEG_LENS = (0, 1, 2, 3, 4, 5, 59, 60, 61, 63, 64, 65, 127, 128, 129, 200)


def seg_lists(g, n, most, lens=SEG_LENS, empty=()):
    """Per item a list of 0..most segment lengths; the items in `empty` get none."""
    return [[] if i in empty else [int(x) for x in g.choice(lens, int(g.integers(0, most + 1)))] for i in range(n)]


def seg_arrays(lists, g, cap, size):
    """(data, seg_offsets, seg_lengths, first) with the list arrays padded to cap + 1 entries; every offset,
    those of empty segments too, lies inside the `size` bytes."""
    flat = [n for li in lists for n in li]
    offs, end = place(flat, g, base=4, gap=2)
    assert end + 8 <= size and len(flat) <= cap
    first = np.concatenate([[0], np.cumsum([len(li) for li in lists])]).astype(np.uint64)
    return rand_bytes(g, size), padded(offs, cap + 1, np.uint64), padded(flat, cap + 1, np.uint32), first


def fed(data, soff, slen, first, i):
    return [span(data, soff[k], slen[k]) for k in range(int(first[i]), int(first[i + 1]))]


class Segments(Case):
    """md5_batch_segments: n records of 0..5 segments."""
    N, MOST = 65, 5

    def __init__(self, brb, orc, seg_line):
        self.brb, self.orc = brb, orc
        self.options = {"seg_line": seg_line}
        self.size = 4 + self.N * self.MOST * 203 + 16
        self.seed = 0x6704

    def inputs(self, r, host):
        g = rng_of(self.seed, r)
        data, soff, slen, first = seg_arrays(seg_lists(g, self.N, self.MOST), g, self.N * self.MOST, self.size)
        return {"data": data, "soff": soff, "slen": slen, "first": first, "out": guarded(self.N, 16)}

    def call(self, t, s):
        self.brb.md5_batch_segments(t["data"], t["soff"], t["slen"], t["first"], out=t["out"][1:self.N + 1], stream=s,
                                    async_=True)

    def expect(self, h):
        want = h["out"].copy()
        for i in range(self.N):
            msg = b"".join(fed(h["data"], h["soff"], h["slen"], h["first"], i))
            want[1 + i] = np.frombuffer(self.orc.md5(msg), np.uint8)
        return {"out": want}


# MetaData packs: a few items of a few bytes, some packs damaged so that every replay sees several codes
MD_N, MD_ITEMS, MD_DATA = 65, 4, 120
MD_MAX = 64 + MD_ITEMS * (24 + MD_DATA + 1)
M64 = 1 << 64
S64, S32 = 0xA5C3A5C3A5C3A5C3, 0xA5C3A5C3
SLOT_GUARD = 37


def md_items(g):
    return [(int(g.integers(0, M64, dtype=np.uint64)), int(g.integers(0, M64, dtype=np.uint64)),
             rand_bytes(g, g.integers(0, MD_DATA + 1)).tobytes()) for _ in range(int(g.integers(0, MD_ITEMS + 1)))]


def md_packs(orc, g):
    """MD_N packs of the oracle; about a third damaged: the magic, the digest, a canary, or cut short."""
    packs = []
    for p in range(MD_N):
        items = md_items(g)
        b = bytearray(orc.metadata_pack(items))
        kind = int(g.integers(0, 12))
        if kind == 0:
            b[16 + int(g.integers(0, 8))] ^= 1 << int(g.integers(0, 8))
        elif kind == 1 and items:
            b[24 + int(g.integers(0, 16))] ^= 1 << int(g.integers(0, 8))
        elif kind == 2 and items:
            b[-1] ^= 0x40
        elif kind == 3:
            b = b[:len(b) - int(g.integers(1, 30))]
        packs.append(bytes(b))
    return packs


def md_buffer(packs, g, size):
    offs, end = place([len(p) for p in packs], g, base=5, gap=7)
    assert end + 8 <= size
    buf = np.full(size, GAP, np.uint8)
    for o, p in zip(offs, packs):
        buf[int(o):int(o) + len(p)] = np.frombuffer(p, np.uint8)
    return buf, offs, np.array([len(p) for p in packs], np.uint32)


class MetaUnpack(Case):
    """metadata_unpack_batch: one BRB_MetaDataUnpackInfo per pack."""

    def __init__(self, brb, orc, seg_line):
        self.brb, self.orc = brb, orc
        self.options = {"seg_line": seg_line}
        self.size = 8 + MD_N * (MD_MAX + 7) + 16
        self.seed = 0x6705

    def inputs(self, r, host):
        g = rng_of(self.seed, r)
        data, offs, lens = md_buffer(md_packs(self.orc, g), g, self.size)
        return {"data": data, "offs": offs, "lens": lens, "info": guarded(MD_N, 32)}

    def call(self, t, s):
        self.brb.metadata_unpack_batch(t["data"], t["offs"], t["lens"], out=t["info"][1:MD_N + 1], stream=s, async_=True)

    def expect(self, h):
        want = h["info"].copy()
        want[1:MD_N + 1] = self.orc.metadata_unpack_batch(h["data"], h["offs"], h["lens"])
        assert len(set(want[1:MD_N + 1, 0].tolist())) >= 3           # several return codes in every replay
        return {"info": want}


class MetaUnpackItems(MetaUnpack):
    """metadata_unpack_items_batch: the info and the item table, slot counts redrawn for every replay."""

    def __init__(self, brb, orc, seg_line):
        super().__init__(brb, orc, seg_line)
        self.walk = sibling("test_metadata_items_cpu")
        self.slots = 2 * SLOT_GUARD + 6 * MD_N
        self.seed = 0x6706

    def inputs(self, r, host):
        d = super().inputs(r, host)
        caps = rng_of(self.seed + 1, r).integers(1, 7, MD_N)             # 1..6 slots: some tables are cut short
        first = np.full(MD_N + 1, SLOT_GUARD, np.uint64)
        first[1:] += np.cumsum(caps).astype(np.uint64)
        d.update(first=first, added=guarded(MD_N, fill=S32, dtype=np.uint32),
                 ioff=np.full(self.slots, S64, np.uint64), ilen=np.full(self.slots, S32, np.uint32),
                 iid=np.full(self.slots, S64, np.uint64), isub=np.full(self.slots, S64, np.uint64))
        return d

    def call(self, t, s):
        self.brb.metadata_unpack_items_batch(t["data"], t["offs"], t["lens"], t["ioff"], t["ilen"], t["iid"], t["isub"],
                                             t["first"], items_added=t["added"][1:MD_N + 1], out=t["info"][1:MD_N + 1],
                                             stream=s, async_=True)

    def expect(self, h):
        want = super().expect(h)
        table = {name: h[name].copy() for name in ("ioff", "ilen", "iid", "isub")}
        added = h["added"].copy()
        infos = want["info"][1:MD_N + 1].copy().view(self.brb.METADATA_INFO_DTYPE).reshape(-1)
        for p in range(MD_N):
            five, items = self.walk.py_unpack_items(span(h["data"], h["offs"][p], h["lens"][p]))
            assert five == tuple(int(x) for x in infos[p].tolist()), p    # the walker agrees with the oracle
            added[1 + p] = len(items)
            s0, cap = int(h["first"][p]), int(h["first"][p + 1]) - int(h["first"][p])
            for j, (o, sz, i, sub) in enumerate(items[:cap]):
                table["ioff"][s0 + j], table["ilen"][s0 + j] = int(h["offs"][p]) + o, sz
                table["iid"][s0 + j], table["isub"][s0 + j] = i, sub
        want.update(table, added=added)
        return want


class MetaPack(Case):
    """metadata_pack_batch: the items scattered over a source buffer, the packs over a patterned output."""

    def __init__(self, brb, orc):
        self.brb, self.orc = brb, orc
        self.cap = MD_N * MD_ITEMS
        self.src = 8 + self.cap * (MD_DATA + 7) + 8
        self.dst = 16 + MD_N * (MD_MAX + 40) + 67
        self.seed = 0x6707

    def inputs(self, r, host):
        g = rng_of(self.seed, r)
        packs = [md_items(g) for _ in range(MD_N)]
        items = [it for p in packs for it in p]
        order = g.permutation(len(items))                               # the items in any order in the source
        ooffs, _ = place([len(items[j][2]) for j in order], g, base=(r + 1) & 7, gap=7)
        ioff = np.zeros(len(items), np.uint64)
        data = rand_bytes(g, self.src)
        for j, o in zip(order, ooffs):
            ioff[j] = o
            d = items[j][2]
            data[int(o):int(o) + len(d)] = np.frombuffer(d, np.uint8)
        first = np.concatenate([[0], np.cumsum([len(p) for p in packs])]).astype(np.uint64)
        sizes = [64 + sum(25 + len(d) for _, _, d in p) for p in packs]
        ooff, end = place(sizes, g, base=(r + 1) & 15, gap=40)
        assert end <= self.dst
        return {"data": data, "ioff": padded(ioff, self.cap + 1, np.uint64),
                "ilen": padded([len(d) for _, _, d in items], self.cap + 1, np.uint32),
                "iid": padded(np.array([i for i, _, _ in items], np.uint64), self.cap + 1, np.uint64),
                "isub": padded(np.array([s for _, s, _ in items], np.uint64), self.cap + 1, np.uint64),
                "first": first, "out": (np.arange(self.dst) % 251).astype(np.uint8), "ooff": ooff}

    def call(self, t, s):
        self.brb.metadata_pack_batch(t["data"], t["ioff"], t["ilen"], t["iid"], t["isub"], t["first"], t["out"], t["ooff"],
                                     stream=s, async_=True)

    def expect(self, h):
        want = h["out"].copy()
        for p in range(MD_N):
            items = [(int(h["iid"][k]), int(h["isub"][k]), span(h["data"], h["ioff"][k], h["ilen"][k]))
                     for k in range(int(h["first"][p]), int(h["first"][p + 1]))]
            w = self.orc.metadata_pack(items)
            want[int(h["ooff"][p]):int(h["ooff"][p]) + len(w)] = np.frombuffer(w, np.uint8)
        return {"out": want}


class Base64Encode(Case):
    N, MOST = 130, 400

    def __init__(self, brb, orc):
        self.brb, self.orc = brb, orc
        self.src = 4 + self.N * (self.MOST + 3) + 8
        self.dst = 4 + self.N * (4 * ((self.MOST + 2) // 3) + 3) + 8
        self.seed = 0x6708

    def inputs(self, r, host):
        g = rng_of(self.seed, r)
        lens = g.integers(0, self.MOST + 1, self.N).astype(np.uint32)
        lens[:8] = g.permutation([0, 1, 2, 3, 4, 5, 399, 400])
        offs, _ = place(lens, g, base=(r + 1) & 3)
        eoffs, end = place(4 * ((lens + 2) // 3), g, base=r + 1)
        assert end <= self.dst
        return {"data": rand_bytes(g, self.src), "offs": offs, "lens": lens, "out": np.full(self.dst, GAP, np.uint8),
                "eoffs": eoffs}

    def call(self, t, s):
        self.brb.base64_encode_batch(t["data"], t["offs"], t["lens"], t["out"], t["eoffs"], stream=s, async_=True)

    def expect(self, h):
        want = h["out"].copy()
        for i in range(self.N):
            w = self.orc.b64_encode(span(h["data"], h["offs"][i], h["lens"][i]))
            want[int(h["eoffs"][i]):int(h["eoffs"][i]) + len(w)] = np.frombuffer(w, np.uint8)
        return {"out": want}


class Base64Decode(Case):
    """Texts of 0..400 characters; every fifth holds a skipped byte, every eleventh a NUL that ends it."""
    N, MOST = 130, 400

    def __init__(self, brb, orc):
        self.brb, self.orc = brb, orc
        self.src = 4 + self.N * (self.MOST + 3) + 8
        self.dst = 4 + self.N * (3 * (self.MOST // 4) + 3) + 8
        self.seed = 0x6709

    def inputs(self, r, host):
        g = rng_of(self.seed, r)
        texts = []
        for i in range(self.N):
            t = bytearray(self.orc.b64_encode(rand_bytes(g, g.integers(0, 3 * self.MOST // 4 + 1)).tobytes()))
            if i % 5 == r % 5 and len(t) > 6:
                t[int(g.integers(0, len(t)))] = ord("\n")
            if i % 11 == r % 11 and len(t) > 10:
                t[int(g.integers(0, len(t)))] = 0
            texts.append(bytes(t))
        lens = np.array([len(t) for t in texts], np.uint32)
        offs, _ = place(lens, g, base=(r + 1) & 3)
        data = np.full(self.src, GAP, np.uint8)
        for o, t in zip(offs, texts):
            data[int(o):int(o) + len(t)] = np.frombuffer(t, np.uint8)
        doffs, end = place(3 * (lens // 4), g, base=r + 1)
        assert end <= self.dst
        return {"data": data, "offs": offs, "lens": lens, "out": np.full(self.dst, GAP, np.uint8), "doffs": doffs,
                "olen": guarded(self.N, fill=S32, dtype=np.uint32)}

    def call(self, t, s):
        self.brb.base64_decode_batch(t["data"], t["offs"], t["lens"], t["out"], t["doffs"], out_lengths=t["olen"][1:self.N + 1],
                                     stream=s, async_=True)

    def expect(self, h):
        want, olen = h["out"].copy(), h["olen"].copy()
        for i in range(self.N):
            w = self.orc.b64_decode(span(h["data"], h["offs"][i], h["lens"][i]))
            want[int(h["doffs"][i]):int(h["doffs"][i]) + len(w)] = np.frombuffer(w, np.uint8)
            olen[1 + i] = len(w)
        return {"out": want, "olen": olen}


WORD_GUARD = np.uint64(0xA5A5A5A5A5A5A5A5)


def bf_key(g):
    return rand_bytes(g, g.integers(4, 57)).tobytes()


class Blowfish(Case):
    """blowfish_encrypt_batch / blowfish_decrypt_batch: 257 blocks in place between guard words; the context
    in device memory is another key's on every replay."""
    BLOCKS = 257

    def __init__(self, brb, orc, decrypt):
        self.orc, self.decrypt = orc, decrypt
        self.fn = brb.blowfish_decrypt_batch if decrypt else brb.blowfish_encrypt_batch
        self.seed = 0x670A

    def inputs(self, r, host):
        g = rng_of(self.seed, r)
        words = np.full(2 * self.BLOCKS + 4, WORD_GUARD, np.uint64)
        words[2:-2] = g.integers(0, 1 << 63, 2 * self.BLOCKS, dtype=np.uint64) | np.uint64(1 << 47)
        return {"ctx": np.frombuffer(self.orc.bf_ctx_bytes(self.orc.bf_init(bf_key(g))), np.uint8), "words": words}

    def call(self, t, s):
        self.fn(t["ctx"], t["words"][2:-2], n_blocks=self.BLOCKS, stream=s, async_=True)

    def expect(self, h):
        want = h["words"].copy()
        ctx = self.orc.BfCtx.from_buffer_copy(h["ctx"].tobytes())
        body = np.ascontiguousarray(want[2:-2])
        self.orc.bf_ecb(ctx, body, self.decrypt)
        want[2:-2] = body
        return {"words": want}


class BlowfishKeyed(Case):
    """Keyed Blowfish: 65 records across 17 contexts; keys, the index, the counts and the placement all redrawn."""
    N, N_CTX = 65, 17
    COUNTS = (0, 1, 2, 63, 64, 65)

    def __init__(self, brb, orc, decrypt):
        self.orc, self.decrypt = orc, decrypt
        self.fn = brb.blowfish_decrypt_batch_keyed if decrypt else brb.blowfish_encrypt_batch_keyed
        self.words = 2 + self.N * (2 * max(self.COUNTS) + 2) + 4
        self.seed = 0x670B

    def inputs(self, r, host):
        g = rng_of(self.seed, r)
        cnt = g.choice(self.COUNTS, self.N).astype(np.uint32)
        idx = g.integers(0, self.N_CTX, self.N).astype(np.uint32)
        idx[:self.N_CTX] = g.permutation(self.N_CTX)                     # every context is used
        woff, pos = np.zeros(self.N, np.uint64), 1
        for i in g.permutation(self.N):                                 # out of memory order, a guard word between
            pos += int(g.integers(0, 2))
            woff[i] = pos
            pos += 2 * int(cnt[i]) + 1
        assert pos + 2 <= self.words
        words = np.full(self.words, WORD_GUARD, np.uint64)
        for o, c in zip(woff, cnt):
            words[int(o):int(o) + 2 * int(c)] = g.integers(0, 1 << 63, 2 * int(c), dtype=np.uint64) | np.uint64(1 << 47)
        ctxs = np.frombuffer(b"".join(self.orc.bf_ctx_bytes(self.orc.bf_init(bf_key(g))) for _ in range(self.N_CTX)), np.uint8)
        return {"ctxs": ctxs.reshape(self.N_CTX, 8336), "words": words, "woff": woff, "cnt": cnt, "idx": idx}

    def call(self, t, s):
        self.fn(t["ctxs"], t["words"], t["woff"], t["cnt"], ctx_index=t["idx"], stream=s, async_=True)

    def expect(self, h):
        want = h["words"].copy()
        for c in range(self.N_CTX):
            ctx = self.orc.BfCtx.from_buffer_copy(h["ctxs"][c].tobytes())
            for i in np.flatnonzero(h["idx"] == c):
                o, k = int(h["woff"][i]), 2 * int(h["cnt"][i])
                if k:
                    body = np.ascontiguousarray(want[o:o + k])
                    self.orc.bf_ecb(ctx, body, self.decrypt)
                    want[o:o + k] = body
        return {"words": want}


class KeySetup(Case):
    """rc4_init_batch / blowfish_init_batch: 65 keys of mixed lengths, back to back at every alignment."""
    N = 65
    LENS = {"rc4": (1, 2, 5, 9, 16, 255, 256, 257, 300), "blowfish": (1, 2, 3, 4, 5, 7, 8, 16, 56, 64, 71, 72, 73, 100)}
    WIDTH = {"rc4": 264, "blowfish": 8336}

    def __init__(self, brb, orc, what):
        self.orc, self.what = orc, what
        self.fn = getattr(brb, what + "_init_batch")
        self.size = self.N * max(self.LENS[what]) + 8
        self.seed = 0x670C

    def inputs(self, r, host):
        g = rng_of(self.seed, r)
        lens = g.choice(self.LENS[self.what], self.N).astype(np.uint32)
        lens[:len(self.LENS[self.what])] = g.permutation(self.LENS[self.what])
        offs, end = place(lens, g, base=(r + 1) & 3, gap=0)
        assert end <= self.size
        return {"keys": rand_bytes(g, self.size), "offs": offs, "lens": lens,
                "out": guarded(self.N, self.WIDTH[self.what])}

    def call(self, t, s):
        self.fn(t["keys"], t["offs"], t["lens"], out=t["out"][1:self.N + 1], stream=s, async_=True)

    def expect(self, h):
        want = h["out"].copy()
        for i in range(self.N):
            key = span(h["keys"], h["offs"][i], h["lens"][i])
            made = self.orc.rc4_init(key) if self.what == "rc4" else self.orc.bf_ctx_bytes(self.orc.bf_init(key))
            want[1 + i] = np.frombuffer(made, np.uint8)
        return {"out": want}


# ---- stateful scenarios: replay k against the oracle run k times ---------------------------------------
RC4_LENS = (0, 1, 63, 64, 65, 255, 256, 257, 700)
RC4_N = 130


def rc4_keys(n, seed):
    g = np.random.default_rng([seed, 0x4B])
    return [rand_bytes(g, g.integers(1, 64)).tobytes() for _ in range(n)]


def guarded_states(brb, n, seed):
    st = guarded(n, 264)
    st[1:n + 1] = brb.rc4_states(rc4_keys(n, seed))
    return st


class Rc4Crypt(Case):
    """rc4_crypt_batch into a separate output: 130 streams whose states advance with every replay."""
    carried = ("states",)
    N = RC4_N

    def __init__(self, brb, orc, pair, stall=0):
        self.brb, self.orc = brb, orc
        self.options = {"rc4_pair": pair, "pair_stall": stall}
        self.size = 4 + self.N * (max(RC4_LENS) + 3) + 8
        self.seed = 0x6710

    def inputs(self, r, host):
        g = rng_of(self.seed, r)
        lens = g.choice(RC4_LENS, self.N).astype(np.uint32)
        lens[:len(RC4_LENS)] = g.permutation(RC4_LENS)
        offs, end = place(lens, g, base=(r + 1) & 3)
        assert end <= self.size
        d = {"data": rand_bytes(g, self.size), "offs": offs, "lens": lens, "out": np.full(self.size, FILL, np.uint8)}
        if not host:
            d["states"] = guarded_states(self.brb, self.N, self.seed + r)
        return d

    def call(self, t, s):
        self.brb.rc4_crypt_batch(t["states"][1:self.N + 1], t["data"], t["offs"], t["lens"], out=t["out"], stream=s,
                                 async_=True)

    def expect(self, h):
        st, out = h["states"].copy(), h["out"].copy()
        for i in range(self.N):
            o, n = int(h["offs"][i]), int(h["lens"][i])
            s2, ob = self.orc.rc4_crypt(st[1 + i].tobytes(), span(h["data"], o, n))
            st[1 + i] = np.frombuffer(s2, np.uint8)
            out[o:o + n] = np.frombuffer(ob, np.uint8)
        return {"states": st, "out": out}


class Rc4Frame(Case):
    """rc4md5_frame_batch: salt | "HASH:" | MD5 | NUL | payload under each stream's running state."""
    carried = ("states",)
    N = RC4_N

    def __init__(self, brb, orc, pair):
        self.brb, self.orc = brb, orc
        self.options = {"rc4md5_pair": pair}
        self.src = 4 + self.N * (max(RC4_LENS) + 3) + 8
        self.dst = self.src + 30 * self.N
        self.seed = 0x6711

    def inputs(self, r, host):
        g = rng_of(self.seed, r)
        lens = g.choice(RC4_LENS, self.N).astype(np.uint32)
        lens[:len(RC4_LENS)] = g.permutation(RC4_LENS)
        offs, _ = place(lens, g, base=(r + 1) & 3)
        foffs, end = place(lens, g, base=(r + 2) & 3, extra=30)
        assert end <= self.dst
        d = {"data": rand_bytes(g, self.src), "offs": offs, "lens": lens,
             "salts": g.integers(0, M64, self.N, dtype=np.uint64), "frames": np.full(self.dst, FILL, np.uint8), "foffs": foffs}
        if not host:
            d["states"] = guarded_states(self.brb, self.N, self.seed + r)
        return d

    def call(self, t, s):
        self.brb.rc4md5_frame_batch(t["states"][1:self.N + 1], t["data"], t["offs"], t["lens"], t["salts"], t["frames"],
                                    t["foffs"], stream=s, async_=True)

    def expect(self, h):
        st, frames = h["states"].copy(), h["frames"].copy()
        inner = np.ascontiguousarray(st[1:self.N + 1])
        self.orc.rc4md5_frame_batch(inner, h["data"], h["offs"], h["lens"], h["salts"], frames, h["foffs"])
        st[1:self.N + 1] = inner
        return {"states": st, "frames": frames}


def wire_buffer(orc, g, state, n):
    """What a peer holding `state` sent in n bytes: a frame of n - 30 payload bytes, or below a header's length
    plain RC4 of anything (the reader must call it invalid and go on).  -> (the peer's state after, bytes)"""
    if n < 30:
        return orc.rc4_crypt(state, rand_bytes(g, n).tobytes())
    return orc.rc4md5_frame(state, rand_bytes(g, n - 30).tobytes(), int(g.integers(0, 1 << 63)))


def tamper(g, buf, offs, lens, share=0.15):
    """One flipped bit behind the salt in about `share` of the frames."""
    for k in np.flatnonzero((g.random(len(lens)) < share) & (np.asarray(lens) > 30)):
        buf[int(offs[k]) + 8 + int(g.integers(0, int(lens[k]) - 8))] ^= 1 << int(g.integers(0, 8))


class Rc4Open(Case):
    """rc4md5_open_batch into a separate output: every replay's frames are written under the states the
    readers hold by then, some tampered with, those shorter than a header invalid."""
    carried = ("states",)
    N = RC4_N

    def __init__(self, brb, orc, pair):
        self.brb, self.orc = brb, orc
        self.options = {"rc4md5_pair": pair}
        self.size = 4 + self.N * (max(RC4_LENS) + 3) + 8
        self.seed = 0x6712

    def inputs(self, r, host):
        g = rng_of(self.seed, r)
        lens = g.choice(RC4_LENS, self.N).astype(np.uint32)
        lens[:len(RC4_LENS)] = g.permutation(RC4_LENS)
        offs, end = place(lens, g, base=(r + 1) & 3)
        assert end <= self.size
        states = host["states"] if host else guarded_states(self.brb, self.N, self.seed + r)
        data = np.full(self.size, GAP, np.uint8)
        for i in range(self.N):
            _, w = wire_buffer(self.orc, g, states[1 + i].tobytes(), int(lens[i]))
            data[int(offs[i]):int(offs[i]) + len(w)] = np.frombuffer(w, np.uint8)
        tamper(g, data, offs, lens)
        d = {"data": data, "offs": offs, "lens": lens, "out": np.full(self.size, FILL, np.uint8),
             "valid": guarded(self.N)}
        if not host:
            d["states"] = states
        return d

    def call(self, t, s):
        self.brb.rc4md5_open_batch(t["states"][1:self.N + 1], t["data"], t["offs"], t["lens"], out=t["out"],
                                   valid=t["valid"][1:self.N + 1], stream=s, async_=True)

    def expect(self, h):
        st, out, valid = h["states"].copy(), h["out"].copy(), h["valid"].copy()
        inner, dec, ok = np.ascontiguousarray(st[1:self.N + 1]), h["data"].copy(), np.zeros(self.N, np.uint8)
        self.orc.rc4md5_open_batch(inner, dec, h["offs"], h["lens"], ok)
        st[1:self.N + 1], valid[1:self.N + 1] = inner, ok
        for o, n in zip(h["offs"].tolist(), h["lens"].tolist()):
            out[o:o + n] = dec[o:o + n]
        assert 0 < int(ok.sum()) < self.N - 20                          # both verdicts, and not a few of each
        return {"states": st, "out": out, "valid": valid}


class Rc4List(Case):
    """The three RC4 list calls: 66 streams of 0..4 buffers, at least one stream with none; the lists, the
    lengths and the placement are redrawn for every replay, the states carried."""
    carried = ("states",)
    N, MOST = 66, 4

    def __init__(self, brb, orc, kind, coop):
        self.brb, self.orc, self.kind = brb, orc, kind
        self.E = sibling("rc4_lists_expect")
        self.options = {"rc4_list_coop": coop}
        self.cap = self.N * self.MOST
        self.size = 4 + self.cap * (max(RC4_LENS) + 33) + 8
        self.seed = 0x6713 + len(kind)

    def inputs(self, r, host):
        g = rng_of(self.seed, r)
        cnt = g.integers(0, self.MOST + 1, self.N)
        cnt[[(7 * (r + 2)) % self.N, 64]] = 0                           # streams with no buffer
        cnt[[0, 63, 65]] = (self.MOST, 1, 2)
        nb = int(cnt.sum())
        lens = g.choice(RC4_LENS, nb).astype(np.uint32)
        first = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
        offs, end = place(lens, g, base=(r + 1) & 3)
        states = host["states"] if host else guarded_states(self.brb, self.N, self.seed + r)
        d = {"offs": padded(offs, self.cap + 1, np.uint64), "lens": padded(lens, self.cap + 1, np.uint32), "first": first}
        if self.kind == "open":
            data = np.full(self.size, GAP, np.uint8)
            for i in range(self.N):
                s = states[1 + i].tobytes()
                for k in range(int(first[i]), int(first[i + 1])):
                    s, w = wire_buffer(self.orc, g, s, int(lens[k]))
                    data[int(offs[k]):int(offs[k]) + len(w)] = np.frombuffer(w, np.uint8)
            tamper(g, data, offs, lens)
            d.update(data=data, out=np.full(self.size, FILL, np.uint8), valid=guarded(self.cap + 1))
        elif self.kind == "frame":
            foffs, end = place(lens, g, base=(r + 2) & 3, extra=30)
            d.update(data=rand_bytes(g, self.size), salts=padded(g.integers(0, M64, nb, dtype=np.uint64), self.cap + 1, np.uint64),
                     frames=np.full(self.size, FILL, np.uint8), foffs=padded(foffs, self.cap + 1, np.uint64))
        else:
            d.update(data=rand_bytes(g, self.size), out=np.full(self.size, FILL, np.uint8))
        assert end <= self.size
        if not host:
            d["states"] = states
        return d

    def call(self, t, s):
        st, kw = t["states"][1:self.N + 1], dict(stream=s, async_=True)
        if self.kind == "crypt":
            self.brb.rc4_crypt_list_batch(st, t["data"], t["offs"], t["lens"], t["first"], out=t["out"], **kw)
        elif self.kind == "frame":
            self.brb.rc4md5_frame_list_batch(st, t["data"], t["offs"], t["lens"], t["salts"], t["frames"], t["foffs"],
                                             t["first"], **kw)
        else:
            self.brb.rc4md5_open_list_batch(st, t["data"], t["offs"], t["lens"], t["first"], out=t["out"],
                                            valid=t["valid"][1:-1], **kw)

    def expect(self, h):
        st = h["states"].copy()
        inner, args = st[1:self.N + 1], (h["offs"], h["lens"])
        want = {}
        if self.kind == "crypt":
            inner, want["out"] = self.E.expect_crypt(self.orc, inner, h["data"], *args, h["first"], out=h["out"])
        elif self.kind == "frame":
            inner, want["frames"] = self.E.expect_frame(self.orc, inner, h["data"], *args, h["salts"], h["frames"],
                                                        h["foffs"], h["first"])
        else:
            inner, want["out"], ok = self.E.expect_open(self.orc, inner, h["data"], *args, h["first"], out=h["out"])
            nb = int(h["first"][-1])
            want["valid"] = h["valid"].copy()
            want["valid"][1:1 + nb] = ok[:nb]
            assert 0 < int(ok[:nb].sum()) < nb
        st[1:self.N + 1] = inner
        want["states"] = st
        return want


# ---- streaming contexts ---------------------------------------------------------------------------------
CTX_WIDTH = {"md5": 168, "sha1": 92}
CTX_HDR = {"md5": 24, "sha1": 28}                   # state words and counters; the block buffer follows
HAVES = (0, 1, 3, 4, 55, 56, 60, 63)
CTX_N = 130


def have_of(alg, row):
    w = np.ascontiguousarray(row).view(np.uint32)
    return int(w[4]) & 63 if alg == "md5" else (int(w[5]) >> 3) & 63


def defined(alg, row):
    """The part of a context that an Update defines: state, counters, the buffered bytes."""
    return row[:CTX_HDR[alg] + have_of(alg, row)].tobytes()


class Contexts(Case):
    """What the two streaming scenarios share: 130 compat contexts that have taken 64 + have bytes, between
    guard rows, and the bytes each has taken so far (for hashlib)."""
    carried = ("ctxs",)
    N = CTX_N

    def __init__(self, brb, alg):
        self.brb, self.alg = brb, alg
        self.c_init, self.c_update, self.c_final = (getattr(brb, f"{alg}_ctx_{op}") for op in ("init", "update", "final"))
        self.msgs = None

    def fresh(self, g, track):
        rows = guarded(self.N, CTX_WIDTH[self.alg])
        msgs = []
        for i in range(self.N):
            msgs.append(rand_bytes(g, 64 + HAVES[i % len(HAVES)]).tobytes())
            self.c_init(rows[1 + i])
            self.c_update(rows[1 + i], msgs[i][:64])
            self.c_update(rows[1 + i], msgs[i][64:])
        if track:
            self.msgs = msgs
        return rows


class StreamUpdate(Contexts):
    """UpdateBatch under a graph: three replays with fresh pieces of 0..200 bytes, then one eager FinalBatch."""

    def __init__(self, brb, alg):
        super().__init__(brb, alg)
        self.size = 8 + self.N * 203 + 8
        self.seed = 0x6720

    def inputs(self, r, host):
        g = rng_of(self.seed, r)
        lens = g.integers(0, 201, self.N).astype(np.uint32)
        lens[[2, 64, 129]] = (0, 200, 0)
        offs, end = place(lens, g, base=4 + ((r + 1) & 3), gap=2)
        assert end <= self.size
        d = {"data": rand_bytes(g, self.size), "offs": offs, "lens": lens}
        if not host:
            d["ctxs"] = self.fresh(g, track=r == 0)
        return d

    def call(self, t, s):
        getattr(self.brb, self.alg + "_update_batch")(t["ctxs"][1:self.N + 1], t["data"], t["offs"], t["lens"], stream=s,
                                                      async_=True)

    def expect(self, h):
        want = h["ctxs"].copy()
        for i in range(self.N):
            piece = span(h["data"], h["offs"][i], h["lens"][i])
            self.c_update(want[1 + i], piece)
            self.msgs[i] += piece
        return {"ctxs": want}

    def compare(self, name, got, want, before, r):
        differs("ctxs guard rows", got[[0, -1]], before[[0, -1]], r)
        for i in range(1, self.N + 1):
            assert defined(self.alg, got[i]) == defined(self.alg, want[i]), (r, i - 1)
        if self.alg == "md5":
            differs("ctxs digest and string", got[:, 88:], before[:, 88:], r)     # an Update does not touch them

    def finish(self, t, host):
        import torch
        fn = getattr(self.brb, self.alg + "_final_batch")
        dig = torch.full((self.N + 2, DIGEST[self.alg]), PAD, dtype=torch.uint8, device="cuda")
        fn(t["ctxs"][1:self.N + 1], out=dig[1:self.N + 1])
        dig = dig.cpu().numpy()
        assert (dig[[0, -1]] == PAD).all()
        want = host["ctxs"].copy()
        for i in range(self.N):
            d = self.c_final(want[1 + i])
            assert dig[1 + i].tobytes() == d == getattr(hashlib, self.alg)(self.msgs[i]).digest(), i


class StreamSegments(Contexts):
    """UpdateSegmentsBatch (`lower`: the lower-text variant) under a graph: replay r finalises the items with
    i % 3 == r, a different third each time; an item takes no further segment once it is finalised, every
    other item takes 0..4 more."""
    MOST = 4

    def __init__(self, brb, alg, lower=False):
        super().__init__(brb, alg)
        self.lower = lower
        self.cap = self.N * self.MOST
        self.size = 8 + self.cap * 203 + 16
        self.seed = 0x6721 + lower

    def inputs(self, r, host):
        g = rng_of(self.seed, r)
        done = [i for i in range(self.N) if r > 0 and i % 3 < r]         # finalised by an earlier replay
        lists = seg_lists(g, self.N, self.MOST, empty=done)
        data, soff, slen, first = seg_arrays(lists, g, self.cap, self.size)
        if self.lower:
            data = g.integers(0x30, 0x80, self.size, dtype=np.uint8)
        fin = np.array([i % 3 == (r % 3 if r >= 0 else 1) for i in range(self.N)], np.uint8)
        d = {"data": data, "soff": soff, "slen": slen, "first": first, "fin": fin,
             "out": guarded(self.N, DIGEST[self.alg])}
        if self.lower:
            d["low"] = padded(g.integers(0, 2, self.cap), self.cap + 1, np.uint8)
        if not host:
            d["ctxs"] = self.fresh(g, track=r == 0)
        return d

    def call(self, t, s):
        args = (t["ctxs"][1:self.N + 1], t["data"], t["soff"], t["slen"], t["first"])
        kw = dict(final=t["fin"], out=t["out"][1:self.N + 1], stream=s, async_=True)
        if self.lower:
            self.brb.md5_update_segments_lower_batch(*args, seg_lower=t["low"], **kw)
        else:
            getattr(self.brb, self.alg + "_update_segments_batch")(*args, **kw)

    def expect(self, h):
        want, out = h["ctxs"].copy(), h["out"].copy()
        self.took = []
        for i in range(self.N):
            took = 0
            for k in range(int(h["first"][i]), int(h["first"][i + 1])):
                seg = span(h["data"], h["soff"][k], h["slen"][k])
                low = self.lower and h["low"][k]
                (self.brb.md5_ctx_update_lower if low else self.c_update)(want[1 + i], seg)
                self.msgs[i] += lowered(seg) if low else seg
                took += len(seg)
            self.took.append(took)
            if h["fin"][i]:
                d = self.c_final(want[1 + i])
                assert d == getattr(hashlib, self.alg)(self.msgs[i]).digest()
                out[1 + i] = np.frombuffer(d, np.uint8)
        self.fin = h["fin"].copy()
        return {"ctxs": want, "out": out}

    def compare(self, name, got, want, before, r):
        if name != "ctxs":
            return differs(name, got, want, r)
        differs("ctxs guard rows", got[[0, -1]], before[[0, -1]], r)
        for i in range(self.N):
            g, w, b = got[1 + i], want[1 + i], before[1 + i]
            if not self.fin[i] and not self.took[i]:
                assert np.array_equal(g, b), (r, i)                         # no bytes, no final: untouched
            elif not self.fin[i]:
                assert defined(self.alg, g) == defined(self.alg, w), (r, i)
                if self.alg == "md5":
                    assert np.array_equal(g[88:], b[88:]), (r, i)           # digest and string are not touched
            elif self.alg == "sha1":
                assert not g.any(), (r, i)                                  # a finalised context is zeroed
            else:
                assert np.array_equal(g[:24], w[:24]), (r, i)               # buf: the final state; bytes: advanced
                assert np.array_equal(g[88:137], w[88:137]), (r, i)         # digest, string[0 .. 33)
                assert np.array_equal(g[137:], b[137:]), (r, i)             # string[33 .. 64) untouched


class StreamInit(Contexts):
    """InitBatch under a graph: state and counters of 130 rows of anything, nothing else."""
    carried = ()

    def __init__(self, brb, orc, alg):
        super().__init__(brb, alg)
        self.seed = 0x6722

    def inputs(self, r, host):
        return {"ctxs": rand_bytes(rng_of(self.seed, r), (self.N + 2) * CTX_WIDTH[self.alg]).reshape(self.N + 2, -1)}

    def call(self, t, s):
        getattr(self.brb, self.alg + "_init_batch")(t["ctxs"][1:self.N + 1], n=self.N, stream=s, async_=True)

    def expect(self, h):
        want = h["ctxs"].copy()
        for i in range(1, self.N + 1):
            self.c_init(want[i])
        assert np.array_equal(want[:, CTX_HDR[self.alg]:], h["ctxs"][:, CTX_HDR[self.alg]:])
        return {"ctxs": want}


class StreamFinal(Contexts):
    """FinalBatch under a graph: 130 contexts that hold 64 + have bytes.  MD5 gets the final state, the last
    block BRB_MD5Final transformed (in), the digest and the hex string and keeps its counters and the string's
    tail; a SHA-1 context is zeroed."""
    carried = ()

    def __init__(self, brb, orc, alg):
        super().__init__(brb, alg)
        self.seed = 0x6723
        self.constant = ("ctxs",) if alg == "sha1" else ()          # all zero after every replay

    def inputs(self, r, host):
        return {"ctxs": self.fresh(rng_of(self.seed, r), track=False), "out": guarded(self.N, DIGEST[self.alg])}

    def call(self, t, s):
        getattr(self.brb, self.alg + "_final_batch")(t["ctxs"][1:self.N + 1], n=self.N, out=t["out"][1:self.N + 1], stream=s,
                                                     async_=True)

    def expect(self, h):
        want, out = h["ctxs"].copy(), h["out"].copy()
        for i in range(1, self.N + 1):
            done = h["ctxs"][i].copy()
            out[i] = np.frombuffer(self.c_final(done), np.uint8)
            if self.alg == "sha1":
                want[i] = 0
            else:
                want[i, :16], want[i, 24:137] = done[:16], done[24:137]
        return {"ctxs": want, "out": out}
