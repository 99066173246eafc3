"""Batched key setup on the GPU: BRB_RC4_InitBatch, BRB_Blowfish_InitBatch and
BRB_TransformBatcherEnableBatch against the oracle's per-key BRB_RC4_Init / BRB_Blowfish_Init, byte
for byte over the whole state or context, at the smallest shapes where the kernels can go wrong:
one key, one less / exactly / one more than a wave and a workgroup (RC4: 256 keys per workgroup;
Blowfish: 16), more than one workgroup, key lengths around every wrap point, keys at every byte
alignment, and one key shared by all records."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RC4_G = 256                  # keys per workgroup of the RC4 key-schedule kernel
BF_G = 16                    # keys per workgroup of the Blowfish key-schedule kernel (its LDS budget)
RC4_LENS = [1, 2, 5, 9, 16, 255, 256, 257, 1000]
BF_LENS = [1, 2, 3, 4, 5, 7, 8, 16, 56, 64, 71, 72, 73, 100]
PAD = 0xA5


@pytest.fixture(scope="module")
def torch_dev(brb):
    import torch
    assert torch.cuda.is_available(), "no HIP device visible to torch"
    assert brb.gpu_available(), brb.lib().BRB_CryptoGPU_LastError()
    return torch


def _keys(n, lens, seed):
    """n keys whose lengths walk through `lens` (mixed within the batch), packed back to back."""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, lens[(i + seed) % len(lens)], dtype=np.uint8).tobytes() for i in range(n)]


def _to_dev(torch, blob, offs, lens):
    return (torch.from_numpy(blob).cuda(), torch.from_numpy(offs.view(np.int64)).cuda(),
            torch.from_numpy(lens.view(np.int32)).cuda())


def _run(brb, torch, fn, width, blob, offs, lens, device, **kw):
    """fn into rows 1 .. n of an (n + 2)-row array pre-filled with PAD; returns (rows, guard rows)."""
    n = len(offs)
    if device:
        big = torch.full((n + 2, width), PAD, dtype=torch.uint8, device="cuda")
        stream = kw.get("stream")
        if stream is not None:
            torch.cuda.synchronize()          # the inputs were made on the default stream
        fn(*_to_dev(torch, blob, offs, lens), out=big[1:n + 1], **kw)
        if stream is not None:
            stream.synchronize()
        big = big.cpu().numpy()
    else:
        big = np.full((n + 2, width), PAD, np.uint8)
        fn(blob, offs, lens, out=big[1:n + 1], **kw)
    return big[1:n + 1], big[[0, n + 1]]


def _rc4_want(orc, keys):
    return np.frombuffer(b"".join(orc.rc4_init(k) for k in keys), np.uint8).reshape(len(keys), 264)


def _bf_want(orc, keys):
    return np.frombuffer(b"".join(orc.bf_ctx_bytes(orc.bf_init(k)) for k in keys), np.uint8).reshape(len(keys), 8336)


def _check_rc4(brb, orc, keys, got, guard):
    assert (guard == PAD).all(), "a row outside states was written"
    assert (got[:, 256:] == 0).all(), "index1, index2 and the six bytes after them must be written as zero"
    want = _rc4_want(orc, keys)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (bad[:8], [len(keys[i]) for i in bad[:8]])
    assert np.array_equal(got, brb.rc4_states(keys))


def _check_bf(orc, keys, got, guard):
    assert (guard == PAD).all(), "a row outside ctxs was written"
    q = np.ascontiguousarray(got).view(np.uint64)
    assert ((q >> np.uint64(32)) != 0).any(axis=1).all(), "every context carries 64-bit carries in its high halves"
    want = _bf_want(orc, keys)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (bad[:8], [len(keys[i]) for i in bad[:8]])


# ---- RC4 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_rc4_init_batch(brb, orc, torch_dev, n, device):
    keys = _keys(n, RC4_LENS, n)
    blob, offs, lens = brb.pack_keys(keys)
    if n >= 63:
        assert {int(o) & 3 for o in offs} == {0, 1, 2, 3}
    got, guard = _run(brb, torch_dev, brb.rc4_init_batch, 264, blob, offs, lens, device)
    _check_rc4(brb, orc, keys, got, guard)


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_rc4_shared_key(brb, orc, torch_dev, device):
    """The daemon's normal case: one key for every connection (all offsets equal), here at an odd
    address inside the blob."""
    n, key = RC4_G + 44, b"one key for every connection"
    blob = np.frombuffer(b"\xee\xee\xee" + key + b"\xee", np.uint8).copy()
    offs, lens = np.full(n, 3, np.uint64), np.full(n, len(key), np.uint32)
    got, guard = _run(brb, torch_dev, brb.rc4_init_batch, 264, blob, offs, lens, device)
    _check_rc4(brb, orc, [key] * n, got, guard)


def test_rc4_golden_keys(brb, golden, torch_dev):
    """States made by the batch call encrypt the published vectors (tests/golden/rc4.json) to their
    recorded ciphertexts, and the recorded streams' keys advance to their recorded states."""
    kat = golden["rc4"]["kat"]
    keys = [bytes.fromhex(v["key"]) for v in kat]
    states = brb.rc4_init_batch(*brb.pack_keys(keys))
    data, offs, lens = brb.pack_keys([bytes.fromhex(v["plain"]) for v in kat])
    brb.rc4_crypt_batch(states, data, offs, lens)
    assert [bytes(p).hex() for p in brb.unpack_keys(data, offs, lens)] == [v["cipher"] for v in kat]
    streams = golden["rc4"]["streams"]
    states = brb.rc4_init_batch(*brb.pack_keys([bytes.fromhex(v["key"]) for v in streams]))
    data, offs, lens = brb.pack_keys([bytes.fromhex(v["data"]) for v in streams])
    brb.rc4_crypt_batch(states, data, offs, lens)
    assert [bytes(p).hex() for p in brb.unpack_keys(data, offs, lens)] == ["".join(v["out"]) for v in streams]
    assert [states[i].tobytes().hex() for i in range(len(streams))] == [v["state_after"] for v in streams]


# ---- Blowfish ----------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("n", [1, BF_G - 1, BF_G, BF_G + 1, 2 * BF_G + 1])
def test_blowfish_init_batch(brb, orc, torch_dev, n, device):
    keys = _keys(n, BF_LENS, n)
    if n == 1:
        keys = [_keys(1, [73], 5)[0]]          # a lone key longer than the 72 bytes used
    blob, offs, lens = brb.pack_keys(keys)
    got, guard = _run(brb, torch_dev, brb.blowfish_init_batch, 8336, blob, offs, lens, device)
    _check_bf(orc, keys, got, guard)


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_blowfish_every_key_length(brb, orc, torch_dev, device):
    """Every listed length at every byte alignment: 4 and 64 are the MemBuffer's two lengths, 73 and
    100 show that bytes past 72 are ignored and that the key cursor does not wrap early."""
    rng = np.random.default_rng(11)
    keys = [rng.integers(0, 256, L, dtype=np.uint8).tobytes() for L in BF_LENS]
    blob, offs, lens = brb.pack_keys(keys)
    for shift in range(4):
        b = np.concatenate([np.full(shift, 0x11, np.uint8), blob, np.full(5, 0x22, np.uint8)])
        got, guard = _run(brb, torch_dev, brb.blowfish_init_batch, 8336, b, offs + np.uint64(shift), lens, device)
        _check_bf(orc, keys, got, guard)
    # bytes past the first 72 do not matter
    long_a, long_b = keys[-1], keys[-1][:72] + bytes(28)
    got, _ = _run(brb, torch_dev, brb.blowfish_init_batch, 8336, *brb.pack_keys([long_a, long_b]), device)
    assert np.array_equal(got[0], got[1])


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_blowfish_shared_key(brb, orc, torch_dev, device):
    n, key = BF_G + 3, b"shared blowfish key!x"
    blob = np.frombuffer(b"\xee" + key + b"\xee\xee", np.uint8).copy()
    offs, lens = np.full(n, 1, np.uint64), np.full(n, len(key), np.uint32)
    got, guard = _run(brb, torch_dev, brb.blowfish_init_batch, 8336, blob, offs, lens, device)
    _check_bf(orc, [key] * n, got, guard)


def test_blowfish_golden_contexts(brb, golden, torch_dev):
    ctxs = golden["blowfish64"]["contexts"]
    got = brb.blowfish_init_batch(*brb.pack_keys([bytes.fromhex(c["key"]) for c in ctxs]))
    assert [hashlib.sha256(got[i].tobytes()).hexdigest() for i in range(len(ctxs))] == [c["sha256"] for c in ctxs]


# ---- consumers: device mode, no host round trip between key setup and use -----------------------------
def test_rc4_crypt_on_batch_made_states(brb, orc, torch_dev):
    torch = torch_dev
    n, L = 65, 100
    keys = _keys(n, RC4_LENS, 3)
    states = brb.rc4_init_batch(*_to_dev(torch, *brb.pack_keys(keys)))
    plain = np.random.default_rng(5).integers(0, 256, n * L, dtype=np.uint8)
    data = torch.from_numpy(plain.copy()).cuda()
    offs = torch.arange(n, dtype=torch.int64, device="cuda") * L
    lens = torch.full((n,), L, dtype=torch.int32, device="cuda")
    brb.rc4_crypt_batch(states, data, offs, lens)
    got = data.cpu().numpy()
    for i, k in enumerate(keys):
        st, out = orc.rc4_crypt(orc.rc4_init(k), plain[i * L:(i + 1) * L].tobytes())
        assert got[i * L:(i + 1) * L].tobytes() == out, i
        assert states[i].cpu().numpy().tobytes() == st, i


def test_blowfish_ecb_on_batch_made_contexts(brb, orc, torch_dev):
    torch = torch_dev
    keys = _keys(5, [4, 64, 16, 73, 7], 0)
    ctxs = brb.blowfish_init_batch(*_to_dev(torch, *brb.pack_keys(keys)))
    w = np.random.default_rng(9).integers(0, 2**63, 2 * 2048, dtype=np.uint64)
    for i in (0, 2, 4):
        dw = torch.from_numpy(w.view(np.int64).copy()).cuda()
        brb.blowfish_encrypt_batch(ctxs[i], dw)
        want = orc.bf_ecb(orc.bf_init(keys[i]), w.copy())
        assert np.array_equal(dw.cpu().numpy().view(np.uint64), want), i
        brb.blowfish_decrypt_batch(ctxs[i], dw)
        assert np.array_equal(dw.cpu().numpy().view(np.uint64), w), i


# ---- async and all devices ---------------------------------------------------------------------------
def test_async_on_a_side_stream(brb, orc, torch_dev):
    torch = torch_dev
    s = torch.cuda.Stream()
    keys = _keys(RC4_G + 1, RC4_LENS, 21)
    got, guard = _run(brb, torch, brb.rc4_init_batch, 264, *brb.pack_keys(keys), True, stream=s, async_=True)
    _check_rc4(brb, orc, keys, got, guard)
    keys = _keys(BF_G + 1, BF_LENS, 22)
    got, guard = _run(brb, torch, brb.blowfish_init_batch, 8336, *brb.pack_keys(keys), True, stream=s, async_=True)
    _check_bf(orc, keys, got, guard)


def test_all_devices_unequal_parts(brb, orc, torch_dev):
    with brb.TestOption("devices", 3):
        keys = _keys(7, RC4_LENS, 31)                      # parts of 2, 2 and 3 keys
        got, guard = _run(brb, torch_dev, brb.rc4_init_batch, 264, *brb.pack_keys(keys), False, all_devices=True)
        _check_rc4(brb, orc, keys, got, guard)
        keys = _keys(2 * BF_G + 1, BF_LENS, 32)            # parts of 11, 11 and 11 keys, none a multiple of 16
        got, guard = _run(brb, torch_dev, brb.blowfish_init_batch, 8336, *brb.pack_keys(keys), False, all_devices=True)
        _check_bf(orc, keys, got, guard)


# ---- the transform batcher --------------------------------------------------------------------------
C = 300


def _conns_and_keys(seed):
    rng = np.random.default_rng(seed)
    conns = [int(c) for c in rng.permutation(C)[:257]]
    return conns, _keys(len(conns), RC4_LENS, seed)


def _round(brb, orc, b, conns, key_of, rnd):
    """One round: every connection reads a frame its peer wrote with a fresh state of its key and
    writes one payload.  Returns the flush results."""
    for c in conns:
        payload = bytes([c & 255, rnd]) * (1 + c % 40)
        _, frame = orc.rc4md5_frame(orc.rc4_init(key_of[c]), payload, 1000 * rnd + c)
        assert b.read(c, frame) == 1, brb.lib().BRB_CryptoGPU_LastError()
        assert b.write(c, payload, 7 * c + rnd) == 1, brb.lib().BRB_CryptoGPU_LastError()
    return b.flush()


@pytest.mark.parametrize("variant", ["plain", "zero_copy", "pipelined", "all_devices"])
def test_enable_batch_equals_enable_loop(brb, orc, torch_dev, variant):
    kw = {"zero_copy": variant == "zero_copy", "pipelined": variant == "pipelined", "all_devices": variant == "all_devices"}
    conns, keys = _conns_and_keys(41)
    key_of = dict(zip(conns, keys))
    with brb.TestOption("devices", 2):
        b1 = brb.TransformBatcher(C, 4 << 20, brb.CRYPTO_FUNC_RC4_MD5, **kw)
        b2 = brb.TransformBatcher(C, 4 << 20, brb.CRYPTO_FUNC_RC4_MD5, **kw)
        try:
            b1.enable_batch(conns, keys)
            for c in conns:
                b2.enable(c, key_of[c])
            for c in conns:
                want = orc.rc4_init(key_of[c])
                assert b1.state(c, brb.OP_READ) == want and b1.state(c, brb.OP_WRITE) == want, c
            unlisted = next(c for c in range(C) if c not in key_of)
            assert b1.read(unlisted, b"x" * 40) == -1
            r1 = _round(brb, orc, b1, conns, key_of, 1)
            r2 = _round(brb, orc, b2, conns, key_of, 1)
            assert len(r1) == 2 * len(conns) and r1 == r2
            for conn, op, out, valid in r1:
                assert valid == 1, (conn, op)
                if op == brb.OP_READ:
                    assert out[30:] == bytes([conn & 255, 1]) * (1 + conn % 40), conn
        finally:
            b1.close()
            b2.close()


def test_enable_batch_rekeys(brb, orc, torch_dev):
    """A connection whose states a round has advanced gets fresh states from a second enable_batch,
    and the next round runs on them; the connections not listed keep their advanced states."""
    conns = list(range(8))
    key_of = {c: bytes([c + 1]) * (c + 3) for c in conns}
    b = brb.TransformBatcher(8, 1 << 20, brb.CRYPTO_FUNC_RC4_MD5)
    try:
        b.enable_batch(conns, [key_of[c] for c in conns])
        w = {c: orc.rc4_init(key_of[c]) for c in conns}          # oracle model of the write states
        for c in conns:
            assert b.write(c, b"first round " * (c + 1), c) == 1
        for conn, _, out, _ in b.flush():
            w[conn], frame = orc.rc4md5_frame(w[conn], b"first round " * (conn + 1), conn)
            assert out == frame
        assert b.state(2, brb.OP_WRITE) == w[2] != orc.rc4_init(key_of[2])
        fresh = {2: b"a new key for two", 5: b"five"}
        b.enable_batch(list(fresh), list(fresh.values()))
        for c, k in fresh.items():
            w[c] = orc.rc4_init(k)
            assert b.state(c, brb.OP_WRITE) == w[c] and b.state(c, brb.OP_READ) == w[c]
        assert b.state(3, brb.OP_WRITE) == w[3]
        for c in conns:
            assert b.write(c, b"second round", 100 + c) == 1
        for conn, _, out, _ in b.flush():
            w[conn], frame = orc.rc4md5_frame(w[conn], b"second round", 100 + conn)
            assert out == frame, conn
    finally:
        b.close()


def test_enable_batch_refusals_change_nothing(brb, orc, torch_dev):
    b = brb.TransformBatcher(8, 1 << 20, brb.CRYPTO_FUNC_RC4_MD5)
    try:
        b.enable_batch([0, 1, 2], [b"zero", b"one", b"two"])
        assert b.write(1, b"advance the state", 9) == 1 and len(b.flush()) == 1
        before = (b.state(1, brb.OP_READ), b.state(1, brb.OP_WRITE))
        assert before[1] != orc.rc4_init(b"one")
        for bad in ([1, 3, 1], [3, 1, 8], [1, 3, 3]):
            with pytest.raises(RuntimeError, match="returned -1"):
                b.enable_batch(bad, [b"x", b"y", b"z"])
            assert (b.state(1, brb.OP_READ), b.state(1, brb.OP_WRITE)) == before
            assert b.read(3, b"y" * 40) == -1                       # still not enabled
        with pytest.raises(RuntimeError, match="returned -1"):
            b.enable_batch([1, 3], [b"x", b""])                     # a zero key length
        assert (b.state(1, brb.OP_READ), b.state(1, brb.OP_WRITE)) == before
        assert b.write(1, b"still usable", 1) == 1 and len(b.flush()) == 1
    finally:
        b.close()
