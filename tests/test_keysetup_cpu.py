"""Batched key setup (BRB_RC4_InitBatch, BRB_Blowfish_InitBatch, BRB_TransformBatcherEnableBatch): the
argument checks and refusals, which run before any device work, and the Python key-packing helpers.
No test here needs a GPU; where one is present the valid call is checked against the oracle instead
of against the refusal."""
import ctypes

import numpy as np
import pytest

KEYS = [b"k", b"cryptokey", bytes(range(1, 17)), b"\x00\xff" * 40]


def _calls(brb):
    L = brb.lib()
    return [(L.BRB_RC4_InitBatch, brb.RC4_STATE_BYTES), (L.BRB_Blowfish_InitBatch, brb.BLOWFISH_CTX_BYTES)]


def _packed(brb):
    blob, offs, lens = brb.pack_keys(KEYS)
    return blob, offs, lens, len(KEYS)


def test_symbols_exported(brb):
    assert {"BRB_RC4_InitBatch", "BRB_Blowfish_InitBatch", "BRB_TransformBatcherEnableBatch"} <= brb.exported_symbols()


def test_host_mode_without_device_refuses_with_a_reason(brb, orc):
    """No CPU fallback: without a usable device the call returns 0 and says why, and writes nothing.
    With a device the same call must produce the oracle's states and contexts."""
    L = brb.lib()
    blob, offs, lens, n = _packed(brb)
    want = {brb.RC4_STATE_BYTES: [orc.rc4_init(k) for k in KEYS],
            brb.BLOWFISH_CTX_BYTES: [orc.bf_ctx_bytes(orc.bf_init(k)) for k in KEYS]}
    have_gpu = brb.gpu_available()
    for fn, width in _calls(brb):
        out = np.full((n, width), 0xA5, np.uint8)
        rc = fn(out.ctypes.data, blob.ctypes.data, offs.ctypes.data, lens.ctypes.data, n, brb.BATCH_HOST, None)
        if have_gpu:
            assert rc == 1, L.BRB_CryptoGPU_LastError()
            assert [out[i].tobytes() for i in range(n)] == want[width]
        else:
            assert rc == 0 and L.BRB_CryptoGPU_LastError()
            assert (out == 0xA5).all()
            rc = fn(out.ctypes.data, blob.ctypes.data, offs.ctypes.data, lens.ctypes.data, n, brb.BATCH_ALL_DEVICES, None)
            assert rc == 0 and L.BRB_CryptoGPU_LastError()


@pytest.mark.parametrize("null_arg", [0, 1, 2, 3])
def test_null_argument_is_refused_and_writes_nothing(brb, null_arg):
    L = brb.lib()
    blob, offs, lens, n = _packed(brb)
    for fn, width in _calls(brb):
        out = np.full((n, width), 0xA5, np.uint8)
        args = [out.ctypes.data, blob.ctypes.data, offs.ctypes.data, lens.ctypes.data]
        args[null_arg] = None
        assert fn(*args, n, brb.BATCH_HOST, None) == -1
        assert b"NULL" in L.BRB_CryptoGPU_LastError()
        assert (out == 0xA5).all()


@pytest.mark.parametrize("where", [0, 2, 3])
def test_zero_key_length_is_refused_in_host_mode(brb, where):
    L = brb.lib()
    blob, offs, lens, n = _packed(brb)
    lens = lens.copy()
    lens[where] = 0
    for fn, width in _calls(brb):
        out = np.full((n, width), 0xA5, np.uint8)
        assert fn(out.ctypes.data, blob.ctypes.data, offs.ctypes.data, lens.ctypes.data, n, brb.BATCH_HOST, None) == -1
        assert b"zero length" in L.BRB_CryptoGPU_LastError()
        assert (out == 0xA5).all()
        assert fn(out.ctypes.data, blob.ctypes.data, offs.ctypes.data, lens.ctypes.data, n, brb.BATCH_ALL_DEVICES,
                  None) == -1
        assert (out == 0xA5).all()


def test_empty_batch_is_done(brb):
    for fn, _ in _calls(brb):
        assert fn(None, None, None, None, 0, brb.BATCH_HOST, None) == 1
        assert fn(None, None, None, None, 0, brb.BATCH_DEVICE | brb.BATCH_ASYNC, None) == 1


def test_all_devices_needs_host_pointers(brb):
    L = brb.lib()
    blob, offs, lens, n = _packed(brb)
    for fn, width in _calls(brb):
        out = np.full((n, width), 0xA5, np.uint8)
        assert fn(out.ctypes.data, blob.ctypes.data, offs.ctypes.data, lens.ctypes.data, n,
                  brb.BATCH_DEVICE | brb.BATCH_ALL_DEVICES, None) == -1
        assert b"ALL_DEVICES" in L.BRB_CryptoGPU_LastError()
        assert (out == 0xA5).all()


def test_oversized_key_count_is_refused(brb):
    L = brb.lib()
    b = ctypes.create_string_buffer(64)
    for fn, _ in _calls(brb):
        assert fn(b, b, b, b, 1 << 33, brb.BATCH_DEVICE, None) == -1
        assert b"split the batch" in L.BRB_CryptoGPU_LastError()


def test_enable_batch_null_batcher(brb):
    L = brb.lib()
    blob, offs, lens, n = _packed(brb)
    conns = np.arange(n, dtype=np.uint32)
    assert L.BRB_TransformBatcherEnableBatch(None, conns.ctypes.data, n, blob.ctypes.data, offs.ctypes.data,
                                             lens.ctypes.data) == -1
    assert L.BRB_CryptoGPU_LastError()
    assert L.BRB_TransformBatcherEnableBatch(None, None, 0, None, None, None) == -1


def test_pack_keys_round_trip(brb):
    rng = np.random.default_rng(7)
    keys = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in (1, 1, 1, 2, 5, 9, 16, 255, 256, 257, 1000)]
    blob, offs, lens = brb.pack_keys(keys)
    assert blob.dtype == np.uint8 and offs.dtype == np.uint64 and lens.dtype == np.uint32
    assert blob.size == sum(len(k) for k in keys) and offs[0] == 0
    assert [int(x) for x in lens] == [len(k) for k in keys]
    assert all(int(offs[i + 1]) == int(offs[i]) + len(keys[i]) for i in range(len(keys) - 1))   # back to back
    assert {int(o) & 3 for o in offs} == {0, 1, 2, 3}
    assert brb.unpack_keys(blob, offs, lens) == keys
    # one key shared by every record: all offsets equal
    shared = brb.unpack_keys(np.frombuffer(b"sharedkey", np.uint8), np.zeros(4, np.uint64), np.full(4, 9, np.uint32))
    assert shared == [b"sharedkey"] * 4
    one, o1, l1 = brb.pack_keys([b"xyz"])
    assert brb.unpack_keys(one, o1, l1) == [b"xyz"] and brb.pack_keys([])[0].size == 0
