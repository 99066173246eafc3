"""Keyed Blowfish ECB and the MemBuffer batch calls: the argument checks and refusals, which run before
any device work, and a pure-Python check that the shapes of tests/test_blowfish_keyed.py hit the edges
they claim.  No test here needs a GPU; where one is present the valid call is checked against the
oracle instead of against the refusal."""
import importlib.util
import os

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("keyed_shapes", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                           "test_blowfish_keyed.py"))
shapes = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(shapes)

KEYS = [b"k", b"cryptokey", bytes(range(1, 17)), b"\x00\xff" * 40]
PAD = np.uint64(0xA5A5A5A5A5A5A5A5)


def _keyed_calls(brb):
    L = brb.lib()
    return [(L.BRB_Blowfish_EncryptBatchKeyed, False), (L.BRB_Blowfish_DecryptBatchKeyed, True)]


def _membuf_calls(brb):
    L = brb.lib()
    return [(L.BRB_MemBufferEncryptBatch, False), (L.BRB_MemBufferDecryptBatch, True)]


def _keyed_args(brb):
    """4 records of 3, 0, 1, 2 blocks with guard words around them, one context per record."""
    ctxs = brb.blowfish_contexts([brb.blowfish_init(k) for k in KEYS])
    cnt = np.array([3, 0, 1, 2], np.uint32)
    woff = np.array([1, 8, 9, 12], np.uint64)
    words = np.full(18, PAD, np.uint64)
    for o, c in zip(woff, cnt):
        words[int(o): int(o) + 2 * int(c)] = np.arange(2 * int(c), dtype=np.uint64) + np.uint64((1 << 40) + 7)
    return ctxs, words, woff, cnt


def _membuf_args():
    """3 buffers of 40, 0 and 9 bytes, grown and zero-filled, 0x5A between them."""
    sizes = np.array([40, 0, 9], np.uint64)
    offs = np.array([16, 144, 272], np.uint64)
    data = np.full(400, 0x5A, np.uint8)
    for o, s in zip(offs, sizes):
        data[int(o): int(o) + shapes.mb_room(int(s), 0)] = 0
        data[int(o): int(o) + int(s)] = np.arange(1, int(s) + 1, dtype=np.uint8)
    return data, offs, sizes


def test_symbols_exported(brb):
    assert {"BRB_Blowfish_EncryptBatchKeyed", "BRB_Blowfish_DecryptBatchKeyed", "BRB_MemBufferEncryptBatch",
            "BRB_MemBufferDecryptBatch"} <= brb.exported_symbols()
    for name in ("blowfish_encrypt_batch_keyed", "blowfish_decrypt_batch_keyed", "membuf_encrypt_batch",
                 "membuf_decrypt_batch"):
        assert callable(getattr(brb, name))


@pytest.mark.parametrize("null_arg", [0, 3, 4, 5])
def test_keyed_null_argument_is_refused_and_writes_nothing(brb, null_arg):
    L = brb.lib()
    ctxs, words, woff, cnt = _keyed_args(brb)
    before = words.copy()
    for fn, _ in _keyed_calls(brb):
        args = [ctxs.ctypes.data, 4, None, words.ctypes.data, woff.ctypes.data, cnt.ctypes.data]
        args[null_arg] = None
        assert fn(*args, 4, brb.BATCH_HOST, None) == -1
        assert b"NULL" in L.BRB_CryptoGPU_LastError()
        assert fn(*args, 4, brb.BATCH_DEVICE, None) == -1
    assert np.array_equal(words, before)


@pytest.mark.parametrize("null_arg", [0, 1, 2, 4, 8])
def test_membuf_null_argument_is_refused_and_writes_nothing(brb, null_arg):
    L = brb.lib()
    data, offs, sizes = _membuf_args()
    before = data.copy()
    seeds, new = np.array([0x4FD9], np.uint32), np.full(3, 99, np.uint64)
    for fn, _ in _membuf_calls(brb):
        args = [data.ctypes.data, offs.ctypes.data, sizes.ctypes.data, None, seeds.ctypes.data, 1, None, 3,
                new.ctypes.data]
        args[null_arg] = None
        assert fn(*args, brb.BATCH_HOST, None) == -1
        assert b"NULL" in L.BRB_CryptoGPU_LastError()
    assert np.array_equal(data, before) and (new == 99).all()


def test_empty_batch_is_done(brb):
    for fn, _ in _keyed_calls(brb):
        assert fn(None, 0, None, None, None, None, 0, brb.BATCH_HOST, None) == 1
        assert fn(None, 0, None, None, None, None, 0, brb.BATCH_DEVICE | brb.BATCH_ASYNC, None) == 1
    for fn, _ in _membuf_calls(brb):
        assert fn(None, None, None, None, None, 0, None, 0, None, brb.BATCH_HOST, None) == 1
        assert fn(None, None, None, None, None, 0, None, 0, None, brb.BATCH_DEVICE, None) == 1


def test_all_devices_needs_host_pointers(brb):
    L = brb.lib()
    ctxs, words, woff, cnt = _keyed_args(brb)
    before = words.copy()
    for fn, _ in _keyed_calls(brb):
        assert fn(ctxs.ctypes.data, 4, None, words.ctypes.data, woff.ctypes.data, cnt.ctypes.data, 4,
                  brb.BATCH_DEVICE | brb.BATCH_ALL_DEVICES, None) == -1
        assert b"ALL_DEVICES" in L.BRB_CryptoGPU_LastError()
    assert np.array_equal(words, before)
    data, offs, sizes = _membuf_args()
    dbefore = data.copy()
    seeds, new = np.array([0x4FD9], np.uint32), np.full(3, 99, np.uint64)
    for fn, _ in _membuf_calls(brb):
        assert fn(data.ctypes.data, offs.ctypes.data, sizes.ctypes.data, None, seeds.ctypes.data, 1, None, 3,
                  new.ctypes.data, brb.BATCH_DEVICE | brb.BATCH_ALL_DEVICES, None) == -1
        assert b"ALL_DEVICES" in L.BRB_CryptoGPU_LastError()
    assert np.array_equal(data, dbefore) and (new == 99).all()


def test_keyed_host_mode_argument_checks(brb):
    """ctx_index[i] >= n_ctx, and a NULL ctx_index with n_ctx != n_rec: -1, nothing written.  Device mode:
    words or ctxs not 8-byte aligned: -1 before any device work."""
    L = brb.lib()
    ctxs, words, woff, cnt = _keyed_args(brb)
    before = words.copy()
    for fn, _ in _keyed_calls(brb):
        for bad in (0, 1, 3):               # also on the record of 0 blocks
            idx = np.array([0, 1, 2, 3], np.uint32)
            idx[bad] = 4
            assert fn(ctxs.ctypes.data, 4, idx.ctypes.data, words.ctypes.data, woff.ctypes.data, cnt.ctypes.data, 4,
                      brb.BATCH_HOST, None) == -1
            assert b"out of range" in L.BRB_CryptoGPU_LastError()
            assert fn(ctxs.ctypes.data, 4, idx.ctypes.data, words.ctypes.data, woff.ctypes.data, cnt.ctypes.data, 4,
                      brb.BATCH_ALL_DEVICES, None) == -1
        for n_ctx in (0, 3, 5):
            assert fn(ctxs.ctypes.data, n_ctx, None, words.ctypes.data, woff.ctypes.data, cnt.ctypes.data, 4,
                      brb.BATCH_HOST, None) == -1
            assert b"n_ctx" in L.BRB_CryptoGPU_LastError()
        wrap = woff.copy()
        wrap[2] = (1 << 61) + 5
        assert fn(ctxs.ctypes.data, 4, None, words.ctypes.data, wrap.ctypes.data, cnt.ctypes.data, 4, brb.BATCH_HOST,
                  None) == -1
        assert b"wraps" in L.BRB_CryptoGPU_LastError()
        assert fn(ctxs.ctypes.data, 4, None, words.ctypes.data + 4, woff.ctypes.data, cnt.ctypes.data, 4,
                  brb.BATCH_DEVICE, None) == -1
        assert b"aligned" in L.BRB_CryptoGPU_LastError()
        assert fn(ctxs.ctypes.data + 2, 4, None, words.ctypes.data, woff.ctypes.data, cnt.ctypes.data, 4,
                  brb.BATCH_DEVICE | brb.BATCH_ASYNC, None) == -1
    assert np.array_equal(words, before)


def test_membuf_host_mode_argument_checks(brb):
    """decrypt sizes[i] < offsets[i], seed_index out of range, n_seeds neither 1 nor n_buf with a NULL
    seed_index, n_seeds == 0: -1, nothing written.  Device mode: data not 8-byte aligned: -1."""
    L = brb.lib()
    data, offs, sizes = _membuf_args()
    before = data.copy()
    new = np.full(3, 99, np.uint64)
    seeds = np.array([1, 2, 3, 4], np.uint32)
    off8 = np.array([0, 8, 0], np.uint64)
    enc, dec = [fn for fn, _ in _membuf_calls(brb)]

    def call(fn, offsets, n_seeds, seed_index, flags=brb.BATCH_HOST, shift=0):
        return fn(data.ctypes.data + shift, offs.ctypes.data, sizes.ctypes.data, None if offsets is None else offsets.ctypes.data,
                  seeds.ctypes.data, n_seeds, None if seed_index is None else seed_index.ctypes.data, 3, new.ctypes.data,
                  flags, None)

    assert call(dec, off8, 1, None) == -1 and b"< offset" in L.BRB_CryptoGPU_LastError()     # sizes[1] = 0 < 8
    for fn in (enc, dec):
        assert call(fn, None, 2, np.array([0, 1, 2], np.uint32)) == -1 and b"out of range" in L.BRB_CryptoGPU_LastError()
        for n_seeds in (0, 2, 4):
            assert call(fn, None, n_seeds, None) == -1 and b"n_seeds" in L.BRB_CryptoGPU_LastError()
        assert call(fn, None, 1, None, brb.BATCH_DEVICE, shift=4) == -1 and b"aligned" in L.BRB_CryptoGPU_LastError()
    assert np.array_equal(data, before) and (new == 99).all()


def test_valid_calls_without_device_refuse_with_a_reason(brb, orc):
    """No CPU fallback: without a usable device a valid call returns 0 and says why, and leaves the
    buffers untouched.  With a device the same call must equal the oracle."""
    L = brb.lib()
    have_gpu = brb.gpu_available()
    ctxs, words, woff, cnt = _keyed_args(brb)
    octx = [orc.bf_init(k) for k in KEYS]
    for fn, decrypt in _keyed_calls(brb):
        for flags in (brb.BATCH_HOST, brb.BATCH_ALL_DEVICES):
            w = words.copy()
            rc = fn(ctxs.ctypes.data, 4, None, w.ctypes.data, woff.ctypes.data, cnt.ctypes.data, 4, flags, None)
            if have_gpu:
                assert rc == 1, L.BRB_CryptoGPU_LastError()
                want = words.copy()
                for i in range(4):
                    seg = want[int(woff[i]): int(woff[i]) + 2 * int(cnt[i])].copy()
                    orc.bf_ecb(octx[i], seg, decrypt)
                    want[int(woff[i]): int(woff[i]) + 2 * int(cnt[i])] = seg
                assert np.array_equal(w, want)
            else:
                assert rc == 0 and L.BRB_CryptoGPU_LastError()
                assert np.array_equal(w, words)
    data, offs, sizes = _membuf_args()
    seeds = np.array([0x4FD9], np.uint32)
    for fn, decrypt in _membuf_calls(brb):
        d, new = data.copy(), np.full(3, 99, np.uint64)
        rc = fn(d.ctypes.data, offs.ctypes.data, sizes.ctypes.data, None, seeds.ctypes.data, 1, None, 3, new.ctypes.data,
                brb.BATCH_HOST, None)
        if have_gpu:
            assert rc == 1, L.BRB_CryptoGPU_LastError()
            for i in range(3):
                b = bytearray(data[int(offs[i]): int(offs[i]) + 112].tobytes())
                ns = (orc.membuf_decrypt if decrypt else orc.membuf_encrypt)(b, int(sizes[i]), 0x4FD9, 0)
                assert int(new[i]) == ns and d[int(offs[i]): int(offs[i]) + 112].tobytes() == bytes(b)
        else:
            assert rc == 0 and L.BRB_CryptoGPU_LastError()
            assert np.array_equal(d, data) and (new == 99).all()


# ---- the GPU file's shapes hit what they claim ----------------------------------------------------
def test_shapes_cover_group_and_lane_edges():
    S, W = shapes.SLOTS, shapes.SLOT_LANES
    assert (S, W) == (16, 64)
    # record counts: one record, one less / exactly / one more than a group, more than two groups
    assert {n % S for n in shapes.N_RECS} >= {1, S - 1, 0} and max(shapes.N_RECS) > 2 * S
    assert {(n + S - 1) // S for n in shapes.N_RECS} >= {1, 2, 3}
    # block counts: none, fewer than / exactly / more than the slot's lanes, more than two rounds of them
    assert {c % W for c in shapes.COUNTS} >= {0, 1, 2, W - 1} and {c // W for c in shapes.COUNTS} >= {0, 1, 2}
    # both ILP-2 tails: a lane whose second block is missing (65..127 blocks) and whose first is (<= 64)
    assert any(W < c < 2 * W for c in shapes.COUNTS) and any(0 < c <= W for c in shapes.COUNTS)
    for n in shapes.N_RECS:
        c = shapes.edge_counts(n)
        assert len(c) == n and set(c.tolist()) <= set(shapes.COUNTS)
        if n >= S:
            assert c[:S - 1].tolist() == [0] * (S - 1) and c[S - 1] > W     # all 0 except the last slot
        if n % S >= 7:
            assert set(c[n - n % S:].tolist()) == set(shapes.COUNTS)        # every count inside one partial group
    assert set(shapes.edge_counts(33)[S:2 * S].tolist()) == set(shapes.COUNTS)   # and inside one full group


def test_shapes_cover_both_word_parities_and_memory_order():
    for n in shapes.N_RECS:
        c = shapes.edge_counts(n)
        woff, total = shapes.layout(c, n)
        ends = woff + 2 * c.astype(np.uint64)
        order = np.argsort(woff, kind="stable")
        assert woff[order[0]] >= 1 and ends.max() < total                    # guard words before and after
        assert (woff[order][1:] > ends[order][:-1]).all()                    # and between: no overlap
        if n > 1:
            assert {int(o) & 1 for o in woff} == {0, 1}
    c = shapes.edge_counts(33)[shapes.SLOTS:]
    woff, _ = shapes.layout(c, 5, shuffle=True)
    assert (np.diff(woff.astype(np.int64)) < 0).any()
    assert {int(o) & 1 for o, k in zip(woff, c) if k} == {0, 1}


@pytest.mark.parametrize("stride", [1, 3, 256])
def test_reuse_shape_is_a_a_b_a(stride):
    S = shapes.SLOTS
    idx, cnt = shapes.reuse_shape(stride)
    assert len(idx) == 4 * stride * S
    for w in {0, stride - 1}:
        for k in range(S):
            seq = [int(idx[(w + r * stride) * S + k]) for r in range(4)]
            assert seq == [k, k, S + k, k]
            has = [int(cnt[(w + r * stride) * S + k]) > 0 for r in range(4)]
            assert has == [True, k != 3, k != 5, True]
    assert set(cnt.tolist()) == {0, 1, 2}


def test_membuf_shapes():
    cases = shapes.membuf_cases([0, 8, 3])
    assert len(cases) == 30 and {s for s, _ in cases} == set(shapes.MB_SIZES) == {0, 1, 7, 8, 15, 16, 17, 1000, 1023, 1024}
    # both roundings of the +2 words to pairs occur, and more buffers than one group of 16
    assert {((s + o) // 8 + 2) % 2 for s, o in cases} == {0, 1} and len(shapes.membuf_cases([0, 8])) > shapes.SLOTS
    for s, o in cases:
        assert shapes.mb_room(s, o) == o + shapes.membuf_span(16 * (((s + o) // 8 + 3) // 2))
