"""Blowfish ECB with a context per record (BRB_Blowfish_EncryptBatchKeyed / DecryptBatchKeyed) and the
MemBuffer batch calls (BRB_MemBufferEncryptBatch / DecryptBatch), byte for byte against the oracle:
per record orc.bf_init + orc.bf_ecb, per buffer orc.membuf_encrypt / orc.membuf_decrypt, guard words
and guard bytes included in every comparison.

The kernel's constants are 16 context slots (records) per group and 64 lanes per record, so the
shapes sit on those edges: record counts 1, 15, 16, 17, 33 and block counts 0, 1, 2, 63, 64, 65, 129
mixed inside a group, one group all 0 except its last slot.  The shape builders at the top are plain
Python; tests/test_blowfish_keyed_cpu.py checks, without a GPU, that they hit what they claim."""
import numpy as np
import pytest

SLOTS = 16                   # records per group (context slots of the LDS image)
SLOT_LANES = 64              # lanes per record
N_RECS = [1, 15, 16, 17, 33]
COUNTS = [0, 1, 2, 63, 64, 65, 129]
GUARD = np.uint64(0xA5A5A5A5A5A5A5A5)
N_KEYS = 40
MB_SIZES = [0, 1, 7, 8, 15, 16, 17, 1000, 1023, 1024]
MB_PAD = 0xC3


def edge_counts(n_rec):
    """Block counts of n_rec records: COUNTS mixed inside every group; with a full first group, that
    group is all 0 except its last slot."""
    c = [COUNTS[(3 * i + n_rec) % len(COUNTS)] for i in range(n_rec)]
    if n_rec >= SLOTS:
        c[:SLOTS] = [0] * (SLOTS - 1) + [65]
    return np.array(c, np.uint32)


def layout(counts, seed, shuffle=False):
    """Word offsets of the records in one buffer: a guard word before, between and after the records,
    starts alternating between even and odd word offsets (16-byte aligned and 8 mod 16) in placement
    order; shuffle places the records out of memory order.  Returns (word_offsets, total_words)."""
    n = len(counts)
    order = np.random.default_rng(seed).permutation(n) if shuffle else np.arange(n)
    woff = np.zeros(n, np.uint64)
    pos = 1
    for r, i in enumerate(order):
        if pos % 2 != r % 2:
            pos += 1
        woff[i] = pos
        pos += 2 * int(counts[i]) + 1
    return woff, pos + 2


def reuse_shape(stride):
    """The slot-reuse case for a persistent grid of `stride` workgroups: 4 * stride groups, so workgroup
    w runs groups w, w + stride, w + 2 stride, w + 3 stride, and its slot k sees contexts A_k, A_k, B_k,
    A_k (A_k = k, B_k = 16 + k): no reload, a reload, a reload back -- a stale table decrypts rounds 2
    or 3 with the wrong key.  Slot 3 has no blocks in round 1 (A, none, B, A) and slot 5 none in round 2
    (A, A, none, A: never reloaded).  Returns (ctx_index, block_counts)."""
    n = 4 * stride * SLOTS
    rec = np.arange(n)
    k, rnd = rec % SLOTS, (rec // SLOTS) // stride
    idx = np.where(rnd == 2, SLOTS + k, k).astype(np.uint32)
    cnt = (1 + (rec % 3 == 0)).astype(np.uint32)
    cnt[(rnd == 1) & (k == 3)] = 0
    cnt[(rnd == 2) & (k == 5)] = 0
    return idx, cnt


def membuf_cases(offsets):
    """(size, offset) of the MemBuffer batch: every size with every offset."""
    return [(s, o) for o in offsets for s in MB_SIZES]


def membuf_span(data_size):
    return ((data_size // 8 + 3) // 2) * 16


def mb_room(size, off):
    """Bytes of a buffer that the caller grows and zero-fills: encrypt's span, and the pair after it,
    which decrypting the encrypted size reads (and stops at)."""
    return off + membuf_span(size + off) + 16


# ---- fixtures --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_dev(brb):
    import torch
    assert torch.cuda.is_available(), "no HIP device visible to torch"
    assert brb.gpu_available(), brb.lib().BRB_CryptoGPU_LastError()
    return torch


@pytest.fixture(scope="module")
def keyset(brb, orc):
    """N_KEYS keys of mixed lengths: the oracle's contexts and the host library's (BRB_Blowfish_Init),
    computed once."""
    rng = np.random.default_rng(2024)
    keys = [rng.integers(0, 256, 4 + (5 * i) % 53, dtype=np.uint8).tobytes() for i in range(N_KEYS)]
    octx = [orc.bf_init(k) for k in keys]
    host = brb.blowfish_contexts([brb.blowfish_init(k) for k in keys])
    assert [host[i].tobytes() for i in range(N_KEYS)] == [orc.bf_ctx_bytes(c) for c in octx]
    return keys, octx, host


def _words(total, woff, cnt, seed):
    """A buffer of guard words with random words (nonzero high halves) in the records."""
    rng = np.random.default_rng(seed)
    buf = np.full(total, GUARD, np.uint64)
    for o, c in zip(woff, cnt):
        w = rng.integers(0, 1 << 63, 2 * int(c), dtype=np.uint64) | np.uint64(1 << 47)
        buf[int(o): int(o) + 2 * int(c)] = w
    return buf


def _want(orc, octx, buf, woff, cnt, idx, decrypt):
    """The oracle's result: one orc.bf_ecb per context over the blocks of its records."""
    want = buf.copy()
    idx = np.arange(len(woff)) if idx is None else idx
    for c in np.unique(idx):
        pos = np.concatenate([np.arange(int(woff[i]), int(woff[i]) + 2 * int(cnt[i])) for i in np.nonzero(idx == c)[0]]
                             + [np.zeros(0, np.int64)]).astype(np.int64)
        if pos.size:
            seg = np.ascontiguousarray(want[pos])
            orc.bf_ecb(octx[int(c)], seg, decrypt)
            want[pos] = seg
    return want


def _run(brb, torch, fn, ctxs, buf, woff, cnt, idx, mode):
    """fn on a copy of buf; returns the resulting words.  mode: host / device / async / all3."""
    if mode in ("host", "all3"):
        out = buf.copy()
        if mode == "all3":
            with brb.TestOption("devices", 3):
                fn(ctxs, out, woff, cnt, idx, all_devices=True)
        else:
            fn(ctxs, out, woff, cnt, idx)
        return out
    d = torch.from_numpy(buf.view(np.int64).copy()).cuda()
    d_off = torch.from_numpy(woff.view(np.int64)).cuda()
    d_cnt = torch.from_numpy(cnt.view(np.int32)).cuda()
    d_idx = None if idx is None else torch.from_numpy(idx.view(np.int32)).cuda()
    d_ctx = ctxs if torch.is_tensor(ctxs) else torch.from_numpy(ctxs).cuda()
    if mode == "async":
        s = torch.cuda.Stream()
        torch.cuda.synchronize()              # the inputs were made on the default stream
        fn(d_ctx, d, d_off, d_cnt, d_idx, stream=s, async_=True)
        s.synchronize()
    else:
        fn(d_ctx, d, d_off, d_cnt, d_idx)
    return d.cpu().numpy().view(np.uint64)


def _three_way(brb, orc, torch, keyset, woff, total, cnt, idx, ctxs, mode, seed):
    """encrypt == oracle, decrypt == oracle, decrypt(encrypt) == the plaintext, in all 64 bits."""
    _, octx, _ = keyset
    plain = _words(total, woff, cnt, seed)
    assert ((plain >> np.uint64(32)) != 0).all()
    enc = _run(brb, torch, brb.blowfish_encrypt_batch_keyed, ctxs, plain, woff, cnt, idx, mode)
    assert np.array_equal(enc, _want(orc, octx, plain, woff, cnt, idx, False)), "encrypt differs from the oracle"
    dec = _run(brb, torch, brb.blowfish_decrypt_batch_keyed, ctxs, plain, woff, cnt, idx, mode)
    assert np.array_equal(dec, _want(orc, octx, plain, woff, cnt, idx, True)), "decrypt differs from the oracle"
    back = _run(brb, torch, brb.blowfish_decrypt_batch_keyed, ctxs, enc, woff, cnt, idx, mode)
    assert np.array_equal(back, plain), "decrypt(encrypt) is not the plaintext"
    if cnt.any():
        assert not np.array_equal(enc, plain)


# ---- group and lane edges ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["device", "host"])
@pytest.mark.parametrize("n_rec", N_RECS)
def test_group_and_lane_edges(brb, orc, torch_dev, keyset, n_rec, mode):
    """Identity context selection (ctx_index NULL, n_ctx == n_rec) with contexts from host
    BRB_Blowfish_Init; host mode runs on pageable numpy arrays."""
    cnt = edge_counts(n_rec)
    woff, total = layout(cnt, n_rec)
    _three_way(brb, orc, torch_dev, keyset, woff, total, cnt, None, keyset[2][:n_rec], mode, 100 + n_rec)


@pytest.mark.gpu
@pytest.mark.parametrize("bf_keyed", [1, 2])
@pytest.mark.parametrize("n_rec", N_RECS)
def test_group_and_lane_edges_kernel_variants(brb, orc, torch_dev, keyset, n_rec, bf_keyed):
    """The same shapes on the other two forms of the keyed kernel (test option bf_keyed: 1 the plain
    image fill, 2 one block per lane; 0, the default, runs above), device mode, encrypt and decrypt."""
    cnt = edge_counts(n_rec)
    woff, total = layout(cnt, n_rec)
    with brb.TestOption("bf_keyed", bf_keyed):
        _three_way(brb, orc, torch_dev, keyset, woff, total, cnt, None, keyset[2][:n_rec], "device", 100 + n_rec)


# ---- placement ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["device", "host"])
def test_placement_out_of_order_both_parities(brb, orc, torch_dev, keyset, mode):
    cnt = edge_counts(33)[SLOTS:]              # 17 records, every count
    woff, total = layout(cnt, 5, shuffle=True)
    assert {int(o) & 1 for o, c in zip(woff, cnt) if c} == {0, 1}
    assert (np.diff(woff.astype(np.int64)) < 0).any()
    _three_way(brb, orc, torch_dev, keyset, woff, total, cnt, None, keyset[2][:len(cnt)], mode, 7)


# ---- context selection ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["all_equal", "permuted"])
def test_context_index(brb, orc, torch_dev, keyset, kind):
    n = 33
    cnt = edge_counts(n)
    woff, total = layout(cnt, 11)
    idx = (np.full(n, 9, np.uint32) if kind == "all_equal"
           else np.random.default_rng(3).permutation(N_KEYS)[:n].astype(np.uint32))
    _three_way(brb, orc, torch_dev, keyset, woff, total, cnt, idx, keyset[2], "device", 13)


@pytest.mark.gpu
def test_slot_reuse_across_groups(brb, orc, torch_dev, keyset):
    """A workgroup's slot keeps its table while its records name the same context and reloads it when
    they do not: A, A, B, A in four consecutive groups of one workgroup (reuse_shape)."""
    stride = torch_dev.cuda.get_device_properties(0).multi_processor_count   # the persistent grid
    idx, cnt = reuse_shape(stride)
    woff = np.zeros(len(cnt), np.uint64)
    woff[1:] = np.cumsum(2 * cnt[:-1].astype(np.uint64))
    total = int(woff[-1]) + 2 * int(cnt[-1]) + 1
    plain = _words(total, woff, cnt, 17)
    enc = _run(brb, torch_dev, brb.blowfish_encrypt_batch_keyed, keyset[2], plain, woff, cnt, idx, "device")
    assert np.array_equal(enc, _want(orc, keyset[1], plain, woff, cnt, idx, False))
    dec = _run(brb, torch_dev, brb.blowfish_decrypt_batch_keyed, keyset[2], enc, woff, cnt, idx, "device")
    assert np.array_equal(dec, plain)


@pytest.mark.gpu
def test_contexts_made_on_the_device(brb, orc, torch_dev, keyset):
    """BRB_Blowfish_InitBatch -> BRB_Blowfish_EncryptBatchKeyed, device mode end to end: the contexts
    never leave HBM."""
    keys, octx, _ = keyset
    blob, koff, klen = brb.pack_keys(keys)
    d_ctx = brb.blowfish_init_batch(torch_dev.from_numpy(blob).cuda(), torch_dev.from_numpy(koff.view(np.int64)).cuda(),
                                    torch_dev.from_numpy(klen.view(np.int32)).cuda())
    n = 33
    cnt = edge_counts(n)
    woff, total = layout(cnt, 19)
    idx = ((np.arange(n) * 7 + 1) % N_KEYS).astype(np.uint32)
    plain = _words(total, woff, cnt, 23)
    enc = _run(brb, torch_dev, brb.blowfish_encrypt_batch_keyed, d_ctx, plain, woff, cnt, idx, "device")
    assert np.array_equal(enc, _want(orc, octx, plain, woff, cnt, idx, False))


# ---- modes ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_async_on_a_side_stream(brb, orc, torch_dev, keyset):
    cnt = edge_counts(17)
    woff, total = layout(cnt, 29)
    _three_way(brb, orc, torch_dev, keyset, woff, total, cnt, None, keyset[2][:17], "async", 31)


@pytest.mark.gpu
@pytest.mark.parametrize("shuffle", [False, True], ids=["disjoint", "interleaved"])
@pytest.mark.parametrize("indexed", [False, True], ids=["identity", "ctx_index"])
def test_all_devices_three_parts(brb, orc, torch_dev, keyset, shuffle, indexed):
    """BRB_BATCH_ALL_DEVICES forced into 3 parts on one GPU: records in memory order split (each part
    stages its own span and uploads its own contexts); interleaved spans do not split and are still right."""
    n = 33
    cnt = edge_counts(n)
    woff, total = layout(cnt, 37, shuffle=shuffle)
    idx = ((np.arange(n) * 11 + 2) % N_KEYS).astype(np.uint32) if indexed else None
    ctxs = keyset[2] if indexed else keyset[2][:n]
    _three_way(brb, orc, torch_dev, keyset, woff, total, cnt, idx, ctxs, "all3", 41)


# ---- MemBuffer batch -----------------------------------------------------------------------------------
def _mb_layout(cases, skew):
    """Buffers back to back: buffer i holds size bytes of data and zeros up to mb_room (what encrypt touches,
    offset + BRB_MEMBUF_SPAN(size + offset), and the one pair more that decrypting the result reads), then
    16 guard bytes; skew = True puts the buffers at every byte alignment (host mode)."""
    offs, pos = [], 16
    for i, (size, off) in enumerate(cases):
        pos = (pos + 15) // 16 * 16 + (i % 16 if skew else 0)
        offs.append(pos)
        pos += mb_room(size, off) + 16
    return np.array(offs, np.uint64), pos + 16


def _mb_fill(cases, offs, total, seed):
    rng = np.random.default_rng(seed)
    data = np.full(total, MB_PAD, np.uint8)
    for (size, off), o in zip(cases, offs):
        o = int(o)
        data[o: o + mb_room(size, off)] = 0
        data[o: o + size] = rng.integers(1, 256, size, dtype=np.uint8)
    return data


def _mb_oracle(orc_fn, data, offs, sizes, offsets, seeds, lens):
    """orc_fn per buffer on its own bytes; returns (whole data expected, new sizes)."""
    want, new = data.copy(), []
    for o, size, off, seed, ln in zip(offs, sizes, offsets, seeds, lens):
        o = int(o)
        b = bytearray(want[o: o + ln].tobytes())
        new.append(orc_fn(b, int(size), int(seed), int(off)))
        want[o: o + ln] = np.frombuffer(bytes(b), np.uint8)
    return want, np.array(new, np.uint64)


def _mb_call(brb, torch, fn, data, offs, sizes, offsets, seeds, seed_index, device):
    if not device:
        out = data.copy()
        new = fn(out, offs, sizes, seeds, offsets, seed_index)
        return out, new
    d = torch.from_numpy(data.copy()).cuda()
    t64 = lambda a: torch.from_numpy(a.view(np.int64)).cuda()
    new = fn(d, t64(offs), t64(sizes), seeds, t64(offsets),
             None if seed_index is None else torch.from_numpy(seed_index.view(np.int32)).cuda())
    return d.cpu().numpy(), new.cpu().numpy().view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("seed_kind", ["kv_seed", "distinct", "alternating"])
@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_membuf_batch_vs_oracle(brb, orc, torch_dev, device, seed_kind):
    cases = membuf_cases([0, 8] if device else [0, 8, 3])
    n = len(cases)
    offs, total = _mb_layout(cases, skew=not device)
    data = _mb_fill(cases, offs, total, 43)
    sizes = np.array([c[0] for c in cases], np.uint64)
    offsets = np.array([c[1] for c in cases], np.uint64)
    lens = [mb_room(size, off) + 16 for size, off in cases]
    if seed_kind == "kv_seed":
        seeds, seed_index, per_buf = [0x4FD9], None, [0x4FD9] * n
    elif seed_kind == "distinct":
        seeds, seed_index = [1000 + 77 * i for i in range(n)], None
        per_buf = seeds
    else:
        seeds, seed_index = [7, 0xFFFFFFF1], (np.arange(n) % 2).astype(np.uint32)
        per_buf = [seeds[i % 2] for i in range(n)]
    want, new_want = _mb_oracle(orc.membuf_encrypt, data, offs, sizes, offsets, per_buf, lens)
    got, new = _mb_call(brb, torch_dev, brb.membuf_encrypt_batch, data, offs, sizes, offsets, seeds, seed_index, device)
    assert np.array_equal(new, new_want)
    assert np.array_equal(got, want), "encrypted buffers (guard bytes included) differ from the oracle"
    # decrypt of the ciphertext (the reference's keyLen-64 quirk: not the plaintext); the data must still fit
    # its buffer: the decrypt span of the encrypted size is one pair more than the encrypt span
    assert all(off + membuf_span(int(ns) - off) == mb_room(size, off) for (size, off), ns in zip(cases, new_want))
    dwant, dnew_want = _mb_oracle(orc.membuf_decrypt, want, offs, new_want, offsets, per_buf, lens)
    dgot, dnew = _mb_call(brb, torch_dev, brb.membuf_decrypt_batch, want, offs, new_want, offsets, seeds, seed_index,
                          device)
    assert np.array_equal(dnew, dnew_want)
    assert np.array_equal(dgot, dwant), "decrypted buffers differ from the oracle"


@pytest.mark.gpu
@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_membuf_decrypt_batch_stops(brb, orc, torch_dev, device):
    """A zero word in pair 0, in a middle pair, in the last pair and in none: new_sizes equal the oracle's
    and the bytes from the stop onward are unchanged."""
    size, pairs = 1024, 65                              # (1024 / 8 + 2 + 1) / 2
    zero_pair = [0, 31, pairs - 1, None, 1, 64, 63, None] * 2 + [17]    # 17 buffers: two groups
    n = len(zero_pair)
    room = 16 * pairs + 16
    offs = (np.arange(n, dtype=np.uint64) * np.uint64(room)) + np.uint64(16)
    data = np.full(int(offs[-1]) + room + 16, MB_PAD, np.uint8)
    rng = np.random.default_rng(47)
    for i, zp in enumerate(zero_pair):
        w = rng.integers(1, 1 << 63, 2 * pairs, dtype=np.uint64)
        if zp is not None:
            w[2 * zp + (i & 1)] = 0                   # a zero xl or xr
        data[int(offs[i]): int(offs[i]) + 16 * pairs] = w.view(np.uint8)
    sizes, offsets = np.full(n, size, np.uint64), np.zeros(n, np.uint64)
    want, new_want = _mb_oracle(orc.membuf_decrypt, data, offs, sizes, offsets, [0x4FD9] * n, [room] * n)
    assert [int(x) for x in new_want] == [16 * (pairs if zp is None else zp) for zp in zero_pair]
    got, new = _mb_call(brb, torch_dev, brb.membuf_decrypt_batch, data, offs, sizes, offsets, [0x4FD9], None, device)
    assert np.array_equal(new, new_want)
    assert np.array_equal(got, want)
    for i in range(n):
        a = int(offs[i]) + int(new_want[i])
        assert np.array_equal(got[a: int(offs[i]) + room], data[a: int(offs[i]) + room])


@pytest.mark.gpu
def test_golden_membuffer_cases_as_one_batch(brb, golden):
    cases = golden["quirks"]["membuffer"]
    n = len(cases)
    room = max(len(c["plain"]) // 2 for c in cases) + 64
    data = np.zeros(n * room, np.uint8)
    offs = np.arange(n, dtype=np.uint64) * np.uint64(room)
    for c, o in zip(cases, offs):
        p = np.frombuffer(bytes.fromhex(c["plain"]), np.uint8)
        data[int(o): int(o) + p.size] = p
    sizes = np.array([c["size"] for c in cases], np.uint64)
    offsets = np.array([c["offset"] for c in cases], np.uint64)
    seeds = [c["seed"] for c in cases]
    new = brb.membuf_encrypt_batch(data, offs, sizes, seeds, offsets)
    assert [int(x) for x in new] == [c["enc_size"] for c in cases]
    for c, o in zip(cases, offs):
        assert data[int(o): int(o) + len(c["enc"]) // 2].tobytes().hex() == c["enc"]
    dnew = brb.membuf_decrypt_batch(data, offs, new, seeds, offsets)
    assert [int(x) for x in dnew] == [c["dec_size"] for c in cases]
    for c, o in zip(cases, offs):
        assert data[int(o): int(o) + len(c["dec"]) // 2].tobytes().hex() == c["dec"]


@pytest.mark.gpu
def test_kv_batch_equals_per_file(brb, torch_dev):
    from brb_framework_amd import kv
    texts = [kv.kv_assemble([(f"k{i}", "v" * (i * 37 % 91)) for i in range(m)]) for m in (0, 1, 3, 20, 77)]
    assert len({len(t) for t in texts}) == 5
    enc = kv.encrypt_texts(texts)
    assert enc == [kv.kv_encrypt(t) for t in texts]
    assert kv.decrypt_files(enc) == [kv.kv_decrypt(e) for e in enc]
    assert kv.encrypt_texts([]) == []


# ---- refusals ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_write_nothing(brb, torch_dev, keyset):
    L = brb.lib()
    n = 17
    cnt = edge_counts(n)
    woff, total = layout(cnt, 53)
    buf = _words(total, woff, cnt, 59)
    ctxs = keyset[2]
    # host mode: a context index out of range
    idx = np.arange(n, dtype=np.uint32)
    idx[11] = N_KEYS
    h = buf.copy()
    for fn in (L.BRB_Blowfish_EncryptBatchKeyed, L.BRB_Blowfish_DecryptBatchKeyed):
        assert fn(ctxs.ctypes.data, N_KEYS, idx.ctypes.data, h.ctypes.data, woff.ctypes.data, cnt.ctypes.data, n,
                  brb.BATCH_HOST, None) == -1
        assert b"out of range" in L.BRB_CryptoGPU_LastError()
    assert np.array_equal(h, buf)
    # device mode: words not 8-byte aligned
    d = torch_dev.from_numpy(buf.view(np.int64).copy()).cuda()
    d_ctx = torch_dev.from_numpy(ctxs).cuda()
    d_off = torch_dev.from_numpy(woff.view(np.int64)).cuda()
    d_cnt = torch_dev.from_numpy(cnt.view(np.int32)).cuda()
    for fn in (L.BRB_Blowfish_EncryptBatchKeyed, L.BRB_Blowfish_DecryptBatchKeyed):
        assert fn(d_ctx.data_ptr(), N_KEYS, None, d.data_ptr() + 4, d_off.data_ptr(), d_cnt.data_ptr(), n,
                  brb.BATCH_DEVICE, None) == -1
        assert b"aligned" in L.BRB_CryptoGPU_LastError()
    torch_dev.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().view(np.uint64), buf)
    # MemBuffer batch: device data not 8-byte aligned; a host-mode decrypt sizes[i] < offsets[i]
    data = np.full(512, 0x5A, np.uint8)
    offs, sizes = np.array([0, 128, 256], np.uint64), np.array([40, 4, 40], np.uint64)
    offsets = np.array([0, 8, 0], np.uint64)
    new = np.full(3, 99, np.uint64)
    seeds = np.array([0x4FD9], np.uint32)
    dd = torch_dev.from_numpy(data.copy()).cuda()
    t64 = lambda a: torch_dev.from_numpy(a.view(np.int64)).cuda()
    d_offs, d_sizes, d_offsets, d_new = t64(offs), t64(sizes), t64(offsets), t64(new)
    for fn in (L.BRB_MemBufferEncryptBatch, L.BRB_MemBufferDecryptBatch):
        assert fn(dd.data_ptr() + 4, d_offs.data_ptr(), d_sizes.data_ptr(), d_offsets.data_ptr(), seeds.ctypes.data, 1,
                  None, 3, d_new.data_ptr(), brb.BATCH_DEVICE, None) == -1
        assert b"aligned" in L.BRB_CryptoGPU_LastError()
    h = data.copy()
    assert L.BRB_MemBufferDecryptBatch(h.ctypes.data, offs.ctypes.data, sizes.ctypes.data, offsets.ctypes.data,
                                       seeds.ctypes.data, 1, None, 3, new.ctypes.data, brb.BATCH_HOST, None) == -1
    assert b"< offset" in L.BRB_CryptoGPU_LastError()
    assert np.array_equal(h, data) and (new == 99).all()
    torch_dev.cuda.synchronize()
    assert np.array_equal(dd.cpu().numpy(), data) and (d_new.cpu().numpy() == 99).all()
