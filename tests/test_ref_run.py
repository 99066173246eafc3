"""Every batch entry point against bytes that the reference's own code produced.

tests/golden/ref_run/*.json was recorded from a build of the reference's units (tests/golden/make_ref_run.py,
oracle/ref_build/).  Here the GPU calls get the same inputs (tests/ref_run_cases.py regenerates them from
their seeds) and their outputs are compared with those files directly, not through the oracle.  Nothing
here reads the reference or oracle/_ref.  Shapes are the smallest that still take the real kernels: the
2 050- and 257-block Blowfish vectors, digest batches of 65 records or a few more, 256 RC4 states.

Where a file holds a hash instead of the bytes (bulk outputs), the output is hashed the same way and its
first and last rows are compared in full; a per-row CRC-32 names the row that differs.

PINNED names, for every *Batch* export of include/brb_crypto.h, the tests below that compare it with these
vectors; EXCLUDED gives the patterns of the exports that are not compared and why.  tests/test_ref_run_cpu.py checks both
against the header.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rc4_model  # noqa: E402
import ref_run_cases as rr  # noqa: E402
import verdict_cases  # noqa: E402

PINNED = {
    "BRB_Blowfish_EncryptBatch": ["test_blowfish_ecb_batch"],
    "BRB_Blowfish_DecryptBatch": ["test_blowfish_ecb_batch"],
    "BRB_Blowfish_EncryptBatchKeyed": ["test_blowfish_keyed_batch"],
    "BRB_Blowfish_DecryptBatchKeyed": ["test_blowfish_keyed_batch"],
    "BRB_Blowfish_InitBatch": ["test_blowfish_init_batch"],
    "BRB_MD5BatchFixed": ["test_fixed_digests_by_route"],
    "BrbSha1_BatchFixed": ["test_fixed_digests_by_route"],
    "BRB_MD5Batch": ["test_var_digests"],
    "BrbSha1_Batch": ["test_var_digests", "test_batch_calls_leave_the_data_alone"],
    "BRB_MD5BatchSegments": ["test_md5_batch_segments"],
    "BRB_MD5InitBatch": ["test_md5_stream_batches"],
    "BRB_MD5UpdateBatch": ["test_md5_stream_batches"],
    "BRB_MD5FinalBatch": ["test_md5_stream_batches"],
    "BrbSha1_InitBatch": ["test_sha1_stream_batches"],
    "BrbSha1_UpdateBatch": ["test_sha1_stream_batches", "test_batch_calls_leave_the_data_alone"],
    "BrbSha1_FinalBatch": ["test_sha1_stream_batches"],
    "BRB_MD5UpdateSegmentsBatch": ["test_update_segments_batches"],
    "BrbSha1_UpdateSegmentsBatch": ["test_update_segments_batches"],
    "BRB_MD5LowerTextBatch": ["test_md5_lower_text_batches"],
    "BRB_MD5UpdateSegmentsLowerBatch": ["test_md5_lower_text_batches"],
    "BRB_RC4_InitBatch": ["test_rc4_init_batch"],
    "BRB_RC4_CryptBatch": ["test_rc4_crypt_batch_on_non_permutations"],
    "BRB_Base64EncodeBatch": ["test_base64_batches"],
    "BRB_Base64DecodeBatch": ["test_base64_batches"],
    "BRB_MemBufferEncryptBatch": ["test_membuffer_batches"],
    "BRB_MemBufferDecryptBatch": ["test_membuffer_batches", "test_membuffer_zero_pair_stops"],
    "BRB_MetaDataPackBatch": ["test_metadata_pack_batch"],
    "BRB_MetaDataUnpackBatch": ["test_metadata_unpack_batches"],
    "BRB_MetaDataUnpackItemsBatch": ["test_metadata_unpack_batches"],
}
_EVENT_LAYER = ("the RC4+MD5 frame is the event layer's (ev_kq_aio_transform.c), outside the units the reference build "
                "holds: a cited restatement whose parts (RC4, MD5, the layout) are pinned one by one")
_LIST = "a buffer list per connection over BRB_RC4_CryptBatch's per-buffer body (rc4_block.h); tests/test_rc4_lists.py ties it to that call"
_BATCHER = "the transform batcher is this project's receive-loop plumbing over the calls above; the reference has no counterpart to record"
EXCLUDED = {                            # a pattern that matches whole export names: the reason
    r"BRB_RC4MD5_(Frame|Open)(List)?Batch": _EVENT_LAYER,
    r"BRB_RC4_(Crypt|Mixed)ListBatch": _LIST,
    r"BRB_TransformBatcher\w+": _BATCHER,
}


@pytest.fixture(scope="module")
def gpu(brb):
    import torch
    assert torch.cuda.is_available(), "no HIP device visible to torch"
    assert brb.gpu_available(), brb.lib().BRB_CryptoGPU_LastError()
    return brb


@pytest.fixture(scope="module")
def vec():
    return {f: rr.load(f) for f in rr.FAMILIES}


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def host(t):
    return t.cpu().numpy()


def same(got, want, what):
    bad = rr.differences(got, want)
    assert not bad, f"{what}:\n" + "\n".join(bad)


# ---- Blowfish ---------------------------------------------------------------------------------------------
def pinned_ctx(brb, vec, n):
    """BRB_Blowfish_Init of the recorded key of n bytes (host compat code), checked against the recorded image."""
    ctx = brb.blowfish_init(rr.bf_key(n), n)
    assert rr.sha(brb.blowfish_ctx_bytes(ctx)) == vec["blowfish"]["contexts"][f"len{n}"]["sha256"]
    return ctx


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["host", "device"])
def test_blowfish_ecb_batch(gpu, vec, mode):
    for n, blocks in rr.BF_ECB:
        ctx = pinned_ctx(gpu, vec, n)
        for cls in rr.BF_CLASSES:
            want = vec["blowfish"]["ecb"][f"len{n}_{blocks}_{cls}"]
            for name, fn in (("encrypt", gpu.blowfish_encrypt_batch), ("decrypt", gpu.blowfish_decrypt_batch)):
                w = rr.bf_words(n, blocks, cls)
                if mode == "device":
                    w = host(fn(ctx, dev(w))).view(np.uint64)
                else:
                    fn(ctx, w)
                same(rr.bulk_words(w), want[name], f"{name} {mode} key {n} {blocks} blocks {cls}")


@pytest.mark.gpu
@pytest.mark.parametrize("bf_keyed", [0, 1, 2])
def test_blowfish_keyed_batch(gpu, vec, bf_keyed):
    """The nine recorded vectors as nine records of one call, three contexts, a record starting at 8 mod 16."""
    ctxs = [pinned_ctx(gpu, vec, n) for n, _ in rr.BF_ECB]
    recs = [(k, n, blocks, cls) for k, (n, blocks) in enumerate(rr.BF_ECB) for cls in rr.BF_CLASSES]
    parts, offs, pos = [], [], 0
    for j, (_, n, blocks, cls) in enumerate(recs):
        gap = j % 2 + 1                                   # 1 or 2 guard words before each record
        parts += [np.full(gap, 0xEEEEEEEEEEEEEEEE, np.uint64), rr.bf_words(n, blocks, cls)]
        offs.append(pos + gap)
        pos += gap + 2 * blocks
    words0 = np.concatenate(parts + [np.full(3, 0xEEEEEEEEEEEEEEEE, np.uint64)])
    offs = np.array(offs, np.uint64)
    counts = np.array([b for _, _, b, _ in recs], np.uint32)
    index = np.array([k for k, _, _, _ in recs], np.uint32)
    assert {int(o) % 2 for o in offs} == {0, 1}
    inside = np.zeros(words0.size, bool)
    for o, b in zip(offs.tolist(), counts.tolist()):
        inside[o:o + 2 * b] = True
    with gpu.TestOption("bf_keyed", bf_keyed):
        for name, fn in (("encrypt", gpu.blowfish_encrypt_batch_keyed), ("decrypt", gpu.blowfish_decrypt_batch_keyed)):
            for mode in ("host", "device"):
                w = words0.copy()
                if mode == "device":
                    w = host(fn(ctxs, dev(w), dev(offs), dev(counts), dev(index))).view(np.uint64)
                else:
                    fn(ctxs, w, offs, counts, index)
                assert np.array_equal(w[~inside], words0[~inside]), "words between the records changed"
                for (_, n, blocks, cls), o in zip(recs, offs.tolist()):
                    same(rr.bulk_words(w[o:o + 2 * blocks]), vec["blowfish"]["ecb"][f"len{n}_{blocks}_{cls}"][name],
                         f"{name} {mode} bf_keyed {bf_keyed} key {n} {cls}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["host", "device"])
def test_blowfish_init_batch(gpu, vec, mode):
    keys = rr.bf_keys()
    blob, offs, lens = gpu.pack_keys([k[:n] for _, k, n in keys])
    rows = gpu.blowfish_init_batch(blob, offs, lens) if mode == "host" else host(gpu.blowfish_init_batch(dev(blob), dev(offs), dev(lens)))
    for (name, _, _), row in zip(keys, rows):
        want = vec["blowfish"]["contexts"][name]
        same(rr.bf_image(row.tobytes()), {k: want[k] for k in ("P", "S_sha256", "sha256", "widest_bits")}, f"{name} {mode}")


# ---- digests ----------------------------------------------------------------------------------------------
def md5_digest(vec, n):
    return rr.unimg(vec["md5"]["cases"][str(n)]["final"])[88:104]


def sha1_digest(vec, n):
    return bytes.fromhex(vec["sha1"]["cases"][str(n)]["digest"])


N_FIXED = 65
FIXED_ROUTES = ((20, 8, ()), (64, 5, ()), (77, 3, ()), (1500, 2, ()), (1501, 3, ()), (129, 4, (("fixed_var_line", 0),)))


@pytest.mark.gpu
@pytest.mark.parametrize("rec_len,route,opts", FIXED_ROUTES, ids=[f"{c[0]}" for c in FIXED_ROUTES])
def test_fixed_digests_by_route(gpu, vec, rec_len, route, opts):
    """A recorded message 65 times back to back (so the rows meet every alignment): DMA_SHORT, B64R_8, VAR_LINE,
    LINE, VAR_LINE and, without the var-line kernel, DMA_TICKET."""
    import contextlib
    d = dev(np.frombuffer(rr.message(rec_len) * N_FIXED, np.uint8))
    with contextlib.ExitStack() as st:
        for name, value in opts:
            st.enter_context(gpu.TestOption(name, value))
        assert gpu.fixed_route(d.data_ptr(), rec_len) == route
        md5 = host(gpu.md5_batch_fixed(d, rec_len, N_FIXED))
        sha1 = host(gpu.sha1_batch_fixed(d, rec_len, N_FIXED))
    assert md5.shape == (N_FIXED, 16) and [r.tobytes().hex() for r in md5] == [md5_digest(vec, rec_len).hex()] * N_FIXED
    assert sha1.shape == (N_FIXED, 20) and [r.tobytes().hex() for r in sha1] == [sha1_digest(vec, rec_len).hex()] * N_FIXED


ALL_LENS = rr.DIGEST_LENS + rr.ROUTE_LENS


def ragged_messages(repeat):
    """Every recorded message `repeat` times, in one buffer with gaps of 0..3 bytes -> (lens list, data, offs, lens)."""
    ns = [n for _ in range(repeat) for n in ALL_LENS]
    offs, lens, total = rc4_model.layout(ns, rr.SEED)
    data = np.full(total, 0xEE, np.uint8)
    for o, n in zip(offs.tolist(), ns):
        data[o:o + n] = np.frombuffer(rr.message(n), np.uint8)
    return ns, data, offs, lens


@pytest.mark.gpu
@pytest.mark.parametrize("var_line", [1, 0])
def test_var_digests(gpu, vec, var_line):
    ns, data, offs, lens = ragged_messages(4)                    # 68 records
    with gpu.TestOption("var_line", var_line):
        for mode in ("host", "device"):
            a = (data, offs, lens) if mode == "host" else (dev(data), dev(offs), dev(lens))
            md5, sha1 = gpu.md5_batch(*a), gpu.sha1_batch(*a)
            if mode == "device":
                md5, sha1 = host(md5), host(sha1)
            assert [r.tobytes().hex() for r in md5] == [md5_digest(vec, n).hex() for n in ns], mode
            assert [r.tobytes().hex() for r in sha1] == [sha1_digest(vec, n).hex() for n in ns], mode


def segment_lists(cases, repeat=1):
    """The pieces of the cases as segments of one buffer (gaps of 0..3 bytes) -> (data, seg_offs, seg_lens, first)."""
    cases = [c for _ in range(repeat) for c in cases]
    pieces = [rr.pieces(n, s) for n, s in cases]
    flat = [p for ps in pieces for p in ps]
    offs, lens, total = rc4_model.layout([len(p) for p in flat], rr.SEED + 1)
    data = np.full(total, 0xEE, np.uint8)
    for o, p in zip(offs.tolist(), flat):
        data[o:o + len(p)] = np.frombuffer(p, np.uint8)
    first = np.concatenate([[0], np.cumsum([len(ps) for ps in pieces])]).astype(np.uint64)
    return cases, data, offs, lens, first


@pytest.mark.gpu
@pytest.mark.parametrize("seg_line", [2, 0])
def test_md5_batch_segments(gpu, vec, seg_line):
    """Every recorded message whole and cut at its recorded split point: 29 records three times over."""
    cases, data, offs, lens, first = segment_lists(rr.digest_cases(), 3)
    with gpu.TestOption("seg_line", seg_line):
        for mode in ("host", "device"):
            a = (data, offs, lens, first) if mode == "host" else tuple(dev(x) for x in (data, offs, lens, first))
            out = gpu.md5_batch_segments(*a)
            out = out if mode == "host" else host(out)
            assert [r.tobytes().hex() for r in out] == [md5_digest(vec, n).hex() for n, _ in cases], mode


# ---- streaming contexts -------------------------------------------------------------------------------------
def case_key(n, s):
    return f"{n}" if s is None else f"{n}@{s}"


def stream_plan():
    """The digest cases as rows of a context table, and the two Update calls: every row's first piece, then the
    second piece of the rows that are cut (named by ctx_index)."""
    cases = rr.digest_cases()
    first = [rr.pieces(n, s)[0] for n, s in cases]
    cut = np.array([k for k, (_, s) in enumerate(cases) if s is not None], np.uint32)
    second = [rr.pieces(*cases[k])[1] for k in cut]
    return cases, first, cut, second


def lay(pieces, seed):
    offs, lens, total = rc4_model.layout([len(p) for p in pieces], seed)
    data = np.full(total, 0xEE, np.uint8)
    for o, p in zip(offs.tolist(), pieces):
        data[o:o + len(p)] = np.frombuffer(p, np.uint8)
    return data, offs, lens


def run_stream(gpu, vec, fam, mode, width, head, init, update, final):
    """Init, Update (first pieces), Update (second pieces of the cut rows), Final over one table; after every step
    the part of every context that the reference's call defines equals the recorded image; after Final all of it."""
    want = vec[fam]
    cases, first, cut, second = stream_plan()
    keys = [case_key(n, s) for n, s in cases]
    up = lambda k, j: np.frombuffer(rr.unimg(want["cases"][k]["update"][j]), np.uint8)       # noqa: E731
    to = (lambda x: x) if mode == "host" else dev
    back = (lambda x: x) if mode == "host" else host
    table = to(np.full((len(cases), width), rr.FILL, np.uint8))
    init(table)
    t = back(table)
    assert (t[:, :head] == np.frombuffer(rr.unimg(want["init"]), np.uint8)[:head]).all(), "after Init"

    def check_defined(rows, taken, step):
        t = back(table)
        for r in rows:
            w = up(keys[r], step(r))
            fill = head + taken[r] % 64
            assert t[r, :fill].tobytes() == w[:fill].tobytes(), (fam, mode, keys[r], "after Update", step(r))

    data, offs, lens = lay(first, rr.SEED + 2)
    update(table, to(data), to(offs), to(lens), None)
    check_defined(range(len(cases)), [len(p) for p in first], lambda r: 0)
    data, offs, lens = lay(second, rr.SEED + 3)
    update(table, to(data), to(offs), to(lens), to(cut))
    check_defined(cut.tolist(), [n for n, _ in cases], lambda r: 1)
    dig = back(final(table))
    t = back(table)
    for r, k in enumerate(keys):
        assert t[r].tobytes() == rr.unimg(want["cases"][k]["final"]), (fam, mode, k, "the context after Final")
    return keys, dig


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["host", "device"])
def test_md5_stream_batches(gpu, vec, mode):
    keys, dig = run_stream(gpu, vec, "md5", mode, 168, 24, gpu.md5_init_batch,
                           lambda t, d, o, n, i: gpu.md5_update_batch(t, d, o, n, ctx_index=i), gpu.md5_final_batch)
    assert [r.tobytes().hex() for r in dig] == [md5_digest(vec, k).hex() for k in keys]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["host", "device"])
def test_sha1_stream_batches(gpu, vec, mode):
    keys, dig = run_stream(gpu, vec, "sha1", mode, 92, 28, gpu.sha1_init_batch,
                           lambda t, d, o, n, i: gpu.sha1_update_batch(t, d, o, n, ctx_index=i), gpu.sha1_final_batch)
    assert [r.tobytes().hex() for r in dig] == [vec["sha1"]["cases"][k]["digest"] for k in keys]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["host", "device"])
def test_update_segments_batches(gpu, vec, mode):
    """A case's pieces as its segment list.  Even rows are finalised in the call (the whole context equals the
    recorded image after Final), odd rows are not (the defined part equals the image after the last Update)."""
    cases, data, offs, lens, first = segment_lists(rr.digest_cases())
    keys = [case_key(n, s) for n, s in cases]
    fin = (np.arange(len(cases)) % 2 == 0).astype(np.uint8)
    to = (lambda x: x) if mode == "host" else dev
    back = (lambda x: x) if mode == "host" else host
    for fam, width, head, dlen, init, call in (("md5", 168, 24, 16, gpu.md5_init_batch, gpu.md5_update_segments_batch),
                                               ("sha1", 92, 28, 20, gpu.sha1_init_batch, gpu.sha1_update_segments_batch)):
        want = vec[fam]["cases"]
        table = to(np.full((len(cases), width), rr.FILL, np.uint8))
        init(table)
        dig = back(call(table, to(data), to(offs), to(lens), to(first), final=to(fin)))
        t = back(table)
        for r, (k, (n, _)) in enumerate(zip(keys, cases)):
            if fin[r]:
                assert t[r].tobytes() == rr.unimg(want[k]["final"]), (fam, mode, k)
                d = md5_digest(vec, k).hex() if fam == "md5" else want[k]["digest"]
                assert dig[r, :dlen].tobytes().hex() == d, (fam, mode, k)
            else:
                w = rr.unimg(want[k]["update"][-1])
                assert t[r, :head + n % 64].tobytes() == w[:head + n % 64], (fam, mode, k)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["host", "device"])
def test_md5_lower_text_batches(gpu, vec, mode):
    """bytes(range(256)) and the bytes around 'A', 'Z' and their signed-char twins: the key call's digests and
    hex strings, and the segment call's contexts (the reference took all 256 bytes in two calls of 128)."""
    want = vec["md5"]["lower_text"]
    keys = [bytes(range(256)), bytes(rr.LOWER_SPECIAL)]
    finals = [rr.unimg(want[k]["final"]) for k in ("all_bytes", "special")]
    to = (lambda x: x) if mode == "host" else dev
    back = (lambda x: x) if mode == "host" else host
    data, offs, lens = lay(keys, rr.SEED + 4)
    dig, strs = gpu.md5_lower_text_batch(to(data), to(offs), to(lens), want_strings=True)
    assert [r.tobytes() for r in back(dig)] == [f[88:104] for f in finals]
    assert [r.tobytes() for r in back(strs)] == [f[104:137] for f in finals]
    segs = [keys[0][:128], keys[0][128:], keys[1]]
    data, offs, lens = lay(segs, rr.SEED + 5)
    first = np.array([0, 2, 3], np.uint64)
    table = to(np.full((2, 168), rr.FILL, np.uint8))
    gpu.md5_init_batch(table)
    gpu.md5_update_segments_lower_batch(table, to(data), to(offs), to(lens), to(first))             # no Final yet
    t = back(table)
    for r, name in enumerate(("all_bytes", "special")):
        w, n = rr.unimg(want[name]["update"]), len(keys[r])
        assert t[r, :24 + n % 64].tobytes() == w[:24 + n % 64], name
    dig = back(gpu.md5_final_batch(table))
    assert [r.tobytes() for r in back(table)] == finals
    assert [r.tobytes() for r in dig] == [f[88:104] for f in finals]


@pytest.mark.gpu
def test_batch_calls_leave_the_data_alone(gpu, vec):
    """The documented deviation: BrbSha1_Update rewrites the caller's blocks in place (the recorded buffer differs
    from the message); BrbSha1_Batch and BrbSha1_UpdateBatch digest the same bytes and write nothing into them."""
    n = 1500
    rec = vec["sha1"]["cases"][str(n)]
    msg = rr.message(n)
    assert rec["data_after"][0]["changed"] and rec["data_after"][0]["sha256"] != rr.sha(msg)
    d = dev(np.frombuffer(msg * 3, np.uint8))
    offs, lens = dev(np.array([0, n, 2 * n], np.uint64)), dev(np.array([n] * 3, np.uint32))
    out = host(gpu.sha1_batch(d, offs, lens))
    assert [r.tobytes().hex() for r in out] == [rec["digest"]] * 3
    table = dev(np.full((3, 92), rr.FILL, np.uint8))
    gpu.sha1_init_batch(table)
    gpu.sha1_update_batch(table, d, offs, lens)
    assert host(table)[0, :28 + n % 64].tobytes() == rr.unimg(rec["update"][0])[:28 + n % 64]
    assert host(d).tobytes() == msg * 3


# ---- RC4 ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["host", "device"])
def test_rc4_init_batch(gpu, vec, mode):
    keys = rr.rc4_keys()
    blob, offs, lens = gpu.pack_keys([k for _, k in keys])
    rows = gpu.rc4_init_batch(blob, offs, lens) if mode == "host" else host(gpu.rc4_init_batch(dev(blob), dev(offs), dev(lens)))
    same({name: rr.rc4_init_entry(name, key, r.tobytes()) for (name, key), r in zip(keys, rows)}, vec["rc4"]["init"], mode)


@pytest.mark.gpu
@pytest.mark.parametrize("rc4_pair", [1, 0])
@pytest.mark.parametrize("cls", ["b", "d"])
def test_rc4_crypt_batch_on_non_permutations(gpu, vec, cls, rc4_pair):
    """256 states that are no permutations (class B; class D with non-zero padding and flags), whose outputs the
    reference produced: keystream and all 264 state bytes per stream."""
    want = vec["rc4"]["classes"][cls]
    states0, lens, rows = rr.rc4_class_rows(cls)
    offs, lens32, total = rc4_model.layout(lens, rr.SEED + 6)
    data0 = np.full(total, 0xEE, np.uint8)
    for o, r in zip(offs.tolist(), rows):
        data0[o:o + len(r)] = np.frombuffer(r, np.uint8)
    with gpu.TestOption("rc4_pair", rc4_pair):
        for mode in ("host", "device"):
            st, data = states0.copy(), data0.copy()
            if mode == "host":
                gpu.rc4_crypt_batch(st, data, offs, lens32)
            else:
                ds, dd = dev(st), dev(data)
                gpu.rc4_crypt_batch(ds, dd, dev(offs), dev(lens32))
                st, data = host(ds), host(dd)
            got = [(st[k].tobytes(), data[o:o + n].tobytes()) for k, (o, n) in enumerate(zip(offs.tolist(), lens.tolist()))]
            same(rr.rc4_class_summary(got), want, f"{mode} rc4_pair {rc4_pair} (a group is {rr.RC4_GROUP} streams)")
            assert np.array_equal(data[~rc4_model.covered(offs, lens, total)], data0[~rc4_model.covered(offs, lens, total)])


# ---- base64 ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("group", [-1, 0])
def test_base64_batches(gpu, vec, group):
    want = vec["base64"]
    plain = [rr.rnd(0x600 + n, n) for n in range(50)] + list(rr.B64_RFC)
    text = [want["encode"][str(n)].encode("latin1") for n in range(50)] + [want["rfc4648"][d.decode()]["text"].encode() for d in rr.B64_RFC]
    odd = [bytes.fromhex(v["text"]) for v in want["odd"].values()]
    dec_in = text + odd
    dec_want = [bytes.fromhex(want["decode"][str(n)]) for n in range(50)] \
        + [bytes.fromhex(want["rfc4648"][d.decode()]["decoded"]) for d in rr.B64_RFC] + [bytes.fromhex(v["decoded"]) for v in want["odd"].values()]
    assert [w[:len(p)] for w, p in zip(dec_want, plain)] == plain          # '=' decodes as 0: up to two bytes more
    with gpu.TestOption("b64_group", group):
        for mode in ("host", "device"):
            to = (lambda x: x) if mode == "host" else dev
            back = (lambda x: x) if mode == "host" else host
            data, offs, lens = lay(plain, rr.SEED + 7)
            ooffs, _, ototal = rc4_model.layout([len(t) for t in text], rr.SEED + 8)
            out = back(gpu.base64_encode_batch(to(data), to(offs), to(lens), to(np.full(ototal, 0xEE, np.uint8)), to(ooffs)))
            assert [out[o:o + len(t)].tobytes() for o, t in zip(ooffs.tolist(), text)] == text, mode
            assert int((out != 0xEE).sum()) <= sum(len(t) for t in text)
            data, offs, lens = lay(dec_in, rr.SEED + 9)
            ooffs, _, ototal = rc4_model.layout([3 * (len(t) // 4) for t in dec_in], rr.SEED + 10)
            buf = to(np.full(ototal, 0xEE, np.uint8))
            n_out = back(gpu.base64_decode_batch(to(data), to(offs), to(lens), buf, to(ooffs)))
            out = back(buf)
            assert [int(x) for x in n_out] == [len(w) for w in dec_want], mode
            assert [out[o:o + len(w)].tobytes() for o, w in zip(ooffs.tolist(), dec_want)] == dec_want, mode


# ---- MemBuffer ------------------------------------------------------------------------------------------------
def img_same(got, rec, what):
    if "hex" in rec:
        assert got.tobytes().hex() == rec["hex"], what
    else:
        assert rr.crc(got.tobytes()) == rec["crc"], what


MB_CASES = [(size, off) for size in rr.MB_SIZES for off in rr.MB_OFFS]


@pytest.mark.gpu
def test_membuffer_single_calls(gpu, vec):
    """BRB_MemBufferEncrypt (keyLen 4) and BRB_MemBufferDecrypt (keyLen 64: not the inverse) on every recorded
    size x offset, host mode, and device mode where buf + offset is 8-byte aligned."""
    for size, off in MB_CASES:
        rec = vec["membuf"]["cases"][f"{size}+{off}"]
        img0 = np.frombuffer(rr.mb_image(size, off, rec["seed"]), np.uint8)
        for mode in ("host",) + (("device",) if off % 8 == 0 else ()):
            b = img0.copy() if mode == "host" else dev(img0)
            assert gpu.membuf_encrypt(b, size, rec["seed"], off) == rec["enc_size"], (size, off, mode)
            img_same(b if mode == "host" else host(b), rec["enc"], (size, off, mode, "encrypt"))
            assert gpu.membuf_decrypt(b, rec["enc_size"], rec["seed"], off) == rec["dec_size"], (size, off, mode)
            img_same(b if mode == "host" else host(b), rec["dec"], (size, off, mode, "decrypt"))


@pytest.mark.gpu
def test_membuffer_batches(gpu, vec):
    """All 72 recorded buffers in one encrypt call and one decrypt call, a seed per buffer, guard bytes between."""
    recs = [vec["membuf"]["cases"][f"{size}+{off}"] for size, off in MB_CASES]
    imgs = [np.frombuffer(rr.mb_image(size, off, r["seed"]), np.uint8) for (size, off), r in zip(MB_CASES, recs)]
    starts = (16 + np.cumsum([0] + [len(i) + 16 for i in imgs[:-1]])).astype(np.uint64)
    data = np.full(int(starts[-1]) + len(imgs[-1]) + 16, 0xEE, np.uint8)
    inside = np.zeros(data.size, bool)
    for s, i in zip(starts.tolist(), imgs):
        data[s:s + len(i)] = i
        inside[s:s + len(i)] = True
    sizes = np.array([s for s, _ in MB_CASES], np.uint64)
    offsets = np.array([o for _, o in MB_CASES], np.uint64)
    seeds = np.array([r["seed"] for r in recs], np.uint32)
    ns = gpu.membuf_encrypt_batch(data, starts, sizes, seeds, offsets=offsets)
    assert ns.tolist() == [r["enc_size"] for r in recs]
    for (c, r, s, i) in zip(MB_CASES, recs, starts.tolist(), imgs):
        img_same(data[s:s + len(i)], r["enc"], (c, "encrypt batch"))
    assert rr.sha(b"".join(data[s:s + len(i)].tobytes() for s, i in zip(starts.tolist(), imgs))) == vec["membuf"]["enc_sha256"]
    ds = gpu.membuf_decrypt_batch(data, starts, ns, seeds, offsets=offsets)
    assert ds.tolist() == [r["dec_size"] for r in recs]
    for (c, r, s, i) in zip(MB_CASES, recs, starts.tolist(), imgs):
        img_same(data[s:s + len(i)], r["dec"], (c, "decrypt batch"))
    assert rr.sha(b"".join(data[s:s + len(i)].tobytes() for s, i in zip(starts.tolist(), imgs))) == vec["membuf"]["dec_sha256"]
    assert (data[~inside] == 0xEE).all()


@pytest.mark.gpu
def test_membuffer_zero_pair_stops(gpu, vec):
    """The six recorded stops at a pair holding a zero word: the single call in both modes and the batch call."""
    want = vec["membuf"]["zero_pair"]
    imgs = []
    for z in rr.MB_ZERO_AT:
        img, size, seed = rr.mb_zero_image(z)
        img = np.frombuffer(img, np.uint8)
        imgs.append(img)
        assert want[str(z)]["dec_size"] == 16 * z
        for mode in ("host", "device"):
            b = img.copy() if mode == "host" else dev(img)
            assert gpu.membuf_decrypt(b, size, seed, 0) == 16 * z, (z, mode)
            assert rr.sha((b if mode == "host" else host(b)).tobytes()) == want[str(z)]["sha256"], (z, mode)
    data = np.concatenate(imgs)
    starts = (np.arange(len(imgs)) * len(imgs[0])).astype(np.uint64)
    ds = gpu.membuf_decrypt_batch(data, starts, np.full(len(imgs), size, np.uint64), [seed])
    assert ds.tolist() == [16 * z for z in rr.MB_ZERO_AT]
    for k, z in enumerate(rr.MB_ZERO_AT):
        assert rr.sha(data[k * len(imgs[0]):(k + 1) * len(imgs[0])].tobytes()) == want[str(z)]["sha256"], z


# ---- MetaData -------------------------------------------------------------------------------------------------
def recorded_packs(vec):
    """{name: (items, pack bytes)}: the packs by verdict_cases.md_pack (struct + hashlib), checked against what the
    reference's MetaDataPack wrote (size and CRC-32 of each, a hash over all, some in full)."""
    lists = rr.md_item_lists()
    packs = {name: verdict_cases.md_pack(items) for name, items in lists.items()}
    same(rr.pack_summary(packs), vec["metadata_pack"], "md_pack")
    return {name: (lists[name], packs[name]) for name in lists}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["host", "device"])
def test_metadata_pack_batch(gpu, vec, mode):
    from test_metadata_pack import build_call, check, run
    packs = recorded_packs(vec)
    c = build_call(np.random.default_rng(rr.SEED), [i for i, _ in packs.values()], [p for _, p in packs.values()], gaps=(0, 9))
    check(run(gpu, c, mode), c)


@pytest.fixture(scope="module")
def unpack_table():
    cases = rr.md_unpack_cases()
    buf, offs, lens = verdict_cases.md_layout([p for _, p in cases], 1, rr.SEED)
    for a in (buf, offs, lens):
        a.setflags(write=False)
    return [n for n, _ in cases], buf, offs, lens


@pytest.mark.gpu
@pytest.mark.parametrize("seg_line", [2, 0])
def test_metadata_unpack_batches(gpu, vec, unpack_table, seg_line):
    """Some 7 000 packs -- valid, cut, every bit flipped -- through both unpack calls: the verdict fields, the
    number of MetaDataItemAdd calls and the item table are the reference's."""
    names, buf, offs, lens = unpack_table
    slots = np.maximum((lens.astype(np.int64) - 64) // 25, 0) + 1
    first = np.concatenate([[0], np.cumsum(slots)]).astype(np.uint64)
    with gpu.TestOption("seg_line", seg_line):
        info = gpu.metadata_unpack_batch(buf, offs, lens)
        ioff, ilen, iid, isub = (np.full(int(first[-1]), 0xEEEEEEEE, t) for t in (np.uint64, np.uint32, np.uint64, np.uint64))
        info2, added = gpu.metadata_unpack_items_batch(buf, offs, lens, ioff, ilen, iid, isub, first)
    assert np.array_equal(info, info2)
    assert (added == info["item_count"] + (info["error_code"] == 3)).all() and (added <= slots).all()
    code = info["error_code"].astype(np.int64).view(np.uint64)
    rows = np.stack([code, code, info["cur_offset"], info["cur_remaining"], info["cur_needed"], added.astype(np.uint64)], axis=1)
    items = []
    for p in range(len(names)):
        s = slice(int(first[p]), int(first[p]) + int(added[p]))
        items.append(np.stack([iid[s], isub[s], ilen[s].astype(np.uint64), ioff[s] - offs[p]], axis=1).astype(np.uint64))
    same(rr.unpack_summary(names, rows.tolist(), items), vec["metadata_unpack"], f"seg_line {seg_line}")
