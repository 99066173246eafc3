"""Batch ends: host-mode chunk edges (host_pipe.hip) and what lies past the last record or block.

Part A runs the host-mode pipeline with 1 MiB chunks (test options host_digest_chunk_mib and
host_chunk_mib), so that batches of a few megabytes take the multi-chunk path: every chunk's kernel
gets a new base alignment c * per * rec_len inside the workspace, every chunk ends next to the next
chunk's bytes (still arriving, or left over from an earlier call), more than 64 chunks wrap the
pipeline's event ring, all-devices parts are chunked too, and several threads share one device's
D2H worker.  Part B runs the device-mode kernels on batches that lie inside a larger buffer of the
test's own, with foreign bytes (0xFF and 0x00) on both sides and pattern guard rows after the
output, and the Blowfish persistent loop at every tail of its 2 x 1024-block iterations with the
words at 8 mod 16.

The shape arithmetic is in pure functions at the top; test_shapes_cover_the_edges (no GPU) asserts
that the shapes chosen below do reach the edges they are meant to reach.  Every comparison is bit
exact against the oracle; hashlib confirms a few records per case.
"""
import contextlib
import hashlib
import threading

import numpy as np
import pytest

from brb_framework_amd import workload

MIB = 1 << 20
K_EVENTS = 64                      # host_pipe.hip kEvents: events reused round-robin by chunk index
GUARD_ROWS = 64                    # digest rows after `out` that must stay untouched (one group)
BF_PER_CHUNK = MIB // 16           # Blowfish blocks per 1 MiB chunk
BF_ITER_PER_CU = 2048              # bf_rep_kernel: 1024 threads x 2 blocks per workgroup and iteration
KEY = workload.CFG4_KEY


# ---- shape arithmetic (pure) -------------------------------------------------------------------
def per_chunk(rec_len, chunk_bytes=MIB):
    """Records per host-mode chunk (host_pipe.hip digest_part / blowfish_part)."""
    return max(1, chunk_bytes // rec_len)


def chunk_plan(n, rec_len, chunk_bytes=MIB):
    """(chunk count, byte bases c * per * rec_len of the chunks, records in the last chunk)."""
    per = per_chunk(rec_len, chunk_bytes)
    count = -(-n // per)
    return count, [c * per * rec_len for c in range(count)], n - (count - 1) * per


def parts_plan(n, parts):
    """Record ranges [lo, hi) of an all-devices split (host_pipe.hip split_devices); one range when
    there are fewer records than parts."""
    if parts <= 1 or n < parts:
        return [(0, n)]
    return [(n * g // parts, n * (g + 1) // parts) for g in range(parts)]


def bf_tail_blocks(cus):
    """Blowfish batch sizes around the persistent grid's iteration I = 2048 * CUs."""
    it = BF_ITER_PER_CU * cus
    return [1023, 1024, 1025, 2047, 2048, 2049, it - 1, it, it + 1, it + 1025, 2 * it + 2047, 3 * it - 2047]


P1500, P1499, P64, P20, PBIG = (per_chunk(x) for x in (1500, 1499, 64, 20, 1_200_000))

# A1: (rec_len, n, b64_kernel or None)
HOST_DIGEST_CASES = [
    (1500, 3 * P1500 + 1, None),       # three full chunks and a last chunk of one record
    (1500, 2 * P1500, None),           # exact multiple: the last chunk is full
    (1499, 4 * P1499 + 5, None),       # chunk bases 0..3 mod 4 (fixed_route VAR_LINE: the var-line kernel)
    (64, 2 * P64 + 65, 2),             # the 64-byte kernels at a chunk edge
    (64, 2 * P64 + 65, 1),
    (20, 2 * P20 + 1, None),
    (1_200_000, 5, None),              # one record per chunk
]
A2_DIGEST = (1500, 70 * P1500 + 3)     # 71 chunks: c % kEvents wraps
A2_BF_BLOCKS = 70 * BF_PER_CHUNK + 7
A3_BF_BLOCKS = [BF_PER_CHUNK + 1, 2 * BF_PER_CHUNK, 3 * BF_PER_CHUNK + 7]
A4_PARTS = 3
A4_DIGEST = (1499, 3 * 2 * P1499 + 2)
A4_BF_BLOCKS = 3 * 2 * BF_PER_CHUNK + 7
A4_FEW = [(1_200_000, 2), (1_200_000, 3)]   # n < parts: the single-part path (two chunks); n == parts

# B2
B2_LENS = [68, 132, 260, 1500, 1532, 1501, 64]
B2_NS = [1, 65, 64 * 33 + 1, 64 * 33 + 63]
B2_BIG = [(132, 64 * 4688 + 1), (260, 64 * 4688 + 1)]   # several groups per wave, one valid row in the last
B2_OFFS = [4, 12]
FOREIGN = 256                      # foreign bytes on each side of a device batch


def test_shapes_cover_the_edges():
    """No GPU: the shapes above reach the edges the GPU tests below are about."""
    assert (P1500, P1499, P64, P20, PBIG, BF_PER_CHUNK) == (699, 699, 16384, 52428, 1, 65536)
    plans = {(L, n): chunk_plan(n, L) for L, n, _ in HOST_DIGEST_CASES}
    for (L, n), (count, bases, last) in plans.items():
        assert count > 1 and per_chunk(L) < n, (L, n)          # the multi-chunk path, not the shortcut
        assert count <= K_EVENTS                                # A1 stays inside the event ring
    # 1500 B x (3 per + 1): four chunks, the last of one record; bases step 52 mod 128 -> 0/4/8/12 mod 16
    count, bases, last = plans[(1500, 3 * P1500 + 1)]
    assert (count, last) == (4, 1)
    assert [b % 128 for b in bases] == [0, 52, 104, 28] and [b % 16 for b in bases] == [0, 4, 8, 12]
    # exact multiple: the last chunk is full
    assert plans[(1500, 2 * P1500)][0] == 2 and plans[(1500, 2 * P1500)][2] == P1500
    # 1499 B: five chunks; the first four bases cover every residue mod 4
    count, bases, last = plans[(1499, 4 * P1499 + 5)]
    assert (count, last) == (5, 5) and sorted(b % 4 for b in bases[:4]) == [0, 1, 2, 3]
    # 64 B: three aligned chunks, the last with one full group and one record
    count, bases, last = plans[(64, 2 * P64 + 65)]
    assert (count, last) == (3, 65) and all(b % 128 == 0 for b in bases)
    count, bases, last = plans[(20, 2 * P20 + 1)]
    assert (count, last) == (3, 1) and [b % 128 for b in bases] == [0, 112, 96]
    count, bases, last = plans[(1_200_000, 5)]
    assert (count, last) == (5, 1)
    # the 4-byte-multiple lengths: at least four distinct chunk-base residues mod 128, one of them
    # off a 16-byte boundary (the 1500 B case alone has them; 64 B and 1 200 000 B chunks are aligned)
    res = {b % 128 for (L, n), (_, bases, _) in plans.items() if L % 4 == 0 for b in bases}
    assert len(res) >= 4 and any(r % 16 for r in res)
    # A2: more chunks than events, for digests and for Blowfish
    count, bases, last = chunk_plan(A2_DIGEST[1], A2_DIGEST[0])
    assert (count, last) == (71, 3) and count > K_EVENTS and len({b % 128 for b in bases}) == 32
    assert chunk_plan(A2_BF_BLOCKS, 16)[0] == 71 and chunk_plan(A2_BF_BLOCKS, 16)[2] == 7
    # A3: two chunks with a one-block tail, two full chunks, four chunks with a 7-block tail
    assert [chunk_plan(nb, 16)[0] for nb in A3_BF_BLOCKS] == [2, 2, 4]
    assert [chunk_plan(nb, 16)[2] for nb in A3_BF_BLOCKS] == [1, BF_PER_CHUNK, 7]
    # A4: every part is itself chunked; digest part bases fall off 4-byte boundaries
    L, n = A4_DIGEST
    parts = parts_plan(n, A4_PARTS)
    assert parts == [(0, 1398), (1398, 2797), (2797, 4196)]
    assert [chunk_plan(hi - lo, L)[0] for lo, hi in parts] == [2, 3, 3]
    assert [lo * L % 4 for lo, _ in parts] == [0, 2, 3]
    parts = parts_plan(A4_BF_BLOCKS, A4_PARTS)
    assert [chunk_plan(hi - lo, 16)[0] for lo, hi in parts] == [3, 3, 3]
    assert parts_plan(2, A4_PARTS) == [(0, 2)] and chunk_plan(2, 1_200_000)[0] == 2
    assert parts_plan(3, A4_PARTS) == [(0, 1), (1, 2), (2, 3)]
    # B1 on an MI355X (256 CUs): at most about 24 MiB; one, two and three iterations of the grid
    # and grids smaller than the CU count; the last workgroup of the last iteration holds 1, 1023,
    # 1024, 1025, 2047 blocks or is full
    sizes = bf_tail_blocks(256)
    assert max(sizes) * 16 <= 24 * MIB and min(sizes) > 0 and len(set(sizes)) == 12
    it = BF_ITER_PER_CU * 256
    assert {-(-nb // it) for nb in sizes} == {1, 2, 3}
    assert {nb % BF_ITER_PER_CU for nb in sizes} >= {0, 1, 1023, 1024, 1025, 2047}
    # B2: the batches end mid-line (the buffer itself is 256-byte aligned).  Five of the 60
    # combinations of length, count and offset end on a line, all at offset 4 (1532 + 4 = 12 lines);
    # they run all the same, and each of those shapes ends mid-line at offset 12.
    shapes = [(L, n) for L in B2_LENS for n in B2_NS] + B2_BIG
    on_line = [(L, n, off) for L, n in shapes for off in B2_OFFS if (off + n * L) % 128 == 0]
    assert on_line == [(132, 2175, 4), (260, 2175, 4), (1532, 1, 4), (1532, 65, 4), (1532, 2113, 4)]
    assert all((12 + n * L) % 128 for L, n in shapes)
    assert all(n % 64 == 1 for _, n in B2_BIG) and {n % 64 for n in B2_NS} == {1, 63}


# ---- helpers --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu(brb):
    assert brb.gpu_available(), brb.lib().BRB_CryptoGPU_LastError()
    return brb


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch
    assert torch.cuda.is_available(), "no HIP device visible to torch"
    return torch


@pytest.fixture(scope="module")
def bf(gpu, orc):
    return gpu.blowfish_init(KEY), orc.bf_init(KEY)


@contextlib.contextmanager
def one_mib_chunks(brb):
    """Both host-mode chunk sizes at 1 MiB, restored on exit."""
    with brb.TestOption("host_digest_chunk_mib", 1), brb.TestOption("host_chunk_mib", 1):
        yield


def pattern_bytes(rows, width):
    return ((np.arange(rows * width, dtype=np.uint32) * 167 + 89) & 0xFF).astype(np.uint8).reshape(rows, width)


def pattern_words(n):
    with np.errstate(over="ignore"):
        return np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)


def pinned(a):
    """A page-locked copy of `a` as a numpy array (a view of the torch tensor that owns the memory)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().numpy()


def digest_fns(brb, orc):
    return ((brb.md5_batch_fixed, orc.md5_batch_fixed, 16, hashlib.md5),
            (brb.sha1_batch_fixed, orc.sha1_batch_fixed, 20, hashlib.sha1))


def check_hashlib(got, data, rec_len, rows, h):
    for r in rows:
        assert got[r].tobytes() == h(data[r * rec_len:(r + 1) * rec_len].tobytes()).digest(), f"record {r}"


def host_digest_case(brb, orc, rec_len, n, pin, **call):
    """One A1-style case, MD5 and SHA-1: dirty the workspace with another batch of the same shape
    through the same entry point, then digest into the first n rows of a pattern array and check the
    digests and the guard rows."""
    data = workload.gen_records(0x5EED0051, 0, n, rec_len)
    dirt = workload.gen_records(0x5EED0052, n, n, rec_len)
    if pin:
        data = pinned(data)
    per = per_chunk(rec_len)
    edges = sorted({0, n - 1} | {r for c in range(1, -(-n // per)) for r in (c * per - 1, c * per)})
    for fn, ofn, width, h in digest_fns(brb, orc):
        want = ofn(data, rec_len, n, threads=16)
        fn(dirt, rec_len, n, **call)
        pat = pattern_bytes(n + GUARD_ROWS, width)
        full = pinned(pat) if pin else pat.copy()
        fn(data, rec_len, n, out=full[:n], **call)
        bad = np.nonzero(~np.all(full[:n] == want, axis=1))[0]
        assert bad.size == 0, f"{fn.__name__}: {bad.size} of {n} digests differ, first at records {bad[:4]}"
        assert np.array_equal(full[n:], pat[n:]), f"{fn.__name__}: rows past the batch were written"
        check_hashlib(full, data, rec_len, edges[:12], h)


def bf_host_round_trip(brb, orc, bf, nb, pin, **call):
    """Blowfish in place inside a host array with pattern guard words on both sides (33 words in
    front: the words start at 8 mod 16, which is all `unsigned long *` promises)."""
    ctx, oc = bf
    front, back = 33, 64
    w = workload.gen_words(workload.SEEDS[4] ^ nb, 2 * nb)
    want = orc.bf_ecb(oc, w.copy(), threads=16)
    pat = pattern_words(front + 2 * nb + back)
    pat[front:front + 2 * nb] = w
    full = pinned(pat) if pin else pat.copy()
    buf = full[front:front + 2 * nb]
    for fn, expect in ((brb.blowfish_encrypt_batch, want), (brb.blowfish_decrypt_batch, w)):
        fn(ctx, buf, **call)
        bad = np.nonzero(buf != expect)[0]
        assert bad.size == 0, f"{fn.__name__}: {bad.size} words differ, first at {bad[:4]} of {2 * nb}"
        end = front + 2 * nb
        assert np.array_equal(full[:front], pat[:front]) and np.array_equal(full[end:], pat[end:]), \
            f"{fn.__name__}: guard words changed"


# ---- A. host mode with 1 MiB chunks ---------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pin", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("rec_len,n,b64", HOST_DIGEST_CASES)
def test_host_digest_chunk_edges(gpu, orc, rec_len, n, b64, pin):
    """A1: fixed-stride digests over several 1 MiB chunks (a full and a one-record last chunk, chunk
    bases at every residue mod 4 and at 0/4/8/12 mod 16, the 64-byte kernels, one record per chunk)
    with a dirtied workspace and guard rows after the output."""
    with one_mib_chunks(gpu), gpu.TestOption("b64_kernel", 2 if b64 is None else b64):
        host_digest_case(gpu, orc, rec_len, n, pin)


@pytest.mark.gpu
def test_host_digest_more_chunks_than_events(gpu, orc):
    """A2: 71 chunks, so the pipeline's 64 events are reused while earlier chunks' D2H copies may
    still be queued; every digest of the batch against the oracle."""
    with one_mib_chunks(gpu):
        host_digest_case(gpu, orc, A2_DIGEST[0], A2_DIGEST[1], False)


@pytest.mark.gpu
def test_host_blowfish_more_chunks_than_events(gpu, orc, bf):
    """A2: the same for Blowfish, 71 chunks each way."""
    with one_mib_chunks(gpu):
        bf_host_round_trip(gpu, orc, bf, A2_BF_BLOCKS, False)


@pytest.mark.gpu
@pytest.mark.parametrize("pin", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("nb", A3_BF_BLOCKS)
def test_host_blowfish_chunk_edges(gpu, orc, bf, nb, pin):
    """A3: Blowfish over 1 MiB chunks (a one-block tail, an exact multiple, a 7-block tail), in
    place between guard words, encrypt against the oracle and decrypt back."""
    with one_mib_chunks(gpu):
        bf_host_round_trip(gpu, orc, bf, nb, pin)


@pytest.mark.gpu
def test_all_devices_parts_are_chunked(gpu, orc, bf):
    """A4: an all-devices split into three parts (on one GPU: three workers, one device) whose
    parts are multi-chunk themselves, digest part bases off 4-byte boundaries; then fewer records
    than parts (one part, two chunks) and as many records as parts."""
    with one_mib_chunks(gpu), gpu.TestOption("devices", A4_PARTS):
        host_digest_case(gpu, orc, A4_DIGEST[0], A4_DIGEST[1], False, all_devices=True)
        bf_host_round_trip(gpu, orc, bf, A4_BF_BLOCKS, False, all_devices=True)
        for rec_len, n in A4_FEW:
            host_digest_case(gpu, orc, rec_len, n, False, all_devices=True)
            bf_host_round_trip(gpu, orc, bf, n, False, all_devices=True)


@pytest.mark.gpu
def test_threads_share_d2h_worker(gpu, orc, bf):
    """A5: four threads, each with its own multi-chunk MD5 batch (4-6 MB, its own record length) and
    multi-chunk Blowfish round trip, three rounds each, odd threads with BRB_BATCH_ALL_DEVICES; all
    of them hand their chunks' D2H copies to the one worker of the device.  Every result exact."""
    ctx, oc = bf
    shapes = [(1500, 3200), (1499, 3500), (1532, 3900), (700, 6500)]
    jobs = []
    for k, (L, n) in enumerate(shapes):
        assert chunk_plan(n, L)[0] >= 4 and 4 * MIB <= n * L <= 6 * MIB
        data = workload.gen_records(0x5EED0060 + k, 0, n, L)
        nb = 4 * BF_PER_CHUNK + 11 * (k + 1)
        w = workload.gen_words(0x5EED0070 + k, 2 * nb)
        jobs.append((L, n, data, orc.md5_batch_fixed(data, L, n, threads=16), w,
                     orc.bf_ecb(oc, w.copy(), threads=16)))
    errs = []

    def run(k):
        L, n, data, want, w, want_bf = jobs[k]
        alld = bool(k & 1)
        try:
            for _ in range(3):
                got = gpu.md5_batch_fixed(data, L, n, all_devices=alld)
                assert np.array_equal(got, want), f"thread {k}: md5 differs"
                buf = w.copy()
                gpu.blowfish_encrypt_batch(ctx, buf, all_devices=alld)
                assert np.array_equal(buf, want_bf), f"thread {k}: blowfish encrypt differs"
                gpu.blowfish_decrypt_batch(ctx, buf, all_devices=alld)
                assert np.array_equal(buf, w), f"thread {k}: blowfish round trip differs"
        except Exception as e:       # noqa: BLE001 -- reported below
            errs.append(repr(e))
        finally:
            gpu.lib().BRB_CryptoGPU_ThreadCleanup()

    with one_mib_chunks(gpu):
        ts = [threading.Thread(target=run, args=(k,), daemon=True) for k in range(4)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=120)
        alive = [k for k, t in enumerate(ts) if t.is_alive()]
    assert not alive, f"threads {alive} did not finish"
    assert not errs, errs


# ---- B. device-mode batch ends ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def bf_dev(gpu, orc, torch_dev, bf):
    """Plaintext and oracle ciphertext of the largest B1 shape, on the device (ECB: a shorter batch
    is a prefix), and the device copy of the context."""
    t = torch_dev
    cus = t.cuda.get_device_properties(0).multi_processor_count
    nb = max(bf_tail_blocks(cus))
    w = workload.gen_words(0x5EED0081, 2 * nb)
    want = orc.bf_ecb(bf[1], w.copy(), threads=16)
    cd = t.frombuffer(bytearray(gpu.blowfish_ctx_bytes(bf[0])), dtype=t.uint8).cuda()
    return cus, t.from_numpy(w.view(np.int64)).cuda(), t.from_numpy(want.view(np.int64)).cuda(), cd


def bf_tail_case(brb, t, bf_dev, nb, start):
    _, plain, want, cd = bf_dev
    back = 1024                                              # 8 KiB of pattern after the words
    pat = t.from_numpy(pattern_words(start + 2 * nb + back).view(np.int64)).cuda()
    buf = pat.clone()
    buf[start:start + 2 * nb] = plain[:2 * nb]
    view = buf[start:start + 2 * nb]
    assert view.data_ptr() % 16 == (8 * start) % 16
    for fn, expect in ((brb.blowfish_encrypt_batch, want), (brb.blowfish_decrypt_batch, plain)):
        fn(cd, view, n_blocks=nb)
        bad = t.nonzero(view != expect[:2 * nb]).flatten()
        assert bad.numel() == 0, f"{fn.__name__}: {bad.numel()} words differ, first at {bad[:4].tolist()} of {2 * nb}"
        assert t.equal(buf[:start], pat[:start]) and t.equal(buf[start + 2 * nb:], pat[start + 2 * nb:]), \
            f"{fn.__name__}: words outside the batch changed"


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(12))
def test_blowfish_persistent_loop_tails(gpu, torch_dev, bf_dev, idx):
    """B1: bf_rep_kernel around its iteration of 2048 blocks per workgroup and 2048 x CUs per grid
    (see bf_tail_blocks), the words at 8 mod 16 inside a pattern buffer: every word against the
    oracle, the pattern intact on both sides, and back."""
    nb = bf_tail_blocks(bf_dev[0])[idx]
    bf_tail_case(gpu, torch_dev, bf_dev, nb, 1)


@pytest.mark.gpu
def test_blowfish_persistent_loop_tail_aligned(gpu, torch_dev, bf_dev):
    """B1 at a 16-byte aligned base, 4 KiB of pattern in front."""
    it = BF_ITER_PER_CU * bf_dev[0]
    bf_tail_case(gpu, torch_dev, bf_dev, it + 1025, 512)


def device_digest_case(brb, t, data_dev, want, fn, width, rec_len, n, off, fill):
    size = n * rec_len
    d = t.full((FOREIGN + off + size + FOREIGN + 64,), fill, dtype=t.uint8, device="cuda")
    assert d.data_ptr() % 256 == 0
    view = d[FOREIGN + off:FOREIGN + off + size]
    view.copy_(data_dev[:size])
    pat = t.from_numpy(pattern_bytes(n + GUARD_ROWS, width)).cuda()
    full = pat.clone()
    fn(view, rec_len, n, out=full[:n])
    what = f"{fn.__name__} rec_len {rec_len} n {n} off {off} fill {fill:#x}"
    bad = t.nonzero((full[:n] != want[:n]).any(dim=1)).flatten()
    assert bad.numel() == 0, f"{what}: {bad.numel()} digests differ, first at records {bad[:4].tolist()}"
    assert t.equal(full[n:], pat[n:]), f"{what}: rows past the batch were written"


def device_digest_shapes(brb, orc, t, rec_len, ns):
    n_max = max(ns)
    data = workload.gen_records(0x5EED0090 ^ rec_len, 0, n_max, rec_len)
    data_dev = t.from_numpy(data).cuda()
    for fn, ofn, width, h in digest_fns(brb, orc):
        want_h = ofn(data, rec_len, n_max, threads=16)
        check_hashlib(want_h, data, rec_len, sorted({0, n_max - 1} | {n - 1 for n in ns}), h)
        want = t.from_numpy(want_h).cuda()
        for n in ns:
            for off in B2_OFFS:
                for fill in (0xFF, 0x00):
                    device_digest_case(brb, t, data_dev, want, fn, width, rec_len, n, off, fill)


@pytest.mark.gpu
@pytest.mark.parametrize("rec_len", B2_LENS)
def test_fixed_digests_next_to_foreign_bytes(gpu, orc, torch_dev, rec_len):
    """B2: fixed-stride batches whose last group holds 1 or 63 valid rows, at 4 and 12 mod 128 in a
    buffer whose other bytes are 0xFF and then 0x00, ending mid-line: the digests equal the oracle
    either way (nothing past the batch end reaches a digest) and the rows after `out` stay as they
    were (no digest is stored for the rows past n)."""
    device_digest_shapes(gpu, orc, torch_dev, rec_len, B2_NS)
    if rec_len == 64:                       # the other 64-byte kernels (2 is the default, run above)
        for kernel in (1, 3, 0):
            with gpu.TestOption("b64_kernel", kernel):
                device_digest_shapes(gpu, orc, torch_dev, rec_len, B2_NS)


@pytest.mark.gpu
@pytest.mark.parametrize("rec_len,n", B2_BIG)
def test_fixed_digests_next_to_foreign_bytes_many_groups(gpu, orc, torch_dev, rec_len, n):
    """B2 with 4 689 groups, so every wave takes several and the last group has one valid row."""
    device_digest_shapes(gpu, orc, torch_dev, rec_len, [n])


def var_case(n, seed):
    """n back-to-back records of 0..700 bytes, the last one non-empty and ending the pool."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 701, n).astype(np.uint32)
    lens[-1] = 1 + int(rng.integers(0, 700))
    offs = (np.cumsum(lens.astype(np.uint64)) - lens).astype(np.uint64)
    pool = workload.gen_records(0x5EED00A0 + seed, 0, 1, int(lens.astype(np.uint64).sum()))
    assert int(offs[-1]) + int(lens[-1]) == pool.size
    return pool, offs, lens


def in_ff(t, pool):
    """`pool` on the device between two runs of FOREIGN 0xFF bytes; returns the view of the pool."""
    d = t.full((FOREIGN + pool.size + FOREIGN,), 0xFF, dtype=t.uint8, device="cuda")
    view = d[FOREIGN:FOREIGN + pool.size]
    view.copy_(t.from_numpy(pool).cuda())
    return view


def check_guarded(t, call, want_h, n, width, what):
    pat = t.from_numpy(pattern_bytes(n + GUARD_ROWS, width)).cuda()
    full = pat.clone()
    call(full[:n])
    assert np.array_equal(full[:n].cpu().numpy(), want_h), f"{what}: digests differ from the oracle"
    assert t.equal(full[n:], pat[n:]), f"{what}: rows past the batch were written"


@pytest.mark.gpu
@pytest.mark.parametrize("var_line", [1, 0])
@pytest.mark.parametrize("n", [1, 65, 64 * 9 + 1])
def test_variable_digests_output_guard(gpu, orc, torch_dev, n, var_line):
    """B3: BRB_MD5Batch and BrbSha1_Batch in device mode, the last record ending on the last byte
    before 0xFF fill, `out` followed by guard rows; the line-staged kernel and the per-lane one."""
    t = torch_dev
    pool, offs, lens = var_case(n, n)
    view = in_ff(t, pool)
    o, ln = t.from_numpy(offs.view(np.int64)).cuda(), t.from_numpy(lens.view(np.int32)).cuda()
    with gpu.TestOption("var_line", var_line):
        for fn, ofn, width in ((gpu.md5_batch, orc.md5_batch, 16), (gpu.sha1_batch, orc.sha1_batch, 20)):
            check_guarded(t, lambda out: fn(view, o, ln, out=out), ofn(pool, offs, lens), n, width,
                          f"{fn.__name__} n {n} var_line {var_line}")


@pytest.mark.gpu
@pytest.mark.parametrize("seg_line", [2, 1, 0])
@pytest.mark.parametrize("n", [1, 65, 64 * 9 + 1])
def test_segment_digests_output_guard(gpu, orc, torch_dev, n, seg_line):
    """B3: BRB_MD5BatchSegments in device mode: records of 1..3 segments cut from back-to-back
    spans, the last segment ending on the last byte before 0xFF fill, `out` followed by guard rows;
    the wave-pair, single-wave and per-lane kernels."""
    t = torch_dev
    rng = np.random.default_rng(1000 + n)
    first = np.zeros(n + 1, np.uint64)
    first[1:] = np.cumsum(rng.integers(1, 4, n))
    pool, offs, lens = var_case(int(first[-1]), 2000 + n)
    want = np.frombuffer(b"".join(
        orc.md5(b"".join(pool[int(offs[k]):int(offs[k]) + int(lens[k])].tobytes()
                         for k in range(int(first[i]), int(first[i + 1])))) for i in range(n)), np.uint8).reshape(n, 16)
    view = in_ff(t, pool)
    o, ln, fi = t.from_numpy(offs).cuda(), t.from_numpy(lens).cuda(), t.from_numpy(first).cuda()
    with gpu.TestOption("seg_line", seg_line):
        check_guarded(t, lambda out: gpu.md5_batch_segments(view, o, ln, fi, out=out), want, n, 16,
                      f"BRB_MD5BatchSegments n {n} seg_line {seg_line}")
