"""Which kernel a fixed-stride digest call runs, pinned, and every route run with data.

BRB_MD5BatchFixed and BrbSha1_BatchFixed pick one of nine kernels from the record length, the base
alignment and the test options fixed_var_line and b64_kernel (csrc/gpu/fixed_route.h).  The choice
is exported as BRB_CryptoGPU_TestFixedRoute, so a test can ask which kernel a shape reaches instead
of saying so in a comment:

    0 LANE_A4     rec_len == 0 or >= 33 554 431, base and length 4-byte multiples (per lane)
    1 LANE_ANY    the same lengths otherwise (per lane)
    2 LINE        64 < rec_len <= 1 MiB, base and length 4-byte multiples
    3 VAR_LINE    64 < rec_len <= 1 MiB otherwise, fixed_var_line = 1 (default)
    4 DMA_TICKET  every other rec_len > 64 (in the product: 1 MiB < rec_len <= 33 554 430)
    5 6 7         rec_len == 64 under b64_kernel 2 (default) / 3 / 1
    8 DMA_SHORT   1 <= rec_len <= 64 otherwise

The CPU part pins that table on both sides of every boundary and asserts (test_cases_cover_every_route)
that the GPU cases below, which live in module-level tables, reach every row with an aligned and an
unaligned `out`.  The GPU part runs them in device mode: every batch lies at a chosen residue mod 4
inside a larger buffer with FOREIGN bytes of 0xFF, then of 0x00, on both sides, `out` lies inside a
pattern buffer that must stay untouched around it, every digest is compared with the oracle and
hashlib confirms a few records per case.  Each GPU case asserts the route of the pointer it passes.
"""
import collections
import hashlib

import numpy as np
import pytest

from brb_framework_amd import workload

MIB = 1 << 20
L_TOP = 33_554_430                 # the longest record the LDS-DMA kernels take (dma_supported)
FOREIGN = 256                      # foreign bytes on each side of a device batch
GUARD_ROWS = 64                    # pattern rows after `out` that must stay untouched (one group)
WAVES = 8                          # waves per workgroup of the ticketed kernel (row 4)
(LANE_A4, LANE_ANY, LINE, VAR_LINE, DMA_TICKET, B64R_8, B64R_4, B64, DMA_SHORT) = range(9)

ROUTE_LENGTHS = [0, 1, 63, 64, 65, MIB, MIB + 1, MIB + 4, L_TOP, L_TOP + 1, L_TOP + 2, 2**32 - 1]

# One GPU case: the route it must take, its shape, the base residues mod 4, the byte offsets of `out`
# inside its (256-byte aligned) pattern buffer, and the test options it runs under.
Case = collections.namedtuple("Case", "row rec_len ns residues out_offs opts")
NO_VAR_LINE = (("fixed_var_line", 0),)

# Row 4 at small shapes (fixed_var_line = 0): t = 0 (128, 192, 256, 1536; at residue 0 these are the
# line kernel's), t >= 56 (127, 191), an odd and an even block count (the last 128-byte
# stage half used or full), both issue forms (rec_len < 128: one M0 write per DMA).
ROW4_NS = (1, 63, 64, 65, 64 * 33 + 1)
ROW4_SMALL = ([Case(DMA_TICKET, L, ROW4_NS, (0, 1, 2, 3), (0, 1), NO_VAR_LINE) for L in (65, 127, 129, 191, 193, 1499, 1501)]
              + [Case(DMA_TICKET, L, ROW4_NS, (1, 2, 3), (0, 1), NO_VAR_LINE) for L in (128, 192, 256, 1536)])
ROW4_ALIGNED_TO_LINE = (128, 192, 256, 1536)


def tickets_n(cus):
    """Records for which every workgroup of the ticketed kernel (one per CU) owns 2 x 8 groups, so
    its eight waves all come back for tickets, plus one group of a single valid row."""
    return 64 * (2 * WAVES * cus) + 1


# n is tickets_n(CUs) at run time
ROW4_TICKETS = [Case(DMA_TICKET, L, None, (3,), (0, 1), NO_VAR_LINE) for L in (129, 1501)]
# rows 0 and 1 with data: three records of 32 MiB, one lane each
LANE_CASES = [Case(LANE_A4, 1 << 25, (3,), (0,), (0, 1), ()),
              Case(LANE_ANY, 1 << 25, (3,), (1,), (0, 1), ()),
              Case(LANE_ANY, (1 << 25) - 1, (3,), (0,), (0, 1), ())]
# row 4 at the longest record it takes: one group of 64 records, 2 GiB
ROW4_TOP = [Case(DMA_TICKET, L_TOP, (64,), (0,), (0, 1), ())]
# the other rows with `out` off its natural alignment (16 bytes for MD5, 4 for SHA-1)
OTHER_ROWS = [Case(LINE, 1500, (65,), (0,), (0, 1, 2), ()),
              Case(VAR_LINE, 1501, (65,), (1,), (0, 1, 2), ()),
              Case(B64R_8, 64, (65,), (0,), (0, 1, 2), (("b64_kernel", 2),)),
              Case(B64R_4, 64, (65,), (0,), (0, 1, 2), (("b64_kernel", 3),)),
              Case(B64, 64, (65,), (0,), (0, 1, 2), (("b64_kernel", 1),)),
              Case(DMA_SHORT, 64, (65,), (0,), (0, 1, 2), (("b64_kernel", 0),)),
              Case(DMA_SHORT, 20, (65,), (3,), (0, 1, 2), ())]
ALL_CASES = ROW4_SMALL + ROW4_TICKETS + LANE_CASES + ROW4_TOP + OTHER_ROWS


def table_route(addr, rec_len, fixed_var_line=1, b64_kernel=2):
    """The routing table of this file's header, restated."""
    a4 = addr % 4 == 0 and rec_len % 4 == 0
    if rec_len == 0 or 64 * rec_len + 64 >= 1 << 31:
        return LANE_A4 if a4 else LANE_ANY
    if 64 < rec_len <= MIB:
        if a4:
            return LINE
        if fixed_var_line:
            return VAR_LINE
    if rec_len > 64:
        return DMA_TICKET
    if rec_len == 64 and b64_kernel:
        return {2: B64R_8, 3: B64R_4, 1: B64}[b64_kernel]
    return DMA_SHORT


def out_is_aligned(width, out_off):
    return out_off % (16 if width == 16 else 4) == 0


@pytest.fixture
def with_opts(brb):
    import contextlib

    @contextlib.contextmanager
    def enter(opts):
        with contextlib.ExitStack() as st:
            for name, value in opts:
                st.enter_context(brb.TestOption(name, value))
            yield
    return enter


# ---- CPU part -------------------------------------------------------------------------------------
def test_route_values_match_the_header(brb):
    names = ["LANE_A4", "LANE_ANY", "LINE", "VAR_LINE", "DMA_TICKET", "B64R_8", "B64R_4", "B64", "DMA_SHORT"]
    assert [getattr(brb, "FIXED_ROUTE_" + n) for n in names] == list(range(9))
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "brb_crypto.h")).read()
    assert re.findall(r"#define BRB_FIXED_ROUTE_(\w+)\s+(\d+)", hdr) == [(n, str(i)) for i, n in enumerate(names)]


def test_fixed_route_table(brb):
    """BRB_CryptoGPU_TestFixedRoute against the table, on both sides of every boundary, at every
    address residue, under both values of fixed_var_line and all four of b64_kernel."""
    base = 0x7F00_0000_1000
    for fvl in (0, 1):
        for b64 in (0, 1, 2, 3):
            with brb.TestOption("fixed_var_line", fvl), brb.TestOption("b64_kernel", b64):
                for L in ROUTE_LENGTHS:
                    for res in range(4):
                        assert brb.fixed_route(base + res, L) == table_route(res, L, fvl, b64), (L, res, fvl, b64)
    # the same, spelled out (defaults: fixed_var_line 1, b64_kernel 2); rows by residue 0..3
    pins = {0: [0, 1, 1, 1], 1: [8] * 4, 63: [8] * 4, 64: [5] * 4, 65: [3] * 4, MIB: [2, 3, 3, 3],
            MIB + 1: [4] * 4, MIB + 4: [4] * 4, L_TOP: [4] * 4, L_TOP + 1: [1] * 4, L_TOP + 2: [0, 1, 1, 1],
            2**32 - 1: [1] * 4}
    assert sorted(pins) == sorted(ROUTE_LENGTHS)
    for L, rows in pins.items():
        assert [brb.fixed_route(base + res, L) for res in range(4)] == rows, L
    with brb.TestOption("fixed_var_line", 0):
        assert [brb.fixed_route(base + res, 65) for res in range(4)] == [4] * 4
        assert [brb.fixed_route(base + res, MIB) for res in range(4)] == [2, 4, 4, 4]
        assert [brb.fixed_route(base + res, 1500) for res in range(4)] == [2, 4, 4, 4]
    for b64, row in ((0, 8), (1, 7), (2, 5), (3, 6)):
        with brb.TestOption("b64_kernel", b64):
            assert [brb.fixed_route(base + res, 64) for res in range(4)] == [row] * 4
            assert brb.fixed_route(base, 63) == 8 and brb.fixed_route(base, 65) == 3
    # the address is taken as 64 bits; only its residue mod 4 matters
    assert brb.fixed_route(2**64 - 4, 1500) == 2 and brb.fixed_route(2**64 - 3, 1500) == 3


def test_longest_dma_record_stays_below_the_descriptor_clamp():
    """Lane 63's largest offset from a group's descriptor base, 63 rec_len + 3072 + 112 (row 63, the
    fourth DMA's instruction offset, the last granule of a 128-byte stage), and the 16 bytes it
    loads stay inside the clamped extent 0x7FFFFFFF for the last length the DMA kernels take."""
    assert 63 * L_TOP + 3072 + 112 == 2_113_932_274 < 2**31
    assert 63 * L_TOP + 3072 + 112 + 16 <= 0x7FFFFFFF
    assert 64 * L_TOP + 64 < 2**31 <= 64 * (L_TOP + 1) + 64


def test_cases_cover_every_route(brb, with_opts):
    """No GPU: the case tables reach every row 0..8 with an aligned and an unaligned `out` for both
    digests, row 4 with both issue forms, and the shapes have the properties the GPU tests are about."""
    seen = collections.defaultdict(set)
    for c in ALL_CASES:
        with with_opts(c.opts):
            for res in c.residues:
                assert brb.fixed_route(0x1000 + FOREIGN + res, c.rec_len) == c.row, c
        for width in (16, 20):
            for off in c.out_offs:
                seen[c.row].add((width, out_is_aligned(width, off), c.rec_len < 128))
    for row in range(9):
        got = {(w, al) for w, al, _ in seen[row]}
        assert got == {(16, True), (16, False), (20, True), (20, False)}, f"row {row}: {sorted(got)}"
    assert {short for _, _, short in seen[DMA_TICKET]} == {True, False}
    # row 4's small lengths: the ones that are 4-byte multiples belong to the line kernel at residue 0
    for L in ROW4_ALIGNED_TO_LINE:
        with brb.TestOption("fixed_var_line", 0):
            assert brb.fixed_route(0x1000, L) == LINE
            assert [brb.fixed_route(0x1000 + r, L) for r in (1, 2, 3)] == [DMA_TICKET] * 3
    lens = [c.rec_len for c in ROW4_SMALL]
    assert sorted(lens) == [65, 127, 128, 129, 191, 192, 193, 256, 1499, 1501, 1536]
    assert {L % 64 for L in lens} >= {0, 1, 63} and any(L % 64 >= 56 for L in lens)
    blocks = {(L // 64 + (1 if L % 64 else 0)) % 2 for L in lens}       # blocks that hold record bytes
    assert blocks == {0, 1}
    assert {n % 64 for n in ROW4_NS} == {0, 1, 63} and max(ROW4_NS) > 64 * 32
    # the ticket shape on 256 CUs: 16 groups per workgroup and one more, the last with one valid row
    n = tickets_n(256)
    assert n == 262_145 and (n + 63) // 64 == 2 * WAVES * 256 + 1 and n % 64 == 1
    assert [c.rec_len for c in ROW4_TICKETS] == [129, 1501] and all(c.residues == (3,) for c in ROW4_TICKETS)
    assert n * 1501 < 400_000_000
    # rows 0 and 1: three records; the top of row 4: one whole group, 2 GiB
    assert [(c.rec_len, c.residues, c.row) for c in LANE_CASES] == [(33_554_432, (0,), 0), (33_554_432, (1,), 1),
                                                                    (33_554_431, (0,), 1)]
    assert ROW4_TOP[0].rec_len * 64 == 2**31 - 128


# ---- GPU part -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu(brb):
    assert brb.gpu_available(), brb.lib().BRB_CryptoGPU_LastError()
    return brb


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch
    assert torch.cuda.is_available(), "no HIP device visible to torch"
    return torch


def algs(brb, orc):
    return {"md5": (brb.md5_batch_fixed, orc.md5_batch_fixed, 16, hashlib.md5),
            "sha1": (brb.sha1_batch_fixed, orc.sha1_batch_fixed, 20, hashlib.sha1)}


def pattern(t, nbytes):
    a = ((np.arange(nbytes, dtype=np.uint32) * 167 + 89) & 0xFF).astype(np.uint8)
    return t.from_numpy(a).cuda()


def embed(t, nbytes, res):
    """A 256-byte aligned buffer with room for nbytes at FOREIGN + res; returns (buffer, view)."""
    d = t.empty(FOREIGN + res + nbytes + FOREIGN + 64, dtype=t.uint8, device="cuda")
    assert d.data_ptr() % 256 == 0
    return d, d[FOREIGN + res:FOREIGN + res + nbytes]


def fill_around(d, nbytes, res, fill):
    d[:FOREIGN + res] = fill
    d[FOREIGN + res + nbytes:] = fill


def check_call(brb, t, fn, width, view, rec_len, n, want, row, out_off, what):
    """One call on `view` with `out` at byte out_off of a pattern buffer; `want` is a device tensor."""
    assert brb.fixed_route(view.data_ptr(), rec_len) == row, f"{what}: route"
    pat = pattern(t, 16 + (n + GUARD_ROWS) * width)
    full = pat.clone()
    assert full.data_ptr() % 256 == 0
    lo, hi = out_off, out_off + n * width
    fn(view, rec_len, n, out=full[lo:hi].view(n, width))
    bad = t.nonzero((full[lo:hi].view(n, width) != want[:n]).any(dim=1)).flatten()
    assert bad.numel() == 0, f"{what}: {bad.numel()} of {n} digests differ, first at records {bad[:4].tolist()}"
    assert t.equal(full[:lo], pat[:lo]) and t.equal(full[hi:], pat[hi:]), f"{what}: bytes around `out` were written"


def check_hashlib(want_h, host, rec_len, rows, h):
    for r in rows:
        assert want_h[r].tobytes() == h(host[r * rec_len:(r + 1) * rec_len].tobytes()).digest(), f"record {r}"


def run_small_case(brb, orc, t, c):
    """A case whose data is a prefix of one generated batch: every n, residue, `out` offset and fill."""
    n_max = max(c.ns)
    data = workload.gen_records(0x5EED00B0 ^ c.rec_len, 0, n_max, c.rec_len)
    data_dev = t.from_numpy(data).cuda()
    for name, (fn, ofn, width, h) in algs(brb, orc).items():
        want_h = ofn(data, c.rec_len, n_max, threads=16)
        check_hashlib(want_h, data, c.rec_len, sorted({0, n_max - 1} | {n - 1 for n in c.ns}), h)
        want = t.from_numpy(want_h).cuda()
        for n in c.ns:
            for res in c.residues:
                d, view = embed(t, n * c.rec_len, res)
                view.copy_(data_dev[:n * c.rec_len])
                for fill in (0xFF, 0x00):
                    fill_around(d, n * c.rec_len, res, fill)
                    for off in c.out_offs:
                        check_call(brb, t, fn, width, view, c.rec_len, n, want, c.row, off,
                                   f"{name} rec_len {c.rec_len} n {n} residue {res} out+{off} fill {fill:#x}")


def run_big_case(brb, orc, t, c, n, res, names, out_offs, oracle_rows=None):
    """A case generated on the device (seeded), copied to the host once for the oracle and hashlib."""
    size = n * c.rec_len
    d, view = embed(t, size, res)
    g = t.Generator(device="cuda").manual_seed(c.rec_len ^ n)
    view.random_(generator=g)                      # uint8: every value 0..255
    host = view.cpu().numpy()
    for name in names:
        fn, ofn, width, h = algs(brb, orc)[name]
        want_h = ofn(host, c.rec_len, n, threads=16)
        check_hashlib(want_h, host, c.rec_len, sorted({0, 1, n - 2, n - 1} & set(range(n))), h)
        want = t.from_numpy(want_h).cuda()
        for fill in (0xFF, 0x00):
            fill_around(d, size, res, fill)
            for off in out_offs:
                check_call(brb, t, fn, width, view, c.rec_len, n, want, c.row, off,
                           f"{name} rec_len {c.rec_len} n {n} residue {res} out+{off} fill {fill:#x}")
    del d, view
    t.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ROW4_SMALL, ids=lambda c: str(c.rec_len))
def test_ticketed_dma_kernel_small_shapes(gpu, orc, torch_dev, with_opts, case):
    """Row 4 (digest_fixed_dma_kernel with ticketed groups) under fixed_var_line = 0, at lengths with
    t = 0, t >= 56, odd and even block counts and both issue forms, batch sizes 1, 63, 64, 65 and
    64 x 33 + 1, every base residue that routes here, `out` aligned and at +1."""
    with with_opts(case.opts):
        run_small_case(gpu, orc, torch_dev, case)


@pytest.mark.gpu
@pytest.mark.parametrize("alg", ["md5", "sha1"])
@pytest.mark.parametrize("case", ROW4_TICKETS, ids=lambda c: str(c.rec_len))
def test_ticketed_dma_kernel_every_wave_takes_tickets(gpu, orc, torch_dev, with_opts, case, alg):
    """Row 4 with 2 x 8 groups per workgroup and one more: every wave takes tickets past its first
    group (take() returns live groups, the ring prefetches across group boundaries, each slot
    remembers its group), and the last group, reached through a ticket, holds one valid row."""
    n = tickets_n(torch_dev.cuda.get_device_properties(0).multi_processor_count)
    with with_opts(case.opts):
        run_big_case(gpu, orc, torch_dev, case, n, case.residues[0], [alg], case.out_offs)


@pytest.mark.gpu
@pytest.mark.parametrize("out_off", [0, 1])
@pytest.mark.parametrize("alg", ["md5", "sha1"])
@pytest.mark.parametrize("case", LANE_CASES, ids=lambda c: f"{c.rec_len}-res{c.residues[0]}")
def test_per_lane_kernels_hash_data(gpu, orc, torch_dev, case, alg, out_off):
    """Rows 0 and 1 (the per-lane kernels) on three records of 32 MiB (and of 32 MiB - 1): the
    one-block software prefetch, tail_word_a4, the FIXED form of the BlockSrc loop and both stores."""
    run_big_case(gpu, orc, torch_dev, case, case.ns[0], case.residues[0], [alg], [out_off])


@pytest.mark.gpu
@pytest.mark.parametrize("rec_len", [1 << 25, (1 << 25) - 1])
def test_per_lane_kernels_host_mode(gpu, orc, rec_len):
    """Host mode, MD5: three records of 32 MiB, one record per 32 MiB chunk of the pipeline."""
    n = 3
    host = np.random.default_rng(rec_len).integers(0, 256, n * rec_len, dtype=np.uint8)
    want = orc.md5_batch_fixed(host, rec_len, n, threads=16)
    check_hashlib(want, host, rec_len, range(n), hashlib.md5)
    pat = ((np.arange((n + GUARD_ROWS) * 16, dtype=np.uint32) * 167 + 89) & 0xFF).astype(np.uint8).reshape(-1, 16)
    full = pat.copy()
    gpu.md5_batch_fixed(host, rec_len, n, out=full[:n])
    assert np.array_equal(full[:n], want)
    assert np.array_equal(full[n:], pat[n:]), "rows past the batch were written"


@pytest.mark.gpu
@pytest.mark.parametrize("alg", ["md5", "sha1"])
def test_ticketed_dma_kernel_longest_record(gpu, orc, torch_dev, alg):
    """Row 4 at rec_len = 33 554 430, the last length dma_supported accepts: one group of 64 records
    in a 2 GiB buffer, lane 63's offsets just below the descriptor's clamped extent.  All 64 digests
    against the oracle, records 0, 1, 62 and 63 against hashlib."""
    case = ROW4_TOP[0]
    run_big_case(gpu, orc, torch_dev, case, case.ns[0], case.residues[0], [alg], case.out_offs)


@pytest.mark.gpu
@pytest.mark.parametrize("case", OTHER_ROWS, ids=lambda c: f"row{c.row}-{c.rec_len}")
def test_unaligned_out_on_every_other_route(gpu, orc, torch_dev, with_opts, case):
    """Rows 2, 3 and 5..8 at n = 65 with `out` aligned, at +1 and at +2 (MD5 stores 16-byte rows,
    SHA-1 five dwords: +2 is unaligned for both, and SHA-1's only 2-byte aligned case)."""
    with with_opts(case.opts):
        run_small_case(gpu, orc, torch_dev, case)
