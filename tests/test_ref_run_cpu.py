"""The oracle, the host compat C and make_golden.py's BigIntBlowfish against vectors that the
reference's own code produced (tests/golden/ref_run/, recorded by tests/golden/make_ref_run.py from a
build of the reference's units, oracle/ref_build/).  No GPU.

The fixture tests need nothing but the committed files and always run.  The live tests load
oracle/_ref/libbrb_ref.so, which exists only where a checkout of the reference was present at build
time; elsewhere they skip and say which file is missing.  They check that the reference still
reproduces the committed files, and run a seeded differential of the oracle against it that reaches
far more inputs than the files hold.

test_every_batch_export_is_pinned reads the *Batch* exports out of include/brb_crypto.h and requires
each to be compared with these vectors in tests/test_ref_run.py, or to be excluded there by name with
a reason.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import ref_run_cases as rr  # noqa: E402

COMPAT_FAMILIES = ("blowfish", "md5", "sha1", "rc4")


def check_family(api, fam):
    bad = rr.differences(rr.FAMILY_FN[fam](api), rr.load(fam))
    assert not bad, f"{api.name} differs from the reference's {fam} vectors:\n" + "\n".join(bad[:8])


# ---- fixture tests: always run -----------------------------------------------------------------------
def test_fixture_files_are_complete():
    have = sorted(f for f in os.listdir(rr.REF_DIR))
    assert have == sorted(f + ".json" for f in rr.FAMILIES)
    for f in have:
        assert os.path.getsize(os.path.join(rr.REF_DIR, f)) <= 61440, f
    assert rr.load("metadata_unpack")["n"] == len(rr.md_unpack_cases())
    widest = {k: v["widest_bits"] for k, v in rr.load("blowfish")["contexts"].items()}
    assert all(32 < b <= 64 for b in widest.values()), widest       # the 64-bit carries are in the vectors


@pytest.mark.parametrize("fam", rr.FAMILIES)
def test_oracle_equals_reference_vectors(orc, fam):
    api = rr.OracleApi(orc)
    assert rr.supports(api, fam)
    check_family(api, fam)


@pytest.mark.parametrize("fam", COMPAT_FAMILIES)
def test_compat_equals_reference_vectors(brb, fam):
    """BRB_MD5*, BrbSha1_* (with the rewritten caller buffer), BRB_Blowfish_*, BRB_RC4_* and BRB_MemBufferKey
    of csrc/host/: context and state images byte for byte."""
    check_family(rr.CompatApi(brb), fam)


def test_compat_families_are_all_the_compat_code_has(brb):
    api = rr.CompatApi(brb)
    assert [f for f in rr.FAMILIES if rr.supports(api, f)] == list(COMPAT_FAMILIES)
    assert not hasattr(brb.lib(), "brb_base64_encode_bin")           # base64 has no host compat entry point to pin


def test_bigint_blowfish_equals_reference_vectors():
    """tests/golden/make_golden.py's big-integer Blowfish, the second restatement: every recorded context word
    and every recorded ECB word."""
    from make_golden import BigIntBlowfish
    want = rr.load("blowfish")
    for name, key, n in rr.bf_keys():
        b = BigIntBlowfish(key, n)
        assert rr.bf_image(b.ctx_bytes()) == {k: want["contexts"][name][k] for k in ("P", "S_sha256", "sha256", "widest_bits")}, name
    for n, blocks in rr.BF_ECB:
        b = BigIntBlowfish(rr.bf_key(n), n)
        for cls in rr.BF_CLASSES:
            w = rr.bf_words(n, blocks, cls).tolist()
            for name, fn in (("encrypt", b.encrypt), ("decrypt", b.decrypt)):
                out = np.array([v for k in range(0, len(w), 2) for v in fn(w[k], w[k + 1])], np.uint64)
                assert rr.bulk_words(out) == want["ecb"][f"len{n}_{blocks}_{cls}"][name], (n, cls, name)


def batch_exports():
    hdr = open(os.path.join(rr.ROOT, "include", "brb_crypto.h")).read()
    names = re.findall(r"^\w[\w \*]*?\b(BRB_\w+|BrbSha1_\w+)\(", hdr, re.M)
    return [n for n in names if "Batch" in n]


def test_every_batch_export_is_pinned():
    import test_ref_run as gpu_tests
    exports = batch_exports()
    assert len(exports) >= 45 and "BRB_MD5BatchFixed" in exports and "BRB_MemBufferDecryptBatch" in exports
    covered = gpu_tests.PINNED
    excluded = {n: why for n in exports for pat, why in gpu_tests.EXCLUDED.items() if re.fullmatch(pat, n)}
    assert not set(covered) & set(excluded)
    missing = [n for n in exports if n not in covered and n not in excluded]
    assert not missing, f"batch exports that tests/test_ref_run.py neither pins nor excludes: {missing}"
    stale = [n for n in covered if n not in exports] + [p for p in gpu_tests.EXCLUDED if not any(re.fullmatch(p, n) for n in exports)]
    assert not stale, f"names that include/brb_crypto.h no longer exports: {stale}"
    for n, tests in covered.items():
        for t in tests:
            fn = getattr(gpu_tests, t, None)
            assert callable(fn) and t.startswith("test_"), (n, t)
            assert any(m.name == "gpu" for m in getattr(fn, "pytestmark", [])), t
    for n, reason in excluded.items():                   # only the frame, open, list, mixed and batcher calls
        assert len(reason) > 20, n
        assert re.search(r"RC4MD5_(Frame|Open)|ListBatch|TransformBatcher", n), f"{n} may not be excluded"
    print("\n".join(f"{n}: " + (", ".join(covered[n]) if n in covered else "excluded: " + excluded[n]) for n in exports))


# ---- live tests: only where the reference was built ---------------------------------------------------
@pytest.fixture(scope="module")
def ref():
    if not os.path.exists(rr.REF_LIB):
        pytest.skip(f"{os.path.relpath(rr.REF_LIB, rr.ROOT)} is missing (built by oracle/ref_build where the reference is present)")
    return rr.RefApi()


@pytest.mark.parametrize("fam", rr.FAMILIES)
def test_live_reference_reproduces_the_fixtures(ref, fam):
    from make_ref_run import text_of
    with open(os.path.join(rr.REF_DIR, fam + ".json")) as f:
        assert f.read() == text_of(rr.FAMILY_FN[fam](ref)), f"run tests/golden/make_ref_run.py --check"


N_FUZZ = 300


def test_differential_blowfish(ref, orc):
    o, rng = rr.OracleApi(orc), np.random.default_rng(rr.SEED + 1)
    for k in range(N_FUZZ):
        key = rng.integers(0, 256, int(rng.integers(1, 73)), dtype=np.uint8).tobytes()
        n = int(rng.integers(1, len(key) + 1)) if k % 4 == 0 else len(key)         # a keyLen below the buffer's
        a, b = ref.bf_init(key, n), o.bf_init(key, n)
        assert a == b, (key.hex(), n)
        w = rng.integers(0, 1 << 64, 16, dtype=np.uint64)
        w[k % 16] &= np.uint64(0xFFFFFFFF)
        for dec in (False, True):
            assert np.array_equal(ref.bf_ecb(a, w, dec), o.bf_ecb(a, w, dec)), (key.hex(), dec)


def _cuts(rng, n):
    k = int(rng.integers(0, 4))
    return [0] + sorted(int(c) for c in rng.integers(0, n + 1, k)) + [n]


def test_differential_digests(ref, orc):
    o, rng = rr.OracleApi(orc), np.random.default_rng(rr.SEED + 2)
    for _ in range(N_FUZZ):
        n = int(rng.integers(0, 3000)) if rng.random() < 0.8 else int(rng.integers(60000, 140000))
        msg = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        cuts = _cuts(rng, n)
        big = rng.random() < 0.3
        for api_pair in ("md5", "sha1"):
            ctxs = [getattr(a, api_pair + "_new")() for a in (ref, o)]
            for a, c in zip((ref, o), ctxs):
                getattr(a, api_pair + "_init")(c)
            for lo, hi in zip(cuts, cuts[1:]):
                if api_pair == "md5":
                    for a, c in zip((ref, o), ctxs):
                        (a.md5_update_big if big else a.md5_update)(c, msg[lo:hi])
                else:
                    after = [a.sha1_update(c, msg[lo:hi]) for a, c in zip((ref, o), ctxs)]
                    assert after[0] == after[1], (n, cuts, "caller's buffer")
                assert ctxs[0].raw == ctxs[1].raw, (api_pair, n, cuts, lo, hi)
            if api_pair == "md5":
                ref.md5_final(ctxs[0])
                o.md5_final(ctxs[1])
            else:
                assert ref.sha1_final(ctxs[0]) == o.sha1_final(ctxs[1]), (n, cuts)
            assert ctxs[0].raw == ctxs[1].raw, (api_pair, n, cuts, "final")


def test_differential_rc4(ref, orc):
    o, rng = rr.OracleApi(orc), np.random.default_rng(rr.SEED + 3)
    for k in range(N_FUZZ):
        key = rng.integers(0, 256, int(rng.integers(1, 301)), dtype=np.uint8).tobytes()
        st = ref.rc4_init(key)
        assert st == o.rc4_init(key), key.hex()
        if k % 3 == 0:                                   # any 264 bytes: no permutation, any indices, any flags
            alphabet = rng.integers(0, 256, int(rng.integers(1, 9)), dtype=np.uint8)
            st = alphabet[rng.integers(0, len(alphabet), 264)].tobytes()
        for _ in range(3):                               # chained calls carry the state
            data = rng.integers(0, 256, int(rng.integers(0, 600)), dtype=np.uint8).tobytes()
            a, b = ref.rc4_crypt(st, data), o.rc4_crypt(st, data)
            assert a == b, (key.hex(), len(data))
            st = a[0]


def test_differential_base64(ref, orc):
    o, rng = rr.OracleApi(orc), np.random.default_rng(rr.SEED + 4)
    code = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/", np.uint8)
    for k in range(N_FUZZ):
        d = rng.integers(0, 256, int(rng.integers(0, 400)), dtype=np.uint8).tobytes()
        t = ref.b64_encode(d)
        assert t == o.b64_encode(d), d.hex()
        text = np.frombuffer(t, np.uint8).copy() if k % 2 else code[rng.integers(0, 64, int(rng.integers(0, 300)))].copy()
        for _ in range(int(rng.integers(0, 6))):         # junk anywhere: '=', NUL, bytes outside the alphabet
            if text.size:
                text[int(rng.integers(0, text.size))] = rng.choice(np.array([0x3D, 0, 0x0A, 0x2D, 0x5F, 0x80, 0xFF, 0x20], np.uint8))
        assert ref.b64_decode(text.tobytes()) == o.b64_decode(text.tobytes()), text.tobytes().hex()


def test_differential_membuf(ref, orc):
    o, rng = rr.OracleApi(orc), np.random.default_rng(rr.SEED + 5)
    for k in range(N_FUZZ):
        size, off = int(rng.integers(0, 3000)), int(rng.integers(0, 41))
        seed = int(rng.integers(0, 1 << 32))
        img = np.zeros(off + (((size + off) // 8 + 4) // 2) * 16 + 16, np.uint8)
        img[:size] = rng.integers(0, 256, size, dtype=np.uint8)
        if k % 5 == 0 and size >= 16:                    # a zero word in the plaintext changes nothing on encrypt
            img[:size - size % 8].view(np.uint64)[int(rng.integers(0, size // 8))] = 0
        enc = ref.membuf(img.tobytes(), size, seed, off, False)
        assert enc == o.membuf(img.tobytes(), size, seed, off, False), (size, off, seed)
        e = np.frombuffer(enc[0], np.uint8).copy()
        if k % 3 == 0 and enc[1] - off >= 16:            # a zero word in the ciphertext stops the decrypt
            e[off:off + (enc[1] - off) // 8 * 8].view(np.uint64)[int(rng.integers(0, (enc[1] - off) // 8))] = 0
        assert ref.membuf(e.tobytes(), enc[1], seed, off, True) == o.membuf(e.tobytes(), enc[1], seed, off, True), (size, off, seed)


def test_differential_metadata(ref, orc):
    from test_metadata_pack import random_items
    o, rng = rr.OracleApi(orc), np.random.default_rng(rr.SEED + 6)
    row = lambda r: None if r is None else [r["rc"]] + r["info"] + [r["count"]]      # noqa: E731
    undefined = 0
    for k in range(N_FUZZ):
        items = random_items(rng, 6, 300)
        pack = ref.md_pack(items)
        assert pack == o.md_pack(items), k
        for _ in range(4):
            p = bytearray(pack)
            how = int(rng.integers(0, 5))
            if how == 0:
                p[int(rng.integers(0, len(p)))] ^= 1 << int(rng.integers(0, 8))
            elif how == 1:
                p = p[:int(rng.integers(0, len(p) + 1))]
            elif how == 2 and items:                     # the first item's size field: any small value, or all ones
                p[64 + 16:64 + 24] = (int(rng.integers(0, 700)) if rng.random() < 0.8 else (1 << 64) - 1).to_bytes(8, "little")
            elif how == 3:
                p[4:8] = int(rng.integers(-2, 9)).to_bytes(4, "little", signed=True)           # item_count
            want = ref.md_unpack(bytes(p))
            if want is None:
                undefined += 1
                continue
            assert row(o.md_unpack(bytes(p))) == row(want), (k, how, bytes(p).hex()[:200])
    assert undefined < N_FUZZ // 2
