"""Host-mode staging of the multi-range batch calls (batch_api.hip: span_rebase, Staging): a call
copies only the byte span [lo, hi) its non-empty items cover, with the offsets rebased to it, and an
empty item gets offset 0 whatever offset the caller gave it.

Each case: 6 items in a 4 KiB host buffer.  The three non-empty items lie in [1024, 3072) -- the
first starts at 1024, the last ends at 3072, so lo > 0 -- and the three empty ones carry an offset
below lo, one inside the span and one above hi (all inside the caller's buffer).  Results equal the
oracle, an empty item writes nothing, and every byte of the caller's buffers outside the items is
unchanged."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZE, LO, HI = 4096, 1024, 3072
EMPTY_OFFS = (100, 2000, 3500)            # below lo, inside the span, above hi
LENGTHS = [(1, 64, 300), (55, 65, 300)]   # the non-empty items of a case


@pytest.fixture(scope="module", autouse=True)
def gpu(brb):
    assert brb.gpu_available(), brb.lib().BRB_CryptoGPU_LastError()


def _pattern(seed, size=SIZE):
    return np.random.default_rng(seed).integers(0, 256, size, dtype=np.uint8)


def _place(lens):
    """Offsets of three non-empty ranges of `lens` bytes in [LO, HI): the first at LO, the second
    at an odd address after it, the last ending at HI."""
    a, b, c = lens
    return LO, LO + a + 401, HI - c


def _items(lens, place=None):
    """(offsets, lengths) in the order: empty below lo, A, empty inside, B, C, empty above hi."""
    oa, ob, oc = _place(place or lens)
    offs = np.array([EMPTY_OFFS[0], oa, EMPTY_OFFS[1], ob, oc, EMPTY_OFFS[2]], np.uint64)
    return offs, np.array([0, lens[0], 0, lens[1], lens[2], 0], np.uint32)


def _ranges(offs, lens):
    return [(int(o), int(o) + int(n)) for o, n in zip(offs, lens)]


def _assert_outside_unchanged(got, before, ranges, what):
    keep = np.ones(before.size, bool)
    for a, b in ranges:
        keep[a:b] = False
    assert np.array_equal(got[keep], before[keep]), f"{what}: bytes outside the items changed"


@pytest.mark.parametrize("lens3", LENGTHS)
@pytest.mark.parametrize("algo", ["md5", "sha1"])
def test_digests(brb, orc, algo, lens3):
    data = _pattern(1)
    offs, lens = _items(lens3)
    before = data.copy()
    got = getattr(brb, algo + "_batch")(data, offs, lens)
    want = getattr(orc, algo + "_batch")(before, offs, lens)
    assert np.array_equal(got, want)
    empty = getattr(orc, algo)(b"")
    for i in (0, 2, 5):
        assert got[i].tobytes() == empty
    assert np.array_equal(data, before)


@pytest.mark.parametrize("lens3", LENGTHS)
@pytest.mark.parametrize("in_place", [True, False])
def test_rc4_crypt(brb, orc, in_place, lens3):
    data = _pattern(2)
    offs, lens = _items(lens3)
    states = brb.rc4_states([b"host-staging-key-%d" % i for i in range(6)])
    want_states, want = states.copy(), data.copy()
    orc.rc4_crypt_batch(want_states, want, offs, lens)
    before = data.copy()
    if in_place:
        out = brb.rc4_crypt_batch(states, data, offs, lens)
        assert out is data
        assert np.array_equal(data, want)           # the oracle leaves everything outside the streams alone
    else:
        out0 = _pattern(3)
        out = out0.copy()
        brb.rc4_crypt_batch(states, data, offs, lens, out=out)
        assert np.array_equal(data, before)
        for a, b in _ranges(offs, lens):
            assert np.array_equal(out[a:b], want[a:b])
        _assert_outside_unchanged(out, out0, _ranges(offs, lens), "out")
    assert np.array_equal(states, want_states)      # an empty stream's state does not advance
    for i in (0, 2, 5):
        assert np.array_equal(want_states[i], brb.rc4_states([b"host-staging-key-%d" % i])[0])


@pytest.mark.parametrize("lens3", LENGTHS)
def test_base64_encode(brb, orc, lens3):
    data = _pattern(4)
    offs, lens = _items(lens3)
    olens = [4 * ((int(n) + 2) // 3) for n in lens]
    ooffs, _ = _items(lens3, place=[olens[1], olens[3], olens[4]])   # the outputs placed the same way
    before, out0 = data.copy(), _pattern(5)
    out = out0.copy()
    brb.base64_encode_batch(data, offs, lens, out, ooffs)
    for o, n, oo in zip(offs, lens, ooffs):
        want = orc.b64_encode(before[int(o):int(o) + int(n)].tobytes())
        assert out[int(oo):int(oo) + len(want)].tobytes() == want
    _assert_outside_unchanged(out, out0, _ranges(ooffs, olens), "out")
    assert np.array_equal(data, before)


@pytest.mark.parametrize("lens3", LENGTHS)
def test_md5_segments(brb, orc, lens3):
    data = _pattern(6)
    offs, lens = _items(lens3)
    # records: one empty segment; no segment; A + empty + B; C + empty
    first = np.array([0, 1, 1, 4, 6], np.uint64)
    before = data.copy()
    got = brb.md5_batch_segments(data, offs, lens, first)
    for i in range(4):
        msg = b"".join(before[int(offs[k]):int(offs[k]) + int(lens[k])].tobytes()
                       for k in range(int(first[i]), int(first[i + 1])))
        assert got[i].tobytes() == orc.md5(msg), f"record {i}"
    assert got[0].tobytes() == got[1].tobytes() == orc.md5(b"")
    assert np.array_equal(data, before)
