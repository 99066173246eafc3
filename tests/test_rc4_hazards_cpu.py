"""The RC4 read-ahead hazards on the CPU (no GPU needed): tests/rc4_model.py against the C oracle and the
compat BRB_RC4_Crypt / BRB_RC4_Init on the directed input classes, the restatement of brb_rc4::Gen
against plain RC4, and the conditions that make those inputs worth running on the card: enough
patch coincidences, and every broken generator visibly wrong.  The floors below are asserted from the
model alone; if a new seed misses them, change the seed (rc4_model.SEED), not the floors.

Model counts with the committed seed 0x52433448 (each printed by its test):
  class A  65 536 streams, 294 912 bytes: patch T 936, T-1 678, T-2 441, double 3, triple 0, i == j 1 152,
           S[i] == 0 1 166; streams differing per mutant: no_t2 436, no_t1 674, no_t 930, reversed 6,
           t2_takes_t1 626
  class B  2 048 streams, 139 776 bytes: patch T 4 992, T-1 3 370, T-2 2 875, double 1 098, triple 74,
           i == j 3 091, S[i] == 0 22 554; mutants: no_t2 818, no_t1 874, no_t 1 037, reversed 659,
           t2_takes_t1 867
"""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest


def _model():
    if "rc4_model" not in sys.modules:
        spec = importlib.util.spec_from_file_location(
            "rc4_model", os.path.join(os.path.dirname(os.path.abspath(__file__)), "rc4_model.py"))
        sys.modules["rc4_model"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules["rc4_model"])
    return sys.modules["rc4_model"]


M = _model()


@pytest.fixture(scope="module")
def cls():
    """Per class: states, lens and the plain model's Result, computed once."""
    out = {}
    for name in "abd":
        st, lens = getattr(M, "class_" + name)()
        out[name] = (st, lens, M.plain(st, lens))
    return out


@pytest.fixture(scope="module")
def gen_ok(cls):
    return {name: M.gen(cls[name][0], cls[name][1]) for name in "ab"}


def _buffers(name, lens):
    offs, lens, total = M.layout(lens, 17 + ord(name))
    return offs, lens, M.fill(offs, lens, total, 23 + ord(name), 0xA5)


def test_input_classes_are_what_they_claim(cls):
    a, la, _ = cls["a"]
    assert a.shape == (65536, 264) and np.array_equal(a[:, 256].astype(int) * 256 + a[:, 257], np.arange(65536))
    assert (np.sort(a[:, :256], axis=1) == np.arange(256)).all() and (a[:, 258:] == 0).all()
    assert np.array_equal(la, 1 + (a[:, 256].astype(int) + a[:, 257]) % 8)
    assert len({r.tobytes() for r in a[:64, :256]}) == 64                      # a fresh permutation each
    b, lb, _ = cls["b"]
    d = (b[:, 257].astype(int) - b[:, 256]) & 255
    assert b.shape == (2048, 264) and len({(int(x), int(y)) for x, y in zip(b[:, 256], d)}) == 2048 and d.max() == 7
    assert set(np.unique(b[:, :256]).tolist()) == set(M.LOW_BYTES)
    assert int(lb.sum()) == 139776 and all({int(x) for x in lb[d == k]} == set(M.B_LENS) for k in range(8))
    dd, ld, _ = cls["d"]
    assert np.array_equal(dd[:, :258], b[:, :258]) and (dd[:, 258:] != 0).all() and np.array_equal(ld, lb)
    c, lc = M.class_c()
    assert c.shape == (512, 264) and lc.shape == (40, 512) and set(np.unique(lc).tolist()) == {0, 1, 2, 3}
    for name in "abd":                                                          # seeded: the same bytes every time
        assert np.array_equal(getattr(M, "class_" + name)()[0], cls[name][0])


@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_oracle_equals_plain_model(orc, cls, name):
    """orc.rc4_crypt (through its batch loop) on arbitrary, non-permutation states and start indices:
    output, all 264 state bytes, padding untouched, bytes between streams untouched."""
    st, lens, p = cls[name]
    offs, lens, data = _buffers(name, lens)
    assert {int(o) & 3 for o in offs} == {0, 1, 2, 3}
    got_st, got = st.copy(), data.copy()
    orc.rc4_crypt_batch(got_st, got, offs, lens)
    assert np.array_equal(got, M.apply_ks(data, p.ks, offs, lens))
    assert np.array_equal(got_st, p.states)
    assert np.array_equal(got_st[:, 258:], st[:, 258:])
    s1, o1 = orc.rc4_crypt(st[5].tobytes(), data[int(offs[5]):int(offs[5]) + int(lens[5])].tobytes())
    assert s1 == p.states[5].tobytes() and o1 == got[int(offs[5]):int(offs[5]) + int(lens[5])].tobytes()


@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_compat_crypt_equals_plain_model(brb, cls, name):
    """The product library's BRB_RC4_Crypt, one call per stream, in place on the state table."""
    st, lens, p = cls[name]
    offs, lens, data = _buffers(name, lens)
    got_st, got = st.copy(), data.copy()
    fn = brb.lib().BRB_RC4_Crypt
    sp, dp = got_st.ctypes.data, got.ctypes.data
    ptr = ctypes.POINTER(brb.BRB_RC4_State)
    for k, (o, n) in enumerate(zip(offs.tolist(), lens.tolist())):
        fn(ctypes.cast(sp + 264 * k, ptr), dp + o, dp + o, n)
    assert np.array_equal(got, M.apply_ks(data, p.ks, offs, lens))
    assert np.array_equal(got_st, p.states)
    assert np.array_equal(got_st[:, 258:], st[:, 258:])


@pytest.mark.parametrize("name", ["a", "b"])
def test_gen_restatement_equals_plain(cls, gen_ok, name):
    p, g = cls[name][2], gen_ok[name]
    assert np.array_equal(g.ks, p.ks) and np.array_equal(g.states, p.states)


def test_gen_restatement_in_tiny_chained_calls(cls):
    """Class C on the model: store() and load() around almost every byte equal one plain run."""
    st, call_lens = M.class_c()
    want = M.plain(st, call_lens.sum(axis=0))
    cur, cols = st, np.zeros(len(st), np.int64)
    for lens in call_lens:
        g = M.gen(cur, lens)
        k, t, _ = M.flat_index(np.zeros(len(st), np.int64), lens)
        assert np.array_equal(g.ks[k, t], want.ks[k, cols[k] + t])
        cur, cols = g.states, cols + lens
    assert np.array_equal(cur, want.states)


def test_class_b_hazard_floors(cls):
    c = cls["b"][2].counts
    print("class B model counts:", c)
    assert c["bytes"] == 139776
    assert c["double"] >= 500 and c["triple"] >= 40
    assert min(c["t"], c["t1"], c["t2"]) >= 1500
    assert c["self_swap"] > 0 and c["a_zero"] > 0 and c["startup"] > 0


def test_class_a_counts(cls):
    c = cls["a"][2].counts
    print("class A model counts:", c)
    assert c["bytes"] == 294912 and min(c["t"], c["t1"], c["t2"], c["self_swap"], c["a_zero"], c["startup"]) > 0


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_mutants_are_caught_on_class_b(cls, mutant):
    st, lens, p = cls["b"]
    bad = M.differing(p, M.gen(st, lens, mutant))
    print(f"class B: mutant {mutant} differs on {bad} of {len(st)} streams")
    assert bad >= len(st) // 4


@pytest.mark.parametrize("mutant", M.DROP_MUTANTS)
def test_drop_mutants_are_caught_on_class_a(cls, mutant):
    st, lens, p = cls["a"]
    bad = M.differing(p, M.gen(st, lens, mutant))
    print(f"class A: mutant {mutant} differs on {bad} of {len(st)} streams")
    assert bad >= 200


# ---- key setup -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,key", M.forced_keys(), ids=[n for n, _ in M.forced_keys()])
def test_forced_keys(brb, orc, name, key):
    """The forced pattern is there (256 steps with j where it was put; the carried value rides through
    255 of them for pattern a, the wrap at i = 255 carrying into no next step), the oracle and the
    compat BRB_RC4_Init equal the model, and the one-patch restatement of the sweep equals it with
    its patch and, where the patch is hit, differs without."""
    state, c = M.ksa(key)
    print(name, len(key), c)
    want = {"a": dict(next=256, self=0, next2=0, carried=255), "b": dict(next=0, self=256, next2=0, carried=0),
            "c": dict(next=0, self=0, next2=256, carried=0), "d": dict(next=128, self=0, next2=128, carried=128)}
    assert c == want[name[0]] and len(key) == int(name[1:])
    assert sorted(state[:256]) == list(range(256))
    assert orc.rc4_init(key) == state
    assert brb.rc4_state_bytes(brb.rc4_init(key)) == state
    assert M.ksa_carried(key) == state
    assert (M.ksa_carried(key, patch=False) != state) == (name[0] in "ad")
    if len(key) > 256:
        assert M.ksa(key[:256])[0] == state                 # the bytes past 256 are never read


def test_forced_key_blob_offsets_are_odd():
    keys = [k for _, k in M.forced_keys()]
    blob, offs, lens = M.odd_blob(keys)
    assert {int(o) & 3 for o in offs} == {1, 3}
    assert [blob[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs, lens)] == keys
