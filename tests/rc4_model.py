"""Python models of RC4 for the read-ahead hazard tests (test_rc4_hazards_cpu.py, test_rc4_hazards.py).

A helper, not a test module: nothing here is collected by pytest and nothing touches a GPU.

* ``plain``    -- textbook RC4 (BRB_RC4_Crypt, rc4.c:64-87) over arbitrary 264-byte states, not
                  necessarily permutations, vectorised over streams, with counters of the events that
                  matter to a generator that reads S[i] ahead of its use.
* ``gen``      -- a restatement of brb_rc4::Gen (csrc/gpu/rc4_device.h): load(), step(), store(),
                  with the same registers, the same order of LDS reads and writes and the same three
                  ordered patches.  ``mutant`` breaks the patches in one of five ways; with
                  ``mutant=None`` it must equal ``plain`` on every input.
* ``ksa`` / ``ksa_carried`` / ``forced_key`` -- the key-scheduling sweep (BRB_RC4_Init), the one-patch
                  carried-value form of rc4_keysetup_kernel (csrc/gpu/keysetup_kernels.hip), and keys
                  built so that j lands where the sweep's patch does or just does not fire.
* ``class_a`` .. ``class_d``, ``layout``, ``fill`` -- the seeded input classes and buffers.

Names: byte T of a call uses i_T = index1 + 1 + T and j_T; "swap T" writes S[i_T] and S[j_T].  The
generator reads S[i_{T+1}] before swaps T-2, T-1 and T are written, so the raw value is stale exactly
when j_s == i_{T+1} for one of s = T-2, T-1, T ("patch T-2 / T-1 / T fires"); when several fire the
latest swap wins, which is why the patches are ordered.
"""
from collections import namedtuple

import numpy as np

STATE_BYTES = 264
SEED = 0x52433448                      # the committed seed of every input class ("RC4H")
MUTANTS = ("no_t2", "no_t1", "no_t", "reversed", "t2_takes_t1")
DROP_MUTANTS = MUTANTS[:3]
LOW_BYTES = (0, 1, 2, 3, 254, 255)     # class B's alphabet: j moves by -2 .. 3 per byte, i by 1
B_LENS = (16, 63, 64, 65, 130, 200, 7, 1)
COUNTERS = ("bytes", "t", "t1", "t2", "double", "triple", "self_swap", "a_zero", "startup")

Result = namedtuple("Result", "ks states counts")


def _rows(states):
    states = np.ascontiguousarray(states, np.uint8)
    assert states.ndim == 2 and states.shape[1] == STATE_BYTES
    return states


def plain(states, lens):
    """Textbook RC4.  states (n, 264) uint8 (not modified), lens (n,) -> Result: ks (n, max len) uint8
    keystream (zero past a stream's length), the states after (bytes 258..263 as they were) and the
    event counters over the bytes produced:

    bytes      keystream bytes in all
    t, t1, t2  byte u (u >= 1 / 2 / 3 of its call) with j_{u-1} / j_{u-2} / j_{u-3} == i_u
    double     bytes with at least two of those three, triple: all three
    self_swap  i == j
    a_zero     S[i] == 0 before the swap (j does not move)
    startup    bytes u <= 2 whose i_u equals the index2 the call started from (the "identity swaps"
               that stand in for swaps -1 and -2 compare equal; they must patch nothing wrongly)
    """
    states = _rows(states)
    lens = np.asarray(lens, np.int64)
    n, L = len(states), int(lens.max()) if len(lens) else 0
    S = states[:, :256].astype(np.int64)
    i, j = states[:, 256].astype(np.int64), states[:, 257].astype(np.int64)
    cj0 = j.copy()
    ks = np.zeros((n, L), np.uint8)
    c = dict.fromkeys(COUNTERS, 0)
    j0, j1, j2 = (np.full(n, -1, np.int64) for _ in range(3))      # j of swaps u-1, u-2, u-3
    for u in range(L):
        r = np.nonzero(lens > u)[0]
        ii = (i[r] + 1) & 255
        f0, f1, f2 = j0[r] == ii, j1[r] == ii, j2[r] == ii
        k = f0.astype(np.int64) + f1 + f2
        a = S[r, ii]
        jj = (j[r] + a) & 255
        b = S[r, jj]
        S[r, ii] = b
        S[r, jj] = a
        ks[r, u] = S[r, (a + b) & 255]
        c["bytes"] += r.size
        c["t"] += int(f0.sum())
        c["t1"] += int(f1.sum())
        c["t2"] += int(f2.sum())
        c["double"] += int((k >= 2).sum())
        c["triple"] += int((k == 3).sum())
        c["self_swap"] += int((ii == jj).sum())
        c["a_zero"] += int((a == 0).sum())
        if u <= 2:
            c["startup"] += int((cj0[r] == ii).sum())
        i[r], j[r] = ii, jj
        j2[r], j1[r], j0[r] = j1[r], j0[r], jj
    out = states.copy()
    out[:, :256] = S
    out[:, 256], out[:, 257] = i, j
    return Result(ks, out, c)


def gen(states, lens, mutant=None):
    """brb_rc4::Gen restated: load(), lens[k] calls of step(), store().  Indices stand for the LDS
    addresses (the lane column never differs within a stream).  Returns Result with counts None."""
    assert mutant is None or mutant in MUTANTS
    states = _rows(states)
    lens = np.asarray(lens, np.int64)
    n, L = len(states), int(lens.max()) if len(lens) else 0
    rows = np.arange(n)
    S = states[:, :256].astype(np.int64)
    rd = lambda x: S[rows, x]                                   # noqa: E731
    # ---- load(): identity swaps before byte 0, byte 0 started, S[i] read ahead at i + 1, i + 2
    ci, cj = states[:, 256].astype(np.int64), states[:, 257].astype(np.int64)
    pai, paj = ci.copy(), cj.copy()
    pa = rd(paj)
    qaj, qa = paj.copy(), pa.copy()
    ai = (ci + 1) & 255
    a = rd(ai)
    aj = (cj + a) & 255
    rb = rd(aj)
    ad1 = (ci + 2) & 255
    r1 = rd(ad1)
    ad2 = (ci + 3) & 255
    r2 = rd(ad2)
    ks = np.zeros((n, L), np.uint8)
    for u in range(L):
        m = lens > u
        r = np.nonzero(m)[0]
        # ---- start byte T+1 at ad1: the three ordered patches
        t2v = pa if mutant == "t2_takes_t1" else qa
        patches = [(qaj == ad1, t2v), (paj == ad1, pa), (aj == ad1, a)]
        if mutant in DROP_MUTANTS:
            del patches[DROP_MUTANTS.index(mutant)]
        if mutant == "reversed":
            patches.reverse()
        a1 = r1
        for hit, v in patches:
            a1 = np.where(hit, v, a1)
        aj1 = (aj + a1) & 255
        ad3 = (ad2 + 1) & 255
        r3 = rd(ad3)                       # before swap T is written
        # ---- complete byte T
        b = rb
        S[r, ai[r]] = b[r]
        S[r, aj[r]] = a[r]
        rb1 = rd(aj1)                      # after swap T: exact
        k = rd((a + b) & 255)
        ks[r, u] = k[r]
        # ---- shift the pipeline (streams past their length keep their registers)
        new = dict(qaj=paj, qa=pa, pai=ai, paj=aj, pa=a, a=a1, rb=rb1, ai=ad1, aj=aj1, r1=r2, ad1=ad2, r2=r3, ad2=ad3)
        old = dict(qaj=qaj, qa=qa, pai=pai, paj=paj, pa=pa, a=a, rb=rb, ai=ai, aj=aj, r1=r1, ad1=ad1, r2=r2, ad2=ad2)
        reg = {name: np.where(m, new[name], old[name]) for name in new}
        qaj, qa, pai, paj, pa, a, rb = (reg[x] for x in ("qaj", "qa", "pai", "paj", "pa", "a", "rb"))
        ai, aj, r1, ad1, r2, ad2 = (reg[x] for x in ("ai", "aj", "r1", "ad1", "r2", "ad2"))
    # ---- store(): the started byte is dropped; indices of the last completed byte
    out = states.copy()
    out[:, :256] = S
    out[:, 256], out[:, 257] = pai, paj
    return Result(ks, out, None)


def differing(x, y):
    """Number of streams on which two Results differ (keystream or state)."""
    return int(((x.ks != y.ks).any(axis=1) | (x.states != y.states).any(axis=1)).sum())


# ---- buffers ---------------------------------------------------------------------------------------
def layout(lens, seed, base=0):
    """Stream offsets with seeded gaps of 0..3 bytes before every stream -> (offs uint64, lens uint32,
    total), total including 8 trailing bytes that belong to no stream."""
    lens = np.asarray(lens, np.int64)
    gaps = np.random.default_rng(seed).integers(0, 4, len(lens))
    ends = np.cumsum(lens + gaps)
    offs = base + ends - lens
    return offs.astype(np.uint64), lens.astype(np.uint32), (int(ends[-1]) if len(lens) else 0) + base + 8


def flat_index(offs, lens):
    """(stream, position in stream, position in buffer) of every stream byte, stream by stream."""
    lens = np.asarray(lens, np.int64)
    k = np.repeat(np.arange(len(lens)), lens)
    first = np.cumsum(lens) - lens
    t = np.arange(int(lens.sum())) - first[k]
    return k, t, np.asarray(offs, np.int64)[k] + t


def fill(offs, lens, total, seed, sentinel):
    """A buffer of `total` bytes: seeded random bytes in the streams, `sentinel` everywhere else."""
    buf = np.full(total, sentinel, np.uint8)
    _, _, pos = flat_index(offs, lens)
    buf[pos] = np.random.default_rng(seed).integers(0, 256, pos.size, dtype=np.uint8)
    return buf


def apply_ks(buf, ks, offs, lens):
    """buf with every stream xored with its keystream row; bytes outside the streams as they were."""
    out = buf.copy()
    k, t, pos = flat_index(offs, lens)
    out[pos] ^= ks[k, t]
    return out


def covered(offs, lens, total):
    m = np.zeros(total, bool)
    m[flat_index(offs, lens)[2]] = True
    return m


# ---- input classes -----------------------------------------------------------------------------------
def class_a(seed=SEED):
    """Every (index1, index2): 65 536 states, a fresh random permutation each, 1 + (i1 + i2) % 8 bytes."""
    rng = np.random.default_rng([seed, 0xA])
    k = np.arange(65536)
    st = np.zeros((65536, STATE_BYTES), np.uint8)
    st[:, :256] = rng.permuted(np.tile(np.arange(256, dtype=np.uint8), (65536, 1)), axis=1)
    st[:, 256], st[:, 257] = k >> 8, k & 255
    return st, (1 + ((k >> 8) + (k & 255)) % 8).astype(np.uint32)


def class_b(seed=SEED):
    """Low-entropy near-index states: all 2 048 (index1, d), index2 = index1 + d, d = 0..7, every byte of
    S from LOW_BYTES (no permutation), lengths cycling through B_LENS so that every d meets every
    length (whole 64-byte blocks, tails of 1..3 bytes, one-byte streams)."""
    rng = np.random.default_rng([seed, 0xB])
    k = np.arange(2048)
    i1, d = k >> 3, k & 7
    st = np.zeros((2048, STATE_BYTES), np.uint8)
    st[:, :256] = np.array(LOW_BYTES, np.uint8)[rng.integers(0, len(LOW_BYTES), (2048, 256))]
    st[:, 256], st[:, 257] = i1, (i1 + d) & 255
    return st, np.array(B_LENS, np.uint32)[(i1 + d) % 8]


def class_d(seed=SEED):
    """Class B with the padding and the flags word (bytes 258..263) random and non-zero."""
    st, lens = class_b(seed)
    st[:, 258:] = np.random.default_rng([seed, 0xD]).integers(1, 256, (len(st), 6), dtype=np.uint8)
    return st, lens


def class_c(seed=SEED, n=512, calls=40):
    """Chained tiny calls: n states, half from class A and half from class B, and per call a length of
    0..3 per stream -> (states, call_lens (calls, n) uint32)."""
    rng = np.random.default_rng([seed, 0xC])
    a, b = class_a(seed)[0], class_b(seed)[0]
    st = np.concatenate([a[rng.choice(len(a), n // 2, replace=False)], b[rng.choice(len(b), n - n // 2, replace=False)]])
    return st, rng.integers(0, 4, (calls, n)).astype(np.uint32)


# ---- key setup -----------------------------------------------------------------------------------------
KSA_PATTERNS = {"a": (1,), "b": (0,), "c": (2,), "d": (1, 2)}     # j - i at step i, cycled


def ksa(key):
    """BRB_RC4_Init's sweep over the first min(len, 256) .. bytes cycled by i % len -> (264-byte state
    with zero indices and padding, counts of steps with j == i + 1, j == i, j == i + 2, all mod 256,
    and `carried`: steps i < 255 with j == i + 1, whose old S[i] is the next step's S[i + 1])."""
    key = bytes(key)
    S, j = list(range(256)), 0
    c = {"next": 0, "self": 0, "next2": 0, "carried": 0}
    for i in range(256):
        j = (j + S[i] + key[i % len(key)]) & 255
        S[i], S[j] = S[j], S[i]
        c["next"] += j == (i + 1) & 255
        c["self"] += j == i
        c["next2"] += j == (i + 2) & 255
        c["carried"] += j == i + 1
    return bytes(S) + bytes(8), c


def ksa_carried(key, patch=True):
    """rc4_keysetup_kernel's sweep restated: S[i + 1] is read before swap i is written and carried to
    the next step; `patch` keeps the old S[i] when j == i + 1.  patch=False is the mutant."""
    key = bytes(key)[:256]
    S, j, a = list(range(256)), 0, 0
    kp, kb = 0, key[0]
    for i in range(256):
        j = (j + a + kb) & 255
        kp = 0 if kp + 1 == len(key) else kp + 1
        i1 = (i + 1) & 255
        u, raw = S[j], S[i1]
        kb = key[kp]
        S[i] = u
        S[j] = a
        a = a if (patch and j == i1) else raw
    return bytes(S) + bytes(8)


def forced_key(pattern, extra=0, seed=SEED):
    """A 256-byte key that puts j at i + KSA_PATTERNS[pattern][i % cycle] (mod 256) at every step of the
    sweep, followed by `extra` random bytes that a 256-step sweep never reads."""
    offs = KSA_PATTERNS[pattern]
    S, j, key = list(range(256)), 0, bytearray(256)
    for i in range(256):
        want = (i + offs[i % len(offs)]) & 255
        key[i] = (want - j - S[i]) & 255
        j = want
        S[i], S[j] = S[j], S[i]
    tail = np.random.default_rng([seed, 0xE, extra]).integers(0, 256, extra, dtype=np.uint8).tobytes()
    return bytes(key) + tail


def forced_keys(seed=SEED):
    """The eight forced keys (patterns a..d at 256 and at 300 bytes) -> [(name, key)]."""
    return [(f"{p}{256 + x}", forced_key(p, x, seed)) for x in (0, 44) for p in "abcd"]


def odd_blob(keys, sentinel=0xEE):
    """The keys in one blob at odd byte offsets, alternating between 1 and 3 mod 4 -> (blob, offs, lens)."""
    parts, offs, pos = [], [], 0
    for n, k in enumerate(keys):
        pad = 1
        while (pos + pad) % 4 != (1 if n % 2 == 0 else 3):
            pad += 1
        parts.append(bytes([sentinel]) * pad + bytes(k))
        offs.append(pos + pad)
        pos += pad + len(k)
    blob = np.frombuffer(b"".join(parts) + bytes([sentinel]) * 5, np.uint8).copy()
    return blob, np.array(offs, np.uint64), np.array([len(k) for k in keys], np.uint32)
