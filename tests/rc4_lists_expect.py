"""Expected values of the RC4 list calls (test_rc4_lists_cpu.py, test_rc4_lists.py): the oracle's scalar
calls chained on the host over each stream's buffer list.

A helper, not a test module: nothing here is collected by pytest and nothing touches a GPU."""
import numpy as np


def _lists(first):
    first = [int(f) for f in first]
    return [range(first[i], first[i + 1]) for i in range(len(first) - 1)]


def expect_crypt(orc, states, data, offs, lens, first, out=None):
    """orc.rc4_crypt per buffer in list order -> (states after, out).  out=None: in place (a copy of
    data); else a copy of `out` with the buffers' bytes replaced."""
    st = np.array(states, np.uint8)
    res = np.array(data if out is None else out, np.uint8)
    for i, ks in enumerate(_lists(first)):
        s = st[i].tobytes()
        for k in ks:
            o, n = int(offs[k]), int(lens[k])
            s, ob = orc.rc4_crypt(s, data[o:o + n].tobytes() if n else b"")
            if n:
                res[o:o + n] = np.frombuffer(ob, np.uint8)
        st[i] = np.frombuffer(s, np.uint8)
    return st, res


def expect_frame(orc, states, payload, offs, lens, salts, frames, foffs, first):
    """orc.rc4md5_frame per buffer in list order -> (states after, a copy of `frames` with the frames)."""
    st = np.array(states, np.uint8)
    res = np.array(frames, np.uint8)
    for i, ks in enumerate(_lists(first)):
        s = st[i].tobytes()
        for k in ks:
            o, n, f = int(offs[k]), int(lens[k]), int(foffs[k])
            s, fr = orc.rc4md5_frame(s, payload[o:o + n].tobytes() if n else b"", int(salts[k]))
            res[f:f + 30 + n] = np.frombuffer(fr, np.uint8)
        st[i] = np.frombuffer(s, np.uint8)
    return st, res


def expect_open(orc, states, frames, offs, lens, first, out=None):
    """orc.rc4md5_open per buffer in list order -> (states after, out, valid uint8 per buffer)."""
    st = np.array(states, np.uint8)
    res = np.array(frames if out is None else out, np.uint8)
    valid = np.zeros(len(offs), np.uint8)
    for i, ks in enumerate(_lists(first)):
        s = st[i].tobytes()
        for k in ks:
            o, n = int(offs[k]), int(lens[k])
            s, dec, ok = orc.rc4md5_open(s, frames[o:o + n].tobytes() if n else b"")
            if n:
                res[o:o + n] = np.frombuffer(dec, np.uint8)
            valid[k] = ok
        st[i] = np.frombuffer(s, np.uint8)
    return st, res, valid
