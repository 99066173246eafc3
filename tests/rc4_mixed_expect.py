"""Expected values of BRB_RC4_MixedListBatch (test_rc4_mixed_cpu.py, test_rc4_mixed.py): every stream goes to
expect_crypt / expect_frame / expect_open of rc4_lists_expect.py -- the oracle's scalar calls chained on
the host over the stream's buffer list -- by its kind, and the results go where the call puts them.

A helper, not a test module: nothing here is collected by pytest and nothing touches a GPU."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CRYPT, FRAME, OPEN = 0, 1, 2


def _sibling(name):
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
        sys.modules[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[name])
    return sys.modules[name]


E = _sibling("rc4_lists_expect")


def expect_mixed(orc, states, kinds, data, offs, lens, ooffs, first, out, salts=None, valid=None, state_index=None):
    """-> (the whole state table after, a copy of `out` with every buffer's result at ooffs[k], a copy of
    `valid` with the entries of OPEN buffers set; None when valid is None).  Stream i uses row
    state_index[i] (None: i) of `states`.  Every stream is handed to the list helper of its kind as a call of
    its own, over a compact copy of its buffers, so the inputs are read before anything is written (a call
    may work in place) and an empty buffer's offsets are never used."""
    st = np.array(states, np.uint8)
    res = np.array(out, np.uint8)
    val = None if valid is None else np.array(valid, np.uint8)
    first = [int(f) for f in first]
    for i in range(len(first) - 1):
        ks = list(range(first[i], first[i + 1]))
        row = i if state_index is None else int(state_index[i])
        n = [int(lens[k]) for k in ks]
        local = np.concatenate([np.zeros(0, np.uint8)] + [np.asarray(data[int(offs[k]):int(offs[k]) + m], np.uint8)
                                                          for k, m in zip(ks, n) if m])
        llens = np.array(n, np.uint32)
        loffs = (np.cumsum([0] + n)[:-1]).astype(np.uint64)
        lfirst = np.array([0, len(ks)], np.uint64)
        one = st[row:row + 1]
        kd = int(kinds[i])
        grow = 30 if kd == FRAME else 0
        if kd == CRYPT:
            one, got = E.expect_crypt(orc, one, local, loffs, llens, lfirst)
        elif kd == FRAME:
            lfo = (loffs + 30 * np.arange(len(ks), dtype=np.uint64)).astype(np.uint64)
            frames = np.zeros(local.size + 30 * len(ks), np.uint8)
            one, got = E.expect_frame(orc, one, local, loffs, llens, [int(salts[k]) for k in ks], frames, lfo, lfirst)
            loffs = lfo
        elif kd == OPEN:
            one, got, ok = E.expect_open(orc, one, local, loffs, llens, lfirst)
            for j, k in enumerate(ks):
                val[k] = ok[j]
        else:
            raise ValueError(f"stream {i}: kind {kd}")
        for j, k in enumerate(ks):
            m = n[j] + grow
            if m:
                res[int(ooffs[k]):int(ooffs[k]) + m] = got[int(loffs[j]):int(loffs[j]) + m]
        st[row] = one[0]
    return st, res, val
