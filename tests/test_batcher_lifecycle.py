"""The transform batcher's life cycle against the host model of batcher_model.py, in every mode.

One schedule per family -- 150 connections, 8 rounds of ragged traffic with Enable, EnableAlgo, EnableBatch,
EnableBatchAlgo, Disable and GetState between a FlushAsync and its round's delivery, every documented refusal,
empty rounds -- is replayed call by call into a real batcher: every return code, every callback list and every
GetState equals the model's, bit for bit.  The model's bytes are the oracle's scalar calls chained on the host;
test_batcher_model_cpu.py checks the schedules and the model themselves.  Nothing on the device fails here and
no fault is injected."""
import importlib.util
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _sibling(name, file=None):
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, (file or name) + ".py"))
        sys.modules[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[name])
    return sys.modules[name]


BM = _sibling("batcher_model")


@pytest.fixture(scope="module")
def torch_dev(brb):
    import torch
    assert torch.cuda.is_available(), "no HIP device visible to torch"
    assert brb.gpu_available(), brb.lib().BRB_CryptoGPU_LastError()
    return torch


def _same_results(got, want, in_order, where):
    """Callback lists: equal as they are (one device), or per connection and direction (delivery part by part)."""
    if in_order:
        if got != want:
            at = next((k for k, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
            g, w = (got[at:at + 1] or ["nothing"])[0], (want[at:at + 1] or ["nothing"])[0]
            raise AssertionError(f"{where}: {len(got)} results for {len(want)}, first difference at {at}: got "
                                 f"{_short(g)}, want {_short(w)}")
        return
    g, w = BM.by_conn(got), BM.by_conn(want)
    if g != w:
        key = next(k for k in sorted(set(g) | set(w)) if g.get(k) != w.get(k))
        raise AssertionError(f"{where}: connection {key[0]} op {key[1]}: got {[_short(x) for x in g.get(key, [])]}, want "
                             f"{[_short(x) for x in w.get(key, [])]}")


def _short(res):
    if isinstance(res, str):
        return res
    *head, out, valid = res
    return (*head, len(out), out[:16].hex(), valid)


def replay(brb, calls, max_conns, max_round_bytes, algo, parts=1, **flags):
    """Drives a brb.TransformBatcher with the calls of a model's trace; each return code, each callback list
    and each state must be the model's.  The life-cycle calls go to the library itself, for their return
    codes; Read, Write and the flushes go through the wrapper (in zero-copy mode: its registered regions)."""
    L = brb.lib()
    keys = lambda ks: brb.pack_keys(list(ks))
    with brb.TestOption("devices", parts if parts > 1 else 0):
        b = brb.TransformBatcher(max_conns, max_round_bytes, algo, all_devices=parts > 1, **flags)
        try:
            for i, (name, args, want) in enumerate(calls):
                where = f"call {i} {name}{tuple(a if isinstance(a, int) else '..' for a in args)}"
                if name == "read":
                    got = b.read(*args)
                elif name == "write":
                    got = b.write(*args)
                elif name in ("flush", "flush_async"):
                    _same_results(getattr(b, name)(), want, parts == 1, where)
                    continue
                elif name == "get_state":
                    got = b.state(*args)
                elif name == "enable":
                    got = L.BRB_TransformBatcherEnable(b.h, args[0], args[1], len(args[1]))
                elif name == "enable_algo":
                    got = L.BRB_TransformBatcherEnableAlgo(b.h, args[0], args[1], args[2], len(args[2]))
                elif name == "disable":
                    got = L.BRB_TransformBatcherDisable(b.h, args[0])
                elif name == "enable_batch":
                    ids, (blob, offs, lens) = np.array(args[0], np.uint32), keys(args[1])
                    got = L.BRB_TransformBatcherEnableBatch(b.h, ids.ctypes.data, len(ids), blob.ctypes.data, offs.ctypes.data,
                                                            lens.ctypes.data)
                else:
                    assert name == "enable_batch_algo", name
                    ids, al, (blob, offs, lens) = np.array(args[0], np.uint32), np.array(args[1], np.uint8), keys(args[2])
                    got = L.BRB_TransformBatcherEnableBatchAlgo(b.h, ids.ctypes.data, len(ids), al.ctypes.data, blob.ctypes.data,
                                                                offs.ctypes.data, lens.ctypes.data)
                if got != want:
                    shown = (got.hex()[:48], want.hex()[:48]) if isinstance(got, bytes) else (got, want)
                    raise AssertionError(f"{where}: got {shown[0]}, want {shown[1]} ({L.BRB_CryptoGPU_LastError().decode()})")
        finally:
            b.close()


def _flags(layout, copy, pipe):
    return dict(conn_lists=layout == "conn_lists", mixed=layout == "mixed", zero_copy=copy == "zero_copy",
                pipelined=pipe == "pipelined")


def _timed(label, fn):
    t0 = time.perf_counter()
    fn()
    print(f"\n{label}: {time.perf_counter() - t0:.2f} s")


MODES = [(copy, pipe, parts) for copy in ("copy", "zero_copy") for pipe in ("flush", "pipelined") for parts in (1, 3)]
MAIN = [(f, layout, *mode) for f in ("rc4", "rc4_md5") for layout in ("plain", "conn_lists") for mode in MODES] + \
    [("mixed", "mixed", *mode) for mode in MODES] + \
    [("rc4_md5", "mixed", "zero_copy", "pipelined", parts) for parts in (1, 3)]      # every connection on the default algo


@pytest.mark.parametrize("family,layout,copy,pipe,parts", MAIN, ids=["-".join(map(str, c[:4])) + f"-parts{c[4]}" for c in MAIN])
def test_life_cycle(brb, orc, torch_dev, family, layout, copy, pipe, parts):
    """The family's schedule (batcher_model.schedule) on a batcher of 320 connections, 150 of them in use, so a
    round is several waves of streams in each layout; 4 MiB rounds, which the traffic never fills."""
    calls, _, _ = BM.case(orc, "main", family, pipe == "pipelined", parts, mixed=layout == "mixed")
    _timed("replay", lambda: replay(brb, calls, BM.MAIN_MAX_CONNS, BM.MAIN_ROUND_BYTES, BM.family_algo(family), parts,
                                   **_flags(layout, copy, pipe)))


FULL = [(f, layout, copy, pipe) for f in ("rc4", "rc4_md5") for layout in ("plain", "conn_lists", "mixed")
        for copy in ("copy", "zero_copy") for pipe in ("flush", "pipelined")]


@pytest.mark.parametrize("family,layout,copy,pipe", FULL, ids=["-".join(c) for c in FULL])
def test_full_rounds(brb, orc, torch_dev, family, layout, copy, pipe):
    """batcher_model.full_schedule on a batcher of 3 connections and 4096 bytes: a round takes exactly 12
    buffers and exactly 4096 input bytes (an RC4_MD5 write's 30 bytes more of output still fit), a refused
    buffer goes through after the flush, and an empty buffer is taken while slots remain."""
    calls, _, _ = BM.case(orc, "full", family, pipe == "pipelined", mixed=layout == "mixed")
    replay(brb, calls, BM.FULL_MAX_CONNS, BM.FULL_ROUND_BYTES, BM.family_algo(family), **_flags(layout, copy, pipe))
