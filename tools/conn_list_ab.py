"""Buffer lists per connection against consecutive single-buffer calls, on one GPU and in one process.

Shape: 16 384 connections x k buffers of 1500 bytes, k = 1, 2, 4, 8, device mode, device events:

  A  k consecutive calls of the existing batch call at the library's defaults (BRB_RC4_CryptBatch,
     BRB_RC4MD5_FrameBatch, BRB_RC4MD5_OpenBatch: the wave-pair kernels), call r over the buffers of rank r
  B  one list call (BRB_RC4_CryptListBatch, ... ; crypt on both load forms of its kernel, test option
     "rc4_list_coop")

Before anything is timed, A and B run once from equal states and their outputs and states are compared.
Then, after a warm-up, A and B alternate round by round; the median, minimum and maximum over the rounds
are reported.  The transform batcher, zero-copy and pipelined, RC4_MD5 writes, with and without
BRB_BATCHER_CONN_LISTS at k = 2 and 4, and with a ragged write queue (0 .. --ragged-max buffers per
connection, seeded): wall clock of FlushAsync + Flush (submission excluded).

  python tools/conn_list_ab.py [--conns 16384] [--bytes 1500] [--rounds 9] [--warmup 3] [--ragged-max 5] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

import brb_framework_amd as brb

ap = argparse.ArgumentParser()
ap.add_argument("--conns", type=int, default=16384)
ap.add_argument("--bytes", type=int, default=1500)
ap.add_argument("--ks", default="1,2,4,8")
ap.add_argument("--batcher-ks", default="2,4")
ap.add_argument("--ragged-max", type=int, default=5)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

Lb = brb.lib()
if not brb.gpu_available():
    raise RuntimeError("no usable HIP device: " + Lb.BRB_CryptoGPU_LastError().decode())
N, L = args.conns, args.bytes
HDR = 30
rng = np.random.default_rng(0xAB115)
STATES0 = torch.from_numpy(brb.rc4_states([rng.integers(0, 256, 16, dtype=np.uint8).tobytes() for _ in range(N)])).cuda()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stat(us):
    return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0


class Shape:
    """k buffers per connection, connection-major: buffer (i, r) at index i k + r."""

    def __init__(self, k):
        self.k = k
        nb = N * k
        idx = np.arange(nb, dtype=np.uint64)
        self.offs, self.lens = dev(idx * L), dev(np.full(nb, L, np.uint32))
        self.foffs, self.flens = dev(idx * (L + HDR)), dev(np.full(nb, L + HDR, np.uint32))
        self.first = dev(np.arange(N + 1, dtype=np.uint64) * k)
        self.salts = dev(idx * 977)
        rank = [(np.arange(N, dtype=np.uint64) * k + r) for r in range(k)]
        self.r_offs = [dev(x * L) for x in rank]
        self.r_foffs = [dev(x * (L + HDR)) for x in rank]
        self.r_salts = [dev(x * 977) for x in rank]
        self.r_lens, self.r_flens = dev(np.full(N, L, np.uint32)), dev(np.full(N, L + HDR, np.uint32))
        self.payload = torch.from_numpy(rng.integers(0, 256, nb * L, dtype=np.uint8)).cuda()
        self.frames = torch.zeros(nb * (L + HDR), dtype=torch.uint8, device="cuda")

    def legs(self, op, st, buf, valid):
        """(A, B) closures of `op` on states st and the in/out buffer buf."""
        kw = dict(async_=True)
        if op == "crypt":
            a = lambda: [brb.rc4_crypt_batch(st, buf, self.r_offs[r], self.r_lens, **kw) for r in range(self.k)]
            b = lambda: brb.rc4_crypt_list_batch(st, buf, self.offs, self.lens, self.first, **kw)
        elif op == "frame":
            a = lambda: [brb.rc4md5_frame_batch(st, self.payload, self.r_offs[r], self.r_lens, self.r_salts[r], buf,
                                                self.r_foffs[r], **kw) for r in range(self.k)]
            b = lambda: brb.rc4md5_frame_list_batch(st, self.payload, self.offs, self.lens, self.salts, buf, self.foffs,
                                                    self.first, **kw)
        else:
            a = lambda: [brb.rc4md5_open_batch(st, buf, self.r_foffs[r], self.r_flens, valid=valid[r], **kw)
                         for r in range(self.k)]
            b = lambda: brb.rc4md5_open_list_batch(st, buf, self.foffs, self.flens, self.first, valid=valid[self.k], **kw)
        return a, b


def run_op(sh, op, coop):
    k = sh.k
    valid = [torch.zeros(N, dtype=torch.uint8, device="cuda") for _ in range(k)] + \
            [torch.zeros(N * k, dtype=torch.uint8, device="cuda")]
    src = sh.payload if op == "crypt" else sh.frames
    # outputs equal between A and B, from equal states (open: the frames the frame leg wrote)
    res = []
    with brb.TestOption("rc4_list_coop", coop):
        for leg in (0, 1):
            st, buf = STATES0.clone(), src.clone()
            sh.legs(op, st, buf, valid)[leg]()
            torch.cuda.synchronize()
            brb.async_fault_check()
            res.append((st, buf))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), (op, k, "A and B differ")
        if op == "open":
            va = torch.stack(valid[:k], dim=1).reshape(-1)
            assert torch.equal(va, valid[k]) and bool(va.all()), (op, k, "valid flags differ")
        if op == "frame":
            sh.frames.copy_(res[1][1])         # what the open legs read
        st, buf = STATES0.clone(), src.clone()
        a, b = sh.legs(op, st, buf, valid)
        for _ in range(args.warmup):
            a()
            b()
        ta, tb = [], []
        for _ in range(args.rounds):
            ta.append(timed(a))
            tb.append(timed(b))
        torch.cuda.synchronize()
        brb.async_fault_check()
    return stat(ta), stat(tb)


def run_batcher(k, rounds, counts=None):
    """RC4_MD5 writes, k per connection (counts: connection c submits counts[c] <= k of them), zero-copy and
    pipelined: wall clock of FlushAsync + Flush."""
    if counts is None:
        counts = np.full(N, k)
    total = int(counts.sum())
    nbytes = N * k * L
    region = brb.crypto.HostRegion(nbytes)
    ctypes.memmove(region.addr, rng.integers(0, 256, nbytes, dtype=np.uint8).tobytes(), nbytes)
    out = {}
    hs = {}
    for lists in (False, True):
        algo = brb.CRYPTO_FUNC_RC4_MD5 | brb.BATCHER_ZERO_COPY | brb.BATCHER_PIPELINED | (brb.BATCHER_CONN_LISTS if lists else 0)
        h = Lb.BRB_TransformBatcherCreate(N, nbytes, algo)
        if not h:
            raise RuntimeError(Lb.BRB_CryptoGPU_LastError().decode())
        keys = [b"%016d" % c for c in range(N)]
        blob, offs, lens = brb.pack_keys(keys)
        ids = np.arange(N, dtype=np.uint32)
        assert Lb.BRB_TransformBatcherEnableBatch(h, ids.ctypes.data, N, blob.ctypes.data, offs.ctypes.data, lens.ctypes.data) == 1
        hs[lists] = h
    times = {False: [], True: []}
    for rnd in range(args.warmup + rounds):
        for lists in (False, True):
            h = hs[lists]
            for r in range(k):
                for c in np.nonzero(counts > r)[0].tolist():
                    Lb.BRB_TransformBatcherWrite(h, c, region.addr + (c * k + r) * L, L, c)
            t0 = time.perf_counter()
            n1 = Lb.BRB_TransformBatcherFlushAsync(h, None, None)
            n2 = Lb.BRB_TransformBatcherFlush(h, None, None)
            dt = (time.perf_counter() - t0) * 1e6
            assert n1 == 0 and n2 == total, (n1, n2, Lb.BRB_CryptoGPU_LastError())
            if rnd >= args.warmup:
                times[lists].append(dt)
    for lists in (False, True):
        Lb.BRB_TransformBatcherDestroy(hs[lists])
        out["conn_lists" if lists else "sub_rounds"] = stat(times[lists])
    region.close()
    return out


result = {"shape": {"connections": N, "buffer_bytes": L}, "rounds": args.rounds, "warmup": args.warmup,
          "device": torch.cuda.get_device_name(0), "calls": {}, "batcher_zero_copy_pipelined_rc4md5_writes": {}}
for k in [int(x) for x in args.ks.split(",") if x]:
    sh = Shape(k)
    row = {}
    for op in ("crypt", "frame", "open"):
        a, b = run_op(sh, op, 0)
        row[op] = {"A_k_calls": a, "B_list_call": b}
        if op == "crypt":
            _, bc = run_op(sh, op, 1)
            row[op]["B_list_call_coop_loads"] = bc
        print(f"k={k} {op}: A {a}  B {b}" + (f"  B(coop) {row[op]['B_list_call_coop_loads']}" if op == "crypt" else ""),
              flush=True)
    result["calls"][str(k)] = row
    del sh
    torch.cuda.empty_cache()
for k in [int(x) for x in args.batcher_ks.split(",") if x]:
    result["batcher_zero_copy_pipelined_rc4md5_writes"][str(k)] = run_batcher(k, max(3, args.rounds // 2))
    print(f"batcher k={k}: {result['batcher_zero_copy_pipelined_rc4md5_writes'][str(k)]}", flush=True)
if args.ragged_max > 0:
    counts = np.random.default_rng(0x4A66).integers(0, args.ragged_max + 1, N)
    r = run_batcher(args.ragged_max, max(3, args.rounds // 2), counts)
    r["buffers"] = int(counts.sum())
    result["batcher_zero_copy_pipelined_rc4md5_writes"][f"ragged_0_{args.ragged_max}"] = r
    print(f"batcher ragged 0..{args.ragged_max}: {r}", flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
print(json.dumps(result))
