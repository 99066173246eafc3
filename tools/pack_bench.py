"""BRB_MetaDataPackBatch at the MetaData bench shape (65 536 packs x 4 items x 375 B, HBM-resident),
beside what a digest-then-copy pack would cost, in one process and interleaved:

  (a)  BRB_MetaDataPackBatch: the items of n source packs packed into an output buffer
  (b)  BRB_MD5BatchSegments over the same item lists with test option seg_line = 0: the same per-lane
       read path (brb_io::BlockSrc + the MD5 funnel) without the writes
  (c)  a device-to-device copy of the output byte count
  (b2) BRB_MD5BatchSegments with the default kernel (line-staged wave pairs): the distance left for a
       line-staged pack kernel; not part of the bound

Expectation: (a) <= (b) + (c), what fusing buys over digest-then-copy.  Timed as the bench legs are:
an untimed settle of the same launches, W warm-up launches, then K launches between two events, on
rotating source buffers larger than the caches; `--rounds` interleaved rounds, the median reported.
The packed output must equal the source packs byte for byte (they hold the same items).

  python tools/pack_bench.py [--n 65536] [--steps 200] [--warmup 20] [--rounds 3] [--out FILE.json]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

import brb_framework_amd as brb
from brb_framework_amd import workload

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=65536)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--settle-s", type=float, default=0.5)
ap.add_argument("--out", default=None)
args = ap.parse_args()

n, K, Q, L = args.n, 4, 375, 1500
P_SZ = 64 + K * (24 + Q + 1)
dev = torch.device("cuda:0")
Lb = brb.lib()
flags = brb.BATCH_DEVICE | brb.BATCH_ASYNC

# the source packs, as bench.py --op metadata builds them
host = workload.gen_records(workload.SEEDS[2], 0, n, L)
packs = np.zeros((n, P_SZ), np.uint8)
packs[:, :24] = np.frombuffer(np.array([0, K], "<i4").tobytes() + np.array([P_SZ - 64], "<u8").tobytes() + b"BRB_META",
                              np.uint8)
packs[:, 24:40] = brb.md5_batch_fixed(host, L, n)
for j in range(K):
    o = 64 + j * (24 + Q + 1)
    packs[:, o:o + 24] = np.frombuffer(np.array([j + 1, 0, Q], "<u8").tobytes(), np.uint8)
    packs[:, o + 24:o + 24 + Q] = host.reshape(n, L)[:, j * Q:(j + 1) * Q]
    packs[:, o + 24 + Q] = 0x1F
flat = packs.reshape(-1)
n_rot = max(2, math.ceil(640e6 / flat.nbytes))
srcs = [torch.from_numpy(flat).to(dev)]
for _ in range(n_rot - 1):
    srcs.append(srcs[0].clone())
outs = [torch.zeros(flat.nbytes, dtype=torch.uint8, device=dev) for _ in range(n_rot)]


def i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(dev)


pack_off = np.arange(n, dtype=np.uint64) * P_SZ
item0 = np.array([64 + j * (24 + Q + 1) + 24 for j in range(K)], np.uint64)
ioff = i64((pack_off[:, None] + item0[None, :]).reshape(-1))
ilen = torch.full((n * K,), Q, dtype=torch.int32, device=dev)
iid = i64(np.tile(np.arange(1, K + 1, dtype=np.uint64), n))
isub = i64(np.zeros(n * K, np.uint64))
first = i64(np.arange(n + 1, dtype=np.uint64) * K)
ooff = i64(pack_off)
digs = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
stream = torch.cuda.current_stream(dev)
h = stream.cuda_stream


def need(rc):
    if rc != 1:
        raise RuntimeError(Lb.BRB_CryptoGPU_LastError().decode())


def pack(k):
    need(Lb.BRB_MetaDataPackBatch(srcs[k % n_rot].data_ptr(), ioff.data_ptr(), ilen.data_ptr(), iid.data_ptr(),
                                  isub.data_ptr(), first.data_ptr(), n, outs[k % n_rot].data_ptr(), ooff.data_ptr(),
                                  flags, h))


def seg(k):
    need(Lb.BRB_MD5BatchSegments(srcs[k % n_rot].data_ptr(), ioff.data_ptr(), ilen.data_ptr(), first.data_ptr(), n,
                                 digs.data_ptr(), flags, h))


def copy(k):
    outs[k % n_rot].copy_(srcs[k % n_rot])


def timed(fn, seg_line=None):
    """us per launch: settle, W warm-up launches, K launches between two events."""
    opt = brb.TestOption("seg_line", seg_line) if seg_line is not None else None
    if opt:
        opt.__enter__()
    try:
        t0, m = time.perf_counter(), 0
        while time.perf_counter() - t0 < args.settle_s:
            for _ in range(8):
                fn(m)
                m += 1
            torch.cuda.synchronize()
        for k in range(args.warmup):
            fn(m + k)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for k in range(args.steps):
            fn(k)
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) / args.steps * 1e3
    finally:
        if opt:
            opt.__exit__(None, None, None)


cases = [("a_pack", pack, None), ("b_md5seg_lane", seg, 0), ("c_copy", copy, None), ("b2_md5seg_pairs", seg, 2)]
times = {name: [] for name, _, _ in cases}
for _ in range(args.rounds):
    for name, fn, sl in cases:
        times[name].append(timed(fn, sl))

# the packed output equals the source packs (same items, ids and digests), in every output buffer used
for k in range(n_rot):
    outs[k].zero_()
    pack(k)
torch.cuda.synchronize()
brb.async_fault_check()
assert all(torch.equal(outs[k], srcs[k]) for k in range(n_rot)), "packed output differs from the source packs"
assert np.array_equal(digs.cpu().numpy(), packs[:, 24:40]), "segment digests differ from the packs' digests"

med = {k: statistics.median(v) for k, v in times.items()}
item_bytes, out_bytes = n * K * Q, n * P_SZ
list_bytes = n * K * (8 + 4 + 8 + 8) + (n + 1) * 8 + n * 8
result = {
    "shape": {"packs": n, "items_per_pack": K, "item_bytes": Q, "pack_bytes": P_SZ},
    "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "settle_s": args.settle_s,
    "us_per_launch": {k: round(v, 2) for k, v in med.items()},
    "us_per_launch_rounds": {k: [round(x, 2) for x in v] for k, v in times.items()},
    "bytes": {"a_read_items": item_bytes, "a_read_lists": list_bytes, "a_written": out_bytes,
              "b_read_items": item_bytes, "b_written": 16 * n, "c_read": out_bytes, "c_written": out_bytes},
    "bound_us": round(med["b_md5seg_lane"] + med["c_copy"], 2),
    "a_within_bound": bool(med["a_pack"] <= med["b_md5seg_lane"] + med["c_copy"]),
    "a_GBps_of_pack_bytes_written": round(out_bytes / med["a_pack"] / 1e3, 1),
    "device": torch.cuda.get_device_name(0),
}
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
