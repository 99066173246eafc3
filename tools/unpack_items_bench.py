"""BRB_MetaDataUnpackItemsBatch beside BRB_MetaDataUnpackBatch at the MetaData bench shape (65 536 packs x
4 items x 375 B, HBM-resident), in one process and interleaved: what writing the item table (4 stores,
28 bytes per item: 7.3 MB on top of 111 MB read) costs the walking wave, for each form of the walk --
the wave pairs (seg_line 2, the default), the line kernel (1) and the per-lane kernel (0).

Timed as the bench legs are: an untimed settle of the same launches, W warm-up launches, then K launches
between two events, on rotating pack buffers larger than the caches; `--rounds` interleaved rounds, the
median reported.  Afterwards the table of every buffer is checked against the layout the packs were
built with, and info against the plain call's.

  python tools/unpack_items_bench.py [--n 65536] [--steps 2000] [--warmup 20] [--rounds 5] [--out FILE.json]
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
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--settle-s", type=float, default=0.5)
ap.add_argument("--out", default=None)
args = ap.parse_args()

n, K, Q, L = args.n, 4, 375, 1500
P_SZ = 64 + K * (24 + Q + 1)
dev = torch.device("cuda:0")
Lb = brb.lib()
flags = brb.BATCH_DEVICE | brb.BATCH_ASYNC

# the packs, as bench.py --op metadata builds them
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


def i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(dev)


pack_off = np.arange(n, dtype=np.uint64) * P_SZ
offs = i64(pack_off)
lens = torch.full((n,), P_SZ, dtype=torch.int32, device=dev)
first = i64(np.arange(n + 1, dtype=np.uint64) * K)
info = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
info_items = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
tabs = [(torch.zeros(n * K, dtype=torch.int64, device=dev), torch.zeros(n * K, dtype=torch.int32, device=dev),
         torch.zeros(n * K, dtype=torch.int64, device=dev), torch.zeros(n * K, dtype=torch.int64, device=dev),
         torch.zeros(n, dtype=torch.int32, device=dev)) for _ in range(n_rot)]
stream = torch.cuda.current_stream(dev)
h = stream.cuda_stream


def need(rc):
    if rc != 1:
        raise RuntimeError(Lb.BRB_CryptoGPU_LastError().decode())


def plain(k):
    need(Lb.BRB_MetaDataUnpackBatch(srcs[k % n_rot].data_ptr(), offs.data_ptr(), lens.data_ptr(), n, info.data_ptr(),
                                    flags, h))


def items(k):
    io, il, ii, isub, added = tabs[k % n_rot]
    need(Lb.BRB_MetaDataUnpackItemsBatch(srcs[k % n_rot].data_ptr(), offs.data_ptr(), lens.data_ptr(), n,
                                         info_items.data_ptr(), io.data_ptr(), il.data_ptr(), ii.data_ptr(),
                                         isub.data_ptr(), first.data_ptr(), added.data_ptr(), flags, h))


def timed(fn, seg_line):
    """us per launch: settle, W warm-up launches, K launches between two events."""
    with brb.TestOption("seg_line", seg_line):
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


FORMS = {2: "pairs", 1: "line", 0: "lane"}
cases = [(f"{kind}_{FORMS[sl]}", fn, sl) for sl in (2, 1, 0) for kind, fn in (("plain", plain), ("items", items))]
times = {name: [] for name, _, _ in cases}
for _ in range(args.rounds):
    for name, fn, sl in cases:
        times[name].append(timed(fn, sl))

# the table of every buffer, by every form of the walk, is the layout the packs were built with
want_off = (pack_off[:, None] + np.array([64 + j * (24 + Q + 1) + 24 for j in range(K)], np.uint64)[None, :]).reshape(-1)
for sl in FORMS:
    for k in range(n_rot):
        for t in tabs[k]:
            t.fill_(-1)
        with brb.TestOption("seg_line", sl):
            items(k)
            plain(k)
        torch.cuda.synchronize()
        brb.async_fault_check()
        io, il, ii, isub, added = (t.cpu().numpy() for t in tabs[k])
        assert np.array_equal(io.view(np.uint64), want_off) and (il == Q).all() and (isub == 0).all(), "table differs"
        assert np.array_equal(ii, np.tile(np.arange(1, K + 1), n)) and (added == K).all(), "table differs"
        assert torch.equal(info, info_items), "info differs from the plain call's"
got = info.cpu().numpy().reshape(-1).view(brb.METADATA_INFO_DTYPE)
assert (got["error_code"] == 7).all() and (got["item_count"] == K).all()

med = {k: statistics.median(v) for k, v in times.items()}
result = {
    "shape": {"packs": n, "items_per_pack": K, "item_bytes": Q, "pack_bytes": P_SZ},
    "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "settle_s": args.settle_s,
    "us_per_launch": {k: round(v, 2) for k, v in med.items()},
    "us_per_launch_rounds": {k: [round(x, 2) for x in v] for k, v in times.items()},
    "items_over_plain": {f: round(med[f"items_{f}"] / med[f"plain_{f}"], 4) for f in FORMS.values()},
    "bytes": {"read_packs": n * P_SZ, "read_lists": n * 12 + (n + 1) * 8, "written_info": 32 * n,
              "written_table": n * K * 28 + 4 * n},
    "device": torch.cuda.get_device_name(0),
}
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
