"""Streaming-context Update beside the whole-record digest calls, on one GPU and in one run, device mode,
event timing.  65 536 contexts, each taking a 1 500-byte piece of one buffer (cfg2's bytes):

  (a)  BRB_MD5UpdateBatch, every context with 0 bytes buffered
  (b)  BRB_MD5UpdateBatch, the buffered counts uniform in 0 .. 63
  (c)  BRB_MD5Batch on the same bytes (the line-staged kernel)
  (d)  BRB_MD5BatchSegments, one segment per record, test option seg_line = 0: the per-lane BlockSrc
       kernel, the yardstick of (a) and (b) -- the same read path, one lane per record
  (e)  a one-thread host loop of BRB_MD5Update over the same pieces (through ctypes; the cost of an empty
       call is measured beside it and taken off in the "net" figure)
  (f)  BRB_MD5FinalBatch
  and (a), (b), (c), (e) for SHA-1.

An Update changes its context, so every launch of a timed region gets a table of its own (warm-up +
steps tables, refilled outside the timed region): every launch sees the buffered counts the leg names, and
no launch finds its table in a cache.  The timed legs are interleaved round by round and the median over
the rounds is reported; before anything is timed, Init + Update + Final is compared with the whole-record
call and with hashlib.

  python tools/stream_bench.py [--contexts 65536] [--steps 20] [--warmup 3] [--rounds 5] [--out FILE.json]
"""
import argparse
import ctypes
import hashlib
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
from brb_framework_amd import workload

ap = argparse.ArgumentParser()
ap.add_argument("--contexts", type=int, default=65536)
ap.add_argument("--piece-bytes", type=int, default=1500)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--host-pieces", type=int, default=4096)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
Lb = brb.lib()
if not brb.gpu_available():
    raise RuntimeError("no usable HIP device: " + Lb.BRB_CryptoGPU_LastError().decode())
FLAGS = brb.BATCH_DEVICE | brb.BATCH_ASYNC
stream = torch.cuda.current_stream(dev)
h = stream.cuda_stream
N, PB = args.contexts, args.piece_bytes
T = args.warmup + args.steps                        # tables per timed region
WIDTH = {"md5": brb.MD5_CTX_BYTES, "sha1": brb.SHA1_CTX_BYTES}
DIG = {"md5": 16, "sha1": 20}
UPDATE = {"md5": Lb.BRB_MD5UpdateBatch, "sha1": Lb.BrbSha1_UpdateBatch}
WHOLE = {"md5": Lb.BRB_MD5Batch, "sha1": Lb.BrbSha1_Batch}


def need(rc):
    if rc != 1:
        raise RuntimeError(Lb.BRB_CryptoGPU_LastError().decode())


host = workload.gen_records(workload.SEEDS[2], 0, N, PB)
data = torch.from_numpy(host).to(dev)
d_off = torch.arange(N, dtype=torch.int64, device=dev) * PB
d_len = torch.full((N,), PB, dtype=torch.int32, device=dev)
d_first = torch.arange(N + 1, dtype=torch.int64, device=dev)
rng = np.random.default_rng(11)

# ---- the results agree before anything is timed -----------------------------------------------------
check = {}
for alg in ("md5", "sha1"):
    ctxs = torch.zeros((N, WIDTH[alg]), dtype=torch.uint8, device=dev)
    getattr(brb, alg + "_init_batch")(ctxs)
    getattr(brb, alg + "_update_batch")(ctxs, data, d_off, d_len)
    got = getattr(brb, alg + "_final_batch")(ctxs)
    whole = getattr(brb, alg + "_batch")(data, d_off, d_len)
    assert torch.equal(got, whole), alg + ": Init + Update + Final differs from the whole-record call"
    for r in (0, N // 2, N - 1):
        assert got[r].cpu().numpy().tobytes() == getattr(hashlib, alg)(host[r * PB:(r + 1) * PB].tobytes()).digest()
    check[alg] = True


def tables(alg, spread, pool=True):
    """(pristine table, pool of T tables or None): contexts after Init (+ an Update of 0 .. 63 bytes when spread)."""
    one = torch.zeros((N, WIDTH[alg]), dtype=torch.uint8, device=dev)
    getattr(brb, alg + "_init_batch")(one)
    if spread:
        pre = torch.from_numpy(rng.integers(0, 64, N).astype(np.int32)).to(dev)
        getattr(brb, alg + "_update_batch")(one, data, d_off, pre)
    return one, torch.empty((T, N, WIDTH[alg]), dtype=torch.uint8, device=dev) if pool else None


def update_leg(alg, spread):
    one, pool = tables(alg, spread)
    k = [0]

    def prepare():
        pool.copy_(one.unsqueeze(0).expand_as(pool))
        k[0] = 0

    def launch():
        need(UPDATE[alg](pool[k[0]].data_ptr(), N, None, data.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), N, FLAGS, h))
        k[0] += 1

    return prepare, launch


def whole_leg(alg):
    out = torch.empty((N, DIG[alg]), dtype=torch.uint8, device=dev)
    return None, lambda: need(WHOLE[alg](data.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), N, out.data_ptr(), FLAGS, h))


def seg_leg():
    out = torch.empty((N, 16), dtype=torch.uint8, device=dev)

    def launch():
        with brb.TestOption("seg_line", 0):
            need(Lb.BRB_MD5BatchSegments(data.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), d_first.data_ptr(), N,
                                         out.data_ptr(), FLAGS, h))
    return None, launch


def final_leg():
    one, _ = tables("md5", True, pool=False)
    return None, lambda: need(Lb.BRB_MD5FinalBatch(one.data_ptr(), N, None, N, None, FLAGS, h))


def timed(prepare, launch):
    """us per launch: warm-up launches, then `steps` launches between two events."""
    if prepare:
        prepare()
    for _ in range(args.warmup):
        launch()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(args.steps):
        launch()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / args.steps * 1e3


legs = {
    "a_md5_update_have0": update_leg("md5", False),
    "b_md5_update_have_spread": update_leg("md5", True),
    "c_md5_batch": whole_leg("md5"),
    "d_md5_segments_per_lane": seg_leg(),
    "f_md5_final": final_leg(),
    "a_sha1_update_have0": update_leg("sha1", False),
    "b_sha1_update_have_spread": update_leg("sha1", True),
    "c_sha1_batch": whole_leg("sha1"),
}
t_settle = time.perf_counter()
while time.perf_counter() - t_settle < 0.3:
    legs["c_md5_batch"][1]()
    torch.cuda.synchronize()
times = {k: [] for k in legs}
for _ in range(args.rounds):
    for k, (prepare, launch) in legs.items():
        times[k].append(timed(prepare, launch))
med = {k: statistics.median(v) for k, v in times.items()}


# ---- leg e: one host thread, one compat Update per piece, wall clock ----------------------------------
def host_loop(fn, ctx, n_bytes):
    """(seconds per call with n_bytes, seconds per empty call) over --host-pieces calls, best of 3."""
    base = host.ctypes.data
    out = []
    for nb in (n_bytes, 0):
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            for i in range(args.host_pieces):
                fn(ctx, base + i * PB, nb)
            dt = (time.perf_counter() - t0) / args.host_pieces
            best = dt if best is None else min(best, dt)
        out.append(best)
    return out


md5_ctx, sha1_ctx = brb.BRB_MD5_CTX(), brb.BrbSha1Ctx()
Lb.BRB_MD5Init(ctypes.byref(md5_ctx))
Lb.BrbSha1_Init(ctypes.byref(sha1_ctx))
host_copy = host.copy()                             # BrbSha1_Update rewrites its input: the MD5 loop runs first
e = {}
for alg, fn, ctx in (("md5", Lb.BRB_MD5Update, ctypes.byref(md5_ctx)), ("sha1", Lb.BrbSha1_Update, ctypes.byref(sha1_ctx))):
    full, empty = host_loop(fn, ctx, PB)
    e[alg] = {"us_per_piece": round(full * 1e6, 3), "us_per_empty_call": round(empty * 1e6, 3),
              "gib_per_s": round(PB / full / 2**30, 3), "gib_per_s_net_of_call": round(PB / (full - empty) / 2**30, 3),
              "us_for_all_pieces_one_thread": round(full * N * 1e6, 1)}
host[:] = host_copy

r2 = lambda x: round(x, 2)
result = {
    "shape": {"contexts": N, "piece_bytes": PB, "piece_bytes_total": N * PB, "md5_context_bytes_moved": 2 * 88 * N,
              "sha1_context_bytes_moved": 2 * 92 * N, "tables_per_region": T},
    "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "checked": check,
    "us_per_launch_median": {k: r2(v) for k, v in med.items()},
    "us_per_launch_rounds": {k: [r2(x) for x in v] for k, v in times.items()},
    "ratios": {
        "a_over_d": r2(med["a_md5_update_have0"] / med["d_md5_segments_per_lane"]),
        "b_over_d": r2(med["b_md5_update_have_spread"] / med["d_md5_segments_per_lane"]),
        "a_over_c": r2(med["a_md5_update_have0"] / med["c_md5_batch"]),
        "sha1_a_over_c": r2(med["a_sha1_update_have0"] / med["c_sha1_batch"]),
        "sha1_b_over_a": r2(med["b_sha1_update_have_spread"] / med["a_sha1_update_have0"]),
    },
    "a_minus_c_us": {"md5": r2(med["a_md5_update_have0"] - med["c_md5_batch"]),
                     "sha1": r2(med["a_sha1_update_have0"] - med["c_sha1_batch"])},
    "within_1_15_of_d": {"a": med["a_md5_update_have0"] <= 1.15 * med["d_md5_segments_per_lane"],
                         "b": med["b_md5_update_have_spread"] <= 1.15 * med["d_md5_segments_per_lane"]},
    "e_host_one_thread": e,
    "device": torch.cuda.get_device_name(0),
}
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
