"""Keyed Blowfish ECB (a context per record) beside what the single-context call offers, on one GPU
and in one run, device mode, event timing:

  (a)  BRB_Blowfish_EncryptBatchKeyed, 4 096 records x 4 KiB, 4 096 distinct contexts made by
       BRB_Blowfish_InitBatch -- one launch
  (b)  the same bytes as a loop of 4 096 BRB_Blowfish_EncryptBatch calls on one stream, record i with
       context i: what the library offered before (the loop is issued from Python through ctypes, so
       the leg is bound by launches and their issue, as such a caller's would be)
  (c)  the same bytes in one single-context call (one key for everything: the floor)
  (d)  leg (a) with every ctx_index 0
  (e)  BRB_MemBufferEncryptBatch / DecryptBatch on 4 096 x 1 KiB buffers with KV_SEED against the loop of
       single calls, wall clock (each single call builds its key schedule on the host and synchronises)
  also (a) and (d) with the plain image fill and with one block per lane (test option "bf_keyed"), and
  (s)  leg (a)'s bytes with one record of 4 MiB among 3 072 of 4 KiB (skewed lengths).

The timed legs are interleaved round by round and the median over the rounds is reported; before
anything is timed (a) is compared with (b) and (c) with the host library.

  python tools/bf_keyed_bench.py [--records 4096] [--steps 20] [--warmup 3] [--rounds 5] [--out FILE.json]
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
from brb_framework_amd import kv

ap = argparse.ArgumentParser()
ap.add_argument("--records", type=int, default=4096)
ap.add_argument("--rec-bytes", type=int, default=4096)
ap.add_argument("--buf-bytes", type=int, default=1024)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--loop-steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--wall-reps", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
Lb = brb.lib()
if not brb.gpu_available():
    raise RuntimeError("no usable HIP device: " + Lb.BRB_CryptoGPU_LastError().decode())
FLAGS = brb.BATCH_DEVICE | brb.BATCH_ASYNC
stream = torch.cuda.current_stream(dev)
h = stream.cuda_stream
N, RB = args.records, args.rec_bytes
BLK = RB // 16
CTX = brb.BLOWFISH_CTX_BYTES


def need(rc):
    if rc != 1:
        raise RuntimeError(Lb.BRB_CryptoGPU_LastError().decode())


rng = np.random.default_rng(9)
keys = rng.integers(0, 256, N * 16, dtype=np.uint8)
d_ctx = brb.blowfish_init_batch(torch.from_numpy(keys).to(dev), torch.arange(N, dtype=torch.int64, device=dev) * 16,
                                torch.full((N,), 16, dtype=torch.int32, device=dev))
plain = torch.from_numpy(rng.integers(0, 1 << 63, N * RB // 8, dtype=np.int64)).to(dev)
words = plain.clone()
d_off = torch.arange(N, dtype=torch.int64, device=dev) * (RB // 8)
d_cnt = torch.full((N,), BLK, dtype=torch.int32, device=dev)
d_zero = torch.zeros(N, dtype=torch.int32, device=dev)
# skew: one record of 4 MiB, the rest 4 KiB, the same bytes in all
n_skew = N - (4 << 20) // RB + 1
skew_cnt = torch.full((n_skew,), BLK, dtype=torch.int32, device=dev)
skew_cnt[n_skew // 2] = (4 << 20) // 16
skew_off = torch.cumsum(skew_cnt.to(torch.int64) * 2, 0) - skew_cnt.to(torch.int64) * 2


def keyed(idx, off=d_off, cnt=d_cnt, n=N):
    need(Lb.BRB_Blowfish_EncryptBatchKeyed(d_ctx.data_ptr(), N, idx.data_ptr() if idx is not None else None,
                                           words.data_ptr(), off.data_ptr(), cnt.data_ptr(), n, FLAGS, h))


def loop_single():
    base, cbase = words.data_ptr(), d_ctx.data_ptr()
    fn = Lb.BRB_Blowfish_EncryptBatch
    for i in range(N):
        if fn(cbase + i * CTX, base + i * RB, BLK, FLAGS, h) != 1:
            need(0)


def one_single():
    need(Lb.BRB_Blowfish_EncryptBatch(d_ctx.data_ptr(), words.data_ptr(), N * BLK, FLAGS, h))


# ---- the results agree before anything is timed -----------------------------------------------------
keyed(None)
got_a = words.clone()
words.copy_(plain)
loop_single()
torch.cuda.synchronize()
assert torch.equal(got_a, words), "keyed call and the loop of single-context calls differ"
words.copy_(plain)
keyed(d_zero)
got_d = words.clone()
words.copy_(plain)
one_single()
torch.cuda.synchronize()
assert torch.equal(got_d, words), "keyed call with one context and the single-context call differ"
ctx0 = brb.BRB_BLOWFISH_CTX.from_buffer_copy(d_ctx[0].cpu().numpy().tobytes())
w0 = plain[:64].cpu().numpy().view(np.uint64).copy()
xl, xr = ctypes.c_ulong(int(w0[0])), ctypes.c_ulong(int(w0[1]))
Lb.BRB_Blowfish_Encrypt(ctypes.byref(ctx0), ctypes.byref(xl), ctypes.byref(xr))
assert (xl.value, xr.value) == tuple(int(x) for x in got_d[:2].cpu().numpy().view(np.uint64)), "differs from the host call"
for variant in (1, 2):
    words.copy_(plain)
    with brb.TestOption("bf_keyed", variant):
        keyed(None)
    torch.cuda.synchronize()
    assert torch.equal(got_a, words), f"bf_keyed variant {variant} differs"


def timed(launch, steps):
    """us per launch: warm-up launches, then `steps` launches between two events."""
    for _ in range(args.warmup):
        launch()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(steps):
        launch()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / steps * 1e3


def with_opt(v, fn):
    def run():
        with brb.TestOption("bf_keyed", v):
            fn()
    return run


legs = {
    "a_keyed_distinct": (lambda: keyed(None), args.steps),
    "b_loop_single_calls": (loop_single, args.loop_steps),
    "c_one_single_call": (one_single, args.steps),
    "d_keyed_one_context": (lambda: keyed(d_zero), args.steps),
    "a_plain_fill": (with_opt(1, lambda: keyed(None)), args.steps),
    "a_ilp1": (with_opt(2, lambda: keyed(None)), args.steps),
    "d_plain_fill": (with_opt(1, lambda: keyed(d_zero)), args.steps),
    "d_ilp1": (with_opt(2, lambda: keyed(d_zero)), args.steps),
    "s_skewed_lengths": (lambda: keyed(None, skew_off, skew_cnt, n_skew), args.steps),
}
t_settle = time.perf_counter()
while time.perf_counter() - t_settle < 0.3:
    one_single()
    torch.cuda.synchronize()
times = {k: [] for k in legs}
for _ in range(args.rounds):
    for k, (fn, steps) in legs.items():
        times[k].append(timed(fn, steps))
med = {k: statistics.median(v) for k, v in times.items()}

# ---- leg e: MemBuffer batch against the loop of single calls, wall clock ------------------------------
BB = args.buf_bytes
room = (BB + brb.membuf_span(BB) + 16 + 15) // 16 * 16
mb_plain = torch.zeros(N * room, dtype=torch.uint8, device=dev)
mb_plain.view(N, room)[:, :BB] = torch.from_numpy(rng.integers(1, 256, (N, BB), dtype=np.uint8)).to(dev)
mb_off = torch.arange(N, dtype=torch.int64, device=dev) * room
mb_size = torch.full((N,), BB, dtype=torch.int64, device=dev)


def wall(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(out), r


def mb_batch(fn, data, sizes):
    return lambda: fn(data, mb_off, sizes, [kv.KV_SEED])


def mb_loop(fn, data, sizes):
    def run():
        base, ns = data.data_ptr(), ctypes.c_ulong(0)
        out = []
        for i in range(N):
            need(fn(base + i * room, sizes[i], kv.KV_SEED, 0, ctypes.byref(ns), brb.BATCH_DEVICE, h))
            out.append(ns.value)
        return out
    return run


sizes_host = [BB] * N
buf = mb_plain.clone()
wall(mb_batch(brb.membuf_encrypt_batch, buf, mb_size), 1)                     # warm: workspace, code objects
buf.copy_(mb_plain)
e_enc_batch, enc_sizes = wall(mb_batch(brb.membuf_encrypt_batch, buf, mb_size), 1)
enc_batch = buf.clone()
buf.copy_(mb_plain)
e_enc_loop, enc_sizes_loop = wall(mb_loop(Lb.BRB_MemBufferEncrypt, buf, sizes_host), 1)
assert torch.equal(buf, enc_batch) and enc_sizes.cpu().tolist() == enc_sizes_loop, "MemBuffer encrypt batch != loop"
e_dec_batch, dec_sizes = wall(mb_batch(brb.membuf_decrypt_batch, buf, enc_sizes), 1)
dec_batch = buf.clone()
enc_times, dec_times = [e_enc_batch], [e_dec_batch]
buf.copy_(enc_batch)
e_dec_loop, dec_sizes_loop = wall(mb_loop(Lb.BRB_MemBufferDecrypt, buf, enc_sizes_loop), 1)
assert torch.equal(buf, dec_batch) and dec_sizes.cpu().tolist() == dec_sizes_loop, "MemBuffer decrypt batch != loop"
# repeat the batch legs for a median, each time from the same bytes
for _ in range(args.wall_reps - 1):
    buf.copy_(mb_plain)
    e_enc_batch_more = wall(mb_batch(brb.membuf_encrypt_batch, buf, mb_size), 1)[0]
    enc_times.append(e_enc_batch_more)
    dec_times.append(wall(mb_batch(brb.membuf_decrypt_batch, buf, enc_sizes), 1)[0])
e_enc_batch, e_dec_batch = statistics.median(enc_times), statistics.median(dec_times)

r2 = lambda x: round(x, 2)
result = {
    "shape": {"records": N, "record_bytes": RB, "contexts": N, "context_bytes": CTX, "membuf_buffers": N,
              "membuf_bytes": BB, "skew": {"records": n_skew, "long_record_bytes": 4 << 20}},
    "steps": args.steps, "loop_steps": args.loop_steps, "warmup": args.warmup, "rounds": args.rounds,
    "us_per_launch_median": {k: r2(v) for k, v in med.items()},
    "us_per_launch_rounds": {k: [r2(x) for x in v] for k, v in times.items()},
    "ratios": {
        "a_over_b": round(med["a_keyed_distinct"] / med["b_loop_single_calls"], 4),
        "a_over_c": r2(med["a_keyed_distinct"] / med["c_one_single_call"]),
        "d_over_c": r2(med["d_keyed_one_context"] / med["c_one_single_call"]),
        "a_plain_fill_over_a": r2(med["a_plain_fill"] / med["a_keyed_distinct"]),
        "a_ilp1_over_a": r2(med["a_ilp1"] / med["a_keyed_distinct"]),
        "d_ilp1_over_d": r2(med["d_ilp1"] / med["d_keyed_one_context"]),
        "s_over_a": r2(med["s_skewed_lengths"] / med["a_keyed_distinct"]),
    },
    "a_less_than_b": med["a_keyed_distinct"] < med["b_loop_single_calls"],
    "e_wall_us": {"encrypt_batch": r2(e_enc_batch), "encrypt_loop_single_calls": r2(e_enc_loop),
                  "decrypt_batch": r2(e_dec_batch), "decrypt_loop_single_calls": r2(e_dec_loop),
                  "encrypt_speedup": r2(e_enc_loop / e_enc_batch), "decrypt_speedup": r2(e_dec_loop / e_dec_batch)},
    "device": torch.cuda.get_device_name(0),
}
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
