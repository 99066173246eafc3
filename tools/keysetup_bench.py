"""Batched key setup beside the per-key host calls it replaces, on one GPU and in one run:

  (a)  BRB_RC4_InitBatch, 16 384 keys x 16 B, device mode, per launch
       | a single-threaded BRB_RC4_Init loop over the same keys
  (b)  BRB_TransformBatcherEnableBatch, 16 384 connections, wall clock
       | a loop of BRB_TransformBatcherEnable (one call, two 264-byte copies and one stream
         synchronisation per connection)
  (c)  BRB_Blowfish_InitBatch, 4 096 keys x 16 B, device mode, per launch
       | a BRB_Blowfish_Init loop on 1 and on 16 host threads

The device legs are timed as the bench legs are: an untimed settle of the same launches, W warm-up
launches, then K launches between two events; `--rounds` rounds with (a) and (c) interleaved, the
median reported.  The host baselines and leg (b) are wall-clock loops in C (tools/keysetup_host.c,
compiled here with the system compiler against the in-tree library), so no interpreter overhead sits
inside a timed loop.  The batch results are compared with the host calls' before anything is printed.

  python tools/keysetup_bench.py [--rc4-keys 16384] [--bf-keys 4096] [--conns 16384] [--threads 16]
                                 [--steps 200] [--bf-steps 40] [--warmup 10] [--rounds 5] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

import brb_framework_amd as brb

ap = argparse.ArgumentParser()
ap.add_argument("--rc4-keys", type=int, default=16384)
ap.add_argument("--bf-keys", type=int, default=4096)
ap.add_argument("--conns", type=int, default=16384)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--bf-steps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--host-reps", type=int, default=5)
ap.add_argument("--settle-s", type=float, default=0.3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

KEY = 16
dev = torch.device("cuda:0")
Lb = brb.lib()
if not brb.gpu_available():
    raise RuntimeError("no usable HIP device: " + Lb.BRB_CryptoGPU_LastError().decode())
flags = brb.BATCH_DEVICE | brb.BATCH_ASYNC
stream = torch.cuda.current_stream(dev)
h = stream.cuda_stream


def need(rc):
    if rc != 1:
        raise RuntimeError(Lb.BRB_CryptoGPU_LastError().decode())


def leg(n, width, fn):
    keys = np.random.default_rng(n).integers(0, 256, n * KEY, dtype=np.uint8)
    d_keys = torch.from_numpy(keys).to(dev)
    d_offs = torch.arange(n, dtype=torch.int64, device=dev) * KEY
    d_lens = torch.full((n,), KEY, dtype=torch.int32, device=dev)
    out = torch.zeros((n, width), dtype=torch.uint8, device=dev)

    def launch():
        need(fn(out.data_ptr(), d_keys.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n, flags, h))

    return keys.reshape(n, KEY), out, launch


def timed(launch, steps):
    """us per launch: settle, W warm-up launches, `steps` launches between two events."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < args.settle_s:
        for _ in range(4):
            launch()
        torch.cuda.synchronize()
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


rc4_keys, rc4_out, rc4_launch = leg(args.rc4_keys, brb.RC4_STATE_BYTES, Lb.BRB_RC4_InitBatch)
bf_keys, bf_out, bf_launch = leg(args.bf_keys, brb.BLOWFISH_CTX_BYTES, Lb.BRB_Blowfish_InitBatch)
times = {"a_rc4_init_batch": [], "c_blowfish_init_batch": []}
for _ in range(args.rounds):
    times["a_rc4_init_batch"].append(timed(rc4_launch, args.steps))
    times["c_blowfish_init_batch"].append(timed(bf_launch, args.bf_steps))

# the batch results equal the host calls' (every RC4 state; every 16th Blowfish context)
assert np.array_equal(rc4_out.cpu().numpy(), brb.rc4_states([k.tobytes() for k in rc4_keys])), "RC4 states differ"
got_bf = bf_out.cpu().numpy()
for i in range(0, args.bf_keys, 16):
    assert got_bf[i].tobytes() == brb.blowfish_ctx_bytes(brb.blowfish_init(bf_keys[i].tobytes())), f"Blowfish context {i}"

# host baselines and the batcher leg, in C, in a process of their own
with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, "keysetup_host")
    libdir = os.path.dirname(brb.LIB_PATH)
    subprocess.run(["gcc", "-O2", "-std=gnu11", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "keysetup_host.c"), "-L", libdir, "-lbrb_crypto_gpu",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    host = json.loads(subprocess.run([exe, str(args.rc4_keys), str(args.bf_keys), str(args.conns), str(args.threads),
                                      str(args.host_reps)], check=True, capture_output=True, text=True).stdout)
assert host["batcher_states_equal"], "EnableBatch and the Enable loop left different states"

med = {k: statistics.median(v) for k, v in times.items()}
result = {
    "shape": {"rc4_keys": args.rc4_keys, "bf_keys": args.bf_keys, "conns": args.conns, "key_bytes": KEY,
              "host_threads": args.threads},
    "steps": args.steps, "bf_steps": args.bf_steps, "warmup": args.warmup, "rounds": args.rounds,
    "host_reps": args.host_reps, "settle_s": args.settle_s,
    "us": {
        "a_rc4_init_batch_per_launch": round(med["a_rc4_init_batch"], 2),
        "a_host_rc4_init_loop_1t": host["rc4_init_loop_us"],
        "b_enable_batch_wall": host["enable_batch_us"],
        "b_host_enable_loop_wall": host["enable_loop_us"],
        "c_blowfish_init_batch_per_launch": round(med["c_blowfish_init_batch"], 2),
        "c_host_blowfish_init_loop_1t": host["bf_init_loop_1t_us"],
        "c_host_blowfish_init_loop_mt": host["bf_init_loop_mt_us"],
    },
    "us_per_launch_rounds": {k: [round(x, 2) for x in v] for k, v in times.items()},
    "speedup": {
        "a_vs_1t": round(host["rc4_init_loop_us"] / med["a_rc4_init_batch"], 2),
        "b_vs_enable_loop": round(host["enable_loop_us"] / host["enable_batch_us"], 2),
        "c_vs_1t": round(host["bf_init_loop_1t_us"] / med["c_blowfish_init_batch"], 2),
        "c_vs_mt": round(host["bf_init_loop_mt_us"] / med["c_blowfish_init_batch"], 2),
    },
    "device": torch.cuda.get_device_name(0),
}
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
