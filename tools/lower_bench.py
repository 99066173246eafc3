"""BRB_MD5LowerTextBatch beside the calls a caller would use without it, on one GPU and in one run, device
mode, event timing (tools/stream_seg_bench.py's method).  Keys of seeded uniform lengths packed back to back in
one device buffer, random bytes (about a tenth of them 'A'..'Z'):

  (A) BRB_MD5LowerTextBatch, digests only
  (C) BRB_MD5Batch on the same keys lower-cased beforehand on the host (the lower-casing is not counted)
  (D) BRB_MD5InitBatch + BRB_MD5UpdateSegmentsLowerBatch with final, one segment per context: what the
      context-free call saves

The legs are interleaved round by round; median, min and max over the rounds are reported.  Before anything is
timed A, C and D are compared with each other and, for a few keys, with hashlib.  A against C is reported, not
gated.  (Leg B of DESIGN §4.8b, the span-staged block source against the per-lane one, went with the path it
measured.)

  python tools/lower_bench.py [--keys 1048576] [--min-len 8] [--max-len 64] [--steps 20] [--warmup 3] [--rounds 7]
                              [--out FILE.json]
  python tools/lower_bench.py --keys 65536 --min-len 1500 --max-len 1500     # cfg2's shape: every group per lane
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

import brb_framework_amd as brb

ap = argparse.ArgumentParser()
ap.add_argument("--keys", type=int, default=1 << 20)
ap.add_argument("--min-len", type=int, default=8)
ap.add_argument("--max-len", type=int, default=64)
ap.add_argument("--seed", type=int, default=20250)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
Lb = brb.lib()
if not brb.gpu_available():
    raise RuntimeError("no usable HIP device: " + Lb.BRB_CryptoGPU_LastError().decode())
FLAGS = brb.BATCH_DEVICE | brb.BATCH_ASYNC
stream = torch.cuda.current_stream(dev)
h = stream.cuda_stream
N = args.keys


def need(rc):
    if rc != 1:
        raise RuntimeError(Lb.BRB_CryptoGPU_LastError().decode())


rng = np.random.default_rng(args.seed)
lens = rng.integers(args.min_len, args.max_len + 1, N).astype(np.uint32)
offs = np.concatenate([[0], np.cumsum(lens, dtype=np.uint64)[:-1]]).astype(np.uint64)
total = int(lens.sum(dtype=np.uint64))
host = rng.integers(0, 256, total + 8, dtype=np.uint8)
upper = (host >= 0x41) & (host <= 0x5A)
host_low = host.copy()
host_low[upper] += 0x20

data = torch.from_numpy(host).to(dev)
data_low = torch.from_numpy(host_low).to(dev)
d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
d_first = torch.arange(N + 1, dtype=torch.int64, device=dev)
fin1 = torch.ones(N, dtype=torch.uint8, device=dev)
ctxs = torch.zeros((N, brb.MD5_CTX_BYTES), dtype=torch.uint8, device=dev)
out = {k: torch.empty((N, 16), dtype=torch.uint8, device=dev) for k in "ACD"}


def leg_a():
    need(Lb.BRB_MD5LowerTextBatch(data.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), N, out["A"].data_ptr(), None, FLAGS, h))


def leg_c():
    need(Lb.BRB_MD5Batch(data_low.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), N, out["C"].data_ptr(), FLAGS, h))


def leg_d():
    need(Lb.BRB_MD5InitBatch(ctxs.data_ptr(), N, None, N, FLAGS, h))
    need(Lb.BRB_MD5UpdateSegmentsLowerBatch(ctxs.data_ptr(), N, None, data.data_ptr(), d_off.data_ptr(), d_len.data_ptr(),
                                            None, d_first.data_ptr(), N, fin1.data_ptr(), out["D"].data_ptr(), FLAGS, h))


legs = {"A_lower_text": leg_a, "C_md5_batch_prelowered": leg_c, "D_init_segments_lower_final": leg_d}

# ---- the results agree before anything is timed -----------------------------------------------------
for launch in legs.values():
    launch()
torch.cuda.synchronize()
for k in "CD":
    assert torch.equal(out["A"], out[k]), f"leg {k} differs from leg A"
for r in (0, 1, N // 2, N - 1):
    key = host_low[int(offs[r]):int(offs[r]) + int(lens[r])].tobytes()
    assert out["A"][r].cpu().numpy().tobytes() == hashlib.md5(key).digest(), r
assert torch.equal(data.cpu(), torch.from_numpy(host)), "data was written"


def timed(launch):
    """us per launch: warm-up launches, then `steps` launches between two events."""
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


times = {k: [] for k in legs}
for _ in range(args.rounds):
    for k, launch in legs.items():
        times[k].append(timed(launch))
r2 = lambda x: round(x, 2)
med = {k: statistics.median(v) for k, v in times.items()}
a, c, d = (med[k] for k in legs)
result = {
    "shape": {"keys": N, "min_len": args.min_len, "max_len": args.max_len, "bytes": total, "seed": args.seed,
              "upper_case_fraction": round(float(upper.mean()), 4)},
    "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "checked": True,
    "us_per_launch": {k: {"median": r2(med[k]), "min": r2(min(v)), "max": r2(max(v))} for k, v in times.items()},
    "us_per_launch_rounds": {k: [r2(x) for x in v] for k, v in times.items()},
    "comparisons": {"A_over_C": round(a / c, 3), "D_over_A": round(d / a, 3)},
    "device": torch.cuda.get_device_name(0),
}
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
