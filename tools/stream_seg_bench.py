"""The segment-list call of the streaming contexts (BRB_MD5UpdateSegmentsBatch / BrbSha1_UpdateSegmentsBatch)
beside the calls it subsumes, on one GPU and in one run, device mode, event timing: tools/stream_bench.py's
method.  65 536 contexts, each taking 1 500 bytes of one buffer (cfg2's bytes):

  (a)   UpdateBatch, one 1 500-byte piece, every context with 0 bytes buffered (stream_bench's leg a)
  (f)   FinalBatch
  (s1)  the new call, one 1 500-byte segment, no final
  (s1f) the new call, one segment and final
  (s4)  the new call, four 375-byte segments, no final
  (u4)  four consecutive UpdateBatch calls over the same four pieces
  (d)   BRB_MD5BatchSegments, one segment per record, test option seg_line = 0 (MD5 only)

Every call here changes its contexts, so every launch of a timed region gets a table of its own (warm-up +
steps tables, refilled outside the timed region; one table per group of four calls for u4): no launch finds
its table in a cache.  The legs are interleaved round by round and the median over the rounds is reported;
before anything is timed the new call's digests are compared with the whole-record call and with hashlib.
Two comparisons count, both against existing calls in the same run: (s4) <= (u4) and (s1f) <= (a) + (f).

  python tools/stream_seg_bench.py [--contexts 65536] [--steps 20] [--warmup 3] [--rounds 5] [--out FILE.json]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch

import brb_framework_amd as brb
from brb_framework_amd import workload

ap = argparse.ArgumentParser()
ap.add_argument("--contexts", type=int, default=65536)
ap.add_argument("--piece-bytes", type=int, default=1500)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
Lb = brb.lib()
if not brb.gpu_available():
    raise RuntimeError("no usable HIP device: " + Lb.BRB_CryptoGPU_LastError().decode())
FLAGS = brb.BATCH_DEVICE | brb.BATCH_ASYNC
stream = torch.cuda.current_stream(dev)
h = stream.cuda_stream
N, PB, K = args.contexts, args.piece_bytes, 4
assert PB % K == 0, "--piece-bytes must divide into four segments"
QB = PB // K
T = args.warmup + args.steps                        # tables per timed region
WIDTH = {"md5": brb.MD5_CTX_BYTES, "sha1": brb.SHA1_CTX_BYTES}
DIG = {"md5": 16, "sha1": 20}
UPDATE = {"md5": Lb.BRB_MD5UpdateBatch, "sha1": Lb.BrbSha1_UpdateBatch}
FINAL = {"md5": Lb.BRB_MD5FinalBatch, "sha1": Lb.BrbSha1_FinalBatch}
SEGS = {"md5": Lb.BRB_MD5UpdateSegmentsBatch, "sha1": Lb.BrbSha1_UpdateSegmentsBatch}


def need(rc):
    if rc != 1:
        raise RuntimeError(Lb.BRB_CryptoGPU_LastError().decode())


host = workload.gen_records(workload.SEEDS[2], 0, N, PB)
data = torch.from_numpy(host).to(dev)
d_off = torch.arange(N, dtype=torch.int64, device=dev) * PB
d_len = torch.full((N,), PB, dtype=torch.int32, device=dev)
d_first = torch.arange(N + 1, dtype=torch.int64, device=dev)
q_off = torch.arange(N * K, dtype=torch.int64, device=dev) * QB      # the same bytes as four segments per context
q_len = torch.full((N * K,), QB, dtype=torch.int32, device=dev)
q_first = torch.arange(N + 1, dtype=torch.int64, device=dev) * K
u_off = [(d_off + j * QB).contiguous() for j in range(K)]            # and as four pieces, one per call
u_len = torch.full((N,), QB, dtype=torch.int32, device=dev)
fin1 = torch.ones(N, dtype=torch.uint8, device=dev)

# ---- the results agree before anything is timed -----------------------------------------------------
check = {}
for alg in ("md5", "sha1"):
    whole = getattr(brb, alg + "_batch")(data, d_off, d_len)
    segs = getattr(brb, alg + "_update_segments_batch")
    for name, (so, sl, sf) in {"s1f": (d_off, d_len, d_first), "s4f": (q_off, q_len, q_first)}.items():
        ctxs = torch.zeros((N, WIDTH[alg]), dtype=torch.uint8, device=dev)
        getattr(brb, alg + "_init_batch")(ctxs)
        got = segs(ctxs, data, so, sl, sf, final=fin1)
        assert torch.equal(got, whole), f"{alg} {name}: Init + segments + final differs from the whole-record call"
    ctxs = torch.zeros((N, WIDTH[alg]), dtype=torch.uint8, device=dev)
    getattr(brb, alg + "_init_batch")(ctxs)
    assert segs(ctxs, data, q_off, q_len, q_first) is None
    got = getattr(brb, alg + "_final_batch")(ctxs)
    assert torch.equal(got, whole), alg + ": Init + segments, then FinalBatch, differs from the whole-record call"
    for r in (0, N // 2, N - 1):
        assert got[r].cpu().numpy().tobytes() == getattr(hashlib, alg)(host[r * PB:(r + 1) * PB].tobytes()).digest()
    check[alg] = True


def pooled(alg, launch_on):
    """A leg whose every launch takes the next of T tables of Init'd contexts (refilled outside the timed region)."""
    one = torch.zeros((N, WIDTH[alg]), dtype=torch.uint8, device=dev)
    getattr(brb, alg + "_init_batch")(one)
    pool = torch.empty((T, N, WIDTH[alg]), dtype=torch.uint8, device=dev)
    k = [0]

    def prepare():
        pool.copy_(one.unsqueeze(0).expand_as(pool))
        k[0] = 0

    def launch():
        launch_on(pool[k[0]].data_ptr())
        k[0] += 1

    return prepare, launch


def update_leg(alg):
    return pooled(alg, lambda c: need(UPDATE[alg](c, N, None, data.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), N, FLAGS, h)))


def update4_leg(alg):
    def four(c):
        for j in range(K):
            need(UPDATE[alg](c, N, None, data.data_ptr(), u_off[j].data_ptr(), u_len.data_ptr(), N, FLAGS, h))
    return pooled(alg, four)


def final_leg(alg):
    out = torch.empty((N, DIG[alg]), dtype=torch.uint8, device=dev)
    return pooled(alg, lambda c: need(FINAL[alg](c, N, None, N, out.data_ptr(), FLAGS, h)))


def seg_leg(alg, so, sl, sf, final):
    out = torch.empty((N, DIG[alg]), dtype=torch.uint8, device=dev)
    fp = fin1.data_ptr() if final else None
    return pooled(alg, lambda c: need(SEGS[alg](c, N, None, data.data_ptr(), so.data_ptr(), sl.data_ptr(), sf.data_ptr(), N,
                                                fp, out.data_ptr() if final else None, FLAGS, h)))


def whole_seg_leg():
    out = torch.empty((N, 16), dtype=torch.uint8, device=dev)

    def launch():
        with brb.TestOption("seg_line", 0):
            need(Lb.BRB_MD5BatchSegments(data.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), d_first.data_ptr(), N,
                                         out.data_ptr(), FLAGS, h))
    return None, launch


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


legs = {}
for alg in ("md5", "sha1"):
    legs[f"a_{alg}_update"] = update_leg(alg)
    legs[f"f_{alg}_final"] = final_leg(alg)
    legs[f"s1_{alg}_segments_1"] = seg_leg(alg, d_off, d_len, d_first, False)
    legs[f"s1f_{alg}_segments_1_final"] = seg_leg(alg, d_off, d_len, d_first, True)
    legs[f"s4_{alg}_segments_4"] = seg_leg(alg, q_off, q_len, q_first, False)
    legs[f"u4_{alg}_update_x4"] = update4_leg(alg)
legs["d_md5_segments_per_lane"] = whole_seg_leg()
t_settle = time.perf_counter()
while time.perf_counter() - t_settle < 0.3:
    legs["d_md5_segments_per_lane"][1]()
    torch.cuda.synchronize()
times = {k: [] for k in legs}
for _ in range(args.rounds):
    for k, (prepare, launch) in legs.items():
        times[k].append(timed(prepare, launch))
med = {k: statistics.median(v) for k, v in times.items()}

r2 = lambda x: round(x, 2)
compare = {}
for alg in ("md5", "sha1"):
    s4, u4 = med[f"s4_{alg}_segments_4"], med[f"u4_{alg}_update_x4"]
    s1f, af = med[f"s1f_{alg}_segments_1_final"], med[f"a_{alg}_update"] + med[f"f_{alg}_final"]
    compare[alg] = {"s4_us": r2(s4), "u4_us": r2(u4), "s4_le_u4": s4 <= u4, "s1f_us": r2(s1f), "a_plus_f_us": r2(af),
                    "s1f_le_a_plus_f": s1f <= af,
                    "s1_over_a": r2(med[f"s1_{alg}_segments_1"] / med[f"a_{alg}_update"])}
result = {
    "shape": {"contexts": N, "piece_bytes": PB, "segments_per_context": K, "segment_bytes": QB, "tables_per_region": T},
    "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "checked": check,
    "us_per_launch_median": {k: r2(v) for k, v in med.items()},
    "us_per_launch_rounds": {k: [r2(x) for x in v] for k, v in times.items()},
    "comparisons": compare,
    "device": torch.cuda.get_device_name(0),
}
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
