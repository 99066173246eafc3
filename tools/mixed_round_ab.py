"""One mixed launch against one launch per kind, on one GPU and in one process.

Device mode, kernels only (device events).  16 384 connections, one 1500-byte read and one 1500-byte write
each, the read and the write state of every connection in one table:

  RC4_MD5  A  BRB_RC4MD5_OpenListBatch over the reads, then BRB_RC4MD5_FrameListBatch over the writes
           B  one BRB_RC4_MixedListBatch, streams sorted by kind (every wave runs one body)
           B' the same call with kind = s % 2: connection c's write and read next to each other, so every
              wave runs both bodies -- the price of a divergent wave
  RC4      A  BRB_RC4_CryptListBatch over the reads, then over the writes (its default cooperative loads,
              and its per-lane loads)
           B  one BRB_RC4_MixedListBatch of 2 x 16 384 crypt streams

The transform batcher, zero-copy and pipelined, wall clock of FlushAsync + Flush (submission excluded):
A = BRB_BATCHER_CONN_LISTS, B = BRB_BATCHER_MIXED on the default algo, RC4_MD5, with one read and one write
per connection and with a ragged queue (seeded, below);
and half the connections RC4, half RC4_MD5: one mixed batcher against two conn_lists batchers flushed one
after the other.  (The ragged queue is §4.6a's 0 .. --ragged-max writes per connection with 0 .. 2 reads
beside them, since a round holds four buffers per connection on average.)

Before anything is timed, A and B run once from equal states and everything they leave is compared.  Then,
after a warm-up, A and B alternate round by round; median, minimum and maximum over the rounds are reported.

  python tools/mixed_round_ab.py [--conns 16384] [--bytes 1500] [--rounds 9] [--warmup 3] [--ragged-max 5] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

import brb_framework_amd as brb

ap = argparse.ArgumentParser()
ap.add_argument("--conns", type=int, default=16384)
ap.add_argument("--bytes", type=int, default=1500)
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
F = L + HDR
CRYPT, FRAME, OPEN = brb.RC4_KIND_CRYPT, brb.RC4_KIND_FRAME, brb.RC4_KIND_OPEN
rng = np.random.default_rng(0xAB116)
KEYS = [rng.integers(0, 256, 16, dtype=np.uint8).tobytes() for _ in range(N)]
HALF = brb.rc4_states(KEYS)
STATES0 = torch.from_numpy(np.concatenate([HALF, HALF])).cuda()      # write states, then read states


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


def alternate(legs):
    """legs: {name: closure}.  Warm-up, then the legs alternate round by round -> {name: stat}."""
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    t = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, fn in legs.items():
            t[name].append(timed(fn))
    torch.cuda.synchronize()
    brb.async_fault_check()
    return {name: stat(v) for name, v in t.items()}


# ---- device mode ---------------------------------------------------------------------------------
# One input buffer: the payloads to write at [0, N L), what was read at [R0, R0 + N F) (frames, or for RC4 N
# buffers of L bytes).  One output buffer: what was read is decrypted at the offsets it came in at (the list
# calls' out mirrors in), the writes' results lie behind, at [W0, ...).
i64 = np.arange(N, dtype=np.uint64)
R0 = (N * L + 255) // 256 * 256
W0 = (R0 + N * F + 255) // 256 * 256
IN_BYTES, OUT_BYTES = W0, W0 + N * F
kw = dict(async_=True)


def compare(what, runs):
    """Every leg once from equal states; everything it leaves must equal the first leg's."""
    ref = None
    for name, fn in runs.items():
        st, out, valid = STATES0.clone(), torch.zeros(OUT_BYTES, dtype=torch.uint8, device="cuda"), \
            torch.full((2 * N,), 0xA5, dtype=torch.uint8, device="cuda")
        got = fn(st, out, valid)
        torch.cuda.synchronize()
        brb.async_fault_check()
        if ref is None:
            ref = got
        else:
            for x, y in zip(ref, got):
                assert torch.equal(x, y), (what, name, "differs from the first leg")
    return ref


def device_rc4md5():
    payload = rng.integers(0, 256, N * L, dtype=np.uint8)
    inb = torch.zeros(IN_BYTES, dtype=torch.uint8, device="cuda")
    inb[:N * L] = torch.from_numpy(payload).cuda()
    n_p_offs, n_p_lens = i64 * L, np.full(N, L, np.uint32)
    n_r_offs, n_r_lens = R0 + i64 * F, np.full(N, F, np.uint32)
    n_w_offs, n_salts = W0 + i64 * F, i64 * 977
    p_offs, p_lens, r_offs, r_lens, w_offs, salts = (dev(x) for x in (n_p_offs, n_p_lens, n_r_offs, n_r_lens, n_w_offs, n_salts))
    first = dev(np.arange(N + 1, dtype=np.uint64))
    # what the peers sent: the frames of other payloads under the read states' keys
    peer = torch.from_numpy(HALF).cuda()
    other = torch.from_numpy(rng.integers(0, 256, N * L, dtype=np.uint8)).cuda()
    brb.rc4md5_frame_list_batch(peer, other, p_offs, p_lens, salts, inb, r_offs, first)
    # B: streams 0 .. N-1 frame (states 0 .. N-1), streams N .. 2N-1 open (states N .. 2N-1)
    b_kind = dev(np.array([FRAME] * N + [OPEN] * N, np.uint8))
    cat = lambda x, y: dev(np.concatenate([x, y]))
    b_offs, b_lens = cat(n_p_offs, n_r_offs), cat(n_p_lens, n_r_lens)
    b_ooffs, b_salts = cat(n_w_offs, n_r_offs), cat(n_salts, n_salts)
    b_first = dev(np.arange(2 * N + 1, dtype=np.uint64))
    b_index = dev(np.arange(2 * N, dtype=np.uint32))
    # B': stream 2c frames connection c's write, stream 2c + 1 opens its read
    il = lambda x, y: dev(np.stack([x, y], axis=1).reshape(-1))
    d_kind = dev(np.array([FRAME, OPEN] * N, np.uint8))
    d_offs, d_lens = il(n_p_offs, n_r_offs), il(n_p_lens, n_r_lens)
    d_ooffs, d_salts = il(n_w_offs, n_r_offs), il(n_salts, n_salts)
    d_index = dev(np.stack([np.arange(N), N + np.arange(N)], axis=1).reshape(-1).astype(np.uint32))

    def leg_a(st, out, valid):
        brb.rc4md5_open_list_batch(st[N:], inb, r_offs, r_lens, first, out=out, valid=valid[N:], **kw)
        brb.rc4md5_frame_list_batch(st[:N], inb, p_offs, p_lens, salts, out, w_offs, first, **kw)
        return st, out, valid[N:]

    def leg_b(st, out, valid):
        brb.rc4_mixed_list_batch(st, b_kind, inb, b_offs, b_lens, b_ooffs, b_first, out=out, salts=b_salts, valid=valid,
                                 state_index=b_index, **kw)
        return st, out, valid[N:]

    def leg_d(st, out, valid):
        brb.rc4_mixed_list_batch(st, d_kind, inb, d_offs, d_lens, d_ooffs, b_first, out=out, salts=d_salts, valid=valid,
                                 state_index=d_index, **kw)
        return st, out, valid[1::2].contiguous()

    ref = compare("rc4md5", {"A": leg_a, "B": leg_b, "B_divergent": leg_d})
    assert bool(ref[2].eq(1).all()), "the frames the peers sent must open valid"
    st, out = STATES0.clone(), torch.zeros(OUT_BYTES, dtype=torch.uint8, device="cuda")
    valid = torch.zeros(2 * N, dtype=torch.uint8, device="cuda")
    return alternate({"A_open_list_then_frame_list": lambda: leg_a(st, out, valid),
                      "B_mixed_sorted_by_kind": lambda: leg_b(st, out, valid),
                      "B_mixed_kind_s_mod_2": lambda: leg_d(st, out, valid)})


def device_rc4():
    inb = torch.from_numpy(rng.integers(0, 256, IN_BYTES, dtype=np.uint8)).cuda()
    n_p_offs, n_r_offs, n_w_offs, n_lens = i64 * L, R0 + i64 * L, W0 + i64 * L, np.full(N, L, np.uint32)
    p_offs, r_offs, lens = dev(n_p_offs), dev(n_r_offs), dev(n_lens)
    first = dev(np.arange(N + 1, dtype=np.uint64))
    b_kind = dev(np.full(2 * N, CRYPT, np.uint8))
    cat = lambda x, y: dev(np.concatenate([x, y]))
    b_offs, b_lens, b_ooffs = cat(n_p_offs, n_r_offs), cat(n_lens, n_lens), cat(n_w_offs, n_r_offs)
    b_first = dev(np.arange(2 * N + 1, dtype=np.uint64))
    b_index = dev(np.arange(2 * N, dtype=np.uint32))

    def leg_a(st, out, valid):
        # a crypt list call writes at its input offsets: the writes' results go behind the reads' through a
        # view of the output that starts at W0
        brb.rc4_crypt_list_batch(st[N:], inb, r_offs, lens, first, out=out, **kw)
        brb.rc4_crypt_list_batch(st[:N], inb, p_offs, lens, first, out=out[W0:], **kw)
        return st, out

    def leg_b(st, out, valid):
        brb.rc4_mixed_list_batch(st, b_kind, inb, b_offs, b_lens, b_ooffs, b_first, out=out, state_index=b_index, **kw)
        return st, out

    res = {}
    for coop in (1, 0):
        with brb.TestOption("rc4_list_coop", coop):
            compare("rc4", {"A": leg_a, "B": leg_b})
            st, out = STATES0.clone(), torch.zeros(OUT_BYTES, dtype=torch.uint8, device="cuda")
            t = alternate({"A": lambda: leg_a(st, out, None), "B": lambda: leg_b(st, out, None)})
        res["A_two_crypt_list_calls_" + ("cooperative_loads" if coop else "per_lane_loads")] = t["A"]
        res["B_mixed_beside_A_" + ("cooperative" if coop else "per_lane")] = t["B"]
    return res


# ---- the batcher ---------------------------------------------------------------------------------
DONE = brb.crypto.TransformDone


def make_batcher(flags, cap, algos=None, conns=None):
    h = Lb.BRB_TransformBatcherCreate(N, cap, flags | brb.BATCHER_ZERO_COPY | brb.BATCHER_PIPELINED)
    if not h:
        raise RuntimeError(Lb.BRB_CryptoGPU_LastError().decode())
    ids = np.arange(N, dtype=np.uint32) if conns is None else np.ascontiguousarray(conns, np.uint32)
    blob, offs, lens = brb.pack_keys([KEYS[c] for c in ids.tolist()])
    if algos is None:
        rc = Lb.BRB_TransformBatcherEnableBatch(h, ids.ctypes.data, len(ids), blob.ctypes.data, offs.ctypes.data, lens.ctypes.data)
    else:
        al = np.ascontiguousarray(algos, np.uint8)
        rc = Lb.BRB_TransformBatcherEnableBatchAlgo(h, ids.ctypes.data, len(ids), al.ctypes.data, blob.ctypes.data,
                                                    offs.ctypes.data, lens.ctypes.data)
    assert rc == 1, Lb.BRB_CryptoGPU_LastError()
    return h


def run_batcher(sides, reads, writes, rounds):
    """sides: {name: [(batcher, the connections it serves or None for all)]}: the batchers of a side are fed
    their connections' buffers and flushed one after the other.  reads / writes: buffers per connection.
    Wall clock of FlushAsync + Flush over a side's batchers; a first round with callbacks compares what the
    sides deliver."""
    k = int(max(reads.max(), writes.max(), 1))
    region = brb.crypto.HostRegion(2 * N * k * F)
    ctypes.memmove(region.addr, rng.integers(0, 256, 2 * N * k * F, dtype=np.uint8).tobytes(), 2 * N * k * F)
    w_base = region.addr + N * k * F
    total = int(reads.sum() + writes.sum())

    def submit(h, conns):
        n = 0
        for r in range(k):
            for c in (np.nonzero(reads > r)[0] if conns is None else [c for c in conns if reads[c] > r]):
                n += Lb.BRB_TransformBatcherRead(h, int(c), region.addr + (int(c) * k + r) * F, F) == 1
            for c in (np.nonzero(writes > r)[0] if conns is None else [c for c in conns if writes[c] > r]):
                n += Lb.BRB_TransformBatcherWrite(h, int(c), w_base + (int(c) * k + r) * F, L, int(c)) == 1
        return n

    def flush(side, cb):
        t0 = time.perf_counter()
        n = 0
        for h, _ in side:                               # a side's batchers one after the other
            n += Lb.BRB_TransformBatcherFlushAsync(h, cb, None)
            n += Lb.BRB_TransformBatcherFlush(h, cb, None)
        return (time.perf_counter() - t0) * 1e6, n

    seen = {}
    for name, side in sides.items():                    # what the sides deliver, per connection and direction
        got = {}
        cb = DONE(lambda _u, conn, op, out, n, valid: got.setdefault((conn, op), []).append(
            (zlib.crc32(ctypes.string_at(out, n)) if n else 0, n, valid)))
        assert sum(submit(h, conns) for h, conns in side) == total, Lb.BRB_CryptoGPU_LastError()
        _, n = flush(side, cb)
        assert n == total, (name, n, total, Lb.BRB_CryptoGPU_LastError())
        seen[name] = got
    first = next(iter(seen.values()))
    assert all(got == first for got in seen.values()), "the sides deliver different results"
    times = {name: [] for name in sides}
    for rnd in range(args.warmup + rounds):
        for name, side in sides.items():
            for h, conns in side:
                submit(h, conns)
            dt, n = flush(side, None)
            assert n == total, (name, n, total, Lb.BRB_CryptoGPU_LastError())
            if rnd >= args.warmup:
                times[name].append(dt)
    region.close()
    out = {name: stat(t) for name, t in times.items()}
    out["buffers"] = total
    return out


def batcher_lines():
    res = {}
    rounds = max(3, args.rounds // 2)
    ones = np.ones(N, np.int64)
    g = np.random.default_rng(0x4A66)
    # the ragged write queue of §4.6a (0 .. ragged-max per connection) with 0 .. 2 reads beside it: a round
    # holds at most 4 buffers per connection on average
    ragged_w, ragged_r = g.integers(0, args.ragged_max + 1, N), g.integers(0, 3, N)
    cap = int(max(N, ragged_w.sum() + ragged_r.sum())) * F
    a = make_batcher(brb.CRYPTO_FUNC_RC4_MD5 | brb.BATCHER_CONN_LISTS, cap)
    b = make_batcher(brb.CRYPTO_FUNC_RC4_MD5 | brb.BATCHER_MIXED, cap)
    sides = {"A_conn_lists": [(a, None)], "B_mixed": [(b, None)]}
    res["rc4md5_one_read_one_write"] = run_batcher(sides, ones, ones, rounds)
    print("batcher k=1:", res["rc4md5_one_read_one_write"], flush=True)
    res[f"rc4md5_ragged_0_{args.ragged_max}"] = run_batcher(sides, ragged_r, ragged_w, rounds)
    print("batcher ragged:", res[f"rc4md5_ragged_0_{args.ragged_max}"], flush=True)
    for h in (a, b):
        Lb.BRB_TransformBatcherDestroy(h)
    # half the connections RC4, half RC4_MD5 (alternating ids)
    algos = np.where(np.arange(N) % 2 == 0, brb.CRYPTO_FUNC_RC4, brb.CRYPTO_FUNC_RC4_MD5).astype(np.uint8)
    even, odd = np.arange(0, N, 2), np.arange(1, N, 2)
    cap = 2 * N * F
    a1 = make_batcher(brb.CRYPTO_FUNC_RC4 | brb.BATCHER_CONN_LISTS, cap, conns=even)
    a2 = make_batcher(brb.CRYPTO_FUNC_RC4_MD5 | brb.BATCHER_CONN_LISTS, cap, conns=odd)
    b = make_batcher(brb.CRYPTO_FUNC_RC4 | brb.BATCHER_MIXED, cap, algos=algos)
    sides = {"A_two_conn_lists_batchers": [(a1, even.tolist()), (a2, odd.tolist())], "B_one_mixed_batcher": [(b, None)]}
    res["half_rc4_half_rc4md5_one_read_one_write"] = run_batcher(sides, ones, ones, rounds)
    print("batcher half and half:", res["half_rc4_half_rc4md5_one_read_one_write"], flush=True)
    for h in (a1, a2, b):
        Lb.BRB_TransformBatcherDestroy(h)
    return res


result = {"shape": {"connections": N, "buffer_bytes": L, "per_connection": "one read and one write"}, "rounds": args.rounds,
          "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
result["device_mode_rc4md5"] = device_rc4md5()
print("device mode, RC4_MD5:", result["device_mode_rc4md5"], flush=True)
result["device_mode_rc4"] = device_rc4()
print("device mode, RC4:", result["device_mode_rc4"], flush=True)
torch.cuda.empty_cache()
result["batcher_zero_copy_pipelined"] = batcher_lines()
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
print(json.dumps(result))
