"""Graph capture and replay of the device-mode BRB_BATCH_ASYNC batch calls (include/brb_crypto.h, "Graph
capture"), every comparison bit for bit against the oracle.

Preconditions, as the header states them: only BRB_BATCH_DEVICE | BRB_BATCH_ASYNC calls are captured; each
kernel has run once eagerly before its first capture (here: one warm-up call on a separate set of buffers
under the same test options); the capture is one chain on one stream, under torch's default
capture_error_mode "global", so a call that allocates, synchronises or copies would fail it.

What is checked (tests/graph_cases.py holds the scenarios and the runner): counts, pointers, the route and
the test options are fixed at capture; everything in device memory -- data bytes, offsets, lengths, segment
and buffer lists, salts, `final` masks, RC4 states and streaming contexts -- is read afresh by each of three
replays, whose inputs are rewritten in place in between.  Stateless calls keep guard rows and fill bytes
around their outputs; for stateful calls replay k equals the oracle applied k times, all 264 bytes of every
state and the defined part of every context.  The capture runs on a thread new to the library, so whatever
the library sets up on a thread's first call happens inside the capture; the replays run on the main thread.

The shapes are the smallest at which the kernels still take their real routes; a case moves well under
1 MiB.  No wrapper had to be bypassed: with explicit outputs none of them reads device memory back.
"""
import importlib.util
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _sibling(name):
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
        sys.modules[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[name])
    return sys.modules[name]


G = _sibling("graph_cases")


@pytest.fixture(scope="module")
def torch_dev(brb):
    import torch
    assert torch.cuda.is_available(), "no HIP device visible to torch"
    assert brb.gpu_available(), brb.lib().BRB_CryptoGPU_LastError()
    return torch


def _fixed(alg, rec_len, n, base, line):
    def make(brb, orc):
        return G.FixedDigest(brb, orc, alg, rec_len, n, base, route=brb.FIXED_ROUTE_LINE if line else None)
    return make


def _of(cls, *args):
    return lambda brb, orc: cls(brb, orc, *args)


STATELESS = {
    # fixed-stride digests: the line kernel, the 64-byte kernel, byte-aligned short records
    "md5_fixed-1500": _fixed("md5", 1500, 130, 4, True), "sha1_fixed-1500": _fixed("sha1", 1500, 130, 4, True),
    "md5_fixed-64": _fixed("md5", 64, 65, 0, False), "sha1_fixed-64": _fixed("sha1", 64, 65, 0, False),
    "md5_fixed-77": _fixed("md5", 77, 130, 1, False), "sha1_fixed-77": _fixed("sha1", 77, 130, 1, False),
    "md5_batch-var_line1": _of(G.VarDigest, "md5", 1), "md5_batch-var_line0": _of(G.VarDigest, "md5", 0),
    "sha1_batch-var_line1": _of(G.VarDigest, "sha1", 1), "sha1_batch-var_line0": _of(G.VarDigest, "sha1", 0),
    "md5_lower_text": _of(G.LowerText),
    "md5_segments-seg_line2": _of(G.Segments, 2), "md5_segments-seg_line1": _of(G.Segments, 1),
    "md5_segments-seg_line0": _of(G.Segments, 0),
    "metadata_unpack-seg_line2": _of(G.MetaUnpack, 2), "metadata_unpack-seg_line0": _of(G.MetaUnpack, 0),
    "metadata_unpack_items-seg_line2": _of(G.MetaUnpackItems, 2), "metadata_unpack_items-seg_line0": _of(G.MetaUnpackItems, 0),
    "metadata_pack": _of(G.MetaPack),
    "base64_encode": _of(G.Base64Encode), "base64_decode": _of(G.Base64Decode),
    "blowfish_encrypt": _of(G.Blowfish, False), "blowfish_decrypt": _of(G.Blowfish, True),
    "blowfish_encrypt_keyed": _of(G.BlowfishKeyed, False), "blowfish_decrypt_keyed": _of(G.BlowfishKeyed, True),
    "rc4_init": _of(G.KeySetup, "rc4"), "blowfish_init": _of(G.KeySetup, "blowfish"),
    # the streaming calls that hold no state across replays (UpdateBatch and the segment calls are below)
    "md5_stream_init": _of(G.StreamInit, "md5"), "sha1_stream_init": _of(G.StreamInit, "sha1"),
    "md5_stream_final": _of(G.StreamFinal, "md5"), "sha1_stream_final": _of(G.StreamFinal, "sha1"),
}


@pytest.mark.parametrize("name", list(STATELESS))
def test_stateless_call_replays(brb, orc, torch_dev, name):
    """One graph per call; three replays on rewritten inputs; outputs, guard rows and fill bytes against the
    oracle, inputs unchanged."""
    G.run_case(brb, torch_dev, STATELESS[name](brb, orc))


def test_fixed_digest_shapes_take_three_routes(brb):
    """The three fixed-stride shapes above are three kernels (the route is a host function of the address's
    low bits and the record length; a device allocation is at least 256-byte aligned)."""
    routes = [brb.fixed_route(4096 + base, rec_len) for rec_len, base in ((1500, 4), (64, 0), (77, 1))]
    assert routes[0] == brb.FIXED_ROUTE_LINE and len(set(routes)) == 3


@pytest.mark.parametrize("pair", [1, 0], ids=["pair", "single"])
@pytest.mark.parametrize("kind", ["crypt", "frame", "open"])
def test_rc4_replays_carry_state(brb, orc, torch_dev, kind, pair):
    """rc4_crypt_batch, rc4md5_frame_batch, rc4md5_open_batch: 130 streams, lengths redrawn from {0, 1, 63, 64,
    65, 255, 256, 257, 700} at byte offsets; outputs, valid flags and whole states after every replay, the
    states being those of the oracle run as often."""
    cls = {"crypt": G.Rc4Crypt, "frame": G.Rc4Frame, "open": G.Rc4Open}[kind]
    G.run_case(brb, torch_dev, cls(brb, orc, pair))


@pytest.mark.parametrize("coop", [1, 0], ids=["coop", "lane"])
@pytest.mark.parametrize("kind", ["crypt", "frame", "open"])
def test_rc4_list_replays_carry_state(brb, orc, torch_dev, kind, coop):
    """The three RC4 list calls: 66 streams of 0..4 buffers, some with none, the lists themselves redrawn."""
    G.run_case(brb, torch_dev, G.Rc4List(brb, orc, kind, coop))


@pytest.mark.parametrize("alg", ["md5", "sha1"])
def test_stream_update_replays_then_final(brb, torch_dev, alg):
    """One graph holding UpdateBatch for 130 contexts, replayed three times on fresh pieces of 0..200 bytes, then
    one eager FinalBatch: the contexts after every replay and the digests against the host compat calls, the
    digests against hashlib of everything a context took as well."""
    G.run_case(brb, torch_dev, G.StreamUpdate(brb, alg))


@pytest.mark.parametrize("variant", ["md5", "sha1", "md5_lower"])
def test_stream_segments_replays_move_the_final_mask(brb, torch_dev, variant):
    """UpdateSegmentsBatch and the lower-text variant: one graph, three replays, the `final` mask (device memory)
    finalising a different third of the items each time."""
    G.run_case(brb, torch_dev, G.StreamSegments(brb, variant.split("_")[0], lower=variant.endswith("lower")))


# ---- whose fault word a captured wave-pair call reports into ---------------------------------------------
def _checks(brb, times):
    out = []
    for _ in range(times):
        try:
            brb.async_fault_check()
            out.append("clean")
        except RuntimeError as e:
            out.append(str(e))
    return out


def _load(torch, dev, arrays):
    for name, a in arrays.items():
        dev[name].copy_(G.as_torch(torch, a))
    torch.cuda.synchronize()


def test_fault_report_of_a_captured_call(brb, orc, torch_dev):
    """The library's injected protocol fault (pair_stall: the kernel ends normally and sets the word) under a
    graph.  A thread that has made no call yet captures rc4_crypt_batch with the stall, so its async fault
    word is allocated inside the capture; it replays once and synchronises: its async_fault_check() raises
    the -4 report and the next one is clean -- the word a capture allocates is armed.  The same call captured
    without the stall then replays to the oracle's bytes and leaves the check clean."""
    torch = torch_dev
    case = G.Rc4Crypt(brb, orc, 1)
    stream = torch.cuda.Stream()
    first = case.inputs(0, {})
    dev = {name: G.as_torch(torch, a).cuda() for name, a in first.items()}
    warm = {name: G.as_torch(torch, a).cuda() for name, a in case.inputs(G.WARM, {}).items()}
    torch.cuda.synchronize()
    brb.async_fault_check()
    worker = G.CaptureThread()
    try:
        with brb.TestOption("rc4_pair", 1):
            with brb.TestOption("pair_stall", 1):
                case.call(warm, stream)                    # the stalling kernel's eager run, on this thread
                stream.synchronize()
                assert "returned -4" in _checks(brb, 1)[0]

                def stalled():
                    graph, err = G.capture(torch, brb, stream, lambda: case.call(dev, stream))
                    if graph is None:
                        return err, None
                    graph.replay()
                    torch.cuda.synchronize()
                    return None, _checks(brb, 2)

                err, reports = worker.run(stalled)
            assert err is None, f"the capture failed: {err}"
            assert "AsyncFaultCheck returned -4: wave-pair protocol fault" in reports[0], reports
            assert reports[1] == "clean"
            assert _checks(brb, 1) == ["clean"]             # the report was the capturing thread's alone
            case.call(warm, stream)                        # the clean kernel's eager run
            stream.synchronize()
            _load(torch, dev, first)                       # the stalled replay left wrong states and outputs

            def clean():
                graph, err = G.capture(torch, brb, stream, lambda: case.call(dev, stream))
                if graph is None:
                    return err, None
                graph.replay()
                torch.cuda.synchronize()
                return None, _checks(brb, 1)

            err, reports = worker.run(clean)
            assert err is None, f"the capture failed: {err}"
            assert reports == ["clean"] and _checks(brb, 1) == ["clean"]
        want = case.expect({name: np.array(a) for name, a in first.items()})
        for name, w in want.items():
            G.differs(name, dev[name].cpu().numpy().view(w.dtype).reshape(w.shape), w, 0)
    finally:
        torch.cuda.synchronize()
        worker.close()


def test_replays_report_to_the_capturing_thread(brb, orc, torch_dev):
    """What the capturing thread owns.  Thread A captures a clean wave-pair call and stays alive; the main
    thread replays it: the results are the oracle's and the main thread's async_fault_check() is clean.

    The rule (include/brb_crypto.h, "Graph capture"): a captured wave-pair call reports into the async fault
    word of the thread that captured it, whichever thread replays the graph.  So the capturing thread is the
    one that calls BRB_CryptoGPU_AsyncFaultCheck() after a replay has been synchronised (as thread A does here,
    and as the stalled replay of test_fault_report_of_a_captured_call shows with a report), a replaying
    thread's own check says nothing about the replay, and thread A neither exits nor calls
    BRB_CryptoGPU_ThreadCleanup() while the graph can still be replayed."""
    torch = torch_dev
    case = G.Rc4Open(brb, orc, 1)
    stream = torch.cuda.Stream()
    first = {name: np.array(a) for name, a in case.inputs(0, {}).items()}
    dev = {name: G.as_torch(torch, a).cuda() for name, a in first.items()}
    warm = {name: G.as_torch(torch, a).cuda() for name, a in case.inputs(G.WARM, {}).items()}
    torch.cuda.synchronize()
    a = G.CaptureThread()
    try:
        with brb.TestOption("rc4md5_pair", 1):
            case.call(warm, stream)
            stream.synchronize()
            brb.async_fault_check()
            graph, err = a.run(lambda: G.capture(torch, brb, stream, lambda: case.call(dev, stream)))
            assert graph is not None, f"the capture failed: {err}"
            graph.replay()                                 # on the main thread; A is alive and idle
            torch.cuda.synchronize()
        assert _checks(brb, 1) == ["clean"]
        assert a.run(lambda: _checks(brb, 1)) == ["clean"]
        for name, w in case.expect(first).items():
            G.differs(name, dev[name].cpu().numpy().view(w.dtype).reshape(w.shape), w, 0)
    finally:
        torch.cuda.synchronize()
        a.close()
