"""The schedules of batcher_model.py, checked on the host before they are replayed into a batcher
(test_batcher_lifecycle.py): each still contains the events it was written for, a mixed round still has the
shape that makes it worth launching, and the model agrees with a second derivation of every mixed round
(rc4_mixed_expect.py on the round laid out as one BRB_RC4_MixedListBatch call).  No GPU."""
import importlib.util
import os
import sys
from collections import Counter

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _sibling(name, file=None):
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, (file or name) + ".py"))
        sys.modules[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[name])
    return sys.modules[name]


BM = _sibling("batcher_model")
X = _sibling("rc4_mixed_expect")
RC4, RC4_MD5, READ, WRITE = BM.RC4, BM.RC4_MD5, BM.READ, BM.WRITE

IN_FLIGHT = ["enable_in_flight", "disable_in_flight", "enable_batch_in_flight", "enable_batch_algo_in_flight",
             "enable_algo_in_flight", "get_state_round_in_flight", "get_state_of_in_flight_conn", "empty_flush_async"]
ANY_BATCHER = ["read", "write", "flush", "flush_async", "enable", "enable_algo", "enable_batch", "enable_batch_algo",
               "disable", "get_state",
               "refused_disable", "refused_enable_algo", "refused_enable_batch_algo", "held_buffer_leaves_after_refusal",
               "read_refused_disabled", "write_refused_disabled", "get_state_zero", "round_without_buffers",
               "enable_brings_back", "enable_algo_brings_back"]
MIXED_ONLY = ["enable_algo_changes_algo_in_flight", "enable_changes_algo_in_flight", "enable_batch_algo_changes_algo_in_flight",
              "refused_enable", "refused_enable_batch"]


def _layout(m, r):
    """Round r of model m as the arguments of one mixed list call, the way plan_round_mixed sorts it: streams
    by kind, inside a kind by first appearance, a stream's buffers in submission order; the inputs and the
    outputs lie in submission order, as in the arenas.  -> dict of arrays, and per item its buffer index."""
    streams, in_off, out_off, at, oat = {}, [], [], 0, 0
    for i, b in enumerate(r.items):
        streams.setdefault((b.op, b.conn), []).append(i)
        in_off.append(at)
        out_off.append(oat)
        at += len(b.data)
        oat += len(b.data) + (BM.HDR if BM.kind_of(b) == BM.FRAME else 0)
    for ks in streams.values():
        assert len({r.items[i].algo for i in ks}) == 1                  # one algo per stream and round
    order = [s for kd in (BM.CRYPT, BM.FRAME, BM.OPEN) for s, ks in streams.items() if BM.kind_of(r.items[ks[0]]) == kd]
    pos, first = {}, [0]
    for s in order:
        for i in streams[s]:
            pos[i] = len(pos)
        first.append(len(pos))
    by_pos = sorted(pos, key=pos.get)
    return dict(order=order, pos=pos, total_out=oat,
                kinds=np.array([BM.kind_of(r.items[streams[s][0]]) for s in order], np.uint8),
                state_index=np.array([op * m.M + c for op, c in order], np.uint32),
                first=np.array(first, np.uint64),
                data=np.frombuffer(b"".join(b.data for b in r.items), np.uint8),
                offs=np.array([in_off[i] for i in by_pos], np.uint64),
                lens=np.array([len(r.items[i].data) for i in by_pos], np.uint32),
                ooffs=np.array([out_off[i] for i in by_pos], np.uint64),
                salts=np.array([r.items[i].salt for i in by_pos], np.uint64))


@pytest.mark.parametrize("family", ["rc4", "rc4_md5", "mixed"])
def test_schedule_contains_its_events(orc, family):
    """Every event the schedule was written for still happens, counted on the model of a pipelined batcher
    (where "in flight" is the round FlushAsync left running); the counts are printed."""
    steps = BM.steps_of("main", family)
    calls, m, census = BM.case(orc, "main", family, pipelined=True)
    assert len(calls) == len(steps)
    names = IN_FLIGHT + ANY_BATCHER + (MIXED_ONLY if family == "mixed" else [])
    life = sum(census[n] for n in ("enable", "enable_algo", "enable_batch", "enable_batch_algo", "disable"))
    print(f"\n{family}: {len(steps)} steps, {len(m.rounds)} rounds launched, {census['read'] + census['write']} buffers, "
          f"{life} life-cycle calls, {census['get_state']} get_state")
    print("   " + ", ".join(f"{n} {census[n]}" for n in names))
    assert [n for n in names if census[n] == 0] == []
    assert len(m.rounds) >= 8
    assert [n for n, _, w in calls if w == -1 and n not in ("read", "write")] == []     # no bad argument anywhere
    # in flight or not, the calls return the same: a batcher without the flag sees the same steps between rounds
    flat, m1, c1 = BM.case(orc, "main", family, pipelined=False)
    assert [(n, w) for n, _, w in flat if n not in ("flush", "flush_async")] == \
        [(n, w) for n, _, w in calls if n not in ("flush", "flush_async")]
    assert [n for n in ANY_BATCHER if c1[n] == 0] == []
    assert sorted(sum((w for n, _, w in flat if n.startswith("flush")), [])) == \
        sorted(sum((w for n, _, w in calls if n.startswith("flush")), []))
    if family != "mixed":                                               # the rc4_md5 family also runs on a mixed batcher
        as_mixed = BM.case(orc, "main", family, pipelined=True, mixed=True)[0]
        assert as_mixed == calls
    verdicts = Counter((BM.kind_of(b), res[3]) for r in m.rounds for b, res in zip(r.items, r.results))
    if family != "rc4":
        assert verdicts[BM.OPEN, 0] > 20 and verdicts[BM.OPEN, 1] > 200 and verdicts[BM.FRAME, 1] > 200
    if family != "rc4_md5":
        assert verdicts[BM.CRYPT, 1] > 200


def test_mixed_rounds_have_the_shape(orc):
    """The mixed family's rounds as the planner sorts them: one of five or more waves of 64 streams, waves of
    one kind beside waves with a kind boundary, an OPEN buffer beyond the first 64 whose verdict is 0, and a
    connection with buffers in one direction only."""
    _, m, _ = BM.case(orc, "main", "mixed", pipelined=True)
    most, census, late_bad_open, one_way = None, None, 0, 0
    for r in m.rounds:
        lay = _layout(m, r)
        kinds = lay["kinds"]
        waves = [sorted(set(kinds[w:w + 64].tolist())) for w in range(0, len(kinds), 64)]
        for i, b in enumerate(r.items):
            late_bad_open += BM.kind_of(b) == BM.OPEN and lay["pos"][i] >= 64 and r.results[i][3] == 0
        have = set(lay["order"])
        one_way += sum((READ, c) in have and (WRITE, c) not in have for c in range(BM.MAIN_CONNS))
        if most is None or len(waves) > len(most):
            most, census = waves, (len(kinds), len(r.items), Counter(kinds.tolist()))
    by_size = Counter(len(w) for w in most)
    print(f"\nlargest mixed round: {census[0]} streams ({dict(census[2])} by kind), {census[1]} buffers, {len(most)} waves: "
          f"{by_size[1]} of one kind, {by_size[2]} of two, {by_size[3]} of three; kinds per wave {most}")
    assert len(most) >= 5
    assert by_size[1] >= 1 and by_size[2] >= 1
    assert late_bad_open >= 1 and one_way >= 1


def test_every_part_of_three_gets_traffic_and_life_cycle(orc):
    """An all-devices batcher in 3 parts (connection c in part c % 3): every part launches rounds and receives
    traffic, life-cycle calls and refusals; what a call returns and what a connection sees do not depend on
    the number of parts."""
    for family in ("rc4", "rc4_md5", "mixed"):
        for pipelined in (False, True):
            _, m, census = BM.case(orc, "main", family, pipelined, parts=3)
            for g in range(3):
                assert census["part", g, "traffic"] > 100 and census["part", g, "life_cycle"] > 20, (family, g)
            assert {r.part for r in m.rounds} == {0, 1, 2}
            assert census["refused_disable"] and census["refused_enable_algo"] and census["refused_enable_batch_algo"]
    # in three parts the calls return what they return in one, and every connection sees the same results
    for family in ("rc4_md5", "mixed"):
        one, three = BM.case(orc, "main", family, True)[0], BM.case(orc, "main", family, True, parts=3)[0]
        assert [(n, w) for n, _, w in one if not n.startswith("flush")] == [(n, w) for n, _, w in three if not n.startswith("flush")]
        assert BM.by_conn(sum((w for n, _, w in one if n.startswith("flush")), [])) == \
            BM.by_conn(sum((w for n, _, w in three if n.startswith("flush")), []))


def test_model_equals_the_mixed_list_expectation(orc):
    """Every round of the mixed schedule, laid out as one BRB_RC4_MixedListBatch call over the table of read
    states then write states (state_index = op * max_conns + conn, kinds from the algo at submission):
    rc4_mixed_expect.py gives the model's outputs, verdicts and states."""
    _, m, _ = BM.case(orc, "main", "mixed", pipelined=True)
    assert len(m.rounds) >= 8
    for n, r in enumerate(m.rounds):
        lay = _layout(m, r)
        table = np.frombuffer(b"".join(r.before[READ] + r.before[WRITE]), np.uint8).reshape(2 * m.M, 264)
        valid = np.full(len(r.items), 0xEE, np.uint8)
        st, out, val = X.expect_mixed(orc, table, lay["kinds"], lay["data"], lay["offs"], lay["lens"], lay["ooffs"],
                                      lay["first"], np.zeros(lay["total_out"], np.uint8), lay["salts"], valid,
                                      lay["state_index"])
        assert st.tobytes() == b"".join(r.after[READ] + r.after[WRITE]), n
        for i, (b, (c, op, res, ok)) in enumerate(zip(r.items, r.results)):
            k = lay["pos"][i]
            o = int(lay["ooffs"][k])
            assert (c, op) == (b.conn, b.op) and out[o:o + len(res)].tobytes() == res, (n, i)
            assert len(res) == len(b.data) + (BM.HDR if BM.kind_of(b) == BM.FRAME else 0), (n, i)
            assert (int(val[k]) if BM.kind_of(b) == BM.OPEN else 1) == ok and (BM.kind_of(b) == BM.OPEN or val[k] == 0xEE), (n, i)


@pytest.mark.parametrize("family", ["rc4_md5", "mixed"])
def test_refusals_leave_the_model_unchanged(orc, family):
    """Every call of the schedules that the model answers with 0 or -1 leaves all of its state as it was."""
    seen = Counter()

    def watch(snap, m, name, want):
        if want in (0, -1) and not name.startswith("flush"):
            assert m.snapshot() == snap, name
            seen[name, want] += 1

    m = BM.Model(orc, BM.MAIN_MAX_CONNS, BM.MAIN_ROUND_BYTES, BM.family_algo(family), True, 1, family == "mixed")
    BM.trace(BM.steps_of("main", family), m, watch=watch)
    assert seen["disable", 0] and seen["enable_algo", 0] and seen["enable_batch_algo", 0] and seen["read", -1] and seen["write", -1]
    m = BM.Model(orc, BM.FULL_MAX_CONNS, BM.FULL_ROUND_BYTES, RC4_MD5, True)
    BM.trace(BM.full_schedule("rc4_md5"), m, watch=watch)
    assert seen["read", 0] == 1 and seen["write", 0] == 4


@pytest.mark.parametrize("pipelined", [False, True], ids=["flush", "pipelined"])
@pytest.mark.parametrize("family", ["rc4", "rc4_md5"])
def test_full_schedule_is_full(orc, family, pipelined):
    """The return codes of full_schedule(), spelled out: 12 buffers go in and the 13th does not, whatever its
    size; after a flush the same buffers do; a round takes exactly 4096 bytes, then only empty buffers."""
    calls, m, census = BM.case(orc, "full", family, pipelined)
    rc = [w for n, _, w in calls if n in ("read", "write")]
    assert rc == [1] * 12 + [0, 0, 0] + [1, 1] + [1, 1] + [1, 0, 1] + [0, 1, 1] + [1]
    sizes = [sum(len(b.data) for b in r.items) for r in m.rounds]
    assert [len(r.items) for r in m.rounds] == [12, 8, 1] and sizes[1:] == [4096, 1]
    twice = {}
    for n, a, w in calls:
        if n in ("read", "write"):
            twice.setdefault((n, a), []).append(w)
    assert [v for v in twice.values() if len(v) > 1] == [[0, 1]] * 3    # refused, then taken: the same bytes
    delivered = sum((w for n, _, w in calls if n.startswith("flush")), [])
    assert len(delivered) == 21 and all(ok == 1 for _, _, out, ok in delivered[:12])
    if family == "rc4_md5":                                             # a full round's frames are 30 bytes longer each
        assert sum(len(out) for c, op, out, ok in m.rounds[1].results) == 4096 + 30 * 5
    assert census["empty_flush_async" if pipelined else "round_without_buffers"] >= 1
