"""A host model of the transform batcher's life cycle and a generator of schedules for it
(test_batcher_model_cpu.py, test_batcher_lifecycle.py).

The model follows include/brb_crypto.h, "Receive-loop batching", not the batcher's code: what every call
returns, which round a buffer runs in, under which key and algo, what Flush / FlushAsync deliver and what
GetState shows.  Every byte comes from the oracle's scalar calls chained on the host.  A schedule is a
plain list of steps; trace() turns it, through a model, into the concrete calls with the result each must
give, and the same trace is replayed into every batcher.

A helper, not a test module: nothing here is collected by pytest and nothing touches a GPU."""
from collections import Counter, namedtuple

import numpy as np

RC4, RC4_MD5 = 1, 2
READ, WRITE = 0, 1
CRYPT, FRAME, OPEN = 0, 1, 2          # BRB_RC4_KIND_*, the order plan_round_mixed sorts a round's streams in
HDR = 30
ZERO = bytes(264)
LENS = [0, 1, 3, 29, 30, 31, 63, 64, 65, 200, 1500]
COUNTS = [0, 1, 1, 1, 2, 2, 2, 3, 3, 4]      # buffers per connection and direction: one stream in ten stays empty

Buf = namedtuple("Buf", "conn op data salt algo")
Round = namedtuple("Round", "part items before results after")


def kind_of(buf):
    return CRYPT if buf.algo != RC4_MD5 else FRAME if buf.op == WRITE else OPEN


class OutOfScope(Exception):
    """Plain Enable / EnableBatch over a pending buffer of a default-algo connection: the header does not say
    which key that buffer runs under, so no schedule may do it."""


class Model:
    """BRB_TransformBatcher on the host.  parts > 1: an all-devices batcher, connection c in part c % parts."""

    def __init__(self, orc, max_conns, max_round_bytes, algo, pipelined=False, parts=1, mixed=False):
        self.orc, self.M, self.cap, self.default = orc, max_conns, max_round_bytes, algo
        self.pipelined, self.G, self.mixed = pipelined, parts, mixed
        self.enabled = [False] * max_conns
        self.algo = [algo] * max_conns
        self.rd, self.wr = [ZERO] * max_conns, [ZERO] * max_conns       # ours
        self.peer_wr, self.peer_rd = [ZERO] * max_conns, [ZERO] * max_conns
        self.filling = [[] for _ in range(parts)]
        self.in_flight = [None] * parts                                 # pipelined: the Round FlushAsync left running
        self.rounds = []                                                # every Round launched, in launch order
        self.last_wire = {}
        self.disabled = set()                                           # turned off by Disable, not back yet

    # ---- what a test may look at
    def pending(self, conn):
        return any(b.conn == conn for b in self.filling[conn % self.G])

    def flying(self, conn):
        r = self.in_flight[conn % self.G]
        return r is not None and any(b.conn == conn for b in r.items)

    def snapshot(self):
        return (list(self.enabled), list(self.algo), list(self.rd), list(self.wr), list(self.peer_wr), list(self.peer_rd),
                [list(f) for f in self.filling], list(self.in_flight), len(self.rounds))

    def part_items(self, g):
        """A round of part g holds 4 buffers per connection of the part."""
        return 4 * ((self.M - g + self.G - 1) // self.G)

    # ---- the peer's side
    def wire(self, conn, payload, salt, spoil=None):
        """What the peer sends for `payload` under the connection's key and algo as they are now."""
        orc = self.orc
        if not self.enabled[conn]:
            w = payload                                                 # no key on either side: never accepted
        elif self.algo[conn] == RC4:
            self.peer_wr[conn], w = orc.rc4_crypt(self.peer_wr[conn], payload)
        elif spoil == "stub":
            self.peer_wr[conn], w = orc.rc4_crypt(self.peer_wr[conn], payload[:29])      # no frame at all
        else:
            self.peer_wr[conn], w = orc.rc4md5_frame(self.peer_wr[conn], payload, salt)
            if spoil == "bit":
                w = bytearray(w)
                w[8 + salt % (len(w) - 8)] ^= 2
                w = bytes(w)
        self.last_wire[conn] = w
        return w

    # ---- the API
    def _submit(self, conn, op, data, salt):
        if not self.enabled[conn]:
            return -1
        g = conn % self.G
        f = self.filling[g]
        if len(f) >= self.part_items(g) or sum(len(b.data) for b in f) + len(data) > self.cap:
            return 0
        f.append(Buf(conn, op, bytes(data), salt, self.algo[conn]))
        return 1

    def read(self, conn, data):
        return self._submit(conn, READ, data, 0)

    def write(self, conn, data, salt):
        return self._submit(conn, WRITE, data, salt)

    def _key(self, conn, key, algo):
        self.rd[conn] = self.wr[conn] = self.peer_wr[conn] = self.peer_rd[conn] = self.orc.rc4_init(key)
        self.algo[conn], self.enabled[conn] = algo, True
        self.disabled.discard(conn)

    def _back_to_default(self, conns):
        """Enable / EnableBatch: 0 for a connection of another algo than the default with a buffer waiting."""
        if self.mixed and any(self.algo[c] != self.default and self.pending(c) for c in conns):
            return False
        if any(self.pending(c) for c in conns):
            raise OutOfScope(conns)
        return True

    def enable(self, conn, key):
        if not self._back_to_default([conn]):
            return 0
        self._key(conn, key, self.default)
        return 1

    def enable_algo(self, conn, algo, key):
        if algo not in (RC4, RC4_MD5) or (not self.mixed and algo != self.default):
            return -1
        if self.pending(conn):
            return 0
        self._key(conn, key, algo)
        return 1

    def enable_batch(self, conns, keys):
        if len(set(conns)) != len(conns):                               # two lanes would write one state
            return -1
        if not self._back_to_default(conns):
            return 0
        for c, k in zip(conns, keys):
            self._key(c, k, self.default)
        return 1

    def enable_batch_algo(self, conns, algos, keys):
        if len(set(conns)) != len(conns) or any(a not in (RC4, RC4_MD5) or (not self.mixed and a != self.default)
                                                for a in algos):
            return -1
        if any(self.pending(c) for c in conns):
            return 0
        for c, a, k in zip(conns, algos, keys):
            self._key(c, k, a)
        return 1

    def disable(self, conn):
        if self.pending(conn):
            return 0
        self.enabled[conn] = False
        self.rd[conn] = self.wr[conn] = ZERO
        self.disabled.add(conn)
        return 1

    def get_state(self, conn, op):
        return (self.rd, self.wr)[op][conn]

    def _launch(self, g):
        """The filling round of part g leaves: its buffers run now, in submission order, on the states as
        they are, each under the algo it was submitted with."""
        items, self.filling[g] = self.filling[g], []
        if not items:
            return None
        orc, before, results = self.orc, (list(self.rd), list(self.wr)), []
        for b in items:
            c = b.conn
            if b.op == READ:
                if b.algo == RC4:
                    self.rd[c], out = orc.rc4_crypt(self.rd[c], b.data)
                    ok = 1
                else:
                    self.rd[c], out, ok = orc.rc4md5_open(self.rd[c], b.data)
            else:                                                       # the peer reads what we write
                if b.algo == RC4:
                    self.wr[c], out = orc.rc4_crypt(self.wr[c], b.data)
                    self.peer_rd[c], back = orc.rc4_crypt(self.peer_rd[c], out)
                    assert back == b.data
                else:
                    self.wr[c], out = orc.rc4md5_frame(self.wr[c], b.data, b.salt)
                    self.peer_rd[c], back, good = orc.rc4md5_open(self.peer_rd[c], out)
                    assert good == 1 and back[HDR:] == b.data and len(out) == len(b.data) + HDR
                ok = 1
            results.append((c, b.op, out, ok))
        r = Round(g, items, before, results, (list(self.rd), list(self.wr)))
        self.rounds.append(r)
        return r

    def flush_async(self):
        if not self.pipelined:
            return self.flush()
        out = []
        launched = [self._launch(g) for g in range(self.G)]             # every part's round is started first
        for g in range(self.G):
            if self.in_flight[g] is not None:
                out += self.in_flight[g].results
            self.in_flight[g] = launched[g]
        return out

    def flush(self):
        out = []
        for g in range(self.G):
            if self.in_flight[g] is not None:
                out += self.in_flight[g].results
                self.in_flight[g] = None
        for r in [self._launch(g) for g in range(self.G)]:
            if r is not None:
                out += r.results
        return out


def by_conn(results):
    """All-devices batchers deliver part by part: results per connection and direction, in order."""
    d = {}
    for c, op, out, valid in results:
        d.setdefault((c, op), []).append((out, valid))
    return d


# ---- steps -> calls -----------------------------------------------------------------------------
# A step:  ("read", conn, payload, salt, spoil)   ("reread", conn): the wire bytes sent last, once more
#          ("write", conn, payload, salt)          ("flush",)  ("flush_async",)
#          ("enable", conn, key)                   ("enable_algo", conn, algo, key)
#          ("enable_batch", conns, keys)           ("enable_batch_algo", conns, algos, keys)
#          ("disable", conn)                       ("get_state", conn, op)
# A call: (name, args, want) -- for a read the args hold the wire bytes.

def _events(m, step, want, held):
    """The names under which test_batcher_model_cpu.py counts a step; m is the model before the step."""
    name = step[0]
    ev = [name]
    listed = [step[1]] if name in ("enable", "enable_algo", "disable") else \
        list(step[1]) if name in ("enable_batch", "enable_batch_algo") else []
    if listed:
        if want == 0:
            ev.append("refused_" + name)
            held.update(c for c in listed if m.pending(c))
        elif want == 1:
            if any(m.flying(c) for c in listed):
                ev.append(name + "_in_flight")
            if name != "disable" and any(c in m.disabled for c in listed):
                ev.append(name + "_brings_back")
            new = [m.default] * len(listed) if name in ("enable", "enable_batch") else \
                [step[2]] if name == "enable_algo" else list(step[2]) if name == "enable_batch_algo" else []
            if any(m.flying(c) and m.algo[c] != a for c, a in zip(listed, new)):
                ev.append(name + "_changes_algo_in_flight")
        for c in listed:
            ev.append(("part", c % m.G, "life_cycle"))
    elif name in ("read", "reread", "write"):
        if want == -1:
            ev.append(name + "_refused_disabled")
        elif want == 0:
            ev.append(name + "_refused_full")
        else:
            ev.append(("part", step[1] % m.G, "traffic"))
    elif name == "get_state":
        if any(r is not None for r in m.in_flight):
            ev.append("get_state_round_in_flight")
        if m.flying(step[1]):
            ev.append("get_state_of_in_flight_conn")
        if want == ZERO and step[1] in m.disabled:
            ev.append("get_state_zero")
    else:
        filling, flying = any(m.filling), any(r is not None for r in m.in_flight)
        if not filling:
            ev.append("empty_" + name if flying else "round_without_buffers")
        if any(b.conn in held for f in m.filling for b in f):
            ev.append("held_buffer_leaves_after_refusal")
            held.clear()
    return ev


def trace(steps, model, census=None, watch=None):
    """Runs the steps through the model -> the calls [(name, args, want)].  census: a Counter of _events.
    watch(snapshot before the call, model, name, want) is called after every call."""
    calls, held = [], set()
    for step in steps:
        name = step[0]
        before = Model.__new__(Model)
        if census is not None:                                          # a view of the model before the step
            before.__dict__.update({k: (type(v)(v) if isinstance(v, (list, set, dict)) else v)
                                    for k, v in model.__dict__.items()})
            before.filling = [list(f) for f in model.filling]
        if name == "read":
            args = (step[1], model.wire(*step[1:]))
        elif name == "reread":
            name, args = "read", (step[1], model.last_wire[step[1]])
        else:
            args = tuple(step[1:])
        snap = model.snapshot() if watch is not None else None
        want = getattr(model, name)(*args)
        calls.append((name, args, want))
        if census is not None:
            census.update(_events(before, step, want, held))
        if watch is not None:
            watch(snap, model, name, want)
    return calls


# ---- the cases both test files run -----------------------------------------------------------------
SEED = 0x11FE
MAIN_CONNS = 150
# connections 150 .. 319 are never enabled; a round of 150 connections holds up to 1200 buffers (4 per connection
# and direction), and an all-devices part of 320 / 3 connections up to 428 >= the 400 its 50 connections can bring
MAIN_MAX_CONNS = 320
MAIN_ROUND_BYTES = 4 << 20
FULL_MAX_CONNS, FULL_ROUND_BYTES = 3, 4096
_steps, _cases = {}, {}


def steps_of(which, family):
    if (which, family) not in _steps:
        _steps[which, family] = schedule(SEED, family, MAIN_CONNS) if which == "main" else full_schedule(family)
    return _steps[which, family]


def case(orc, which, family, pipelined, parts=1, mixed=None):
    """The model's run of a schedule, computed once -> (calls, model, census).  which: "main" or "full";
    mixed: the batcher's flag (default: the mixed family's batchers have it)."""
    mixed = family == "mixed" if mixed is None else mixed
    key = (which, family, pipelined, parts, mixed)
    if key not in _cases:
        size = (MAIN_MAX_CONNS, MAIN_ROUND_BYTES) if which == "main" else (FULL_MAX_CONNS, FULL_ROUND_BYTES)
        m = Model(orc, *size, family_algo(family), pipelined, parts, mixed)
        census = Counter()
        _cases[key] = (trace(steps_of(which, family), m, census), m, census)
    return _cases[key]


# ---- schedules -----------------------------------------------------------------------------------

def family_algo(family):
    """The algo a batcher for this family is created with (mixed: the default Enable gives)."""
    return RC4_MD5 if family == "rc4_md5" else RC4


def schedule(seed, family, C=150, rounds=8):
    """`rounds` rounds of an event loop over C connections with the life cycle running beside the traffic.
    Steps between a round's flush_async and the next round's first buffer find that round in flight on a
    pipelined batcher and delivered on any other."""
    rng = np.random.default_rng([seed, 0xBA7C4])
    default = family_algo(family)
    mixed = family == "mixed"
    steps = []
    algo, enabled, pending, flying, gone = {}, set(), set(), set(), []

    def key():
        return rng.integers(0, 256, int(rng.integers(4, 32)), dtype=np.uint8).tobytes()

    def pick(pool, n):
        pool = sorted(pool)
        return [pool[i] for i in rng.permutation(len(pool))[:n]]

    def an_algo(c=None, flip=False):
        if not mixed:
            return default
        return (RC4 + RC4_MD5 - algo[c]) if flip else int(rng.choice([RC4, RC4_MD5]))

    def states(conns):
        for c in conns:
            steps.extend([("get_state", c, READ), ("get_state", c, WRITE)])

    def keyed(conns, algos):
        for c, a in zip(conns, algos):
            algo[c] = a
            enabled.add(c)
            if c in gone:
                gone.remove(c)

    def life_cycle(touched):
        """With nothing in the filling round: every call goes through."""
        for c in pick(flying & enabled, 6):                             # a new key behind the round
            steps.append(("enable", c, key()))
            keyed([c], [default])
            touched.add(c)
        for c in pick(flying & enabled - touched, 6):                   # mixed: the other algo behind the round
            a = an_algo(c, flip=True)
            steps.append(("enable_algo", c, a, key()))
            keyed([c], [a])
            touched.add(c)
        back = pick(gone, max(len(gone) - 4, 0))                        # some of those disabled earlier come back
        for c in pick(flying & enabled - touched, 6):
            steps.append(("disable", c))
            enabled.discard(c)
            gone.append(c)
            touched.add(c)
        states(pick(gone, 2))
        for i, c in enumerate(back):
            a = an_algo()
            steps.append(("enable_algo", c, a, key()) if i % 2 else ("enable", c, key()))
            keyed([c], [a if i % 2 else default])
            touched.add(c)
        if gone:                                                        # off and on again behind the same round
            c = gone[-1]
            steps.append(("enable", c, key()))
            keyed([c], [default])
        for with_algo in (False, True):
            conns = pick((flying | set(gone[:1])) - touched, 8)
            conns += pick(set(range(C)) - flying - touched - set(conns), 12)
            conns = [conns[i] for i in rng.permutation(len(conns))]
            algos = [an_algo() for _ in conns] if with_algo else [default] * len(conns)
            ks = [key() for _ in conns]
            steps.append(("enable_batch_algo", conns, algos, ks) if with_algo else ("enable_batch", conns, ks))
            keyed(conns, algos)
            touched.update(conns)

    def refusals(touched):
        """With buffers in the filling round: each call that names one of their connections returns 0."""
        free = set(range(C)) - pending
        c = pick(pending, 1)[0]
        steps.append(("disable", c))
        steps.append(("enable_algo", c, an_algo(c, flip=True), key()))
        conns = pick(pending, 2) + pick(free & enabled, 6)
        steps.append(("enable_batch_algo", conns, [an_algo() for _ in conns], [key() for _ in conns]))
        touched.update([c] + conns)
        other = [p for p in sorted(pending) if algo[p] != default]
        if other:                                                       # a mixed batcher: Enable is EnableAlgo(default)
            conns = other[:1] + pick(free & enabled, 5)
            steps.append(("enable", other[0], key()))
            steps.append(("enable_batch", conns, [key() for _ in conns]))
            touched.update(conns)
        c = pick(free & enabled, 1)[0]                                  # no buffer of its own in the round: it goes,
        steps.append(("disable", c))                                    # and what the round still brings for it is refused
        enabled.discard(c)
        gone.append(c)
        touched.add(c)

    conns = list(range(C))
    algos = [an_algo() for _ in conns]
    ks = [key() for _ in conns]
    steps.append(("enable_batch_algo", conns, algos, ks) if mixed else ("enable_batch", conns, ks))
    keyed(conns, algos)
    states([0, C - 1])
    steps.extend([("read", C, b"never enabled", 0, None), ("write", C, b"never enabled", 0)])
    for r in range(rounds):
        touched = set()
        todo = [(c, op) for c in range(C) for op in (READ, WRITE) for _ in range(int(rng.choice(COUNTS)))]
        for i, t in enumerate(rng.permutation(len(todo))):
            c, op = todo[t]
            payload = rng.integers(0, 256, int(rng.choice(LENS)), dtype=np.uint8).tobytes()
            salt = int(rng.integers(0, 2**32))
            if op == READ:
                spoil = [None, "stub", "bit"][int(rng.choice([0] * 8 + [1, 2]))]
                steps.append(("read", c, payload, salt, spoil))
            else:
                steps.append(("write", c, payload, salt))
            if c in enabled:
                pending.add(c)
            if i == 40:
                refusals(touched)
                states(sorted(touched))
        last = r == rounds - 1
        steps.append(("flush",) if r == 3 or last else ("flush_async",))
        flying, pending = pending, set()
        states(pick(flying, 3))                                         # untouched, its round in flight
        life_cycle(touched)
        states(sorted(touched | set(range(r % 7, C, 7))))
        if r == 4:                                                      # a round that no buffer enters
            steps.extend([("flush_async",), ("flush_async",), ("flush",)])
            flying = set()
            life_cycle(touched)
            states(sorted(touched))
    steps.append(("flush",))
    states(range(C))
    return steps


def full_schedule(family):
    """Rounds filled to the brim on a batcher of 3 connections and 4096 bytes: 12 buffers, then 4096 bytes."""
    assert family in ("rc4", "rc4_md5")
    rng = np.random.default_rng([0xF011, family_algo(family)])
    grow = HDR if family == "rc4_md5" else 0                            # a framed read is 30 bytes longer on the wire

    def data(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    steps = [("enable_batch", [0, 1, 2], [b"full key 0", b"full key one", b"k2"])]
    for i in range(12):                                                 # exactly 4 * max_conns buffers
        c, n = i % 3, [5, 40, 0, 31, 64, 7][i % 6]
        steps.append(("read", c, data(n), 100 + i, None) if i % 4 < 2 else ("write", c, data(n), 100 + i))
    late = ("write", 1, data(10), 8)
    steps += [("read", 2, data(33), 7, None), late, ("write", 0, b"", 9)]                # the 13th: 0, whatever its size
    steps += [("get_state", 2, READ), ("flush_async",), ("reread", 2), late]             # the same buffers: 1
    used = 33 + grow + 10
    steps += [("write", 0, data(1500), 1), ("read", 1, data(1500 - grow), 2, None)]
    used += 3000
    steps += [("write", 2, data(4096 - used - 1), 3), ("write", 2, data(2), 4), ("write", 2, data(1), 5)]   # 4095; 4097: 0; 4096
    one_more = ("write", 0, data(1), 6)
    steps += [one_more, ("read", 0, b"", 0, "stub"), ("write", 1, b"", 11)]              # full; empty ones still go in
    steps += [("flush",), one_more, ("flush_async",), ("flush_async",)]
    steps += [("get_state", c, op) for c in range(3) for op in (READ, WRITE)]
    return steps
