// round_plan.h -- a transform-batcher round's groups and the image of its metadata, as plain C++.
//
// No HIP and no api_util.h here: tests/c/round_plan_check.cpp builds this header on its own, with
// ASan and UBSan, and checks it against a naive model (tests/test_round_plan_cpu.py).
//
// A group is one kernel launch.  Its metadata: sidx u32[streams], with connection lists first
// u64[streams + 1], then per buffer offs u64[], lens u32[], ooffs u64[], salts u64[], every array
// 8-byte aligned.  Without connection lists a group is one (sub-round, direction), each of its
// buffers a stream of its own; with them it is one direction, its streams in order of first
// appearance and stream i's buffers first[i] .. first[i + 1] - 1 in submission order.  Groups come in
// key order -- 2 * sub-round + op, with lists op -- so READ before WRITE; empty ones are skipped.
//
// The mixed layout (plan_round_mixed, BRB_BATCHER_MIXED) is one group for the whole round: every
// (direction, connection) is a stream of the mixed kernel, with its kind in kind u8[streams] behind
// first.  Streams are sorted by kind (a wave whose lanes agree runs one body), inside a kind in order
// of first appearance; stream i's buffers are first[i] .. first[i + 1] - 1 in submission order.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace brb_plan {

inline size_t up(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct Item {
    uint32_t conn;
    int op;
    uint64_t in_off;  // copy mode: offset in the input arena; zero-copy: device address of the buffer
    uint32_t in_len;
    uint64_t out_off;
    uint32_t out_len;
    uint64_t salt;
    uint32_t round;   // sub-round: the buffer's rank among its connection's buffers in its direction
    uint32_t epoch;   // the connection's key epoch at submission (BRB_TransformBatcher::epoch)
    uint32_t pos;     // the buffer's index in its group
    uint8_t algo;     // the connection's algo at submission (1 RC4, 2 RC4_MD5); read by the mixed layout only
};

struct Group {
    int op;
    uint32_t count;     // buffers
    uint32_t streams;   // entries of sidx (without connection lists: count)
    size_t o_sidx, o_first, o_offs, o_lens, o_ooffs, o_salts;   // o_first: connection lists only
    size_t o_kind = 0;                                          // the mixed layout only
};

struct Plan {
    std::vector<Group> groups;        // in launch order
    std::vector<int64_t> group_of;    // key (see above) -> group, -1: none
    size_t o_valid = 0;               // the metadata's byte count; one valid flag per buffer may follow
};

inline size_t group_key(const Item &it, bool lists) { return lists ? size_t(it.op) : size_t(it.round) * 2 + it.op; }

// Reserves the arrays of a metadata image of `cap` bytes, one behind the other.
struct Cursor {
    size_t cap, at = 0;
    bool fits = true;
    // offset of `count` elements of `size` bytes, 8-byte aligned; once one does not fit, fits stays false
    size_t take(size_t count, size_t size)
    {
        const size_t o = at;
        if (!fits || o > cap || count > (cap - o) / size)
            fits = false;
        else
            at = up(o + count * size, 8);   // may pass cap by the padding, which nobody writes
        return o;
    }
};

template <typename T>
inline T *meta_at(uint8_t *meta, size_t off)
{
    return reinterpret_cast<T *>(meta + off);
}

// Plans the round of `items` (in submission order): sets every item's round and pos, fills *p and
// writes the metadata into meta[0, p->o_valid).  zc: in_off is a device address and goes into offs
// relative to zc_base.  Returns false, with nothing written to meta, when the metadata and a valid
// flag per item do not fit in cap bytes.
inline bool plan_round(std::vector<Item> &items, uint32_t max_conns, bool lists, bool zc, uint64_t zc_base, uint8_t *meta,
                       size_t cap, Plan *p)
{
    // rank per (direction, connection); `seen` ends as every stream's buffer count
    std::vector<uint32_t> seen(size_t(2) * max_conns, 0);
    uint32_t rounds = 0;
    for (Item &it : items) {
        it.round = seen[size_t(it.op) * max_conns + it.conn]++;
        if (it.round >= rounds)
            rounds = it.round + 1;
    }
    // count per key
    struct Count {
        uint32_t bufs = 0, streams = 0;
    };
    std::vector<Count> n(lists ? 2 : size_t(rounds) * 2);
    for (const Item &it : items) {
        Count &c = n[group_key(it, lists)];
        ++c.bufs;
        c.streams += !lists || it.round == 0;
    }
    // lay out
    Cursor cur{cap};
    p->groups.clear();
    p->group_of.assign(n.size(), -1);
    for (size_t k = 0; k < n.size(); k++) {
        if (!n[k].bufs)
            continue;
        Group g;
        g.op = int(k & 1);
        g.count = n[k].bufs;
        g.streams = n[k].streams;
        g.o_sidx = cur.take(g.streams, 4);
        g.o_first = lists ? cur.take(size_t(g.streams) + 1, 8) : 0;
        g.o_offs = cur.take(g.count, 8);
        g.o_lens = cur.take(g.count, 4);
        g.o_ooffs = cur.take(g.count, 8);
        g.o_salts = cur.take(g.count, 8);
        p->group_of[k] = int64_t(p->groups.size());
        p->groups.push_back(g);
    }
    p->o_valid = cur.at;
    if (!cur.fits || cur.at > cap || items.size() > cap - cur.at)
        return false;
    // fill: an item that opens a stream takes the stream's range of its group's buffers, and `seen`
    // turns into the stream's next free index (without lists every item opens a stream of one buffer)
    std::vector<Count> placed(p->groups.size());   // per group, so far
    for (Item &it : items) {
        const size_t gi = size_t(p->group_of[group_key(it, lists)]), c = size_t(it.op) * max_conns + it.conn;
        const Group &g = p->groups[gi];
        if (!lists || it.round == 0) {
            const uint32_t s = placed[gi].streams++, bufs = lists ? seen[c] : 1;
            meta_at<uint32_t>(meta, g.o_sidx)[s] = uint32_t(c);
            if (lists)
                meta_at<uint64_t>(meta, g.o_first)[s] = placed[gi].bufs;
            seen[c] = placed[gi].bufs;
            placed[gi].bufs += bufs;
        }
        const uint32_t k = it.pos = seen[c]++;
        meta_at<uint64_t>(meta, g.o_offs)[k] = zc ? it.in_off - zc_base : it.in_off;
        meta_at<uint32_t>(meta, g.o_lens)[k] = it.in_len;
        meta_at<uint64_t>(meta, g.o_ooffs)[k] = it.out_off;
        meta_at<uint64_t>(meta, g.o_salts)[k] = it.salt;
    }
    for (const Group &g : p->groups)
        if (lists)
            meta_at<uint64_t>(meta, g.o_first)[g.streams] = g.count;
    return true;
}

// ---- the mixed layout ---------------------------------------------------------------------------
// Stream kinds, the values of BRB_RC4_KIND_* (brb_crypto.h is not included here).
constexpr uint8_t kKindCrypt = 0, kKindFrame = 1, kKindOpen = 2;

// An RC4 connection crypts either way; an RC4_MD5 connection opens what it reads and frames what it writes.
inline uint8_t item_kind(const Item &it) { return it.algo != 2 ? kKindCrypt : it.op == 1 ? kKindFrame : kKindOpen; }

// plan_round for a round that is one launch of the mixed kernel: p->groups holds one group (none for
// an empty round) and group_of is {0}.  A stream's kind is that of its first buffer.  Sets every
// item's round and pos (its index among the round's buffers, also its valid flag's).  Returns false,
// with nothing written to meta, when the metadata and a valid flag per item do not fit in cap bytes.
inline bool plan_round_mixed(std::vector<Item> &items, uint32_t max_conns, bool zc, uint64_t zc_base, uint8_t *meta,
                             size_t cap, Plan *p)
{
    // rank per (direction, connection); `seen` ends as every stream's buffer count
    std::vector<uint32_t> seen(size_t(2) * max_conns, 0);
    std::vector<uint8_t> kind_of(size_t(2) * max_conns, 0);
    uint32_t n_streams[3] = {0, 0, 0}, n_bufs[3] = {0, 0, 0};
    for (Item &it : items) {
        const size_t c = size_t(it.op) * max_conns + it.conn;
        it.round = seen[c]++;
        if (it.round == 0)
            ++n_streams[kind_of[c] = item_kind(it)];
        ++n_bufs[kind_of[c]];
    }
    Cursor cur{cap};
    p->groups.clear();
    p->group_of.assign(1, -1);
    Group g;
    g.op = 0;
    g.count = n_bufs[0] + n_bufs[1] + n_bufs[2];
    g.streams = n_streams[0] + n_streams[1] + n_streams[2];
    if (g.count) {
        g.o_sidx = cur.take(g.streams, 4);
        g.o_first = cur.take(size_t(g.streams) + 1, 8);
        g.o_kind = cur.take(g.streams, 1);
        g.o_offs = cur.take(g.count, 8);
        g.o_lens = cur.take(g.count, 4);
        g.o_ooffs = cur.take(g.count, 8);
        g.o_salts = cur.take(g.count, 8);
        p->group_of[0] = 0;
        p->groups.push_back(g);
    }
    p->o_valid = cur.at;
    if (!cur.fits || cur.at > cap || items.size() > cap - cur.at)
        return false;
    // fill: the next free stream and buffer index of every kind; an item that opens a stream takes the
    // stream's range of buffers, and `seen` turns into the stream's next free index
    uint32_t s_at[3] = {0, n_streams[0], n_streams[0] + n_streams[1]}, b_at[3] = {0, n_bufs[0], n_bufs[0] + n_bufs[1]};
    for (Item &it : items) {
        const size_t c = size_t(it.op) * max_conns + it.conn;
        if (it.round == 0) {
            const uint8_t kd = kind_of[c];
            const uint32_t s = s_at[kd]++;
            meta_at<uint32_t>(meta, g.o_sidx)[s] = uint32_t(c);
            meta_at<uint64_t>(meta, g.o_first)[s] = b_at[kd];
            meta_at<uint8_t>(meta, g.o_kind)[s] = kd;
            const uint32_t bufs = seen[c];
            seen[c] = b_at[kd];
            b_at[kd] += bufs;
        }
        const uint32_t k = it.pos = seen[c]++;
        meta_at<uint64_t>(meta, g.o_offs)[k] = zc ? it.in_off - zc_base : it.in_off;
        meta_at<uint32_t>(meta, g.o_lens)[k] = it.in_len;
        meta_at<uint64_t>(meta, g.o_ooffs)[k] = it.out_off;
        meta_at<uint64_t>(meta, g.o_salts)[k] = it.salt;
    }
    if (g.count)
        meta_at<uint64_t>(meta, g.o_first)[g.streams] = g.count;
    return true;
}

}  // namespace brb_plan
