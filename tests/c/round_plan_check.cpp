// round_plan_check.cpp -- the transform batcher's round planner (csrc/gpu/round_plan.h) against a
// naive model, built with ASan + UBSan by tests/test_round_plan_cpu.py.  Every metadata buffer is a
// heap block of exactly the capacity handed to the planner, so a byte written past it is ASan's find.
// Exit status 0 and "ok" on success; the first failed check is printed and exits 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <utility>
#include <vector>

#include "round_plan.h"

using brb_plan::Group;
using brb_plan::Item;
using brb_plan::Plan;
using brb_plan::up;

#define CHECK(cond)                                                                                       \
    do {                                                                                                  \
        if (!(cond)) {                                                                                    \
            fprintf(stderr, "%s:%d: %s failed: %s\n", __FILE__, __LINE__, #cond, g_case);                 \
            exit(1);                                                                                      \
        }                                                                                                 \
    } while (0)

static char g_case[160];
static const uint64_t kZcBase = 0x00007f3a00001000ull;
static const uint8_t kFill = 0xA5;

static size_t meta_cap(uint32_t max_conns) { return up(size_t(80) * 4 * max_conns + 4096, 256); }   // Create's formula

template <typename T>
static T rd(const uint8_t *meta, size_t off, size_t i)
{
    T v;
    memcpy(&v, meta + off + i * sizeof(T), sizeof(T));
    return v;
}

// What a round must look like, worked out the slow way: per key the streams in order of first
// appearance, each with its members (indices into items) in submission order.
struct ModelGroup {
    size_t key;
    std::vector<std::pair<uint32_t, std::vector<size_t>>> streams;   // (op * max_conns + conn, members)
};

static std::vector<ModelGroup> model(const std::vector<Item> &items, uint32_t max_conns, bool lists,
                                     std::vector<uint32_t> *rank)
{
    std::map<size_t, ModelGroup> by_key;   // ascending keys: sub-round by sub-round, READ before WRITE
    rank->assign(items.size(), 0);
    for (size_t i = 0; i < items.size(); i++) {
        for (size_t j = 0; j < i; j++)
            (*rank)[i] += items[j].conn == items[i].conn && items[j].op == items[i].op;
        const size_t key = lists ? size_t(items[i].op) : size_t((*rank)[i]) * 2 + items[i].op;
        ModelGroup &g = by_key[key];
        g.key = key;
        const uint32_t c = uint32_t(items[i].op) * max_conns + items[i].conn;
        auto s = g.streams.begin();
        while (lists && s != g.streams.end() && s->first != c)
            ++s;
        if (!lists || s == g.streams.end())
            s = g.streams.insert(g.streams.end(), {c, {}});
        s->second.push_back(i);
    }
    std::vector<ModelGroup> out;
    for (auto &kv : by_key)
        out.push_back(std::move(kv.second));
    return out;
}

// Plans `items` into a fresh buffer of exactly `cap` bytes and checks everything; returns the bytes
// the round needs (metadata + one valid flag per item).
static size_t check_plan(const std::vector<Item> &in, uint32_t max_conns, bool lists, bool zc, size_t cap)
{
    std::vector<Item> items = in;
    std::unique_ptr<uint8_t[]> meta(new uint8_t[cap]);
    memset(meta.get(), kFill, cap);
    Plan p;
    CHECK(brb_plan::plan_round(items, max_conns, lists, zc, kZcBase, meta.get(), cap, &p));
    std::vector<uint32_t> rank;
    const std::vector<ModelGroup> want = model(items, max_conns, lists, &rank);

    // group order, group_of
    CHECK(p.groups.size() == want.size());
    size_t n_keys = lists ? 2 : 0;
    for (const ModelGroup &g : want)
        n_keys = std::max(n_keys, (g.key | 1) + 1);
    CHECK(p.group_of.size() == n_keys);
    std::vector<int64_t> group_of(n_keys, -1);
    for (size_t gi = 0; gi < want.size(); gi++)
        group_of[want[gi].key] = int64_t(gi);
    CHECK(p.group_of == group_of);

    // array placement: in order, 8-byte aligned, disjoint, the valid flags behind the last one; the byte
    // count is the one of the ladder m = up(m + size * count, 8) over the same arrays
    size_t end = 0, ladder = 0;
    for (size_t gi = 0; gi < want.size(); gi++) {
        const Group &g = p.groups[gi];
        size_t bufs = 0;
        for (const auto &s : want[gi].streams)
            bufs += s.second.size();
        CHECK(g.op == int(want[gi].key & 1) && g.count == bufs && g.streams == want[gi].streams.size());
        CHECK(lists || g.streams == g.count);
        std::vector<std::pair<size_t, size_t>> arrays = {{g.o_sidx, 4 * size_t(g.streams)}};
        if (lists)
            arrays.push_back({g.o_first, 8 * (size_t(g.streams) + 1)});
        for (auto a : {std::make_pair(g.o_offs, 8), std::make_pair(g.o_lens, 4), std::make_pair(g.o_ooffs, 8),
                       std::make_pair(g.o_salts, 8)})
            arrays.push_back({a.first, size_t(a.second) * g.count});
        for (const auto &a : arrays) {
            CHECK(a.first % 8 == 0 && a.first >= end && a.first == ladder);
            end = a.first + a.second;
            ladder = up(ladder + a.second, 8);
        }
    }
    CHECK(p.o_valid == up(end, 8) && p.o_valid == ladder);
    CHECK(p.o_valid + items.size() <= cap);
    for (size_t i = p.o_valid; i < cap; i++)
        CHECK(meta[i] == kFill);

    // membership, order inside a group, metadata contents
    std::vector<uint8_t> placed(items.size(), 0);
    for (size_t gi = 0; gi < want.size(); gi++) {
        const Group &g = p.groups[gi];
        uint32_t pos = 0;
        for (size_t s = 0; s < want[gi].streams.size(); s++) {
            const auto &st = want[gi].streams[s];
            CHECK(rd<uint32_t>(meta.get(), g.o_sidx, s) == st.first);
            if (lists)
                CHECK(rd<uint64_t>(meta.get(), g.o_first, s) == pos);   // starts at 0, non-decreasing, contiguous
            else
                CHECK(st.second.size() == 1);
            size_t before = 0;
            for (size_t i : st.second) {
                const Item &it = items[i];
                CHECK(i >= before);                                       // submission order
                before = i;
                CHECK(!placed[i]++);
                CHECK(it.round == rank[i] && it.pos == pos);
                CHECK(p.group_of[brb_plan::group_key(it, lists)] == int64_t(gi));
                CHECK(uint32_t(it.op) * max_conns + it.conn == st.first);
                CHECK(rd<uint64_t>(meta.get(), g.o_offs, pos) == (zc ? it.in_off - kZcBase : it.in_off));
                CHECK(rd<uint32_t>(meta.get(), g.o_lens, pos) == it.in_len);
                CHECK(rd<uint64_t>(meta.get(), g.o_ooffs, pos) == it.out_off);
                CHECK(rd<uint64_t>(meta.get(), g.o_salts, pos) == it.salt);
                // what the planner must leave alone
                CHECK(it.conn == in[i].conn && it.op == in[i].op && it.in_off == in[i].in_off && it.epoch == in[i].epoch);
                ++pos;
            }
        }
        CHECK(pos == g.count);
        if (lists)
            CHECK(rd<uint64_t>(meta.get(), g.o_first, g.streams) == g.count);
        // without lists: at most one buffer per connection, the connection's k-th in sub-round k
        for (size_t s = 0; !lists && s < want[gi].streams.size(); s++) {
            CHECK(rank[want[gi].streams[s].second[0]] == want[gi].key / 2);
            for (size_t t = 0; t < s; t++)
                CHECK(want[gi].streams[t].first != want[gi].streams[s].first);
        }
        // with lists: streams in order of first appearance
        for (size_t s = 1; lists && s < want[gi].streams.size(); s++)
            CHECK(want[gi].streams[s - 1].second[0] < want[gi].streams[s].second[0]);
    }
    for (uint8_t x : placed)
        CHECK(x == 1);
    return p.o_valid + items.size();
}

// The same round with one byte less than it needs: "does not fit", and not a byte written.
static void check_does_not_fit(const std::vector<Item> &in, uint32_t max_conns, bool lists, bool zc, size_t need)
{
    if (need == 0)
        return;
    std::vector<Item> items = in;
    const size_t cap = need - 1;
    std::unique_ptr<uint8_t[]> meta(new uint8_t[cap]);
    memset(meta.get(), kFill, cap);
    Plan p;
    CHECK(!brb_plan::plan_round(items, max_conns, lists, zc, kZcBase, meta.get(), cap, &p));
    for (size_t i = 0; i < cap; i++)
        CHECK(meta[i] == kFill);
}

static Item make_item(std::mt19937_64 &rng, uint32_t conn, int op)
{
    Item it{};
    it.conn = conn;
    it.op = op;
    it.in_off = rng();
    it.in_len = uint32_t(rng());
    it.out_off = rng();
    it.out_len = uint32_t(rng());
    it.salt = rng();
    it.round = it.pos = 0xDEADBEEFu;
    it.epoch = uint32_t(rng());
    return it;
}

static void run(const char *what, const std::vector<Item> &items, uint32_t max_conns)
{
    for (int lists = 0; lists < 2; lists++)
        for (int zc = 0; zc < 2; zc++) {
            snprintf(g_case, sizeof g_case, "%s, max_conns %u, %zu items, lists %d, zc %d", what, max_conns, items.size(),
                     lists, zc);
            // the budget: Create's meta_cap holds any round of up to 4 * max_conns items
            const size_t need = check_plan(items, max_conns, lists, zc, meta_cap(max_conns));
            check_plan(items, max_conns, lists, zc, need);   // and the round fits its own byte count exactly
            check_does_not_fit(items, max_conns, lists, zc, need);
        }
}

// 65 536 buffers of one connection in one direction: one group each without lists, in linear time.
static void quadratic_case()
{
    const uint32_t max_conns = 16384, n = 4 * max_conns;
    snprintf(g_case, sizeof g_case, "one connection, %u items", n);
    std::mt19937_64 rng(7);
    std::vector<Item> items;
    for (uint32_t i = 0; i < n; i++)
        items.push_back(make_item(rng, 5, 0));
    const size_t cap = meta_cap(max_conns);
    std::unique_ptr<uint8_t[]> meta(new uint8_t[cap]);
    Plan p;
    CHECK(brb_plan::plan_round(items, max_conns, false, false, 0, meta.get(), cap, &p));
    CHECK(p.groups.size() == n && p.group_of.size() == size_t(2) * n && p.o_valid == size_t(40) * n);
    for (uint32_t i = 0; i < n; i++) {
        const Group &g = p.groups[i];
        CHECK(items[i].round == i && items[i].pos == 0 && p.group_of[size_t(2) * i] == i && p.group_of[size_t(2) * i + 1] == -1);
        CHECK(g.op == 0 && g.count == 1 && g.streams == 1 && g.o_sidx == size_t(40) * i);
        CHECK(rd<uint32_t>(meta.get(), g.o_sidx, 0) == 5 && rd<uint64_t>(meta.get(), g.o_salts, 0) == items[i].salt);
    }
}

int main()
{
    std::mt19937_64 rng(0x706c616e);
    for (uint32_t max_conns : {1u, 2u, 3u, 64u}) {
        const uint32_t full = 4 * max_conns;
        std::vector<Item> items;
        // the extremes, each a full round
        for (uint32_t i = 0; i < full; i++)
            items.push_back(make_item(rng, max_conns - 1, 1));
        run("one connection, one direction", items, max_conns);
        items.clear();
        for (uint32_t i = 0; i < full; i++)
            items.push_back(make_item(rng, 0, int(i & 1)));
        run("one connection, alternating directions", items, max_conns);
        for (int dirs = 1; dirs <= 2; dirs++) {
            items.clear();
            for (uint32_t i = 0; i < full; i++)
                items.push_back(make_item(rng, i % max_conns, dirs == 1 ? 0 : int(i / max_conns) & 1));
            run(dirs == 1 ? "four per connection, one direction" : "four per connection, two and two", items, max_conns);
        }
        items.clear();
        for (uint32_t i = 0; i < max_conns; i++)
            items.push_back(make_item(rng, max_conns - 1 - i, int(i % 3 == 0)));
        run("one per connection", items, max_conns);
        run("empty round", {}, max_conns);
        // seeded random rounds: any size up to full, connections drawn evenly or crowded onto a few
        for (int trial = 0; trial < 40; trial++) {
            items.clear();
            const uint32_t n = uint32_t(rng() % (full + 1)), few = 1 + uint32_t(rng() % max_conns);
            const uint32_t span = trial % 2 ? few : max_conns, write_in = 1 + uint32_t(rng() % 4);
            for (uint32_t i = 0; i < n; i++)
                items.push_back(make_item(rng, uint32_t(rng() % span), rng() % write_in == 0));
            char what[32];
            snprintf(what, sizeof what, "random round %d", trial);
            run(what, items, max_conns);
        }
    }
    quadratic_case();
    puts("ok");
    return 0;
}
