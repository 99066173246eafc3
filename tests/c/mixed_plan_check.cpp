// mixed_plan_check.cpp -- the mixed layout of the transform batcher's round planner
// (brb_plan::plan_round_mixed, csrc/gpu/round_plan.h) against a naive model, built with ASan + UBSan by
// tests/test_rc4_mixed_cpu.py.  Every metadata buffer is a heap block of exactly the capacity handed to
// the planner, so a byte written past it is ASan's find.  Exit status 0 and "ok" on success; the first
// failed check is printed and exits 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// The kind of a buffer, written out: RC4 (algo 1) crypts either way (0), RC4_MD5 (algo 2) frames what it
// writes (1) and opens what it reads (2).
static uint8_t kind_of(const Item &it) { return it.algo == 1 ? 0 : it.op == 1 ? 1 : 2; }

// What the round must look like, worked out the slow way: the streams of kind 0, then 1, then 2, inside a
// kind in order of first appearance, each with its members (indices into items) in submission order.
struct ModelStream {
    uint32_t c;   // op * max_conns + conn
    uint8_t kind;
    std::vector<size_t> members;
};

static std::vector<ModelStream> model(const std::vector<Item> &items, uint32_t max_conns)
{
    std::vector<ModelStream> out;
    for (uint8_t kind = 0; kind < 3; kind++) {
        const size_t k0 = out.size();
        for (size_t i = 0; i < items.size(); i++) {
            const uint32_t c = uint32_t(items[i].op) * max_conns + items[i].conn;
            // the stream's kind is that of its first buffer
            size_t f = 0;
            while (uint32_t(items[f].op) * max_conns + items[f].conn != c)
                ++f;
            if (kind_of(items[f]) != kind)
                continue;
            size_t s = k0;
            while (s < out.size() && out[s].c != c)
                ++s;
            if (s == out.size())
                out.push_back(ModelStream{c, kind, {}});
            out[s].members.push_back(i);
        }
    }
    return out;
}

static size_t check_plan(const std::vector<Item> &in, uint32_t max_conns, bool zc, size_t cap)
{
    std::vector<Item> items = in;
    std::unique_ptr<uint8_t[]> meta(new uint8_t[cap]);
    memset(meta.get(), kFill, cap);
    Plan p;
    CHECK(brb_plan::plan_round_mixed(items, max_conns, zc, kZcBase, meta.get(), cap, &p));
    const std::vector<ModelStream> want = model(items, max_conns);

    // one group for the round, none for an empty one
    CHECK(p.group_of.size() == 1);
    if (items.empty()) {
        CHECK(p.groups.empty() && p.group_of[0] == -1 && p.o_valid == 0);
        for (size_t i = 0; i < cap; i++)
            CHECK(meta[i] == kFill);
        return 0;
    }
    CHECK(p.groups.size() == 1 && p.group_of[0] == 0);
    const Group &g = p.groups[0];
    CHECK(g.count == items.size() && g.streams == want.size());

    // array placement: in order, 8-byte aligned, disjoint, the valid flags behind the last one
    const std::pair<size_t, size_t> arrays[] = {{g.o_sidx, 4 * size_t(g.streams)},  {g.o_first, 8 * (size_t(g.streams) + 1)},
                                                {g.o_kind, size_t(g.streams)},      {g.o_offs, 8 * size_t(g.count)},
                                                {g.o_lens, 4 * size_t(g.count)},    {g.o_ooffs, 8 * size_t(g.count)},
                                                {g.o_salts, 8 * size_t(g.count)}};
    size_t end = 0, ladder = 0;
    for (const auto &a : arrays) {
        CHECK(a.first % 8 == 0 && a.first >= end && a.first == ladder);
        end = a.first + a.second;
        ladder = up(ladder + a.second, 8);
    }
    CHECK(p.o_valid == up(end, 8) && p.o_valid == ladder);
    CHECK(p.o_valid + items.size() <= cap);
    for (size_t i = p.o_valid; i < cap; i++)
        CHECK(meta[i] == kFill);

    // membership, kind order, first appearance inside a kind, buffer order inside a stream, contents
    std::vector<uint8_t> placed(items.size(), 0);
    std::vector<uint32_t> rank(items.size(), 0);
    for (size_t i = 0; i < items.size(); i++)
        for (size_t j = 0; j < i; j++)
            rank[i] += items[j].conn == items[i].conn && items[j].op == items[i].op;
    uint32_t pos = 0;
    for (size_t s = 0; s < want.size(); s++) {
        const ModelStream &st = want[s];
        CHECK(rd<uint32_t>(meta.get(), g.o_sidx, s) == st.c);
        CHECK(rd<uint8_t>(meta.get(), g.o_kind, s) == st.kind);
        CHECK(rd<uint64_t>(meta.get(), g.o_first, s) == pos);
        if (s) {
            CHECK(want[s - 1].kind <= st.kind);                                        // sorted by kind
            if (want[s - 1].kind == st.kind)
                CHECK(want[s - 1].members[0] < st.members[0]);                         // first appearance inside a kind
        }
        size_t before = 0;
        for (size_t i : st.members) {
            const Item &it = items[i];
            CHECK(i >= before);                                                        // submission order
            before = i;
            CHECK(!placed[i]++);
            CHECK(it.round == rank[i] && it.pos == pos);
            CHECK(uint32_t(it.op) * max_conns + it.conn == st.c);
            CHECK(rd<uint64_t>(meta.get(), g.o_offs, pos) == (zc ? it.in_off - kZcBase : it.in_off));
            CHECK(rd<uint32_t>(meta.get(), g.o_lens, pos) == it.in_len);
            CHECK(rd<uint64_t>(meta.get(), g.o_ooffs, pos) == it.out_off);
            CHECK(rd<uint64_t>(meta.get(), g.o_salts, pos) == it.salt);
            // what the planner must leave alone
            CHECK(it.conn == in[i].conn && it.op == in[i].op && it.in_off == in[i].in_off && it.epoch == in[i].epoch &&
                  it.algo == in[i].algo && it.out_len == in[i].out_len);
            ++pos;
        }
    }
    CHECK(pos == g.count && rd<uint64_t>(meta.get(), g.o_first, g.streams) == g.count);
    for (uint8_t x : placed)
        CHECK(x == 1);
    return p.o_valid + items.size();
}

// The same round with one byte less than it needs: "does not fit", and not a byte written.
static void check_does_not_fit(const std::vector<Item> &in, uint32_t max_conns, bool zc, size_t need)
{
    if (need == 0)
        return;
    std::vector<Item> items = in;
    const size_t cap = need - 1;
    std::unique_ptr<uint8_t[]> meta(new uint8_t[cap]);
    memset(meta.get(), kFill, cap);
    Plan p;
    CHECK(!brb_plan::plan_round_mixed(items, max_conns, zc, kZcBase, meta.get(), cap, &p));
    for (size_t i = 0; i < cap; i++)
        CHECK(meta[i] == kFill);
}

static Item make_item(std::mt19937_64 &rng, uint32_t conn, int op, const std::vector<uint8_t> &algos)
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
    it.algo = algos[conn];
    return it;
}

static void run(const char *what, const std::vector<Item> &items, uint32_t max_conns, int mix)
{
    for (int zc = 0; zc < 2; zc++) {
        snprintf(g_case, sizeof g_case, "%s, max_conns %u, %zu items, algo mix %d, zc %d", what, max_conns, items.size(), mix, zc);
        // the budget: Create's meta_cap holds any round of up to 4 * max_conns items
        const size_t need = check_plan(items, max_conns, zc, meta_cap(max_conns));
        check_plan(items, max_conns, zc, need);   // and the round fits its own byte count exactly
        check_does_not_fit(items, max_conns, zc, need);
    }
}

int main()
{
    std::mt19937_64 rng(0x6d697865);
    for (uint32_t max_conns : {1u, 2u, 3u, 64u})
        // every mix of algos: all RC4, all RC4_MD5, alternating, alternating the other way, seeded random
        for (int mix = 0; mix < 5; mix++) {
            std::vector<uint8_t> algos(max_conns);
            for (uint32_t c = 0; c < max_conns; c++)
                algos[c] = mix == 0 ? 1 : mix == 1 ? 2 : mix == 2 ? 1 + c % 2 : mix == 3 ? 2 - c % 2 : 1 + uint8_t(rng() & 1);
            const uint32_t full = 4 * max_conns;
            std::vector<Item> items;
            // the extremes, each a full round
            for (uint32_t i = 0; i < full; i++)
                items.push_back(make_item(rng, max_conns - 1, 1, algos));
            run("one connection, one direction", items, max_conns, mix);
            items.clear();
            for (uint32_t i = 0; i < full; i++)
                items.push_back(make_item(rng, 0, int(i & 1), algos));
            run("one connection, alternating directions", items, max_conns, mix);
            items.clear();
            for (uint32_t i = 0; i < full; i++)
                items.push_back(make_item(rng, i % max_conns, int(i / max_conns) & 1, algos));
            run("four per connection, two and two", items, max_conns, mix);
            items.clear();
            for (uint32_t i = 0; i < 2 * max_conns; i++)     // every stream there is, one buffer each: the most streams
                items.push_back(make_item(rng, max_conns - 1 - i % max_conns, int(i / max_conns), algos));
            run("one per stream", items, max_conns, mix);
            run("empty round", {}, max_conns, mix);
            // seeded random rounds: any size up to full, connections drawn evenly or crowded onto a few
            for (int trial = 0; trial < 30; trial++) {
                items.clear();
                const uint32_t n = uint32_t(rng() % (full + 1)), few = 1 + uint32_t(rng() % max_conns);
                const uint32_t span = trial % 2 ? few : max_conns, write_in = 1 + uint32_t(rng() % 4);
                for (uint32_t i = 0; i < n; i++)
                    items.push_back(make_item(rng, uint32_t(rng() % span), rng() % write_in == 0, algos));
                char what[32];
                snprintf(what, sizeof what, "random round %d", trial);
                run(what, items, max_conns, mix);
            }
        }
    puts("ok");
    return 0;
}
