// lane_io_check.cpp -- the per-lane byte I/O primitives of the device headers, run on the host one
// lane at a time: brb_io::Src / Snk / SectorSnk / BlockSrc, lower4 / lower16 / add_marker
// (byte_stream.h), tail_word_a4 / word_any (brb_gpu_common.h), the base64 pieces (b64_piece.h) and
// SegWalk::start's "start up to 3 bytes early, never load below the segment" (seg_walk.h).
// Built by tests/test_lane_io_cpu.py with ROCm's clang++ against tests/c/host_shim, plain and with
// ASan + UBSan (-DBRB_GLOBAL= : ASan does not instrument address_space(1) accesses).
//
// What the sanitized build adds to the values: every range under test lies in a heap block that is
// exactly the range's dword hull [align_down(a, 4), align_up(a + n, 4)), so the first dword that
// holds none of the range's bytes, on either side, is ASan's redzone; an empty range is handed a
// pointer into poisoned memory.  Output blocks are prefilled with a sentinel pattern and compared
// whole.  Expected values come from byte loops here and, for base64, from oracle/brb_oracle.c.
//
// Not covered: BlockSrcW (needs 64 lanes in lockstep), the word funnel's LDS ring (LDS addresses
// formed with and-or arithmetic) and the kernels' own loops.
//
// Exit status 0 and "ok"; the first mismatch prints the primitive and the case and exits 1.
// --plant-load / --plant-store: one access through ldg() / stg() to the dword just past an
// exact-fit block, the positive control of the sanitized build.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <sys/mman.h>

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#include <sanitizer/asan_interface.h>
#endif
#endif
#ifndef ASAN_POISON_MEMORY_REGION
#define ASAN_POISON_MEMORY_REGION(a, n) ((void)(a), (void)(n))
#define ASAN_UNPOISON_MEMORY_REGION(a, n) ((void)(a), (void)(n))
#endif

#include "b64_piece.h"
#include "seg_walk.h"

#include "brb_oracle.h"

static char g_case[200];
#define CASE(...) snprintf(g_case, sizeof g_case, __VA_ARGS__)
#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            fprintf(stderr, "%s:%d: %s failed: %s\n", __FILE__, __LINE__, #cond, g_case);        \
            exit(1);                                                                             \
        }                                                                                        \
    } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return uint32_t(g_rng >> 24);
}

static size_t up4(size_t v) { return (v + 3) & ~size_t(3); }
static uint8_t sentinel(size_t i) { return uint8_t(0xA5u + 29u * i); }

// ---- arenas ------------------------------------------------------------------------------------

// A byte range of n bytes at address & 3 == s inside a heap block that is exactly its dword hull.
// n == 0: a pointer into a wholly poisoned block.  lead: that many bytes (a multiple of 4) in front
// of the hull belong to the block too, so that the hull can start anywhere in a 64-byte sector;
// they are poisoned as far as ASan's 8-byte granules allow and, for outputs, checked as sentinels.
struct Arena {
    uint8_t *block = nullptr;
    size_t lead = 0, hull = 0, s = 0, n = 0;
    uint8_t *p = nullptr;     // the range

    Arena(size_t s_, size_t n_, size_t lead_ = 0) : lead(lead_), s(s_), n(n_)
    {
        if (n == 0 && lead == 0) {
            hull = 0;
            block = static_cast<uint8_t *>(malloc(64));
            CHECK(block);
            p = block + 32 + s;
            ASAN_POISON_MEMORY_REGION(block, 64);
            return;
        }
        hull = up4(s + n);
        if (lead) {
            void *q = nullptr;
            CHECK(posix_memalign(&q, 64, lead + hull) == 0);
            block = static_cast<uint8_t *>(q);
        } else {
            block = static_cast<uint8_t *>(malloc(hull));
        }
        CHECK(block && (reinterpret_cast<uintptr_t>(block) & 3) == 0);
        p = block + lead + s;
    }
    Arena(const Arena &) = delete;
    Arena &operator=(const Arena &) = delete;
    ~Arena()
    {
        unpoison();
        free(block);
    }
    uint8_t *hull0() const { return block + lead; }
    void poison_lead() const { ASAN_POISON_MEMORY_REGION(block, lead & ~size_t(7)); }
    void unpoison() const
    {
        if (n == 0 && lead == 0)
            ASAN_UNPOISON_MEMORY_REGION(block, 64);
        else
            ASAN_UNPOISON_MEMORY_REGION(block, lead);
    }

    // input: the hull's bytes outside the range hold noise (they may be loaded, never used)
    void fill_input(const uint8_t *data)
    {
        for (size_t i = 0; i < hull; i++)
            hull0()[i] = uint8_t(rnd() | 1u);
        if (n)
            memcpy(p, data, n);
        poison_lead();
    }
    void fill_sentinel()
    {
        for (size_t i = 0; i < lead + hull; i++)
            block[i] = sentinel(i);
        poison_lead();
    }
    // the block is the sentinels with exactly want[0..cnt) at the range's start
    bool holds(const uint8_t *want, size_t cnt) const
    {
        unpoison();
        bool ok = true;
        for (size_t i = 0; i < lead + hull; i++) {
            const size_t r = i - lead - s;       // wraps below the range
            const uint8_t w = i >= lead + s && r < cnt ? want[r] : sentinel(i);
            ok = ok && block[i] == w;
        }
        if (n == 0 && lead == 0)
            ASAN_POISON_MEMORY_REGION(block, 64);
        else
            poison_lead();
        return ok;
    }
};

// n bytes that differ from the sentinel of the position they are headed for (block offset off0 + i)
static std::vector<uint8_t> payload(size_t n, size_t off0)
{
    std::vector<uint8_t> v(n + 1);
    for (size_t i = 0; i < n; i++) {
        v[i] = uint8_t(rnd());
        if (v[i] == sentinel(off0 + i))
            v[i] ^= 0x55;
    }
    return v;
}

static std::vector<uint8_t> noise(size_t n)
{
    std::vector<uint8_t> v(n + 1);
    for (size_t i = 0; i < n; i++)
        v[i] = uint8_t(rnd() | 1u);        // never 0: a byte wrongly zeroed or kept shows
    return v;
}

static uint32_t le32(const uint8_t *b, size_t pos, size_t n)    // bytes pos..pos+3 of b[0..n), 0 past n
{
    uint32_t v = 0;
    for (size_t k = 0; k < 4; k++)
        if (pos + k < n)
            v |= uint32_t(b[pos + k]) << (8 * k);
    return v;
}

// ---- Src, BlockSrc -----------------------------------------------------------------------------

static void check_src()
{
    for (size_t s = 0; s < 4; s++)
        for (size_t n = 0; n <= 200; n++) {
            const std::vector<uint8_t> d = noise(n);
            Arena in(s, n);
            in.fill_input(d.data());
            brb_io::Src src;
            src.init(in.p, n);
            for (size_t c = 0; c < (n + 3) / 4 + 2; c++) {
                CASE("Src s=%zu n=%zu chunk=%zu", s, n, c);
                CHECK(src.next() == le32(d.data(), 4 * c, n));
            }
        }
}

static void check_block_src()
{
    for (size_t s = 0; s < 4; s++)
        for (size_t n = 0; n <= 300; n++) {
            const std::vector<uint8_t> d = noise(n);
            Arena in(s, n);
            in.fill_input(d.data());
            brb_io::BlockSrc src;
            src.init(in.p, n);
            for (size_t b = 0; b < n / 64 + 2; b++) {
                uint32_t c[16];
                src.fetch(c);
                for (size_t i = 0; i < 16; i++) {
                    CASE("BlockSrc s=%zu n=%zu block=%zu chunk=%zu", s, n, b, i);
                    CHECK(c[i] == le32(d.data(), 64 * b + 4 * i, n));
                }
            }
        }
}

// the range starts e bytes before the segment; the block is the hull of the segment alone.  Once
// through BlockSrc::init(a - e, len + e, a), once through SegWalk::start.
static void check_block_src_lo()
{
    for (int via_walk = 0; via_walk < 2; via_walk++)
        for (uint32_t e = 0; e < 4; e++)
            for (size_t s = 0; s < 4; s++)
                for (size_t len = 1; len <= 200; len++) {
                    const std::vector<uint8_t> d = noise(len);
                    Arena in(s, len);
                    in.fill_input(d.data());
                    brb_io::BlockSrc src;
                    if (via_walk) {
                        brb_funnel::SegWalk w = {};
                        w.data = in.p - 1000;
                        w.start(src, 1000, uint32_t(len), 0x7FFFFFF4u + e);
                    } else {
                        src.init(in.p - e, len + e, in.p);
                    }
                    const size_t n = len + e;
                    for (size_t b = 0; b < n / 64 + 2; b++) {
                        uint32_t c[16];
                        src.fetch(c);
                        for (size_t pos = 64 * b; pos < 64 * b + 64; pos++) {
                            if (pos < e)
                                continue;                   // the carried bytes: any value
                            CASE("BlockSrc+lo walk=%d e=%u s=%zu len=%zu pos=%zu", via_walk, e, s, len, pos);
                            const uint8_t got = uint8_t(c[(pos & 63) >> 2] >> (8 * (pos & 3)));
                            CHECK(got == (pos < n ? d[pos - e] : 0));
                        }
                    }
                }
}

// ---- Snk, SectorSnk ----------------------------------------------------------------------------

// The LDS row of a SectorSnk: 144 bytes, 16-byte aligned, below 4 GiB (the struct keeps a 32-bit
// LDS address), in the middle of a page of sentinels.
struct LdsRow {
    uint8_t *page;
    static constexpr size_t kAt = 256, kPage = 4096, kWatched = 656;    // 256 sentinels on either side
    LdsRow()
    {
        void *m = mmap(nullptr, kPage, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_32BIT, -1, 0);
        CASE("mmap(MAP_32BIT) of the LDS row");
        CHECK(m != MAP_FAILED && reinterpret_cast<uintptr_t>(m) + kPage <= 0xFFFFFFFFull);
        page = static_cast<uint8_t *>(m);
        for (size_t i = 0; i < kPage; i++)
            page[i] = sentinel(i);
    }
    ~LdsRow() { munmap(page, kPage); }
    uint32_t addr() const { return uint32_t(reinterpret_cast<uintptr_t>(page + kAt)); }
    bool around_intact() const
    {
        for (size_t i = 0; i < kWatched; i++)
            if ((i < kAt || i >= kAt + brb_io::SectorSnk::kRowBytes) && page[i] != sentinel(i))
                return false;
        return true;
    }
};

// Snk takes put() and put16() in any order.  SectorSnk's row positions are fixed at init() for blocks
// that start a multiple of 16 chunks into the stream: its single put()s come after its last put16(),
// as in the RC4 kernels (whole blocks, then the tail), so its mix is blocks first, then single chunks.
struct SnkLane {
    static constexpr bool kFreeMix = true;
    brb_io::Snk s;
    void init(uint8_t *a, uint64_t n, uint32_t) { s.init(a, n); }
    void put(uint32_t v) { s.put(v); }
    void put16(const uint32_t (&v)[16]) { s.put16(v); }
    void flush() { s.flush(); }
};
struct SectorLane {
    static constexpr bool kFreeMix = false;
    brb_io::SectorSnk s;
    void init(uint8_t *a, uint64_t n, uint32_t row) { s.init(a, n, row); }
    void put(uint32_t v) { s.put(v); }
    void put16(const uint32_t (&v)[16]) { s.put16(v); }
    void flush() { s.flush(); }
};

// mode 0: put only; 1: put16 while 16 chunks are left to offer; 2: a mix that changes with the case
template <class Lane>
static void check_sink(const char *name, size_t nmax, size_t lead_max, const LdsRow &row)
{
    for (size_t lead = 0; lead <= lead_max; lead += 4)
        for (size_t s = 0; s < 4; s++)
            for (size_t n = 0; n <= nmax; n++)
                for (int mode = 0; mode < 3; mode++) {
                    CASE("%s lead=%zu s=%zu n=%zu mode=%d", name, lead, s, n, mode);
                    // chunks past the range carry bytes that must not land anywhere
                    const size_t offered = up4(n) + 4 * 40;
                    std::vector<uint8_t> d = payload(offered, lead + s);
                    Arena out(s, n, lead);
                    out.fill_sentinel();
                    Lane k;
                    k.init(out.p, n, row.addr());
                    size_t c = 0;
                    const size_t chunks = offered / 4;
                    uint32_t mix = uint32_t(n * 7 + s * 3 + lead) * 2654435761u;
                    const size_t tail_from = 16 * ((mix >> 8) % (chunks / 16 + 1));
                    while (c < chunks) {
                        bool block = mode == 1;
                        if (mode == 2 && Lane::kFreeMix) {
                            mix = mix * 1103515245u + 12345u;
                            block = (mix >> 16) & 1;
                        } else if (mode == 2) {
                            block = c < tail_from;
                        }
                        if (block && c + 16 <= chunks) {
                            uint32_t v[16];
                            for (size_t i = 0; i < 16; i++)
                                v[i] = le32(d.data(), 4 * (c + i), offered);
                            k.put16(v);
                            c += 16;
                        } else {
                            k.put(le32(d.data(), 4 * c, offered));
                            c++;
                        }
                    }
                    k.flush();
                    CHECK(out.holds(d.data(), n));
                    // the sink is full and flushed: nothing more may be written
                    uint32_t v[16];
                    for (size_t i = 0; i < 16; i++)
                        v[i] = ~le32(d.data(), 4 * i, offered);
                    k.put(v[0]);
                    k.put16(v);
                    k.flush();
                    k.flush();
                    CHECK(out.holds(d.data(), n));
                    CHECK(row.around_intact());
                }
}

// ---- tail_word_a4, word_any ----------------------------------------------------------------------

static uint32_t padded_word(const uint8_t *d, size_t len, size_t pos)   // 0x80 at len, zeros behind
{
    uint32_t v = 0;
    for (size_t k = 0; k < 4; k++) {
        const size_t o = pos + k;
        v |= uint32_t(o < len ? d[o] : o == len ? 0x80u : 0u) << (8 * k);
    }
    return v;
}

static void check_tail_words()
{
    for (uint32_t t = 0; t < 64; t++) {
        const std::vector<uint8_t> d = noise(t);
        Arena in(0, t);
        in.fill_input(d.data());
        for (uint32_t i = 0; i < 16; i++) {
            CASE("tail_word_a4 t=%u i=%u", t, i);
            CHECK(tail_word_a4(in.p, t, i) == padded_word(d.data(), t, 4 * i));
        }
    }
    for (size_t s = 0; s < 4; s++)
        for (size_t len = 0; len <= 200; len++) {
            const std::vector<uint8_t> d = noise(len);
            Arena in(s, len);
            in.fill_input(d.data());
            for (size_t off = 0; off <= len; off++)
                for (uint32_t i = 0; i < 16; i++) {
                    CASE("word_any s=%zu len=%zu blk_off=%zu i=%u", s, len, off, i);
                    CHECK(word_any(in.p, len, off, i) == padded_word(d.data(), len, off + 4 * i));
                }
        }
}

// ---- lower4 / lower16, add_marker ----------------------------------------------------------------

static uint32_t lower_bytes(uint32_t w)
{
    uint32_t r = 0;
    for (uint32_t k = 0; k < 4; k++) {
        uint32_t b = (w >> (8 * k)) & 0xFFu;
        if (b >= 'A' && b <= 'Z')
            b += 0x20;
        r |= b << (8 * k);
    }
    return r;
}

static void check_lower_marker()
{
    static const uint32_t kNeighbour[4] = {0x00, 0x40, 0x5A, 0xFF};
    uint32_t blk[16], want[16];
    size_t fill = 0;
    for (uint32_t pos = 0; pos < 4; pos++)
        for (uint32_t nb = 0; nb < 4; nb++)
            for (uint32_t b = 0; b < 256; b++) {
                const uint32_t w = (0x01010101u * kNeighbour[nb] & ~(0xFFu << (8 * pos))) | (b << (8 * pos));
                CASE("lower4 byte=0x%02x pos=%u neighbours=0x%02x", b, pos, kNeighbour[nb]);
                CHECK(brb_io::lower4(w) == lower_bytes(w));
                blk[fill] = w;
                want[fill] = lower_bytes(w);
                if (++fill == 16) {
                    brb_io::lower16(blk);
                    CASE("lower16 ending at byte=0x%02x pos=%u neighbours=0x%02x", b, pos, kNeighbour[nb]);
                    CHECK(memcmp(blk, want, sizeof blk) == 0);
                    fill = 0;
                }
            }
    for (uint32_t t = 0; t < 64; t++)
        for (int high = 0; high < 2; high++)
            for (int pre = 0; pre < 2; pre++) {
                uint32_t w[16], base[16];
                for (uint32_t i = 0; i < 16; i++)
                    w[i] = base[i] = pre ? 0x01010101u * (i + 1) : 0u;
                const uint64_t len = (high ? 0x123456789ull * 64 : 0) + t;
                brb_io::add_marker(w, len);
                for (uint32_t i = 0; i < 16; i++) {
                    CASE("add_marker len=%llu word=%u prefilled=%d", (unsigned long long)len, i, pre);
                    CHECK(w[i] == (base[i] | (i == t / 4 ? 0x80u << (8 * (t & 3)) : 0u)));
                }
            }
}

// ---- base64 pieces -------------------------------------------------------------------------------

static void check_piece_io()
{
    for (size_t s = 0; s < 4; s++)
        for (uint32_t m = 0; m <= 16; m++) {
            const std::vector<uint8_t> d = noise(m);
            Arena in(s, m);
            in.fill_input(d.data());
            uint32_t w[4] = {~0u, ~0u, ~0u, ~0u};
            brb_b64::load_piece(in.p, m, w);
            for (size_t k = 0; k < 4; k++) {
                CASE("load_piece s=%zu m=%u dword=%zu", s, m, k);
                CHECK(w[k] == le32(d.data(), 4 * k, m));
            }
        }
    {
        const std::vector<uint8_t> d = noise(12);
        Arena in(0, 12);
        in.fill_input(d.data());
        uint32_t w[4] = {~0u, ~0u, ~0u, ~0u};
        brb_b64::load12_a4(in.p, w);
        for (size_t k = 0; k < 4; k++) {
            CASE("load12_a4 dword=%zu", k);
            CHECK(w[k] == le32(d.data(), 4 * k, 12));
        }
    }
    for (size_t s = 0; s < 4; s++)
        for (uint32_t q = 0; q <= 16; q++) {
            CASE("store_piece s=%zu q=%u", s, q);
            const std::vector<uint8_t> d = payload(16, s);
            Arena out(s, q);
            if (q)
                out.fill_sentinel();
            const uint32_t v[4] = {le32(d.data(), 0, 16), le32(d.data(), 4, 16), le32(d.data(), 8, 16),
                                   le32(d.data(), 12, 16)};
            brb_b64::store_piece(out.p, q, v);
            if (q)
                CHECK(out.holds(d.data(), q));
        }
}

static const char kAlphabet[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";

static void check_encode_piece()
{
    // the kernel's LDS table, built as the kernel builds it
    static uint16_t pair[4096];
    for (uint32_t e = 0; e < 4096; e++)
        pair[e] = uint16_t(brb_b64::alpha(e >> 6) | (brb_b64::alpha(e & 63) << 8));
    for (uint32_t i = 0; i < 64; i++) {
        CASE("alpha(%u)", i);
        CHECK(brb_b64::alpha(i) == uint32_t(kAlphabet[i]));
    }
    for (uint32_t m = 1; m <= 12; m++)
        for (int trial = 0; trial < 300; trial++) {
            uint8_t in[12] = {0};
            for (uint32_t i = 0; i < m; i++)
                in[i] = trial == 0 ? 0x00 : trial == 1 ? 0xFF : uint8_t(rnd());
            const uint32_t d[4] = {le32(in, 0, 12), le32(in, 4, 12), le32(in, 8, 12), 0};
            uint32_t c[4] = {0, 0, 0, 0};
            const uint32_t q = brb_b64::encode_piece(pair, d, m, c);
            char want[17] = {0};
            const uint64_t wq = orc_b64_encode(in, m, want);
            CASE("encode_piece m=%u trial=%d", m, trial);
            CHECK(q == wq && q == 4 * ((m + 2) / 3));
            uint8_t got[16];
            memcpy(got, c, 16);
            CHECK(memcmp(got, want, q) == 0);
        }
}

static int8_t g_val[256];    // the decode kernel's LDS table, built as the kernel builds it

static void check_decode_piece()
{
    for (uint32_t e = 0; e < 256; e++) {
        g_val[e] = int8_t(brb_b64::b64_value(e));
        const char *at = e ? strchr(kAlphabet, int(e)) : nullptr;
        CASE("b64_value(0x%02x)", e);
        CHECK(g_val[e] == (e == '=' ? 0 : at ? int(at - kAlphabet) : -1));
    }
    static const uint8_t kDirty[5] = {0x00, '\n', '*', 0x80, 0xFF};
    for (int trial = 0; trial < 200; trial++)
        for (int dirty = -1; dirty < 5; dirty++)
            for (uint32_t at = 0; at < (dirty < 0 ? 1u : 16u); at++) {
                uint8_t ch[16];
                for (uint32_t i = 0; i < 16; i++)
                    ch[i] = rnd() % 9 == 0 ? uint8_t('=') : uint8_t(kAlphabet[rnd() & 63]);
                if (dirty >= 0)
                    ch[at] = kDirty[dirty];
                const uint32_t d[4] = {le32(ch, 0, 16), le32(ch, 4, 16), le32(ch, 8, 16), le32(ch, 12, 16)};
                for (uint32_t groups = 0; groups <= 4; groups++) {
                    uint32_t b[4] = {~0u, ~0u, ~0u, ~0u};
                    const uint32_t f = brb_b64::decode_piece(g_val, d, groups, b);
                    CASE("decode_piece trial=%d dirty=%d at=%u groups=%u", trial, dirty, at, groups);
                    CHECK(f == (dirty >= 0 && at / 4 < groups ? 0x80000000u : 0u));
                    CHECK(b[3] == 0);
                    uint8_t got[12];
                    memcpy(got, b, 12);
                    if (dirty < 0) {
                        uint8_t want[12];
                        CHECK(orc_b64_decode(reinterpret_cast<const char *>(ch), 16, want) == 12);
                        CHECK(memcmp(got, want, 12) == 0);
                    } else {
                        for (uint32_t g = 0; g < 4; g++) {      // the clean groups stand on their own
                            if (g == at / 4)
                                continue;
                            uint8_t want[3];
                            CHECK(orc_b64_decode(reinterpret_cast<const char *>(ch + 4 * g), 4, want) == 3);
                            CHECK(memcmp(got + 3 * g, want, 3) == 0);
                        }
                    }
                }
            }
}

static void check_decode_serial()
{
    // defect kinds: none, one skipped byte, a NUL, a run of three skipped bytes, '='
    for (size_t len = 0; len <= 80; len++)
        for (int kind = 0; kind < 5; kind++)
            for (size_t at = 0; at < (kind == 0 ? 1 : len); at++) {
                std::vector<uint8_t> text(len + 1);
                for (size_t i = 0; i < len; i++)
                    text[i] = uint8_t(kAlphabet[rnd() & 63]);
                size_t defect_end = at;          // [at, defect_end) is not clean
                if (kind == 1) {
                    text[at] = '\n';
                    defect_end = at + 1;
                } else if (kind == 2) {
                    text[at] = 0;
                    defect_end = at + 1;
                } else if (kind == 3) {
                    for (size_t i = at; i < at + 3 && i < len; i++)
                        text[i] = i == at ? ' ' : i == at + 1 ? 0x80 : 0xFF;
                    defect_end = at + 3;
                } else if (kind == 4) {
                    text[at] = '=';
                }
                std::vector<uint8_t> want(3 * (len / 4) + 4);
                const uint64_t wn = orc_b64_decode(reinterpret_cast<const char *>(text.data()), len, want.data());
                const size_t cap = 3 * (len / 4);
                CASE("decode_serial len=%zu kind=%d at=%zu: oracle length", len, kind, at);
                CHECK(wn <= cap);
                for (size_t si = 0; si < 4; si++) {
                    Arena in(si, len);
                    in.fill_input(text.data());
                    for (size_t so = 0; so < 4; so++)
                        for (size_t pos = 0; pos <= len; pos += 16) {
                            if (defect_end > at && pos > at)
                                break;                          // the prefix must be clean
                            const uint32_t produced = uint32_t(12 * pos / 16);
                            if (produced > cap)
                                break;
                            CASE("decode_serial len=%zu kind=%d at=%zu in&3=%zu out&3=%zu pos=%zu", len, kind, at, si,
                                 so, pos);
                            Arena out(so, cap);
                            if (cap)
                                out.fill_sentinel();
                            // the bytes before `produced` are other lanes': they stay sentinels here
                            std::vector<uint8_t> img(cap + 1);
                            for (size_t i = 0; i < cap; i++)
                                img[i] = i < produced ? sentinel(so + i) : i < wn ? want[i] : sentinel(so + i);
                            const uint32_t got = brb_b64::decode_serial(g_val, in.p, len, pos, out.p, produced);
                            CHECK(got == wn);
                            if (cap)
                                CHECK(out.holds(img.data(), cap));
                        }
                }
            }
}

// ---- positive controls ---------------------------------------------------------------------------

static int plant(bool store)
{
    uint32_t *p = static_cast<uint32_t *>(malloc(16));
    p[0] = p[1] = p[2] = p[3] = 0;
    uint32_t *volatile past = p + 4;    // through a volatile: the compiler must not know the block's size,
    uint32_t *q = past;                 // or UBSan's object-size check reports it before ASan can
    uint32_t v = 0;
    if (store)
        stg(q, 1u);
    else
        v = ldg(q);
    free(p);
    printf("planted %s done (%u)\n", store ? "store" : "load", v & 1u);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && strcmp(argv[1], "--plant-load") == 0)
        return plant(false);
    if (argc > 1 && strcmp(argv[1], "--plant-store") == 0)
        return plant(true);
    LdsRow row;
    check_src();
    check_block_src();
    check_block_src_lo();
    check_sink<SnkLane>("Snk", 200, 0, row);
    check_sink<SectorLane>("SectorSnk", 400, 60, row);
    check_tail_words();
    check_lower_marker();
    check_piece_io();
    check_encode_piece();
    check_decode_piece();
    check_decode_serial();
    printf("ok\n");
    return 0;
}
