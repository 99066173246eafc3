// batch_api.hip -- the batch entry points of the exported C ABI; see include/brb_crypto.h.  The
// per-thread runtime they use (errors, device probe, workspaces, fault words, BRB_CryptoGPU_*) is in
// api_runtime.hip, the chunked host-mode pipelines of the fixed-stride calls in host_pipe.hip.
//
// Host mode (BRB_BATCH_HOST): inputs are copied into a per-thread device workspace, the kernel
// runs, results are copied back, and the call returns after the stream has drained.
// Device mode (BRB_BATCH_DEVICE): the caller's HBM-resident buffers are used in place.
// There is no CPU fallback anywhere in this file: a missing or failing device returns
// BRB_BATCH_NOT_DONE with the reason in BRB_CryptoGPU_LastError().
//
// An entry point reads: arguments and checks; the device branch (device_run); the host branch
// (span_rebase, Staging's adders, Staging::run with the launch in a lambda).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "brb_crypto.h"
#include "api_util.h"
#include "brb_kernels.h"
#include "host_pipe.h"

namespace {

using brb_api::align_up;
using brb_api::device_ok;
using brb_api::fail_hip;
using brb_api::PairFault;
using brb_api::set_err;
using brb_api::t_err;
using brb_api::workspace;
using brb_host::FixedLauncher;

inline const uint8_t *bytes(const void *p) { return static_cast<const uint8_t *>(p); }
inline uint8_t *bytes(void *p) { return static_cast<uint8_t *>(p); }

// One-lane-per-item kernels (variable-length digests, RC4 streams, segments, base64) launch one
// work-item per item, and a launch holds fewer than 2^32 work-items per dimension.
constexpr uint64_t kMaxItems = (uint64_t(1) << 32) - (uint64_t(1) << 16);

bool items_ok(uint64_t n)
{
    if (n <= kMaxItems)
        return true;
    set_err("%llu items in one call (at most %llu): split the batch", (unsigned long long)n,
            (unsigned long long)kMaxItems);
    return false;
}

// BRB_BATCH_ALL_DEVICES splits host-mode batches only (device pointers belong to one device).
bool flags_ok(unsigned flags)
{
    if ((flags & BRB_BATCH_ALL_DEVICES) && (flags & BRB_BATCH_DEVICE)) {
        set_err("BRB_BATCH_ALL_DEVICES needs host pointers (device pointers belong to one device)");
        return false;
    }
    return true;
}

int finish(hipStream_t s, unsigned flags)
{
    if ((flags & BRB_BATCH_DEVICE) && (flags & BRB_BATCH_ASYNC))
        return BRB_BATCH_OK;
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess)
        return fail_hip("hipStreamSynchronize", e);
    return BRB_BATCH_OK;
}

// a launcher's result as a BRB code
int launched(hipError_t e)
{
    return e == hipSuccess ? BRB_BATCH_OK : fail_hip("kernel launch", e);
}

// Device mode: the launch has been issued on the caller's buffers; synchronise unless ASYNC, then
// (calls on wave-pair kernels) read the fault word.
int device_run(hipError_t launch_result, hipStream_t s, unsigned flags, const PairFault *pf = nullptr)
{
    if (launch_result != hipSuccess)
        return launched(launch_result);
    const int rc = finish(s, flags);
    return pf ? pf->check(rc) : rc;
}

// ---- host-mode staging --------------------------------------------------------------------------
// Segments are laid out back to back (256-B aligned) in the per-thread workspace; `in` segments are
// copied H2D before the launch, `out` segments D2H after it (`inout`: both; `scratch`: neither).
// run() is the one place in this file that uploads, launches, downloads and synchronises.
struct Staging {
    struct Seg {
        const void *h_in;
        void *h_out;
        size_t bytes, off;
    };
    static constexpr size_t kMaxSegs = 12;           // the most any call adds is 9; no allocation per call
    Seg segs[kMaxSegs];
    size_t n_segs = 0, total = 0;
    uint8_t *ws = nullptr;

    // each returns the segment's index for dev(); a NULL host pointer or 0 bytes copies nothing
    size_t in(const void *h, size_t bytes) { return add(h, nullptr, bytes); }
    size_t out(void *h, size_t bytes) { return add(nullptr, h, bytes); }
    size_t inout(void *h, size_t bytes) { return add(h, h, bytes); }
    size_t scratch(size_t bytes) { return add(nullptr, nullptr, bytes); }

    template <class T = uint8_t>
    T *dev(size_t i) const
    {
        return reinterpret_cast<T *>(ws + segs[i].off);
    }

    // Uploads the `in` segments, calls body() -- it issues the launch or launches on `s` and returns
    // a BRB code -- then downloads the `out` segments, synchronises and (pf) reads the fault word.
    // On any failure the stream is drained before the first error is returned, so the workspace is
    // never regrown under a copy.
    template <class Body>
    int run(hipStream_t s, const PairFault *pf, Body body)
    {
        int rc = upload(s);
        if (rc == BRB_BATCH_OK)
            rc = body();
        if (rc != BRB_BATCH_OK) {
            (void)hipStreamSynchronize(s);
            return rc;
        }
        rc = download(s);
        return pf ? pf->check(rc) : rc;
    }

private:
    size_t add(const void *h_in, void *h_out, size_t bytes)
    {
        assert(n_segs < kMaxSegs);
        segs[n_segs] = {h_in, h_out, bytes, total};
        total = align_up(total + bytes, 256);
        return n_segs++;
    }
    int upload(hipStream_t s)
    {
        hipError_t e;
        ws = static_cast<uint8_t *>(workspace(std::max<size_t>(total, 256), &e));
        if (!ws)
            return fail_hip("device workspace", e);
        for (size_t i = 0; i < n_segs; i++) {
            const Seg &g = segs[i];
            if (g.h_in && g.bytes && (e = hipMemcpyAsync(ws + g.off, g.h_in, g.bytes, hipMemcpyHostToDevice, s)) != hipSuccess)
                return fail_hip("hipMemcpyAsync H2D", e);
        }
        return BRB_BATCH_OK;
    }
    int download(hipStream_t s)
    {
        hipError_t e;
        for (size_t i = 0; i < n_segs; i++) {
            const Seg &g = segs[i];
            if (g.h_out && g.bytes && (e = hipMemcpyAsync(g.h_out, ws + g.off, g.bytes, hipMemcpyDeviceToHost, s)) != hipSuccess)
                return fail_hip("hipMemcpyAsync D2H", e);
        }
        return finish(s, 0);
    }
};

// [lo, hi) covered by ranges offsets[i] .. + lengths[i] + extra (empty ranges ignored); false (and
// the error set) when a range wraps the address space
template <typename LenT>   // uint32_t, or uint64_t for the keyed Blowfish records (16 bytes x a uint32 block count)
bool span_of(const uint64_t *offs, const LenT *lens, uint64_t n, uint64_t extra, uint64_t &lo, uint64_t &hi)
{
    lo = UINT64_MAX;
    hi = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t len = uint64_t(lens[i]) + extra;
        if (!len)
            continue;
        if (offs[i] > UINT64_MAX - len) {
            set_err("range %llu: offset %llu + %llu bytes wraps", (unsigned long long)i, (unsigned long long)offs[i],
                    (unsigned long long)len);
            return false;
        }
        lo = std::min(lo, offs[i]);
        hi = std::max(hi, offs[i] + len);
    }
    if (lo == UINT64_MAX)
        lo = hi = 0;
    return true;
}

// The byte span [lo, hi) a host-mode call stages for its ranges, and the ranges' offsets inside it.
// An empty range (length + extra == 0) gets offset 0: its caller's offset may lie anywhere, also
// outside the span, and no kernel forms an address from it.  !ok: a range wraps (the error is set).
struct Span {
    bool ok = false;
    uint64_t lo = 0, hi = 0;
    std::vector<uint64_t> off;
    size_t bytes() const { return size_t(hi - lo); }
};

template <typename LenT>
Span span_rebase(const uint64_t *offs, const LenT *lens, uint64_t n, uint64_t extra = 0)
{
    Span sp;
    if (!(sp.ok = span_of(offs, lens, n, extra, sp.lo, sp.hi)))
        return sp;
    sp.off.resize(n);
    for (uint64_t i = 0; i < n; i++)
        sp.off[i] = uint64_t(lens[i]) + extra ? offs[i] - sp.lo : 0;
    return sp;
}

// The data segments of a call that reads `in` and writes `out`, which may be the same bytes: in place, one
// segment staged in both directions; else the input in and the output in both directions, so that the bytes
// of the output's span the call does not write survive.
struct InOut { size_t in, out; };

InOut stage_in_out(Staging &st, bool in_place, const uint8_t *in, size_t in_bytes, uint8_t *out, size_t out_bytes)
{
    if (in_place) {
        const size_t i = st.inout(out, out_bytes);
        return {i, i};
    }
    const size_t i = st.in(in, in_bytes);
    return {i, st.inout(out, out_bytes)};
}

// BRB_BATCH_ALL_DEVICES for the multi-range calls whose host-mode parts write a byte span back
// (RC4 streams, frames, base64 outputs): part g stages and returns the span its ranges
// [g n/G, (g+1) n/G) cover, so the split is taken only when those spans are pairwise disjoint --
// otherwise a part would write back bytes of another part's ranges.  Streams of different
// connections are disjoint by contract; ranges in submission order give disjoint spans.  Ranges
// in any other order run on the calling thread's device (same results, one device).
template <typename LenT>
bool parts_disjoint(const uint64_t *offs, const LenT *lens, uint64_t n, uint64_t extra)
{
    const int G = brb_host::split_parts();
    if (G <= 1 || n < uint64_t(G))
        return false;
    std::vector<std::pair<uint64_t, uint64_t>> sp;
    for (int g = 0; g < G; g++) {
        const uint64_t a = n * uint64_t(g) / uint64_t(G), b = n * uint64_t(g + 1) / uint64_t(G);
        uint64_t lo, hi;
        if (!span_of(offs + a, lens + a, b - a, extra, lo, hi))
            return false;
        if (hi > lo)
            sp.push_back({lo, hi});
    }
    std::sort(sp.begin(), sp.end());
    for (size_t i = 1; i < sp.size(); i++)
        if (sp[i].first < sp[i - 1].second)
            return false;
    return true;
}

// A host-mode "first" list (item i owns [first[i], first[i + 1])), checked: the range [k0, k0 + count) of
// the caller's arrays it covers and, made where the call stages, the copy rebased to start at 0.  !ok: not
// non-decreasing (the error names the list), or each(i), run after item i's check, refused (its own error).
struct FirstList {
    const uint64_t *first;
    uint64_t n, k0, count;
    bool ok;
    std::vector<uint64_t> rebased() const
    {
        std::vector<uint64_t> rel(first, first + n + 1);
        for (uint64_t &f : rel)
            f -= k0;
        return rel;
    }
};

template <class Each>
FirstList first_list(const uint64_t *first, uint64_t n, const char *name, Each each)
{
    FirstList fl{first, n, first[0], first[n] - first[0], false};
    for (uint64_t i = 0; i < n; i++) {
        if (first[i + 1] < first[i]) {
            set_err("%s is not non-decreasing at %llu", name, (unsigned long long)i);
            return fl;
        }
        if (!each(i))
            return fl;
    }
    fl.ok = true;
    return fl;
}

// count_items: the range must also fit one launch (items_ok: the RC4 list kernels' per-buffer arrays)
FirstList first_list(const uint64_t *first, uint64_t n, const char *name, bool count_items = false)
{
    FirstList fl = first_list(first, n, name, [](uint64_t) { return true; });
    fl.ok = fl.ok && (!count_items || items_ok(fl.count));
    return fl;
}

// parts_disjoint for streams that own buffer lists: stream i's written span is the span of buffers
// first[i] .. first[i + 1] - 1 (+ extra bytes each); a stream without buffers writes nothing.
bool stream_parts_disjoint(const uint64_t *offs, const uint32_t *lens, const uint64_t *first, uint64_t n, uint64_t extra)
{
    std::vector<uint64_t> so(n), sl(n);
    for (uint64_t i = 0; i < n; i++) {
        uint64_t lo, hi;
        if (!span_of(offs + first[i], lens + first[i], first[i + 1] - first[i], extra, lo, hi))
            return false;
        so[i] = lo;
        sl[i] = hi - lo;
    }
    return parts_disjoint(so.data(), sl.data(), n, 0);
}

// The contexts a host-mode call names in a context table: item i acts on ctxs[ix ? ix[i] : i].  ok() checks
// the index list (dup_hint: what to do instead of naming a context twice); gather() is what the call stages
// in both directions, the named contexts in item order, so the kernel runs without an index; scatter() puts
// them back after a run that succeeded.
struct NamedCtx {
    uint8_t *ctxs;
    const uint32_t *ix;
    uint64_t n;
    size_t stride;
    std::vector<uint8_t> rows;

    bool ok(uint64_t n_ctx, const char *dup_hint) const
    {
        if (!ix) {
            if (n > n_ctx)
                set_err("ctx_index is NULL and n (%llu) > n_ctx (%llu)", (unsigned long long)n, (unsigned long long)n_ctx);
            return n <= n_ctx;
        }
        for (uint64_t i = 0; i < n; i++)
            if (ix[i] >= n_ctx) {
                set_err("item %llu: ctx_index %u out of range (%llu contexts)", (unsigned long long)i, ix[i],
                        (unsigned long long)n_ctx);
                return false;
            }
        std::vector<uint32_t> sorted(ix, ix + n);
        std::sort(sorted.begin(), sorted.end());
        const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
        if (dup != sorted.end())
            set_err("context %u is named twice (%s)", *dup, dup_hint);
        return dup == sorted.end();
    }
    uint8_t *gather()
    {
        rows.resize(ix ? n * stride : 0);
        for (uint64_t i = 0; ix && i < n; i++)
            memcpy(rows.data() + i * stride, ctxs + ix[i] * stride, stride);
        return ix ? rows.data() : ctxs;
    }
    int scatter(int rc) const
    {
        for (uint64_t i = 0; rc == BRB_BATCH_OK && ix && i < n; i++)
            memcpy(ctxs + ix[i] * stride, rows.data() + i * stride, stride);
        return rc;
    }
};

// ---- digests ------------------------------------------------------------------------------------
using VarLauncher = hipError_t (*)(const uint8_t *, const uint64_t *, const uint32_t *, uint64_t, uint8_t *,
                                   hipStream_t);

int digest_fixed(FixedLauncher launch, size_t dig_len, const void *data, uint32_t rec_len, uint64_t n_rec,
                 void *digests, unsigned flags, void *stream)
{
    t_err.clear();
    if (n_rec == 0)
        return BRB_BATCH_OK;
    if (!digests || (!data && rec_len)) {
        set_err("NULL data or digests");
        return BRB_BATCH_BADARG;
    }
    if ((rec_len == 0 && !items_ok(n_rec)) || !flags_ok(flags))   // empty records: one-lane-per-record kernel
        return BRB_BATCH_BADARG;
    if (int ok = device_ok(); ok != BRB_BATCH_OK)
        return ok;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (flags & BRB_BATCH_DEVICE)
        return device_run(launch(bytes(data), rec_len, n_rec, bytes(digests), s), s, flags);
    return brb_host::digest_fixed(launch, dig_len, bytes(data), rec_len, n_rec, bytes(digests), flags, s);
}

int digest_var(VarLauncher launch, size_t dig_len, const void *data, const uint64_t *offsets,
               const uint32_t *lengths, uint64_t n_rec, void *digests, unsigned flags, void *stream)
{
    t_err.clear();
    if (n_rec == 0)
        return BRB_BATCH_OK;
    if (!digests || !offsets || !lengths || !data) {
        set_err("NULL data, offsets, lengths or digests");
        return BRB_BATCH_BADARG;
    }
    if (!items_ok(n_rec) || !flags_ok(flags))
        return BRB_BATCH_BADARG;
    if (int ok = device_ok(); ok != BRB_BATCH_OK)
        return ok;
    if (flags & BRB_BATCH_ALL_DEVICES)   // contiguous record ranges, one per device
        return brb_host::split_devices(n_rec, [&](int, uint64_t lo, uint64_t hi) {
            return digest_var(launch, dig_len, data, offsets + lo, lengths + lo, hi - lo, bytes(digests) + lo * dig_len,
                              flags & ~BRB_BATCH_ALL_DEVICES, nullptr);
        });
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (flags & BRB_BATCH_DEVICE)
        return device_run(launch(bytes(data), offsets, lengths, n_rec, bytes(digests), s), s, flags);
    // host mode: copy the byte range the records cover, rebased to its first byte
    const Span sp = span_rebase(offsets, lengths, n_rec);
    if (!sp.ok)
        return BRB_BATCH_BADARG;
    Staging st;
    const size_t i_d = st.in(bytes(data) + sp.lo, sp.bytes());
    const size_t i_o = st.in(sp.off.data(), 8 * n_rec);
    const size_t i_l = st.in(lengths, 4 * n_rec);
    const size_t i_out = st.out(digests, dig_len * n_rec);
    return st.run(s, nullptr, [&] {
        return launched(launch(st.dev(i_d), st.dev<uint64_t>(i_o), st.dev<uint32_t>(i_l), n_rec, st.dev(i_out), s));
    });
}

// ---- streaming digest contexts as a batch (digest_stream_kernels.hip) --------------------------
// BRB_MD5{Init,Update,Final}Batch and the BrbSha1_ three.  Item i acts on ctxs[ctx_index ? ctx_index[i] : i].
// Host mode checks the index list before anything runs, stages only the named contexts (gathered in
// item order, so the kernel runs without an index, and scattered back after it) and, for Update, the
// pieces' span.  No wave-pair kernel: no fault word.
enum StreamOp { kStreamInit, kStreamUpdate, kStreamFinal };

int digest_stream(bool sha1, StreamOp op, void *ctxs, uint64_t n_ctx, const uint32_t *ctx_index, const void *data,
                  const uint64_t *offsets, const uint32_t *lengths, uint64_t n, void *digests, unsigned flags, void *stream)
{
    t_err.clear();
    if (n == 0)
        return BRB_BATCH_OK;
    if (!ctxs || (op == kStreamUpdate && (!offsets || !lengths)) || (op == kStreamFinal && sha1 && !digests)) {
        set_err(op == kStreamUpdate ? "NULL ctxs, offsets or lengths" : op == kStreamFinal ? "NULL ctxs or digests" : "NULL ctxs");
        return BRB_BATCH_BADARG;
    }
    if (!items_ok(n) || !flags_ok(flags))
        return BRB_BATCH_BADARG;
    const size_t stride = sha1 ? sizeof(BrbSha1Ctx) : sizeof(BRB_MD5_CTX), dig = sha1 ? 20 : 16;
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto launch = [&](uint8_t *c, const uint32_t *ix, const uint8_t *d, const uint64_t *o, const uint32_t *l, uint8_t *dg) {
        return op == kStreamInit     ? brb::launch_digest_stream_init(sha1, c, ix, n, s)
               : op == kStreamUpdate ? brb::launch_digest_stream_update(sha1, c, ix, d, o, l, n, s)
                                     : brb::launch_digest_stream_final(sha1, c, ix, n, dg, s);
    };
    if (flags & BRB_BATCH_DEVICE) {
        if (int ok = device_ok(); ok != BRB_BATCH_OK)
            return ok;
        return device_run(launch(bytes(ctxs), ctx_index, bytes(data), offsets, lengths, bytes(digests)), s, flags);
    }
    // host mode: every list is host memory and is checked before anything runs
    NamedCtx named{bytes(ctxs), ctx_index, n, stride, {}};
    if (!named.ok(n_ctx, "two pieces of one chain in one call is a race"))
        return BRB_BATCH_BADARG;
    Span sp;
    if (op == kStreamUpdate) {
        sp = span_rebase(offsets, lengths, n);
        if (!sp.ok)
            return BRB_BATCH_BADARG;
        if (!data && sp.bytes()) {
            set_err("NULL data with a piece that has bytes");
            return BRB_BATCH_BADARG;
        }
    }
    if (int ok = device_ok(); ok != BRB_BATCH_OK)
        return ok;
    if (flags & BRB_BATCH_ALL_DEVICES)   // contiguous item ranges, one per device; the contexts go with their items
        return brb_host::split_devices(n, [&](int, uint64_t lo, uint64_t hi) {
            return digest_stream(sha1, op, ctx_index ? ctxs : bytes(ctxs) + lo * stride, ctx_index ? n_ctx : n_ctx - lo,
                                 ctx_index ? ctx_index + lo : nullptr, data, offsets ? offsets + lo : nullptr,
                                 lengths ? lengths + lo : nullptr, hi - lo, digests ? bytes(digests) + lo * dig : nullptr,
                                 flags & ~BRB_BATCH_ALL_DEVICES, nullptr);
        });
    Staging st;
    const size_t i_c = st.inout(named.gather(), n * stride);
    const size_t i_d = op == kStreamUpdate ? st.in(data ? bytes(data) + sp.lo : nullptr, sp.bytes()) : 0;
    const size_t i_o = op == kStreamUpdate ? st.in(sp.off.data(), 8 * n) : 0;
    const size_t i_l = op == kStreamUpdate ? st.in(lengths, 4 * n) : 0;
    const size_t i_g = op == kStreamFinal && digests ? st.out(digests, dig * n) : 0;
    return named.scatter(st.run(s, nullptr, [&] {
        return launched(launch(st.dev(i_c), nullptr, st.dev(i_d), st.dev<uint64_t>(i_o), st.dev<uint32_t>(i_l),
                               op == kStreamFinal && digests ? st.dev(i_g) : nullptr));
    }));
}

// BRB_MD5UpdateSegmentsBatch / BrbSha1_UpdateSegmentsBatch: item i advances ctxs[ctx_index ? ctx_index[i] : i] by
// the segments first[i] .. first[i + 1] - 1 and is then finalised when fin && fin[i].  digest_stream's index checks
// and context staging, BRB_MD5BatchSegments' segment staging; the digests are staged in both directions, so the rows
// of items that are not finalised keep the caller's bytes.  lower (BRB_MD5UpdateSegmentsLowerBatch, MD5 only): segment
// k is taken as BRB_MD5UpdateLowerText when slow[k] != 0, every segment when slow is NULL; slow is staged over the
// named segment range like the lengths.
int digest_stream_segments(bool sha1, void *ctxs, uint64_t n_ctx, const uint32_t *ctx_index, const void *data,
                           const uint64_t *soff, const uint32_t *slen, const uint64_t *first, uint64_t n,
                           const uint8_t *fin, void *digests, unsigned flags, void *stream, bool lower = false,
                           const uint8_t *slow = nullptr)
{
    t_err.clear();
    if (n == 0)
        return BRB_BATCH_OK;
    if (!ctxs || !soff || !slen || !first || (sha1 && fin && !digests)) {
        set_err("NULL ctxs, seg_offsets, seg_lengths, item_first_seg or digests");
        return BRB_BATCH_BADARG;
    }
    if (!items_ok(n) || !flags_ok(flags))
        return BRB_BATCH_BADARG;
    const size_t stride = sha1 ? sizeof(BrbSha1Ctx) : sizeof(BRB_MD5_CTX), dig = sha1 ? 20 : 16;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!fin)
        digests = nullptr;                           // no item is finalised: not used
    auto launch = [&](uint8_t *c, const uint32_t *ix, const uint8_t *d, const uint64_t *o, const uint32_t *l, const uint8_t *w,
                      const uint64_t *f, const uint8_t *fi, uint8_t *dg) {
        return lower ? brb::launch_md5_stream_segments_lower(c, ix, d, o, l, w, f, n, fi, dg, s)
                     : brb::launch_digest_stream_segments(sha1, c, ix, d, o, l, f, n, fi, dg, s);
    };
    if (flags & BRB_BATCH_DEVICE) {
        if (int ok = device_ok(); ok != BRB_BATCH_OK)
            return ok;
        return device_run(launch(bytes(ctxs), ctx_index, bytes(data), soff, slen, slow, first, fin, bytes(digests)), s, flags);
    }
    // host mode: every list is host memory and is checked before anything runs
    NamedCtx named{bytes(ctxs), ctx_index, n, stride, {}};
    if (!named.ok(n_ctx, "a chain's pieces of one call go in its segment list"))
        return BRB_BATCH_BADARG;
    const FirstList fl = first_list(first, n, "item_first_seg");
    if (!fl.ok)
        return BRB_BATCH_BADARG;
    const uint64_t k0 = fl.k0, nseg = fl.count;
    const Span sp = span_rebase(soff + k0, slen + k0, nseg);
    if (!sp.ok)
        return BRB_BATCH_BADARG;
    if (!data && sp.bytes()) {
        set_err("NULL data with a segment that has bytes");
        return BRB_BATCH_BADARG;
    }
    if (int ok = device_ok(); ok != BRB_BATCH_OK)
        return ok;
    if (flags & BRB_BATCH_ALL_DEVICES)   // contiguous item ranges, one per device; contexts and segment lists go with them
        return brb_host::split_devices(n, [&](int, uint64_t lo, uint64_t hi) {
            return digest_stream_segments(sha1, ctx_index ? ctxs : bytes(ctxs) + lo * stride, ctx_index ? n_ctx : n_ctx - lo,
                                          ctx_index ? ctx_index + lo : nullptr, data, soff, slen, first + lo, hi - lo,
                                          fin ? fin + lo : nullptr, digests ? bytes(digests) + lo * dig : nullptr,
                                          flags & ~BRB_BATCH_ALL_DEVICES, nullptr, lower, slow);
        });
    const std::vector<uint64_t> rfirst = fl.rebased();
    Staging st;
    const size_t i_c = st.inout(named.gather(), n * stride);
    const size_t i_d = st.in(data ? bytes(data) + sp.lo : nullptr, sp.bytes());
    const size_t i_o = st.in(sp.off.data(), 8 * nseg);
    const size_t i_l = st.in(slen + k0, 4 * nseg);
    const size_t i_w = slow ? st.in(slow + k0, nseg) : 0;
    const size_t i_f = st.in(rfirst.data(), 8 * (n + 1));
    const size_t i_n = fin ? st.in(fin, n) : 0;
    const size_t i_g = digests ? st.inout(digests, dig * n) : 0;
    return named.scatter(st.run(s, nullptr, [&] {
        return launched(launch(st.dev(i_c), nullptr, st.dev(i_d), st.dev<uint64_t>(i_o), st.dev<uint32_t>(i_l),
                               slow ? st.dev(i_w) : nullptr, st.dev<uint64_t>(i_f), fin ? st.dev(i_n) : nullptr,
                               digests ? st.dev(i_g) : nullptr));
    }));
}

// BRB_MD5LowerTextBatch (md5_lower_kernels.hip): digests[i] and / or strings[i] of key i lower-cased.  BRB_MD5Batch's
// flags and modes; the host-mode checks -- every list is host memory there -- come before anything runs, and the
// outputs are fixed-stride rows, so all-devices always splits.  No wave-pair kernel: no fault word.
int md5_lower_text(const void *data, const uint64_t *offsets, const uint32_t *lengths, uint64_t n, void *digests,
                   void *strings, unsigned flags, void *stream)
{
    t_err.clear();
    if (n == 0)
        return BRB_BATCH_OK;
    if (!offsets || !lengths) {
        set_err("NULL offsets or lengths");
        return BRB_BATCH_BADARG;
    }
    if (!digests && !strings) {
        set_err("NULL digests and strings: nothing to write");
        return BRB_BATCH_BADARG;
    }
    if (!items_ok(n) || !flags_ok(flags))
        return BRB_BATCH_BADARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (flags & BRB_BATCH_DEVICE) {
        if (int ok = device_ok(); ok != BRB_BATCH_OK)
            return ok;
        return device_run(brb::launch_md5_lower(bytes(data), offsets, lengths, n, bytes(digests), bytes(strings), s), s, flags);
    }
    // host mode: the span of the non-empty keys, rebased to its first byte
    const Span sp = span_rebase(offsets, lengths, n);
    if (!sp.ok)
        return BRB_BATCH_BADARG;
    if (!data && sp.bytes()) {
        set_err("NULL data with a key that has bytes");
        return BRB_BATCH_BADARG;
    }
    if (int ok = device_ok(); ok != BRB_BATCH_OK)
        return ok;
    if (flags & BRB_BATCH_ALL_DEVICES)   // contiguous key ranges, one per device
        return brb_host::split_devices(n, [&](int, uint64_t lo, uint64_t hi) {
            return md5_lower_text(data, offsets + lo, lengths + lo, hi - lo, digests ? bytes(digests) + lo * 16 : nullptr,
                                  strings ? bytes(strings) + lo * 33 : nullptr, flags & ~BRB_BATCH_ALL_DEVICES, nullptr);
        });
    Staging st;
    const size_t i_d = st.in(data ? bytes(data) + sp.lo : nullptr, sp.bytes());
    const size_t i_o = st.in(sp.off.data(), 8 * n);
    const size_t i_l = st.in(lengths, 4 * n);
    const size_t i_g = digests ? st.out(digests, 16 * n) : 0;
    const size_t i_s = strings ? st.out(strings, 33 * n) : 0;
    return st.run(s, nullptr, [&] {
        return launched(brb::launch_md5_lower(st.dev(i_d), st.dev<uint64_t>(i_o), st.dev<uint32_t>(i_l), n,
                                              digests ? st.dev(i_g) : nullptr, strings ? st.dev(i_s) : nullptr, s));
    });
}

int blowfish_batch(const BRB_BLOWFISH_CTX *ctx, unsigned long *words, uint64_t n_blocks, unsigned flags,
                   void *stream, bool decrypt)
{
    t_err.clear();
    if (n_blocks == 0)
        return BRB_BATCH_OK;
    if (!ctx || !words) {
        set_err("NULL ctx or words");
        return BRB_BATCH_BADARG;
    }
    if (!flags_ok(flags))
        return BRB_BATCH_BADARG;
    if (int ok = device_ok(); ok != BRB_BATCH_OK)
        return ok;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint64_t *w = reinterpret_cast<uint64_t *>(words);
    if (flags & BRB_BATCH_DEVICE)
        return device_run(brb::launch_blowfish(reinterpret_cast<const uint64_t *>(ctx), w, n_blocks, decrypt, s), s, flags);
    return brb_host::blowfish(ctx, w, n_blocks, decrypt, flags, s);
}

// ---- key setup (EvAIOReqTransform_CryptoEnable for many keys; keysetup_kernels.hip) -----------
// blowfish: BRB_Blowfish_InitBatch (8336-byte contexts, 72 key bytes used); else BRB_RC4_InitBatch
// (264-byte states, 256 key bytes used).  Outputs are fixed-stride, so BRB_BATCH_ALL_DEVICES always
// splits into contiguous ranges.  No wave-pair kernel: no fault word.
int keysetup_batch(bool blowfish, void *out, const void *keys, const uint64_t *koffs, const uint32_t *klens, uint64_t n,
                   unsigned flags, void *stream)
{
    t_err.clear();
    if (n == 0)
        return BRB_BATCH_OK;
    if (!out || !keys || !koffs || !klens) {
        set_err("NULL %s, keys, key_offsets or key_lengths", blowfish ? "ctxs" : "states");
        return BRB_BATCH_BADARG;
    }
    if (!items_ok(n) || !flags_ok(flags))
        return BRB_BATCH_BADARG;
    const size_t stride = blowfish ? sizeof(BRB_BLOWFISH_CTX) : sizeof(BRB_RC4_State);
    const uint32_t used_max = blowfish ? 72u : 256u;
    std::vector<uint32_t> used;                 // host mode: the key bytes the schedule reads
    if (!(flags & BRB_BATCH_DEVICE)) {
        used.resize(n);
        for (uint64_t i = 0; i < n; i++) {
            if (klens[i] == 0) {
                set_err("key %llu: zero length", (unsigned long long)i);
                return BRB_BATCH_BADARG;
            }
            used[i] = std::min(klens[i], used_max);
        }
    }
    if (int ok = device_ok(); ok != BRB_BATCH_OK)
        return ok;
    if (flags & BRB_BATCH_ALL_DEVICES)   // contiguous key ranges, one per device
        return brb_host::split_devices(n, [&](int, uint64_t lo, uint64_t hi) {
            return keysetup_batch(blowfish, bytes(out) + lo * stride, keys, koffs + lo, klens + lo, hi - lo,
                                  flags & ~BRB_BATCH_ALL_DEVICES, nullptr);
        });
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto launch = [&](uint8_t *o, const uint8_t *k, const uint64_t *off, const uint32_t *len) {
        return blowfish ? brb::launch_blowfish_keysetup(reinterpret_cast<uint64_t *>(o), k, off, len, n, s)
                        : brb::launch_rc4_keysetup(o, k, off, len, n, s);
    };
    if (flags & BRB_BATCH_DEVICE)
        return device_run(launch(bytes(out), bytes(keys), koffs, klens), s, flags);
    // host mode: the span of the key bytes read, with the offsets rebased to it and the lengths clamped
    // to the bytes used (the same schedule: RC4 indexes key[k % len] with k < 256, Blowfish takes 72 bytes)
    const Span sp = span_rebase(koffs, used.data(), n);
    if (!sp.ok)
        return BRB_BATCH_BADARG;
    Staging st;
    const size_t i_k = st.in(bytes(keys) + sp.lo, sp.bytes());
    const size_t i_o = st.in(sp.off.data(), 8 * n);
    const size_t i_l = st.in(used.data(), 4 * n);
    const size_t i_out = st.out(out, stride * n);
    return st.run(s, nullptr, [&] {
        return launched(launch(st.dev(i_out), st.dev(i_k), st.dev<uint64_t>(i_o), st.dev<uint32_t>(i_l)));
    });
}

// ---- base64 --------------------------------------------------------------------
int b64_batch(bool decode, const void *in, const uint64_t *offs, const uint32_t *lens, uint64_t n, void *out,
              const uint64_t *ooffs, uint32_t *olens, unsigned flags, void *stream)
{
    t_err.clear();
    if (n == 0)
        return BRB_BATCH_OK;
    if (!in || !offs || !lens || !out || !ooffs || (decode && !olens)) {
        set_err("NULL data, offsets, lengths, out, out_offsets or out_lengths");
        return BRB_BATCH_BADARG;
    }
    if (!items_ok(n) || !flags_ok(flags))
        return BRB_BATCH_BADARG;
    if (int ok = device_ok(); ok != BRB_BATCH_OK)
        return ok;
    // host mode (the lengths are host memory): the mean length, and the output extents -- encode
    // 4 * ceil(len / 3), decode at most 3 * (len / 4)
    uint64_t mean_len = 0;                      // unknown in device mode
    std::vector<uint32_t> omax;
    if (!(flags & BRB_BATCH_DEVICE)) {
        omax.resize(n);
        uint64_t sum = 0;
        for (uint64_t i = 0; i < n; i++) {
            sum += lens[i];
            omax[i] = decode ? 3u * (lens[i] / 4) : 4u * ((lens[i] + 2) / 3);
        }
        mean_len = sum / n + 1;
    }
    if (flags & BRB_BATCH_ALL_DEVICES) {   // outputs are written back: their spans must not interleave
        flags &= ~BRB_BATCH_ALL_DEVICES;
        if (parts_disjoint(ooffs, omax.data(), n, 0))
            return brb_host::split_devices(n, [&](int, uint64_t lo, uint64_t hi) {
                return b64_batch(decode, in, offs + lo, lens + lo, hi - lo, out, ooffs + lo, olens ? olens + lo : nullptr,
                                 flags, nullptr);
            });
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto launch = [&](const uint8_t *i, const uint64_t *o, const uint32_t *l, uint8_t *d, const uint64_t *oo,
                      uint32_t *ol) {
        return decode ? brb::launch_b64_decode(i, o, l, n, d, oo, ol, mean_len, s)
                      : brb::launch_b64_encode(i, o, l, n, d, oo, mean_len, s);
    };
    if (flags & BRB_BATCH_DEVICE)
        return device_run(launch(bytes(in), offs, lens, bytes(out), ooffs, olens), s, flags);
    // the outputs are staged in both directions, so the bytes between them survive
    const Span si = span_rebase(offs, lens, n), so = span_rebase(ooffs, omax.data(), n);
    if (!si.ok || !so.ok)
        return BRB_BATCH_BADARG;
    Staging st;
    const size_t i_in = st.in(bytes(in) + si.lo, si.bytes());
    const size_t i_out = st.inout(bytes(out) + so.lo, so.bytes());
    const size_t i_o = st.in(si.off.data(), 8 * n);
    const size_t i_l = st.in(lens, 4 * n);
    const size_t i_oo = st.in(so.off.data(), 8 * n);
    const size_t i_ol = decode ? st.out(olens, 4 * n) : 0;
    return st.run(s, nullptr, [&] {
        return launched(launch(st.dev(i_in), st.dev<uint64_t>(i_o), st.dev<uint32_t>(i_l), st.dev(i_out),
                               st.dev<uint64_t>(i_oo), decode ? st.dev<uint32_t>(i_ol) : nullptr));
    });
}

// ---- MemBuffer Blowfish -------------------------------------------------------
int membuf_crypt(void *buf, unsigned long size, unsigned int seed, unsigned long offset, unsigned long *new_size,
                 unsigned flags, void *stream, bool decrypt)
{
    t_err.clear();
    if (!buf || !new_size) {
        set_err("NULL buf or new_size");
        return BRB_BATCH_BADARG;
    }
    if (decrypt && size < offset) {
        set_err("size %lu < offset %lu (the reference would walk ~2^61 words)", size, offset);
        return BRB_BATCH_BADARG;
    }
    const bool device = (flags & BRB_BATCH_DEVICE) != 0;
    uint8_t *raw = bytes(buf) + offset;
    if (device && (reinterpret_cast<uintptr_t>(raw) & 7)) {
        set_err("device mode needs buf + offset 8-byte aligned");
        return BRB_BATCH_BADARG;
    }
    if (int ok = device_ok(); ok != BRB_BATCH_OK)
        return ok;
    // host side: key (mem_buf.c:1511-1515) and the reference's keyLen quirk (:1528 vs :1582)
    unsigned int key[16];
    BRB_MemBufferKey(seed, key);
    BRB_BLOWFISH_CTX *ctx = static_cast<BRB_BLOWFISH_CTX *>(malloc(sizeof(BRB_BLOWFISH_CTX)));
    if (!ctx) {
        set_err("out of host memory");
        return BRB_BATCH_NOT_DONE;
    }
    BRB_Blowfish_Init(ctx, reinterpret_cast<unsigned char *>(key), decrypt ? int(sizeof(key)) : int(sizeof(key[0])));
    const uint64_t words = (decrypt ? (size - offset) : (size + offset)) / 8 + 2;
    const uint64_t pairs = (words + 1) / 2;
    hipStream_t s = static_cast<hipStream_t>(stream);
    Staging st;
    const size_t i_ctx = st.in(ctx, sizeof(BRB_BLOWFISH_CTX));
    const size_t i_first = st.scratch(8);
    const size_t i_w = device ? 0 : st.inout(raw, size_t(16) * pairs);
    unsigned long long done = pairs;
    // device mode stages the context alone and synchronises too (ASYNC is ignored)
    const int rc = st.run(s, nullptr, [&] {
        uint64_t *w = device ? reinterpret_cast<uint64_t *>(raw) : st.dev<uint64_t>(i_w);
        if (decrypt) {                                 // stop at the first all-zero pair: its index, read back
            unsigned long long *first = st.dev<unsigned long long>(i_first);
            hipError_t e;
            if ((e = hipMemcpyAsync(first, &done, 8, hipMemcpyHostToDevice, s)) != hipSuccess)
                return fail_hip("hipMemcpyAsync H2D", e);
            if (int r = launched(brb::launch_first_zero_pair(w, pairs, first, s)); r != BRB_BATCH_OK)
                return r;
            if ((e = hipMemcpyAsync(&done, first, 8, hipMemcpyDeviceToHost, s)) != hipSuccess ||
                (e = hipStreamSynchronize(s)) != hipSuccess)
                return fail_hip("zero-pair scan", e);
        }
        return launched(brb::launch_blowfish(st.dev<uint64_t>(i_ctx), w, done, decrypt, s));
    });
    free(ctx);
    if (rc == BRB_BATCH_OK)
        *new_size = static_cast<unsigned long>(16 * done + offset);
    return rc;
}

// ---- Blowfish ECB with a context per record (blowfish_keyed_kernels.hip) -----------------------
// No wave-pair kernel: no fault word.
int blowfish_keyed(const BRB_BLOWFISH_CTX *ctxs, uint64_t n_ctx, const uint32_t *ctx_index, unsigned long *words,
                   const uint64_t *woffs, const uint32_t *counts, uint64_t n, unsigned flags, void *stream, bool decrypt)
{
    t_err.clear();
    if (n == 0)
        return BRB_BATCH_OK;
    if (!ctxs || !words || !woffs || !counts) {
        set_err("NULL ctxs, words, word_offsets or block_counts");
        return BRB_BATCH_BADARG;
    }
    if (!flags_ok(flags))
        return BRB_BATCH_BADARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (flags & BRB_BATCH_DEVICE) {
        if ((reinterpret_cast<uintptr_t>(words) | reinterpret_cast<uintptr_t>(ctxs)) & 7) {
            set_err("device mode needs words and ctxs 8-byte aligned");
            return BRB_BATCH_BADARG;
        }
        if (int ok = device_ok(); ok != BRB_BATCH_OK)
            return ok;
        return device_run(brb::launch_blowfish_keyed(reinterpret_cast<const uint64_t *>(ctxs), ctx_index,
                                                     reinterpret_cast<uint64_t *>(words), woffs, counts, n, decrypt, nullptr, s),
                          s, flags);
    }
    // host mode: every list is host memory and is checked before anything runs
    if (!ctx_index && n_ctx != n) {
        set_err("ctx_index is NULL and n_ctx (%llu) != n_rec (%llu)", (unsigned long long)n_ctx, (unsigned long long)n);
        return BRB_BATCH_BADARG;
    }
    std::vector<uint64_t> boff(n), blen(n);          // the records in bytes
    for (uint64_t i = 0; i < n; i++) {
        if (ctx_index && ctx_index[i] >= n_ctx) {
            set_err("record %llu: ctx_index %u out of range (%llu contexts)", (unsigned long long)i, ctx_index[i],
                    (unsigned long long)n_ctx);
            return BRB_BATCH_BADARG;
        }
        if (woffs[i] > UINT64_MAX / 8) {
            set_err("record %llu: word offset %llu wraps", (unsigned long long)i, (unsigned long long)woffs[i]);
            return BRB_BATCH_BADARG;
        }
        boff[i] = 8 * woffs[i];
        blen[i] = 16 * uint64_t(counts[i]);
    }
    Span sp = span_rebase(boff.data(), blen.data(), n);
    if (!sp.ok)
        return BRB_BATCH_BADARG;
    if (int ok = device_ok(); ok != BRB_BATCH_OK)
        return ok;
    if (flags & BRB_BATCH_ALL_DEVICES) {   // records are written back: their spans must not interleave
        flags &= ~BRB_BATCH_ALL_DEVICES;
        if (parts_disjoint(boff.data(), blen.data(), n, 0))
            return brb_host::split_devices(n, [&](int, uint64_t a, uint64_t b) {
                return blowfish_keyed(ctx_index ? ctxs : ctxs + a, ctx_index ? n_ctx : b - a,
                                      ctx_index ? ctx_index + a : nullptr, words, woffs + a, counts + a, b - a, flags,
                                      nullptr, decrypt);
            });
    }
    // the contexts the records with blocks name, compacted in index order (runs of neighbours = one copy)
    std::vector<uint32_t> cidx(n, 0);
    std::vector<uint64_t> used;
    used.reserve(n);
    for (uint64_t i = 0; i < n; i++)
        if (counts[i])
            used.push_back(ctx_index ? ctx_index[i] : i);
    std::sort(used.begin(), used.end());
    used.erase(std::unique(used.begin(), used.end()), used.end());
    for (uint64_t i = 0; i < n; i++)
        if (counts[i])
            cidx[i] = uint32_t(std::lower_bound(used.begin(), used.end(), ctx_index ? ctx_index[i] : i) - used.begin());
    for (uint64_t &o : sp.off)
        o /= 8;                                      // lo is a record's start: the differences are whole words
    Staging st;
    const size_t i_w = st.inout(bytes(words) + sp.lo, sp.bytes());
    const size_t i_o = st.in(sp.off.data(), 8 * n);
    const size_t i_c = st.in(counts, 4 * n);
    const size_t i_x = st.in(cidx.data(), 4 * n);
    const size_t i_ctx = st.scratch(sizeof(BRB_BLOWFISH_CTX) * std::max<size_t>(used.size(), 1));
    return st.run(s, nullptr, [&] {
        for (size_t a = 0, b; a < used.size(); a = b) {      // one copy per run of neighbouring contexts
            b = a + 1;
            while (b < used.size() && used[b] == used[b - 1] + 1)
                b++;
            const hipError_t e = hipMemcpyAsync(st.dev<BRB_BLOWFISH_CTX>(i_ctx) + a, ctxs + used[a],
                                                sizeof(BRB_BLOWFISH_CTX) * (b - a), hipMemcpyHostToDevice, s);
            if (e != hipSuccess)
                return fail_hip("hipMemcpyAsync H2D", e);
        }
        return launched(brb::launch_blowfish_keyed(st.dev<uint64_t>(i_ctx), st.dev<uint32_t>(i_x), st.dev<uint64_t>(i_w),
                                                   st.dev<uint64_t>(i_o), st.dev<uint32_t>(i_c), n, decrypt, nullptr, s));
    });
}

// ---- MemBuffer Blowfish as a batch ---------------------------------------------------------------
// One key-setup launch for the n_seeds seeds into the thread's workspace, a plan (host mode: on the
// host; device mode: a kernel), one keyed launch, one synchronisation.  The contexts live in the
// workspace, so device mode synchronises too (ASYNC is ignored, as by the single calls).
int membuf_batch(void *data, const uint64_t *buf_offsets, const uint64_t *sizes, const uint64_t *offsets,
                 const unsigned int *seeds, uint64_t n_seeds, const uint32_t *seed_index, uint64_t n, uint64_t *new_sizes,
                 unsigned flags, void *stream, bool decrypt)
{
    t_err.clear();
    if (n == 0)
        return BRB_BATCH_OK;
    if (!data || !buf_offsets || !sizes || !seeds || !new_sizes) {
        set_err("NULL data, buf_offsets, sizes, seeds or new_sizes");
        return BRB_BATCH_BADARG;
    }
    if (!flags_ok(flags))
        return BRB_BATCH_BADARG;
    if (n_seeds == 0 || (!seed_index && n_seeds != 1 && n_seeds != n)) {
        set_err("n_seeds %llu with %s seed_index (%llu buffers)", (unsigned long long)n_seeds, seed_index ? "a" : "NULL",
                (unsigned long long)n);
        return BRB_BATCH_BADARG;
    }
    const bool device = (flags & BRB_BATCH_DEVICE) != 0;
    if (device && (reinterpret_cast<uintptr_t>(data) & 7)) {
        set_err("device mode needs data 8-byte aligned (and every buf_offsets[i] + offsets[i])");
        return BRB_BATCH_BADARG;
    }
    // host mode: the plan, checked before anything runs
    std::vector<uint64_t> woffs, starts;
    std::vector<uint32_t> counts, idx;
    std::vector<uint8_t> stage;
    if (!device) {
        woffs.resize(n);
        starts.resize(n);
        counts.resize(n);
        idx.resize(n);
        uint64_t total = 0;
        for (uint64_t i = 0; i < n; i++) {
            const uint64_t off = offsets ? offsets[i] : 0;
            if (decrypt && sizes[i] < off) {
                set_err("buffer %llu: size %llu < offset %llu (the reference would walk ~2^61 words)", (unsigned long long)i,
                        (unsigned long long)sizes[i], (unsigned long long)off);
                return BRB_BATCH_BADARG;
            }
            const uint64_t si = seed_index ? uint64_t(seed_index[i]) : (n_seeds == 1 ? 0 : i);
            if (si >= n_seeds) {
                set_err("buffer %llu: seed_index %llu out of range (%llu seeds)", (unsigned long long)i,
                        (unsigned long long)si, (unsigned long long)n_seeds);
                return BRB_BATCH_BADARG;
            }
            if (!decrypt && sizes[i] > UINT64_MAX - off) {
                set_err("buffer %llu: size + offset wraps", (unsigned long long)i);
                return BRB_BATCH_BADARG;
            }
            const uint64_t pairs = (((decrypt ? sizes[i] - off : sizes[i] + off) >> 3) + 3) >> 1;
            if (pairs > UINT32_MAX) {
                set_err("buffer %llu: %llu pairs (at most 2^32 - 1 per buffer)", (unsigned long long)i,
                        (unsigned long long)pairs);
                return BRB_BATCH_BADARG;
            }
            starts[i] = buf_offsets[i] + off;
            woffs[i] = total / 8;
            counts[i] = uint32_t(pairs);
            idx[i] = uint32_t(si);
            total += 16 * pairs;
        }
        stage.resize(std::max<uint64_t>(total, 16));   // 8-byte aligned staging whatever the buffers' alignment
    }
    if (int ok = device_ok(); ok != BRB_BATCH_OK)
        return ok;
    // keys (mem_buf.c:1511-1515) and the reference's keyLen quirk (:1528 vs :1582)
    std::vector<unsigned int> keys(16 * n_seeds);
    std::vector<uint64_t> koffs(n_seeds);
    std::vector<uint32_t> klens(n_seeds, decrypt ? 64u : 4u);
    for (uint64_t k = 0; k < n_seeds; k++) {
        BRB_MemBufferKey(seeds[k], &keys[16 * k]);
        koffs[k] = 64 * k;
    }
    if (!device)
        for (uint64_t i = 0; i < n; i++)
            memcpy(stage.data() + 8 * woffs[i], bytes(data) + starts[i], 16 * size_t(counts[i]));
    std::vector<uint32_t> done(device || !decrypt ? 0 : n);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Staging st;
    const size_t i_k = st.in(keys.data(), 64 * n_seeds);
    const size_t i_ko = st.in(koffs.data(), 8 * n_seeds);
    const size_t i_kl = st.in(klens.data(), 4 * n_seeds);
    const size_t i_ctx = st.scratch(sizeof(BRB_BLOWFISH_CTX) * n_seeds);
    const size_t i_o = st.in(device ? nullptr : woffs.data(), 8 * n);      // device mode: the plan kernel writes these
    const size_t i_c = st.in(device ? nullptr : counts.data(), 4 * n);
    const size_t i_x = st.in(device ? nullptr : idx.data(), 4 * n);
    const size_t i_d = st.out(done.empty() ? nullptr : done.data(), 4 * n);   // host-mode decrypt: the stops
    const size_t i_w = device ? 0 : st.inout(stage.data(), stage.size());
    const int rc = st.run(s, nullptr, [&] {
        uint64_t *w = device ? static_cast<uint64_t *>(data) : st.dev<uint64_t>(i_w), *d_o = st.dev<uint64_t>(i_o);
        uint32_t *d_c = st.dev<uint32_t>(i_c), *d_x = st.dev<uint32_t>(i_x), *d_d = st.dev<uint32_t>(i_d);
        int r = launched(brb::launch_blowfish_keysetup(st.dev<uint64_t>(i_ctx), st.dev(i_k), st.dev<uint64_t>(i_ko),
                                                       st.dev<uint32_t>(i_kl), n_seeds, s));
        if (r == BRB_BATCH_OK && device)
            r = launched(brb::launch_membuf_plan(buf_offsets, sizes, offsets, seed_index, n_seeds, n, decrypt, d_o, d_c, d_x,
                                                 new_sizes, s));
        if (r == BRB_BATCH_OK)
            r = launched(brb::launch_blowfish_keyed(st.dev<uint64_t>(i_ctx), d_x, w, d_o, d_c, n, decrypt,
                                                    decrypt ? d_d : nullptr, s));
        if (r == BRB_BATCH_OK && device && decrypt)
            r = launched(brb::launch_membuf_finish(d_d, offsets, n, new_sizes, s));
        return r;
    });
    if (rc != BRB_BATCH_OK || device)
        return rc;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t did = decrypt ? done[i] : counts[i];    // bytes from the stop onward are not written
        memcpy(bytes(data) + starts[i], stage.data() + 8 * woffs[i], 16 * size_t(did));
        new_sizes[i] = 16 * did + (offsets ? offsets[i] : 0);
    }
    return rc;
}

// ---- RC4, RC4+MD5 frame and RC4+MD5 open (rc4_kernels.hip, rc4_list_kernels.hip) -------------------
// BRB_RC4_CryptBatch, BRB_RC4MD5_FrameBatch, BRB_RC4MD5_OpenBatch (a buffer per stream) and their List forms
// (stream i owns buffers first[i] .. first[i + 1] - 1 of the per-buffer arrays).  `c` holds the caller's
// arguments as the launch takes them (brb::Rc4Launch; ooffs = the frame offsets), so device mode launches it
// as it stands.  Host mode stages, of buffers [fl.k0, fl.k0 + fl.count): the n states and the outputs' span in
// both directions, the inputs' span (sp; frames: sf) and the lengths, salts and rebased offsets in, valid out.
// The single-buffer form is the list form over buffers [0, n) with no list staged (rfirst NULL).
int rc4_stage(const brb::Rc4Launch &c, const FirstList &fl, const Span &sp, const Span &sf, const uint64_t *rfirst,
              const PairFault *pf, hipStream_t s)
{
    const bool frame = c.kind == BRB_RC4_KIND_FRAME, open = c.kind == BRB_RC4_KIND_OPEN;
    const uint64_t n = c.n, k0 = fl.k0, count = fl.count;
    const Span &so = frame ? sf : sp;               // crypt and open write at the inputs' offsets in `out`
    Staging st;
    const size_t i_st = st.inout(c.states, sizeof(BRB_RC4_State) * n);
    const InOut io = stage_in_out(st, !frame && c.in == c.out, c.in + sp.lo, sp.bytes(), c.out + so.lo, so.bytes());
    const size_t i_off = st.in(sp.off.data(), 8 * count);
    const size_t i_fo = frame ? st.in(sf.off.data(), 8 * count) : 0;
    const size_t i_len = st.in(c.lens + k0, 4 * count);
    const size_t i_salt = frame ? st.in(c.salts + k0, 8 * count) : 0;
    const size_t i_first = rfirst ? st.in(rfirst, 8 * (n + 1)) : 0;
    const size_t i_val = open ? st.out(c.valid + k0, count) : 0;
    return st.run(s, pf, [&] {
        brb::Rc4Launch l = c;                        // the kind and the count; every pointer is the staged copy's
        l.states = st.dev(i_st);
        l.in = st.dev(io.in);
        l.out = st.dev(io.out);
        l.offs = st.dev<uint64_t>(i_off);
        l.lens = st.dev<uint32_t>(i_len);
        l.ooffs = frame ? st.dev<uint64_t>(i_fo) : nullptr;
        l.salts = frame ? st.dev<uint64_t>(i_salt) : nullptr;
        l.first = rfirst ? st.dev<uint64_t>(i_first) : nullptr;
        l.valid = open ? st.dev(i_val) : nullptr;
        return launched(brb::launch_rc4(l, s));
    });
}

// The two forms take their refusals in different orders, and each keeps its own.  A buffer per stream: NULL
// pointers, counts and flags, the device, the all-devices split, the fault word (wave-pair kernels), then
// device mode launches and host mode looks at the ranges.  List: NULL pointers, counts and flags, then device
// mode probes and launches (lone waves: no fault word) and host mode checks everything -- the list, the
// ranges -- before any device work: the device, the all-devices split, the staging.  nulls: the NULL refusal.
int rc4_batch(const brb::Rc4Launch &c, bool list, const char *nulls, unsigned flags, void *stream)
{
    t_err.clear();
    const uint64_t n = c.n;
    if (n == 0)
        return BRB_BATCH_OK;
    const bool frame = c.kind == BRB_RC4_KIND_FRAME, open = c.kind == BRB_RC4_KIND_OPEN;
    if (!c.states || !c.in || !c.out || !c.offs || !c.lens || (list && !c.first) || (frame && (!c.salts || !c.ooffs)) ||
        (open && !c.valid)) {
        set_err("%s", nulls);
        return BRB_BATCH_BADARG;
    }
    if (!items_ok(n) || !flags_ok(flags))
        return BRB_BATCH_BADARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool device = (flags & BRB_BATCH_DEVICE) != 0;
    FirstList fl{c.first, n, 0, n, true};           // a buffer per stream: buffer i is stream i's
    Span sp, sf;
    // the list form stops at the first range that wraps; the other looks at both spans (the later text stands)
    auto spans = [&] {
        sp = span_rebase(c.offs + fl.k0, c.lens + fl.k0, fl.count);
        if (frame && (sp.ok || !list))
            sf = span_rebase(c.ooffs + fl.k0, c.lens + fl.k0, fl.count, BRB_RC4MD5_HEADER);
        return sp.ok && (!frame || sf.ok);
    };
    if (list && !device) {
        fl = first_list(c.first, n, "stream_first_buf", true);
        if (!fl.ok || !spans())
            return BRB_BATCH_BADARG;
    }
    if (int ok = device_ok(); ok != BRB_BATCH_OK)
        return ok;
    if (list && device)
        return device_run(brb::launch_rc4(c, s), s, flags);
    if (flags & BRB_BATCH_ALL_DEVICES) {   // streams split over the devices, their states and buffers with them
        flags &= ~BRB_BATCH_ALL_DEVICES;
        // what a part writes is copied back: the parts' spans (frames: of the frames) must not interleave
        const uint64_t *woffs = frame ? c.ooffs : c.offs;
        const uint64_t extra = frame ? BRB_RC4MD5_HEADER : 0;
        if (list ? stream_parts_disjoint(woffs, c.lens, c.first, n, extra) : parts_disjoint(woffs, c.lens, n, extra))
            return brb_host::split_devices(n, [&](int, uint64_t lo, uint64_t hi) {
                brb::Rc4Launch p = c;
                p.states += lo * sizeof(BRB_RC4_State);
                p.n = hi - lo;
                if (list) {
                    p.first += lo;                   // the per-buffer arrays stay: the list names the part's range
                } else {
                    p.offs += lo;
                    p.lens += lo;
                    p.ooffs = frame ? c.ooffs + lo : nullptr;
                    p.salts = frame ? c.salts + lo : nullptr;
                    p.valid = open ? c.valid + lo : nullptr;
                }
                return rc4_batch(p, list, nulls, flags, nullptr);
            });
    }
    if (list)
        return rc4_stage(c, fl, sp, sf, fl.rebased().data(), nullptr, s);
    const PairFault pf(flags);                       // pair_fault.h
    if (int ok = pf.ready(); ok != BRB_BATCH_OK)
        return ok;
    if (device)
        return device_run(brb::launch_rc4(c, s), s, flags, &pf);
    if (!spans())
        return BRB_BATCH_BADARG;
    return rc4_stage(c, fl, sp, sf, nullptr, &pf, s);
}

// the caller's arguments of the six calls as a launch; the wrappers add salts, frame offsets and valid
brb::Rc4Launch rc4_args(int kind, BRB_RC4_State *states, const void *in, void *out, const uint64_t *offs,
                        const uint32_t *lens, const uint64_t *first, uint64_t n)
{
    brb::Rc4Launch c;
    c.kind = kind;
    c.states = reinterpret_cast<uint8_t *>(states);
    c.in = bytes(in);
    c.out = bytes(out);
    c.offs = offs;
    c.lens = lens;
    c.first = first;
    c.n = n;
    return c;
}

}  // namespace

extern "C" {

// Streams of mixed kind (rc4_mixed_kernels.hip): stream i is of kind[i] and uses states[sidx ? sidx[i] : i].
// Host mode: NamedCtx stages the named states densely, so the kernel runs without an index; the inputs'
// span in, the outputs' span in both directions (one span when the call works in place), valid over the
// named buffers in both directions, so the entries of buffers that are not OPEN keep the caller's bytes.
int BRB_RC4_MixedListBatch(BRB_RC4_State *states, uint64_t n_states, const uint32_t *sidx, const uint8_t *kind,
                           const void *in, void *out, const uint64_t *offsets, const uint32_t *lengths,
                           const uint64_t *out_offsets, const uint64_t *salts, const uint64_t *first, uint64_t n,
                           uint8_t *valid, unsigned flags, void *stream)
{
    t_err.clear();
    if (n == 0)
        return BRB_BATCH_OK;
    if (!states || !kind || !in || !out || !offsets || !lengths || !out_offsets || !first) {
        set_err("NULL states, stream_kind, in, out, buf_offsets, buf_lengths, out_offsets or stream_first_buf");
        return BRB_BATCH_BADARG;
    }
    if (flags & BRB_BATCH_ALL_DEVICES) {
        set_err("BRB_RC4_MixedListBatch does not split over devices: call it per device");
        return BRB_BATCH_BADARG;
    }
    if (!items_ok(n) || !flags_ok(flags))
        return BRB_BATCH_BADARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (flags & BRB_BATCH_DEVICE) {
        if (int ok = device_ok(); ok != BRB_BATCH_OK)
            return ok;
        brb::Rc4Launch l = rc4_args(0, states, in, out, offsets, lengths, first, n);
        l.kinds = kind;
        l.sidx = sidx;
        l.ooffs = out_offsets;
        l.salts = salts;
        l.valid = valid;
        return device_run(brb::launch_rc4(l, s), s, flags);
    }
    // host mode: every list is host memory and is checked before anything runs
    bool any_frame = false, any_open = false;
    for (uint64_t i = 0; i < n; i++) {
        if (kind[i] > BRB_RC4_KIND_OPEN) {
            set_err("stream %llu: kind %u (0 crypt, 1 frame, 2 open)", (unsigned long long)i, unsigned(kind[i]));
            return BRB_BATCH_BADARG;
        }
        any_frame |= kind[i] == BRB_RC4_KIND_FRAME;
        any_open |= kind[i] == BRB_RC4_KIND_OPEN;
    }
    if ((any_frame && !salts) || (any_open && !valid)) {
        set_err(any_frame && !salts ? "NULL salts with a FRAME stream" : "NULL valid with an OPEN stream");
        return BRB_BATCH_BADARG;
    }
    const FirstList fl = first_list(first, n, "stream_first_buf", true);
    if (!fl.ok)
        return BRB_BATCH_BADARG;
    const uint64_t k0 = fl.k0, count = fl.count;
    const std::vector<uint64_t> rfirst = fl.rebased();
    NamedCtx named{bytes(states), sidx, n, sizeof(BRB_RC4_State), {}};
    if (!named.ok(n_states, "a connection's buffers of one call go in its stream's list"))
        return BRB_BATCH_BADARG;
    std::vector<uint64_t> olen(count);   // bytes written per buffer
    for (uint64_t i = 0; i < n; i++)
        for (uint64_t k = rfirst[i]; k < rfirst[i + 1]; k++)
            olen[k] = uint64_t(lengths[k0 + k]) + (kind[i] == BRB_RC4_KIND_FRAME ? BRB_RC4MD5_HEADER : 0);
    Span sp = span_rebase(offsets + k0, lengths + k0, count);
    if (!sp.ok)
        return BRB_BATCH_BADARG;
    Span so = span_rebase(out_offsets + k0, olen.data(), count);
    if (!so.ok)
        return BRB_BATCH_BADARG;
    if (int ok = device_ok(); ok != BRB_BATCH_OK)
        return ok;
    const bool in_place = in == out && sp.bytes() && so.bytes();
    if (in_place) {   // one span, staged in both directions
        const uint64_t lo = std::min(sp.lo, so.lo), hi = std::max(sp.hi, so.hi);
        for (uint64_t k = 0; k < count; k++) {
            sp.off[k] += lengths[k0 + k] ? sp.lo - lo : 0;
            so.off[k] += olen[k] ? so.lo - lo : 0;
        }
        sp.lo = so.lo = lo;
        sp.hi = so.hi = hi;
    }
    Staging st;
    const size_t i_st = st.inout(named.gather(), sizeof(BRB_RC4_State) * n);
    const InOut io = stage_in_out(st, in_place, bytes(in) + sp.lo, sp.bytes(), bytes(out) + so.lo, so.bytes());
    const size_t i_off = st.in(sp.off.data(), 8 * count);
    const size_t i_ooff = st.in(so.off.data(), 8 * count);
    const size_t i_len = st.in(lengths + k0, 4 * count);
    const size_t i_salt = any_frame ? st.in(salts + k0, 8 * count) : 0;
    const size_t i_first = st.in(rfirst.data(), 8 * (n + 1));
    const size_t i_kind = st.in(kind, n);
    const size_t i_val = any_open ? st.inout(valid + k0, count) : 0;
    return named.scatter(st.run(s, nullptr, [&] {
        brb::Rc4Launch l;
        l.kinds = st.dev(i_kind);
        l.states = st.dev(i_st);
        l.in = st.dev(io.in);
        l.out = st.dev(io.out);
        l.offs = st.dev<uint64_t>(i_off);
        l.lens = st.dev<uint32_t>(i_len);
        l.ooffs = st.dev<uint64_t>(i_ooff);
        l.salts = any_frame ? st.dev<uint64_t>(i_salt) : nullptr;
        l.first = st.dev<uint64_t>(i_first);
        l.n = n;
        l.valid = any_open ? st.dev(i_val) : nullptr;
        return launched(brb::launch_rc4(l, s));
    }));
}

int BRB_MD5BatchSegments(const void *data, const uint64_t *soff, const uint32_t *slen, const uint64_t *first, uint64_t n_rec,
                         unsigned char (*digests)[16], unsigned flags, void *stream)
{
    t_err.clear();
    if (n_rec == 0)
        return BRB_BATCH_OK;
    if (!digests || !first || (!data || !soff || !slen)) {
        set_err("NULL data, seg_offsets, seg_lengths, rec_first_seg or digests");
        return BRB_BATCH_BADARG;
    }
    if (!items_ok(n_rec) || !flags_ok(flags))
        return BRB_BATCH_BADARG;
    if (int ok = device_ok(); ok != BRB_BATCH_OK)
        return ok;
    if (flags & BRB_BATCH_ALL_DEVICES)   // contiguous record ranges (segment lists with them), one per device
        return brb_host::split_devices(n_rec, [&](int, uint64_t lo, uint64_t hi) {
            return BRB_MD5BatchSegments(data, soff, slen, first + lo, hi - lo, digests + lo, flags & ~BRB_BATCH_ALL_DEVICES,
                                        nullptr);
        });
    hipStream_t s = static_cast<hipStream_t>(stream);
    const PairFault pf(flags);                       // pair_fault.h
    if (int ok = pf.ready(); ok != BRB_BATCH_OK)
        return ok;
    if (flags & BRB_BATCH_DEVICE)
        return device_run(brb::launch_md5_segments(bytes(data), soff, slen, first, n_rec, bytes(digests), s), s, flags, &pf);
    // host mode: rebase the segment lists to start at 0 and copy the byte span they cover
    const FirstList fl = first_list(first, n_rec, "rec_first_seg");
    if (!fl.ok)
        return BRB_BATCH_BADARG;
    const uint64_t k0 = fl.k0, nseg = fl.count;
    const Span sp = span_rebase(soff + k0, slen + k0, nseg);
    if (!sp.ok)
        return BRB_BATCH_BADARG;
    const std::vector<uint64_t> rfirst = fl.rebased();
    Staging st;
    const size_t i_d = st.in(bytes(data) + sp.lo, sp.bytes());
    const size_t i_o = st.in(sp.off.data(), 8 * nseg);
    const size_t i_l = st.in(slen + k0, 4 * nseg);
    const size_t i_f = st.in(rfirst.data(), 8 * (n_rec + 1));
    const size_t i_out = st.out(digests, 16 * n_rec);
    return st.run(s, &pf, [&] {
        return launched(brb::launch_md5_segments(st.dev(i_d), st.dev<uint64_t>(i_o), st.dev<uint32_t>(i_l),
                                                 st.dev<uint64_t>(i_f), n_rec, st.dev(i_out), s));
    });
}

// ---- MetaData packs ------------------------------------------------------------
int BRB_MetaDataUnpackBatch(const void *data, const uint64_t *offs, const uint32_t *lens, uint64_t n,
                            BRB_MetaDataUnpackInfo *info, unsigned flags, void *stream)
{
    t_err.clear();
    if (n == 0)
        return BRB_BATCH_OK;
    if (!data || !offs || !lens || !info) {
        set_err("NULL data, offsets, lengths or info");
        return BRB_BATCH_BADARG;
    }
    if (!items_ok(n) || !flags_ok(flags))
        return BRB_BATCH_BADARG;
    if (int ok = device_ok(); ok != BRB_BATCH_OK)
        return ok;
    if (flags & BRB_BATCH_ALL_DEVICES)   // contiguous pack ranges, one per device
        return brb_host::split_devices(n, [&](int, uint64_t lo, uint64_t hi) {
            return BRB_MetaDataUnpackBatch(data, offs + lo, lens + lo, hi - lo, info + lo, flags & ~BRB_BATCH_ALL_DEVICES,
                                           nullptr);
        });
    hipStream_t s = static_cast<hipStream_t>(stream);
    const PairFault pf(flags);                       // pair_fault.h
    if (int ok = pf.ready(); ok != BRB_BATCH_OK)
        return ok;
    if (flags & BRB_BATCH_DEVICE)
        return device_run(brb::launch_metadata_unpack(bytes(data), offs, lens, n, info, s), s, flags, &pf);
    // host mode: copy the byte span the packs cover, with the offsets rebased to it
    const Span sp = span_rebase(offs, lens, n);
    if (!sp.ok)
        return BRB_BATCH_BADARG;
    Staging st;
    const size_t i_d = st.in(bytes(data) + sp.lo, sp.bytes());
    const size_t i_o = st.in(sp.off.data(), 8 * n);
    const size_t i_l = st.in(lens, 4 * n);
    const size_t i_out = st.out(info, sizeof(BRB_MetaDataUnpackInfo) * n);
    return st.run(s, &pf, [&] {
        return launched(brb::launch_metadata_unpack(st.dev(i_d), st.dev<uint64_t>(i_o), st.dev<uint32_t>(i_l), n,
                                                    st.dev<BRB_MetaDataUnpackInfo>(i_out), s));
    });
}

// MetaDataUnpack with the item table.  Host mode stages the four item arrays over the slots the call
// owns, [first[0], first[n]), in both directions -- slots no item reaches keep their values -- and
// passes the staged span's base to the kernel, so item offsets are offsets in the caller's data.
int BRB_MetaDataUnpackItemsBatch(const void *data, const uint64_t *offs, const uint32_t *lens, uint64_t n,
                                 BRB_MetaDataUnpackInfo *info, uint64_t *ioff, uint32_t *ilen, uint64_t *iid,
                                 uint64_t *isub, const uint64_t *first, uint32_t *added, unsigned flags, void *stream)
{
    t_err.clear();
    if (n == 0)
        return BRB_BATCH_OK;
    if (!data || !offs || !lens || !info || !ioff || !ilen || !iid || !isub || !first || !added) {
        set_err("NULL data, offsets, lengths, info, item_offsets, item_lengths, item_ids, item_sub_ids, pack_first_slot "
                "or items_added");
        return BRB_BATCH_BADARG;
    }
    if (!items_ok(n) || !flags_ok(flags))
        return BRB_BATCH_BADARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (flags & BRB_BATCH_DEVICE) {
        if (int ok = device_ok(); ok != BRB_BATCH_OK)
            return ok;
        const PairFault pf(flags);                   // pair_fault.h
        if (int ok = pf.ready(); ok != BRB_BATCH_OK)
            return ok;
        return device_run(brb::launch_metadata_unpack_items(bytes(data), 0, offs, lens, n, info, ioff, ilen, iid, isub,
                                                            first, added, s),
                          s, flags, &pf);
    }
    // host mode: the slot list and the packs' span are host memory, so they are checked before anything runs
    const FirstList fl = first_list(first, n, "pack_first_slot");
    if (!fl.ok)
        return BRB_BATCH_BADARG;
    const Span sp = span_rebase(offs, lens, n);
    if (!sp.ok)
        return BRB_BATCH_BADARG;
    if (int ok = device_ok(); ok != BRB_BATCH_OK)
        return ok;
    if (flags & BRB_BATCH_ALL_DEVICES)   // contiguous pack ranges, one per device; their slot ranges go with them
        return brb_host::split_devices(n, [&](int, uint64_t lo, uint64_t hi) {
            return BRB_MetaDataUnpackItemsBatch(data, offs + lo, lens + lo, hi - lo, info + lo, ioff, ilen, iid, isub,
                                                first + lo, added + lo, flags & ~BRB_BATCH_ALL_DEVICES, nullptr);
        });
    const PairFault pf(flags);
    if (int ok = pf.ready(); ok != BRB_BATCH_OK)
        return ok;
    const uint64_t k0 = fl.k0, nslot = fl.count;
    const std::vector<uint64_t> rfirst = fl.rebased();
    Staging st;
    const size_t i_d = st.in(bytes(data) + sp.lo, sp.bytes());
    const size_t i_o = st.in(sp.off.data(), 8 * n);
    const size_t i_l = st.in(lens, 4 * n);
    const size_t i_info = st.out(info, sizeof(BRB_MetaDataUnpackInfo) * n);
    const size_t i_io = st.inout(ioff + k0, 8 * nslot);
    const size_t i_il = st.inout(ilen + k0, 4 * nslot);
    const size_t i_id = st.inout(iid + k0, 8 * nslot);
    const size_t i_sub = st.inout(isub + k0, 8 * nslot);
    const size_t i_f = st.in(rfirst.data(), 8 * (n + 1));
    const size_t i_add = st.out(added, 4 * n);
    return st.run(s, &pf, [&] {
        return launched(brb::launch_metadata_unpack_items(
            st.dev(i_d), sp.lo, st.dev<uint64_t>(i_o), st.dev<uint32_t>(i_l), n, st.dev<BRB_MetaDataUnpackInfo>(i_info),
            st.dev<uint64_t>(i_io), st.dev<uint32_t>(i_il), st.dev<uint64_t>(i_id), st.dev<uint64_t>(i_sub),
            st.dev<uint64_t>(i_f), st.dev<uint32_t>(i_add), s));
    });
}

// MetaDataPack of n packs (metadata_pack_kernels.hip).  Host mode validates the item lists, stages the
// span of the items and -- in both directions, so the bytes between packs survive -- the span of the
// packs, as b64_batch stages its outputs.
int BRB_MetaDataPackBatch(const void *data, const uint64_t *ioff, const uint32_t *ilen, const uint64_t *iid,
                          const uint64_t *isub, const uint64_t *first, uint64_t n, void *out, const uint64_t *ooff,
                          unsigned flags, void *stream)
{
    t_err.clear();
    if (n == 0)
        return BRB_BATCH_OK;
    if (!data || !ioff || !ilen || !iid || !isub || !first || !out || !ooff) {
        set_err("NULL data, item_offsets, item_lengths, item_ids, item_sub_ids, pack_first_item, out or out_offsets");
        return BRB_BATCH_BADARG;
    }
    if (!items_ok(n) || !flags_ok(flags))
        return BRB_BATCH_BADARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (flags & BRB_BATCH_DEVICE) {
        if (int ok = device_ok(); ok != BRB_BATCH_OK)
            return ok;
        return device_run(brb::launch_metadata_pack(bytes(data), ioff, ilen, iid, isub, first, n, bytes(out), ooff, s), s,
                          flags);
    }
    // host mode: the item lists are host memory, so they are checked before anything runs
    std::vector<uint32_t> plen(n);              // pack sizes (a pack the unpack call can take: a uint32 length)
    const FirstList fl = first_list(first, n, "pack_first_item", [&](uint64_t p) {   // per pack, in the list's order
        if (first[p + 1] - first[p] > uint64_t(INT32_MAX)) {
            set_err("pack %llu: %llu items (the header's item count is an int)", (unsigned long long)p,
                    (unsigned long long)(first[p + 1] - first[p]));
            return false;
        }
        uint64_t size = BRB_METADATA_HEADER_SIZE;
        for (uint64_t k = first[p]; k < first[p + 1]; k++)
            size += uint64_t(ilen[k]) + BRB_METADATA_ITEM_RAW_SIZE + 1;
        if (size > UINT32_MAX) {
            set_err("pack %llu: %llu bytes (host mode packs at most 4 GiB - 1, the unpack call's length)",
                    (unsigned long long)p, (unsigned long long)size);
            return false;
        }
        plen[p] = uint32_t(size);
        return true;
    });
    if (!fl.ok)
        return BRB_BATCH_BADARG;
    if (int ok = device_ok(); ok != BRB_BATCH_OK)
        return ok;
    if (flags & BRB_BATCH_ALL_DEVICES) {   // packs are written back: their spans must not interleave
        flags &= ~BRB_BATCH_ALL_DEVICES;
        if (parts_disjoint(ooff, plen.data(), n, 0))
            return brb_host::split_devices(n, [&](int, uint64_t lo, uint64_t hi) {
                return BRB_MetaDataPackBatch(data, ioff, ilen, iid, isub, first + lo, hi - lo, out, ooff + lo, flags, nullptr);
            });
    }
    const uint64_t k0 = fl.k0, nitem = fl.count;
    const Span si = span_rebase(ioff + k0, ilen + k0, nitem), so = span_rebase(ooff, plen.data(), n);
    if (!si.ok || !so.ok)
        return BRB_BATCH_BADARG;
    const std::vector<uint64_t> rfirst = fl.rebased();
    Staging st;
    const size_t i_d = st.in(bytes(data) + si.lo, si.bytes());
    const size_t i_out = st.inout(bytes(out) + so.lo, so.bytes());
    const size_t i_o = st.in(si.off.data(), 8 * nitem);
    const size_t i_l = st.in(ilen + k0, 4 * nitem);
    const size_t i_id = st.in(iid + k0, 8 * nitem);
    const size_t i_sub = st.in(isub + k0, 8 * nitem);
    const size_t i_f = st.in(rfirst.data(), 8 * (n + 1));
    const size_t i_oo = st.in(so.off.data(), 8 * n);
    return st.run(s, nullptr, [&] {
        return launched(brb::launch_metadata_pack(st.dev(i_d), st.dev<uint64_t>(i_o), st.dev<uint32_t>(i_l),
                                                  st.dev<uint64_t>(i_id), st.dev<uint64_t>(i_sub), st.dev<uint64_t>(i_f), n,
                                                  st.dev(i_out), st.dev<uint64_t>(i_oo), s));
    });
}

// ---- the calls that add a launcher or a direction to a shared implementation --------------------
int BRB_MD5BatchFixed(const void *data, uint32_t rec_len, uint64_t n_rec, unsigned char (*digests)[16], unsigned flags,
                      void *hip_stream)
{
    return digest_fixed(brb::launch_md5_fixed, 16, data, rec_len, n_rec, digests, flags, hip_stream);
}

int BRB_MD5Batch(const void *data, const uint64_t *offsets, const uint32_t *lengths, uint64_t n_rec,
                 unsigned char (*digests)[16], unsigned flags, void *hip_stream)
{
    return digest_var(brb::launch_md5_var, 16, data, offsets, lengths, n_rec, digests, flags, hip_stream);
}

int BrbSha1_BatchFixed(const void *data, uint32_t rec_len, uint64_t n_rec, uint8_t (*digests)[20], unsigned flags,
                       void *hip_stream)
{
    return digest_fixed(brb::launch_sha1_fixed, 20, data, rec_len, n_rec, digests, flags, hip_stream);
}

int BrbSha1_Batch(const void *data, const uint64_t *offsets, const uint32_t *lengths, uint64_t n_rec,
                  uint8_t (*digests)[20], unsigned flags, void *hip_stream)
{
    return digest_var(brb::launch_sha1_var, 20, data, offsets, lengths, n_rec, digests, flags, hip_stream);
}

int BRB_MD5InitBatch(BRB_MD5_CTX *ctxs, uint64_t n_ctx, const uint32_t *ctx_index, uint64_t n, unsigned flags,
                     void *hip_stream)
{
    return digest_stream(false, kStreamInit, ctxs, n_ctx, ctx_index, nullptr, nullptr, nullptr, n, nullptr, flags, hip_stream);
}

int BRB_MD5UpdateBatch(BRB_MD5_CTX *ctxs, uint64_t n_ctx, const uint32_t *ctx_index, const void *data,
                       const uint64_t *offsets, const uint32_t *lengths, uint64_t n, unsigned flags, void *hip_stream)
{
    return digest_stream(false, kStreamUpdate, ctxs, n_ctx, ctx_index, data, offsets, lengths, n, nullptr, flags, hip_stream);
}

int BRB_MD5FinalBatch(BRB_MD5_CTX *ctxs, uint64_t n_ctx, const uint32_t *ctx_index, uint64_t n,
                      unsigned char (*digests)[16], unsigned flags, void *hip_stream)
{
    return digest_stream(false, kStreamFinal, ctxs, n_ctx, ctx_index, nullptr, nullptr, nullptr, n, digests, flags, hip_stream);
}

int BrbSha1_InitBatch(BrbSha1Ctx *ctxs, uint64_t n_ctx, const uint32_t *ctx_index, uint64_t n, unsigned flags,
                      void *hip_stream)
{
    return digest_stream(true, kStreamInit, ctxs, n_ctx, ctx_index, nullptr, nullptr, nullptr, n, nullptr, flags, hip_stream);
}

int BrbSha1_UpdateBatch(BrbSha1Ctx *ctxs, uint64_t n_ctx, const uint32_t *ctx_index, const void *data,
                        const uint64_t *offsets, const uint32_t *lengths, uint64_t n, unsigned flags, void *hip_stream)
{
    return digest_stream(true, kStreamUpdate, ctxs, n_ctx, ctx_index, data, offsets, lengths, n, nullptr, flags, hip_stream);
}

int BrbSha1_FinalBatch(BrbSha1Ctx *ctxs, uint64_t n_ctx, const uint32_t *ctx_index, uint64_t n, uint8_t (*digests)[20],
                       unsigned flags, void *hip_stream)
{
    return digest_stream(true, kStreamFinal, ctxs, n_ctx, ctx_index, nullptr, nullptr, nullptr, n, digests, flags, hip_stream);
}

int BRB_MD5UpdateSegmentsBatch(BRB_MD5_CTX *ctxs, uint64_t n_ctx, const uint32_t *ctx_index, const void *data,
                               const uint64_t *seg_offsets, const uint32_t *seg_lengths, const uint64_t *item_first_seg,
                               uint64_t n, const uint8_t *final, unsigned char (*digests)[16], unsigned flags,
                               void *hip_stream)
{
    return digest_stream_segments(false, ctxs, n_ctx, ctx_index, data, seg_offsets, seg_lengths, item_first_seg, n, final,
                                  digests, flags, hip_stream);
}

int BRB_MD5UpdateSegmentsLowerBatch(BRB_MD5_CTX *ctxs, uint64_t n_ctx, const uint32_t *ctx_index, const void *data,
                                    const uint64_t *seg_offsets, const uint32_t *seg_lengths, const uint8_t *seg_lower,
                                    const uint64_t *item_first_seg, uint64_t n, const uint8_t *final,
                                    unsigned char (*digests)[16], unsigned flags, void *hip_stream)
{
    return digest_stream_segments(false, ctxs, n_ctx, ctx_index, data, seg_offsets, seg_lengths, item_first_seg, n, final,
                                  digests, flags, hip_stream, true, seg_lower);
}

int BRB_MD5LowerTextBatch(const void *data, const uint64_t *offsets, const uint32_t *lengths, uint64_t n,
                          unsigned char (*digests)[16], char (*strings)[33], unsigned flags, void *hip_stream)
{
    return md5_lower_text(data, offsets, lengths, n, digests, strings, flags, hip_stream);
}

int BrbSha1_UpdateSegmentsBatch(BrbSha1Ctx *ctxs, uint64_t n_ctx, const uint32_t *ctx_index, const void *data,
                                const uint64_t *seg_offsets, const uint32_t *seg_lengths, const uint64_t *item_first_seg,
                                uint64_t n, const uint8_t *final, uint8_t (*digests)[20], unsigned flags, void *hip_stream)
{
    return digest_stream_segments(true, ctxs, n_ctx, ctx_index, data, seg_offsets, seg_lengths, item_first_seg, n, final,
                                  digests, flags, hip_stream);
}

int BRB_Base64EncodeBatch(const void *data, const uint64_t *offsets, const uint32_t *lengths, uint64_t n, void *out,
                          const uint64_t *out_offsets, unsigned flags, void *hip_stream)
{
    return b64_batch(false, data, offsets, lengths, n, out, out_offsets, nullptr, flags, hip_stream);
}

int BRB_Base64DecodeBatch(const void *text, const uint64_t *offsets, const uint32_t *lengths, uint64_t n, void *out,
                          const uint64_t *out_offsets, uint32_t *out_lengths, unsigned flags, void *hip_stream)
{
    return b64_batch(true, text, offsets, lengths, n, out, out_offsets, out_lengths, flags, hip_stream);
}

int BRB_RC4_InitBatch(BRB_RC4_State *states, const void *keys, const uint64_t *key_offsets, const uint32_t *key_lengths,
                      uint64_t n_keys, unsigned flags, void *hip_stream)
{
    return keysetup_batch(false, states, keys, key_offsets, key_lengths, n_keys, flags, hip_stream);
}

int BRB_Blowfish_InitBatch(BRB_BLOWFISH_CTX *ctxs, const void *keys, const uint64_t *key_offsets,
                           const uint32_t *key_lengths, uint64_t n_keys, unsigned flags, void *hip_stream)
{
    return keysetup_batch(true, ctxs, keys, key_offsets, key_lengths, n_keys, flags, hip_stream);
}

int BRB_RC4_CryptBatch(BRB_RC4_State *states, const void *in, void *out, const uint64_t *offsets, const uint32_t *lengths,
                       uint64_t n, unsigned flags, void *hip_stream)
{
    return rc4_batch(rc4_args(BRB_RC4_KIND_CRYPT, states, in, out, offsets, lengths, nullptr, n), false,
                     "NULL states, in, out, offsets or lengths", flags, hip_stream);
}

int BRB_RC4MD5_FrameBatch(BRB_RC4_State *states, const void *payload, const uint64_t *offsets, const uint32_t *lengths,
                          const uint64_t *salts, void *frames, const uint64_t *frame_offsets, uint64_t n, unsigned flags,
                          void *hip_stream)
{
    brb::Rc4Launch c = rc4_args(BRB_RC4_KIND_FRAME, states, payload, frames, offsets, lengths, nullptr, n);
    c.salts = salts;
    c.ooffs = frame_offsets;
    return rc4_batch(c, false, "NULL states, payload, offsets, lengths, salts, frames or frame_offsets", flags, hip_stream);
}

int BRB_RC4MD5_OpenBatch(BRB_RC4_State *states, const void *frames, void *out, const uint64_t *offsets,
                         const uint32_t *lengths, uint64_t n, uint8_t *valid, unsigned flags, void *hip_stream)
{
    brb::Rc4Launch c = rc4_args(BRB_RC4_KIND_OPEN, states, frames, out, offsets, lengths, nullptr, n);
    c.valid = valid;
    return rc4_batch(c, false, "NULL states, frames, out, offsets, lengths or valid", flags, hip_stream);
}

int BRB_RC4_CryptListBatch(BRB_RC4_State *states, const void *in, void *out, const uint64_t *buf_offsets,
                           const uint32_t *buf_lengths, const uint64_t *stream_first_buf, uint64_t n, unsigned flags,
                           void *hip_stream)
{
    return rc4_batch(rc4_args(BRB_RC4_KIND_CRYPT, states, in, out, buf_offsets, buf_lengths, stream_first_buf, n), true,
                     "NULL states, in, out, buf_offsets, buf_lengths or stream_first_buf", flags, hip_stream);
}

int BRB_RC4MD5_FrameListBatch(BRB_RC4_State *states, const void *payload, const uint64_t *buf_offsets,
                              const uint32_t *buf_lengths, const uint64_t *salts, void *frames, const uint64_t *frame_offsets,
                              const uint64_t *stream_first_buf, uint64_t n, unsigned flags, void *hip_stream)
{
    brb::Rc4Launch c = rc4_args(BRB_RC4_KIND_FRAME, states, payload, frames, buf_offsets, buf_lengths, stream_first_buf, n);
    c.salts = salts;
    c.ooffs = frame_offsets;
    return rc4_batch(c, true, "NULL states, payload, buf_offsets, buf_lengths, salts, frames, frame_offsets or stream_first_buf",
                     flags, hip_stream);
}

int BRB_RC4MD5_OpenListBatch(BRB_RC4_State *states, const void *frames, void *out, const uint64_t *buf_offsets,
                             const uint32_t *buf_lengths, const uint64_t *stream_first_buf, uint64_t n, uint8_t *valid,
                             unsigned flags, void *hip_stream)
{
    brb::Rc4Launch c = rc4_args(BRB_RC4_KIND_OPEN, states, frames, out, buf_offsets, buf_lengths, stream_first_buf, n);
    c.valid = valid;
    return rc4_batch(c, true, "NULL states, frames, out, buf_offsets, buf_lengths, stream_first_buf or valid", flags,
                     hip_stream);
}

int BRB_Blowfish_EncryptBatch(const BRB_BLOWFISH_CTX *ctx, unsigned long *words, uint64_t n_blocks, unsigned flags,
                              void *hip_stream)
{
    return blowfish_batch(ctx, words, n_blocks, flags, hip_stream, false);
}

int BRB_Blowfish_DecryptBatch(const BRB_BLOWFISH_CTX *ctx, unsigned long *words, uint64_t n_blocks, unsigned flags,
                              void *hip_stream)
{
    return blowfish_batch(ctx, words, n_blocks, flags, hip_stream, true);
}

int BRB_Blowfish_EncryptBatchKeyed(const BRB_BLOWFISH_CTX *ctxs, uint64_t n_ctx, const uint32_t *ctx_index,
                                   unsigned long *words, const uint64_t *word_offsets, const uint32_t *block_counts,
                                   uint64_t n_rec, unsigned flags, void *hip_stream)
{
    return blowfish_keyed(ctxs, n_ctx, ctx_index, words, word_offsets, block_counts, n_rec, flags, hip_stream, false);
}

int BRB_Blowfish_DecryptBatchKeyed(const BRB_BLOWFISH_CTX *ctxs, uint64_t n_ctx, const uint32_t *ctx_index,
                                   unsigned long *words, const uint64_t *word_offsets, const uint32_t *block_counts,
                                   uint64_t n_rec, unsigned flags, void *hip_stream)
{
    return blowfish_keyed(ctxs, n_ctx, ctx_index, words, word_offsets, block_counts, n_rec, flags, hip_stream, true);
}

void BRB_MemBufferKey(unsigned int seed, unsigned int key[16])
{
    for (unsigned long i = 0; i < 16; i++) {          // mem_buf.c:1511-1515 (unsigned long i)
        key[i] = static_cast<unsigned int>(((i + seed) * seed) + (13 * i));
        seed = key[i] * seed;
    }
}

int BRB_MemBufferEncrypt(void *buf, unsigned long size, unsigned int seed, unsigned long offset, unsigned long *new_size,
                         unsigned flags, void *hip_stream)
{
    return membuf_crypt(buf, size, seed, offset, new_size, flags, hip_stream, false);
}

int BRB_MemBufferDecrypt(void *buf, unsigned long size, unsigned int seed, unsigned long offset, unsigned long *new_size,
                         unsigned flags, void *hip_stream)
{
    return membuf_crypt(buf, size, seed, offset, new_size, flags, hip_stream, true);
}

int BRB_MemBufferEncryptBatch(void *data, const uint64_t *buf_offsets, const uint64_t *sizes, const uint64_t *offsets,
                              const unsigned int *seeds, uint64_t n_seeds, const uint32_t *seed_index, uint64_t n_buf,
                              uint64_t *new_sizes, unsigned flags, void *hip_stream)
{
    return membuf_batch(data, buf_offsets, sizes, offsets, seeds, n_seeds, seed_index, n_buf, new_sizes, flags, hip_stream,
                        false);
}

int BRB_MemBufferDecryptBatch(void *data, const uint64_t *buf_offsets, const uint64_t *sizes, const uint64_t *offsets,
                              const unsigned int *seeds, uint64_t n_seeds, const uint32_t *seed_index, uint64_t n_buf,
                              uint64_t *new_sizes, unsigned flags, void *hip_stream)
{
    return membuf_batch(data, buf_offsets, sizes, offsets, seeds, n_seeds, seed_index, n_buf, new_sizes, flags, hip_stream,
                        true);
}

}  // extern "C"
