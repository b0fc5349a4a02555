// host_sanitize queues: the properties of pt_queue_plan.h (see host_sanitize.cpp's header).  Every expectation here is recomputed in 64-bit
// arithmetic or derived from what the OTHER side of a producer / consumer pair computes; nothing is compared with itself.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pt_queue_plan.h"

namespace qsweep {
using namespace pt;

struct Rng
{
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    uint32_t below(uint64_t n) { return (uint32_t)(next() % n); } // n <= 2^32
    // log-uniform in [1, 2^bits)
    uint32_t log_uniform(uint32_t bits) { const uint32_t b = 1u + below(bits); const uint64_t lo = 1ull << (b - 1u); return (uint32_t)(lo + next() % lo); }
};

struct Tally
{
    unsigned long long p1_cases = 0, p1_chunks = 0, p1_static = 0, p2_cases = 0, p2_regions = 0, p2_slots = 0, p2_refused = 0, p3_cases = 0, p4_divisors = 0,
                       p4_divisions = 0, p5_cases = 0, p5_ids = 0, failures = 0;
};
static Tally g;
static uint32_t g_case[5]; // the P1 case at hand: n, grid, waves per workgroup, chunk divisor, taper
#define QCHECK(COND, ...)                                                                            \
    do {                                                                                             \
        if (!(COND))                                                                                 \
        {                                                                                            \
            if (g.failures++ < 20)                                                                   \
            {                                                                                        \
                std::fprintf(stderr, "FAIL %s: ", #COND);                                            \
                std::fprintf(stderr, __VA_ARGS__);                                                   \
                std::fprintf(stderr, " (last fetch plan: n %u grid %u wpb %u div %u taper %u)\n", g_case[0], g_case[1], g_case[2], g_case[3], g_case[4]); \
            }                                                                                        \
        }                                                                                            \
    } while (0)

// 1..4200, every 2^k - 1, 2^k, 2^k + 1 up to 2^29 - 1, `extra` log-uniform values; sorted, unique
static std::vector<uint32_t> ray_counts(Rng& rng, uint32_t extra)
{
    std::vector<uint32_t> v;
    for (uint32_t n = 1; n <= 4200u; ++n) v.push_back(n);
    for (uint32_t k = 1; k <= 29u; ++k)
        for (int d = -1; d <= 1; ++d)
        {
            const uint64_t n = (1ull << k) + d;
            if (n >= 1 && n <= (1ull << 29) - 1) v.push_back((uint32_t)n);
        }
    for (uint32_t i = 0; i < extra; ++i) v.push_back(rng.log_uniform(29));
    // found by this sweep: 14251 rays, one workgroup of one wave, chunk divisor 4, taper 2: partitions of 256 slots whose 256-ray level
    // held 64 slots, a 64-ray chunk in front of the 128-ray one (chunk_of now carries a level's remainder on to the next level)
    v.push_back(14251u);
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    return v;
}

// ---- P1
struct Chunk { uint32_t start, len; };
// chunk i of a partition, checked against its predecessor: the chunks tile the partition in order, never grow, start on multiples of 64
static bool chunk_checked(const FetchPlan& pl, uint32_t i, Chunk& c)
{
    c = Chunk{0u, 0u};
    const bool ok = chunk_of(pl, i, c.start, c.len);
    if (ok) QCHECK(c.len >= 1u && c.len <= pl.chunk && (c.start & 63u) == 0u && (uint64_t)c.start + c.len <= pl.psize, "n %u i %u start %u len %u", pl.n, i, c.start, c.len);
    return ok;
}
static void adjacent(const FetchPlan& pl, uint32_t i, const Chunk& a, const Chunk& b)
{
    QCHECK(a.start + a.len == b.start && b.len <= a.len, "n %u chunk %u [%u +%u) then [%u +%u)", pl.n, i, a.start, a.len, b.start, b.len);
}
// claim (p, i) against the clip of the partition-local chunk to the dynamic part, recomputed in 64 bits
static void claim_checked(const FetchPlan& pl, uint32_t p, uint32_t i, bool exists, const Chunk& c)
{
    const uint64_t dyn = (uint64_t)pl.n - pl.n_static, off = (uint64_t)p * pl.psize + c.start;
    uint32_t cur = 0xdeadbeefu, end = 0xdeadbeefu;
    const bool got = claim_range(pl, p, i, cur, end);
    const bool want = exists && off < dyn;
    QCHECK(got == want, "n %u p %u i %u accepted %d, expected %d", pl.n, p, i, (int)got, (int)want);
    if (got && want)
    {
        const uint64_t lo = pl.n_static + off, hi = pl.n_static + std::min(off + c.len, dyn);
        QCHECK(lo < (1ull << 32) && hi <= pl.n && cur == lo && end == hi && (cur & 63u) == 0u, "n %u p %u i %u [%u, %u) expected [%llu, %llu)", pl.n, p, i, cur, end,
               (unsigned long long)lo, (unsigned long long)hi);
    }
    if (!got) QCHECK(cur == 0xdeadbeefu && end == 0xdeadbeefu, "n %u p %u i %u: a refused claim wrote a range", pl.n, p, i);
    ++g.p1_chunks;
}
static void p1_case(Rng& rng, uint32_t n, uint32_t grid, uint32_t wpb, uint32_t div, uint32_t taper)
{
    const FetchPlan pl = fetch_plan(n, div, taper, grid, wpb);
    ++g.p1_cases;
    g_case[0] = n; g_case[1] = grid; g_case[2] = wpb; g_case[3] = div; g_case[4] = taper;
    QCHECK(pl.n == n && pl.blocks >= 1u && pl.blocks <= grid, "n %u grid %u wpb %u: blocks %u", n, grid, wpb, pl.blocks);
    QCHECK(pl.chunk >= 64u && pl.chunk <= (uint32_t)PT_CHUNK_MAX && (pl.chunk & 63u) == 0u, "n %u chunk %u", n, pl.chunk);
    const uint64_t waves = (uint64_t)pl.blocks * wpb, st64 = waves * pl.chunk;
    QCHECK(pl.n_static == std::min<uint64_t>(n, st64), "n %u grid %u wpb %u: n_static %u, waves * chunk %llu", n, grid, wpb, pl.n_static, (unsigned long long)st64);
    QCHECK((uint64_t)taper * waves * 64u < (1ull << 32), "n %u: taper product overflows", n);
    // the static ranges of the participating waves: [0, n_static) in order, then empty ones
    uint64_t pos = 0;
    for (uint32_t w = 0; w < waves; ++w)
    {
        uint32_t cur, end;
        static_range(pl, w, cur, end);
        ++g.p1_static;
        if (cur == n && end == n) QCHECK(pos == pl.n_static, "n %u wave %u is empty at %llu of %u static rays", n, w, (unsigned long long)pos, pl.n_static);
        else
        {
            QCHECK(cur == pos && end > cur && end <= pl.n_static && cur == (uint64_t)w * pl.chunk && end - cur <= pl.chunk, "n %u wave %u [%u, %u) at %llu", n, w, cur, end, (unsigned long long)pos);
            pos = end;
        }
    }
    QCHECK(pos == pl.n_static, "n %u grid %u wpb %u: static ranges end at %llu of %u", n, grid, wpb, (unsigned long long)pos, pl.n_static);
    const uint64_t dyn = (uint64_t)n - pl.n_static;
    QCHECK((pl.psize & 63u) == 0u && (uint64_t)pl.psize * kQueueHeads >= dyn, "n %u: %u partitions of %u slots for %llu rays", n, (uint32_t)kQueueHeads, pl.psize, (unsigned long long)dyn);
    if (dyn != 0) QCHECK((pl.n_static & 63u) == 0u, "n %u n_static %u", n, pl.n_static);
    // how many chunks a partition has: chunk_of is true below cnt, false from cnt on
    uint32_t lo = 0, hi = (pl.psize >> 6) + 1u; // a chunk holds at least 64 slots
    Chunk c;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; uint32_t a, b; if (chunk_of(pl, mid, a, b)) lo = mid + 1u; else hi = mid; }
    const uint32_t cnt = lo;
    QCHECK((cnt == 0u) == (pl.psize == 0u), "n %u psize %u: %u chunks", n, pl.psize, cnt);
    for (uint32_t i : {cnt, cnt + 1u, cnt + 64u, 2u * cnt + 1u, 0x7fffffffu, 0xfffffffeu, 0xffffffffu})
        if (i >= cnt) { QCHECK(!chunk_checked(pl, i, c), "n %u: chunk %u of %u exists", n, i, cnt); for (uint32_t p : {0u, 63u}) claim_checked(pl, p, i, false, c); }
    const bool exhaustive = cnt <= 4096u;
    if (exhaustive)
    {
        // every chunk of the partition, and every claim of every partition against the clip; then the accepted claims walked in queue order
        std::vector<Chunk> ch(cnt);
        for (uint32_t i = 0; i < cnt; ++i)
        {
            QCHECK(chunk_checked(pl, i, ch[i]), "n %u: chunk %u of %u missing", n, i, cnt);
            if (i) adjacent(pl, i, ch[i - 1u], ch[i]);
        }
        if (cnt) QCHECK(ch[0].start == 0u && ch[cnt - 1u].start + ch[cnt - 1u].len == pl.psize, "n %u: chunks cover [%u, %u) of %u", n, ch[0].start, ch[cnt - 1u].start + ch[cnt - 1u].len, pl.psize);
        const bool all = (uint64_t)cnt * kQueueHeads <= 16384u;
        uint64_t at = pl.n_static;
        for (uint32_t p = 0; p < kQueueHeads; ++p)
        {
            bool refused = false;
            for (uint32_t i = 0; i < cnt; ++i)
            {
                if (!all && i >= 2u && i + 2u < cnt && (uint64_t)p * pl.psize + ch[i + 2u].start < dyn && rng.below(16)) continue; // long partitions: ends, the clip's neighbourhood and 1 in 16
                claim_checked(pl, p, i, true, ch[i]);
                if (!all) continue;
                uint32_t cur, end;
                if (claim_range(pl, p, i, cur, end))
                {
                    QCHECK(!refused && cur == at && end > cur && end <= n, "n %u grid %u wpb %u div %u taper %u: claim (%u, %u) = [%u, %u) at %llu", n, grid, wpb, div, taper, p, i, cur, end, (unsigned long long)at);
                    at = end;
                }
                else refused = true;
            }
            if (all && at < n) QCHECK(at == pl.n_static + (uint64_t)(p + 1u) * pl.psize, "n %u: partition %u ends at %llu", n, p, (unsigned long long)at);
        }
        if (all) QCHECK(at == n, "n %u grid %u wpb %u div %u taper %u: claims end at %llu", n, grid, wpb, div, taper, (unsigned long long)at);
        return;
    }
    // a long partition: its first 1024 and last 2048 chunks (every tapered level lies there) one after the other, adjacent pairs in between
    Chunk prev{0u, 0u};
    auto run = [&](uint32_t from, uint32_t to) {
        for (uint32_t i = from; i < to; ++i)
        {
            QCHECK(chunk_checked(pl, i, c), "n %u: chunk %u of %u missing", n, i, cnt);
            if (i > from) adjacent(pl, i, prev, c);
            prev = c;
            for (uint32_t p : {0u, 1u, 31u, 62u, 63u, (uint32_t)((dyn - 1u) / pl.psize), rng.below(kQueueHeads)}) claim_checked(pl, p, i, true, c);
        }
    };
    run(0u, 1024u);
    QCHECK(chunk_checked(pl, 0u, c) && c.start == 0u, "n %u: first chunk starts at %u", n, c.start);
    run(cnt - 2048u, cnt);
    QCHECK(prev.start + prev.len == pl.psize, "n %u: last chunk ends at %u of %u", n, prev.start + prev.len, pl.psize);
    const uint32_t pe = (uint32_t)((dyn - 1u) / pl.psize); // the partition the queue ends in
    for (uint32_t t = 0; t < 512u; ++t)
    {
        const uint32_t i = t < 8u ? 1023u + t * ((cnt - 3072u) / 8u) : 1023u + rng.below(cnt - 3071u);
        Chunk a, b;
        QCHECK(chunk_checked(pl, i, a) && chunk_checked(pl, i + 1u, b), "n %u: chunk %u of %u missing", n, i, cnt);
        adjacent(pl, i + 1u, a, b);
        claim_checked(pl, rng.below(kQueueHeads), i, true, a);
        claim_checked(pl, pe, i + 1u, true, b);
    }
    // the clip's neighbourhood: the chunk of partition pe that holds the queue's last ray, by bisection on the starts, and its neighbours
    const uint64_t last = dyn - 1u - (uint64_t)pe * pl.psize;
    uint32_t a = 0, b = cnt;
    while (b - a > 1u) { const uint32_t mid = a + (b - a) / 2u; uint32_t s, l; chunk_of(pl, mid, s, l); if (s <= last) a = mid; else b = mid; }
    for (uint32_t i = a >= 2u ? a - 2u : 0u; i < std::min(cnt, a + 3u); ++i)
    {
        QCHECK(chunk_checked(pl, i, c), "n %u: chunk %u missing", n, i);
        for (uint32_t p : {pe, pe + 1u, pe ? pe - 1u : 0u}) if (p < kQueueHeads) claim_checked(pl, p, i, true, c);
    }
}

// ---- P2
static void p2_case(Rng& rng, uint32_t n_key, Stripes& prev)
{
    const Stripes st = stripes_for(n_key);
    ++g.p2_cases;
    QCHECK(st.log_r >= 6u && st.log_r <= 13u && st.log_k <= 6u, "n_key %u: log_r %u log_k %u", n_key, st.log_r, st.log_k);
    QCHECK(st.log_r >= prev.log_r && st.log_k >= prev.log_k, "n_key %u: log_r %u -> %u, log_k %u -> %u", n_key, prev.log_r, st.log_r, prev.log_k, st.log_k);
    prev = st;
    const uint32_t K = 1u << st.log_k;
    const uint64_t R = 1ull << st.log_r;
    for (const uint32_t cap : {n_key, n_key + 1u, n_key + (n_key >> 3) + 63u, (uint32_t)std::min<uint64_t>(0xffffffffull - kQueueDumpSlots, (uint64_t)n_key * 8u)})
    {
        // random tails, zeros among them; the regions the producers reserved, by ticket and stripe
        uint32_t tail[kTailStripes] = {};
        const uint32_t most = 1u + rng.below(5);
        for (uint32_t k = 0; k < K; ++k) tail[k] = rng.below(3) ? rng.below(most + 1u) : 0u;
        std::vector<uint64_t> bases;
        for (uint32_t k = 0; k < K; ++k)
            for (uint32_t r = 0; r < tail[k]; ++r) bases.push_back(stripe_region_base(st, r, k));
        std::sort(bases.begin(), bases.end());
        for (size_t i = 0; i < bases.size(); ++i)
        {
            QCHECK(bases[i] % R == 0 && (i == 0 || bases[i] >= bases[i - 1] + R), "n_key %u: regions at %llu and %llu overlap", n_key, (unsigned long long)(i ? bases[i - 1] : 0), (unsigned long long)bases[i]);
            ++g.p2_regions;
        }
        auto reserved = [&](uint64_t idx) {
            auto it = std::upper_bound(bases.begin(), bases.end(), idx);
            return it != bases.begin() && idx < *(it - 1) + R;
        };
        // every region up to one round past the longest stripe: first, last and a random slot, and the slots either side of it
        for (uint64_t gi = 0; gi < (uint64_t)K * (most + 1u); ++gi)
            for (const uint64_t idx : {gi * R, gi * R + R - 1u, gi * R + rng.below(R), gi * R + R})
            {
                QCHECK(stripe_valid(tail, st, (uint32_t)idx) == reserved(idx), "n_key %u slot %llu: valid %d, reserved %d", n_key, (unsigned long long)idx, (int)stripe_valid(tail, st, (uint32_t)idx), (int)reserved(idx));
                ++g.p2_slots;
            }
        // the extent: the end of the furthest reserved region, clamped
        uint32_t ext = 0;
        for (uint32_t l = 0; l < kTailStripes; ++l) ext = std::max(ext, stripe_extent(st, l, l < K ? tail[l] : 0u, cap));
        const uint64_t want = bases.empty() ? 0ull : std::min<uint64_t>(cap, bases.back() + R);
        QCHECK(ext == want, "n_key %u cap %u: extent %u, expected %llu", n_key, cap, ext, (unsigned long long)want);
        // a region that would pass the capacity is refused (the predicate only: nothing is stored)
        const uint32_t rc = (uint32_t)(((uint64_t)cap >> st.log_r) >> st.log_k);
        for (const uint32_t r : {0u, rc > 0u ? rc - 1u : 0u, rc, rc + 1u, 0x7fffffffu, 0xffffffffu})
            for (const uint32_t k : {0u, K - 1u, rng.below(K)})
            {
                const uint64_t base = stripe_region_base(st, r, k);
                const uint64_t gidx = (uint64_t)r * K + k;
                QCHECK(base == gidx * R, "n_key %u ticket %u stripe %u: base %llu", n_key, r, k, (unsigned long long)base);
                const bool fits = stripe_region_fits(st, base, cap);
                QCHECK(fits == (gidx * R + R <= (uint64_t)cap), "n_key %u cap %u ticket %u stripe %u: fits %d", n_key, cap, r, k, (int)fits);
                if (fits) QCHECK(base + R <= cap && base < (1ull << 32), "n_key %u cap %u: accepted base %llu", n_key, cap, (unsigned long long)base);
                else ++g.p2_refused;
            }
    }
}

// ---- P3
static void p3_case(uint32_t n_in, uint32_t producers, uint32_t least)
{
    const uint32_t r = region_size(n_in, producers, least);
    const uint64_t raw = (uint64_t)n_in / (std::max<uint64_t>(producers, 1u) * (uint64_t)PT_REGION_DIV);
    const uint64_t want = (std::min<uint64_t>(std::max<uint64_t>(raw, least), kQueueDumpSlots) + 63u) & ~63ull;
    ++g.p3_cases;
    QCHECK((r & 63u) == 0u && r >= ((least + 63u) & ~63u) && r <= kQueueDumpSlots && r == want, "n_in %u producers %u least %u: %u, expected %llu", n_in, producers, least, r, (unsigned long long)want);
}

// ---- P4
static void p4_divisor(Rng& rng, uint32_t d)
{
    const FastDiv f = fastdiv_make(d);
    ++g.p4_divisors;
    auto one = [&](uint32_t n) {
        const uint32_t q = fastdiv(n, f);
        QCHECK(q == n / d, "%u / %u = %u, fastdiv %u", n, d, n / d, q);
        ++g.p4_divisions;
    };
    for (const uint32_t n : {0u, 1u, d - 1u, d, d + 1u, 0x7fffffffu, 0x80000000u, 0x80000001u, 0xfffffffeu, 0xffffffffu}) one(n);
    for (int i = 0; i < 6; ++i)
    {
        const uint32_t k = rng.below(0xffffffffull / d + 1u);
        const uint64_t kd = (uint64_t)k * d;
        for (const uint64_t n : {kd - 1u, kd, kd + 1u}) if (n <= 0xffffffffull) one((uint32_t)n); // (k = 0: kd - 1 wraps past 32 bits and is skipped)
        one((uint32_t)rng.next());
        one(rng.log_uniform(32));
    }
    const uint32_t top = 0xffffffffu / d;
    for (const uint64_t n : {(uint64_t)top * d - 1u, (uint64_t)top * d, (uint64_t)top * d + 1u}) if (n <= 0xffffffffull) one((uint32_t)n);
}

// ---- P5
static void p5_case(Rng& rng, uint32_t act_pixels, uint32_t count)
{
    RenderParams rp{};
    rp.act_pixels = act_pixels;
    rp.batch_samples = count;
    rp.n_paths = act_pixels * count;
    pid_block_layout(rp);
    ++g.p5_cases;
    const uint32_t B = 1u << rp.blk_log;
    QCHECK(B <= (uint32_t)PT_PID_BLOCK && B <= count && (2u * B > count || B == (uint32_t)PT_PID_BLOCK), "count %u: blocks of %u", count, B);
    QCHECK(rp.n_blk == (count + B - 1u) / B && rp.blk_last >= 1u && rp.blk_last <= B && (rp.n_blk - 1u) * B + rp.blk_last == count, "count %u: %u blocks of %u, last %u", count, rp.n_blk, B, rp.blk_last);
    const uint32_t N = rp.n_paths;
    auto pair = [&](uint32_t s, uint32_t k) {
        const uint32_t pid = pid_join(rp, s, k);
        QCHECK(pid < N, "pixels %u samples %u: (%u, %u) -> %u", act_pixels, count, s, k, pid);
        const PidParts pp = pid_split(rp, pid);
        QCHECK(pp.s == s && pp.k == k, "pixels %u samples %u: (%u, %u) -> %u -> (%u, %u)", act_pixels, count, s, k, pid, pp.s, pp.k);
        ++g.p5_ids;
        return pid;
    };
    auto id = [&](uint32_t pid) {
        const PidParts pp = pid_split(rp, pid);
        QCHECK(pp.s < count && pp.k < act_pixels && pid_join(rp, pp.s, pp.k) == pid, "pixels %u samples %u: %u -> (%u, %u)", act_pixels, count, pid, pp.s, pp.k);
        ++g.p5_ids;
    };
    if (N <= (1u << 21))
    {
        std::vector<uint8_t> seen(N, 0);
        for (uint32_t s = 0; s < count; ++s)
            for (uint32_t k = 0; k < act_pixels; ++k)
            {
                const uint32_t pid = pair(s, k);
                if (pid < N) { QCHECK(!seen[pid], "pixels %u samples %u: id %u twice", act_pixels, count, pid); seen[pid] = 1; }
            }
        for (uint32_t pid = 0; pid < N; ++pid) id(pid);
        return;
    }
    // too many ids for a table: the corners, the block boundaries and random ones, both ways
    for (const uint32_t s : {0u, 1u % count, B - 1u, B % count, (rp.n_blk - 1u) * B, count - 1u, rng.below(count), rng.below(count)})
        for (const uint32_t k : {0u, 1u, act_pixels / 2u, act_pixels - 2u, act_pixels - 1u}) pair(s, k);
    for (int i = 0; i < 20000; ++i) pair(rng.below(count), rng.below(act_pixels));
    const uint32_t per_blk = act_pixels << rp.blk_log;
    for (uint32_t b = 0; b < rp.n_blk; ++b)
        for (const uint64_t pid : {(uint64_t)b * per_blk - 1u, (uint64_t)b * per_blk, (uint64_t)b * per_blk + 1u, (uint64_t)b * per_blk + B}) if (pid < N) id((uint32_t)pid);
    id(N - 1u);
    for (int i = 0; i < 20000; ++i) id(rng.below(N));
}

static int queues_sweep(uint64_t seed)
{
    Rng rng{seed};
    const std::vector<uint32_t> counts = ray_counts(rng, 300);
    for (const uint32_t n : counts)
        for (const uint32_t grid : {1u, 2u, 7u, 256u, 1280u, 2048u, 2560u})
            for (const uint32_t wpb : {1u, 2u, 4u})
                for (const uint32_t div : {4u, 16u})
                    for (const uint32_t taper : {0u, 2u}) p1_case(rng, n, grid, wpb, div, taper);
    Stripes prev{6u, 0u};
    for (const uint32_t n : counts) p2_case(rng, n, prev);
    std::vector<uint32_t> producers = {0u, 1u, 2u, 3u, 4u, 7u, 64u, 255u, 256u, 1024u, 4096u, 5120u, 10240u, 16383u, 16384u};
    for (int i = 0; i < 16; ++i) producers.push_back(rng.below(16385));
    for (const uint32_t n : counts)
        for (const uint32_t p : producers)
            for (const uint32_t least : {64u, 256u}) p3_case(n, p, least);
    for (const uint32_t p : producers) for (const uint32_t least : {64u, 256u}) { p3_case(0u, p, least); p3_case(1u << 29, p, least); }
    for (uint32_t d = 1; d <= 4096u; ++d) p4_divisor(rng, d);
    for (uint32_t k = 1; k <= 32u; ++k)
        for (int e = -1; e <= 1; ++e)
        {
            const uint64_t d = (1ull << k) + e;
            if (d >= 1 && d <= 0xffffffffull) p4_divisor(rng, (uint32_t)d);
        }
    for (int i = 0; i < 4000; ++i) p4_divisor(rng, i & 1 ? rng.log_uniform(32) : (uint32_t)std::max<uint64_t>(1, rng.next() & 0xffffffffull));
    std::vector<uint32_t> samples;
    for (uint32_t c = 1; c <= 70u; ++c) samples.push_back(c);
    for (const uint32_t c : {255u, 256u, 257u}) samples.push_back(c);
    for (const uint32_t px : {1u, 2u, 63u, 64u, 65u, 2239u, 2240u, 2073600u})
        for (const uint32_t c : samples)
            if ((uint64_t)px * c < (1ull << 29)) p5_case(rng, px, c); // (plan_batches refuses a batch of 2^29 paths or more)
    std::printf("{\"p1_cases\": %llu, \"p1_static\": %llu, \"p1_chunks\": %llu, \"p2_cases\": %llu, \"p2_regions\": %llu, \"p2_slots\": %llu, \"p2_refused\": %llu, "
                "\"p3_cases\": %llu, \"p4_divisors\": %llu, \"p4_divisions\": %llu, \"p5_cases\": %llu, \"p5_ids\": %llu, \"failures\": %llu}\n",
                g.p1_cases, g.p1_static, g.p1_chunks, g.p2_cases, g.p2_regions, g.p2_slots, g.p2_refused, g.p3_cases, g.p4_divisors, g.p4_divisions, g.p5_cases, g.p5_ids,
                g.failures);
    return g.failures ? 1 : 0;
}
#undef QCHECK

} // namespace qsweep
