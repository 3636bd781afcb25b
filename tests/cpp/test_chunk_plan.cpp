// Host-side pin of the decisions a chunk of hypotheses is issued by (misc3d_amd/csrc/m3d_chunk_plan.hpp: plan_chunk, the text
// issue_chunk compiles): no GPU, no library.  (a) named scenarios with the whole expected plan written out, each read off the
// conditions issue_chunk carried in its body before the plan existed; (b) every combination of the boolean inputs, at three
// window lengths and two tile counts, held to the implications the stages rely on.
#include <cstdint>
#include <cstdio>
#include <limits>

#include "../../misc3d_amd/csrc/m3d_chunk_plan.hpp"

using namespace m3d;

static int bad = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (++bad <= 40) printf("FAILED line %d: %s\n", __LINE__, #cond); \
        }                                                                    \
    } while (0)

#define PLAN_FIELDS(X)                                                                                                             \
    X(m) X(count) X(sl_pad) X(h_pad) X(n_groups) X(g0) X(g1) X(ga) X(g_lo) X(dense_tiles) X(tombstones_ride) X(dense) X(cull32)     \
    X(prune_scratch) X(lead_prepared) X(all_prepared) X(own_real) X(prune) X(fuse_lead) X(lead_elsewhere) X(phased) X(bound_on)     \
    X(bound_forced) X(ref_on) X(ref_min_count) X(touched_wanted) X(ubsum_at) X(timing) X(solo) X(records_to_host)                   \
    X(records_on_device) X(counts_reserved) X(polls)

static void expect_plan(const char* name, const ChunkPlan& got, const ChunkPlan& want) {
    int diffs = 0;
#define X(field)                                                                                            \
    if ((long long)got.field != (long long)want.field) {                                                    \
        printf("%s: %s is %lld, expected %lld\n", name, #field, (long long)got.field, (long long)want.field); \
        ++diffs;                                                                                            \
    }
    PLAN_FIELDS(X)
#undef X
    if (got.head != want.head) {
        printf("%s: head runs on the %s stream\n", name, got.head == HeadStream::kPre ? "pre" : "main");
        ++diffs;
    }
    printf("%-64s %s\n", name, diffs ? "FAILED" : "ok");
    bad += diffs;
}

static const int kSomething = 0;
static const PickFinal* const kPick = reinterpret_cast<const PickFinal*>(&kSomething);   // (never dereferenced by the plan)
static m3d_comm* const kComm = reinterpret_cast<m3d_comm*>(const_cast<int*>(&kSomething));

// C2's cloud: 1 000 000 points = 1954 tiles of 512 in the sorted copy, padded to 489 dense scoring tiles of 2048; frames built
static ChunkFacts c2_cloud(int kind = M3D_PLANE) {
    ChunkFacts f;
    f.kind = kind;
    f.n_pad = 1001472;
    f.n_tiles = 1954;
    f.radius = 7.5;
    f.has_frames = true;
    f.score_phases = kind == M3D_CYLINDER ? 3 : 0;   // m3d_config.score_phases = -1
    return f;
}
// C2's fit as run_ransac asks for it: probability 1, 10 000 hypotheses in one chunk, lead 128, polled completion
static ChunkRequest c2_request() {
    ChunkRequest r;
    r.end = 10000;
    r.prune = true;
    r.lead = 128;
    r.new_fit = true;
    r.device_records = true;
    r.pick_final = kPick;
    r.nothing_to_prune = true;   // (the only chunk; with a lead pass it changes nothing)
    return r;
}
static ChunkPlan c2_plan() {
    ChunkPlan p;
    p.m = 3; p.count = 10000; p.sl_pad = 10048; p.h_pad = 10048; p.n_groups = 157; p.g0 = 0; p.g1 = 157; p.ga = 2; p.g_lo = 2;
    p.dense_tiles = 489;
    p.cull32 = true; p.prune_scratch = true; p.lead_prepared = true; p.own_real = true; p.prune = true; p.fuse_lead = true;
    p.bound_on = true; p.ref_on = true; p.ref_min_count = 8 * 1954; p.ubsum_at = 10048;
    p.records_to_host = true; p.records_on_device = true; p.counts_reserved = true; p.polls = true;
    return p;
}
// a later chunk of a long probability-1 fit: 23 976 hypotheses behind a first chunk of 2048
static ChunkRequest later_request() {
    ChunkRequest r;
    r.begin = 2048;
    r.end = 2048 + 23976;
    r.prune = true;
    r.device_records = true;
    r.pick_final = kPick;
    r.pre_wanted = true;
    return r;
}
static ChunkPlan later_plan(int m) {
    ChunkPlan p;
    p.m = m; p.count = 23976; p.sl_pad = 24000; p.h_pad = 24000; p.n_groups = 375; p.g1 = 375; p.dense_tiles = 489;
    p.cull32 = true; p.prune_scratch = true; p.own_real = true; p.prune = true;
    p.records_to_host = true; p.records_on_device = true; p.counts_reserved = true; p.polls = true;
    return p;
}

static void scenarios() {
    {   // `prune` off: no ub, no incumbent, nothing but box tests, keep-all masks and scoring; records straight to the host
        ChunkFacts f = c2_cloud();
        ChunkRequest r;
        r.end = 5000;
        ChunkPlan p;
        p.m = 3; p.count = 5000; p.sl_pad = 5056; p.h_pad = 5056; p.n_groups = 79; p.g1 = 79; p.dense_tiles = 489;
        p.cull32 = true; p.own_real = true; p.records_to_host = true;
        expect_plan("score_range: plain records", plan_chunk(f, r), p);
    }
    {   // use_lead, lead_prepared (new fit), cull_lead_k, bound_pays(1954, 10 000), ref_on with min_count 8 per tile
        expect_plan("C2 plane fit, ref_bound 1", plan_chunk(c2_cloud(), c2_request()), c2_plan());
    }
    {   // `config().ref_bound != 0`
        ChunkFacts f = c2_cloud();
        f.ref_bound = 0;
        ChunkPlan p = c2_plan();
        p.ref_on = false; p.ref_min_count = 0;
        expect_plan("C2 plane fit, ref_bound 0", plan_chunk(f, c2_request()), p);
    }
    {   // bound_mode: ref_bound 2 forces the bound's launch, and any lead count builds the histograms
        ChunkFacts f = c2_cloud();
        f.ref_bound = 2;
        ChunkPlan p = c2_plan();
        p.bound_forced = true; p.ref_min_count = 1;
        expect_plan("C2 plane fit, ref_bound 2", plan_chunk(f, c2_request()), p);
    }
    {   // `sv.frames` in bound_on
        ChunkFacts f = c2_cloud();
        f.has_frames = false;
        ChunkPlan p = c2_plan();
        p.bound_on = false; p.ubsum_at = 0; p.ref_on = false; p.ref_min_count = 0;
        expect_plan("C2 plane fit without frames", plan_chunk(f, c2_request()), p);
    }
    {   // `sv.radius < 1e18`: fp64 box tests, hence no cull_lead_k; the plane bound does not need them
        ChunkFacts f = c2_cloud();
        f.radius = std::numeric_limits<double>::infinity();
        ChunkPlan p = c2_plan();
        p.cull32 = false; p.fuse_lead = false;
        expect_plan("C2 plane fit, radius unknown", plan_chunk(f, c2_request()), p);
    }
    {   // `!sv.has_dead` in ref_on (and in the phased scoring, which planes do not use)
        ChunkFacts f = c2_cloud();
        f.has_dead = true;
        ChunkPlan p = c2_plan();
        p.ref_on = false; p.ref_min_count = 0;
        expect_plan("C2 plane fit on a cloud with tombstones", plan_chunk(f, c2_request()), p);
    }
    {   // `pre`: a later chunk, pruned, no lead, one GPU, stream and event exist; an incumbent exists (!new_fit): bound on, no ref
        ChunkFacts f = c2_cloud();
        f.has_pre_stream = f.has_pre_done = true;
        ChunkPlan p = later_plan(3);
        p.head = HeadStream::kPre; p.bound_on = true; p.ubsum_at = 24000;
        expect_plan("later chunk, pre wanted, pre-stream exists", plan_chunk(f, later_request()), p);
    }
    {   // `ctx->pre_stream && s.pre_done`
        ChunkPlan p = later_plan(3);
        p.bound_on = true; p.ubsum_at = 24000;
        expect_plan("later chunk, pre wanted, no pre-stream", plan_chunk(c2_cloud(), later_request()), p);
    }
    {   // cylinders: phased scoring AND the bound (sums behind the phase counters), `g1 - g0 >= 128u` for the touched words
        ChunkPlan p = later_plan(2);
        p.phased = true; p.bound_on = true; p.ubsum_at = 48000; p.touched_wanted = true;
        expect_plan("cylinder window of 375 groups", plan_chunk(c2_cloud(M3D_CYLINDER), later_request()), p);
    }
    {   // ... 64 groups: bound_pays says no (4096 < 8192), so the bound is forced; too few groups for cull_hyp32_k's words
        ChunkFacts f = c2_cloud(M3D_CYLINDER);
        f.plane_bound = 2;
        ChunkRequest r = later_request();
        r.end = r.begin + 4096;
        ChunkPlan p = later_plan(2);
        p.count = 4096; p.sl_pad = 4096; p.h_pad = 4096; p.n_groups = 64; p.g1 = 64;
        p.phased = true; p.bound_on = true; p.bound_forced = true; p.ubsum_at = 8192;
        expect_plan("cylinder window of 64 groups, bound forced", plan_chunk(f, r), p);
    }
    {   // `kind != M3D_SPHERE` unless forced
        expect_plan("sphere window, plane_bound 1", plan_chunk(c2_cloud(M3D_SPHERE), later_request()), later_plan(4));
        ChunkFacts f = c2_cloud(M3D_SPHERE);
        f.plane_bound = 2;
        ChunkPlan p = later_plan(4);
        p.bound_on = true; p.bound_forced = true; p.ubsum_at = 24000;
        expect_plan("sphere window, plane_bound 2", plan_chunk(f, later_request()), p);
    }
    {   // all_prepared: the only chunk of a new fit, no lead: minimal_fit_k keeps everything; no incumbent, so no bound
        ChunkRequest r;
        r.end = 2000;
        r.prune = r.new_fit = r.nothing_to_prune = true;
        r.pick_final = kPick;
        ChunkPlan p;
        p.m = 3; p.count = 2000; p.sl_pad = 2048; p.h_pad = 2048; p.n_groups = 32; p.g1 = 32; p.dense_tiles = 489;
        p.cull32 = true; p.prune_scratch = true; p.all_prepared = true; p.own_real = true; p.prune = true;
        p.records_to_host = true; p.polls = true;
        expect_plan("nothing_to_prune with lead 0", plan_chunk(c2_cloud(), r), p);
        // the adaptive fit's hinted first chunk with no_prune_hint, the loop longer than the chunk: keep_mask_k runs as ever
        r.nothing_to_prune = false;
        p.all_prepared = false;
        expect_plan("adaptive first chunk, no_prune_hint, more to come", plan_chunk(c2_cloud(), r), p);
    }
    {   // dense: nothing of the culled path, counts reserved for the copies, no polling even if asked
        ChunkFacts f = c2_cloud();
        f.dense = true;
        ChunkRequest r = c2_request();
        r.device_records = false;
        r.pick_final = nullptr;
        ChunkPlan p;
        p.m = 3; p.count = 10000; p.sl_pad = 10048; p.h_pad = 10048; p.n_groups = 157; p.g1 = 157; p.dense_tiles = 489;
        p.dense = true; p.own_real = true; p.prune = true; p.counts_reserved = true;
        expect_plan("dense scoring", plan_chunk(f, r), p);
    }
    for (uint32_t rank = 0; rank < 2; ++rank) {   // slices of 5056 >= lead + 64: a lead pass; rank 1 tests the lead's boxes apart
        ChunkFacts f = c2_cloud();
        f.has_comm = true; f.world = 2; f.rank = rank;
        ChunkRequest r = c2_request();
        r.comm = kComm;
        r.pick_final = nullptr;
        r.caller_ships_records = true;
        ChunkPlan p;
        p.m = 3; p.count = 10000; p.sl_pad = 5056; p.h_pad = 10112; p.n_groups = 158; p.g0 = rank * 79; p.g1 = p.g0 + 79; p.ga = 2;
        p.g_lo = rank ? 79 : 2; p.dense_tiles = 489;
        p.cull32 = true; p.prune_scratch = true; p.lead_prepared = true; p.own_real = true; p.prune = true;
        p.fuse_lead = rank == 0; p.lead_elsewhere = rank == 1;
        p.records_on_device = true; p.counts_reserved = true;   // bound_pays(1954, 5056): no
        expect_plan(rank ? "world 2, rank 1, slices above lead + 64" : "world 2, rank 0, slices above lead + 64", plan_chunk(f, r), p);
        // `!comm || sl_pad >= lead + 64`: slices of 128 leave no room behind the lead
        r.end = 256;
        p = ChunkPlan();
        p.m = 3; p.count = 256; p.sl_pad = 128; p.h_pad = 256; p.n_groups = 4; p.g0 = rank * 2; p.g1 = p.g0 + 2; p.g_lo = p.g0;
        p.dense_tiles = 489;
        p.cull32 = true; p.prune_scratch = true; p.own_real = true; p.prune = true;
        p.records_on_device = true; p.counts_reserved = true;
        expect_plan(rank ? "world 2, rank 1, slices below lead + 64" : "world 2, rank 0, slices below lead + 64", plan_chunk(f, r), p);
    }
    {   // own_real: 60 hypotheses in slices of 64, rank 1 starts at 64
        ChunkFacts f = c2_cloud();
        f.has_comm = true; f.world = 2; f.rank = 1;
        ChunkRequest r;
        r.begin = 10000; r.end = 10060;
        r.prune = true;
        r.comm = kComm;
        ChunkPlan p;
        p.m = 3; p.count = 60; p.sl_pad = 64; p.h_pad = 128; p.n_groups = 2; p.g0 = 1; p.g1 = 2; p.g_lo = 1; p.dense_tiles = 489;
        p.cull32 = true; p.prune_scratch = true; p.prune = true; p.records_on_device = true; p.counts_reserved = true;
        expect_plan("short last window, rank 1 without hypotheses", plan_chunk(f, r), p);
    }
    for (int rccl = 1; rccl >= 0; --rccl) {   // `solo`: one rank over RCCL ships like one GPU; a host transport's gather is always called
        ChunkFacts f = c2_cloud();
        f.has_comm = true; f.rccl = rccl != 0;
        ChunkRequest r = c2_request();
        r.comm = kComm;
        r.pick_final = nullptr;
        r.caller_ships_records = true;
        ChunkPlan p = c2_plan();
        p.ref_on = false; p.ref_min_count = 0; p.polls = false;   // (`!comm` in ref_on)
        p.solo = rccl != 0; p.records_to_host = rccl != 0;
        expect_plan(rccl ? "world 1 over RCCL" : "world 1 over a host transport", plan_chunk(f, r), p);
    }
    {   // a pending tombstone pass rides in a plane's minimal_fit_k launch -- on the main stream
        ChunkFacts f = c2_cloud();
        f.has_pre_stream = f.has_pre_done = true;
        f.tombstones_pending = true;
        ChunkPlan p = later_plan(3);
        p.tombstones_ride = true; p.bound_on = true; p.ubsum_at = 24000;
        expect_plan("tombstone pass pending", plan_chunk(f, later_request()), p);
    }
}

static void sweep() {
    const size_t windows[3] = {64, 2048, 24576};
    const uint32_t tiles[2] = {40, 1954};
    const struct { uint32_t world, rank; } ranks[3] = {{1, 0}, {2, 0}, {2, 1}};
    unsigned long long n = 0, mix = 0;
    for (uint32_t bits = 0; bits < (1u << 17); ++bits)
        for (size_t w : windows)
            for (uint32_t t : tiles)
                for (int kind = 0; kind < 3; ++kind)
                    for (uint32_t lead = 0; lead <= 128; lead += 128)
                        for (const auto& wr : ranks) {
                            ChunkFacts f;
                            ChunkRequest r;
                            r.begin = 4096;
                            r.end = r.begin + w;
                            r.lead = lead;
                            r.prune = bits & 1u;
                            r.new_fit = bits & 2u;
                            r.device_records = bits & 4u;
                            r.caller_ships_records = bits & 8u;
                            r.pick_final = (bits & 16u) ? kPick : nullptr;
                            r.nothing_to_prune = bits & 32u;
                            r.pre_wanted = bits & 64u;
                            r.first_of_stream = bits & 128u;
                            f.has_dead = bits & 256u;
                            f.has_frames = bits & 512u;
                            f.has_pre_stream = bits & 1024u;
                            f.has_pre_done = bits & 2048u;
                            f.tombstones_pending = bits & 4096u;
                            f.has_comm = bits & 8192u;
                            f.rccl = bits & 16384u;
                            f.dense = bits & 32768u;
                            f.kernel_timing = (bits & 65536u) ? 1 : 0;
                            r.comm = f.has_comm ? kComm : nullptr;
                            f.kind = kind;
                            f.n_tiles = t;
                            f.n_pad = t * 512;
                            f.world = wr.world;
                            f.rank = wr.rank;
                            // the inputs that are no booleans take every value in turn, out of step with the loops above
                            ++mix;
                            f.plane_bound = (int)(mix % 3);
                            f.ref_bound = (int)(mix / 3 % 3);
                            f.cull_fp32 = (int)(mix / 9 % 2);
                            f.radius = (mix / 18 % 2) ? 7.5 : std::numeric_limits<double>::infinity();
                            f.score_phases = (int)(mix / 36 % 5 == 0 ? 0 : (mix / 36 % 5 == 1 ? 2 : 3));
                            const ChunkPlan p = plan_chunk(f, r);
                            ++n;
                            const uint32_t world = f.has_comm ? f.world : 1u;
                            CHECK(!p.ref_on || p.bound_on);
                            CHECK(!p.bound_on || (r.prune && f.has_frames && !f.dense));
                            CHECK(!p.touched_wanted || (p.bound_on && kind == M3D_CYLINDER && p.g1 - p.g0 >= 128u));
                            CHECK(!(p.lead_prepared && p.all_prepared));
                            CHECK(!(p.lead_prepared || p.all_prepared) || r.new_fit);
                            CHECK(p.head != HeadStream::kPre ||
                                  (!f.dense && !f.has_comm && r.lead == 0 && !r.new_fit && !f.tombstones_pending));
                            CHECK(p.g0 <= p.g1 && p.g1 <= p.n_groups);
                            CHECK(p.h_pad % 64 == 0 && p.h_pad == p.sl_pad * world && p.sl_pad % 64 == 0 && p.h_pad >= p.count);
                            CHECK(p.n_groups * 64 == p.h_pad);
                            CHECK(p.ga <= p.n_groups);
                            CHECK(!p.solo || world == 1);
                        }
    printf("sweep: %llu plans\n", n);
}

int main() {
    scenarios();
    sweep();
    if (bad) {
        printf("%d FAILED\n", bad);
        return 1;
    }
    printf("all ok\n");
    return 0;
}
