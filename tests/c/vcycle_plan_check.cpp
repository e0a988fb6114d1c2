// Stand-alone check of parelagmc_amd/csrc/vcycle_plan.hpp (make test-vcycle-plan; tests/test_vcycle_plan.py runs it): no
// library, no device.  namespace before holds the predicates Multigrid carried before the plan existed - level_path,
// inner_f32, cycle_role, top_reads_r32, the row-split condition and the fp32 hand-over of cycle() - written out over the same
// facts, line by line as they stood.  The plan must agree with them
//   1. on every combination of one level's facts, its position and the cycle settings,
//   2. on seeded random hierarchies of 1 to 10 levels, for every start level, level and width,
//   3. on the ten handle / storage regimes of tests/test_gpu_sampler_precond.py, which must also take the documented paths;
// and the cases must reach every LevelPath and every role.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vcycle_plan.hpp"

using namespace pmc;

// a hierarchy as the predicates saw it: per-level facts, the tail descriptors (tail[l]: one starts on level l) and the settings
// (fixed arrays: the exhaustive part builds some ten million of them)
constexpr int kMaxLevels = 10;
struct Hier {
    struct Levels {
        LevelFacts v[kMaxLevels];   // tail_here / tail_next are NOT read from here: see facts_of
        int count = 0;
        int size() const { return count; }
        const LevelFacts& operator[](size_t l) const { return v[l]; }
        LevelFacts& operator[](size_t l) { return v[l]; }
    } L;
    struct Tails {                  // Multigrid::tail after build_tails: one entry per level
        bool v[kMaxLevels] = {};
        int count = 0;
        int size() const { return count; }
        bool operator[](size_t l) const { return v[l]; }
        bool& operator[](size_t l) { return v[l]; }
    } tail;
    CycleFacts c;
    explicit Hier(int nl) { L.count = tail.count = c.nlevels = nl; }
};
// what Multigrid::level_facts hands the plan
static LevelFacts facts_of(const Hier& h, int l) {
    LevelFacts f = h.L[(size_t)l];
    f.tail_here = l < (int)h.tail.size() && h.tail[(size_t)l];
    f.tail_next = l + 1 < (int)h.tail.size() && h.tail[(size_t)l + 1];
    return f;
}

namespace before {
struct LevelPath {
    bool last = false, dense = false, tail_here = false, f32_shared = false, f32_bv = false;
};
static const bool use_tail = true;

static LevelPath level_path(const Hier& h, int l, int l0, int nb) {
    const LevelFacts& lv = h.L[(size_t)l];
    LevelPath p;
    p.last = (l == (int)h.L.size() - 1) || lv.is_last;
    p.dense = l > l0 && nb <= h.c.dense_nb && lv.has_dense_inv;
    if (p.dense) return p;
    const bool tail_later = nb <= h.c.tail_later_nb && lv.n > 4096 && !p.last && l + 1 < (int)h.tail.size() && h.tail[(size_t)l + 1];
    p.tail_here = use_tail && l < (int)h.tail.size() && h.tail[(size_t)l] && !tail_later;
    if (p.tail_here) return p;
    p.f32_shared = !p.last && !lv.bv && lv.has_sp && (lv.p_oct || h.c.f32_any_injection) && h.c.smooth_degree == 2 &&
                   lv.has_scaled && h.c.f32_intermediates;
    p.f32_bv = !p.last && lv.bv && lv.f32 && lv.p_oct && h.c.smooth_degree == 2 && lv.has_scaled32 && h.c.f32_intermediates;
    return p;
}

static bool inner_f32(const Hier& h, int l, int l0, int nb) {
    if (!h.c.f32_intermediates || !h.c.coarse_f32 || l <= l0 || l >= (int)h.L.size() || h.L[(size_t)l].bv) return false;
    const LevelPath p = level_path(h, l, l0, nb);
    return p.dense || p.tail_here || p.f32_shared;
}

static bool top_reads_r32(const Hier& h, int l0, int nb) {
    if (l0 < 0 || l0 + 1 >= (int)h.L.size()) return false;
    const LevelFacts& lv = h.L[(size_t)l0];
    const bool tail_later = nb <= h.c.tail_later_nb && lv.n > 4096 && l0 + 1 < (int)h.tail.size() && h.tail[(size_t)l0 + 1];
    const bool tail_here = use_tail && l0 < (int)h.tail.size() && h.tail[(size_t)l0] && !tail_later;
    return !tail_here && !lv.is_last && !lv.bv && lv.has_sp && !lv.p_oct && h.c.f32_any_injection && h.c.smooth_degree == 2 &&
           lv.has_scaled && h.c.f32_intermediates;
}

static int cycle_role(const Hier& h, int l0, int nb, int l, bool* in_tail) {
    bool tail_on = false;
    for (int q = l0; q < (int)h.L.size(); ++q) {
        const LevelFacts& lv = h.L[(size_t)q];
        const bool last = q == (int)h.L.size() - 1 || lv.is_last;
        int role = -1;
        if (!tail_on) {
            if (q > l0 && nb <= h.c.dense_nb && lv.has_dense_inv) {
                role = 2;
            } else {
                const bool tail_later = nb <= h.c.tail_later_nb && lv.n > 4096 && !last && q + 1 < (int)h.tail.size() && h.tail[(size_t)q + 1];
                tail_on = use_tail && q < (int)h.tail.size() && h.tail[(size_t)q] && !tail_later;
            }
        }
        if (role < 0) role = !last ? 0 : (tail_on && lv.has_ainv) ? 2 : 1;
        if (q == l) {
            if (in_tail) *in_tail = tail_on;
            return role;
        }
        if (role != 0) break;
    }
    if (in_tail) *in_tail = false;
    return 3;
}

// cycle() as a walk: the body level l runs (one of the new enumerators, by the order of cycle()'s branches), whether the cycle
// ends there and whether its right-hand side arrives in fp32 (the storage of the rc its parent constructed).  reached = false:
// the cycle ended above l.  Below the top level target, ztarget and dot_partial are null, as in cycle()'s recursive calls.
struct Body {
    bool reached = false, ends = false, io32 = false;
    pmc::LevelPath path = pmc::LevelPath::Generic;
};
static Body cycle_body(const Hier& h, int l0, int nb, int l, bool top_dot_partial) {
    bool io32 = false;
    for (int q = l0; q < (int)h.L.size(); ++q) {
        const LevelFacts& lv = h.L[(size_t)q];
        const LevelPath path = level_path(h, q, l0, nb);
        const bool target = q == l0, dot_partial = q == l0 && top_dot_partial;   // (target or ztarget: one of them at the top)
        Body b;
        b.reached = true;
        b.io32 = io32;
        bool next32 = false;
        if (path.dense && !(target || dot_partial)) {
            b.path = pmc::LevelPath::Dense, b.ends = true;
        } else if (path.tail_here) {
            b.path = pmc::LevelPath::Tail, b.ends = true;
        } else if (path.f32_shared) {
            next32 = inner_f32(h, q + 1, l0, nb);   // const zvec rc(lc.r.p, inner_f32(l + 1, l0, nb));
            const bool split = q > l0 && nb <= h.c.dense_nb && lv.split_log2 > 0 && !lv.p_oct && !lv.p_agg && !dot_partial;
            b.path = split ? pmc::LevelPath::F32SharedSplit : pmc::LevelPath::F32Shared;
        } else if (path.f32_bv) {
            b.path = pmc::LevelPath::F32Bv;         // zvec(lc.r.p, false)
        } else if (path.last) {
            b.path = pmc::LevelPath::GenericBottom, b.ends = true;
        } else {
            b.path = pmc::LevelPath::Generic;       // zvec(lc.r.p, false)
        }
        if (q == l) return b;
        if (b.ends) break;
        io32 = next32;
    }
    return Body();
}
}  // namespace before

static long long n_checked = 0;
static bool seen_path[7], seen_role[4];

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "%s:%d: FAILED %s\n", __FILE__, __LINE__, #cond);   \
            return false;                                                            \
        }                                                                            \
    } while (0)

// the plan against the old predicates on one hierarchy, start level and width: every level
static bool check_cycle(const Hier& h, int l0, int nb) {
    const int nl = (int)h.L.size();
    LevelFacts lev[kMaxLevels];
    for (int l = 0; l < nl; ++l) lev[l] = facts_of(h, l);
    // top_reads_r32 as Multigrid states it now
    const bool top_r32 = level_step(lev[(size_t)l0], h.c, l0, l0, nb, nullptr).path == LevelPath::F32Shared && !lev[(size_t)l0].p_oct;
    CHECK(top_r32 == before::top_reads_r32(h, l0, nb));
    LevelStep parent_step;
    bool running = true;   // the walk of cycle(): each level's step from its parent's
    int ends = 0;
    bool role_ended = false;
    for (int l = l0; l < nl; ++l) {
        const LevelFacts& f = lev[(size_t)l];
        // questions about the level alone: level_path, inner_f32
        const LevelStep alone = level_step(f, h.c, l, l0, nb, nullptr);
        const before::LevelPath op = before::level_path(h, l, l0, nb);
        CHECK((alone.path == LevelPath::Dense) == op.dense);
        CHECK((alone.path == LevelPath::Tail) == op.tail_here);
        CHECK(f32_shared_path(alone.path) == op.f32_shared);
        CHECK((alone.path == LevelPath::F32Bv) == op.f32_bv);
        CHECK((alone.path == LevelPath::GenericBottom) == (op.last && !op.dense && !op.tail_here));
        CHECK(alone.ends == (op.dense || op.tail_here || op.last));
        CHECK(!alone.io32);
        CHECK(alone.f32_capable == before::inner_f32(h, l, l0, nb));
        // roles
        bool old_tail = false;
        const int old_role = before::cycle_role(h, l0, nb, l, &old_tail);
        const LevelRole role = cycle_role(lev, h.c, l0, nb, l);
        CHECK(role.role == old_role && role.in_tail == old_tail);
        seen_role[role.role] = true;
        // the walk
        const before::Body body = before::cycle_body(h, l0, nb, l, false);
        const before::Body body_dot = before::cycle_body(h, l0, nb, l, true);   // a fused dot at the top changes no path
        CHECK(body.reached == running && body_dot.reached == running);
        if (running) {
            const LevelStep step = level_step(f, h.c, l, l0, nb, l > l0 ? &parent_step : nullptr);
            CHECK(step.path == body.path && step.ends == body.ends && step.io32 == body.io32);
            CHECK(step.path == body_dot.path && step.ends == body_dot.ends && step.io32 == body_dot.io32);
            CHECK(step.path == alone.path && step.f32_capable == alone.f32_capable);
            CHECK(!step.io32 || step.f32_capable);
            seen_path[(int)step.path] = true;
            // the host's walk ends where a role ends the cycle, or where the LDS tail kernel takes over the levels below
            CHECK(step.ends ? (old_role == 1 || old_role == 2 || (old_role == 0 && step.path == LevelPath::Tail)) : old_role == 0);
            CHECK(old_tail == (step.path == LevelPath::Tail));
            if (step.ends) ++ends, running = false;
            parent_step = step;
        } else {
            CHECK(old_role == 3 || old_tail);   // below the host's end only the tail kernel reaches a level
        }
        // structure (tests/test_gpu_sampler_precond.py): exactly one level ends the cycle, every level above it descends, every
        // level below it is not reached
        CHECK(role_ended ? old_role == 3 : old_role != 3);
        if (old_role == 1 || old_role == 2) role_ended = true;
        ++n_checked;
    }
    CHECK(ends == 1 && role_ended);
    return true;
}

static const int kWidths[] = {1, 8, 9, 64, 256, 257};

// 1. every combination of one level's facts x its position x the settings.  The level sits at index 0 (top) or 1 (inner, below
// a level that is or is not on the fp32 shared path) and is the last by index or has one more level below it.  Widths: both
// sides of the only thresholds there are (tail_later_nb, dense_nb: 0 or 8) - the run time goes with their number; the random
// part runs all of kWidths.
static bool exhaustive() {
    for (int bits = 0; bits < (1 << 12); ++bits)
        for (int n : {4096, 4097})
            for (int split : {0, 2})
                for (int pos = 0; pos < 3; ++pos)           // 0 top, 1 inner below a generic level, 2 inner below an injection level
                    for (int last_by_index = 0; last_by_index < 2; ++last_by_index)
                        for (int flags = 0; flags < 16; ++flags)
                            for (int tl_nb : {0, 8})
                                for (int d_nb : {0, 8}) {
                                    const int l = pos == 0 ? 0 : 1;
                                    Hier h(l + (last_by_index ? 1 : 2));
                                    for (int q = 0; q < h.L.size(); ++q) h.L[(size_t)q].n = 100;
                                    if (pos == 2) {
                                        h.L[0].has_sp = h.L[0].has_scaled = true;
                                        h.L[0].p_oct = (bits & 1) != 0;   // octree or aggregation, with the level's own bit 0
                                    }
                                    LevelFacts& f = h.L[(size_t)l];
                                    f.n = n;
                                    f.split_log2 = split;
                                    f.is_last = bits & 1, f.bv = bits & 2, f.f32 = bits & 4, f.has_sp = bits & 8;
                                    f.p_oct = bits & 16, f.p_agg = bits & 32, f.has_scaled = bits & 64, f.has_scaled32 = bits & 128;
                                    f.has_dense_inv = bits & 256, f.has_ainv = bits & 512;
                                    h.tail[(size_t)l] = bits & 1024;
                                    if (!last_by_index) h.tail[(size_t)l + 1] = bits & 2048;
                                    h.c.smooth_degree = (flags & 1) ? 2 : 3;
                                    h.c.f32_intermediates = flags & 2, h.c.f32_any_injection = flags & 4, h.c.coarse_f32 = flags & 8;
                                    h.c.tail_later_nb = tl_nb, h.c.dense_nb = d_nb;
                                    for (int nb : {8, 9})
                                        if (!check_cycle(h, 0, nb)) return false;
                                }
    return true;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {   // xorshift64*
    rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}
static bool coin(int percent) { return (int)(rnd() % 100) < percent; }

// 2. random hierarchies; half of them resemble the ones the handles build (one kind of values, injections, a tail and dense
// inverses towards the bottom), so that long descents through the fp32 paths occur, the other half are arbitrary
static bool random_hierarchies(int count) {
    static const int sizes[] = {60, 500, 4096, 4097, 40000};
    for (int it = 0; it < count; ++it) {
        const int nl = 1 + (int)(rnd() % kMaxLevels);
        Hier h(nl);
        const bool shaped = coin(50), bv = coin(30), oct = coin(50);
        for (int l = 0; l < nl; ++l) {
            LevelFacts& f = h.L[(size_t)l];
            f.n = sizes[rnd() % 5];
            f.split_log2 = coin(40) ? 1 + (int)(rnd() % 3) : 0;
            if (shaped) {
                f.bv = bv, f.f32 = bv && coin(80), f.has_sp = !bv && coin(90), f.p_oct = oct && coin(90);
                f.p_agg = !oct && coin(30), f.has_scaled = !bv || !f.f32, f.has_scaled32 = bv && f.f32;
                f.is_last = coin(5), f.has_dense_inv = l > nl / 2 && coin(30), f.has_ainv = coin(50);
                h.tail[(size_t)l] = l >= nl / 2 && coin(40);
            } else {
                f.is_last = coin(15), f.bv = coin(30), f.f32 = coin(50), f.has_sp = coin(60), f.p_oct = coin(50), f.p_agg = coin(30);
                f.has_scaled = coin(80), f.has_scaled32 = coin(50), f.has_dense_inv = coin(20), f.has_ainv = coin(30);
                h.tail[(size_t)l] = coin(25);
            }
        }
        h.c.smooth_degree = coin(85) ? 2 : 3;
        h.c.f32_intermediates = coin(75), h.c.f32_any_injection = coin(50), h.c.coarse_f32 = coin(85);
        h.c.tail_later_nb = coin(50) ? 8 : 0, h.c.dense_nb = coin(50) ? 8 : 0;
        for (int l0 = 0; l0 < nl; ++l0)
            for (int nb : kWidths)
                if (!check_cycle(h, l0, nb)) return false;
    }
    return true;
}

// 3. the handles of tests/test_gpu_sampler_precond.py (its docstring) in both storages: the facts their setup produces, and
// the path each level is documented to take in wide (64) and narrow (1, 8) launches
using P = LevelPath;
struct NamedRow {
    const char* name;
    Hier h{0};
    std::vector<P> wide, narrow;   // from level 0 to the level that ends the cycle
};
static LevelFacts shared_level(int n, bool oct, bool sp) {
    LevelFacts f;
    f.n = n, f.has_scaled = true, f.has_sp = sp, f.p_oct = oct;
    return f;
}
static NamedRow named_row(const char* name, bool fp32, std::vector<LevelFacts> L, int first_tail, bool hybrid, std::vector<P> wide,
                          std::vector<P> narrow) {
    NamedRow r;
    r.name = name;
    r.h = Hier((int)L.size());
    for (size_t l = 0; l < L.size(); ++l) r.h.L[l] = L[l];
    for (size_t l = (size_t)first_tail; l < L.size(); ++l) r.h.tail[l] = true;   // build_tails: every level from which the rest fits
    r.h.c.f32_intermediates = fp32;
    r.h.c.f32_any_injection = hybrid;
    r.h.c.tail_later_nb = hybrid ? 8 : 0;
    r.h.c.dense_nb = hybrid ? 8 : 0;
    r.wide = wide, r.narrow = narrow;
    return r;
}
static bool named_rows() {
    std::vector<NamedRow> rows;
    for (int fp32 = 0; fp32 < 2; ++fp32) {
        // hex32-saddle: Schur levels 32 768 / 4 096 / 512 / 64 with octree injections; level 0 leaves the tail: the fp32
        // kernels with the octree restriction fused, or the generic fp64 path
        {
            std::vector<LevelFacts> L = {shared_level(32768, true, true), shared_level(4096, true, true),
                                         shared_level(512, true, true), shared_level(64, false, false)};
            const P top = fp32 ? P::F32Shared : P::Generic;
            rows.push_back(named_row(fp32 ? "hex32-saddle fp32" : "hex32-saddle fp64", fp32, L, 1, false, {top, P::Tail}, {top, P::Tail}));
        }
        // tet-saddle: 384 / 48 / 6 elements, the cycle of hex32-saddle inside the LDS tail
        {
            std::vector<LevelFacts> L = {shared_level(384, true, true), shared_level(48, true, true), shared_level(6, false, false)};
            rows.push_back(named_row(fp32 ? "tet-saddle fp32" : "tet-saddle fp64", fp32, L, 0, false, {P::Tail}, {P::Tail}));
        }
        // hex32-sa: internal smoothed aggregation (P not an injection): the generic fp64 path in both storages outside the tail
        {
            std::vector<LevelFacts> L = {shared_level(32768, false, false), shared_level(2600, false, false),
                                         shared_level(260, false, false)};
            rows.push_back(named_row(fp32 ? "hex32-sa fp32" : "hex32-sa fp64", fp32, L, 1, false, {P::Generic, P::Tail},
                                     {P::Generic, P::Tail}));
        }
        // hex12-hybrid: 5 616 multipliers, aggregates of about 8: the whole cycle fits the tail for wide launches; narrow ones
        // start it one level later (level 0: fused aggregate restriction on kernels) and end on level 1 with the dense inverse
        {
            std::vector<LevelFacts> L = {shared_level(5616, false, true), shared_level(702, false, true), shared_level(88, false, false)};
            L[0].p_agg = true;
            L[1].has_dense_inv = true;
            L[2].has_ainv = true;
            const P top = fp32 ? P::F32Shared : P::Generic;
            rows.push_back(named_row(fp32 ? "hex12-hybrid fp32" : "hex12-hybrid fp64", fp32, L, 0, true, {P::Tail}, {top, P::Dense}));
        }
        // hex24-hybrid: 43 200 multipliers: level 0 outside the tail at every width (fused aggregate restriction), level 1
        // row-split for narrow launches, which end on level 2 with the dense inverse
        {
            std::vector<LevelFacts> L = {shared_level(43200, false, true), shared_level(5400, false, true),
                                         shared_level(675, false, true), shared_level(84, false, false)};
            L[0].p_agg = true;
            L[1].split_log2 = 2;
            L[2].has_dense_inv = true;
            L[3].has_ainv = true;
            const P top = fp32 ? P::F32Shared : P::Generic;
            rows.push_back(named_row(fp32 ? "hex24-hybrid fp32" : "hex24-hybrid fp64", fp32, L, 1, true, {top, P::Tail},
                                     {top, fp32 ? P::F32SharedSplit : P::Generic, P::Dense}));
        }
    }
    CHECK(rows.size() == 10);
    for (const NamedRow& r : rows) {
        for (int nb : {1, 8, 64}) {
            const std::vector<P>& want = nb <= 8 ? r.narrow : r.wide;
            if (!check_cycle(r.h, 0, nb)) return false;
            LevelStep parent;
            for (size_t l = 0; l < want.size(); ++l) {
                const LevelStep s = level_step(facts_of(r.h, (int)l), r.h.c, (int)l, 0, nb, l ? &parent : nullptr);
                if (s.path != want[l] || s.ends != (l + 1 == want.size())) {
                    std::fprintf(stderr, "%s width %d level %zu: path %d, documented %d\n", r.name, nb, l, (int)s.path, (int)want[l]);
                    return false;
                }
                // the fp32 hand-over exists exactly below the fp32 shared path of the multiplier hierarchies' fp32 storage
                CHECK(s.io32 == (l > 0 && f32_shared_path(want[l - 1])));
                parent = s;
            }
        }
    }
    return true;
}

int main() {
    if (!exhaustive()) return 1;
    const long long n1 = n_checked;
    if (!random_hierarchies(100000)) return 1;
    const long long n2 = n_checked - n1;
    if (!named_rows()) return 1;
    for (int p = 0; p < 7; ++p)
        if (!seen_path[p]) return std::fprintf(stderr, "LevelPath %d never reached\n", p), 1;
    for (int r = 0; r < 4; ++r)
        if (!seen_role[r]) return std::fprintf(stderr, "role %d never reached\n", r), 1;
    std::printf("vcycle_plan_check OK: %lld exhaustive, %lld random, %lld named level checks\n", n1, n2, n_checked - n1 - n2);
    return 0;
}
