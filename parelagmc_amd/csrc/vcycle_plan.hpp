// Which kernels Multigrid::cycle runs on a level: the one place that decides it.  Pure functions of a few setup facts, the
// level's position in the cycle and the launch width - no device types, so tests/c/vcycle_plan_check.cpp compiles this header
// alone and checks it against a restatement of the predicates it replaced.
#pragma once

namespace pmc {

// what the decision reads from one MgLevel (MgLevel::facts) and from the tail descriptors around it
struct LevelFacts {
    int n = 0;
    bool is_last = false, bv = false, f32 = false, has_sp = false, p_oct = false, p_agg = false;
    bool has_scaled = false;      // column-scaled values (MgLevel::vals_scaled)
    bool has_scaled32 = false;    // their fp32 copy (MgLevel::scaled32)
    bool has_dense_inv = false;   // MgLevel::dense_inv
    bool has_ainv = false;        // MgLevel::ainv
    int split_log2 = 0;
    bool tail_here = false;       // an LDS tail descriptor starts on this level (Multigrid::tail[l])
    bool tail_next = false;       // ... on the next one
};

// what it reads from the Multigrid (Multigrid::cycle_facts)
struct CycleFacts {
    int smooth_degree = 2;
    bool f32_intermediates = true, f32_any_injection = false;
    int tail_later_nb = 0, dense_nb = 0;
    int nlevels = 0;
    bool coarse_f32 = true;       // PMC_COARSE_F32 (laboratory builds; always true in the product library)
};

// one enumerator per body of Multigrid::cycle
enum class LevelPath {
    Dense,            // ends the cycle with the dense inverse of an inner level (narrow launches)
    Tail,             // the LDS tail kernel runs this level and everything below it
    F32Shared,        // shared values, injection prolongator: iterate and residuals in fp32
    F32SharedSplit,   // the same with the row-split operators (inner level of a narrow launch)
    F32Bv,            // per-realization fp32 values with the octree restriction
    GenericBottom,    // ends the cycle with a Chebyshev polynomial (fp64)
    Generic           // smooths, descends, smooths (fp64)
};

struct LevelStep {
    LevelPath path = LevelPath::Generic;
    bool ends = false;         // the cycle ends on this level (Dense, Tail, GenericBottom)
    bool f32_capable = false;  // the level's kernels can take the right-hand side and return the correction in fp32
    bool io32 = false;         // ... and in this cycle they do
};

// the last supplied level and every level marked is_last end the recursion
inline bool level_is_bottom(const LevelFacts& f, const CycleFacts& c, int l) { return l == c.nlevels - 1 || f.is_last; }

inline bool f32_shared_path(LevelPath p) { return p == LevelPath::F32Shared || p == LevelPath::F32SharedSplit; }

// The step of level l in a cycle from level l0 at width nb.  `parent`: the step of level l - 1 (null for l == l0 and for
// questions about the level alone, which leave io32 false).
inline LevelStep level_step(const LevelFacts& f, const CycleFacts& c, int l, int l0, int nb, const LevelStep* parent) {
    const bool last = level_is_bottom(f, c, l);
    const bool narrow = nb <= c.dense_nb;
    const bool degree2 = c.smooth_degree == 2 && c.f32_intermediates;
    // a narrow launch leaves a tail that would start on a level of several thousand rows to the next level (LAB_NOTES 9.16)
    const bool tail_later = nb <= c.tail_later_nb && f.n > 4096 && !last && f.tail_next;
    LevelStep s;
    if (l > l0 && narrow && f.has_dense_inv)
        s.path = LevelPath::Dense;
    else if (f.tail_here && !tail_later)
        s.path = LevelPath::Tail;
    else if (!last && !f.bv && f.has_sp && (f.p_oct || c.f32_any_injection) && degree2 && f.has_scaled)
        s.path = (l > l0 && narrow && f.split_log2 > 0 && !f.p_oct && !f.p_agg) ? LevelPath::F32SharedSplit
                                                                                 : LevelPath::F32Shared;
    else if (!last && f.bv && f.f32 && f.p_oct && degree2 && f.has_scaled32)
        s.path = LevelPath::F32Bv;
    else
        s.path = last ? LevelPath::GenericBottom : LevelPath::Generic;
    s.ends = s.path == LevelPath::Dense || s.path == LevelPath::Tail || s.path == LevelPath::GenericBottom;
    // The vectors between two levels live only inside one application of the preconditioner.  A shared-value inner level on
    // the dense, tail or fp32 shared path can read its right-hand side and write its correction in fp32 (Multigrid::inner_f32)
    s.f32_capable = c.f32_intermediates && c.coarse_f32 && l > l0 && l < c.nlevels && !f.bv &&
                    (s.path == LevelPath::Dense || s.path == LevelPath::Tail || f32_shared_path(s.path));
    // ... and does so exactly when the level above it is on the fp32 shared path: only those kernels write an fp32 coarse
    // right-hand side and gather an fp32 correction
    s.io32 = parent && f32_shared_path(parent->path) && s.f32_capable;
    return s;
}

// What a cycle from level l0 at width nb does with level l (the setup export pmc_sampler_vcycle_level): role 0 = smooths and
// descends, 1 = ends the cycle with a polynomial, 2 = ends it with an exact solve (ainv at the bottom of the LDS tail, the
// dense inverse of a narrow launch), 3 = not reached; in_tail: the level runs inside the LDS tail kernel.
// lev[0 .. c.nlevels): the facts of every level.
struct LevelRole {
    int role = 3;
    bool in_tail = false;
};
inline LevelRole cycle_role(const LevelFacts* lev, const CycleFacts& c, int l0, int nb, int l) {
    bool in_tail = false;
    LevelStep step, *parent = nullptr;
    for (int q = l0; q < c.nlevels; ++q) {
        const LevelFacts& f = lev[q];
        if (!in_tail) {   // inside the tail kernel nothing is decided any more: it runs down to the first bottom level
            step = level_step(f, c, q, l0, nb, parent);
            parent = &step;
            in_tail = step.path == LevelPath::Tail;
        }
        const bool last = level_is_bottom(f, c, q);
        const int role = (!in_tail && step.path == LevelPath::Dense) ? 2 : !last ? 0 : (in_tail && f.has_ainv) ? 2 : 1;
        if (q == l) return LevelRole{role, in_tail};
        if (role != 0) break;
    }
    return LevelRole{};
}

}  // namespace pmc
