// TEST — the iteration log of the LM state machine (limo_amd/csrc/kba_lm.hpp:lm_log_push), driven by hand-made reductions.
// A stand-alone host program: lm_solve_init / lm_decide_lin / lm_decide_step / sched_advance / sched_after_trim are called the way the
// kernels call them, and the recorded limo_ba_iteration entries are held against what Ceres' TrustRegionMinimizer would have pushed
// (oracle/ceres_like.cpp:463-586).  Built twice by tests/iteration_log_common.py: plain, and with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../limo_amd/csrc/kba_lm.hpp"

using namespace kba;

namespace {

int g_fail = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond);          \
            ++g_fail;                                                           \
        }                                                                       \
    } while (0)

SolveConsts consts(int rounds = 0, int trim_iters = 2, int max_iters = 100) {
    SolveConsts c;
    std::memset(&c, 0, sizeof(c));
    c.function_tolerance = 1e-6;
    c.gradient_tolerance = 1e-10;
    c.parameter_tolerance = 1e-8;
    c.initial_radius = 1e4;
    c.max_radius = 1e16;
    c.min_radius = 1e-32;
    c.min_relative_decrease = 1e-3;
    c.max_invalid = 5;
    c.num_trim_rounds = rounds;
    c.trim_iters = trim_iters;
    c.max_iters = max_iters;
    return c;
}

struct Rig {
    WinState s;
    std::vector<limo_ba_iteration> log;
    explicit Rig(int cap = 64) : log((size_t)cap + 1) {
        std::memset(&s, 0, sizeof(s));
        s.term = -1;
        std::memset(log.data(), 0xEE, sizeof(limo_ba_iteration) * log.size());  // (the entry behind the capacity must stay as it is)
        s.log = log.data();
        s.log_cap = cap;
    }
    bool guard_intact() const {
        const unsigned char* p = reinterpret_cast<const unsigned char*>(&log.back());
        for (size_t i = 0; i < sizeof(limo_ba_iteration); ++i)
            if (p[i] != 0xEE) return false;
        return true;
    }
};

WinRed lin(double cost, double gmax, double xnorm2 = 4.0) {
    WinRed r;
    std::memset(&r, 0, sizeof(r));
    r.lin_cost = cost;
    r.gmax = gmax;
    r.xnorm2 = xnorm2;
    return r;
}
WinRed step(double mcc, double step2, double cand2, double cand_cost) {
    WinRed r;
    std::memset(&r, 0, sizeof(r));
    r.mcc = mcc;
    r.step2 = step2;
    r.cand2 = cand2;
    r.cand_cost = cand_cost;
    return r;
}
WinRed invalid_step() {
    WinRed r = step(1.0, 0.01, 4.0, 1.0);
    r.chol_fail = 1;
    return r;
}

bool entry_is(const limo_ba_iteration& e, int solve, int kind, int it, int valid, int succ, double cost, double change, double gmax, double stepn, double rho,
              double radius) {
    return e.solve == solve && e.solve_kind == kind && e.iteration == it && e.step_is_valid == valid && e.step_is_successful == succ && e.pad[0] == 0 &&
           e.pad[1] == 0 && e.cost == cost && e.cost_change == change && e.gradient_max_norm == gmax && e.step_norm == stepn && e.relative_decrease == rho &&
           e.trust_region_radius == radius;
}

const double kFixed = 0.5;
const double kR3 = 1e4 / std::fmax(1.0 / 3.0, 0.0);  // the radius after an accepted step with rho = 1 (kba_lm.hpp: q = 1)
const double kStep = std::sqrt(0.01);

// iteration 0, an accepted, a rejected and an invalid step of a final solve
void test_accept_reject_invalid() {
    const SolveConsts c = consts();
    Rig g;
    lm_solve_init(g.s, true, c.max_iters, c);
    CHECK(g.s.log_n == 0);
    lm_decide_lin(g.s, lin(10.0, 1.0), kFixed, c);
    CHECK(g.s.log_n == 1);
    CHECK(entry_is(g.log[0], 0, 2, 0, 1, 1, 10.5, 0.0, 1.0, 0.0, 0.0, 1e4));
    // accepted: rho = (10 - 8) / 2 = 1 -> radius x 3; the entry waits for the relinearisation
    lm_decide_step(g.s, step(2.0, 0.01, 4.1, 8.0), c);
    CHECK(g.s.accept == 1 && g.s.log_n == 1);
    lm_decide_lin(g.s, lin(-1.0, 0.5), kFixed, c);  // (the cost of a relinearisation is not read: cost_pending)
    CHECK(g.s.log_n == 2);
    CHECK(entry_is(g.log[1], 0, 2, 1, 1, 1, 8.5, 2.0, 0.5, kStep, 1.0, kR3));
    // rejected: rho = (8 - 9) / 2
    lm_decide_step(g.s, step(2.0, 0.04, 4.2, 9.0), c);
    CHECK(g.s.accept == 0 && g.s.log_n == 3);
    CHECK(entry_is(g.log[2], 0, 2, 2, 1, 0, 9.5, -1.0, 0.5, std::sqrt(0.04), -0.5, kR3 / 2.0));
    // invalid: the factor has doubled, radius / 4
    lm_decide_step(g.s, invalid_step(), c);
    CHECK(g.s.log_n == 4);
    CHECK(entry_is(g.log[3], 0, 2, 3, 0, 0, 8.5, 0.0, 0.5, 0.0, 0.0, kR3 / 2.0 / 4.0));
    // a model cost change that is not positive is an invalid step as well; radius / 8
    lm_decide_step(g.s, step(-1.0, 0.01, 4.0, 7.0), c);
    CHECK(g.s.log_n == 5);
    CHECK(entry_is(g.log[4], 0, 2, 4, 0, 0, 8.5, 0.0, 0.5, 0.0, 0.0, kR3 / 2.0 / 4.0 / 8.0));
    CHECK(g.s.active == 1);
    CHECK(g.guard_intact());
}

void test_five_invalid_steps() {
    const SolveConsts c = consts();
    Rig g;
    lm_solve_init(g.s, true, c.max_iters, c);
    lm_decide_lin(g.s, lin(10.0, 1.0), kFixed, c);
    double radius = 1e4, f = 2.0;
    for (int k = 1; k <= 4; ++k) {
        lm_decide_step(g.s, invalid_step(), c);
        radius /= f;
        f *= 2.0;
        CHECK(g.s.log_n == 1 + k);
        CHECK(entry_is(g.log[k], 0, 2, k, 0, 0, 10.5, 0.0, 1.0, 0.0, 0.0, radius));
    }
    lm_decide_step(g.s, invalid_step(), c);  // the fifth: FAILURE, no entry
    CHECK(g.s.term == LIMO_FAILURE && g.s.active == 0);
    CHECK(g.s.log_n == 5);
    CHECK(g.s.iter == 5);  // (limo_ba_report::iterations_total counts it)
}

void test_tolerances_have_no_entry() {
    const SolveConsts c = consts();
    {
        Rig g;
        lm_solve_init(g.s, true, c.max_iters, c);
        lm_decide_lin(g.s, lin(10.0, 1.0), kFixed, c);
        lm_decide_step(g.s, step(2.0, 1e-20, 4.0, 8.0), c);  // |step| = 1e-10 <= 1e-8 (2 + 1e-8)
        CHECK(g.s.term == LIMO_CONVERGENCE && g.s.active == 0 && g.s.iter == 1);
        CHECK(g.s.log_n == 1);
    }
    {
        Rig g;
        lm_solve_init(g.s, true, c.max_iters, c);
        lm_decide_lin(g.s, lin(10.0, 1.0), kFixed, c);
        lm_decide_step(g.s, step(2.0, 0.01, 4.0, 10.0 - 1e-6), c);  // |cost change| ~ 1e-6 <= 1e-6 x 10
        CHECK(g.s.term == LIMO_CONVERGENCE && g.s.active == 0 && g.s.iter == 1);
        CHECK(g.s.log_n == 1);
    }
}

void test_stops_with_an_entry() {
    {   // iteration cap behind an accepted step: the entry, then NO_CONVERGENCE
        const SolveConsts c = consts();
        Rig g;
        lm_solve_init(g.s, true, 1, c);
        lm_decide_lin(g.s, lin(10.0, 1.0), kFixed, c);
        lm_decide_step(g.s, step(2.0, 0.01, 4.1, 8.0), c);
        CHECK(g.s.active == 1);
        lm_decide_lin(g.s, lin(0.0, 0.5), kFixed, c);
        CHECK(g.s.term == LIMO_NO_CONVERGENCE && g.s.active == 0);
        CHECK(g.s.log_n == 2 && entry_is(g.log[1], 0, 2, 1, 1, 1, 8.5, 2.0, 0.5, kStep, 1.0, kR3));
    }
    {   // iteration cap behind a rejected step
        const SolveConsts c = consts();
        Rig g;
        lm_solve_init(g.s, true, 1, c);
        lm_decide_lin(g.s, lin(10.0, 1.0), kFixed, c);
        lm_decide_step(g.s, step(2.0, 0.01, 4.1, 11.0), c);
        CHECK(g.s.term == LIMO_NO_CONVERGENCE && g.s.active == 0);
        CHECK(g.s.log_n == 2 && entry_is(g.log[1], 0, 2, 1, 1, 0, 11.5, -1.0, 1.0, kStep, -0.5, 5e3));
    }
    {   // minimum radius behind a rejected step
        SolveConsts c = consts();
        c.min_radius = 6e3;
        Rig g;
        lm_solve_init(g.s, true, c.max_iters, c);
        lm_decide_lin(g.s, lin(10.0, 1.0), kFixed, c);
        CHECK(g.s.active == 1);
        lm_decide_step(g.s, step(2.0, 0.01, 4.1, 11.0), c);
        CHECK(g.s.term == LIMO_CONVERGENCE && g.s.active == 0);
        CHECK(g.s.log_n == 2 && g.log[1].trust_region_radius == 5e3 && g.log[1].step_is_successful == 0);
    }
    {   // gradient tolerance behind an accepted step, and at iteration 0
        const SolveConsts c = consts();
        Rig g;
        lm_solve_init(g.s, true, c.max_iters, c);
        lm_decide_lin(g.s, lin(10.0, 1.0), kFixed, c);
        lm_decide_step(g.s, step(2.0, 0.01, 4.1, 8.0), c);
        lm_decide_lin(g.s, lin(0.0, 1e-12), kFixed, c);
        CHECK(g.s.term == LIMO_CONVERGENCE && g.s.active == 0);
        CHECK(g.s.log_n == 2 && g.log[1].gradient_max_norm == 1e-12 && g.log[1].step_is_successful == 1);
        Rig h;
        lm_solve_init(h.s, true, c.max_iters, c);
        lm_decide_lin(h.s, lin(10.0, 1e-12), kFixed, c);
        CHECK(h.s.term == LIMO_CONVERGENCE && h.s.active == 0);
        CHECK(h.s.log_n == 1 && entry_is(h.log[0], 0, 2, 0, 1, 1, 10.5, 0.0, 1e-12, 0.0, 0.0, 1e4));
    }
}

void test_no_entries() {
    const SolveConsts c = consts();
    {   // the first evaluation fails
        Rig g;
        lm_solve_init(g.s, true, c.max_iters, c);
        WinRed r = lin(10.0, 1.0);
        r.lin_fail = 1;
        lm_decide_lin(g.s, r, kFixed, c);
        CHECK(g.s.term == LIMO_FAILURE && g.s.log_n == 0);
    }
    {   // no variable parameter block
        Rig g;
        lm_solve_init(g.s, true, c.max_iters, c);
        WinRed r = lin(0.0, 0.0);
        r.no_variable = 1;
        lm_decide_lin(g.s, r, kFixed, c);
        CHECK(g.s.term == LIMO_CONVERGENCE && g.s.log_n == 0 && g.s.solve_final_cost == kFixed);
    }
    {   // the relinearisation behind an accepted step fails: no entry for that step
        Rig g;
        lm_solve_init(g.s, true, c.max_iters, c);
        lm_decide_lin(g.s, lin(10.0, 1.0), kFixed, c);
        lm_decide_step(g.s, step(2.0, 0.01, 4.1, 8.0), c);
        WinRed r = lin(0.0, 0.5);
        r.lin_fail = 1;
        lm_decide_lin(g.s, r, kFixed, c);
        CHECK(g.s.term == LIMO_FAILURE && g.s.log_n == 1);
    }
    {   // switched off: nothing is written anywhere, the log fields stay as they were
        Rig g;
        g.s.log = nullptr;
        g.s.log_cap = 0;
        lm_solve_init(g.s, true, c.max_iters, c);
        lm_decide_lin(g.s, lin(10.0, 1.0), kFixed, c);
        lm_decide_step(g.s, step(2.0, 0.01, 4.1, 11.0), c);
        CHECK(g.s.log_n == 0 && g.s.log_solve == 0 && g.s.log_si == 0 && g.s.log_kind == 0);
        const unsigned char* p = reinterpret_cast<const unsigned char*>(g.log.data());
        CHECK(p[0] == 0xEE && p[63] == 0xEE);
    }
    {   // the capacity bounds the stores
        Rig g(2);
        lm_solve_init(g.s, true, c.max_iters, c);
        lm_decide_lin(g.s, lin(10.0, 1.0), kFixed, c);
        for (int k = 0; k < 3; ++k) lm_decide_step(g.s, step(2.0, 0.01, 4.1, 11.0), c);
        CHECK(g.s.log_n == 2 && g.guard_intact());
    }
}

// One solve of the schedule that ends at its first step by the function tolerance: final cost == initial cost, "did not reduce".
// reduce = true: an accepted step first.
void run_short_solve(WinState& s, const SolveConsts& c, bool reduce) {
    lm_decide_lin(s, lin(10.0, 1.0), kFixed, c);
    if (reduce) {
        lm_decide_step(s, step(2.0, 0.01, 4.1, 8.0), c);
        lm_decide_lin(s, lin(0.0, 0.5), kFixed, c);
        lm_decide_step(s, step(2.0, 0.01, 4.1, 8.0), c);  // function tolerance
    } else {
        lm_decide_step(s, step(2.0, 0.01, 4.1, 10.0), c);  // function tolerance at once
    }
    CHECK(s.active == 0 && s.term == LIMO_CONVERGENCE);
}

// a trimming solve that does not reduce the cost: kinds 0, 1, 2 with solve indices 0, 1, 2 - on the streaming phase machine ...
void test_retry_kinds_streaming() {
    const SolveConsts c = consts(1);
    WinDesc wd;
    std::memset(&wd, 0, sizeof(wd));
    wd.do_trim = 1;
    Rig g;
    g.s.phase = PH_IDLE;
    CHECK(sched_advance(g.s, wd, c) == 1 && g.s.phase == PH_TRIM_SOLVE);
    run_short_solve(g.s, c, false);
    CHECK(sched_advance(g.s, wd, c) == 1 && g.s.phase == PH_RETRY);
    CHECK(g.s.max_iter == 3 * c.trim_iters);
    run_short_solve(g.s, c, true);
    CHECK(sched_advance(g.s, wd, c) == 1 && g.s.phase == PH_TRIM);
    sched_after_trim(g.s, c);
    CHECK(g.s.phase == PH_FINAL);
    run_short_solve(g.s, c, true);
    CHECK(sched_advance(g.s, wd, c) == 2);
    CHECK(g.s.log_n == 1 + 2 + 2);
    const int want[5][3] = {{0, 0, 0}, {1, 1, 0}, {1, 1, 1}, {2, 2, 0}, {2, 2, 1}};
    for (int i = 0; i < 5; ++i) CHECK(g.log[i].solve == want[i][0] && g.log[i].solve_kind == want[i][1] && g.log[i].iteration == want[i][2]);
    CHECK(g.s.acc_solves == 3 && g.s.log_si == 0);
    // a window that does not trim: one solve, kind 2
    Rig h;
    wd.do_trim = 0;
    h.s.phase = PH_IDLE;
    CHECK(sched_advance(h.s, wd, c) == 1 && h.s.phase == PH_FINAL);
    run_short_solve(h.s, c, true);
    CHECK(h.s.log_n == 2 && h.log[0].solve == 0 && h.log[0].solve_kind == 2 && h.log[1].solve_kind == 2);
}

// ... and on the list of solves the lock-step schedule and the one-launch kernels walk (sched_solve / sched_selected): three windows -
// one whose trimming solve does not reduce the cost, one whose does, one that does not trim
void test_retry_kinds_lockstep() {
    const SolveConsts c = consts(1);
    WinDesc wd[3];
    std::memset(wd, 0, sizeof(wd));
    wd[0].do_trim = wd[1].do_trim = 1;
    Rig g[3];
    for (int si = 0; si < 2 * c.num_trim_rounds + 1; ++si) {
        const SchedSolve sv = sched_solve(si, c);
        for (int w = 0; w < 3; ++w) {
            lm_solve_init(g[w].s, sched_selected(sv.select, wd[w], g[w].s), sv.max_iter, c);
            if (g[w].s.active) run_short_solve(g[w].s, c, !(w == 0 && si == 0));
        }
    }
    CHECK(g[0].s.log_n == 5 && g[1].s.log_n == 4 && g[2].s.log_n == 2);
    const int want0[5][2] = {{0, 0}, {1, 1}, {1, 1}, {2, 2}, {2, 2}};
    for (int i = 0; i < 5; ++i) CHECK(g[0].log[i].solve == want0[i][0] && g[0].log[i].solve_kind == want0[i][1]);
    const int want1[4][2] = {{0, 0}, {0, 0}, {1, 2}, {1, 2}};
    for (int i = 0; i < 4; ++i) CHECK(g[1].log[i].solve == want1[i][0] && g[1].log[i].solve_kind == want1[i][1]);
    for (int i = 0; i < 2; ++i) CHECK(g[2].log[i].solve == 0 && g[2].log[i].solve_kind == 2);
    for (int w = 0; w < 3; ++w) CHECK(g[w].s.log_si == 3 && g[w].s.log_solve == g[w].s.acc_solves);
    // the same bytes as the streaming machine gives window 0
    Rig h;
    h.s.phase = PH_IDLE;
    sched_advance(h.s, wd[0], c);
    run_short_solve(h.s, c, false);
    sched_advance(h.s, wd[0], c);
    run_short_solve(h.s, c, true);
    sched_advance(h.s, wd[0], c);
    sched_after_trim(h.s, c);
    run_short_solve(h.s, c, true);
    CHECK(h.s.log_n == 5 && std::memcmp(h.log.data(), g[0].log.data(), 5 * sizeof(limo_ba_iteration)) == 0);
}

}  // namespace

int main() {
    static_assert(sizeof(limo_ba_iteration) == 64, "limo_ba_iteration is 64 bytes");
    test_accept_reject_invalid();
    test_five_invalid_steps();
    test_tolerances_have_no_entry();
    test_stops_with_an_entry();
    test_no_entries();
    test_retry_kinds_streaming();
    test_retry_kinds_lockstep();
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("iteration log: all checks passed\n");
    return 0;
}
