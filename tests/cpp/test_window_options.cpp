// The host rule of per-window solve options (limo_amd/csrc/kba_window_options.hpp) as a stand-alone host program: which fields of
// limo_ba_options may differ between the windows of a batch, the error text per field, "all equal gives no table", and a record's
// bytes against make_consts of its entry.  Built with -fsanitize=address together with kba_pack.cpp by
// tests/test_window_options_cpu.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../limo_amd/csrc/kba_window_options.hpp"

using namespace kba;

static int n_checks = 0, n_failed = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        ++n_checks;                                                          \
        if (!(cond)) {                                                       \
            ++n_failed;                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
        }                                                                    \
    } while (0)

static limo_ba_options defaults() {  // limo_ba_default_options restated (that function lives in the HIP library)
    limo_ba_options o;
    std::memset(&o, 0, sizeof(o));
    o.depth_thres = 0.16, o.reprojection_thres = 1.6, o.depth_quantile = 0.95, o.reprojection_quantile = 0.95;
    o.num_trim_rounds = 1, o.trim_solver_iterations = 2, o.min_landmarks_for_trimming = 100, o.minimum_number_residual_groups = 30;
    o.max_num_iterations = 100, o.max_solver_time_sec = -1.0;
    o.function_tolerance = 1e-6, o.gradient_tolerance = 1e-10, o.parameter_tolerance = 1e-8;
    o.initial_trust_region_radius = 1e4, o.max_trust_region_radius = 1e16, o.min_trust_region_radius = 1e-32;
    o.min_lm_diagonal = 1e-6, o.max_lm_diagonal = 1e32, o.min_relative_decrease = 1e-3;
    o.max_num_consecutive_invalid_steps = 5, o.jacobi_scaling = 1;
    return o;
}

struct Fixed {
    const char* name;
    void (*change)(limo_ba_options&);
};
// every field that must be equal, and a change of it
static const Fixed kFixed[] = {
    {"num_trim_rounds", [](limo_ba_options& o) { o.num_trim_rounds += 1; }},
    {"trim_solver_iterations", [](limo_ba_options& o) { o.trim_solver_iterations += 1; }},
    {"min_landmarks_for_trimming", [](limo_ba_options& o) { o.min_landmarks_for_trimming = 30; }},
    {"minimum_number_residual_groups", [](limo_ba_options& o) { o.minimum_number_residual_groups = 10; }},
    {"max_num_iterations", [](limo_ba_options& o) { o.max_num_iterations = 50; }},
    {"max_solver_time_sec", [](limo_ba_options& o) { o.max_solver_time_sec = 0.2; }},
    {"function_tolerance", [](limo_ba_options& o) { o.function_tolerance = 1e-7; }},
    {"gradient_tolerance", [](limo_ba_options& o) { o.gradient_tolerance = 1e-9; }},
    {"parameter_tolerance", [](limo_ba_options& o) { o.parameter_tolerance = 1e-9; }},
    {"initial_trust_region_radius", [](limo_ba_options& o) { o.initial_trust_region_radius = 1e3; }},
    {"max_trust_region_radius", [](limo_ba_options& o) { o.max_trust_region_radius = 1e15; }},
    {"min_trust_region_radius", [](limo_ba_options& o) { o.min_trust_region_radius = 1e-30; }},
    {"min_lm_diagonal", [](limo_ba_options& o) { o.min_lm_diagonal = 1e-5; }},
    {"max_lm_diagonal", [](limo_ba_options& o) { o.max_lm_diagonal = 1e30; }},
    {"min_relative_decrease", [](limo_ba_options& o) { o.min_relative_decrease = 1e-2; }},
    {"max_num_consecutive_invalid_steps", [](limo_ba_options& o) { o.max_num_consecutive_invalid_steps = 4; }},
    {"jacobi_scaling", [](limo_ba_options& o) { o.jacobi_scaling = 0; }},
};
struct Free {
    const char* name;
    double limo_ba_options::*field;
};
static const Free kFree[] = {{"depth_thres", &limo_ba_options::depth_thres},
                             {"reprojection_thres", &limo_ba_options::reprojection_thres},
                             {"depth_quantile", &limo_ba_options::depth_quantile},
                             {"reprojection_quantile", &limo_ba_options::reprojection_quantile}};

static bool bits_equal(double a, double b) {
    return std::memcmp(&a, &b, sizeof(double)) == 0;
}

int main() {
    const int n = 5;
    std::string err;
    bool uniform = false;
    // ---- all equal: fine, uniform, no table
    {
        std::vector<limo_ba_options> o(n, defaults());
        CHECK(check_window_options(n, n, o.data(), &uniform, err) == LIMO_OK && uniform);
        std::vector<WinOpts> table(3);
        window_options_table(n, o.data(), uniform, table);
        CHECK(table.empty());
        // (a single window is uniform by definition)
        CHECK(check_window_options(1, 1, o.data(), &uniform, err) == LIMO_OK && uniform);
    }
    // ---- each of the four free fields may differ, alone and together: fine, not uniform, a record per window
    for (const Free& f : kFree) {
        std::vector<limo_ba_options> o(n, defaults());
        o[3].*(f.field) *= 0.5;
        uniform = true;
        CHECK(check_window_options(n, n, o.data(), &uniform, err) == LIMO_OK && !uniform);
        CHECK(!window_options_equal(o[0], o[3]) && window_options_equal(o[0], o[2]) && window_options_fixed_diff(o[0], o[3]) == nullptr);
        std::vector<WinOpts> table;
        window_options_table(n, o.data(), uniform, table);
        CHECK((int)table.size() == n);
    }
    // ---- a record's bytes are make_consts of ITS entry, field for field (the IEEE division behind inv_a_*2 included)
    {
        std::vector<limo_ba_options> o(n, defaults());
        const double dt[] = {0.08, 0.16, 0.4, 0.3, 1e-3}, rt[] = {0.8, 1.6, 3.0, 2.4, 7.0}, qd[] = {0.8, 0.95, 1.0, 0.85, 0.5}, qr[] = {1.0, 0.8, 0.95, 0.9, 0.99};
        for (int w = 0; w < n; ++w) o[w].depth_thres = dt[w], o[w].reprojection_thres = rt[w], o[w].depth_quantile = qd[w], o[w].reprojection_quantile = qr[w];
        CHECK(check_window_options(n, n, o.data(), &uniform, err) == LIMO_OK && !uniform);
        std::vector<WinOpts> table;
        window_options_table(n, o.data(), uniform, table);
        CHECK((int)table.size() == n);
        for (int w = 0; w < n && w < (int)table.size(); ++w) {
            const SolveConsts c = make_consts(o[w]);
            const WinOpts& r = table[w];
            CHECK(bits_equal(r.a_rep, c.a_rep) && bits_equal(r.a_rep, rt[w]));
            CHECK(bits_equal(r.a_dep, c.a_dep) && bits_equal(r.a_dep, dt[w]));
            CHECK(bits_equal(r.inv_a_rep2, c.inv_a_rep2) && bits_equal(r.inv_a_rep2, 1.0 / (rt[w] * rt[w])));
            CHECK(bits_equal(r.inv_a_dep2, c.inv_a_dep2) && bits_equal(r.inv_a_dep2, 1.0 / (dt[w] * dt[w])));
            CHECK(bits_equal(r.depth_quantile, c.depth_quantile) && bits_equal(r.depth_quantile, qd[w]));
            CHECK(bits_equal(r.reprojection_quantile, c.reprojection_quantile) && bits_equal(r.reprojection_quantile, qr[w]));
            CHECK(r.pad[0] == 0.0 && r.pad[1] == 0.0);
        }
        CHECK(sizeof(WinOpts) == 64 && alignof(WinOpts) == 64);
    }
    // ---- every other field must be equal: refused, the first offending window and the field named
    for (const Fixed& f : kFixed) {
        std::vector<limo_ba_options> o(n, defaults());
        o[2].depth_thres = 0.3;  // (a permitted difference in front of the offending window changes nothing)
        f.change(o[3]);
        f.change(o[4]);
        err.clear();
        CHECK(check_window_options(n, n, o.data(), &uniform, err) == LIMO_ERR_INVALID);
        CHECK(err == std::string("window 3: ") + f.name);
        CHECK(std::string(window_options_fixed_diff(o[0], o[3]) ? window_options_fixed_diff(o[0], o[3]) : "") == f.name);
        // ... and the same change in EVERY entry is no difference
        std::vector<limo_ba_options> all(n, defaults());
        for (auto& e : all) f.change(e);
        CHECK(check_window_options(n, n, all.data(), &uniform, err) == LIMO_OK && uniform);
    }
    CHECK(sizeof(kFixed) / sizeof(kFixed[0]) + sizeof(kFree) / sizeof(kFree[0]) == 21);  // every member of limo_ba_options is in one of the two lists
    // ---- a threshold or quantile that is not a finite number: refused with its window, also in entry 0
    for (const Free& f : kFree)
        for (double bad : {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()})
            for (int at : {0, 4}) {
                std::vector<limo_ba_options> o(n, defaults());
                o[at].*(f.field) = bad;
                err.clear();
                CHECK(check_window_options(n, n, o.data(), &uniform, err) == LIMO_ERR_INVALID);
                CHECK(err == "window " + std::to_string(at) + ": " + f.name + " is not finite");
            }
    // ---- the array itself
    {
        std::vector<limo_ba_options> o(n, defaults());
        err.clear();
        CHECK(check_window_options(n, n - 1, o.data(), &uniform, err) == LIMO_ERR_INVALID && err.find("n_opts (4)") != std::string::npos);
        CHECK(check_window_options(n, n + 1, o.data(), &uniform, err) == LIMO_ERR_INVALID);
        CHECK(check_window_options(n, n, nullptr, &uniform, err) == LIMO_ERR_INVALID && err == "opts is NULL");
        // -0.0 and +0.0 are different bits: "bitwise equal" is what the rule says
        o[1].max_solver_time_sec = 0.0, o[0].max_solver_time_sec = 0.0;
        o[2].max_solver_time_sec = 0.0, o[3].max_solver_time_sec = 0.0, o[4].max_solver_time_sec = -0.0;
        CHECK(check_window_options(n, n, o.data(), &uniform, err) == LIMO_ERR_INVALID && err == "window 4: max_solver_time_sec");
    }
    std::printf("%d checks, %d failed checks\n", n_checks, n_failed);
    return n_failed ? 1 : 0;
}
