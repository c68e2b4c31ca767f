// Example: a few interior-point iterations that never leave the GPU, through the C ABI only
// (include/ipx_kkt_hip.h; no reference code, no Python).  Builds a small random LP
//     min c'x  s.t.  A x + s = b,  x >= 0,  s >= 0
// in solver form (AI = [A I]), puts an interior iterate on the device and repeats what IPM::Driver
// does per iteration (reference src/ipm.cc:74-150): KKTSolver::Factorize for the current iterate, then
// predictor + corrector + step sizes + update (ipxk_ipm_step).  Prints the residual norms and mu.
// Then -- as LpSolver does when it switches from the initial to the main IPM (src/lp_solver.cc:375-462) -- the
// basis-preconditioned phase: ipxk_ipm_driver_basis runs IPM::Driver around the basis solver (Maxvolume, LU
// factorization and Prepare on the device every iteration) from the slack basis until the termination test holds.
// With a fifth argument p > 0, p percent of the rows are equality rows (slack lb = ub = 0): the run then starts from
// ipxk_ipm_starting_point, and between the two phases ipxk_ipm_starting_basis (StartingBasis, src/starting_basis.cc) pivots
// the fixed slacks out of the slack basis, which is where the main phase goes on.
// With 2 as the fourth argument the program makes ONE call instead, ipxk_ipm_solve (LpSolver::InteriorPointSolve: starting
// point, initial iterations, starting basis, main phase, postprocessing), and prints the evaluation of the postprocessed
// iterate -- the reference's interior solution -- and the dropping residuals crossover starts from (crossover_start = 1e-8);
// then ipxk_crossover_run turns it into a vertex in solver form and the pushes, pivots, status and infeasibilities are printed.
// A sixth argument t > 0 sets both drop tolerances (ipxk_ipm_set_drop_tolerances; the reference's default is 1e-9): the main
// phase then takes nearly degenerate variables out of the barrier problem before every Maxvolume, and the counts are printed.
//
//   g++ -std=c++14 -O2 -Iinclude examples/ipm_loop.cc -Lipx_amd/lib -lipx_kkt_hip -Wl,-rpath,$PWD/ipx_amd/lib -o ipm_loop
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "ipx_kkt_hip.h"

#define CHECK(call)                                                                   \
    do {                                                                              \
        const int rc_ = (call);                                                       \
        if (rc_ != IPXK_OK) { std::fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, ipxk_last_error()); return 1; } \
    } while (0)

int main(int argc, char** argv) {
    const ipxint m = argc > 1 ? std::atol(argv[1]) : 2000, n = argc > 2 ? std::atol(argv[2]) : 5000;
    const int iterations = argc > 3 ? std::atoi(argv[3]) : 6;
    const int eq_percent = argc > 5 ? std::atoi(argv[5]) : 0;
    const double drop_tol = argc > 6 ? std::atof(argv[6]) : 0.0;
    std::mt19937_64 rng(7);
    std::uniform_real_distribution<double> mag(0.5, 4.0), unit(0.0, 1.0);
    // A: 8 entries per column, sorted rows
    std::vector<ipxint> Ap(n + 1, 0), Ai;
    std::vector<double> Ax;
    for (ipxint j = 0; j < n; j++) {
        std::vector<ipxint> rows;
        while ((ipxint)rows.size() < std::min<ipxint>(8, m)) {
            const ipxint r = (ipxint)(rng() % (uint64_t)m);
            bool dup = false;
            for (ipxint q : rows) dup |= q == r;
            if (!dup) rows.push_back(r);
        }
        std::sort(rows.begin(), rows.end());
        for (ipxint r : rows) { Ai.push_back(r); Ax.push_back((rng() & 1 ? 1.0 : -1.0) * mag(rng)); }
        Ap[j + 1] = (ipxint)Ai.size();
    }
    const ipxint N = n + m;
    // a feasible, bounded LP: b = A x0 + s0 with x0, s0 > 0;  c = A'y0 + z0 with z0 > 0
    std::vector<double> x0(N), y0(m), z0(N), b(m, 0.0), c(N, 0.0), lb(N, 0.0), ub(N, INFINITY);
    for (auto& v : x0) v = 0.5 + unit(rng);
    for (auto& v : z0) v = 0.5 + unit(rng);
    for (auto& v : y0) v = unit(rng) - 0.5;
    for (ipxint j = 0; j < n; j++)
        for (ipxint p = Ap[j]; p < Ap[j + 1]; p++) { b[Ai[p]] += Ax[p] * x0[j]; c[j] += Ax[p] * y0[Ai[p]]; }
    for (ipxint i = 0; i < m; i++) { b[i] += x0[n + i]; c[n + i] = y0[i]; }
    for (ipxint j = 0; j < N; j++) c[j] += z0[j];
    for (ipxint i = 0; i < m; i++)
        if ((int)(rng() % 100) < eq_percent) { b[i] -= x0[n + i]; ub[n + i] = 0.0; c[n + i] = 0.0; }     // row i is '='

    ipxk_context* ctx = nullptr;
    CHECK(ipxk_create(m, n, Ap.data(), Ai.data(), Ax.data(), 0, &ctx));
    CHECK(ipxk_ipm_set_drop_tolerances(ctx, drop_tol, drop_tol));
    auto print_drops = [&]() {
        ipxint primal = 0, dual = 0, updates = 0;
        if (ipxk_ipm_drop_counts(ctx, &primal, &dual, &updates) == IPXK_OK)
            std::printf("drops (tolerance %.1e): %ld primal, %ld dual, %ld exchanges\n", drop_tol, (long)primal, (long)dual, (long)updates);
    };
    if (argc > 4 && std::atoi(argv[4]) == 2) {           // the whole interior point solve in one call
        ipxk_solve_params prm{};
        prm.kkt_tol = 0.3; prm.feasibility_tol = 1e-6; prm.optimality_tol = 1e-8; prm.crossover_start = 1e-8;
        prm.dependency_tol = 1e-6; prm.ipm_maxiter = 300; prm.switchiter = -1; prm.max_etas = 100; prm.precond_dense_cols = 1;
        ipxk_solve_info info;
        std::vector<ipxint> basis(m), status(N);
        CHECK(ipxk_ipm_solve(ctx, b.data(), c.data(), lb.data(), ub.data(), &prm, &info, basis.data(), status.data(), nullptr, nullptr));
        std::printf("solve: status %ld after %ld iterations (%ld initial, ended by status %ld), %ld CR iterations, %ld exchanges for the "
                    "starting basis, %ld basis updates, %ld dependent rows, %ld dependent columns\n", (long)info.status_ipm, (long)info.iter,
                    (long)info.iter_initial, (long)info.status_initial, (long)info.kktiter, (long)info.updates_start, (long)info.basis_updates,
                    (long)info.dependent_rows, (long)info.dependent_cols);
        std::printf("interior solution: pobjective %.10e dobjective %.10e rel_objgap %.2e rel_presidual %.2e rel_dresidual %.2e; "
                    "dropping residuals %.2e %.2e\n", info.pobjective, info.dobjective, info.rel_objgap, info.rel_presidual,
                    info.rel_dresidual, info.pres_dropping, info.dres_dropping);
        print_drops();
        if (info.status_ipm != 1) { ipxk_destroy(ctx); return 1; }
        // crossover in solver form from the postprocessed iterate and the last basis: push phases, then the basic solution
        ipxk_crossover_info cross;
        std::vector<double> xv(N), yv(m), zv(N);
        std::vector<ipxint> basic_statuses(N);
        CHECK(ipxk_crossover_run(ctx, b.data(), c.data(), lb.data(), ub.data(), nullptr, basis.data(), nullptr, &cross, xv.data(), yv.data(),
                                 zv.data(), basic_statuses.data(), nullptr, 0, nullptr, nullptr));
        double objective = 0.0;
        for (ipxint j = 0; j < N; j++) objective += c[j] * xv[j];
        std::printf("crossover: status %ld, %ld dual pushes (%ld pivots, %.3f s), %ld primal pushes (%ld pivots, %.3f s); vertex objective "
                    "%.10e, primal infeasibility %.2e, dual infeasibility %.2e\n", (long)cross.status_crossover, (long)cross.dual_pushes,
                    (long)cross.dual_pivots, cross.seconds_dual, (long)cross.primal_pushes, (long)cross.primal_pivots, cross.seconds_primal,
                    objective, cross.primal_infeas, cross.dual_infeas);
        ipxk_destroy(ctx);
        return cross.status_crossover == 1 ? 0 : 1;
    }
    // interior start away from the solution: x = xl = 1, y = 0, zl = 1 (all variables have a lower bound only)
    std::vector<double> x(N, 1.0), xl(N, 1.0), xu(N, INFINITY), y(m, 0.0), zl(N, 1.0), zu(N, 0.0);
    std::vector<unsigned char> state(N, IPXK_STATE_BARRIER_LB);
    if (eq_percent > 0) {
        ipxk_ipm_params prm{0.3, 1e-6, 1e-8, -1, 100, 1};
        ipxk_ipm_info info;
        CHECK(ipxk_ipm_starting_point(ctx, b.data(), c.data(), lb.data(), ub.data(), &prm, &info, nullptr, nullptr));
        if (info.errflag) { std::fprintf(stderr, "starting point errflag %ld\n", (long)info.errflag); return 1; }
    } else {
        CHECK(ipxk_iterate_set(ctx, x.data(), xl.data(), xu.data(), y.data(), zl.data(), zu.data(), state.data()));
    }
    std::printf("%4s %10s %10s %10s %8s %8s %6s %6s\n", "iter", "presidual", "dresidual", "mu", "step_p", "step_d", "kkt1", "kkt2");
    for (int it = 0; it < iterations; it++) {
        ipxint errflag = 0;
        CHECK(ipxk_iterate_factorize_diag(ctx, 1, &errflag));
        if (errflag) { std::fprintf(stderr, "factorize errflag %ld\n", (long)errflag); break; }
        ipxk_ipm_step_info info;
        CHECK(ipxk_ipm_step(ctx, 0, b.data(), c.data(), lb.data(), ub.data(), 0.3, 2000, &info, nullptr, nullptr));
        std::printf("%4d %10.3e %10.3e %10.3e %8.4f %8.4f %6ld %6ld\n", it, info.presidual, info.dresidual, info.mu_before,
                    info.step_primal, info.step_dual, (long)info.kktiter_predictor, (long)info.kktiter_corrector);
        if (info.errflag) { std::fprintf(stderr, "KKT solve errflag %ld\n", (long)info.errflag); break; }
    }
    double comp[4];
    CHECK(ipxk_iterate_complementarity(ctx, comp));
    std::printf("final mu %.3e\n", comp[1]);
    if (argc > 4 && std::atoi(argv[4]) != 0) {           // main IPM with the basis solver
        ipxk_ipm_params prm{0.3, 1e-6, 1e-8, -1, 100, 1};
        ipxk_ipm_info info;
        if (eq_percent > 0) {
            ipxk_starting_basis_info sb;
            CHECK(ipxk_ipm_starting_basis(ctx, b.data(), c.data(), lb.data(), ub.data(), nullptr, &sb, nullptr, nullptr, nullptr, 0, nullptr, nullptr));
            std::printf("starting basis: errflag %ld, %ld exchanges, %ld dependent rows, %ld dependent columns, %.3f s\n", (long)sb.errflag,
                        (long)sb.updates_start, (long)sb.dependent_rows, (long)sb.dependent_cols, sb.seconds);
            if (sb.errflag) return 1;
        }
        CHECK(ipxk_ipm_driver_basis(ctx, b.data(), c.data(), lb.data(), ub.data(), &prm, &info, nullptr, nullptr, nullptr, nullptr));
        std::printf("main IPM: status %ld after %ld iterations, %ld CR iterations, %ld basis updates; pobjective %.10e dobjective %.10e "
                    "presidual %.2e dresidual %.2e\n", (long)info.status_ipm, (long)info.iter, (long)info.kktiter, (long)info.basis_updates,
                    info.pobjective, info.dobjective, info.presidual, info.dresidual);
        print_drops();
    }
    ipxk_destroy(ctx);
    return 0;
}
