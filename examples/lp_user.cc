// Example: an LP stated the way a user states it, solved on the GPU through the C ABI only (include/ipx_kkt_hip.h,
// section "user model"; no reference code, no Python):
//     min  x0 + 2 x1 - x2
//     s.t. x0 + x1 + x2       =  4
//          x0           + x3 <=  3
//               x1      + x3 >=  1
//          x0 >= 0,  x1 <= 5,  0 <= x2 <= 3,  x3 free
// -- all three row types and the four kinds of bounds.  ipxk_lp_create validates the model and presolves it on the device
// (slack bounds from the row types, dualization when that pays, equilibration) into a context the lp owns, ipxk_lp_solve
// runs the interior-point solve on it, ipxk_lp_postsolve returns the interior solution in the user's own variables and
// ipxk_lp_evaluate its residuals and objectives.  ipxk_lp_crossover then pushes the interior solution to a vertex:
// ipxk_lp_get_basic_solution returns it with the statuses of the user's own variables and rows (vbasis: 0 basic, -1 at the
// lower, -2 at the upper bound, -3 superbasic; cbasis: 0 basic, -1 nonbasic).  The optimum is x = (1.5, -0.5, 3, 1.5) with
// objective -2.5.
// With 1 as the first argument the dual form is forced (ipxk_lp_params::dualize); the answer is the same.
//
//   g++ -std=c++14 -O2 -Iinclude examples/lp_user.cc -Lipx_amd/lib -lipx_kkt_hip -Wl,-rpath,$PWD/ipx_amd/lib -o lp_user
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "ipx_kkt_hip.h"

#define CHECK(call)                                                                   \
    do {                                                                              \
        const int rc_ = (call);                                                       \
        if (rc_ != IPXK_OK) { std::fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, ipxk_last_error()); return 1; } \
    } while (0)

int main(int argc, char** argv) {
    const ipxint num_constr = 3, num_var = 4;
    // A by columns
    const ipxint Ap[] = {0, 2, 4, 5, 7};
    const ipxint Ai[] = {0, 1, 0, 2, 0, 1, 2};
    const double Ax[] = {1, 1, 1, 1, 1, 1, 1};
    const double rhs[] = {4, 3, 1};
    const char constr_type[] = {'=', '<', '>'};
    const double obj[] = {1, 2, -1, 0};
    const double lb[] = {0, -INFINITY, 0, -INFINITY};
    const double ub[] = {INFINITY, 5, 3, INFINITY};

    ipxk_lp_params params = {argc > 1 ? std::atol(argv[1]) : -1, 1, 0};
    ipxk_lp_info info;
    ipxk_lp* lp = nullptr;
    CHECK(ipxk_lp_create(num_constr, num_var, Ap, Ai, Ax, rhs, constr_type, obj, lb, ub, &params, &info, &lp));
    std::printf("solver form: %ld rows, %ld columns, %ld entries, %s; %ld boxed, %ld free variables, %ld equality rows\n",
                (long)info.m, (long)info.n, (long)info.nnz, info.dualized ? "dualized" : "primal", (long)info.num_boxed,
                (long)info.num_free_var, (long)info.num_eqconstr);

    ipxk_solve_params sp = {0.3, 1e-6, 1e-8, 1e-8, 1e-6, 300, -1, 100, 1, 0};      // crossover_start 1e-8: crossover follows
    ipxk_solve_info si;
    CHECK(ipxk_lp_solve(lp, &sp, &si, nullptr, nullptr));
    std::printf("status_ipm %ld after %ld iterations\n", (long)si.status_ipm, (long)si.iter);

    double x[4], xl[4], xu[4], slack[3], y[3], zl[4], zu[4];
    CHECK(ipxk_lp_postsolve(lp, x, xl, xu, slack, y, zl, zu));
    for (int j = 0; j < 4; j++) std::printf("x%d = %10.6f   zl = %9.2e  zu = %9.2e\n", j, x[j], zl[j], zu[j]);
    for (int i = 0; i < 3; i++) std::printf("row %d (%c): slack = %10.6f  y = %10.6f\n", i, constr_type[i], slack[i], y[i]);

    ipxk_lp_eval ev;
    CHECK(ipxk_lp_evaluate(lp, &ev));
    std::printf("objective %.8f (dual %.8f), residuals %.2e primal, %.2e dual\n", ev.pobjval, ev.dobjval, ev.abs_presidual,
                ev.abs_dresidual);

    ipxk_crossover_info ci;
    ipxk_lp_basic_eval be;
    CHECK(ipxk_lp_crossover(lp, nullptr, &ci, &be, nullptr, nullptr));
    std::printf("status_crossover %ld after %ld dual and %ld primal pushes\n", (long)ci.status_crossover, (long)ci.dual_pushes,
                (long)ci.primal_pushes);
    double z[4];
    ipxint cbasis[3], vbasis[4];
    CHECK(ipxk_lp_get_basic_solution(lp, x, slack, y, z, cbasis, vbasis));
    for (int j = 0; j < 4; j++) std::printf("vertex x%d = %16.12f   z = %9.2e  vbasis %ld\n", j, x[j], z[j], (long)vbasis[j]);
    for (int i = 0; i < 3; i++)
        std::printf("vertex row %d (%c): slack = %16.12f  y = %16.12f  cbasis %ld\n", i, constr_type[i], slack[i], y[i], (long)cbasis[i]);
    std::printf("vertex objval %.12f, infeasibilities %.2e primal, %.2e dual\n", be.objval, be.primal_infeas, be.dual_infeas);
    ipxk_lp_destroy(lp);
    return si.status_ipm == 1 && std::fabs(ev.pobjval + 2.5) < 1e-5 && ci.status_crossover == 1 && std::fabs(be.objval + 2.5) < 1e-9 ? 0 : 1;
}
