// TEST-ONLY host build of the budget readout's arithmetic (stark_amd/csrc/budget.hpp compiled with g++): lets the CPU test suite check the exact device
// arithmetic against the numpy reference of tests/budget_ref.py without a GPU. Not part of the product library.
#include "../../stark_amd/csrc/budget.hpp"

using namespace mistark;

// in: [n][23] gathered inputs of EnergyLumpedInertia in binding order, group: [n], rec: [n_groups][13] (items added in list order)
extern "C" int host_budget_points(const double* in, const int* group, int n, int n_groups, const double* about, double* rec)
{
    for (int g = 0; g < n_groups; g++) {
        BudgetAcc acc;
        for (int i = 0; i < n; i++)
            if (group[i] == g) budget_add_inertia_item(acc, in + (size_t)i * 23, V3<double>(about[0], about[1], about[2]));
        budget_store(acc, rec + (size_t)g * BUDGET_REC);
    }
    return 0;
}
// one record per body
extern "C" int host_budget_bodies(const double* t0, const double* q0, const double* v1, const double* w1, const double* mass, const double* J_loc, int n, double dt,
                                  const double* about, const double* gravity, double* rec)
{
    for (int b = 0; b < n; b++) {
        BudgetAcc acc;
        budget_add_body(acc, t0 + 3 * b, q0 + 4 * b, v1 + 3 * b, w1 + 3 * b, mass[b], J_loc + 9 * b, dt, V3<double>(about[0], about[1], about[2]),
                        V3<double>(gravity[0], gravity[1], gravity[2]));
        budget_store(acc, rec + (size_t)b * BUDGET_REC);
    }
    return 0;
}
// R[9] row-major = R(q1), q1 advanced from q0 by w over dt: the function every rigid-body potential and the contact detector's vertices use
extern "C" int host_budget_R1(const double* q0, const double* w, double dt, double* R)
{
    const M3<double> M = rb_R1(q0, V3<double>(w[0], w[1], w[2]), dt);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[3 * i + j] = M.m[i][j];
    return 0;
}
