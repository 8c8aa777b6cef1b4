// TEST-ONLY host build of the bending report's per-hinge header (stark_amd/csrc/bending_report.hpp compiled with g++): lets the CPU test suite check the
// exact device arithmetic against the numpy reference of tests/bending_ref.py without a GPU. Not part of the product library.
#include "../../stark_amd/csrc/bending_report.hpp"

using namespace mistark;

// in: [n][nin] gathered inputs in binding order, threshold: [n] per row or null (none), group: [n] or null (0), rec: [n][16]; kind 0 complete, 1 flat
extern "C" int host_bending_eval(int kind, const double* in, int nin, int n, const double* threshold, const int* group, double* rec)
{
    if (nin != 31) return -2;
    for (int e = 0; e < n; e++) {
        const double* ie = in + (size_t)e * nin;
        double* re = rec + (size_t)e * BEND_REC;
        const double thr = threshold ? threshold[e] : -1.0;
        if (kind == 0) shells_bending_record(ie, thr, re);
        else if (kind == 1) flat_bending_record(ie, thr, re);
        else return -1;
        re[14] = group ? (double)group[e] : 0.0;
    }
    return 0;
}
