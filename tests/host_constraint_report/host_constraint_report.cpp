// TEST-ONLY host build of the constraint report's per-row arithmetic (stark_amd/csrc/constraint_report.hpp compiled with g++): lets the CPU test suite check
// the exact device arithmetic against the numpy restatement of tests/constraint_report_ref.py without a GPU. Not part of the product library.
#include <cstring>

#include "../../stark_amd/csrc/constraint_report.hpp"

using namespace mistark;

// info[6] of kind code `kind` (0..16): gathered inputs per row, group column, first block of side a, of side b, direction-type, unit; name: registry name
extern "C" int host_constraint_kind(int kind, int* info, char* name, int name_bytes)
{
#define X(En)                                                                     \
    if (ConstraintKind<En>::code == kind) {                                       \
        using K = ConstraintKind<En>;                                             \
        const int v[6] = {En::Layout::NIN, K::group_col, K::block_a, K::block_b, K::dir_type ? 1 : 0, K::unit}; \
        std::memcpy(info, v, sizeof(v));                                          \
        std::strncpy(name, En::name, (size_t)name_bytes - 1);                     \
        name[name_bytes - 1] = 0;                                                 \
        return 0;                                                                 \
    }
    MISTARK_FOR_EACH_CONSTRAINT(X)
#undef X
    return -1;
}

// in: [n][NIN of the kind] gathered inputs in binding order, tolerance: [n] per row (negative: none) or null; rec: [n][16], aux: [n][2]
extern "C" int host_constraint_rows(int kind, const double* in, int n, const double* tolerance, double* rec, double* aux)
{
#define X(En)                                                                                                                            \
    if (ConstraintKind<En>::code == kind) {                                                                                              \
        for (int i = 0; i < n; i++)                                                                                                      \
            constraint_record<En>(in + (size_t)i * En::Layout::NIN, tolerance ? tolerance[i] : -1.0, rec + (size_t)i * CONSTRAINT_REC, aux + (size_t)i * 2); \
        return 0;                                                                                                                        \
    }
    MISTARK_FOR_EACH_CONSTRAINT(X)
#undef X
    return -1;
}
