// TEST-ONLY host build of the spectrum report's per-element header (stark_amd/csrc/spectrum_report.hpp compiled with g++): lets the CPU test suite check
// the record function against exact spectra (tests/psd_cases.py) and the numpy restatement (tests/spectrum_ref.py) without a GPU. Not part of the product.
#include "../../stark_amd/csrc/spectrum_report.hpp"

#include <cstddef>

using namespace mistark;

template <int NB>
static void run(const double* H, int ne, double eps, double* rec, double* spec)
{
    constexpr int n = 3 * NB;
    for (int e = 0; e < ne; e++) spectrum_record<n>(H + (size_t)e * n * n, eps, rec + (size_t)e * SPEC_REC, spec ? spec + (size_t)e * n : nullptr);
}

// H: [ne][3 nb][3 nb] row-major, rec: [ne][10], spec: [ne][3 nb] or null
extern "C" int host_spectrum_eval(int nb, const double* H, int ne, double eps, double* rec, double* spec)
{
    switch (nb) {
        case 1: run<1>(H, ne, eps, rec, spec); break;
        case 2: run<2>(H, ne, eps, rec, spec); break;
        case 3: run<3>(H, ne, eps, rec, spec); break;
        case 4: run<4>(H, ne, eps, rec, spec); break;
        case 5: run<5>(H, ne, eps, rec, spec); break;
        case 6: run<6>(H, ne, eps, rec, spec); break;
        case 7: run<7>(H, ne, eps, rec, spec); break;
        case 8: run<8>(H, ne, eps, rec, spec); break;
        default: return -1;
    }
    return 0;
}
