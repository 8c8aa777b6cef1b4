// TEST-ONLY host build of the stress readout's constitutive header (stark_amd/csrc/stress.hpp compiled with g++): lets the CPU test suite check the
// exact device arithmetic against the numpy reference of tests/stress_ref.py without a GPU. Not part of the product library.
#include "../../stark_amd/csrc/stress.hpp"

using namespace mistark;

// in: [n_elem][nin] gathered inputs in binding order, rec: [n_elem][16]; kind 0 tet, 1 triangle, 2 segment
extern "C" int host_stress_eval(int kind, int full, const double* in, int nin, int n_elem, double* rec)
{
    for (int e = 0; e < n_elem; e++) {
        const double* ie = in + (size_t)e * nin;
        double* re = rec + (size_t)e * STRESS_REC;
        if (kind == 0) full ? tet_stress<true>(ie, re) : tet_stress<false>(ie, re);
        else if (kind == 1) full ? tri_stress<true>(ie, re) : tri_stress<false>(ie, re);
        else if (kind == 2) full ? seg_stress<true>(ie, re) : seg_stress<false>(ie, re);
        else return -1;
    }
    return 0;
}
