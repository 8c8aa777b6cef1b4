// TEST-ONLY host build of ONE emitted user-defined potential: the two functions prog_energy / prog_condition that custom.hip's emitter wrote
// (cut out of the source mistark_custom_emit returns, tests/test_custom_cases_cpu.py) compiled with g++ against the repository's own hdual.hpp
// and custom_math.hpp, and evaluated with every (i <= j) seed per element like the emitted kernels do. It checks the register allocator's
// output and the emitter's text without a GPU. Not part of the product library.
//   g++ -D__device__= -D__forceinline__=inline -DHOST_CUSTOM_PROG='"<file with the two functions>"' -DHOST_CUSTOM_NIN=<inputs> -DHOST_CUSTOM_NB=<blocks>
//       [-DHOST_CUSTOM_COND]
#include <cstring>
#include "../../stark_amd/csrc/hdual.hpp"
#include "../../stark_amd/csrc/custom_math.hpp"

static inline double __longlong_as_double(long long b) { double v; std::memcpy(&v, &b, 8); return v; }

using namespace mistark;
#include HOST_CUSTOM_PROG

// in: [n_elem, NIN] gathered inputs; E [n_elem], g [n_elem, n], H [n_elem, n, n], active [n_elem]; an inactive element is not evaluated (zeros)
extern "C" int host_custom_eval(const double* in, int n_elem, double* E, double* g, double* H, int* active)
{
    constexpr int NIN = HOST_CUSTOM_NIN, n = 3 * HOST_CUSTOM_NB;
    for (int e = 0; e < n_elem; e++) {
        double x[NIN > 0 ? NIN : 1];
        std::memcpy(x, in + (size_t)e * NIN, sizeof(double) * NIN);
        bool on = true;
#ifdef HOST_CUSTOM_COND
        on = prog_condition(x, -1, -1).v > 0.0;
#endif
        active[e] = on ? 1 : 0;
        E[e] = 0.0;
        for (int k = 0; k < n; k++) g[(size_t)e * n + k] = 0.0;
        for (int k = 0; k < n * n; k++) H[(size_t)e * n * n + k] = 0.0;
        if (!on) continue;
        E[e] = prog_energy(x, -1, -1).v;
        for (int i = 0; i < n; i++)
            for (int j = i; j < n; j++) {
                const HDual r = prog_energy(x, i, j);
                H[((size_t)e * n + i) * n + j] = r.ab;
                H[((size_t)e * n + j) * n + i] = r.ab;
                if (i == j) g[(size_t)e * n + i] = r.a;
            }
    }
    return 0;
}
