/* include/bre_fmath.h's bre_sincos_2pi as a shared library for tests/test_glossy_refpy.py (built with the flags of
   tests/test_fmath_libm.py: no contraction, so the host evaluates exactly what the device does). */
#include "bre_fmath.h"

void fmath_sincos_2pi(const double *phi, long n, double *s, double *c) {
    for (long i = 0; i < n; ++i) bre_sincos_2pi(phi[i], &s[i], &c[i]);
}
