// The K-weighting cascade as a linear recurrence, shared by the meter (loudness.hip) and the stream leveler (leveler.hip): one sample's step,
// the 4 x 4 product and the per-rate table (the coefficients c[10] and A^m, the state transition over one segment of zero input; the segment
// length is loudness_segment_len).  Both files run the same expressions in the same order, so a segment's end state and partial sum have the
// same bits in either.
#pragma once
#include <cstring>

#include "common.h"
#include "loudness.h"

namespace sbv2 {

// one sample through the cascade (transposed direct form II, as scipy.signal.lfilter): returns w, updates the state
__device__ __forceinline__ double kw_step(const double* c, double* s, double x) {
    const double u = fma(c[0], x, s[0]);
    s[0] = fma(c[1], x, fma(-c[3], u, s[1]));
    s[1] = fma(c[2], x, -c[4] * u);
    const double w = fma(c[5], u, s[2]);
    s[2] = fma(c[6], u, fma(-c[8], w, s[3]));
    s[3] = fma(c[7], u, -c[9] * w);
    return w;
}

// r = M v (+ r0)
__device__ __forceinline__ void kw_matvec(const double* M, const double* v, const double* r0, double* r) {
    double t[4];
    for (int i = 0; i < 4; ++i) {
        double a = r0 ? r0[i] : 0.0;
        for (int j = 0; j < 4; ++j) a = fma(M[4 * i + j], v[j], a);
        t[i] = a;
    }
    for (int i = 0; i < 4; ++i) r[i] = t[i];
}

// the cascade's state transition over one sample with zero input (state = shelf s1 s2, high-pass s1 s2)
inline void kw_transition(const double* c, double* A) {
    const double a1 = c[3], a2 = c[4], h0 = c[5], h1 = c[6], h2 = c[7], d1 = c[8], d2 = c[9];
    const double T[16] = {-a1, 1, 0, 0,
                          -a2, 0, 0, 0,
                          h1 - d1 * h0, 0, -d1, 1,
                          h2 - d2 * h0, 0, -d2, 0};
    std::memcpy(A, T, sizeof(T));
}

inline void kw_host_matmul(const double* X, const double* Y, double* R) {
    double t[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += X[4 * i + k] * Y[4 * k + j];
            t[4 * i + j] = s;
        }
    std::memcpy(R, t, sizeof(t));
}

// c[10] and A^m[16] (row-major) of a rate: t[26]; throws for an unsupported rate
inline void kw_table(int rate, double* t) {
    loudness_kweight(rate, t);
    double A1[16];
    kw_transition(t, A1);
    std::memcpy(t + 10, A1, sizeof(A1));
    for (int i = 1, m = loudness_segment_len(rate); i < m; ++i) kw_host_matmul(A1, t + 10, t + 10);
}

}  // namespace sbv2
