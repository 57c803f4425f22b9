// jacobi_f32.h -- OpenCV 2.4.9's JacobiSVDImpl_<float> (modules/core/src/lapack.cpp) for any (rows, length), as DESIGN.md
// section 4 reads it: one-sided Hestenes on the N rows of `At`, each of length M, with W and the inner products in double and
// the rotation's c and s narrowed to float; cyclic (i, j) sweeps, at most max(M, 30), until one rotates nothing; W = the row
// norms; a selection sort to descending W that swaps the rows of At and Vt; then the completion loop, which scales row i by
// (float)(1/W[i]) and GENERATES a row whose W is <= FLT_MIN, or that lies past N, from cv::RNG(0x12345678) and two rounds of
// Gram-Schmidt.  tests/init_reference.py states the same steps with numpy scalars and is the definition.
//
// Element (i, k) of a matrix lives at [(i*cols + k)*S]: S = 1 for one matrix in LDS, S = the workgroup size for one matrix per
// thread laid out element-major (no bank conflicts, no private memory).  The loops are not unrolled: the matrices are meant
// for LDS, where a runtime index costs nothing.  Every operation goes through an _rn intrinsic, so no contraction changes a bit.
#ifndef PG_JACOBI_F32_H
#define PG_JACOBI_F32_H
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define JF_HD __device__ __forceinline__
JF_HD float jf_add(float a, float b) { return __fadd_rn(a, b); }
JF_HD float jf_sub(float a, float b) { return __fsub_rn(a, b); }
JF_HD float jf_mul(float a, float b) { return __fmul_rn(a, b); }
JF_HD float jf_div(float a, float b) { return __fdiv_rn(a, b); }
JF_HD double jd_add(double a, double b) { return __dadd_rn(a, b); }
JF_HD double jd_sub(double a, double b) { return __dsub_rn(a, b); }
JF_HD double jd_mul(double a, double b) { return __dmul_rn(a, b); }
JF_HD double jd_div(double a, double b) { return __ddiv_rn(a, b); }
JF_HD double jd_sqrt(double a) { return __dsqrt_rn(a); }
JF_HD float jd_f(double a) { return __double2float_rn(a); }
// a float square root: the double root rounded once more gives the correctly rounded float root
JF_HD float jf_sqrt(float a) { return jd_f(jd_sqrt((double)a)); }

#define JF_FLT_MIN 1.1754943508222875e-38
#define JF_COMPLETION_TRIES 4

// OpenCV's hypot template in double
JF_HD double jf_hypot(double a, double b)
{
    a = fabs(a); b = fabs(b);
    if (a > b) { b = jd_div(b, a); return jd_mul(a, jd_sqrt(jd_add(1.0, jd_mul(b, b)))); }
    if (b > 0) { a = jd_div(a, b); return jd_mul(b, jd_sqrt(jd_add(1.0, jd_mul(a, a)))); }
    return 0.0;
}

// The Jacobi up to and including the sort.  At: N rows of M (modified: the rotated, sorted rows, not normalised); Vt: null or
// N rows of N, set to the identity here; W [N]: the singular values in double, descending.
template <int N, int M, int S>
JF_HD void jf_jacobi(float* At, float* Vt, double* W)
{
    for (int i = 0; i < N; i++) {
        double sd = 0.0;
        for (int k = 0; k < M; k++) { const double t = (double)At[(i * M + k) * S]; sd = jd_add(sd, jd_mul(t, t)); }
        W[i * S] = sd;
        if (Vt) for (int k = 0; k < N; k++) Vt[(i * N + k) * S] = i == k ? 1.f : 0.f;
    }
    const double eps = (double)2.3841857910156250e-07f;             // FLT_EPSILON*2
    const int maxIter = M > 30 ? M : 30;
    for (int iter = 0; iter < maxIter; iter++) {
        bool changed = false;
        for (int i = 0; i < N - 1; i++)
            for (int j = i + 1; j < N; j++) {
                float* Ai = At + i * M * S;
                float* Aj = At + j * M * S;
                const double a = W[i * S], b = W[j * S];
                double p = 0.0;
                for (int k = 0; k < M; k++) p = jd_add(p, jd_mul((double)Ai[k * S], (double)Aj[k * S]));
                if (fabs(p) <= jd_mul(eps, jd_sqrt(jd_mul(a, b)))) continue;
                p = jd_mul(p, 2.0);
                const double beta = jd_sub(a, b), gamma = jf_hypot(p, beta);
                float c, s;
                if (beta < 0) {
                    const double delta = jd_mul(jd_sub(gamma, beta), 0.5);
                    s = jd_f(jd_sqrt(jd_div(delta, gamma)));
                    c = jd_f(jd_div(p, jd_mul(jd_mul(gamma, (double)s), 2.0)));
                } else {
                    c = jd_f(jd_sqrt(jd_div(jd_add(gamma, beta), jd_mul(gamma, 2.0))));
                    s = jd_f(jd_div(p, jd_mul(jd_mul(gamma, (double)c), 2.0)));
                }
                double na = 0.0, nb = 0.0;
                for (int k = 0; k < M; k++) {
                    const float x = Ai[k * S], y = Aj[k * S];
                    const float t0 = jf_add(jf_mul(c, x), jf_mul(s, y));
                    const float t1 = jf_add(jf_mul(-s, x), jf_mul(c, y));
                    Ai[k * S] = t0; Aj[k * S] = t1;
                    na = jd_add(na, jd_mul((double)t0, (double)t0)); nb = jd_add(nb, jd_mul((double)t1, (double)t1));
                }
                W[i * S] = na; W[j * S] = nb;
                changed = true;
                if (Vt) {
                    float* Vi = Vt + i * N * S;
                    float* Vj = Vt + j * N * S;
                    for (int k = 0; k < N; k++) {
                        const float x = Vi[k * S], y = Vj[k * S];
                        Vi[k * S] = jf_add(jf_mul(c, x), jf_mul(s, y));
                        Vj[k * S] = jf_add(jf_mul(-s, x), jf_mul(c, y));
                    }
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < N; i++) {
        double sd = 0.0;
        for (int k = 0; k < M; k++) { const double t = (double)At[(i * M + k) * S]; sd = jd_add(sd, jd_mul(t, t)); }
        W[i * S] = jd_sqrt(sd);
    }
    for (int i = 0; i < N - 1; i++) {
        int j = i;
        for (int k = i + 1; k < N; k++) if (W[j * S] < W[k * S]) j = k;
        if (i != j) {
            const double tw = W[i * S]; W[i * S] = W[j * S]; W[j * S] = tw;
            for (int k = 0; k < M; k++) { const float t = At[(i * M + k) * S]; At[(i * M + k) * S] = At[(j * M + k) * S]; At[(j * M + k) * S] = t; }
            if (Vt) for (int k = 0; k < N; k++) { const float t = Vt[(i * N + k) * S]; Vt[(i * N + k) * S] = Vt[(j * N + k) * S]; Vt[(j * N + k) * S] = t; }
        }
    }
}

// cv::RNG::next(): the multiply-with-carry generator
JF_HD uint32_t jf_rng_next(uint64_t& state)
{
    state = (uint64_t)(uint32_t)state * 4164903690ull + (state >> 32);
    return (uint32_t)state;
}

// The completion loop over rows 0 .. N1-1 of At (room for N1 rows of M; W holds N values): see the head of this file.  The
// generation is a `while (sd <= minval)` in OpenCV; it is bounded at JF_COMPLETION_TRIES rounds here and in the reference.
template <int N, int M, int N1, int S>
JF_HD void jf_complete(float* At, const double* W)
{
    uint64_t rng = 0x12345678ull;
    for (int i = 0; i < N1; i++) {
        float* Ai = At + i * M * S;
        double sd = i < N ? W[i * S] : 0.0;
        for (int tries = 0; sd <= JF_FLT_MIN && tries < JF_COMPLETION_TRIES; tries++) {
            const float val0 = jd_f(jd_div(1.0, (double)M));
            for (int k = 0; k < M; k++) Ai[k * S] = (jf_rng_next(rng) & 256) != 0 ? val0 : -val0;
            for (int iter = 0; iter < 2; iter++)
                for (int j = 0; j < i; j++) {
                    const float* Aj = At + j * M * S;
                    sd = 0.0;
                    for (int k = 0; k < M; k++) sd = jd_add(sd, (double)jf_mul(Ai[k * S], Aj[k * S]));
                    float asum = 0.f;
                    for (int k = 0; k < M; k++) {
                        const float t = jd_f(jd_sub((double)Ai[k * S], jd_mul(sd, (double)Aj[k * S])));
                        Ai[k * S] = t;
                        asum = jf_add(asum, fabsf(t));
                    }
                    asum = asum != 0.f ? jf_div(1.f, asum) : 0.f;
                    for (int k = 0; k < M; k++) Ai[k * S] = jf_mul(Ai[k * S], asum);
                }
            sd = 0.0;
            for (int k = 0; k < M; k++) { const double t = (double)Ai[k * S]; sd = jd_add(sd, jd_mul(t, t)); }
            sd = jd_sqrt(sd);
        }
        const float s = jd_f(jd_div(1.0, sd));
        for (int k = 0; k < M; k++) Ai[k * S] = jf_mul(Ai[k * S], s);
    }
}
#endif
