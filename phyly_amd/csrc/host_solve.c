/*
 * host_solve.c -- the solve behind arbplf-inv-hess, arbplf-newton-delta and arbplf-newton-update
 * (src/arbplfhess.c:169-234: inverse Hessian, delta = -H^-1 g).  Host only, no engine involved.
 *
 * The reference solves in ball arithmetic and raises the precision until the result is certified; a singular Hessian
 * never gets there (src/arbplfhess.c:1225-1236).  Here: Gauss-Jordan elimination with partial pivoting on [H | I] in IEEE
 * binary128 on the (hi, lo) entries, rounded once to double, and a refusal where no digit of the result would mean anything.
 */
#include <quadmath.h>
#include <stdlib.h>

#include "plk.h"

typedef __float128 qd;

/* the Hessian is good to 1e-11 of its largest entry (tests/test_gpu_hess.py): with cond_inf(H) * E * 1e-11 >= 1 the
 * first-order perturbation bound of the solve exceeds the solution itself */
#define PLK_HESS_REL_ERR 1e-11

int plk_solve_second_order(int E, const double *hess, const double *grad, double *inv_out, double *delta_out, double *cond_out)
{
    if (E < 1 || !hess || (delta_out && !grad)) return PLK_E_ARG;
    const size_t n = (size_t)E, w = 2 * n;
    qd *R = malloc(n * w * sizeof(qd));            /* [H | I] -> [I | H^-1] */
    if (!R) return PLK_E_NOMEM;
    int rc = PLK_OK;
    qd hnorm = 0;
    for (size_t i = 0; i < n; i++) {
        qd row = 0;
        for (size_t j = 0; j < n; j++) {
            const qd v = (qd)hess[2 * (i * n + j)] + (qd)hess[2 * (i * n + j) + 1];
            R[i * w + j] = v;
            R[i * w + n + j] = i == j ? 1 : 0;
            row += fabsq(v);
        }
        if (row > hnorm) hnorm = row;
    }
    if (!(hnorm > 0) || !finiteq(hnorm)) { rc = PLK_E_ARG; goto done; }
    /* Gauss-Jordan with partial pivoting */
    for (size_t c = 0; c < n; c++) {
        size_t p = c;
        qd best = fabsq(R[c * w + c]);
        for (size_t r = c + 1; r < n; r++) if (fabsq(R[r * w + c]) > best) { best = fabsq(R[r * w + c]); p = r; }
        if (!(best > 0)) { rc = PLK_E_ARG; goto done; }
        if (p != c) for (size_t j = 0; j < w; j++) { const qd t = R[c * w + j]; R[c * w + j] = R[p * w + j]; R[p * w + j] = t; }
        const qd piv = R[c * w + c];
        for (size_t j = 0; j < w; j++) R[c * w + j] /= piv;
        for (size_t r = 0; r < n; r++) {
            if (r == c) continue;
            const qd f = R[r * w + c];
            if (f == 0) continue;
            for (size_t j = c; j < w; j++) R[r * w + j] -= f * R[c * w + j];
        }
    }
    /* symmetrise, condition number in the infinity norm */
    qd inorm = 0;
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < i; j++) {
            const qd v = (R[i * w + n + j] + R[j * w + n + i]) / 2;
            R[i * w + n + j] = R[j * w + n + i] = v;
        }
    for (size_t i = 0; i < n; i++) {
        qd row = 0;
        for (size_t j = 0; j < n; j++) row += fabsq(R[i * w + n + j]);
        if (row > inorm) inorm = row;
    }
    const qd cond = hnorm * inorm;
    if (cond_out) *cond_out = (double)cond;
    if (!finiteq(cond) || !(cond * (qd)E * (qd)PLK_HESS_REL_ERR < 1)) { rc = PLK_E_ARG; goto done; }
    if (inv_out)
        for (size_t i = 0; i < n; i++)
            for (size_t j = 0; j < n; j++) inv_out[i * n + j] = (double)R[i * w + n + j];
    if (delta_out)
        for (size_t i = 0; i < n; i++) {
            qd acc = 0;
            for (size_t j = 0; j < n; j++) acc += R[i * w + n + j] * ((qd)grad[2 * j] + (qd)grad[2 * j + 1]);
            delta_out[i] = (double)(-acc);
        }
done:
    free(R);
    return rc;
}
