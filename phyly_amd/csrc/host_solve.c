/*
 * host_solve.c -- the solve behind arbplf-inv-hess, arbplf-newton-delta and arbplf-newton-update
 * (src/arbplfhess.c:169-234: inverse Hessian, delta = -H^-1 g).  Host only, no engine involved.
 *
 * The reference solves in ball arithmetic and raises the precision until the result is certified; a singular Hessian
 * never gets there (src/arbplfhess.c:1225-1236).  Here: Gauss-Jordan elimination with partial pivoting on [H | I] in IEEE
 * binary128 on the (hi, lo) entries, rounded once to double, and a refusal where no digit of the result would mean anything.
 *
 * Also here, for the same reason (host only, binary128, rounded once): plk_rate_matrix_chain, the chain rule from the
 * gradient in the normalised rate matrix to the entries of the user's rate_matrix (arbplf-rate-matrix-deriv).
 */
#include <quadmath.h>
#include <stdio.h>
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

/* ---------------------------------------------------------------------------------------------------------------- */
/* chain rule of arbplf-rate-matrix-deriv (include/plk.h: plk_rate_matrix_chain)                                     */
/* ---------------------------------------------------------------------------------------------------------------- */

/* Gauss-Jordan with partial pivoting on the n x w matrix R (n <= w), reducing its left n x n block to the identity.
 * A pivot at or below tiny counts as zero: -1. */
static int qd_gauss_jordan(qd *R, size_t n, size_t w, qd tiny)
{
    for (size_t c = 0; c < n; c++) {
        size_t p = c;
        qd best = fabsq(R[c * w + c]);
        for (size_t r = c + 1; r < n; r++) if (fabsq(R[r * w + c]) > best) { best = fabsq(R[r * w + c]); p = r; }
        if (!(best > tiny)) return -1;
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
    return 0;
}

static int chain_fail(char *err, size_t errlen, const char *msg)
{
    if (err && errlen) snprintf(err, errlen, "%s", msg);
    return PLK_E_ARG;
}

int plk_rate_matrix_chain(int k, const double *rate_matrix, int divisor_mode, double divisor, int root_mode,
                          const double *G, const double *root, double *grad_out, char *err, size_t errlen)
{
    if (err && errlen) err[0] = 0;
    if (k < 1 || !rate_matrix || !G || !grad_out) return chain_fail(err, errlen, "plk_rate_matrix_chain: bad arguments");
    if (divisor_mode != PLK_DIVISOR_NUMBER && divisor_mode != PLK_DIVISOR_EXIT_RATE) return chain_fail(err, errlen, "plk_rate_matrix_chain: bad divisor form");
    if (divisor_mode == PLK_DIVISOR_NUMBER && !(divisor > 0)) return chain_fail(err, errlen, "plk_rate_matrix_chain: the divisor must be greater than zero");
    const int eq_root = root_mode == PLK_ROOT_EQUILIBRIUM;
    if (eq_root && !root) return chain_fail(err, errlen, "plk_rate_matrix_chain: the equilibrium root prior needs the root gradient");
    const int need_pi = eq_root || divisor_mode == PLK_DIVISOR_EXIT_RATE;
    const size_t n = (size_t)k, nn = n * n;
    qd *Q = malloc((nn + 1) * sizeof(qd)), *Gq = malloc((nn + 1) * sizeof(qd));
    qd *A = NULL, *Z = NULL, *pi = NULL, *v = NULL;
    int rc = PLK_OK;
    if (!Q || !Gq) { rc = PLK_E_NOMEM; goto done; }
    qd qmax = 0;
    for (size_t i = 0; i < n; i++) {
        qd row = 0;
        for (size_t j = 0; j < n; j++) {
            Gq[i * n + j] = (qd)G[2 * (i * n + j)] + (qd)G[2 * (i * n + j) + 1];
            if (i == j) continue;
            const qd q = rate_matrix[i * n + j];
            if (!(q >= 0) || !finiteq(q)) { rc = chain_fail(err, errlen, "plk_rate_matrix_chain: rate_matrix entries must be finite and non-negative"); goto done; }
            Q[i * n + j] = q;
            row += q;
            if (q > qmax) qmax = q;
        }
        Q[i * n + i] = -row;
    }
    qd d = divisor;
    if (need_pi) {
        /* pi^T Q = 0, sum pi = 1: Q^T with its last equation replaced by the normalisation */
        A = malloc(n * (n + 1) * sizeof(qd));
        Z = malloc(n * 2 * n * sizeof(qd));
        pi = malloc(n * sizeof(qd));
        v = malloc(n * sizeof(qd));
        if (!A || !Z || !pi || !v) { rc = PLK_E_NOMEM; goto done; }
        const qd tiny = qmax * 0x1p-80q;
        for (size_t r = 0; r < n; r++) {
            for (size_t c = 0; c < n; c++) A[r * (n + 1) + c] = r + 1 < n ? Q[c * n + r] : (qmax > 0 ? qmax : 1);
            A[r * (n + 1) + n] = r + 1 < n ? 0 : (qmax > 0 ? qmax : 1);
        }
        if (qd_gauss_jordan(A, n, n + 1, tiny)) { rc = chain_fail(err, errlen, "rate matrix is reducible: its stationary distribution is not unique"); goto done; }
        for (size_t m = 0; m < n; m++) pi[m] = A[m * (n + 1) + n];
        /* Z = (1 pi^T - Q)^-1 */
        for (size_t r = 0; r < n; r++)
            for (size_t c = 0; c < n; c++) {
                Z[r * 2 * n + c] = pi[c] * (qmax > 0 ? qmax : 1) - Q[r * n + c];      /* (qmax 1 pi^T - Q): same inverse action on */
                Z[r * 2 * n + n + c] = r == c ? 1 : 0;                               /* vectors orthogonal to 1, better scaled  */
            }
        if (qd_gauss_jordan(Z, n, 2 * n, tiny)) { rc = chain_fail(err, errlen, "rate matrix is reducible: its stationary distribution is not unique"); goto done; }
        if (divisor_mode == PLK_DIVISOR_EXIT_RATE) {
            d = 0;
            for (size_t m = 0; m < n; m++) d += pi[m] * -Q[m * n + m];
            if (!(d > 0)) { rc = chain_fail(err, errlen, "plk_rate_matrix_chain: the equilibrium exit rate is zero"); goto done; }
        }
        /* v_m: the coefficient of dpi_m in df: root_m (equilibrium prior) + (df/dd)(-Q_mm) (exit-rate divisor) */
        qd dfdd = 0;
        if (divisor_mode == PLK_DIVISOR_EXIT_RATE) {
            for (size_t i = 0; i < nn; i++) dfdd += Gq[i] * (Q[i] / d);
            dfdd = -dfdd / d;
        }
        for (size_t m = 0; m < n; m++) {
            v[m] = 0;
            if (eq_root) v[m] += (qd)root[2 * m] + (qd)root[2 * m + 1];
            if (divisor_mode == PLK_DIVISOR_EXIT_RATE) v[m] += dfdd * -Q[m * n + m];
        }
        /* u = Z v: dpi/dq_ij . v = pi_i (u_j - u_i).  (Z above inverts qmax 1 pi^T - Q; on e_j - e_i, whose image under the
         * true Z has zero sum, (e_j - e_i)^T Z is the same row vector: both inverses agree on the complement of pi) */
        for (size_t r = 0; r < n; r++) {
            qd acc = 0;
            for (size_t c = 0; c < n; c++) acc += Z[r * 2 * n + n + c] * v[c];
            A[r] = acc;                              /* A is free now: u */
        }
        for (size_t i = 0; i < n; i++)
            for (size_t j = 0; j < n; j++) {
                if (i == j) { grad_out[i * n + j] = 0; continue; }
                qd g = (Gq[i * n + j] - Gq[i * n + i]) / d + pi[i] * (A[j] - A[i]);
                if (divisor_mode == PLK_DIVISOR_EXIT_RATE) g += dfdd * pi[i];
                grad_out[i * n + j] = (double)g;
            }
    } else {
        for (size_t i = 0; i < n; i++)
            for (size_t j = 0; j < n; j++)
                grad_out[i * n + j] = i == j ? 0 : (double)((Gq[i * n + j] - Gq[i * n + i]) / d);
    }
done:
    free(Q); free(Gq); free(A); free(Z); free(pi); free(v);
    return rc;
}
