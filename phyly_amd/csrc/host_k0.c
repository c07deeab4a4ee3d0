/*
 * host_k0.c -- site-agnostic model preparation on the host ("K0").
 *
 * Product code (host C).  Turns the user's raw rate matrix, rate divisor, root
 * prior and rate-mixture description into what the device engine consumes
 * (plk_set_model): the normalised rate matrix Qn, category rates and priors,
 * and the stationary distribution.  Evaluated in IEEE binary128 (__float128,
 * libquadmath) and rounded once; the normalised matrix is handed over as a
 * double-double (hi, lo) pair so that its rows sum to zero to ~1e-32.
 * P = exp(Qn r t) itself is computed on the GPU.
 *
 * Follows the order of operations of the reference
 * (paths relative to argriffing/phyly):
 *   src/cross_site_ws.c:200-242   cross_site_ws_update_with_edge_rates
 *   src/cross_site_ws.c:175-191   _update_rate_divisor
 *   src/equilibrium.c:21-88       stationary distribution via a bordered solve
 *   src/rate_mixture.c:92-137,167-229,288-339   mixture expectation / gamma / summary
 *   src/gamma_discretization.c:209-370          quantiles and mean / median rates
 */
#include <math.h>
#include <quadmath.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "host_k0.h"
#include "plk.h"

typedef __float128 ld;

/* regularised lower incomplete gamma P(s, x), all-positive series:
 * P = x^s e^-x / Gamma(s+1) * sum_{n>=0} x^n / ((s+1)...(s+n)) */
static ld gamma_p(ld s, ld x)
{
    if (!(x > 0)) return 0;
    if (isinfq(x)) return 1;
    ld lead = s * logq(x) - x - lgammaq(s + 1);
    ld term = 1, sum = 1;
    for (int n = 1; n < 200000; n++) {
        term *= x / (s + n);
        sum += term;
        if (term < sum * 1e-36Q) break;
    }
    ld r = expq(lead) * sum;
    return r > 1 ? 1 : r;
}

/* unit-scale quantile: P(s, q) = p.  Bisection on log2 q, then on q. */
static ld gamma_quantile(ld s, ld p)
{
    ld lo = -16000, hi = 16000;
    if (gamma_p(s, ldexpq(1.0Q, (int)lo)) >= p) return 0;
    for (int it = 0; it < 200; it++) {
        ld mid = 0.5Q * (lo + hi);
        if (gamma_p(s, exp2q(mid)) < p) lo = mid; else hi = mid;
    }
    ld a = exp2q(lo), b = exp2q(hi);
    for (int it = 0; it < 200; it++) {
        ld m = 0.5Q * (a + b);
        if (m <= a || m >= b) break;
        if (gamma_p(s, m) < p) a = m; else b = m;
    }
    return 0.5Q * (a + b);
}

static void gamma_rates(int mode, int n, ld shape, ld *rates)
{
    if (mode == K0_MIX_GAMMA) {
        /* Yang 1994 category means: n * (P(s+1, q_{j+1}) - P(s+1, q_j)) */
        ld prev = 0;
        for (int j = 0; j < n; j++) {
            ld next = 1;
            if (j + 1 < n) next = gamma_p(shape + 1, gamma_quantile(shape, (ld)(j + 1) / (ld)n));
            rates[j] = (next - prev) * n;
            prev = next;
        }
    } else {
        ld tot = 0;
        for (int j = 0; j < n; j++) {
            rates[j] = gamma_quantile(shape, (ld)(2 * j + 1) / (ld)(2 * n));
            tot += rates[j];
        }
        for (int j = 0; j < n; j++) rates[j] = rates[j] / tot * n;
    }
}

/* stationary distribution: [Q^T e; e^T 0][pi; l] = 1, diagonal of Q ignored */
static int equilibrium(int k, const ld *Q, ld *pi)
{
    int n = k + 1, w = n + 1;
    ld *R = calloc((size_t)n * w, sizeof(ld));
    if (!R) return -1;
    for (int i = 0; i < k; i++) {
        ld exitr = 0;
        for (int j = 0; j < k; j++) if (j != i) { exitr += Q[i * k + j]; R[i * w + j] = Q[j * k + i]; }
        R[i * w + i] = -exitr;
        R[i * w + k] = 1;
        R[k * w + i] = 1;
    }
    for (int i = 0; i < n; i++) R[i * w + n] = 1;
    int ok = 0;
    for (int c = 0; c < n; c++) {
        int p = c;
        ld best = fabsq(R[c * w + c]);
        for (int r = c + 1; r < n; r++) if (fabsq(R[r * w + c]) > best) { best = fabsq(R[r * w + c]); p = r; }
        if (best == 0) { ok = -1; break; }
        if (p != c) for (int j = 0; j < w; j++) { ld t = R[c * w + j]; R[c * w + j] = R[p * w + j]; R[p * w + j] = t; }
        for (int r = 0; r < n; r++) {
            if (r == c) continue;
            ld f = R[r * w + c] / R[c * w + c];
            if (f != 0) for (int j = c; j < w; j++) R[r * w + j] -= f * R[c * w + j];
        }
    }
    for (int i = 0; i < k; i++) pi[i] = ok ? (ld)NAN : R[i * w + n] / R[i * w + i];
    free(R);
    return ok;
}

int arbplf_k0_category_count(const k0_mixture *mix)
{
    if (mix->mode == K0_MIX_NONE) return 1;
    if (mix->mode == K0_MIX_CUSTOM || mix->mode == K0_MIX_UNIFORM) return mix->n;
    return mix->n + (mix->invariable_prior != 0 ? 1 : 0);
}

int arbplf_k0_prepare(int k, const double *rate_matrix,
                      int use_equilibrium_divisor, double divisor_value, int need_equilibrium,
                      const k0_mixture *mix,
                      double *cat_rates, double *cat_prior, double *pi_out, double *Qn_out, double *Qn_lo_out)
{
    const int C = arbplf_k0_category_count(mix);
    ld expect = 1;
    ld *rates = calloc((size_t)C, sizeof(ld));
    if (!rates) return -1;
    if (mix->mode == K0_MIX_NONE) {
        rates[0] = 1; cat_prior[0] = 1;
    } else if (mix->mode == K0_MIX_CUSTOM) {
        expect = 0;
        for (int i = 0; i < C; i++) { rates[i] = mix->rates[i]; cat_prior[i] = mix->prior[i]; expect += (ld)mix->rates[i] * (ld)mix->prior[i]; }
    } else if (mix->mode == K0_MIX_UNIFORM) {
        expect = 0;
        for (int i = 0; i < C; i++) { rates[i] = mix->rates[i]; cat_prior[i] = (double)(1.0Q / (ld)C); expect += (ld)mix->rates[i]; }
        expect /= C;
    } else {
        ld p = mix->invariable_prior, q = 1 - p;
        gamma_rates(mix->mode, mix->n, (ld)mix->gamma_shape, rates);
        for (int i = 0; i < mix->n; i++) { rates[i] /= q; cat_prior[i] = (double)(q / mix->n); }
        if (mix->invariable_prior != 0) { rates[mix->n] = 0; cat_prior[mix->n] = mix->invariable_prior; }
        expect = 1;
    }
    for (int i = 0; i < C; i++) cat_rates[i] = (double)rates[i];
    free(rates);

    const size_t kk = (size_t)k * k;
    ld *Q = malloc(kk * sizeof(ld)), *pi = calloc((size_t)k, sizeof(ld));
    if (!Q || !pi) { free(Q); free(pi); return -1; }
    for (size_t i = 0; i < kk; i++) Q[i] = rate_matrix[i];
    if (need_equilibrium) equilibrium(k, Q, pi);
    for (int i = 0; i < k; i++) { Q[i * k + i] = 0; pi_out[i] = (double)pi[i]; }
    ld divisor = divisor_value;
    if (use_equilibrium_divisor) {
        divisor = 0;
        for (int i = 0; i < k; i++) {
            ld rs = 0;
            for (int j = 0; j < k; j++) rs += Q[i * k + j];
            divisor += rs * pi[i];
        }
        divisor *= expect;
    }
    for (int i = 0; i < k; i++) {
        ld rs = 0;
        for (int j = 0; j < k; j++) if (j != i) { Q[i * k + j] /= divisor; rs += Q[i * k + j]; }
        Q[i * k + i] = -rs;
    }
    for (size_t i = 0; i < kk; i++) {
        Qn_out[i] = (double)Q[i];
        if (Qn_lo_out) Qn_lo_out[i] = (double)(Q[i] - (ld)Qn_out[i]);
    }
    free(Q); free(pi);
    return C;
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* chain rule of arbplf-mixture-deriv (include/plk.h: plk_mixture_chain)                                             */
/* ---------------------------------------------------------------------------------------------------------------- */

static int mix_fail(char *err, size_t errlen, const char *msg)
{
    if (err && errlen) snprintf(err, errlen, "%s", msg);
    return PLK_E_ARG;
}

/*
 * dg[j] = d g_j / d shape of gamma_rates, in binary128: central differences at h and h / 2 with h = shape * 2^-17 and
 * one Richardson step, D = (4 D(h/2) - D(h)) / 3.
 * Estimate, relative to max_j |g_j'|: gamma_rates is analytic in the shape and is evaluated to about 1e-32 relative
 * (series cut at 1e-36, quantiles bisected to the last bit), so rounding contributes about 1e-32 / 2^-17 * 3 ~ 4e-27 in
 * units of g / shape.  D(h) = g' + h^2 g''' / 6 + h^4 g^(5) / 120 + ..., so the Richardson step leaves -h^4 g^(5) / 480:
 * with h / shape = 7.6e-6, (h / shape)^4 / 480 = 7e-24 times shape^4 g^(5) / g', which would have to reach 1e8 to matter
 * (it is below 1e3 for 0.05 <= shape <= 100).  Both stay far below 1e-15.
 */
static int gamma_rates_deriv(int mode, int n, ld shape, ld *dg)
{
    ld *buf = calloc((size_t)4 * n, sizeof(ld));
    if (!buf) return -1;
    const ld h = ldexpq(shape, -17);
    gamma_rates(mode, n, shape + h, buf);
    gamma_rates(mode, n, shape - h, buf + n);
    gamma_rates(mode, n, shape + h / 2, buf + 2 * n);
    gamma_rates(mode, n, shape - h / 2, buf + 3 * n);
    for (int j = 0; j < n; j++) {
        const ld d1 = (buf[j] - buf[n + j]) / (2 * h), d2 = (buf[2 * n + j] - buf[3 * n + j]) / h;
        dg[j] = (4 * d2 - d1) / 3;
    }
    free(buf);
    return 0;
}

int plk_mixture_chain(int mode, int n, const double *rates, const double *prior, double gamma_shape, double invariable_prior,
                      int divisor_mode, const double *prior_sens, const double *rate_sens,
                      double *drates_out, double *dprior_out, double *dshape_out, double *dinvariable_out,
                      int *has_invariable_out, char *err, size_t errlen)
{
    if (err && errlen) err[0] = 0;
    if (has_invariable_out) *has_invariable_out = 0;
    if (mode == K0_MIX_NONE) return mix_fail(err, errlen, "plk_mixture_chain: the model has no rate mixture, there is nothing to differentiate");
    if (mode != K0_MIX_CUSTOM && mode != K0_MIX_UNIFORM && mode != K0_MIX_GAMMA && mode != K0_MIX_GAMMA_MEDIAN)
        return mix_fail(err, errlen, "plk_mixture_chain: bad rate mixture mode");
    if (n < 1 || !prior_sens || !rate_sens) return mix_fail(err, errlen, "plk_mixture_chain: bad arguments");
    if (divisor_mode != PLK_DIVISOR_NUMBER && divisor_mode != PLK_DIVISOR_EXIT_RATE) return mix_fail(err, errlen, "plk_mixture_chain: bad divisor form");
#define SENS(a, c) ((ld)(a)[2 * (c)] + (ld)(a)[2 * (c) + 1])
    if (mode == K0_MIX_CUSTOM || mode == K0_MIX_UNIFORM) {
        if (!rates || !drates_out || (mode == K0_MIX_CUSTOM && (!prior || !dprior_out))) return mix_fail(err, errlen, "plk_mixture_chain: bad arguments");
        /* the divisor of the exit-rate form carries expect = sum_c r_c p_c: f(Qn / expect), and df/d(scale of Qn) = T */
        ld expect = 0, T = 0;
        for (int c = 0; c < n; c++) {
            const ld p = mode == K0_MIX_CUSTOM ? (ld)prior[c] : 1.0Q / (ld)n;
            expect += (ld)rates[c] * p;
            T += (ld)rates[c] * SENS(rate_sens, c);
        }
        const int exitr = divisor_mode == PLK_DIVISOR_EXIT_RATE;
        if (exitr && !(expect != 0 && finiteq(expect))) return mix_fail(err, errlen, "plk_mixture_chain: the expected rate of the mixture is zero, the exit-rate divisor is undefined");
        for (int c = 0; c < n; c++) {
            const ld p = mode == K0_MIX_CUSTOM ? (ld)prior[c] : 1.0Q / (ld)n;
            drates_out[c] = (double)(SENS(rate_sens, c) - (exitr ? p * T / expect : 0));
            if (mode == K0_MIX_CUSTOM) dprior_out[c] = (double)(SENS(prior_sens, c) - (exitr ? (ld)rates[c] * T / expect : 0));
        }
        return PLK_OK;
    }
    if (!dshape_out) return mix_fail(err, errlen, "plk_mixture_chain: bad arguments");
    if (!(gamma_shape > 0) || !isfinite(gamma_shape)) return mix_fail(err, errlen, "plk_mixture_chain: gamma_shape must be positive");
    if (!(invariable_prior >= 0 && invariable_prior < 1)) return mix_fail(err, errlen, "plk_mixture_chain: invariable_prior must be in [0, 1)");
    const int inv = invariable_prior != 0;
    if (inv && !dinvariable_out) return mix_fail(err, errlen, "plk_mixture_chain: bad arguments");
    ld *g = calloc((size_t)2 * n, sizeof(ld));
    if (!g) return PLK_E_NOMEM;
    ld *dg = g + n;
    gamma_rates(mode, n, (ld)gamma_shape, g);
    if (gamma_rates_deriv(mode, n, (ld)gamma_shape, dg)) { free(g); return PLK_E_NOMEM; }
    const ld q = 1 - (ld)invariable_prior;
    ld dshape = 0, dpi = 0;
    for (int j = 0; j < n; j++) {
        dshape += SENS(rate_sens, j) * dg[j] / q;
        dpi += SENS(rate_sens, j) * (g[j] / q) / q - SENS(prior_sens, j) / (ld)n;
    }
    *dshape_out = (double)dshape;
    if (inv) {
        *dinvariable_out = (double)(dpi + SENS(prior_sens, n));
        if (has_invariable_out) *has_invariable_out = 1;
    }
#undef SENS
    free(g);
    return PLK_OK;
}
