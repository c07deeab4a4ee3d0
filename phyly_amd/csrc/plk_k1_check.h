/*
 * plk_k1_check.h -- what K1 (k_expm_dd: P = exp(Qn r_c t_e) by scaling and squaring) accepts, and how many squarings
 * it runs.  Plain C99 / C++ with no HIP in it: the engine (plk_engine.hip), the drivers (host_drivers.c) and a
 * stand-alone test program include it.  The checks are host code; plk_k1_squarings is what the kernel itself calls, for
 * which the engine gives it the device qualifier through PLK_K1_FN.  DESIGN.md section 6 has the derivation of the limit.
 *
 * K1 scales s Qn (s = r_c t_e) down by 2^sq to infinity norm <= 2^-5 and squares the Taylor polynomial sq times.  Each
 * squaring can double the drift of the row sums, so the error of a row is at most k 2^sq 2^-104; keeping it below 2^-53
 * at k = 64 gives sq <= 45, that is s |Qn| <= 2^-5 2^45 = 2^40 (about 1e12 expected substitutions on one edge).
 * Values beyond it, negative rates or priors and anything not finite are refused (PLK_E_ARG) before a kernel sees them.
 */
#ifndef PLK_K1_CHECK_H
#define PLK_K1_CHECK_H

#include <math.h>
#include <stddef.h>
#include <stdio.h>

#define PLK_K1_MAX_NORM 1099511627776.0   /* 2^40 */
/* the squarings of the largest finite double (2^1024 (1 - 2^-53): exponent 1024, + 5) stay below it, so the clamp
 * changes no count a finite norm had; a norm that is not finite gets exactly this many */
#define PLK_K1_MAX_SQ 1030

/* the qualifier of plk_k1_squarings: a file that also calls it from a kernel defines it before the include */
#ifndef PLK_K1_FN
#define PLK_K1_FN static inline
#endif

/* The smallest sq >= 0 with norm 2^-sq <= 2^-5, from the exponent of norm: what the loop
 * `while (norm > 0.03125) { norm *= 0.5; sq++; }` counts for every finite norm, without a loop an input could keep
 * running.  norm = m 2^ex with m in [0.5, 1): norm 2^-sq <= 2^-5 needs ex - sq <= -5, or -4 when m is exactly 0.5. */
PLK_K1_FN int plk_k1_squarings(double norm)
{
    if (norm <= 0.03125) return 0;
    if (!(norm <= 1.7976931348623157e308)) return PLK_K1_MAX_SQ;      /* inf (a NaN norm compares false above) */
    int ex;
    const double m = frexp(norm, &ex);
    const int sq = ex + 5 - (m == 0.5 ? 1 : 0);
    return sq > PLK_K1_MAX_SQ ? PLK_K1_MAX_SQ : sq;
}

static inline int plk_k1_isfinite(double v) { return v - v == 0.0; }      /* false for inf and NaN */

/* every entry of a k x k direction matrix (hi and, unless NULL, lo) finite?  0 when so, else 1 + the index of the first bad entry */
static inline long plk_k1_check_matrix(int k, const double *hi, const double *lo)
{
    const long kk = (long)k * k;
    for (long i = 0; i < kk; i++)
        if (!plk_k1_isfinite(hi[i]) || (lo && !plk_k1_isfinite(lo[i]))) return 1 + i;
    return 0;
}

/*
 * 0 when K1 accepts the model, else nonzero with one line in err (no newline; err may be NULL):
 *   any value not finite (Qn, Qn_lo unless NULL, edge rates, category rates and priors, root_w when root_mode reads it:
 *   2 custom, 4 equilibrium); a negative edge rate, category rate or category prior (-0.0 is zero); any pair (c, e) with
 *   r_c t_e |Qn|_inf not finite or above 2^40.  |Qn|_inf is the largest absolute row sum of the high words.
 */
static inline int plk_k1_check_values(int k, int C, int E, const double *Qn, const double *Qn_lo, const double *edge_rates,
                                      const double *cat_rates, const double *cat_prior, int root_mode, const double *root_w,
                                      char *err, size_t errlen)
{
#define PLK_K1_FAIL(...) do { if (err && errlen) snprintf(err, errlen, __VA_ARGS__); return 1; } while (0)
    if (k < 1 || C < 1 || E < 0 || !Qn || (E > 0 && !edge_rates) || !cat_rates || !cat_prior) PLK_K1_FAIL("model values: bad arguments");
    double qnorm = 0;
    for (int i = 0; i < k; i++) {
        double row = 0;
        for (int j = 0; j < k; j++) {
            const size_t ij = (size_t)i * k + j;
            if (!plk_k1_isfinite(Qn[ij]) || (Qn_lo && !plk_k1_isfinite(Qn_lo[ij])))
                PLK_K1_FAIL("the normalised rate matrix is not finite at entry (%d, %d)", i, j);
            row += fabs(Qn[ij]);
        }
        if (row > qnorm) qnorm = row;
    }
    if (!plk_k1_isfinite(qnorm)) PLK_K1_FAIL("the row sums of the normalised rate matrix are not finite");
    for (int c = 0; c < C; c++) {
        if (!plk_k1_isfinite(cat_rates[c]) || cat_rates[c] < 0) PLK_K1_FAIL("the rate of rate category %d is %g: it must be finite and not negative", c, cat_rates[c]);
        if (!plk_k1_isfinite(cat_prior[c]) || cat_prior[c] < 0) PLK_K1_FAIL("the prior of rate category %d is %g: it must be finite and not negative", c, cat_prior[c]);
    }
    if ((root_mode == 2 || root_mode == 4) && root_w)
        for (int i = 0; i < k; i++)
            if (!plk_k1_isfinite(root_w[i])) PLK_K1_FAIL("the root prior of state %d is not finite", i);
    for (int e = 0; e < E; e++)
        if (!plk_k1_isfinite(edge_rates[e]) || edge_rates[e] < 0) PLK_K1_FAIL("the rate of edge %d is %g: it must be finite and not negative", e, edge_rates[e]);
    for (int c = 0; c < C; c++)
        for (int e = 0; e < E; e++) {
            const double v = cat_rates[c] * edge_rates[e] * qnorm;
            if (!plk_k1_isfinite(v) || v > PLK_K1_MAX_NORM)
                PLK_K1_FAIL("edge %d (rate %g) under rate category %d (rate %g): rate x length x |Qn| = %g is beyond 2^40, "
                            "the limit of the transition matrix kernel", e, edge_rates[e], c, cat_rates[c], v);
        }
    return 0;
#undef PLK_K1_FAIL
}

#endif
