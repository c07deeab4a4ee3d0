/*
 * tests/k1_args_main.c -- AddressSanitizer / UBSan driver for phyly_amd/csrc/plk_k1_check.h (the host-only check of the
 * values K1 is given, and its squaring count), built and run by tests/test_k1_args_host.py on the CPU.
 *
 * usage: k1_args <file>     one case per line:  name k C E root_mode has_lo has_rw  then the numbers (C99 hexadecimal
 *                           floats, inf, nan): Qn[k*k], Qn_lo[k*k] if has_lo, edge_rates[E], cat_rates[C], cat_prior[C],
 *                           root_w[k] if has_rw.  Every array lives in a heap block of exactly its size.
 *                           Prints "name rc diagnostic" per case.
 *        k1_args            checks plk_k1_squarings against the loop it replaced; prints "ok <norms>"
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "plk_k1_check.h"

static double *read_doubles(FILE *f, size_t n)
{
    double *p = malloc((n ? n : 1) * sizeof(double));
    if (!p) exit(3);
    for (size_t i = 0; i < n; i++) {
        char tok[64];
        if (fscanf(f, "%63s", tok) != 1) { fprintf(stderr, "short case\n"); exit(3); }
        p[i] = strtod(tok, NULL);
    }
    return p;
}

static int old_loop(double norm)
{
    int sq = 0;
    while (norm > 0.03125) { norm *= 0.5; sq++; }
    return sq;
}

static int squarings(void)
{
    long n = 0;
    unsigned long long state = 88172645463325252ULL;
    /* every power of two of the double range with its neighbours, and random mantissas at every exponent */
    for (int ex = -1074; ex <= 1023; ex++) {
        const double p = ldexp(1.0, ex);
        double v[6] = {p, nextafter(p, 0.0), nextafter(p, INFINITY), 0, 0, 0};
        for (int r = 3; r < 6; r++) {
            state ^= state << 13; state ^= state >> 7; state ^= state << 17;
            v[r] = ldexp(1.0 + (double)(state >> 11) * 0x1p-53, ex);
        }
        for (int r = 0; r < 6; r++, n++)
            if (plk_k1_squarings(v[r]) != old_loop(v[r])) { printf("squarings differ at %a: %d, loop %d\n", v[r], plk_k1_squarings(v[r]), old_loop(v[r])); return 1; }
    }
    const double maxd = 1.7976931348623157e308;
    if (plk_k1_squarings(0.0) != 0 || plk_k1_squarings(-0.0) != 0 || plk_k1_squarings(0.03125) != 0) return 1;
    if (plk_k1_squarings(maxd) != 1029 || plk_k1_squarings(maxd) >= PLK_K1_MAX_SQ) return 1;
    if (plk_k1_squarings(INFINITY) != PLK_K1_MAX_SQ) return 1;
    if (plk_k1_squarings(PLK_K1_MAX_NORM) != 45) return 1;          /* the limit of the check is the sq <= 45 of its derivation */
    (void)plk_k1_squarings(NAN);                                     /* any count: bounded */
    if (plk_k1_squarings(NAN) < 0 || plk_k1_squarings(NAN) > PLK_K1_MAX_SQ) return 1;
    printf("ok %ld\n", n);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) return squarings();
    FILE *f = fopen(argv[1], "r");
    if (!f) return 3;
    char name[128];
    int k, C, E, root_mode, has_lo, has_rw;
    while (fscanf(f, "%127s %d %d %d %d %d %d", name, &k, &C, &E, &root_mode, &has_lo, &has_rw) == 7) {
        const size_t kk = (size_t)k * k;
        double *Qn = read_doubles(f, kk), *lo = has_lo ? read_doubles(f, kk) : NULL;
        double *er = read_doubles(f, (size_t)E), *cr = read_doubles(f, (size_t)C), *cp = read_doubles(f, (size_t)C);
        double *rw = has_rw ? read_doubles(f, (size_t)k) : NULL;
        char msg[320] = "";
        const int rc = plk_k1_check_values(k, C, E, Qn, lo, er, cr, cp, root_mode, rw, msg, sizeof msg);
        char tiny[8];                                                /* a short buffer is never overrun */
        const int rc2 = plk_k1_check_values(k, C, E, Qn, lo, er, cr, cp, root_mode, rw, tiny, sizeof tiny);
        const int rc3 = plk_k1_check_values(k, C, E, Qn, lo, er, cr, cp, root_mode, rw, NULL, 0);
        if (rc2 != rc || rc3 != rc || strlen(tiny) >= sizeof tiny) { printf("%s inconsistent\n", name); return 1; }
        if (plk_k1_check_matrix(k, Qn, lo) != 0 && rc == 0) { printf("%s matrix check disagrees\n", name); return 1; }
        printf("%s %d %s\n", name, rc, msg);
        free(Qn); free(lo); free(er); free(cr); free(cp); free(rw);
    }
    fclose(f);
    return 0;
}
