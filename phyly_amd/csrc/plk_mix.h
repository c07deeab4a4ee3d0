/*
 * plk_mix.h -- plk_mix_term: one category's term added to a site's scaled mixture sum, without a branch.
 * Host and device (k_ll_fused4_v4s, plk_fused4_v4s.h; tests/mixcheck_main.cpp compares it with the three-way form it
 * replaced, bit for bit).
 *
 * A site's mixture sum is kept as sum * 2^E.  E == PLK_V4S_NO_TERM says that no nonzero term has been added yet (sum is
 * then 0): the exponent carries the state, there is no flag beside it.  A term of exponent esc is added at the larger of
 * the two exponents; a term that is zero changes nothing.
 */
#ifndef PLK_MIX_H
#define PLK_MIX_H

#include <limits.h>
#include <math.h>

#define PLK_V4S_NO_TERM INT_MIN

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PLK_MIX_FN __host__ __device__ __forceinline__
#else
#define PLK_MIX_FN static inline
#endif

/* Beyond this distance ldexp gives a zero of its operand's sign for every finite operand (2^1024 * 2^-2200 is below half
 * the least denormal), so a larger distance is cut to it: the bits stay and no shift count leaves the range of int. */
#define PLK_MIX_MAX_SHIFT 2200u

/* sum, E: the state, updated.  The three-way form this replaces, with have == (E != PLK_V4S_NO_TERM):
 *     if (term != 0.0) {
 *         if (!have) { sum = term; E = esc; }
 *         else if (esc > E) { sum = ldexp(sum, E - esc) + term; E = esc; }
 *         else sum += ldexp(term, esc - E);
 *     }
 * The sentinel is the least int, so the first term is the case "esc > E" with a distance that is cut: ldexp(0, .) + term is
 * term.  The distance is formed in unsigned arithmetic (esc - E as int overflows on the sentinel); the operand order of the
 * addition is the three-way form's in either case. */
PLK_MIX_FN void plk_mix_term(double &sum, int &E, double term, int esc)
{
    const bool up = esc > E;
    const unsigned dist = up ? (unsigned)esc - (unsigned)E : (unsigned)E - (unsigned)esc;
    const int shift = -(int)(dist < PLK_MIX_MAX_SHIFT ? dist : PLK_MIX_MAX_SHIFT);
    const double moved = ldexp(up ? sum : term, shift);
    const double added = up ? moved + term : sum + moved;
    const bool use = term != 0.0;
    sum = use ? added : sum;
    E = use ? (up ? esc : E) : E;
}

#endif
