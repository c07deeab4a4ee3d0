/*
 * mixcheck_main.cpp -- plk_mix_term (phyly_amd/csrc/plk_mix.h), the branch-free mixing of a category's term into a site's scaled
 * sum, against a verbatim copy of the three-way form the streamed k = 4 kernel held before it, on the uint64 view of the sum.
 * Stand-alone host program (tests/test_k4_mix_host.py builds it with -fsanitize=address,undefined: the exponent arithmetic on
 * the sentinel must not overflow).
 *
 * Sequences of (term, exponent) per site: random ones, all categories zero, a zero term first / in the middle / last, ascending
 * and descending exponents, exponent gaps of +-2100 (beyond the range of ldexp), denormal terms.  After every term the state of
 * plk_mix_term must have the bits of the three-way form's state, and what is written between the phases (the sum and the
 * exponent, or the sentinel) and the final log likelihood must agree too.
 *
 * Three deliberately wrong variants run over the same sequences: the two ldexp swapped, `>=` for `>`, a sentinel treated as a
 * term.  The first and the third must differ from the reference somewhere.  The second cannot: with equal exponents both
 * distances are zero and either branch adds the same two operands in the same order, so `esc >= E` is the same function as
 * `esc > E` -- the program requires that it never differs and prints the count, so that a change of the form under which the
 * comparison starts to matter shows up here.
 *
 * Prints "ok <sequences> <terms> <differences of the three variants>" and exits 0, or says what differs and exits 1.
 */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "plk_mix.h"

static uint64_t bits(double x) { uint64_t u; std::memcpy(&u, &x, 8); return u; }

/* the kernel's form before plk_mix_term, verbatim (sum, Eexp, have of one site j) */
struct Ref {
    double sum = 0.0;
    int Eexp = 0;
    bool have = false;
    void add(double term, int esc)
    {
        if (term != 0.0) {
            if (!have) { sum = term; Eexp = esc; have = true; }
            else if (esc > Eexp) { sum = ldexp(sum, Eexp - esc) + term; Eexp = esc; }
            else sum += ldexp(term, esc - Eexp);
        }
    }
    int stored_exp() const { return have ? Eexp : PLK_V4S_NO_TERM; }
};

/* the wrong variants, written on plk_mix_term's text */
static void mix_swapped(double &sum, int &E, double term, int esc)
{
    const bool up = esc > E;
    const unsigned dist = up ? (unsigned)esc - (unsigned)E : (unsigned)E - (unsigned)esc;
    const int shift = -(int)(dist < PLK_MIX_MAX_SHIFT ? dist : PLK_MIX_MAX_SHIFT);
    const double moved = ldexp(up ? term : sum, shift);         /* the operand at the larger exponent is moved */
    const double added = up ? sum + moved : moved + term;
    const bool use = term != 0.0;
    sum = use ? added : sum;
    E = use ? (up ? esc : E) : E;
}

static void mix_ge(double &sum, int &E, double term, int esc)
{
    const bool up = esc >= E;
    const unsigned dist = up ? (unsigned)esc - (unsigned)E : (unsigned)E - (unsigned)esc;
    const int shift = -(int)(dist < PLK_MIX_MAX_SHIFT ? dist : PLK_MIX_MAX_SHIFT);
    const double moved = ldexp(up ? sum : term, shift);
    const double added = up ? moved + term : sum + moved;
    const bool use = term != 0.0;
    sum = use ? added : sum;
    E = use ? (up ? esc : E) : E;
}

static void mix_sentinel_is_term(double &sum, int &E, double term, int esc)
{
    /* "no term yet" read as an exponent of 0, as the state was initialised beside the flag */
    int e = E == PLK_V4S_NO_TERM ? 0 : E;
    plk_mix_term(sum, e, term, esc);
    E = term != 0.0 || E != PLK_V4S_NO_TERM ? e : E;
}

struct Term { double v; int e; };

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}
static double rnd_unit() { return (double)(rnd() >> 11) * 0x1p-53; }

static double final_ll(double sum, int E) { return E != PLK_V4S_NO_TERM ? log(sum) + (double)E * 0.6931471805599453094 : -INFINITY; }

typedef void (*MixFn)(double &, int &, double, int);

/* -> number of terms after which the state differs from the reference's (bits of the sum, the exponent as stored) */
static long run(const std::vector<Term> &seq, MixFn fn, bool report)
{
    Ref r;
    double sum = 0.0;
    int E = PLK_V4S_NO_TERM;
    long bad = 0;
    for (size_t i = 0; i < seq.size(); i++) {
        r.add(seq[i].v, seq[i].e);
        fn(sum, E, seq[i].v, seq[i].e);
        const bool same = E == r.stored_exp() && bits(sum) == bits(r.sum);
        if (!same) {
            bad++;
            if (report && bad == 1) {
                std::fprintf(stderr, "term %zu of %zu (%a, %d): sum %a exponent %d, the three-way form has %a and %d\n", i, seq.size(), seq[i].v,
                             seq[i].e, sum, E, r.sum, r.stored_exp());
            }
        }
    }
    const double a = final_ll(sum, E), b = r.have ? log(r.sum) + (double)r.Eexp * 0.6931471805599453094 : -INFINITY;
    if (bits(a) != bits(b)) {
        bad++;
        if (report) std::fprintf(stderr, "final log likelihood %a, the three-way form has %a\n", a, b);
    }
    return bad;
}

int main()
{
    std::vector<std::vector<Term>> seqs;
    /* random: up to 8 categories, terms over many binades, exponents like the kernel's (multiples of nothing in particular,
     * non-positive mostly), some terms zero */
    for (int n = 0; n < 20000; n++) {
        std::vector<Term> s(1 + rnd() % 8);
        for (Term &t : s) {
            t.v = rnd() % 7 == 0 ? 0.0 : ldexp(rnd_unit(), -(int)(rnd() % 200));
            t.e = -(int)(rnd() % 3000) + (int)(rnd() % 40);
        }
        seqs.push_back(s);
    }
    /* random with close exponents, so that both branches and ties occur often */
    for (int n = 0; n < 20000; n++) {
        std::vector<Term> s(2 + rnd() % 7);
        const int base = -(int)(rnd() % 5000);
        for (Term &t : s) { t.v = rnd() % 9 == 0 ? 0.0 : rnd_unit() + 0x1p-60; t.e = base + (int)(rnd() % 5) - 2; }
        seqs.push_back(s);
    }
    const double x = 0.3125, y = 0.7109375;
    /* all categories zero: the site has likelihood zero (both signs of zero) */
    seqs.push_back({{0.0, 0}, {0.0, -12}, {0.0, 5}, {0.0, -2000}});
    seqs.push_back({{-0.0, 0}, {0.0, 7}});
    seqs.push_back({{0.0, INT_MIN}, {0.0, INT_MAX}});
    /* a zero term first, in the middle, last */
    seqs.push_back({{0.0, -3}, {x, -700}, {y, -698}, {x, -702}});
    seqs.push_back({{x, -700}, {0.0, 40}, {y, -698}, {x, -702}});
    seqs.push_back({{x, -700}, {y, -698}, {x, -702}, {0.0, 123456}});
    seqs.push_back({{0.0, 1000}, {0.0, -1000}, {y, -5}});
    /* ascending and descending exponents, ties */
    seqs.push_back({{x, -40}, {y, -30}, {x, -20}, {y, -10}, {x, 0}, {y, 10}});
    seqs.push_back({{x, 10}, {y, 0}, {x, -10}, {y, -20}, {x, -30}, {y, -40}});
    seqs.push_back({{x, -17}, {y, -17}, {x, -17}, {y, -17}});
    seqs.push_back({{x, 0}, {y, 0}});
    /* gaps beyond the range of ldexp, both ways, and at its edges */
    for (int gap : {2100, 2200, 2199, 2201, 2098, 2099, 1075, 1074, 1022, 1023, 4000, 1 << 20, 1 << 30}) {
        seqs.push_back({{x, 0}, {y, gap}, {x, 0}});
        seqs.push_back({{x, 0}, {y, -gap}, {x, 0}});
        seqs.push_back({{x, -gap}, {y, 0}, {x, -gap}, {y, gap / 2}});
        seqs.push_back({{0x1.fffffffffffffp+1023, 0}, {y, gap}, {0x1.fffffffffffffp+1023, 0}});
        seqs.push_back({{0x1p-1074, gap}, {0x1.fffffffffffffp+1023, 0}});
    }
    {
        /* distances that no int holds (the three-way form's own subtraction overflows on these, so the expected state is written
         * out): nothing here may trip the sanitizer */
        double s = 0.0;
        int E = PLK_V4S_NO_TERM;
        plk_mix_term(s, E, x, INT_MAX);
        plk_mix_term(s, E, y, INT_MIN + 1);
        plk_mix_term(s, E, x, INT_MAX);
        if (bits(s) != bits(2 * x) || E != INT_MAX) { std::fprintf(stderr, "widest distance downwards: %a %d\n", s, E); return 1; }
        s = 0.0; E = PLK_V4S_NO_TERM;
        plk_mix_term(s, E, x, INT_MIN + 1);
        plk_mix_term(s, E, y, INT_MAX);
        plk_mix_term(s, E, 0.0, 0);
        if (bits(s) != bits(y) || E != INT_MAX) { std::fprintf(stderr, "widest distance upwards: %a %d\n", s, E); return 1; }
    }
    /* denormal terms, and terms whose shifted value becomes denormal or rounds to zero */
    seqs.push_back({{0x1p-1074, -5}, {0x1.8p-1070, -3}, {0x1p-1060, -9}});
    seqs.push_back({{0x1.23456789abcdep-1030, 0}, {0x1.fp-1040, 7}, {0x1.1p-1050, -7}});
    seqs.push_back({{x, 0}, {0x1.23456789abcdep-1022, -60}, {0x1.23456789abcdfp-1022, 52}});
    seqs.push_back({{0x1.fffffffffffffp-1, -1000}, {0x1.0000000000001p-1, 60}, {0x1p-1074, 1100}});
    for (int n = 0; n < 5000; n++) {
        std::vector<Term> s(2 + rnd() % 4);
        for (Term &t : s) { t.v = ldexp(rnd_unit(), -1022 - (int)(rnd() % 53)); t.e = (int)(rnd() % 120) - 60; }
        seqs.push_back(s);
    }

    long terms = 0, bad = 0, diff[3] = {0, 0, 0};
    const MixFn wrong[3] = {mix_swapped, mix_ge, mix_sentinel_is_term};
    for (const std::vector<Term> &s : seqs) {
        terms += (long)s.size();
        bad += run(s, plk_mix_term, bad == 0);
        for (int v = 0; v < 3; v++) diff[v] += run(s, wrong[v], false) != 0;
    }
    if (bad) { std::fprintf(stderr, "plk_mix_term differs from the three-way form after %ld terms\n", bad); return 1; }
    if (diff[0] == 0) { std::fprintf(stderr, "the variant with the two ldexp swapped was not told apart\n"); return 1; }
    if (diff[2] == 0) { std::fprintf(stderr, "the variant that takes the sentinel for a term was not told apart\n"); return 1; }
    if (diff[1] != 0) { std::fprintf(stderr, "`>=` for `>` differs in %ld sequences: at equal exponents the two branches are no longer the same sum\n", diff[1]); return 1; }
    std::printf("ok %zu %ld %ld %ld %ld\n", seqs.size(), terms, diff[0], diff[1], diff[2]);
    return 0;
}
