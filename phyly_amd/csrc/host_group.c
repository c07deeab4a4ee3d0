/*
 * host_group.c -- several GPUs in one process: plk_group_* of include/plk.h (host C over plk_engine handles).
 *
 * Replaces nothing in the reference one for one: its site loops are sequential (src/arbplfll.c:139-170,
 * src/arbplfderiv.c:329-356, src/arbplfmarginal.c:237-256) and meet only in nd_accum_accumulate
 * (src/ndaccum.c:198-254).  Here the loop is cut into contiguous site blocks, one engine (GPU) per block, one host
 * thread per engine while a query runs; per-site results land at their global positions, aggregated results are the
 * engines' {hi, lo} partial sums added in engine order in long double (deterministic, no atomics, no collective).
 * No HIP in this file: it is exercised on the CPU with the stand-in engine of tests/sanitize_host.c.
 */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "plk.h"

#define GROUP_MAX 64

struct plk_group {
    int G;
    plk_engine *eng[GROUP_MAX];
    int device[GROUP_MAX];
    int N, E, k;
    long S, s0[GROUP_MAX + 1];       /* block of engine i: [s0[i], s0[i+1]) */
    int have_patterns;
    char err[512];
};

static int fail(plk_group *g, int rc, const char *msg)
{
    snprintf(g->err, sizeof g->err, "%s", msg);
    return rc;
}

int plk_group_create(plk_group **out, int ndev, const int *devices)
{
    if (!out) return PLK_E_ARG;
    *out = NULL;
    if (ndev < 1 || ndev > GROUP_MAX || !devices) return PLK_E_ARG;
    plk_group *g = calloc(1, sizeof(*g));
    if (!g) return PLK_E_NOMEM;
    g->G = ndev;
    for (int i = 0; i < ndev; i++) {
        g->device[i] = devices[i];
        int rc = plk_create(&g->eng[i], devices[i]);
        if (rc) {
            for (int j = 0; j < i; j++) plk_destroy(g->eng[j]);
            free(g);
            return rc;               /* plk_create_error() has the text */
        }
    }
    *out = g;
    return PLK_OK;
}

void plk_group_destroy(plk_group *g)
{
    if (!g) return;
    for (int i = 0; i < g->G; i++) plk_destroy(g->eng[i]);
    free(g);
}

const char *plk_group_last_error(const plk_group *g) { return g ? g->err : "null group"; }
int plk_group_size(const plk_group *g) { return g ? g->G : 0; }
plk_engine *plk_group_engine(plk_group *g, int i) { return g && i >= 0 && i < g->G ? g->eng[i] : NULL; }

int plk_group_block(const plk_group *g, int i, long *s0, long *s1)
{
    if (!g || i < 0 || i >= g->G || !g->have_patterns) return PLK_E_ARG;
    if (s0) *s0 = g->s0[i];
    if (s1) *s1 = g->s0[i + 1];
    return PLK_OK;
}

/* ---- one host thread per engine ------------------------------------------------------------------------- */
typedef int (*job_fn)(plk_group *g, int i, void *ctx);
typedef struct { plk_group *g; int i; job_fn fn; void *ctx; int rc; } job;

static void *job_main(void *p)
{
    job *j = p;
    j->rc = j->fn(j->g, j->i, j->ctx);
    return NULL;
}

/* runs fn for every engine (skip_empty: only engines whose block is not empty); first failure wins */
static int for_each(plk_group *g, job_fn fn, void *ctx, int skip_empty)
{
    job jobs[GROUP_MAX];
    pthread_t th[GROUP_MAX];
    int started[GROUP_MAX];
    int rc = PLK_OK;
    for (int i = 0; i < g->G; i++) {
        jobs[i].g = g; jobs[i].i = i; jobs[i].fn = fn; jobs[i].ctx = ctx; jobs[i].rc = PLK_OK;
        started[i] = 0;
    }
    for (int i = 1; i < g->G; i++) {
        if (skip_empty && g->s0[i + 1] == g->s0[i]) continue;
        if (pthread_create(&th[i], NULL, job_main, &jobs[i]) == 0) started[i] = 1;
        else job_main(&jobs[i]);     /* no thread: run it here */
    }
    if (!(skip_empty && g->s0[1] == g->s0[0])) job_main(&jobs[0]);
    for (int i = 1; i < g->G; i++) if (started[i]) pthread_join(th[i], NULL);
    for (int i = 0; i < g->G; i++)
        if (jobs[i].rc && !rc) {
            rc = jobs[i].rc;
            snprintf(g->err, sizeof g->err, "engine %d (device %d): %s", i, g->device[i], plk_last_error(g->eng[i]));
        }
    return rc;
}

/* ---- broadcast calls ------------------------------------------------------------------------------------ */
typedef struct { int N; const int *indptr, *indices, *preorder; } tree_ctx;
static int job_tree(plk_group *g, int i, void *p) { tree_ctx *c = p; return plk_set_tree(g->eng[i], c->N, c->indptr, c->indices, c->preorder); }

int plk_group_set_tree(plk_group *g, int N, const int *indptr, const int *indices, const int *preorder)
{
    if (!g) return PLK_E_ARG;
    tree_ctx c = {N, indptr, indices, preorder};
    g->have_patterns = 0;
    int rc = for_each(g, job_tree, &c, 0);
    if (!rc) { g->N = N; g->E = N - 1; g->k = 0; }
    return rc;
}

typedef struct { int k, C, root_mode; const double *Qn, *Qn_lo, *er, *cr, *cp, *rw; } model_ctx;
static int job_model(plk_group *g, int i, void *p)
{
    model_ctx *c = p;
    return plk_set_model(g->eng[i], c->k, c->C, c->Qn, c->Qn_lo, c->er, c->cr, c->cp, c->root_mode, c->rw);
}

int plk_group_set_model(plk_group *g, int k, int C, const double *Qn, const double *Qn_lo, const double *edge_rates_csr,
                        const double *cat_rates, const double *cat_prior, int root_mode, const double *root_w)
{
    if (!g) return PLK_E_ARG;
    model_ctx c = {k, C, root_mode, Qn, Qn_lo, edge_rates_csr, cat_rates, cat_prior, root_w};
    if (g->k != k) g->have_patterns = 0;
    int rc = for_each(g, job_model, &c, 0);
    if (!rc) g->k = k;
    return rc;
}

static int job_rates(plk_group *g, int i, void *p) { return plk_update_edge_rates(g->eng[i], p); }
int plk_group_update_edge_rates(plk_group *g, const double *edge_rates_csr)
{
    if (!g || !edge_rates_csr) return PLK_E_ARG;
    return for_each(g, job_rates, (void *)edge_rates_csr, 0);
}

/* ---- patterns: contiguous blocks of ceil(S / G) sites ----------------------------------------------------- */
static void set_blocks(plk_group *g, long S)
{
    const long per = (S + g->G - 1) / g->G;
    g->S = S;
    for (int i = 0; i <= g->G; i++) {
        long v = (long)i * per;
        g->s0[i] = v < S ? v : S;
    }
}

typedef struct { const uint8_t *codes; int nchar; const double *defs; const double *B; } pat_ctx;

static int job_codes(plk_group *g, int i, void *p)
{
    pat_ctx *c = p;
    const long a = g->s0[i], n = g->s0[i + 1] - a;
    if (g->G == 1) return plk_set_patterns_codes(g->eng[i], n, c->codes, PLK_HOST, c->nchar, c->defs);
    uint8_t *blk = malloc((size_t)g->N * (size_t)n);
    if (!blk) return PLK_E_NOMEM;
    for (int r = 0; r < g->N; r++) memcpy(blk + (size_t)r * n, c->codes + (size_t)r * g->S + a, (size_t)n);
    int rc = plk_set_patterns_codes(g->eng[i], n, blk, PLK_HOST, c->nchar, c->defs);
    free(blk);
    return rc;
}

int plk_group_set_patterns_codes(plk_group *g, long S, const uint8_t *codes, int nchar, const double *defs)
{
    if (!g) return PLK_E_ARG;
    if (S < 1 || !codes || !defs || g->k == 0) return fail(g, PLK_E_ARG, "plk_group_set_patterns_codes: bad arguments or call order");
    set_blocks(g, S);
    pat_ctx c = {codes, nchar, defs, NULL};
    int rc = for_each(g, job_codes, &c, 1);
    g->have_patterns = !rc;
    return rc;
}

static int job_dense(plk_group *g, int i, void *p)
{
    pat_ctx *c = p;
    const long a = g->s0[i], n = g->s0[i + 1] - a;
    if (g->G == 1) return plk_set_patterns_dense(g->eng[i], n, c->B, PLK_HOST);
    const size_t rows = (size_t)g->N * g->k;
    double *blk = malloc(rows * (size_t)n * sizeof(double));
    if (!blk) return PLK_E_NOMEM;
    for (size_t r = 0; r < rows; r++) memcpy(blk + r * (size_t)n, c->B + r * (size_t)g->S + a, (size_t)n * sizeof(double));
    int rc = plk_set_patterns_dense(g->eng[i], n, blk, PLK_HOST);
    free(blk);
    return rc;
}

int plk_group_set_patterns_dense(plk_group *g, long S, const double *B)
{
    if (!g) return PLK_E_ARG;
    if (S < 1 || !B || g->k == 0) return fail(g, PLK_E_ARG, "plk_group_set_patterns_dense: bad arguments or call order");
    set_blocks(g, S);
    pat_ctx c = {NULL, 0, NULL, B};
    int rc = for_each(g, job_dense, &c, 1);
    g->have_patterns = !rc;
    return rc;
}

static int job_weights(plk_group *g, int i, void *p)
{
    const double *w = p;
    return plk_set_site_weights(g->eng[i], w ? w + g->s0[i] : NULL, PLK_HOST);
}

int plk_group_set_site_weights(plk_group *g, const double *w)
{
    if (!g) return PLK_E_ARG;
    if (!g->have_patterns) return fail(g, PLK_E_ARG, "plk_group_set_site_weights: set the patterns first");
    return for_each(g, job_weights, (void *)w, 1);
}

/* ---- queries -------------------------------------------------------------------------------------------- */
/* every engine writes its per-site rows at its global offset and its partial sums into its own slice of `part`;
 * the slices are then added in engine order */
typedef struct {
    int kind;                      /* 0 ll, 1 deriv, 2 marginal, 3 edge expectations, 4 hess, 5 gradient and / or Hessian */
    int want_grad, want_hess;      /* kind 5 */
    const int *mask;
    double *site_out;              /* global buffer or NULL */
    size_t site_row;               /* doubles per site in site_out */
    double *part;                  /* [G][nsum][2] or NULL */
    size_t nsum;
    int nL, coef_mode;
    const double *L_hi, *L_lo;
} q_ctx;

/* The engine's gradient-and-Hessian entry is bound weakly: the host-only test programs (tests/group_check.c,
 * tests/sanitize_host.c) link this file against stand-in engines that have the older entry points only; there the same
 * sums come from plk_deriv and plk_hess.  libarbplf_amd.so always has the entry, so the library never takes that branch. */
extern int plk_second_order(plk_engine *h, double *grad_sums_out, double *hess_sums_out) __attribute__((weak));

static int job_query(plk_group *g, int i, void *p)
{
    q_ctx *c = p;
    double *site = c->site_out ? c->site_out + (size_t)g->s0[i] * c->site_row : NULL;
    double *sums = c->part ? c->part + (size_t)i * c->nsum * 2 : NULL;
    switch (c->kind) {
    case 0: return plk_ll(g->eng[i], site, PLK_HOST, sums);
    case 1: return plk_deriv(g->eng[i], c->mask, site, sums);
    case 2: return plk_marginal(g->eng[i], c->mask, site, sums);
    case 3: return plk_edge_expect_multi(g->eng[i], c->nL, c->L_hi, c->L_lo, c->coef_mode, c->mask, site, sums);
    case 5: {                                     /* [E] gradient and / or [E][E] Hessian, in that order */
        double *gs = c->want_grad ? sums : NULL;
        double *hs = c->want_hess ? sums + (c->want_grad ? 2 * (size_t)g->E : 0) : NULL;
        if (plk_second_order) return plk_second_order(g->eng[i], gs, hs);
        int rc = gs ? plk_deriv(g->eng[i], NULL, NULL, gs) : 0;
        return rc || !hs ? rc : plk_hess(g->eng[i], hs);
    }
    default: return plk_hess(g->eng[i], sums);
    }
}

static int run_query(plk_group *g, q_ctx *c, double *sums_out)
{
    if (!g->have_patterns) return fail(g, PLK_E_ARG, "plk_group: tree, model and patterns must be set");
    if (sums_out && g->G == 1) {         /* one engine: its sums are the result, bit for bit */
        c->part = sums_out;
        return for_each(g, job_query, c, 1);
    }
    if (sums_out) {
        c->part = calloc((size_t)g->G * c->nsum * 2 + 2, sizeof(double));
        if (!c->part) return fail(g, PLK_E_NOMEM, "plk_group: out of host memory");
    }
    int rc = for_each(g, job_query, c, 1);
    if (!rc && sums_out) {
        for (size_t r = 0; r < c->nsum; r++) {
            long double acc = 0;
            for (int i = 0; i < g->G; i++) {
                if (g->s0[i + 1] == g->s0[i]) continue;
                acc += (long double)c->part[((size_t)i * c->nsum + r) * 2];
                acc += (long double)c->part[((size_t)i * c->nsum + r) * 2 + 1];
            }
            const double hi = (double)acc;
            sums_out[2 * r] = hi;
            sums_out[2 * r + 1] = (double)(acc - (long double)hi);
        }
    }
    if (sums_out) free(c->part);
    return rc;
}

int plk_group_ll(plk_group *g, double *site_ll_out, double *sum_out)
{
    if (!g) return PLK_E_ARG;
    q_ctx c = {0};
    c.kind = 0; c.site_out = site_ll_out; c.site_row = 1; c.nsum = 1;
    return run_query(g, &c, sum_out);
}

int plk_group_deriv(plk_group *g, const int *edge_mask, double *site_edge_out, double *edge_sums_out)
{
    if (!g) return PLK_E_ARG;
    q_ctx c = {0};
    c.kind = 1; c.mask = edge_mask; c.site_out = site_edge_out; c.site_row = (size_t)g->E; c.nsum = (size_t)g->E;
    return run_query(g, &c, edge_sums_out);
}

int plk_group_marginal(plk_group *g, const int *node_mask, double *site_out, double *sums_out)
{
    if (!g) return PLK_E_ARG;
    q_ctx c = {0};
    c.kind = 2; c.mask = node_mask; c.site_out = site_out; c.site_row = (size_t)g->N * g->k; c.nsum = (size_t)g->N * g->k;
    return run_query(g, &c, sums_out);
}

int plk_group_edge_expect_multi(plk_group *g, int nL, const double *L_hi, const double *L_lo, int coef_mode,
                                const int *edge_mask, double *site_out, double *sums_out)
{
    if (!g) return PLK_E_ARG;
    if (nL < 1) return fail(g, PLK_E_ARG, "plk_group_edge_expect_multi: bad direction count");
    q_ctx c = {0};
    c.kind = 3; c.mask = edge_mask; c.site_out = site_out; c.site_row = (size_t)nL * g->E; c.nsum = (size_t)nL * g->E;
    c.nL = nL; c.L_hi = L_hi; c.L_lo = L_lo; c.coef_mode = coef_mode;
    return run_query(g, &c, sums_out);
}

/* rate-category posteriors: two per-site outputs of different row widths, C + 1 sums.  Bound weakly for the same reason
 * as plk_second_order above: the stand-in engines of the host-only test programs do not have it. */
extern int plk_cat_posterior(plk_engine *h, double *post_out, double *rate_out, double *post_sums_out, double *rate_sum_out) __attribute__((weak));
extern int plk_get_info(plk_engine *h, int what, long *out) __attribute__((weak));

typedef struct { int C; double *post, *rate, *part; int want_post_sums, want_rate_sum; } cp_ctx;

static int job_cat_posterior(plk_group *g, int i, void *p)
{
    cp_ctx *c = p;
    double *sums = c->part ? c->part + (size_t)i * (c->C + 1) * 2 : NULL;
    return plk_cat_posterior(g->eng[i], c->post ? c->post + (size_t)g->s0[i] * c->C : NULL, c->rate ? c->rate + g->s0[i] : NULL,
                             c->want_post_sums ? sums : NULL, c->want_rate_sum ? sums + 2 * (size_t)c->C : NULL);
}

int plk_group_cat_posterior(plk_group *g, double *post_out, double *rate_out, double *post_sums_out, double *rate_sum_out)
{
    if (!g) return PLK_E_ARG;
    if (!plk_cat_posterior || !plk_get_info) return fail(g, PLK_E_UNSUPPORTED, "plk_group_cat_posterior: the engine has no plk_cat_posterior");
    if (!g->have_patterns) return fail(g, PLK_E_ARG, "plk_group: tree, model and patterns must be set");
    long C = 0;
    if (plk_get_info(g->eng[0], PLK_INFO_CATEGORIES, &C) || C < 1) return fail(g, PLK_E_ARG, "plk_group_cat_posterior: the model is not set");
    cp_ctx c = {(int)C, post_out, rate_out, NULL, post_sums_out != NULL, rate_sum_out != NULL};
    const int want_sums = c.want_post_sums || c.want_rate_sum;
    if (want_sums) {
        c.part = calloc((size_t)g->G * (C + 1) * 2 + 2, sizeof(double));
        if (!c.part) return fail(g, PLK_E_NOMEM, "plk_group: out of host memory");
    }
    int rc = for_each(g, job_cat_posterior, &c, 1);
    if (!rc && want_sums) {
        for (long r = 0; r <= C; r++) {
            double *dst = r < C ? (post_sums_out ? post_sums_out + 2 * r : NULL) : rate_sum_out;
            if (!dst) continue;
            if (g->G == 1) { dst[0] = c.part[2 * r]; dst[1] = c.part[2 * r + 1]; continue; }   /* one engine: its sums, bit for bit */
            long double acc = 0;
            for (int i = 0; i < g->G; i++) {
                if (g->s0[i + 1] == g->s0[i]) continue;
                acc += (long double)c.part[((size_t)i * (C + 1) + r) * 2];
                acc += (long double)c.part[((size_t)i * (C + 1) + r) * 2 + 1];
            }
            const double hi = (double)acc;
            dst[0] = hi;
            dst[1] = (double)(acc - (long double)hi);
        }
    }
    free(c.part);
    return rc;
}

/* edge pair sums and the gradient in the rate matrix: sums only.  Weak for the same reason as above. */
extern int plk_edge_pair_sums(plk_engine *h, const int *edge_mask, double *W_out, double *root_out) __attribute__((weak));
extern int plk_rate_matrix_sens(plk_engine *h, double *G_out, double *root_out) __attribute__((weak));

typedef struct { int sens; const int *mask; size_t n_main, n_root; int want_root; double *part; } ps_ctx;

static int job_pair_sums(plk_group *g, int i, void *p)
{
    ps_ctx *c = p;
    double *mainp = c->part + (size_t)i * (c->n_main + c->n_root) * 2;
    double *rootp = c->want_root ? mainp + 2 * c->n_main : NULL;
    if (g->s0[i + 1] == g->s0[i]) return PLK_OK;           /* an engine without sites adds nothing */
    return c->sens ? plk_rate_matrix_sens(g->eng[i], mainp, rootp) : plk_edge_pair_sums(g->eng[i], c->mask, mainp, rootp);
}

static int group_pair_sums(plk_group *g, int sens, const int *edge_mask, double *main_out, double *root_out)
{
    if (!g || !main_out) return PLK_E_ARG;
    if (!plk_edge_pair_sums || !plk_rate_matrix_sens || !plk_get_info) return fail(g, PLK_E_UNSUPPORTED, "plk_group: the engine has no plk_edge_pair_sums");
    if (!g->have_patterns) return fail(g, PLK_E_ARG, "plk_group: tree, model and patterns must be set");
    long C = 0;
    if (plk_get_info(g->eng[0], PLK_INFO_CATEGORIES, &C) || C < 1) return fail(g, PLK_E_ARG, "plk_group: the model is not set");
    const size_t kk = (size_t)g->k * g->k;
    ps_ctx c = {sens, edge_mask, sens ? kk : (size_t)C * g->E * kk, sens ? (size_t)g->k : (size_t)C * g->k, root_out != NULL, NULL};
    const size_t per = c.n_main + c.n_root;
    c.part = calloc((size_t)g->G * per * 2 + 2, sizeof(double));
    if (!c.part) return fail(g, PLK_E_NOMEM, "plk_group: out of host memory");
    int rc = for_each(g, job_pair_sums, &c, 1);
    if (!rc) {
        for (size_t r = 0; r < per; r++) {
            double *dst = r < c.n_main ? main_out + 2 * r : (root_out ? root_out + 2 * (r - c.n_main) : NULL);
            if (!dst) continue;
            if (g->G == 1) { dst[0] = c.part[2 * r]; dst[1] = c.part[2 * r + 1]; continue; }   /* one engine: its sums, bit for bit */
            long double acc = 0;
            for (int i = 0; i < g->G; i++) {
                if (g->s0[i + 1] == g->s0[i]) continue;
                acc += (long double)c.part[((size_t)i * per + r) * 2];
                acc += (long double)c.part[((size_t)i * per + r) * 2 + 1];
            }
            const double hi = (double)acc;
            dst[0] = hi;
            dst[1] = (double)(acc - (long double)hi);
        }
    }
    free(c.part);
    return rc;
}

int plk_group_edge_pair_sums(plk_group *g, const int *edge_mask, double *W_out, double *root_out)
{
    return group_pair_sums(g, 0, edge_mask, W_out, root_out);
}

int plk_group_rate_matrix_sens(plk_group *g, double *G_out, double *root_out)
{
    return group_pair_sums(g, 1, NULL, G_out, root_out);
}

/* gradient in the rate-mixture parameters: 2 C sums.  Weak for the same reason as above. */
extern int plk_mixture_sens(plk_engine *h, double *prior_out, double *rate_out) __attribute__((weak));

typedef struct { size_t C; double *part; } mix_ctx;

static int job_mixture_sens(plk_group *g, int i, void *p)
{
    mix_ctx *c = p;
    if (g->s0[i + 1] == g->s0[i]) return PLK_OK;           /* an engine without sites adds nothing */
    double *mine = c->part + (size_t)i * c->C * 4;
    return plk_mixture_sens(g->eng[i], mine, mine + 2 * c->C);
}

int plk_group_mixture_sens(plk_group *g, double *prior_out, double *rate_out)
{
    if (!g || !prior_out || !rate_out) return PLK_E_ARG;
    if (!plk_mixture_sens || !plk_get_info) return fail(g, PLK_E_UNSUPPORTED, "plk_group: the engine has no plk_mixture_sens");
    if (!g->have_patterns) return fail(g, PLK_E_ARG, "plk_group: tree, model and patterns must be set");
    long C = 0;
    if (plk_get_info(g->eng[0], PLK_INFO_CATEGORIES, &C) || C < 1) return fail(g, PLK_E_ARG, "plk_group: the model is not set");
    mix_ctx c = {(size_t)C, NULL};
    const size_t per = 2 * c.C;
    c.part = calloc((size_t)g->G * per * 2 + 2, sizeof(double));
    if (!c.part) return fail(g, PLK_E_NOMEM, "plk_group: out of host memory");
    int rc = for_each(g, job_mixture_sens, &c, 1);
    if (!rc) {
        for (size_t r = 0; r < per; r++) {
            double *dst = r < c.C ? prior_out + 2 * r : rate_out + 2 * (r - c.C);
            if (g->G == 1) { dst[0] = c.part[2 * r]; dst[1] = c.part[2 * r + 1]; continue; }   /* one engine: its sums, bit for bit */
            long double acc = 0;
            for (int i = 0; i < g->G; i++) {
                if (g->s0[i + 1] == g->s0[i]) continue;
                acc += (long double)c.part[((size_t)i * per + r) * 2];
                acc += (long double)c.part[((size_t)i * per + r) * 2 + 1];
            }
            const double hi = (double)acc;
            dst[0] = hi;
            dst[1] = (double)(acc - (long double)hi);
        }
    }
    free(c.part);
    return rc;
}

/* log likelihood of nearest-neighbour interchanges: per-site rows [swap][site] of the engines' blocks put side by side,
 * sums added in engine order as the pair sums are.  Weak for the same reason as above. */
extern int plk_nni_ll(plk_engine *h, int n_swaps, const int *swaps, double *site_out, double *sums_out) __attribute__((weak));

typedef struct { int n; const int *swaps; double *site, *part; int want_sums; } nni_ctx;

static int job_nni_ll(plk_group *g, int i, void *p)
{
    nni_ctx *c = p;
    const long s0 = g->s0[i], ni = g->s0[i + 1] - s0, S = g->S;
    if (ni == 0) return PLK_OK;                            /* an engine without sites adds nothing */
    double *mine = NULL;
    if (c->site && c->n > 0 && !(mine = malloc((size_t)c->n * ni * sizeof(double)))) return PLK_E_NOMEM;
    const int rc = plk_nni_ll(g->eng[i], c->n, c->swaps, mine, c->want_sums ? c->part + (size_t)i * c->n * 2 : NULL);
    if (!rc && mine)
        for (int r = 0; r < c->n; r++) memcpy(c->site + (size_t)r * S + s0, mine + (size_t)r * ni, (size_t)ni * sizeof(double));
    free(mine);
    return rc;
}

int plk_group_nni_ll(plk_group *g, int n_swaps, const int *swaps, double *site_out, double *sums_out)
{
    if (!g) return PLK_E_ARG;
    if (!plk_nni_ll) return fail(g, PLK_E_UNSUPPORTED, "plk_group: the engine has no plk_nni_ll");
    if (!g->have_patterns) return fail(g, PLK_E_ARG, "plk_group: tree, model and patterns must be set");
    if (n_swaps < 0) return fail(g, PLK_E_ARG, "plk_group_nni_ll: negative number of swaps");
    nni_ctx c = {n_swaps, swaps, site_out, NULL, sums_out != NULL};
    c.part = calloc((size_t)g->G * n_swaps * 2 + 2, sizeof(double));
    if (!c.part) return fail(g, PLK_E_NOMEM, "plk_group: out of host memory");
    int rc = for_each(g, job_nni_ll, &c, 1);
    if (!rc && sums_out) {
        for (int r = 0; r < n_swaps; r++) {
            double *dst = sums_out + 2 * (size_t)r;
            if (g->G == 1) { dst[0] = c.part[2 * r]; dst[1] = c.part[2 * r + 1]; continue; }   /* one engine: its sums, bit for bit */
            long double acc = 0;
            for (int i = 0; i < g->G; i++) {
                if (g->s0[i + 1] == g->s0[i]) continue;
                acc += (long double)c.part[((size_t)i * n_swaps + r) * 2];
                acc += (long double)c.part[((size_t)i * n_swaps + r) * 2 + 1];
            }
            const double hi = (double)acc;
            dst[0] = hi;
            dst[1] = (double)(acc - (long double)hi);
        }
    }
    free(c.part);
    return rc;
}

/* log likelihood of placements: every engine gets its site block of the query rows and returns rows [query][edge][site] of
 * its block; they are put side by side, the sums added in engine order as for the swaps.  Weak for the same reason. */
extern int plk_place_ll(plk_engine *h, int n_queries, const uint8_t *q_codes, const double *q_dense, int n_edges, const int *edges,
                        double split, double pendant_rate, double *site_out, double *sums_out) __attribute__((weak));

typedef struct {
    int Q, ne; const uint8_t *codes; const double *dense; const int *edges; double split, pendant;
    double *site, *part; int want_sums;
} place_ctx;

static int job_place_ll(plk_group *g, int i, void *p)
{
    place_ctx *c = p;
    const long s0 = g->s0[i], ni = g->s0[i + 1] - s0, S = g->S;
    if (ni == 0) return PLK_OK;                            /* an engine without sites adds nothing */
    const size_t rows = (size_t)c->Q * c->ne, qrows = c->codes ? (size_t)c->Q : (size_t)c->Q * g->k;
    double *mine = NULL, *qd = NULL;
    uint8_t *qc = NULL;
    int rc = PLK_E_NOMEM;
    if (c->site && rows > 0 && !(mine = malloc(rows * ni * sizeof(double)))) goto done;
    if (g->G > 1 && c->codes) {
        if (!(qc = malloc(qrows * ni + 1))) goto done;
        for (size_t r = 0; r < qrows; r++) memcpy(qc + r * ni, c->codes + r * S + s0, (size_t)ni);
    } else if (g->G > 1) {
        if (!(qd = malloc((qrows * ni + 1) * sizeof(double)))) goto done;
        for (size_t r = 0; r < qrows; r++) memcpy(qd + r * ni, c->dense + r * S + s0, (size_t)ni * sizeof(double));
    }
    rc = plk_place_ll(g->eng[i], c->Q, g->G > 1 ? qc : c->codes, g->G > 1 ? qd : c->dense, c->ne, c->edges, c->split, c->pendant,
                      mine, c->want_sums ? c->part + (size_t)i * rows * 2 : NULL);
    if (!rc && mine)
        for (size_t r = 0; r < rows; r++) memcpy(c->site + r * S + s0, mine + r * ni, (size_t)ni * sizeof(double));
done:
    free(mine); free(qc); free(qd);
    return rc;
}

int plk_group_place_ll(plk_group *g, int n_queries, const uint8_t *q_codes, const double *q_dense, int n_edges, const int *edges,
                       double split, double pendant_rate, double *site_out, double *sums_out)
{
    if (!g) return PLK_E_ARG;
    if (!plk_place_ll) return fail(g, PLK_E_UNSUPPORTED, "plk_group: the engine has no plk_place_ll");
    if (!g->have_patterns) return fail(g, PLK_E_ARG, "plk_group: tree, model and patterns must be set");
    if (n_queries < 0 || n_edges < 0) return fail(g, PLK_E_ARG, "plk_group_place_ll: n_queries or n_edges is negative");
    if ((q_codes != NULL) == (q_dense != NULL)) return fail(g, PLK_E_ARG, "plk_group_place_ll: exactly one of q_codes and q_dense must be given");
    const size_t rows = (size_t)n_queries * n_edges;
    place_ctx c = {n_queries, n_edges, q_codes, q_dense, edges, split, pendant_rate, site_out, NULL, sums_out != NULL};
    c.part = calloc((size_t)g->G * rows * 2 + 2, sizeof(double));
    if (!c.part) return fail(g, PLK_E_NOMEM, "plk_group: out of host memory");
    int rc = for_each(g, job_place_ll, &c, 1);
    if (!rc && sums_out) {
        for (size_t r = 0; r < rows; r++) {
            double *dst = sums_out + 2 * r;
            if (g->G == 1) { dst[0] = c.part[2 * r]; dst[1] = c.part[2 * r + 1]; continue; }   /* one engine: its sums, bit for bit */
            long double acc = 0;
            for (int i = 0; i < g->G; i++) {
                if (g->s0[i + 1] == g->s0[i]) continue;
                acc += (long double)c.part[((size_t)i * rows + r) * 2];
                acc += (long double)c.part[((size_t)i * rows + r) * 2 + 1];
            }
            const double hi = (double)acc;
            dst[0] = hi;
            dst[1] = (double)(acc - (long double)hi);
        }
    }
    free(c.part);
    return rc;
}

/* log likelihood of prune-and-regraft moves: per-site rows [move][site] of the engines' blocks put side by side, sums added
 * in engine order as for the swaps.  Weak for the same reason. */
extern int plk_spr_ll(plk_engine *h, int n_moves, const int *moves, double split, double *site_out, double *sums_out) __attribute__((weak));

typedef struct { int n; const int *moves; double split; double *site, *part; int want_sums; } spr_ctx;

static int job_spr_ll(plk_group *g, int i, void *p)
{
    spr_ctx *c = p;
    const long s0 = g->s0[i], ni = g->s0[i + 1] - s0, S = g->S;
    if (ni == 0) return PLK_OK;                            /* an engine without sites adds nothing */
    double *mine = NULL;
    if (c->site && c->n > 0 && !(mine = malloc((size_t)c->n * ni * sizeof(double)))) return PLK_E_NOMEM;
    const int rc = plk_spr_ll(g->eng[i], c->n, c->moves, c->split, mine, c->want_sums ? c->part + (size_t)i * c->n * 2 : NULL);
    if (!rc && mine)
        for (int r = 0; r < c->n; r++) memcpy(c->site + (size_t)r * S + s0, mine + (size_t)r * ni, (size_t)ni * sizeof(double));
    free(mine);
    return rc;
}

int plk_group_spr_ll(plk_group *g, int n_moves, const int *moves, double split, double *site_out, double *sums_out)
{
    if (!g) return PLK_E_ARG;
    if (!plk_spr_ll) return fail(g, PLK_E_UNSUPPORTED, "plk_group: the engine has no plk_spr_ll");
    if (!g->have_patterns) return fail(g, PLK_E_ARG, "plk_group: tree, model and patterns must be set");
    if (n_moves < 0) return fail(g, PLK_E_ARG, "plk_group_spr_ll: negative number of moves");
    spr_ctx c = {n_moves, moves, split, site_out, NULL, sums_out != NULL};
    c.part = calloc((size_t)g->G * n_moves * 2 + 2, sizeof(double));
    if (!c.part) return fail(g, PLK_E_NOMEM, "plk_group: out of host memory");
    int rc = for_each(g, job_spr_ll, &c, 1);
    if (!rc && sums_out) {
        for (int r = 0; r < n_moves; r++) {
            double *dst = sums_out + 2 * (size_t)r;
            if (g->G == 1) { dst[0] = c.part[2 * r]; dst[1] = c.part[2 * r + 1]; continue; }   /* one engine: its sums, bit for bit */
            long double acc = 0;
            for (int i = 0; i < g->G; i++) {
                if (g->s0[i + 1] == g->s0[i]) continue;
                acc += (long double)c.part[((size_t)i * n_moves + r) * 2];
                acc += (long double)c.part[((size_t)i * n_moves + r) * 2 + 1];
            }
            const double hi = (double)acc;
            dst[0] = hi;
            dst[1] = (double)(acc - (long double)hi);
        }
    }
    free(c.part);
    return rc;
}

int plk_group_hess(plk_group *g, double *hess_sums_out)
{
    if (!g || !hess_sums_out) return PLK_E_ARG;
    q_ctx c = {0};
    c.kind = 4; c.nsum = (size_t)g->E * g->E;
    return run_query(g, &c, hess_sums_out);
}

/* gradient and Hessian sums of the engines added as one vector of E and / or E*E double-double entries: only what is
 * asked for is computed, allocated and reduced */
int plk_group_second_order(plk_group *g, double *grad_sums_out, double *hess_sums_out)
{
    if (!g || (!grad_sums_out && !hess_sums_out)) return PLK_E_ARG;
    const size_t E = (size_t)g->E, ng = grad_sums_out ? E : 0, nh = hess_sums_out ? E * E : 0;
    q_ctx c = {0};
    c.kind = 5; c.nsum = ng + nh; c.want_grad = grad_sums_out != NULL; c.want_hess = hess_sums_out != NULL;
    if (!grad_sums_out) return run_query(g, &c, hess_sums_out);
    if (!hess_sums_out) return run_query(g, &c, grad_sums_out);
    double *both = calloc(2 * c.nsum + 2, sizeof(double));
    if (!both) return fail(g, PLK_E_NOMEM, "plk_group: out of host memory");
    const int rc = run_query(g, &c, both);
    if (!rc) { memcpy(grad_sums_out, both, 2 * ng * sizeof(double)); memcpy(hess_sums_out, both + 2 * ng, 2 * nh * sizeof(double)); }
    free(both);
    return rc;
}
