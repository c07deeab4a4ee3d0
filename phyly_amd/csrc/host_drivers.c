/*
 * host_drivers.c -- the three query drivers behind include/arbplf.h (host C).
 *
 * Each driver follows the reference's _parse -> _query -> table sequence
 * (src/arbplfll.c:250-323, src/arbplfderiv.c:445-531, src/arbplfmarginal.c:348-446)
 * with the precision-doubling loop and the per-site Arb evaluation replaced by
 * one pass of the GPU engine (include/plk.h).  Selection / aggregation
 * semantics are those of src/reduction.c:25-118 and src/ndaccum.c:198-437:
 * only selected sites are uploaded and evaluated, aggregated site axes are
 * reduced on the device (double-double), other axes on the host (long double).
 */
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "arbplf.h"
#include "plk.h"
#include "host_json.h"
#include "host_k0.h"
#include "host_model.h"
#include "plk_k1_check.h"

static pthread_mutex_t g_mu = PTHREAD_MUTEX_INITIALIZER;
static plk_group *g_grp = NULL;
static char g_grp_spec[256];

/* The engines of this process: one per entry of ARBPLF_DEVICES (comma separated device ids; a device may be listed
 * twice), else the single device ARBPLF_DEVICE, else device 0.  The site patterns of a query are cut into one
 * contiguous block per engine (plk_group_*, host_group.c).  The group is cached across queries and rebuilt when the
 * environment names another device list. */
static plk_group *get_group(void)
{
    const char *list = getenv("ARBPLF_DEVICES"), *one = getenv("ARBPLF_DEVICE");
    const char *spec = list && *list ? list : (one && *one ? one : "0");
    if (g_grp && strncmp(spec, g_grp_spec, sizeof g_grp_spec)) { plk_group_destroy(g_grp); g_grp = NULL; }
    if (!g_grp) {
        int dev[64], n = 0;
        const char *p = spec;
        while (*p && n < 64) {
            char *end;
            long v = strtol(p, &end, 10);
            if (end == p || v < 0 || v > 1023) { fprintf(stderr, "error: ARBPLF_DEVICES: expected a comma separated list of device ids\n"); return NULL; }
            dev[n++] = (int)v;
            p = end;
            while (*p == ',' || *p == ' ') p++;
        }
        if (n == 0 || *p) { fprintf(stderr, "error: ARBPLF_DEVICES: expected 1 to 64 device ids\n"); return NULL; }
        if (plk_group_create(&g_grp, n, dev)) {
            fprintf(stderr, "error: %s\n", plk_create_error());
            g_grp = NULL;
            return NULL;
        }
        snprintf(g_grp_spec, sizeof g_grp_spec, "%s", spec);
    }
    return g_grp;
}

void arbplf_shutdown(void)
{
    pthread_mutex_lock(&g_mu);
    if (g_grp) { plk_group_destroy(g_grp); g_grp = NULL; }
    pthread_mutex_unlock(&g_mu);
}

/* ------------------------------------------------------------------ */
typedef struct {
    host_model m;
    host_reduction r_site, r_a, r_b;   /* site + up to two further axes */
    int *pair_first, *pair_second;     /* trans_reduction: state pairs parallel to r_b.selection */
    /* prepared model */
    int C;
    double *cat_rates, *cat_prior, *pi, *Qn, *Qn_lo;
    /* selected unique sites */
    long U;
    long *usites;      /* unique selected sites, ascending */
    long *site_to_u;   /* S entries, -1 when not selected */
    long double *w_site, div_site;  /* per-site aggregation weights (S) */
    plk_group *eng;    /* the engines of this query: one site block per device */
    /* further per-site bytes that tell patterns apart (the query columns of a placement): [S][xrow_bytes] or NULL */
    const unsigned char *xrows;
    size_t xrow_bytes;
} query;

static void query_init(query *q)
{
    memset(q, 0, sizeof(*q));
    host_model_init(&q->m);
    host_reduction_init(&q->r_site);
    host_reduction_init(&q->r_a);
    host_reduction_init(&q->r_b);
}

static void query_clear(query *q)
{
    host_model_clear(&q->m);
    host_reduction_clear(&q->r_site);
    host_reduction_clear(&q->r_a);
    host_reduction_clear(&q->r_b);
    free(q->cat_rates); free(q->cat_prior); free(q->pi); free(q->Qn); free(q->Qn_lo);
    free(q->usites); free(q->site_to_u); free(q->w_site);
    free(q->pair_first); free(q->pair_second);
}

#define ENG(q, call) do { if (call) { fprintf(stderr, "error: %s\n", plk_group_last_error((q)->eng)); return -1; } } while (0)

/* K0: the prepared model (host, long double) and the check of its values against what the transition matrix kernel
 * accepts (plk_k1_check.h), before any device work; returns 0 / -1 with one diagnostic line */
static int query_k0(query *q)
{
    host_model *m = &q->m;
    const int k = m->k;
    const int need_pi = (m->root_mode == HM_ROOT_EQUILIBRIUM) || m->use_equilibrium_divisor;
    q->C = arbplf_k0_category_count(&m->mix);
    q->cat_rates = malloc(q->C * sizeof(double));
    q->cat_prior = malloc(q->C * sizeof(double));
    q->pi = calloc(k, sizeof(double));
    q->Qn = malloc((size_t)k * k * sizeof(double));
    q->Qn_lo = malloc((size_t)k * k * sizeof(double));
    if (!q->cat_rates || !q->cat_prior || !q->pi || !q->Qn || !q->Qn_lo) return -1;
    if (arbplf_k0_prepare(k, m->rate_matrix, m->use_equilibrium_divisor, m->rate_divisor, need_pi, &m->mix,
                          q->cat_rates, q->cat_prior, q->pi, q->Qn, q->Qn_lo) != q->C) {
        fprintf(stderr, "error: model preparation failed\n");
        return -1;
    }
    for (int i = 0; i < k * k; i++)
        if (!isfinite(q->Qn[i])) { fprintf(stderr, "error: the normalised rate matrix is not finite (zero rate divisor or singular equilibrium system)\n"); return -1; }
    char msg[320];
    const double *root_w = m->root_mode == HM_ROOT_CUSTOM ? m->root_custom : (m->root_mode == HM_ROOT_EQUILIBRIUM ? q->pi : NULL);
    /* the check numbers the edges as its array does: give it the rates in the order of the user's `edges`, so that this
     * line names the edge as the document does.  A later refusal by the engine (the rates of a fit or Newton step)
     * comes through ENG() in the engine's words, which say that they count in CSR order. */
    double *er_user = malloc((size_t)(m->E + 1) * sizeof(double));
    if (!er_user) return -1;
    for (int e = 0; e < m->E; e++) er_user[m->csr_to_user[e]] = m->edge_rates_csr[e];
    const int bad = plk_k1_check_values(k, q->C, m->E, q->Qn, q->Qn_lo, er_user, q->cat_rates, q->cat_prior, m->root_mode, root_w, msg, sizeof msg);
    free(er_user);
    if (bad) { fprintf(stderr, "error: %s\n", msg); return -1; }
    return 0;
}

/* K0 + engine set-up + upload of the selected sites; returns 0 / -1 */
static int query_prepare(query *q)
{
    host_model *m = &q->m;
    const int k = m->k, N = m->N;
    const long S = m->S;
    /* selected sites */
    q->site_to_u = malloc((size_t)(S + 1) * sizeof(long));
    q->usites = malloc((size_t)(S + 1) * sizeof(long));
    q->w_site = malloc((size_t)(S + 1) * sizeof(long double));
    if (!q->site_to_u || !q->usites || !q->w_site) return -1;
    for (long s = 0; s < S; s++) q->site_to_u[s] = -1;
    for (int i = 0; i < q->r_site.selection_len; i++) q->site_to_u[q->r_site.selection[i]] = 0;
    /* Pattern compression: selected sites with identical observation rows share one
     * evaluated pattern; usites[] holds one representative site per pattern, site_to_u[] maps every
     * selected site to its pattern.  Aggregation weights are summed per pattern further down.  This is
     * what users of the reference do by hand (the BEAST examples ship pre-compressed patterns + weights). */
    q->U = 0;
    {
        const size_t row_bytes = m->codes8 ? (size_t)N : (size_t)N * k * sizeof(double);
        const unsigned char *rows = m->codes8 ? (const unsigned char *)m->codes8 : (const unsigned char *)m->prob;
        long nsel = 0;
        for (long s = 0; s < S; s++) if (q->site_to_u[s] == 0) nsel++;
        size_t tsize = 16;
        while (tsize < (size_t)nsel * 2) tsize <<= 1;
        long *table = malloc(tsize * sizeof(long));
        if (!table) return -1;
        for (size_t i = 0; i < tsize; i++) table[i] = -1;
        for (long s = 0; s < S; s++) {
            if (q->site_to_u[s] != 0) continue;
            const unsigned char *row = rows + (size_t)s * row_bytes;
            unsigned long long hsh = 1469598103934665603ULL;          /* FNV-1a */
            for (size_t b = 0; b < row_bytes; b++) { hsh ^= row[b]; hsh *= 1099511628211ULL; }
            const unsigned char *xrow = q->xrows ? q->xrows + (size_t)s * q->xrow_bytes : NULL;
            for (size_t b = 0; xrow && b < q->xrow_bytes; b++) { hsh ^= xrow[b]; hsh *= 1099511628211ULL; }
            size_t pos = (size_t)hsh & (tsize - 1);
            long found = -1;
            while (table[pos] >= 0) {
                const long p = table[pos];
                if (!memcmp(rows + (size_t)q->usites[p] * row_bytes, row, row_bytes) &&
                    (!xrow || !memcmp(q->xrows + (size_t)q->usites[p] * q->xrow_bytes, xrow, q->xrow_bytes))) { found = p; break; }
                pos = (pos + 1) & (tsize - 1);
            }
            if (found < 0) { found = q->U; table[pos] = found; q->usites[q->U++] = s; }
            q->site_to_u[s] = found;
        }
        free(table);
    }
    q->div_site = 1;
    if (q->r_site.agg_mode != AGG_NONE) host_reduction_weights(&q->r_site, q->w_site, &q->div_site);
    if (q->U == 0) return 0;

    if (query_k0(q)) return -1;

    q->eng = get_group();
    if (!q->eng) return -1;
    ENG(q, plk_group_set_tree(q->eng, N, m->indptr, m->indices, m->preorder));
    const double *root_w = m->root_mode == HM_ROOT_CUSTOM ? m->root_custom : (m->root_mode == HM_ROOT_EQUILIBRIUM ? q->pi : NULL);
    ENG(q, plk_group_set_model(q->eng, k, q->C, q->Qn, q->Qn_lo, m->edge_rates_csr, q->cat_rates, q->cat_prior, m->root_mode, root_w));

    /* observations of the selected sites, device layout (site fastest) */
    const long U = q->U;
    if (m->codes8) {
        uint8_t *codes = malloc((size_t)N * U);
        if (!codes) return -1;
        for (long u = 0; u < U; u++) {
            const uint8_t *src = m->codes8 + (size_t)q->usites[u] * N;
            for (int a = 0; a < N; a++) codes[(size_t)a * U + u] = src[a];
        }
        int rc = plk_group_set_patterns_codes(q->eng, U, codes, m->nchar, m->defs);
        free(codes);
        ENG(q, rc);
    } else {
        double *B = malloc((size_t)N * k * U * sizeof(double));
        if (!B) return -1;
        for (long u = 0; u < U; u++) {
            const double *src = m->prob + (size_t)q->usites[u] * N * k;
            for (int a = 0; a < N; a++)
                for (int j = 0; j < k; j++) B[((size_t)a * k + j) * U + u] = src[(size_t)a * k + j];
        }
        int rc = plk_group_set_patterns_dense(q->eng, U, B);
        free(B);
        ENG(q, rc);
    }
    if (q->r_site.agg_mode != AGG_NONE) {
        double *w = malloc((size_t)U * sizeof(double));
        if (!w) return -1;
        long double *wp = calloc((size_t)U, sizeof(long double));
        if (!wp) { free(w); return -1; }
        for (long s = 0; s < S; s++) if (q->site_to_u[s] >= 0) wp[q->site_to_u[s]] += q->w_site[s];
        for (long u = 0; u < U; u++) w[u] = (double)wp[u];
        free(wp);
        int rc = plk_group_set_site_weights(q->eng, w);
        free(w);
        ENG(q, rc);
    }
    return 0;
}

static double clean(long double v)
{
    double d = (double)v;
    if (d == 0.0) d = 0.0; /* -0.0 -> 0.0 (src/util.c:44-48) */
    return d;
}

static void table_begin(jbuf *b, const char *const *names, const host_reduction *const *reds, int ndim)
{
    jbuf_puts(b, "{\"columns\": [");
    for (int i = 0; i < ndim; i++)
        if (reds[i]->agg_mode == AGG_NONE) { jbuf_puts(b, "\""); jbuf_puts(b, names[i]); jbuf_puts(b, "\", "); }
    jbuf_puts(b, "\"value\"], \"data\": [");
}

static int check_finite(double v, const char *what)
{
    if (isfinite(v)) return 0;
    fprintf(stderr, "error: %s is not finite (a selected site has likelihood zero, or the computation overflowed); "
                    "the reference does not terminate on such input\n", what);
    return -1;
}

/* _parse of the drivers: kind 0 ll, 1 deriv, 2 marginal, 3 dwell, 4 trans, 5 em-update, 6 the second-order family,
 * 7 cat-posterior, 8 site-rate, 9 rate-matrix-deriv, 10 mixture-deriv, 11 nni, 12 place, 13 spr (no counterpart in the reference: its reduction grammar, its table layout)
 * (src/arbplfll.c:250-288, src/arbplfderiv.c:445-493, src/arbplfmarginal.c:348-405,
 *  src/arbplfdwell.c:507-566, src/arbplftrans.c:553-614, src/arbplfem.c:505-545) */
static int query_parse(query *q, int kind, const jval *root)
{
    static const char *const req[] = {"model_and_data", NULL};
    static const char *const all_ll[] = {"model_and_data", "site_reduction", NULL};
    static const char *const all_deriv[] = {"model_and_data", "site_reduction", "edge_reduction", NULL};
    static const char *const all_marg[] = {"model_and_data", "site_reduction", "node_reduction", "state_reduction", NULL};
    static const char *const all_dwell[] = {"model_and_data", "site_reduction", "edge_reduction", "state_reduction", NULL};
    static const char *const all_trans[] = {"model_and_data", "site_reduction", "edge_reduction", "trans_reduction", NULL};
    static const char *const all_catpost[] = {"model_and_data", "site_reduction", "category_reduction", NULL};
    static const char *const all_nni[] = {"model_and_data", "site_reduction", "swaps", NULL};
    static const char *const all_place[] = {"model_and_data", "site_reduction", "placement", NULL};
    static const char *const all_spr[] = {"model_and_data", "site_reduction", "spr", NULL};
    const char *const *allowed = kind == 0 ? all_ll : kind == 1 ? all_deriv : kind == 2 ? all_marg :
                                 kind == 3 ? all_dwell : kind == 4 ? all_trans : kind == 7 ? all_catpost : kind == 11 ? all_nni : kind == 12 ? all_place : kind == 13 ? all_spr : all_ll;
    if (host_check_keys(root, req, allowed, "input")) return -1;
    if (host_model_parse(&q->m, j_get(root, "model_and_data"))) return -1;
    if (host_reduction_parse(&q->r_site, (int)q->m.S, "site", j_get(root, "site_reduction"))) return -1;
    if (kind == 1 && host_reduction_parse(&q->r_a, q->m.E, "edge", j_get(root, "edge_reduction"))) return -1;
    if (kind == 2 && host_reduction_parse(&q->r_a, q->m.N, "node", j_get(root, "node_reduction"))) return -1;
    if (kind == 2 && host_reduction_parse(&q->r_b, q->m.k, "state", j_get(root, "state_reduction"))) return -1;
    if ((kind == 3 || kind == 4) && host_reduction_parse(&q->r_a, q->m.E, "edge", j_get(root, "edge_reduction"))) return -1;
    if (kind == 3 && host_reduction_parse(&q->r_b, q->m.k, "state", j_get(root, "state_reduction"))) return -1;
    if (kind == 4 && host_pair_reduction_parse(&q->r_b, &q->pair_first, &q->pair_second, q->m.k, "trans",
                                               j_get(root, "trans_reduction"))) return -1;
    /* the category axis has the length the mixture gives it (Gamma categories first, the invariable one last) */
    if (kind == 7 && host_reduction_parse(&q->r_a, arbplf_k0_category_count(&q->m.mix), "category", j_get(root, "category_reduction"))) return -1;
    if ((kind == 6 || kind == 9 || kind == 10) && !j_get(root, "site_reduction")) { fprintf(stderr, "error: site_reduction is required\n"); return -1; }
    if ((kind == 5 || kind == 6 || kind == 9 || kind == 10) && q->r_site.agg_mode == AGG_NONE) { fprintf(stderr, "error: aggregation over sites is required\n"); return -1; }
    if (kind == 10 && q->m.mix.mode == K0_MIX_NONE) { fprintf(stderr, "error: the model has no rate mixture, there is nothing to differentiate\n"); return -1; }
    return 0;
}

/* ------------------------------------------------------------------ ll */
static int run_ll(const jval *root, jbuf *out)
{
    query q;
    int rc = -1;
    double *site_ll = NULL;
    query_init(&q);
    if (query_parse(&q, 0, root)) goto done;
    if (query_prepare(&q)) goto done;
    const char *names[] = {"site"};
    const host_reduction *reds[] = {&q.r_site};
    table_begin(out, names, reds, 1);
    if (q.r_site.agg_mode != AGG_NONE) {
        double sum[2] = {0, 0};
        if (q.U > 0 && plk_group_ll(q.eng, NULL, sum)) { fprintf(stderr, "error: %s\n", plk_group_last_error(q.eng)); goto done; }
        double v = clean(((long double)sum[0] + (long double)sum[1]) / q.div_site);
        if (check_finite(v, "the aggregated log likelihood")) goto done;
        jbuf_puts(out, "[");
        jbuf_real(out, v);
        jbuf_puts(out, "]");
    } else {
        site_ll = malloc((size_t)(q.U + 1) * sizeof(double));
        if (!site_ll) goto done;
        if (q.U > 0 && plk_group_ll(q.eng, site_ll, NULL)) { fprintf(stderr, "error: %s\n", plk_group_last_error(q.eng)); goto done; }
        for (int i = 0; i < q.r_site.selection_len; i++) {
            int s = q.r_site.selection[i];
            double v = clean(site_ll[q.site_to_u[s]]);
            if (check_finite(v, "a site log likelihood")) goto done;
            if (i) jbuf_puts(out, ", ");
            jbuf_puts(out, "["); jbuf_int(out, s); jbuf_puts(out, ", "); jbuf_real(out, v); jbuf_puts(out, "]");
        }
    }
    jbuf_puts(out, "]}");
    rc = 0;
done:
    free(site_ll);
    query_clear(&q);
    return rc;
}

/* ------------------------------------------------------------------ deriv */
static int run_deriv(const jval *root, jbuf *out)
{
    query q;
    int rc = -1;
    int *mask = NULL;
    double *vals = NULL, *sums = NULL;
    long double *w_edge = NULL;
    query_init(&q);
    if (query_parse(&q, 1, root)) goto done;
    if (query_prepare(&q)) goto done;
    const int E = q.m.E;
    const host_reduction *re = &q.r_a;
    mask = calloc(E + 1, sizeof(int));
    w_edge = malloc((size_t)(E + 1) * sizeof(long double));
    if (!mask || !w_edge) goto done;
    for (int i = 0; i < re->selection_len; i++) mask[q.m.edge_order[re->selection[i]]] = 1;
    long double div_edge = 1;
    if (re->agg_mode != AGG_NONE) host_reduction_weights(re, w_edge, &div_edge);
    const int site_agg = q.r_site.agg_mode != AGG_NONE, edge_agg = re->agg_mode != AGG_NONE;
    if (site_agg) {
        sums = calloc((size_t)E * 2 + 2, sizeof(double));
        if (!sums) goto done;
        if (q.U > 0 && re->selection_len > 0 && plk_group_deriv(q.eng, mask, NULL, sums)) { fprintf(stderr, "error: %s\n", plk_group_last_error(q.eng)); goto done; }
    } else {
        vals = calloc((size_t)q.U * E + 1, sizeof(double));
        if (!vals) goto done;
        if (q.U > 0 && re->selection_len > 0 && plk_group_deriv(q.eng, mask, vals, NULL)) { fprintf(stderr, "error: %s\n", plk_group_last_error(q.eng)); goto done; }
    }
    const char *names[] = {"site", "edge"};
    const host_reduction *reds[] = {&q.r_site, re};
    table_begin(out, names, reds, 2);
    int first = 1;
    const int nsite_rows = site_agg ? 1 : q.r_site.selection_len;
    for (int si = 0; si < nsite_rows; si++) {
        const int s = site_agg ? -1 : q.r_site.selection[si];
        const long u = site_agg ? -1 : q.site_to_u[s];
        const int nedge_rows = edge_agg ? 1 : re->selection_len;
        for (int ei = 0; ei < nedge_rows; ei++) {
            long double v = 0;
            if (edge_agg) {
                for (int ue = 0; ue < E; ue++) {
                    if (w_edge[ue] == 0) continue;
                    const int ce = q.m.edge_order[ue];
                    long double x = site_agg ? ((long double)sums[2 * ce] + (long double)sums[2 * ce + 1]) / q.div_site
                                             : (long double)vals[(size_t)u * E + ce];
                    v += x * w_edge[ue] / div_edge;
                }
            } else {
                const int ce = q.m.edge_order[re->selection[ei]];
                v = site_agg ? ((long double)sums[2 * ce] + (long double)sums[2 * ce + 1]) / q.div_site
                             : (long double)vals[(size_t)u * E + ce];
            }
            double d = clean(v);
            if (check_finite(d, "a log likelihood derivative")) goto done;
            if (!first) jbuf_puts(out, ", ");
            first = 0;
            jbuf_puts(out, "[");
            if (!site_agg) { jbuf_int(out, s); jbuf_puts(out, ", "); }
            if (!edge_agg) { jbuf_int(out, re->selection[ei]); jbuf_puts(out, ", "); }
            jbuf_real(out, d);
            jbuf_puts(out, "]");
        }
    }
    jbuf_puts(out, "]}");
    rc = 0;
done:
    free(mask); free(vals); free(sums); free(w_edge);
    query_clear(&q);
    return rc;
}

/* ------------------------------------------------------------------ marginal */
static int run_marginal(const jval *root, jbuf *out)
{
    query q;
    int rc = -1;
    int *mask = NULL;
    double *vals = NULL, *sums = NULL;
    long double *w_node = NULL, *w_state = NULL;
    query_init(&q);
    if (query_parse(&q, 2, root)) goto done;
    if (query_prepare(&q)) goto done;
    const int N = q.m.N, k = q.m.k;
    const host_reduction *rn = &q.r_a, *rs = &q.r_b;
    mask = calloc(N + 1, sizeof(int));
    w_node = malloc((size_t)(N + 1) * sizeof(long double));
    w_state = malloc((size_t)(k + 1) * sizeof(long double));
    if (!mask || !w_node || !w_state) goto done;
    for (int i = 0; i < rn->selection_len; i++) mask[rn->selection[i]] = 1;
    long double div_node = 1, div_state = 1;
    const int site_agg = q.r_site.agg_mode != AGG_NONE, node_agg = rn->agg_mode != AGG_NONE, state_agg = rs->agg_mode != AGG_NONE;
    if (node_agg) host_reduction_weights(rn, w_node, &div_node);
    if (state_agg) host_reduction_weights(rs, w_state, &div_state);
    const int need = q.U > 0 && rn->selection_len > 0 && rs->selection_len > 0;
    if (site_agg) {
        sums = calloc((size_t)N * k * 2 + 2, sizeof(double));
        if (!sums) goto done;
        if (need && plk_group_marginal(q.eng, mask, NULL, sums)) { fprintf(stderr, "error: %s\n", plk_group_last_error(q.eng)); goto done; }
    } else {
        vals = calloc((size_t)q.U * N * k + 1, sizeof(double));
        if (!vals) goto done;
        if (need && plk_group_marginal(q.eng, mask, vals, NULL)) { fprintf(stderr, "error: %s\n", plk_group_last_error(q.eng)); goto done; }
    }
    const char *names[] = {"site", "node", "state"};
    const host_reduction *reds[] = {&q.r_site, rn, rs};
    table_begin(out, names, reds, 3);
    int first = 1;
    const int nsite_rows = site_agg ? 1 : q.r_site.selection_len;
    const int nnode_rows = node_agg ? 1 : rn->selection_len;
    const int nstate_rows = state_agg ? 1 : rs->selection_len;
    for (int si = 0; si < nsite_rows; si++) {
        const int s = site_agg ? -1 : q.r_site.selection[si];
        const long u = site_agg ? -1 : q.site_to_u[s];
        for (int ni = 0; ni < nnode_rows; ni++)
            for (int ti = 0; ti < nstate_rows; ti++) {
                long double v = 0;
                const int a_lo = node_agg ? 0 : rn->selection[ni], a_hi = node_agg ? N : a_lo + 1;
                const int j_lo = state_agg ? 0 : rs->selection[ti], j_hi = state_agg ? k : j_lo + 1;
                for (int a = a_lo; a < a_hi; a++) {
                    const long double wa = node_agg ? w_node[a] / div_node : 1;
                    if (node_agg && w_node[a] == 0) continue;
                    for (int j = j_lo; j < j_hi; j++) {
                        if (state_agg && w_state[j] == 0) continue;
                        const long double wj = state_agg ? w_state[j] / div_state : 1;
                        const size_t cell = (size_t)a * k + j;
                        long double x = site_agg ? ((long double)sums[2 * cell] + (long double)sums[2 * cell + 1]) / q.div_site
                                                 : (long double)vals[(size_t)u * N * k + cell];
                        v += x * wa * wj;
                    }
                }
                double d = clean(v);
                if (check_finite(d, "a marginal probability")) goto done;
                if (!first) jbuf_puts(out, ", ");
                first = 0;
                jbuf_puts(out, "[");
                if (!site_agg) { jbuf_int(out, s); jbuf_puts(out, ", "); }
                if (!node_agg) { jbuf_int(out, rn->selection[ni]); jbuf_puts(out, ", "); }
                if (!state_agg) { jbuf_int(out, rs->selection[ti]); jbuf_puts(out, ", "); }
                jbuf_real(out, d);
                jbuf_puts(out, "]");
            }
    }
    jbuf_puts(out, "]}");
    rc = 0;
done:
    free(mask); free(vals); free(sums); free(w_node); free(w_state);
    query_clear(&q);
    return rc;
}

/* ------------------------------------------------------------------ dwell / trans */
/* split a long double into an unevaluated (hi, lo) pair of doubles */
static void split_ld(long double v, double *hi, double *lo)
{
    *hi = (double)v;
    *lo = isfinite(*hi) ? (double)(v - (long double)*hi) : 0.0;
}

/*
 * arbplf-dwell (kind 3, src/arbplfdwell.c:303-505) and arbplf-trans (kind 4, src/arbplftrans.c:346-551).
 * The third axis (states / state pairs) is either aggregated -- then its weights go into the one
 * direction matrix L ("linear algebra trick", src/arbplfdwell.c:159-204, src/arbplftrans.c:162-224) --
 * or listed, one engine pass per selected state / pair (src/arbplfdwell.c:117-157, src/arbplftrans.c:116-160).
 */
static int run_edge_expect(const jval *root, jbuf *out, int kind)
{
    query q;
    int rc = -1;
    int *mask = NULL;
    double *vals_all = NULL, *sums_all = NULL, *Lall_hi = NULL, *Lall_lo = NULL, *Lhi = NULL, *Llo = NULL;
    long double *w_edge = NULL, *w_third = NULL, *Lacc = NULL;
    int npass = 0;
    query_init(&q);
    if (query_parse(&q, kind, root)) goto done;
    if (query_prepare(&q)) goto done;
    const int E = q.m.E, k = q.m.k;
    const host_reduction *re = &q.r_a, *rt = &q.r_b;
    const int site_agg = q.r_site.agg_mode != AGG_NONE, edge_agg = re->agg_mode != AGG_NONE, third_agg = rt->agg_mode != AGG_NONE;
    const int coef = kind == 3 ? PLK_COEF_PRIOR : PLK_COEF_PRIOR_RATE_EDGE;
    mask = calloc(E + 1, sizeof(int));
    w_edge = malloc((size_t)(E + 1) * sizeof(long double));
    w_third = malloc((size_t)(rt->n + 1) * sizeof(long double));
    Lhi = calloc((size_t)k * k + 1, sizeof(double));
    Llo = calloc((size_t)k * k + 1, sizeof(double));
    Lacc = calloc((size_t)k * k + 1, sizeof(long double));
    if (!mask || !w_edge || !w_third || !Lhi || !Llo || !Lacc) goto done;
    for (int i = 0; i < re->selection_len; i++) mask[q.m.edge_order[re->selection[i]]] = 1;
    long double div_edge = 1, div_third = 1;
    if (edge_agg) host_reduction_weights(re, w_edge, &div_edge);
    if (third_agg) host_reduction_weights(rt, w_third, &div_third);
    npass = third_agg ? 1 : rt->selection_len;
    Lall_hi = calloc((size_t)npass * k * k + 1, sizeof(double));
    Lall_lo = calloc((size_t)npass * k * k + 1, sizeof(double));
    if (!Lall_hi || !Lall_lo) goto done;
    for (int t = 0; t < npass; t++) {
        /* direction matrix; for trans its entries are multiplied by the normalised rates
         * (src/arbplftrans.c:137-138, :196), hi/lo parts of Qn included */
        for (int i = 0; i < k * k; i++) Lacc[i] = 0;
        if (third_agg) {
            for (int x = 0; x < rt->n; x++) {
                if (w_third[x] == 0) continue;
                const int a = kind == 3 ? x : q.pair_first[x], b = kind == 3 ? x : q.pair_second[x];
                Lacc[a * k + b] += w_third[x];
            }
        } else {
            const int x = rt->selection[t];
            const int a = kind == 3 ? x : q.pair_first[x], b = kind == 3 ? x : q.pair_second[x];
            Lacc[a * k + b] = 1;
        }
        if (q.U > 0)
            for (int i = 0; i < k * k; i++) {
                long double v = Lacc[i];
                if (kind == 4) v *= (long double)q.Qn[i] + (long double)q.Qn_lo[i];
                v /= div_third;
                split_ld(v, &Lhi[i], &Llo[i]);
            }
        memcpy(Lall_hi + (size_t)t * k * k, Lhi, (size_t)k * k * sizeof(double));
        memcpy(Lall_lo + (size_t)t * k * k, Llo, (size_t)k * k * sizeof(double));
    }
    /* one engine call for all directions: the k = 4 kernels carry up to four of them per pass */
    if (site_agg) sums_all = calloc((size_t)npass * E * 2 + 2, sizeof(double));
    else vals_all = calloc((size_t)q.U * npass * E + 1, sizeof(double));
    if (!sums_all && !vals_all) goto done;
    if (q.U > 0 && re->selection_len > 0 && npass > 0 &&
        plk_group_edge_expect_multi(q.eng, npass, Lall_hi, Lall_lo, coef, mask, vals_all, sums_all)) {
        fprintf(stderr, "error: %s\n", plk_group_last_error(q.eng)); goto done;
    }
#define EXP_SUM(t, ce) (((long double)sums_all[((size_t)(t) * E + (ce)) * 2] + (long double)sums_all[((size_t)(t) * E + (ce)) * 2 + 1]) / q.div_site)
#define EXP_VAL(t, u, ce) ((long double)vals_all[((size_t)(u) * npass + (t)) * E + (ce)])
    /* table header; the trans axis prints its two component indices (src/ndaccum.c:355-366, :401-409) */
    jbuf_puts(out, "{\"columns\": [");
    if (!site_agg) jbuf_puts(out, "\"site\", ");
    if (!edge_agg) jbuf_puts(out, "\"edge\", ");
    if (!third_agg) jbuf_puts(out, kind == 3 ? "\"state\", " : "\"first_state\", \"second_state\", ");
    jbuf_puts(out, "\"value\"], \"data\": [");
    int first = 1;
    const int nsite_rows = site_agg ? 1 : q.r_site.selection_len;
    const int nedge_rows = edge_agg ? 1 : re->selection_len;
    for (int si = 0; si < nsite_rows; si++) {
        const int s = site_agg ? -1 : q.r_site.selection[si];
        const long u = site_agg ? -1 : q.site_to_u[s];
        for (int ei = 0; ei < nedge_rows; ei++) {
            for (int t = 0; t < npass; t++) {
                long double v = 0;
                if (edge_agg) {
                    for (int ue = 0; ue < E; ue++) {
                        if (w_edge[ue] == 0) continue;
                        const int ce = q.m.edge_order[ue];
                        long double x = site_agg ? EXP_SUM(t, ce) : EXP_VAL(t, u, ce);
                        v += x * w_edge[ue] / div_edge;
                    }
                } else {
                    const int ce = q.m.edge_order[re->selection[ei]];
                    v = site_agg ? EXP_SUM(t, ce) : EXP_VAL(t, u, ce);
                }
                double d = clean(v);
                if (check_finite(d, kind == 3 ? "a dwell expectation" : "a transition count expectation")) goto done;
                if (!first) jbuf_puts(out, ", ");
                first = 0;
                jbuf_puts(out, "[");
                if (!site_agg) { jbuf_int(out, s); jbuf_puts(out, ", "); }
                if (!edge_agg) { jbuf_int(out, re->selection[ei]); jbuf_puts(out, ", "); }
                if (!third_agg) {
                    const int x = rt->selection[t];
                    if (kind == 3) { jbuf_int(out, x); jbuf_puts(out, ", "); }
                    else { jbuf_int(out, q.pair_first[x]); jbuf_puts(out, ", "); jbuf_int(out, q.pair_second[x]); jbuf_puts(out, ", "); }
                }
                jbuf_real(out, d);
                jbuf_puts(out, "]");
            }
        }
    }
    jbuf_puts(out, "]}");
    rc = 0;
done:
#undef EXP_SUM
#undef EXP_VAL
    free(vals_all); free(sums_all); free(Lall_hi); free(Lall_lo);
    free(mask); free(w_edge); free(w_third); free(Lhi); free(Llo); free(Lacc);
    query_clear(&q);
    return rc;
}

static int run_dwell(const jval *root, jbuf *out) { return run_edge_expect(root, out, 3); }
static int run_trans(const jval *root, jbuf *out) { return run_edge_expect(root, out, 4); }

/* ------------------------------------------------------------------ em-update */
/* arbplf-em-update (src/arbplfem.c:397-503): edge_rate_e * E[transitions on e] / E[rate-weighted dwell on e],
 * both accumulated over the weighted sites; exactly 0 where the expected transition count is 0. */
static int run_em_update(const jval *root, jbuf *out)
{
    query q;
    int rc = -1;
    double *Lhi = NULL, *Llo = NULL, *dw = NULL, *tr = NULL, *both = NULL;
    query_init(&q);
    if (query_parse(&q, 5, root)) goto done;
    if (query_prepare(&q)) goto done;
    const int E = q.m.E, k = q.m.k;
    Lhi = calloc((size_t)k * k * 2 + 1, sizeof(double));
    Llo = calloc((size_t)k * k * 2 + 1, sizeof(double));
    dw = calloc((size_t)E * 2 + 2, sizeof(double));
    tr = calloc((size_t)E * 2 + 2, sizeof(double));
    if (!Lhi || !Llo || !dw || !tr) goto done;
    if (q.U > 0 && E > 0) {
        /* L_dwell: exit rates on the diagonal; L_trans: rates off the diagonal (src/arbplfem.c:118-129) */
        for (int i = 0; i < k; i++)
            for (int j = 0; j < k; j++) {
                Lhi[i * k + j] = i == j ? -q.Qn[i * k + j] : 0.0;
                Llo[i * k + j] = i == j ? -q.Qn_lo[i * k + j] : 0.0;
            }
        for (int i = 0; i < k; i++)
            for (int j = 0; j < k; j++) {
                Lhi[k * k + i * k + j] = i != j ? q.Qn[i * k + j] : 0.0;
                Llo[k * k + i * k + j] = i != j ? q.Qn_lo[i * k + j] : 0.0;
            }
        /* both expectations in one call: [2][E][2] sums (dwell first) */
        both = calloc((size_t)E * 4 + 4, sizeof(double));
        if (!both) goto done;
        if (plk_group_edge_expect_multi(q.eng, 2, Lhi, Llo, PLK_COEF_PRIOR_RATE, NULL, NULL, both)) { fprintf(stderr, "error: %s\n", plk_group_last_error(q.eng)); goto done; }
        memcpy(dw, both, (size_t)E * 2 * sizeof(double));
        memcpy(tr, both + (size_t)E * 2, (size_t)E * 2 * sizeof(double));
    }
    jbuf_puts(out, "{\"columns\": [\"edge\", \"value\"], \"data\": [");
    for (int ue = 0; ue < E; ue++) {
        const int ce = q.m.edge_order[ue];
        const long double t = (long double)tr[2 * ce] + (long double)tr[2 * ce + 1];
        const long double d = (long double)dw[2 * ce] + (long double)dw[2 * ce + 1];
        double v = 0.0;
        if (t != 0) v = clean(t / d * (long double)q.m.edge_rates_csr[ce]);
        if (check_finite(v, "an updated edge rate coefficient")) goto done;
        if (ue) jbuf_puts(out, ", ");
        jbuf_puts(out, "["); jbuf_int(out, ue); jbuf_puts(out, ", "); jbuf_real(out, v); jbuf_puts(out, "]");
    }
    jbuf_puts(out, "]}");
    rc = 0;
done:
    free(Lhi); free(Llo); free(dw); free(tr); free(both);
    query_clear(&q);
    return rc;
}

/* ------------------------------------------------------------------ hess */
/* arbplf-hess (src/arbplfhess.c:1163-1206 _parse_second_order, :1279-1343 hess_query): the E x E matrix of
 * second derivatives of the site-aggregated log likelihood, all user edges in order on both axes */
static int run_hess(const jval *root, jbuf *out)
{
    query q;
    int rc = -1;
    double *hs = NULL;
    query_init(&q);
    if (query_parse(&q, 6, root)) goto done;
    if (query_prepare(&q)) goto done;
    const int E = q.m.E;
    hs = calloc((size_t)E * E * 2 + 2, sizeof(double));
    if (!hs) goto done;
    if (q.U > 0 && E > 0 && plk_group_hess(q.eng, hs)) { fprintf(stderr, "error: %s\n", plk_group_last_error(q.eng)); goto done; }
    jbuf_puts(out, "{\"columns\": [\"first_edge\", \"second_edge\", \"value\"], \"data\": [");
    for (int a = 0; a < E; a++)
        for (int b = 0; b < E; b++) {
            const size_t pos = (size_t)q.m.edge_order[a] * E + q.m.edge_order[b];
            double v = clean(((long double)hs[2 * pos] + (long double)hs[2 * pos + 1]) / q.div_site);
            if (check_finite(v, "a second derivative of the log likelihood")) goto done;
            if (a || b) jbuf_puts(out, ", ");
            jbuf_puts(out, "["); jbuf_int(out, a); jbuf_puts(out, ", "); jbuf_int(out, b); jbuf_puts(out, ", ");
            jbuf_real(out, v); jbuf_puts(out, "]");
        }
    jbuf_puts(out, "]}");
    rc = 0;
done:
    free(hs);
    query_clear(&q);
    return rc;
}

/* arbplf-inv-hess, arbplf-newton-delta, arbplf-newton-update (src/arbplfhess.c:1238-1267 inv_hess_query, :1372-1388
 * newton_delta_query, :1427-1443 newton_point_query; parsing shared with hess): gradient and Hessian of the
 * site-aggregated log likelihood from one engine run, then the host solve.  mode 0: H^-1, E^2 rows; 1: delta = -H^-1 g;
 * 2: edge_rate_coefficients + delta, unclamped.  User edge order throughout. */
static int run_second_order_solve(const jval *root, jbuf *out, int mode)
{
    query q;
    int rc = -1;
    double *gs = NULL, *hs = NULL, *hu = NULL, *gu = NULL, *inv = NULL, *delta = NULL;
    query_init(&q);
    if (query_parse(&q, 6, root)) goto done;
    if (query_prepare(&q)) goto done;
    const int E = q.m.E;
    const size_t n = (size_t)E;
    gs = calloc(n * 2 + 2, sizeof(double)); hs = calloc(n * n * 2 + 2, sizeof(double));
    hu = calloc(n * n * 2 + 2, sizeof(double)); gu = calloc(n * 2 + 2, sizeof(double));
    inv = calloc(n * n + 1, sizeof(double)); delta = calloc(n + 1, sizeof(double));
    if (!gs || !hs || !hu || !gu || !inv || !delta) goto done;
    if (q.U > 0 && E > 0 && plk_group_second_order(q.eng, gs, hs)) { fprintf(stderr, "error: %s\n", plk_group_last_error(q.eng)); goto done; }
    for (int a = 0; a < E; a++) {
        const size_t ea = (size_t)q.m.edge_order[a];
        const long double g = ((long double)gs[2 * ea] + (long double)gs[2 * ea + 1]) / q.div_site;
        if (check_finite((double)g, "a derivative of the log likelihood")) goto done;
        split_ld(g, &gu[2 * a], &gu[2 * a + 1]);
        for (int b = 0; b < E; b++) {
            const size_t pos = ea * n + (size_t)q.m.edge_order[b];
            const long double v = ((long double)hs[2 * pos] + (long double)hs[2 * pos + 1]) / q.div_site;
            if (check_finite((double)v, "a second derivative of the log likelihood")) goto done;
            split_ld(v, &hu[2 * (a * n + b)], &hu[2 * (a * n + b) + 1]);
        }
    }
    if (E < 1 || plk_solve_second_order(E, hu, gu, inv, delta, NULL)) {
        fprintf(stderr, "error: Hessian is singular to working precision; the reference does not terminate on such input\n");
        goto done;
    }
    if (mode == 0) {
        jbuf_puts(out, "{\"columns\": [\"first_edge\", \"second_edge\", \"value\"], \"data\": [");
        for (int a = 0; a < E; a++)
            for (int b = 0; b < E; b++) {
                if (a || b) jbuf_puts(out, ", ");
                jbuf_puts(out, "["); jbuf_int(out, a); jbuf_puts(out, ", "); jbuf_int(out, b); jbuf_puts(out, ", ");
                jbuf_real(out, clean(inv[a * n + b])); jbuf_puts(out, "]");
            }
    } else {
        jbuf_puts(out, "{\"columns\": [\"edge\", \"value\"], \"data\": [");
        for (int a = 0; a < E; a++) {
            double v = delta[a];
            if (mode == 2) v += q.m.edge_rates_csr[q.m.edge_order[a]];
            if (a) jbuf_puts(out, ", ");
            jbuf_puts(out, "["); jbuf_int(out, a); jbuf_puts(out, ", "); jbuf_real(out, clean(v)); jbuf_puts(out, "]");
        }
    }
    jbuf_puts(out, "]}");
    rc = 0;
done:
    free(gs); free(hs); free(hu); free(gu); free(inv); free(delta);
    query_clear(&q);
    return rc;
}
static int run_inv_hess(const jval *root, jbuf *out) { return run_second_order_solve(root, out, 0); }
static int run_newton_delta(const jval *root, jbuf *out) { return run_second_order_solve(root, out, 1); }
static int run_newton_update(const jval *root, jbuf *out) { return run_second_order_solve(root, out, 2); }

/* ------------------------------------------------------------------ cat-posterior / site-rate */
/* a failed sums call of the engine because a weighted site has likelihood zero gets the drivers' usual diagnostic */
static int catpost_failed(const query *q, const char *what)
{
    const char *msg = plk_group_last_error(q->eng);
    if (strstr(msg, "site likelihood zero")) return check_finite(NAN, what);
    fprintf(stderr, "error: %s\n", msg);
    return -1;
}

/* arbplf-cat-posterior: posterior probability of every rate category at every site, axes site x category.  Site-aggregated
 * requests take the engine's device-side sums; the [sites][categories] plane comes to the host only for per-site rows. */
static int run_cat_posterior(const jval *root, jbuf *out)
{
    query q;
    int rc = -1;
    double *vals = NULL, *sums = NULL;
    long double *w_cat = NULL;
    query_init(&q);
    if (query_parse(&q, 7, root)) goto done;
    if (query_prepare(&q)) goto done;
    const host_reduction *rcat = &q.r_a;
    const int C = rcat->n;
    w_cat = malloc((size_t)(C + 1) * sizeof(long double));
    if (!w_cat) goto done;
    long double div_cat = 1;
    const int site_agg = q.r_site.agg_mode != AGG_NONE, cat_agg = rcat->agg_mode != AGG_NONE;
    if (cat_agg) host_reduction_weights(rcat, w_cat, &div_cat);
    const int need = q.U > 0 && rcat->selection_len > 0;
    if (need && q.C != C) { fprintf(stderr, "internal error: category count\n"); goto done; }
    if (site_agg) {
        sums = calloc((size_t)C * 2 + 2, sizeof(double));
        if (!sums) goto done;
        if (need && plk_group_cat_posterior(q.eng, NULL, NULL, sums, NULL)) { catpost_failed(&q, "a site-aggregated category posterior"); goto done; }
    } else {
        vals = calloc((size_t)q.U * C + 1, sizeof(double));
        if (!vals) goto done;
        if (need && plk_group_cat_posterior(q.eng, vals, NULL, NULL, NULL)) { catpost_failed(&q, "a category posterior"); goto done; }
    }
    const char *names[] = {"site", "category"};
    const host_reduction *reds[] = {&q.r_site, rcat};
    table_begin(out, names, reds, 2);
    int first = 1;
    const int nsite_rows = site_agg ? 1 : q.r_site.selection_len;
    const int ncat_rows = cat_agg ? 1 : rcat->selection_len;
    for (int si = 0; si < nsite_rows; si++) {
        const int s = site_agg ? -1 : q.r_site.selection[si];
        const long u = site_agg ? -1 : q.site_to_u[s];
        for (int ci = 0; ci < ncat_rows; ci++) {
            long double v = 0;
            const int c_lo = cat_agg ? 0 : rcat->selection[ci], c_hi = cat_agg ? C : c_lo + 1;
            for (int c = c_lo; c < c_hi; c++) {
                if (cat_agg && w_cat[c] == 0) continue;
                const long double wc = cat_agg ? w_cat[c] / div_cat : 1;
                const long double x = site_agg ? ((long double)sums[2 * c] + (long double)sums[2 * c + 1]) / q.div_site
                                               : (long double)vals[(size_t)u * C + c];
                v += x * wc;
            }
            double d = clean(v);
            if (check_finite(d, "a category posterior")) goto done;
            if (!first) jbuf_puts(out, ", ");
            first = 0;
            jbuf_puts(out, "[");
            if (!site_agg) { jbuf_int(out, s); jbuf_puts(out, ", "); }
            if (!cat_agg) { jbuf_int(out, rcat->selection[ci]); jbuf_puts(out, ", "); }
            jbuf_real(out, d);
            jbuf_puts(out, "]");
        }
    }
    jbuf_puts(out, "]}");
    rc = 0;
done:
    free(vals); free(sums); free(w_cat);
    query_clear(&q);
    return rc;
}

/* arbplf-site-rate: the posterior mean relative rate of every site, sum_c post[s][c] * rate_c */
static int run_site_rate(const jval *root, jbuf *out)
{
    query q;
    int rc = -1;
    double *rate = NULL;
    query_init(&q);
    if (query_parse(&q, 8, root)) goto done;
    if (query_prepare(&q)) goto done;
    const char *names[] = {"site"};
    const host_reduction *reds[] = {&q.r_site};
    table_begin(out, names, reds, 1);
    if (q.r_site.agg_mode != AGG_NONE) {
        double sum[2] = {0, 0};
        if (q.U > 0 && plk_group_cat_posterior(q.eng, NULL, NULL, NULL, sum)) { catpost_failed(&q, "the aggregated site rate"); goto done; }
        double v = clean(((long double)sum[0] + (long double)sum[1]) / q.div_site);
        if (check_finite(v, "the aggregated site rate")) goto done;
        jbuf_puts(out, "[");
        jbuf_real(out, v);
        jbuf_puts(out, "]");
    } else {
        rate = malloc((size_t)(q.U + 1) * sizeof(double));
        if (!rate) goto done;
        if (q.U > 0 && plk_group_cat_posterior(q.eng, NULL, rate, NULL, NULL)) { catpost_failed(&q, "a site rate"); goto done; }
        for (int i = 0; i < q.r_site.selection_len; i++) {
            int s = q.r_site.selection[i];
            double v = clean(rate[q.site_to_u[s]]);
            if (check_finite(v, "a site rate")) goto done;
            if (i) jbuf_puts(out, ", ");
            jbuf_puts(out, "["); jbuf_int(out, s); jbuf_puts(out, ", "); jbuf_real(out, v); jbuf_puts(out, "]");
        }
    }
    jbuf_puts(out, "]}");
    rc = 0;
done:
    free(rate);
    query_clear(&q);
    return rc;
}

/* ------------------------------------------------------------------ rate-matrix-deriv */
/* arbplf-rate-matrix-deriv: d(site-aggregated log likelihood) / d(rate_matrix entry), every ordered pair of distinct
 * states, row-major.  The engine gives the gradient in the normalised matrix and in the root weights from one down
 * pass, one up pass and one Frechet run (plk_rate_matrix_sens); plk_rate_matrix_chain takes them through the divisor,
 * the stationary distribution and the equilibrium root prior to the raw entries. */
static int run_rate_matrix_deriv(const jval *root, jbuf *out)
{
    query q;
    int rc = -1;
    double *G = NULL, *rt = NULL, *grad = NULL;
    query_init(&q);
    if (query_parse(&q, 9, root)) goto done;
    if (query_prepare(&q)) goto done;
    const int k = q.m.k;
    G = calloc((size_t)k * k * 2 + 2, sizeof(double));
    rt = calloc((size_t)k * 2 + 2, sizeof(double));
    grad = calloc((size_t)k * k + 1, sizeof(double));
    if (!G || !rt || !grad) goto done;
    if (q.U > 0) {
        if (plk_group_rate_matrix_sens(q.eng, G, rt)) {
            const char *msg = plk_group_last_error(q.eng);
            if (strstr(msg, "site likelihood zero")) check_finite(NAN, "the rate matrix gradient");
            else fprintf(stderr, "error: %s\n", msg);
            goto done;
        }
        char err[160];
        if (plk_rate_matrix_chain(k, q.m.rate_matrix, q.m.use_equilibrium_divisor ? PLK_DIVISOR_EXIT_RATE : PLK_DIVISOR_NUMBER, q.m.rate_divisor,
                                  q.m.root_mode, G, rt, grad, err, sizeof err)) {
            fprintf(stderr, "error: %s\n", err[0] ? err : "the chain rule of the rate matrix gradient failed");
            goto done;
        }
    }
    jbuf_puts(out, "{\"columns\": [\"first_state\", \"second_state\", \"value\"], \"data\": [");
    int first = 1;
    for (int i = 0; i < k; i++)
        for (int j = 0; j < k; j++) {
            if (i == j) continue;
            double v = clean((long double)grad[(size_t)i * k + j] / q.div_site);
            if (check_finite(v, "the rate matrix gradient")) goto done;
            if (!first) jbuf_puts(out, ", ");
            first = 0;
            jbuf_puts(out, "["); jbuf_int(out, i); jbuf_puts(out, ", "); jbuf_int(out, j); jbuf_puts(out, ", "); jbuf_real(out, v); jbuf_puts(out, "]");
        }
    jbuf_puts(out, "]}");
    rc = 0;
done:
    free(G); free(rt); free(grad);
    query_clear(&q);
    return rc;
}

/* ------------------------------------------------------------------ mixture-deriv */
/* arbplf-mixture-deriv: d(site-aggregated log likelihood) / d(parameter of the rate mixture).  The engine gives the
 * gradient in the category priors and rates, taken as independent, from one down pass and one up pass
 * (plk_mixture_sens); plk_mixture_chain takes them to gamma_shape / invariable_prior or to the rates / prior arrays of a
 * custom mixture, the exit-rate divisor's dependence on the expected rate included. */
static void mixture_row(jbuf *out, int *first, const char *name, int c, double v)
{
    if (!*first) jbuf_puts(out, ", ");
    *first = 0;
    jbuf_puts(out, "[\""); jbuf_puts(out, name); jbuf_puts(out, "\", "); jbuf_int(out, c); jbuf_puts(out, ", "); jbuf_real(out, v); jbuf_puts(out, "]");
}

static int run_mixture_deriv(const jval *root, jbuf *out)
{
    query q;
    int rc = -1;
    double *ps = NULL, *rs = NULL, *dr = NULL, *dp = NULL;
    query_init(&q);
    if (query_parse(&q, 10, root)) goto done;
    if (query_prepare(&q)) goto done;
    const k0_mixture *mix = &q.m.mix;
    const int C = arbplf_k0_category_count(mix), n = mix->n;
    const int gamma = mix->mode == K0_MIX_GAMMA || mix->mode == K0_MIX_GAMMA_MEDIAN;
    ps = calloc((size_t)C * 2 + 2, sizeof(double));
    rs = calloc((size_t)C * 2 + 2, sizeof(double));
    dr = calloc((size_t)n + 1, sizeof(double));
    dp = calloc((size_t)n + 1, sizeof(double));
    if (!ps || !rs || !dr || !dp) goto done;
    double dshape = 0, dinv = 0;
    int has_inv = gamma && mix->invariable_prior != 0;
    if (q.U > 0) {
        if (plk_group_mixture_sens(q.eng, ps, rs)) {
            const char *msg = plk_group_last_error(q.eng);
            if (strstr(msg, "site likelihood zero")) check_finite(NAN, "the mixture gradient");
            else fprintf(stderr, "error: %s\n", msg);
            goto done;
        }
        char err[200];
        if (plk_mixture_chain(mix->mode, n, mix->rates, mix->prior, mix->gamma_shape, mix->invariable_prior,
                              q.m.use_equilibrium_divisor ? PLK_DIVISOR_EXIT_RATE : PLK_DIVISOR_NUMBER, ps, rs,
                              dr, dp, &dshape, &dinv, &has_inv, err, sizeof err)) {
            fprintf(stderr, "error: %s\n", err[0] ? err : "the chain rule of the mixture gradient failed");
            goto done;
        }
    }
    jbuf_puts(out, "{\"columns\": [\"parameter\", \"category\", \"value\"], \"data\": [");
    int first = 1;
    if (gamma) {
        double v = clean((long double)dshape / q.div_site);
        if (check_finite(v, "the mixture gradient")) goto done;
        mixture_row(out, &first, "gamma_shape", 0, v);
        if (has_inv) {
            v = clean((long double)dinv / q.div_site);
            if (check_finite(v, "the mixture gradient")) goto done;
            mixture_row(out, &first, "invariable_prior", 0, v);
        }
    } else {
        for (int c = 0; c < n; c++) {
            double v = clean((long double)dr[c] / q.div_site);
            if (check_finite(v, "the mixture gradient")) goto done;
            mixture_row(out, &first, "rate", c, v);
        }
        if (mix->mode == K0_MIX_CUSTOM)
            for (int c = 0; c < n; c++) {
                double v = clean((long double)dp[c] / q.div_site);
                if (check_finite(v, "the mixture gradient")) goto done;
                mixture_row(out, &first, "prior", c, v);
            }
    }
    jbuf_puts(out, "]}");
    rc = 0;
done:
    free(ps); free(rs); free(dr); free(dp);
    query_clear(&q);
    return rc;
}

/* ------------------------------------------------------------------ nni (kind 11)
 * The log likelihood of nearest-neighbour interchanges of the tree (no counterpart in the reference; include/plk.h:
 * plk_nni_ll).  "swaps": [[a, b], ...] in the user's edge indices, a = (v -> c) and b = (u -> s) with v a child of u and
 * s != v; omitted: every swap of the tree, ordered by (a, b) in the user's indices.  Columns site, first_edge,
 * second_edge, value; rows in the order of the request, site outermost; the site column goes under site aggregation. */
static int nni_pair_cmp(const void *x, const void *y)
{
    const int *p = x, *q = y;
    return p[0] != q[0] ? (p[0] > q[0]) - (p[0] < q[0]) : (p[1] > q[1]) - (p[1] < q[1]);
}

static int run_nni(const jval *root, jbuf *out)
{
    query q;
    int rc = -1;
    int *user = NULL, *csr = NULL, *user_to_csr = NULL;
    double *vals = NULL;
    query_init(&q);
    if (query_parse(&q, 11, root)) goto done;
    const host_model *m = &q.m;
    const int E = m->E;
    user_to_csr = malloc((size_t)(E + 1) * sizeof(int));
    if (!user_to_csr) goto done;
    for (int e = 0; e < E; e++) user_to_csr[m->csr_to_user[e]] = e;
    const jval *sw = j_get(root, "swaps");
    int n = 0;
    if (sw) {
        if (!j_is_array(sw)) { fprintf(stderr, "error: swaps must be an array of pairs of edge indices\n"); goto done; }
        n = (int)j_len(sw);
        user = malloc((size_t)(2 * n + 2) * sizeof(int));
        if (!user) goto done;
        for (int i = 0; i < n; i++) {
            const jval *p = j_at(sw, i);
            if (!j_is_array(p) || j_len(p) != 2) { fprintf(stderr, "error: swaps: entry %d is not a pair of edge indices\n", i); goto done; }
            for (int j = 0; j < 2; j++) {
                const jval *x = j_at(p, j);
                if (!j_is_int(x)) { fprintf(stderr, "error: swaps: entry %d: edge indices must be integers\n", i); goto done; }
                if (x->u.i < 0 || x->u.i >= E) { fprintf(stderr, "error: swaps: entry %d: edge index %lld is out of range\n", i, x->u.i); goto done; }
                user[2 * i + j] = (int)x->u.i;
            }
        }
    } else {
        n = plk_nni_swaps(m->N, m->indptr, m->indices, NULL);
        user = malloc((size_t)(2 * n + 2) * sizeof(int));
        if (!user) goto done;
        plk_nni_swaps(m->N, m->indptr, m->indices, user);
        for (int i = 0; i < 2 * n; i++) user[i] = m->csr_to_user[user[i]];
        qsort(user, (size_t)n, 2 * sizeof(int), nni_pair_cmp);
    }
    csr = malloc((size_t)(2 * n + 2) * sizeof(int));
    if (!csr) goto done;
    for (int i = 0; i < 2 * n; i++) csr[i] = user_to_csr[user[i]];
    /* a pair that is no swap is refused here, in the user's indices, whether or not a site is selected */
    {
        const int count = plk_nni_swaps(m->N, m->indptr, m->indices, NULL);
        int *all = malloc((size_t)(2 * count + 2) * sizeof(int));
        if (!all) goto done;
        plk_nni_swaps(m->N, m->indptr, m->indices, all);           /* sorted by (a, b) in CSR indices */
        for (int i = 0; i < n; i++)
            if (!bsearch(csr + 2 * i, all, (size_t)count, 2 * sizeof(int), nni_pair_cmp)) {
                fprintf(stderr, "error: swaps: entry %d: edges (%d, %d) are no swap: the first must start at a child of the node "
                                "the second starts at, and the second must not end there\n", i, user[2 * i], user[2 * i + 1]);
                free(all);
                goto done;
            }
        free(all);
    }
    if (query_prepare(&q)) goto done;
    const int agg = q.r_site.agg_mode != AGG_NONE;
    const long U = q.U;
    vals = malloc(((size_t)n * (agg ? 2 : (size_t)U) + 2) * sizeof(double));
    if (!vals) goto done;
    if (U > 0 && n > 0 && plk_group_nni_ll(q.eng, n, csr, agg ? NULL : vals, agg ? vals : NULL)) {
        fprintf(stderr, "error: %s\n", plk_group_last_error(q.eng));
        goto done;
    }
    jbuf_puts(out, agg ? "{\"columns\": [\"first_edge\", \"second_edge\", \"value\"], \"data\": ["
                       : "{\"columns\": [\"site\", \"first_edge\", \"second_edge\", \"value\"], \"data\": [");
    int first = 1;
    if (agg) {
        for (int i = 0; i < n; i++) {
            const double v = U > 0 ? clean(((long double)vals[2 * i] + (long double)vals[2 * i + 1]) / q.div_site) : 0.0;
            if (check_finite(v, "the aggregated log likelihood of a swapped tree")) goto done;
            if (!first) jbuf_puts(out, ", ");
            first = 0;
            jbuf_puts(out, "["); jbuf_int(out, user[2 * i]); jbuf_puts(out, ", "); jbuf_int(out, user[2 * i + 1]); jbuf_puts(out, ", ");
            jbuf_real(out, v); jbuf_puts(out, "]");
        }
    } else {
        for (int si = 0; si < q.r_site.selection_len; si++) {
            const int s = q.r_site.selection[si];
            for (int i = 0; i < n; i++) {
                const double v = clean(vals[(size_t)i * U + q.site_to_u[s]]);
                if (check_finite(v, "a site log likelihood of a swapped tree")) goto done;
                if (!first) jbuf_puts(out, ", ");
                first = 0;
                jbuf_puts(out, "["); jbuf_int(out, s); jbuf_puts(out, ", "); jbuf_int(out, user[2 * i]); jbuf_puts(out, ", ");
                jbuf_int(out, user[2 * i + 1]); jbuf_puts(out, ", "); jbuf_real(out, v); jbuf_puts(out, "]");
            }
        }
    }
    jbuf_puts(out, "]}");
    rc = 0;
done:
    free(user); free(csr); free(user_to_csr); free(vals);
    query_clear(&q);
    return rc;
}

/* ------------------------------------------------------------------ spr (kind 13)
 * The log likelihood of subtree prune-and-regraft moves of the tree (no counterpart in the reference; include/plk.h:
 * plk_spr_ll).  "spr" (optional): {"moves": [[prune, target], ...] in the user's edge indices, prune = (w -> x) and target
 * neither prune nor an edge below x (optional: every move of the tree, ordered by (prune, target) in the user's indices;
 * repeats allowed), "split" (optional, 0.5)}.  Columns site, prune, target, value; rows in the order of the request, site
 * outermost; the site column goes under site aggregation. */
static int run_spr(const jval *root, jbuf *out)
{
    static const char *const none[] = {NULL};
    static const char *const all[] = {"moves", "split", NULL};
    query q;
    int rc = -1;
    int *user = NULL, *csr = NULL, *user_to_csr = NULL, *canon = NULL;
    double *vals = NULL;
    double split = 0.5;
    query_init(&q);
    if (query_parse(&q, 13, root)) goto done;
    const host_model *m = &q.m;
    const int E = m->E;
    const jval *sp = j_get(root, "spr"), *mv = NULL;
    if (sp) {
        if (!j_is_object(sp)) { fprintf(stderr, "error: spr must be an object\n"); goto done; }
        if (host_check_keys(sp, none, all, "spr")) goto done;
        const jval *x = j_get(sp, "split");
        if (x) {
            if (!j_is_number(x) || !(j_number(x) >= 0 && j_number(x) <= 1)) { fprintf(stderr, "error: spr.split must be a number in [0, 1]\n"); goto done; }
            split = j_number(x);
        }
        mv = j_get(sp, "moves");
    }
    user_to_csr = malloc((size_t)(E + 1) * sizeof(int));
    if (!user_to_csr) goto done;
    for (int e = 0; e < E; e++) user_to_csr[m->csr_to_user[e]] = e;
    const int count = plk_spr_moves(m->N, m->indptr, m->indices, NULL);
    canon = malloc((size_t)(2 * (size_t)count + 2) * sizeof(int));
    if (!canon) goto done;
    plk_spr_moves(m->N, m->indptr, m->indices, canon);           /* sorted by (prune, target) in CSR indices */
    int n = 0;
    if (mv) {
        if (!j_is_array(mv)) { fprintf(stderr, "error: spr.moves must be an array of pairs of edge indices\n"); goto done; }
        n = (int)j_len(mv);
        user = malloc((size_t)(2 * (size_t)n + 2) * sizeof(int));
        if (!user) goto done;
        for (int i = 0; i < n; i++) {
            const jval *p = j_at(mv, i);
            if (!j_is_array(p) || j_len(p) != 2) { fprintf(stderr, "error: spr.moves: entry %d is not a pair of edge indices\n", i); goto done; }
            for (int j = 0; j < 2; j++) {
                const jval *x = j_at(p, j);
                if (!j_is_int(x)) { fprintf(stderr, "error: spr.moves: entry %d: edge indices must be integers\n", i); goto done; }
                if (x->u.i < 0 || x->u.i >= E) { fprintf(stderr, "error: spr.moves: entry %d: edge index %lld is out of range\n", i, x->u.i); goto done; }
                user[2 * i + j] = (int)x->u.i;
            }
        }
    } else {
        n = count;
        user = malloc((size_t)(2 * (size_t)n + 2) * sizeof(int));
        if (!user) goto done;
        for (int i = 0; i < 2 * n; i++) user[i] = m->csr_to_user[canon[i]];
        qsort(user, (size_t)n, 2 * sizeof(int), nni_pair_cmp);
    }
    csr = malloc((size_t)(2 * (size_t)n + 2) * sizeof(int));
    if (!csr) goto done;
    for (int i = 0; i < 2 * n; i++) csr[i] = user_to_csr[user[i]];
    /* a pair that is no move is refused here, in the user's indices, whether or not a site is selected */
    for (int i = 0; i < n; i++)
        if (!bsearch(csr + 2 * i, canon, (size_t)count, 2 * sizeof(int), nni_pair_cmp)) {
            fprintf(stderr, "error: spr.moves: entry %d: edges (%d, %d) are no move: the target must be neither the pruned edge nor "
                            "an edge of the subtree below it\n", i, user[2 * i], user[2 * i + 1]);
            goto done;
        }
    if (query_prepare(&q)) goto done;
    const int agg = q.r_site.agg_mode != AGG_NONE;
    const long U = q.U;
    vals = malloc(((size_t)n * (agg ? 2 : (size_t)U) + 2) * sizeof(double));
    if (!vals) goto done;
    if (U > 0 && n > 0 && plk_group_spr_ll(q.eng, n, csr, split, agg ? NULL : vals, agg ? vals : NULL)) {
        fprintf(stderr, "error: %s\n", plk_group_last_error(q.eng));
        goto done;
    }
    jbuf_puts(out, agg ? "{\"columns\": [\"prune\", \"target\", \"value\"], \"data\": ["
                       : "{\"columns\": [\"site\", \"prune\", \"target\", \"value\"], \"data\": [");
    int first = 1;
    if (agg) {
        for (int i = 0; i < n; i++) {
            const double v = U > 0 ? clean(((long double)vals[2 * i] + (long double)vals[2 * i + 1]) / q.div_site) : 0.0;
            if (check_finite(v, "the aggregated log likelihood of a moved tree")) goto done;
            if (!first) jbuf_puts(out, ", ");
            first = 0;
            jbuf_puts(out, "["); jbuf_int(out, user[2 * i]); jbuf_puts(out, ", "); jbuf_int(out, user[2 * i + 1]); jbuf_puts(out, ", ");
            jbuf_real(out, v); jbuf_puts(out, "]");
        }
    } else {
        for (int si = 0; si < q.r_site.selection_len; si++) {
            const int s = q.r_site.selection[si];
            for (int i = 0; i < n; i++) {
                const double v = clean(vals[(size_t)i * U + q.site_to_u[s]]);
                if (check_finite(v, "a site log likelihood of a moved tree")) goto done;
                if (!first) jbuf_puts(out, ", ");
                first = 0;
                jbuf_puts(out, "["); jbuf_int(out, s); jbuf_puts(out, ", "); jbuf_int(out, user[2 * i]); jbuf_puts(out, ", ");
                jbuf_int(out, user[2 * i + 1]); jbuf_puts(out, ", "); jbuf_real(out, v); jbuf_puts(out, "]");
            }
        }
    }
    jbuf_puts(out, "]}");
    rc = 0;
done:
    free(user); free(csr); free(user_to_csr); free(canon); free(vals);
    query_clear(&q);
    return rc;
}

/* ------------------------------------------------------------------ place (kind 12)
 * The log likelihood of the tree with a new taxon attached to an edge (no counterpart in the reference; include/plk.h:
 * plk_place_ll).  "placement": {"character_data": [site][query] character indices into the model's
 * character_definitions (a model with probability_array: "probability_array": [site][query][state]), "edges": user edge
 * indices (optional: every edge in document order; repeats allowed), "split" (optional, 0.5), "pendant_rate"}.
 * Columns site, query, edge, value; rows ordered by site, then query, then edge as listed; the site column goes under
 * site aggregation.  Patterns are compressed on the columns of the tree and of the queries together. */
typedef struct {
    int Q, n;              /* queries; listed edges */
    int *user;             /* [n] edges as listed */
    double split, pendant;
    uint8_t *codes;        /* [S][Q], when the model holds codes */
    double *prob;          /* [S][Q][k] otherwise */
} place_req;

static void place_clear(place_req *pr)
{
    free(pr->user); free(pr->codes); free(pr->prob);
    memset(pr, 0, sizeof *pr);
}

/* row c of the model's character definitions: the model's own copy, or the document's where the model kept none */
static void place_def_row(const host_model *m, const jval *defs, int c, double *out)
{
    if (m->defs) { memcpy(out, m->defs + (size_t)c * m->k, (size_t)m->k * sizeof(double)); return; }
    const jval *row = j_at(defs, c);
    for (int j = 0; j < m->k; j++) out[j] = j_number(j_at(row, j));
}

/* the model's observations back in dense form (a probability_array that had been re-expressed as codes) */
static int place_model_to_dense(host_model *m)
{
    const size_t rows = (size_t)m->S * m->N, k = (size_t)m->k;
    m->prob = malloc((rows * k + 1) * sizeof(double));
    if (!m->prob) return -1;
    for (size_t r = 0; r < rows; r++) memcpy(m->prob + r * k, m->defs + (size_t)m->codes8[r] * k, k * sizeof(double));
    free(m->codes8); m->codes8 = NULL;
    free(m->defs); m->defs = NULL;
    m->nchar = 0;
    return 0;
}

#define PLACE_FAIL(...) do { fprintf(stderr, __VA_ARGS__); return -1; } while (0)

static int place_parse(place_req *pr, host_model *m, const jval *root)
{
    static const char *const req[] = {"pendant_rate", NULL};
    static const char *const all[] = {"character_data", "probability_array", "edges", "split", "pendant_rate", NULL};
    const jval *pl = j_get(root, "placement"), *md = j_get(root, "model_and_data");
    if (!pl) PLACE_FAIL("error: placement is required\n");
    if (!j_is_object(pl)) PLACE_FAIL("error: placement must be an object\n");
    if (host_check_keys(pl, req, all, "placement")) return -1;
    const int k = m->k, E = m->E;
    const long S = m->S;
    const int model_pa = j_get(md, "probability_array") && !j_is_null(j_get(md, "probability_array"));
    const jval *cd = j_get(pl, "character_data"), *pa = j_get(pl, "probability_array");
    if (cd && pa) PLACE_FAIL("error: placement: give either character_data or probability_array, not both\n");
    if (model_pa && !pa) PLACE_FAIL("error: placement: the model holds a probability_array, so the queries must come as placement.probability_array\n");
    if (!model_pa && !cd) PLACE_FAIL("error: placement: the model holds character data, so the queries must come as placement.character_data\n");
    const jval *qd = cd ? cd : pa;
    const char *name = cd ? "placement.character_data" : "placement.probability_array";
    if (!j_is_array(qd)) PLACE_FAIL("error: %s: a list per site with one entry per query is required\n", name);
    if ((long)j_len(qd) != S) PLACE_FAIL("error: %s: %ld rows, the model has %ld sites\n", name, (long)j_len(qd), S);
    pr->Q = S > 0 && j_is_array(j_at(qd, 0)) ? (int)j_len(j_at(qd, 0)) : 0;
    const int Q = pr->Q;
    for (long s = 0; s < S; s++) {
        const jval *x = j_at(qd, s);
        if (!j_is_array(x)) PLACE_FAIL("error: %s: a list per site with one entry per query is required\n", name);
        if ((int)j_len(x) != Q) PLACE_FAIL("error: %s: rows of unequal length (site %ld lists %d queries, site 0 lists %d)\n", name, s, (int)j_len(x), Q);
    }
    const jval *defs = j_get(md, "character_definitions");
    const int ndefs = cd ? (m->defs ? m->nchar : (int)j_len(defs)) : 0;
    /* the queries in the form the model's observations have now: codes, or dense rows */
    pr->prob = malloc(((size_t)S * Q * k + 1) * sizeof(double));
    if (!pr->prob) return -1;
    for (long s = 0; s < S; s++)
        for (int qi = 0; qi < Q; qi++) {
            const jval *y = j_at(j_at(qd, s), qi);
            double *row = pr->prob + ((size_t)s * Q + qi) * k;
            if (cd) {
                if (!j_is_int(y)) PLACE_FAIL("error: %s: a character index is not an integer\n", name);
                if (y->u.i < 0 || y->u.i >= ndefs) PLACE_FAIL("error: %s: character index %lld is out of range: the model has %d definitions\n", name, y->u.i, ndefs);
                place_def_row(m, defs, (int)y->u.i, row);
            } else {
                if (!j_is_array(y) || (int)j_len(y) != k) PLACE_FAIL("error: %s: every query needs one row of %d probabilities per site\n", name, k);
                for (int j = 0; j < k; j++) {
                    const jval *z = j_at(y, j);
                    if (!j_is_number(z) || !(j_number(z) >= 0) || !isfinite(j_number(z)))
                        PLACE_FAIL("error: %s: entries must be finite numbers that are not negative\n", name);
                    row[j] = j_number(z);
                }
            }
        }
    if (m->codes8) {
        /* codes: the character index itself, or for a probability_array the row's place among the definitions the model
         * derived, which take the rows of the queries too while there is room for them */
        pr->codes = malloc((size_t)S * Q + 1);
        if (!pr->codes) return -1;
        int fits = 1;
        for (size_t r = 0; fits && r < (size_t)S * Q; r++) {
            const double *row = pr->prob + r * k;
            if (cd) { pr->codes[r] = (uint8_t)j_at(j_at(qd, r / Q), r % Q)->u.i; continue; }
            int found = -1;
            for (int c = 0; c < m->nchar && found < 0; c++)
                if (!memcmp(m->defs + (size_t)c * k, row, (size_t)k * sizeof(double))) found = c;
            /* room for the new row: parse_probability_array (host_model.c) allocates the derived definitions for 256 rows
             * whatever their number, and only such models come here (cd == NULL) */
            if (found < 0 && m->nchar < 256) { memcpy(m->defs + (size_t)m->nchar * k, row, (size_t)k * sizeof(double)); found = m->nchar++; }
            if (found < 0) fits = 0;
            else pr->codes[r] = (uint8_t)found;
        }
        if (fits) { free(pr->prob); pr->prob = NULL; }
        else {
            free(pr->codes); pr->codes = NULL;
            if (place_model_to_dense(m)) return -1;
        }
    }
    /* edges */
    const jval *ed = j_get(pl, "edges");
    if (ed && !j_is_array(ed)) PLACE_FAIL("error: placement.edges must be an array of edge indices\n");
    pr->n = ed ? (int)j_len(ed) : E;
    pr->user = malloc((size_t)(pr->n + 1) * sizeof(int));
    if (!pr->user) return -1;
    for (int i = 0; i < pr->n; i++) {
        if (!ed) { pr->user[i] = i; continue; }
        const jval *x = j_at(ed, i);
        if (!j_is_int(x)) PLACE_FAIL("error: placement.edges: entry %d: edge indices must be integers\n", i);
        if (x->u.i < 0 || x->u.i >= E) PLACE_FAIL("error: placement.edges: entry %d: edge index %lld is out of range\n", i, x->u.i);
        pr->user[i] = (int)x->u.i;
    }
    const jval *sp = j_get(pl, "split"), *pe = j_get(pl, "pendant_rate");
    pr->split = 0.5;
    if (sp) {
        if (!j_is_number(sp) || !(j_number(sp) >= 0 && j_number(sp) <= 1)) PLACE_FAIL("error: placement.split must be a number in [0, 1]\n");
        pr->split = j_number(sp);
    }
    if (!j_is_number(pe) || !(j_number(pe) >= 0) || !isfinite(j_number(pe))) PLACE_FAIL("error: placement.pendant_rate must be a finite number that is not negative\n");
    pr->pendant = j_number(pe);
    return 0;
}

/* the rates of the new edges against what the transition matrix kernel accepts, naming edges as the document does;
 * query_k0 has run */
static int place_k1(const query *q, const place_req *pr)
{
    const host_model *m = &q->m;
    const double *root_w = m->root_mode == HM_ROOT_CUSTOM ? m->root_custom : (m->root_mode == HM_ROOT_EQUILIBRIUM ? q->pi : NULL);
    const double lower = 1.0 - pr->split;
    for (int i = 0; i <= pr->n; i++) {
        const double r_e = i < pr->n ? m->edge_rates_user[pr->user[i]] : 0.0;
        const double rates[2] = {i < pr->n ? pr->split * r_e : pr->pendant, lower * r_e};
        for (int j = 0; j < (i < pr->n ? 2 : 1); j++)
            if (plk_k1_check_values(m->k, q->C, 1, q->Qn, q->Qn_lo, rates + j, q->cat_rates, q->cat_prior, m->root_mode, root_w, NULL, 0)) {
                if (i == pr->n) fprintf(stderr, "error: placement.pendant_rate %g: rate x length x |Qn| is beyond 2^40, the limit of the transition matrix kernel\n", rates[j]);
                else fprintf(stderr, "error: placement: the %s part of edge %d (rate %g): rate x length x |Qn| is beyond 2^40, the limit of the transition matrix kernel\n",
                             j ? "lower" : "upper", pr->user[i], rates[j]);
                return -1;
            }
    }
    return 0;
}

static int run_place(const jval *root, jbuf *out)
{
    query q;
    place_req pr;
    int rc = -1;
    int *csr = NULL;
    uint8_t *codes = NULL;
    double *dense = NULL, *vals = NULL;
    query_init(&q);
    memset(&pr, 0, sizeof pr);
    if (query_parse(&q, 12, root)) goto done;
    if (place_parse(&pr, &q.m, root)) goto done;
    const host_model *m = &q.m;
    const int Q = pr.Q, n = pr.n, k = m->k;
    /* two sites are one pattern only when they agree on the tree's columns and on every query */
    q.xrows = pr.codes ? (const unsigned char *)pr.codes : (const unsigned char *)pr.prob;
    q.xrow_bytes = pr.codes ? (size_t)Q : (size_t)Q * k * sizeof(double);
    if (query_prepare(&q)) goto done;
    const int agg = q.r_site.agg_mode != AGG_NONE;
    const long U = q.U;
    if (U > 0 && place_k1(&q, &pr)) goto done;
    csr = malloc((size_t)(n + 1) * sizeof(int));
    if (!csr) goto done;
    for (int i = 0; i < n; i++) csr[i] = m->edge_order[pr.user[i]];
    /* the queries of the evaluated patterns, device layout (site fastest) */
    if (pr.codes) {
        codes = malloc((size_t)Q * U + 1);
        if (!codes) goto done;
        for (long u = 0; u < U; u++)
            for (int qi = 0; qi < Q; qi++) codes[(size_t)qi * U + u] = pr.codes[(size_t)q.usites[u] * Q + qi];
    } else {
        dense = malloc(((size_t)Q * k * U + 1) * sizeof(double));
        if (!dense) goto done;
        for (long u = 0; u < U; u++)
            for (int qi = 0; qi < Q; qi++)
                for (int j = 0; j < k; j++) dense[((size_t)qi * k + j) * U + u] = pr.prob[((size_t)q.usites[u] * Q + qi) * k + j];
    }
    const size_t rows = (size_t)Q * n;
    vals = malloc((rows * (agg ? 2 : (size_t)U) + 2) * sizeof(double));
    if (!vals) goto done;
    if (U > 0 && rows > 0 && plk_group_place_ll(q.eng, Q, codes, dense, n, csr, pr.split, pr.pendant, agg ? NULL : vals, agg ? vals : NULL)) {
        fprintf(stderr, "error: %s\n", plk_group_last_error(q.eng));
        goto done;
    }
    jbuf_puts(out, agg ? "{\"columns\": [\"query\", \"edge\", \"value\"], \"data\": ["
                       : "{\"columns\": [\"site\", \"query\", \"edge\", \"value\"], \"data\": [");
    int first = 1;
    for (int si = 0; si < (agg ? 1 : q.r_site.selection_len); si++) {
        const int s = agg ? 0 : q.r_site.selection[si];
        for (int qi = 0; qi < Q; qi++)
            for (int i = 0; i < n; i++) {
                const size_t r = (size_t)qi * n + i;
                const double v = agg ? (U > 0 ? clean(((long double)vals[2 * r] + (long double)vals[2 * r + 1]) / q.div_site) : 0.0)
                                     : clean(vals[r * U + q.site_to_u[s]]);
                if (check_finite(v, agg ? "the aggregated log likelihood of a placement" : "a site log likelihood of a placement")) goto done;
                if (!first) jbuf_puts(out, ", ");
                first = 0;
                jbuf_puts(out, "[");
                if (!agg) { jbuf_int(out, s); jbuf_puts(out, ", "); }
                jbuf_int(out, qi); jbuf_puts(out, ", "); jbuf_int(out, pr.user[i]); jbuf_puts(out, ", ");
                jbuf_real(out, v); jbuf_puts(out, "]");
            }
    }
    jbuf_puts(out, "]}");
    rc = 0;
done:
    free(csr); free(codes); free(dense); free(vals);
    place_clear(&pr);
    query_clear(&q);
    return rc;
}

/* ------------------------------------------------------------------ string API */
static char *string_hom(int (*run)(const jval *, jbuf *), void *userdata, const char *s_in, int *retcode)
{
    char err[256];
    char *s_out = NULL;
    int rc = -1;
    if (retcode) *retcode = -1;
    if (userdata) { fprintf(stderr, "internal error: unexpected userdata\n"); return NULL; }
    if (!s_in) { fprintf(stderr, "error: null input\n"); return NULL; }
    json_doc *doc = json_doc_parse(s_in, err, sizeof err);
    if (!doc) { fprintf(stderr, "%s\n", err); return NULL; }
    jbuf b;
    jbuf_init(&b);
    pthread_mutex_lock(&g_mu);
    rc = run(json_doc_root(doc), &b);
    pthread_mutex_unlock(&g_mu);
    json_doc_free(doc);
    if (rc == 0) {
        s_out = jbuf_take(&b);
        if (!s_out) { fprintf(stderr, "error: failed to dump the json object to a string\n"); rc = -1; }
    } else {
        free(jbuf_take(&b));
    }
    if (retcode) *retcode = rc;
    return s_out;
}

char *arbplf_ll_string(void *userdata, const char *s_in, int *retcode) { return string_hom(run_ll, userdata, s_in, retcode); }
char *arbplf_deriv_string(void *userdata, const char *s_in, int *retcode) { return string_hom(run_deriv, userdata, s_in, retcode); }
char *arbplf_marginal_string(void *userdata, const char *s_in, int *retcode) { return string_hom(run_marginal, userdata, s_in, retcode); }
char *arbplf_dwell_string(void *userdata, const char *s_in, int *retcode) { return string_hom(run_dwell, userdata, s_in, retcode); }
char *arbplf_trans_string(void *userdata, const char *s_in, int *retcode) { return string_hom(run_trans, userdata, s_in, retcode); }
char *arbplf_em_update_string(void *userdata, const char *s_in, int *retcode) { return string_hom(run_em_update, userdata, s_in, retcode); }
char *arbplf_hess_string(void *userdata, const char *s_in, int *retcode) { return string_hom(run_hess, userdata, s_in, retcode); }
char *arbplf_inv_hess_string(void *userdata, const char *s_in, int *retcode) { return string_hom(run_inv_hess, userdata, s_in, retcode); }
char *arbplf_newton_delta_string(void *userdata, const char *s_in, int *retcode) { return string_hom(run_newton_delta, userdata, s_in, retcode); }
char *arbplf_newton_update_string(void *userdata, const char *s_in, int *retcode) { return string_hom(run_newton_update, userdata, s_in, retcode); }
char *arbplf_cat_posterior_string(void *userdata, const char *s_in, int *retcode) { return string_hom(run_cat_posterior, userdata, s_in, retcode); }
char *arbplf_site_rate_string(void *userdata, const char *s_in, int *retcode) { return string_hom(run_site_rate, userdata, s_in, retcode); }
char *arbplf_rate_matrix_deriv_string(void *userdata, const char *s_in, int *retcode) { return string_hom(run_rate_matrix_deriv, userdata, s_in, retcode); }
char *arbplf_mixture_deriv_string(void *userdata, const char *s_in, int *retcode) { return string_hom(run_mixture_deriv, userdata, s_in, retcode); }
char *arbplf_nni_string(void *userdata, const char *s_in, int *retcode) { return string_hom(run_nni, userdata, s_in, retcode); }
char *arbplf_place_string(void *userdata, const char *s_in, int *retcode) { return string_hom(run_place, userdata, s_in, retcode); }
char *arbplf_spr_string(void *userdata, const char *s_in, int *retcode) { return string_hom(run_spr, userdata, s_in, retcode); }

/* Host-only validation (JSON grammar, model, reductions and, where a site is selected, the prepared model's values
 * against what the transition matrix kernel accepts); no GPU is touched.
 * what: "ll", "deriv", "marginal", "dwell", "trans", "em_update", "hess", "inv_hess", "newton_delta", "newton_update",
 * "cat_posterior", "site_rate", "rate_matrix_deriv", "mixture_deriv", "nni" (the model and the reductions; the swap
 * list is checked by the query itself), "place" (with the whole "placement" object and the rates of its new edges) or
 * "spr" (the model and the reductions; the "spr" object is checked by the query itself).
 * Returns 0 when the input would be accepted. */
int arbplf_validate_string(const char *what, const char *s_in)
{
    char err[256];
    int kind = !strcmp(what, "ll") ? 0 : !strcmp(what, "deriv") ? 1 : !strcmp(what, "marginal") ? 2 :
               !strcmp(what, "dwell") ? 3 : !strcmp(what, "trans") ? 4 : !strcmp(what, "em_update") ? 5 : !strcmp(what, "hess") ? 6 :
               (!strcmp(what, "inv_hess") || !strcmp(what, "newton_delta") || !strcmp(what, "newton_update")) ? 6 :
               !strcmp(what, "cat_posterior") ? 7 : !strcmp(what, "site_rate") ? 8 : !strcmp(what, "rate_matrix_deriv") ? 9 :
               !strcmp(what, "mixture_deriv") ? 10 : !strcmp(what, "nni") ? 11 : !strcmp(what, "place") ? 12 : !strcmp(what, "spr") ? 13 : -1;
    if (kind < 0 || !s_in) return -1;
    json_doc *doc = json_doc_parse(s_in, err, sizeof err);
    if (!doc) { fprintf(stderr, "%s\n", err); return -1; }
    query q;
    query_init(&q);
    int rc = query_parse(&q, kind, json_doc_root(doc));
    place_req pr;
    memset(&pr, 0, sizeof pr);
    if (rc == 0 && kind == 12) rc = place_parse(&pr, &q.m, json_doc_root(doc));
    /* as query_prepare: a document that selects no site is answered without preparing its model */
    if (rc == 0 && q.r_site.selection_len > 0) rc = query_k0(&q);
    if (rc == 0 && kind == 12 && q.r_site.selection_len > 0) rc = place_k1(&q, &pr);
    place_clear(&pr);
    query_clear(&q);
    json_doc_free(doc);
    return rc;
}

/* src/runjson.c:88-147: read all of stdin, run, print one line */
int arbplf_run_stdin(char *(*f)(void *, const char *, int *))
{
    size_t cap = 1 << 16, n = 0;
    char *buf = malloc(cap);
    if (!buf) { fprintf(stderr, "failed to read string from stdin\n"); return -1; }
    while (1) {
        if (n + 4096 > cap) {
            cap *= 2;
            char *nb = realloc(buf, cap);
            if (!nb) { free(buf); fprintf(stderr, "failed to read string from stdin\n"); return -1; }
            buf = nb;
        }
        size_t got = fread(buf + n, 1, cap - n - 1, stdin);
        n += got;
        if (got == 0) break;
    }
    buf[n] = 0;
    int retcode = 0;
    char *s_out = f(NULL, buf, &retcode);
    free(buf);
    if (s_out) { puts(s_out); free(s_out); }
    arbplf_shutdown();
    return retcode;
}
