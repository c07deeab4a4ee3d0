/*
 * oracle/plf_site.inc -- TEST INFRASTRUCTURE (included three times by
 * plf_core.c with REAL = binary128 / long double / double).  Per-site evaluators restating
 * src/evaluate_site_lhood.c, src/evaluate_site_forward.c,
 * src/evaluate_site_marginal.c and src/arbplfderiv.c:112-207.
 */

typedef struct {
    REAL *base;   /* N*k  base node vectors (src/model.c:182-199) */
    REAL *lnode;  /* N*k  lhood node vectors */
    REAL *ledge;  /* E*k  lhood edge vectors */
    REAL *fnode;  /* N*k  forward node vectors */
    REAL *fedge;  /* E*k  forward edge vectors */
    REAL *dnode;  /* N*k  derivative node vectors */
    REAL *acc;    /* max(N*k, E) cross-category accumulators */
    REAL *tmp;    /* k */
    int *b_to_idx, *idx_to_a; /* src/util.c _csr_graph_get_backward_maps */
} SUF(site_ws);

static void *SUF(site_ws_alloc)(const orc_problem *p)
{
    size_t nk = (size_t)p->N * p->k, ek = (size_t)p->E * p->k;
    size_t accn = nk > (size_t)p->E ? nk : (size_t)p->E;
    size_t reals = 4 * nk + 2 * ek + accn + p->k;
    char *mem = malloc(sizeof(SUF(site_ws)) + reals * sizeof(REAL) + (p->N + p->E) * sizeof(int) + 64);
    SUF(site_ws) *w = (SUF(site_ws) *)mem;
    REAL *r = (REAL *)(mem + ((sizeof(SUF(site_ws)) + 15) / 16) * 16);
    w->base = r; r += nk; w->lnode = r; r += nk; w->fnode = r; r += nk; w->dnode = r; r += nk;
    w->ledge = r; r += ek; w->fedge = r; r += ek; w->acc = r; r += accn; w->tmp = r; r += p->k;
    w->b_to_idx = (int *)r; w->idx_to_a = w->b_to_idx + p->N;
    for (int a = 0; a < p->N; a++) w->b_to_idx[a] = -1;
    for (int a = 0; a < p->N; a++)
        for (int idx = p->indptr[a]; idx < p->indptr[a + 1]; idx++) {
            w->idx_to_a[idx] = a;
            w->b_to_idx[p->indices[idx]] = idx;
        }
    return w;
}

static void SUF(load_base)(const orc_problem *p, SUF(site_ws) *w, long s)
{
    int N = p->N, k = p->k;
    for (int a = 0; a < N; a++) {
        const double *src = p->B ? p->B + ((size_t)s * N + a) * k
                                 : p->defs + (size_t)p->codes[(size_t)s * N + a] * k;
        for (int j = 0; j < k; j++) w->base[(size_t)a * k + j] = (REAL)src[j];
    }
}

/* src/model.c:283-350 root_prior_expectation */
static REAL SUF(root_expect)(const orc_problem *p, const REAL *v)
{
    int k = p->k;
    REAL out = 0;
    if (p->root_mode == 1) { for (int i = 0; i < k; i++) out += v[i]; }
    else if (p->root_mode == 3) { for (int i = 0; i < k; i++) out += v[i]; out /= (REAL)k; }
    else { for (int i = 0; i < k; i++) out += (REAL)p->root_w[i] * v[i]; }
    return out;
}

/*
 * src/evaluate_site_lhood.c:7-63.  Returns the category likelihood; when
 * RESCALE is on (double build) node vectors are renormalised by an exact
 * power of two and *scale_out accumulates the exponent (only valid when
 * store_edges == 0, i.e. the ll path).
 */
static REAL SUF(site_lhood)(const orc_problem *p, SUF(site_ws) *w, int cat,
                            int store_edges, long *scale_out)
{
    int N = p->N, k = p->k;
    long scale = 0;
    const PT *Pc = (const PT *)p->P + (size_t)cat * p->E * k * k;
    for (int u = 0; u < N; u++) {
        int a = p->preorder[N - 1 - u];
        REAL *na = w->lnode + (size_t)a * k;
        for (int j = 0; j < k; j++) na[j] = w->base[(size_t)a * k + j];
        for (int idx = p->indptr[a]; idx < p->indptr[a + 1]; idx++) {
            int b = p->indices[idx];
            const PT *T = Pc + (size_t)idx * k * k;
            const REAL *nb = w->lnode + (size_t)b * k;
            REAL *ev = store_edges ? w->ledge + (size_t)idx * k : w->tmp;
            int constant = 1; /* exact constant column: A*B = B (src/util.c:276-283) */
            for (int j = 1; j < k; j++) if (nb[j] != nb[0]) { constant = 0; break; }
            if (constant) { for (int i = 0; i < k; i++) ev[i] = nb[0]; }
            else for (int i = 0; i < k; i++) {
                REAL acc = 0;
                for (int j = 0; j < k; j++) acc += (REAL)T[i * k + j] * nb[j];
                ev[i] = acc;
            }
            for (int i = 0; i < k; i++) na[i] *= ev[i];
        }
#if RESCALE
        if (!store_edges && p->indptr[a + 1] > p->indptr[a]) {
            REAL m = 0;
            for (int j = 0; j < k; j++) if (na[j] > m) m = na[j];
            if (m > 0 && m < 0x1p-200) {
                int e = ilogb(m);
                for (int j = 0; j < k; j++) na[j] = scalbn(na[j], -e);
                scale += e;
            }
        }
#endif
    }
    if (scale_out) *scale_out = scale;
    return SUF(root_expect)(p, w->lnode + (size_t)p->preorder[0] * k);
}

/* src/arbplfll.c:139-170: ll_s = log(sum_c prior_c * lhood_{s,c}) */
static double SUF(site_ll)(const orc_problem *p, void *wsv, long s)
{
    SUF(site_ws) *w = wsv;
    SUF(load_base)(p, w, s);
#if RESCALE
    /* combine categories at a common exponent */
    REAL vals[64]; long exps[64];
    int C = p->C;
    long emax = -(1L << 60);
    REAL total = 0;
    if (C > 64) return NAN;
    for (int c = 0; c < C; c++) {
        vals[c] = (REAL)p->cat_prior[c] * SUF(site_lhood)(p, w, c, 0, &exps[c]);
        if (vals[c] != 0 && exps[c] > emax) emax = exps[c];
    }
    if (emax == -(1L << 60)) emax = 0;
    for (int c = 0; c < C; c++)
        if (vals[c] != 0) total += scalbn(vals[c], (int)(exps[c] - emax));
    return (double)(log(total) + (REAL)emax * (REAL)0.6931471805599453094172321214581766L);
#else
    REAL total = 0;
    for (int c = 0; c < p->C; c++)
        total += (REAL)p->cat_prior[c] * SUF(site_lhood)(p, w, c, 0, NULL);
    return (double)LOGF(total);
#endif
}

/* src/evaluate_site_forward.c:32-105 */
static void SUF(site_forward)(const orc_problem *p, SUF(site_ws) *w, int cat)
{
    int N = p->N, k = p->k;
    const PT *Pc = (const PT *)p->P + (size_t)cat * p->E * k * k;
    {
        REAL *fr = w->fnode + (size_t)p->preorder[0] * k;
        /* src/model.c:226-280 root_prior_mul_col_vec applied to ones */
        for (int i = 0; i < k; i++) {
            if (p->root_mode == 1) fr[i] = 1;
            else if (p->root_mode == 3) fr[i] = (REAL)1 / (REAL)k;
            else fr[i] = (REAL)p->root_w[i];
        }
    }
    for (int u = 0; u < N; u++) {
        int a = p->preorder[u];
        int start = p->indptr[a], stop = p->indptr[a + 1];
        for (int i = 0; i < k; i++)
            w->tmp[i] = w->fnode[(size_t)a * k + i] * w->base[(size_t)a * k + i];
        for (int idx = start; idx < stop; idx++) {
            int b = p->indices[idx];
            REAL *fe = w->fedge + (size_t)idx * k;
            REAL *fb = w->fnode + (size_t)b * k;
            for (int i = 0; i < k; i++) fe[i] = w->tmp[i];
            for (int idx2 = start; idx2 < stop; idx2++)
                if (idx2 != idx)
                    for (int i = 0; i < k; i++) fe[i] *= w->ledge[(size_t)idx2 * k + i];
            const PT *T = Pc + (size_t)idx * k * k;
            for (int i = 0; i < k; i++) {
                REAL acc = 0;
                for (int j = 0; j < k; j++) acc += (REAL)T[j * k + i] * fe[j];
                fb[i] = acc;
            }
        }
    }
}

/* src/arbplfmarginal.c:111-264 (one site, all nodes and states) */
static void SUF(site_marginal)(const orc_problem *p, void *wsv, long s, double *out)
{
    SUF(site_ws) *w = wsv;
    int N = p->N, k = p->k;
    size_t nk = (size_t)N * k;
    SUF(load_base)(p, w, s);
    for (size_t i = 0; i < nk; i++) w->acc[i] = 0;
    REAL site_lhood = 0;
    for (int c = 0; c < p->C; c++) {
        REAL post = (REAL)p->cat_prior[c] * SUF(site_lhood)(p, w, c, 1, NULL);
        if (post == 0) continue;          /* :190-191 */
        site_lhood += post;
        SUF(site_forward)(p, w, c);
        for (size_t i = 0; i < nk; i++)   /* src/evaluate_site_marginal.c:7-21 */
            w->acc[i] += w->fnode[i] * w->lnode[i] * (REAL)p->cat_prior[c];
    }
    for (size_t i = 0; i < nk; i++) out[i] = (double)(w->acc[i] / site_lhood);
}

/* src/arbplfderiv.c:112-207 + :294-342, reference's root-path formulation */
static void SUF(site_deriv)(const orc_problem *p, void *wsv, long s,
                            const int *edge_requested, double *out)
{
    SUF(site_ws) *w = wsv;
    int N = p->N, E = p->E, k = p->k;
    (void)N;
    SUF(load_base)(p, w, s);
    for (int e = 0; e < E; e++) w->acc[e] = 0;
    REAL post_sum = 0;
    for (int c = 0; c < p->C; c++) {
        const PT *Pc = (const PT *)p->P + (size_t)c * E * k * k;
        REAL cat_lhood = SUF(site_lhood)(p, w, c, 1, NULL);
        post_sum += (REAL)p->cat_prior[c] * cat_lhood;
        for (int de = 0; de < E; de++) {
            if (edge_requested && !edge_requested[de]) continue;
            int curr = de;
            while (curr != -1) {
                int a = w->idx_to_a[curr];
                REAL *na = w->dnode + (size_t)a * k;
                for (int j = 0; j < k; j++) na[j] = w->base[(size_t)a * k + j];
                for (int idx = p->indptr[a]; idx < p->indptr[a + 1]; idx++) {
                    if (idx == de) {
                        /* _prune_update_rate: na o= Q * Ev_e (src/util.c:304-362) */
                        const REAL *ev = w->ledge + (size_t)idx * k;
                        for (int i = 0; i < k; i++) {
                            REAL acc = 0;
                            for (int j = 0; j < k; j++) acc += (REAL)((const PT *)p->Qn)[i * k + j] * ev[j];
                            w->tmp[i] = acc;
                        }
                        for (int i = 0; i < k; i++) na[i] *= w->tmp[i];
                    } else if (idx == curr) {
                        int b = p->indices[idx];
                        const PT *T = Pc + (size_t)idx * k * k;
                        const REAL *nb = w->dnode + (size_t)b * k;
                        for (int i = 0; i < k; i++) {
                            REAL acc = 0;
                            for (int j = 0; j < k; j++) acc += (REAL)T[i * k + j] * nb[j];
                            w->tmp[i] = acc;
                        }
                        for (int i = 0; i < k; i++) na[i] *= w->tmp[i];
                    } else {
                        const REAL *ev = w->ledge + (size_t)idx * k;
                        for (int i = 0; i < k; i++) na[i] *= ev[i];
                    }
                }
                curr = w->b_to_idx[a];
            }
            REAL d = SUF(root_expect)(p, w->dnode + (size_t)p->preorder[0] * k);
            w->acc[de] += d * (REAL)p->cat_rates[c] * (REAL)p->cat_prior[c];
        }
    }
    for (int e = 0; e < E; e++) out[e] = (double)(w->acc[e] / post_sum);
}

/*
 * Conditional edge expectations from Frechet matrices:
 * src/evaluate_site_frechet.c:5-42 for one category, accumulated over
 * categories and divided by the site likelihood as in
 * src/arbplfdwell.c:205-300 (coef_mode 0: prior_c),
 * src/arbplftrans.c:233-330 (coef_mode 1: prior_c * cat_rate_c * edge_rate_e) and
 * src/arbplfem.c:258-390 (coef_mode 2: prior_c * cat_rate_c).
 * F is [C][E][k][k] in the build's matrix type.
 */
static void SUF(site_edge_expect)(const orc_problem *p, void *wsv, long s,
                                  const int *edge_requested, const PT *F, int coef_mode,
                                  const double *edge_rates_csr, double *out)
{
    SUF(site_ws) *w = wsv;
    int E = p->E, k = p->k;
    SUF(load_base)(p, w, s);
    for (int e = 0; e < E; e++) w->acc[e] = 0;
    REAL site_lhood = 0;
    for (int c = 0; c < p->C; c++) {
        REAL cat_lhood = (REAL)p->cat_prior[c] * SUF(site_lhood)(p, w, c, 1, NULL);
        site_lhood += cat_lhood;
        /* every category counts, also one whose likelihood is 0 at this site (the rate-0 category under data that
         * changes along the tree): the category loops of src/arbplfdwell.c:228-278 and src/arbplftrans.c skip none,
         * and fe^T F L_b need not vanish there for a direction L with off-diagonal entries (include/plk.h,
         * plk_edge_expect).  The JSON drivers cannot tell the difference: for their directions (diagonal, or weights
         * o Qn) F_{c,e} is 0 wherever P_{c,e} is, so their terms vanish with the category likelihood */
        SUF(site_forward)(p, w, c);
        for (int idx = 0; idx < E; idx++) {
            if (edge_requested && !edge_requested[idx]) continue;
            int b = p->indices[idx];
            const PT *Fm = F + ((size_t)c * E + idx) * k * k;
            const REAL *lb = w->lnode + (size_t)b * k;
            const REAL *fe = w->fedge + (size_t)idx * k;
            REAL tot = 0;
            for (int i = 0; i < k; i++) {
                REAL acc = 0;
                for (int j = 0; j < k; j++) acc += (REAL)Fm[i * k + j] * lb[j];
                tot += acc * fe[i];
            }
            REAL coef = (REAL)p->cat_prior[c];
            if (coef_mode == 1) coef *= (REAL)p->cat_rates[c] * (REAL)edge_rates_csr[idx];
            else if (coef_mode == 2) coef *= (REAL)p->cat_rates[c];
            w->acc[idx] += tot * coef;
        }
    }
    for (int e = 0; e < E; e++) out[e] = (double)(w->acc[e] / site_lhood);
}

/*
 * Likelihood with Q applied once on edge e1 and once on edge e2 (e1 == e2: twice; -1: not at all):
 * the down pass of src/evaluate_site_lhood.c with the substitutions that
 * evaluate_site_derivatives (src/arbplfhess.c:343-437) makes along the root paths.
 * Constant columns map to themselves under P and to 0 under Q (src/util.c:276-283, :338-345).
 */
static REAL SUF(site_lhood_q)(const orc_problem *p, SUF(site_ws) *w, int cat, int e1, int e2)
{
    int N = p->N, k = p->k;
    const PT *Pc = (const PT *)p->P + (size_t)cat * p->E * k * k;
    const PT *Q = (const PT *)p->Qn;
    for (int u = 0; u < N; u++) {
        int a = p->preorder[N - 1 - u];
        REAL *na = w->dnode + (size_t)a * k;
        for (int j = 0; j < k; j++) na[j] = w->base[(size_t)a * k + j];
        for (int idx = p->indptr[a]; idx < p->indptr[a + 1]; idx++) {
            int b = p->indices[idx];
            const PT *T = Pc + (size_t)idx * k * k;
            const REAL *nb = w->dnode + (size_t)b * k;
            REAL *ev = w->fedge, *ev2 = w->tmp;     /* scratch k-vectors */
            int constant = 1;
            for (int j = 1; j < k; j++) if (nb[j] != nb[0]) { constant = 0; break; }
            if (constant) { for (int i = 0; i < k; i++) ev[i] = nb[0]; }
            else for (int i = 0; i < k; i++) {
                REAL acc = 0;
                for (int j = 0; j < k; j++) acc += (REAL)T[i * k + j] * nb[j];
                ev[i] = acc;
            }
            int times = (idx == e1) + (idx == e2);
            for (int t = 0; t < times; t++) {
                constant = 1;
                for (int j = 1; j < k; j++) if (ev[j] != ev[0]) { constant = 0; break; }
                for (int i = 0; i < k; i++) {
                    REAL acc = 0;
                    if (!constant) for (int j = 0; j < k; j++) acc += (REAL)Q[i * k + j] * ev[j];
                    ev2[i] = acc;
                }
                for (int i = 0; i < k; i++) ev[i] = ev2[i];
            }
            for (int i = 0; i < k; i++) na[i] *= ev[i];
        }
    }
    return SUF(root_expect)(p, w->dnode + (size_t)p->preorder[0] * k);
}

/*
 * Hessian of the site log likelihood with respect to the edge rate coefficients, [E][E] in CSR
 * edge order: src/arbplfhess.c:503-760 (_recompute_second_order) with _lhood_hess_to_ll_hess
 * (:455-493).  Returns 0, or -1 when a category with a nonzero rate is infeasible (:629-648).
 */
static int SUF(site_hess)(const orc_problem *p, void *wsv, long s, REAL *H /* E*E */, REAL *g /* E */, double *out)
{
    SUF(site_ws) *w = wsv;
    int E = p->E;
    SUF(load_base)(p, w, s);
    for (int i = 0; i < E * E; i++) H[i] = 0;
    for (int i = 0; i < E; i++) g[i] = 0;
    REAL f = 0;
    for (int c = 0; c < p->C; c++) {
        REAL rc = (REAL)p->cat_rates[c], pc = (REAL)p->cat_prior[c];
        REAL lh = pc * SUF(site_lhood_q)(p, w, c, -1, -1);
        if (lh == 0) {
            if (rc == 0) continue;
            return -1;
        }
        f += lh;
        for (int i = 0; i < E; i++) {
            g[i] += SUF(site_lhood_q)(p, w, c, i, -1) * rc * pc;
            for (int j = 0; j <= i; j++)
                H[i * E + j] += SUF(site_lhood_q)(p, w, c, i, j) * rc * rc * pc;
        }
    }
    for (int i = 0; i < E; i++)
        for (int j = 0; j <= i; j++) {
            REAL v = (H[i * E + j] - g[i] * g[j] / f) / f;
            out[i * E + j] = out[j * E + i] = (double)v;
        }
    return 0;
}
