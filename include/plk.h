/*
 * plk.h -- C-ABI of the MI355X pruning-likelihood engine (libarbplf_amd.so).
 *
 * This is the device boundary of the drop-in: everything above it is host C
 * (model parsing, tree, rate mixtures, reductions, JSON), everything below it
 * is hand-written HIP for gfx950.  The entry points replace, one for one, the
 * pieces of the reference (argriffing/phyly, paths relative to its root) that
 * its three query drivers call between "model parsed" and "table written":
 *
 *   plk_set_tree        <- csr_graph_struct + navigation preorder
 *                          (src/csr_graph.h:17-24, src/model.h:62-67)
 *   plk_set_model       <- cross_site_ws_update: normalised Q, category
 *                          rates/priors, P[c][e] = exp(Q r_c t_e)
 *                          (src/cross_site_ws.c:151-168, :200-242)
 *   plk_set_patterns_*  <- pmat_struct observation likelihoods
 *                          (src/model.h:41-47, src/parsemodel.c:459-628)
 *   plk_ll              <- ll _nd_accum_update: site loop x category loop x
 *                          evaluate_site_lhood + log + site aggregation
 *                          (src/arbplfll.c:110-177, src/evaluate_site_lhood.c:7-63)
 *   plk_deriv           <- deriv _nd_accum_update + evaluate_site_derivatives
 *                          (src/arbplfderiv.c:112-371)
 *   plk_marginal        <- marginal _nd_accum_update + evaluate_site_forward +
 *                          evaluate_site_marginal_unnormalized
 *                          (src/arbplfmarginal.c:111-264)
 * and add what the reference does not have: plk_cat_posterior (rate-category posteriors), plk_edge_pair_sums and
 * plk_rate_matrix_sens (site-summed outer products per edge; the gradient of the log likelihood in the rate matrix),
 * plk_nni_ll (the log likelihood of every nearest-neighbour interchange of the tree from one down pass),
 * plk_place_ll (the log likelihood of the tree with a new taxon attached to every edge, for many new taxa at once).
 *
 * Conventions: every function returns 0 on success and a nonzero PLK_E_* code
 * on failure (plk_last_error() gives the text).  The caller owns all buffers
 * it passes; the engine owns its device memory.  Calls are synchronous.  One
 * engine may be used from one thread at a time; distinct engines are
 * independent (one per GPU / per process rank).  There is no CPU fallback: if
 * no gfx950 device is usable, plk_create fails.
 *
 * The engine keeps tables, matrix streams and work buffers from one call to the next and recomputes what a call made
 * stale.  None of that shows: every query gives the same bits whatever ran on the engine before it -- other queries,
 * changes of rates, model, patterns, weights, tree or options and back, a fit, a refused call -- as on a new engine that
 * was brought to the same tree, model, patterns, weights and options and ran nothing else (tests/test_gpu_query_order.py).
 *
 * Edge indices at this boundary are CSR edge indices (position in
 * `indices`), as in the reference's cross_site_ws; the host layer maps user
 * edge order <-> CSR order (src/csr_graph.c:29-46).
 */
#ifndef PLK_H
#define PLK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct plk_engine plk_engine;

enum {
    PLK_OK = 0,
    PLK_E_DEVICE = 1,    /* no usable GPU / HIP runtime error */
    PLK_E_ARG = 2,       /* invalid argument or call order */
    PLK_E_NOMEM = 3,     /* host or device allocation failed */
    PLK_E_UNSUPPORTED = 4
};

/* root prior modes, numbered as enum root_prior_mode in src/model.h:16-21 */
enum {
    PLK_ROOT_NONE = 1,        /* plain sum over root states */
    PLK_ROOT_CUSTOM = 2,      /* root_w = user distribution */
    PLK_ROOT_UNIFORM = 3,     /* 1/k */
    PLK_ROOT_EQUILIBRIUM = 4  /* root_w = stationary distribution */
};

/* where a caller buffer lives */
enum { PLK_HOST = 0, PLK_DEVICE = 1 };

/* Create an engine on HIP device `device` (0-based).  Fails loudly
 * (PLK_E_DEVICE) when the HIP runtime reports no device. */
int plk_create(plk_engine **out, int device);
void plk_destroy(plk_engine *h);
const char *plk_last_error(const plk_engine *h);
/* text for failures of plk_create itself (no engine yet) */
const char *plk_create_error(void);

/* Tree in CSR out-adjacency form; `preorder` is the BFS order from the root
 * (preorder[0] = root), all host arrays.  N nodes, E = N-1 edges. */
int plk_set_tree(plk_engine *h, int N, const int *indptr, const int *indices,
                 const int *preorder);

/* Model: k states, C rate categories.
 * Qn[k*k] row-major: rate matrix already divided by the rate divisor, with
 * its diagonal set to minus the row sums (src/cross_site_ws.c:217-232).
 * Qn_lo[k*k] (may be NULL = zeros): low-order words, Qn + Qn_lo being the
 * normalised matrix to ~106 bits; the reference normalises in exact ball
 * arithmetic, and d/dt exp(Qt) = Q exp(Qt) at long branches is only as accurate
 * as the zero row sums of Q (examples/JC.long.branch of the reference).
 * edge_rates_csr[E], cat_rates[C], cat_prior[C], root_w[k] (ignored for
 * NONE/UNIFORM).  Runs the device exp(Q r t) kernel for all (c, e). */
int plk_set_model(plk_engine *h, int k, int C, const double *Qn, const double *Qn_lo,
                  const double *edge_rates_csr,
                  const double *cat_rates, const double *cat_prior,
                  int root_mode, const double *root_w);

/* Recompute P for new edge rates only (branch-length optimisation loops). */
int plk_update_edge_rates(plk_engine *h, const double *edge_rates_csr);

/*
 * What plk_set_model and plk_update_edge_rates accept, on its own: host only, no engine and no GPU involved
 * (phyly_amd/csrc/plk_k1_check.h; E edge rates, otherwise the arguments of plk_set_model).  PLK_E_ARG for
 *   - any value that is not finite: Qn, Qn_lo, edge rates, category rates and priors, root_w where the root mode reads it;
 *   - a negative edge rate, category rate or category prior (-0.0 counts as zero);
 *   - any pair (c, e) with cat_rates[c] * edge_rates[e] * |Qn|_inf not finite or above 2^40 (|Qn|_inf: the largest
 *     absolute row sum).  The transition matrix kernel squares once per doubling of that number; each squaring can
 *     double the drift of the row sums, at most k 2^sq 2^-104, and 2^40 keeps it below 2^-53 at k = 64 (DESIGN.md
 *     section 6).  The reference, working in Arb, accepts such inputs; here about 1e12 expected substitutions on one
 *     edge is the documented limit.
 * plk_set_model, plk_update_edge_rates and every call that recomputes the transition matrices return PLK_E_ARG on the
 * same terms, the diagnostic (plk_last_error) naming the edge and the category; the engine then keeps its previous model
 * and rates and stays usable.  plk_get_frechet_matrices, plk_edge_expect(_multi) and their group forms return PLK_E_ARG
 * for a direction matrix with an entry that is not finite; plk_rate_matrix_sens for pair sums that are not finite.
 */
int plk_check_model_values(int k, int C, int E, const double *Qn, const double *Qn_lo, const double *edge_rates,
                           const double *cat_rates, const double *cat_prior, int root_mode, const double *root_w);

/* Observations, compact form: codes[N][S] (site index fastest, one byte per
 * node per site) + definitions defs[nchar][k] (host).  `where` says whether
 * `codes` is a host or a device pointer; the engine copies it either way.
 * New patterns (either form) drop the site weights of the previous ones: all weights are 1 until the next
 * plk_set_site_weights. */
int plk_set_patterns_codes(plk_engine *h, long S, const uint8_t *codes, int where,
                           int nchar, const double *defs);

/* Observations, dense form: B[N][k][S] doubles (site index fastest).  Drops the site weights, as the compact form does. */
int plk_set_patterns_dense(plk_engine *h, long S, const double *B, int where);

/* Optional per-site weights for the aggregated outputs (NULL = all 1): S doubles for the patterns the engine holds.
 * They last until the next plk_set_site_weights or the next plk_set_patterns_*, which drops them.
 * A weight of exactly 0 still evaluates the site; selection is the caller's.  In the sums of plk_ll, plk_deriv and
 * plk_marginal a weight of exactly 0 drops the site's term whatever the term is: a site of likelihood 0 (ll -inf,
 * derivatives and marginals inf or NaN) under weight 0 leaves those sums equal to the sums of the alignment without the
 * site.  plk_edge_expect(_multi), plk_hess and plk_second_order make no such promise: where one of their sums
 * multiplies the weight into a term that is not finite, that sum is NaN whatever the weight. */
int plk_set_site_weights(plk_engine *h, const double *w, int where);

/*
 * Log likelihoods.  site_ll_out: NULL or S doubles (host/device per `where`).
 * sum_out: NULL or 2 doubles {hi, lo}: sum_s w_s * ll_s as an unevaluated
 * double-double (hi + lo), summed in a fixed order (deterministic).  A site of weight exactly 0 adds nothing to the
 * sum, also where its ll is -inf (likelihood 0).
 */
int plk_ll(plk_engine *h, double *site_ll_out, int where, double *sum_out);

/*
 * The same evaluation queued on the engine's stream without waiting for it (optimisation loops, several GPUs):
 * site_ll_dev (NULL or S doubles) and sum_dev (NULL or 2 doubles {hi, lo}) are DEVICE buffers of the caller; nothing is
 * copied to the host.  plk_sync() -- or any synchronous call on the engine -- waits for the queued work.
 * plk_set_stream() makes the engine issue its work on a HIP stream of the caller (hipStream_t passed as void *; NULL =
 * the engine's own stream again), so that the caller's collectives and events are ordered with the engine's kernels.
 */
int plk_ll_async(plk_engine *h, double *site_ll_dev, double *sum_dev);
int plk_sync(plk_engine *h);
int plk_set_stream(plk_engine *h, void *hip_stream);

/*
 * Edge-rate derivatives d ll_s / d edge_rate_coefficient_e (CSR edge order).
 * edge_mask: NULL (all) or E ints, nonzero = requested.
 * site_edge_out: NULL or [S][E] doubles, host; unrequested edges get 0.
 * edge_sums_out: NULL or [E][2] double-double sums of w_s * d_{s,e}; a site of weight exactly 0 adds nothing, also
 * where its derivatives are not finite (likelihood 0).
 *
 * Nodes with many factors: plk_deriv, plk_marginal, plk_edge_expect(_multi), plk_edge_pair_sums, plk_rate_matrix_sens,
 * plk_mixture_sens, plk_nni_ll, plk_place_ll, plk_second_order and plk_hess keep one rescaling factor per node.  On a tree with a node that takes
 * more than 32 edge factors at once (33 leaf children, or three children over 16 edges each) they first measure the
 * node products on the device; where one has no entry of at least 2^-969 at some site they return PLK_E_ARG, the
 * diagnostic naming the query and the node, and the engine stays usable.  With ordinary branch lengths nothing is refused.
 * A product that is exactly 0 because every entry took a factor of exactly 0 (the rate-0 category under children that show
 * different states) has not left the range and is not refused.
 * plk_ll and plk_cat_posterior rescale inside such a node and always answer.
 */
int plk_deriv(plk_engine *h, const int *edge_mask,
              double *site_edge_out, double *edge_sums_out);

/*
 * Marginal state distributions.  node_mask: NULL (all) or N ints.
 * site_out: NULL or [S][N][k] doubles, host (unrequested nodes get 0).
 * sums_out: NULL or [N][k][2] double-double sums over sites of w_s * m_{s,a,i}; a site of weight exactly 0 adds
 * nothing, also where its marginals are not finite (likelihood 0), whether or not site_out is asked for.
 */
int plk_marginal(plk_engine *h, const int *node_mask,
                 double *site_out, double *sums_out);

/*
 * Rate-category posteriors and posterior mean site rates (empirical Bayes; the reference has no such query).
 * With L_{s,c} the site likelihood under category c alone (root prior included), in the category order of plk_set_model:
 *     post[s][c] = cat_prior_c L_{s,c} / sum_c' cat_prior_c' L_{s,c'}        rate[s] = sum_c post[s][c] cat_rates[c]
 * One traversal for all categories (plk_catpost.h).  post_out: NULL or [S][C] host; rate_out: NULL or [S] host;
 * post_sums_out: NULL or [C][2]; rate_sum_out: NULL or [2]: double-double sums over sites of w_s post[s][c] and
 * w_s rate[s].  A category of prior 0 has posterior exactly 0.  A site of likelihood 0 gets NaN in post and rate (-inf in
 * site_ll); when sums are asked for and such a site has a non-zero weight the call fails with PLK_E_ARG ("site likelihood
 * zero").
 * plk_cat_posterior_ll is the same call with the by-products: site_ll_out NULL or [S] host, ll_sum_out NULL or [2].
 */
int plk_cat_posterior(plk_engine *h, double *post_out, double *rate_out, double *post_sums_out, double *rate_sum_out);
int plk_cat_posterior_ll(plk_engine *h, double *post_out, double *rate_out, double *site_ll_out,
                         double *post_sums_out, double *rate_sum_out, double *ll_sum_out);

/*
 * Conditional edge expectations: the shared core of arbplf-dwell, arbplf-trans
 * and arbplf-em-update.  For a direction matrix L (k x k, given as
 * an unevaluated sum L_hi + L_lo; L_lo may be NULL) the engine forms, per category c
 * and edge e, the Frechet derivative of the matrix exponential
 *     F_{c,e} = int_0^1 exp(s Qn u) L exp(s Qn (1-u)) du,   s = cat_rate_c * edge_rate_e
 * (the top-right block of exp([[s Qn, L], [0, s Qn]]), src/util.c:501-548) and returns
 *     x_{s,e} = sum_c prior_c * coef_{c,e} * fe_{c,e}^T F_{c,e} L_{c,b} / lhood_s
 * (src/evaluate_site_frechet.c:5-42 and the category loops of src/arbplfdwell.c:205-300,
 * src/arbplftrans.c:233-330, src/arbplfem.c:258-390), with coef_{c,e} =
 *   PLK_COEF_PRIOR            1                         (dwell: L = e_s e_s^T or diag(weights))
 *   PLK_COEF_PRIOR_RATE_EDGE  cat_rate_c * edge_rate_e  (trans: L = weights o Qn)
 *   PLK_COEF_PRIOR_RATE       cat_rate_c                (em-update numerators / denominators)
 * Outputs as for plk_deriv (CSR edge order, unrequested edges 0).
 */
enum { PLK_COEF_PRIOR = 0, PLK_COEF_PRIOR_RATE_EDGE = 1, PLK_COEF_PRIOR_RATE = 2 };
int plk_edge_expect(plk_engine *h, const double *L_hi, const double *L_lo, int coef_mode,
                    const int *edge_mask, double *site_edge_out, double *edge_sums_out);
/* nL direction matrices in one call (L_hi / L_lo: [nL][k][k]); site_out: NULL or [S][nL][E], sums_out: NULL or
 * [nL][E][2].  The k = 4 kernels evaluate up to four directions per pass (shared down pass and forward vectors):
 * em-update's two expectations, dwell per state, trans per state pair. */
int plk_edge_expect_multi(plk_engine *h, int nL, const double *L_hi, const double *L_lo, int coef_mode,
                          const int *edge_mask, double *site_out, double *sums_out);
/*
 * Edge pair sums (the reference has no such query).  For every category c and edge e = (a -> b), with fe the vector above
 * the edge (forward vector of a, its observation and the messages of b's siblings) and L_b the vector below it:
 *     W[c][e][i][j] = sum_s w_s prior_c fe_{s,c,e}[i] L_{s,c,b}[j] / lhood_s
 *     R[c][i]       = sum_s w_s prior_c (B_root o messages)_{s,c}[i] / lhood_s        (root vector without the root prior)
 * Every site-summed edge form is a contraction of W: sum_s w_s x_{s,e} = sum_c <W[c][e], M_{c,e}> for dP or a scaled
 * Frechet matrix M, and <W[c][e], P[c][e]> = sum_s w_s post_{s,c} on every edge.  One down pass and one up pass
 * (plk_pairsums.h); the partial sums live on a fixed grid, so their storage does not depend on S, and the order of every
 * sum is fixed (two calls give the same bits).  Preconditions as for plk_deriv; edge_mask: NULL (all) or E ints.
 * W_out: [C][E][k][k][2] double-double entries in CSR edge order, masked edges exactly 0; root_out: NULL or [C][k][2].
 * A site of likelihood 0 with a non-zero weight makes the call fail with PLK_E_ARG ("site likelihood zero"); with weight
 * 0 it contributes nothing.
 */
int plk_edge_pair_sums(plk_engine *h, const int *edge_mask, double *W_out, double *root_out);

/*
 * Gradient of sum_s w_s ll_s in the normalised rate matrix, all k^2 entries taken as independent:
 *     G[i][j] = d/dQn[i][j] = sum_{c,e} s (F_{c,e}(W[c][e]^T))^T,   s = cat_rate_c * edge_rate_e
 * (F the Frechet matrix of plk_edge_expect; the adjoint identity <W, F(L)> = <L, F(W^T)^T> turns k^2 directions into one
 * per (category, edge)), and root_out[i] = d/droot_w[i] = sum_c R[c][i].  One down pass, one up pass, one Frechet K1 run.
 * G_out: [k][k][2], root_out: NULL or [k][2], double-double.  plk_rate_matrix_chain takes both to the user's parameters.
 */
int plk_rate_matrix_sens(plk_engine *h, double *G_out, double *root_out);

/*
 * The chain rule from (G, root) of plk_rate_matrix_sens to the raw off-diagonal entries q_ij of the user's rate_matrix;
 * host only, no engine and no GPU involved, IEEE binary128 rounded once.  The diagonal of rate_matrix is ignored (it is
 * minus the row sums, as at parse time).  With d the divisor, Qn = Q / d, pi the stationary distribution and
 * Z = (1 pi^T - Q)^-1:
 *   fixed divisor           d/dq_ij = (G_ij - G_ii) / d
 *   PLK_DIVISOR_EXIT_RATE   d = sum_m pi_m sum_{n != m} q_mn; adds (df/dd)(dd/dq_ij) with df/dd = -(1/d) sum_mn G_mn Qn_mn,
 *                           dd/dq_ij = pi_i + sum_m (dpi_m/dq_ij)(-Q_mm),  dpi/dq_ij = pi_i (e_j - e_i)^T Z
 *   PLK_ROOT_EQUILIBRIUM    adds sum_m root_m dpi_m/dq_ij (custom, uniform and no root prior do not depend on Q)
 * rate_matrix: [k][k]; divisor: the number (ignored for PLK_DIVISOR_EXIT_RATE); G: [k][k][2]; root: [k][2], NULL unless
 * root_mode is PLK_ROOT_EQUILIBRIUM; grad_out: [k][k], diagonal 0.  err / errlen: NULL / 0 or a buffer for the diagnostic.
 * Returns PLK_E_ARG for bad arguments and for a reducible rate matrix when pi is needed ("rate matrix is reducible").
 */
enum { PLK_DIVISOR_NUMBER = 0, PLK_DIVISOR_EXIT_RATE = 1 };
int plk_rate_matrix_chain(int k, const double *rate_matrix, int divisor_mode, double divisor, int root_mode,
                          const double *G, const double *root, double *grad_out, char *err, size_t errlen);

/*
 * Gradient of sum_s w_s ll_s in the parameters of the rate mixture, priors and rates taken as independent (the reference
 * has no such query).  With L_{s,c} the site likelihood under category c alone (root prior included), lhood_s = sum_c p_c L_{s,c}:
 *     prior_out[c] = d/dp_c = sum_s w_s L_{s,c} / lhood_s                 (no factor p_c: right for a category of prior 0)
 *     rate_out[c]  = d/dr_c = sum_e t_e sum_s w_s p_c fe_{s,c,e}^T (Qn P_{c,e}) L_{s,c,b} / lhood_s      (at fixed Qn)
 * The direction matrices t_e Qn P_{c,e} are built as such (not as dP / r_c), so rate_out is right at r_c = 0, the
 * invariable category, where P = I; edges of rate 0 contribute nothing.  One down pass and one up pass that keeps its
 * 2 C numbers in registers and writes no per-site plane (plk_mixsens.h); fixed grid and fixed order of every sum as for
 * plk_edge_pair_sums, whose preconditions and zero-likelihood behaviour apply (PLK_E_ARG, "site likelihood zero").
 * prior_out, rate_out: [C][2] double-double.  Identities: sum_c p_c prior_out[c] = sum_s w_s;
 * sum_c r_c rate_out[c] = sum_e t_e (edge sums of plk_deriv); p_c prior_out[c] = post_sums[c] of plk_cat_posterior.
 */
int plk_mixture_sens(plk_engine *h, double *prior_out, double *rate_out);

/*
 * The chain rule from (prior_out, rate_out) of plk_mixture_sens to the user's rate-mixture parameters, following the map
 * of the model preparation (host_k0.c); host only, IEEE binary128 rounded once.  mode: the rate mixture as numbered in
 * host_k0.h (2 custom with array prior, 3 custom with uniform prior, 4 gamma, 5 median gamma); n: custom: the number of
 * categories, gamma: gamma_categories; rates / prior: the custom arrays (prior NULL for mode 3; both ignored for gamma).
 *   custom, fixed divisor     d/drates[c] = rate_out[c], d/dprior[c] = prior_out[c]
 *   custom, exit-rate divisor the divisor carries expect = sum_c r_c p_c; with T = sum_c r_c rate_out[c] (Euler: scaling
 *                             Qn equals scaling every rate) d/drates[c] = rate_out[c] - p_c T / expect,
 *                             d/dprior[c] = prior_out[c] - r_c T / expect; expect = 0 is refused
 *   uniform prior             rates only, p_c = 1 / n, same divisor term
 *   gamma (+I)                r_j = g_j(shape) / (1 - pi), p_j = (1 - pi) / n, last category r = 0, p = pi; expect = 1:
 *                             d/dshape = sum_j rate_out[j] g_j'(shape) / (1 - pi),
 *                             d/dpi = sum_j rate_out[j] r_j / (1 - pi) - (1/n) sum_j prior_out[j] + prior_out[n]
 *                             (only when invariable_prior != 0: without an invariable category nothing is reported for it)
 * prior_sens / rate_sens: [C][2] with C = n (+ 1 for gamma with invariable_prior != 0).
 * drates_out: [n] (custom) ; dprior_out: [n] (mode 2) ; dshape_out, dinvariable_out: one double each (gamma).  Outputs that
 * do not apply to the mode may be NULL and are left alone; *has_invariable_out (may be NULL) is 1 when dinvariable_out was
 * written.  err / errlen as for plk_rate_matrix_chain.  Returns PLK_E_ARG for bad arguments, no mixture, expect = 0.
 */
int plk_mixture_chain(int mode, int n, const double *rates, const double *prior, double gamma_shape, double invariable_prior,
                      int divisor_mode, const double *prior_sens, const double *rate_sens,
                      double *drates_out, double *dprior_out, double *dshape_out, double *dinvariable_out,
                      int *has_invariable_out, char *err, size_t errlen);

/*
 * Nearest-neighbour interchanges (the reference has no such query).  The tree is rooted and directed as everywhere here.
 * A swap is a pair of CSR edges (a, b) with a = (v -> c), b = (u -> s), v a child of u and s != v.  The swapped tree has
 * a = (u -> c) and b = (v -> s): the two subtrees exchange parents; each edge keeps its index, its rate coefficient and
 * the subtree below it; data on u, v and every other node stay where they are; every node keeps its number of children.
 * Multifurcations, unary nodes, leaves as c or s and the root as u are all allowed; a leaf v has no swap.
 *
 * plk_nni_swaps: host only, no engine and no GPU involved.  Returns the number of swaps of the tree (0 for arrays that are
 * no tree) and, when pairs_out is not NULL, fills the canonical list [count][2], ordered by a, then by b.
 *
 * plk_nni_ll: the log likelihood ll'_s of every site under every listed swapped tree, from the vectors of ONE down pass
 * over the current tree and one up pass per 256 swaps (plk_nni.h): a swap costs a handful of k x k products at u and v,
 * whatever the size of the tree.  swaps: [n_swaps][2] CSR edge pairs; NULL = the canonical list, n_swaps being its length.
 * Repeated pairs are allowed, and a pair has the same bits wherever it stands in whatever list.  site_out: NULL or
 * [n_swaps][S] host; sums_out: NULL or [n_swaps][2] double-double sums of w_s ll'_s, summed in a fixed order.
 * Nothing is divided by the likelihood of the current tree: a swapped tree may have positive likelihood where the current
 * one has none, and the other way round.  A site of likelihood 0 under the swapped tree has ll' = -inf; in the sums it
 * behaves as in plk_ll (weight exactly 0: it adds nothing; otherwise the sum is not finite).
 * PLK_E_ARG, the diagnostic naming the pair, for a pair that is no swap (the same edge twice, s = v, edges further apart,
 * reversed order, an index out of range); nothing has run then and the engine stays usable.  Preconditions as for
 * plk_deriv (nodes with more than 32 factors: the same range check and refusal).  Which tree the engine holds does not
 * change.  PLK_INFO_NNI_KERNEL, PLK_INFO_DOWN4_KERNEL and PLK_INFO_LAST_QUERY_NS report on the call.
 */
int plk_nni_swaps(int N, const int *indptr, const int *indices, int *pairs_out /* NULL or [count][2] */);
int plk_nni_ll(plk_engine *h, int n_swaps, const int *swaps, double *site_out, double *sums_out);

/*
 * Placements (the reference has no such query): the log likelihood of the current tree with a new taxon attached to an
 * edge, for every listed edge and every query taxon, from the vectors of ONE down pass over the current tree and one up
 * pass per 256 (query, edge) rows (plk_place.h).  A placement onto the CSR edge e = (u -> b) with rate coefficient r_e
 * replaces e by three edges: (u -> m) with rate fl(split r_e), (m -> b) with rate fl(fl(1 - split) r_e) and (m -> q) with
 * rate pendant_rate; m is a new node without data, q a new leaf with the query's observation.  Every other edge, node and
 * datum, the root and the root prior stay.  What does not depend on the query is computed once per (edge, category, site)
 * and shared by every query of that edge in the pass.
 * q_codes: [n_queries][S] host, character codes into the definitions of plk_set_patterns_codes, for an engine that holds
 * compact patterns (else NULL); q_dense: [n_queries][k][S] host for an engine that holds dense patterns (else NULL).
 * edges: [n_edges] CSR edge indices, repeats allowed; NULL = every edge in CSR order, n_edges being E.  A row has the
 * same bits wherever it stands in whatever list, alone or with others, in one site chunk or several.
 * site_out: NULL or [n_queries][n_edges][S] host; sums_out: NULL or [n_queries][n_edges][2] double-double sums of
 * w_s ll'_s, summed in a fixed order; with both NULL the arguments are checked and nothing runs.
 * Nothing is divided by the likelihood of the current tree.  A placement of likelihood 0 at a site has ll' = -inf there; in the sums it behaves as in plk_ll (weight exactly 0: it adds nothing; otherwise the
 * sum is not finite).  An all-missing query (a constant observation row) reproduces the log likelihood of the current tree.
 * PLK_E_ARG, the diagnostic naming the argument: tree, model or patterns not set; neither or both query arrays, or the
 * form the engine does not hold; a code >= nchar; a dense entry negative or not finite; an edge index out of range; split
 * outside [0, 1] or not finite; pendant_rate negative or not finite; a rate the transition matrix kernel refuses
 * (plk_check_model_values; the diagnostic names the edge and the upper part, the lower part or the pendant edge).
 * Nothing has run then and the engine stays usable.  Preconditions as for plk_deriv (nodes with more than 32 factors: the
 * same range check and refusal).  The transition matrices of the three new edges live in buffers of the call's own: the
 * engine's matrices, tables and rates do not change, and the call is invisible to every later query.
 * PLK_INFO_PLACE_KERNEL, PLK_INFO_DOWN4_KERNEL and PLK_INFO_LAST_QUERY_NS report on the call.
 */
int plk_place_ll(plk_engine *h, int n_queries, const uint8_t *q_codes, const double *q_dense, int n_edges, const int *edges,
                 double split, double pendant_rate, double *site_out, double *sums_out);

/*
 * Subtree prune-and-regraft moves (the reference has no such query).  The tree is rooted and directed as everywhere here.
 * A move is a pair of CSR edges (p, e), p = (w -> x) the pruned edge and e = (u -> b) the target, e neither p nor an edge
 * of the subtree below x.  In the moved tree e is replaced by (u -> m) with rate fl(split r_e) and (m -> b) with rate
 * fl(fl(1 - split) r_e), exactly as plk_place_ll rounds them; p becomes (m -> x) and keeps its index, its rate r_p and the
 * whole subtree below x; m is a new node without data; w stays where it is with one child fewer (it may become unary, or a
 * leaf whose vector is its own observation row, constant if it has no data) and keeps its data.  Every other node, datum
 * and edge, the root and the root prior stay.  Multifurcations, unary nodes, data on internal nodes, a leaf as x, the root
 * as w or u, a sibling edge of p (u = w) and the edge into w as the target are all allowed.  For a w with two children and
 * no data the value equals, mathematically, the usual SPR in which the two edges at w merge.  A move with split = 0 onto
 * a sibling edge of p gives the log likelihood of the current tree; a move whose x is a leaf equals the placement of that
 * leaf's observations onto e in the tree without the leaf, with pendant_rate = r_p.
 *
 * plk_spr_moves: host only, no engine and no GPU involved.  Returns the number of moves of the tree (0 for arrays that are
 * no tree) and, when pairs_out is not NULL, fills the canonical list [count][2], ordered by p, then by e: every (p, e) with
 * e outside {p} and the edges below x.
 *
 * plk_spr_ll: the log likelihood ll'_s of every site under every listed moved tree, from the vectors of ONE down pass per
 * site chunk over the current tree; per prune edge one pass recomputes the vectors of the tree without the pruned subtree
 * (the down vectors on the path from w to the root and the forward vectors outside the subtree of x), and one pass per 256
 * moves of that edge ends them as placements whose pendant vector is the message the pruned subtree sends today
 * (plk_spr.h).  moves: [n_moves][2] CSR edge pairs (p, e); NULL = the canonical list, n_moves being its length.  Repeated
 * moves are allowed, and a move has the same bits wherever it stands in whatever list, alone or with others, in one site
 * chunk or several.  site_out: NULL or [n_moves][S] host; sums_out: NULL or [n_moves][2] double-double sums of w_s ll'_s,
 * summed in a fixed order; with both NULL the arguments are checked and nothing runs.  Nothing is divided by the likelihood
 * of the current tree.  A site of likelihood 0 under the moved tree has ll' = -inf; in the sums it behaves as in plk_ll
 * (weight exactly 0: it adds nothing; otherwise the sum is not finite).
 * PLK_E_ARG, the diagnostic naming the pair or the argument: tree, model or patterns not set; an index out of range;
 * e == p; e below x; split outside [0, 1] or not finite; a rate the transition matrix kernel refuses
 * (plk_check_model_values).  Nothing has run then and the engine stays usable.  Preconditions as for plk_deriv (nodes with
 * more than 32 factors: the same range check and refusal).  The transition matrices of the split target edges live in
 * buffers of the call's own: the engine's tree, matrices, tables, rates and dirty flags do not change, and the call is
 * invisible to every later query.  PLK_INFO_SPR_KERNEL, PLK_INFO_DOWN4_KERNEL and PLK_INFO_LAST_QUERY_NS report on the call.
 */
int plk_spr_moves(int N, const int *indptr, const int *indices, int *pairs_out /* NULL or [count][2] */);
int plk_spr_ll(plk_engine *h, int n_moves, const int *moves /* [n_moves][2] (p, e), NULL = canonical list */,
               double split, double *site_out /* NULL or [n_moves][S] host */, double *sums_out /* NULL or [n_moves][2] */);

/* the scaled Frechet matrices coef_{c,e} * F_{c,e} themselves, [C][E][k][k] host (tests) */
int plk_get_frechet_matrices(plk_engine *h, const double *L_hi, const double *L_lo, int coef_mode,
                             double *F_out);

/*
 * Fit the edge rate coefficients by maximum likelihood with the patterns, weights and tree resident on the
 * device.  The reference has no driver for this: its old-examples/opt.py and
 * old-examples/gell_dna_opt.py drive scipy's L-BFGS-B with arbplf_ll / arbplf_deriv through the Python API,
 * and test_scripts/test_em_monotonicity.py:95-130 iterates arbplf_em_update; this entry point is that loop.
 * method PLK_FIT_EM: r_e <- r_e * E[transitions on e] / E[rate-weighted dwell on e] (src/arbplfem.c:397-503);
 * method PLK_FIT_LBFGS: L-BFGS on log r_e, gradient from the deriv pass.  Edges with rate 0 or outside
 * edge_mask stay fixed.  Stops after max_iter iterations or when the gain in the weighted log likelihood is
 * <= ftol * max(1, |ll|).  rates_inout: E doubles, CSR order (also left set in the engine);
 * ll_trace: NULL or max_iter + 1 doubles (ll before the first and after every iteration).
 */
enum { PLK_FIT_EM = 0, PLK_FIT_LBFGS = 1 };
int plk_fit_edge_rates(plk_engine *h, int method, int max_iter, double ftol, const int *edge_mask,
                       double *rates_inout, double *ll_trace, int *iters_out, long *evals_out);

/*
 * Hessian of sum_s w_s ll_s with respect to the edge rate coefficients (SURVEY.md 8f-4, fp64 and
 * uncertified): replaces _recompute_second_order of src/arbplfhess.c:503-760 with its helpers
 * evaluate_site_derivatives (:343-437) and _lhood_hess_to_ll_hess (:455-493).
 * hess_sums_out: [E][E][2] double-double entries, CSR edge order, symmetric.
 */
int plk_hess(plk_engine *h, double *hess_sums_out);

/*
 * Gradient and Hessian of sum_s w_s ll_s from ONE run: pass 0 of the Hessian produces g / f per site anyway, so a
 * Newton step (src/arbplfhess.c:169-234) does not pay a separate plk_deriv.  grad_sums_out: NULL or [E][2], hess_sums_out:
 * NULL or [E][E][2] (not both NULL), double-double entries in CSR edge order.  plk_hess(h, out) is
 * plk_second_order(h, NULL, out).  k = 4 with compact codes and at most 4 rate categories runs the one-thread-per-site
 * second-order pass (plk_hess4.h: four edge-modified models per launch, two or one for the last rows), everything else the generic passes.
 */
int plk_second_order(plk_engine *h, double *grad_sums_out, double *hess_sums_out);

/*
 * The solve behind arbplf-inv-hess / -newton-delta / -newton-update; host only, no engine and no GPU involved.
 * hess: [E][E][2] and grad: [E][2] (NULL unless delta_out is asked for) as (hi, lo) pairs, any consistent edge order.
 * inv_out: NULL or [E][E] = H^-1, symmetrised; delta_out: NULL or [E] = -H^-1 g; cond_out: NULL or the infinity-norm
 * condition number ||H|| ||H^-1|| from the computed inverse.  Gauss-Jordan elimination with partial pivoting on [H | I] in
 * IEEE binary128, rounded once.
 * Returns PLK_E_ARG -- nothing but *cond_out written -- for a zero pivot and when cond * E * 1e-11 >= 1: the Hessian is
 * good to 1e-11 of its largest entry, so no digit of such a solve means anything (the reference's precision loop does
 * not terminate on a singular Hessian, src/arbplfhess.c:1225-1236).
 */
int plk_solve_second_order(int E, const double *hess, const double *grad, double *inv_out, double *delta_out, double *cond_out);

/*
 * One process per GPU: the reduction step of the site-sharded path on RCCL, issued from the engine.
 * Sites are independent given (tree, Q, rates); every rank evaluates its block of site patterns and the only exchange
 * is the sum of the aggregated outputs (src/ndaccum.c:198-254 is the reference's only cross-site step): 2 doubles for
 * ll, 2E for edge gradients, 2Nk for site-summed marginals, always {hi, lo} words.  The engine loads the RCCL the
 * process already has (librccl.so.1; no link-time dependency) and queues ncclAllReduce on its own stream, behind the
 * kernels that produce the sums -- no framework call per step.
 *   plk_comm_unique_id   rank 0 makes the 128-byte id; the caller hands it to the other ranks (torch.distributed, MPI, a file)
 *   plk_comm_init        collective: every rank calls it with the same id
 *   plk_allreduce_sum_async  in-place sum over ranks of `count` doubles in DEVICE memory, queued on the engine's stream
 */
int plk_comm_available(void);                 /* 1 when RCCL can be loaded in this process (local, not a collective) */
int plk_comm_unique_id(unsigned char id_out[128]);
int plk_comm_init(plk_engine *h, int nranks, int rank, const unsigned char id[128]);
int plk_allreduce_sum_async(plk_engine *h, double *dev, long count);
int plk_comm_destroy(plk_engine *h);

/* Introspection for tests and profiling. */
int plk_get_transition_matrices(plk_engine *h, double *P_out /* [C][E][k][k] host */);
int plk_get_info(plk_engine *h, int what, long *out);
enum {
    PLK_INFO_LL_KERNEL = 0,       /* 0 = none yet, 1 = fused register-stack (k=4), 2 = generic vector, 3 = fp64 MFMA,
                                     4 = register-resident vector kernel (9 <= k <= 32) */
    PLK_INFO_STACK_SLOTS = 1,     /* register-stack slots the tree needs */
    PLK_INFO_PROGRAM_OPS = 2,     /* ops in the traversal program */
    PLK_INFO_LAST_LL_KERNEL_NS = 3, /* HIP-event time of the last ll traversal kernel */
    PLK_INFO_LAST_LL_TOTAL_NS = 4,  /* HIP-event time of the last whole plk_ll device work */
    PLK_INFO_LL_KERNEL_NS_SUM = 5,  /* HIP-event time of the traversal kernels of all ll evaluations since this item was */
    PLK_INFO_LL_KERNEL_COUNT = 6,   /* last read, and their number (reading waits for queued evaluations, then resets) */
    PLK_INFO_LL_VARIANT = 7,        /* k = 4 tile kernel of the last evaluation: 1 assembly interpreter, 3 C++ interpreter,
                                       5 assembly interpreter with pair tables, 6 the same with two sites per lane, 0 another kernel */
    PLK_INFO_PAIR_TABLES = 8,       /* two-leaf subtrees the last k = 4 evaluation read from tables */
    PLK_INFO_LL_EXEC_FLOPS = 9,     /* fp64 flops per site the last ll traversal kernel executed (all categories): 2k^2 - k per
                                       matrix-vector product it ran (k padded to 16 rows on the matrix cores), k per elementwise
                                       multiply (leaf rows, stack pops); table look-ups, moves and rescaling count nothing */
    PLK_INFO_UPDOWN_KERNEL = 10,    /* down / up kernels of the last deriv, marginal, expectation or second-order query: 0 = none
                                       yet, 1 = k = 4 kernels, 2 = generic, 3 = fp64 MFMA, 4 = register-resident vector
                                       (9 <= k <= 20), 5 = k = 4 second-order pass (after plk_hess / plk_second_order) */
    PLK_INFO_CAT_POSTERIOR_KERNEL = 11, /* kernel of the last plk_cat_posterior: 0 = none yet, 1 = k = 4 register kernel
                                       (compact codes, at most 8 categories), 2 = generic */
    PLK_INFO_CATEGORIES = 12,       /* rate categories of the model (0 before plk_set_model) */
    PLK_INFO_LAST_CAT_POSTERIOR_NS = 13, /* HIP-event time of the device work of the last plk_cat_posterior (K1 when the rates
                                       changed, tables, kernel, sums); for tools/time_cat_posterior.py */
    PLK_INFO_PAIR_SUMS_KERNEL = 14, /* up pass of the last plk_edge_pair_sums / plk_rate_matrix_sens: 0 = none yet, 1 = the k = 4
                                       kernel (compact codes, at most 4 categories), 2 = generic */
    PLK_INFO_LAST_QUERY_NS = 15,    /* HIP-event time from the first to the last device operation of the last plk_deriv,
                                       plk_edge_expect(_multi), plk_edge_pair_sums, plk_rate_matrix_sens, plk_mixture_sens, plk_nni_ll, plk_place_ll or plk_spr_ll
                                       (0 when it could not be taken); for tools/time_rate_matrix_deriv.py and
                                       tools/time_mixture_deriv.py */
    PLK_INFO_MIXTURE_SENS_KERNEL = 16, /* up pass of the last plk_mixture_sens: 0 = none yet, 1 = the k = 4 kernel (compact
                                       codes, at most 4 categories), 2 = generic */
    PLK_INFO_UP4_PATH = 17,         /* k = 4 up pass of the last deriv, marginal or expectation query, a bit mask: 1 = node-visit
                                       pass (k_up4_nodes; otherwise k_up4), 2 = with pair messages (at least one two-leaf node
                                       read from a table), 4 = with rebuilt tables (at least one node whose vector is the
                                       product of two table rows), 8 = two-leaf nodes finished inside their parent's visit
                                       (one rate category); 0 when another kernel family ran */
    PLK_INFO_DOWN4_KERNEL = 18,     /* k = 4 down pass of the last query that ran on the k = 4 up/down kernels (deriv, marginal,
                                       expectations, and the pair-sum, mixture-gradient, swap, placement and prune-and-regraft passes): 4, 8 or 16 = k_down_fused4<D>
                                       with a register stack of that depth, 0 = k_down_store4 (the staged code rows do not fit
                                       the LDS, or the tree needs more than 16 slots) or no such query yet */
    PLK_INFO_LL_FORM = 19,          /* form of the last ll evaluation's k = 4 pair-table kernel: 1 = streamed codes with the tables
                                       of all categories resident in LDS (k_ll_fused4_v4s; PLK_INFO_LL_VARIANT reports 6),
                                       0 = a tile kernel or another family */
    PLK_INFO_LL_PAIRMUL = 21,       /* pair products in the last ll evaluation's streamed kernel: 0 = the form did not run (another
                                       kernel, a tree that needs 4 stack slots, PLK_OPT_PAIR_TABLES + 64 / + 128 / + 256 / + 512, or
                                       a stream that did not replay), else bit 0 = k_ll_fused4_v4s<768, true, true> ran its op stream and bits 8-23 =
                                       PAIR ops of one category (two table rows multiplied under one dispatch, saturating; can be 0) */
    PLK_INFO_LL_FOLD = 20,          /* op stream of the last ll evaluation's streamed kernel (0 for every other kernel), bit fields:
                                       bit 0 = the folded op stream ran, bit 1 = the first chunks of a unit were held across the
                                       categories, bits 4-7 = stack slots d whose MATVEC + POPMUL + SCALE handler the stream
                                       dispatches, bits 8-15 = SCALE ops left with a dispatch of their own, bits 16-23 / 24-30 =
                                       observation ops of one category with ADVANCE_0 / ADVANCE_1 folded in (saturating).  Under
                                       the pair-product form (PLK_INFO_LL_PAIRMUL) bits 0 and 4-30 describe the folded stream it was
                                       derived next to: a PAIR op with an ADVANCE counts as the observation op that carried it */
    PLK_INFO_NNI_KERNEL = 22,       /* up pass of the last plk_nni_ll: 0 = none yet, 1 = the k = 4 kernel (compact codes, at most
                                       4 categories), 2 = generic */
    PLK_INFO_LL_QUAD = 24,          /* four-leaf tables in the last ll evaluation's streamed kernel: 0 = the form did not run (as for
                                       PLK_INFO_LL_TRIPLE; also: a leaf with more than 4 occurring codes under every node that
                                       would qualify, PLK_OPT_PAIR_TABLES + 32768, or + 1024 without + 16384), else bit 0 = it ran
                                       and bits 8-23 = nodes of a category that are look-ups of a four-leaf table.
                                       PLK_INFO_LL_TRIPLE then reports the groups and the three-leaf tables beside them */
    PLK_INFO_LL_TRIPLE = 23,        /* three-leaf tables in the last ll evaluation's streamed kernel: 0 = the form did not run (another
                                       kernel, no node that qualifies, too few sites for the default, PLK_OPT_PAIR_TABLES + 2048, or
                                       formats that did not replay), else bit 0 = it ran, bits 4-7 = groups the categories ran in
                                       (phases of the one launch), bits 8-23 = nodes of a category that are look-ups of a
                                       three-leaf table (a cherry, a leaf and the edge above their parent in one row).
                                       PLK_INFO_PAIR_TABLES then counts the cherries that still have a table of their own, and
                                       PLK_INFO_LL_EXEC_FLOPS the stream that ran */
    PLK_INFO_PLACE_KERNEL = 25,     /* up pass of the last plk_place_ll: 0 = none yet, 1 = the k = 4 kernel (compact codes, at most
                                       4 categories), 2 = generic */
    PLK_INFO_SPR_KERNEL = 27,       /* up pass of the last plk_spr_ll: 0 = none yet, 1 = the k = 4 kernel (compact codes, at most
                                       4 categories), 2 = generic */
    PLK_INFO_LL_BARRIER = 26        /* workgroup barrier of the last ll evaluation's streamed kernel as it was launched: 0 = another
                                       kernel ran, else bits 0-1 = 1 the waves never met, 2 they met before every unit, 3 before
                                       every category, and bit 4 = no bit of PLK_OPT_PAIR_TABLES forced it: it was decided, once
                                       per upload, on the formats that run (plk_k4_stream by plk_v4s_auto_sync) */
};

/* force the generic (HBM-resident partials) traversal even where the fused
 * kernel applies; used by tests and by bench.py --kernel generic.
 * Which ll kernel runs is decided once, when the device formats of the program are uploaded (the engine's ll plan), not
 * per evaluation.  Setting any option that decision reads (PLK_OPT_FUSED_SITES_PER_LANE, _FUSED_ASM, _MFMA, _PAIR_TABLES,
 * _VEC_REG_STACK, _MFMA_NS2, _STREAM_GRID) marks the plan stale, PLK_OPT_FORCE_GENERIC the program itself: the next evaluation
 * decides and uploads again. */
int plk_set_option(plk_engine *h, int option, long value);
enum { PLK_OPT_FORCE_GENERIC = 0, PLK_OPT_SITE_CHUNK = 1, PLK_OPT_FUSED_SITES_PER_LANE = 2 /* 0 auto, 1, 2 */,
       PLK_OPT_FUSED_ASM = 3 /* 1 (default): assembly interpreter loop where applicable, 0: C++ loop */,
       PLK_OPT_MFMA = 4 /* 1 (default): register-resident vector kernel for 9 <= k <= 32, fp64 matrix-core kernel for
                           33 <= k <= 64; 2: matrix-core kernel for all of 9 <= k <= 64; 0: generic vector kernel */,
       PLK_OPT_UP_NODES = 5 /* node-visit up pass for derivative queries, a bit per kernel family (default 2):
                               bit 1 (2): k = 4 kernels (k_up4_nodes: a third fewer HBM bytes than k_up4);
                               bit 2 (4): k = 4 kernels WITHOUT the table rebuild of nodes whose two children are leaves or
                               two-leaf nodes (by default their vectors do not go through HBM in either pass);
                               bit 3 (8): k = 4 kernels WITHOUT finishing two-leaf nodes inside their parent's visit (done for models with one
                               rate category: with four in flight the visit has no registers left for it);
                               bit 0 (1): matrix-core kernels, 21 <= k <= 64 or all of 9 <= k <= 64 under PLK_OPT_MFMA = 2
                               (k_up_nodes_mfma: fewer HBM bytes, same speed as measured in round 2).
                               Marginal queries always take the one-edge-at-a-time passes.  ARBPLF_UP_NODES in the
                               environment sets the initial value. */,
       PLK_OPT_PAIR_TABLES = 6 /* k = 4 trees within 4 stack slots and 16 character definitions: two-leaf subtrees as table
                               look-ups, grid-stride tile loop, one workgroup per CU.  1 (default): the streamed form of 7 where it
                               fits, else the interpreter with two sites per lane (k_ll_fused4_v4) on 1536-site tiles, or 1024-site tiles when the
                               tables leave less LDS, else one site per lane; 5 / 6: two sites per lane on 1024 / 1536
                               sites; 2 / 3: one site per lane (k_ll_fused4_asm_pt) on 1024 / 512 sites; 0: the round-2
                               interpreter over 256-site tiles, no pair tables; 7: two sites per lane with the codes
                               streamed from a per-unit stream in device memory (built when the formats are uploaded:
                               about one byte per site and leaf or cherry) and the tables of all categories resident in
                               LDS (k_ll_fused4_v4s) wherever C x table bytes fit the LDS and the stream fits device
                               memory, otherwise as 1; the default takes that form under the same conditions.  + 8: without the
                               scalar-cache warm-up; streamed form: by default its waves meet before every category, except
                               where one category is resident at a time (one rate category, or a group per category) and
                               its matrix stream and op words fit the 16 KB scalar cache: then they never meet (DESIGN.md
                               section 4); + 16: they meet before every unit, + 32: never (+ 32 wins over + 16), + 65536: before
                               every category, whatever the plan (measurements; PLK_INFO_LL_BARRIER reports what ran); + 64: the streamed form without the folded op
                               stream and without the held first chunks (the checked stream as it is built, ADVANCE and SCALE
                               ops dispatched on their own, every category requesting the unit's first three chunks itself:
                               the kernel as it was before the fold, and what runs when the fold does not replay);
                               + 128: without the held chunks only, + 256: without the fold only (measurements);
                               + 512: without the pair products of trees within 3 stack slots (k_ll_fused4_v4s<768, true, true>: a second
                               look-up buffer in the registers of slot 3, two table rows multiplied under one dispatch):
                               the folded stream with held chunks on k_ll_fused4_v4s, the default before that form
                               (measurements; + 64 / + 128 / + 256 imply it);
                               + 1024: the three-leaf form of the streamed kernel wherever it applies (a node that is not the
                               root and whose children are a cherry and a leaf becomes, with the edge above it, one look-up
                               of a table of nchar^3 rows, nchar^3 <= 256; to make room the categories may run in groups,
                               the tables of one group resident at a time, in phases of the one launch); the default takes
                               it only where every wave walks enough units per phase to pay for the phases (DESIGN.md
                               section 4); + 2048: never; + 4096 / + 8192 / both: the categories in one group / one group
                               per category / two groups instead of the cost model's choice (measurements);
                               + 16384: the four-leaf form wherever it applies, whatever the site count (a node that is not
                               the root, with four leaves below it as ((cherry, leaf), leaf) or (cherry, cherry), each leaf
                               taking at most 4 of the nchar codes in the uploaded patterns, becomes with the edge above it
                               one look-up of a 256-row table indexed by the leaves' code ranks; any nchar <= 16); it
                               implies + 1024 for the nodes it leaves, and the default takes it under the same rule as the
                               three-leaf form; + 32768: never.  + 1024 alone keeps to three-leaf tables, + 2048 forbids
                               both (PLK_INFO_LL_QUAD) */,
       PLK_OPT_VEC_REG_STACK = 7 /* 1 (default): the vector kernels (9 <= k <= 20) keep the three busiest stack slots in
                               registers (2 waves per SIMD); 0: every waiting vector goes through HBM slots (round 2) */,
       PLK_OPT_MFMA_NS2 = 8 /* 1: the matrix-core ll kernel for 33 <= k <= 64 gives a wave two groups of 16 sites (every staged
                               matrix and every fragment read serve 128 sites of a workgroup); 0 (default): one group.  Measured
                               equal at BASELINE config 5 */,
       PLK_OPT_STREAM_GRID = 9 /* 0 (default): the streamed k = 4 ll kernel launches one workgroup per CU; n > 0: at most n
                               workgroups, and its plan (three- and four-leaf tables, category groups) is made for n CUs.
                               For tests: with 1 or 2 workgroups every wave walks several units at a few thousand sites */ };

/* ------------------------------------------------------------------------------------------------------------
 * Several GPUs in one process: a group of engines, one per listed device, behind the same calls.
 *
 * Sites are independent given (tree, Q, rates); the only cross-site operations of the reference are the axis
 * reductions of nd_accum_accumulate (src/ndaccum.c:198-254) at the end of the site loops (src/arbplfll.c:139-170,
 * src/arbplfderiv.c:329-356, src/arbplfmarginal.c:237-256).  A group therefore gives engine i the contiguous block
 * [i*ceil(S/G), min(S, (i+1)*ceil(S/G))) of the site patterns (and of the weights), runs the engines concurrently
 * (one host thread each), returns per-site outputs at their global positions and adds the {hi, lo} partial sums of
 * the engines in engine order (long double): ll (2 doubles), edge sums (2E), node/state sums (2Nk), Hessian (2EE).
 * Deterministic for a given device list.  Every engine computes the same transition matrices itself (cheaper than
 * moving them).  The same device may be listed more than once (two engines then share it).
 * The host drivers (arbplf-ll and friends) build their group from the environment: ARBPLF_DEVICES=0,1,2,...
 * (default: ARBPLF_DEVICE or device 0).  Host buffers only; every call is synchronous.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct plk_group plk_group;

int plk_group_create(plk_group **out, int ndev, const int *devices);
void plk_group_destroy(plk_group *g);
const char *plk_group_last_error(const plk_group *g);
int plk_group_size(const plk_group *g);
plk_engine *plk_group_engine(plk_group *g, int i);           /* for plk_set_option / plk_get_info */
/* site block of engine i as set by the last plk_group_set_patterns_*: [*s0, *s1) */
int plk_group_block(const plk_group *g, int i, long *s0, long *s1);

int plk_group_set_tree(plk_group *g, int N, const int *indptr, const int *indices, const int *preorder);
int plk_group_set_model(plk_group *g, int k, int C, const double *Qn, const double *Qn_lo, const double *edge_rates_csr,
                        const double *cat_rates, const double *cat_prior, int root_mode, const double *root_w);
int plk_group_update_edge_rates(plk_group *g, const double *edge_rates_csr);
int plk_group_set_patterns_codes(plk_group *g, long S, const uint8_t *codes /* [N][S] host */, int nchar, const double *defs);
int plk_group_set_patterns_dense(plk_group *g, long S, const double *B /* [N][k][S] host */);
int plk_group_set_site_weights(plk_group *g, const double *w /* [S] host or NULL */);
int plk_group_ll(plk_group *g, double *site_ll_out, double *sum_out);
int plk_group_deriv(plk_group *g, const int *edge_mask, double *site_edge_out, double *edge_sums_out);
int plk_group_marginal(plk_group *g, const int *node_mask, double *site_out, double *sums_out);
int plk_group_edge_expect_multi(plk_group *g, int nL, const double *L_hi, const double *L_lo, int coef_mode,
                                const int *edge_mask, double *site_out, double *sums_out);
/* post_out [S][C] and rate_out [S] at their global positions; post_sums_out [C][2], rate_sum_out [2] (any may be NULL) */
int plk_group_cat_posterior(plk_group *g, double *post_out, double *rate_out, double *post_sums_out, double *rate_sum_out);
/* W_out [C][E][k][k][2], root_out NULL or [C][k][2]; G_out [k][k][2], root_out NULL or [k][2]: partial sums of the engines
 * added in engine order (long double), as for the other sums */
int plk_group_edge_pair_sums(plk_group *g, const int *edge_mask, double *W_out, double *root_out);
int plk_group_rate_matrix_sens(plk_group *g, double *G_out, double *root_out);
/* prior_out, rate_out [C][2]: partial sums of the engines added in engine order (long double) */
int plk_group_mixture_sens(plk_group *g, double *prior_out, double *rate_out);
/* site_out [n_swaps][S] at the global site positions; sums_out [n_swaps][2]: partial sums of the engines added in engine
 * order (long double) */
int plk_group_nni_ll(plk_group *g, int n_swaps, const int *swaps, double *site_out, double *sums_out);
/* arguments and outputs as plk_place_ll with S the sites of the group; each engine gets its site block of the query rows;
 * sums_out: partial sums of the engines added in engine order (long double) */
int plk_group_place_ll(plk_group *g, int n_queries, const uint8_t *q_codes, const double *q_dense, int n_edges, const int *edges,
                       double split, double pendant_rate, double *site_out, double *sums_out);
/* arguments and outputs as plk_spr_ll with S the sites of the group: site_out [n_moves][S] at the global site positions;
 * sums_out [n_moves][2]: partial sums of the engines added in engine order (long double) */
int plk_group_spr_ll(plk_group *g, int n_moves, const int *moves, double split, double *site_out, double *sums_out);
int plk_group_hess(plk_group *g, double *hess_sums_out);
int plk_group_second_order(plk_group *g, double *grad_sums_out, double *hess_sums_out);   /* either may be NULL */

#ifdef __cplusplus
}
#endif
#endif
