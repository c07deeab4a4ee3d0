/*
 * arbplf.h -- the operator-level C-ABI of the drop-in (libarbplf_amd.so).
 *
 * The reference exposes each query as a json_hom_fn_t
 *     json_t *arbplf_ll_run(void *userdata, json_t *root, int *retcode);
 * (src/arbplfll.h:10, src/arbplfderiv.h, src/arbplfmarginal.h; type in
 * src/runjson.h:32-33) and derives from it the string form
 *     char *(*string_hom_fn_t)(void *userdata, const char *s_in, int *retcode);
 * (src/runjson.h:28-29, jsonwrap in src/runjson.c:10-66), which is what its CLI
 * mains (src/arbplf-ll.c:4-15) and its Python module (src/arbplf.c:209-250) call.
 * jansson is not a dependency of this build, so the string form is the boundary:
 * the three functions below have exactly the string_hom_fn_t signature.
 *
 * Contract (as in the reference): `userdata` must be NULL; `s_in` is one JSON
 * document; on success *retcode = 0 and the return value is a malloc'd JSON
 * string the caller frees with free(); on failure *retcode != 0, NULL is
 * returned and a diagnostic has been written to stderr.  Never uses errno.
 * Unlike the reference (flint_cleanup at the end of every call) the functions
 * are thread-safe; calls are serialised on one cached GPU engine.
 *
 * The likelihood work runs on the GPU selected by the environment variable
 * ARBPLF_DEVICE (default 0).  There is no CPU path: without a usable MI355X
 * the call fails with a diagnostic.
 */
#ifndef ARBPLF_H
#define ARBPLF_H

#ifdef __cplusplus
extern "C" {
#endif

char *arbplf_ll_string(void *userdata, const char *s_in, int *retcode);
char *arbplf_deriv_string(void *userdata, const char *s_in, int *retcode);
char *arbplf_marginal_string(void *userdata, const char *s_in, int *retcode);
/* the expectation queries that reuse the same down / up passes
 * (src/arbplfdwell.h, src/arbplftrans.h, src/arbplfem.h: arbplf_dwell_run, arbplf_trans_run,
 * arbplf_em_update_run) */
char *arbplf_dwell_string(void *userdata, const char *s_in, int *retcode);
char *arbplf_trans_string(void *userdata, const char *s_in, int *retcode);
char *arbplf_em_update_string(void *userdata, const char *s_in, int *retcode);
/* the Hessian of the log likelihood (hess_query behind arbplf_second_order_run,
 * src/arbplfhess.c:1279-1343, :1736-1771), fp64 and uncertified */
char *arbplf_hess_string(void *userdata, const char *s_in, int *retcode);
/* what the Hessian is for (inv_hess_query, newton_delta_query, newton_point_query of src/arbplfhess.c:1238-1267,
 * :1372-1388, :1427-1443): its inverse, the Newton step -H^-1 g, and edge_rate_coefficients + that step.  A Hessian
 * that is singular to working precision is refused (plk_solve_second_order in plk.h). */
char *arbplf_inv_hess_string(void *userdata, const char *s_in, int *retcode);
char *arbplf_newton_delta_string(void *userdata, const char *s_in, int *retcode);
char *arbplf_newton_update_string(void *userdata, const char *s_in, int *retcode);
/* Rate-category posteriors and posterior mean site rates of a rate mixture (empirical Bayes; the reference has no such
 * command).  cat_posterior: model_and_data, optional site_reduction and category_reduction (the reference's reduction
 * grammar), columns ["site", "category", "value"] with aggregated axes dropped; categories in the order of the mixture,
 * the invariable one last.  site_rate: model_and_data, optional site_reduction, columns ["site", "value"].  A model
 * without a mixture has one category: posterior 1, rate 1. */
char *arbplf_cat_posterior_string(void *userdata, const char *s_in, int *retcode);
char *arbplf_site_rate_string(void *userdata, const char *s_in, int *retcode);
/* Gradient of the site-aggregated log likelihood in the entries of rate_matrix (the reference has no such command; it
 * differentiates in the edge rates only).  model_and_data plus a site_reduction whose aggregation is mandatory ("sum",
 * "avg" or a weight array; selection optional); any other key is rejected.  Columns ["first_state", "second_state",
 * "value"]: d/dq_ij for every ordered pair i != j, row-major, the diagonal being minus the row sums; the rate divisor
 * (a number or "equilibrium_exit_rate") and an equilibrium root prior are differentiated through. */
char *arbplf_rate_matrix_deriv_string(void *userdata, const char *s_in, int *retcode);
/* Gradient of the site-aggregated log likelihood in the parameters of the rate mixture (the reference has no such
 * command).  The request grammar of rate_matrix_deriv: model_and_data plus a site_reduction whose aggregation is
 * mandatory.  Columns ["parameter", "category", "value"].  gamma_rate_mixture and normalized_median_gamma_rate_mixture:
 * ["gamma_shape", 0, v] and, when invariable_prior is given and not 0, ["invariable_prior", 0, v] (without an invariable
 * category there is nothing to report; pass a tiny positive value for the one-sided derivative).  rate_mixture:
 * ["rate", c, v] for every category, then ["prior", c, v] for every category when the prior is an array (priors taken as
 * independent); an "equilibrium_exit_rate" divisor is differentiated through (it carries the expected rate).  A model
 * without a mixture is refused. */
char *arbplf_mixture_deriv_string(void *userdata, const char *s_in, int *retcode);
/* Log likelihood of nearest-neighbour interchanges of the tree (the reference has no such command): what a tree search
 * asks between two fits, from one pass over the current tree (plk_nni_ll in plk.h) in place of one arbplf-ll per candidate.
 * Input: model_and_data, an optional site_reduction exactly as for arbplf-ll, and an optional "swaps": [[a, b], ...] in the
 * edge indices of the document's `edges`.  A swap is a pair of edges a = (v -> c), b = (u -> s) with v a child of u and
 * s != v; the swapped tree has a = (u -> c) and b = (v -> s): the two subtrees exchange parents, each edge keeps its index
 * and rate, all data stay where they are.  Without "swaps": every swap of the tree, ordered by (a, b).
 * Columns ["site", "first_edge", "second_edge", "value"], without the site column under site aggregation; rows in the
 * order of the request, site outermost.  A pair that is no swap, a non-integer or an index out of range is an error; a
 * value that is not finite (likelihood 0 under the swapped tree) is refused as arbplf-ll refuses it. */
char *arbplf_nni_string(void *userdata, const char *s_in, int *retcode);
/* Log likelihood of the tree with a new taxon attached to an edge, for every query taxon and every listed edge (the
 * reference has no such command): placement of reads, stepwise addition, the regraft half of an SPR move, from one pass
 * over the current tree (plk_place_ll in plk.h) in place of one arbplf-ll per (query, edge).
 * Input: model_and_data, an optional site_reduction exactly as for arbplf-ll, and
 *   "placement": {"character_data": [[c_q0, c_q1, ...], ... one row per site ...], "edges": [3, 0, 7], "split": 0.5,
 *                 "pendant_rate": 0.1}
 * The query characters index the model's character_definitions (also for a model with character_data_file); a model with
 * probability_array takes "probability_array": [site][query][state] instead.  "edges" are indices into the document's
 * `edges`, repeats allowed; omitted: every edge in document order.  "split" in [0, 1] (default 0.5) is the share of the
 * target edge's rate coefficient above the new node; "pendant_rate" (required, finite, not negative) is the rate
 * coefficient of the new leaf's edge.  The edge (u -> b) with rate r becomes (u -> m) with rate split r, (m -> b) with
 * rate (1 - split) r and (m -> query) with rate pendant_rate.
 * Columns ["site", "query", "edge", "value"], without the site column under site aggregation; rows ordered by site, then
 * query, then edge as listed.  Sites are compressed to patterns on the columns of the tree and of the queries together.  A
 * value that is not finite (likelihood 0 under the placement) is refused as arbplf-ll refuses it. */
char *arbplf_place_string(void *userdata, const char *s_in, int *retcode);
/* Log likelihood of subtree prune-and-regraft moves of the tree (the reference has no such command): a whole subtree is
 * cut and attached to another edge, from one pass over the current tree and one pass per pruned edge (plk_spr_ll in plk.h)
 * in place of one arbplf-ll per candidate.
 * Input: model_and_data, an optional site_reduction exactly as for arbplf-ll, and an optional
 *   "spr": {"moves": [[prune, target], ...], "split": 0.5}
 * in the edge indices of the document's `edges`.  A move prunes the edge prune = (w -> x) with the subtree below x and
 * attaches it to the edge target = (u -> b), which is neither prune nor an edge below x: target becomes (u -> m) with rate
 * split r and (m -> b) with rate (1 - split) r, prune becomes (m -> x) with its own rate; w stays with one child fewer and
 * keeps its data.  Without "moves": every move of the tree, ordered by (prune, target); repeats are allowed.  "split" in
 * [0, 1] (default 0.5) is the share of the target edge's rate coefficient above the new node.
 * Columns ["site", "prune", "target", "value"], without the site column under site aggregation; rows in the order of the
 * request, site outermost.  A pair that is no move, a non-integer or an index out of range is an error; a value that is
 * not finite (likelihood 0 under the moved tree) is refused as arbplf-ll refuses it. */
char *arbplf_spr_string(void *userdata, const char *s_in, int *retcode);

/* Host-only validation of an input document (JSON grammar, model_and_data,
 * reductions) exactly as the corresponding query would perform it, without
 * touching the GPU.  what = "ll" | "deriv" | "marginal" | "dwell" | "trans" | "em_update" | "hess" |
 * "inv_hess" | "newton_delta" | "newton_update" | "cat_posterior" | "site_rate" | "rate_matrix_deriv" |
 * "mixture_deriv" | "nni" (the swap list is checked by the query itself) | "place" (with its "placement" object) | "spr" (the "spr" object is checked by the query itself).  0 = accepted.  Where the document selects at least one site this includes the preparation of the
 * model on the host (normalised rate matrix, category rates and priors) and the check of its values that every query
 * makes before any device work (plk_check_model_values in plk.h: non-finite or negative values, rate x length x |Qn|
 * beyond 2^40); the diagnostic names the edge in the order of the document's `edges`.  A document that selects no site
 * is accepted without it, as the query answers it without preparing the model. */
int arbplf_validate_string(const char *what, const char *s_in);

/* stdin -> stdout filter used by the CLI mains (run_string_script,
 * src/runjson.c:118-147): returns the process exit status */
int arbplf_run_stdin(char *(*f)(void *, const char *, int *));

/* release the cached engine (optional; e.g. before unloading the library) */
void arbplf_shutdown(void);

#ifdef __cplusplus
}
#endif
#endif
