/*
 * host_spr.c -- plk_spr_moves of include/plk.h: the canonical list of subtree prune-and-regraft moves of a rooted tree
 * in CSR form.  Host only: no engine and no GPU involved; the engine (plk_spr_ll with moves = NULL) and the JSON driver
 * (arbplf-spr without "moves") both take their list from here.
 *
 * A move is a pair of CSR edges (p, e), p = (w -> x) the pruned edge and e = (u -> b) the target, e neither p nor an
 * edge of the subtree below x.  The list is ordered by p, then by e: one rule, so the moves onto a sibling edge of p,
 * which at split 0 give back the current tree, stay in it.
 */
#include <stdlib.h>

#include "plk.h"

int plk_spr_moves(int N, const int *indptr, const int *indices, int *pairs_out)
{
    if (N < 1 || !indptr || indptr[0] != 0) return 0;
    for (int a = 0; a < N; a++) if (indptr[a + 1] < indptr[a]) return 0;
    const int E = N - 1;
    if (indptr[N] != E || (E > 0 && !indices)) return 0;
    if (E == 0) return 0;
    /* edge into every node (-1: the root), upper node of every edge, preorder position and subtree size of every node;
     * arrays that are no tree give no moves */
    int *in = malloc((size_t)N * sizeof(int)), *par = malloc((size_t)E * sizeof(int));
    int *pos = malloc((size_t)N * sizeof(int)), *size = malloc((size_t)N * sizeof(int)), *stack = malloc((size_t)N * sizeof(int));
    int ok = in && par && pos && size && stack;
    long count = 0;
    for (int a = 0; ok && a < N; a++) in[a] = -1;
    for (int a = 0; ok && a < N; a++)
        for (int idx = indptr[a]; idx < indptr[a + 1]; idx++) {
            const int b = indices[idx];
            if (b < 0 || b >= N || b == a || in[b] >= 0) { ok = 0; break; }
            in[b] = idx;
            par[idx] = a;
        }
    if (ok) {
        int root = -1, seen = 0, top = 0;
        for (int a = 0; a < N; a++) if (in[a] < 0) root = a;      /* N - 1 edges into distinct nodes: exactly one */
        stack[top++] = root;
        while (top > 0) {
            const int a = stack[--top];
            pos[a] = seen++;
            for (int idx = indptr[a + 1] - 1; idx >= indptr[a]; idx--) stack[top++] = indices[idx];
        }
        if (seen != N) ok = 0;                                     /* a cycle beside the tree */
        /* sizes: nodes in reverse preorder add themselves to their parent (stack reused as the preorder itself) */
        for (int a = 0; ok && a < N; a++) { stack[pos[a]] = a; size[a] = 1; }
        for (int u = N - 1; ok && u > 0; u--) size[par[in[stack[u]]]] += size[stack[u]];
    }
    for (int p = 0; ok && p < E; p++) {
        const int x = indices[p];
        for (int e = 0; e < E; e++) {
            const int u = par[e];
            if (e == p || (pos[u] >= pos[x] && pos[u] < pos[x] + size[x])) continue;
            if (pairs_out) { pairs_out[2 * count] = p; pairs_out[2 * count + 1] = e; }
            count++;
            if (count > 0x3fffffffL) { ok = 0; break; }           /* the count is an int, and so are the plane's rows */
        }
    }
    free(in); free(par); free(pos); free(size); free(stack);
    return ok ? (int)count : 0;
}
