/*
 * host_nni.c -- plk_nni_swaps of include/plk.h: the canonical list of nearest-neighbour interchanges of a rooted tree in
 * CSR form.  Host only: no engine and no GPU involved; the engine (plk_nni_ll with swaps = NULL) and the JSON driver
 * (arbplf-nni without "swaps") both take their list from here.
 *
 * A swap is a pair of CSR edges (a, b), a = (v -> c), b = (u -> s), v a child of u, s != v.  The list is ordered by a,
 * then by b: for every edge a whose upper node v has a parent u, the edges of u other than (u -> v) in CSR order.
 */
#include <stdlib.h>

#include "plk.h"

int plk_nni_swaps(int N, const int *indptr, const int *indices, int *pairs_out)
{
    if (N < 1 || !indptr || indptr[0] != 0) return 0;
    for (int a = 0; a < N; a++) if (indptr[a + 1] < indptr[a]) return 0;
    const int E = N - 1;
    if (indptr[N] != E || (E > 0 && !indices)) return 0;
    if (E == 0) return 0;
    /* edge into every node (-1: the root) and upper node of every edge; arrays that are no tree give no swaps */
    int *in = malloc((size_t)N * sizeof(int)), *par = malloc((size_t)E * sizeof(int));
    int count = 0, ok = in && par;
    for (int a = 0; ok && a < N; a++) in[a] = -1;
    for (int a = 0; ok && a < N; a++)
        for (int idx = indptr[a]; idx < indptr[a + 1]; idx++) {
            const int b = indices[idx];
            if (b < 0 || b >= N || b == a || in[b] >= 0) { ok = 0; break; }
            in[b] = idx;
            par[idx] = a;
        }
    for (int a = 0; ok && a < E; a++) {
        const int v = par[a];
        if (in[v] < 0) continue;
        const int u = par[in[v]];
        for (int b = indptr[u]; b < indptr[u + 1]; b++) {
            if (indices[b] == v) continue;
            if (pairs_out) { pairs_out[2 * count] = a; pairs_out[2 * count + 1] = b; }
            count++;
        }
    }
    free(in); free(par);
    return ok ? count : 0;
}
