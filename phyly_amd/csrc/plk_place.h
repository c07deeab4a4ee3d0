/*
 * plk_place.h -- up passes of plk_place_ll: the log likelihood of the current tree with a new leaf attached to an edge,
 * for many new leaves (queries) and many edges, from the vectors one down pass leaves in device memory.  Included by
 * plk_engine.hip after plk_nni.h, whose rescaling helpers (nni_norm, nni_norm4, nni_normK, NniSum) it uses.  The
 * reference has no such pass.
 *
 * A placement onto the edge e = (u -> b) with rate coefficient r_e, split rho and pendant rate p replaces e by
 * (u -> m) with rate fl(rho r_e), (m -> b) with rate fl(fl(1 - rho) r_e) and (m -> q) with rate p; m has no data, q
 * carries the query's observation x_q.  Per site and category
 *     g  = F_u o data_u SC_u                       G = g o prod_{w child of u, w != b} m_w
 *     H  = A^T G      A = exp(Qn r_c fl(rho r_e))
 *     M  = B L_b      B = exp(Qn r_c fl(fl(1 - rho) r_e))          (a leaf b: B times its definition row)
 *     T  = D x_q      D = exp(Qn r_c p)
 *     N_c = sum_j H[j] M[j] T[j]
 *     ll' = log(sum_c prior_c N_c 2^(X_c + e_c - Emax)) + Emax log 2
 * A, B and D come from one launch of K1 over the rates of the call, in buffers of the call's own; the engine's matrices
 * are not touched.  A constant vector passes a transition matrix unchanged (the project's rule), so an all-missing query
 * has T = 1 exactly.
 *
 * Exponents: G and L_b together take every rescaled node of the tree exactly once (the argument at the top of
 * plk_nni.h: F_u holds the factors outside the subtree of u, SC_u is u's own, the stored L of every child holds those of
 * its subtree), so N_c sits at the exponent X_c of the down pass.  G and M are each brought to [1, 2) by an exact power
 * of two before they meet, and the dot product once more; these exponents and that of SC_u form e_c.  Nothing is divided
 * by the likelihood of the current tree; a placement of likelihood 0 gives -inf.
 *
 * W = H o M does not depend on the query: it is formed once per (record, category, site) and every query of the record
 * costs one row of the pendant table, a dot product and its share of one log.
 *
 * The host sorts the records of a pass by the preorder position of u.  A record of PLACE_REC ints:
 *     [0] preorder position of u   [1] CSR edge e = (u -> b)   [2] index j of the edge among the call's distinct target
 *     edges: A is matrix 2 j, B matrix 2 j + 1 of the call's matrices, D the last one
 *     [3] first query of the run   [4] number of queries   [5] plane row of the first query; query [3] + i goes to row [5] + i
 * Launch: a grid over the site chunk, one site per lane, as k_up4_nni; the first pass over a chunk stores the forward
 * vectors, later passes read them and visit only the nodes their records name.
 */
#ifndef PLK_PLACE_H
#define PLK_PLACE_H

#define PLACE_REC 6
#define PLACE_MAX_ROWS 256        /* rows of the per-site plane of one pass */

struct PlaceOut {
    const int *rec;      /* [nrec][PLACE_REC], sorted by rec[0] */
    int nrec;
    int store_fn;        /* 1: store the forward vectors (the first pass over a chunk) */
    int EQ;              /* matrices per category of the call: 2 (distinct target edges) + 1 */
    const double *QP;    /* k = 4: [C][EQ][16] row-major; generic: not read */
    const double *QPT, *QPN;   /* generic: [C][EQ][K*K] transposed / plain, as UpArgs.PT / PN */
    const double *T;     /* pendant tables [C][nchar][4] (k = 4) or [C][nchar][K] (generic, compact codes) */
    const uint8_t *q_codes;    /* [Q][Spad] or null */
    const double *q_dense;     /* [Q][k][S] or null */
    double *WS;          /* generic: [C][k][n] W of the record at hand; XW [C][n] its exponents */
    double *XW;
    double *plane;       /* [rows][n] */
};

/* pendant table of the generic kernel: T[c][code][i] = sum_j D[i][j] defs[code][j] in up_matvec's order, a constant
 * definition row unchanged; DT is the transposed padded D of every category ([C][EQ][K*K], matrix EQ - 1) */
__global__ void k_place_table(int k, int K, int EQ, int nchar, const double *__restrict__ QPT, const double *__restrict__ defs, double *__restrict__ T)
{
    const int c = blockIdx.x;
    const double *M = QPT + ((size_t)c * EQ + (EQ - 1)) * K * K;
    for (int idx = threadIdx.x; idx < nchar * K; idx += blockDim.x) {
        const int code = idx / K, i = idx - code * K;
        const double *d = defs + (size_t)code * K;
        bool is_const = true;
        double m = 0.0;
        for (int j = 0; j < k; j++) { is_const = is_const && d[j] == d[0]; m = fma(M[j * K + i], d[j], m); }
        if (is_const) m = i < k ? d[0] : 0.0;
        T[((size_t)c * nchar + code) * K + i] = m;
    }
}

#define PLACE4_MAX_C 4

/*
 * k = 4, compact codes, at most four categories: the walk of k_up4_nni with the placements of a node in place of its
 * swaps.  The pendant tables of all categories are staged in LDS (C nchar 32 bytes, at most 32 KiB; the kernel holds
 * no other LDS); W of the four categories stays in registers across the queries of a record.
 */
__global__ __launch_bounds__(UD4_BLOCK) void k_up4_place(Up4Args a, PlaceOut o)
{
    extern __shared__ double place_T[];                  /* [C][nchar][4] */
    const long sl = (long)blockIdx.x * UD4_BLOCK + threadIdx.x;
    const bool valid = sl < a.n;
    const long slc = valid ? sl : a.n - 1;
    const long sg = a.s0 + slc;
    const size_t n = (size_t)a.n;
    const PLK_AS4 int *pre = as_uniform(a.preorder), *ip = as_uniform(a.indptr), *ix = as_uniform(a.indices);
    const PLK_AS4 int *has = as_uniform(a.node_has_data), *etip = as_uniform(a.edge_tip);
    const PLK_AS4 int *nint = as_uniform(a.node_int), *nsc = as_uniform(a.node_scale);
    const PLK_AS4 int *rec = as_uniform(o.rec);
    const PLK_AS4 double *Pm = as_uniform(a.P), *Qm = as_uniform(o.QP);
    const PLK_AS4 double *prior = as_uniform(a.cat_prior), *rw = as_uniform(a.root_w);
    const size_t tabc = (size_t)(a.ntips + 1) * a.nchar * 4;
    const int root = pre[0];

    for (int i = threadIdx.x; i < a.C * a.nchar * 4; i += UD4_BLOCK) place_T[i] = o.T[i];
    __syncthreads();

    if (o.store_fn && valid) {
        const v4 w = v4{rw[0], rw[1], rw[2], rw[3]};
        for (int c = 0; c < a.C; c++) st4(a.FN + (((size_t)nint[root] * a.C + c) * n + slc) * 4, w);
    }

    int r = 0;
    for (int u = 0; u < a.N; u++) {
        if (!o.store_fn) {                                /* only the nodes the records name */
            if (r >= o.nrec) break;
            u = rec[r * PLACE_REC];
        }
        const int nd = pre[u];
        const int start = ip[nd], stop = ip[nd + 1];
        if (start == stop) continue;
        const bool hd = has[nd] != 0;
        const int slot = nsc[nd];
        const double *fn_nd = a.FN + ((size_t)nint[nd] * a.C) * n * 4;
        const int cd_nd = hd ? a.codes[(size_t)nd * a.Spad + sg] : 0;

        /* forward vectors of the internal children: F_b = P_e^T (g o messages of the other children), as k_up4_nni */
        if (o.store_fn) {
            for (int idx = start; idx < stop; idx++) {
                if (etip[idx] >= 0) continue;
                const int b = ix[idx];
                for (int c = 0; c < a.C; c++) {
                    const double *tipc = a.tip + (size_t)c * tabc;
                    v4 g = ld4(fn_nd + ((size_t)c * n + slc) * 4);
                    if (hd) g = mul4(g, ld4(tipc + ((size_t)a.ntips * a.nchar + cd_nd) * 4));
                    if (slot >= 0) {
                        const double sc = a.SC[((size_t)slot * a.C + c) * n + slc];
                        g.a *= sc; g.b *= sc; g.c *= sc; g.d *= sc;
                    }
                    v4 fe = g;
                    for (int idx2 = start; idx2 < stop; idx2++) {
                        if (idx2 == idx) continue;
                        fe = mul4(fe, nni4_msg(a, c, idx2, sg, slc, tipc, Pm));
                    }
                    if (valid) st4(a.FN + (((size_t)nint[b] * a.C + c) * n + slc) * 4, mtv4(Pm + ((size_t)c * a.E + idx) * 16, fe));
                }
            }
        }

        /* the placements onto the edges below nd */
        for (; r < o.nrec && rec[r * PLACE_REC] == u; r++) {
            const int idx_b = rec[r * PLACE_REC + 1], j = rec[r * PLACE_REC + 2];
            const int q0 = rec[r * PLACE_REC + 3], nq = rec[r * PLACE_REC + 4], row0 = rec[r * PLACE_REC + 5];
            const int tb = etip[idx_b], b = ix[idx_b];
            const int cd_b = tb >= 0 ? a.codes[(size_t)b * a.Spad + sg] : 0;
            v4 W[PLACE4_MAX_C];
            int ew[PLACE4_MAX_C];
#pragma unroll
            for (int c = 0; c < PLACE4_MAX_C; c++) {
                W[c] = v4{0.0, 0.0, 0.0, 0.0};
                ew[c] = 0;
                if (c >= a.C) continue;
                const double *tipc = a.tip + (size_t)c * tabc;
                int eb = (int)a.XC[(size_t)c * n + slc];
                /* G: what u holds without the message of b */
                v4 G = ld4(fn_nd + ((size_t)c * n + slc) * 4);
                if (hd) G = mul4(G, ld4(tipc + ((size_t)a.ntips * a.nchar + cd_nd) * 4));
                if (slot >= 0) eb += ilogb(a.SC[((size_t)slot * a.C + c) * n + slc]);
                for (int idx2 = start; idx2 < stop; idx2++) {
                    if (idx2 == idx_b) continue;
                    G = mul4(G, nni4_msg(a, c, idx2, sg, slc, tipc, Pm));
                }
                eb += nni_norm4(G);
                const v4 H = mtv4(Qm + ((size_t)c * o.EQ + 2 * j) * 16, G);
                /* M = B L_b, a constant L_b unchanged */
                v4 L;
                if (tb >= 0) L = ld4(tipc + ((size_t)a.ntips * a.nchar + cd_b) * 4);
                else L = ld4(a.LN + (((size_t)nint[b] * a.C + c) * n + slc) * 4);
                v4 M = mv4(Qm + ((size_t)c * o.EQ + 2 * j + 1) * 16, L);
                if (const4(L)) M = L;
                eb += nni_norm4(M);
                W[c] = mul4(H, M);
                ew[c] = eb;
            }
            for (int qi = 0; qi < nq; qi++) {
                const int code = o.q_codes[(size_t)(q0 + qi) * a.Spad + sg];
                NniSum s = {0.0, 0, false};
#pragma unroll
                for (int c = 0; c < PLACE4_MAX_C; c++) {
                    if (c >= a.C) continue;
                    const double *t = place_T + ((size_t)c * a.nchar + code) * 4;
                    double d = fma(W[c].d, t[3], fma(W[c].c, t[2], fma(W[c].b, t[1], W[c].a * t[0])));
                    double sc;
                    const int ed = nni_norm(d, sc);
                    d *= sc;
                    nni_sum_add(s, prior[c] * d, ew[c] + ed);
                }
                if (valid) o.plane[(size_t)(row0 + qi) * n + sl] = nni_sum_ll(s);
            }
        }
    }
}

/*
 * Every other state count, dense observations, more than four categories: the planes and stored edge vectors of
 * k_up_nni<K> (whose FORWARD instantiation stores the forward vectors of a chunk before the first pass), one wave per
 * workgroup.  W of a record goes to a small plane of the call's own (WS [C][k][n], exponents XW [C][n]): the lane that
 * writes a column is the lane that reads it back, once per query.  T is a row of the pendant table for compact codes
 * and D x_q for dense ones.  Correct first: this kernel is not tuned.
 */
template <int K>
__global__ __launch_bounds__(GEN_BLOCK) void k_up_place(UpArgs a, PlaceOut o)
{
    __shared__ double xs[K][GEN_BLOCK];                  /* a lane reads and writes its own column only */
    const int tid = threadIdx.x;
    const long sl = (long)blockIdx.x * GEN_BLOCK + tid;
    const bool valid = sl < a.n;
    if (!valid) return;                                  /* no barrier below; a lane past the chunk must not touch WS */
    const long slc = sl;
    const long sg = a.s0 + slc;
    const size_t n = (size_t)a.n;
    const int k = a.k;
    const PLK_AS4 int *rec = as_uniform(o.rec);

    for (int r = 0; r < o.nrec; r++) {
        const int nd = as_uniform(a.preorder)[rec[r * PLACE_REC]];
        const int idx_b = rec[r * PLACE_REC + 1], j = rec[r * PLACE_REC + 2];
        const int q0 = rec[r * PLACE_REC + 3], nq = rec[r * PLACE_REC + 4], row0 = rec[r * PLACE_REC + 5];
        const int start = as_uniform(a.indptr)[nd], stop = as_uniform(a.indptr)[nd + 1];
        const bool has = as_uniform(a.node_has_data)[nd];
        const int slot = a.node_scale ? as_uniform(a.node_scale)[nd] : -1;
        const int b = as_uniform(a.indices)[idx_b];
        const bool b_leaf = as_uniform(a.indptr)[b] == as_uniform(a.indptr)[b + 1];
        for (int c = 0; c < a.C; c++) {
            long slo = slc, sgo = sg;                    /* opaque per category, as in k_up_nni */
            asm volatile("" : "+v"(slo), "+v"(sgo));
            int eb = a.XC ? (int)a.XC[(size_t)c * n + slo] : 0;
            double *ws = o.WS + (size_t)c * k * n + slo;
            /* M = B L_b first; it waits in WS while H is formed */
            {
                double L[K];
                if (b_leaf) up_load_obs_reg<K>(a, b, sgo, L);
                else {
                    const double *ln = a.LN + ((size_t)b * a.C + c) * k * n + slo;
#pragma unroll
                    for (int i = 0; i < K; i++) L[i] = i < k ? ln[(size_t)i * n] : 0.0;
                }
#pragma unroll
                for (int i = 0; i < K; i++) xs[i][tid] = L[i];
                double M[K];
                up_matvec<K, 1>(o.QPT + ((size_t)c * o.EQ + 2 * j + 1) * K * K, k, xs, tid, M);
                eb += nni_normK<K>(M);
#pragma unroll
                for (int i = 0; i < K; i++)
                    if (i < k) ws[(size_t)i * n] = M[i];
            }
            double G[K];
            const double *fa = a.FN + ((size_t)nd * a.C + c) * k * n + slo;
#pragma unroll
            for (int i = 0; i < K; i++) G[i] = i < k ? fa[(size_t)i * n] : 0.0;
            if (has) {
                double bnd[K];
                up_load_obs_reg<K>(a, nd, sgo, bnd);
#pragma unroll
                for (int i = 0; i < K; i++) G[i] *= bnd[i];
            }
            if (slot >= 0) eb += ilogb(a.SC[((size_t)slot * a.C + c) * n + slo]);
            for (int idx2 = start; idx2 < stop; idx2++) {
                if (idx2 == idx_b) continue;
                nni_mul_msg<K>(a, c, idx2, sgo, slo, tid, xs, G);
            }
            eb += nni_normK<K>(G);
            /* H[j] = sum_i A[i][j] G[i], then W = H o M */
#pragma unroll
            for (int i = 0; i < K; i++) xs[i][tid] = G[i];
            double H[K];
            up_matvec<K, 0>(o.QPN + ((size_t)c * o.EQ + 2 * j) * K * K, k, xs, tid, H);
#pragma unroll
            for (int i = 0; i < K; i++)
                if (i < k) ws[(size_t)i * n] *= H[i];
            o.XW[(size_t)c * n + slo] = (double)eb;
        }
        for (int qi = 0; qi < nq; qi++) {
            NniSum s = {0.0, 0, false};
            const int code = o.q_codes ? o.q_codes[(size_t)(q0 + qi) * a.Spad + sg] : 0;
            if (!o.q_codes) {
                const double *bp = o.q_dense + (size_t)(q0 + qi) * k * a.S + sg;
                for (int i = 0; i < k; i++) xs[i][tid] = bp[(size_t)i * a.S];
            }
            for (int c = 0; c < a.C; c++) {
                const double *ws = o.WS + (size_t)c * k * n + slc;
                double d = 0.0;
                if (o.q_codes) {
                    const double *t = o.T + ((size_t)c * a.nchar + code) * K;
#pragma unroll
                    for (int i = 0; i < K; i++)
                        if (i < k) d = fma(ws[(size_t)i * n], t[i], d);
                } else {
                    nni_matvec_each<K>(o.QPT + ((size_t)c * o.EQ + (o.EQ - 1)) * K * K, k, xs, tid,
                                       [&](int i, double m) { if (i < k) d = fma(ws[(size_t)i * n], m, d); });
                }
                double sc;
                const int ed = nni_norm(d, sc);
                d *= sc;
                nni_sum_add(s, as_uniform(a.cat_prior)[c] * d, (int)o.XW[(size_t)c * n + slc] + ed);
            }
            if (valid) o.plane[(size_t)(row0 + qi) * n + sl] = nni_sum_ll(s);
        }
    }
}

#endif
