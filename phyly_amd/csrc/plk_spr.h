/*
 * plk_spr.h -- up passes of plk_spr_ll: the log likelihood of subtree prune-and-regraft moves of the current tree from
 * the vectors one down pass leaves in device memory.  Included by plk_engine.hip after plk_place.h; it uses the
 * rescaling helpers and messages of plk_nni.h (nni_norm, nni_norm4, nni_normK, NniSum, nni4_msg, nni_mul_msg).  The
 * reference has no such pass.
 *
 * A move is a pair of CSR edges (p, e), p = (w -> x) and e = (u -> b), e neither p nor an edge below x.  The moved tree
 * has e replaced by (u -> m) with rate fl(rho r_e) and (m -> b) with rate fl(fl(1 - rho) r_e), p = (m -> x) with its
 * index, its rate r_p and the whole subtree below x; m is a new node without data; w stays with one child fewer (it may
 * become unary, or a leaf whose vector is its own observation row) and keeps its data.  For a w with two children and no
 * data this is, mathematically, the usual SPR in which the two edges at w merge: the unary node w multiplies their
 * transition matrices.
 *
 * The ending of a move is the ending of a placement (plk_place.h) whose pendant vector is the message the pruned subtree
 * sends today, T = P_p L_x.  What a placement never needed are the vectors of the tree WITHOUT the pruned subtree
 * (primed below).  Per prune edge, site and category:
 *   Path.     For y = w, parent(w), ..., root:  L'_y = data_y o prod_{children} messages, times the SAME factor SC_y the
 *             down pass chose; at w the message of p is left out, above w the child on the path sends P L'_child (a
 *             constant vector unchanged, the project's rule).  The products are formed again: nothing is divided.
 *   Forward.  F'_b = P_e^T (F'_u o data_u SC_u o prod_{other children} messages) for every internal node outside the
 *             subtree of x, as the store section of k_up4_place, with p skipped among the children of w and a child on
 *             the path sending the message of its L'.
 *   Ending.   G' = F'_u o data_u o prod_{children other than b and p} messages (the same substitutions),  H = A^T G',
 *             M = B L'_b (L_b itself where b is not on the path, the tip row for a leaf b),
 *             N_c = sum_j H[j] M[j] T[j],   ll' = log(sum_c prior_c N_c 2^(X_c + e_c - Emax)) + Emax log 2.
 * A = exp(Qn r_c fl(rho r_e)) and B = exp(Qn r_c fl(fl(1 - rho) r_e)) come from one launch of K1 over the distinct
 * target edges of the call into buffers of the call's own; they do not depend on p.  The pendant keeps r_p and the
 * engine's P.
 *
 * Exponents.  SC stays at the nodes the down pass chose, so G', L'_b and T together take every rescaled node exactly once
 * (the argument at the top of plk_nni.h) and N_c sits at X_c (XC) plus the exponents of the normalisations: G' and M
 * are brought to [1, 2) by exact powers of two before they meet, the dot product once more.  Leaving one message out of a
 * product on an unchanged scale can only enlarge it, by at most the reciprocal of that message's smallest positive entry
 * (DESIGN.md section 6).
 *
 * With pos the position of a node in a depth-first preorder (the engine's own order only puts parents before children), a
 * node y is w or above w exactly when pos[y] <= pos[w] < pos[y] + size[y], and below x or x when
 * pos[x] <= pos[y] < pos[x] + size[x]: five tables of N ints serve every prune edge of the call.
 *
 * The host groups the moves by p; a pass holds at most PLACE_MAX_ROWS moves of one prune edge, sorted by the preorder
 * position of u into records of SPR_REC ints:
 *     [0] position of u in the engine's order   [1] CSR edge e = (u -> b)   [2] index j of e among the call's distinct target edges:
 *     A is matrix 2 j, B matrix 2 j + 1   [3] plane row
 * Launch: a grid over the site chunk, one site per lane.  The first pass of a prune edge over a chunk stores the path
 * plane and F' (in the forward plane of the chunk, which nothing else reads); later passes of that edge read them.  The
 * lane that stores a vector is the lane that reads it back.
 */
#ifndef PLK_SPR_H
#define PLK_SPR_H

#define SPR_REC 4

struct SprOut {
    const int *rec;      /* [nrec][SPR_REC], sorted by rec[0] */
    int nrec;
    int store_fn;        /* 1: store the path plane and F' (the first pass of the prune edge over a chunk) */
    int p;               /* CSR edge (w -> x) */
    const int *pos, *size, *depth, *par, *in;   /* [N]: depth-first preorder position, subtree size, depth, parent, edge into the node (-1: root) */
    int EQ;              /* matrices per category of the call: 2 (distinct target edges) */
    const double *QP;    /* k = 4: [C][EQ][16] row-major */
    const double *QPT, *QPN;   /* generic: [C][EQ][K*K] transposed / plain */
    double *LP;          /* path plane: k = 4 [depth][C][n][4], generic [depth][C][k][n] */
    double *plane;       /* [rows][n] */
};

/* y is w or an ancestor of w (pw = preorder position of w) */
__device__ static inline bool spr_on_path(const SprOut &o, int y, int pw)
{
    const int py = as_uniform(o.pos)[y];
    return py <= pw && pw < py + as_uniform(o.size)[y];
}

/* message of the child behind CSR edge idx in the pruned tree: P L' for a child on the path, today's otherwise */
__device__ static inline v4 spr4_msg(const Up4Args &a, const SprOut &o, int pw, int c, int idx, long sg, long slc, const double *tipc,
                                     const PLK_AS4 double *Pm)
{
    const int b = as_uniform(a.indices)[idx];
    if (as_uniform(a.edge_tip)[idx] < 0 && spr_on_path(o, b, pw)) {
        const v4 x = ld4(o.LP + (((size_t)as_uniform(o.depth)[b] * a.C + c) * (size_t)a.n + slc) * 4);
        v4 m = mv4(Pm + ((size_t)c * a.E + idx) * 16, x);
        if (const4(x)) m = x;
        return m;
    }
    return nni4_msg(a, c, idx, sg, slc, tipc, Pm);
}

/*
 * k = 4, compact codes, at most four categories: the walk and launch shape of k_up4_place.  T is formed where it is
 * used (one stored vector and one 4 x 4 product per record and category) instead of being held across the walk.
 */
__global__ __launch_bounds__(UD4_BLOCK) void k_up4_spr(Up4Args a, SprOut o)
{
    const long sl = (long)blockIdx.x * UD4_BLOCK + threadIdx.x;
    const bool valid = sl < a.n;
    const long slc = valid ? sl : a.n - 1;
    const long sg = a.s0 + slc;
    const size_t n = (size_t)a.n;
    const PLK_AS4 int *pre = as_uniform(a.preorder), *ip = as_uniform(a.indptr), *ix = as_uniform(a.indices);
    const PLK_AS4 int *has = as_uniform(a.node_has_data), *etip = as_uniform(a.edge_tip);
    const PLK_AS4 int *nint = as_uniform(a.node_int), *nsc = as_uniform(a.node_scale);
    const PLK_AS4 int *rec = as_uniform(o.rec);
    const PLK_AS4 int *pos = as_uniform(o.pos), *size = as_uniform(o.size), *depth = as_uniform(o.depth);
    const PLK_AS4 int *par = as_uniform(o.par), *in = as_uniform(o.in);
    const PLK_AS4 double *Pm = as_uniform(a.P), *Qm = as_uniform(o.QP);
    const PLK_AS4 double *prior = as_uniform(a.cat_prior), *rw = as_uniform(a.root_w);
    const size_t tabc = (size_t)(a.ntips + 1) * a.nchar * 4;
    const int root = pre[0];
    const int x = ix[o.p], w = par[x];
    const int pw = pos[w], px = pos[x], sx = size[x];

    if (o.store_fn) {
        /* path: L' of w and of every node above it, on the factor the down pass chose */
        int skip = o.p;
        for (int y = w;;) {
            const int start = ip[y], stop = ip[y + 1];
            const bool hd = has[y] != 0;
            const int slot = nsc[y];
            const int cd = hd ? a.codes[(size_t)y * a.Spad + sg] : 0;
            for (int c = 0; c < a.C; c++) {
                const double *tipc = a.tip + (size_t)c * tabc;
                v4 acc = v4{1.0, 1.0, 1.0, 1.0};
                if (hd) acc = ld4(tipc + ((size_t)a.ntips * a.nchar + cd) * 4);
                for (int idx = start; idx < stop; idx++) {
                    if (idx == o.p) continue;
                    if (idx == skip) {
                        const v4 lc = ld4(o.LP + (((size_t)depth[ix[idx]] * a.C + c) * n + slc) * 4);
                        v4 m = mv4(Pm + ((size_t)c * a.E + idx) * 16, lc);
                        if (const4(lc)) m = lc;
                        acc = mul4(acc, m);
                    } else acc = mul4(acc, nni4_msg(a, c, idx, sg, slc, tipc, Pm));
                }
                if (slot >= 0) {
                    const double sc = a.SC[((size_t)slot * a.C + c) * n + slc];
                    acc.a *= sc; acc.b *= sc; acc.c *= sc; acc.d *= sc;
                }
                if (valid) st4(o.LP + (((size_t)depth[y] * a.C + c) * n + slc) * 4, acc);
            }
            if (in[y] < 0) break;
            skip = in[y];
            y = par[y];
        }
        if (valid) {
            const v4 r4 = v4{rw[0], rw[1], rw[2], rw[3]};
            for (int c = 0; c < a.C; c++) st4(a.FN + (((size_t)nint[root] * a.C + c) * n + slc) * 4, r4);
        }
    }

    int r = 0;
    for (int u = 0; u < a.N; u++) {
        if (!o.store_fn) {                                /* only the nodes the records name */
            if (r >= o.nrec) break;
            u = rec[r * SPR_REC];
        }
        const int nd = pre[u];
        if (o.store_fn && pos[nd] >= px && pos[nd] < px + sx) continue;     /* nothing below x is visited (no record names it) */
        const int start = ip[nd], stop = ip[nd + 1];
        if (start == stop) continue;
        const bool hd = has[nd] != 0;
        const int slot = nsc[nd];
        const double *fn_nd = a.FN + ((size_t)nint[nd] * a.C) * n * 4;
        const int cd_nd = hd ? a.codes[(size_t)nd * a.Spad + sg] : 0;

        /* forward vectors of the internal children in the pruned tree */
        if (o.store_fn) {
            for (int idx = start; idx < stop; idx++) {
                if (etip[idx] >= 0 || idx == o.p) continue;
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
                        if (idx2 == idx || idx2 == o.p) continue;
                        fe = mul4(fe, spr4_msg(a, o, pw, c, idx2, sg, slc, tipc, Pm));
                    }
                    if (valid) st4(a.FN + (((size_t)nint[b] * a.C + c) * n + slc) * 4, mtv4(Pm + ((size_t)c * a.E + idx) * 16, fe));
                }
            }
        }

        /* the moves of p onto the edges below nd */
        for (; r < o.nrec && rec[r * SPR_REC] == u; r++) {
            const int idx_b = rec[r * SPR_REC + 1], j = rec[r * SPR_REC + 2], row = rec[r * SPR_REC + 3];
            const int tb = etip[idx_b], b = ix[idx_b];
            const int cd_b = tb >= 0 ? a.codes[(size_t)b * a.Spad + sg] : 0;
            const bool b_path = tb < 0 && spr_on_path(o, b, pw);
            NniSum s = {0.0, 0, false};
            for (int c = 0; c < a.C; c++) {
                const double *tipc = a.tip + (size_t)c * tabc;
                int eb = (int)a.XC[(size_t)c * n + slc];
                /* G': what u holds in the pruned tree without the message of b */
                v4 G = ld4(fn_nd + ((size_t)c * n + slc) * 4);
                if (hd) G = mul4(G, ld4(tipc + ((size_t)a.ntips * a.nchar + cd_nd) * 4));
                if (slot >= 0) eb += ilogb(a.SC[((size_t)slot * a.C + c) * n + slc]);
                for (int idx2 = start; idx2 < stop; idx2++) {
                    if (idx2 == idx_b || idx2 == o.p) continue;
                    G = mul4(G, spr4_msg(a, o, pw, c, idx2, sg, slc, tipc, Pm));
                }
                eb += nni_norm4(G);
                const v4 H = mtv4(Qm + ((size_t)c * o.EQ + 2 * j) * 16, G);
                /* M = B L'_b, a constant vector unchanged */
                v4 L;
                if (tb >= 0) L = ld4(tipc + ((size_t)a.ntips * a.nchar + cd_b) * 4);
                else if (b_path) L = ld4(o.LP + (((size_t)depth[b] * a.C + c) * n + slc) * 4);
                else L = ld4(a.LN + (((size_t)nint[b] * a.C + c) * n + slc) * 4);
                v4 M = mv4(Qm + ((size_t)c * o.EQ + 2 * j + 1) * 16, L);
                if (const4(L)) M = L;
                eb += nni_norm4(M);
                const v4 W = mul4(H, M);
                /* T: the message the pruned subtree sends today */
                const v4 T = nni4_msg(a, c, o.p, sg, slc, tipc, Pm);
                double d = fma(W.d, T.d, fma(W.c, T.c, fma(W.b, T.b, W.a * T.a)));
                double sc;
                const int ed = nni_norm(d, sc);
                d *= sc;
                nni_sum_add(s, prior[c] * d, eb + ed);
            }
            if (valid) o.plane[(size_t)row * n + sl] = nni_sum_ll(s);
        }
    }
}

/* x *= message of the child behind CSR edge idx in the pruned tree (generic planes) */
template <int K>
__device__ static inline void spr_mul_msg(const UpArgs &a, const SprOut &o, int pw, int c, int idx, long sg, long slc, int tid,
                                          double (*xs)[GEN_BLOCK], double (&x)[K])
{
    const int b = as_uniform(a.indices)[idx];
    if (as_uniform(a.indptr)[b] != as_uniform(a.indptr)[b + 1] && spr_on_path(o, b, pw)) {
        const double *lp = o.LP + ((size_t)as_uniform(o.depth)[b] * a.C + c) * a.k * (size_t)a.n + slc;
        for (int jj = 0; jj < a.k; jj++) xs[jj][tid] = lp[(size_t)jj * a.n];
        nni_matvec_each<K>(a.PT + ((size_t)c * a.E + idx) * K * K, a.k, xs, tid, [&](int i, double m) { x[i] *= m; });
    } else nni_mul_msg<K>(a, c, idx, sg, slc, tid, xs, x);
}

/*
 * Every other state count, dense observations, more than four categories: the planes and stored edge vectors of
 * k_up_nni<K>, one wave per workgroup.  Two instantiations, so that neither holds the other's registers: FORWARD stores
 * the path plane and F' of a prune edge (once per chunk), the other evaluates a pass of its moves from them.  Correct
 * first: this kernel is not tuned.
 */
template <int K, bool FORWARD>
__global__ __launch_bounds__(GEN_BLOCK) void k_up_spr(UpArgs a, SprOut o)
{
    __shared__ double xs[K][GEN_BLOCK], ys[K][GEN_BLOCK];     /* a lane reads and writes its own column only */
    const int tid = threadIdx.x;
    const long sl = (long)blockIdx.x * GEN_BLOCK + tid;
    if (sl >= a.n) return;                               /* no barrier below; a lane past the chunk must not touch LP */
    const long slc = sl;
    const long sg = a.s0 + slc;
    const size_t n = (size_t)a.n;
    const int k = a.k;
    const PLK_AS4 int *rec = as_uniform(o.rec);
    const PLK_AS4 int *pre = as_uniform(a.preorder), *ip = as_uniform(a.indptr), *ix = as_uniform(a.indices);
    const PLK_AS4 int *pos = as_uniform(o.pos), *size = as_uniform(o.size), *depth = as_uniform(o.depth);
    const PLK_AS4 int *par = as_uniform(o.par), *in = as_uniform(o.in);
    const int root = pre[0];
    const int x = ix[o.p], w = par[x];
    const int pw = pos[w], px = pos[x], sx = size[x];

    if (FORWARD) {
        /* path: spr_mul_msg sends P L' for the child on the path, which the round before stored */
        for (int y = w;;) {
            const int start = ip[y], stop = ip[y + 1];
            const bool hd = as_uniform(a.node_has_data)[y];
            const int slot = a.node_scale ? as_uniform(a.node_scale)[y] : -1;
            for (int c = 0; c < a.C; c++) {
                double acc[K];
                if (hd) up_load_obs_reg<K>(a, y, sg, acc);
                else {
#pragma unroll
                    for (int i = 0; i < K; i++) acc[i] = i < k ? 1.0 : 0.0;
                }
                for (int idx = start; idx < stop; idx++) {
                    if (idx == o.p) continue;
                    spr_mul_msg<K>(a, o, pw, c, idx, sg, slc, tid, xs, acc);
                }
                if (slot >= 0) {
                    const double sc = a.SC[((size_t)slot * a.C + c) * n + slc];
#pragma unroll
                    for (int i = 0; i < K; i++) acc[i] *= sc;
                }
                double *lp = o.LP + ((size_t)depth[y] * a.C + c) * k * n + slc;
#pragma unroll
                for (int i = 0; i < K; i++)
                    if (i < k) lp[(size_t)i * n] = acc[i];
            }
            if (in[y] < 0) break;
            y = par[y];
        }
        for (int c = 0; c < a.C; c++) {
            double *fr = a.FN + ((size_t)root * a.C + c) * k * n + slc;
            for (int i = 0; i < k; i++) fr[(size_t)i * n] = as_uniform(a.root_w)[i];
        }
    }

    int r = 0;
    for (int u = 0; u < a.N; u++) {
        if (!FORWARD) {
            if (r >= o.nrec) break;
            u = rec[r * SPR_REC];
        }
        const int nd = pre[u];
        if (FORWARD && pos[nd] >= px && pos[nd] < px + sx) continue;
        const int start = ip[nd], stop = ip[nd + 1];
        if (start == stop) continue;
        const bool has = as_uniform(a.node_has_data)[nd];
        const int slot = a.node_scale ? as_uniform(a.node_scale)[nd] : -1;

        if (FORWARD) {
            for (int idx = start; idx < stop; idx++) {
                const int b = ix[idx];
                if (ip[b] == ip[b + 1] || idx == o.p) continue;
                for (int c = 0; c < a.C; c++) {
                    double fe[K];
                    const double *fa = a.FN + ((size_t)nd * a.C + c) * k * n + slc;
#pragma unroll
                    for (int i = 0; i < K; i++) fe[i] = i < k ? fa[(size_t)i * n] : 0.0;
                    if (has) {
                        double bnd[K];
                        up_load_obs_reg<K>(a, nd, sg, bnd);
#pragma unroll
                        for (int i = 0; i < K; i++) fe[i] *= bnd[i];
                    }
                    if (slot >= 0) {
                        const double sc = a.SC[((size_t)slot * a.C + c) * n + slc];
#pragma unroll
                        for (int i = 0; i < K; i++) fe[i] *= sc;
                    }
                    for (int idx2 = start; idx2 < stop; idx2++) {
                        if (idx2 == idx || idx2 == o.p) continue;
                        spr_mul_msg<K>(a, o, pw, c, idx2, sg, slc, tid, xs, fe);
                    }
#pragma unroll
                    for (int i = 0; i < K; i++) xs[i][tid] = fe[i];
                    double fb[K];
                    up_matvec<K, 0>(a.PN + ((size_t)c * a.E + idx) * K * K, k, xs, tid, fb);
                    double *fo = a.FN + ((size_t)b * a.C + c) * k * n + slc;
#pragma unroll
                    for (int i = 0; i < K; i++)
                        if (i < k) fo[(size_t)i * n] = fb[i];
                }
            }
        }

        for (; !FORWARD && r < o.nrec && rec[r * SPR_REC] == u; r++) {
            const int idx_b = rec[r * SPR_REC + 1], j = rec[r * SPR_REC + 2], row = rec[r * SPR_REC + 3];
            const int b = ix[idx_b];
            const bool b_leaf = ip[b] == ip[b + 1];
            const bool b_path = !b_leaf && spr_on_path(o, b, pw);
            NniSum s = {0.0, 0, false};
            for (int c = 0; c < a.C; c++) {
                long slo = slc, sgo = sg;                    /* opaque per category, as in k_up_nni */
                asm volatile("" : "+v"(slo), "+v"(sgo));
                int eb = a.XC ? (int)a.XC[(size_t)c * n + slo] : 0;
                /* M = B L'_b, then o T; the result waits in LDS (ys) while H is formed */
                {
                    double L[K];
                    if (b_leaf) up_load_obs_reg<K>(a, b, sgo, L);
                    else {
                        const double *ln = b_path ? o.LP + ((size_t)depth[b] * a.C + c) * k * n + slo
                                                  : a.LN + ((size_t)b * a.C + c) * k * n + slo;
#pragma unroll
                        for (int i = 0; i < K; i++) L[i] = i < k ? ln[(size_t)i * n] : 0.0;
                    }
#pragma unroll
                    for (int i = 0; i < K; i++) xs[i][tid] = L[i];
                    double M[K];
                    up_matvec<K, 1>(o.QPT + ((size_t)c * o.EQ + 2 * j + 1) * K * K, k, xs, tid, M);
                    eb += nni_normK<K>(M);
                    nni_mul_msg<K>(a, c, o.p, sgo, slo, tid, xs, M);
#pragma unroll
                    for (int i = 0; i < K; i++) ys[i][tid] = M[i];
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
                    if (idx2 == idx_b || idx2 == o.p) continue;
                    spr_mul_msg<K>(a, o, pw, c, idx2, sgo, slo, tid, xs, G);
                }
                eb += nni_normK<K>(G);
                /* H[j] = sum_i A[i][j] G[i], then the dot product with M o T */
#pragma unroll
                for (int i = 0; i < K; i++) xs[i][tid] = G[i];
                double H[K];
                up_matvec<K, 0>(o.QPN + ((size_t)c * o.EQ + 2 * j) * K * K, k, xs, tid, H);
                double d = 0.0;
#pragma unroll
                for (int i = 0; i < K; i++) d = fma(H[i], ys[i][tid], d);
                double sc;
                const int ed = nni_norm(d, sc);
                d *= sc;
                nni_sum_add(s, as_uniform(a.cat_prior)[c] * d, eb + ed);
            }
            o.plane[(size_t)row * n + sl] = nni_sum_ll(s);
        }
    }
}

#endif
