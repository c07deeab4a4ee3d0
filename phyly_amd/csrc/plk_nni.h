/*
 * plk_nni.h -- up passes of plk_nni_ll: the log likelihood of nearest-neighbour interchanges of the current tree from
 * the vectors one down pass leaves in device memory.  Included by plk_engine.hip.  The reference has no such pass.
 *
 * A swap is a pair of edges a = (v -> c), b = (u -> s) with v a child of u and s != v; the swapped tree has a = (u -> c)
 * and b = (v -> s).  Every edge keeps its index and its rate, so the message of a moved subtree is the vector it sends
 * today, m_c = P_a L_c and m_s = P_b L_s; only the products at u and v change.  Per site and category
 *     N'_c = sum_i (g o prod_{w child of u, w not in {v, s}} m_w o m_c)[i]
 *                  (P_v (data_v SC_v prod_{w child of v, w != c} m_w o m_s))[i],      g = F_u o data_u SC_u
 *     ll'  = log(sum_c prior_c N'_c 2^(X_c - E)) + E log 2
 * with F_u the forward vector the up pass stores (k_up4_pairsums / k_up_pairsums<K>, the same arithmetic here), X_c the
 * exponent the down pass accumulated for the category (XC) and E the largest exponent among the categories whose term
 * is not zero.  Nothing is divided by a message or by the likelihood of the current tree: a swapped tree may have
 * positive likelihood where the current one has none, and the other way round (ll' = -inf).
 *
 * Why the stored factors carry over.  A stored lower vector L_w holds the factors 2^-e of every rescaled node of its
 * subtree, w included; F_u holds those of every rescaled node outside the subtree of u; SC_u is applied to g as in every
 * up pass.  The swap moves whole subtrees and keeps u, v and everything else in place, so the product above takes each
 * rescaled node of the tree exactly once, as the root vector of the down pass does: N'_c sits at the exponent X_c of the
 * down pass, whatever the factors of u and v were chosen for.  They are exact powers of two; here they are added to the
 * exponent instead of multiplied in, which gives the same bits.
 *
 * Nodes without a slot.  plk_program_build rescales a node once 16 edge factors have accumulated, so a stored vector
 * holds at most 15 unscaled factors and a product of two children at most PLK_SCALE_RUN = 32.  A swap replaces the
 * message of c in v's product by that of s: up to 32 - 1 + 16 = 47 factors, past that bound.  And the vector above
 * (u -> v), which today meets the whole message of v, meets m_c alone.  So both rebuilt products are rescaled inside:
 * the part that stays (g and the other children of u; data_v and the other children of v) is brought to [1, 2) by an
 * exact power of two before the moved message is multiplied in, and the dot product once more; the three exponents join
 * X_c.  Each part is a product the current tree forms too (at most PLK_SCALE_RUN factors, or range-checked by
 * check_stored_range before the query runs, as for every stored-vector query), so with these three steps the swap
 * stays as far inside the double range as the passes of the current tree.
 *
 * Launch: a grid over the site chunk, one site per lane, as k_up4 / k_up.  The pair-sum passes run on a fixed grid
 * because they reduce over sites inside the kernel and want partial sums whose number does not grow with S; this pass
 * reduces nothing -- every value goes to its site's place in a [swaps of this pass][n] plane -- so a batch loop would
 * only add a loop.  The site sums are the weighted double-double row sums of that plane (wsum_rows), whose order the
 * launch geometry of that kernel fixes.  The lane that stores a forward vector is the lane that reads it back.
 *
 * The host sorts the swaps of a pass by the preorder position of u into records of NNI_REC ints:
 *     [0] preorder position of u   [1] CSR edge (u -> v)   [2] CSR edge b = (u -> s)
 *     [3] CSR edge a1 = (v -> c1)  [4] plane row of (a1, b) or -1
 *     [5] CSR edge a2 = (v -> c2) or -1   [6] plane row of (a2, b) or -1
 * Where u and v both have two children, both swaps of the edge (u -> v) share one record -- F_u, L_s, L_c1 and L_c2 are
 * read once per category -- and such swaps ALWAYS go through a record of that form, asked for together or not, so a
 * swap has the same bits in every list.  Every other degree takes one swap per record with the messages recomputed.
 */
#ifndef PLK_NNI_H
#define PLK_NNI_H

#define NNI_REC 8
#define NNI_MAX_ROWS 256          /* swaps per up pass: rows of the per-site plane */

struct NniOut {
    const int *rec;      /* [nrec][NNI_REC], sorted by rec[0] */
    int nrec;
    int store_fn;        /* 1: store the forward vectors (the first pass over a chunk); later passes read them */
    double *plane;       /* [rows][n] */
};

/* the running sum over categories of terms t 2^e, kept at the largest exponent (the ll kernels' rule) */
struct NniSum {
    double sum;
    int e;
    bool have;
};

__device__ static inline void nni_sum_add(NniSum &s, double term, int e)
{
    if (term == 0.0) return;
    if (!s.have) { s.sum = term; s.e = e; s.have = true; }
    else if (e > s.e) { s.sum = ldexp(s.sum, s.e - e) + term; s.e = e; }
    else s.sum += ldexp(term, e - s.e);
}

__device__ static inline double nni_sum_ll(const NniSum &s)
{
    return s.have ? log(s.sum) + (double)s.e * 0.6931471805599453094 : -INFINITY;
}

/* exponent e of the largest entry mx and the factor 2^-e that brings it to [1, 2); 0 and 1 for a zero or non-finite mx */
__device__ static inline int nni_norm(double mx, double &sc)
{
    sc = 1.0;
    if (!(mx > 0.0 && mx < INFINITY)) return 0;
    const int e = ilogb(mx);
    /* 2^-e in two steps: e reaches -1074 for a subnormal entry, where 2^1074 is no double */
    sc = e < -1000 ? 0x1p+1000 : ldexp(1.0, -e);
    return e < -1000 ? -1000 : e;
}

__device__ static inline int nni_norm4(v4 &x)
{
    double sc;
    const int e = nni_norm(fmax(fmax(x.a, x.b), fmax(x.c, x.d)), sc);
    x.a *= sc; x.b *= sc; x.c *= sc; x.d *= sc;
    return e;
}

/* lower vector of the child behind CSR edge idx: its row of the definition unit for a leaf, the stored L otherwise */
__device__ static inline v4 nni4_msg(const Up4Args &a, int c, int idx, long sg, long slc, const double *tipc, const PLK_AS4 double *Pm)
{
    const int t = as_uniform(a.edge_tip)[idx], b = as_uniform(a.indices)[idx];
    v4 x = v4{0.0, 0.0, 0.0, 0.0};
    int code = 0;
    if (t >= 0) code = a.codes[(size_t)b * a.Spad + sg];
    else x = ld4(a.LN + (((size_t)as_uniform(a.node_int)[b] * a.C + c) * (size_t)a.n + slc) * 4);
    return ud4_child_msg(a, c, idx, t, code, tipc, Pm, x);
}

/* one swap of one category: A = (what stays at u, in [1, 2)) o m_c, B = P_v ((what stays at v, in [1, 2)) o m_s);
 * the term prior_c A.B joins the sum at exponent ebase + (exponent of the dot product) */
__device__ static inline void nni4_term(NniSum &s, const v4 &A0, const v4 &mc, const v4 &B0, const v4 &ms,
                                        const PLK_AS4 double *Pv, double prior, int ebase)
{
    const v4 A = mul4(A0, mc);
    const v4 B1 = mul4(B0, ms);
    v4 B = mv4(Pv, B1);
    if (const4(B1)) B = B1;
    double d = fma(A.d, B.d, fma(A.c, B.c, fma(A.b, B.b, A.a * B.a)));
    double sc;
    const int ed = nni_norm(d, sc);
    d *= sc;
    nni_sum_add(s, prior * d, ebase + ed);
}

/*
 * k = 4, compact codes, at most four categories: k_up4_pairsums' walk (interleaved LN / FN, SC, tip tables for the leaf
 * messages, the definition unit for observations at internal nodes) with the swaps of a node in place of its outer
 * products.  Leaf messages come from the edge units of the tip table, so no leaf vector is needed on its own.
 */
__global__ __launch_bounds__(UD4_BLOCK) void k_up4_nni(Up4Args a, NniOut o)
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
    const PLK_AS4 double *Pm = as_uniform(a.P);
    const PLK_AS4 double *prior = as_uniform(a.cat_prior), *rw = as_uniform(a.root_w);
    const size_t tabc = (size_t)(a.ntips + 1) * a.nchar * 4;
    const int root = pre[0];

    if (o.store_fn && valid) {
        const v4 w = v4{rw[0], rw[1], rw[2], rw[3]};
        for (int c = 0; c < a.C; c++) st4(a.FN + (((size_t)nint[root] * a.C + c) * n + slc) * 4, w);
    }

    int r = 0;
    for (int u = 0; u < a.N; u++) {
        const int nd = pre[u];
        const int start = ip[nd], stop = ip[nd + 1];
        if (start == stop) continue;
        const bool hd = has[nd] != 0;
        const int slot = nsc[nd];
        const double *fn_nd = a.FN + ((size_t)nint[nd] * a.C) * n * 4;
        const int cd_nd = hd ? a.codes[(size_t)nd * a.Spad + sg] : 0;

        /* forward vectors of the internal children: F_b = P_e^T (g o messages of the other children), as k_up4_pairsums */
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

        /* the swaps whose upper node is nd */
        for (; r < o.nrec && rec[r * NNI_REC] == u; r++) {
            const int idx_v = rec[r * NNI_REC + 1], idx_s = rec[r * NNI_REC + 2];
            const int idx_c1 = rec[r * NNI_REC + 3], row1 = rec[r * NNI_REC + 4];
            const int idx_c2 = rec[r * NNI_REC + 5], row2 = rec[r * NNI_REC + 6];
            const bool two = idx_c2 >= 0;
            const int v = ix[idx_v];
            const int vstart = ip[v], vstop = ip[v + 1];
            const bool vhd = has[v] != 0;
            const int vslot = nsc[v];
            const int cd_v = vhd ? a.codes[(size_t)v * a.Spad + sg] : 0;
            NniSum s1 = {0.0, 0, false}, s2 = {0.0, 0, false};
            for (int c = 0; c < a.C; c++) {
                const double *tipc = a.tip + (size_t)c * tabc;
                int eb = (int)a.XC[(size_t)c * n + slc];
                /* what stays at u */
                v4 A0 = ld4(fn_nd + ((size_t)c * n + slc) * 4);
                if (hd) A0 = mul4(A0, ld4(tipc + ((size_t)a.ntips * a.nchar + cd_nd) * 4));
                if (slot >= 0) eb += ilogb(a.SC[((size_t)slot * a.C + c) * n + slc]);
                for (int idx2 = start; idx2 < stop; idx2++) {
                    if (idx2 == idx_v || idx2 == idx_s) continue;
                    A0 = mul4(A0, nni4_msg(a, c, idx2, sg, slc, tipc, Pm));
                }
                eb += nni_norm4(A0);
                /* what stays at v (a record of two swaps: v has the two children c1 and c2, and nothing else stays) */
                v4 B0 = v4{1.0, 1.0, 1.0, 1.0};
                if (vhd) B0 = ld4(tipc + ((size_t)a.ntips * a.nchar + cd_v) * 4);
                if (vslot >= 0) eb += ilogb(a.SC[((size_t)vslot * a.C + c) * n + slc]);
                if (!two)
                    for (int idx2 = vstart; idx2 < vstop; idx2++) {
                        if (idx2 == idx_c1) continue;
                        B0 = mul4(B0, nni4_msg(a, c, idx2, sg, slc, tipc, Pm));
                    }
                const v4 ms = nni4_msg(a, c, idx_s, sg, slc, tipc, Pm);
                const v4 mc1 = nni4_msg(a, c, idx_c1, sg, slc, tipc, Pm);
                const PLK_AS4 double *Pv = Pm + ((size_t)c * a.E + idx_v) * 16;
                if (two) {
                    const v4 mc2 = nni4_msg(a, c, idx_c2, sg, slc, tipc, Pm);
                    v4 B01 = mul4(B0, mc2), B02 = mul4(B0, mc1);
                    const int e1 = nni_norm4(B01), e2 = nni_norm4(B02);
                    nni4_term(s1, A0, mc1, B01, ms, Pv, prior[c], eb + e1);
                    nni4_term(s2, A0, mc2, B02, ms, Pv, prior[c], eb + e2);
                } else {
                    const int e1 = nni_norm4(B0);
                    nni4_term(s1, A0, mc1, B0, ms, Pv, prior[c], eb + e1);
                }
            }
            if (valid && row1 >= 0) o.plane[(size_t)row1 * n + sl] = nni_sum_ll(s1);
            if (valid && two && row2 >= 0) o.plane[(size_t)row2 * n + sl] = nni_sum_ll(s2);
        }
    }
}

template <int K>
__device__ static inline int nni_normK(double (&x)[K])
{
    double mx = 0.0;
#pragma unroll
    for (int i = 0; i < K; i++) mx = fmax(mx, x[i]);
    double sc;
    const int e = nni_norm(mx, sc);
#pragma unroll
    for (int i = 0; i < K; i++) x[i] *= sc;
    return e;
}

/* y[i] = sum_j M[j*K+i] xs[j] one entry at a time (up_matvec's sums in up_matvec's order, CONST_MODE 1: a constant input
 * maps to itself), so that no vector of K accumulators is held next to the caller's: F(i, y_i) takes each entry */
template <int K, typename F>
__device__ static inline void nni_matvec_each(const double *M, int k, double (*xs)[GEN_BLOCK], int tid, F &&f)
{
    const double x0 = xs[0][tid];
    bool is_const = true;
    for (int j = 1; j < k; j++) is_const = is_const && (xs[j][tid] == x0);
#pragma unroll
    for (int i = 0; i < K; i++) {
        double m = 0.0;
        for (int j = 0; j < k; j++) m = fma(M[j * K + i], xs[j][tid], m);
        if (is_const) m = i < k ? x0 : 0.0;
        f(i, m);
    }
}

/* x *= message of the child behind CSR edge idx: the stored edge vector, or P_e B_b for a leaf */
template <int K>
__device__ static inline void nni_mul_msg(const UpArgs &a, int c, int idx, long sg, long slc, int tid, double (*xs)[GEN_BLOCK], double (&x)[K])
{
    const int b = as_uniform(a.indices)[idx];
    if (as_uniform(a.indptr)[b] == as_uniform(a.indptr)[b + 1]) {
        up_stage_obs<K>(a, b, sg, tid, xs);
        nni_matvec_each<K>(a.PT + ((size_t)c * a.E + idx) * K * K, a.k, xs, tid, [&](int i, double m) { x[i] *= m; });
    } else {
        const double *ev = a.EV + ((size_t)idx * a.C + c) * a.k * (size_t)a.n + slc;
#pragma unroll
        for (int i = 0; i < K; i++)
            if (i < a.k) x[i] *= ev[(size_t)i * a.n];
    }
}

/*
 * Every other state count, dense observations, more than four categories: k_up_pairsums<K>'s planes
 * ([entity][category][state][site]) and stored edge vectors, one swap per record ([5] and [6] are not read), one wave per
 * workgroup.  Two launches, so that neither holds the other's registers: FORWARD stores the forward vectors of a chunk
 * (once), the other instantiation evaluates a group of swaps from them.  Correct first: this kernel is not tuned.
 */
template <int K, bool FORWARD>
__global__ __launch_bounds__(GEN_BLOCK) void k_up_nni(UpArgs a, NniOut o)
{
    __shared__ double xs[K][GEN_BLOCK], ys[K][GEN_BLOCK];     /* a lane reads and writes its own column only */
    const int tid = threadIdx.x;
    const long sl = (long)blockIdx.x * GEN_BLOCK + tid;
    const bool valid = sl < a.n;
    const long slc = valid ? sl : a.n - 1;
    const long sg = a.s0 + slc;
    const size_t n = (size_t)a.n;
    const int k = a.k;
    const int root = as_uniform(a.preorder)[0];
    const PLK_AS4 int *rec = as_uniform(o.rec);

    if (FORWARD && valid)
        for (int c = 0; c < a.C; c++) {
            double *fr = a.FN + ((size_t)root * a.C + c) * k * n + slc;
            for (int i = 0; i < k; i++) fr[(size_t)i * n] = as_uniform(a.root_w)[i];
        }

    int r = 0;
    for (int u = 0; u < a.N; u++) {
        const int nd = as_uniform(a.preorder)[u];
        const int start = as_uniform(a.indptr)[nd], stop = as_uniform(a.indptr)[nd + 1];
        if (start == stop) continue;
        const bool has = as_uniform(a.node_has_data)[nd];
        const int slot = a.node_scale ? as_uniform(a.node_scale)[nd] : -1;

        if (FORWARD) {
            for (int idx = start; idx < stop; idx++) {
                const int b = as_uniform(a.indices)[idx];
                if (as_uniform(a.indptr)[b] == as_uniform(a.indptr)[b + 1]) continue;
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
                        if (idx2 == idx) continue;
                        nni_mul_msg<K>(a, c, idx2, sg, slc, tid, xs, fe);
                    }
                    /* F_b[j] = sum_i P[i][j] fe[i] */
#pragma unroll
                    for (int i = 0; i < K; i++) xs[i][tid] = fe[i];
                    double fb[K];
                    up_matvec<K, 0>(a.PN + ((size_t)c * a.E + idx) * K * K, k, xs, tid, fb);
                    double *fo = a.FN + ((size_t)b * a.C + c) * k * n + slc;
#pragma unroll
                    for (int i = 0; i < K; i++)
                        if (i < k && valid) fo[(size_t)i * n] = fb[i];
                }
            }
        }

        for (; !FORWARD && r < o.nrec && rec[r * NNI_REC] == u; r++) {
            const int idx_v = rec[r * NNI_REC + 1], idx_s = rec[r * NNI_REC + 2];
            const int idx_c = rec[r * NNI_REC + 3], row = rec[r * NNI_REC + 4];
            const int v = as_uniform(a.indices)[idx_v];
            const int vstart = as_uniform(a.indptr)[v], vstop = as_uniform(a.indptr)[v + 1];
            const bool vhas = as_uniform(a.node_has_data)[v];
            const int vslot = a.node_scale ? as_uniform(a.node_scale)[v] : -1;
            NniSum s = {0.0, 0, false};
            for (int c = 0; c < a.C; c++) {
                /* the lane's site indices made opaque per category: the compiler otherwise keeps the 2 K row addresses of
                 * both sides (128 VGPRs at K = 64) alive across the category loop and spills */
                long slo = slc, sgo = sg;
                asm volatile("" : "+v"(slo), "+v"(sgo));
                int eb = a.XC ? (int)a.XC[(size_t)c * n + slo] : 0;
                /* what stays at v, then the message of s, then P_v; the result waits in LDS (ys) while the other side is
                 * formed, so that at most two vectors of K doubles are in registers at a time */
                {
                    double B[K];
                    if (vhas) up_load_obs_reg<K>(a, v, sgo, B);
                    else {
#pragma unroll
                        for (int i = 0; i < K; i++) B[i] = i < k ? 1.0 : 0.0;
                    }
                    if (vslot >= 0) eb += ilogb(a.SC[((size_t)vslot * a.C + c) * n + slo]);
                    for (int idx2 = vstart; idx2 < vstop; idx2++) {
                        if (idx2 == idx_c) continue;
                        nni_mul_msg<K>(a, c, idx2, sgo, slo, tid, xs, B);
                    }
                    eb += nni_normK<K>(B);
                    nni_mul_msg<K>(a, c, idx_s, sgo, slo, tid, xs, B);
#pragma unroll
                    for (int i = 0; i < K; i++) xs[i][tid] = B[i];
                    nni_matvec_each<K>(a.PT + ((size_t)c * a.E + idx_v) * K * K, k, xs, tid, [&](int i, double m) { ys[i][tid] = m; });
                }
                /* what stays at u, then the message of c */
                double A[K];
                const double *fa = a.FN + ((size_t)nd * a.C + c) * k * n + slo;
#pragma unroll
                for (int i = 0; i < K; i++) A[i] = i < k ? fa[(size_t)i * n] : 0.0;
                if (has) {
                    double bnd[K];
                    up_load_obs_reg<K>(a, nd, sgo, bnd);
#pragma unroll
                    for (int i = 0; i < K; i++) A[i] *= bnd[i];
                }
                if (slot >= 0) eb += ilogb(a.SC[((size_t)slot * a.C + c) * n + slo]);
                for (int idx2 = start; idx2 < stop; idx2++) {
                    if (idx2 == idx_v || idx2 == idx_s) continue;
                    nni_mul_msg<K>(a, c, idx2, sgo, slo, tid, xs, A);
                }
                eb += nni_normK<K>(A);
                nni_mul_msg<K>(a, c, idx_c, sgo, slo, tid, xs, A);
                double d = 0.0;
#pragma unroll
                for (int i = 0; i < K; i++) d = fma(A[i], ys[i][tid], d);
                double sc;
                const int ed = nni_norm(d, sc);
                d *= sc;
                nni_sum_add(s, as_uniform(a.cat_prior)[c] * d, eb + ed);
            }
            if (valid && row >= 0) o.plane[(size_t)row * n + sl] = nni_sum_ll(s);
        }
    }
}

#endif
