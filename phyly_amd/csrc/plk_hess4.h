/*
 * plk_hess4.h -- down and up pass of edge-modified models for k = 4 with compact character data: the
 * second-order pass of plk_second_order / plk_hess.  Included by plk_engine.hip after plk_updown4.h, whose
 * register form (v4, ld4, st4, mv4, mtv4) and interleaved vector layout [(entity * C + c)][site][4] it shares.
 *
 * Row j of the likelihood Hessian is the derivative pass of a model in which edge j carries dP_j = r Q P_j in the
 * role of P_j and d2P_j = r^2 Q Q P_j in the role of dP_j (src/arbplfhess.c:343-437 substitutes Q along both root
 * paths; here for all i at once).  The kernels do exactly what k_down_store / k_up do under UpArgs.mod_edge, with
 *   - one thread per site, all categories of the site in the thread, no LDS; matrices are wave-uniform scalar
 *     operands, leaf-edge messages rows of the tip tables of P, dP and d2P (k_build_tip / k_build_dtip4);
 *   - NM modified models per launch: pattern codes, matrices and table rows are fetched once per node visit and
 *     serve NM rows of the Hessian; only the node vectors are per model;
 *   - rescaling by exact powers of two taken from max |.| (the vectors of a modified model are not sign
 *     definite), the factors stored per model, node and category; the common exponent of every model is
 *     reconciled with that of the unmodified one in the division by its likelihood.
 * mod[m] = -1 evaluates the model itself (pass 0: f and g / f).
 */
#ifndef PLK_HESS4_H
#define PLK_HESS4_H

#define H4_MAX_NM 4

struct Hess4Args {
    long Spad, s0, n;
    int N, E, C, nchar, ntips, root_mode;
    int mod[H4_MAX_NM];            /* CSR edge modified in model m, -1: none */
    const int *indptr, *indices, *preorder;
    const int *node_has_data, *edge_tip, *node_int, *node_scale;
    const double *P, *dP, *d2P;    /* [C][E][4][4] row-major */
    const double *tip, *dtip, *d2tip;   /* [C][ntips+1][nchar][4]; slot ntips of tip = raw definitions */
    const uint8_t *codes;
    const double *cat_prior, *root_w;
    /* per model m: base + m * stride */
    double *LN, *FN; size_t vstride;    /* [(ent*C + c)][n][4] */
    double *SC; size_t scstride;        /* [(slot*C + c)][n]: 2^-e applied to L_a at rescaled nodes */
    double *CW, *XC;                    /* [C][n] (stride C*n): 2^(X_c - Xmax); X_c */
    double *XM, *LH;                    /* [n] (stride n): Xmax; likelihood at 2^Xmax */
    double *DV;                         /* [E][n] (stride E*n) */
    const double *LHdiv, *XMdiv;        /* [n]: likelihood and Xmax of the unmodified model; null = the model's own (pass 0) */
};

__device__ static inline double h4_maxabs(const v4 &x)
{
    return fmax(fmax(fabs(x.a), fabs(x.b)), fmax(fabs(x.c), fabs(x.d)));
}
__device__ static inline double dot4(const v4 &x, const v4 &y)
{
    return fma(x.d, y.d, fma(x.c, y.c, fma(x.b, y.b, x.a * y.a)));
}

/* message of edge idx towards its parent: P_e L_b, or dP_e L_b on the modified edge.  Leaf edges: a table row.  A
 * constant L_b maps to itself under P (src/util.c:276-283) and to zero under dP (zero row sums, src/util.c:338-345);
 * both rules are exact whatever model L_b comes from. */
__device__ static inline v4 h4_msg(const Hess4Args &a, int c, size_t tabc, int idx, int t, unsigned row, bool mod, const v4 &x)
{
    if (t >= 0) return ld4((mod ? a.dtip : a.tip) + (size_t)c * tabc + (size_t)t * a.nchar * 4 + row);
    const PLK_AS4 double *M = as_uniform(mod ? a.dP : a.P) + ((size_t)c * a.E + idx) * 16;
    v4 m = mv4(M, x);
    if (const4(x)) m = mod ? v4{0.0, 0.0, 0.0, 0.0} : x;
    return m;
}
/* edge form of edge idx: dP_e L_b, or d2P_e L_b on the modified edge (both matrices have zero row sums) */
__device__ static inline v4 h4_form(const Hess4Args &a, int c, size_t tabc, int idx, int t, unsigned row, bool mod, const v4 &x)
{
    if (t >= 0) return ld4((mod ? a.d2tip : a.dtip) + (size_t)c * tabc + (size_t)t * a.nchar * 4 + row);
    if (const4(x)) return v4{0.0, 0.0, 0.0, 0.0};
    return mv4(as_uniform(mod ? a.d2P : a.dP) + ((size_t)c * a.E + idx) * 16, x);
}

template <int NM>
__global__ __launch_bounds__(UD4_BLOCK) void k_hess4_down(Hess4Args a)
{
    const long sl = (long)blockIdx.x * UD4_BLOCK + threadIdx.x;
    const bool valid = sl < a.n;
    const long slc = valid ? sl : a.n - 1;
    const long sg = a.s0 + slc;
    const size_t n = (size_t)a.n;
    const PLK_AS4 int *pre = as_uniform(a.preorder), *ip = as_uniform(a.indptr), *ix = as_uniform(a.indices);
    const PLK_AS4 int *has = as_uniform(a.node_has_data), *etip = as_uniform(a.edge_tip);
    const PLK_AS4 int *nint = as_uniform(a.node_int), *nsc = as_uniform(a.node_scale);
    const PLK_AS4 double *prior = as_uniform(a.cat_prior), *rw = as_uniform(a.root_w);
    const size_t tabc = (size_t)(a.ntips + 1) * a.nchar * 4;
    int xmax[NM], xall[NM];
#pragma unroll
    for (int m = 0; m < NM; m++) xmax[m] = xall[m] = INT_MIN;
    for (int c = 0; c < a.C; c++) {
        double lh_c[NM];
        int X[NM];
#pragma unroll
        for (int m = 0; m < NM; m++) { lh_c[m] = 0.0; X[m] = 0; }
        for (int u = a.N - 1; u >= 0; u--) {
            const int nd = pre[u];
            const int start = ip[nd], stop = ip[nd + 1];
            if (start == stop) continue;
            v4 acc[NM];
            {
                v4 ob = v4{1.0, 1.0, 1.0, 1.0};
                if (has[nd]) ob = ld4(a.tip + (size_t)c * tabc + ((size_t)a.ntips * a.nchar + a.codes[(size_t)nd * a.Spad + sg]) * 4);
#pragma unroll
                for (int m = 0; m < NM; m++) acc[m] = ob;
            }
            for (int idx = start; idx < stop; idx++) {
                const int b = ix[idx];
                const int t = etip[idx];
                const unsigned row = t >= 0 ? 4u * a.codes[(size_t)b * a.Spad + sg] : 0u;
                v4 shared = v4{0.0, 0.0, 0.0, 0.0};
                if (t >= 0) shared = ld4(a.tip + (size_t)c * tabc + (size_t)t * a.nchar * 4 + row);
#pragma unroll
                for (int m = 0; m < NM; m++) {
                    const bool mod = idx == a.mod[m];
                    v4 msg = shared;
                    if (t < 0 || mod) {
                        v4 x = v4{0.0, 0.0, 0.0, 0.0};
                        if (t < 0) x = ld4(a.LN + m * a.vstride + (((size_t)nint[b] * a.C + c) * n + slc) * 4);
                        msg = h4_msg(a, c, tabc, idx, t, row, mod, x);
                    }
                    acc[m] = mul4(acc[m], msg);
                }
            }
            const int slot = nsc[nd];
#pragma unroll
            for (int m = 0; m < NM; m++) {
                if (slot >= 0) {
                    const double mx = h4_maxabs(acc[m]);
                    double sc = 1.0;
                    if (mx > 0x1p-1000 && mx < 0x1p+1000) {
                        const int e = ilogb(mx);
                        sc = ldexp(1.0, -e);
                        acc[m].a *= sc; acc[m].b *= sc; acc[m].c *= sc; acc[m].d *= sc;
                        X[m] += e;
                    }
                    if (valid) a.SC[m * a.scstride + ((size_t)slot * a.C + c) * n + slc] = sc;
                }
                if (valid) st4(a.LN + m * a.vstride + (((size_t)nint[nd] * a.C + c) * n + slc) * 4, acc[m]);
                if (u == 0) {
                    const v4 &r = acc[m];
                    if (a.root_mode == PLK_ROOT_NONE) lh_c[m] = ((r.a + r.b) + r.c) + r.d;
                    else if (a.root_mode == PLK_ROOT_UNIFORM) lh_c[m] = (((r.a + r.b) + r.c) + r.d) * 0.25;
                    else lh_c[m] = fma(rw[3], r.d, fma(rw[2], r.c, fma(rw[1], r.b, rw[0] * r.a)));
                }
            }
        }
#pragma unroll
        for (int m = 0; m < NM; m++) {
            const double l = lh_c[m] * prior[c];
            if (l != 0.0 && X[m] > xmax[m]) xmax[m] = X[m];
            if (X[m] > xall[m]) xall[m] = X[m];
            if (valid) {
                a.XC[((size_t)m * a.C + c) * n + slc] = (double)X[m];
                a.CW[((size_t)m * a.C + c) * n + slc] = l;
            }
        }
    }
    /* combine the categories at the largest exponent: LH = sum_c prior_c lh_c 2^(X_c - Xmax).  When every term is zero
     * (the site does not depend on the modified edge) the exponent of the vectors themselves is kept, so that the
     * division by the unmodified likelihood stays finite.  As in k_down_store, a category whose own root term is exactly
     * zero (dP maps a constant vector to zero) takes no part in Xmax: were its X_c more than 1023 above Xmax, its weight
     * 2^(X_c - Xmax) would overflow and be used by the up pass.  No known input reaches this; a clamp belongs in both
     * kernels at once, so that the two paths keep agreeing. */
    if (valid) {
#pragma unroll
        for (int m = 0; m < NM; m++) {
            int xm = xmax[m];
            if (xm == INT_MIN) xm = xall[m] == INT_MIN ? 0 : xall[m];
            double lh_total = 0.0;
            for (int c = 0; c < a.C; c++) {
                const size_t o = ((size_t)m * a.C + c) * n + slc;
                const double w = ldexp(1.0, (int)a.XC[o] - xm);
                lh_total = fma(a.CW[o], w, lh_total);
                a.CW[o] = w;
            }
            a.XM[(size_t)m * n + slc] = (double)xm;
            a.LH[(size_t)m * n + slc] = lh_total;
        }
    }
}

/*
 * up pass in BFS order (the formulas of k_up4).  For every edge e = (a -> b) of model m with modified edge j:
 *   fe  = F_a o B_a o s_a o prod_{siblings} message          F_b = (e == j ? dP_e : P_e)^T fe
 *   d_e = sum_c prior_c 2^(X_c - Xmax) fe . (e == j ? d2P_e : dP_e) L_b / f
 * with f the likelihood of the unmodified model, brought to this model's exponent.
 */
template <int NM>
__global__ __launch_bounds__(UD4_BLOCK) void k_hess4_up(Hess4Args a)
{
    const long sl = (long)blockIdx.x * UD4_BLOCK + threadIdx.x;
    const bool valid = sl < a.n;
    const long slc = valid ? sl : a.n - 1;
    const long sg = a.s0 + slc;
    const size_t n = (size_t)a.n;
    const PLK_AS4 int *pre = as_uniform(a.preorder), *ip = as_uniform(a.indptr), *ix = as_uniform(a.indices);
    const PLK_AS4 int *has = as_uniform(a.node_has_data), *etip = as_uniform(a.edge_tip);
    const PLK_AS4 int *nint = as_uniform(a.node_int), *nsc = as_uniform(a.node_scale);
    const PLK_AS4 double *prior = as_uniform(a.cat_prior), *rw = as_uniform(a.root_w);
    const size_t tabc = (size_t)(a.ntips + 1) * a.nchar * 4;
    const v4 zero = v4{0.0, 0.0, 0.0, 0.0};
    double inv[NM];
#pragma unroll
    for (int m = 0; m < NM; m++) {
        const double f = a.LHdiv ? a.LHdiv[slc] : a.LH[(size_t)m * n + slc];
        inv[m] = 1.0 / f;
        if (a.XMdiv) inv[m] = ldexp(inv[m], (int)(a.XM[(size_t)m * n + slc] - a.XMdiv[slc]));
    }
    const int root = pre[0];
    {
        const v4 w = v4{rw[0], rw[1], rw[2], rw[3]};
        if (valid)
            for (int c = 0; c < a.C; c++)
#pragma unroll
                for (int m = 0; m < NM; m++) st4(a.FN + m * a.vstride + (((size_t)nint[root] * a.C + c) * n + slc) * 4, w);
    }
    for (int u = 0; u < a.N; u++) {
        const int nd = pre[u];
        const int start = ip[nd], stop = ip[nd + 1];
        const int deg = stop - start;
        if (deg == 0) continue;
        const bool hd = has[nd] != 0;
        const unsigned rown = hd ? 4u * a.codes[(size_t)nd * a.Spad + sg] : 0u;
        const int slot = nsc[nd];
        const size_t vnd = (size_t)nint[nd] * a.C;

        if (deg <= 2) {
            /* both children together: F_a, L_b0 and L_b1 are read once per model, no message is computed twice */
            const int i0 = start, i1 = deg == 2 ? start + 1 : start;
            const int b0 = ix[i0], b1 = ix[i1];
            const int t0 = etip[i0], t1 = etip[i1];
            const unsigned r0 = t0 >= 0 ? 4u * a.codes[(size_t)b0 * a.Spad + sg] : 0u;
            const unsigned r1 = t1 >= 0 ? 4u * a.codes[(size_t)b1 * a.Spad + sg] : 0u;
            double d0[NM], d1[NM];
#pragma unroll
            for (int m = 0; m < NM; m++) d0[m] = d1[m] = 0.0;
            for (int c = 0; c < a.C; c++) {
                v4 ob = v4{1.0, 1.0, 1.0, 1.0};
                if (hd) ob = ld4(a.tip + (size_t)c * tabc + (size_t)a.ntips * a.nchar * 4 + rown);
                /* table rows of the unmodified leaf edges serve every model */
                v4 s0 = zero, s1 = zero, y0 = zero, y1 = zero;
                if (t0 >= 0) { s0 = ld4(a.tip + (size_t)c * tabc + (size_t)t0 * a.nchar * 4 + r0); y0 = ld4(a.dtip + (size_t)c * tabc + (size_t)t0 * a.nchar * 4 + r0); }
                if (deg == 2 && t1 >= 0) { s1 = ld4(a.tip + (size_t)c * tabc + (size_t)t1 * a.nchar * 4 + r1); y1 = ld4(a.dtip + (size_t)c * tabc + (size_t)t1 * a.nchar * 4 + r1); }
#pragma unroll
                for (int m = 0; m < NM; m++) {
                    const bool mod0 = i0 == a.mod[m], mod1 = deg == 2 && i1 == a.mod[m];
                    v4 g = mul4(ld4(a.FN + m * a.vstride + ((vnd + c) * n + slc) * 4), ob);
                    if (slot >= 0) {
                        const double sc = a.SC[m * a.scstride + ((size_t)slot * a.C + c) * n + slc];
                        g.a *= sc; g.b *= sc; g.c *= sc; g.d *= sc;
                    }
                    const double pc = prior[c] * a.CW[((size_t)m * a.C + c) * n + slc];
                    v4 x0 = zero, x1 = zero;
                    if (t0 < 0) x0 = ld4(a.LN + m * a.vstride + (((size_t)nint[b0] * a.C + c) * n + slc) * 4);
                    if (deg == 2 && t1 < 0) x1 = ld4(a.LN + m * a.vstride + (((size_t)nint[b1] * a.C + c) * n + slc) * 4);
                    v4 fe0 = g, fe1 = g;
                    if (deg == 2) {
                        fe0 = mul4(g, (t1 >= 0 && !mod1) ? s1 : h4_msg(a, c, tabc, i1, t1, r1, mod1, x1));
                        fe1 = mul4(g, (t0 >= 0 && !mod0) ? s0 : h4_msg(a, c, tabc, i0, t0, r0, mod0, x0));
                    }
                    d0[m] = fma(pc, dot4(fe0, (t0 >= 0 && !mod0) ? y0 : h4_form(a, c, tabc, i0, t0, r0, mod0, x0)), d0[m]);
                    if (t0 < 0) {
                        const v4 fb = mtv4(as_uniform(mod0 ? a.dP : a.P) + ((size_t)c * a.E + i0) * 16, fe0);
                        if (valid) st4(a.FN + m * a.vstride + (((size_t)nint[b0] * a.C + c) * n + slc) * 4, fb);
                    }
                    if (deg == 2) {
                        d1[m] = fma(pc, dot4(fe1, (t1 >= 0 && !mod1) ? y1 : h4_form(a, c, tabc, i1, t1, r1, mod1, x1)), d1[m]);
                        if (t1 < 0) {
                            const v4 fb = mtv4(as_uniform(mod1 ? a.dP : a.P) + ((size_t)c * a.E + i1) * 16, fe1);
                            if (valid) st4(a.FN + m * a.vstride + (((size_t)nint[b1] * a.C + c) * n + slc) * 4, fb);
                        }
                    }
                }
            }
            if (valid) {
#pragma unroll
                for (int m = 0; m < NM; m++) {
                    a.DV[((size_t)m * a.E + i0) * n + sl] = d0[m] * inv[m];
                    if (deg == 2) a.DV[((size_t)m * a.E + i1) * n + sl] = d1[m] * inv[m];
                }
            }
            continue;
        }

        /* three or more children (an unrooted tree's root, a star): one edge at a time, sibling messages recomputed */
        for (int idx = start; idx < stop; idx++) {
            const int b = ix[idx], t = etip[idx];
            const unsigned row = t >= 0 ? 4u * a.codes[(size_t)b * a.Spad + sg] : 0u;
            double ds[NM];
#pragma unroll
            for (int m = 0; m < NM; m++) ds[m] = 0.0;
            for (int c = 0; c < a.C; c++) {
                v4 ob = v4{1.0, 1.0, 1.0, 1.0};
                if (hd) ob = ld4(a.tip + (size_t)c * tabc + (size_t)a.ntips * a.nchar * 4 + rown);
#pragma unroll
                for (int m = 0; m < NM; m++) {
                    v4 fe = mul4(ld4(a.FN + m * a.vstride + ((vnd + c) * n + slc) * 4), ob);
                    if (slot >= 0) {
                        const double sc = a.SC[m * a.scstride + ((size_t)slot * a.C + c) * n + slc];
                        fe.a *= sc; fe.b *= sc; fe.c *= sc; fe.d *= sc;
                    }
                    for (int idx2 = start; idx2 < stop; idx2++) {
                        if (idx2 == idx) continue;
                        const int b2 = ix[idx2], t2 = etip[idx2];
                        v4 x2 = zero;
                        unsigned row2 = 0u;
                        if (t2 >= 0) row2 = 4u * a.codes[(size_t)b2 * a.Spad + sg];
                        else x2 = ld4(a.LN + m * a.vstride + (((size_t)nint[b2] * a.C + c) * n + slc) * 4);
                        fe = mul4(fe, h4_msg(a, c, tabc, idx2, t2, row2, idx2 == a.mod[m], x2));
                    }
                    const bool mod = idx == a.mod[m];
                    const double pc = prior[c] * a.CW[((size_t)m * a.C + c) * n + slc];
                    v4 x = zero;
                    if (t < 0) x = ld4(a.LN + m * a.vstride + (((size_t)nint[b] * a.C + c) * n + slc) * 4);
                    ds[m] = fma(pc, dot4(fe, h4_form(a, c, tabc, idx, t, row, mod, x)), ds[m]);
                    if (t < 0) {
                        const v4 fb = mtv4(as_uniform(mod ? a.dP : a.P) + ((size_t)c * a.E + idx) * 16, fe);
                        if (valid) st4(a.FN + m * a.vstride + (((size_t)nint[b] * a.C + c) * n + slc) * 4, fb);
                    }
                }
            }
            if (valid) {
#pragma unroll
                for (int m = 0; m < NM; m++) a.DV[((size_t)m * a.E + idx) * n + sl] = ds[m] * inv[m];
            }
        }
    }
}

#endif
