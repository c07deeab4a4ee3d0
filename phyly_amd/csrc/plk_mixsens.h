/*
 * plk_mixsens.h -- up passes of plk_mixture_sens: the gradient of sum_s w_s ll_s in the priors and the rates of the rate
 * mixture, both taken as independent,
 *     prior_out[c] = sum_s w_s L_{s,c} / lhood_s
 *     rate_out[c]  = sum_e sum_s w_s prior_c fe_{s,c,e}^T D_{c,e} L_{s,c,b} / lhood_s,     D_{c,e} = t_e Qn P_{c,e}
 * with L_{s,c} the site likelihood under category c alone (root prior included), fe the vector above the edge e = (a -> b)
 * and L_b the vector below it (plk_pairsums.h has the same two vectors).  D is dP/dr_c itself, not dP/dt_e rescaled: at
 * r_c = 0 (the invariable category) P = I and D = t_e Qn, which is the true derivative there.  Included by plk_engine.hip.
 * The reference has no such pass.
 *
 * Geometry, reduction and forward vectors are those of plk_pairsums.h: fixed grid, a workgroup walks the site batches
 * b = blockIdx.x, blockIdx.x + gridDim.x, ... of the chunk, the lane that stored F_b for a site reads it back.  A lane
 * carries ONE number per category through the whole up pass, the sum over its sites and over all edges of the edge form,
 * and one more for the prior row; they are reduced over the workgroup once, after the last node (ps_block_reduce), go to
 * the workgroup's column of part[row][workgroup] and are finished by k_wsum_rows / k_dd_final.  No [E][n] plane, no
 * atomics: the order of every sum is fixed by the launch geometry alone.
 */
#ifndef PLK_MIXSENS_H
#define PLK_MIXSENS_H

#define MIX4_MAX_C 4             /* categories the k = 4 kernel keeps in registers */

struct MixSensOut {
    double *part;        /* [rows][gridDim.x]; generic kernel: rows 0 .. C-1 prior, C .. 2C-1 rate; k = 4 kernel: see its end */
    int *flag;           /* set to 1 when a site of likelihood 0 has a non-zero weight */
    const double *wsite; /* [n] weights of the chunk or null */
    const double *D;     /* k = 4 kernel: [C][E][4][4] row-major direction matrices t_e Qn P_{c,e} (the generic kernel reads
                            them transposed and padded from UpArgs.DT) */
};

/* D[c][e] = t_e Qn P[c][e] from the stored double-double P, every entry a double-double sum rounded once: K1's own
 * product (dd_rate_product) with the edge rate in the place of the category rate.  An edge of rate 0 gets exact zeros. */
__global__ __launch_bounds__(1024) void k_mix_dir(int k, int E, const double *__restrict__ Qn, const double *__restrict__ edge_rates,
                                                  const dd *__restrict__ Pdd, double *__restrict__ D, int tiled)
{
    extern __shared__ double smem_raw[];
    const int ce = blockIdx.x, e = ce % E;
    const size_t kk = (size_t)k * k;
    dd_rate_product(k, Qn, Pdd + ce * kk, edge_rates[e], D + ce * kk, tiled ? reinterpret_cast<dd *>(smem_raw) : nullptr);
}

/* fe^T D x; D has zero row sums, so a constant x gives exactly 0 (as the dzero edge forms of k_up4) */
__device__ __forceinline__ double mix4_form(const PLK_AS4 double *Dm, const v4 &fe, const v4 &x)
{
    if (const4(x)) return 0.0;
    const v4 y = mv4(Dm, x);
    return fma(fe.d, y.d, fma(fe.c, y.c, fma(fe.b, y.b, fe.a * y.a)));
}

/*
 * k = 4, compact codes, C <= 4: the traversal of k_up4_pairsums (one visit per internal node, tip tables for the leaf
 * messages, rescaling through SC / CW) with the scalar edge form in place of the outer product.  The category loop is
 * unrolled over MIX4_MAX_C so that the accumulators are named registers for the whole pass.
 */
__global__ __launch_bounds__(PS4_BLOCK) void k_up4_mixsens(Up4Args a, MixSensOut o, int nbatch)
{
    __shared__ double sh[PS4_BLOCK / 64][2 * MIX4_MAX_C];
    const size_t n = (size_t)a.n;
    const size_t G = gridDim.x;
    const PLK_AS4 int *pre = as_uniform(a.preorder), *ip = as_uniform(a.indptr), *ix = as_uniform(a.indices);
    const PLK_AS4 int *has = as_uniform(a.node_has_data), *etip = as_uniform(a.edge_tip);
    const PLK_AS4 int *nint = as_uniform(a.node_int), *nsc = as_uniform(a.node_scale);
    const PLK_AS4 double *Pm = as_uniform(a.P), *Dm = as_uniform(o.D);
    const PLK_AS4 double *prior = as_uniform(a.cat_prior), *rw = as_uniform(a.root_w);
    const size_t tabc = (size_t)(a.ntips + 1) * a.nchar * 4;
    const int root = pre[0];
    const v4 w = v4{rw[0], rw[1], rw[2], rw[3]};
    const v4 zero = v4{0.0, 0.0, 0.0, 0.0};

    /* acc[c]: prior row, acc[MIX4_MAX_C + c]: rate row */
    double acc[2 * MIX4_MAX_C];
#pragma unroll
    for (int q = 0; q < 2 * MIX4_MAX_C; q++) acc[q] = 0.0;

    /* root: forward vector = root prior weights; L_{s,c} / lhood_s = CW_c (w . L_root) / LH (L_root carries every rescaling) */
#pragma unroll
    for (int c = 0; c < MIX4_MAX_C; c++) {
        if (c >= a.C) continue;
        for (int bt = blockIdx.x; bt < nbatch; bt += gridDim.x) {
            const long sl = (long)bt * PS4_BLOCK + threadIdx.x;
            const bool valid = sl < a.n;
            const long slc = valid ? sl : a.n - 1;
            if (valid) st4(a.FN + (((size_t)nint[root] * a.C + c) * n + slc) * 4, w);
            const double lh = a.LH[slc];
            const double ws = o.wsite ? o.wsite[slc] : 1.0;
            if (c == 0 && valid && lh == 0.0 && ws != 0.0) *o.flag = 1;
            const double wf = valid && lh != 0.0 ? ws * a.CW[(size_t)c * n + slc] / lh : 0.0;
            const v4 l = ld4(a.LN + (((size_t)nint[root] * a.C + c) * n + slc) * 4);
            acc[c] = fma(wf, fma(w.d, l.d, fma(w.c, l.c, fma(w.b, l.b, w.a * l.a))), acc[c]);
        }
    }

    for (int u = 0; u < a.N; u++) {
        const int nd = pre[u];
        const int start = ip[nd], stop = ip[nd + 1];
        const int deg = stop - start;
        if (deg == 0) continue;
        const bool hd = has[nd] != 0;
        const int slot = nsc[nd];
        const double *fn_nd = a.FN + ((size_t)nint[nd] * a.C) * n * 4;
        const bool both = deg == 2;
        for (int idx = start; idx < stop; idx += both ? 2 : 1) {
            const int idx1 = both ? idx + 1 : idx;
            const int b0 = ix[idx], b1 = ix[idx1];
            const int t0 = etip[idx], t1 = etip[idx1];
#pragma unroll
            for (int c = 0; c < MIX4_MAX_C; c++) {
                if (c >= a.C) continue;
                const double *tipc = a.tip + (size_t)c * tabc;
                for (int bt = blockIdx.x; bt < nbatch; bt += gridDim.x) {
                    const long sl = (long)bt * PS4_BLOCK + threadIdx.x;
                    const bool valid = sl < a.n;
                    const long slc = valid ? sl : a.n - 1;
                    const long sg = a.s0 + slc;
                    const double lh = a.LH[slc];
                    const double wf = valid && lh != 0.0 ? (o.wsite ? o.wsite[slc] : 1.0) * prior[c] * a.CW[(size_t)c * n + slc] / lh : 0.0;
                    v4 g = ld4(fn_nd + ((size_t)c * n + slc) * 4);
                    if (hd) g = mul4(g, ld4(tipc + ((size_t)a.ntips * a.nchar + a.codes[(size_t)nd * a.Spad + sg]) * 4));
                    if (slot >= 0) {
                        const double sc = a.SC[((size_t)slot * a.C + c) * n + slc];
                        g.a *= sc; g.b *= sc; g.c *= sc; g.d *= sc;
                    }
                    /* child 0: lower vector x0, vector above its edge fe0 = g o (messages of the other children) */
                    const int code0 = t0 >= 0 ? a.codes[(size_t)b0 * a.Spad + sg] : 0;
                    const v4 x0 = t0 >= 0 ? ld4(tipc + ((size_t)a.ntips * a.nchar + code0) * 4)
                                          : ld4(a.LN + (((size_t)nint[b0] * a.C + c) * n + slc) * 4);
                    v4 fe0 = g;
                    double form = 0.0;
                    if (both) {
                        const int code1 = t1 >= 0 ? a.codes[(size_t)b1 * a.Spad + sg] : 0;
                        const v4 x1 = t1 >= 0 ? ld4(tipc + ((size_t)a.ntips * a.nchar + code1) * 4)
                                              : ld4(a.LN + (((size_t)nint[b1] * a.C + c) * n + slc) * 4);
                        fe0 = mul4(g, ud4_child_msg(a, c, idx1, t1, code1, tipc, Pm, x1));
                        const v4 fe1 = mul4(g, ud4_child_msg(a, c, idx, t0, code0, tipc, Pm, x0));
                        form = mix4_form(Dm + ((size_t)c * a.E + idx1) * 16, fe1, x1);
                        if (t1 < 0 && valid) st4(a.FN + (((size_t)nint[b1] * a.C + c) * n + slc) * 4, mtv4(Pm + ((size_t)c * a.E + idx1) * 16, fe1));
                    } else {
                        for (int idx2 = start; idx2 < stop; idx2++) {
                            if (idx2 == idx) continue;
                            const int t2 = etip[idx2], b2 = ix[idx2];
                            v4 x2 = zero;
                            int code2 = 0;
                            if (t2 >= 0) code2 = a.codes[(size_t)b2 * a.Spad + sg];
                            else x2 = ld4(a.LN + (((size_t)nint[b2] * a.C + c) * n + slc) * 4);
                            fe0 = mul4(fe0, ud4_child_msg(a, c, idx2, t2, code2, tipc, Pm, x2));
                        }
                    }
                    form += mix4_form(Dm + ((size_t)c * a.E + idx) * 16, fe0, x0);
                    acc[MIX4_MAX_C + c] = fma(wf, form, acc[MIX4_MAX_C + c]);
                    if (t0 < 0 && valid) st4(a.FN + (((size_t)nint[b0] * a.C + c) * n + slc) * 4, mtv4(Pm + ((size_t)c * a.E + idx) * 16, fe0));
                }
            }
        }
    }

    /* one reduction for all rows: the k = 4 kernel always writes 2 MIX4_MAX_C rows (prior c at row c, rate c at row
     * MIX4_MAX_C + c; rows of categories the model does not have are 0), the launcher picks out the 2 C it wants */
    ps_block_reduce<2 * MIX4_MAX_C, PS4_BLOCK / 64>(acc, sh, o.part + blockIdx.x, G);
}

/*
 * Every other state count, dense observations, more than four categories: the traversal of k_up_pairsums<K> (one site
 * per lane, [entity][category][state][site] planes, stored edge vectors for the sibling messages).  One visit per edge:
 * the vector above the edge is formed once, the edge form fe . (D L_b) is added to the lane's number and F_b is stored
 * for an internal child.  One wave per workgroup (a lane reads only its own column of xs).  Not tuned.
 */
template <int K>
__global__ __launch_bounds__(GEN_BLOCK) void k_up_mixsens(UpArgs a, MixSensOut o, int nbatch)
{
    __shared__ double xs[K][GEN_BLOCK];
    const int tid = threadIdx.x;
    const size_t n = (size_t)a.n;
    const size_t G = gridDim.x;
    const int k = a.k;
    const int root = as_uniform(a.preorder)[0];

    /* category outermost: FN planes are per category, so the pass of one category never reads what another wrote, and the
     * lane needs two numbers only */
    for (int c = 0; c < a.C; c++) {
        double pacc = 0.0, racc = 0.0;
        for (int bt = blockIdx.x; bt < nbatch; bt += gridDim.x) {
            const long sl = (long)bt * GEN_BLOCK + tid;
            const bool valid = sl < a.n;
            const long slc = valid ? sl : a.n - 1;
            double *fr = a.FN + ((size_t)root * a.C + c) * k * n + slc;
            const double *lr = a.LN + ((size_t)root * a.C + c) * k * n + slc;
            const double lh = a.LH[slc];
            const double ws = o.wsite ? o.wsite[slc] : 1.0;
            if (c == 0 && valid && lh == 0.0 && ws != 0.0) *o.flag = 1;
            const double wf = valid && lh != 0.0 ? ws * (a.CW ? a.CW[(size_t)c * n + slc] : 1.0) / lh : 0.0;
            double dot = 0.0;
#pragma unroll
            for (int i = 0; i < K; i++) {
                if (i < k) {
                    const double rwi = as_uniform(a.root_w)[i];
                    if (valid) fr[(size_t)i * n] = rwi;
                    dot = fma(rwi, lr[(size_t)i * n], dot);
                }
            }
            pacc = fma(wf, dot, pacc);
        }

        for (int u = 0; u < a.N; u++) {
            const int nd = as_uniform(a.preorder)[u];
            const int start = as_uniform(a.indptr)[nd], stop = as_uniform(a.indptr)[nd + 1];
            if (start == stop) continue;
            const bool has = as_uniform(a.node_has_data)[nd];
            const int slot = a.node_scale ? as_uniform(a.node_scale)[nd] : -1;
            for (int idx = start; idx < stop; idx++) {
                const int b = as_uniform(a.indices)[idx];
                const bool b_leaf = as_uniform(a.indptr)[b] == as_uniform(a.indptr)[b + 1];
                for (int bt = blockIdx.x; bt < nbatch; bt += gridDim.x) {
                    const long sl = (long)bt * GEN_BLOCK + tid;
                    const bool valid = sl < a.n;
                    const long slc = valid ? sl : a.n - 1;
                    const long sg = a.s0 + slc;
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
                        const int b2 = as_uniform(a.indices)[idx2];
                        if (as_uniform(a.indptr)[b2] == as_uniform(a.indptr)[b2 + 1]) {
                            double m2[K];
                            up_stage_obs<K>(a, b2, sg, tid, xs);
                            up_matvec<K, 1>(a.PT + ((size_t)c * a.E + idx2) * K * K, k, xs, tid, m2);
#pragma unroll
                            for (int i = 0; i < K; i++) fe[i] *= m2[i];
                        } else {
                            const double *ev = a.EV + ((size_t)idx2 * a.C + c) * k * n + slc;
#pragma unroll
                            for (int i = 0; i < K; i++)
                                if (i < k) fe[i] *= ev[(size_t)i * n];
                        }
                    }
                    /* y = D L_b (zero row sums: exact zero for a constant L_b), form = fe . y */
                    if (b_leaf) up_stage_obs<K>(a, b, sg, tid, xs);
                    else {
                        const double *lb = a.LN + ((size_t)b * a.C + c) * k * n + slc;
                        for (int j = 0; j < k; j++) xs[j][tid] = lb[(size_t)j * n];
                    }
                    double y[K];
                    up_matvec<K, 2>(a.DT + ((size_t)c * a.E + idx) * K * K, k, xs, tid, y);
                    double d = 0.0;
#pragma unroll
                    for (int i = 0; i < K; i++) d = fma(fe[i], y[i], d);
                    const double lh = a.LH[slc];
                    const double wf = valid && lh != 0.0 ? (o.wsite ? o.wsite[slc] : 1.0) * as_uniform(a.cat_prior)[c] * (a.CW ? a.CW[(size_t)c * n + slc] : 1.0) / lh : 0.0;
                    racc = fma(wf, d, racc);
                    if (!b_leaf) {
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
        }
        const double rp = wave64_sum_lane63(pacc), rr = wave64_sum_lane63(racc);
        if (tid == 63) {
            o.part[(size_t)c * G + blockIdx.x] = rp;
            o.part[((size_t)a.C + c) * G + blockIdx.x] = rr;
        }
    }
}

#endif
