/*
 * plk_pairsums.h -- up passes of plk_edge_pair_sums: per category c and edge e = (a -> b) the site-summed outer product
 *     W[c][e][i][j] = sum_s w_s prior_c fe_{s,c,e}[i] L_{s,c,b}[j] / lhood_s
 * of the vector above the edge (fe = F_a o B_a o sibling messages, src/evaluate_site_forward.c:69-94) and the vector
 * below it, and the root vector R[c][i] = sum_s w_s prior_c L_{s,c,root}[i] / lhood_s.  Every site-summed edge form of
 * the up pass is a contraction of W: <W[c][e], dP[c][e]> summed over c is the edge derivative, <W[c][e], P[c][e]> the
 * summed category posterior; plk_rate_matrix_sens contracts it with the adjoint Frechet derivative.
 * Included by plk_engine.hip.  The reference has no such pass.
 *
 * Both kernels run on a fixed grid: a workgroup walks the site batches b = blockIdx.x, blockIdx.x + gridDim.x, ... of
 * the chunk for one (node, category) at a time, every lane adds the terms of its own sites (a handful: batches per
 * workgroup) in registers, and the k x k values of an edge are reduced over the workgroup ONCE per (edge, category), not
 * once per 64 sites: DPP sums inside the wave, the waves in wave order by one thread per value.  The workgroup's sums go
 * to its column of part[row][workgroup]; k_wsum_rows / k_dd_final add the columns in double-double.  part has
 * rows x gridDim.x entries whatever S is.  No atomics: the order of every sum is fixed by the launch geometry alone.
 *
 * Forward vectors go through FN as in k_up4 / k_up: the lane that stored F_b for a site is the lane that reads it back
 * (batch -> workgroup and site -> lane are fixed), so the node-outer loop needs no synchronisation between visits.
 */
#ifndef PLK_PAIRSUMS_H
#define PLK_PAIRSUMS_H

#define PS4_BLOCK UD4_BLOCK

struct PairSumOut {
    double *part;        /* [rows][gridDim.x]; rows = C*E*k*k edge rows, then C*k root rows */
    int *flag;           /* set to 1 when a site of likelihood 0 has a non-zero weight */
    const double *wsite; /* [n] weights of the chunk or null */
    int want_root;
};

/* sum of v over the workgroup's lanes, waves in wave order; the result is valid in thread 0 .. nval - 1 as sh[value] */
template <int NV, int NW>
__device__ __forceinline__ void ps_block_reduce(const double (&v)[NV], double (*sh)[NV], double *dst, size_t stride)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double r[NV];
#pragma unroll
    for (int q = 0; q < NV; q++) r[q] = wave64_sum_lane63(v[q]);
    __syncthreads();                     /* the previous round's readers are done */
    if (lane == 63) {
#pragma unroll
        for (int q = 0; q < NV; q++) sh[wave][q] = r[q];
    }
    __syncthreads();
    if ((int)threadIdx.x < NV) {
        double s = sh[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < NW; w++) s += sh[w][threadIdx.x];
        dst[(size_t)threadIdx.x * stride] = s;
    }
}

/* acc[i*4 + j] += f[i] * x[j] */
__device__ __forceinline__ void ps4_outer(double (&acc)[16], const v4 &f, const v4 &x)
{
    acc[0] = fma(f.a, x.a, acc[0]); acc[1] = fma(f.a, x.b, acc[1]); acc[2] = fma(f.a, x.c, acc[2]); acc[3] = fma(f.a, x.d, acc[3]);
    acc[4] = fma(f.b, x.a, acc[4]); acc[5] = fma(f.b, x.b, acc[5]); acc[6] = fma(f.b, x.c, acc[6]); acc[7] = fma(f.b, x.d, acc[7]);
    acc[8] = fma(f.c, x.a, acc[8]); acc[9] = fma(f.c, x.b, acc[9]); acc[10] = fma(f.c, x.c, acc[10]); acc[11] = fma(f.c, x.d, acc[11]);
    acc[12] = fma(f.d, x.a, acc[12]); acc[13] = fma(f.d, x.b, acc[13]); acc[14] = fma(f.d, x.c, acc[14]); acc[15] = fma(f.d, x.d, acc[15]);
}

/*
 * k = 4, compact codes: k_up4's pass (one site per lane, interleaved LN / FN, rescaling through SC / CW, tip tables for
 * the leaf messages) with the outer product in place of the edge form.  The lower vector of a leaf edge is its row of
 * the definition unit (slot ntips) of the tip table.  Every internal node has its own visit here (k_up4 finishes nodes
 * whose children are all leaves inside their parent's visit; their edges are ordinary edges of this pass).  A node with
 * two children handles both in one visit (F_a, L_b0, L_b1 read once); other degrees take one edge at a time with the
 * sibling messages recomputed.
 */
__global__ __launch_bounds__(PS4_BLOCK) void k_up4_pairsums(Up4Args a, PairSumOut o, int nbatch)
{
    __shared__ double sh[PS4_BLOCK / 64][16];
    const size_t n = (size_t)a.n;
    const size_t G = gridDim.x;
    const PLK_AS4 int *pre = as_uniform(a.preorder), *ip = as_uniform(a.indptr), *ix = as_uniform(a.indices);
    const PLK_AS4 int *has = as_uniform(a.node_has_data), *etip = as_uniform(a.edge_tip);
    const PLK_AS4 int *nint = as_uniform(a.node_int), *nsc = as_uniform(a.node_scale);
    const PLK_AS4 double *Pm = as_uniform(a.P);
    const PLK_AS4 double *prior = as_uniform(a.cat_prior), *rw = as_uniform(a.root_w);
    const size_t tabc = (size_t)(a.ntips + 1) * a.nchar * 4;
    const int root = pre[0];
    const v4 w = v4{rw[0], rw[1], rw[2], rw[3]};
    const v4 zero = v4{0.0, 0.0, 0.0, 0.0};
    const size_t root_row0 = (size_t)a.C * a.E * 16;

    /* root: forward vector = root prior weights; R[c] = sum_s w_s prior_c L_root / lhood (L_root carries every rescaling) */
    for (int c = 0; c < a.C; c++) {
        double racc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int bt = blockIdx.x; bt < nbatch; bt += gridDim.x) {
            const long sl = (long)bt * PS4_BLOCK + threadIdx.x;
            const bool valid = sl < a.n;
            const long slc = valid ? sl : a.n - 1;
            if (valid) st4(a.FN + (((size_t)nint[root] * a.C + c) * n + slc) * 4, w);
            const double lh = a.LH[slc];
            const double ws = o.wsite ? o.wsite[slc] : 1.0;
            if (c == 0 && valid && lh == 0.0 && ws != 0.0) *o.flag = 1;
            if (o.want_root) {
                const double wf = valid && lh != 0.0 ? ws * prior[c] * a.CW[(size_t)c * n + slc] / lh : 0.0;
                const v4 l = ld4(a.LN + (((size_t)nint[root] * a.C + c) * n + slc) * 4);
                racc[0] = fma(wf, l.a, racc[0]); racc[1] = fma(wf, l.b, racc[1]);
                racc[2] = fma(wf, l.c, racc[2]); racc[3] = fma(wf, l.d, racc[3]);
            }
        }
        if (o.want_root)
            ps_block_reduce<4, PS4_BLOCK / 64>(racc, reinterpret_cast<double (*)[4]>(&sh[0][0]), o.part + (root_row0 + (size_t)c * 4) * G + blockIdx.x, G);
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
            const bool want0 = !a.edge_mask || as_uniform(a.edge_mask)[idx];
            const bool want1 = both && (!a.edge_mask || as_uniform(a.edge_mask)[idx1]);
            if (!want0 && !want1 && t0 >= 0 && (!both || t1 >= 0)) continue;      /* nothing below needs a forward vector */
            for (int c = 0; c < a.C; c++) {
                const double *tipc = a.tip + (size_t)c * tabc;
                double acc0[16], acc1[16];
#pragma unroll
                for (int q = 0; q < 16; q++) acc0[q] = acc1[q] = 0.0;
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
                    v4 x0 = t0 >= 0 ? ld4(tipc + ((size_t)a.ntips * a.nchar + code0) * 4)
                                    : ld4(a.LN + (((size_t)nint[b0] * a.C + c) * n + slc) * 4);
                    v4 fe0 = g;
                    if (both) {
                        const int code1 = t1 >= 0 ? a.codes[(size_t)b1 * a.Spad + sg] : 0;
                        const v4 x1 = t1 >= 0 ? ld4(tipc + ((size_t)a.ntips * a.nchar + code1) * 4)
                                              : ld4(a.LN + (((size_t)nint[b1] * a.C + c) * n + slc) * 4);
                        fe0 = mul4(g, ud4_child_msg(a, c, idx1, t1, code1, tipc, Pm, x1));
                        const v4 fe1 = mul4(g, ud4_child_msg(a, c, idx, t0, code0, tipc, Pm, x0));
                        if (want1) ps4_outer(acc1, v4{fe1.a * wf, fe1.b * wf, fe1.c * wf, fe1.d * wf}, x1);
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
                    if (want0) ps4_outer(acc0, v4{fe0.a * wf, fe0.b * wf, fe0.c * wf, fe0.d * wf}, x0);
                    if (t0 < 0 && valid) st4(a.FN + (((size_t)nint[b0] * a.C + c) * n + slc) * 4, mtv4(Pm + ((size_t)c * a.E + idx) * 16, fe0));
                }
                if (want0) ps_block_reduce<16, PS4_BLOCK / 64>(acc0, sh, o.part + ((size_t)c * a.E + idx) * 16 * G + blockIdx.x, G);
                if (want1) ps_block_reduce<16, PS4_BLOCK / 64>(acc1, sh, o.part + ((size_t)c * a.E + idx1) * 16 * G + blockIdx.x, G);
            }
        }
    }
}

/*
 * Every other state count, dense observations, more than four categories: k_up<K>'s pass (one site per lane, vectors in
 * [entity][category][state][site] planes, stored edge vectors for the sibling messages).  The k x k sums of an edge are
 * formed one row i at a time: K accumulators per lane, the vector above the edge recomputed per row from the stored
 * planes (correctness first: this kernel is not tuned).  One wave per workgroup.
 */
template <int K>
__global__ __launch_bounds__(GEN_BLOCK) void k_up_pairsums(UpArgs a, PairSumOut o, int nbatch)
{
    __shared__ double xs[K][GEN_BLOCK];
    const int tid = threadIdx.x;
    const size_t n = (size_t)a.n;
    const size_t G = gridDim.x;
    const int k = a.k;
    const int root = as_uniform(a.preorder)[0];
    const size_t root_row0 = (size_t)a.C * a.E * k * k;

    for (int c = 0; c < a.C; c++) {
        double racc[K];
#pragma unroll
        for (int i = 0; i < K; i++) racc[i] = 0.0;
        for (int bt = blockIdx.x; bt < nbatch; bt += gridDim.x) {
            const long sl = (long)bt * GEN_BLOCK + tid;
            const bool valid = sl < a.n;
            const long slc = valid ? sl : a.n - 1;
            double *fr = a.FN + ((size_t)root * a.C + c) * k * n + slc;
            const double *lr = a.LN + ((size_t)root * a.C + c) * k * n + slc;
            const double lh = a.LH[slc];
            const double ws = o.wsite ? o.wsite[slc] : 1.0;
            if (c == 0 && valid && lh == 0.0 && ws != 0.0) *o.flag = 1;
            const double wf = valid && lh != 0.0 ? ws * as_uniform(a.cat_prior)[c] * (a.CW ? a.CW[(size_t)c * n + slc] : 1.0) / lh : 0.0;
#pragma unroll
            for (int i = 0; i < K; i++) {
                if (i < k) {
                    if (valid) fr[(size_t)i * n] = as_uniform(a.root_w)[i];
                    if (o.want_root) racc[i] = fma(wf, lr[(size_t)i * n], racc[i]);
                }
            }
        }
        if (o.want_root) {
#pragma unroll
            for (int i = 0; i < K; i++) {
                const double r = wave64_sum_lane63(racc[i]);
                if (tid == 63 && i < k) o.part[(root_row0 + (size_t)c * k + i) * G + blockIdx.x] = r;
            }
        }
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
            const bool want = !a.edge_mask || as_uniform(a.edge_mask)[idx];
            if (!want && b_leaf) continue;
            for (int c = 0; c < a.C; c++) {
                /* pass 0 stores F_b; passes 1 .. k (wanted edges) accumulate row i = pass - 1 of the outer product */
                for (int pass = b_leaf ? 1 : 0; pass <= (want ? k : 0); pass++) {
                    double acc[K];
#pragma unroll
                    for (int j = 0; j < K; j++) acc[j] = 0.0;
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
                        if (pass == 0) {
                            /* F_b[j] = sum_i P[i][j] fe[i] */
#pragma unroll
                            for (int i = 0; i < K; i++) xs[i][tid] = fe[i];
                            double fb[K];
                            up_matvec<K, 0>(a.PN + ((size_t)c * a.E + idx) * K * K, k, xs, tid, fb);
                            double *fo = a.FN + ((size_t)b * a.C + c) * k * n + slc;
#pragma unroll
                            for (int i = 0; i < K; i++)
                                if (i < k && valid) fo[(size_t)i * n] = fb[i];
                            continue;
                        }
                        const double lh = a.LH[slc];
                        const double wf = valid && lh != 0.0 ? (o.wsite ? o.wsite[slc] : 1.0) * as_uniform(a.cat_prior)[c] * (a.CW ? a.CW[(size_t)c * n + slc] : 1.0) / lh : 0.0;
                        double fi = 0.0;
#pragma unroll
                        for (int i = 0; i < K; i++) fi = i == pass - 1 ? fe[i] : fi;
                        fi *= wf;
                        if (b_leaf) {
                            double lb[K];
                            up_load_obs_reg<K>(a, b, sg, lb);
#pragma unroll
                            for (int j = 0; j < K; j++) acc[j] = fma(fi, lb[j], acc[j]);
                        } else {
                            const double *lb = a.LN + ((size_t)b * a.C + c) * k * n + slc;
#pragma unroll
                            for (int j = 0; j < K; j++)
                                if (j < k) acc[j] = fma(fi, lb[(size_t)j * n], acc[j]);
                        }
                    }
                    if (pass == 0) continue;
#pragma unroll
                    for (int j = 0; j < K; j++) {
                        const double r = wave64_sum_lane63(acc[j]);
                        if (tid == 63 && j < k) o.part[((((size_t)c * a.E + idx) * k + (pass - 1)) * k + j) * G + blockIdx.x] = r;
                    }
                }
            }
        }
    }
}

#endif
