/* plk_catpost.h -- rate-category posteriors and posterior mean site rates; included by plk_engine.hip */
#ifndef PLK_CATPOST_H
#define PLK_CATPOST_H

/*
 * post[s][c] = prior_c L_{s,c} / sum_c' prior_c' L_{s,c'},   rate[s] = sum_c post[s][c] * cat_rates[c]
 *
 * The ll kernels form term_c = prior_c * L_{s,c} (a mantissa and the exponent the OP_SCALE ops took out) per category
 * and fold it into one running sum.  The kernels here run the same traversal and keep the C terms instead: after the
 * last category they are brought to the largest exponent, summed and divided.  Outputs leave as [C][S] planes (site
 * index fastest: every store of a wave is one contiguous 512-byte run), the weighted site sums as one double-double
 * partial per workgroup and output row (rows 0 .. C-1: w_s post[s][c]; row C: w_s rate[s]; row C+1: w_s ll_s), which
 * k_dd_slices / k_dd_final finish.  A site of likelihood zero gets NaN posteriors and rate and ll = -inf; it adds
 * nothing to the partial sums and raises *zero_flag when its weight is not zero, so that the host refuses the sums.
 */
#define PLK_CATPOST_REG_C 8      /* categories the k = 4 kernel keeps in registers */

struct CatPostArgs {
    FusedArgs f;               /* the C++ interpreter's formats (plk_fused4.h); f.partial is not used */
    const double *cat_rates;   /* [C] */
    double *post;              /* [C][S] */
    double *rate;              /* [S] or null */
    dd *partial;               /* [C + 2][gridDim.x] or null */
    int *zero_flag;
};

/* common last step of both kernels for one site: weighted contributions of a finished site to the workgroup's sums */
__device__ static inline dd catpost_weighted(const double *w, long s, bool live, double x)
{
    if (!live) return dd_make(0.0, 0.0);
    return w ? dd_two_prod(w[s], x) : dd_make(x, 0.0);
}

#define PLK_CP_LOAD_M(P_)                                                                       \
    do {                                                                                        \
        m0 = (P_)[0]; m1 = (P_)[1]; m2 = (P_)[2]; m3 = (P_)[3]; m4 = (P_)[4]; m5 = (P_)[5]; m6 = (P_)[6]; m7 = (P_)[7]; \
        m8 = (P_)[8]; m9 = (P_)[9]; m10 = (P_)[10]; m11 = (P_)[11]; m12 = (P_)[12]; m13 = (P_)[13]; m14 = (P_)[14]; m15 = (P_)[15]; \
    } while (0)

/* one traversal op, OUT = f(IN): the op set of the C++ interpreter, one site per lane.  This is PLK_FUSED_EXEC of
 * plk_fused4.h at NS = 1 (that header undefines its macros): the two must change together. */
#define PLK_CP_EXEC(OX, OY, OZ, IN, OUT)                                                                  \
    do {                                                                                                  \
        const int code_ = (OX) & 0xff;                                                                    \
        if (code_ == OP_MATVEC) {                                                                         \
            double n0 = m0 * IN[0], n1 = m1 * IN[0], n2 = m2 * IN[0], n3 = m3 * IN[0];                    \
            n0 = fma(m4, IN[1], n0); n1 = fma(m5, IN[1], n1); n2 = fma(m6, IN[1], n2); n3 = fma(m7, IN[1], n3);       \
            n0 = fma(m8, IN[2], n0); n1 = fma(m9, IN[2], n1); n2 = fma(m10, IN[2], n2); n3 = fma(m11, IN[2], n3);     \
            n0 = fma(m12, IN[3], n0); n1 = fma(m13, IN[3], n1); n2 = fma(m14, IN[3], n2); n3 = fma(m15, IN[3], n3);   \
            OUT[0] = n0; OUT[1] = n1; OUT[2] = n2; OUT[3] = n3;                                           \
            mi++;                                                                                         \
            PLK_CP_LOAD_M(PSc + mi * 16);   /* matrices are consumed in stream order */                   \
        } else if (code_ == OP_TIP_MUL || code_ == OP_TIP_SET) {                                          \
            const int t_ = (OX) >> 8;                                                                     \
            const double2 *tp = reinterpret_cast<const double2 *>(tip_lds + t_ * nchar4 + ch_next * 4);   \
            const double2 v01 = tp[0], v23 = tp[1];                                                       \
            ch_next = code_lds[(OZ) * PLK_TILE + tid];                                                    \
            if (code_ == OP_TIP_SET) { OUT[0] = v01.x; OUT[1] = v01.y; OUT[2] = v23.x; OUT[3] = v23.y; }  \
            else { OUT[0] = IN[0] * v01.x; OUT[1] = IN[1] * v01.y; OUT[2] = IN[2] * v23.x; OUT[3] = IN[3] * v23.y; } \
        } else if (code_ == OP_POPMUL) {                                                                  \
            OUT[0] = IN[0]; OUT[1] = IN[1]; OUT[2] = IN[2]; OUT[3] = IN[3];                               \
            stack_popmul<D, 1>((OY), 0, OUT[0], OUT[1], OUT[2], OUT[3]);                                  \
        } else if (code_ == OP_PUSH) {                                                                    \
            stack_push<D, 1>((OY), 0, IN[0], IN[1], IN[2], IN[3]);                                        \
            OUT[0] = IN[0]; OUT[1] = IN[1]; OUT[2] = IN[2]; OUT[3] = IN[3];                               \
        } else if (code_ == OP_SCALE) {                                                                   \
            const double mx = fmax(fmax(IN[0], IN[1]), fmax(IN[2], IN[3]));                               \
            const int e = frexp_exp(mx);                                                                  \
            OUT[0] = ldexp(IN[0], -e); OUT[1] = ldexp(IN[1], -e);                                         \
            OUT[2] = ldexp(IN[2], -e); OUT[3] = ldexp(IN[3], -e);                                         \
            esc += e;                                                                                     \
        } else if (code_ == OP_NODE_MUL) {                                                                \
            const double *dv = a.f.defs + ch_next * 4;                                                    \
            ch_next = code_lds[(OZ) * PLK_TILE + tid];                                                    \
            OUT[0] = IN[0] * dv[0]; OUT[1] = IN[1] * dv[1]; OUT[2] = IN[2] * dv[2]; OUT[3] = IN[3] * dv[3]; \
        } else { /* OP_END / padding: pass through */                                                     \
            OUT[0] = IN[0]; OUT[1] = IN[1]; OUT[2] = IN[2]; OUT[3] = IN[3];                               \
        }                                                                                                 \
    } while (0)

/*
 * k = 4, compact codes, C <= 8: one site per lane, the waiting vectors in the AGPR stack of plk_fused4.h, the tip table
 * of the current category and the tile's code rows in LDS, ops and matrices through scalar loads.  The C terms and
 * their exponents stay in registers until the last category is done.
 */
template <int D>
__global__ __launch_bounds__(PLK_TILE) void k_ll_fused4_catpost(CatPostArgs a)
{
    /* reserve the AGPRs the stack uses (8 per slot) */
    if constexpr (D <= 4) asm volatile("" ::: PLK_CLOBBER_A0_31);
    else if constexpr (D <= 8) asm volatile("" ::: PLK_CLOBBER_A0_31, PLK_CLOBBER_A32_63);
    else asm volatile("" ::: PLK_CLOBBER_A0_31, PLK_CLOBBER_A32_63, PLK_CLOBBER_A64_127);

    extern __shared__ double lds_dyn[];
    double *tip_lds = lds_dyn;
    const int tip_doubles = a.f.ntips * a.f.nchar * 4;
    uint8_t *code_lds = reinterpret_cast<uint8_t *>(lds_dyn + tip_doubles);

    const long tile0 = (long)blockIdx.x * PLK_TILE;
    const int tid = threadIdx.x;
    const long S = a.f.S;
    const int C = a.f.C;

    /* stage codes[obs][PLK_TILE] of this tile: rows are padded to Spad (a multiple of the tile) */
    {
        const int ndw = a.f.nobs * (PLK_TILE / 4);
        uint32_t *dst = reinterpret_cast<uint32_t *>(code_lds);
        for (int idx = tid; idx < ndw; idx += PLK_TILE) {
            int row = idx / (PLK_TILE / 4), col = idx - row * (PLK_TILE / 4);
            const uint32_t *src = reinterpret_cast<const uint32_t *>(a.f.codes + (size_t)a.f.obs_nodes[row] * a.f.Spad + tile0);
            dst[idx] = src[col];
        }
    }

    const PLK_AS4 int *ops = as_uniform(reinterpret_cast<const int *>(a.f.ops));
    const PLK_AS4 double *prior = as_uniform(a.f.cat_prior);
    const PLK_AS4 double *rootw = as_uniform(a.f.root_w);
    const PLK_AS4 double *crate = as_uniform(a.cat_rates);
    const int nchar4 = a.f.nchar * 4;

    double term[PLK_CATPOST_REG_C];
    int texp[PLK_CATPOST_REG_C];
#pragma unroll
    for (int i = 0; i < PLK_CATPOST_REG_C; i++) { term[i] = 0.0; texp[i] = 0; }
    int emax = 0;
    bool have = false;

    for (int c = 0; c < C; c++) {
        __syncthreads();
        {
            const double2 *src = reinterpret_cast<const double2 *>(a.f.tip + (size_t)c * tip_doubles);
            double2 *dst = reinterpret_cast<double2 *>(tip_lds);
            for (int idx = tid; idx < tip_doubles / 2; idx += PLK_TILE) dst[idx] = src[idx];
        }
        __syncthreads();

        double A[4], B[4];
        A[0] = A[1] = A[2] = A[3] = 1.0;
        int esc = 0;
        int ch_next = code_lds[a.f.first_row * PLK_TILE + tid];   /* code for the first observation op */
        const PLK_AS4 double *PSc = as_uniform(a.f.PS) + (size_t)c * (a.f.nmat + 1) * 16;
        int mi = 0;
        double m0, m1, m2, m3, m4, m5, m6, m7, m8, m9, m10, m11, m12, m13, m14, m15;
        PLK_CP_LOAD_M(PSc);
        int ax = ops[0], ay = ops[1], az = ops[2];
        int bx = ops[4], by = ops[5], bz = ops[6];

        /* ops are executed in pairs (program padded to an even count + one spare pair) */
        for (int pc = 0; pc < a.f.nops; pc += 2) {
            const int nax = ops[4 * pc + 8], nay = ops[4 * pc + 9], naz = ops[4 * pc + 10];
            const int nbx = ops[4 * pc + 12], nby = ops[4 * pc + 13], nbz = ops[4 * pc + 14];
            PLK_CP_EXEC(ax, ay, az, A, B);
            PLK_CP_EXEC(bx, by, bz, B, A);
            ax = nax; ay = nay; az = naz; bx = nbx; by = nby; bz = nbz;
        }
        double lh;
        if (a.f.root_mode == PLK_ROOT_NONE) lh = ((A[0] + A[1]) + A[2]) + A[3];
        else if (a.f.root_mode == PLK_ROOT_UNIFORM) lh = (((A[0] + A[1]) + A[2]) + A[3]) * 0.25;
        else lh = fma(rootw[3], A[3], fma(rootw[2], A[2], fma(rootw[1], A[1], rootw[0] * A[0])));
        const double t = prior[c] * lh;
        if (t != 0.0) { emax = have ? max(emax, esc) : esc; have = true; }
        /* c is uniform: a chain of selects, the terms never leave their registers */
#pragma unroll
        for (int i = 0; i < PLK_CATPOST_REG_C; i++)
            if (i == c) { term[i] = t; texp[i] = esc; }
    }

    /* common exponent, one sum, normalise */
    const long s = tile0 + tid;
    const bool valid = s < S;
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < PLK_CATPOST_REG_C; i++) {
        term[i] = term[i] != 0.0 ? ldexp(term[i], max(texp[i] - emax, -4000)) : 0.0;
        sum += term[i];
    }
    const double ll = have ? log(sum) + (double)emax * 0.6931471805599453094 : -INFINITY;
    double rate = 0.0;
#pragma unroll
    for (int i = 0; i < PLK_CATPOST_REG_C; i++) {
        term[i] = have ? term[i] / sum : NAN;
        if (i < C) {
            rate = fma(term[i], crate[i], rate);
            if (valid) a.post[(size_t)i * S + s] = term[i];
        }
    }
    if (valid) {
        if (a.rate) a.rate[s] = rate;
        if (a.f.site_ll) a.f.site_ll[s] = ll;
    }
    if (a.partial) {
        const bool live = valid && have;
        if (valid && !have && (!a.f.w || a.f.w[s] != 0.0)) *a.zero_flag = 1;
#pragma unroll
        for (int i = 0; i < PLK_CATPOST_REG_C; i++)
            if (i < C) {
                const dd r = dd_block_sum(catpost_weighted(a.f.w, s, live, term[i]));
                if (tid == 0) a.partial[(size_t)i * gridDim.x + blockIdx.x] = r;
            }
        const dd rr = dd_block_sum(catpost_weighted(a.f.w, s, live, rate));
        if (tid == 0) a.partial[(size_t)C * gridDim.x + blockIdx.x] = rr;
        const dd rl = dd_block_sum(catpost_weighted(a.f.w, s, live, ll));
        if (tid == 0) a.partial[(size_t)(C + 1) * gridDim.x + blockIdx.x] = rl;
    }
}
#undef PLK_CP_LOAD_M
#undef PLK_CP_EXEC

/*
 * Every other case (any k <= 64, any C <= 64, dense or compact patterns): the structure of k_ll_generic<K>, stack slots
 * in HBM.  The C terms do not fit in registers, so each category's term and exponent go to the output plane as they are
 * formed; a second loop of the same lane over what it wrote brings them to the common exponent and sums, a third divides.
 */
struct CatPostGenArgs {
    GenArgs g;                 /* g.partial is not used */
    const double *cat_rates;
    double *post;              /* [C][S] */
    int *expo;                 /* [C][S] workspace */
    double *rate;
    dd *partial;               /* [C + 2][gridDim.x] or null */
    int *zero_flag;
};

template <int K>
__global__ __launch_bounds__(GEN_BLOCK) void k_catpost_generic(CatPostGenArgs ca)
{
    const GenArgs &a = ca.g;
    __shared__ double xs[K][GEN_BLOCK];
    const int tid = threadIdx.x;
    const long s = (long)blockIdx.x * GEN_BLOCK + tid;
    const bool valid = s < a.S;
    const long sc = valid ? s : a.S - 1;

    int emax = 0;
    bool have = false;

    for (int c = 0; c < a.C; c++) {
        double cur[K];
#pragma unroll
        for (int i = 0; i < K; i++) cur[i] = 1.0;
        int esc = 0;
        const double *PSc = a.PS + (size_t)c * a.nops * K * K;
        for (int pc = 0; pc < a.nops; pc++) {
            int2 op;
            op.x = as_uniform(reinterpret_cast<const int *>(a.ops))[2 * pc];
            op.y = as_uniform(reinterpret_cast<const int *>(a.ops))[2 * pc + 1];
            const int code = op.x & 0xff;
            if (code == OP_MATVEC || code == OP_TIP_SET || code == OP_TIP_MUL) {
                if (code == OP_MATVEC) {
#pragma unroll
                    for (int j = 0; j < K; j++) xs[j][tid] = cur[j];
                } else {
                    gen_load_obs<K>(a, op.y, sc, tid, xs);
                }
                const double *M = PSc + (size_t)pc * K * K;
                double acc[K];
#pragma unroll
                for (int i = 0; i < K; i++) acc[i] = 0.0;
                for (int j = 0; j < a.k; j++) {
                    const double x = xs[j][tid];
                    const double *col = M + j * K;
#pragma unroll
                    for (int i = 0; i < K; i++) acc[i] = fma(col[i], x, acc[i]);
                }
                if (code == OP_TIP_MUL) {
#pragma unroll
                    for (int i = 0; i < K; i++) cur[i] *= acc[i];
                } else {
#pragma unroll
                    for (int i = 0; i < K; i++) cur[i] = acc[i];
                }
            } else if (code == OP_PUSH) {
                double *sp = a.slots + (size_t)op.y * a.k * a.S + sc;
#pragma unroll
                for (int i = 0; i < K; i++)
                    if (i < a.k && valid) sp[(size_t)i * a.S] = cur[i];
            } else if (code == OP_POPMUL) {
                const double *sp = a.slots + (size_t)op.y * a.k * a.S + sc;
#pragma unroll
                for (int i = 0; i < K; i++)
                    if (i < a.k) cur[i] *= valid ? sp[(size_t)i * a.S] : 1.0;
            } else if (code == OP_NODE_MUL) {
                gen_load_obs<K>(a, op.y, sc, tid, xs);
#pragma unroll
                for (int i = 0; i < K; i++)
                    if (i < a.k) cur[i] *= xs[i][tid];
            } else if (code == OP_SCALE) {
                double m = 0.0;
#pragma unroll
                for (int i = 0; i < K; i++) m = fmax(m, cur[i]);
                const int e = frexp_exp(m);
#pragma unroll
                for (int i = 0; i < K; i++) cur[i] = ldexp(cur[i], -e);
                esc += e;
            }
        }
        double lh = 0.0;
        if (a.root_mode == PLK_ROOT_NONE || a.root_mode == PLK_ROOT_UNIFORM) {
#pragma unroll
            for (int i = 0; i < K; i++)
                if (i < a.k) lh += cur[i];
            if (a.root_mode == PLK_ROOT_UNIFORM) lh /= (double)a.k;
        } else {
#pragma unroll
            for (int i = 0; i < K; i++) lh = fma(a.root_w[i], cur[i], lh);
        }
        const double t = a.cat_prior[c] * lh;
        if (t != 0.0) { emax = have ? max(emax, esc) : esc; have = true; }
        if (valid) { ca.post[(size_t)c * a.S + s] = t; ca.expo[(size_t)c * a.S + s] = esc; }
    }

    /* the lane reads back what it wrote itself: common exponent and sum, then the division */
    double sum = 0.0;
    if (valid)
        for (int c = 0; c < a.C; c++) {
            const double t = ca.post[(size_t)c * a.S + s];
            const double x = t != 0.0 ? ldexp(t, max(ca.expo[(size_t)c * a.S + s] - emax, -4000)) : 0.0;
            ca.post[(size_t)c * a.S + s] = x;
            sum += x;
        }
    const double ll = have ? log(sum) + (double)emax * 0.6931471805599453094 : -INFINITY;
    const bool live = valid && have;
    if (ca.partial && valid && !have && (!a.w || a.w[s] != 0.0)) *ca.zero_flag = 1;
    double rate = 0.0;
    for (int c = 0; c < a.C; c++) {
        double p = 0.0;
        if (valid) {
            p = have ? ca.post[(size_t)c * a.S + s] / sum : NAN;
            ca.post[(size_t)c * a.S + s] = p;
            rate = fma(p, ca.cat_rates[c], rate);
        }
        if (ca.partial) {
            const dd r = dd_block_sum(catpost_weighted(a.w, s, live, p));
            if (tid == 0) ca.partial[(size_t)c * gridDim.x + blockIdx.x] = r;
        }
    }
    if (valid) {
        if (ca.rate) ca.rate[s] = rate;
        if (a.site_ll) a.site_ll[s] = ll;
    }
    if (ca.partial) {
        const dd rr = dd_block_sum(catpost_weighted(a.w, s, live, rate));
        if (tid == 0) ca.partial[(size_t)a.C * gridDim.x + blockIdx.x] = rr;
        const dd rl = dd_block_sum(catpost_weighted(a.w, s, live, ll));
        if (tid == 0) ca.partial[(size_t)(a.C + 1) * gridDim.x + blockIdx.x] = rl;
    }
}

#endif
