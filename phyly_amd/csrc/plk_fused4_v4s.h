/*
 * plk_fused4_v4s.h -- k_ll_fused4_v4s: the two-sites-per-lane pair-table interpreter (plk_fused4_v4.h) with the codes
 * STREAMED to registers and the tables of all categories resident in LDS.
 * Included by plk_engine.hip after plk_fused4_v4.h.
 *
 * k_ll_fused4_v4 keeps a tile's staged code rows in LDS (67 B x 1536 sites at BASELINE config 3), which leaves room for one
 * category's tables: every tile and category restages 32 KB of tables between two workgroup barriers, every tile
 * recomputes code(b) * nchar + code(c) of its pair rows, and a CU runs one workgroup whose waves idle at the barriers.
 * Here nothing but the tables is in LDS: they are staged once per launch (C x units x nchar x 32 bytes) and every wave
 * walks its own 128-site units.  The waves of a workgroup still meet once per unit and category, before the
 * scalar-cache warm-up: left to drift, they read the matrix streams and op words of different categories at the same
 * time (4 x 13 KB at config 3 through a 16 KB scalar cache) and the kernel runs 10 % longer (measured, DESIGN.md
 * section 4).  Nothing is staged between those barriers, so they cost the waves' skew only.  The codes come from a stream in
 * global memory that holds, per unit, the bytes of the observation ops in program order, four to a dword, one wave-wide
 * 8-byte load per chunk of four observations (layout: plk_program.h, plk_stream_dword); it is built by
 * k_build_code_stream when the formats are uploaded, not per evaluation -- it depends on the patterns and the tree only.
 * The interpreter (tools/gen_fused4_v4.py, streamed mode -> plk_fused4_v4s_asm.h) extracts the next observation's code
 * from the current dword (v_bfe_u32) and keeps two chunks in flight; per site the arithmetic is k_ll_fused4_v4's, instruction
 * for instruction, so site log likelihoods are bit-identical.  The sum differs in the order of its double-double terms
 * only: a wave keeps one running sum over its units (static assignment: reproducible) and writes one partial.
 *
 * Two things remove dispatches and one stall without touching that arithmetic (both off under PLK_OPT_PAIR_TABLES + 64):
 * the op stream the kernel runs is the FOLDED one (plk_fused_v4s_fold in plk_program.h: an ADVANCE rides in the
 * observation handler after it, a SCALE in the MATVEC + POPMUL before it; replayed against the checked stream before it is
 * uploaded), and the HELD instantiation loads a unit's first three chunks once per unit instead of once per category --
 * the next unit's while this unit's log and store run -- so that no category starts with all twelve waves of the CU waiting
 * on the same three loads behind the barrier.
 *
 * The PAIR instantiation (k_ll_fused4_v4s<768, true, true>) is the same kernel around a third text of the interpreter (PLK_V4P_PROGRAM_HELD, pair products: programs
 * within three stack slots).  The registers of stack slot 3 hold a second prefetched table row, the look-up chain runs two
 * observations ahead, and where a node's two children are both look-ups one PAIR op multiplies the two rows straight into
 * the vector under construction: eight v_mul_f64 per lane where the folded stream runs two dispatches, eight v_mov_b64 and
 * the same eight v_mul_f64.  The op stream is plk_fused_v4p_build's (plk_program.h), replayed against the checked stream
 * before it is uploaded; the operands of every multiply are the ones of the folded stream's, so site log likelihoods are
 * bit-identical.  PLK_OPT_PAIR_TABLES + 512 runs the folded stream on k_ll_fused4_v4s<768, true> instead.
 */
#ifndef PLK_FUSED4_V4S_H
#define PLK_FUSED4_V4S_H

#include "plk_fused4_v4s_asm.h"
#include "plk_fused4_v4p_asm.h"
#include "plk_mix.h"

struct FusedV4SArgs {
    FusedPTArgs pt;             /* words = C op streams of stride dwords, nwords = stride; row_nodes / first_row / ntiles unused */
    const unsigned *stream;     /* [units of 128 sites][chunks][64 lanes][site A dword, site B dword] */
    int chunks;                 /* chunks of a unit, the spare ones included */
    int sync;                   /* workgroup barrier: 1 before every unit, 2 before every category, 0 none */
    int groups, cg;             /* GROUPS instantiation: phases of the launch, categories per phase (category c reads image c % cg) */
    const PlkV4SRecord *rec;    /* [C] what the interpreter statement loads itself: op and matrix stream, first tables, root weights */
    double *part_sum;           /* GROUPS: per site, the mixture sum after the phases so far (padded to whole units) ... */
    int *part_exp;              /* ... and its exponent; PLK_V4S_NO_TERM (plk_mix.h): no term yet */
};

/* The kernel's arguments, read where they are used.  The interpreter statement clobbers s20 .. s99, so about twenty scalar
 * registers hold what the loops around it keep: the counters do, values loaded once from the arguments on top of them do not,
 * and the compiler then parks them in lanes of a vector register and moves them in and out around every statement.  The
 * pointer goes through an empty statement, so the loads are not moved out of the loops. */
__device__ __forceinline__ const PLK_AS4 FusedV4SArgs *fused_v4s_args()
{
    auto p = __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return (const PLK_AS4 FusedV4SArgs *)p;
}

/* stream[unit][chunk][lane][half]: one thread per dword; sites past S carry code 0 (the code rows are zero padded), which a
 * four-leaf row's rank tables (luts, PlkFusedPT::lut; may be null without such rows) map to rank 0 whether it occurs or not */
__global__ __launch_bounds__(256) void k_build_code_stream(const uint8_t *__restrict__ codes, long Spad, long nunits,
                                                           const int *__restrict__ obs_row, int nobs, const int *__restrict__ row_nodes /* [5][nrows] */,
                                                           int nrows, int nchar, int chunks, const uint8_t *__restrict__ luts, unsigned *__restrict__ out)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)nunits * chunks * PLK_V4S_UNIT;
    if (idx >= total) return;
    const int half = (int)(idx & 1), lane = (int)((idx >> 1) & 63);
    const size_t uc = idx >> 7, unit = uc / (size_t)chunks;
    const int chunk = (int)(uc - unit * (size_t)chunks);
    const size_t site = unit * PLK_V4S_UNIT + (size_t)half * 64 + lane;
    out[plk_stream_dword(unit, chunk, lane, half, chunks)] =
        site < (size_t)Spad ? plk_stream_site_dword(codes, (size_t)Spad, site, obs_row, nobs, row_nodes, nrows, nchar, chunk, 5, luts) : 0u;
}

/* The interpreter statement for one unit and category.  rec: the category's record, from which the text itself loads the op
 * stream, the matrix stream, the first tables and the root weights into registers it clobbers anyway; the scalar operands are
 * rec and strm only.
 * HELD: the unit's first three chunks (c0 the current dword pair, c1 and c2 the two "in flight") are operands, loaded by
 * the kernel once per unit; otherwise the statement requests them itself, in every category */
template <bool HELD, bool PAIR>
__device__ __forceinline__ void fused_run_program_v4s(double &lha, double &lhb, int &ea, int &eb, const void *rec, const void *strm, unsigned voff,
                                                       unsigned long long c0, unsigned long long c1, unsigned long long c2)
{
    int al, ah, bl, bh;
#ifdef PLK_EXP_EMPTY
    al = bl = 0; ah = bh = 0x3ff00000; ea = eb = 0;
#else
    static_assert(HELD || !PAIR, "the pair-product text has the held prologue only");
    if constexpr (PAIR)
        asm volatile(PLK_V4P_PROGRAM_HELD
                     : [al] "=v"(al), [ah] "=v"(ah), [bl] "=v"(bl), [bh] "=v"(bh), [ea] "=v"(ea), [eb] "=v"(eb)
                     : [voff] "v"(voff), [rec] "s"(rec), [strm] "s"(strm), [c0] "v"(c0), [c1] "v"(c1), [c2] "v"(c2)
                     : PLK_V4S_CLOBBERS);
    else if constexpr (HELD)
        asm volatile(PLK_V4S_PROGRAM_HELD
                     : [al] "=v"(al), [ah] "=v"(ah), [bl] "=v"(bl), [bh] "=v"(bh), [ea] "=v"(ea), [eb] "=v"(eb)
                     : [voff] "v"(voff), [rec] "s"(rec), [strm] "s"(strm), [c0] "v"(c0), [c1] "v"(c1), [c2] "v"(c2)
                     : PLK_V4S_CLOBBERS);
    else
        asm volatile(PLK_V4S_PROGRAM
                     : [al] "=v"(al), [ah] "=v"(ah), [bl] "=v"(bl), [bh] "=v"(bh), [ea] "=v"(ea), [eb] "=v"(eb)
                     : [voff] "v"(voff), [rec] "s"(rec), [strm] "s"(strm)
                     : PLK_V4S_CLOBBERS);
#endif
    lha = __hiloint2double(ah, al);
    lhb = __hiloint2double(bh, bl);
}

/* GROUPS: the categories run in va.groups phases of va.cg categories (the three-leaf form, plk_v4t_plan: fewer resident images
 * leave room for more tables).  A phase stages its group's tables -- behind a barrier that ends the look-ups of the phase
 * before -- and every wave walks the same units as in every other phase, for the group's categories only; between the phases
 * a site's partial mixture sum and exponent wait in va.part_sum / va.part_exp, written and read by the same lane.  The terms
 * of a site are added in category order as without groups, so its log likelihood has the same bits.
 *
 * The frame around the statement is kept lean, because it runs once per unit and category beside ~2000 vector instructions:
 * units, passes and strides are counted in 32 bits (the upload refuses streams beyond that), what else the loops need is read
 * again from the arguments (fused_v4s_args), a site's state between the categories is its sum and its exponent alone
 * (plk_mix_term), and in phases after the first the partial sums are requested a unit ahead, with the unit's first chunks, and
 * not touched before the first statement has run. */
template <int THREADS, bool HELD = false, bool PAIR = false, bool GROUPS = false>
__global__ __launch_bounds__(THREADS) void k_ll_fused4_v4s(FusedV4SArgs va)
{
    constexpr unsigned NW = THREADS / 64;
    extern __shared__ double lds_dyn[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane(tid >> 6);
    dd acc = dd_make(0.0, 0.0);
    /* every wave makes the same number of passes (va.sync: the waves of the workgroup meet before every unit / category, so
     * that they read the same category's matrices and op words through the scalar cache at the same time) */
    const unsigned nunits = (unsigned)((va.pt.f.S + PLK_V4S_UNIT - 1) / PLK_V4S_UNIT);
    const unsigned stride = gridDim.x * NW, first = blockIdx.x * NW + wave, passes = (nunits + stride - 1) / stride;
    const int ngroups = GROUPS ? va.groups : 1;
    for (int g = 0; g < ngroups; g++) {
        int c_hi;
        /* the tables of the resident categories (all of them, once per launch, without GROUPS); the only barrier of the kernel
         * that something is staged behind */
        if (GROUPS && g > 0) __syncthreads();
        {
            const PLK_AS4 FusedV4SArgs *k = fused_v4s_args();
            const int C = k->pt.f.C, c_lo = GROUPS ? g * k->cg : 0;
            c_hi = GROUPS ? min(C, c_lo + k->cg) : C;
            const int tip_doubles = k->pt.f.ntips * k->pt.f.nchar * 4;
            const double2 *src = reinterpret_cast<const double2 *>(k->pt.f.tip) + (size_t)c_lo * (tip_doubles / 2);
            double2 *dst = reinterpret_cast<double2 *>(lds_dyn);
            const int n2 = (c_hi - c_lo) * (tip_doubles / 2);
            /* GROUPS: the thread's index formed again in every phase from the wave's number and the lane count (kept across
             * the interpreter, it and the addresses made from it are spilled to scratch) */
            int i_first = tid;
            if (GROUPS) {
                int l;
                asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
                i_first = (int)wave * 64 + l;
            }
            for (int i0 = i_first; i0 < n2; i0 += 4 * THREADS) {
                double2 v[4];
#pragma unroll
                for (int u = 0; u < 4; u++) v[u] = i0 + u * THREADS < n2 ? src[i0 + u * THREADS] : double2{0.0, 0.0};
#pragma unroll
                for (int u = 0; u < 4; u++) if (i0 + u * THREADS < n2) dst[i0 + u * THREADS] = v[u];
            }
        }
        __syncthreads();
        /* HELD: chunks 0 .. 2 of a unit are the same bytes in every category.  They are requested once per unit -- the next
         * unit's before this unit's epilogue, the first unit's here -- and every category's prologue copies them.  A wave whose
         * next unit does not exist requests nothing: no load goes past the stream (a unit has at least three chunks). */
        unsigned long long c0 = 0, c1 = 0, c2 = 0;
        auto request = [&](unsigned unit) {
            asm volatile("" : "+s"(unit));      /* its 64-bit products are formed here, not kept from one unit to the next */
            const PLK_AS4 FusedV4SArgs *k = fused_v4s_args();
            /* uniform base + the lane's 32-bit offset, formed here: a per-lane 64-bit address kept across the interpreter costs
             * the two registers that decide between 168 VGPRs and a spill */
            unsigned off = (unsigned)lane * 8u;
            asm volatile("" : "+v"(off));
            const char *p = reinterpret_cast<const char *>(k->stream) + (size_t)unit * ((size_t)(unsigned)k->chunks * (PLK_V4S_UNIT * sizeof(unsigned))) + off;
            c0 = *reinterpret_cast<const unsigned long long *>(p);
            c1 = *reinterpret_cast<const unsigned long long *>(p + PLK_V4S_CHUNK_BYTES);
            c2 = *reinterpret_cast<const unsigned long long *>(p + 2 * PLK_V4S_CHUNK_BYTES);
        };
        /* nsum, nexp: the state a unit's first category starts from -- a site's sum of the terms so far and its exponent
         * (PLK_V4S_NO_TERM: none yet).  In phases after the first it comes from part_sum / part_exp and is requested a unit ahead,
         * right in front of the request for the unit's chunks: both travel while the current unit is stored or its log runs, and
         * the one wait in front of the unit's first statement (for the chunks, which the statement reads) covers them, where they
         * are older in the memory queue.  In registers of their own, so that neither the store of the current state nor its log
         * stands between the requests and their issue.  part_sum / part_exp are padded to whole units and a unit that does not
         * exist is not loaded: no load goes past them. */
        double nsum[2];
        int nexp[2];
        auto start = [&](unsigned unit, bool exists) {
            if (GROUPS && g > 0 && exists) {
                asm volatile("" : "+s"(unit));
                const PLK_AS4 FusedV4SArgs *k = fused_v4s_args();
                unsigned off = (unsigned)lane * 8u, off4 = (unsigned)lane * 4u;
                asm volatile("" : "+v"(off), "+v"(off4));
                const char *ps = reinterpret_cast<const char *>(k->part_sum) + (size_t)unit * (PLK_V4S_UNIT * sizeof(double)) + off;
                const char *pe = reinterpret_cast<const char *>(k->part_exp) + (size_t)unit * (PLK_V4S_UNIT * sizeof(int)) + off4;
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    nsum[j] = *reinterpret_cast<const double *>(ps + j * 64 * sizeof(double));
                    nexp[j] = *reinterpret_cast<const int *>(pe + j * 64 * sizeof(int));
                }
            } else {
                nsum[0] = nsum[1] = 0.0;
                nexp[0] = nexp[1] = PLK_V4S_NO_TERM;
            }
        };
        start(first, first < nunits);
        if (HELD && first < nunits) request(first);
        for (unsigned pass = 0; pass < passes; pass++) {
            unsigned u = pass * stride + first;
            asm volatile("" : "+s"(u));
            const bool active = u < nunits;
            double sum[2] = {nsum[0], nsum[1]};
            int Eexp[2] = {nexp[0], nexp[1]};
            if (fused_v4s_args()->sync & 1) __syncthreads();
            for (unsigned c = GROUPS ? (unsigned)(g * fused_v4s_args()->cg) : 0u; c < (unsigned)c_hi; c++) {
                const PLK_AS4 FusedV4SArgs *k = fused_v4s_args();
                if (k->sync & 2) __syncthreads();
                if (!active) continue;
                /* the category and the unit as the statement's operands see them: what is made from them (64-bit products and
                 * offsets) is made here, in scalar registers the statement frees again, not carried around the loop */
                unsigned cc = c, uu = u;
                asm volatile("" : "+s"(cc), "+s"(uu));
                if (k->pt.warm) {
                    /* scalar-cache warm-up of the category's matrix stream and op words: the waves of a CU start a unit's category
                     * loosely in step, each touches its share of the lines (no barrier: best effort) */
                    const int nmat = k->pt.f.nmat, nwords = k->pt.nwords;
                    fused_touch_lines(k->pt.f.PS + (size_t)cc * (nmat + 1) * 16, (unsigned)(nmat + 1) * 128u, wave * 64u, NW * 64u);
                    fused_touch_lines(k->pt.words + (size_t)cc * nwords, (unsigned)nwords * 4u, wave * 64u, NW * 64u);
                }
                const unsigned *strm = k->stream + (size_t)uu * ((size_t)(unsigned)k->chunks * PLK_V4S_UNIT);
                double lhs[2];
                int esc[2];
                fused_run_program_v4s<HELD, PAIR>(lhs[0], lhs[1], esc[0], esc[1], k->rec + cc, strm, (unsigned)lane * 8u, c0, c1, c2);
                const double prior = as_uniform(fused_v4s_args()->pt.f.cat_prior)[c];
#pragma unroll
                for (int j = 0; j < 2; j++) plk_mix_term(sum[j], Eexp[j], prior * lhs[j], esc[j]);
            }
            /* the next unit's first chunks, and its state, travel while this unit's log, store and sum run */
            const bool next = active && u + stride < nunits;
            start(u + stride, next);
            if (HELD && next) request(u + stride);
            const PLK_AS4 FusedV4SArgs *k = fused_v4s_args();
            if (GROUPS && g + 1 < ngroups) {
                if (active) {
                    unsigned off = (unsigned)lane * 8u, off4 = (unsigned)lane * 4u;
                    char *ps = reinterpret_cast<char *>(k->part_sum) + (size_t)u * (PLK_V4S_UNIT * sizeof(double)) + off;
                    char *pe = reinterpret_cast<char *>(k->part_exp) + (size_t)u * (PLK_V4S_UNIT * sizeof(int)) + off4;
#pragma unroll
                    for (int j = 0; j < 2; j++) {
                        *reinterpret_cast<double *>(ps + j * 64 * sizeof(double)) = sum[j];
                        *reinterpret_cast<int *>(pe + j * 64 * sizeof(int)) = Eexp[j];
                    }
                }
            } else {
                const long S = k->pt.f.S;
                double *site_ll = k->pt.f.site_ll;
                const double *w = k->pt.f.w;
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const long s = (long)u * PLK_V4S_UNIT + j * 64 + lane;
                    const double ll = Eexp[j] != PLK_V4S_NO_TERM ? log(sum[j]) + (double)Eexp[j] * 0.6931471805599453094 : -INFINITY;
                    if (active && s < S) {
                        if (site_ll) site_ll[s] = ll;
                        acc = dd_add(acc, dd_weighted(w, s, ll));
                    }
                }
            }
        }
    }
    if (va.pt.f.partial) {
        const dd r = dd_wave_sum(acc);
        if (lane == 0) va.pt.f.partial[(size_t)blockIdx.x * NW + wave] = r;
    }
}

#endif

