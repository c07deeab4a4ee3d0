/*
 * plk_engine.hip -- MI355X (gfx950) pruning-likelihood engine behind include/plk.h.
 *
 * Kernels (all fp64; see DESIGN.md for layouts and rooflines).  In this file:
 *   k_expm_dd<F>     P[c][e] = exp(Qn * r_c * t_e) in double-double arithmetic, one workgroup per (c, e);
 *                    replaces arb_mat_exp in src/cross_site_ws.c:151-168.  F = true: the 2k x 2k block
 *                    exponential whose top-right block is the Frechet matrix (src/util.c:501-548).
 *   k_build_*        P gathered into traversal-program order, tip tables P_e * defs[code]
 *   k_ll_generic<K>  post-order traversal program for any k <= 64, stack slots in HBM
 *   k_down_store<K>, k_up<K>   down pass with stored vectors + BFS up pass (deriv, marginal, edge
 *                    expectations, Hessian rows) for dense observations and small k
 *   k_wsum_rows, k_dd_final, k_gram   deterministic double-double reductions over sites
 *                    (src/ndaccum.c:198-254 for aggregated site axes)
 * and in the included headers:
 *   plk_fused4_asm.h   k_ll_fused4_asm: the k = 4 headline kernel, interpreter in CDNA4 assembly
 *                      (src/arbplfll.c:139-170 x src/evaluate_site_lhood.c:21-57 x src/util.c:242-301)
 *   plk_fused4.h       the same program interpreted by a C++ loop (deeper stacks, two sites per lane option)
 *   plk_updown4.h      k_down_fused4 / k_down_store4 / k_up4: k = 4 deriv, marginal, expectations
 *                      (src/evaluate_site_forward.c:32-105, src/arbplfderiv.c:112-371,
 *                      src/arbplfmarginal.c:111-264, src/evaluate_site_frechet.c:5-42)
 *   plk_vec.h          k_ll_vec: 9 <= k <= 32 on the vector pipe
 *   plk_mfma.h, plk_mfma_updown.h   fp64 matrix-core kernels for k up to 64
 * Host side of the engine: model / pattern set-up, program builder (Sethi-Ullman ordered post-order),
 * plk_ll / plk_deriv / plk_marginal / plk_edge_expect(_multi) / plk_fit_edge_rates / plk_hess.
 *
 * There is no CPU path in this file: every entry point needs a HIP device.
 */
#include <hip/hip_runtime.h>
#include <algorithm>
#include <utility>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <mutex>
#include <set>
#include <string>
#include <type_traits>
#include <vector>

#include "plk.h"
#include "plk_dd.h"
#define PLK_K1_FN __host__ __device__ static inline      /* k_expm_dd calls plk_k1_squarings: the header itself has no HIP in it */
#include "plk_k1_check.h"     /* what K1 accepts (host) and its squaring count (host and, by the line above, device) */
#include "plk_program.h"     /* traversal program: opcodes, builder, device formats and their checkers (host only) */

#define PLK_MAX_K 64
#define PLK_MAX_C 64

/* Which ll kernel runs for the engine's state, and how it is launched: the only record of the choice.  upload_formats
 * writes it together with the device formats it names; ll_impl, build_tables, run_expm and plk_get_info read it.  What the
 * streamed k = 4 form runs is one value, k4s (plk_k4_stream, plk_program.h): the engine uploads what it names and launches from it. */
enum LlFamily { LL_FUSED4 = 1, LL_GENERIC = 2, LL_MFMA = 3, LL_VEC = 4 };      /* the values of PLK_INFO_LL_KERNEL */
struct LlPlan {
    LlFamily family = LL_GENERIC;
    PlkK4Choice k4;                      /* LL_FUSED4: variant, sites per tile, NS, D, pack4, table base (plk_k4_choose) */
    PlkK4Stream k4s;                     /* PLK_K4_V4S: the op streams that run (their pair-table format is the engine's fpt), which words are uploaded, held
                                            chunks, tables and groups, LDS, barrier, PLK_INFO_LL_FOLD / _PAIRMUL / _TRIPLE / _QUAD */
    bool pair_tables = false;            /* LL_FUSED4, LL_VEC: the formats are the pair-table ones (fpt) ... */
    int npairs = 0;                      /* ... with so many cherries as tables (PLK_INFO_PAIR_TABLES) */
    int block = 0, wg_sites = 0;         /* lanes per workgroup; sites per workgroup (k = 4: per tile) */
    size_t lds = 0;                      /* dynamic LDS of the launch */
    int mfma_T = 0;                      /* LL_MFMA: 16-row tiles of a matrix; two 16-site groups per wave */
    bool mfma_ns2 = false;
    bool vec_rs = false;                 /* LL_VEC: register stack, and its window of three slots */
    int vec_reg_lo = 0;
    long info_variant = 0, info_form = 0, info_exec_flops = 0;     /* PLK_INFO_LL_VARIANT, _FORM, _LL_EXEC_FLOPS */
};

struct plk_engine {
    int device = 0;
    hipStream_t stream = nullptr, own_stream = nullptr;   /* stream in use; the engine's own one */
    bool info_pending = false;           /* event times of the last ll evaluation not read yet */
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
    /* HIP-event pairs around the traversal kernel of the last PLK_EV_RING ll evaluations (read lazily, so that
     * queued evaluations are not serialised by the measurement) */
    hipEvent_t evk[64][2] = {};
    bool evk_pending[64] = {};
    int evk_next = 0;
    long evk_sum_ns = 0, evk_count = 0;
    std::string err;

    /* tree */
    int N = 0, E = 0;
    std::vector<int> indptr, indices, preorder, b_to_idx, idx_to_a;
    int *d_indptr = nullptr, *d_indices = nullptr, *d_preorder = nullptr;

    /* model */
    int k = 0, C = 0, K = 0, root_mode = 0;
    std::vector<double> Qn, edge_rates, cat_rates, cat_prior, root_w;
    double *d_Qn = nullptr, *d_edge_rates = nullptr, *d_cat_rates = nullptr, *d_cat_prior = nullptr;
    double *d_root_w = nullptr;          /* K, zero padded; the weights of the root dot */
    dd *d_Pdd = nullptr;                 /* [C][E][k*k] unrounded */
    double *d_P = nullptr, *d_dP = nullptr; /* [C][E][k][k] rounded; dP = r_c Qn P */
    bool dp_valid = false;                  /* d_dP holds dP of the current P (K1 skips it for ll evaluations: ensure_dP) */
    dd *d_scratch = nullptr;
    size_t pdd_cap = 0, p_cap = 0, dp_cap = 0, scratch_cap = 0;
    bool model_dirty = true;

    /* patterns */
    long S = 0, Spad = 0;
    int pat_mode = 0;                    /* 0 none, 1 codes, 2 dense */
    uint8_t *d_codes = nullptr;          /* [N][Spad] */
    int nchar = 0;
    std::vector<double> defs;            /* [nchar][k] host */
    std::vector<char> node_observed;     /* N: every site's code at the node is a single observed state (definition = one 1.0) */
    double *d_defs = nullptr;            /* [nchar][K] zero padded */
    double *d_B = nullptr;               /* [N][k][S] */
    std::vector<char> node_has_data;     /* internal nodes whose observations are not all-ones */
    std::vector<int> node_codes;         /* N, codes with nchar <= 16 only (else empty): bit `code` set when some site carries it at the node */
    double *d_w = nullptr;

    /* traversal program (plk_program.h) */
    /* prog_dirty: the program must be rebuilt (tree / patterns / PLK_OPT_FORCE_GENERIC changed); fmt_dirty: the ll plan
     * and the device formats it chose are stale (set by build_program and by every option the plan reads);
     * tables_dirty: the P-dependent tables (matrix stream, tip tables, A fragments) are older than P */
    bool prog_dirty = true, fmt_dirty = true, tables_dirty = true;
    LlPlan plan;                         /* which ll kernel runs, and how: written by upload_formats, valid while !fmt_dirty */
    PlkK4StreamCaps k4_caps;             /* held, pair, groups: k_ll_fused4_v4s<768, true>, <768, true, true>, <768, true, true, true> can be described
                                            and have the static LDS of <768, false> (asked once, with k4_static_lds) */
    size_t k4_static_lds[3] = {};        /* PlkK4Shape::static_lds, asked of the runtime once (k4_static_lds_known) */
    hipError_t k4_static_lds_err[3] = {};
    bool k4_static_lds_known = false;
    PlkProgram pg;
    std::vector<plk_op2> &ops = pg.ops;
    std::vector<int> &op_edge = pg.op_edge;          /* CSR edge per op or -1 */
    std::vector<int> &tip_edge = pg.tip_edge;        /* CSR edge per tip slot */
    std::vector<char> &scale_node = pg.scale_node;   /* N: node vectors rescaled here (every >= 16 accumulated edges) */
    std::vector<int> &obs_nodes = pg.obs_nodes;      /* nodes whose codes the fused kernels stage */
    int &slots_needed = pg.slots_needed;
    PlkFused fu;                         /* fused k = 4 formats of the program */
    PlkFusedPT fpt;                      /* ... and of the pair-table interpreter (k_ll_fused4_asm_pt) */
    unsigned *d_words_pt = nullptr;
    PlkFusedV4 fv4;                      /* 64-bit ops of the two-sites-per-lane interpreter */
    PlkVecPT vpt;                        /* the vector ll kernel's program on pair tables */
    unsigned *d_cstream = nullptr; size_t cstream_cap = 0;   /* the code stream (plk_stream_dword), built by upload_formats */
    int *d_obs_row = nullptr;            /* staged row per observation of the program */
    int *d_row_nodes = nullptr, *d_tabs = nullptr;   /* [5][rows] staged-row nodes (third: the leaf of a three-leaf row; fourth and the index
                                                        of the rank tables: four-leaf rows); [10][ntab] unit, edge, leaf edges of a pair,
                                                        edge above the cherry and leaf edge of a three-leaf table, shape and further edges
                                                        of a four-leaf table; the list ends with fpt.ntriples three-leaf tables and then
                                                        fpt.nquads four-leaf tables */
    uint8_t *d_quad_lut = nullptr;       /* four-leaf rows: PlkFusedPT::lut, [nquads][4][16] code -> rank (the stream builder's) */
    int *d_quad_codes = nullptr;         /* ... and [nquads][4][4] rank -> code (the table builder's; a rank that does not occur: the code of rank 0) */
    double *d_llstate = nullptr; size_t llstate_cap = 0;   /* category groups: per site the partial mixture sum, then the exponents */
    PlkV4SRecord *d_v4s_rec = nullptr;   /* streamed k = 4 kernel: what its interpreter statement loads per category */
    int num_cus = 256;
    int2 *d_ops = nullptr;
    int4 *d_fops = nullptr;              /* fused-kernel program (C++ interpreter) */
    unsigned *d_words = nullptr;         /* fused-kernel program (assembly interpreter) */
    std::vector<int> &mat_edge = fu.mat_edge;        /* CSR edge per compact matrix of the fused stream */
    int *d_op_edge = nullptr, *d_tip_edge = nullptr, *d_obs_nodes = nullptr, *d_mat_edge = nullptr, *d_edge_slot = nullptr;
    double *d_PS = nullptr;              /* [C][nops][K*K] transposed: PS[j*K+i] = P[i][j] */
    double *d_tip = nullptr;             /* [C][ntips][nchar][4] */
    double *d_frag = nullptr; size_t frag_cap = 0;   /* MFMA A fragments */
    double *d_root_wd = nullptr;         /* root weights, distributed layout */
    int4 *d_mops = nullptr;              /* MFMA program (observation ops chained for the value prefetch) */
    double *d_exL = nullptr, *d_exF = nullptr;   /* edge expectations: directions, scaled Frechet matrices */
    int *d_exmask = nullptr;
    dd *d_exscr = nullptr;
    size_t exL_cap = 0, exF_cap = 0, exmask_cap = 0, exscr_cap = 0;
    int *d_u4pack = nullptr;             /* k = 4 down / up passes: the call's integer tables, one block */
    double *d_u4tip = nullptr;           /* ... and its tip / edge-form tip tables */
    size_t u4pack_cap = 0, u4tip_cap = 0;
    double *d_stage = nullptr; size_t stage_cap = 0;   /* transposed per-site outputs on their way to the host */
    double *d_uvmat = nullptr; size_t uvmat_cap = 0;   /* vector down / up passes: PT and the up-pass matrix stream */
    int mfma_first_mv = -1, mfma_first_slot = -1, mfma_first_row = 0, vec_second_row = 0;
    size_t ps_cap = 0, tip_cap = 0;

    /* rate-category posteriors (plk_catpost.h): the query's own copies of the program formats and of the P-dependent
     * tables, so that what plk_ll has cached (pair-table, assembly or C++ formats, whichever it selected) is never touched.
     * cp_kind: 0 nothing uploaded for the current program, 1 the C++ interpreter's k = 4 formats, 2 the generic ones */
    int cp_kind = 0;
    bool cp_tables_valid = false;        /* the query's matrix stream and tip tables hold the current P (cleared by K1) */
    PlkFused cpf;
    hipEvent_t cp_ev0 = nullptr, cp_ev1 = nullptr;   /* around the device work of the last call (PLK_INFO_LAST_CAT_POSTERIOR_NS) */
    long info_cat_posterior_ns = 0;
    int4 *d_cp_fops = nullptr;
    int2 *d_cp_ops = nullptr;
    int *d_cp_mat_edge = nullptr, *d_cp_tip_edge = nullptr, *d_cp_obs_nodes = nullptr, *d_cp_op_edge = nullptr, *d_cp_expo = nullptr, *d_cp_flag = nullptr;
    double *d_cp_PS = nullptr, *d_cp_tip = nullptr, *d_cp_out = nullptr;
    dd *d_cp_partial = nullptr;
    size_t cp_ps_cap = 0, cp_tip_cap = 0, cp_out_cap = 0, cp_expo_cap = 0, cp_partial_cap = 0;

    /* workspaces */
    double *d_slots = nullptr; size_t slots_cap = 0;
    double *d_site_ll = nullptr; size_t site_ll_cap = 0;
    dd *d_partial = nullptr; size_t partial_cap = 0;
    double *d_work = nullptr; size_t work_cap = 0;   /* deriv / marginal workspace */

    /* options / info */
    long opt_force_generic = 0, opt_site_chunk = 0, opt_fused_ns = 0, opt_fused_asm = 1, opt_mfma = 1, opt_up_nodes = 2, opt_pair_tables = 1, opt_vec_reg_stack = 1, opt_mfma_ns2 = 0, opt_stream_grid = 0;
    void *comm = nullptr;                /* ncclComm_t of the one-process-per-GPU reduction step */
    int comm_ranks = 0;
    long info_pair_sums_kernel = 0, info_query_ns = 0;
    double *d_mixD = nullptr; size_t mixd_cap = 0;   /* plk_mixture_sens: its direction matrices t_e Qn P[c][e] (the query's own; d_dP is not touched) */
    long info_mixture_sens_kernel = 0;
    long info_nni_kernel = 0;                        /* PLK_INFO_NNI_KERNEL: up pass of the last plk_nni_ll */
    /* plk_place_ll: the call's own transition matrices (upper and lower part of every target edge, the pendant edge),
     * their rates, padded streams and pendant tables, and the query observations; the engine's P, dP and tables stay */
    dd *d_plPdd = nullptr; double *d_plP = nullptr, *d_plrates = nullptr, *d_plstream = nullptr, *d_plT = nullptr, *d_pldense = nullptr;
    uint8_t *d_plcodes = nullptr;
    size_t plpdd_cap = 0, plp_cap = 0, plrates_cap = 0, plstream_cap = 0, plt_cap = 0, pldense_cap = 0, plcodes_cap = 0;
    long info_place_kernel = 0;                      /* PLK_INFO_PLACE_KERNEL: up pass of the last plk_place_ll */
    long info_spr_kernel = 0;                        /* PLK_INFO_SPR_KERNEL: up pass of the last plk_spr_ll */
    long info_up4_path = 0;                          /* PLK_INFO_UP4_PATH: which k = 4 up pass the last up/down query took */
    long info_down4_kernel = 0;                      /* PLK_INFO_DOWN4_KERNEL: the k = 4 down pass run_updown4 launched last */
    hipEvent_t q_ev0 = nullptr, q_ev1 = nullptr;     /* around the device work of the last timed query (PLK_INFO_LAST_QUERY_NS) */
    long info_ll_kernel = 0, info_updown_kernel = 0, info_ll_kernel_ns = 0, info_ll_total_ns = 0, info_ll_variant = 0, info_ll_form = 0, info_ll_fold = 0, info_ll_pairmul = 0, info_ll_triple = 0, info_ll_quad = 0, info_ll_barrier = 0, info_ll_exec_flops = 0, info_cat_posterior_kernel = 0;
};

static std::string g_create_error;

/* RCCL is taken from the process at run time (the framework's copy when there is one): no link-time dependency, and a
 * process that never calls plk_comm_* never touches it */
struct PlkNcclId { char internal[128]; };
struct PlkRccl {
    void *lib = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(void **, int, /* ncclUniqueId by value: 128 bytes */ PlkNcclId, int) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    std::string err;
};
static PlkRccl g_rccl;
static std::mutex g_rccl_mu;

static bool rccl_load()
{
    std::lock_guard<std::mutex> lk(g_rccl_mu);
    if (g_rccl.lib) return true;
    const char *names[] = {"librccl.so.1", "librccl.so"};
    void *lib = nullptr;
    for (const char *n : names) if (!lib) lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD);     /* the copy already in the process */
    for (const char *n : names) if (!lib) lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (!lib) { g_rccl.err = std::string("RCCL is not available: ") + (dlerror() ? dlerror() : "librccl.so.1 not found"); return false; }
    g_rccl.GetUniqueId = reinterpret_cast<int (*)(void *)>(dlsym(lib, "ncclGetUniqueId"));
    g_rccl.CommInitRank = reinterpret_cast<int (*)(void **, int, PlkNcclId, int)>(dlsym(lib, "ncclCommInitRank"));
    g_rccl.AllReduce = reinterpret_cast<int (*)(const void *, void *, size_t, int, int, void *, hipStream_t)>(dlsym(lib, "ncclAllReduce"));
    g_rccl.CommDestroy = reinterpret_cast<int (*)(void *)>(dlsym(lib, "ncclCommDestroy"));
    g_rccl.GetErrorString = reinterpret_cast<const char *(*)(int)>(dlsym(lib, "ncclGetErrorString"));
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce || !g_rccl.CommDestroy) { g_rccl.err = "RCCL: entry points missing"; return false; }
    g_rccl.lib = lib;
    return true;
}

static std::string rccl_text(int rc) { return g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : ("code " + std::to_string(rc)); }



/* Live engine handles.  Every entry point refuses a handle that plk_create did not return or that plk_destroy has
 * already taken (PLK_E_ARG instead of a use after free); plk_destroy of such a handle is a no-op.  Once the process
 * is exiting (atexit) handles are only forgotten, not torn down: the HIP runtime's own exit handlers may already
 * have run by the time a late destructor (a garbage-collected binding object, a static of the caller) gets here. */
static std::mutex g_live_mu;
static std::set<const plk_engine *> g_live;
static bool g_exiting = false, g_atexit_set = false;

static bool plk_live(const plk_engine *h)
{
    if (!h) return false;
    std::lock_guard<std::mutex> lk(g_live_mu);
    return !g_exiting && g_live.count(h) != 0;
}

#define HIPCHK(h, call)                                                            \
    do {                                                                           \
        hipError_t e_ = (call);                                                    \
        if (e_ != hipSuccess) {                                                    \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);         \
            return PLK_E_DEVICE;                                                   \
        }                                                                          \
    } while (0)

template <typename T>
static int dev_alloc(plk_engine *h, T **p, size_t n)
{
    if (*p) { (void)hipFree(*p); *p = nullptr; }
    if (n == 0) n = 1;
    hipError_t e = hipMalloc((void **)p, n * sizeof(T));
    if (e != hipSuccess) {
        h->err = std::string("hipMalloc: ") + hipGetErrorString(e);
        *p = nullptr;
        return PLK_E_NOMEM;
    }
    return PLK_OK;
}

template <typename T>
static int dev_upload(plk_engine *h, T **p, const T *src, size_t n)
{
    int rc = dev_alloc(h, p, n);
    if (rc) return rc;
    if (n) HIPCHK(h, hipMemcpy(*p, src, n * sizeof(T), hipMemcpyHostToDevice));
    return PLK_OK;
}

template <typename T>
static int dev_reserve(plk_engine *h, T **p, size_t *cap, size_t n)
{
    if (*p && *cap >= n) return PLK_OK;
    int rc = dev_alloc(h, p, n);
    *cap = rc ? 0 : n;
    return rc;
}

/* ====================================================================== */
/* K1: P = exp(Qn * r_c * t_e) in double-double                            */
/* ====================================================================== */

__device__ static inline dd dd_div_d(dd x, double y)
{
    double q1 = x.hi / y;
    dd p = dd_two_prod(q1, y);
    dd r = dd_add(x, dd_make(-p.hi, -p.lo));
    double q2 = r.hi / y;
    return dd_quick_two_sum(q1, q2);
}

__device__ static void dd_matmul_block(int k, const dd *A, const dd *B, dd *Cm)
{
    int kk = k * k;
    for (int idx = threadIdx.x; idx < kk; idx += blockDim.x) {
        int i = idx / k, j = idx - i * k;
        /* compensated dot product (Ogita, Rump & Oishi's Dot2 on double-double operands): the high words are summed with
         * an exact two-sum, every rounding error and the cross terms go to one low accumulator, one renormalisation at the
         * end -- 12 flops per term instead of the 28 of dd_add(dd_mul); the result carries ~2^-104 relative to
         * sum |a||b|, the same class as before (K1 for k = 61: 0.99 -> see profiles/r03_exp_codon_kernel_variants.json) */
        double sh = 0.0, sl = 0.0;
        for (int l = 0; l < k; l++) {
            const dd a = A[i * k + l], b = B[l * k + j];
            const double p = a.hi * b.hi;
            double e = fma(a.hi, b.hi, -p);
            e = fma(a.hi, b.lo, e);
            e = fma(a.lo, b.hi, e);
            const double t = sh + p, bb = t - sh;
            sl += ((sh - (t - bb)) + (p - bb)) + e;
            sh = t;
        }
        Cm[idx] = dd_quick_two_sum(sh, sl);
    }
}

/* The same product for matrices that live in global scratch (k > 26: codon models, every Frechet block matrix from
 * k = 14 up).  One thread per entry (above) sends two 16-byte loads per term through the CU's vector memory path, which
 * is what bounded K1 at k = 61.  Here a wave owns R rows x 64 columns of the result: it copies its R rows of A into its
 * own LDS strip once, then per term l every lane loads its B[l][j] (coalesced) and reads the R values A[i0 + r][l] from
 * the LDS strip (one address for the whole wave: a broadcast) -- 1 vector-memory load per R terms instead of 2 per term.
 * The sums run over l in the same order with the same Dot2 update, so the result is the one dd_matmul_block gives. */
#define EXPM_TILE_ROWS 4
template <int R>
__device__ static void dd_matmul_tiled(int k, const dd *A, const dd *B, dd *Cm, dd *strips)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    dd *arow = strips + (size_t)wave * EXPM_TILE_ROWS * k;
    const int ngroups = (k + R - 1) / R, nchunks = (k + 63) / 64;
    for (int item = wave; item < ngroups * nchunks; item += nw) {
        const int g = item / nchunks, ch = item - g * nchunks;
        const int i0 = g * R, j = ch * 64 + lane;
        __builtin_amdgcn_wave_barrier();                 /* the strip's previous reads are done (same wave: in order) */
#pragma unroll
        for (int r = 0; r < R; r++)
            for (int t = lane; t < k; t += 64) arow[r * k + t] = i0 + r < k ? A[(size_t)(i0 + r) * k + t] : dd_make(0.0, 0.0);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const bool act = j < k;
        const dd *bcol = B + (act ? j : 0);
        double sh[R], sl[R];
#pragma unroll
        for (int r = 0; r < R; r++) { sh[r] = 0.0; sl[r] = 0.0; }
#pragma unroll 2
        for (int l = 0; l < k; l++) {
            const dd b = bcol[(size_t)l * k];
#pragma unroll
            for (int r = 0; r < R; r++) {
                const dd a = arow[r * k + l];
                const double p = a.hi * b.hi;
                double e = fma(a.hi, b.hi, -p);
                e = fma(a.hi, b.lo, e);
                e = fma(a.lo, b.hi, e);
                const double t = sh[r] + p, bb = t - sh[r];
                sl[r] += ((sh[r] - (t - bb)) + (p - bb)) + e;
                sh[r] = t;
            }
        }
        if (act) {
#pragma unroll
            for (int r = 0; r < R; r++) if (i0 + r < k) Cm[(size_t)(i0 + r) * k + j] = dd_quick_two_sum(sh[r], sl[r]);
        }
    }
}

/* strips == nullptr: the buffers are in LDS (small k), one thread per entry */
__device__ static void dd_matmul(int k, const dd *A, const dd *B, dd *Cm, dd *strips)
{
    if (!strips) { dd_matmul_block(k, A, B, Cm); return; }
    const int nw = blockDim.x >> 6;
    if (((k + 3) / 4) * ((k + 63) / 64) >= nw) dd_matmul_tiled<4>(k, A, B, Cm, strips);
    else dd_matmul_tiled<2>(k, A, B, Cm, strips);
}

/* dP = r_c Qn P, rounded, every entry a double-double sum over l in order (src/util.c:338-345 is what reads it);
 * strips as for dd_matmul: null = one thread per entry, else a wave owns 4 rows x 64 columns and keeps its rows of Qn in LDS */
__device__ static void dd_rate_product(int k, const double *__restrict__ Qn /* [2][k*k] */, const dd *O, double rc, double *dPout, dd *strips)
{
    const int kk = k * k;
    if (!strips) {
        for (int idx = threadIdx.x; idx < kk; idx += blockDim.x) {
            const int i = idx / k, j = idx - i * k;
            dd acc = dd_make(0.0, 0.0);
            for (int l = 0; l < k; l++) acc = dd_add(acc, dd_mul(O[l * k + j], dd_make(Qn[i * k + l], Qn[kk + i * k + l])));
            dPout[idx] = dd_mul_d(acc, rc).hi;
        }
        return;
    }
    constexpr int R = EXPM_TILE_ROWS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    dd *arow = strips + (size_t)wave * R * k;
    const int ngroups = (k + R - 1) / R, nchunks = (k + 63) / 64;
    for (int item = wave; item < ngroups * nchunks; item += nw) {
        const int g = item / nchunks, ch = item - g * nchunks;
        const int i0 = g * R, j = ch * 64 + lane;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < R; r++)
            for (int t = lane; t < k; t += 64)
                arow[r * k + t] = i0 + r < k ? dd_make(Qn[(i0 + r) * k + t], Qn[kk + (i0 + r) * k + t]) : dd_make(0.0, 0.0);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const bool act = j < k;
        const dd *bcol = O + (act ? j : 0);
        dd acc[R];
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = dd_make(0.0, 0.0);
        for (int l = 0; l < k; l++) {
            const dd b = bcol[(size_t)l * k];
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] = dd_add(acc[r], dd_mul(b, arow[r * k + l]));
        }
        if (act) {
#pragma unroll
            for (int r = 0; r < R; r++) if (i0 + r < k) dPout[(size_t)(i0 + r) * k + j] = dd_mul_d(acc[r], rc).hi;
        }
    }
}

/* dynamic LDS of a k_expm_dd launch on kdim x kdim matrices: the six buffers, or one strip of rows per wave */
static inline size_t expm_lds_bytes(size_t kdim, int threads, int *use_lds)
{
    const size_t buffers = 6 * kdim * kdim * sizeof(dd);
    *use_lds = buffers <= 64 * 1024;
    return *use_lds ? buffers : (size_t)(threads / 64) * EXPM_TILE_ROWS * kdim * sizeof(dd);
}

#define EXPM_TERMS 16     /* with |A| <= 2^-5 after scaling: 2^-80 / 16! < 1e-37, below double-double resolution */
/* The degree-16 Taylor polynomial is evaluated by Paterson-Stockmeyer: powers A^2, A^3, A^4 (three products), then
 * Horner in A^4 over the four cubic blocks B_i = c_4i I + c_4i+1 A + c_4i+2 A^2 + c_4i+3 A^3 (three more products) --
 * 6 double-double matrix products instead of 15, before the squarings.  Six k x k buffers per matrix instead of four. */
#define EXPM_BUFFERS 6

/*
 * FRECHET = false: P = exp(s Qn), s = r_c t_e; outputs unrounded / rounded P and dP = r_c Qn P.
 * FRECHET = true: the 2k x 2k block matrix [[s Qn, L], [0, s Qn]] is exponentiated instead and the
 * top-right block -- the Frechet derivative of exp at s Qn in direction L, i.e.
 * int_0^1 exp(s Qn u) L exp(s Qn (1-u)) du (src/util.c:501-548) -- is written to Fout, scaled by
 * coef = 1 (PLK_COEF_PRIOR), s (PLK_COEF_PRIOR_RATE_EDGE) or r_c (PLK_COEF_PRIOR_RATE).
 */
/* k = 4, fused kernels: K1 also writes what the traversal reads, so that an evaluation with new edge rates is K1 + the
 * traversal kernel + the reduction and nothing else: P_e (transposed) into its matrix of the stream for an internal
 * edge, P_e * defs[code] (double-double, constant rows exact) into its tip slot for a leaf edge */
struct ExpmPost {
    const int *edge_slot;      /* [2][E]: matrix index of the edge or -1 | tip slot of the edge or -1; null: no post */
    int nmat1, ntips1, nchar;  /* matrices / tip slots per category (incl. the spare / pseudo one), definitions */
    const double *defs;        /* [nchar][4] */
    double *PS, *tip;
    int skip_dP;               /* an ll evaluation does not read dP: k_dP_dd makes it when a derivative asks (ensure_dP) */
};

template <bool FRECHET>
__global__ __launch_bounds__(1024) void k_expm_dd(int ks, int E, const double *__restrict__ Qn /* [2][ks*ks]: hi then lo */,
                          const double *__restrict__ edge_rates,
                          const double *__restrict__ cat_rates,
                          dd *__restrict__ Pdd, double *__restrict__ P, double *__restrict__ dP,
                          dd *gscratch, int use_lds,
                          const double *__restrict__ Lm /* [2][ks*ks] */, long Lm_stride /* doubles between the directions of consecutive (category, edge) blocks; 0: one direction for all */, int coef_mode,
                          const int *__restrict__ edge_mask, double *__restrict__ Fout, ExpmPost post)
{
    extern __shared__ double smem_raw[];
    __shared__ double s_row[2 * PLK_MAX_K];
    __shared__ int s_sq;
    __shared__ dd s_coef[EXPM_TERMS + 1];           /* 1 / n! in double-double */
    const int ce = blockIdx.x;
    const int c = ce / E, e = ce - c * E;
    const int k = FRECHET ? 2 * ks : ks;
    const int kk = k * k, kks = ks * ks;
    if (FRECHET) Lm += (size_t)ce * Lm_stride;
    if (FRECHET && edge_mask && !edge_mask[e]) {
        for (int idx = threadIdx.x; idx < kks; idx += blockDim.x) Fout[(size_t)ce * kks + idx] = 0.0;
        return;
    }
    dd *base = use_lds ? reinterpret_cast<dd *>(smem_raw) : gscratch + (size_t)ce * EXPM_BUFFERS * kk;
    dd *strips = use_lds ? nullptr : reinterpret_cast<dd *>(smem_raw);       /* global buffers: row strips of the tiled product */
    dd *X = base, *X2 = base + kk, *O = base + 2 * kk, *W = base + 3 * kk, *X3 = base + 4 * kk, *X4 = base + 5 * kk;

    const dd s = dd_two_prod(cat_rates[c], edge_rates[e]);
    for (int idx = threadIdx.x; idx < kk; idx += blockDim.x) {
        if (!FRECHET) {
            X[idx] = dd_mul(s, dd_make(Qn[idx], Qn[kk + idx]));
        } else {
            const int i = idx / k, j = idx - i * k;
            const int bi = i >= ks, bj = j >= ks;
            const int q = (i - bi * ks) * ks + (j - bj * ks);
            dd v = dd_make(0.0, 0.0);
            if (bi == bj) v = dd_mul(s, dd_make(Qn[q], Qn[kks + q]));
            else if (!bi) v = dd_make(Lm[q], Lm[kks + q]);
            X[idx] = v;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < k) {
        double r = 0;
        for (int j = 0; j < k; j++) r += fabs(X[threadIdx.x * k + j].hi);
        s_row[threadIdx.x] = r;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double norm = 0;
        for (int i = 0; i < k; i++) norm = fmax(norm, s_row[i]);
        s_sq = plk_k1_squarings(norm);      /* from the exponent, at most PLK_K1_MAX_SQ: no input decides how long this runs */
        dd cn = dd_make(1.0, 0.0);
        s_coef[0] = cn;
        for (int n = 1; n <= EXPM_TERMS; n++) { cn = dd_div_d(cn, (double)n); s_coef[n] = cn; }
    }
    __syncthreads();
    const int sq = s_sq;
    for (int idx = threadIdx.x; idx < kk; idx += blockDim.x) X[idx] = dd_ldexp(X[idx], -sq);
    __syncthreads();
    dd_matmul(k, X, X, X2, strips);
    __syncthreads();
    dd_matmul(k, X2, X, X3, strips);
    dd_matmul(k, X2, X2, X4, strips);
    __syncthreads();
    /* cubic block i of the polynomial at entry idx */
    auto block = [&](int ib, int idx) -> dd {
        const int i = idx / k, j = idx - i * k;
        dd v = dd_add(dd_mul(s_coef[4 * ib + 1], X[idx]), dd_add(dd_mul(s_coef[4 * ib + 2], X2[idx]), dd_mul(s_coef[4 * ib + 3], X3[idx])));
        if (i == j) v = dd_add(v, s_coef[4 * ib]);
        return v;
    };
    for (int idx = threadIdx.x; idx < kk; idx += blockDim.x) O[idx] = dd_add(block(3, idx), dd_mul(s_coef[16], X4[idx]));
    __syncthreads();
    for (int ib = 2; ib >= 0; ib--) {
        dd_matmul(k, X4, O, W, strips);
        __syncthreads();
        for (int idx = threadIdx.x; idx < kk; idx += blockDim.x) O[idx] = dd_add(block(ib, idx), W[idx]);
        __syncthreads();
    }
    for (int q = 0; q < sq; q++) {
        dd_matmul(k, O, O, W, strips);
        __syncthreads();
        for (int idx = threadIdx.x; idx < kk; idx += blockDim.x) O[idx] = W[idx];
        __syncthreads();
    }
    const double rc = cat_rates[c];
    if (FRECHET) {
        for (int idx = threadIdx.x; idx < kks; idx += blockDim.x) {
            const int i = idx / ks, j = idx - i * ks;
            dd v = O[i * k + ks + j];
            if (coef_mode == PLK_COEF_PRIOR_RATE_EDGE) v = dd_mul(v, s);
            else if (coef_mode == PLK_COEF_PRIOR_RATE) v = dd_mul_d(v, rc);
            Fout[(size_t)ce * kks + idx] = v.hi;
        }
        return;
    }
    /* outputs: unrounded P, rounded P, rounded dP = r_c * Qn * P */
    for (int idx = threadIdx.x; idx < kk; idx += blockDim.x) {
        dd v = O[idx];
        if (v.hi < 0) v = dd_make(0.0, 0.0);
        Pdd[(size_t)ce * kk + idx] = v;
        P[(size_t)ce * kk + idx] = v.hi;
    }
    if (!post.skip_dP) {
        /* from the clamped matrix, as k_dP_dd computes it later from Pdd: one definition of dP whichever kernel wrote it */
        __syncthreads();
        dd_rate_product(k, Qn, Pdd + (size_t)ce * kk, rc, dP + (size_t)ce * kk, strips);
    }
    if (!FRECHET && post.edge_slot && k == 4) {
        const int mi = post.edge_slot[e], t = post.edge_slot[E + e];
        if (mi >= 0)
            for (int idx = threadIdx.x; idx < 16; idx += blockDim.x) {
                const int j = idx >> 2, i = idx & 3;
                const double v = O[i * 4 + j].hi;
                const size_t slot = (size_t)c * post.nmat1 + mi;
                post.PS[slot * 16 + idx] = v < 0 ? 0.0 : v;
            }
        if (t >= 0)
            for (int idx = threadIdx.x; idx < post.nchar * 4; idx += blockDim.x) {
                const int code = idx >> 2, i = idx & 3;
                const double *d = post.defs + code * 4;
                double out;
                if (d[0] == d[1] && d[0] == d[2] && d[0] == d[3]) out = d[0];      /* src/util.c:276-283 */
                else {
                    dd acc = dd_make(0.0, 0.0);
                    for (int j = 0; j < 4; j++) {
                        dd pij = O[i * 4 + j];
                        if (pij.hi < 0) pij = dd_make(0.0, 0.0);
                        acc = dd_add(acc, dd_mul_d(pij, d[j]));
                    }
                    out = acc.hi;
                }
                post.tip[(((size_t)c * post.ntips1 + t) * post.nchar + code) * 4 + i] = out;
            }
    }
}

/* dP = r_c Qn P for every (category, edge) from the stored double-double P: what K1 skips for an ll evaluation */
__global__ __launch_bounds__(1024) void k_dP_dd(int k, int E, const double *__restrict__ Qn, const double *__restrict__ cat_rates,
                                                const dd *__restrict__ Pdd, double *__restrict__ dP, int tiled)
{
    extern __shared__ double smem_raw[];
    const int ce = blockIdx.x, c = ce / E;
    const size_t kk = (size_t)k * k;
    dd_rate_product(k, Qn, Pdd + ce * kk, cat_rates[c], dP + ce * kk, tiled ? reinterpret_cast<dd *>(smem_raw) : nullptr);
}

/* PS[c][pc][j*K + i] = P[c][edge(pc)][i][j], zero padded to K (transposed so that
 * the column needed for one input state is contiguous for scalar loads) */
__global__ void k_build_stream(int k, int K, int E, int nops, const int *__restrict__ op_edge,
                               const double *__restrict__ P, double *__restrict__ PS)
{
    const int pc = blockIdx.x, c = blockIdx.y;
    const int e = op_edge[pc];
    double *dst = PS + ((size_t)c * nops + pc) * K * K;
    for (int idx = threadIdx.x; idx < K * K; idx += blockDim.x) {
        int j = idx / K, i = idx - j * K;
        double v = 0.0;
        if (e >= 0 && i < k && j < k) v = P[((size_t)c * E + e) * k * k + i * k + j];
        dst[idx] = v;
    }
}

/* tip[c][t][code][i] = sum_j P[c][edge(t)][i][j] * defs[code][j] in dd (k = 4).
 * An exactly constant definition row (e.g. all-ones "missing") maps to itself,
 * which is what the reference's exact shortcut produces (src/util.c:276-283). */
__global__ void k_build_tip(int E, int ntips, int nchar, const int *__restrict__ tip_edge,
                            const dd *__restrict__ Pdd, const double *__restrict__ defs /* [nchar][4] */,
                            double *__restrict__ tip)
{
    const int t = blockIdx.x, c = blockIdx.y;
    const int e = tip_edge[t];
    const dd *Pm = Pdd + ((size_t)c * E + (e < 0 ? 0 : e)) * 16;
    for (int idx = threadIdx.x; idx < nchar * 4; idx += blockDim.x) {
        int code = idx >> 2, i = idx & 3;
        const double *d = defs + code * 4;
        double out;
        if (e < 0) {
            out = d[i];                          /* pseudo slot: the definition itself */
        } else if (d[0] == d[1] && d[0] == d[2] && d[0] == d[3]) {
            out = d[0];
        } else {
            dd acc = dd_make(0.0, 0.0);
            for (int j = 0; j < 4; j++) acc = dd_add(acc, dd_mul_d(Pm[i * 4 + j], d[j]));
            out = acc.hi;
        }
        tip[(((size_t)c * ntips + t) * nchar + code) * 4 + i] = out;
    }
}

/* Tables of the pair-table interpreter (plk_fused4_asm.h: k_ll_fused4_asm_pt), one block per (table, category), from
 * the unrounded P in double-double.  tab[4][ntab]: first unit | edge (leaf edge of a single table, edge above the cherry
 * of a pair table, -1 pseudo) | pair: the two leaf edges, else -1.
 *   single  out[code][i]         = (P_e defs[code])_i
 *   pair    out[cb*nchar+cc][i]  = (P_a (P_b defs[cb] o P_c defs[cc]))_i    (src/evaluate_site_lhood.c:36-56 for a cherry)
 *   pseudo  out[code][i]         = defs[code][i]
 * A constant vector maps to itself exactly under a stochastic matrix, as the reference's shortcut does (src/util.c:276-283). */
/* P_e defs[code] in double-double (a constant definition row maps to itself) */
__device__ __forceinline__ void pt_leaf_dd(const dd *Pm, const double *d, dd (&v)[4])
{
    if (d[0] == d[1] && d[0] == d[2] && d[0] == d[3]) { for (int i = 0; i < 4; i++) v[i] = dd_make(d[0], 0.0); return; }
    for (int i = 0; i < 4; i++) {
        dd acc = dd_make(0.0, 0.0);
        for (int j = 0; j < 4; j++) acc = dd_add(acc, dd_mul_d(Pm[i * 4 + j], d[j]));
        v[i] = acc;
    }
}

/* the rounded row of a cherry's pair table: (P_a (P_b db o P_c dc))_i, the one definition for k_build_tables_pt and k_build_tables_t */
__device__ __forceinline__ void pt_pair_row(const dd *Pa, const dd *Pb, const dd *Pc, const double *db, const double *dc, double *out)
{
    dd vb[4], vc[4], pr[4];
    pt_leaf_dd(Pb, db, vb);
    pt_leaf_dd(Pc, dc, vc);
    bool cst = true;
    for (int j = 0; j < 4; j++) { pr[j] = dd_mul(vb[j], vc[j]); cst = cst && pr[j].hi == pr[0].hi && pr[j].lo == pr[0].lo; }
    for (int i = 0; i < 4; i++) {
        dd acc = pr[0];
        if (!cst) {
            acc = dd_make(0.0, 0.0);
            for (int j = 0; j < 4; j++) acc = dd_add(acc, dd_mul(Pa[i * 4 + j], pr[j]));
        }
        out[i] = acc.hi;
    }
}

__device__ __forceinline__ void build_table_pt(int t, int c, int E, int ntab, int units, int nchar, const int *__restrict__ tab,
                                               const dd *__restrict__ Pdd, const double *__restrict__ defs /* [nchar][4] */,
                                               double *__restrict__ tip)
{
    const int unit = tab[t], e = tab[ntab + t], eb = tab[2 * ntab + t], ec = tab[3 * ntab + t];
    double *out = tip + ((size_t)c * units + unit) * nchar * 4;
    if (eb < 0) {
        const dd *Pm = Pdd + ((size_t)c * E + (e < 0 ? 0 : e)) * 16;
        for (int code = threadIdx.x; code < nchar; code += blockDim.x) {
            const double *d = defs + code * 4;
            dd v[4];
            if (e < 0) { for (int i = 0; i < 4; i++) out[code * 4 + i] = d[i]; continue; }
            pt_leaf_dd(Pm, d, v);
            for (int i = 0; i < 4; i++) out[code * 4 + i] = v[i].hi;
        }
        return;
    }
    const dd *Pa = Pdd + ((size_t)c * E + e) * 16, *Pb = Pdd + ((size_t)c * E + eb) * 16, *Pc = Pdd + ((size_t)c * E + ec) * 16;
    for (int comb = threadIdx.x; comb < nchar * nchar; comb += blockDim.x) {
        const int cb = comb / nchar, cc = comb - cb * nchar;
        pt_pair_row(Pa, Pb, Pc, defs + cb * 4, defs + cc * 4, out + comb * 4);
    }
}

__global__ void k_build_tables_pt(int E, int ntab, int units, int nchar, const int *__restrict__ tab,
                                  const dd *__restrict__ Pdd, const double *__restrict__ defs /* [nchar][4] */,
                                  double *__restrict__ tip)
{
    build_table_pt(blockIdx.x, blockIdx.y, E, ntab, units, nchar, tab, Pdd, defs, tip);
}

/* Three-leaf tables of the streamed form (plk_fused_v4t_build), one block per (table, category): tab[6][ntab] as for
 * k_build_tables_pt, then the edge above the cherry and the leaf edge; the tables built here are first .. first + gridDim.x - 1
 * of the list.  A row is the MATVEC handler's fp64 sequence (plk_v4t_row) on what the interpreter would have looked up and
 * loaded: the rounded row of the cherry's pair table and the rounded row of the leaf's table (pt_pair_row, pt_leaf_dd: the
 * functions k_build_tables_pt writes them with), and the rounded matrix of the edge above the node as K1 writes it to the matrix stream.
 *   out[(cb*nchar+cc)*nchar+cl][i] = (P_d (pair[cb*nchar+cc] o tip[cl]))_i */
__device__ __forceinline__ void build_table_t(int t, int c, int E, int ntab, int units, int nchar, const int *__restrict__ tab,
                                              const dd *__restrict__ Pdd, const double *__restrict__ defs /* [nchar][4] */,
                                              double *__restrict__ tip)
{
    const int unit = tab[t], e = tab[ntab + t], eb = tab[2 * ntab + t], ec = tab[3 * ntab + t], ea = tab[4 * ntab + t], el = tab[5 * ntab + t];
    double *out = tip + ((size_t)c * units + unit) * nchar * 4;
    const dd *Pd = Pdd + ((size_t)c * E + e) * 16, *Pa = Pdd + ((size_t)c * E + ea) * 16, *Pb = Pdd + ((size_t)c * E + eb) * 16,
             *Pc = Pdd + ((size_t)c * E + ec) * 16, *Pl = Pdd + ((size_t)c * E + el) * 16;
    double M[16];
    for (int idx = 0; idx < 16; idx++) M[idx] = Pd[(idx & 3) * 4 + (idx >> 2)].hi;     /* the stream's layout: M[4 j + i] = P[i][j] (Pdd is clamped at 0) */
    for (int comb = threadIdx.x; comb < nchar * nchar * nchar; comb += blockDim.x) {
        const int cl = comb % nchar, cbc = comb / nchar, cb = cbc / nchar, cc = cbc - cb * nchar;
        dd vl[4];
        double pair[4], tipv[4];
        pt_pair_row(Pa, Pb, Pc, defs + cb * 4, defs + cc * 4, pair);
        pt_leaf_dd(Pl, defs + cl * 4, vl);
        for (int i = 0; i < 4; i++) tipv[i] = vl[i].hi;
        plk_v4t_row(M, pair, tipv, out + (size_t)comb * 4);
    }
}

__global__ void k_build_tables_t(int E, int ntab, int first, int units, int nchar, const int *__restrict__ tab,
                                 const dd *__restrict__ Pdd, const double *__restrict__ defs /* [nchar][4] */,
                                 double *__restrict__ tip)
{
    build_table_t(first + blockIdx.x, blockIdx.y, E, ntab, units, nchar, tab, Pdd, defs, tip);
}

/* The tables of formats with four-leaf tables (plk_fused_v4q_build), ALL of them in one launch of 256-thread blocks, one
 * block per (table, category): tables 0 .. first_t - 1 of the list as k_build_tables_pt builds them, first_t .. first_q - 1
 * as k_build_tables_t does (the same device functions; a launch less than the three-leaf form needs, so the step outside
 * the traversal kernel does not grow with the form), the rest four-leaf tables, one row per thread: tab[10][ntab] as
 * above, then shape and the further edges; rank_codes[16 q + 4 j + r] is the code of rank r at leaf j of the q-th
 * four-leaf table (plk_v4q_rank_codes).
 * One set of device functions now serves two launch shapes, and the two must stay in step: without four-leaf tables
 * run_expm still launches k_build_tables_pt and k_build_tables_t on their own, in 64-thread blocks over their part of the
 * list; here build_table_pt / build_table_t run in 256-thread blocks indexed by the whole list.  Both bodies only loop
 * over their rows with a blockDim.x stride, use no barrier and no shared memory, and return for the whole block at once, which is
 * what lets them run in front of this kernel's first __syncthreads; a change to either that breaks one of these breaks the
 * fused launch.  (A single table's nchar rows leave most of a 256-thread block idle; the launch saved outweighs it, see
 * DESIGN.md section 4.)  The
 * operands are the rounded rows k_build_tables_pt writes (pt_pair_row, pt_leaf_dd) and the rounded matrices K1 writes to the
 * matrix stream; every distinct one is computed once per block (16 pair rows and 4 tip rows at most per child, 64 inner
 * rows of shape A), then
 *   A  t[(rb*4+rc)*4+r1] = plk_v4t_row(M_et, pair[rb*4+rc], tip1[r1]);  out[.. *4 + r2] = plk_v4t_row(M_ed, t, tip2[r2])
 *   B  out[(rb*4+rc)*16 + rf*4+rg] = plk_v4t_row(M_ed, pair[rb*4+rc], pair2[rf*4+rg])
 * The elementwise product inside plk_v4t_row is the TIP_MUL / POPMUL handlers' v_mul_f64, which commutes bit for bit. */
__global__ __launch_bounds__(256) void k_build_tables_q(int E, int ntab, int first_t, int first_q, int units, int nchar, const int *__restrict__ tab,
                                                        const int *__restrict__ rank_codes, const dd *__restrict__ Pdd,
                                                        const double *__restrict__ defs /* [nchar][4] */, double *__restrict__ tip)
{
    __shared__ double s_pair[2][16][4], s_tip[2][4][4], s_t[64][4], s_M[2][16];
    const int t = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    /* block-uniform: the whole block leaves before the first barrier */
    if (t < first_t) { build_table_pt(t, c, E, ntab, units, nchar, tab, Pdd, defs, tip); return; }
    if (t < first_q) { build_table_t(t, c, E, ntab, units, nchar, tab, Pdd, defs, tip); return; }
    const int unit = tab[t], e = tab[ntab + t], eb = tab[2 * ntab + t], ec = tab[3 * ntab + t], ea = tab[4 * ntab + t], el = tab[5 * ntab + t],
              shape = tab[6 * ntab + t], et = tab[7 * ntab + t], ef = tab[8 * ntab + t], eg = tab[9 * ntab + t];
    const int *rc4 = rank_codes + 16 * (size_t)(t - first_q);
    const dd *Pc0 = Pdd + (size_t)c * E * 16;
    double *out = tip + ((size_t)c * units + unit) * nchar * 4;
    const bool A = shape == PLK_V4Q_A;
    if (tid < 16) {
        pt_pair_row(Pc0 + (size_t)ea * 16, Pc0 + (size_t)eb * 16, Pc0 + (size_t)ec * 16, defs + rc4[tid >> 2] * 4, defs + rc4[4 + (tid & 3)] * 4, s_pair[0][tid]);
    } else if (tid < 32 && !A) {
        const int q = tid - 16;
        pt_pair_row(Pc0 + (size_t)et * 16, Pc0 + (size_t)ef * 16, Pc0 + (size_t)eg * 16, defs + rc4[8 + (q >> 2)] * 4, defs + rc4[12 + (q & 3)] * 4, s_pair[1][q]);
    } else if (tid < 24 && A) {
        const int q = tid - 16, which = q >> 2, r = q & 3;
        dd v[4];
        pt_leaf_dd(Pc0 + (size_t)(which ? ef : el) * 16, defs + rc4[8 + 4 * which + r] * 4, v);
        for (int i = 0; i < 4; i++) s_tip[which][r][i] = v[i].hi;
    } else if (tid >= 64 && tid < 96) {
        /* the stream's layout: M[4 j + i] = P[i][j] (Pdd is clamped at 0); matrix 0 above d, matrix 1 above t (shape A) */
        const int m = (tid - 64) >> 4, idx = tid & 15;
        if (m == 0 || A) s_M[m][idx] = Pc0[(size_t)(m ? et : e) * 16 + (idx & 3) * 4 + (idx >> 2)].hi;
    }
    __syncthreads();
    if (A && tid < 64) plk_v4t_row(s_M[1], s_pair[0][tid >> 2], s_tip[0][tid & 3], s_t[tid]);
    __syncthreads();
    if (A) plk_v4t_row(s_M[0], s_t[tid >> 2], s_tip[1][tid & 3], out + (size_t)tid * 4);
    else plk_v4t_row(s_M[0], s_pair[0][tid >> 4], s_pair[1][tid & 15], out + (size_t)tid * 4);
    /* the rows that round the table up to whole units: no byte can name them; zero, so that the staged image is defined */
    const int spare = plk_v4q_units(nchar) * nchar - PLK_V4Q_ROWS;
    if (tid < spare) for (int i = 0; i < 4; i++) out[(size_t)(PLK_V4Q_ROWS + tid) * 4 + i] = 0.0;
}

/* flags[n] bit 0: some site's code at node n is not an all-ones definition; bit 1: some code is >= nchar
 * (the kernels index LDS and the tip tables with the codes: an out-of-range code must never reach them); bit 2: some
 * code's definition is not a single 1.0 among zeros (code_trivial[ch]: bit 0 all-ones definition, bit 1 single state).
 * seen[n] (nchar <= 16, else not touched): bit `code` set when some site < S carries that code at node n (four-leaf tables) */
__global__ void k_node_flags(long S, long Spad, const uint8_t *__restrict__ codes, int nchar,
                             const int *__restrict__ code_trivial, int *__restrict__ flags, int *__restrict__ seen)
{
    /* 16 codes per lane and iteration (rows are 1024-byte padded with code 0 beyond S;
     * the tail is masked), grid-stride over the row */
    const int n = blockIdx.y;
    const uint4 *row = reinterpret_cast<const uint4 *>(codes + (size_t)n * Spad);
    const long nvec = (S + 15) / 16;
    int bad = 0, mask = 0;
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (long)gridDim.x * blockDim.x) {
        const uint4 q = row[v];
        const unsigned wds[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const long s = v * 16 + j;
            const int ch = (wds[j >> 2] >> ((j & 3) * 8)) & 0xff;
            if (s < S) {
                const int ct = ch >= nchar ? 0 : code_trivial[ch]; bad |= ch >= nchar ? 2 : ((ct & 1) ? 0 : 1) | ((ct & 2) ? 0 : 4);
                if (ch < 16) mask |= 1 << ch;
            }
        }
    }
    const int wbad = (__any(bad & 1) ? 1 : 0) | (__any(bad & 2) ? 2 : 0) | (__any(bad & 4) ? 4 : 0);
    if (wbad && (threadIdx.x & 63) == 0) atomicOr(&flags[n], wbad);
    if (nchar <= 16) {
        for (int off = 32; off > 0; off >>= 1) mask |= __shfl_xor(mask, off, 64);
        if (mask && (threadIdx.x & 63) == 0) atomicOr(&seen[n], mask);
    }
}

/* ====================================================================== */
/* deterministic double-double reductions                                  */
/* ====================================================================== */

__device__ static inline dd dd_wave_sum(dd v)
{
    for (int off = 32; off > 0; off >>= 1) {
        dd o;
        o.hi = __shfl_down(v.hi, off, 64);
        o.lo = __shfl_down(v.lo, off, 64);
        v = dd_add(v, o);
    }
    return v;
}

/* block-wide dd sum, result valid in thread 0; blockDim.x multiple of 64, <= 1024 */
__device__ static inline dd dd_block_sum(dd v)
{
    __shared__ double sh_hi[16], sh_lo[16];
    v = dd_wave_sum(v);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) { sh_hi[wave] = v.hi; sh_lo[wave] = v.lo; }
    __syncthreads();
    dd r = dd_make(0.0, 0.0);
    if (threadIdx.x == 0) {
        const int nw = (blockDim.x + 63) >> 6;
        for (int i = 0; i < nw; i++) r = dd_add(r, dd_make(sh_hi[i], sh_lo[i]));
    }
    return r;
}

/* out[row] = sum over blocks of partial[row][block]; one block per row */
__global__ void k_dd_final(int nblocks, const dd *__restrict__ partial, dd *__restrict__ out)
{
    const int row = blockIdx.x;
    dd acc = dd_make(0.0, 0.0);
    for (int b = threadIdx.x; b < nblocks; b += blockDim.x) acc = dd_add(acc, partial[(size_t)row * nblocks + b]);
    dd r = dd_block_sum(acc);
    if (threadIdx.x == 0) out[row] = r;
}

/* out[b] = sum of the b-th of gridDim.x contiguous slices of partial[0 .. n) */
__global__ void k_dd_slices(int n, const dd *__restrict__ partial, dd *__restrict__ out)
{
    const int per = (n + gridDim.x - 1) / gridDim.x;
    const int lo = blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    dd acc = dd_make(0.0, 0.0);
    for (int b = lo + threadIdx.x; b < hi; b += blockDim.x) acc = dd_add(acc, partial[b]);
    dd r = dd_block_sum(acc);
    if (threadIdx.x == 0) out[blockIdx.x] = r;
}

/* partial[row][block] = sum_{s in block's range} w[s] * X[row][s] */
__global__ void k_wsum_rows(long S, long row_stride, const double *__restrict__ X,
                            const double *__restrict__ w, int nblocks, dd *__restrict__ partial)
{
    const int row = blockIdx.y;
    const long per = (S + nblocks - 1) / nblocks;
    const long lo = (long)blockIdx.x * per;
    const long hi = lo + per < S ? lo + per : S;
    dd acc = dd_make(0.0, 0.0);
    for (long s = lo + threadIdx.x; s < hi; s += blockDim.x) {
        double x = X[(size_t)row * row_stride + s];
        dd t = dd_weighted(w, s, x);
        acc = dd_add(acc, t);
    }
    dd r = dd_block_sum(acc);
    if (threadIdx.x == 0) partial[(size_t)row * nblocks + blockIdx.x] = r;
}

/* ---- site sums taken where the values are produced (site-aggregated marginals; src/arbplfmarginal.c:237-256) ----
 * Cross-lane sums by data-parallel-primitive moves: every lane of a row of 16 ends with the row's sum (quad swaps,
 * half-row mirror, row mirror), then row 3 collects the four rows (row broadcasts): lane 63 holds the sum of the 64
 * lanes.  All lanes must be active; lanes without a site contribute 0.  Plain fp64 within the wave (a pairwise tree of
 * 64 terms), double-double across waves afterwards (k_wsum_rows / k_dd_final). */
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_fetch(double x)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, ROW_MASK, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double row16_sum(double x)
{
    x += dpp_fetch<0xB1, 0xf>(x);      /* quad_perm [1,0,3,2] */
    x += dpp_fetch<0x4E, 0xf>(x);      /* quad_perm [2,3,0,1] */
    x += dpp_fetch<0x141, 0xf>(x);     /* row_half_mirror */
    x += dpp_fetch<0x140, 0xf>(x);     /* row_mirror */
    return x;
}
__device__ __forceinline__ double wave64_sum_lane63(double x)
{
    x = row16_sum(x);
    x += dpp_fetch<0x142, 0xa>(x);     /* row_bcast15 into rows 1 and 3 */
    x += dpp_fetch<0x143, 0xc>(x);     /* row_bcast31 into rows 2 and 3 */
    return x;
}

#include "plk_fused4.h"
#include "plk_fused4_asm.h"
#include "plk_fused4_v4.h"
#include "plk_fused4_v4s.h"
#include "plk_mfma.h"
#include "plk_mfma_updown.h"
#include "plk_vec.h"
#include "plk_updown_vec.h"
#include "plk_updown4.h"
#include "plk_hess4.h"

/* ====================================================================== */
/* K2+K3 generic: any k <= K, stack slots in HBM                           */
/* ====================================================================== */

struct GenArgs {
    long S, Spad;
    int k, C, nops, nchar, pat_mode, root_mode;
    const int2 *ops;
    const double *PS;        /* [C][nops][K*K] transposed, zero padded */
    const uint8_t *codes;    /* [N][Spad] */
    const double *defs;      /* [nchar][K] zero padded */
    const double *B;         /* [N][k][S] */
    const double *cat_prior, *root_w, *w;
    double *slots;           /* [nslots][k][S] */
    double *site_ll;
    dd *partial;
};

#define GEN_BLOCK 64

template <int K>
__device__ static inline void gen_load_obs(const GenArgs &a, int node, long sc, int tid, double (*xs)[GEN_BLOCK])
{
    if (a.pat_mode == 1) {
        const int ch = a.codes[(size_t)node * a.Spad + sc];
        const double *dv = a.defs + (size_t)ch * K;
        for (int j = 0; j < a.k; j++) xs[j][tid] = dv[j];
    } else {
        const double *bp = a.B + (size_t)node * a.k * a.S + sc;
        for (int j = 0; j < a.k; j++) xs[j][tid] = bp[(size_t)j * a.S];
    }
}

template <int K>
__global__ __launch_bounds__(GEN_BLOCK) void k_ll_generic(GenArgs a)
{
    __shared__ double xs[K][GEN_BLOCK];
    const int tid = threadIdx.x;
    const long s = (long)blockIdx.x * GEN_BLOCK + tid;
    const bool valid = s < a.S;
    const long sc = valid ? s : a.S - 1;

    double sum = 0.0;
    int Eexp = 0;
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
        const double term = a.cat_prior[c] * lh;
        if (term != 0.0) {
            if (!have) { sum = term; Eexp = esc; have = true; }
            else if (esc > Eexp) { sum = ldexp(sum, Eexp - esc) + term; Eexp = esc; }
            else sum += ldexp(term, esc - Eexp);
        }
    }
    const double ll = have ? log(sum) + (double)Eexp * 0.6931471805599453094 : -INFINITY;
    if (valid && a.site_ll) a.site_ll[s] = ll;
    if (a.partial) {
        dd v = dd_make(0.0, 0.0);
        if (valid) v = dd_weighted(a.w, s, ll);
        dd r = dd_block_sum(v);
        if (tid == 0) a.partial[blockIdx.x] = r;
    }
}

/*
 * Dynamic range of the passes that store node vectors, on a tree with a node that is rescaled inside (PlkProgram::mid_scales).
 * Those passes keep one factor per node, so they skip the OP_SCALE ops inside a node (op_mid) and see the node's whole
 * product at the OP_SCALE after its last child.  This kernel walks the program the same way and raises *flag where such a
 * product, or the root vector, has no entry of at least 2^-969 in some category at some site: below that magnitude an entry
 * within 2^-53 of the largest can be subnormal, and the stored vectors are no longer good to the stated bars.  A product
 * that is exactly zero because every entry took a factor of exactly 0.0 (the rate-0 category, P = I, under leaves that show
 * different states) has left no range: `live` keeps one bit per entry, cleared by the first zero factor, and only a product
 * with a live entry can be low.  The matrices are read by edge (PS = [C][E][K*K], transposed).  No output but the flag.
 */
template <int K>
__global__ __launch_bounds__(GEN_BLOCK) void k_range_check(GenArgs a, int E, const int *op_edge, const int *op_mid, int *flag)
{
    __shared__ double xs[K][GEN_BLOCK];
    const int tid = threadIdx.x;
    const long s = (long)blockIdx.x * GEN_BLOCK + tid;
    const bool valid = s < a.S;
    const long sc = valid ? s : a.S - 1;
    bool low = false;
    const unsigned long long kmask = a.k >= 64 ? ~0ull : (1ull << a.k) - 1;     /* the k entries of a vector (K >= k is padding) */
    for (int c = 0; c < a.C; c++) {
        double cur[K];
#pragma unroll
        for (int i = 0; i < K; i++) cur[i] = 1.0;
        unsigned long long live = ~0ull;
        for (int pc = 0; pc < a.nops; pc++) {
            const int ox = as_uniform(reinterpret_cast<const int *>(a.ops))[2 * pc], oy = as_uniform(reinterpret_cast<const int *>(a.ops))[2 * pc + 1];
            const int code = ox & 0xff;
            if (code == OP_MATVEC || code == OP_TIP_SET || code == OP_TIP_MUL) {
                if (code == OP_MATVEC) {
#pragma unroll
                    for (int j = 0; j < K; j++) xs[j][tid] = cur[j];
                } else {
                    gen_load_obs<K>(a, oy, sc, tid, xs);
                }
                const double *M = a.PS + ((size_t)c * E + as_uniform(op_edge)[pc]) * K * K;
                double acc[K];
#pragma unroll
                for (int i = 0; i < K; i++) acc[i] = 0.0;
                for (int j = 0; j < a.k; j++) {
                    const double x = xs[j][tid];
                    const double *col = M + j * K;
#pragma unroll
                    for (int i = 0; i < K; i++) acc[i] = fma(col[i], x, acc[i]);
                }
#pragma unroll
                for (int i = 0; i < K; i++) cur[i] = code == OP_TIP_MUL ? cur[i] * acc[i] : acc[i];
                if (code != OP_TIP_MUL) live = ~0ull;
#pragma unroll
                for (int i = 0; i < K; i++)
                    if (i < a.k && acc[i] == 0.0) live &= ~(1ull << i);
            } else if (code == OP_PUSH) {
                double *sp = a.slots + (size_t)oy * a.k * a.S + sc;
#pragma unroll
                for (int i = 0; i < K; i++)
                    if (i < a.k && valid) sp[(size_t)i * a.S] = cur[i];
            } else if (code == OP_POPMUL) {
                const double *sp = a.slots + (size_t)oy * a.k * a.S + sc;
#pragma unroll
                for (int i = 0; i < K; i++)
                    if (i < a.k) {
                        const double x = valid ? sp[(size_t)i * a.S] : 1.0;
                        cur[i] *= x;
                        if (x == 0.0) live &= ~(1ull << i);
                    }
            } else if (code == OP_NODE_MUL) {
                gen_load_obs<K>(a, oy, sc, tid, xs);
#pragma unroll
                for (int i = 0; i < K; i++)
                    if (i < a.k) {
                        cur[i] *= xs[i][tid];
                        if (xs[i][tid] == 0.0) live &= ~(1ull << i);
                    }
            } else if (code == OP_SCALE && !as_uniform(op_mid)[pc]) {
                double m = 0.0;
#pragma unroll
                for (int i = 0; i < K; i++) m = fmax(m, cur[i]);
                if (!(m >= 0x1p-969) && (live & kmask)) low = true;
                const int e = frexp_exp(m);
#pragma unroll
                for (int i = 0; i < K; i++) cur[i] = ldexp(cur[i], -e);
            }
        }
        double m = 0.0;
#pragma unroll
        for (int i = 0; i < K; i++) m = fmax(m, cur[i]);
        if (!(m >= 0x1p-969) && (live & kmask)) low = true;
    }
    if (low && valid) *flag = 1;
}

#include "plk_catpost.h"

/* ====================================================================== */
/* K2 with stored vectors + K4/K5/K6 (up pass): deriv and marginal         */
/* ====================================================================== */

struct UpArgs {
    long S, Spad;        /* full pattern extent (row pitch of codes / B) */
    long s0, n;          /* chunk [s0, s0+n) */
    int N, E, k, C, nchar, pat_mode, root_mode;
    int dzero;           /* 1: the edge-form matrices have zero row sums (dP): exact zero for constant inputs */
    const int *indptr, *indices, *preorder;
    const int *node_has_data;  /* N */
    const double *PT;    /* [C][E][K*K] transposed P:  PT[j*K+i] = P[i][j]  */
    const double *PN;    /* [C][E][K*K] plain P:       PN[i*K+j] = P[i][j]  */
    const double *DT;    /* [C][E][K*K] transposed dP: DT[j*K+i] = dP[i][j] */
    /* second-order passes (plk_hess): edge mod_edge uses dP in the role of P and d2P = r^2 Q Q P in the
     * role of dP; DN = plain dP, D2T = transposed d2P; LHdiv = likelihoods of the unmodified model */
    int mod_edge;        /* -1: none */
    const double *DN, *D2T, *LHdiv;
    /* exact power-of-two rescaling (deriv / marginal / edge expectations; off for the Hessian passes):
     * node_scale[N] = slot or -1 (null = no rescaling), SC[(slot*C + c)][n] = 2^-e, CW[C][n] = 2^(X_c - Xmax) */
    const int *node_scale;
    double *SC, *CW, *XC;
    double *XM;          /* [n] or null: the common exponent Xmax of the site (LH and the edge forms are at 2^Xmax) */
    const double *XMdiv; /* [n] or null: Xmax of the model LHdiv belongs to (second-order passes) */
    const uint8_t *codes;
    const double *defs;  /* [nchar][K] */
    const double *B;     /* [N][k][S] */
    const double *cat_prior, *root_w;
    const int *edge_mask, *node_mask;   /* device, may be null = all */
    double *EV;          /* [E][C][k][n] */
    double *LN;          /* [N][C][k][n] (internal nodes only are written) */
    double *FN;          /* [N][C][k][n] */
    double *LH;          /* [n] site likelihood */
    double *DV;          /* [E][n] derivative values */
    double *MV;          /* [N][k][n] marginal values */
};

template <int K>
__device__ static inline void up_load_obs_reg(const UpArgs &a, int node, long sg, double (&out)[K])
{
    if (a.pat_mode == 1) {
        const int ch = a.codes[(size_t)node * a.Spad + sg];
        const double *dv = a.defs + (size_t)ch * K;
#pragma unroll
        for (int i = 0; i < K; i++) out[i] = dv[i];
    } else {
        const double *bp = a.B + (size_t)node * a.k * a.S + sg;
#pragma unroll
        for (int i = 0; i < K; i++) out[i] = i < a.k ? bp[(size_t)i * a.S] : 0.0;
    }
}

template <int K>
__device__ static inline void up_stage_obs(const UpArgs &a, int node, long sg, int tid, double (*xs)[GEN_BLOCK])
{
    if (a.pat_mode == 1) {
        const int ch = a.codes[(size_t)node * a.Spad + sg];
        const double *dv = a.defs + (size_t)ch * K;
        for (int j = 0; j < a.k; j++) xs[j][tid] = dv[j];
    } else {
        const double *bp = a.B + (size_t)node * a.k * a.S + sg;
        for (int j = 0; j < a.k; j++) xs[j][tid] = bp[(size_t)j * a.S];
    }
}

/* acc[i] = sum_j M[j*K+i] * xs[j]  (M uniform, zero padded).
 * CONST_MODE mirrors the reference's exact shortcut for a constant input column
 * (src/util.c:276-283, :338-345; src/arb_mat_extras.c:36-51): a stochastic matrix maps
 * it to itself (1), a rate matrix with zero row sums maps it to zero (2). */
template <int K, int CONST_MODE>
__device__ static inline void up_matvec(const double *M, int k, double (*xs)[GEN_BLOCK], int tid, double (&acc)[K])
{
#pragma unroll
    for (int i = 0; i < K; i++) acc[i] = 0.0;
    const double x0 = xs[0][tid];
    bool is_const = true;
    for (int j = 0; j < k; j++) {
        const double x = xs[j][tid];
        is_const = is_const && (x == x0);
        const double *col = M + j * K;
#pragma unroll
        for (int i = 0; i < K; i++) acc[i] = fma(col[i], x, acc[i]);
    }
    if (CONST_MODE != 0 && is_const) {
#pragma unroll
        for (int i = 0; i < K; i++) acc[i] = (CONST_MODE == 1 && i < k) ? x0 : 0.0;
    }
}

/* down pass storing every edge vector and internal node vector (no rescaling) */
template <int K>
__global__ __launch_bounds__(GEN_BLOCK) void k_down_store(UpArgs a)
{
    __shared__ double xs[K][GEN_BLOCK];
    const int tid = threadIdx.x;
    const long sl = (long)blockIdx.x * GEN_BLOCK + tid;   /* local site */
    const bool valid = sl < a.n;
    const long slc = valid ? sl : a.n - 1;
    const long sg = a.s0 + slc;
    const size_t n = (size_t)a.n;
    double lh_total = 0.0;
    int xmax = INT_MIN, xall = INT_MIN;
    for (int c = 0; c < a.C; c++) {
        double lh_c = 0.0;
        int X = 0;
        for (int u = a.N - 1; u >= 0; u--) {
            const int nd = as_uniform(a.preorder)[u];
            const int start = as_uniform(a.indptr)[nd], stop = as_uniform(a.indptr)[nd + 1];
            if (start == stop) continue;
            double acc[K];
            if (as_uniform(a.node_has_data)[nd]) up_load_obs_reg<K>(a, nd, sg, acc);
            else {
#pragma unroll
                for (int i = 0; i < K; i++) acc[i] = 1.0;
            }
            for (int idx = start; idx < stop; idx++) {
                const int b = as_uniform(a.indices)[idx];
                const bool b_leaf = as_uniform(a.indptr)[b] == as_uniform(a.indptr)[b + 1];
                if (b_leaf) up_stage_obs<K>(a, b, sg, tid, xs);
                else {
                    const double *lb = a.LN + ((size_t)b * a.C + c) * a.k * n + slc;
                    for (int j = 0; j < a.k; j++) xs[j][tid] = lb[(size_t)j * n];
                }
                double m[K];
                if (idx == a.mod_edge) up_matvec<K, 2>(a.DT + ((size_t)c * a.E + idx) * K * K, a.k, xs, tid, m);
                else up_matvec<K, 1>(a.PT + ((size_t)c * a.E + idx) * K * K, a.k, xs, tid, m);
                /* leaf-edge vectors are not stored: the up pass recomputes them (k^2 flops vs 2k doubles of HBM) */
                double *ev = a.EV + ((size_t)idx * a.C + c) * a.k * n + slc;
#pragma unroll
                for (int i = 0; i < K; i++) {
                    if (!b_leaf && i < a.k && valid) ev[(size_t)i * n] = m[i];
                    acc[i] *= m[i];
                }
            }
            const int slot = a.node_scale ? as_uniform(a.node_scale)[nd] : -1;
            if (slot >= 0) {
                double mx = 0.0;       /* |.|: the vectors of an edge-modified model (plk_hess) are not sign definite */
#pragma unroll
                for (int i = 0; i < K; i++) mx = fmax(mx, fabs(acc[i]));
                double sc = 1.0;
                if (mx > 0x1p-1000 && mx < 0x1p+1000) {
                    const int e = ilogb(mx);
                    sc = ldexp(1.0, -e);
#pragma unroll
                    for (int i = 0; i < K; i++) acc[i] *= sc;
                    X += e;
                }
                if (valid) a.SC[((size_t)slot * a.C + c) * n + sl] = sc;
            }
            double *ln = a.LN + ((size_t)nd * a.C + c) * a.k * n + slc;
#pragma unroll
            for (int i = 0; i < K; i++)
                if (i < a.k && valid) ln[(size_t)i * n] = acc[i];
            if (u == 0) {
                if (a.root_mode == PLK_ROOT_NONE || a.root_mode == PLK_ROOT_UNIFORM) {
#pragma unroll
                    for (int i = 0; i < K; i++)
                        if (i < a.k) lh_c += acc[i];
                    if (a.root_mode == PLK_ROOT_UNIFORM) lh_c /= (double)a.k;
                } else {
#pragma unroll
                    for (int i = 0; i < K; i++) lh_c = fma(as_uniform(a.root_w)[i], acc[i], lh_c);
                }
            }
        }
        if (!a.node_scale) { lh_total = fma(as_uniform(a.cat_prior)[c], lh_c, lh_total); continue; }
        lh_c *= as_uniform(a.cat_prior)[c];
        if (lh_c != 0.0 && X > xmax) xmax = X;
        if (X > xall) xall = X;
        if (valid) { a.XC[(size_t)c * n + sl] = (double)X; a.CW[(size_t)c * n + sl] = lh_c; }
    }
    if (a.node_scale && valid) {
        /* combine the categories at the largest exponent: LH = sum_c prior_c lh_c 2^(X_c - Xmax).  When every term is
         * zero (an edge-modified model of plk_hess at a site that does not depend on the edge) the exponent of the
         * vectors themselves is kept, so that the division by the unmodified likelihood stays finite */
        /* (a category whose own term is exactly zero takes no part in xmax; were its X_c more than 1023 above xmax, its
         * weight 2^(X_c - xmax) below would overflow.  Not reached by any known input; k_hess4_down does the same) */
        if (xmax == INT_MIN) xmax = xall == INT_MIN ? 0 : xall;
        if (a.XM) a.XM[sl] = (double)xmax;
        for (int c = 0; c < a.C; c++) {
            const double w = ldexp(1.0, (int)a.XC[(size_t)c * n + sl] - xmax);
            lh_total = fma(a.CW[(size_t)c * n + sl], w, lh_total);
            a.CW[(size_t)c * n + sl] = w;
        }
    }
    if (valid) a.LH[sl] = lh_total;
}

/*
 * up pass in BFS order.  For every edge e = (a -> b):
 *   fe   = F_a o B_a o prod_{siblings j != e} Ev_j          (src/evaluate_site_forward.c:69-94)
 *   d_e  = sum_c prior_c * fe . (dP_{c,e} L_b) / lhood       (dP = r_c Q P; equals the reference's
 *          rate * rootward recomputation with Q Ev_e, src/arbplfderiv.c:112-207, :312-342)
 *   F_b  = P_e^T fe                                          (src/evaluate_site_forward.c:97-100)
 *   m_b  = sum_c prior_c * F_b o L_b / lhood                 (src/arbplfmarginal.c:206-234)
 */
template <int K, bool DERIV, bool MARG>
__global__ __launch_bounds__(GEN_BLOCK) void k_up(UpArgs a)
{
    __shared__ double xs[K][GEN_BLOCK];
    const int tid = threadIdx.x;
    const long sl = (long)blockIdx.x * GEN_BLOCK + tid;
    const bool valid = sl < a.n;
    const long slc = valid ? sl : a.n - 1;
    const long sg = a.s0 + slc;
    const size_t n = (size_t)a.n;
    /* second-order passes divide by the likelihood of the unmodified model, which sits at its own exponent */
    double inv = 1.0 / (a.LHdiv ? a.LHdiv[slc] : a.LH[slc]);
    if (a.LHdiv && a.XM && a.XMdiv) inv = ldexp(inv, (int)(a.XM[slc] - a.XMdiv[slc]));
    const int root = as_uniform(a.preorder)[0];

    /* root: forward vector = root prior weights; its marginal */
    {
        double macc[K];
#pragma unroll
        for (int i = 0; i < K; i++) macc[i] = 0.0;
        for (int c = 0; c < a.C; c++) {
            double *fr = a.FN + ((size_t)root * a.C + c) * a.k * n + slc;
            const double *lr = a.LN + ((size_t)root * a.C + c) * a.k * n + slc;
#pragma unroll
            for (int i = 0; i < K; i++) {
                if (i < a.k) {
                    if (valid) fr[(size_t)i * n] = as_uniform(a.root_w)[i];
                    if (MARG) macc[i] = fma(as_uniform(a.cat_prior)[c] * (a.CW ? a.CW[(size_t)c * n + slc] : 1.0) * as_uniform(a.root_w)[i], lr[(size_t)i * n], macc[i]);
                }
            }
        }
        if (MARG && (!a.node_mask || as_uniform(a.node_mask)[root])) {
            double *mv = a.MV + (size_t)root * a.k * n + slc;
#pragma unroll
            for (int i = 0; i < K; i++)
                if (i < a.k && valid) mv[(size_t)i * n] = macc[i] * inv;
        }
    }

    for (int u = 0; u < a.N; u++) {
        const int nd = as_uniform(a.preorder)[u];
        const int start = as_uniform(a.indptr)[nd], stop = as_uniform(a.indptr)[nd + 1];
        if (start == stop) continue;
        double bnd[K];
        const bool has = as_uniform(a.node_has_data)[nd];
        if (has) up_load_obs_reg<K>(a, nd, sg, bnd);
        const int slot = a.node_scale ? as_uniform(a.node_scale)[nd] : -1;
        for (int idx = start; idx < stop; idx++) {
            const int b = as_uniform(a.indices)[idx];
            const bool b_leaf = as_uniform(a.indptr)[b] == as_uniform(a.indptr)[b + 1];
            const bool want_d = DERIV && (!a.edge_mask || as_uniform(a.edge_mask)[idx]);
            const bool want_m = MARG && (!a.node_mask || as_uniform(a.node_mask)[b]);
            const bool want_f = !b_leaf || want_m;
            if (!want_d && !want_f) continue;
            double dsum = 0.0;
            double macc[K];
#pragma unroll
            for (int i = 0; i < K; i++) macc[i] = 0.0;
            for (int c = 0; c < a.C; c++) {
                double fe[K];
                const double *fa = a.FN + ((size_t)nd * a.C + c) * a.k * n + slc;
#pragma unroll
                for (int i = 0; i < K; i++) fe[i] = i < a.k ? fa[(size_t)i * n] : 0.0;
                if (has) {
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
                        if (idx2 == a.mod_edge) up_matvec<K, 2>(a.DT + ((size_t)c * a.E + idx2) * K * K, a.k, xs, tid, m2);
                        else up_matvec<K, 1>(a.PT + ((size_t)c * a.E + idx2) * K * K, a.k, xs, tid, m2);
#pragma unroll
                        for (int i = 0; i < K; i++) fe[i] *= m2[i];
                    } else {
                        const double *ev = a.EV + ((size_t)idx2 * a.C + c) * a.k * n + slc;
#pragma unroll
                        for (int i = 0; i < K; i++)
                            if (i < a.k) fe[i] *= ev[(size_t)i * n];
                    }
                }
                const double prior = as_uniform(a.cat_prior)[c] * (a.CW ? a.CW[(size_t)c * n + slc] : 1.0);
                if (want_d) {
                    /* y = dP_e * L_b ; d = fe . y */
                    if (b_leaf) up_stage_obs<K>(a, b, sg, tid, xs);
                    else {
                        const double *lb = a.LN + ((size_t)b * a.C + c) * a.k * n + slc;
                        for (int j = 0; j < a.k; j++) xs[j][tid] = lb[(size_t)j * n];
                    }
                    double y[K];
                    if (idx == a.mod_edge) up_matvec<K, 2>(a.D2T + ((size_t)c * a.E + idx) * K * K, a.k, xs, tid, y);
                    else if (a.dzero) up_matvec<K, 2>(a.DT + ((size_t)c * a.E + idx) * K * K, a.k, xs, tid, y);
                    else up_matvec<K, 0>(a.DT + ((size_t)c * a.E + idx) * K * K, a.k, xs, tid, y);
                    double d = 0.0;
#pragma unroll
                    for (int i = 0; i < K; i++) d = fma(fe[i], y[i], d);
                    dsum = fma(prior, d, dsum);
                }
                if (want_f) {
                    /* F_b[j] = sum_i P[i][j] fe[i]: stage fe, use the plain (row-major) P as the "transposed" operand */
#pragma unroll
                    for (int i = 0; i < K; i++) xs[i][tid] = fe[i];
                    double fb[K];
                    up_matvec<K, 0>((idx == a.mod_edge ? a.DN : a.PN) + ((size_t)c * a.E + idx) * K * K, a.k, xs, tid, fb);
                    if (!b_leaf) {
                        double *fo = a.FN + ((size_t)b * a.C + c) * a.k * n + slc;
#pragma unroll
                        for (int i = 0; i < K; i++)
                            if (i < a.k && valid) fo[(size_t)i * n] = fb[i];
                    }
                    if (want_m) {
                        if (b_leaf) {
                            double lb[K];
                            up_load_obs_reg<K>(a, b, sg, lb);
#pragma unroll
                            for (int i = 0; i < K; i++) macc[i] = fma(prior * fb[i], lb[i], macc[i]);
                        } else {
                            const double *lb = a.LN + ((size_t)b * a.C + c) * a.k * n + slc;
#pragma unroll
                            for (int i = 0; i < K; i++)
                                if (i < a.k) macc[i] = fma(prior * fb[i], lb[(size_t)i * n], macc[i]);
                        }
                    }
                }
            }
            if (want_d && valid) a.DV[(size_t)idx * n + sl] = dsum * inv;
            if (want_m) {
                double *mv = a.MV + (size_t)b * a.k * n + slc;
#pragma unroll
                for (int i = 0; i < K; i++)
                    if (i < a.k && valid) mv[(size_t)i * n] = macc[i] * inv;
            }
        }
    }
}

#include "plk_pairsums.h"
#include "plk_mixsens.h"
#include "plk_nni.h"
#include "plk_place.h"
#include "plk_spr.h"

/* padded edge-indexed matrix streams for the up/down kernels:
 * mode 0: out[j*K+i] = M[i][j] (transposed), mode 1: out[i*K+j] = M[i][j] */
__global__ void k_build_edge_stream(int k, int K, int mode, const double *__restrict__ M, double *__restrict__ out)
{
    const size_t ce = blockIdx.x;
    const double *src = M + ce * k * k;
    double *dst = out + ce * K * K;
    for (int idx = threadIdx.x; idx < K * K; idx += blockDim.x) {
        int r = idx / K, q = idx - r * K;
        double v = 0.0;
        if (r < k && q < k) v = mode == 0 ? src[q * k + r] : src[r * k + q];
        dst[idx] = v;
    }
}

/* ====================================================================== */
/* host side                                                               */
/* ====================================================================== */

static int pad_K(int k)
{
    const int ks[] = {2, 4, 8, 16, 20, 32, 61, 64};
    for (int v : ks) if (k <= v) return v;
    return -1;
}

extern "C" const char *plk_create_error(void) { return g_create_error.c_str(); }

extern "C" int plk_create(plk_engine **out, int device)
{
    if (!out) return PLK_E_ARG;
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_create_error = std::string("plk_create: no HIP device available (") +
                         (e != hipSuccess ? hipGetErrorString(e) : "device count 0") +
                         "); this engine has no CPU fallback";
        return PLK_E_DEVICE;
    }
    if (device < 0 || device >= ndev) {
        g_create_error = "plk_create: device index out of range";
        return PLK_E_ARG;
    }
    e = hipSetDevice(device);
    if (e != hipSuccess) {
        g_create_error = std::string("hipSetDevice: ") + hipGetErrorString(e);
        return PLK_E_DEVICE;
    }
    plk_engine *h = new plk_engine();
    h->device = device;
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) h->num_cus = cus; }
    /* ARBPLF_UP_NODES = 1: initial value of PLK_OPT_UP_NODES, so that the JSON drivers (which own their engines) can be
     * run with the node-visit up pass too: tests/test_gpu_differential.py compares the two */
    if (const char *v = getenv("ARBPLF_UP_NODES")) h->opt_up_nodes = atol(v);
    if (hipStreamCreate(&h->own_stream) != hipSuccess ||
        hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess ||
        hipEventCreate(&h->ev2) != hipSuccess || hipEventCreate(&h->ev3) != hipSuccess) {
        g_create_error = "plk_create: stream/event creation failed";
        delete h;
        return PLK_E_DEVICE;
    }
    {
        std::lock_guard<std::mutex> lk(g_live_mu);
        if (!g_atexit_set) {
            g_atexit_set = true;
            atexit([]() { std::lock_guard<std::mutex> lk2(g_live_mu); g_exiting = true; g_live.clear(); });
        }
        g_live.insert(h);
    }
    h->stream = h->own_stream;
    for (int i = 0; i < 64; i++)
        if (hipEventCreate(&h->evk[i][0]) != hipSuccess || hipEventCreate(&h->evk[i][1]) != hipSuccess) {
            g_create_error = "plk_create: event creation failed";
            plk_destroy(h);
            return PLK_E_DEVICE;
        }
    *out = h;
    return PLK_OK;
}

extern "C" void plk_destroy(plk_engine *h)
{
    if (!h) return;
    {
        std::lock_guard<std::mutex> lk(g_live_mu);
        if (g_exiting || !g_live.erase(h)) return;
    }
    (void)hipSetDevice(h->device);
    if (h->comm && g_rccl.CommDestroy) { (void)hipStreamSynchronize(h->stream); (void)g_rccl.CommDestroy(h->comm); h->comm = nullptr; }
    void *ptrs[] = {h->d_indptr, h->d_indices, h->d_preorder, h->d_Qn, h->d_edge_rates, h->d_cat_rates,
                    h->d_cat_prior, h->d_root_w, h->d_Pdd, h->d_P, h->d_dP, h->d_scratch, h->d_codes,
                    h->d_defs, h->d_B, h->d_w, h->d_ops, h->d_fops, h->d_words, h->d_mat_edge, h->d_edge_slot, h->d_op_edge, h->d_tip_edge, h->d_obs_nodes,
                    h->d_words_pt, h->d_row_nodes, h->d_tabs, h->d_quad_lut, h->d_quad_codes, h->d_llstate, h->d_v4s_rec, h->d_cstream, h->d_obs_row, h->d_PS, h->d_tip, h->d_frag, h->d_root_wd, h->d_mops, h->d_u4pack, h->d_u4tip, h->d_uvmat, h->d_stage, h->d_exL, h->d_exF, h->d_exmask, h->d_exscr, h->d_slots, h->d_site_ll, h->d_partial, h->d_work,
                    h->d_cp_fops, h->d_cp_ops, h->d_cp_mat_edge, h->d_cp_tip_edge, h->d_cp_obs_nodes, h->d_cp_op_edge, h->d_cp_expo, h->d_cp_flag,
                    h->d_cp_PS, h->d_cp_tip, h->d_cp_out, h->d_cp_partial, h->d_mixD,
                    h->d_plPdd, h->d_plP, h->d_plrates, h->d_plstream, h->d_plT, h->d_pldense, h->d_plcodes};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->ev2) (void)hipEventDestroy(h->ev2);
    if (h->ev3) (void)hipEventDestroy(h->ev3);
    if (h->cp_ev0) (void)hipEventDestroy(h->cp_ev0);
    if (h->q_ev0) (void)hipEventDestroy(h->q_ev0);
    if (h->q_ev1) (void)hipEventDestroy(h->q_ev1);
    if (h->cp_ev1) (void)hipEventDestroy(h->cp_ev1);
    for (int i = 0; i < 64; i++) for (int j = 0; j < 2; j++) if (h->evk[i][j]) (void)hipEventDestroy(h->evk[i][j]);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
}

extern "C" const char *plk_last_error(const plk_engine *h) { return plk_live(h) ? h->err.c_str() : "invalid engine handle"; }

extern "C" int plk_set_option(plk_engine *h, int option, long value)
{
    if (!plk_live(h)) return PLK_E_ARG;
    if (option == PLK_OPT_FORCE_GENERIC) { h->opt_force_generic = value; h->prog_dirty = true; return PLK_OK; }
    if (option == PLK_OPT_SITE_CHUNK) { h->opt_site_chunk = value; return PLK_OK; }
    if (option == PLK_OPT_FUSED_SITES_PER_LANE) { h->opt_fused_ns = value; h->fmt_dirty = true; return PLK_OK; }
    if (option == PLK_OPT_FUSED_ASM) { h->opt_fused_asm = value; h->fmt_dirty = true; return PLK_OK; }
    if (option == PLK_OPT_UP_NODES) { h->opt_up_nodes = value; return PLK_OK; }
    if (option == PLK_OPT_MFMA) { h->opt_mfma = value; h->fmt_dirty = true; return PLK_OK; }
    if (option == PLK_OPT_MFMA_NS2) { h->opt_mfma_ns2 = value; h->fmt_dirty = true; return PLK_OK; }
    if (option == PLK_OPT_VEC_REG_STACK) { h->opt_vec_reg_stack = value; h->fmt_dirty = true; return PLK_OK; }
    if (option == PLK_OPT_PAIR_TABLES) { h->opt_pair_tables = value; h->fmt_dirty = true; return PLK_OK; }
    if (option == PLK_OPT_STREAM_GRID) {
        if (value < 0) { h->err = "PLK_OPT_STREAM_GRID: a workgroup count, or 0 for the default"; return PLK_E_ARG; }
        h->opt_stream_grid = value; h->fmt_dirty = true; return PLK_OK;
    }
    h->err = "plk_set_option: unknown option";
    return PLK_E_ARG;
}

/* read the event pair of ring slot i (waits for it) into the running sum */
static int evk_resolve(plk_engine *h, int i)
{
    if (!h->evk_pending[i]) return PLK_OK;
    float ms = 0;
    HIPCHK(h, hipEventSynchronize(h->evk[i][1]));
    HIPCHK(h, hipEventElapsedTime(&ms, h->evk[i][0], h->evk[i][1]));
    h->evk_pending[i] = false;
    h->info_ll_kernel_ns = (long)(ms * 1e6);
    h->evk_sum_ns += h->info_ll_kernel_ns;
    h->evk_count++;
    return PLK_OK;
}

extern "C" int plk_get_info(plk_engine *h, int what, long *out)
{
    if (!plk_live(h) || !out) return PLK_E_ARG;
    if (what >= PLK_INFO_LAST_LL_KERNEL_NS && what <= PLK_INFO_LL_KERNEL_COUNT) {
        HIPCHK(h, hipSetDevice(h->device));
        int rc;
        for (int j = 0; j < 64; j++) if ((rc = evk_resolve(h, (h->evk_next + j) & 63))) return rc;     /* oldest first */
        if (h->info_pending) {
            float ms_t = 0;
            HIPCHK(h, hipEventSynchronize(h->ev3));
            HIPCHK(h, hipEventElapsedTime(&ms_t, h->ev0, h->ev3));
            h->info_ll_total_ns = (long)(ms_t * 1e6);
            h->info_pending = false;
        }
    }
    switch (what) {
    case PLK_INFO_LL_KERNEL_NS_SUM: *out = h->evk_sum_ns; h->evk_sum_ns = 0; return PLK_OK;
    case PLK_INFO_LL_KERNEL_COUNT: *out = h->evk_count; h->evk_count = 0; return PLK_OK;
    case PLK_INFO_LL_KERNEL: *out = h->info_ll_kernel; return PLK_OK;
    case PLK_INFO_UPDOWN_KERNEL: *out = h->info_updown_kernel; return PLK_OK;
    case PLK_INFO_CAT_POSTERIOR_KERNEL: *out = h->info_cat_posterior_kernel; return PLK_OK;
    case PLK_INFO_CATEGORIES: *out = h->C; return PLK_OK;
    case PLK_INFO_LAST_CAT_POSTERIOR_NS: *out = h->info_cat_posterior_ns; return PLK_OK;
    case PLK_INFO_PAIR_SUMS_KERNEL: *out = h->info_pair_sums_kernel; return PLK_OK;
    case PLK_INFO_LAST_QUERY_NS: *out = h->info_query_ns; return PLK_OK;
    case PLK_INFO_MIXTURE_SENS_KERNEL: *out = h->info_mixture_sens_kernel; return PLK_OK;
    case PLK_INFO_NNI_KERNEL: *out = h->info_nni_kernel; return PLK_OK;
    case PLK_INFO_PLACE_KERNEL: *out = h->info_place_kernel; return PLK_OK;
    case PLK_INFO_SPR_KERNEL: *out = h->info_spr_kernel; return PLK_OK;
    case PLK_INFO_UP4_PATH: *out = h->info_up4_path; return PLK_OK;
    case PLK_INFO_DOWN4_KERNEL: *out = h->info_down4_kernel; return PLK_OK;
    case PLK_INFO_LL_VARIANT: *out = h->info_ll_variant; return PLK_OK;
    case PLK_INFO_LL_FORM: *out = h->info_ll_form; return PLK_OK;
    case PLK_INFO_LL_FOLD: *out = h->info_ll_fold; return PLK_OK;
    case PLK_INFO_LL_PAIRMUL: *out = h->info_ll_pairmul; return PLK_OK;
    case PLK_INFO_LL_TRIPLE: *out = h->info_ll_triple; return PLK_OK;
    case PLK_INFO_LL_QUAD: *out = h->info_ll_quad; return PLK_OK;
    case PLK_INFO_LL_BARRIER: *out = h->info_ll_barrier; return PLK_OK;
    case PLK_INFO_LL_EXEC_FLOPS: *out = h->info_ll_exec_flops; return PLK_OK;
    case PLK_INFO_PAIR_TABLES: *out = !h->fmt_dirty && h->plan.pair_tables ? h->plan.npairs : 0; return PLK_OK;
    case PLK_INFO_STACK_SLOTS: *out = h->slots_needed; return PLK_OK;
    case PLK_INFO_PROGRAM_OPS: *out = (long)h->ops.size(); return PLK_OK;
    case PLK_INFO_LAST_LL_KERNEL_NS: *out = h->info_ll_kernel_ns; return PLK_OK;
    case PLK_INFO_LAST_LL_TOTAL_NS: *out = h->info_ll_total_ns; return PLK_OK;
    }
    h->err = "plk_get_info: unknown item";
    return PLK_E_ARG;
}

extern "C" int plk_set_tree(plk_engine *h, int N, const int *indptr, const int *indices, const int *preorder)
{
    if (!plk_live(h)) return PLK_E_ARG;
    if (N < 2 || !indptr || !indices || !preorder) { h->err = "plk_set_tree: bad arguments"; return PLK_E_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    const int E = N - 1;
    if (indptr[0] != 0 || indptr[N] != E) { h->err = "plk_set_tree: indptr does not describe N-1 edges"; return PLK_E_ARG; }
    std::vector<int> b2i(N, -1), i2a(E, -1);
    for (int a = 0; a < N; a++) {
        if (indptr[a + 1] < indptr[a]) { h->err = "plk_set_tree: indptr not monotone"; return PLK_E_ARG; }
        for (int idx = indptr[a]; idx < indptr[a + 1]; idx++) {
            int b = indices[idx];
            if (b < 0 || b >= N || b == a || b2i[b] != -1) { h->err = "plk_set_tree: not a tree"; return PLK_E_ARG; }
            b2i[b] = idx;
            i2a[idx] = a;
        }
    }
    std::vector<char> seen(N, 0);
    for (int u = 0; u < N; u++) {
        int a = preorder[u];
        if (a < 0 || a >= N || seen[a]) { h->err = "plk_set_tree: preorder is not a permutation"; return PLK_E_ARG; }
        if (u == 0 ? b2i[a] != -1 : (b2i[a] == -1 || !seen[i2a[b2i[a]]])) {
            h->err = "plk_set_tree: preorder does not start at the root / parents first";
            return PLK_E_ARG;
        }
        seen[a] = 1;
    }
    h->N = N; h->E = E;
    h->indptr.assign(indptr, indptr + N + 1);
    h->indices.assign(indices, indices + E);
    h->preorder.assign(preorder, preorder + N);
    h->b_to_idx = b2i; h->idx_to_a = i2a;
    int rc;
    if ((rc = dev_upload(h, &h->d_indptr, indptr, (size_t)N + 1))) return rc;
    if ((rc = dev_upload(h, &h->d_indices, indices, (size_t)E))) return rc;
    if ((rc = dev_upload(h, &h->d_preorder, preorder, (size_t)N))) return rc;
    h->prog_dirty = true;
    h->model_dirty = true;
    h->pat_mode = 0;
    h->k = 0;
    return PLK_OK;
}

/* The engine's arrays are in CSR order, and so is the edge that the check's line names; the drivers, which name edges in
 * the order of the user's `edges` in their own check, print the engine's line as it is, so it says which order it means. */
#define K1_CSR_NOTE " (edges numbered in CSR order)"

/* the model values of the engine with `edge_rates` against what K1 accepts (plk_k1_check.h); PLK_E_ARG and the diagnostic */
static int k1_check(plk_engine *h, const char *who, const double *edge_rates)
{
    char msg[320];
    const size_t kk = (size_t)h->k * h->k;
    if (plk_k1_check_values(h->k, h->C, h->E, h->Qn.data(), h->Qn.data() + kk, edge_rates, h->cat_rates.data(), h->cat_prior.data(),
                            h->root_mode, h->root_w.data(), msg, sizeof msg)) {
        h->err = std::string(who) + ": " + msg + K1_CSR_NOTE;
        return PLK_E_ARG;
    }
    return PLK_OK;
}

/* a direction matrix of the Frechet entry points: every entry finite */
static int k1_check_direction(plk_engine *h, const char *who, int nL, const double *L_hi, const double *L_lo)
{
    const size_t kk = (size_t)h->k * h->k;
    for (int m = 0; m < nL; m++) {
        const long bad = plk_k1_check_matrix(h->k, L_hi + m * kk, L_lo ? L_lo + m * kk : nullptr);
        if (bad) {
            h->err = std::string(who) + ": direction matrix " + std::to_string(m) + " is not finite at entry (" +
                     std::to_string((bad - 1) / h->k) + ", " + std::to_string((bad - 1) % h->k) + ")";
            return PLK_E_ARG;
        }
    }
    return PLK_OK;
}

static int run_expm(plk_engine *h, bool post = false, bool need_dP = true)
{
    const int k = h->k, C = h->C, E = h->E;
    const size_t kk = (size_t)k * k, n = (size_t)C * E * kk;
    int rc;
    /* Belt and braces: plk_set_model and plk_update_edge_rates are the only writers of h->edge_rates today (the fit and
     * Newton drivers go through the latter) and both have run this check, so it cannot fire.  It is here for a writer
     * added later: should it fire, the refused rates stay in h->edge_rates until the next plk_update_edge_rates. */
    if ((rc = k1_check(h, "K1", h->edge_rates.data()))) return rc;
    if ((rc = dev_reserve(h, &h->d_Pdd, &h->pdd_cap, n))) return rc;
    if ((rc = dev_reserve(h, &h->d_P, &h->p_cap, n))) return rc;
    if ((rc = dev_reserve(h, &h->d_dP, &h->dp_cap, n))) return rc;
    /* one thread per few matrix entries: the dd matrix products are the whole cost for k = 61 */
    const int threads = kk >= 1024 ? 1024 : (kk >= 256 ? 256 : 64);
    int use_lds;
    const size_t lds_bytes = expm_lds_bytes((size_t)k, threads, &use_lds);
    if (!use_lds) { if ((rc = dev_reserve(h, &h->d_scratch, &h->scratch_cap, (size_t)C * E * EXPM_BUFFERS * kk))) return rc; }
    ExpmPost ep = {};
    const bool pt = h->plan.pair_tables;
    post = post && k == 4 && !h->fmt_dirty && h->plan.family == LL_FUSED4 && h->d_edge_slot;
    if (post) {
        ep.edge_slot = h->d_edge_slot; ep.nmat1 = (int)h->mat_edge.size() + 1; ep.ntips1 = (int)h->tip_edge.size() + 1;
        ep.nchar = h->nchar; ep.defs = h->d_defs; ep.PS = h->d_PS; ep.tip = h->d_tip;
        if (pt) { ep.nmat1 = (int)h->fpt.mat_edge.size() + 1; ep.ntips1 = h->fpt.units; }    /* no tip slots in edge_slot: tables below */
    }
    ep.skip_dP = need_dP ? 0 : 1;
    hipLaunchKernelGGL(k_expm_dd<false>, dim3(C * E), dim3(threads), lds_bytes, h->stream,
                       k, E, h->d_Qn, h->d_edge_rates, h->d_cat_rates, h->d_Pdd, h->d_P, h->d_dP,
                       h->d_scratch, use_lds, (const double *)nullptr, 0L, 0, (const int *)nullptr, (double *)nullptr, ep);
    HIPCHK(h, hipGetLastError());
    if (post && pt) {
        const int ntab = (int)h->fpt.tab_unit.size(), ntri = h->fpt.ntriples, nquad = h->fpt.nquads;
        if (nquad > 0) {
            /* one launch for every table of the list */
            hipLaunchKernelGGL(k_build_tables_q, dim3(ntab, C), dim3(256), 0, h->stream,
                               E, ntab, ntab - ntri - nquad, ntab - nquad, h->fpt.units, h->nchar, h->d_tabs, h->d_quad_codes, h->d_Pdd, h->d_defs, h->d_tip);
        } else {
            hipLaunchKernelGGL(k_build_tables_pt, dim3(ntab - ntri, C), dim3(64), 0, h->stream,
                               E, ntab, h->fpt.units, h->nchar, h->d_tabs, h->d_Pdd, h->d_defs, h->d_tip);
            if (ntri > 0)
                hipLaunchKernelGGL(k_build_tables_t, dim3(ntri, C), dim3(64), 0, h->stream,
                                   E, ntab, ntab - ntri, h->fpt.units, h->nchar, h->d_tabs, h->d_Pdd, h->d_defs, h->d_tip);
        }
        HIPCHK(h, hipGetLastError());
    }
    h->model_dirty = false;
    h->dp_valid = need_dP;
    h->tables_dirty = !post;
    h->cp_tables_valid = false;
    return PLK_OK;
}

/* the derivative paths read dP; an ll evaluation at new rates leaves it to the first of them */
static int ensure_dP(plk_engine *h)
{
    if (h->dp_valid || h->E == 0) return PLK_OK;
    const int k = h->k;
    const size_t kk = (size_t)k * k;
    const int threads = kk >= 1024 ? 1024 : (kk >= 256 ? 256 : 64);
    int use_lds;
    const size_t strip_bytes = expm_lds_bytes((size_t)k, threads, &use_lds);
    hipLaunchKernelGGL(k_dP_dd, dim3(h->C * h->E), dim3(threads), use_lds ? 0 : strip_bytes, h->stream,
                       k, h->E, h->d_Qn, h->d_cat_rates, h->d_Pdd, h->d_dP, use_lds ? 0 : 1);
    HIPCHK(h, hipGetLastError());
    h->dp_valid = true;
    return PLK_OK;
}

extern "C" int plk_set_model(plk_engine *h, int k, int C, const double *Qn, const double *Qn_lo,
                             const double *edge_rates_csr,
                             const double *cat_rates, const double *cat_prior, int root_mode,
                             const double *root_w)
{
    if (!plk_live(h)) return PLK_E_ARG;
    if (h->N == 0) { h->err = "plk_set_model: set the tree first"; return PLK_E_ARG; }
    if (k < 1 || C < 1 || !Qn || !edge_rates_csr || !cat_rates || !cat_prior) { h->err = "plk_set_model: bad arguments"; return PLK_E_ARG; }
    if (k > PLK_MAX_K) { h->err = "plk_set_model: more than 64 states is not supported yet"; return PLK_E_UNSUPPORTED; }
    if (C > PLK_MAX_C) { h->err = "plk_set_model: more than 64 rate categories is not supported"; return PLK_E_UNSUPPORTED; }
    if (root_mode < PLK_ROOT_NONE || root_mode > PLK_ROOT_EQUILIBRIUM) { h->err = "plk_set_model: bad root mode"; return PLK_E_ARG; }
    if ((root_mode == PLK_ROOT_CUSTOM || root_mode == PLK_ROOT_EQUILIBRIUM) && !root_w) { h->err = "plk_set_model: root_w required"; return PLK_E_ARG; }
    {
        /* before anything of the engine changes: a refused model leaves the previous one in place */
        char msg[320];
        if (plk_k1_check_values(k, C, h->E, Qn, Qn_lo, edge_rates_csr, cat_rates, cat_prior, root_mode, root_w, msg, sizeof msg)) {
            h->err = std::string("plk_set_model: ") + msg + K1_CSR_NOTE;
            return PLK_E_ARG;
        }
    }
    HIPCHK(h, hipSetDevice(h->device));
    if (h->k != k) { h->pat_mode = 0; }
    h->k = k; h->C = C; h->K = pad_K(k); h->root_mode = root_mode;
    h->Qn.assign(Qn, Qn + (size_t)k * k);
    h->Qn.resize(2 * (size_t)k * k, 0.0);             /* [hi | lo] */
    if (Qn_lo) std::copy(Qn_lo, Qn_lo + (size_t)k * k, h->Qn.begin() + (size_t)k * k);
    h->edge_rates.assign(edge_rates_csr, edge_rates_csr + h->E);
    h->cat_rates.assign(cat_rates, cat_rates + C);
    h->cat_prior.assign(cat_prior, cat_prior + C);
    std::vector<double> rw(h->K, 0.0);
    for (int i = 0; i < k; i++) {
        if (root_mode == PLK_ROOT_NONE) rw[i] = 1.0;
        else if (root_mode == PLK_ROOT_UNIFORM) rw[i] = 1.0 / (double)k;
        else rw[i] = root_w[i];
    }
    h->root_w = rw;
    int rc;
    if ((rc = dev_upload(h, &h->d_Qn, h->Qn.data(), h->Qn.size()))) return rc;
    if ((rc = dev_upload(h, &h->d_edge_rates, h->edge_rates.data(), h->edge_rates.size()))) return rc;
    if ((rc = dev_upload(h, &h->d_cat_rates, h->cat_rates.data(), h->cat_rates.size()))) return rc;
    if ((rc = dev_upload(h, &h->d_cat_prior, h->cat_prior.data(), h->cat_prior.size()))) return rc;
    if ((rc = dev_upload(h, &h->d_root_w, rw.data(), rw.size()))) return rc;
    h->prog_dirty = true;
    if ((rc = run_expm(h))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PLK_OK;
}

extern "C" int plk_update_edge_rates(plk_engine *h, const double *edge_rates_csr)
{
    if (!plk_live(h) || !edge_rates_csr) return PLK_E_ARG;
    if (h->k == 0) { h->err = "plk_update_edge_rates: set the model first"; return PLK_E_ARG; }
    { int rc = k1_check(h, "plk_update_edge_rates", edge_rates_csr); if (rc) return rc; }      /* refused: the previous rates stay */
    HIPCHK(h, hipSetDevice(h->device));
    h->edge_rates.assign(edge_rates_csr, edge_rates_csr + h->E);
    HIPCHK(h, hipMemcpyAsync(h->d_edge_rates, h->edge_rates.data(), h->E * sizeof(double), hipMemcpyHostToDevice, h->stream));
    h->model_dirty = true;
    return PLK_OK;
}

/* the check of plk_set_model / plk_update_edge_rates on its own: no engine, no GPU */
extern "C" int plk_check_model_values(int k, int C, int E, const double *Qn, const double *Qn_lo, const double *edge_rates,
                                      const double *cat_rates, const double *cat_prior, int root_mode, const double *root_w)
{
    if (k > PLK_MAX_K || C > PLK_MAX_C) return PLK_E_UNSUPPORTED;
    if (root_mode < PLK_ROOT_NONE || root_mode > PLK_ROOT_EQUILIBRIUM) return PLK_E_ARG;
    if ((root_mode == PLK_ROOT_CUSTOM || root_mode == PLK_ROOT_EQUILIBRIUM) && !root_w) return PLK_E_ARG;
    return plk_k1_check_values(k, C, E, Qn, Qn_lo, edge_rates, cat_rates, cat_prior, root_mode, root_w, nullptr, 0) ? PLK_E_ARG : PLK_OK;
}

extern "C" int plk_get_transition_matrices(plk_engine *h, double *P_out)
{
    if (!plk_live(h) || !P_out) return PLK_E_ARG;
    if (h->k == 0) { h->err = "plk_get_transition_matrices: set the model first"; return PLK_E_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    if (h->model_dirty) { int rc = run_expm(h); if (rc) return rc; }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(P_out, h->d_P, (size_t)h->C * h->E * h->k * h->k * sizeof(double), hipMemcpyDeviceToHost));
    return PLK_OK;
}

static int copy_in(plk_engine *h, void *dst, const void *src, size_t bytes, int where)
{
    HIPCHK(h, hipMemcpy(dst, src, bytes, where == PLK_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    return PLK_OK;
}

extern "C" int plk_set_patterns_codes(plk_engine *h, long S, const uint8_t *codes, int where, int nchar,
                                      const double *defs)
{
    if (!plk_live(h)) return PLK_E_ARG;
    if (h->k == 0) { h->err = "plk_set_patterns_codes: set the model first"; return PLK_E_ARG; }
    if (S < 1 || !codes || nchar < 1 || nchar > 256 || !defs) { h->err = "plk_set_patterns_codes: bad arguments"; return PLK_E_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    const int k = h->k, K = h->K, N = h->N;
    const long Spad = (S + 3071) / 3072 * 3072;      /* rows padded to a whole number of 1024- and 1536-site tiles */
    int rc;
    if ((rc = dev_alloc(h, &h->d_codes, (size_t)N * Spad))) return rc;
    HIPCHK(h, hipMemset(h->d_codes, 0, (size_t)N * Spad));
    HIPCHK(h, hipMemcpy2D(h->d_codes, Spad, codes, S, S, N,
                          where == PLK_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    h->defs.assign(defs, defs + (size_t)nchar * k);
    std::vector<double> dpad((size_t)nchar * K, 0.0);
    std::vector<int> trivial(nchar, 1);                 /* bit 0: all-ones definition; bit 1: a single 1.0 among zeros */
    for (int ch = 0; ch < nchar; ch++) {
        int nnz = 0, ones = 0;
        for (int j = 0; j < k; j++) {
            const double d = defs[(size_t)ch * k + j];
            dpad[(size_t)ch * K + j] = d;
            if (d != 1.0) trivial[ch] = 0;
            if (d != 0.0) nnz++;
            if (d == 1.0) ones++;
        }
        if (nnz == 1 && ones == 1) trivial[ch] |= 2;
    }
    if ((rc = dev_upload(h, &h->d_defs, dpad.data(), dpad.size()))) return rc;
    h->S = S; h->Spad = Spad; h->nchar = nchar; h->pat_mode = 1;
    if (h->d_B) { (void)hipFree(h->d_B); h->d_B = nullptr; }
    if (h->d_w) { (void)hipFree(h->d_w); h->d_w = nullptr; }
    /* which nodes carry observations that are not all-ones */
    int *d_triv = nullptr, *d_flags = nullptr;
    if ((rc = dev_upload(h, &d_triv, trivial.data(), trivial.size()))) return rc;
    if ((rc = dev_alloc(h, &d_flags, (size_t)2 * N))) { (void)hipFree(d_triv); return rc; }      /* flags | occurring codes */
    HIPCHK(h, hipMemset(d_flags, 0, 2 * N * sizeof(int)));
    hipLaunchKernelGGL(k_node_flags, dim3((unsigned)std::min<long>(64, (S + 4095) / 4096), N), dim3(256), 0, h->stream,
                       S, Spad, h->d_codes, nchar, d_triv, d_flags, d_flags + N);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<int> flags(2 * (size_t)N);
    HIPCHK(h, hipMemcpy(flags.data(), d_flags, 2 * N * sizeof(int), hipMemcpyDeviceToHost));
    (void)hipFree(d_triv); (void)hipFree(d_flags);
    /* a property of the patterns, like node_has_data: every upload recomputes it, and prog_dirty below makes the formats stale */
    h->node_codes.clear();
    if (nchar <= 16) h->node_codes.assign(flags.begin() + N, flags.end());
    h->node_has_data.assign(N, 0);
    h->node_observed.assign(N, 0);
    for (int a = 0; a < N; a++) {
        if (flags[a] & 2) {
            h->pat_mode = 0;
            h->err = "plk_set_patterns_codes: a pattern code is not less than the number of character definitions";
            return PLK_E_ARG;
        }
        h->node_has_data[a] = (flags[a] & 3) ? 1 : 0;
        h->node_observed[a] = (flags[a] & 4) ? 0 : 1;
    }
    h->prog_dirty = true;
    return PLK_OK;
}

extern "C" int plk_set_patterns_dense(plk_engine *h, long S, const double *B, int where)
{
    if (!plk_live(h)) return PLK_E_ARG;
    if (h->k == 0) { h->err = "plk_set_patterns_dense: set the model first"; return PLK_E_ARG; }
    if (S < 1 || !B) { h->err = "plk_set_patterns_dense: bad arguments"; return PLK_E_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    const size_t n = (size_t)h->N * h->k * S;
    int rc;
    if ((rc = dev_alloc(h, &h->d_B, n))) return rc;
    if ((rc = copy_in(h, h->d_B, B, n * sizeof(double), where))) return rc;
    if (h->d_codes) { (void)hipFree(h->d_codes); h->d_codes = nullptr; }
    if (h->d_w) { (void)hipFree(h->d_w); h->d_w = nullptr; }
    h->S = S; h->Spad = S; h->pat_mode = 2; h->nchar = 0;
    h->node_has_data.assign(h->N, 1);
    h->node_observed.clear();
    h->node_codes.clear();
    h->prog_dirty = true;
    return PLK_OK;
}

extern "C" int plk_set_site_weights(plk_engine *h, const double *w, int where)
{
    if (!plk_live(h)) return PLK_E_ARG;
    if (h->pat_mode == 0) { h->err = "plk_set_site_weights: set the patterns first"; return PLK_E_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    if (!w) { if (h->d_w) { (void)hipFree(h->d_w); h->d_w = nullptr; } return PLK_OK; }
    int rc;
    if ((rc = dev_alloc(h, &h->d_w, (size_t)h->S))) return rc;
    return copy_in(h, h->d_w, w, (size_t)h->S * sizeof(double), where);
}

/* ---------------------------------------------------------------------- */
/* traversal program                                                       */
/* ---------------------------------------------------------------------- */

static int build_program(plk_engine *h)
{
    if (h->node_has_data.size() != (size_t)h->N) h->node_has_data.assign(h->N, 1);
    plk_program_build(h->N, h->indptr.data(), h->indices.data(), h->preorder.data(), h->node_has_data.data(), h->pg);
    const std::string bad = plk_program_check(h->N, h->indptr.data(), h->indices.data(), h->preorder.data(),
                                              h->node_has_data.data(), h->pg);
    if (!bad.empty()) { h->err = "internal: " + bad; return PLK_E_ARG; }
    h->prog_dirty = false;
    h->fmt_dirty = true;
    h->tables_dirty = true;
    h->cp_kind = 0;
    return PLK_OK;
}

/* register-resident vector kernel (plk_vec.h): 9 <= k <= 32 with compact codes (amino acids); PLK_OPT_MFMA = 2
 * forces the matrix-core kernel instead */
static bool use_vec(const plk_engine *h)
{
    return !h->opt_force_generic && h->opt_mfma == 1 && h->pat_mode == 1 && h->k >= 9 && h->k <= 32;
}

/* fp64 matrix-core kernel: larger state spaces with compact codes */
static bool use_mfma(const plk_engine *h)
{
    return !h->opt_force_generic && h->opt_mfma && h->pat_mode == 1 && h->k >= 9 && h->k <= 64;
}

/* dynamic LDS of k_ll_mfma / k_ll_mfma_ns2: the A fragments of one matrix + one code row of the workgroup's sites
 * (MF_SITES, or twice that with two 16-site groups per wave) per observed node */
static size_t mfma_ll_lds_bytes(const plk_engine *h, int sites)
{
    const int T = (h->k + 15) / 16, kk4 = (h->k + 3) / 4;
    return (size_t)T * kk4 * 64 * sizeof(double) + h->obs_nodes.size() * (size_t)sites;
}

/* the window of three stack slots that takes most pushes (register stack of the vector kernels) */
static int vec_reg_window(const plk_engine *h)
{
    std::vector<long> per_slot(std::max(h->slots_needed, 1), 0);
    for (const plk_op2 &o : h->ops) if ((o.x & 0xff) == OP_PUSH && o.y < (int)per_slot.size()) per_slot[o.y]++;
    long best = -1;
    int lo_best = 0;
    for (int lo = 0; lo + 3 <= std::max(h->slots_needed, 3); lo++) {
        long cnt = 0;
        for (int q = lo; q < lo + 3 && q < (int)per_slot.size(); q++) cnt += per_slot[q];
        if (cnt > best) { best = cnt; lo_best = lo; }
    }
    return lo_best;
}

/* the pair-table formats both the k = 4 and the vector kernels read: [3][rows] staged-row nodes; [6][ntab] unit, edge,
 * leaf edges of a pair, edge above the cherry and leaf edge of a three-leaf table (-1 where a row or a table has none).
 * The list names every table's first unit, so its order is free: the three-leaf tables come last, which lets
 * k_build_tables_pt build the others and k_build_tables_t these from one list. */
static int upload_pair_table_lists(plk_engine *h)
{
    const PlkFusedPT &f = h->fpt;
    int rc;
    const size_t nrows = f.row_node.size(), ntab = f.tab_unit.size();
    std::vector<int> rn(5 * nrows, -1);
    for (size_t r = 0; r < nrows; r++) {
        rn[r] = f.row_node[r]; rn[nrows + r] = f.row_node2[r];
        if (r < f.row_node3.size()) rn[2 * nrows + r] = f.row_node3[r];
        if (r < f.row_node4.size()) { rn[3 * nrows + r] = f.row_node4[r]; rn[4 * nrows + r] = f.row_lut[r]; }
    }
    if ((rc = dev_upload(h, &h->d_row_nodes, rn.data(), rn.size()))) return rc;
    auto kind = [&](size_t t) { return t < f.tab_shape.size() && f.tab_shape[t] ? 2 : t < f.tab_el.size() && f.tab_el[t] >= 0 ? 1 : 0; };
    std::vector<size_t> order;
    for (int pass = 0; pass < 3; pass++)
        for (size_t t = 0; t < ntab; t++) if (kind(t) == pass) order.push_back(t);
    std::vector<int> tabs(10 * ntab, -1);
    std::vector<int> qcodes;
    for (size_t q = 0; q < ntab; q++) {
        const size_t t = order[q];
        tabs[q] = f.tab_unit[t]; tabs[ntab + q] = f.tab_edge[t]; tabs[2 * ntab + q] = f.tab_eb[t]; tabs[3 * ntab + q] = f.tab_ec[t];
        if (t < f.tab_el.size()) { tabs[4 * ntab + q] = f.tab_ea[t]; tabs[5 * ntab + q] = f.tab_el[t]; }
        if (t < f.tab_shape.size()) { tabs[6 * ntab + q] = f.tab_shape[t]; tabs[7 * ntab + q] = f.tab_et[t]; tabs[8 * ntab + q] = f.tab_ef[t]; tabs[9 * ntab + q] = f.tab_eg[t]; }
        if (kind(t) != 2) continue;
        /* the codes behind the ranks of the table's row (the one row that reads it), in the list's order of four-leaf tables */
        const int row = t < f.tab_row.size() ? f.tab_row[t] : -1;      /* checked by plk_fused_check_v4q against the look-up that reads the table */
        if (row < 0 || (size_t)row >= nrows || f.row_lut[row] < 0 || h->node_codes.size() != (size_t)h->N) { h->err = "internal: a four-leaf table without its rank tables"; return PLK_E_ARG; }
        const int nd[4] = {f.row_node[row], f.row_node2[row], f.row_node3[row], f.row_node4[row]};
        for (int j = 0; j < 4; j++) {
            int code_of[4];
            plk_v4q_rank_codes(h->node_codes[nd[j]], code_of);
            qcodes.insert(qcodes.end(), code_of, code_of + 4);
        }
    }
    if (f.nquads > 0) {
        if ((rc = dev_upload(h, &h->d_quad_lut, f.lut.data(), f.lut.size()))) return rc;
        if ((rc = dev_upload(h, &h->d_quad_codes, qcodes.data(), qcodes.size()))) return rc;
    }
    return dev_upload(h, &h->d_tabs, tabs.data(), tabs.size());
}

/* workgroups the streamed k = 4 kernel may launch, and the CU count its plan is made for: the device's CUs, or fewer under
 * PLK_OPT_STREAM_GRID (tests: every wave then walks several units at a few thousand sites) */
static int stream_cus(const plk_engine *h) { return h->opt_stream_grid > 0 ? (int)std::min<long>(h->opt_stream_grid, h->num_cus) : h->num_cus; }

/* k = 4 with compact codes: the fused kernel plk_k4_choose picks, or PLK_K4_NONE in p.k4.variant and nothing uploaded */
static int upload_formats_fused4(plk_engine *h, LlPlan &p)
{
    int rc;
    if (!h->k4_static_lds_known) {
        /* a kernel the runtime cannot describe: the streamed form is then not chosen, a v4 tile kernel fails the query once chosen */
        const void *fns[3] = {(const void *)k_ll_fused4_v4s<768>, (const void *)k_ll_fused4_v4<768>, (const void *)k_ll_fused4_v4<512>};
        for (int i = 0; i < 3; i++) {
            hipFuncAttributes fa;
            h->k4_static_lds_err[i] = hipFuncGetAttributes(&fa, fns[i]);
            if (h->k4_static_lds_err[i] == hipSuccess) h->k4_static_lds[i] = fa.sharedSizeBytes;
            else (void)hipGetLastError();
        }
        /* the held-chunks instantiation of the streamed kernel shares the plan's table base: it runs only if it has the same static LDS */
        auto same_static_lds = [&](const void *fn) {
            hipFuncAttributes fh;
            if (hipFuncGetAttributes(&fh, fn) != hipSuccess) { (void)hipGetLastError(); return false; }
            return h->k4_static_lds_err[PLK_K4_LDS_V4S_768] == hipSuccess && fh.sharedSizeBytes == h->k4_static_lds[PLK_K4_LDS_V4S_768];
        };
        h->k4_caps.held = same_static_lds((const void *)k_ll_fused4_v4s<768, true>);
        h->k4_caps.pair = same_static_lds((const void *)k_ll_fused4_v4s<768, true, true>);
        h->k4_caps.groups = same_static_lds((const void *)k_ll_fused4_v4s<768, true, true, true>);
        h->k4_static_lds_known = true;
    }
    PlkK4Shape sh = {h->nchar, h->C, h->S, stream_cus(h), h->opt_pair_tables, h->opt_fused_asm, h->opt_fused_ns, {}};
    std::copy(h->k4_static_lds, h->k4_static_lds + 3, sh.static_lds);
    sh.node_codes = h->nchar <= 16 && h->node_codes.size() == (size_t)h->N ? h->node_codes.data() : nullptr;
    const long nunits = (h->S + PLK_V4S_UNIT - 1) / PLK_V4S_UNIT;
    PlkFusedV4S fv4s;                    /* the checked stream; the one that runs is p.k4s.fv4s */
    p.k4 = plk_k4_choose(h->N, h->indptr.data(), h->indices.data(), h->pg, sh, h->k4_static_lds_err[PLK_K4_LDS_V4S_768] == hipSuccess, h->fu, h->fpt, h->fv4, fv4s);
    if (p.k4.variant == PLK_K4_V4S && dev_reserve(h, &h->d_cstream, &h->cstream_cap, (size_t)nunits * fv4s.chunks * PLK_V4S_UNIT) != PLK_OK) {
        /* a stream that cannot be allocated sends the query to the tile kernels, it does not fail it */
        h->err.clear();
        (void)hipGetLastError();
        p.k4 = plk_k4_choose(h->N, h->indptr.data(), h->indices.data(), h->pg, sh, false, h->fu, h->fpt, h->fv4, fv4s);
    }
    const PlkK4Choice &c = p.k4;
    if (c.variant == PLK_K4_NONE) return PLK_OK;
    if (c.variant == PLK_K4_V4) HIPCHK(h, h->k4_static_lds_err[c.tile == 1536 ? PLK_K4_LDS_V4_768 : PLK_K4_LDS_V4_512]);
    if (!c.bad.empty()) { h->err = "internal: " + c.bad; return PLK_E_ARG; }
    p.family = LL_FUSED4;
    p.block = c.block; p.wg_sites = c.tile; p.lds = c.lds;
    p.info_variant = c.variant == PLK_K4_CPP ? 3 : c.variant == PLK_K4_ASM ? 1 : c.variant == PLK_K4_ASM_PT ? 5 : 6;
    p.info_form = c.variant == PLK_K4_V4S ? 1 : 0;
    if (c.variant == PLK_K4_V4S) {
        /* the formats that run, derived from the checked ones and replayed against them (plk_k4_stream: tables and category groups,
         * the folded and the pair-product stream, the barrier); the engine's part is the room for the partial sums of the groups */
        PlkK4StreamCaps caps = h->k4_caps;
        if (c.triple.nodes + c.triple.quads > 0 && c.triple.groups > 1 && plk_k4_stream_can_group(c, caps) &&
            dev_reserve(h, &h->d_llstate, &h->llstate_cap, (size_t)nunits * PLK_V4S_UNIT * 3 / 2) != PLK_OK) {
            /* no room for the partial sums: one group */
            h->err.clear();
            (void)hipGetLastError();
            caps.partial_sums = false;
        }
        p.k4s = plk_k4_stream(h->N, h->indptr.data(), h->indices.data(), h->pg, sh, c, caps, h->fpt, std::move(fv4s));
        p.lds = p.k4s.lds;
        if (!p.k4s.note.empty()) h->err = p.k4s.note;
    }
    const int ntips = (int)h->tip_edge.size();
    if (c.variant == PLK_K4_CPP || c.variant == PLK_K4_ASM) {
        /* int4 ops of the C++ interpreter, 32-bit op words of the assembly interpreter, compact matrix list */
        if ((rc = dev_upload(h, &h->d_fops, reinterpret_cast<const int4 *>(h->fu.fops.data()), h->fu.fops.size()))) return rc;
        if ((rc = dev_upload(h, &h->d_words, h->fu.words.data(), h->fu.words.size()))) return rc;
        std::vector<int> me = h->mat_edge;
        me.push_back(-1);                            /* the spare matrix is all zeros */
        if ((rc = dev_upload(h, &h->d_mat_edge, me.data(), me.size()))) return rc;
        /* where K1 itself puts P of edge e: its matrix of the stream (internal edges) or its tip slot (leaf edges) */
        std::vector<int> em(2 * (size_t)h->E, -1);
        for (size_t mi = 0; mi < h->mat_edge.size(); mi++) em[h->mat_edge[mi]] = (int)mi;
        for (int t = 0; t < ntips; t++) em[(size_t)h->E + h->tip_edge[t]] = t;
        if ((rc = dev_upload(h, &h->d_edge_slot, em.data(), em.size()))) return rc;
        if ((rc = dev_reserve(h, &h->d_PS, &h->ps_cap, (size_t)h->C * (h->mat_edge.size() + 1) * 16))) return rc;
        if ((rc = dev_reserve(h, &h->d_tip, &h->tip_cap, (size_t)h->C * (ntips + 1) * h->nchar * 4))) return rc;
        /* K1 fills the stream and the tip slots of the edges; the spare matrices stay zero and the pseudo tip slot
         * (raw definitions) is written here */
        HIPCHK(h, hipMemsetAsync(h->d_PS, 0, (size_t)h->C * (h->mat_edge.size() + 1) * 16 * sizeof(double), h->stream));
        hipLaunchKernelGGL(k_build_tip, dim3(ntips + 1, h->C), dim3(64), 0, h->stream,
                           h->E, ntips + 1, h->nchar, h->d_tip_edge, h->d_Pdd, h->d_defs, h->d_tip);
        HIPCHK(h, hipGetLastError());
        return PLK_OK;
    }
    /* pair-table interpreters: op words, staged-row nodes, table list; K1 writes the matrix stream itself, the tables
     * are built from the unrounded P after it (k_build_tables_pt) */
    const PlkFusedPT &f = h->fpt;
    p.pair_tables = true; p.npairs = f.npairs;
    const PlkFusedV4S &vs = p.k4s.fv4s;
    const std::vector<unsigned> &words = c.variant == PLK_K4_V4S ? p.k4s.words() : c.variant == PLK_K4_V4 ? h->fv4.words : f.words;
    if ((rc = dev_upload(h, &h->d_words_pt, words.data(), words.size()))) return rc;
    /* d_obs_row before the pair-table lists: the order in which these buffers were first allocated when the kernels were
     * measured (with it after them, the streamed kernel at 1.25M sites of BASELINE config 3 ran 0.3 % longer) */
    if (c.variant == PLK_K4_V4S && (rc = dev_upload(h, &h->d_obs_row, vs.obs_row.data(), vs.obs_row.size()))) return rc;
    if ((rc = upload_pair_table_lists(h))) return rc;
    if (c.variant == PLK_K4_V4S) {
        /* streamed codes: the stream itself from the resident code rows */
        const size_t total = (size_t)nunits * vs.chunks * PLK_V4S_UNIT;
        /* the kernel counts units in 32 bits (the grid of k_build_code_stream is the tighter bound: a unit has at least three chunks) */
        if (total > h->cstream_cap || (total + 255) / 256 > 0x7fffffffu || nunits > 0x7fffffff) { h->err = "internal: code stream size"; return PLK_E_ARG; }
        hipLaunchKernelGGL(k_build_code_stream, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, h->d_codes, h->Spad, nunits,
                           h->d_obs_row, vs.nobs, h->d_row_nodes, (int)f.row_node.size(), h->nchar, vs.chunks,
                           f.nquads > 0 ? h->d_quad_lut : (const uint8_t *)nullptr, h->d_cstream);
        HIPCHK(h, hipGetLastError());
    }
    std::vector<int> em(2 * (size_t)h->E, -1);
    for (size_t mi = 0; mi < f.mat_edge.size(); mi++) em[f.mat_edge[mi]] = (int)mi;
    if ((rc = dev_upload(h, &h->d_edge_slot, em.data(), em.size()))) return rc;
    if ((rc = dev_reserve(h, &h->d_PS, &h->ps_cap, (size_t)h->C * (f.mat_edge.size() + 1) * 16))) return rc;
    if ((rc = dev_reserve(h, &h->d_tip, &h->tip_cap, (size_t)h->C * f.units * h->nchar * 4))) return rc;
    HIPCHK(h, hipMemsetAsync(h->d_PS, 0, (size_t)h->C * (f.mat_edge.size() + 1) * 16 * sizeof(double), h->stream));
    if (c.variant == PLK_K4_V4S) {
        /* the records of the interpreter statement, last: they name the op words and the matrix streams where they now are, and
         * hold the root weights of the model (a model change makes the formats stale, so this runs again after it) */
        const std::vector<PlkV4SRecord> recs = plk_v4s_records(p.k4s, h->C, (unsigned)(f.units * h->nchar), (unsigned long long)(uintptr_t)h->d_words_pt,
                                                               (unsigned long long)(uintptr_t)h->d_PS, f.mat_edge.size(), h->root_w.data());
        if ((rc = dev_upload(h, &h->d_v4s_rec, recs.data(), recs.size()))) return rc;
    }
    return PLK_OK;
}

/* what the generic, vector and matrix-core kernels share: the int2 program, the edge per op, room for the matrix stream */
static int upload_formats_generic(plk_engine *h, LlPlan &p)
{
    int rc;
    const int nops = (int)h->ops.size();
    /* OP_MATVEC ops name the next OP_MATVEC (y, wrapping to the first): the vector kernel touches the
     * cache lines of the next matrix while it multiplies with the current one */
    std::vector<plk_op2> gops(h->ops);
    int first = -1, prev = -1;
    for (int pc = 0; pc < nops; pc++)
        if ((gops[pc].x & 0xff) == OP_MATVEC) {
            if (first < 0) first = pc;
            if (prev >= 0) gops[prev].y = pc;
            prev = pc;
        }
    if (prev >= 0) gops[prev].y = first;
    if ((rc = dev_upload(h, &h->d_ops, reinterpret_cast<const int2 *>(gops.data()), gops.size()))) return rc;
    if ((rc = dev_upload(h, &h->d_op_edge, h->op_edge.data(), h->op_edge.size()))) return rc;
    if ((rc = dev_reserve(h, &h->d_PS, &h->ps_cap, (size_t)h->C * std::max(nops, 1) * h->K * h->K))) return rc;
    p.family = LL_GENERIC;
    p.block = GEN_BLOCK; p.wg_sites = GEN_BLOCK;
    return PLK_OK;
}

/* 9 <= k <= 32 with compact codes: register-resident vector kernel (plk_vec.h), on pair tables where there are cherries */
static int upload_formats_vec(plk_engine *h, LlPlan &p)
{
    int rc;
    if ((rc = upload_formats_generic(h, p))) return rc;
    p.family = LL_VEC;
    p.block = VEC_BLOCK; p.wg_sites = VEC_BLOCK;
    /* register stack (PLK_OPT_VEC_REG_STACK, default on): the window of three slots that takes most pushes */
    p.vec_rs = h->opt_vec_reg_stack && h->K <= 20 && h->slots_needed >= 1;
    p.vec_reg_lo = p.vec_rs ? vec_reg_window(h) : 0;
    if (h->opt_pair_tables && h->K <= 32 && !h->obs_nodes.empty()) {
        /* pair-table program for the vector kernel: two-leaf subtrees as rows of L2-resident tables (nchar^2 rows of K
         * doubles each), as many as 64 MB of tables per category take */
        const long per_pair = (long)h->nchar * h->nchar * h->K * (long)sizeof(double);
        const int max_pairs = (int)std::min<long>(INT_MAX, (64L << 20) / std::max<long>(per_pair, 1));
        plk_fused_pt_build(h->N, h->indptr.data(), h->indices.data(), h->pg, h->nchar, max_pairs, h->fpt, false);
        if (h->fpt.npairs > 0) {
            plk_vec_pt_build(h->fpt, h->nchar, h->vpt);
            const std::string bad = plk_vec_pt_check(h->N, h->indptr.data(), h->indices.data(), h->pg, h->fpt, h->vpt, h->nchar, h->E);
            if (!bad.empty()) { h->err = "internal: " + bad; return PLK_E_ARG; }
            if ((rc = upload_pair_table_lists(h)) ||
                (rc = dev_upload(h, &h->d_mops, reinterpret_cast<const int4 *>(h->vpt.ops.data()), h->vpt.ops.size())) ||
                (rc = dev_upload(h, &h->d_op_edge, h->vpt.op_edge.data(), h->vpt.op_edge.size())) ||
                (rc = dev_reserve(h, &h->d_PS, &h->ps_cap, (size_t)h->C * h->vpt.ops.size() * h->K * h->K)) ||
                (rc = dev_reserve(h, &h->d_tip, &h->tip_cap, (size_t)h->C * h->fpt.units * h->nchar * h->K))) return rc;
            p.pair_tables = true; p.npairs = h->fpt.npairs;
            return PLK_OK;
        }
    }
    if ((rc = dev_reserve(h, &h->d_tip, &h->tip_cap, (size_t)h->C * (h->tip_edge.size() + 1) * h->nchar * h->K))) return rc;
    /* vector program: observation ops chained two ahead (value of the next op, code of the one after) */
    PlkChain ch;
    plk_chain_build(h->N, h->pg, 3, h->indices.data(), nullptr, nullptr, nullptr, ch);
    const std::string bad = plk_chain_check(h->N, h->pg, ch, 3, INT_MAX, 0, 0, 0, 0, 0);
    if (!bad.empty()) { h->err = "internal: " + bad; return PLK_E_ARG; }
    h->mfma_first_slot = ch.first_slot; h->mfma_first_row = ch.first_row; h->vec_second_row = ch.second_row;
    return dev_upload(h, &h->d_mops, reinterpret_cast<const int4 *>(ch.ops.data()), ch.ops.size());
}

/* 9 <= k <= 64 with compact codes: fp64 matrix-core kernel (plk_mfma.h) */
static int upload_formats_mfma(plk_engine *h, LlPlan &p)
{
    int rc;
    if ((rc = upload_formats_generic(h, p))) return rc;
    const int nops = (int)h->ops.size(), ntips = (int)h->tip_edge.size();
    const int T = (h->k + 15) / 16, R = 4 * T, kk4 = (h->k + 3) / 4;
    p.family = LL_MFMA;
    p.mfma_T = T;
    /* two 16-site groups per wave (PLK_OPT_MFMA_NS2) when the staged code rows of 128 sites fit the LDS */
    p.mfma_ns2 = h->opt_mfma_ns2 == 1 && T >= 3 && mfma_ll_lds_bytes(h, 2 * MF_SITES) <= PLK_LDS_LIMIT;
    p.block = MF_BLOCK; p.wg_sites = p.mfma_ns2 ? 2 * MF_SITES : MF_SITES;
    p.lds = mfma_ll_lds_bytes(h, p.wg_sites);
    std::vector<double> rwd((size_t)4 * R, 0.0);
    for (int i = 0; i < h->k; i++) rwd[(size_t)(i & 3) * R + (i >> 2)] = h->root_w[i];
    if ((rc = dev_upload(h, &h->d_root_wd, rwd.data(), rwd.size()))) return rc;
    if ((rc = dev_reserve(h, &h->d_frag, &h->frag_cap, (size_t)h->C * nops * T * kk4 * 64))) return rc;
    if ((rc = dev_reserve(h, &h->d_tip, &h->tip_cap, (size_t)h->C * (ntips + 1) * h->nchar * 4 * R))) return rc;
    /* MFMA program: observation ops name their staged code row and the next observation op */
    PlkChain ch;
    plk_chain_build(h->N, h->pg, 0, nullptr, nullptr, nullptr, nullptr, ch);
    const std::string bad = plk_chain_check(h->N, h->pg, ch, 0, INT_MAX, 0, 0, 0, MF_SITES, (size_t)h->obs_nodes.size() * MF_SITES);
    if (!bad.empty()) { h->err = "internal: " + bad; return PLK_E_ARG; }
    h->mfma_first_slot = ch.first_slot; h->mfma_first_row = ch.first_row;
    h->mfma_first_mv = -1;
    for (size_t pc = 0; pc < h->pg.ops.size() && h->mfma_first_mv < 0; pc++) if ((h->pg.ops[pc].x & 0xff) == OP_MATVEC) h->mfma_first_mv = (int)pc;
    return dev_upload(h, &h->d_mops, reinterpret_cast<const int4 *>(ch.ops.data()), ch.ops.size());
}

/* executed fp64 work per site (PLK_INFO_LL_EXEC_FLOPS): products and elementwise multiplies of the program the plan runs */
static long ll_exec_flops(const plk_engine *h, const LlPlan &p)
{
    long nprod = 0, nmul = 0;
    if (p.family == LL_VEC && p.pair_tables) {
        for (const PlkFusedPT::VOp &o : h->fpt.vops) { if (o.code == OP_MATVEC) nprod++; if (o.code == OP_TIP_MUL || o.code == OP_POPMUL) nmul++; }
    } else if (p.family == LL_FUSED4 && p.pair_tables) {
        nprod = (long)h->fpt.mat_edge.size();
        for (unsigned w : h->fpt.words) {
            const unsigned hx = w & 31;
            if (hx == OP_TIP_MUL || hx == PLK_WORD_TIPMUL_NOWAIT || hx == PLK_WORD_MATVEC_TIPMUL) nmul++;
            if ((hx >= 16 && hx < 20) || hx >= 28 || (hx >= PLK_WORD_SET_POPMUL && hx < PLK_WORD_SET_POPMUL + 4)) nmul++;
        }
    } else {
        for (const plk_op2 &o : h->ops) {
            const int code = o.x & 0xff;
            if (code == OP_MATVEC) nprod++;
            /* leaf edges: a table row multiplied in (fused, vector and matrix-core kernels) or a full product (generic) */
            if (code == OP_TIP_MUL || code == OP_NODE_MUL || code == OP_POPMUL) nmul++;
            if ((code == OP_TIP_SET || code == OP_TIP_MUL) && p.family == LL_GENERIC) { nprod++; if (code == OP_TIP_MUL) nmul++; }
        }
    }
    const long kp = p.family == LL_MFMA ? (h->k + 15) / 16 * 16 : h->k;
    return (long)h->C * (nprod * (2 * kp * kp - kp) + nmul * h->k);
}

/* The ll plan of the engine's state and the device formats it names: chosen, replayed on the host and uploaded when the
 * program or an option the plan reads changes, not per evaluation.  On an error the formats stay dirty, so the next
 * evaluation fails the same way. */
static int upload_formats(plk_engine *h)
{
    int rc;
    h->fmt_dirty = true;
    std::vector<int> te = h->tip_edge;
    te.push_back(-1);                                /* pseudo slot: the raw definitions (internal nodes with data) */
    if ((rc = dev_upload(h, &h->d_tip_edge, te.data(), te.size()))) return rc;
    if ((rc = dev_upload(h, &h->d_obs_nodes, h->obs_nodes.data(), h->obs_nodes.size()))) return rc;
    LlPlan p;
    if (!h->opt_force_generic && h->k == 4 && h->pat_mode == 1 && (rc = upload_formats_fused4(h, p))) return rc;
    if (p.family != LL_FUSED4) {
        /* trees with so many observed nodes that their staged code rows do not fit in LDS take the generic kernel */
        if (use_vec(h)) rc = upload_formats_vec(h, p);
        else if (use_mfma(h) && mfma_ll_lds_bytes(h, MF_SITES) <= PLK_LDS_LIMIT) rc = upload_formats_mfma(h, p);
        else rc = upload_formats_generic(h, p);
        if (rc) return rc;
    }
    p.info_exec_flops = ll_exec_flops(h, p);
    h->plan = std::move(p);
    h->fmt_dirty = false;
    h->tables_dirty = true;
    return PLK_OK;
}

/* P-dependent tables of the plan's kernel family, from the current P (used when K1 ran without writing them itself) */
static int build_tables(plk_engine *h)
{
    const LlPlan &p = h->plan;
    const int nops = (int)h->ops.size(), ntips = (int)h->tip_edge.size(), K = h->K, C = h->C;
    if (p.family == LL_FUSED4) return run_expm(h, true);      /* the fused formats are written by K1 itself (ExpmPost) */
    if (p.family == LL_VEC && p.pair_tables) {
        const int nv = (int)h->vpt.ops.size(), ntab = (int)h->fpt.tab_unit.size();
        hipLaunchKernelGGL(k_build_stream, dim3(nv, C), dim3(K * K >= 256 ? 256 : 64), 0, h->stream,
                           h->k, K, h->E, nv, h->d_op_edge, h->d_P, h->d_PS);
        hipLaunchKernelGGL(k_build_tables_pt_vec, dim3(ntab, C, 8), dim3(256), (size_t)4 * h->nchar * h->k * sizeof(double), h->stream,
                           h->k, K, h->E, ntab, h->fpt.units, h->nchar, h->d_tabs, h->d_Pdd, h->d_defs, h->d_tip);
        HIPCHK(h, hipGetLastError());
        h->tables_dirty = false;
        return PLK_OK;
    }
    if (nops > 0)
        hipLaunchKernelGGL(k_build_stream, dim3(nops, C), dim3(K * K >= 256 ? 256 : 64), 0, h->stream,
                           h->k, K, h->E, nops, h->d_op_edge, h->d_P, h->d_PS);
    if (p.family == LL_VEC) {
        hipLaunchKernelGGL(k_build_tip_vec, dim3(ntips + 1, C), dim3(256), 0, h->stream,
                           h->k, K, h->E, ntips, h->nchar, h->d_tip_edge, h->d_Pdd, h->d_defs, h->d_tip);
    } else if (p.family == LL_MFMA) {
        const int T = p.mfma_T, R = 4 * T, kk4 = (h->k + 3) / 4;
        hipLaunchKernelGGL(k_build_frag, dim3(nops, C), dim3(256), 0, h->stream,
                           h->k, T, kk4, h->E, nops, h->d_op_edge, h->d_P, h->d_frag);
        hipLaunchKernelGGL(k_build_tip_dist, dim3(ntips + 1, C), dim3(256), 0, h->stream,
                           h->k, R, h->E, ntips, h->nchar, h->d_tip_edge, h->d_Pdd, h->d_defs, h->K, h->d_tip);
    }
    HIPCHK(h, hipGetLastError());
    h->tables_dirty = false;
    return PLK_OK;
}

template <int D, int NS>
static void launch_fused(plk_engine *h, const FusedArgs &a, unsigned grid, size_t lds)
{
    hipLaunchKernelGGL((k_ll_fused4<D, NS>), dim3(grid), dim3(PLK_TILE), lds, h->stream, a);
}

/* the padded state counts the generic kernels are compiled for: f(std::integral_constant<int, K>) with the engine's K */
template <typename F>
static void dispatch_K(int K, F &&f)
{
    switch (K) {
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 20: f(std::integral_constant<int, 20>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    case 61: f(std::integral_constant<int, 61>{}); break;
    default: f(std::integral_constant<int, 64>{}); break;
    }
}

template <int K>
static void launch_generic(plk_engine *h, const GenArgs &a, unsigned grid)
{
    hipLaunchKernelGGL(k_ll_generic<K>, dim3(grid), dim3(GEN_BLOCK), 0, h->stream, a);
}

#define PLK_PARTIAL_OFF 72      /* d_partial: [0] the sum, [4, 68) second-stage inputs, [72, ...) one partial per workgroup */

/* room for n partial sums behind PLK_PARTIAL_OFF when the sum is wanted: where the kernel writes them, or null */
static int reserve_partials(plk_engine *h, bool want_sum, unsigned n, dd **partial)
{
    *partial = nullptr;
    if (!want_sum) return PLK_OK;
    const int rc = dev_reserve(h, &h->d_partial, &h->partial_cap, (size_t)n + PLK_PARTIAL_OFF);
    if (rc == PLK_OK) *partial = h->d_partial + PLK_PARTIAL_OFF;
    return rc;
}

/* The launch functions, one per kernel family: fill the argument struct, reserve the partial sums (*npartials of them),
 * launch on the engine's stream. */
static int launch_ll_fused4(plk_engine *h, const LlPlan &p, double *d_out, bool want_sum, unsigned *npartials)
{
    const PlkK4Choice &c = p.k4;
    const long S = h->S;
    const int ntiles = (int)((S + p.wg_sites - 1) / p.wg_sites);
    /* C++ and assembly interpreters: a workgroup per tile.  Pair-table interpreters: one workgroup per CU (two of 512
     * sites), every workgroup walks the tiles with a grid stride.  Streamed codes: 768 lanes per CU, a wave per 128-site
     * unit.  One partial sum per tile (per wave of the streamed form). */
    unsigned grid = (unsigned)ntiles;
    if (c.variant == PLK_K4_V4S) grid = (unsigned)std::min<long>(((S + PLK_V4S_UNIT - 1) / PLK_V4S_UNIT + 11) / 12, stream_cus(h));
    else if (c.variant == PLK_K4_V4 || c.variant == PLK_K4_ASM_PT) grid = (unsigned)std::min(ntiles, c.tile == 512 ? 2 * h->num_cus : h->num_cus);
    *npartials = c.variant == PLK_K4_V4S ? grid * 12 : (unsigned)ntiles;
    int rc;
    FusedArgs a;
    if ((rc = reserve_partials(h, want_sum, *npartials, &a.partial))) return rc;
    a.S = S; a.Spad = h->Spad; a.C = h->C; a.nops = (int)h->ops.size(); a.nmat = (int)h->mat_edge.size();
    a.ntips = (int)h->tip_edge.size() + 1; a.nchar = h->nchar; a.nobs = (int)h->obs_nodes.size();
    a.ops = h->d_fops; a.PS = h->d_PS; a.tip = h->d_tip;
    a.codes = h->d_codes; a.obs_nodes = h->d_obs_nodes; a.defs = h->d_defs;
    a.cat_prior = h->d_cat_prior; a.root_w = h->d_root_w; a.w = h->d_w;
    a.site_ll = d_out;
    a.root_mode = h->root_mode; a.first_row = h->fu.first_row;
    if (p.pair_tables) {
        const PlkFusedPT &f = h->fpt;
        FusedPTArgs pa;
        pa.f = a;
        pa.f.nmat = (int)f.mat_edge.size(); pa.f.ntips = f.units; pa.f.nobs = (int)f.row_node.size();
        pa.words = h->d_words_pt; pa.row_nodes = h->d_row_nodes; pa.nwords = (int)(c.variant == PLK_K4_ASM_PT ? f.words.size() : h->fv4.words.size());
        pa.first_unit = f.first_unit; pa.first_row = f.first_row; pa.second_row = f.second_row; pa.ntiles = ntiles;
        pa.warm = c.warm;
        if (c.variant == PLK_K4_V4S) {
            FusedV4SArgs sa;
            sa.pt = pa;
            const PlkK4Stream &r = p.k4s;
            const bool pairmul = r.runs == PlkK4Stream::PAIR;
            sa.pt.nwords = (int)r.stride();
            sa.stream = h->d_cstream; sa.chunks = r.fv4s.chunks;
            sa.sync = r.sync;
            h->info_ll_barrier = (sa.sync == 0 ? 1 : sa.sync == 1 ? 2 : 3) | (r.sync_auto ? 16 : 0);
            sa.groups = r.triple.groups; sa.cg = r.triple.Cg > 0 ? r.triple.Cg : h->C;
            sa.rec = h->d_v4s_rec;
            sa.part_sum = h->d_llstate;
            sa.part_exp = h->d_llstate ? reinterpret_cast<int *>(h->d_llstate + (size_t)((S + PLK_V4S_UNIT - 1) / PLK_V4S_UNIT) * PLK_V4S_UNIT) : nullptr;
            if (sa.groups > 1) {
                /* phases: only with the plan's checks behind it (pair products, room for the partial sums of every unit) */
                if (!pairmul || !h->d_llstate || h->llstate_cap < (size_t)((S + PLK_V4S_UNIT - 1) / PLK_V4S_UNIT) * PLK_V4S_UNIT * 3 / 2) { h->err = "internal: category groups without their plan"; return PLK_E_ARG; }
                hipLaunchKernelGGL((k_ll_fused4_v4s<768, true, true, true>), dim3(grid), dim3(p.block), p.lds, h->stream, sa);
            } else if (pairmul) hipLaunchKernelGGL((k_ll_fused4_v4s<768, true, true>), dim3(grid), dim3(p.block), p.lds, h->stream, sa);
            else if (r.held) hipLaunchKernelGGL((k_ll_fused4_v4s<768, true>), dim3(grid), dim3(p.block), p.lds, h->stream, sa);
            else hipLaunchKernelGGL((k_ll_fused4_v4s<768, false>), dim3(grid), dim3(p.block), p.lds, h->stream, sa);
        } else if (c.variant == PLK_K4_V4) {
            FusedV4Args va;
            va.pt = pa; va.first_y = h->fv4.first_y; va.first_z = h->fv4.first_z; va.second_z = h->fv4.second_z;
            if (c.tile == 1536) hipLaunchKernelGGL(k_ll_fused4_v4<768>, dim3(grid), dim3(p.block), p.lds, h->stream, va);
            else hipLaunchKernelGGL(k_ll_fused4_v4<512>, dim3(grid), dim3(p.block), p.lds, h->stream, va);
        } else if (c.tile == 1024) hipLaunchKernelGGL(k_ll_fused4_asm_pt<1024>, dim3(grid), dim3(p.block), p.lds, h->stream, pa);
        else hipLaunchKernelGGL(k_ll_fused4_asm_pt<512>, dim3(grid), dim3(p.block), p.lds, h->stream, pa);
        return PLK_OK;
    }
    if (c.variant == PLK_K4_ASM) {
        FusedAsmArgs aa;
        aa.f = a; aa.words = h->d_words;
        aa.first_tip = h->fu.asm_first_tip; aa.first_row = h->fu.asm_first_row; aa.second_row = h->fu.asm_second_row;
        aa.pack4 = c.pack4;
        if (c.D == 4) hipLaunchKernelGGL(k_ll_fused4_asm<4>, dim3(grid), dim3(p.block), p.lds, h->stream, aa);
        else hipLaunchKernelGGL(k_ll_fused4_asm<8>, dim3(grid), dim3(p.block), p.lds, h->stream, aa);
        return PLK_OK;
    }
    if (c.NS == 2) {
        if (c.D == 4) launch_fused<4, 2>(h, a, grid, p.lds);
        else launch_fused<8, 2>(h, a, grid, p.lds);
    } else {
        if (c.D == 4) launch_fused<4, 1>(h, a, grid, p.lds);
        else if (c.D == 8) launch_fused<8, 1>(h, a, grid, p.lds);
        else launch_fused<16, 1>(h, a, grid, p.lds);
    }
    return PLK_OK;
}

static int launch_ll_vec(plk_engine *h, const LlPlan &p, double *d_out, bool want_sum, unsigned *npartials)
{
    const long S = h->S;
    const int K = h->K;
    const unsigned grid = (unsigned)((S + p.wg_sites - 1) / p.wg_sites);
    *npartials = grid;
    int rc;
    VecArgs a;
    if ((rc = reserve_partials(h, want_sum, grid, &a.partial))) return rc;
    if ((rc = dev_reserve(h, &h->d_slots, &h->slots_cap, (size_t)std::max(h->slots_needed, 1) * K * S))) return rc;
    a.S = S; a.Spad = h->Spad; a.k = h->k; a.C = h->C; a.nops = (int)h->ops.size(); a.ntips = (int)h->tip_edge.size(); a.nchar = h->nchar;
    a.root_mode = h->root_mode; a.ops = h->d_mops; a.PS = h->d_PS; a.tip = h->d_tip; a.codes = h->d_codes;
    a.obs_nodes = h->d_obs_nodes; a.first_slot = h->mfma_first_slot; a.first_row = h->mfma_first_row; a.second_row = h->vec_second_row;
    a.obs_nodes2 = nullptr; a.units = 0;
    if (p.pair_tables) {
        const int nrows = (int)h->fpt.row_node.size();
        a.nops = (int)h->vpt.ops.size(); a.obs_nodes = h->d_row_nodes; a.obs_nodes2 = h->d_row_nodes + nrows; a.units = h->fpt.units;
        a.first_slot = 0; a.first_row = h->vpt.first_row;
    }
    a.cat_prior = h->d_cat_prior; a.root_w = h->d_root_w; a.w = h->d_w; a.slots = h->d_slots; a.site_ll = d_out;
    a.reg_lo = p.vec_reg_lo;
    if (p.vec_rs && K == 16) hipLaunchKernelGGL((k_ll_vec_rs<16, 3>), dim3(grid), dim3(p.block), 0, h->stream, a);
    else if (p.vec_rs) hipLaunchKernelGGL((k_ll_vec_rs<20, 3>), dim3(grid), dim3(p.block), 0, h->stream, a);
    else if (K == 16) hipLaunchKernelGGL(k_ll_vec<16>, dim3(grid), dim3(p.block), 0, h->stream, a);
    else if (K == 20) hipLaunchKernelGGL(k_ll_vec<20>, dim3(grid), dim3(p.block), 0, h->stream, a);
    else hipLaunchKernelGGL(k_ll_vec<32>, dim3(grid), dim3(p.block), 0, h->stream, a);
    return PLK_OK;
}

static int launch_ll_mfma(plk_engine *h, const LlPlan &p, double *d_out, bool want_sum, unsigned *npartials)
{
    const long S = h->S;
    const int T = p.mfma_T, R = 4 * T, kk4 = (h->k + 3) / 4;
    const unsigned grid = (unsigned)((S + p.wg_sites - 1) / p.wg_sites);
    *npartials = grid;
    int rc;
    MfmaArgs a;
    if ((rc = reserve_partials(h, want_sum, grid, &a.partial))) return rc;
    const long slot_stride = (long)grid * p.wg_sites * 4;
    if ((rc = dev_reserve(h, &h->d_slots, &h->slots_cap, (size_t)std::max(h->slots_needed, 1) * R * slot_stride))) return rc;
    a.S = S; a.Spad = h->Spad; a.k = h->k; a.kk4 = kk4; a.C = h->C; a.nops = (int)h->ops.size(); a.ntips = (int)h->tip_edge.size();
    a.nchar = h->nchar; a.root_mode = h->root_mode; a.ops = h->d_mops; a.frag = h->d_frag; a.tip = h->d_tip;
    a.obs_nodes = h->d_obs_nodes; a.nobs = (int)h->obs_nodes.size();
    a.first_slot = h->mfma_first_slot; a.first_row = h->mfma_first_row; a.first_mv = h->mfma_first_mv;
    a.codes = h->d_codes; a.cat_prior = h->d_cat_prior; a.root_wd = h->d_root_wd; a.w = h->d_w;
    a.slots = h->d_slots; a.slot_stride = slot_stride; a.site_ll = d_out;
    if (p.mfma_ns2 && T == 3) hipLaunchKernelGGL(k_ll_mfma_ns2<3>, dim3(grid), dim3(p.block), p.lds, h->stream, a);
    else if (p.mfma_ns2) hipLaunchKernelGGL(k_ll_mfma_ns2<4>, dim3(grid), dim3(p.block), p.lds, h->stream, a);
    else if (T == 1) hipLaunchKernelGGL(k_ll_mfma<1>, dim3(grid), dim3(p.block), p.lds, h->stream, a);
    else if (T == 2) hipLaunchKernelGGL(k_ll_mfma<2>, dim3(grid), dim3(p.block), p.lds, h->stream, a);
    else if (T == 3) hipLaunchKernelGGL(k_ll_mfma_occ4<3>, dim3(grid), dim3(p.block), p.lds, h->stream, a);
    else hipLaunchKernelGGL(k_ll_mfma_occ4<4>, dim3(grid), dim3(p.block), p.lds, h->stream, a);
    return PLK_OK;
}

static int launch_ll_generic(plk_engine *h, const LlPlan &p, double *d_out, bool want_sum, unsigned *npartials)
{
    const long S = h->S;
    const unsigned grid = (unsigned)((S + p.wg_sites - 1) / p.wg_sites);
    *npartials = grid;
    int rc;
    GenArgs a;
    if ((rc = reserve_partials(h, want_sum, grid, &a.partial))) return rc;
    if ((rc = dev_reserve(h, &h->d_slots, &h->slots_cap, (size_t)std::max(h->slots_needed, 1) * h->k * S))) return rc;
    a.S = S; a.Spad = h->Spad; a.k = h->k; a.C = h->C; a.nops = (int)h->ops.size(); a.nchar = h->nchar;
    a.pat_mode = h->pat_mode; a.root_mode = h->root_mode; a.ops = h->d_ops; a.PS = h->d_PS;
    a.codes = h->d_codes; a.defs = h->d_defs; a.B = h->d_B; a.cat_prior = h->d_cat_prior;
    a.root_w = h->d_root_w; a.w = h->d_w; a.slots = h->d_slots; a.site_ll = d_out;
    dispatch_K(h->K, [&](auto Kc) { launch_generic<decltype(Kc)::value>(h, a, grid); });
    return PLK_OK;
}

/* sum_dev != null: the {hi, lo} sum is left in device memory (2 doubles) and nothing is copied or waited for */
static int ll_impl(plk_engine *h, double *site_ll_out, int where, double *sum_out, double *sum_dev, bool async)
{
    if (h->k == 0 || h->pat_mode == 0) { h->err = "plk_ll: tree, model and patterns must be set"; return PLK_E_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    /* the plan with its formats, K1, the P-dependent tables */
    if (h->prog_dirty) { if ((rc = build_program(h))) return rc; }
    if (h->fmt_dirty) { if ((rc = upload_formats(h))) return rc; }
    if (h->model_dirty) { if ((rc = run_expm(h, true, false))) return rc; }      /* K1 without dP; for k = 4 it writes the stream and tip tables too */
    if (h->tables_dirty) { if ((rc = build_tables(h))) return rc; }
    const LlPlan &p = h->plan;
    const bool want_sum = sum_out || sum_dev;
    const long S = h->S;
    double *d_out = nullptr;
    if (site_ll_out) {
        if (where == PLK_DEVICE) d_out = site_ll_out;
        else { if ((rc = dev_reserve(h, &h->d_site_ll, &h->site_ll_cap, (size_t)S))) return rc; d_out = h->d_site_ll; }
    }
    const int evi = h->evk_next;
    h->evk_next = (evi + 1) & 63;
    if ((rc = evk_resolve(h, evi))) return rc;           /* only waits when 64 evaluations are queued */
    HIPCHK(h, hipEventRecord(h->evk[evi][0], h->stream));
    unsigned npartials = 0;
    h->info_ll_barrier = 0;                              /* the streamed launch sets it */
    switch (p.family) {
    case LL_FUSED4: rc = launch_ll_fused4(h, p, d_out, want_sum, &npartials); break;
    case LL_VEC: rc = launch_ll_vec(h, p, d_out, want_sum, &npartials); break;
    case LL_MFMA: rc = launch_ll_mfma(h, p, d_out, want_sum, &npartials); break;
    default: rc = launch_ll_generic(h, p, d_out, want_sum, &npartials); break;
    }
    if (rc) return rc;
    h->info_ll_kernel = p.family; h->info_ll_variant = p.info_variant; h->info_ll_form = p.info_form; h->info_ll_fold = p.k4s.info_fold; h->info_ll_pairmul = p.k4s.info_pairmul; h->info_ll_triple = p.k4s.info_triple; h->info_ll_quad = p.k4s.info_quad; h->info_ll_exec_flops = p.info_exec_flops;
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->evk[evi][1], h->stream));
    h->evk_pending[evi] = true;
    if (want_sum) {
        /* fixed-order double-double sum of the partials: up to 64 slices, then one small block */
        dd *out = sum_dev ? reinterpret_cast<dd *>(sum_dev) : h->d_partial;
        const int g2 = npartials > 1024 ? (int)std::min<unsigned>(64u, (npartials + 511) / 512) : 1;
        if (g2 > 1) {
            hipLaunchKernelGGL(k_dd_slices, dim3(g2), dim3(256), 0, h->stream, (int)npartials, h->d_partial + PLK_PARTIAL_OFF, h->d_partial + 4);
            hipLaunchKernelGGL(k_dd_final, dim3(1), dim3(64), 0, h->stream, g2, h->d_partial + 4, out);
        } else {
            hipLaunchKernelGGL(k_dd_final, dim3(1), dim3(256), 0, h->stream, (int)npartials, h->d_partial + PLK_PARTIAL_OFF, out);
        }
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipEventRecord(h->ev3, h->stream));
    h->info_pending = true;
    if (async) return PLK_OK;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (sum_out) {
        dd r;
        HIPCHK(h, hipMemcpy(&r, h->d_partial, sizeof(dd), hipMemcpyDeviceToHost));
        sum_out[0] = r.hi; sum_out[1] = r.lo;
    }
    if (site_ll_out && where != PLK_DEVICE)
        HIPCHK(h, hipMemcpy(site_ll_out, h->d_site_ll, (size_t)S * sizeof(double), hipMemcpyDeviceToHost));
    return PLK_OK;
}

extern "C" int plk_ll(plk_engine *h, double *site_ll_out, int where, double *sum_out)
{
    if (!plk_live(h)) return PLK_E_ARG;
    return ll_impl(h, site_ll_out, where, sum_out, nullptr, false);
}

/* The same evaluation queued on the engine's stream without waiting: per-site values (optional) and the {hi, lo} sum
 * (optional) are left in DEVICE memory the caller owns.  plk_sync() or any synchronous call waits for it. */
extern "C" int plk_ll_async(plk_engine *h, double *site_ll_dev, double *sum_dev)
{
    if (!plk_live(h)) return PLK_E_ARG;
    return ll_impl(h, site_ll_dev, PLK_DEVICE, nullptr, sum_dev, true);
}

extern "C" int plk_sync(plk_engine *h)
{
    if (!plk_live(h)) return PLK_E_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PLK_OK;
}

/* Run the engine's work on a stream of the caller (e.g. the framework's current stream, so that its collectives and
 * events are ordered with the engine's kernels); NULL returns to the engine's own stream. */
extern "C" int plk_set_stream(plk_engine *h, void *hip_stream)
{
    if (!plk_live(h)) return PLK_E_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    return PLK_OK;
}

template <int K>
static void launch_updown(plk_engine *h, const UpArgs &a, unsigned grid, bool deriv, bool marg)
{
    hipLaunchKernelGGL(k_down_store<K>, dim3(grid), dim3(GEN_BLOCK), 0, h->stream, a);
    if (deriv && marg) hipLaunchKernelGGL((k_up<K, true, true>), dim3(grid), dim3(GEN_BLOCK), 0, h->stream, a);
    else if (deriv) hipLaunchKernelGGL((k_up<K, true, false>), dim3(grid), dim3(GEN_BLOCK), 0, h->stream, a);
    else hipLaunchKernelGGL((k_up<K, false, true>), dim3(grid), dim3(GEN_BLOCK), 0, h->stream, a);
}

/* generic down pass + the outer-product up pass on its fixed grid (plk_pairsums.h) */
template <int K>
static void launch_pairsums(plk_engine *h, const UpArgs &a, const PairSumOut &o, unsigned grid, unsigned pgrid)
{
    hipLaunchKernelGGL(k_down_store<K>, dim3(grid), dim3(GEN_BLOCK), 0, h->stream, a);
    hipLaunchKernelGGL(k_up_pairsums<K>, dim3(pgrid), dim3(GEN_BLOCK), 0, h->stream, a, o, (int)grid);
}

/* generic down pass (with the first group of swaps of a chunk) + the swap up pass on the chunk's grid (plk_nni.h) */
template <int K>
static void launch_nni(plk_engine *h, const UpArgs &a, const NniOut &o, unsigned grid, bool down)
{
    if (down) {
        hipLaunchKernelGGL(k_down_store<K>, dim3(grid), dim3(GEN_BLOCK), 0, h->stream, a);
        hipLaunchKernelGGL((k_up_nni<K, true>), dim3(grid), dim3(GEN_BLOCK), 0, h->stream, a, o);
    }
    hipLaunchKernelGGL((k_up_nni<K, false>), dim3(grid), dim3(GEN_BLOCK), 0, h->stream, a, o);
}

/* ... the same for the placement pass (plk_place.h): the forward vectors are those of the swap pass */
template <int K>
static void launch_place(plk_engine *h, const UpArgs &a, const PlaceOut &o, unsigned grid, bool down)
{
    if (down) {
        NniOut none = {};
        hipLaunchKernelGGL(k_down_store<K>, dim3(grid), dim3(GEN_BLOCK), 0, h->stream, a);
        hipLaunchKernelGGL((k_up_nni<K, true>), dim3(grid), dim3(GEN_BLOCK), 0, h->stream, a, none);
    }
    hipLaunchKernelGGL(k_up_place<K>, dim3(grid), dim3(GEN_BLOCK), 0, h->stream, a, o);
}

/* the prune-and-regraft pass (plk_spr.h): the down pass once per chunk, the path plane and F' once per prune edge */
template <int K>
static void launch_spr(plk_engine *h, const UpArgs &a, const SprOut &o, unsigned grid, bool down)
{
    if (down) hipLaunchKernelGGL(k_down_store<K>, dim3(grid), dim3(GEN_BLOCK), 0, h->stream, a);
    if (o.store_fn) hipLaunchKernelGGL((k_up_spr<K, true>), dim3(grid), dim3(GEN_BLOCK), 0, h->stream, a, o);
    hipLaunchKernelGGL((k_up_spr<K, false>), dim3(grid), dim3(GEN_BLOCK), 0, h->stream, a, o);
}

/* ... and the mixture-gradient up pass on the same grid (plk_mixsens.h) */
template <int K>
static void launch_mixsens(plk_engine *h, const UpArgs &a, const MixSensOut &o, unsigned grid, unsigned pgrid)
{
    hipLaunchKernelGGL(k_down_store<K>, dim3(grid), dim3(GEN_BLOCK), 0, h->stream, a);
    hipLaunchKernelGGL(k_up_mixsens<K>, dim3(pgrid), dim3(GEN_BLOCK), 0, h->stream, a, o, (int)grid);
}

/* rows x n weighted sums of X (row stride n) accumulated into acc[rows] (long double pairs) */
static int wsum_rows(plk_engine *h, int rows, long n, const double *X, const double *w, long double *acc)
{
    int rc;
    const int nblocks = (int)std::min<long>(256, (n + 2047) / 2048);
    if ((rc = dev_reserve(h, &h->d_partial, &h->partial_cap, (size_t)rows * nblocks + rows + 8))) return rc;
    dd *outp = h->d_partial;
    dd *part = h->d_partial + rows + 8;
    hipLaunchKernelGGL(k_wsum_rows, dim3(nblocks, rows), dim3(256), 0, h->stream, n, n, X, w, nblocks, part);
    hipLaunchKernelGGL(k_dd_final, dim3(rows), dim3(64), 0, h->stream, nblocks, part, outp);
    HIPCHK(h, hipGetLastError());
    std::vector<dd> host(rows);
    HIPCHK(h, hipMemcpyAsync(host.data(), outp, rows * sizeof(dd), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int r = 0; r < rows; r++) acc[r] += (long double)host[r].hi + (long double)host[r].lo;
    return PLK_OK;
}

/* per-site outputs leave the kernels as [row][site] planes (site fastest: coalesced stores); callers want
 * [site][row].  Transposed on the device through LDS tiles, then one contiguous copy to the host. */
__global__ __launch_bounds__(256) void k_transpose_rows(long rows, long n, const double *__restrict__ src, double *__restrict__ dst)
{
    __shared__ double tile[32][33];
    const long r0 = (long)blockIdx.y * 32, s0 = (long)blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int j = ty; j < 32; j += 8)
        if (r0 + j < rows && s0 + tx < n) tile[j][tx] = src[(size_t)(r0 + j) * n + s0 + tx];
    __syncthreads();
    for (int j = ty; j < 32; j += 8)
        if (s0 + j < n && r0 + tx < rows) dst[(size_t)(s0 + j) * rows + r0 + tx] = tile[tx][j];
}

static int copy_site_rows(plk_engine *h, size_t rows, long n, long s0, const double *d_src, double *site_out)
{
    if (rows == 0 || n == 0) return PLK_OK;
    int rc;
    if ((rc = dev_reserve(h, &h->d_stage, &h->stage_cap, rows * (size_t)n))) return rc;
    hipLaunchKernelGGL(k_transpose_rows, dim3((unsigned)((n + 31) / 32), (unsigned)((rows + 31) / 32)), dim3(256), 0, h->stream,
                       (long)rows, n, d_src, h->d_stage);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(site_out + (size_t)s0 * rows, h->d_stage, rows * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PLK_OK;
}

/* ---------------------------------------------------------------------- */
/* what the down / up drivers share: storage maps, the call's integer      */
/* tables, the site-chunk plan and the output epilogue                     */
/* ---------------------------------------------------------------------- */

/* storage indices of the current program (plk_program.h); build_program() has run */
static PlkStorageMaps storage_maps(const plk_engine *h)
{
    PlkStorageMaps m;
    plk_storage_maps_build(h->N, h->E, h->indptr.data(), h->tip_edge, h->scale_node.data(), m);
    return m;
}

/* node_has_data as the kernels read it: one int per node (all ones until patterns say otherwise) */
static std::vector<int> has_data_ints(plk_engine *h)
{
    if (h->node_has_data.size() != (size_t)h->N) h->node_has_data.assign(h->N, 1);
    return std::vector<int>(h->node_has_data.begin(), h->node_has_data.end());
}

/* The integer tables of one call, gathered into one host block that goes to the grow-only d_u4pack in one copy.  put()
 * returns the table's offset in the block; every table starts at a multiple of 4 ints (the op tables are read as int4). */
struct IntPack {
    std::vector<int> words;
    size_t put(const int *src, size_t n)
    {
        const size_t off = words.size();
        words.insert(words.end(), src, src + n);
        while (words.size() % 4) words.push_back(0);
        return off;
    }
    size_t put_opt(const int *src, size_t n) { return src ? put(src, n) : 0; }     /* an optional mask */
    size_t put_has_data(plk_engine *h) { const std::vector<int> hd = has_data_ints(h); return put(hd.data(), hd.size()); }
    /* four spare words follow the tables; the pair-sum passes keep their flag in the first one (flag()) */
    int upload(plk_engine *h)
    {
        int rc;
        if ((rc = dev_reserve(h, &h->d_u4pack, &h->u4pack_cap, words.size() + 4))) return rc;
        HIPCHK(h, hipMemcpyAsync(h->d_u4pack, words.data(), words.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));      /* the block is a local of the caller */
        return PLK_OK;
    }
    int *flag(const plk_engine *h) const { return h->d_u4pack + words.size(); }
};

/* sites per pass of a down / up driver (plk_site_chunk in plk_program.h), or PLK_E_NOMEM in the name of the query */
static int plan_site_chunk(plk_engine *h, const char *who, size_t bytes_per_site, int tile, bool whole_tiles, long *chunk)
{
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    *chunk = plk_site_chunk(h->S, free_b, h->work_cap * sizeof(double), bytes_per_site, h->opt_site_chunk, tile, whole_tiles);
    if (*chunk > 0) return PLK_OK;
    h->err = std::string(who) + (whole_tiles ? ": not enough device memory" : ": not enough device memory for one site");
    return PLK_E_NOMEM;
}

/* site-summed marginals without per-site output: the up passes of the specialised drivers leave one weighted sum per
 * wave, node and state (MVS) instead of the N k planes */
static bool marginal_sums_only(bool deriv, bool marg, const double *site_out, const double *sums_out)
{
    return marg && !site_out && sums_out && !deriv;
}

/* the outputs of one site chunk: edge rows DV (drows of them, 0 unless a derivative was asked for) and marginal rows MV
 * (mrows), or per-wave marginal sums MVS ([mrows][nwv]) in place of MV */
struct UpDownOut {
    size_t drows = 0, mrows = 0, nwv = 0;
    const double *DV = nullptr, *MV = nullptr;
    const double *MVS = nullptr;       /* null unless the pass left per-wave sums in place of MV (marginal_sums_only) */
};

/* per-chunk epilogue: weighted row sums into dsum / msum (when sums are wanted), per-site rows to the host */
static int updown_chunk_out(plk_engine *h, const UpDownOut &o, long n, long s0, bool want_sums, long double *dsum, long double *msum,
                            double *site_out)
{
    int rc;
    if (want_sums) {
        const double *w = h->d_w ? h->d_w + s0 : nullptr;
        if (o.drows && (rc = wsum_rows(h, (int)o.drows, n, o.DV, w, dsum))) return rc;
        if (o.mrows && o.MVS) { if ((rc = wsum_rows(h, (int)o.mrows, (long)o.nwv, o.MVS, nullptr, msum))) return rc; }
        else if (o.mrows && (rc = wsum_rows(h, (int)o.mrows, n, o.MV, w, msum))) return rc;
    }
    if (site_out) return copy_site_rows(h, o.drows ? o.drows : o.mrows, n, s0, o.drows ? o.DV : o.MV, site_out);
    return PLK_OK;
}

static inline void put_dd(double *dst, long double v)
{
    const double hi = (double)v;
    dst[0] = hi;
    dst[1] = (double)(v - (long double)hi);
}

/* the final split of n accumulated sums into {hi, lo} pairs */
static void put_dd_rows(double *dst, const long double *src, size_t n)
{
    for (size_t r = 0; r < n; r++) put_dd(dst + 2 * r, src[r]);
}

/* end of a deriv / marginal query: wait for the stream, then hand out the sums (when asked for) */
static int updown_finish(plk_engine *h, double *sums_out, const std::vector<long double> &sums)
{
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { h->err = std::string("plk_deriv/plk_marginal: ") + hipGetErrorString(e); return PLK_E_DEVICE; }
    if (sums_out) put_dd_rows(sums_out, sums.data(), sums.size());
    return PLK_OK;
}

template <int K>
static void launch_range_check(plk_engine *h, const GenArgs &a, unsigned grid, const int *op_edge, const int *op_mid, int *flag)
{
    hipLaunchKernelGGL(k_range_check<K>, dim3(grid), dim3(GEN_BLOCK), 0, h->stream, a, h->E, op_edge, op_mid, flag);
}

/*
 * The passes that store node vectors (derivatives, marginals, edge expectations, pair sums, mixture gradients, second
 * order) keep ONE power-of-two factor per node (SC) and multiply all of a node's children before they look at the
 * magnitude; the program's OP_SCALE ops inside a node are not taken there (plk_chain_build).  On a tree that has such a
 * node (PlkProgram::mid_scales, e.g. a root over three deep subtrees, or 33 leaf children) the products are measured
 * first (k_range_check, one extra traversal without output): with ordinary branch lengths they stay far inside the
 * double range and the query runs as on any tree; where one falls below 2^-969 the query is refused, not miscomputed.
 * Trees without such a node -- every tree whose nodes have at most two children -- pay nothing.  P is current here.
 */
static int check_stored_range(plk_engine *h, const char *who)
{
    int rc;
    if (h->prog_dirty && (rc = build_program(h))) return rc;
    const PlkProgram &pg = h->pg;
    if (pg.mid_scales == 0 || pg.ops.empty()) return PLK_OK;
    const int k = h->k, K = h->K, C = h->C, E = h->E;
    const long S = h->S;
    const size_t strm = ((size_t)C * E * K * K + 31) / 32 * 32;
    if ((rc = dev_reserve(h, &h->d_uvmat, &h->uvmat_cap, strm))) return rc;
    if ((rc = dev_reserve(h, &h->d_slots, &h->slots_cap, (size_t)std::max(pg.slots_needed, 1) * k * S))) return rc;
    hipLaunchKernelGGL(k_build_edge_stream, dim3(C * E), dim3(K * K >= 256 ? 256 : 64), 0, h->stream, k, K, 0, h->d_P, h->d_uvmat);
    IntPack pack;
    std::vector<int> mid(pg.op_mid.begin(), pg.op_mid.end()), edge(pg.op_edge);
    for (int &e : edge) if (e < 0) e = 0;                   /* ops without an edge read no matrix */
    const size_t o_ops = pack.put(reinterpret_cast<const int *>(pg.ops.data()), 2 * pg.ops.size());
    const size_t o_edge = pack.put(edge.data(), edge.size()), o_mid = pack.put(mid.data(), mid.size());
    if ((rc = pack.upload(h))) return rc;
    int *d_flag = pack.flag(h);
    HIPCHK(h, hipMemsetAsync(d_flag, 0, sizeof(int), h->stream));
    GenArgs a = {};
    a.S = S; a.Spad = h->Spad; a.k = k; a.C = C; a.nops = (int)pg.ops.size(); a.nchar = h->nchar;
    a.pat_mode = h->pat_mode; a.root_mode = h->root_mode; a.ops = reinterpret_cast<const int2 *>(h->d_u4pack + o_ops); a.PS = h->d_uvmat;
    a.codes = h->d_codes; a.defs = h->d_defs; a.B = h->d_B; a.slots = h->d_slots;
    const unsigned grid = (unsigned)((S + GEN_BLOCK - 1) / GEN_BLOCK);
    dispatch_K(K, [&](auto Kc) { launch_range_check<decltype(Kc)::value>(h, a, grid, h->d_u4pack + o_edge, h->d_u4pack + o_mid, d_flag); });
    HIPCHK(h, hipGetLastError());
    int low = 0;
    HIPCHK(h, hipMemcpyAsync(&low, d_flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (!low) return PLK_OK;
    const int nd = pg.wide_node;
    h->err = std::string(who) + ": the product of the children of a node leaves the double range (largest entry below 2^-969 at some site; "
             "node " + std::to_string(nd) + " with " + std::to_string(h->indptr[nd + 1] - h->indptr[nd]) + " children is the first that takes more than " +
             std::to_string(PLK_SCALE_RUN) + " edge factors at once): this query keeps one rescaling factor per node and refuses such data "
             "(the log likelihood and category posterior queries rescale inside the node and answer)";
    return PLK_E_ARG;
}

template <int T>
static void launch_updown_mfma(plk_engine *h, const MUpArgs &a, const MDownProg &pg, unsigned grid, size_t lds, bool deriv, bool marg, bool nodes)
{
    const size_t lds_down = lds + (size_t)pg.nobs * MF_SITES;
    if (nodes)          /* the caller has checked that the depth-first down pass fits */
        hipLaunchKernelGGL((k_down_fused_mfma<T, false>), dim3(grid), dim3(MF_BLOCK), lds_down, h->stream, a, pg);
    else if (lds_down <= 60 * 1024 && (a.s0 % MF_SITES) == 0)
        hipLaunchKernelGGL((k_down_fused_mfma<T, true>), dim3(grid), dim3(MF_BLOCK), lds_down, h->stream, a, pg);
    else
        hipLaunchKernelGGL(k_down_store_mfma<T>, dim3(grid), dim3(MF_BLOCK), lds, h->stream, a);
    if (nodes) hipLaunchKernelGGL(k_up_nodes_mfma<T>, dim3(grid), dim3(MF_BLOCK), lds, h->stream, a);
    else if (deriv && marg) hipLaunchKernelGGL((k_up_mfma<T, true, true>), dim3(grid), dim3(MF_BLOCK), lds, h->stream, a);
    else if (deriv) hipLaunchKernelGGL((k_up_mfma<T, true, false>), dim3(grid), dim3(MF_BLOCK), lds, h->stream, a);
    else hipLaunchKernelGGL((k_up_mfma<T, false, true>), dim3(grid), dim3(MF_BLOCK), lds, h->stream, a);
}

/* deriv / marginal for 9 <= k <= 64 with compact codes: matrix-core kernels (plk_mfma_updown.h) */
static int run_updown_mfma(plk_engine *h, bool deriv, bool marg, const int *edge_mask, const int *node_mask,
                           double *site_out, double *sums_out, const double *d_M, int dzero)
{
    int rc;
    const int N = h->N, E = h->E, k = h->k, C = h->C;
    const int T = (k + 15) / 16, R = 4 * T, kk4 = (k + 3) / 4;
    const long S = h->S;
    if (h->prog_dirty) { if ((rc = build_program(h))) return rc; }
    const PlkStorageMaps sm = storage_maps(h);
    const std::vector<int> &edge_tip = sm.edge_tip, &edge_int = sm.edge_int, &node_int = sm.node_int, &node_scale = sm.node_scale;
    const int ntips = sm.ntips, nie = sm.nie, nin = sm.nin, nsc = sm.nsc;
    std::vector<double> rwd((size_t)4 * R, 0.0);
    for (int i = 0; i < k; i++) rwd[(size_t)(i & 3) * R + (i >> 2)] = h->root_w[i];

    /* derivative queries without marginals on the edge-at-a-time up pass: nodes whose children are all leaves are finished
     * inside their parent's visit (their F never goes through HBM), and the up pass rebuilds their L from the tip tables,
     * so the down pass does not store it either */
    const bool nodes_wanted = deriv && !marg && (h->opt_up_nodes & 1);
    std::vector<int> node_inl(N, 0);
    std::vector<char> skip_l(N, 0);
    bool any_inl = false;
    if (deriv && !marg && !nodes_wanted)
        for (int u = 1; u < N; u++) {
            const int b = h->preorder[u];
            if (plk_up_inlinable(h->indptr.data(), edge_tip.data(), b, false)) { node_inl[b] = 1; skip_l[b] = 1; any_inl = true; }
        }
    /* program of the depth-first down pass (k_down_fused_mfma) */
    PlkChain dch;
    plk_chain_build(N, h->pg, 2, h->indices.data(), node_int.data(), edge_int.data(), node_scale.data(), dch, any_inl ? skip_l.data() : nullptr);
    {
        const std::string bad = plk_chain_check(N, h->pg, dch, 2, INT_MAX, nin, nie, nsc, MF_SITES, (size_t)h->obs_nodes.size() * MF_SITES);
        if (!bad.empty()) { h->err = "internal: " + bad; return PLK_E_ARG; }
    }
    const std::vector<plk_op4> &dops = dch.ops;
    const int nslots_m = std::max(h->slots_needed, 1);
    if (h->node_has_data.size() != (size_t)N) h->node_has_data.assign(N, 1);
    /* PLK_OPT_UP_NODES = 1: derivative queries without marginals take the node-visit up pass over edge vectors only
     * (k_up_nodes_mfma), when the depth-first down pass applies (its staged code rows fit the LDS).  Measured equal to
     * k_up_mfma at BASELINE config 5 (32.1 against 31.7 ms per step: the down pass gains what the up pass loses), so
     * not the default; DESIGN.md section 4 has the counters */
    const bool nodes = deriv && !marg && (h->opt_up_nodes & 1) &&
                       (size_t)T * kk4 * 64 * sizeof(double) + h->obs_nodes.size() * (size_t)MF_SITES <= 60 * 1024;
    PlkUpNodes un;
    if (nodes) {
        plk_up_nodes_build(N, h->indptr.data(), h->indices.data(), h->preorder.data(), h->node_has_data.data(), edge_tip.data(),
                           node_int.data(), node_scale.data(), edge_mask, un);
        const std::string bad = plk_up_nodes_check(N, E, h->indptr.data(), h->indices.data(), un, nin, ntips, nsc);
        if (!bad.empty()) { h->err = "internal: " + bad; return PLK_E_ARG; }
    }
    /* the call's integer tables, one upload: [ops (16-byte aligned first)][edge_tip][edge_int][node_int][tip edges][node_scale]
     * [obs nodes][has_data][edge mask][node mask] */
    IntPack pack;
    const size_t o_ops = pack.put(reinterpret_cast<const int *>(dops.data()), dops.size() * 4);
    const size_t o_et = pack.put(edge_tip.data(), (size_t)E), o_ei = pack.put(edge_int.data(), (size_t)E), o_ni = pack.put(node_int.data(), (size_t)N);
    const size_t o_te = pack.put(sm.tip_edges.data(), sm.tip_edges.size()), o_ns = pack.put(node_scale.data(), (size_t)N);
    const size_t o_obs = pack.put(h->obs_nodes.data(), h->obs_nodes.size());
    const size_t o_has = pack.put_has_data(h);
    const size_t o_em = pack.put_opt(edge_mask, (size_t)E), o_nm = pack.put_opt(node_mask, (size_t)N);
    const size_t o_vis = nodes ? pack.put(un.rec.data(), un.rec.size()) : 0;
    const size_t o_inl = any_inl ? pack.put(node_inl.data(), (size_t)N) : 0;
    const size_t nfr = (size_t)C * E * T * kk4 * 64, ntab = (size_t)C * (ntips + 1) * h->nchar * 4 * R;
    if ((rc = dev_reserve(h, &h->d_u4tip, &h->u4tip_cap, 2 * ntab + rwd.size())) ||
        (rc = dev_reserve(h, &h->d_uvmat, &h->uvmat_cap, 3 * nfr))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_u4tip + 2 * ntab, rwd.data(), rwd.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if ((rc = pack.upload(h))) return rc;            /* its wait covers rwd, a local too */
    const int *pk = h->d_u4pack;
    const int4 *d_dops = reinterpret_cast<const int4 *>(pk + o_ops);
    const int *d_et = pk + o_et, *d_ei = pk + o_ei, *d_ni = pk + o_ni, *d_te = pk + o_te, *d_ns = pk + o_ns, *d_obsm = pk + o_obs, *d_has = pk + o_has;
    const int *d_emask = edge_mask ? pk + o_em : nullptr, *d_nmask = node_mask ? pk + o_nm : nullptr;
    double *d_fP = h->d_uvmat, *d_fPT = d_fP + nfr, *d_fD = d_fPT + nfr;
    double *d_tipd = h->d_u4tip, *d_dtip = d_tipd + ntab, *d_rwd = d_dtip + ntab;
    hipLaunchKernelGGL(k_build_frag_edges, dim3(C * E), dim3(256), 0, h->stream, k, T, kk4, 0, h->d_P, d_fP);
    hipLaunchKernelGGL(k_build_frag_edges, dim3(C * E), dim3(256), 0, h->stream, k, T, kk4, 1, h->d_P, d_fPT);
    hipLaunchKernelGGL(k_build_frag_edges, dim3(C * E), dim3(256), 0, h->stream, k, T, kk4, nodes ? 1 : 0, d_M, d_fD);   /* node visits apply M^T */
    hipLaunchKernelGGL(k_build_tip_dist, dim3(ntips + 1, C), dim3(256), 0, h->stream,
                       k, R, E, ntips, h->nchar, d_te, h->d_Pdd, h->d_defs, h->K, d_tipd);
    hipLaunchKernelGGL(k_build_dtip_dist, dim3(ntips + 1, C), dim3(256), 0, h->stream,
                       k, R, E, ntips, h->nchar, d_te, d_M, h->d_defs, h->K, d_dtip, dzero);
    if (hipGetLastError() != hipSuccess) { h->err = "plk_deriv/plk_marginal: table build failed"; return PLK_E_DEVICE; }

    const bool msum_only = marginal_sums_only(deriv, marg, site_out, sums_out);
    const size_t per_site = ((size_t)(nie + 2 * (size_t)nin) * C * R * 4 + (size_t)nslots_m * R * 4 + (size_t)(nsc + 2) * C + 1 + (deriv ? E : 0) + (marg && !msum_only ? (size_t)N * k : 0)) * sizeof(double);
    long chunk;
    if ((rc = plan_site_chunk(h, "plk_deriv/plk_marginal", per_site + (msum_only ? ((size_t)N * h->k / 64 + 1) * sizeof(double) : 0), MF_SITES, true, &chunk))) return rc;
    /* site-summed marginals: one weighted sum per wave, node and state (sized for a whole chunk) */
    const size_t mvs_doubles = msum_only ? (size_t)N * k * (size_t)((chunk + MF_SITES - 1) / MF_SITES) * (MF_BLOCK / 64) : 0;
    if ((rc = dev_reserve(h, &h->d_work, &h->work_cap, per_site / sizeof(double) * (size_t)chunk + mvs_doubles))) return rc;

    std::vector<long double> dsum(deriv ? E : 0, 0.0L), msum(marg ? (size_t)N * k : 0, 0.0L);
    for (long s0 = 0; s0 < S; s0 += chunk) {
        const long n = std::min(chunk, S - s0);
        const unsigned grid = (unsigned)((n + MF_SITES - 1) / MF_SITES);
        MUpArgs a;
        a.S = S; a.Spad = h->Spad; a.s0 = s0; a.n = n;
        a.N = N; a.E = E; a.k = k; a.kk4 = kk4; a.C = C; a.nchar = h->nchar; a.ntips = ntips; a.root_mode = h->root_mode;
        a.dzero = dzero;
        a.indptr = h->d_indptr; a.indices = h->d_indices; a.preorder = h->d_preorder; a.node_has_data = d_has;
        a.edge_tip = d_et; a.edge_int = d_ei; a.node_int = d_ni;
        a.fragP = d_fP; a.fragPT = d_fPT; a.fragD = d_fD; a.tip = d_tipd; a.dtip = d_dtip;
        a.codes = h->d_codes; a.cat_prior = h->d_cat_prior; a.root_wd = d_rwd; a.edge_mask = d_emask; a.node_mask = d_nmask;
        a.stride = (long)grid * MF_SITES * 4;
        double *p = h->d_work;
        a.EV = p; p += (size_t)nie * C * R * a.stride;
        a.LN = p; p += (size_t)nin * C * R * a.stride;
        a.FN = p; p += (size_t)nin * C * R * a.stride;
        a.node_scale = d_ns;
        MDownProg pg;
        pg.ops = d_dops; pg.nops = (int)h->ops.size(); pg.nobs = (int)h->obs_nodes.size(); pg.obs_nodes = d_obsm;
        pg.slots = p; p += (size_t)nslots_m * R * a.stride;
        a.SC = p; p += (size_t)nsc * C * n;
        a.CW = p; p += (size_t)C * n;
        a.XC = p; p += (size_t)C * n;
        a.LH = p; p += n;
        a.DV = p; if (deriv) p += (size_t)E * n;
        const size_t nwv = (size_t)grid * (MF_BLOCK / 64);
        a.MV = p; a.MVS = nullptr; a.wsite = nullptr;
        if (marg && msum_only) { a.MVS = p; a.wsite = h->d_w ? h->d_w + s0 : nullptr; p += (size_t)N * k * nwv; }
        else if (marg) p += (size_t)N * k * n;
        if (deriv && edge_mask) HIPCHK(h, hipMemsetAsync(a.DV, 0, (size_t)E * n * sizeof(double), h->stream));   /* without a mask every edge's row is written by the up pass */
        if (marg) HIPCHK(h, hipMemsetAsync(a.MV, 0, (msum_only ? (size_t)N * k * nwv : (size_t)N * k * n) * sizeof(double), h->stream));
        const size_t lds = (size_t)T * kk4 * 64 * sizeof(double);
        a.visits = nodes ? pk + o_vis : nullptr; a.nvisits = un.nvisits;
        a.node_inline = any_inl ? pk + o_inl : nullptr;
        const bool nv = nodes && (s0 % MF_SITES) == 0;       /* chunks start at multiples of the site tile */
        if (T == 1) launch_updown_mfma<1>(h, a, pg, grid, lds, deriv, marg, nv);
        else if (T == 2) launch_updown_mfma<2>(h, a, pg, grid, lds, deriv, marg, nv);
        else if (T == 3) launch_updown_mfma<3>(h, a, pg, grid, lds, deriv, marg, nv);
        else launch_updown_mfma<4>(h, a, pg, grid, lds, deriv, marg, nv);
        if (hipGetLastError() != hipSuccess) { h->err = "plk_deriv/plk_marginal: kernel launch failed"; return PLK_E_DEVICE; }
        UpDownOut o;
        o.drows = dsum.size(); o.mrows = msum.size(); o.nwv = nwv; o.DV = a.DV; o.MV = a.MV; o.MVS = a.MVS;
        if ((rc = updown_chunk_out(h, o, n, s0, sums_out != nullptr, dsum.data(), msum.data(), site_out))) return rc;
    }
    return updown_finish(h, sums_out, deriv ? dsum : msum);
}

/* deriv / marginal for k = 4 with compact codes: interleaved-vector kernels (plk_updown4.h) */
/* plk_edge_pair_sums asks the down / up drivers for the outer-product pass instead of an edge form: deriv = marg = false,
 * no edge-form matrices; acc receives [C][E][k][k] edge rows and then [C][k] root rows */
struct PairSumReq {
    std::vector<long double> acc;
    bool want_root = false;
    bool zero_lh = false;        /* a site of likelihood 0 with a non-zero weight was met */
    /* plk_mixture_sens: the same drivers run the mixture-gradient pass (plk_mixsens.h) when mix_D is set: [C][E][k][k]
     * direction matrices on the device; acc then receives the rows that pass writes (the k = 4 kernel: 2 MIX4_MAX_C rows,
     * prior c at c, rate c at MIX4_MAX_C + c; the generic kernel: C prior rows, then C rate rows) */
    const double *mix_D = nullptr;
};
/* plk_nni_ll asks the same drivers for the swap pass (plk_nni.h) instead of an edge form: deriv = marg = false, no
 * edge-form matrices.  swaps: [n][2] validated CSR edge pairs (a, b); the up pass runs once per group of NNI_MAX_ROWS */
struct NniReq {
    int n = 0;
    const int *swaps = nullptr;
    double *site_out = nullptr;        /* null or [n][S] host */
    std::vector<long double> acc;      /* [n] weighted site sums (filled when want_sums) */
    bool want_sums = false;
    /* maps of the tree, made once by plk_nni_ll for the check of the pairs and for the records of every group */
    std::vector<int> par, in, pos;     /* upper node of every CSR edge; edge into every node (-1: root); preorder position */
};

/* parent node of every CSR edge */
static std::vector<int> edge_parents(int N, const int *indptr)
{
    std::vector<int> par(indptr[N], -1);
    for (int a = 0; a < N; a++)
        for (int idx = indptr[a]; idx < indptr[a + 1]; idx++) par[idx] = a;
    return par;
}

/* "" when (a, b) is a swap of the tree: a = (v -> c), b = (u -> s), v a child of u, s != v; else why it is none */
static std::string nni_pair_fault(int N, const int *indptr, const int *indices, const std::vector<int> &par,
                                  const std::vector<int> &in_edge, int a, int b)
{
    const int E = indptr[N];
    if (a < 0 || a >= E || b < 0 || b >= E) return "edge index out of range";
    if (a == b) return "the same edge twice";
    const int v = par[a], u = par[b];
    if (in_edge[v] < 0) return "the first edge starts at the root";
    if (par[in_edge[v]] != u) return "the first edge does not start at a child of the second edge's upper node";
    if (indices[b] == v) return "the second edge ends where the first starts";
    return "";
}

/* edge into every node (-1 for the root) */
static std::vector<int> in_edges(int N, const int *indptr, const int *indices)
{
    std::vector<int> in(N, -1);
    for (int idx = 0; idx < indptr[N]; idx++) in[indices[idx]] = idx;
    return in;
}

/* records of plk_nni.h for the swaps [g0, g0 + ng) of the request, sorted by the preorder position of the upper node;
 * pair_ok: the kernel takes records of two swaps (the k = 4 kernel) */
static std::vector<int> nni_records(const plk_engine *h, const NniReq &q, int g0, int ng, bool pair_ok)
{
    const int *ip = h->indptr.data();
    const std::vector<int> &par = q.par, &in = q.in, &pos = q.pos;
    struct Rec { int w[NNI_REC]; };
    std::vector<Rec> recs;
    std::vector<int> open_rec((size_t)h->E, -1);     /* per edge (u -> v): the record of two swaps still taking rows, by b */
    for (int i = 0; i < ng; i++) {
        const int a = q.swaps[2 * (g0 + i)], b = q.swaps[2 * (g0 + i) + 1];
        const int v = par[a], u = par[b], idx_v = in[v];
        const bool two = pair_ok && ip[u + 1] - ip[u] == 2 && ip[v + 1] - ip[v] == 2;
        if (two) {
            const int second = a == ip[v] ? 0 : 1;
            int ri = open_rec[idx_v];
            if (ri < 0 || recs[ri].w[4 + 2 * second] >= 0) {
                Rec r = {{pos[u], idx_v, b, ip[v], -1, ip[v] + 1, -1, 0}};
                ri = (int)recs.size();
                recs.push_back(r);
                open_rec[idx_v] = ri;
            }
            recs[ri].w[4 + 2 * second] = i;
        } else {
            Rec r = {{pos[u], idx_v, b, a, i, -1, -1, 0}};
            recs.push_back(r);
        }
    }
    std::stable_sort(recs.begin(), recs.end(), [](const Rec &x, const Rec &y) { return x.w[0] < y.w[0]; });
    std::vector<int> out;
    out.reserve(recs.size() * NNI_REC);
    for (const Rec &r : recs) out.insert(out.end(), r.w, r.w + NNI_REC);
    return out;
}

/* per group of swaps: the records go to the device with the call's other integer tables */
struct NniGroups {
    std::vector<size_t> off;           /* offset of the group's records in the pack */
    std::vector<int> nrec;
    int rows = 0;                      /* rows of the plane: the largest group */
    void put(const plk_engine *h, const NniReq &q, bool pair_ok, IntPack &pack)
    {
        for (int g0 = 0; g0 < q.n; g0 += NNI_MAX_ROWS) {
            const int ng = std::min(NNI_MAX_ROWS, q.n - g0);
            const std::vector<int> r = nni_records(h, q, g0, ng, pair_ok);
            off.push_back(pack.put(r.data(), r.size()));
            nrec.push_back((int)(r.size() / NNI_REC));
            rows = std::max(rows, ng);
        }
    }
};

/* one chunk's outputs of one group: rows of the plane to their places in site_out, weighted row sums into acc */
static int nni_group_out(plk_engine *h, NniReq *q, int g0, int ng, long n, long s0, const double *plane)
{
    int rc;
    if (q->want_sums && (rc = wsum_rows(h, ng, n, plane, h->d_w ? h->d_w + s0 : nullptr, q->acc.data() + g0))) return rc;
    if (q->site_out) {
        HIPCHK(h, hipMemcpy2DAsync(q->site_out + (size_t)g0 * h->S + s0, (size_t)h->S * sizeof(double), plane, (size_t)n * sizeof(double),
                                   (size_t)n * sizeof(double), (size_t)ng, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return PLK_OK;
}

/* plk_place_ll asks the same drivers for the placement pass (plk_place.h).  Rows are counted edge-major, t = ei Q + q
 * for position ei of the edge list and query q, so that a pass of PLACE_MAX_ROWS rows names as few edges as it can; the
 * caller's order [Q][n_edges] is restored when rows leave (place_group_out, plk_place_ll) */
struct PlaceReq {
    int Q = 0, ne = 0;
    const int *edges = nullptr;        /* [ne] validated CSR edges */
    std::vector<int> slot;             /* [ne] index of the edge among the distinct target edges of the call */
    std::vector<double> rates;         /* [2 distinct + 1]: upper part, lower part of every distinct edge; the pendant edge */
    bool compact = false;              /* the queries are codes (d_plcodes) or dense rows (d_pldense) */
    double *site_out = nullptr;        /* null or [Q][ne][S] host */
    std::vector<long double> acc;      /* [ne][Q] weighted site sums (filled when want_sums) */
    bool want_sums = false;
    std::vector<int> par, pos;         /* upper node of every CSR edge; preorder position of every node */
    std::vector<double> stage;         /* per-site rows of one pass on their way to site_out */
    long total() const { return (long)ne * Q; }
};

/* the call's transition matrices: one more launch of K1 over the call's rates into the call's buffers (no dP) */
static int call_matrices(plk_engine *h, const std::vector<double> &rates)
{
    const int k = h->k, C = h->C, EQ = (int)rates.size();
    const size_t kk = (size_t)k * k, nmat = (size_t)C * EQ * kk;
    int rc;
    if ((rc = dev_reserve(h, &h->d_plPdd, &h->plpdd_cap, nmat)) || (rc = dev_reserve(h, &h->d_plP, &h->plp_cap, nmat)) ||
        (rc = dev_reserve(h, &h->d_plrates, &h->plrates_cap, (size_t)EQ))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_plrates, rates.data(), (size_t)EQ * sizeof(double), hipMemcpyHostToDevice, h->stream));
    const int threads = kk >= 1024 ? 1024 : (kk >= 256 ? 256 : 64);
    int use_lds;
    const size_t lds_bytes = expm_lds_bytes((size_t)k, threads, &use_lds);
    if (!use_lds) { if ((rc = dev_reserve(h, &h->d_scratch, &h->scratch_cap, (size_t)C * std::max(EQ, h->E) * EXPM_BUFFERS * kk))) return rc; }
    ExpmPost ep = {};
    ep.skip_dP = 1;
    hipLaunchKernelGGL(k_expm_dd<false>, dim3(C * EQ), dim3(threads), lds_bytes, h->stream,
                       k, EQ, h->d_Qn, h->d_plrates, h->d_cat_rates, h->d_plPdd, h->d_plP, (double *)nullptr,
                       h->d_scratch, use_lds, (const double *)nullptr, 0L, 0, (const int *)nullptr, (double *)nullptr, ep);
    HIPCHK(h, hipGetLastError());
    return PLK_OK;
}

static int place_matrices(plk_engine *h, const PlaceReq &q) { return call_matrices(h, q.rates); }

/* records of plk_place.h for every pass of the call; they go to the device with the call's other integer tables */
struct PlaceGroups {
    std::vector<size_t> off;           /* offset of the pass's records in the pack */
    std::vector<int> nrec;
    int rows = 0;                      /* rows of the plane: the largest pass */
    void put(const PlaceReq &q, IntPack &pack)
    {
        struct Rec { int w[PLACE_REC]; };
        for (long g0 = 0; g0 < q.total(); g0 += PLACE_MAX_ROWS) {
            const long g1 = std::min<long>(g0 + PLACE_MAX_ROWS, q.total());
            std::vector<Rec> recs;
            for (long t = g0; t < g1;) {
                const int ei = (int)(t / q.Q), q0 = (int)(t % q.Q);
                const int cnt = (int)std::min<long>(q.Q - q0, g1 - t);
                const int e = q.edges[ei];
                Rec r = {{q.pos[q.par[e]], e, q.slot[ei], q0, cnt, (int)(t - g0)}};
                recs.push_back(r);
                t += cnt;
            }
            std::stable_sort(recs.begin(), recs.end(), [](const Rec &x, const Rec &y) { return x.w[0] < y.w[0]; });
            std::vector<int> out;
            for (const Rec &r : recs) out.insert(out.end(), r.w, r.w + PLACE_REC);
            off.push_back(pack.put(out.data(), out.size()));
            nrec.push_back((int)recs.size());
            rows = std::max(rows, (int)(g1 - g0));
        }
    }
};

/* one chunk's outputs of one pass: weighted row sums into acc (edge-major), rows of the plane to their places in site_out */
static int place_group_out(plk_engine *h, PlaceReq *q, long g0, int ng, long n, long s0, const double *plane)
{
    int rc;
    if (q->want_sums && (rc = wsum_rows(h, ng, n, plane, h->d_w ? h->d_w + s0 : nullptr, q->acc.data() + g0))) return rc;
    if (q->site_out) {
        q->stage.resize((size_t)ng * n);
        HIPCHK(h, hipMemcpyAsync(q->stage.data(), plane, (size_t)ng * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (int i = 0; i < ng; i++) {
            const long t = g0 + i, ei = t / q->Q, qi = t % q->Q;
            std::copy(q->stage.begin() + (size_t)i * n, q->stage.begin() + (size_t)(i + 1) * n, q->site_out + ((size_t)qi * q->ne + ei) * h->S + s0);
        }
    }
    return PLK_OK;
}

/* plk_spr_ll asks the same drivers for the prune-and-regraft pass (plk_spr.h).  The moves are grouped by their prune edge
 * (order: by p, ties in the caller's order); rows and sums are kept in that order and leave in the caller's */
struct SprReq {
    int n = 0;
    const int *moves = nullptr;        /* [n][2] validated (p, e) */
    std::vector<int> order;            /* [n] positions in the caller's list, grouped by p */
    std::vector<int> slot;             /* [n] (caller's order) index of e among the distinct target edges of the call */
    std::vector<double> rates;         /* [2 distinct]: upper part, lower part of every distinct target edge */
    double *site_out = nullptr;        /* null or [n][S] host */
    std::vector<long double> acc;      /* [n] weighted site sums in grouped order (filled when want_sums) */
    bool want_sums = false;
    std::vector<int> epar;             /* upper node of every CSR edge */
    std::vector<int> pos;              /* position of every node in the engine's order (what the records are sorted by) */
    std::vector<int> dpos, size, depth, par, in;   /* the node tables of SprOut (dpos: depth-first preorder position) */
    int max_depth = 0;
    std::vector<double> stage;         /* per-site rows of one pass on their way to site_out */
};

/* the passes of the call and their records; they go to the device with the call's other integer tables */
struct SprGroups {
    struct Pass { int p; int first; size_t off; int nrec; int g0; };
    std::vector<Pass> pass;
    size_t o_pos = 0, o_size = 0, o_depth = 0, o_par = 0, o_in = 0;
    int rows = 0;
    void put(const SprReq &q, IntPack &pack)
    {
        struct Rec { int w[SPR_REC]; };
        const int N = (int)q.pos.size();
        o_pos = pack.put(q.dpos.data(), (size_t)N); o_size = pack.put(q.size.data(), (size_t)N); o_depth = pack.put(q.depth.data(), (size_t)N);
        o_par = pack.put(q.par.data(), (size_t)N); o_in = pack.put(q.in.data(), (size_t)N);
        for (int g0 = 0; g0 < q.n;) {
            const int p = q.moves[2 * q.order[g0]];
            int gend = g0;
            while (gend < q.n && q.moves[2 * q.order[gend]] == p) gend++;
            for (int t0 = g0; t0 < gend; t0 += PLACE_MAX_ROWS) {
                const int t1 = std::min(t0 + PLACE_MAX_ROWS, gend);
                std::vector<Rec> recs;
                for (int t = t0; t < t1; t++) {
                    const int i = q.order[t], e = q.moves[2 * i + 1];
                    recs.push_back(Rec{{q.pos[q.epar[e]], e, q.slot[i], t - t0}});
                }
                std::stable_sort(recs.begin(), recs.end(), [](const Rec &x, const Rec &y) { return x.w[0] < y.w[0]; });
                std::vector<int> out;
                for (const Rec &r : recs) out.insert(out.end(), r.w, r.w + SPR_REC);
                pass.push_back(Pass{p, t0 == g0 ? 1 : 0, pack.put(out.data(), out.size()), (int)recs.size(), t0});
                rows = std::max(rows, t1 - t0);
            }
            g0 = gend;
        }
    }
    SprOut out(const SprReq &q, const int *b, size_t i) const
    {
        SprOut o = {};
        o.rec = b + pass[i].off; o.nrec = pass[i].nrec; o.store_fn = pass[i].first; o.p = pass[i].p;
        o.pos = b + o_pos; o.size = b + o_size; o.depth = b + o_depth; o.par = b + o_par; o.in = b + o_in;
        o.EQ = (int)q.rates.size();
        return o;
    }
};

/* one chunk's outputs of one pass: weighted row sums into acc (grouped order), rows of the plane to their places in site_out */
static int spr_group_out(plk_engine *h, SprReq *q, int g0, int ng, long n, long s0, const double *plane)
{
    int rc;
    if (q->want_sums && (rc = wsum_rows(h, ng, n, plane, h->d_w ? h->d_w + s0 : nullptr, q->acc.data() + g0))) return rc;
    if (q->site_out) {
        q->stage.resize((size_t)ng * n);
        HIPCHK(h, hipMemcpyAsync(q->stage.data(), plane, (size_t)ng * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (int i = 0; i < ng; i++)
            std::copy(q->stage.begin() + (size_t)i * n, q->stage.begin() + (size_t)(i + 1) * n, q->site_out + (size_t)q->order[g0 + i] * h->S + s0);
    }
    return PLK_OK;
}

/* workgroups of the pair-sum passes: fixed by the device, so the partial sums never grow with S */
static unsigned pair_sums_grid(const plk_engine *h, long nbatch) { return (unsigned)std::min<long>(nbatch, 4L * h->num_cus); }

static int pair_sums_finish(plk_engine *h, PairSumReq *ps, size_t rows, unsigned grid, const double *part, const int *d_flag)
{
    int rc;
    for (size_t r0 = 0; r0 < rows; r0 += 32768) {       /* gridDim.y of k_wsum_rows */
        const size_t nr = std::min<size_t>(32768, rows - r0);
        if ((rc = wsum_rows(h, (int)nr, (long)grid, part + r0 * grid, nullptr, ps->acc.data() + r0))) return rc;
    }
    int flag = 0;
    HIPCHK(h, hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (flag) ps->zero_lh = true;
    return PLK_OK;
}

static int run_updown4(plk_engine *h, bool deriv, bool marg, const int *edge_mask, const int *node_mask,
                       double *site_out, double *sums_out, const double *d_M, int dzero, int nM, PairSumReq *ps = nullptr, NniReq *nni = nullptr,
                       PlaceReq *pl = nullptr, SprReq *sp = nullptr)
{
    int rc;
    const int N = h->N, E = h->E, C = h->C;
    const int ER = nM * E;                 /* rows of the edge-form output: [form][edge] */
    const long S = h->S;
    if (h->prog_dirty) { if ((rc = build_program(h))) return rc; }
    const PlkStorageMaps sm = storage_maps(h);               /* E > 0 here (use_updown4, pair_sums_run): the edge mask and the edge rows below are never empty */
    const std::vector<int> &edge_tip = sm.edge_tip, &edge_int = sm.edge_int, &node_int = sm.node_int, &node_scale = sm.node_scale;
    const int ntips = sm.ntips, nie = sm.nie, nin = sm.nin, nsc = sm.nsc;

    /* nodes the up pass handles inside their parent's visit (see Up4Args.node_inline) */
    std::vector<int> node_inline(N, 0);
    for (int p = 0; p < N; p++) {
        const int pdeg = h->indptr[p + 1] - h->indptr[p];
        if (pdeg < 1 || pdeg > 2) continue;
        for (int idx = h->indptr[p]; idx < h->indptr[p + 1]; idx++) {
            const int b = h->indices[idx];
            const int bdeg = h->indptr[b + 1] - h->indptr[b];
            if (bdeg < 1 || bdeg > 2) continue;
            bool all_leaves = true;
            for (int j = h->indptr[b]; j < h->indptr[b + 1]; j++) all_leaves = all_leaves && edge_tip[j] >= 0;
            if (all_leaves) node_inline[b] = 1;
        }
    }
    /* derivative queries proper (edge form dP, no marginals, at most 4 rate categories; the expectation queries keep k_up4,
     * whose several-forms-per-pass variant they must agree with bit for bit): node-visit up pass k_up4_nodes, which
     * keeps the vector of a continued child in registers for all categories; PLK_OPT_UP_NODES bit 1 switches it off */
    const bool nodes4 = deriv && !marg && nM == 1 && dzero && C <= 4 && E > 0 && (h->opt_up_nodes & 2);
    /* Pair messages (round 3): a node whose two children are leaves, without data of its own, sends its parent one of
     * nchar^2 vectors P_a (P_b B_b o P_c B_c).  With the node-visit up pass those come from a table (k_build_tables_pt, the
     * ll kernels' pair tables), so the down pass does not store L_a and the up pass does not read it: a third of the
     * down pass's writes and a fifth of the up pass's reads at BASELINE config 3. */
    std::vector<int> pair_of(N, -1), pair_tabs;
    std::vector<char> skip_l(N, 0);
    int npairs4 = 0;
    if (nodes4 && h->nchar <= 16 && h->opt_pair_tables) {
        if (h->node_has_data.size() != (size_t)N) h->node_has_data.assign(N, 1);
        std::vector<int> t_unit, t_edge, t_eb, t_ec;
        for (int b = 0; b < N; b++) {
            const int e0 = h->indptr[b];
            if (h->indptr[b + 1] - e0 != 2 || h->b_to_idx[b] < 0 || h->node_has_data[b]) continue;
            if (edge_tip[e0] < 0 || edge_tip[e0 + 1] < 0) continue;
            pair_of[b] = npairs4; skip_l[b] = 1;
            t_unit.push_back(npairs4 * h->nchar); t_edge.push_back(h->b_to_idx[b]); t_eb.push_back(e0); t_ec.push_back(e0 + 1);
            npairs4++;
        }
        pair_tabs = t_unit;
        pair_tabs.insert(pair_tabs.end(), t_edge.begin(), t_edge.end());
        pair_tabs.insert(pair_tabs.end(), t_eb.begin(), t_eb.end());
        pair_tabs.insert(pair_tabs.end(), t_ec.begin(), t_ec.end());
    }
    /* One level up: a node whose two children are leaves or pair nodes has L = (row of one table) o (row of another).  The
     * down pass does not store it and the node-visit up pass multiplies the two rows (plk_up_rebuild_table; PLK_OPT_UP_NODES
     * bit 2 switches it off). */
    std::vector<char> rebuild_n;
    std::vector<int> rebuild_tab;
    bool any_rebuild = false;
    if (nodes4 && !(h->opt_up_nodes & 4)) {
        if (h->node_has_data.size() != (size_t)N) h->node_has_data.assign(N, 1);
        plk_up_rebuild_table(N, h->indptr.data(), h->indices.data(), h->node_has_data.data(), edge_tip.data(), node_int.data(),
                             node_scale.data(), pair_of.data(), nin, rebuild_n, rebuild_tab);
        for (int b = 0; b < N; b++) if (rebuild_n[b]) { skip_l[b] = 1; any_rebuild = true; }
    }
    /* down-pass program: observation ops carry their staged code row and the (slot, row) of the next one */
    PlkChain ch2;
    plk_chain_build(N, h->pg, 1, h->indices.data(), node_int.data(), nullptr, node_scale.data(), ch2, npairs4 || any_rebuild ? skip_l.data() : nullptr);
    const int nobs2 = (int)h->obs_nodes.size();
    {
        const int D2 = h->slots_needed <= 4 ? 4 : (h->slots_needed <= 8 ? 8 : (h->slots_needed <= 16 ? 16 : INT_MAX));
        const std::string bad = plk_chain_check(N, h->pg, ch2, 1, D2, nin, nie, nsc, UD4_BLOCK, (size_t)nobs2 * UD4_BLOCK);
        if (!bad.empty()) { h->err = "internal: " + bad; return PLK_E_ARG; }
    }
    const std::vector<plk_op4> &ops2 = ch2.ops;
    const int first_slot2 = ch2.first_slot, first_row2 = ch2.first_row;
    PlkUpNodes un4;
    const bool inline4 = npairs4 > 0 && C == 1 && !(h->opt_up_nodes & 8);      /* two-leaf nodes finish inside their parent's visit */
    if (nodes4) {
        if (h->node_has_data.size() != (size_t)N) h->node_has_data.assign(N, 1);
        plk_up_nodes_build(N, h->indptr.data(), h->indices.data(), h->preorder.data(), h->node_has_data.data(), edge_tip.data(),
                           node_int.data(), node_scale.data(), edge_mask, un4, npairs4 ? pair_of.data() : nullptr,
                           any_rebuild ? rebuild_n.data() : nullptr, inline4);
        const std::string bad = plk_up_nodes_check(N, E, h->indptr.data(), h->indices.data(), un4, nin, ntips, nsc, npairs4, edge_tip.data(),
                                                   any_rebuild ? rebuild_tab.data() : nullptr, pair_of.data());
        if (!bad.empty()) { h->err = "internal: " + bad; return PLK_E_ARG; }
    }
    if (!ps && !nni && !pl && !sp) h->info_up4_path = nodes4 ? 1 | (npairs4 > 0 ? 2 : 0) | (any_rebuild ? 4 : 0) | (inline4 ? 8 : 0) : 0;
    const size_t ntab = (size_t)C * (ntips + 1) * h->nchar * 4;
    /* all small integer tables of this call in one host block, one upload */
    IntPack pack;
    const size_t o_ops = pack.put(reinterpret_cast<const int *>(ops2.data()), ops2.size() * 4);
    const size_t o_et = pack.put(edge_tip.data(), (size_t)E), o_ei = pack.put(edge_int.data(), (size_t)E), o_ni = pack.put(node_int.data(), (size_t)N);
    const size_t o_te = pack.put(sm.tip_edges.data(), sm.tip_edges.size()), o_has = pack.put_has_data(h), o_ns = pack.put(node_scale.data(), (size_t)N);
    const size_t o_oe = pack.put(h->op_edge.data(), h->op_edge.size()), o_obs = pack.put(h->obs_nodes.data(), h->obs_nodes.size());
    const size_t o_inl = pack.put(node_inline.data(), (size_t)N);
    const size_t o_em = pack.put_opt(edge_mask, (size_t)E), o_nm = pack.put_opt(node_mask, (size_t)N);
    const size_t o_vis = nodes4 ? pack.put(un4.rec.data(), un4.rec.size()) : 0;
    const size_t o_pt = npairs4 ? pack.put(pair_tabs.data(), pair_tabs.size()) : 0;
    const size_t o_rb = any_rebuild ? pack.put(rebuild_tab.data(), rebuild_tab.size()) : 0;
    NniGroups ng4;
    if (nni) ng4.put(h, *nni, true, pack);
    PlaceGroups pg4;
    const int pl_tip_edge = pl ? (int)pl->rates.size() - 1 : 0;      /* the pendant matrix, as the one "tip edge" of its table */
    const size_t o_pte = pl ? pack.put(&pl_tip_edge, 1) : 0;
    if (pl) pg4.put(*pl, pack);
    SprGroups sg4;
    if (sp) sg4.put(*sp, pack);
    const size_t nptab = (size_t)C * npairs4 * h->nchar * h->nchar * 4;
    if ((rc = dev_reserve(h, &h->d_u4tip, &h->u4tip_cap, ntab * (size_t)(1 + nM) + nptab)) || (rc = pack.upload(h))) return rc;
    int *const d_psflag = pack.flag(h);
    const int *b = h->d_u4pack;
    const int4 *d_ops2 = reinterpret_cast<const int4 *>(b + o_ops);
    const int *d_et = b + o_et, *d_ei = b + o_ei, *d_ni = b + o_ni, *d_te = b + o_te, *d_has = b + o_has, *d_ns = b + o_ns;
    const int *d_oe2 = b + o_oe, *d_obs2 = b + o_obs, *d_inl = b + o_inl;
    const int *d_emask = edge_mask ? b + o_em : nullptr, *d_nmask = node_mask ? b + o_nm : nullptr;
    const int *d_vis4 = nodes4 ? b + o_vis : nullptr, *d_ptabs = npairs4 ? b + o_pt : nullptr, *d_rebuild = any_rebuild ? b + o_rb : nullptr;
    double *d_tip4 = h->d_u4tip, *d_dtip4 = h->d_u4tip + ntab, *d_ptab4 = h->d_u4tip + ntab * (size_t)(1 + nM);
    hipLaunchKernelGGL(k_build_tip, dim3(ntips + 1, C), dim3(64), 0, h->stream,
                       E, ntips + 1, h->nchar, d_te, h->d_Pdd, h->d_defs, d_tip4);
    for (int m = 0; m < nM; m++)
        hipLaunchKernelGGL(k_build_dtip4, dim3(ntips + 1, C), dim3(64), 0, h->stream,
                           E, ntips, h->nchar, d_te, d_M + (size_t)m * C * E * 16, h->d_defs, d_dtip4 + (size_t)m * ntab, dzero);
    if (npairs4)       /* pair tables: [C][npairs * nchar units][nchar][4], the ll kernels' builder on a list of pairs only */
        hipLaunchKernelGGL(k_build_tables_pt, dim3(npairs4, C), dim3(64), 0, h->stream,
                           E, npairs4, npairs4 * h->nchar, h->nchar, d_ptabs, h->d_Pdd, h->d_defs, d_ptab4);
    if (pl) {
        /* pendant tables [C][nchar][4] = D defs[code], built as the tip tables are (double-double, constant rows unchanged) */
        if ((rc = dev_reserve(h, &h->d_plT, &h->plt_cap, (size_t)C * h->nchar * 4))) return rc;
        hipLaunchKernelGGL(k_build_tip, dim3(1, C), dim3(64), 0, h->stream,
                           (int)pl->rates.size(), 1, h->nchar, b + o_pte, h->d_plPdd, h->d_defs, h->d_plT);
    }
    if (hipGetLastError() != hipSuccess) { h->err = "plk_deriv/plk_marginal: table build failed"; return PLK_E_DEVICE; }

    const bool msum_only = marginal_sums_only(deriv, marg, site_out, sums_out);      /* per-wave sums instead of the N x 4 planes */
    const size_t per_site = ((size_t)(2 * (size_t)nin) * C * 4 + (size_t)(nsc + 2) * C + 1 + (deriv ? ER : 0) + (marg && !msum_only ? (size_t)N * 4 : 0) + (size_t)ng4.rows + (size_t)pg4.rows +
                             (sp ? (size_t)sg4.rows + (size_t)(sp->max_depth + 1) * C * 4 + 1 : 0)) * sizeof(double);
    long chunk;
    if ((rc = plan_site_chunk(h, "plk_deriv/plk_marginal", per_site + (msum_only ? ((size_t)N * h->k / 64 + 1) * sizeof(double) : 0), UD4_BLOCK, false, &chunk))) return rc;
    const size_t mvs_doubles = msum_only ? (size_t)N * 4 * (size_t)((chunk + UD4_BLOCK - 1) / UD4_BLOCK) * (UD4_BLOCK / 64) : 0;   /* per-wave marginal sums */
    const size_t ps_rows = ps ? (ps->mix_D ? (size_t)2 * MIX4_MAX_C : (size_t)C * E * 16 + (size_t)C * 4) : 0;
    const size_t ps_doubles = ps ? ps_rows * pair_sums_grid(h, (chunk + PS4_BLOCK - 1) / PS4_BLOCK) : 0;
    if ((rc = dev_reserve(h, &h->d_work, &h->work_cap, per_site / sizeof(double) * (size_t)chunk + mvs_doubles + ps_doubles))) return rc;
    if (ps) {
        ps->acc.assign(ps_rows, 0.0L);
        HIPCHK(h, hipMemsetAsync(d_psflag, 0, sizeof(int), h->stream));
    }

    std::vector<long double> dsum(deriv ? ER : 0, 0.0L), msum(marg ? (size_t)N * 4 : 0, 0.0L);
    for (long s0 = 0; s0 < S; s0 += chunk) {
        const long n = std::min(chunk, S - s0);
        Up4Args a;
        a.S = S; a.Spad = h->Spad; a.s0 = s0; a.n = n;
        a.N = N; a.E = E; a.C = C; a.nchar = h->nchar; a.ntips = ntips; a.root_mode = h->root_mode;
        a.dzero = dzero;
        a.indptr = h->d_indptr; a.indices = h->d_indices; a.preorder = h->d_preorder; a.node_has_data = d_has;
        a.edge_tip = d_et; a.edge_int = d_ei; a.node_int = d_ni; a.node_scale = d_ns; a.node_inline = d_inl;
        a.P = h->d_P; a.dP = d_M; a.tip = d_tip4; a.dtip = d_dtip4; a.nM = nM;
        a.codes = h->d_codes; a.cat_prior = h->d_cat_prior; a.root_w = h->d_root_w; a.edge_mask = d_emask; a.node_mask = d_nmask;
        double *p = h->d_work;
        a.LN = p; p += (size_t)nin * C * 4 * n;
        a.FN = p; p += (size_t)nin * C * 4 * n;
        a.SC = p; p += (size_t)nsc * C * n;
        a.CW = p; p += (size_t)C * n;
        a.XC = p; p += (size_t)C * n;
        a.LH = p; p += n;
        a.DV = p; if (deriv) p += (size_t)ER * n;
        const unsigned grid = (unsigned)((n + UD4_BLOCK - 1) / UD4_BLOCK);
        const size_t nwv = (size_t)grid * (UD4_BLOCK / 64);
        a.MV = p; a.MVS = nullptr; a.wsite = nullptr;
        if (marg && msum_only) { a.MVS = p; a.wsite = h->d_w ? h->d_w + s0 : nullptr; p += (size_t)N * 4 * nwv; }
        else if (marg) p += (size_t)N * 4 * n;
        a.visits = d_vis4; a.nvisits = un4.nvisits; a.ptab = npairs4 ? d_ptab4 : nullptr; a.npairs = npairs4; a.rebuild = d_rebuild;
        /* (the node-visit pass writes the row of every wanted edge: rows need clearing only under a mask) */
        if (deriv && E > 0 && !(nodes4 && !edge_mask)) HIPCHK(h, hipMemsetAsync(a.DV, 0, (size_t)ER * n * sizeof(double), h->stream));
        if (marg) HIPCHK(h, hipMemsetAsync(a.MV, 0, (msum_only ? (size_t)N * 4 * nwv : (size_t)N * 4 * n) * sizeof(double), h->stream));
        const size_t lds_codes = (size_t)nobs2 * UD4_BLOCK;
        const bool fused_ok = d_ops2 && lds_codes <= 60 * 1024 && (s0 % UD4_BLOCK) == 0;
        h->info_down4_kernel = !fused_ok || h->slots_needed > 16 ? 0 : (h->slots_needed <= 4 ? 4 : (h->slots_needed <= 8 ? 8 : 16));
        if (fused_ok && h->slots_needed <= 4) hipLaunchKernelGGL(k_down_fused4<4>, dim3(grid), dim3(UD4_BLOCK), lds_codes, h->stream, a, d_ops2, d_oe2, (int)h->ops.size(), d_obs2, nobs2, first_slot2, first_row2);
        else if (fused_ok && h->slots_needed <= 8) hipLaunchKernelGGL(k_down_fused4<8>, dim3(grid), dim3(UD4_BLOCK), lds_codes, h->stream, a, d_ops2, d_oe2, (int)h->ops.size(), d_obs2, nobs2, first_slot2, first_row2);
        else if (fused_ok && h->slots_needed <= 16) hipLaunchKernelGGL(k_down_fused4<16>, dim3(grid), dim3(UD4_BLOCK), lds_codes, h->stream, a, d_ops2, d_oe2, (int)h->ops.size(), d_obs2, nobs2, first_slot2, first_row2);
        else hipLaunchKernelGGL(k_down_store4, dim3(grid), dim3(UD4_BLOCK), 0, h->stream, a);
        if (nni) {
            /* one up pass per group of swaps over the vectors of this chunk; the first stores the forward vectors */
            for (size_t gi = 0; gi < ng4.off.size(); gi++) {
                NniOut no;
                no.rec = b + ng4.off[gi]; no.nrec = ng4.nrec[gi]; no.store_fn = gi == 0 ? 1 : 0; no.plane = p;
                hipLaunchKernelGGL(k_up4_nni, dim3(grid), dim3(UD4_BLOCK), 0, h->stream, a, no);
                if (hipGetLastError() != hipSuccess) { h->err = "plk_nni_ll: kernel launch failed"; return PLK_E_DEVICE; }
                const int g0 = (int)gi * NNI_MAX_ROWS;
                if ((rc = nni_group_out(h, nni, g0, std::min(NNI_MAX_ROWS, nni->n - g0), n, s0, p))) return rc;
            }
            continue;
        }
        if (pl) {
            /* one up pass per PLACE_MAX_ROWS rows over the vectors of this chunk; the first stores the forward vectors */
            for (size_t gi = 0; gi < pg4.off.size(); gi++) {
                PlaceOut po = {};
                po.rec = b + pg4.off[gi]; po.nrec = pg4.nrec[gi]; po.store_fn = gi == 0 ? 1 : 0; po.EQ = (int)pl->rates.size();
                po.QP = h->d_plP; po.T = h->d_plT; po.q_codes = h->d_plcodes; po.plane = p;
                hipLaunchKernelGGL(k_up4_place, dim3(grid), dim3(UD4_BLOCK), (size_t)C * h->nchar * 4 * sizeof(double), h->stream, a, po);
                if (hipGetLastError() != hipSuccess) { h->err = "plk_place_ll: kernel launch failed"; return PLK_E_DEVICE; }
                const long g0 = (long)gi * PLACE_MAX_ROWS;
                if ((rc = place_group_out(h, pl, g0, (int)std::min<long>(PLACE_MAX_ROWS, pl->total() - g0), n, s0, p))) return rc;
            }
            continue;
        }
        if (sp) {
            /* per prune edge: the first pass stores the path plane (after the rows) and F', later passes of the edge read them */
            for (size_t gi = 0; gi < sg4.pass.size(); gi++) {
                SprOut so = sg4.out(*sp, b, gi);
                so.QP = h->d_plP; so.plane = p; so.LP = p + (size_t)sg4.rows * n;
                if ((uintptr_t)so.LP & 15) so.LP++;               /* the vectors are read as pairs of doubles: the spare double of per_site */
                hipLaunchKernelGGL(k_up4_spr, dim3(grid), dim3(UD4_BLOCK), 0, h->stream, a, so);
                if (hipGetLastError() != hipSuccess) { h->err = "plk_spr_ll: kernel launch failed"; return PLK_E_DEVICE; }
                if ((rc = spr_group_out(h, sp, sg4.pass[gi].g0, sg4.pass[gi].nrec, n, s0, p))) return rc;
            }
            continue;
        }
        if (ps) {
            const long nbatch = (n + PS4_BLOCK - 1) / PS4_BLOCK;
            const unsigned pgrid = pair_sums_grid(h, nbatch);
            if (ps->mix_D) {
                MixSensOut mo;
                mo.part = p; mo.flag = d_psflag; mo.wsite = h->d_w ? h->d_w + s0 : nullptr; mo.D = ps->mix_D;
                hipLaunchKernelGGL(k_up4_mixsens, dim3(pgrid), dim3(PS4_BLOCK), 0, h->stream, a, mo, (int)nbatch);   /* every row of part is written */
                if (hipGetLastError() != hipSuccess) { h->err = "plk_mixture_sens: kernel launch failed"; return PLK_E_DEVICE; }
                if ((rc = pair_sums_finish(h, ps, ps_rows, pgrid, mo.part, d_psflag))) return rc;
                continue;
            }
            PairSumOut o;
            o.part = p; o.flag = d_psflag; o.wsite = h->d_w ? h->d_w + s0 : nullptr; o.want_root = ps->want_root ? 1 : 0;
            HIPCHK(h, hipMemsetAsync(o.part, 0, ps_rows * pgrid * sizeof(double), h->stream));     /* masked edges: exactly 0 */
            hipLaunchKernelGGL(k_up4_pairsums, dim3(pgrid), dim3(PS4_BLOCK), 0, h->stream, a, o, (int)nbatch);
            if (hipGetLastError() != hipSuccess) { h->err = "plk_edge_pair_sums: kernel launch failed"; return PLK_E_DEVICE; }
            if ((rc = pair_sums_finish(h, ps, ps_rows, pgrid, o.part, d_psflag))) return rc;
            continue;
        }
        if (nodes4 && C == 1) hipLaunchKernelGGL(k_up4_nodes<1>, dim3(grid), dim3(UD4_BLOCK), 0, h->stream, a);
        else if (nodes4) hipLaunchKernelGGL(k_up4_nodes<4>, dim3(grid), dim3(UD4_BLOCK), 0, h->stream, a);
        else if (deriv && marg) hipLaunchKernelGGL((k_up4<true, true>), dim3(grid), dim3(UD4_BLOCK), 0, h->stream, a);
        else if (deriv && nM == 2) hipLaunchKernelGGL((k_up4<true, false, 2>), dim3(grid), dim3(UD4_BLOCK), 0, h->stream, a);
        else if (deriv && nM == 3) hipLaunchKernelGGL((k_up4<true, false, 3>), dim3(grid), dim3(UD4_BLOCK), 0, h->stream, a);
        else if (deriv && nM == 4) hipLaunchKernelGGL((k_up4<true, false, 4>), dim3(grid), dim3(UD4_BLOCK), 0, h->stream, a);
        else if (deriv) hipLaunchKernelGGL((k_up4<true, false>), dim3(grid), dim3(UD4_BLOCK), 0, h->stream, a);
        else hipLaunchKernelGGL((k_up4<false, true>), dim3(grid), dim3(UD4_BLOCK), 0, h->stream, a);
        if (hipGetLastError() != hipSuccess) { h->err = "plk_deriv/plk_marginal: kernel launch failed"; return PLK_E_DEVICE; }
        UpDownOut o;
        o.drows = dsum.size(); o.mrows = msum.size(); o.nwv = nwv; o.DV = a.DV; o.MV = a.MV; o.MVS = a.MVS;
        if ((rc = updown_chunk_out(h, o, n, s0, sums_out != nullptr, dsum.data(), msum.data(), site_out))) return rc;
    }
    return updown_finish(h, sums_out, deriv ? dsum : msum);
}

/* deriv / marginal / edge expectations for 9 <= k <= 20 with compact codes: register-resident vector kernels
 * (plk_updown_vec.h) */
static bool use_updown_vec(const plk_engine *h)
{
    return !h->opt_force_generic && h->opt_mfma == 1 && h->pat_mode == 1 && h->k >= 9 && h->k <= 20 && h->E > 0;
}

template <int K>
static void launch_updown_vec(plk_engine *h, const UpVecArgs &a, const int *d_obs, unsigned grid, bool deriv, bool marg)
{
    hipLaunchKernelGGL(k_down_vec<K>, dim3(grid), dim3(UDV_BLOCK), 0, h->stream, a, d_obs);
    if (deriv && marg) hipLaunchKernelGGL((k_up_vec<K, true, true>), dim3(grid), dim3(UDV_BLOCK), 0, h->stream, a);
    else if (deriv) hipLaunchKernelGGL((k_up_vec<K, true, false>), dim3(grid), dim3(UDV_BLOCK), 0, h->stream, a);
    else hipLaunchKernelGGL((k_up_vec<K, false, true>), dim3(grid), dim3(UDV_BLOCK), 0, h->stream, a);
}

static int run_updown_vec(plk_engine *h, bool deriv, bool marg, const int *edge_mask, const int *node_mask,
                          double *site_out, double *sums_out, const double *d_M, int dzero)
{
    int rc;
    const int N = h->N, E = h->E, k = h->k, K = h->K, C = h->C;
    const long S = h->S;
    if (h->prog_dirty) { if ((rc = build_program(h))) return rc; }
    const PlkStorageMaps sm = storage_maps(h);
    const std::vector<int> &edge_tip = sm.edge_tip, &node_int = sm.node_int, &node_scale = sm.node_scale;
    const int ntips = sm.ntips, nie = sm.nie, nin = sm.nin, nsc = sm.nsc;
    /* down-pass program and up-pass visit records + matrix list, both checked before anything is launched */
    /* nodes finished inside their parent's visit (no marginals asked for): the up pass rebuilds their L vector from the
     * tip tables, so the down pass does not store it (a third of the stored vectors at BASELINE config 4) */
    std::vector<char> skip_l(N, 0);
    const char *leaf_obs = h->node_observed.size() == (size_t)N ? h->node_observed.data() : nullptr;
    for (int u = 1; u < N; u++) { const int b = h->preorder[u]; skip_l[b] = plk_up_inlinable(h->indptr.data(), edge_tip.data(), b, marg, h->indices.data(), leaf_obs); }
    PlkChain ch;
    plk_chain_build(N, h->pg, 3, h->indices.data(), node_int.data(), nullptr, node_scale.data(), ch, skip_l.data());
    PlkUpVisits uv;
    plk_up_visits_build(N, h->indptr.data(), h->indices.data(), h->preorder.data(), h->node_has_data.data(), edge_tip.data(),
                        node_int.data(), node_scale.data(), deriv, marg, edge_mask, node_mask, uv, leaf_obs);
    {
        std::string bad = plk_chain_check(N, h->pg, ch, 3, INT_MAX, nin, nie, nsc, 0, 0);
        if (bad.empty()) bad = plk_up_visits_check(N, E, uv, nin, ntips, nsc, deriv);
        if (!bad.empty()) { h->err = "internal: " + bad; return PLK_E_ARG; }
    }
    const int nstream = (int)uv.kind.size();
    const int nslots = std::max(h->slots_needed, 1);
    /* integer tables of this call: one upload into the grow-only block */
    IntPack pack;
    const size_t o_ops = pack.put(reinterpret_cast<const int *>(ch.ops.data()), ch.ops.size() * 4);
    const size_t o_obs = pack.put(h->obs_nodes.data(), h->obs_nodes.size());
    const size_t o_vis = pack.put(uv.rec.data(), uv.rec.size());
    const size_t o_kind = pack.put(uv.kind.data(), uv.kind.size()), o_edge = pack.put(uv.edge.data(), uv.edge.size());
    const size_t o_te = pack.put(sm.tip_edges.data(), sm.tip_edges.size());
    /* the state a character code observes: its definition row is one 1.0 among zeros (leaf marginals of such codes are one
     * dot product in the up pass instead of a matrix-vector product) */
    std::vector<int> code_state((size_t)std::max(h->nchar, 1), -1);
    for (int cd = 0; cd < h->nchar && h->defs.size() == (size_t)h->nchar * k; cd++) {
        int nnz = 0, at = -1;
        for (int j = 0; j < k; j++) if (h->defs[(size_t)cd * k + j] != 0.0) { nnz++; at = j; }
        if (nnz == 1 && h->defs[(size_t)cd * k + at] == 1.0) code_state[cd] = at;
    }
    const size_t o_cs = pack.put(code_state.data(), code_state.size());
    const size_t ntab = (size_t)C * (ntips + 1) * h->nchar * K;
    const size_t nmat = (size_t)C * E * K * K + (size_t)C * (nstream + 3) * K * K;
    if ((rc = dev_reserve(h, &h->d_u4tip, &h->u4tip_cap, 2 * ntab)) ||
        (rc = dev_reserve(h, &h->d_uvmat, &h->uvmat_cap, nmat)) || (rc = pack.upload(h))) return rc;
    const int *b = h->d_u4pack;
    double *d_PT = h->d_uvmat, *d_MS = h->d_uvmat + (size_t)C * E * K * K;
    double *d_tipv = h->d_u4tip, *d_dtipv = h->d_u4tip + ntab;
    const int bt = K * K >= 256 ? 256 : 64;
    hipLaunchKernelGGL(k_build_edge_stream, dim3(C * E), dim3(bt), 0, h->stream, k, K, 0, h->d_P, d_PT);
    hipLaunchKernelGGL(k_build_up_stream, dim3(nstream + 3, C), dim3(bt), 0, h->stream, k, K, E, nstream, b + o_kind, b + o_edge,
                       h->d_P, d_M, d_MS);
    hipLaunchKernelGGL(k_build_tip_vec, dim3(ntips + 1, C), dim3(256), 0, h->stream,
                       k, K, E, ntips, h->nchar, b + o_te, h->d_Pdd, h->d_defs, d_tipv);
    hipLaunchKernelGGL(k_build_dtip_vec, dim3(ntips + 1, C), dim3(256), 0, h->stream,
                       k, K, E, ntips, h->nchar, b + o_te, d_M, h->d_defs, K, d_dtipv, dzero);
    if (hipGetLastError() != hipSuccess) { h->err = "plk_deriv/plk_marginal: table build failed"; return PLK_E_DEVICE; }

    const bool msum_only = marginal_sums_only(deriv, marg, site_out, sums_out);      /* per-wave sums instead of the N x k planes */
    const size_t per_site = ((size_t)(2 * (size_t)nin) * C * K + (size_t)nslots * K + (size_t)(nsc + 2) * C + 1 + (deriv ? E : 0) + (marg && !msum_only ? (size_t)N * k : 0)) * sizeof(double);
    long chunk;
    if ((rc = plan_site_chunk(h, "plk_deriv/plk_marginal", per_site + (msum_only ? ((size_t)N * h->k / 64 + 1) * sizeof(double) : 0), UDV_BLOCK, false, &chunk))) return rc;
    const size_t mvs_doubles = msum_only ? (size_t)N * k * (size_t)((chunk + UDV_BLOCK - 1) / UDV_BLOCK) * (UDV_BLOCK / 64) : 0;   /* per-wave marginal sums */
    if ((rc = dev_reserve(h, &h->d_work, &h->work_cap, per_site / sizeof(double) * (size_t)chunk + mvs_doubles))) return rc;

    std::vector<long double> dsum(deriv ? E : 0, 0.0L), msum(marg ? (size_t)N * k : 0, 0.0L);
    for (long s0 = 0; s0 < S; s0 += chunk) {
        const long n = std::min(chunk, S - s0);
        UpVecArgs a;
        a.S = S; a.Spad = h->Spad; a.s0 = s0; a.n = n;
        a.N = N; a.E = E; a.k = k; a.C = C; a.nchar = h->nchar; a.ntips = ntips; a.root_mode = h->root_mode; a.dzero = dzero;
        a.ops = reinterpret_cast<const int4 *>(b + o_ops); a.nops = (int)h->ops.size(); a.root_int = node_int[h->preorder[0]];
        a.first_slot = ch.first_slot; a.first_row = ch.first_row; a.second_row = ch.second_row;
        a.PT = d_PT; a.tip = d_tipv; a.dtip = d_dtipv; a.codes = h->d_codes; a.cat_prior = h->d_cat_prior; a.root_w = h->d_root_w;
        a.visits = b + o_vis; a.nvisits = uv.nvisits; a.MS = d_MS; a.nstream = nstream;
        a.reg_lo = vec_reg_window(h);
        a.code_state = b + o_cs;
        double *p = h->d_work;
        a.LN = p; p += (size_t)nin * C * K * n;
        a.FN = p; p += (size_t)nin * C * K * n;
        a.slots = p; p += (size_t)nslots * K * n;
        a.SC = p; p += (size_t)nsc * C * n;
        a.CW = p; p += (size_t)C * n;
        a.XC = p; p += (size_t)C * n;
        a.LH = p; p += n;
        a.DV = p; if (deriv) p += (size_t)E * n;
        const unsigned grid = (unsigned)((n + UDV_BLOCK - 1) / UDV_BLOCK);
        const size_t nwv = (size_t)grid * (UDV_BLOCK / 64);
        a.MV = p; a.MVS = nullptr; a.wsite = nullptr;
        if (marg && msum_only) { a.MVS = p; a.wsite = h->d_w ? h->d_w + s0 : nullptr; p += (size_t)N * k * nwv; }
        else if (marg) p += (size_t)N * k * n;
        if (deriv && edge_mask) HIPCHK(h, hipMemsetAsync(a.DV, 0, (size_t)E * n * sizeof(double), h->stream));   /* without a mask every edge's row is written by the up pass */
        if (marg) HIPCHK(h, hipMemsetAsync(a.MV, 0, (msum_only ? (size_t)N * k * nwv : (size_t)N * k * n) * sizeof(double), h->stream));
        if (K == 16) launch_updown_vec<16>(h, a, b + o_obs, grid, deriv, marg);
        else launch_updown_vec<20>(h, a, b + o_obs, grid, deriv, marg);
        if (hipGetLastError() != hipSuccess) { h->err = "plk_deriv/plk_marginal: kernel launch failed"; return PLK_E_DEVICE; }
        UpDownOut o;
        o.drows = dsum.size(); o.mrows = msum.size(); o.nwv = nwv; o.DV = a.DV; o.MV = a.MV; o.MVS = a.MVS;
        if ((rc = updown_chunk_out(h, o, n, s0, sums_out != nullptr, dsum.data(), msum.data(), site_out))) return rc;
    }
    return updown_finish(h, sums_out, deriv ? dsum : msum);
}

static bool use_updown4(const plk_engine *h)
{
    return !h->opt_force_generic && h->k == 4 && h->pat_mode == 1 && h->E > 0;
}

/* d_M: the per-(category, edge) matrices of the edge bilinear form fe^T M L_b: dP for the derivative
 * (dzero = 1: rows sum to zero), scaled Frechet matrices for dwell / trans / em-update (dzero = 0) */
static int run_updown(plk_engine *h, bool deriv, bool marg, const int *edge_mask, const int *node_mask,
                      double *site_out, double *sums_out, const double *d_M_in = nullptr, int dzero = 1, int nM = 1, PairSumReq *ps = nullptr,
                      NniReq *nni = nullptr, PlaceReq *pl = nullptr, SprReq *sp = nullptr)
{
    if (h->k == 0 || h->pat_mode == 0) { h->err = "plk_deriv/plk_marginal: tree, model and patterns must be set"; return PLK_E_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    if (h->model_dirty) { if ((rc = run_expm(h))) return rc; }
    if ((rc = check_stored_range(h, sp ? "plk_spr_ll" : pl ? "plk_place_ll" : nni ? "plk_nni_ll" : ps ? (ps->mix_D ? "plk_mixture_sens" : "plk_edge_pair_sums/plk_rate_matrix_sens")
                                       : marg ? (deriv ? "plk_deriv/plk_marginal" : "plk_marginal") : d_M_in ? "plk_edge_expect" : "plk_deriv"))) return rc;
    if (!d_M_in && !ps && !nni && !pl && !sp && (rc = ensure_dP(h))) return rc;
    const double *d_M = d_M_in ? d_M_in : h->d_dP;
    if (!ps && !nni && !pl && !sp) h->info_up4_path = 0;
    if (sp) {
        /* the k = 4 kernel takes compact codes and at most four categories, as for the placements */
        if ((rc = call_matrices(h, sp->rates))) return rc;
        if (use_updown4(h) && h->C <= 4) { h->info_spr_kernel = 1; return run_updown4(h, false, false, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, sp); }
        h->info_spr_kernel = 2;
    } else
    if (pl) {
        /* the k = 4 kernel takes compact codes and at most four categories, as for the swaps */
        if ((rc = place_matrices(h, *pl))) return rc;
        if (use_updown4(h) && h->C <= 4) { h->info_place_kernel = 1; return run_updown4(h, false, false, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, pl); }
        h->info_place_kernel = 2;
    } else
    if (nni) {
        /* as for the pair sums: the k = 4 kernel takes compact codes and at most four categories */
        if (use_updown4(h) && h->C <= 4) { h->info_nni_kernel = 1; return run_updown4(h, false, false, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nni); }
        h->info_nni_kernel = 2;
    } else
    if (ps) {
        /* the k = 4 kernel takes compact codes and at most four categories; everything else the generic kernel below */
        long &info = ps->mix_D ? h->info_mixture_sens_kernel : h->info_pair_sums_kernel;
        if (use_updown4(h) && h->C <= 4) { info = 1; return run_updown4(h, false, false, edge_mask, nullptr, nullptr, nullptr, nullptr, 0, 0, ps); }
        info = 2;
    } else
    if (use_updown_vec(h) && nM == 1) { h->info_updown_kernel = 4; return run_updown_vec(h, deriv, marg, edge_mask, node_mask, site_out, sums_out, d_M, dzero); }
    else if (use_mfma(h)) { h->info_updown_kernel = 3; return run_updown_mfma(h, deriv, marg, edge_mask, node_mask, site_out, sums_out, d_M, dzero); }
    else if (use_updown4(h)) { h->info_updown_kernel = 1; return run_updown4(h, deriv, marg, edge_mask, node_mask, site_out, sums_out, d_M, dzero, nM); }
    if (nM != 1) { h->err = "internal: several edge forms per pass need the k = 4 kernels"; return PLK_E_ARG; }
    if (!ps && !nni && !pl && !sp) h->info_updown_kernel = 2;
    const int N = h->N, E = h->E, k = h->k, K = h->K, C = h->C;
    const long S = h->S;
    /* padded edge-indexed streams in the grow-only matrix buffer; each starts at a multiple of 32 doubles (256 bytes, what
     * an allocation of its own would give it), also when K K C E is odd */
    const size_t strm = ((size_t)C * E * K * K + 31) / 32 * 32;
    if ((rc = dev_reserve(h, &h->d_uvmat, &h->uvmat_cap, 3 * strm))) return rc;
    double *d_PT = h->d_uvmat, *d_PN = d_PT + strm, *d_DT = d_PN + strm;
    const int bt = K * K >= 256 ? 256 : 64;
    hipLaunchKernelGGL(k_build_edge_stream, dim3(C * E), dim3(bt), 0, h->stream, k, K, 0, h->d_P, d_PT);
    hipLaunchKernelGGL(k_build_edge_stream, dim3(C * E), dim3(bt), 0, h->stream, k, K, 1, h->d_P, d_PN);
    if (!nni && !pl && !sp && (!ps || ps->mix_D)) hipLaunchKernelGGL(k_build_edge_stream, dim3(C * E), dim3(bt), 0, h->stream, k, K, 0, ps ? ps->mix_D : d_M, d_DT);
    /* the call's integer tables; of the storage maps the generic kernels take the rescaling slots only */
    if (h->prog_dirty) { if ((rc = build_program(h))) return rc; }
    const PlkStorageMaps sm = storage_maps(h);
    const int nsc = sm.nsc;
    IntPack pack;
    const size_t o_em = pack.put_opt(edge_mask, (size_t)E), o_nm = pack.put_opt(node_mask, (size_t)N);
    const size_t o_has = pack.put_has_data(h), o_ns = pack.put(sm.node_scale.data(), (size_t)N);
    NniGroups ngg;
    if (nni) ngg.put(h, *nni, false, pack);
    PlaceGroups pgg;
    if (pl) pgg.put(*pl, pack);
    SprGroups sgg;
    if (sp) sgg.put(*sp, pack);
    if ((rc = pack.upload(h))) return rc;
    const int EQ = pl ? (int)pl->rates.size() : sp ? (int)sp->rates.size() : 0;
    const size_t qstrm = ((size_t)C * EQ * K * K + 31) / 32 * 32;
    if (pl) {
        /* the call's matrices as padded streams (transposed, plain) and, for compact codes, the pendant tables [C][nchar][K] */
        if ((rc = dev_reserve(h, &h->d_plstream, &h->plstream_cap, 2 * qstrm)) ||
            (rc = dev_reserve(h, &h->d_plT, &h->plt_cap, (size_t)C * std::max(h->nchar, 1) * K))) return rc;
        hipLaunchKernelGGL(k_build_edge_stream, dim3(C * EQ), dim3(bt), 0, h->stream, k, K, 0, h->d_plP, h->d_plstream);
        hipLaunchKernelGGL(k_build_edge_stream, dim3(C * EQ), dim3(bt), 0, h->stream, k, K, 1, h->d_plP, h->d_plstream + qstrm);
        if (pl->compact) hipLaunchKernelGGL(k_place_table, dim3(C), dim3(256), 0, h->stream, k, K, EQ, h->nchar, h->d_plstream, h->d_defs, h->d_plT);
        if (hipGetLastError() != hipSuccess) { h->err = "plk_place_ll: table build failed"; return PLK_E_DEVICE; }
    }
    if (sp) {
        /* the call's matrices as padded streams (transposed, plain) */
        if ((rc = dev_reserve(h, &h->d_plstream, &h->plstream_cap, 2 * qstrm))) return rc;
        hipLaunchKernelGGL(k_build_edge_stream, dim3(C * EQ), dim3(bt), 0, h->stream, k, K, 0, h->d_plP, h->d_plstream);
        hipLaunchKernelGGL(k_build_edge_stream, dim3(C * EQ), dim3(bt), 0, h->stream, k, K, 1, h->d_plP, h->d_plstream + qstrm);
        if (hipGetLastError() != hipSuccess) { h->err = "plk_spr_ll: stream build failed"; return PLK_E_DEVICE; }
    }
    const int *pk = h->d_u4pack;
    const int *d_emask = edge_mask ? pk + o_em : nullptr, *d_nmask = node_mask ? pk + o_nm : nullptr, *d_has = pk + o_has, *d_ns = pk + o_ns;
    int *const d_psflag = pack.flag(h);

    /* chunk the site axis so that the stored vectors fit */
    const size_t per_site = ((size_t)(E + 2 * (size_t)N) * C * k + (size_t)(nsc + 2) * C + 1 + (deriv ? E : 0) + (marg ? (size_t)N * k : 0) + (size_t)ngg.rows +
                             (pl ? (size_t)pgg.rows + (size_t)C * k + C : 0) + (sp ? (size_t)sgg.rows + (size_t)(sp->max_depth + 1) * C * k : 0)) * sizeof(double);
    long chunk;
    if ((rc = plan_site_chunk(h, "plk_deriv/plk_marginal", per_site, GEN_BLOCK, false, &chunk))) return rc;
    const size_t ps_rows = ps ? (ps->mix_D ? (size_t)2 * C : (size_t)C * E * k * k + (size_t)C * k) : 0;
    const size_t ps_doubles = ps ? ps_rows * pair_sums_grid(h, (chunk + GEN_BLOCK - 1) / GEN_BLOCK) : 0;
    if ((rc = dev_reserve(h, &h->d_work, &h->work_cap, per_site / sizeof(double) * (size_t)chunk + ps_doubles))) return rc;
    if (ps) {
        ps->acc.assign(ps_rows, 0.0L);
        HIPCHK(h, hipMemsetAsync(d_psflag, 0, sizeof(int), h->stream));
    }

    std::vector<long double> dsum(deriv ? E : 0, 0.0L), msum(marg ? (size_t)N * k : 0, 0.0L);
    for (long s0 = 0; s0 < S; s0 += chunk) {
        const long n = std::min(chunk, S - s0);
        UpArgs a;
        a.S = S; a.Spad = h->Spad; a.s0 = s0; a.n = n;
        a.N = N; a.E = E; a.k = k; a.C = C; a.nchar = h->nchar; a.pat_mode = h->pat_mode; a.root_mode = h->root_mode;
        a.dzero = dzero;
        a.mod_edge = -1; a.DN = nullptr; a.D2T = nullptr; a.LHdiv = nullptr; a.XM = nullptr; a.XMdiv = nullptr;
        a.node_scale = d_ns;
        a.indptr = h->d_indptr; a.indices = h->d_indices; a.preorder = h->d_preorder; a.node_has_data = d_has;
        a.PT = d_PT; a.PN = d_PN; a.DT = d_DT; a.codes = h->d_codes; a.defs = h->d_defs; a.B = h->d_B;
        a.cat_prior = h->d_cat_prior; a.root_w = h->d_root_w; a.edge_mask = d_emask; a.node_mask = d_nmask;
        double *p = h->d_work;
        a.EV = p; p += (size_t)E * C * k * n;
        a.LN = p; p += (size_t)N * C * k * n;
        a.FN = p; p += (size_t)N * C * k * n;
        a.SC = p; p += (size_t)nsc * C * n;
        a.CW = p; p += (size_t)C * n;
        a.XC = p; p += (size_t)C * n;
        a.LH = p; p += n;
        a.DV = p; if (deriv) p += (size_t)E * n;
        a.MV = p; if (marg) p += (size_t)N * k * n;
        if (deriv) HIPCHK(h, hipMemsetAsync(a.DV, 0, (size_t)E * n * sizeof(double), h->stream));
        if (marg) HIPCHK(h, hipMemsetAsync(a.MV, 0, (size_t)N * k * n * sizeof(double), h->stream));
        const unsigned grid = (unsigned)((n + GEN_BLOCK - 1) / GEN_BLOCK);
        if (nni) {
            for (size_t gi = 0; gi < ngg.off.size(); gi++) {
                NniOut no;
                no.rec = pk + ngg.off[gi]; no.nrec = ngg.nrec[gi]; no.store_fn = gi == 0 ? 1 : 0; no.plane = p;
                dispatch_K(K, [&](auto Kc) { launch_nni<decltype(Kc)::value>(h, a, no, grid, gi == 0); });
                if (hipGetLastError() != hipSuccess) { h->err = "plk_nni_ll: kernel launch failed"; return PLK_E_DEVICE; }
                const int g0 = (int)gi * NNI_MAX_ROWS;
                if ((rc = nni_group_out(h, nni, g0, std::min(NNI_MAX_ROWS, nni->n - g0), n, s0, p))) return rc;
            }
            continue;
        }
        if (pl) {
            /* down pass and forward vectors once per chunk (k_up_nni's FORWARD instantiation), then one pass per PLACE_MAX_ROWS rows */
            for (size_t gi = 0; gi < pgg.off.size(); gi++) {
                PlaceOut po = {};
                po.rec = pk + pgg.off[gi]; po.nrec = pgg.nrec[gi]; po.store_fn = gi == 0 ? 1 : 0; po.EQ = EQ;
                po.QPT = h->d_plstream; po.QPN = h->d_plstream + qstrm; po.T = h->d_plT;
                po.q_codes = pl->compact ? h->d_plcodes : nullptr; po.q_dense = pl->compact ? nullptr : h->d_pldense;
                po.plane = p; po.WS = p + (size_t)pgg.rows * n; po.XW = po.WS + (size_t)C * k * n;
                dispatch_K(K, [&](auto Kc) { launch_place<decltype(Kc)::value>(h, a, po, grid, gi == 0); });
                if (hipGetLastError() != hipSuccess) { h->err = "plk_place_ll: kernel launch failed"; return PLK_E_DEVICE; }
                const long g0 = (long)gi * PLACE_MAX_ROWS;
                if ((rc = place_group_out(h, pl, g0, (int)std::min<long>(PLACE_MAX_ROWS, pl->total() - g0), n, s0, p))) return rc;
            }
            continue;
        }
        if (sp) {
            /* the down pass once per chunk; per prune edge the path plane and F' once, then one pass per PLACE_MAX_ROWS moves */
            for (size_t gi = 0; gi < sgg.pass.size(); gi++) {
                SprOut so = sgg.out(*sp, pk, gi);
                so.QPT = h->d_plstream; so.QPN = h->d_plstream + qstrm; so.plane = p; so.LP = p + (size_t)sgg.rows * n;
                dispatch_K(K, [&](auto Kc) { launch_spr<decltype(Kc)::value>(h, a, so, grid, gi == 0); });
                if (hipGetLastError() != hipSuccess) { h->err = "plk_spr_ll: kernel launch failed"; return PLK_E_DEVICE; }
                if ((rc = spr_group_out(h, sp, sgg.pass[gi].g0, sgg.pass[gi].nrec, n, s0, p))) return rc;
            }
            continue;
        }
        if (ps) {
            const unsigned pgrid = pair_sums_grid(h, (long)grid);
            if (ps->mix_D) {
                MixSensOut mo;
                mo.part = p; mo.flag = d_psflag; mo.wsite = h->d_w ? h->d_w + s0 : nullptr; mo.D = nullptr;
                dispatch_K(K, [&](auto Kc) { launch_mixsens<decltype(Kc)::value>(h, a, mo, grid, pgrid); });
                if (hipGetLastError() != hipSuccess) { h->err = "plk_mixture_sens: kernel launch failed"; return PLK_E_DEVICE; }
                if ((rc = pair_sums_finish(h, ps, ps_rows, pgrid, mo.part, d_psflag))) return rc;
                continue;
            }
            PairSumOut o;
            o.part = p; o.flag = d_psflag; o.wsite = h->d_w ? h->d_w + s0 : nullptr; o.want_root = ps->want_root ? 1 : 0;
            HIPCHK(h, hipMemsetAsync(o.part, 0, ps_rows * pgrid * sizeof(double), h->stream));     /* masked edges: exactly 0 */
            dispatch_K(K, [&](auto Kc) { launch_pairsums<decltype(Kc)::value>(h, a, o, grid, pgrid); });
            if (hipGetLastError() != hipSuccess) { h->err = "plk_edge_pair_sums: kernel launch failed"; return PLK_E_DEVICE; }
            if ((rc = pair_sums_finish(h, ps, ps_rows, pgrid, o.part, d_psflag))) return rc;
            continue;
        }
        dispatch_K(K, [&](auto Kc) { launch_updown<decltype(Kc)::value>(h, a, grid, deriv, marg); });
        if (hipGetLastError() != hipSuccess) { h->err = "plk_deriv/plk_marginal: kernel launch failed"; return PLK_E_DEVICE; }
        UpDownOut o;
        o.drows = dsum.size(); o.mrows = msum.size(); o.DV = a.DV; o.MV = a.MV;
        if ((rc = updown_chunk_out(h, o, n, s0, sums_out != nullptr, dsum.data(), msum.data(), site_out))) return rc;
    }
    return updown_finish(h, sums_out, deriv ? dsum : msum);
}

/* ====================================================================== */
/* X1: the reduction step over ranks on RCCL (one process per GPU)         */
/* ====================================================================== */

extern "C" int plk_comm_available(void) { return rccl_load() ? 1 : 0; }

extern "C" int plk_comm_unique_id(unsigned char id_out[128])
{
    if (!id_out) return PLK_E_ARG;
    if (!rccl_load()) { g_create_error = g_rccl.err; return PLK_E_UNSUPPORTED; }
    PlkNcclId id;
    const int rc = g_rccl.GetUniqueId(&id);
    if (rc) { g_create_error = "ncclGetUniqueId: " + rccl_text(rc); return PLK_E_DEVICE; }
    memcpy(id_out, id.internal, 128);
    return PLK_OK;
}

extern "C" int plk_comm_init(plk_engine *h, int nranks, int rank, const unsigned char id[128])
{
    if (!plk_live(h) || !id || nranks < 1 || rank < 0 || rank >= nranks) return PLK_E_ARG;
    if (!rccl_load()) { h->err = g_rccl.err; return PLK_E_UNSUPPORTED; }
    HIPCHK(h, hipSetDevice(h->device));
    if (h->comm) { (void)g_rccl.CommDestroy(h->comm); h->comm = nullptr; }
    PlkNcclId nid;
    memcpy(nid.internal, id, 128);
    const int rc = g_rccl.CommInitRank(&h->comm, nranks, nid, rank);
    if (rc) { h->comm = nullptr; h->err = "ncclCommInitRank: " + rccl_text(rc); return PLK_E_DEVICE; }
    h->comm_ranks = nranks;
    return PLK_OK;
}

extern "C" int plk_allreduce_sum_async(plk_engine *h, double *dev, long count)
{
    if (!plk_live(h) || !dev || count < 1) return PLK_E_ARG;
    if (!h->comm) { h->err = "plk_allreduce_sum_async: plk_comm_init first"; return PLK_E_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    const int rc = g_rccl.AllReduce(dev, dev, (size_t)count, /* ncclDouble */ 8, /* ncclSum */ 0, h->comm, h->stream);
    if (rc) { h->err = "ncclAllReduce: " + rccl_text(rc); return PLK_E_DEVICE; }
    return PLK_OK;
}

extern "C" int plk_comm_destroy(plk_engine *h)
{
    if (!plk_live(h)) return PLK_E_ARG;
    if (h->comm) {
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream);
        (void)g_rccl.CommDestroy(h->comm);
        h->comm = nullptr;
    }
    return PLK_OK;
}

/* HIP events around everything a query queues (PLK_INFO_LAST_QUERY_NS); the events are made on first use */
struct QueryTimer {
    plk_engine *h;
    bool on = false;
    explicit QueryTimer(plk_engine *h_) : h(h_)
    {
        if (hipSetDevice(h->device) != hipSuccess) return;
        if (!h->q_ev0 && (hipEventCreate(&h->q_ev0) != hipSuccess || hipEventCreate(&h->q_ev1) != hipSuccess)) { h->q_ev0 = h->q_ev1 = nullptr; return; }
        on = hipEventRecord(h->q_ev0, h->stream) == hipSuccess;
    }
    ~QueryTimer()
    {
        h->info_query_ns = 0;
        if (!on) return;
        float ms = 0.f;
        if (hipEventRecord(h->q_ev1, h->stream) == hipSuccess && hipEventSynchronize(h->q_ev1) == hipSuccess &&
            hipEventElapsedTime(&ms, h->q_ev0, h->q_ev1) == hipSuccess) h->info_query_ns = (long)(ms * 1e6);
    }
};

extern "C" int plk_deriv(plk_engine *h, const int *edge_mask, double *site_edge_out, double *edge_sums_out)
{
    if (!plk_live(h)) return PLK_E_ARG;
    QueryTimer qt(h);
    return run_updown(h, true, false, edge_mask, nullptr, site_edge_out, edge_sums_out);
}

/* Several direction matrices at once: the k = 4 kernels carry up to four edge forms per pass (one down pass, one
 * up pass, shared forward vectors); other state counts run one pass per direction.
 * site_out: NULL or [S][nL][E]; sums_out: NULL or [nL][E][2]. */
extern "C" int plk_edge_expect_multi(plk_engine *h, int nL, const double *L_hi, const double *L_lo, int coef_mode,
                                     const int *edge_mask, double *site_out, double *sums_out)
{
    if (!plk_live(h)) return PLK_E_ARG;
    if (h->k == 0 || h->pat_mode == 0) { h->err = "plk_edge_expect: tree, model and patterns must be set"; return PLK_E_ARG; }
    if (!L_hi || nL < 1 || coef_mode < PLK_COEF_PRIOR || coef_mode > PLK_COEF_PRIOR_RATE) { h->err = "plk_edge_expect: bad direction matrix or coefficient mode"; return PLK_E_ARG; }
    { int rcL = k1_check_direction(h, "plk_edge_expect", nL, L_hi, L_lo); if (rcL) return rcL; }
    HIPCHK(h, hipSetDevice(h->device));
    QueryTimer qt(h);
    int rc;
    if (h->model_dirty) { if ((rc = run_expm(h))) return rc; }
    const int k = h->k, C = h->C, E = h->E;
    const long S = h->S;
    if (E == 0) return PLK_OK;
    const size_t kk = (size_t)k * k, n2 = 4 * kk;
    /* how many directions one pass of the kernels can carry */
    const int per_pass = use_updown4(h) && !use_mfma(h) ? 4 : 1;
    /* everything below lives in grow-only engine buffers: no per-call hipMalloc / hipFree */
    const int threads = n2 >= 1024 ? 1024 : (n2 >= 256 ? 256 : 64);
    int use_lds;
    const size_t lds_bytes = expm_lds_bytes((size_t)2 * k, threads, &use_lds);
    if ((rc = dev_reserve(h, &h->d_exL, &h->exL_cap, (size_t)per_pass * 2 * kk)) ||
        (rc = dev_reserve(h, &h->d_exF, &h->exF_cap, (size_t)per_pass * C * E * kk)) ||
        (rc = dev_reserve(h, &h->d_exmask, &h->exmask_cap, (size_t)E)) ||
        (!use_lds && (rc = dev_reserve(h, &h->d_exscr, &h->exscr_cap, (size_t)C * E * EXPM_BUFFERS * n2)))) return rc;
    double *d_L = h->d_exL, *d_F = h->d_exF;
    int *d_mask = nullptr;
    dd *d_scr = h->d_exscr;
    if (edge_mask) {
        HIPCHK(h, hipMemcpyAsync(h->d_exmask, edge_mask, (size_t)E * sizeof(int), hipMemcpyHostToDevice, h->stream));
        d_mask = h->d_exmask;
    }
    std::vector<double> L((size_t)per_pass * 2 * kk), tmp_site, tmp_sums;
    for (int m0 = 0; m0 < nL; m0 += per_pass) {
        const int nm = std::min(per_pass, nL - m0);
        for (int m = 0; m < nm; m++) {
            double *Lm = L.data() + (size_t)m * 2 * kk;
            std::copy(L_hi + (size_t)(m0 + m) * kk, L_hi + (size_t)(m0 + m + 1) * kk, Lm);
            if (L_lo) std::copy(L_lo + (size_t)(m0 + m) * kk, L_lo + (size_t)(m0 + m + 1) * kk, Lm + kk);
            else std::fill(Lm + kk, Lm + 2 * kk, 0.0);
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));          /* the previous pass may still read d_L */
        HIPCHK(h, hipMemcpyAsync(d_L, L.data(), (size_t)nm * 2 * kk * sizeof(double), hipMemcpyHostToDevice, h->stream));
        for (int m = 0; m < nm; m++) {
            hipLaunchKernelGGL(k_expm_dd<true>, dim3(C * E), dim3(threads), lds_bytes, h->stream,
                               k, E, h->d_Qn, h->d_edge_rates, h->d_cat_rates, (dd *)nullptr, (double *)nullptr, (double *)nullptr,
                               d_scr, use_lds, d_L + (size_t)m * 2 * kk, 0L, coef_mode, d_mask, d_F + (size_t)m * C * E * kk, ExpmPost{});
        }
        if (hipGetLastError() != hipSuccess) { h->err = "plk_edge_expect: Frechet kernel launch failed"; return PLK_E_DEVICE; }
        HIPCHK(h, hipStreamSynchronize(h->stream));          /* L is a host local */
        /* outputs of this pass: [S][nm*E] and [nm*E][2]; scattered into [S][nL*E] / [nL*E][2] */
        double *so = nullptr, *su = nullptr;
        if (site_out) { if (nm == nL) so = site_out; else { tmp_site.assign((size_t)S * nm * E, 0.0); so = tmp_site.data(); } }
        if (sums_out) su = sums_out + (size_t)m0 * E * 2;
        rc = run_updown(h, true, false, edge_mask, nullptr, so, su, d_F, 0, nm);
        if (rc) return rc;
        if (site_out && nm != nL)
            for (long s = 0; s < S; s++)
                for (int r = 0; r < nm * E; r++)
                    site_out[((size_t)s * nL + m0) * E + r] = tmp_site[(size_t)s * nm * E + r];
    }
    return PLK_OK;
}

/* Conditional edge expectations (dwell / trans / em-update numerators): replaces
 * src/evaluate_site_frechet.c:5-42 + the Frechet matrix set-up of src/arbplfdwell.c:117-204,
 * src/arbplftrans.c:116-224, src/arbplfem.c:100-158. */
extern "C" int plk_edge_expect(plk_engine *h, const double *L_hi, const double *L_lo, int coef_mode,
                               const int *edge_mask, double *site_edge_out, double *edge_sums_out)
{
    return plk_edge_expect_multi(h, 1, L_hi, L_lo, coef_mode, edge_mask, site_edge_out, edge_sums_out);
}

extern "C" int plk_get_frechet_matrices(plk_engine *h, const double *L_hi, const double *L_lo, int coef_mode, double *F_out)
{
    if (!plk_live(h) || !L_hi || !F_out) return PLK_E_ARG;
    if (h->k == 0) { h->err = "plk_get_frechet_matrices: model must be set"; return PLK_E_ARG; }
    if (coef_mode < PLK_COEF_PRIOR || coef_mode > PLK_COEF_PRIOR_RATE) { h->err = "plk_get_frechet_matrices: bad coefficient mode"; return PLK_E_ARG; }
    { int rcL = k1_check_direction(h, "plk_get_frechet_matrices", 1, L_hi, L_lo); if (rcL) return rcL; }
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    if (h->model_dirty) { if ((rc = run_expm(h))) return rc; }
    const int k = h->k, C = h->C, E = h->E;
    if (E == 0) return PLK_OK;
    const size_t kk = (size_t)k * k, n2 = 4 * kk;
    std::vector<double> L(2 * kk, 0.0);
    std::copy(L_hi, L_hi + kk, L.begin());
    if (L_lo) std::copy(L_lo, L_lo + kk, L.begin() + kk);
    double *d_L = nullptr, *d_F = nullptr;
    dd *d_scr = nullptr;
    auto cleanup = [&]() {
        if (d_L) (void)hipFree(d_L);
        if (d_F) (void)hipFree(d_F);
        if (d_scr) (void)hipFree(d_scr);
    };
    if ((rc = dev_upload(h, &d_L, L.data(), L.size())) || (rc = dev_alloc(h, &d_F, (size_t)C * E * kk))) { cleanup(); return rc; }
    const int threads = n2 >= 1024 ? 1024 : (n2 >= 256 ? 256 : 64);
    int use_lds;
    const size_t lds_bytes = expm_lds_bytes((size_t)2 * k, threads, &use_lds);
    if (!use_lds && (rc = dev_alloc(h, &d_scr, (size_t)C * E * EXPM_BUFFERS * n2))) { cleanup(); return rc; }
    hipLaunchKernelGGL(k_expm_dd<true>, dim3(C * E), dim3(threads), lds_bytes, h->stream,
                       k, E, h->d_Qn, h->d_edge_rates, h->d_cat_rates, (dd *)nullptr, (double *)nullptr, (double *)nullptr,
                       d_scr, use_lds, d_L, 0L, coef_mode, (const int *)nullptr, d_F, ExpmPost{});
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(F_out, d_F, (size_t)C * E * kk * sizeof(double), hipMemcpyDeviceToHost);
    cleanup();
    if (e != hipSuccess) { h->err = std::string("plk_get_frechet_matrices: ") + hipGetErrorString(e); return PLK_E_DEVICE; }
    return PLK_OK;
}

/* ---------------------------------------------------------------------- */
/* edge pair sums and the gradient in the rate matrix (plk_pairsums.h)     */
/* ---------------------------------------------------------------------- */

static int pair_sums_run(plk_engine *h, const int *edge_mask, PairSumReq &ps, const char *who)
{
    if (h->k == 0 || h->pat_mode == 0) { h->err = std::string(who) + ": tree, model and patterns must be set"; return PLK_E_ARG; }
    if (h->E == 0) { h->err = std::string(who) + ": the tree has no edge"; return PLK_E_ARG; }
    const int rc = run_updown(h, false, false, edge_mask, nullptr, nullptr, nullptr, nullptr, 1, 1, &ps);
    if (rc) return rc;
    if (ps.zero_lh) { h->err = std::string(who) + ": site likelihood zero at a site of non-zero weight, the sums are undefined"; return PLK_E_ARG; }
    return PLK_OK;
}

extern "C" int plk_edge_pair_sums(plk_engine *h, const int *edge_mask, double *W_out, double *root_out)
{
    if (!plk_live(h)) return PLK_E_ARG;
    if (!W_out) { h->err = "plk_edge_pair_sums: no output buffer"; return PLK_E_ARG; }
    QueryTimer qt(h);
    PairSumReq ps;
    ps.want_root = root_out != nullptr;
    int rc;
    if ((rc = pair_sums_run(h, edge_mask, ps, "plk_edge_pair_sums"))) return rc;
    const size_t nW = (size_t)h->C * h->E * h->k * h->k;
    put_dd_rows(W_out, ps.acc.data(), nW);
    if (root_out) put_dd_rows(root_out, ps.acc.data() + nW, (size_t)h->C * h->k);
    return PLK_OK;
}

/*
 * G[i][j] = d(sum_s w_s ll_s) / dQn[i][j] = sum_{c,e} <W[c][e], s F_{c,e}(e_i e_j^T)>, s = r_c t_e.  The Frechet
 * derivative is self-adjoint under the trace pairing up to transposition, <W, F(L)> = <L, F(W^T)^T>, so one Frechet
 * run per (category, edge) in direction W[c][e]^T gives all k^2 entries: G = sum_{c,e} s F_{c,e}(W[c][e]^T)^T.
 * K1 takes its scaling-and-squaring count from the norm of the block matrix [[sQ, L], [0, sQ]] and W grows with the sum
 * of the weights, so every direction is scaled by an exact power of two to infinity norm <= 1 (F is linear in L) and the
 * factor is put back on the result.  The sum over (c, e) runs on the host in long double, in (c, e) order.
 */
extern "C" int plk_rate_matrix_sens(plk_engine *h, double *G_out, double *root_out)
{
    if (!plk_live(h)) return PLK_E_ARG;
    if (!G_out) { h->err = "plk_rate_matrix_sens: no output buffer"; return PLK_E_ARG; }
    QueryTimer qt(h);
    PairSumReq ps;
    ps.want_root = root_out != nullptr;
    int rc;
    if ((rc = pair_sums_run(h, nullptr, ps, "plk_rate_matrix_sens"))) return rc;
    const int k = h->k, C = h->C, E = h->E;
    const size_t kk = (size_t)k * k, n2 = 4 * kk, CE = (size_t)C * E;
    std::vector<double> L(CE * 2 * kk);
    std::vector<int> expo(CE, 0);
    for (size_t ce = 0; ce < CE; ce++) {
        const long double *Wm = ps.acc.data() + ce * kk;
        long double norm = 0;
        for (int i = 0; i < k; i++) {          /* row i of W^T = column i of W */
            long double row = 0;
            for (int j = 0; j < k; j++) row += fabsl(Wm[(size_t)j * k + i]);
            norm = std::max(norm, row);
        }
        if (!(norm < INFINITY)) { h->err = "plk_rate_matrix_sens: the pair sums are not finite"; return PLK_E_ARG; }
        int e = 0;
        if (norm > 0) (void)frexpl(norm, &e);   /* norm = m 2^e, m in [0.5, 1) */
        expo[ce] = e;
        double *hi = L.data() + ce * 2 * kk, *lo = hi + kk;
        for (int i = 0; i < k; i++)
            for (int j = 0; j < k; j++) {
                const long double v = ldexpl(Wm[(size_t)j * k + i], -e);
                hi[(size_t)i * k + j] = (double)v;
                lo[(size_t)i * k + j] = (double)(v - (long double)hi[(size_t)i * k + j]);
            }
    }
    const int threads = n2 >= 1024 ? 1024 : (n2 >= 256 ? 256 : 64);
    int use_lds;
    const size_t lds_bytes = expm_lds_bytes((size_t)2 * k, threads, &use_lds);
    if ((rc = dev_reserve(h, &h->d_exL, &h->exL_cap, CE * 2 * kk)) ||
        (rc = dev_reserve(h, &h->d_exF, &h->exF_cap, CE * kk)) ||
        (!use_lds && (rc = dev_reserve(h, &h->d_exscr, &h->exscr_cap, CE * EXPM_BUFFERS * n2)))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_exL, L.data(), L.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_expm_dd<true>, dim3(C * E), dim3(threads), lds_bytes, h->stream,
                       k, E, h->d_Qn, h->d_edge_rates, h->d_cat_rates, (dd *)nullptr, (double *)nullptr, (double *)nullptr,
                       h->d_exscr, use_lds, h->d_exL, (long)(2 * kk), (int)PLK_COEF_PRIOR_RATE_EDGE, (const int *)nullptr, h->d_exF, ExpmPost{});
    if (hipGetLastError() != hipSuccess) { h->err = "plk_rate_matrix_sens: Frechet kernel launch failed"; return PLK_E_DEVICE; }
    std::vector<double> F(CE * kk);
    HIPCHK(h, hipMemcpyAsync(F.data(), h->d_exF, F.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<long double> G(kk, 0.0L);
    for (size_t ce = 0; ce < CE; ce++)
        for (int i = 0; i < k; i++)
            for (int j = 0; j < k; j++) G[(size_t)i * k + j] += ldexpl((long double)F[ce * kk + (size_t)j * k + i], expo[ce]);
    put_dd_rows(G_out, G.data(), kk);
    if (root_out) {
        const size_t nW = CE * kk;
        for (int i = 0; i < k; i++) {
            long double acc = 0;
            for (int c = 0; c < C; c++) acc += ps.acc[nW + (size_t)c * k + i];
            put_dd(root_out + 2 * i, acc);
        }
    }
    return PLK_OK;
}

/*
 * Gradient of sum_s w_s ll_s in the priors and rates of the rate mixture (plk_mixsens.h).  The direction matrices
 * D[c][e] = t_e Qn P[c][e] live in a buffer of the query's own and are rebuilt on every call from the stored
 * double-double P (C E small products), so nothing another query caches is read stale or overwritten.
 */
extern "C" int plk_mixture_sens(plk_engine *h, double *prior_out, double *rate_out)
{
    if (!plk_live(h)) return PLK_E_ARG;
    if (!prior_out || !rate_out) { h->err = "plk_mixture_sens: no output buffer"; return PLK_E_ARG; }
    if (h->k == 0 || h->pat_mode == 0) { h->err = "plk_mixture_sens: tree, model and patterns must be set"; return PLK_E_ARG; }
    if (h->E == 0) { h->err = "plk_mixture_sens: the tree has no edge"; return PLK_E_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    QueryTimer qt(h);
    int rc;
    if (h->model_dirty) { if ((rc = run_expm(h))) return rc; }
    const int k = h->k, C = h->C, E = h->E;
    const size_t kk = (size_t)k * k;
    if ((rc = dev_reserve(h, &h->d_mixD, &h->mixd_cap, (size_t)C * E * kk))) return rc;
    {
        const int threads = kk >= 1024 ? 1024 : (kk >= 256 ? 256 : 64);
        int use_lds;
        const size_t strip_bytes = expm_lds_bytes((size_t)k, threads, &use_lds);
        hipLaunchKernelGGL(k_mix_dir, dim3(C * E), dim3(threads), use_lds ? 0 : strip_bytes, h->stream,
                           k, E, h->d_Qn, h->d_edge_rates, h->d_Pdd, h->d_mixD, use_lds ? 0 : 1);
        if (hipGetLastError() != hipSuccess) { h->err = "plk_mixture_sens: direction matrix kernel launch failed"; return PLK_E_DEVICE; }
    }
    PairSumReq ps;
    ps.mix_D = h->d_mixD;
    if ((rc = pair_sums_run(h, nullptr, ps, "plk_mixture_sens"))) return rc;
    const size_t rate_row0 = h->info_mixture_sens_kernel == 1 ? (size_t)MIX4_MAX_C : (size_t)C;
    for (int c = 0; c < C; c++) {
        put_dd(prior_out + 2 * c, ps.acc[c]);
        put_dd(rate_out + 2 * c, ps.acc[rate_row0 + c]);
    }
    return PLK_OK;
}

/*
 * Log likelihood of nearest-neighbour interchanges of the current tree (plk_nni.h): one down pass per site chunk, one up
 * pass per group of NNI_MAX_ROWS swaps.  Every pair is checked before anything is queued.
 */
extern "C" int plk_nni_ll(plk_engine *h, int n_swaps, const int *swaps, double *site_out, double *sums_out)
{
    if (!plk_live(h)) return PLK_E_ARG;
    if (h->k == 0 || h->pat_mode == 0) { h->err = "plk_nni_ll: tree, model and patterns must be set"; return PLK_E_ARG; }
    if (n_swaps < 0) { h->err = "plk_nni_ll: negative number of swaps"; return PLK_E_ARG; }
    const int N = h->N;
    const int *ip = h->indptr.data(), *ix = h->indices.data();
    std::vector<int> canon;
    NniReq q;
    q.par = edge_parents(N, ip); q.in = in_edges(N, ip, ix);
    q.pos.assign((size_t)N, 0);
    for (int u = 0; u < N; u++) q.pos[h->preorder[u]] = u;
    if (!swaps) {
        canon.resize((size_t)2 * std::max(1, plk_nni_swaps(N, ip, ix, nullptr)));
        const int count = plk_nni_swaps(N, ip, ix, canon.data());
        if (n_swaps != count) {
            h->err = "plk_nni_ll: the canonical list has " + std::to_string(count) + " swaps, the call asks for " + std::to_string(n_swaps);
            return PLK_E_ARG;
        }
        swaps = canon.data();
    } else {
        for (int i = 0; i < n_swaps; i++) {
            const std::string bad = nni_pair_fault(N, ip, ix, q.par, q.in, swaps[2 * i], swaps[2 * i + 1]);
            if (!bad.empty()) {
                h->err = "plk_nni_ll: pair " + std::to_string(i) + " (" + std::to_string(swaps[2 * i]) + ", " + std::to_string(swaps[2 * i + 1]) +
                         ") is no swap: " + bad;
                return PLK_E_ARG;
            }
        }
    }
    if (n_swaps == 0) return PLK_OK;
    QueryTimer qt(h);
    q.n = n_swaps; q.swaps = swaps; q.site_out = site_out; q.want_sums = sums_out != nullptr;
    q.acc.assign((size_t)n_swaps, 0.0L);
    const int rc = run_updown(h, false, false, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr, &q);
    if (rc) return rc;
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { h->err = std::string("plk_nni_ll: ") + hipGetErrorString(e); return PLK_E_DEVICE; }
    if (sums_out) put_dd_rows(sums_out, q.acc.data(), (size_t)n_swaps);
    return PLK_OK;
}

/*
 * Log likelihood of the tree with a new leaf attached to an edge, for every (query, edge) of the call (plk_place.h): one
 * down pass per site chunk, one up pass per PLACE_MAX_ROWS rows.  Every argument is checked, the rates of the three new
 * edges by the check of the model's rates, before anything is queued.
 */
extern "C" int plk_place_ll(plk_engine *h, int n_queries, const uint8_t *q_codes, const double *q_dense, int n_edges, const int *edges,
                            double split, double pendant_rate, double *site_out, double *sums_out)
{
    if (!plk_live(h)) return PLK_E_ARG;
    if (h->k == 0 || h->pat_mode == 0) { h->err = "plk_place_ll: tree, model and patterns must be set"; return PLK_E_ARG; }
    if (n_queries < 0) { h->err = "plk_place_ll: n_queries is negative"; return PLK_E_ARG; }
    if (n_edges < 0) { h->err = "plk_place_ll: n_edges is negative"; return PLK_E_ARG; }
    if ((q_codes != nullptr) == (q_dense != nullptr)) { h->err = "plk_place_ll: exactly one of q_codes and q_dense must be given"; return PLK_E_ARG; }
    if (q_codes && h->pat_mode != 1) { h->err = "plk_place_ll: q_codes given, but the engine holds dense patterns: give q_dense"; return PLK_E_ARG; }
    if (q_dense && h->pat_mode != 2) { h->err = "plk_place_ll: q_dense given, but the engine holds compact patterns: give q_codes"; return PLK_E_ARG; }
    const int N = h->N, E = h->E, k = h->k;
    const long S = h->S;
    if (!(split >= 0.0 && split <= 1.0)) { h->err = "plk_place_ll: split must be a number in [0, 1]"; return PLK_E_ARG; }
    if (!(pendant_rate >= 0.0 && pendant_rate < INFINITY)) { h->err = "plk_place_ll: pendant_rate must be finite and not negative"; return PLK_E_ARG; }
    if (!edges && n_edges != E) {
        h->err = "plk_place_ll: edges is NULL (every edge), but n_edges is " + std::to_string(n_edges) + " and the tree has " + std::to_string(E) + " edges";
        return PLK_E_ARG;
    }
    for (int i = 0; edges && i < n_edges; i++)
        if (edges[i] < 0 || edges[i] >= E) {
            h->err = "plk_place_ll: edges[" + std::to_string(i) + "] = " + std::to_string(edges[i]) + " is out of range";
            return PLK_E_ARG;
        }
    if (q_codes)
        for (int q = 0; q < n_queries; q++)
            for (long s = 0; s < S; s++)
                if (q_codes[(size_t)q * S + s] >= h->nchar) {
                    h->err = "plk_place_ll: q_codes: query " + std::to_string(q) + ", site " + std::to_string(s) + ": code " +
                             std::to_string((int)q_codes[(size_t)q * S + s]) + " is not below nchar = " + std::to_string(h->nchar);
                    return PLK_E_ARG;
                }
    if (q_dense)
        for (size_t i = 0; i < (size_t)n_queries * k * S; i++)
            if (!(q_dense[i] >= 0.0 && q_dense[i] < INFINITY)) {
                h->err = "plk_place_ll: q_dense: query " + std::to_string(i / ((size_t)k * S)) + ", state " + std::to_string(i / S % k) + ", site " +
                         std::to_string(i % S) + " is negative or not finite";
                return PLK_E_ARG;
            }
    PlaceReq q;
    std::vector<int> all;
    if (!edges) { all.resize((size_t)E); for (int e = 0; e < E; e++) all[e] = e; edges = all.data(); }
    q.Q = n_queries; q.ne = n_edges; q.edges = edges; q.compact = q_codes != nullptr;
    /* the distinct target edges in the order of their first appearance, and the rates of the call */
    {
        std::vector<int> slot_of((size_t)std::max(E, 1), -1);
        const double lower = 1.0 - split;
        for (int i = 0; i < n_edges; i++) {
            int &sl = slot_of[edges[i]];
            if (sl < 0) {
                sl = (int)q.rates.size() / 2;
                q.rates.push_back(split * h->edge_rates[edges[i]]);
                q.rates.push_back(lower * h->edge_rates[edges[i]]);
            }
            q.slot.push_back(sl);
        }
        q.rates.push_back(pendant_rate);
        /* Of the three, only the pendant rate can be refused today: split is in [0, 1], so both parts of an edge are at most
         * the rate plk_set_model / plk_update_edge_rates accepted for it.  The parts are checked all the same, for a writer
         * of h->edge_rates added later (as in run_expm). */
        const size_t kk = (size_t)k * k;
        for (size_t j = 0; j < q.rates.size(); j++)
            if (plk_k1_check_values(k, h->C, 1, h->Qn.data(), h->Qn.data() + kk, &q.rates[j], h->cat_rates.data(), h->cat_prior.data(),
                                    h->root_mode, h->root_w.data(), nullptr, 0)) {
                char msg[200];
                int e = -1;
                for (int i = 0; i < n_edges && e < 0; i++) if (q.slot[i] == (int)j / 2) e = edges[i];
                if (j + 1 == q.rates.size()) snprintf(msg, sizeof msg, "the pendant edge (rate %g)", q.rates[j]);
                else snprintf(msg, sizeof msg, "the %s part of edge %d (rate %g)", j % 2 ? "lower" : "upper", e, q.rates[j]);
                h->err = std::string("plk_place_ll: the transition matrix kernel refuses ") + msg +
                         ": rate x length x |Qn| must be finite and at most 2^40" + K1_CSR_NOTE;
                return PLK_E_ARG;
            }
    }
    if (n_queries == 0 || n_edges == 0 || (!site_out && !sums_out)) return PLK_OK;      /* nothing asked for: nothing runs */
    HIPCHK(h, hipSetDevice(h->device));
    QueryTimer qt(h);
    int rc;
    if (q_codes) {
        if ((rc = dev_reserve(h, &h->d_plcodes, &h->plcodes_cap, (size_t)n_queries * h->Spad))) return rc;
        HIPCHK(h, hipMemsetAsync(h->d_plcodes, 0, (size_t)n_queries * h->Spad, h->stream));
        HIPCHK(h, hipMemcpy2DAsync(h->d_plcodes, (size_t)h->Spad, q_codes, (size_t)S, (size_t)S, (size_t)n_queries, hipMemcpyHostToDevice, h->stream));
    } else {
        if ((rc = dev_reserve(h, &h->d_pldense, &h->pldense_cap, (size_t)n_queries * k * S))) return rc;
        HIPCHK(h, hipMemcpyAsync(h->d_pldense, q_dense, (size_t)n_queries * k * S * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    q.par = edge_parents(N, h->indptr.data());
    q.pos.assign((size_t)N, 0);
    for (int u = 0; u < N; u++) q.pos[h->preorder[u]] = u;
    q.site_out = site_out; q.want_sums = sums_out != nullptr;
    q.acc.assign((size_t)q.total(), 0.0L);
    rc = run_updown(h, false, false, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr, nullptr, &q);
    const hipError_t e = hipStreamSynchronize(h->stream);        /* the uploads above read the caller's arrays */
    if (rc) return rc;
    if (e != hipSuccess) { h->err = std::string("plk_place_ll: ") + hipGetErrorString(e); return PLK_E_DEVICE; }
    if (sums_out)
        for (int qi = 0; qi < n_queries; qi++)
            for (int ei = 0; ei < n_edges; ei++) put_dd(sums_out + 2 * ((size_t)qi * n_edges + ei), q.acc[(size_t)ei * n_queries + qi]);
    return PLK_OK;
}

/*
 * Log likelihood of subtree prune-and-regraft moves of the current tree (plk_spr.h): one down pass per site chunk, per
 * prune edge one pass that stores the vectors of the pruned tree and one pass per PLACE_MAX_ROWS moves.  Every pair is
 * checked, the rates of the two parts of every target edge by the check of the model's rates, before anything is queued.
 */
extern "C" int plk_spr_ll(plk_engine *h, int n_moves, const int *moves, double split, double *site_out, double *sums_out)
{
    if (!plk_live(h)) return PLK_E_ARG;
    if (h->k == 0 || h->pat_mode == 0) { h->err = "plk_spr_ll: tree, model and patterns must be set"; return PLK_E_ARG; }
    if (n_moves < 0) { h->err = "plk_spr_ll: negative number of moves"; return PLK_E_ARG; }
    if (!(split >= 0.0 && split <= 1.0)) { h->err = "plk_spr_ll: split must be a number in [0, 1]"; return PLK_E_ARG; }
    const int N = h->N, E = h->E, k = h->k;
    const int *ip = h->indptr.data(), *ix = h->indices.data();
    SprReq q;
    q.epar = edge_parents(N, ip); q.in = in_edges(N, ip, ix);
    q.pos.assign((size_t)N, 0); q.size.assign((size_t)N, 1); q.depth.assign((size_t)N, 0); q.par.assign((size_t)N, -1);
    for (int u = 0; u < N; u++) q.pos[h->preorder[u]] = u;
    for (int u = 1; u < N; u++) { const int y = h->preorder[u]; q.par[y] = q.epar[q.in[y]]; q.depth[y] = q.depth[q.par[y]] + 1; q.max_depth = std::max(q.max_depth, q.depth[y]); }
    for (int u = N - 1; u > 0; u--) { const int y = h->preorder[u]; q.size[q.par[y]] += q.size[y]; }
    {
        /* depth-first positions: the subtree of a node is an interval of them, which the engine's order does not promise */
        q.dpos.assign((size_t)N, 0);
        std::vector<int> stack(1, h->preorder[0]);
        int seen = 0;
        while (!stack.empty()) {
            const int y = stack.back();
            stack.pop_back();
            q.dpos[y] = seen++;
            for (int idx = ip[y + 1] - 1; idx >= ip[y]; idx--) stack.push_back(ix[idx]);
        }
    }
    std::vector<int> canon;
    if (!moves) {
        canon.resize((size_t)2 * std::max(1, plk_spr_moves(N, ip, ix, nullptr)));
        const int count = plk_spr_moves(N, ip, ix, canon.data());
        if (n_moves != count) {
            h->err = "plk_spr_ll: the canonical list has " + std::to_string(count) + " moves, the call asks for " + std::to_string(n_moves);
            return PLK_E_ARG;
        }
        moves = canon.data();
    } else {
        for (int i = 0; i < n_moves; i++) {
            const int p = moves[2 * i], e = moves[2 * i + 1];
            const char *bad = nullptr;
            if (p < 0 || p >= E || e < 0 || e >= E) bad = "edge index out of range";
            else if (p == e) bad = "the target is the pruned edge";
            else {
                const int x = ix[p], u = q.epar[e];
                if (q.dpos[u] >= q.dpos[x] && q.dpos[u] < q.dpos[x] + q.size[x]) bad = "the target lies below the pruned edge";
            }
            if (bad) {
                h->err = "plk_spr_ll: pair " + std::to_string(i) + " (" + std::to_string(p) + ", " + std::to_string(e) + ") is no move: " + bad;
                return PLK_E_ARG;
            }
        }
    }
    /* the distinct target edges in the order of their first appearance, and the rates of the call */
    {
        std::vector<int> slot_of((size_t)std::max(E, 1), -1), first_of;
        const double lower = 1.0 - split;
        for (int i = 0; i < n_moves; i++) {
            const int e = moves[2 * i + 1];
            int &sl = slot_of[e];
            if (sl < 0) {
                sl = (int)q.rates.size() / 2;
                q.rates.push_back(split * h->edge_rates[e]);
                q.rates.push_back(lower * h->edge_rates[e]);
                first_of.push_back(e);
            }
            q.slot.push_back(sl);
        }
        /* both parts of an edge are at most the rate the model's check accepted for it; they are checked all the same, as
         * in plk_place_ll */
        const size_t kk = (size_t)k * k;
        for (size_t j = 0; j < q.rates.size(); j++)
            if (plk_k1_check_values(k, h->C, 1, h->Qn.data(), h->Qn.data() + kk, &q.rates[j], h->cat_rates.data(), h->cat_prior.data(),
                                    h->root_mode, h->root_w.data(), nullptr, 0)) {
                char msg[200];
                snprintf(msg, sizeof msg, "the %s part of target edge %d (rate %g)", j % 2 ? "lower" : "upper", first_of[j / 2], q.rates[j]);
                h->err = std::string("plk_spr_ll: the transition matrix kernel refuses ") + msg +
                         ": rate x length x |Qn| must be finite and at most 2^40" + K1_CSR_NOTE;
                return PLK_E_ARG;
            }
    }
    if (n_moves == 0 || (!site_out && !sums_out)) return PLK_OK;      /* nothing asked for: nothing runs */
    HIPCHK(h, hipSetDevice(h->device));
    QueryTimer qt(h);
    q.n = n_moves; q.moves = moves; q.site_out = site_out; q.want_sums = sums_out != nullptr;
    q.order.resize((size_t)n_moves);
    for (int i = 0; i < n_moves; i++) q.order[i] = i;
    std::stable_sort(q.order.begin(), q.order.end(), [&](int x, int y) { return moves[2 * x] < moves[2 * y]; });
    q.acc.assign((size_t)n_moves, 0.0L);
    const int rc = run_updown(h, false, false, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, &q);
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (rc) return rc;
    if (e != hipSuccess) { h->err = std::string("plk_spr_ll: ") + hipGetErrorString(e); return PLK_E_DEVICE; }
    if (sums_out)
        for (int t = 0; t < n_moves; t++) put_dd(sums_out + 2 * (size_t)q.order[t], q.acc[t]);
    return PLK_OK;
}

extern "C" int plk_marginal(plk_engine *h, const int *node_mask, double *site_out, double *sums_out)
{
    if (!plk_live(h)) return PLK_E_ARG;
    return run_updown(h, false, true, nullptr, node_mask, site_out, sums_out);
}

/* ====================================================================== */
/* Edge-rate optimisation with the patterns resident      */
/* ====================================================================== */

/* ---------------------------------------------------------------------- */
/* rate-category posteriors and posterior mean site rates (plk_catpost.h)  */
/* ---------------------------------------------------------------------- */

/* the k = 4 kernel: what plk_k4_choose asks of the C++ interpreter (its LDS image at one site per lane), C terms in registers */
static bool use_catpost4(const plk_engine *h)
{
    if (h->opt_force_generic || h->k != 4 || h->pat_mode != 1 || h->C > PLK_CATPOST_REG_C) return false;
    if (h->slots_needed > PLK_FUSED_SLOTS) return false;
    return plk_fused_lds_bytes(h->pg, h->nchar, PLK_TILE) <= PLK_LDS_LIMIT;
}

template <int K>
static void launch_catpost_generic(plk_engine *h, const CatPostGenArgs &a, unsigned grid)
{
    hipLaunchKernelGGL(k_catpost_generic<K>, dim3(grid), dim3(GEN_BLOCK), 0, h->stream, a);
}

/* every output may be NULL; per-site outputs are host buffers ([S][C], [S], [S]), sums {hi, lo} pairs ([C][2], [2], [2]) */
static int cat_posterior_impl(plk_engine *h, double *post_out, double *rate_out, double *site_ll_out,
                              double *post_sums_out, double *rate_sum_out, double *ll_sum_out)
{
    if (h->k == 0 || h->pat_mode == 0) { h->err = "plk_cat_posterior: tree, model and patterns must be set"; return PLK_E_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    if (!h->cp_ev0) { HIPCHK(h, hipEventCreate(&h->cp_ev0)); HIPCHK(h, hipEventCreate(&h->cp_ev1)); }
    HIPCHK(h, hipEventRecord(h->cp_ev0, h->stream));
    /* the program and P are brought up to date the way plk_ll does it; the formats plk_ll has cached stay as they are */
    if (h->prog_dirty) { if ((rc = build_program(h))) return rc; }
    if (h->model_dirty) { if ((rc = run_expm(h, true, false))) return rc; }
    const long S = h->S;
    const int C = h->C, K = h->K, nops = (int)h->ops.size(), ntips = (int)h->tip_edge.size();
    const bool k4 = use_catpost4(h);
    const int kind = k4 ? 1 : 2;
    const bool want_sums = post_sums_out || rate_sum_out || ll_sum_out;
    if (h->cp_kind != kind) {
        if (k4) {
            plk_fused_build(h->N, h->pg, h->cpf);
            std::vector<int> me = h->cpf.mat_edge, te = h->tip_edge;
            me.push_back(-1);                            /* the spare matrix is all zeros */
            te.push_back(-1);                            /* pseudo slot: the raw definitions */
            if ((rc = dev_upload(h, &h->d_cp_fops, reinterpret_cast<const int4 *>(h->cpf.fops.data()), h->cpf.fops.size())) ||
                (rc = dev_upload(h, &h->d_cp_mat_edge, me.data(), me.size())) ||
                (rc = dev_upload(h, &h->d_cp_tip_edge, te.data(), te.size())) ||
                (rc = dev_upload(h, &h->d_cp_obs_nodes, h->obs_nodes.data(), h->obs_nodes.size()))) return rc;
        } else {
            if ((rc = dev_upload(h, &h->d_cp_ops, reinterpret_cast<const int2 *>(h->ops.data()), h->ops.size())) ||
                (rc = dev_upload(h, &h->d_cp_op_edge, h->op_edge.data(), h->op_edge.size()))) return rc;
        }
        h->cp_kind = kind;
        h->cp_tables_valid = false;
    }
    if (!h->d_cp_flag) { if ((rc = dev_alloc(h, &h->d_cp_flag, 1))) return rc; }
    HIPCHK(h, hipMemsetAsync(h->d_cp_flag, 0, sizeof(int), h->stream));
    /* outputs: [C][S] posteriors, [S] rates, [S] log likelihoods */
    if ((rc = dev_reserve(h, &h->d_cp_out, &h->cp_out_cap, (size_t)(C + 2) * S))) return rc;
    double *d_post = h->d_cp_out, *d_rate = h->d_cp_out + (size_t)C * S, *d_ll = d_rate + S;
    const unsigned grid = k4 ? (unsigned)((S + PLK_TILE - 1) / PLK_TILE) : (unsigned)((S + GEN_BLOCK - 1) / GEN_BLOCK);
    const int rows = C + 2;
    if (want_sums) { if ((rc = dev_reserve(h, &h->d_cp_partial, &h->cp_partial_cap, (size_t)rows * grid + rows))) return rc; }
    dd *d_sums = h->d_cp_partial, *d_part = want_sums ? h->d_cp_partial + rows : nullptr;
    if (k4) {
        const int nmat1 = (int)h->cpf.mat_edge.size() + 1;
        if ((rc = dev_reserve(h, &h->d_cp_PS, &h->cp_ps_cap, (size_t)C * nmat1 * 16))) return rc;
        if ((rc = dev_reserve(h, &h->d_cp_tip, &h->cp_tip_cap, (size_t)C * (ntips + 1) * h->nchar * 4))) return rc;
        if (!h->cp_tables_valid) {
            /* the matrix stream and the tip tables of the current P: rebuilt after K1 ran or the program changed */
            hipLaunchKernelGGL(k_build_stream, dim3(nmat1, C), dim3(64), 0, h->stream, 4, 4, h->E, nmat1, h->d_cp_mat_edge, h->d_P, h->d_cp_PS);
            hipLaunchKernelGGL(k_build_tip, dim3(ntips + 1, C), dim3(64), 0, h->stream,
                               h->E, ntips + 1, h->nchar, h->d_cp_tip_edge, h->d_Pdd, h->d_defs, h->d_cp_tip);
            HIPCHK(h, hipGetLastError());
            h->cp_tables_valid = true;
        }
        CatPostArgs a;
        a.f.S = S; a.f.Spad = h->Spad; a.f.C = C; a.f.nops = nops; a.f.nmat = nmat1 - 1;
        a.f.ntips = ntips + 1; a.f.nchar = h->nchar; a.f.nobs = (int)h->obs_nodes.size();
        a.f.ops = h->d_cp_fops; a.f.PS = h->d_cp_PS; a.f.tip = h->d_cp_tip;
        a.f.codes = h->d_codes; a.f.obs_nodes = h->d_cp_obs_nodes; a.f.defs = h->d_defs;
        a.f.cat_prior = h->d_cat_prior; a.f.root_w = h->d_root_w; a.f.w = h->d_w;
        a.f.site_ll = d_ll; a.f.partial = nullptr;
        a.f.root_mode = h->root_mode; a.f.first_row = h->cpf.first_row;
        a.cat_rates = h->d_cat_rates; a.post = d_post; a.rate = d_rate; a.partial = d_part; a.zero_flag = h->d_cp_flag;
        const size_t lds = plk_fused_lds_bytes(h->pg, h->nchar, PLK_TILE);
        const int D = h->slots_needed <= 4 ? 4 : (h->slots_needed <= 8 ? 8 : 16);
        /* replay the interpreter's fetches and LDS addresses on the host before launching (plk_program.h) */
        const std::string bad = plk_fused_check_cpp(h->N, h->pg, h->cpf, h->nchar, D, 1, lds);
        if (!bad.empty()) { h->err = "internal: " + bad; return PLK_E_ARG; }
        if (D == 4) hipLaunchKernelGGL(k_ll_fused4_catpost<4>, dim3(grid), dim3(PLK_TILE), lds, h->stream, a);
        else if (D == 8) hipLaunchKernelGGL(k_ll_fused4_catpost<8>, dim3(grid), dim3(PLK_TILE), lds, h->stream, a);
        else hipLaunchKernelGGL(k_ll_fused4_catpost<16>, dim3(grid), dim3(PLK_TILE), lds, h->stream, a);
        h->info_cat_posterior_kernel = 1;
    } else {
        if ((rc = dev_reserve(h, &h->d_cp_PS, &h->cp_ps_cap, (size_t)C * std::max(nops, 1) * K * K))) return rc;
        if ((rc = dev_reserve(h, &h->d_cp_expo, &h->cp_expo_cap, (size_t)C * S))) return rc;
        const int nslots = std::max(h->slots_needed, 1);
        if ((rc = dev_reserve(h, &h->d_slots, &h->slots_cap, (size_t)nslots * h->k * S))) return rc;
        if (nops > 0 && !h->cp_tables_valid)
            hipLaunchKernelGGL(k_build_stream, dim3(nops, C), dim3(K * K >= 256 ? 256 : 64), 0, h->stream,
                               h->k, K, h->E, nops, h->d_cp_op_edge, h->d_P, h->d_cp_PS);
        h->cp_tables_valid = true;
        CatPostGenArgs a;
        a.g.S = S; a.g.Spad = h->Spad; a.g.k = h->k; a.g.C = C; a.g.nops = nops; a.g.nchar = h->nchar;
        a.g.pat_mode = h->pat_mode; a.g.root_mode = h->root_mode; a.g.ops = h->d_cp_ops; a.g.PS = h->d_cp_PS;
        a.g.codes = h->d_codes; a.g.defs = h->d_defs; a.g.B = h->d_B; a.g.cat_prior = h->d_cat_prior;
        a.g.root_w = h->d_root_w; a.g.w = h->d_w; a.g.slots = h->d_slots; a.g.site_ll = d_ll; a.g.partial = nullptr;
        a.cat_rates = h->d_cat_rates; a.post = d_post; a.expo = h->d_cp_expo; a.rate = d_rate; a.partial = d_part; a.zero_flag = h->d_cp_flag;
        dispatch_K(K, [&](auto Kc) { launch_catpost_generic<decltype(Kc)::value>(h, a, grid); });
        h->info_cat_posterior_kernel = 2;
    }
    HIPCHK(h, hipGetLastError());
    if (want_sums) {
        /* fixed-order double-double sums of the workgroups' partials, one block per output row */
        hipLaunchKernelGGL(k_dd_final, dim3(rows), dim3(256), 0, h->stream, (int)grid, d_part, d_sums);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipEventRecord(h->cp_ev1, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    {
        float ms = 0;
        HIPCHK(h, hipEventElapsedTime(&ms, h->cp_ev0, h->cp_ev1));
        h->info_cat_posterior_ns = (long)(ms * 1e6);
    }
    if (want_sums) {
        int flag = 0;
        HIPCHK(h, hipMemcpy(&flag, h->d_cp_flag, sizeof(int), hipMemcpyDeviceToHost));
        if (flag) { h->err = "plk_cat_posterior: site likelihood zero at a site of non-zero weight, the sums are undefined"; return PLK_E_ARG; }
        std::vector<dd> host(rows);
        HIPCHK(h, hipMemcpy(host.data(), d_sums, rows * sizeof(dd), hipMemcpyDeviceToHost));
        if (post_sums_out) for (int c = 0; c < C; c++) { post_sums_out[2 * c] = host[c].hi; post_sums_out[2 * c + 1] = host[c].lo; }
        if (rate_sum_out) { rate_sum_out[0] = host[C].hi; rate_sum_out[1] = host[C].lo; }
        if (ll_sum_out) { ll_sum_out[0] = host[C + 1].hi; ll_sum_out[1] = host[C + 1].lo; }
    }
    if (post_out) { if ((rc = copy_site_rows(h, (size_t)C, S, 0, d_post, post_out))) return rc; }
    if (rate_out) HIPCHK(h, hipMemcpy(rate_out, d_rate, (size_t)S * sizeof(double), hipMemcpyDeviceToHost));
    if (site_ll_out) HIPCHK(h, hipMemcpy(site_ll_out, d_ll, (size_t)S * sizeof(double), hipMemcpyDeviceToHost));
    return PLK_OK;
}

extern "C" int plk_cat_posterior_ll(plk_engine *h, double *post_out, double *rate_out, double *site_ll_out,
                                    double *post_sums_out, double *rate_sum_out, double *ll_sum_out)
{
    if (!plk_live(h)) return PLK_E_ARG;
    return cat_posterior_impl(h, post_out, rate_out, site_ll_out, post_sums_out, rate_sum_out, ll_sum_out);
}

extern "C" int plk_cat_posterior(plk_engine *h, double *post_out, double *rate_out, double *post_sums_out, double *rate_sum_out)
{
    if (!plk_live(h)) return PLK_E_ARG;
    return cat_posterior_impl(h, post_out, rate_out, nullptr, post_sums_out, rate_sum_out, nullptr);
}

static int fit_objective(plk_engine *h, const std::vector<double> &rates, long double *ll_out)
{
    int rc;
    if ((rc = plk_update_edge_rates(h, rates.data()))) return rc;
    double s[2] = {0.0, 0.0};
    if ((rc = plk_ll(h, nullptr, PLK_HOST, s))) return rc;
    *ll_out = (long double)s[0] + (long double)s[1];
    return PLK_OK;
}

/*
 * Maximise sum_s w_s ll_s over the edge rate coefficients.  The reference has no driver for this; its
 * old-examples/opt.py and old-examples/gell_dna_opt.py run scipy's L-BFGS-B over arbplf_ll / arbplf_deriv
 * through the Python API, and test_scripts/test_em_monotonicity.py iterates arbplf_em_update.  Here the loop
 * runs next to the device: patterns, weights and the tree stay resident, an iteration re-runs K1 and the
 * traversal kernels only.
 *   PLK_FIT_EM     r_e <- r_e * E[transitions on e] / E[rate-weighted dwell on e]   (src/arbplfem.c:397-503)
 *   PLK_FIT_LBFGS  L-BFGS (8 pairs, Armijo backtracking) on log r_e with the gradient r_e * d ll / d r_e
 */
extern "C" int plk_fit_edge_rates(plk_engine *h, int method, int max_iter, double ftol, const int *edge_mask,
                                  double *rates_inout, double *ll_trace, int *iters_out, long *evals_out)
{
    if (!plk_live(h) || !rates_inout) return PLK_E_ARG;
    if (h->k == 0 || h->pat_mode == 0) { h->err = "plk_fit_edge_rates: tree, model and patterns must be set"; return PLK_E_ARG; }
    if (method != PLK_FIT_EM && method != PLK_FIT_LBFGS) { h->err = "plk_fit_edge_rates: unknown method"; return PLK_E_ARG; }
    const int E = h->E, k = h->k;
    const size_t kk = (size_t)k * k;
    int rc;
    long evals = 0;
    std::vector<double> rates(rates_inout, rates_inout + E);
    for (int e = 0; e < E; e++)
        if (!(rates[e] >= 0.0) || !std::isfinite(rates[e])) { h->err = "plk_fit_edge_rates: rates must be finite and non-negative"; return PLK_E_ARG; }
    std::vector<int> free_e;
    for (int e = 0; e < E; e++) if ((!edge_mask || edge_mask[e]) && rates[e] > 0.0) free_e.push_back(e);
    std::vector<int> mask(std::max(E, 1), 0);
    for (int e : free_e) mask[e] = 1;
    long double ll = 0;
    if ((rc = fit_objective(h, rates, &ll))) return rc;
    evals++;
    if (ll_trace) ll_trace[0] = (double)ll;
    int it = 0;
    if (!std::isfinite((double)ll)) { h->err = "plk_fit_edge_rates: the initial log likelihood is not finite"; return PLK_E_ARG; }

    if (method == PLK_FIT_EM) {
        std::vector<double> Ld(2 * kk, 0.0), Lt(2 * kk, 0.0), dw((size_t)2 * E + 2), tr((size_t)2 * E + 2);
        for (int i = 0; i < k; i++)
            for (int j = 0; j < k; j++) {
                const size_t q = (size_t)i * k + j;
                if (i == j) { Ld[q] = -h->Qn[q]; Ld[kk + q] = -h->Qn[kk + q]; }
                else { Lt[q] = h->Qn[q]; Lt[kk + q] = h->Qn[kk + q]; }
            }
        for (; it < max_iter && !free_e.empty(); ) {
            /* both expectations in one pass where the kernels allow it */
            std::vector<double> Lh(2 * kk), Ll(2 * kk), both((size_t)4 * E + 4);
            std::copy(Ld.begin(), Ld.begin() + kk, Lh.begin()); std::copy(Lt.begin(), Lt.begin() + kk, Lh.begin() + kk);
            std::copy(Ld.begin() + kk, Ld.end(), Ll.begin()); std::copy(Lt.begin() + kk, Lt.end(), Ll.begin() + kk);
            if ((rc = plk_edge_expect_multi(h, 2, Lh.data(), Ll.data(), PLK_COEF_PRIOR_RATE, mask.data(), nullptr, both.data()))) return rc;
            std::copy(both.begin(), both.begin() + 2 * E, dw.begin());
            std::copy(both.begin() + 2 * E, both.begin() + 4 * E, tr.begin());
            for (int e : free_e) {
                const long double t = (long double)tr[2 * e] + (long double)tr[2 * e + 1];
                const long double d = (long double)dw[2 * e] + (long double)dw[2 * e + 1];
                const double v = t == 0 ? 0.0 : (double)(t / d * (long double)rates[e]);
                if (!std::isfinite(v) || v < 0) { h->err = "plk_fit_edge_rates: EM update is not finite"; return PLK_E_DEVICE; }
                rates[e] = v;
            }
            long double ll_new = 0;
            if ((rc = fit_objective(h, rates, &ll_new))) return rc;
            evals++;
            it++;
            if (ll_trace) ll_trace[it] = (double)ll_new;
            const long double gain = ll_new - ll;
            ll = ll_new;
            if (fabsl(gain) <= (long double)ftol * std::max<long double>(1.0L, fabsl(ll))) break;
        }
    } else {
        const int n = (int)free_e.size(), M = 8;
        std::vector<double> x(n), g(n), xn(n), gn(n), d(n), sums((size_t)2 * E + 2);
        std::vector<std::vector<double>> Sh, Yh;
        std::vector<double> rho;
        auto gradient = [&](const std::vector<double> &r, std::vector<double> &out) -> int {
            /* rates are already current on the device (set by the accepted objective evaluation) */
            int rc2 = plk_deriv(h, mask.data(), nullptr, sums.data());
            if (rc2) return rc2;
            for (int i = 0; i < n; i++) {
                const int e = free_e[i];
                out[i] = -(double)(((long double)sums[2 * e] + (long double)sums[2 * e + 1]) * (long double)r[e]);
            }
            return PLK_OK;
        };
        for (int i = 0; i < n; i++) x[i] = std::log(rates[free_e[i]]);
        if (n > 0 && (rc = gradient(rates, g))) return rc;
        double f = -(double)ll;
        for (; it < max_iter && n > 0; ) {
            /* two-loop recursion */
            d = g;
            const int hs = (int)Sh.size();
            std::vector<double> alpha(hs);
            for (int j = hs - 1; j >= 0; j--) {
                double a = 0; for (int i = 0; i < n; i++) a += Sh[j][i] * d[i];
                a *= rho[j]; alpha[j] = a;
                for (int i = 0; i < n; i++) d[i] -= a * Yh[j][i];
            }
            if (hs > 0) {
                double sy = 0, yy = 0;
                for (int i = 0; i < n; i++) { sy += Sh[hs - 1][i] * Yh[hs - 1][i]; yy += Yh[hs - 1][i] * Yh[hs - 1][i]; }
                const double gam = sy / yy;
                for (int i = 0; i < n; i++) d[i] *= gam;
            }
            for (int j = 0; j < hs; j++) {
                double b = 0; for (int i = 0; i < n; i++) b += Yh[j][i] * d[i];
                b *= rho[j];
                for (int i = 0; i < n; i++) d[i] += Sh[j][i] * (alpha[j] - b);
            }
            double gd = 0, gnorm = 0, dmax = 0;
            for (int i = 0; i < n; i++) { d[i] = -d[i]; gd += g[i] * d[i]; gnorm = std::max(gnorm, std::fabs(g[i])); }
            if (!(gd < 0)) { Sh.clear(); Yh.clear(); rho.clear(); gd = 0; for (int i = 0; i < n; i++) { d[i] = -g[i]; gd += g[i] * d[i]; } }
            if (gnorm == 0) break;
            for (int i = 0; i < n; i++) dmax = std::max(dmax, std::fabs(d[i]));
            double t = Sh.empty() ? std::min(1.0, 1.0 / dmax) : 1.0;
            if (t * dmax > 5.0) t = 5.0 / dmax;                 /* at most a factor e^5 per step on any rate */
            bool ok = false;
            long double ll_new = 0;
            std::vector<double> rn = rates;
            for (int ls = 0; ls < 40; ls++, t *= 0.5) {
                for (int i = 0; i < n; i++) { xn[i] = x[i] + t * d[i]; rn[free_e[i]] = std::exp(xn[i]); }
                if ((rc = fit_objective(h, rn, &ll_new))) return rc;
                evals++;
                const double fn = -(double)ll_new;
                if (std::isfinite(fn) && fn <= f + 1e-4 * t * gd) { ok = true; break; }
            }
            if (!ok) { if ((rc = plk_update_edge_rates(h, rates.data()))) return rc; break; }
            if ((rc = gradient(rn, gn))) return rc;
            std::vector<double> s(n), y(n);
            double sy = 0, ss = 0, yy = 0;
            for (int i = 0; i < n; i++) { s[i] = xn[i] - x[i]; y[i] = gn[i] - g[i]; sy += s[i] * y[i]; ss += s[i] * s[i]; yy += y[i] * y[i]; }
            if (sy > 1e-10 * std::sqrt(ss * yy)) {
                if ((int)Sh.size() == M) { Sh.erase(Sh.begin()); Yh.erase(Yh.begin()); rho.erase(rho.begin()); }
                Sh.push_back(s); Yh.push_back(y); rho.push_back(1.0 / sy);
            }
            const double fn = -(double)ll_new, gain = f - fn;
            x = xn; g = gn; rates = rn; f = fn; ll = ll_new;
            it++;
            if (ll_trace) ll_trace[it] = (double)ll;
            if (gain <= ftol * std::max(1.0, std::fabs(f))) break;
        }
    }
    if ((rc = plk_update_edge_rates(h, rates.data()))) return rc;
    std::copy(rates.begin(), rates.end(), rates_inout);
    if (iters_out) *iters_out = it;
    if (evals_out) *evals_out = evals;
    return PLK_OK;
}

/* ====================================================================== */
/* Second derivatives of the log likelihood               */
/* ====================================================================== */

/* d2P[c][e] = r_c^2 * (Qn Qn) * P[c][e], accumulated in double-double from the unrounded P */
__global__ void k_d2p(int k, int E, const double *__restrict__ Q2 /* [2][k*k] hi, lo */, const dd *__restrict__ Pdd,
                      const double *__restrict__ cat_rates, double *__restrict__ out)
{
    const int ce = blockIdx.x, c = ce / E;
    const int kk = k * k;
    const dd *P = Pdd + (size_t)ce * kk;
    const double r = cat_rates[c];
    for (int idx = threadIdx.x; idx < kk; idx += blockDim.x) {
        const int i = idx / k, j = idx - i * k;
        dd acc = dd_make(0.0, 0.0);
        for (int l = 0; l < k; l++) acc = dd_add(acc, dd_mul(dd_make(Q2[i * k + l], Q2[kk + i * k + l]), P[l * k + j]));
        acc = dd_mul_d(dd_mul_d(acc, r), r);
        out[(size_t)ce * kk + idx] = acc.hi;
    }
}

/* G[i][j] = sum_s w_s D[i][s] D[j][s] for i >= j, one workgroup per pair, double-double accumulation */
__global__ __launch_bounds__(256) void k_gram(int E, long n, const double *__restrict__ D, const double *__restrict__ w,
                                              dd *__restrict__ out)
{
    const int i = blockIdx.x, j = blockIdx.y;
    if (j > i) return;
    const double *di = D + (size_t)i * n, *dj = D + (size_t)j * n;
    dd acc = dd_make(0.0, 0.0);
    for (long s = threadIdx.x; s < n; s += 256) {
        dd p = dd_two_prod(di[s], dj[s]);
        if (w) p = dd_mul_d(p, w[s]);
        acc = dd_add(acc, p);
    }
    acc = dd_block_sum(acc);
    if (threadIdx.x == 0) out[(size_t)i * E + j] = acc;
}

template <int K>
static void launch_hess_pass(plk_engine *h, const UpArgs &a, unsigned grid)
{
    hipLaunchKernelGGL(k_down_store<K>, dim3(grid), dim3(GEN_BLOCK), 0, h->stream, a);
    hipLaunchKernelGGL((k_up<K, true, false>), dim3(grid), dim3(GEN_BLOCK), 0, h->stream, a);
}

static void launch_hess_pass_k(plk_engine *h, const UpArgs &a, unsigned grid)
{
    dispatch_K(h->K, [&](auto Kc) { launch_hess_pass<decltype(Kc)::value>(h, a, grid); });
}

/*
 * Hessian of sum_s w_s ll_s with respect to the edge rate coefficients (CSR edge order), replacing
 * _recompute_second_order of src/arbplfhess.c:503-760 for the fp64, uncertified case.
 *
 *   d^2 ll / dr_i dr_j = H_ij / f - (g_i / f)(g_j / f)            (src/arbplfhess.c:455-493)
 * with f the site likelihood, g its gradient and H its Hessian.  g_i / f is the ordinary derivative pass.
 * Row j of H is obtained from the same two kernels run on a modified model in which edge j carries
 * dP_j = r Q P_j in the role of P_j and r^2 Q Q P_j in the role of dP_j: the derivative of that model with
 * respect to edge i is the second derivative (i, j) of the original one -- the reference's substitution of Q
 * along both root paths (src/arbplfhess.c:343-437) done for all i at once in O(E k^2) per site and row.
 * E + 1 passes per site chunk on the generic vector kernels, with the same exact power-of-two rescaling as the
 * first-order passes (each pass stores its factors; the common exponents of the modified and the unmodified model
 * are reconciled in the division).
 */
/* Qn^2 in double-double on the host, uploaded as [2][k*k] (hi, lo) */
static int upload_Q2(plk_engine *h, double **d_Q2)
{
    const int k = h->k;
    const size_t kk = (size_t)k * k;
    std::vector<double> Q2(2 * kk);
    for (int i = 0; i < k; i++)
        for (int j = 0; j < k; j++) {
            dd acc = dd_make(0.0, 0.0);
            for (int l = 0; l < k; l++)
                acc = dd_add(acc, dd_mul(dd_make(h->Qn[(size_t)i * k + l], h->Qn[kk + (size_t)i * k + l]),
                                         dd_make(h->Qn[(size_t)l * k + j], h->Qn[kk + (size_t)l * k + j])));
            Q2[(size_t)i * k + j] = acc.hi; Q2[kk + (size_t)i * k + j] = acc.lo;
        }
    return dev_upload(h, d_Q2, Q2.data(), Q2.size());
}

/* the E + 1 passes on the generic vector kernels (any k, dense patterns, any number of categories): Hrow[j][i] += the
 * weighted sums of row j of H / f, G[i][j] += sum_s w_s (g_i / f)(g_j / f) for i >= j, gsum[i] += sum_s w_s g_i / f */
static int second_order_generic(plk_engine *h, std::vector<long double> &Hrow, std::vector<long double> &G, long double *gsum)
{
    int rc;
    const int N = h->N, E = h->E, k = h->k, K = h->K, C = h->C;
    const long S = h->S;
    const size_t kk = (size_t)k * k, strm = (size_t)C * E * K * K;

    double *d_Q2 = nullptr, *d_d2P = nullptr, *d_PT = nullptr, *d_PN = nullptr, *d_DT = nullptr, *d_DN = nullptr, *d_D2T = nullptr;
    double *d_LH0 = nullptr, *d_D0 = nullptr, *d_XM0 = nullptr;
    dd *d_G = nullptr;
    int *d_has = nullptr, *d_ns = nullptr;
    auto cleanup = [&]() {
        void *ps[] = {d_Q2, d_d2P, d_PT, d_PN, d_DT, d_DN, d_D2T, d_LH0, d_D0, d_XM0, d_G, d_has, d_ns};
        for (void *p : ps) if (p) (void)hipFree(p);
    };
    if ((rc = upload_Q2(h, &d_Q2)) || (rc = dev_alloc(h, &d_d2P, (size_t)C * E * kk)) ||
        (rc = dev_alloc(h, &d_PT, strm)) || (rc = dev_alloc(h, &d_PN, strm)) || (rc = dev_alloc(h, &d_DT, strm)) ||
        (rc = dev_alloc(h, &d_DN, strm)) || (rc = dev_alloc(h, &d_D2T, strm)) || (rc = dev_alloc(h, &d_G, (size_t)E * E))) { cleanup(); return rc; }
    hipLaunchKernelGGL(k_d2p, dim3(C * E), dim3(kk >= 256 ? 256 : 64), 0, h->stream, k, E, d_Q2, h->d_Pdd, h->d_cat_rates, d_d2P);
    const int bt = K * K >= 256 ? 256 : 64;
    hipLaunchKernelGGL(k_build_edge_stream, dim3(C * E), dim3(bt), 0, h->stream, k, K, 0, h->d_P, d_PT);
    hipLaunchKernelGGL(k_build_edge_stream, dim3(C * E), dim3(bt), 0, h->stream, k, K, 1, h->d_P, d_PN);
    hipLaunchKernelGGL(k_build_edge_stream, dim3(C * E), dim3(bt), 0, h->stream, k, K, 0, h->d_dP, d_DT);
    hipLaunchKernelGGL(k_build_edge_stream, dim3(C * E), dim3(bt), 0, h->stream, k, K, 1, h->d_dP, d_DN);
    hipLaunchKernelGGL(k_build_edge_stream, dim3(C * E), dim3(bt), 0, h->stream, k, K, 0, d_d2P, d_D2T);
    if (hipGetLastError() != hipSuccess) { cleanup(); h->err = "plk_hess: matrix set-up failed"; return PLK_E_DEVICE; }
    { const std::vector<int> hd = has_data_ints(h); if ((rc = dev_upload(h, &d_has, hd.data(), (size_t)N))) { cleanup(); return rc; } }

    /* exact power-of-two rescaling as in the first-order passes (trees of any size): the traversal program marks the
     * nodes, the factors are stored per pass, every pass reports the common exponent of its site likelihoods */
    if (h->prog_dirty) { if ((rc = build_program(h))) { cleanup(); return rc; } }
    const PlkStorageMaps sm = storage_maps(h);
    const int nsc = sm.nsc;
    if ((rc = dev_upload(h, &d_ns, sm.node_scale.data(), (size_t)N))) { cleanup(); return rc; }
    const size_t per_site_d = (size_t)(E + 2 * (size_t)N) * C * k + (size_t)(nsc + 2) * C + 2 + (size_t)E;
    const size_t per_site = (per_site_d + 2 + (size_t)E) * sizeof(double);
    long chunk;
    if ((rc = plan_site_chunk(h, "plk_hess", per_site, GEN_BLOCK, false, &chunk))) { cleanup(); return rc; }
    if ((rc = dev_reserve(h, &h->d_work, &h->work_cap, per_site_d * (size_t)chunk)) ||
        (rc = dev_alloc(h, &d_LH0, (size_t)chunk)) || (rc = dev_alloc(h, &d_XM0, (size_t)chunk)) ||
        (rc = dev_alloc(h, &d_D0, (size_t)E * chunk))) { cleanup(); return rc; }

    std::vector<dd> gh((size_t)E * E);
    for (long s0 = 0; s0 < S; s0 += chunk) {
        const long n = std::min(chunk, S - s0);
        UpArgs a;
        a.S = S; a.Spad = h->Spad; a.s0 = s0; a.n = n;
        a.N = N; a.E = E; a.k = k; a.C = C; a.nchar = h->nchar; a.pat_mode = h->pat_mode; a.root_mode = h->root_mode;
        a.dzero = 1;
        a.indptr = h->d_indptr; a.indices = h->d_indices; a.preorder = h->d_preorder; a.node_has_data = d_has;
        a.PT = d_PT; a.PN = d_PN; a.DT = d_DT; a.DN = d_DN; a.D2T = d_D2T;
        a.node_scale = d_ns;
        a.codes = h->d_codes; a.defs = h->d_defs; a.B = h->d_B;
        a.cat_prior = h->d_cat_prior; a.root_w = h->d_root_w; a.edge_mask = nullptr; a.node_mask = nullptr;
        double *p = h->d_work;
        a.EV = p; p += (size_t)E * C * k * n;
        a.LN = p; p += (size_t)N * C * k * n;
        a.FN = p; p += (size_t)N * C * k * n;
        a.SC = p; p += (size_t)nsc * C * n;
        a.CW = p; p += (size_t)C * n;
        a.XC = p; p += (size_t)C * n;
        a.XM = p; p += n;
        a.LH = p; p += n;
        a.DV = p; p += (size_t)E * n;
        a.MV = nullptr;
        const unsigned grid = (unsigned)((n + GEN_BLOCK - 1) / GEN_BLOCK);
        const double *w = h->d_w ? h->d_w + s0 : nullptr;
        /* pass 0: the model itself -> f and g / f */
        a.mod_edge = -1; a.LHdiv = nullptr; a.XMdiv = nullptr;
        launch_hess_pass_k(h, a, grid);
        hipError_t e = hipMemcpyAsync(d_LH0, a.LH, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_XM0, a.XM, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_D0, a.DV, (size_t)E * n * sizeof(double), hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_gram, dim3(E, E), dim3(256), 0, h->stream, E, n, d_D0, w, d_G);
            e = hipMemcpyAsync(gh.data(), d_G, (size_t)E * E * sizeof(dd), hipMemcpyDeviceToHost, h->stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) { cleanup(); h->err = std::string("plk_hess: ") + hipGetErrorString(e); return PLK_E_DEVICE; }
        for (int i = 0; i < E; i++)
            for (int j = 0; j <= i; j++) G[(size_t)i * E + j] += (long double)gh[(size_t)i * E + j].hi + (long double)gh[(size_t)i * E + j].lo;
        if (gsum && (rc = wsum_rows(h, E, n, d_D0, w, gsum))) { cleanup(); return rc; }
        /* passes 1..E: row j of the likelihood Hessian, normalised by the unmodified likelihood */
        a.LHdiv = d_LH0; a.XMdiv = d_XM0;
        for (int j = 0; j < E; j++) {
            a.mod_edge = j;
            launch_hess_pass_k(h, a, grid);
            if (hipGetLastError() != hipSuccess) { cleanup(); h->err = "plk_hess: kernel launch failed"; return PLK_E_DEVICE; }
            if ((rc = wsum_rows(h, E, n, a.DV, w, Hrow.data() + (size_t)j * E))) { cleanup(); return rc; }
        }
    }
    cleanup();
    return PLK_OK;
}

/* the k = 4 second-order pass (plk_hess4.h) applies: compact codes, at most four rate categories */
static bool use_hess4(const plk_engine *h)
{
    return !h->opt_force_generic && h->k == 4 && h->pat_mode == 1 && h->C <= 4 && h->E > 0;
}

template <int NM>
static void launch_hess4(plk_engine *h, const Hess4Args &a, unsigned grid)
{
    hipLaunchKernelGGL(k_hess4_down<NM>, dim3(grid), dim3(UD4_BLOCK), 0, h->stream, a);
    hipLaunchKernelGGL(k_hess4_up<NM>, dim3(grid), dim3(UD4_BLOCK), 0, h->stream, a);
}

/* rows of the Hessian the next launch carries when `left` rows remain: 4, 2 or 1 models, no idle row (three rows: 2 + 1) */
static int hess4_nm(int left) { return left >= 4 ? 4 : (left >= 2 ? 2 : 1); }

/* the same sums as second_order_generic on the k = 4 kernels: pass 0 (one model, no modified edge), then
 * launches of four edge-modified models each (two or one for the last rows) */
static int second_order_k4(plk_engine *h, std::vector<long double> &Hrow, std::vector<long double> &G, long double *gsum)
{
    int rc;
    const int N = h->N, E = h->E, C = h->C;
    const long S = h->S;
    if (h->prog_dirty) { if ((rc = build_program(h))) return rc; }
    const PlkStorageMaps sm = storage_maps(h);
    const std::vector<int> &edge_tip = sm.edge_tip, &node_int = sm.node_int, &node_scale = sm.node_scale, &te = sm.tip_edges;
    const int ntips = sm.ntips, nin = sm.nin, nsc = sm.nsc;
    const std::vector<int> hd = has_data_ints(h);

    double *d_Q2 = nullptr, *d_d2P = nullptr, *d_tab = nullptr, *d_LH0 = nullptr, *d_XM0 = nullptr, *d_D0 = nullptr;
    dd *d_G = nullptr;
    int *d_et = nullptr, *d_ni = nullptr, *d_ns = nullptr, *d_te = nullptr, *d_has = nullptr;
    auto cleanup = [&]() {
        void *ps[] = {d_Q2, d_d2P, d_tab, d_LH0, d_XM0, d_D0, d_G, d_et, d_ni, d_ns, d_te, d_has};
        for (void *p : ps) if (p) (void)hipFree(p);
    };
    const size_t ntab = (size_t)C * (ntips + 1) * h->nchar * 4;
    if ((rc = upload_Q2(h, &d_Q2)) || (rc = dev_alloc(h, &d_d2P, (size_t)C * E * 16)) || (rc = dev_alloc(h, &d_tab, 3 * ntab)) ||
        (rc = dev_alloc(h, &d_G, (size_t)E * E)) || (rc = dev_upload(h, &d_et, edge_tip.data(), (size_t)E)) ||
        (rc = dev_upload(h, &d_ni, node_int.data(), (size_t)N)) || (rc = dev_upload(h, &d_ns, node_scale.data(), (size_t)N)) ||
        (rc = dev_upload(h, &d_te, te.data(), te.size())) || (rc = dev_upload(h, &d_has, hd.data(), (size_t)N))) { cleanup(); return rc; }
    double *d_tip = d_tab, *d_dtip = d_tab + ntab, *d_d2tip = d_tab + 2 * ntab;
    hipLaunchKernelGGL(k_d2p, dim3(C * E), dim3(64), 0, h->stream, 4, E, d_Q2, h->d_Pdd, h->d_cat_rates, d_d2P);
    hipLaunchKernelGGL(k_build_tip, dim3(ntips + 1, C), dim3(64), 0, h->stream, E, ntips + 1, h->nchar, d_te, h->d_Pdd, h->d_defs, d_tip);
    hipLaunchKernelGGL(k_build_dtip4, dim3(ntips + 1, C), dim3(64), 0, h->stream, E, ntips, h->nchar, d_te, h->d_dP, h->d_defs, d_dtip, 1);
    hipLaunchKernelGGL(k_build_dtip4, dim3(ntips + 1, C), dim3(64), 0, h->stream, E, ntips, h->nchar, d_te, d_d2P, h->d_defs, d_d2tip, 1);
    if (hipGetLastError() != hipSuccess) { cleanup(); h->err = "plk_second_order: matrix set-up failed"; return PLK_E_DEVICE; }

    const int NMX = hess4_nm(E);
    const size_t vs1 = (size_t)nin * C * 4, sc1 = (size_t)nsc * C;        /* per site and model */
    const size_t per_model = 2 * vs1 + sc1 + 2 * (size_t)C + 2 + (size_t)E;
    const size_t per_site_d = (size_t)NMX * per_model;
    const size_t per_site = (per_site_d + 2 + (size_t)E) * sizeof(double);
    long chunk;
    if ((rc = plan_site_chunk(h, "plk_second_order", per_site, UD4_BLOCK, false, &chunk))) { cleanup(); return rc; }
    if ((rc = dev_reserve(h, &h->d_work, &h->work_cap, per_site_d * (size_t)chunk)) ||
        (rc = dev_alloc(h, &d_LH0, (size_t)chunk)) || (rc = dev_alloc(h, &d_XM0, (size_t)chunk)) ||
        (rc = dev_alloc(h, &d_D0, (size_t)E * chunk))) { cleanup(); return rc; }

    std::vector<dd> gh((size_t)E * E);
    for (long s0 = 0; s0 < S; s0 += chunk) {
        const long n = std::min(chunk, S - s0);
        Hess4Args a;
        a.Spad = h->Spad; a.s0 = s0; a.n = n;
        a.N = N; a.E = E; a.C = C; a.nchar = h->nchar; a.ntips = ntips; a.root_mode = h->root_mode;
        a.indptr = h->d_indptr; a.indices = h->d_indices; a.preorder = h->d_preorder;
        a.node_has_data = d_has; a.edge_tip = d_et; a.node_int = d_ni; a.node_scale = d_ns;
        a.P = h->d_P; a.dP = h->d_dP; a.d2P = d_d2P; a.tip = d_tip; a.dtip = d_dtip; a.d2tip = d_d2tip;
        a.codes = h->d_codes; a.cat_prior = h->d_cat_prior; a.root_w = h->d_root_w;
        a.vstride = vs1 * n; a.scstride = sc1 * n;
        double *p = h->d_work;
        a.LN = p; p += (size_t)NMX * vs1 * n;
        a.FN = p; p += (size_t)NMX * vs1 * n;
        a.SC = p; p += (size_t)NMX * sc1 * n;
        a.CW = p; p += (size_t)NMX * C * n;
        a.XC = p; p += (size_t)NMX * C * n;
        a.XM = p; p += (size_t)NMX * n;
        a.LH = p; p += (size_t)NMX * n;
        a.DV = p; p += (size_t)NMX * E * n;
        const unsigned grid = (unsigned)((n + UD4_BLOCK - 1) / UD4_BLOCK);
        const double *w = h->d_w ? h->d_w + s0 : nullptr;
        /* pass 0: the model itself -> f and g / f */
        for (int m = 0; m < H4_MAX_NM; m++) a.mod[m] = -1;
        a.LHdiv = nullptr; a.XMdiv = nullptr;
        launch_hess4<1>(h, a, grid);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(d_LH0, a.LH, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_XM0, a.XM, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_D0, a.DV, (size_t)E * n * sizeof(double), hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_gram, dim3(E, E), dim3(256), 0, h->stream, E, n, d_D0, w, d_G);
            e = hipMemcpyAsync(gh.data(), d_G, (size_t)E * E * sizeof(dd), hipMemcpyDeviceToHost, h->stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) { cleanup(); h->err = std::string("plk_second_order: ") + hipGetErrorString(e); return PLK_E_DEVICE; }
        for (int i = 0; i < E; i++)
            for (int j = 0; j <= i; j++) G[(size_t)i * E + j] += (long double)gh[(size_t)i * E + j].hi + (long double)gh[(size_t)i * E + j].lo;
        if (gsum && (rc = wsum_rows(h, E, n, d_D0, w, gsum))) { cleanup(); return rc; }
        /* rows j0 .. j0 + rows - 1 of the likelihood Hessian per launch, normalised by the unmodified likelihood */
        a.LHdiv = d_LH0; a.XMdiv = d_XM0;
        for (int j0 = 0; j0 < E;) {
            const int nm = hess4_nm(E - j0), rows = nm;
            for (int m = 0; m < H4_MAX_NM; m++) a.mod[m] = m < rows ? j0 + m : -1;
            if (nm == 4) launch_hess4<4>(h, a, grid);
            else if (nm == 2) launch_hess4<2>(h, a, grid);
            else launch_hess4<1>(h, a, grid);
            if (hipGetLastError() != hipSuccess) { cleanup(); h->err = "plk_second_order: kernel launch failed"; return PLK_E_DEVICE; }
            if ((rc = wsum_rows(h, rows * E, n, a.DV, w, Hrow.data() + (size_t)j0 * E))) { cleanup(); return rc; }
            j0 += rows;
        }
    }
    cleanup();
    return PLK_OK;
}

/*
 * Site-weighted gradient and Hessian from one run: pass 0 of the Hessian already produces g / f per site, so a
 * Newton step (src/arbplfhess.c:169-234 needs both) does not pay a separate derivative query.  k = 4 with compact
 * codes and at most four rate categories runs the one-thread-per-site pass of plk_hess4.h, everything else the
 * generic passes.
 */
extern "C" int plk_second_order(plk_engine *h, double *grad_sums_out /* [E][2] or NULL */, double *hess_sums_out /* [E][E][2] or NULL */)
{
    if (!plk_live(h) || (!grad_sums_out && !hess_sums_out)) return PLK_E_ARG;
    if (h->k == 0 || h->pat_mode == 0) { h->err = "plk_second_order: tree, model and patterns must be set"; return PLK_E_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    if (h->model_dirty) { if ((rc = run_expm(h))) return rc; }
    if ((rc = ensure_dP(h))) return rc;
    const int E = h->E;
    if (E == 0) return PLK_OK;
    if ((rc = check_stored_range(h, "plk_second_order/plk_hess"))) return rc;
    std::vector<long double> Hrow((size_t)E * E, 0.0L), G((size_t)E * E, 0.0L), gsum((size_t)E, 0.0L);
    if (use_hess4(h)) { h->info_updown_kernel = 5; rc = second_order_k4(h, Hrow, G, grad_sums_out ? gsum.data() : nullptr); }
    else { h->info_updown_kernel = 2; rc = second_order_generic(h, Hrow, G, grad_sums_out ? gsum.data() : nullptr); }
    if (rc) return rc;
    if (grad_sums_out) put_dd_rows(grad_sums_out, gsum.data(), gsum.size());
    if (hess_sums_out)
        for (int i = 0; i < E; i++)
            for (int j = 0; j <= i; j++) {
                /* both triangles of the likelihood Hessian were computed; average them */
                const long double v = (Hrow[(size_t)i * E + j] + Hrow[(size_t)j * E + i]) * 0.5L - G[(size_t)i * E + j];
                put_dd(hess_sums_out + 2 * ((size_t)i * E + j), v);
                put_dd(hess_sums_out + 2 * ((size_t)j * E + i), v);
            }
    return PLK_OK;
}

extern "C" int plk_hess(plk_engine *h, double *hess_sums_out /* [E][E][2] */)
{
    if (!hess_sums_out) return PLK_E_ARG;
    return plk_second_order(h, nullptr, hess_sums_out);
}
