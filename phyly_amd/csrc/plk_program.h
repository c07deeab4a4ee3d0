/*
 * plk_program.h -- the traversal program of the pruning kernels: builder, device formats and checkers.
 * Host-only C++ (no HIP types), included by plk_engine.hip and by the CPU test driver tests/progcheck_main.cpp.
 *
 * The reference walks the tree with pointers per site (src/evaluate_site_lhood.c:21-57 over the preorder of
 * src/model.h:62-67).  Here the walk is compiled once per query into a wave-uniform post-order *program* that the
 * kernels interpret for every site; the formats derived from it are what the device code indexes LDS, the matrix
 * stream, the tip tables and the register stack with.  Everything the device will dereference is therefore
 * decided on the host, and the plk_check_* functions below replay the interpreters' address arithmetic on the
 * host (same field widths, same look-ahead fetches) so that a program that would step outside a buffer is
 * refused with PLK_E_ARG before any launch.
 */
#ifndef PLK_PROGRAM_H
#define PLK_PROGRAM_H

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

/* traversal program opcodes */
enum {
    OP_TIP_SET = 0,   /* cur  = P_e * B_b         (b a leaf child)          */
    OP_TIP_MUL = 1,   /* cur *= P_e * B_b                                   */
    OP_MATVEC = 2,    /* cur  = P_e * cur         (b an internal child)     */
    OP_PUSH = 3,      /* slot[d] = cur                                      */
    OP_POPMUL = 4,    /* cur *= slot[d]                                     */
    OP_NODE_MUL = 5,  /* cur *= B_a               (internal node with data) */
    OP_SCALE = 6,     /* cur *= 2^-e, exponent accumulated (exact)          */
    OP_END = 7
};
/* handler 3 of the assembly interpreter's word format: TIP_MUL that may skip its wait (plk_fused4_asm.h) */
#define PLK_WORD_TIPMUL_NOWAIT 3u
#define PLK_WORD_SET_POPMUL 12u        /* + slot: TIP_SET and the POPMUL that follows it (two-sites-per-lane interpreter only) */
#define PLK_WORD_SET_PUSH 20u          /* + slot: TIP_SET and the PUSH that follows it */
#define PLK_WORD_MATVEC_TIPMUL 4u      /* assembly interpreter: MATVEC and the TIP_MUL that follows it, as one op word (handler slots 4 and 5) */

struct plk_op2 { int x, y; };          /* layout of HIP's int2: x = opcode | tip_slot << 8, y = node / stack slot */
struct plk_op4 { int x, y, z, w; };    /* layout of HIP's int4 */

#define PLK_TILE 256                   /* sites per workgroup of the fused k = 4 kernels */
#define PLK_FUSED_SLOTS 16             /* deepest register stack any fused kernel is compiled for */
#define PLK_LDS_LIMIT (150 * 1024)     /* dynamic LDS the fused kernels may ask for (160 KB per CU on gfx950) */

struct PlkProgram {
    std::vector<plk_op2> ops;
    std::vector<int> op_edge;          /* CSR edge per op or -1 */
    std::vector<int> tip_edge;         /* CSR edge per tip slot */
    std::vector<char> scale_node;      /* N: node vectors rescaled here (every >= 16 accumulated edges) */
    std::vector<char> mid_scale_node;  /* N: nodes with an OP_SCALE between two of their children (more than PLK_SCALE_RUN factors) */
    int mid_scales = 0;                /* number of such nodes; 0 on every tree whose nodes have at most two children */
    int wide_node = -1;                /* the first of them in program order, for messages */
    std::vector<char> op_mid;          /* per op: 1 for an OP_SCALE inside a node (the passes that store node vectors skip those) */
    std::vector<int> obs_nodes;        /* nodes whose code rows the fused kernels stage, in order of first use */
    int slots_needed = 0;              /* Sethi-Ullman number of the tree = depth of the waiting-vector stack */
};

/* most edge factors a vector takes between two rescalings: a node is rescaled once 16 have accumulated, so the product of
 * two children holds at most 2 * 16 */
#define PLK_SCALE_RUN 32

/*
 * Post-order program of a rooted tree in CSR form (preorder[0] = root, parents first).  Internal children are
 * visited in order of decreasing stack need, so the stack depth is the tree's Sethi-Ullman number (<= log2 of the
 * leaf count for binary trees).  node_has_data[a] != 0 for internal nodes whose observation row is not all ones.
 *
 * Rescaling: a node's vector is rescaled after its last child once 16 or more edge factors have accumulated since the
 * last rescaling below it (scale_node).  Under a node with many children that alone leaves the run unbounded, so an
 * OP_SCALE is also placed INSIDE a node, before the child whose factors would take the run past PLK_SCALE_RUN
 * (mid_scale_node).  A node whose run stays within PLK_SCALE_RUN gets none: every tree whose nodes have at most two
 * children has the program it had before the rule existed.
 */
static inline void plk_program_build(int N, const int *ip, const int *ix, const int *preorder,
                                     const char *node_has_data, PlkProgram &pg)
{
    std::vector<int> need(N, 0), since(N, 0);
    pg.scale_node.assign(N, 0);
    pg.mid_scale_node.assign(N, 0);
    pg.mid_scales = 0; pg.wide_node = -1;
    std::vector<std::vector<int>> ichild(N); /* internal children (CSR edge idx), sorted by need desc */
    for (int u = N - 1; u >= 0; u--) {
        const int a = preorder[u];
        if (ip[a + 1] == ip[a]) continue;
        std::vector<int> &ic = ichild[a];
        for (int idx = ip[a]; idx < ip[a + 1]; idx++)
            if (ip[ix[idx] + 1] > ip[ix[idx]]) ic.push_back(idx);
        std::stable_sort(ic.begin(), ic.end(), [&](int x, int y) { return need[ix[x]] > need[ix[y]]; });
        int nd = 0;
        for (size_t i = 0; i < ic.size(); i++) nd = std::max(nd, need[ix[ic[i]]] + (i > 0 ? 1 : 0));
        need[a] = nd;
        /* the run of factors in the order of emission below: first internal child, leaves, further internal children */
        int acc = 0;
        auto merge = [&](int add) { if (acc + add > PLK_SCALE_RUN) { acc = 0; pg.mid_scale_node[a] = 1; } acc += add; };
        if (!ic.empty()) merge(since[ix[ic[0]]] + 1);
        for (int idx = ip[a]; idx < ip[a + 1]; idx++) if (ip[ix[idx] + 1] == ip[ix[idx]]) merge(1);
        for (size_t i = 1; i < ic.size(); i++) merge(since[ix[ic[i]]] + 1);
        if (pg.mid_scale_node[a]) pg.mid_scales++;
        /* a node rescaled inside is always rescaled after its last child too: the passes that store node vectors, which skip
         * the inner ones, then look at its magnitude there */
        if (acc >= 16 || pg.mid_scale_node[a]) { pg.scale_node[a] = 1; acc = 0; }
        since[a] = acc;
    }
    const int root = preorder[0];
    pg.slots_needed = need[root];

    pg.ops.clear(); pg.op_edge.clear(); pg.tip_edge.clear(); pg.obs_nodes.clear(); pg.op_mid.clear();
    std::vector<int> obs_row(N, -1);
    auto obs = [&](int node) {
        if (obs_row[node] < 0) { obs_row[node] = (int)pg.obs_nodes.size(); pg.obs_nodes.push_back(node); }
        return obs_row[node];
    };
    auto emit = [&](int code, int tslot, int arg, int edge) {
        plk_op2 o; o.x = code | (tslot << 8); o.y = arg;
        pg.ops.push_back(o); pg.op_edge.push_back(edge); pg.op_mid.push_back(0);
    };
    /* iterative post-order emission; frame = (node, depth, stage) */
    struct Frame { int a, depth, stage; bool started; int run; };   /* run: factors in cur since its last OP_SCALE */
    std::vector<Frame> stk;
    stk.push_back({root, 0, 0, false, 0});
    /* OP_SCALE inside node a, before the child that brings `add` factors (the rule of merge() above) */
    auto mid_scale = [&](Frame &f, int add) {
        if (f.run + add > PLK_SCALE_RUN) {
            emit(OP_SCALE, 0, f.a, -1);
            pg.op_mid.back() = 1;
            f.run = 0;
            if (pg.wide_node < 0) pg.wide_node = f.a;
        }
        f.run += add;
    };
    while (!stk.empty()) {
        Frame &f = stk.back();
        const int a = f.a;
        const std::vector<int> &ic = ichild[a];
        if (f.stage == 0) {
            f.stage = 1;
            if (!ic.empty()) { const Frame nf = {ix[ic[0]], f.depth, 0, false, 0}; stk.push_back(nf); continue; }
        }
        if (f.stage == 1) {
            if (!ic.empty()) { emit(OP_MATVEC, 0, 0, ic[0]); f.started = true; f.run = since[ix[ic[0]]] + 1; }
            for (int idx = ip[a]; idx < ip[a + 1]; idx++) {
                const int b = ix[idx];
                if (ip[b + 1] > ip[b]) continue;
                const int t = (int)pg.tip_edge.size();
                pg.tip_edge.push_back(idx);
                mid_scale(f, 1);
                emit(f.started ? OP_TIP_MUL : OP_TIP_SET, t, b, idx);
                obs(b);
                f.started = true;
            }
            f.stage = 2;
        }
        if (f.stage >= 2) {
            const int i = f.stage - 1; /* next internal child index (>= 1) */
            if (f.stage > 2) { /* returning from child i-1 */
                emit(OP_MATVEC, 0, 0, ic[i - 1]);
                emit(OP_POPMUL, 0, f.depth, -1);
            }
            if (i < (int)ic.size()) {
                mid_scale(f, since[ix[ic[i]]] + 1);
                emit(OP_PUSH, 0, f.depth, -1);
                f.stage++;
                const Frame nf = {ix[ic[i]], f.depth + 1, 0, false, 0};
                stk.push_back(nf);      /* invalidates f */
                continue;
            }
            if (node_has_data[a]) { emit(OP_NODE_MUL, 0, a, -1); obs(a); }
            if (pg.scale_node[a]) emit(OP_SCALE, 0, a, -1);   /* y = the node (used by the storing down pass) */
            stk.pop_back();
        }
    }
}

static inline std::string plk_fmt(const char *fmt, long a = 0, long b = 0, long c = 0)
{
    char buf[256];
    snprintf(buf, sizeof buf, fmt, a, b, c);
    return std::string(buf);
}

/*
 * Invariants of the program itself, by abstract interpretation: every internal node's vector is completed exactly
 * once, every edge is applied exactly once, the stack is used as a stack inside [0, slots_needed), and the op
 * arguments name existing nodes / tip slots.  Returns "" when the program is well formed.
 */
static inline std::string plk_program_check(int N, const int *ip, const int *ix, const int *preorder,
                                            const char *node_has_data, const PlkProgram &pg)
{
    const int E = N - 1;
    const int nops = (int)pg.ops.size();
    if ((int)pg.op_edge.size() != nops || (int)pg.op_mid.size() != nops) return "program: op_edge size";
    if ((int)pg.scale_node.size() != N || (int)pg.mid_scale_node.size() != N) return "program: scale_node size";
    if (pg.slots_needed < 0) return "program: negative stack depth";
    std::vector<int> edge_seen(std::max(E, 1), 0), tip_seen(pg.tip_edge.size(), 0);
    std::vector<char> slot_full(std::max(pg.slots_needed, 1), 0);
    int depth = 0;
    bool have_cur = false;
    for (int pc = 0; pc < nops; pc++) {
        const int code = pg.ops[pc].x & 0xff, t = pg.ops[pc].x >> 8, y = pg.ops[pc].y, e = pg.op_edge[pc];
        switch (code) {
        case OP_TIP_SET: case OP_TIP_MUL:
            if (t < 0 || t >= (int)pg.tip_edge.size() || tip_seen[t]++) return plk_fmt("program: op %ld: bad tip slot %ld", pc, t);
            if (e != pg.tip_edge[t] || e < 0 || e >= E || ix[e] != y) return plk_fmt("program: op %ld: tip edge mismatch", pc);
            if (ip[y + 1] != ip[y]) return plk_fmt("program: op %ld: tip op on an internal node", pc);
            if (edge_seen[e]++) return plk_fmt("program: edge %ld applied twice", e);
            if ((code == OP_TIP_SET) == have_cur) return plk_fmt("program: op %ld: TIP_SET/TIP_MUL does not match the state", pc);
            have_cur = true;
            break;
        case OP_MATVEC:
            if (e < 0 || e >= E || edge_seen[e]++) return plk_fmt("program: op %ld: bad or repeated edge %ld", pc, e);
            if (ip[ix[e] + 1] == ip[ix[e]]) return plk_fmt("program: op %ld: MATVEC on a leaf edge", pc);
            if (!have_cur) return plk_fmt("program: op %ld: MATVEC without a vector", pc);
            break;
        case OP_PUSH:
            if (y != depth || y >= pg.slots_needed || slot_full[y] || !have_cur) return plk_fmt("program: op %ld: bad PUSH to slot %ld (depth %ld)", pc, y, depth);
            slot_full[y] = 1; depth++; have_cur = false;
            break;
        case OP_POPMUL:
            if (y != depth - 1 || y < 0 || !slot_full[y] || !have_cur) return plk_fmt("program: op %ld: bad POPMUL of slot %ld (depth %ld)", pc, y, depth);
            slot_full[y] = 0; depth--;
            break;
        case OP_NODE_MUL:
            if (y < 0 || y >= N || ip[y + 1] == ip[y] || !node_has_data[y] || !have_cur) return plk_fmt("program: op %ld: bad NODE_MUL", pc);
            break;
        case OP_SCALE:
            if (y < 0 || y >= N || !(pg.scale_node[y] || pg.mid_scale_node[y]) || !have_cur) return plk_fmt("program: op %ld: bad SCALE", pc);
            break;
        default:
            return plk_fmt("program: op %ld: unknown opcode %ld", pc, code);
        }
    }
    if (depth != 0) return "program: stack not empty at the end";
    if (E > 0 && !have_cur) return "program: no root vector";
    for (int e = 0; e < E; e++) if (edge_seen[e] != 1) return plk_fmt("program: edge %ld applied %ld times", e, edge_seen[e]);
    for (size_t r = 0; r < pg.obs_nodes.size(); r++)
        if (pg.obs_nodes[r] < 0 || pg.obs_nodes[r] >= N) return "program: staged row names a node out of range";
    (void)preorder;
    return "";
}

/* ------------------------------------------------------------------------------------------------------------ */
/* fused k = 4 kernels: int4 program of the C++ interpreter, 32-bit op words of the assembly interpreter           */
/* ------------------------------------------------------------------------------------------------------------ */

struct PlkFused {
    std::vector<plk_op4> fops;         /* x = opcode | tip<<8, y = row / slot, z = next observation row, w = matrix index */
    std::vector<int> mat_edge;         /* CSR edge per matrix of the compact stream (the kernels add one spare) */
    std::vector<unsigned> words;       /* blocks of 8, END padded, one spare block */
    int first_row = 0;
    int asm_first_tip = 0, asm_first_row = 0, asm_second_row = 0;
    bool asm_ok = false;               /* the assembly interpreter's field widths and stack depth suffice */
};

/* the assembly interpreter's op-word fields: 8 stack slots, 11 bits of tip slot, 16 bits of staged row */
static inline bool plk_fused_asm_ok(const PlkProgram &pg)
{
    return pg.slots_needed <= 8 && pg.tip_edge.size() + 1 < 2048 && pg.obs_nodes.size() < 65536;
}

static inline void plk_fused_build(int N, const PlkProgram &pg, PlkFused &fu)
{
    const int nops = (int)pg.ops.size();
    std::vector<int> row(N, -1);
    for (size_t r = 0; r < pg.obs_nodes.size(); r++) row[pg.obs_nodes[r]] = (int)r;
    /* C++ interpreter: ops are executed in pairs and fetched one pair ahead: even count + one spare pair */
    const int npad = ((nops + 1) / 2) * 2 + 2;
    fu.fops.assign(npad, plk_op4{OP_END, 0, 0, 0});
    fu.mat_edge.clear();
    int next_row = 0;
    for (int pc = nops - 1; pc >= 0; pc--) {
        const plk_op2 o = pg.ops[pc];
        const int code = o.x & 0xff;
        plk_op4 f = {o.x, o.y, next_row, 0};
        if (code == OP_TIP_SET || code == OP_TIP_MUL || code == OP_NODE_MUL) { f.y = row[o.y]; next_row = f.y; }
        fu.fops[pc] = f;
    }
    fu.first_row = next_row;
    for (int pc = 0; pc < nops; pc++)
        if ((fu.fops[pc].x & 0xff) == OP_MATVEC) { fu.fops[pc].w = (int)fu.mat_edge.size(); fu.mat_edge.push_back(pg.op_edge[pc]); }
    /* assembly interpreter: 32-bit words {handler index | y<<5 | z<<16} in blocks of 8 (handler index = opcode, or
     * 8 + slot for PUSH, 16 + slot for POPMUL: the interpreter jumps to base + 256 * index); an observation op carries
     * the tip slot of the NEXT observation op (y) and the code row of the one after next (z): the prefetch chain of
     * plk_fused4_asm.h.  An internal node's own data is an observation on the pseudo tip slot ntips. */
    const int ntips = (int)pg.tip_edge.size();
    std::vector<int> obs_t, obs_row;
    for (int pc = 0; pc < nops; pc++) {
        const int code = fu.fops[pc].x & 0xff;
        if (code == OP_TIP_SET || code == OP_TIP_MUL) { obs_t.push_back(fu.fops[pc].x >> 8); obs_row.push_back(fu.fops[pc].y); }
        else if (code == OP_NODE_MUL) { obs_t.push_back(ntips); obs_row.push_back(fu.fops[pc].y); }
    }
    const int nwords = ((nops + 1 + 7) / 8) * 8 + 8;
    fu.words.assign(nwords, (unsigned)OP_END);
    size_t oi = 0, nw = 0;
    bool matvec_since_obs = false;   /* a MATVEC (full wait) ran since the last observation op */
    for (int pc = 0; pc < nops; pc++) {
        const int code = fu.fops[pc].x & 0xff;
        unsigned wv = (unsigned)code;
        auto obs_fields = [&]() {
            const unsigned tn = oi + 1 < obs_t.size() ? (unsigned)obs_t[oi + 1] : 0u;
            const unsigned rn = oi + 2 < obs_row.size() ? (unsigned)obs_row[oi + 2] : 0u;
            return (tn << 5) | (rn << 16);
        };
        if (code == OP_MATVEC) {
            const int nx = pc + 1 < nops ? (fu.fops[pc + 1].x & 0xff) : OP_END;
            if ((nx == OP_TIP_MUL || nx == OP_NODE_MUL) && oi > 0) {
                /* MATVEC followed by TIP_MUL (an internal child, then a leaf child or the node's own data): one word,
                 * handler 3; the product's wait covers the prefetched tip value */
                fu.words[nw++] = PLK_WORD_MATVEC_TIPMUL | obs_fields();
                oi++;
                matvec_since_obs = false;
                pc++;
                continue;
            }
            matvec_since_obs = true;
            if ((nx == OP_PUSH || nx == OP_POPMUL) && pg.slots_needed <= 4) {
                /* MATVEC followed by PUSH / POPMUL (a node with two internal children): one word, handlers 24 + d /
                 * 28 + d of the 4-slot interpreter */
                fu.words[nw++] = (nx == OP_PUSH ? 24u : 28u) + (unsigned)fu.fops[pc + 1].y;
                pc++;
                continue;
            }
        }
        if (code == OP_TIP_SET || code == OP_TIP_MUL || code == OP_NODE_MUL) {
            const unsigned oc = code == OP_TIP_SET ? (unsigned)OP_TIP_SET
                                                   : (matvec_since_obs && oi > 0 ? PLK_WORD_TIPMUL_NOWAIT : (unsigned)OP_TIP_MUL);
            wv = oc | obs_fields();
            matvec_since_obs = false;
            oi++;
        } else if (code == OP_PUSH || code == OP_POPMUL) {
            wv = (code == OP_PUSH ? 8u : 16u) + (unsigned)fu.fops[pc].y;
        }
        fu.words[nw++] = wv;
    }
    fu.asm_first_tip = obs_t.empty() ? 0 : obs_t[0];
    fu.asm_first_row = obs_row.empty() ? 0 : obs_row[0];
    fu.asm_second_row = obs_row.size() > 1 ? obs_row[1] : 0;
    fu.asm_ok = plk_fused_asm_ok(pg);
}

/* dynamic LDS of the fused ll kernels: tip tables of ncat categories (ntips + the pseudo slot each) + staged code rows */
static inline size_t plk_fused_lds_bytes(const PlkProgram &pg, int nchar, int bytes_per_row, int ncat = 1)
{
    return (size_t)ncat * (pg.tip_edge.size() + 1) * nchar * 4 * sizeof(double) + pg.obs_nodes.size() * (size_t)bytes_per_row;
}

/* the observation sequence of the program: (tip slot incl. pseudo slot, staged row) per observation op */
static inline void plk_obs_sequence(int N, const PlkProgram &pg, std::vector<int> &slot, std::vector<int> &rowv, std::vector<int> &opc)
{
    std::vector<int> row(N, -1);
    for (size_t r = 0; r < pg.obs_nodes.size(); r++) row[pg.obs_nodes[r]] = (int)r;
    slot.clear(); rowv.clear(); opc.clear();
    for (size_t pc = 0; pc < pg.ops.size(); pc++) {
        const int code = pg.ops[pc].x & 0xff;
        if (code == OP_TIP_SET || code == OP_TIP_MUL) { slot.push_back(pg.ops[pc].x >> 8); rowv.push_back(row[pg.ops[pc].y]); opc.push_back(code); }
        else if (code == OP_NODE_MUL) { slot.push_back((int)pg.tip_edge.size()); rowv.push_back(row[pg.ops[pc].y]); opc.push_back(code); }
    }
}

/*
 * Replays k_ll_fused4_asm<D> (plk_fused4_asm.h) on the host: the block-ahead word fetch, the matrix stream that is
 * always one matrix ahead, the LDS addresses of the tip-value prefetch chain (for the largest code, nchar - 1) and of
 * the code bytes, the 13-bit / 16-bit fields, the AGPR slot numbers -- and checks that the values the chain delivers
 * to each observation op are the ones the program asks for.  pack4: two codes per staged byte (nchar <= 16).
 */
static inline std::string plk_fused_check_asm(int N, const PlkProgram &pg, const PlkFused &fu, int nchar, int D, int pack4,
                                              size_t lds_bytes_launched, int ncat_lds = 1)
{
    const int nops = (int)pg.ops.size(), ntips1 = (int)pg.tip_edge.size() + 1, nobs = (int)pg.obs_nodes.size();
    const int nmat = (int)fu.mat_edge.size();
    if (nchar < 1 || nchar > 256) return "asm program: nchar out of range";
    if (pack4 && nchar > 16) return "asm program: 4-bit codes need nchar <= 16";
    if (D != 4 && D != 8) return "asm program: stack depth variant";
    if (pg.slots_needed > D) return "asm program: the tree needs a deeper register stack";
    if (fu.words.size() % 8 != 0 || (int)fu.words.size() < ((nops + 1 + 7) / 8) * 8 + 8) return "asm program: word buffer too short";
    const size_t row_bytes = pack4 ? PLK_TILE / 2 : PLK_TILE;
    const size_t tip_bytes = (size_t)ntips1 * nchar * 32, code_bytes = (size_t)nobs * row_bytes;
    if (ncat_lds < 1) return "asm program: categories per pass";
    if ((size_t)ncat_lds * tip_bytes + code_bytes > lds_bytes_launched) return "asm program: LDS image larger than the launch's dynamic LDS";
    if (lds_bytes_launched > PLK_LDS_LIMIT) return "asm program: dynamic LDS above the limit";
    if (nobs < 1) return "asm program: no observation rows";
    std::vector<int> slot, rowv, opc;
    plk_obs_sequence(N, pg, slot, rowv, opc);
    auto tip_ok = [&](long t) { return t >= 0 && t < ntips1 && (size_t)t * nchar * 32 + (size_t)(nchar - 1) * 32 + 32 <= tip_bytes; };
    auto row_ok = [&](long r) { return r >= 0 && r < nobs && (size_t)r * row_bytes + (row_bytes - 1) < code_bytes; };
    if (!tip_ok(fu.asm_first_tip) || !row_ok(fu.asm_first_row) || !row_ok(fu.asm_second_row)) return "asm program: prologue prefetch out of range";
    /* prefetch chain state: value in flight = (cur_tip, cur_row), code in flight = next_row */
    long cur_tip = fu.asm_first_tip, cur_row = fu.asm_first_row, next_row = fu.asm_second_row;
    size_t oi = 0;
    int mi = 0;                       /* matrix currently loaded; the kernel loads mi + 1 after each MATVEC */
    bool waited = true;               /* lgkmcnt(0) seen since the in-flight value was requested (prologue waits) */
    std::vector<char> full(D, 0);
    const size_t nblocks = fu.words.size() / 8;
    size_t pc = 0;                    /* op of the program the next word stands for (a pair word stands for two) */
    /* one observation op of the chain: the word's fields name the next observation's slot and the row after next */
    auto observation = [&](size_t wi, unsigned y, unsigned z, bool is_set, bool no_wait) -> std::string {
        if ((int)pc >= nops) return "asm program: op beyond the program";
        const int code = pg.ops[pc].x & 0xff;
        if (code != OP_TIP_SET && code != OP_TIP_MUL && code != OP_NODE_MUL) return plk_fmt("asm program: word %ld is not an observation op", (long)wi);
        if (is_set != (code == OP_TIP_SET)) return plk_fmt("asm program: word %ld: SET/MUL mismatch", (long)wi);
        if (no_wait && !waited) return plk_fmt("asm program: word %ld skips a wait it needs", (long)wi);
        if (oi >= slot.size() || cur_tip != slot[oi] || cur_row != rowv[oi]) return plk_fmt("asm program: prefetch chain delivers the wrong observation at word %ld", (long)wi);
        if (!tip_ok(y) || !row_ok(z)) return plk_fmt("asm program: word %ld prefetches out of range (slot %ld, row %ld)", (long)wi, y, z);
        cur_tip = y; cur_row = next_row; next_row = z;
        if (oi + 1 < slot.size() && (cur_tip != slot[oi + 1] || cur_row != rowv[oi + 1])) return plk_fmt("asm program: chain after word %ld", (long)wi);
        oi++;
        waited = false;
        pc++;
        return "";
    };
    auto product = [&](size_t wi) -> std::string {
        if ((int)pc >= nops) return "asm program: op beyond the program";
        if ((pg.ops[pc].x & 0xff) != OP_MATVEC) return plk_fmt("asm program: word %ld is not the program's op", (long)wi);
        if (mi >= nmat || fu.mat_edge[mi] != pg.op_edge[pc]) return plk_fmt("asm program: matrix %ld is not the op's edge", mi);
        mi++;                                   /* loads matrix mi (<= nmat: the spare) */
        waited = true;
        pc++;
        return "";
    };
    for (size_t b = 0;; b++) {
        if (b + 1 >= nblocks) return "asm program: ran past the spare block (no END)";
        /* s_load_dwordx8 of block b + 1 is issued here: in range by the test above */
        for (int i = 0; i < 8; i++) {
            const size_t wi = b * 8 + i;
            const unsigned w = fu.words[wi];
            /* the kernel jumps to handler (w & 31): 0..7 = opcode (3 = TIP_MUL without wait, 4 = MATVEC + TIP_MUL, occupying slots 4 and 5),
             * 8 + d = PUSH slot d, 16 + d = POPMUL slot d, 24 + d / 28 + d = MATVEC then PUSH / POPMUL slot d (4-slot
             * interpreter only) */
            const unsigned hidx = w & 31, z = w >> 16;
            if (hidx == 5 || (hidx >= 24 && D != 4)) return plk_fmt("asm program: word %ld jumps to an empty handler slot", (long)wi);
            const unsigned y = hidx >= 24 ? (hidx & 3) : hidx >= 8 ? (hidx & 7) : (w >> 5) & 0x7ff;
            std::string bad;
            if (hidx == OP_END) {
                if ((int)pc != nops) return plk_fmt("asm program: END at word %ld after %ld of the program's ops", (long)wi, (long)pc);
                if (oi != slot.size()) return "asm program: observation ops missing";
                if (mi != nmat) return "asm program: matrix stream not consumed";
                return "";
            } else if (hidx == OP_MATVEC) bad = product(wi);
            else if (hidx == PLK_WORD_MATVEC_TIPMUL) { bad = product(wi); if (bad.empty()) bad = observation(wi, y, z, false, true); }
            else if (hidx == OP_TIP_SET || hidx == OP_TIP_MUL || hidx == PLK_WORD_TIPMUL_NOWAIT) bad = observation(wi, y, z, hidx == OP_TIP_SET, hidx == PLK_WORD_TIPMUL_NOWAIT);
            else if (hidx == OP_SCALE) { if ((int)pc >= nops || (pg.ops[pc].x & 0xff) != OP_SCALE) bad = plk_fmt("asm program: word %ld is not the program's op", (long)wi); pc++; }
            else {
                if (hidx >= 24) { bad = product(wi); if (!bad.empty()) return bad; }         /* MATVEC + PUSH / POPMUL */
                const bool push = hidx >= 24 ? hidx < 28 : hidx < 16;
                if ((int)pc >= nops || (pg.ops[pc].x & 0xff) != (push ? OP_PUSH : OP_POPMUL) || (int)y >= D || (int)y != pg.ops[pc].y || (full[y] != 0) == push)
                    bad = plk_fmt(push ? "asm program: bad PUSH at word %ld" : "asm program: bad POPMUL at word %ld", (long)wi);
                else full[y] = push;
                pc++;
            }
            if (!bad.empty()) return bad;
        }
        waited = true;                /* s_waitcnt lgkmcnt(0) at the end of every block */
    }
}

/* ------------------------------------------------------------------------------------------------------------ */
/* pair-table interpreter k_ll_fused4_asm_pt (plk_fused4_asm.h): 512-site tiles, byte rows, cherries as look-ups     */
/* ------------------------------------------------------------------------------------------------------------ */

/* dynamic LDS the pair-table kernels may ask for, by sites per tile: one workgroup per CU (1024 sites on 1024 lanes, or
 * 1024 / 1536 sites on 512 / 768 lanes with two sites each), or two 512-site workgroups */
static inline size_t plk_pt_lds_limit(int tile) { return tile >= 1024 ? (size_t)156 * 1024 : (size_t)78 * 1024; }
static inline bool plk_pt_tile_ok(int tile) { return tile == 512 || tile == 1024 || tile == 1536; }

struct PlkFusedPT {
    std::vector<unsigned> words;       /* blocks of 8, END padded, one spare block (format of PlkFused::words; the y field
                                          counts table UNITS of nchar * 32 bytes) */
    std::vector<int> mat_edge;         /* CSR edge per matrix of the stream (the kernel adds one spare) */
    std::vector<int> row_node, row_node2;   /* staged rows: node | second node of a pair row or -1 */
    /* tables of one category, in unit order: a single leaf (1 unit: P_e defs), a pair (nchar units:
     * P_a (P_b defs[i] o P_c defs[j]) at code i * nchar + j) or the pseudo table (1 unit: the raw definitions) */
    std::vector<int> tab_unit, tab_edge, tab_eb, tab_ec;   /* first unit | leaf edge, edge above the cherry or -1 | pair: leaf edges, else -1 */
    int units = 0, npairs = 0;
    /* three-leaf tables (plk_fused_v4t_build only; empty lists = none): a node d whose children are a cherry a = (b, c) and a
     * leaf l, with the edge above d, as nchar * nchar units: P_d ((pair row of a) o (tip row of l)) at code
     * (code_b * nchar + code_c) * nchar + code_l.  tab_edge = the edge above d, tab_eb / tab_ec the cherry's leaf edges,
     * tab_ea the edge above the cherry, tab_el the leaf edge; row_node3 = l in the row of (b, c, l) */
    std::vector<int> row_node3, tab_ea, tab_el;
    int ntriples = 0;
    /* four-leaf tables (plk_fused_v4q_build only; empty lists = none): a node d with four leaves below it, each of which takes
     * at most four of the nchar codes, with the edge above d, as 256 rows in ceil(256 / nchar) units.  The row index is in
     * fixed radix 4 over the leaves' RANKS, ((r1 * 4 + r2) * 4 + r3) * 4 + r4, in the order row_node, row_node2, row_node3,
     * row_node4 of the row; lut[64 q + 16 j + code] is the rank of `code` at leaf j of four-leaf table q (row_lut[row] = q,
     * -1 for every other row): the rank of an occurring code among the leaf's occurring codes in increasing order, 0 for a
     * code that does not occur.
     *   shape A (PLK_V4Q_A): d = (t, l2), t = (a, l1), a = (b, c): leaves b, c, l1, l2; tab_edge above d, tab_et above t, tab_ea
     *            above a, tab_eb / tab_ec / tab_el / tab_ef the leaf edges of b, c, l1, l2
     *   shape B (PLK_V4Q_B): d = (a, a'), a = (b, c), a' = (f, g): leaves b, c, f, g; tab_edge above d, tab_ea above a, tab_et
     *            above a', tab_eb / tab_ec / tab_ef / tab_eg the leaf edges (tab_el = -1) */
    std::vector<int> row_node4, row_lut, tab_shape, tab_et, tab_ef, tab_eg;
    std::vector<int> tab_row;          /* per table: the staged row of the one look-up that reads a four-leaf table (its leaves, its rank tables), else -1 */
    std::vector<uint8_t> lut;
    int nquads = 0;
    int first_unit = 0, first_row = 0, second_row = 0;
    /* the program after folding the cherries, op by op (what the words encode; the vector kernel's int4 program is made from it) */
    struct VOp { int code, unit, row, d, edge; };
    std::vector<VOp> vops;
};

/* the node whose CSR child range holds edge idx */
static inline int plk_edge_parent(int N, const int *ip, int idx)
{
    int lo = 0, hi = N - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) / 2; if (ip[mid] <= idx) lo = mid; else hi = mid - 1; }
    return lo;
}

/* does the program continue at pc with TIP_SET(b), TIP_MUL(c), MATVEC(edge into a) for a node a whose only children
 * are the leaves b and c? */
static inline bool plk_pair_at(int N, const int *ip, const int *ix, const PlkProgram &pg, size_t pc)
{
    if (pc + 2 >= pg.ops.size()) return false;
    if ((pg.ops[pc].x & 0xff) != OP_TIP_SET || (pg.ops[pc + 1].x & 0xff) != OP_TIP_MUL || (pg.ops[pc + 2].x & 0xff) != OP_MATVEC) return false;
    const int eb = pg.op_edge[pc], ec = pg.op_edge[pc + 1], ea = pg.op_edge[pc + 2];
    const int a = plk_edge_parent(N, ip, eb);
    if (ip[a + 1] - ip[a] != 2 || plk_edge_parent(N, ip, ec) != a || eb == ec) return false;
    return ea >= 0 && ix[ea] == a;
}

/* the 32-bit op words and the prologue fields of fu.vops (tables and rows are in place) */
static inline void plk_fused_pt_words(int slots_needed, bool fuse_set, PlkFusedPT &fu)
{
    const std::vector<PlkFusedPT::VOp> &v = fu.vops;
    std::vector<int> ou, orow;
    for (const PlkFusedPT::VOp &o : v) if (o.code == OP_TIP_SET || o.code == OP_TIP_MUL) { ou.push_back(o.unit); orow.push_back(o.row); }
    const int nv = (int)v.size();
    fu.words.assign(((nv + 1 + 7) / 8) * 8 + 8, (unsigned)OP_END);
    size_t oi = 0, nw = 0;
    bool matvec_since_obs = false;
    for (int i = 0; i < nv; i++) {
        const int code = v[i].code;
        unsigned wv = (unsigned)code;
        auto obs_fields = [&]() {
            /* cyclic: the last observations request the first ones again, so that every request of the chain pairs a
             * table with a row of its own kind (the values are dropped; the next category's prologue asks again) */
            const unsigned un = (unsigned)ou[(oi + 1) % ou.size()];
            const unsigned rn = (unsigned)orow[(oi + 2) % orow.size()];
            return (un << 5) | (rn << 16);
        };
        if (code == OP_MATVEC) {
            const int nx = i + 1 < nv ? v[i + 1].code : OP_END;
            if (nx == OP_TIP_MUL && oi > 0) {
                fu.words[nw++] = PLK_WORD_MATVEC_TIPMUL | obs_fields();
                oi++; matvec_since_obs = false; i++;
                continue;
            }
            matvec_since_obs = true;
            if ((nx == OP_PUSH || nx == OP_POPMUL) && slots_needed <= 4) {
                fu.words[nw++] = (nx == OP_PUSH ? 24u : 28u) + (unsigned)v[i + 1].d;
                i++;
                continue;
            }
        }
        if (code == OP_TIP_SET || code == OP_TIP_MUL) {
            unsigned oc = code == OP_TIP_SET ? (unsigned)OP_TIP_SET
                                             : (matvec_since_obs && oi > 0 ? PLK_WORD_TIPMUL_NOWAIT : (unsigned)OP_TIP_MUL);
            const int nx = i + 1 < nv ? v[i + 1].code : OP_END;
            if (fuse_set && code == OP_TIP_SET && (nx == OP_POPMUL || nx == OP_PUSH)) {
                /* TIP_SET followed by POPMUL / PUSH (a look-up as the last or as an earlier internal child): one word, handlers
                 * 12 + d / 20 + d of the two-sites-per-lane interpreter; the value goes straight into the product / the slot */
                oc = (nx == OP_POPMUL ? PLK_WORD_SET_POPMUL : PLK_WORD_SET_PUSH) + (unsigned)v[i + 1].d;
                i++;
            }
            wv = oc | obs_fields();
            matvec_since_obs = false;
            oi++;
        } else if (code == OP_PUSH || code == OP_POPMUL) {
            wv = (code == OP_PUSH ? 8u : 16u) + (unsigned)v[i].d;
        }
        fu.words[nw++] = wv;
    }
    fu.first_unit = ou.empty() ? 0 : ou[0];
    fu.first_row = orow.empty() ? 0 : orow[0];
    fu.second_row = orow.size() > 1 ? orow[1] : 0;
}

/* max_pairs: how many cherries may become tables (LDS budget); nchar * nchar <= 256 is the caller's business */
static inline void plk_fused_pt_build(int N, const int *ip, const int *ix, const PlkProgram &pg, int nchar, int max_pairs, PlkFusedPT &fu,
                                      bool fuse_set = false)
{
    const int nops = (int)pg.ops.size();
    typedef PlkFusedPT::VOp VOp;
    std::vector<VOp> &v = fu.vops;
    v.clear();
    fu.mat_edge.clear(); fu.row_node.clear(); fu.row_node2.clear();
    fu.tab_unit.clear(); fu.tab_edge.clear(); fu.tab_eb.clear(); fu.tab_ec.clear();
    fu.units = 0; fu.npairs = 0;
    fu.row_node3.clear(); fu.tab_ea.clear(); fu.tab_el.clear(); fu.ntriples = 0;
    fu.row_node4.clear(); fu.row_lut.clear(); fu.tab_shape.clear(); fu.tab_et.clear(); fu.tab_ef.clear(); fu.tab_eg.clear(); fu.tab_row.clear(); fu.lut.clear(); fu.nquads = 0;
    std::vector<int> row_of(N, -1);
    auto single_row = [&](int node) {
        if (row_of[node] < 0) { row_of[node] = (int)fu.row_node.size(); fu.row_node.push_back(node); fu.row_node2.push_back(-1); }
        return row_of[node];
    };
    auto table = [&](int edge, int eb, int ec, int nunits) {
        fu.tab_unit.push_back(fu.units); fu.tab_edge.push_back(edge); fu.tab_eb.push_back(eb); fu.tab_ec.push_back(ec);
        const int u = fu.units; fu.units += nunits; return u;
    };
    int pseudo_unit = -1;
    for (int pc = 0; pc < nops; pc++) {
        const int code = pg.ops[pc].x & 0xff;
        if (code == OP_TIP_SET && fu.npairs < max_pairs && plk_pair_at(N, ip, ix, pg, (size_t)pc)) {
            const int row = (int)fu.row_node.size();
            fu.row_node.push_back(pg.ops[pc].y); fu.row_node2.push_back(pg.ops[pc + 1].y);
            v.push_back(VOp{OP_TIP_SET, table(pg.op_edge[pc + 2], pg.op_edge[pc], pg.op_edge[pc + 1], nchar), row, 0, -1});
            fu.npairs++;
            pc += 2;
        } else if (code == OP_TIP_SET || code == OP_TIP_MUL) {
            v.push_back(VOp{code, table(pg.op_edge[pc], -1, -1, 1), single_row(pg.ops[pc].y), 0, -1});
        } else if (code == OP_NODE_MUL) {
            if (pseudo_unit < 0) pseudo_unit = table(-1, -1, -1, 1);
            v.push_back(VOp{OP_TIP_MUL, pseudo_unit, single_row(pg.ops[pc].y), 0, -1});
        } else if (code == OP_MATVEC) {
            fu.mat_edge.push_back(pg.op_edge[pc]);
            v.push_back(VOp{OP_MATVEC, 0, 0, 0, pg.op_edge[pc]});
        } else {
            v.push_back(VOp{code, 0, 0, pg.ops[pc].y, -1});
        }
    }
    if (pseudo_unit < 0) table(-1, -1, -1, 1);      /* always present: keeps the image non-empty and the layout regular */
    plk_fused_pt_words(pg.slots_needed, fuse_set, fu);
}

static inline size_t plk_fused_pt_lds_bytes(const PlkFusedPT &fu, int nchar, int tile)
{
    return (size_t)fu.units * nchar * 32 + fu.row_node.size() * (size_t)tile;
}

/*
 * Replays k_ll_fused4_asm_pt on the host against the PROGRAM (not against the builder's intermediate list): block-ahead
 * word fetch, matrix stream one ahead, LDS addresses of the value / code prefetch chain for the largest code of every
 * table, field widths, stack slots; every observation word must deliver the table and the staged row of the program's
 * next leaf op -- or, for a pair table, stand for exactly TIP_SET(b), TIP_MUL(c), MATVEC(edge above) of one cherry.
 */
static inline std::string plk_fused_check_pt(int N, const int *ip, const int *ix, const PlkProgram &pg, const PlkFusedPT &fu, int nchar,
                                             int tile, size_t lds_bytes_launched, bool fused_set_words = false, bool rows_in_lds = true)
{
    if (!rows_in_lds) tile = 1;            /* streamed codes (k_ll_fused4_v4s): rows are indices only, the LDS holds C table images */
    const int nops = (int)pg.ops.size(), nrows = (int)fu.row_node.size(), nmat = (int)fu.mat_edge.size(), ntab = (int)fu.tab_unit.size();
    if (nchar < 1 || nchar > 16) return "pt program: pair tables need nchar <= 16";
    if (pg.slots_needed > 4) return "pt program: the tree needs a deeper register stack";
    if (fu.words.size() % 8 != 0 || fu.words.size() < 16) return "pt program: word buffer";
    if ((int)fu.row_node2.size() != nrows || (int)fu.tab_edge.size() != ntab || (int)fu.tab_eb.size() != ntab || (int)fu.tab_ec.size() != ntab) return "pt program: table sizes";
    const size_t tip_bytes = (size_t)fu.units * nchar * 32, code_bytes = (size_t)nrows * tile;
    if (rows_in_lds && tip_bytes + code_bytes > lds_bytes_launched) return "pt program: LDS image larger than the launch's dynamic LDS";
    if (rows_in_lds && (!plk_pt_tile_ok(tile) || lds_bytes_launched > plk_pt_lds_limit(tile))) return "pt program: dynamic LDS above the limit";
    if (nrows < 1 || fu.units < 1 || fu.units >= 2048 || nrows >= 65536) return "pt program: field widths";
    for (int r = 0; r < nrows; r++)
        if (fu.row_node[r] < 0 || fu.row_node[r] >= N || fu.row_node2[r] < -1 || fu.row_node2[r] >= N) return "pt program: staged row names a node out of range";
    /* tables tile the unit range without gaps */
    std::vector<int> table_at(fu.units, -1);
    int expect = 0;
    for (int t = 0; t < ntab; t++) {
        const int nu = fu.tab_eb[t] >= 0 ? nchar : 1;
        if (fu.tab_unit[t] != expect || expect + nu > fu.units) return "pt program: table layout";
        table_at[expect] = t;
        expect += nu;
    }
    if (expect != fu.units) return "pt program: table layout";
    auto unit_ok = [&](long u) {
        if (u < 0 || u >= fu.units || table_at[u] < 0) return false;
        const long ncodes = fu.tab_eb[table_at[u]] >= 0 ? (long)nchar * nchar : nchar;
        return (size_t)u * nchar * 32 + (size_t)ncodes * 32 <= tip_bytes;
    };
    auto row_ok = [&](long r) { return r >= 0 && r < nrows && (size_t)r * tile + (tile - 1) < code_bytes; };
    if (!unit_ok(fu.first_unit) || !row_ok(fu.first_row) || !row_ok(fu.second_row)) return "pt program: prologue prefetch out of range";
    if (fu.row_node2[fu.first_row] >= 0 && fu.tab_eb[table_at[fu.first_unit]] < 0) return "pt program: the prologue indexes a one-unit table with a pair row's code";
    long cur_unit = fu.first_unit, cur_row = fu.first_row, next_row = fu.second_row;
    int mi = 0;
    bool waited = true, any_obs = false;
    std::vector<char> full(4, 0), tab_used(ntab, 0);
    const size_t nblocks = fu.words.size() / 8;
    size_t pc = 0;
    auto code_at = [&](size_t q) { return q < (size_t)nops ? (pg.ops[q].x & 0xff) : (int)OP_END; };
    auto observation = [&](size_t wi, unsigned y, unsigned z, bool is_set, bool no_wait) -> std::string {
        if (no_wait && !waited) return plk_fmt("pt program: word %ld skips a wait it needs", (long)wi);
        if (!unit_ok(cur_unit) || !row_ok(cur_row)) return plk_fmt("pt program: word %ld consumes an observation out of range", (long)wi);
        const int t = table_at[cur_unit];
        if (tab_used[t]++ && fu.tab_edge[t] >= 0) return plk_fmt("pt program: table %ld used twice", (long)t);
        const int code = code_at(pc);
        if (fu.tab_eb[t] >= 0) {
            /* a pair: the program must continue with the cherry's three ops */
            if (!is_set || !plk_pair_at(N, ip, ix, pg, pc)) return plk_fmt("pt program: word %ld is a pair look-up where the program has no cherry", (long)wi);
            if (fu.tab_eb[t] != pg.op_edge[pc] || fu.tab_ec[t] != pg.op_edge[pc + 1] || fu.tab_edge[t] != pg.op_edge[pc + 2]) return plk_fmt("pt program: pair table %ld holds other edges than the cherry at word %ld", (long)t, (long)wi);
            if (fu.row_node[cur_row] != pg.ops[pc].y || fu.row_node2[cur_row] != pg.ops[pc + 1].y) return plk_fmt("pt program: pair row of word %ld", (long)wi);
            pc += 3;
        } else {
            if (code != OP_TIP_SET && code != OP_TIP_MUL && code != OP_NODE_MUL) return plk_fmt("pt program: word %ld is not an observation op", (long)wi);
            if (is_set != (code == OP_TIP_SET)) return plk_fmt("pt program: word %ld: SET/MUL mismatch", (long)wi);
            if (fu.row_node[cur_row] != pg.ops[pc].y || fu.row_node2[cur_row] != -1) return plk_fmt("pt program: word %ld reads the wrong staged row", (long)wi);
            if (fu.tab_edge[t] != (code == OP_NODE_MUL ? -1 : pg.op_edge[pc])) return plk_fmt("pt program: word %ld reads the wrong table", (long)wi);
            pc++;
        }
        /* what the word requests: the value of the next observation = table y at the code that is in flight (row next_row),
         * and the code of the observation after that (row z).  A pair row's codes reach nchar^2 - 1: only a pair table holds them. */
        if (!unit_ok(y) || !row_ok(z) || !row_ok(next_row)) return plk_fmt("pt program: word %ld prefetches out of range (unit %ld, row %ld)", (long)wi, y, z);
        if (fu.row_node2[next_row] >= 0 && fu.tab_eb[table_at[y]] < 0) return plk_fmt("pt program: word %ld indexes a one-unit table with a pair row's code", (long)wi);
        cur_unit = y; cur_row = next_row; next_row = z;
        waited = false; any_obs = true;
        return "";
    };
    auto product = [&](size_t wi) -> std::string {
        if (code_at(pc) != OP_MATVEC) return plk_fmt("pt program: word %ld is not the program's op", (long)wi);
        if (mi >= nmat || fu.mat_edge[mi] != pg.op_edge[pc]) return plk_fmt("pt program: matrix %ld is not the op's edge", mi);
        mi++; waited = true; pc++;
        return "";
    };
    for (size_t b = 0;; b++) {
        if (b + 1 >= nblocks) return "pt program: ran past the spare block (no END)";
        for (int i = 0; i < 8; i++) {
            const size_t wi = b * 8 + i;
            const unsigned w = fu.words[wi];
            const unsigned hidx = w & 31, z = w >> 16;
            if (hidx == 5) return plk_fmt("pt program: word %ld jumps to an empty handler slot", (long)wi);
            const bool setstack = (hidx >= PLK_WORD_SET_POPMUL && hidx < PLK_WORD_SET_POPMUL + 4) || (hidx >= PLK_WORD_SET_PUSH && hidx < PLK_WORD_SET_PUSH + 4);
            if (setstack && !fused_set_words) return plk_fmt("pt program: word %ld jumps to an empty handler slot", (long)wi);
            const unsigned y = setstack ? (w >> 5) & 0x7ff : hidx >= 24 ? (hidx & 3) : hidx >= 8 ? (hidx & 7) : (w >> 5) & 0x7ff;
            std::string bad;
            if (setstack) {
                /* TIP_SET (single or pair look-up), then POPMUL / PUSH of slot hidx & 3 */
                bad = observation(wi, y, z, true, false);
                if (!bad.empty()) return bad;
                const bool push = hidx >= PLK_WORD_SET_PUSH;
                const unsigned d = hidx & 3;
                if (code_at(pc) != (push ? OP_PUSH : OP_POPMUL) || (int)d != pg.ops[pc].y || (full[d] != 0) == push)
                    return plk_fmt(push ? "pt program: bad SET + PUSH at word %ld" : "pt program: bad SET + POPMUL at word %ld", (long)wi);
                full[d] = push;
                pc++;
                continue;
            }
            if (hidx == OP_END) {
                if ((int)pc != nops) return plk_fmt("pt program: END at word %ld after %ld of the program's ops", (long)wi, (long)pc);
                if (mi != nmat) return "pt program: matrix stream not consumed";
                for (int t = 0; t < ntab; t++) if (fu.tab_edge[t] >= 0 && tab_used[t] != 1) return plk_fmt("pt program: table %ld is never read", (long)t);
                (void)any_obs;
                return "";
            } else if (hidx == OP_MATVEC) bad = product(wi);
            else if (hidx == PLK_WORD_MATVEC_TIPMUL) { bad = product(wi); if (bad.empty()) bad = observation(wi, y, z, false, true); }
            else if (hidx == OP_TIP_SET || hidx == OP_TIP_MUL || hidx == PLK_WORD_TIPMUL_NOWAIT) bad = observation(wi, y, z, hidx == OP_TIP_SET, hidx == PLK_WORD_TIPMUL_NOWAIT);
            else if (hidx == OP_SCALE) { if (code_at(pc) != OP_SCALE) bad = plk_fmt("pt program: word %ld is not the program's op", (long)wi); pc++; }
            else {
                if (hidx >= 24) { bad = product(wi); if (!bad.empty()) return bad; }
                const bool push = hidx >= 24 ? hidx < 28 : hidx < 16;
                if (code_at(pc) != (push ? OP_PUSH : OP_POPMUL) || (int)y >= 4 || (int)y != pg.ops[pc].y || (full[y] != 0) == push)
                    bad = plk_fmt(push ? "pt program: bad PUSH at word %ld" : "pt program: bad POPMUL at word %ld", (long)wi);
                else full[y] = push;
                pc++;
            }
            if (!bad.empty()) return bad;
        }
        waited = true;
    }
}

/*
 * 64-bit ops of the two-sites-per-lane interpreter k_ll_fused4_v4 (plk_fused4_v4.h), a re-encoding of PlkFusedPT::words:
 *   lo = handler index * 512;  hi (observation ops) = (LDS offset / 32 of the next observation's table) << 16 |
 *        (offset / 64 of the code row after next, relative to row 0);  tip_base = LDS byte address of the table image.
 */
#define PLK_V4_HANDLER_BYTES 512
#define PLK_V4_HANDLER_SLOTS 64
#define PLK_V4_REFILL_A 32
#define PLK_V4_REFILL_B 33
struct PlkFusedV4 {
    std::vector<unsigned> words;       /* 2 dwords per op, blocks of 7 ops + 1 REFILL op, two spare blocks */
    unsigned first_y = 0, first_z = 0, second_z = 0;
};

static inline bool plk_word_is_obs(unsigned hidx)
{
    return hidx == OP_TIP_SET || hidx == OP_TIP_MUL || hidx == PLK_WORD_TIPMUL_NOWAIT || hidx == PLK_WORD_MATVEC_TIPMUL ||
           (hidx >= PLK_WORD_SET_POPMUL && hidx < PLK_WORD_SET_POPMUL + 4) || (hidx >= PLK_WORD_SET_PUSH && hidx < PLK_WORD_SET_PUSH + 4);
}

/* Threaded op stream of k_ll_fused4_v4: blocks of 8 ops = 7 ops of the program + one REFILL op (REFILL_A in even blocks,
 * REFILL_B in odd ones: the handler that requests the block after next into its own half of the kernel's op ring); the
 * program's ops up to its END, END padding to the end of that block, then two spare blocks (the ring reads two ahead). */
static inline void plk_fused_v4_words(const PlkFusedPT &fu, int nchar, int tile, unsigned tip_base, PlkFusedV4 &v4)
{
    const unsigned tb32 = tip_base / 32, rg = (unsigned)tile / 64;
    size_t nreal = 0;
    while (nreal < fu.words.size() && (fu.words[nreal] & 31) != OP_END) nreal++;
    nreal++;                                                  /* the END itself */
    const size_t nblocks = (nreal + 6) / 7 + 2;
    v4.words.assign(nblocks * 16, 0u);
    size_t src = 0;
    for (size_t b = 0; b < nblocks; b++)
        for (int j = 0; j < 8; j++) {
            unsigned *o = &v4.words[(b * 8 + j) * 2];
            if (j == 7) { o[0] = (unsigned)((b & 1) ? PLK_V4_REFILL_B : PLK_V4_REFILL_A) * PLK_V4_HANDLER_BYTES; continue; }
            const unsigned w = src < nreal && src < fu.words.size() ? fu.words[src] : (unsigned)OP_END, hidx = w & 31;
            src++;
            o[0] = hidx * PLK_V4_HANDLER_BYTES;
            if (plk_word_is_obs(hidx)) o[1] = ((tb32 + ((w >> 5) & 0x7ff) * (unsigned)nchar) << 16) | ((w >> 16) * rg);
        }
    v4.first_y = tb32 + (unsigned)fu.first_unit * (unsigned)nchar;
    v4.first_z = (unsigned)fu.first_row * rg;
    v4.second_z = (unsigned)fu.second_row * rg;
}

/* the 32-bit program is checked by plk_fused_check_pt; this checks the re-encoding: the stream is the program's ops in
 * order with a REFILL op of the right kind closing every block, an END is reached, two whole blocks follow the block of the
 * END (what the ring has requested by then), every field fits its 16 bits, is the 32-bit word's field times its granule,
 * and the byte addresses the kernel forms from it stay inside the launch's LDS */
static inline std::string plk_fused_check_v4(const PlkFusedPT &fu, const PlkFusedV4 &v4, int nchar, int tile, unsigned tip_base,
                                             size_t lds_bytes_launched)
{
    if (tip_base % 32 != 0 || tile % 64 != 0) return "v4 program: LDS base or tile granule";
    if (v4.words.size() % 16 != 0 || v4.words.size() < 48) return "v4 program: word count";
    const size_t tip_bytes = (size_t)fu.units * nchar * 32, lds_end = tip_base + lds_bytes_launched;
    const unsigned tb32 = tip_base / 32, rg = (unsigned)tile / 64;
    auto y_ok = [&](unsigned y, unsigned unit) { return y == tb32 + unit * (unsigned)nchar && y < 65536u && (size_t)y * 32 >= tip_base && (size_t)y * 32 < tip_base + tip_bytes; };
    auto z_ok = [&](unsigned z, unsigned row) { return z == row * rg && z < 65536u && tip_base + tip_bytes + (size_t)z * 64 + (size_t)tile <= lds_end; };
    if (!y_ok(v4.first_y, (unsigned)fu.first_unit) || !z_ok(v4.first_z, (unsigned)fu.first_row) || !z_ok(v4.second_z, (unsigned)fu.second_row)) return "v4 program: prologue fields";
    const size_t nblocks = v4.words.size() / 16;
    size_t src = 0;
    long end_block = -1;
    for (size_t b = 0; b < nblocks; b++)
        for (int j = 0; j < 8; j++) {
            const unsigned lo = v4.words[(b * 8 + j) * 2], hi = v4.words[(b * 8 + j) * 2 + 1];
            if (lo % PLK_V4_HANDLER_BYTES != 0 || lo >= (unsigned)PLK_V4_HANDLER_SLOTS * PLK_V4_HANDLER_BYTES) return plk_fmt("v4 program: handler offset in block %ld", (long)b);
            const unsigned hidx = lo / PLK_V4_HANDLER_BYTES;
            if (j == 7) {
                if (hidx != (unsigned)((b & 1) ? PLK_V4_REFILL_B : PLK_V4_REFILL_A) || hi != 0) return plk_fmt("v4 program: block %ld does not end in its REFILL op", (long)b);
                continue;
            }
            if (hidx >= 32) return plk_fmt("v4 program: REFILL op inside block %ld", (long)b);
            if (end_block >= 0) { if (hidx != OP_END || hi != 0) return "v4 program: ops after END"; continue; }
            if (src >= fu.words.size()) return "v4 program: more ops than the program";
            const unsigned w = fu.words[src++];
            if (hidx != (w & 31)) return plk_fmt("v4 program: op %ld is not the program's", (long)(src - 1));
            if (hidx == OP_END) { if (hi != 0) return "v4 program: stray fields in END"; end_block = (long)b; continue; }
            if (!plk_word_is_obs(hidx)) { if (hi != 0) return plk_fmt("v4 program: stray fields in op %ld", (long)(src - 1)); continue; }
            if (!y_ok(hi >> 16, (w >> 5) & 0x7ff) || !z_ok(hi & 0xffff, w >> 16)) return plk_fmt("v4 program: fields of op %ld", (long)(src - 1));
        }
    if (end_block < 0) return "v4 program: no END";
    if ((size_t)end_block + 2 >= nblocks) return "v4 program: fewer than two spare blocks after the END";
    return "";
}

/*
 * Streamed codes: k_ll_fused4_v4s (plk_fused4_v4s.h) keeps the tables of ALL categories in LDS and no code rows; the codes
 * of the observation ops reach the interpreter through registers, from a stream in global memory that is built when the
 * formats are uploaded (k_build_code_stream).  A wave walks 128-site UNITS (lane l carries sites 128 u + l and
 * 128 u + 64 + l).  Observation n of the program (in program order; its staged row is obs_row[n], a pair row's byte is
 * code(b) * nchar + code(c)) is byte n % 4 of the site's dword in chunk n / 4; a chunk is one wave-wide 8-byte load,
 *   dword index = ((unit * chunks + chunk) * 64 + lane) * 2 + half,
 * and a unit has ceil(nobs / 4) chunks and PLK_V4S_AHEAD spare ones, which the interpreter's prefetch reads past the end.
 * Op words as for k_ll_fused4_v4, one stream per category (stride dwords apart); an observation op's hi dword is
 *   (LDS offset / 32 of the NEXT observation's table in that category's image) << 16 | bit offset of the NEXT
 *   observation's code in its dword (the last observation names itself: its look-up is repeated and dropped),
 * and an ADVANCE_k op (handler PLK_V4S_ADVANCE + k, k alternating from 0) stands before the observation op that
 * extracts byte 0 of a new chunk: it waits for the older of the two chunks in flight, makes it the current dword and
 * requests the chunk after next.
 */
#define PLK_V4S_ADVANCE 34
#define PLK_V4S_CHUNK_BYTES 512
#define PLK_V4S_UNIT 128               /* sites per unit */
#define PLK_V4S_AHEAD 2                /* chunks in flight next to the current one = spare chunks of a unit */
#ifdef __HIPCC__
#define PLK_HD __host__ __device__
#else
#define PLK_HD
#endif

PLK_HD static inline int plk_stream_chunks(int nobs) { return (nobs + 3) / 4 + PLK_V4S_AHEAD; }
PLK_HD static inline size_t plk_stream_dword(size_t unit, int chunk, int lane, int half, int chunks)
{
    return ((unit * (size_t)chunks + (size_t)chunk) * 64 + (size_t)lane) * 2 + (size_t)half;
}
/* byte offset of (unit, chunk, lane, site half, byte) in the stream */
PLK_HD static inline size_t plk_stream_byte(size_t unit, int chunk, int lane, int half, int byte, int chunks)
{
    return plk_stream_dword(unit, chunk, lane, half, chunks) * 4 + (size_t)byte;
}
/* the dword of chunk `chunk` for one site: the bytes of observations 4 chunk .. 4 chunk + 3, 0 past the last;
 * row_nodes = [nlists][nrows] as uploaded (node | second node of a pair row or -1 | with nlists = 3: third node of a
 * three-leaf row or -1; the byte of (b, c, l) is (code_b * nchar + code_c) * nchar + code_l), codes = [N][Spad].
 * With nlists = 5 and luts: fourth node of a four-leaf row or -1 | index q of the row's rank tables or -1; the byte of such a
 * row is ((r1 * 4 + r2) * 4 + r3) * 4 + r4 with r_j = luts[64 q + 16 j + code at the row's j-th node] (PlkFusedPT::lut) */
PLK_HD static inline unsigned plk_stream_site_dword(const uint8_t *codes, size_t Spad, size_t site, const int *obs_row, int nobs,
                                                    const int *row_nodes, int nrows, int nchar, int chunk, int nlists = 2,
                                                    const uint8_t *luts = nullptr)
{
    unsigned d = 0;
    for (int b = 0; b < 4; b++) {
        const int n = 4 * chunk + b;
        if (n >= nobs) break;
        const int row = obs_row[n], nb = row_nodes[row], nc = row_nodes[nrows + row];
        const int q = nlists > 4 && luts ? row_nodes[4 * nrows + row] : -1;
        if (q >= 0) {
            const uint8_t *lu = luts + (size_t)q * 64;
            unsigned code = 0;
            for (int j = 0; j < 4; j++) code = code * 4u + (lu[16 * j + (codes[(size_t)row_nodes[j * nrows + row] * Spad + site] & 15u)] & 3u);
            d |= code << (8 * b);
            continue;
        }
        unsigned code = codes[(size_t)nb * Spad + site];
        if (nc >= 0) code = code * (unsigned)nchar + codes[(size_t)nc * Spad + site];
        const int nl = nlists > 2 ? row_nodes[2 * nrows + row] : -1;
        if (nl >= 0) code = code * (unsigned)nchar + codes[(size_t)nl * Spad + site];
        d |= (code & 0xffu) << (8 * b);
    }
    return d;
}

struct PlkFusedV4S {
    std::vector<unsigned> words;       /* C streams of stride dwords: 2 dwords per op, blocks of 7 ops + 1 REFILL op, two spare blocks */
    size_t stride = 0;
    std::vector<int> obs_row;          /* staged row of observation n, program order */
    std::vector<unsigned> first_y;     /* per category: LDS offset / 32 of the first observation's table */
    int nobs = 0, chunks = 0, C = 0;
    int Cg = 0;                        /* categories whose tables are resident at a time (C unless the kernel runs them in groups):
                                          category c reads the image of c % Cg */
};

/* codes of table t: nchar (one leaf, the pseudo table), nchar^2 (a cherry), nchar^3 (a three-leaf table) or 256 (a four-leaf table) */
#define PLK_V4Q_A 1
#define PLK_V4Q_B 2
#define PLK_V4Q_ROWS 256
static inline size_t plk_pt_table_codes(const PlkFusedPT &fu, size_t t, int nchar)
{
    if (t < fu.tab_shape.size() && fu.tab_shape[t] != 0) return (size_t)PLK_V4Q_ROWS;
    if (t < fu.tab_el.size() && fu.tab_el[t] >= 0) return (size_t)nchar * nchar * nchar;
    return fu.tab_eb[t] >= 0 ? (size_t)nchar * nchar : (size_t)nchar;
}
/* allocation units of nchar rows that table t takes */
static inline int plk_pt_table_units(const PlkFusedPT &fu, size_t t, int nchar)
{
    return (int)((plk_pt_table_codes(fu, t, nchar) + (size_t)nchar - 1) / (size_t)nchar);
}

static inline size_t plk_fused_v4s_lds_bytes(const PlkFusedPT &fu, int nchar, int C) { return (size_t)C * fu.units * nchar * 32; }

static inline void plk_fused_v4s_words(const PlkFusedPT &fu, int nchar, int C, unsigned tip_base, PlkFusedV4S &vs, int Cg = 0)
{
    if (Cg < 1 || Cg > C) Cg = C;
    vs.Cg = Cg;
    std::vector<unsigned> ou;
    vs.obs_row.clear();
    for (const PlkFusedPT::VOp &o : fu.vops) if (o.code == OP_TIP_SET || o.code == OP_TIP_MUL) { ou.push_back((unsigned)o.unit); vs.obs_row.push_back(o.row); }
    const int nobs = (int)ou.size();
    vs.nobs = nobs; vs.chunks = plk_stream_chunks(nobs); vs.C = C;
    /* ops of one category with table fields relative to the category's image: {handler, unit * nchar << 16 | bit offset} */
    struct Op { unsigned h, hi; bool obs; };
    std::vector<Op> ops;
    int oi = 0;
    for (size_t src = 0; src < fu.words.size(); src++) {
        const unsigned w = fu.words[src], hidx = w & 31;
        if (hidx == OP_END) break;
        if (!plk_word_is_obs(hidx) || oi >= nobs) { ops.push_back(Op{hidx, 0u, false}); continue; }
        const int next = oi + 1 < nobs ? oi + 1 : oi;
        if (next != oi && next % 4 == 0) ops.push_back(Op{(unsigned)PLK_V4S_ADVANCE + (unsigned)((next / 4 - 1) & 1), 0u, false});
        ops.push_back(Op{hidx, ((ou[next] * (unsigned)nchar) << 16) | (unsigned)(8 * (next % 4)), true});
        oi++;
    }
    ops.push_back(Op{(unsigned)OP_END, 0u, false});
    const size_t nblocks = (ops.size() + 6) / 7 + 2;
    vs.stride = nblocks * 16;
    vs.words.assign((size_t)C * vs.stride, 0u);
    vs.first_y.assign(C, 0u);
    const unsigned tb32 = tip_base / 32, cat32 = (unsigned)fu.units * (unsigned)nchar;
    for (int c = 0; c < C; c++) {
        const unsigned base = tb32 + (unsigned)(c % Cg) * cat32;
        unsigned *o = &vs.words[(size_t)c * vs.stride];
        size_t src = 0;
        for (size_t b = 0; b < nblocks; b++)
            for (int j = 0; j < 8; j++, o += 2) {
                if (j == 7) { o[0] = (unsigned)((b & 1) ? PLK_V4_REFILL_B : PLK_V4_REFILL_A) * PLK_V4_HANDLER_BYTES; continue; }
                const Op op = src < ops.size() ? ops[src] : Op{(unsigned)OP_END, 0u, false};
                src++;
                o[0] = op.h * PLK_V4_HANDLER_BYTES;
                if (op.obs) o[1] = op.hi + (base << 16);
            }
        vs.first_y[c] = base + (nobs ? ou[0] : 0u) * (unsigned)nchar;
    }
}

/* Replays the streamed interpreter's fetches against the 32-bit program (which plk_fused_check_pt has checked against the
 * tree's program: the chain of its row and table fields names, observation by observation, the staged row and the
 * table of the program's op -- a pair row and a pair table for a cherry's three ops).  For every category: the stream is
 * the program's ops in order with a REFILL op closing every block, an END and two spare blocks after its block; every
 * observation op extracts the byte of the next observation's row (obs_row = the chain's rows) from the chunk that is
 * the current one, which was requested two ADVANCEs (or the prologue) earlier and waited for; no request goes past the
 * unit's chunks; table fields fit 16 bits and the LDS address of the largest code stays inside C x table bytes. */
static inline std::string plk_fused_check_v4s(const PlkFusedPT &fu, const PlkFusedV4S &vs, int nchar, int C, unsigned tip_base,
                                              size_t lds_bytes_launched)
{
    if (tip_base % 32 != 0) return "v4s program: LDS base granule";
    if (C < 1 || vs.C != C || vs.stride % 16 != 0 || vs.stride < 48 || vs.words.size() != (size_t)C * vs.stride || (int)vs.first_y.size() != C) return "v4s program: word count";
    const int Cg = vs.Cg;
    if (Cg < 1 || Cg > C) return "v4s program: categories per group";
    const size_t tip_bytes = (size_t)fu.units * nchar * 32;
    if ((size_t)Cg * tip_bytes > lds_bytes_launched || tip_base + lds_bytes_launched > plk_pt_lds_limit(1024)) return "v4s program: table images larger than the launch's dynamic LDS";
    /* the chain of the 32-bit words: row and unit of every observation */
    std::vector<long> crow, cunit;
    std::vector<size_t> real;          /* indices of the program's words up to the END */
    {
        crow.push_back(fu.first_row); crow.push_back(fu.second_row); cunit.push_back(fu.first_unit);
        size_t w = 0;
        for (; w < fu.words.size() && (fu.words[w] & 31) != OP_END; w++) {
            real.push_back(w);
            if (plk_word_is_obs(fu.words[w] & 31)) { cunit.push_back((fu.words[w] >> 5) & 0x7ff); crow.push_back(fu.words[w] >> 16); }
        }
        if (w == fu.words.size()) return "v4s program: no END in the 32-bit program";
    }
    const int nobs = (int)cunit.size() - 1;
    if (nobs < 1 || vs.nobs != nobs || (int)vs.obs_row.size() != nobs) return "v4s program: observation count";
    if (vs.chunks != plk_stream_chunks(nobs) || PLK_V4S_AHEAD >= vs.chunks) return "v4s program: chunks of a unit";
    for (int n = 0; n < nobs; n++) if (vs.obs_row[n] != crow[n] || crow[n] < 0 || crow[n] >= (long)fu.row_node.size()) return plk_fmt("v4s program: observation %ld streams another row than the program reads", n);
    std::vector<size_t> unit_codes(fu.units, (size_t)nchar);
    for (size_t t = 0; t < fu.tab_unit.size(); t++) if (fu.tab_unit[t] >= 0 && fu.tab_unit[t] < fu.units) unit_codes[fu.tab_unit[t]] = plk_pt_table_codes(fu, t, nchar);
    const unsigned tb32 = tip_base / 32, cat32 = (unsigned)fu.units * (unsigned)nchar;
    const size_t nblocks = vs.stride / 16;
    for (int c = 0; c < C; c++) {
        const int cl = c % Cg;             /* the image the category reads */
        const unsigned base = tb32 + (unsigned)cl * cat32;
        auto y_ok = [&](unsigned y, long unit) {
            if (unit < 0 || unit >= fu.units || y != base + (unsigned)unit * (unsigned)nchar || y >= 65536u) return false;
            const size_t ncodes = unit_codes[unit];
            return (size_t)y * 32 >= tip_base + (size_t)cl * tip_bytes && ((size_t)y + ncodes) * 32 <= tip_base + (size_t)(cl + 1) * tip_bytes;
        };
        if (!y_ok(vs.first_y[c], cunit[0])) return "v4s program: prologue table field";
        const unsigned *wd = &vs.words[(size_t)c * vs.stride];
        /* prologue: chunk 0 is waited for and current, chunks 1 .. AHEAD are in flight */
        int cur = 0, requested = PLK_V4S_AHEAD, nadv = 0, oi = 0;
        if (requested >= vs.chunks) return "v4s program: the prologue reads past the unit";
        size_t src = 0;
        long end_block = -1;
        for (size_t b = 0; b < nblocks; b++)
            for (int j = 0; j < 8; j++) {
                const unsigned lo = wd[(b * 8 + j) * 2], hi = wd[(b * 8 + j) * 2 + 1];
                if (lo % PLK_V4_HANDLER_BYTES != 0 || lo >= (unsigned)PLK_V4_HANDLER_SLOTS * PLK_V4_HANDLER_BYTES) return plk_fmt("v4s program: handler offset in block %ld", (long)b);
                const unsigned hidx = lo / PLK_V4_HANDLER_BYTES;
                if (j == 7) {
                    if (hidx != (unsigned)((b & 1) ? PLK_V4_REFILL_B : PLK_V4_REFILL_A) || hi != 0) return plk_fmt("v4s program: block %ld does not end in its REFILL op", (long)b);
                    continue;
                }
                if (end_block >= 0) { if (hidx != OP_END || hi != 0) return "v4s program: ops after END"; continue; }
                if (hidx == (unsigned)PLK_V4S_ADVANCE || hidx == (unsigned)PLK_V4S_ADVANCE + 1) {
                    if (hi != 0 || hidx - PLK_V4S_ADVANCE != (unsigned)(nadv & 1)) return plk_fmt("v4s program: ADVANCE %ld of the wrong kind", nadv);
                    /* the older chunk in flight becomes current; the chunk after the ones in flight is requested */
                    cur = requested - (PLK_V4S_AHEAD - 1);
                    requested++;
                    if (requested >= vs.chunks) return plk_fmt("v4s program: ADVANCE %ld reads past the unit's chunks", nadv);
                    nadv++;
                    continue;
                }
                if (hidx >= 32) return plk_fmt("v4s program: REFILL op inside block %ld", (long)b);
                if (hidx == OP_END) {
                    if (hi != 0) return "v4s program: stray fields in END";
                    if (src != real.size() || oi != nobs) return "v4s program: END before the program's last op";
                    end_block = (long)b;
                    continue;
                }
                if (src >= real.size()) return "v4s program: more ops than the program";
                const unsigned w = fu.words[real[src++]];
                if (hidx != (w & 31)) return plk_fmt("v4s program: op %ld is not the program's", (long)(src - 1));
                if (!plk_word_is_obs(hidx)) { if (hi != 0) return plk_fmt("v4s program: stray fields in op %ld", (long)(src - 1)); continue; }
                if (oi >= nobs) return "v4s program: more observation ops than observations";
                const int next = oi + 1 < nobs ? oi + 1 : oi;
                if ((hi & 0xffffu) != (unsigned)(8 * (next % 4))) return plk_fmt("v4s program: observation %ld extracts the wrong byte", oi);
                if (cur != next / 4) return plk_fmt("v4s program: observation %ld extracts from chunk %ld, its code is in chunk %ld", oi, cur, next / 4);
                if (!y_ok(hi >> 16, cunit[next])) return plk_fmt("v4s program: table field of observation %ld", oi);
                oi++;
            }
        if (end_block < 0) return "v4s program: no END";
        if ((size_t)end_block + 2 >= nblocks) return "v4s program: fewer than two spare blocks after the END";
    }
    return "";
}

/*
 * The FOLDED op stream of k_ll_fused4_v4s: the checked stream above with fewer dispatches.  An ADVANCE_k op is removed and
 * the observation op after it goes to handler PLK_V4S_FOLD_ADV + 2 j + k (j = plk_v4s_obs_index of its handler: the same
 * arithmetic, ADVANCE_k, then the same extraction); a SCALE op after MATVEC + POPMUL slot d is removed and that op goes to
 * handler PLK_V4S_FOLD_SCALE + d.  A SCALE after any other op keeps its own dispatch.  The result is cut into blocks of
 * 7 ops and a REFILL again (two spare blocks), so a REFILL between the two ops of a pair does not stop the fold.  The
 * fields of the ops are not touched: stream layout, byte offsets and table fields are the checked stream's.
 */
#define PLK_V4S_FOLD_ADV 36
#define PLK_V4S_FOLD_SCALE 60

struct PlkV4SOp { unsigned h, hi; };           /* handler index, field dword */

static inline int plk_v4s_obs_index(unsigned hidx)
{
    if (hidx == OP_TIP_SET) return 0;
    if (hidx == OP_TIP_MUL) return 1;
    if (hidx == PLK_WORD_TIPMUL_NOWAIT) return 2;
    if (hidx == PLK_WORD_MATVEC_TIPMUL) return 3;
    if (hidx >= PLK_WORD_SET_POPMUL && hidx < PLK_WORD_SET_POPMUL + 4) return 4 + (int)(hidx - PLK_WORD_SET_POPMUL);
    if (hidx >= PLK_WORD_SET_PUSH && hidx < PLK_WORD_SET_PUSH + 4) return 8 + (int)(hidx - PLK_WORD_SET_PUSH);
    return -1;
}
static inline unsigned plk_v4s_obs_handler(int j)
{
    static const unsigned first[4] = {OP_TIP_SET, OP_TIP_MUL, PLK_WORD_TIPMUL_NOWAIT, PLK_WORD_MATVEC_TIPMUL};
    return j < 4 ? first[j] : j < 8 ? PLK_WORD_SET_POPMUL + (unsigned)(j - 4) : PLK_WORD_SET_PUSH + (unsigned)(j - 8);
}

/* the ops of one category's stream up to (without) its END, REFILL ops left out; false: no END, or a handler offset off its grid */
static inline bool plk_v4s_stream_ops(const unsigned *wd, size_t stride, std::vector<PlkV4SOp> &ops)
{
    ops.clear();
    for (size_t i = 0; i < stride / 2; i++) {
        if (i % 8 == 7) continue;
        const unsigned lo = wd[2 * i];
        if (lo % PLK_V4_HANDLER_BYTES != 0) return false;
        if (lo / PLK_V4_HANDLER_BYTES == OP_END) return true;
        ops.push_back(PlkV4SOp{lo / PLK_V4_HANDLER_BYTES, wd[2 * i + 1]});
    }
    return false;
}

static inline void plk_v4s_fold_ops(const std::vector<PlkV4SOp> &in, std::vector<PlkV4SOp> &out)
{
    out.clear();
    int pending = -1;                                     /* kind of the ADVANCE waiting for its observation op */
    for (const PlkV4SOp &op : in) {
        if (pending >= 0) {
            const int j = plk_v4s_obs_index(op.h);
            if (j >= 0) { out.push_back(PlkV4SOp{(unsigned)(PLK_V4S_FOLD_ADV + 2 * j + pending), op.hi}); pending = -1; continue; }
            out.push_back(PlkV4SOp{(unsigned)(PLK_V4S_ADVANCE + pending), 0u});
            pending = -1;
        }
        if (op.h == (unsigned)PLK_V4S_ADVANCE || op.h == (unsigned)PLK_V4S_ADVANCE + 1) { pending = (int)(op.h - PLK_V4S_ADVANCE); continue; }
        if (op.h == OP_SCALE && !out.empty() && out.back().h >= 28 && out.back().h < 32) { out.back().h += PLK_V4S_FOLD_SCALE - 28; continue; }
        out.push_back(op);
    }
    if (pending >= 0) out.push_back(PlkV4SOp{(unsigned)(PLK_V4S_ADVANCE + pending), 0u});
}

/* what a folded op list executes, one handler's work per entry: the list plk_v4s_fold_ops was given, if it is a fold of one */
static inline void plk_v4s_unfold_ops(const std::vector<PlkV4SOp> &in, std::vector<PlkV4SOp> &out)
{
    out.clear();
    for (const PlkV4SOp &op : in) {
        if (op.h >= PLK_V4S_FOLD_ADV && op.h < PLK_V4S_FOLD_SCALE) {
            out.push_back(PlkV4SOp{(unsigned)PLK_V4S_ADVANCE + ((op.h - PLK_V4S_FOLD_ADV) & 1), 0u});
            out.push_back(PlkV4SOp{plk_v4s_obs_handler((int)(op.h - PLK_V4S_FOLD_ADV) / 2), op.hi});
        } else if (op.h >= PLK_V4S_FOLD_SCALE && op.h < PLK_V4S_FOLD_SCALE + 4) {
            out.push_back(PlkV4SOp{28u + (op.h - PLK_V4S_FOLD_SCALE), op.hi});
            out.push_back(PlkV4SOp{(unsigned)OP_SCALE, 0u});
        } else out.push_back(op);
    }
}

/* blocks of 7 ops + REFILL (A in even blocks, B in odd ones), the END, END padding, two spare blocks */
static inline size_t plk_v4s_block_stride(size_t nops) { return ((nops + 1 + 6) / 7 + 2) * 16; }
static inline void plk_v4s_block_ops(const std::vector<PlkV4SOp> &ops, unsigned *o, size_t stride)
{
    size_t src = 0;
    for (size_t b = 0; b < stride / 16; b++)
        for (int j = 0; j < 8; j++, o += 2) {
            o[0] = o[1] = 0u;
            if (j == 7) { o[0] = (unsigned)((b & 1) ? PLK_V4_REFILL_B : PLK_V4_REFILL_A) * PLK_V4_HANDLER_BYTES; continue; }
            if (src < ops.size()) { o[0] = ops[src].h * PLK_V4_HANDLER_BYTES; o[1] = ops[src].hi; }
            else o[0] = (unsigned)OP_END * PLK_V4_HANDLER_BYTES;
            src++;
        }
}

struct PlkFusedV4SFold {
    std::vector<unsigned> words;       /* C streams of stride dwords, as PlkFusedV4S::words */
    size_t stride = 0;
    int nadv[2] = {0, 0};              /* folded ADVANCE_0 / ADVANCE_1 of one category */
    int standalone_adv = 0, standalone_scale = 0;
    unsigned scale_slots = 0;          /* bit d: MATVEC + POPMUL slot d + SCALE occurs */
};

/* vs: a stream plk_fused_check_v4s has accepted */
static inline void plk_fused_v4s_fold(const PlkFusedV4S &vs, PlkFusedV4SFold &fo)
{
    fo = PlkFusedV4SFold();
    std::vector<PlkV4SOp> ops, folded;
    for (int c = 0; c < vs.C; c++) {
        if (!plk_v4s_stream_ops(&vs.words[(size_t)c * vs.stride], vs.stride, ops)) { fo = PlkFusedV4SFold(); return; }
        plk_v4s_fold_ops(ops, folded);
        if (c == 0) {
            fo.stride = plk_v4s_block_stride(folded.size());
            fo.words.assign((size_t)vs.C * fo.stride, 0u);
            for (const PlkV4SOp &op : folded) {
                if (op.h >= PLK_V4S_FOLD_ADV && op.h < PLK_V4S_FOLD_SCALE) fo.nadv[(op.h - PLK_V4S_FOLD_ADV) & 1]++;
                else if (op.h >= PLK_V4S_FOLD_SCALE && op.h < PLK_V4S_FOLD_SCALE + 4) fo.scale_slots |= 1u << (op.h - PLK_V4S_FOLD_SCALE);
                else if (op.h == OP_SCALE) fo.standalone_scale++;
                else if (op.h == (unsigned)PLK_V4S_ADVANCE || op.h == (unsigned)PLK_V4S_ADVANCE + 1) fo.standalone_adv++;
            }
        } else if (plk_v4s_block_stride(folded.size()) != fo.stride) { fo = PlkFusedV4SFold(); return; }
        plk_v4s_block_ops(folded, &fo.words[(size_t)c * fo.stride], fo.stride);
    }
}

/* Replays the folded stream against the checked one: every block ends in its REFILL (A, B, A, ... from A), handler offsets
 * are on the grid and inside the table, an END is reached with two whole blocks after its block and nothing but END
 * after it, and the ops, unfolded, are the checked stream's ops exactly -- handlers in order (so a folded ADVANCE has the
 * kind of the op it replaces, and a + SCALE variant stands where a SCALE followed), table fields and bit offsets. */
static inline std::string plk_fused_check_v4s_fold(const PlkFusedV4S &vs, const PlkFusedV4SFold &fo)
{
    if (fo.stride % 16 != 0 || fo.stride < 48 || fo.words.size() != (size_t)vs.C * fo.stride) return "v4s fold: word count";
    std::vector<PlkV4SOp> want, got, un;
    for (int c = 0; c < vs.C; c++) {
        const unsigned *wd = &fo.words[(size_t)c * fo.stride];
        const size_t nblocks = fo.stride / 16;
        long end_block = -1;
        got.clear();
        for (size_t b = 0; b < nblocks; b++)
            for (int j = 0; j < 8; j++) {
                const unsigned lo = wd[(b * 8 + j) * 2], hi = wd[(b * 8 + j) * 2 + 1];
                if (lo % PLK_V4_HANDLER_BYTES != 0 || lo >= (unsigned)PLK_V4_HANDLER_SLOTS * PLK_V4_HANDLER_BYTES) return plk_fmt("v4s fold: handler offset in block %ld", (long)b);
                const unsigned hidx = lo / PLK_V4_HANDLER_BYTES;
                if (j == 7) {
                    if (hidx != (unsigned)((b & 1) ? PLK_V4_REFILL_B : PLK_V4_REFILL_A) || hi != 0) return plk_fmt("v4s fold: block %ld does not end in its REFILL op", (long)b);
                    continue;
                }
                if (hidx == (unsigned)PLK_V4_REFILL_A || hidx == (unsigned)PLK_V4_REFILL_B) return plk_fmt("v4s fold: REFILL op inside block %ld", (long)b);
                if (end_block >= 0) { if (hidx != OP_END || hi != 0) return "v4s fold: ops after END"; continue; }
                if (hidx == OP_END) { if (hi != 0) return "v4s fold: stray fields in END"; end_block = (long)b; continue; }
                got.push_back(PlkV4SOp{hidx, hi});
            }
        if (end_block < 0) return "v4s fold: no END";
        if ((size_t)end_block + 2 >= nblocks) return "v4s fold: fewer than two spare blocks after the END";
        if (!plk_v4s_stream_ops(&vs.words[(size_t)c * vs.stride], vs.stride, want)) return "v4s fold: the checked stream has no END";
        plk_v4s_unfold_ops(got, un);
        if (un.size() != want.size()) return plk_fmt("v4s fold: %ld ops unfolded, the checked stream has %ld", (long)un.size(), (long)want.size());
        for (size_t i = 0; i < un.size(); i++)
            if (un[i].h != want[i].h || un[i].hi != want[i].hi) return plk_fmt("v4s fold: unfolded op %ld is not the checked stream's", (long)i);
    }
    return "";
}

/*
 * The PAIR-PRODUCT op stream of k_ll_fused4_v4s<768, true, true> (tools/gen_fused4_v4.py, third emission mode): the checked stream for
 * programs within PLK_V4P_STACK_SLOTS stack slots.  The registers of slot 3 are a second look-up buffer; the row of
 * observation n lands in buffer n & 1, its handler consumes that buffer and requests observation min(n + 2, last) into it.
 * Adjacent (TIP_SET, TIP_MUL) and adjacent (TIP_SET + PUSH d, TIP_SET + POPMUL d) -- at most an ADVANCE between them in the
 * checked stream -- become one PAIR op: x = P[n] * P[n + 1] from the two buffers (the slot form computes slot = P[n],
 * x = P[n + 1] * slot and leaves the slot dead: the same product, IEEE multiplication of the two rows commutes), then the
 * requests of n + 2 and n + 3.  Codes are still extracted in increasing observation order, so the ADVANCEs are the checked
 * stream's in number and kind.  The extraction that needs a new dword is the one of an observation whose index is a multiple
 * of 4; two ahead, it falls into the handler of an even observation, before the first extraction of a PAIR of an even one or
 * between the two of a PAIR of an odd one, and handlers with an ADVANCE inside exist for exactly those cases -- except for
 * TIP_SET alone and TIP_MUL without wait (binary trees produce neither), whose ADVANCE keeps a dispatch in front of them.
 * TIP_SET + PUSH slot 0 has its handler on buffer 0 without ADVANCE only.  No property of the program builder is relied on
 * for that: in the trees tried it is the program's first observation and nothing else (tests/pairmulcheck_main.cpp), and a
 * stream that asks for it on buffer 1 is simply not derived -- plk_v4p_derive_ops returns false, the engine runs the folded
 * stream on such a tree and PLK_INFO_LL_PAIRMUL reports 0 (no error text: nothing failed); with an ADVANCE it keeps the
 * ADVANCE as a dispatch, like the two kinds above.
 * SCALE after MATVEC + POPMUL folds as in the folded stream.  The table has the 64 slots of the streamed one; handler indices
 * and the field dword of a PAIR: the generator's text.
 */
#define PLK_V4P_STACK_SLOTS 3
#define PLK_V4P_FOLD_ADV 36
#define PLK_V4P_PAIR_EVEN 52
#define PLK_V4P_PAIR_ODD 55

static inline int plk_v4p_obs_index(unsigned hidx)
{
    if (hidx == OP_TIP_SET) return 0;
    if (hidx == OP_TIP_MUL) return 1;
    if (hidx == PLK_WORD_TIPMUL_NOWAIT) return 2;
    if (hidx == PLK_WORD_MATVEC_TIPMUL) return 3;
    if (hidx >= PLK_WORD_SET_POPMUL && hidx < PLK_WORD_SET_POPMUL + PLK_V4P_STACK_SLOTS) return 4 + (int)(hidx - PLK_WORD_SET_POPMUL);
    if (hidx >= PLK_WORD_SET_PUSH && hidx < PLK_WORD_SET_PUSH + PLK_V4P_STACK_SLOTS) return 7 + (int)(hidx - PLK_WORD_SET_PUSH);
    return -1;
}
static inline unsigned plk_v4p_obs_handler(int j)
{
    static const unsigned first[4] = {OP_TIP_SET, OP_TIP_MUL, PLK_WORD_TIPMUL_NOWAIT, PLK_WORD_MATVEC_TIPMUL};
    return j < 4 ? first[j] : j < 7 ? PLK_WORD_SET_POPMUL + (unsigned)(j - 4) : PLK_WORD_SET_PUSH + (unsigned)(j - 7);
}
#define PLK_V4P_NONE 0xffffffffu
/* handler of observation kind j (plk_v4p_obs_index) on buffer p carrying v = 0 no ADVANCE, 1 + k ADVANCE_k; NONE: no such handler */
static inline unsigned plk_v4p_obs_slot(int j, int v, int p)
{
    static const unsigned odd[10] = {5, 11, 15, 19, 23, 27, 31, PLK_V4P_NONE, 59, 63};
    static const int folded[10] = {-1, 0, -1, 1, 2, 3, 4, -1, 5, 6};
    if (j < 0 || j >= 10 || v < 0 || v > 2 || p < 0 || p > 1) return PLK_V4P_NONE;
    if (v == 0) return p ? odd[j] : plk_v4p_obs_handler(j);
    return p == 0 && folded[j] >= 0 ? (unsigned)(PLK_V4P_FOLD_ADV + 2 * folded[j] + (v - 1)) : PLK_V4P_NONE;
}
/* PAIR handler of an observation of parity p; v = 0 no ADVANCE, 1 + k ADVANCE_k before the first extraction, 3 + k between the two */
static inline unsigned plk_v4p_pair_slot(int v, int p)
{
    if (v == 0) return p ? PLK_V4P_PAIR_ODD : PLK_V4P_PAIR_EVEN;
    if (p == 0 && (v == 1 || v == 2)) return (unsigned)(PLK_V4P_PAIR_EVEN + v);
    if (p == 1 && (v == 3 || v == 4)) return (unsigned)(PLK_V4P_PAIR_ODD + v - 2);
    return PLK_V4P_NONE;
}
struct PlkV4PHandler { int kind, j, v, p; };       /* kind: 0 no observation handler, 1 one observation, 2 PAIR */
static inline PlkV4PHandler plk_v4p_decode(unsigned h)
{
    for (int p = 0; p < 2; p++) {
        for (int v = 0; v < 5; v++) if (plk_v4p_pair_slot(v, p) == h) return PlkV4PHandler{2, -1, v, p};
        for (int j = 0; j < 10; j++) for (int v = 0; v < 3; v++) if (plk_v4p_obs_slot(j, v, p) == h) return PlkV4PHandler{1, j, v, p};
    }
    return PlkV4PHandler{0, -1, 0, 0};
}
static inline bool plk_v4p_is_obs(unsigned h) { return plk_v4p_decode(h).kind == 1; }
static inline bool plk_v4p_is_pair(unsigned h) { return plk_v4p_decode(h).kind == 2; }
static inline bool plk_v4s_is_advance(unsigned h) { return h == (unsigned)PLK_V4S_ADVANCE || h == (unsigned)PLK_V4S_ADVANCE + 1; }
/* the two ops of the checked stream a PAIR stands for */
static inline bool plk_v4p_pairable(unsigned a, unsigned b)
{
    if (a == OP_TIP_SET && b == OP_TIP_MUL) return true;
    return a >= PLK_WORD_SET_PUSH && a < PLK_WORD_SET_PUSH + PLK_V4P_STACK_SLOTS && b == a - PLK_WORD_SET_PUSH + PLK_WORD_SET_POPMUL;
}

struct PlkFusedV4P {
    std::vector<unsigned> words;       /* C streams of stride dwords, as PlkFusedV4S::words */
    size_t stride = 0;
    std::vector<unsigned> first_y1;    /* per category: LDS offset / 32 of the second observation's table (the prologue's) */
    unsigned first_b1 = 0;             /* bit offset of the second observation's code in chunk 0 */
    int npair = 0;                     /* PAIR ops of one category */
    int pair_adv[2] = {0, 0};          /* of them with an ADVANCE before the first / between the two extractions */
};

/* one category: in = the checked stream's ops (plk_v4s_stream_ops), first_y = its prologue table field; false: the
 * stream does not fit the form (a handler of slot 3, a table field beyond 13 bits, an observation count that is not nobs) */
static inline bool plk_v4p_derive_ops(const std::vector<PlkV4SOp> &in, unsigned first_y, int nobs, std::vector<PlkV4SOp> &out,
                                      unsigned &y1, unsigned &b1, int &npair, int pair_adv[2])
{
    out.clear(); npair = 0; pair_adv[0] = pair_adv[1] = 0;
    if (nobs < 1) return false;
    const int last = nobs - 1;
    std::vector<unsigned> T(nobs, 0u);
    std::vector<PlkV4SOp> items;
    T[0] = first_y;
    int k = 0;
    for (const PlkV4SOp &op : in) {
        if (plk_v4s_is_advance(op.h)) continue;
        items.push_back(op);
        if (!plk_word_is_obs(op.h)) continue;
        if (k >= nobs) return false;
        if (k < last) T[k + 1] = op.hi >> 16;
        k++;
    }
    if (k != nobs) return false;
    for (unsigned t : T) if (t >= (1u << 13)) return false;
    int cur = 0, nadv = 0, oi = 0;
    auto need_adv = [&](int m) { if (m / 4 <= cur) return 0; cur++; return 1 + (nadv++ & 1); };
    for (size_t i = 0; i < items.size(); i++) {
        const unsigned h = items[i].h;
        if (plk_word_is_obs(h)) {
            const int j = plk_v4p_obs_index(h), p = oi & 1;
            if (j < 0) return false;
            if (oi + 1 < nobs && i + 1 < items.size() && plk_v4p_pairable(h, items[i + 1].h)) {
                const int m1 = std::min(oi + 2, last), m2 = std::min(oi + 3, last);
                const int a1 = need_adv(m1), a2 = need_adv(m2), v = a1 ? a1 : a2 ? 2 + a2 : 0;
                if (plk_v4p_pair_slot(v, p) == PLK_V4P_NONE) return false;
                out.push_back(PlkV4SOp{plk_v4p_pair_slot(v, p), (unsigned)(m1 % 4) | (unsigned)(m2 % 4) << 3 | T[m1] << 5 | T[m2] << 18});
                npair++; if (a1) pair_adv[0]++; if (a2) pair_adv[1]++;
                oi += 2; i++;
            } else {
                const int m = std::min(oi + 2, last);
                int a = need_adv(m);
                /* no handler with this ADVANCE inside: it keeps its dispatch, in front of the op (the op's arithmetic does not read the dword) */
                if (a && plk_v4p_obs_slot(j, a, p) == PLK_V4P_NONE) { out.push_back(PlkV4SOp{(unsigned)(PLK_V4S_ADVANCE + a - 1), 0u}); a = 0; }
                if (plk_v4p_obs_slot(j, a, p) == PLK_V4P_NONE) return false;
                out.push_back(PlkV4SOp{plk_v4p_obs_slot(j, a, p), T[m] << 16 | (unsigned)(8 * (m % 4))});
                oi++;
            }
            continue;
        }
        const bool stack_op = (h >= 8 && h < 8 + PLK_V4P_STACK_SLOTS) || (h >= 16 && h < 16 + PLK_V4P_STACK_SLOTS) ||
                              (h >= 24 && h < 24 + PLK_V4P_STACK_SLOTS) || (h >= 28 && h < 28 + PLK_V4P_STACK_SLOTS);
        if (h != OP_MATVEC && h != OP_SCALE && !stack_op) return false;
        if (h == OP_SCALE && !out.empty() && out.back().h >= 28 && out.back().h < 28 + PLK_V4P_STACK_SLOTS) { out.back().h += PLK_V4S_FOLD_SCALE - 28; continue; }
        out.push_back(PlkV4SOp{h, 0u});
    }
    y1 = T[std::min(1, last)]; b1 = (unsigned)(8 * (std::min(1, last) % 4));
    return true;
}

/* vs: a stream plk_fused_check_v4s has accepted; vp.words stays empty where the form does not apply */
static inline void plk_fused_v4p_build(const PlkFusedV4S &vs, PlkFusedV4P &vp)
{
    vp = PlkFusedV4P();
    std::vector<PlkV4SOp> ops, out;
    std::vector<unsigned> words, y1s;
    size_t stride = 0;
    for (int c = 0; c < vs.C; c++) {
        unsigned y1 = 0, b1 = 0;
        int npair = 0, pair_adv[2];
        if (!plk_v4s_stream_ops(&vs.words[(size_t)c * vs.stride], vs.stride, ops)) return;
        if (!plk_v4p_derive_ops(ops, vs.first_y[c], vs.nobs, out, y1, b1, npair, pair_adv)) return;
        if (c == 0) {
            stride = plk_v4s_block_stride(out.size());
            words.assign((size_t)vs.C * stride, 0u);
            vp.first_b1 = b1; vp.npair = npair; vp.pair_adv[0] = pair_adv[0]; vp.pair_adv[1] = pair_adv[1];
        } else if (plk_v4s_block_stride(out.size()) != stride || b1 != vp.first_b1 || npair != vp.npair) { vp = PlkFusedV4P(); return; }
        plk_v4s_block_ops(out, &words[(size_t)c * stride], stride);
        y1s.push_back(y1);
    }
    vp.words.swap(words); vp.stride = stride; vp.first_y1.swap(y1s);
}

/* Replays the pair-product stream against the checked one.  Blocks, REFILLs, END and spare blocks as for the folded
 * stream; every handler is one the 3-slot table has.  Walking both streams in step, with the ADVANCE ops of the checked
 * one skipped: a non-observation op is the checked stream's op (a + SCALE variant: MATVEC + POPMUL d and the SCALE after
 * it); an observation handler stands for the checked stream's observation op of the same kind, a PAIR for two adjacent ones
 * that plk_v4p_pairable accepts -- so, unfolded, the ops are the checked stream's exactly.  The machine state is replayed
 * with them: a handler of parity p consumes buffer p, which must hold the row of exactly its observation (requested, not
 * overwritten since, and waited for: every handler but TIP_MUL-without-wait starts with a wait for all outstanding
 * look-ups, that one needs a waiting handler since the request); every extraction names the byte and the table the checked
 * stream names for that observation and reads the chunk that is current; folded ADVANCEs alternate in kind from 0, are as
 * many as the checked stream's and request no chunk past the unit's. */
static inline std::string plk_fused_check_v4p(const PlkFusedV4S &vs, const PlkFusedV4P &vp)
{
    if (vp.stride % 16 != 0 || vp.stride < 48 || vp.words.size() != (size_t)vs.C * vp.stride || (int)vp.first_y1.size() != vs.C) return "v4p stream: word count";
    const int nobs = vs.nobs, last = nobs - 1;
    if (nobs < 1 || vs.chunks != plk_stream_chunks(nobs)) return "v4p stream: observation count";
    std::vector<PlkV4SOp> want, got;
    std::vector<unsigned> T(nobs);
    for (int c = 0; c < vs.C; c++) {
        const unsigned *wd = &vp.words[(size_t)c * vp.stride];
        const size_t nblocks = vp.stride / 16;
        long end_block = -1;
        got.clear();
        for (size_t b = 0; b < nblocks; b++)
            for (int j = 0; j < 8; j++) {
                const unsigned lo = wd[(b * 8 + j) * 2], hi = wd[(b * 8 + j) * 2 + 1];
                if (lo % PLK_V4_HANDLER_BYTES != 0 || lo >= (unsigned)PLK_V4_HANDLER_SLOTS * PLK_V4_HANDLER_BYTES) return plk_fmt("v4p stream: handler offset in block %ld", (long)b);
                const unsigned hidx = lo / PLK_V4_HANDLER_BYTES;
                if (j == 7) {
                    if (hidx != (unsigned)((b & 1) ? PLK_V4_REFILL_B : PLK_V4_REFILL_A) || hi != 0) return plk_fmt("v4p stream: block %ld does not end in its REFILL op", (long)b);
                    continue;
                }
                if (hidx == (unsigned)PLK_V4_REFILL_A || hidx == (unsigned)PLK_V4_REFILL_B) return plk_fmt("v4p stream: REFILL op inside block %ld", (long)b);
                if (end_block >= 0) { if (hidx != OP_END || hi != 0) return "v4p stream: ops after END"; continue; }
                if (hidx == OP_END) { if (hi != 0) return "v4p stream: stray fields in END"; end_block = (long)b; continue; }
                got.push_back(PlkV4SOp{hidx, hi});
            }
        if (end_block < 0) return "v4p stream: no END";
        if ((size_t)end_block + 2 >= nblocks) return "v4p stream: fewer than two spare blocks after the END";
        if (!plk_v4s_stream_ops(&vs.words[(size_t)c * vs.stride], vs.stride, want)) return "v4p stream: the checked stream has no END";
        /* byte and table of every observation, as the checked stream names them */
        int k = 0, nadv_want = 0;
        T[0] = vs.first_y[c];
        for (const PlkV4SOp &op : want) {
            if (plk_v4s_is_advance(op.h)) { nadv_want++; continue; }
            if (!plk_word_is_obs(op.h)) continue;
            if (k >= nobs) return "v4p stream: the checked stream has more observation ops than observations";
            const int next = std::min(k + 1, last);
            if ((op.hi & 0xffffu) != (unsigned)(8 * (next % 4)) || (k == last && (op.hi >> 16) != T[last])) return "v4p stream: fields of the checked stream";
            T[next] = op.hi >> 16;
            k++;
        }
        if (k != nobs) return "v4p stream: the checked stream's observation count";
        if (vp.first_y1[c] != T[std::min(1, last)] || vp.first_b1 != (unsigned)(8 * (std::min(1, last) % 4))) return "v4p stream: prologue fields of the second observation";
        /* prologue: chunk 0 current, chunks 1 .. AHEAD in flight; observations 0 and 1 requested and waited for */
        long buf[2] = {0, std::min(1, last)};
        bool landed[2] = {true, true};
        int cur = 0, requested = PLK_V4S_AHEAD, nadv = 0, oi = 0;
        if (requested >= vs.chunks) return "v4p stream: the prologue reads past the unit";
        size_t wi = 0;
        std::string bad;
        auto skip_adv = [&]() { while (wi < want.size() && plk_v4s_is_advance(want[wi].h)) wi++; };
        auto advance = [&](int kind) {
            if (kind != (nadv & 1)) { bad = plk_fmt("v4p stream: ADVANCE %ld of the wrong kind", nadv); return; }
            cur = requested - (PLK_V4S_AHEAD - 1);
            requested++;
            if (requested >= vs.chunks) bad = plk_fmt("v4p stream: ADVANCE %ld reads past the unit's chunks", nadv);
            nadv++;
        };
        auto extract = [&](int m, unsigned byte, unsigned table) {
            if (!bad.empty()) return;
            if (byte != (unsigned)(m % 4)) bad = plk_fmt("v4p stream: the request of observation %ld extracts the wrong byte", m);
            else if (cur != m / 4) bad = plk_fmt("v4p stream: the request of observation %ld extracts from chunk %ld, its code is in chunk %ld", m, cur, m / 4);
            else if (table != T[m]) bad = plk_fmt("v4p stream: table field of the request of observation %ld", m);
        };
        for (size_t g = 0; g < got.size(); g++) {
            const unsigned h = got[g].h, hi = got[g].hi;
            const PlkV4PHandler hd = plk_v4p_decode(h);
            if (plk_v4s_is_advance(h)) {
                /* an ADVANCE with a dispatch of its own */
                if (hi != 0) return plk_fmt("v4p stream: stray fields in op %ld", (long)g);
                advance((int)(h - PLK_V4S_ADVANCE));
                if (!bad.empty()) return bad;
                continue;
            }
            skip_adv();
            if (wi >= want.size()) return "v4p stream: more ops than the checked stream";
            if (hd.kind == 1) {
                const int j = hd.j, v = hd.v, p = hd.p;
                if (want[wi].h != plk_v4p_obs_handler(j)) return plk_fmt("v4p stream: op %ld is not the checked stream's", (long)g);
                wi++;
                if (oi >= nobs || p != (oi & 1)) return plk_fmt("v4p stream: observation %ld handled on the other buffer", oi);
                if (j != 2) landed[0] = landed[1] = true;
                if (buf[p] != oi || !landed[p]) return plk_fmt("v4p stream: buffer %ld does not hold observation %ld", p, oi);
                if (v) advance(v - 1);
                const int m = std::min(oi + 2, last);
                if ((hi & 0xffe7u) != 0) return plk_fmt("v4p stream: stray bits in the fields of observation %ld", oi);
                extract(m, (hi & 0x18u) >> 3, hi >> 16);
                if (!bad.empty()) return bad;
                buf[p] = m; landed[p] = false; oi++;
            } else if (hd.kind == 2) {
                const int v = hd.v, p = hd.p;
                const unsigned a = want[wi].h;
                wi++;
                skip_adv();
                if (wi >= want.size() || !plk_v4p_pairable(a, want[wi].h)) return plk_fmt("v4p stream: PAIR op %ld where the checked stream has no pair of look-ups", (long)g);
                wi++;
                if (oi + 1 >= nobs || p != (oi & 1)) return plk_fmt("v4p stream: PAIR of observation %ld on the other buffers", oi);
                landed[0] = landed[1] = true;
                if (buf[p] != oi || buf[1 - p] != oi + 1) return plk_fmt("v4p stream: the buffers do not hold observations %ld and %ld", oi, oi + 1);
                if ((hi & 0x80000004u) != 0) return plk_fmt("v4p stream: stray bits in the fields of the PAIR of observation %ld", oi);
                const int m1 = std::min(oi + 2, last), m2 = std::min(oi + 3, last);
                if (v == 1 || v == 2) advance(v - 1);
                extract(m1, hi & 3u, (hi >> 5) & 0x1fffu);
                if (v >= 3) advance(v - 3);
                extract(m2, (hi >> 3) & 3u, (hi >> 18) & 0x1fffu);
                if (!bad.empty()) return bad;
                buf[p] = m1; buf[1 - p] = m2; landed[0] = landed[1] = false; oi += 2;
            } else {
                if (hi != 0) return plk_fmt("v4p stream: stray fields in op %ld", (long)g);
                if (h >= PLK_V4S_FOLD_SCALE && h < PLK_V4S_FOLD_SCALE + PLK_V4P_STACK_SLOTS) {
                    if (want[wi].h != h - PLK_V4S_FOLD_SCALE + 28 || wi + 1 >= want.size() || want[wi + 1].h != OP_SCALE) return plk_fmt("v4p stream: + SCALE variant at op %ld where no SCALE follows", (long)g);
                    wi += 2;
                    landed[0] = landed[1] = true;
                    continue;
                }
                const bool matvec = h == OP_MATVEC || (h >= 24 && h < 24 + PLK_V4P_STACK_SLOTS) || (h >= 28 && h < 28 + PLK_V4P_STACK_SLOTS);
                const bool plain = h == OP_SCALE || (h >= 8 && h < 8 + PLK_V4P_STACK_SLOTS) || (h >= 16 && h < 16 + PLK_V4P_STACK_SLOTS);
                if (!matvec && !plain) return plk_fmt("v4p stream: op %ld names a handler the 3-slot table does not have", (long)g);
                if (want[wi].h != h || want[wi].hi != 0) return plk_fmt("v4p stream: op %ld is not the checked stream's", (long)g);
                wi++;
                if (matvec) landed[0] = landed[1] = true;
            }
        }
        skip_adv();
        if (wi != want.size() || oi != nobs) return "v4p stream: END before the checked stream's last op";
        if (nadv != nadv_want) return "v4p stream: another number of ADVANCEs than the checked stream's";
    }
    return "";
}

/*
 * THREE-LEAF TABLES of the streamed form (plk_fused_v4t_build).  A node d that is not the root and whose children are a
 * cherry a = (b, c) and a leaf l reads, in the checked pair-table program, TIP_SET (pair table of a), TIP_MUL (table of l),
 * MATVEC (edge above d): one of nchar^3 vectors per category.  With that vector in a table of its own (nchar^2 units,
 * code (code_b * nchar + code_c) * nchar + code_l, which must stay a byte: nchar^3 <= 256) the three ops become one TIP_SET;
 * the pair table of a, the table of l, their two staged rows and the matrix of the edge leave the formats.  What followed
 * the MATVEC stays where it was -- PUSH, POPMUL, TIP_MUL, SCALE are ops of their own in PlkFusedPT::vops, and the word
 * builder fuses TIP_SET + PUSH / POPMUL as it does for any look-up -- so no SCALE moves, appears or disappears.  A SCALE
 * between the look-ups and the MATVEC (d rescaled) keeps the node as it is, and so does a third child or data at d: the
 * MATVEC must follow the two look-ups directly.  The program builder visits an internal child before the leaves, so the
 * cherry is always the TIP_SET; the product of the two rows commutes bit for bit, so the order of the children in the tree
 * makes no difference to the row.
 * The rows are NOT built in double-double: a row is the handlers' own fp64 sequence on the handlers' own operands
 * (plk_v4t_row: the rounded pair-table row, the rounded tip row, the matrix the stream would have delivered), so the
 * looked-up vector is bit for bit what the interpreter computes from the three ops.
 * The fold and pair-product derivations run on the rewritten formats as on any other.
 */
/* M in the matrix stream's layout (M[4 j + i] = P[i][j]); the MATVEC handler's sequence (tools/gen_fused4_v4.py, matvec):
 * x = a o b, then per row one multiply and three fused multiply-adds in column order */
PLK_HD static inline void plk_v4t_row(const double *M, const double *a, const double *b, double *out)
{
    double x[4];
    for (int j = 0; j < 4; j++) x[j] = a[j] * b[j];
    for (int i = 0; i < 4; i++) {
        double acc = M[i] * x[0];
        for (int j = 1; j < 4; j++) acc = fma(M[4 * j + i], x[j], acc);
        out[i] = acc;
    }
}

/* LDS bytes a three-leaf table adds to one category's image: nchar^2 units for the nchar + 1 of its cherry and its leaf */
static inline size_t plk_v4t_extra_bytes(int nchar) { return (size_t)(nchar * nchar - nchar - 1) * nchar * 32; }

/* the nodes that qualify, in program order: index into in.vops of the TIP_SET of (pair look-up, leaf look-up, MATVEC) */
static inline void plk_v4t_candidates(const PlkFusedPT &in, int nchar, std::vector<int> &at)
{
    at.clear();
    if (nchar < 2 || nchar * nchar * nchar > 256 || in.ntriples != 0) return;
    std::vector<int> table_at(std::max(in.units, 1), -1);
    for (size_t t = 0; t < in.tab_unit.size(); t++) if (in.tab_unit[t] >= 0 && in.tab_unit[t] < in.units) table_at[in.tab_unit[t]] = (int)t;
    const std::vector<PlkFusedPT::VOp> &v = in.vops;
    for (size_t i = 0; i + 2 < v.size(); i++) {
        if (v[i].code != OP_TIP_SET || v[i + 1].code != OP_TIP_MUL || v[i + 2].code != OP_MATVEC) continue;
        const int tp = table_at[v[i].unit], tl = table_at[v[i + 1].unit];
        if (tp < 0 || tl < 0 || in.tab_eb[tp] < 0 || in.tab_eb[tl] >= 0 || in.tab_edge[tl] < 0) continue;
        at.push_back((int)i);
        i += 2;
    }
}

/* in: a pair-table program plk_fused_check_pt has accepted; extra_bytes: LDS one category's image may grow by.  Takes the
 * qualifying nodes in program order as long as they fit; out.ntriples == 0: out is a copy of in. */
static inline void plk_fused_v4t_build(const PlkFusedPT &in, int slots_needed, int nchar, size_t extra_bytes, bool fuse_set, PlkFusedPT &out)
{
    std::vector<int> at;
    plk_v4t_candidates(in, nchar, at);
    const size_t per = plk_v4t_extra_bytes(nchar);
    size_t take = per ? std::min(at.size(), extra_bytes / per) : 0;
    /* the unit field of the op words has 11 bits */
    while (take > 0 && (size_t)in.units + take * (size_t)(nchar * nchar - nchar - 1) >= 2048) take--;
    if (take == 0) { out = in; return; }
    at.resize(take);
    typedef PlkFusedPT::VOp VOp;
    PlkFusedPT o;
    const int ntab = (int)in.tab_unit.size(), nrows = (int)in.row_node.size();
    std::vector<int> table_at(std::max(in.units, 1), -1), new_unit(ntab, -1), new_row(nrows, -1);
    for (int t = 0; t < ntab; t++) table_at[in.tab_unit[t]] = t;
    auto table = [&](int edge, int eb, int ec, int ea, int el, int nunits) {
        o.tab_unit.push_back(o.units); o.tab_edge.push_back(edge); o.tab_eb.push_back(eb); o.tab_ec.push_back(ec);
        o.tab_ea.push_back(ea); o.tab_el.push_back(el);
        const int u = o.units; o.units += nunits; return u;
    };
    auto row = [&](int n1, int n2, int n3) {
        o.row_node.push_back(n1); o.row_node2.push_back(n2); o.row_node3.push_back(n3);
        return (int)o.row_node.size() - 1;
    };
    bool pseudo = false;
    size_t next = 0;
    const std::vector<VOp> &v = in.vops;
    for (size_t i = 0; i < v.size(); i++) {
        if (next < at.size() && (size_t)at[next] == i) {
            const int tp = table_at[v[i].unit], tl = table_at[v[i + 1].unit], rp = v[i].row, rl = v[i + 1].row;
            const int u = table(v[i + 2].edge, in.tab_eb[tp], in.tab_ec[tp], in.tab_edge[tp], in.tab_edge[tl], nchar * nchar);
            o.vops.push_back(VOp{OP_TIP_SET, u, row(in.row_node[rp], in.row_node2[rp], in.row_node[rl]), 0, -1});
            o.ntriples++;
            next++; i += 2;
            continue;
        }
        VOp w = v[i];
        if (w.code == OP_TIP_SET || w.code == OP_TIP_MUL) {
            const int t = table_at[w.unit];
            if (new_unit[t] < 0) {
                new_unit[t] = table(in.tab_edge[t], in.tab_eb[t], in.tab_ec[t], -1, -1, in.tab_eb[t] >= 0 ? nchar : 1);
                if (in.tab_eb[t] >= 0) o.npairs++;
                if (in.tab_edge[t] < 0) pseudo = true;
            }
            if (new_row[w.row] < 0) new_row[w.row] = row(in.row_node[w.row], in.row_node2[w.row], -1);
            w.unit = new_unit[t]; w.row = new_row[w.row];
        } else if (w.code == OP_MATVEC) o.mat_edge.push_back(w.edge);
        o.vops.push_back(w);
    }
    if (!pseudo) table(-1, -1, -1, -1, -1, 1);
    plk_fused_pt_words(slots_needed, fuse_set, o);
    out = std::move(o);
}

/*
 * Replays the rewritten formats against the checked pair-table program they were derived from (in: accepted by
 * plk_fused_check_pt).  The 32-bit words are decoded with their look-up chain into the ops they execute, which must be
 * out.vops; those, with every three-leaf look-up unfolded into (pair look-up, leaf look-up, MATVEC), must be in.vops
 * exactly: same opcodes, stack slots and SCALE positions, tables of the same edges read through rows of the same nodes, the
 * matrix stream consumed exactly (the absorbed matrices are the ones missing).  A three-leaf table stands for a node of
 * the tree that is not the root, whose children are exactly the cherry and the leaf, under the edge it names; the tables
 * tile the unit range without gaps, so the largest code of every row kind addresses inside its table; unit and row fields
 * fit the op words.  (The LDS offsets of the streamed words are plk_fused_check_v4s's business, which knows the table
 * sizes; the rows themselves are checked against the fp64 replay by tests/triplecheck_main.cpp with plk_v4t_row, the
 * function the device builder calls.)
 */
static inline std::string plk_fused_check_v4t(int N, const int *ip, const int *ix, const PlkFusedPT &in, const PlkFusedPT &out, int nchar)
{
    typedef PlkFusedPT::VOp VOp;
    const int ntab = (int)out.tab_unit.size(), nrows = (int)out.row_node.size(), E = N - 1;
    if (nchar < 2 || nchar * nchar * nchar > 256) return "v4t program: the combined code must stay a byte";
    if ((int)out.tab_edge.size() != ntab || (int)out.tab_eb.size() != ntab || (int)out.tab_ec.size() != ntab || (int)out.tab_ea.size() != ntab ||
        (int)out.tab_el.size() != ntab || (int)out.row_node2.size() != nrows || (int)out.row_node3.size() != nrows) return "v4t program: table sizes";
    if (nrows < 1 || out.units < 1 || out.units >= 2048 || nrows >= 65536) return "v4t program: field widths";
    std::vector<int> table_at(out.units, -1), in_table_at(std::max(in.units, 1), -1);
    int expect = 0, ntri = 0;
    for (int t = 0; t < ntab; t++) {
        const int nu = (int)(plk_pt_table_codes(out, (size_t)t, nchar) / (size_t)nchar);
        if (out.tab_unit[t] != expect || expect + nu > out.units) return "v4t program: table layout";
        table_at[expect] = t;
        expect += nu;
        if (out.tab_el[t] >= 0) ntri++;
    }
    if (expect != out.units || ntri != out.ntriples) return "v4t program: table layout";
    for (size_t t = 0; t < in.tab_unit.size(); t++) if (in.tab_unit[t] >= 0 && in.tab_unit[t] < in.units) in_table_at[in.tab_unit[t]] = (int)t;
    /* the words, decoded: the chain delivers (cur_unit, cur_row) to every observation handler */
    std::vector<VOp> dec;
    {
        if (out.words.size() % 8 != 0 || out.words.size() < 16) return "v4t program: word buffer";
        auto unit_ok = [&](long u) { return u >= 0 && u < out.units && table_at[u] >= 0; };
        auto row_ok = [&](long r) { return r >= 0 && r < nrows; };
        long cur_unit = out.first_unit, cur_row = out.first_row, next_row = out.second_row;
        if (!unit_ok(cur_unit) || !row_ok(cur_row) || !row_ok(next_row)) return "v4t program: prologue fields";
        bool waited = true, ended = false;
        for (size_t wi = 0; wi < out.words.size() && !ended; wi++) {
            const unsigned w = out.words[wi], hidx = w & 31, y = (w >> 5) & 0x7ff, z = w >> 16;
            auto observe = [&](int code) -> bool {
                dec.push_back(VOp{code, (int)cur_unit, (int)cur_row, 0, -1});
                if (!unit_ok(y) || !row_ok(z)) return false;
                /* a row's largest code must fit the table it indexes: rows and tables of one kind */
                const int t = table_at[y];
                const int kind_t = out.tab_el[t] >= 0 ? 3 : out.tab_eb[t] >= 0 ? 2 : 1;
                const int kind_r = out.row_node3[next_row] >= 0 ? 3 : out.row_node2[next_row] >= 0 ? 2 : 1;
                if (kind_r > kind_t) return false;
                cur_unit = y; cur_row = next_row; next_row = z;
                waited = false;
                return true;
            };
            bool ok = true;
            if (hidx == OP_END) ended = true;
            else if (hidx == OP_MATVEC) { dec.push_back(VOp{OP_MATVEC, 0, 0, 0, -1}); waited = true; }
            else if (hidx == PLK_WORD_MATVEC_TIPMUL) { dec.push_back(VOp{OP_MATVEC, 0, 0, 0, -1}); waited = true; ok = observe(OP_TIP_MUL); }
            else if (hidx == OP_TIP_SET) ok = observe(OP_TIP_SET);
            else if (hidx == OP_TIP_MUL) ok = observe(OP_TIP_MUL);
            else if (hidx == PLK_WORD_TIPMUL_NOWAIT) { if (!waited) return plk_fmt("v4t program: word %ld skips a wait it needs", (long)wi); ok = observe(OP_TIP_MUL); }
            else if (hidx == OP_SCALE) dec.push_back(VOp{OP_SCALE, 0, 0, 0, -1});
            else if (hidx >= PLK_WORD_SET_POPMUL && hidx < PLK_WORD_SET_POPMUL + 4) { ok = observe(OP_TIP_SET); dec.push_back(VOp{OP_POPMUL, 0, 0, (int)(hidx & 3), -1}); }
            else if (hidx >= PLK_WORD_SET_PUSH && hidx < PLK_WORD_SET_PUSH + 4) { ok = observe(OP_TIP_SET); dec.push_back(VOp{OP_PUSH, 0, 0, (int)(hidx & 3), -1}); }
            else if (hidx >= 24) { dec.push_back(VOp{OP_MATVEC, 0, 0, 0, -1}); waited = true; dec.push_back(VOp{hidx < 28 ? OP_PUSH : OP_POPMUL, 0, 0, (int)(hidx & 3), -1}); }
            else if (hidx >= 8 && hidx < 12) dec.push_back(VOp{OP_PUSH, 0, 0, (int)(hidx & 7), -1});
            else if (hidx >= 16 && hidx < 20) dec.push_back(VOp{OP_POPMUL, 0, 0, (int)(hidx & 7), -1});
            else return plk_fmt("v4t program: word %ld jumps to an empty handler slot", (long)wi);
            if (!ok) return plk_fmt("v4t program: word %ld requests a table or a row out of range", (long)wi);
        }
        if (!ended) return "v4t program: no END";
    }
    if (dec.size() != out.vops.size()) return plk_fmt("v4t program: the words execute %ld ops, the rewritten program has %ld", (long)dec.size(), (long)out.vops.size());
    for (size_t i = 0; i < dec.size(); i++) {
        const VOp &a = dec[i], &b = out.vops[i];
        const bool obs = b.code == OP_TIP_SET || b.code == OP_TIP_MUL;
        if (a.code != b.code || (obs && (a.unit != b.unit || a.row != b.row)) || ((b.code == OP_PUSH || b.code == OP_POPMUL) && a.d != b.d))
            return plk_fmt("v4t program: decoded op %ld is not the rewritten program's", (long)i);
    }
    /* the rewritten ops, unfolded, against the checked ones */
    size_t j = 0, mi = 0;
    int absorbed = 0;
    std::vector<char> used(ntab, 0);
    auto same_single = [&](const VOp &a, const VOp &b) {       /* a of out, b of in: one look-up of the same table through the same row */
        if (b.unit < 0 || b.unit >= in.units || in_table_at[b.unit] < 0 || b.row < 0 || b.row >= (int)in.row_node.size()) return false;
        const int t = table_at[a.unit], ti = in_table_at[b.unit];
        return out.tab_el[t] < 0 && out.tab_edge[t] == in.tab_edge[ti] && out.tab_eb[t] == in.tab_eb[ti] && out.tab_ec[t] == in.tab_ec[ti] &&
               out.row_node[a.row] == in.row_node[b.row] && out.row_node2[a.row] == in.row_node2[b.row] && out.row_node3[a.row] == -1;
    };
    for (size_t i = 0; i < out.vops.size(); i++) {
        const VOp &a = out.vops[i];
        if (j >= in.vops.size()) return "v4t program: more ops than the checked program";
        const VOp &b = in.vops[j];
        if (a.code == OP_TIP_SET || a.code == OP_TIP_MUL) {
            const int t = table_at[a.unit];
            if (used[t]++ && out.tab_edge[t] >= 0) return plk_fmt("v4t program: table %ld used twice", (long)t);
            if (out.tab_el[t] < 0) {
                if (a.code != b.code || !same_single(a, b)) return plk_fmt("v4t program: look-up %ld is not the checked program's", (long)i);
                j++;
                continue;
            }
            /* a three-leaf look-up: the checked program continues with the cherry's look-up, the leaf's and the MATVEC */
            if (a.code != OP_TIP_SET || j + 2 >= in.vops.size()) return plk_fmt("v4t program: three-leaf look-up %ld", (long)i);
            const VOp &bp = in.vops[j], &bl = in.vops[j + 1], &bm = in.vops[j + 2];
            if (bp.code != OP_TIP_SET || bl.code != OP_TIP_MUL || bm.code != OP_MATVEC) return plk_fmt("v4t program: three-leaf look-up %ld does not stand for look-up, look-up, MATVEC", (long)i);
            const int tp = in_table_at[bp.unit], tl = in_table_at[bl.unit];
            if (tp < 0 || tl < 0 || in.tab_eb[tp] < 0 || in.tab_eb[tl] >= 0 || in.tab_edge[tl] < 0) return plk_fmt("v4t program: three-leaf look-up %ld: not a cherry and a leaf", (long)i);
            if (out.tab_eb[t] != in.tab_eb[tp] || out.tab_ec[t] != in.tab_ec[tp] || out.tab_ea[t] != in.tab_edge[tp] || out.tab_el[t] != in.tab_edge[tl] ||
                out.tab_edge[t] != bm.edge) return plk_fmt("v4t program: three-leaf table %ld holds other edges than the ops it stands for", (long)t);
            if (out.row_node[a.row] != in.row_node[bp.row] || out.row_node2[a.row] != in.row_node2[bp.row] || out.row_node3[a.row] != in.row_node[bl.row] ||
                in.row_node2[bl.row] != -1) return plk_fmt("v4t program: row of three-leaf look-up %ld", (long)i);
            /* the tree: d under the absorbed edge, not the root (it has an edge above it), children exactly a and l */
            const int e = out.tab_edge[t], ea = out.tab_ea[t], el = out.tab_el[t];
            if (e < 0 || e >= E || ea < 0 || ea >= E || el < 0 || el >= E) return plk_fmt("v4t program: edges of three-leaf table %ld", (long)t);
            const int d = ix[e];
            if (ip[d + 1] - ip[d] != 2 || plk_edge_parent(N, ip, ea) != d || plk_edge_parent(N, ip, el) != d || ea == el ||
                plk_edge_parent(N, ip, out.tab_eb[t]) != ix[ea] || ip[ix[el] + 1] != ip[ix[el]] || out.row_node3[a.row] != ix[el])
                return plk_fmt("v4t program: three-leaf table %ld is not a cherry and a leaf under one node", (long)t);
            absorbed++;
            j += 3;
            continue;
        }
        if (a.code != b.code) return plk_fmt("v4t program: op %ld is not the checked program's", (long)i);
        if (a.code == OP_MATVEC) {
            if (mi >= out.mat_edge.size() || out.mat_edge[mi] != b.edge || a.edge != b.edge) return plk_fmt("v4t program: matrix %ld is not the op's edge", (long)mi);
            mi++;
        } else if ((a.code == OP_PUSH || a.code == OP_POPMUL) && a.d != b.d) return plk_fmt("v4t program: stack op %ld", (long)i);
        j++;
    }
    if (j != in.vops.size()) return "v4t program: the checked program's ops are not all covered";
    if (mi != out.mat_edge.size() || out.mat_edge.size() + (size_t)absorbed != in.mat_edge.size()) return "v4t program: matrix stream not consumed exactly";
    if (absorbed != out.ntriples) return "v4t program: three-leaf tables that no op reads";
    return "";
}

/*
 * Which three-leaf form the streamed kernel takes: the categories in G groups of Cg = ceil(C / G) (the tables of one group
 * resident at a time: G phases in one launch) and `nodes` three-leaf tables in the room that leaves.  Candidates G = 1, 2, C.
 * Per unit and category an absorbed node saves PLK_V4T_NODE_INSTS vector instructions (the 32 of the product, the 8 of the
 * elementwise product, 4 of the look-up's address); a further phase costs, per unit, the prologue of a category once more
 * and the round trip of the partial mixture sum (PLK_V4T_PHASE_UNIT_INSTS), and once the restaging of the tables and the
 * skew of two barriers (PLK_V4T_PHASE_INSTS, in instructions of one wave).  The best candidate with a gain is taken when
 * the option forces the form; the default also asks every wave to walk at least PLK_V4T_MIN_PASSES units per phase: the
 * smallest count at which the form was measured to win (3 at config 2, with four-leaf tables: kernel - 26 %, whole step - 7 %,
 * the tables' build included; DESIGN.md section 4, profiles/ll_k4_nextreq_ab.json.  With three-leaf tables alone it was even there).
 * The phase charge was first fitted at one site count, with the waves meeting before every category: 6000 + 180 a unit.  Since
 * the phases of one category run without that barrier (plk_v4s_auto_sync) it is fitted to forced runs at two counts, an
 * instruction per unit priced at the 5 to 8 ns the kernel's time per executed instruction gives: at 26 units per wave G = 4 with
 * 16 three-leaf tables runs 0.045 ms longer than G = 2 with 15 where its instructions say 0.023 to 0.036 ms shorter, so a phase
 * costs 5200 to 6700 there; at 4 units per wave (1.25M sites) G = 4 with the mix runs 0.067 ms shorter than G = 2 with 15
 * where the instructions alone say 0.054 to 0.082: a phase costs between nothing and 1000.  So the cost is per unit -- the
 * prologue, the partial sums' round trip -- and the fixed part is small: 200 + 250 a unit.
 */
#define PLK_V4T_NODE_INSTS 44
#define PLK_V4T_PHASE_UNIT_INSTS 250
#define PLK_V4T_PHASE_INSTS 200
#define PLK_V4T_MIN_PASSES 3
/* quads > 0: the four-leaf form (plk_fused_v4q_build) with the nodes listed, as indices into the checked program's vops:
 * quad_at / quad_shape the four-leaf nodes, tri_at the `nodes` three-leaf nodes that are not below one of them */
struct PlkV4TPlan {
    int groups = 1, Cg = 0, nodes = 0; size_t extra_bytes = 0;
    int quads = 0;
    std::vector<int> tri_at, quad_at, quad_shape;
};

static inline PlkV4TPlan plk_v4q_plan(const PlkFusedPT &fpt, int nchar, int C, long S, int num_cus, size_t static_lds, int quad, int groups_opt,
                                      const int *node_codes);

/* triple: 0 forbidden, 1 default, 2 forced;  groups_opt: 0 the model's choice, 1 one group, 2 two groups, -1 a group per category;
 * quad: 0 three-leaf tables only, 1 / 2 four-leaf tables too where node_codes (the occurring codes per node) allow them, by
 * default / forced (plk_v4q_plan; forced implies triple = 2) */
static inline PlkV4TPlan plk_v4t_plan(const PlkFusedPT &fpt, int nchar, int C, long S, int num_cus, size_t static_lds, int triple, int groups_opt,
                                      int quad = 0, const int *node_codes = nullptr)
{
    if (quad > 0 && triple > 0 && node_codes) {
        const PlkV4TPlan q = plk_v4q_plan(fpt, nchar, C, S, num_cus, static_lds, quad, groups_opt, node_codes);
        if (q.quads > 0) return q;
        if (quad == 2) triple = 2;
    }
    PlkV4TPlan best;
    best.Cg = C;
    std::vector<int> at;
    plk_v4t_candidates(fpt, nchar, at);
    if (triple == 0 || at.empty() || C < 1 || S < 1) return best;
    const long nunits = (S + PLK_V4S_UNIT - 1) / PLK_V4S_UNIT;
    const long waves = std::min<long>((nunits + 11) / 12, std::max(num_cus, 1)) * 12;
    const long passes = (nunits + waves - 1) / waves;
    const size_t per = plk_v4t_extra_bytes(nchar), image = (size_t)fpt.units * nchar * 32, limit = plk_pt_lds_limit(1024);
    double best_gain = triple == 2 ? -1e300 : 0.0;     /* forced: the best candidate whatever the model says of it */
    const int cand[3] = {1, 2, C};
    for (int q = 0; q < 3; q++) {
        const int G = cand[q];
        if (G < 1 || G > C || (q > 0 && G == cand[q - 1]) || (q == 2 && G == 1)) continue;
        if (groups_opt > 0 && G != std::min(groups_opt, C)) continue;
        if (groups_opt == -1 && G != C) continue;
        const int Cg = (C + G - 1) / G, groups = (C + Cg - 1) / Cg;
        if (static_lds + (size_t)Cg * image > limit) continue;
        const size_t room = (limit - static_lds) / (size_t)Cg - image;
        size_t t = std::min(at.size(), room / per);
        while (t > 0 && (size_t)fpt.units + t * (size_t)(nchar * nchar - nchar - 1) >= 2048) t--;
        if (t == 0) continue;
        if (triple == 1 && passes < PLK_V4T_MIN_PASSES) continue;
        const double gain = (double)C * (double)t * PLK_V4T_NODE_INSTS * (double)passes -
                            (double)(groups - 1) * (PLK_V4T_PHASE_INSTS + (double)PLK_V4T_PHASE_UNIT_INSTS * (double)passes);
        if (gain > best_gain) {
            best_gain = gain; best.groups = groups; best.Cg = Cg; best.nodes = (int)t; best.extra_bytes = t * per;
        }
    }
    return best;
}

/*
 * FOUR-LEAF TABLES of the streamed form (plk_fused_v4q_build).  Table rows are indexed in radix nchar, the number of
 * DECLARED character definitions, which stops the three-leaf form at nchar^3 <= 256.  Which codes a leaf really takes is a
 * property of the patterns (node_codes[n]: bit `code` set when some site < S carries it at node n; k_node_flags, once per
 * upload).  Where each of the four leaves below a node d takes at most four codes, the codes are re-coded per leaf into
 * ranks 0 .. 3 and (d, the edge above it) becomes one look-up of a 256-row table.  The shapes, in the checked pair-table
 * program's ops as plk_program_build emits them (first internal child, leaves, PUSH / further internal child / POPMUL; the
 * MATVEC of an edge is emitted by the node above it):
 *   A  d = (t, l2), t = (a, l1), a a cherry:  TIP_SET(pair a) TIP_MUL(l1) MATVEC(e_t) TIP_MUL(l2) MATVEC(e_d)
 *      absorbs two products; the three-leaf candidate t inside it is not a table of its own
 *   B  d = (a, a'), both cherries:            TIP_SET(pair a) PUSH(s) TIP_SET(pair a') POPMUL(s) MATVEC(e_d)
 *      absorbs one product and the stack round trip
 * directly adjacent: a SCALE in the run, a third child or data at d or t put another op in between and the node stays as it
 * is.  What follows the last MATVEC stays an op of its own, as for three-leaf tables, so no SCALE moves.  The final MATVEC
 * makes d a non-root node: only a parent emits it.
 * Rows: the handlers' fp64 sequence on the handlers' operands (plk_v4t_row), A: t = row(M_et, pair(a), tip(l1)),
 * row(M_ed, t, tip(l2)); B: row(M_ed, pair(a), pair(a')).  TIP_MUL and POPMUL multiply elementwise with v_mul_f64, which
 * commutes bit for bit, so the operand order of the products is free.  A row whose index names a rank that does not occur
 * is the row of rank 0 in that digit (padding sites carry code 0, which maps to rank 0 where it does not occur).
 */
struct PlkV4QCand { int at, shape; };

static inline int plk_popcount16(int m) { int n = 0; for (int b = 0; b < 16; b++) n += (m >> b) & 1; return n; }
/* rank of every code at a leaf with the occurring codes `mask` (at most four): increasing code order, 0 where the code does not occur */
static inline void plk_v4q_lut(int mask, uint8_t *lut16)
{
    int r = 0;
    for (int code = 0; code < 16; code++) lut16[code] = (uint8_t)(((mask >> code) & 1) && r < 4 ? r++ : 0);
}
/* the inverse, for the table builder: the code of rank r; a rank that does not occur names the code of rank 0 */
static inline void plk_v4q_rank_codes(int mask, int *code4)
{
    int r = 0;
    for (int code = 0; code < 16 && r < 4; code++) if ((mask >> code) & 1) code4[r++] = code;
    if (r == 0) code4[r++] = 0;
    for (; r < 4; r++) code4[r] = code4[0];
}
/* allocation units of a four-leaf table, and what a table of either shape adds to the image (can be negative) */
PLK_HD static inline int plk_v4q_units(int nchar) { return (PLK_V4Q_ROWS + nchar - 1) / nchar; }
static inline long plk_v4q_extra_units(int nchar, int shape) { return (long)plk_v4q_units(nchar) - (shape == PLK_V4Q_A ? nchar + 2 : 2 * nchar); }

/* the nodes that qualify, in program order: index into in.vops of the first of the five ops */
static inline void plk_v4q_candidates(const PlkFusedPT &in, int nchar, const int *node_codes, std::vector<PlkV4QCand> &at)
{
    at.clear();
    if (!node_codes || nchar < 2 || nchar > 16 || in.ntriples != 0 || in.nquads != 0) return;
    std::vector<int> table_at(std::max(in.units, 1), -1);
    for (size_t t = 0; t < in.tab_unit.size(); t++) if (in.tab_unit[t] >= 0 && in.tab_unit[t] < in.units) table_at[in.tab_unit[t]] = (int)t;
    const std::vector<PlkFusedPT::VOp> &v = in.vops;
    const int nrows = (int)in.row_node.size();
    auto leaf_ok = [&](int node) { const int m = node < 0 ? 0 : node_codes[node]; return m > 0 && m < (1 << nchar) && plk_popcount16(m) <= 4; };
    auto is_pair = [&](const PlkFusedPT::VOp &o) {
        if (o.unit < 0 || o.unit >= in.units || o.row < 0 || o.row >= nrows) return false;
        const int t = table_at[o.unit];
        return t >= 0 && in.tab_eb[t] >= 0 && in.row_node2[o.row] >= 0 && leaf_ok(in.row_node[o.row]) && leaf_ok(in.row_node2[o.row]);
    };
    auto is_leaf = [&](const PlkFusedPT::VOp &o) {
        if (o.unit < 0 || o.unit >= in.units || o.row < 0 || o.row >= nrows) return false;
        const int t = table_at[o.unit];
        return t >= 0 && in.tab_eb[t] < 0 && in.tab_edge[t] >= 0 && in.row_node2[o.row] < 0 && leaf_ok(in.row_node[o.row]);
    };
    for (size_t i = 0; i + 4 < v.size(); i++) {
        if (v[i].code != OP_TIP_SET || v[i + 4].code != OP_MATVEC || !is_pair(v[i])) continue;
        int shape = 0;
        if (v[i + 1].code == OP_TIP_MUL && v[i + 2].code == OP_MATVEC && v[i + 3].code == OP_TIP_MUL && is_leaf(v[i + 1]) && is_leaf(v[i + 3])) shape = PLK_V4Q_A;
        else if (v[i + 1].code == OP_PUSH && v[i + 2].code == OP_TIP_SET && v[i + 3].code == OP_POPMUL && v[i + 3].d == v[i + 1].d && is_pair(v[i + 2])) shape = PLK_V4Q_B;
        if (!shape) continue;
        at.push_back(PlkV4QCand{(int)i, shape});
        i += 4;
    }
}

/* in: a pair-table program plk_fused_check_pt has accepted.  quad_at / quad_shape: the four-leaf nodes to take (entries that
 * plk_v4q_candidates does not name are ignored), tri_at: the three-leaf nodes (plk_v4t_candidates; one inside a taken
 * shape-A node is ignored), all ascending.  out.nquads == 0 && out.ntriples == 0: out is a copy of in. */
static inline void plk_fused_v4q_build(const PlkFusedPT &in, int slots_needed, int nchar, const int *node_codes, const std::vector<int> &tri_at,
                                       const std::vector<int> &quad_at, const std::vector<int> &quad_shape, bool fuse_set, PlkFusedPT &out)
{
    typedef PlkFusedPT::VOp VOp;
    const std::vector<VOp> &v = in.vops;
    std::vector<PlkV4QCand> qc;
    std::vector<int> tc;
    plk_v4q_candidates(in, nchar, node_codes, qc);
    plk_v4t_candidates(in, nchar, tc);
    std::vector<char> kind(v.size(), 0);                  /* 1: A, 2: B, 3: three-leaf */
    for (size_t q = 0; q < quad_at.size() && q < quad_shape.size(); q++)
        for (const PlkV4QCand &c : qc) if (c.at == quad_at[q] && c.shape == quad_shape[q]) kind[c.at] = (char)c.shape;
    for (int a : tri_at) if (std::find(tc.begin(), tc.end(), a) != tc.end() && !kind[a]) kind[a] = 3;
    PlkFusedPT o;
    const int ntab = (int)in.tab_unit.size(), nrows = (int)in.row_node.size(), U4 = plk_v4q_units(std::max(nchar, 1));
    std::vector<int> table_at(std::max(in.units, 1), -1), new_unit(ntab, -1), new_row(nrows, -1);
    for (int t = 0; t < ntab; t++) table_at[in.tab_unit[t]] = t;
    auto table = [&](int edge, int eb, int ec, int ea, int el, int shape, int et, int ef, int eg, int nunits) {
        o.tab_unit.push_back(o.units); o.tab_edge.push_back(edge); o.tab_eb.push_back(eb); o.tab_ec.push_back(ec);
        o.tab_ea.push_back(ea); o.tab_el.push_back(el);
        o.tab_shape.push_back(shape); o.tab_et.push_back(et); o.tab_ef.push_back(ef); o.tab_eg.push_back(eg); o.tab_row.push_back(-1);
        const int u = o.units; o.units += nunits; return u;
    };
    auto row = [&](int n1, int n2, int n3, int n4, int q) {
        o.row_node.push_back(n1); o.row_node2.push_back(n2); o.row_node3.push_back(n3); o.row_node4.push_back(n4); o.row_lut.push_back(q);
        return (int)o.row_node.size() - 1;
    };
    auto quad_row = [&](int n1, int n2, int n3, int n4) {
        const int q = o.nquads++, nd[4] = {n1, n2, n3, n4};
        o.lut.resize((size_t)64 * o.nquads);
        for (int j = 0; j < 4; j++) plk_v4q_lut(node_codes[nd[j]], &o.lut[(size_t)64 * q + 16 * j]);
        return row(n1, n2, n3, n4, q);
    };
    bool pseudo = false;
    for (size_t i = 0; i < v.size(); i++) {
        if (kind[i] == PLK_V4Q_A) {
            const int tp = table_at[v[i].unit], t1 = table_at[v[i + 1].unit], t2 = table_at[v[i + 3].unit], rp = v[i].row;
            const int u = table(v[i + 4].edge, in.tab_eb[tp], in.tab_ec[tp], in.tab_edge[tp], in.tab_edge[t1], PLK_V4Q_A, v[i + 2].edge, in.tab_edge[t2], -1, U4);
            o.vops.push_back(VOp{OP_TIP_SET, u, quad_row(in.row_node[rp], in.row_node2[rp], in.row_node[v[i + 1].row], in.row_node[v[i + 3].row]), 0, -1});
            o.tab_row.back() = o.vops.back().row;
            i += 4;
            continue;
        }
        if (kind[i] == PLK_V4Q_B) {
            const int tp = table_at[v[i].unit], tq = table_at[v[i + 2].unit], rp = v[i].row, rq = v[i + 2].row;
            const int u = table(v[i + 4].edge, in.tab_eb[tp], in.tab_ec[tp], in.tab_edge[tp], -1, PLK_V4Q_B, in.tab_edge[tq], in.tab_eb[tq], in.tab_ec[tq], U4);
            o.vops.push_back(VOp{OP_TIP_SET, u, quad_row(in.row_node[rp], in.row_node2[rp], in.row_node[rq], in.row_node2[rq]), 0, -1});
            o.tab_row.back() = o.vops.back().row;
            i += 4;
            continue;
        }
        if (kind[i] == 3) {
            const int tp = table_at[v[i].unit], tl = table_at[v[i + 1].unit], rp = v[i].row, rl = v[i + 1].row;
            const int u = table(v[i + 2].edge, in.tab_eb[tp], in.tab_ec[tp], in.tab_edge[tp], in.tab_edge[tl], 0, -1, -1, -1, nchar * nchar);
            o.vops.push_back(VOp{OP_TIP_SET, u, row(in.row_node[rp], in.row_node2[rp], in.row_node[rl], -1, -1), 0, -1});
            o.ntriples++;
            i += 2;
            continue;
        }
        VOp w = v[i];
        if (w.code == OP_TIP_SET || w.code == OP_TIP_MUL) {
            const int t = table_at[w.unit];
            if (new_unit[t] < 0) {
                new_unit[t] = table(in.tab_edge[t], in.tab_eb[t], in.tab_ec[t], -1, -1, 0, -1, -1, -1, in.tab_eb[t] >= 0 ? nchar : 1);
                if (in.tab_eb[t] >= 0) o.npairs++;
                if (in.tab_edge[t] < 0) pseudo = true;
            }
            if (new_row[w.row] < 0) new_row[w.row] = row(in.row_node[w.row], in.row_node2[w.row], -1, -1, -1);
            w.unit = new_unit[t]; w.row = new_row[w.row];
        } else if (w.code == OP_MATVEC) o.mat_edge.push_back(w.edge);
        o.vops.push_back(w);
    }
    if (o.nquads == 0 && o.ntriples == 0) { out = in; return; }
    if (!pseudo) table(-1, -1, -1, -1, -1, 0, -1, -1, -1, 1);
    plk_fused_pt_words(slots_needed, fuse_set, o);
    out = std::move(o);
}

/*
 * plk_fused_check_v4t for formats with four-leaf tables: the words are decoded with their look-up chain into out.vops;
 * those, with every four-leaf look-up unfolded into its five ops and every three-leaf look-up into its three, must be
 * in.vops exactly (opcodes, stack slots, SCALE positions, tables of the same edges through rows of the same nodes); the
 * matrix stream is consumed exactly, the absorbed matrices (two per shape A, one per shape B, one per three-leaf table)
 * being the ones missing; every four-leaf table stands for a non-root node of the tree with exactly those children and
 * leaves; the tables tile the unit range; every rank table is the bijection of its leaf's occurring codes (node_codes)
 * onto 0 .. n - 1, n <= 4, in increasing order, and 0 elsewhere; unit and row fields fit the op words.
 */
static inline std::string plk_fused_check_v4q(int N, const int *ip, const int *ix, const PlkFusedPT &in, const PlkFusedPT &out, int nchar,
                                              const int *node_codes)
{
    typedef PlkFusedPT::VOp VOp;
    const int ntab = (int)out.tab_unit.size(), nrows = (int)out.row_node.size(), E = N - 1;
    if (!node_codes || nchar < 2 || nchar > 16) return "v4q program: four-leaf tables need the occurring codes and nchar <= 16";
    if ((int)out.tab_edge.size() != ntab || (int)out.tab_eb.size() != ntab || (int)out.tab_ec.size() != ntab || (int)out.tab_ea.size() != ntab ||
        (int)out.tab_el.size() != ntab || (int)out.tab_shape.size() != ntab || (int)out.tab_et.size() != ntab || (int)out.tab_ef.size() != ntab ||
        (int)out.tab_eg.size() != ntab || (int)out.tab_row.size() != ntab || (int)out.row_node2.size() != nrows || (int)out.row_node3.size() != nrows ||
        (int)out.row_node4.size() != nrows || (int)out.row_lut.size() != nrows) return "v4q program: table sizes";
    if (nrows < 1 || out.units < 1 || out.units >= 2048 || nrows >= 65536) return "v4q program: field widths";
    if (out.nquads < 0 || out.lut.size() != (size_t)64 * out.nquads) return "v4q program: rank tables";
    auto tkind = [&](int t) { return out.tab_shape[t] != 0 ? 4 : out.tab_el[t] >= 0 ? 3 : out.tab_eb[t] >= 0 ? 2 : 1; };
    auto rkind = [&](long r) { return out.row_node4[r] >= 0 ? 4 : out.row_node3[r] >= 0 ? 3 : out.row_node2[r] >= 0 ? 2 : 1; };
    std::vector<int> table_at(out.units, -1), in_table_at(std::max(in.units, 1), -1);
    int expect = 0, ntri = 0, nquad = 0;
    for (int t = 0; t < ntab; t++) {
        if (out.tab_shape[t] != 0 && out.tab_shape[t] != PLK_V4Q_A && out.tab_shape[t] != PLK_V4Q_B) return "v4q program: table shape";
        if (tkind(t) == 3 && nchar * nchar * nchar > 256) return "v4q program: the combined code must stay a byte";
        const int nu = plk_pt_table_units(out, (size_t)t, nchar);
        if (out.tab_unit[t] != expect || expect + nu > out.units) return "v4q program: table layout";
        table_at[expect] = t;
        expect += nu;
        if (tkind(t) == 3) ntri++;
        if (tkind(t) == 4) nquad++;
    }
    if (expect != out.units || ntri != out.ntriples || nquad != out.nquads) return "v4q program: table layout";
    for (size_t t = 0; t < in.tab_unit.size(); t++) if (in.tab_unit[t] >= 0 && in.tab_unit[t] < in.units) in_table_at[in.tab_unit[t]] = (int)t;
    /* rows: a four-leaf row names four nodes and a rank table of its own, which is the bijection of the nodes' codes */
    {
        std::vector<char> lut_used(std::max(out.nquads, 1), 0);
        for (int r = 0; r < nrows; r++) {
            const int q = out.row_lut[r];
            if ((q >= 0) != (out.row_node4[r] >= 0)) return plk_fmt("v4q program: row %ld and its rank tables", r);
            if (q < 0) continue;
            if (q >= out.nquads || lut_used[q]++) return plk_fmt("v4q program: rank tables of row %ld", r);
            const int nd[4] = {out.row_node[r], out.row_node2[r], out.row_node3[r], out.row_node4[r]};
            for (int j = 0; j < 4; j++) {
                if (nd[j] < 0 || nd[j] >= N) return plk_fmt("v4q program: row %ld names a node out of range", r);
                const int m = node_codes[nd[j]];
                if (m <= 0 || m >= (1 << nchar) || plk_popcount16(m) > 4) return plk_fmt("v4q program: leaf %ld of row %ld takes more than four codes", j, r);
                int rank = 0;
                for (int code = 0; code < 16; code++) {
                    const int want = ((m >> code) & 1) ? rank++ : 0;
                    if (out.lut[(size_t)64 * q + 16 * j + code] != want) return plk_fmt("v4q program: rank table of leaf %ld of row %ld at code %ld", j, r, code);
                }
            }
        }
    }
    /* the words, decoded: the chain delivers (cur_unit, cur_row) to every observation handler */
    std::vector<VOp> dec;
    {
        if (out.words.size() % 8 != 0 || out.words.size() < 16) return "v4q program: word buffer";
        auto unit_ok = [&](long u) { return u >= 0 && u < out.units && table_at[u] >= 0; };
        auto row_ok = [&](long r) { return r >= 0 && r < nrows; };
        long cur_unit = out.first_unit, cur_row = out.first_row, next_row = out.second_row;
        if (!unit_ok(cur_unit) || !row_ok(cur_row) || !row_ok(next_row)) return "v4q program: prologue fields";
        if (rkind(cur_row) > tkind(table_at[cur_unit]) || (rkind(cur_row) == 4) != (tkind(table_at[cur_unit]) == 4)) return "v4q program: prologue fields";
        bool waited = true, ended = false;
        for (size_t wi = 0; wi < out.words.size() && !ended; wi++) {
            const unsigned w = out.words[wi], hidx = w & 31, y = (w >> 5) & 0x7ff, z = w >> 16;
            auto observe = [&](int code) -> bool {
                dec.push_back(VOp{code, (int)cur_unit, (int)cur_row, 0, -1});
                if (!unit_ok(y) || !row_ok(z)) return false;
                /* a row's largest code must fit the table it indexes; a four-leaf row's byte is a rank index: its own kind only */
                const int kt = tkind(table_at[y]), kr = rkind(next_row);
                if (kr > kt || (kr == 4) != (kt == 4)) return false;
                cur_unit = y; cur_row = next_row; next_row = z;
                waited = false;
                return true;
            };
            bool ok = true;
            if (hidx == OP_END) ended = true;
            else if (hidx == OP_MATVEC) { dec.push_back(VOp{OP_MATVEC, 0, 0, 0, -1}); waited = true; }
            else if (hidx == PLK_WORD_MATVEC_TIPMUL) { dec.push_back(VOp{OP_MATVEC, 0, 0, 0, -1}); waited = true; ok = observe(OP_TIP_MUL); }
            else if (hidx == OP_TIP_SET) ok = observe(OP_TIP_SET);
            else if (hidx == OP_TIP_MUL) ok = observe(OP_TIP_MUL);
            else if (hidx == PLK_WORD_TIPMUL_NOWAIT) { if (!waited) return plk_fmt("v4q program: word %ld skips a wait it needs", (long)wi); ok = observe(OP_TIP_MUL); }
            else if (hidx == OP_SCALE) dec.push_back(VOp{OP_SCALE, 0, 0, 0, -1});
            else if (hidx >= PLK_WORD_SET_POPMUL && hidx < PLK_WORD_SET_POPMUL + 4) { ok = observe(OP_TIP_SET); dec.push_back(VOp{OP_POPMUL, 0, 0, (int)(hidx & 3), -1}); }
            else if (hidx >= PLK_WORD_SET_PUSH && hidx < PLK_WORD_SET_PUSH + 4) { ok = observe(OP_TIP_SET); dec.push_back(VOp{OP_PUSH, 0, 0, (int)(hidx & 3), -1}); }
            else if (hidx >= 24) { dec.push_back(VOp{OP_MATVEC, 0, 0, 0, -1}); waited = true; dec.push_back(VOp{hidx < 28 ? OP_PUSH : OP_POPMUL, 0, 0, (int)(hidx & 3), -1}); }
            else if (hidx >= 8 && hidx < 12) dec.push_back(VOp{OP_PUSH, 0, 0, (int)(hidx & 7), -1});
            else if (hidx >= 16 && hidx < 20) dec.push_back(VOp{OP_POPMUL, 0, 0, (int)(hidx & 7), -1});
            else return plk_fmt("v4q program: word %ld jumps to an empty handler slot", (long)wi);
            if (!ok) return plk_fmt("v4q program: word %ld requests a table or a row out of range", (long)wi);
        }
        if (!ended) return "v4q program: no END";
    }
    if (dec.size() != out.vops.size()) return plk_fmt("v4q program: the words execute %ld ops, the rewritten program has %ld", (long)dec.size(), (long)out.vops.size());
    for (size_t i = 0; i < dec.size(); i++) {
        const VOp &a = dec[i], &b = out.vops[i];
        const bool obs = b.code == OP_TIP_SET || b.code == OP_TIP_MUL;
        if (a.code != b.code || (obs && (a.unit != b.unit || a.row != b.row)) || ((b.code == OP_PUSH || b.code == OP_POPMUL) && a.d != b.d))
            return plk_fmt("v4q program: decoded op %ld is not the rewritten program's", (long)i);
    }
    /* the rewritten ops, unfolded, against the checked ones */
    size_t j = 0, mi = 0;
    int absorbed = 0, tri_seen = 0, quad_seen = 0;
    std::vector<char> used(ntab, 0);
    auto in_tab = [&](const VOp &b) { return b.unit < 0 || b.unit >= in.units || b.row < 0 || b.row >= (int)in.row_node.size() ? -1 : in_table_at[b.unit]; };
    auto same_single = [&](const VOp &a, const VOp &b) {       /* a of out, b of in: one look-up of the same table through the same row */
        const int ti = in_tab(b);
        if (ti < 0) return false;
        const int t = table_at[a.unit];
        return tkind(t) <= 2 && out.tab_edge[t] == in.tab_edge[ti] && out.tab_eb[t] == in.tab_eb[ti] && out.tab_ec[t] == in.tab_ec[ti] &&
               out.row_node[a.row] == in.row_node[b.row] && out.row_node2[a.row] == in.row_node2[b.row] && out.row_node3[a.row] == -1 && out.row_node4[a.row] == -1;
    };
    auto edge_ok = [&](int e) { return e >= 0 && e < E; };
    auto is_leaf = [&](int n) { return n >= 0 && n < N && ip[n + 1] == ip[n]; };
    /* a = ix[ea] is a cherry of the leaf edges eb, ec */
    auto cherry = [&](int ea, int eb, int ec) {
        if (!edge_ok(ea) || !edge_ok(eb) || !edge_ok(ec) || eb == ec) return false;
        const int a = ix[ea];
        return ip[a + 1] - ip[a] == 2 && plk_edge_parent(N, ip, eb) == a && plk_edge_parent(N, ip, ec) == a && is_leaf(ix[eb]) && is_leaf(ix[ec]);
    };
    for (size_t i = 0; i < out.vops.size(); i++) {
        const VOp &a = out.vops[i];
        if (j >= in.vops.size()) return "v4q program: more ops than the checked program";
        const VOp &b = in.vops[j];
        if (a.code == OP_TIP_SET || a.code == OP_TIP_MUL) {
            const int t = table_at[a.unit], kt = tkind(t);
            if (used[t]++ && out.tab_edge[t] >= 0) return plk_fmt("v4q program: table %ld used twice", (long)t);
            if (kt <= 2) {
                if (a.code != b.code || !same_single(a, b)) return plk_fmt("v4q program: look-up %ld is not the checked program's", (long)i);
                j++;
                continue;
            }
            const int e = out.tab_edge[t], ea = out.tab_ea[t], eb = out.tab_eb[t], ec = out.tab_ec[t];
            if (a.code != OP_TIP_SET || !edge_ok(e)) return plk_fmt("v4q program: table look-up %ld", (long)i);
            const int d = ix[e];
            if (ip[d + 1] - ip[d] != 2 || !cherry(ea, eb, ec) || out.row_node[a.row] != ix[eb] || out.row_node2[a.row] != ix[ec])
                return plk_fmt("v4q program: table %ld does not stand for a node with two children above a cherry", (long)t);
            if (kt == 3) {
                /* a three-leaf look-up: the checked program continues with the cherry's look-up, the leaf's and the MATVEC */
                if (j + 2 >= in.vops.size()) return plk_fmt("v4q program: three-leaf look-up %ld", (long)i);
                const VOp &bp = in.vops[j], &bl = in.vops[j + 1], &bm = in.vops[j + 2];
                if (bp.code != OP_TIP_SET || bl.code != OP_TIP_MUL || bm.code != OP_MATVEC) return plk_fmt("v4q program: three-leaf look-up %ld does not stand for look-up, look-up, MATVEC", (long)i);
                const int tp = in_tab(bp), tl = in_tab(bl), el = out.tab_el[t];
                if (tp < 0 || tl < 0 || in.tab_eb[tp] < 0 || in.tab_eb[tl] >= 0 || in.tab_edge[tl] < 0) return plk_fmt("v4q program: three-leaf look-up %ld: not a cherry and a leaf", (long)i);
                if (eb != in.tab_eb[tp] || ec != in.tab_ec[tp] || ea != in.tab_edge[tp] || el != in.tab_edge[tl] || e != bm.edge)
                    return plk_fmt("v4q program: three-leaf table %ld holds other edges than the ops it stands for", (long)t);
                if (out.row_node[a.row] != in.row_node[bp.row] || out.row_node2[a.row] != in.row_node2[bp.row] || out.row_node3[a.row] != in.row_node[bl.row] ||
                    in.row_node2[bl.row] != -1 || out.row_node4[a.row] != -1) return plk_fmt("v4q program: row of three-leaf look-up %ld", (long)i);
                if (!edge_ok(el) || plk_edge_parent(N, ip, ea) != d || plk_edge_parent(N, ip, el) != d || ea == el || !is_leaf(ix[el]) || out.row_node3[a.row] != ix[el])
                    return plk_fmt("v4q program: three-leaf table %ld is not a cherry and a leaf under one node", (long)t);
                absorbed++; tri_seen++;
                j += 3;
                continue;
            }
            if (j + 4 >= in.vops.size()) return plk_fmt("v4q program: four-leaf look-up %ld", (long)i);
            const VOp *bb = &in.vops[j];
            const int et = out.tab_et[t], ef = out.tab_ef[t];
            if (out.tab_shape[t] == PLK_V4Q_A) {
                if (bb[0].code != OP_TIP_SET || bb[1].code != OP_TIP_MUL || bb[2].code != OP_MATVEC || bb[3].code != OP_TIP_MUL || bb[4].code != OP_MATVEC)
                    return plk_fmt("v4q program: four-leaf look-up %ld does not stand for look-up, look-up, MATVEC, look-up, MATVEC", (long)i);
                const int tp = in_tab(bb[0]), t1 = in_tab(bb[1]), t2 = in_tab(bb[3]), el = out.tab_el[t];
                if (tp < 0 || t1 < 0 || t2 < 0 || in.tab_eb[tp] < 0 || in.tab_eb[t1] >= 0 || in.tab_edge[t1] < 0 || in.tab_eb[t2] >= 0 || in.tab_edge[t2] < 0)
                    return plk_fmt("v4q program: four-leaf look-up %ld: not a cherry and two leaves", (long)i);
                if (eb != in.tab_eb[tp] || ec != in.tab_ec[tp] || ea != in.tab_edge[tp] || el != in.tab_edge[t1] || et != bb[2].edge || ef != in.tab_edge[t2] ||
                    e != bb[4].edge || out.tab_eg[t] != -1) return plk_fmt("v4q program: four-leaf table %ld holds other edges than the ops it stands for", (long)t);
                if (out.row_node[a.row] != in.row_node[bb[0].row] || out.row_node2[a.row] != in.row_node2[bb[0].row] || out.row_node3[a.row] != in.row_node[bb[1].row] ||
                    out.row_node4[a.row] != in.row_node[bb[3].row] || in.row_node2[bb[1].row] != -1 || in.row_node2[bb[3].row] != -1)
                    return plk_fmt("v4q program: row of four-leaf look-up %ld", (long)i);
                /* the tree: d = (t, l2) under e, t = (a, l1) under et */
                if (!edge_ok(et) || !edge_ok(ef) || !edge_ok(el) || et == ef || plk_edge_parent(N, ip, et) != d || plk_edge_parent(N, ip, ef) != d)
                    return plk_fmt("v4q program: four-leaf table %ld: children of its node", (long)t);
                const int tn = ix[et];
                if (ip[tn + 1] - ip[tn] != 2 || plk_edge_parent(N, ip, ea) != tn || plk_edge_parent(N, ip, el) != tn || ea == el || !is_leaf(ix[el]) || !is_leaf(ix[ef]) ||
                    out.row_node3[a.row] != ix[el] || out.row_node4[a.row] != ix[ef]) return plk_fmt("v4q program: four-leaf table %ld is not ((cherry, leaf), leaf)", (long)t);
                absorbed += 2;
            } else {
                if (bb[0].code != OP_TIP_SET || bb[1].code != OP_PUSH || bb[2].code != OP_TIP_SET || bb[3].code != OP_POPMUL || bb[4].code != OP_MATVEC || bb[1].d != bb[3].d)
                    return plk_fmt("v4q program: four-leaf look-up %ld does not stand for look-up, PUSH, look-up, POPMUL, MATVEC", (long)i);
                const int tp = in_tab(bb[0]), tq = in_tab(bb[2]), eg = out.tab_eg[t];
                if (tp < 0 || tq < 0 || in.tab_eb[tp] < 0 || in.tab_eb[tq] < 0) return plk_fmt("v4q program: four-leaf look-up %ld: not two cherries", (long)i);
                if (eb != in.tab_eb[tp] || ec != in.tab_ec[tp] || ea != in.tab_edge[tp] || ef != in.tab_eb[tq] || eg != in.tab_ec[tq] || et != in.tab_edge[tq] ||
                    e != bb[4].edge || out.tab_el[t] != -1) return plk_fmt("v4q program: four-leaf table %ld holds other edges than the ops it stands for", (long)t);
                if (out.row_node[a.row] != in.row_node[bb[0].row] || out.row_node2[a.row] != in.row_node2[bb[0].row] || out.row_node3[a.row] != in.row_node[bb[2].row] ||
                    out.row_node4[a.row] != in.row_node2[bb[2].row]) return plk_fmt("v4q program: row of four-leaf look-up %ld", (long)i);
                if (!cherry(et, ef, eg) || ea == et || plk_edge_parent(N, ip, ea) != d || plk_edge_parent(N, ip, et) != d ||
                    out.row_node3[a.row] != ix[ef] || out.row_node4[a.row] != ix[eg]) return plk_fmt("v4q program: four-leaf table %ld is not (cherry, cherry)", (long)t);
                absorbed += 1;
            }
            if (out.tab_row[t] != a.row) return plk_fmt("v4q program: four-leaf table %ld names another row than the look-up that reads it", (long)t);
            quad_seen++;
            j += 5;
            continue;
        }
        if (a.code != b.code) return plk_fmt("v4q program: op %ld is not the checked program's", (long)i);
        if (a.code == OP_MATVEC) {
            if (mi >= out.mat_edge.size() || out.mat_edge[mi] != b.edge || a.edge != b.edge) return plk_fmt("v4q program: matrix %ld is not the op's edge", (long)mi);
            mi++;
        } else if ((a.code == OP_PUSH || a.code == OP_POPMUL) && a.d != b.d) return plk_fmt("v4q program: stack op %ld", (long)i);
        j++;
    }
    if (j != in.vops.size()) return "v4q program: the checked program's ops are not all covered";
    if (mi != out.mat_edge.size() || out.mat_edge.size() + (size_t)absorbed != in.mat_edge.size()) return "v4q program: matrix stream not consumed exactly";
    if (tri_seen != out.ntriples || quad_seen != out.nquads) return "v4q program: tables that no op reads";
    return "";
}

/*
 * The plan with four-leaf tables: for every candidate G of plk_v4t_plan the room is filled greedily by gain per unit with
 *   a three-leaf table                      PLK_V4T_NODE_INSTS      for nchar^2 - nchar - 1 units
 *   a shape-A table over a taken three-leaf table   + PLK_V4T_NODE_INSTS  for the difference (alone: twice, for 256 / nchar - nchar - 2)
 *   a shape-B table                         PLK_V4T_NODE_INSTS      for 256 / nchar - 2 nchar units
 * (tables that shrink the image first), and the G with the largest gain under plk_v4t_plan's phase charge wins.  quad = 1
 * keeps the PLK_V4T_MIN_PASSES gate of the default, quad = 2 takes the best candidate whatever the model says of it.
 */
static inline PlkV4TPlan plk_v4q_plan(const PlkFusedPT &fpt, int nchar, int C, long S, int num_cus, size_t static_lds, int quad, int groups_opt,
                                      const int *node_codes)
{
    PlkV4TPlan best;
    best.Cg = C;
    std::vector<PlkV4QCand> qc;
    std::vector<int> tc;
    plk_v4q_candidates(fpt, nchar, node_codes, qc);
    if (quad == 0 || qc.empty() || C < 1 || S < 1) return best;
    plk_v4t_candidates(fpt, nchar, tc);
    const long nunits = (S + PLK_V4S_UNIT - 1) / PLK_V4S_UNIT;
    const long waves = std::min<long>((nunits + 11) / 12, std::max(num_cus, 1)) * 12;
    const long passes = (nunits + waves - 1) / waves;
    if (quad == 1 && passes < PLK_V4T_MIN_PASSES) return best;
    const size_t unit_bytes = (size_t)nchar * 32, image = (size_t)fpt.units * unit_bytes, limit = plk_pt_lds_limit(1024);
    const long tri_units = (long)nchar * nchar - nchar - 1;
    struct Item { int kind, at; long gain, cost; double density; };      /* kind: 0 three-leaf, PLK_V4Q_A, PLK_V4Q_B */
    std::vector<Item> items;
    auto item = [&](int kind, int at, long gain, long cost) { items.push_back(Item{kind, at, gain, cost, cost <= 0 ? 1e300 : (double)gain / (double)cost}); };
    for (int a : tc) item(0, a, PLK_V4T_NODE_INSTS, tri_units);
    for (const PlkV4QCand &c : qc) {
        const bool over = c.shape == PLK_V4Q_A && std::find(tc.begin(), tc.end(), c.at) != tc.end();
        if (c.shape == PLK_V4Q_A) item(PLK_V4Q_A, c.at, over ? PLK_V4T_NODE_INSTS : 2 * PLK_V4T_NODE_INSTS, plk_v4q_extra_units(nchar, PLK_V4Q_A) - (over ? tri_units : 0));
        else item(PLK_V4Q_B, c.at, PLK_V4T_NODE_INSTS, plk_v4q_extra_units(nchar, PLK_V4Q_B));
    }
    std::stable_sort(items.begin(), items.end(), [](const Item &x, const Item &y) { return x.density > y.density; });
    double best_gain = quad == 2 ? -1e300 : 0.0;
    const int cand[3] = {1, 2, C};
    for (int q = 0; q < 3; q++) {
        const int G = cand[q];
        if (G < 1 || G > C || (q > 0 && G == cand[q - 1]) || (q == 2 && G == 1)) continue;
        if (groups_opt > 0 && G != std::min(groups_opt, C)) continue;
        if (groups_opt == -1 && G != C) continue;
        const int Cg = (C + G - 1) / G, groups = (C + Cg - 1) / Cg;
        if (static_lds + (size_t)Cg * image > limit) continue;
        long room = (long)(((limit - static_lds) / (size_t)Cg - image) / unit_bytes), units = fpt.units, insts = 0;
        std::vector<int> tri, qa, qs;
        auto fits = [&](long cost) { return cost <= room && units + cost < 2048; };
        for (const Item &it : items) {
            if (it.kind == 0) {
                if (std::find(qa.begin(), qa.end(), it.at) != qa.end() || !fits(it.cost)) continue;
                tri.push_back(it.at); room -= it.cost; units += it.cost; insts += it.gain;
            } else if (it.kind == PLK_V4Q_A) {
                const std::vector<int>::iterator inner = std::find(tri.begin(), tri.end(), it.at);
                const bool over = std::find(tc.begin(), tc.end(), it.at) != tc.end();
                /* priced over its three-leaf table: where that one was not taken, the whole table and both products */
                const long cost = over && inner == tri.end() ? it.cost + tri_units : it.cost, gain = over && inner == tri.end() ? 2 * it.gain : it.gain;
                if (!fits(cost)) continue;
                if (inner != tri.end()) tri.erase(inner);
                qa.push_back(it.at); qs.push_back(PLK_V4Q_A); room -= cost; units += cost; insts += gain;
            } else {
                if (!fits(it.cost)) continue;
                qa.push_back(it.at); qs.push_back(PLK_V4Q_B); room -= it.cost; units += it.cost; insts += it.gain;
            }
        }
        if (tri.empty() && qa.empty()) continue;
        const double gain = (double)C * (double)insts * (double)passes -
                            (double)(groups - 1) * (PLK_V4T_PHASE_INSTS + (double)PLK_V4T_PHASE_UNIT_INSTS * (double)passes);
        if (gain > best_gain) {
            best_gain = gain; best.groups = groups; best.Cg = Cg; best.nodes = (int)tri.size(); best.quads = (int)qa.size();
            best.extra_bytes = (size_t)std::max<long>(units - fpt.units, 0) * unit_bytes;
            std::sort(tri.begin(), tri.end());
            std::vector<size_t> ord(qa.size());
            for (size_t k = 0; k < ord.size(); k++) ord[k] = k;
            std::sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return qa[x] < qa[y]; });
            best.tri_at = tri; best.quad_at.clear(); best.quad_shape.clear();
            for (size_t k : ord) { best.quad_at.push_back(qa[k]); best.quad_shape.push_back(qs[k]); }
        }
    }
    return best;
}

/*
 * The vector ll kernel (k_ll_vec, plk_vec.h) on the pair-table program: int4 ops
 *   observation (TIP_SET / TIP_MUL)  x = opcode, y = first row of the op's table (unit * nchar: the kernel adds the code),
 *                                    w = staged row of the NEXT observation op (cyclic)
 *   MATVEC                           x = opcode, z = op index of the next MATVEC (cyclic; its matrix lines are touched ahead)
 *   PUSH / POPMUL y = slot;  SCALE
 * op_edge[pc] = CSR edge of a MATVEC op (-1 otherwise): the matrix stream is indexed by op.
 */
struct PlkVecPT {
    std::vector<plk_op4> ops;
    std::vector<int> op_edge;
    int first_base = 0, first_row = 0;
};

static inline void plk_vec_pt_build(const PlkFusedPT &fu, int nchar, PlkVecPT &vp)
{
    const int n = (int)fu.vops.size();
    vp.ops.assign(n, plk_op4{OP_END, 0, 0, 0});
    vp.op_edge.assign(n, -1);
    std::vector<int> obs_idx, mv_idx;
    for (int i = 0; i < n; i++) {
        const PlkFusedPT::VOp &o = fu.vops[i];
        vp.ops[i].x = o.code;
        if (o.code == OP_TIP_SET || o.code == OP_TIP_MUL) { vp.ops[i].y = o.unit * nchar; obs_idx.push_back(i); }
        else if (o.code == OP_MATVEC) { vp.op_edge[i] = o.edge; mv_idx.push_back(i); }
        else if (o.code == OP_PUSH || o.code == OP_POPMUL) vp.ops[i].y = o.d;
    }
    for (size_t q = 0; q < obs_idx.size(); q++) vp.ops[obs_idx[q]].w = fu.vops[obs_idx[(q + 1) % obs_idx.size()]].row;
    for (size_t q = 0; q < mv_idx.size(); q++) vp.ops[mv_idx[q]].z = mv_idx[(q + 1) % mv_idx.size()];
    vp.first_base = obs_idx.empty() ? 0 : fu.vops[obs_idx[0]].unit * nchar;
    vp.first_row = obs_idx.empty() ? 0 : fu.vops[obs_idx[0]].row;
}

/* replay against the program: the ops fold exactly the program's ops (a pair look-up stands for a cherry's three ops), rows
 * and tables are the ones of the op, every index is in range */
static inline std::string plk_vec_pt_check(int N, const int *ip, const int *ix, const PlkProgram &pg, const PlkFusedPT &fu, const PlkVecPT &vp,
                                           int nchar, int E)
{
    const int nops = (int)pg.ops.size(), n = (int)vp.ops.size(), nrows = (int)fu.row_node.size(), ntab = (int)fu.tab_unit.size();
    if ((int)vp.op_edge.size() != n || (int)fu.vops.size() != n) return "vec pt program: sizes";
    std::vector<int> table_at(std::max(fu.units, 1), -1);
    for (int t = 0; t < ntab; t++) if (fu.tab_unit[t] >= 0 && fu.tab_unit[t] < fu.units) table_at[fu.tab_unit[t]] = t;
    size_t pc = 0;
    long next_row = vp.first_row, next_base = vp.first_base;
    bool first = true;
    std::vector<char> full(std::max(pg.slots_needed, 1), 0);
    int last_mv = -1, first_mv = -1;
    for (int i = 0; i < n; i++) {
        const plk_op4 &o = vp.ops[i];
        const int code = o.x & 0xff;
        if (pc >= (size_t)nops) return "vec pt program: more ops than the program";
        const int pcode = pg.ops[pc].x & 0xff;
        if (code == OP_TIP_SET || code == OP_TIP_MUL) {
            if (o.y % nchar != 0 || o.y / nchar < 0 || o.y / nchar >= fu.units || table_at[o.y / nchar] < 0) return plk_fmt("vec pt program: op %ld names no table", i);
            const int t = table_at[o.y / nchar];
            if (o.w < 0 || o.w >= nrows) return plk_fmt("vec pt program: op %ld prefetches a row out of range", i);
            if (next_row < 0 || next_row >= nrows || (!first && false)) return "vec pt program: row chain";
            if (next_base != o.y) return plk_fmt("vec pt program: op %ld: the chain's table is not the op's", i);
            const int row = (int)next_row;
            if (fu.tab_eb[t] >= 0) {
                if (code != OP_TIP_SET || !plk_pair_at(N, ip, ix, pg, pc)) return plk_fmt("vec pt program: op %ld is a pair look-up where the program has no cherry", i);
                if (fu.tab_eb[t] != pg.op_edge[pc] || fu.tab_ec[t] != pg.op_edge[pc + 1] || fu.tab_edge[t] != pg.op_edge[pc + 2]) return plk_fmt("vec pt program: pair table of op %ld", i);
                if (fu.row_node[row] != pg.ops[pc].y || fu.row_node2[row] != pg.ops[pc + 1].y) return plk_fmt("vec pt program: pair row of op %ld", i);
                pc += 3;
            } else {
                if (pcode != OP_TIP_SET && pcode != OP_TIP_MUL && pcode != OP_NODE_MUL) return plk_fmt("vec pt program: op %ld is not an observation", i);
                if ((code == OP_TIP_SET) != (pcode == OP_TIP_SET)) return plk_fmt("vec pt program: op %ld SET/MUL", i);
                if (fu.row_node[row] != pg.ops[pc].y || fu.row_node2[row] != -1) return plk_fmt("vec pt program: row of op %ld", i);
                if (fu.tab_edge[t] != (pcode == OP_NODE_MUL ? -1 : pg.op_edge[pc])) return plk_fmt("vec pt program: table of op %ld", i);
                pc++;
            }
            /* the chain: this op names the row of the next observation; its table base is found at that op */
            next_row = o.w;
            next_base = -1;
            for (int q = 1; q <= n; q++) {
                const plk_op4 &o2 = vp.ops[(i + q) % n];
                if ((o2.x & 0xff) == OP_TIP_SET || (o2.x & 0xff) == OP_TIP_MUL) { next_base = o2.y; break; }
            }
            first = false;
        } else if (code == OP_MATVEC) {
            if (pcode != OP_MATVEC || vp.op_edge[i] != pg.op_edge[pc] || vp.op_edge[i] < 0 || vp.op_edge[i] >= E) return plk_fmt("vec pt program: product %ld", i);
            if (o.z < 0 || o.z >= n || (vp.ops[o.z].x & 0xff) != OP_MATVEC) return plk_fmt("vec pt program: op %ld names no next product", i);
            if (first_mv < 0) first_mv = i;
            last_mv = i;
            pc++;
        } else if (code == OP_PUSH || code == OP_POPMUL) {
            if (pcode != code || o.y != pg.ops[pc].y || o.y < 0 || o.y >= (int)full.size() || (full[o.y] != 0) == (code == OP_PUSH)) return plk_fmt("vec pt program: stack op %ld", i);
            full[o.y] = code == OP_PUSH;
            pc++;
        } else if (code == OP_SCALE) {
            if (pcode != OP_SCALE) return plk_fmt("vec pt program: op %ld", i);
            pc++;
        } else return plk_fmt("vec pt program: unknown op %ld", i);
    }
    if ((int)pc != nops) return "vec pt program: the program's ops are not all covered";
    if (last_mv >= 0 && vp.ops[last_mv].z != first_mv) return "vec pt program: the product chain does not wrap to the first";
    return "";
}

/* the C++ interpreter k_ll_fused4<D, NS> (plk_fused4.h): pair-ahead fetch, one-ahead code row chain */
static inline std::string plk_fused_check_cpp(int N, const PlkProgram &pg, const PlkFused &fu, int nchar, int D, int NS,
                                              size_t lds_bytes_launched)
{
    const int nops = (int)pg.ops.size(), ntips1 = (int)pg.tip_edge.size() + 1, nobs = (int)pg.obs_nodes.size();
    if (D != 4 && D != 8 && D != 16) return "fused program: stack depth variant";
    if (pg.slots_needed > D) return "fused program: the tree needs a deeper register stack";
    if (nchar < 1 || nchar > 256) return "fused program: nchar out of range";
    if ((size_t)ntips1 * nchar * 32 + (size_t)nobs * PLK_TILE * NS > lds_bytes_launched) return "fused program: LDS image larger than the launch's dynamic LDS";
    if (lds_bytes_launched > PLK_LDS_LIMIT) return "fused program: dynamic LDS above the limit";
    /* the loop runs over even pc < nops and fetches the pair (pc + 2, pc + 3) while it executes (pc, pc + 1) */
    const int last_pc = nops > 0 ? ((nops - 1) / 2) * 2 : 0;
    if (fu.fops.size() < 2 || (nops > 0 && (size_t)(last_pc + 3) >= fu.fops.size())) return "fused program: op buffer too short for the look-ahead";
    std::vector<int> slot, rowv, opc;
    plk_obs_sequence(N, pg, slot, rowv, opc);
    if (fu.first_row < 0 || fu.first_row >= std::max(nobs, 1)) return "fused program: first row out of range";
    long cur_row = fu.first_row;
    size_t oi = 0;
    int mi = 0;
    for (int pc = 0; pc < nops; pc++) {
        const plk_op4 f = fu.fops[pc];
        const int code = f.x & 0xff;
        if (code != (pg.ops[pc].x & 0xff)) return "fused program: opcode mismatch";
        if (code == OP_TIP_SET || code == OP_TIP_MUL || code == OP_NODE_MUL) {
            if (oi >= slot.size() || cur_row != rowv[oi]) return plk_fmt("fused program: code chain delivers the wrong row at op %ld", pc);
            if (code != OP_NODE_MUL && ((f.x >> 8) < 0 || (f.x >> 8) >= ntips1 - 1)) return "fused program: tip slot out of range";
            if (f.z < 0 || f.z >= nobs) return "fused program: next row out of range";
            cur_row = f.z;
            oi++;
        } else if (code == OP_MATVEC) {
            if (f.w != mi || fu.mat_edge[mi] != pg.op_edge[pc]) return "fused program: matrix index mismatch";
            mi++;
        } else if (code == OP_PUSH || code == OP_POPMUL) {
            if (f.y < 0 || f.y >= D) return "fused program: stack slot out of range";
        }
    }
    for (size_t pc = nops; pc < fu.fops.size(); pc++) if ((fu.fops[pc].x & 0xff) != OP_END) return "fused program: padding is not END";
    return "";
}

/* ------------------------------------------------------------------------------------------------------------ */
/* which k = 4 ll kernel runs and which formats: the one place that decides, for the engine and the CPU tests  */
/* ------------------------------------------------------------------------------------------------------------ */

enum PlkK4Variant { PLK_K4_NONE = 0, PLK_K4_CPP, PLK_K4_ASM, PLK_K4_ASM_PT, PLK_K4_V4, PLK_K4_V4S };
enum { PLK_K4_LDS_V4S_768 = 0, PLK_K4_LDS_V4_768, PLK_K4_LDS_V4_512 };     /* PlkK4Shape::static_lds */

/* PLK_OPT_PAIR_TABLES: & 7 which pair-table kernel (0 with the whole value 0: none; 1 the default order; 2, 3, 5, 6 one
 * kernel and tile, forced; 7 the streamed form wherever it fits), + 8 without the scalar-cache warm-up, + 16 / + 32 the
 * waves of the streamed form meet before every unit only / never (+ 32 wins over + 16), + 65536 before every category whatever
 * the plan (default: before every category, or never where one category is resident at a time: plk_v4s_auto_sync), + 64 the streamed form
 * as it was before the folded op stream and the held first chunks (the checked stream unfolded, every category requests
 * the unit's first three chunks itself), + 128 / + 256 without the held chunks only / without the fold only, + 512 without the
 * pair-product form (the folded stream with held chunks on every tree; that form needs both, so + 64 / + 128 / + 256 turn
 * it off as well), + 1024 the three-leaf form of the streamed kernel (plk_fused_v4t_build) wherever it applies, whatever the
 * site count, + 2048 never, + 4096 / + 8192 / both its categories in one group / a group per category / two groups (more
 * than one group needs the pair-product form), + 16384 the four-leaf form (plk_fused_v4q_build) wherever it applies, whatever
 * the site count (it implies + 1024), + 32768 never; + 1024 alone keeps to three-leaf tables, + 2048 forbids both.
 * The + bits are for measurements. */
struct PlkPairTablesOpt { bool on; int mode, warm, sync /* -1: the plan's choice */, fold, held, pair, triple, groups, quad; };
static inline PlkPairTablesOpt plk_pair_tables_opt(long v)
{
    const int quad = (v & (2048 | 32768)) ? 0 : (v & 16384) ? 2 : (v & 1024) ? 0 : 1;
    return {v != 0, (int)(v & 7), (v & 8) ? 0 : 1, (v & 32) ? 0 : (v & 16) ? 1 : (v & 65536) ? 2 : -1, (v & (64 | 256)) ? 0 : 1, (v & (64 | 128)) ? 0 : 1,
            (v & (64 | 128 | 256 | 512)) ? 0 : 1, (v & 2048) ? 0 : (v & 1024) || quad == 2 ? 2 : 1,
            (v & (4096 | 8192)) == (4096 | 8192) ? 2 : (v & 4096) ? 1 : (v & 8192) ? -1 : 0, quad};
}

/* Do the waves of a workgroup of the streamed form meet before every category (2) or never (0)?  The barrier keeps them on
 * the same category's matrix stream and op words, so that the 16 KB scalar cache holds what all of them read.  Where one
 * category is resident at a time -- one rate category, or a group per category: a phase of the launch has one -- they read
 * the same category whatever their drift, and if its matrix stream (nmat matrices and the spare one, 128 bytes each) and op
 * words (nwords dwords) fit the cache the barrier only costs: all twelve waves of the CU then start every unit together
 * and, as the code reads, wait together for its first chunks from device memory (timings and counters: DESIGN.md section 4) */
#define PLK_V4S_SCALAR_CACHE_BYTES (16 * 1024)
static inline int plk_v4s_auto_sync(int Cg, size_t nmat, size_t nwords)
{
    return Cg == 1 && (nmat + 1) * 128 + nwords * 4 <= (size_t)PLK_V4S_SCALAR_CACHE_BYTES ? 0 : 2;
}

struct PlkK4Shape {
    int nchar, C;
    long S;
    int num_cus;
    long pair_tables, fused_asm, sites_per_lane;     /* the option values as set */
    size_t static_lds[3];                            /* of k_ll_fused4_v4s<768>, k_ll_fused4_v4<768>, k_ll_fused4_v4<512> */
    const int *node_codes = nullptr;                 /* [N] occurring codes per node as bit masks (nchar <= 16), or none: no four-leaf tables */
};

struct PlkK4Choice {
    PlkK4Variant variant = PLK_K4_NONE;              /* PLK_K4_NONE: not fused, another kernel family takes the tree */
    int tile = 0;                                    /* sites per tile (v4s: per tile of the tile count it is handed) */
    int NS = 1, D = 4, pack4 = 0;                    /* sites per lane, register stack depth, two codes per staged byte */
    int block = 0;                                   /* lanes per workgroup */
    size_t lds = 0;                                  /* dynamic LDS of the launch */
    unsigned tip_base = 0;                           /* v4 / v4s: LDS address of the table image = static LDS of the kernel */
    int warm = 1, sync = 2;                          /* pair-table kernels: the measurement bits of PLK_OPT_PAIR_TABLES */
    bool sync_auto = false;                          /* v4s: no option bit forces sync; plk_k4_stream decides it (plk_v4s_auto_sync) on the formats that run */
    int fold = 1, held = 1;                          /* v4s, asked for: folded op stream, first chunks held across the categories */
    int pair = 0;                                    /* v4s: the pair-product form is asked for and the program is within its 3 slots */
    PlkV4TPlan triple;                               /* v4s: the plan of three-leaf / four-leaf tables and category groups (plk_v4t_plan; nodes + quads == 0: none) */
    std::string bad;                                 /* the replay check of the chosen variant's formats; empty: fine */
};

/*
 * Order of preference.  Pair tables (option on, assembly allowed, one site per lane asked, <= 4 stack slots, nchar <= 16,
 * something observed): the streamed form for modes 1 and 7 when every cherry as a table with the tables of all C categories
 * fits and allow_stream (the engine clears it when the stream itself cannot be allocated); then the candidates of the mode,
 * each with as many cherries as its LDS limit takes; forced modes 2, 3, 5, 6 have one candidate.  Then the assembly
 * interpreter, then the C++ interpreter, then PLK_K4_NONE.  Builds the formats of the chosen variant (fu | fpt, fv4, fv4s)
 * and replays them once (bad).
 * For the streamed form that is the kernel, the checked formats and the wishes (fold, held, pair, the table plan, the barrier's
 * option bits): what runs is plk_k4_stream's to say, from this choice and from what the engine could obtain.
 */
static inline PlkK4Choice plk_k4_choose(int N, const int *ip, const int *ix, const PlkProgram &pg, const PlkK4Shape &sh, bool allow_stream,
                                        PlkFused &fu, PlkFusedPT &fpt, PlkFusedV4 &fv4, PlkFusedV4S &fv4s)
{
    PlkK4Choice ch;
    const int nchar = sh.nchar;
    /* two sites per lane only in the C++ interpreter, and only within 8 stack slots; the assembly interpreter stages 4-bit
     * codes when there are at most 16 character definitions, which lets it take about twice the taxa of the C++ one */
    const int NS = sh.sites_per_lane == 2 && pg.slots_needed <= 8 ? 2 : 1, pack4 = nchar <= 16 ? 1 : 0;
    const size_t lds_asm = plk_fused_lds_bytes(pg, nchar, pack4 ? PLK_TILE / 2 : PLK_TILE), lds_cpp = plk_fused_lds_bytes(pg, nchar, PLK_TILE * NS);
    const bool asm_fits = NS == 1 && plk_fused_asm_ok(pg) && sh.fused_asm && lds_asm <= PLK_LDS_LIMIT;
    if (pg.slots_needed > PLK_FUSED_SLOTS || (!asm_fits && lds_cpp > PLK_LDS_LIMIT)) return ch;
    const PlkPairTablesOpt po = plk_pair_tables_opt(sh.pair_tables);
    ch.warm = po.warm; ch.sync = po.sync < 0 ? 2 : po.sync; ch.sync_auto = po.sync < 0; ch.fold = po.fold; ch.held = po.held;
    if (po.on && sh.fused_asm && sh.sites_per_lane != 2 && pg.slots_needed <= 4 && nchar <= 16 && !pg.obs_nodes.empty()) {
        if ((po.mode == 1 || po.mode == 7) && sh.S > 0 && allow_stream) {
            /* measured faster than the tile kernels at every shape tried (profiles/ll_k4_stream_ab.json), so no site count
             * sends the default back to them */
            plk_fused_pt_build(N, ip, ix, pg, nchar, INT_MAX, fpt, true);
            const size_t lds = plk_fused_v4s_lds_bytes(fpt, nchar, sh.C), st = sh.static_lds[PLK_K4_LDS_V4S_768];
            bool any_obs = false;
            for (const PlkFusedPT::VOp &o : fpt.vops) if (o.code == OP_TIP_SET || o.code == OP_TIP_MUL) any_obs = true;
            if (any_obs && lds + st <= plk_pt_lds_limit(1024) && (st + lds) / 32 < 65536 && fpt.units < 2048 && fpt.row_node.size() < 65536) {
                ch.variant = PLK_K4_V4S; ch.tile = 1536; ch.NS = 2; ch.block = 768; ch.lds = lds; ch.tip_base = (unsigned)st;
                ch.pair = po.pair && pg.slots_needed <= PLK_V4P_STACK_SLOTS;
                plk_fused_v4s_words(fpt, nchar, sh.C, ch.tip_base, fv4s);
                /* the 32-bit program is replayed whatever the form (streamed: no code rows in LDS; its fields are the chain the
                 * streamed words are checked against) */
                ch.bad = plk_fused_check_pt(N, ip, ix, pg, fpt, nchar, 1, 0, true, false);
                if (ch.bad.empty()) ch.bad = plk_fused_check_v4s(fpt, fv4s, nchar, sh.C, ch.tip_base, lds);
                /* three-leaf tables: which nodes and how many groups (the phases exist in the pair-product instantiation only);
                 * the formats themselves are derived from fpt and replayed like the fold and the pair products */
                if (ch.bad.empty())
                    ch.triple = plk_v4t_plan(fpt, nchar, sh.C, sh.S, sh.num_cus, st, po.triple, ch.pair && ch.fold && ch.held ? po.groups : 1, po.quad, sh.node_codes);
                return ch;
            }
        }
        struct Cand { PlkK4Variant variant; int tile; };
        std::vector<Cand> cands;
        switch (po.mode) {
        case 2: cands = {{PLK_K4_ASM_PT, 1024}}; break;
        case 3: cands = {{PLK_K4_ASM_PT, 512}}; break;
        case 5: cands = {{PLK_K4_V4, 1024}}; break;
        case 6: cands = {{PLK_K4_V4, 1536}}; break;
        default: {
            /* 1536-site tiles run 1.3 x as long as 1024-site tiles (109 against 84 us a round at BASELINE config 3) and carry 1.5 x
             * the sites; every CU runs ceil(tiles / CUs) rounds.  Few sites per GPU (a rank of an 8-way split) can need fewer
             * round-times with the smaller tile: 1.25M sites are 4 rounds of 1536 (436 us) or 5 rounds of 1024 (420 us). */
            auto rounds = [&](long tile) { const long nt = (sh.S + tile - 1) / tile; return (double)((nt + sh.num_cus - 1) / sh.num_cus); };
            if (sh.S > 0 && rounds(1024) * 1.0 < rounds(1536) * 1.3) cands = {{PLK_K4_V4, 1024}, {PLK_K4_V4, 1536}, {PLK_K4_ASM_PT, 1024}, {PLK_K4_ASM_PT, 512}};
            else cands = {{PLK_K4_V4, 1536}, {PLK_K4_V4, 1024}, {PLK_K4_ASM_PT, 1024}, {PLK_K4_ASM_PT, 512}};
            break;
        }
        }
        for (const Cand &cd : cands) {
            const bool v4 = cd.variant == PLK_K4_V4;
            const long limit = (long)plk_pt_lds_limit(cd.tile);
            int max_pairs = INT_MAX;
            for (int attempt = 0; attempt < 3; attempt++) {
                plk_fused_pt_build(N, ip, ix, pg, nchar, max_pairs, fpt, v4);
                const long bytes = (long)plk_fused_pt_lds_bytes(fpt, nchar, cd.tile);
                if (bytes <= limit && fpt.units < 2048 && fpt.row_node.size() < 65536) {
                    /* v4: two sites per lane, one workgroup of tile / 2 lanes per CU; asm_pt: one site per lane */
                    ch.variant = cd.variant; ch.tile = cd.tile; ch.NS = v4 ? 2 : 1; ch.block = v4 ? cd.tile / 2 : cd.tile; ch.lds = (size_t)bytes;
                    ch.bad = plk_fused_check_pt(N, ip, ix, pg, fpt, nchar, cd.tile, ch.lds, v4);
                    if (v4) {
                        ch.tip_base = (unsigned)sh.static_lds[cd.tile == 1536 ? PLK_K4_LDS_V4_768 : PLK_K4_LDS_V4_512];
                        plk_fused_v4_words(fpt, nchar, cd.tile, ch.tip_base, fv4);
                        if (ch.bad.empty()) ch.bad = plk_fused_check_v4(fpt, fv4, nchar, cd.tile, ch.tip_base, ch.lds);
                    }
                    return ch;
                }
                if (fpt.npairs == 0) break;
                /* a cherry as a table costs nchar - 2 more units and one row less than its two leaves */
                const long per_pair = (long)(nchar - 2) * nchar * 32 - cd.tile;
                if (per_pair <= 0) break;                       /* tables only shrink the image: nothing to give back */
                const long drop = (bytes - limit + per_pair - 1) / per_pair;
                max_pairs = drop >= fpt.npairs ? 0 : fpt.npairs - (int)drop;
            }
        }
    }
    plk_fused_build(N, pg, fu);
    ch.tile = PLK_TILE * NS; ch.NS = NS; ch.block = PLK_TILE;
    ch.D = pg.slots_needed <= 4 ? 4 : (pg.slots_needed <= 8 ? 8 : 16);
    if (asm_fits) {
        ch.variant = PLK_K4_ASM; ch.pack4 = pack4; ch.lds = lds_asm;
        ch.bad = plk_fused_check_asm(N, pg, fu, nchar, ch.D, pack4, lds_asm);
    } else {
        ch.variant = PLK_K4_CPP; ch.lds = lds_cpp;
        ch.bad = plk_fused_check_cpp(N, pg, fu, nchar, ch.D, NS, lds_cpp);
    }
    return ch;
}

/*
 * The formats the streamed form runs, derived from the checked ones of a PLK_K4_V4S choice by one host-only sequence, for the
 * engine and for the CPU tests alike; what the engine could obtain from the runtime comes in as PlkK4StreamCaps.
 *   1. tables (ch.triple): the groups are taken back (plk_v4t_plan with one group) where the instantiation with phases cannot run
 *      or the partial sums have no room; the rewritten format and its words are built and replayed against the checked ones, at
 *      most twice (a rewritten stream the pair-product form does not take is planned again with one group);
 *   2. the folded stream, 3. the pair-product stream (with the fold, the held chunks and the capability): if derived and replayed;
 *   4. the barrier, where no option bit forces it: plk_v4s_auto_sync on what runs.
 * A form that does not replay is not run: the one before it is, and `note` says why (the last reason stays).
 */
/* k_ll_fused4_v4s<768, true>, <768, true, true> and <768, true, true, true> can run; there is room for the partial sums of the phases */
struct PlkK4StreamCaps { bool held = true, pair = true, groups = true, partial_sums = true; };

struct PlkK4Stream {
    PlkFusedV4S fv4s;                               /* the stream that runs (of the rewritten format where tables were taken) ... */
    PlkFusedV4SFold fold; PlkFusedV4P pair;         /* ... its folded form and its pair-product form, where derived */
    enum Words { CHECKED, FOLDED, PAIR } runs = CHECKED;      /* the op words uploaded: fv4s.words, fold.words or pair.words */
    bool held = false;                              /* the first chunks are held across the categories */
    PlkV4TPlan triple;                              /* the tables taken (nodes + quads == 0: none) and their category groups */
    size_t lds = 0;                                 /* dynamic LDS of the launch */
    int sync = 2; bool sync_auto = false;           /* the barrier as launched; no option bit forced it */
    long info_fold = 0, info_pairmul = 0, info_triple = 0, info_quad = 0;     /* PLK_INFO_LL_FOLD, _PAIRMUL, _TRIPLE, _QUAD */
    std::string note;                               /* why a derived form does not run ("internal: ..."), or empty */
    const std::vector<unsigned> &words() const { return runs == PAIR ? pair.words : runs == FOLDED ? fold.words : fv4s.words; }
    size_t stride() const { return runs == PAIR ? pair.stride : runs == FOLDED ? fold.stride : fv4s.stride; }
    int Cg(int C) const { return triple.nodes + triple.quads > 0 && triple.Cg > 0 ? triple.Cg : C; }     /* categories resident at a time */
};

/* What the interpreter statement of the streamed kernel takes per category and per launch, one record per category in device
 * memory: the prologue loads the first half with one scalar load and the epilogue the root weights with another (the offsets are
 * named in tools/gen_fused4_v4.py), so that the statement's scalar operands are this record's address and the code stream.
 * Written where the formats are uploaded; a model change makes the formats stale, so the weights follow it. */
struct PlkV4SRecord {
    unsigned long long ops, mstream;   /* device addresses of the category's op words and of its matrix stream */
    unsigned first_y, first_y1, first_b1, pad;     /* LDS offset / 32 of the first and of the second observation's table in the
                                                      category's resident image, bit offset of the second observation's code */
    double w[4];                       /* root weights: 1 without a prior, 1/4 for the uniform one */
};
static_assert(sizeof(PlkV4SRecord) == 64 && offsetof(PlkV4SRecord, first_y) == 16 && offsetof(PlkV4SRecord, w) == 32, "the assembly text names these offsets");

/* words, ps: device addresses of the uploaded op words (C streams of r.stride() dwords) and of the matrix streams (C x (nmat + 1)
 * matrices); cat32: rows of a category's table image (table units x nchar); in phases category c reads the image of c % Cg */
static inline std::vector<PlkV4SRecord> plk_v4s_records(const PlkK4Stream &r, int C, unsigned cat32, unsigned long long words, unsigned long long ps,
                                                       size_t nmat, const double *root_w)
{
    std::vector<PlkV4SRecord> out((size_t)C);
    const bool pairmul = r.runs == PlkK4Stream::PAIR;
    const int cg = r.triple.groups > 1 && r.triple.Cg > 0 ? r.triple.Cg : C;     /* as the launch: phases only with more than one group */
    for (int c = 0; c < C; c++) {
        PlkV4SRecord &q = out[c];
        q.ops = words + (unsigned long long)c * r.stride() * sizeof(unsigned);
        q.mstream = ps + (unsigned long long)c * (nmat + 1) * 16 * sizeof(double);
        const unsigned image = (unsigned)(c % cg) * cat32;
        q.first_y = r.fv4s.first_y[0] + image;
        q.first_y1 = pairmul ? r.pair.first_y1[0] + image : 0u;
        q.first_b1 = pairmul ? r.pair.first_b1 : 0u;
        q.pad = 0;
        for (int i = 0; i < 4; i++) q.w[i] = root_w[i];
    }
    return out;
}

/* more than one group: only in the pair-product instantiation, with the fold and the held chunks (the engine reserves the partial sums only then) */
static inline bool plk_k4_stream_can_group(const PlkK4Choice &ch, const PlkK4StreamCaps &caps) { return ch.pair && ch.fold && ch.held && caps.held && caps.pair && caps.groups; }

/* steps 2 and 3 on r.fv4s; pair_kept: r.pair is already that stream's pair-product form, replayed */
static inline void plk_k4_stream_fold_pair(PlkK4Stream &r, bool fold, bool pair, bool pair_kept = false)
{
    r.runs = PlkK4Stream::CHECKED; r.info_fold = r.held ? 2 : 0; r.info_pairmul = 0;
    if (fold) {
        plk_fused_v4s_fold(r.fv4s, r.fold);
        const std::string bad = plk_fused_check_v4s_fold(r.fv4s, r.fold);
        if (bad.empty()) {
            r.runs = PlkK4Stream::FOLDED;
            r.info_fold |= 1 | (long)(r.fold.scale_slots & 15) << 4 | (long)std::min(r.fold.standalone_scale, 255) << 8 |
                           (long)std::min(r.fold.nadv[0], 255) << 16 | (long)std::min(r.fold.nadv[1], 127) << 24;
        } else r.note = "internal: " + bad + " (the unfolded op stream runs)";
    }
    if (!pair || r.runs != PlkK4Stream::FOLDED || !r.held) return;
    /* where the form does not apply (a table field beyond its 13 bits, an observation kind without a handler on its buffer)
     * nothing is derived and the folded stream runs */
    if (!pair_kept) plk_fused_v4p_build(r.fv4s, r.pair);
    if (r.pair.words.empty()) return;
    const std::string bad = pair_kept ? "" : plk_fused_check_v4p(r.fv4s, r.pair);
    if (bad.empty()) { r.runs = PlkK4Stream::PAIR; r.info_pairmul = 1 | (long)std::min(r.pair.npair, 65535) << 8; }
    else r.note = "internal: " + bad + " (the folded op stream runs)";
}

/* ch: a PLK_K4_V4S choice with empty bad, of this tree, program and shape; fpt, fv4s: its checked formats.  fpt becomes the
 * pair-table format that runs (the engine's three kernel families share that member), the rest is returned */
static inline PlkK4Stream plk_k4_stream(int N, const int *ip, const int *ix, const PlkProgram &pg, const PlkK4Shape &sh, const PlkK4Choice &ch,
                                        const PlkK4StreamCaps &caps, PlkFusedPT &fpt, PlkFusedV4S fv4s)
{
    PlkK4Stream r;
    r.fv4s = std::move(fv4s); r.held = ch.held && caps.held; r.lds = ch.lds; r.sync = ch.sync; r.sync_auto = ch.sync_auto;
    const PlkPairTablesOpt po = plk_pair_tables_opt(sh.pair_tables);
    PlkV4TPlan tp = ch.triple;
    auto one_group = [&]() { return plk_v4t_plan(fpt, sh.nchar, sh.C, sh.S, sh.num_cus, ch.tip_base, po.triple, 1, po.quad, sh.node_codes); };
    if (tp.groups > 1 && !plk_k4_stream_can_group(ch, caps)) tp = one_group();
    if (tp.nodes + tp.quads > 0 && tp.groups > 1 && !caps.partial_sums) tp = one_group();
    bool pair_kept = false;
    for (int attempt = 0; attempt < 2 && tp.nodes + tp.quads > 0; attempt++) {
        PlkFusedPT fpt_t; PlkFusedV4S fv4s_t;        /* the rewritten formats while they are derived and checked */
        std::string bad;
        if (tp.quads > 0) {
            /* four-leaf tables and the three-leaf tables beside them, from the plan's lists */
            plk_fused_v4q_build(fpt, pg.slots_needed, sh.nchar, sh.node_codes, tp.tri_at, tp.quad_at, tp.quad_shape, true, fpt_t);
            bad = plk_fused_check_v4q(N, ip, ix, fpt, fpt_t, sh.nchar, sh.node_codes);
            if (bad.empty() && fpt_t.nquads != tp.quads) bad = "v4q program: the builder took another number of four-leaf nodes than the plan";
        } else {
            plk_fused_v4t_build(fpt, pg.slots_needed, sh.nchar, tp.extra_bytes, true, fpt_t);
            bad = plk_fused_check_v4t(N, ip, ix, fpt, fpt_t, sh.nchar);
        }
        const size_t lds = plk_fused_v4s_lds_bytes(fpt_t, sh.nchar, tp.Cg);
        if (bad.empty() && fpt_t.ntriples != tp.nodes) bad = "v4t program: the builder took another number of nodes than the plan";
        if (bad.empty()) {
            plk_fused_v4s_words(fpt_t, sh.nchar, sh.C, ch.tip_base, fv4s_t, tp.Cg);
            bad = plk_fused_check_v4s(fpt_t, fv4s_t, sh.nchar, sh.C, ch.tip_base, lds);
        }
        /* fewer observations: the stream fits the room reserved for the checked one */
        if (bad.empty() && fv4s_t.chunks > r.fv4s.chunks) bad = "v4t program: more chunks than the checked stream";
        if (bad.empty() && tp.groups > 1) {
            /* the phases exist in the pair-product instantiation only: a rewritten stream that form does not take runs in one group */
            plk_fused_v4p_build(fv4s_t, r.pair);
            if (r.pair.words.empty() || !plk_fused_check_v4p(fv4s_t, r.pair).empty()) { tp = one_group(); continue; }
            pair_kept = true;
        }
        if (bad.empty()) {
            fpt = std::move(fpt_t); r.fv4s = std::move(fv4s_t); r.lds = lds; r.triple = tp;
            r.info_triple = 1 | (long)std::min(tp.groups, 15) << 4 | (long)std::min(tp.nodes, 65535) << 8;
            r.info_quad = tp.quads > 0 ? 1 | (long)std::min(tp.quads, 65535) << 8 : 0;
        } else r.note = "internal: " + bad + (tp.quads > 0 ? " (the stream without four-leaf and three-leaf tables runs)" : " (the stream without three-leaf tables runs)");
        break;
    }
    plk_k4_stream_fold_pair(r, ch.fold != 0, ch.pair && caps.pair, pair_kept);
    if (r.sync_auto) r.sync = plk_v4s_auto_sync(r.Cg(sh.C), fpt.mat_edge.size(), r.stride());
    return r;
}

/* ------------------------------------------------------------------------------------------------------------ */
/* what the down / up drivers share: dense storage indices of the stored vectors, and the site-chunk plan         */
/* ------------------------------------------------------------------------------------------------------------ */

/*
 * Where the down / up passes keep what they store per site: a leaf edge has a tip slot and no vector, an internal edge a
 * dense index into the edge vectors, a node with children a dense index into the node vectors, and a rescaled such node a
 * dense index into the stored factors.  Everything else is -1.  All indices grow with the edge / node number.
 */
struct PlkStorageMaps {
    std::vector<int> edge_tip;         /* E: tip slot of a leaf edge */
    std::vector<int> edge_int;         /* E: storage index of an internal edge */
    std::vector<int> node_int;         /* N: storage index of a node with children */
    std::vector<int> node_scale;       /* N: rescaling slot of a stored node the program rescales */
    std::vector<int> tip_edges;        /* ntips + 1: CSR edge per tip slot, then -1 for the pseudo slot (raw definitions) */
    int ntips = 0, nie = 0, nin = 0, nsc = 0;
};

/* (run_updown4 used to give a tree without any node with children a root vector.  Every driver is reached with E > 0 only,
 * where the root has a child, so that rule never fired and is not kept.) */
static inline void plk_storage_maps_build(int N, int E, const int *indptr, const std::vector<int> &tip_edge, const char *scale_node,
                                          PlkStorageMaps &m)
{
    m.ntips = (int)tip_edge.size();
    m.edge_tip.assign(E, -1); m.edge_int.assign(E, -1); m.node_int.assign(N, -1); m.node_scale.assign(N, -1);
    m.nie = m.nin = m.nsc = 0;
    for (int t = 0; t < m.ntips; t++) m.edge_tip[tip_edge[t]] = t;
    for (int e = 0; e < E; e++) if (m.edge_tip[e] < 0) m.edge_int[e] = m.nie++;
    for (int a = 0; a < N; a++) if (indptr[a + 1] > indptr[a]) m.node_int[a] = m.nin++;
    for (int a = 0; a < N; a++) if (m.node_int[a] >= 0 && scale_node[a]) m.node_scale[a] = m.nsc++;
    m.tip_edges = tip_edge;
    m.tip_edges.push_back(-1);
}

/*
 * Sites per pass of a down / up driver whose workspace takes bytes_per_site: what fits the free device memory (all but
 * 4 GiB of it, or half of it at 6 GiB and below) plus the workspace the engine already holds, capped by S and by
 * opt_site_chunk (> 0).  A chunk shorter than S is a whole number of tiles, at least one.  whole_tiles (the matrix-core
 * kernels, whose grids cover whole tiles): S counts rounded up to the tile and the chunk is always rounded down to whole
 * tiles.  Returns 0 when not even one site (whole_tiles: one tile) fits.
 */
static inline long plk_site_chunk(long S, size_t free_bytes, size_t retained_work_bytes, size_t bytes_per_site, long opt_site_chunk,
                                  int tile, bool whole_tiles)
{
    size_t budget = free_bytes > (size_t)(6ull << 30) ? free_bytes - (size_t)(4ull << 30) : free_bytes / 2;
    budget += retained_work_bytes;
    const size_t all = whole_tiles ? (size_t)((S + tile - 1) / tile * tile) : (size_t)S;
    long chunk = (long)std::min<size_t>(all, budget / bytes_per_site);
    if (opt_site_chunk > 0) chunk = std::min<long>(chunk, opt_site_chunk);
    if (whole_tiles) return chunk / tile * tile;
    if (chunk < 1) return 0;
    if (chunk < S) chunk = std::max<long>(tile, chunk / tile * tile);
    return chunk;
}

/* ------------------------------------------------------------------------------------------------------------ */
/* down passes that traverse the program (k_down_fused4, k_ll_mfma, k_down_fused_mfma): int4 ops with an          */
/* observation chain (z = tip slot of the next observation op, w = its staged row; the last one wraps with bit 30) */
/* ------------------------------------------------------------------------------------------------------------ */

struct PlkChain {
    std::vector<plk_op4> ops;          /* + one trailing OP_END (k_down_fused4 reads one op ahead) */
    int first_slot = -1, first_row = 0;
    int second_row = 0;                /* mode 3: staged row of the second observation op */
};

/* mode 3 (k_ll_vec, k_down_vec): as mode 1, and every observation op also carries in y the staged row of the observation
 * op AFTER the next one (the prefetch chain runs two ops ahead: value of the next op, code of the one after; the
 * sequence wraps to the start for the next category); MATVEC w = CSR edge of the next MATVEC.
 * mode 0: MATVEC keeps (x, y) of the program, z = op index of the next MATVEC, wrapping (k_ll_mfma); mode 1: MATVEC y = CSR edge, z = storage index of the
 * child node, w = CSR edge of the next MATVEC, wrapping to the first (k_down_fused4, k_down_vec); mode 2: as 1 but
 * w = storage index of the edge (k_down_fused_mfma, no chain).  SCALE y = rescaling slot of the node or -1 (modes 1, 2). */
static inline void plk_chain_build(int N, const PlkProgram &pg, int mode, const int *indices, const int *node_int,
                                   const int *edge_int, const int *node_scale, PlkChain &ch, const char *skip_store = nullptr)
{
    const int ntips = (int)pg.tip_edge.size();
    std::vector<int> row(N, -1);
    for (size_t r = 0; r < pg.obs_nodes.size(); r++) row[pg.obs_nodes[r]] = (int)r;
    ch.ops.assign(pg.ops.size() + 1, plk_op4{OP_END, 0, 0, 0});
    ch.first_slot = -1; ch.first_row = 0;
    int prev = -1;
    for (size_t pc = 0; pc < pg.ops.size(); pc++) {
        const int code = pg.ops[pc].x & 0xff;
        plk_op4 o = {pg.ops[pc].x, pg.ops[pc].y, 0, 0};
        if (code == OP_TIP_SET || code == OP_TIP_MUL || code == OP_NODE_MUL) {
            const int slot = code == OP_NODE_MUL ? ntips : (o.x >> 8);
            o.y = row[pg.ops[pc].y];
            if (mode != 2) {
                if (prev < 0) { ch.first_slot = slot; ch.first_row = o.y; }
                else { ch.ops[prev].z = slot; ch.ops[prev].w = o.y; }
                prev = (int)pc;
            }
        } else if (code == OP_MATVEC && mode >= 1) {
            o.y = pg.op_edge[pc];
            o.z = node_int ? node_int[indices[o.y]] : 0;
            if (mode >= 1 && skip_store && skip_store[indices[o.y]]) o.z = -1;      /* this child's vector is not stored */
            if (mode == 2) o.w = edge_int[o.y];
        } else if (code == OP_SCALE && mode >= 1 && node_scale) {
            /* one stored factor per node: the OP_SCALE inside a node is not taken (y = -1), the one after its last child is */
            o.y = pc < pg.op_mid.size() && pg.op_mid[pc] ? -1 : node_scale[pg.ops[pc].y];
        }
        ch.ops[pc] = o;
    }
    if (prev >= 0) { ch.ops[prev].z = ch.first_slot | (1 << 30); ch.ops[prev].w = ch.first_row; }
    if (mode == 3) {
        /* y of an observation op = staged row of the op two observations later (cyclically) */
        std::vector<int> opc_, rows_;
        for (size_t pc = 0; pc < pg.ops.size(); pc++) {
            const int code = pg.ops[pc].x & 0xff;
            if (code == OP_TIP_SET || code == OP_TIP_MUL || code == OP_NODE_MUL) { opc_.push_back((int)pc); rows_.push_back(ch.ops[pc].y); }
        }
        const size_t no = opc_.size();
        ch.second_row = no ? rows_[1 % no] : 0;
        for (size_t i = 0; i < no; i++) ch.ops[opc_[i]].y = rows_[(i + 2) % no];
    }
    if (mode == 0) {
        /* MATVEC z = op index of the next MATVEC, wrapping to the first (k_ll_mfma requests its matrix fragments early) */
        int first_mv = -1, prev_mv = -1;
        for (size_t pc = 0; pc < pg.ops.size(); pc++)
            if ((pg.ops[pc].x & 0xff) == OP_MATVEC) {
                if (first_mv < 0) first_mv = (int)pc;
                if (prev_mv >= 0) ch.ops[prev_mv].z = (int)pc;
                prev_mv = (int)pc;
            }
        if (prev_mv >= 0) ch.ops[prev_mv].z = first_mv;
    }
    if (mode == 1 || mode == 3) {
        /* MATVEC w = CSR edge of the next MATVEC (wrapping); without node storage (ll kernels) z = its op index */
        int first_mv = -1, prev_mv = -1;
        for (size_t pc = 0; pc < pg.ops.size(); pc++)
            if ((pg.ops[pc].x & 0xff) == OP_MATVEC) {
                if (first_mv < 0) first_mv = (int)pc;
                if (prev_mv >= 0) { ch.ops[prev_mv].w = pg.op_edge[pc]; if (!node_int) ch.ops[prev_mv].z = (int)pc; }
                prev_mv = (int)pc;
            }
        if (prev_mv >= 0) { ch.ops[prev_mv].w = pg.op_edge[first_mv]; if (!node_int) ch.ops[prev_mv].z = first_mv; }
    }
}

/*
 * Up pass of the vector kernels (k_up_vec, plk_updown_vec.h): visit records of the internal nodes in BFS order and
 * the list of matrices in the exact order the kernel consumes them (kind 0: P for a child message, 1: the edge-form
 * matrix, 2: P for the forward vector of a child).  The builder and the kernel are the two halves of one contract;
 * plk_up_visits_check() replays the kernel's consumption against the list.
 *   header (8 ints): node, number of children, storage index of the node, rescaling slot or -1, has_data,
 *                    first CSR edge, marginal of the root wanted (first record only), 0
 *   child (4 ints):  node, tip slot or -1, PLK_UP_* flags, storage index (internal child) or -1
 * An internal child whose own children (one or two) are all leaves is handled INSIDE this visit when no marginals are
 * asked for (PLK_UP_INLINE): its forward vector is used while it is in registers and never stored, the node gets no
 * visit of its own, and the child's fourth int is the offset (in rec) of a 12-int record placed after all visits:
 *   node, has_data, rescaling slot or -1, number of leaves (1 or 2), first CSR edge,
 *   leaf 0: node, tip slot, wanted (bit 0 derivative, bit 1 marginal);  leaf 1: node, tip slot, wanted;  0
 * With marginals a child is inlined only if all its leaves observe single states at every site (leaf_observed).
 */
enum { PLK_UP_WANT_D = 1, PLK_UP_WANT_F = 2, PLK_UP_WANT_M = 4, PLK_UP_STORE_F = 8, PLK_UP_INLINE = 16 };

/* a node whose one or two children are all leaves is finished inside its parent's visit when no marginals are asked for:
 * its forward vector is never stored, and neither is its L vector (the up pass rebuilds it from the tip tables) */
static inline bool plk_up_inlinable(const int *ip, const int *edge_tip, int b, bool marg, const int *ix = nullptr,
                                    const char *leaf_observed = nullptr)
{
    const int d = ip[b + 1] - ip[b];
    if (d < 1 || d > 2) return false;
    /* with marginals: only when every site of every leaf below observes a single state (leaf_observed, from the pattern
     * upload) -- the leaf's marginal is then one dot product per site, done in the parent's parent's visit too */
    if (marg && (!ix || !leaf_observed)) return false;
    for (int idx = ip[b]; idx < ip[b + 1]; idx++) {
        if (edge_tip[idx] < 0) return false;
        if (marg && !leaf_observed[ix[idx]]) return false;
    }
    return true;
}

struct PlkUpVisits {
    std::vector<int> rec;              /* visit records, then the inline records */
    size_t visit_ints = 0;             /* ints of rec taken by the visit records */
    int nvisits = 0;
    std::vector<int> kind, edge;       /* the matrix stream */
};

static inline void plk_up_visits_build(int N, const int *ip, const int *ix, const int *preorder, const char *node_has_data,
                                       const int *edge_tip, const int *node_int, const int *node_scale, bool deriv, bool marg,
                                       const int *edge_mask, const int *node_mask, PlkUpVisits &uv, const char *leaf_observed = nullptr)
{
    uv.rec.clear(); uv.kind.clear(); uv.edge.clear(); uv.nvisits = 0;
    auto flags = [&](int idx, int b) {
        const bool leaf = edge_tip[idx] >= 0;
        const bool wd = deriv && (!edge_mask || edge_mask[idx]);
        const bool wm = marg && (!node_mask || node_mask[b]);
        const bool wf = !leaf || wm;
        return (wd ? PLK_UP_WANT_D : 0) | (wf ? PLK_UP_WANT_F : 0) | (wm ? PLK_UP_WANT_M : 0) | (!leaf ? PLK_UP_STORE_F : 0);
    };
    auto put = [&](int kind, int edge) { uv.kind.push_back(kind); uv.edge.push_back(edge); };
    auto inlinable = [&](int b) { return plk_up_inlinable(ip, edge_tip, b, marg, ix, leaf_observed); };
    std::vector<int> inl;                /* inline records, appended after the visits */
    std::vector<size_t> fix;             /* positions in rec that hold an offset into inl */
    for (int u = 0; u < N; u++) {
        const int a = preorder[u];
        const int start = ip[a], deg = ip[a + 1] - start;
        if (deg == 0) continue;
        if (u > 0 && inlinable(a)) continue;             /* handled inside its parent's visit */
        const int root_m = u == 0 && marg && (!node_mask || node_mask[a]);
        const int hdr[8] = {a, deg, node_int[a], node_scale[a], node_has_data[a] ? 1 : 0, start, root_m, 0};
        uv.rec.insert(uv.rec.end(), hdr, hdr + 8);
        for (int j = 0; j < deg; j++) {
            const int idx = start + j, b = ix[idx];
            int fl = flags(idx, b), second = edge_tip[idx];
            const int fourth = edge_tip[idx] >= 0 ? -1 : node_int[b];
            if (edge_tip[idx] < 0 && inlinable(b)) {
                fl = (fl & ~PLK_UP_STORE_F) | PLK_UP_INLINE | PLK_UP_WANT_F;
                const int s0 = ip[b], db = ip[b + 1] - s0;
                int r[12] = {b, node_has_data[b] ? 1 : 0, node_scale[b], db, s0, 0, 0, 0, 0, 0, 0, 0};
                for (int q = 0; q < db; q++) {
                    r[5 + 3 * q] = ix[s0 + q];
                    r[6 + 3 * q] = edge_tip[s0 + q];
                    r[7 + 3 * q] = (deriv && (!edge_mask || edge_mask[s0 + q]) ? 1 : 0) | (marg && (!node_mask || node_mask[ix[s0 + q]]) ? 2 : 0);
                }
                second = (int)inl.size();            /* becomes -2 - (visit_ints + offset) below */
                fix.push_back(uv.rec.size() + 1);
                inl.insert(inl.end(), r, r + 12);
            }
            const int cr[4] = {b, second, fl, fourth};
            uv.rec.insert(uv.rec.end(), cr, cr + 4);
        }
        uv.nvisits++;
        for (int j = 0; j < deg; j++) {
            const int idx = start + j, fl = flags(idx, ix[idx]) | (edge_tip[idx] < 0 && inlinable(ix[idx]) ? PLK_UP_WANT_F : 0);
            if (!(fl & (PLK_UP_WANT_D | PLK_UP_WANT_F))) continue;
            for (int j2 = 0; j2 < deg; j2++)
                if (j2 != j && edge_tip[start + j2] < 0) put(0, start + j2);
            if ((fl & PLK_UP_WANT_D) && edge_tip[idx] < 0) put(1, idx);
            if (fl & PLK_UP_WANT_F) put(2, idx);
        }
    }
    uv.visit_ints = uv.rec.size();
    for (size_t f : fix) uv.rec[f] = -2 - (uv.rec[f] + (int)uv.visit_ints);
    uv.rec.insert(uv.rec.end(), inl.begin(), inl.end());
}

/* replays k_up_vec's walk over the records: every index in range, every stored forward vector written before it is
 * read, and the matrices consumed are exactly the list, in order */
static inline std::string plk_up_visits_check(int N, int E, const PlkUpVisits &uv, int nint_nodes, int ntips, int nscale_slots,
                                              bool deriv)
{
    std::vector<char> f_written(std::max(nint_nodes, 1), 0), visited(N, 0), inlined(N, 0);
    size_t vp = 0, ms = 0;
    for (int v = 0; v < uv.nvisits; v++) {
        if (vp + 8 > uv.rec.size()) return "up visits: record overrun";
        const int *h = &uv.rec[vp];
        const int a = h[0], deg = h[1], ai = h[2], slot = h[3], e0 = h[5];
        if (a < 0 || a >= N || deg < 1 || ai < 0 || ai >= nint_nodes || slot < -1 || slot >= nscale_slots) return plk_fmt("up visits: bad header %ld", v);
        if (e0 < 0 || e0 + deg > E) return plk_fmt("up visits: bad edge range in visit %ld", v);
        if (vp + 8 + 4 * (size_t)deg > uv.rec.size()) return "up visits: record overrun";
        if (v == 0) f_written[ai] = 1;       /* the root's forward vector is written first */
        if (!f_written[ai]) return plk_fmt("up visits: forward vector of node %ld read before it is written", a);
        visited[a] = 1;
        const int *ch = h + 8;
        auto need = [&](int kind, int edge) -> bool { const bool ok = ms < uv.kind.size() && uv.kind[ms] == kind && uv.edge[ms] == edge; ms++; return ok; };
        for (int j = 0; j < deg; j++) {
            const int b = ch[4 * j], t = ch[4 * j + 1], fl = ch[4 * j + 2], bi = ch[4 * j + 3];
            if (b < 0 || b >= N || t >= ntips || ((t < -1) != ((fl & PLK_UP_INLINE) != 0))) return plk_fmt("up visits: bad child in visit %ld", v);
            if (t < 0 && (bi < 0 || bi >= nint_nodes)) return plk_fmt("up visits: bad storage index in visit %ld", v);
            if (fl & PLK_UP_INLINE) {
                /* the child's leaves are handled here: its record must lie behind the visits and be in range */
                const long off = -2 - (long)t;
                if ((fl & PLK_UP_STORE_F) || !(fl & PLK_UP_WANT_F)) return plk_fmt("up visits: flags of an inline child in visit %ld", v);
                if (off < (long)uv.visit_ints || (size_t)off + 12 > uv.rec.size()) return plk_fmt("up visits: inline record out of range in visit %ld", v);
                const int *q = &uv.rec[off];
                if (q[0] != b || q[2] < -1 || q[2] >= nscale_slots || q[3] < 1 || q[3] > 2 || q[4] < 0 || q[4] + q[3] > E) return plk_fmt("up visits: bad inline record in visit %ld", v);
                for (int l = 0; l < q[3]; l++)
                    if (q[5 + 3 * l] < 0 || q[5 + 3 * l] >= N || q[6 + 3 * l] < 0 || q[6 + 3 * l] >= ntips) return plk_fmt("up visits: bad inline leaf in visit %ld", v);
                inlined[b] = 1;
                continue;
            }
            if (((fl & PLK_UP_STORE_F) != 0) != (t < 0) || (t < 0 && !(fl & PLK_UP_WANT_F))) return plk_fmt("up visits: flags of an internal child in visit %ld", v);
            if (!deriv && (fl & PLK_UP_WANT_D)) return "up visits: derivative flag without a derivative pass";
        }
        for (int j = 0; j < deg; j++) {
            const int fl = ch[4 * j + 2];
            if (!(fl & (PLK_UP_WANT_D | PLK_UP_WANT_F))) continue;
            for (int j2 = 0; j2 < deg; j2++)
                if (j2 != j && ch[4 * j2 + 1] < 0 && !need(0, e0 + j2)) return plk_fmt("up visits: stream mismatch (sibling) in visit %ld", v);
            if ((fl & PLK_UP_WANT_D) && ch[4 * j + 1] < 0 && !need(1, e0 + j)) return plk_fmt("up visits: stream mismatch (edge form) in visit %ld", v);
            if ((fl & PLK_UP_WANT_F) && !need(2, e0 + j)) return plk_fmt("up visits: stream mismatch (forward) in visit %ld", v);
        }
        for (int j = 0; j < deg; j++) if (ch[4 * j + 2] & PLK_UP_STORE_F) f_written[ch[4 * j + 3]] = 1;
        vp += 8 + 4 * (size_t)deg;
    }
    if (vp != uv.visit_ints) return "up visits: trailing records";
    for (int a = 0; a < N; a++) if (visited[a] && inlined[a]) return plk_fmt("up visits: node %ld is both visited and inlined", a);
    if (ms != uv.kind.size()) return "up visits: matrix stream not consumed";
    for (size_t i = 0; i < uv.edge.size(); i++) if (uv.edge[i] < 0 || uv.edge[i] >= E || uv.kind[i] < 0 || uv.kind[i] > 2) return "up visits: bad stream entry";
    return "";
}

/*
 * Node visits of k_up_nodes_mfma (plk_mfma_updown.h): the derivative pass without marginals.  One visit per internal
 * node a; what is stored per internal node is the vector G_a at the TOP of the edge into a (forward vector of the
 * parent with the parent's observation, rescaling factor and the sibling messages folded in), not the forward vector
 * at a.  A visit finishes the derivative of a's own edge from G_a and the child messages (stored edge vectors / tip
 * tables; L_a is not read), forms F_a = P_a^T G_a and the G_b of every child.  Visits are in depth-first order; the G
 * of the last internal child that still has work below it is not stored but handed to the next visit in registers
 * (PLK_UN_CONTINUE on the child -- always the LAST child record -- and PLK_UN_FROM_REGS on the next header).
 *   header (8 ints): node, number of children, storage index, rescaling slot or -1, has_data, first CSR edge,
 *                    CSR edge into the node (-1: root, whose visit is the first and takes the root prior from
 *                    registers), PLK_UN_* header flags
 *   child (4 ints):  node, tip slot or -1, PLK_UN_* child flags | position among the node's CSR children << 4,
 *                    storage index (internal child) or -1
 */
enum { PLK_UN_OWN_D = 1, PLK_UN_FROM_REGS = 2 };                                              /* header flags */
enum { PLK_UN_LEAF_D = 1, PLK_UN_STORE_G = 2, PLK_UN_CONTINUE = 4, PLK_UN_PAIR = 8, PLK_UN_REBUILD = 16,
       PLK_UN_INL_OWN = 32, PLK_UN_INL_L0 = 64, PLK_UN_INL_L1 = 128, PLK_UN_INL = 224, PLK_UN_WORK = 7 | 224, PLK_UN_POS_SHIFT = 8 };   /* child flags;
   PLK_UN_INL_*: a pair child that is FINISHED INSIDE this visit (it gets no visit of its own and its G is neither stored nor
   handed on): the derivative of the edge into it (OWN) and of its first / second leaf edge (L0 / L1) are wanted;
   PLK_UN_PAIR: the child's message P_b L_b comes from pair table number `fifth field` (its two leaves' codes), L_b is not stored;
   the record's fourth int then still holds the storage index (the child's own visit needs its G);
   PLK_UN_REBUILD: L_b is not stored either: b has two children, each a leaf or a pair node, and L_b is the product of their
   two messages (tip-table row / pair-table row), listed in the rebuild table at 4 * storage index (plk_up_rebuild_table) */

struct PlkUpNodes {
    std::vector<int> rec;
    int nvisits = 0;
};

/* Nodes whose L vector the k = 4 node-visit passes rebuild from tables instead of moving it through HBM: two children,
 * each a leaf or a pair node, no data of its own, no rescaling at the node (with <= 6 edges below it, it never is one).
 * rebuild[b] = 1 for them; table[4 * node_int[b]] = {t0, n0, t1, n1}: t >= 0 the tip slot of leaf child n, t <= -2 the pair
 * table -2 - t of pair child n. */
static inline void plk_up_rebuild_table(int N, const int *ip, const int *ix, const char *node_has_data, const int *edge_tip,
                                        const int *node_int, const int *node_scale, const int *pair_of, int nint_nodes,
                                        std::vector<char> &rebuild, std::vector<int> &table)
{
    rebuild.assign(N, 0);
    table.assign(4 * (size_t)std::max(nint_nodes, 1), -1);
    std::vector<int> edge_into(N, -1);
    for (int a = 0; a < N; a++) for (int idx = ip[a]; idx < ip[a + 1]; idx++) edge_into[ix[idx]] = idx;
    for (int b = 0; b < N; b++) {
        const int e0 = ip[b];
        if (ip[b + 1] - e0 != 2 || edge_into[b] < 0 || node_has_data[b] || node_scale[b] >= 0 || pair_of[b] >= 0 || node_int[b] < 0) continue;
        int rec[4];
        bool ok = true;
        for (int j = 0; j < 2; j++) {
            const int ch = ix[e0 + j];
            if (edge_tip[e0 + j] >= 0) rec[2 * j] = edge_tip[e0 + j];
            else if (pair_of[ch] >= 0) rec[2 * j] = -2 - pair_of[ch];
            else ok = false;
            rec[2 * j + 1] = ch;
        }
        if (!ok) continue;
        rebuild[b] = 1;
        for (int q = 0; q < 4; q++) table[4 * (size_t)node_int[b] + q] = rec[q];
    }
}

/* pair_of: null, or N ints: index of the node's pair table (its message comes from the table, not from a stored L) or -1.
 * A pair child's flags carry PLK_UN_PAIR and its tip-slot field holds -2 - pair (tip slots are >= 0, -1 = internal).
 * rebuild: null, or N chars of plk_up_rebuild_table: such a child's flags carry PLK_UN_REBUILD. */
static inline void plk_up_nodes_build(int N, const int *ip, const int *ix, const int *preorder, const char *node_has_data,
                                      const int *edge_tip, const int *node_int, const int *node_scale, const int *edge_mask,
                                      PlkUpNodes &un, const int *pair_of = nullptr, const char *rebuild = nullptr,
                                      bool inline_pairs = false)
{
    un.rec.clear(); un.nvisits = 0;
    std::vector<int> edge_into(N, -1);
    for (int a = 0; a < N; a++) for (int idx = ip[a]; idx < ip[a + 1]; idx++) edge_into[ix[idx]] = idx;
    auto wanted = [&](int idx) { return !edge_mask || edge_mask[idx]; };
    /* below[a]: some edge strictly below a is wanted; sub[a]: below[a] or the edge into a */
    std::vector<char> below(N, 0), sub(N, 0);
    for (int u = N - 1; u >= 0; u--) {
        const int a = preorder[u];
        for (int idx = ip[a]; idx < ip[a + 1]; idx++) if (sub[ix[idx]]) below[a] = 1;
        sub[a] = below[a] || (edge_into[a] >= 0 && wanted(edge_into[a]));
    }
    std::vector<int> stack;
    const int root = preorder[0];
    if (ip[root + 1] > ip[root] && sub[root]) stack.push_back(root);
    int from_regs = -1;                   /* node whose G the previous visit left in registers */
    while (!stack.empty() || from_regs >= 0) {
        int a;
        if (from_regs >= 0) a = from_regs; else { a = stack.back(); stack.pop_back(); }
        const int start = ip[a], deg = ip[a + 1] - start, ea = edge_into[a];
        const int hfl = (ea >= 0 && wanted(ea) ? PLK_UN_OWN_D : 0) | (from_regs >= 0 || ea < 0 ? PLK_UN_FROM_REGS : 0);
        from_regs = -1;
        const int hdr[8] = {a, deg, node_int[a], node_scale[a], node_has_data[a] ? 1 : 0, start, ea, hfl};
        un.rec.insert(un.rec.end(), hdr, hdr + 8);
        /* inline_pairs: a pair child (two leaves, no data) is finished inside this visit: its G is used while it is in
         * registers, never stored, and the node gets no visit */
        auto inl = [&](int j) { return inline_pairs && deg <= 2 && pair_of && edge_tip[start + j] < 0 && pair_of[ix[start + j]] >= 0; };      /* (the kernel's path for more than two children has no inline form) */
        /* the child that continues in registers: the last internal child with work; its record goes last */
        int cont = -1;
        if (below[a]) for (int j = 0; j < deg; j++) if (edge_tip[start + j] < 0 && sub[ix[start + j]] && !inl(j)) cont = j;
        for (int pass = 0; pass < 2; pass++)
            for (int j = 0; j < deg; j++) {
                if ((j == cont) != (pass == 1)) continue;
                const int idx = start + j, b = ix[idx];
                const bool leaf = edge_tip[idx] >= 0;
                int fl = 0;
                if (below[a]) {
                    if (leaf) fl = wanted(idx) ? PLK_UN_LEAF_D : 0;
                    else if (inl(j)) fl = (wanted(idx) ? PLK_UN_INL_OWN : 0) | (wanted(ip[b]) ? PLK_UN_INL_L0 : 0) | (wanted(ip[b] + 1) ? PLK_UN_INL_L1 : 0);
                    else if (sub[b]) fl = j == cont ? PLK_UN_CONTINUE : PLK_UN_STORE_G;
                }
                const bool pr = !leaf && pair_of && pair_of[b] >= 0;
                const bool rbd = !leaf && !pr && rebuild && rebuild[b];
                const int cr[4] = {b, pr ? -2 - pair_of[b] : edge_tip[idx], fl | (pr ? PLK_UN_PAIR : 0) | (rbd ? PLK_UN_REBUILD : 0) | (j << PLK_UN_POS_SHIFT), leaf ? -1 : node_int[b]};
                un.rec.insert(un.rec.end(), cr, cr + 4);
            }
        un.nvisits++;
        /* stored children are visited later (depth first: the most recently stored first), the continued one next */
        for (int j = 0; j < deg; j++) if (j != cont && edge_tip[start + j] < 0 && below[a] && sub[ix[start + j]] && !inl(j)) stack.push_back(ix[start + j]);
        if (cont >= 0) from_regs = ix[start + cont];
    }
}

/* replays the kernel's walk: indices in range, every child position once, every G read after it was written (or
 * handed over in registers by the visit just before) */
static inline std::string plk_up_nodes_check(int N, int E, const int *ip, const int *ix, const PlkUpNodes &un, int nint_nodes, int ntips,
                                             int nscale_slots, int npairs = 0, const int *edge_tip = nullptr,
                                             const int *rebuild_table = nullptr, const int *pair_of = nullptr)
{
    std::vector<char> g_written(std::max(nint_nodes, 1), 0), visited(N, 0);
    size_t vp = 0;
    int handed = -1;                     /* node whose G is in registers */
    for (int v = 0; v < un.nvisits; v++) {
        if (vp + 8 > un.rec.size()) return "up nodes: record overrun";
        const int *h = &un.rec[vp];
        const int a = h[0], deg = h[1], ai = h[2], slot = h[3], e0 = h[5], ea = h[6], hfl = h[7];
        if (a < 0 || a >= N || deg < 1 || ai < 0 || ai >= nint_nodes || slot < -1 || slot >= nscale_slots) return plk_fmt("up nodes: bad header %ld", v);
        if (e0 != ip[a] || deg != ip[a + 1] - ip[a] || e0 + deg > E || ea < -1 || ea >= E || (ea >= 0 && ix[ea] != a)) return plk_fmt("up nodes: bad edge range in visit %ld", v);
        if (vp + 8 + 4 * (size_t)deg > un.rec.size()) return "up nodes: record overrun";
        if (visited[a]) return plk_fmt("up nodes: node %ld visited twice", a);
        visited[a] = 1;
        if (ea < 0) { if (v != 0 || !(hfl & PLK_UN_FROM_REGS) || handed >= 0) return "up nodes: the root's visit must be the first and take its vector from registers"; }
        else if (hfl & PLK_UN_FROM_REGS) { if (handed != a) return plk_fmt("up nodes: visit %ld expects a vector in registers that the previous visit did not leave", v); }
        else if (handed >= 0) return plk_fmt("up nodes: the vector left in registers before visit %ld is dropped", v);
        else if (!g_written[ai]) return plk_fmt("up nodes: vector of node %ld read before it is written", a);
        if (ea < 0 && (hfl & PLK_UN_OWN_D)) return "up nodes: the root has no edge";
        handed = -1;
        const int *ch = h + 8;
        std::vector<char> seen(deg, 0);
        for (int j = 0; j < deg; j++) {
            const int b = ch[4 * j], fl = ch[4 * j + 2] & ((1 << PLK_UN_POS_SHIFT) - 1), pos = ch[4 * j + 2] >> PLK_UN_POS_SHIFT, bi = ch[4 * j + 3];
            int t = ch[4 * j + 1];
            if (pos < 0 || pos >= deg || seen[pos]) return plk_fmt("up nodes: child positions of visit %ld", v);
            seen[pos] = 1;
            if (fl & PLK_UN_INL) {
                /* finished inside this visit: a pair child with nothing stored or handed on, never visited itself */
                if (!(fl & PLK_UN_PAIR) || (fl & (PLK_UN_STORE_G | PLK_UN_CONTINUE | PLK_UN_LEAF_D)) || b < 0 || b >= N) return plk_fmt("up nodes: flags of an inline pair child in visit %ld", v);
                if (visited[b]) return plk_fmt("up nodes: inline pair child %ld is also visited", b);
                visited[b] = 1;
            }
            if (fl & PLK_UN_PAIR) {
                /* the message of this child is a pair-table row: two leaf children, table index in range */
                const int pi = -2 - t;
                if (pi < 0 || pi >= npairs || b < 0 || b >= N || ip[b + 1] - ip[b] != 2) return plk_fmt("up nodes: bad pair child in visit %ld", v);
                if (edge_tip && (edge_tip[ip[b]] < 0 || edge_tip[ip[b] + 1] < 0)) return plk_fmt("up nodes: pair child with an internal child in visit %ld", v);
                t = -1;
            }
            if (fl & PLK_UN_REBUILD) {
                /* L of this child is rebuilt from its table entry: two children, each the leaf / pair node the entry names,
                 * tip slots and pair tables in range and the ones of those children */
                if ((fl & PLK_UN_PAIR) || t != -1 || !rebuild_table || !edge_tip || !pair_of || bi < 0 || bi >= nint_nodes || b < 0 || b >= N || ip[b + 1] - ip[b] != 2)
                    return plk_fmt("up nodes: bad rebuild child in visit %ld", v);
                const int *rt = rebuild_table + 4 * (size_t)bi;
                for (int q = 0; q < 2; q++) {
                    const int cn = ix[ip[b] + q], ct = edge_tip[ip[b] + q];
                    if (rt[2 * q + 1] != cn) return plk_fmt("up nodes: rebuild entry of visit %ld names the wrong child", v);
                    if (ct >= 0 ? rt[2 * q] != ct : (pair_of[cn] < 0 || pair_of[cn] >= npairs || rt[2 * q] != -2 - pair_of[cn]))
                        return plk_fmt("up nodes: rebuild entry of visit %ld names the wrong table", v);
                }
            }
            if (b != ix[e0 + pos] || t < -1 || t >= ntips) return plk_fmt("up nodes: bad child in visit %ld", v);
            if (t < 0 && (bi < 0 || bi >= nint_nodes)) return plk_fmt("up nodes: bad storage index in visit %ld", v);
            if (t >= 0 && (fl & (PLK_UN_STORE_G | PLK_UN_CONTINUE))) return plk_fmt("up nodes: a leaf gets a stored vector in visit %ld", v);
            if (t < 0 && (fl & PLK_UN_LEAF_D)) return plk_fmt("up nodes: leaf flag on an internal child in visit %ld", v);
            if ((fl & PLK_UN_CONTINUE) && (j != deg - 1 || (fl & PLK_UN_STORE_G))) return plk_fmt("up nodes: the continued child must be the last record of visit %ld", v);
            if (fl & PLK_UN_CONTINUE) handed = b;
            if (fl & PLK_UN_STORE_G) g_written[bi] = 1;
        }
        vp += 8 + 4 * (size_t)deg;
    }
    if (handed >= 0) return "up nodes: a vector is left in registers at the end";
    if (vp != un.rec.size()) return "up nodes: trailing records";
    return "";
}

static inline std::string plk_chain_check(int N, const PlkProgram &pg, const PlkChain &ch, int mode, int D, int nint_nodes,
                                          int nint_edges, int nscale_slots, int site_block, size_t lds_code_bytes)
{
    const int nops = (int)pg.ops.size(), ntips = (int)pg.tip_edge.size(), nobs = (int)pg.obs_nodes.size();
    if ((int)ch.ops.size() != nops + 1 || (ch.ops[nops].x & 0xff) != OP_END) return "down program: missing END";
    if (pg.slots_needed > D) return "down program: the tree needs a deeper stack";
    if ((size_t)nobs * site_block > lds_code_bytes) return "down program: staged code rows exceed the launch's LDS";
    std::vector<int> slot, rowv, opc;
    plk_obs_sequence(N, pg, slot, rowv, opc);
    long cur_slot = ch.first_slot, cur_row = ch.first_row;
    if (mode != 2 && !slot.empty() && (cur_slot != slot[0] || cur_row != rowv[0])) return "down program: first observation";
    if (mode != 2 && slot.empty() && ch.first_slot >= 0) return "down program: first observation without observations";
    size_t oi = 0;
    for (int pc = 0; pc < nops; pc++) {
        const plk_op4 o = ch.ops[pc];
        const int code = o.x & 0xff;
        if (code != (pg.ops[pc].x & 0xff)) return "down program: opcode mismatch";
        if (code == OP_TIP_SET || code == OP_TIP_MUL || code == OP_NODE_MUL) {
            if (mode == 3) {
                /* two-ahead chain: y = row of the observation after next (cyclic) */
                if (o.y < 0 || o.y >= nobs || o.y != rowv[(oi + 2) % rowv.size()]) return plk_fmt("down program: op %ld prefetches the wrong row", pc);
            } else
            if (o.y < 0 || o.y >= nobs || o.y != rowv[oi]) return plk_fmt("down program: op %ld names the wrong staged row", pc);
            if (code != OP_NODE_MUL && ((o.x >> 8) < 0 || (o.x >> 8) >= ntips)) return "down program: tip slot out of range";
            if (mode != 2) {
                const int wrap = (o.z >> 30) & 1, ns = o.z & 0x3fffffff;
                if (ns < 0 || ns > ntips || o.w < 0 || o.w >= nobs) return plk_fmt("down program: op %ld prefetches out of range", pc);
                if (cur_slot != slot[oi] || cur_row != rowv[oi]) return plk_fmt("down program: chain delivers the wrong observation at op %ld", pc);
                const size_t nx = oi + 1 < slot.size() ? oi + 1 : 0;
                if (wrap != (oi + 1 == slot.size()) || ns != slot[nx] || o.w != rowv[nx]) return plk_fmt("down program: chain link after op %ld", pc);
                cur_slot = ns; cur_row = o.w;
            }
            oi++;
        } else if (code == OP_MATVEC && mode == 0) {
            /* z = the next MATVEC's op index, cyclically */
            int nx = (int)pc;
            do { nx = nx + 1 < nops ? nx + 1 : 0; } while ((pg.ops[nx].x & 0xff) != OP_MATVEC);
            if (o.z != nx) return plk_fmt("down program: op %ld names the wrong next product", pc);
        } else if (code == OP_MATVEC && mode >= 1) {
            if (o.y != pg.op_edge[pc] || o.z < (mode >= 1 && nint_nodes > 0 ? -1 : 0) || o.z >= (nint_nodes > 0 ? nint_nodes : nops)) return plk_fmt("down program: op %ld stores to a bad node index", pc);
            if (mode == 2 && (o.w < 0 || o.w >= nint_edges)) return plk_fmt("down program: op %ld stores to a bad edge index", pc);
        } else if (code == OP_PUSH || code == OP_POPMUL) {
            if (o.y < 0 || o.y >= D) return "down program: stack slot out of range";
        } else if (code == OP_SCALE && mode >= 1 && nscale_slots > 0) {
            if (o.y < -1 || o.y >= nscale_slots) return "down program: rescaling slot out of range";
        }
    }
    if (oi != slot.size()) return "down program: observation count";
    if (mode == 3 && !rowv.empty() && ch.second_row != rowv[1 % rowv.size()]) return "down program: second row";
    return "";
}

#endif
