/*
 * tests/pairmulcheck_main.cpp -- CPU driver for the PAIR-PRODUCT op stream of the streamed k = 4 interpreter
 * (k_ll_fused4_v4s<768, true, true>; plk_v4p_derive_ops, plk_fused_v4p_build and plk_fused_check_v4p in phyly_amd/csrc/plk_program.h), built
 * with AddressSanitizer + UBSan by tests/test_k4_pairmul_host.py.
 *
 * Over the seeded random trees of tests/progcheck_main.cpp (same generator, same seed, same 6000 iterations, nchar 4, 5
 * and 16, the skip rules of tests/streamcheck_main.cpp) it builds the checked stream and, for every tree taken:
 *   - a program that needs 4 stack slots gives no pair-product stream (plk_fused_v4p_build leaves the words empty and
 *     plk_k4_choose does not ask for the form), so the folded stream is what runs;
 *   - a program within 3 slots gives one, and the replay check accepts it;
 *   - independently of that check: walked next to the checked stream, every op stands for the checked stream's op or ops
 *     (ADVANCE aside), a PAIR exactly where two adjacent look-ups are a (TIP_SET, TIP_MUL) or a (TIP_SET + PUSH d,
 *     TIP_SET + POPMUL d), observation n sits on parity n & 1, and the ADVANCEs carried are as many as the checked stream's;
 *   - an ADVANCE keeps a dispatch only in front of the two observation kinds
 *     that have no handler with an ADVANCE inside (TIP_SET alone, TIP_MUL without wait);
 *   - the replay check refuses: a flipped parity (the handler's twin on the other buffer, at an even and at an odd observation,
 *     refused for the buffer and nothing else), the two field groups of a PAIR swapped, another request's table in the last
 *     observation op that is no PAIR (refused for the table field), a dropped observation op (its requests with it), an ADVANCE moved to the neighbouring observation op, a REFILL of the other kind.
 * Every observation and PAIR handler of the table must occur somewhere in the sweep: the six PAIR handlers (both parities;
 * no ADVANCE, ADVANCE_0 / _1 before the first extraction of an even and between the two of an odd observation's PAIR), the
 * ten observation kinds on either buffer (TIP_SET + PUSH slot 0 on buffer 0 only: the program's first observation) and the
 * seven with an ADVANCE inside, both kinds; the ones that never occur are printed and fail the run.
 * Before the sweep the handler numbering of plk_program.h (plk_v4p_obs_slot, plk_v4p_pair_slot) is compared with the tables the
 * generator wrote into plk_fused4_v4p_asm.h.
 * With a file name as argument (the tree of BASELINE config 3 as tests/foldcheck_main.cpp reads it; nchar 5, C 4) it also
 * requires 20 PAIR ops in one category and prints "config3 <PAIR ops> <dispatches folded> <dispatches with pair products>".
 * Prints "ok <trees within 3 slots> <trees with 4 slots> <PAIR ops> <ADVANCEs left with a dispatch> <controls run: parity of an odd observation, table field, parity of an even observation, swap, drop, advance, refill>" and
 * exits 0, or the first failure and exits 1.
 */
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "plk_program.h"
#include "plk_fused4_v4p_asm.h"      /* macros only: the generator's numbering */

struct Tree { int N; std::vector<int> ip, ix, pre; };

/* as in progcheck_main.cpp */
static bool make_tree(int N, const std::vector<int> &ea, const std::vector<int> &eb, Tree &t)
{
    t.N = N; t.ip.assign(N + 1, 0); t.ix.assign(N > 1 ? N - 1 : 1, 0); t.pre.clear();
    std::vector<int> indeg(N, 0);
    for (int e = 0; e < N - 1; e++) { t.ip[ea[e] + 1]++; indeg[eb[e]]++; }
    for (int a = 0; a < N; a++) t.ip[a + 1] += t.ip[a];
    std::vector<int> fill(t.ip.begin(), t.ip.end() - 1);
    for (int e = 0; e < N - 1; e++) t.ix[fill[ea[e]]++] = eb[e];
    int root = -1;
    for (int a = 0; a < N; a++) if (!indeg[a]) { if (root >= 0) return false; root = a; }
    if (root < 0) return false;
    t.pre.push_back(root);
    for (size_t h = 0; h < t.pre.size(); h++)
        for (int idx = t.ip[t.pre[h]]; idx < t.ip[t.pre[h] + 1]; idx++) t.pre.push_back(t.ix[idx]);
    return (int)t.pre.size() == N;
}

static long g_taken3 = 0, g_taken4 = 0, g_pairs = 0, g_adv_left = 0, g_ctl[7] = {0, 0, 0, 0, 0, 0, 0};
static std::set<unsigned> g_seen;

static long dispatches(const unsigned *wd, size_t stride)
{
    for (size_t i = 0; i < stride / 2; i++) if (wd[2 * i] / PLK_V4_HANDLER_BYTES == OP_END) return (long)i + 1;
    return -1;
}

static PlkFusedV4P reblocked(const PlkFusedV4S &vs, const PlkFusedV4P &vp, const std::vector<std::vector<PlkV4SOp>> &ops)
{
    PlkFusedV4P m = vp;
    m.stride = plk_v4s_block_stride(ops[0].size());
    m.words.assign((size_t)vs.C * m.stride, 0u);
    for (int c = 0; c < vs.C; c++) plk_v4s_block_ops(ops[c], &m.words[(size_t)c * m.stride], m.stride);
    return m;
}

/* ADVANCE carried by an observation or PAIR op: 0 none, 1 + k (a PAIR: before the first extraction), 3 + k between */
static int carried(unsigned h) { return plk_v4p_decode(h).v; }
/* the same handler carrying v; PLK_V4P_NONE: the table has none */
static unsigned with_carried(unsigned h, int v)
{
    const PlkV4PHandler hd = plk_v4p_decode(h);
    return hd.kind == 1 ? plk_v4p_obs_slot(hd.j, v, hd.p) : plk_v4p_pair_slot(v, hd.p);
}

static std::string check_tree(const Tree &t, const std::vector<char> &has, int nchar, int C, long *config3)
{
    const int N = t.N;
    PlkProgram pg;
    plk_program_build(N, t.ip.data(), t.ix.data(), t.pre.data(), has.data(), pg);
    if (pg.slots_needed > 4 || pg.obs_nodes.empty()) return "";
    PlkFusedPT fp;
    plk_fused_pt_build(N, t.ip.data(), t.ix.data(), pg, nchar, 1 << 30, fp, true);
    const unsigned tip_base = 0;
    const size_t lds = plk_fused_v4s_lds_bytes(fp, nchar, C);
    if (lds > plk_pt_lds_limit(1024) || lds / 32 >= 65536 || fp.units >= 2048 || fp.row_node.size() >= 65536) return "";
    std::string bad = plk_fused_check_pt(N, t.ip.data(), t.ix.data(), pg, fp, nchar, 1, 0, true, false);
    if (!bad.empty()) return "32-bit program: " + bad;
    PlkFusedV4S vs;
    plk_fused_v4s_words(fp, nchar, C, tip_base, vs);
    bad = plk_fused_check_v4s(fp, vs, nchar, C, tip_base, lds);
    if (!bad.empty()) return bad;

    PlkFusedV4P vp;
    plk_fused_v4p_build(vs, vp);
    /* what the engine's plan is handed for this tree */
    {
        PlkK4Shape sh = {nchar, C, 1000, 256, 1, 1, 0, {0, 0, 0}};
        PlkFused fu; PlkFusedPT fpt; PlkFusedV4 fv4; PlkFusedV4S fv4s;
        const PlkK4Choice ch = plk_k4_choose(N, t.ip.data(), t.ix.data(), pg, sh, true, fu, fpt, fv4, fv4s);
        if (!ch.bad.empty()) return "plk_k4_choose: " + ch.bad;
        /* (a tree whose tip vectors do not fit the round-2 interpreters' LDS either is sent to another kernel family) */
        if (ch.variant == PLK_K4_V4S) {
            if ((ch.pair != 0) != (pg.slots_needed <= 3)) return "plk_k4_choose: the pair-product form and the stack slots";
            sh.pair_tables = 1 + 512;
            if (plk_k4_choose(N, t.ip.data(), t.ix.data(), pg, sh, true, fu, fpt, fv4, fv4s).pair) return "plk_k4_choose: + 512 still asks for the pair-product form";
        } else if (ch.pair) return "plk_k4_choose: the pair-product form without the streamed form";
    }
    if (pg.slots_needed > 3) {
        if (!vp.words.empty()) return "a 4-slot program got a pair-product stream";
        /* asked for pair products all the same, the engine's sequence runs the folded stream */
        PlkK4Stream st;
        st.fv4s = vs; st.held = true;
        plk_k4_stream_fold_pair(st, true, true);
        if (st.runs != PlkK4Stream::FOLDED || !st.note.empty() || !plk_fused_check_v4s_fold(vs, st.fold).empty()) return "the folded stream of a 4-slot program";
        g_taken4++;
        return "";
    }
    if (vp.words.empty()) {
        /* the one reason left: a table field beyond the 13 bits a PAIR has for it */
        for (unsigned y : vs.first_y) if (y >= 8192u) return "";
        for (size_t i = 0; i < vs.words.size(); i += 2) if (plk_word_is_obs(vs.words[i] / PLK_V4_HANDLER_BYTES) && (vs.words[i + 1] >> 16) >= 8192u) return "";
        return "no pair-product stream for a program within 3 slots";
    }
    bad = plk_fused_check_v4p(vs, vp);
    if (!bad.empty()) return bad;
    {
        /* and the engine's sequence runs exactly this stream */
        PlkK4Stream st;
        st.fv4s = vs; st.held = true;
        plk_k4_stream_fold_pair(st, true, true);
        if (st.runs != PlkK4Stream::PAIR || !st.note.empty() || st.pair.words != vp.words || st.stride() != vp.stride) return "the pair-product stream is not the one that runs";
    }
    g_taken3++;

    std::vector<std::vector<PlkV4SOp>> pops(C);
    for (int c = 0; c < C; c++) {
        std::vector<PlkV4SOp> src;
        if (!plk_v4s_stream_ops(&vp.words[(size_t)c * vp.stride], vp.stride, pops[c])) return "the pair-product stream has no END";
        if (!plk_v4s_stream_ops(&vs.words[(size_t)c * vs.stride], vs.stride, src)) return "the checked stream has no END";
        std::vector<PlkV4SOp> items;
        long nadv_src = 0, nadv = 0, npair = 0;
        for (const PlkV4SOp &op : src) { if (plk_v4s_is_advance(op.h)) nadv_src++; else items.push_back(op); }
        size_t wi = 0;
        int oi = 0;
        for (const PlkV4SOp &op : pops[c]) {
            const unsigned h = op.h;
            if (c == 0) g_seen.insert(h);
            const PlkV4PHandler hd = plk_v4p_decode(h);
            if (plk_v4s_is_advance(h)) {
                /* only in front of TIP_SET alone and TIP_MUL without wait, the two kinds without an ADVANCE inside */
                const size_t at = (size_t)(&op - pops[c].data());
                const PlkV4PHandler nx = at + 1 < pops[c].size() ? plk_v4p_decode(pops[c][at + 1].h) : PlkV4PHandler{0, -1, 0, 0};
                if (nx.kind != 1 || nx.v != 0 || (nx.p == 0 && nx.j != 0 && nx.j != 2 && nx.j != 7)) return "an ADVANCE keeps its own dispatch where a handler could carry it";
                nadv++; g_adv_left++;
                continue;
            }
            /* (the table has no handler of stack slot 3: its indices 11, 19, 27, 31 and 63 are observation handlers on buffer 1) */
            if (wi >= items.size()) return "more ops than the checked stream";
            if (hd.kind == 2) {
                if (wi + 1 >= items.size() || !plk_v4p_pairable(items[wi].h, items[wi + 1].h)) return "a PAIR where the checked stream has no pair of look-ups";
                if (hd.p != (oi & 1)) return "a PAIR on the wrong parity";
                nadv += carried(h) != 0; npair++; wi += 2; oi += 2;
            } else if (hd.kind == 1) {
                if (items[wi].h != plk_v4p_obs_handler(hd.j)) return "an observation op of another kind than the checked stream's";
                if (wi + 1 < items.size() && plk_v4p_pairable(items[wi].h, items[wi + 1].h)) return "two look-ups that pair were left as two ops";
                if (hd.p != (oi & 1)) return "an observation op on the wrong parity";
                nadv += carried(h) != 0; wi++; oi++;
            } else if (h >= PLK_V4S_FOLD_SCALE && h < PLK_V4S_FOLD_SCALE + 3) {
                if (wi + 1 >= items.size() || items[wi].h != h - PLK_V4S_FOLD_SCALE + 28 || items[wi + 1].h != OP_SCALE) return "a + SCALE variant where no SCALE follows";
                wi += 2;
            } else {
                if (items[wi].h != h) return "an op that is not the checked stream's";
                if (h >= 28 && h < 31 && wi + 1 < items.size() && items[wi + 1].h == OP_SCALE) return "a SCALE after MATVEC + POPMUL keeps its own dispatch";
                wi++;
            }
        }
        if (wi != items.size() || oi != vs.nobs) return "the pair-product stream does not cover the checked stream";
        if (nadv != nadv_src) return "the ADVANCEs carried are not the checked stream's in number";
        if (npair != vp.npair) return "the stream's PAIR count";
        if (c == 0) g_pairs += npair;
    }
    if (config3) {
        PlkFusedV4SFold fo;
        plk_fused_v4s_fold(vs, fo);
        config3[0] = vp.npair; config3[1] = dispatches(fo.words.data(), fo.stride); config3[2] = dispatches(vp.words.data(), vp.stride);
    }

    /* negative controls */
    {
        std::vector<std::vector<PlkV4SOp>> m = pops;
        size_t at = (size_t)-1;
        /* the same handler on the other buffer, for an even and for an odd observation: the first op of each parity whose twin
         * the table has (every PAIR and observation handler without ADVANCE but TIP_SET + PUSH slot 0); what must refuse it is
         * the parity or the buffer's content, not the op's kind or its chunk */
        for (int parity = 0; parity < 2; parity++) {
            m = pops; at = (size_t)-1;
            unsigned twin = PLK_V4P_NONE;
            for (size_t i = 0; i < m[C - 1].size() && at == (size_t)-1; i++) {
                const PlkV4PHandler hd = plk_v4p_decode(m[C - 1][i].h);
                if (!hd.kind || hd.p != parity || hd.v != 0) continue;
                twin = hd.kind == 1 ? plk_v4p_obs_slot(hd.j, 0, 1 - hd.p) : plk_v4p_pair_slot(0, 1 - hd.p);
                if (twin != PLK_V4P_NONE) at = i;
            }
            if (at == (size_t)-1) continue;
            const PlkV4PHandler was = plk_v4p_decode(m[C - 1][at].h), now = plk_v4p_decode(twin);
            if (now.kind != was.kind || now.j != was.j || now.v != was.v || now.p != 1 - was.p) return "negative control: the twin is not the same handler on the other buffer";
            m[C - 1][at].h = twin;
            const std::string why = plk_fused_check_v4p(vs, reblocked(vs, vp, m));
            if (why.empty()) return "negative control: flipped parity accepted";
            if (why.find("other buffer") == std::string::npos) return "negative control: flipped parity refused for another reason: " + why;
            g_ctl[parity ? 5 : 0]++;
        }
        /* the request of the last observation op that is no PAIR names the table of another such op's request */
        m = pops; at = (size_t)-1;
        for (size_t i = 0; i < m[0].size(); i++) if (plk_v4p_is_obs(m[0][i].h)) at = i;
        if (at != (size_t)-1) {
            size_t from = (size_t)-1;
            for (size_t i = 0; i < at; i++) if (plk_v4p_is_obs(m[0][i].h) && (m[0][i].hi >> 16) != (m[0][at].hi >> 16)) from = i;
            if (from != (size_t)-1) {
                m[0][at].hi = (m[0][at].hi & 0xffffu) | (m[0][from].hi & 0xffff0000u);
                const std::string why = plk_fused_check_v4p(vs, reblocked(vs, vp, m));
                if (why.empty()) return "negative control: wrong table field in an observation op accepted";
                if (why.find("table field") == std::string::npos) return "negative control: wrong table field refused for another reason: " + why;
                g_ctl[6]++;
            }
        }
        /* the last PAIR whose two requests differ */
        m = pops; at = (size_t)-1;
        for (size_t i = 0; i < m[0].size(); i++) {
            const unsigned hi = m[0][i].hi;
            if (plk_v4p_is_pair(m[0][i].h) && ((hi & 3u) != ((hi >> 3) & 3u) || ((hi >> 5) & 0x1fffu) != ((hi >> 18) & 0x1fffu))) at = i;
        }
        if (at != (size_t)-1) {
            const unsigned hi = m[0][at].hi;
            m[0][at].hi = ((hi >> 3) & 3u) | (hi & 3u) << 3 | ((hi >> 18) & 0x1fffu) << 5 | ((hi >> 5) & 0x1fffu) << 18;
            if (plk_fused_check_v4p(vs, reblocked(vs, vp, m)).empty()) return "negative control: swapped field pair accepted";
            g_ctl[1]++;
        }
        m = pops; at = (size_t)-1;
        for (size_t i = 0; i < m[0].size() && at == (size_t)-1; i++) if (plk_v4p_is_obs(m[0][i].h) || plk_v4p_is_pair(m[0][i].h)) at = i;
        for (int c = 0; c < C; c++) m[c].erase(m[c].begin() + (long)at);
        if (plk_fused_check_v4p(vs, reblocked(vs, vp, m)).empty()) return "negative control: dropped observation op accepted";
        g_ctl[2]++;
        /* an ADVANCE moved to the next observation op (the previous one where it rides in the last) */
        m = pops; at = (size_t)-1;
        std::vector<size_t> obs;
        for (size_t i = 0; i < m[0].size(); i++) if (plk_v4p_is_obs(m[0][i].h) || plk_v4p_is_pair(m[0][i].h)) obs.push_back(i);
        for (size_t q = 0; q < obs.size() && at == (size_t)-1; q++) if (carried(m[0][obs[q]].h)) at = q;
        if (at != (size_t)-1 && obs.size() > 1) {
            const size_t to = at + 1 < obs.size() ? at + 1 : at - 1;
            /* (onto whichever handler of that op's kind and parity carries one, of the same ADVANCE kind) */
            const int k = (carried(m[0][obs[at]].h) - 1) & 1;
            unsigned moved = with_carried(m[0][obs[to]].h, 1 + k);
            if (moved == PLK_V4P_NONE) moved = with_carried(m[0][obs[to]].h, 3 + k);
            if (!carried(m[0][obs[to]].h) && moved != PLK_V4P_NONE) {
                m[0][obs[at]].h = with_carried(m[0][obs[at]].h, 0);
                m[0][obs[to]].h = moved;
                if (plk_fused_check_v4p(vs, reblocked(vs, vp, m)).empty()) return "negative control: ADVANCE moved by one op accepted";
                g_ctl[3]++;
            }
        }
        PlkFusedV4P f2 = vp;
        f2.words[(size_t)(C - 1) * vp.stride + 2 * 7] ^= (unsigned)PLK_V4_HANDLER_BYTES;       /* REFILL_A <-> REFILL_B */
        if (plk_fused_check_v4p(vs, f2).empty()) return "negative control: REFILL of the wrong kind accepted";
        g_ctl[4]++;
    }
    return "";
}

static int config3(const char *path)
{
    FILE *f = fopen(path, "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    Tree t;
    bool ok = fscanf(f, "%d", &t.N) == 1 && t.N >= 2 && t.N < 100000;
    if (ok) {
        t.ip.resize(t.N + 1); t.ix.resize(t.N - 1); t.pre.resize(t.N);
        for (int &v : t.ip) ok = ok && fscanf(f, "%d", &v) == 1;
        for (int &v : t.ix) ok = ok && fscanf(f, "%d", &v) == 1 && v >= 0 && v < t.N;
        for (int &v : t.pre) ok = ok && fscanf(f, "%d", &v) == 1 && v >= 0 && v < t.N;
        ok = ok && t.ip[0] == 0 && t.ip[t.N] == t.N - 1;
        for (int a = 0; ok && a < t.N; a++) ok = t.ip[a + 1] >= t.ip[a];
    }
    fclose(f);
    if (!ok) { fprintf(stderr, "%s: not a tree file\n", path); return 2; }
    const long before = g_taken3;
    long c3[3] = {-1, -1, -1};
    const std::string bad = check_tree(t, std::vector<char>(t.N, 0), 5, 4, c3);
    if (!bad.empty() || g_taken3 == before) { fprintf(stderr, "config 3 tree: %s\n", bad.empty() ? "not taken by the pair-product form" : bad.c_str()); return 1; }
    if (c3[0] != 20) { fprintf(stderr, "config 3 tree: %ld PAIR ops in a category, 20 expected\n", c3[0]); return 1; }
    printf("config3 %ld %ld %ld\n", c3[0], c3[1], c3[2]);
    g_taken3 = before; g_pairs = 0; g_adv_left = 0;
    for (long &v : g_ctl) v = 0;
    g_seen.clear();
    return 0;
}

/* the numbering plk_program.h states by hand is the one the generator emitted the handler table with */
static const char *numbering()
{
    static const int even[] = PLK_V4P_GEN_OBS_EVEN, odd[] = PLK_V4P_GEN_OBS_ODD, folded[] = PLK_V4P_GEN_OBS_FOLDED;
    if (sizeof even / sizeof *even != 10 || sizeof odd / sizeof *odd != 10) return "ten observation kinds";
    int nf = 0;
    for (int j = 0; j < 10; j++) {
        if (plk_v4p_obs_slot(j, 0, 0) != (unsigned)even[j] || plk_v4p_obs_handler(j) != (unsigned)even[j]) return "observation handlers on buffer 0";
        if (plk_v4p_obs_slot(j, 0, 1) != (odd[j] < 0 ? PLK_V4P_NONE : (unsigned)odd[j])) return "observation handlers on buffer 1";
        int jj = -1;
        for (int q = 0; q < (int)(sizeof folded / sizeof *folded); q++) if (folded[q] == even[j]) jj = q;
        for (int k = 0; k < 2; k++) {
            if (plk_v4p_obs_slot(j, 1 + k, 0) != (jj < 0 ? PLK_V4P_NONE : (unsigned)(PLK_V4P_FOLD_ADV + 2 * jj + k))) return "observation handlers with an ADVANCE inside";
            if (plk_v4p_obs_slot(j, 1 + k, 1) != PLK_V4P_NONE) return "an ADVANCE inside a handler on buffer 1";
        }
        nf += jj >= 0;
    }
    if (nf != (int)(sizeof folded / sizeof *folded)) return "kinds with an ADVANCE inside";
    if (plk_v4p_pair_slot(0, 0) != PLK_V4P_PAIR_EVEN || plk_v4p_pair_slot(1, 0) != PLK_V4P_PAIR_EVEN + 1 || plk_v4p_pair_slot(2, 0) != PLK_V4P_PAIR_EVEN + 2 ||
        plk_v4p_pair_slot(0, 1) != PLK_V4P_PAIR_ODD || plk_v4p_pair_slot(3, 1) != PLK_V4P_PAIR_ODD + 1 || plk_v4p_pair_slot(4, 1) != PLK_V4P_PAIR_ODD + 2) return "PAIR handlers";
    /* no two handlers share a slot, none sits on a slot of the ops both tables have */
    std::set<unsigned> used = {OP_MATVEC, OP_SCALE, OP_END, 8, 9, 10, 16, 17, 18, 24, 25, 26, 28, 29, 30, PLK_V4_REFILL_A, PLK_V4_REFILL_B,
                               PLK_V4S_ADVANCE, PLK_V4S_ADVANCE + 1, PLK_V4S_FOLD_SCALE, PLK_V4S_FOLD_SCALE + 1, PLK_V4S_FOLD_SCALE + 2};
    for (int p = 0; p < 2; p++) {
        for (int v = 0; v < 5; v++) if (plk_v4p_pair_slot(v, p) != PLK_V4P_NONE && !used.insert(plk_v4p_pair_slot(v, p)).second) return "a slot used twice";
        for (int j = 0; j < 10; j++) for (int v = 0; v < 3; v++) if (plk_v4p_obs_slot(j, v, p) != PLK_V4P_NONE && !used.insert(plk_v4p_obs_slot(j, v, p)).second) return "a slot used twice";
    }
    for (unsigned h : used) if (h >= (unsigned)PLK_V4_HANDLER_SLOTS) return "a slot beyond the table";
    return nullptr;
}

int main(int argc, char **argv)
{
    if (const char *bad = numbering()) { fprintf(stderr, "handler numbering of plk_program.h against the generated header: %s\n", bad); return 1; }
    if (argc > 1) { const int rc = config3(argv[1]); if (rc) return rc; }
    std::mt19937_64 rng(20250355);
    auto rnd = [&](int n) { return (int)(rng() % (unsigned long long)n); };
    const int nchars[3] = {4, 5, 16}, Cs[2] = {1, 4};
    for (int iter = 0; iter < 6000; iter++) {
        const int shape = iter % 8;
        int N;
        if (shape == 7) N = 2 + rnd(3);
        else if (iter % 97 == 0) N = 500 + rnd(3000);
        else N = 2 + rnd(iter % 5 == 0 ? 300 : 40);
        std::vector<int> ea(N - 1), eb(N - 1), label(N);
        for (int i = 0; i < N; i++) label[i] = i;
        for (int i = N - 1; i > 0; i--) std::swap(label[i], label[rnd(i + 1)]);
        for (int i = 1; i < N; i++) {
            int parent;
            switch (shape) {
            case 0: parent = rnd(i); break;
            case 1: parent = i - 1; break;
            case 2: parent = (i - 1) / 2; break;
            case 3: parent = i % 2 ? i - 1 - (i > 1) : i - 2; if (parent < 0) parent = 0; break;
            case 4: parent = 0; break;
            case 5: parent = rnd(10) < 7 ? rnd(i) : std::max(0, i - 1 - rnd(std::min(i, 3))); break;
            case 6: parent = (i - 1) / 3; break;
            default: parent = rnd(i); break;
            }
            ea[i - 1] = label[parent]; eb[i - 1] = label[i];
        }
        for (int e = N - 2; e > 0; e--) { const int j = rnd(e + 1); std::swap(ea[e], ea[j]); std::swap(eb[e], eb[j]); }
        Tree t;
        if (!make_tree(N, ea, eb, t)) { fprintf(stderr, "generator produced a non-tree\n"); return 2; }
        std::vector<char> has(N, 0);
        const int pdata = iter % 3 == 0 ? 0 : (iter % 3 == 1 ? 30 : 100);
        for (int a = 0; a < N; a++) has[a] = t.ip[a + 1] > t.ip[a] && rnd(100) < pdata;
        (void)rnd(8);                         /* progcheck draws its nchar here: keep the tree sequence the same */
        const int nchar = nchars[(iter / 3) % 3], C = Cs[(iter / 9) % 2];
        const std::string bad = check_tree(t, has, nchar, C, nullptr);
        if (!bad.empty()) { fprintf(stderr, "iteration %d (shape %d, N = %d, nchar = %d, C = %d): %s\n", iter, shape, N, nchar, C, bad.c_str()); return 1; }
    }
    /* every handler the builder can emit occurred */
    int missing = 0;
    for (unsigned h = 0; h < (unsigned)PLK_V4_HANDLER_SLOTS; h++) {
        const PlkV4PHandler hd = plk_v4p_decode(h);
        if (hd.kind && !g_seen.count(h)) {
            fprintf(stderr, "%s handler %u (kind %d, ADVANCE %d, parity %d) never occurred\n", hd.kind == 2 ? "PAIR" : "observation", h, hd.j, hd.v, hd.p);
            missing++;
        }
    }
    if (missing) return 1;
    printf("ok %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld\n", g_taken3, g_taken4, g_pairs, g_adv_left, g_ctl[5], g_ctl[6], g_ctl[0], g_ctl[1], g_ctl[2], g_ctl[3], g_ctl[4]);
    return 0;
}
